"""The confidence-weighted FiLM aggregation's C ABI and Python surface, without a GPU: exports, validation
before any launch, zero sizes, the workspace query, and the wrappers' argument checks."""
import ctypes
import os
import re
import types

import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib
from conftest import ROOT

HIP_INVALID_VALUE = 1
DUMMY = ctypes.c_void_p(16)


def _fwd(lib, **kw):
    a = dict(dtype=0, x=None, xs=0, gb=None, w=None, ws=0, indptr=None, src=None, eid=None, goff=None, B=0, maxn=0,
             kind=0, Nt=0, E=0, C=0, P=0, flags=0, wagg=0, out=None, os=0, stream=None)
    a.update(kw)
    return lib.mrp_film_wmean_fwd(a["dtype"], a["x"], a["xs"], a["gb"], a["w"], a["ws"], a["indptr"], a["src"],
                                  a["eid"], a["goff"], a["B"], a["maxn"], a["kind"], a["Nt"], a["E"], a["C"], a["P"],
                                  a["flags"], a["wagg"], a["out"], a["os"], a["stream"])


def _bwd(lib, **kw):
    a = dict(dtype=0, g=None, gs=0, x=None, xs=0, gb=None, w=None, ws=0, indptr=None, src=None, eid=None, goff=None,
             B=0, maxn=0, kind=0, Nt=0, E=0, C=0, P=0, flags=0, wagg=0, dx=None, dxs=0, base=None, bs=0, dgb=None,
             dw=None, dws=0, work=None, wbytes=0, stream=None)
    a.update(kw)
    return lib.mrp_film_wmean_bwd(a["dtype"], a["g"], a["gs"], a["x"], a["xs"], a["gb"], a["w"], a["ws"],
                                  a["indptr"], a["src"], a["eid"], a["goff"], a["B"], a["maxn"], a["kind"], a["Nt"],
                                  a["E"], a["C"], a["P"], a["flags"], a["wagg"], a["dx"], a["dxs"], a["base"],
                                  a["bs"], a["dgb"], a["dw"], a["dws"], a["work"], a["wbytes"], a["stream"])


def test_exports_match_the_header_and_the_abi_is_22():
    text = open(os.path.join(ROOT, "include", "mrp_gnn.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*|void)\s+(mrp_\w+)\s*\(", text, re.M))
    assert {"mrp_film_wmean_fwd", "mrp_film_wmean_bwd", "mrp_film_wmean_workspace"} <= declared
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert re.search(r"MRP_WAGG_MEAN\s*=\s*0\b", text) and re.search(r"MRP_WAGG_SUM\s*=\s*1\b", text)
    assert (_lib.WAGG_MEAN, _lib.WAGG_SUM) == (0, 1)
    lib = m.load_library()
    for name in ("mrp_film_wmean_fwd", "mrp_film_wmean_bwd", "mrp_film_wmean_workspace"):
        assert hasattr(lib, name)
    assert lib.mrp_abi_version() == 22 == _lib.ABI_VERSION
    assert "film_wmean" not in _lib.MODES  # that table numbers the `mode` of mrp_film_mean_*


def test_forward_declines_before_launch():
    lib = m.load_library()
    ok = dict(B=1, maxn=2, Nt=2, goff=DUMMY, indptr=DUMMY, C=2, P=4, x=DUMMY, out=DUMMY, xs=8, os=8, w=DUMMY, ws=4)
    assert _fwd(lib) == 0  # empty batch: no-op
    assert _fwd(lib, kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16) == 0  # consistent, empty features: no-op
    assert _fwd(lib, **dict(ok, P=0, xs=0, os=0, ws=0)) == 0
    assert _fwd(lib, maxn=17, B=1, Nt=1, goff=DUMMY, indptr=DUMMY) == HIP_INVALID_VALUE  # > MRP_MAX_NODES
    for bad in (dict(dtype=3), dict(dtype=-1), dict(kind=2), dict(kind=7), dict(flags=1), dict(flags=3),
                dict(flags=0x101), dict(wagg=2), dict(wagg=-1), dict(C=-1), dict(P=-1), dict(B=-1), dict(Nt=-1),
                dict(E=-1), dict(maxn=-1)):
        assert _fwd(lib, **bad) == HIP_INVALID_VALUE, bad
    assert _fwd(lib, **dict(ok, xs=7)) == HIP_INVALID_VALUE  # node stride < C * P
    assert _fwd(lib, **dict(ok, os=7)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, ws=3)) == HIP_INVALID_VALUE  # w node stride < P
    assert _fwd(lib, **dict(ok, w=None)) == HIP_INVALID_VALUE  # NULL w with work to do
    assert _fwd(lib, **dict(ok, x=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, out=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, goff=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, indptr=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, E=2, src=DUMMY, eid=DUMMY, gb=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, E=2, src=None, eid=DUMMY, gb=DUMMY)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, Nt=3)) == HIP_INVALID_VALUE  # more nodes than num_graphs * max_nodes
    assert _fwd(lib, kind=1, B=2, maxn=4, Nt=8, E=23) == HIP_INVALID_VALUE  # COMPLETE, inconsistent counts
    assert _fwd(lib, kind=1, B=2, maxn=4, Nt=7, E=24) == HIP_INVALID_VALUE
    assert _fwd(lib, kind=_lib.graph_regular(2), B=1, maxn=4, Nt=4, E=7, goff=DUMMY, indptr=DUMMY) == \
        HIP_INVALID_VALUE


def test_backward_declines_before_launch():
    lib = m.load_library()
    ok = dict(B=1, maxn=2, Nt=2, goff=DUMMY, indptr=DUMMY, C=2, P=4, g=DUMMY, gs=8, x=DUMMY, xs=8, dx=DUMMY, dxs=8,
              w=DUMMY, ws=4)
    assert _bwd(lib) == 0  # nothing requested
    assert _bwd(lib, **dict(ok, dx=None)) == 0  # work, but no output wanted
    assert _bwd(lib, dx=DUMMY, dgb=DUMMY, dw=DUMMY) == 0  # empty work
    assert _bwd(lib, kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16, dx=DUMMY) == 0
    assert _bwd(lib, maxn=17, B=1, Nt=1, goff=DUMMY, indptr=DUMMY, dx=DUMMY) == HIP_INVALID_VALUE
    for bad in (dict(dtype=3), dict(kind=2), dict(flags=2), dict(flags=0x102), dict(wagg=2), dict(wagg=-1),
                dict(C=-1), dict(P=-1), dict(B=-1), dict(Nt=-1), dict(E=-1)):
        assert _bwd(lib, dx=DUMMY, **bad) == HIP_INVALID_VALUE, bad
    for key in ("gs", "xs", "dxs"):
        assert _bwd(lib, **dict(ok, **{key: 7})) == HIP_INVALID_VALUE, key  # node stride < C * P
    assert _bwd(lib, **dict(ok, ws=3)) == HIP_INVALID_VALUE
    assert _bwd(lib, **dict(ok, w=None)) == HIP_INVALID_VALUE
    assert _bwd(lib, **dict(ok, dx=None, dw=DUMMY, dws=3)) == HIP_INVALID_VALUE  # grad_w node stride < P
    assert _bwd(lib, **dict(ok, base=DUMMY, bs=7)) == HIP_INVALID_VALUE
    assert _bwd(lib, **dict(ok, g=None)) == HIP_INVALID_VALUE  # NULL pointers with work to do
    assert _bwd(lib, **dict(ok, x=None)) == HIP_INVALID_VALUE
    assert _bwd(lib, **dict(ok, E=2, src=DUMMY, eid=DUMMY, gb=None)) == HIP_INVALID_VALUE
    assert _bwd(lib, kind=1, B=2, maxn=4, Nt=8, E=23, dx=DUMMY) == HIP_INVALID_VALUE
    assert _bwd(lib, kind=1, B=2, maxn=4, Nt=7, E=24, dx=DUMMY) == HIP_INVALID_VALUE
    # more than 16 channels: grad_w needs the workspace
    wide = dict(ok, C=17, gs=68, xs=68, dxs=68, dx=None, dw=DUMMY, dws=4)
    need = lib.mrp_film_wmean_workspace(1, 2, 0, 2, 0, 17, 4)
    assert need == 2 * 2 * 4 * 4
    assert _bwd(lib, **dict(wide, work=None, wbytes=need)) == HIP_INVALID_VALUE
    assert _bwd(lib, **dict(wide, work=DUMMY, wbytes=need - 1)) == HIP_INVALID_VALUE


def test_workspace_sizes():
    lib = m.load_library()
    ws = lib.mrp_film_wmean_workspace
    assert ws(0, 0, 0, 0, 0, 0, 0) == 0
    assert ws(2, 8, 1, 16, 112, 16, 1024) == 0  # one channel block: grad_w is written directly
    assert ws(2, 8, 1, 16, 112, 17, 1024) == 2 * 16 * 1024 * 4
    assert ws(2, 8, 1, 16, 112, 256, 1024) == 16 * 16 * 1024 * 4
    assert ws(3, 16, _lib.graph_regular(4), 48, 192, 64, 64) == 4 * 48 * 64 * 4
    assert ws(1, 4, 0, 4, 0, 64, 0) == 0 and ws(1, 4, 0, 0, 0, 64, 8) == 0


def test_python_argument_checks_and_no_cpu_fallback():
    g = m.complete_graph(3)
    x = torch.randn(3, 2, 4, 4)
    gb = torch.rand(6, 2, 2)
    w = torch.rand(3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.film_wmean(x, gb, w, g.csr("cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.film_wmean_forward_into(x, gb, w, g.csr("cpu"), 0, torch.empty_like(x))
    with pytest.raises(ValueError, match="mean"):
        m.film_wmean(x, gb, w, g.csr("cpu"), mode="max")
    from mrp_gnn_amd.aggregate import _wmean_weights, _require_device
    import mrp_gnn_amd.aggregate as agg
    real = agg._require_device
    agg._require_device = lambda *ts: None  # the shape / dtype checks, reached without a device
    try:
        assert _wmean_weights(w, 3, 4, 4)[1] == 16
        assert _wmean_weights(w[:, None], 3, 4, 4)[0].shape == (3, 4, 4)
        wide = torch.rand(3, 3, 4, 4)
        assert _wmean_weights(wide[:, 1], 3, 4, 4)[1] == 48  # a strided view: one plane per node
        for bad in (w.double(), w[:, :, :3], torch.rand(3, 4, 8)[:, :, ::2], torch.rand(2, 4, 4)):
            with pytest.raises(ValueError):
                _wmean_weights(bad, 3, 4, 4)
    finally:
        agg._require_device = real
    assert _require_device is real


def test_gcn_confidence_option_without_a_gpu():
    C = 8
    ns = types.SimpleNamespace
    base = m.GCNStack(ns(feature_dim=C, gcn_layers=2, gcn_combine="cat_compress"))
    off = m.GCNStack(ns(feature_dim=C, gcn_layers=2, gcn_combine="cat_compress", gcn_confidence=False))
    on = m.GCNStack(ns(feature_dim=C, gcn_layers=2, gcn_combine="cat_compress", gcn_confidence=True))
    assert list(off.state_dict()) == list(base.state_dict())  # off: today's keys, in today's order
    assert set(on.state_dict()) - set(base.state_dict()) == {f"gcn{i}.confidence.{p}" for i in (1, 2)
                                                            for p in ("weight", "bias")}
    for combine in ("cat_compress", "cat", "residual", "initial_mix"):
        for mode in ("film_mean", "film_sum", "copy_mean"):
            m.GCNStack(ns(feature_dim=C, gcn_mode=mode, gcn_combine=combine, gcn_confidence=True,
                          gcn_layers=1 if combine == "cat" else 2))
    m.multi_view_dgl_model(ns(feature_dim=C, compress_gcn=True, multi_gcn=True, gcn_confidence=True))
    for bad in (dict(gcn_mode="film_max"), dict(gcn_mode="film_attn"), dict(gcn_message_dtype="fp8_e5m2"),
                dict(gcn_confidence_threshold=1.5)):
        with pytest.raises(ValueError):
            m.GCN(ns(feature_dim=C, gcn_confidence=True, **bad))
    # the map itself is plain torch: (N, 1, H, W) fp32 in (0, 1), hard-gated by the threshold
    torch.manual_seed(0)
    soft = m.GCN(ns(feature_dim=C, gcn_confidence=True))
    hard = m.GCN(ns(feature_dim=C, gcn_confidence=True, gcn_confidence_threshold=0.5))
    hard.load_state_dict(soft.state_dict())
    x = torch.randn(3, C, 4, 4)
    ws, wh = soft.confidence_map(x), hard.confidence_map(x.bfloat16())
    assert ws.shape == (3, 1, 4, 4) and ws.dtype == wh.dtype == torch.float32 and ws.is_contiguous()
    assert bool(((ws > 0) & (ws < 1)).all())
    assert bool((wh[wh != 0] >= 0.5).all()) and bool((wh == 0).any()) and bool((wh != 0).any())
    # CPU tensors: the weighted aggregation is device-only, as the other operators
    g = m.complete_graph(3)
    g.edata["pose"] = torch.randn(6, 9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        soft(g, x)
    plain = m.GCN(ns(feature_dim=C, gcn_mode="film_max"))
    with pytest.raises(ValueError, match="film_max"):
        plain(g, x, weights=torch.rand(3, 4, 4))
    with pytest.raises(ValueError, match="gcn_confidence"):
        plain.confidence_map(x)
