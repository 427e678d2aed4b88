"""The confidence-gated attention fusion's C ABI and Python surface, without a GPU: exports, validation before
any launch, zero sizes, the workspace query, and the model's option handling."""
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
NAMES = ("mrp_film_wattn_fwd", "mrp_film_wattn_bwd", "mrp_film_wattn_workspace")


def _fwd(lib, **kw):
    a = dict(dtype=0, x=None, xs=0, gb=None, w=None, ws=0, indptr=None, src=None, eid=None, goff=None, B=0, maxn=0,
             kind=0, Nt=0, E=0, C=0, P=0, flags=0, out=None, os=0, scale=1.0, attn=None, rate=None, work=None,
             wbytes=0, stream=None)
    a.update(kw)
    return lib.mrp_film_wattn_fwd(a["dtype"], a["x"], a["xs"], a["gb"], a["w"], a["ws"], a["indptr"], a["src"],
                                  a["eid"], a["goff"], a["B"], a["maxn"], a["kind"], a["Nt"], a["E"], a["C"], a["P"],
                                  a["flags"], a["out"], a["os"], a["scale"], a["attn"], a["rate"], a["work"],
                                  a["wbytes"], a["stream"])


def _bwd(lib, **kw):
    a = dict(dtype=0, g=None, gs=0, x=None, xs=0, gb=None, w=None, ws=0, indptr=None, src=None, eid=None, goff=None,
             B=0, maxn=0, kind=0, Nt=0, E=0, C=0, P=0, flags=0, dx=None, dxs=0, base=None, bs=0, dgb=None, scale=1.0,
             attn=None, rate=None, dw=None, dws=0, work=None, wbytes=0, stream=None)
    a.update(kw)
    return lib.mrp_film_wattn_bwd(a["dtype"], a["g"], a["gs"], a["x"], a["xs"], a["gb"], a["w"], a["ws"],
                                  a["indptr"], a["src"], a["eid"], a["goff"], a["B"], a["maxn"], a["kind"], a["Nt"],
                                  a["E"], a["C"], a["P"], a["flags"], a["dx"], a["dxs"], a["base"], a["bs"], a["dgb"],
                                  a["scale"], a["attn"], a["rate"], a["dw"], a["dws"], a["work"], a["wbytes"],
                                  a["stream"])


def test_exports_match_the_header():
    text = open(os.path.join(ROOT, "include", "mrp_gnn.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*|void)\s+(mrp_\w+)\s*\(", text, re.M))
    assert set(NAMES) <= declared
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    lib = m.load_library()
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.mrp_abi_version() == 22 == _lib.ABI_VERSION
    # the signatures are film_attn's plus (w, w_node_stride), rate, and (rate, grad_w, gw_node_stride)
    assert len(lib.mrp_film_wattn_fwd.argtypes) == len(lib.mrp_film_attn_fwd.argtypes) + 3
    assert len(lib.mrp_film_wattn_bwd.argtypes) == len(lib.mrp_film_attn_bwd.argtypes) + 5
    for name in ("film_wattn", "film_wattn_cat", "film_wattn_residual", "film_wattn_mix", "film_wattn_forward_into",
                 "film_wattn_backward", "FilmWAttnFunction", "FilmWAttnCatFunction"):
        assert hasattr(m, name), name


def test_forward_declines_before_launch():
    lib = m.load_library()
    ok = dict(B=1, maxn=2, Nt=2, goff=DUMMY, indptr=DUMMY, C=2, P=4, x=DUMMY, out=DUMMY, xs=8, os=8, w=DUMMY, ws=4)
    assert _fwd(lib) == 0  # empty batch: no-op
    assert _fwd(lib, kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16) == 0  # consistent, empty features: no-op
    assert _fwd(lib, **dict(ok, P=0, xs=0, os=0, ws=0)) == 0
    assert _fwd(lib, maxn=17, B=1, Nt=1, goff=DUMMY, indptr=DUMMY) == HIP_INVALID_VALUE  # > MRP_MAX_NODES
    assert _fwd(lib, kind=_lib.graph_regular(17), B=1, maxn=16, Nt=16, E=16 * 17, goff=DUMMY, indptr=DUMMY,
                src=DUMMY, eid=DUMMY) == HIP_INVALID_VALUE  # REGULAR(17) > MRP_FILM_ATTN_DEGREE
    for bad in (dict(dtype=3), dict(dtype=-1), dict(kind=2), dict(kind=7), dict(flags=1), dict(flags=3),
                dict(flags=0x101), dict(C=-1), dict(P=-1), dict(B=-1), dict(Nt=-1), dict(E=-1), dict(maxn=-1),
                dict(scale=float("nan")), dict(scale=float("inf")), dict(wbytes=-1)):
        assert _fwd(lib, **bad) == HIP_INVALID_VALUE, bad
    assert _fwd(lib, **dict(ok, xs=7)) == HIP_INVALID_VALUE  # node stride < C * P
    assert _fwd(lib, **dict(ok, os=7)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, ws=3)) == HIP_INVALID_VALUE  # w node stride < P
    assert _fwd(lib, **dict(ok, w=None)) == HIP_INVALID_VALUE  # NULL w with work to do
    assert _fwd(lib, **dict(ok, x=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, out=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, goff=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, indptr=None)) == HIP_INVALID_VALUE
    edges = dict(ok, E=2, src=DUMMY, eid=DUMMY, gb=DUMMY, attn=DUMMY)
    assert _fwd(lib, **dict(edges, gb=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(edges, attn=None)) == HIP_INVALID_VALUE  # NULL attn where there are edges
    assert _fwd(lib, **dict(edges, src=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, Nt=3)) == HIP_INVALID_VALUE  # more nodes than num_graphs * max_nodes
    assert _fwd(lib, kind=1, B=2, maxn=4, Nt=8, E=23) == HIP_INVALID_VALUE  # COMPLETE, inconsistent counts
    assert _fwd(lib, kind=1, B=2, maxn=4, Nt=7, E=24) == HIP_INVALID_VALUE


def test_backward_declines_before_launch():
    lib = m.load_library()
    ok = dict(B=1, maxn=2, Nt=2, goff=DUMMY, indptr=DUMMY, C=2, P=4, g=DUMMY, gs=8, x=DUMMY, xs=8, dx=DUMMY, dxs=8,
              w=DUMMY, ws=4)
    assert _bwd(lib) == 0  # nothing requested
    assert _bwd(lib, **dict(ok, dx=None)) == 0  # work, but no output wanted: success without a launch
    assert _bwd(lib, kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16, dx=DUMMY) == 0  # empty work
    assert _bwd(lib, maxn=17, B=1, Nt=1, goff=DUMMY, indptr=DUMMY, dx=DUMMY) == HIP_INVALID_VALUE
    assert _bwd(lib, kind=_lib.graph_regular(17), B=1, maxn=16, Nt=16, E=16 * 17, goff=DUMMY, indptr=DUMMY,
                src=DUMMY, eid=DUMMY, dx=DUMMY) == HIP_INVALID_VALUE
    for bad in (dict(dtype=3), dict(kind=2), dict(flags=2), dict(flags=0x102), dict(C=-1), dict(P=-1), dict(B=-1),
                dict(Nt=-1), dict(E=-1), dict(scale=float("nan")), dict(wbytes=-1)):
        assert _bwd(lib, dx=DUMMY, **bad) == HIP_INVALID_VALUE, bad
    for key in ("gs", "xs", "dxs"):
        assert _bwd(lib, **dict(ok, **{key: 7})) == HIP_INVALID_VALUE, key  # node stride < C * P
    assert _bwd(lib, **dict(ok, ws=3)) == HIP_INVALID_VALUE  # w node stride < P
    assert _bwd(lib, **dict(ok, w=None)) == HIP_INVALID_VALUE  # NULL w with work to do
    assert _bwd(lib, **dict(ok, dx=None, dw=DUMMY, dws=3)) == HIP_INVALID_VALUE  # grad_w node stride < P
    assert _bwd(lib, **dict(ok, base=DUMMY, bs=7)) == HIP_INVALID_VALUE
    assert _bwd(lib, **dict(ok, g=None)) == HIP_INVALID_VALUE  # NULL pointers with work to do
    assert _bwd(lib, **dict(ok, x=None)) == HIP_INVALID_VALUE
    edges = dict(ok, E=2, src=DUMMY, eid=DUMMY, gb=DUMMY, attn=DUMMY, rate=DUMMY)
    assert _bwd(lib, **dict(edges, gb=None)) == HIP_INVALID_VALUE
    assert _bwd(lib, **dict(edges, attn=None)) == HIP_INVALID_VALUE
    assert _bwd(lib, **dict(edges, dx=None, dw=DUMMY, dws=4, rate=None)) == HIP_INVALID_VALUE  # grad_w needs rate
    assert _bwd(lib, kind=1, B=2, maxn=4, Nt=8, E=23, dx=DUMMY) == HIP_INVALID_VALUE
    assert _bwd(lib, kind=1, B=2, maxn=4, Nt=7, E=24, dx=DUMMY) == HIP_INVALID_VALUE
    # a plane over several tiles: grad_gb needs the workspace
    wide = dict(edges, P=65, gs=130, xs=130, dxs=130, ws=65, dx=None, dgb=DUMMY)
    need = lib.mrp_film_wattn_workspace(1, 1, 2, 0, 2, 2, 2, 65)
    assert need == 2 * 2 * 2 * 2 * 4
    assert _bwd(lib, **dict(wide, work=None, wbytes=need)) == HIP_INVALID_VALUE
    assert _bwd(lib, **dict(wide, work=DUMMY, wbytes=need - 1)) == HIP_INVALID_VALUE


def test_workspace_sizes():
    lib = m.load_library()
    ws, ref = lib.mrp_film_wattn_workspace, lib.mrp_film_attn_workspace
    assert ws(0, 0, 0, 0, 0, 0, 0, 0) == 0 and ws(1, 0, 0, 0, 0, 0, 0, 0) == 0
    assert ws(0, 2, 8, 1, 16, 112, 16, 1024) == 0  # the forward needs none
    assert ws(1, 2, 8, 1, 16, 112, 16, 64) == 0  # one tile: grad_gb is written directly; grad_w never needs any
    assert ws(1, 2, 8, 1, 16, 112, 16, 65) == 2 * 112 * 16 * 2 * 4
    assert ws(1, 2, 8, 1, 16, 112, 16, 1024) == 16 * 112 * 16 * 2 * 4
    for args in ((1, 3, 16, _lib.graph_regular(4), 48, 192, 64, 100), (1, 1, 4, 0, 4, 0, 64, 512),
                 (1, 1, 4, 0, 4, 9, 0, 512), (0, 1, 4, 0, 4, 9, 7, 512)):
        assert ws(*args) == ref(*args), args


def test_python_argument_checks_and_no_cpu_fallback():
    g = m.complete_graph(3)
    x = torch.randn(3, 2, 4, 4)
    gb = torch.rand(6, 2, 2)
    w = torch.rand(3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.film_wattn(x, gb, w, g.csr("cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.film_wattn_forward_into(x, gb, w, g.csr("cpu"), 0, torch.empty_like(x))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.film_wattn_cat(x, gb, w, g.csr("cpu"))
    unknown = g.csr("cpu")._replace(max_in_degree=-1)
    with pytest.raises(ValueError, match="in-degree"):
        m.film_wattn(x, gb, w, unknown)


def test_gcn_mode_option_without_a_gpu():
    C = 8
    ns = types.SimpleNamespace
    base = m.GCNStack(ns(feature_dim=C, gcn_layers=2, gcn_combine="cat_compress"))
    plain = m.GCNStack(ns(feature_dim=C, gcn_layers=2, gcn_combine="cat_compress", gcn_mode="film_wattn"))
    on = m.GCNStack(ns(feature_dim=C, gcn_layers=2, gcn_combine="cat_compress", gcn_mode="film_wattn",
                       gcn_confidence=True))
    assert list(plain.state_dict()) == list(base.state_dict())  # option off: no parameter, no key
    assert set(on.state_dict()) - set(base.state_dict()) == {f"gcn{i}.confidence.{p}" for i in (1, 2)
                                                            for p in ("weight", "bias")}
    for combine in ("cat_compress", "cat", "residual", "initial_mix"):
        for conf in (False, True):
            m.GCNStack(ns(feature_dim=C, gcn_mode="film_wattn", gcn_combine=combine, gcn_confidence=conf,
                          gcn_confidence_threshold=0.5, gcn_attn_scale=0.3, gcn_layers=1 if combine == "cat" else 2))
    m.GCNBlock(ns(feature_dim=C, compress_gcn=True, multi_gcn=True, gcn_mode="film_wattn", gcn_confidence=True))
    m.multi_view_dgl_model(ns(feature_dim=C, compress_gcn=True, multi_gcn=True, gcn_mode="film_wattn",
                              gcn_confidence=True))
    # FP8 messages: not provided for this reducer, with or without the head
    for conf in (False, True):
        with pytest.raises(ValueError, match="gcn_message_dtype"):
            m.GCN(ns(feature_dim=C, gcn_mode="film_wattn", gcn_message_dtype="fp8_e4m3", gcn_confidence=conf))
    # the refusals that were there stay
    for bad in (dict(gcn_mode="film_max"), dict(gcn_mode="film_attn")):
        with pytest.raises(ValueError, match="confidence-weighted"):
            m.GCN(ns(feature_dim=C, gcn_confidence=True, **bad))
    g = m.complete_graph(3)
    g.edata["pose"] = torch.randn(6, 9)
    x = torch.randn(3, C, 4, 4)
    for mode in ("film_max", "film_attn"):
        with pytest.raises(ValueError, match=mode):
            m.GCN(ns(feature_dim=C, gcn_mode=mode))(g, x, weights=torch.rand(3, 4, 4))
    # CPU tensors: device-only, with explicit maps, with the head and with neither (film_attn's route)
    for net, kw in ((m.GCN(ns(feature_dim=C, gcn_mode="film_wattn")), dict(weights=torch.rand(3, 4, 4))),
                    (m.GCN(ns(feature_dim=C, gcn_mode="film_wattn", gcn_confidence=True)), {}),
                    (m.GCN(ns(feature_dim=C, gcn_mode="film_wattn")), {})):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            net(g, x, **kw)
