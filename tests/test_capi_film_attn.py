"""The attention-pooled FiLM aggregation's C ABI and Python surface, without a GPU launch: exports, validation
before any launch, the workspace query, the in-degree limit."""
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
    a = dict(dtype=0, x=None, xs=0, gb=None, indptr=None, src=None, eid=None, goff=None, B=0, maxn=0, kind=0, Nt=0,
             E=0, C=0, P=0, flags=0, out=None, os=0, scale=1.0, attn=None, ws=None, wsb=0, stream=None)
    a.update(kw)
    return lib.mrp_film_attn_fwd(a["dtype"], a["x"], a["xs"], a["gb"], a["indptr"], a["src"], a["eid"], a["goff"],
                                 a["B"], a["maxn"], a["kind"], a["Nt"], a["E"], a["C"], a["P"], a["flags"], a["out"],
                                 a["os"], a["scale"], a["attn"], a["ws"], a["wsb"], a["stream"])


def _bwd(lib, **kw):
    a = dict(dtype=0, g=None, gs=0, x=None, xs=0, gb=None, indptr=None, src=None, eid=None, goff=None, B=0, maxn=0,
             kind=0, Nt=0, E=0, C=0, P=0, flags=0, dx=None, dxs=0, base=None, bs=0, dgb=None, scale=1.0, attn=None,
             ws=None, wsb=0, stream=None)
    a.update(kw)
    return lib.mrp_film_attn_bwd(a["dtype"], a["g"], a["gs"], a["x"], a["xs"], a["gb"], a["indptr"], a["src"],
                                 a["eid"], a["goff"], a["B"], a["maxn"], a["kind"], a["Nt"], a["E"], a["C"], a["P"],
                                 a["flags"], a["dx"], a["dxs"], a["base"], a["bs"], a["dgb"], a["scale"], a["attn"],
                                 a["ws"], a["wsb"], a["stream"])


def test_exports_match_the_header_and_the_abi_is_22():
    text = open(os.path.join(ROOT, "include", "mrp_gnn.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*|void)\s+(mrp_\w+)\s*\(", text, re.M))
    assert {"mrp_film_attn_fwd", "mrp_film_attn_bwd", "mrp_film_attn_workspace"} <= declared
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert re.search(r"#define\s+MRP_FILM_ATTN_DEGREE\s+16\b", text)
    assert _lib.FILM_ATTN_DEGREE == 16
    lib = m.load_library()
    for name in ("mrp_film_attn_fwd", "mrp_film_attn_bwd", "mrp_film_attn_workspace"):
        assert hasattr(lib, name)
    assert lib.mrp_abi_version() == 22 == _lib.ABI_VERSION
    assert "film_attn" not in _lib.MODES  # that table numbers the `mode` of mrp_film_mean_*


def test_forward_declines_before_launch():
    lib = m.load_library()
    ok = dict(B=1, maxn=2, Nt=2, goff=DUMMY, indptr=DUMMY, C=2, P=4, x=DUMMY, out=DUMMY, xs=8, os=8)
    assert _fwd(lib) == 0  # empty batch: no-op
    assert _fwd(lib, kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16) == 0  # consistent, empty features: no-op
    assert _fwd(lib, maxn=17, B=1, Nt=1, goff=DUMMY, indptr=DUMMY) == HIP_INVALID_VALUE  # > MRP_MAX_NODES
    for bad in (dict(dtype=3), dict(dtype=-1), dict(kind=2), dict(kind=7), dict(flags=1), dict(flags=3),
                dict(flags=0x101), dict(C=-1), dict(P=-1), dict(B=-1), dict(Nt=-1), dict(E=-1), dict(maxn=-1),
                dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=float("-inf")), dict(wsb=-1)):
        assert _fwd(lib, **bad) == HIP_INVALID_VALUE, bad
    assert _fwd(lib, **dict(ok, xs=7)) == HIP_INVALID_VALUE  # node stride < C * P
    assert _fwd(lib, **dict(ok, os=7)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, x=None)) == HIP_INVALID_VALUE  # NULL pointers with work to do
    assert _fwd(lib, **dict(ok, out=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, goff=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, indptr=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, E=2, src=DUMMY, eid=DUMMY, gb=None, attn=DUMMY)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, E=2, src=DUMMY, eid=DUMMY, gb=DUMMY, attn=None)) == HIP_INVALID_VALUE  # NULL attn
    assert _fwd(lib, **dict(ok, E=2, src=None, eid=DUMMY, gb=DUMMY, attn=DUMMY)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, Nt=3)) == HIP_INVALID_VALUE  # more nodes than num_graphs * max_nodes
    # COMPLETE with inconsistent node / edge counts
    assert _fwd(lib, kind=1, B=2, maxn=4, Nt=8, E=23) == HIP_INVALID_VALUE
    assert _fwd(lib, kind=1, B=2, maxn=4, Nt=7, E=24) == HIP_INVALID_VALUE
    # REGULAR(k): k * num_nodes edges, and k within the operator's in-degree limit
    assert _fwd(lib, kind=_lib.graph_regular(2), B=1, maxn=4, Nt=4, E=7, goff=DUMMY, indptr=DUMMY) == \
        HIP_INVALID_VALUE
    assert _fwd(lib, kind=_lib.graph_regular(17), B=1, maxn=16, Nt=16, E=17 * 16, goff=DUMMY, indptr=DUMMY,
                src=DUMMY, eid=DUMMY) == HIP_INVALID_VALUE


def test_backward_declines_before_launch():
    lib = m.load_library()
    ok = dict(B=1, maxn=2, Nt=2, goff=DUMMY, indptr=DUMMY, C=2, P=4, g=DUMMY, gs=8, x=DUMMY, xs=8, dx=DUMMY, dxs=8)
    assert _bwd(lib) == 0  # nothing requested
    assert _bwd(lib, **dict(ok, dx=None)) == 0  # work, but neither output wanted
    assert _bwd(lib, dx=DUMMY, dgb=DUMMY) == 0  # empty work
    assert _bwd(lib, kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16, dx=DUMMY) == 0
    assert _bwd(lib, maxn=17, B=1, Nt=1, goff=DUMMY, indptr=DUMMY, dx=DUMMY) == HIP_INVALID_VALUE
    for bad in (dict(dtype=3), dict(kind=2), dict(flags=2), dict(flags=0x102), dict(C=-1), dict(P=-1), dict(B=-1),
                dict(Nt=-1), dict(E=-1), dict(scale=float("nan")), dict(scale=float("inf")), dict(wsb=-1)):
        assert _bwd(lib, dx=DUMMY, **bad) == HIP_INVALID_VALUE, bad
    for key in ("gs", "xs", "dxs"):
        assert _bwd(lib, **dict(ok, **{key: 7})) == HIP_INVALID_VALUE, key  # node stride < C * P
    assert _bwd(lib, **dict(ok, base=DUMMY, bs=7)) == HIP_INVALID_VALUE
    assert _bwd(lib, **dict(ok, g=None)) == HIP_INVALID_VALUE  # NULL pointers with work to do
    assert _bwd(lib, **dict(ok, x=None)) == HIP_INVALID_VALUE
    assert _bwd(lib, **dict(ok, E=2, src=DUMMY, eid=DUMMY, gb=None, attn=DUMMY)) == HIP_INVALID_VALUE
    assert _bwd(lib, **dict(ok, E=2, src=DUMMY, eid=DUMMY, gb=DUMMY, attn=None)) == HIP_INVALID_VALUE  # NULL attn
    assert _bwd(lib, kind=1, B=2, maxn=4, Nt=8, E=23, dx=DUMMY) == HIP_INVALID_VALUE
    assert _bwd(lib, kind=1, B=2, maxn=4, Nt=7, E=24, dx=DUMMY) == HIP_INVALID_VALUE
    assert _bwd(lib, kind=_lib.graph_regular(17), B=1, maxn=16, Nt=16, E=17 * 16, goff=DUMMY, indptr=DUMMY,
                src=DUMMY, eid=DUMMY, dx=DUMMY) == HIP_INVALID_VALUE
    # grad_gb of a plane that spans several tiles needs the queried workspace
    big = dict(kind=1, B=1, maxn=2, Nt=2, E=2, C=2, P=256, g=DUMMY, gs=512, x=DUMMY, xs=512, gb=DUMMY, attn=DUMMY,
               dgb=DUMMY)
    need = lib.mrp_film_attn_workspace(1, 1, 2, 1, 2, 2, 2, 256)
    assert need > 0
    assert _bwd(lib, **big) == HIP_INVALID_VALUE  # no workspace
    assert _bwd(lib, **dict(big, ws=DUMMY, wsb=need - 1)) == HIP_INVALID_VALUE  # smaller than the query
    assert _bwd(lib, **dict(big, ws=None, wsb=need)) == HIP_INVALID_VALUE


def test_workspace_query():
    lib = m.load_library()
    q = lib.mrp_film_attn_workspace
    assert q(0, 2, 8, 1, 16, 112, 64, 1024) == 0  # the forward needs none
    assert q(1, 0, 0, 0, 0, 0, 0, 0) == 0
    assert q(1, 2, 8, 1, 16, 112, 64, 0) == 0 and q(1, 2, 8, 1, 16, 0, 64, 1024) == 0
    prev = 0
    for P in (1, 16, 49, 64, 65, 128, 129, 256, 1024, 4096):
        for direction in (0, 1):
            assert q(direction, 2, 8, 1, 16, 112, 64, P) >= 0
        cur = q(1, 2, 8, 1, 16, 112, 64, P)
        assert cur >= prev  # monotone in P
        prev = cur
    assert q(1, 2, 8, 1, 16, 112, 64, 64) == 0  # one tile: grad_gb is written directly
    assert q(1, 2, 8, 1, 16, 112, 64, 1024) == 16 * 112 * 64 * 2 * 4  # one partial per tile


def test_no_cpu_fallback():
    g = m.complete_graph(3)
    x = torch.randn(3, 2, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.film_attn(x, torch.rand(6, 2, 2), g.csr("cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.film_attn_forward_into(x, torch.rand(6, 2, 2), g.csr("cpu"), 0, torch.empty_like(x))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.film_attn_backward(x, x, torch.rand(6, 2, 2), torch.rand(6, 16), g.csr("cpu"), 0, True, True)


def test_in_degree_bound_is_checked_before_the_device():
    s, d = m.complete_edges(16)
    s, d = s + list(range(16)), d + list(range(16))
    at_limit = m.RobotGraph(s, d, num_nodes=16).csr("cpu")
    over = m.RobotGraph(s + [3], d + [5], num_nodes=16).csr("cpu")
    assert at_limit.max_in_degree == 16 and over.max_in_degree == 17
    x = torch.randn(16, 2, 4, 4)
    with pytest.raises(ValueError, match="16"):
        m.film_attn(x, torch.rand(over.num_edges, 2, 2), over)
    with pytest.raises(ValueError, match="16"):
        m.film_attn_cat(x, torch.rand(over.num_edges, 2, 2), over)
    with pytest.raises(ValueError, match="16"):
        m.film_attn_backward(x, x, torch.rand(over.num_edges, 2, 2), torch.rand(over.num_edges, 16), over, 0,
                             True, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # at the limit the graph is accepted
        m.film_attn(x, torch.rand(at_limit.num_edges, 2, 2), at_limit)
    unknown = at_limit._replace(max_in_degree=-1)
    with pytest.raises(ValueError, match="16"):
        m.film_attn(x, torch.rand(unknown.num_edges, 2, 2), unknown)


def test_python_argument_checks():
    g = m.complete_graph(3).csr("cpu")
    x = torch.randn(3, 2, 4, 4)
    from mrp_gnn_amd import aggregate, compress
    with pytest.raises(ValueError, match="finite"):
        aggregate._attn_scale(float("nan"), 4)
    assert aggregate._attn_scale(None, 4) == 0.5 and aggregate._attn_scale(0, 4) == 0.0
    with pytest.raises(ValueError, match="flags"):
        aggregate._check_attn_flags(1)
    conv = torch.nn.Conv2d(4, 2, 1)
    with pytest.raises(ValueError, match="reducer"):
        compress.film_compress(conv, x, torch.rand(6, 2, 2), g, 0, reducer="median")
    with pytest.raises(ValueError, match="GB_LOGITS"):
        compress.film_compress(conv, x, torch.rand(6, 2, 2), g, 2, reducer="attn")
    with pytest.raises(ValueError, match="scale"):
        compress.film_compress(conv, x, torch.rand(6, 2, 2), g, 0, reducer="max", scale=1.0)


def test_gcn_with_film_attn_constructs():
    opt = types.SimpleNamespace(feature_dim=8, gcn_mode="film_attn", gcn_attn_scale=0.5)
    gcn = m.GCN(opt)
    assert gcn.opt.gcn_mode == "film_attn" and gcn._attn_scale() == 0.5
    assert m.GCN(types.SimpleNamespace(feature_dim=8, gcn_mode="film_attn"))._attn_scale() is None
    for combine in ("cat_compress", "cat", "residual", "initial_mix"):
        m.GCNStack(types.SimpleNamespace(feature_dim=8, gcn_mode="film_attn", gcn_combine=combine,
                                         gcn_layers=1 if combine == "cat" else 2))
