"""The max-pooled FiLM aggregation's C ABI and Python surface, without a GPU: exports, validation before
any launch, the in-degree limit, and the separation from the mean entry points' modes."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib
from conftest import ROOT

HIP_INVALID_VALUE = 1
DUMMY = ctypes.c_void_p(16)


def _fwd(lib, **kw):
    a = dict(dtype=0, x=None, xs=0, gb=None, indptr=None, src=None, eid=None, goff=None, B=0, maxn=0, kind=0, Nt=0,
             E=0, C=0, P=0, flags=0, out=None, os=0, stream=None)
    a.update(kw)
    return lib.mrp_film_max_fwd(a["dtype"], a["x"], a["xs"], a["gb"], a["indptr"], a["src"], a["eid"], a["goff"],
                                a["B"], a["maxn"], a["kind"], a["Nt"], a["E"], a["C"], a["P"], a["flags"], a["out"],
                                a["os"], a["stream"])


def _bwd(lib, **kw):
    a = dict(dtype=0, g=None, gs=0, x=None, xs=0, gb=None, indptr=None, src=None, eid=None, goff=None, B=0, maxn=0,
             kind=0, Nt=0, E=0, C=0, P=0, flags=0, dx=None, dxs=0, base=None, bs=0, dgb=None, stream=None)
    a.update(kw)
    return lib.mrp_film_max_bwd(a["dtype"], a["g"], a["gs"], a["x"], a["xs"], a["gb"], a["indptr"], a["src"],
                                a["eid"], a["goff"], a["B"], a["maxn"], a["kind"], a["Nt"], a["E"], a["C"], a["P"],
                                a["flags"], a["dx"], a["dxs"], a["base"], a["bs"], a["dgb"], a["stream"])


def test_exports_match_the_header_and_the_abi_is_22():
    text = open(os.path.join(ROOT, "include", "mrp_gnn.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*|void)\s+(mrp_\w+)\s*\(", text, re.M))
    assert {"mrp_film_max_fwd", "mrp_film_max_bwd"} <= declared
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert re.search(r"#define\s+MRP_FILM_MAX_DEGREE\s+16\b", text)
    assert _lib.FILM_MAX_DEGREE == 16
    lib = m.load_library()
    assert hasattr(lib, "mrp_film_max_fwd") and hasattr(lib, "mrp_film_max_bwd")
    assert lib.mrp_abi_version() == 22 == _lib.ABI_VERSION
    assert "film_max" not in _lib.MODES  # that table numbers the `mode` of mrp_film_mean_*


def test_forward_declines_before_launch():
    lib = m.load_library()
    ok = dict(B=1, maxn=2, Nt=2, goff=DUMMY, indptr=DUMMY, C=2, P=4, x=DUMMY, out=DUMMY, xs=8, os=8)
    assert _fwd(lib) == 0  # empty batch: no-op
    assert _fwd(lib, kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16) == 0  # consistent, empty features: no-op
    assert _fwd(lib, maxn=17, B=1, Nt=1, goff=DUMMY, indptr=DUMMY) == HIP_INVALID_VALUE  # > MRP_MAX_NODES
    for bad in (dict(dtype=3), dict(dtype=-1), dict(kind=2), dict(kind=7), dict(flags=1), dict(flags=3),
                dict(flags=0x101), dict(C=-1), dict(P=-1), dict(B=-1), dict(Nt=-1), dict(E=-1), dict(maxn=-1)):
        assert _fwd(lib, **bad) == HIP_INVALID_VALUE, bad
    assert _fwd(lib, **dict(ok, xs=7)) == HIP_INVALID_VALUE  # node stride < C * P
    assert _fwd(lib, **dict(ok, os=7)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, x=None)) == HIP_INVALID_VALUE  # NULL pointers with work to do
    assert _fwd(lib, **dict(ok, out=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, goff=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, indptr=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, E=2, src=DUMMY, eid=DUMMY, gb=None)) == HIP_INVALID_VALUE
    assert _fwd(lib, **dict(ok, E=2, src=None, eid=DUMMY, gb=DUMMY)) == HIP_INVALID_VALUE
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
                dict(Nt=-1), dict(E=-1)):
        assert _bwd(lib, dx=DUMMY, **bad) == HIP_INVALID_VALUE, bad
    for key in ("gs", "xs", "dxs"):
        assert _bwd(lib, **dict(ok, **{key: 7})) == HIP_INVALID_VALUE, key  # node stride < C * P
    assert _bwd(lib, **dict(ok, base=DUMMY, bs=7)) == HIP_INVALID_VALUE
    assert _bwd(lib, **dict(ok, g=None)) == HIP_INVALID_VALUE  # NULL pointers with work to do
    assert _bwd(lib, **dict(ok, x=None)) == HIP_INVALID_VALUE
    assert _bwd(lib, **dict(ok, E=2, src=DUMMY, eid=DUMMY, gb=None)) == HIP_INVALID_VALUE
    assert _bwd(lib, kind=1, B=2, maxn=4, Nt=8, E=23, dx=DUMMY) == HIP_INVALID_VALUE
    assert _bwd(lib, kind=1, B=2, maxn=4, Nt=7, E=24, dx=DUMMY) == HIP_INVALID_VALUE


def test_mode_3_is_still_rejected_by_the_mean_entry_point():
    lib = m.load_library()
    assert lib.mrp_film_mean_fwd(None, 0, None, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 3, None, 0,
                                 None) == HIP_INVALID_VALUE
    with pytest.raises(KeyError):
        _lib.MODES["film_max"]


def test_no_cpu_fallback():
    g = m.complete_graph(3)
    x = torch.randn(3, 2, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.film_max(x, torch.rand(6, 2, 2), g.csr("cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.film_max_forward_into(x, torch.rand(6, 2, 2), g.csr("cpu"), 0, torch.empty_like(x))


def test_in_degree_bound_of_host_and_unknown_graphs():
    assert m.complete_graph(16).csr("cpu").max_in_degree == 15
    assert m.complete_graph(1).csr("cpu").max_in_degree == 0
    # 16-node complete + self-loops: in-degree 16, the limit; one parallel edge more: 17
    s, d = m.complete_edges(16)
    s, d = s + list(range(16)), d + list(range(16))
    at_limit = m.RobotGraph(s, d, num_nodes=16).csr("cpu")
    assert at_limit.max_in_degree == 16
    over = m.RobotGraph(s + [3], d + [5], num_nodes=16).csr("cpu")
    assert over.max_in_degree == 17
    x = torch.randn(16, 2, 4, 4)
    with pytest.raises(ValueError, match="16"):
        m.film_max(x, torch.rand(over.num_edges, 2, 2), over)
    with pytest.raises(ValueError, match="16"):
        m.film_max_backward(x, x, torch.rand(over.num_edges, 2, 2), over, 0, True, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # at the limit the graph is accepted
        m.film_max(x, torch.rand(at_limit.num_edges, 2, 2), at_limit)
    unknown = at_limit._replace(max_in_degree=-1)
    assert m.GraphCSR(*at_limit[:9]).max_in_degree == -1  # the trailing field defaults to "unknown"
    with pytest.raises(ValueError, match="16"):
        m.film_max(x, torch.rand(unknown.num_edges, 2, 2), unknown)
    # a masked graph counts its active edges
    mask = np.ones(len(s), bool)
    mask[np.asarray(d) == 0] = False
    masked = m.RobotGraph(s, d, num_nodes=16, edge_active=torch.from_numpy(mask)).csr("cpu")
    assert masked.graph_kind == _lib.GRAPH_SIMPLE and masked.max_in_degree == 16


def test_gcn_with_film_max_constructs():
    opt = types.SimpleNamespace(feature_dim=8, gcn_mode="film_max")
    gcn = m.GCN(opt)
    assert gcn.opt.gcn_mode == "film_max"
    for combine in ("cat_compress", "cat", "residual", "initial_mix"):
        m.GCNStack(types.SimpleNamespace(feature_dim=8, gcn_mode="film_max", gcn_combine=combine,
                                         gcn_layers=1 if combine == "cat" else 2))
