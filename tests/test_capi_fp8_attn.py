"""CPU: the FP8 receiver-side entry points of the max and attention reducers (``mrp_film_max_fwd_q``,
``mrp_film_attn_fwd_q``, ``mrp_film_wattn_fwd_q``, added to ABI 22 without a new number): exports, every rejection
the header lists — all decided on the host before any launch, so dummy pointers do and no GPU is needed — and the
zero-size no-op paths."""
import ctypes
import os

import pytest

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib
from conftest import ROOT

HIP_INVALID_VALUE = 1
DUMMY = ctypes.c_void_p(1 << 20)  # never dereferenced on the host
QDTYPES = [_lib.QDTYPE_E4M3, _lib.QDTYPE_E5M2]
DTYPES = [_lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16]
NEW = ("mrp_film_max_fwd_q", "mrp_film_attn_fwd_q", "mrp_film_wattn_fwd_q")
# two complete graphs of 4 nodes, C = 4, P = 16
FULL = dict(kind=_lib.GRAPH_COMPLETE, B=2, maxn=4, Nt=8, E=24, C=4, P=16, gb=DUMMY, xq=DUMMY, xs=64, q=DUMMY, qs=64,
            out=DUMMY, os=64, attn=DUMMY, w=DUMMY, wst=16, heads=1, scale=0.5)


def _args(kw):
    a = dict(xq=None, xs=0, xscale=None, q=None, qs=0, gb=None, w=None, wst=0, indptr=None, src=None, eid=None,
             goff=None, B=0, maxn=0, kind=0, Nt=0, E=0, C=0, P=0, flags=0, heads=1, out=None, os=0, scale=1.0,
             attn=None, rate=None, wsb=0)
    a.update(kw)
    return a


def _graph(a):
    return (a["indptr"], a["src"], a["eid"], a["goff"], a["B"], a["maxn"], a["kind"], a["Nt"], a["E"], a["C"],
            a["P"], a["flags"])


def _max(lib, qdtype, dtype, **kw):
    a = _args(kw)
    return lib.mrp_film_max_fwd_q(qdtype, a["xq"], a["xs"], a["xscale"], dtype, a["gb"], *_graph(a), a["out"],
                                  a["os"], None)


def _attn(lib, qdtype, dtype, **kw):
    a = _args(kw)
    return lib.mrp_film_attn_fwd_q(qdtype, a["xq"], a["xs"], a["xscale"], dtype, a["q"], a["qs"], a["gb"],
                                   *_graph(a), a["heads"], a["out"], a["os"], a["scale"], a["attn"], None, a["wsb"],
                                   None)


def _wattn(lib, qdtype, dtype, **kw):
    a = _args(kw)
    return lib.mrp_film_wattn_fwd_q(qdtype, a["xq"], a["xs"], a["xscale"], dtype, a["q"], a["qs"], a["gb"], a["w"],
                                    a["wst"], *_graph(a), a["heads"], a["out"], a["os"], a["scale"], a["attn"],
                                    a["rate"], None, a["wsb"], None)


def test_symbols_exported_and_abi_unchanged():
    lib = m.load_library()
    for s in NEW:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert lib.mrp_abi_version() == _lib.ABI_VERSION == 22
    header = open(os.path.join(ROOT, "include", "mrp_gnn.h"), encoding="utf-8").read()
    for s in NEW:
        assert f"int {s}(" in header


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("qdtype", QDTYPES)
@pytest.mark.parametrize("call", [_max, _attn, _wattn], ids=["max", "attn", "wattn"])
def test_rejections_come_before_any_launch(call, qdtype, dtype):
    lib = m.load_library()
    bad = lambda **kw: call(lib, qdtype, dtype, **dict(FULL, **kw)) == HIP_INVALID_VALUE  # noqa: E731
    for q in (-1, 2, 7):  # a bad qdtype, even for an empty batch
        assert call(lib, q, dtype) == HIP_INVALID_VALUE
        assert call(lib, q, dtype, **FULL) == HIP_INVALID_VALUE
    for t in (-1, 3, 7):  # a bad dtype / out_dtype
        assert call(lib, qdtype, t) == HIP_INVALID_VALUE
        assert call(lib, qdtype, t, **FULL) == HIP_INVALID_VALUE
    assert bad(xq=None) and bad(out=None) and bad(gb=None)  # a NULL pointer with work to do
    assert bad(xs=63) and bad(os=63)  # a node stride < C * P
    assert bad(maxn=17, Nt=34, E=2 * 17 * 16)  # max_nodes over 16
    regular = dict(indptr=DUMMY, src=DUMMY, eid=DUMMY, goff=DUMMY)
    assert bad(kind=_lib.graph_regular(17), maxn=16, Nt=32, E=17 * 32, **regular)  # in-degree over 16
    assert bad(kind=4)  # an unknown graph kind
    assert bad(flags=1) and bad(flags=0x200)  # an unknown flag
    assert bad(E=23)  # a complete graph with the wrong edge count
    if call is not _max:
        assert bad(q=None) and bad(attn=None)
        assert bad(qs=63)
        assert bad(heads=0) and bad(heads=-1) and bad(heads=3)  # heads not dividing C = 4
        assert bad(scale=float("nan")) and bad(scale=float("inf"))
        assert bad(wsb=-1)
    if call is _wattn:
        assert bad(w=None) and bad(wst=15)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("qdtype", QDTYPES)
@pytest.mark.parametrize("call", [_max, _attn, _wattn], ids=["max", "attn", "wattn"])
def test_zero_sizes_are_noops(call, qdtype, dtype):
    """No kernel, no memset (attn / rate are not passed): the calls succeed on a host without a GPU."""
    lib = m.load_library()
    assert call(lib, qdtype, dtype) == 0  # empty batch
    base = dict(kind=_lib.GRAPH_COMPLETE, B=2, maxn=4, Nt=8, E=24, C=4, P=16)
    for kw in (dict(base, C=0), dict(base, P=0), dict(base, B=0, Nt=0, E=0)):
        assert call(lib, qdtype, dtype, **kw) == 0
        if call is not _max:
            assert call(lib, qdtype, dtype, **dict(kw, heads=2)) == 0
            # the rejections still come first
            assert call(lib, qdtype, dtype, **dict(kw, heads=0)) == HIP_INVALID_VALUE
        assert call(lib, -1, dtype, **kw) == HIP_INVALID_VALUE


def test_existing_entry_points_are_as_they_were():
    """Nothing existing changed: the typed forwards still reject dtype codes 3 and 7, and the FP8 mean still
    rejects an own-feature epilogue."""
    lib = m.load_library()
    graph = (DUMMY, None, None, None, None, 2, 4, 1, 8, 24, 4, 16, 0)
    for bad in (3, 7):
        assert lib.mrp_film_max_fwd(bad, DUMMY, 64, *graph, DUMMY, 64, None) == HIP_INVALID_VALUE
        assert lib.mrp_film_attn_fwd_mh(bad, DUMMY, 64, *graph, 1, DUMMY, 64, 0.5, DUMMY, None, 0, None) == \
            HIP_INVALID_VALUE
    ep = _lib.Epilogue(1.0, 1.0, None, 0, 0.0, None, 0)
    assert lib.mrp_film_mean_fwd_q(0, DUMMY, 64, None, 0, *graph, DUMMY, 64, ctypes.byref(ep), None) == \
        HIP_INVALID_VALUE
