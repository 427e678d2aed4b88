"""CPU: the pixel-major (channels-last) aggregation entry points ``mrp_film_mean_fwd_cl`` /
``mrp_film_mean_bwd_cl`` / ``mrp_film_mean_bwd_cl_workspace``: exports (header, ``_lib`` and the shared
object agree, ABI still 22), every validation rule's return code, the zero-size no-ops and the workspace
query — all decided on the host before anything is enqueued, so no GPU is needed."""
import ctypes
import os
import re

import pytest

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib

HIP_INVALID_VALUE = 1
HIP_NOT_SUPPORTED = _lib.HIP_ERROR_NOT_SUPPORTED
DTYPES = [_lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16]
DUMMY = ctypes.c_void_p(64)  # never dereferenced on the host
NEW = ("mrp_film_mean_fwd_cl", "mrp_film_mean_bwd_cl", "mrp_film_mean_bwd_cl_workspace")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mrp_gnn.h")

# two complete 4-node graphs, C = 8, P = 16: dense channels-last strides are (P * C, C) = (128, 8)
FULL = dict(kind=1, B=2, maxn=4, Nt=8, E=24, C=8, P=16, gb=DUMMY)


def _fwd(lib, dtype, **kw):
    a = dict(x=None, xs=0, xp=0, gb=None, indptr=None, src=None, eid=None, goff=None, B=0, maxn=0, kind=0, Nt=0,
             E=0, C=0, P=0, mode=0, out=None, os=0, op=0, ep=None, stream=None)
    a.update(kw)
    return lib.mrp_film_mean_fwd_cl(dtype, a["x"], a["xs"], a["xp"], a["gb"], a["indptr"], a["src"], a["eid"],
                                    a["goff"], a["B"], a["maxn"], a["kind"], a["Nt"], a["E"], a["C"], a["P"],
                                    a["mode"], a["out"], a["os"], a["op"], a["ep"], a["stream"])


def _bwd(lib, dtype, **kw):
    a = dict(g=None, gs=0, gp=0, x=None, xs=0, xp=0, gb=None, indptr=None, src=None, eid=None, goff=None, B=0,
             maxn=0, kind=0, Nt=0, E=0, C=0, P=0, mode=0, dx=None, dxs=0, dxp=0, base=None, bs=0, bp=0, dgb=None,
             ep=None, ws=None, wsb=0, stream=None)
    a.update(kw)
    return lib.mrp_film_mean_bwd_cl(dtype, a["g"], a["gs"], a["gp"], a["x"], a["xs"], a["xp"], a["gb"], a["indptr"],
                                    a["src"], a["eid"], a["goff"], a["B"], a["maxn"], a["kind"], a["Nt"], a["E"],
                                    a["C"], a["P"], a["mode"], a["dx"], a["dxs"], a["dxp"], a["base"], a["bs"],
                                    a["bp"], a["dgb"], a["ep"], a["ws"], a["wsb"], a["stream"])


def test_header_bindings_and_library_agree():
    lib = m.load_library()
    declared = set(re.findall(r"\b(mrp_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for s in NEW:
        assert s in declared and s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s)
    for s in _lib.EXPORTED_SYMBOLS:  # (the header's comments also name functions of earlier ABIs)
        assert s in declared and hasattr(lib, s), s
    assert lib.mrp_abi_version() == _lib.ABI_VERSION == 22  # extended without a new number
    # mrp_agg_epilogue_cl = mrp_agg_epilogue + the two pixel strides
    names = [f[0] for f in _lib.EpilogueCl._fields_]
    assert names[:len(_lib.Epilogue._fields_)] == [f[0] for f in _lib.Epilogue._fields_]
    assert names[-2:] == ["x0_pixel_stride", "xcopy_pixel_stride"]


@pytest.mark.parametrize("bad", [-1, 3, 7])
def test_unknown_dtype_is_invalid(bad):
    lib = m.load_library()
    assert _fwd(lib, bad) == HIP_INVALID_VALUE  # even for an empty batch
    assert _bwd(lib, bad) == HIP_INVALID_VALUE
    assert _fwd(lib, bad, x=DUMMY, xs=128, xp=8, out=DUMMY, os=128, op=8, **FULL) == HIP_INVALID_VALUE
    assert _bwd(lib, bad, g=DUMMY, gs=128, gp=8, dx=DUMMY, dxs=128, dxp=8, **FULL) == HIP_INVALID_VALUE


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_validation(dtype):
    lib = m.load_library()
    ok = dict(x=DUMMY, xs=128, xp=8, out=DUMMY, os=128, op=8)

    def call(**kw):
        a = dict(ok)
        a.update(FULL)
        a.update(kw)
        return _fwd(lib, dtype, **a)

    assert call(x=None) == HIP_INVALID_VALUE           # NULL with work to do
    assert call(out=None) == HIP_INVALID_VALUE
    assert call(gb=None) == HIP_INVALID_VALUE          # FiLM mode without gamma/beta
    assert call(xp=7) == HIP_INVALID_VALUE             # pixel_stride < C
    assert call(op=7) == HIP_INVALID_VALUE
    assert call(xs=127) == HIP_INVALID_VALUE           # node_stride < P * pixel_stride
    assert call(xp=16, xs=255) == HIP_INVALID_VALUE    # ... with a wider pixel stride (a cat half)
    assert call(os=127) == HIP_INVALID_VALUE
    assert call(maxn=17, Nt=34, E=2 * 17 * 16) == HIP_INVALID_VALUE  # max_nodes > MRP_MAX_NODES
    assert call(mode=3) == HIP_INVALID_VALUE
    # the epilogue's tensors follow the same rules
    ep = _lib.EpilogueCl(1.0, 0.0, 64, 128, 0.5, 0, 0, 7, 0)          # x0 pixel stride < C
    assert call(ep=ctypes.byref(ep)) == HIP_INVALID_VALUE
    ep = _lib.EpilogueCl(1.0, 0.0, 0, 0, 0.0, 64, 127, 0, 8)          # xcopy node stride < P * pixel stride
    assert call(ep=ctypes.byref(ep)) == HIP_INVALID_VALUE


@pytest.mark.parametrize("dtype", DTYPES)
def test_span_beyond_the_kernels_offsets_is_not_supported(dtype):
    """P * pixel_stride * sizeof(T) >= 2^31: the lanes' 32-bit byte offsets would not hold a node's span."""
    lib = m.load_library()
    P, C = 1 << 20, 8
    ps = 1 << 11  # 2^31 elements per node: >= 2^32 bytes
    big = dict(kind=1, B=1, maxn=2, Nt=2, E=2, C=C, P=P, gb=DUMMY)
    assert _fwd(lib, dtype, x=DUMMY, xs=P * ps, xp=ps, out=DUMMY, os=P * C, op=C, **big) == HIP_NOT_SUPPORTED
    assert _fwd(lib, dtype, x=DUMMY, xs=P * C, xp=C, out=DUMMY, os=P * ps, op=ps, **big) == HIP_NOT_SUPPORTED
    assert _bwd(lib, dtype, g=DUMMY, gs=P * ps, gp=ps, dx=DUMMY, dxs=P * C, dxp=C, **big) == HIP_NOT_SUPPORTED
    # an invalid argument is reported first
    assert _fwd(lib, dtype, x=None, xs=P * ps, xp=ps, out=DUMMY, os=P * C, op=C, **big) == HIP_INVALID_VALUE


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_validation(dtype):
    lib = m.load_library()
    ok = dict(g=DUMMY, gs=128, gp=8, x=DUMMY, xs=128, xp=8, dx=DUMMY, dxs=128, dxp=8)

    def call(**kw):
        a = dict(ok)
        a.update(FULL)
        a.update(kw)
        return _bwd(lib, dtype, **a)

    assert call(g=None) == HIP_INVALID_VALUE                       # grad_x wanted without grad_out
    assert call(gp=7) == HIP_INVALID_VALUE
    assert call(gs=127) == HIP_INVALID_VALUE
    assert call(dxp=7) == HIP_INVALID_VALUE
    assert call(dxs=127) == HIP_INVALID_VALUE
    assert call(base=DUMMY, bs=128, bp=7) == HIP_INVALID_VALUE     # the base's pixel stride < C
    assert call(base=DUMMY, bs=127, bp=8) == HIP_INVALID_VALUE
    assert call(dx=None, dgb=DUMMY, x=None) == HIP_INVALID_VALUE   # grad_gb wanted without x
    assert call(dx=None, dgb=DUMMY, xp=7) == HIP_INVALID_VALUE
    assert call(gb=None) == HIP_INVALID_VALUE
    assert call(maxn=17, Nt=34, E=2 * 17 * 16) == HIP_INVALID_VALUE


def test_workspace_query_and_what_the_backward_accepts():
    lib = m.load_library()
    q = lib.mrp_film_mean_bwd_cl_workspace
    # two 8-node graphs, C = 8, 32x32: a split plane
    args = (2, 8, _lib.GRAPH_COMPLETE, 8, 1024)
    need = q(*args, _lib.MODE_FILM_MEAN, 1)
    assert need > 0 and need % 4 == 0
    assert q(*args, _lib.MODE_FILM_MEAN | _lib.GB_LOGITS, 1) == need
    assert q(*args, _lib.MODE_FILM_MEAN, 0) == 0   # grad_gb not wanted
    assert q(*args, _lib.MODE_COPY_MEAN, 1) == 0   # grad_gb is a zero fill
    assert q(0, 8, _lib.GRAPH_COMPLETE, 8, 1024, 0, 1) == 0
    # many graphs and channel blocks: whole planes, nothing to reduce
    assert q(64, 8, _lib.GRAPH_COMPLETE, 512, 64, 0, 1) == 0
    # the backward rejects a smaller workspace, and a missing one, before any launch
    shape = dict(kind=1, B=2, maxn=8, Nt=16, E=112, C=8, P=1024, gb=DUMMY, g=DUMMY, gs=8192, gp=8, x=DUMMY,
                 xs=8192, xp=8, dgb=DUMMY)
    for dtype in DTYPES:
        assert _bwd(lib, dtype, ws=DUMMY, wsb=need - 4, **shape) == HIP_INVALID_VALUE
        assert _bwd(lib, dtype, ws=None, wsb=need, **shape) == HIP_INVALID_VALUE
        assert _bwd(lib, dtype, ws=None, wsb=0, **shape) == HIP_INVALID_VALUE


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_sizes_are_noops(dtype):
    lib = m.load_library()
    assert _fwd(lib, dtype) == 0  # empty batch
    assert _bwd(lib, dtype) == 0  # nothing requested
    assert _fwd(lib, dtype, kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16) == 0
    assert _fwd(lib, dtype, kind=1, B=2, maxn=4, Nt=8, E=24, C=8, P=0) == 0
    assert _fwd(lib, dtype, kind=1, B=0, maxn=4, Nt=0, E=0, C=8, P=16) == 0
    assert _bwd(lib, dtype, kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16, dx=DUMMY) == 0
    assert _bwd(lib, dtype, kind=1, B=2, maxn=4, Nt=8, E=24, C=8, P=0, dx=DUMMY) == 0
    assert _bwd(lib, dtype, kind=1, B=0, maxn=4, Nt=0, E=0, C=8, P=16, dx=DUMMY) == 0
    assert _bwd(lib, dtype, **FULL) == 0  # sizes given, neither gradient wanted
