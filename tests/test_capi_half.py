"""CPU: the typed aggregation entry points (ABI 22, ``mrp_film_mean_fwd_t`` / ``mrp_film_mean_bwd_t``):
exports, dtype and pointer validation, and the zero-size no-op paths — all decided on the host before
any launch, so no GPU is needed."""
import ctypes

import pytest

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib

HIP_INVALID_VALUE = 1
DTYPES = [_lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16]
DUMMY = ctypes.c_void_p(64)  # never dereferenced on the host


def _fwd(lib, dtype, **kw):
    a = dict(x=None, xs=0, gb=None, indptr=None, src=None, eid=None, goff=None, B=0, maxn=0, kind=0, Nt=0, E=0,
             C=0, P=0, mode=0, out=None, os=0, ep=None, stream=None)
    a.update(kw)
    return lib.mrp_film_mean_fwd_t(dtype, a["x"], a["xs"], a["gb"], a["indptr"], a["src"], a["eid"], a["goff"],
                                   a["B"], a["maxn"], a["kind"], a["Nt"], a["E"], a["C"], a["P"], a["mode"],
                                   a["out"], a["os"], a["ep"], a["stream"])


def _bwd(lib, dtype, **kw):
    a = dict(g=None, gs=0, x=None, xs=0, gb=None, indptr=None, src=None, eid=None, goff=None, B=0, maxn=0, kind=0,
             Nt=0, E=0, C=0, P=0, mode=0, dx=None, dxs=0, base=None, bs=0, dgb=None, ep=None, stream=None)
    a.update(kw)
    return lib.mrp_film_mean_bwd_t(dtype, a["g"], a["gs"], a["x"], a["xs"], a["gb"], a["indptr"], a["src"],
                                   a["eid"], a["goff"], a["B"], a["maxn"], a["kind"], a["Nt"], a["E"], a["C"],
                                   a["P"], a["mode"], a["dx"], a["dxs"], a["base"], a["bs"], a["dgb"], a["ep"],
                                   a["stream"])


def test_typed_symbols_exported():
    lib = m.load_library()
    for s in ("mrp_film_mean_fwd_t", "mrp_film_mean_bwd_t"):
        assert s in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, s)
    assert lib.mrp_abi_version() == _lib.ABI_VERSION == 22
    assert (_lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16) == (0, 1, 2)


@pytest.mark.parametrize("bad", [-1, 3, 7])
def test_unknown_dtype_is_invalid(bad):
    lib = m.load_library()
    assert _fwd(lib, bad) == HIP_INVALID_VALUE  # even for an empty batch
    assert _bwd(lib, bad) == HIP_INVALID_VALUE
    # complete graphs, consistent sizes, pointers given: still the dtype that is rejected
    full = dict(kind=1, B=2, maxn=4, Nt=8, E=24, C=2, P=16, gb=DUMMY)
    assert _fwd(lib, bad, x=DUMMY, out=DUMMY, xs=32, os=32, **full) == HIP_INVALID_VALUE
    assert _bwd(lib, bad, g=DUMMY, gs=32, x=DUMMY, xs=32, dx=DUMMY, dxs=32, dgb=DUMMY, **full) == HIP_INVALID_VALUE


@pytest.mark.parametrize("dtype", DTYPES)
def test_null_feature_pointers_with_work_are_invalid(dtype):
    lib = m.load_library()
    full = dict(kind=1, B=2, maxn=4, Nt=8, E=24, C=2, P=16, gb=DUMMY)  # complete graphs: no index arrays read
    assert _fwd(lib, dtype, x=None, out=DUMMY, xs=32, os=32, **full) == HIP_INVALID_VALUE
    assert _fwd(lib, dtype, x=DUMMY, out=None, xs=32, os=32, **full) == HIP_INVALID_VALUE
    assert _fwd(lib, dtype, x=DUMMY, out=DUMMY, xs=31, os=32, **full) == HIP_INVALID_VALUE  # stride < C*P
    # backward: grad_x wanted without grad_out; grad_gb wanted without x
    assert _bwd(lib, dtype, g=None, gs=32, dx=DUMMY, dxs=32, **full) == HIP_INVALID_VALUE
    assert _bwd(lib, dtype, g=DUMMY, gs=32, x=None, xs=32, dgb=DUMMY, **full) == HIP_INVALID_VALUE
    assert _bwd(lib, dtype, g=DUMMY, gs=32, dx=DUMMY, dxs=31, **full) == HIP_INVALID_VALUE


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_sizes_are_noops(dtype):
    lib = m.load_library()
    assert _fwd(lib, dtype) == 0  # empty batch (num_nodes = 0)
    assert _bwd(lib, dtype) == 0  # nothing requested
    assert _fwd(lib, dtype, kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16) == 0  # C = 0
    assert _fwd(lib, dtype, kind=1, B=2, maxn=4, Nt=8, E=24, C=2, P=0) == 0   # P = 0
    assert _fwd(lib, dtype, kind=1, B=0, maxn=4, Nt=0, E=0, C=2, P=16) == 0   # num_nodes = 0
    # backward with grad_x wanted but nothing to compute
    assert _bwd(lib, dtype, kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16, dx=DUMMY) == 0
    assert _bwd(lib, dtype, kind=1, B=2, maxn=4, Nt=8, E=24, C=2, P=0, dx=DUMMY) == 0
    assert _bwd(lib, dtype, kind=1, B=0, maxn=4, Nt=0, E=0, C=2, P=16, dx=DUMMY) == 0


def test_f32_forwards_to_the_fp32_validation():
    """MRP_DTYPE_F32 is the fp32 entry point: the same answers on the same malformed arguments."""
    lib = m.load_library()
    for kw in (dict(mode=3), dict(C=-1), dict(kind=2), dict(kind=1, B=2, maxn=4, Nt=8, E=23)):
        assert _fwd(lib, _lib.DTYPE_F32, **kw) == HIP_INVALID_VALUE
        assert _fwd(lib, _lib.DTYPE_BF16, **kw) == HIP_INVALID_VALUE
