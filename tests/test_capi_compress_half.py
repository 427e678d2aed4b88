"""CPU: the typed compress entry points (``mrp_compress_pack_t`` / ``_fwd_t`` / ``_bwd_data_t`` /
``_bwd_weight_t`` and their size queries, added to ABI 22): exports, dtype / pointer / stride /
alignment validation, the zero-size no-op paths and the declined shapes — all decided on the host before
any launch, so no GPU is needed."""
import ctypes

import pytest

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib

HIP_INVALID_VALUE = 1
HALF = [_lib.DTYPE_BF16, _lib.DTYPE_F16]
BAD_DTYPES = [_lib.DTYPE_F32, -1, 3, 7]
P_ = ctypes.c_void_p
D = P_(4096)  # never dereferenced on the host
ODD = P_(4096 + 8)  # 8-byte but not 16-byte aligned
SYMBOLS = ("mrp_compress_pack_t_bytes", "mrp_compress_pack_t", "mrp_compress_fwd_t", "mrp_compress_bwd_data_t",
           "mrp_compress_bwd_weight_t_workspace", "mrp_compress_bwd_weight_t")
N, C, P = 3, 32, 64
PLANE = C * P


def _pack(lib, dt, w=D, ld=2 * C, tr=0, M=C, K=2 * C, out=D):
    return lib.mrp_compress_pack_t(dt, w, ld, tr, M, K, out, None)


def _fwd(lib, dt, x=D, xs=PLANE, a=D, as_=PLANE, n=N, c=C, p=P, w=D, b=None, y=D, ys=PLANE):
    return lib.mrp_compress_fwd_t(dt, x, xs, a, as_, n, c, p, w, b, y, ys, None)


def _dgrad(lib, dt, gy=D, gs=PLANE, n=N, c=C, p=P, w=D, gx=D, gxs=PLANE, ga=D, gas=PLANE):
    return lib.mrp_compress_bwd_data_t(dt, gy, gs, n, c, p, w, gx, gxs, ga, gas, None)


def _wgrad(lib, dt, gy=D, gs=PLANE, x=D, xs=PLANE, a=D, as_=PLANE, n=N, c=C, p=P, gw=D, gb=None, ws=None, wsb=0):
    return lib.mrp_compress_bwd_weight_t(dt, gy, gs, x, xs, a, as_, n, c, p, gw, gb, ws, wsb, None)


def test_symbols_exported_and_abi_unchanged():
    lib = m.load_library()
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, s)
    assert lib.mrp_abi_version() == _lib.ABI_VERSION == 22


@pytest.mark.parametrize("bad", BAD_DTYPES)
def test_f32_and_unknown_dtypes_are_invalid(bad):
    lib = m.load_library()
    for call in (_pack, _fwd, _dgrad, _wgrad):
        assert call(lib, bad) == HIP_INVALID_VALUE
    assert _fwd(lib, bad, n=0) == HIP_INVALID_VALUE  # even with nothing to do


@pytest.mark.parametrize("dt", HALF)
def test_null_pointers_with_work_are_invalid(dt):
    lib = m.load_library()
    assert _pack(lib, dt, w=None) == HIP_INVALID_VALUE
    assert _pack(lib, dt, out=None) == HIP_INVALID_VALUE
    for kw in (dict(x=None), dict(a=None), dict(w=None), dict(y=None)):
        assert _fwd(lib, dt, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gy=None), dict(w=None), dict(gx=None), dict(ga=None)):
        assert _dgrad(lib, dt, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gy=None), dict(x=None), dict(a=None), dict(gw=None, gb=D)):
        assert _wgrad(lib, dt, **kw) == HIP_INVALID_VALUE


@pytest.mark.parametrize("dt", HALF)
def test_short_strides_and_misalignment_are_invalid(dt):
    lib = m.load_library()
    for kw in (dict(xs=PLANE - 8), dict(as_=PLANE - 8), dict(ys=PLANE - 8)):
        assert _fwd(lib, dt, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gs=PLANE - 8), dict(gxs=PLANE - 8), dict(gas=PLANE - 8)):
        assert _dgrad(lib, dt, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gs=PLANE - 8), dict(xs=PLANE - 8), dict(as_=PLANE - 8)):
        assert _wgrad(lib, dt, **kw) == HIP_INVALID_VALUE
    assert _pack(lib, dt, ld=2 * C - 1) == HIP_INVALID_VALUE
    # pointers that are not 16-byte aligned, node strides that are not whole 16-byte pieces
    assert _pack(lib, dt, out=ODD) == HIP_INVALID_VALUE
    for kw in (dict(x=ODD), dict(a=ODD), dict(w=ODD), dict(y=ODD), dict(xs=PLANE + 4), dict(ys=PLANE + 4)):
        assert _fwd(lib, dt, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gy=ODD), dict(gx=ODD), dict(ga=ODD), dict(gas=PLANE + 4)):
        assert _dgrad(lib, dt, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gy=ODD), dict(x=ODD), dict(a=ODD), dict(gw=ODD), dict(gs=PLANE + 4)):
        assert _wgrad(lib, dt, **kw) == HIP_INVALID_VALUE
    # negative sizes
    assert _fwd(lib, dt, n=-1) == HIP_INVALID_VALUE
    assert _dgrad(lib, dt, c=-32) == HIP_INVALID_VALUE
    assert _wgrad(lib, dt, p=-64) == HIP_INVALID_VALUE


@pytest.mark.parametrize("dt", HALF)
def test_zero_sizes_are_noops(dt):
    lib = m.load_library()
    assert _pack(lib, dt, M=0) == 0 and _pack(lib, dt, K=0) == 0
    for kw in (dict(n=0), dict(c=0), dict(p=0)):
        assert _fwd(lib, dt, x=None, a=None, w=None, y=None, **kw) == 0
        assert _dgrad(lib, dt, gy=None, w=None, gx=None, ga=None, **kw) == 0
    assert _wgrad(lib, dt, c=0) == 0
    assert _wgrad(lib, dt, gw=None, gb=None) == 0  # nothing wanted
    assert _wgrad(lib, dt, n=0, gw=None, gb=None) == 0


@pytest.mark.parametrize("dt", HALF)
def test_untiled_shapes_are_declined(dt):
    lib = m.load_library()
    ns = _lib.HIP_ERROR_NOT_SUPPORTED
    assert _pack(lib, dt, M=48) == ns and _pack(lib, dt, K=48, ld=48) == ns
    c2, p2 = 48, 60  # C % 32 != 0; P % 8 != 0 (strides kept whole 16-byte pieces)
    assert _fwd(lib, dt, c=c2, xs=c2 * P, as_=c2 * P, ys=c2 * P) == ns
    assert _fwd(lib, dt, p=p2, xs=C * 64, as_=C * 64, ys=C * 64) == ns
    assert _dgrad(lib, dt, c=c2, gs=c2 * P, gxs=c2 * P, gas=c2 * P) == ns
    assert _dgrad(lib, dt, p=p2, gs=C * 64, gxs=C * 64, gas=C * 64) == ns
    assert _wgrad(lib, dt, c=c2, gs=c2 * P, xs=c2 * P, as_=c2 * P) == ns
    assert _wgrad(lib, dt, p=16, gs=C * 16, xs=C * 16, as_=C * 16) == ns  # P % 8 == 0 but P % 32 != 0
    # the A/B knob turns the native kernels off: every shape is declined
    assert lib.mrp_tuning_set(b"compress_half", 0) == 0
    try:
        assert _fwd(lib, dt) == ns and _dgrad(lib, dt) == ns and _wgrad(lib, dt) == ns
    finally:
        assert lib.mrp_tuning_set(b"compress_half", 1) == 0


def test_size_queries():
    lib = m.load_library()
    assert lib.mrp_compress_pack_t_bytes(32, 64) == 32 * 64 * 2
    assert lib.mrp_compress_pack_t_bytes(512, 1024) == 512 * 1024 * 2
    for M, K in ((0, 64), (32, 0), (48, 64), (32, 48), (32, 16), (-32, 64)):
        assert lib.mrp_compress_pack_t_bytes(M, K) == 0
    ws = lib.mrp_compress_bwd_weight_t_workspace
    assert ws(0, 32, 64) == 0 and ws(4, 48, 64) == 0 and ws(4, 32, 16) == 0
    try:
        # a forced split count: [splits][C][2C] partial tiles + [splits][C] row sums, fp32; K = 4096 has
        # 128 stages; one split needs no workspace; more splits than stages are clamped
        assert lib.mrp_tuning_set(b"half_nt_splits", 3) == 0
        assert ws(64, 64, 64) == (3 * 64 * 128 + 3 * 64) * 4
        assert lib.mrp_tuning_set(b"half_nt_splits", 1) == 0
        assert ws(64, 64, 64) == 0
        assert lib.mrp_tuning_set(b"half_nt_splits", 256) == 0
        assert ws(1, 32, 64) == (2 * 32 * 64 + 2 * 32) * 4
        assert lib.mrp_tuning_set(b"half_nt_splits", 257) == HIP_INVALID_VALUE
    finally:
        assert lib.mrp_tuning_set(b"half_nt_splits", 0) == 0
    # a too-small workspace is refused before the launch
    assert lib.mrp_tuning_set(b"half_nt_splits", 2) == 0
    try:
        for dt in HALF:
            assert _wgrad(lib, dt, ws=None, wsb=0) == HIP_INVALID_VALUE
            assert _wgrad(lib, dt, ws=D, wsb=16) == HIP_INVALID_VALUE
    finally:
        assert lib.mrp_tuning_set(b"half_nt_splits", 0) == 0
