"""CPU: the pixel-major compress entry points (``mrp_compress_fwd_cl`` / ``_bwd_data_cl`` /
``_bwd_weight_cl`` and the workspace query, added to ABI 22): exports, dtype / pointer / stride / alignment
validation, the zero-size no-op paths, the declined shapes and the tuning knobs — all decided on the host
before any launch, so no GPU is needed."""
import ctypes
import os

import pytest

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib
from conftest import ROOT

HIP_INVALID_VALUE = 1
NS = _lib.HIP_ERROR_NOT_SUPPORTED
HALF = [_lib.DTYPE_BF16, _lib.DTYPE_F16]
BAD_DTYPES = [_lib.DTYPE_F32, -1, 3, 7]
P_ = ctypes.c_void_p
D = P_(4096)  # never dereferenced on the host
ODD = P_(4096 + 8)  # 8-byte but not 16-byte aligned
SYMBOLS = ("mrp_compress_fwd_cl", "mrp_compress_bwd_data_cl", "mrp_compress_bwd_weight_cl_workspace",
           "mrp_compress_bwd_weight_cl")
N, C, P = 3, 32, 49
NSTR = C * P  # dense channels_last: node stride P C, pixel stride C


def _fwd(lib, dt, x=D, xn=NSTR, xp=C, a=D, an=NSTR, ap=C, n=N, c=C, p=P, w=D, b=None, y=D, yn=NSTR, yp=C):
    return lib.mrp_compress_fwd_cl(dt, x, xn, xp, a, an, ap, n, c, p, w, b, y, yn, yp, None)


def _dgrad(lib, dt, gy=D, gn=NSTR, gp=C, n=N, c=C, p=P, w=D, gx=D, gxn=NSTR, gxp=C, ga=D, gan=NSTR, gap=C):
    return lib.mrp_compress_bwd_data_cl(dt, gy, gn, gp, n, c, p, w, gx, gxn, gxp, ga, gan, gap, None)


def _wgrad(lib, dt, gy=D, gn=NSTR, gp=C, x=D, xn=NSTR, xp=C, a=D, an=NSTR, ap=C, n=N, c=C, p=P, gw=D, gb=None,
           ws=None, wsb=0):
    return lib.mrp_compress_bwd_weight_cl(dt, gy, gn, gp, x, xn, xp, a, an, ap, n, c, p, gw, gb, ws, wsb, None)


def test_symbols_exported_and_abi_unchanged():
    lib = m.load_library()
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, s)
    assert lib.mrp_abi_version() == _lib.ABI_VERSION == 22


@pytest.mark.parametrize("bad", BAD_DTYPES)
def test_f32_and_unknown_dtypes_are_invalid(bad):
    lib = m.load_library()
    for call in (_fwd, _dgrad, _wgrad):
        assert call(lib, bad) == HIP_INVALID_VALUE
    assert _fwd(lib, bad, n=0) == HIP_INVALID_VALUE  # even with nothing to do


@pytest.mark.parametrize("dt", HALF)
def test_null_pointers_with_work_are_invalid(dt):
    lib = m.load_library()
    for kw in (dict(x=None), dict(a=None), dict(w=None), dict(y=None)):
        assert _fwd(lib, dt, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gy=None), dict(w=None), dict(gx=None), dict(ga=None)):
        assert _dgrad(lib, dt, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gy=None), dict(x=None), dict(a=None), dict(gw=None, gb=D)):
        assert _wgrad(lib, dt, **kw) == HIP_INVALID_VALUE


@pytest.mark.parametrize("dt", HALF)
def test_short_strides_and_misalignment_are_invalid(dt):
    lib = m.load_library()
    # pixel stride below C; node stride below P pixel strides (dense, and for a 2C buffer's half)
    for kw in (dict(xp=C - 8), dict(ap=C - 8), dict(yp=C - 8), dict(xn=NSTR - 8), dict(an=NSTR - 8),
               dict(yn=NSTR - 8), dict(xp=2 * C, xn=NSTR), dict(yp=2 * C, yn=2 * NSTR - 8)):
        assert _fwd(lib, dt, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gp=C - 8), dict(gxp=C - 8), dict(gap=C - 8), dict(gn=NSTR - 8), dict(gxn=NSTR - 8),
               dict(gan=NSTR - 8), dict(gap=2 * C, gan=NSTR)):
        assert _dgrad(lib, dt, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gp=C - 8), dict(xp=C - 8), dict(ap=C - 8), dict(gn=NSTR - 8), dict(xn=NSTR - 8),
               dict(an=NSTR - 8)):
        assert _wgrad(lib, dt, **kw) == HIP_INVALID_VALUE
    # pointers that are not 16-byte aligned; strides that are not whole 16-byte pieces
    for kw in (dict(x=ODD), dict(a=ODD), dict(w=ODD), dict(y=ODD), dict(xn=NSTR + 4), dict(yn=NSTR + 4),
               dict(xp=C + 4, xn=2 * NSTR), dict(yp=C + 4, yn=2 * NSTR)):
        assert _fwd(lib, dt, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gy=ODD), dict(w=ODD), dict(gx=ODD), dict(ga=ODD), dict(gan=NSTR + 4),
               dict(gxp=C + 4, gxn=2 * NSTR)):
        assert _dgrad(lib, dt, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gy=ODD), dict(x=ODD), dict(a=ODD), dict(gw=ODD), dict(gn=NSTR + 4),
               dict(ap=C + 4, an=2 * NSTR)):
        assert _wgrad(lib, dt, **kw) == HIP_INVALID_VALUE
    # negative sizes
    assert _fwd(lib, dt, n=-1) == HIP_INVALID_VALUE
    assert _dgrad(lib, dt, c=-32) == HIP_INVALID_VALUE
    assert _wgrad(lib, dt, p=-64) == HIP_INVALID_VALUE


@pytest.mark.parametrize("dt", HALF)
def test_strided_operands_are_accepted_up_to_the_launch(dt):
    """Halves of a channels_last 2C buffer (pixel stride 2C) and a batch slice (node stride > P ps) pass
    every check: with the A/B knob off the next answer is hipErrorNotSupported, not invalid-value."""
    lib = m.load_library()
    assert lib.mrp_tuning_set(b"compress_half_cl", 0) == 0
    try:
        wide = dict(xp=2 * C, xn=2 * NSTR, ap=2 * C, an=4 * NSTR)
        assert _fwd(lib, dt, **wide) == NS
        assert _dgrad(lib, dt, gxp=2 * C, gxn=2 * NSTR, gap=2 * C, gan=2 * NSTR) == NS
        assert _wgrad(lib, dt, **wide) == NS
    finally:
        assert lib.mrp_tuning_set(b"compress_half_cl", 1) == 0


@pytest.mark.parametrize("dt", HALF)
def test_zero_sizes_are_noops(dt):
    lib = m.load_library()
    for kw in (dict(n=0), dict(c=0), dict(p=0)):
        assert _fwd(lib, dt, x=None, a=None, w=None, y=None, **kw) == 0
        assert _dgrad(lib, dt, gy=None, w=None, gx=None, ga=None, **kw) == 0
    assert _wgrad(lib, dt, c=0) == 0
    assert _wgrad(lib, dt, gw=None, gb=None) == 0  # nothing wanted
    assert _wgrad(lib, dt, n=0, gw=None, gb=None) == 0


@pytest.mark.parametrize("dt", HALF)
def test_untiled_channel_counts_are_declined(dt):
    lib = m.load_library()
    c2 = 40  # C % 32 != 0 (strides kept whole 16-byte pieces)
    s = dict(c=c2)
    assert _fwd(lib, dt, xn=c2 * P, xp=c2, an=c2 * P, ap=c2, yn=c2 * P, yp=c2, **s) == NS
    assert _dgrad(lib, dt, gn=c2 * P, gp=c2, gxn=c2 * P, gxp=c2, gan=c2 * P, gap=c2, **s) == NS
    assert _wgrad(lib, dt, gn=c2 * P, gp=c2, xn=c2 * P, xp=c2, an=c2 * P, ap=c2, **s) == NS
    assert lib.mrp_compress_bwd_weight_cl_workspace(4, c2, P) == 0
    # any P is tiled: with valid arguments only the knob declines
    assert lib.mrp_tuning_set(b"compress_half_cl", 0) == 0
    try:
        assert _fwd(lib, dt) == NS and _dgrad(lib, dt) == NS and _wgrad(lib, dt) == NS
    finally:
        assert lib.mrp_tuning_set(b"compress_half_cl", 1) == 0


def test_workspace_query_and_short_workspace():
    lib = m.load_library()
    ws = lib.mrp_compress_bwd_weight_cl_workspace
    assert ws(0, 32, 64) == 0 and ws(4, 32, 0) == 0 and ws(-1, 32, 64) == 0
    try:
        # a forced split count: [splits][C][2C] partial tiles + [splits][C] bias sums, fp32; K = 4096 is 128
        # stages; one split needs no workspace; more splits than stages are clamped (K = 49: 2 stages)
        assert lib.mrp_tuning_set(b"half_cl_splits", 3) == 0
        assert ws(64, 64, 64) == (3 * 64 * 128 + 3 * 64) * 4
        assert lib.mrp_tuning_set(b"half_cl_splits", 1) == 0
        assert ws(64, 64, 64) == 0
        assert lib.mrp_tuning_set(b"half_cl_splits", 256) == 0
        assert ws(1, 32, 49) == (2 * 32 * 64 + 2 * 32) * 4
        assert lib.mrp_tuning_set(b"half_cl_splits", 257) == HIP_INVALID_VALUE
        assert lib.mrp_tuning_set(b"half_cl_splits", 2) == 0
        for dt in HALF:  # a too-small workspace is refused before the launch
            assert _wgrad(lib, dt, ws=None, wsb=0) == HIP_INVALID_VALUE
            assert _wgrad(lib, dt, ws=D, wsb=16) == HIP_INVALID_VALUE
            assert _wgrad(lib, dt, ws=ODD, wsb=1 << 20) == HIP_INVALID_VALUE
    finally:
        assert lib.mrp_tuning_set(b"half_cl_splits", 0) == 0


def test_knobs_accepted_and_named_in_the_header():
    lib = m.load_library()
    header = open(os.path.join(ROOT, "include", "mrp_gnn.h"), "rb").read()
    for name, lo, hi in ((b"compress_half_cl", 0, 1), (b"half_cl_splits", 0, 256)):
        assert b'"' + name + b'"' in header
        assert lib.mrp_tuning_set(name, lo - 1) == HIP_INVALID_VALUE
        assert lib.mrp_tuning_set(name, hi + 1) == HIP_INVALID_VALUE
        assert lib.mrp_tuning_set(name, hi) == 0
    assert lib.mrp_tuning_set(b"compress_half_cl", 1) == 0 and lib.mrp_tuning_set(b"half_cl_splits", 0) == 0
    for s in SYMBOLS:
        assert s.encode() in header
