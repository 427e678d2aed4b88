"""CPU: the pixel-major fp32 split-bf16 compress entry points (``mrp_compress_fwd_split_cl`` /
``_bwd_data_split_cl`` / ``_bwd_weight_split_cl`` and the workspace query, added to ABI 22): exports, the
``parts`` check, pointer / stride / alignment validation, the zero-size no-op paths, the declined shapes and
the tuning knobs — all decided on the host before any launch, so no GPU is needed."""
import ctypes
import os

import pytest

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib
from conftest import ROOT

HIP_INVALID_VALUE = 1
NS = _lib.HIP_ERROR_NOT_SUPPORTED
PARTS = [1, 2, 3]
P_ = ctypes.c_void_p
D = P_(4096)  # never dereferenced on the host
ODD = P_(4096 + 8)  # 8-byte but not 16-byte aligned
SYMBOLS = ("mrp_compress_fwd_split_cl", "mrp_compress_bwd_data_split_cl",
           "mrp_compress_bwd_weight_split_cl_workspace", "mrp_compress_bwd_weight_split_cl")
N, C, P = 3, 32, 49
NSTR = C * P  # dense channels_last: node stride P C, pixel stride C


def _fwd(lib, parts, x=D, xn=NSTR, xp=C, a=D, an=NSTR, ap=C, n=N, c=C, p=P, w=D, b=None, y=D, yn=NSTR, yp=C):
    return lib.mrp_compress_fwd_split_cl(x, xn, xp, a, an, ap, n, c, p, w, b, y, yn, yp, parts, None)


def _dgrad(lib, parts, gy=D, gn=NSTR, gp=C, n=N, c=C, p=P, w=D, gx=D, gxn=NSTR, gxp=C, ga=D, gan=NSTR, gap=C):
    return lib.mrp_compress_bwd_data_split_cl(gy, gn, gp, n, c, p, w, gx, gxn, gxp, ga, gan, gap, parts, None)


def _wgrad(lib, parts, gy=D, gn=NSTR, gp=C, x=D, xn=NSTR, xp=C, a=D, an=NSTR, ap=C, n=N, c=C, p=P, gw=D, gb=None,
           ws=None, wsb=0):
    return lib.mrp_compress_bwd_weight_split_cl(gy, gn, gp, x, xn, xp, a, an, ap, n, c, p, gw, gb, ws, wsb, parts,
                                                None)


@pytest.fixture
def knob_off():
    """The A/B knob at 0: a call that passes every check answers hipErrorNotSupported instead of launching."""
    lib = m.load_library()
    assert lib.mrp_tuning_set(b"compress_split_cl", 0) == 0
    try:
        yield lib
    finally:
        assert lib.mrp_tuning_set(b"compress_split_cl", 1) == 0


def test_symbols_exported_and_abi_unchanged():
    lib = m.load_library()
    header = open(os.path.join(ROOT, "include", "mrp_gnn.h"), "rb").read()
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, s)
        assert s.encode() in header
    assert lib.mrp_abi_version() == _lib.ABI_VERSION == 22


@pytest.mark.parametrize("bad", [0, 4, -1, 7])
def test_parts_are_checked_before_everything_else(bad):
    lib = m.load_library()
    for call in (_fwd, _dgrad, _wgrad):
        assert call(lib, bad) == HIP_INVALID_VALUE
    # before the zero-size no-ops, the NULL checks and the declined shapes
    assert _fwd(lib, bad, n=0) == HIP_INVALID_VALUE
    assert _dgrad(lib, bad, c=0, gy=None) == HIP_INVALID_VALUE
    assert _wgrad(lib, bad, gw=None, gb=None) == HIP_INVALID_VALUE
    assert _fwd(lib, bad, c=40, xn=40 * P, xp=40, an=40 * P, ap=40, yn=40 * P, yp=40) == HIP_INVALID_VALUE


@pytest.mark.parametrize("parts", PARTS)
def test_null_pointers_with_work_are_invalid(parts):
    lib = m.load_library()
    for kw in (dict(x=None), dict(a=None), dict(w=None), dict(y=None)):
        assert _fwd(lib, parts, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gy=None), dict(w=None), dict(gx=None), dict(ga=None)):
        assert _dgrad(lib, parts, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gy=None), dict(x=None), dict(a=None), dict(gw=None, gb=D)):
        assert _wgrad(lib, parts, **kw) == HIP_INVALID_VALUE


@pytest.mark.parametrize("parts", PARTS)
def test_short_strides_and_misalignment_are_invalid(parts):
    lib = m.load_library()
    # pixel stride below C; node stride below P pixel strides (dense, and for a 2C buffer's half)
    for kw in (dict(xp=C - 4), dict(ap=C - 4), dict(yp=C - 4), dict(xn=NSTR - 4), dict(an=NSTR - 4),
               dict(yn=NSTR - 4), dict(xp=2 * C, xn=NSTR), dict(yp=2 * C, yn=2 * NSTR - 4)):
        assert _fwd(lib, parts, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gp=C - 4), dict(gxp=C - 4), dict(gap=C - 4), dict(gn=NSTR - 4), dict(gxn=NSTR - 4),
               dict(gan=NSTR - 4), dict(gap=2 * C, gan=NSTR)):
        assert _dgrad(lib, parts, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gp=C - 4), dict(xp=C - 4), dict(ap=C - 4), dict(gn=NSTR - 4), dict(xn=NSTR - 4),
               dict(an=NSTR - 4)):
        assert _wgrad(lib, parts, **kw) == HIP_INVALID_VALUE
    # pointers that are not 16-byte aligned; strides that are not whole 16-byte pieces (4 elements)
    for kw in (dict(x=ODD), dict(a=ODD), dict(w=ODD), dict(y=ODD), dict(xn=NSTR + 2), dict(yn=NSTR + 2),
               dict(xp=C + 2, xn=2 * NSTR), dict(yp=C + 2, yn=2 * NSTR)):
        assert _fwd(lib, parts, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gy=ODD), dict(w=ODD), dict(gx=ODD), dict(ga=ODD), dict(gan=NSTR + 2),
               dict(gxp=C + 2, gxn=2 * NSTR)):
        assert _dgrad(lib, parts, **kw) == HIP_INVALID_VALUE
    for kw in (dict(gy=ODD), dict(x=ODD), dict(a=ODD), dict(gw=ODD), dict(gn=NSTR + 2),
               dict(ap=C + 2, an=2 * NSTR)):
        assert _wgrad(lib, parts, **kw) == HIP_INVALID_VALUE
    # negative sizes
    assert _fwd(lib, parts, n=-1) == HIP_INVALID_VALUE
    assert _dgrad(lib, parts, c=-32) == HIP_INVALID_VALUE
    assert _wgrad(lib, parts, p=-64) == HIP_INVALID_VALUE


@pytest.mark.parametrize("parts", PARTS)
def test_strided_operands_are_accepted_up_to_the_launch(parts, knob_off):
    """Halves of a channels_last 2C buffer (pixel stride 2C), a batch slice (node stride > P ps) and strides
    that are multiples of 4 but not of 8 elements pass every check: with the A/B knob off the next answer is
    hipErrorNotSupported, not invalid-value."""
    lib = knob_off
    wide = dict(xp=2 * C, xn=2 * NSTR, ap=2 * C, an=4 * NSTR)
    assert _fwd(lib, parts, **wide) == NS
    assert _dgrad(lib, parts, gxp=2 * C, gxn=2 * NSTR, gap=2 * C, gan=2 * NSTR) == NS
    assert _wgrad(lib, parts, **wide) == NS
    assert _fwd(lib, parts, xp=C + 4, xn=(C + 4) * P + 4) == NS
    assert _fwd(lib, parts) == NS and _dgrad(lib, parts) == NS and _wgrad(lib, parts) == NS


@pytest.mark.parametrize("parts", PARTS)
def test_zero_sizes_are_noops(parts):
    lib = m.load_library()
    for kw in (dict(n=0), dict(c=0), dict(p=0)):
        assert _fwd(lib, parts, x=None, a=None, w=None, y=None, **kw) == 0
        assert _dgrad(lib, parts, gy=None, w=None, gx=None, ga=None, **kw) == 0
    assert _wgrad(lib, parts, c=0) == 0
    assert _wgrad(lib, parts, gw=None, gb=None) == 0  # nothing wanted
    assert _wgrad(lib, parts, n=0, gw=None, gb=None) == 0


@pytest.mark.parametrize("parts", PARTS)
def test_untiled_channel_counts_are_declined(parts):
    lib = m.load_library()
    c2 = 40  # C % 32 != 0 (strides kept whole 16-byte pieces)
    s = dict(c=c2)
    assert _fwd(lib, parts, xn=c2 * P, xp=c2, an=c2 * P, ap=c2, yn=c2 * P, yp=c2, **s) == NS
    assert _dgrad(lib, parts, gn=c2 * P, gp=c2, gxn=c2 * P, gxp=c2, gan=c2 * P, gap=c2, **s) == NS
    assert _wgrad(lib, parts, gn=c2 * P, gp=c2, xn=c2 * P, xp=c2, an=c2 * P, ap=c2, **s) == NS
    assert lib.mrp_compress_bwd_weight_split_cl_workspace(4, c2, P) == 0


def test_workspace_query_and_short_workspace():
    lib = m.load_library()
    ws = lib.mrp_compress_bwd_weight_split_cl_workspace
    assert ws(0, 32, 64) == 0 and ws(4, 32, 0) == 0 and ws(-1, 32, 64) == 0
    try:
        # a forced split count: [splits][C][2C] partial tiles + [splits][C] bias sums, fp32; K = 4096 is 128
        # stages; one split needs no workspace; more splits than stages are clamped (K = 49: 2 stages)
        prev = -1
        for forced in (1, 2, 3, 5, 8, 128):  # monotone in the forced count
            assert lib.mrp_tuning_set(b"split_cl_splits", forced) == 0
            got = ws(64, 64, 64)
            assert got == (0 if forced == 1 else forced * (64 * 128 + 64) * 4)
            assert got > prev
            prev = got
        assert lib.mrp_tuning_set(b"split_cl_splits", 256) == 0
        assert ws(1, 32, 49) == (2 * 32 * 64 + 2 * 32) * 4
        assert lib.mrp_tuning_set(b"split_cl_splits", 257) == HIP_INVALID_VALUE
        assert lib.mrp_tuning_set(b"split_cl_splits", 2) == 0
        for parts in PARTS:  # a too-small workspace is refused before the launch, for every part count
            assert _wgrad(lib, parts, ws=None, wsb=0) == HIP_INVALID_VALUE
            assert _wgrad(lib, parts, ws=D, wsb=16) == HIP_INVALID_VALUE
            assert _wgrad(lib, parts, ws=ODD, wsb=1 << 20) == HIP_INVALID_VALUE
    finally:
        assert lib.mrp_tuning_set(b"split_cl_splits", 0) == 0


def test_knobs_accepted_and_named_in_the_header():
    lib = m.load_library()
    header = open(os.path.join(ROOT, "include", "mrp_gnn.h"), "rb").read()
    for name, lo, hi in ((b"compress_split_cl", 0, 1), (b"split_cl_splits", 0, 256)):
        assert b'"' + name + b'"' in header
        assert lib.mrp_tuning_set(name, lo - 1) == HIP_INVALID_VALUE
        assert lib.mrp_tuning_set(name, hi + 1) == HIP_INVALID_VALUE
        assert lib.mrp_tuning_set(name, hi) == 0
    assert lib.mrp_tuning_set(b"compress_split_cl", 1) == 0 and lib.mrp_tuning_set(b"split_cl_splits", 0) == 0


def test_python_switch_defaults_to_convert():
    from mrp_gnn_amd import compress
    assert compress.channels_last_compress_fp32() == "convert"
    assert m.set_channels_last_compress_fp32 is compress.set_channels_last_compress_fp32
    assert m.channels_last_compress_fp32 is compress.channels_last_compress_fp32
    try:
        assert compress.set_channels_last_compress_fp32("native") == "convert"
        assert compress.channels_last_compress_fp32() == "native"
        for bad in ("on", "", None, "Native"):
            with pytest.raises(ValueError):
                compress.set_channels_last_compress_fp32(bad)
        assert compress.channels_last_compress_fp32() == "native"
    finally:
        assert compress.set_channels_last_compress_fp32("convert") == "native"
