"""CPU: the part-count entry points of the split-bf16 compress (``mrp_compress_fwd_split_p`` /
``_bwd_data_split_p`` / ``_bwd_weight_split_p``): exported and declared, and their argument validation and
no-op paths, which return before any launch (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import pytest

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib
from conftest import ROOT

HIP_INVALID_VALUE = 1
NS = _lib.HIP_ERROR_NOT_SUPPORTED
NAMES = ("mrp_compress_fwd_split_p", "mrp_compress_bwd_data_split_p", "mrp_compress_bwd_weight_split_p")
D = ctypes.c_void_p(16)  # a non-null, 16-byte aligned pointer that is never dereferenced on the host


def _fwd(lib, n, C, P, parts, ptr=None):
    return lib.mrp_compress_fwd_split_p(ptr, C * P, ptr, C * P, n, C, P, ptr, None, ptr, C * P, parts, None)


def _dgrad(lib, n, C, P, parts, ptr=None):
    return lib.mrp_compress_bwd_data_split_p(ptr, C * P, n, C, P, ptr, ptr, C * P, ptr, C * P, parts, None)


def _wgrad(lib, n, C, P, parts, ptr=None, gw=None):
    return lib.mrp_compress_bwd_weight_split_p(ptr, C * P, ptr, C * P, ptr, C * P, n, C, P, gw, None, None, 0, parts,
                                               None)


def test_symbols_exported_and_declared():
    lib = m.load_library()
    header = open(os.path.join(ROOT, "include", "mrp_gnn.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (mrp_\w+)$", out, re.M))
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name in exported
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert re.search(name + r"\([^;]*int32_t parts, void\* stream\);", header), name  # parts before stream
    assert "3.1 x 2^-18" in header and "2.01 x 2^-9" in header  # the error model
    assert lib.mrp_abi_version() == 22  # extended without a new number


@pytest.mark.parametrize("parts", [0, 4, -1])
def test_parts_out_of_range_is_invalid_before_anything_else(parts):
    lib = m.load_library()
    for call in (_fwd, _dgrad, _wgrad):
        assert call(lib, 2, 64, 64, parts, D) == HIP_INVALID_VALUE
        assert call(lib, 0, 64, 64, parts) == HIP_INVALID_VALUE  # even where the sizes alone would be a no-op
        assert call(lib, 2, 48, 64, parts, D) == HIP_INVALID_VALUE  # and where the shape alone would be declined


@pytest.mark.parametrize("parts", [1, 2, 3])
def test_zero_sizes_succeed_without_a_launch(parts):
    lib = m.load_library()
    for n, C, P in ((0, 64, 64), (2, 0, 64), (2, 64, 0)):
        assert _fwd(lib, n, C, P, parts) == 0
        assert _dgrad(lib, n, C, P, parts) == 0
    assert _wgrad(lib, 2, 0, 64, parts) == 0
    assert _wgrad(lib, 2, 64, 64, parts) == 0  # nothing wanted (gw and gbias NULL)
    for call in (_fwd, _dgrad, _wgrad):
        assert call(lib, -1, 64, 64, parts) == HIP_INVALID_VALUE


@pytest.mark.parametrize("parts", [1, 2, 3])
def test_declined_shapes_are_those_of_the_existing_entry_points(parts):
    lib = m.load_library()
    # C = 48 (C % 32) and P = 6 (P % 4): forward and data gradient; the weight gradient also P = 16 (P % 32)
    for n, C, P in ((2, 48, 64), (2, 64, 6)):
        assert _fwd(lib, n, C, P, parts, D) == NS
        assert _dgrad(lib, n, C, P, parts, D) == NS
        assert _wgrad(lib, n, C, P, parts, D, D) == NS
        assert lib.mrp_compress_fwd_split(D, C * P, D, C * P, n, C, P, D, None, D, C * P, None) == NS
        assert lib.mrp_compress_bwd_data_split(D, C * P, n, C, P, D, D, C * P, D, C * P, None) == NS
        assert lib.mrp_compress_bwd_weight_split(D, C * P, D, C * P, D, C * P, n, C, P, D, None, None, 0, None) == NS
    assert _wgrad(lib, 2, 64, 16, parts, D, D) == NS
    assert lib.mrp_compress_bwd_weight_split(D, 1024, D, 1024, D, 1024, 2, 64, 16, D, None, None, 0, None) == NS
    # tiled shapes with missing operands: invalid, as before
    assert _fwd(lib, 2, 64, 64, parts) == HIP_INVALID_VALUE
    assert _dgrad(lib, 2, 64, 64, parts) == HIP_INVALID_VALUE
    assert _wgrad(lib, 2, 64, 64, parts, None, D) == HIP_INVALID_VALUE
