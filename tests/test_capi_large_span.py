"""CPU: the declining rows of ``span_cases.EXPECTED`` — the return codes of the entry points on operands that
span more than 2 and 4 GiB (``tests/test_gpu_large_span.py`` runs the whole table on the GPU).  The library
decides every decline on the host before it enqueues anything and never dereferences on the host, so these
rows are asserted with made-up, suitably aligned pointer values and no GPU; the same table object drives
both files."""
import ctypes

import pytest

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib
import span_cases as sp

BASE = 1 << 40  # never dereferenced on the host
SLOT = 1 << 20


def _ptr(slot):
    return ctypes.c_void_p(BASE + slot * SLOT)


def _call(lib, entry, key, case, n=None, out_stride=None):
    nodes, C, H, W = sp.COMPRESS[case]
    n = nodes if n is None else n
    P, dt = H * W, sp.ENUM[key]
    s = sp.NODE_STRIDE // 2  # elements of a 16-bit type
    so = s if out_stride is None else out_stride
    if entry == "mrp_compress_fwd_t":
        return lib.mrp_compress_fwd_t(dt, _ptr(0), s, _ptr(1), s, n, C, P, _ptr(2), None, _ptr(3), so, None)
    if entry == "mrp_compress_bwd_data_t":
        return lib.mrp_compress_bwd_data_t(dt, _ptr(0), s, n, C, P, _ptr(2), _ptr(3), so, _ptr(4), so, None)
    raise AssertionError(f"no host-side call written for {entry}")


def test_table_names_known_entry_points_and_cases():
    assert sp.NS == _lib.HIP_ERROR_NOT_SUPPORTED
    for (entry, key, case), code in sp.EXPECTED.items():
        assert entry in _lib.EXPORTED_SYMBOLS and key in sp.DTYPES and code in (0, sp.NS)
        assert case in sp.COMPRESS or case in sp.AGG or case in sp.ENCODER
    assert sp.declining(), "the table has no declining row"


@pytest.fixture
def lib():
    """The library with every knob at its default: with ``compress_half`` 0 the typed entry points decline
    every shape, and each assertion below would hold for the wrong reason.  (That the same entry points
    accept what lies inside the limit is the GPU file's 7- and 8-node cases: an accepted call launches.)"""
    lib = m.load_library()
    assert lib.mrp_tuning_set(b"reset", 0) == 0
    return lib


@pytest.mark.parametrize("entry,key,case", sp.declining())
def test_declining_rows(lib, entry, key, case):
    assert _call(lib, entry, key, case) == sp.NS


@pytest.mark.parametrize("entry", ["mrp_compress_fwd_t", "mrp_compress_bwd_data_t"])
@pytest.mark.parametrize("key", ["bf16", "f16"])
def test_the_limit_is_the_outputs_node_range(lib, entry, key):
    """The header's limit: (nodes - 1) output node strides + C P elements of 2 bytes reach 2^31 bytes.  With
    S = 2^28 bytes + 64 KiB that is 9 nodes (8 S > 2^31 > 7 S + a block), and for 18 nodes the smallest
    output stride (in whole 16-byte pieces) whose node range reaches 2^31 bytes.  (The accepted side of either
    boundary would launch: the GPU file's 7-node case.)"""
    assert _call(lib, entry, key, "n18_c32_p32", n=9) == sp.NS
    _, C, H, W = sp.COMPRESS["n18_c32_p32"]
    per_stride = -(-((1 << 30) - C * H * W) // 17)  # 17 strides + C P >= 2^30 elements
    first_too_wide = -(-per_stride // 8) * 8
    assert (17 * first_too_wide + C * H * W) * 2 >= 1 << 31 > (17 * (first_too_wide - 8) + C * H * W) * 2
    assert _call(lib, entry, key, "n18_c32_p32", out_stride=first_too_wide) == sp.NS


#: (C, P, output node stride in elements): this file's stride, a dense 2 GiB-per-node output, strides just
#: below and above a power of two, a block-sized stride
SPAN_NODES = [(32, 32, sp.NODE_STRIDE // 2), (32, 32, 1 << 30), (64, 64, (1 << 20) - 8), (256, 1024, 256 * 1024),
              (32, 32, (1 << 27) + 8), (32, 8, 1 << 29)]


@pytest.mark.parametrize("entry", ["mrp_compress_fwd_t", "mrp_compress_bwd_data_t"])
@pytest.mark.parametrize("C,P,stride", SPAN_NODES)
def test_python_node_ranges_match_the_librarys_limit(lib, entry, C, P, stride):
    """``compress._span_nodes`` — the nodes per call of ``compress_forward`` / ``compress_backward_data`` on
    16-bit features — is the most the library takes: k nodes lie inside the header's limit by its formula,
    and the library declines k + 1 (asked on the host; a call of k nodes would launch)."""
    from mrp_gnn_amd import compress
    k = compress._span_nodes(1 << 20, C, P, stride, C * P)
    assert k >= 1 and ((k - 1) * stride + C * P) * 2 < 1 << 31 <= (k * stride + C * P) * 2
    assert compress._span_nodes(k, C, P, stride) == k and compress._span_nodes(3, C, P, C * P) == 3
    dt = sp.ENUM["bf16"]
    if entry == "mrp_compress_fwd_t":
        code = lib.mrp_compress_fwd_t(dt, _ptr(0), C * P, _ptr(1), C * P, k + 1, C, P, _ptr(2), None, _ptr(3), stride,
                                      None)
    else:
        code = lib.mrp_compress_bwd_data_t(dt, _ptr(0), C * P, k + 1, C, P, _ptr(2), _ptr(3), C * P, _ptr(4), stride,
                                           None)
    assert code == sp.NS
