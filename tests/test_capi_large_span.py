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
    # the four later families: both entry points of each, every dtype, every graph set, none declined
    assert set(sp.AGG_FAMILIES) == set(sp.AGG) == set(sp.AGG_S) | {"wide_3x8_c17_p80", "complete_1x16_s512"}
    assert sorted(sp.FAMILY_ENTRIES) == ["attn", "max", "wattn", "wmean"]
    for fam, entries in sp.FAMILY_ENTRIES.items():
        assert entries == (f"mrp_film_{fam}_fwd", f"mrp_film_{fam}_bwd")
        for entry in entries:
            rows = {(k, ca): v for (e, k, ca), v in sp.EXPECTED.items() if e == entry}
            assert rows == {(k, ca): 0 for k in sp.DTYPES for ca in sp.AGG_FAMILIES}, entry
    # the mean: the typed entry points on every graph set but the wide one, the pixel-major ones on AGG_CL_SPAN
    for entry, cases in (("mrp_film_mean_fwd_t", sp.AGG_S + ("complete_1x16_s512",)),
                         ("mrp_film_mean_fwd_cl", sp.AGG_CL_SPAN)):
        for e in (entry, entry.replace("fwd", "bwd")):
            assert {(k, ca) for (e2, k, ca) in sp.EXPECTED if e2 == e} == {(k, ca) for k in sp.DTYPES for ca in cases}


@pytest.mark.parametrize("case", sp.AGG_FAMILIES)
@pytest.mark.parametrize("es", [4, 2])
def test_aggregation_cases_cross_both_boundaries(case, es):
    """Every graph set the four families run has nodes beyond 2^31 and beyond 2^32 bytes of their tensor; the
    self-spanning case has them beyond both boundaries measured from its own graph's first node too (no other case
    has: a graph of at most 12 nodes S apart ends 2.75 GiB from its first), from node 4 and node 8 onward."""
    offs = sp.agg_node_offsets(case, es)
    assert len(offs) == sum(sp.AGG[case][0])
    in_tensor = [a for a, _ in offs]
    assert any(1 << 31 <= a < 1 << 32 for a in in_tensor) and any(a >= 1 << 32 for a in in_tensor)
    _, C, H, W = sp.AGG[case][1:5]
    assert in_tensor[-1] + (sp.MAX_SLOTS - 1) * sp.SLOT + C * H * W * es <= sp.WORK  # inside the working span
    in_graph = [b for _, b in offs]
    if case == "complete_1x16_s512":
        assert [i for i, b in enumerate(in_graph) if b >= 1 << 31][0] == 4
        assert [i for i, b in enumerate(in_graph) if b >= 1 << 32][0] == 8
    else:
        assert max(in_graph) < 1 << 32


MFMA_OPERANDS = ("grad_out", "grad_x", "base", "x")


@pytest.mark.parametrize("kind", ["complete", "knn4"])
@pytest.mark.parametrize("key", ["f32", "bf16"])
def test_matrix_core_backward_steps_aside_where_15_strides_do_not_fit(lib, key, kind):
    """film_bwd_mfma addresses a graph's 16 node rows by 32-bit per-lane byte offsets from the graph's first node, so
    its launcher takes it only where 15 node strides and a block's channel pair fit, for every strided operand it
    reads or writes: 15 s esz + (C P + P) esz < 2^32 (film_mean_bwd.hip).  s is computed here from that formula: the
    largest multiple of 4 elements that fits plans film_bwd_mfma, s + 4 plans a VALU kernel with a sound plan —
    through each operand by itself as well."""
    import geometry_cases as gc
    from mrp_gnn_amd import aggregate
    C, P, esz = 8, 64, gc.ELEM[key]
    g = gc.graph_ns(kind, (16, 16))
    s = ((1 << 32) - 1 - (C * P + P) * esz) // (15 * esz) // 4 * 4
    assert 15 * s * esz + (C * P + P) * esz < 1 << 32 <= 15 * (s + 4) * esz + (C * P + P) * esz

    def plan(**kw):
        return aggregate.launch_plan("bwd", g, C, P, dtype=gc.DTYPES[key], grad_x_base=True, **kw)

    fits = plan(stride=s)
    assert fits.kernel_name == "film_bwd_mfma" and gc.violations(fits, key, g, C, P, 16) == []
    other = plan(stride=s + 4)
    assert other.kernel_name == ("film_bwd_regular" if (kind, key) == ("knn4", "f32") else "film_bwd_dx_gram")
    assert gc.violations(other, key, g, C, P, 16) == [], gc.plan_tuple(other)
    assert gc.plan_tuple(other) == gc.plan_tuple(plan(stride=1 << 40))  # and stays there
    for name in MFMA_OPERANDS:  # one operand alone beyond the limit, the others dense
        assert plan(strides={name: s}).kernel_name == "film_bwd_mfma", name
        assert gc.plan_tuple(plan(strides={name: s + 4})) == gc.plan_tuple(other), name
    # an operand the call does not use does not count: x without grad_gb, the base and grad_x without grad_x
    assert plan(strides={"x": s + 4}, need_dgb=False).kernel_name == "film_bwd_mfma"
    assert aggregate.launch_plan("bwd", g, C, P, dtype=gc.DTYPES[key], strides={"base": s + 4}).kernel_name == \
        "film_bwd_mfma"
    assert plan(strides={"base": s + 4, "grad_x": s + 4}, need_dx=False).kernel_name == "film_bwd_mfma"


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
