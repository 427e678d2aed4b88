"""CPU: the aggregation's launch planner over the whole accepted range of every geometry knob.

``tools/sweep_geometry.py`` and its kin time the kernels at knob settings and the defaults in
``csrc/tuning.hpp`` came from such sweeps; no sweep checks a result.  Here every setting a knob accepts is
planned through ``mrp_film_mean_fwd_plan`` / ``mrp_film_mean_bwd_plan`` — the planner the launch path itself
calls, with no GPU call — and each plan is held to what the kernel it names requires
(``geometry_cases.violations``, each requirement beside the kernel source it comes from).  test_gpu_geometry.py
then launches a table of such plans (``geometry_cases.ROWS``) against float64; the tests at the end of this
file keep that table honest: every row reaches the kernel and geometry it names, and its knobs move the plan.

What the enumeration found when it was written, and the planner now prevents (film_mean_bwd.hip):

* ``bwd_regular_lanes`` = 33..64 with 1-element slices planned 128 lanes per plane for film_bwd_regular, which
  reduces over one wave and stores from lane 0 alone: the second wave's Gram partial was dropped.  Capped at 64.
* ``bwd_fused_cap`` = 64 with logits on complete 8-node graphs and 4 lanes per plane asked for 70,688 bytes of
  dynamic LDS, above the 64 KiB no launcher raises.  The channels per workgroup are halved until it fits.
* at default knobs, the Gram pass of complete 16-node graphs with logits and >= 16 channels on a plane
  film_bwd_mfma does not take asked for 67,392 bytes.  The same halving.

``fwd_hi`` / ``fwd_regular_hi`` above 64 are sound: no lane of film_fwd / film_fwd_regular reads another's values.

``film_max_fwd`` and ``film_wmean_fwd`` call the same ``make_geometry`` with film_fwd's knobs and have no plan query:
``geometry_cases.make_geometry`` mirrors it (pinned to the source text, and held equal to the plan query's film_fwd
plans over the knobs' ranges), and the hand-written geometries of ``geometry_cases.FWD_ROWS`` are held to the mirror.

Also here: ``tile_of`` and ``xcd_remap`` (gemm_common.hpp), the GEMMs' workgroup -> tile order behind the
``gemm_group`` / ``nt_group`` knobs, restated in Python (pinned to the source text) and checked by brute force
to be bijections.
"""
import itertools
import os
import re

import numpy as np
import pytest

from mrp_gnn_amd import aggregate
import geometry_cases as gc

RANGES = gc.knob_ranges()
KEYS = ("f32", "bf16", "f16")
KINDS = ("complete", "csr", "knn1", "knn4", "knn5", "knn8")
MAX_NODES = (1, 2, 8, 9, 12, 16)
CS = (1, 3, 16, 17, 40, 64, 100)
PS = (1, 4, 6, 16, 28, 64, 144, 256, 1024)
ALIGNS = (16, 8, 4, 2)


def graphs(kind, n):
    """Two graphs of n nodes (for the kinds that allow it, the second one node short)."""
    return gc.graph_ns(kind, (n, n) if kind == "complete" or n == 1 else (n, n - 1))


def check(direction, key, kind, n, C, P, align, found, **kw):
    """Plan one call and collect what the plan breaks."""
    if align % gc.ELEM[key]:
        return None  # a pointer no tensor of this dtype can have
    g = graphs(kind, n)
    p = aggregate.launch_plan(direction, g, C, P, dtype=gc.DTYPES[key], align=align, **kw)
    assert p.kernel != 0
    bad = gc.violations(p, key, g, C, P, align)
    if bad:
        found.append((direction, key, kind, n, C, P, align, kw, gc.plan_tuple(p), bad))
    return p


def report(found):
    assert not found, f"{len(found)} plans break a kernel's requirements, the first: {found[:5]}"


def test_knob_table_is_the_one_the_issue_lists():
    """The geometry knobs and their accepted ranges, as ``mrp_tuning_set`` has them."""
    want = {"fwd_lo": (1, 256), "fwd_hi": (1, 256), "fwd_cap": (1, 16), "fwd_vec2_below": (0, 1 << 20),
            "fwd_regular_split": (0, 1), "fwd_regular_lo": (1, 256), "fwd_regular_hi": (1, 256),
            "fwd_regular_cap": (1, 16), "bwd_fused_lo": (1, 256), "bwd_fused_hi": (1, 256), "bwd_fused_cap": (1, 64),
            "bwd_pre2": (0, 2), "bwd_regular_vec": (1, 2), "bwd_regular_lanes": (1, 64), "bwd_mfma_cpw": (1, 2)}
    assert {k: RANGES[k] for k in want} == want
    assert len(RANGES) == 33


# every shape, dtype, alignment and graph kind: at the defaults, and with every geometry knob at the end of
# its range that asks the most of a kernel (the widest planes, the most channels, the lab-only paths)
EXTREME = dict(fwd_hi=256, fwd_lo=256, fwd_regular_hi=256, fwd_regular_lo=256, fwd_regular_split=1, fwd_vec2_below=1 << 20,
               bwd_fused_hi=256, bwd_fused_lo=256, bwd_fused_cap=64, bwd_pre2=1, bwd_regular_vec=1, bwd_regular_lanes=64,
               bwd_mfma_cpw=1)
SMALLEST = dict(fwd_hi=1, fwd_lo=1, fwd_cap=1, fwd_regular_hi=1, fwd_regular_lo=1, fwd_regular_cap=1, bwd_fused_hi=1,
                bwd_fused_lo=1, bwd_fused_cap=1, bwd_pre2=0, bwd_regular_lanes=1, bwd_regular_mfma=0, bwd_complete_mfma=0)


@pytest.mark.parametrize("setting", [{}, EXTREME, SMALLEST], ids=["defaults", "extreme", "smallest"])
def test_every_shape(setting):
    found = []
    with gc.knobs(**setting):
        for key, kind, n, C, P, align in itertools.product(KEYS, KINDS, MAX_NODES, CS, PS, ALIGNS):
            check("fwd", key, kind, n, C, P, align, found)
            for base, logits in ((False, False), (True, True)):
                check("bwd", key, kind, n, C, P, align, found, grad_x_base=base, logits=logits)
    report(found)


def lo_hi_pairs():
    """Each of lo and hi over its whole range 1..256 against the other at its ends and in the middle: lo > hi,
    lo == hi, and no powers of two among them."""
    pairs = {(lo, hi) for lo in range(1, 257) for hi in (1, 3, 64, 256)}
    pairs |= {(lo, hi) for hi in range(1, 257) for lo in (1, 16, 100, 256)}
    return sorted(pairs)


# (dtype, alignment): every slice width a forward or backward kernel has
WIDTHS = (("f32", 16), ("f32", 4), ("bf16", 16), ("bf16", 8), ("f16", 2))


@pytest.mark.parametrize("family, direction, kind, n", [
    ("fwd", "fwd", "complete", 8), ("fwd_regular", "fwd", "knn5", 16), ("bwd_fused", "bwd", "complete", 8)])
def test_lo_hi_over_their_whole_range(family, direction, kind, n):
    assert RANGES[family + "_lo"] == RANGES[family + "_hi"] == (1, 256)
    found = []
    extra = [{}]
    if family == "fwd":
        extra = [{}, dict(fwd_vec2_below=1 << 20)]
    elif family == "fwd_regular":
        extra = [{}, dict(fwd_regular_split=1)]
    elif family == "bwd_fused":
        extra = [dict(bwd_pre2=1), dict(bwd_fused_cap=64, bwd_pre2=2)]
    for lo, hi in lo_hi_pairs():
        for more in extra:
            with gc.knobs(**{family + "_lo": lo, family + "_hi": hi}, **more):
                for (key, align), P in itertools.product(WIDTHS[:3], PS):
                    if direction == "fwd":
                        check("fwd", key, kind, n, 100, P, align, found)
                    else:
                        check("bwd", key, kind, n, 100, P, align, found, logits=True)
    report(found)


@pytest.mark.parametrize("family, direction, kinds", [("fwd", "fwd", ("complete", "csr")),
                                                      ("fwd_regular", "fwd", ("knn1", "knn8")),
                                                      ("bwd_fused", "bwd", ("complete", "csr"))])
def test_cap_over_its_whole_range(family, direction, kinds):
    """Channels per workgroup: the whole range of the cap, every C, at lanes per plane from 1 to 256."""
    lo, hi = RANGES[family + "_cap"]
    found = []
    for cap, lanes in itertools.product(range(lo, hi + 1), (4, 256) if direction == "bwd" else (1, 4, 64, 256)):
        with gc.knobs(**{family + "_cap": cap, family + "_lo": lanes, family + "_hi": lanes}):
            for kind, n, C, P, (key, align) in itertools.product(kinds, (2, 8) if direction == "bwd" else (1, 8, 16), CS, PS,
                                                                 (WIDTHS[0], WIDTHS[3])):
                if direction == "fwd":
                    check("fwd", key, kind, n, C, P, align, found)
                else:
                    for logits in (False, True):
                        check("bwd", key, kind, n, C, P, align, found, logits=logits, grad_x_base=logits)
    report(found)


def test_bwd_regular_vec_and_lanes_over_their_whole_range():
    found = []
    lo, hi = RANGES["bwd_regular_lanes"]
    assert RANGES["bwd_regular_vec"] == (1, 2)
    for vec, lanes, mfma in itertools.product((1, 2), range(lo, hi + 1), (0, 1)):
        with gc.knobs(bwd_regular_vec=vec, bwd_regular_lanes=lanes, bwd_regular_mfma=mfma):
            for kind, n, C, P, align in itertools.product(("knn1", "knn4", "knn5", "knn8"), (9, 12, 16), (3, 17, 100), PS,
                                                          (16, 8, 4)):
                p = check("bwd", "f32", kind, n, C, P, align, found, grad_x_base=bool(lanes & 1))
                assert p.kernel_name in ("film_bwd_regular", "film_bwd_mfma")
    report(found)


def test_the_remaining_geometry_knobs():
    """bwd_pre2, bwd_mfma_cpw, fwd_vec2_below and fwd_regular_split over every value (fwd_vec2_below: the ends and
    each side of every plane size), on every shape that reaches their kernels."""
    found = []
    settings = [dict(bwd_pre2=v) for v in (0, 1, 2)] + [dict(bwd_mfma_cpw=v) for v in (1, 2)]
    settings += [dict(fwd_regular_split=v) for v in (0, 1)]
    settings += [dict(fwd_vec2_below=v) for v in sorted({0, 1 << 20} | {p + d for p in PS for d in (0, 1)})]
    for s in settings:
        with gc.knobs(**s):
            for kind, n, C, P, align in itertools.product(KINDS, MAX_NODES, (3, 17, 100), PS, (16, 8, 4)):
                if "fwd_vec2_below" in s or "fwd_regular_split" in s:
                    check("fwd", "f32", kind, n, C, P, align, found)
                else:
                    for key in ("f32", "f16"):
                        for base in (False, True):
                            check("bwd", key, kind, n, C, P, align, found, grad_x_base=base, logits=base)
    report(found)


def test_plans_agree_with_validation_and_empty_calls():
    """The query returns what the entry points return before launching: an error for arguments they reject,
    success and kernel 'none' where they have nothing to launch."""
    import ctypes
    from mrp_gnn_amd import _lib
    lib = _lib.load_library()
    plan = _lib.AggPlan()
    a = ctypes.c_void_p(1 << 20)
    ok = (0, a, 64, a, a, a, a, a, 2, 4, _lib.GRAPH_COMPLETE, 8, 24, 4, 16, 0, a, 64, None)
    assert lib.mrp_film_mean_fwd_plan(*ok, ctypes.byref(plan)) == 0 and plan.kernel_name == "film_fwd"
    assert lib.mrp_film_mean_fwd_plan(*ok, None) == 1  # no plan to fill
    assert lib.mrp_film_mean_fwd_plan(3, *ok[1:], ctypes.byref(plan)) == 1  # unknown dtype
    short = ok[:2] + (63,) + ok[3:]
    assert lib.mrp_film_mean_fwd_plan(*short, ctypes.byref(plan)) == 1  # node stride < C P
    empty = ok[:13] + (0,) + ok[14:]  # C = 0
    assert lib.mrp_film_mean_fwd_plan(*empty, ctypes.byref(plan)) == 0 and plan.kernel_name == "none"
    g = gc.graph_ns("complete", (4, 4))
    p = aggregate.launch_plan("bwd", g, 4, 16, need_dx=False, need_dgb=False)
    assert p.kernel_name == "none" and gc.plan_tuple(p)[1:] == (0,) * 9
    p = aggregate.launch_plan("bwd", g, 4, 16, mode="copy_mean", need_dx=False)  # grad_gb only cleared
    assert p.kernel_name == "none"
    g16 = gc.graph_ns("complete", (16, 16))
    only_dx = aggregate.launch_plan("bwd", g16, 17, 16, logits=True, need_dgb=False)
    both = aggregate.launch_plan("bwd", g16, 17, 16, logits=True)
    # film_bwd_dx alone keeps its 16 channels; with the Gram pass's sigmoid values both run 8
    assert (only_dx.cpb, both.cpb) == (16, 8) and only_dx.lds_bytes < both.lds_bytes <= gc.MAX_LDS


# ------------------------------------------------------------------------------------------- the GPU table
def row_plan(row, direction, knobs_):
    g = gc.graph_ns(row.kind, row.ns)
    with gc.knobs(**knobs_):
        return aggregate.launch_plan(direction, g, row.C, row.H * row.W, dtype=gc.DTYPES[row.key], mode=row.mode,
                                     logits=row.logits, grad_x_base=row.base, x0=row.epi, xcopy=row.epi), g


@pytest.mark.parametrize("row", gc.ROWS, ids=[r.name for r in gc.ROWS])
def test_row_reaches_what_it_names_and_moves_the_plan(row):
    assert len(row.ns) == 2 and all(k in RANGES for k in row.knobs)
    assert row.fwd or row.bwd
    moved = False
    for direction, want in (("fwd", row.fwd), ("bwd", row.bwd)):
        p, g = row_plan(row, direction, row.knobs)
        assert gc.violations(p, row.key, g, row.C, row.H * row.W, 16) == [], (direction, gc.plan_tuple(p))
        if want is None:
            continue
        got = (p.kernel_name, p.vec, p.lpc, p.cpb) + ((p.pre2,) if len(want) == 5 else ())
        assert got == tuple(want), (direction, gc.plan_tuple(p))
        if p.kernel_name != "film_bwd_mfma":  # more than one channel block, the last one ragged
            assert p.ncb >= 2 and (p.cpb == 1 or row.C % p.cpb), (row.C, p.cpb)
        other, _ = row_plan(row, direction, row.versus)
        moved = moved or gc.plan_tuple(other) != gc.plan_tuple(p)
    # a row whose knobs leave the plan where it was has no teeth (d01: the default plan is its subject)
    assert moved or not row.knobs, "the row's knobs change nothing"


def test_table_covers_what_it_must():
    """Every value the table has to hold for each knob is in some row."""
    def values(*names):
        return {tuple(r.knobs[n] for n in names) for r in gc.ROWS if all(n in r.knobs for n in names)}
    assert values("fwd_lo", "fwd_hi") >= {(1, 1), (4, 4), (64, 64), (128, 128), (256, 256), (64, 4), (3, 100)}
    assert values("fwd_cap") >= {(1,), (3,), (16,)} and values("fwd_vec2_below") >= {(0,), (1 << 20,)}
    assert values("fwd_regular_split", "fwd_regular_lo", "fwd_regular_hi", "fwd_regular_cap") >= {
        (s, l, l, c) for s, l, c in itertools.product((0, 1), (8, 32, 64), (1, 4, 16))}
    assert values("bwd_fused_lo", "bwd_fused_hi") >= {(1, 1), (4, 4), (8, 128), (128, 128), (256, 256)}
    assert values("bwd_fused_cap") >= {(1,), (3,), (16,), (32,), (64,)} and values("bwd_pre2") >= {(0,), (1,), (2,)}
    # film_bwd_regular: vec x lanes at k = 4 and k = 5, each on 12x12 and on 16x16 with bwd_regular_mfma = 0
    regular = {(int(r.kind[3:]), r.knobs["bwd_regular_vec"], r.knobs["bwd_regular_lanes"], r.H,
                r.knobs.get("bwd_regular_mfma", 1), max(r.ns))
               for r in gc.ROWS if r.bwd and r.bwd[0] == "film_bwd_regular" and r.H == r.W}
    assert {t[:5] for t in regular} >= {(k, v, l, h, int(h == 12)) for k, v, l, h in itertools.product(
        (4, 5), (1, 2), (1, 8, 16, 24, 32, 64), (12, 16))}
    assert {t[5] for t in regular} == {9, 12, 16}
    assert values("bwd_mfma_cpw") == {(1,), (2,)}
    assert {r.mode for r in gc.ROWS if r.fwd} == {"film_mean", "film_sum", "copy_mean"}
    assert {max(r.ns) for r in gc.ROWS if r.fwd and r.fwd[0] == "film_fwd"} >= {1, 5, 8, 16}
    assert {r.kind for r in gc.ROWS if r.fwd and r.fwd[0] == "film_fwd_regular"} == {"knn1", "knn4", "knn5", "knn8"}


# ------------------------------------------------ film_max_fwd / film_wmean_fwd: the planner's mirror, the rows
def _source(name):
    return " ".join(open(os.path.join(gc.CSRC, name)).read().split())


def test_make_geometry_mirror_is_the_source():
    """The lines ``geometry_cases.make_geometry`` restates, in order, inside the planner; the two launchers' calls
    of it, their slice widths and plane splits as ``forward_geometry`` quotes them; the knobs' defaults."""
    text = _source("film_mean_kernels.hpp")
    body = text[text.index("inline Geometry make_geometry(int C, int P, int vec, int lo, int hi, int max_cpb) {"):]
    body = body[:body.index("return g;")]
    at = 0
    for line in gc.MAKE_GEOMETRY_SOURCE:
        assert line in body[at:], line
        at = body.index(line, at) + len(line)
    assert f"constexpr int kBlock = {gc.KBLOCK};" in text
    assert "int fwd_lo = 16, fwd_hi = 64, fwd_cap = 16;" in _source("tuning.hpp")
    call = "Geometry g = make_geometry(C, P, vec, tu.fwd_lo, tu.fwd_hi, tu.fwd_cap);"
    split = "g.psplit = graph_kind == MRP_GRAPH_COMPLETE ? (pv + g.lpc - 1) / g.lpc : 1;"
    fmax, fwmean = _source("film_max_fwd.hip"), _source("film_wmean_fwd.hip")
    assert call in fmax and call in fwmean and split in fmax and split in fwmean
    assert "int vec = 1; if (elem == 2 && max_nodes <= 8 && sc.ok(8, elem)) vec = 8; else if (sc.ok(4, elem)) vec = 4;" \
        in fmax
    assert "const int vec = sc.ok(4, elem) && aligned16(w) && w_node_stride % 4 == 0 ? 4 : 1;" in fwmean


def _film_fwd_planner():
    """plan(C, P, graphs) -> (vec, lpc, cpb, threads, ncb, psplit, grid) of film_fwd for fp32 features on dense
    16-byte aligned tensors, straight from mrp_film_mean_fwd_plan (made-up pointers: it makes no GPU call)."""
    import ctypes
    from mrp_gnn_amd import _lib
    lib = _lib.load_library()
    plan = _lib.AggPlan()
    ref = ctypes.byref(plan)
    a = ctypes.c_void_p(1 << 20)

    def run(C, P, g):
        code = lib.mrp_film_mean_fwd_plan(0, a, C * P, a, a, a, a, a, g.num_graphs, g.max_nodes, g.graph_kind,
                                          g.num_nodes, g.num_edges, C, P, 0, a, C * P, None, ref)
        assert code == 0 and plan.kernel_name == "film_fwd"
        return plan.vec, plan.lpc, plan.cpb, plan.threads, plan.ncb, plan.psplit, plan.grid
    return lib, run


def test_make_geometry_mirror_is_the_planner():
    """``geometry_cases.make_geometry`` against what the plan query reports for film_fwd — the same
    ``make_geometry(C, P, vec, tu.fwd_lo, tu.fwd_hi, tu.fwd_cap)`` call the two launchers make — for fp32 CSR graphs
    with ``fwd_vec2_below`` 0, at every shape of ``FWD_ROWS``: fwd_cap over its whole range against each of fwd_lo
    and fwd_hi over its whole range (the other at its ends and in between: ``lo_hi_pairs``), and the whole
    fwd_lo x fwd_hi product at the default cap."""
    assert RANGES["fwd_lo"] == RANGES["fwd_hi"] == (1, 256) and RANGES["fwd_cap"] == (1, 16)
    shapes = sorted({(r.C, r.H * r.W, max(r.ns)) for r in gc.FWD_ROWS})
    graphs_ = {n: gc.graph_ns("csr", (n, max(n - 1, 1))) for _, _, n in shapes}
    lib, plan = _film_fwd_planner()
    settings = [(lo, hi, cap) for lo, hi in lo_hi_pairs() for cap in range(1, 17)]
    settings += [(lo, hi, 16) for lo in range(1, 257) for hi in range(1, 257)]
    try:
        assert lib.mrp_tuning_set(b"reset", 0) == 0 and lib.mrp_tuning_set(b"fwd_vec2_below", 0) == 0
        for lo, hi, cap in settings:
            assert lib.mrp_tuning_set(b"fwd_lo", lo) == lib.mrp_tuning_set(b"fwd_hi", hi) == \
                lib.mrp_tuning_set(b"fwd_cap", cap) == 0
            for C, P, n in shapes:
                vec = 4 if P % 4 == 0 else 1
                lpc, cpb, threads, ncb = gc.make_geometry(C, P, vec, lo, hi, cap)
                want = (vec, lpc, cpb, threads, ncb, 1, 2 * ncb)
                assert plan(C, P, graphs_[n]) == want, (lo, hi, cap, C, P, n)
    finally:
        assert lib.mrp_tuning_set(b"reset", 0) == 0


@pytest.mark.parametrize("row", gc.FWD_ROWS, ids=[r.name for r in gc.FWD_ROWS])
def test_forward_row_names_the_geometry_its_knobs_reach(row):
    assert set(row.knobs) <= {"fwd_lo", "fwd_hi", "fwd_cap"} and row.knobs and len(row.ns) == 2
    kn = {k[4:]: v for k, v in row.knobs.items()}
    assert tuple(row.geo) == gc.forward_geometry(row, **kn), gc.forward_geometry(row, **kn)
    assert tuple(row.geo) != gc.forward_geometry(row), "the row's knobs change nothing"
    vec, lpc, cpb, psplit = row.geo
    assert (row.H * row.W) % vec == 0 and cpb * lpc <= gc.KBLOCK
    assert row.C % cpb or cpb == 1  # the last channel block is ragged
    if row.kind == "complete":
        assert len(set(row.ns)) == 1
    else:
        assert row.ns[1] < row.ns[0] and psplit == 1


@pytest.mark.parametrize("family", ["max", "wmean"])
def test_forward_rows_cover_what_they_must(family):
    rows = [r for r in gc.FWD_ROWS if r.family == family]
    assert len(rows) >= 12
    assert {r.geo[1] for r in rows} >= {1, 2, 4, 64, 128, 256}
    assert any(r.geo[1] == 256 and (r.H, r.W, r.key) == (32, 32, "f32") for r in rows)
    assert {r.knobs.get("fwd_cap") for r in rows} >= {1, 3, 16}
    assert any(r.C % r.geo[2] for r in rows if "fwd_cap" in r.knobs)
    assert any(r.knobs.get("fwd_lo", 0) > r.knobs.get("fwd_hi", 256) for r in rows)
    assert any((r.knobs.get("fwd_lo"), r.knobs.get("fwd_hi")) == (3, 100) for r in rows)
    assert {4 if max(r.ns) <= 4 else 8 if max(r.ns) <= 8 else 16 for r in rows} == {4, 8, 16}  # "max_bucket"
    # a complete graph's plane split with a ragged last segment; CSR and k-NN rows whose lanes walk several slices
    assert any(r.kind == "complete" and r.geo[3] > 1 and (r.H * r.W // r.geo[0]) % r.geo[1] for r in rows)
    for kind in ("csr", "knn4"):
        assert any(r.kind == kind and r.H * r.W // r.geo[0] >= 2 * r.geo[1] for r in rows)
    assert any(r.geo[0] == 1 and (r.H, r.W) == (5, 5) for r in rows)
    assert {r.key for r in rows} == {"f32", "bf16", "f16"}
    if family == "wmean":
        assert {r.mode for r in rows} == {"mean", "sum"}
        assert any(r.w_odd and r.geo[0] == 1 and (r.H * r.W) % 4 == 0 for r in rows)
    else:
        assert any(r.geo[0] == 8 for r in rows)


# ------------------------------------------------------------------- the GEMMs' workgroup -> tile order
def c_function(name):
    """The statements of a function of gemm_common.hpp, whitespace squeezed."""
    text = open(os.path.join(gc.CSRC, "gemm_common.hpp")).read()
    body = re.search(r"\b%s\([^)]*\) \{\n(.*?)\n\}" % name, text, re.S).group(1)
    return [" ".join(s.split()) for s in body.split(";") if s.strip()]


def tile_of(t, mtiles, ntiles, group):
    """gemm_common.hpp ``tile_of``, statement for statement (``test_restatements_are_the_source`` pins them), for
    an array of workgroup ids t."""
    gmax = group if 0 < group < mtiles else mtiles
    run = gmax * ntiles
    g = t // run
    first = g * gmax
    gm = np.where(mtiles - first < gmax, mtiles - first, gmax)
    rem = t - g * run
    return first + rem % gm, rem // gm


def xcd_remap(orig, nwg):
    """gemm_common.hpp ``xcd_remap``."""
    q, r, xcd = nwg // 8, nwg % 8, orig % 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + orig // 8


def test_restatements_are_the_source():
    """The C++ the two functions above restate; a change to either has to be made in both places."""
    assert c_function("tile_of") == [
        "const int gmax = group > 0 && group < mtiles ? group : mtiles",
        "const int run = gmax * ntiles",
        "const int g = t / run, first = g * gmax",
        "const int gm = mtiles - first < gmax ? mtiles - first : gmax",
        "const int rem = t - g * run",
        "mt = first + rem % gm",
        "nt = rem / gm"]
    assert c_function("xcd_remap") == [
        "const int q = nwg / 8, r = nwg % 8, xcd = orig % 8",
        "return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / 8"]


def test_tile_of_is_a_bijection_onto_the_grid():
    for mtiles, ntiles, group in itertools.product(range(1, 21), range(1, 41), range(0, 65)):
        mt, nt = tile_of(np.arange(mtiles * ntiles), mtiles, ntiles, group)
        assert mt.min() >= 0 and mt.max() < mtiles and nt.min() >= 0 and nt.max() < ntiles, (mtiles, ntiles, group)
        assert np.array_equal(np.sort(mt * ntiles + nt), np.arange(mtiles * ntiles)), (mtiles, ntiles, group)


def test_xcd_remap_is_a_bijection():
    for nwg in range(1, 301):
        assert sorted(xcd_remap(o, nwg) for o in range(nwg)) == list(range(nwg)), nwg
