"""Shared by test_geometry_cpu.py and test_gpu_geometry.py: the tuning knobs' accepted ranges (read from the
table in ``mrp_tuning_set``), a context manager that sets knobs and restores every default, what the
aggregation kernels require of a launch plan (``violations``: each requirement beside the line of kernel
source it comes from), the table of GPU cases (``ROWS``), and — for ``film_max_fwd`` and ``film_wmean_fwd``, which
are sized by film_fwd's knobs but have no plan query — a mirror of the planner's ``make_geometry`` with a table of
their own (``FWD_ROWS``).

A launch plan is what ``mrp_film_mean_fwd_plan`` / ``mrp_film_mean_bwd_plan`` report (``aggregate.launch_plan``):
the launchers act on the very same planner, so a plan that holds every requirement here is a launch that
does.  The plan query makes no GPU call: everything in this module but ``ROWS``' use runs without a GPU.
"""
import collections
import os
import re
import types

import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib
from conftest import ROOT

CSRC = os.path.join(ROOT, "multi-robot-perception-gnn-1_amd", "csrc")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ELEM = {"f32": 4, "bf16": 2, "f16": 2}


def knob_ranges():
    """name -> (lo, hi) from the ``knobs[]`` table of ``mrp_tuning_set`` (film_mean_fwd.hip)."""
    text = open(os.path.join(CSRC, "film_mean_fwd.hip")).read()
    rows = re.findall(r'\{"(\w+)", &t\.(\w+), (-?\d+), (\d+(?: << \d+)?)\}', text)
    assert rows and all(a == b for a, b, _, _ in rows)
    def value(text):  # an integer or "1 << 20"
        base, _, shift = text.partition(" << ")
        return int(base) << int(shift or 0)
    return {a: (int(lo), value(hi)) for a, _, lo, hi in rows}


class knobs:
    """``with knobs(fwd_lo=4, fwd_hi=4):`` sets tuning knobs; every default is restored on the way out."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        lib = m.load_library()
        for k, v in self.kw.items():
            assert lib.mrp_tuning_set(k.encode(), v) == 0, (k, v)
        return self

    def __exit__(self, *exc):
        assert m.load_library().mrp_tuning_set(b"reset", 0) == 0


def graph_ns(kind, ns):
    """The graph arguments (what ``launch_plan`` reads of a ``GraphCSR``) of a batch of graphs with ``ns`` nodes
    each: kind "complete", "csr" (complete frames handed over as plain CSR) or "knn<k>" (REGULAR(k))."""
    B, N = len(ns), max(ns)
    if kind.startswith("knn"):
        k = int(kind[3:])
        return types.SimpleNamespace(num_graphs=B, max_nodes=N, graph_kind=_lib.graph_regular(k), num_nodes=sum(ns),
                                     num_edges=k * sum(ns))
    E = sum(n * (n - 1) for n in ns)
    if kind == "complete":
        assert len(set(ns)) == 1
        return types.SimpleNamespace(num_graphs=B, max_nodes=N, graph_kind=_lib.GRAPH_COMPLETE, num_nodes=sum(ns),
                                     num_edges=E)
    assert kind == "csr"
    return types.SimpleNamespace(num_graphs=B, max_nodes=N, graph_kind=_lib.GRAPH_CSR, num_nodes=sum(ns), num_edges=E)


def plan_tuple(p):
    return (p.kernel_name, p.vec, p.lpc, p.cpb, p.threads, p.psplit, p.ncb, p.pre2, p.grid, p.lds_bytes)


# Slice widths each kernel is instantiated for (film_mean_fwd_launch.hpp, film_mean_bwd_launch.hpp).
VECS = {
    ("film_fwd", 4): (4, 2, 1), ("film_fwd", 2): (8, 4, 1),
    ("film_fwd_regular", 4): (4, 1), ("film_fwd_regular", 2): (8, 4, 1),
    ("film_bwd_fused", 4): (4, 2, 1), ("film_bwd_fused", 2): (4, 1),
    ("film_bwd_dx_gram", 4): (4, 2, 1), ("film_bwd_dx_gram", 2): (4, 1),
    ("film_bwd_regular", 4): (2, 1),
    ("film_bwd_mfma", 4): (4,), ("film_bwd_mfma", 2): (4,),
}
# Lanes per plane a kernel can run: what its cross-lane reduction covers.
#   film_fwd / film_fwd_regular: no lane reads another's values ("const int grp = threadIdx.x / a.lpc;",
#     "j += a.lpc;" are the only uses), so any power of two up to the 256-thread workgroup;
#   film_bwd_fused, one pass: "const int wpc = a.lpc > 64 ? a.lpc >> 6 : 1;" — a plane on lpc/64 waves, one
#     Gram partial per wave, added by the epilogue ("for (int w = 1; w < wpc; ++w)"): up to 256;
#   film_bwd_regular: "with_lanes(a.lpc, ...)" whose widest case is "default: f(std::integral_constant<int,
#     64>{})", then "if (active && li == 0)" alone stores: one wave, 64;
#   film_bwd_dx + Gram pass: the planner asks for 64 ("make_geometry(C, P, vec, 64, 64, ...)") and sizes the
#     Gram pass's LDS for one partial per channel ("lds_bwd(max_nodes, g.cpb, sig_lds)", lpc = 64): 64;
#   film_bwd_mfma: "one wave = one channel plane": 64 exactly.
MAX_LANES = {"film_fwd": 256, "film_fwd_regular": 256, "film_bwd_fused": 256, "film_bwd_regular": 64,
             "film_bwd_dx_gram": 64, "film_bwd_mfma": 64}
MAX_LDS = 65536  # no aggregation launcher raises hipFuncAttributeMaxDynamicSharedMemorySize


def violations(p, key, g, C, P, align):
    """What of the kernels' requirements the plan ``p`` (features ``key``, graph arguments ``g``, C channels of
    P pixels, storage aligned to ``align`` bytes) breaks: a list of strings, empty for a sound plan."""
    bad = []
    k = p.kernel_name
    if k == "none":
        return bad
    if p.vec not in VECS.get((k, ELEM[key]), ()):
        bad.append(f"{k} is not instantiated for slices of {p.vec} {key} elements")
    # "load_frag<VEC, true>(at_bytes(xb + ..., lane_plane + (uint32_t)jj * VEC * (uint32_t)sizeof(T)))": one
    # access of VEC elements, so rows of whole slices and pointers aligned to a slice
    if P % p.vec or align % min(p.vec * ELEM[key], 16):
        bad.append(f"slices of {p.vec} elements on P = {P}, {align}-byte aligned storage")
    pv = P // p.vec
    # "const int lir = (int)threadIdx.x & (a.lpc - 1);  // (lpc is a power of two)"; "int j = jbeg + li;" with
    # "if (active && j < jend) load_slice(j);": lanes past the plane idle, a plan should not have them
    # (film_bwd_mfma: a wave walks a plane in groups of 64 pixels, its 64 "lanes per plane" are the wave)
    if p.lpc < 1 or p.lpc & (p.lpc - 1) or (p.lpc > pv and k != "film_bwd_mfma"):
        bad.append(f"lpc {p.lpc} is no power of two <= P / vec = {pv}")
    # "__global__ void __launch_bounds__(kBlock) ..." with "constexpr int kBlock = 256;"
    if k == "film_bwd_mfma":
        # "constexpr int CPB = 4 * CPW * CB;  // channels per workgroup", CPW 1 or 2, 4 waves
        if p.threads != 256 or p.cpb not in (4, 8):
            bad.append(f"film_bwd_mfma with {p.threads} threads, {p.cpb} channels")
    elif not (1 <= p.threads == p.cpb * p.lpc <= 256):
        bad.append(f"threads {p.threads} != cpb {p.cpb} x lpc {p.lpc} or outside 1..256")
    # "const int c0 = cb * a.cpb;" ... "const bool active = grp < a.cpb && c < a.C;": the ncb blocks cover C
    if p.cpb < 1 or p.ncb * p.cpb < C or (p.ncb - 1) * p.cpb >= C:
        bad.append(f"{p.ncb} blocks of {p.cpb} channels for C = {C}")
    if p.lpc > MAX_LANES[k] or (k == "film_bwd_mfma" and p.lpc != 64):
        bad.append(f"{k} cannot reduce over {p.lpc} lanes per plane (MAX_LANES)")
    # "if (PRE2 && active && li < a.PV) load_into(gv2, xv2, 0, li + a.lpc);" and "the second (last) slice is
    # already in registers": exactly two slices per lane; instantiated for fp32 16-byte slices only
    if p.pre2 and not (k == "film_bwd_fused" and key == "f32" and p.vec == 4 and pv == 2 * p.lpc):
        bad.append(f"PRE2 with PV = {pv}, lpc = {p.lpc}, vec = {p.vec}, {key}")
    # "Requirements (launcher): P % 64 == 0, 16-byte aligned operands and node strides % 4 == 0."
    if k == "film_bwd_mfma" and (P % 64 or p.vec != 4 or not 9 <= g.max_nodes <= 16):
        bad.append(f"film_bwd_mfma at P = {P}, vec = {p.vec}, {g.max_nodes} nodes")
    if not 0 < p.lds_bytes <= MAX_LDS:
        bad.append(f"{p.lds_bytes} bytes of dynamic LDS")
    # "const int b = item / a.ncb;" (forward: "const int item = blockIdx.x / ps;")
    if p.psplit < 1 or p.grid != g.num_graphs * p.ncb * p.psplit or (p.psplit > 1 and p.psplit * p.lpc < pv):
        bad.append(f"grid {p.grid} for {g.num_graphs} graphs x {p.ncb} blocks x {p.psplit} segments")
    return bad


# ------------------------------------------------------------------------------------------------ GPU cases
# A row: knobs, a batch of B = 2 graphs (for the CSR / REGULAR kinds the second has fewer nodes than
# max_nodes), C = cpb + 3 or 2 cpb + 1 channels (more than one channel block, the last one ragged; C = 1, 7, 9
# for film_bwd_mfma), the smallest plane that gives the row's lanes per plane — and the kernel and (vec, lpc,
# cpb[, pre2]) its knobs are meant to reach, forward (``fwd``) and / or backward (``bwd``); the plan query
# must agree (test_geometry_cpu.py), and must differ from the plan under ``versus`` (the default knobs,
# or, for a row whose subject is a knob's default value, the knob's other value).
Row = collections.namedtuple("Row", "name kind ns C H W key knobs fwd bwd logits base mode epi versus")


def R(name, kind, ns, C, H, W, knobs, fwd=None, bwd=None, key="f32", logits=False, base=False, mode="film_mean",
      epi=False, versus=None):
    return Row(name, kind, ns, C, H, W, key, knobs, fwd, bwd, logits, base, mode, epi, versus or {})


FWD, FWR = "film_fwd", "film_fwd_regular"
FUS, REG, MFM, DXG = "film_bwd_fused", "film_bwd_regular", "film_bwd_mfma", "film_bwd_dx_gram"
BIG = 1 << 20


def FR(split, lanes, cap):
    return dict(fwd_regular_split=split, fwd_regular_lo=lanes, fwd_regular_hi=lanes, fwd_regular_cap=cap)


# film_bwd_regular (fp32, N = 9, 12, 16): bwd_regular_vec x bwd_regular_lanes, at k = 4 and k = 5, each on a 12x12
# plane (not one of film_bwd_mfma's) and on a 16x16 plane with bwd_regular_mfma = 0.  Lanes per plane the knobs
# are meant to give, by (slice width, bwd_regular_lanes): 8-byte slices the knob's power of two, 1-element
# slices (k = 5 always; k = 4 with bwd_regular_vec = 1) twice that, at most 64 — 2 x 64 asked for on a plane of
# 144 or 256 single elements is where the kernel's one-wave reduction needs the planner's cap.  Channels fill
# 256 threads up to 16.  Where a setting gives the default plan (12x12: lanes 16 / 24 of the default slice
# width), the row is held against bwd_regular_lanes = 1.
REG_LPC = {(2, 1): 1, (2, 8): 8, (2, 16): 16, (2, 24): 16, (2, 32): 32, (2, 64): 64,
           (1, 1): 2, (1, 8): 16, (1, 16): 32, (1, 24): 32, (1, 32): 64, (1, 64): 64}
REG_CPB = {1: 16, 2: 16, 8: 16, 16: 16, 32: 8, 64: 4}
REGULAR_SETTINGS = [(k, vec, lanes, plane) for k in (4, 5) for vec in (1, 2) for lanes in (1, 8, 16, 24, 32, 64)
                    for plane in (12, 16)]


def _regular_rows():
    rows = []
    for i, (k, vec, lanes, plane) in enumerate(REGULAR_SETTINGS):
        width = vec if k == 4 else 1  # k > 4 fits 1-element slices only
        lpc = REG_LPC[(width, lanes)]
        cpb = REG_CPB[lpc]
        kn = dict(bwd_regular_vec=vec, bwd_regular_lanes=lanes)
        if plane == 16:
            kn["bwd_regular_mfma"] = 0
        default = plane == 12 and lpc == REG_LPC[(width, 16)] and (k == 5 or vec == 2)
        rows.append(R(f"g_k{k}_v{vec}_l{lanes}_p{plane}", f"knn{k}", ((9, 6), (12, 9), (16, 12))[i % 3], cpb + 3, plane,
                      plane, kn, bwd=("film_bwd_regular", width, lpc, cpb), logits=i % 4 == 1, base=i % 4 == 2,
                      versus=dict(bwd_regular_lanes=1) if default else None))
    return rows

REGULAR_ROWS = _regular_rows()

ROWS = [
    # ---- film_fwd, complete and CSR: fwd_lo / fwd_hi, fwd_cap, fwd_vec2_below; N = 1, 5, 8, 16; every mode
    R("f01", "complete", (5, 5), 19, 4, 4, dict(fwd_lo=1, fwd_hi=1), fwd=(FWD, 4, 1, 16)),
    R("f02", "csr", (8, 5), 19, 8, 8, dict(fwd_lo=4, fwd_hi=4), fwd=(FWD, 4, 4, 16)),
    R("f03", "complete", (8, 8), 7, 16, 16, dict(fwd_lo=64, fwd_hi=64), fwd=(FWD, 4, 64, 4)),
    R("f04", "csr", (16, 9), 5, 32, 16, dict(fwd_lo=128, fwd_hi=128, fwd_vec2_below=0), fwd=(FWD, 4, 128, 2)),
    R("f05", "complete", (8, 8), 4, 32, 32, dict(fwd_lo=256, fwd_hi=256), fwd=(FWD, 4, 256, 1)),
    R("f06", "complete", (1, 1), 19, 8, 8, dict(fwd_lo=64, fwd_hi=4), fwd=(FWD, 4, 4, 16)),  # lo > hi
    R("f07", "csr", (5, 3), 19, 4, 4, dict(fwd_lo=3, fwd_hi=100), fwd=(FWD, 4, 2, 16)),  # no powers of two
    R("f08", "complete", (16, 16), 4, 8, 8, dict(fwd_cap=1), fwd=(FWD, 4, 16, 1)),
    R("f09", "csr", (8, 6), 7, 8, 8, dict(fwd_cap=3), fwd=(FWD, 4, 16, 3)),
    R("f10", "csr", (5, 4), 19, 8, 8, dict(fwd_cap=16, fwd_lo=4, fwd_hi=4), fwd=(FWD, 4, 4, 16), mode="film_sum"),
    R("f11", "complete", (5, 5), 19, 8, 8, dict(fwd_vec2_below=BIG), fwd=(FWD, 2, 16, 16)),
    R("f12", "csr", (8, 7), 19, 4, 4, dict(fwd_vec2_below=BIG), fwd=(FWD, 2, 8, 16), mode="copy_mean"),
    R("f13", "complete", (8, 8), 7, 16, 16, dict(fwd_lo=64, fwd_hi=64), fwd=(FWD, 4, 64, 4), epi=True),
    R("f14", "complete", (16, 16), 19, 4, 4, dict(fwd_lo=1, fwd_hi=1), fwd=(FWD, 4, 1, 16), key="bf16"),
    R("f15", "complete", (8, 8), 19, 8, 8, dict(fwd_lo=4, fwd_hi=4), fwd=(FWD, 8, 4, 16), key="f16"),
    R("f16", "complete", (5, 5), 19, 8, 8, dict(fwd_lo=4, fwd_hi=4), fwd=(FWD, 4, 4, 16), mode="film_sum"),
    R("f17", "complete", (8, 8), 19, 8, 8, dict(fwd_lo=4, fwd_hi=4), fwd=(FWD, 4, 4, 16), mode="copy_mean"),
    R("f18", "csr", (16, 11), 19, 5, 5, dict(fwd_lo=4, fwd_hi=4), fwd=(FWD, 1, 4, 16)),  # 1-element slices
    # ---- film_fwd_regular, k = 1, 4, 5, 8: fwd_regular_split x lo / hi x cap; N <= 8 and N = 16
    R("r01", "knn1", (8, 5), 4, 8, 8, dict(fwd_regular_split=1, fwd_regular_lo=8, fwd_regular_hi=8, fwd_regular_cap=1),
      fwd=(FWR, 4, 8, 1)),
    R("r02", "knn4", (8, 6), 9, 8, 8, dict(fwd_regular_split=0, fwd_regular_lo=8, fwd_regular_hi=8, fwd_regular_cap=4),
      fwd=(FWR, 4, 8, 4)),  # fp32 k = 4 mean: the compile-time-degree variant
    R("r03", "knn5", (8, 7), 19, 8, 8, dict(fwd_regular_split=1, fwd_regular_lo=8, fwd_regular_hi=8,
                                            fwd_regular_cap=16), fwd=(FWR, 4, 8, 16)),
    R("r04", "knn8", (16, 12), 4, 16, 16, dict(fwd_regular_split=0, fwd_regular_lo=32, fwd_regular_hi=32,
                                               fwd_regular_cap=1), fwd=(FWR, 4, 32, 1)),
    R("r05", "knn4", (16, 9), 7, 16, 16, dict(fwd_regular_split=1, fwd_regular_lo=32, fwd_regular_hi=32,
                                              fwd_regular_cap=4), fwd=(FWR, 4, 32, 4)),
    R("r06", "knn1", (16, 10), 11, 16, 16, dict(fwd_regular_split=1, fwd_regular_lo=32, fwd_regular_hi=32,
                                                fwd_regular_cap=16), fwd=(FWR, 4, 32, 8)),
    R("r07", "knn5", (8, 6), 4, 16, 16, dict(fwd_regular_split=0, fwd_regular_lo=64, fwd_regular_hi=64,
                                             fwd_regular_cap=1), fwd=(FWR, 4, 64, 1)),
    R("r08", "knn8", (16, 9), 7, 16, 16, dict(fwd_regular_split=1, fwd_regular_lo=64, fwd_regular_hi=64,
                                              fwd_regular_cap=4), fwd=(FWR, 4, 64, 4)),
    R("r09", "knn4", (16, 12), 7, 16, 16, dict(fwd_regular_split=0, fwd_regular_lo=64, fwd_regular_hi=64,
                                               fwd_regular_cap=16), fwd=(FWR, 4, 64, 4)),
    R("r10", "knn4", (8, 5), 9, 5, 5, dict(fwd_regular_split=1, fwd_regular_lo=8, fwd_regular_hi=8, fwd_regular_cap=4),
      fwd=(FWR, 1, 8, 4)),
    R("r11", "knn5", (8, 6), 7, 8, 8, dict(fwd_regular_split=1, fwd_regular_lo=8, fwd_regular_hi=8, fwd_regular_cap=4),
      fwd=(FWR, 8, 8, 4), key="bf16"),
    # the rest of fwd_regular_split x lo / hi x cap (r16 holds the default setting: against split = 1)
    R("r12", "knn4", (8, 6), 4, 8, 8, FR(0, 8, 1), fwd=(FWR, 4, 8, 1)),
    R("r13", "knn8", (16, 12), 19, 8, 8, FR(0, 8, 16), fwd=(FWR, 4, 8, 16)),
    R("r14", "knn5", (16, 9), 4, 16, 16, FR(1, 32, 1), fwd=(FWR, 4, 32, 1)),
    R("r15", "knn1", (8, 5), 7, 16, 16, FR(0, 32, 4), fwd=(FWR, 4, 32, 4)),
    R("r16", "knn8", (16, 9), 11, 16, 16, FR(0, 32, 16), fwd=(FWR, 4, 32, 8), versus=dict(fwd_regular_split=1)),
    R("r17", "knn4", (8, 7), 4, 16, 16, FR(1, 64, 1), fwd=(FWR, 4, 64, 1)),
    R("r18", "knn1", (16, 10), 7, 16, 16, FR(0, 64, 4), fwd=(FWR, 4, 64, 4)),
    R("r19", "knn5", (8, 6), 7, 16, 16, FR(1, 64, 16), fwd=(FWR, 4, 64, 4)),
    # ---- film_bwd_fused (N <= 8): bwd_fused_lo / hi, bwd_fused_cap, bwd_pre2; N = 8 complete (reduce-scatter
    # epilogue at >= 64 lanes) and N = 5; CSR; logits on and off; fp32 and bf16
    R("b01", "complete", (8, 8), 19, 4, 4, dict(bwd_fused_lo=1, bwd_fused_hi=1), bwd=(FUS, 4, 1, 16), logits=True),
    R("b02", "complete", (5, 5), 19, 8, 8, dict(bwd_fused_lo=4, bwd_fused_hi=4), bwd=(FUS, 4, 4, 16)),
    R("b03", "csr", (8, 5), 5, 32, 32, dict(bwd_fused_lo=128, bwd_fused_hi=128, bwd_pre2=0), bwd=(FUS, 4, 128, 2, 0)),
    R("b04", "complete", (8, 8), 4, 32, 32, dict(bwd_fused_lo=256, bwd_fused_hi=256), bwd=(FUS, 4, 256, 1, 0),
      logits=True),
    # bwd_pre2 where PV == 2 lpc (32x32 on 128 lanes, 8x8 on 8) and where it is not (32x32 on 64 lanes)
    R("b05", "complete", (8, 8), 5, 32, 32, dict(bwd_fused_lo=8, bwd_fused_hi=128, bwd_pre2=1), bwd=(FUS, 4, 128, 2, 1),
      base=True),
    R("b06", "complete", (8, 8), 5, 32, 32, dict(bwd_pre2=0), bwd=(FUS, 4, 128, 2, 0)),
    R("b07", "complete", (8, 8), 7, 32, 32, dict(bwd_pre2=2, bwd_fused_lo=64, bwd_fused_hi=64), bwd=(FUS, 4, 64, 4, 0)),
    R("b08", "complete", (5, 5), 19, 8, 8, dict(bwd_pre2=1), bwd=(FUS, 4, 8, 16, 1), base=True),
    R("b09", "complete", (8, 8), 5, 32, 32, dict(bwd_pre2=2), bwd=(FUS, 4, 128, 2, 1), versus=dict(bwd_pre2=0)),
    R("b10", "complete", (8, 8), 5, 32, 32, dict(bwd_pre2=2), bwd=(FUS, 4, 128, 2, 0), base=True,
      versus=dict(bwd_pre2=1)),
    R("b11", "complete", (8, 8), 4, 4, 4, dict(bwd_fused_cap=1), bwd=(FUS, 4, 4, 1)),
    R("b12", "csr", (8, 6), 7, 4, 4, dict(bwd_fused_cap=3), bwd=(FUS, 4, 4, 3), logits=True),
    R("b13", "csr", (5, 3), 19, 4, 4, dict(bwd_fused_cap=16, bwd_fused_lo=1, bwd_fused_hi=1), bwd=(FUS, 4, 1, 16)),
    R("b14", "complete", (8, 8), 35, 4, 4, dict(bwd_fused_cap=32), bwd=(FUS, 4, 4, 32), logits=True),
    # 64 channels of 8-node tiles with the sigmoid values are 70,688 bytes of LDS: the planner runs 32
    R("b15", "complete", (8, 8), 65, 4, 4, dict(bwd_fused_cap=64), bwd=(FUS, 4, 4, 32), logits=True),
    R("b16", "complete", (8, 8), 67, 4, 4, dict(bwd_fused_cap=64), bwd=(FUS, 4, 4, 64)),
    R("b17", "csr", (5, 4), 67, 4, 4, dict(bwd_fused_cap=64), bwd=(FUS, 4, 4, 64), logits=True),
    R("b18", "complete", (8, 8), 19, 8, 8, dict(bwd_fused_lo=4, bwd_fused_hi=4), bwd=(FUS, 4, 4, 16), key="bf16"),
    R("b19", "complete", (8, 8), 4, 32, 32, dict(bwd_fused_lo=256, bwd_fused_hi=256), bwd=(FUS, 4, 256, 1), key="bf16",
      logits=True),
    R("b20", "csr", (5, 3), 67, 4, 4, dict(bwd_fused_cap=64), bwd=(FUS, 4, 4, 64), key="bf16"),
    R("b21", "complete", (5, 5), 19, 5, 5, dict(bwd_fused_lo=4, bwd_fused_hi=4), bwd=(FUS, 1, 4, 16)),
    # ---- film_bwd_regular: generated below (REGULAR_ROWS)
    *REGULAR_ROWS,
    # ---- film_bwd_mfma: bwd_mfma_cpw at C = 1, 7, 9 (fewer than, and ragged against, the workgroup's 4 or 8
    # channels); regular and complete; N = 9, 16; fp32 and fp16.  2 is the default: those rows against 1
    R("m01", "complete", (9, 9), 1, 8, 8, dict(bwd_mfma_cpw=1), bwd=(MFM, 4, 64, 4)),
    R("m02", "complete", (16, 16), 7, 8, 8, dict(bwd_mfma_cpw=1), bwd=(MFM, 4, 64, 4), logits=True),
    R("m03", "knn4", (16, 12), 9, 8, 8, dict(bwd_mfma_cpw=1), bwd=(MFM, 4, 64, 4)),
    R("m04", "knn5", (16, 9), 7, 8, 8, dict(bwd_mfma_cpw=1), bwd=(MFM, 4, 64, 4), key="f16"),
    R("m05", "complete", (16, 16), 9, 8, 8, dict(bwd_mfma_cpw=2), bwd=(MFM, 4, 64, 8), key="f16",
      versus=dict(bwd_mfma_cpw=1)),
    R("m06", "knn4", (9, 6), 1, 8, 8, dict(bwd_mfma_cpw=2), bwd=(MFM, 4, 64, 8), versus=dict(bwd_mfma_cpw=1)),
    R("m07", "knn8", (16, 10), 7, 8, 16, dict(bwd_mfma_cpw=2), bwd=(MFM, 4, 64, 8), base=True,
      versus=dict(bwd_mfma_cpw=1)),
    R("m08", "complete", (9, 9), 9, 8, 8, dict(bwd_mfma_cpw=1), bwd=(MFM, 4, 64, 4), key="f16", logits=True),
    # ---- default knobs: the Gram pass of complete 16-node graphs with logits at C >= 16 asked for 67,392
    # bytes of LDS (a launch error) before the planner halved its channels
    R("d01", "complete", (16, 16), 17, 4, 4, {}, bwd=(DXG, 4, 4, 8), logits=True),
]


# ------------------------------------------------------------------ film_max_fwd and film_wmean_fwd under the knobs
# Both size their launch with "make_geometry(C, P, vec, tu.fwd_lo, tu.fwd_hi, tu.fwd_cap)" (film_max_fwd.hip,
# film_wmean_fwd.hip), film_fwd's knobs, and have no plan query.  ``make_geometry`` below restates the planner
# (test_geometry_cpu.py holds it equal to what mrp_film_mean_fwd_plan reports for film_fwd over the knobs' ranges, and
# pins the restated lines to the source); ``forward_geometry`` adds each launcher's slice width and plane split.
MAKE_GEOMETRY_SOURCE = [  # film_mean_kernels.hpp, make_geometry
    "const int pv = P / g.vec;",
    "const int target = std::min(std::max(pv / 2, lo), hi);",
    "int lpc = 1;",
    "while (lpc * 2 <= pv && lpc * 2 <= target) lpc *= 2;",
    "int cpb = mrp::kBlock / lpc;",
    "if (cpb > max_cpb) cpb = max_cpb;",
    "if (cpb > C) cpb = C;",
    "g.threads = cpb * lpc;",
    "g.ncb = (C + cpb - 1) / cpb;",
]
KBLOCK = 256  # "constexpr int kBlock = 256;"


def make_geometry(C, P, vec, lo, hi, cap):
    """(lpc, cpb, threads, ncb): MAKE_GEOMETRY_SOURCE, line for line."""
    pv = P // vec
    target = min(max(pv // 2, lo), hi)
    lpc = 1
    while lpc * 2 <= pv and lpc * 2 <= target:
        lpc *= 2
    cpb = KBLOCK // lpc
    if cpb > cap:
        cpb = cap
    if cpb > C:
        cpb = C
    return lpc, cpb, cpb * lpc, (C + cpb - 1) // cpb


def forward_geometry(row, lo=16, hi=64, cap=16):
    """(vec, lpc, cpb, psplit) of a FWD_ROWS row's launch on dense, 16-byte aligned x and out under the given knobs
    (defaults: "int fwd_lo = 16", "fwd_hi = 64", "fwd_cap = 16" of tuning.hpp).  Slice width, film_max_fwd.hip:
    "if (elem == 2 && max_nodes <= 8 && sc.ok(8, elem)) vec = 8; else if (sc.ok(4, elem)) vec = 4;";
    film_wmean_fwd.hip: "sc.ok(4, elem) && aligned16(w) && w_node_stride % 4 == 0 ? 4 : 1".  Plane split, both:
    "g.psplit = graph_kind == MRP_GRAPH_COMPLETE ? (pv + g.lpc - 1) / g.lpc : 1;"."""
    P = row.H * row.W
    if row.family == "max":
        vec = 8 if ELEM[row.key] == 2 and max(row.ns) <= 8 and P % 8 == 0 else 4 if P % 4 == 0 else 1
    else:
        vec = 4 if P % 4 == 0 and not row.w_odd else 1
    lpc, cpb, _, _ = make_geometry(row.C, P, vec, lo, hi, cap)
    pv = P // vec
    return vec, lpc, cpb, (pv + lpc - 1) // lpc if row.kind == "complete" else 1


# A row: the family, a batch of two graphs (CSR / k-NN: the second smaller), C with a ragged last channel block, the
# smallest plane that gives the row's lanes, the knobs, and the (vec, lpc, cpb, psplit) they are meant to reach —
# written by hand; test_geometry_cpu.py holds them equal to ``forward_geometry``.  ``mode``: film_wmean's; ``w_odd``:
# w with a node stride of P + 1 elements, which allows x 4-element slices but not w.
FwdRow = collections.namedtuple("FwdRow", "name family kind ns C H W key knobs geo mode w_odd")


def F(name, family, kind, ns, C, H, W, knobs, geo, key="f32", mode="mean", w_odd=False):
    return FwdRow(name, family, kind, ns, C, H, W, key, knobs, geo, mode, w_odd)


def LH(lanes):
    return dict(fwd_lo=lanes, fwd_hi=lanes)


FWD_ROWS = [
    # ---- film_max_fwd
    F("x01", "max", "complete", (5, 5), 19, 4, 4, LH(1), (4, 1, 16, 4)),  # one lane, the plane in 4 segments
    F("x02", "max", "csr", (8, 5), 19, 4, 4, LH(2), (4, 2, 16, 1)),  # a lane walks 2 slices
    F("x03", "max", "csr", (16, 9), 19, 8, 8, LH(4), (4, 4, 16, 1)),  # a lane walks 4 slices
    F("x04", "max", "complete", (8, 8), 7, 16, 16, LH(64), (4, 64, 4, 1)),
    F("x05", "max", "knn4", (16, 12), 5, 32, 16, LH(128), (4, 128, 2, 1)),
    F("x06", "max", "complete", (4, 4), 4, 32, 32, LH(256), (4, 256, 1, 1)),
    # 20 slices on 8 lanes: 3 segments, the last ragged (6 x 8 on 8 lanes is ragged too, but is the default plan)
    F("x07", "max", "complete", (8, 8), 19, 8, 10, LH(8), (4, 8, 16, 3)),
    F("x08", "max", "complete", (3, 3), 4, 8, 8, dict(fwd_cap=1), (4, 16, 1, 1)),
    F("x09", "max", "csr", (8, 6), 7, 8, 8, dict(fwd_cap=3), (4, 16, 3, 1)),
    F("x10", "max", "knn4", (8, 6), 19, 8, 8, dict(fwd_cap=16, fwd_lo=64, fwd_hi=4), (4, 4, 16, 1)),  # lo > hi
    F("x11", "max", "csr", (5, 3), 19, 4, 4, dict(fwd_lo=3, fwd_hi=100), (4, 2, 16, 1)),  # no powers of two
    F("x12", "max", "csr", (16, 11), 19, 5, 5, LH(4), (1, 4, 16, 1)),  # 1-element slices
    F("x13", "max", "complete", (8, 8), 19, 8, 8, LH(4), (8, 4, 16, 2), key="bf16"),  # 8-element slices
    F("x14", "max", "knn4", (16, 12), 19, 8, 8, LH(4), (4, 4, 16, 1), key="f16"),
    F("x15", "max", "complete", (16, 16), 19, 4, 4, LH(1), (4, 1, 16, 4), key="bf16"),
    # ---- film_wmean_fwd
    F("w01", "wmean", "complete", (5, 5), 19, 4, 4, LH(1), (4, 1, 16, 4)),
    F("w02", "wmean", "csr", (8, 5), 19, 4, 4, LH(2), (4, 2, 16, 1), mode="sum"),
    F("w03", "wmean", "knn4", (16, 9), 19, 8, 8, LH(4), (4, 4, 16, 1)),
    F("w04", "wmean", "complete", (8, 8), 7, 16, 16, LH(64), (4, 64, 4, 1), mode="sum"),
    F("w05", "wmean", "csr", (16, 9), 5, 32, 16, LH(128), (4, 128, 2, 1)),
    F("w06", "wmean", "complete", (4, 4), 4, 32, 32, LH(256), (4, 256, 1, 1)),
    F("w07", "wmean", "complete", (8, 8), 19, 8, 10, LH(8), (4, 8, 16, 3), mode="sum"),
    F("w08", "wmean", "complete", (3, 3), 4, 8, 8, dict(fwd_cap=1), (4, 16, 1, 1)),
    F("w09", "wmean", "csr", (8, 6), 7, 8, 8, dict(fwd_cap=3), (4, 16, 3, 1), mode="sum"),
    F("w10", "wmean", "knn4", (8, 6), 19, 8, 8, dict(fwd_cap=16, fwd_lo=64, fwd_hi=4), (4, 4, 16, 1)),
    F("w11", "wmean", "csr", (5, 3), 19, 4, 4, dict(fwd_lo=3, fwd_hi=100), (4, 2, 16, 1)),
    F("w12", "wmean", "csr", (16, 11), 19, 5, 5, LH(4), (1, 4, 16, 1)),
    F("w13", "wmean", "complete", (8, 8), 19, 8, 8, LH(4), (4, 4, 16, 4), key="bf16"),
    F("w14", "wmean", "knn4", (16, 12), 19, 8, 8, LH(4), (4, 4, 16, 1), key="f16", mode="sum"),
    F("w15", "wmean", "complete", (8, 8), 19, 8, 8, LH(4), (1, 4, 16, 16), w_odd=True),  # w forces single elements
]
