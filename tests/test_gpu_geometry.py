"""GPU: the aggregation kernels at the launch geometries the tuning knobs select, and the GEMMs at the tile
orders theirs select — each against float64, none of which the knob sweeps in tools/ ever checked.

A parity test, not a probe: every row of ``geometry_cases.ROWS`` is first planned through the plan query
(``mrp_film_mean_fwd_plan`` / ``_bwd_plan``, the planner the launch itself calls) and is launched only if the
plan holds every requirement of the kernel it names (``geometry_cases.violations``) and is the geometry the row
says it reaches; test_geometry_cpu.py does the same for the whole knob ranges without a GPU.

Bars: fp32 features ``rel_err <= TOL`` (test_gpu_properties); 16-bit features ``half_cases``' elementwise and
relative bars; the GEMMs the bars of their families' own tests (imported from them).  On top of the bar, every
output whose per-element arithmetic does not depend on the geometry must have the bits of the default-knob run:
the forward and grad_x of the VALU kernels, where a lane computes its elements alone, in source order — but not
grad_gb, whose reduction tree follows the lanes per plane — and every GEMM output, since the tile order changes
which workgroup computes a tile, not the tile.

``film_max_fwd`` and ``film_wmean_fwd`` take film_fwd's ``fwd_lo`` / ``fwd_hi`` / ``fwd_cap`` and have no plan query:
``geometry_cases.FWD_ROWS`` names by hand the geometry each row's knobs reach, test_geometry_cpu.py holds that to a
mirror of the planner (itself held to the plan query), and ``test_forward_row_under_knobs`` runs each row under its
knobs and under the defaults: bit-identical, the default run under the family's own bar.
"""
import functools

import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import aggregate, compress
import geometry_cases as gc
import half_cases as hc
import max_cases as mc
import oracle
import test_gpu_compress_cl as t_half_cl
import test_gpu_compress_gemm as t_split
import test_gpu_compress_half as t_half
import test_gpu_compress_split_cl as t_split_cl
import test_gpu_film_wmean as t_wmean
import wmean_cases as wmc
from conftest import rel_err
from test_gpu_properties import TOL

pytestmark = pytest.mark.gpu

VALU = ("film_fwd", "film_fwd_regular", "film_bwd_fused", "film_bwd_regular", "film_bwd_dx_gram")


@functools.lru_cache(maxsize=None)
def graph(kind, ns):
    seed = 7 + sum(ns) + len(kind)
    return hc._frames(list(ns), seed, knn=int(kind[3:]) if kind.startswith("knn") else None)


def csr_of(row, dev):
    g = graph(row.kind, row.ns)
    csr = g.csr(dev) if row.kind != "csr" else g.csr(dev, allow_complete=False, allow_regular=False)
    want = gc.graph_ns(row.kind, row.ns)
    assert (csr.num_graphs, csr.max_nodes, csr.graph_kind, csr.num_nodes, csr.num_edges) == (
        want.num_graphs, want.max_nodes, want.graph_kind, want.num_nodes, want.num_edges)
    return csr


@functools.lru_cache(maxsize=None)
def case(name):
    """CPU inputs of a row and its float64 (and, for the 16-bit bars, float32) oracle results, computed once."""
    row = next(r for r in gc.ROWS if r.name == name)
    T = gc.DTYPES[row.key]
    g = graph(row.kind, row.ns)
    n, E = g.num_nodes(), g.num_edges()
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 977)
    x, G, G0, x0 = (torch.randn(n, row.C, row.H, row.W, generator=gen).to(T) for _ in range(4))
    z = torch.randn(E, row.C, 2, generator=gen)
    gb = torch.sigmoid(z)  # fp32: what the kernel is given without logits
    src, dst = (t.numpy() for t in g.edges())
    ref = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        gbt = torch.sigmoid(z.to(dt)) if row.logits else gb.to(dt)
        ref["out" + tag] = oracle.film_aggregate(x.to(dt), gbt, src, dst, row.mode)
        if E == 0:
            ref["dx" + tag], dgb = torch.zeros_like(x, dtype=dt), torch.zeros_like(gbt)
        else:
            ref["dx" + tag], dgb = oracle.film_aggregate_grads(x.to(dt), gbt, src, dst, G.to(dt), row.mode)
        ref["dgb" + tag] = dgb * gbt * (1 - gbt) if row.logits else dgb  # the gradient of the logits
    return row, x, G, G0, x0, z, gb, ref


def planned(row, csr, direction, check_row):
    """The plan of the call about to be made (under the knobs now set); fails, before any launch, if it breaks
    a requirement of its kernel or (check_row: under the row's own knobs) is not what the row names."""
    p = aggregate.launch_plan(direction, csr, row.C, row.H * row.W, dtype=gc.DTYPES[row.key], mode=row.mode,
                              logits=row.logits, grad_x_base=row.base, x0=row.epi, xcopy=row.epi)
    bad = gc.violations(p, row.key, csr, row.C, row.H * row.W, 16)
    assert not bad, (row.name, direction, gc.plan_tuple(p), bad)
    want = (row.fwd if direction == "fwd" else row.bwd) if check_row else None
    if want is not None:
        got = (p.kernel_name, p.vec, p.lpc, p.cpb) + ((p.pre2,) if len(want) == 5 else ())
        assert got == tuple(want), (row.name, direction, gc.plan_tuple(p))
    return p


def run(row, dev, knobs_, check_row):
    """Forward and backward of a row under the given knobs: (plans, out, xcopy, dx, dgb).  check_row: the knobs are
    the row's own, so the plans must be what the row names — checked, like the requirements, before any launch."""
    _, x, G, G0, x0, z, gb, _ = case(row.name)
    csr = csr_of(row, dev)
    x, G, G0, x0 = (t.to(dev) for t in (x, G, G0, x0))
    w = (z if row.logits else gb).to(dev)
    assert all(t.data_ptr() % 16 == 0 and t.is_contiguous() for t in (x, G, G0, x0))  # what `planned` assumes
    mode = aggregate._mode_flags(row.mode, row.logits)
    copy = row.mode == "copy_mean"
    with gc.knobs(**knobs_):
        plans = {d: planned(row, csr, d, check_row) for d in ("fwd", "bwd")}
        xc = None
        if row.epi:  # 0.7 a + 0.3 x0, and a copy of x (the first half of a concatenation)
            out, xc = torch.empty_like(x), torch.empty_like(x)
            aggregate.film_mean_forward_into(x, w, csr, mode, out,
                                             epilogue=aggregate.EpilogueSpec(0.7, 0.0, x0, 0.3, xc))
        else:
            out = m.film_mean(x, None if copy else w, csr, row.mode, logits=row.logits)
        dx, dgb = aggregate.film_mean_backward(G, x, None if copy else w, csr, mode, True, not copy and csr.num_edges > 0,
                                               grad_x_base=G0 if row.base else None)
        torch.cuda.synchronize()
    return plans, out, xc, dx, dgb


@functools.lru_cache(maxsize=None)
def default_run(name, dev):
    return run(next(r for r in gc.ROWS if r.name == name), dev, {}, False)


def hold(got, ref, name, row, what):
    """The bar of the row's dtype for output `name` ("out", "dx", "dgb")."""
    T = gc.DTYPES[row.key]
    e = rel_err(got.detach().float().cpu().numpy(), ref[name + "64"].numpy()) if ref[name + "64"].numel() else 0.0
    print(row.name, what, name, "rel_err", e)
    if row.key == "f32":
        assert got.dtype == torch.float32 and e <= TOL, (row.name, what, name, e)
    elif name == "dgb":
        assert got.dtype == torch.float32
        hc.assert_relative(got, ref["dgb32"], ref["dgb64"], (row.name, what, name))
    else:
        assert got.dtype == T
        hc.assert_elementwise(got, ref[name + "64"], T, (row.name, what, name))


@pytest.mark.parametrize("name", [r.name for r in gc.ROWS])
def test_row_against_float64(cuda_device, name):
    row, x, G, G0, x0, z, gb, ref = case(name)
    dev = cuda_device
    plans, out, xc, dx, dgb = run(row, dev, row.knobs, True)
    ref = dict(ref)
    if row.epi:
        for tag in ("64", "32"):
            ref["out" + tag] = 0.7 * ref["out" + tag] + 0.3 * x0.to(ref["out" + tag].dtype)
        assert torch.equal(hc.bits(xc), hc.bits(x))
    if row.base:
        for tag in ("64", "32"):
            ref["dx" + tag] = ref["dx" + tag] + G0.to(ref["dx" + tag].dtype)
    hold(out, ref, "out", row, "knobs")
    hold(dx, ref, "dx", row, "knobs")
    if dgb is not None:
        hold(dgb.view(z.shape), ref, "dgb", row, "knobs")
    if not row.knobs:
        return
    # the default-knob run: the same bars, and the same bits wherever the geometry cannot change them
    dplans, dout, dxc, ddx, ddgb = default_run(name, dev)
    hold(dout, ref, "out", row, "defaults")
    hold(ddx, ref, "dx", row, "defaults")
    if ddgb is not None:
        hold(ddgb.view(z.shape), ref, "dgb", row, "defaults")
    if plans["fwd"].kernel_name == dplans["fwd"].kernel_name and plans["fwd"].kernel_name in VALU:
        assert torch.equal(hc.bits(out), hc.bits(dout)), (name, "forward bits depend on the geometry")
    if plans["bwd"].kernel_name == dplans["bwd"].kernel_name and plans["bwd"].kernel_name in VALU:
        assert torch.equal(hc.bits(dx), hc.bits(ddx)), (name, "grad_x bits depend on the geometry")


# ------------------------------------------------- film_max_fwd and film_wmean_fwd under film_fwd's knobs
@functools.lru_cache(maxsize=None)
def fwd_case(name):
    """CPU inputs of a ``geometry_cases.FWD_ROWS`` row and its reference: film_max on the 2^-3 lattice (every
    message exact in every dtype: ``max_cases.reference`` in fp32 is the exact result), film_wmean on random
    operands with ``wmean_cases``' weights against ``wmean_cases.forward`` in float64."""
    row = next(r for r in gc.FWD_ROWS if r.name == name)
    T = gc.DTYPES[row.key]
    g = graph(row.kind, row.ns)
    seed = sum(map(ord, name)) * 977
    if row.family == "max":
        x, gb, _, _ = mc.lattice_operands(g, row.C, row.H, row.W, seed)
        return row, x.to(T), gb, None, mc.reference(g, x, gb)[0]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g.num_nodes(), row.C, row.H, row.W, generator=gen).to(T)
    gb = torch.sigmoid(torch.randn(g.num_edges(), row.C, 2, generator=gen))
    w = wmc.weights_of(g.num_nodes(), row.H, row.W, gen)
    return row, x, gb, w, wmc.forward(g, x.double(), gb.double(), w.double(), row.mode)


def fwd_run(row, dev, knobs_, w_odd):
    """The row's forward under the given knobs.  w_odd: w as rows of a (N, P + 1) buffer, a node stride that is no
    multiple of 4 elements."""
    _, x, gb, w, _ = fwd_case(row.name)
    csr = csr_of(row, dev)
    xd, gbd = x.to(dev), gb.to(dev)
    assert xd.data_ptr() % 16 == 0 and xd.is_contiguous()  # what ``forward_geometry`` assumes
    out = torch.empty_like(xd)
    key = "%s_fwd_%s" % (row.family, row.key)
    before = aggregate.PATH_COUNTS[key]
    with gc.knobs(**knobs_):
        if row.family == "max":
            aggregate.film_max_forward_into(xd, gbd, csr, 0, out)
        else:
            n, P = w.shape[0], row.H * row.W
            wd = w.to(dev)
            if w_odd:
                buf = torch.zeros(n, P + 1, device=dev)
                buf[:, :P] = wd.view(n, P)
                wd = buf.as_strided((n, row.H, row.W), (P + 1, row.W, 1))
                assert P % 4 == 0 and wd.stride(0) % 4 and wd.data_ptr() % 16 == 0
            aggregate.film_wmean_forward_into(xd, gbd, wd, csr, 0, out, row.mode)
        torch.cuda.synchronize()
    assert aggregate.PATH_COUNTS[key] == before + 1
    return out.cpu()


@pytest.mark.parametrize("name", [r.name for r in gc.FWD_ROWS])
def test_forward_row_under_knobs(cuda_device, name):
    """film_max_fwd / film_wmean_fwd at the geometry the row's knobs select (test_geometry_cpu.py holds the row's
    hand-written geometry to the planner's mirror) against the default-knob run: bit-identical — a lane computes its
    pixels alone, the row's sources in source order, whatever the lanes per plane, the channels per workgroup and
    the plane split — and the default-knob run under the family's own bar against its reference."""
    row, x, gb, w, ref = fwd_case(name)
    T = gc.DTYPES[row.key]
    knobbed = fwd_run(row, cuda_device, row.knobs, row.w_odd)
    default = fwd_run(row, cuda_device, {}, row.w_odd)
    assert knobbed.dtype == default.dtype == T
    assert torch.equal(hc.bits(knobbed), hc.bits(default)), (name, "forward bits depend on the geometry")
    if row.family == "max":
        assert torch.equal(hc.bits(default), hc.bits(ref.to(T))), name
    elif row.key == "f32":
        e = rel_err(default.numpy(), ref.numpy())
        print(name, "rel_err", e)
        assert e <= t_wmean.TOL, (name, e)
    else:
        hc.assert_elementwise(default, ref, T, name)
    if row.w_odd:  # single elements because of w alone: "the per-element sums do not depend on slice width"
        aligned = fwd_run(row, cuda_device, {}, False)
        assert torch.equal(hc.bits(aligned), hc.bits(default)), (name, "forward bits depend on the slice width")


# ----------------------------------------------------------------------------- the GEMMs' tile order
# C = 768: 3 row tiles of 256 (the data gradient: 6), so runs of 2 and 5 end ragged; 4 x 8 x 8 = 256 pixel
# rows: 2 column tiles of 128.  gemm_group orders the forward and the data gradient, nt_group the weight
# gradient (gemm_common.hpp tile_of); the weight gradient's split count is pinned by the family's own knob,
# so only the order differs between two runs.
GEMM_SHAPE = (768, 4, 8, 8)
GROUPS = (0, 1, 2, 3, 5, 64)
NAMES = ("y", "gx", "ga", "gw", "gb")


def _gemm_operands(family, dev):
    C, n, H, W = GEMM_SHAPE
    if FAMILIES[family][1] == "f32":
        gen = torch.Generator().manual_seed(768)
        w = torch.randn(C, 2 * C, 1, 1, generator=gen) / (2 * C) ** 0.5
        b = torch.randn(C, generator=gen)
        x, a, gy = (torch.randn(n, C, H, W, generator=gen) for _ in range(3))
        w, b, x, a, gy = (t.to(dev) for t in (w, b, x, a, gy))
        r64, r32 = (t_split._ref(w, b, x, a, gy, dt) for dt in (torch.float64, torch.float32))
        ref = {"64": dict(zip(NAMES, r64)), "32": dict(zip(NAMES, r32))}
        return w, b, x, a, gy, ref
    if family == "compress_half":
        w, b, x, a, gy, ref = t_half._case(C, n, H, W, "bf16")
        return tuple(t.to(dev) for t in (w, b, x, a, gy)) + (ref,)
    if family == "compress_half_cl":
        w, b, x, a, gy, ref = t_half_cl._case(C, n, H, W, "f16")
    else:
        w, b, x, a, gy, ref = t_split_cl._case(C, n, H, W)
    return (w.to(dev), b.to(dev)) + tuple(t_half_cl._cl(t, dev) for t in (x, a, gy)) + (ref,)


FAMILIES = {  # family -> (knobs that pin the route and the weight gradient's split count, the counters that move)
    # fp32 NCHW on the split-bf16 kernels; C = 768 < 1024 takes the weight gradient that splits both operands in
    # the kernel (split_nt 3), split_nt = 4 the one that reads dy pre-split (split_rows + gemm_nt_psa): nt_group
    # orders both (the planner's split count depends on the shape alone: the family has no knob for it)
    "compress_split": (dict(), "f32"),
    "compress_split_nt4": (dict(split_nt=4), "f32"),
    "compress_half": (dict(half_nt_splits=2), "bf16"),
    "compress_half_cl": (dict(half_cl_splits=2), "cl_f16"),
    "compress_split_cl": (dict(split_cl_splits=2), "cl_f32"),
}


def _gemm_products(family, dev, group):
    w, b, x, a, gy, _ = gemm_case(family, dev)
    pin, key = FAMILIES[family]
    C, P = GEMM_SHAPE[0], GEMM_SHAPE[2] * GEMM_SHAPE[3]
    before = dict(compress.PATH_COUNTS)
    with gc.knobs(gemm_group=group[0], nt_group=group[1], **pin):
        if key == "f32":
            with t_split._path("split"):
                # the Python layer routes all three products to the split-bf16 entry points, not the fp32 MFMA
                assert all(compress._split(op) for op in ("fwd", "dgrad", "wgrad")) and C % 64 == 0 and P % 32 == 0
                outs = t_split_cl._products(w, b, x, a, gy)
        elif family == "compress_split_cl":
            with t_split_cl._native():
                outs = t_split_cl._products(w, b, x, a, gy)
        else:
            outs = t_split_cl._products(w, b, x, a, gy)
        torch.cuda.synchronize()
    # the family's own kernels ran, each once
    moved = {k: v - before.get(k, 0) for k, v in compress.PATH_COUNTS.items() if v != before.get(k, 0)}
    assert moved == {f"{p}_{key}": 1 for p in ("fwd", "dgrad", "wgrad")}, moved
    return outs


@functools.lru_cache(maxsize=None)
def gemm_case(family, dev):
    return _gemm_operands(family, dev)


@functools.lru_cache(maxsize=None)
def gemm_default(family, dev):
    """The products at the default tile orders (gemm_group 4, nt_group 0), computed once."""
    return _gemm_products(family, dev, (4, 0))


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_tile_order_changes_no_product(cuda_device, family, group):
    dev = cuda_device
    ref = gemm_case(family, dev)[5]
    outs = _gemm_products(family, dev, (group, group))
    what = f"{family} gemm_group = nt_group = {group}"
    for name, got in zip(NAMES, outs):
        if FAMILIES[family][1] == "f32":
            t_split._check(got, ref["32"][name], ref["64"][name], f"{what} {name}")
        elif family == "compress_split_cl":
            t_split_cl._check(got, ref, name, what)
        elif name in ("gw", "gb"):
            t_half._check_f32(got, ref, name, what)
        else:
            t_half._check_t(got, ref, name, torch.bfloat16 if family == "compress_half" else torch.float16, what)
    for name, got, want in zip(NAMES, outs, gemm_default(family, dev)):
        assert torch.equal(hc.bits(got), hc.bits(want)), (what, name, "differs from the default order's bits")
