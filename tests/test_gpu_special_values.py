"""GPU: every kernel on zeros, subnormals, infinities, NaNs and overflow (inputs and references from
``special_cases``; ``test_special_values_cpu.py`` pins that each input discriminates).

1. the mean's division: special sums in every group position of the node-major COMPLETE forward (the fast
   division's gate and its IEEE branch), in the pixel-major, REGULAR and CSR forwards — bit for bit the fp32
   oracle, cast once for 16-bit features;
2. the fast sigmoid at saturation, forward and backward, and a NaN logit's confinement;
3. the store to bf16 / fp16 at overflow, ties, subnormals, NaN, +-inf, -0: torch's CPU cast, bit for bit;
4. one non-finite element stays visible and stays where the reference puts it: aggregation forward
   (strict: the reference's set exactly), aggregation backward (its graph, channel and pixel), the four compress
   families, the encoder's entry points;
5. the split-bf16 products are bit-equivariant under power-of-two scaling of their operands, and the upper
   edge of their domain (0x7f7f8000 rounds to a bf16 infinity).

Comparisons use bits where the reference is finite and "is NaN" where it is NaN.  Every poisoned value is data
inside valid buffers."""
import ctypes

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib, aggregate, compress
import half_cases as hc
import oracle
import span_cases as sp
import special_cases as spc
import split_cases as sc
from conftest import rel_err
from test_gpu_large_span import FAMILY, Dense, _acase, _agraph, _call_dgrad, _call_fwd, _call_wgrad

pytestmark = pytest.mark.gpu

ALL = ["f32", "bf16", "f16"]
HALF = ["bf16", "f16"]
CL = torch.channels_last
FILM_MEAN, FILM_SUM, LOGITS = _lib.MODE_FILM_MEAN, _lib.MODE_FILM_SUM, _lib.GB_LOGITS
NCHW_CASES = list(hc.CASES)
CL_CASES = ["a", "b", "c", "d", "e", "f", "g"]  # h, i4, i1 are node-major views
LAYOUT_CASES = [("nchw", n) for n in NCHW_CASES] + [("cl", n) for n in CL_CASES]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---- aggregation through the C ABI ---------------------------------------------------------------------------
class Op:
    """A device (n, C, H, W) tensor as the entry points see it: pointer, node stride, pixel stride."""

    def __init__(self, t, layout):
        self.t, self.layout = t, layout
        self.address, self.ptr = t.data_ptr(), ctypes.c_void_p(t.data_ptr())
        self.ns = t.stride(0)
        self.ps = t.stride(3) if layout == "cl" else 0
        if layout == "cl":
            assert t.stride(1) == 1 and t.stride(2) == t.shape[3] * self.ps
        else:
            assert t.stride(3) == 1 and t.stride(2) == t.shape[3] and t.stride(1) == t.shape[2] * t.shape[3]

    def host(self):
        return self.t.cpu().contiguous()


def _op(t, dev, layout, name=None):
    """The CPU tensor t on the device in ``layout``; for the cases h / i4 / i1 as that case's strided or
    misaligned view (``half_cases.embed``)."""
    t = t.to(dev)
    if layout == "cl":
        return Op(t.contiguous(memory_format=CL), layout)
    if name in ("h", "i4", "i1"):
        leaf, view = hc.embed(name, t)
        return Op(view(leaf), layout)
    return Op(t.contiguous(), layout)


def _new(shape, T, dev, layout):
    t = torch.empty(shape, dtype=T, device=dev)
    return Op(t.contiguous(memory_format=CL) if layout == "cl" else t, layout)


def agg_forward(dev, g, key, layout, X, gb, mode, scales=None, X0=None, xcopy=False):
    """``mrp_film_mean_fwd_t`` / ``_fwd_cl`` -> (out, xcopy or None) on the CPU; ``scales`` = (agg, self, x0)."""
    lib, csr = m.load_library(), g.csr(dev)
    n, C, H, W = X.t.shape
    T = spc.DTYPES[key]
    gbd = gb.to(dev).contiguous()
    graph = aggregate._graph_args(gbd, csr, C, H * W, mode)
    OUT = _new((n, C, H, W), T, dev, layout)
    XC = _new((n, C, H, W), T, dev, layout) if xcopy else None
    ep = None
    if scales is not None or xcopy:
        s = scales or (1.0, 0.0, 0.0)
        base = (s[0], s[1], X0.address if X0 is not None else None, X0.ns if X0 is not None else 0, s[2],
                XC.address if xcopy else None, XC.ns if xcopy else 0)
        ep = _lib.Epilogue(*base) if layout == "nchw" else \
            _lib.EpilogueCl(*base, X0.ps if X0 is not None else 0, XC.ps if xcopy else 0)
    epp = ctypes.byref(ep) if ep is not None else None
    if layout == "nchw":
        code = lib.mrp_film_mean_fwd_t(sp.ENUM[key], X.ptr, X.ns, *graph, OUT.ptr, OUT.ns, epp, _st(dev))
    else:
        code = lib.mrp_film_mean_fwd_cl(sp.ENUM[key], X.ptr, X.ns, X.ps, *graph, OUT.ptr, OUT.ns, OUT.ps, epp, _st(dev))
    assert code == 0, code
    torch.cuda.synchronize(dev)
    return OUT.host(), (XC.host() if xcopy else None)


def agg_backward(dev, g, key, layout, G, X, gb, mode, B=None, want_dgb=True):
    """``mrp_film_mean_bwd_t`` / ``_bwd_cl`` -> (grad_x, grad_gb or None) on the CPU."""
    lib, csr = m.load_library(), g.csr(dev)
    n, C, H, W = X.t.shape
    T = spc.DTYPES[key]
    gbd = gb.to(dev).contiguous()
    graph = aggregate._graph_args(gbd, csr, C, H * W, mode)
    DX = _new((n, C, H, W), T, dev, layout)
    dgb = torch.full((csr.num_edges, C, 2), float("nan"), device=dev) if want_dgb else None
    bp, bn, bps = (B.ptr, B.ns, B.ps) if B is not None else (None, 0, 0)
    if layout == "nchw":
        code = lib.mrp_film_mean_bwd_t(sp.ENUM[key], G.ptr, G.ns, X.ptr, X.ns, *graph, DX.ptr, DX.ns, bp, bn, _p(dgb),
                                       None, _st(dev))
    else:
        nbytes = int(lib.mrp_film_mean_bwd_cl_workspace(csr.num_graphs, csr.max_nodes, csr.graph_kind, C, H * W,
                                                        mode, 1)) if want_dgb else 0
        ws = torch.empty((nbytes + 3) // 4, device=dev) if nbytes > 0 else None
        code = lib.mrp_film_mean_bwd_cl(sp.ENUM[key], G.ptr, G.ns, G.ps, X.ptr, X.ns, X.ps, *graph, DX.ptr, DX.ns,
                                        DX.ps, bp, bn, bps, _p(dgb), None, _p(ws), nbytes, _st(dev))
    assert code == 0, code
    torch.cuda.synchronize(dev)
    return DX.host(), (dgb.cpu() if want_dgb else None)


# ---- 1. the mean's division -------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("key", ALL)
@pytest.mark.parametrize("n", range(2, 17))
def test_mean_division_special_sums(cuda_device, n, key, residual):
    """A complete batch [n, n], gamma = 1, beta = 0: sums that are +0, subnormal, below 2^-124 with a wrong
    fast quotient (n - 1 in 6, 10, 12, 14), +-inf and NaN, in the first, a middle and the last (short) group of
    four destinations — the node-major COMPLETE forward's gate must take the IEEE division for exactly those
    groups; the pixel-major forward divides by IEEE throughout.  Both: the fp32 oracle's bits."""
    c = spc.division_case(n, key)
    T = spc.DTYPES[key]
    want = spc.aggregate_ref(c["graph"], c["x"], c["gb"], self_scale=1.0 if residual else 0.0).to(T)
    for layout in ("nchw", "cl"):
        X = _op(c["x"], cuda_device, layout)
        out, _ = agg_forward(cuda_device, c["graph"], key, layout, X, c["gb"], FILM_MEAN,
                             scales=(1.0, 1.0, 0.0) if residual else None)
        spc.assert_same(out, want, f"{layout} {key} n={n}")


@pytest.mark.parametrize("key", ALL)
@pytest.mark.parametrize("name", ["e", "g"])
@pytest.mark.parametrize("layout", ["nchw", "cl"])
def test_mean_division_regular_and_csr(cuda_device, layout, name, key):
    """REGULAR(4) (case e) and CSR with mixed in-degrees (case g): the same kinds of sums; IEEE division."""
    c = spc.special_sums_case(name, key)
    want = spc.aggregate_ref(c["graph"], c["x"], c["gb"]).to(spc.DTYPES[key])
    out, _ = agg_forward(cuda_device, c["graph"], key, layout, _op(c["x"], cuda_device, layout), c["gb"], FILM_MEAN)
    spc.assert_same(out, want, f"{layout} {key} {name}")


@pytest.mark.parametrize("exp", [-120, 100])
def test_mean_division_scale_pins(cuda_device, exp):
    """Case b in fp32 with x and beta scaled by 2^-120 (sums on both sides of the gate's 2^-124) and by 2^100:
    the oracle's bits on the scaled inputs."""
    g = hc.graph("b")
    x, gb, _, _ = hc.host_inputs("b", "bf16")
    x = x.float() * 2.0 ** exp
    gb = gb.clone()
    gb[:, :, 1] *= 2.0 ** exp
    want = spc.aggregate_ref(g, x, gb)
    sums = spc.aggregate_ref(g, x, gb, "film_sum").abs()
    if exp < 0:
        assert bool((sums < 2.0 ** -124).any()) and bool((sums >= 2.0 ** -124).any())
    out, _ = agg_forward(cuda_device, g, "f32", "nchw", _op(x, cuda_device, "nchw"), gb, FILM_MEAN)
    spc.assert_same(out, want, f"case b x 2^{exp}")


# ---- 2. the sigmoid at saturation ---------------------------------------------------------------------------------
#: (graph sizes, layout, dtype): the <= 8-node and 9-16-node kernels (whole 64-pixel planes: the 16-bit backward
#: of 12 nodes is the matrix-core one) and the pixel-major kernels
SIG = [((5, 5), "nchw", "f32"), ((5, 5), "nchw", "bf16"), ((12,), "nchw", "f32"), ((12,), "nchw", "bf16"),
       ((5, 5), "cl", "f32"), ((12,), "cl", "bf16")]
SIG_C, SIG_HW = 8, 8


def _sig_graph(sizes):
    return hc._frames(list(sizes), 40 + sizes[0])


def _sig_slots(g, C):
    """(edge, channel) slots of the first graph's in-edges from its node 0, one per value of LOGITS."""
    src, dst = (t.numpy() for t in g.edges())
    edges = [e for e in range(len(src)) if src[e] == 0]
    slots = [(e, ch) for e in edges for ch in range(C)][:len(spc.LOGITS)]
    assert len(slots) == len(spc.LOGITS)
    return slots, src, dst


@pytest.mark.parametrize("sizes,layout,key", SIG, ids=str)
def test_sigmoid_saturation_forward(cuda_device, sizes, layout, key):
    """Logits mode against the same kernel fed gb = fl32(sigmoid64(z)), z from LOGITS at chosen slots and randn
    elsewhere: finite, and within the suite's bars (rel_err <= 1e-5 for fp32, assert_elementwise for 16-bit)."""
    g = _sig_graph(sizes)
    T = spc.DTYPES[key]
    gen = torch.Generator().manual_seed(sizes[0])
    x = torch.randn(g.num_nodes(), SIG_C, SIG_HW, SIG_HW, generator=gen).to(T)
    z = torch.randn(g.num_edges(), SIG_C, 2, generator=gen)
    slots, _, _ = _sig_slots(g, SIG_C)
    for i, (e, ch) in enumerate(slots):
        z[e, ch, i % 2] = spc.LOGITS[i]
        z[e, ch, 1 - i % 2] = spc.LOGITS[len(slots) - 1 - i]
    gb = torch.from_numpy(spc.sigmoid64(z.numpy())).float()
    X = _op(x, cuda_device, layout)
    a, _ = agg_forward(cuda_device, g, key, layout, X, z, FILM_MEAN | LOGITS)
    b, _ = agg_forward(cuda_device, g, key, layout, X, gb, FILM_MEAN)
    assert bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(b.float()).all())
    if key == "f32":
        e = rel_err(a.numpy(), b.numpy())
        print("rel_err", e)
        assert e <= 1e-5, e
    else:
        ref = oracle.film_aggregate(x.double(), torch.from_numpy(spc.sigmoid64(z.numpy())), *(t.numpy() for t in g.edges()))
        hc.assert_elementwise(a, ref, T, "logits")
        hc.assert_elementwise(b, ref, T, "gb")


@pytest.mark.parametrize("sizes,layout", [((5, 5), "nchw"), ((12,), "nchw"), ((5, 5), "cl"), ((12,), "cl")], ids=str)
@pytest.mark.parametrize("which", [0, 1], ids=["gamma", "beta"])
def test_sigmoid_saturation_per_slot(cuda_device, sizes, layout, which):
    """fp32 ``film_sum`` with x = 1 on node 0 and 0 elsewhere and every beta logit -inf: the output of
    destination v is gamma(0 -> v) itself (with x = 0 everywhere and one beta per destination: that beta).
    |sigma - sigma64| <= (2.5 2^-23 + 2^-24 |z|) sigma64 + 2^-126; exactly 1 from z = 20 + 24 ln 2 on, exactly
    0 at z = -inf."""
    g = _sig_graph(sizes)
    n = g.num_nodes()
    slots, src, dst = _sig_slots(g, SIG_C)
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(g.num_edges(), SIG_C, 2, generator=gen)
    z[:, :, 1] = float("-inf")
    x = torch.zeros(n, SIG_C, SIG_HW, SIG_HW)
    if which == 0:
        x[0] = 1.0
    for i, (e, ch) in enumerate(slots):
        z[e, ch, which] = spc.LOGITS[i]
    out, _ = agg_forward(cuda_device, g, "f32", layout, _op(x, cuda_device, layout), z, FILM_SUM | LOGITS)
    assert bool(torch.isfinite(out).all())
    for i, (e, ch) in enumerate(slots):
        zv = spc.LOGITS[i]
        got = out[dst[e], ch].double()
        assert bool((got == got[0, 0]).all()), "one value per plane"
        s, s64 = float(got[0, 0]), float(spc.sigmoid64(zv))
        print(f"z = {zv!r}: sigma {s!r}, float64 {s64!r}, bound {float(spc.sigmoid_bound(zv)):.3g}")
        assert abs(s - s64) <= float(spc.sigmoid_bound(zv)), (zv, s, s64)
        if zv >= spc.ONE_FROM:
            assert s == 1.0, (zv, s)
        if zv == float("-inf"):
            assert s == 0.0 and not np.signbit(s), (zv, s)


@pytest.mark.parametrize("sizes,layout,key", SIG, ids=str)
def test_sigmoid_saturation_backward(cuda_device, sizes, layout, key):
    """grad_gb in logits mode (``film_sum``; x and grad_out small powers of two, so every upstream gradient g
    is exact in fp32) against float64: finite, |dz - dz64| <= 1e-6 |g| per slot (the bar ``fast_math.hpp``
    names), exactly 0 at z = +-inf and |z| >= 104."""
    g = _sig_graph(sizes)
    T = spc.DTYPES[key]
    n = g.num_nodes()
    gen = torch.Generator().manual_seed(11 + sizes[0])
    pw = torch.tensor([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0])
    x = pw[torch.randint(0, 6, (n, SIG_C, SIG_HW, SIG_HW), generator=gen)].to(T)
    G = pw[torch.randint(0, 6, (n, SIG_C, SIG_HW, SIG_HW), generator=gen)].to(T)
    z = torch.randn(g.num_edges(), SIG_C, 2, generator=gen)
    slots, src, dst = _sig_slots(g, SIG_C)
    for i, (e, ch) in enumerate(slots):
        z[e, ch, i % 2] = spc.LOGITS[i]
        z[e, ch, 1 - i % 2] = spc.LOGITS[len(slots) - 1 - i]
    up = torch.stack(((G.double()[dst] * x.double()[src]).sum((2, 3)), G.double()[dst].sum((2, 3))), -1)  # (E, C, 2)
    assert torch.equal(up.float().double(), up)
    dz64 = up * torch.from_numpy(spc.dsigmoid64(z.numpy()))
    dx, dz = agg_backward(cuda_device, g, key, layout, _op(G, cuda_device, layout), _op(x, cuda_device, layout), z,
                          FILM_SUM | LOGITS)
    assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(dx.float()).all())
    excess = (dz.double() - dz64).abs() - 1e-6 * up.abs()
    print("largest |dz - dz64| / |g|", float(((dz.double() - dz64).abs() / up.abs().clamp(min=1e-300)).max()))
    assert float(excess.max()) <= 0.0, float(excess.max())
    flat = z.abs() >= 104
    assert int(flat.sum()) >= 8 and not bool(dz[flat].any()), "dz at |z| >= 104 and z = +-inf is exactly 0"


@pytest.mark.parametrize("sizes,layout,key", SIG, ids=str)
def test_nan_logit_is_confined(cuda_device, sizes, layout, key):
    """One NaN gamma logit on edge e, channel c: NaN in out[dst e, c] only; in the backward in grad_gb[e, c, 0]
    and grad_x[src e, c] only; everything else has the clean run's bits."""
    g = _sig_graph(sizes)
    T = spc.DTYPES[key]
    n = g.num_nodes()
    src, dst = (t.numpy() for t in g.edges())
    gen = torch.Generator().manual_seed(5 + sizes[0])
    x, G = (torch.randn(n, SIG_C, SIG_HW, SIG_HW, generator=gen).to(T) for _ in range(2))
    z = torch.randn(g.num_edges(), SIG_C, 2, generator=gen)
    e, ch = g.num_edges() // 3, 5
    zp = z.clone()
    zp[e, ch, 0] = float("nan")
    X, Gd = _op(x, cuda_device, layout), _op(G, cuda_device, layout)
    mode = FILM_MEAN | LOGITS
    clean, _ = agg_forward(cuda_device, g, key, layout, X, z, mode)
    got, _ = agg_forward(cuda_device, g, key, layout, X, zp, mode)
    ref = clean.clone().float()
    ref[dst[e], ch] = float("nan")
    spc.assert_confined(got, clean, ref, f"forward {layout} {key}")
    dx0, dz0 = agg_backward(cuda_device, g, key, layout, Gd, X, z, mode)
    dx1, dz1 = agg_backward(cuda_device, g, key, layout, Gd, X, zp, mode)
    rx, rz = dx0.clone().float(), dz0.clone()
    rx[src[e], ch] = float("nan")
    rz[e, ch, 0] = float("nan")
    spc.assert_confined(dx1, dx0, rx, f"grad_x {layout} {key}")
    spc.assert_confined(dz1, dz0, rz, f"grad_gb {layout} {key}")


# ---- 3. the store to bf16 / fp16 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("key", HALF)
def test_aggregation_store_rounds_once(cuda_device, key, layout):
    """``film_sum`` on complete 3-node graphs with gamma a power of two and beta = 0: out[0] = gamma (x[1] + x[2])
    is each fp32 target of the table exactly, and the store must be torch's CPU cast of it — forward, its
    ``xcopy`` (x's own bits, the NaN included), and grad_x with grad_out in x's role and a grad_x base that
    passes through where the sum is zero."""
    c = spc.store_case(key)
    T = spc.DTYPES[key]
    g, x, gb = c["graph"], c["x"], c["gb"]
    X = _op(x, cuda_device, layout)
    out, xc = agg_forward(cuda_device, g, key, layout, X, gb, FILM_SUM, xcopy=True)
    spc.assert_same(out, c["want"], f"forward {key} {layout}")
    assert torch.equal(spc.bits(xc), spc.bits(x)), "xcopy carries x's bits"
    # backward: grad_out = x; graph 1's grad_out is zero and its base ordinary, graph 0's base zero
    G = x.clone()
    G[3:] = 0.0
    base = torch.zeros_like(x)
    base[3:] = x[3:]
    src, dst = (t.numpy() for t in g.edges())
    with np.errstate(all="ignore"):
        want, _ = oracle.film_aggregate_grads(x.float(), gb, src, dst, G.float(), "film_sum")
    want = (want + base.float()).to(T)
    assert torch.equal(spc.bits(want[0, :2]), spc.bits(c["want"][0, :2])), "the same targets reach grad_x[0]"
    dx, _ = agg_backward(cuda_device, g, key, layout, _op(G, cuda_device, layout), X, gb, FILM_SUM,
                         B=_op(base, cuda_device, layout), want_dgb=False)
    spc.assert_same(dx, want, f"grad_x {key} {layout}")


@pytest.mark.parametrize("mfma", [1, 0], ids=["matrix-core", "valu"])
@pytest.mark.parametrize("key", HALF)
def test_backward_store_rounds_once_12_nodes(cuda_device, key, mfma):
    """The 9-16-node backward's store (the matrix-core kernel: 12 nodes, whole 64-pixel planes; and the VALU
    kernels it replaces, by the knobs): grad_out holds the finite rows of the table on nodes 1 and 2 and zero
    elsewhere, so grad_x[u] = gamma (a + b) + zeros for every other u — torch's CPU cast of the fp32 oracle."""
    T = spc.DTYPES[key]
    a, b, gam, _ = spc.store_table(key)
    g = hc._frames([12], 12)
    src, dst = (t.numpy() for t in g.edges())
    C, H, W = 4, 8, 8
    G = torch.zeros(12, C, H * W, dtype=T)
    rows = [i for i in range(len(a)) if bool(torch.isfinite(a[i].float()) & torch.isfinite(b[i].float()))]
    for j, i in enumerate(rows):
        G[1, 0 if float(gam[i]) == 1.0 else 1, j], G[2, 0 if float(gam[i]) == 1.0 else 1, j] = a[i], b[i]
    G = G.view(12, C, H, W)
    gb = torch.zeros(len(src), C, 2)
    gb[:, :, 0] = 1.0
    gb[:, 1, 0] = 0.25
    x = torch.randn(12, C, H, W, generator=torch.Generator().manual_seed(1)).to(T)
    want, _ = oracle.film_aggregate_grads(x.float(), gb, src, dst, G.float(), "film_sum")
    assert int(torch.isinf(want.to(T)).sum()) > int(torch.isinf(want).sum()), "a finite sum overflows at the store"
    with sc.knobs(compress.compress_path(), bwd_complete_mfma=mfma):
        dx, _ = agg_backward(cuda_device, g, key, "nchw", _op(G, cuda_device, "nchw"), _op(x, cuda_device, "nchw"), gb,
                             FILM_SUM)
    spc.assert_same(dx, want.to(T), f"12 nodes {key} mfma={mfma}")


@pytest.mark.parametrize("fam", ["half", "cl"])
@pytest.mark.parametrize("key", HALF)
def test_compress_store_rounds_once(cuda_device, fam, key):
    """The table through ``mrp_compress_fwd_t`` / ``_bwd_data_t`` (``_fwd_cl`` / ``_bwd_data_cl``) with selection
    weights: y = s x + s agg and gx = gagg = s (gy[c] + gy[c + 16]) are the fp32 targets exactly, stored as torch's
    CPU cast.  The operands include T's subnormals: the matrix cores must keep them.  Weight gradient: 96
    products of T's smallest subnormal (gy) with 1 (x) give gw and gbias the exact fp32 sum."""
    dev = cuda_device
    c = spc.compress_store_case(key)
    n, C, H, W = spc.COMPRESS_STORE_SHAPE
    zero = torch.zeros(C, device=dev)
    cf = dict(x=c["x"], wd=c["wf"].to(dev), bd=zero)
    cd = dict(x=c["x"], wd=c["wd"].to(dev), bd=zero)
    r = _compress_run(fam, key, cf, dev, c["x"], c["a"], c["gy"], ("fwd",))
    spc.assert_same(r["y"], c["y"], f"{fam} {key} y")
    r = _compress_run(fam, key, cd, dev, c["x"], c["a"], c["gy"], ("dgrad",))
    spc.assert_same(r["gx"], c["gx"], f"{fam} {key} gx")
    spc.assert_same(r["ga"], c["gx"], f"{fam} {key} gagg")
    r = _compress_run(fam, key, cf, dev, c["xw"], c["xw"], c["gyw"], ("wgrad",))
    gw, gb = r["gw"], r["gb"]
    print(f"gw[5, 3] {float(gw[5, 3])!r}, gw[5, C + 3] {float(gw[5, C + 3])!r}, gbias[5] {float(gb[5])!r}, want {c['gw53']!r}")
    assert float(gw[5, 3]) == c["gw53"] and float(gw[5, C + 3]) == c["gw53"] and float(gb[5]) == c["gw53"]
    rest = torch.ones(C, dtype=torch.bool)
    rest[5] = False
    assert not bool(gw[rest].any()) and not bool(gb[rest].any())


# ---- 4. poison: aggregation ----------------------------------------------------------------------------------------
def _inputs(name, key):
    x, gb, z, G = hc.host_inputs(name, key if key != "f32" else "bf16")
    return (x.float(), gb, z, G.float()) if key == "f32" else (x, gb, z, G)


@pytest.mark.parametrize("epilogue", ["plain", "mix"])
@pytest.mark.parametrize("key", ALL)
@pytest.mark.parametrize("layout,name", LAYOUT_CASES, ids=str)
def test_forward_confines_poison(cuda_device, layout, name, key, epilogue):
    """One poisoned element per chosen node of x (``special_cases.poison_places``) — "skipped, never multiplied by
    zero": the non-finite set of the output equals the fp32 oracle's, everything else has the clean run's bits.
    "mix": with the self term and x0 (both scales 1), x0 poisoned too, and xcopy, which carries x's bits."""
    g = hc.graph(name)
    x, gb, _, _ = _inputs(name, key)
    T = spc.DTYPES[key]
    places = spc.poison_places(name)
    mix = epilogue == "mix"
    gen = torch.Generator().manual_seed(17)
    x0 = torch.randn(x.shape, generator=gen).to(T)
    x0_place = [(x.shape[0] - 1, 0, 0)]
    scales = (1.0, 1.0, 1.0) if mix else None

    def run(xx, xx0):
        X = _op(xx, cuda_device, layout, name)
        X0 = _op(xx0, cuda_device, layout) if mix else None
        return agg_forward(cuda_device, g, key, layout, X, gb, FILM_MEAN, scales=scales, X0=X0, xcopy=mix)

    clean, _ = run(x, x0)
    for pname, value in spc.POISON.items():
        xp = spc.poisoned(x, places, value)
        x0p = spc.poisoned(x0, x0_place, value) if mix else x0
        ref = spc.aggregate_ref(g, xp, gb, self_scale=1.0 if mix else 0.0)
        if mix:
            ref = ref + x0p.float()
        got, xc = run(xp, x0p)
        spc.assert_confined(got, clean, ref, f"{layout} {name} {key} {epilogue} {pname}")
        if mix:
            assert torch.equal(spc.bits(xc), spc.bits(xp)), "xcopy carries x's bits, the payload included"


@pytest.mark.parametrize("key", ALL)
@pytest.mark.parametrize("layout,name", LAYOUT_CASES, ids=str)
def test_backward_confines_poison(cuda_device, layout, name, key):
    """grad_out poisoned at (v, c, p): grad_x may be non-finite only at (nodes of v's graph, c, p) and grad_gb only
    at (edges of v's graph, c), and both cover the fp32 oracle's set.  x poisoned at (u, c, p): grad_x has the
    clean run's bits, grad_gb is confined to (edges of u's graph, c)."""
    g = hc.graph(name)
    x, gb, _, G = _inputs(name, key)
    _check_backward(cuda_device, g, key, layout, x, G, gb, spc.poison_places(name), f"{layout} {name} {key}", name)


def _check_backward(dev, g, key, layout, x, G, gb, places, what0, name=None):
    n, C, H, W = x.shape
    src, dst = (t.numpy() for t in g.edges())
    ax = torch.zeros(n, C, H * W, dtype=torch.bool)
    ae = torch.zeros(len(src), C, 2, dtype=torch.bool)
    for node, c, p in places:
        lo, hi = spc.graph_nodes(g, node)
        ax[lo:hi, c, p] = True
        ae[torch.from_numpy((dst >= lo) & (dst < hi)), c] = True
    ax = ax.view(n, C, H, W)

    def run(GG, xx):
        return agg_backward(dev, g, key, layout, _op(GG, dev, layout, name), _op(xx, dev, layout, name), gb, FILM_MEAN)

    dx0, dgb0 = run(G, x)
    for pname, value in spc.POISON.items():
        what = f"{what0} {pname}"
        Gp = spc.poisoned(G, places, value)
        with np.errstate(all="ignore"):
            rx, rgb = oracle.film_aggregate_grads(x.float(), gb, src, dst, Gp.float())
        dx, dgb = run(Gp, x)
        strict = [torch.equal(~torch.isfinite(t.float()), ~torch.isfinite(r)) for t, r in ((dx, rx), (dgb, rgb))]
        print(f"{what}: grad_x / grad_gb non-finite exactly where the oracle's are: {strict}")
        spc.assert_confined(dx, dx0, rx, what + " grad_out -> grad_x", ax)
        spc.assert_confined(dgb, dgb0, rgb, what + " grad_out -> grad_gb", ae)
        xp = spc.poisoned(x, places, value)
        with np.errstate(all="ignore"):
            _, rgb = oracle.film_aggregate_grads(xp.float(), gb, src, dst, G.float())
        dx, dgb = run(G, xp)
        assert torch.equal(spc.bits(dx), spc.bits(dx0)), what + ": x -> grad_x changed"
        spc.assert_confined(dgb, dgb0, rgb, what + " x -> grad_gb", ae)


@pytest.mark.parametrize("key", ALL)
@pytest.mark.parametrize("case", sp.AGG_CL)
def test_pixel_major_span_cases_confine_poison(cuda_device, case, key):
    """The pixel-major kernels on ``span_cases.AGG_CL``'s graphs (3 complete graphs of 8 nodes; 2 k-NN(4) graphs of
    12), C = 8, 8 x 8: the forward's non-finite set is the oracle's exactly, the backward's is confined."""
    g = _agraph(case)
    x, G, _, gb = _acase(case, key)
    first = int(g.batch_num_nodes()[0])
    n, C, H, W = x.shape
    places = [(0, C - 1, 1), (first - 1, 3, H * W - 1), (first, 6, 11), (n - 1, 1, 16)]
    X = _op(x, cuda_device, "cl")
    clean, _ = agg_forward(cuda_device, g, key, "cl", X, gb, FILM_MEAN)
    for pname, value in spc.POISON.items():
        xp = spc.poisoned(x, places, value)
        got, _ = agg_forward(cuda_device, g, key, "cl", _op(xp, cuda_device, "cl"), gb, FILM_MEAN)
        spc.assert_confined(got, clean, spc.aggregate_ref(g, xp, gb), f"cl {case} {key} {pname}")
    _check_backward(cuda_device, g, key, "cl", x, G, gb, places, f"cl {case} {key}")


# ---- 4. poison: compress ---------------------------------------------------------------------------------------------
def _cshape(case, n=3):
    """A ``span_cases.COMPRESS`` shape with its node count dropped to n."""
    return (n,) + tuple(sp.COMPRESS[case][1:])


#: (family, dtype, (n, C, H, W)): the ``span_cases.COMPRESS`` shapes at 3 nodes (5 for the pixel-major P = 49 case,
#: whose 64-row stages then cross node boundaries and end in a ragged one).  C = 256: M = C is a multiple of 256, so
#: the forward takes the 256-row form (``gemm_nn_split_w4_mf16``); C = 128 (beyond the table): the data gradient's
#: M = 2C = 256 takes it too, while at C = 64 both run the 128-row form.
COMPRESS = [("hip", "f32", _cshape("n18_c32_p32")), ("split", "f32", _cshape("n18_c64_p32")),
            ("split", "f32", _cshape("n18_c256_p32")), ("split", "f32", (3, 128, 4, 8)),
            ("half", "bf16", _cshape("n18_c32_p32")), ("half", "f16", _cshape("n18_c32_p32")),
            ("cl", "bf16", _cshape("n18_c32_p49", 5)), ("cl", "f16", _cshape("n18_c32_p49", 5))]


def _compress_case(shape, key, dev, seed=0):
    n, C, H, W = shape
    T = spc.DTYPES[key]
    gen = torch.Generator().manual_seed(C * 11 + n + seed)
    w = torch.randn(C, 2 * C, 1, 1, generator=gen) / (2 * C) ** 0.5
    b = torch.randn(C, generator=gen)
    x, a, gy = (torch.randn(n, C, H, W, generator=gen).to(T) for _ in range(3))
    return dict(w=w, b=b, x=x, a=a, gy=gy, wd=w.to(dev), bd=b.to(dev))


def _compress_places(shape):
    """(node, channel, pixel): in a stage that crosses the first node boundary, and the last pixel of all."""
    n, C, H, W = shape
    return [(1, 3, 5), (n - 1, C - 2, H * W - 1)]


def _pixel_mask(shape, places):
    """Every channel of the places' (node, pixel) columns."""
    n, C, H, W = shape
    pix = torch.zeros(n, C, H * W, dtype=torch.bool)
    for node, c, p in places:
        pix[node, :, p] = True
    return pix.view(n, C, H, W)


def _compress_run(fam, key, c, dev, x, a, gy, ops=("fwd", "dgrad", "wgrad")):
    layout = FAMILY[fam][0]
    n, C, H, W = c["x"].shape
    T = spc.DTYPES[key]
    st = _st(dev)
    r = {}
    with sc.knobs("hip" if fam == "hip" else "split") as lib:
        X, A, G = (Dense(t.to(dev), layout) for t in (x, a, gy))
        if "fwd" in ops:
            Y = Dense(torch.empty((n, C, H, W), dtype=T, device=dev), layout)
            assert _call_fwd(fam, lib, key, c, X, A, Y, st) == 0
            r["y"] = Y.read()
        if "dgrad" in ops:
            GX, GA = (Dense(torch.empty((n, C, H, W), dtype=T, device=dev), layout) for _ in range(2))
            assert _call_dgrad(fam, lib, key, c, G, GX, GA, st) == 0
            r["gx"], r["ga"] = GX.read(), GA.read()
        if "wgrad" in ops:
            code, r["gw"], r["gb"] = _call_wgrad(fam, lib, key, c, G, X, A, st)
            assert code == 0
        torch.cuda.synchronize(dev)
    return r


def _nonfinite_like(clean, mask):
    ref = clean.clone().float()
    ref[mask] = float("nan")
    return ref


def _check_compress_poison(run, c, shape, what):
    """``run(x, a, gy)`` -> dict of y, gx, ga, gw, gb: each of x, agg and gy poisoned on its own, with each poison."""
    n, C, H, W = shape
    places = _compress_places(shape)
    pix = _pixel_mask(shape, places)
    clean = run(c["x"], c["a"], c["gy"])
    for pname, value in spc.POISON.items():
        for op in ("x", "a"):
            xs = {"x": c["x"], "a": c["a"]}
            xs[op] = spc.poisoned(xs[op], places, value)
            r = run(xs["x"], xs["a"], c["gy"])
            spc.assert_confined(r["y"], clean["y"], _nonfinite_like(clean["y"], pix), f"{what} {pname} {op} -> y")
            col = torch.zeros(C, 2 * C, dtype=torch.bool)
            for _, ch, _ in places:
                col[:, ch + (C if op == "a" else 0)] = True
            spc.assert_confined(r["gw"], clean["gw"], _nonfinite_like(clean["gw"], col), f"{what} {pname} {op} -> gw")
            assert torch.equal(spc.bits(r["gb"]), spc.bits(clean["gb"])), f"{what} {pname} {op} -> gbias changed"
            for k in ("gx", "ga"):
                assert torch.equal(spc.bits(r[k]), spc.bits(clean[k])), f"{what} {pname} {op} -> {k} changed"
        r = run(c["x"], c["a"], spc.poisoned(c["gy"], places, value))
        assert torch.equal(spc.bits(r["y"]), spc.bits(clean["y"])), f"{what} {pname} gy -> y changed"
        for k in ("gx", "ga"):
            spc.assert_confined(r[k], clean[k], _nonfinite_like(clean[k], pix), f"{what} {pname} gy -> {k}")
        row = torch.zeros(C, 2 * C, dtype=torch.bool)
        rb = torch.zeros(C, dtype=torch.bool)
        for _, o, _ in places:
            row[o], rb[o] = True, True
        spc.assert_confined(r["gw"], clean["gw"], _nonfinite_like(clean["gw"], row), f"{what} {pname} gy -> gw")
        spc.assert_confined(r["gb"], clean["gb"], _nonfinite_like(clean["gb"], rb), f"{what} {pname} gy -> gbias")


@pytest.mark.parametrize("fam,key,shape", COMPRESS, ids=str)
def test_compress_confines_poison(cuda_device, fam, key, shape):
    """Forward: x or agg poisoned at (n, c, p) -> y[n, :, p] non-finite, nothing else.  Data gradient: gy at
    (n, o, p) -> gx[n, :, p] and gagg[n, :, p].  Weight gradient: x at (., c, .) -> column c of gw, gbias clean; gy
    at (., o, .) -> row o of gw and gbias[o].  Everything else has the clean run's bits."""
    c = _compress_case(shape, key, cuda_device)
    _check_compress_poison(lambda x, a, gy: _compress_run(fam, key, c, cuda_device, x, a, gy), c, shape, f"{fam} {key}")


#: (dtype, (n, C, H, W), channels_last, precision): the Python routes — the zero-padding route (C = 48, 7 x 7), the
#: reduced forms (parts = 2 and 1) of the split product at C = 64 and in the 256-row form (C = 256), and the
#: pixel-major fp32 split kernels with every part count
PY_COMPRESS = [("f32", (3, 48, 7, 7), False, None), ("bf16", (3, 48, 7, 7), False, None),
               ("f32", _cshape("n18_c64_p32"), False, "high"), ("f32", _cshape("n18_c64_p32"), False, "medium"),
               ("f32", _cshape("n18_c256_p32"), False, "high"), ("f32", _cshape("n18_c256_p32"), False, "medium"),
               ("f32", (5, 64, 7, 7), True, None), ("f32", (5, 64, 7, 7), True, "high"), ("f32", (5, 64, 7, 7), True, "medium"),
               ("f32", _cshape("n18_c256_p32"), True, None)]


def _py_compress(c, dev, x, a, gy, cl, precision):
    f = (lambda t: t.to(dev).contiguous(memory_format=CL)) if cl else (lambda t: t.to(dev))
    x, a, gy = f(x), f(a), f(gy)
    with sc.knobs("split"):
        y = compress._fwd(c["wd"], c["bd"], x, a, cl=cl, precision=precision)
        gx, ga = compress._bwd_data(c["wd"], gy, cl=cl, precision=precision)
        gw, gb = compress._bwd_weight(gy, x, a, True, c["wd"], c["bd"], cl=cl, precision=precision)
        torch.cuda.synchronize(dev)
    C = x.shape[1]
    return dict(y=y.cpu().contiguous(), gx=gx.cpu().contiguous(), ga=ga.cpu().contiguous(),
                gw=gw.reshape(C, 2 * C).cpu(), gb=gb.cpu())


@pytest.mark.parametrize("key,shape,cl,precision", PY_COMPRESS, ids=str)
def test_compress_python_routes_confine_poison(cuda_device, key, shape, cl, precision):
    """The same contract, every poison on x, agg and gy each on its own, through ``compress.py``: the zero-padded
    route, ``mrp_compress_*_split_p`` with parts 2 and 1, ``mrp_compress_*_split_cl`` with parts 3, 2 and 1."""
    c = _compress_case(shape, key, cuda_device, seed=1)
    _check_compress_poison(lambda x, a, gy: _py_compress(c, cuda_device, x, a, gy, cl, precision), c, shape,
                           f"python {key} {shape} cl={cl} {precision}")


# ---- 4. poison: encoder ------------------------------------------------------------------------------------------------
def _layers(c, dev):
    l1, l2 = torch.nn.Linear(9, c["C"]), torch.nn.Linear(c["C"], 2 * c["C"])
    with torch.no_grad():
        l1.weight.copy_(c["w1"]), l1.bias.copy_(c["b1"]), l2.weight.copy_(c["w2"]), l2.bias.copy_(c["b2"])
    return l1.to(dev), l2.to(dev)


def _encode(route, c, l1, l2, pose, dev):
    """(z (E, 2C), h (E, C) or None) on the CPU through one route."""
    lib, st = m.load_library(), _st(dev)
    E, C = c["E"], c["C"]
    pose = pose.to(dev).contiguous()
    z = torch.full((E, 2 * C), 7.0, device=dev)
    w1, b1, w2, b2 = (t.detach().contiguous() for t in (l1.weight, l1.bias, l2.weight, l2.bias))
    if route == "hidden_logits":
        h = torch.full((E, C), 7.0, device=dev)
        assert lib.mrp_edge_hidden_fwd(_p(pose), _p(w1), _p(b1), E, C, _p(h), st) == 0
        assert lib.mrp_edge_logits_fwd(_p(h), E, C, _p(w2), _p(b2), _p(z), st) == 0
    elif route == "split":
        h = None
        assert lib.mrp_edge_encoder_fwd_split(_p(pose), _p(m.encoder.packed_weights(l1, l2)), _p(b2), E, C, _p(z), st) == 0
    elif route == "split_train":
        hT = torch.full((C, E), 7.0, device=dev)
        assert lib.mrp_edge_encoder_fwd_split_train(_p(pose), _p(m.encoder.packed_weights(l1, l2)), _p(b2), E, C, _p(z),
                                                    _p(hT), E, st) == 0
        h = hT.t()
    else:  # "padded": the product route for shapes the split kernels do not tile
        before = m.encoder.PATH_COUNTS["split_padded"]
        z = m.encoder.edge_logits(torch.nn.Sequential(l1, torch.nn.ReLU(), l2), pose).detach()
        assert m.encoder.PATH_COUNTS["split_padded"] == before + 1
        h = None
    torch.cuda.synchronize(dev)
    return z.cpu(), (h.cpu().contiguous() if h is not None else None)


ENC = [(E, C, r) for E, C in spc.ENCODER_SHAPES + tuple((E, C) for C, E in sp.ENCODER.values()) for r in ("hidden_logits", "split", "split_train")] + \
    [spc.ENCODER_PADDED + ("padded",)]


@pytest.mark.parametrize("poison", list(spc.POISON))
@pytest.mark.parametrize("E,C,route", ENC, ids=str)
def test_encoder_confines_poison(cuda_device, E, C, route, poison):
    """pose[e, j] poisoned: every logit of row e is non-finite, and h[e, :] wherever the reference's is; no other
    row changes.  (A ReLU written as ``acc > 0 ? acc : 0`` or as an integer max on the bits turns the NaN hidden
    units into 0 and the logits finite.)"""
    c = spc.encoder_case(E, C)
    l1, l2 = _layers(c, cuda_device)
    z0, h0 = _encode(route, c, l1, l2, c["pose"], cuda_device)
    for row, col in zip(c["rows"], c["col"]):
        pose = c["pose"].clone()
        pose[row, col] = spc.POISON[poison]
        href, zref = spc.encoder_ref(c, pose)
        z, h = _encode(route, c, l1, l2, pose, cuda_device)
        az = torch.zeros(E, 2 * C, dtype=torch.bool)
        az[row] = True
        what = f"{route} ({E}, {C}) {poison} pose[{row}, {col}]"
        assert bool((~torch.isfinite(zref[row])).all())
        spc.assert_confined(z, z0, zref, what + " z", az)
        if h is not None:
            ah = torch.zeros(E, C, dtype=torch.bool)
            ah[row] = True
            spc.assert_confined(h, h0, href, what + " h", ah)


# ---- 5. scale equivariance and the split kernels' domain ---------------------------------------------------------------
#: span_cases' split shapes at 3 nodes — C = 64: the 128-row form; C = 256: the forward in the 256-row form — and
#: C = 128, whose data gradient (M = 2C = 256) takes the 256-row form
SCALE_SHAPES = [_cshape("n18_c64_p32"), _cshape("n18_c256_p32"), (3, 128, 4, 8)]


def _split_products(c, shape, dev, cl, parts, sa=0, sb=0):
    """(y, gx, ga, gw, gbias) of the split-bf16 compress with the weight (gy in the weight gradient) scaled by
    2^sa, the features by 2^sb and the bias by 2^(sa + sb)."""
    f = (lambda t: t.to(dev).contiguous(memory_format=CL)) if cl else (lambda t: t.to(dev))
    C = shape[1]
    ka, kb = 2.0 ** sa, 2.0 ** sb
    w = (c["w"] * ka).view(C, 2 * C, 1, 1).to(dev)
    b = (c["b"] * (ka * kb)).to(dev)
    x, a, gy = (f((c[k] * kb).view(shape)) for k in ("x", "a", "gy"))
    gy_a = f((c["gy"] * ka).view(shape))
    precision = {3: "highest", 2: "high"}[parts]
    with sc.knobs("split"):
        y = compress._fwd(w, b, x, a, cl=cl, precision=precision)
        gx, ga = compress._bwd_data(w, gy, cl=cl, precision=precision)
        gw, gb = compress._bwd_weight(gy_a, x, a, True, w, b, cl=cl, precision=precision)
        torch.cuda.synchronize(dev)
    return dict(y=(y.cpu().contiguous(), sa + sb), gx=(gx.cpu().contiguous(), sa + sb), ga=(ga.cpu().contiguous(), sa + sb),
                gw=(gw.reshape(C, 2 * C).cpu(), sa + sb), gb=(gb.cpu(), sa))


@pytest.mark.parametrize("shape", SCALE_SHAPES, ids=str)
@pytest.mark.parametrize("parts", [3, 2])
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "cl"])
def test_split_compress_is_scale_equivariant(cuda_device, cl, parts, shape):
    """Operands sign (0.25 + |randn|); scaled by 2^sa (weight side), 2^sb (feature side), the bias by 2^(sa + sb):
    the result is 2^(sa + sb) x the unscaled one, bit for bit, for every pair of ``special_cases.scale_pairs`` —
    no hidden absolute threshold, no flushed part."""
    n, C, H, W = shape
    c = spc.scale_case(n, C, H * W)
    base = _split_products(c, shape, cuda_device, cl, parts)
    for sa, sb in spc.scale_pairs(C):
        got = _split_products(c, shape, cuda_device, cl, parts, sa, sb)
        for k, (t, e) in got.items():
            want = base[k][0] * 2.0 ** e
            assert bool(torch.isfinite(want).all()) and bool((want != 0).all())
            assert torch.equal(spc.bits(t), spc.bits(want)), \
                f"{k} {shape} cl={cl} parts={parts} (2^{sa}, 2^{sb}): {int((spc.bits(t) != spc.bits(want)).sum())} of {t.numel()} differ"


@pytest.mark.parametrize("E,C", spc.ENCODER_SHAPES)
def test_split_encoder_is_scale_equivariant(cuda_device, E, C):
    """W1 scaled by 2^sa, pose by 2^sb, b1 and b2 by 2^(sa + sb): z is 2^(sa + sb) x the unscaled one, bit for bit."""
    c = spc.encoder_scale_case(E, C)
    l1, l2 = _layers(c, cuda_device)
    z0, _ = _encode("split", c, l1, l2, c["pose"], cuda_device)
    assert bool((z0 != 0).all())
    for sa, sb in spc.ENC_SCALE_PAIRS:
        cs = spc.encoder_scaled(c, sa, sb)
        l1s, l2s = _layers(cs, cuda_device)
        z, _ = _encode("split", cs, l1s, l2s, cs["pose"], cuda_device)
        assert torch.equal(spc.bits(z), spc.bits(z0 * 2.0 ** (sa + sb))), f"({E}, {C}) (2^{sa}, 2^{sb})"


@pytest.mark.parametrize("shape", SCALE_SHAPES, ids=str)
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "cl"])
def test_split_compress_upper_edge(cuda_device, cl, shape):
    """One finite element of x, then of gy, at 0x7f7f8000 = 2^128 - 2^119 (it rounds to a bf16 infinity, its
    residual is -inf, the next part NaN): y[n, :, p] (gx[n, :, p] and gagg[n, :, p]) is non-finite, everything else
    has the clean run's bits."""
    n, C, H, W = shape
    c = spc.scale_case(n, C, H * W)
    base = _split_products(c, shape, cuda_device, cl, 3)
    c2 = dict(c, x=c["x"].clone(), gy=c["gy"].clone())
    c2["x"][1, 7, 9] = spc.from_bits(spc.TOP)
    c2["gy"][1, 7, 9] = spc.from_bits(spc.TOP)
    got = _split_products(c2, shape, cuda_device, cl, 3)
    mask = torch.zeros(n, C, H * W, dtype=torch.bool)
    mask[1, :, 9] = True
    for k in ("y", "gx", "ga"):
        spc.assert_confined(got[k][0], base[k][0], _nonfinite_like(base[k][0], mask.view(n, C, H, W)),
                            f"upper edge {k} {shape} cl={cl}")
