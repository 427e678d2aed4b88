"""The confidence-weighted FiLM aggregation on the GPU (G1-G10 of its issue): bit-for-bit against the mean
where the operators coincide, against the float64 restatement of the definition (tests/wmean_cases.py)
elsewhere.  Shapes and graphs are tests/half_cases.py's; bars are the project's own (1e-5 of max-abs for fp32
tensors, half_cases.assert_elementwise for 16-bit ones, stack_ref.within for the fp32 reductions)."""
import types

import numpy as np
import pytest
import torch

import half_cases as hc
import mrp_gnn_amd as m
import stack_ref
import wmean_cases as wc
from conftest import rel_err
from mrp_gnn_amd import _lib, aggregate, compress

pytestmark = pytest.mark.gpu

TOL = 1e-5
CASES = list(hc.CASES)
KEYS = ["f32", "bf16", "f16"]
bits = hc.bits


def beq(a, b):
    a, b = bits(a), bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def operands(dev, name, key):
    """x as the case hands it to the kernels (a strided / offset view for h, i4, i1), gb, z, G, w on dev."""
    x, gb, z, G, w = wc.inputs(name, key)
    leaf, view = hc.embed(name, x.to(dev))
    return view(leaf), gb.to(dev), z.to(dev), G.to(dev), w.to(dev)


def run_fwd(x, gb, w, csr, mode="mean", logits=False):
    out = torch.empty(tuple(x.shape), device=x.device, dtype=x.dtype)
    m.film_wmean_forward_into(x, gb, w, csr, _lib.GB_LOGITS if logits else 0, out, mode)
    return out


def run_bwd(G, x, gb, w, csr, mode="mean", logits=False, need=(True, True, True), base=None):
    return m.film_wmean_backward(G, x, gb, w, csr, _lib.GB_LOGITS if logits else 0, *need, grad_x_base=base,
                                 mode=mode)


# ---- G1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", CASES)
def test_g1_unit_weights_are_the_mean_bit_for_bit(cuda_device, name, key):
    x, gb, z, _, w = operands(cuda_device, name, key)
    csr = hc.graph(name).csr(cuda_device)
    one = torch.ones_like(w)
    before = aggregate.PATH_COUNTS["wmean_fwd_" + key]
    for logits in (False, True):
        for mode, mmode in (("mean", "film_mean"), ("sum", "film_sum")):
            ours = run_fwd(x, z if logits else gb, one, csr, mode, logits)
            ref = m.film_mean(x, z if logits else gb, csr, mmode, logits=logits)
            assert beq(ours, ref), (logits, mode, float((ours.float() - ref.float()).abs().max()))
    assert aggregate.PATH_COUNTS["wmean_fwd_" + key] == before + 4


# ---- G2 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["a", "b", "d", "e", "f", "g"])
def test_g2_silent_robots_are_inactive_out_edges(cuda_device, name, key):
    x, gb, _, _, w = operands(cuda_device, name, key)
    g = hc.graph(name)
    n = g.num_nodes()
    silent = torch.zeros(n, dtype=torch.bool)
    silent[torch.randperm(n, generator=torch.Generator().manual_seed(5))[:max(1, n // 3)]] = True
    w01 = (~silent).float()[:, None, None].expand_as(w).contiguous().to(cuda_device)
    src, dst = g.edges()
    masked = m.RobotGraph(src, dst, num_nodes=n, batch_num_nodes=g.batch_num_nodes().tolist(),
                          batch_num_edges=g.batch_num_edges().tolist(), edge_active=~silent[src.cpu()])
    mcsr = masked.csr(cuda_device)
    assert mcsr.graph_kind == _lib.GRAPH_SIMPLE
    ours = run_fwd(x, gb, w01, g.csr(cuda_device))
    ref = m.film_mean(x, gb, mcsr, "film_mean")
    assert beq(ours, ref)


# ---- G3, G5 ---------------------------------------------------------------------------------------------
def _check_against_float64(got, r, T, tag):
    out, dx, dgb, dw = got
    if T == torch.float32:
        assert rel_err(out.cpu().numpy(), r["out64"].numpy()) <= TOL, tag
        assert rel_err(dx.cpu().numpy(), r["dx64"].numpy()) <= TOL, tag
    else:
        hc.assert_elementwise(out, r["out64"], T, tag + " out")
        hc.assert_elementwise(dx, r["dx64"], T, tag + " dx")
    return dgb, dw


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", CASES)
def test_g3_random_maps_against_float64(cuda_device, name, key):
    T = wc.KEYS[key]
    x, gb, z, G, w = operands(cuda_device, name, key)
    csr = hc.graph(name).csr(cuda_device)
    before = aggregate.PATH_COUNTS["wmean_bwd_" + key]
    for mode in ("mean", "sum"):
        r = wc.reference(name, key, mode)
        out = run_fwd(x, gb, w, csr, mode)
        dx, dgb, dw = run_bwd(G, x, gb, w, csr, mode)
        assert out.dtype == T and dx.dtype == T and dgb.dtype == torch.float32 and dw.dtype == torch.float32
        dgb, dw = _check_against_float64((out, dx, dgb, dw), r, T, f"{name} {key} {mode}")
        for got, what in ((dgb, "dgb"), (dw, "dw")):
            ok, e = stack_ref.within(got, r[what + "32"], r[what + "64"])
            print(name, key, mode, what, e)
            assert ok, (what, mode, e)
        # logits: the same aggregate from z, the gb gradient as d logits
        outz = run_fwd(x, z, w, csr, mode, logits=True)
        dxz, dz, dwz = run_bwd(G, x, z, w, csr, mode, logits=True)
        _check_against_float64((outz, dxz, dz, dwz), r, T, f"{name} {key} {mode} logits")
        for got, what in ((dz, "dz"), (dwz, "dw")):
            ok, e = stack_ref.within(got, r[what + "32"], r[what + "64"])
            assert ok, (what, mode, "logits", e)
    assert aggregate.PATH_COUNTS["wmean_bwd_" + key] == before + 4


@pytest.mark.parametrize("key", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["a", "d", "e", "g"])
def test_g5_silent_pixels_and_unnamed_rows_are_exact_zeros(cuda_device, name, key):
    x, gb, _, G, w = operands(cuda_device, name, key)
    g = hc.graph(name)
    csr = g.csr(cuda_device)
    n, C, H, W = x.shape
    out = run_fwd(x, gb, w, csr).reshape(n, C, -1)
    silent = [0, (H * W) // 2]  # wmean_cases.weights: every sender is silent there
    assert bool((bits(out[:, :, silent]) == 0).all())  # +0, not -0
    # every D = 0 pixel of every destination, not only the two forced ones
    indptr, src, _ = wc.rows(g)
    wc_ = w.cpu()
    for v in range(n):
        u = torch.as_tensor(src[indptr[v]:indptr[v + 1]].astype(np.int64))
        D = wc_[u].sum(0).reshape(-1) if len(u) else torch.zeros(H * W)
        assert bool((bits(out[v][:, D == 0]) == 0).all())
    # contributions of D = 0 pixels: a gradient that lives only there gives exact zeros everywhere
    Gs = torch.zeros_like(G).reshape(n, C, -1)
    Gs[:, :, silent] = G.reshape(n, C, -1)[:, :, silent]
    dx, dgb, dw = run_bwd(Gs.reshape(G.shape), x, gb, w, csr)
    assert bool((dx == 0).all()) and bool((dw == 0).all()) and bool((dgb == 0).all())
    # grad_gb rows no CSR entry names: a masked graph leaves its inactive edges' rows zero
    srcs, dsts = g.edges()
    mask = torch.ones(g.num_edges(), dtype=torch.bool)
    mask[::3] = False
    masked = m.RobotGraph(srcs, dsts, num_nodes=n, batch_num_nodes=g.batch_num_nodes().tolist(),
                          batch_num_edges=g.batch_num_edges().tolist(), edge_active=mask)
    _, dgbm, _ = run_bwd(G, x, gb, w, masked.csr(cuda_device))
    assert bool((bits(dgbm[~mask.to(cuda_device)]) == 0).all()) and bool((dgbm[mask.to(cuda_device)] != 0).any())


# ---- G4 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["bf16", "f16"])
@pytest.mark.parametrize("name", CASES)
def test_g4_16_bit_forward_is_the_cast_fp32_run(cuda_device, name, key):
    T = wc.KEYS[key]
    x, gb, z, _, w = operands(cuda_device, name, key)
    csr = hc.graph(name).csr(cuda_device)
    for mode in ("mean", "sum"):
        for logits in (False, True):
            p = z if logits else gb
            got = run_fwd(x, p, w, csr, mode, logits)
            ref = run_fwd(x.float().contiguous(), p, w, csr, mode, logits).to(T)
            assert beq(got, ref), (mode, logits)


# ---- G6 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["h", "i4", "i1", "e"])
def test_g6_strided_operands_touch_nothing_else(cuda_device, name, key):
    T = wc.KEYS[key]
    dev = cuda_device
    x, gb, _, G, w = operands(dev, name, key)
    csr = hc.graph(name).csr(dev)
    n, C, H, W = x.shape
    ref_out = run_fwd(x, gb, w, csr)
    ref_dx, ref_dgb, ref_dw = run_bwd(G, x, gb, w, csr)
    # a strided w (one plane of a wider tensor), out and grad_out as second halves of cat buffers
    wbuf = torch.full((n, 3, H, W), 9.0, device=dev)
    wbuf[:, 1] = w
    cat = torch.full((n, 2 * C, H, W), -5.0, device=dev, dtype=T)
    m.film_wmean_forward_into(x, gb, wbuf[:, 1], csr, 0, cat[:, C:])
    assert beq(cat[:, C:], ref_out)
    assert bool((cat[:, :C] == -5.0).all()) and bool((wbuf[:, 0] == 9.0).all()) and bool((wbuf[:, 2] == 9.0).all())
    gbuf = torch.full((n, 2 * C, H, W), 3.0, device=dev, dtype=T)
    gbuf[:, C:] = G
    base = torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(3)).to(T).to(dev)
    gbuf[:, :C] = base
    dx, dgb, dw = run_bwd(gbuf[:, C:], x, gb, wbuf[:, 1], csr, base=gbuf[:, :C])
    dx0, _, _ = run_bwd(G, x, gb, w, csr, base=base)
    assert beq(dx, dx0) and beq(dgb, ref_dgb) and beq(dw, ref_dw)
    if T == torch.float32:
        assert rel_err(dx.cpu().numpy(), (ref_dx + base).cpu().numpy()) <= TOL
    assert bool((gbuf[:, C:] == G).all()) and bool((gbuf[:, :C] == base).all())
    # outputs are exactly their extents: sentinels around flat allocations
    pad = 64
    flat = torch.full((n * C * H * W + 2 * pad,), 77.0, device=dev, dtype=T)
    o = flat[pad:pad + n * C * H * W].view(n, C, H, W)
    m.film_wmean_forward_into(x, gb, w, csr, 0, o)
    assert beq(o, ref_out) and bool((flat[:pad] == 77.0).all()) and bool((flat[-pad:] == 77.0).all())
    # the autograd form of the cat composition
    xd = x.detach().clone().requires_grad_(True)
    gbd = gb.clone().requires_grad_(True)
    wd = w.clone().requires_grad_(True)
    buf = m.film_wmean_cat(xd, gbd, wd, csr)
    assert beq(buf[:, :C], x) and beq(buf[:, C:], ref_out)
    buf.backward(gbuf)
    # (the lower-level call on the same, now dense, operands: a plane sum's order follows the slice width)
    dxa, dgba, dwa = run_bwd(gbuf[:, C:], xd.detach(), gb, w, csr, base=gbuf[:, :C])
    assert beq(xd.grad, dxa) and beq(gbd.grad, dgba) and beq(wd.grad, dwa)
    assert beq(dxa, dx0) and beq(dwa, ref_dw)  # per-element sums: independent of the slice width


# ---- G7 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mean", "sum"])
@pytest.mark.parametrize("name", ["a", "c", "e", "f", "g"])
def test_g7_outputs_wanted_separately_and_deterministic(cuda_device, name, mode):
    x, gb, _, G, w = operands(cuda_device, name, "f32")
    csr = hc.graph(name).csr(cuda_device)
    dx, dgb, dw = run_bwd(G, x, gb, w, csr, mode)
    for i, full in enumerate((dx, dgb, dw)):
        need = tuple(j == i for j in range(3))
        got = run_bwd(G, x, gb, w, csr, mode, need=need)
        assert all(got[j] is None for j in range(3) if j != i)
        assert beq(got[i], full), i
    again = run_bwd(G, x, gb, w, csr, mode)
    assert all(beq(a, b) for a, b in zip(again, (dx, dgb, dw)))
    assert beq(run_fwd(x, gb, w, csr, mode), run_fwd(x, gb, w, csr, mode))
    assert run_bwd(G, x, gb, w, csr, mode, need=(False, False, False)) == (None, None, None)


def test_g7_wide_channels_take_the_workspace_route(cuda_device):
    """More than 16 channels: grad_w is the block-ordered sum of per-block partials (C = 40: three blocks)."""
    dev = cuda_device
    g = hc.graph("b")
    n, _, H, W = hc.shape("b")
    C = 40
    gen = torch.Generator().manual_seed(11)
    x, G = torch.randn(n, C, H, W, generator=gen), torch.randn(n, C, H, W, generator=gen)
    gb = torch.rand(g.num_edges(), C, 2, generator=gen)
    w = wc.weights("b")
    assert m.load_library().mrp_film_wmean_workspace(2, 5, 1, n, g.num_edges(), C, H * W) == 3 * n * H * W * 4
    r64 = wc.backward(g, x.double(), gb.double(), w.double(), G.double())
    r32 = wc.backward(g, x, gb, w, G)
    csr = g.csr(dev)
    dx, dgb, dw = run_bwd(G.to(dev), x.to(dev), gb.to(dev), w.to(dev), csr)
    assert rel_err(dx.cpu().numpy(), r64[1].numpy()) <= TOL
    for got, i in ((dgb, 2), (dw, 3)):
        ok, e = stack_ref.within(got, r32[i], r64[i])
        assert ok, (i, e)
    only = run_bwd(G.to(dev), x.to(dev), gb.to(dev), w.to(dev), csr, need=(False, False, True))[2]
    assert beq(only, dw)


# ---- G8 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "e", "g"])
def test_g8_non_finite_values_are_contained(cuda_device, name):
    x, gb, _, _, w = operands(cuda_device, name, "f32")
    g = hc.graph(name)
    csr = g.csr(cuda_device)
    n, C, H, W = x.shape
    clean = run_fwd(x, gb, w, csr)
    src, dst = (t.cpu() for t in g.edges())
    u = int(src[0])
    consumers = torch.zeros(n, dtype=torch.bool)
    consumers[dst[src == u]] = True
    # a NaN in w[u, p]: the consumers of u at pixel p (every channel), and nothing else
    wn = w.clone()
    wn[u, 1, 1] = float("nan")
    out = run_fwd(x, gb, wn, csr)
    bad = torch.isnan(out).cpu()
    expect = torch.zeros_like(bad)
    expect[consumers, :, 1, 1] = True
    assert torch.equal(bad, expect)
    assert beq(torch.where(expect.to(out.device), torch.zeros_like(out), out),
               torch.where(expect.to(out.device), torch.zeros_like(out), clean))
    # a NaN in x[u, c, p] at a pixel u transmits: the consumers of u at (c, p) only
    p = int(torch.nonzero(w[u].reshape(-1))[0])
    xn = x.clone()
    xn.view(n, C, -1)[u, 2 % C, p] = float("nan")
    out = run_fwd(xn, gb, w, csr)
    bad = torch.isnan(out).cpu().reshape(n, C, -1)
    expect = torch.zeros_like(bad)
    expect[consumers, 2 % C, p] = True
    assert torch.equal(bad, expect)


# ---- G9 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["plain", "cat", "residual", "mix", "compress", "channels_last"])
def test_g9_autograd_routes(cuda_device, route):
    dev = cuda_device
    name = "a"
    g = hc.graph(name)
    csr = g.csr(dev)
    x, gb, z, _, w = wc.inputs(name, "f32")
    n, C, H, W = x.shape
    gen = torch.Generator().manual_seed(21)
    x0 = torch.randn(x.shape, generator=gen)
    conv = torch.nn.Conv2d(2 * C, C, 1)
    Gc = torch.randn(n, 2 * C if route == "cat" else C, H, W, generator=gen)

    def compose(agg, xx, x0_, conv_w, conv_b):
        if route == "cat":
            return torch.cat((xx, agg), 1)
        if route == "residual":
            return xx + agg
        if route == "mix":
            return 0.75 * agg + 0.25 * x0_
        if route == "compress":
            return torch.einsum("oc,nchw->nohw", conv_w.reshape(C, 2 * C), torch.cat((xx, agg), 1)) + \
                conv_b[None, :, None, None]
        return agg

    refs = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        leaves = [t.detach().to(dt).clone().requires_grad_(True) for t in (x, z, w, conv.weight, conv.bias)]
        xx, zz, ww, cw, cb = leaves
        out = compose(wc.forward(g, xx, torch.sigmoid(zz), ww), xx, x0.to(dt), cw, cb)
        out.backward(Gc.to(dt))
        refs[tag] = [out.detach()] + [t.grad for t in leaves]
    xd = x.to(dev)
    if route == "channels_last":
        xd = xd.contiguous(memory_format=torch.channels_last)
    xd = xd.requires_grad_(True)
    zd, wd = z.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    conv = conv.to(dev)
    if route == "cat":
        out = m.film_wmean_cat(xd, zd, wd, csr, logits=True)
    elif route == "residual":
        out = m.film_wmean_residual(xd, zd, wd, csr, logits=True)
    elif route == "mix":
        out = m.film_wmean_mix(xd, zd, wd, csr, x0.to(dev), 0.25, logits=True)
    elif route == "compress":
        assert compress.film_compress_supported(conv, xd)
        out = compress.film_compress(conv, xd, zd, csr, _lib.MODE_FILM_MEAN | _lib.GB_LOGITS, reducer="wmean",
                                     weights=wd)
    else:
        out = m.film_wmean(xd, zd, wd, csr, logits=True)
    out.backward(Gc.to(dev))
    got = [out.detach(), xd.grad, zd.grad, wd.grad, conv.weight.grad, conv.bias.grad]
    names = ["out", "dx", "dz", "dw", "dW", "db"]
    for i, what in enumerate(names):
        if refs["64"][i] is None:
            assert got[i] is None, what
            continue
        ok, e = stack_ref.within(got[i].reshape(refs["64"][i].shape), refs["32"][i], refs["64"][i])
        print(route, what, e)
        assert ok, (what, e)


def test_g9_needs_input_grad_is_honoured(cuda_device):
    dev = cuda_device
    g = hc.graph("b")
    x, gb, _, G, w = (t.to(dev) for t in wc.inputs("b", "f32"))
    csr = g.csr(dev)
    wd = w.clone().requires_grad_(True)
    before = aggregate.PATH_COUNTS["wmean_bwd_f32"]
    out = m.film_wmean(x, gb, wd, csr)
    out.backward(G)
    assert aggregate.PATH_COUNTS["wmean_bwd_f32"] == before + 1
    full = run_bwd(G, x, gb, w, csr)
    assert beq(wd.grad, full[2])
    with pytest.raises(ValueError):
        m.film_wmean(x, gb, w.double(), csr)
    with pytest.raises(ValueError):
        m.film_wmean(x, gb, w[:, :, :4], csr)


# ---- G10 ------------------------------------------------------------------------------------------------
def _frames(B, n, seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.uniform(-1, 1, (B, n, 3)), rng.standard_normal((B, n, 4))], 2).astype(np.float32)


def _opt(C, combine, layers, **kw):
    return types.SimpleNamespace(feature_dim=C, gcn_layers=layers, gcn_combine=combine, gcn2_alpha=0.25, **kw)


@pytest.mark.parametrize("mode", ["film_mean", "film_sum"])
@pytest.mark.parametrize("combine", ["cat_compress", "cat", "residual", "initial_mix"])
def test_g10_stack_on_a_device_built_range_graph(cuda_device, combine, mode):
    dev = cuda_device
    C, H, W = 8, 4, 4
    layers = 1 if combine == "cat" else 2
    B, n = 2, 9
    poses = torch.from_numpy(_frames(B, n, seed=5)).to(dev)
    active = torch.ones(B, n, dtype=torch.bool, device=dev)
    active[0, 3] = False
    g = m.frame_batch(poses, max_range=1.2, active=active)
    assert g.csr(dev).graph_kind == _lib.GRAPH_SIMPLE
    torch.manual_seed(0)
    net = m.GCNStack(_opt(C, combine, layers, gcn_confidence=True, gcn_mode=mode)).to(dev)
    pose = g.edata["pose"].cpu()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B * n, C, H, W, generator=gen)
    G = torch.randn(B * n, 2 * C if combine == "cat" else C, H, W, generator=gen)
    xd = x.to(dev).requires_grad_(True)
    before = aggregate.PATH_COUNTS["wmean_fwd_f32"], aggregate.PATH_COUNTS["wmean_bwd_f32"]
    out = net(g, xd)
    out.backward(G.to(dev))
    assert aggregate.PATH_COUNTS["wmean_fwd_f32"] == before[0] + layers
    assert aggregate.PATH_COUNTS["wmean_bwd_f32"] == before[1] + layers
    params = {k: v.detach() for k, v in net.named_parameters()}
    wmode = "sum" if mode == "film_sum" else "mean"
    r64 = wc.stack_reference(params, g, x, pose, G, layers, combine, 0.25, wmode)
    r32 = wc.stack_reference(params, g, x, pose, G, layers, combine, 0.25, wmode, dtype=torch.float32)
    for got, i, what in ((out, 0, "out"), (xd.grad, 1, "dx")):
        ok, e = stack_ref.within(got, r32[i], r64[i])
        assert ok, (what, e)
    for k, p in net.named_parameters():
        ok, e = stack_ref.within(p.grad, r32[2][k], r64[2][k])
        assert ok, (k, e)
        if "confidence" in k:
            assert float(p.grad.abs().max()) > 0, k


def test_g10_copy_mean_and_explicit_weights(cuda_device):
    dev = cuda_device
    g = hc.graph("b")
    x, _, _, _, w = (t.to(dev) for t in wc.inputs("b", "f32"))
    gd = g.to(dev)
    gcn = m.GCN(types.SimpleNamespace(feature_dim=x.shape[1], gcn_mode="copy_mean")).to(dev)
    assert "confidence" not in gcn._modules
    out = gcn(gd, x, weights=w)
    ones = torch.zeros(g.num_edges(), x.shape[1], 2)
    ones[:, :, 0] = 1.0
    ref = wc.forward(g, x.cpu().double(), ones.double(), w.cpu().double())
    assert rel_err(out.cpu().numpy(), ref.numpy()) <= TOL
    assert beq(gcn(gd, x, weights=torch.ones_like(w)), gcn(gd, x))  # w == 1: the unweighted layer's bits
    assert beq(gcn.forward_cat(gd, x, weights=w)[:, x.shape[1]:], out)
    assert beq(gcn.forward_residual(gd, x, weights=w), x + out)
    with pytest.raises(ValueError, match="gcn_confidence"):
        gcn.confidence_map(x)


def test_g10_state_dict_keys_threshold_and_forbidden_combinations(cuda_device):
    dev = cuda_device
    C = 8
    base = m.GCNStack(_opt(C, "cat_compress", 2))
    off = m.GCNStack(_opt(C, "cat_compress", 2, gcn_confidence=False))
    on = m.GCNStack(_opt(C, "cat_compress", 2, gcn_confidence=True))
    assert list(off.state_dict()) == list(base.state_dict())
    assert not any("confidence" in k for k in base.state_dict())
    extra = set(on.state_dict()) - set(base.state_dict())
    assert extra == {f"gcn{i}.confidence.{p}" for i in (1, 2) for p in ("weight", "bias")}
    assert tuple(on.gcn1.confidence.weight.shape) == (1, C, 1, 1)
    for bad in (dict(gcn_mode="film_max"), dict(gcn_mode="film_attn"), dict(gcn_message_dtype="fp8_e4m3")):
        with pytest.raises(ValueError):
            m.GCN(types.SimpleNamespace(feature_dim=C, gcn_confidence=True, **bad))
        m.GCN(types.SimpleNamespace(feature_dim=C, **bad))  # without the option: as before
    # threshold gating zeroes what it should, and the aggregate is film_wmean of that map
    g = hc.graph("b")
    gd = g.to(dev)
    x = wc.inputs("b", "f32")[0][:, :C].contiguous().to(dev)
    torch.manual_seed(3)
    soft = m.GCN(types.SimpleNamespace(feature_dim=C, gcn_confidence=True)).to(dev)
    hard = m.GCN(types.SimpleNamespace(feature_dim=C, gcn_confidence=True, gcn_confidence_threshold=0.5)).to(dev)
    hard.load_state_dict(soft.state_dict())
    ws, wh = soft.confidence_map(x), hard.confidence_map(x)
    assert ws.shape == (x.shape[0], 1, x.shape[2], x.shape[3]) and ws.dtype == torch.float32
    keep = ws >= 0.5
    assert bool(keep.any()) and bool((~keep).any())
    assert bool((wh[~keep] == 0).all()) and beq(wh[keep], ws[keep])
    z = hard.edge_encoder.logits(gd.edata["pose"])
    assert beq(hard(gd, x), m.film_wmean(x, z, wh, g.csr(dev), logits=True))
    xr = x.clone().requires_grad_(True)
    hard(gd, xr).square().sum().backward()
    assert float(hard.confidence.weight.grad.abs().max()) > 0  # the gradient flows through the kept values


def test_g10_multi_view_model_training_step(cuda_device):
    dev = cuda_device
    C, H, W = 8, 8, 8
    g = m.batch([m.frame_graph(p) for p in _frames(2, 5, seed=2)]).to(dev)
    torch.manual_seed(0)
    net = m.multi_view_dgl_model(_opt(C, "cat_compress", 2, gcn_confidence=True, compress_gcn=True,
                                      multi_gcn=True)).to(dev)
    g.ndata["image"] = torch.randn(10, C, H, W, device=dev)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    net(g).square().mean().backward()
    for k, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert float(net.gcn1.confidence.weight.grad.abs().max()) > 0
    assert float(net.gcn2.confidence.bias.grad.abs().max()) > 0
    opt.step()
    assert not torch.equal(net.gcn1.confidence.weight.detach(), before["gcn1.confidence.weight"])
