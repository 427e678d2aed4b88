"""The max-pooled FiLM aggregation on the GPU against the torch restatement of its definition
(tests/max_cases.py).  Operands on the 2^-3 lattice make every message and every gradient sum exact in
fp32 (and the messages exact in bf16 / fp16), so ties are exact ties and results are compared bit for bit."""
import os

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib, aggregate
import max_cases as mc
from conftest import rel_err
from graph_strategies import batches

pytestmark = pytest.mark.gpu

TOL = 1e-5  # the suite's bar (tests/test_gpu_properties.py)
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(INT_VIEW[a.dtype]), b.view(INT_VIEW[b.dtype]))


def run(dev, g, x, gb, G=None, base=None, logits=False, need_dx=True, need_dgb=True):
    """out, dx, dgb of the kernels (the entry points without autograd) for host operands."""
    csr = g.csr(dev)
    flags = _lib.GB_LOGITS if logits else 0
    xd, gbd = x.to(dev), gb.to(dev)
    out = torch.empty_like(xd)
    m.film_max_forward_into(xd, gbd, csr, flags, out)
    if G is None:
        return out.cpu(), None, None
    dx, dgb = m.film_max_backward(G.to(dev), xd, gbd, csr, flags, need_dx, need_dgb,
                                  grad_x_base=base.to(dev) if base is not None else None)
    return out.cpu(), None if dx is None else dx.cpu(), None if dgb is None else dgb.cpu()


def tie_fraction(g, x, gb):
    """On the reference alone: the fraction of exact ties among the elements of rows with two or more entries
    (None: no such row, a tie cannot happen)."""
    mg = mc.margins(g, x, gb)
    return float((mg == 0).double().mean()) if mg.numel() else None


def assert_ties(g, x, gb):
    fr = tie_fraction(g, x, gb)
    assert fr is None or fr >= 0.005


def tied_lattice_operands(g, C, H, W):
    """Lattice operands of the first seed in 0..7 whose reference has >= 0.5 % ties (a one-channel plane of a
    three-node graph has six (gamma, beta) pairs in all: whether they can tie is one draw, not a rate)."""
    for seed in range(8):
        ops = mc.lattice_operands(g, C, H, W, seed)
        fr = tie_fraction(g, ops[0], ops[1])
        if fr is None or fr >= 0.005:
            return ops
    raise AssertionError("no seed in 0..7 gives the tie rate the test is about")


GRAPHS = {
    **{f"complete{n}": (lambda n=n: mc.complete(n)) for n in (1, 2, 3, 5, 8, 9, 12, 16)},
    "knn16_4": lambda: mc.knn(16, 4),
    "knn12_1": lambda: mc.knn(12, 1),
    "knn9_8": lambda: mc.knn(9, 8),
    "ragged_simple": mc.ragged_simple,
    "general_csr": mc.general_csr,
    "masked_small": mc.masked_small,
}
# ragged channel blocks, single-element slices (7x7), 16 / 32 / 64 lanes per plane with the plane split
SHAPES = [(1, 8, 8), (3, 7, 7), (17, 8, 8), (40, 16, 16), (8, 32, 32)]
# each graph with four of the five shapes (the one left out rotates): 56 cases, not the full product
LATTICE_CASES = [(name, SHAPES[(i + s) % 5]) for i, name in enumerate(GRAPHS) for s in range(4)]


@pytest.mark.parametrize("name,shape", LATTICE_CASES, ids=[f"{n}-{s[0]}x{s[1]}x{s[2]}" for n, s in LATTICE_CASES])
def test_lattice_bit_equal_fp32(cuda_device, name, shape):
    g = GRAPHS[name]()
    C, H, W = shape
    x, gb, G, base = tied_lattice_operands(g, C, H, W)
    assert_ties(g, x, gb)
    kinds = {"ragged_simple": _lib.GRAPH_SIMPLE, "masked_small": _lib.GRAPH_SIMPLE, "general_csr": _lib.GRAPH_CSR, "knn16_4": _lib.graph_regular(4),
             "knn12_1": _lib.graph_regular(1), "knn9_8": _lib.graph_regular(8)}
    assert g.csr(cuda_device).graph_kind == kinds.get(name, _lib.GRAPH_COMPLETE)
    ref_out, ref_dx, ref_dgb = mc.reference(g, x, gb, G)
    out, dx, dgb = run(cuda_device, g, x, gb, G)
    assert bits_equal(out, ref_out)
    assert bits_equal(dx, ref_dx)
    assert bits_equal(dgb, ref_dgb)
    _, dxb, dgb2 = run(cuda_device, g, x, gb, G, base=base)
    assert bits_equal(dxb, ref_dx + base)
    assert bits_equal(dgb2, ref_dgb)


def test_reference_fp32_equals_float64_and_has_ties():
    """The lattice claim itself, on the reference alone: the fp32 restatement is exact."""
    g = mc.complete(5, B=2)
    x, gb, G, _ = mc.lattice_operands(g, 3, 16, 16, seed=1)
    r32 = mc.reference(g, x, gb, G)
    r64 = mc.reference(g, x, gb, G, dtype=torch.float64)
    for a, b in zip(r32, r64):
        assert torch.equal(a.double(), b)
    assert_ties(g, x, gb)


def test_parallel_edges_are_separate_candidates(cuda_device):
    g = mc.general_csr()
    x, gb, _, _ = mc.lattice_operands(g, 8, 8, 8, seed=2)
    ones = torch.ones_like(x)
    _, _, wins = mc.reference(g, x, gb, ones)  # d beta = the number of pixels an entry wins
    assert wins[0, :, 1].sum() > 0 and wins[2, :, 1].sum() > 0  # both 0 -> 1 edges win somewhere
    _, _, dgb = run(cuda_device, g, x, gb, ones)
    assert bits_equal(dgb, wins)


@pytest.mark.parametrize("name", ["complete8", "complete12", "knn16_4", "general_csr", "masked_small"])
def test_outputs_wanted_separately(cuda_device, name):
    g = GRAPHS[name]()
    x, gb, G, base = mc.lattice_operands(g, 5, 8, 8, seed=3)
    _, dx, dgb = run(cuda_device, g, x, gb, G, base=base)
    _, dx1, none1 = run(cuda_device, g, x, gb, G, base=base, need_dgb=False)
    _, none2, dgb2 = run(cuda_device, g, x, gb, G, base=base, need_dx=False)
    assert none1 is None and none2 is None
    assert bits_equal(dx1, dx) and bits_equal(dgb2, dgb)


@pytest.mark.parametrize("name", ["complete8", "complete16", "ragged_simple"])
@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
def test_strided_operands(cuda_device, name, T):
    g = GRAPHS[name]()
    C, H, W = 6, 8, 8
    x, gb, G, base = mc.lattice_operands(g, C, H, W, seed=4)
    dev = cuda_device
    csr = g.csr(dev)
    N = x.shape[0]
    ref_out, ref_dx, ref_dgb = mc.reference(g, x, gb, G)
    xbuf = torch.full((N, 2 * C, H, W), 7.0, device=dev, dtype=T)
    xbuf[:, :C] = x.to(dev)
    cat = torch.full((N, 2 * C, H, W), -5.0, device=dev, dtype=T)
    m.film_max_forward_into(xbuf[:, :C], gb.to(dev), csr, 0, cat[:, C:])
    assert bits_equal(cat[:, C:], ref_out.to(T))
    assert bool((cat[:, :C] == -5.0).all()) and bool((xbuf[:, C:] == 7.0).all())  # the other halves: untouched
    gbuf = torch.full((N, 2 * C, H, W), 3.0, device=dev, dtype=T)
    gbuf[:, C:] = G.to(dev)
    gbuf[:, :C] = base.to(dev)
    dx, dgb = m.film_max_backward(gbuf[:, C:], xbuf[:, :C], gb.to(dev), csr, 0, True, True, grad_x_base=gbuf[:, :C])
    assert bits_equal(dx, (ref_dx + base).to(T))
    assert bits_equal(dgb, ref_dgb)
    # the autograd form of the same composition
    xd = x.to(dev).to(T).requires_grad_(True)
    gbd = gb.to(dev).requires_grad_(True)
    buf = aggregate.film_max_cat(xd, gbd, csr)
    assert bits_equal(buf[:, :C], x.to(T)) and bits_equal(buf[:, C:], ref_out.to(T))
    buf.backward(gbuf)
    assert bits_equal(xd.grad, (ref_dx + base).to(T)) and bits_equal(gbd.grad, ref_dgb)


@pytest.mark.parametrize("n", [5, 8, 12, 16])
@pytest.mark.parametrize("T", [torch.bfloat16, torch.float16])
def test_16_bit_contract(cuda_device, n, T):
    g = mc.complete(n)
    x, gb, G, base = mc.lattice_operands(g, 9, 16, 16, seed=5)
    assert_ties(g, x, gb)
    key = {torch.bfloat16: "bf16", torch.float16: "f16"}[T]
    before = aggregate.PATH_COUNTS["max_fwd_" + key], aggregate.PATH_COUNTS["max_bwd_" + key]
    out, dx, dgb = run(cuda_device, g, x.to(T), gb, G.to(T), base=base.to(T))
    assert (aggregate.PATH_COUNTS["max_fwd_" + key], aggregate.PATH_COUNTS["max_bwd_" + key]) == \
        (before[0] + 1, before[1] + 1)
    assert out.dtype == T and dx.dtype == T and dgb.dtype == torch.float32
    # the reference, cast once (the lattice values are 16-bit values: widening them changes nothing)
    ref_out, ref_dx, ref_dgb = mc.reference(g, x, gb, G, base=base)
    assert bits_equal(out, ref_out.to(T)) and bits_equal(dx, ref_dx.to(T)) and bits_equal(dgb, ref_dgb)
    # the fp32 kernels on the widened input, cast
    out32, dx32, dgb32 = run(cuda_device, g, x.to(T).float(), gb, G.to(T).float(), base=base.to(T).float())
    assert bits_equal(out, out32.to(T)) and bits_equal(dx, dx32.to(T)) and bits_equal(dgb, dgb32)


def _logits_operands(g, C, H, W, T):
    """The first seed in 0..15 whose float64 reference separates best and runner-up by >= 2^-16 (relative to
    max(|best|, 1)) at every output element: about 6x the kernel sigmoid's distance from float64's, so no
    near-tie can be routed differently without being wrong.  A condition on the inputs, from the reference."""
    for seed in range(16):
        gen = torch.Generator().manual_seed(seed)
        x = torch.randn(g.num_nodes(), C, H, W, generator=gen).to(T).float()
        z = 2.0 * torch.randn(g.num_edges(), C, 2, generator=gen)
        G = torch.randn(x.shape, generator=gen).to(T).float()
        mg = mc.margins(g, x, z, logits=True)
        if mg.numel() == 0 or float(mg.min()) >= 2.0 ** -16:
            return x, z, G
    return None


@pytest.mark.parametrize("name", ["complete8", "complete16", "knn8_4", "knn16_4"])
@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
def test_logits_random_operands(cuda_device, name, T):
    g = {"knn8_4": lambda: mc.knn(8, 4)}.get(name, GRAPHS.get(name))()
    ops = _logits_operands(g, 4, 8, 8, T)
    assert ops is not None, "no seed in 0..15 meets the margin condition"
    x, z, G = ops  # fp32 tensors holding values of T
    r_out, r_dx, r_dz = mc.reference(g, x, z, G, logits=True, dtype=torch.float64)
    out, dx, dz = run(cuda_device, g, x, z, G, logits=True)
    assert rel_err(out.numpy(), r_out.numpy()) <= TOL
    assert rel_err(dx.numpy(), r_dx.numpy()) <= TOL
    assert rel_err(dz.numpy(), r_dz.numpy()) <= TOL
    if T != torch.float32:
        # 16-bit features: the fp32 arithmetic above on the widened input, rounded once at each store
        out_t, dx_t, dz_t = run(cuda_device, g, x.to(T), z, G.to(T), logits=True)
        assert bits_equal(out_t, out.to(T)) and bits_equal(dx_t, dx.to(T))
        assert rel_err(dz_t.numpy(), r_dz.numpy()) <= TOL


def test_special_values(cuda_device):
    g = mc.complete(5, B=2)
    C, H, W = 4, 8, 8
    x, gb, G, _ = mc.lattice_operands(g, C, H, W, seed=6)
    gb[:, :, 0].clamp_(min=0.125)  # gamma > 0: an infinite x gives an infinite message, not 0 * inf
    G[G == 0] = 0.5
    clean_out, clean_dx, clean_dgb = run(cuda_device, g, x, gb, G)
    xs, gs = x.clone(), gb.clone()
    xs[1, 2, 3, 4] = float("nan")
    xs[7, 0, 0, 1] = float("inf")
    xs[3, 1, 5, 5] = float("-inf")  # loses to every finite message
    gs[9, 3, 0] = float("nan")  # edge 9 = 2 -> 1 of graph 0, channel 3: every pixel of its message
    gs[25, 1, 0] = float("inf")  # edge 25 = 6 -> 7 (graph 1), channel 1
    r_out, r_dx, r_dgb = mc.reference(g, xs, gs, G)
    out, dx, dgb = run(cuda_device, g, xs, gs, G)
    for got, ref in ((out, r_out), (dx, r_dx), (dgb, r_dgb)):
        assert torch.equal(torch.isnan(got), torch.isnan(ref))
        assert torch.equal(torch.isinf(got), torch.isinf(ref))
        fin = torch.isfinite(ref)
        assert torch.equal(got[fin], ref[fin])
    assert torch.isfinite(r_out[:5, 1, 5, 5]).all()  # the -inf message lost at every destination of its graph
    # only the planted (destination, channel, pixel) positions changed bits in the forward
    changed = out.view(torch.int32) != clean_out.view(torch.int32)
    planted = torch.zeros_like(changed)
    planted[[0, 2, 3, 4], 2, 3, 4] = True  # x[1] NaN: every other node of graph 0
    planted[[5, 6, 8, 9], 0, 0, 1] = True  # x[7] inf: every other node of graph 1
    planted[1, 3] = True  # gamma NaN on 2 -> 1
    planted[7, 1] = True  # gamma inf on 6 -> 7
    planted[[0, 1, 2, 4], 1, 5, 5] = True  # x[3] -inf: where node 3 had won, the runner-up takes over
    assert not bool((changed & ~planted).any())
    # an all -inf row gives -inf
    xm = x.clone()
    xm[:5, 0, 2, 2] = float("-inf")
    out_m, _, _ = run(cuda_device, g, xm, gb)
    assert bool((out_m[:5, 0, 2, 2] == float("-inf")).all())
    assert bits_equal(out_m, mc.reference(g, xm, gb)[0])


def test_deterministic(cuda_device):
    g = mc.knn(16, 4, B=3)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(g.num_nodes(), 12, 16, 16, generator=gen)
    z = torch.randn(g.num_edges(), 12, 2, generator=gen)
    G = torch.randn(x.shape, generator=gen)
    a = run(cuda_device, g, x, z, G, logits=True)
    b = run(cuda_device, g, x, z, G, logits=True)
    for p, q in zip(a, b):
        assert bits_equal(p, q)


def test_autograd_and_channels_last(cuda_device):
    g = mc.complete(8)
    x, gb, G, _ = mc.lattice_operands(g, 8, 8, 8, seed=8)
    ref_out, ref_dx, ref_dgb = mc.reference(g, x, gb, G)
    csr = g.csr(cuda_device)
    for fmt in (torch.contiguous_format, torch.channels_last):
        xd = x.to(cuda_device).contiguous(memory_format=fmt).requires_grad_(True)
        gbd = gb.to(cuda_device).requires_grad_(True)
        out = m.film_max(xd, gbd, csr)
        out.backward(G.to(cuda_device))
        assert bits_equal(out.contiguous(), ref_out) and bits_equal(xd.grad.contiguous(), ref_dx)
        assert bits_equal(gbd.grad, ref_dgb)


SETTINGS = settings(max_examples=int(os.environ.get("MRP_PROPERTY_EXAMPLES", "40")), deadline=None,
                    derandomize=not os.environ.get("MRP_PROPERTY_HUNT"), database=None,
                    suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large,
                                           HealthCheck.function_scoped_fixture])


def _edges_per_graph(bnn, dst):
    goff = np.concatenate([[0], np.cumsum(bnn)])
    dst = np.asarray(dst, np.int64)
    return [int(((dst >= goff[i]) & (dst < goff[i + 1])).sum()) for i in range(len(bnn))]


@SETTINGS
@given(batches(max_deg=16), st.integers(1, 20), st.sampled_from([(1, 1), (3, 5), (7, 7), (8, 8), (4, 16)]),
       st.integers(0, 2 ** 31 - 1))
def test_arbitrary_graphs_bit_equal(cuda_device, case, C, hw, seed):
    """Batches of <= 16-node graphs with in-degree <= 16: multi-edges, self-loops, zero in-degree, empty graphs."""
    bnn, src, dst = case
    g = m.RobotGraph(src, dst, num_nodes=int(sum(bnn)), batch_num_nodes=bnn,
                     batch_num_edges=_edges_per_graph(bnn, dst))
    if g.num_nodes() == 0:
        return
    x, gb, G, _ = mc.lattice_operands(g, C, hw[0], hw[1], seed % 1000)
    ref = mc.reference(g, x, gb, G)
    got = run(cuda_device, g, x, gb, G)
    for a, b in zip(got, ref):
        assert bits_equal(a, b)


# ------------------------------------------------------------------------------------------------ the model
def _frames(B, n, seed):
    # robots within a metre or so of each other: the encoder's logits stay O(1).  (At tens of metres its sigmoid
    # saturates to exactly 1.0 in float64 too, and saturated messages tie exactly: no seed could separate them.)
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.uniform(-1, 1, (B, n, 3)), rng.standard_normal((B, n, 4))], 2).astype(np.float32)


def _stack(C, layers, combine):
    import types
    torch.manual_seed(0)
    return m.GCNStack(types.SimpleNamespace(feature_dim=C, gcn_mode="film_max", gcn_layers=layers,
                                            gcn_combine=combine, gcn2_alpha=0.25))


def _layer1_logits(net, pose):
    import torch.nn.functional as F
    L = net.gcn1.edge_encoder.layers
    with torch.no_grad():
        hid = F.relu(F.linear(pose.double().cpu(), L[0].weight.double().cpu(), L[0].bias.double().cpu()))
        return F.linear(hid, L[2].weight.double().cpu(), L[2].bias.double().cpu()).view(pose.shape[0], -1, 2)


def _model_inputs(net, g, pose, C, H, W, T):
    """Features of the first seed in 0..15 that meets test_logits_random_operands' margin condition on layer
    1's messages (float64, from the reference alone)."""
    z1 = _layer1_logits(net, pose)
    for seed in range(16):
        gen = torch.Generator().manual_seed(seed)
        x = torch.randn(g.num_nodes(), C, H, W, generator=gen).to(T).float()
        mg = mc.margins(g, x, z1, logits=True)
        if mg.numel() == 0 or float(mg.min()) >= 2.0 ** -16:
            return x, torch.randn(x.shape, generator=gen)
    raise AssertionError("no seed in 0..15 meets the margin condition")


def _check_model(dev, net, g, pose, x, G, layers, combine):
    net = net.to(dev)
    params = {k: v.detach() for k, v in net.named_parameters()}
    xd = x.to(dev).requires_grad_(True)
    before = aggregate.PATH_COUNTS["max_fwd_f32"], aggregate.PATH_COUNTS["max_bwd_f32"]
    out = net(g, xd)
    out.backward(G.to(dev))
    assert aggregate.PATH_COUNTS["max_fwd_f32"] == before[0] + layers
    assert aggregate.PATH_COUNTS["max_bwd_f32"] == before[1] + layers
    r_out, r_dx, r_p = mc.stack_reference(params, g, x, pose, G, layers, combine, 0.25)
    assert rel_err(out.detach().cpu().numpy(), r_out.numpy()) <= TOL
    assert rel_err(xd.grad.cpu().numpy(), r_dx.numpy()) <= TOL
    for k, p in net.named_parameters():
        assert rel_err(p.grad.cpu().numpy(), r_p[k].numpy()) <= TOL, k
    return out.detach()


@pytest.mark.parametrize("combine", ["cat_compress", "residual", "initial_mix"])
def test_model_stack_fp32(cuda_device, combine):
    C, H, W, layers = 8, 4, 4, 2
    g = m.batch([m.frame_graph(p) for p in _frames(2, 8, seed=3)])
    net = _stack(C, layers, combine)
    pose = g.edata["pose"]
    x, G = _model_inputs(net, g, pose, C, H, W, torch.float32)
    gd = g.to(cuda_device)
    out = _check_model(cuda_device, net, gd, pose, x, G, layers, combine)
    # a channels_last leaf gives the NCHW run's values, forward and backward (copied first, then the same
    # kernels; the layer's dx comes back NCHW and lands in the leaf's gradient)
    grads = {}
    for fmt in (torch.contiguous_format, torch.channels_last):
        net.zero_grad(set_to_none=True)
        leaf = x.to(cuda_device).contiguous(memory_format=fmt).requires_grad_(True)
        o = net(gd, leaf)
        o.backward(G.to(cuda_device))
        grads[fmt] = (o.detach(), leaf.grad, {k: p.grad.clone() for k, p in net.named_parameters()})
    a, b = grads[torch.contiguous_format], grads[torch.channels_last]
    assert bits_equal(b[0].contiguous(), out.contiguous()) and bits_equal(a[0].contiguous(), out.contiguous())
    assert bits_equal(b[1].contiguous(), a[1].contiguous())
    for k in a[2]:
        assert bits_equal(b[2][k], a[2][k]), k


U_BF16 = 2.0 ** -8  # bf16's spacing relative to a value in [1, 2): one rounding moves a value by at most half of it


def _run_stack(net, gd, x, G):
    net.zero_grad(set_to_none=True)
    leaf = x.requires_grad_(True)
    out = net(gd, leaf)
    out.backward(G.to(out.dtype))
    return out.detach(), leaf.grad, {k: p.grad.clone() for k, p in net.named_parameters()}


@pytest.mark.parametrize("combine", ["cat_compress", "residual", "initial_mix"])
def test_model_stack_bf16(cuda_device, combine):
    """bf16 features.  Every store rounds to bf16, so the float64 bar of the fp32 test cannot apply to values
    held in bf16; the yardstick is the same model's fp32 run on the same bf16-valued input and output gradient,
    as tests/test_gpu_half_model.py does, with bounds counted from the roundings (max-abs relative, rel_err).

    Two layers: the 16-bit max kernels run once per layer, forward and backward, and the forward stays within
    three roundings per layer on the value path (aggregate, compress weight or mix product, layer output):
    6 x u/2 = 3 u.  Its gradients are only checked finite: layer 2 selects among layer 1's *rounded* outputs, a
    perturbation of u/2 that no margin on the inputs excludes, so a handful of layer-2 winners legitimately
    differ from the fp32 run's and each moves a gradient element by a whole |gamma G|.

    One layer: the input is identical in both runs, layer 1's margin condition holds, so the winners are the
    fp32 run's and dx and every parameter gradient are compared.  From the loss to any gradient there are at
    most four roundings to bf16 (the scaled output gradient of the mix or the compress data gradient's gx / ga
    store, the saved aggregate that enters the weight gradient, grad_x's store, the final sum of x's two
    gradient terms), each at most u/2 of its value; 4 u allows the sums over a row's <= 7 entries and the
    pixels twice that: bound 4 u of the tensor's largest element."""
    C, H, W = 8, 4, 4
    dev = cuda_device
    g = m.batch([m.frame_graph(p) for p in _frames(2, 8, seed=3)])
    gd = g.to(dev)
    for layers in (2, 1):
        net = _stack(C, layers, combine).to(dev)
        x, G = _model_inputs(net, g, g.edata["pose"], C, H, W, torch.bfloat16)
        G = G.to(torch.bfloat16).float()  # both runs backpropagate the same bf16-valued gradient
        ref = _run_stack(net, gd, x.to(dev), G.to(dev))
        before = aggregate.PATH_COUNTS["max_fwd_bf16"], aggregate.PATH_COUNTS["max_bwd_bf16"]
        got = _run_stack(net, gd, x.to(dev).to(torch.bfloat16), G.to(dev))
        assert got[0].dtype == torch.bfloat16 and got[1].dtype == torch.bfloat16
        assert aggregate.PATH_COUNTS["max_fwd_bf16"] == before[0] + layers
        assert aggregate.PATH_COUNTS["max_bwd_bf16"] == before[1] + layers
        e = rel_err(got[0].float().cpu().numpy(), ref[0].cpu().numpy())
        print(combine, layers, "layers: forward", e, "bar", 3 * layers * U_BF16 / 2)
        assert e <= 3 * layers * U_BF16 / 2
        assert bool(torch.isfinite(got[1]).all()) and all(bool(torch.isfinite(v).all()) for v in got[2].values())
        if layers == 1:
            e = rel_err(got[1].float().cpu().numpy(), ref[1].cpu().numpy())
            print(combine, "dx", e, "bar", 4 * U_BF16)
            assert e <= 4 * U_BF16
            for k in ref[2]:
                e = rel_err(got[2][k].float().cpu().numpy(), ref[2][k].cpu().numpy())
                print(combine, k, e, "bar", 4 * U_BF16)
                assert e <= 4 * U_BF16, k


def test_model_on_a_device_built_range_graph(cuda_device):
    C, H, W, layers = 8, 4, 4, 1
    B, n = 2, 9
    poses = torch.from_numpy(_frames(B, n, seed=5)).to(cuda_device)
    active = torch.ones(B, n, dtype=torch.bool, device=cuda_device)
    active[0, 3] = False
    g = m.frame_batch(poses, max_range=1.2, active=active)
    csr = g.csr(cuda_device)
    assert csr.graph_kind == _lib.GRAPH_SIMPLE and csr.max_in_degree == n - 1
    net = _stack(C, layers, "cat_compress")
    pose = g.edata["pose"].cpu()
    x, G = _model_inputs(net, g, pose, C, H, W, torch.float32)
    _check_model(cuda_device, net, g, pose, x, G, layers, "cat_compress")
