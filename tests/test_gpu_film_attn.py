"""The attention-pooled FiLM aggregation on the GPU against the float64 restatement of its definition
(tests/attn_cases.py), at the suite's bar; exact anchors where the operator has them; the 16-bit contract,
strided operands, determinism and the containment of non-finite values bit for bit."""
import os
import types

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib, aggregate
import attn_cases as ac
import max_cases as mc
from conftest import rel_err
from graph_strategies import batches

pytestmark = pytest.mark.gpu

TOL = 1e-5  # the suite's bar (TOL of tests/test_gpu_film_max.py); tests/test_film_attn_cpu.py shows its teeth
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
ULP1 = 2.0 ** -23  # fp32 spacing at 1


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(INT_VIEW[a.dtype]), b.view(INT_VIEW[b.dtype]))


def close(got, ref):
    return rel_err(got.detach().float().cpu().numpy(), ref.numpy()) <= TOL


def run(dev, g, x, gb, G=None, base=None, logits=False, need_dx=True, need_dgb=True, scale=None):
    """out, attn, dx, dgb of the kernels (the entry points without autograd) for host operands."""
    csr = g.csr(dev)
    flags = _lib.GB_LOGITS if logits else 0
    xd, gbd = x.to(dev), gb.to(dev)
    out = torch.empty_like(xd)
    attn = m.film_attn_forward_into(xd, gbd, csr, flags, out, scale)
    if G is None:
        return out.cpu(), attn.cpu(), None, None
    dx, dgb = m.film_attn_backward(G.to(dev), xd, gbd, attn, csr, flags, need_dx, need_dgb,
                                   grad_x_base=base.to(dev) if base is not None else None, scale=scale)
    return out.cpu(), attn.cpu(), None if dx is None else dx.cpu(), None if dgb is None else dgb.cpu()


GRAPHS = {
    **{f"complete{n}": (lambda n=n: mc.complete(n)) for n in (1, 2, 3, 5, 8, 9, 12, 16)},
    "knn16_4": lambda: mc.knn(16, 4),
    "knn12_1": lambda: mc.knn(12, 1),
    "knn9_8": lambda: mc.knn(9, 8),
    "ragged_simple": mc.ragged_simple,
    "general_csr": mc.general_csr,
    "masked_small": mc.masked_small,
}
KINDS = {"ragged_simple": _lib.GRAPH_SIMPLE, "masked_small": _lib.GRAPH_SIMPLE, "general_csr": _lib.GRAPH_CSR,
         "knn16_4": _lib.graph_regular(4), "knn12_1": _lib.graph_regular(1), "knn9_8": _lib.graph_regular(8)}
# one channel; a ragged tile (49 of 64 pixels); a ragged channel chunk; channels over many chunks with a
# remainder; a plane spanning 16 pixel tiles (grad_gb through the workspace)
SHAPES = [(1, 8, 8), (3, 7, 7), (17, 8, 8), (130, 8, 8), (8, 32, 32)]
# each graph with four of the five shapes (the one left out rotates), not the full product
CASES = [(name, SHAPES[(i + s) % 5]) for i, name in enumerate(GRAPHS) for s in range(4)]


@pytest.mark.parametrize("name,shape", CASES, ids=[f"{n}-{s[0]}x{s[1]}x{s[2]}" for n, s in CASES])
def test_against_float64(cuda_device, name, shape):
    g = GRAPHS[name]()
    C, H, W = shape
    assert g.csr(cuda_device).graph_kind == KINDS.get(name, _lib.GRAPH_COMPLETE)
    x, gb, z, G, base = ac.random_operands(g, C, H, W, seed=len(name) + C)
    for logits, w in ((False, gb), (True, z)):
        r_out, r_attn, r_dx, r_dgb = ac.reference(g, x, w, G, logits=logits, dtype=torch.float64)
        out, attn, dx, dgb = run(cuda_device, g, x, w, G, logits=logits)
        errs = [rel_err(a.numpy(), b.numpy()) for a, b in ((out, r_out), (attn, r_attn), (dx, r_dx), (dgb, r_dgb))]
        print(name, shape, "logits" if logits else "plain", errs)
        assert max(errs) <= TOL
        _, _, dxb, dgb2 = run(cuda_device, g, x, w, G, base=base, logits=logits)
        assert close(dxb, r_dx + base.double())
        assert bits_equal(dgb2, dgb)


@pytest.mark.parametrize("shape", [(3, 7, 7), (17, 8, 8), (8, 32, 32)])
def test_in_degree_one_equals_film_max_bit_for_bit(cuda_device, shape):
    """One entry per row: a = 1 and ds = 0 exactly, so the operator is the row's message, as film_max's is."""
    g = mc.knn(12, 1)
    x, gb, G, base = mc.lattice_operands(g, *shape, seed=2)
    dev = cuda_device
    csr = g.csr(dev)
    out, attn, dx, dgb = run(dev, g, x, gb, G, base=base)
    ref_out = torch.empty_like(x, device=dev)
    m.film_max_forward_into(x.to(dev), gb.to(dev), csr, 0, ref_out)
    ref_dx, ref_dgb = m.film_max_backward(G.to(dev), x.to(dev), gb.to(dev), csr, 0, True, True,
                                          grad_x_base=base.to(dev))
    assert bool((attn == 1).all())
    assert bits_equal(out, ref_out) and bits_equal(dx, ref_dx) and bits_equal(dgb, ref_dgb)


@pytest.mark.parametrize("name", ["complete5", "complete16", "knn9_8", "masked_small", "general_csr"])
def test_weights_zero_scale_row_sums_unnamed_rows(cuda_device, name):
    g = GRAPHS[name]()
    C, H, W = 6, 8, 8
    x, gb, _, _, _ = ac.random_operands(g, C, H, W, seed=11)
    indptr, src, eid = ac.rows(g)
    named = torch.zeros(g.num_edges(), dtype=torch.bool)
    named[torch.as_tensor(eid[: int(indptr[-1])].astype(np.int64))] = True
    if name == "masked_small":
        assert not bool(named.all())  # the case that has rows no entry names
    # scale 0: uniform weights, and the output is the mean of the messages
    out0, attn0, _, _ = run(cuda_device, g, x, gb, scale=0.0)
    _, attn, _, _ = run(cuda_device, g, x, gb)
    for v in range(g.num_nodes()):
        lo, hi = int(indptr[v]), int(indptr[v + 1])
        if hi == lo:
            continue
        e = torch.as_tensor(eid[lo:hi].astype(np.int64))
        want = np.float32(1.0) / np.float32(hi - lo)
        ulp = float(np.spacing(want))
        assert float((attn0[e].double() - float(want)).abs().max()) <= 4 * ulp
        assert float((attn[e].double().sum(0) - 1.0).abs().max()) <= 16 * ULP1
    assert bool((attn[~named] == 0).all()) and bool((attn0[~named] == 0).all())
    assert bool((attn[named] >= 0).all())
    mean_ref = mc_mean_reference(g, x, gb)
    assert close(out0, mean_ref)


def mc_mean_reference(g, x, gb):
    """film_mean's definition in float64: the mean of the row's messages (zeros for an empty row)."""
    indptr, src, eid = ac.rows(g)
    xr, gr = x.double(), gb.double()
    outs = []
    for v in range(x.shape[0]):
        lo, hi = int(indptr[v]), int(indptr[v + 1])
        if hi == lo:
            outs.append(torch.zeros(x.shape[1:], dtype=torch.float64))
            continue
        e = torch.as_tensor(eid[lo:hi].astype(np.int64))
        u = torch.as_tensor(src[lo:hi].astype(np.int64))
        outs.append((gr[e, :, 0, None, None] * xr[u] + gr[e, :, 1, None, None]).mean(0))
    return torch.stack(outs)


@pytest.mark.parametrize("n", [5, 8, 12, 16])
@pytest.mark.parametrize("shape", [(4, 8, 8), (40, 16, 16)])
@pytest.mark.parametrize("T", [torch.bfloat16, torch.float16])
def test_16_bit_contract(cuda_device, n, shape, T):
    g = mc.complete(n)
    x, gb, _, G, base = ac.random_operands(g, *shape, seed=5)
    xT, GT, bT = x.to(T), G.to(T), base.to(T)
    key = {torch.bfloat16: "bf16", torch.float16: "f16"}[T]
    before = aggregate.PATH_COUNTS["attn_fwd_" + key], aggregate.PATH_COUNTS["attn_bwd_" + key]
    out, attn, dx, dgb = run(cuda_device, g, xT, gb, GT, base=bT)
    assert (aggregate.PATH_COUNTS["attn_fwd_" + key], aggregate.PATH_COUNTS["attn_bwd_" + key]) == \
        (before[0] + 1, before[1] + 1)
    assert out.dtype == T and dx.dtype == T and dgb.dtype == torch.float32 and attn.dtype == torch.float32
    # the fp32 kernels on the widened input, cast
    out32, attn32, dx32, dgb32 = run(cuda_device, g, xT.float(), gb, GT.float(), base=bT.float())
    assert bits_equal(out, out32.to(T)) and bits_equal(dx, dx32.to(T))
    assert bits_equal(attn, attn32) and bits_equal(dgb, dgb32)
    r = ac.reference(g, xT.float(), gb, GT.float(), base=bT.float(), dtype=torch.float64)
    e = rel_err(dgb.numpy(), r[3].numpy())
    print(n, shape, T, "dgb", e)
    assert e <= TOL


@pytest.mark.parametrize("name", ["complete8", "complete16", "ragged_simple"])
@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
def test_strided_operands(cuda_device, name, T):
    g = GRAPHS[name]()
    C, H, W = 6, 9, 9  # 81 pixels: two tiles, the second ragged; odd strides
    x, gb, _, G, base = ac.random_operands(g, C, H, W, seed=4)
    dev = cuda_device
    csr = g.csr(dev)
    N = x.shape[0]
    d_out, d_attn, d_dx, d_dgb = run(dev, g, x.to(T), gb, G.to(T), base=base.to(T))  # the dense run
    xbuf = torch.full((N, 2 * C, H, W), 7.0, device=dev, dtype=T)
    xbuf[:, :C] = x.to(dev)
    cat = torch.full((N, 2 * C, H, W), -5.0, device=dev, dtype=T)
    attn = m.film_attn_forward_into(xbuf[:, :C], gb.to(dev), csr, 0, cat[:, C:])
    assert bits_equal(cat[:, C:], d_out) and bits_equal(attn, d_attn)
    assert bool((cat[:, :C] == -5.0).all()) and bool((xbuf[:, C:] == 7.0).all())  # the other halves: untouched
    gbuf = torch.full((N, 2 * C, H, W), 3.0, device=dev, dtype=T)
    gbuf[:, C:] = G.to(dev)
    gbuf[:, :C] = base.to(dev)
    # grad_out and the base are the two halves of one buffer (strided reads); grad_x comes back dense
    dx, dgb = m.film_attn_backward(gbuf[:, C:], xbuf[:, :C], gb.to(dev), attn, csr, 0, True, True,
                                   grad_x_base=gbuf[:, :C])
    assert bits_equal(dx, d_dx) and bits_equal(dgb, d_dgb)
    assert bool((xbuf[:, C:] == 7.0).all()) and bits_equal(gbuf[:, C:], G.to(T)) and bits_equal(gbuf[:, :C], base.to(T))
    # the C entry point with a strided grad_x too: written into the first half of a sentinel-filled (N, 2C, H, W)
    # buffer through gx_node_stride, the second half untouched
    dxbuf = torch.full((N, 2 * C, H, W), 9.0, device=dev, dtype=T)
    dgb2 = torch.full((g.num_edges(), C, 2), 9.0, device=dev)
    gbd = gb.to(dev).contiguous()
    lib = _lib.load_library()
    P = H * W
    nbytes = lib.mrp_film_attn_workspace(1, csr.num_graphs, csr.max_nodes, csr.graph_kind, csr.num_nodes,
                                         csr.num_edges, C, P)
    ws = torch.empty(max(nbytes // 4, 1), device=dev)
    code = lib.mrp_film_attn_bwd(aggregate.FEATURE_DTYPES[T], aggregate._ptr(gbuf[:, C:]), 2 * C * P,
                                 aggregate._ptr(xbuf[:, :C]), 2 * C * P, *aggregate._graph_args(gbd, csr, C, P, 0),
                                 aggregate._ptr(dxbuf[:, :C]), 2 * C * P, aggregate._ptr(gbuf[:, :C]), 2 * C * P,
                                 aggregate._ptr(dgb2), ac.default_scale(C), aggregate._ptr(attn), aggregate._ptr(ws),
                                 nbytes, aggregate._stream(dev))
    assert code == 0
    assert bits_equal(dxbuf[:, :C], d_dx) and bits_equal(dgb2, d_dgb)
    assert bool((dxbuf[:, C:] == 9.0).all())
    # the autograd form of the same composition
    xd = x.to(dev).to(T).requires_grad_(True)
    gbd = gb.to(dev).requires_grad_(True)
    buf = aggregate.film_attn_cat(xd, gbd, csr)
    assert bits_equal(buf[:, :C], x.to(T)) and bits_equal(buf[:, C:], d_out)
    buf.backward(gbuf)
    assert bits_equal(xd.grad, d_dx) and bits_equal(gbd.grad, d_dgb)


@pytest.mark.parametrize("name", ["complete8", "complete12", "knn16_4", "general_csr", "masked_small"])
@pytest.mark.parametrize("shape", [(5, 8, 8), (3, 12, 12)])
def test_outputs_wanted_separately(cuda_device, name, shape):
    g = GRAPHS[name]()
    x, _, z, G, base = ac.random_operands(g, *shape, seed=3)
    _, _, dx, dgb = run(cuda_device, g, x, z, G, base=base, logits=True)
    _, _, dx1, none1 = run(cuda_device, g, x, z, G, base=base, logits=True, need_dgb=False)
    _, _, none2, dgb2 = run(cuda_device, g, x, z, G, base=base, logits=True, need_dx=False)
    assert none1 is None and none2 is None
    assert bits_equal(dx1, dx) and bits_equal(dgb2, dgb)


def test_no_channels_gives_zero_weights(cuda_device):
    """C == 0: nothing to score and no kernel runs; the weights handed in are written as zeros."""
    g = mc.general_csr()
    csr = g.csr(cuda_device)
    x = torch.zeros(g.num_nodes(), 0, 4, 4, device=cuda_device)
    attn = torch.full((g.num_edges(), 16), 3.0, device=cuda_device)
    got = m.film_attn_forward_into(x, torch.zeros(g.num_edges(), 0, 2, device=cuda_device), csr, 0,
                                   torch.empty_like(x), attn=attn)
    assert got is attn and bool((attn == 0).all())
    fresh = m.film_attn_forward_into(x, torch.zeros(g.num_edges(), 0, 2, device=cuda_device), csr, 0,
                                     torch.empty_like(x))
    assert bool((fresh == 0).all())


def test_deterministic(cuda_device):
    g = mc.knn(16, 4, B=3)
    x, _, z, G, _ = ac.random_operands(g, 12, 16, 16, seed=7)
    a = run(cuda_device, g, x, z, G, logits=True)
    b = run(cuda_device, g, x, z, G, logits=True)
    for p, q in zip(a, b):
        assert bits_equal(p, q)


def test_special_values_are_contained(cuda_device):
    g = mc.complete(5, B=2)
    C, H, W = 4, 8, 8
    x, gb, _, G, _ = ac.random_operands(g, C, H, W, seed=6)
    gb[:, :, 0].clamp_(min=0.125)  # gamma > 0: an infinite x gives an infinite message, not 0 * inf
    clean = run(cuda_device, g, x, gb, G)
    xs = x.clone()
    xs[1, 2, 3, 4] = float("nan")  # graph 0, pixel 28
    xs[7, 0, 0, 1] = float("inf")  # graph 1, pixel 1
    out, attn, dx, dgb = run(cuda_device, g, xs, gb, G)
    N, E, P = x.shape[0], gb.shape[0], H * W
    node_hit = torch.zeros(N, P, dtype=torch.bool)
    node_hit[:5, 3 * W + 4] = True
    node_hit[5:, 1] = True
    edge_hit = torch.zeros(E, P, dtype=torch.bool)
    edge_hit[:20, 3 * W + 4] = True  # graph 0's edges are 0..19, graph 1's 20..39
    edge_hit[20:, 1] = True
    same_out = (out.view(torch.int32) == clean[0].view(torch.int32)).reshape(N, C, P)
    assert bool(same_out[~node_hit[:, None, :].expand(N, C, P)].all())
    assert bool((attn.view(torch.int32) == clean[1].view(torch.int32))[~edge_hit].all())
    same_dx = (dx.view(torch.int32) == clean[2].view(torch.int32)).reshape(N, C, P)
    assert bool(same_dx[~node_hit[:, None, :].expand(N, C, P)].all())
    assert not bool(torch.isfinite(out[[0, 2, 3, 4], 2, 3, 4]).any())  # every receiver of the NaN
    assert not bool(torch.isfinite(out[[5, 6, 8, 9], 0, 0, 1]).any())  # every receiver of the infinity


def test_autograd_layouts_and_weights(cuda_device):
    g = mc.complete(8)
    C, H, W = 8, 8, 8
    x, gb, z, G, base = ac.random_operands(g, C, H, W, seed=8)
    dev = cuda_device
    csr = g.csr(dev)
    r_out, r_attn, r_dx, r_dz = ac.reference(g, x, z, G, logits=True, dtype=torch.float64)
    res = {}
    for fmt in (torch.contiguous_format, torch.channels_last):
        xd = x.to(dev).contiguous(memory_format=fmt).requires_grad_(True)
        zd = z.to(dev).requires_grad_(True)
        out, attn = m.film_attn(xd, zd, csr, logits=True, return_weights=True)
        assert not attn.requires_grad and tuple(attn.shape) == (g.num_edges(), H * W)
        out.backward(G.to(dev))
        assert close(out, r_out) and close(attn, r_attn) and close(xd.grad, r_dx) and close(zd.grad, r_dz)
        res[fmt] = (out.detach().contiguous(), attn, xd.grad.contiguous(), zd.grad)
    for a, b in zip(res[torch.contiguous_format], res[torch.channels_last]):
        assert bits_equal(a, b)  # copied to NCHW first: the same kernels on the same values
    # the weights returned are the ones the entry point writes
    o2 = torch.empty_like(x, device=dev)
    attn2 = m.film_attn_forward_into(x.to(dev), z.to(dev), csr, _lib.GB_LOGITS, o2)
    assert bits_equal(attn2, res[torch.contiguous_format][1])
    # the concatenated form, with an explicit scale
    xd = x.to(dev).requires_grad_(True)
    zd = z.to(dev).requires_grad_(True)
    buf = m.film_attn_cat(xd, zd, csr, logits=True, scale=0.2)
    Gcat = torch.cat((base, G), 1)
    buf.backward(Gcat.to(dev))
    r = ac.reference(g, x, z, G, base=base, logits=True, dtype=torch.float64, scale=0.2)
    assert bits_equal(buf[:, :C], x) and close(buf[:, C:], r[0]) and close(xd.grad, r[2]) and close(zd.grad, r[3])
    # plain torch ops around the operator
    xd = x.to(dev).requires_grad_(True)
    y = aggregate.film_attn_residual(xd, z.to(dev), csr, logits=True)
    assert close(y, x.double() + r_out)
    y = aggregate.film_attn_mix(xd, z.to(dev), csr, base.to(dev), 0.25, logits=True)
    assert close(y, 0.75 * r_out + 0.25 * base.double())


SETTINGS = settings(max_examples=int(os.environ.get("MRP_PROPERTY_EXAMPLES", "25")), deadline=None,
                    derandomize=not os.environ.get("MRP_PROPERTY_HUNT"), database=None,
                    suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large,
                                           HealthCheck.function_scoped_fixture])


def _edges_per_graph(bnn, dst):
    goff = np.concatenate([[0], np.cumsum(bnn)])
    dst = np.asarray(dst, np.int64)
    return [int(((dst >= goff[i]) & (dst < goff[i + 1])).sum()) for i in range(len(bnn))]


@SETTINGS
@given(batches(max_deg=16), st.integers(1, 20), st.sampled_from([(1, 1), (3, 5), (7, 7), (8, 8), (5, 16)]),
       st.integers(0, 2 ** 31 - 1), st.booleans())
def test_arbitrary_graphs(cuda_device, case, C, hw, seed, logits):
    """Batches of <= 16-node graphs with in-degree <= 16: multi-edges, self-loops, zero in-degree, empty graphs."""
    bnn, src, dst = case
    g = m.RobotGraph(src, dst, num_nodes=int(sum(bnn)), batch_num_nodes=bnn,
                     batch_num_edges=_edges_per_graph(bnn, dst))
    if g.num_nodes() == 0:
        return
    x, gb, z, G, base = ac.random_operands(g, C, hw[0], hw[1], seed % 1000)
    w = z if logits else gb
    ref = ac.reference(g, x, w, G, base=base, logits=logits, dtype=torch.float64)
    got = run(cuda_device, g, x, w, G, base=base, logits=logits)
    for a, b in zip(got, ref):
        assert rel_err(a.numpy(), b.numpy()) <= TOL


# ------------------------------------------------------------------------------------------------ the model
def _frames(B, n, seed):
    # robots within a metre or so of each other: the encoder's logits stay O(1)
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.uniform(-1, 1, (B, n, 3)), rng.standard_normal((B, n, 4))], 2).astype(np.float32)


def _opt(C, layers, combine, scale=None):
    opt = types.SimpleNamespace(feature_dim=C, gcn_mode="film_attn", gcn_layers=layers, gcn_combine=combine,
                                gcn2_alpha=0.25)
    if scale is not None:
        opt.gcn_attn_scale = scale
    return opt


def _stack(C, layers, combine, scale=None):
    torch.manual_seed(0)
    return m.GCNStack(_opt(C, layers, combine, scale))


def _inputs(g, C, H, W, T, seed=1):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g.num_nodes(), C, H, W, generator=gen).to(T).float()
    return x, torch.randn(x.shape, generator=gen)


def _check_model(dev, net, call, g, pose, x, G, layers, combine, scale=None):
    params = {k: v.detach() for k, v in net.named_parameters()}
    xd = x.to(dev).requires_grad_(True)
    before = aggregate.PATH_COUNTS["attn_fwd_f32"], aggregate.PATH_COUNTS["attn_bwd_f32"]
    out = call(xd)
    out.backward(G.to(dev))
    assert aggregate.PATH_COUNTS["attn_fwd_f32"] == before[0] + layers
    assert aggregate.PATH_COUNTS["attn_bwd_f32"] == before[1] + layers
    r_out, r_dx, r_p = ac.stack_reference(params, g, x, pose, G, layers, combine, 0.25, scale=scale)
    assert close(out, r_out)
    assert close(xd.grad, r_dx)
    for k, p in net.named_parameters():
        assert close(p.grad, r_p[k]), k
    return out.detach()


# scale None: 1/sqrt(C) = 0.354 at C = 8; 0.5: another value set through opt.gcn_attn_scale (it must reach the
# forward and the backward of every composition, FilmCompressFunction's ctx.scale included)
@pytest.mark.parametrize("scale", [None, 0.5])
@pytest.mark.parametrize("combine", ["cat_compress", "residual", "initial_mix"])
def test_model_stack_fp32(cuda_device, combine, scale):
    C, H, W, layers = 8, 4, 4, 2
    g = m.batch([m.frame_graph(p) for p in _frames(2, 8, seed=3)])
    net = _stack(C, layers, combine, scale).to(cuda_device)
    x, G = _inputs(g, C, H, W, torch.float32)
    gd = g.to(cuda_device)
    _check_model(cuda_device, net, lambda t: net(gd, t), gd, g.edata["pose"], x, G, layers, combine, scale)
    if scale is not None:
        # the scale matters: the default's output is elsewhere
        r_def = ac.stack_reference({k: v.detach() for k, v in net.named_parameters()}, gd, x, g.edata["pose"], G,
                                   layers, combine, 0.25)[0]
        r_set = ac.stack_reference({k: v.detach() for k, v in net.named_parameters()}, gd, x, g.edata["pose"], G,
                                   layers, combine, 0.25, scale=scale)[0]
        assert rel_err(r_def.numpy(), r_set.numpy()) > 100 * TOL


U_BF16 = 2.0 ** -8  # bf16's spacing relative to a value in [1, 2): one rounding moves a value by at most half of it


def _layer(net, gd, i, h, h0):
    """Layer i of the stack, as models._run_stack composes it."""
    gcn = getattr(net, f"gcn{i}")
    if net.gcn_combine == "cat_compress":
        return gcn.forward_cat_compress(gd, h, getattr(net, f"conv{i}"))
    if net.gcn_combine == "residual":
        return gcn.forward_residual(gd, h)
    return gcn.forward_mix(gd, h, h0, 0.25)


def _run_layer(net, gd, i, h, h0, G):
    """out, dh and the layer's parameter gradients for input h (a fresh leaf) and output gradient G."""
    net.zero_grad(set_to_none=True)
    leaf = h.detach().clone().requires_grad_(True)
    out = _layer(net, gd, i, leaf, h0)
    out.backward(G.to(out.dtype))
    grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    return out.detach(), leaf.grad, grads


@pytest.mark.parametrize("scale", [None, 0.5])
@pytest.mark.parametrize("combine", ["cat_compress", "residual", "initial_mix"])
def test_model_stack_bf16(cuda_device, combine, scale):
    """A two-layer stack on bf16 features, held to the fp32 run on the same bf16-valued input, layer by layer.

    Every store rounds to bf16, so the float64 bar of the fp32 test cannot apply to values held in bf16; the
    yardstick is the same module's fp32 evaluation, as tests/test_gpu_film_max.py does, with bounds counted from
    the roundings (max-abs relative, rel_err).  A whole-stack comparison has no usable bound here: layer 2
    scores layer 1's rounded outputs, and the softmax passes a perturbation of its scores on with a factor that
    only a worst-case estimate limits (1 + 4 scale C (M + X) M for features up to X and messages up to M: in the
    hundreds).  So the chain is cut where the rounding happens: the bf16 stack is run whole; its layer-1 output
    h1 (bf16) and the gradient dh1 (bf16) that its layer 2 returns are taken from that run; and each layer of the
    bf16 run is compared with the fp32 evaluation of *that layer* on the widened bf16 tensors it actually
    received.  The inputs of the two evaluations of a layer are then identical, so by the 16-bit contract the
    scores and weights are equal bit for bit and nothing is amplified, and both layers, forward and backward,
    are held:

    forward, per layer: three roundings on the value path (the aggregate's store, the compress weight or the mix
    product, the layer output), each at most u/2 of its value: 3 u / 2;
    backward, per layer: from the layer's output gradient to any of its gradients at most four roundings to bf16
    (the scaled output gradient of the mix or the compress data gradient's gx / ga store, the saved aggregate
    that enters the weight gradient, grad_x's store, the final sum of x's two gradient terms), each at most u/2
    of its value; the attention backward is linear in the rounded ga.  4 u allows the sums over a row's <= 7
    entries, the channels and the pixels twice that: 4 u of the tensor's largest element.

    That the layers compose as the stack does is asserted bit for bit (the chained bf16 layers reproduce the
    whole-stack run's output, dx and parameter gradients)."""
    C, H, W, layers = 8, 4, 4, 2
    dev = cuda_device
    bf = torch.bfloat16
    g = m.batch([m.frame_graph(p) for p in _frames(2, 8, seed=3)])
    gd = g.to(dev)
    net = _stack(C, layers, combine, scale).to(dev)
    x, G = _inputs(g, C, H, W, bf)
    G = G.to(bf).float().to(dev)  # a bf16-valued output gradient
    xb = x.to(dev).to(bf)
    # the bf16 stack, whole
    before = aggregate.PATH_COUNTS["attn_fwd_bf16"], aggregate.PATH_COUNTS["attn_bwd_bf16"]
    net.zero_grad(set_to_none=True)
    leaf = xb.clone().requires_grad_(True)
    out = net(gd, leaf)
    out.backward(G.to(bf))
    whole = out.detach(), leaf.grad, {k: p.grad.clone() for k, p in net.named_parameters()}
    assert whole[0].dtype == bf and whole[1].dtype == bf
    assert aggregate.PATH_COUNTS["attn_fwd_bf16"] == before[0] + layers
    assert aggregate.PATH_COUNTS["attn_bwd_bf16"] == before[1] + layers
    # the same stack as a chain of its bf16 layers: h1, then layer 2 and its dh1, then layer 1's backward
    with torch.no_grad():
        h1 = _layer(net, gd, 1, xb, xb)
    assert h1.dtype == bf
    got2 = _run_layer(net, gd, 2, h1, xb, G)
    dh1 = got2[1]
    got1 = _run_layer(net, gd, 1, xb, xb, dh1.float())
    assert bits_equal(got2[0], whole[0])
    for k, v in {**got1[2], **got2[2]}.items():
        assert bits_equal(v, whole[2][k]), k
    if combine != "initial_mix":
        assert bits_equal(got1[1], whole[1])
    else:
        # x is also h0: besides layer 1's own dx it receives alpha dh1 and alpha G directly (alpha = 1/4: exact
        # products), summed by autograd in bf16: two additions, each rounding once by at most 2^-8 of its result
        want = got1[1].float() + 0.25 * dh1.float() + 0.25 * G
        assert rel_err(whole[1].float().cpu().numpy(), want.cpu().numpy()) <= 2 * U_BF16
    # each layer against its fp32 evaluation on the widened tensors the bf16 layer received
    ref2 = _run_layer(net, gd, 2, h1.float(), xb.float(), G)
    ref1 = _run_layer(net, gd, 1, xb.float(), xb.float(), dh1.float())
    for i, got, ref in ((1, (h1,) + got1[1:], ref1), (2, got2, ref2)):
        e = rel_err(got[0].float().cpu().numpy(), ref[0].cpu().numpy())
        print(combine, scale, "layer", i, "forward", e, "bar", 3 * U_BF16 / 2)
        assert e <= 3 * U_BF16 / 2
        e = rel_err(got[1].float().cpu().numpy(), ref[1].cpu().numpy())
        print(combine, scale, "layer", i, "dh", e, "bar", 4 * U_BF16)
        assert e <= 4 * U_BF16
        assert set(got[2]) == set(ref[2]) and got[2]
        for k in ref[2]:
            e = rel_err(got[2][k].float().cpu().numpy(), ref[2][k].cpu().numpy())
            print(combine, scale, "layer", i, k, e, "bar", 4 * U_BF16)
            assert e <= 4 * U_BF16, k


def test_model_step_on_a_device_built_range_graph(cuda_device):
    C, H, W, layers = 8, 4, 4, 1
    B, n = 2, 9
    poses = torch.from_numpy(_frames(B, n, seed=5)).to(cuda_device)
    active = torch.ones(B, n, dtype=torch.bool, device=cuda_device)
    active[0, 3] = False
    g = m.frame_batch(poses, max_range=1.2, active=active)
    csr = g.csr(cuda_device)
    assert csr.graph_kind == _lib.GRAPH_SIMPLE and csr.max_in_degree == n - 1
    torch.manual_seed(0)
    net = m.multi_view_dgl_model(types.SimpleNamespace(feature_dim=C, gcn_mode="film_attn", compress_gcn=True,
                                                       multi_gcn=False)).to(cuda_device)
    pose = g.edata["pose"].cpu()
    x, G = _inputs(g, C, H, W, torch.float32)

    def call(t):
        g.ndata["image"] = t
        return net(g)
    _check_model(cuda_device, net, call, g, pose, x, G, layers, "cat_compress")
