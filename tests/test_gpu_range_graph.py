"""GPU: range-limited / drop-out robot graphs.

* the device builder (``frame_batch(poses, knn, max_range, active)`` -> ``mrp_frame_graph_build_range``)
  against the host builder, a capture of it included;
* the aggregation on ``GRAPH_SIMPLE`` graphs of 9..16 nodes — the matrix-core backward in its CSR-row form —
  against the float64 oracle on the active edge list, with the suite's bars (``TOL`` for fp32, ``half_cases``'
  for 16-bit features), bit-stable, and with the 16-bit kernels' contract against the fp32 run;
* the same arrays handed over as ``GRAPH_CSR`` and as ``GRAPH_SIMPLE``;
* a 2-layer ``GCNStack`` on a device-built range graph against a float64 restatement with a per-edge mask.
"""
import functools
import math

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib, aggregate
import geometry_cases as gc
import half_cases as hc
import oracle
import stack_ref
from conftest import rel_err
from test_gpu_properties import TOL
from test_range_graph_cpu import actives, lattice_poses

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


# ------------------------------------------------------------------------------------------------ builder
def batch_poses(B, n, nan=False):
    return np.stack([lattice_poses(n, seed=b, nan_robot=(2 if nan and b % 2 == 0 else None)) for b in range(B)]) \
        if B else np.zeros((0, n, 7), np.float32)


def batch_active(B, n, which):
    if which == "all":
        return None
    rows = [np.roll(actives(n)[which], b) for b in range(B)]
    return np.stack(rows) if rows else np.zeros((0, n), bool)


def check_builder(dev, poses, max_range, active, knn):
    B, n = poses.shape[:2]
    host = m.batch([m.frame_graph(poses[b], knn=knn, max_range=max_range, active=None if active is None else active[b])
                    for b in range(B)])
    indptr, src, eid, goff, _ = host.host_csr()
    pd = torch.from_numpy(poses).to(dev)
    g = m.frame_batch(pd, knn=knn, max_range=max_range, active=None if active is None else torch.from_numpy(active).to(dev))
    csr = g.csr(dev)
    E = B * n * (n - 1)
    assert csr.graph_kind == _lib.GRAPH_SIMPLE and csr.num_edges == E == g.num_edges() and csr.num_nodes == B * n
    assert (csr.num_graphs, csr.max_nodes) == (B, n)
    ea = int(indptr[-1])
    assert np.array_equal(csr.indptr.cpu().numpy(), indptr)
    assert np.array_equal(csr.src.cpu().numpy()[:ea], src)
    assert np.array_equal(csr.eid.cpu().numpy()[:ea], eid)
    assert np.array_equal(csr.graph_off.cpu().numpy(), goff)
    assert np.array_equal(csr.graph_off.cpu().numpy(), np.arange(B + 1) * n)
    full = m.frame_batch(pd)
    assert torch.equal(g.edata["pose"].view(torch.int32), full.edata["pose"].view(torch.int32))
    assert torch.equal(g.edge_active, host.edge_active)
    assert g.csr(dev, simple=False).graph_kind == _lib.GRAPH_CSR and not g.is_complete()
    return g


@pytest.mark.parametrize("act", ["all", "some", "none"])
@pytest.mark.parametrize("max_range", [0.0, 5.0, 9.0, math.inf])
@pytest.mark.parametrize("n", [1, 2, 5, 9, 16])
@pytest.mark.parametrize("B", [1, 3])
def test_builder_matches_the_host_builder(cuda_device, B, n, max_range, act):
    poses = batch_poses(B, n, nan=max_range in (5.0, math.inf))
    for knn in (None, 1, 4):
        if knn is None or knn < n:
            check_builder(cuda_device, poses, max_range, batch_active(B, n, act), knn)


@pytest.mark.parametrize("n,knn,act", [(16, None, "some"), (16, 4, "all"), (9, 1, "some"), (5, None, "all"),
                                        (2, None, "some"), (1, None, "all")])
def test_builder_on_a_batch_that_spans_several_scan_workgroups(cuda_device, n, knn, act):
    """300 frames: 4800 robots at n = 16, so the in-degrees' prefix sum crosses 19 workgroups' totals."""
    check_builder(cuda_device, batch_poses(300, n, nan=True), 7.0, batch_active(300, n, act), knn)


def test_builder_only_with_active(cuda_device):
    g = check_builder(cuda_device, batch_poses(3, 9), None, batch_active(3, 9, "some"), None)
    assert 0 < int(g.edge_active.sum()) < g.num_edges()


def test_builder_is_capturable_and_replays_on_new_poses(cuda_device):
    """The build alone on one stream in a captured graph: replayed on poses written into the captured input
    afterwards it gives the new frames' graph — nothing in it came from the host."""
    B, n = 3, 9
    first, second = batch_poses(B, n), batch_poses(B, n)[::-1].copy() + np.float32(1.0)
    second[..., 3:] = batch_poses(B, n)[..., 3:]
    active = torch.from_numpy(batch_active(B, n, "some")).to(cuda_device)
    buf = torch.from_numpy(first).to(cuda_device)
    m.frame_batch(buf, max_range=6.0, active=active, knn=4)  # library loaded, allocator warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = m.frame_batch(buf, max_range=6.0, active=active, knn=4)
    buf.copy_(torch.from_numpy(second))
    active.copy_(torch.from_numpy(batch_active(B, n, "some")[::-1].copy()))
    graph.replay()
    torch.cuda.synchronize()
    act = active.cpu().numpy()
    host = m.batch([m.frame_graph(second[b], knn=4, max_range=6.0, active=act[b]) for b in range(B)])
    indptr, src, eid, goff, _ = host.host_csr()
    csr = g.csr(cuda_device)
    ea = int(indptr[-1])
    assert np.array_equal(csr.indptr.cpu().numpy(), indptr)
    assert np.array_equal(csr.src.cpu().numpy()[:ea], src) and np.array_equal(csr.eid.cpu().numpy()[:ea], eid)
    assert torch.equal(g.edata["pose"].cpu().view(torch.int32), host.edata["pose"].view(torch.int32))


# ------------------------------------------------------------------------------------------------ aggregation
def one_graph(nn, rng):
    """Edge slots: every ordered pair plus the self-loop 1 -> 1.  Node 0 has in-degree 0, node 1 in-degree
    nn - 1 (every active robot and itself), robot 3 is inactive (no edge in or out), the rest is random."""
    src, dst = (list(t) for t in m.complete_edges(nn))
    src.append(1)
    dst.append(1)
    s, d = np.asarray(src), np.asarray(dst)
    mask = rng.rand(len(s)) < 0.5
    mask[d == 0] = False
    mask[d == 1] = True
    mask[(s == 3) | (d == 3)] = False
    return m.RobotGraph(s, d, num_nodes=nn, edge_active=torch.from_numpy(mask))


@functools.lru_cache(maxsize=None)
def simple_batch(n):
    rng = np.random.RandomState(900 + n)
    g = m.batch([one_graph(n, rng), one_graph(n, rng), one_graph(n - 2, rng)])
    deg = g.in_degrees().numpy()
    assert deg[0] == 0 and deg[1] == n - 1 and deg[3] == 0 and deg[2 * n + 1] == n - 3
    return g


@functools.lru_cache(maxsize=None)
def inputs(n, C, P, key):
    """(x, gb, z, G, G0) on the CPU: features drawn in fp32 and rounded to the dtype; gb == sigmoid(z)."""
    g = simple_batch(n)
    gen = torch.Generator().manual_seed(n * 1000 + C * 10 + P + len(key))
    shape = (g.num_nodes(), C, 8, P // 8)
    x, G, G0 = (torch.randn(shape, generator=gen).to(DT[key]) for _ in range(3))
    z = torch.randn(g.num_edges(), C, 2, generator=gen)
    return x, torch.sigmoid(z), z, G, G0


@functools.lru_cache(maxsize=None)
def reference(n, C, P, key, mode, prec="64"):
    """The oracle on the active edge list: out, dx and dgb scattered into all E rows (zeros elsewhere)."""
    g = simple_batch(n)
    x, gb, _, G, _ = inputs(n, C, P, key)
    dt = torch.float64 if prec == "64" else torch.float32
    mask = g.edge_active
    src, dst = (t[mask].numpy() for t in g.edges())
    out = oracle.film_aggregate(x.to(dt), gb[mask].to(dt), src, dst, mode)
    dx, dgb_a = oracle.film_aggregate_grads(x.to(dt), gb[mask].to(dt), src, dst, G.to(dt), mode)
    dgb = torch.zeros(g.num_edges(), C, 2, dtype=dt)
    dgb[mask] = dgb_a
    return out, dx, dgb


def sigmoid_chain(dgb, gb):
    """d logits = d gamma/beta * s (1 - s)."""
    return dgb * (gb.to(dgb.dtype) * (1 - gb.to(dgb.dtype)))


def run_backward(dev, n, C, P, key, mode="film_mean", logits=False, op="plain", kind="simple", dtype=None,
                 expect="film_bwd_mfma"):
    g = simple_batch(n)
    x, gb, z, G, G0 = (t.to(dev) for t in inputs(n, C, P, key))
    if dtype is not None:
        x, G, G0 = x.to(dtype), G.to(dtype), G0.to(dtype)
    csr = g.csr(dev, simple=kind == "simple")
    assert csr.graph_kind == (_lib.GRAPH_SIMPLE if kind == "simple" else _lib.GRAPH_CSR)
    plan = aggregate.launch_plan("bwd", csr, C, P, dtype=x.dtype, mode=mode, logits=logits, grad_x_base=op == "cat")
    assert plan.kernel_name == expect, plan.kernel_name
    k = {v: k for k, v in DT.items()}[x.dtype]
    assert gc.violations(plan, k, csr, C, P, 16) == []
    copy = mode == "copy_mean"
    flags = aggregate._mode_flags(mode, logits)
    ep = aggregate.EpilogueSpec(1.0, 1.0) if op == "residual" else None
    dx, dgb = aggregate.film_mean_backward(G, x, None if copy else (z if logits else gb), csr, flags, True, not copy,
                                           grad_x_base=G0 if op == "cat" else None, epilogue=ep)
    return dx, dgb


def check_against_float64(dev, n, C, P, key, mode, logits, op):
    g = simple_batch(n)
    T = DT[key]
    dx, dgb = run_backward(dev, n, C, P, key, mode, logits, op)
    dx2, dgb2 = run_backward(dev, n, C, P, key, mode, logits, op)
    assert torch.equal(hc.bits(dx), hc.bits(dx2))  # deterministic
    x, gb, _, G, G0 = inputs(n, C, P, key)
    _, dx64, dgb64 = reference(n, C, P, key, mode)
    dx64 = dx64 + (G0.double() if op == "cat" else G.double() if op == "residual" else 0.0)
    if logits:
        dgb64 = sigmoid_chain(dgb64, gb)
    if key == "f32":
        e = rel_err(dx.cpu().numpy(), dx64.numpy())
        print("dx rel_err", e)
        assert e <= TOL
    else:
        assert dx.dtype == T
        hc.assert_elementwise(dx, dx64, T, "dx")
    if mode == "copy_mean":
        return
    assert torch.equal(hc.bits(dgb), hc.bits(dgb2))
    absent = ~g.edge_active
    assert int(absent.sum()) > 0 and torch.count_nonzero(dgb.cpu()[absent]) == 0  # exactly zero (+0.0 bits below)
    assert torch.count_nonzero(hc.bits(dgb)[absent]) == 0
    if key == "f32":
        e = rel_err(dgb.cpu().numpy(), dgb64.numpy())
        print("dgb rel_err", e)
        assert e <= TOL
    else:
        _, _, dgb32 = reference(n, C, P, key, mode, "32")
        if logits:
            dgb32 = sigmoid_chain(dgb32, gb)
        hc.assert_relative(dgb, dgb32, dgb64, "dgb")


@pytest.mark.parametrize("mode", ["film_mean", "film_sum", "copy_mean"])
@pytest.mark.parametrize("key", list(DT))
@pytest.mark.parametrize("P", [64, 128])
@pytest.mark.parametrize("C", [1, 7, 9])
@pytest.mark.parametrize("n", [9, 12, 16])
def test_backward_against_float64(cuda_device, n, C, P, key, mode):
    check_against_float64(cuda_device, n, C, P, key, mode, logits=False, op="plain")


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("op", ["plain", "cat", "residual"])
@pytest.mark.parametrize("mode", ["film_mean", "film_sum"])
@pytest.mark.parametrize("key", list(DT))
@pytest.mark.parametrize("n", [9, 12, 16])
def test_backward_epilogues_and_logits_against_float64(cuda_device, n, key, mode, op, logits):
    if op == "plain" and not logits:
        return  # the test above
    check_against_float64(cuda_device, n, 9, 128, key, mode, logits, op)


@pytest.mark.parametrize("cpw", [1, 2])
@pytest.mark.parametrize("key", list(DT))
@pytest.mark.parametrize("n", [9, 12, 16])
def test_backward_with_more_channels_than_two_workgroups(cuda_device, n, key, cpw):
    with gc.knobs(bwd_mfma_cpw=cpw):
        check_against_float64(cuda_device, n, 17, 64, key, "film_mean", logits=True, op="cat")


@pytest.mark.parametrize("mode", ["film_mean", "film_sum", "copy_mean"])
@pytest.mark.parametrize("key", list(DT))
@pytest.mark.parametrize("n", [9, 16])
def test_forward_against_float64(cuda_device, n, key, mode):
    C, P = 9, 128
    g = simple_batch(n)
    x, gb, z, _, _ = (t.to(cuda_device) for t in inputs(n, C, P, key))
    out64, _, _ = reference(n, C, P, key, mode)
    for logits in (False, True):
        out = torch.empty_like(x)
        aggregate.film_mean_forward_into(x, None if mode == "copy_mean" else (z if logits else gb), g.csr(cuda_device),
                                         aggregate._mode_flags(mode, logits), out)
        if key == "f32":
            assert rel_err(out.cpu().numpy(), out64.numpy()) <= TOL
        else:
            hc.assert_elementwise(out, out64, DT[key], "out")
    assert torch.count_nonzero(out[0]) == 0  # in-degree 0: zeros


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("op", ["plain", "cat", "residual"])
@pytest.mark.parametrize("key", ["bf16", "f16"])
@pytest.mark.parametrize("n", [9, 16])
def test_16_bit_contract_against_the_fp32_run(cuda_device, n, key, op, logits):
    """grad_gb bit-equal to the fp32 kernel's on the widened inputs, grad_x that kernel's rounded once."""
    dx, dgb = run_backward(cuda_device, n, 9, 128, key, "film_mean", logits, op)
    dx32, dgb32 = run_backward(cuda_device, n, 9, 128, key, "film_mean", logits, op, dtype=torch.float32)
    assert dx32.dtype == torch.float32 and dx.dtype == DT[key]
    assert torch.equal(hc.bits(dgb), hc.bits(dgb32))
    assert torch.equal(hc.bits(dx), hc.bits(dx32.to(DT[key])))


# ------------------------------------------------------------------------------------------------ CSR vs SIMPLE
@functools.lru_cache(maxsize=None)
def small_batch():
    rng = np.random.RandomState(5)
    return m.batch([one_graph(8, rng), one_graph(6, rng)])


def both_kinds(dev, g, C, H, W, key, channels_last=False, seed=3):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda: torch.randn(g.num_nodes(), C, H, W, generator=gen).to(DT[key]).to(dev)  # noqa: E731
    x, G = mk(), mk()
    if channels_last:
        x, G = (t.contiguous(memory_format=torch.channels_last) for t in (x, G))
    gb = torch.rand(g.num_edges(), C, 2, generator=gen).to(dev)
    res = []
    for simple in (True, False):
        csr = g.csr(dev, simple=simple)
        out = aggregate._empty_like_layout(x)
        aggregate.film_mean_forward_into(x, gb, csr, _lib.MODE_FILM_MEAN, out)
        dx, dgb = aggregate.film_mean_backward(G, x, gb, csr, _lib.MODE_FILM_MEAN, True, True)
        res.append((out, dx, dgb))
    return res


def same_plans(dev, g, C, P, key, direction):
    a, b = (aggregate.launch_plan(direction, g.csr(dev, simple=s), C, P, dtype=DT[key]) for s in (True, False))
    return gc.plan_tuple(a) == gc.plan_tuple(b), a.kernel_name, b.kernel_name


@pytest.mark.parametrize("key", list(DT))
def test_csr_and_simple_are_bit_equal_where_they_plan_the_same_kernel(cuda_device, key):
    dev = cuda_device
    # graphs of <= 8 nodes; 12-node graphs on 4x4 planes (P = 16): the same kernels, forward and backward
    for g, C, H, W in ((small_batch(), 9, 8, 8), (simple_batch(12), 7, 4, 4)):
        for direction in ("fwd", "bwd"):
            same, ka, kb = same_plans(dev, g, C, H * W, key, direction)
            assert same, (direction, ka, kb)
        (o1, dx1, dgb1), (o2, dx2, dgb2) = both_kinds(dev, g, C, H, W, key)
        assert torch.equal(hc.bits(o1), hc.bits(o2)) and torch.equal(hc.bits(dx1), hc.bits(dx2))
        assert torch.equal(hc.bits(dgb1), hc.bits(dgb2))
        assert torch.count_nonzero(hc.bits(dgb1)[~g.edge_active]) == 0
    # the forward at a shape whose backward differs
    g = simple_batch(12)
    assert same_plans(dev, g, 9, 64, key, "fwd")[0]
    (o1, dx1, dgb1), (o2, dx2, dgb2) = both_kinds(dev, g, 9, 8, 8, key)
    assert torch.equal(hc.bits(o1), hc.bits(o2))
    # channels_last: one pair of kernels for both kinds
    before = aggregate.PATH_COUNTS["bwd_cl_" + key]
    (o1, dx1, dgb1), (o2, dx2, dgb2) = both_kinds(dev, g, 16, 8, 8, key, channels_last=True)
    assert aggregate.PATH_COUNTS["bwd_cl_" + key] == before + 2
    assert torch.equal(hc.bits(o1), hc.bits(o2)) and torch.equal(hc.bits(dx1), hc.bits(dx2))
    assert torch.equal(hc.bits(dgb1), hc.bits(dgb2))
    assert torch.count_nonzero(hc.bits(dgb1)[~g.edge_active]) == 0


@pytest.mark.parametrize("key", list(DT))
@pytest.mark.parametrize("n", [9, 12, 16])
def test_csr_route_and_simple_route_agree_under_the_bars(cuda_device, n, key):
    """Where only the routes differ (film_bwd_dx + Gram pass against film_bwd_mfma): both under the bars
    against float64, the CSR route's unnamed gradient rows cleared by the Python layer."""
    C, P = 9, 64
    g = simple_batch(n)
    dx_c, dgb_c = run_backward(cuda_device, n, C, P, key, kind="csr", expect="film_bwd_dx_gram")
    dx_s, dgb_s = run_backward(cuda_device, n, C, P, key)
    _, dx64, dgb64 = reference(n, C, P, key, "film_mean")
    _, _, dgb32 = reference(n, C, P, key, "film_mean", "32")
    for dx, dgb in ((dx_c, dgb_c), (dx_s, dgb_s)):
        assert torch.count_nonzero(hc.bits(dgb)[~g.edge_active]) == 0
        if key == "f32":
            assert rel_err(dx.cpu().numpy(), dx64.numpy()) <= TOL and rel_err(dgb.cpu().numpy(), dgb64.numpy()) <= TOL
        else:
            hc.assert_elementwise(dx, dx64, DT[key], "dx")
            hc.assert_relative(dgb, dgb32, dgb64, "dgb")


# ------------------------------------------------------------------------------------------------ model
def masked_stack(params, x, pose, src, dst, mask, layers):
    """stack_ref.stack_forward('cat_compress') with a dense per-edge mask: absent edges send nothing and do
    not count in the mean."""
    h = x
    w = mask.to(x.dtype)
    deg = torch.zeros(x.shape[0], dtype=x.dtype, device=x.device).index_add_(0, dst, w).clamp_min(1)
    for i in range(1, layers + 1):
        gb = stack_ref.edge_gb(params, f"gcn{i}.edge_encoder.", pose)
        msg = (gb[:, :, 0, None, None] * h.index_select(0, src) + gb[:, :, 1, None, None]) * w[:, None, None, None]
        a = torch.zeros_like(h).index_add_(0, dst, msg) / deg[:, None, None, None]
        h = stack_ref.conv1x1(torch.cat((h, a), 1), params[f"conv{i}.weight"], params[f"conv{i}.bias"])
    return h


def run_masked(params, x, pose, src, dst, mask, G, dtype):
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    xx = x.detach().to(dtype).requires_grad_(True)
    out = masked_stack(p, xx, pose, src, dst, mask, 2)
    out.backward(G.to(dtype))
    return out.detach(), xx.grad, {k: v.grad for k, v in p.items()}


def test_two_layer_stack_on_a_device_built_range_graph(cuda_device):
    import test_gpu_configs as cfg
    dev = cuda_device
    B, n, C, H = 2, 12, 32, 8
    rng = np.random.RandomState(12)
    poses = np.concatenate([rng.uniform(-6, 6, (B, n, 3)), rng.standard_normal((B, n, 4))], -1).astype(np.float32)
    active = np.ones((B, n), bool)
    active[0, 5] = active[1, 0] = False
    build = lambda p: m.frame_batch(p, max_range=7.0, active=torch.from_numpy(active).to(dev))  # noqa: E731
    g = build(torch.from_numpy(poses).to(dev))
    mask = g.edge_active
    assert 0 < int(mask.sum()) < g.num_edges()
    net = cfg.model(C, 2).to(dev)
    torch.manual_seed(3)
    x0 = torch.randn(B * n, C, H, H, device=dev)
    G = torch.randn(B * n, C, H, H, device=dev)

    def step(graph):
        net.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        out = net(graph, x)
        out.backward(G)
        return out.detach(), x.grad, {k: p.grad.clone() for k, p in net.named_parameters()}

    csr = g.csr(dev)
    assert aggregate.launch_plan("bwd", csr, C, H * H, grad_x_base=True, logits=True).kernel_name == "film_bwd_mfma"
    out, dx, grads = step(g)
    params = {k: v.detach() for k, v in net.named_parameters()}
    src, dst = (t.to(dev) for t in g.edges())
    args = (params, x0, g.edata["pose"], src, dst, mask.to(dev), G)
    f64, f32 = run_masked(*args, torch.float64), run_masked(*args, torch.float32)
    for name, ours, a32, a64 in [("out", out, f32[0], f64[0]), ("dx", dx, f32[1], f64[1])] + \
                                [(k, grads[k], f32[2][k], f64[2][k]) for k in grads]:
        ok, e = stack_ref.within(ours, a32, a64)
        print(name, e)
        assert ok, (name, e)
    # an absent edge's pose row reaches nothing
    g2 = build(torch.from_numpy(poses).to(dev))
    absent = int(torch.nonzero(~mask)[0])
    g2.edata["pose"][absent] += 1.0
    out2, dx2, grads2 = step(g2)
    assert torch.equal(hc.bits(out), hc.bits(out2)) and torch.equal(hc.bits(dx), hc.bits(dx2))
    for k in grads:
        assert torch.equal(hc.bits(grads[k]), hc.bits(grads2[k])), k


def test_gcn_and_multi_view_model_run_on_range_graphs(cuda_device):
    """The drop-in modules need no change: ``GCN`` (forward and gradients against float64 with the per-edge
    mask) and ``multi_view_dgl_model`` (the same stack as ``GCNStack``: the same bits)."""
    import types
    import test_gpu_configs as cfg
    dev = cuda_device
    B, n, C, H = 2, 12, 32, 8
    rng = np.random.RandomState(21)
    poses = np.concatenate([rng.uniform(-6, 6, (B, n, 3)), rng.standard_normal((B, n, 4))], -1).astype(np.float32)
    g = m.frame_batch(torch.from_numpy(poses).to(dev), max_range=8.0, knn=5)
    mask = g.edge_active.to(dev)
    assert 0 < int(mask.sum()) < g.num_edges() and int(g.in_degrees().max()) <= 5
    torch.manual_seed(4)
    x0 = torch.randn(B * n, C, H, H, device=dev)
    G = torch.randn(B * n, C, H, H, device=dev)
    gcn = m.GCN(types.SimpleNamespace(feature_dim=C)).to(dev)
    x = x0.clone().requires_grad_(True)
    out = gcn(g, x)
    out.backward(G)
    src, dst = (t.to(dev) for t in g.edges())
    params = {k: v.detach() for k, v in gcn.edge_encoder.named_parameters()}

    def layer(dtype):
        p = {k: v.to(dtype).requires_grad_(True) for k, v in params.items()}
        xx = x0.to(dtype).requires_grad_(True)
        gb = stack_ref.edge_gb(p, "", g.edata["pose"])
        w = mask.to(dtype)
        msg = (gb[:, :, 0, None, None] * xx.index_select(0, src) + gb[:, :, 1, None, None]) * w[:, None, None, None]
        deg = torch.zeros(B * n, dtype=dtype, device=dev).index_add_(0, dst, w).clamp_min(1)
        a = torch.zeros_like(xx).index_add_(0, dst, msg) / deg[:, None, None, None]
        a.backward(G.to(dtype))
        return a.detach(), xx.grad, {k: v.grad for k, v in p.items()}

    f64, f32 = layer(torch.float64), layer(torch.float32)
    for name, ours, a32, a64 in [("out", out, f32[0], f64[0]), ("dx", x.grad, f32[1], f64[1])] + \
                                [(k, p.grad, f32[2][k], f64[2][k]) for k, p in gcn.edge_encoder.named_parameters()]:
        ok, e = stack_ref.within(ours, a32, a64)
        assert ok, (name, e)
    stack = cfg.model(C, 2).to(dev)
    opt = types.SimpleNamespace(feature_dim=C, compress_gcn=True, multi_gcn=False, gcn_layers=2,
                                gcn_combine="cat_compress", gcn2_alpha=0.25)
    mv = m.multi_view_dgl_model(opt).to(dev)
    mv.load_state_dict(stack.state_dict())
    g.ndata["image"] = x0
    with torch.no_grad():
        assert torch.equal(hc.bits(mv(g)), hc.bits(stack(g, x0)))
    assert g.edge_active is not None and g.csr(dev).graph_kind == _lib.GRAPH_SIMPLE  # local_scope kept the mask
