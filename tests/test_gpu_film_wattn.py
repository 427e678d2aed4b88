"""The confidence-gated attention fusion on the GPU against the float64 restatement of its definition
(tests/wattn_cases.py), at the suite's bar; its three bit-for-bit consequences (unit weights are film_attn, a node
mask is film_attn on the compacted graph, the 16-bit contract); exact zeros, strided operands, determinism, the
containment of a silent sender's non-finite features; autograd and the GCN mode."""
import types

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib, aggregate
import attn_cases as ac
import wattn_cases as wc
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5  # the suite's bar (tests/test_gpu_film_attn.py); tests/test_film_wattn_cpu.py shows its teeth
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
NAMES = ("out", "attn", "rate", "dx", "dgb", "dw")


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(INT_VIEW[a.dtype]), b.view(INT_VIEW[b.dtype]))


def close(got, ref):
    return rel_err(got.detach().float().cpu().numpy(), ref.numpy()) <= TOL


def _cpu(t):
    return None if t is None else t.cpu()


def run(dev, g, x, gb, w, G=None, base=None, logits=False, need=(True, True, True), scale=None):
    """out, attn, rate, dx, dgb, dw of the kernels (the entry points without autograd) for host operands."""
    csr = g.csr(dev)
    flags = _lib.GB_LOGITS if logits else 0
    xd, gbd, wd = x.to(dev), gb.to(dev), w.to(dev)
    out = torch.empty_like(xd)
    attn, rate = m.film_wattn_forward_into(xd, gbd, wd, csr, flags, out, scale, rate=True)
    if G is None:
        return out.cpu(), attn.cpu(), rate.cpu(), None, None, None
    dx, dgb, dw = m.film_wattn_backward(G.to(dev), xd, gbd, wd, attn, rate, csr, flags, *need,
                                        grad_x_base=base.to(dev) if base is not None else None, scale=scale)
    return out.cpu(), attn.cpu(), rate.cpu(), _cpu(dx), _cpu(dgb), _cpu(dw)


def run_attn(dev, g, x, gb, G, base=None, logits=False):
    """out, attn, dx, dgb of film_attn's entry points."""
    csr = g.csr(dev)
    flags = _lib.GB_LOGITS if logits else 0
    xd, gbd = x.to(dev), gb.to(dev)
    out = torch.empty_like(xd)
    attn = m.film_attn_forward_into(xd, gbd, csr, flags, out)
    dx, dgb = m.film_attn_backward(G.to(dev), xd, gbd, attn, csr, flags, True, True,
                                   grad_x_base=base.to(dev) if base is not None else None)
    return out.cpu(), attn.cpu(), dx.cpu(), dgb.cpu()


def _frames(B, n, seed):
    # robots within a metre or so of each other: the encoder's logits stay O(1)
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.uniform(-1, 1, (B, n, 3)), rng.standard_normal((B, n, 4))], 2).astype(np.float32)


def range_batch(dev):
    """A device-built range-limited / drop-out batch (2 frames of 9 robots) with an isolated robot."""
    poses = torch.from_numpy(_frames(2, 9, seed=5)).to(dev)
    active = torch.ones(2, 9, dtype=torch.bool, device=dev)
    active[0, 3] = False
    g = m.frame_batch(poses, max_range=1.2, active=active)
    assert int(g.in_degrees()[3]) == 0 and not bool(g.edge_active[np.asarray(g.edges()[0]) == 3].any())
    return g


GRAPHS = {
    **{f"complete{n}": (lambda dev, n=n: wc.complete(n)) for n in (2, 5, 8, 9, 16)},
    "knn16_4": lambda dev: wc.knn(16, 4),
    "range_batch": range_batch,
    "loud_csr": lambda dev: wc.loud_csr(),
}
KINDS = {"knn16_4": _lib.graph_regular(4), "range_batch": _lib.GRAPH_SIMPLE, "loud_csr": _lib.GRAPH_CSR}
# one tile; a ragged tile (49 of 64 pixels); a ragged channel chunk; channels over many chunks with a remainder;
# a plane spanning 16 pixel tiles (grad_gb through the workspace)
SHAPES = [(1, 8, 8), (3, 7, 7), (17, 8, 8), (130, 8, 8), (8, 32, 32)]
# each graph with three of the five shapes (the two left out rotate), not the full product
CASES = [(name, SHAPES[(2 * i + s) % 5]) for i, name in enumerate(GRAPHS) for s in range(3)]


@pytest.mark.parametrize("name,shape", CASES, ids=[f"{n}-{s[0]}x{s[1]}x{s[2]}" for n, s in CASES])
def test_against_float64(cuda_device, name, shape):
    g = GRAPHS[name](cuda_device)
    C, H, W = shape
    assert g.csr(cuda_device).graph_kind == KINDS.get(name, _lib.GRAPH_COMPLETE)
    x, gb, z, G, base, w, louds = wc.random_operands(g, C, H, W, seed=len(name) + C)
    assert bool(louds) == (name == "loud_csr")
    if name == "loud_csr":
        assert g.csr(cuda_device).max_in_degree == 16
    for logits, p in ((False, gb), (True, z)):
        ref = list(wc.reference(g, x, p, w, G, logits=logits, loud=louds))
        got = list(run(cuda_device, g, x, p, w, G, logits=logits))
        for t in (ref, got):
            t[2], t[5] = wc.drop_loud(g, t[2], t[5], louds)  # a loud node's own rate and dw: IEEE's, not compared
        if g.csr(cuda_device).max_in_degree <= 1:
            # one entry per row: a = 1 where it delivers and da - dbar = 0 exactly, so grad_w is identically 0;
            # the reference holds its own rounding noise there, which no ratio can be taken against
            assert float(ref[5].abs().max()) <= 1e-12 and bool((got[5] == 0).all())
            ref[5] = torch.zeros_like(ref[5])
        errs = [rel_err(a.numpy(), b.numpy()) for a, b in zip(got, ref)]
        print(name, shape, "logits" if logits else "plain", dict(zip(NAMES, errs)))
        assert max(errs) <= TOL and all(np.isfinite(errs))
        again = run(cuda_device, g, x, p, w, G, base=base, logits=logits)
        assert close(again[3], ref[3] + base.double())
        assert bits_equal(again[4], got[4])


@pytest.mark.parametrize("name", ["complete5", "complete9", "complete16", "knn16_4", "loud_csr"])
@pytest.mark.parametrize("shape", [(3, 7, 7), (17, 8, 8), (8, 32, 32)])
def test_unit_weights_are_film_attn_bit_for_bit(cuda_device, name, shape):
    g = GRAPHS[name](cuda_device)
    x, _, z, G, base, _, _ = wc.random_operands(g, *shape, seed=2, loud=False)
    ones = torch.ones(g.num_nodes(), shape[1], shape[2])
    out, attn, rate, dx, dgb, dw = run(cuda_device, g, x, z, ones, G, base=base, logits=True)
    r_out, r_attn, r_dx, r_dgb = run_attn(cuda_device, g, x, z, G, base=base, logits=True)
    assert bits_equal(out, r_out) and bits_equal(attn, r_attn) and bits_equal(rate, attn)
    assert bits_equal(dx, r_dx) and bits_equal(dgb, r_dgb)
    assert bool(torch.isfinite(dw).all())


@pytest.mark.parametrize("shape", [(3, 7, 7), (17, 8, 8), (8, 32, 32)])
def test_node_mask_is_film_attn_on_the_compacted_graph(cuda_device, shape):
    """A 0/1 map constant over each node's plane against film_attn on ``frame_batch(active=mask)``: the same E and
    edge ids, the rows compacted.  That graph also drops the silent robots' in-edges, so their own rows are left
    out of the forward comparison and they are given no output gradient; everything else is compared whole."""
    dev = cuda_device
    B, n = 2, 9
    poses = torch.from_numpy(_frames(B, n, seed=9)).to(dev)
    mask = torch.ones(B, n, dtype=torch.bool)
    mask[0, 3] = mask[1, 0] = mask[1, 7] = False
    full = m.frame_batch(poses)
    part = m.frame_batch(poses, active=mask.to(dev))
    assert full.csr(dev).graph_kind == _lib.GRAPH_COMPLETE and part.num_edges() == full.num_edges()
    C, H, W = shape
    x, gb, _, G, base, _, _ = wc.random_operands(full, C, H, W, seed=6, loud=False)
    on = mask.reshape(-1)
    G[~on] = 0.0  # +0: the silent rows then add +0 everywhere, as rows that are not there do
    w = on.float()[:, None, None].expand(B * n, H, W).contiguous()
    out, attn, _, dx, dgb, _ = run(dev, full, x, gb, w, G, base=base)
    r_out, r_attn, r_dx, r_dgb = run_attn(dev, part, x, gb, G, base=base)
    src, dst = (np.asarray(t) for t in full.edges())
    heard = torch.as_tensor(on.numpy()[dst])
    removed = torch.as_tensor(~on.numpy()[src])
    assert bits_equal(out[on], r_out[on]) and bits_equal(attn[heard], r_attn[heard])
    assert bits_equal(dx, r_dx) and bits_equal(dgb, r_dgb)
    assert bool((attn[removed] == 0).all()) and bool((dgb[removed] == 0).all())
    assert bool((r_attn[removed] == 0).all()) and bool((r_dgb[removed] == 0).all())
    assert bool((out[on] != 0).any())


@pytest.mark.parametrize("name", ["complete9", "knn16_4"])
def test_node_mask_on_a_host_compacted_graph(cuda_device, name):
    """The same consequence with only the silent robots' out-edges removed (a host-built masked graph): every row,
    every gradient."""
    g = GRAPHS[name](cuda_device)
    N = g.num_nodes()
    C, H, W = 5, 9, 9
    x, gb, _, G, base, _, _ = wc.random_operands(g, C, H, W, seed=8, loud=False)
    silent = np.zeros(N, bool)
    silent[[1, 4, N - 2]] = True
    w = torch.as_tensor(~silent).float()[:, None, None].expand(N, H, W).contiguous()
    out, attn, _, dx, dgb, _ = run(cuda_device, g, x, gb, w, G, base=base)
    ref = run_attn(cuda_device, wc.compacted(g, silent), x, gb, G, base=base)
    for a, b in zip((out, attn, dx, dgb), ref):
        assert bits_equal(a, b)


@pytest.mark.parametrize("n", [5, 9, 16])
@pytest.mark.parametrize("shape", [(4, 8, 8), (40, 16, 16)])
@pytest.mark.parametrize("T", [torch.bfloat16, torch.float16])
def test_16_bit_contract(cuda_device, n, shape, T):
    g = wc.complete(n)
    x, gb, _, G, base, w, _ = wc.random_operands(g, *shape, seed=5)
    xT, GT, bT = x.to(T), G.to(T), base.to(T)
    key = {torch.bfloat16: "bf16", torch.float16: "f16"}[T]
    before = aggregate.PATH_COUNTS["wattn_fwd_" + key], aggregate.PATH_COUNTS["wattn_bwd_" + key]
    out, attn, rate, dx, dgb, dw = run(cuda_device, g, xT, gb, w, GT, base=bT)
    assert (aggregate.PATH_COUNTS["wattn_fwd_" + key], aggregate.PATH_COUNTS["wattn_bwd_" + key]) == \
        (before[0] + 1, before[1] + 1)
    assert out.dtype == T and dx.dtype == T
    assert all(t.dtype == torch.float32 for t in (attn, rate, dgb, dw))
    # the fp32 kernels on the widened input, cast
    o32, a32, r32, dx32, dgb32, dw32 = run(cuda_device, g, xT.float(), gb, w, GT.float(), base=bT.float())
    assert bits_equal(out, o32.to(T)) and bits_equal(dx, dx32.to(T))
    assert bits_equal(attn, a32) and bits_equal(rate, r32) and bits_equal(dgb, dgb32) and bits_equal(dw, dw32)
    r = wc.reference(g, xT.float(), gb, w, GT.float(), base=bT.float())
    errs = [rel_err(dgb.numpy(), r[4].numpy()), rel_err(dw.numpy(), r[5].numpy())]
    print(n, shape, T, "dgb, dw", errs)
    assert max(errs) <= TOL


@pytest.mark.parametrize("name", ["complete5", "knn16_4", "range_batch", "loud_csr"])
def test_exact_zeros(cuda_device, name):
    """Where nobody delivered: out, attn, rate and grad_w are exact zeros; rows no CSR entry names are zeros."""
    g = GRAPHS[name](cuda_device)
    C, H, W = 6, 9, 9  # two tiles, the second ragged
    seed = 70  # the all-silent pixel is 70: in the second tile
    x, gb, _, G, _, w, _ = wc.random_operands(g, C, H, W, seed=seed)
    w.view(g.num_nodes(), -1)[:, 3] = 0.0  # and one in the first
    # NaN-filled outputs: what the kernels do not write stays NaN
    dev = cuda_device
    csr = g.csr(dev)
    E, P = g.num_edges(), H * W
    out = torch.full((g.num_nodes(), C, H, W), float("nan"), device=dev)
    attn = torch.full((E, P), float("nan"), device=dev)
    rate = torch.full((E, P), float("nan"), device=dev)
    m.film_wattn_forward_into(x.to(dev), gb.to(dev), w.to(dev), csr, 0, out, attn=attn, rate=rate)
    dx, dgb, dw = m.film_wattn_backward(G.to(dev), x.to(dev), gb.to(dev), w.to(dev), attn, rate, csr, 0, True, True,
                                        True)
    out, attn, rate, dw = out.cpu().view(-1, C, P), attn.cpu(), rate.cpu(), dw.cpu().view(-1, P)
    for p in (3, seed):
        assert bool((out[:, :, p] == 0).all()) and bool((attn[:, p] == 0).all()) and bool((rate[:, p] == 0).all())
        assert bool((dw[:, p] == 0).all())
    for t in (out, attn, dx, dgb):
        assert bool(torch.isfinite(t).all())
    indptr, src, eid = wc.rows(g)
    named = torch.zeros(E, dtype=torch.bool)
    named[torch.as_tensor(eid[: int(indptr[-1])].astype(np.int64))] = True
    if name == "range_batch":
        assert not bool(named.all())
    assert bool((attn[~named] == 0).all()) and bool((rate[~named] == 0).all()) and bool((dgb.cpu()[~named] == 0).all())
    # a node without in-edges: zeros; a silent entry: zero weight, zero grad_gb row where silent on the whole plane
    deg = np.diff(indptr)
    assert bool((out[torch.as_tensor(deg == 0)] == 0).all())
    q, _ = wc.silent_node(g)
    from_q = torch.as_tensor(np.asarray(g.edges()[0]) == q)
    assert bool((attn[from_q] == 0).all()) and bool((dgb.cpu()[from_q] == 0).all())
    assert bool((attn[:, [0, 1, 2]] != 0).any())


@pytest.mark.parametrize("name", ["complete8", "complete16", "loud_csr"])
@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
def test_strided_operands(cuda_device, name, T):
    g = GRAPHS[name](cuda_device)
    C, H, W = 6, 9, 9  # 81 pixels: two tiles, the second ragged; odd strides
    x, gb, _, G, base, w, _ = wc.random_operands(g, C, H, W, seed=4, loud=False)
    dev = cuda_device
    csr = g.csr(dev)
    N, P = x.shape[0], H * W
    dense = run(dev, g, x.to(T), gb, w, G.to(T), base=base.to(T))
    xbuf = torch.full((N, 2 * C, H, W), 7.0, device=dev, dtype=T)
    xbuf[:, :C] = x.to(dev)
    wbuf = torch.full((N, 3, H, W), -1.0, device=dev)  # the map is the middle plane of three: node stride 3 P
    wbuf[:, 1] = w.to(dev)
    cat = torch.full((N, 2 * C, H, W), -5.0, device=dev, dtype=T)
    attn, rate = m.film_wattn_forward_into(xbuf[:, :C], gb.to(dev), wbuf[:, 1], csr, 0, cat[:, C:], rate=True)
    assert bits_equal(cat[:, C:], dense[0]) and bits_equal(attn, dense[1]) and bits_equal(rate, dense[2])
    assert bool((cat[:, :C] == -5.0).all()) and bool((xbuf[:, C:] == 7.0).all())  # the other halves: untouched
    gbuf = torch.full((N, 2 * C, H, W), 3.0, device=dev, dtype=T)
    gbuf[:, C:] = G.to(dev)
    gbuf[:, :C] = base.to(dev)
    dx, dgb, dw = m.film_wattn_backward(gbuf[:, C:], xbuf[:, :C], gb.to(dev), wbuf[:, 1], attn, rate, csr, 0, True,
                                        True, True, grad_x_base=gbuf[:, :C])
    assert bits_equal(dx, dense[3]) and bits_equal(dgb, dense[4]) and bits_equal(dw, dense[5])
    # the C entry point with strided grad_x and grad_w too, into sentinel-filled buffers
    dxbuf = torch.full((N, 2 * C, H, W), 9.0, device=dev, dtype=T)
    dwbuf = torch.full((N, 3, H, W), 9.0, device=dev)
    dgb2 = torch.full((g.num_edges(), C, 2), 9.0, device=dev)
    gbd = gb.to(dev).contiguous()
    lib = _lib.load_library()
    nbytes = lib.mrp_film_wattn_workspace(1, csr.num_graphs, csr.max_nodes, csr.graph_kind, csr.num_nodes,
                                          csr.num_edges, C, P)
    ws = torch.empty(max(nbytes // 4, 1), device=dev)
    ga = aggregate._graph_args(gbd, csr, C, P, 0)
    code = lib.mrp_film_wattn_bwd(aggregate.FEATURE_DTYPES[T], aggregate._ptr(gbuf[:, C:]), 2 * C * P,
                                  aggregate._ptr(xbuf[:, :C]), 2 * C * P, ga[0], aggregate._ptr(wbuf[:, 1]), 3 * P,
                                  *ga[1:], aggregate._ptr(dxbuf[:, :C]), 2 * C * P, aggregate._ptr(gbuf[:, :C]),
                                  2 * C * P, aggregate._ptr(dgb2), ac.default_scale(C), aggregate._ptr(attn),
                                  aggregate._ptr(rate), aggregate._ptr(dwbuf[:, 1]), 3 * P, aggregate._ptr(ws), nbytes,
                                  aggregate._stream(dev))
    assert code == 0
    assert bits_equal(dxbuf[:, :C], dense[3]) and bits_equal(dgb2, dense[4]) and bits_equal(dwbuf[:, 1], dense[5])
    assert bool((dxbuf[:, C:] == 9.0).all()) and bool((dwbuf[:, [0, 2]] == 9.0).all())
    assert bool((wbuf[:, [0, 2]] == -1.0).all())
    # the autograd form of the same composition
    xd = x.to(dev).to(T).requires_grad_(True)
    gbd = gb.to(dev).requires_grad_(True)
    wd = wbuf[:, 1:2].detach().requires_grad_(True)  # (N, 1, H, W), strided
    buf = aggregate.film_wattn_cat(xd, gbd, wd, csr)
    assert bits_equal(buf[:, :C], x.to(T)) and bits_equal(buf[:, C:], dense[0])
    buf.backward(gbuf)
    assert bits_equal(xd.grad, dense[3]) and bits_equal(gbd.grad, dense[4])
    assert bits_equal(wd.grad[:, 0], dense[5])


@pytest.mark.parametrize("name", ["complete8", "complete16", "knn16_4", "loud_csr", "range_batch"])
@pytest.mark.parametrize("shape", [(5, 8, 8), (3, 12, 12)])
def test_outputs_wanted_separately(cuda_device, name, shape):
    g = GRAPHS[name](cuda_device)
    x, _, z, G, base, w, _ = wc.random_operands(g, *shape, seed=3)
    full = run(cuda_device, g, x, z, w, G, base=base, logits=True)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        got = run(cuda_device, g, x, z, w, G, base=base, logits=True, need=need)
        for want, a, b in zip(need, got[3:], full[3:]):
            assert (a is None) if not want else bits_equal(a, b), need
    # without rate (inference): the same out and attn
    dev = cuda_device
    out = torch.empty_like(x, device=dev)
    attn, rate = m.film_wattn_forward_into(x.to(dev), z.to(dev), w.to(dev), g.csr(dev), _lib.GB_LOGITS, out)
    assert rate is None and bits_equal(out, full[0]) and bits_equal(attn, full[1])


def test_no_channels_gives_zeros(cuda_device):
    """C == 0: nothing to score and no kernel runs; the weights, rates and grad_w handed in are written as zeros."""
    g = wc.general_csr()
    dev = cuda_device
    csr = g.csr(dev)
    x = torch.zeros(g.num_nodes(), 0, 4, 4, device=dev)
    gb = torch.zeros(g.num_edges(), 0, 2, device=dev)
    w = torch.rand(g.num_nodes(), 4, 4, device=dev)
    attn = torch.full((g.num_edges(), 16), 3.0, device=dev)
    rate = torch.full((g.num_edges(), 16), 3.0, device=dev)
    got = m.film_wattn_forward_into(x, gb, w, csr, 0, torch.empty_like(x), attn=attn, rate=rate)
    assert got[0] is attn and got[1] is rate and bool((attn == 0).all()) and bool((rate == 0).all())
    dx, dgb, dw = m.film_wattn_backward(x, x, gb, w, attn, rate, csr, 0, True, True, True)
    assert bool((dw == 0).all()) and dx.numel() == 0 and dgb.numel() == 0


def test_deterministic(cuda_device):
    g = wc.knn(16, 4, B=3)
    x, _, z, G, _, w, _ = wc.random_operands(g, 12, 16, 16, seed=7)
    a = run(cuda_device, g, x, z, w, G, logits=True)
    b = run(cuda_device, g, x, z, w, G, logits=True)
    for p, q in zip(a, b):
        assert bits_equal(p, q)


@pytest.mark.parametrize("shape", [(4, 8, 8), (5, 9, 9)])
def test_a_silent_senders_nan_is_contained(cuda_device, shape):
    """NaN and infinities in the features of a sender that is silent everywhere (and has no row of its own: its
    features are also its row's query) change nothing but that sender's rate and grad_w."""
    g = wc.loud_csr()
    C, H, W = shape
    x, gb, _, G, base, w, _ = wc.random_operands(g, C, H, W, seed=6, loud=False)
    q, rowless = wc.silent_node(g)
    assert rowless and bool((w[q] == 0).all())
    clean = run(cuda_device, g, x, gb, w, G, base=base)
    xs = x.clone()
    xs[q, 0, 1, 2] = float("nan")
    xs[q, C - 1, 3, 4] = float("inf")
    xs[q, 1, 5, 5] = -float("inf")
    xs[q, :, 6, 6] = 3.0e38
    got = run(cuda_device, g, xs, gb, w, G, base=base)
    src = np.asarray(g.edges()[0])
    own = torch.as_tensor(src == q)
    for k, a, b in zip(NAMES, got, clean):
        if k == "rate":
            assert bits_equal(a[~own], b[~own])
            assert not bool(torch.isfinite(a[own]).all())  # it does reach the sender's own rate
        elif k == "dw":
            keep = torch.arange(x.shape[0]) != q
            assert bits_equal(a[keep], b[keep])
            assert not bool(torch.isfinite(a[q]).all())
        else:
            assert bits_equal(a, b), k


def test_autograd_layouts_and_weights(cuda_device):
    g = wc.complete(8)
    C, H, W = 8, 8, 8
    x, gb, z, G, base, w, _ = wc.random_operands(g, C, H, W, seed=8)
    dev = cuda_device
    csr = g.csr(dev)
    r = wc.reference(g, x, z, w, G, logits=True)
    res = {}
    for fmt in (torch.contiguous_format, torch.channels_last):
        xd = x.to(dev).contiguous(memory_format=fmt).requires_grad_(True)
        zd = z.to(dev).requires_grad_(True)
        wd = w.to(dev).requires_grad_(True)
        before = aggregate.PATH_COUNTS["wattn_fwd_f32"], aggregate.PATH_COUNTS["wattn_bwd_f32"]
        out, attn = m.film_wattn(xd, zd, wd, csr, logits=True, return_weights=True)
        assert not attn.requires_grad and tuple(attn.shape) == (g.num_edges(), H * W)
        out.backward(G.to(dev))
        assert (aggregate.PATH_COUNTS["wattn_fwd_f32"], aggregate.PATH_COUNTS["wattn_bwd_f32"]) == \
            (before[0] + 1, before[1] + 1)
        assert close(out, r[0]) and close(attn, r[1]) and close(xd.grad, r[3]) and close(zd.grad, r[4])
        assert close(wd.grad, r[5]) and wd.grad.shape == w.shape
        res[fmt] = (out.detach().contiguous(), attn, xd.grad.contiguous(), zd.grad, wd.grad)
    for a, b in zip(res[torch.contiguous_format], res[torch.channels_last]):
        assert bits_equal(a, b)  # copied to NCHW first: the same kernels on the same values
    # maps that need no gradient: no rate is computed, the other gradients are the same bits
    xd = x.to(dev).requires_grad_(True)
    zd = z.to(dev).requires_grad_(True)
    out = m.film_wattn(xd, zd, w.to(dev)[:, None], csr, logits=True)  # (N, 1, H, W)
    out.backward(G.to(dev))
    assert bits_equal(xd.grad, res[torch.contiguous_format][2]) and bits_equal(zd.grad, res[torch.contiguous_format][3])
    # the concatenated form, with an explicit scale
    xd = x.to(dev).requires_grad_(True)
    zd = z.to(dev).requires_grad_(True)
    wd = w.to(dev).requires_grad_(True)
    buf = m.film_wattn_cat(xd, zd, wd, csr, logits=True, scale=0.2)
    buf.backward(torch.cat((base, G), 1).to(dev))
    rc = wc.reference(g, x, z, w, G, base=base, logits=True, scale=0.2)
    assert bits_equal(buf[:, :C], x) and close(buf[:, C:], rc[0])
    assert close(xd.grad, rc[3]) and close(zd.grad, rc[4]) and close(wd.grad, rc[5])
    # plain torch ops around the operator
    y = aggregate.film_wattn_residual(x.to(dev), z.to(dev), w.to(dev), csr, logits=True)
    assert close(y, x.double() + r[0])
    y = aggregate.film_wattn_mix(x.to(dev), z.to(dev), w.to(dev), csr, base.to(dev), 0.25, logits=True)
    assert close(y, 0.75 * r[0] + 0.25 * base.double())


# ------------------------------------------------------------------------------------------------ the model
TAU = 0.5  # the head's gate: sigmoid(conv(x)) of a freshly initialised head straddles it


def _opt(C, layers, combine, scale=None, head=True, mode="film_wattn"):
    opt = types.SimpleNamespace(feature_dim=C, gcn_mode=mode, gcn_layers=layers, gcn_combine=combine, gcn2_alpha=0.25)
    if head:
        opt.gcn_confidence, opt.gcn_confidence_threshold = True, TAU
    if scale is not None:
        opt.gcn_attn_scale = scale
    return opt


def _stack(C, layers, combine, scale=None, head=True, mode="film_wattn"):
    torch.manual_seed(0)
    return m.GCNStack(_opt(C, layers, combine, scale, head, mode))


def _inputs(g, C, H, W, T, seed=1):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g.num_nodes(), C, H, W, generator=gen).to(T).float()
    return x, torch.randn(x.shape, generator=gen)


def _check_model(dev, net, call, g, pose, x, G, layers, combine, scale=None):
    params = {k: v.detach() for k, v in net.named_parameters()}
    xd = x.to(dev).requires_grad_(True)
    before = aggregate.PATH_COUNTS["wattn_fwd_f32"], aggregate.PATH_COUNTS["wattn_bwd_f32"]
    out = call(xd)
    out.backward(G.to(dev))
    assert aggregate.PATH_COUNTS["wattn_fwd_f32"] == before[0] + layers
    assert aggregate.PATH_COUNTS["wattn_bwd_f32"] == before[1] + layers
    r_out, r_dx, r_p, gap = wc.stack_reference(params, g, x, pose, G, layers, combine, 0.25, scale=scale, tau=TAU)
    # the gate is a comparison: the two evaluations agree on it only where no confidence sits on the threshold.
    # 4e-6 is 64 fp32 spacings at 0.5; the head's fp32 sigmoid(conv) is within a few of them of the float64 one
    assert gap > 4e-6, gap
    assert close(out, r_out)
    assert close(xd.grad, r_dx)
    for k, p in net.named_parameters():
        assert close(p.grad, r_p[k]), k
    assert any("confidence" in k for k, _ in net.named_parameters())
    return out.detach()


@pytest.mark.parametrize("scale", [None, 0.5])
@pytest.mark.parametrize("combine", ["cat_compress", "cat", "residual", "initial_mix"])
def test_model_stack_fp32(cuda_device, combine, scale):
    C, H, W = 8, 4, 4
    layers = 1 if combine == "cat" else 2  # stacked layers need a compress (models.stack_layout)
    g = m.batch([m.frame_graph(p) for p in _frames(2, 8, seed=3)])
    net = _stack(C, layers, combine, scale).to(cuda_device)
    x, G = _inputs(g, C, H, W, torch.float32)
    if combine == "cat":
        G = torch.cat((G, G.flip(0)), 1)
    gd = g.to(cuda_device)
    _check_model(cuda_device, net, lambda t: net(gd, t), gd, g.edata["pose"], x, G, layers, combine, scale)
    with torch.no_grad():
        gated = net.gcn1.confidence_map(x.to(cuda_device))
    assert bool((gated == 0).any()) and bool((gated != 0).any())  # the threshold silences some, not all


U_BF16 = 2.0 ** -8  # bf16's spacing relative to a value in [1, 2): one rounding moves a value by at most half of it


def _layer(net, gd, i, h, h0):
    """Layer i of the stack, as models._run_stack composes it."""
    gcn = getattr(net, f"gcn{i}")
    if net.gcn_combine == "cat_compress":
        return gcn.forward_cat_compress(gd, h, getattr(net, f"conv{i}"))
    if net.gcn_combine == "cat":
        return gcn.forward_cat(gd, h)
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


@pytest.mark.parametrize("combine", ["cat_compress", "cat", "residual", "initial_mix"])
def test_model_stack_bf16(cuda_device, combine):
    """A stack on bf16 features, held to the fp32 run on the same bf16-valued input, layer by layer, with the
    bounds and the argument of tests/test_gpu_film_attn.py::test_model_stack_bf16: each bf16 layer is compared
    with the fp32 evaluation of that layer on the widened bf16 tensors it actually received (forward 3 u / 2,
    gradients 4 u, max-abs relative).  The confidence head reads the widened features in fp32 in both
    evaluations, so the maps and the gate are the same bits and, by the 16-bit contract, so are the scores, the
    weights and the rates.  The head adds one fp32 gradient term to dh, rounded to bf16 and added in bf16: two more
    roundings of at most u / 2 each, inside the 4 u."""
    C, H, W = 8, 4, 4
    layers = 1 if combine == "cat" else 2
    dev = cuda_device
    bf = torch.bfloat16
    g = m.batch([m.frame_graph(p) for p in _frames(2, 8, seed=3)])
    gd = g.to(dev)
    net = _stack(C, layers, combine).to(dev)
    x, G = _inputs(g, C, H, W, bf)
    if combine == "cat":
        G = torch.cat((G, G.flip(0)), 1)
    G = G.to(bf).float().to(dev)  # a bf16-valued output gradient
    xb = x.to(dev).to(bf)
    before = aggregate.PATH_COUNTS["wattn_fwd_bf16"], aggregate.PATH_COUNTS["wattn_bwd_bf16"]
    net.zero_grad(set_to_none=True)
    leaf = xb.clone().requires_grad_(True)
    out = net(gd, leaf)
    out.backward(G.to(bf))
    whole = out.detach(), leaf.grad, {k: p.grad.clone() for k, p in net.named_parameters()}
    assert whole[0].dtype == bf and whole[1].dtype == bf
    assert aggregate.PATH_COUNTS["wattn_fwd_bf16"] == before[0] + layers
    assert aggregate.PATH_COUNTS["wattn_bwd_bf16"] == before[1] + layers
    # the same stack as a chain of its bf16 layers
    if layers == 2:
        with torch.no_grad():
            h1 = _layer(net, gd, 1, xb, xb)
        got2 = _run_layer(net, gd, 2, h1, xb, G)
        dh1 = got2[1]
        got1 = _run_layer(net, gd, 1, xb, xb, dh1.float())
        assert bits_equal(got2[0], whole[0])
        for k, v in {**got1[2], **got2[2]}.items():
            if "confidence" in k:
                # the head is torch's convolution: its parameter gradients are fp32 sums over nodes and pixels in
                # an order torch does not fix, so they are held to the fp32 bar, not to bits
                assert rel_err(v.float().cpu().numpy(), whole[2][k].float().cpu().numpy()) <= TOL, k
            else:
                assert bits_equal(v, whole[2][k]), k
        ref2 = _run_layer(net, gd, 2, h1.float(), xb.float(), G)
        ref1 = _run_layer(net, gd, 1, xb.float(), xb.float(), dh1.float())
        pairs = ((1, (h1,) + got1[1:], ref1), (2, got2, ref2))
    else:
        got1 = _run_layer(net, gd, 1, xb, xb, G)
        assert bits_equal(got1[0], whole[0]) and bits_equal(got1[1], whole[1])
        pairs = ((1, got1, _run_layer(net, gd, 1, xb.float(), xb.float(), G)),)
    for i, got, ref in pairs:
        e = rel_err(got[0].float().cpu().numpy(), ref[0].cpu().numpy())
        print(combine, "layer", i, "forward", e, "bar", 3 * U_BF16 / 2)
        assert e <= 3 * U_BF16 / 2
        e = rel_err(got[1].float().cpu().numpy(), ref[1].cpu().numpy())
        print(combine, "layer", i, "dh", e, "bar", 4 * U_BF16)
        assert e <= 4 * U_BF16
        assert set(got[2]) == set(ref[2]) and any("confidence" in k for k in got[2])
        for k in ref[2]:
            e = rel_err(got[2][k].float().cpu().numpy(), ref[2][k].cpu().numpy())
            print(combine, "layer", i, k, e, "bar", 4 * U_BF16)
            assert e <= 4 * U_BF16, k


def test_model_step_on_a_device_built_range_graph(cuda_device):
    C, H, W, layers = 8, 4, 4, 1
    g = range_batch(cuda_device)
    torch.manual_seed(0)
    net = m.multi_view_dgl_model(types.SimpleNamespace(feature_dim=C, gcn_mode="film_wattn", compress_gcn=True,
                                                       multi_gcn=False, gcn_confidence=True,
                                                       gcn_confidence_threshold=TAU)).to(cuda_device)
    pose = g.edata["pose"].cpu()
    x, G = _inputs(g, C, H, W, torch.float32)

    def call(t):
        g.ndata["image"] = t
        return net(g)
    _check_model(cuda_device, net, call, g, pose, x, G, layers, "cat_compress")
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    opt.step()  # the gradients of the step above
    assert all(not torch.equal(p.detach(), before[k]) for k, p in net.named_parameters())


@pytest.mark.parametrize("combine", ["cat_compress", "cat", "residual", "initial_mix"])
def test_mode_without_weights_is_film_attn_bit_for_bit(cuda_device, combine):
    C, H, W = 8, 4, 4
    layers = 1 if combine == "cat" else 2
    dev = cuda_device
    g = m.batch([m.frame_graph(p) for p in _frames(2, 8, seed=3)]).to(dev)
    x, G = _inputs(g, C, H, W, torch.float32)
    if combine == "cat":
        G = torch.cat((G, G.flip(0)), 1)
    res = []
    for mode in ("film_wattn", "film_attn"):
        net = _stack(C, layers, combine, 0.4, head=False, mode=mode).to(dev)
        xd = x.to(dev).requires_grad_(True)
        before = aggregate.PATH_COUNTS["attn_fwd_f32"], aggregate.PATH_COUNTS["wattn_fwd_f32"]
        out = net(g, xd)
        out.backward(G.to(dev))
        assert aggregate.PATH_COUNTS["attn_fwd_f32"] == before[0] + layers  # film_attn's own kernels
        assert aggregate.PATH_COUNTS["wattn_fwd_f32"] == before[1]
        res.append((out.detach(), xd.grad, *[p.grad for p in net.parameters()]))
    assert len(res[0]) == len(res[1])
    for a, b in zip(*res):
        assert bits_equal(a, b)
    # explicit maps reach the gated kernels through every forward
    net = m.GCN(_opt(C, 1, "cat", head=False)).to(dev)
    w = torch.rand(x.shape[0], H, W, device=dev)
    before = aggregate.PATH_COUNTS["wattn_fwd_f32"]
    with torch.no_grad():
        net(g, x.to(dev), weights=w)
        net.forward_cat(g, x.to(dev), weights=w)
        net.forward_residual(g, x.to(dev), weights=w)
        net.forward_mix(g, x.to(dev), x.to(dev), 0.25, weights=w)
        net.forward_cat_compress(g, x.to(dev), torch.nn.Conv2d(2 * C, C, 1).to(dev), weights=w)
    assert aggregate.PATH_COUNTS["wattn_fwd_f32"] == before + 5
