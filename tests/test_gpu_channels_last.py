"""GPU: the FiLM-mean aggregation on pixel-major (``torch.channels_last``) feature maps
(``mrp_film_mean_fwd_cl`` / ``mrp_film_mean_bwd_cl``), fp32, bf16 and fp16.

Contract: the arithmetic is the NCHW kernels', operation for operation, so

* forward: ``film_mean(x_cl, ...) == film_mean(x_cl.contiguous(), ...)`` bit for bit (as values), for every
  graph kind, mode, epilogue, ``logits`` and dtype, and the result is channels_last;
* ``grad_x`` for graphs of <= 8 nodes: bit-equal to the NCHW path's (one fmaf chain per element on both
  sides); for 9-16 nodes (the NCHW path may sum in another grouping) it is held to the float64 oracle;
* ``grad_gb`` (fp32, summed over the pixels in an order of its own): ``rel_err <= max(1e-5, 4 x the error
  of the same oracle in float32)`` against float64, for gamma/beta and for logits;
* deterministic; a node-major ``grad_out`` is converted once; ``set_channels_last("convert")`` is the
  route before these kernels existed.

Without the feature the outputs come back NCHW-contiguous and no ``fwd_cl_*`` counter moves.

Cases (graphs from ``half_cases``' builders):

====  ==========================  ==  =====  ==========================================================
a     2 complete, 8 nodes         64  8x8    vector path, a full channel block, <= 8-node backward
b     2 complete, 5 nodes         40  6x6    last channel block partly filled, odd pixel counts per pass
c     2 complete, 4 nodes          6  5x5    C * sizeof(T) % 16 != 0: one element per access
d     1 complete, 3 nodes          3  3x3    everything odd
e     2 x 16 nodes, k-NN(4)       32  8x8    REGULAR(4) slots, 9-16-node backward
f     1 complete, 12 nodes        16  4x4    132 slots, four destination blocks in the Gram pass
f16   1 complete, 16 nodes         8  4x4    240 slots: the LDS tile budget and channel-block choice
g     ragged 2 / 5 / 8 nodes      16  4x4    CSR: in-degree 0, a multi-edge, a self-loop
h     as b, x = buf[:, C:]        40  6x6    pixel stride 2C on input (and through cat on output, grads)
i     as a, x = buf[:, 1:C+1]     64  8x8    misaligned start: element path with pixel stride C + 2
j     2 complete, 8 nodes          8  32x32  many pixels per lane, plane split, workspace reduction
====  ==========================  ==  =====  ==========================================================
"""
import functools
import types

import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib, aggregate
import half_cases as hc
import oracle
import stack_ref
from conftest import rel_err

pytestmark = pytest.mark.gpu

CL = torch.channels_last
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
KEYS = list(DTYPES)
CASES = {
    "a": (lambda: hc._frames([8, 8], 1), 64, 8, 8),
    "b": (lambda: hc._frames([5, 5], 2), 40, 6, 6),
    "c": (lambda: hc._frames([4, 4], 3), 6, 5, 5),
    "d": (lambda: hc._frames([3], 4), 3, 3, 3),
    "e": (lambda: hc._frames([16, 16], 5, knn=4), 32, 8, 8),
    "f": (lambda: hc._frames([12], 6), 16, 4, 4),
    "f16": (lambda: hc._frames([16], 8), 8, 4, 4),
    "g": (lambda: hc._ragged(7), 16, 4, 4),
    "h": (lambda: hc._frames([5, 5], 2), 40, 6, 6),
    "i": (lambda: hc._frames([8, 8], 1), 64, 8, 8),
    "j": (lambda: hc._frames([8, 8], 9), 8, 32, 32),
}
ALL = list(CASES)
BIG = ["e", "f", "f16"]  # 9-16 nodes: the NCHW backward may group its sums differently
SMALL = [c for c in ALL if c not in BIG]
ALPHA = 0.1


@functools.lru_cache(maxsize=None)
def graph(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def host_inputs(name, key):
    """(x, gb, z, G, G0, x0) on the CPU: features drawn in fp32 and rounded to T, logits z fp32 with
    gb = sigmoid(z); G0 is the first half of a cat's incoming gradient, x0 the mix's second tensor."""
    T = DTYPES[key]
    _, C, H, W = CASES[name]
    n = graph(name).num_nodes()
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 977 + KEYS.index(key))
    x, G, G0, x0 = (torch.randn(n, C, H, W, generator=gen).to(T) for _ in range(4))
    z = torch.randn(graph(name).num_edges(), C, 2, generator=gen)
    return x, torch.sigmoid(z), z, G, G0, x0


def embed(name, x):
    """A pixel-major device tensor holding x's values: (leaf, view) with view(leaf) == x."""
    n, C, H, W = x.shape
    if name == "h":  # the second half of a channels_last concatenation buffer: pixel stride 2C
        leaf = torch.zeros(n, 2 * C, H, W, dtype=x.dtype, device=x.device).contiguous(memory_format=CL)
        leaf[:, C:] = x
        return leaf, (lambda t: t[:, C:])
    if name == "i":  # one channel into a (C + 2)-channel buffer: no 16-byte alignment, pixel stride C + 2
        leaf = torch.zeros(n, C + 2, H, W, dtype=x.dtype, device=x.device).contiguous(memory_format=CL)
        leaf[:, 1:C + 1] = x
        return leaf, (lambda t: t[:, 1:C + 1])
    return x.contiguous(memory_format=CL).clone(memory_format=torch.preserve_format), (lambda t: t)


@functools.lru_cache(maxsize=None)
def oracle_ref(name, key):
    """float64 and float32 oracle gradients of film_mean on the widened inputs: dx, dgb and (through
    gb = sigmoid(z)) dz, for grad_out G."""
    x, _, z, G, _, _ = host_inputs(name, key)
    src, dst = (t.numpy() for t in graph(name).edges())
    ref = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        xx = x.to(dt).requires_grad_(True)
        zz = z.to(dt).requires_grad_(True)
        gb = torch.sigmoid(zz)
        gb.retain_grad()
        oracle.film_aggregate(xx, gb, src, dst, "film_mean").backward(G.to(dt))
        ref["dx" + tag], ref["dgb" + tag], ref["dz" + tag] = xx.grad, gb.grad.detach(), zz.grad
    return ref


def _apply(op, x, gb, csr, logits, x0=None):
    if op == "cat":
        return m.film_mean_cat(x, gb, csr, logits=logits)
    if op == "residual":
        return m.film_mean_residual(x, gb, csr, logits=logits)
    if op == "mix":
        return m.film_mean_mix(x, gb, csr, x0, ALPHA, logits=logits)
    return m.film_mean(x, gb, csr, op, logits=logits)


def _cl_counts():
    return {k: v for k, v in aggregate.PATH_COUNTS.items() if "_cl_" in k}


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("key", KEYS)
def test_forward_bit_equal_to_nchw_kernels(cuda_device, key, name, logits):
    dev = cuda_device
    x, gb, z, _, _, x0 = (t.to(dev) for t in host_inputs(name, key))
    w = z if logits else gb
    csr = graph(name).csr(dev)
    leaf, view = embed(name, x)
    xv = view(leaf)
    assert aggregate.pixel_strides(xv) is not None and aggregate.node_stride(xv) is None
    x0cl = x0.contiguous(memory_format=CL)
    C = x.shape[1]
    with torch.no_grad():
        for op in ("film_mean", "film_sum", "copy_mean", "residual", "mix", "cat"):
            before = aggregate.PATH_COUNTS["fwd_cl_" + key]
            got = _apply(op, xv, w, csr, logits, x0cl)
            assert aggregate.PATH_COUNTS["fwd_cl_" + key] == before + 1, op
            assert got.is_contiguous(memory_format=CL) and got.dtype == x.dtype, op
            ref = _apply(op, xv.contiguous(), w, csr, logits, x0)
            assert aggregate.PATH_COUNTS["fwd_cl_" + key] == before + 1, op  # the reference leg: NCHW kernels
            assert ref.is_contiguous()
            assert torch.equal(hc.bits(got.contiguous()), hc.bits(ref.contiguous())), (op, name, key)
            if op == "cat":  # the first half holds x's own bits
                assert torch.equal(hc.bits(got[:, :C].contiguous()), hc.bits(x))


def _backward(op, leaf, view, w, csr, G, logits):
    leaf = leaf.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    out = _apply(op, view(leaf), w, csr, logits)
    out.backward(G)
    return view(leaf.grad), w.grad, out


def _grad_out(op, G, G0, cl):
    g = torch.cat((G0, G), 1) if op == "cat" else G  # cat: the first half is grad_x's base
    return g.contiguous(memory_format=CL) if cl else g.contiguous()


@pytest.mark.parametrize("op", ["film_mean", "residual", "cat"])
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("key", KEYS)
def test_grad_x(cuda_device, key, name, op):
    """<= 8 nodes: bit-equal to the NCHW path.  9-16 nodes: against float64 (16-bit: one rounding of T
    elementwise; fp32: within max(1e-5, 4 x the fp32 oracle's error))."""
    T = DTYPES[key]
    dev = cuda_device
    x, gb, z, G, G0, _ = (t.to(dev) for t in host_inputs(name, key))
    csr = graph(name).csr(dev)
    leaf, view = embed(name, x)
    before = aggregate.PATH_COUNTS["bwd_cl_" + key]
    dx, dz, out = _backward(op, leaf, view, z, csr, _grad_out(op, G, G0, True), True)
    assert aggregate.PATH_COUNTS["bwd_cl_" + key] == before + 1
    assert dx.dtype == T and dz.dtype == torch.float32 and out.is_contiguous(memory_format=CL)
    if name in SMALL:
        dxr, _, _ = _backward(op, x.contiguous(), lambda t: t, z, csr, _grad_out(op, G, G0, False), True)
        assert aggregate.PATH_COUNTS["bwd_cl_" + key] == before + 1
        assert torch.equal(hc.bits(dx.contiguous()), hc.bits(dxr)), (name, key, op)
        return
    ref = oracle_ref(name, key)
    extra = {"film_mean": None, "residual": G, "cat": G0}[op]  # d out / d x beside the aggregate's
    r64, r32 = ref["dx64"], ref["dx32"]
    if extra is not None:
        r64, r32 = r64 + extra.cpu().double(), r32 + extra.cpu().float()
    if key == "f32":
        ok, errs = stack_ref.within(dx.detach().cpu(), r32, r64)
        print(name, key, op, "grad_x err, fp32 oracle err", errs)
        assert ok, (name, op, errs)
    else:
        hc.assert_elementwise(dx, r64, T, (name, key, op))


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("key", KEYS)
def test_grad_gb_against_float64(cuda_device, key, name):
    dev = cuda_device
    x, gb, z, G, _, _ = (t.to(dev) for t in host_inputs(name, key))
    csr = graph(name).csr(dev)
    leaf, view = embed(name, x)
    Gcl = G.contiguous(memory_format=CL)
    ref = oracle_ref(name, key)
    _, dgb, _ = _backward("film_mean", leaf, view, gb, csr, Gcl, False)
    _, dz, _ = _backward("film_mean", leaf, view, z, csr, Gcl, True)
    for what, got, tag in (("dgb", dgb, "dgb"), ("dz", dz, "dz")):
        print(name, key, what, "rel_err", rel_err(got.cpu().numpy(), ref[tag + "64"].numpy()),
              "fp32 oracle", rel_err(ref[tag + "32"].numpy(), ref[tag + "64"].numpy()))
        hc.assert_relative(got, ref[tag + "32"], ref[tag + "64"], (name, key, what))
    # copy_mean: gamma/beta do not reach the output
    dxc, dgbc = aggregate.film_mean_backward(Gcl, view(leaf), gb, csr, _lib.MODE_COPY_MEAN, True, True)
    assert dgbc.shape == gb.shape and not dgbc.any() and dxc.is_contiguous(memory_format=CL)


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("key", KEYS)
def test_one_gradient_alone_gives_the_same_bits(cuda_device, key, name):
    dev = cuda_device
    x, gb, z, G, _, _ = (t.to(dev) for t in host_inputs(name, key))
    csr = graph(name).csr(dev)
    leaf, view = embed(name, x)
    Gcl = G.contiguous(memory_format=CL)
    mode = _lib.MODE_FILM_MEAN | _lib.GB_LOGITS
    dx, dgb = aggregate.film_mean_backward(Gcl, view(leaf), z, csr, mode, True, True)
    dx1, none1 = aggregate.film_mean_backward(Gcl, view(leaf), z, csr, mode, True, False)
    none2, dgb2 = aggregate.film_mean_backward(Gcl, view(leaf), z, csr, mode, False, True)
    assert none1 is None and none2 is None
    assert torch.equal(hc.bits(dx), hc.bits(dx1)) and torch.equal(hc.bits(dgb), hc.bits(dgb2))


@pytest.mark.parametrize("name", ["j", "f16"])
@pytest.mark.parametrize("key", KEYS)
def test_deterministic(cuda_device, key, name):
    dev = cuda_device
    x, gb, z, G, _, _ = (t.to(dev) for t in host_inputs(name, key))
    csr = graph(name).csr(dev)
    xcl, Gcl = x.contiguous(memory_format=CL), G.contiguous(memory_format=CL)
    runs = []
    for _ in range(2):
        with torch.no_grad():
            out = m.film_mean(xcl, z, csr, logits=True)
        dx, dz = aggregate.film_mean_backward(Gcl, xcl, z, csr, _lib.MODE_FILM_MEAN | _lib.GB_LOGITS, True, True)
        runs.append((out, dx, dz))
    for a, b in zip(*runs):
        assert torch.equal(hc.bits(a), hc.bits(b))


@pytest.mark.parametrize("key", KEYS)
def test_node_major_grad_out_is_converted(cuda_device, key):
    dev = cuda_device
    x, gb, z, G, _, _ = (t.to(dev) for t in host_inputs("b", key))
    csr = graph("b").csr(dev)
    leaf, view = embed("b", x)
    dx_cl, dz_cl, _ = _backward("film_mean", leaf, view, z, csr, G.contiguous(memory_format=CL), True)
    before = aggregate.PATH_COUNTS["bwd_cl_" + key]
    dx_nm, dz_nm, _ = _backward("film_mean", leaf, view, z, csr, G.contiguous(), True)
    assert aggregate.PATH_COUNTS["bwd_cl_" + key] == before + 1
    assert torch.equal(hc.bits(dx_cl), hc.bits(dx_nm)) and torch.equal(hc.bits(dz_cl), hc.bits(dz_nm))


@pytest.mark.parametrize("key", KEYS)
def test_convert_route_is_the_previous_behaviour(cuda_device, key):
    dev = cuda_device
    x, gb, z, G, _, _ = (t.to(dev) for t in host_inputs("a", key))
    csr = graph("a").csr(dev)
    xcl = x.contiguous(memory_format=CL)
    dx_ref, dz_ref, ref = _backward("film_mean", x.contiguous(), lambda t: t, z, csr, G, True)
    assert aggregate.set_channels_last("convert") == "native"
    try:
        counts = _cl_counts()
        dx, dz, out = _backward("film_mean", xcl, lambda t: t, z, csr, G.contiguous(memory_format=CL), True)
        assert _cl_counts() == counts  # no pixel-major kernel ran
        assert out.is_contiguous() and not out.is_contiguous(memory_format=CL)
        assert torch.equal(hc.bits(out), hc.bits(ref))
        assert torch.equal(hc.bits(dx), hc.bits(dx_ref)) and torch.equal(hc.bits(dz), hc.bits(dz_ref))
    finally:
        assert aggregate.set_channels_last("native") == "convert"


def _module_inputs(dev):
    g = graph("b")
    _, C, H, W = CASES["b"]
    x = host_inputs("b", "bf16")[0].to(dev)
    return g.to(dev), x, C


def _param_grads(module, run):
    module.zero_grad(set_to_none=True)
    out = run()
    out.float().square().sum().backward()
    return out.detach(), {k: p.grad.detach().clone() for k, p in module.named_parameters()}


@pytest.mark.parametrize("which", ["residual_stack", "forward_cat"])
def test_modules_take_and_return_channels_last(cuda_device, which):
    """bf16 channels_last features through a two-layer residual ``GCNStack`` / ``GCN.forward_cat``: the
    output is channels_last and bit-equal to the same module on the contiguous input, with no conversion
    in between (every layer's launch is a pixel-major one); the parameter gradients of the two runs agree
    to 1e-5 (the floor of the grad_gb bar: both runs receive bit-equal incoming gradients)."""
    dev = cuda_device
    gd, x, C = _module_inputs(dev)
    torch.manual_seed(5)
    if which == "residual_stack":
        mod = m.GCNStack(types.SimpleNamespace(feature_dim=C, gcn_layers=2, gcn_combine="residual")).to(dev)
        layers, run = 2, (lambda t: mod(gd, t))
    else:
        mod = m.GCN(types.SimpleNamespace(feature_dim=C)).to(dev)
        layers, run = 1, (lambda t: mod.forward_cat(gd, t))
    xcl = x.contiguous(memory_format=CL)
    before = aggregate.PATH_COUNTS["fwd_cl_bf16"], aggregate.PATH_COUNTS["bwd_cl_bf16"]
    leaf = xcl.clone(memory_format=torch.preserve_format).requires_grad_(True)
    out, grads = _param_grads(mod, lambda: run(leaf))
    assert aggregate.PATH_COUNTS["fwd_cl_bf16"] == before[0] + layers
    assert aggregate.PATH_COUNTS["bwd_cl_bf16"] == before[1] + layers
    assert out.is_contiguous(memory_format=CL) and out.dtype == torch.bfloat16
    leaf_nm = x.contiguous().clone().requires_grad_(True)
    ref, grads_nm = _param_grads(mod, lambda: run(leaf_nm))
    assert aggregate.PATH_COUNTS["fwd_cl_bf16"] == before[0] + layers
    assert torch.equal(hc.bits(out), hc.bits(ref))
    assert torch.equal(hc.bits(leaf.grad), hc.bits(leaf_nm.grad))  # 5-node graphs: the same fmaf chains
    for k in grads:
        e = rel_err(grads[k].cpu().numpy(), grads_nm[k].cpu().numpy())
        print(which, k, "param grad rel_err vs the contiguous run", e)
        assert e <= 1e-5, (k, e)


def test_capture_and_replay(cuda_device):
    """One no-grad bf16 channels_last ``film_mean`` captured into a graph and replayed equals the eager run."""
    dev = cuda_device
    x, gb = (t.to(dev) for t in host_inputs("b", "bf16")[:2])
    x = x.contiguous(memory_format=CL)
    csr = graph("b").csr(dev)
    with torch.no_grad():
        eager = m.film_mean(x, gb, csr)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            m.film_mean(x, gb, csr)  # warm the allocator outside the capture
            torch.cuda.current_stream().synchronize()
            with torch.cuda.graph(cg, stream=side):
                out = m.film_mean(x, gb, csr)
    out.zero_()
    torch.cuda.synchronize()
    cg.replay()
    torch.cuda.synchronize()
    assert out.is_contiguous(memory_format=CL) and torch.equal(hc.bits(out), hc.bits(eager))


def test_capture_and_replay_backward_with_workspace(cuda_device):
    """The backward of case j (a split plane: the op allocates the workspace, then the grad_x sweep, the
    Gram pass and the ordered finish pass) captured into a graph and replayed equals the eager run."""
    dev = cuda_device
    x, _, z, G = (t.to(dev).contiguous(memory_format=CL) if t.dim() == 4 else t.to(dev)
                  for t in host_inputs("j", "bf16")[:4])
    csr = graph("j").csr(dev)
    mode = _lib.MODE_FILM_MEAN | _lib.GB_LOGITS
    _, C, H, W = CASES["j"]
    assert _lib.load_library().mrp_film_mean_bwd_cl_workspace(csr.num_graphs, csr.max_nodes, csr.graph_kind, C,
                                                              H * W, mode, 1) > 0
    with torch.no_grad():
        dx_e, dz_e = aggregate.film_mean_backward(G, x, z, csr, mode, True, True)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            aggregate.film_mean_backward(G, x, z, csr, mode, True, True)  # warm the allocator outside the capture
            torch.cuda.current_stream().synchronize()
            with torch.cuda.graph(cg, stream=side):
                dx, dz = aggregate.film_mean_backward(G, x, z, csr, mode, True, True)
    dx.zero_()
    dz.zero_()
    torch.cuda.synchronize()
    cg.replay()
    torch.cuda.synchronize()
    assert torch.equal(hc.bits(dx), hc.bits(dx_e)) and torch.equal(hc.bits(dz), hc.bits(dz_e))
