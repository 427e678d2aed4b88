"""GPU: ``GCNStack(cat_compress)`` on bf16 / fp16 feature maps with fp32 parameters through the native
16-bit compress (``compress_half.hip``), outside ``torch.autocast`` and inside it, against the fp32 stack,
the float64 restatement (``stack_ref.run``) and the earlier route (the 16-bit cat kernel + torch's
convolution under autocast, ``compress.set_half_compress("torch")``); and a stream capture of one layer."""
import contextlib
import types

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib, compress
import half_cases as hc
import stack_ref
from conftest import rel_err

pytestmark = pytest.mark.gpu

KEYS = list(hc.DTYPES)
C, HW = 32, 8
#: name -> (node counts, k-NN k or None, layers)
CASES = {"two_complete_5": ((5, 5), None, 2), "knn4_16": ((16,), 4, 1)}
GROUPS = ("dx", "conv", "encoder")


def _frames(ns, knn, seed):
    rng = np.random.RandomState(seed)
    graphs = []
    for n in ns:
        poses = np.concatenate([rng.uniform(-10, 10, (n, 3)), rng.standard_normal((n, 4))], 1).astype(np.float32)
        graphs.append(m.frame_graph(poses, knn=knn))
    g = m.batch(graphs)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g.num_nodes(), C, HW, HW, generator=gen)
    G = torch.randn(g.num_nodes(), C, HW, HW, generator=gen)
    return g, x, G


def _run(stack, gd, xT, GT, dev, autocast):
    """(out, dx, {param: grad}, PATH_COUNTS deltas) of one forward + backward of ``GT``."""
    for p in stack.parameters():
        p.grad = None
    leaf = xT.to(dev).requires_grad_(True)
    before = dict(compress.PATH_COUNTS)
    ctx = torch.autocast("cuda", dtype=xT.dtype) if autocast else contextlib.nullcontext()
    with ctx:
        out = stack(gd, leaf)
    out.backward(GT.to(dev))
    moved = {k: v - before.get(k, 0) for k, v in compress.PATH_COUNTS.items() if v != before.get(k, 0)}
    return out.detach(), leaf.grad, {k: p.grad.detach().clone() for k, p in stack.named_parameters()}, moved


def _group_errs(dx, grads, ref_dx, ref_grads):
    """max-abs relative error against float64 of dx, the conv parameters and the encoder parameters."""
    e = {"dx": stack_ref.err(dx, ref_dx), "conv": 0.0, "encoder": 0.0}
    for k, g in grads.items():
        grp = "conv" if k.startswith("conv") else "encoder"
        e[grp] = max(e[grp], stack_ref.err(g, ref_grads[k]))
    return e


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("case", list(CASES))
def test_stack_native_half_compress(cuda_device, key, case):
    """fp32 parameters, T features.  The native route outside autocast (where the earlier route raises on
    mixed dtypes) and inside it: dtypes, the route counters, the output within 2 layers u_T (max-abs
    relative) of the fp32 stack on the widened input — the existing autocast test's bar, per layer — and
    the gradients against float64 no worse than 1.5 x the earlier route's under autocast (the two routes
    round different intermediates, so equal-quality results scatter).  Errors per (dtype, case), max-abs
    relative against float64, are printed: native outside / inside autocast, then the torch route."""
    T, dev = hc.DTYPES[key], cuda_device
    ns, knn, layers = CASES[case]
    g, x, G = _frames(ns, knn, seed=21 + layers)
    gd = g.to(dev)
    torch.manual_seed(5)
    stack = m.GCNStack(types.SimpleNamespace(feature_dim=C, gcn_layers=layers, gcn_combine="cat_compress")).to(dev)
    xT, GT = x.to(T), G.to(T)
    params = {k: v.detach().cpu() for k, v in stack.named_parameters()}
    src, dst = (t.long() for t in g.edges())
    _, ref_dx, ref_grads = stack_ref.run(params, xT, g.edata["pose"].double(), src, dst, GT, torch.float64,
                                         layers=layers, combine="cat_compress")
    with torch.no_grad():
        ref32 = stack(gd, xT.float().to(dev)).cpu().numpy()

    assert compress.half_compress() == "native"
    native = {}
    for autocast in (False, True):
        out, dx, grads, moved = _run(stack, gd, xT, GT, dev, autocast)
        assert out.dtype == T and dx.dtype == T
        for k, gr in grads.items():
            assert gr.dtype == torch.float32 and bool(torch.isfinite(gr).all()), k
        assert moved == {"fwd_" + key: layers, "dgrad_" + key: layers, "wgrad_" + key: layers}, moved
        e = rel_err(out.float().cpu().numpy(), ref32)
        print(key, case, "autocast" if autocast else "plain", "out rel_err", e, "bar", 2 * layers * hc.UNIT[T])
        assert e <= 2 * layers * hc.UNIT[T]
        native[autocast] = _group_errs(dx, grads, ref_dx, ref_grads)

    prev = compress.set_half_compress("torch")
    try:
        assert prev == "native"
        out, dx, grads, moved = _run(stack, gd, xT, GT, dev, True)
        assert out.dtype == T and moved == {"torch_16": layers}, moved
        torch_route = _group_errs(dx, grads, ref_dx, ref_grads)
    finally:
        assert compress.set_half_compress(prev) == "torch"
    for grp in GROUPS:
        print(key, case, grp, "err native plain / autocast / torch route:", native[False][grp], native[True][grp],
              torch_route[grp])
    for autocast in (False, True):
        for grp in GROUPS:
            assert native[autocast][grp] <= 1.5 * torch_route[grp], (grp, autocast, native[autocast], torch_route)


def test_set_half_compress_validates():
    with pytest.raises(ValueError):
        compress.set_half_compress("library")
    assert compress.half_compress() == "native"


def test_conv_stored_in_16_bits_keeps_the_torch_route(cuda_device):
    """A module cast with ``.to(bfloat16)`` (weights stored in T) is out of the native route's scope."""
    dev = cuda_device
    g, x, _ = _frames((5, 5), None, seed=3)
    stack = m.GCNStack(types.SimpleNamespace(feature_dim=C, gcn_layers=1, gcn_combine="cat_compress")).to(dev)
    stack.conv1.to(torch.bfloat16)
    before = dict(compress.PATH_COUNTS)
    with torch.no_grad():
        out = stack(g.to(dev), x.to(torch.bfloat16).to(dev))
    assert out.dtype == torch.bfloat16
    assert compress.PATH_COUNTS["torch_16"] == before.get("torch_16", 0) + 1
    assert compress.PATH_COUNTS["fwd_bf16"] == before.get("fwd_bf16", 0)


def test_capture_and_replay_native_layer(cuda_device):
    """A stream capture of one no-grad native bf16 layer (aggregation + compress; gamma/beta given, so the
    encoder stays outside the captured region and the graph has one branch), replayed once, equals the
    eager bits."""
    dev = cuda_device
    T = torch.bfloat16
    g, x, _ = _frames((5, 5), None, seed=9)
    csr = g.csr(dev)
    gen = torch.Generator().manual_seed(9)
    gb = torch.sigmoid(torch.randn(g.num_edges(), C, 2, generator=gen)).to(dev)
    torch.manual_seed(9)
    conv = torch.nn.Conv2d(2 * C, C, kernel_size=1).to(dev)
    x = x.to(T).to(dev)
    assert compress.film_compress_supported(conv, x)
    with torch.no_grad():
        eager = compress.film_compress(conv, x, gb, csr, _lib.MODE_FILM_MEAN)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            compress.film_compress(conv, x, gb, csr, _lib.MODE_FILM_MEAN)  # warm the allocator and the weight image
            torch.cuda.current_stream().synchronize()
            with torch.cuda.graph(graph, stream=side):
                out = compress.film_compress(conv, x, gb, csr, _lib.MODE_FILM_MEAN)
    out.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert out.dtype == T and eager.dtype == T and torch.equal(hc.bits(out), hc.bits(eager))
