"""GPU: the matrix-core backward (``film_bwd_mfma``) on bf16 / fp16 feature maps, graphs of 9..16 nodes.

Contract: every loaded element is widened exactly to fp32, both products run the fp32
kernel's ``v_mfma_f32_16x16x4_f32`` sequence on the fp32 kernel's pixel layout, and each ``grad_x`` element
is rounded once (to nearest even) at the store.  So, at knob ``bwd_half_mfma = 1``,

* ``grad_x`` is bit-equal to the fp32 path's ``grad_x`` on the widened inputs, cast to T;
* ``grad_gb`` (fp32) is bit-equal to the fp32 path's;
* both are also held to the float64 oracle with the bars of ``half_cases`` — at knob 0 (``film_bwd_dx`` +
  the Gram pass, the route of every shape the kernel does not take) as well.

Every test that selects a route sets the knob, which the library rejects before the kernel existed.

Cases (the smallest shapes at which the kernel can still go wrong):

  m1  complete [9]       C 1, 8x8    smallest graph, one channel in an 8-channel workgroup (idle waves),
                                      one pixel group, 7 padded rows
  m2  complete [16, 16]  C 9, 8x16   full 16 rows, ragged second channel block, 2 groups (both register sets)
  m3  k-NN(4) [16, 12]   C 8, 16x16  REGULAR, KMAX 4, graphs of different n in one batch, 4 groups
  m4  k-NN(6) [10]       C 5, 8x24   KMAX 8 with K = 6, 3 groups (the pipeline's tail)
  m5  as m2, x / grad_out / the base as channel slices of wider tensors (node stride != C P)
  m6  as m3, operands 4 elements into a flat buffer (8- but not 16-byte aligned: still the kernel) and
      1 element in (2-byte aligned: the old route)
"""
import functools
import types

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import aggregate
import half_cases as hc
import oracle
import stack_ref
from conftest import rel_err

pytestmark = pytest.mark.gpu

KEYS = list(hc.DTYPES)
KNOBS = (0, 1)   # every accepted value of bwd_half_mfma
FORMS = (1,)     # the non-zero ones: the matrix-core kernel on 64-pixel groups
OPS = ["film_mean", "cat", "residual"]

#: name -> (node counts, k of k-NN or None, C, H, W)
CASES = {
    "m1": ((9,), None, 1, 8, 8),
    "m2": ((16, 16), None, 9, 8, 16),
    "m3": ((16, 12), 4, 8, 16, 16),
    "m4": ((10,), 6, 5, 8, 24),
}
#: embedding -> (case, how the operands are laid out)
EMBED = {"m1": ("m1", None), "m2": ("m2", None), "m3": ("m3", None), "m4": ("m4", None),
         "m5": ("m2", "slice"), "m6_4": ("m3", 4), "m6_1": ("m3", 1)}
BIT_CASES = ["m1", "m2", "m3", "m4", "m5", "m6_4"]  # m6_4: 8-byte alignment still reaches the kernel


@functools.lru_cache(maxsize=None)
def graph(case):
    ns, knn, _, _, _ = CASES[case]
    return hc._frames(list(ns), 40 + int(case[1:]), knn=knn)


@functools.lru_cache(maxsize=None)
def host_inputs(case, key):
    """(x, gb, z, G, G0) on the CPU, drawn as ``half_cases.host_inputs`` draws them: x, the incoming gradient
    G and the grad_x base G0 in fp32 rounded to T, logits z with gb == sigmoid(z) to fp32 rounding."""
    T = hc.DTYPES[key]
    g = graph(case)
    _, _, C, H, W = CASES[case]
    gen = torch.Generator().manual_seed(sum(map(ord, case)) * 131 + (0 if key == "bf16" else 1))
    x = torch.randn(g.num_nodes(), C, H, W, generator=gen).to(T)
    G = torch.randn(g.num_nodes(), C, H, W, generator=gen).to(T)
    z = torch.randn(g.num_edges(), C, 2, generator=gen)
    G0 = torch.randn(g.num_nodes(), C, H, W, generator=gen).to(T)
    return x, torch.sigmoid(z), z, G, G0


@functools.lru_cache(maxsize=None)
def oracle_ref(case, key):
    """Float64 and float32 oracle gradients of film_mean on the widened inputs (computed once)."""
    x, gb, _, G, _ = host_inputs(case, key)
    src, dst = (t.numpy() for t in graph(case).edges())
    ref = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        ref["dx" + tag], ref["dgb" + tag] = oracle.film_aggregate_grads(x.to(dt), gb.to(dt), src, dst, G.to(dt))
    return ref


def place(t, how):
    """A tensor holding t's values laid out as the embedding asks: a channel slice of a wider tensor, or a
    view `how` elements into a flat buffer."""
    if how is None:
        return t.clone()
    n, C, H, W = t.shape
    if how == "slice":
        wide = torch.zeros(n, C + 3, H, W, dtype=t.dtype, device=t.device)
        wide[:, 2:C + 2] = t
        return wide[:, 2:C + 2]
    flat = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    flat[how:how + t.numel()] = t.reshape(-1)
    return flat[how:how + t.numel()].view(n, C, H, W)


def backward(dev, emb, key, op, logits, dtype=None, need_dx=True, need_dgb=True):
    """(grad_x, grad_gb) of ``aggregate.film_mean_backward`` (the Python layer over ``mrp_film_mean_bwd_t``)
    for the op's epilogue; dtype=torch.float32 runs the fp32 path on the widened, contiguous inputs."""
    case, how = EMBED[emb]
    x, gb, z, G, G0 = (t.to(dev) for t in host_inputs(case, key))
    if dtype is not None:
        x, G, G0, how = x.to(dtype), G.to(dtype), G0.to(dtype), None
    csr = graph(case).csr(dev)
    mode = aggregate._mode_flags("film_mean", logits)
    base = place(G0, how) if op == "cat" and need_dx else None
    ep = aggregate.EpilogueSpec(1.0, 1.0) if op == "residual" else None
    k = "bwd_" + hc.KEY[x.dtype]
    before = aggregate.PATH_COUNTS[k]
    dx, dgb = aggregate.film_mean_backward(place(G, how), place(x, how), z if logits else gb, csr, mode, need_dx,
                                           need_dgb, grad_x_base=base, epilogue=ep)
    assert aggregate.PATH_COUNTS[k] == before + 1
    return dx, dgb


@functools.lru_cache(maxsize=None)
def fp32_path(dev, case, key, op, logits):
    """The fp32 library path (``film_bwd_mfma``) on the widened inputs: computed once, never modified."""
    return backward(dev, case, key, op, logits, dtype=torch.float32)


class knob:
    """``with knob(v):`` sets bwd_half_mfma and restores every default on the way out."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        assert m.load_library().mrp_tuning_set(b"bwd_half_mfma", self.v) == 0, "bwd_half_mfma is unknown"

    def __exit__(self, *exc):
        assert m.load_library().mrp_tuning_set(b"reset", 0) == 0


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("emb", BIT_CASES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", KEYS)
def test_grad_x_bit_equal_to_fp32_path(cuda_device, key, form, emb, op, logits):
    T = hc.DTYPES[key]
    with knob(form):
        dx, dgb = backward(cuda_device, emb, key, op, logits)
    assert dx.dtype == T and dgb.dtype == torch.float32
    dx32, _ = fp32_path(cuda_device, EMBED[emb][0], key, op, logits)
    assert dx32.dtype == torch.float32
    assert torch.equal(hc.bits(dx), hc.bits(dx32.to(T)))


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("key", KEYS)
def test_grad_gb_bit_equal_to_fp32_path(cuda_device, key, case, op, logits):
    """The 64-pixel-group form sums the Gram in the fp32 kernel's order: the same bits."""
    with knob(1):
        _, dgb = backward(cuda_device, case, key, op, logits)
    _, dgb32 = fp32_path(cuda_device, case, key, op, logits)
    assert torch.equal(hc.bits(dgb), hc.bits(dgb32))


@pytest.mark.parametrize("emb", list(EMBED))
@pytest.mark.parametrize("value", KNOBS)
@pytest.mark.parametrize("key", KEYS)
def test_gradients_against_float64(cuda_device, key, value, emb):
    """Both routes, every case and layout (for m6's 1-element view this is the only check)."""
    T = hc.DTYPES[key]
    case = EMBED[emb][0]
    with knob(value):
        dx, dgb = backward(cuda_device, emb, key, "film_mean", False)
    ref = oracle_ref(case, key)
    print(emb, key, value, "dgb rel_err", rel_err(dgb.cpu().numpy(), ref["dgb64"].numpy()),
          "fp32 oracle", rel_err(ref["dgb32"].numpy(), ref["dgb64"].numpy()))
    hc.assert_relative(dgb, ref["dgb32"], ref["dgb64"], (emb, key, value, "dgb"))
    assert dx.dtype == T
    hc.assert_elementwise(dx, ref["dx64"], T, (emb, key, value, "dx"))


@pytest.mark.parametrize("op", ["cat", "residual"])
@pytest.mark.parametrize("key", KEYS)
def test_epilogues_against_float64(cuda_device, key, op):
    """The grad_x base (cat) and the self term (residual) of m2, against float64: d(x + a(x)) = G + dx,
    d cat = G0 + dx."""
    T = hc.DTYPES[key]
    with knob(1):
        dx, dgb = backward(cuda_device, "m2", key, op, False)
    ref = oracle_ref("m2", key)
    _, _, _, G, G0 = host_inputs("m2", key)
    hc.assert_elementwise(dx, ref["dx64"] + (G0 if op == "cat" else G).double(), T, (key, op, "dx"))
    hc.assert_relative(dgb, ref["dgb32"], ref["dgb64"], (key, op, "dgb"))


@pytest.mark.parametrize("value", KNOBS)
@pytest.mark.parametrize("case", ["m1", "m3"])
@pytest.mark.parametrize("key", KEYS)
def test_single_gradients(cuda_device, key, case, value):
    """Only grad_x wanted / only grad_gb wanted: the absent output is not allocated (a write to it would be
    a write through a null pointer), the present one has the bits of the run that wants both."""
    with knob(value):
        dx, dgb = backward(cuda_device, case, key, "film_mean", True)
        dx_only, none_gb = backward(cuda_device, case, key, "film_mean", True, need_dgb=False)
        none_dx, dgb_only = backward(cuda_device, case, key, "film_mean", True, need_dx=False)
    assert none_gb is None and none_dx is None
    assert torch.equal(hc.bits(dx_only), hc.bits(dx))
    assert torch.equal(hc.bits(dgb_only), hc.bits(dgb))


@pytest.mark.parametrize("key", KEYS)
def test_two_runs_give_identical_bits(cuda_device, key):
    with knob(1):
        a = backward(cuda_device, "m3", key, "residual", True)
        b = backward(cuda_device, "m3", key, "residual", True)
    assert torch.equal(hc.bits(a[0]), hc.bits(b[0])) and torch.equal(hc.bits(a[1]), hc.bits(b[1]))


@pytest.mark.parametrize("key", KEYS)
def test_default_is_the_matrix_core_kernel(cuda_device, key):
    """Default knobs and after "reset": the bits of knob 1, grad_gb included (the old route sums the Gram
    in another order; were the default 0, m3's 1792 fp32 sums would all have to agree by accident).
    bwd_regular_mfma = 0 sends 16-bit features down the old route as it does fp32 ones: still correct."""
    lib = m.load_library()
    with knob(1):
        want = backward(cuda_device, "m3", key, "film_mean", False)
    got = backward(cuda_device, "m3", key, "film_mean", False)
    assert torch.equal(hc.bits(got[0]), hc.bits(want[0])) and torch.equal(hc.bits(got[1]), hc.bits(want[1]))
    try:
        assert lib.mrp_tuning_set(b"bwd_regular_mfma", 0) == 0
        dx, dgb = backward(cuda_device, "m3", key, "film_mean", False)
    finally:
        assert lib.mrp_tuning_set(b"reset", 0) == 0
    ref = oracle_ref("m3", key)
    hc.assert_elementwise(dx, ref["dx64"], hc.DTYPES[key], (key, "dx, bwd_regular_mfma 0"))
    hc.assert_relative(dgb, ref["dgb32"], ref["dgb64"], (key, "dgb, bwd_regular_mfma 0"))


@pytest.mark.parametrize("op", ["film_mean", "cat", "residual", "mix"])
@pytest.mark.parametrize("key", KEYS)
def test_autograd_functions_reach_the_kernel(cuda_device, key, op):
    """``FilmMeanFunction`` / ``FilmMeanCatFunction`` on m2 (16 nodes) at default knobs: the gradients autograd
    returns are those of the direct call (mix: agg_scale 0.7 enters the weights, so float64 holds it)."""
    T = hc.DTYPES[key]
    dev = cuda_device
    x, gb, z, G, G0 = (t.to(dev) for t in host_inputs("m2", key))
    csr = graph("m2").csr(dev)
    leaf = x.clone().requires_grad_(True)
    zl = z.clone().requires_grad_(True)
    before = aggregate.PATH_COUNTS["bwd_" + key]
    if op == "cat":
        m.film_mean_cat(leaf, zl, csr, logits=True).backward(torch.cat((G0, G), 1))
    elif op == "residual":
        m.film_mean_residual(leaf, zl, csr, logits=True).backward(G)
    elif op == "mix":
        m.film_mean_mix(leaf, zl, csr, G0, 0.3, logits=True).backward(G)
    else:
        m.film_mean(leaf, zl, csr, logits=True).backward(G)
    assert aggregate.PATH_COUNTS["bwd_" + key] == before + 1
    assert leaf.grad.dtype == T and zl.grad.dtype == torch.float32
    if op == "mix":
        ref = oracle_ref("m2", key)
        hc.assert_elementwise(leaf.grad, 0.7 * ref["dx64"], T, (key, "mix dx"))
        return
    with knob(1):
        dx, dgb = backward(dev, "m2", key, op, True)
    assert torch.equal(hc.bits(leaf.grad), hc.bits(dx))
    assert torch.equal(hc.bits(zl.grad), hc.bits(dgb.view(zl.shape)))


def test_stack_residual_two_layers_12_nodes(cuda_device):
    """Model level, default knobs: a two-layer residual ``GCNStack`` on bf16 features, two complete 12-node
    frames, C = 8, 8x8, forward + backward, against the float64 restatement of the stack (``stack_ref``) on
    the widened input, backpropagating the gradient the kernels received (2 out, exact in bf16).

    Bar: ``2 u_T`` max-abs relative, ``test_gpu_half_model.test_stack_residual_two_layers``'s: gamma / beta
    depend on the poses alone, so the only differences from float64 beyond fp32 rounding are the single
    rounding to T of each stored feature map, and at most two of those lie on the path to any compared
    quantity (out: h1 and out; grad_x: grad_h1 and grad_x; layer-2 parameters: h1; layer-1: grad_h1)."""
    T, key = torch.bfloat16, "bf16"
    dev = cuda_device
    C, HW = 8, 8
    rng = np.random.RandomState(21)
    g = m.batch([m.frame_graph(hc._poses(rng, 12)) for _ in range(2)])
    x = torch.randn(g.num_nodes(), C, HW, HW, generator=torch.Generator().manual_seed(21)).to(T)
    torch.manual_seed(5)
    stack = m.GCNStack(types.SimpleNamespace(feature_dim=C, gcn_layers=2, gcn_combine="residual")).to(dev)
    params = {k: v.detach().cpu().clone() for k, v in stack.named_parameters()}
    gd = g.to(dev)
    leaf = x.to(dev).requires_grad_(True)
    before = aggregate.PATH_COUNTS["fwd_" + key], aggregate.PATH_COUNTS["bwd_" + key]
    out = stack(gd, leaf)
    out.float().square().sum().backward()
    assert out.dtype == T and leaf.grad.dtype == T
    assert aggregate.PATH_COUNTS["fwd_" + key] == before[0] + 2
    assert aggregate.PATH_COUNTS["bwd_" + key] == before[1] + 2
    src, dst = g.edges()
    ref = stack_ref.run(params, x, g.edata["pose"], src.long(), dst.long(), 2.0 * out.detach().cpu(), torch.float64,
                        layers=2, combine="residual")
    bar = 2 * hc.UNIT[T]
    e_out, e_dx = stack_ref.err(out, ref[0]), stack_ref.err(leaf.grad, ref[1])
    print("stack 12 nodes: out", e_out, "dx", e_dx, "bar", bar)
    assert e_out <= bar and e_dx <= bar
    for k, p in stack.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32
        e = stack_ref.err(p.grad, ref[2][k])
        print("stack 12 nodes:", k, e)
        assert e <= bar, (k, e)
