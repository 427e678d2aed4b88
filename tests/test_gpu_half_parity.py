"""GPU: the FiLM-mean aggregation on bf16 / fp16 feature maps (``mrp_film_mean_fwd_t`` / ``_bwd_t``).

Contract: every loaded element is widened exactly to fp32, the arithmetic is the fp32 kernels' own, and
each output element is rounded once (to nearest even) at the store.  So

* forward: ``film_mean(x_T) == film_mean(x_T.float()).to(T)`` bit for bit, every case, mode and epilogue;
* ``grad_x`` for graphs of <= 8 nodes (fp32: ``film_bwd_fused``, whose per-element fma chain does not
  depend on the lane geometry): bit-equal to the fp32 path's ``grad_x`` on the widened inputs, cast;
* ``grad_gb`` (fp32, summed over the plane in a geometry-dependent order) and ``grad_x`` for 9-16-node
  graphs (another kernel than fp32's): held to the float64 oracle with the bars of ``half_cases``;
* the forward of every case is also held to float64, so a bug shared by both sides of a bit-equality
  cannot hide.

Cases: ``half_cases.CASES``.  Without the feature ``film_mean`` on a bf16 tensor raises ``TypeError``."""
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import aggregate
import half_cases as hc

pytestmark = pytest.mark.gpu

KEYS = list(hc.DTYPES)
ALL = list(hc.CASES)
OPS = ["film_sum", "copy_mean", "cat", "residual", "mix"]
ALPHA = 0.3


def _apply(op, x, gb, csr, logits, x0=None):
    if op == "cat":
        return m.film_mean_cat(x, gb, csr, logits=logits)
    if op == "residual":
        return m.film_mean_residual(x, gb, csr, logits=logits)
    if op == "mix":
        return m.film_mean_mix(x, gb, csr, x0, ALPHA, logits=logits)
    return m.film_mean(x, gb, csr, op, logits=logits)


def _inputs(name, key, dev, logits):
    x, gb, z, G = hc.host_inputs(name, key)
    return x.to(dev), (z if logits else gb).to(dev), G.to(dev)


def _x0(x):
    """The mix's second feature tensor, in x's dtype (values representable in it)."""
    gen = torch.Generator().manual_seed(99)
    return torch.randn(x.shape, generator=gen).to(x.dtype).to(x.device)


def _forward_pair(name, key, dev, op, logits):
    """(16-bit result on the case's embedded x, fp32 result on the widened contiguous x, x as handed in)."""
    T = hc.DTYPES[key]
    x, gb, _ = _inputs(name, key, dev, logits)
    csr = hc.graph(name).csr(dev)
    leaf, view = hc.embed(name, x)
    xv = view(leaf)
    x0 = _x0(x) if op == "mix" else None
    before = aggregate.PATH_COUNTS["fwd_" + key]
    with torch.no_grad():
        got = _apply(op, xv, gb, csr, logits, x0)
        assert aggregate.PATH_COUNTS["fwd_" + key] == before + 1
        ref = _apply(op, x.float(), gb, csr, logits, x0.float() if x0 is not None else None)
    assert got.dtype == T and ref.dtype == torch.float32
    return got, ref, x


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("key", KEYS)
def test_forward_bit_equal_to_fp32_path(cuda_device, key, name, logits):
    T = hc.DTYPES[key]
    got, ref, _ = _forward_pair(name, key, cuda_device, "film_mean", logits)
    assert torch.equal(hc.bits(got), hc.bits(ref.to(T)))
    # and against float64 (gb == sigmoid(z) up to fp32 rounding, far inside the bar)
    hc.assert_elementwise(got, hc.oracle_ref(name, key)["out64"], T, (name, key))


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("key", KEYS)
def test_forward_modes_and_epilogues_bit_equal(cuda_device, key, name, op):
    T = hc.DTYPES[key]
    got, ref, x = _forward_pair(name, key, cuda_device, op, True)
    assert torch.equal(hc.bits(got), hc.bits(ref.to(T)))
    if op == "cat":  # the first half is x's own bits
        C = x.shape[1]
        assert torch.equal(hc.bits(got[:, :C]), hc.bits(x))
    if op in ("film_sum", "copy_mean"):
        hc.assert_elementwise(got, hc.oracle_ref(name, key, op)["out64"], T, (name, key, op))


@pytest.mark.parametrize("key", KEYS)
def test_forward_into_cat_buffer_half(cuda_device, key):
    """Case h: x a channel slice of a wider tensor, out the second half of a concatenation buffer."""
    T = hc.DTYPES[key]
    dev = cuda_device
    x, gb, _ = _inputs("h", key, dev, False)
    csr = hc.graph("h").csr(dev)
    leaf, view = hc.embed("h", x)
    n, C, H, W = x.shape
    buf = torch.zeros(n, 2 * C, H, W, dtype=T, device=dev)
    aggregate.film_mean_forward_into(view(leaf), gb, csr, 0, buf[:, C:])
    ref = torch.empty(n, C, H, W, dtype=torch.float32, device=dev)
    aggregate.film_mean_forward_into(x.float(), gb, csr, 0, ref)
    assert torch.equal(hc.bits(buf[:, C:]), hc.bits(ref.to(T)))
    assert not buf[:, :C].any()  # the other half untouched


def _backward(op, leaf, view, gb, csr, G, logits, x0=None):
    leaf = leaf.detach().clone().requires_grad_(True)
    gb = gb.detach().clone().requires_grad_(True)
    out = _apply(op, view(leaf), gb, csr, logits, x0)
    out.backward(G.to(out.dtype))
    return view(leaf.grad), gb.grad, leaf.grad


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("op", ["film_mean", "cat", "residual"])
@pytest.mark.parametrize("name", hc.SMALL)
@pytest.mark.parametrize("key", KEYS)
def test_grad_x_bit_equal_to_fp32_path(cuda_device, key, name, op, logits):
    T = hc.DTYPES[key]
    dev = cuda_device
    x, gb, G = _inputs(name, key, dev, logits)
    csr = hc.graph(name).csr(dev)
    if op == "cat":  # the incoming gradient covers both halves: the first is grad_x's base
        G = torch.cat((G, _x0(x)), 1)
    leaf, view = hc.embed(name, x)
    before = aggregate.PATH_COUNTS["bwd_" + key]
    dx, dgb, leaf_grad = _backward(op, leaf, view, gb, csr, G, logits)
    assert aggregate.PATH_COUNTS["bwd_" + key] == before + 1
    assert dx.dtype == T and leaf_grad.dtype == T and dgb.dtype == torch.float32
    dx32, dgb32, _ = _backward(op, x.float(), lambda t: t, gb, csr, G.float(), logits)
    assert dx32.dtype == torch.float32
    assert torch.equal(hc.bits(dx), hc.bits(dx32.to(T)))
    # (grad_gb sums the same fp32 products in another order: held to float64 below)
    assert dgb.shape == dgb32.shape and bool(torch.isfinite(dgb).all())


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("key", KEYS)
def test_gradients_against_float64(cuda_device, key, name):
    """grad_gb (fp32) of every case within max(1e-5, 4 x the fp32 oracle's error); grad_x elementwise
    within one rounding of T (for the 9-16-node cases e and f this is their only grad_x check)."""
    T = hc.DTYPES[key]
    dev = cuda_device
    x, gb, G = _inputs(name, key, dev, False)
    leaf, view = hc.embed(name, x)
    dx, dgb, _ = _backward("film_mean", leaf, view, gb, hc.graph(name).csr(dev), G, False)
    ref = hc.oracle_ref(name, key)
    print(name, key, "dgb rel_err", hc.rel_err(dgb.cpu().numpy(), ref["dgb64"].numpy()),
          "fp32 oracle", hc.rel_err(ref["dgb32"].numpy(), ref["dgb64"].numpy()))
    hc.assert_relative(dgb, ref["dgb32"], ref["dgb64"], (name, key, "dgb"))
    assert dx.dtype == T
    hc.assert_elementwise(dx, ref["dx64"], T, (name, key, "dx"))


@pytest.mark.parametrize("key", KEYS)
def test_other_dtypes_and_devices_still_raise(cuda_device, key):
    dev = cuda_device
    x, gb, _ = _inputs("d", key, dev, False)
    csr = hc.graph("d").csr(dev)
    assert m.film_mean(x, gb, csr).dtype == hc.DTYPES[key]  # TypeError before 16-bit features existed
    with pytest.raises(TypeError):
        m.film_mean(x.double(), gb, csr)
    with pytest.raises(TypeError):
        m.film_mean(x.to(torch.int32), gb, csr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.film_mean(x.cpu(), gb.cpu(), hc.graph("d").csr("cpu"))


@pytest.mark.parametrize("key", KEYS)
def test_mixed_dtype_x0_and_grad_out_are_cast(cuda_device, key):
    """x0 and grad_out in another dtype than x are cast to x's (as fp32 already casts x0)."""
    T = hc.DTYPES[key]
    dev = cuda_device
    x, gb, G = _inputs("b", key, dev, False)
    csr = hc.graph("b").csr(dev)
    x0 = _x0(x)
    a = m.film_mean_mix(x, gb, csr, x0.float(), ALPHA)
    b = m.film_mean_mix(x, gb, csr, x0, ALPHA)
    assert a.dtype == T and torch.equal(hc.bits(a), hc.bits(b))
    xa = x.clone().requires_grad_(True)
    m.film_mean(xa, gb, csr).backward(G)
    xb = x.clone().requires_grad_(True)
    (m.film_mean(xb, gb, csr).float()).backward(G.float())  # autograd casts the fp32 gradient to T
    assert xa.grad.dtype == T and torch.equal(hc.bits(xa.grad), hc.bits(xb.grad))
