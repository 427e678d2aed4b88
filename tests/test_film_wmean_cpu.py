"""The confidence-weighted aggregation's reference (tests/wmean_cases.py), checked without a GPU on the GPU
tests' own operands: the manual backward against autograd, the float32 restatement against float64 and the
bars, w == 1 against the oracle, the weight generator, and that each dropped term moves the result far beyond
the bars the GPU tests apply."""
import numpy as np
import pytest
import torch

import half_cases as hc
import oracle
import stack_ref
import wmean_cases as wc
from conftest import rel_err

CASES = list(hc.CASES)
SMALL = ["c", "d", "g", "b"]


def _e(a, b):
    return rel_err(a.detach().numpy(), b.detach().numpy())


@pytest.mark.parametrize("name", CASES)
def test_weight_generator(name):
    w = wc.weights(name)
    n, _, H, W = hc.shape(name)
    assert w.shape == (n, H, W) and w.dtype == torch.float32 and w.is_contiguous()
    nz = w[w != 0]
    assert float(nz.min()) >= 1.0 / 16 and float(nz.max()) <= 1.0
    assert 0.2 <= float((w == 0).float().mean()) < 0.5
    # every destination has pixels at which all of its senders are silent, and pixels with some delivery
    indptr, src, _ = wc.rows(hc.graph(name))
    for v in range(n):
        u = src[indptr[v]:indptr[v + 1]]
        if len(u):
            D = w[torch.as_tensor(u.astype(np.int64))].sum(0)
            assert bool((D == 0).any()) and bool((D > 0).any())
    assert torch.equal(w, wc.weights(name))  # deterministic


@pytest.mark.parametrize("mode", ["mean", "sum"])
@pytest.mark.parametrize("name", CASES)
def test_manual_backward_is_autograd_in_float64(name, mode):
    x, gb, _, G, w = wc.inputs(name, "f32")
    g = hc.graph(name)
    args = (x.double(), gb.double(), w.double(), G.double())
    man = wc.backward(g, *args, mode=mode)
    ag = wc.autograd(g, *args, mode=mode)
    for a, b, what in zip(man, ag, ("out", "dx", "dgb", "dw")):
        assert _e(a, b) <= 1e-13, (what, _e(a, b))


@pytest.mark.parametrize("key", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", CASES)
def test_float32_restatement_is_within_the_bars(name, key):
    """The fp32 restatement itself meets the fp32 bars on these operands (so the weights' range keeps the
    float64 comparison a test of the arithmetic, not of cancellation)."""
    for mode in ("mean", "sum"):
        r = wc.reference(name, key, mode)
        for what in ("out", "dx"):
            assert _e(r[what + "32"], r[what + "64"]) <= 1e-5, (what, mode)
        for what in ("dgb", "dw", "dz"):
            assert _e(r[what + "32"], r[what + "64"]) <= 1e-5, (what, mode)
        # pixels nobody delivered to: exact zeros in out and in their gradient contributions
        if mode == "mean":
            assert bool((r["out64"][:, :, 0, 0] == 0).all())
            assert bool((r["dw64"][:, 0, 0] == 0).all()) and bool((r["dx64"][:, :, 0, 0] == 0).all())


@pytest.mark.parametrize("name", CASES)
def test_unit_weights_give_the_oracle_aggregate(name):
    x, gb, _, _, w = wc.inputs(name, "f32")
    g = hc.graph(name)
    src, dst = (t.numpy() for t in g.edges())
    one = torch.ones_like(w).double()
    for mode, omode in (("mean", "film_mean"), ("sum", "film_sum")):
        ours = wc.forward(g, x.double(), gb.double(), one, mode)
        ref = oracle.film_aggregate(x.double(), gb.double(), src, dst, omode)
        assert torch.equal(ours, ref), (mode, float((ours - ref).abs().max()))


@pytest.mark.parametrize("name", SMALL)
def test_each_dropped_term_is_far_beyond_the_bar(name):
    x, gb, _, G, w = wc.inputs(name, "f32")
    g = hc.graph(name)
    args = (x.double(), gb.double(), w.double(), G.double())
    out, dx, dgb, dw = wc.backward(g, *args)
    bar = 1e-5
    o2 = wc.forward(g, *args[:3], drop="w_on_beta")
    assert _e(o2, out) > 1e3 * bar
    o3, dx3, dgb3, dw3 = wc.backward(g, *args, drop="degree_D")
    assert _e(o3, out) > 1e3 * bar and _e(dx3, dx) > 1e3 * bar and _e(dgb3, dgb) > 1e3 * bar
    assert _e(wc.backward(g, *args, drop="out_term")[3], dw) > 1e3 * bar
    assert _e(wc.backward(g, *args, drop="w_in_dx")[1], dx) > 1e3 * bar


def test_stack_ref_bar_accepts_the_restatement():
    r = wc.reference("g", "f32")
    ok, _ = stack_ref.within(r["dw32"], r["dw32"], r["dw64"])
    assert ok
