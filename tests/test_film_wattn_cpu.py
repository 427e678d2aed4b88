"""The confidence-gated attention fusion's reference (tests/wattn_cases.py) checked against itself, without a
GPU: the header's backward formulas against float64 autograd, the two reductions to film_attn, the room the
suite's bar leaves an fp32 evaluation, and three defects that bar sees."""
import numpy as np
import pytest
import torch

import attn_cases as ac
import wattn_cases as wc
from conftest import rel_err

TOL = 1e-5  # the bar of tests/test_gpu_film_wattn.py

GRAPHS = {"complete5": lambda: wc.complete(5), "knn16_4": lambda: wc.knn(16, 4), "ragged_simple": wc.ragged_simple,
          "general_csr": wc.general_csr, "loud_csr": wc.loud_csr}
NAMES = ("out", "attn", "rate", "dx", "dgb", "dw")


def _errs(g, got, ref, louds):
    """rel_err per output (the suite's normalisation), the loud nodes' own rate and dw left out."""
    got, ref = list(got), list(ref)
    for t in (got, ref):
        t[2], t[5] = wc.drop_loud(g, t[2], t[5], louds)
    return {k: rel_err(a.double().numpy(), b.double().numpy()) for k, a, b in zip(NAMES, got, ref)}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_manual_backward_equals_autograd(name):
    g = GRAPHS[name]()
    x, gb, _, G, _, w, louds = wc.random_operands(g, 5, 4, 4, seed=3)
    ref = wc.reference(g, x, gb, w, G, loud=louds)
    got = wc.formulas(g, x, gb, w, G)
    assert louds or name not in ("ragged_simple", "loud_csr")  # those two have a loud node
    # float64 both: the formulas are the derivative, not an approximation of it
    for k, e in _errs(g, got, ref, louds).items():
        assert e <= 1e-12, (k, e)
    dx, dgb, dw = wc.manual_backward(g, x, gb, w, G)
    assert torch.equal(dx, got[3]) and torch.equal(dgb, got[4])
    # the operands have what the kernels must survive: exact zeros, a pixel nobody delivers to, a silent node
    N = g.num_nodes()
    assert bool((w == 0).any()) and bool((w.view(N, -1) == 0).all(0).any()) and bool((w.view(N, -1) == 0).all(1).any())
    nz = w[w != 0]
    assert 0.25 <= float(nz.min()) and float(nz.max()) <= 1.0 and 0.2 < float((w == 0).float().mean()) < 0.55
    # grad_w at silent entries is part of the derivative: in general not zero
    silent_dw = ref[5][(w == 0) & torch.as_tensor(np.isin(np.arange(N), np.unique(wc.rows(g)[1])))[:, None, None]]
    assert bool((silent_dw != 0).any())


@pytest.mark.parametrize("name", ["complete5", "knn16_4", "general_csr"])
def test_unit_weights_reproduce_film_attn(name):
    g = GRAPHS[name]()
    x, gb, z, G, base, _, _ = wc.random_operands(g, 6, 4, 4, seed=2, loud=False)
    ones = torch.ones(g.num_nodes(), 4, 4)
    for logits, p in ((False, gb), (True, z)):
        out, attn, rate, dx, dgb, _ = wc.reference(g, x, p, ones, G, base=base, logits=logits)
        r = ac.reference(g, x, p, G, base=base, logits=logits, dtype=torch.float64)
        for a, b in zip((out, attn, dx, dgb), r):
            assert rel_err(a.numpy(), b.numpy()) <= 1e-13
        assert rel_err(rate.numpy(), attn.numpy()) <= 1e-13


@pytest.mark.parametrize("name", ["complete5", "knn16_4", "general_csr"])
def test_node_mask_reproduces_film_attn_on_the_compacted_graph(name):
    g = GRAPHS[name]()
    N = g.num_nodes()
    x, gb, _, G, base, _, _ = wc.random_operands(g, 6, 4, 4, seed=4, loud=False)
    silent = torch.zeros(N, dtype=torch.bool)
    silent[[1, N - 2]] = True
    w = (~silent).double()[:, None, None].expand(N, 4, 4)
    out, attn, _, dx, dgb, _ = wc.reference(g, x, gb, w, G, base=base)
    gc = wc.compacted(g, silent.numpy())
    assert gc.num_edges() == g.num_edges() and int(gc.in_degrees().sum()) < int(g.in_degrees().sum())
    r = ac.reference(gc, x, gb, G, base=base, dtype=torch.float64)
    for a, b in zip((out, attn, dx, dgb), r):
        assert rel_err(a.numpy(), b.numpy()) <= 1e-13
    src = np.asarray(g.edges()[0])
    removed = torch.as_tensor(silent.numpy()[src])
    assert bool((attn[removed] == 0).all()) and bool((dgb[removed] == 0).all())
    assert bool((r[1][removed] == 0).all()) and bool((r[3][removed] == 0).all())


CASES = [("ragged_simple", (17, 8, 8)), ("loud_csr", (3, 7, 7)), ("loud_csr", (8, 8, 8))]


@pytest.fixture(scope="module")
def fp32_cases():
    """Operands, the float64 reference and the fp32 restatement's errors, once per case."""
    res = {}
    for name, shape in CASES:
        g = GRAPHS[name]()
        ops = wc.random_operands(g, *shape, seed=len(name) + shape[0])
        x, gb, _, G, _, w, louds = ops
        assert louds
        ref = wc.reference(g, x, gb, w, G, loud=louds)
        errs = _errs(g, wc.formulas(g, x, gb, w, G, dtype=torch.float32), ref, louds)
        res[name, shape] = g, ops, ref, errs
    return res


def test_fp32_restatement_sits_under_the_bar(fp32_cases):
    """The header's formulas evaluated in fp32 (torch's summation orders, not a kernel's) against float64, on
    graphs with a loud sender: the largest error over out, attn, rate, dx, dgb, dw (the loud node's own rate and
    dw left out: infinities and NaNs by the header) must leave the bar a factor of at least 4.

    Measured: 2.9e-7 (ragged_simple 17x8x8), 1.3e-7 (loud_csr 3x7x7), 1.7e-7 (loud_csr 8x8x8): margins 35, 78
    and 60."""
    for key, (g, ops, ref, errs) in fp32_cases.items():
        worst = max(errs.values())
        print(key, errs, "margin", TOL / worst)
        assert np.isfinite(worst) and worst * 4 <= TOL, (key, errs)


@pytest.mark.parametrize("defect,where", [("max_over_all", ("out", "attn")), ("zero_silent_dw", ("dw",)),
                                          ("dbar_all", ("dx", "dgb"))])
def test_the_bar_sees_the_defects(fp32_cases, defect, where):
    """Each defect, in the same fp32 evaluation on the same operands, exceeds the bar.  The first and the third
    change nothing in exact arithmetic; it is the loud silent sender whose scores (+inf in fp32) and da (inf or
    NaN) they let in: a max over all entries underflows every delivered term, and 0 * da is NaN."""
    for key, (g, ops, ref, errs) in fp32_cases.items():
        x, gb, _, G, _, w, louds = ops
        bad = _errs(g, wc.formulas(g, x, gb, w, G, dtype=torch.float32, **{defect: True}), ref, louds)
        print(key, defect, bad)
        assert any(not bad[k] <= TOL for k in where), (key, defect, bad)
