"""The attention-pooled FiLM aggregation's yardstick, checked without a GPU.

These tests run no kernel and no code of the package beyond its graph builders: they exercise only the torch
restatement in tests/attn_cases.py, so they pass with or without the operator.  Their purpose is to calibrate
the reference and the bar that tests/test_gpu_film_attn.py holds the kernels to: the float64 restatement agrees
with the header's backward formulas, an fp32 evaluation with another summation order stays well inside the
tolerance, and the tolerance sees each path of the backward when it is dropped."""
import pytest
import torch

import attn_cases as ac

TOL = 1e-5  # the suite's bar, the one tests/test_gpu_film_attn.py holds the kernels to

SHAPES = [(5, 4, 8, 8), (8, 17, 8, 8), (16, 40, 4, 4)]  # (nodes, C, H, W)


def rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def cases():
    """Per shape: the graph, the GPU tests' random operands and the float64 reference, computed once."""
    res = {}
    for n, C, H, W in SHAPES:
        g = ac.complete(n, B=1)
        x, gb, _, G, _ = ac.random_operands(g, C, H, W, seed=n)
        res[(n, C, H, W)] = (g, x, gb, G, ac.reference(g, x, gb, G, dtype=torch.float64))
    return res


@pytest.mark.parametrize("shape", SHAPES)
def test_manual_backward_equals_autograd(cases, shape):
    g, x, gb, G, (_, _, dx, dgb) = cases[shape]
    mdx, mdgb = ac.manual_backward(g, x, gb, G)
    assert rel(mdx, dx) <= 1e-13 and rel(mdgb, dgb) <= 1e-13


@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_restatement_is_within_tol_of_float64(cases, shape):
    g, x, gb, G, (out, attn, dx, dgb) = cases[shape]
    out32, attn32, dx32, dgb32 = ac.reference(g, x, gb, G)
    errs = [rel(out32, out), rel(attn32, attn), rel(dx32, dx), rel(dgb32, dgb)]
    c_out, c_dx, c_dgb = ac.chunked_reference(g, x, gb, G)
    errs += [rel(c_out, out), rel(c_dx, dx), rel(c_dgb, dgb)]
    print(shape, errs)
    assert max(errs) <= TOL


def test_fp32_restatement_within_tol_on_general_graphs_and_logits():
    for g in (ac.general_csr(), ac.masked_small(), ac.knn(9, 8)):
        x, _, z, G, base = ac.random_operands(g, 17, 8, 8, seed=3)
        r64 = ac.reference(g, x, z, G, base=base, logits=True, dtype=torch.float64)
        r32 = ac.reference(g, x, z, G, base=base, logits=True)
        for a, b in zip(r32, r64):
            assert rel(a, b) <= TOL
        # weights of a row sum to one; rows no entry names stay zero
        indptr, _, eid = ac.rows(g)
        named = torch.zeros(g.num_edges(), dtype=torch.bool)
        named[torch.as_tensor(eid[: int(indptr[-1])].astype("int64"))] = True
        assert bool((r64[1][~named] == 0).all())
        for v in range(g.num_nodes()):
            lo, hi = int(indptr[v]), int(indptr[v + 1])
            if hi > lo:
                tot = r64[1][torch.as_tensor(eid[lo:hi].astype("int64"))].sum(0)
                assert float((tot - 1).abs().max()) <= 1e-12


DEFECTS = [dict(key_path=False), dict(query_path=False), dict(subtract=False), dict(use_scale=False)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("defect", DEFECTS, ids=lambda d: next(iter(d)))
def test_each_defect_is_far_outside_tol(cases, shape, defect):
    g, x, gb, G, (_, _, dx, dgb) = cases[shape]
    bdx, bdgb = ac.manual_backward(g, x, gb, G, **defect)
    moved = max(rel(bdx, dx), rel(bdgb, dgb))
    print(shape, defect, moved)
    assert moved > 100 * TOL


def test_in_degree_one_and_zero_scale_anchors():
    """The exact anchors the GPU test uses, on the reference: with one entry the weight is 1 and the score
    paths vanish; with scale 0 the weights are 1/d and the output is the mean of the messages."""
    g = ac.knn(12, 1)
    x, gb, G, _ = ac.lattice_operands(g, 3, 4, 4, seed=0)
    out, attn, dx, dgb = ac.reference(g, x, gb, G, dtype=torch.float64)
    assert bool((attn == 1).all())
    mdx, mdgb = ac.manual_backward(g, x, gb, G, key_path=False, query_path=False)
    assert torch.equal(mdx, dx) and torch.equal(mdgb, dgb)
    g = ac.complete(5)
    x, gb, _, G, _ = ac.random_operands(g, 4, 4, 4, seed=1)
    out, attn, _, _ = ac.reference(g, x, gb, G, dtype=torch.float64, scale=0.0)
    assert float((attn - 0.25).abs().max()) <= 1e-15
