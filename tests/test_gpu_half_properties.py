"""GPU, property-based (hypothesis): the 16-bit aggregation on arbitrary batches of up to 16-node graphs
(any in-degree, multi-edges, self-loops, any edge order — ``graph_strategies.batches``), C <= 8, P <= 16,
against the float64 oracle on the widened inputs.  Forward and grad_x elementwise within one rounding of
T, grad_gb (fp32) within max(1e-5, 4 x the fp32 oracle's error) — the bars of ``half_cases``.  A small
fixed (derandomized) example set keeps each dtype to a few seconds."""
import os

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import mrp_gnn_amd as m
from mrp_gnn_amd import aggregate
import half_cases as hc
import oracle
from graph_strategies import batches

pytestmark = pytest.mark.gpu

SETTINGS = settings(max_examples=int(os.environ.get("MRP_PROPERTY_EXAMPLES", "25")), deadline=None,
                    derandomize=not os.environ.get("MRP_PROPERTY_HUNT"), database=None,
                    suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large,
                                           HealthCheck.function_scoped_fixture])


def _edges_per_graph(bnn, dst):
    goff = np.concatenate([[0], np.cumsum(bnn)])
    dst = np.asarray(dst, np.int64)
    return [int(((dst >= goff[i]) & (dst < goff[i + 1])).sum()) for i in range(len(bnn))]


def _check(dev, T, case, C, H, W, mode, seed):
    bnn, src, dst = case
    g = m.RobotGraph(src, dst, num_nodes=int(sum(bnn)), batch_num_nodes=bnn,
                     batch_num_edges=_edges_per_graph(bnn, dst))
    N, E = g.num_nodes(), g.num_edges()
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen).to(T)
    G = torch.randn(N, C, H, W, generator=gen).to(T)
    gb = torch.rand(E, C, 2, generator=gen)
    src, dst = (t.numpy() for t in g.edges())
    csr = g.csr(dev)
    key = hc.KEY[T]
    before = aggregate.PATH_COUNTS["fwd_" + key]
    xd = x.to(dev).requires_grad_(True)
    gbd = gb.to(dev).requires_grad_(True)
    out = m.film_mean(xd, gbd, csr, mode)
    assert out.dtype == T and aggregate.PATH_COUNTS["fwd_" + key] == before + 1
    ref64 = oracle.film_aggregate(x.double(), gb.double(), src, dst, mode)
    hc.assert_elementwise(out, ref64, T, "out")
    if N == 0:
        return
    out.backward(G.to(dev))
    assert xd.grad.dtype == T
    if E == 0:  # the aggregate is all zeros, independent of x
        assert not xd.grad.any()
        return
    dx64, dgb64 = oracle.film_aggregate_grads(x.double(), gb.double(), src, dst, G.double(), mode)
    hc.assert_elementwise(xd.grad, dx64, T, "dx")
    if mode == "copy_mean":  # gamma/beta do not enter: no gradient (or zeros), grad_x alone is checked
        assert gbd.grad is None or not gbd.grad.any()
        return
    _, dgb32 = oracle.film_aggregate_grads(x.float(), gb, src, dst, G.float(), mode)
    hc.assert_relative(gbd.grad, dgb32, dgb64, "dgb")


@pytest.mark.parametrize("key", list(hc.DTYPES))
def test_arbitrary_graphs_vs_float64(cuda_device, key):
    T = hc.DTYPES[key]

    @SETTINGS
    @given(batches(), st.integers(1, 8), st.sampled_from([(1, 1), (1, 3), (2, 2), (2, 4), (3, 3), (3, 5), (4, 4)]),
           st.sampled_from(["film_mean", "film_sum", "copy_mean"]), st.integers(0, 2 ** 31 - 1))
    def run(case, C, hw, mode, seed):
        _check(cuda_device, T, case, C, hw[0], hw[1], mode, seed)

    run()
