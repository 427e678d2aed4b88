"""Test infrastructure shared by the 16-bit feature tests (test_gpu_half_*.py): the graphs / shapes that
reach each code path of the bf16 / fp16 aggregation, the error bars, and cached float64 / float32 oracle
references (computed once per case and dtype, never modified).

Bars (all from the number formats, none from what the kernels give):

* elementwise, for a 16-bit output against float64: ``|got - ref| <= u_T |ref| + 1e-5 max|ref|`` with
  ``u_bf16 = 2^-8``, ``u_fp16 = 2^-11`` — one round-to-nearest of a value whose fp32 error is within
  the project's 1e-5 max-abs bar;
* relative, for the fp32 ``grad_gb``: ``rel_err <= max(1e-5, 4 x rel_err of the same oracle run in
  float32)`` (``stack_ref.within``'s bar).
"""
import functools

import numpy as np
import torch

import mrp_gnn_amd as m
import oracle
from conftest import rel_err

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
KEY = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}


def _poses(rng, n):
    return np.concatenate([rng.uniform(-10, 10, (n, 3)), rng.standard_normal((n, 4))], 1).astype(np.float32)


def _frames(ns, seed, knn=None):
    rng = np.random.RandomState(seed)
    return m.batch([m.frame_graph(_poses(rng, n), knn=knn) for n in ns])


def _ragged(seed):
    """Frames of 2 and 8 robots around a 5-node graph with mixed in-degrees: node 4 has none, 0->1 is
    a multi-edge, 3->3 a self-loop (as tests/golden's mixed_ragged case)."""
    rng = np.random.RandomState(seed)
    mid = m.RobotGraph([0, 0, 2, 3, 1, 0, 2], [1, 1, 1, 3, 0, 2, 3], num_nodes=5)
    g2, g8 = m.frame_graph(_poses(rng, 2)), m.frame_graph(_poses(rng, 8))
    return m.batch([g2, mid, g8])  # (the aggregation needs no edge poses: gamma/beta are given)


#: name -> (graph builder, C, H, W, what it reaches)
CASES = {
    "a": (lambda: _frames([8, 8], 1), 8, 32, 32, "16-byte slices, 64 lanes per plane, plane split, fused backward"),
    "b": (lambda: _frames([5, 5], 2), 16, 8, 8, "the reference's camera count, small planes, 16-channel workgroups"),
    "c": (lambda: _frames([4, 4], 3), 6, 6, 6, "P % 8 != 0: 4-element slices; C no multiple of the block"),
    "d": (lambda: _frames([3], 4), 3, 3, 3, "odd P: one element per access"),
    "e": (lambda: _frames([16, 16], 5, knn=4), 8, 16, 16, "REGULAR(4) forward, 9-16-node backward"),
    "f": (lambda: _frames([12], 6), 4, 8, 8, "9-12-node backward unit"),
    "g": (lambda: _ragged(7), 8, 4, 4, "CSR: ragged batch, a node without in-edges (zero fill)"),
    # h: the slice starts 64 elements (128 bytes) in and its node stride is 1152 elements, so it is still
    # 16-byte aligned and reaches only "node stride != C P"; the misalignment fallbacks are i4 and i1
    "h": (lambda: _frames([5, 5], 2), 16, 8, 8, "x a channel slice of a wider tensor: node stride != C P"),
    # beyond the issue's table: the slice-width fallbacks by pointer alignment
    "i4": (lambda: _frames([5, 5], 2), 16, 8, 8, "x 8-byte but not 16-byte aligned: 4-element slices"),
    "i1": (lambda: _frames([5, 5], 2), 16, 8, 8, "x 2-byte aligned only: one element per access"),
}
SMALL = ["a", "b", "c", "d", "g", "h", "i4", "i1"]  # <= 8 nodes: the fp32 backward is film_bwd_fused


@functools.lru_cache(maxsize=None)
def graph(name):
    return CASES[name][0]()


def shape(name):
    g = graph(name)
    _, C, H, W, _ = CASES[name]
    return g.num_nodes(), C, H, W


@functools.lru_cache(maxsize=None)
def host_inputs(name, key):
    """(x, gb, z, G) on the CPU: x and G drawn in fp32 and rounded to T (returned in T), gb uniform
    (0, 1) and logits z with gb == sigmoid(z) to fp32 rounding, both fp32."""
    T = DTYPES[key]
    n, C, H, W = shape(name)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 131 + (0 if key == "bf16" else 1))
    x = torch.randn(n, C, H, W, generator=gen).to(T)
    G = torch.randn(n, C, H, W, generator=gen).to(T)
    z = torch.randn(graph(name).num_edges(), C, 2, generator=gen)
    return x, torch.sigmoid(z), z, G


def embed(name, x):
    """The tensor a case hands the kernels, holding x's values: (leaf, view) with view == x.  Case h: a
    channel slice of a (Nt, 18, H, W) tensor; i4 / i1: a view 4 / 1 elements into a flat buffer."""
    n, C, H, W = x.shape
    if name == "h":
        leaf = torch.zeros(n, C + 2, H, W, dtype=x.dtype, device=x.device)
        leaf[:, 1:C + 1] = x
        return leaf, (lambda t: t[:, 1:C + 1])
    if name in ("i4", "i1"):
        off = 4 if name == "i4" else 1
        leaf = torch.zeros(x.numel() + 8, dtype=x.dtype, device=x.device)
        leaf[off:off + x.numel()] = x.reshape(-1)
        return leaf, (lambda t: t[off:off + n * C * H * W].view(n, C, H, W))
    return x.clone(), (lambda t: t)


@functools.lru_cache(maxsize=None)
def oracle_ref(name, key, mode="film_mean"):
    """Float64 and float32 oracle runs on the widened inputs: dict of out / dx / dgb for each."""
    x, gb, _, G = host_inputs(name, key)
    src, dst = (t.numpy() for t in graph(name).edges())
    ref = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        xx, gg, GG = x.to(dt), gb.to(dt), G.to(dt)
        ref["out" + tag] = oracle.film_aggregate(xx, gg, src, dst, mode)
        ref["dx" + tag], ref["dgb" + tag] = oracle.film_aggregate_grads(xx, gg, src, dst, GG, mode)
    return ref


def assert_elementwise(got, ref64, T, what=""):
    """|got - ref| <= u_T |ref| + 1e-5 max|ref| for every element (see module docstring)."""
    got = got.detach().double().cpu()
    ref = ref64.detach().double().cpu()
    assert got.shape == ref.shape
    if ref.numel() == 0:
        return
    bound = UNIT[T] * ref.abs() + 1e-5 * ref.abs().max()
    excess = ((got - ref).abs() - bound).max()
    assert float(excess) <= 0.0, (what, float(excess), float((got - ref).abs().max()))


def assert_relative(got, ref32, ref64, what=""):
    """rel_err(got) <= max(1e-5, 4 rel_err(fp32 oracle)) against float64."""
    e, e32 = rel_err(got.detach().cpu().numpy(), ref64.numpy()), rel_err(ref32.numpy(), ref64.numpy())
    assert e <= max(1e-5, 4.0 * e32), (what, e, e32)


def bits(t):
    """The raw bits of a tensor (NaN-safe, sign-of-zero-exact comparison)."""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)
