"""Test infrastructure for the reduced precision modes of the split-bf16 compress
(``compress.set_compress_precision``: ``"high"`` keeps two bf16 parts per operand and the products
``a0 b0 + a0 b1 + a1 b0``, ``"medium"`` one part and ``a0 b0``; in general parts ``p < parts`` and the
products with ``i + j < parts``).

On the lattice operands of ``tests/split_cases.py`` every part is known by construction and every partial
sum is an fp32 value, so a kernel that keeps exactly the products of its mode must reproduce
:func:`trunc_product` BIT FOR BIT — and, because the truncated product differs from the six-product value
in most outputs (asserted here: at least half, else the case proves nothing), a kernel that keeps a product
it should drop, or drops one it should keep, fails.
"""
import functools

import torch

import split_cases as sc

#: mode -> bf16 parts kept per operand
PARTS = {"highest": 3, "high": 2, "medium": 1}
REDUCED = ("high", "medium")
#: per-term truncation bounds of the reduced modes (include/mrp_gnn.h): c x sum_k |a_k b_k|
TERM_BOUND = {"high": 3.1 * 2.0 ** -18, "medium": 2.01 * 2.0 ** -9}


def trunc_product(A, B, parts, bias=None, what=""):
    """The float64 sum over k of the ``split3`` part products ``a_i b_j`` with ``i + j < parts`` (+ bias down
    the rows) of fp32 CPU operands A (M, K) and B (K, N).  Asserts that the result is an fp32 value and that
    it differs from the full product in at least half of the outputs."""
    pa = [p.double() for p in sc.split3(A)]
    pb = [p.double() for p in sc.split3(B)]
    assert torch.equal(pa[0] + pa[1] + pa[2], A.double()) and torch.equal(pb[0] + pb[1] + pb[2], B.double()), \
        f"{what}: operands are not three-part values"
    out = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float64)
    for i in range(parts):
        for j in range(parts - i):
            out = out + pa[i] @ pb[j]
    full = A.double() @ B.double()
    if bias is not None:
        out = out + bias.double()[:, None]
        full = full + bias.double()[:, None]
    assert torch.equal(out.float().double(), out), f"{what}: the truncated product is not an fp32 value"
    if parts < 3:
        differ = int((out != full).sum())
        assert differ * 2 >= out.numel(), \
            f"{what}: parts={parts} differs from the six-product value in only {differ} of {out.numel()} outputs"
    return out


@functools.lru_cache(maxsize=None)
def compress_case(n, C, P, pairing):
    return sc.compress_case(n, C, P, pairing)


@functools.lru_cache(maxsize=None)
def compress_trunc_refs(n, C, P, pairing, parts, bias=True):
    """Float64 results of a compress lattice case in a reduced mode, in the kernels' layouts: y, gx, ga
    (n, C, P), gw (C, 2C) — and gb (C), the exact row sums of the FULL gy (no truncation in any mode)."""
    c = compress_case(n, C, P, pairing)
    tag = f"{sc.pairing_id(pairing)} n={n} C={C} P={P} parts={parts}"
    r = {k: trunc_product(A, B, parts, bb, f"compress {k} {tag}")
         for k, (A, B, bb) in sc.compress_products(c, bias).items()}
    g = r["dgrad"].view(2 * C, n, P).permute(1, 0, 2)
    gb = sc._rows(c["gy_s"]).double().sum(1)
    assert torch.equal(gb.float().double(), gb)
    return {"y": r["fwd"].view(C, n, P).permute(1, 0, 2).contiguous(), "gx": g[:, :C].contiguous(),
            "ga": g[:, C:].contiguous(), "gw": r["wgrad"], "gb": gb}


def moved(before, counts):
    """PATH_COUNTS keys that changed since the snapshot ``before`` -> by how much."""
    return {k: v - before.get(k, 0) for k, v in counts.items() if v != before.get(k, 0)}
