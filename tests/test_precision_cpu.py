"""CPU: the teeth of the reduced-precision lattice test (``tests/precision_cases.py``) and the semantics of
``set_compress_precision`` / ``compress_precision`` / ``compress_precision_scope`` — no GPU needed."""
import pytest
import torch

import mrp_gnn_amd as m
import precision_cases as pc
import split_cases as sc
from mrp_gnn_amd import compress


@pytest.mark.parametrize("parts", [2, 1])
@pytest.mark.parametrize("n,C,P", sc.COMPRESS_SHAPES)
@pytest.mark.parametrize("pairing", sc.PAIRINGS, ids=sc.pairing_id)
def test_truncated_lattice_products_are_exact_and_differ(pairing, n, C, P, parts):
    """For every compress lattice case and product: the sum of the part products with i + j < parts is an
    fp32 value (so a correct kernel must reproduce it bit for bit) and differs from the six-product value
    in at least half of the outputs (so a kernel that keeps or drops the wrong product fails) — both
    asserted inside ``trunc_product``; and at parts = 3 it is the exact product."""
    c = pc.compress_case(n, C, P, pairing)
    for bias in (True, False):
        for name, (A, B, bb) in sc.compress_products(c, bias).items():
            t = pc.trunc_product(A, B, parts, bb, f"{name} {sc.pairing_id(pairing)}")
            full = pc.trunc_product(A, B, 3, bb)
            ref = A.double() @ B.double() + (bb.double()[:, None] if bb is not None else 0.0)
            assert torch.equal(full, ref)
            frac = float((t != full).double().mean())
            assert frac >= 0.5, (name, frac)
    r = pc.compress_trunc_refs(n, C, P, pairing, parts)
    assert torch.equal(r["gb"], sc.compress_refs(c)["gb"])  # the row sums are of the full gy in every mode


def test_precision_setter_semantics():
    assert compress.compress_precision() == "highest"  # the default
    assert m.compress_precision is compress.compress_precision
    assert m.set_compress_precision is compress.set_compress_precision
    assert m.compress_precision_scope is compress.compress_precision_scope
    try:
        assert compress.set_compress_precision("high") == "highest"
        assert compress.compress_precision() == "high"
        assert compress.set_compress_precision("medium") == "high"
        assert compress.set_compress_precision("highest") == "medium"
        for bad in ("low", "tf32", "", None, 3):
            with pytest.raises(ValueError):
                compress.set_compress_precision(bad)
            assert compress.compress_precision() == "highest"
        with compress.compress_precision_scope("high"):
            assert compress.compress_precision() == "high"
            with compress.compress_precision_scope("medium"):
                assert compress.compress_precision() == "medium"
            assert compress.compress_precision() == "high"
        assert compress.compress_precision() == "highest"
        with pytest.raises(RuntimeError, match="boom"):
            with compress.compress_precision_scope("medium"):
                assert compress.compress_precision() == "medium"
                raise RuntimeError("boom")
        assert compress.compress_precision() == "highest"  # restored on an exception too
        with pytest.raises(ValueError):
            with compress.compress_precision_scope("fast"):
                pass
        assert compress.compress_precision() == "highest"
    finally:
        compress.set_compress_precision("highest")


def test_mode_keys():
    assert compress.PRECISION_PARTS == pc.PARTS
    assert compress._mode_key("fwd_f32", "highest") == "fwd_f32"
    assert compress._mode_key("dgrad_f32", "high") == "dgrad_f32_high"
    assert compress._mode_key("wgrad_f32", "medium") == "wgrad_f32_medium"
