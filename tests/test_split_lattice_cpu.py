"""The teeth of the split-bf16 accuracy tests (``test_gpu_split_lattice.py``, ``test_gpu_split_fp32.py``),
pinned without a GPU: a torch emulation of the six-product scheme (``split_cases.emulate``: bf16 casts
for the split, float64 block products, hi and lo sums in fp32) run on the very operands the GPU tests
generate.  The correct form reproduces the float64 product bit for bit; every defective form — each of
the six partial products dropped, a two-way split, first-order products only — misses it in the
pairings listed in :data:`CATCHES`; and on the random shapes every defective form is past 2 x the fp32
GEMM's error while the correct form is not.  A later edit to the generators that blunts them fails here."""
import pytest
import torch

import split_cases as sc

#: defective form -> the pairings (A kind x B kind) whose lattice cases it must fail
CATCHES = {
    "drop_a0b0": {"threexbf16", "bf16xthree", "twoxtwo"},
    "drop_a1b0": {"threexbf16", "twoxtwo"},
    "drop_a0b1": {"bf16xthree", "twoxtwo"},
    "drop_a2b0": {"threexbf16"},
    "drop_a0b2": {"bf16xthree"},
    "drop_a1b1": {"twoxtwo"},
    "two_way": {"threexbf16", "bf16xthree"},
    "first_order": {"threexbf16", "bf16xthree", "twoxtwo"},
}


def _wrong(A, B, bias, form, ref64):
    got = sc.emulate(A, B, form, bias)
    return int((got != ref64.float()).sum()), got.numel()


def _lattice_products():
    """(label, pairing id, A, B, bias, float64 product) of every 2-D product of the GPU tests' compress and
    encoder-backward lattice cases (the builders assert the sparsity and representability conditions)."""
    out = []
    for shape in sc.COMPRESS_SHAPES:
        for p in sc.PAIRINGS:
            c = sc.compress_case(*shape, p)
            refs = sc.compress_refs(c)
            r2 = {"fwd": sc._rows(refs["y"]), "dgrad": torch.cat((sc._rows(refs["gx"]), sc._rows(refs["ga"])), 0),
                  "wgrad": refs["gw"]}
            for k, (A, B, b) in sc.compress_products(c).items():
                out.append((f"compress {k} {shape}", sc.pairing_id(p), A, B, b, r2[k]))
    for shape in sc.ENCODER_BWD_SHAPES:
        for p in sc.PAIRINGS:
            c = sc.encoder_bwd_case(*shape, p)
            for k, (A, B, b) in sc.encoder_bwd_products(c).items():
                # the B-side kind sits in A for dh^T (A = W2^T): the pairing as (A kind, B kind)
                pid = sc.pairing_id(p if k == "dw2" else p[::-1])
                out.append((f"encoder {k} {shape}", pid, A, B, b, c["dhT_d"] if k == "dhT" else c["dw2"]))
    return out


@pytest.fixture(scope="module")
def lattice_products():
    return _lattice_products()


def test_six_products_are_exact_on_every_lattice_case(lattice_products):
    for label, pid, A, B, b, ref in lattice_products:
        wrong, n = _wrong(A, B, b, "six", ref)
        assert wrong == 0, f"{label} {pid}: the six-product form misses {wrong} of {n} outputs"


@pytest.mark.parametrize("form", sc.DEFECTS)
def test_defective_form_fails_exactness(lattice_products, form):
    """Each defective form fails exactly the pairings of :data:`CATCHES`, in every kernel's product, and
    there on more than a quarter of the outputs (a lost term is +-q per non-zero product: the few
    outputs where those cancel, or whose sum is empty, stay right)."""
    report = []
    for label, pid, A, B, b, ref in lattice_products:
        wrong, n = _wrong(A, B, b, form, ref)
        report.append(f"{label} {pid}: {wrong}/{n}")
        if pid in CATCHES[form]:
            assert 4 * wrong > n, f"{form} goes unnoticed by {pid} in {label}: {wrong} of {n} outputs wrong"
        else:
            assert wrong == 0, f"{form}: {pid} was not expected to catch it in {label} ({wrong} of {n} wrong)"
    assert CATCHES[form], f"{form} is caught by no pairing\n" + "\n".join(report)


def test_every_defect_is_caught_by_some_pairing():
    caught = {p: sorted(f for f in sc.DEFECTS if p in CATCHES[f]) for p in map(sc.pairing_id, sc.PAIRINGS)}
    for f in sc.DEFECTS:
        assert any(f in v for v in caught.values()), f"{f} is caught by no pairing; pairings catch {caught}"


@pytest.mark.parametrize("E,C", sc.ENCODER_SHAPES)
@pytest.mark.parametrize("variant", list(sc.ENCODER_VARIANTS))
def test_encoder_chain_is_exact(E, C, variant):
    """Both stages of every encoder forward case: conditions (asserted by the builder) and the emulation."""
    c = sc.encoder_case(E, C, variant)
    pre = c["pose"].double() @ c["w1"].double().t()
    for k, (A, B, b) in sc.encoder_products(c).items():
        ref = pre.t() if k == "hidden" else c["z64"].t()
        wrong, n = _wrong(A, B, b, "six", ref)
        assert wrong == 0, f"{variant} {k}: the six-product form misses {wrong} of {n} outputs"


def test_encoder_variants_need_every_part():
    """Over the variants each stage of the chain sees all three pairings: per stage, every defective form
    is caught by some variant."""
    E, C = 33, 96
    for stage in ("hidden", "logits"):
        missed = set(sc.DEFECTS)
        seen = {}
        for variant in sc.ENCODER_VARIANTS:
            c = sc.encoder_case(E, C, variant)
            A, B, b = sc.encoder_products(c)[stage]
            ref = (c["pose"].double() @ c["w1"].double().t()).t() if stage == "hidden" else c["z64"].t()
            for f in sc.DEFECTS:
                if _wrong(A, B, b, f, ref)[0] > 0:
                    missed.discard(f)
                    seen.setdefault(variant, []).append(f)
        assert not missed, f"encoder {stage}: no variant catches {sorted(missed)}; variants catch {seen}"


@pytest.mark.parametrize("pairing", sc.PAIRINGS, ids=sc.pairing_id)
def test_reduce_and_coarse_cases_hold_their_conditions(pairing):
    for E, C in sc.ENCODER_BWD_SHAPES:
        sc.encoder_reduce_case(E, C, pairing)
        sc.encoder_dw1_refs(sc.encoder_bwd_case(E, C, ("bf16", "two")))


#: (name, M, K, N) of the random-operand products of test_gpu_split_fp32.py, as A (M, K) B (K, N)
RANDOM_SHAPES = [("compress fwd / dgrad n=2 C=512 P=32", 512, 1024, 64), ("compress wgrad n=32 C=64 P=32", 64, 1024, 128),
                 ("encoder z E=64 C=1024", 2048, 1024, 64), ("encoder dW2 E=1024 C=64", 128, 1024, 64),
                 ("encoder dhT C=512 E=64", 512, 1024, 64)]
FACTOR = 2.0


@pytest.mark.parametrize("name,M,K,N", RANDOM_SHAPES, ids=[s[0] for s in RANDOM_SHAPES])
def test_random_operands_separate_the_forms(name, M, K, N):
    g = torch.Generator().manual_seed(K + M)
    A = torch.randn(M, K, generator=g) / K ** 0.5
    B = torch.randn(K, N, generator=g)
    f64 = A.double() @ B.double()
    f32 = A @ B
    ok, (e, e32) = sc.within_fp32(sc.emulate(A, B, "six"), f32, f64, FACTOR)
    assert ok, f"{name}: the six-product form {e:.3g} against fp32 {e32:.3g}"
    for form in sc.DEFECTS:
        ok, (e, e32) = sc.within_fp32(sc.emulate(A, B, form), f32, f64, FACTOR)
        assert not ok, f"{name}: {form} passes the factor-{FACTOR:g} bound ({e:.3g} against fp32 {e32:.3g})"
