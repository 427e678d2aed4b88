"""The teeth of ``test_gpu_special_values.py``, pinned without a GPU: the inputs ``special_cases`` builds are
run through torch / numpy emulations of the defective forms a kernel could have — ``div_fast`` without its
gate, a ReLU that drops NaN (``max(x, 0)``) or a NaN with its sign bit set (integer max on the bits), a
saturating and a truncating 16-bit store, a bf16 rounding without its NaN guard, a dense ``0 * inf`` forward —
and each defect must fail the very check the GPU test applies, while the reference evaluation passes it.  The
scale pairs of the split-bf16 equivariance test are checked on ``split_cases.emulate`` with the operands
used.  Inputs that no defect can fail on test nothing; a later edit that blunts them fails here."""
import numpy as np
import pytest
import torch

import half_cases as hc
import special_cases as spc
import split_cases as sc

HALF = ["bf16", "f16"]


# ---- 1. the division ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", range(2, 16))
def test_div_fast_is_wrong_where_the_gate_says(D):
    """+-0 loses its sign, +-inf gives NaN, and below 2^-124 the quotient is wrong for D in TINY_DIVISORS (for
    the other divisors the search finds nothing); on ordinary values the emulation equals x / D."""
    q = spc.div_fast(np.float32([0.0, -0.0, np.inf, -np.inf]), D)
    assert not np.signbit(q[0]) and not np.signbit(q[1]) and np.isnan(q[2]) and np.isnan(q[3])
    x = np.random.RandomState(D).randn(1 << 14).astype(np.float32)
    assert np.array_equal(spc.div_fast(x, D), x / np.float32(D))
    tiny = spc.tiny_mismatches(D)
    assert bool(tiny) == (D in spc.TINY_DIVISORS)
    for v in tiny:
        assert 0.0 < v < 2.0 ** -124
        assert spc.div_fast(np.float32([v]), D)[0] != np.float32(v) / np.float32(D)


@pytest.mark.parametrize("key", ["f32"] + HALF)
@pytest.mark.parametrize("n", range(2, 17))
def test_division_inputs_fail_an_ungated_div_fast(n, key):
    c = spc.division_case(n, key)
    D = n - 1
    sums = spc.division_sums(c)
    flat = sums.view(2 * n, spc.DIV_C, -1)
    ref = spc.aggregate_ref(c["graph"], c["x"], c["gb"])
    with np.errstate(all="ignore"):
        spc.assert_same(torch.from_numpy(sums.numpy() / np.float32(D)), ref, "sum / D is the oracle's mean")
    ungated = torch.from_numpy(spc.div_fast(sums.numpy(), D)).view_as(flat)
    kinds = {k for k, *_ in c["slots"]}
    assert {"zero", "pinf", "ninf"} <= kinds and (n == 2 or "nan" in kinds)
    assert ("subnormal" in kinds) == (key != "f16") and ("tiny" in kinds) == (key == "f32" and D in spc.TINY_DIVISORS)
    # the special sums are what they claim, the last destination (the short group when n % 4 != 0) among them
    assert n - 1 in {v % n for kind, v, ch, p in c["slots"] if kind == "zero"}
    refl = ref.view_as(flat)
    for kind, v, ch, p in c["slots"]:
        s = float(flat[v, ch, p])
        if kind == "zero":
            assert s == 0.0 and not np.signbit(s)
        elif kind == "subnormal":
            assert 0.0 < s < 2.0 ** -126
        elif kind == "tiny":
            assert 0.0 < s < 2.0 ** -124 and float(ungated[v, ch, p]) != float(refl[v, ch, p])
        elif kind in ("pinf", "ninf"):
            assert s == (np.inf if kind == "pinf" else -np.inf) and np.isnan(float(ungated[v, ch, p]))
        else:
            assert np.isnan(s)
    with pytest.raises(AssertionError):
        spc.assert_same(ungated.view_as(ref), ref, "ungated")
    # most sums stay ordinary: they share the groups of four with the special ones
    assert int((torch.isfinite(flat) & (flat.abs() >= 2.0 ** -124)).sum()) > flat.numel() // 2


# ---- 3. the store -------------------------------------------------------------------------------------------
#: the first rows of the tables, written out: what one round to nearest even gives
STORE_WANT = {
    "f16": [65504.0, np.inf, np.inf, -np.inf, 2.0 ** -24, 0.0, -0.0, 2.0 ** -24, 2.0 ** -15 + 2.0 ** -24, 1.0, 1.0 + 2.0 ** -9,
            1.0, 1.0 + 2.0 ** -10],
    "bf16": [2.0 ** 128 - 2.0 ** 120, np.inf, -np.inf, 2.0 ** -133, 0.0, -0.0, 2.0 ** -133, 2.0 ** -127 + 2.0 ** -133, 1.0,
             1.0 + 2.0 ** -6, 1.0, 1.0 + 2.0 ** -7],
}


@pytest.mark.parametrize("key", HALF)
def test_store_table_rounds_as_written(key):
    T = spc.DTYPES[key]
    _, _, _, t32 = spc.store_table(key)
    want = torch.tensor(STORE_WANT[key], dtype=torch.float64)
    got = t32.to(T)
    assert torch.equal(got[:len(want)].double(), want)
    assert torch.equal(torch.signbit(got[:len(want)]), torch.signbit(want))
    tail = got[len(want):].double()
    assert torch.isnan(tail[0]) and tail[1] == np.inf and tail[2] == -np.inf and torch.isnan(tail[3])
    assert bool(torch.signbit(got[len(want) + 4])) is False  # -0 + 0 = +0 in the sum
    if key == "bf16":
        assert int(spc.bits(t32[1:2])) == spc.TOP


@pytest.mark.parametrize("key", HALF)
def test_store_inputs_fail_the_defective_casts(key):
    T = spc.DTYPES[key]
    c = spc.store_case(key)
    want32 = c["want32"]
    spc.assert_same(want32.to(T), c["want"], "torch's cast")
    out0 = want32[0]
    assert int(torch.isinf(out0.to(T)).sum()) > int(torch.isinf(out0).sum()), "no finite sum overflows at the store"
    for name, cast in (("saturating", spc.cast_saturating), ("truncating", spc.cast_truncating)):
        with pytest.raises(AssertionError):
            spc.assert_same(cast(want32, T), c["want"], name)
    # the guard-less bf16 rounding: the NaN gamma's payload carries into the exponent and sign.  Assumption: the
    # hardware hands the store gamma's all-ones payload (it propagates an operand NaN), substituted here; if a
    # kernel's arithmetic canonicalised the NaN to 0x7fc00000 first, this defect would round it to a NaN too and
    # pass the GPU test — a 16-bit x cannot carry such a payload (its widened NaNs end in sixteen zero bits)
    nan = torch.isnan(want32)
    assert bool(nan[0, 2].all())
    payload = torch.where(nan, spc.FULL_NAN, want32)  # what hardware that propagates payloads hands the store
    guardless = spc.cast_bf16_no_nan_guard(payload)
    assert not bool(torch.isnan(guardless[0, 2]).any())
    if key == "bf16":
        finite = ~nan
        assert torch.equal(spc.bits(guardless)[finite], spc.bits(c["want"])[finite]), "the emulation itself rounds to even"
        with pytest.raises(AssertionError):
            spc.assert_same(guardless, c["want"], "guard-less")


# ---- 4. poison ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["e", "g"])
@pytest.mark.parametrize("poison", list(spc.POISON))
def test_forward_poison_fails_a_dense_forward(name, poison):
    """k-NN (case e) and the ragged batch with an edgeless node (case g): the reference confines the poison to
    the poisoned nodes' out-neighbours; a dense forward (0 x inf, 0 x NaN) spreads it over the whole graph."""
    g = hc.graph(name)
    x, gb, _, _ = hc.host_inputs(name, "bf16")
    x = x.float()
    places = spc.poison_places(name)
    xp = spc.poisoned(x, places, spc.POISON[poison])
    ref, refp = spc.aggregate_ref(g, x, gb), spc.aggregate_ref(g, xp, gb)
    spc.assert_confined(refp, ref, refp, "the reference")
    dense, densep = spc.dense_forward(g, x, gb), spc.dense_forward(g, xp, gb)
    assert float((dense - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    with pytest.raises(AssertionError, match="outside the allowed set"):
        spc.assert_confined(densep, dense, refp, "dense")
    if name == "g":  # the edgeless node's poison reaches nobody: its own place in the reference stays zero
        node = 6
        assert not bool(refp[node].any()) and (6 in [p[0] for p in places])


@pytest.mark.parametrize("E,C", spc.ENCODER_SHAPES + (spc.ENCODER_PADDED,))
@pytest.mark.parametrize("poison", list(spc.POISON))
def test_encoder_poison_fails_the_defective_relus(E, C, poison):
    """Assumption of the integer-max emulation: the NaN hidden pre-activations have their sign bit set (forced
    here).  An integer max keeps a positive NaN (``test_integer_max_relu_drops_only_the_negative_nan``), so this
    defect fails the GPU test only where the kernel's arithmetic hands the ReLU a NaN with its sign set — which
    the sign-bit poison asks of a NaN-propagating multiply; what the matrix cores return is not modelled here."""
    c = spc.encoder_case(E, C)
    h0, z0 = spc.encoder_ref(c, c["pose"])
    assert 0.2 < float((h0 > 0).float().mean()) < 0.8
    for row, col in zip(c["rows"], c["col"]):
        pose = c["pose"].clone()
        pose[row, col] = spc.POISON[poison]
        h, z = spc.encoder_ref(c, pose)
        allowed = torch.zeros_like(z, dtype=torch.bool)
        allowed[row] = True
        assert bool((~torch.isfinite(z[row])).all())
        spc.assert_confined(z, z0, z, "reference", allowed)
        hk, zk = spc.encoder_ref(c, pose, spc.relu_keeps_nan)
        spc.assert_confined(zk, z0, z, "x < 0 ? 0 : x", allowed)
        if poison == "inf":
            continue  # relu(+inf) = inf under every form: the NaN poisons are the discriminating ones
        for name, relu in (("drops", spc.relu_drops_nan), ("integer", lambda t: spc.relu_integer_max(
                torch.where(torch.isnan(t), spc.NEG_NAN, t)))):
            hd, zd = spc.encoder_ref(c, pose, relu)
            with pytest.raises(AssertionError, match="are finite"):
                spc.assert_confined(zd, z0, z, name, allowed)


def test_integer_max_relu_drops_only_the_negative_nan():
    t = torch.stack([spc.POISON["nan"], spc.NEG_NAN, torch.tensor(-0.0), torch.tensor(2.0), torch.tensor(-3.0)])
    r = spc.relu_integer_max(t)
    assert torch.isnan(r[0]) and float(r[1]) == 0.0 and float(r[3]) == 2.0 and float(r[4]) == 0.0
    k = spc.relu_keeps_nan(t)
    assert torch.isnan(k[0]) and torch.isnan(k[1]) and float(k[3]) == 2.0 and float(k[4]) == 0.0


# ---- 2. the sigmoid ---------------------------------------------------------------------------------------------
def test_sigmoid_bound_admits_an_fp32_evaluation_and_pins_saturation():
    z = np.array(spc.LOGITS, np.float64)
    s32 = torch.sigmoid(torch.tensor(spc.LOGITS, dtype=torch.float32)).double().numpy()
    assert bool((np.abs(s32 - spc.sigmoid64(z)) <= spc.sigmoid_bound(z)).all())
    assert bool((np.float32(spc.sigmoid64(z[z >= spc.ONE_FROM])) == 1.0).all()) and spc.sigmoid64(-np.inf) == 0.0
    assert bool((spc.dsigmoid64(z[np.abs(z) >= 104]) < 2.0 ** -149).all())  # below fp32's smallest subnormal: 0


# ---- 5. scale equivariance ----------------------------------------------------------------------------------------
#: (n, C, P) of the GPU test's SCALE_SHAPES
SHAPES = ((3, 64, 32), (3, 256, 32), (3, 128, 32))


def _scaled(A, B, bias, sa, sb):
    return A * 2.0 ** sa, B * 2.0 ** sb, bias * 2.0 ** (sa + sb) if bias is not None else None


def _equivariant(A, B, bias, sa, sb, form="six"):
    base = sc.emulate(A, B, form, bias)
    As, Bs, bs = _scaled(A, B, bias, sa, sb)
    got = sc.emulate(As, Bs, form, bs)
    ok_parts = spc.parts_normal(As) and spc.parts_normal(Bs)
    return torch.equal(spc.bits(got), spc.bits(base * 2.0 ** (sa + sb))) and bool(torch.isfinite(got).all()), ok_parts


@pytest.mark.parametrize("shape,pair", [(sh, p) for sh in SHAPES for p in spc.scale_pairs(sh[1])], ids=str)
def test_emulation_is_scale_equivariant_on_the_pairs_used(shape, pair):
    c = spc.scale_case(*shape)
    for name, (A, B, bias) in spc.scale_products(c).items():
        sa, sb = pair  # A is the weight (gy in the weight gradient), B the features
        eq, normal = _equivariant(A, B, bias, sa, sb)
        assert eq and normal, (name, pair, eq, normal)
        eq2, _ = _equivariant(A, B, bias, sa, sb, "two_way")  # parts = 2
        assert eq2, (name, pair, "parts = 2")


@pytest.mark.parametrize("E,C", spc.ENCODER_SHAPES)
@pytest.mark.parametrize("pair", spc.ENC_SCALE_PAIRS, ids=str)
def test_encoder_emulation_is_scale_equivariant_on_the_pairs_used(E, C, pair):
    c = spc.encoder_scale_case(E, C)
    h0, z0, _ = spc.encoder_emulate(c)
    h, z, products = spc.encoder_emulate(spc.encoder_scaled(c, *pair))
    k = 2.0 ** sum(pair)
    assert torch.equal(spc.bits(h), spc.bits(h0 * k)) and torch.equal(spc.bits(z), spc.bits(z0 * k))
    assert bool(torch.isfinite(z).all()) and bool((z != 0).all())
    for A, B in products:
        assert spc.parts_normal(A) and spc.parts_normal(B)


@pytest.mark.parametrize("shape", [sh for sh in SHAPES if (-55, -55) not in spc.scale_pairs(sh[1])])
def test_pair_left_out_at_the_wider_shapes_fails_the_check(shape):
    """(-55, -55) at C = 128 and 256: some product's scaled operands have a part below bf16's normal range."""
    c = spc.scale_case(*shape)
    assert not all(all(_equivariant(A, B, bias, -55, -55)) for A, B, bias in spc.scale_products(c).values())


@pytest.mark.parametrize("pair", spc.SCALE_BROKEN, ids=str)
def test_emulation_breaks_outside_the_domain(pair):
    assert not any(pair in spc.scale_pairs(sh[1]) for sh in SHAPES)
    c = spc.scale_case(*SHAPES[0])
    broke = []
    for name, (A, B, bias) in spc.scale_products(c).items():
        eq, normal = _equivariant(A, B, bias, *pair)
        broke.append(not (eq and normal))
    assert any(broke), pair


def test_upper_edge_of_the_split_domain():
    """A finite operand at 0x7f7f8000 = 2^128 - 2^119 rounds to a bf16 infinity; its residual is -inf and the
    next part NaN: the products that read it are non-finite, the others keep their bits."""
    top = spc.from_bits(spc.TOP)
    assert bool(torch.isfinite(top)) and bool(torch.isinf(top.bfloat16()))
    below = spc.from_bits(spc.TOP - 1)
    assert bool(torch.isfinite(below.bfloat16())) and spc.parts_normal(below.reshape(1))
    c = spc.scale_case(*SHAPES[0])
    A, B, bias = spc.scale_products(c)["fwd"]
    B2 = B.clone()
    B2[5, 7] = top
    base, got = sc.emulate(A, B, "six", bias), sc.emulate(A, B2, "six", bias)
    assert not bool(torch.isfinite(got[:, 7]).any())
    keep = torch.ones(B.shape[1], dtype=torch.bool)
    keep[7] = False
    assert torch.equal(spc.bits(got[:, keep]), spc.bits(base[:, keep]))
