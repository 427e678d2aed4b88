"""The multi-head attention tests' references against each other on the CPU, the teeth of the GPU tests' bar, and
the model option ``gcn_attn_heads`` — no GPU.

Measured here (every case x graph of tests/heads_cases.py, plain and gated, gamma/beta and logits):
the two float64 restatements differ by at most 6.4e-16 (relative, max-norm), and the header's backward formulas from
autograd by less than the 1e-12 asserted; the fp32 slice reference is within 6.2e-7 of float64 (worst: grad_w of the
gated form; the bar is 1e-5); the H-head ``out`` differs from the single-head ``out`` on the same operands by at
least 0.31, i.e. 31000 bars.
"""
import types

import pytest
import torch

import mrp_gnn_amd as m
import heads_cases as hc
from conftest import rel_err

TOL = 1e-5  # the suite's bar
PAIRS = [(n, c) for n in hc.GRAPHS for c in hc.CASES]
PAIR_IDS = [f"{n}-{i}" for n in hc.GRAPHS for i in hc.CASE_IDS]
NAMES = ("out", "attn", "rate", "dx", "dgb", "dw")


def _errs(got, ref):
    return {k: rel_err(a.numpy(), b.numpy()) for k, a, b in zip(NAMES, got, ref) if b is not None}


@pytest.mark.parametrize("name,case", PAIRS, ids=PAIR_IDS)
def test_the_two_references_agree(name, case):
    g, x, gb, z, G, base, w = hc.operands(name, case)
    H = case[1]
    worst = 0.0
    for ww in (None, w):
        for logits, p in ((False, gb), (True, z)):
            a = hc.slice_reference(g, x, p, H, G, base, logits, w=ww)
            b = hc.direct_reference(g, x, p, H, G, base, logits, w=ww)
            errs = _errs(a, b)
            print(name, case, "gated" if ww is not None else "plain", "logits" if logits else "gb", errs)
            assert set(errs) == (set(NAMES) if ww is not None else {"out", "attn", "dx", "dgb"})
            worst = max(worst, *errs.values())
        dx, dgb, dw = hc.slice_manual_backward(g, x, gb, H, G, w=ww)
        ref = hc.direct_reference(g, x, gb, H, G, w=ww)
        worst = max(worst, rel_err(dx.numpy(), ref[3].numpy()), rel_err(dgb.numpy(), ref[4].numpy()))
        if ww is not None:
            worst = max(worst, rel_err(dw.numpy(), ref[5].numpy()))
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("name,case", PAIRS, ids=PAIR_IDS)
def test_fp32_slice_reference_is_within_the_bar(name, case):
    g, x, gb, z, G, base, w = hc.operands(name, case)
    H = case[1]
    for ww in (None, w):
        ref = hc.direct_reference(g, x, z, H, G, base, True, w=ww)
        got = hc.slice_reference(g, x, z, H, G, base, True, dtype=torch.float32, w=ww)
        errs = _errs(got, ref)
        print(name, case, "gated" if ww is not None else "plain", errs)
        assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("name,case", [(n, c) for n, c in PAIRS if c[1] > 1],
                         ids=[i for i, (n, c) in zip(PAIR_IDS, PAIRS) if c[1] > 1])
def test_heads_change_the_result_far_beyond_the_bar(name, case):
    """A kernel that ignored ``heads`` would compute the single-head operator: 100 bars away at the least."""
    g, x, gb, z, G, base, w = hc.operands(name, case)
    H = case[1]
    for ww in (None, w):
        multi = hc.direct_reference(g, x, gb, H, w=ww)[0]
        single = hc.direct_reference(g, x, gb, 1, w=ww)[0]
        # the same scale too: the difference is the heads' own softmaxes, not the default scale
        same_scale = hc.direct_reference(g, x, gb, 1, scale=hc.head_scale(case[0], H), w=ww)[0]
        for other in (single, same_scale):
            e = rel_err(multi.numpy(), other.numpy())
            print(name, case, "gated" if ww is not None else "plain", e)
            assert e > 100 * TOL, e


def test_heads_1_is_the_single_head_reference():
    g, x, gb, z, G, base, w = hc.operands("knn16_4", (12, 1, 8, 8))
    out, attn, _, dx, dgb, _ = hc.slice_reference(g, x, z, 1, G, base, True)
    r = hc.ac.reference(g, x, z, G, base, True, torch.float64)
    assert torch.equal(out, r[0]) and torch.equal(attn[0], r[1]) and torch.equal(dx, r[2]) and torch.equal(dgb, r[3])


# ------------------------------------------------------------------------------------------------ the model option
def _opt(**kw):
    return types.SimpleNamespace(feature_dim=8, **kw)


@pytest.mark.parametrize("mode", ["film_attn", "film_wattn"])
@pytest.mark.parametrize("combine", ["cat_compress", "cat", "residual", "initial_mix"])
def test_the_option_adds_no_parameter_and_draws_no_random_number(mode, combine):
    layers = 1 if combine == "cat" else 2
    nets, states = [], []
    for extra in ({}, {"gcn_attn_heads": 1}, {"gcn_attn_heads": 4}):
        torch.manual_seed(5)
        nets.append(m.GCNStack(_opt(gcn_mode=mode, gcn_combine=combine, gcn_layers=layers, **extra)))
        states.append(torch.get_rng_state())
    ref = nets[0].state_dict()
    for net, st in zip(nets[1:], states[1:]):
        sd = net.state_dict()
        assert list(sd) == list(ref)
        assert all(torch.equal(sd[k], ref[k]) for k in ref)
        assert torch.equal(st, states[0])
    assert nets[0].gcn1._attn_heads() == 1 and nets[1].gcn1._attn_heads() == 1 and nets[2].gcn1._attn_heads() == 4
    # the same for the other builders
    for build in (m.GCN, m.multi_view_dgl_model):
        torch.manual_seed(5)
        a = build(_opt(gcn_mode=mode, compress_gcn=True, multi_gcn=False)).state_dict()
        torch.manual_seed(5)
        b = build(_opt(gcn_mode=mode, compress_gcn=True, multi_gcn=False, gcn_attn_heads=2)).state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    m.GCNBlock(_opt(gcn_mode=mode, compress_gcn=True, multi_gcn=True, gcn_attn_heads=8))


@pytest.mark.parametrize("build", [m.GCN, m.GCNStack, m.multi_view_dgl_model],
                         ids=["GCN", "GCNStack", "multi_view_dgl_model"])
def test_the_option_is_checked_when_the_module_is_built(build):
    for mode in ("film_attn", "film_wattn"):
        for bad in (0, -1, 3, 16, 2.0, "2", True, None):
            with pytest.raises(ValueError, match="gcn_attn_heads"):
                build(_opt(gcn_mode=mode, compress_gcn=True, gcn_attn_heads=bad))
        for good in (1, 2, 4, 8):
            build(_opt(gcn_mode=mode, compress_gcn=True, gcn_attn_heads=good))
    for mode in ("film_mean", "film_sum", "copy_mean", "film_max"):
        build(_opt(gcn_mode=mode, compress_gcn=True, gcn_attn_heads=1))
        with pytest.raises(ValueError, match="gcn_attn_heads"):
            build(_opt(gcn_mode=mode, compress_gcn=True, gcn_attn_heads=2))
    with pytest.raises(ValueError, match="gcn_attn_heads"):
        build(_opt(compress_gcn=True, gcn_attn_heads=2))  # the default mode is film_mean
    # the refusals that were there stay: FP8 messages with the attention modes, confidence with max / attn
    with pytest.raises(ValueError, match="gcn_message_dtype"):
        build(_opt(gcn_mode="film_wattn", compress_gcn=True, gcn_attn_heads=2, gcn_message_dtype="fp8_e4m3"))
    with pytest.raises(ValueError, match="confidence"):
        build(_opt(gcn_mode="film_attn", compress_gcn=True, gcn_attn_heads=2, gcn_confidence=True))
    with pytest.raises(ValueError, match="confidence"):
        build(_opt(gcn_mode="film_max", compress_gcn=True, gcn_confidence=True))


def test_ops_check_heads_on_the_host_and_cpu_tensors_still_raise():
    g = m.complete_graph(3).csr("cpu")
    x = torch.randn(3, 4, 4, 4)
    gb = torch.rand(6, 4, 2)
    w = torch.rand(3, 4, 4)
    from mrp_gnn_amd import aggregate, compress
    for bad in (0, -1, 3, 8, 2.0, True):
        with pytest.raises(ValueError, match="heads"):
            m.film_attn(x, gb, g, heads=bad)
        with pytest.raises(ValueError, match="heads"):
            aggregate.film_attn_cat(x, gb, g, heads=bad)
        with pytest.raises(ValueError, match="heads"):
            aggregate.film_attn_residual(x, gb, g, heads=bad)
        with pytest.raises(ValueError, match="heads"):
            aggregate.film_attn_mix(x, gb, g, x, 0.5, heads=bad)
        with pytest.raises(ValueError, match="heads"):
            m.film_wattn(x, gb, w, g, heads=bad)
        with pytest.raises(ValueError, match="heads"):
            aggregate.film_wattn_cat(x, gb, w, g, heads=bad)
        with pytest.raises(ValueError, match="heads"):
            compress.film_compress(torch.nn.Conv2d(8, 4, 1), x, gb, g, 0, reducer="attn", heads=bad)
    with pytest.raises(ValueError, match="heads"):
        compress.film_compress(torch.nn.Conv2d(8, 4, 1), x, gb, g, 0, reducer="max", heads=2)
    assert aggregate._attn_scale(None, 16 // 4) == 0.5  # the default scale of a 4-head call on 16 channels
    for heads in (1, 2, 4):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.film_attn(x, gb, g, heads=heads)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.film_wattn(x, gb, w, g, heads=heads)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.film_attn_forward_into(x, gb, g, 0, torch.empty_like(x), heads=heads)
        attn = torch.rand((6, 16) if heads == 1 else (heads, 6, 16))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.film_attn_backward(x, x, gb, attn, g, 0, True, True, heads=heads)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.film_wattn_backward(x, x, gb, w, attn, attn, g, 0, True, True, True, heads=heads)
