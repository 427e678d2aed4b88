"""CPU: the FP8 quantiser (``quantize_features`` / ``dequantize_features``), its error model, what quantised
messages cost the aggregate (float64 oracle), the teeth of the GPU decode-table test, and the model options
``gcn_message_dtype`` / ``gcn_message_scale``.  Bars: ``fp8_cases``' docstring."""
import types

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import aggregate, models
import fp8_cases as fc
import half_cases as hc
import oracle

FMTS = list(fc.FORMATS)


def _features(seed, shape=(5, 6, 8, 8)):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen) * torch.logspace(-3, 2, shape[1])[None, :, None, None]
    x[0, 1] *= 1e-6  # a plane deep in the subnormal range of nothing: its own scale carries it
    return x


@pytest.mark.parametrize("per", ["channel", "node"])
@pytest.mark.parametrize("fmt", FMTS)
def test_quantize_shapes_dtypes_and_scale_rule(fmt, per):
    qdtype, _, fmax, _, _ = fc.FORMATS[fmt]
    x = _features(1)
    x[2, 3] = 0.0  # an all-zero plane
    if per == "node":
        x[4] = 0.0  # an all-zero node
    for xin in (x, x.to(torch.bfloat16), x.to(memory_format=torch.channels_last)):
        xq, s = m.quantize_features(xin, fmt, per)
        assert xq.dtype == qdtype and tuple(xq.shape) == tuple(x.shape) and xq.is_contiguous()
        assert s.dtype == torch.float32 and tuple(s.shape) == tuple(x.shape[:2]) and s.is_contiguous()
        assert not xq.requires_grad and not s.requires_grad
        assert bool(torch.isfinite(xq.float()).all())  # no NaN / inf code from finite features
        xf = xin.float()
        a = xf.abs().amax((2, 3)) if per == "channel" else xf.abs().amax((1, 2, 3))[:, None].expand(-1, x.shape[1])
        want = torch.where(a > 0, a / fmax, torch.ones_like(a))
        assert torch.equal(s, want)
        # the largest magnitude of every scaled group lands on +-FMAX exactly (it is x / (x / FMAX))
        top = xq.float().abs().amax((2, 3)) if per == "channel" else xq.float().abs().amax((1, 2, 3))[:, None]
        assert bool(((top == fmax) | (a == 0)).all() if per == "channel" else ((top == fmax) | (a[:, :1] == 0)).all())
        if per == "channel":
            assert float(s[2, 3]) == 1.0 and not bool(xq[2, 3].view(torch.uint8).any())  # scale 1, codes 0
        else:
            assert bool((s[4] == 1.0).all()) and not bool(xq[4].view(torch.uint8).any())
            assert bool((s == s[:, :1]).all())  # one scale per node, repeated
    assert torch.equal(m.dequantize_features(xq, s), xq.float() * s[:, :, None, None])
    assert torch.equal(m.dequantize_features(xq, s[:, 0]), xq.float() * s[:, :1, None, None])  # (N,) and (N, 1)
    assert torch.equal(m.dequantize_features(xq, None), xq.float())


def test_quantize_argument_errors():
    x = _features(2)
    with pytest.raises(ValueError):
        m.quantize_features(x, "e3m4")
    with pytest.raises(ValueError):
        m.quantize_features(x, "e4m3", per="pixel")
    with pytest.raises(ValueError):
        m.quantize_features(x[0], "e4m3")
    with pytest.raises(TypeError):
        m.dequantize_features(x, None)
    xq, s = m.quantize_features(x)
    with pytest.raises(ValueError):
        m.dequantize_features(xq, s[:, :2])
    e = m.quantize_features(x[:0])
    assert tuple(e[0].shape) == (0, 6, 8, 8) and tuple(e[1].shape) == (0, 6)


@pytest.mark.parametrize("per", ["channel", "node"])
@pytest.mark.parametrize("fmt", FMTS)
def test_quantisation_error_bound(fmt, per):
    """|x^ - x| <= u |x| + s m / 2 + 2^-22 |x| for every element."""
    _, _, _, u, sub = fc.FORMATS[fmt]
    for seed in (3, 4):
        x = _features(seed, (4, 6, 16, 16))
        xq, s = m.quantize_features(x, fmt, per)
        xh = m.dequantize_features(xq, s).double()
        xd, sd = x.double(), s.double()[:, :, None, None]
        bound = u * xd.abs() + sd * sub / 2 + 2.0 ** -22 * xd.abs()
        excess = float(((xh - xd).abs() - bound).max())
        assert excess <= 0.0, (fmt, per, seed, excess)


@pytest.mark.parametrize("mode", ["film_mean", "copy_mean"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("robots", [5, 8])
def test_aggregate_of_quantised_messages_stays_within_u(robots, fmt, mode):
    """gamma, beta in (0, 1) and a mean cannot amplify an input error: the float64 oracle on x^ stays within
    u max|x| of the oracle on x."""
    u = fc.FORMATS[fmt][3]
    g = hc._frames([robots, robots], 20 + robots)
    gen = torch.Generator().manual_seed(robots)
    x = torch.randn(g.num_nodes(), 6, 8, 8, generator=gen)
    gb = torch.sigmoid(torch.randn(g.num_edges(), 6, 2, generator=gen))
    src, dst = (t.numpy() for t in g.edges())
    xh = m.dequantize_features(*m.quantize_features(x, fmt))
    ref = oracle.film_aggregate(x.double(), gb.double(), src, dst, mode)
    got = oracle.film_aggregate(xh.double(), gb.double(), src, dst, mode)
    worst = float((got - ref).abs().max())
    print(f"{robots} robots {fmt} {mode}: worst {worst / float(x.abs().max()):.4f} max|x|, bound {u}")
    assert worst <= u * float(x.abs().max())


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_tables_ocp_against_fnuz(fmt):
    """The teeth of the GPU decode-table test: read as FNUZ, the same bytes mean something else in all but one
    code.  FNUZ's exponent bias is one larger, so every non-zero number halves; 0x80 is NaN instead of -0; the
    OCP NaN codes (and E5M2's infinities) are ordinary FNUZ numbers.  Only 0x00 agrees."""
    ocp, fnuz = fc.decode_ocp(fmt), fc.decode_fnuz(fmt)
    same = (ocp == fnuz) | (torch.isnan(ocp) & torch.isnan(fnuz))
    differing = int((~same).sum())
    assert differing == 255 and bool(same[0])
    # torch's OCP table itself: the special codes the header names
    if fmt == "e4m3":
        assert int(torch.isnan(ocp).sum()) == 2 and not bool(torch.isinf(ocp).any())
        assert bool(torch.isnan(ocp[0x7F])) and bool(torch.isnan(ocp[0xFF])) and float(ocp[0x7E]) == 448.0
        assert float(ocp[1]) == 2.0 ** -9
    else:
        assert int(torch.isinf(ocp).sum()) == 2 and int(torch.isnan(ocp).sum()) == 6
        assert float(ocp[0x7C]) == float("inf") and float(ocp[0x7B]) == 57344.0 and float(ocp[1]) == 2.0 ** -16
        # the `byte << 8` reading: an E5M2 code is the high byte of the fp16 with the same value
        f16 = (fc.all_codes().to(torch.int32) << 8).to(torch.int16).view(torch.float16).float()
        assert bool(((f16 == ocp) | (torch.isnan(f16) & torch.isnan(ocp))).all())
    if hasattr(torch, "float8_e4m3fnuz"):  # torch's own FNUZ tables agree with the restatement above
        t = fc.all_codes().view(torch.float8_e4m3fnuz if fmt == "e4m3" else torch.float8_e5m2fnuz).float()
        assert bool(((t == fnuz) | (torch.isnan(t) & torch.isnan(fnuz))).all())


# ---- model options --------------------------------------------------------------------------------------------
def _opt(**kw):
    return types.SimpleNamespace(feature_dim=8, **kw)


def test_unknown_option_values_raise_when_the_module_is_built():
    for kw in (dict(gcn_message_dtype="fp8"), dict(gcn_message_dtype="int8"), dict(gcn_message_dtype="e4m3"),
               dict(gcn_message_dtype="fp8_e4m3", gcn_message_scale="pixel")):
        with pytest.raises(ValueError):
            m.GCN(_opt(**kw))
        with pytest.raises(ValueError):
            m.GCNStack(_opt(gcn_layers=2, gcn_combine="residual", **kw))
        with pytest.raises(ValueError):
            models.multi_view_dgl_model(_opt(compress_gcn=True, multi_gcn=False, **kw))
    for dt in ("fp8_e4m3", "fp8_e5m2"):
        for per in ("channel", "node"):
            assert models.message_format(_opt(gcn_message_dtype=dt, gcn_message_scale=per)) == (dt[4:], per)
    assert models.message_format(_opt()) == (None, "channel")


def test_default_leaves_construction_and_state_dict_untouched():
    torch.manual_seed(0)
    plain = m.GCNStack(_opt(gcn_layers=2, gcn_combine="cat_compress"))
    torch.manual_seed(0)
    none = m.GCNStack(_opt(gcn_layers=2, gcn_combine="cat_compress", gcn_message_dtype=None))
    torch.manual_seed(0)
    fp8 = m.GCNStack(_opt(gcn_layers=2, gcn_combine="cat_compress", gcn_message_dtype="fp8_e4m3"))
    for other in (none, fp8):  # the option adds no parameter and draws no random number
        assert list(other.state_dict()) == list(plain.state_dict())
        assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), other.state_dict().values()))
    fp8.load_state_dict(plain.state_dict())


@pytest.mark.parametrize("kw", [dict(gcn_mode="film_max"), dict(gcn_mode="film_attn"), dict(gcn_return="input")])
def test_message_dtype_with_max_attn_or_input_raises_at_forward(kw):
    gcn = m.GCN(_opt(gcn_message_dtype="fp8_e5m2", **kw))  # building is fine
    g = hc._frames([3], 1)
    x = torch.randn(3, 8, 4, 4)
    for call in (lambda: gcn(g, x), lambda: gcn.forward_cat(g, x), lambda: gcn.forward_residual(g, x),
                 lambda: gcn.forward_mix(g, x, x, 0.1),
                 lambda: gcn.forward_cat_compress(g, x, torch.nn.Conv2d(16, 8, 1))):
        with pytest.raises(ValueError, match="gcn_message_dtype"):
            call()


def test_inference_op_argument_errors_need_no_gpu():
    g = hc._frames([3], 1)
    x = torch.randn(3, 8, 4, 4)
    with pytest.raises(TypeError):
        aggregate.film_mean_q(x, None, None, None)  # not FP8
    with pytest.raises(TypeError):
        aggregate.film_mean_q(x.to(torch.bfloat16), None, None, None)
    xq, s = m.quantize_features(x)
    with pytest.raises(TypeError):
        aggregate.film_mean_q(xq, s, None, None, out_dtype=torch.float8_e4m3fn)  # FP8 outputs are not provided
    with pytest.raises(TypeError):
        aggregate.film_mean(xq, None, None)  # the existing op still rejects FP8 features
