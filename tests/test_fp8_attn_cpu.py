"""CPU: the FP8 receiver-side operators of the max and attention reducers (``film_max_q`` / ``film_max_fq``,
``film_attn_q``, ``film_wattn_q``, ``GCN.forward_received`` / ``forward_cat_received``): their argument and
grad-mode errors, which need no GPU; the refusals of ``gcn_message_dtype``, which stay; and the teeth of the
split-query check of tests/test_gpu_fp8_attn.py — the float64 reference with the query apart from the messages
is ``attn_cases.reference`` when the two coincide, and a kernel that took the dequantised messages for the query
would miss it by more than a hundred times the bar on the very inputs the GPU test uses."""
import types

import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import aggregate
import attn_cases as ac
import attnq_cases as aq
import half_cases as hc
from conftest import rel_err

TOL = 1e-5  # tests/test_gpu_film_attn.py's bar


def _opt(**kw):
    return types.SimpleNamespace(feature_dim=8, **kw)


def _inputs():
    g = hc._frames([3], 1)
    x = torch.randn(3, 8, 4, 4)
    xq, s = m.quantize_features(x)
    z = torch.randn(g.num_edges(), 8, 2)
    return g, g.csr(torch.device("cpu")), x, xq, s, z


def test_exports():
    for name in ("film_max_q", "film_max_q_forward_into", "film_max_fq", "film_attn_q", "film_attn_q_forward_into",
                 "film_wattn_q", "film_wattn_q_forward_into"):
        assert callable(getattr(m, name)) and getattr(aggregate, name) is getattr(m, name)
    assert callable(m.GCN.forward_received) and callable(m.GCN.forward_cat_received)


def test_argument_errors_need_no_gpu():
    g, csr, x, xq, s, z = _inputs()
    w = torch.ones(3, 4, 4)
    with pytest.raises(TypeError):
        m.film_max_q(x, s, z, csr)  # not FP8
    with pytest.raises(TypeError):
        m.film_max_q(xq, s, z, csr, out_dtype=torch.float8_e5m2)  # FP8 outputs are not provided
    with pytest.raises(TypeError):
        m.film_attn_q(x, x, s, z, csr)  # messages not FP8
    with pytest.raises(TypeError):
        m.film_wattn_q(x, x.to(torch.bfloat16), s, z, w, csr)
    with pytest.raises(ValueError):
        m.film_attn_q(xq, xq, s, z, csr)  # own features must be fp32 / bf16 / fp16
    with pytest.raises(ValueError):
        m.film_attn_q(x[:, :4], xq, s, z, csr)  # x and xq differ in shape
    with pytest.raises(ValueError):
        m.film_attn_q(x[:2], xq[:2], s[:2], z, csr)  # node count
    for heads in (0, 3, True, 2.0):
        with pytest.raises(ValueError):
            m.film_attn_q(x, xq, s, z, csr, heads=heads)
        with pytest.raises(ValueError):
            m.film_wattn_q(x, xq, s, z, w, csr, heads=heads)
    with pytest.raises(ValueError):
        m.film_attn_q(x, xq, s, z, csr, scale=float("inf"))
    with pytest.raises(ValueError):
        m.film_attn_q(x, xq, torch.ones(3, 5), z, csr)  # scale neither (N,), (N, 1) nor (N, C)
    with pytest.raises(ValueError):
        m.film_max_q(xq, torch.ones(2), z, csr)
    with pytest.raises(ValueError):
        m.film_wattn_q(x, xq, s, z, None, csr)  # no maps
    with pytest.raises(ValueError):
        m.film_max_q(xq, s, z, None)  # no in-degree bound
    with pytest.raises(ValueError):
        m.film_max_q_forward_into(xq, s, z, csr, torch.empty(3, 8, 4, 5))
    # host-side checks passed: what remains is the device (there is no CPU fallback)
    for call in (lambda: m.film_max_q(xq, s, z, csr), lambda: m.film_attn_q(x, xq, s, z, csr, heads=2),
                 lambda: m.film_wattn_q(x, xq, None, z, w, csr), lambda: m.film_max_fq(x, z, csr)):
        with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
            call()


def test_inference_ops_refuse_to_drop_a_gradient():
    g, csr, x, xq, s, z = _inputs()
    w = torch.ones(3, 4, 4)
    zg, xg, wg = z.clone().requires_grad_(True), x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    for call in (lambda: m.film_max_q(xq, s, zg, csr), lambda: m.film_attn_q(xg, xq, s, z, csr),
                 lambda: m.film_attn_q(x, xq, s, zg, csr), lambda: m.film_wattn_q(x, xq, s, z, wg, csr),
                 lambda: m.film_wattn_q(x, xq, s.clone().requires_grad_(True), z, w, csr)):
        with pytest.raises(RuntimeError, match="inference op"):
            call()
        with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):  # fine without grad mode: on to the device
            call()


@pytest.mark.parametrize("mode", ["film_mean", "film_sum", "copy_mean", "film_max", "film_attn", "film_wattn"])
def test_forward_received_errors(mode):
    g, csr, x, xq, s, z = _inputs()
    gcn = m.GCN(_opt(gcn_mode=mode))
    for call in (gcn.forward_received, gcn.forward_cat_received):
        with pytest.raises(RuntimeError, match="inference-only"):
            call(g, x, xq, s)
        with torch.no_grad():
            with pytest.raises(ValueError):
                call(g, x[:, :4], xq, s)
            if mode != "film_wattn":
                with pytest.raises(ValueError, match="weights"):
                    call(g, x, xq, s, weights=torch.ones(3, 4, 4))
            with pytest.raises(RuntimeError, match="GPU"):
                call(g, x, xq, s)
    with torch.no_grad(), pytest.raises(ValueError, match="gcn_return"):
        m.GCN(_opt(gcn_mode=mode, gcn_return="input")).forward_received(g, x, xq, s)


def test_message_dtype_refusals_stay():
    """``opt.gcn_message_dtype`` still refuses the max and attention reducers: at build for film_wattn and with
    gcn_confidence, at forward for film_max / film_attn."""
    g, csr, x, xq, s, z = _inputs()
    with pytest.raises(ValueError, match="gcn_message_dtype"):
        m.GCN(_opt(gcn_message_dtype="fp8_e4m3", gcn_mode="film_wattn"))
    with pytest.raises(ValueError):
        m.GCN(_opt(gcn_message_dtype="fp8_e4m3", gcn_confidence=True))
    for mode in ("film_max", "film_attn"):
        gcn = m.GCN(_opt(gcn_message_dtype="fp8_e5m2", gcn_mode=mode))
        for call in (lambda: gcn(g, x), lambda: gcn.forward_cat(g, x), lambda: gcn.forward_residual(g, x)):
            with pytest.raises(ValueError, match="gcn_message_dtype"):
                call()
    with pytest.raises(ValueError):
        m.GCN(_opt(gcn_mode="film_max", gcn_confidence=True))


# ---- the teeth of the split-query check -----------------------------------------------------------------------
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("name", list(aq.GRAPHS))
def test_split_reference_with_query_equal_messages_is_the_existing_reference(name, heads):
    g, q, xq, s, xh, z, w = aq.operands(name, "e4m3")
    out, attn = aq.reference(g, xh, xh, z, logits=True, heads=heads)
    Ch = aq.C // heads
    for k in range(heads):
        sl = slice(k * Ch, (k + 1) * Ch)
        r_out, r_attn, _, _ = ac.reference(g, xh[:, sl], z[:, sl], logits=True, dtype=torch.float64)
        assert torch.equal(out[:, sl], r_out)
        assert torch.equal(attn if heads == 1 else attn[k], r_attn)


@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("fmt", aq.FORMATS)
@pytest.mark.parametrize("name", list(aq.GRAPHS))
def test_quantised_query_misses_the_reference_by_100_bars(name, fmt, heads):
    """The defect "the kernel used x^ as the query": on the GPU test's own inputs (a query drawn independently of
    the messages) it is at least 100 x the bar away from the true reference, in out and in the weights."""
    g, q, xq, s, xh, z, w = aq.operands(name, fmt)
    out, attn = aq.reference(g, q, xh, z, logits=True, heads=heads)
    bad_out, bad_attn = aq.reference(g, xh, xh, z, logits=True, heads=heads)
    e_out, e_attn = rel_err(bad_out.numpy(), out.numpy()), rel_err(bad_attn.numpy(), attn.numpy())
    print(name, fmt, heads, "out", e_out, "attn", e_attn, "bar", TOL)
    assert e_out >= 100 * TOL and e_attn >= 100 * TOL
