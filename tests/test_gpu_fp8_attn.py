"""GPU: FP8 messages for the max and attention reducers, receiver side (``mrp_film_max_fwd_q``,
``mrp_film_attn_fwd_q``, ``mrp_film_wattn_fwd_q``; ``aggregate.film_max_q`` / ``film_attn_q`` / ``film_wattn_q``;
``GCN.forward_received``).  Every quantisation is torch's cast on the CPU and the bytes are uploaded
(tests/attnq_cases.py), ``film_max_fq`` excepted: it is the route that quantises on the device.

The contracts, for both formats, the three feature types T and every graph kind:

    film_max_q(xq, s, out_dtype=T)   == film_max(x^).to(T)                       bit for bit   (x^ = dequantised, fp32)
    film_attn_q(x^, xq, s)           == film_attn(x^), out and weights           bit for bit   (also heads, wattn, rate)
    film_attn_q(x_T, xq, s)          == film_attn_q(x_T.float(), xq, s).to(T), the same weights
    film_attn_q(q, xq, s)            within tests/test_gpu_film_attn.py's bar of the float64 split-query reference

and the properties only a split query has: x[u] is nobody's message (locality), a silent sender's codes reach
nothing."""
import types

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import aggregate
import attn_cases as ac
import attnq_cases as aq
import half_cases as hc
import wattn_cases as wc
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5  # tests/test_gpu_film_attn.py's bar
NAMES = list(aq.GRAPHS)
TYPES = [torch.float32, torch.bfloat16, torch.float16]
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def same_bits(a, b):
    """Equal bit for bit, except that NaNs need only be NaNs in the same places."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    eq = a.view(INT_VIEW[a.dtype]) == b.view(INT_VIEW[b.dtype])
    return bool(torch.equal(na, nb) and (eq | na).all())


def dev_operands(dev, name, fmt, plane=aq.PLANE):
    g, q, xq, s, xh, z, w = aq.operands(name, fmt, plane)
    return g, g.csr(dev), q.to(dev), xq.view(torch.uint8).to(dev).view(xq.dtype), s.to(dev), xh.to(dev), z.to(dev), \
        w.to(dev)


# ---- 1: the max ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", aq.FORMATS)
@pytest.mark.parametrize("name", NAMES)
def test_max_equals_the_fp32_operator_on_dequantised_messages(cuda_device, name, fmt):
    g, csr, q, xq, s, xh, z, w = dev_operands(cuda_device, name, fmt)
    with torch.no_grad():
        want = m.film_max(xh, z, csr, logits=True)
        before = aggregate.PATH_COUNTS["max_fwd_q_" + fmt]
        for T in TYPES:
            got = m.film_max_q(xq, s, z, csr, logits=True, out_dtype=T)
            assert got.dtype == T and same_bits(got, want.to(T)), T
        assert aggregate.PATH_COUNTS["max_fwd_q_" + fmt] == before + 3
        # a plane of 25 pixels, no scales, gamma / beta given
        g2, csr2, _, xq2, _, xh2, z2, _ = dev_operands(cuda_device, name, fmt, aq.SMALL_PLANE)
        gb2 = torch.sigmoid(z2)
        assert same_bits(m.film_max_q(xq2, None, gb2, csr2, out_dtype=torch.float32),
                         m.film_max(xq2.float(), gb2, csr2))


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("fmt", aq.FORMATS)
def test_max_fake_quant_route_gives_the_same_forward_bits(cuda_device, fmt, T):
    g, csr, q, xq, s, xh, z, w = dev_operands(cuda_device, "general_csr", fmt)
    x = q.to(T).requires_grad_(True)
    zz = z.clone().requires_grad_(True)
    out = m.film_max_fq(x, zz, csr, fmt, logits=True)
    with torch.no_grad():
        want = m.film_max_q(*m.quantize_features(x, fmt), zz, csr, logits=True, out_dtype=T)
    assert out.dtype == T and same_bits(out, want)
    out.float().sum().backward()  # the straight-through route is differentiable
    assert x.grad is not None and zz.grad is not None and bool(torch.isfinite(x.grad.float()).all())


# ---- 2: tied to the existing kernels ---------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("fmt", aq.FORMATS)
@pytest.mark.parametrize("name", NAMES)
def test_attention_with_dequantised_query_is_the_existing_operator(cuda_device, name, fmt, heads):
    g, csr, q, xq, s, xh, z, w = dev_operands(cuda_device, name, fmt)
    key = ("_fwd_q_" if heads == 1 else "_fwd_q_mh_") + fmt
    before = aggregate.PATH_COUNTS["attn" + key], aggregate.PATH_COUNTS["wattn" + key]
    with torch.no_grad():
        out, attn = m.film_attn_q(xh, xq, s, z, csr, logits=True, heads=heads, return_weights=True)
        r_out, r_attn = m.film_attn(xh, z, csr, logits=True, heads=heads, return_weights=True)
        assert same_bits(out, r_out) and same_bits(attn, r_attn)
        wo, wro = torch.empty_like(xh), torch.empty_like(xh)
        wa, wr = m.film_wattn_q_forward_into(xh, xq, s, z, w, csr, wo, logits=True, heads=heads, rate=True)
        ra, rr = m.film_wattn_forward_into(xh, z, w, csr, aggregate._lib.GB_LOGITS, wro, heads=heads, rate=True)
        assert same_bits(wo, wro) and same_bits(wa, ra) and same_bits(wr, rr)
    assert (aggregate.PATH_COUNTS["attn" + key], aggregate.PATH_COUNTS["wattn" + key]) == (before[0] + 1, before[1] + 1)


@pytest.mark.parametrize("fmt", aq.FORMATS)
def test_nan_codes_propagate_as_in_the_existing_operator(cuda_device, fmt):
    """A NaN code in one (node, channel, pixel): NaNs in the same places as film_attn(x^), all else bit-equal."""
    g, csr, q, xq, s, xh, z, w = dev_operands(cuda_device, "complete8", fmt)
    codes = xq.view(torch.uint8).clone()
    codes[3, 7, 2, 5] = aq.NAN_CODE[fmt]
    xq2 = codes.view(xq.dtype)
    xh2 = m.dequantize_features(xq2, s)
    assert int(torch.isnan(xh2).sum()) == 1
    with torch.no_grad():
        out, attn = m.film_attn_q(xh2, xq2, s, z, csr, logits=True, return_weights=True)
        r_out, r_attn = m.film_attn(xh2, z, csr, logits=True, return_weights=True)
        assert same_bits(out, r_out) and same_bits(attn, r_attn) and bool(torch.isnan(out).any())
        # with a clean query the NaN still reaches exactly pixel (2, 5) of node 3's listeners, in out
        out2 = m.film_attn_q(xh, xq2, s, z, csr, logits=True)
    nan = torch.isnan(out2)
    assert bool(nan.any()) and not bool(nan[3].any()) and not bool(nan[8:].any())
    rest = nan.clone()
    rest[:, :, 2, 5] = False
    assert not bool(rest.any())


# ---- 3: the 16-bit contract ------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_sixteen_bit_query_is_widened_exactly_and_out_rounded_once(cuda_device, name, heads, T):
    fmt = "e4m3" if heads == 1 else "e5m2"
    g, csr, q, xq, s, xh, z, w = dev_operands(cuda_device, name, fmt)
    qT = q.to(T)
    with torch.no_grad():
        out, attn = m.film_attn_q(qT, xq, s, z, csr, logits=True, heads=heads, return_weights=True)
        r_out, r_attn = m.film_attn_q(qT.float(), xq, s, z, csr, logits=True, heads=heads, return_weights=True)
        assert out.dtype == T and same_bits(out, r_out.to(T)) and same_bits(attn, r_attn)
        wo, wa = m.film_wattn_q(qT, xq, s, z, w, csr, logits=True, heads=heads, return_weights=True)
        ro, ra = m.film_wattn_q(qT.float(), xq, s, z, w, csr, logits=True, heads=heads, return_weights=True)
        assert same_bits(wo, ro.to(T)) and same_bits(wa, ra)


# ---- 4: the split query against float64 ------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("fmt", aq.FORMATS)
@pytest.mark.parametrize("name", NAMES)
def test_split_query_against_float64(cuda_device, name, fmt, heads):
    """The query is drawn independently of the messages; tests/test_fp8_attn_cpu.py shows that a kernel scoring
    with x^ instead misses this reference by more than 100 x the bar on these inputs."""
    g, csr, q, xq, s, xh, z, w = dev_operands(cuda_device, name, fmt)
    cg, cq, _, _, cxh, cz, _ = aq.operands(name, fmt)
    ref_out, ref_attn = aq.reference(cg, cq, cxh, cz, logits=True, heads=heads)
    with torch.no_grad():
        out, attn = m.film_attn_q(q, xq, s, z, csr, logits=True, heads=heads, return_weights=True)
    e_out = rel_err(out.cpu().numpy(), ref_out.numpy())
    e_attn = rel_err(attn.cpu().numpy(), ref_attn.numpy())
    print(name, fmt, heads, "out", e_out, "attn", e_attn, "bar", TOL)
    assert e_out <= TOL and e_attn <= TOL


def test_split_query_small_plane_scale_and_plain_gb(cuda_device):
    """P = 25 < 64, an explicit scale, gamma / beta given (no logits), scales per node."""
    g, csr, q, xq, s, xh, z, w = dev_operands(cuda_device, "general_csr", "e5m2", aq.SMALL_PLANE)
    cg, cq, cxq, cs, _, cz, _ = aq.operands("general_csr", "e5m2", aq.SMALL_PLANE)
    s1 = s[:, :1].contiguous()  # (N, 1)
    cxh = m.dequantize_features(cxq, cs[:, :1])
    gb = torch.sigmoid(z)
    ref_out, ref_attn = aq.reference(cg, cq, cxh, torch.sigmoid(cz), scale=0.37, heads=2)
    with torch.no_grad():
        out, attn = m.film_attn_q(q, xq, s1, gb, csr, scale=0.37, heads=2, return_weights=True)
        out1 = m.film_attn_q(q, xq, s1[:, 0], gb, csr, scale=0.37, heads=2)  # (N,)
    assert rel_err(out.cpu().numpy(), ref_out.numpy()) <= TOL and rel_err(attn.cpu().numpy(), ref_attn.numpy()) <= TOL
    assert same_bits(out, out1)


# ---- 5: locality -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_own_features_are_nobodys_message(cuda_device, name, heads):
    """Changing x[u] changes out[v] for no v != u, bit for bit — gated or not."""
    g, csr, q, xq, s, xh, z, w = dev_operands(cuda_device, name, "e4m3")
    u = 1
    q2 = q.clone()
    q2[u] = 3.0 * q[u] + 1.0
    others = [v for v in range(q.shape[0]) if v != u]
    with torch.no_grad():
        a, b = (m.film_attn_q(t, xq, s, z, csr, logits=True, heads=heads) for t in (q, q2))
        c, d = (m.film_wattn_q(t, xq, s, z, w, csr, logits=True, heads=heads) for t in (q, q2))
    assert same_bits(a[others], b[others]) and same_bits(c[others], d[others])
    assert not same_bits(a[u], b[u])  # u itself has in-edges in every graph here: its own output moves


# ---- 6: heads --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", aq.FORMATS)
@pytest.mark.parametrize("name", NAMES)
def test_head_k_is_the_single_head_operator_on_slice_k(cuda_device, name, fmt):
    g, csr, q, xq, s, xh, z, w = dev_operands(cuda_device, name, fmt)
    H, Ch = 2, aq.C // 2
    with torch.no_grad():
        out, attn = m.film_attn_q(q, xq, s, z, csr, logits=True, heads=H, return_weights=True)
        wout, wattn = m.film_wattn_q(q, xq, s, z, w, csr, logits=True, heads=H, return_weights=True)
        for k in range(H):
            sl = slice(k * Ch, (k + 1) * Ch)
            args = (q[:, sl], xq[:, sl], s[:, sl], z[:, sl])
            o, a = m.film_attn_q(*args, csr, logits=True, return_weights=True)
            assert same_bits(out[:, sl], o) and same_bits(attn[k], a), k
            o, a = m.film_wattn_q(*args, w, csr, logits=True, return_weights=True)
            assert same_bits(wout[:, sl], o) and same_bits(wattn[k], a), k
        # an E4M3 / E5M2 NaN code in head 1 leaves head 0 untouched
        codes = xq.view(torch.uint8).clone()
        codes[0, Ch + 3, 1, 1] = aq.NAN_CODE[fmt]
        out2, attn2 = m.film_attn_q(q, codes.view(xq.dtype), s, z, csr, logits=True, heads=H, return_weights=True)
    assert same_bits(out2[:, :Ch], out[:, :Ch]) and same_bits(attn2[0], attn[0])
    assert not bool(torch.isnan(out2[:, :Ch]).any())


# ---- 7: gating -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_all_ones_map_gives_the_ungated_bits(cuda_device, name, heads):
    g, csr, q, xq, s, xh, z, w = dev_operands(cuda_device, name, "e5m2")
    with torch.no_grad():
        a, aa = m.film_attn_q(q, xq, s, z, csr, logits=True, heads=heads, return_weights=True)
        b, ba = m.film_wattn_q(q, xq, s, z, torch.ones_like(w), csr, logits=True, heads=heads, return_weights=True)
    assert same_bits(a, b) and same_bits(aa, ba)


@pytest.mark.parametrize("name", ["complete5", "complete8", "knn16_4"])
def test_silent_robots_are_the_graph_without_their_out_edges(cuda_device, name):
    """A 0 / 1 map per robot: the bits of the compacted graph; the silent robots' codes (all NaN) reach nothing."""
    fmt = "e4m3"
    g, csr, q, xq, s, xh, z, w = dev_operands(cuda_device, name, fmt)
    n = g.num_nodes()
    silent = np.zeros(n, bool)
    silent[[1, n - 2]] = True
    w01 = torch.ones_like(w)
    w01[torch.from_numpy(silent).to(w.device)] = 0.0
    codes = xq.view(torch.uint8).clone()
    codes[torch.from_numpy(silent).to(w.device)] = aq.NAN_CODE[fmt]
    xq_nan = codes.view(xq.dtype)
    gc = wc.compacted(g, silent)
    with torch.no_grad():
        want, want_attn = m.film_attn_q(q, xq, s, z, gc.csr(cuda_device), logits=True, return_weights=True)
        got, got_attn = m.film_wattn_q(q, xq, s, z, w01, csr, logits=True, return_weights=True)
        got_nan, attn_nan = m.film_wattn_q(q, xq_nan, s, z, w01, csr, logits=True, return_weights=True)
    assert same_bits(got, want) and same_bits(got_attn, want_attn)
    assert not bool(torch.isnan(got_nan).any()) and same_bits(got_nan, got) and same_bits(attn_nan, got_attn)


# ---- 8: layout -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("name", ["complete5", "general_csr"])
def test_strided_inputs_and_cat_buffer_output(cuda_device, name, T):
    g, csr, q, xq, s, xh, z, w = dev_operands(cuda_device, name, "e4m3")
    n, C, H, W = q.shape
    plane = C * H * W
    qT = q.to(T)
    # node strides larger than C * P on the codes and on the own features
    xq_buf = torch.zeros((n, plane + 37), device=q.device, dtype=torch.uint8)
    xq_buf[:, :plane] = xq.view(torch.uint8).reshape(n, plane)
    xq_s = xq_buf[:, :plane].view(xq.dtype).view(n, C, H, W)
    q_buf = torch.zeros((n, plane + 11), device=q.device, dtype=T)
    q_buf[:, :plane] = qT.reshape(n, plane)
    q_s = q_buf[:, :plane].view(n, C, H, W)
    assert xq_s.stride(0) == plane + 37 and q_s.stride(0) == plane + 11
    sentinel = 12345.0 if T != torch.float16 else 1234.0
    with torch.no_grad():
        for heads in (1, 2):
            dense, dattn = m.film_attn_q(qT, xq, s, z, csr, logits=True, heads=heads, return_weights=True)
            cat = torch.full((n, 2 * C, H, W), sentinel, device=q.device, dtype=T)
            attn = m.film_attn_q_forward_into(q_s, xq_s, s, z, csr, cat[:, C:], logits=True, heads=heads)
            assert same_bits(cat[:, C:], dense) and same_bits(attn, dattn)
            assert bool((cat[:, :C] == sentinel).all())
            wdense = m.film_wattn_q(qT, xq, s, z, w, csr, logits=True, heads=heads)
            cat.fill_(sentinel)
            m.film_wattn_q_forward_into(q_s, xq_s, s, z, w, csr, cat[:, C:], logits=True, heads=heads)
            assert same_bits(cat[:, C:], wdense) and bool((cat[:, :C] == sentinel).all())
        mdense = m.film_max_q(xq, s, z, csr, logits=True, out_dtype=T)
        cat = torch.full((n, 2 * C, H, W), sentinel, device=q.device, dtype=T)
        m.film_max_q_forward_into(xq_s, s, z, csr, cat[:, C:], logits=True)
        assert same_bits(cat[:, C:], mdense) and bool((cat[:, :C] == sentinel).all())
        # channels_last codes and own features: made NCHW first
        cl = m.film_attn_q(qT.to(memory_format=torch.channels_last), xq.view(torch.uint8).to(
            memory_format=torch.channels_last).view(xq.dtype), s, z, csr, logits=True)
        assert same_bits(cl, m.film_attn_q(qT, xq, s, z, csr, logits=True))


# ---- 9: the model ----------------------------------------------------------------------------------------------
def _opt(C, **kw):
    return types.SimpleNamespace(feature_dim=C, **kw)


@pytest.mark.parametrize("fmt", aq.FORMATS)
@pytest.mark.parametrize("mode", ["film_mean", "film_sum", "copy_mean"])
def test_model_mean_modes_equal_the_simulated_link(cuda_device, mode, fmt):
    dev = cuda_device
    g = hc._frames([5, 8], 3).to(dev)
    torch.manual_seed(0)
    x = torch.randn(13, 12, 9, 9, device=dev).to(torch.bfloat16)
    torch.manual_seed(1)
    sim = m.GCN(_opt(12, gcn_mode=mode, gcn_message_dtype="fp8_" + fmt)).to(dev)
    rec = m.GCN(_opt(12, gcn_mode=mode)).to(dev)
    rec.load_state_dict(sim.state_dict())
    before = aggregate.PATH_COUNTS["fwd_q_" + fmt]
    with torch.no_grad():
        xq, s = m.quantize_features(x, fmt)
        want = sim(g, x)
        got = rec.forward_received(g, x, xq, s)
        cat = rec.forward_cat_received(g, x, xq, s)
    assert got.dtype == x.dtype and same_bits(got, want)
    assert same_bits(cat, torch.cat((x, got), 1))
    assert aggregate.PATH_COUNTS["fwd_q_" + fmt] == before + 3


@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode,heads", [("film_max", 1), ("film_attn", 1), ("film_attn", 2), ("film_wattn", 1),
                                        ("film_wattn", 2)])
def test_model_max_and_attention_modes_equal_the_operators(cuda_device, mode, heads, T):
    dev = cuda_device
    fmt = "e4m3"
    g = hc._frames([5, 8], 3).to(dev)
    C = 12
    torch.manual_seed(0)
    x = torch.randn(13, C, 9, 9, device=dev).to(T)
    xq, s = (t.to(dev) for t in m.quantize_features(torch.randn(13, C, 9, 9), fmt))
    w = (torch.rand(13, 9, 9, device=dev) > 0.3).float() * torch.rand(13, 9, 9, device=dev)
    kw = dict(gcn_mode=mode, gcn_attn_scale=0.4)
    if heads > 1:
        kw["gcn_attn_heads"] = heads
    gcn = m.GCN(_opt(C, **kw)).to(dev)
    csr = g.csr(dev)
    counts = dict(aggregate.PATH_COUNTS)
    with torch.no_grad():
        z = gcn.edge_encoder.logits(g.edata["pose"])
        got = gcn.forward_received(g, x, xq, s)
        cat = gcn.forward_cat_received(g, x, xq, s)
        if mode == "film_max":
            want = m.film_max_q(xq, s, z, csr, logits=True, out_dtype=T)
            key = "max_fwd_q_" + fmt
        else:
            want = m.film_attn_q(x, xq, s, z, csr, logits=True, scale=0.4, heads=heads)
            key = ("attn_fwd_q_" if heads == 1 else "attn_fwd_q_mh_") + fmt
        assert got.dtype == T and same_bits(got, want) and same_bits(cat, torch.cat((x, want), 1))
        assert aggregate.PATH_COUNTS[key] == counts.get(key, 0) + 3
        if mode == "film_wattn":
            wkey = ("wattn_fwd_q_" if heads == 1 else "wattn_fwd_q_mh_") + fmt
            wbefore = aggregate.PATH_COUNTS[wkey]
            gotw = gcn.forward_received(g, x, xq, s, weights=w)
            catw = gcn.forward_cat_received(g, x, xq, s, weights=w)
            wantw = m.film_wattn_q(x, xq, s, z, w, csr, logits=True, scale=0.4, heads=heads)
            assert same_bits(gotw, wantw) and same_bits(catw, torch.cat((x, wantw), 1))
            assert not same_bits(gotw, got)
            assert aggregate.PATH_COUNTS[wkey] == wbefore + 3
