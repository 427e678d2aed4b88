"""The split-bf16 kernels' defining property — fp32 accuracy from six bf16 partial products per product
(``csrc/compress_split.hip``, ``csrc/encoder_split.hip``, ``csrc/encoder_split.hpp``) — as a hard gate:
on lattice operands whose three bf16 parts are known by construction, made sparse so that every output
is an fp32 value whatever the summation order (``tests/split_cases.py``), every kernel and form must
reproduce the float64 product BIT FOR BIT, and so must the fp32-MFMA ``hip`` path.  A dropped copy of
any of the six products, a swapped part in either operand, or the loss of either operand's third part
— in one tile form, one packed image or one ragged tail only — changes most outputs
(``tests/test_split_lattice_cpu.py`` pins that on the same operands without a GPU)."""
import pytest
import torch

import mrp_gnn_amd as m
import split_cases as sc
from mrp_gnn_amd.aggregate import _ptr
from split_cases import FUSED_FORMS, GEMM_FORMS, NT_FORMS
from split_cases import bwd_fused as _bwd_fused
from split_cases import bwd_split as _bwd_split
from split_cases import knobs as _knobs
from split_cases import stream as _stream

pytestmark = pytest.mark.gpu

PAIR = pytest.mark.parametrize("pairing", sc.PAIRINGS, ids=sc.pairing_id)


def _nchw(t, dev):
    """(n, C, P) CPU -> (n, C, 4, P / 4) on the device."""
    n, C, P = t.shape
    return t.view(n, C, 4, P // 4).to(dev)


def _ncp(t):
    return t.reshape(t.shape[0], t.shape[1], -1)


@pytest.mark.parametrize("form", list(GEMM_FORMS))
@pytest.mark.parametrize("n,C,P", sc.COMPRESS_SHAPES)
@PAIR
def test_compress_forward_and_data_gradient_exact(cuda_device, pairing, n, C, P, form):
    """``mrp_compress_fwd_split`` (W's packed image) and ``mrp_compress_bwd_data_split`` (the transposed
    pack): the A-side kind in the weight, the B-side kind in x / a / gy; with and without bias; and once
    more with x and a, and gx and ga, the two halves of cat buffers (node stride 2 C P)."""
    dev = cuda_device
    c = sc.compress_case(n, C, P, pairing)
    ref, ref0 = sc.compress_refs(c), sc.compress_refs(c, bias=False)
    w = c["w"].view(C, 2 * C, 1, 1).to(dev)
    b = c["b"].to(dev)
    x, a, gy = (_nchw(c[k], dev) for k in ("x", "a", "gy"))
    cat = torch.cat((x, a), 1)
    gcat = torch.full((n, 2 * C, 4, P // 4), float("nan"), device=dev)
    path, knobs = GEMM_FORMS[form]
    tag = f"{form} {sc.pairing_id(pairing)} n={n} C={C} P={P}"
    with _knobs(path, **knobs):
        before = m.compress.PATH_COUNTS["fwd_f32"], m.compress.PATH_COUNTS["dgrad_f32"]
        y = m.compress.compress_forward(w, b, x, a)
        y0 = m.compress.compress_forward(w, None, x, a)
        ycat = m.compress.compress_forward(w, b, cat[:, :C], cat[:, C:])
        gx, ga = m.compress.compress_backward_data(w, gy)
        m.compress.compress_backward_data(w, gy, gcat[:, :C], gcat[:, C:])
        assert m.compress.PATH_COUNTS["fwd_f32"] == before[0] + 3 and m.compress.PATH_COUNTS["dgrad_f32"] == before[1] + 2
    sc.assert_bit_equal(_ncp(y), ref["y"], f"y {tag}")
    sc.assert_bit_equal(_ncp(y0), ref0["y"], f"y without bias {tag}")
    sc.assert_bit_equal(_ncp(ycat), ref["y"], f"y from a cat buffer's halves {tag}")
    sc.assert_bit_equal(_ncp(gx), ref["gx"], f"gx {tag}")
    sc.assert_bit_equal(_ncp(ga), ref["ga"], f"ga {tag}")
    sc.assert_bit_equal(_ncp(gcat), torch.cat((ref["gx"], ref["ga"]), 1), f"[gx; ga] into a cat buffer {tag}")


#: weight-gradient shapes: n P = 96 (three 32-pixel stages, no split-K in the 32-k-stage form: workspace 0)
#: and n P = 256 (split-K: a non-zero workspace, the fixed-order sum of the partial tiles)
WGRAD_SHAPES = ((3, 64, 32), (8, 64, 32), (3, 256, 32))


@pytest.mark.parametrize("form", list(NT_FORMS))
@pytest.mark.parametrize("n,C,P", WGRAD_SHAPES)
@PAIR
def test_compress_weight_gradient_exact(cuda_device, pairing, n, C, P, form):
    """``mrp_compress_bwd_weight_split``, both operands split in the kernel (split_nt 3) or gy pre-split
    into a packed image (split_nt 4: ``split_rows`` + ``gemm_nt_psa``), with and without split-K; gbias
    against the exact row sums of gy; and ``mrp_compress_bwd_weight`` on the fp32 MFMA."""
    dev = cuda_device
    c = sc.compress_case(n, C, P, pairing)
    ref = sc.compress_refs(c)
    gy, x, a = (_nchw(c[k], dev) for k in ("gy_s", "xs", "as_"))
    path, knobs = NT_FORMS[form]
    tag = f"{form} {sc.pairing_id(pairing)} n={n} C={C} P={P}"
    with _knobs(path, **knobs) as lib:
        if form == "split_nt3":  # the query runs on the host: which shapes split K
            ws = lib.mrp_compress_bwd_weight_split_workspace(n, C, P)
            assert (ws > 0) == (n == 8), (tag, ws)
        elif form == "split_nt4":  # the image alone is 6 bytes per element of gy
            assert lib.mrp_compress_bwd_weight_split_workspace(n, C, P) >= 6 * C * n * P, tag
        before = m.compress.PATH_COUNTS["wgrad_f32"]
        gw, gb = m.compress.compress_backward_weight(gy, x, a)
        assert m.compress.PATH_COUNTS["wgrad_f32"] == before + 1
    sc.assert_bit_equal(gw.view(C, 2 * C), ref["gw"], f"gw {tag}")
    sc.assert_bit_equal(gb, ref["gb"], f"gbias {tag}")


@pytest.mark.parametrize("path", ["split", "hip"])
@PAIR
def test_compress_function_padded_exact(cuda_device, pairing, path):
    """C = 48, P = 15 through ``CompressFunction``: the same kernels on zero-padded operands — the zeros
    keep every output exact."""
    dev = cuda_device
    n, C, P = 3, 48, 15
    c = sc.compress_case(n, C, P, pairing, cover=False)
    qa, qb = sc.QUANTUM[pairing[0]], sc.QUANTUM[pairing[1]]
    cat = torch.cat((sc._rows(c["xs"]), sc._rows(c["as_"])), 0)
    tag = f"padded {path} {sc.pairing_id(pairing)}"
    # one gy serves both gradients here: sparse (the weight gradient's sums), and of a kind whose product
    # with the weight and with the activations stays within three parts
    kg = "two" if pairing == ("two", "two") else "bf16"
    gy_s = sc.lattice(kg, (n, C, P), 31) * (c["gy_s"] != 0)
    qg = sc.QUANTUM[kg]
    ry = sc.exact_product(c["w"], cat, qa, qb, c["b"], f"y {tag}")
    rg = sc.exact_product(c["w"].t().contiguous(), sc._rows(gy_s), qa, qg, None, f"gcat {tag}", most=False)
    rw = sc.exact_product(sc._rows(gy_s), cat.t().contiguous(), qg, qb, None, f"gw {tag}")
    w = c["w"].view(C, 2 * C, 1, 1).to(dev).requires_grad_(True)
    b = c["b"].to(dev).requires_grad_(True)
    x, a = (c[k].view(n, C, 3, 5).to(dev).requires_grad_(True) for k in ("xs", "as_"))
    with _knobs(path):
        y = m.compress.CompressFunction.apply(x, a, w, b)
        y.backward(gy_s.view(n, C, 3, 5).to(dev))
    unrow = lambda r, ch: r.view(ch, n, P).permute(1, 0, 2)  # noqa: E731
    sc.assert_bit_equal(_ncp(y), unrow(ry, C), f"y {tag}")
    sc.assert_bit_equal(_ncp(x.grad), unrow(rg, 2 * C)[:, :C], f"gx {tag}")
    sc.assert_bit_equal(_ncp(a.grad), unrow(rg, 2 * C)[:, C:], f"ga {tag}")
    sc.assert_bit_equal(w.grad.view(C, 2 * C), rw, f"gw {tag}")
    sc.assert_bit_equal(b.grad, sc._rows(gy_s).double().sum(1), f"gb {tag}")


# ---- the edge encoder -----------------------------------------------------------------------------------

VARIANT = pytest.mark.parametrize("variant", list(sc.ENCODER_VARIANTS))


def _encoder_dev(c, dev):
    t = {k: c[k].to(dev) for k in ("pose", "w1", "b1", "w2", "b2")}
    t["img"] = m.encoder._pack(t["w1"], t["b1"], t["w2"])
    return t


@pytest.mark.parametrize("waves", [1, 3, -1])
@pytest.mark.parametrize("E,C", sc.ENCODER_SHAPES)
@VARIANT
def test_encoder_forward_exact(cuda_device, variant, E, C, waves):
    """``mrp_edge_encoder_fwd_split`` with 4 waves (edge_split_v 1), 8 waves (3) and the per-shape choice:
    the three pairings rotated through (pose, W1) and through (h, W2)."""
    dev = cuda_device
    c = sc.encoder_case(E, C, variant)
    t = _encoder_dev(c, dev)
    z = torch.full((E, 2 * C), float("nan"), device=dev)
    with _knobs(edge_split_v=waves) as lib:
        m._lib.check(lib.mrp_edge_encoder_fwd_split(_ptr(t["pose"]), _ptr(t["img"]), _ptr(t["b2"]), E, C, _ptr(z),
                                                    _stream(dev)), "mrp_edge_encoder_fwd_split")
        torch.cuda.synchronize()
    sc.assert_bit_equal(z, c["z64"], f"z {variant} E={E} C={C} edge_split_v={waves}")


@pytest.mark.parametrize("allx", [0, 1])
@pytest.mark.parametrize("waves,C", [(1, 256), (1, 288), (3, 512), (3, 544)])
@pytest.mark.parametrize("variant", ["three.bf16/three.bf16", "-/two.two"])
def test_encoder_forward_exact_edge_allx(cuda_device, variant, waves, C, allx):
    """``edge_allx`` (every hidden block before z, where ``C / 32 <= 2 nwv`` lets them fit LDS) on and off, at
    the largest C that takes the form and the first above it, for 4 waves (nwv 4: C = 256 | 288) and 8 (512 |
    544): the same exact product either way (``test_encoder_forward_exact``'s check, one ragged edge tile)."""
    dev = cuda_device
    E = 33
    c = sc.encoder_case(E, C, variant)
    t = _encoder_dev(c, dev)
    z = torch.full((E, 2 * C), float("nan"), device=dev)
    with _knobs(edge_split_v=waves, edge_allx=allx) as lib:
        m._lib.check(lib.mrp_edge_encoder_fwd_split(_ptr(t["pose"]), _ptr(t["img"]), _ptr(t["b2"]), E, C, _ptr(z),
                                                    _stream(dev)), "mrp_edge_encoder_fwd_split")
        torch.cuda.synchronize()
    sc.assert_bit_equal(z, c["z64"], f"z {variant} E={E} C={C} edge_split_v={waves} edge_allx={allx}")


@pytest.mark.parametrize("waves", [1, 3])
@pytest.mark.parametrize("E,C", [(33, 32), (96, 96), (33, 608)])
@VARIANT
def test_encoder_training_forward_exact(cuda_device, variant, E, C, waves):
    """``mrp_edge_encoder_fwd_split_train``: z exact and h^T exact in rows of hT_stride > E whose padding
    (NaN before the call) stays untouched — every hidden block before z (C <= 64 x waves) and round by
    round (C = 608: 19 hidden blocks); ``mrp_edge_logits_fwd`` (fp32 MFMA) on the same h."""
    dev = cuda_device
    c = sc.encoder_case(E, C, variant)
    t = _encoder_dev(c, dev)
    stride = E + 7
    z = torch.full((E, 2 * C), float("nan"), device=dev)
    hT = torch.full((C, stride), float("nan"), device=dev)
    tag = f"{variant} E={E} C={C} edge_split_v={waves}"
    with _knobs(edge_split_v=waves) as lib:
        m._lib.check(lib.mrp_edge_encoder_fwd_split_train(_ptr(t["pose"]), _ptr(t["img"]), _ptr(t["b2"]), E, C, _ptr(z),
                                                          _ptr(hT), stride, _stream(dev)), "mrp_edge_encoder_fwd_split_train")
        torch.cuda.synchronize()
    sc.assert_bit_equal(z, c["z64"], f"z {tag}")
    sc.assert_bit_equal(hT[:, :E], c["h64"].t(), f"hT {tag}")
    assert bool(torch.isnan(hT[:, E:]).all()), f"hT's row padding was written ({tag})"
    z2 = m.encoder.logits_forward(hT[:, :E].t().contiguous(), t["w2"], t["b2"])
    sc.assert_bit_equal(z2, c["z64"], f"mrp_edge_logits_fwd {tag}")


def _bwd_dev(c, dev):
    t = {k: c[k].to(dev) for k in ("dz", "dz_d", "w2", "hT", "pose")}
    t["w2t"] = t["w2"].t().contiguous()
    return t


@pytest.mark.parametrize("E,C", sc.ENCODER_BWD_SHAPES)
@PAIR
def test_encoder_backward_split_exact(cuda_device, pairing, E, C):
    """``mrp_edge_encoder_bwd_split``: dh^T = W2^T dz^T and dW2 = dz^T h (db2 on the same pass) in one call,
    and each alone with the other output NULL (dh^T then from a dense dz); dz^T by ``_bwd_prep``."""
    dev = cuda_device
    c = sc.encoder_bwd_case(E, C, pairing)
    t = _bwd_dev(c, dev)
    lib = m.load_library()
    tag = f"{sc.pairing_id(pairing)} E={E} C={C}"
    dzT = torch.empty(2 * C, E, device=dev)
    m._lib.check(lib.mrp_edge_encoder_bwd_prep(_ptr(t["dz"]), E, C, _ptr(dzT), E, _stream(dev)), "mrp_edge_encoder_bwd_prep")
    assert torch.equal(dzT, t["dz"].t())
    new = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    dhT, dw2, db2 = new(C, E), new(2 * C, C), new(2 * C)
    _bwd_split(lib, dev, E, C, t["dz"], dzT, t["w2t"], t["hT"], dhT, dw2, db2)
    sc.assert_bit_equal(dhT, c["dhT"], f"dhT (both outputs) {tag}")
    sc.assert_bit_equal(dw2, c["dw2"], f"dW2 (both outputs) {tag}")
    sc.assert_bit_equal(db2, c["db2"], f"db2 (both outputs) {tag}")
    dhT = new(C, E)
    _bwd_split(lib, dev, E, C, t["dz_d"], None, t["w2t"], None, dhT, None, None)
    sc.assert_bit_equal(dhT, c["dhT_d"], f"dhT alone {tag}")
    dw2, db2 = new(2 * C, C), new(2 * C)
    _bwd_split(lib, dev, E, C, None, dzT, None, t["hT"], None, dw2, db2)
    sc.assert_bit_equal(dw2, c["dw2"], f"dW2 alone {tag}")
    sc.assert_bit_equal(db2, c["db2"], f"db2 alone {tag}")


@pytest.mark.parametrize("knobs", FUSED_FORMS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
@pytest.mark.parametrize("E,C", sc.ENCODER_BWD_SHAPES)
@pytest.mark.parametrize("pairing", sc.PAIRINGS + (("bf16", "two"),), ids=sc.pairing_id)
def test_encoder_backward_fused_exact(cuda_device, pairing, E, C, knobs):
    """``mrp_edge_encoder_bwd_fused``: dW2 and db2 exact in every pairing; dW1 and db1, which come after a
    second summation (over all edges, in fp32), in the coarse pairing (dz +-1, W2 two: dh^T a multiple of
    2^-10) where that sum stays exact too."""
    dev = cuda_device
    c = sc.encoder_bwd_case(E, C, pairing)
    t = _bwd_dev(c, dev)
    tag = f"{sc.pairing_id(pairing)} E={E} C={C} {knobs}"
    with _knobs(**knobs) as lib:
        dw1, db1, dw2, db2 = _bwd_fused(lib, dev, c, t)
    sc.assert_bit_equal(dw2, c["dw2"], f"dW2 {tag}")
    sc.assert_bit_equal(db2, c["db2"], f"db2 {tag}")
    if pairing == ("bf16", "two"):
        r1, rb1 = sc.encoder_dw1_refs(c)
        sc.assert_bit_equal(dw1, r1, f"dW1 {tag}")
        sc.assert_bit_equal(db1, rb1, f"db1 {tag}")


@pytest.mark.parametrize("E,C", sc.ENCODER_BWD_SHAPES + ((100, 32),))
@PAIR
def test_encoder_reductions_exact(cuda_device, pairing, E, C):
    """``mrp_edge_encoder_bwd_t`` (dW1, db1) and ``mrp_edge_encoder_bwd_pose`` fed lattice dh^T / h^T / pose /
    W1 directly, rows of dh^T and h^T with a stride above E."""
    dev = cuda_device
    c = sc.encoder_reduce_case(E, C, pairing)
    lib = m.load_library()
    tag = f"{sc.pairing_id(pairing)} E={E} C={C}"
    stride = E + 4
    pad = lambda x: torch.cat((x, torch.full((C, 4), float("nan"))), 1).to(dev)  # noqa: E731
    hT, dhT, dhT_p = pad(c["hT"]), pad(c["dhT"]), pad(c["dhT_p"])
    pose, w1 = c["pose"].to(dev), c["w1"].to(dev)
    dw1, db1 = torch.full((C, 9), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
    nbytes = max(int(lib.mrp_edge_encoder_bwd_t_workspace(E, C)), 4)
    ws = torch.empty((nbytes + 3) // 4, device=dev)
    m._lib.check(lib.mrp_edge_encoder_bwd_t(_ptr(dhT), stride, _ptr(hT), stride, _ptr(pose), E, C, _ptr(dw1), _ptr(db1),
                                            _ptr(ws), nbytes, _stream(dev)), "mrp_edge_encoder_bwd_t")
    torch.cuda.synchronize()
    sc.assert_bit_equal(dw1, c["dw1"], f"dW1 {tag}")
    sc.assert_bit_equal(db1, c["db1"], f"db1 {tag}")
    dpose = m.encoder.pose_grad(dhT_p[:, :E], hT[:, :E], w1)
    sc.assert_bit_equal(dpose, c["dpose"], f"dpose {tag}")


@pytest.mark.parametrize("fused", [True, False])
@VARIANT
def test_encoder_padded_function_exact(cuda_device, variant, fused):
    """E = 31, C = 48 through ``EdgeEncoderPaddedFunction`` (the split kernels on zero-padded operands): z,
    and for a dz with at most 12 non-zero edges per column dW2 and db2, bit for bit."""
    dev = cuda_device
    E, C = 31, 48
    c = sc.encoder_case(E, C, variant)
    kh = sc.ENCODER_VARIANTS[variant][2]
    dz = sc.lattice("bf16", (E, 2 * C), 977) * sc.sparse_mask(2 * C, E).t()
    rdw2 = sc.exact_product(dz.t().contiguous(), c["h64"].float(), 1.0, sc.QUANTUM[kh], None, f"padded dW2 {variant}")
    enc = m.edge_encoder([C, C]).to(dev)
    l1, l2 = enc.layers[0], enc.layers[2]
    with torch.no_grad():
        for p, k in ((l1.weight, "w1"), (l1.bias, "b1"), (l2.weight, "w2"), (l2.bias, "b2")):
            p.copy_(c[k])
    m.encoder.set_fused_backward(fused)
    try:
        before = m.encoder.PATH_COUNTS["split_padded"]
        z = m.encoder.edge_logits(enc.layers, c["pose"].to(dev))
        assert m.encoder.PATH_COUNTS["split_padded"] == before + 1
        z.backward(dz.to(dev))
    finally:
        m.encoder.set_fused_backward(True)
    tag = f"{variant} fused={fused}"
    sc.assert_bit_equal(z, c["z64"], f"padded z {tag}")
    sc.assert_bit_equal(l2.weight.grad, rdw2, f"padded dW2 {tag}")
    sc.assert_bit_equal(l2.bias.grad, dz.double().sum(0), f"padded db2 {tag}")
