"""The split-bf16 kernels on random operands, measured against the fp32 GEMM with no floor: the error
against float64 (``stack_ref.err``: max |d| / max |ref|) must be at most 2 x the error of torch's own
fp32 evaluation of the same product on the GPU (``split_cases.within_fp32``) — the project's claim is
"fp32 accuracy".  Reduction lengths of 1024, where an emulation of the correct six-product form with
exact block sums sits at 0.1 - 0.25 x the fp32 error and every defective form (a partial product dropped,
a two-way split) at 6 x or more (``tests/test_split_lattice_cpu.py`` pins both on the CPU); the kernels
themselves measure 0.34 - 1.31 x on the MI355X (the MFMA rounds its own 16- or 32-term sums), which
leaves the factor 2 a margin of 1.5 x above and 3 x below.  The fp32-MFMA ``hip`` path is held to the same
bound: its forward was one fmaf chain over K per output and measured 2.60 x at K = 1024 before
``gemm_nn`` cut the chain every 128 terms (0.58 x since).  Each case prints its measured ratio
ours / fp32 (``pytest -s``; DESIGN.md §3.5 records them)."""
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

FACTOR = 2.0


def _check(ours, f32, f64, what):
    ok, (e, e32) = sc.within_fp32(ours, f32, f64, FACTOR)
    print(f"\nRATIO {what}: ours {e:.3g} / fp32 {e32:.3g} = {e / e32:.3f}")
    assert ok, f"{what}: error {e:.3g} against float64 is {e / e32:.2f} x the fp32 GEMM's {e32:.3g} (bound {FACTOR:g} x)"


def _rand(dev, *shape, scale=1.0):
    return torch.randn(*shape, device=dev) * scale


@pytest.fixture(scope="module")
def compress_gemm_case(cuda_device):
    """n = 2, C = 512, P = 32 (K = 2C = 1024 forward, K = C data gradient) with both references."""
    torch.manual_seed(11)
    n, C, P = 2, 512, 32
    dev = cuda_device
    w = _rand(dev, C, 2 * C, scale=(2 * C) ** -0.5)
    b = _rand(dev, C)
    cat = _rand(dev, n, 2 * C, P)
    gy = _rand(dev, n, C, P)
    ref = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        ref[name] = (torch.matmul(w.to(dt), cat.to(dt)) + b.to(dt)[None, :, None], torch.matmul(w.to(dt).t(), gy.to(dt)))
    return n, C, P, w, b, cat, gy, ref


@pytest.mark.parametrize("form", list(GEMM_FORMS))
def test_compress_forward_and_data_gradient_within_fp32(cuda_device, compress_gemm_case, form):
    n, C, P, w, b, cat, gy, ref = compress_gemm_case
    x, a = (cat[:, i * C:(i + 1) * C].reshape(n, C, 4, P // 4) for i in (0, 1))
    path, knobs = GEMM_FORMS[form]
    with _knobs(path, **knobs):
        y = m.compress.compress_forward(w.view(C, 2 * C, 1, 1), b, x, a)
        gx, ga = m.compress.compress_backward_data(w.view(C, 2 * C, 1, 1), gy.view(n, C, 4, P // 4))
    _check(y.view(n, C, P), ref["f32"][0], ref["f64"][0], f"compress fwd {form}")
    _check(torch.cat((gx, ga), 1).view(n, 2 * C, P), ref["f32"][1], ref["f64"][1], f"compress dgrad {form}")


@pytest.fixture(scope="module")
def compress_wgrad_case(cuda_device):
    """n = 32, C = 64, P = 32 (K = n P = 1024)."""
    torch.manual_seed(12)
    n, C, P = 32, 64, 32
    dev = cuda_device
    gy = _rand(dev, n, C, P, scale=(n * P) ** -0.5)
    cat = _rand(dev, n, 2 * C, P)
    ref = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        g2 = gy.to(dt).permute(1, 0, 2).reshape(C, n * P)
        ref[name] = (g2 @ cat.to(dt).permute(1, 0, 2).reshape(2 * C, n * P).t(), g2.sum(1))
    return n, C, P, gy, cat, ref


@pytest.mark.parametrize("form", list(NT_FORMS))
def test_compress_weight_gradient_within_fp32(cuda_device, compress_wgrad_case, form):
    n, C, P, gy, cat, ref = compress_wgrad_case
    x, a = (cat[:, i * C:(i + 1) * C].reshape(n, C, 4, P // 4) for i in (0, 1))
    path, knobs = NT_FORMS[form]
    with _knobs(path, **knobs):
        gw, gb = m.compress.compress_backward_weight(gy.view(n, C, 4, P // 4), x, a)
    _check(gw.view(C, 2 * C), ref["f32"][0], ref["f64"][0], f"compress wgrad {form}")


@pytest.fixture(scope="module")
def encoder_z_case(cuda_device):
    """E = 64, C = 1024: the encoder's logits (K = C) against the reference layers in fp32 and float64."""
    torch.manual_seed(13)
    E, C = 64, 1024
    enc = m.edge_encoder([C, C]).to(cuda_device)
    l1, l2 = enc.layers[0], enc.layers[2]
    pose = _rand(cuda_device, E, 9)
    ref = {}
    with torch.no_grad():
        for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
            h = torch.relu(torch.nn.functional.linear(pose.to(dt), l1.weight.to(dt), l1.bias.to(dt)))
            ref[name] = torch.nn.functional.linear(h, l2.weight.to(dt), l2.bias.to(dt))
    return E, C, pose, m.encoder.packed_weights(l1, l2), l2.bias.detach().contiguous(), ref, enc


@pytest.mark.parametrize("waves", [1, 3, -1])
@pytest.mark.parametrize("train", [False, True], ids=["inference", "train"])
def test_encoder_logits_within_fp32(cuda_device, encoder_z_case, train, waves):
    E, C, pose, img, b2, ref, _enc = encoder_z_case
    dev = cuda_device
    z = torch.empty(E, 2 * C, device=dev)
    hT = torch.empty(C, E, device=dev)
    with _knobs(edge_split_v=waves) as lib:
        if train:
            m._lib.check(lib.mrp_edge_encoder_fwd_split_train(_ptr(pose), _ptr(img), _ptr(b2), E, C, _ptr(z), _ptr(hT), E,
                                                              _stream(dev)), "mrp_edge_encoder_fwd_split_train")
        else:
            m._lib.check(lib.mrp_edge_encoder_fwd_split(_ptr(pose), _ptr(img), _ptr(b2), E, C, _ptr(z), _stream(dev)),
                         "mrp_edge_encoder_fwd_split")
        torch.cuda.synchronize()
    _check(z, ref["f32"], ref["f64"], f"encoder z {'train' if train else 'inference'} edge_split_v={waves}")


def _encoder_bwd_operands(dev, E, C, seed):
    torch.manual_seed(seed)
    t = {"dz": _rand(dev, E, 2 * C), "w2": _rand(dev, 2 * C, C, scale=(2 * C) ** -0.5),
         "hT": torch.relu(_rand(dev, C, E, scale=E ** -0.5)), "pose": _rand(dev, E, 9)}
    t["w2t"] = t["w2"].t().contiguous()
    t["dzT"] = t["dz"].t().contiguous()
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        t["dhT_" + name] = t["w2t"].to(dt) @ t["dzT"].to(dt)
        t["dw2_" + name] = t["dzT"].to(dt) @ t["hT"].to(dt).t()
    return t


@pytest.fixture(scope="module")
def encoder_dw2_case(cuda_device):
    return _encoder_bwd_operands(cuda_device, 1024, 64, 14)  # dW2 = dz^T h: K = E = 1024


@pytest.fixture(scope="module")
def encoder_dht_case(cuda_device):
    return _encoder_bwd_operands(cuda_device, 64, 512, 15)  # dh^T = W2^T dz^T: K = 2C = 1024


def test_encoder_backward_split_within_fp32(cuda_device, encoder_dw2_case, encoder_dht_case):
    dev = cuda_device
    lib = m.load_library()
    t = encoder_dw2_case
    E, C = 1024, 64
    dw2, db2 = torch.empty(2 * C, C, device=dev), torch.empty(2 * C, device=dev)
    _bwd_split(lib, dev, E, C, None, t["dzT"], None, t["hT"], None, dw2, db2)
    _check(dw2, t["dw2_f32"], t["dw2_f64"], "encoder dW2 bwd_split")
    t = encoder_dht_case
    E, C = 64, 512
    dhT = torch.empty(C, E, device=dev)
    _bwd_split(lib, dev, E, C, t["dz"], None, t["w2t"], None, dhT, None, None)
    _check(dhT, t["dhT_f32"], t["dhT_f64"], "encoder dhT bwd_split")


@pytest.mark.parametrize("knobs", FUSED_FORMS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_encoder_backward_fused_within_fp32(cuda_device, encoder_dw2_case, knobs):
    """dW2 (K = E = 1024) from ``mrp_edge_encoder_bwd_fused`` in each of its forms (dh^T is not an output
    of the fused form)."""
    t = encoder_dw2_case
    with _knobs(**knobs) as lib:
        _dw1, _db1, dw2, _db2 = _bwd_fused(lib, cuda_device, {"E": 1024, "C": 64}, t)
    _check(dw2, t["dw2_f32"], t["dw2_f64"], f"encoder dW2 bwd_fused {knobs}")
