"""GPU: the selectable precision of the fp32 split-bf16 compress (``compress.set_compress_precision``;
``mrp_compress_fwd_split_p`` / ``_bwd_data_split_p`` / ``_bwd_weight_split_p``).

1. On lattice operands (``tests/precision_cases.py``) every kernel form in ``"high"`` and ``"medium"`` must
   reproduce the sum of exactly its mode's part products BIT FOR BIT, gbias the exact row sums of the full
   dy, and only the mode's own ``PATH_COUNTS`` keys may move.
2. ``parts = 3`` through the new entry points is bit-identical to the existing ones.
3. On random operands the error against float64 is bounded elementwise by the derived truncation bound
   (``include/mrp_gnn.h``: 3.1 x 2^-18 / 2.01 x 2^-9 of sum_k |a_k b_k|) plus the suite's fp32 yardstick
   (2 x the largest error of torch's fp32 evaluation).
4. The autograd functions keep the forward's mode for both gradients; odd shapes stay on the HIP kernels;
   bf16 features ignore the mode; a two-layer training step is closer to float64 in ``"high"`` than in
   ``"medium"``.
"""
import types

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
import precision_cases as pc
import split_cases as sc
import stack_ref
from mrp_gnn_amd import _lib, compress
from mrp_gnn_amd.aggregate import _ptr
from split_cases import knobs as _knobs
from split_cases import stream as _stream

pytestmark = pytest.mark.gpu

PAIR = pytest.mark.parametrize("pairing", sc.PAIRINGS, ids=sc.pairing_id)
MODE = pytest.mark.parametrize("mode", pc.REDUCED)
#: the forward / data-gradient forms (gemm_split: per shape, 128-row workgroups, 256-row where M % 256 == 0)
#: and the weight gradient's (both operands split in the kernel; dy split once)
GEMM_KNOBS = {"split": {}, "split2": {"gemm_split": 2}, "split7": {"gemm_split": 7}}
NT_KNOBS = {"split_nt3": {"split_nt": 3}, "split_nt4": {"split_nt": 4}}
WGRAD_SHAPES = ((3, 64, 32), (8, 64, 32), (3, 256, 32))


def _nchw(t, dev):
    n, C, P = t.shape
    return t.view(n, C, 4, P // 4).to(dev)


def _ncp(t):
    return t.reshape(t.shape[0], t.shape[1], -1)


# ---- 1. lattice exactness per mode -------------------------------------------------------------------

@pytest.mark.parametrize("form", list(GEMM_KNOBS))
@pytest.mark.parametrize("n,C,P", sc.COMPRESS_SHAPES)
@PAIR
@MODE
def test_forward_and_data_gradient_keep_exactly_the_modes_products(cuda_device, mode, pairing, n, C, P, form):
    dev = cuda_device
    parts = pc.PARTS[mode]
    c = pc.compress_case(n, C, P, pairing)
    ref, ref0 = pc.compress_trunc_refs(n, C, P, pairing, parts), pc.compress_trunc_refs(n, C, P, pairing, parts, False)
    w = c["w"].view(C, 2 * C, 1, 1).to(dev)
    b = c["b"].to(dev)
    x, a, gy = (_nchw(c[k], dev) for k in ("x", "a", "gy"))
    cat = torch.cat((x, a), 1)
    gcat = torch.full((n, 2 * C, 4, P // 4), float("nan"), device=dev)
    tag = f"{mode} {form} {sc.pairing_id(pairing)} n={n} C={C} P={P}"
    with _knobs("split", **GEMM_KNOBS[form]):
        before = dict(compress.PATH_COUNTS)
        with compress.compress_precision_scope(mode):
            y = compress.compress_forward(w, b, x, a)
            y0 = compress.compress_forward(w, None, x, a)
            ycat = compress.compress_forward(w, b, cat[:, :C], cat[:, C:])
            gx, ga = compress.compress_backward_data(w, gy)
            compress.compress_backward_data(w, gy, gcat[:, :C], gcat[:, C:])
        assert pc.moved(before, compress.PATH_COUNTS) == {f"fwd_f32_{mode}": 3, f"dgrad_f32_{mode}": 2}, tag
    sc.assert_bit_equal(_ncp(y), ref["y"], f"y {tag}")
    sc.assert_bit_equal(_ncp(y0), ref0["y"], f"y without bias {tag}")
    sc.assert_bit_equal(_ncp(ycat), ref["y"], f"y from a cat buffer's halves {tag}")
    sc.assert_bit_equal(_ncp(gx), ref["gx"], f"gx {tag}")
    sc.assert_bit_equal(_ncp(ga), ref["ga"], f"ga {tag}")
    sc.assert_bit_equal(_ncp(gcat), torch.cat((ref["gx"], ref["ga"]), 1), f"[gx; ga] into a cat buffer {tag}")


@pytest.mark.parametrize("form", list(NT_KNOBS))
@pytest.mark.parametrize("n,C,P", WGRAD_SHAPES)
@PAIR
@MODE
def test_weight_gradient_keeps_exactly_the_modes_products(cuda_device, mode, pairing, n, C, P, form):
    dev = cuda_device
    c = pc.compress_case(n, C, P, pairing)
    ref = pc.compress_trunc_refs(n, C, P, pairing, pc.PARTS[mode])
    gy, x, a = (_nchw(c[k], dev) for k in ("gy_s", "xs", "as_"))
    tag = f"{mode} {form} {sc.pairing_id(pairing)} n={n} C={C} P={P}"
    with _knobs("split", **NT_KNOBS[form]):
        before = dict(compress.PATH_COUNTS)
        with compress.compress_precision_scope(mode):
            gw, gb = compress.compress_backward_weight(gy, x, a)
        assert pc.moved(before, compress.PATH_COUNTS) == {f"wgrad_f32_{mode}": 1}, tag
    sc.assert_bit_equal(gw.view(C, 2 * C), ref["gw"], f"gw {tag}")
    sc.assert_bit_equal(gb, ref["gb"], f"gbias (the row sums of the full gy) {tag}")


# ---- 2. parts = 3 is the existing entry point ---------------------------------------------------------

@pytest.mark.parametrize("split_nt", [3, 4])
def test_three_parts_is_bit_identical_to_the_existing_entry_points(cuda_device, split_nt):
    dev = cuda_device
    n, C, P = 3, 256, 32
    torch.manual_seed(41)
    w = torch.randn(C, 2 * C, 1, 1, device=dev) / (2 * C) ** 0.5
    b = torch.randn(C, device=dev)
    x, a, gy = (torch.randn(n, C, 4, P // 4, device=dev) for _ in range(3))
    st = _stream(dev)
    new = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    with _knobs("split", split_nt=split_nt) as lib:
        wf, wb = compress.packed_weight(w, "fwd"), compress.packed_weight(w, "bwd")
        y0, y1 = new(n, C, P), new(n, C, P)
        _lib.check(lib.mrp_compress_fwd_split(_ptr(x), C * P, _ptr(a), C * P, n, C, P, _ptr(wf), _ptr(b), _ptr(y0), C * P,
                                              st), "mrp_compress_fwd_split")
        _lib.check(lib.mrp_compress_fwd_split_p(_ptr(x), C * P, _ptr(a), C * P, n, C, P, _ptr(wf), _ptr(b), _ptr(y1),
                                                C * P, 3, st), "mrp_compress_fwd_split_p")
        g0, g1 = new(n, 2 * C, P), new(n, 2 * C, P)
        _lib.check(lib.mrp_compress_bwd_data_split(_ptr(gy), C * P, n, C, P, _ptr(wb), _ptr(g0), 2 * C * P,
                                                   _ptr(g0[:, C:]), 2 * C * P, st), "mrp_compress_bwd_data_split")
        _lib.check(lib.mrp_compress_bwd_data_split_p(_ptr(gy), C * P, n, C, P, _ptr(wb), _ptr(g1), 2 * C * P,
                                                     _ptr(g1[:, C:]), 2 * C * P, 3, st), "mrp_compress_bwd_data_split_p")
        nbytes = int(lib.mrp_compress_bwd_weight_split_workspace(n, C, P))
        ws = torch.empty(max(nbytes, 4) // 4 + 1, device=dev)
        dw0, dw1, db0, db1 = new(C, 2 * C), new(C, 2 * C), new(C), new(C)
        _lib.check(lib.mrp_compress_bwd_weight_split(_ptr(gy), C * P, _ptr(x), C * P, _ptr(a), C * P, n, C, P, _ptr(dw0),
                                                     _ptr(db0), _ptr(ws), nbytes, st), "mrp_compress_bwd_weight_split")
        _lib.check(lib.mrp_compress_bwd_weight_split_p(_ptr(gy), C * P, _ptr(x), C * P, _ptr(a), C * P, n, C, P,
                                                       _ptr(dw1), _ptr(db1), _ptr(ws), nbytes, 3, st),
                   "mrp_compress_bwd_weight_split_p")
        torch.cuda.synchronize()
    for name, p, q in (("y", y0, y1), ("[gx; ga]", g0, g1), ("gw", dw0, dw1), ("gbias", db0, db1)):
        assert bool(torch.isfinite(p).all()), name
        assert torch.equal(p, q), f"{name}: parts = 3 differs from the existing entry point"


# ---- 3. random operands against the derived bound -------------------------------------------------------

@pytest.fixture(scope="module")
def random_cases(cuda_device):
    """The shapes of ``test_gpu_split_fp32.py``: forward n = 2, C = 512, P = 32 (K = 1024), the data gradient
    at the same C (K = 512), the weight gradient n = 32, C = 64, P = 32 (K = 1024).  Per product: the
    float64 result, sum_k |a_k b_k| and the largest error of torch's fp32 evaluation."""
    dev = cuda_device
    torch.manual_seed(11)
    n, C, P = 2, 512, 32
    w = torch.randn(C, 2 * C, device=dev) * (2 * C) ** -0.5
    b = torch.randn(C, device=dev)
    cat = torch.randn(n, 2 * C, P, device=dev)
    gy = torch.randn(n, C, P, device=dev)
    torch.manual_seed(12)
    n2, C2, P2 = 32, 64, 32
    gy2 = torch.randn(n2, C2, P2, device=dev) * (n2 * P2) ** -0.5
    cat2 = torch.randn(n2, 2 * C2, P2, device=dev)

    def both(f):
        f64, f32 = f(torch.float64), f(torch.float32)
        return f64, float((f32.double() - f64).abs().max())

    def rows(t, dt):
        return t.to(dt).permute(1, 0, 2).reshape(t.shape[1], -1)

    r = {"fwd": both(lambda dt: torch.matmul(w.to(dt), cat.to(dt)) + b.to(dt)[None, :, None]) +
         (torch.matmul(w.double().abs(), cat.double().abs()),),
         "dgrad": both(lambda dt: torch.matmul(w.to(dt).t(), gy.to(dt))) +
         (torch.matmul(w.double().abs().t(), gy.double().abs()),),
         "wgrad": both(lambda dt: rows(gy2, dt) @ rows(cat2, dt).t()) +
         (rows(gy2, torch.float64).abs() @ rows(cat2, torch.float64).abs().t(),)}
    return {"fwd_ops": (n, C, P, w, b, cat, gy), "wgrad_ops": (n2, C2, P2, gy2, cat2), "ref": r}


def _bounded(got, ref, mode, what):
    """|got - f64| <= c (|A| |B|) + 2 max |torch_fp32 - f64| elementwise; returns stack_ref.err of got."""
    f64, e32, mag = ref
    d = (got.double() - f64).abs()
    bound = pc.TERM_BOUND[mode] * mag + 2.0 * e32
    worst = float((d / bound).max())
    trunc = float((d / (pc.TERM_BOUND[mode] * mag)).max())
    e = stack_ref.err(got, f64)
    print(f"\nPRECISION {what} {mode}: err {e:.3g}, worst |d| / bound {worst:.3f}, "
          f"|d| / truncation term alone {trunc:.3f}, fp32 yardstick {e32:.3g}")
    assert worst <= 1.0, f"{what} {mode}: |got - f64| reaches {worst:.3f} x the derived bound"
    return e


def test_random_operands_within_the_derived_bound(cuda_device, random_cases):
    n, C, P, w, b, cat, gy = random_cases["fwd_ops"]
    n2, C2, P2, gy2, cat2 = random_cases["wgrad_ops"]
    ref = random_cases["ref"]
    x, a = (cat[:, i * C:(i + 1) * C].reshape(n, C, 4, P // 4) for i in (0, 1))
    x2, a2 = (cat2[:, i * C2:(i + 1) * C2].reshape(n2, C2, 4, P2 // 4) for i in (0, 1))
    errs = {}
    for mode in pc.REDUCED:
        with _knobs("split"), compress.compress_precision_scope(mode):
            y = compress.compress_forward(w.view(C, 2 * C, 1, 1), b, x, a)
            gx, ga = compress.compress_backward_data(w.view(C, 2 * C, 1, 1), gy.view(n, C, 4, P // 4))
            gw, _gb = compress.compress_backward_weight(gy2.view(n2, C2, 4, P2 // 4), x2, a2)
        errs[mode] = {"fwd": _bounded(y.view(n, C, P), ref["fwd"], mode, "fwd"),
                      "dgrad": _bounded(torch.cat((gx, ga), 1).view(n, 2 * C, P), ref["dgrad"], mode, "dgrad"),
                      "wgrad": _bounded(gw.view(C2, 2 * C2), ref["wgrad"], mode, "wgrad")}
    for op in ("fwd", "dgrad", "wgrad"):
        assert errs["high"][op] < errs["medium"][op], (op, errs)


# ---- 4. autograd and routes -----------------------------------------------------------------------------

C4, HW4 = 64, 8


def _frames(ns, seed, C=C4, hw=HW4):
    rng = np.random.RandomState(seed)
    graphs = []
    for n in ns:
        poses = np.concatenate([rng.uniform(-10, 10, (n, 3)), rng.standard_normal((n, 4))], 1).astype(np.float32)
        graphs.append(m.frame_graph(poses))
    g = m.batch(graphs)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g.num_nodes(), C, hw, hw, generator=gen)
    G = torch.randn(g.num_nodes(), C, hw, hw, generator=gen)
    return g, x, G


def _no_library_gemm(monkeypatch):
    def boom(*_a, **_k):
        raise AssertionError("a library GEMM ran on the product path")
    for name in ("_lib_forward", "_lib_backward_data", "_lib_backward_weight"):
        monkeypatch.setattr(compress, name, boom)


def _high_keys(k=1):
    return {"fwd_f32_high": k, "dgrad_f32_high": k, "wgrad_f32_high": k}


def test_functions_keep_the_forwards_mode_for_both_gradients(cuda_device):
    """Complete 4-robot graphs, B = 2, C = 64, 8 x 8: forward inside ``compress_precision_scope("high")``,
    backward after the scope has closed — only the ``_high`` keys move, one of each per function."""
    dev = cuda_device
    g, x, G = _frames((4, 4), seed=5)
    csr = g.csr(dev)
    torch.manual_seed(6)
    conv = torch.nn.Conv2d(2 * C4, C4, kernel_size=1).to(dev)
    gb = torch.sigmoid(torch.randn(g.num_edges(), C4, 2)).to(dev).requires_grad_(True)
    xd = x.to(dev).requires_grad_(True)
    ad = torch.randn_like(x).to(dev).requires_grad_(True)
    assert compress.compress_precision() == "highest"
    for build in (lambda: compress.CompressFunction.apply(xd, ad, conv.weight, conv.bias),
                  lambda: compress.film_compress(conv, xd, gb, csr, _lib.MODE_FILM_MEAN)):
        before = dict(compress.PATH_COUNTS)
        with compress.compress_precision_scope("high"):
            y = build()
        assert compress.compress_precision() == "highest"
        y.backward(G.to(dev))
        torch.cuda.synchronize()
        assert pc.moved(before, compress.PATH_COUNTS) == _high_keys(), pc.moved(before, compress.PATH_COUNTS)
        assert all(bool(torch.isfinite(t.grad).all()) for t in (xd, conv.weight, conv.bias))


def test_odd_shape_in_high_stays_on_the_hip_kernels(cuda_device, monkeypatch):
    """C = 40, 5 x 5: zero-padded operands through the same reduced kernels, never torch's GEMMs; the results
    within the "high" bound of float64."""
    _no_library_gemm(monkeypatch)
    dev = cuda_device
    torch.manual_seed(7)
    n, C, H, W = 3, 40, 5, 5
    w = (torch.randn(C, 2 * C, 1, 1, device=dev) / (2 * C) ** 0.5).requires_grad_(True)
    b = torch.randn(C, device=dev, requires_grad=True)
    x = torch.randn(n, C, H, W, device=dev, requires_grad=True)
    a = torch.randn(n, C, H, W, device=dev, requires_grad=True)
    gy = torch.randn(n, C, H, W, device=dev)
    before = dict(compress.PATH_COUNTS)
    with compress.compress_precision_scope("high"):
        y = compress.CompressFunction.apply(x, a, w, b)
        y.backward(gy)
    assert pc.moved(before, compress.PATH_COUNTS) == _high_keys()
    w64, cat64 = w.detach().double().view(C, 2 * C), torch.cat((x, a), 1).detach().double()
    y64 = torch.einsum("oc,nchw->nohw", w64, cat64) + b.detach().double()[None, :, None, None]
    mag = torch.einsum("oc,nchw->nohw", w64.abs(), cat64.abs())
    # the truncation bound plus fp32 rounding of the K = 80 sums and the bias add (2^-23 per operation)
    assert bool(((y.double() - y64).abs() <= pc.TERM_BOUND["high"] * mag + 2.0 ** -20 * (mag + 1)).all())
    gw64 = torch.einsum("nohw,nchw->oc", gy.double(), cat64)
    assert stack_ref.err(w.grad.view(C, 2 * C), gw64) < 1e-4
    assert torch.allclose(b.grad.double(), gy.double().sum((0, 2, 3)), rtol=1e-5, atol=1e-5)


def test_bf16_features_ignore_the_mode(cuda_device):
    dev = cuda_device
    g, x, G = _frames((4, 4), seed=8)
    torch.manual_seed(9)
    stack = m.GCNStack(types.SimpleNamespace(feature_dim=C4, gcn_layers=1, gcn_combine="cat_compress")).to(dev)
    xd = x.to(torch.bfloat16).to(dev).requires_grad_(True)
    before = dict(compress.PATH_COUNTS)
    with compress.compress_precision_scope("high"):
        out = stack(g.to(dev), xd)
        out.backward(G.to(torch.bfloat16).to(dev))
    assert pc.moved(before, compress.PATH_COUNTS) == {"fwd_bf16": 1, "dgrad_bf16": 1, "wgrad_bf16": 1}


def test_two_layer_training_step_high_is_closer_than_medium(cuda_device):
    dev = cuda_device
    layers = 2
    g, x, G = _frames((4, 4), seed=10)
    gd = g.to(dev)
    torch.manual_seed(11)
    stack = m.GCNStack(types.SimpleNamespace(feature_dim=C4, gcn_layers=layers, gcn_combine="cat_compress")).to(dev)
    params = {k: v.detach().cpu() for k, v in stack.named_parameters()}
    src, dst = (t.long() for t in g.edges())
    ref_out, ref_dx, ref_grads = stack_ref.run(params, x, g.edata["pose"].double(), src, dst, G, torch.float64,
                                               layers=layers, combine="cat_compress")
    errs = {}
    for mode in pc.REDUCED:
        for p in stack.parameters():
            p.grad = None
        leaf = x.to(dev).requires_grad_(True)
        before = dict(compress.PATH_COUNTS)
        with compress.compress_precision_scope(mode):
            out = stack(gd, leaf)
            out.backward(G.to(dev))
        torch.cuda.synchronize()
        assert pc.moved(before, compress.PATH_COUNTS) == {f"{op}_f32_{mode}": layers for op in ("fwd", "dgrad", "wgrad")}
        grads = {k: p.grad for k, p in stack.named_parameters()}
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(leaf.grad).all())
        assert all(bool(torch.isfinite(v).all()) for v in grads.values())
        errs[mode] = {"out": stack_ref.err(out, ref_out), "dx": stack_ref.err(leaf.grad, ref_dx),
                      "conv": max(stack_ref.err(v, ref_grads[k]) for k, v in grads.items() if k.startswith("conv"))}
    print("\nPRECISION two-layer step errors against float64:", errs)
    for k in ("out", "dx", "conv"):
        assert errs["high"][k] < errs["medium"][k], (k, errs)
