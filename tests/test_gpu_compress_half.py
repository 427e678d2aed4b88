"""GPU: the 1x1 compress and both gradients on bf16 / fp16 feature maps (``csrc/compress_half.hip``:
``mrp_compress_fwd_t`` / ``_bwd_data_t`` / ``_bwd_weight_t``), each product through ``compress.py``.

Inputs are drawn in fp32 and rounded to T; the weight is ``randn / sqrt(2C)``, fp32.  Yardstick: float64
on the widened operands with the weight rounded to T (``W.to(T).double()``: the contract rounds it once
when it is packed).  Bars, from the number formats (``half_cases.assert_elementwise``,
``stack_ref.within``):

* T outputs (y, gx, ga): elementwise ``|got - ref| <= u_T |ref| + 1e-5 max|ref|``;
* fp32 ``dW`` / ``db``: ``err <= max(1e-5, 4 x the error of the same product computed in fp32 by torch on
  the CPU)``.

Tile geometry the shapes are named against: 256 x 128 output tiles, 32-k stages, two LDS buffers."""
import ctypes
import functools

import pytest
import torch

import mrp_gnn_amd as m
import half_cases as hc
import stack_ref

pytestmark = pytest.mark.gpu

KEYS = list(hc.DTYPES)
#: (C, Nt, H, W): what it reaches
SHAPES = [
    (32, 3, 8, 8),   # one partly filled row tile; a full plus a ragged column tile; K = 2 stages
    (96, 2, 8, 8),   # K = 6 stages, so the buffer ring wraps; M ragged
    (256, 2, 8, 8),  # whole-tile form; the data gradient has M = 512 = two row tiles, gx in one and ga in the other
    (64, 5, 4, 4),   # P < a tile's columns, several nodes per column tile; P % 32 != 0: the weight gradient pads
]
PADDED = [(5, 3, 3, 3), (33, 2, 7, 7)]  # C % 32 != 0 and P % 8 != 0: the zero-padded route
WGRAD_K4096 = (64, 64, 8, 8)


@functools.lru_cache(maxsize=None)
def _case(C, n, H, W, key, bias=True):
    """CPU operands (w, b fp32; x, a, gy in T) and the float64 / fp32 references, computed once."""
    T = hc.DTYPES[key]
    gen = torch.Generator().manual_seed(C * 1009 + n * 31 + H * 7 + W + (0 if key == "bf16" else 1))
    w = torch.randn(C, 2 * C, 1, 1, generator=gen) / (2 * C) ** 0.5
    b = torch.randn(C, generator=gen) if bias else None
    x, a, gy = (torch.randn(n, C, H, W, generator=gen).to(T) for _ in range(3))
    ref = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        w2 = w.reshape(C, 2 * C).to(T).to(dt)  # the weight as the kernels hold it
        cat, g = torch.cat((x, a), 1).to(dt), gy.to(dt)
        y = torch.einsum("oc,nchw->nohw", w2, cat)
        if b is not None:
            y = y + b.to(dt)[None, :, None, None]
        gcat = torch.einsum("oc,nohw->nchw", w2, g)
        ref[tag] = dict(y=y, gx=gcat[:, :C], ga=gcat[:, C:],
                        gw=torch.einsum("nohw,nchw->oc", g, cat).reshape(C, 2 * C, 1, 1), gb=g.sum((0, 2, 3)))
    return w, b, x, a, gy, ref


def _check_t(got, ref, name, T, what):
    assert got.dtype == T, (what, name, got.dtype)
    hc.assert_elementwise(got, ref["64"][name], T, f"{what} {name}")


def _check_f32(got, ref, name, what):
    assert got.dtype == torch.float32
    ok, errs = stack_ref.within(got, ref["32"][name], ref["64"][name])
    print(what, name, "err, fp32 torch err", errs)
    assert ok, (what, name, errs)


def _counts():
    return dict(m.compress.PATH_COUNTS)


def _moved(before):
    return {k: v - before.get(k, 0) for k, v in m.compress.PATH_COUNTS.items() if v != before.get(k, 0)}


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("C,n,H,W", SHAPES)
def test_products_match_float64(cuda_device, key, C, n, H, W):
    """Forward, data gradient and weight gradient; the counters move on T's keys only."""
    T, dev = hc.DTYPES[key], cuda_device
    w, b, x, a, gy, ref = _case(C, n, H, W, key)
    w, b, x, a, gy = (t.to(dev) for t in (w, b, x, a, gy))
    before = _counts()
    y = m.compress.compress_forward(w, b, x, a)
    gx, ga = m.compress.compress_backward_data(w, gy)
    gw, gb = m.compress._bwd_weight(gy, x, a, True, None, None)
    assert _moved(before) == {"fwd_" + key: 1, "dgrad_" + key: 1, "wgrad_" + key: 1}
    what = f"{key} {(C, n, H, W)}"
    for name, got in (("y", y), ("gx", gx), ("ga", ga)):
        _check_t(got, ref, name, T, what)
    for name, got in (("gw", gw), ("gb", gb)):
        _check_f32(got, ref, name, what)
    # the same launches again: the same bits (fixed-order sums, no atomics)
    assert torch.equal(hc.bits(m.compress.compress_forward(w, b, x, a)), hc.bits(y))
    gw2, gb2 = m.compress._bwd_weight(gy, x, a, True, None, None)
    assert torch.equal(gw2, gw) and torch.equal(gb2, gb)


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("C,n,H,W", PADDED)
def test_padded_shapes_run_the_native_kernels(cuda_device, monkeypatch, key, C, n, H, W):
    """Shapes the kernels do not tile: the same kernels on zero-padded operands, never torch's GEMMs."""
    def boom(*_a, **_k):
        raise AssertionError("a library GEMM ran on the product path")
    for name in ("_lib_forward", "_lib_backward_data", "_lib_backward_weight"):
        monkeypatch.setattr(m.compress, name, boom)
    T, dev = hc.DTYPES[key], cuda_device
    w, b, x, a, gy, ref = _case(C, n, H, W, key)
    w, b, x, a = (t.to(dev).requires_grad_(True) for t in (w, b, x, a))
    before = _counts()
    y = m.compress.CompressFunction.apply(x, a, w, b)
    y.backward(gy.to(dev))
    assert _moved(before) == {"fwd_" + key: 1, "dgrad_" + key: 1, "wgrad_" + key: 1}
    what = f"padded {key} {(C, n, H, W)}"
    for name, got in (("y", y), ("gx", x.grad), ("ga", a.grad)):
        _check_t(got, ref, name, T, what)
    for name, got in (("gw", w.grad), ("gb", b.grad)):
        _check_f32(got, ref, name, what)


@pytest.mark.parametrize("key", KEYS)
def test_weight_gradient_splits(cuda_device, key):
    """K = 4096 with the split count forced to 1 (unsplit form, written straight to dW), 3 (partial tiles
    + the fixed-order sum) and 0 (the planner's): each within the bar, each bit-equal to itself on a second
    run, and the three agree within the bar's sum."""
    dev = cuda_device
    C, n, H, W = WGRAD_K4096
    _, _, x, a, gy, ref = _case(C, n, H, W, key)
    x, a, gy = (t.to(dev) for t in (x, a, gy))
    lib = m.load_library()
    got = {}
    try:
        for s in (1, 3, 0):
            assert lib.mrp_tuning_set(b"half_nt_splits", s) == 0
            nbytes = int(lib.mrp_compress_bwd_weight_t_workspace(n, C, H * W))
            assert (nbytes == 0) if s == 1 else (nbytes == (3 * C * 2 * C + 3 * C) * 4 if s == 3 else nbytes >= 0)
            gw, gb = m.compress.compress_backward_weight(gy, x, a)
            gw2, gb2 = m.compress.compress_backward_weight(gy, x, a)
            assert torch.equal(gw, gw2) and torch.equal(gb, gb2), s
            _check_f32(gw, ref, "gw", f"{key} splits {s}")
            _check_f32(gb, ref, "gb", f"{key} splits {s}")
            got[s] = (gw, gb)
    finally:
        assert lib.mrp_tuning_set(b"half_nt_splits", 0) == 0
    bar = 2 * max(1e-5, 4.0 * stack_ref.err(ref["32"]["gw"], ref["64"]["gw"]))
    for s in (3, 0):
        assert stack_ref.err(got[s][0], got[1][0]) <= bar


def _raw_forward(lib, T, x, a, img, b, y, n, C, P):
    st = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    return lib.mrp_compress_fwd_t(m.compress.HALF_DTYPES[T], p(x), x.stride(0), p(a), a.stride(0), n, C, P, p(img), p(b),
                                  p(y), y.stride(0), st)


@pytest.mark.parametrize("key", KEYS)
def test_cat_buffer_halves_sentinels_and_guard(cuda_device, key):
    """x and a as the halves of a (Nt, 2C, H, W) buffer (node stride 2 C P); gx / ga written into halves
    of gradient buffers whose other halves keep their sentinel; and Nt P = 192 columns end in a ragged
    column tile (64 of 128): one more node allocated after each output stays untouched."""
    T, dev = hc.DTYPES[key], cuda_device
    C, n, H, W = SHAPES[0]
    P = H * W
    w, b, x, a, gy, ref = _case(C, n, H, W, key)
    w, b, gy = w.to(dev), b.to(dev), gy.to(dev)
    cat = torch.cat((x, a), 1).to(dev)
    xv, av = cat[:, :C], cat[:, C:]
    assert m.compress._nstride(av) == 2 * C * P
    y = m.compress.compress_forward(w, b, xv, av)
    _check_t(y, ref, "y", T, key + " cat halves")
    gw, gb = m.compress.compress_backward_weight(gy, xv, av)
    _check_f32(gw, ref, "gw", key + " cat halves")
    _check_f32(gb, ref, "gb", key + " cat halves")

    sentinel = -7.0
    ga_buf = torch.full((n + 1, 2 * C, H, W), sentinel, device=dev, dtype=T)
    gx_buf = torch.full((n + 1, 2 * C, H, W), sentinel, device=dev, dtype=T)
    m.compress.compress_backward_data(w, gy, gx=gx_buf[:n, :C], ga=ga_buf[:n, C:])
    _check_t(gx_buf[:n, :C], ref, "gx", T, key + " halves")
    _check_t(ga_buf[:n, C:], ref, "ga", T, key + " halves")
    assert bool((gx_buf[:, C:] == sentinel).all()) and bool((ga_buf[:, :C] == sentinel).all())
    assert bool((gx_buf[n] == sentinel).all()) and bool((ga_buf[n] == sentinel).all())
    # both halves of one gradient buffer
    gcat = torch.full((n + 1, 2 * C, H, W), sentinel, device=dev, dtype=T)
    m.compress.compress_backward_data(w, gy, gx=gcat[:n, :C], ga=gcat[:n, C:])
    assert torch.equal(hc.bits(gcat[:n, :C]), hc.bits(gx_buf[:n, :C]))
    assert torch.equal(hc.bits(gcat[:n, C:]), hc.bits(ga_buf[:n, C:]))
    assert bool((gcat[n] == sentinel).all())
    # the forward into a buffer with a guard node behind it (the C entry point: compress_forward allocates y)
    ybuf = torch.full((n + 1, C, H, W), sentinel, device=dev, dtype=T)
    img = m.compress.packed_weight(w, "fwd", T)
    assert _raw_forward(m.load_library(), T, xv, av, img, b, ybuf, n, C, P) == 0
    assert torch.equal(hc.bits(ybuf[:n]), hc.bits(y)) and bool((ybuf[n] == sentinel).all())


@pytest.mark.parametrize("key", KEYS)
def test_no_bias(cuda_device, key):
    """``bias=None`` in the forward and ``db`` not wanted in the weight gradient."""
    T, dev = hc.DTYPES[key], cuda_device
    C, n, H, W = SHAPES[1]
    w, b, x, a, gy, ref = _case(C, n, H, W, key, bias=False)
    assert b is None
    w, x, a, gy = (t.to(dev) for t in (w, x, a, gy))
    _check_t(m.compress.compress_forward(w, None, x, a), ref, "y", T, key + " no bias")
    gw, gb = m.compress.compress_backward_weight(gy, x, a, want_bias=False)
    assert gb is None
    _check_f32(gw, ref, "gw", key + " no bias")


def test_packed_image_cached_per_dtype_and_version(cuda_device):
    """One image per (weight version, kind, dtype); the fp32 image is untouched by the 16-bit ones."""
    dev = cuda_device
    w = (torch.randn(32, 64, 1, 1) / 8).to(dev)
    f32 = m.compress.packed_weight(w, "fwd")
    bf = m.compress.packed_weight(w, "fwd", torch.bfloat16)
    fh = m.compress.packed_weight(w, "fwd", torch.float16)
    assert m.compress.packed_weight(w, "fwd") is f32 and m.compress.packed_weight(w, "fwd", torch.bfloat16) is bf
    assert bf is not fh and bf.numel() * 4 == 32 * 64 * 2 and f32.numel() * 4 == 32 * 64 * 6
    w.mul_(2.0)
    assert m.compress.packed_weight(w, "fwd", torch.bfloat16) is not bf
    # the image holds the weight rounded to nearest even, in `pack`'s lane order: unit (mb KS + ks) 64 + lane
    # = row 32 mb + (lane & 31), k = 16 ks + 8 (lane >> 5) ..
    img = m.compress.packed_weight(w, "fwd", torch.bfloat16).view(torch.bfloat16)[:32 * 64].view(4, 2, 32, 8).cpu()
    want = w.reshape(32, 64).to(torch.bfloat16).cpu().view(32, 4, 2, 8).permute(1, 2, 0, 3)
    assert torch.equal(hc.bits(img), hc.bits(want))
