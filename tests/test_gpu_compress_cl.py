"""GPU: the 1x1 compress and both gradients on pixel-major (``torch.channels_last``) bf16 / fp16 feature
maps (``csrc/compress_half_cl.hip``: ``mrp_compress_fwd_cl`` / ``_bwd_data_cl`` / ``_bwd_weight_cl``),
through ``compress.py``, ``GCN.forward_cat_compress``, ``GCNStack`` and ``multi_view_dgl_model``.

Yardsticks are ``tests/test_gpu_compress_half.py``'s: float64 on the widened operands with the weight
rounded to T; T outputs elementwise within ``u_T |ref| + 1e-5 max|ref|`` (``half_cases.assert_elementwise``),
fp32 ``dW`` / ``db`` within ``max(1e-5, 4 x torch's fp32 CPU error)`` (``stack_ref.within``).  Bit-equality
with the NCHW kernels is not required (the k order inside one MFMA differs); whether it happens is printed.

Tile geometry the shapes are named against: 256 x 128 output tiles (channels x pixel rows in the forward
and data gradient), 32-k stages (32 pixel rows in the weight gradient), two LDS buffers."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib, aggregate, compress
import half_cases as hc
import stack_ref
from conftest import rel_err

pytestmark = pytest.mark.gpu

CL = torch.channels_last
KEYS = list(hc.DTYPES)
#: (C, Nt, H, W): what it reaches
SHAPES = [
    (32, 3, 8, 8),   # partial row tile (M = 32 / 64 of 256), 192 pixel rows: a full and a ragged column tile
    (96, 2, 8, 8),   # K = 6 stages forward, the buffer ring wraps
    (256, 2, 8, 8),  # whole tiles; the data gradient's M = 512: gx and ga land in different row tiles
    (64, 5, 7, 7),   # P = 49: weight-gradient stages cross node boundaries, 245 rows: the last stage is ragged
    (64, 1, 1, 3),   # fewer pixel rows than one stage
]
WGRAD_K4096 = (64, 64, 8, 8)


@functools.lru_cache(maxsize=None)
def _case(C, n, H, W, key):
    """CPU operands (w, b fp32; x, a, gy in T, NCHW) and the float64 / fp32 references, computed once."""
    T = hc.DTYPES[key]
    gen = torch.Generator().manual_seed(C * 1013 + n * 37 + H * 7 + W + (0 if key == "bf16" else 1))
    w = torch.randn(C, 2 * C, 1, 1, generator=gen) / (2 * C) ** 0.5
    b = torch.randn(C, generator=gen)
    x, a, gy = (torch.randn(n, C, H, W, generator=gen).to(T) for _ in range(3))
    ref = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        w2 = w.reshape(C, 2 * C).to(T).to(dt)  # the weight as the kernels hold it
        cat, g = torch.cat((x, a), 1).to(dt), gy.to(dt)
        y = torch.einsum("oc,nchw->nohw", w2, cat) + b.to(dt)[None, :, None, None]
        gcat = torch.einsum("oc,nohw->nchw", w2, g)
        ref[tag] = dict(y=y, gx=gcat[:, :C], ga=gcat[:, C:],
                        gw=torch.einsum("nohw,nchw->oc", g, cat).reshape(C, 2 * C, 1, 1), gb=g.sum((0, 2, 3)))
    return w, b, x, a, gy, ref


def _cl(t, dev):
    return t.to(dev).contiguous(memory_format=CL)


def _check_t(got, ref, name, T, what):
    assert got.dtype == T, (what, name, got.dtype)
    hc.assert_elementwise(got, ref["64"][name], T, f"{what} {name}")


def _check_f32(got, ref, name, what):
    assert got.dtype == torch.float32
    ok, errs = stack_ref.within(got, ref["32"][name], ref["64"][name])
    print(what, name, "err, fp32 torch err", errs)
    assert ok, (what, name, errs)


def _counts():
    return dict(compress.PATH_COUNTS)


def _moved(before, counter=None):
    counter = compress.PATH_COUNTS if counter is None else counter
    return {k: v - before.get(k, 0) for k, v in counter.items() if v != before.get(k, 0)}


def _is_cl(t):
    return aggregate.pixel_strides(t) == (t.shape[1] * t.shape[2] * t.shape[3], t.shape[1])


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("C,n,H,W", SHAPES)
def test_products_match_float64(cuda_device, key, C, n, H, W):
    """All five outputs against the bars, the counters move on the ``_cl_`` keys only, a second run gives
    the same bits; the outputs are dense channels_last."""
    T, dev = hc.DTYPES[key], cuda_device
    w, b, x, a, gy, ref = _case(C, n, H, W, key)
    w, b = w.to(dev), b.to(dev)
    x, a, gy = (_cl(t, dev) for t in (x, a, gy))
    before = _counts()
    y = compress.compress_forward(w, b, x, a)
    gx, ga = compress.compress_backward_data(w, gy)
    gw, gb = compress._bwd_weight(gy, x, a, True, None, None)
    assert _moved(before) == {"fwd_cl_" + key: 1, "dgrad_cl_" + key: 1, "wgrad_cl_" + key: 1}
    what = f"cl {key} {(C, n, H, W)}"
    for name, got in (("y", y), ("gx", gx), ("ga", ga)):
        assert _is_cl(got), (what, name, got.stride())
        _check_t(got, ref, name, T, what)
    for name, got in (("gw", gw), ("gb", gb)):
        _check_f32(got, ref, name, what)
    y2 = compress.compress_forward(w, b, x, a)
    gx2, ga2 = compress.compress_backward_data(w, gy)
    gw2, gb2 = compress._bwd_weight(gy, x, a, True, None, None)
    assert torch.equal(hc.bits(y2), hc.bits(y)) and torch.equal(hc.bits(gx2), hc.bits(gx))
    assert torch.equal(hc.bits(ga2), hc.bits(ga)) and torch.equal(gw2, gw) and torch.equal(gb2, gb)
    if H * W % 32 == 0:  # informational: the NCHW kernels on the same operands
        yn = compress.compress_forward(w, b, x.contiguous(), a.contiguous())
        gwn, _ = compress._bwd_weight(gy.contiguous(), x.contiguous(), a.contiguous(), True, None, None)
        print(what, "bit-equal to the NCHW kernels: y", torch.equal(hc.bits(yn), hc.bits(y.contiguous())),
              "gw", torch.equal(gwn, gw))


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("key", KEYS)
def test_strides_sentinels_and_guard(cuda_device, key):
    """x and a as the halves of a channels_last 2C buffer (pixel stride 2C) that is a batch slice of a
    larger one (node stride > P ps); gx and ga written into the halves of one sentinel-filled channels_last
    2C gradient buffer with a guard node; the forward into a channels_last buffer with a guard node.  The
    guard nodes and, where a half is written alone, the other half keep their sentinel."""
    T, dev = hc.DTYPES[key], cuda_device
    C, n, H, W = SHAPES[0]
    P = H * W
    w, b, x, a, gy, ref = _case(C, n, H, W, key)
    w, b = w.to(dev), b.to(dev)
    gy = _cl(gy, dev)
    # every second node of a (2n, 2C, H, W) channels_last buffer: node stride 2 (P 2C)
    big = torch.zeros((2 * n, 2 * C, H, W), device=dev, dtype=T).contiguous(memory_format=CL)
    cat = big[::2]
    cat.copy_(torch.cat((x, a), 1))
    xv, av = cat[:, :C], cat[:, C:]
    assert aggregate.pixel_strides(xv) == (2 * P * 2 * C, 2 * C) == aggregate.pixel_strides(av)
    before = _counts()
    y = compress.compress_forward(w, b, xv, av)
    gw, gb = compress.compress_backward_weight(gy, xv, av)
    assert _moved(before) == {"fwd_cl_" + key: 1, "wgrad_cl_" + key: 1}
    _check_t(y, ref, "y", T, key + " cl halves")
    _check_f32(gw, ref, "gw", key + " cl halves")
    _check_f32(gb, ref, "gb", key + " cl halves")

    sentinel = -7.0
    full = lambda ch: torch.full((n + 1, ch, H, W), sentinel, device=dev, dtype=T).contiguous(memory_format=CL)  # noqa: E731
    gx_buf, ga_buf, gcat = full(2 * C), full(2 * C), full(2 * C)
    compress.compress_backward_data(w, gy, gx=gx_buf[:n, :C], ga=ga_buf[:n, C:])
    _check_t(gx_buf[:n, :C], ref, "gx", T, key + " cl halves")
    _check_t(ga_buf[:n, C:], ref, "ga", T, key + " cl halves")
    assert bool((gx_buf[:, C:] == sentinel).all()) and bool((ga_buf[:, :C] == sentinel).all())
    assert bool((gx_buf[n] == sentinel).all()) and bool((ga_buf[n] == sentinel).all())
    compress.compress_backward_data(w, gy, gx=gcat[:n, :C], ga=gcat[:n, C:])
    assert torch.equal(hc.bits(gcat[:n, :C]), hc.bits(gx_buf[:n, :C]))
    assert torch.equal(hc.bits(gcat[:n, C:]), hc.bits(ga_buf[:n, C:]))
    assert bool((gcat[n] == sentinel).all())
    # the forward's C entry point into a buffer with a guard node behind it
    ybuf = full(C)
    img = compress.packed_weight(w, "fwd", T)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    (xn, xp), (an, ap) = aggregate.pixel_strides(xv), aggregate.pixel_strides(av)
    code = m.load_library().mrp_compress_fwd_cl(compress.HALF_DTYPES[T], _p(xv), xn, xp, _p(av), an, ap, n, C, P,
                                                _p(img), _p(b), _p(ybuf), P * C, C, st)
    assert code == 0
    assert torch.equal(hc.bits(ybuf[:n]), hc.bits(y)) and bool((ybuf[n] == sentinel).all())


@pytest.mark.parametrize("key", KEYS)
def test_weight_gradient_splits(cuda_device, key):
    """K = 4096 with ``half_cl_splits`` forced to 1, 3 and 0 (the planner's): each within the bar and
    bit-repeatable; the workspace query is [3][C][2C] + [3][C] floats at 3 and 0 at 1."""
    dev = cuda_device
    C, n, H, W = WGRAD_K4096
    _, _, x, a, gy, ref = _case(C, n, H, W, key)
    x, a, gy = (_cl(t, dev) for t in (x, a, gy))
    lib = m.load_library()
    try:
        for s in (1, 3, 0):
            assert lib.mrp_tuning_set(b"half_cl_splits", s) == 0
            nbytes = int(lib.mrp_compress_bwd_weight_cl_workspace(n, C, H * W))
            part = (C * 2 * C + C) * 4  # one split's [C][2C] partial tile and [C] bias sums, fp32
            if s == 1:
                assert nbytes == 0
            elif s == 3:
                assert nbytes == 3 * part
            else:  # the planner's: none, or a whole number (>= 2, at most one per stage) of partials
                assert nbytes % part == 0 and nbytes // part != 1 and nbytes // part <= n * H * W // 32
            before = _counts()
            gw, gb = compress.compress_backward_weight(gy, x, a)
            gw2, gb2 = compress.compress_backward_weight(gy, x, a)
            assert _moved(before) == {"wgrad_cl_" + key: 2}
            assert torch.equal(gw, gw2) and torch.equal(gb, gb2), s
            _check_f32(gw, ref, "gw", f"cl {key} splits {s}")
            _check_f32(gb, ref, "gb", f"cl {key} splits {s}")
    finally:
        assert lib.mrp_tuning_set(b"half_cl_splits", 0) == 0


# ---- the layer ----------------------------------------------------------------------------------------
LC, LHW = 64, 6
#: name -> (node counts, k-NN k or None, layers, module)
LAYER_CASES = {"gcn_complete_5": ((5, 5), None, 1, "gcn"), "stack2_complete_5": ((5, 5), None, 2, "stack"),
               "stack2_knn4_16": ((16,), 4, 2, "stack"), "model_complete_5": ((5, 5), None, 1, "model")}


def _frames(ns, knn, seed):
    rng = np.random.RandomState(seed)
    graphs = []
    for n in ns:
        poses = np.concatenate([rng.uniform(-10, 10, (n, 3)), rng.standard_normal((n, 4))], 1).astype(np.float32)
        graphs.append(m.frame_graph(poses, knn=knn))
    g = m.batch(graphs)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g.num_nodes(), LC, LHW, LHW, generator=gen)
    G = torch.randn(g.num_nodes(), LC, LHW, LHW, generator=gen)
    return g, x, G


def _run(mod, call, x_dev, G_dev, autocast_dtype=None):
    for p in mod.parameters():
        p.grad = None
    leaf = x_dev.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    before, before_agg = _counts(), dict(aggregate.PATH_COUNTS)
    if autocast_dtype is not None:
        with torch.autocast("cuda", dtype=autocast_dtype):
            out = call(leaf)
    else:
        out = call(leaf)
    out.backward(G_dev)
    grads = {k: p.grad.detach().clone() for k, p in mod.named_parameters()}
    return out.detach(), leaf.grad, grads, _moved(before), _moved(before_agg, aggregate.PATH_COUNTS)


def _group_errs(dx, grads, ref_dx, ref_grads):
    e = {"dx": stack_ref.err(dx, ref_dx), "conv": 0.0, "encoder": 0.0}
    for k, g in grads.items():
        grp = "conv" if k.startswith("conv") else "encoder"
        e[grp] = max(e[grp], stack_ref.err(g, ref_grads[k]))
    return e


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("case", list(LAYER_CASES))
def test_layer_channels_last(cuda_device, key, case):
    """channels_last T features through ``GCN.forward_cat_compress``, a two-layer ``GCNStack(cat_compress)``
    and ``multi_view_dgl_model(compress_gcn)``: channels_last T output, one pixel-major aggregation forward /
    backward and one of each pixel-major compress product per layer, no convert route and no torch
    convolution; the bars are ``tests/test_gpu_half_compress_model.py``'s — the output within 2 layers u_T
    (max-abs relative) of the fp32 module on the widened input, dx and the parameter gradients against
    float64 (``stack_ref.run``) no worse than 1.5 x the earlier route's (the 16-bit cat kernel + torch's
    convolution under autocast, on the NCHW input)."""
    T, dev = hc.DTYPES[key], cuda_device
    ns, knn, layers, kind = LAYER_CASES[case]
    g, x, G = _frames(ns, knn, seed=31 + layers)
    gd = g.to(dev)
    torch.manual_seed(5)
    if kind == "gcn":
        mod = torch.nn.Module()
        mod.gcn1 = m.GCN(types.SimpleNamespace(feature_dim=LC))
        mod.conv1 = torch.nn.Conv2d(2 * LC, LC, kernel_size=1)
        mod = mod.to(dev)
        call = lambda t: mod.gcn1.forward_cat_compress(gd, t, mod.conv1)  # noqa: E731
    elif kind == "stack":
        mod = m.GCNStack(types.SimpleNamespace(feature_dim=LC, gcn_layers=layers, gcn_combine="cat_compress")).to(dev)
        call = lambda t: mod(gd, t)  # noqa: E731
    else:
        mod = m.multi_view_dgl_model(types.SimpleNamespace(feature_dim=LC, compress_gcn=True, multi_gcn=False)).to(dev)

        def call(t):
            gd.ndata["image"] = t
            return mod(gd)
    xT, GT = x.to(T), G.to(T)
    params = {k: v.detach().cpu() for k, v in mod.named_parameters()}
    src, dst = (t.long() for t in g.edges())
    _, ref_dx, ref_grads = stack_ref.run(params, xT, g.edata["pose"].double(), src, dst, GT, torch.float64,
                                         layers=layers, combine="cat_compress")
    with torch.no_grad():
        ref32 = call(xT.float().to(dev)).cpu().numpy()

    out, dx, grads, moved, moved_agg = _run(mod, call, _cl(xT, dev), _cl(GT, dev))
    assert out.dtype == T and _is_cl(out) and dx.dtype == T and _is_cl(dx)
    assert moved == {"fwd_cl_" + key: layers, "dgrad_cl_" + key: layers, "wgrad_cl_" + key: layers}, moved
    assert moved_agg == {"fwd_cl_" + key: layers, "bwd_cl_" + key: layers}, moved_agg
    for k, gr in grads.items():
        assert gr.dtype == torch.float32 and bool(torch.isfinite(gr).all()), k
    e = rel_err(out.float().cpu().numpy(), ref32)
    print("cl", key, case, "out rel_err", e, "bar", 2 * layers * hc.UNIT[T])
    assert e <= 2 * layers * hc.UNIT[T]
    native = _group_errs(dx, grads, ref_dx, ref_grads)

    prev = compress.set_half_compress("torch")
    try:
        _, dx_t, grads_t, moved_t, _ = _run(mod, call, xT.to(dev), GT.to(dev), autocast_dtype=T)
        assert moved_t == {"torch_16": layers}, moved_t
        torch_route = _group_errs(dx_t, grads_t, ref_dx, ref_grads)
    finally:
        assert compress.set_half_compress(prev) == "torch"
    for grp in ("dx", "conv", "encoder"):
        print("cl", key, case, grp, "err native / torch route:", native[grp], torch_route[grp])
        assert native[grp] <= 1.5 * torch_route[grp], (grp, native, torch_route)


# ---- routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_convert_route_is_the_previous_behaviour(cuda_device, key):
    """``set_channels_last_compress("convert")`` (and ``aggregate.set_channels_last("convert")``): the NCHW
    kernels on converted operands — NCHW results, bit-equal to the NCHW run; only the node-major keys and
    ``convert_cl`` move."""
    T, dev = hc.DTYPES[key], cuda_device
    C, n, H, W = SHAPES[0]
    w, b, x, a, gy, ref = _case(C, n, H, W, key)
    w, b = w.to(dev), b.to(dev)
    nm = [t.to(dev) for t in (x, a, gy)]
    y_ref = compress._fwd(w, b, nm[0], nm[1])
    gx_ref, ga_ref = compress._bwd_data(w, nm[2], T, like=nm[0])
    gw_ref, gb_ref = compress._bwd_weight(nm[2], nm[0], nm[1], True, None, None)
    xc, ac, gc = (_cl(t, dev) for t in (x, a, gy))
    for setter in (compress.set_channels_last_compress, aggregate.set_channels_last):
        assert setter("convert") == "native"
        try:
            before = _counts()
            y = compress._fwd(w, b, xc, ac)
            gx, ga = compress._bwd_data(w, gc, T, like=xc)
            gw, gb = compress._bwd_weight(gc, xc, ac, True, None, None)
            assert _moved(before) == {"fwd_" + key: 1, "dgrad_" + key: 1, "wgrad_" + key: 1, "convert_cl": 3}
        finally:
            assert setter("native") == "convert"
        for got, want in ((y, y_ref), (gx, gx_ref), (ga, ga_ref)):
            assert got.is_contiguous() and torch.equal(hc.bits(got), hc.bits(want))
        assert torch.equal(gw, gw_ref) and torch.equal(gb, gb_ref)
    with pytest.raises(ValueError):
        compress.set_channels_last_compress("library")
    assert compress.channels_last_compress() == "native"


@pytest.mark.parametrize("key", KEYS)
def test_c40_takes_the_convert_route_without_library_gemms(cuda_device, monkeypatch, key):
    """C % 32 != 0 (no reference configuration): the NCHW kernels on zero-padded operands, never torch's GEMMs."""
    def boom(*_a, **_k):
        raise AssertionError("a library GEMM ran on the product path")
    for name in ("_lib_forward", "_lib_backward_data", "_lib_backward_weight"):
        monkeypatch.setattr(compress, name, boom)
    T, dev = hc.DTYPES[key], cuda_device
    C, n, H, W = 40, 2, 4, 4
    w, b, x, a, gy, ref = _case(C, n, H, W, key)
    w, b = (t.to(dev).requires_grad_(True) for t in (w, b))
    x, a = (_cl(t, dev).requires_grad_(True) for t in (x, a))
    before = _counts()
    y = compress.CompressFunction.apply(x, a, w, b)
    y.backward(_cl(gy, dev))
    assert _moved(before) == {"fwd_" + key: 1, "dgrad_" + key: 1, "wgrad_" + key: 1, "convert_cl": 3}
    what = f"cl C=40 {key}"
    for name, got in (("y", y), ("gx", x.grad), ("ga", a.grad)):
        _check_t(got, ref, name, T, what)
    for name, got in (("gw", w.grad), ("gb", b.grad)):
        _check_f32(got, ref, name, what)


def test_fp32_channels_last_is_unchanged(cuda_device):
    """fp32 channels_last features keep the convert route (the split-bf16 NCHW kernels): NCHW results,
    bit-equal to the run on the contiguous input; no ``_cl`` key and not ``convert_cl`` moves."""
    dev = cuda_device
    C, n, H, W = SHAPES[0]
    gen = torch.Generator().manual_seed(77)
    w = (torch.randn(C, 2 * C, 1, 1, generator=gen) / (2 * C) ** 0.5).to(dev)
    b = torch.randn(C, generator=gen).to(dev)
    x, a, gy = (torch.randn(n, C, H, W, generator=gen).to(dev) for _ in range(3))
    want = (compress._fwd(w, b, x, a), *compress._bwd_data(w, gy, like=x), *compress._bwd_weight(gy, x, a, True, None, None))
    before = _counts()
    xc, ac, gc = (t.contiguous(memory_format=CL) for t in (x, a, gy))
    got = (compress._fwd(w, b, xc, ac), *compress._bwd_data(w, gc, like=xc),
           *compress._bwd_weight(gc, xc, ac, True, None, None))
    assert _moved(before) == {"fwd_f32": 1, "dgrad_f32": 1, "wgrad_f32": 1}
    for g_, w_ in zip(got, want):
        assert g_.is_contiguous() and torch.equal(g_, w_)


def test_compress_1x1_reads_a_channels_last_cat_buffer_in_place(cuda_device):
    """``compress_1x1`` on a channels_last (N, 2C, H, W) buffer: its halves with pixel stride 2C."""
    T, dev, key = torch.bfloat16, cuda_device, "bf16"
    C, n, H, W = SHAPES[0]
    w, b, x, a, gy, ref = _case(C, n, H, W, key)
    conv = torch.nn.Conv2d(2 * C, C, kernel_size=1).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    h = _cl(torch.cat((x, a), 1), dev).requires_grad_(True)
    before = _counts()
    y = compress.compress_1x1(conv, h)
    y.backward(_cl(gy, dev))
    assert _moved(before) == {"fwd_cl_" + key: 1, "dgrad_cl_" + key: 1, "wgrad_cl_" + key: 1}
    assert _is_cl(y)
    _check_t(y, ref, "y", T, "compress_1x1 cl")
    _check_t(h.grad[:, :C], ref, "gx", T, "compress_1x1 cl")
    _check_t(h.grad[:, C:], ref, "ga", T, "compress_1x1 cl")
    _check_f32(conv.weight.grad, ref, "gw", "compress_1x1 cl")
    _check_f32(conv.bias.grad, ref, "gb", "compress_1x1 cl")


def test_backward_follows_the_forwards_route(cuda_device):
    """The route is decided once, in the forward: toggling ``set_channels_last_compress`` between forward
    and backward does not move the backward to the other kernel family (either way round)."""
    T, dev, key = torch.bfloat16, cuda_device, "bf16"
    g, x, G = _frames((5, 5), None, seed=13)
    gd = g.to(dev)
    torch.manual_seed(5)
    mod = m.GCNStack(types.SimpleNamespace(feature_dim=LC, gcn_layers=1, gcn_combine="cat_compress")).to(dev)
    want = {"native": {"fwd_cl_" + key: 1, "dgrad_cl_" + key: 1, "wgrad_cl_" + key: 1},
            "convert": {"fwd_" + key: 1, "dgrad_" + key: 1, "wgrad_" + key: 1, "convert_cl": 3}}
    outs = {}
    for first, then in (("native", "convert"), ("convert", "native")):
        leaf = _cl(x.to(T), dev).requires_grad_(True)
        mod.zero_grad(set_to_none=True)
        before, before_agg = _counts(), dict(aggregate.PATH_COUNTS)
        compress.set_channels_last_compress(first)
        try:
            out = mod(gd, leaf)
            compress.set_channels_last_compress(then)
            out.backward(_cl(G.to(T), dev))
        finally:
            compress.set_channels_last_compress("native")
        assert _moved(before) == want[first], (first, _moved(before))
        agg = "_cl_" if first == "native" else "_"
        assert _moved(before_agg, aggregate.PATH_COUNTS) == {"fwd" + agg + key: 1, "bwd" + agg + key: 1}
        outs[first] = (out.detach(), leaf.grad, mod.conv1.weight.grad.clone())
    # the two families compute the same layer (§3.8's contract either way)
    assert stack_ref.err(outs["native"][0], outs["convert"][0].double().cpu()) <= 2 * hc.UNIT[T]


@pytest.fixture
def world1():
    import socket
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


def test_parameter_gradients_land_in_the_reducers_buckets(cuda_device, world1):
    """A gradient all-reducer attached to a two-layer bf16 channels_last ``cat_compress`` stack (one rank,
    as ``tests/test_gpu_dist.py``): both layers' ``dW`` / ``db`` from ``mrp_compress_bwd_weight_cl`` are written
    in their bucket slots by the kernel (the step's copies number at most the other parameters; measured: 8 of
    12 parameters on this route, 12 on the NCHW route's first step), every gradient lies in its bucket, 16-byte
    aligned, and is bit-equal to the run without a reducer."""
    from mrp_gnn_amd.dist import GradAllReducer
    T, dev, key = torch.bfloat16, cuda_device, "bf16"
    g, x, G = _frames((5, 5), None, seed=17)
    gd = g.to(dev)
    xT, GT = _cl(x.to(T), dev), _cl(G.to(T), dev)

    def make():
        torch.manual_seed(0)
        return m.GCNStack(types.SimpleNamespace(feature_dim=LC, gcn_layers=2, gcn_combine="cat_compress")).to(dev)
    ref = make()
    ref(gd, xT).backward(GT)
    net = make()
    red = GradAllReducer(net.parameters())
    try:
        # the NCHW route's copy count on the same input is the yardstick ("as on the NCHW route")
        for p in net.parameters():
            p.grad = None
        copies = red.copies
        red.arm()
        net(gd, xT.contiguous()).backward(GT.contiguous())
        red.synchronize()
        nchw_copies = red.copies - copies
        for step in range(2):
            for p in net.parameters():
                p.grad = None
            copies, before = red.copies, _counts()
            red.arm()
            net(gd, xT).backward(GT)
            red.synchronize()
            assert _moved(before) == {"fwd_cl_" + key: 2, "dgrad_cl_" + key: 2, "wgrad_cl_" + key: 2}
            print("reducer copies per step: channels_last", red.copies - copies, "nchw", nchw_copies)
            # every parameter whose gradient a kernel did not write in its slot costs one copy: the four
            # compress parameters (two layers' weight and bias) are not among them
            nparams = sum(1 for _ in net.parameters())
            assert red.copies - copies <= nparams - 4, (step, red.copies - copies, nchw_copies)
            for (k, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
                flat = red._flat[red._bucket_of[id(p)]]
                assert flat.data_ptr() <= p.grad.data_ptr() < flat.data_ptr() + flat.numel() * 4, k
                assert p.grad.data_ptr() % 16 == 0, k
                assert torch.equal(p.grad, q.grad), k
    finally:
        red.remove()


# ---- capture --------------------------------------------------------------------------------------------
def test_capture_and_replay(cuda_device):
    """One no-grad bf16 channels_last layer (pixel-major aggregation + compress) and one backward whose weight
    gradient takes a workspace (3 splits), captured into a graph and replayed, equal the eager run."""
    dev, T = cuda_device, torch.bfloat16
    g, x, G = _frames((5, 5), None, seed=9)
    csr = g.csr(dev)
    gen = torch.Generator().manual_seed(9)
    gb = torch.sigmoid(torch.randn(g.num_edges(), LC, 2, generator=gen)).to(dev)
    torch.manual_seed(9)
    conv = torch.nn.Conv2d(2 * LC, LC, kernel_size=1).to(dev)
    x, G = _cl(x.to(T), dev), _cl(G.to(T), dev)
    a = _cl(torch.randn(x.shape, generator=gen).to(T), dev)
    lib = m.load_library()
    assert lib.mrp_tuning_set(b"half_cl_splits", 3) == 0
    try:
        assert lib.mrp_compress_bwd_weight_cl_workspace(x.shape[0], LC, LHW * LHW) > 0

        def work():
            y = compress.film_compress(conv, x, gb, csr, _lib.MODE_FILM_MEAN)
            gx, ga = compress.compress_backward_data(conv.weight, G)
            gw, gbias = compress.compress_backward_weight(G, x, a)
            return y, gx, ga, gw, gbias

        with torch.no_grad():
            eager = work()
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                work()  # warm the allocator and the weight images outside the capture
                torch.cuda.current_stream().synchronize()
                with torch.cuda.graph(graph, stream=side):
                    outs = work()
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
    finally:
        assert lib.mrp_tuning_set(b"half_cl_splits", 0) == 0
    assert _is_cl(outs[0]) and outs[0].dtype == T
    for o, e in zip(outs, eager):
        assert torch.equal(hc.bits(o) if o.dtype == T else o, hc.bits(e) if e.dtype == T else e)
