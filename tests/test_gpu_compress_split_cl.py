"""GPU: the split-bf16 1x1 compress and both gradients on pixel-major (``torch.channels_last``) fp32 feature
maps (``csrc/compress_split_cl.hip``: ``mrp_compress_fwd_split_cl`` / ``_bwd_data_split_cl`` /
``_bwd_weight_split_cl``), behind ``compress.set_channels_last_compress_fp32("native")``, through
``compress.py``, ``compress_1x1``, ``GCNStack`` and ``multi_view_dgl_model``.

Yardsticks: float64 with ``stack_ref.within`` (4 x torch's fp32 CPU error, floor 1e-5) at the tile-geometry
shapes; ``split_cases.within_fp32`` (2 x torch's fp32 error, no floor) at K = 1024; bit-equality with the
float64 product on the lattice operands of ``split_cases`` / ``precision_cases`` in every precision mode; the
derived truncation bound of ``tests/test_gpu_compress_precision.py`` for the reduced modes on random operands.
Bit-equality with the NCHW kernels is not required (the k order inside one MFMA differs); whether it happens
is printed.

Tile geometry the shapes are named against: 256 x 128 output tiles (channels x pixel rows in the forward
and data gradient), 32-k stages (32 pixel rows in the weight gradient), two LDS buffers."""
import contextlib
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import aggregate, compress
import precision_cases as pc
import span_cases as sp
import split_cases as sc
import stack_ref

pytestmark = pytest.mark.gpu

CL = torch.channels_last
#: (C, Nt, H, W): what it reaches
SHAPES = [
    (32, 3, 8, 8),   # partial row tile (M = 32 / 64 of 256), 192 pixel rows: a full and a ragged column tile
    (96, 2, 8, 8),   # K = 6 stages forward, the buffer ring wraps
    (256, 2, 8, 8),  # whole tiles; the data gradient's M = 512: gx and ga land in different row tiles
    (64, 5, 7, 7),   # P = 49: weight-gradient stages cross node boundaries, 245 rows: the last stage is ragged
    (64, 1, 1, 3),   # fewer pixel rows than one stage
]
MODES = ("highest", "high", "medium")
CL_KEYS = {"fwd_cl_f32": 1, "dgrad_cl_f32": 1, "wgrad_cl_f32": 1}


@contextlib.contextmanager
def _native():
    """The opt-in switch on; ``"convert"`` (the default) restored on the way out."""
    prev = compress.set_channels_last_compress_fp32("native")
    try:
        yield
    finally:
        compress.set_channels_last_compress_fp32("convert")
    assert prev == "convert"


@functools.lru_cache(maxsize=None)
def _case(C, n, H, W):
    """CPU fp32 operands (NCHW) and the float64 / fp32 references, computed once."""
    gen = torch.Generator().manual_seed(C * 1013 + n * 37 + H * 7 + W)
    w = torch.randn(C, 2 * C, 1, 1, generator=gen) / (2 * C) ** 0.5
    b = torch.randn(C, generator=gen)
    x, a, gy = (torch.randn(n, C, H, W, generator=gen) for _ in range(3))
    ref = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        w2 = w.reshape(C, 2 * C).to(dt)
        cat, g = torch.cat((x, a), 1).to(dt), gy.to(dt)
        y = torch.einsum("oc,nchw->nohw", w2, cat) + b.to(dt)[None, :, None, None]
        gcat = torch.einsum("oc,nohw->nchw", w2, g)
        ref[tag] = dict(y=y, gx=gcat[:, :C], ga=gcat[:, C:],
                        gw=torch.einsum("nohw,nchw->oc", g, cat).reshape(C, 2 * C, 1, 1), gb=g.sum((0, 2, 3)))
    return w, b, x, a, gy, ref


def _cl(t, dev):
    return t.to(dev).contiguous(memory_format=CL)


def _check(got, ref, name, what):
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


def _products(w, b, x, a, gy):
    y = compress.compress_forward(w, b, x, a)
    gx, ga = compress.compress_backward_data(w, gy)
    gw, gb = compress._bwd_weight(gy, x, a, True, None, None)
    return y, gx, ga, gw, gb


# ---- 1. the float64 yardstick ---------------------------------------------------------------------------

@pytest.mark.parametrize("C,n,H,W", SHAPES)
def test_products_match_float64(cuda_device, C, n, H, W):
    """Mode "highest": all five outputs against the bar, dense channels_last outputs, only the three
    ``*_cl_f32`` counters move, a second run gives the same bits."""
    dev = cuda_device
    w, b, x, a, gy, ref = _case(C, n, H, W)
    w, b = w.to(dev), b.to(dev)
    x, a, gy = (_cl(t, dev) for t in (x, a, gy))
    what = f"cl f32 {(C, n, H, W)}"
    with _native():
        before = _counts()
        outs = _products(w, b, x, a, gy)
        assert _moved(before) == CL_KEYS
        again = _products(w, b, x, a, gy)
    for name, got in zip(("y", "gx", "ga", "gw", "gb"), outs):
        if name in ("y", "gx", "ga"):
            assert _is_cl(got), (what, name, got.stride())
        _check(got, ref, name, what)
    for name, p, q in zip(("y", "gx", "ga", "gw", "gb"), outs, again):
        assert torch.equal(p, q), (what, name, "a second run differs")
    if H * W % 32 == 0:  # informational: the NCHW kernels on the same operands
        nchw = _products(w, b, x.contiguous(), a.contiguous(), gy.contiguous())
        print(what, "bit-equal to the NCHW kernels:",
              {k: torch.equal(p.contiguous(), q) for k, p, q in zip(("y", "gx", "ga", "gw", "gb"), outs, nchw)})


# ---- 2. the fp32 claim at K = 1024 ----------------------------------------------------------------------

FACTOR = 2.0


def _claim(ours, f32, f64, what):
    ok, (e, e32) = sc.within_fp32(ours, f32, f64, FACTOR)
    print(f"\nRATIO {what}: ours {e:.3g} / fp32 {e32:.3g} = {e / e32:.3f}")
    assert ok, f"{what}: error {e:.3g} against float64 is {e / e32:.2f} x the fp32 GEMM's {e32:.3g} (bound {FACTOR:g} x)"


def _rows(t, dt):
    return t.to(dt).permute(1, 0, 2).reshape(t.shape[1], -1)


def _planes(t, dev=None):
    """(n, C, P) -> a channels_last (n, C, 4, P / 4) map with the same (node, channel, pixel) values."""
    n, C, P = t.shape
    t = t.reshape(n, C, 4, P // 4)
    return (t if dev is None else t.to(dev)).contiguous(memory_format=CL)


def test_forward_and_data_gradient_within_fp32(cuda_device):
    """n = 2, C = 512, P = 32: K = 2C = 1024 forward, K = C = 512 data gradient (``test_gpu_split_fp32.py``'s
    shape, factor and references)."""
    dev = cuda_device
    torch.manual_seed(11)
    n, C, P = 2, 512, 32
    w = torch.randn(C, 2 * C, device=dev) * (2 * C) ** -0.5
    b = torch.randn(C, device=dev)
    cat = torch.randn(n, 2 * C, P, device=dev)
    gy = torch.randn(n, C, P, device=dev)
    ref = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        ref[name] = (torch.matmul(w.to(dt), cat.to(dt)) + b.to(dt)[None, :, None], torch.matmul(w.to(dt).t(), gy.to(dt)))
    x, a = (_planes(cat[:, i * C:(i + 1) * C]) for i in (0, 1))
    with _native():
        before = _counts()
        y = compress.compress_forward(w.view(C, 2 * C, 1, 1), b, x, a)
        gx, ga = compress.compress_backward_data(w.view(C, 2 * C, 1, 1), _planes(gy))
        assert _moved(before) == {"fwd_cl_f32": 1, "dgrad_cl_f32": 1}
    _claim(y.reshape(n, C, P), ref["f32"][0], ref["f64"][0], "compress fwd split_cl")
    _claim(torch.cat((gx, ga), 1).reshape(n, 2 * C, P), ref["f32"][1], ref["f64"][1], "compress dgrad split_cl")


def test_weight_gradient_within_fp32(cuda_device):
    """n = 32, C = 64, P = 32 (K = n P = 1024)."""
    dev = cuda_device
    torch.manual_seed(12)
    n, C, P = 32, 64, 32
    gy = torch.randn(n, C, P, device=dev) * (n * P) ** -0.5
    cat = torch.randn(n, 2 * C, P, device=dev)
    ref = {name: _rows(gy, dt) @ _rows(cat, dt).t() for name, dt in (("f32", torch.float32), ("f64", torch.float64))}
    x, a = (_planes(cat[:, i * C:(i + 1) * C]) for i in (0, 1))
    with _native():
        before = _counts()
        gw, gb = compress.compress_backward_weight(_planes(gy), x, a)
        assert _moved(before) == {"wgrad_cl_f32": 1}
    _claim(gw.view(C, 2 * C), ref["f32"], ref["f64"], "compress wgrad split_cl")


# ---- 3. lattice exactness per mode ----------------------------------------------------------------------

LATTICE_SHAPES = ((3, 64, 32), (3, 256, 32), (5, 64, 49))
PLANE = {32: (4, 8), 49: (7, 7)}


@functools.lru_cache(maxsize=None)
def _lattice_refs(n, C, P, pairing, mode):
    if mode == "highest":
        return sc.compress_refs(pc.compress_case(n, C, P, pairing))
    return pc.compress_trunc_refs(n, C, P, pairing, pc.PARTS[mode])


def _lat(t, P, dev):
    n, C, _ = t.shape
    return t.reshape(n, C, *PLANE[P]).to(dev).contiguous(memory_format=CL)


def _ncp(t):
    return t.reshape(t.shape[0], t.shape[1], -1)


@pytest.mark.parametrize("n,C,P", LATTICE_SHAPES)
@pytest.mark.parametrize("pairing", sc.PAIRINGS, ids=sc.pairing_id)
@pytest.mark.parametrize("mode", MODES)
def test_lattice_operands_give_the_modes_products_bit_for_bit(cuda_device, mode, pairing, n, C, P):
    """Every output equals the float64 sum of the mode's partial products (mode "highest": the float64
    product itself) bit for bit; ``gb`` is exact in every mode; the weight gradient also with the split count
    forced to 1, 2 and 5."""
    dev = cuda_device
    c = pc.compress_case(n, C, P, pairing)
    ref = _lattice_refs(n, C, P, pairing, mode)
    w = c["w"].view(C, 2 * C, 1, 1).to(dev)
    b = c["b"].to(dev)
    x, a, gy, gy_s, xs, as_ = (_lat(c[k], P, dev) for k in ("x", "a", "gy", "gy_s", "xs", "as_"))
    tag = f"{mode} {sc.pairing_id(pairing)} n={n} C={C} P={P}"
    suffix = "" if mode == "highest" else "_" + mode
    with _native(), compress.compress_precision_scope(mode):
        before = _counts()
        y = compress.compress_forward(w, b, x, a)
        gx, ga = compress.compress_backward_data(w, gy)
        assert _moved(before) == {"fwd_cl_f32" + suffix: 1, "dgrad_cl_f32" + suffix: 1}, tag
        sc.assert_bit_equal(_ncp(y), ref["y"], f"y {tag}")
        sc.assert_bit_equal(_ncp(gx), ref["gx"], f"gx {tag}")
        sc.assert_bit_equal(_ncp(ga), ref["ga"], f"ga {tag}")
        for splits in (0, 1, 2, 5):
            with sc.knobs("split", split_cl_splits=splits):
                before = _counts()
                gw, gb = compress.compress_backward_weight(gy_s, xs, as_)
                assert _moved(before) == {"wgrad_cl_f32" + suffix: 1}, tag
            sc.assert_bit_equal(gw.view(C, 2 * C), ref["gw"], f"gw {tag} splits={splits}")
            sc.assert_bit_equal(gb, ref["gb"], f"gbias (the row sums of the full gy) {tag} splits={splits}")


# ---- 4. the reduced modes on random operands ------------------------------------------------------------

def _bounded(got, f64, f32, mag, mode, what):
    """|got - f64| <= c (|A| |B|) + 2 max |torch_fp32 - f64| elementwise (``test_gpu_compress_precision.py``)."""
    e32 = float((f32.double() - f64).abs().max())
    d = (got.double().cpu() - f64).abs()
    bound = pc.TERM_BOUND[mode] * mag + 2.0 * e32
    worst = float((d / bound).max())
    e = stack_ref.err(got, f64)
    print(f"\nPRECISION cl {what} {mode}: err {e:.3g}, worst |d| / bound {worst:.3f}, fp32 yardstick {e32:.3g}")
    assert worst <= 1.0, f"{what} {mode}: |got - f64| reaches {worst:.3f} x the derived bound"
    return e


@pytest.mark.parametrize("C,n,H,W", [SHAPES[1], SHAPES[3]])
def test_reduced_modes_on_random_operands_within_the_derived_bound(cuda_device, C, n, H, W):
    dev = cuda_device
    w, b, x, a, gy, ref = _case(C, n, H, W)
    w2, cat = w.reshape(C, 2 * C).double().abs(), torch.cat((x, a), 1).double().abs()
    mag = {"y": torch.einsum("oc,nchw->nohw", w2, cat) + b.double().abs()[None, :, None, None],
           "g": torch.einsum("oc,nohw->nchw", w2, gy.double().abs()),
           "gw": torch.einsum("nohw,nchw->oc", gy.double().abs(), cat).reshape(C, 2 * C, 1, 1)}
    wd, bd = w.to(dev), b.to(dev)
    xd, ad, gd = (_cl(t, dev) for t in (x, a, gy))
    errs = {}
    for mode in pc.REDUCED:
        with _native(), compress.compress_precision_scope(mode):
            before = _counts()
            y, gx, ga, gw, gb = _products(wd, bd, xd, ad, gd)
            assert _moved(before) == {k + "_" + mode: 1 for k in CL_KEYS}
        what = f"{(C, n, H, W)}"
        r64, r32 = ref["64"], ref["32"]
        errs[mode] = {
            "fwd": _bounded(y, r64["y"], r32["y"], mag["y"], mode, "fwd " + what),
            "dgrad": _bounded(torch.cat((gx, ga), 1), torch.cat((r64["gx"], r64["ga"]), 1),
                              torch.cat((r32["gx"], r32["ga"]), 1), mag["g"], mode, "dgrad " + what),
            "wgrad": _bounded(gw, r64["gw"], r32["gw"], mag["gw"], mode, "wgrad " + what)}
        _check(gb, ref, "gb", f"gb {mode} {what}")  # the fp32 sum of the full gy in every mode
    for op in ("fwd", "dgrad", "wgrad"):
        assert errs["high"][op] < errs["medium"][op], (op, errs)


# ---- 5. strided operands --------------------------------------------------------------------------------

def test_halves_of_channels_last_buffers_and_compress_1x1(cuda_device):
    """x and agg as the halves of one channels_last (N, 2C, H, W) buffer (pixel stride 2C), gx and ga written
    into the halves of another; ``compress_1x1`` on that buffer: all equal to the dense run's bits."""
    dev = cuda_device
    C, n, H, W = SHAPES[0]
    w, b, x, a, gy, ref = _case(C, n, H, W)
    w, b = w.to(dev), b.to(dev)
    xd, ad, gd = (_cl(t, dev) for t in (x, a, gy))
    cat = _cl(torch.cat((x, a), 1), dev)
    xv, av = cat[:, :C], cat[:, C:]
    assert aggregate.pixel_strides(xv) == (H * W * 2 * C, 2 * C) == aggregate.pixel_strides(av)
    sentinel = -7.0
    gcat = torch.full((n + 1, 2 * C, H, W), sentinel, device=dev).contiguous(memory_format=CL)
    with _native():
        y, gx, ga, gw, gb = _products(w, b, xd, ad, gd)
        before = _counts()
        y2 = compress.compress_forward(w, b, xv, av)
        compress.compress_backward_data(w, gd, gx=gcat[:n, :C], ga=gcat[:n, C:])
        gw2, gb2 = compress.compress_backward_weight(gd, xv, av)
        assert _moved(before) == CL_KEYS
        assert torch.equal(y2, y) and torch.equal(gcat[:n, :C], gx) and torch.equal(gcat[:n, C:], ga)
        assert torch.equal(gw2, gw) and torch.equal(gb2, gb)
        assert bool((gcat[n] == sentinel).all())  # the guard node
        # a half written alone leaves the other half alone
        half = torch.full((n, 2 * C, H, W), sentinel, device=dev).contiguous(memory_format=CL)
        other = torch.empty((n, C, H, W), device=dev).contiguous(memory_format=CL)
        compress.compress_backward_data(w, gd, gx=half[:, :C], ga=other)
        assert torch.equal(half[:, :C], gx) and torch.equal(other, ga) and bool((half[:, C:] == sentinel).all())

        conv = torch.nn.Conv2d(2 * C, C, kernel_size=1).to(dev)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        h = cat.clone(memory_format=torch.preserve_format).requires_grad_(True)
        before = _counts()
        yc = compress.compress_1x1(conv, h)
        yc.backward(gd)
        assert _moved(before) == CL_KEYS
    assert _is_cl(yc)
    assert torch.equal(yc.detach(), y) and torch.equal(h.grad[:, :C], gx) and torch.equal(h.grad[:, C:], ga)
    assert torch.equal(conv.weight.grad, gw) and torch.equal(conv.bias.grad, gb)
    for name, got in (("y", yc.detach()), ("gx", h.grad[:, :C]), ("ga", h.grad[:, C:]), ("gw", conv.weight.grad),
                      ("gb", conv.bias.grad)):
        _check(got, ref, name, "compress_1x1 cl f32")


# ---- 6. layer and model ---------------------------------------------------------------------------------

LC, LHW = 64, 5
#: name -> (node counts, k-NN k or None, layers, module)
LAYER_CASES = {"stack2_complete_5": ((5, 5), None, 2, "stack"), "stack2_knn4_16": ((16,), 4, 2, "stack"),
               "model_complete_5": ((5, 5), None, 1, "model"), "model_knn4_16": ((16,), 4, 1, "model")}


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


def _module(kind, layers, gd, dev):
    torch.manual_seed(5)
    if kind == "stack":
        mod = m.GCNStack(types.SimpleNamespace(feature_dim=LC, gcn_layers=layers, gcn_combine="cat_compress")).to(dev)
        return mod, lambda t: mod(gd, t)
    mod = m.multi_view_dgl_model(types.SimpleNamespace(feature_dim=LC, compress_gcn=True, multi_gcn=False)).to(dev)

    def call(t):
        gd.ndata["image"] = t
        return mod(gd)
    return mod, call


def _run(mod, call, x_dev, G_dev, between=None):
    for p in mod.parameters():
        p.grad = None
    leaf = x_dev.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    before, before_agg = _counts(), dict(aggregate.PATH_COUNTS)
    out = call(leaf)
    fwd_moved = _moved(before)
    if between is not None:
        between()
    out.backward(G_dev)
    grads = {k: p.grad.detach().clone() for k, p in mod.named_parameters()}
    return out.detach(), leaf.grad, grads, _moved(before), _moved(before_agg, aggregate.PATH_COUNTS), fwd_moved


@pytest.mark.parametrize("case", list(LAYER_CASES))
def test_layer_and_model_stay_channels_last(cuda_device, case):
    """fp32 channels_last features through a two-layer ``GCNStack(cat_compress)`` and
    ``multi_view_dgl_model(compress_gcn)``: channels_last output and leaf gradient, one pixel-major
    aggregation forward / backward and one of each pixel-major compress product per layer; the output, dx and
    every parameter gradient against float64 (``stack_ref.run``) with ``stack_ref.within``."""
    dev = cuda_device
    ns, knn, layers, kind = LAYER_CASES[case]
    g, x, G = _frames(ns, knn, seed=31 + layers)
    gd = g.to(dev)
    mod, call = _module(kind, layers, gd, dev)
    params = {k: v.detach().cpu() for k, v in mod.named_parameters()}
    src, dst = (t.long() for t in g.edges())
    ref = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        ref[tag] = stack_ref.run(params, x, g.edata["pose"].to(dt), src, dst, G, dt, layers=layers,
                                 combine="cat_compress")
    with _native():
        out, dx, grads, moved, moved_agg, _ = _run(mod, call, _cl(x, dev), _cl(G, dev))
    assert _is_cl(out) and _is_cl(dx), (out.stride(), dx.stride())
    assert moved == {k: layers for k in CL_KEYS}, moved
    assert moved_agg == {"fwd_cl_f32": layers, "bwd_cl_f32": layers}, moved_agg

    def hold(got, i, key, name):
        f32, f64 = (ref[t][i] if key is None else ref[t][i][key] for t in ("32", "64"))
        ok, errs = stack_ref.within(got, f32, f64)
        print("cl f32", case, name, "err, fp32 torch err", errs)
        assert ok, (case, name, errs)
    hold(out, 0, None, "out")
    hold(dx, 1, None, "dx")
    for k, gr in grads.items():
        hold(gr, 2, k, k)


def test_backward_follows_the_forwards_route_and_precision(cuda_device):
    """The route is decided once, in the forward: toggling the switch between forward and backward does not
    move the backward, either way round; a node created under ``compress_precision_scope("high")`` runs both
    gradients on the ``_high`` keys after the scope ends."""
    dev = cuda_device
    g, x, G = _frames((5, 5), None, seed=13)
    gd = g.to(dev)
    mod, call = _module("stack", 1, gd, dev)
    xd, Gd = _cl(x, dev), _cl(G, dev)
    want = {"native": CL_KEYS, "convert": {"fwd_f32": 1, "dgrad_f32": 1, "wgrad_f32": 1}}
    outs = {}
    try:
        for first, then in (("native", "convert"), ("convert", "native")):
            compress.set_channels_last_compress_fp32(first)
            out, dx, grads, moved, moved_agg, _ = _run(
                mod, call, xd, Gd, between=lambda: compress.set_channels_last_compress_fp32(then))
            assert moved == want[first], (first, moved)
            agg = "_cl_" if first == "native" else "_"
            assert moved_agg == {"fwd" + agg + "f32": 1, "bwd" + agg + "f32": 1}, (first, moved_agg)
            assert _is_cl(out) == (first == "native")
            outs[first] = out
        assert stack_ref.err(outs["native"], outs["convert"]) <= 1e-5

        compress.set_channels_last_compress_fp32("native")
        state = {}

        def forward(t):
            with compress.compress_precision_scope("high"):
                return call(t)
        out, dx, grads, moved, _, fwd_moved = _run(mod, forward, xd, Gd,
                                                   between=lambda: state.update(mode=compress.compress_precision()))
        assert state["mode"] == "highest"  # the scope had ended before the backward ran
        assert fwd_moved == {"fwd_cl_f32_high": 1}
        assert moved == {"fwd_cl_f32_high": 1, "dgrad_cl_f32_high": 1, "wgrad_cl_f32_high": 1}, moved
    finally:
        compress.set_channels_last_compress_fp32("convert")


# ---- 7. route conditions --------------------------------------------------------------------------------

def _no_library_gemm(monkeypatch):
    def boom(*_a, **_k):
        raise AssertionError("a library GEMM ran on the product path")
    for name in ("_lib_forward", "_lib_backward_data", "_lib_backward_weight"):
        monkeypatch.setattr(compress, name, boom)


@pytest.mark.parametrize("why", ["c40", "hip_path", "aggregate_convert", "split_ops"])
def test_other_conditions_keep_the_convert_route(cuda_device, monkeypatch, why):
    """With the switch on, C % 32 != 0, ``set_compress_path("hip")``, ``aggregate.set_channels_last("convert")``
    and a narrowed ``split_ops`` still take the convert route: NCHW results on the ``*_f32`` keys, no library
    GEMM."""
    _no_library_gemm(monkeypatch)
    dev = cuda_device
    C, n, H, W = (40, 2, 4, 4) if why == "c40" else SHAPES[0]
    w, b, x, a, gy, ref = _case(C, n, H, W)
    w, b = (t.to(dev).requires_grad_(True) for t in (w, b))
    x, a = (_cl(t, dev).requires_grad_(True) for t in (x, a))
    try:
        if why == "hip_path":
            compress.set_compress_path("hip")
        elif why == "aggregate_convert":
            assert aggregate.set_channels_last("convert") == "native"
        elif why == "split_ops":
            compress.set_compress_path("split", split_ops=("fwd", "dgrad"))
        with _native():
            before = _counts()
            y = compress.CompressFunction.apply(x, a, w, b)
            y.backward(_cl(gy, dev))
            assert _moved(before) == {"fwd_f32": 1, "dgrad_f32": 1, "wgrad_f32": 1}
    finally:
        compress.set_compress_path("split", split_ops=("fwd", "dgrad", "wgrad"))
        aggregate.set_channels_last("native")
    assert y.is_contiguous()  # (autograd lays a leaf's .grad out like the leaf, whatever the function returns)
    what = f"convert route ({why})"
    for name, got in (("y", y.detach()), ("gx", x.grad), ("ga", a.grad), ("gw", w.grad), ("gb", b.grad)):
        _check(got, ref, name, what)


def test_default_leaves_fp32_channels_last_on_the_convert_route(cuda_device):
    dev = cuda_device
    assert compress.channels_last_compress_fp32() == "convert"
    w, b, x, a, gy, ref = _case(*SHAPES[0])
    before = _counts()
    outs = _products(w.to(dev), b.to(dev), *(_cl(t, dev) for t in (x, a, gy)))
    assert _moved(before) == {"fwd_f32": 1, "dgrad_f32": 1, "wgrad_f32": 1}
    assert all(o.is_contiguous() for o in outs)


# ---- 8. span ----------------------------------------------------------------------------------------------

def _st(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def test_operands_spanning_more_than_4_gib(cuda_device):
    """17 nodes of C = 32, 2 x 3 planes, 2^28 bytes + 64 KiB apart in the sentinel-filled arena of
    ``span_cases`` (node 16 lies beyond 2^32 bytes), x / agg and gx / ga as the halves of channels_last 2C
    buffers: all three products bit-equal to the dense run, no byte touched outside the output blocks."""
    dev = cuda_device
    n, C, H, W = 17, 32, 2, 3
    P = H * W
    gen = torch.Generator().manual_seed(171)
    w = (torch.randn(C, 2 * C, 1, 1, generator=gen) / (2 * C) ** 0.5).to(dev)
    b = torch.randn(C, generator=gen).to(dev)
    x, a, gy = (torch.randn(n, C, H, W, generator=gen) for _ in range(3))
    lib = m.load_library()
    st = _st(dev)
    with _native():
        dense = _products(w, b, *(_cl(t, dev) for t in (x, a, gy)))
    wf, wb = compress.packed_weight(w, "fwd"), compress.packed_weight(w, "bwd")
    arena = sp.Arena(dev)
    try:
        kw = dict(layout="cl", ps=2 * C)
        X = arena.place(x, **kw)
        A = arena.place(a, beside=X, **kw)
        G = arena.place(gy, layout="cl")
        Y = arena.reserve((n, C, H, W), torch.float32, layout="cl")
        GX = arena.reserve((n, C, H, W), torch.float32, **kw)
        GA = arena.reserve((n, C, H, W), torch.float32, beside=GX, **kw)
        ins = [X, A, G]
        assert (n - 1) * sp.NODE_STRIDE >= 1 << 32
        assert lib.mrp_compress_fwd_split_cl(X.ptr, X.ns, X.ps, A.ptr, A.ns, A.ps, n, C, P, _p(wf), _p(b), Y.ptr, Y.ns,
                                             Y.ps, 3, st) == 0
        (y,) = arena.check(ins, [Y])
        assert torch.equal(sp.bits(y), sp.bits(dense[0]))
        assert lib.mrp_compress_bwd_data_split_cl(G.ptr, G.ns, G.ps, n, C, P, _p(wb), GX.ptr, GX.ns, GX.ps, GA.ptr,
                                                  GA.ns, GA.ps, 3, st) == 0
        gx, ga = arena.check(ins, [GX, GA])
        assert torch.equal(sp.bits(gx), sp.bits(dense[1])) and torch.equal(sp.bits(ga), sp.bits(dense[2]))
        nbytes = int(lib.mrp_compress_bwd_weight_split_cl_workspace(n, C, P))
        ws = torch.empty(nbytes // 4 + 4, device=dev)
        gw = torch.full((C, 2 * C, 1, 1), float("nan"), device=dev)
        gb = torch.full((C,), float("nan"), device=dev)
        assert lib.mrp_compress_bwd_weight_split_cl(G.ptr, G.ns, G.ps, X.ptr, X.ns, X.ps, A.ptr, A.ns, A.ps, n, C, P,
                                                    _p(gw), _p(gb), _p(ws), nbytes, 3, st) == 0
        arena.check(ins, [])
        assert torch.equal(gw, dense[3]) and torch.equal(gb, dense[4])
    finally:
        del arena.buf
