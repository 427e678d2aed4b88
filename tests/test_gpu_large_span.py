"""GPU: every feature-map entry point of ``include/mrp_gnn.h`` on operands that span more than 2 and 4 GiB.

The entry points see only pointers and strides, so each feature tensor — inputs and outputs — is a few
tiny node blocks placed ``S = 2^28 bytes + 64 KiB`` apart in a sentinel-filled arena (``span_cases``): node
8 onward lies beyond 2^31 bytes, node 16 onward beyond 2^32 bytes, and an offset that is wrong or truncated
to 32 bits lands inside the arena, where it shows as a wrong value or a touched sentinel.  Parameters,
``gb`` / ``grad_gb``, graph arrays and workspaces are ordinary small tensors.

Each call asserts: the return code is ``span_cases.EXPECTED``'s; an accepted call's outputs agree with the
float64 reference of the operation under the bar the suite already uses for that output
(``half_cases.assert_elementwise`` for bf16 / fp16 outputs, ``stack_ref.within`` for fp32 ``dW`` / ``db`` and
the fp32-MFMA products, ``split_cases.within_fp32`` at the factor of ``test_gpu_split_fp32.py`` for the
split-bf16 products, ``test_gpu_parity.TOL`` for the fp32 aggregation, ``half_cases.assert_relative`` for
a 16-bit aggregation's ``grad_gb``); where the arithmetic cannot depend on the addresses (forward, data
gradient, aggregation forward, ``grad_x``) the output bits equal the same entry point's on a dense copy of
the operands; a declined call wrote nothing; and in both cases no byte outside the permitted blocks was
touched and the inputs hold their bits (``Arena.check``).  The Python routes (``compress.py``,
``aggregate.py``) must return correct values for the same sparse views — a ``RuntimeError`` for a legal
tensor is a failure.

One aggregation case, ``complete_1x16_s512``, is a single 16-node graph with nodes ``2^29 bytes + 64 KiB`` apart: it
spans 2^32 bytes by itself, which no graph of the others does.  The mean's matrix-core backward cannot address
that (32-bit lane offsets over a graph's nodes) and its launcher must run the VALU kernels instead: grad_x and
grad_gb are held to the bits of the dense run with the matrix-core knobs off, and grad_gb must differ from the dense
default-knob run's.

The max-pooled, attention-pooled, confidence-weighted and confidence-gated aggregations
(``mrp_film_{max,attn,wmean,wattn}_{fwd,bwd}``) run on all seven graph sets of ``span_cases.AGG`` with x, out,
grad_out, grad_x, grad_x_base, w and grad_w sparse: every output, the dense fp32 ones included, has the bits of
the dense run, and the dense run is held to the family's own reference under the family's own bar
(``_fam_bars``)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib, aggregate, compress
import attn_cases as ac
import half_cases as hc
import max_cases as mc
import oracle
import span_cases as sp
import split_cases as sc
import stack_ref
import test_gpu_film_attn as t_attn
import test_gpu_film_max as t_max
import test_gpu_film_wattn as t_wattn
import test_gpu_film_wmean as t_wmean
import wattn_cases as wac
import wmean_cases as wmc
from conftest import rel_err
from test_gpu_parity import TOL
from test_gpu_split_fp32 import FACTOR

pytestmark = pytest.mark.gpu

ALL = ["f32", "bf16", "f16"]
HALF = ["bf16", "f16"]
CL = torch.channels_last


@pytest.fixture(scope="module")
def module_arena(cuda_device):
    arena = sp.Arena(cuda_device)
    yield arena
    del arena.buf


@pytest.fixture
def arena(module_arena):
    yield module_arena
    module_arena.clear()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class Dense:
    """An ordinary dense tensor behind the interface of ``span_cases.Placed`` (ptr, ns, ps, read)."""

    def __init__(self, t, layout):
        n, C, H, W = t.shape
        self.t = t.contiguous(memory_format=CL) if layout == "cl" else t.contiguous()
        self.ptr, self.ns, self.ps = _p(self.t), C * H * W, C if layout == "cl" else None
        self.address = self.t.data_ptr()

    def read(self):
        return self.t.cpu().contiguous()


def _dense_in(t, dev, layout):
    return Dense(t.to(dev), layout)


def _dense_out(shape, T, dev, layout):
    return Dense(torch.empty(shape, dtype=T, device=dev), layout)


def _same_bits(a, b, what):
    assert torch.equal(sp.bits(a), sp.bits(b)), f"{what}: the sparse run's bits differ from the dense run's"


# ---- compress -------------------------------------------------------------------------------------------
#: family -> (layout, forward, data gradient, weight gradient entry points)
FAMILY = {
    "hip": ("nchw", "mrp_compress_fwd", "mrp_compress_bwd_data", "mrp_compress_bwd_weight"),
    "split": ("nchw", "mrp_compress_fwd_split", "mrp_compress_bwd_data_split", "mrp_compress_bwd_weight_split"),
    "half": ("nchw", "mrp_compress_fwd_t", "mrp_compress_bwd_data_t", "mrp_compress_bwd_weight_t"),
    "cl": ("cl", "mrp_compress_fwd_cl", "mrp_compress_bwd_data_cl", "mrp_compress_bwd_weight_cl"),
}


def _cref(w, b, x, a, gy, T, dt):
    """(y, gx, ga, gw, gb) of conv(cat(x, a)) in dt by einsum, the weight as the kernels hold it."""
    C = x.shape[1]
    w2 = w.reshape(C, 2 * C).to(T).to(dt)
    cat, g = torch.cat((x, a), 1).to(dt), gy.to(dt)
    y = torch.einsum("oc,nchw->nohw", w2, cat) + b.to(dt)[None, :, None, None]
    gcat = torch.einsum("oc,nohw->nchw", w2, g)
    return dict(y=y, gx=gcat[:, :C], ga=gcat[:, C:], gw=torch.einsum("nohw,nchw->oc", g, cat),
                gb=g.sum((0, 2, 3)))


@functools.lru_cache(maxsize=None)
def _ccase(case, key, dev):
    """CPU operands (w, b fp32; x, a, gy in T) and the float64 / fp32 references, computed once.  The fp32
    reference is torch's on the GPU for fp32 features (``test_gpu_compress_gemm.py``, ``test_gpu_split_fp32.py``)
    and on the CPU for 16-bit ones (``test_gpu_compress_cl.py``).  The parameters on ``dev`` (the arena's
    device) are kept here too, so that ``compress.packed_weight`` packs each weight once."""
    n, C, H, W = sp.COMPRESS[case]
    T = sp.DTYPES[key]
    gen = torch.Generator().manual_seed(C * 1013 + n * 37 + H * 7 + W + ALL.index(key))
    w = torch.randn(C, 2 * C, 1, 1, generator=gen) / (2 * C) ** 0.5
    b = torch.randn(C, generator=gen)
    x, a, gy = (torch.randn(n, C, H, W, generator=gen).to(T) for _ in range(3))
    ref = {"64": _cref(w, b, x, a, gy, T, torch.float64)}
    if key == "f32":
        ref["32"] = {k: v.cpu() for k, v in _cref(*(t.to(dev) for t in (w, b, x, a, gy)), T, torch.float32).items()}
    else:
        ref["32"] = _cref(w, b, x, a, gy, T, torch.float32)
    return dict(w=w, b=b, x=x, a=a, gy=gy, ref=ref, wd=w.to(dev), bd=b.to(dev))


def _bar(fam, key, name, got, c, what):
    ref, T = c["ref"], sp.DTYPES[key]
    if name in ("y", "gx", "ga") and key != "f32":
        assert got.dtype == T
        hc.assert_elementwise(got, ref["64"][name], T, f"{what} {name}")
        return
    assert got.dtype == torch.float32
    if fam == "split" and name != "gb":
        ok, (e, e32) = sc.within_fp32(got, ref["32"][name], ref["64"][name], FACTOR)
    else:
        ok, (e, e32) = stack_ref.within(got, ref["32"][name], ref["64"][name])
    print(f"{what} {name}: err {e:.3g}, fp32 torch err {e32:.3g}")
    assert ok, (what, name, e, e32)


def _call_fwd(fam, lib, key, c, X, A, Y, st):
    n, C, H, W = c["x"].shape
    P, T = H * W, sp.DTYPES[key]
    wd, bd = c["wd"], c["bd"]
    if fam == "hip":
        return lib.mrp_compress_fwd(X.ptr, X.ns, A.ptr, A.ns, n, C, P, _p(wd), _p(bd), Y.ptr, Y.ns, st)
    img = compress.packed_weight(wd, "fwd", T)
    if fam == "split":
        return lib.mrp_compress_fwd_split(X.ptr, X.ns, A.ptr, A.ns, n, C, P, _p(img), _p(bd), Y.ptr, Y.ns, st)
    if fam == "half":
        return lib.mrp_compress_fwd_t(sp.ENUM[key], X.ptr, X.ns, A.ptr, A.ns, n, C, P, _p(img), _p(bd), Y.ptr, Y.ns, st)
    return lib.mrp_compress_fwd_cl(sp.ENUM[key], X.ptr, X.ns, X.ps, A.ptr, A.ns, A.ps, n, C, P, _p(img), _p(bd),
                                   Y.ptr, Y.ns, Y.ps, st)


def _call_dgrad(fam, lib, key, c, G, GX, GA, st):
    n, C, H, W = c["x"].shape
    P, T = H * W, sp.DTYPES[key]
    wd = c["wd"]
    if fam == "hip":
        wt = torch.empty((2 * C, C), device=wd.device, dtype=torch.float32)
        assert lib.mrp_compress_weight_transpose(_p(wd), _p(wt), C, st) == 0
        return lib.mrp_compress_bwd_data(G.ptr, G.ns, n, C, P, _p(wt), GX.ptr, GX.ns, GA.ptr, GA.ns, st)
    img = compress.packed_weight(wd, "bwd", T)
    if fam == "split":
        return lib.mrp_compress_bwd_data_split(G.ptr, G.ns, n, C, P, _p(img), GX.ptr, GX.ns, GA.ptr, GA.ns, st)
    if fam == "half":
        return lib.mrp_compress_bwd_data_t(sp.ENUM[key], G.ptr, G.ns, n, C, P, _p(img), GX.ptr, GX.ns, GA.ptr, GA.ns, st)
    return lib.mrp_compress_bwd_data_cl(sp.ENUM[key], G.ptr, G.ns, G.ps, n, C, P, _p(img), GX.ptr, GX.ns, GX.ps,
                                        GA.ptr, GA.ns, GA.ps, st)


def _call_wgrad(fam, lib, key, c, G, X, A, st):
    """(code, gw (C, 2C), gb (C)) with the workspace the query asks for."""
    n, C, H, W = c["x"].shape
    P, dev = H * W, c["wd"].device
    gw = torch.full((C, 2 * C), float("nan"), device=dev)
    gb = torch.full((C,), float("nan"), device=dev)
    if fam == "hip":
        nbytes = int(lib.mrp_compress_bwd_weight_workspace(n, C, P, max(G.ns, X.ns, A.ns)))
    elif fam == "split":
        nbytes = int(lib.mrp_compress_bwd_weight_split_workspace(n, C, P))
    elif fam == "half":
        nbytes = int(lib.mrp_compress_bwd_weight_t_workspace(n, C, P))
    else:
        nbytes = int(lib.mrp_compress_bwd_weight_cl_workspace(n, C, P))
    ws = torch.empty((nbytes + 3) // 4, device=dev, dtype=torch.float32) if nbytes > 0 else None
    tail = (n, C, P, _p(gw), _p(gb), _p(ws), nbytes, st)
    if fam == "hip":
        code = lib.mrp_compress_bwd_weight(G.ptr, G.ns, X.ptr, X.ns, A.ptr, A.ns, *tail)
    elif fam == "split":
        code = lib.mrp_compress_bwd_weight_split(G.ptr, G.ns, X.ptr, X.ns, A.ptr, A.ns, *tail)
    elif fam == "half":
        code = lib.mrp_compress_bwd_weight_t(sp.ENUM[key], G.ptr, G.ns, X.ptr, X.ns, A.ptr, A.ns, *tail)
    else:
        code = lib.mrp_compress_bwd_weight_cl(sp.ENUM[key], G.ptr, G.ns, G.ps, X.ptr, X.ns, X.ps, A.ptr, A.ns, A.ps,
                                              *tail)
    torch.cuda.synchronize(dev)
    return code, gw.cpu(), gb.cpu()


def _place_compress(arena, c, layout, key):
    """x, a, gy sparse in the arena and y, gx, ga reserved; pixel-major: pixel stride 2C, a beside x and ga
    beside gx (the halves of a channels_last concatenation buffer and of its gradient)."""
    n, C, H, W = c["x"].shape
    T = sp.DTYPES[key]
    kw = dict(layout=layout, ps=2 * C if layout == "cl" else None)
    X = arena.place(c["x"], **kw)
    A = arena.place(c["a"], beside=X if layout == "cl" else None, **kw)
    G = arena.place(c["gy"], **kw)
    Y = arena.reserve((n, C, H, W), T, **kw)
    GX = arena.reserve((n, C, H, W), T, **kw)
    GA = arena.reserve((n, C, H, W), T, beside=GX if layout == "cl" else None, **kw)
    return X, A, G, Y, GX, GA


def _run_compress(arena, fam, key, case, ops=("fwd", "dgrad", "wgrad"), knobs=None, dense_knobs=None):
    """The family's entry points on sparse operands under ``knobs``; the dense copy runs under
    ``dense_knobs`` (default: the same)."""
    knobs = knobs or {}
    dense_knobs = knobs if dense_knobs is None else dense_knobs
    dev = arena.dev
    st = _st(dev)
    layout, e_fwd, e_dgrad, e_wgrad = FAMILY[fam]
    c = _ccase(case, key, dev)
    n, C, H, W = c["x"].shape
    T = sp.DTYPES[key]
    X, A, G, Y, GX, GA = _place_compress(arena, c, layout, key)
    ins = [X, A, G]
    what = f"{fam} {key} {case} {knobs}"
    if "fwd" in ops:
        with sc.knobs(compress.compress_path(), **knobs) as lib:
            code = _call_fwd(fam, lib, key, c, X, A, Y, st)
        assert code == sp.expected(e_fwd, key, case), (what, e_fwd, code)
        (y,) = arena.check(ins, [Y], untouched=code != 0)
        if code == 0:
            _bar(fam, key, "y", y, c, what)
            dY = _dense_out((n, C, H, W), T, dev, layout)
            with sc.knobs(compress.compress_path(), **dense_knobs) as lib:
                assert _call_fwd(fam, lib, key, c, _dense_in(c["x"], dev, layout), _dense_in(c["a"], dev, layout),
                                 dY, st) == 0
            _same_bits(y, dY.read(), what + " y")
    if "dgrad" in ops:
        with sc.knobs(compress.compress_path(), **knobs) as lib:
            code = _call_dgrad(fam, lib, key, c, G, GX, GA, st)
        assert code == sp.expected(e_dgrad, key, case), (what, e_dgrad, code)
        gx, ga = arena.check(ins, [GX, GA], untouched=code != 0)
        if code == 0:
            _bar(fam, key, "gx", gx, c, what)
            _bar(fam, key, "ga", ga, c, what)
            dGX, dGA = (_dense_out((n, C, H, W), T, dev, layout) for _ in range(2))
            with sc.knobs(compress.compress_path(), **dense_knobs) as lib:
                assert _call_dgrad(fam, lib, key, c, _dense_in(c["gy"], dev, layout), dGX, dGA, st) == 0
            _same_bits(gx, dGX.read(), what + " gx")
            _same_bits(ga, dGA.read(), what + " ga")
    if "wgrad" in ops:
        with sc.knobs(compress.compress_path(), **knobs) as lib:
            code, gw, gb = _call_wgrad(fam, lib, key, c, G, X, A, st)
        assert code == sp.expected(e_wgrad, key, case), (what, e_wgrad, code)
        arena.check(ins, [])
        if code == 0:  # the split plan may change with the stride: the float64 bar only
            _bar(fam, key, "gw", gw, c, what)
            _bar(fam, key, "gb", gb, c, what)
        else:
            assert bool(torch.isnan(gw).all()) and bool(torch.isnan(gb).all())


def test_compress_fp32_mfma(arena):
    """``mrp_compress_fwd`` / ``_bwd_data`` / ``_bwd_weight``, 18 nodes, C = 32, P = 32: a column tile's four
    nodes are addressed from the tile's first node (``launch_nn_cfg``'s guard), the weight gradient's splits
    are capped at 5 nodes by ``plan_nt``'s branch for large node strides."""
    _run_compress(arena, "hip", "f32", "n18_c32_p32")


@pytest.mark.parametrize("gemm_split", [-1, 2, 7])
def test_compress_split_forward_and_data_gradient(arena, gemm_split):
    _run_compress(arena, "split", "f32", "n18_c64_p32", ops=("fwd", "dgrad"), knobs={"gemm_split": gemm_split})


@pytest.mark.parametrize("split_nt", [-1, 3, 4])
def test_compress_split_weight_gradient(arena, split_nt):
    _run_compress(arena, "split", "f32", "n18_c64_p32", ops=("wgrad",), knobs={"split_nt": split_nt})


@pytest.mark.parametrize("gemm_split", [-1, 2, 7])
def test_compress_split_forward_c256_takes_the_128_row_form(arena, gemm_split):
    """M = 256 admits the 256-row form, whose epilogue writes through 32-bit buffer offsets: ``mf16_ok``'s
    span test is the deciding condition and switches to the 128-row form (64-bit stores) — so under every
    ``gemm_split`` the bits are the dense run's under ``gemm_split`` 2."""
    _run_compress(arena, "split", "f32", "n18_c256_p32", ops=("fwd",), knobs={"gemm_split": gemm_split},
                  dense_knobs={"gemm_split": 2})


@pytest.mark.parametrize("case", ["n18_c32_p32", "n7_c32_p32", "n8_c32_p32"])
@pytest.mark.parametrize("key", HALF)
def test_compress_half(arena, key, case):
    """``mrp_compress_fwd_t`` / ``_bwd_data_t`` / ``_bwd_weight_t``: 18 nodes — the forward and the data gradient
    decline (their stores go through 31-bit buffer offsets) and write nothing, the weight gradient (64-bit
    loads) runs; 7 nodes (1.75 GiB) and 8 nodes (the most the output guard accepts at this stride) — all three
    run."""
    _run_compress(arena, "half", key, case)


@pytest.mark.parametrize("key", HALF)
def test_compress_half_channels_last(arena, key):
    """``mrp_compress_fwd_cl`` / ``_bwd_data_cl`` / ``_bwd_weight_cl``, 18 nodes, P = 49 (stages cross node
    boundaries), pixel stride 2C: only the row count and the packed image are guarded, the kernels form
    64-bit node addresses."""
    _run_compress(arena, "cl", key, "n18_c32_p49")


# ---- compress: the Python routes --------------------------------------------------------------------------
#: (dtype, case, layout, compress path, products): every case of ``span_cases.COMPRESS`` through the family that
#: takes it; C = 256 is the forward-only case of the table
PY_ROUTES = [("f32", "n18_c64_p32", "nchw", "split", "fdw"), ("f32", "n18_c256_p32", "nchw", "split", "f"),
             ("f32", "n18_c32_p32", "nchw", "hip", "fdw")]
PY_ROUTES += [(k, ca, "nchw", "split", "fdw") for k in HALF for ca in ("n18_c32_p32", "n7_c32_p32", "n8_c32_p32")]
PY_ROUTES += [(k, "n18_c32_p49", "cl", "split", "fdw") for k in HALF]
#: calls of mrp_compress_bwd_data_t that cover the sparse gx / ga of each 16-bit NCHW case: 8 nodes per call
#: at this stride (7 S + a block < 2^31 bytes <= 8 S), so 18 nodes take 3 and 8 nodes exactly 1
DGRAD_CALLS = {"n18_c32_p32": 3, "n7_c32_p32": 1, "n8_c32_p32": 1}


class _Counted:
    """Counts the calls of one entry point of the loaded library (restored on exit)."""

    def __init__(self, lib, name):
        self.lib, self.name, self.calls = lib, name, 0

    def __enter__(self):
        fn = getattr(self.lib, self.name)
        self.fn = fn

        def counted(*args):
            self.calls += 1
            return fn(*args)
        setattr(self.lib, self.name, counted)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.fn)


@pytest.mark.parametrize("key,case,layout,path,ops", PY_ROUTES, ids=lambda v: str(v))
def test_compress_python_routes(arena, key, case, layout, path, ops):
    """``compress.compress_forward`` on sparse x / a views, ``compress_backward_data`` into given sparse gx /
    ga views and ``compress_backward_weight``: correct values, no ``RuntimeError`` — where an entry point
    declines for span alone the module issues it over node ranges that fit (as many calls as
    ``DGRAD_CALLS`` says, one where the whole output fits), with the dense run's bits."""
    fam = {"nchw": "half" if key != "f32" else path, "cl": "cl"}[layout]
    dev = arena.dev
    c = _ccase(case, key, dev)
    n, C, H, W = c["x"].shape
    X, A, G, _Y, GX, GA = _place_compress(arena, c, layout, key)
    ins = [X, A, G]
    what = f"python {fam} {key} {case}"
    dx, da, dg = (_dense_in(c[k], dev, layout).t for k in ("x", "a", "gy"))
    with sc.knobs(path) as lib:
        with _Counted(lib, "mrp_compress_fwd_t") as fwd_calls:
            y = compress.compress_forward(c["wd"], c["bd"], X.view(), A.view())
        arena.check(ins, [])
        _bar(fam, key, "y", y.cpu(), c, what)
        _same_bits(y, compress.compress_forward(c["wd"], c["bd"], dx, da), what + " y")
        if fam == "half":
            assert fwd_calls.calls == 1, what  # y is dense: its node range fits
        if "d" in ops:
            with _Counted(lib, "mrp_compress_bwd_data_t") as dgrad_calls:
                compress.compress_backward_data(c["wd"], G.view(), gx=GX.view(), ga=GA.view())
            gx, ga = arena.check(ins, [GX, GA])
            if fam == "half":
                assert dgrad_calls.calls == DGRAD_CALLS[case], (what, dgrad_calls.calls)
            gxd, gad = compress.compress_backward_data(c["wd"], dg)
            for name, got, dense in (("gx", gx, gxd), ("ga", ga, gad)):
                _bar(fam, key, name, got, c, what)
                _same_bits(got, dense, f"{what} {name}")
        if "w" in ops:
            r = compress.compress_backward_weight(G.view(), X.view(), A.view())
            arena.check(ins, [])
            assert r is not None, what
            _bar(fam, key, "gw", r[0].reshape(C, 2 * C).cpu(), c, what)
            _bar(fam, key, "gb", r[1].cpu(), c, what)


@pytest.mark.parametrize("key", HALF)
def test_compress_python_node_ranges(arena, key, monkeypatch):
    """The node-range loops of ``compress_forward`` and ``compress_backward_data`` themselves: with the
    nodes per call forced to 5, 18 nodes take 4 calls of each entry point (5, 5, 5, 3 nodes, every
    pointer advanced by its own node stride) and give the bits of the single call — dense operands, so that
    the single call is legal."""
    dev = arena.dev
    c = _ccase("n18_c32_p32", key, dev)
    x, a, gy = (c[k].to(dev) for k in ("x", "a", "gy"))
    lib = m.load_library()
    y1 = compress.compress_forward(c["wd"], c["bd"], x, a)
    gx1, ga1 = compress.compress_backward_data(c["wd"], gy)
    monkeypatch.setattr(compress, "_span_nodes", lambda n, C, P, *strides: 5)
    with _Counted(lib, "mrp_compress_fwd_t") as f, _Counted(lib, "mrp_compress_bwd_data_t") as d:
        y4 = compress.compress_forward(c["wd"], c["bd"], x, a)
        gx4, ga4 = compress.compress_backward_data(c["wd"], gy)
    assert (f.calls, d.calls) == (4, 4)
    for name, one, four in (("y", y1, y4), ("gx", gx1, gx4), ("ga", ga1, ga4)):
        _same_bits(four, one, f"{key} {name} in 4 node ranges")
        _bar("half", key, name, four.cpu(), c, f"node ranges {key}")


# ---- aggregation ----------------------------------------------------------------------------------------
MODES = {"film_mean": _lib.MODE_FILM_MEAN, "film_sum": _lib.MODE_FILM_SUM, "copy_mean": _lib.MODE_COPY_MEAN}
#: (case, mode): all three modes on the first graph set
AGG_RUNS = [("complete_3x8", mo) for mo in MODES] + \
    [(ca, "film_mean") for ca in sp.AGG_S[1:] + ("complete_1x16_s512",)]
AGG_CL_RUNS = [(ca, "film_mean") for ca in sp.AGG_CL_SPAN]
#: cases whose backward is given a grad_x base (the first half of a concatenation's gradient)
WITH_BASE = ("complete_3x8", "ragged_8_5_1_8")
#: 9..16-node graphs with whole 64-pixel planes: the matrix-core backward
MFMA_CASES = ("complete_2x12", "knn4_2x12")
#: the 16-node graph whose own nodes lie more than 2^32 bytes apart: the matrix-core backward must step aside
SELF_SPAN = "complete_1x16_s512"


@functools.lru_cache(maxsize=None)
def _agraph(case):
    sizes, knn = sp.AGG[case][:2]
    rng = np.random.RandomState(sum(map(ord, case)))
    if case.startswith("ragged"):  # the 5-node graph: node 4 has no in-edge, 0->1 a multi-edge, 3->3 a self-loop
        mid = m.RobotGraph([0, 0, 2, 3, 1, 0, 2], [1, 1, 1, 3, 0, 2, 3], num_nodes=5)
        gs = [m.frame_graph(hc._poses(rng, 8)), mid, m.frame_graph(hc._poses(rng, 1)), m.frame_graph(hc._poses(rng, 8))]
    else:
        gs = [m.frame_graph(hc._poses(rng, k), knn=knn) for k in sizes]
    g = m.batch(gs)
    assert g.num_nodes() == sum(sizes)
    assert (sum(sizes) - 1) * sp.agg_stride(case, 2) >= 1 << 32  # the last node lies beyond 2^32 bytes
    return g


@functools.lru_cache(maxsize=None)
def _acase(case, key):
    """(x, G, base in T; gb fp32) on the CPU."""
    _, _, C, H, W, _ = sp.AGG[case]
    T = sp.DTYPES[key]
    g = _agraph(case)
    gen = torch.Generator().manual_seed(sum(map(ord, case)) * 131 + ALL.index(key))
    x, G, base = (torch.randn(g.num_nodes(), C, H, W, generator=gen).to(T) for _ in range(3))
    gb = torch.sigmoid(torch.randn(g.num_edges(), C, 2, generator=gen))
    return x, G, base, gb


@functools.lru_cache(maxsize=None)
def _aref(case, key, mode):
    x, G, base, gb = _acase(case, key)
    src, dst = (t.numpy() for t in _agraph(case).edges())
    ref = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        xx, gg, GG = x.to(dt), gb.to(dt), G.to(dt)
        ref["out" + tag] = oracle.film_aggregate(xx, gg, src, dst, mode)
        ref["dx" + tag], ref["dgb" + tag] = oracle.film_aggregate_grads(xx, gg, src, dst, GG, mode)
    return ref


def _agg_bar(got, ref64, key, what):
    T = sp.DTYPES[key]
    assert got.dtype == T
    if key == "f32":
        e = rel_err(got.numpy(), ref64.numpy())
        assert e <= TOL, (what, e)
    else:
        hc.assert_elementwise(got, ref64, T, what)


def _dgb_bar(got, ref, key, mode, what):
    if mode == "copy_mean":
        assert not bool(got.any()), what  # zero-filled
    elif key == "f32":
        e = rel_err(got.numpy(), ref["dgb64"].numpy())
        assert e <= TOL, (what, e)
    else:
        hc.assert_relative(got, ref["dgb32"], ref["dgb64"], what)


def _graph(case, dev, gbd, C, P, mode):
    csr = _agraph(case).csr(dev)
    knn = sp.AGG[case][1]
    want = _lib.graph_regular(knn) if knn else _lib.GRAPH_CSR if case.startswith("ragged") else _lib.GRAPH_COMPLETE
    assert csr.graph_kind == want
    return csr, aggregate._graph_args(gbd if MODES[mode] != _lib.MODE_COPY_MEAN else None, csr, C, P, MODES[mode])


def _agg_fwd(lib, key, layout, X, graph, OUT, XC, st):
    if layout == "nchw":
        ep = _lib.Epilogue(1.0, 0.0, None, 0, 0.0, XC.address, XC.ns) if XC is not None else None
        return lib.mrp_film_mean_fwd_t(sp.ENUM[key], X.ptr, X.ns, *graph, OUT.ptr, OUT.ns,
                                       ctypes.byref(ep) if ep is not None else None, st)
    ep = _lib.EpilogueCl(1.0, 0.0, None, 0, 0.0, XC.address, XC.ns, 0, XC.ps) if XC is not None else None
    return lib.mrp_film_mean_fwd_cl(sp.ENUM[key], X.ptr, X.ns, X.ps, *graph, OUT.ptr, OUT.ns, OUT.ps,
                                    ctypes.byref(ep) if ep is not None else None, st)


def _agg_bwd(lib, key, layout, case, mode, G, X, graph, DX, B, dgb, st):
    bp, bn, bps = (B.ptr, B.ns, B.ps) if B is not None else (None, 0, 0)
    if layout == "nchw":
        return lib.mrp_film_mean_bwd_t(sp.ENUM[key], G.ptr, G.ns, X.ptr, X.ns, *graph, DX.ptr, DX.ns, bp, bn, _p(dgb),
                                       None, st)
    sizes, _, C, H, W, _ = sp.AGG[case]
    csr = _agraph(case).csr(dgb.device)
    nbytes = int(lib.mrp_film_mean_bwd_cl_workspace(csr.num_graphs, csr.max_nodes, csr.graph_kind, C, H * W,
                                                    MODES[mode], 1))
    ws = torch.empty((nbytes + 3) // 4, device=dgb.device, dtype=torch.float32) if nbytes > 0 else None
    return lib.mrp_film_mean_bwd_cl(sp.ENUM[key], G.ptr, G.ns, G.ps, X.ptr, X.ns, X.ps, *graph, DX.ptr, DX.ns, DX.ps,
                                    bp, bn, bps or 0, _p(dgb), None, _p(ws), nbytes, st)


def _run_aggregation(arena, key, case, mode, layout):
    """Forward (with the cat epilogue's ``xcopy`` in the arena on the first graph set) and backward of one
    case, sparse against float64 and against the dense run."""
    dev = arena.dev
    lib, st = m.load_library(), _st(dev)
    sizes, _, C, H, W, extra = sp.AGG[case]
    T = sp.DTYPES[key]
    x, Gc, base, gb = _acase(case, key)
    n, P = x.shape[0], H * W
    ref = _aref(case, key, mode)
    gbd = gb.to(dev)
    csr, graph = _graph(case, dev, gbd, C, P, mode)
    kw = dict(layout=layout, ps=2 * C if layout == "cl" else None, stride_bytes=sp.agg_stride(case, x.element_size()))
    fwd, bwd = ("mrp_film_mean_fwd_t", "mrp_film_mean_bwd_t") if layout == "nchw" else \
        ("mrp_film_mean_fwd_cl", "mrp_film_mean_bwd_cl")
    what = f"{layout} {key} {case} {mode}"
    shape = (n, C, H, W)

    # forward; on the first graph set as torch.cat((x, a), 1): xcopy the first half, out the second
    cat = case == "complete_3x8"
    X = arena.place(x, **kw)
    XC = arena.reserve(shape, T, **kw) if cat else None
    OUT = arena.reserve(shape, T, beside=XC if cat and layout == "cl" else None, **kw)
    code = _agg_fwd(lib, key, layout, X, graph, OUT, XC, st)
    assert code == sp.expected(fwd, key, case), (what, code)
    got = arena.check([X], [OUT] + ([XC] if cat else []))
    _agg_bar(got[0], ref["out64"], key, what + " out")
    dOUT = _dense_out(shape, T, dev, layout)
    dXC = _dense_out(shape, T, dev, layout) if cat else None
    assert _agg_fwd(lib, key, layout, _dense_in(x, dev, layout), graph, dOUT, dXC, st) == 0
    _same_bits(got[0], dOUT.read(), what + " out")
    if cat:
        _same_bits(got[1], x, what + " xcopy")

    # backward
    G = arena.place(Gc, **kw)
    with_base = case in WITH_BASE
    B = arena.place(base, beside=None, **kw) if with_base else None
    DX = arena.reserve(shape, T, **kw)
    dgb = torch.full((csr.num_edges, C, 2), float("nan"), device=dev)
    code = _agg_bwd(lib, key, layout, case, mode, G, X, graph, DX, B, dgb, st)
    assert code == sp.expected(bwd, key, case), (what, code)
    (dx,) = arena.check([X, G] + ([B] if with_base else []), [DX])
    want = ref["dx64"] + (base.double() if with_base else 0)
    _agg_bar(dx, want, key, what + " grad_x")
    _dgb_bar(dgb.cpu(), ref, key, mode, what + " grad_gb")
    dDX = _dense_out(shape, T, dev, layout)
    dgb2 = torch.empty_like(dgb)
    assert _agg_bwd(lib, key, layout, case, mode, _dense_in(Gc, dev, layout), _dense_in(x, dev, layout), graph, dDX,
                    _dense_in(base, dev, layout) if with_base else None, dgb2, st) == 0
    self_span = layout == "nchw" and case == SELF_SPAN
    if not self_span:  # (there the dense run is another kernel's, whose grad_x is a matrix-core product: below)
        _same_bits(dx, dDX.read(), what + " grad_x")
    if layout == "nchw" and case in MFMA_CASES:
        # The matrix-core backward's launcher checks 15 node strides + two planes against 2^32 and, if they do
        # not fit, quietly runs film_bwd_dx + the Gram pass instead.  15 S fits, so the matrix-core kernel must
        # be the one that ran here: grad_gb has the bits of the dense run, and not those of the dense run with
        # the matrix-core kernels switched off (which sums over the plane in another order).
        _same_bits(dgb, dgb2, what + " grad_gb")
        dgb3 = torch.empty_like(dgb)
        with sc.knobs(compress.compress_path(), bwd_complete_mfma=0, bwd_regular_mfma=0):
            assert _agg_bwd(lib, key, layout, case, mode, _dense_in(Gc, dev, layout), _dense_in(x, dev, layout), graph,
                            _dense_out(shape, T, dev, layout), None, dgb3, st) == 0
        _dgb_bar(dgb3.cpu(), ref, key, mode, what + " grad_gb, VALU kernels")
        assert not torch.equal(dgb3, dgb2), what + ": the knobs did not change the kernel"
    if self_span:
        # The mirror image: 15 node strides of 2^29 bytes + 64 KiB do not fit the matrix-core backward's 32-bit
        # lane offsets, so the launcher must have kept film_bwd_dx + the Gram pass: grad_x and grad_gb have the
        # bits of the dense run with the matrix-core kernels switched off, and grad_gb not those of the dense
        # default-knob run (whose strides fit, and which therefore ran the matrix-core kernel).
        dgb3 = torch.empty_like(dgb)
        dDX3 = _dense_out(shape, T, dev, layout)
        with sc.knobs(compress.compress_path(), bwd_complete_mfma=0, bwd_regular_mfma=0):
            assert _agg_bwd(lib, key, layout, case, mode, _dense_in(Gc, dev, layout), _dense_in(x, dev, layout), graph,
                            dDX3, None, dgb3, st) == 0
        _same_bits(dx, dDX3.read(), what + " grad_x, VALU kernels")
        _agg_bar(dDX.read(), want, key, what + " grad_x, dense matrix-core run")
        _same_bits(dgb, dgb3, what + " grad_gb, VALU kernels")
        _dgb_bar(dgb2.cpu(), ref, key, mode, what + " grad_gb, dense matrix-core run")
        assert not torch.equal(dgb, dgb2), what + ": the matrix-core kernel ran on strides its lane offsets cannot hold"


@pytest.mark.parametrize("case,mode", AGG_RUNS, ids=lambda v: str(v))
@pytest.mark.parametrize("key", ALL)
def test_aggregation_node_major(arena, key, case, mode):
    """``mrp_film_mean_fwd_t`` / ``_bwd_t``: 64-bit per-graph bases, 32-bit per-lane byte offsets.  3 x 8 nodes:
    the fused backward, 16-byte slices, the cat epilogue; 2 x 12: the matrix-core backward (its lane offsets
    hold up to 15 node strides); k-NN(4); ragged CSR with a node without in-edges and a grad_x base; P = 15
    with an odd node stride: one element per access; one 16-node graph 2^29 bytes + 64 KiB a node: a graph that
    spans 2^32 bytes by itself, where the matrix-core backward must leave the call to the VALU kernels."""
    _run_aggregation(arena, key, case, mode, "nchw")


@pytest.mark.parametrize("case,mode", AGG_CL_RUNS, ids=lambda v: str(v))
@pytest.mark.parametrize("key", ALL)
def test_aggregation_pixel_major(arena, key, case, mode):
    """``mrp_film_mean_fwd_cl`` / ``_bwd_cl`` (workspace from the query), pixel stride 2C: the halves of a
    channels_last concatenation buffer."""
    _run_aggregation(arena, key, case, mode, "cl")


#: (layout, case, mode): every C-ABI case of either layout, and all three modes on the first graph set of both
AGG_PY_RUNS = [("nchw", ca, mo) for ca, mo in AGG_RUNS] + \
    [("cl", "complete_3x8", mo) for mo in MODES] + [("cl", ca, "film_mean") for ca in sp.AGG_CL_SPAN[1:]]


@pytest.mark.parametrize("layout,case,mode", AGG_PY_RUNS, ids=lambda v: str(v))
@pytest.mark.parametrize("key", ALL)
def test_aggregation_python_routes(arena, key, layout, case, mode):
    """``aggregate.film_mean_forward_into`` on a sparse x into a sparse out with the cat epilogue's sparse xcopy,
    and ``aggregate.film_mean_backward`` on sparse grad_out / x / base views, for every case and mode of the
    C-ABI tests (the odd node stride included: ``node_stride`` takes it as it is): values under the same
    bars, the dense run's bits."""
    dev = arena.dev
    sizes, _, C, H, W, extra = sp.AGG[case]
    T = sp.DTYPES[key]
    x, Gc, base, gb = _acase(case, key)
    ref = _aref(case, key, mode)
    gbd = gb.to(dev) if mode != "copy_mean" else None
    csr = _agraph(case).csr(dev)
    kw = dict(layout=layout, ps=2 * C if layout == "cl" else None,
              stride_bytes=sp.agg_stride(case, x.element_size()))
    what = f"python {layout} {key} {case} {mode}"
    X = arena.place(x, **kw)
    XC = arena.reserve(x.shape, T, **kw)
    OUT = arena.reserve(x.shape, T, beside=XC if layout == "cl" else None, **kw)
    before = dict(aggregate.PATH_COUNTS)
    aggregate.film_mean_forward_into(X.view(), gbd, csr, MODES[mode], OUT.view(),
                                     epilogue=aggregate.EpilogueSpec(xcopy=XC.view()))
    out, xc = arena.check([X], [OUT, XC])
    _agg_bar(out, ref["out64"], key, what + " out")
    _same_bits(xc, x, what + " xcopy")
    G = arena.place(Gc, **kw)
    B = arena.place(base, **kw)
    dx, dgb = aggregate.film_mean_backward(G.view(), X.view(), gbd, csr, MODES[mode], True, True, grad_x_base=B.view())
    arena.check([X, G, B], [])
    # the sparse views ran in place, on the kernels of their own layout: no conversion route
    tag = ("_cl_" if layout == "cl" else "_") + key
    moved = {k: v - before.get(k, 0) for k, v in aggregate.PATH_COUNTS.items() if v != before.get(k, 0)}
    assert moved == {"fwd" + tag: 1, "bwd" + tag: 1}, (what, moved)
    _agg_bar(dx.cpu().contiguous(), ref["dx64"] + base.double(), key, what + " grad_x")
    _dgb_bar(dgb.cpu(), ref, key, mode, what + " grad_gb")
    dX, dG, dB = (_dense_in(t, dev, layout).t for t in (x, Gc, base))
    dOUT = _dense_out(x.shape, T, dev, layout).t
    aggregate.film_mean_forward_into(dX, gbd, csr, MODES[mode], dOUT)
    _same_bits(out, dOUT, what + " out")
    # the self-spanning graph: the sparse views do not fit the matrix-core backward's lane offsets, so they ran
    # film_bwd_dx + the Gram pass — the dense operands' kernels only with the matrix-core ones switched off
    valu = dict(bwd_complete_mfma=0, bwd_regular_mfma=0) if (layout, case) == ("nchw", SELF_SPAN) else {}
    with sc.knobs(compress.compress_path(), **valu):
        dxd, dgbd = aggregate.film_mean_backward(dG, dX, gbd, csr, MODES[mode], True, True, grad_x_base=dB)
    _same_bits(dx, dxd, what + " grad_x")
    if valu:
        _same_bits(dgb, dgbd, what + " grad_gb")


# ---- the max-pooled, attention-pooled, confidence-weighted and confidence-gated aggregations -----------------
FAMILIES = ("max", "attn", "wmean", "wattn")
FAM_TOL = {"max": t_max.TOL, "attn": t_attn.TOL, "wmean": t_wmean.TOL, "wattn": t_wattn.TOL}
#: the outputs of each family: out, grad_x (features, node-strided), grad_w (fp32, node-strided), the rest dense fp32
FAM_OUTS = {"max": ("out", "dx", "dgb"), "attn": ("out", "attn", "dx", "dgb"), "wmean": ("out", "dx", "dgb", "dw"),
            "wattn": ("out", "attn", "rate", "dx", "dgb", "dw")}
WIDE = "wide_3x8_c17_p80"
#: (family, case, film_wmean's mode): every graph set; film_wmean in both modes on the first
FAM_RUNS = [(fam, ca, "mean") for fam in FAMILIES for ca in sp.AGG_FAMILIES] + [("wmean", "complete_3x8", "sum")]
FAM_PY_RUNS = [(fam, ca) for fam in FAMILIES for ca in ("complete_3x8", "ragged_8_5_1_8", WIDE)]


def _fam_base(case):
    return case in WITH_BASE or case == WIDE


@functools.lru_cache(maxsize=None)
def _fops(fam, case, key):
    """CPU operands of a family on a graph set: x, G, base in T (drawn in fp32, rounded once), gb fp32 gamma / beta,
    w fp32 sender maps (None for the families without them).  film_max: ``max_cases.lattice_operands``, whose values
    every dtype holds exactly; film_wattn: without loud senders; film_wmean: ``wmean_cases``' weights."""
    _, _, C, H, W, _ = sp.AGG[case]
    g = _agraph(case)
    n, E = g.num_nodes(), g.num_edges()
    seed = sum(map(ord, case + fam)) * 131
    w = None
    if fam == "max":
        x, gb, G, base = mc.lattice_operands(g, C, H, W, seed)
    elif fam == "attn":
        x, gb, _, G, base = ac.random_operands(g, C, H, W, seed)
    elif fam == "wattn":
        x, gb, _, G, base, w, louds = wac.random_operands(g, C, H, W, seed, loud=False)
        assert louds == ()
    else:
        gen = torch.Generator().manual_seed(seed)
        x, G, base = (torch.randn(n, C, H, W, generator=gen) for _ in range(3))
        gb = torch.sigmoid(torch.randn(E, C, 2, generator=gen))
        w = wmc.weights_of(n, H, W, gen)
    T = sp.DTYPES[key]
    return dict(x=x.to(T), G=G.to(T), base=base.to(T), gb=gb, w=w)


@functools.lru_cache(maxsize=None)
def _fref(fam, case, key, mode):
    """The family's own reference on the widened operands: name -> float64 tensor (film_max: fp32, exact on the
    lattice; film_wmean: also name + "32", the fp32 restatement ``stack_ref.within`` measures against)."""
    o = _fops(fam, case, key)
    g = _agraph(case)
    x, G = o["x"].float(), o["G"].float()
    base = o["base"].float() if _fam_base(case) else None
    if fam == "max":
        return dict(zip(FAM_OUTS[fam], mc.reference(g, x, o["gb"], G, base=base)))
    if fam == "attn":
        return dict(zip(FAM_OUTS[fam], ac.reference(g, x, o["gb"], G, base=base, dtype=torch.float64)))
    if fam == "wattn":
        return dict(zip(FAM_OUTS[fam], wac.reference(g, x, o["gb"], o["w"], G, base=base, dtype=torch.float64)))
    ref = {}
    for tag, dt in (("", torch.float64), ("32", torch.float32)):
        out, dx, dgb, dw = wmc.backward(g, x.to(dt), o["gb"].to(dt), o["w"].to(dt), G.to(dt), mode=mode)
        ref.update({"out" + tag: out, "dx" + tag: dx + (base.to(dt) if base is not None else 0), "dgb" + tag: dgb,
                    "dw" + tag: dw})
    return ref


def _fam_fwd(lib, fam, key, case, mode, csr, gbd, X, Wt, OUT, st):
    """The family's forward entry point on operands with ``ptr`` / ``ns``: (code, attn, rate); attn and rate are
    dense (E, P) fp32 tensors (the ABI gives them no stride), NaN-filled before the call."""
    _, _, C, H, W, _ = sp.AGG[case]
    P, dev, dt = H * W, gbd.device, sp.ENUM[key]
    ga = aggregate._graph_args(gbd, csr, C, P, 0)
    attn = rate = None
    if fam in ("attn", "wattn"):
        attn = torch.full((csr.num_edges, P), float("nan"), device=dev)
        scale = ac.default_scale(C)
    if fam == "max":
        code = lib.mrp_film_max_fwd(dt, X.ptr, X.ns, *ga, OUT.ptr, OUT.ns, st)
    elif fam == "attn":
        assert lib.mrp_film_attn_workspace(0, *ga[5:12]) == 0
        code = lib.mrp_film_attn_fwd(dt, X.ptr, X.ns, *ga, OUT.ptr, OUT.ns, scale, _p(attn), None, 0, st)
    elif fam == "wmean":
        code = lib.mrp_film_wmean_fwd(dt, X.ptr, X.ns, ga[0], Wt.ptr, Wt.ns, *ga[1:], aggregate.WAGG_MODES[mode],
                                      OUT.ptr, OUT.ns, st)
    else:
        assert lib.mrp_film_wattn_workspace(0, *ga[5:12]) == 0
        rate = torch.full((csr.num_edges, P), float("nan"), device=dev)
        code = lib.mrp_film_wattn_fwd(dt, X.ptr, X.ns, ga[0], Wt.ptr, Wt.ns, *ga[1:], OUT.ptr, OUT.ns, scale, _p(attn),
                                      _p(rate), None, 0, st)
    torch.cuda.synchronize(dev)
    return code, attn, rate


def _fam_bwd(lib, fam, key, case, mode, csr, gbd, G, X, Wt, DX, B, DW, attn, rate, st):
    """The family's backward entry point with the workspace its query asks for: (code, grad_gb).  On the wide
    case the attention families' per-tile grad_gb partials (P = 80: two tiles) and film_wmean's per-block grad_w
    partials (C = 17: two blocks) go through that workspace."""
    _, _, C, H, W, _ = sp.AGG[case]
    P, dev, dt = H * W, gbd.device, sp.ENUM[key]
    ga = aggregate._graph_args(gbd, csr, C, P, 0)
    dgb = torch.full((csr.num_edges, C, 2), float("nan"), device=dev)
    head = (dt, G.ptr, G.ns, X.ptr, X.ns)
    tail = (DX.ptr, DX.ns) + ((B.ptr, B.ns) if B is not None else (None, 0)) + (_p(dgb),)
    if fam == "max":
        code = lib.mrp_film_max_bwd(*head, *ga, *tail, st)
    else:
        query = {"attn": lambda: lib.mrp_film_attn_workspace(1, *ga[5:12]),
                 "wattn": lambda: lib.mrp_film_wattn_workspace(1, *ga[5:12]),
                 "wmean": lambda: lib.mrp_film_wmean_workspace(*ga[5:12])}[fam]
        nbytes = int(query())
        assert nbytes >= 0 and (nbytes > 0 or case != WIDE), (fam, case, nbytes)
        ws = torch.full(((nbytes + 3) // 4,), float("nan"), device=dev) if nbytes > 0 else None
        if fam == "attn":
            code = lib.mrp_film_attn_bwd(*head, *ga, *tail, ac.default_scale(C), _p(attn), _p(ws), nbytes, st)
        elif fam == "wmean":
            code = lib.mrp_film_wmean_bwd(*head, ga[0], Wt.ptr, Wt.ns, *ga[1:], aggregate.WAGG_MODES[mode], *tail,
                                          DW.ptr, DW.ns, _p(ws), nbytes, st)
        else:
            code = lib.mrp_film_wattn_bwd(*head, ga[0], Wt.ptr, Wt.ns, *ga[1:], *tail, ac.default_scale(C), _p(attn),
                                          _p(rate), DW.ptr, DW.ns, _p(ws), nbytes, st)
    torch.cuda.synchronize(dev)
    return code, dgb


def _fam_dense_of(lib, st, fam, key, case, mode, dev, o, T):
    """Forward and backward of the family's entry points in ``key`` (elements of T) on dense copies of the operands
    ``o``, widened exactly where T is wider than they are: name -> CPU tensor."""
    x, Gc, base = (o[k].to(T) for k in ("x", "G", "base"))
    n, C, H, W = x.shape
    csr, gbd = _agraph(case).csr(dev), o["gb"].to(dev)
    X, G = _dense_in(x, dev, "nchw"), _dense_in(Gc, dev, "nchw")
    B = _dense_in(base, dev, "nchw") if _fam_base(case) else None
    Wt = _dense_in(o["w"].view(n, 1, H, W), dev, "nchw") if o["w"] is not None else None
    OUT, DX = (_dense_out((n, C, H, W), T, dev, "nchw") for _ in range(2))
    DW = _dense_out((n, 1, H, W), torch.float32, dev, "nchw") if Wt is not None else None
    code, attn, rate = _fam_fwd(lib, fam, key, case, mode, csr, gbd, X, Wt, OUT, st)
    assert code == 0, (fam, key, case, code)
    code, dgb = _fam_bwd(lib, fam, key, case, mode, csr, gbd, G, X, Wt, DX, B, DW, attn, rate, st)
    assert code == 0, (fam, key, case, code)
    res = dict(out=OUT.read(), dx=DX.read(), dgb=dgb.cpu())
    for name, t in (("attn", attn), ("rate", rate)):
        if t is not None:
            res[name] = t.cpu()
    if DW is not None:
        res["dw"] = DW.read()
    return res


@functools.lru_cache(maxsize=None)
def _fam_bars(fam, key, case, mode, dev):
    """The dense run of the entry points in ``key``, held to the family's own bar against its own reference; the
    sparse runs are then compared with it bit for bit.  Computed once per (family, dtype, case, mode).

    The fp32 kernels (on the operands widened exactly): film_max bit for bit with ``max_cases.reference`` (lattice
    operands: every message and sum is exact, no near-tie can be routed differently); film_attn and film_wattn every
    output within ``TOL`` of the float64 reference (``test_against_float64``); film_wmean out and grad_x within
    ``TOL``, grad_gb and grad_w under ``stack_ref.within`` (``test_g3_random_maps_against_float64``).  16-bit features
    as each family's own 16-bit contract test holds them: the fp32 kernels' outputs on the widened input, out and
    grad_x cast once, the fp32 outputs bit for bit; film_wmean (whose header promises that of the forward alone):
    the forward so, and out, grad_x, grad_gb, grad_w under the bars of ``test_g3``."""
    lib, st = m.load_library(), _st(dev)
    o = _fops(fam, case, key)
    ref = _fref(fam, case, key, mode)
    what = f"dense {fam} {key} {case} {mode}"
    r32 = _fam_dense_of(lib, st, fam, "f32", case, mode, dev, o, torch.float32)
    for name in FAM_OUTS[fam]:
        got = r32[name].reshape(ref[name].shape)
        if fam == "max":
            _same_bits(got, ref[name], f"{what} {name} against the reference")
        elif fam == "wmean" and name in ("dgb", "dw"):
            ok, errs = stack_ref.within(got, ref[name + "32"], ref[name])
            print(what, name, "err, fp32 torch err", errs)
            assert ok, (what, name, errs)
        else:
            e = rel_err(got.numpy(), ref[name].numpy())
            print(what, name, "rel_err", e)
            assert e <= FAM_TOL[fam], (what, name, e)
    if key == "f32":
        return r32
    T = sp.DTYPES[key]
    rT = _fam_dense_of(lib, st, fam, key, case, mode, dev, o, T)
    for name in FAM_OUTS[fam]:
        assert rT[name].dtype == (T if name in ("out", "dx") else torch.float32), (what, name)
        if fam != "wmean" or name == "out":
            _same_bits(rT[name], r32[name].to(rT[name].dtype), f"{what} {name} against the fp32 kernels', cast once")
        if fam == "wmean" and name in ("out", "dx"):
            hc.assert_elementwise(rT[name], ref[name], T, f"{what} {name}")
        elif fam == "wmean":
            ok, errs = stack_ref.within(rT[name].reshape(ref[name].shape), ref[name + "32"], ref[name])
            assert ok, (what, name, errs)
    return rT


def _fam_place(arena, fam, key, case):
    """x, grad_out, grad_x_base and w sparse in the arena, each in a slot of its own (the outputs are reserved by
    the caller).  w (n, 1, H, W) fp32 at the case's stride in its own element size."""
    o = _fops(fam, case, key)
    n, C, H, W = o["x"].shape
    kw = dict(stride_bytes=sp.agg_stride(case, o["x"].element_size()))
    kw32 = dict(stride_bytes=sp.agg_stride(case, 4))
    X = arena.place(o["x"], **kw)
    G = arena.place(o["G"], **kw)
    B = arena.place(o["base"], **kw) if _fam_base(case) else None
    Wt = arena.place(o["w"].view(n, 1, H, W), **kw32) if o["w"] is not None else None
    return X, G, B, Wt, kw, kw32


@pytest.mark.parametrize("fam,case,mode", FAM_RUNS, ids=lambda v: str(v))
@pytest.mark.parametrize("key", ALL)
def test_family_node_major(arena, key, fam, case, mode):
    """``mrp_film_{max,attn,wmean,wattn}_{fwd,bwd}`` with x, out, grad_out, grad_x, grad_x_base, w and grad_w sparse
    in the arena (gb, attn, rate, grad_gb and the workspaces dense: the ABI gives them no stride): the return code
    of the table, ``Arena.check``, and every output — grad_gb, attn, rate and grad_w included — with the bits of
    the dense run, which ``_fam_bars`` holds to the family's own reference.

    Why the bits cannot depend on the strides.  Every kernel is deterministic (no atomics, one writer per element).
    film_max, film_wmean: a lane computes its own elements, the sources of a row in row order; grad_gb is summed
    per lane over its slices, then by a fixed butterfly over the plane's lanes, and film_wmean's grad_w over
    channels in blocks of 16 — orders fixed by C, P, the graph and the slice width, and the slice width is the same
    in both runs (every stride here is a multiple of 16 bytes but the P = 15 case's, where both runs take single
    elements).  film_attn, film_wattn: every access is one element and the order of every sum is a function of C, P
    and the graph alone (the header says so)."""
    dev = arena.dev
    lib, st = m.load_library(), _st(dev)
    dense = _fam_bars(fam, key, case, mode, dev)
    o = _fops(fam, case, key)
    n, C, H, W = o["x"].shape
    T = sp.DTYPES[key]
    csr, gbd = _agraph(case).csr(dev), o["gb"].to(dev)
    e_fwd, e_bwd = sp.FAMILY_ENTRIES[fam]
    what = f"{fam} {key} {case} {mode}"
    X, G, B, Wt, kw, kw32 = _fam_place(arena, fam, key, case)
    ins = [p for p in (X, G, B, Wt) if p is not None]
    OUT = arena.reserve((n, C, H, W), T, **kw)
    code, attn, rate = _fam_fwd(lib, fam, key, case, mode, csr, gbd, X, Wt, OUT, st)
    assert code == sp.expected(e_fwd, key, case), (what, code)
    (out,) = arena.check(ins, [OUT])
    _same_bits(out, dense["out"], what + " out")
    for name, t in (("attn", attn), ("rate", rate)):
        if t is not None:
            _same_bits(t, dense[name], f"{what} {name}")
    DX = arena.reserve((n, C, H, W), T, **kw)
    DW = arena.reserve((n, 1, H, W), torch.float32, **kw32) if Wt is not None else None
    code, dgb = _fam_bwd(lib, fam, key, case, mode, csr, gbd, G, X, Wt, DX, B, DW, attn, rate, st)
    assert code == sp.expected(e_bwd, key, case), (what, code)
    got = arena.check(ins, [DX] + ([DW] if DW is not None else []))
    _same_bits(got[0], dense["dx"], what + " grad_x")
    _same_bits(dgb, dense["dgb"], what + " grad_gb")
    if DW is not None:
        _same_bits(got[1], dense["dw"], what + " grad_w")


@pytest.mark.parametrize("fam,case", FAM_PY_RUNS, ids=lambda v: str(v))
@pytest.mark.parametrize("key", ALL)
def test_family_python_routes(arena, key, fam, case):
    """``aggregate.film_*_forward_into`` on sparse x and w views into a sparse out, and ``film_*_backward`` on sparse
    grad_out / x / grad_x_base / w views (its outputs are its own dense tensors): the dense run's bits, one forward
    and one backward of the family's own dtype key, and nothing else moved."""
    dev = arena.dev
    dense = _fam_bars(fam, key, case, "mean", dev)
    o = _fops(fam, case, key)
    n, C, H, W = o["x"].shape
    T = sp.DTYPES[key]
    csr, gbd = _agraph(case).csr(dev), o["gb"].to(dev)
    what = f"python {fam} {key} {case}"
    X, G, B, Wt, kw, _ = _fam_place(arena, fam, key, case)
    ins = [p for p in (X, G, B, Wt) if p is not None]
    OUT = arena.reserve((n, C, H, W), T, **kw)
    before = dict(aggregate.PATH_COUNTS)
    attn = rate = None
    if fam == "max":
        aggregate.film_max_forward_into(X.view(), gbd, csr, 0, OUT.view())
    elif fam == "attn":
        attn = aggregate.film_attn_forward_into(X.view(), gbd, csr, 0, OUT.view())
    elif fam == "wmean":
        aggregate.film_wmean_forward_into(X.view(), gbd, Wt.view(), csr, 0, OUT.view())
    else:
        attn, rate = aggregate.film_wattn_forward_into(X.view(), gbd, Wt.view(), csr, 0, OUT.view(), rate=True)
    (out,) = arena.check(ins, [OUT])
    dw = None
    if fam == "max":
        dx, dgb = aggregate.film_max_backward(G.view(), X.view(), gbd, csr, 0, True, True, grad_x_base=B.view())
    elif fam == "attn":
        dx, dgb = aggregate.film_attn_backward(G.view(), X.view(), gbd, attn, csr, 0, True, True, grad_x_base=B.view())
    elif fam == "wmean":
        dx, dgb, dw = aggregate.film_wmean_backward(G.view(), X.view(), gbd, Wt.view(), csr, 0, True, True, True,
                                                    grad_x_base=B.view())
    else:
        dx, dgb, dw = aggregate.film_wattn_backward(G.view(), X.view(), gbd, Wt.view(), attn, rate, csr, 0, True, True,
                                                    True, grad_x_base=B.view())
    arena.check(ins, [])
    moved = {k: v - before.get(k, 0) for k, v in aggregate.PATH_COUNTS.items() if v != before.get(k, 0)}
    assert moved == {f"{fam}_fwd_{key}": 1, f"{fam}_bwd_{key}": 1}, (what, moved)
    got = dict(out=out, attn=attn, rate=rate, dx=dx, dgb=dgb, dw=dw)
    for name in FAM_OUTS[fam]:
        _same_bits(got[name].reshape(dense[name].shape), dense[name], f"{what} {name}")


# ---- encoder: row strides ---------------------------------------------------------------------------------
def _within(got, f32, f64, what):
    ok, errs = stack_ref.within(got, f32, f64)
    print(what, "err, fp32 torch err", errs)
    assert ok, (what, errs)


def test_encoder_row_strides(arena):
    """``mrp_edge_encoder_fwd_split_train`` (h^T rows of ``hT_stride``), ``_bwd_prep`` (dz^T rows of
    ``dzT_stride``), ``_bwd_t`` and ``_bwd_pose`` (dh^T and h^T rows), C = 32, E = 64, rows 2^27 bytes + 8 MiB
    apart: row 16 past 2 GiB, row 31 past 4 GiB, dz^T's row 63 at 8.4 GiB.  Bars: ``stack_ref.within``
    (``tests/test_gpu_encoder_train.py``); the transpose is exact; every output's bits equal the dense run's."""
    case = "enc_c32_e64"
    C, E = sp.ENCODER[case]
    dev = arena.dev
    lib, st = m.load_library(), _st(dev)
    rows = dict(stride_bytes=sp.ROW_STRIDE)
    torch.manual_seed(E + C)
    enc = m.edge_encoder([C, C]).to(dev)
    l1, l2 = enc.layers[0], enc.layers[2]
    w1, b2 = l1.weight.detach().contiguous(), l2.bias.detach().contiguous()
    pose = (torch.randn(E, 9) * 8).to(dev)
    img = m.encoder.packed_weights(l1, l2)

    # forward: h^T sparse, the logits dense
    HT = arena.reserve((C, 1, 1, E), torch.float32, **rows)
    z, zd = torch.empty(E, 2 * C, device=dev), torch.empty(E, 2 * C, device=dev)
    hTd = torch.full((C, E), float("nan"), device=dev)
    code = lib.mrp_edge_encoder_fwd_split_train(_p(pose), _p(img), _p(b2), E, C, _p(z), HT.ptr, HT.ns, st)
    assert code == sp.expected("mrp_edge_encoder_fwd_split_train", "f32", case)
    (hT,) = arena.check([], [HT])
    hT = hT.view(C, E)
    assert lib.mrp_edge_encoder_fwd_split_train(_p(pose), _p(img), _p(b2), E, C, _p(zd), _p(hTd), E, st) == 0
    with torch.no_grad():
        h32 = torch.relu(torch.nn.functional.linear(pose, l1.weight, l1.bias)).t()
        h64 = torch.relu(torch.nn.functional.linear(pose.double(), l1.weight.double(), l1.bias.double())).t()
    _within(hT, h32, h64, "h^T")
    _same_bits(hT, hTd, "h^T")
    _same_bits(z, zd, "z")

    # dz^T = transpose(dz): exact
    dz = torch.randn(E, 2 * C, device=dev)
    DZT = arena.reserve((2 * C, 1, 1, E), torch.float32, **rows)
    code = lib.mrp_edge_encoder_bwd_prep(_p(dz), E, C, DZT.ptr, DZT.ns, st)
    assert code == sp.expected("mrp_edge_encoder_bwd_prep", "f32", case)
    (dzT,) = arena.check([], [DZT])
    _same_bits(dzT.view(2 * C, E), dz.t(), "dz^T")

    # dW1 / db1 and dpose from sparse dh^T and h^T
    gen = torch.Generator().manual_seed(E * 7 + C)
    dh_c, h_c = torch.randn(C, E, generator=gen), torch.randn(C, E, generator=gen)
    DH, HI = (arena.place(t.view(C, 1, 1, E), **rows) for t in (dh_c, h_c))
    dh, h = dh_c.to(dev), h_c.to(dev)
    d = dh * (h > 0)

    def bwd_t(dhp, dhs, hp, hs):
        nbytes = int(lib.mrp_edge_encoder_bwd_t_workspace(E, C))
        ws = torch.empty((nbytes + 3) // 4, device=dev)
        dw1, db1 = torch.full((C, 9), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
        code = lib.mrp_edge_encoder_bwd_t(dhp, dhs, hp, hs, _p(pose), E, C, _p(dw1), _p(db1), _p(ws), nbytes, st)
        torch.cuda.synchronize(dev)
        return code, dw1, db1

    code, dw1, db1 = bwd_t(DH.ptr, DH.ns, HI.ptr, HI.ns)
    assert code == sp.expected("mrp_edge_encoder_bwd_t", "f32", case)
    arena.check([DH, HI], [])
    _within(dw1, d.mm(pose), d.double().mm(pose.double()), "dW1")
    _within(db1, d.sum(1), d.double().sum(1), "db1")
    code, dw1d, db1d = bwd_t(_p(dh), E, _p(h), E)
    assert code == 0
    _same_bits(dw1, dw1d, "dW1")
    _same_bits(db1, db1d, "db1")

    def bwd_pose(dhp, dhs, hp, hs):
        nbytes = int(lib.mrp_edge_encoder_bwd_pose_workspace(E, C))
        ws = torch.empty((nbytes + 3) // 4, device=dev) if nbytes > 0 else None
        dpose = torch.full((E, 9), float("nan"), device=dev)
        code = lib.mrp_edge_encoder_bwd_pose(dhp, dhs, hp, hs, _p(w1), E, C, _p(dpose), _p(ws), nbytes, st)
        torch.cuda.synchronize(dev)
        return code, dpose

    code, dpose = bwd_pose(DH.ptr, DH.ns, HI.ptr, HI.ns)
    assert code == sp.expected("mrp_edge_encoder_bwd_pose", "f32", case)
    arena.check([DH, HI], [])
    _within(dpose, d.t().mm(w1), d.double().t().mm(w1.double()), "dpose")
    code, dposed = bwd_pose(_p(dh), E, _p(h), E)
    assert code == 0
    _same_bits(dpose, dposed, "dpose")


# ---- the checker itself ---------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["guard", "below_a_block", "behind_a_block", "tail"])
def test_checker_notices_one_stray_byte(arena, where):
    """One byte written outside the permitted blocks — in the guard, right before and right behind an output
    block beyond 4 GiB, in the tail — fails ``Arena.check``; so does one changed input bit."""
    x = torch.randn(18, 8, 2, 4).to(torch.bfloat16)
    X = arena.place(x)
    OUT = arena.reserve(x.shape, torch.bfloat16)
    arena.check([X], [OUT])
    block = sp.GUARD + OUT.off + 17 * OUT.stride_bytes
    at = {"guard": 12345, "below_a_block": block - 1, "behind_a_block": block + 8 * 2 * 4 * 2,
          "tail": sp.TOTAL - 1}[where]
    arena.buf[at] = 0
    with pytest.raises(AssertionError, match="touched outside"):
        arena.check([X], [OUT])
    arena.buf[at] = sp.SENTINEL
    arena.check([X], [OUT])
    X.node(16)[0, 0, 0] = 1.0
    with pytest.raises(AssertionError, match="input block changed"):
        arena.check([X], [OUT])
