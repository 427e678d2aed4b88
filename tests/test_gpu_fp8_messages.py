"""GPU: FP8 messages (``mrp_film_mean_fwd_q``, ``aggregate.film_mean_q`` / ``film_mean_fq``, the model option
``gcn_message_dtype``).  Every quantisation here is torch's cast on the CPU and the bytes are uploaded, so no
test rests on a GPU cast (G7 / G8 excepted: they are about the routes that quantise on the device).

The contract under test, for every graph kind, mode, ``logits``, epilogue and output type T:

    film_mean_q(xq, s, ..., out_dtype=T)  ==  film_mean(dequantize_features(xq, s) [fp32], ...).to(T)   bit for bit

Bars where a value is compared and not bits: ``fp8_cases``' docstring."""
import ctypes
import types

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib, aggregate
import fp8_cases as fc
import half_cases as hc
import oracle
import span_cases as sp

pytestmark = pytest.mark.gpu

FMTS = list(fc.FORMATS)
OUTS = list(fc.OUT_DTYPES)


def _same(a, b):
    """Numerically equal elementwise, NaN positions compared as NaN (+0 == -0)."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _pair(dev):
    return m.batch([m.RobotGraph([0, 1], [1, 0], num_nodes=2)]).csr(dev)


# ---- G1: the decode table -------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [None, 0.75, "mixed", 0.3])
@pytest.mark.parametrize("fmt", FMTS)
def test_g1_decode_table(cuda_device, fmt, scale):
    """Two robots, copy_mean, C = 2, 16 x 16 planes holding each of the 256 codes once (every plane in another
    order): robot v receives robot 1 - v's planes, so the fp32 output is ``codes.view(fmt).float() * s`` bit for
    bit — OCP, not FNUZ (255 codes differ: test_fp8_quant_cpu.py) — subnormal codes exactly, the NaN (and
    E5M2 inf) codes as NaN (inf); the bf16 / fp16 output is that value cast.  ``scale``: NULL, 0.75 (the
    issue's), a different one per (node, channel) (the index s[u, c]) and 0.3 (products that round)."""
    dev = cuda_device
    qdtype = fc.FORMATS[fmt][0]
    gen = torch.Generator().manual_seed(5)
    codes = torch.stack([fc.all_codes()[torch.randperm(256, generator=gen)] for _ in range(4)]).view(2, 2, 16, 16)
    codes[0, 0] = fc.all_codes().view(16, 16)  # one plane in code order
    if scale is None:
        s = None
    elif scale == "mixed":
        s = torch.tensor([[0.75, 1.5], [0.375, 3.0]])
    else:
        s = torch.full((2, 2), float(scale))
    want = codes.view(qdtype).float()
    if s is not None:
        want = want * s[:, :, None, None]  # one fp32 product
    want = want.flip(0)  # out[v] = x^[1 - v]
    assert bool(torch.isnan(want).any()) and (fmt == "e4m3" or bool(torch.isinf(want).any()))
    csr = _pair(dev)
    xq = codes.to(dev).view(qdtype)
    sd = s.to(dev) if s is not None else None
    for key, T in fc.OUT_DTYPES.items():
        out = aggregate.film_mean_q(xq, sd, None, csr, "copy_mean", out_dtype=T)
        assert out.dtype == T
        assert _same(out, want.to(T)), (fmt, scale, key)
        if T == torch.float32:  # bit for bit wherever a bit pattern is defined (not NaN, not a zero)
            o = out.cpu()
            keep = ~torch.isnan(want) & (want != 0)
            assert torch.equal(fc.bits(o)[keep], fc.bits(want)[keep])
    # the FNUZ reading of the same bytes would have given other values in all but the zero code
    fnuz = fc.decode_fnuz(fmt)[codes.long()]
    assert not _same(fnuz * (s[:, :, None, None] if s is not None else 1.0), want.flip(0))


# ---- G2: the contract ------------------------------------------------------------------------------------------
def _device_case(name, fmt, dev):
    xq, s, xhat, gb, z = fc.host_inputs(name, fmt)
    return fc.embed(name, xq, dev), s.to(dev), xhat.to(dev), gb.to(dev), z.to(dev)


@pytest.mark.parametrize("key", OUTS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(fc.CASES))
def test_g2_contract(cuda_device, name, fmt, key):
    """Every case of ``half_cases.CASES`` and the FP8 byte-offset views, in both formats and all three output
    types; per case the three modes with gamma/beta given and with logits: bit-equal to the fp32 ``film_mean``
    on x^ cast to T, run on the same GPU, and within the bars of the float64 oracle on x^."""
    dev = cuda_device
    T = fc.OUT_DTYPES[key]
    xq, s, xhat, gb, z = _device_case(name, fmt, dev)
    csr = fc.graph(name).csr(dev)
    n, C, H, W = fc.shape(name)
    # the slice width this case is here for (the plan query is host-only)
    plan = _lib.AggPlan()
    code = m.load_library().mrp_film_mean_fwd_q_plan(
        fc.FORMATS[fmt][1], ctypes.c_void_p(xq.data_ptr()), xq.stride(0), ctypes.c_void_p(s.data_ptr()),
        aggregate.FEATURE_DTYPES[T], *aggregate._graph_args(gb, csr, C, H * W, 0), ctypes.c_void_p(1 << 20), C * H * W,
        None, ctypes.byref(plan))
    assert code == 0
    want_vec = {"c": 4, "d": 1, "i4": 4, "v4": 4, "i1": 1, "v1": 1}.get(name, 8 if csr.max_nodes <= 8 else 4)
    if T == torch.float32:
        want_vec = min(want_vec, 4)
    assert plan.vec == want_vec, (name, plan.vec)
    before = aggregate.PATH_COUNTS["fwd_q_" + fmt]
    runs = 0
    for mode in fc.MODES:
        for logits in (False, True):
            if mode == "copy_mean" and logits:
                continue
            w = z if logits else gb
            got = aggregate.film_mean_q(xq, s, w, csr, mode, logits=logits, out_dtype=T)
            runs += 1
            ref = aggregate.film_mean(xhat, w, csr, mode, logits=logits)
            assert got.dtype == T and ref.dtype == torch.float32
            assert torch.equal(fc.bits(got), fc.bits(ref.to(T))), (name, fmt, key, mode, logits)
            if not logits:
                fc.assert_bars(got, fc.ref64(name, fmt, mode), T, f"{name} {fmt} {key} {mode}")
    assert aggregate.PATH_COUNTS["fwd_q_" + fmt] == before + runs


# ---- G3: epilogue and placement -------------------------------------------------------------------------------
@pytest.mark.parametrize("key", OUTS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["b", "e", "g"])
def test_g3_epilogue_and_placement(cuda_device, name, fmt, key):
    """Residual and mix through x0 (in the output type), ``out`` the second half of a cat buffer embedded in a
    sentinel-filled allocation: bit-equal to the fp32 ``FilmMeanFunction`` with the same epilogue, cast; not one
    byte outside ``out`` changes."""
    dev = cuda_device
    T = fc.OUT_DTYPES[key]
    es = torch.empty((), dtype=T).element_size()
    xq, s, xhat, gb, z = _device_case(name, fmt, dev)
    csr = fc.graph(name).csr(dev)
    n, C, H, W = fc.shape(name)
    gen = torch.Generator().manual_seed(17)
    h = torch.randn(n, C, H, W, generator=gen).to(T).to(dev)  # the layer's own, unquantised features
    m_flags = _lib.MODE_FILM_MEAN | _lib.GB_LOGITS
    for agg_scale, x0_scale in ((1.0, 1.0), (0.9, 0.1), (0.5, 0.0)):
        x0 = h if x0_scale else None
        ref = aggregate.FilmMeanFunction.apply(xhat, z, x0.float() if x0 is not None else None, csr, m_flags,
                                               (agg_scale, 0.0, x0_scale)).to(T)
        got = aggregate.film_mean_q(xq, s, z, csr, "film_mean", logits=True, out_dtype=T, x0=x0, agg_scale=agg_scale,
                                    x0_scale=x0_scale)
        assert torch.equal(fc.bits(got), fc.bits(ref)), (name, fmt, key, agg_scale)
        # into the second half of a (n, 2C, H, W) buffer that starts 64 bytes into a sentinel-filled allocation
        nbytes = n * 2 * C * H * W * es
        raw = torch.full((nbytes + 128,), sp.SENTINEL, dtype=torch.uint8, device=dev)
        cat = raw[64:64 + nbytes].view(T).view(n, 2 * C, H, W)
        aggregate.film_mean_q_forward_into(xq, s, z, csr, cat[:, C:], "film_mean", logits=True, x0=x0,
                                           agg_scale=agg_scale, x0_scale=x0_scale)
        assert torch.equal(fc.bits(cat[:, C:]), fc.bits(ref))
        cat[:, C:].view(torch.uint8 if es == 1 else {2: torch.int16, 4: torch.int32}[es]).fill_(
            {2: -13365, 4: -875836469}[es])  # the sentinel's bytes (0xCB...) back over out
        assert bool((raw == sp.SENTINEL).all()), "a byte outside out changed"


# ---- G4: a range-limited / drop-out batch ----------------------------------------------------------------------
@pytest.mark.parametrize("key", OUTS)
@pytest.mark.parametrize("fmt", FMTS)
def test_g4_range_limited_dropout_batch(cuda_device, fmt, key):
    """``frame_batch(max_range=..., active=...)``: kind SIMPLE, 12 robots, masked edges, robots without
    in-edges — through the same contract, and against the float64 oracle on the active edge list."""
    dev = cuda_device
    T = fc.OUT_DTYPES[key]
    B, n, C, H = 2, 12, 8, 8
    rng = np.random.RandomState(12)
    poses = np.concatenate([rng.uniform(-6, 6, (B, n, 3)), rng.standard_normal((B, n, 4))], -1).astype(np.float32)
    active = np.ones((B, n), bool)
    active[0, 5] = active[1, 0] = False
    g = m.frame_batch(torch.from_numpy(poses).to(dev), max_range=7.0, active=torch.from_numpy(active).to(dev))
    csr = g.csr(dev)
    assert csr.graph_kind == _lib.GRAPH_SIMPLE and csr.max_nodes == 12
    mask = g.edge_active
    assert 0 < int(mask.sum()) < g.num_edges()
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(B * n, C, H, H, generator=gen) * 2.0
    gb = torch.sigmoid(torch.randn(g.num_edges(), C, 2, generator=gen))
    xq, s = m.quantize_features(x, fmt)  # on the CPU
    xhat = m.dequantize_features(xq, s)
    src, dst = (t[mask].numpy() for t in g.edges())
    xqd, sd, xhd, gbd = xq.view(torch.uint8).to(dev).view(xq.dtype), s.to(dev), xhat.to(dev), gb.to(dev)
    for mode in fc.MODES:
        got = aggregate.film_mean_q(xqd, sd, gbd, csr, mode, out_dtype=T)
        ref = aggregate.film_mean(xhd, gbd, csr, mode)
        assert torch.equal(fc.bits(got), fc.bits(ref.to(T))), (fmt, key, mode)
        fc.assert_bars(got, oracle.film_aggregate(xhat.double(), gb[mask].double(), src, dst, mode), T, mode)


# ---- G5: special values ------------------------------------------------------------------------------------------
SPECIAL = [("e4m3", 0x7F, "nan"), ("e4m3", 0xFF, "nan"), ("e5m2", 0x7E, "nan"), ("e5m2", 0xFF, "nan"),
           ("e5m2", 0x7C, "inf"), ("e5m2", 0xFC, "inf")]


@pytest.mark.parametrize("fmt,code,what", SPECIAL, ids=lambda v: str(v))
@pytest.mark.parametrize("name", ["b", "e", "g"])
def test_g5_special_codes_reach_their_destinations_only(cuda_device, name, fmt, code, what):
    """One NaN (inf) code in one source pixel: non-finite exactly at the destinations that have that source as
    an in-neighbour, at that channel and pixel; every other element keeps the bits of the clean run.  Complete
    5-robot frames, k-NN(4) 16-robot frames, the ragged CSR batch (a multi-edge, a self-loop, in-degree 0)."""
    dev = cuda_device
    xq, s, _, gb, _ = fc.host_inputs(name, fmt)
    g = fc.graph(name)
    csr = g.csr(dev)
    n, C, H, W = fc.shape(name)
    src, dst = (t.numpy() for t in g.edges())
    raw = xq.view(torch.uint8).clone()
    sd, gbd = s.to(dev), gb.to(dev)
    clean = aggregate.film_mean_q(raw.to(dev).view(xq.dtype), sd, gbd, csr, "film_mean", out_dtype=torch.float32).cpu()
    assert bool(torch.isfinite(clean).all())
    sources = sorted(set(int(u) for u in src))
    for u in (sources[0], sources[len(sources) // 2], sources[-1]):
        c, p = (3 * u + 1) % C, (7 * u + 2) % (H * W)
        bad = raw.clone()
        bad.view(n, C, H * W)[u, c, p] = code
        out = aggregate.film_mean_q(bad.to(dev).view(xq.dtype), sd, gbd, csr, "film_mean",
                                    out_dtype=torch.float32).cpu()
        expect = torch.zeros(n, C, H * W, dtype=torch.bool)
        for v in set(int(v) for v in dst[src == u]):
            expect[v, c, p] = True
        assert bool(expect.any())
        expect = expect.view(n, C, H, W)
        hit = torch.isnan(out) if what == "nan" else torch.isinf(out)
        assert torch.equal(hit, expect), (name, fmt, hex(code), u)
        assert torch.equal(~torch.isfinite(out), expect)
        if what == "inf":  # gamma > 0: the sign survives
            assert bool((out[expect] < 0).all() if code & 0x80 else (out[expect] > 0).all())
        assert torch.equal(fc.bits(out)[~expect], fc.bits(clean)[~expect]), "an element elsewhere changed"


@pytest.mark.parametrize("fmt", FMTS)
def test_g5_subnormal_codes_times_a_scale_below_one(cuda_device, fmt):
    """The subnormal codes of either sign (E4M3: 7, E5M2: 3 a sign) with scales below 1, some of them far
    below: the exact fp32 product, no flush to zero on the way."""
    dev = cuda_device
    qdtype, mant = fc.FORMATS[fmt][0], (3 if fmt == "e4m3" else 2)
    sub = [c | sgn for sgn in (0, 0x80) for c in range(1, 1 << mant)]
    codes = torch.tensor(sub * 16, dtype=torch.int16).to(torch.uint8)[:2 * 2 * 16].view(2, 2, 4, 4)
    s = torch.tensor([[0.75, 0.3], [2.0 ** -20 * 0.7, 1e-30]])
    want = (codes.view(qdtype).float() * s[:, :, None, None]).flip(0)
    assert bool((want != 0).all())
    out = aggregate.film_mean_q(codes.to(dev).view(qdtype), s.to(dev), None, _pair(dev), "copy_mean",
                                out_dtype=torch.float32)
    assert torch.equal(fc.bits(out), fc.bits(want))


# ---- G6: span ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena(cuda_device):
    a = sp.Arena(cuda_device)
    yield a
    del a.buf


@pytest.mark.parametrize("fmt,key", [("e4m3", "bf16"), ("e5m2", "f32"), ("e4m3", "f16")])
def test_g6_span(arena, fmt, key):
    """2 x 12 robots whose node blocks lie ``span_cases.NODE_STRIDE`` bytes apart in a ``torch.uint8`` arena (node
    16 onward is more than 2^32 bytes from node 0): first the FP8 codes placed so and a dense output, then dense
    codes and the output (and the epilogue's x0) placed so.  No span is declined (the header says so): both runs
    return the dense run's bits, and no sentinel byte outside the outputs changes."""
    dev = arena.dev
    T = fc.OUT_DTYPES[key]
    g = hc._frames([12, 12], 31)
    csr = g.csr(dev)
    n, C, H, W = g.num_nodes(), 8, 8, 8
    assert n == 24 and (n - 1) * sp.NODE_STRIDE > 1 << 32
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(n, C, H, W, generator=gen)
    z = torch.randn(g.num_edges(), C, 2, generator=gen).to(dev)
    h = torch.randn(n, C, H, W, generator=gen).to(T)
    xq, s = m.quantize_features(x, fmt)
    raw = xq.view(torch.uint8)
    sd = s.to(dev)
    kw = dict(mode="film_mean", logits=True, agg_scale=0.9, x0_scale=0.1)
    dense = aggregate.film_mean_q(raw.to(dev).view(xq.dtype), sd, z, csr, out_dtype=T, x0=h.to(dev), **kw).cpu()
    try:
        # (1) the codes' node blocks more than 2^32 bytes apart
        X = arena.place(raw)
        assert X.ns == sp.NODE_STRIDE  # elements = bytes
        out1 = aggregate.film_mean_q(X.view().view(xq.dtype), sd, z, csr, out_dtype=T, x0=h.to(dev), **kw)
        assert torch.equal(fc.bits(out1), fc.bits(dense))
        arena.check([X], [])
        # (2) the output's and x0's node blocks more than 2^32 bytes apart
        X0 = arena.place(h)
        OUT = arena.reserve((n, C, H, W), T)
        aggregate.film_mean_q_forward_into(raw.to(dev).view(xq.dtype), sd, z, csr, OUT.view(), x0=X0.view(), **kw)
        (got,) = arena.check([X, X0], [OUT])
        assert torch.equal(fc.bits(got), fc.bits(dense))
        # (3) both at once
        OUT2 = arena.reserve((n, C, H, W), T)
        aggregate.film_mean_q_forward_into(X.view().view(xq.dtype), sd, z, csr, OUT2.view(), x0=X0.view(), **kw)
        (got,) = arena.check([X, X0], [OUT2])
        assert torch.equal(fc.bits(got), fc.bits(dense))
    finally:
        arena.clear()


# ---- G7: fake-quant ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", OUTS)
@pytest.mark.parametrize("per", ["channel", "node"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["b", "e", "g"])
def test_g7_fake_quant_route(cuda_device, name, fmt, per, key):
    """``film_mean_fq``: forward bits == ``film_mean_q`` on ``quantize_features(x)``; dx and dgb == the fp32
    ``film_mean`` backward on x^, bit for bit (the straight-through estimator); the inference op refuses to drop
    a gradient."""
    dev = cuda_device
    T = fc.OUT_DTYPES[key]
    n, C, H, W = fc.shape(name)
    csr = fc.graph(name).csr(dev)
    gen = torch.Generator().manual_seed(23)
    x = (torch.randn(n, C, H, W, generator=gen) * 2).to(T).to(dev).requires_grad_(True)
    z = torch.randn(csr.num_edges, C, 2, generator=gen).to(dev).requires_grad_(True)
    G = torch.randn(n, C, H, W, generator=gen).to(T).to(dev)
    before = dict(aggregate.PATH_COUNTS)
    out = aggregate.film_mean_fq(x, z, csr, fmt, per, "film_mean", logits=True)
    assert out.dtype == T and aggregate.PATH_COUNTS["fwd_q_" + fmt] == before.get("fwd_q_" + fmt, 0)
    out.backward(G)
    xq, s = m.quantize_features(x, fmt, per)  # on the device: the route's own quantiser
    with torch.no_grad():
        native = aggregate.film_mean_q(xq, s, z, csr, "film_mean", logits=True, out_dtype=T)
    assert torch.equal(fc.bits(out), fc.bits(native))
    xhat = m.dequantize_features(xq, s).requires_grad_(True)
    z2 = z.detach().clone().requires_grad_(True)
    ref = aggregate.film_mean(xhat, z2, csr, "film_mean", logits=True)
    ref.backward(G.float())
    assert x.grad.dtype == T and torch.equal(fc.bits(x.grad), fc.bits(xhat.grad.to(T)))
    assert torch.equal(fc.bits(z.grad), fc.bits(z2.grad))
    with pytest.raises(RuntimeError, match="film_mean_fq"):
        aggregate.film_mean_q(xq, s, z, csr, "film_mean", logits=True, out_dtype=T)
    with pytest.raises(RuntimeError, match="film_mean_fq"):
        aggregate.film_mean_q(xq, s, z.detach(), csr, "film_mean", logits=True, out_dtype=T,
                              x0=x, x0_scale=1.0)
    aggregate.film_mean_q(xq, s, z.detach(), csr, "film_mean", logits=True, out_dtype=T)  # nothing to drop: fine


# ---- G8: the model ----------------------------------------------------------------------------------------------
STACKS = [("cat_compress", 1), ("cat_compress", 2), ("cat", 1), ("residual", 1), ("residual", 2), ("initial_mix", 1),
          ("initial_mix", 2)]
FRAMES = {"complete5": ((5, 5), None), "knn4x16": ((16, 16), 4)}
MC, MHW = 32, 8


def _model_frames(which, dev):
    ns, knn = FRAMES[which]
    rng = np.random.RandomState(41)
    g = m.batch([m.frame_graph(hc._poses(rng, n), knn=knn) for n in ns])
    x = torch.randn(g.num_nodes(), MC, MHW, MHW, generator=torch.Generator().manual_seed(43))
    return g.to(dev), x


def _q_counts():
    return aggregate.PATH_COUNTS["fwd_q_e4m3"] + aggregate.PATH_COUNTS["fwd_q_e5m2"]


@pytest.mark.parametrize("key", ["bf16", "f32"])
@pytest.mark.parametrize("mdtype", ["fp8_e4m3", "fp8_e5m2"])
@pytest.mark.parametrize("which", list(FRAMES))
@pytest.mark.parametrize("combine,layers", STACKS)
def test_g8_stack_routes_agree(cuda_device, combine, layers, which, mdtype, key):
    """``GCNStack`` with ``gcn_message_dtype``: the ``torch.no_grad()`` route (quantise + the native FP8 kernel)
    and the grad-mode route (fake-quant on the fp32 kernels) return the same bits; ``fwd_q_*`` counts only on the
    no-grad route; the encoder, the convs and the features get gradients."""
    dev = cuda_device
    T = fc.OUT_DTYPES[key]
    gd, x = _model_frames(which, dev)
    torch.manual_seed(5)
    opt = types.SimpleNamespace(feature_dim=MC, gcn_layers=layers, gcn_combine=combine, gcn_message_dtype=mdtype,
                                gcn_message_scale="node" if layers == 2 else "channel")
    stack = m.GCNStack(opt).to(dev)
    leaf = x.to(T).to(dev).requires_grad_(True)
    q0 = _q_counts()
    out = stack(gd, leaf)
    assert _q_counts() == q0, "the grad-mode route launched the inference kernel"
    assert out.dtype == T and tuple(out.shape) == (x.shape[0], 2 * MC if combine == "cat" else MC, MHW, MHW)
    out.float().square().sum().backward()
    assert leaf.grad is not None and leaf.grad.dtype == T and bool(torch.isfinite(leaf.grad.float()).all())
    assert bool(leaf.grad.float().abs().sum() > 0)
    for pname, p in stack.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), pname
        assert bool(p.grad.abs().sum() > 0), pname
    with torch.no_grad():
        q0 = _q_counts()
        fast = stack(gd, leaf.detach())
        assert _q_counts() == q0 + layers
        assert aggregate.PATH_COUNTS["fwd_q_" + mdtype[4:]] >= layers
    assert fast.dtype == T and torch.equal(fc.bits(fast), fc.bits(out))


@pytest.mark.parametrize("key", ["bf16", "f32"])
@pytest.mark.parametrize("mdtype", ["fp8_e4m3", "fp8_e5m2"])
@pytest.mark.parametrize("which", list(FRAMES))
def test_g8_gcn_forward_against_the_unquantised_run(cuda_device, which, mdtype, key):
    """A single ``GCN.forward``: both routes agree bit for bit, and the result stays within ``u max|x|`` (gamma,
    beta in (0, 1) and a mean amplify no input error) + the output type's bar of the unquantised run."""
    dev = cuda_device
    T = fc.OUT_DTYPES[key]
    gd, x = _model_frames(which, dev)
    xd = x.to(T).to(dev)
    torch.manual_seed(7)
    plain = m.GCN(types.SimpleNamespace(feature_dim=MC)).to(dev)
    quant = m.GCN(types.SimpleNamespace(feature_dim=MC, gcn_message_dtype=mdtype)).to(dev)
    quant.load_state_dict(plain.state_dict())
    leaf = xd.clone().requires_grad_(True)
    slow = quant(gd, leaf)
    slow.float().sum().backward()
    assert leaf.grad is not None and all(p.grad is not None for p in quant.parameters())
    with torch.no_grad():
        q0 = _q_counts()
        fast = quant(gd, xd)
        assert _q_counts() == q0 + 1
        ref = plain(gd, xd.float())
    assert fast.dtype == T and torch.equal(fc.bits(fast), fc.bits(slow))
    u = fc.FORMATS[mdtype[4:]][3]
    refd, gotd = ref.double().cpu(), fast.double().cpu()
    bound = u * float(xd.float().abs().max()) + fc.UNIT[T] * refd.abs() + 1e-5 * float(refd.abs().max())
    excess = float(((gotd - refd).abs() - bound).max())
    print(which, mdtype, key, "worst", float((gotd - refd).abs().max()), "u max|x|", u * float(xd.float().abs().max()))
    assert excess <= 0.0
