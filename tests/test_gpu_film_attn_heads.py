"""Multi-head attention fusion on the GPU (``heads=H`` of film_attn / film_wattn, ``mrp_film_*attn_*_mh``).

The contract is bit-level: head k of the H-head call is the single-head operator on channel slice k, for every
output; grad_w is the heads' sum, ascending.  Around it: H = 1 is the existing operators, fp32 accuracy against
the float64 restatement (tests/heads_cases.py) at the suite's bar, the 16-bit contract, the weights' row sums,
the gated form's consequences, strided operands, non-finite containment per head, determinism, autograd and
the GCN option.

Accuracy measured (fp32 against float64, every case x graph, relative max-norm; the bar is 1e-5):
film_attn heads: out 3.1e-07, attn 3.4e-07, dx 3.5e-07, dgb 4.1e-07;
film_wattn heads: out 4.0e-07, attn 2.2e-07, rate 6.0e-07, dx 8.6e-07, dgb 2.8e-07, dw 5.3e-07.
"""
import types

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib, aggregate
import heads_cases as hc
import wattn_cases as wc
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5  # the suite's bar; tests/test_film_attn_heads_cpu.py shows its teeth
ULP1 = 2.0 ** -23  # fp32 spacing at 1
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
KEYS = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
NAMES = ("out", "attn", "rate", "dx", "dgb", "dw")
PAIRS = [(n, c) for n in hc.GRAPHS for c in hc.CASES]
PAIR_IDS = [f"{n}-{i}" for n in hc.GRAPHS for i in hc.CASE_IDS]
KINDS = {"complete8": _lib.GRAPH_COMPLETE, "loud_csr": _lib.GRAPH_CSR, "knn16_4": _lib.graph_regular(4),
         "range12": _lib.GRAPH_SIMPLE}
OPS = ("attn", "wattn")


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(INT_VIEW[a.dtype]), b.view(INT_VIEW[b.dtype]))


def close(got, ref):
    return rel_err(got.detach().float().cpu().numpy(), ref.numpy()) <= TOL


def _cpu(t):
    return None if t is None else t.cpu()


def run(dev, g, x, gb, H, w=None, G=None, base=None, logits=False, need=(True, True, True), heads_kw=True):
    """[out, attn, rate, dx, dgb, dw] on the host of the H-head entry points (no autograd); rate and dw None
    without ``w``.  ``heads_kw=False`` leaves the argument out (the existing single-head calls)."""
    csr = g.csr(dev)
    flags = _lib.GB_LOGITS if logits else 0
    kw = {"heads": H} if heads_kw else {}
    xd, gbd = x.to(dev), gb.to(dev)
    out = torch.empty(tuple(x.shape), device=dev, dtype=x.dtype)
    bd = None if base is None else base.to(dev)
    if w is None:
        attn = m.film_attn_forward_into(xd, gbd, csr, flags, out, **kw)
        if G is None:
            return [out.cpu(), attn.cpu(), None, None, None, None]
        dx, dgb = m.film_attn_backward(G.to(dev), xd, gbd, attn, csr, flags, need[0], need[1], grad_x_base=bd, **kw)
        return [out.cpu(), attn.cpu(), None, _cpu(dx), _cpu(dgb), None]
    wd = w.to(dev)
    attn, rate = m.film_wattn_forward_into(xd, gbd, wd, csr, flags, out, rate=True, **kw)
    if G is None:
        return [out.cpu(), attn.cpu(), rate.cpu(), None, None, None]
    dx, dgb, dw = m.film_wattn_backward(G.to(dev), xd, gbd, wd, attn, rate, csr, flags, *need, grad_x_base=bd, **kw)
    return [out.cpu(), attn.cpu(), rate.cpu(), _cpu(dx), _cpu(dgb), _cpu(dw)]


def per_head(dev, g, x, gb, H, w=None, G=None, base=None, logits=False):
    """The same list assembled from the existing single-head entry points on the heads' channel slices: x, out,
    grad_out and the base as strided views of the full tensors (offset k Ch P, the full node stride), a contiguous
    copy of gb's columns, attn[k] / rate[k]; grad_w summed over the heads, ascending, in fp32."""
    csr = g.csr(dev)
    flags = _lib.GB_LOGITS if logits else 0
    N, C, hh, ww = x.shape
    Ch, E, P = C // H, g.num_edges(), hh * ww
    xd, gbd = x.to(dev), gb.to(dev)
    Gd = None if G is None else G.to(dev)
    bd = None if base is None else base.to(dev)
    wd = None if w is None else w.to(dev)
    out = torch.empty(tuple(x.shape), device=dev, dtype=x.dtype)
    attn = torch.empty((H, E, P), device=dev)
    rate = None if w is None else torch.empty((H, E, P), device=dev)
    dx = None if G is None else torch.empty(tuple(x.shape), device=dev, dtype=x.dtype)
    dgb = None if G is None else torch.empty((E, C, 2), device=dev)
    dw = None
    for k in range(H):
        sl = slice(k * Ch, (k + 1) * Ch)
        gbk = gbd[:, sl].contiguous()
        bk = None if bd is None else bd[:, sl]
        if w is None:
            m.film_attn_forward_into(xd[:, sl], gbk, csr, flags, out[:, sl], attn=attn[k])
            if G is not None:
                dxk, dgbk = m.film_attn_backward(Gd[:, sl], xd[:, sl], gbk, attn[k], csr, flags, True, True,
                                                 grad_x_base=bk)
        else:
            m.film_wattn_forward_into(xd[:, sl], gbk, wd, csr, flags, out[:, sl], attn=attn[k], rate=rate[k])
            if G is not None:
                dxk, dgbk, dwk = m.film_wattn_backward(Gd[:, sl], xd[:, sl], gbk, wd, attn[k], rate[k], csr, flags,
                                                       True, True, True, grad_x_base=bk)
                dw = dwk if dw is None else dw + dwk  # head 0's value first, one fp32 add per further head
        if G is not None:
            dx[:, sl] = dxk
            dgb[:, sl] = dgbk
    return [out.cpu(), attn.cpu(), _cpu(rate), _cpu(dx), _cpu(dgb), _cpu(dw)]


def _ops(name, case, op):
    g, x, gb, z, G, base, w = hc.operands(name, case)
    return g, x, gb, z, G, base, (w if op == "wattn" else None)


# ------------------------------------------------------------------------------------------------ 1. the contract
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name,case", PAIRS, ids=PAIR_IDS)
def test_head_k_is_the_single_head_operator_on_slice_k(cuda_device, name, case, op):
    g, x, gb, z, G, base, w = _ops(name, case, op)
    H = case[1]
    assert g.csr(cuda_device).graph_kind == KINDS[name]
    for T in (torch.float32, torch.bfloat16, torch.float16):
        for logits, p in ((False, gb), (True, z)):
            before = {k: aggregate.PATH_COUNTS[f"{op}_{d}_mh_{KEYS[T]}"] for k, d in (("f", "fwd"), ("b", "bwd"))}
            got = run(cuda_device, g, x.to(T), p, H, w, G.to(T), base.to(T), logits)
            if H > 1:
                assert aggregate.PATH_COUNTS[f"{op}_fwd_mh_{KEYS[T]}"] == before["f"] + 1
                assert aggregate.PATH_COUNTS[f"{op}_bwd_mh_{KEYS[T]}"] == before["b"] + 1
                assert tuple(got[1].shape) == (H, g.num_edges(), case[2] * case[3])
            ref = per_head(cuda_device, g, x.to(T), p, H, w, G.to(T), base.to(T), logits)
            if H == 1:
                ref[1] = ref[1][0]
                ref[2] = None if ref[2] is None else ref[2][0]
            for k, a, b in zip(NAMES, got, ref):
                assert (a is None and b is None) or bits_equal(a, b), (k, T, logits)
            # without the base: the same grad_gb (and grad_w), grad_x of its own
            nb = run(cuda_device, g, x.to(T), p, H, w, G.to(T), None, logits)
            rb = per_head(cuda_device, g, x.to(T), p, H, w, G.to(T), None, logits)
            assert bits_equal(nb[3], rb[3]) and bits_equal(nb[4], got[4])
            assert w is None or bits_equal(nb[5], got[5])
            assert not bits_equal(nb[3], got[3])


# ------------------------------------------------------------------------------------------------ 2. H = 1
def _mh_entry_points(dev, g, x, gb, w, G, base, heads):
    """The four _mh entry points called directly (ctypes): out, attn, rate, dx, dgb, dw."""
    lib = _lib.load_library()
    csr = g.csr(dev)
    N, C, hh, ww = x.shape
    P, E = hh * ww, g.num_edges()
    xd, gbd, Gd, bd = x.to(dev), gb.to(dev).contiguous(), G.to(dev), base.to(dev)
    T = aggregate.FEATURE_DTYPES[x.dtype]
    ga = aggregate._graph_args(gbd, csr, C, P, 0)
    ptr, st = aggregate._ptr, aggregate._stream(dev)
    scale = hc.head_scale(C, heads)
    out, dx = torch.empty_like(xd), torch.empty_like(xd)
    attn = torch.empty((heads, E, P), device=dev)
    dgb = torch.empty((E, C, 2), device=dev)
    sizes = (1, csr.num_graphs, csr.max_nodes, csr.graph_kind, csr.num_nodes, csr.num_edges, C, P, heads)
    if w is None:
        assert lib.mrp_film_attn_fwd_mh(T, ptr(xd), C * P, *ga, heads, ptr(out), C * P, scale, ptr(attn), None, 0,
                                        st) == 0
        nbytes = lib.mrp_film_attn_workspace_mh(*sizes)
        ws = torch.empty(max(nbytes // 4, 1), device=dev)
        assert lib.mrp_film_attn_bwd_mh(T, ptr(Gd), C * P, ptr(xd), C * P, *ga, heads, ptr(dx), C * P, ptr(bd), C * P,
                                        ptr(dgb), scale, ptr(attn), ptr(ws), nbytes, st) == 0
        return [out.cpu(), attn.cpu(), None, dx.cpu(), dgb.cpu(), None]
    wd = w.to(dev)
    rate = torch.empty((heads, E, P), device=dev)
    dw = torch.empty((N, hh, ww), device=dev)
    assert lib.mrp_film_wattn_fwd_mh(T, ptr(xd), C * P, ga[0], ptr(wd), P, *ga[1:], heads, ptr(out), C * P, scale,
                                     ptr(attn), ptr(rate), None, 0, st) == 0
    nbytes = lib.mrp_film_wattn_workspace_mh(*sizes)
    ws = torch.empty(max(nbytes // 4, 1), device=dev)
    assert lib.mrp_film_wattn_bwd_mh(T, ptr(Gd), C * P, ptr(xd), C * P, ga[0], ptr(wd), P, *ga[1:], heads, ptr(dx),
                                     C * P, ptr(bd), C * P, ptr(dgb), scale, ptr(attn), ptr(rate), ptr(dw), P, ptr(ws),
                                     nbytes, st) == 0
    return [out.cpu(), attn.cpu(), rate.cpu(), dx.cpu(), dgb.cpu(), dw.cpu()]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", list(hc.GRAPHS))
def test_one_head_is_the_existing_operator(cuda_device, name, op):
    case = (12, 1, 8, 8)
    g, x, gb, z, G, base, w = _ops(name, case, op)
    for T in (torch.float32, torch.bfloat16, torch.float16):
        old = run(cuda_device, g, x.to(T), gb, 1, w, G.to(T), base.to(T), heads_kw=False)
        keys = [f"{op}_{d}_{KEYS[T]}" for d in ("fwd", "bwd")] + [f"{op}_{d}_mh_{KEYS[T]}" for d in ("fwd", "bwd")]
        before = [aggregate.PATH_COUNTS[k] for k in keys]
        new = run(cuda_device, g, x.to(T), gb, 1, w, G.to(T), base.to(T))
        # heads=1 takes today's path: the existing keys advance, the _mh ones do not
        assert [aggregate.PATH_COUNTS[k] for k in keys] == [before[0] + 1, before[1] + 1, before[2], before[3]]
        direct = _mh_entry_points(cuda_device, g, x.to(T), gb, w, G.to(T), base.to(T), 1)
        direct[1] = direct[1][0]
        direct[2] = None if direct[2] is None else direct[2][0]
        for k, a, b, c in zip(NAMES, old, new, direct):
            assert (a is None and b is None and c is None) or (bits_equal(a, b) and bits_equal(a, c)), (k, T)
        assert tuple(new[1].shape) == (g.num_edges(), 64)


@pytest.mark.parametrize("op", OPS)
def test_the_entry_points_called_directly(cuda_device, op):
    """The _mh entry points through ctypes with H > 1 against the ops (which add nothing but checks)."""
    case = (27, 3, 8, 10)
    for name in ("complete8", "range12"):
        g, x, gb, z, G, base, w = _ops(name, case, op)
        direct = _mh_entry_points(cuda_device, g, x, gb, w, G, base, 3)
        got = run(cuda_device, g, x, gb, 3, w, G, base)
        for k, a, b in zip(NAMES, direct, got):
            assert (a is None and b is None) or bits_equal(a, b), k


# ------------------------------------------------------------------------------------------------ 3. accuracy
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name,case", PAIRS, ids=PAIR_IDS)
def test_against_float64(cuda_device, name, case, op):
    g, x, gb, z, G, base, w = _ops(name, case, op)
    H = case[1]
    ref = list(hc.direct_reference(g, x, z, H, G, base, True, w=w))
    got = run(cuda_device, g, x, z, H, w, G, base, True)
    if H == 1:
        ref[1] = ref[1][0]
        ref[2] = None if ref[2] is None else ref[2][0]
    errs = {k: rel_err(a.numpy(), b.numpy()) for k, a, b in zip(NAMES, got, ref) if b is not None}
    print(op, name, case, errs)
    assert set(errs) == (set(NAMES) if w is not None else {"out", "attn", "dx", "dgb"})
    assert max(errs.values()) <= TOL and all(np.isfinite(list(errs.values())))


# ------------------------------------------------------------------------------------------------ 4. 16-bit contract
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("T", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name,case", [p for p in PAIRS if p[1][1] > 1][::3], ids=[
    i for i, p in zip(PAIR_IDS, PAIRS) if p[1][1] > 1][::3])
def test_16_bit_contract(cuda_device, name, case, T, op):
    g, x, gb, z, G, base, w = _ops(name, case, op)
    H = case[1]
    xT, GT, bT = x.to(T), G.to(T), base.to(T)
    got = run(cuda_device, g, xT, z, H, w, GT, bT, True)
    wide = run(cuda_device, g, xT.float(), z, H, w, GT.float(), bT.float(), True)
    assert got[0].dtype == T and got[3].dtype == T
    assert bits_equal(got[0], wide[0].to(T)) and bits_equal(got[3], wide[3].to(T))
    for i in (1, 2, 4, 5):
        assert (got[i] is None and wide[i] is None) or (got[i].dtype == torch.float32 and bits_equal(got[i], wide[i]))


# ------------------------------------------------------------------------------------------------ 5. the weights
@pytest.mark.parametrize("name", list(hc.GRAPHS))
def test_weights_sum_to_one_per_head_and_unnamed_rows_are_zero(cuda_device, name):
    for case in ((27, 3, 8, 10), (8, 8, 4, 4)):
        g, x, gb, z, G, base, _ = hc.operands(name, case)
        H = case[1]
        attn = run(cuda_device, g, x, gb, H)[1]
        indptr, src, eid = hc.ac.rows(g)
        named = torch.zeros(g.num_edges(), dtype=torch.bool)
        named[torch.as_tensor(eid[: int(indptr[-1])].astype(np.int64))] = True
        if name == "range12":
            assert not bool(named.all())  # the case that has rows no entry names
        for v in range(g.num_nodes()):
            lo, hi = int(indptr[v]), int(indptr[v + 1])
            if hi == lo:
                continue
            e = torch.as_tensor(eid[lo:hi].astype(np.int64))
            assert float((attn[:, e].double().sum(1) - 1.0).abs().max()) <= 16 * ULP1  # every head, every pixel
        assert bool((attn[:, ~named] == 0).all()) and bool((attn[:, named] >= 0).all())
        assert not bits_equal(attn[0], attn[1])  # the heads have their own softmaxes


# ------------------------------------------------------------------------------------------------ 6. the gated form
@pytest.mark.parametrize("name,case", PAIRS[::2], ids=PAIR_IDS[::2])
def test_unit_maps_are_multi_head_film_attn(cuda_device, name, case):
    g, x, gb, z, G, base, _ = hc.operands(name, case)
    H = case[1]
    ones = torch.ones(g.num_nodes(), case[2], case[3])
    got = run(cuda_device, g, x, z, H, ones, G, base, True)
    ref = run(cuda_device, g, x, z, H, None, G, base, True)
    assert bits_equal(got[0], ref[0]) and bits_equal(got[1], ref[1]) and bits_equal(got[2], ref[1])
    assert bits_equal(got[3], ref[3]) and bits_equal(got[4], ref[4])
    assert bool(torch.isfinite(got[5]).all())


@pytest.mark.parametrize("name", ["complete8", "knn16_4"])
@pytest.mark.parametrize("case", [(6, 2, 7, 7), (27, 3, 8, 10)])
def test_a_robot_mask_is_multi_head_film_attn_on_the_pruned_graph(cuda_device, name, case):
    g, x, gb, z, G, base, _ = hc.operands(name, case)
    H = case[1]
    N = g.num_nodes()
    silent = np.zeros(N, bool)
    silent[[1, 4, N - 2]] = True
    w = torch.as_tensor(~silent).float()[:, None, None].expand(N, case[2], case[3]).contiguous()
    got = run(cuda_device, g, x, gb, H, w, G, base)
    ref = run(cuda_device, wc.compacted(g, silent), x, gb, H, None, G, base)
    for i in (0, 1, 3, 4):
        assert bits_equal(got[i], ref[i]), NAMES[i]


@pytest.mark.parametrize("case", [(6, 2, 7, 7), (27, 3, 8, 10)])
def test_a_silent_senders_nan_reaches_only_its_own_rate_and_grad_w(cuda_device, case):
    g, x, gb, z, G, base, w = hc.operands("loud_csr", case)
    H, C = case[1], case[0]
    q, rowless = wc.silent_node(g)
    assert rowless and bool((w[q] == 0).all())
    clean = run(cuda_device, g, x, gb, H, w, G, base)
    xs = x.clone()
    xs[q, 0, 1, 2] = float("nan")
    xs[q, C - 1, 3, 4] = float("inf")
    xs[q, 1, 5, 5] = -float("inf")
    xs[q, :, 6, 6] = 3.0e38
    got = run(cuda_device, g, xs, gb, H, w, G, base)
    own = torch.as_tensor(np.asarray(g.edges()[0]) == q)
    keep = torch.arange(x.shape[0]) != q
    for k, a, b in zip(NAMES, got, clean):
        if k == "rate":
            assert bits_equal(a[:, ~own], b[:, ~own])
            assert not bool(torch.isfinite(a[:, own]).all())  # it does reach the sender's own rate
        elif k == "dw":
            assert bits_equal(a[keep], b[keep])
            assert not bool(torch.isfinite(a[q]).all())
        else:
            assert bits_equal(a, b), k


# ------------------------------------------------------------------------------------------------ 7. strided operands
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["complete8", "loud_csr"])
def test_strided_operands(cuda_device, name, T, op):
    case = (27, 3, 8, 10)
    g, x, gb, z, G, base, w = _ops(name, case, op)
    C, H, hh, ww = case
    dev = cuda_device
    csr = g.csr(dev)
    N = x.shape[0]
    dense = run(dev, g, x.to(T), gb, H, w, G.to(T), base.to(T))
    xbuf = torch.full((N, 2 * C, hh, ww), 7.0, device=dev, dtype=T)
    xbuf[:, :C] = x.to(dev)
    cat = torch.full((N, 2 * C, hh, ww), -5.0, device=dev, dtype=T)
    gbuf = torch.full((N, 2 * C, hh, ww), 3.0, device=dev, dtype=T)
    gbuf[:, C:] = G.to(dev)
    gbuf[:, :C] = base.to(dev)
    gbd = gb.to(dev)
    if w is None:
        attn = m.film_attn_forward_into(xbuf[:, :C], gbd, csr, 0, cat[:, C:], heads=H)
        dx, dgb = m.film_attn_backward(gbuf[:, C:], xbuf[:, :C], gbd, attn, csr, 0, True, True,
                                       grad_x_base=gbuf[:, :C], heads=H)
        rate = dw = None
    else:
        wbuf = torch.full((N, 3, hh, ww), -1.0, device=dev)  # the map is the middle plane of three
        wbuf[:, 1] = w.to(dev)
        attn, rate = m.film_wattn_forward_into(xbuf[:, :C], gbd, wbuf[:, 1], csr, 0, cat[:, C:], rate=True, heads=H)
        dx, dgb, dw = m.film_wattn_backward(gbuf[:, C:], xbuf[:, :C], gbd, wbuf[:, 1], attn, rate, csr, 0, True, True,
                                            True, grad_x_base=gbuf[:, :C], heads=H)
        assert bool((wbuf[:, [0, 2]] == -1.0).all())
    for k, a, b in zip(NAMES, (cat[:, C:], attn, rate, dx, dgb, dw), dense):
        assert (a is None and b is None) or bits_equal(a, b), k
    # the gaps: untouched
    assert bool((cat[:, :C] == -5.0).all()) and bool((xbuf[:, C:] == 7.0).all())
    assert bits_equal(gbuf[:, C:], G.to(T)) and bits_equal(gbuf[:, :C], base.to(T))
    # the compositions with heads against torch's on the dense result
    xd = x.to(dev).to(T).requires_grad_(True)
    gd = gb.to(dev).requires_grad_(True)
    if w is None:
        args = (xd, gd, csr)
        fns = aggregate.film_attn_cat, aggregate.film_attn_residual, aggregate.film_attn_mix
    else:
        wd = w.to(dev).requires_grad_(True)
        args = (xd, gd, wd, csr)
        fns = aggregate.film_wattn_cat, aggregate.film_wattn_residual, aggregate.film_wattn_mix
    buf, attn2 = fns[0](*args, return_weights=True, heads=H)
    assert bits_equal(buf[:, :C], x.to(T)) and bits_equal(buf[:, C:], dense[0]) and bits_equal(attn2, dense[1])
    buf.backward(gbuf)
    assert bits_equal(xd.grad, dense[3]) and bits_equal(gd.grad, dense[4])
    assert w is None or bits_equal(wd.grad, dense[5])
    with torch.no_grad():
        d_out, x0 = dense[0].to(dev), base.to(dev).to(T)
        assert bits_equal(fns[1](*args, heads=H), xd + d_out)
        assert bits_equal(fns[2](*args, x0, 0.25, heads=H), 0.75 * d_out + 0.25 * x0)


# ------------------------------------------------------------------------------------------------ 8. containment
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_value_stays_in_its_head(cuda_device, op, bad):
    case = (16, 2, 8, 8)
    g, x, gb, z, G, base, w = _ops("complete8", case, op)
    C, H, hh, ww = case
    Ch, P = C // H, hh * ww
    if w is not None:
        w = w.clamp(min=0.25)  # everybody delivers everywhere: the value is heard
    clean = run(cuda_device, g, x, gb, H, w, G, base)
    xs = x.clone()
    node, c, py, px = 2, Ch + 3, 3, 5  # graph 0, a channel of head 1
    xs[node, c, py, px] = bad
    got = run(cuda_device, g, xs, gb, H, w, G, base)
    p = py * ww + px
    other_p = torch.arange(P) != p
    out, attn, rate, dx, dgb, dw = got
    c_out, c_attn, c_rate, c_dx, c_dgb, c_dw = clean
    # head 0: the clean run's bits, everywhere
    assert bits_equal(out[:, :Ch], c_out[:, :Ch]) and bits_equal(attn[0], c_attn[0])
    assert bits_equal(dx[:, :Ch], c_dx[:, :Ch]) and bits_equal(dgb[:, :Ch], c_dgb[:, :Ch])
    assert rate is None or bits_equal(rate[0], c_rate[0])
    # head 1: every other pixel and the other graph
    flat = lambda t: t.reshape(t.shape[0], t.shape[1], P)  # noqa: E731
    assert bits_equal(flat(out)[:, :, other_p], flat(c_out)[:, :, other_p])
    assert bits_equal(flat(dx)[:, :, other_p], flat(c_dx)[:, :, other_p])
    assert bits_equal(attn[:, :, other_p], c_attn[:, :, other_p])
    assert bits_equal(out[8:], c_out[8:]) and bits_equal(dx[8:], c_dx[8:])
    second = torch.as_tensor(np.asarray(g.edges()[0]) >= 8)
    assert bits_equal(attn[:, second], c_attn[:, second]) and bits_equal(dgb[second], c_dgb[second])
    if w is not None:
        assert bits_equal(rate[:, :, other_p], c_rate[:, :, other_p])
        assert bits_equal(dw.reshape(-1, P)[:, other_p], c_dw.reshape(-1, P)[:, other_p])
        assert bits_equal(dw[8:], c_dw[8:])
    # and it does reach head 1 at that pixel
    assert not bool(torch.isfinite(flat(out)[:8, Ch:, p]).all())
    assert bool(torch.isfinite(flat(out)[:, :Ch]).all())


# ------------------------------------------------------------------------------------------------ 9. determinism
@pytest.mark.parametrize("op", OPS)
def test_deterministic(cuda_device, op):
    case = (27, 3, 8, 10)
    for name in ("knn16_4", "loud_csr"):
        g, x, gb, z, G, base, w = _ops(name, case, op)
        a = run(cuda_device, g, x, z, 3, w, G, base, True)
        b = run(cuda_device, g, x, z, 3, w, G, base, True)
        for k, p, q in zip(NAMES, a, b):
            assert (p is None and q is None) or bits_equal(p, q), k
        assert w is None or bool((a[5] != 0).any())


# ------------------------------------------------------------------------------------------------ 10. autograd
@pytest.mark.parametrize("name,case", [("complete8", (16, 2, 8, 8)), ("loud_csr", (27, 3, 8, 10)),
                                       ("range12", (8, 8, 4, 4)), ("knn16_4", (34, 2, 8, 8))])
def test_autograd(cuda_device, name, case):
    g, x, gb, z, G, base, w = hc.operands(name, case)
    H = case[1]
    dev = cuda_device
    csr = g.csr(dev)
    E, P = g.num_edges(), case[2] * case[3]
    for ww in (None, w):
        ref = hc.direct_reference(g, x, z, H, G, None, True, w=ww)
        res = {}
        for fmt in (torch.contiguous_format, torch.channels_last):
            xd = x.to(dev).contiguous(memory_format=fmt).requires_grad_(True)
            zd = z.to(dev).requires_grad_(True)
            op = "attn" if ww is None else "wattn"
            before = aggregate.PATH_COUNTS[op + "_fwd_mh_f32"], aggregate.PATH_COUNTS[op + "_bwd_mh_f32"]
            if ww is None:
                out, attn = m.film_attn(xd, zd, csr, logits=True, return_weights=True, heads=H)
            else:
                wd = ww.to(dev).requires_grad_(True)
                out, attn = m.film_wattn(xd, zd, wd, csr, logits=True, return_weights=True, heads=H)
            assert not attn.requires_grad and tuple(attn.shape) == (H, E, P)
            out.backward(G.to(dev))
            assert (aggregate.PATH_COUNTS[op + "_fwd_mh_f32"], aggregate.PATH_COUNTS[op + "_bwd_mh_f32"]) == \
                (before[0] + 1, before[1] + 1)
            assert close(out, ref[0]) and close(attn, ref[1]) and close(xd.grad, ref[3]) and close(zd.grad, ref[4])
            res[fmt] = [out.detach().contiguous(), attn, xd.grad.contiguous(), zd.grad]
            if ww is not None:
                assert close(wd.grad, ref[5]) and wd.grad.shape == ww.shape
                res[fmt].append(wd.grad)
        for a, b in zip(res[torch.contiguous_format], res[torch.channels_last]):
            assert bits_equal(a, b)  # channels_last is copied to NCHW first: the same kernels on the same values
    # an explicit scale serves all heads
    xd, zd = x.to(dev).requires_grad_(True), z.to(dev).requires_grad_(True)
    out = m.film_attn(xd, zd, csr, logits=True, scale=0.2, heads=H)
    out.backward(G.to(dev))
    rs = hc.direct_reference(g, x, z, H, G, None, True, scale=0.2)
    assert close(out, rs[0]) and close(xd.grad, rs[3]) and close(zd.grad, rs[4])


# ------------------------------------------------------------------------------------------------ 11. the model
TAU = 0.5


def _frames(B, n, seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.uniform(-1, 1, (B, n, 3)), rng.standard_normal((B, n, 4))], 2).astype(np.float32)


def _inputs(g, C, H, W, seed=1):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g.num_nodes(), C, H, W, generator=gen)
    return x, torch.randn(x.shape, generator=gen)


@pytest.mark.parametrize("combine", ["cat_compress", "cat", "residual", "initial_mix"])
def test_model_stack_fp32(cuda_device, combine):
    C, H, W, heads = 8, 4, 4, 2
    layers = 1 if combine == "cat" else 2
    dev = cuda_device
    g = m.batch([m.frame_graph(p) for p in _frames(2, 8, seed=3)])
    torch.manual_seed(0)
    net = m.GCNStack(types.SimpleNamespace(feature_dim=C, gcn_mode="film_attn", gcn_layers=layers, gcn_combine=combine,
                                           gcn2_alpha=0.25, gcn_attn_heads=heads)).to(dev)
    x, G = _inputs(g, C, H, W)
    if combine == "cat":
        G = torch.cat((G, G.flip(0)), 1)
    gd = g.to(dev)
    params = {k: v.detach() for k, v in net.named_parameters()}
    xd = x.to(dev).requires_grad_(True)
    keys = ("attn_fwd_mh_f32", "attn_bwd_mh_f32", "attn_fwd_f32", "attn_bwd_f32")
    before = [aggregate.PATH_COUNTS[k] for k in keys]
    out = net(gd, xd)
    out.backward(G.to(dev))
    assert [aggregate.PATH_COUNTS[k] for k in keys] == [before[0] + layers, before[1] + layers, before[2], before[3]]
    r_out, r_dx, r_p = hc.stack_reference(params, g, x, g.edata["pose"], G, layers, combine, 0.25, heads)
    assert close(out, r_out) and close(xd.grad, r_dx)
    for k, p in net.named_parameters():
        assert close(p.grad, r_p[k]), k
    # the heads matter: the single-head model on the same parameters is another function
    one = hc.stack_reference(params, g, x, g.edata["pose"], G, layers, combine, 0.25, 1)[0]
    assert rel_err(out.detach().cpu().numpy(), one.numpy()) > 100 * TOL


def test_model_step_on_a_device_built_range_graph(cuda_device):
    C, H, W, heads = 8, 4, 4, 2
    dev = cuda_device
    poses = torch.from_numpy(_frames(2, 9, seed=5)).to(dev)
    active = torch.ones(2, 9, dtype=torch.bool, device=dev)
    active[0, 3] = False
    g = m.frame_batch(poses, max_range=1.2, active=active)
    assert g.csr(dev).graph_kind == _lib.GRAPH_SIMPLE and int(g.in_degrees()[3]) == 0
    torch.manual_seed(0)
    net = m.multi_view_dgl_model(types.SimpleNamespace(feature_dim=C, gcn_mode="film_wattn", compress_gcn=True,
                                                       multi_gcn=False, gcn_confidence=True,
                                                       gcn_confidence_threshold=TAU, gcn_attn_heads=heads)).to(dev)
    pose = g.edata["pose"].cpu()
    x, G = _inputs(g, C, H, W)
    params = {k: v.detach() for k, v in net.named_parameters()}
    xd = x.to(dev).requires_grad_(True)
    keys = ("wattn_fwd_mh_f32", "wattn_bwd_mh_f32", "wattn_fwd_f32", "wattn_bwd_f32")
    before = [aggregate.PATH_COUNTS[k] for k in keys]
    g.ndata["image"] = xd
    out = net(g)
    out.backward(G.to(dev))
    assert [aggregate.PATH_COUNTS[k] for k in keys] == [before[0] + 1, before[1] + 1, before[2], before[3]]
    gaps = []

    def weights_of(p, i, h):
        cw = p[f"gcn{i}.confidence.weight"]
        wm = torch.sigmoid(torch.einsum("oc,nchw->nohw", cw.reshape(1, -1), h) +
                           p[f"gcn{i}.confidence.bias"][None, :, None, None])[:, 0]
        gaps.append(float((wm.detach() - TAU).abs().min()))
        return torch.where(wm >= TAU, wm, torch.zeros_like(wm))
    r_out, r_dx, r_p = hc.stack_reference(params, g, x, pose, G, 1, "cat_compress", 0.25, heads,
                                          weights_of=weights_of)
    # the gate is a comparison: both evaluations agree on it only where no confidence sits on the threshold
    # (4e-6 is 64 fp32 spacings at 0.5, as in tests/test_gpu_film_wattn.py)
    assert min(gaps) > 4e-6, gaps
    assert close(out, r_out) and close(xd.grad, r_dx)
    for k, p in net.named_parameters():
        assert close(p.grad, r_p[k]), k
    assert any("confidence" in k for k in params)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    old = {k: p.detach().clone() for k, p in net.named_parameters()}
    opt.step()
    assert all(not torch.equal(p.detach(), old[k]) for k, p in net.named_parameters())
