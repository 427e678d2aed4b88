"""The references, cases and operands of the multi-head attention tests (tests/test_film_attn_heads_cpu.py,
tests/test_gpu_film_attn_heads.py).

Two restatements of ``heads=H``: ``slice_reference`` runs the single-head references of tests/attn_cases.py and
tests/wattn_cases.py on each head's channel slice and assembles the results — the operator's contract, head k is
the single-head operator on slice k — and ``direct_reference`` restates the definition at once in float64 on
tensors reshaped to (N, H, Ch, P), one einsum per head dimension.  They share no code beyond the row lookup.
"""
import functools

import numpy as np
import torch

import mrp_gnn_amd as m
import attn_cases as ac
import wattn_cases as wc

# (C, H, height, width)
CASES = [
    (6, 2, 7, 7),    # Ch = 3, ragged first chunk; P = 49, ragged tile
    (16, 2, 8, 8),   # Ch = 8, exactly one forward chunk
    (27, 3, 8, 10),  # Ch = 9, second chunk ragged; P = 80: two tiles, the second ragged (grad_gb workspace)
    (34, 2, 8, 8),   # Ch = 17, ragged against backward chunks of 4 and 2
    (8, 8, 4, 4),    # Ch = 1; P = 16
    (12, 1, 8, 8),   # H = 1
]
CASE_IDS = [f"C{c}-H{h}-{a}x{b}" for c, h, a, b in CASES]


def range12():
    """A 12-node range-limited / drop-out frame (MRP_GRAPH_SIMPLE): robot 4 dropped out, so isolated."""
    rng = np.random.RandomState(11)
    poses = np.concatenate([rng.uniform(-1, 1, (12, 3)), rng.standard_normal((12, 4))], 1).astype(np.float32)
    active = np.ones(12, bool)
    active[4] = False
    return m.batch([m.frame_graph(poses, max_range=1.1, active=active)])


GRAPHS = {
    "complete8": lambda: ac.complete(8),
    "loud_csr": wc.loud_csr,
    "knn16_4": lambda: ac.knn(16, 4),
    "range12": range12,
}


def head_scale(C, H):
    return ac.default_scale(C // H)


@functools.lru_cache(maxsize=None)
def operands(name, case):
    """(g, x, gb, z, G, base, w) of a (graph, case): wattn_cases' operands without the loud features (w has exact
    zeros, an all-silent pixel and a sender silent everywhere).  Cached: treat as read-only."""
    g = GRAPHS[name]()
    C, H, hh, ww = case
    x, gb, z, G, base, w, _ = wc.random_operands(g, C, hh, ww, seed=3 + C + len(name), loud=False)
    return g, x, gb, z, G, base, w


def _slices(C, H):
    Ch = C // H
    return [slice(k * Ch, (k + 1) * Ch) for k in range(H)]


def slice_reference(g, x, gb, H, G=None, base=None, logits=False, dtype=torch.float64, scale=None, w=None):
    """out, attn (H, E, P), rate (H, E, P) or None, dx, dgb, dw or None of the H-head operators, assembled from the
    single-head references on channel slices; ``w`` given: the gated form.  grad_w is the heads' sum, ascending."""
    C = x.shape[1]
    scale = head_scale(C, H) if scale is None else scale
    outs, attns, rates, dxs, dgbs, dw = [], [], [], [], [], None
    for sl in _slices(C, H):
        Gs = None if G is None else G[:, sl]
        bs = None if base is None else base[:, sl]
        if w is None:
            o, a, dx, dgb = ac.reference(g, x[:, sl], gb[:, sl], Gs, bs, logits, dtype, scale)
        else:
            o, a, r, dx, dgb, dwk = wc.reference(g, x[:, sl], gb[:, sl], w, Gs, bs, logits, dtype, scale)
            rates.append(r)
            if dwk is not None:
                dw = dwk if dw is None else dw + dwk
        outs.append(o)
        attns.append(a)
        dxs.append(dx)
        dgbs.append(dgb)
    cat = (lambda ts: None if ts[0] is None else torch.cat(ts, 1))
    return (torch.cat(outs, 1), torch.stack(attns), torch.stack(rates) if rates else None, cat(dxs), cat(dgbs), dw)


def slice_manual_backward(g, x, gb, H, G, scale=None, dtype=torch.float64, w=None):
    """dx, dgb, dw (None without w) by the header's backward formulas (``manual_backward`` of the single-head case
    modules) on channel slices, plain gamma/beta."""
    C = x.shape[1]
    scale = head_scale(C, H) if scale is None else scale
    dxs, dgbs, dw = [], [], None
    for sl in _slices(C, H):
        if w is None:
            dx, dgb = ac.manual_backward(g, x[:, sl], gb[:, sl], G[:, sl], scale, dtype)
        else:
            dx, dgb, dwk = wc.manual_backward(g, x[:, sl], gb[:, sl], w, G[:, sl], scale, dtype)
            dw = dwk if dw is None else dw + dwk
        dxs.append(dx)
        dgbs.append(dgb)
    return torch.cat(dxs, 1), torch.cat(dgbs, 1), dw


def direct_aggregate(g, x, gam, H, scale=None, w=None, attn_out=None, rate_out=None):
    """The H-head aggregate of x (N, C, h, w) under gamma/beta gam (E, C, 2), differentiable, on (N, H, Ch, P)
    views; ``w`` (N, h, w): the gated form.  attn_out / rate_out (H, E, P) receive the weights / rates."""
    N, C, hh, ww = x.shape
    Ch, P = C // H, hh * ww
    scale = head_scale(C, H) if scale is None else scale
    indptr, src, eid = ac.rows(g)
    xh = x.reshape(N, H, Ch, P)
    gh = gam.reshape(gam.shape[0], H, Ch, 2)
    wp = None if w is None else w.reshape(N, 1, P)
    outs = []
    for v in range(N):
        e, u = ac._row(indptr, src, eid, v)
        if e.numel() == 0:
            outs.append(torch.zeros(H, Ch, P, dtype=x.dtype))
            continue
        mb = gh[e, :, :, 0, None] * xh[u] + gh[e, :, :, 1, None]  # (d, H, Ch, P)
        s = scale * torch.einsum("hcp,dhcp->dhp", xh[v], mb)
        if wp is None:
            a = torch.softmax(s, 0)
        else:
            _, uu, t, zpos, Z = wc._gate(s, wp[u].expand_as(s))
            a = torch.where(zpos, t / Z, torch.zeros_like(t))
            if rate_out is not None:
                rate_out[:, e] = torch.where(zpos, uu / Z, torch.zeros_like(uu)).detach().permute(1, 0, 2)
        if attn_out is not None:
            attn_out[:, e] = a.detach().permute(1, 0, 2)
        outs.append(torch.einsum("dhp,dhcp->hcp", a, mb))
    return torch.stack(outs).reshape(N, C, hh, ww)


def direct_reference(g, x, gb, H, G=None, base=None, logits=False, scale=None, w=None):
    """The same tuple as ``slice_reference`` in float64, by autograd through ``direct_aggregate``."""
    dt = torch.float64
    need = G is not None
    xr = x.detach().to(dt).clone().requires_grad_(need)
    gr = gb.detach().to(dt).clone().requires_grad_(need)
    wr = None if w is None else w.detach().to(dt).clone().requires_grad_(need)
    gam = torch.sigmoid(gr) if logits else gr
    E, P = gb.shape[0], x.shape[2] * x.shape[3]
    attn = torch.zeros(H, E, P, dtype=dt)
    rate = None if w is None else torch.zeros(H, E, P, dtype=dt)
    out = direct_aggregate(g, xr, gam, H, scale, wr, attn, rate)
    if not need:
        return out.detach(), attn, rate, None, None, None
    if out.requires_grad:
        out.backward(G.to(dt))
    grads = [t.grad if t.grad is not None else torch.zeros_like(t) for t in (xr, gr)]
    dw = None if wr is None else (wr.grad if wr.grad is not None else torch.zeros_like(wr))
    dx = grads[0] if base is None else grads[0] + base.to(dt)
    return out.detach(), attn, rate, dx.detach(), grads[1].detach(), dw


def stack_reference(params, g, x, pose, G, layers, combine, alpha, H, scale=None, weights_of=None):
    """(out, dx, {param: grad}) of a GCNStack with ``gcn_attn_heads=H`` in float64: ``attn_cases.stack_reference``
    with the H-head aggregate.  ``weights_of(params, i, h)``, if given, returns layer i's sender maps (N, h, w):
    the gated mode."""
    import torch.nn.functional as F
    dt = torch.float64
    p = {k: v.detach().cpu().to(dt).requires_grad_(True) for k, v in params.items()}
    xx = x.detach().cpu().to(dt).requires_grad_(True)
    pose = pose.detach().cpu().to(dt)
    h0 = h = xx
    for i in range(1, layers + 1):
        pre = f"gcn{i}.edge_encoder.layers."
        hid = F.relu(F.linear(pose, p[pre + "0.weight"], p[pre + "0.bias"]))
        gam = torch.sigmoid(F.linear(hid, p[pre + "2.weight"], p[pre + "2.bias"])).view(pose.shape[0], -1, 2)
        a = direct_aggregate(g, h, gam, H, scale, None if weights_of is None else weights_of(p, i, h))
        if combine == "cat_compress":
            cv = p[f"conv{i}.weight"]
            h = torch.einsum("oc,nchw->nohw", cv.reshape(cv.shape[0], cv.shape[1]), torch.cat((h, a), 1)) + \
                p[f"conv{i}.bias"][None, :, None, None]
        elif combine == "cat":
            h = torch.cat((h, a), 1)
        elif combine == "residual":
            h = h + a
        else:
            h = (1.0 - alpha) * a + alpha * h0
    h.backward(G.detach().cpu().to(dt))
    return h.detach(), xx.grad, {k: v.grad for k, v in p.items()}
