"""The reference and the operands of the confidence-gated attention fusion's tests (tests/test_gpu_film_wattn.py,
tests/test_film_wattn_cpu.py): a torch restatement of the operator's definition in include/mrp_gnn.h.

``reference`` is differentiable in x, gb and w by autograd; ``formulas`` restates the forward and the header's
backward formulas in any dtype with the kernels' selects (a silent entry is skipped, never multiplied), with
switches for three defects the CPU test shows the tolerance can see.

A *loud* node (``random_operands``): a sender that is silent everywhere and has no in-edges, whose features are
so large that its messages' scores overflow fp32.  Nothing of it may reach any output but its own ``rate`` and
``grad_w`` (which the header leaves to IEEE: infinities and NaNs there), so those two are not compared for it;
everything else is, and that is what gives the defects "the max taken over all entries" and "dbar including
silent entries" something to break: in exact arithmetic neither changes a result.
"""
import numpy as np
import torch

import mrp_gnn_amd as m
from attn_cases import default_scale, _row
from max_cases import complete, general_csr, knn, masked_small, ragged_simple, rows  # noqa: F401


def _gate(s, wj, quiet=None):
    """(delivered, u, t, Z > 0, Z or 1) of one row: scores s (d, H, W), weights wj (d, H, W).  ``quiet`` (d,)
    bool: entries of a loud source, whose score is replaced by 0 before the exponential (their u means nothing)."""
    d = wj > 0
    neg = torch.full_like(s, -float("inf"))
    mx = torch.where(d, s, neg).max(0).values.detach()
    mx = torch.where(d.any(0), mx, torch.zeros_like(mx))
    if quiet is not None and bool(quiet.any()):
        s = torch.where(quiet[:, None, None], torch.zeros_like(s), s)
    u = torch.exp(s - mx)
    t = wj.clamp(min=0) * u  # a zero weight is a zero term, and its one-sided derivative is u
    Z = t.sum(0)
    zpos = Z > 0
    return d, u, t, zpos, torch.where(zpos, Z, torch.ones_like(Z))


def aggregate(g, x, gam, w, scale=None, attn_out=None, rate_out=None, loud=()):
    """The gated attention aggregate of x (N, C, H, W) under gamma/beta gam (E, C, 2) and sender maps w
    (N, H, W), differentiable in all three, in x's dtype.  ``attn_out`` / ``rate_out`` (E, H*W), if given,
    receive a and r by edge id (detached)."""
    indptr, src, eid = rows(g)
    scale = default_scale(x.shape[1]) if scale is None else scale
    w = w.reshape(x.shape[0], x.shape[2], x.shape[3])
    loud = torch.as_tensor(sorted(loud), dtype=torch.int64, device=x.device)
    outs = []
    for v in range(x.shape[0]):
        e, u = _row(indptr, src, eid, v, x.device)
        if e.numel() == 0:
            outs.append(torch.zeros(x.shape[1:], dtype=x.dtype, device=x.device))
            continue
        mb = gam[e, :, 0, None, None] * x[u] + gam[e, :, 1, None, None]  # (deg, C, H, W), row order
        s = scale * (x[v][None] * mb).sum(1)
        _, uu, t, zpos, Z = _gate(s, w[u], torch.isin(u, loud))
        a = torch.where(zpos, t / Z, torch.zeros_like(t))
        if attn_out is not None:
            attn_out[e] = a.detach().reshape(e.numel(), -1).to(attn_out.dtype)
        if rate_out is not None:
            r = torch.where(zpos, uu / Z, torch.zeros_like(uu))
            rate_out[e] = r.detach().reshape(e.numel(), -1).to(rate_out.dtype)
        outs.append((a[:, None] * mb).sum(0))
    return torch.stack(outs)


def reference(g, x, gb, w, G=None, base=None, logits=False, dtype=torch.float64, scale=None, loud=()):
    """out, attn, rate, dx, dgb, dw (the gradients None without G) of film_wattn in ``dtype`` on the CPU by
    autograd.  attn, rate (E, H*W) by edge id, unnamed rows zero; rate and dw of a loud node mean nothing."""
    need = G is not None
    xr = x.detach().to(dtype).clone().requires_grad_(need)
    gr = gb.detach().to(dtype).clone().requires_grad_(need)
    wr = w.detach().to(dtype).clone().requires_grad_(need)
    gam = torch.sigmoid(gr) if logits else gr
    P = x.shape[2] * x.shape[3]
    attn, rate = torch.zeros(gb.shape[0], P, dtype=dtype), torch.zeros(gb.shape[0], P, dtype=dtype)
    out = aggregate(g, xr, gam, wr, scale, attn, rate, loud)
    if not need:
        return out.detach(), attn, rate, None, None, None
    if out.requires_grad:
        out.backward(G.to(dtype))
    dx, dgb, dw = (t.grad if t.grad is not None else torch.zeros_like(t) for t in (xr, gr, wr))
    if base is not None:
        dx = dx + base.to(dtype)
    return out.detach(), attn, rate, dx.detach(), dgb.detach(), dw.detach()


def formulas(g, x, gb, w, G, scale=None, dtype=torch.float64, max_over_all=False, zero_silent_dw=False,
             dbar_all=False):
    """out, attn, rate, dx, dgb, dw by the header's formulas in ``dtype`` (plain gamma/beta), silent entries
    skipped by selects as the kernels do.  The switches are the defects: the softmax's max taken over every
    entry of the row; grad_w left 0 at silent entries; dbar summed over every entry (a silent one as 0 * da)."""
    indptr, src, eid = rows(g)
    x, gb, G = x.to(dtype), gb.to(dtype), G.to(dtype)
    N, C, H, W = x.shape
    w = w.to(dtype).reshape(N, H, W)
    scale = default_scale(C) if scale is None else scale
    out = torch.zeros_like(x)
    dx, dgb, dw = torch.zeros_like(x), torch.zeros_like(gb), torch.zeros_like(w)
    attn, rate = torch.zeros(gb.shape[0], H * W, dtype=dtype), torch.zeros(gb.shape[0], H * W, dtype=dtype)
    zero = torch.zeros((), dtype=dtype)
    for v in range(N):
        e, u = _row(indptr, src, eid, v)
        if e.numel() == 0:
            continue
        mb = gb[e, :, 0, None, None] * x[u] + gb[e, :, 1, None, None]
        s = scale * (x[v][None] * mb).sum(1)
        wj = w[u]
        d = wj > 0
        neg = torch.full_like(s, -float("inf"))
        mx = (s if max_over_all else torch.where(d, s, neg)).max(0).values
        uu = torch.exp(s - mx)
        t = torch.where(d, wj * uu, zero)
        Z = t.sum(0)
        zpos = d.any(0) & (Z > 0)
        a = torch.where(d & zpos, t / Z, zero)
        r = torch.where(zpos, uu / Z, zero)
        attn[e], rate[e] = a.reshape(e.numel(), -1), r.reshape(e.numel(), -1)
        out[v] = torch.where(d[:, None], a[:, None] * mb, zero).sum(0)
        da = (G[v][None] * mb).sum(1)
        dbar = (a * da if dbar_all else torch.where(d, a * da, zero)).sum(0)
        ds = torch.where(d, a * (da - dbar), zero)
        dm = torch.where(d[:, None], a[:, None] * G[v][None] + scale * ds[:, None] * x[v][None], zero)
        dx[v] += scale * torch.where(d[:, None], ds[:, None] * mb, zero).sum(0)
        dx.index_add_(0, u, torch.where(d[:, None], gb[e, :, 0, None, None] * dm, zero))
        dgb[e, :, 0] += torch.where(d[:, None], x[u] * dm, zero).sum((2, 3))  # edge ids are distinct within a row
        dgb[e, :, 1] += dm.sum((2, 3))
        gw = r * (da - dbar)
        if zero_silent_dw:
            gw = torch.where(d, gw, zero)
        dw.index_add_(0, u, gw)
    return out, attn, rate, dx, dgb, dw


def manual_backward(g, x, gb, w, G, scale=None, dtype=torch.float64, **defects):
    """dx, dgb, dw by the header's backward formulas (``formulas`` without its forward outputs)."""
    return formulas(g, x, gb, w, G, scale, dtype, **defects)[3:]


def silent_node(g):
    """(node, loud?): the node ``random_operands`` silences everywhere.  A node with out-edges and no in-edges,
    if the graph has one (it can be loud: no row of its own to disturb), else the first node with out-edges."""
    indptr, src, _ = rows(g)
    named = np.unique(src[: int(indptr[-1])])
    for u in named:
        if indptr[u + 1] == indptr[u]:
            return int(u), True
    return (int(named[0]) if named.size else 0), False


def random_operands(g, C, H, W, seed, loud=True):
    """x, gb (gamma/beta in (0, 1)), z (their logits), G, base, w, loud nodes (a tuple, empty if none).

    Nonzero weights are uniform in [0.25, 1]; about 30 % of the entries are exactly 0; one pixel (seed % P) has
    every sender silent; ``silent_node(g)`` is silent everywhere and, if it has no in-edges and ``loud``, its
    features are +-2^127: its messages' scores overflow fp32."""
    gen = torch.Generator().manual_seed(seed)
    N, E = g.num_nodes(), g.num_edges()
    x = torch.randn(N, C, H, W, generator=gen)
    z = 1.5 * torch.randn(E, C, 2, generator=gen)
    G = torch.randn(N, C, H, W, generator=gen)
    base = torch.randn(N, C, H, W, generator=gen)
    w = 0.25 + 0.75 * torch.rand(N, H, W, generator=gen)
    w[torch.rand(N, H, W, generator=gen) < 0.3] = 0.0
    w.view(N, -1)[:, seed % (H * W)] = 0.0
    q, can_be_loud = silent_node(g)
    w[q] = 0.0
    louds = ()
    if loud and can_be_loud:
        x[q] = torch.where(x[q] < 0, -1.0, 1.0) * 2.0 ** 127
        louds = (q,)
    return x, torch.sigmoid(z), z, G, base, w, louds


def drop_loud(g, rate, dw, louds):
    """rate and dw with the loud nodes' own entries (rate rows of their out-edges, their dw planes) zeroed: what
    remains is compared."""
    rate, dw = rate.clone(), dw.clone()
    if louds:
        src, _ = (np.asarray(t) for t in g.edges())
        rate[torch.as_tensor(np.isin(src, list(louds)))] = 0
        dw[list(louds)] = 0
    return rate, dw


def compacted(g, silent):
    """g without the out-edges of the nodes in ``silent`` (bool per node): the same E and edge ids, the rows
    compacted (a masked graph).  g must hold every edge slot (an unmasked graph)."""
    src, dst = (np.asarray(t) for t in g.edges())
    keep = ~np.asarray(silent, bool)[src]
    return m.RobotGraph(src, dst, num_nodes=g.num_nodes(), batch_num_nodes=list(g.batch_num_nodes()),
                        batch_num_edges=list(g.batch_num_edges()), edge_active=torch.from_numpy(keep))


def loud_csr():
    """A MRP_GRAPH_CSR batch of a 6- and a 16-node graph with parallel edges, self-loops, one row of in-degree
    16 (node 6 + 3: every other node of its graph, a self-loop and a second 5 -> 3), a node without in-edges
    that others hear (6 + 0: the loud one) and an isolated node (5)."""
    e0 = [(0, 1), (2, 1), (0, 1), (1, 1), (3, 0), (4, 2), (1, 3), (2, 3), (0, 3), (3, 4), (1, 4)]  # node 5 isolated
    rng = np.random.default_rng(7)
    e1 = [(u, 3) for u in range(16) if u != 3] + [(3, 3)]  # 16 entries into node 3
    for v in (1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15):  # node 0: heard, never addressed
        for u in rng.choice(16, size=int(rng.integers(1, 7)), replace=True):
            e1.append((int(u), v))
    e1 = [(u + 6, v + 6) for u, v in e1]
    src = [u for u, _ in e0 + e1]
    dst = [v for _, v in e0 + e1]
    return m.RobotGraph(src, dst, num_nodes=22, batch_num_nodes=[6, 16], batch_num_edges=[len(e0), len(e1)])


def stack_reference(params, g, x, pose, G, layers, combine, alpha, dtype=torch.float64, scale=None, tau=None,
                    weights=None):
    """(out, dx, {param: grad}, smallest |w - tau| seen) of a GCNStack with gcn_mode="film_wattn" and the
    confidence head (or fixed ``weights``), restated in ``dtype`` on the CPU: the edge encoder's two Linears,
    sigmoid, the head's 1x1 conv, sigmoid and hard gate, the gated attention aggregate, the layer's combination."""
    import torch.nn.functional as F
    p = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in params.items()}
    xx = x.detach().cpu().to(dtype).requires_grad_(True)
    pose = pose.detach().cpu().to(dtype)
    h0 = h = xx
    gap = float("inf")
    for i in range(1, layers + 1):
        pre = f"gcn{i}.edge_encoder.layers."
        hid = F.relu(F.linear(pose, p[pre + "0.weight"], p[pre + "0.bias"]))
        gam = torch.sigmoid(F.linear(hid, p[pre + "2.weight"], p[pre + "2.bias"])).view(pose.shape[0], -1, 2)
        if weights is not None:
            w = weights.detach().cpu().to(dtype)
        else:
            cw = p[f"gcn{i}.confidence.weight"]
            w = torch.sigmoid(torch.einsum("oc,nchw->nohw", cw.reshape(1, -1), h) +
                              p[f"gcn{i}.confidence.bias"][None, :, None, None])[:, 0]
            if tau is not None:
                gap = min(gap, float((w.detach() - tau).abs().min()))
                w = torch.where(w >= tau, w, torch.zeros_like(w))
        a = aggregate(g, h, gam, w, scale)
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
    h.backward(G.detach().cpu().to(dtype))
    return h.detach(), xx.grad, {k: v.grad for k, v in p.items()}, gap
