"""The reference and the operands of the confidence-weighted FiLM aggregation's tests
(tests/test_film_wmean_cpu.py, tests/test_gpu_film_wmean.py): the operator's definition in include/mrp_gnn.h
restated in torch, forward and the manual backward, with switches that each drop one term (the CPU tests show
that every dropped term moves the result far beyond the bars, so the GPU comparisons have teeth).

For each destination the row's messages are stacked in row order (the project's host CSR: edge-id order):

    m_j = gamma_j x[u_j] + beta_j;  acc = sum_j w[u_j] m_j;  D = sum_j w[u_j];  out = acc / D where D > 0 else 0

Weights are drawn from {0} u [1/16, 1]: uniform in [1/16, 1], about a quarter of the entries an exact 0, and two
pixels at which every node is silent (so every destination has pixels with D = 0).  The lower bound keeps 1/D
moderate, so a float64 comparison tests the kernel rather than cancellation.
"""
import functools

import numpy as np
import torch

import half_cases as hc

DROPS = ("w_on_beta", "out_term", "w_in_dx", "degree_D")
KEYS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def rows(g):
    indptr, src, eid = g.host_csr()[:3]
    return np.asarray(indptr), np.asarray(src), np.asarray(eid)


def weights(name, seed=0):
    """(N, H, W) fp32 sender maps of a half_cases case (see the module docstring)."""
    n, _, H, W = hc.shape(name)
    return weights_of(n, H, W, torch.Generator().manual_seed(sum(map(ord, name)) * 977 + 13 + seed))


def weights_of(n, H, W, gen):
    """(n, H, W) fp32 sender maps drawn from ``gen`` (see the module docstring)."""
    w = 1.0 / 16 + (1.0 - 1.0 / 16) * torch.rand(n, H, W, generator=gen)
    w.view(-1)[torch.randperm(w.numel(), generator=gen)[:w.numel() // 4]] = 0.0  # a quarter: exact zeros
    flat = w.view(n, -1)
    flat[:, 0] = 0.0  # every sender silent: D = 0 for every destination
    flat[:, (H * W) // 2] = 0.0
    return w.contiguous()


@functools.lru_cache(maxsize=None)
def inputs(name, key):
    """(x, gb, z, G, w) on the CPU: x and G in the case's dtype (drawn in fp32, rounded), gb = sigmoid(z) fp32."""
    T = KEYS[key]
    n, C, H, W = hc.shape(name)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 131 + {"f32": 2, "bf16": 0, "f16": 1}[key])
    x = torch.randn(n, C, H, W, generator=gen).to(T)
    G = torch.randn(n, C, H, W, generator=gen).to(T)
    z = torch.randn(hc.graph(name).num_edges(), C, 2, generator=gen)
    return x, torch.sigmoid(z), z, G, weights(name)


def forward(g, x, gb, w, mode="mean", drop=None):
    """The aggregate in the dtype of x (differentiable: plain torch ops).  gb (E, C, 2) gamma/beta."""
    indptr, src, eid = rows(g)
    outs = []
    for v in range(x.shape[0]):
        lo, hi = int(indptr[v]), int(indptr[v + 1])
        if hi == lo:
            outs.append(torch.zeros(x.shape[1:], dtype=x.dtype))
            continue
        e = torch.as_tensor(eid[lo:hi].astype(np.int64))
        u = torch.as_tensor(src[lo:hi].astype(np.int64))
        we = w[u][:, None]  # (deg, 1, H, W)
        if drop == "w_on_beta":
            mb = we * (gb[e, :, 0, None, None] * x[u]) + gb[e, :, 1, None, None]
        else:
            mb = we * (gb[e, :, 0, None, None] * x[u] + gb[e, :, 1, None, None])
        acc = mb.sum(0)
        if mode == "sum":
            outs.append(acc)
            continue
        D = torch.full_like(we[0], float(hi - lo)) if drop == "degree_D" else we.sum(0)
        outs.append(torch.where(D > 0, acc / torch.where(D > 0, D, torch.ones_like(D)), torch.zeros_like(acc)))
    return torch.stack(outs)


def backward(g, x, gb, w, G, mode="mean", drop=None, logits_z=None):
    """(out, dx, dgb, dw) by the header's formulas, in the dtype of x.  With logits_z, dgb is d logits."""
    indptr, src, eid = rows(g)
    out = forward(g, x, gb, w, mode, drop="degree_D" if drop == "degree_D" else None)
    dx, dgb, dw = torch.zeros_like(x), torch.zeros_like(gb), torch.zeros_like(w)
    for v in range(x.shape[0]):
        lo, hi = int(indptr[v]), int(indptr[v + 1])
        if hi == lo:
            continue
        e = torch.as_tensor(eid[lo:hi].astype(np.int64))
        u = torch.as_tensor(src[lo:hi].astype(np.int64))
        we = w[u][:, None]
        gam, bet = gb[e, :, 0, None, None], gb[e, :, 1, None, None]
        msg = gam * x[u] + bet
        if mode == "mean":
            D = torch.full_like(we[0], float(hi - lo)) if drop == "degree_D" else we.sum(0)
            Gh = torch.where(D > 0, G[v] / torch.where(D > 0, D, torch.ones_like(D)), torch.zeros_like(G[v]))
        else:
            Gh = G[v]
        dx.index_add_(0, u, (1.0 if drop == "w_in_dx" else we) * gam * Gh)
        dgb[:, :, 0].index_add_(0, e, (we * x[u] * Gh).sum((2, 3)))
        dgb[:, :, 1].index_add_(0, e, (we * Gh).expand_as(msg).sum((2, 3)))
        inner = msg if (mode == "sum" or drop == "out_term") else msg - out[v]
        dw.index_add_(0, u, (Gh * inner).sum(1))
    if logits_z is not None:
        s = torch.sigmoid(logits_z.to(gb.dtype))
        dgb = dgb * s * (1 - s)
    return out, dx, dgb, dw


def autograd(g, x, gb, w, G, mode="mean"):
    """(out, dx, dgb, dw) through torch.autograd of forward()."""
    xr, gr, wr = (t.detach().clone().requires_grad_(True) for t in (x, gb, w))
    out = forward(g, xr, gr, wr, mode)
    grads = torch.autograd.grad(out, (xr, gr, wr), G, allow_unused=True)
    return (out.detach(),) + tuple(torch.zeros_like(t) if gr_ is None else gr_ for t, gr_ in zip((x, gb, w), grads))


@functools.lru_cache(maxsize=None)
def reference(name, key, mode="mean"):
    """Float64 and float32 restatements on the widened operands: dict of out / dx / dgb / dw / dz for each
    ("64", "32"); dz is the gradient of the logits z with gb = sigmoid(z)."""
    x, gb, z, G, w = inputs(name, key)
    g = hc.graph(name)
    ref = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        args = (x.to(dt), gb.to(dt), w.to(dt), G.to(dt))
        out, dx, dgb, dw = backward(g, *args, mode=mode)
        s = args[1]
        ref.update({"out" + tag: out, "dx" + tag: dx, "dgb" + tag: dgb, "dw" + tag: dw,
                    "dz" + tag: dgb * s * (1 - s)})
    return ref


def stack_reference(params, g, x, pose, G, layers, combine, alpha, mode="mean", dtype=torch.float64):
    """(out, dx, {param: grad}) of a GCNStack with opt.gcn_confidence (no threshold), restated in ``dtype`` on
    the CPU: the edge encoder, the 1x1 confidence head and its sigmoid, the weighted aggregate, the layer's
    combination."""
    import torch.nn.functional as F
    p = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in params.items()}
    xx = x.detach().cpu().to(dtype).requires_grad_(True)
    pose = pose.detach().cpu().to(dtype)
    h0 = h = xx
    for i in range(1, layers + 1):
        pre = f"gcn{i}.edge_encoder.layers."
        hid = F.relu(F.linear(pose, p[pre + "0.weight"], p[pre + "0.bias"]))
        gam = torch.sigmoid(F.linear(hid, p[pre + "2.weight"], p[pre + "2.bias"])).view(pose.shape[0], -1, 2)
        cw = p[f"gcn{i}.confidence.weight"]
        conf = torch.sigmoid(torch.einsum("oc,nchw->nohw", cw.reshape(1, -1), h) + p[f"gcn{i}.confidence.bias"])[:, 0]
        a = forward(g, h, gam, conf, mode)
        if combine == "cat_compress":
            w = p[f"conv{i}.weight"]
            h = torch.einsum("oc,nchw->nohw", w.reshape(w.shape[0], w.shape[1]), torch.cat((h, a), 1)) + \
                p[f"conv{i}.bias"][None, :, None, None]
        elif combine == "cat":
            h = torch.cat((h, a), 1)
        elif combine == "residual":
            h = h + a
        else:
            h = (1.0 - alpha) * a + alpha * h0
    h.backward(G.detach().cpu().to(dtype))
    return h.detach(), xx.grad, {k: v.grad for k, v in p.items()}
