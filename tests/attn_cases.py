"""The reference and the operands of the attention-pooled FiLM aggregation's tests (tests/test_gpu_film_attn.py,
tests/test_film_attn_cpu.py): a torch restatement of the operator's definition in include/mrp_gnn.h.

For each destination the row's messages are stacked in row order (the project's host CSR: edge-id order),
scored against the destination's own features over the channels, ``torch.softmax`` over the row weights them,
and the gradients come from autograd.  ``manual_backward`` restates the header's backward formulas, with
switches that drop one path each: the defects the CPU test shows the tolerance can see.
"""
import math

import numpy as np
import torch

from max_cases import (complete, general_csr, knn, lattice_operands, masked_small, ragged_simple,  # noqa: F401
                       rows)


def default_scale(C):
    return 1.0 / math.sqrt(C)


def _row(indptr, src, eid, v, device=None):
    lo, hi = int(indptr[v]), int(indptr[v + 1])
    e = torch.as_tensor(eid[lo:hi].astype(np.int64), device=device)
    u = torch.as_tensor(src[lo:hi].astype(np.int64), device=device)
    return e, u


def aggregate(g, x, gam, scale=None, attn_out=None):
    """The attention aggregate of x (N, C, H, W) under gamma/beta gam (E, C, 2), differentiable, in x's dtype.
    ``attn_out`` (E, H*W), if given, receives the weights by edge id (detached)."""
    indptr, src, eid = rows(g)
    scale = default_scale(x.shape[1]) if scale is None else scale
    outs = []
    for v in range(x.shape[0]):
        e, u = _row(indptr, src, eid, v, x.device)
        if e.numel() == 0:
            outs.append(torch.zeros(x.shape[1:], dtype=x.dtype, device=x.device))
            continue
        mb = gam[e, :, 0, None, None] * x[u] + gam[e, :, 1, None, None]  # (deg, C, H, W), row order
        s = scale * (x[v][None] * mb).sum(1)  # (deg, H, W)
        a = torch.softmax(s, 0)
        if attn_out is not None:
            attn_out[e] = a.detach().reshape(e.numel(), -1).to(attn_out.dtype)
        outs.append((a[:, None] * mb).sum(0))
    return torch.stack(outs)


def reference(g, x, gb, G=None, base=None, logits=False, dtype=torch.float32, scale=None):
    """out, attn, dx, dgb (dx / dgb None without G) of film_attn in ``dtype`` arithmetic on the CPU.

    x (N, C, H, W), gb (E, C, 2) gamma/beta or their logits; attn (E, H*W) by edge id, unnamed rows zero."""
    xr = x.detach().to(dtype).clone().requires_grad_(G is not None)
    gr = gb.detach().to(dtype).clone().requires_grad_(G is not None)
    gam = torch.sigmoid(gr) if logits else gr
    attn = torch.zeros(gb.shape[0], x.shape[2] * x.shape[3], dtype=dtype)
    out = aggregate(g, xr, gam, scale, attn)
    if G is None:
        return out.detach(), attn, None, None
    if out.requires_grad:
        out.backward(G.to(dtype))
    dx = xr.grad if xr.grad is not None else torch.zeros_like(xr)
    dgb = gr.grad if gr.grad is not None else torch.zeros_like(gr)
    if base is not None:
        dx = dx + base.to(dtype)
    return out.detach(), attn, dx.detach(), dgb.detach()


def manual_backward(g, x, gb, G, scale=None, dtype=torch.float64, key_path=True, query_path=True, subtract=True,
                    use_scale=True):
    """dx, dgb by the header's formulas (plain gamma/beta).  The switches drop the key path, the query path, the
    ``sum_k a_k da_k`` term of the softmax backward, or the scale of the two score paths."""
    indptr, src, eid = rows(g)
    x, gb, G = x.to(dtype), gb.to(dtype), G.to(dtype)
    scale = default_scale(x.shape[1]) if scale is None else scale
    bscale = scale if use_scale else 1.0
    dx, dgb = torch.zeros_like(x), torch.zeros_like(gb)
    for v in range(x.shape[0]):
        e, u = _row(indptr, src, eid, v)
        if e.numel() == 0:
            continue
        mb = gb[e, :, 0, None, None] * x[u] + gb[e, :, 1, None, None]
        a = torch.softmax(scale * (x[v][None] * mb).sum(1), 0)  # (d, H, W)
        da = (G[v][None] * mb).sum(1)
        ds = a * (da - ((a * da).sum(0, keepdim=True) if subtract else 0.0))
        dm = a[:, None] * G[v][None]
        if key_path:
            dm = dm + bscale * ds[:, None] * x[v][None]
        if query_path:
            dx[v] += bscale * (ds[:, None] * mb).sum(0)
        dx.index_add_(0, u, gb[e, :, 0, None, None] * dm)
        dgb[e, :, 0] += (x[u] * dm).sum((2, 3))  # edge ids are distinct within a row
        dgb[e, :, 1] += dm.sum((2, 3))
    return dx, dgb


def chunked_reference(g, x, gb, G, scale=None, chunk=32):
    """out, dx, dgb in fp32 with every channel sum formed in ``chunk``-wide pieces: an fp32 evaluation whose
    summation order differs from torch's, standing in for a kernel's."""
    indptr, src, eid = rows(g)
    xr = x.detach().float().clone().requires_grad_(True)
    gr = gb.detach().float().clone().requires_grad_(True)
    scale = default_scale(x.shape[1]) if scale is None else scale
    outs = []
    for v in range(x.shape[0]):
        e, u = _row(indptr, src, eid, v)
        if e.numel() == 0:
            outs.append(torch.zeros(x.shape[1:]))
            continue
        mb = gr[e, :, 0, None, None] * xr[u] + gr[e, :, 1, None, None]
        prod = xr[v][None] * mb
        s = sum(p.sum(1) for p in prod.split(chunk, 1))
        a = torch.softmax(scale * s, 0)
        outs.append((a[:, None] * mb).sum(0))
    out = torch.stack(outs)
    out.backward(G.float())
    return out.detach(), xr.grad, gr.grad


def random_operands(g, C, H, W, seed, signed=True):
    """x, gb (gamma/beta in (0, 1)), z (their logits), G, base: the GPU tests' random operands."""
    gen = torch.Generator().manual_seed(seed)
    N, E = g.num_nodes(), g.num_edges()
    x = torch.randn(N, C, H, W, generator=gen)
    if not signed:
        x = x.relu()
    z = 1.5 * torch.randn(E, C, 2, generator=gen)
    G = torch.randn(N, C, H, W, generator=gen)
    base = torch.randn(N, C, H, W, generator=gen)
    return x, torch.sigmoid(z), z, G, base


def stack_reference(params, g, x, pose, G, layers, combine, alpha, dtype=torch.float64, scale=None):
    """(out, dx, {param: grad}) of a GCNStack with gcn_mode="film_attn", restated in ``dtype`` on the CPU:
    the edge encoder's two Linears, sigmoid, the attention aggregate, and the layer's combination."""
    import torch.nn.functional as F
    p = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in params.items()}
    xx = x.detach().cpu().to(dtype).requires_grad_(True)
    pose = pose.detach().cpu().to(dtype)
    h0 = h = xx
    for i in range(1, layers + 1):
        pre = f"gcn{i}.edge_encoder.layers."
        hid = F.relu(F.linear(pose, p[pre + "0.weight"], p[pre + "0.bias"]))
        gam = torch.sigmoid(F.linear(hid, p[pre + "2.weight"], p[pre + "2.bias"])).view(pose.shape[0], -1, 2)
        a = aggregate(g, h, gam, scale)
        if combine == "cat_compress":
            w = p[f"conv{i}.weight"]
            h = torch.einsum("oc,nchw->nohw", w.reshape(w.shape[0], w.shape[1]), torch.cat((h, a), 1)) + \
                p[f"conv{i}.bias"][None, :, None, None]
        elif combine == "residual":
            h = h + a
        else:
            h = (1.0 - alpha) * a + alpha * h0
    h.backward(G.detach().cpu().to(dtype))
    return h.detach(), xx.grad, {k: v.grad for k, v in p.items()}
