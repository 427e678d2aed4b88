"""The reference and the operands of the max-pooled FiLM aggregation's tests (tests/test_gpu_film_max.py,
tests/test_capi_film_max.py): a small torch restatement of the operator's definition in include/mrp_gnn.h.

For each destination the row's messages are stacked in row order (the project's host CSR: edge-id order,
DGL's mailbox order), reduced by ``torch.max(mb, 0)``, and the gradients come from autograd.  On the CPU
``torch.max`` returns the first maximal entry and the first NaN, which is the operator's tie rule.
"""
import numpy as np
import torch

import mrp_gnn_amd as m


def rows(g):
    """(indptr, src, eid) of the graph's host CSR: row v lists v's in-edges in edge-id order."""
    indptr, src, eid = g.host_csr()[:3]
    return np.asarray(indptr), np.asarray(src), np.asarray(eid)


def reference(g, x, gb, G=None, base=None, logits=False, dtype=torch.float32):
    """out, dx, dgb (dx / dgb None without G) of film_max in ``dtype`` arithmetic on the CPU.

    x (N, C, H, W), gb (E, C, 2) gamma/beta or their logits; messages fl(fl(gamma x) + beta) as two torch ops."""
    indptr, src, eid = rows(g)
    xr = x.detach().to(dtype).clone().requires_grad_(G is not None)
    gr = gb.detach().to(dtype).clone().requires_grad_(G is not None)
    gam = torch.sigmoid(gr) if logits else gr
    outs = []
    for v in range(x.shape[0]):
        lo, hi = int(indptr[v]), int(indptr[v + 1])
        if hi == lo:
            outs.append(torch.zeros(x.shape[1:], dtype=dtype))
            continue
        e = torch.as_tensor(eid[lo:hi].astype(np.int64))
        u = torch.as_tensor(src[lo:hi].astype(np.int64))
        mb = gam[e, :, 0, None, None] * xr[u] + gam[e, :, 1, None, None]  # (deg, C, H, W), row order
        outs.append(torch.max(mb, 0).values)
    out = torch.stack(outs) if outs else torch.zeros(x.shape, dtype=dtype)
    if G is None:
        return out.detach(), None, None
    if out.requires_grad:
        out.backward(G.to(dtype))
    dx = xr.grad if xr.grad is not None else torch.zeros_like(xr)
    dgb = gr.grad if gr.grad is not None else torch.zeros_like(gr)
    if base is not None:
        dx = dx + base.to(dtype)
    return out.detach(), dx.detach(), dgb.detach()


def aggregate(g, x, gam):
    """The max aggregate of x (N, C, H, W) under gamma/beta gam (E, C, 2), differentiable, in x's dtype."""
    indptr, src, eid = rows(g)
    outs = []
    for v in range(x.shape[0]):
        lo, hi = int(indptr[v]), int(indptr[v + 1])
        if hi == lo:
            outs.append(torch.zeros(x.shape[1:], dtype=x.dtype, device=x.device))
            continue
        e = torch.as_tensor(eid[lo:hi].astype(np.int64), device=x.device)
        u = torch.as_tensor(src[lo:hi].astype(np.int64), device=x.device)
        outs.append(torch.max(gam[e, :, 0, None, None] * x[u] + gam[e, :, 1, None, None], 0).values)
    return torch.stack(outs)


def stack_reference(params, g, x, pose, G, layers, combine, alpha, dtype=torch.float64):
    """(out, dx, {param: grad}) of a GCNStack with gcn_mode="film_max", restated in ``dtype`` on the CPU:
    the edge encoder's two Linears, sigmoid, the max aggregate, and the layer's combination."""
    import torch.nn.functional as F
    p = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in params.items()}
    xx = x.detach().cpu().to(dtype).requires_grad_(True)
    pose = pose.detach().cpu().to(dtype)
    h0 = h = xx
    for i in range(1, layers + 1):
        pre = f"gcn{i}.edge_encoder.layers."
        hid = F.relu(F.linear(pose, p[pre + "0.weight"], p[pre + "0.bias"]))
        gam = torch.sigmoid(F.linear(hid, p[pre + "2.weight"], p[pre + "2.bias"])).view(pose.shape[0], -1, 2)
        a = aggregate(g, h, gam)
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


def margins(g, x, gb, logits=False):
    """Per output element of a row with >= 2 entries, in float64: (best - runner-up) / max(|best|, 1).
    0 marks an exact tie.  One flat tensor (empty if no row has two entries)."""
    indptr, src, eid = rows(g)
    xr, gr = x.double(), gb.double()
    gam = torch.sigmoid(gr) if logits else gr
    res = []
    for v in range(x.shape[0]):
        lo, hi = int(indptr[v]), int(indptr[v + 1])
        if hi - lo < 2:
            continue
        e = torch.as_tensor(eid[lo:hi].astype(np.int64))
        u = torch.as_tensor(src[lo:hi].astype(np.int64))
        mb = gam[e, :, 0, None, None] * xr[u] + gam[e, :, 1, None, None]
        top = torch.topk(mb, 2, dim=0).values
        res.append(((top[0] - top[1]) / top[0].abs().clamp_min(1.0)).reshape(-1))
    return torch.cat(res) if res else torch.zeros(0, dtype=torch.float64)


def lattice(shape, lo, hi, gen):
    """Multiples of 2^-3 in [lo, hi]: every message and every gradient sum of the tests is then exact in fp32."""
    return torch.randint(int(lo * 8), int(hi * 8) + 1, shape, generator=gen).float() / 8.0


def lattice_operands(g, C, H, W, seed):
    """x, gb, G, base on the lattice: x, G, base in [-2, 2], gamma / beta in [0, 1]."""
    gen = torch.Generator().manual_seed(seed)
    N, E = g.num_nodes(), g.num_edges()
    x = lattice((N, C, H, W), -2, 2, gen)
    gb = lattice((E, C, 2), 0, 1, gen)
    G = lattice((N, C, H, W), -2, 2, gen)
    base = lattice((N, C, H, W), -2, 2, gen)
    return x, gb, G, base


# ------------------------------------------------------------------------------------------------ graphs
def complete(n, B=2):
    return m.batch([m.complete_graph(n) for _ in range(B)])


def knn(n, k, B=2, seed=0):
    rng = np.random.default_rng(seed)
    gs = []
    for _ in range(B):
        gs.append(m.RobotGraph(*m.knn_edges(rng.standard_normal((n, 3)), k), num_nodes=n))
    return m.batch(gs)


def ragged_simple(seed=0):
    """A masked (MRP_GRAPH_SIMPLE) batch of 3-, 16- and 9-node graphs: complete edge slots, a random half of
    them active; node 1 of the 16-node graph keeps its out-edges but has in-degree 0, node 2 is isolated."""
    rng = np.random.default_rng(seed)
    sizes = [3, 16, 9]
    src, dst, bne = [], [], []
    off = 0
    for n in sizes:
        s, d = m.complete_edges(n)
        src += [int(a) + off for a in s]
        dst += [int(a) + off for a in d]
        bne.append(len(s))
        off += n
    src, dst = np.array(src), np.array(dst)
    active = rng.random(src.shape[0]) < 0.5
    a, b = 3 + 1, 3 + 2
    active[dst == a] = False
    active[src == a] = True
    active[(dst == b) | (src == b)] = False
    g = m.RobotGraph(src, dst, num_nodes=off, batch_num_nodes=sizes, batch_num_edges=bne,
                     edge_active=torch.from_numpy(active))
    return g


def masked_small(seed=1):
    """A masked batch of 6- and 8-node graphs, so kind MRP_GRAPH_SIMPLE, whose rows nevertheless hold
    self-loops and parallel edges (film_max does not need that kind's promise): node 0 of the 8-node graph has
    11 in-entries (7 neighbours, a self-loop, three more copies of 3 -> 0), more than the graph has nodes."""
    rng = np.random.default_rng(seed)
    sizes = [6, 8]
    src, dst, bne = [], [], []
    off = 0
    for n in sizes:
        s, d = m.complete_edges(n)
        s, d = list(s) + list(range(n)), list(d) + list(range(n))  # + self-loops
        if n == 8:
            s, d = s + [3, 3, 3, 5], d + [0, 0, 0, 2]  # parallel edges, each with its own (gamma, beta)
        src += [a + off for a in s]
        dst += [a + off for a in d]
        bne.append(len(s))
        off += n
    src, dst = np.array(src), np.array(dst)
    active = rng.random(src.shape[0]) < 0.7
    active[dst == 6] = True  # node 0 of the 8-node graph keeps all 11 entries
    return m.RobotGraph(src, dst, num_nodes=off, batch_num_nodes=sizes, batch_num_edges=bne,
                        edge_active=torch.from_numpy(active))


def general_csr():
    """A MRP_GRAPH_CSR batch (5 and 7 nodes) with a self-loop, parallel edges 0 -> 1 carrying their own
    (gamma, beta), and a node without in-edges."""
    e0 = [(0, 1), (2, 1), (0, 1), (1, 1), (3, 0), (4, 2), (1, 3), (2, 3), (0, 3)]  # node 4: in-degree 0
    rng = np.random.default_rng(5)
    e1 = [(int(rng.integers(0, 7)) + 5, int(rng.integers(0, 7)) + 5) for _ in range(30)]
    src = [u for u, _ in e0 + e1]
    dst = [v for _, v in e0 + e1]
    return m.RobotGraph(src, dst, num_nodes=12, batch_num_nodes=[5, 7], batch_num_edges=[len(e0), len(e1)])
