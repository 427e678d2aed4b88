"""The reference, cases and operands of the FP8 receiver-side attention tests (tests/test_gpu_fp8_attn.py,
tests/test_fp8_attn_cpu.py): tests/attn_cases.py's restatement of the operator with the one thing that is new —
the query is a tensor of its own.

    m_j = gamma_j * xh[u_j] + beta_j        xh: the dequantised messages
    s_j = scale * sum_c q[v, c] * m_j[c]    q: the receiver's own features, never quantised
    out = sum_j softmax_j(s_j) * m_j

``reference(..., q=xh)`` is ``attn_cases.reference`` (asserted on the CPU).  Every quantisation is torch's cast on
the CPU; the GPU tests upload the bytes.
"""
import functools

import torch

import mrp_gnn_amd as m
import attn_cases as ac
import heads_cases as hcs
from max_cases import rows

FORMATS = ("e4m3", "e5m2")
QDTYPES = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
NAN_CODE = {"e4m3": 0x7F, "e5m2": 0x7F}  # E4M3: the NaN; E5M2: exponent all ones, mantissa 11: a NaN

# complete n = 5 (KS 4) and n = 8 (KS 8), k-NN(4) n = 16 (KS 4, 16 nodes), a general CSR with parallel edges, a
# self-loop and an empty row (KS 16), a 12-node range-limited frame with an isolated robot (SIMPLE, KS 16)
GRAPHS = {
    "complete5": lambda: ac.complete(5),
    "complete8": lambda: ac.complete(8),
    "knn16_4": lambda: ac.knn(16, 4),
    "general_csr": ac.general_csr,
    "range12": hcs.range12,
}
C = 20  # heads 1, 2: Ch = 10 crosses one 8-channel chunk raggedly
PLANE = (9, 9)  # two 64-pixel tiles, the second ragged
SMALL_PLANE = (5, 5)  # P < 64


def aggregate(g, q, xh, gam, scale=None, attn_out=None):
    """attn_cases.aggregate with the query q (N, C, H, W) apart from the messages' source xh."""
    indptr, src, eid = rows(g)
    scale = ac.default_scale(xh.shape[1]) if scale is None else scale
    outs = []
    for v in range(xh.shape[0]):
        e, u = ac._row(indptr, src, eid, v, xh.device)
        if e.numel() == 0:
            outs.append(torch.zeros(xh.shape[1:], dtype=xh.dtype, device=xh.device))
            continue
        mb = gam[e, :, 0, None, None] * xh[u] + gam[e, :, 1, None, None]
        s = scale * (q[v][None] * mb).sum(1)
        a = torch.softmax(s, 0)
        if attn_out is not None:
            attn_out[e] = a.detach().reshape(e.numel(), -1).to(attn_out.dtype)
        outs.append((a[:, None] * mb).sum(0))
    return torch.stack(outs)


def reference(g, q, xh, gb, logits=False, dtype=torch.float64, scale=None, heads=1):
    """out (N, C, H, W), attn ((E, P), or (heads, E, P)) in ``dtype`` arithmetic on the CPU; head k is the operator
    on channel slice k with scale 1 / sqrt(C / heads) unless given."""
    q, xh, gb = q.detach().to(dtype), xh.detach().to(dtype), gb.detach().to(dtype)
    gam = torch.sigmoid(gb) if logits else gb
    Cc, P = xh.shape[1], xh.shape[2] * xh.shape[3]
    Ch = Cc // heads
    scale = ac.default_scale(Ch) if scale is None else scale
    outs, attns = [], []
    for k in range(heads):
        sl = slice(k * Ch, (k + 1) * Ch)
        attn = torch.zeros(gb.shape[0], P, dtype=dtype)
        outs.append(aggregate(g, q[:, sl], xh[:, sl], gam[:, sl], scale, attn))
        attns.append(attn)
    return torch.cat(outs, 1), (attns[0] if heads == 1 else torch.stack(attns))


@functools.lru_cache(maxsize=None)
def operands(name, fmt, plane=PLANE, channels=C, seed=0):
    """(g, q, xq, s, xh, z, w) on the CPU: the query q drawn independently of the messages, whose codes xq and
    scales s are torch's cast of a second draw and xh their fp32 dequantisation; z the FiLM logits; w a sender
    map with exact zeros.  Cached: treat as read-only."""
    g = GRAPHS[name]()
    gen = torch.Generator().manual_seed(1000 * seed + 7 * len(name) + (fmt == "e5m2"))
    N, E = g.num_nodes(), g.num_edges()
    H, W = plane
    q = torch.randn(N, channels, H, W, generator=gen)
    xm = torch.randn(N, channels, H, W, generator=gen)
    xq, s = m.quantize_features(xm, fmt)
    xh = m.dequantize_features(xq, s)
    z = 1.5 * torch.randn(E, channels, 2, generator=gen)
    w = torch.rand(N, H, W, generator=gen)
    w = torch.where(w < 0.3, torch.zeros_like(w), w)
    return g, q, xq, s, xh, z, w
