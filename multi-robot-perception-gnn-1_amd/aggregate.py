"""FiLM-mean message passing on the GPU: the replacement for ``g.update_all(edge_udf, node_udf)``.

Reference semantics (``dgl/model/models.py:207-211,223``)::

    m_e   = gamma_e * x[src(e)] + beta_e        # edge_udf, gamma/beta broadcast over H x W
    out_v = mean_{e: dst(e) = v} m_e            # node_udf over v's mailbox; zeros if deg v = 0

``gb`` is the edge encoder's sigmoid output viewed ``(E, C, 2)`` (gamma = ``[..., 0]``,
beta = ``[..., 1]``, ``models.py:154-155``) and is read in place, never split or copied.

Feature maps are taken in either layout: NCHW (a contiguous C*H*W block per node) or pixel-major
``torch.channels_last`` (``pixel_strides``), each with kernels of its own and the same arithmetic; a
channels_last input gives a channels_last output with no conversion (``set_channels_last``).

Everything here dispatches to the HIP library through its C ABI; a CPU tensor raises.
"""
from __future__ import annotations

import collections
import ctypes
import math
from typing import Optional

import torch

from . import _lib
from .graph import GraphCSR


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


#: Feature dtypes the kernels read and write natively -> enum mrp_dtype (include/mrp_gnn.h).  16-bit
#: features are widened exactly on load, the arithmetic is fp32, each output is rounded once at the store.
FEATURE_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}
_DTYPE_KEYS = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}

#: Which kernels ran: ``fwd_f32`` / ``fwd_bf16`` / ``fwd_f16`` and ``bwd_...`` count the launches per
#: feature dtype (like ``encoder.PATH_COUNTS``); tests use them to assert that the 16-bit kernels ran.
PATH_COUNTS = collections.Counter()


def node_stride(t: torch.Tensor) -> Optional[int]:
    """Node stride (in elements) of a (N, C, H, W) fp32 / bf16 / fp16 tensor whose per-node C*H*W block
    is contiguous, else None (then the caller makes it contiguous)."""
    if t.dim() != 4 or t.dtype not in FEATURE_DTYPES:
        return None
    n, c, h, w = t.shape
    if n == 0 or c * h * w == 0:
        return c * h * w
    s = t.stride()
    if (w == 1 or s[3] == 1) and (h == 1 or s[2] == w) and (c == 1 or s[1] == h * w) and (n == 1 or s[0] >= c * h * w):
        return s[0] if n > 1 else c * h * w
    return None


def _as_node_major(t: torch.Tensor):
    s = node_stride(t)
    if s is None:
        t = t.contiguous()
        s = t.shape[1] * t.shape[2] * t.shape[3]
    return t, s


#: How a pixel-major (channels_last) feature map is aggregated: "native" runs the pixel-major kernels
#: (``mrp_film_mean_fwd_cl`` / ``_bwd_cl``) and returns channels_last; "convert" copies it to NCHW first
#: and runs the node-major kernels (the route before the pixel-major kernels existed; for A/B runs).
_CHANNELS_LAST = "native"


def set_channels_last(mode: str) -> str:
    """Select the route of channels_last inputs ("native" or "convert"); returns the previous setting."""
    global _CHANNELS_LAST
    if mode not in ("native", "convert"):
        raise ValueError(f'channels_last route must be "native" or "convert", got {mode!r}')
    prev, _CHANNELS_LAST = _CHANNELS_LAST, mode
    return prev


def pixel_strides(t: torch.Tensor):
    """(node_stride, pixel_stride) in elements of a pixel-major (N, C, H, W) fp32 / bf16 / fp16 tensor —
    every pixel a row of C contiguous channels, the rows of a node ``pixel_stride >= C`` apart in (h, w)
    order: ``torch.channels_last`` tensors (pixel stride C) and channel slices of them, such as either
    half of a channels_last concatenation buffer (pixel stride 2C) — else None.  Node-major wins every
    ambiguous case: a tensor ``node_stride`` accepts, C == 1 or H*W == 1 give None."""
    if t.dim() != 4 or t.dtype not in FEATURE_DTYPES:
        return None
    n, c, h, w = t.shape
    if n == 0 or c <= 1 or h * w <= 1 or node_stride(t) is not None:
        return None
    s = t.stride()
    if s[1] != 1:
        return None
    ps = s[3] if w > 1 else s[2]
    if ps < c or (w > 1 and h > 1 and s[2] != w * ps):
        return None
    if n > 1 and s[0] < h * w * ps:
        return None
    return (s[0] if n > 1 else h * w * ps), ps


def _as_pixel_major(t: torch.Tensor):
    """(tensor, node_stride, pixel_stride), converting (one copy) a tensor that is not pixel-major."""
    s = pixel_strides(t)
    if s is None:
        t = t.contiguous(memory_format=torch.channels_last)
        s = pixel_strides(t)
        if s is None:  # C == 1 or H*W == 1: both layouts at once; the dense strides describe it
            n, c, h, w = t.shape
            s = (c * h * w, c)
    return t, s[0], s[1]


def _native_cl(t: torch.Tensor) -> bool:
    return _CHANNELS_LAST == "native" and pixel_strides(t) is not None


def _empty_like_layout(x: torch.Tensor, shape=None) -> torch.Tensor:
    """An output for x: dense channels_last when x takes the pixel-major kernels, else NCHW-contiguous."""
    shape = tuple(x.shape) if shape is None else shape
    if _native_cl(x):
        return torch.empty(shape, device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
    return torch.empty(shape, device=x.device, dtype=x.dtype)


def _require_device(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "mrp_gnn: the FiLM-mean aggregation runs only on the GPU (HIP, gfx950); got a "
                f"{t.device} tensor. There is no CPU fallback.")


def _stream(dev: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def film_mean_forward_into(x: torch.Tensor, gb: Optional[torch.Tensor], csr: GraphCSR, mode: int,
                           out: torch.Tensor, epilogue: Optional["EpilogueSpec"] = None) -> torch.Tensor:
    """Run the forward kernel into ``out`` (N, C, H, W) — which may be a strided view such as
    the second half of a ``torch.cat((h, g_h), 1)`` buffer.  No autograd."""
    return _forward(x, gb, csr, mode, out, epilogue=epilogue)


def film_mean_cat_forward_into(x: torch.Tensor, gb: Optional[torch.Tensor], csr: GraphCSR, mode: int,
                               cat: torch.Tensor) -> torch.Tensor:
    """``cat[:, :C] = x; cat[:, C:] = film_mean(x)`` for a (N, 2C, H, W) buffer, one kernel pass
    (``mrp_film_mean_cat_fwd``).  No autograd."""
    C = x.shape[1]
    if cat.dim() != 4 or tuple(cat.shape) != (x.shape[0], 2 * C) + tuple(x.shape[2:]):
        raise ValueError(f"cat must be {(x.shape[0], 2 * C) + tuple(x.shape[2:])} in x's dtype")
    return _forward(x, gb, csr, mode, cat[:, C:], epilogue=EpilogueSpec(xcopy=cat[:, :C]))


class EpilogueSpec:
    """What the forward writes per destination v (``mrp_agg_epilogue``, include/mrp_gnn.h):
    ``out[v] = agg_scale * a + self_scale * x[v] + x0_scale * x0[v]``, optionally also ``xcopy[v] = x[v]``.

    * residual ``h = g_h + h`` (``dgl/model/dgl_models.py:36-37``): ``self_scale=1``;
    * initial-feature mix ``(1 - alpha) a + alpha x0`` (GCN2-style; not in the reference):
      ``agg_scale=1-alpha, x0=h0, x0_scale=alpha``;
    * ``torch.cat((x, a), 1)`` (``dgl/model/models.py:182``): ``xcopy`` = the first half."""

    def __init__(self, agg_scale: float = 1.0, self_scale: float = 0.0, x0: Optional[torch.Tensor] = None,
                 x0_scale: float = 0.0, xcopy: Optional[torch.Tensor] = None):
        self.agg_scale = float(agg_scale)
        self.self_scale = float(self_scale)
        self.x0 = x0
        self.x0_scale = float(x0_scale)
        self.xcopy = xcopy

    def is_plain(self) -> bool:
        return self.agg_scale == 1.0 and self.self_scale == 0.0 and self.x0 is None and self.xcopy is None


def _epilogue_struct(ep: Optional[EpilogueSpec], shape, dtype=torch.float32):
    """(ctypes Epilogue or None, tensors to keep alive); x0 is cast to the features' ``dtype``."""
    if ep is None or ep.is_plain():
        return None, ()
    keep = []
    x0p, x0s, xcp, xcs = 0, 0, 0, 0
    if ep.x0 is not None:
        if tuple(ep.x0.shape) != tuple(shape):
            raise ValueError(f"x0 must have the node features' shape {tuple(shape)}")
        _require_device(ep.x0)
        x0, x0s = _as_node_major(ep.x0.to(dtype) if ep.x0.dtype != dtype else ep.x0)
        keep.append(x0)
        x0p = x0.data_ptr()
    if ep.xcopy is not None:
        xcs = node_stride(ep.xcopy)
        if xcs is None or tuple(ep.xcopy.shape) != tuple(shape) or ep.xcopy.dtype != dtype:
            raise ValueError("xcopy must be (N, C, H, W) in x's dtype with a contiguous block per node")
        _require_device(ep.xcopy)
        xcp = ep.xcopy.data_ptr()
    st = _lib.Epilogue(ep.agg_scale, ep.self_scale, x0p, x0s, ep.x0_scale, xcp, xcs)
    return st, keep


def _gb_fp32(gb, csr, C, mode):
    if (mode & ~_lib.GB_LOGITS) == _lib.MODE_COPY_MEAN:
        return None
    if gb is None:
        raise ValueError("gamma/beta tensor required for FiLM modes")
    gb = gb.reshape(csr.num_edges, C, 2)
    if not gb.is_contiguous() or gb.dtype != torch.float32:
        gb = gb.contiguous().float()
    _require_device(gb)
    return gb


def _graph_args(gb, csr, C, P, mode):
    return (_ptr(gb), _ptr(csr.indptr), _ptr(csr.src), _ptr(csr.eid), _ptr(csr.graph_off),
            csr.num_graphs, csr.max_nodes, csr.graph_kind, csr.num_nodes, csr.num_edges, C, P, mode)


def _forward_cl(x, gb, csr, mode, out, epilogue=None):
    """The forward on pixel-major tensors (``mrp_film_mean_fwd_cl``); ``out`` is pixel-major, x (and the
    epilogue's x0) are converted to that layout if they are not."""
    n, C, H, W = x.shape
    if tuple(out.shape) != (n, C, H, W) or out.dtype != x.dtype:
        raise ValueError(f"out must be {(n, C, H, W)} {x.dtype}")
    if n != csr.num_nodes:
        raise ValueError(f"x has {n} nodes, graph has {csr.num_nodes}")
    x, xs, xp = _as_pixel_major(x)
    os_, op = pixel_strides(out)
    gb = _gb_fp32(gb, csr, C, mode)
    ep, keep = None, []
    if epilogue is not None and not epilogue.is_plain():
        x0p = x0s = x0ps = xcp = xcs = xcps = 0
        if epilogue.x0 is not None:
            if tuple(epilogue.x0.shape) != (n, C, H, W):
                raise ValueError(f"x0 must have the node features' shape {(n, C, H, W)}")
            _require_device(epilogue.x0)
            x0, x0s, x0ps = _as_pixel_major(epilogue.x0.to(x.dtype) if epilogue.x0.dtype != x.dtype else epilogue.x0)
            keep.append(x0)
            x0p = x0.data_ptr()
        if epilogue.xcopy is not None:
            xc = epilogue.xcopy
            st = pixel_strides(xc)
            if st is None or tuple(xc.shape) != (n, C, H, W) or xc.dtype != x.dtype:
                raise ValueError("xcopy must be a pixel-major (N, C, H, W) tensor in x's dtype")
            _require_device(xc)
            xcp, (xcs, xcps) = xc.data_ptr(), st
        ep = _lib.EpilogueCl(epilogue.agg_scale, epilogue.self_scale, x0p, x0s, epilogue.x0_scale, xcp, xcs,
                             x0ps, xcps)
    lib = _lib.load_library()
    with torch.cuda.device(x.device):
        code = lib.mrp_film_mean_fwd_cl(FEATURE_DTYPES[x.dtype], _ptr(x), xs, xp, *_graph_args(gb, csr, C, H * W, mode),
                                        _ptr(out), os_, op, ctypes.byref(ep) if ep is not None else None,
                                        _stream(x.device))
    _lib.check(code, "mrp_film_mean_fwd_cl")
    PATH_COUNTS["fwd_cl_" + _DTYPE_KEYS[x.dtype]] += 1
    return out


def _forward(x, gb, csr, mode, out, epilogue=None):
    _require_device(x, out)
    if _native_cl(out):  # x follows out's layout family
        return _forward_cl(x, gb, csr, mode, out, epilogue)
    n, C, H, W = x.shape
    x, xs = _as_node_major(x)
    os_ = node_stride(out)
    if os_ is None or tuple(out.shape) != (n, C, H, W) or out.dtype != x.dtype:
        raise ValueError(f"out must be {(n, C, H, W)} {x.dtype} with a contiguous block per node")
    if (mode & ~_lib.GB_LOGITS) != _lib.MODE_COPY_MEAN:
        if gb is None:
            raise ValueError("gamma/beta tensor required for FiLM modes")
        gb = gb.reshape(csr.num_edges, C, 2)
        if not gb.is_contiguous() or gb.dtype != torch.float32:
            gb = gb.contiguous().float()
        _require_device(gb)
    else:
        gb = None
    if n != csr.num_nodes:
        raise ValueError(f"x has {n} nodes, graph has {csr.num_nodes}")
    ep, _keep = _epilogue_struct(epilogue, x.shape, x.dtype)
    lib = _lib.load_library()
    graph = (_ptr(gb), _ptr(csr.indptr), _ptr(csr.src), _ptr(csr.eid), _ptr(csr.graph_off),
             csr.num_graphs, csr.max_nodes, csr.graph_kind, csr.num_nodes, csr.num_edges, C, H * W, mode)
    tail = (_ptr(out), os_, ctypes.byref(ep) if ep is not None else None, _stream(x.device))
    with torch.cuda.device(x.device):
        if x.dtype == torch.float32:  # the fp32 entry point, as before the typed ones existed
            what = "mrp_film_mean_fwd_ex"
            code = lib.mrp_film_mean_fwd_ex(_ptr(x), xs, *graph, *tail)
        else:
            what = "mrp_film_mean_fwd_t"
            code = lib.mrp_film_mean_fwd_t(FEATURE_DTYPES[x.dtype], _ptr(x), xs, *graph, *tail)
    _lib.check(code, what)
    PATH_COUNTS["fwd_" + _DTYPE_KEYS[x.dtype]] += 1
    return out


def _alloc_grad_gb(csr: GraphCSR, C: int, device) -> torch.Tensor:
    """grad_gb (E, C, 2).  The kernels write every row an edge id names; a masked graph's arrays leave rows
    unnamed, which kind GRAPH_SIMPLE has the library clear and the GRAPH_CSR route has cleared here."""
    sparse = getattr(csr, "sparse_eid", False) and csr.graph_kind != _lib.GRAPH_SIMPLE
    return (torch.zeros if sparse else torch.empty)((csr.num_edges, C, 2), device=device, dtype=torch.float32)


def film_mean_backward(grad_out: torch.Tensor, x: torch.Tensor, gb: Optional[torch.Tensor], csr: GraphCSR,
                       mode: int, need_dx: bool, need_dgb: bool, grad_x_base: Optional[torch.Tensor] = None,
                       epilogue: Optional[EpilogueSpec] = None, pixel_major: bool = True):
    """(grad_x or None, grad_gb (E, C, 2) or None) for the forward above; ``grad_x_base`` (N, C, H, W),
    if given, is added into grad_x by the kernel.  ``epilogue``: the forward's (its agg_scale and
    self_scale enter here; the gradient of x0 is x0_scale * grad_out, formed by the caller).
    A pixel-major (channels_last) x takes the pixel-major kernels and gives a channels_last grad_x,
    unless ``pixel_major=False`` (a caller whose forward ran the NCHW kernels on a converted x)."""
    _require_device(grad_out, x)
    if pixel_major and _native_cl(x):
        return _backward_cl(grad_out, x, gb, csr, mode, need_dx, need_dgb, grad_x_base, epilogue)
    n, C, H, W = x.shape
    dtype = x.dtype  # the feature dtype: grad_out and the base are cast to it, grad_x is allocated in it
    if grad_out.dtype != dtype:
        grad_out = grad_out.to(dtype)
    grad_out, gs = _as_node_major(grad_out)
    bs = 0
    if grad_x_base is not None:
        if grad_x_base.dtype != dtype:
            grad_x_base = grad_x_base.to(dtype)
        grad_x_base, bs = _as_node_major(grad_x_base)
    dx = torch.empty((n, C, H, W), device=x.device, dtype=dtype) if need_dx else None
    dgb = _alloc_grad_gb(csr, C, x.device) if need_dgb else None
    xs = 0
    if need_dgb and (mode & ~_lib.GB_LOGITS) != _lib.MODE_COPY_MEAN:
        x, xs = _as_node_major(x)
    if gb is not None:
        # the kernel reads fp32 (gamma, beta) pairs: the same conversion as the forward
        gb = gb.reshape(csr.num_edges, C, 2)
        if not gb.is_contiguous() or gb.dtype != torch.float32:
            gb = gb.contiguous().float()
    ep = None
    if epilogue is not None and (epilogue.agg_scale != 1.0 or epilogue.self_scale != 0.0):
        ep = _lib.Epilogue(epilogue.agg_scale, epilogue.self_scale, 0, 0, 0.0, 0, 0)
    lib = _lib.load_library()
    ws = None
    if need_dgb:  # scratch for the plane-split k-NN backward (the library never allocates)
        nbytes = int(lib.mrp_film_mean_bwd_workspace(csr.num_graphs, csr.max_nodes, csr.graph_kind, C, H * W))
        if nbytes > 0:
            ws = torch.empty(nbytes // 4 + 1, device=x.device, dtype=torch.float32)
    args = (_ptr(grad_out), gs, _ptr(x), xs, _ptr(gb), _ptr(csr.indptr), _ptr(csr.src), _ptr(csr.eid),
            _ptr(csr.graph_off), csr.num_graphs, csr.max_nodes, csr.graph_kind, csr.num_nodes, csr.num_edges, C,
            H * W, mode,
            _ptr(dx), (C * H * W) if dx is not None else 0, _ptr(grad_x_base), bs, _ptr(dgb),
            ctypes.byref(ep) if ep is not None else None)
    with torch.cuda.device(x.device):
        if dtype == torch.float32:  # the fp32 entry point, as before the typed ones existed
            what = "mrp_film_mean_bwd_ex"
            code = lib.mrp_film_mean_bwd_ex(*args, _ptr(ws), ws.numel() * 4 if ws is not None else 0,
                                            _stream(x.device))
        else:
            what = "mrp_film_mean_bwd_t"
            code = lib.mrp_film_mean_bwd_t(FEATURE_DTYPES[dtype], *args, _stream(x.device))
    _lib.check(code, what)
    PATH_COUNTS["bwd_" + _DTYPE_KEYS[dtype]] += 1
    return dx, dgb


def _backward_cl(grad_out, x, gb, csr, mode, need_dx, need_dgb, grad_x_base, epilogue):
    """``film_mean_backward`` for a pixel-major x (``mrp_film_mean_bwd_cl``): grad_out and the base are
    cast to x's dtype and converted (once) to its layout if they arrive otherwise; grad_x is dense
    channels_last."""
    n, C, H, W = x.shape
    dtype = x.dtype
    if grad_out.dtype != dtype:
        grad_out = grad_out.to(dtype)
    grad_out, gs, gp = _as_pixel_major(grad_out)
    base, bs, bp = None, 0, 0
    if grad_x_base is not None and need_dx:
        if grad_x_base.dtype != dtype:
            grad_x_base = grad_x_base.to(dtype)
        base, bs, bp = _as_pixel_major(grad_x_base)
    dx = torch.empty((n, C, H, W), device=x.device, dtype=dtype, memory_format=torch.channels_last) if need_dx else None
    dgb = _alloc_grad_gb(csr, C, x.device) if need_dgb else None
    xs, xp = pixel_strides(x)
    dxs, dxp = pixel_strides(dx) if dx is not None else (0, 0)
    if gb is not None:
        gb = gb.reshape(csr.num_edges, C, 2)
        if not gb.is_contiguous() or gb.dtype != torch.float32:
            gb = gb.contiguous().float()
    ep = None
    if epilogue is not None and (epilogue.agg_scale != 1.0 or epilogue.self_scale != 0.0):
        ep = _lib.EpilogueCl(epilogue.agg_scale, epilogue.self_scale, 0, 0, 0.0, 0, 0, 0, 0)
    lib = _lib.load_library()
    ws, nbytes = None, 0
    if need_dgb:  # partial Gram sums of a split plane (the library never allocates)
        nbytes = int(lib.mrp_film_mean_bwd_cl_workspace(csr.num_graphs, csr.max_nodes, csr.graph_kind, C, H * W,
                                                        mode, 1))
        if nbytes > 0:
            ws = torch.empty((nbytes + 3) // 4, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        code = lib.mrp_film_mean_bwd_cl(FEATURE_DTYPES[dtype], _ptr(grad_out), gs, gp, _ptr(x), xs, xp,
                                        *_graph_args(gb, csr, C, H * W, mode), _ptr(dx), dxs, dxp,
                                        _ptr(base), bs, bp, _ptr(dgb), ctypes.byref(ep) if ep is not None else None,
                                        _ptr(ws), nbytes, _stream(x.device))
    _lib.check(code, "mrp_film_mean_bwd_cl")
    PATH_COUNTS["bwd_cl_" + _DTYPE_KEYS[dtype]] += 1
    return dx, dgb


class FilmMeanFunction(torch.autograd.Function):
    """Autograd wrapper: forward = ``mrp_film_mean_fwd_ex``, backward = ``mrp_film_mean_bwd_ex``.
    ``mode`` may carry ``_lib.GB_LOGITS`` (gb = pre-sigmoid logits; the gradient is then d logits).
    ``scales`` = (agg_scale, self_scale, x0_scale) of the epilogue (``EpilogueSpec``); x0 may be None."""

    @staticmethod
    def forward(ctx, x, gb, x0, csr: GraphCSR, mode: int, scales=(1.0, 0.0, 0.0)):
        out = _empty_like_layout(x)  # channels_last for a channels_last x
        ep = EpilogueSpec(scales[0], scales[1], x0, scales[2])
        film_mean_forward_into(x, gb, csr, mode, out, epilogue=ep)
        ctx.save_for_backward(x, gb)
        ctx.csr = csr
        ctx.mode = mode
        ctx.scales = scales
        ctx.x0_dtype = x0.dtype if x0 is not None else None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, gb = ctx.saved_tensors
        need_dx = ctx.needs_input_grad[0]
        need_dgb = gb is not None and ctx.needs_input_grad[1]
        ep = EpilogueSpec(ctx.scales[0], ctx.scales[1])
        dx, dgb = film_mean_backward(grad_out, x, gb, ctx.csr, ctx.mode, need_dx, need_dgb, epilogue=ep)
        if dgb is not None:
            dgb = dgb.view(gb.shape).to(gb.dtype)
        dx0 = None
        if ctx.needs_input_grad[2]:
            dx0 = (grad_out * ctx.scales[2]).to(ctx.x0_dtype)
        return dx, dgb, dx0, None, None, None


def _mode_flags(mode, logits: bool) -> int:
    m = _lib.MODES[mode] if isinstance(mode, str) else int(mode)
    if m != _lib.MODE_COPY_MEAN and logits:
        m |= _lib.GB_LOGITS
    return m


def launch_plan(direction: str, graph, C: int, P: int, dtype=torch.float32, mode="film_mean", logits: bool = False,
                align: int = 16, grad_x_base: bool = False, need_dx: bool = True, need_dgb: bool = True,
                x0: bool = False, xcopy: bool = False, stride: Optional[int] = None,
                strides: Optional[dict] = None) -> _lib.AggPlan:
    """The launch plan (``mrp_film_mean_fwd_plan`` / ``_bwd_plan``: kernel, slice width, lanes per plane,
    channels per workgroup, LDS ...) of the ``"fwd"`` or ``"bwd"`` aggregation under the current tuning
    knobs, for dense (N, C, H*W = P) tensors whose storage is aligned to ``align`` bytes.  ``graph`` is
    anything with ``num_graphs``, ``max_nodes``, ``graph_kind``, ``num_nodes`` and ``num_edges`` (a
    ``GraphCSR``).  Host-only: no tensor is needed and no GPU call is made — the library looks at pointers
    for their alignment alone, so made-up ones stand in.  x0 / xcopy: the forward epilogue's extra tensors.
    ``stride``: every tensor's node stride in elements (default dense, C * P); ``strides``: the backward's
    operands that have another one, by name (``"grad_out"``, ``"x"``, ``"grad_x"``, ``"base"``)."""
    base = 1 << 20
    p = ctypes.c_void_p(base if align % 16 == 0 else base + align)
    null = ctypes.c_void_p(0)
    ns = C * P if stride is None else stride
    strides = dict(strides or {})
    if direction != "bwd" and strides:
        raise ValueError("per-operand strides are the backward's")
    gs, xs, gxs, bs = (strides.pop(k, ns) for k in ("grad_out", "x", "grad_x", "base"))
    if strides:
        raise ValueError(f"unknown operands {sorted(strides)}")
    m = _mode_flags(mode, logits)
    copy = (m & ~_lib.GB_LOGITS) == _lib.MODE_COPY_MEAN
    args = (null if copy else p, p, p, p, p, graph.num_graphs, graph.max_nodes, graph.graph_kind, graph.num_nodes,
            graph.num_edges, C, P, m)
    plan = _lib.AggPlan()
    lib = _lib.load_library()
    if direction == "fwd":
        ep = None
        if x0 or xcopy:
            ep = _lib.Epilogue(1.0, 0.0, p.value if x0 else 0, ns, 0.5 if x0 else 0.0, p.value if xcopy else 0, ns)
        code = lib.mrp_film_mean_fwd_plan(FEATURE_DTYPES[dtype], p, ns, *args, p, ns,
                                          ctypes.byref(ep) if ep is not None else None, ctypes.byref(plan))
        _lib.check(code, "mrp_film_mean_fwd_plan")
    elif direction == "bwd":
        code = lib.mrp_film_mean_bwd_plan(FEATURE_DTYPES[dtype], p, gs, p, xs, *args, p if need_dx else null, gxs,
                                          p if (grad_x_base and need_dx) else null, bs, p if need_dgb else null,
                                          None, ctypes.byref(plan))
        _lib.check(code, "mrp_film_mean_bwd_plan")
    else:
        raise ValueError(f"direction must be 'fwd' or 'bwd', got {direction!r}")
    return plan


def _check_x(x):
    if x.dim() != 4:
        raise ValueError(f"node features must be (N, C, H, W), got {tuple(x.shape)}")
    if x.dtype not in FEATURE_DTYPES:
        raise TypeError(f"node features must be float32 (the reference path), bfloat16 or float16, got {x.dtype}")
    _require_device(x)


def film_mean(x: torch.Tensor, gb: Optional[torch.Tensor], csr: GraphCSR, mode="film_mean",
              logits: bool = False) -> torch.Tensor:
    """``mean_e(gamma_e * x_src + beta_e)`` per destination node (see module docstring).

    x: (N, C, H, W) fp32, bf16 or fp16 on a ROCm device (the output has x's dtype; 16-bit features are
    widened exactly, aggregated in fp32 and rounded once at the store); gb: (E, 2C) or (E, C, 2) interleaved gamma/beta
    (ignored for ``mode='copy_mean'``), or their pre-sigmoid logits with ``logits=True`` (the
    encoder's Sigmoid then runs inside the kernel); csr: ``RobotGraph.csr(device)``.
    """
    _check_x(x)
    m = _mode_flags(mode, logits)
    if (m & ~_lib.GB_LOGITS) == _lib.MODE_COPY_MEAN:
        gb = None
    return FilmMeanFunction.apply(x, gb, None, csr, m)


def film_mean_residual(x: torch.Tensor, gb: Optional[torch.Tensor], csr: GraphCSR, mode="film_mean",
                       logits: bool = False) -> torch.Tensor:
    """``x + film_mean(x, ...)`` in one pass — the residual combination ``h = g_h + h`` of
    ``dgl/model/dgl_models.py:36-37`` (x[v] is already in registers: no extra traffic)."""
    _check_x(x)
    m = _mode_flags(mode, logits)
    if (m & ~_lib.GB_LOGITS) == _lib.MODE_COPY_MEAN:
        gb = None
    return FilmMeanFunction.apply(x, gb, None, csr, m, (1.0, 1.0, 0.0))


def film_mean_mix(x: torch.Tensor, gb: Optional[torch.Tensor], csr: GraphCSR, x0: torch.Tensor, alpha: float,
                  mode="film_mean", logits: bool = False) -> torch.Tensor:
    """``(1 - alpha) * film_mean(x, ...) + alpha * x0`` in one pass: the initial-feature mix of a
    GCN2-style layer (BASELINE configs[3]'s "GCN2Conv"; not in the reference, parity unpinned)."""
    _check_x(x)
    m = _mode_flags(mode, logits)
    if (m & ~_lib.GB_LOGITS) == _lib.MODE_COPY_MEAN:
        gb = None
    return FilmMeanFunction.apply(x, gb, x0, csr, m, (1.0 - float(alpha), 0.0, float(alpha)))


class FilmMeanCatFunction(torch.autograd.Function):
    """``torch.cat((x, film_mean(x, gb)), 1)`` without the concatenation pass for the aggregate
    (``dgl/model/models.py:181-182,187-188``): the kernel writes the aggregate into the second half of
    the (N, 2C, H, W) buffer and x, whose slices it holds anyway, into the first; backward hands the
    kernel the second half of the incoming gradient as grad_out and the first half as the base of
    x's gradient."""

    @staticmethod
    def forward(ctx, x, gb, csr: GraphCSR, mode: int):
        n, C, H, W = x.shape
        buf = _empty_like_layout(x, (n, 2 * C, H, W))  # channels_last x: halves with pixel stride 2C
        film_mean_cat_forward_into(x, gb, csr, mode, buf)  # the kernel also writes x into buf[:, :C]
        ctx.save_for_backward(x, gb)
        ctx.csr = csr
        ctx.mode = mode
        return buf

    @staticmethod
    def backward(ctx, grad_buf):
        x, gb = ctx.saved_tensors
        C = x.shape[1]
        need_dx = ctx.needs_input_grad[0]
        need_dgb = gb is not None and ctx.needs_input_grad[1]
        dx, dgb = film_mean_backward(grad_buf[:, C:], x, gb, ctx.csr, ctx.mode, need_dx, need_dgb,
                                     grad_x_base=grad_buf[:, :C] if need_dx else None)
        if dgb is not None:
            dgb = dgb.view(gb.shape).to(gb.dtype)
        return dx, dgb, None, None


def film_mean_cat(x: torch.Tensor, gb: Optional[torch.Tensor], csr: GraphCSR, mode="film_mean",
                  logits: bool = False) -> torch.Tensor:
    """``torch.cat((x, film_mean(x, gb, csr, mode, logits)), dim=1)`` in one kernel pass."""
    if x.dim() != 4 or x.dtype not in FEATURE_DTYPES:
        raise ValueError("node features must be (N, C, H, W) float32, bfloat16 or float16")
    _require_device(x)
    m = _mode_flags(mode, logits)
    if (m & ~_lib.GB_LOGITS) == _lib.MODE_COPY_MEAN:
        gb = None
    return FilmMeanCatFunction.apply(x, gb, csr, m)


# ---------------------------------------------------------------------------------------------------------
# FP8 messages (``mrp_film_mean_fwd_q``): feature maps that crossed the radio link quantised to 8 bits are
# aggregated as they arrive.  The kernel decodes every code exactly and multiplies it once by its
# per-(source node, channel) scale, x^ = fl32(s * decode(q)); from there on it is the fp32 kernel, operation
# for operation, with one rounding at the store:
#
#     film_mean_q(xq, s, ..., out_dtype=T) == film_mean(dequantize_features(xq, s), ...).to(T)    bit for bit
#
# for every graph kind, mode, ``logits``, epilogue and T.  ``film_mean_q`` is an inference op;
# ``film_mean_fq`` is the differentiable fake-quant route on the existing fp32 kernels, with the same forward
# bits.  OCP FP8 only (``torch.float8_e4m3fn`` / ``torch.float8_e5m2``), never the FNUZ encodings.  Not
# provided: pixel-major FP8 kernels (a channels_last FP8 tensor is made NCHW-contiguous first), FP8 for
# film_wmean, FP8 outputs (quantising is left to torch: ``quantize_features``), FP8 backward.  The max and
# attention reducers on FP8 messages: ``film_max_q`` / ``film_attn_q`` / ``film_wattn_q`` at the end of this file.
# ---------------------------------------------------------------------------------------------------------
#: fmt -> (torch dtype, largest finite value, enum mrp_qdtype)
QUANT_FORMATS = {"e4m3": (torch.float8_e4m3fn, 448.0, _lib.QDTYPE_E4M3),
                 "e5m2": (torch.float8_e5m2, 57344.0, _lib.QDTYPE_E5M2)}
_QDTYPES = {dt: (name, code) for name, (dt, _fmax, code) in QUANT_FORMATS.items()}


def quantize_features(x: torch.Tensor, fmt: str = "e4m3", per: str = "channel"):
    """``(xq, scale)``: x (N, C, H, W) as FP8 codes with one fp32 scale per (node, channel) — what a robot
    would transmit.  torch ops only (CPU or GPU), no autograd.

    ``a = amax |x|`` over (H, W) (``per="channel"``) or over (C, H, W) (``per="node"``) in fp32;
    ``s = a / FMAX`` where ``a > 0``, else 1 (FMAX = 448 for ``"e4m3"``, 57344 for ``"e5m2"``);
    ``xq = (x.float() / s).clamp(-FMAX, FMAX).to(float8)``, NCHW-contiguous.  ``scale`` is always a
    contiguous fp32 (N, C) (``per="node"``: the node's scale repeated).  Non-finite features are outside
    the contract (an infinite amax gives an infinite scale and NaN codes)."""
    if fmt not in QUANT_FORMATS:
        raise ValueError(f"fmt must be one of {tuple(QUANT_FORMATS)}, got {fmt!r}")
    if per not in ("channel", "node"):
        raise ValueError(f'per must be "channel" or "node", got {per!r}')
    if x.dim() != 4:
        raise ValueError(f"node features must be (N, C, H, W), got {tuple(x.shape)}")
    qdtype, fmax, _code = QUANT_FORMATS[fmt]
    n, C = x.shape[:2]
    with torch.no_grad():
        xf = x.detach().float()
        if xf.numel() == 0:
            return torch.empty(x.shape, device=x.device, dtype=qdtype), torch.ones((n, C), device=x.device)
        if per == "channel":
            a = xf.abs().amax(dim=(2, 3))
        else:
            a = xf.abs().amax(dim=(1, 2, 3)).unsqueeze(1).expand(n, C)
        s = torch.where(a > 0, a / fmax, torch.ones_like(a)).contiguous()
        xq = (xf / s[:, :, None, None]).clamp(-fmax, fmax).to(qdtype).contiguous()
    return xq, s


def _q_scale(scale: Optional[torch.Tensor], n: int, C: int) -> Optional[torch.Tensor]:
    """scale as (N, C): given as (N,), (N, 1) or (N, C)."""
    if scale is None:
        return None
    if scale.dim() == 1:
        scale = scale.unsqueeze(1)
    if scale.dim() != 2 or scale.shape[0] != n or scale.shape[1] not in (1, C):
        raise ValueError(f"scale must be ({n},), ({n}, 1) or ({n}, {C}), got {tuple(scale.shape)}")
    return scale.expand(n, C)


def dequantize_features(xq: torch.Tensor, scale: Optional[torch.Tensor]) -> torch.Tensor:
    """``xq.float() * scale[:, :, None, None]`` in fp32: exactly the x^ the kernel forms in registers (the
    decode is exact, the product one fp32 rounding).  ``scale``: (N,), (N, 1), (N, C) or None (all 1)."""
    if xq.dtype not in _QDTYPES:
        raise TypeError(f"xq must be float8_e4m3fn or float8_e5m2, got {xq.dtype}")
    if xq.dim() != 4:
        raise ValueError(f"quantised features must be (N, C, H, W), got {tuple(xq.shape)}")
    xf = xq.float()
    if scale is None:
        return xf
    return xf * _q_scale(scale, xq.shape[0], xq.shape[1]).float()[:, :, None, None]


def _dense_node_stride(t: torch.Tensor) -> Optional[int]:
    """``node_stride`` without its dtype check (FP8 codes)."""
    n, c, h, w = t.shape
    if n == 0 or c * h * w == 0:
        return c * h * w
    s = t.stride()
    if (w == 1 or s[3] == 1) and (h == 1 or s[2] == w) and (c == 1 or s[1] == h * w) and (n == 1 or s[0] >= c * h * w):
        return s[0] if n > 1 else c * h * w
    return None


def film_mean_q_forward_into(xq: torch.Tensor, scale: Optional[torch.Tensor], gb: Optional[torch.Tensor],
                             csr: GraphCSR, out: torch.Tensor, mode="film_mean", logits: bool = False,
                             x0: Optional[torch.Tensor] = None, agg_scale: float = 1.0,
                             x0_scale: float = 0.0) -> torch.Tensor:
    """:func:`film_mean_q` into ``out`` (N, C, H, W) fp32 / bf16 / fp16 — which may be a strided view with a
    contiguous block per node, such as the second half of a ``torch.cat((h, g_h), 1)`` buffer."""
    if xq.dtype not in _QDTYPES:
        raise TypeError(f"xq must be float8_e4m3fn or float8_e5m2 (quantize_features), got {xq.dtype}")
    if xq.dim() != 4:
        raise ValueError(f"quantised features must be (N, C, H, W), got {tuple(xq.shape)}")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (gb, x0, scale)):
        raise RuntimeError("mrp_gnn: film_mean_q is an inference op and would drop the gradient of gb / x0; "
                           "run it under torch.no_grad(), or train through film_mean_fq (same forward bits)")
    n, C, H, W = xq.shape
    if n != csr.num_nodes:
        raise ValueError(f"xq has {n} nodes, graph has {csr.num_nodes}")
    if out.dim() != 4 or tuple(out.shape) != (n, C, H, W):
        raise ValueError(f"out must be {(n, C, H, W)}, got {tuple(out.shape)}")
    if out.dtype not in FEATURE_DTYPES:
        raise TypeError(f"out must be float32, bfloat16 or float16 (FP8 outputs are not provided), got {out.dtype}")
    os_ = node_stride(out)
    if os_ is None:
        raise ValueError("out must have a contiguous C*H*W block per node (pixel-major FP8 kernels are not provided)")
    _require_device(xq, out, scale)
    xs = _dense_node_stride(xq)
    if xs is None:  # channels_last or otherwise strided codes: made NCHW-contiguous first
        xq = xq.contiguous()
        xs = C * H * W
    sc = _q_scale(scale, n, C)
    if sc is not None:
        sc = sc.float().contiguous()
    m = _mode_flags(mode, logits)
    gb = _gb_fp32(gb, csr, C, m)
    ep, keep = None, None
    if x0 is not None or float(agg_scale) != 1.0:
        x0p = x0s = 0
        if x0 is not None:
            if tuple(x0.shape) != (n, C, H, W):
                raise ValueError(f"x0 must have the node features' shape {(n, C, H, W)}")
            _require_device(x0)
            keep, x0s = _as_node_major(x0.detach().to(out.dtype) if x0.dtype != out.dtype else x0.detach())
            x0p = keep.data_ptr()
        ep = _lib.Epilogue(float(agg_scale), 0.0, x0p, x0s, float(x0_scale) if x0 is not None else 0.0, 0, 0)
    name, code = _QDTYPES[xq.dtype]
    lib = _lib.load_library()
    with torch.cuda.device(xq.device):
        rc = lib.mrp_film_mean_fwd_q(code, _ptr(xq), xs, _ptr(sc), FEATURE_DTYPES[out.dtype],
                                     *_graph_args(gb, csr, C, H * W, m), _ptr(out), os_,
                                     ctypes.byref(ep) if ep is not None else None, _stream(xq.device))
    _lib.check(rc, "mrp_film_mean_fwd_q")
    PATH_COUNTS["fwd_q_" + name] += 1
    return out


def film_mean_q(xq: torch.Tensor, scale: Optional[torch.Tensor], gb: Optional[torch.Tensor], csr: GraphCSR,
                mode="film_mean", logits: bool = False, out_dtype: torch.dtype = torch.bfloat16,
                x0: Optional[torch.Tensor] = None, agg_scale: float = 1.0, x0_scale: float = 0.0) -> torch.Tensor:
    """The FiLM-mean aggregation of FP8 messages, read natively (``mrp_film_mean_fwd_q``).

    xq: (N, C, H, W) ``torch.float8_e4m3fn`` / ``torch.float8_e5m2`` codes; scale: their fp32 scales, (N,),
    (N, 1) or (N, C) (``quantize_features``), or None; gb / csr / mode / logits as :func:`film_mean`.
    Returns ``agg_scale * aggregate + x0_scale * x0`` in ``out_dtype`` (fp32, bf16 or fp16) — x0 (cast to
    ``out_dtype``) carries a layer's own, unquantised features: a robot's own maps never cross the link.
    Bit-equal to ``film_mean(dequantize_features(xq, scale), ...)`` with the same epilogue, cast once.
    An inference op: under grad mode with a ``gb`` / ``x0`` that requires grad it raises (``film_mean_fq``
    is the differentiable route)."""
    if xq.dim() != 4:
        raise ValueError(f"quantised features must be (N, C, H, W), got {tuple(xq.shape)}")
    if out_dtype not in FEATURE_DTYPES:
        raise TypeError(f"out_dtype must be float32, bfloat16 or float16, got {out_dtype}")
    out = torch.empty(xq.shape, device=xq.device, dtype=out_dtype)
    return film_mean_q_forward_into(xq, scale, gb, csr, out, mode, logits, x0, agg_scale, x0_scale)


class _StraightThrough(torch.autograd.Function):
    """``xh`` in the forward (its bits untouched), the gradient handed to ``x`` as if ``xh`` were ``x``."""

    @staticmethod
    def forward(ctx, x, xh):
        ctx.x_dtype = x.dtype
        return xh.view_as(xh)

    @staticmethod
    def backward(ctx, grad):
        return grad.to(ctx.x_dtype), None


def film_mean_fq(x: torch.Tensor, gb: Optional[torch.Tensor], csr: GraphCSR, fmt: str = "e4m3",
                 per: str = "channel", mode="film_mean", logits: bool = False, x0: Optional[torch.Tensor] = None,
                 agg_scale: float = 1.0, x0_scale: float = 0.0) -> torch.Tensor:
    """The differentiable fake-quant route of :func:`film_mean_q`, on the existing kernels: x is quantised
    (``quantize_features``), x^ formed in fp32 (``dequantize_features``) with a straight-through estimator
    (the gradient reaches x as if x^ = x), and the fp32 ``FilmMeanFunction`` run on it with the epilogue
    (``x0.float()``); the result is cast to ``x.dtype``.  Its forward bits equal
    ``film_mean_q(*quantize_features(x, fmt, per), ..., out_dtype=x.dtype)``."""
    _check_x(x)
    xq, s = quantize_features(x, fmt, per)
    xh = dequantize_features(xq, s)
    if torch.is_grad_enabled() and x.requires_grad:
        xh = _StraightThrough.apply(x, xh)
    m = _mode_flags(mode, logits)
    if (m & ~_lib.GB_LOGITS) == _lib.MODE_COPY_MEAN:
        gb = None
    if x0 is not None:
        # the native kernel reads x0 in the output type: the same value, widened exactly
        x0 = x0.to(x.dtype).float()
    out = FilmMeanFunction.apply(xh, gb, x0, csr, m, (float(agg_scale), 0.0, float(x0_scale) if x0 is not None else 0.0))
    return out.to(x.dtype)


# ---------------------------------------------------------------------------------------------------------
# Max-pooled FiLM aggregation: ``node_udf = torch.max(mailbox, 1)`` (``mrp_film_max_fwd`` / ``_bwd``).
#
#     m_j   = gamma_e * x[src(e)] + beta_e          for v's in-edges e in edge-id (mailbox) order
#     out_v = max_j m_j                             element-wise; zeros if deg v = 0
#
# and torch's autograd of it: on a tie the first maximal message takes the whole gradient, a NaN message
# beats every number and the first NaN wins.  An operator of its own, not a value of ``_lib.MODES`` (that
# table numbers the ``mode`` argument of ``mrp_film_mean_*``).  Every CSR entry is its own candidate, so
# parallel edges and self-loops are meaningful; every in-degree must be <= ``_lib.FILM_MAX_DEGREE``.
# channels_last features take the copy-first route: copied to NCHW, aggregated by the NCHW kernels.
# ---------------------------------------------------------------------------------------------------------
def _check_max_degree(csr: GraphCSR) -> None:
    bound = getattr(csr, "max_in_degree", -1)
    if bound < 0:
        raise ValueError("film_max needs the graph's in-degree bound: GraphCSR.max_in_degree is unknown (-1); "
                         f"every in-degree must be <= {_lib.FILM_MAX_DEGREE}")
    if bound > _lib.FILM_MAX_DEGREE:
        raise ValueError(f"film_max: a node has in-degree {bound}; the limit is {_lib.FILM_MAX_DEGREE} "
                         "(MRP_FILM_MAX_DEGREE)")


def _max_gb(gb, csr, C):
    if gb is None:
        raise ValueError("gamma/beta tensor required for film_max")
    gb = gb.reshape(csr.num_edges, C, 2)
    if not gb.is_contiguous() or gb.dtype != torch.float32:
        gb = gb.contiguous().float()
    _require_device(gb)
    return gb


def _check_max_flags(flags: int) -> int:
    flags = int(flags)
    if flags not in (0, _lib.GB_LOGITS):
        raise ValueError(f"film_max flags must be 0 or GB_LOGITS ({_lib.GB_LOGITS:#x}), got {flags:#x}")
    return flags


def film_max_forward_into(x: torch.Tensor, gb: torch.Tensor, csr: GraphCSR, flags: int,
                          out: torch.Tensor) -> torch.Tensor:
    """Run ``mrp_film_max_fwd`` into ``out`` (N, C, H, W) — which may be a strided view such as the second
    half of a ``torch.cat((h, g_h), 1)`` buffer.  ``flags``: 0 or ``_lib.GB_LOGITS``.  No autograd."""
    _check_max_degree(csr)  # a host-side property of the graph: checked before anything touches a device
    _require_device(x, out)
    flags = _check_max_flags(flags)
    if x.dim() != 4 or x.dtype not in FEATURE_DTYPES:
        raise ValueError("node features must be (N, C, H, W) float32, bfloat16 or float16")
    n, C, H, W = x.shape
    x, xs = _as_node_major(x)  # a channels_last x is copied to NCHW here
    os_ = node_stride(out)
    if os_ is None or tuple(out.shape) != (n, C, H, W) or out.dtype != x.dtype:
        raise ValueError(f"out must be {(n, C, H, W)} {x.dtype} with a contiguous block per node")
    if n != csr.num_nodes:
        raise ValueError(f"x has {n} nodes, graph has {csr.num_nodes}")
    gb = _max_gb(gb, csr, C)
    lib = _lib.load_library()
    with torch.cuda.device(x.device):
        code = lib.mrp_film_max_fwd(FEATURE_DTYPES[x.dtype], _ptr(x), xs, *_graph_args(gb, csr, C, H * W, flags),
                                    _ptr(out), os_, _stream(x.device))
    _lib.check(code, "mrp_film_max_fwd")
    PATH_COUNTS["max_fwd_" + _DTYPE_KEYS[x.dtype]] += 1
    return out


def film_max_backward(grad_out: torch.Tensor, x: torch.Tensor, gb: torch.Tensor, csr: GraphCSR, flags: int,
                      need_dx: bool, need_dgb: bool, grad_x_base: Optional[torch.Tensor] = None):
    """(grad_x or None, grad_gb (E, C, 2) or None) of :func:`film_max_forward_into`; ``grad_x_base``
    (N, C, H, W), if given, is added into grad_x by the kernel.  The winners are recomputed from x and gb
    (no argmax is saved); grad_x is NCHW in x's dtype, grad_gb fp32 with every unnamed row zero."""
    _check_max_degree(csr)
    _require_device(grad_out, x)
    flags = _check_max_flags(flags)
    if x.dim() != 4 or x.dtype not in FEATURE_DTYPES:
        raise ValueError("node features must be (N, C, H, W) float32, bfloat16 or float16")
    n, C, H, W = x.shape
    if n != csr.num_nodes:
        raise ValueError(f"x has {n} nodes, graph has {csr.num_nodes}")
    # the kernel reads grad_out and the base with x's extents: a mismatch would be an out-of-bounds read
    if tuple(grad_out.shape) != (n, C, H, W):
        raise ValueError(f"grad_out must be {(n, C, H, W)}, got {tuple(grad_out.shape)}")
    if grad_x_base is not None and tuple(grad_x_base.shape) != (n, C, H, W):
        raise ValueError(f"grad_x_base must be {(n, C, H, W)}, got {tuple(grad_x_base.shape)}")
    if grad_x_base is not None:
        _require_device(grad_x_base)
    dtype = x.dtype
    if grad_out.dtype != dtype:
        grad_out = grad_out.to(dtype)
    grad_out, gs = _as_node_major(grad_out)
    x, xs = _as_node_major(x)
    bs = 0
    if grad_x_base is not None and need_dx:
        if grad_x_base.dtype != dtype:
            grad_x_base = grad_x_base.to(dtype)
        grad_x_base, bs = _as_node_major(grad_x_base)
    else:
        grad_x_base = None
    dx = torch.empty((n, C, H, W), device=x.device, dtype=dtype) if need_dx else None
    dgb = torch.empty((csr.num_edges, C, 2), device=x.device, dtype=torch.float32) if need_dgb else None
    if not (need_dx or need_dgb):
        return None, None
    gb = _max_gb(gb, csr, C)
    lib = _lib.load_library()
    with torch.cuda.device(x.device):
        code = lib.mrp_film_max_bwd(FEATURE_DTYPES[dtype], _ptr(grad_out), gs, _ptr(x), xs,
                                    *_graph_args(gb, csr, C, H * W, flags), _ptr(dx),
                                    (C * H * W) if dx is not None else 0, _ptr(grad_x_base), bs, _ptr(dgb),
                                    _stream(x.device))
    _lib.check(code, "mrp_film_max_bwd")
    PATH_COUNTS["max_bwd_" + _DTYPE_KEYS[dtype]] += 1
    return dx, dgb


class FilmMaxFunction(torch.autograd.Function):
    """Autograd wrapper: forward = ``mrp_film_max_fwd``, backward = ``mrp_film_max_bwd``.  ``flags`` may be
    ``_lib.GB_LOGITS`` (gb = pre-sigmoid logits; the gradient is then d logits)."""

    @staticmethod
    def forward(ctx, x, gb, csr: GraphCSR, flags: int):
        out = torch.empty(tuple(x.shape), device=x.device, dtype=x.dtype)
        film_max_forward_into(x, gb, csr, flags, out)
        ctx.save_for_backward(x, gb)
        ctx.csr, ctx.flags = csr, flags
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, gb = ctx.saved_tensors
        dx, dgb = film_max_backward(grad_out, x, gb, ctx.csr, ctx.flags, ctx.needs_input_grad[0],
                                    ctx.needs_input_grad[1])
        if dgb is not None:
            dgb = dgb.view(gb.shape).to(gb.dtype)
        return dx, dgb, None, None


def film_max(x: torch.Tensor, gb: torch.Tensor, csr: GraphCSR, logits: bool = False) -> torch.Tensor:
    """``max_e(gamma_e * x_src + beta_e)`` per destination node, element-wise over (C, H, W): the reducer
    ``torch.max(mailbox, 1)`` in place of the reference's mean, with torch's autograd of it (first maximal
    message on a tie, first NaN wins).

    x: (N, C, H, W) fp32, bf16 or fp16 on a ROCm device (16-bit features are widened exactly, the messages
    are fp32, the output is rounded once); gb: (E, 2C) or (E, C, 2) interleaved gamma/beta, or their
    pre-sigmoid logits with ``logits=True``; csr: ``RobotGraph.csr(device)``, every in-degree
    <= ``_lib.FILM_MAX_DEGREE`` (``ValueError`` otherwise)."""
    _check_max_degree(csr)  # a host-side property of the graph: checked before anything touches a device
    _check_x(x)
    return FilmMaxFunction.apply(x, gb, csr, _lib.GB_LOGITS if logits else 0)


class FilmMaxCatFunction(torch.autograd.Function):
    """``torch.cat((x, film_max(x, gb)), 1)``: the kernel writes the aggregate into the second half of the
    (N, 2C, H, W) buffer through its node stride, x is copied into the first half by torch; backward hands
    the kernel the second half of the incoming gradient as grad_out and the first half as grad_x's base."""

    @staticmethod
    def forward(ctx, x, gb, csr: GraphCSR, flags: int):
        n, C, H, W = x.shape
        buf = torch.empty((n, 2 * C, H, W), device=x.device, dtype=x.dtype)
        film_max_forward_into(x, gb, csr, flags, buf[:, C:])
        buf[:, :C].copy_(x)
        ctx.save_for_backward(x, gb)
        ctx.csr, ctx.flags = csr, flags
        return buf

    @staticmethod
    def backward(ctx, grad_buf):
        x, gb = ctx.saved_tensors
        C = x.shape[1]
        need_dx = ctx.needs_input_grad[0]
        dx, dgb = film_max_backward(grad_buf[:, C:], x, gb, ctx.csr, ctx.flags, need_dx, ctx.needs_input_grad[1],
                                    grad_x_base=grad_buf[:, :C] if need_dx else None)
        if dgb is not None:
            dgb = dgb.view(gb.shape).to(gb.dtype)
        return dx, dgb, None, None


def film_max_cat(x: torch.Tensor, gb: torch.Tensor, csr: GraphCSR, logits: bool = False) -> torch.Tensor:
    """``torch.cat((x, film_max(x, gb, csr, logits)), dim=1)`` without a concatenation pass for the aggregate."""
    _check_max_degree(csr)
    _check_x(x)
    return FilmMaxCatFunction.apply(x, gb, csr, _lib.GB_LOGITS if logits else 0)


def film_max_residual(x: torch.Tensor, gb: torch.Tensor, csr: GraphCSR, logits: bool = False) -> torch.Tensor:
    """``x + film_max(x, ...)`` (the sum by torch: no fused epilogue for this reducer)."""
    return x + film_max(x, gb, csr, logits)


def film_max_mix(x: torch.Tensor, gb: torch.Tensor, csr: GraphCSR, x0: torch.Tensor, alpha: float,
                 logits: bool = False) -> torch.Tensor:
    """``(1 - alpha) * film_max(x, ...) + alpha * x0`` (by torch ops: no fused epilogue for this reducer)."""
    return (1.0 - float(alpha)) * film_max(x, gb, csr, logits) + float(alpha) * x0


# ---------------------------------------------------------------------------------------------------------
# Attention-pooled FiLM aggregation: per-location attention fusion (``mrp_film_attn_fwd`` / ``_bwd``).
#
#     m_j   = gamma_e * x[src(e)] + beta_e                       for v's in-edges e in edge-id order
#     s_j   = scale * sum_c x[v, c] * m_j[c]                     per pixel; scale defaults to 1 / sqrt(C)
#     a     = softmax_j s_j                                      per pixel, over the row's entries
#     out_v = sum_j a_j * m_j                                    zeros if deg v = 0
#
# and its full autograd (value, key and query paths).  The weights are an output: ``attn`` (E, H*W) fp32 by
# edge id, rows no CSR entry names zero; the backward reads them back and recomputes only the messages.
# Every CSR entry is its own message (parallel edges, self-loops); every in-degree must be
# <= ``_lib.FILM_ATTN_DEGREE``.  channels_last features take the copy-first route, as for the max.
#
# ``heads=H`` > 1 (``mrp_film_attn_fwd_mh`` / ``_bwd_mh``): head k owns channels [k C/H, (k+1) C/H) and has its
# own scores and softmax — bit for bit the single-head operator on that channel slice — in one launch whose
# grid is H times larger; the weights are (H, E, H*W) head-major and scale defaults to 1 / sqrt(C / H).
# ---------------------------------------------------------------------------------------------------------
def _check_attn_degree(csr: GraphCSR) -> None:
    bound = getattr(csr, "max_in_degree", -1)
    if bound < 0:
        raise ValueError("film_attn needs the graph's in-degree bound: GraphCSR.max_in_degree is unknown (-1); "
                         f"every in-degree must be <= {_lib.FILM_ATTN_DEGREE}")
    if bound > _lib.FILM_ATTN_DEGREE:
        raise ValueError(f"film_attn: a node has in-degree {bound}; the limit is {_lib.FILM_ATTN_DEGREE} "
                         "(MRP_FILM_ATTN_DEGREE)")


def _attn_gb(gb, csr, C):
    if gb is None:
        raise ValueError("gamma/beta tensor required for film_attn")
    gb = gb.reshape(csr.num_edges, C, 2)
    if not gb.is_contiguous() or gb.dtype != torch.float32:
        gb = gb.contiguous().float()
    _require_device(gb)
    return gb


def _check_attn_flags(flags: int) -> int:
    flags = int(flags)
    if flags not in (0, _lib.GB_LOGITS):
        raise ValueError(f"film_attn flags must be 0 or GB_LOGITS ({_lib.GB_LOGITS:#x}), got {flags:#x}")
    return flags


def _attn_scale(scale, C: int) -> float:
    s = 1.0 / math.sqrt(C) if scale is None and C > 0 else (0.0 if scale is None else float(scale))
    if not math.isfinite(s):
        raise ValueError(f"film_attn scale must be finite, got {scale!r}")
    return s


def _check_heads(heads, C: int) -> int:
    """The head count of a multi-head call: a positive int that divides C."""
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
        raise ValueError(f"film_attn heads must be a positive int, got {heads!r}")
    if C % heads:
        raise ValueError(f"film_attn heads must divide the channels: C = {C}, heads = {heads}")
    return heads


def _weights_shape(csr: GraphCSR, P: int, heads: int):
    """(E, P) of a single-head call, (H, E, P) head-major of a multi-head one."""
    return (csr.num_edges, P) if heads == 1 else (heads, csr.num_edges, P)


def _attn_workspace(lib, direction: int, csr: GraphCSR, C: int, P: int, device):
    nbytes = lib.mrp_film_attn_workspace(direction, csr.num_graphs, csr.max_nodes, csr.graph_kind, csr.num_nodes,
                                         csr.num_edges, C, P)
    if nbytes <= 0:
        return None, 0
    return torch.empty(((nbytes + 3) // 4,), device=device, dtype=torch.float32), nbytes


def film_attn_forward_into(x: torch.Tensor, gb: torch.Tensor, csr: GraphCSR, flags: int, out: torch.Tensor,
                           scale: Optional[float] = None, attn: Optional[torch.Tensor] = None,
                           heads: int = 1) -> torch.Tensor:
    """Run ``mrp_film_attn_fwd`` into ``out`` (N, C, H, W) — which may be a strided view such as the second
    half of a ``torch.cat((h, g_h), 1)`` buffer — and return the weights ``attn`` (E, H*W) fp32 (written
    into the given tensor, else a new one).  ``flags``: 0 or ``_lib.GB_LOGITS``.  ``heads`` > 1 runs
    ``mrp_film_attn_fwd_mh``: attn is then (heads, E, H*W).  No autograd."""
    _check_attn_degree(csr)  # a host-side property of the graph: checked before anything touches a device
    _require_device(x, out, attn)
    flags = _check_attn_flags(flags)
    if x.dim() != 4 or x.dtype not in FEATURE_DTYPES:
        raise ValueError("node features must be (N, C, H, W) float32, bfloat16 or float16")
    n, C, H, W = x.shape
    heads = _check_heads(heads, C)
    scale = _attn_scale(scale, C // heads)
    x, xs = _as_node_major(x)  # a channels_last x is copied to NCHW here
    os_ = node_stride(out)
    if os_ is None or tuple(out.shape) != (n, C, H, W) or out.dtype != x.dtype:
        raise ValueError(f"out must be {(n, C, H, W)} {x.dtype} with a contiguous block per node")
    if n != csr.num_nodes:
        raise ValueError(f"x has {n} nodes, graph has {csr.num_nodes}")
    gb = _attn_gb(gb, csr, C)
    wshape = _weights_shape(csr, H * W, heads)
    if attn is None:
        attn = torch.empty(wshape, device=x.device, dtype=torch.float32)
    elif tuple(attn.shape) != wshape or attn.dtype != torch.float32 or not attn.is_contiguous():
        raise ValueError(f"attn must be a contiguous {wshape} float32 tensor")
    lib = _lib.load_library()
    with torch.cuda.device(x.device):
        ws, nbytes = _attn_workspace(lib, 0, csr, C, H * W, x.device)
        ga = _graph_args(gb, csr, C, H * W, flags)
        if heads == 1:
            code = lib.mrp_film_attn_fwd(FEATURE_DTYPES[x.dtype], _ptr(x), xs, *ga, _ptr(out), os_, scale,
                                         _ptr(attn), _ptr(ws), nbytes, _stream(x.device))
        else:
            code = lib.mrp_film_attn_fwd_mh(FEATURE_DTYPES[x.dtype], _ptr(x), xs, *ga, heads, _ptr(out), os_, scale,
                                            _ptr(attn), _ptr(ws), nbytes, _stream(x.device))
    _lib.check(code, "mrp_film_attn_fwd" if heads == 1 else "mrp_film_attn_fwd_mh")
    PATH_COUNTS[("attn_fwd_" if heads == 1 else "attn_fwd_mh_") + _DTYPE_KEYS[x.dtype]] += 1
    return attn


def film_attn_backward(grad_out: torch.Tensor, x: torch.Tensor, gb: torch.Tensor, attn: torch.Tensor, csr: GraphCSR,
                       flags: int, need_dx: bool, need_dgb: bool, grad_x_base: Optional[torch.Tensor] = None,
                       scale: Optional[float] = None, heads: int = 1):
    """(grad_x or None, grad_gb (E, C, 2) or None) of :func:`film_attn_forward_into`, ``attn`` being the
    weights it returned (``heads`` as there); ``grad_x_base`` (N, C, H, W), if given, is added into grad_x by
    the kernel.  grad_x is NCHW in x's dtype, grad_gb fp32 with every unnamed row zero."""
    _check_attn_degree(csr)
    _require_device(grad_out, x, attn)
    flags = _check_attn_flags(flags)
    if x.dim() != 4 or x.dtype not in FEATURE_DTYPES:
        raise ValueError("node features must be (N, C, H, W) float32, bfloat16 or float16")
    n, C, H, W = x.shape
    heads = _check_heads(heads, C)
    scale = _attn_scale(scale, C // heads)
    if n != csr.num_nodes:
        raise ValueError(f"x has {n} nodes, graph has {csr.num_nodes}")
    # the kernel reads grad_out, the base and attn with x's extents: a mismatch would be an out-of-bounds read
    if tuple(grad_out.shape) != (n, C, H, W):
        raise ValueError(f"grad_out must be {(n, C, H, W)}, got {tuple(grad_out.shape)}")
    if grad_x_base is not None and tuple(grad_x_base.shape) != (n, C, H, W):
        raise ValueError(f"grad_x_base must be {(n, C, H, W)}, got {tuple(grad_x_base.shape)}")
    wshape = _weights_shape(csr, H * W, heads)
    if tuple(attn.shape) != wshape or attn.dtype != torch.float32:
        raise ValueError(f"attn must be {wshape} float32, got {tuple(attn.shape)} {attn.dtype}")
    if grad_x_base is not None:
        _require_device(grad_x_base)
    attn = attn.contiguous()
    dtype = x.dtype
    if grad_out.dtype != dtype:
        grad_out = grad_out.to(dtype)
    grad_out, gs = _as_node_major(grad_out)
    x, xs = _as_node_major(x)
    bs = 0
    if grad_x_base is not None and need_dx:
        if grad_x_base.dtype != dtype:
            grad_x_base = grad_x_base.to(dtype)
        grad_x_base, bs = _as_node_major(grad_x_base)
    else:
        grad_x_base = None
    dx = torch.empty((n, C, H, W), device=x.device, dtype=dtype) if need_dx else None
    dgb = torch.empty((csr.num_edges, C, 2), device=x.device, dtype=torch.float32) if need_dgb else None
    if not (need_dx or need_dgb):
        return None, None
    gb = _attn_gb(gb, csr, C)
    lib = _lib.load_library()
    with torch.cuda.device(x.device):
        ws, nbytes = _attn_workspace(lib, 1, csr, C, H * W, x.device) if need_dgb else (None, 0)
        ga = _graph_args(gb, csr, C, H * W, flags)
        tail = (_ptr(dx), (C * H * W) if dx is not None else 0, _ptr(grad_x_base), bs, _ptr(dgb), scale, _ptr(attn),
                _ptr(ws), nbytes, _stream(x.device))
        if heads == 1:
            code = lib.mrp_film_attn_bwd(FEATURE_DTYPES[dtype], _ptr(grad_out), gs, _ptr(x), xs, *ga, *tail)
        else:
            code = lib.mrp_film_attn_bwd_mh(FEATURE_DTYPES[dtype], _ptr(grad_out), gs, _ptr(x), xs, *ga, heads, *tail)
    _lib.check(code, "mrp_film_attn_bwd" if heads == 1 else "mrp_film_attn_bwd_mh")
    PATH_COUNTS[("attn_bwd_" if heads == 1 else "attn_bwd_mh_") + _DTYPE_KEYS[dtype]] += 1
    return dx, dgb


class FilmAttnFunction(torch.autograd.Function):
    """Autograd wrapper: forward = ``mrp_film_attn_fwd``, backward = ``mrp_film_attn_bwd``.  Returns
    (out, attn); attn is saved for the backward and is not differentiable.  ``flags`` may be
    ``_lib.GB_LOGITS`` (gb = pre-sigmoid logits; the gradient is then d logits)."""

    @staticmethod
    def forward(ctx, x, gb, csr: GraphCSR, flags: int, scale, heads: int = 1):
        out = torch.empty(tuple(x.shape), device=x.device, dtype=x.dtype)
        attn = film_attn_forward_into(x, gb, csr, flags, out, scale, heads=heads)
        ctx.save_for_backward(x, gb, attn)
        ctx.csr, ctx.flags, ctx.scale, ctx.heads = csr, flags, scale, heads
        ctx.mark_non_differentiable(attn)
        return out, attn

    @staticmethod
    def backward(ctx, grad_out, _grad_attn):
        x, gb, attn = ctx.saved_tensors
        dx, dgb = film_attn_backward(grad_out, x, gb, attn, ctx.csr, ctx.flags, ctx.needs_input_grad[0],
                                     ctx.needs_input_grad[1], scale=ctx.scale, heads=ctx.heads)
        if dgb is not None:
            dgb = dgb.view(gb.shape).to(gb.dtype)
        return dx, dgb, None, None, None, None


def film_attn(x: torch.Tensor, gb: torch.Tensor, csr: GraphCSR, logits: bool = False,
              scale: Optional[float] = None, return_weights: bool = False, heads: int = 1):
    """Per-location attention over the FiLM messages of each destination's in-neighbours: at every pixel the
    receiver's feature vector scores each message ``gamma_e * x_src + beta_e`` (``scale`` times their dot
    product over the channels, ``1/sqrt(C)`` by default), a softmax over the node's in-edges turns the scores
    into weights, and the output is the weighted sum of the messages; gradients reach x and gb through the
    values, the keys and the query.

    x: (N, C, H, W) fp32, bf16 or fp16 on a ROCm device (16-bit features are widened exactly; messages,
    scores and weights are fp32; the output is rounded once); gb: (E, 2C) or (E, C, 2) interleaved
    gamma/beta, or their pre-sigmoid logits with ``logits=True``; csr: ``RobotGraph.csr(device)``, every
    in-degree <= ``_lib.FILM_ATTN_DEGREE`` (``ValueError`` otherwise).  A self-loop lets a node attend to
    itself.  With ``return_weights=True`` returns ``(out, attn)``, attn (E, H*W) fp32 by edge id — the
    weights saved for the backward, not differentiable.

    ``heads=H`` > 1 is multi-head attention in one launch: head k owns channels [k C/H, (k+1) C/H) with its own
    scores and softmax (exactly ``film_attn`` on that channel slice), ``scale`` defaults to ``1/sqrt(C/H)``
    and attn is (H, E, H*W).  ``ValueError`` unless H is a positive int dividing C."""
    _check_attn_degree(csr)  # a host-side property of the graph: checked before anything touches a device
    heads = _check_heads(heads, x.shape[1] if x.dim() == 4 else 0)  # host-side too
    _check_x(x)
    out, attn = FilmAttnFunction.apply(x, gb, csr, _lib.GB_LOGITS if logits else 0, scale, heads)
    return (out, attn) if return_weights else out


class FilmAttnCatFunction(torch.autograd.Function):
    """``torch.cat((x, film_attn(x, gb)), 1)``: the kernel writes the aggregate into the second half of the
    (N, 2C, H, W) buffer through its node stride, x is copied into the first half by torch; backward hands
    the kernel the second half of the incoming gradient as grad_out and the first half as grad_x's base."""

    @staticmethod
    def forward(ctx, x, gb, csr: GraphCSR, flags: int, scale, heads: int = 1):
        n, C, H, W = x.shape
        buf = torch.empty((n, 2 * C, H, W), device=x.device, dtype=x.dtype)
        attn = film_attn_forward_into(x, gb, csr, flags, buf[:, C:], scale, heads=heads)
        buf[:, :C].copy_(x)
        ctx.save_for_backward(x, gb, attn)
        ctx.csr, ctx.flags, ctx.scale, ctx.heads = csr, flags, scale, heads
        ctx.mark_non_differentiable(attn)
        return buf, attn

    @staticmethod
    def backward(ctx, grad_buf, _grad_attn):
        x, gb, attn = ctx.saved_tensors
        C = x.shape[1]
        need_dx = ctx.needs_input_grad[0]
        dx, dgb = film_attn_backward(grad_buf[:, C:], x, gb, attn, ctx.csr, ctx.flags, need_dx,
                                     ctx.needs_input_grad[1], grad_x_base=grad_buf[:, :C] if need_dx else None,
                                     scale=ctx.scale, heads=ctx.heads)
        if dgb is not None:
            dgb = dgb.view(gb.shape).to(gb.dtype)
        return dx, dgb, None, None, None, None


def film_attn_cat(x: torch.Tensor, gb: torch.Tensor, csr: GraphCSR, logits: bool = False,
                  scale: Optional[float] = None, return_weights: bool = False, heads: int = 1):
    """``torch.cat((x, film_attn(x, gb, csr, logits, scale, heads=heads)), dim=1)`` without a concatenation pass
    for the aggregate."""
    _check_attn_degree(csr)
    heads = _check_heads(heads, x.shape[1] if x.dim() == 4 else 0)  # host-side too
    _check_x(x)
    buf, attn = FilmAttnCatFunction.apply(x, gb, csr, _lib.GB_LOGITS if logits else 0, scale, heads)
    return (buf, attn) if return_weights else buf


def film_attn_residual(x: torch.Tensor, gb: torch.Tensor, csr: GraphCSR, logits: bool = False,
                       scale: Optional[float] = None, heads: int = 1) -> torch.Tensor:
    """``x + film_attn(x, ...)`` (the sum by torch: no fused epilogue for this reducer)."""
    return x + film_attn(x, gb, csr, logits, scale, heads=heads)


def film_attn_mix(x: torch.Tensor, gb: torch.Tensor, csr: GraphCSR, x0: torch.Tensor, alpha: float,
                  logits: bool = False, scale: Optional[float] = None, heads: int = 1) -> torch.Tensor:
    """``(1 - alpha) * film_attn(x, ...) + alpha * x0`` (by torch ops: no fused epilogue for this reducer)."""
    return (1.0 - float(alpha)) * film_attn(x, gb, csr, logits, scale, heads=heads) + float(alpha) * x0


# ---------------------------------------------------------------------------------------------------------
# Confidence-weighted FiLM aggregation: per-pixel sender maps (``mrp_film_wmean_fwd`` / ``_bwd``).
#
#     m_j   = gamma_e * x[src(e)] + beta_e                      for v's in-edges e
#     out_v = sum_j w[src(e_j)] * m_j / sum_j w[src(e_j)]       pixel by pixel; 0 where nobody delivered
#
# ``w`` (N, H, W) fp32 >= 0 is the sender's spatial confidence map (Where2comm-style sparse messaging): a
# sender transmits only the locations worth sending and the receiver averages over what arrived.  With
# ``mode="sum"`` the weighted sum is not normalised.  An operator of its own with gradients for x, gb and w;
# with w == 1 it gives ``film_mean``'s bits.  channels_last features take the copy-first route.
# ---------------------------------------------------------------------------------------------------------
WAGG_MODES = {"mean": _lib.WAGG_MEAN, "sum": _lib.WAGG_SUM}


def _wagg(mode) -> int:
    if isinstance(mode, str):
        if mode not in WAGG_MODES:
            raise ValueError(f'film_wmean mode must be "mean" or "sum", got {mode!r}')
        return WAGG_MODES[mode]
    mode = int(mode)
    if mode not in WAGG_MODES.values():
        raise ValueError(f"film_wmean mode must be WAGG_MEAN or WAGG_SUM, got {mode}")
    return mode


def _check_wmean_flags(flags: int) -> int:
    flags = int(flags)
    if flags not in (0, _lib.GB_LOGITS):
        raise ValueError(f"film_wmean flags must be 0 or GB_LOGITS ({_lib.GB_LOGITS:#x}), got {flags:#x}")
    return flags


def _wmean_weights(w: torch.Tensor, n: int, H: int, W: int):
    """(w, node stride in elements) of a sender map (N, H, W) or (N, 1, H, W): fp32, each node's plane
    contiguous, the planes ``>= H*W`` apart."""
    if w is None:
        raise ValueError("film_wmean needs the sender maps w (N, H, W)")
    _require_device(w)
    if w.dim() == 4 and w.shape[1] == 1:
        w = w[:, 0]
    if w.dim() != 3 or tuple(w.shape) != (n, H, W):
        raise ValueError(f"w must be {(n, H, W)} or {(n, 1, H, W)}, got {tuple(w.shape)}")
    if w.dtype != torch.float32:
        raise ValueError(f"w must be float32, got {w.dtype}")
    s = w.stride()
    P = H * W
    ok = n == 0 or P == 0 or ((W == 1 or s[2] == 1) and (H == 1 or s[1] == W) and (n == 1 or s[0] >= P))
    if not ok:
        raise ValueError("w must have a contiguous (H, W) plane per node")
    return w, (s[0] if n > 1 else P)


def film_wmean_forward_into(x: torch.Tensor, gb: torch.Tensor, w: torch.Tensor, csr: GraphCSR, flags: int,
                            out: torch.Tensor, mode="mean") -> torch.Tensor:
    """Run ``mrp_film_wmean_fwd`` into ``out`` (N, C, H, W) — which may be a strided view such as the second
    half of a ``torch.cat((h, g_h), 1)`` buffer.  ``flags``: 0 or ``_lib.GB_LOGITS``.  No autograd."""
    _require_device(x, out)
    flags, wagg = _check_wmean_flags(flags), _wagg(mode)
    if x.dim() != 4 or x.dtype not in FEATURE_DTYPES:
        raise ValueError("node features must be (N, C, H, W) float32, bfloat16 or float16")
    n, C, H, W = x.shape
    x, xs = _as_node_major(x)  # a channels_last x is copied to NCHW here
    os_ = node_stride(out)
    if os_ is None or tuple(out.shape) != (n, C, H, W) or out.dtype != x.dtype:
        raise ValueError(f"out must be {(n, C, H, W)} {x.dtype} with a contiguous block per node")
    if n != csr.num_nodes:
        raise ValueError(f"x has {n} nodes, graph has {csr.num_nodes}")
    w, ws = _wmean_weights(w, n, H, W)
    gb = _max_gb(gb, csr, C)
    ga = _graph_args(gb, csr, C, H * W, flags)
    lib = _lib.load_library()
    with torch.cuda.device(x.device):
        code = lib.mrp_film_wmean_fwd(FEATURE_DTYPES[x.dtype], _ptr(x), xs, ga[0], _ptr(w), ws, *ga[1:], wagg,
                                      _ptr(out), os_, _stream(x.device))
    _lib.check(code, "mrp_film_wmean_fwd")
    PATH_COUNTS["wmean_fwd_" + _DTYPE_KEYS[x.dtype]] += 1
    return out


def film_wmean_backward(grad_out: torch.Tensor, x: torch.Tensor, gb: torch.Tensor, w: torch.Tensor, csr: GraphCSR,
                        flags: int, need_dx: bool, need_dgb: bool, need_dw: bool,
                        grad_x_base: Optional[torch.Tensor] = None, mode="mean"):
    """(grad_x, grad_gb (E, C, 2), grad_w (N, H, W)) of :func:`film_wmean_forward_into`, each None unless
    asked for; ``grad_x_base`` (N, C, H, W), if given, is added into grad_x by the kernel.  The kernels
    recompute the aggregate (nothing is saved by the forward); grad_x is NCHW in x's dtype, grad_gb and grad_w
    are fp32."""
    _require_device(grad_out, x)
    flags, wagg = _check_wmean_flags(flags), _wagg(mode)
    if x.dim() != 4 or x.dtype not in FEATURE_DTYPES:
        raise ValueError("node features must be (N, C, H, W) float32, bfloat16 or float16")
    n, C, H, W = x.shape
    if n != csr.num_nodes:
        raise ValueError(f"x has {n} nodes, graph has {csr.num_nodes}")
    # the kernel reads grad_out and the base with x's extents: a mismatch would be an out-of-bounds read
    if tuple(grad_out.shape) != (n, C, H, W):
        raise ValueError(f"grad_out must be {(n, C, H, W)}, got {tuple(grad_out.shape)}")
    if grad_x_base is not None and tuple(grad_x_base.shape) != (n, C, H, W):
        raise ValueError(f"grad_x_base must be {(n, C, H, W)}, got {tuple(grad_x_base.shape)}")
    if grad_x_base is not None:
        _require_device(grad_x_base)
    w, ws = _wmean_weights(w, n, H, W)
    if not (need_dx or need_dgb or need_dw):
        return None, None, None
    dtype = x.dtype
    if grad_out.dtype != dtype:
        grad_out = grad_out.to(dtype)
    grad_out, gs = _as_node_major(grad_out)
    x, xs = _as_node_major(x)
    bs = 0
    if grad_x_base is not None and need_dx:
        if grad_x_base.dtype != dtype:
            grad_x_base = grad_x_base.to(dtype)
        grad_x_base, bs = _as_node_major(grad_x_base)
    else:
        grad_x_base = None
    dx = torch.empty((n, C, H, W), device=x.device, dtype=dtype) if need_dx else None
    dgb = torch.empty((csr.num_edges, C, 2), device=x.device, dtype=torch.float32) if need_dgb else None
    dw = torch.empty((n, H, W), device=x.device, dtype=torch.float32) if need_dw else None
    gb = _max_gb(gb, csr, C)
    ga = _graph_args(gb, csr, C, H * W, flags)
    lib = _lib.load_library()
    work, nbytes = None, 0
    if need_dw:
        nbytes = lib.mrp_film_wmean_workspace(csr.num_graphs, csr.max_nodes, csr.graph_kind, csr.num_nodes,
                                              csr.num_edges, C, H * W)
        if nbytes > 0:
            work = torch.empty(((nbytes + 3) // 4,), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        code = lib.mrp_film_wmean_bwd(FEATURE_DTYPES[dtype], _ptr(grad_out), gs, _ptr(x), xs, ga[0], _ptr(w), ws,
                                      *ga[1:], wagg, _ptr(dx), (C * H * W) if dx is not None else 0,
                                      _ptr(grad_x_base), bs, _ptr(dgb), _ptr(dw), H * W if dw is not None else 0,
                                      _ptr(work), nbytes, _stream(x.device))
    _lib.check(code, "mrp_film_wmean_bwd")
    PATH_COUNTS["wmean_bwd_" + _DTYPE_KEYS[dtype]] += 1
    return dx, dgb, dw


class FilmWMeanFunction(torch.autograd.Function):
    """Autograd wrapper: forward = ``mrp_film_wmean_fwd``, backward = ``mrp_film_wmean_bwd`` with gradients
    for x, gb and w.  ``flags`` may be ``_lib.GB_LOGITS`` (the gb gradient is then d logits)."""

    @staticmethod
    def forward(ctx, x, gb, w, csr: GraphCSR, flags: int, wagg: int):
        out = torch.empty(tuple(x.shape), device=x.device, dtype=x.dtype)
        film_wmean_forward_into(x, gb, w, csr, flags, out, wagg)
        ctx.save_for_backward(x, gb, w)
        ctx.csr, ctx.flags, ctx.wagg = csr, flags, wagg
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, gb, w = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dgb, dw = film_wmean_backward(grad_out, x, gb, w, ctx.csr, ctx.flags, need[0], need[1], need[2],
                                          mode=ctx.wagg)
        if dgb is not None:
            dgb = dgb.view(gb.shape).to(gb.dtype)
        if dw is not None:
            dw = dw.view(w.shape)
        return dx, dgb, dw, None, None, None


def film_wmean(x: torch.Tensor, gb: torch.Tensor, w: torch.Tensor, csr: GraphCSR, mode="mean",
               logits: bool = False) -> torch.Tensor:
    """``sum_e w[src e] (gamma_e * x_src + beta_e) / sum_e w[src e]`` per destination node and pixel
    (``mode="sum"``: the numerator alone); pixels nobody delivered to give 0.  Differentiable in x, gb and w.

    x: (N, C, H, W) fp32, bf16 or fp16 on a ROCm device; gb: (E, 2C) or (E, C, 2) interleaved gamma/beta, or
    their pre-sigmoid logits with ``logits=True``; w: (N, H, W) or (N, 1, H, W) fp32 >= 0, each node's plane
    contiguous — the sender's map, indexed by source node; csr: ``RobotGraph.csr(device)``."""
    wagg = _wagg(mode)  # a host-side argument: checked before anything touches a device
    _check_x(x)
    return FilmWMeanFunction.apply(x, gb, w, csr, _lib.GB_LOGITS if logits else 0, wagg)


class FilmWMeanCatFunction(torch.autograd.Function):
    """``torch.cat((x, film_wmean(x, gb, w)), 1)``: the kernel writes the aggregate into the second half of
    the (N, 2C, H, W) buffer through its node stride, x is copied into the first half by torch; backward hands
    the kernel the second half of the incoming gradient as grad_out and the first half as grad_x's base."""

    @staticmethod
    def forward(ctx, x, gb, w, csr: GraphCSR, flags: int, wagg: int):
        n, C, H, W = x.shape
        buf = torch.empty((n, 2 * C, H, W), device=x.device, dtype=x.dtype)
        film_wmean_forward_into(x, gb, w, csr, flags, buf[:, C:], wagg)
        buf[:, :C].copy_(x)
        ctx.save_for_backward(x, gb, w)
        ctx.csr, ctx.flags, ctx.wagg = csr, flags, wagg
        return buf

    @staticmethod
    def backward(ctx, grad_buf):
        x, gb, w = ctx.saved_tensors
        C = x.shape[1]
        need = ctx.needs_input_grad
        dx, dgb, dw = film_wmean_backward(grad_buf[:, C:], x, gb, w, ctx.csr, ctx.flags, need[0], need[1], need[2],
                                          grad_x_base=grad_buf[:, :C] if need[0] else None, mode=ctx.wagg)
        if dgb is not None:
            dgb = dgb.view(gb.shape).to(gb.dtype)
        if dw is not None:
            dw = dw.view(w.shape)
        return dx, dgb, dw, None, None, None


def film_wmean_cat(x: torch.Tensor, gb: torch.Tensor, w: torch.Tensor, csr: GraphCSR, mode="mean",
                   logits: bool = False) -> torch.Tensor:
    """``torch.cat((x, film_wmean(x, gb, w, csr, mode, logits)), dim=1)`` without a concatenation pass for the
    aggregate."""
    wagg = _wagg(mode)
    _check_x(x)
    return FilmWMeanCatFunction.apply(x, gb, w, csr, _lib.GB_LOGITS if logits else 0, wagg)


def film_wmean_residual(x: torch.Tensor, gb: torch.Tensor, w: torch.Tensor, csr: GraphCSR, mode="mean",
                        logits: bool = False) -> torch.Tensor:
    """``x + film_wmean(x, ...)`` (the sum by torch: no fused epilogue for this reducer)."""
    return x + film_wmean(x, gb, w, csr, mode, logits)


def film_wmean_mix(x: torch.Tensor, gb: torch.Tensor, w: torch.Tensor, csr: GraphCSR, x0: torch.Tensor,
                   alpha: float, mode="mean", logits: bool = False) -> torch.Tensor:
    """``(1 - alpha) * film_wmean(x, ...) + alpha * x0`` (by torch ops: no fused epilogue for this reducer)."""
    return (1.0 - float(alpha)) * film_wmean(x, gb, w, csr, mode, logits) + float(alpha) * x0


# ---------------------------------------------------------------------------------------------------------
# Confidence-gated attention fusion (``mrp_film_wattn_fwd`` / ``_bwd``): ``film_attn`` over what was delivered.
#
#     m_j, s_j  as film_attn                                     for v's in-edges e_j, u_j = src(e_j)
#     a_j   = w[u_j] exp(s_j - mx) / sum_k w[u_k] exp(s_k - mx)  per pixel, over the entries with w[u_j] > 0
#     out_v = sum_j a_j * m_j                                    0 where nobody delivered
#
# ``w`` (N, H, W) fp32 >= 0 is ``film_wmean``'s sender map; an entry with w == 0 at a pixel is silent there: it
# takes no part in the softmax and its features reach nothing.  Gradients for x, gb and w; ``attn`` (E, H*W)
# is an output as for ``film_attn``, and ``rate`` (E, H*W), the softmax's response to each sender's weight, is
# computed only when w needs a gradient.  With w == 1 it gives ``film_attn``'s bits.  channels_last features
# take the copy-first route.
# ---------------------------------------------------------------------------------------------------------
def film_wattn_forward_into(x: torch.Tensor, gb: torch.Tensor, w: torch.Tensor, csr: GraphCSR, flags: int,
                            out: torch.Tensor, scale: Optional[float] = None, attn: Optional[torch.Tensor] = None,
                            rate=False, heads: int = 1):
    """Run ``mrp_film_wattn_fwd`` into ``out`` (N, C, H, W) — which may be a strided view such as the second
    half of a ``torch.cat((h, g_h), 1)`` buffer — and return ``(attn, rate)``: the weights (E, H*W) fp32
    (written into the given tensor, else a new one) and, with ``rate=True`` or a tensor to write into, the
    rates (E, H*W) fp32 the backward needs for grad_w (else None).  ``flags``: 0 or ``_lib.GB_LOGITS``.
    ``heads`` > 1 runs ``mrp_film_wattn_fwd_mh``: attn and rate are then (heads, E, H*W).  No autograd."""
    _check_attn_degree(csr)  # a host-side property of the graph: checked before anything touches a device
    _require_device(x, out, attn, rate if isinstance(rate, torch.Tensor) else None)
    flags = _check_attn_flags(flags)
    if x.dim() != 4 or x.dtype not in FEATURE_DTYPES:
        raise ValueError("node features must be (N, C, H, W) float32, bfloat16 or float16")
    n, C, H, W = x.shape
    heads = _check_heads(heads, C)
    scale = _attn_scale(scale, C // heads)
    x, xs = _as_node_major(x)  # a channels_last x is copied to NCHW here
    os_ = node_stride(out)
    if os_ is None or tuple(out.shape) != (n, C, H, W) or out.dtype != x.dtype:
        raise ValueError(f"out must be {(n, C, H, W)} {x.dtype} with a contiguous block per node")
    if n != csr.num_nodes:
        raise ValueError(f"x has {n} nodes, graph has {csr.num_nodes}")
    w, wst = _wmean_weights(w, n, H, W)
    gb = _attn_gb(gb, csr, C)
    wshape = _weights_shape(csr, H * W, heads)
    bufs = []
    for name, t in (("attn", attn), ("rate", rate)):
        if t is None or t is False:
            t = None if name == "rate" else torch.empty(wshape, device=x.device, dtype=torch.float32)
        elif t is True:
            t = torch.empty(wshape, device=x.device, dtype=torch.float32)
        elif tuple(t.shape) != wshape or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {wshape} float32 tensor")
        bufs.append(t)
    attn, rate = bufs
    lib = _lib.load_library()
    ga = _graph_args(gb, csr, C, H * W, flags)
    with torch.cuda.device(x.device):
        tail = (_ptr(out), os_, scale, _ptr(attn), _ptr(rate), None, 0, _stream(x.device))
        if heads == 1:
            code = lib.mrp_film_wattn_fwd(FEATURE_DTYPES[x.dtype], _ptr(x), xs, ga[0], _ptr(w), wst, *ga[1:], *tail)
        else:
            code = lib.mrp_film_wattn_fwd_mh(FEATURE_DTYPES[x.dtype], _ptr(x), xs, ga[0], _ptr(w), wst, *ga[1:], heads,
                                             *tail)
    _lib.check(code, "mrp_film_wattn_fwd" if heads == 1 else "mrp_film_wattn_fwd_mh")
    PATH_COUNTS[("wattn_fwd_" if heads == 1 else "wattn_fwd_mh_") + _DTYPE_KEYS[x.dtype]] += 1
    return attn, rate


def film_wattn_backward(grad_out: torch.Tensor, x: torch.Tensor, gb: torch.Tensor, w: torch.Tensor,
                        attn: torch.Tensor, rate: Optional[torch.Tensor], csr: GraphCSR, flags: int, need_dx: bool,
                        need_dgb: bool, need_dw: bool, grad_x_base: Optional[torch.Tensor] = None,
                        scale: Optional[float] = None, heads: int = 1):
    """(grad_x, grad_gb (E, C, 2), grad_w (N, H, W)) of :func:`film_wattn_forward_into`, each None unless asked
    for; ``attn`` and ``rate`` are what it returned, ``heads`` as there (``rate`` is needed for grad_w only;
    with several heads grad_w is the sum over the heads, ascending); ``grad_x_base``
    (N, C, H, W), if given, is added into grad_x by the kernel.  grad_x is NCHW in x's dtype, grad_gb and grad_w
    are fp32."""
    _check_attn_degree(csr)
    _require_device(grad_out, x, attn, rate)
    flags = _check_attn_flags(flags)
    if x.dim() != 4 or x.dtype not in FEATURE_DTYPES:
        raise ValueError("node features must be (N, C, H, W) float32, bfloat16 or float16")
    n, C, H, W = x.shape
    heads = _check_heads(heads, C)
    scale = _attn_scale(scale, C // heads)
    wshape = _weights_shape(csr, H * W, heads)
    if n != csr.num_nodes:
        raise ValueError(f"x has {n} nodes, graph has {csr.num_nodes}")
    # the kernel reads grad_out, the base, attn and rate with x's extents: a mismatch would be an out-of-bounds read
    if tuple(grad_out.shape) != (n, C, H, W):
        raise ValueError(f"grad_out must be {(n, C, H, W)}, got {tuple(grad_out.shape)}")
    if grad_x_base is not None and tuple(grad_x_base.shape) != (n, C, H, W):
        raise ValueError(f"grad_x_base must be {(n, C, H, W)}, got {tuple(grad_x_base.shape)}")
    for name, t in (("attn", attn), ("rate", rate)):
        if t is None and name == "rate":
            if need_dw:
                raise ValueError("grad_w needs the forward's rate (film_wattn_forward_into(..., rate=True))")
            continue
        if tuple(t.shape) != wshape or t.dtype != torch.float32:
            raise ValueError(f"{name} must be {wshape} float32, got {tuple(t.shape)} {t.dtype}")
    if grad_x_base is not None:
        _require_device(grad_x_base)
    w, wst = _wmean_weights(w, n, H, W)
    if not (need_dx or need_dgb or need_dw):
        return None, None, None
    attn = attn.contiguous()
    rate = rate.contiguous() if rate is not None and need_dw else None
    dtype = x.dtype
    if grad_out.dtype != dtype:
        grad_out = grad_out.to(dtype)
    grad_out, gs = _as_node_major(grad_out)
    x, xs = _as_node_major(x)
    bs = 0
    if grad_x_base is not None and need_dx:
        if grad_x_base.dtype != dtype:
            grad_x_base = grad_x_base.to(dtype)
        grad_x_base, bs = _as_node_major(grad_x_base)
    else:
        grad_x_base = None
    dx = torch.empty((n, C, H, W), device=x.device, dtype=dtype) if need_dx else None
    dgb = torch.empty((csr.num_edges, C, 2), device=x.device, dtype=torch.float32) if need_dgb else None
    dw = torch.empty((n, H, W), device=x.device, dtype=torch.float32) if need_dw else None
    gb = _attn_gb(gb, csr, C)
    ga = _graph_args(gb, csr, C, H * W, flags)
    lib = _lib.load_library()
    work, nbytes = None, 0
    if need_dgb or (need_dw and heads > 1):  # the tiles' grad_gb partials, the heads' grad_w partials
        sizes = (1, csr.num_graphs, csr.max_nodes, csr.graph_kind, csr.num_nodes, csr.num_edges, C, H * W)
        nbytes = lib.mrp_film_wattn_workspace(*sizes) if heads == 1 else lib.mrp_film_wattn_workspace_mh(*sizes, heads)
        if nbytes > 0:
            work = torch.empty(((nbytes + 3) // 4,), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        tail = (_ptr(dx), (C * H * W) if dx is not None else 0, _ptr(grad_x_base), bs, _ptr(dgb), scale, _ptr(attn),
                _ptr(rate), _ptr(dw), H * W if dw is not None else 0, _ptr(work), nbytes, _stream(x.device))
        head = (FEATURE_DTYPES[dtype], _ptr(grad_out), gs, _ptr(x), xs, ga[0], _ptr(w), wst, *ga[1:])
        code = lib.mrp_film_wattn_bwd(*head, *tail) if heads == 1 else lib.mrp_film_wattn_bwd_mh(*head, heads, *tail)
    _lib.check(code, "mrp_film_wattn_bwd" if heads == 1 else "mrp_film_wattn_bwd_mh")
    PATH_COUNTS[("wattn_bwd_" if heads == 1 else "wattn_bwd_mh_") + _DTYPE_KEYS[dtype]] += 1
    return dx, dgb, dw


def _wattn_grads(ctx, grad_out, base):
    x, gb, w, attn, rate = ctx.saved_tensors
    need = ctx.needs_input_grad
    dx, dgb, dw = film_wattn_backward(grad_out, x, gb, w, attn, rate, ctx.csr, ctx.flags, need[0], need[1], need[2],
                                      grad_x_base=base if need[0] else None, scale=ctx.scale, heads=ctx.heads)
    if dgb is not None:
        dgb = dgb.view(gb.shape).to(gb.dtype)
    if dw is not None:
        dw = dw.view(w.shape)
    return dx, dgb, dw, None, None, None, None


class FilmWAttnFunction(torch.autograd.Function):
    """Autograd wrapper: forward = ``mrp_film_wattn_fwd``, backward = ``mrp_film_wattn_bwd`` with gradients for
    x, gb and w.  Returns (out, attn); attn is saved for the backward and is not differentiable; the rates are
    computed and saved only when w requires a gradient.  ``flags`` may be ``_lib.GB_LOGITS``."""

    @staticmethod
    def forward(ctx, x, gb, w, csr: GraphCSR, flags: int, scale, heads: int = 1):
        out = torch.empty(tuple(x.shape), device=x.device, dtype=x.dtype)
        attn, rate = film_wattn_forward_into(x, gb, w, csr, flags, out, scale, rate=ctx.needs_input_grad[2],
                                             heads=heads)
        ctx.save_for_backward(x, gb, w, attn, rate)
        ctx.csr, ctx.flags, ctx.scale, ctx.heads = csr, flags, scale, heads
        ctx.mark_non_differentiable(attn)
        return out, attn

    @staticmethod
    def backward(ctx, grad_out, _grad_attn):
        return _wattn_grads(ctx, grad_out, None)


def film_wattn(x: torch.Tensor, gb: torch.Tensor, w: torch.Tensor, csr: GraphCSR, logits: bool = False,
               scale: Optional[float] = None, return_weights: bool = False, heads: int = 1):
    """:func:`film_attn` over what was delivered: at every pixel the receiver attends over the in-neighbours
    whose map ``w`` is positive there, each softmax term weighted by the sender's confidence
    (``a_j ~ w[src e_j] exp(s_j)``); pixels nobody delivered to give 0, and a silent sender's features reach
    nothing.  Differentiable in x, gb and w (w's gradient includes the entries at w == 0: the one-sided
    derivative).

    x: (N, C, H, W) fp32, bf16 or fp16 on a ROCm device; gb: (E, 2C) or (E, C, 2) interleaved gamma/beta, or
    their pre-sigmoid logits with ``logits=True``; w: (N, H, W) or (N, 1, H, W) fp32 >= 0, each node's plane
    contiguous — the sender's map, indexed by source node; csr: ``RobotGraph.csr(device)``, every in-degree <=
    ``_lib.FILM_ATTN_DEGREE``.  With ``return_weights=True`` returns ``(out, attn)``, attn (E, H*W) fp32 by edge
    id, not differentiable.  ``heads=H`` > 1: as for :func:`film_attn`; the maps w are shared by the heads and
    w's gradient sums over them."""
    _check_attn_degree(csr)  # a host-side property of the graph: checked before anything touches a device
    heads = _check_heads(heads, x.shape[1] if x.dim() == 4 else 0)  # host-side too
    _check_x(x)
    out, attn = FilmWAttnFunction.apply(x, gb, w, csr, _lib.GB_LOGITS if logits else 0, scale, heads)
    return (out, attn) if return_weights else out


class FilmWAttnCatFunction(torch.autograd.Function):
    """``torch.cat((x, film_wattn(x, gb, w)), 1)``: the kernel writes the aggregate into the second half of the
    (N, 2C, H, W) buffer through its node stride, x is copied into the first half by torch; backward hands
    the kernel the second half of the incoming gradient as grad_out and the first half as grad_x's base."""

    @staticmethod
    def forward(ctx, x, gb, w, csr: GraphCSR, flags: int, scale, heads: int = 1):
        n, C, H, W = x.shape
        buf = torch.empty((n, 2 * C, H, W), device=x.device, dtype=x.dtype)
        attn, rate = film_wattn_forward_into(x, gb, w, csr, flags, buf[:, C:], scale, rate=ctx.needs_input_grad[2],
                                             heads=heads)
        buf[:, :C].copy_(x)
        ctx.save_for_backward(x, gb, w, attn, rate)
        ctx.csr, ctx.flags, ctx.scale, ctx.heads = csr, flags, scale, heads
        ctx.mark_non_differentiable(attn)
        return buf, attn

    @staticmethod
    def backward(ctx, grad_buf, _grad_attn):
        C = ctx.saved_tensors[0].shape[1]
        return _wattn_grads(ctx, grad_buf[:, C:], grad_buf[:, :C])


def film_wattn_cat(x: torch.Tensor, gb: torch.Tensor, w: torch.Tensor, csr: GraphCSR, logits: bool = False,
                   scale: Optional[float] = None, return_weights: bool = False, heads: int = 1):
    """``torch.cat((x, film_wattn(x, gb, w, csr, logits, scale, heads=heads)), dim=1)`` without a concatenation
    pass for the aggregate."""
    _check_attn_degree(csr)
    heads = _check_heads(heads, x.shape[1] if x.dim() == 4 else 0)  # host-side too
    _check_x(x)
    buf, attn = FilmWAttnCatFunction.apply(x, gb, w, csr, _lib.GB_LOGITS if logits else 0, scale, heads)
    return (buf, attn) if return_weights else buf


def film_wattn_residual(x: torch.Tensor, gb: torch.Tensor, w: torch.Tensor, csr: GraphCSR, logits: bool = False,
                        scale: Optional[float] = None, heads: int = 1) -> torch.Tensor:
    """``x + film_wattn(x, ...)`` (the sum by torch: no fused epilogue for this reducer)."""
    return x + film_wattn(x, gb, w, csr, logits, scale, heads=heads)


def film_wattn_mix(x: torch.Tensor, gb: torch.Tensor, w: torch.Tensor, csr: GraphCSR, x0: torch.Tensor, alpha: float,
                   logits: bool = False, scale: Optional[float] = None, heads: int = 1) -> torch.Tensor:
    """``(1 - alpha) * film_wattn(x, ...) + alpha * x0`` (by torch ops: no fused epilogue for this reducer)."""
    return (1.0 - float(alpha)) * film_wattn(x, gb, w, csr, logits, scale, heads=heads) + float(alpha) * x0


# ---------------------------------------------------------------------------------------------------------
# FP8 messages for the max and attention reducers, receiver side (``mrp_film_max_fwd_q``,
# ``mrp_film_attn_fwd_q``, ``mrp_film_wattn_fwd_q``).  A receiver holds its own features ``x`` at full precision
# and is handed its neighbours' maps as FP8 codes ``xq`` with scales ``xscale`` (and, for the gated fusion, their
# confidence maps ``w``).  The messages are formed from x^ = fl32(s * decode(q)), as in ``film_mean_q``; the
# attention's query is x[v] — a robot's own maps never cross the link — so query and messages are two tensors:
#
#     film_max_q(xq, s, ..., out_dtype=T)  == film_max(dequantize_features(xq, s), ...).to(T)     bit for bit
#     film_attn_q(x^, xq, s, ...)          == film_attn(x^, ...)   (x^ fp32), out and weights     bit for bit
#     film_attn_q(x_T, ...)                == film_attn_q(x_T.float(), ...).to(T), the same weights
#
# Inference ops, as ``film_mean_q`` is.  ``film_max_fq`` is the differentiable fake-quant route of the max on the
# existing kernels; there is no fake-quant attention: under the straight-through estimator the backward would
# read the query from x and the sources from x^, which the backward kernels (one tensor for both) cannot.
# ---------------------------------------------------------------------------------------------------------
def _q_inputs(name: str, xq: torch.Tensor, xscale: Optional[torch.Tensor], csr: GraphCSR, *others):
    """The host-side checks the FP8 receiver ops share (nothing here touches a device)."""
    if not isinstance(xq, torch.Tensor) or xq.dtype not in _QDTYPES:
        raise TypeError(f"xq must be float8_e4m3fn or float8_e5m2 (quantize_features), got "
                        f"{getattr(xq, 'dtype', type(xq))}")
    if xq.dim() != 4:
        raise ValueError(f"quantised features must be (N, C, H, W), got {tuple(xq.shape)}")
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (xscale,) + others):
        raise RuntimeError(f"mrp_gnn: {name} is an inference op and would drop the gradient of its inputs; "
                           "run it under torch.no_grad()"
                           + (", or train through film_max_fq (same forward bits)" if name == "film_max_q" else ""))
    n, C, H, W = xq.shape
    if n != csr.num_nodes:
        raise ValueError(f"xq has {n} nodes, graph has {csr.num_nodes}")
    _q_scale(xscale, n, C)  # its shape: a host-side check


def _q_device(xq: torch.Tensor, xscale: Optional[torch.Tensor]):
    """(xq NCHW, its node stride, scale (N, C) fp32 contiguous or None) for the kernel."""
    n, C, H, W = xq.shape
    _require_device(xq, xscale)
    xs = _dense_node_stride(xq)
    if xs is None:  # channels_last or otherwise strided codes: made NCHW-contiguous first
        xq = xq.contiguous()
        xs = C * H * W
    sc = _q_scale(xscale, n, C)
    if sc is not None:
        sc = sc.float().contiguous()
    return xq, xs, sc


def film_max_q_forward_into(xq: torch.Tensor, xscale: Optional[torch.Tensor], gb: torch.Tensor, csr: GraphCSR,
                            out: torch.Tensor, logits: bool = False) -> torch.Tensor:
    """:func:`film_max_q` into ``out`` (N, C, H, W) fp32 / bf16 / fp16 — which may be a strided view with a
    contiguous block per node, such as the second half of a ``torch.cat((h, g_h), 1)`` buffer."""
    _check_max_degree(csr)  # a host-side property of the graph: checked before anything touches a device
    _q_inputs("film_max_q", xq, xscale, csr, gb)
    n, C, H, W = xq.shape
    if out.dim() != 4 or tuple(out.shape) != (n, C, H, W):
        raise ValueError(f"out must be {(n, C, H, W)}, got {tuple(out.shape)}")
    if out.dtype not in FEATURE_DTYPES:
        raise TypeError(f"out must be float32, bfloat16 or float16 (FP8 outputs are not provided), got {out.dtype}")
    os_ = node_stride(out)
    if os_ is None:
        raise ValueError("out must have a contiguous C*H*W block per node")
    _require_device(out)
    xq, xs, sc = _q_device(xq, xscale)
    gb = _max_gb(gb, csr, C)
    name, code = _QDTYPES[xq.dtype]
    lib = _lib.load_library()
    with torch.cuda.device(xq.device):
        rc = lib.mrp_film_max_fwd_q(code, _ptr(xq), xs, _ptr(sc), FEATURE_DTYPES[out.dtype],
                                    *_graph_args(gb, csr, C, H * W, _lib.GB_LOGITS if logits else 0), _ptr(out), os_,
                                    _stream(xq.device))
    _lib.check(rc, "mrp_film_max_fwd_q")
    PATH_COUNTS["max_fwd_q_" + name] += 1
    return out


def film_max_q(xq: torch.Tensor, xscale: Optional[torch.Tensor], gb: torch.Tensor, csr: GraphCSR,
               logits: bool = False, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """:func:`film_max` of FP8 messages, read natively (``mrp_film_max_fwd_q``).

    xq: (N, C, H, W) ``torch.float8_e4m3fn`` / ``torch.float8_e5m2`` codes; xscale: their fp32 scales, (N,),
    (N, 1) or (N, C) (``quantize_features``), or None; gb / csr / logits as :func:`film_max`.  Returns the
    aggregate in ``out_dtype`` (fp32, bf16 or fp16): bit-equal to ``film_max(dequantize_features(xq, xscale),
    ...)`` cast once.  An inference op: under grad mode with an input that requires grad it raises
    (:func:`film_max_fq` is the differentiable route)."""
    if isinstance(xq, torch.Tensor) and xq.dim() != 4:
        raise ValueError(f"quantised features must be (N, C, H, W), got {tuple(xq.shape)}")
    if out_dtype not in FEATURE_DTYPES:
        raise TypeError(f"out_dtype must be float32, bfloat16 or float16, got {out_dtype}")
    if not isinstance(xq, torch.Tensor) or xq.dtype not in _QDTYPES:
        raise TypeError(f"xq must be float8_e4m3fn or float8_e5m2 (quantize_features), got "
                        f"{getattr(xq, 'dtype', type(xq))}")
    out = torch.empty(xq.shape, device=xq.device, dtype=out_dtype)
    return film_max_q_forward_into(xq, xscale, gb, csr, out, logits)


def film_max_fq(x: torch.Tensor, gb: torch.Tensor, csr: GraphCSR, fmt: str = "e4m3", per: str = "channel",
                logits: bool = False) -> torch.Tensor:
    """The differentiable fake-quant route of :func:`film_max_q`, on the existing kernels: x is quantised
    (``quantize_features``), x^ formed in fp32 (``dequantize_features``) with a straight-through estimator (the
    gradient reaches x as if x^ = x), and the fp32 ``FilmMaxFunction`` run on it; the result is cast to
    ``x.dtype``.  Its forward bits equal ``film_max_q(*quantize_features(x, fmt, per), ..., out_dtype=x.dtype)``."""
    _check_max_degree(csr)
    _check_x(x)
    xq, s = quantize_features(x, fmt, per)
    xh = dequantize_features(xq, s)
    if torch.is_grad_enabled() and x.requires_grad:
        xh = _StraightThrough.apply(x, xh)
    return FilmMaxFunction.apply(xh, gb, csr, _lib.GB_LOGITS if logits else 0).to(x.dtype)


def _attn_q_forward_into(name: str, x, xq, xscale, gb, w, csr: GraphCSR, out, logits, scale, heads, attn, rate):
    """The forward behind film_attn_q (w None) and film_wattn_q; returns (attn, rate)."""
    _check_attn_degree(csr)  # a host-side property of the graph: checked before anything touches a device
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype not in FEATURE_DTYPES:
        raise ValueError("the receiver's own features x must be (N, C, H, W) float32, bfloat16 or float16")
    _q_inputs(name, xq, xscale, csr, x, gb, w)
    n, C, H, W = xq.shape
    if tuple(x.shape) != (n, C, H, W):
        raise ValueError(f"x must have the messages' shape {(n, C, H, W)}, got {tuple(x.shape)}")
    heads = _check_heads(heads, C)
    scale = _attn_scale(scale, C // heads)
    _require_device(x, out, attn, rate if isinstance(rate, torch.Tensor) else None)
    xq, xs, sc = _q_device(xq, xscale)
    x, qs = _as_node_major(x)  # a channels_last x is copied to NCHW here
    os_ = node_stride(out)
    if os_ is None or tuple(out.shape) != (n, C, H, W) or out.dtype != x.dtype:
        raise ValueError(f"out must be {(n, C, H, W)} {x.dtype} with a contiguous block per node")
    if w is not None:
        w, wst = _wmean_weights(w, n, H, W)
    gb = _attn_gb(gb, csr, C)
    wshape = _weights_shape(csr, H * W, heads)
    bufs = []
    for what, t in (("attn", attn), ("rate", rate)):
        if t is None or t is False:
            t = None if what == "rate" else torch.empty(wshape, device=x.device, dtype=torch.float32)
        elif t is True:
            t = torch.empty(wshape, device=x.device, dtype=torch.float32)
        elif tuple(t.shape) != wshape or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous {wshape} float32 tensor")
        bufs.append(t)
    attn, rate = bufs
    if w is None:
        rate = None
    fname, code = _QDTYPES[xq.dtype]
    lib = _lib.load_library()
    ga = _graph_args(gb, csr, C, H * W, _lib.GB_LOGITS if logits else 0)
    head = (code, _ptr(xq), xs, _ptr(sc), FEATURE_DTYPES[x.dtype], _ptr(x), qs, ga[0])
    with torch.cuda.device(x.device):
        if w is None:
            rc = lib.mrp_film_attn_fwd_q(*head, *ga[1:], heads, _ptr(out), os_, scale, _ptr(attn), None, 0,
                                         _stream(x.device))
        else:
            rc = lib.mrp_film_wattn_fwd_q(*head, _ptr(w), wst, *ga[1:], heads, _ptr(out), os_, scale, _ptr(attn),
                                          _ptr(rate), None, 0, _stream(x.device))
    _lib.check(rc, "mrp_film_attn_fwd_q" if w is None else "mrp_film_wattn_fwd_q")
    PATH_COUNTS[("attn" if w is None else "wattn") + ("_fwd_q_" if heads == 1 else "_fwd_q_mh_") + fname] += 1
    return attn, rate


def film_attn_q_forward_into(x: torch.Tensor, xq: torch.Tensor, xscale: Optional[torch.Tensor], gb: torch.Tensor,
                             csr: GraphCSR, out: torch.Tensor, logits: bool = False, scale: Optional[float] = None,
                             heads: int = 1, attn: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`film_attn_q` into ``out`` (N, C, H, W) of x's dtype — which may be a strided view such as the second
    half of a ``torch.cat((h, g_h), 1)`` buffer; returns the weights (written into ``attn`` if given)."""
    return _attn_q_forward_into("film_attn_q", x, xq, xscale, gb, None, csr, out, logits, scale, heads, attn, None)[0]


def film_attn_q(x: torch.Tensor, xq: torch.Tensor, xscale: Optional[torch.Tensor], gb: torch.Tensor, csr: GraphCSR,
                logits: bool = False, scale: Optional[float] = None, heads: int = 1, return_weights: bool = False):
    """:func:`film_attn` on the receiver's side of an FP8 link (``mrp_film_attn_fwd_q``): the messages
    ``gamma_e * x^[src] + beta_e`` are formed from the codes ``xq`` (N, C, H, W) ``torch.float8_e4m3fn`` /
    ``torch.float8_e5m2`` and their scales ``xscale`` ((N,), (N, 1), (N, C) or None), and scored by the receiver's
    own, unquantised features ``x`` (N, C, H, W) fp32, bf16 or fp16, whose dtype is the output's.  gb / csr /
    logits / scale / heads / return_weights as :func:`film_attn`.  Row v of ``x`` is read as v's query only: it
    is nobody's message.  An inference op: under grad mode with an input that requires grad it raises."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype not in FEATURE_DTYPES:
        raise ValueError("the receiver's own features x must be (N, C, H, W) float32, bfloat16 or float16")
    out = torch.empty(tuple(x.shape), device=x.device, dtype=x.dtype)
    attn = film_attn_q_forward_into(x, xq, xscale, gb, csr, out, logits, scale, heads)
    return (out, attn) if return_weights else out


def film_wattn_q_forward_into(x: torch.Tensor, xq: torch.Tensor, xscale: Optional[torch.Tensor], gb: torch.Tensor,
                              w: torch.Tensor, csr: GraphCSR, out: torch.Tensor, logits: bool = False,
                              scale: Optional[float] = None, heads: int = 1, attn: Optional[torch.Tensor] = None,
                              rate=False):
    """:func:`film_wattn_q` into ``out`` (as :func:`film_attn_q_forward_into`); returns ``(attn, rate)``, rate
    (the softmax's response to each sender's weight) only with ``rate=True`` or a tensor to write into."""
    if w is None:
        raise ValueError("film_wattn_q needs the sender maps w (N, H, W)")
    return _attn_q_forward_into("film_wattn_q", x, xq, xscale, gb, w, csr, out, logits, scale, heads, attn, rate)


def film_wattn_q(x: torch.Tensor, xq: torch.Tensor, xscale: Optional[torch.Tensor], gb: torch.Tensor,
                 w: torch.Tensor, csr: GraphCSR, logits: bool = False, scale: Optional[float] = None, heads: int = 1,
                 return_weights: bool = False):
    """:func:`film_wattn` on the receiver's side of an FP8 link (``mrp_film_wattn_fwd_q``): :func:`film_attn_q`
    gated and weighted by the received sender maps ``w`` (N, H, W) fp32 >= 0.  A sender that is silent at a
    pixel is never read there, whatever its codes.  With ``w == 1`` it gives :func:`film_attn_q`'s bits."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype not in FEATURE_DTYPES:
        raise ValueError("the receiver's own features x must be (N, C, H, W) float32, bfloat16 or float16")
    out = torch.empty(tuple(x.shape), device=x.device, dtype=x.dtype)
    attn, _ = film_wattn_q_forward_into(x, xq, xscale, gb, w, csr, out, logits, scale, heads)
    return (out, attn) if return_weights else out
