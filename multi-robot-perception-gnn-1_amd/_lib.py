"""ctypes binding of the HIP C-ABI library ``lib/libmrp_gnn.so`` (declared in ``include/mrp_gnn.h``).

The library is built in-tree by ``__graft_entry__.build()`` (or ``python -m mrp_gnn_amd.build``).
There is deliberately no CPU fallback: if the shared object is missing, every compute call
raises.  torch is imported first so that the process already holds torch's HIP runtime
(soname ``libamdhip64.so.7``) and the library binds to that same runtime, making torch's
streams and device pointers valid inside it.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  (must be loaded before the HIP library, see module docstring)

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "lib", "libmrp_gnn.so")

#: Every symbol ``include/mrp_gnn.h`` declares.
EXPORTED_SYMBOLS = (
    "mrp_film_mean_fwd",
    "mrp_film_mean_cat_fwd",
    "mrp_film_mean_bwd",
    "mrp_film_mean_fwd_ex",
    "mrp_film_mean_bwd_ex",
    "mrp_film_mean_fwd_t",
    "mrp_film_mean_bwd_t",
    "mrp_film_mean_fwd_plan",
    "mrp_film_mean_bwd_plan",
    "mrp_film_mean_fwd_q",
    "mrp_film_mean_fwd_q_plan",
    "mrp_film_max_fwd_q",
    "mrp_film_attn_fwd_q",
    "mrp_film_wattn_fwd_q",
    "mrp_film_mean_bwd_workspace",
    "mrp_film_mean_fwd_cl",
    "mrp_film_mean_bwd_cl",
    "mrp_film_mean_bwd_cl_workspace",
    "mrp_film_max_fwd",
    "mrp_film_max_bwd",
    "mrp_film_attn_fwd",
    "mrp_film_attn_bwd",
    "mrp_film_attn_workspace",
    "mrp_film_wattn_fwd",
    "mrp_film_wattn_bwd",
    "mrp_film_wattn_workspace",
    "mrp_film_attn_fwd_mh",
    "mrp_film_attn_bwd_mh",
    "mrp_film_attn_workspace_mh",
    "mrp_film_wattn_fwd_mh",
    "mrp_film_wattn_bwd_mh",
    "mrp_film_wattn_workspace_mh",
    "mrp_film_wmean_fwd",
    "mrp_film_wmean_bwd",
    "mrp_film_wmean_workspace",
    "mrp_compress_fwd",
    "mrp_compress_weight_transpose",
    "mrp_compress_bwd_data",
    "mrp_compress_bwd_weight_workspace",
    "mrp_compress_bwd_weight",
    "mrp_compress_split_pack_bytes",
    "mrp_compress_split_pack",
    "mrp_compress_fwd_split",
    "mrp_compress_bwd_data_split",
    "mrp_compress_bwd_weight_split_workspace",
    "mrp_compress_bwd_weight_split",
    "mrp_compress_fwd_split_p",
    "mrp_compress_bwd_data_split_p",
    "mrp_compress_bwd_weight_split_p",
    "mrp_compress_pack_t_bytes",
    "mrp_compress_pack_t",
    "mrp_compress_fwd_t",
    "mrp_compress_bwd_data_t",
    "mrp_compress_bwd_weight_t_workspace",
    "mrp_compress_bwd_weight_t",
    "mrp_compress_fwd_cl",
    "mrp_compress_bwd_data_cl",
    "mrp_compress_bwd_weight_cl_workspace",
    "mrp_compress_bwd_weight_cl",
    "mrp_compress_fwd_split_cl",
    "mrp_compress_bwd_data_split_cl",
    "mrp_compress_bwd_weight_split_cl_workspace",
    "mrp_compress_bwd_weight_split_cl",
    "mrp_edge_hidden_fwd",
    "mrp_edge_logits_fwd",
    "mrp_edge_encoder_pack_bytes",
    "mrp_edge_encoder_pack",
    "mrp_edge_encoder_fwd_split",
    "mrp_edge_encoder_fwd_split_train",
    "mrp_edge_encoder_bwd_workspace",
    "mrp_edge_encoder_bwd",
    "mrp_edge_encoder_bwd_prep",
    "mrp_edge_encoder_bwd_split_workspace",
    "mrp_edge_encoder_bwd_split",
    "mrp_edge_encoder_bwd_fused_workspace",
    "mrp_edge_encoder_bwd_fused",
    "mrp_edge_encoder_bwd_t_workspace",
    "mrp_edge_encoder_bwd_t",
    "mrp_edge_encoder_bwd_pose_workspace",
    "mrp_edge_encoder_bwd_pose",
    "mrp_frame_graph_build",
    "mrp_frame_graph_build_range",
    "mrp_frame_graph_build_range_workspace",
    "mrp_stream_copy",
    "mrp_stream_join",
    "mrp_tuning_set",
    "mrp_abi_version",
    "mrp_error_string",
)
ABI_VERSION = 22
MAX_NODES = 16
FILM_MAX_DEGREE = 16  # MRP_FILM_MAX_DEGREE: largest in-degree of the max-pooled aggregation
FILM_ATTN_DEGREE = 16  # MRP_FILM_ATTN_DEGREE: largest in-degree of the attention-pooled aggregation
WAGG_MEAN = 0  # enum mrp_wagg_mode: the confidence-weighted aggregation's normalised / plain weighted sum
WAGG_SUM = 1

HIP_ERROR_NOT_SUPPORTED = 801  # hipErrorNotSupported: a fused path declines this shape

MODE_FILM_MEAN = 0
MODE_FILM_SUM = 1
MODE_COPY_MEAN = 2
GB_LOGITS = 0x100  # mode flag: gb holds pre-sigmoid logits
DTYPE_F32 = 0  # enum mrp_dtype: the feature storage type of the typed entry points
DTYPE_BF16 = 1
DTYPE_F16 = 2
QDTYPE_E4M3 = 0  # enum mrp_qdtype: the FP8 format of mrp_film_mean_fwd_q's messages (OCP, never FNUZ)
QDTYPE_E5M2 = 1
GRAPH_CSR = 0
GRAPH_COMPLETE = 1
GRAPH_SIMPLE = 3  # CSR arrays in which no two entries share a (source, destination) pair


MAX_REGULAR_K = 8  # largest in-degree the per-edge-slot backward handles


def graph_regular(k: int) -> int:
    """MRP_GRAPH_REGULAR(k): every node has exactly k in-edges."""
    return (k << 8) | 2
MODES = {"film_mean": MODE_FILM_MEAN, "film_sum": MODE_FILM_SUM, "copy_mean": MODE_COPY_MEAN}

class Epilogue(ctypes.Structure):
    """``mrp_agg_epilogue`` (include/mrp_gnn.h): out = agg_scale*a + self_scale*x[v] + x0_scale*x0[v],
    plus an optional copy of x[v] (the first half of a concatenation buffer)."""

    _fields_ = [("agg_scale", ctypes.c_float), ("self_scale", ctypes.c_float), ("x0", ctypes.c_void_p),
                ("x0_node_stride", ctypes.c_int64), ("x0_scale", ctypes.c_float), ("xcopy", ctypes.c_void_p),
                ("xcopy_node_stride", ctypes.c_int64)]


#: enum mrp_agg_kernel: the kernel a launch plan names
AGG_KERNELS = ("none", "film_fwd", "film_fwd_regular", "film_bwd_fused", "film_bwd_dx_gram", "film_bwd_regular",
               "film_bwd_mfma")


class AggPlan(ctypes.Structure):
    """``mrp_agg_plan``: what ``mrp_film_mean_fwd_plan`` / ``mrp_film_mean_bwd_plan`` report (no GPU call)."""

    _fields_ = [("kernel", ctypes.c_int32), ("vec", ctypes.c_int32), ("lpc", ctypes.c_int32),
                ("cpb", ctypes.c_int32), ("threads", ctypes.c_int32), ("psplit", ctypes.c_int32),
                ("ncb", ctypes.c_int32), ("pre2", ctypes.c_int32), ("grid", ctypes.c_int64),
                ("lds_bytes", ctypes.c_int64)]

    @property
    def kernel_name(self) -> str:
        return AGG_KERNELS[self.kernel]


class EpilogueCl(ctypes.Structure):
    """``mrp_agg_epilogue_cl``: ``Epilogue`` plus the pixel strides of x0 and xcopy (pixel-major tensors)."""

    _fields_ = Epilogue._fields_ + [("x0_pixel_stride", ctypes.c_int64), ("xcopy_pixel_stride", ctypes.c_int64)]


_lock = threading.Lock()
_lib = None

_P = ctypes.c_void_p
_I32 = ctypes.c_int32
_I64 = ctypes.c_int64


def _declare(lib: ctypes.CDLL) -> None:
    graph = [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32]  # indptr..mode
    lib.mrp_film_mean_fwd.argtypes = [_P, _I64, _P] + graph + [_P, _I64, _P]
    lib.mrp_film_mean_fwd.restype = ctypes.c_int
    lib.mrp_film_mean_cat_fwd.argtypes = [_P, _I64, _P] + graph + [_P, _I64, _P]
    lib.mrp_film_mean_cat_fwd.restype = ctypes.c_int
    lib.mrp_film_mean_bwd.argtypes = [_P, _I64, _P, _I64, _P] + graph + [_P, _I64, _P, _I64, _P, _P]
    lib.mrp_film_mean_bwd.restype = ctypes.c_int
    ep = ctypes.POINTER(Epilogue)
    lib.mrp_film_mean_fwd_ex.argtypes = [_P, _I64, _P] + graph + [_P, _I64, ep, _P]
    lib.mrp_film_mean_fwd_ex.restype = ctypes.c_int
    lib.mrp_film_mean_bwd_ex.argtypes = [_P, _I64, _P, _I64, _P] + graph + [_P, _I64, _P, _I64, _P, ep, _P, _I64, _P]
    lib.mrp_film_mean_bwd_ex.restype = ctypes.c_int
    lib.mrp_film_mean_fwd_t.argtypes = [_I32, _P, _I64, _P] + graph + [_P, _I64, ep, _P]
    lib.mrp_film_mean_fwd_t.restype = ctypes.c_int
    lib.mrp_film_mean_bwd_t.argtypes = [_I32, _P, _I64, _P, _I64, _P] + graph + [_P, _I64, _P, _I64, _P, ep, _P]
    lib.mrp_film_mean_bwd_t.restype = ctypes.c_int
    plan = ctypes.POINTER(AggPlan)
    lib.mrp_film_mean_fwd_plan.argtypes = [_I32, _P, _I64, _P] + graph + [_P, _I64, ep, plan]
    lib.mrp_film_mean_fwd_plan.restype = ctypes.c_int
    lib.mrp_film_mean_bwd_plan.argtypes = [_I32, _P, _I64, _P, _I64, _P] + graph + [_P, _I64, _P, _I64, _P, ep, plan]
    lib.mrp_film_mean_bwd_plan.restype = ctypes.c_int
    # FP8 messages: qdtype, xq, stride, x_scale, out_dtype, then the typed forward's tail
    lib.mrp_film_mean_fwd_q.argtypes = [_I32, _P, _I64, _P, _I32, _P] + graph + [_P, _I64, ep, _P]
    lib.mrp_film_mean_fwd_q.restype = ctypes.c_int
    lib.mrp_film_mean_fwd_q_plan.argtypes = [_I32, _P, _I64, _P, _I32, _P] + graph + [_P, _I64, ep, plan]
    lib.mrp_film_mean_fwd_q_plan.restype = ctypes.c_int
    lib.mrp_film_mean_bwd_workspace.argtypes = [_I32, _I32, _I32, _I32, _I32]
    lib.mrp_film_mean_bwd_workspace.restype = ctypes.c_int64
    epc = ctypes.POINTER(EpilogueCl)
    lib.mrp_film_mean_fwd_cl.argtypes = [_I32, _P, _I64, _I64, _P] + graph + [_P, _I64, _I64, epc, _P]
    lib.mrp_film_mean_fwd_cl.restype = ctypes.c_int
    lib.mrp_film_mean_bwd_cl.argtypes = ([_I32, _P, _I64, _I64, _P, _I64, _I64, _P] + graph +
                                         [_P, _I64, _I64, _P, _I64, _I64, _P, epc, _P, _I64, _P])
    lib.mrp_film_mean_bwd_cl.restype = ctypes.c_int
    lib.mrp_film_mean_bwd_cl_workspace.argtypes = [_I32, _I32, _I32, _I32, _I32, _I32, _I32]
    lib.mrp_film_mean_bwd_cl_workspace.restype = ctypes.c_int64
    # the max-pooled aggregation: `flags` (0 or GB_LOGITS) sits where the mean's `mode` does
    lib.mrp_film_max_fwd.argtypes = [_I32, _P, _I64, _P] + graph + [_P, _I64, _P]
    lib.mrp_film_max_fwd.restype = ctypes.c_int
    lib.mrp_film_max_bwd.argtypes = [_I32, _P, _I64, _P, _I64, _P] + graph + [_P, _I64, _P, _I64, _P, _P]
    lib.mrp_film_max_bwd.restype = ctypes.c_int
    # the attention-pooled aggregation: film_max's lists plus scale, attn, workspace, workspace_bytes
    tail = [ctypes.c_float, _P, _P, _I64, _P]
    lib.mrp_film_attn_fwd.argtypes = lib.mrp_film_max_fwd.argtypes[:-1] + tail
    lib.mrp_film_attn_fwd.restype = ctypes.c_int
    lib.mrp_film_attn_bwd.argtypes = lib.mrp_film_max_bwd.argtypes[:-1] + tail
    lib.mrp_film_attn_bwd.restype = ctypes.c_int
    lib.mrp_film_attn_workspace.argtypes = [_I32] * 8
    lib.mrp_film_attn_workspace.restype = ctypes.c_int64
    # the confidence-gated attention fusion: film_attn's lists with (w, w_node_stride) after gb; the forward adds
    # rate after attn, the backward rate, grad_w, gw_node_stride
    fa, ba = lib.mrp_film_attn_fwd.argtypes, lib.mrp_film_attn_bwd.argtypes
    lib.mrp_film_wattn_fwd.argtypes = fa[:4] + [_P, _I64] + fa[4:-3] + [_P] + fa[-3:]
    lib.mrp_film_wattn_fwd.restype = ctypes.c_int
    lib.mrp_film_wattn_bwd.argtypes = ba[:6] + [_P, _I64] + ba[6:-3] + [_P, _P, _I64] + ba[-3:]
    lib.mrp_film_wattn_bwd.restype = ctypes.c_int
    lib.mrp_film_wattn_workspace.argtypes = [_I32] * 8
    lib.mrp_film_wattn_workspace.restype = ctypes.c_int64
    # the multi-head forms: `heads` follows `C, P, flags` (`C, P` in the workspace queries)
    wf, wb = lib.mrp_film_wattn_fwd.argtypes, lib.mrp_film_wattn_bwd.argtypes
    for name, args, at in (("mrp_film_attn_fwd_mh", fa, 16), ("mrp_film_attn_bwd_mh", ba, 18),
                           ("mrp_film_wattn_fwd_mh", wf, 18), ("mrp_film_wattn_bwd_mh", wb, 20)):
        fn = getattr(lib, name)
        fn.argtypes = args[:at] + [_I32] + args[at:]
        fn.restype = ctypes.c_int
    # FP8 messages, receiver side: qdtype, xq, stride, x_scale, then out_dtype (max) or dtype, query, stride
    # (attention), then the typed entry's list from gb on (the attention forms: the multi-head one's)
    lib.mrp_film_max_fwd_q.argtypes = [_I32, _P, _I64, _P, _I32] + lib.mrp_film_max_fwd.argtypes[3:]
    lib.mrp_film_max_fwd_q.restype = ctypes.c_int
    lib.mrp_film_attn_fwd_q.argtypes = [_I32, _P, _I64, _P, _I32, _P, _I64] + lib.mrp_film_attn_fwd_mh.argtypes[3:]
    lib.mrp_film_attn_fwd_q.restype = ctypes.c_int
    lib.mrp_film_wattn_fwd_q.argtypes = [_I32, _P, _I64, _P, _I32, _P, _I64] + lib.mrp_film_wattn_fwd_mh.argtypes[3:]
    lib.mrp_film_wattn_fwd_q.restype = ctypes.c_int
    lib.mrp_film_attn_workspace_mh.argtypes = [_I32] * 9
    lib.mrp_film_attn_workspace_mh.restype = ctypes.c_int64
    lib.mrp_film_wattn_workspace_mh.argtypes = [_I32] * 9
    lib.mrp_film_wattn_workspace_mh.restype = ctypes.c_int64
    # the confidence-weighted aggregation: (w, w_node_stride) follow gb, wagg follows flags; the backward
    # ends with grad_w, gw_node_stride, workspace, workspace_bytes, stream
    lib.mrp_film_wmean_fwd.argtypes = [_I32, _P, _I64, _P, _P, _I64] + graph[:-1] + [_I32, _I32, _P, _I64, _P]
    lib.mrp_film_wmean_fwd.restype = ctypes.c_int
    lib.mrp_film_wmean_bwd.argtypes = ([_I32, _P, _I64, _P, _I64, _P, _P, _I64] + graph[:-1] +
                                       [_I32, _I32, _P, _I64, _P, _I64, _P, _P, _I64, _P, _I64, _P])
    lib.mrp_film_wmean_bwd.restype = ctypes.c_int
    lib.mrp_film_wmean_workspace.argtypes = [_I32] * 7
    lib.mrp_film_wmean_workspace.restype = ctypes.c_int64
    lib.mrp_tuning_set.argtypes = [ctypes.c_char_p, _I32]
    lib.mrp_tuning_set.restype = ctypes.c_int
    lib.mrp_compress_fwd.argtypes = [_P, _I64, _P, _I64, _I32, _I32, _I32, _P, _P, _P, _I64, _P]
    lib.mrp_compress_fwd.restype = ctypes.c_int
    lib.mrp_compress_weight_transpose.argtypes = [_P, _P, _I32, _P]
    lib.mrp_compress_weight_transpose.restype = ctypes.c_int
    lib.mrp_compress_bwd_data.argtypes = [_P, _I64, _I32, _I32, _I32, _P, _P, _I64, _P, _I64, _P]
    lib.mrp_compress_bwd_data.restype = ctypes.c_int
    lib.mrp_compress_bwd_weight_workspace.argtypes = [_I32, _I32, _I32, _I64]
    lib.mrp_compress_bwd_weight_workspace.restype = ctypes.c_int64
    lib.mrp_compress_bwd_weight.argtypes = [_P, _I64, _P, _I64, _P, _I64, _I32, _I32, _I32, _P, _P, _P, _I64, _P]
    lib.mrp_compress_bwd_weight.restype = ctypes.c_int
    lib.mrp_compress_split_pack_bytes.argtypes = [_I32, _I32]
    lib.mrp_compress_split_pack_bytes.restype = ctypes.c_int64
    lib.mrp_compress_split_pack.argtypes = [_P, _I64, _I32, _I32, _I32, _P, _P]
    lib.mrp_compress_split_pack.restype = ctypes.c_int
    lib.mrp_compress_fwd_split.argtypes = [_P, _I64, _P, _I64, _I32, _I32, _I32, _P, _P, _P, _I64, _P]
    lib.mrp_compress_fwd_split.restype = ctypes.c_int
    lib.mrp_compress_bwd_data_split.argtypes = [_P, _I64, _I32, _I32, _I32, _P, _P, _I64, _P, _I64, _P]
    lib.mrp_compress_bwd_data_split.restype = ctypes.c_int
    lib.mrp_compress_bwd_weight_split_workspace.argtypes = [_I32, _I32, _I32]
    lib.mrp_compress_bwd_weight_split_workspace.restype = ctypes.c_int64
    lib.mrp_compress_bwd_weight_split.argtypes = lib.mrp_compress_bwd_weight.argtypes
    lib.mrp_compress_bwd_weight_split.restype = ctypes.c_int
    # the same with a trailing part count (3 / 2 / 1 bf16 parts kept per operand) before the stream
    lib.mrp_compress_fwd_split_p.argtypes = lib.mrp_compress_fwd_split.argtypes[:-1] + [_I32, _P]
    lib.mrp_compress_fwd_split_p.restype = ctypes.c_int
    lib.mrp_compress_bwd_data_split_p.argtypes = lib.mrp_compress_bwd_data_split.argtypes[:-1] + [_I32, _P]
    lib.mrp_compress_bwd_data_split_p.restype = ctypes.c_int
    lib.mrp_compress_bwd_weight_split_p.argtypes = lib.mrp_compress_bwd_weight.argtypes[:-1] + [_I32, _P]
    lib.mrp_compress_bwd_weight_split_p.restype = ctypes.c_int
    lib.mrp_compress_pack_t_bytes.argtypes = [_I32, _I32]
    lib.mrp_compress_pack_t_bytes.restype = ctypes.c_int64
    lib.mrp_compress_pack_t.argtypes = [_I32] + lib.mrp_compress_split_pack.argtypes
    lib.mrp_compress_pack_t.restype = ctypes.c_int
    lib.mrp_compress_fwd_t.argtypes = [_I32] + lib.mrp_compress_fwd_split.argtypes
    lib.mrp_compress_fwd_t.restype = ctypes.c_int
    lib.mrp_compress_bwd_data_t.argtypes = [_I32] + lib.mrp_compress_bwd_data_split.argtypes
    lib.mrp_compress_bwd_data_t.restype = ctypes.c_int
    lib.mrp_compress_bwd_weight_t_workspace.argtypes = [_I32, _I32, _I32]
    lib.mrp_compress_bwd_weight_t_workspace.restype = ctypes.c_int64
    lib.mrp_compress_bwd_weight_t.argtypes = [_I32] + lib.mrp_compress_bwd_weight.argtypes
    lib.mrp_compress_bwd_weight_t.restype = ctypes.c_int
    t3 = [_P, _I64, _I64]  # a pixel-major tensor: pointer, node stride, pixel stride
    lib.mrp_compress_fwd_cl.argtypes = [_I32] + t3 + t3 + [_I32, _I32, _I32, _P, _P] + t3 + [_P]
    lib.mrp_compress_fwd_cl.restype = ctypes.c_int
    lib.mrp_compress_bwd_data_cl.argtypes = [_I32] + t3 + [_I32, _I32, _I32, _P] + t3 + t3 + [_P]
    lib.mrp_compress_bwd_data_cl.restype = ctypes.c_int
    lib.mrp_compress_bwd_weight_cl_workspace.argtypes = [_I32, _I32, _I32]
    lib.mrp_compress_bwd_weight_cl_workspace.restype = ctypes.c_int64
    lib.mrp_compress_bwd_weight_cl.argtypes = [_I32] + t3 + t3 + t3 + [_I32, _I32, _I32, _P, _P, _P, _I64, _P]
    lib.mrp_compress_bwd_weight_cl.restype = ctypes.c_int
    # the pixel-major fp32 forms: no dtype, `parts` before the stream
    lib.mrp_compress_fwd_split_cl.argtypes = lib.mrp_compress_fwd_cl.argtypes[1:-1] + [_I32, _P]
    lib.mrp_compress_fwd_split_cl.restype = ctypes.c_int
    lib.mrp_compress_bwd_data_split_cl.argtypes = lib.mrp_compress_bwd_data_cl.argtypes[1:-1] + [_I32, _P]
    lib.mrp_compress_bwd_data_split_cl.restype = ctypes.c_int
    lib.mrp_compress_bwd_weight_split_cl_workspace.argtypes = [_I32, _I32, _I32]
    lib.mrp_compress_bwd_weight_split_cl_workspace.restype = ctypes.c_int64
    lib.mrp_compress_bwd_weight_split_cl.argtypes = lib.mrp_compress_bwd_weight_cl.argtypes[1:-1] + [_I32, _P]
    lib.mrp_compress_bwd_weight_split_cl.restype = ctypes.c_int
    lib.mrp_edge_hidden_fwd.argtypes = [_P, _P, _P, _I32, _I32, _P, _P]
    lib.mrp_edge_hidden_fwd.restype = ctypes.c_int
    lib.mrp_edge_logits_fwd.argtypes = [_P, _I32, _I32, _P, _P, _P, _P]
    lib.mrp_edge_logits_fwd.restype = ctypes.c_int
    lib.mrp_edge_encoder_pack_bytes.argtypes = [_I32]
    lib.mrp_edge_encoder_pack_bytes.restype = ctypes.c_int64
    lib.mrp_edge_encoder_pack.argtypes = [_P, _P, _P, _I32, _P, _P]
    lib.mrp_edge_encoder_pack.restype = ctypes.c_int
    lib.mrp_edge_encoder_fwd_split.argtypes = [_P, _P, _P, _I32, _I32, _P, _P]
    lib.mrp_edge_encoder_fwd_split.restype = ctypes.c_int
    lib.mrp_edge_encoder_fwd_split_train.argtypes = [_P, _P, _P, _I32, _I32, _P, _P, _I64, _P]
    lib.mrp_edge_encoder_fwd_split_train.restype = ctypes.c_int
    lib.mrp_edge_encoder_bwd_prep.argtypes = [_P, _I32, _I32, _P, _I64, _P]
    lib.mrp_edge_encoder_bwd_prep.restype = ctypes.c_int
    lib.mrp_edge_encoder_bwd_split_workspace.argtypes = [_I32, _I32]
    lib.mrp_edge_encoder_bwd_split_workspace.restype = ctypes.c_int64
    lib.mrp_edge_encoder_bwd_split.argtypes = [_P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _I64, _P]
    lib.mrp_edge_encoder_bwd_split.restype = ctypes.c_int
    lib.mrp_edge_encoder_bwd_fused_workspace.argtypes = [_I32, _I32]
    lib.mrp_edge_encoder_bwd_fused_workspace.restype = ctypes.c_int64
    lib.mrp_edge_encoder_bwd_fused.argtypes = [_P, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _I64, _P]
    lib.mrp_edge_encoder_bwd_fused.restype = ctypes.c_int
    lib.mrp_edge_encoder_bwd_t_workspace.argtypes = [_I32, _I32]
    lib.mrp_edge_encoder_bwd_t_workspace.restype = ctypes.c_int64
    lib.mrp_edge_encoder_bwd_t.argtypes = [_P, _I64, _P, _I64, _P, _I32, _I32, _P, _P, _P, _I64, _P]
    lib.mrp_edge_encoder_bwd_t.restype = ctypes.c_int
    lib.mrp_edge_encoder_bwd_pose_workspace.argtypes = [_I32, _I32]
    lib.mrp_edge_encoder_bwd_pose_workspace.restype = ctypes.c_int64
    lib.mrp_edge_encoder_bwd_pose.argtypes = [_P, _I64, _P, _I64, _P, _I32, _I32, _P, _P, _I64, _P]
    lib.mrp_edge_encoder_bwd_pose.restype = ctypes.c_int
    lib.mrp_edge_encoder_bwd_workspace.argtypes = [_I32, _I32]
    lib.mrp_edge_encoder_bwd_workspace.restype = ctypes.c_int64
    lib.mrp_edge_encoder_bwd.argtypes = [_P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P]
    lib.mrp_edge_encoder_bwd.restype = ctypes.c_int
    lib.mrp_frame_graph_build.argtypes = [_P, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P]
    lib.mrp_frame_graph_build.restype = ctypes.c_int
    lib.mrp_frame_graph_build_range.argtypes = [_P, _P, _I32, _I32, _I32, ctypes.c_double, _P, _P, _P, _P, _P, _P,
                                                _I64, _P]
    lib.mrp_frame_graph_build_range.restype = ctypes.c_int
    lib.mrp_frame_graph_build_range_workspace.argtypes = [_I32, _I32]
    lib.mrp_frame_graph_build_range_workspace.restype = ctypes.c_int64
    lib.mrp_stream_copy.argtypes = [_P, _P, _I64, _P]
    lib.mrp_stream_copy.restype = ctypes.c_int
    lib.mrp_stream_join.argtypes = [_P, _P]
    lib.mrp_stream_join.restype = ctypes.c_int
    lib.mrp_abi_version.argtypes = []
    lib.mrp_abi_version.restype = ctypes.c_int
    lib.mrp_error_string.argtypes = [ctypes.c_int]
    lib.mrp_error_string.restype = ctypes.c_char_p


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load (once) and return the HIP library; raise if it has not been built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.isfile(path):
            raise RuntimeError(
                f"mrp_gnn: HIP library not found at {path}. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback for the aggregation kernels."
            )
        lib = ctypes.CDLL(path)
        _declare(lib)
        got = lib.mrp_abi_version()
        if got != ABI_VERSION:
            raise RuntimeError(f"mrp_gnn: ABI version mismatch: library {got}, bindings {ABI_VERSION}")
        _lib = lib
        return lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = load_library().mrp_error_string(code)
        text = msg.decode() if msg else "unknown error"
        raise RuntimeError(f"mrp_gnn: {what} failed with HIP error {code}: {text}")
