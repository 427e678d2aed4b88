// film_max_fwd_q.hip — FP8 messages for the max-pooled FiLM aggregation: launcher and C ABI (mrp_film_max_fwd_q).
// film_max_fwd's plan with x as 1-byte codes (film_max_fwd with TX = q8_t).  Kernels and design notes:
// film_max_kernels.hpp.
#include "film_max_kernels.hpp"
#include "film_mean_fwd_launch.hpp"

using namespace mrp_host;

namespace {

template <typename T>
hipError_t launch_max_fwd_q(const MaxArgs& m, const Geometry& g, int bucket, hipStream_t st) {
  const dim3 grid((unsigned)g.grid), block(g.threads);
#define MRP_MAX_FWD_Q(NT, VEC) hipLaunchKernelGGL((mrp::film_max_fwd<NT, VEC, T, mrp::q8_t>), grid, block, g.lds, st, m)
#define MRP_MAX_FWD_Q_NT(NT)                       \
  do {                                             \
    if (g.vec == 4)                                \
      MRP_MAX_FWD_Q(NT, 4);                        \
    else if (g.vec == 1)                           \
      MRP_MAX_FWD_Q(NT, 1);                        \
    else if constexpr (sizeof(T) == 2 && NT <= 8)  \
      MRP_MAX_FWD_Q(NT, 8);                        \
    else                                           \
      return hipErrorInvalidValue;                 \
  } while (0)
  if (bucket == 4)
    MRP_MAX_FWD_Q_NT(4);
  else if (bucket == 8)
    MRP_MAX_FWD_Q_NT(8);
  else
    MRP_MAX_FWD_Q_NT(16);
#undef MRP_MAX_FWD_Q_NT
#undef MRP_MAX_FWD_Q
  return hipGetLastError();
}

}  // namespace

extern "C" int mrp_film_max_fwd_q(int32_t qdtype, const void* xq, int64_t xq_node_stride, const float* x_scale,
                                  int32_t out_dtype, const float* gb, const int32_t* indptr, const int32_t* src,
                                  const int32_t* eid, const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                                  int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P,
                                  int32_t flags, void* out, int64_t out_node_stride, void* stream) {
  if (qdtype != MRP_QDTYPE_E4M3 && qdtype != MRP_QDTYPE_E5M2) return hipErrorInvalidValue;
  if (out_dtype != MRP_DTYPE_F32 && out_dtype != MRP_DTYPE_BF16 && out_dtype != MRP_DTYPE_F16)
    return hipErrorInvalidValue;
  if (flags != 0 && flags != MRP_AGG_GB_LOGITS) return hipErrorInvalidValue;
  if (!common_args_ok(indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P,
                      MRP_AGG_FILM_MEAN))
    return hipErrorInvalidValue;
  const int32_t kdeg = MRP_GRAPH_IS_REGULAR(graph_kind) ? MRP_GRAPH_REGULAR_K(graph_kind) : 0;
  if (kdeg > MRP_FILM_MAX_DEGREE) return hipErrorInvalidValue;
  if (num_graphs == 0 || num_nodes == 0 || max_nodes == 0 || C == 0 || P == 0) return hipSuccess;
  const int64_t plane = (int64_t)C * P;
  if (xq == nullptr || out == nullptr || xq_node_stride < plane || out_node_stride < plane)
    return hipErrorInvalidValue;
  if (num_edges > 0 && gb == nullptr) return hipErrorInvalidValue;
  const size_t elem = out_dtype == MRP_DTYPE_F32 ? 4 : 2;
  // the widest slice (elements) for which the codes (1 byte) and out (elem bytes) are both aligned: 8 (16-bit
  // outputs, <= 8 nodes: an 8-byte load, a 16-byte store), 4, else single elements
  SliceCheck scx, sco;
  scx.strides = sco.strides = P;
  scx.add(xq, xq_node_stride);
  sco.add(out, out_node_stride);
  int vec = 1;
  if (elem == 2 && max_nodes <= 8 && scx.ok(8, 1) && sco.ok(8, elem))
    vec = 8;
  else if (scx.ok(4, 1) && sco.ok(4, elem))
    vec = 4;
  const Tuning& tu = tuning();
  Geometry g = make_geometry(C, P, vec, tu.fwd_lo, tu.fwd_hi, tu.fwd_cap);
  const int bucket = max_bucket(max_nodes);
  g.lds = lds_max(bucket, g.cpb);
  const int32_t pv = P / g.vec;
  g.psplit = graph_kind == MRP_GRAPH_COMPLETE ? (pv + g.lpc - 1) / g.lpc : 1;
  g.grid = (int64_t)num_graphs * g.ncb * g.psplit;
  if (g.grid > 0x7fffffff || g.lds > kMaxDynamicLds) return hipErrorInvalidValue;
  MaxArgs m = {};
  AggArgs& a = m.a;
  a.x = xq;
  a.xs = xq_node_stride;
  a.xscale = x_scale;
  a.qfmt = qdtype;
  a.gb = gb;
  a.indptr = indptr;
  a.src = src;
  a.eid = eid;
  a.goff = graph_off;
  a.out = out;
  a.os = out_node_stride;
  a.C = C;
  a.P = P;
  a.PV = pv;
  a.lpc = g.lpc;
  a.cpb = g.cpb;
  a.ncb = g.ncb;
  a.logits = flags ? 1 : 0;
  a.psplit = g.psplit;
  a.kdeg = kdeg;
  a.nmax = max_nodes;
  m.complete = graph_kind == MRP_GRAPH_COMPLETE;
  m.nvb = 1;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (out_dtype) {
    case MRP_DTYPE_F32: return launch_max_fwd_q<float>(m, g, bucket, st);
    case MRP_DTYPE_BF16: return launch_max_fwd_q<mrp::bf16_t>(m, g, bucket, st);
    default: return launch_max_fwd_q<mrp::f16_t>(m, g, bucket, st);
  }
}
