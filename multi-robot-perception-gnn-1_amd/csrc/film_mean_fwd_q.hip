// film_mean_fwd_q.hip — FP8 messages: the C ABI (mrp_film_mean_fwd_q, mrp_film_mean_fwd_q_plan), their
// planner and the fp32-output instantiations.  bf16 / fp16 outputs: film_mean_fwd_q_{bf16,f16}.hip.
// Kernels and design notes: film_mean_kernels.hpp (film_fwd / film_fwd_regular, TX = q8_t).
#include "film_mean_fwd_q_launch.hpp"

namespace mrp_host {

hipError_t dispatch_fwd_q_f32(int nt, bool complete, const AggArgs& a, const Geometry& g, hipStream_t st) {
  return dispatch_fwd_q<float>(nt, complete, a, g, st);
}

// Validation and launch plan of the FP8-message forward: the typed forward's planner (film_fwd_plan) with
// x as 1-byte elements, after the checks that are this entry point's own.  No GPU call.
static int film_fwd_q_plan(int32_t qdtype, const void* xq, int64_t x_node_stride, const float* x_scale,
                           int32_t out_dtype, const float* gb, const int32_t* indptr, const int32_t* src,
                           const int32_t* eid, const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                           int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P,
                           int32_t mode_flags, void* out, int64_t out_node_stride, const mrp_agg_epilogue* ep,
                           AggArgs& a, Geometry& g) {
  g = Geometry();
  if (qdtype != MRP_QDTYPE_E4M3 && qdtype != MRP_QDTYPE_E5M2) return hipErrorInvalidValue;
  if (out_dtype != MRP_DTYPE_F32 && out_dtype != MRP_DTYPE_BF16 && out_dtype != MRP_DTYPE_F16)
    return hipErrorInvalidValue;
  // a robot's own features never cross the link: no own-feature term can come from the codes
  if (ep != nullptr && (ep->self_scale != 0.f || ep->xcopy != nullptr)) return hipErrorInvalidValue;
  const int rc = film_fwd_plan(out_dtype == MRP_DTYPE_F32 ? 4 : 2, xq, x_node_stride, gb, indptr, src, eid, graph_off,
                               num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P, mode_flags, out,
                               out_node_stride, ep, a, g, 1);
  if (rc != hipSuccess || g.kernel == MRP_AGG_KERNEL_NONE) return rc;
  a.xscale = x_scale;
  a.qfmt = qdtype;
  return hipSuccess;
}

}  // namespace mrp_host

using namespace mrp_host;

extern "C" {

int mrp_film_mean_fwd_q(int32_t qdtype, const void* xq, int64_t x_node_stride, const float* x_scale,
                        int32_t out_dtype, const float* gb, const int32_t* indptr, const int32_t* src,
                        const int32_t* eid, const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                        int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P,
                        int32_t mode_flags, void* out, int64_t out_node_stride, const mrp_agg_epilogue* epilogue,
                        void* stream) {
  AggArgs a = {};
  Geometry g;
  const int rc = film_fwd_q_plan(qdtype, xq, x_node_stride, x_scale, out_dtype, gb, indptr, src, eid, graph_off,
                                 num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P, mode_flags, out,
                                 out_node_stride, epilogue, a, g);
  if (rc != hipSuccess || g.kernel == MRP_AGG_KERNEL_NONE) return rc;
  const bool complete = graph_kind == MRP_GRAPH_COMPLETE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (out_dtype) {
    case MRP_DTYPE_F32: return dispatch_fwd_q_f32(max_nodes, complete, a, g, st);
    case MRP_DTYPE_BF16: return dispatch_fwd_q_bf16(max_nodes, complete, a, g, st);
    default: return dispatch_fwd_q_f16(max_nodes, complete, a, g, st);
  }
}

int mrp_film_mean_fwd_q_plan(int32_t qdtype, const void* xq, int64_t x_node_stride, const float* x_scale,
                             int32_t out_dtype, const float* gb, const int32_t* indptr, const int32_t* src,
                             const int32_t* eid, const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                             int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P,
                             int32_t mode_flags, void* out, int64_t out_node_stride,
                             const mrp_agg_epilogue* epilogue, mrp_agg_plan* plan) {
  if (plan == nullptr) return hipErrorInvalidValue;
  AggArgs a = {};
  Geometry g;
  const int rc = film_fwd_q_plan(qdtype, xq, x_node_stride, x_scale, out_dtype, gb, indptr, src, eid, graph_off,
                                 num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P, mode_flags, out,
                                 out_node_stride, epilogue, a, g);
  if (rc == hipSuccess) fill_plan(g, 0, 0, plan);
  return rc;
}

}  // extern "C"
