// film_max_bwd.hip — backward planner, fp32 launches and C ABI of the max-pooled FiLM aggregation
// (mrp_film_max_bwd).  Kernels and design notes: film_max_kernels.hpp; 16-bit launches: film_max_bwd_{bf16,f16}.hip.
#include "film_max_kernels.hpp"
#include "film_mean_fwd_launch.hpp"

using namespace mrp_host;

namespace mrp_host {
hipError_t launch_max_bwd_f32(const MaxArgs& m, const MaxBwdPlan& p, hipStream_t st) {
  return launch_max_bwd<float>(m, p, st);
}
}  // namespace mrp_host

extern "C" int mrp_film_max_bwd(int32_t dtype, const void* grad_out, int64_t g_node_stride, const void* x,
                                int64_t x_node_stride, const float* gb, const int32_t* indptr, const int32_t* src,
                                const int32_t* eid, const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                                int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P,
                                int32_t flags, void* grad_x, int64_t gx_node_stride, const void* grad_x_base,
                                int64_t base_node_stride, float* grad_gb, void* stream) {
  if (dtype != MRP_DTYPE_F32 && dtype != MRP_DTYPE_BF16 && dtype != MRP_DTYPE_F16) return hipErrorInvalidValue;
  if (flags != 0 && flags != MRP_AGG_GB_LOGITS) return hipErrorInvalidValue;
  if (!common_args_ok(indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P,
                      MRP_AGG_FILM_MEAN))
    return hipErrorInvalidValue;
  const int32_t kdeg = MRP_GRAPH_IS_REGULAR(graph_kind) ? MRP_GRAPH_REGULAR_K(graph_kind) : 0;
  if (kdeg > MRP_FILM_MAX_DEGREE) return hipErrorInvalidValue;
  const bool want_dx = grad_x != nullptr, want_dgb = grad_gb != nullptr;
  if (!want_dx && !want_dgb) return hipSuccess;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool complete = graph_kind == MRP_GRAPH_COMPLETE;
  const bool empty = num_graphs == 0 || num_nodes == 0 || max_nodes == 0 || C == 0 || P == 0;
  const int64_t plane = (int64_t)C * P;
  if (!empty) {
    if (grad_out == nullptr || x == nullptr || g_node_stride < plane || x_node_stride < plane)
      return hipErrorInvalidValue;
    if (num_edges > 0 && gb == nullptr) return hipErrorInvalidValue;
    if (want_dx && gx_node_stride < plane) return hipErrorInvalidValue;
    if (want_dx && grad_x_base != nullptr && base_node_stride < plane) return hipErrorInvalidValue;
  }
  // rows of grad_gb no CSR entry names are zeros (COMPLETE graphs name every row)
  if (want_dgb && !complete && num_edges > 0 && C > 0) {
    const hipError_t e = hipMemsetAsync(grad_gb, 0, (size_t)num_edges * C * 2 * sizeof(float), st);
    if (e != hipSuccess) return e;
  }
  if (empty) return hipSuccess;

  const size_t elem = dtype == MRP_DTYPE_F32 ? 4 : 2;
  SliceCheck sc;
  sc.strides = P;
  sc.add(grad_out, g_node_stride);
  sc.add(x, x_node_stride);
  if (want_dx) sc.add(grad_x, gx_node_stride);
  if (want_dx && grad_x_base != nullptr) sc.add(grad_x_base, base_node_stride);
  MaxBwdPlan p;
  p.bucket = max_bucket(max_nodes);
  // in-degree bound the graph kind gives.  Only COMPLETE and REGULAR(k) give one: this operator does not rely on
  // MRP_GRAPH_SIMPLE's promise (its rows may hold parallel edges here), so SIMPLE is bounded as CSR is, by the
  // operator's limit, and takes the 16-slot kernels
  const int maxdeg = complete ? max_nodes - 1 : (kdeg > 0 ? kdeg : MRP_FILM_MAX_DEGREE);
  const bool fused = want_dgb && (p.bucket == 4 || (p.bucket == 8 && maxdeg <= 8));
  // 4-element slices for every dtype (16 / 8 bytes), 2-element ones in the fused kernels: the widths at
  // which no instantiation spills beside its partial sums (DESIGN §3.13's table)
  const int vec = sc.ok(4, elem) ? (fused ? 2 : 4) : 1;
  p.g = make_geometry(C, P, vec, 8, 64, mrp::kMaxChanPerBlock);  // lpc <= 64: a plane's lanes in one wave
  p.g.lds = lds_max(p.bucket, p.g.cpb);
  p.g.grid = (int64_t)num_graphs * p.g.ncb;
  if (!want_dgb) {
    p.run_dx = 1;
  } else if (fused) {
    p.fused = 1;
    p.ks = p.bucket == 4 ? 16 : 8;
  } else {
    p.run_dx = want_dx;
    p.run_dgb = 1;
    p.ks = 16;
    p.nvb = (max_nodes + 3) / 4;
  }
  if (p.g.grid * p.nvb > 0x7fffffff || p.g.lds > kMaxDynamicLds) return hipErrorInvalidValue;

  MaxArgs m = {};
  AggArgs& a = m.a;
  a.x = x;
  a.xs = x_node_stride;
  a.g = grad_out;
  a.gs = g_node_stride;
  a.gb = gb;
  a.indptr = indptr;
  a.src = src;
  a.eid = eid;
  a.goff = graph_off;
  a.out = grad_x;
  a.os = gx_node_stride;
  a.dgb = grad_gb;
  a.dxb = want_dx ? grad_x_base : nullptr;
  a.dxbs = base_node_stride;
  a.C = C;
  a.P = P;
  a.PV = P / vec;
  a.lpc = p.g.lpc;
  a.cpb = p.g.cpb;
  a.ncb = p.g.ncb;
  a.want_dx = want_dx;
  a.want_dgb = want_dgb;
  a.logits = flags ? 1 : 0;
  a.kdeg = kdeg;
  a.nmax = max_nodes;
  m.complete = complete;
  m.nvb = 1;
  if (dtype == MRP_DTYPE_F32) return launch_max_bwd_f32(m, p, st);
  return dtype == MRP_DTYPE_BF16 ? launch_max_bwd_bf16(m, p, st) : launch_max_bwd_f16(m, p, st);
}
