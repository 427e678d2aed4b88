// film_wmean_fwd.hip — forward launcher, workspace query and C ABI of the confidence-weighted FiLM aggregation
// (mrp_film_wmean_fwd, mrp_film_wmean_workspace).  Kernels and design notes: film_wmean_kernels.hpp.
#include "film_wmean_kernels.hpp"
#include "film_mean_fwd_launch.hpp"

using namespace mrp_host;

namespace {

template <typename T>
hipError_t launch_wmean_fwd(const WArgs& m, const Geometry& g, int bucket, hipStream_t st) {
  const dim3 grid((unsigned)g.grid), block(g.threads);
#define MRP_WMEAN_FWD(NT)                                                                    \
  do {                                                                                       \
    if (g.vec == 4)                                                                          \
      hipLaunchKernelGGL((mrp::film_wmean_fwd<NT, 4, T>), grid, block, g.lds, st, m);        \
    else                                                                                     \
      hipLaunchKernelGGL((mrp::film_wmean_fwd<NT, 1, T>), grid, block, g.lds, st, m);        \
  } while (0)
  if (bucket == 4)
    MRP_WMEAN_FWD(4);
  else if (bucket == 8)
    MRP_WMEAN_FWD(8);
  else
    MRP_WMEAN_FWD(16);
#undef MRP_WMEAN_FWD
  return hipGetLastError();
}

}  // namespace

extern "C" int64_t mrp_film_wmean_workspace(int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                                            int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P) {
  (void)graph_kind;
  (void)num_edges;
  if (num_graphs <= 0 || max_nodes <= 0 || num_nodes <= 0 || C <= 0 || P <= 0) return 0;
  return wmean_workspace_bytes(num_nodes, C, P);
}

extern "C" int mrp_film_wmean_fwd(int32_t dtype, const void* x, int64_t x_node_stride, const float* gb,
                                  const float* w, int64_t w_node_stride, const int32_t* indptr, const int32_t* src,
                                  const int32_t* eid, const int32_t* graph_off, int32_t num_graphs,
                                  int32_t max_nodes, int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                                  int32_t C, int32_t P, int32_t flags, int32_t wagg, void* out,
                                  int64_t out_node_stride, void* stream) {
  if (dtype != MRP_DTYPE_F32 && dtype != MRP_DTYPE_BF16 && dtype != MRP_DTYPE_F16) return hipErrorInvalidValue;
  if (flags != 0 && flags != MRP_AGG_GB_LOGITS) return hipErrorInvalidValue;
  if (wagg != MRP_WAGG_MEAN && wagg != MRP_WAGG_SUM) return hipErrorInvalidValue;
  if (!common_args_ok(indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P,
                      MRP_AGG_FILM_MEAN))
    return hipErrorInvalidValue;
  const int32_t kdeg = MRP_GRAPH_IS_REGULAR(graph_kind) ? MRP_GRAPH_REGULAR_K(graph_kind) : 0;
  if (num_graphs == 0 || num_nodes == 0 || max_nodes == 0 || C == 0 || P == 0) return hipSuccess;
  const int64_t plane = (int64_t)C * P;
  if (x == nullptr || out == nullptr || x_node_stride < plane || out_node_stride < plane) return hipErrorInvalidValue;
  if (w == nullptr || w_node_stride < P) return hipErrorInvalidValue;
  if (num_edges > 0 && gb == nullptr) return hipErrorInvalidValue;
  const size_t elem = dtype == MRP_DTYPE_F32 ? 4 : 2;
  SliceCheck sc;
  sc.strides = P;
  sc.add(x, x_node_stride);
  sc.add(out, out_node_stride);
  // 4-element slices (16-byte w loads) where x, out and w allow, else single elements
  const int vec = sc.ok(4, elem) && aligned16(w) && w_node_stride % 4 == 0 ? 4 : 1;
  const Tuning& tu = tuning();
  Geometry g = make_geometry(C, P, vec, tu.fwd_lo, tu.fwd_hi, tu.fwd_cap);
  const int bucket = wmean_bucket(max_nodes);
  g.lds = lds_wmean(bucket, g.cpb);
  // COMPLETE graphs: one slice per lane, the plane split over workgroups (arithmetic prologue); the other
  // kinds keep whole planes, as the mean forward does: their prologue walks the CSR
  const int32_t pv = P / g.vec;
  g.psplit = graph_kind == MRP_GRAPH_COMPLETE ? (pv + g.lpc - 1) / g.lpc : 1;
  g.grid = (int64_t)num_graphs * g.ncb * g.psplit;
  if (g.grid > 0x7fffffff || g.lds > kMaxDynamicLds) return hipErrorInvalidValue;
  WArgs m = {};
  AggArgs& a = m.a;
  a.x = x;
  a.xs = x_node_stride;
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
  m.w = w;
  m.ws = w_node_stride;
  m.complete = graph_kind == MRP_GRAPH_COMPLETE;
  m.mean = wagg == MRP_WAGG_MEAN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case MRP_DTYPE_F32: return launch_wmean_fwd<float>(m, g, bucket, st);
    case MRP_DTYPE_BF16: return launch_wmean_fwd<mrp::bf16_t>(m, g, bucket, st);
    default: return launch_wmean_fwd<mrp::f16_t>(m, g, bucket, st);
  }
}
