// film_wattn_fwd.hip — forward launcher, workspace query and C ABI of the confidence-gated attention fusion
// (mrp_film_wattn_fwd, mrp_film_wattn_workspace) and of its multi-head form (mrp_film_wattn_fwd_mh,
// mrp_film_wattn_workspace_mh; the MH launches: film_attn_mh_fwd.hip): film_attn's kernels with WGT = true.
// Kernels and design notes: film_attn_kernels.hpp.
#include "film_attn_kernels.hpp"

using namespace mrp_host;

namespace {

template <typename T>
hipError_t launch_wattn_fwd(const WAttnArgs& m, int ks, size_t lds, int64_t grid, hipStream_t st) {
  const dim3 g((unsigned)grid), block(mrp::kBlock);
  if (ks == 4)
    hipLaunchKernelGGL((mrp::film_attn_fwd<T, 4, true>), g, block, lds, st, m);
  else if (ks == 8)
    hipLaunchKernelGGL((mrp::film_attn_fwd<T, 8, true>), g, block, lds, st, m);
  else
    hipLaunchKernelGGL((mrp::film_attn_fwd<T, 16, true>), g, block, lds, st, m);
  return hipGetLastError();
}

// Both entry points; heads = 1 launches the single-head kernels.
int wattn_fwd(int32_t dtype, const void* x, int64_t x_node_stride, const float* gb, const float* w,
              int64_t w_node_stride, const int32_t* indptr, const int32_t* src, const int32_t* eid,
              const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind, int32_t num_nodes,
              int32_t num_edges, int32_t C, int32_t P, int32_t flags, int32_t heads, void* out,
              int64_t out_node_stride, float scale, float* attn, float* rate, int64_t workspace_bytes, void* stream);

}  // namespace

extern "C" int64_t mrp_film_wattn_workspace(int32_t direction, int32_t num_graphs, int32_t max_nodes,
                                            int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C,
                                            int32_t P) {
  (void)num_graphs;
  (void)max_nodes;
  (void)graph_kind;
  (void)num_nodes;
  // the forward needs none; grad_w is reduced inside the workgroup, so the backward's is film_attn's
  if (direction == 0 || num_edges <= 0 || C <= 0 || P <= 0) return 0;
  return attn_workspace_bytes(num_edges, C, P);
}

extern "C" int64_t mrp_film_wattn_workspace_mh(int32_t direction, int32_t num_graphs, int32_t max_nodes,
                                               int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C,
                                               int32_t P, int32_t heads) {
  // the backward's grad_gb partials hold every head's columns; grad_w's per-head partials follow them
  const int64_t base =
      mrp_film_wattn_workspace(direction, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P);
  if (direction == 0 || num_nodes <= 0 || P <= 0) return base;
  return base + attn_gw_partial_bytes(heads, num_nodes, P);
}

extern "C" int mrp_film_wattn_fwd(int32_t dtype, const void* x, int64_t x_node_stride, const float* gb, const float* w,
                                  int64_t w_node_stride, const int32_t* indptr, const int32_t* src, const int32_t* eid,
                                  const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                                  int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t flags, void* out,
                                  int64_t out_node_stride, float scale, float* attn, float* rate, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  (void)workspace;
  return wattn_fwd(dtype, x, x_node_stride, gb, w, w_node_stride, indptr, src, eid, graph_off, num_graphs, max_nodes,
                   graph_kind, num_nodes, num_edges, C, P, flags, 1, out, out_node_stride, scale, attn, rate,
                   workspace_bytes, stream);
}

extern "C" int mrp_film_wattn_fwd_mh(int32_t dtype, const void* x, int64_t x_node_stride, const float* gb,
                                     const float* w, int64_t w_node_stride, const int32_t* indptr, const int32_t* src,
                                     const int32_t* eid, const int32_t* graph_off, int32_t num_graphs,
                                     int32_t max_nodes, int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                                     int32_t C, int32_t P, int32_t flags, int32_t heads, void* out,
                                     int64_t out_node_stride, float scale, float* attn, float* rate, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  (void)workspace;
  return wattn_fwd(dtype, x, x_node_stride, gb, w, w_node_stride, indptr, src, eid, graph_off, num_graphs, max_nodes,
                   graph_kind, num_nodes, num_edges, C, P, flags, heads, out, out_node_stride, scale, attn, rate,
                   workspace_bytes, stream);
}

namespace {

int wattn_fwd(int32_t dtype, const void* x, int64_t x_node_stride, const float* gb, const float* w,
              int64_t w_node_stride, const int32_t* indptr, const int32_t* src, const int32_t* eid,
              const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind, int32_t num_nodes,
              int32_t num_edges, int32_t C, int32_t P, int32_t flags, int32_t heads, void* out,
              int64_t out_node_stride, float scale, float* attn, float* rate, int64_t workspace_bytes, void* stream) {
  if (!attn_common_ok(dtype, flags, indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes,
                      num_edges, C, P, scale) ||
      !attn_heads_ok(C, heads))
    return hipErrorInvalidValue;
  if (workspace_bytes < 0) return hipErrorInvalidValue;  // the forward's query is 0
  hipStream_t st = static_cast<hipStream_t>(stream);
  // attn and rate of every head
  const size_t ep_bytes =
      (size_t)heads * (size_t)(num_edges > 0 ? num_edges : 0) * (size_t)(P > 0 ? P : 0) * sizeof(float);
  if (num_graphs == 0 || num_nodes == 0 || max_nodes == 0 || C == 0 || P == 0) {
    // nothing to score: no kernel runs, and the weights and rates, where the caller passed buffers, are zeros
    if (ep_bytes > 0) {
      if (attn != nullptr) {
        const hipError_t e = hipMemsetAsync(attn, 0, ep_bytes, st);
        if (e != hipSuccess) return e;
      }
      if (rate != nullptr) return hipMemsetAsync(rate, 0, ep_bytes, st);
    }
    return hipSuccess;
  }
  const int64_t plane = (int64_t)C * P;
  if (x == nullptr || out == nullptr || x_node_stride < plane || out_node_stride < plane) return hipErrorInvalidValue;
  if (w == nullptr || w_node_stride < P) return hipErrorInvalidValue;
  if (num_edges > 0 && (gb == nullptr || attn == nullptr)) return hipErrorInvalidValue;
  const int ntile = attn_tiles(P);
  const int64_t grid = (int64_t)num_graphs * ntile;
  const size_t lds = lds_attn(max_nodes, mrp::kAttnFwdChunk, false, true);
  if (grid > 0x7fffffff || heads > kMaxGridY || lds > kMaxDynamicLds) return hipErrorInvalidValue;
  // rows of attn and rate no CSR entry names are zeros (COMPLETE graphs name every row)
  if (graph_kind != MRP_GRAPH_COMPLETE && num_edges > 0) {
    hipError_t e = hipMemsetAsync(attn, 0, ep_bytes, st);
    if (e == hipSuccess && rate != nullptr) e = hipMemsetAsync(rate, 0, ep_bytes, st);
    if (e != hipSuccess) return e;
  }
  WAttnArgs m = {};
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
  a.PV = P;
  a.logits = flags ? 1 : 0;
  a.kdeg = MRP_GRAPH_IS_REGULAR(graph_kind) ? MRP_GRAPH_REGULAR_K(graph_kind) : 0;
  a.nmax = max_nodes;
  m.complete = graph_kind == MRP_GRAPH_COMPLETE;
  m.ntile = ntile;
  m.nnodes = num_nodes;
  m.scale = scale;
  m.attn = attn;
  m.E = num_edges;
  m.w = w;
  m.wst = w_node_stride;
  m.rate = num_edges > 0 ? rate : nullptr;
  const int ks = attn_slots_for(graph_kind, max_nodes);
  if (heads > 1) {
    mrp::AttnMhArgs<true> mh = {};
    static_cast<WAttnArgs&>(mh) = m;
    mh.a.C = C / heads;
    mh.gbC = C;
    return launch_wattn_mh_fwd(dtype, mh, ks, lds, grid, heads, st);
  }
  switch (dtype) {
    case MRP_DTYPE_F32: return launch_wattn_fwd<float>(m, ks, lds, grid, st);
    case MRP_DTYPE_BF16: return launch_wattn_fwd<mrp::bf16_t>(m, ks, lds, grid, st);
    default: return launch_wattn_fwd<mrp::f16_t>(m, ks, lds, grid, st);
  }
}

}  // namespace
