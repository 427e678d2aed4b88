// film_attn_fwd_q.hip — FP8 messages for the attention reducers, receiver side: the C ABI (mrp_film_attn_fwd_q,
// mrp_film_wattn_fwd_q), the host checks both share and the launches of the ungated kernels (film_attn_fwd, TX = q8_t, with
// WGT = false, single- and multi-head).  The gated launches: film_wattn_fwd_q.hip.  Kernels and design notes:
// film_attn_kernels.hpp.
#include "film_attn_kernels.hpp"

namespace mrp_host {

hipError_t launch_attn_fwd_q(int32_t dtype, const mrp::AttnQArgs<false, false>& m, int ks, size_t lds, int64_t grid,
                             int heads, hipStream_t st) {
  return launch_attn_fwd_q_dtype<false, false>(dtype, m, ks, lds, grid, heads, st);
}
hipError_t launch_attn_fwd_q(int32_t dtype, const mrp::AttnQArgs<false, true>& m, int ks, size_t lds, int64_t grid,
                             int heads, hipStream_t st) {
  return launch_attn_fwd_q_dtype<false, true>(dtype, m, ks, lds, grid, heads, st);
}

namespace {

// the argument block of one form, from the single-head ungated one
template <bool WGT, bool MH>
hipError_t launch_form(int32_t dtype, const AttnArgs& base, const void* query, int64_t qs, const float* w, int64_t wst,
                       float* rate, int32_t C, int ks, size_t lds, int64_t grid, int heads, hipStream_t st) {
  mrp::AttnQArgs<WGT, MH> m = {};
  static_cast<AttnArgs&>(m) = base;
  m.q = query;
  m.qs = qs;
  if constexpr (WGT) {
    m.w = w;
    m.wst = wst;
    m.rate = rate;
  }
  if constexpr (MH) {
    m.a.C = C / heads;
    m.gbC = C;
  }
  return launch_attn_fwd_q(dtype, m, ks, lds, grid, heads, st);
}

}  // namespace

int attn_fwd_q(bool weighted, int32_t qdtype, const void* xq, int64_t xq_node_stride, const float* x_scale,
               int32_t dtype, const void* query, int64_t query_node_stride, const float* gb, const float* w,
               int64_t w_node_stride, const int32_t* indptr, const int32_t* src, const int32_t* eid,
               const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind, int32_t num_nodes,
               int32_t num_edges, int32_t C, int32_t P, int32_t flags, int32_t heads, void* out,
               int64_t out_node_stride, float scale, float* attn, float* rate, int64_t workspace_bytes, void* stream) {
  if (qdtype != MRP_QDTYPE_E4M3 && qdtype != MRP_QDTYPE_E5M2) return hipErrorInvalidValue;
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
      if (weighted && rate != nullptr) return hipMemsetAsync(rate, 0, ep_bytes, st);
    }
    return hipSuccess;
  }
  const int64_t plane = (int64_t)C * P;
  if (xq == nullptr || query == nullptr || out == nullptr) return hipErrorInvalidValue;
  if (xq_node_stride < plane || query_node_stride < plane || out_node_stride < plane) return hipErrorInvalidValue;
  if (weighted && (w == nullptr || w_node_stride < P)) return hipErrorInvalidValue;
  if (num_edges > 0 && (gb == nullptr || attn == nullptr)) return hipErrorInvalidValue;
  const int ntile = attn_tiles(P);
  const int64_t grid = (int64_t)num_graphs * ntile;
  const size_t lds = lds_attn(max_nodes, mrp::kAttnFwdChunk, false, weighted);
  if (grid > 0x7fffffff || heads > kMaxGridY || lds > kMaxDynamicLds) return hipErrorInvalidValue;
  // rows of attn and rate no CSR entry names are zeros (COMPLETE graphs name every row), in every head
  if (graph_kind != MRP_GRAPH_COMPLETE && num_edges > 0) {
    hipError_t e = hipMemsetAsync(attn, 0, ep_bytes, st);
    if (e == hipSuccess && weighted && rate != nullptr) e = hipMemsetAsync(rate, 0, ep_bytes, st);
    if (e != hipSuccess) return e;
  }
  AttnArgs m = {};
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
  float* rt = num_edges > 0 ? rate : nullptr;
  const int ks = attn_slots_for(graph_kind, max_nodes);
  if (weighted)
    return heads > 1 ? launch_form<true, true>(dtype, m, query, query_node_stride, w, w_node_stride, rt, C, ks, lds,
                                               grid, heads, st)
                     : launch_form<true, false>(dtype, m, query, query_node_stride, w, w_node_stride, rt, C, ks, lds,
                                                grid, 1, st);
  return heads > 1 ? launch_form<false, true>(dtype, m, query, query_node_stride, nullptr, 0, nullptr, C, ks, lds, grid,
                                              heads, st)
                   : launch_form<false, false>(dtype, m, query, query_node_stride, nullptr, 0, nullptr, C, ks, lds,
                                               grid, 1, st);
}

}  // namespace mrp_host

using namespace mrp_host;

extern "C" int mrp_film_attn_fwd_q(int32_t qdtype, const void* xq, int64_t xq_node_stride, const float* x_scale,
                                   int32_t dtype, const void* query, int64_t query_node_stride, const float* gb,
                                   const int32_t* indptr, const int32_t* src, const int32_t* eid,
                                   const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                                   int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t flags,
                                   int32_t heads, void* out, int64_t out_node_stride, float scale, float* attn,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
  (void)workspace;
  return attn_fwd_q(false, qdtype, xq, xq_node_stride, x_scale, dtype, query, query_node_stride, gb, nullptr, 0,
                    indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P, flags,
                    heads, out, out_node_stride, scale, attn, nullptr, workspace_bytes, stream);
}

extern "C" int mrp_film_wattn_fwd_q(int32_t qdtype, const void* xq, int64_t xq_node_stride, const float* x_scale,
                                    int32_t dtype, const void* query, int64_t query_node_stride, const float* gb,
                                    const float* w, int64_t w_node_stride, const int32_t* indptr, const int32_t* src,
                                    const int32_t* eid, const int32_t* graph_off, int32_t num_graphs,
                                    int32_t max_nodes, int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                                    int32_t C, int32_t P, int32_t flags, int32_t heads, void* out,
                                    int64_t out_node_stride, float scale, float* attn, float* rate, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  (void)workspace;
  return attn_fwd_q(true, qdtype, xq, xq_node_stride, x_scale, dtype, query, query_node_stride, gb, w, w_node_stride,
                    indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P, flags,
                    heads, out, out_node_stride, scale, attn, rate, workspace_bytes, stream);
}
