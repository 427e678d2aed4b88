// film_wattn_bwd.hip — backward launcher and C ABI of the confidence-gated attention fusion
// (mrp_film_wattn_bwd) and of its multi-head form (mrp_film_wattn_bwd_mh; the MH launches: film_attn_mh_bwd*.hip),
// and the fp32 launches: film_attn's backward kernel with WGT = true.  Kernels and design
// notes: film_attn_kernels.hpp; 16-bit launches: film_wattn_bwd_{bf16,f16}.hip.
#include "film_attn_kernels.hpp"

using namespace mrp_host;

namespace mrp_host {
hipError_t launch_wattn_bwd_f32(const WAttnArgs& m, int ck, int ks, size_t lds, int64_t grid, hipStream_t st) {
  return launch_attn_bwd<float, true>(m, ck, ks, lds, grid, st);
}
}  // namespace mrp_host

namespace {

// Both entry points; heads = 1 launches the single-head kernels.
int wattn_bwd(int32_t dtype, const void* grad_out, int64_t g_node_stride, const void* x, int64_t x_node_stride,
              const float* gb, const float* w, int64_t w_node_stride, const int32_t* indptr, const int32_t* src,
              const int32_t* eid, const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
              int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t flags, int32_t heads, void* grad_x,
              int64_t gx_node_stride, const void* grad_x_base, int64_t base_node_stride, float* grad_gb, float scale,
              const float* attn, const float* rate, float* grad_w, int64_t gw_node_stride, void* workspace,
              int64_t workspace_bytes, void* stream) {
  if (!attn_common_ok(dtype, flags, indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes,
                      num_edges, C, P, scale) ||
      !attn_heads_ok(C, heads))
    return hipErrorInvalidValue;
  if (workspace_bytes < 0) return hipErrorInvalidValue;
  const bool want_dx = grad_x != nullptr, want_dgb = grad_gb != nullptr, want_dw = grad_w != nullptr;
  if (!want_dx && !want_dgb && !want_dw) return hipSuccess;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool complete = graph_kind == MRP_GRAPH_COMPLETE;
  const bool empty = num_graphs == 0 || num_nodes == 0 || max_nodes == 0 || C == 0 || P == 0;
  const int64_t plane = (int64_t)C * P;
  // grad_gb's tile partials: only where it is wanted, there are edges and a plane spans several tiles
  const int64_t dgb_ws = want_dgb && !empty && num_edges > 0 ? attn_workspace_bytes(num_edges, C, P) : 0;
  // grad_w's per-head partials (H, nodes, P) follow them: only where grad_w is wanted and there are several heads
  const int64_t need_ws = dgb_ws + (want_dw && !empty ? attn_gw_partial_bytes(heads, num_nodes, P) : 0);
  if (want_dw && gw_node_stride < P) return hipErrorInvalidValue;
  if (!empty) {
    if (grad_out == nullptr || x == nullptr || g_node_stride < plane || x_node_stride < plane)
      return hipErrorInvalidValue;
    if (w == nullptr || w_node_stride < P) return hipErrorInvalidValue;
    if (num_edges > 0 && (gb == nullptr || attn == nullptr)) return hipErrorInvalidValue;
    if (num_edges > 0 && want_dw && rate == nullptr) return hipErrorInvalidValue;
    if (want_dx && gx_node_stride < plane) return hipErrorInvalidValue;
    if (want_dx && grad_x_base != nullptr && base_node_stride < plane) return hipErrorInvalidValue;
    if (need_ws > 0 && (workspace == nullptr || workspace_bytes < need_ws)) return hipErrorInvalidValue;
  }
  const int ntile = attn_tiles(P);
  const int64_t grid = (int64_t)num_graphs * ntile;
  const int ck = attn_bwd_chunk(max_nodes);
  const size_t lds = lds_attn(max_nodes, ck, true, true);
  const int64_t rblocks = ((int64_t)num_nodes * mrp::kAttnSlots * C + mrp::kBlock - 1) / mrp::kBlock;
  if (!empty && (grid > 0x7fffffff || heads > kMaxGridY || rblocks > 0x7fffffff || lds > kMaxDynamicLds))
    return hipErrorInvalidValue;
  // rows of grad_gb no CSR entry names are zeros (COMPLETE graphs name every row)
  if (want_dgb && !complete && num_edges > 0 && C > 0) {
    const hipError_t e = hipMemsetAsync(grad_gb, 0, (size_t)num_edges * C * 2 * sizeof(float), st);
    if (e != hipSuccess) return e;
  }
  if (empty) {
    // no channels: nothing depends on w
    if (want_dw && num_nodes > 0 && P > 0)
      return hipMemset2DAsync(grad_w, (size_t)gw_node_stride * sizeof(float), 0, (size_t)P * sizeof(float),
                              (size_t)num_nodes, st);
    return hipSuccess;
  }

  WAttnArgs m = {};
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
  a.PV = P;
  a.want_dx = want_dx;
  a.want_dgb = want_dgb && num_edges > 0;
  a.logits = flags ? 1 : 0;
  a.kdeg = MRP_GRAPH_IS_REGULAR(graph_kind) ? MRP_GRAPH_REGULAR_K(graph_kind) : 0;
  a.nmax = max_nodes;
  m.complete = complete;
  m.ntile = ntile;
  m.nnodes = num_nodes;
  m.scale = scale;
  m.attn = const_cast<float*>(attn);
  m.ws = static_cast<float*>(workspace);
  m.E = num_edges;
  m.w = w;
  m.wst = w_node_stride;
  m.rate = const_cast<float*>(rate);
  m.gw = grad_w;
  m.gwst = gw_node_stride;
  const int ks = attn_slots_for(graph_kind, max_nodes);
  hipError_t rc;
  if (heads > 1) {
    mrp::AttnMhArgs<true> mh = {};
    static_cast<WAttnArgs&>(mh) = m;
    mh.a.C = C / heads;
    mh.gbC = C;
    float* part = reinterpret_cast<float*>(static_cast<char*>(workspace) + dgb_ws);
    if (want_dw) {
      // every head writes its own (nodes, P) partial; film_attn_gw_reduce sums them, heads ascending
      mh.gw = part;
      mh.gwst = P;
      mh.gwhs = (int64_t)num_nodes * P;
    }
    switch (dtype) {
      case MRP_DTYPE_F32: rc = launch_wattn_mh_bwd_f32(mh, ck, ks, lds, grid, heads, st); break;
      case MRP_DTYPE_BF16: rc = launch_wattn_mh_bwd_bf16(mh, ck, ks, lds, grid, heads, st); break;
      default: rc = launch_wattn_mh_bwd_f16(mh, ck, ks, lds, grid, heads, st); break;
    }
    if (rc == hipSuccess && want_dw)
      rc = launch_attn_gw_reduce(part, heads, num_nodes, P, grad_w, gw_node_stride, st);
  } else {
    switch (dtype) {
      case MRP_DTYPE_F32: rc = launch_wattn_bwd_f32(m, ck, ks, lds, grid, st); break;
      case MRP_DTYPE_BF16: rc = launch_wattn_bwd_bf16(m, ck, ks, lds, grid, st); break;
      default: rc = launch_wattn_bwd_f16(m, ck, ks, lds, grid, st); break;
    }
  }
  if (rc != hipSuccess) return rc;
  if (a.want_dgb && ntile > 1) rc = launch_attn_dgb_reduce(m, rblocks, st);
  return rc;
}

}  // namespace

extern "C" int mrp_film_wattn_bwd(int32_t dtype, const void* grad_out, int64_t g_node_stride, const void* x,
                                  int64_t x_node_stride, const float* gb, const float* w, int64_t w_node_stride,
                                  const int32_t* indptr, const int32_t* src, const int32_t* eid,
                                  const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                                  int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t flags,
                                  void* grad_x, int64_t gx_node_stride, const void* grad_x_base,
                                  int64_t base_node_stride, float* grad_gb, float scale, const float* attn,
                                  const float* rate, float* grad_w, int64_t gw_node_stride, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  return wattn_bwd(dtype, grad_out, g_node_stride, x, x_node_stride, gb, w, w_node_stride, indptr, src, eid,
                   graph_off, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P, flags, 1, grad_x,
                   gx_node_stride, grad_x_base, base_node_stride, grad_gb, scale, attn, rate, grad_w, gw_node_stride,
                   workspace, workspace_bytes, stream);
}

extern "C" int mrp_film_wattn_bwd_mh(int32_t dtype, const void* grad_out, int64_t g_node_stride, const void* x,
                                     int64_t x_node_stride, const float* gb, const float* w, int64_t w_node_stride,
                                     const int32_t* indptr, const int32_t* src, const int32_t* eid,
                                     const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                                     int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P,
                                     int32_t flags, int32_t heads, void* grad_x, int64_t gx_node_stride,
                                     const void* grad_x_base, int64_t base_node_stride, float* grad_gb, float scale,
                                     const float* attn, const float* rate, float* grad_w, int64_t gw_node_stride,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
  return wattn_bwd(dtype, grad_out, g_node_stride, x, x_node_stride, gb, w, w_node_stride, indptr, src, eid,
                   graph_off, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P, flags, heads, grad_x,
                   gx_node_stride, grad_x_base, base_node_stride, grad_gb, scale, attn, rate, grad_w, gw_node_stride,
                   workspace, workspace_bytes, stream);
}
