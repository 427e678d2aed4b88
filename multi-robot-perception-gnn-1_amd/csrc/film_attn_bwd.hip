// film_attn_bwd.hip — backward launcher and C ABI of the attention-pooled FiLM aggregation
// (mrp_film_attn_bwd) and of its multi-head form (mrp_film_attn_bwd_mh; the MH launches: film_attn_mh_bwd*.hip),
// and the fp32 launches.  Kernels and design notes: film_attn_kernels.hpp; 16-bit launches:
// film_attn_bwd_{bf16,f16}.hip.
#include "film_attn_kernels.hpp"

using namespace mrp_host;

namespace mrp {

// grad_gb of a plane that spans several tiles: the tiles' partials of every CSR entry summed in tile order.
// One thread per (node, slot, channel), channel fastest.
__global__ void __launch_bounds__(kBlock) film_attn_dgb_reduce(AttnArgs m) {
  const AggArgs& a = m.a;
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= (int64_t)m.nnodes * kAttnSlots * a.C) return;
  const int c = (int)(idx % a.C);
  const int rest = (int)(idx / a.C);
  const int node = rest / kAttnSlots, j = rest - node * kAttnSlots;
  int e;
  if (m.complete) {
    const int n = a.nmax, b = node / n, v = node - b * n;
    if (j >= n - 1) return;
    const int u = j < v ? j : j + 1;
    e = b * n * (n - 1) + u * (n - 1) + (v < u ? v : v - 1);
  } else {
    const int beg = a.kdeg > 0 ? node * a.kdeg : a.indptr[node];
    const int end = a.kdeg > 0 ? beg + a.kdeg : a.indptr[node + 1];
    if (j >= end - beg) return;
    e = a.eid[beg + j];
  }
  const int64_t off = ((int64_t)e * a.C + c) * 2;
  float2 r = make_float2(0.f, 0.f);
  for (int t = 0; t < m.ntile; ++t) {
    const float2 q = *reinterpret_cast<const float2*>(m.ws + (int64_t)t * m.E * a.C * 2 + off);
    r.x = __fadd_rn(r.x, q.x);
    r.y = __fadd_rn(r.y, q.y);
  }
  if (a.logits) r = sigmoid_backward(r, *reinterpret_cast<const float2*>(a.gb + off));
  *reinterpret_cast<float2*>(a.dgb + off) = r;
}

}  // namespace mrp

namespace mrp_host {
hipError_t launch_attn_bwd_f32(const AttnArgs& m, int ck, int ks, size_t lds, int64_t grid, hipStream_t st) {
  return launch_attn_bwd<float>(m, ck, ks, lds, grid, st);
}
hipError_t launch_attn_dgb_reduce(const AttnArgs& m, int64_t blocks, hipStream_t st) {
  hipLaunchKernelGGL(mrp::film_attn_dgb_reduce, dim3((unsigned)blocks), dim3(mrp::kBlock), 0, st, m);
  return hipGetLastError();
}
}  // namespace mrp_host

namespace {

// Both entry points; heads = 1 launches the single-head kernels.
int attn_bwd(int32_t dtype, const void* grad_out, int64_t g_node_stride, const void* x, int64_t x_node_stride,
             const float* gb, const int32_t* indptr, const int32_t* src, const int32_t* eid, const int32_t* graph_off,
             int32_t num_graphs, int32_t max_nodes, int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C,
             int32_t P, int32_t flags, int32_t heads, void* grad_x, int64_t gx_node_stride, const void* grad_x_base,
             int64_t base_node_stride, float* grad_gb, float scale, const float* attn, void* workspace,
             int64_t workspace_bytes, void* stream) {
  if (!attn_common_ok(dtype, flags, indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes,
                      num_edges, C, P, scale) ||
      !attn_heads_ok(C, heads))
    return hipErrorInvalidValue;
  if (workspace_bytes < 0) return hipErrorInvalidValue;
  const bool want_dx = grad_x != nullptr, want_dgb = grad_gb != nullptr;
  if (!want_dx && !want_dgb) return hipSuccess;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool complete = graph_kind == MRP_GRAPH_COMPLETE;
  const bool empty = num_graphs == 0 || num_nodes == 0 || max_nodes == 0 || C == 0 || P == 0;
  const int64_t plane = (int64_t)C * P;
  // grad_gb's tile partials: only where it is wanted, there are edges and a plane spans several tiles
  const int64_t need_ws = want_dgb && !empty && num_edges > 0 ? attn_workspace_bytes(num_edges, C, P) : 0;
  if (!empty) {
    if (grad_out == nullptr || x == nullptr || g_node_stride < plane || x_node_stride < plane)
      return hipErrorInvalidValue;
    if (num_edges > 0 && (gb == nullptr || attn == nullptr)) return hipErrorInvalidValue;
    if (want_dx && gx_node_stride < plane) return hipErrorInvalidValue;
    if (want_dx && grad_x_base != nullptr && base_node_stride < plane) return hipErrorInvalidValue;
    if (need_ws > 0 && (workspace == nullptr || workspace_bytes < need_ws)) return hipErrorInvalidValue;
  }
  const int ntile = attn_tiles(P);
  const int64_t grid = (int64_t)num_graphs * ntile;
  const int ck = attn_bwd_chunk(max_nodes);
  const size_t lds = lds_attn(max_nodes, ck, true);
  const int64_t rblocks = ((int64_t)num_nodes * mrp::kAttnSlots * C + mrp::kBlock - 1) / mrp::kBlock;
  if (!empty && (grid > 0x7fffffff || heads > kMaxGridY || rblocks > 0x7fffffff || lds > kMaxDynamicLds))
    return hipErrorInvalidValue;
  // rows of grad_gb no CSR entry names are zeros (COMPLETE graphs name every row)
  if (want_dgb && !complete && num_edges > 0 && C > 0) {
    const hipError_t e = hipMemsetAsync(grad_gb, 0, (size_t)num_edges * C * 2 * sizeof(float), st);
    if (e != hipSuccess) return e;
  }
  if (empty) return hipSuccess;

  AttnArgs m = {};
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
  const int ks = attn_slots_for(graph_kind, max_nodes);
  hipError_t rc;
  if (heads > 1) {
    mrp::AttnMhArgs<false> mh = {};
    static_cast<AttnArgs&>(mh) = m;
    mh.a.C = C / heads;
    mh.gbC = C;
    switch (dtype) {
      case MRP_DTYPE_F32: rc = launch_attn_mh_bwd_f32(mh, ck, ks, lds, grid, heads, st); break;
      case MRP_DTYPE_BF16: rc = launch_attn_mh_bwd_bf16(mh, ck, ks, lds, grid, heads, st); break;
      default: rc = launch_attn_mh_bwd_f16(mh, ck, ks, lds, grid, heads, st); break;
    }
  } else {
    switch (dtype) {
      case MRP_DTYPE_F32: rc = launch_attn_bwd_f32(m, ck, ks, lds, grid, st); break;
      case MRP_DTYPE_BF16: rc = launch_attn_bwd_bf16(m, ck, ks, lds, grid, st); break;
      default: rc = launch_attn_bwd_f16(m, ck, ks, lds, grid, st); break;
    }
  }
  if (rc != hipSuccess) return rc;
  if (a.want_dgb && ntile > 1) {
    hipLaunchKernelGGL(mrp::film_attn_dgb_reduce, dim3((unsigned)rblocks), dim3(mrp::kBlock), 0, st, m);
    rc = hipGetLastError();
  }
  return rc;
}

}  // namespace

extern "C" int mrp_film_attn_bwd(int32_t dtype, const void* grad_out, int64_t g_node_stride, const void* x,
                                 int64_t x_node_stride, const float* gb, const int32_t* indptr, const int32_t* src,
                                 const int32_t* eid, const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                                 int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P,
                                 int32_t flags, void* grad_x, int64_t gx_node_stride, const void* grad_x_base,
                                 int64_t base_node_stride, float* grad_gb, float scale, const float* attn,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  return attn_bwd(dtype, grad_out, g_node_stride, x, x_node_stride, gb, indptr, src, eid, graph_off, num_graphs,
                  max_nodes, graph_kind, num_nodes, num_edges, C, P, flags, 1, grad_x, gx_node_stride, grad_x_base,
                  base_node_stride, grad_gb, scale, attn, workspace, workspace_bytes, stream);
}

extern "C" int mrp_film_attn_bwd_mh(int32_t dtype, const void* grad_out, int64_t g_node_stride, const void* x,
                                    int64_t x_node_stride, const float* gb, const int32_t* indptr, const int32_t* src,
                                    const int32_t* eid, const int32_t* graph_off, int32_t num_graphs,
                                    int32_t max_nodes, int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                                    int32_t C, int32_t P, int32_t flags, int32_t heads, void* grad_x,
                                    int64_t gx_node_stride, const void* grad_x_base, int64_t base_node_stride,
                                    float* grad_gb, float scale, const float* attn, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  return attn_bwd(dtype, grad_out, g_node_stride, x, x_node_stride, gb, indptr, src, eid, graph_off, num_graphs,
                  max_nodes, graph_kind, num_nodes, num_edges, C, P, flags, heads, grad_x, gx_node_stride, grad_x_base,
                  base_node_stride, grad_gb, scale, attn, workspace, workspace_bytes, stream);
}
