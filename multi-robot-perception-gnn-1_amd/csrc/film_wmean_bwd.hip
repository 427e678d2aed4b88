// film_wmean_bwd.hip — backward planner, fp32 launches and C ABI of the confidence-weighted FiLM aggregation
// (mrp_film_wmean_bwd).  Kernels and design notes: film_wmean_kernels.hpp; 16-bit launches:
// film_wmean_bwd_{bf16,f16}.hip.
#include "film_wmean_kernels.hpp"
#include "film_mean_fwd_launch.hpp"

using namespace mrp_host;

namespace mrp_host {
hipError_t launch_wmean_bwd_f32(const WArgs& m, const WBwdPlan& p, hipStream_t st) {
  return launch_wmean_bwd<float>(m, p, st);
}
}  // namespace mrp_host

extern "C" int mrp_film_wmean_bwd(int32_t dtype, const void* grad_out, int64_t g_node_stride, const void* x,
                                  int64_t x_node_stride, const float* gb, const float* w, int64_t w_node_stride,
                                  const int32_t* indptr, const int32_t* src, const int32_t* eid,
                                  const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                                  int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t flags,
                                  int32_t wagg, void* grad_x, int64_t gx_node_stride, const void* grad_x_base,
                                  int64_t base_node_stride, float* grad_gb, float* grad_w, int64_t gw_node_stride,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  if (dtype != MRP_DTYPE_F32 && dtype != MRP_DTYPE_BF16 && dtype != MRP_DTYPE_F16) return hipErrorInvalidValue;
  if (flags != 0 && flags != MRP_AGG_GB_LOGITS) return hipErrorInvalidValue;
  if (wagg != MRP_WAGG_MEAN && wagg != MRP_WAGG_SUM) return hipErrorInvalidValue;
  if (!common_args_ok(indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P,
                      MRP_AGG_FILM_MEAN))
    return hipErrorInvalidValue;
  const int32_t kdeg = MRP_GRAPH_IS_REGULAR(graph_kind) ? MRP_GRAPH_REGULAR_K(graph_kind) : 0;
  const bool want_dx = grad_x != nullptr, want_dgb = grad_gb != nullptr, want_dw = grad_w != nullptr;
  if (!want_dx && !want_dgb && !want_dw) return hipSuccess;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool complete = graph_kind == MRP_GRAPH_COMPLETE;
  const bool no_planes = num_graphs == 0 || num_nodes == 0 || max_nodes == 0 || P == 0;
  const bool empty = no_planes || C == 0;
  const int64_t plane = (int64_t)C * P;
  const int64_t ws_need = want_dw && !empty ? wmean_workspace_bytes(num_nodes, C, P) : 0;
  if (!empty) {
    if (grad_out == nullptr || x == nullptr || g_node_stride < plane || x_node_stride < plane)
      return hipErrorInvalidValue;
    if (w == nullptr || w_node_stride < P) return hipErrorInvalidValue;
    if (num_edges > 0 && gb == nullptr) return hipErrorInvalidValue;
    if (want_dx && gx_node_stride < plane) return hipErrorInvalidValue;
    if (want_dx && grad_x_base != nullptr && base_node_stride < plane) return hipErrorInvalidValue;
    if (ws_need > 0 && (workspace == nullptr || workspace_bytes < ws_need)) return hipErrorInvalidValue;
  }
  if (want_dw && !no_planes && gw_node_stride < P) return hipErrorInvalidValue;
  // rows of grad_gb no CSR entry names are zeros (COMPLETE graphs name every row)
  if (want_dgb && !complete && num_edges > 0 && C > 0) {
    const hipError_t e = hipMemsetAsync(grad_gb, 0, (size_t)num_edges * C * 2 * sizeof(float), st);
    if (e != hipSuccess) return e;
  }
  // without channels there is nothing to sum: grad_w is zeros
  if (want_dw && !no_planes && C == 0) {
    const hipError_t e = hipMemset2DAsync(grad_w, (size_t)gw_node_stride * sizeof(float), 0, (size_t)P * sizeof(float),
                                          (size_t)num_nodes, st);
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
  bool f32_ok = aligned16(w) && w_node_stride % 4 == 0;
  if (want_dw) f32_ok = f32_ok && aligned16(grad_w) && gw_node_stride % 4 == 0 && (ws_need == 0 || aligned16(workspace));
  WBwdPlan p;
  p.bucket = wmean_bucket(max_nodes);
  // 4-element slices up to 8 nodes; beyond, the slices of x, w, grad_out and the accumulators of 16 nodes at
  // 4 elements each pass the register file
  p.vec = p.bucket <= 8 && sc.ok(4, elem) && f32_ok ? 4 : 1;
  const int32_t pv = P / p.vec;
  if (want_dx || want_dw) {
    p.run_xw = 1;
    p.cpb_xw = std::min<int>(C, mrp::kWChanBlock);
    p.ncb_xw = wmean_dw_blocks(C);
    p.threads_xw = 64;
    while (p.threads_xw < pv && p.threads_xw < mrp::kBlock) p.threads_xw *= 2;
    p.nseg = (pv + p.threads_xw - 1) / p.threads_xw;
    p.grid_xw = (int64_t)num_graphs * p.ncb_xw * p.nseg;
    p.lds_xw = lds_wmean(p.bucket, p.cpb_xw);
    if (p.grid_xw > 0x7fffffff || p.lds_xw > kMaxDynamicLds) return hipErrorInvalidValue;
    if (((int64_t)num_nodes * P + mrp::kBlock - 1) / mrp::kBlock > 0x7fffffff) return hipErrorInvalidValue;
  }
  if (want_dgb) {
    p.run_gb = 1;
    p.g = make_geometry(C, P, p.vec, 8, 64, mrp::kMaxChanPerBlock);  // lpc <= 64: a plane's lanes in one wave
    p.g.lds = lds_wmean_gb(p.bucket, p.g.cpb);
    p.nvb = (max_nodes + mrp::kWDestBlock - 1) / mrp::kWDestBlock;
    p.g.grid = (int64_t)num_graphs * p.g.ncb * p.nvb;
    if (p.g.grid > 0x7fffffff || p.g.lds > kMaxDynamicLds) return hipErrorInvalidValue;
  }

  WArgs m = {};
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
  a.PV = pv;
  a.want_dx = want_dx;
  a.want_dgb = want_dgb;
  a.logits = flags ? 1 : 0;
  a.kdeg = kdeg;
  a.nmax = max_nodes;
  m.w = w;
  m.ws = w_node_stride;
  m.complete = complete;
  m.mean = wagg == MRP_WAGG_MEAN;
  m.want_dw = want_dw;
  if (want_dw && ws_need > 0) {
    m.dw = static_cast<float*>(workspace);
    m.dws = P;
    m.dwbs = (int64_t)num_nodes * P;
  } else {
    m.dw = grad_w;
    m.dws = gw_node_stride;
    m.dwbs = 0;
  }
  hipError_t e;
  if (dtype == MRP_DTYPE_F32)
    e = launch_wmean_bwd_f32(m, p, st);
  else
    e = dtype == MRP_DTYPE_BF16 ? launch_wmean_bwd_bf16(m, p, st) : launch_wmean_bwd_f16(m, p, st);
  if (e != hipSuccess) return e;
  if (want_dw && ws_need > 0) {
    // (a node outside every graph gets no partial: the workspace rows of such nodes are not written, so only
    // batches whose graphs cover all nodes are supported, as everywhere in this library)
    const int64_t total = (int64_t)num_nodes * P;
    const int64_t blocks = (total + mrp::kBlock - 1) / mrp::kBlock;
    hipLaunchKernelGGL((mrp::film_wmean_dw_reduce<0>), dim3((unsigned)blocks), dim3(mrp::kBlock), 0, st,
                       static_cast<const float*>(workspace), p.ncb_xw, m.dwbs, grad_w, gw_node_stride, total, P);
    return hipGetLastError();
  }
  return hipSuccess;
}
