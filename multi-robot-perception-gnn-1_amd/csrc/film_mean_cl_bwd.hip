// film_mean_cl_bwd.hip — mrp_film_mean_bwd_cl and its workspace query: the aggregation backward on
// pixel-major (channels-last) feature maps, as two launches (grad_x sweep, Gram pass) plus the ordered
// reduction of a split plane.  Kernels and design notes: film_mean_cl_kernels.hpp.
#include "film_mean_cl_kernels.hpp"

using namespace mrp_host;

namespace {

template <int NT, typename T>
hipError_t launch_dx_cl(bool vec, const ClArgs& a, int64_t grid, size_t lds, hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(T);
  if (vec)
    hipLaunchKernelGGL((mrp::film_bwd_dx_cl<NT, V, T>), dim3((unsigned)grid), dim3(mrp::kBlock), lds, st, a);
  else
    hipLaunchKernelGGL((mrp::film_bwd_dx_cl<NT, 1, T>), dim3((unsigned)grid), dim3(mrp::kBlock), lds, st, a);
  return hipGetLastError();
}

template <typename T>
hipError_t dispatch_dx_cl(int nt, bool vec, const ClArgs& a, int64_t grid, size_t lds, hipStream_t st) {
  switch (nt) {
    case 4: return launch_dx_cl<4, T>(vec, a, grid, lds, st);
    case 8: return launch_dx_cl<8, T>(vec, a, grid, lds, st);
    default: return launch_dx_cl<16, T>(vec, a, grid, lds, st);
  }
}

template <int NT, typename T>
hipError_t launch_gram_cl(bool vec, const ClArgs& a, int64_t items, hipStream_t st) {
  if (vec)
    hipLaunchKernelGGL((mrp::film_bwd_gram_cl<NT, true, T>), dim3((unsigned)(items * a.nseg)), dim3(mrp::kBlock), 0, st, a);
  else
    hipLaunchKernelGGL((mrp::film_bwd_gram_cl<NT, false, T>), dim3((unsigned)(items * a.nseg)), dim3(mrp::kBlock), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.nseg <= 1) return e;
  hipLaunchKernelGGL((mrp::film_gram_finish_cl<NT>), dim3((unsigned)items), dim3(mrp::kBlock), 0, st, a);
  return hipGetLastError();
}

template <typename T>
hipError_t dispatch_gram_cl(int nt, bool vec, const ClArgs& a, int64_t items, hipStream_t st) {
  switch (nt) {
    case 4: return launch_gram_cl<4, T>(vec, a, items, st);
    case 8: return launch_gram_cl<8, T>(vec, a, items, st);
    default: return launch_gram_cl<16, T>(vec, a, items, st);
  }
}

bool gram_wanted(int32_t mode, int32_t num_edges) { return mode != MRP_AGG_COPY_MEAN && num_edges > 0; }

}  // namespace

extern "C" {

int64_t mrp_film_mean_bwd_cl_workspace(int32_t num_graphs, int32_t max_nodes, int32_t graph_kind, int32_t C,
                                       int32_t P, int32_t mode_flags, int32_t want_grad_gb) {
  (void)graph_kind;
  const int32_t mode = mode_flags & ~MRP_AGG_GB_LOGITS;
  if (!want_grad_gb || mode == MRP_AGG_COPY_MEAN) return 0;
  if (num_graphs <= 0 || max_nodes <= 0 || max_nodes > MRP_MAX_NODES || C <= 0 || P <= 0) return 0;
  return cl_gram_geometry(num_graphs, max_nodes, C, P).ws_bytes;
}

int mrp_film_mean_bwd_cl(int32_t dtype, const void* grad_out, int64_t g_node_stride, int64_t g_pixel_stride,
                         const void* x, int64_t x_node_stride, int64_t x_pixel_stride, const float* gb,
                         const int32_t* indptr, const int32_t* src, const int32_t* eid, const int32_t* graph_off,
                         int32_t num_graphs, int32_t max_nodes, int32_t graph_kind, int32_t num_nodes,
                         int32_t num_edges, int32_t C, int32_t P, int32_t mode_flags, void* grad_x,
                         int64_t gx_node_stride, int64_t gx_pixel_stride, const void* grad_x_base,
                         int64_t base_node_stride, int64_t base_pixel_stride, float* grad_gb,
                         const mrp_agg_epilogue_cl* ep, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!cl_dtype_ok(dtype)) return hipErrorInvalidValue;
  const float agg_scale = ep != nullptr ? ep->agg_scale : 1.f;
  const float self_scale = ep != nullptr ? ep->self_scale : 0.f;
  const int32_t logits = (mode_flags & MRP_AGG_GB_LOGITS) ? 1 : 0;
  const int32_t mode = mode_flags & ~MRP_AGG_GB_LOGITS;
  if (!common_args_ok(indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P,
                      mode))
    return hipErrorInvalidValue;
  const bool sized = !(num_graphs == 0 || num_nodes == 0 || max_nodes == 0 || C == 0 || P == 0);
  const bool want_dgb = grad_gb != nullptr && gram_wanted(mode, num_edges) && agg_scale != 0.f && sized;
  const bool want_dx = grad_x != nullptr && sized;
  // MRP_GRAPH_SIMPLE: the rows of grad_gb that no CSR entry names are zero (cleared before the Gram pass)
  const bool zero_dgb = grad_gb != nullptr && num_edges > 0 && C > 0 && (!want_dgb || graph_kind == MRP_GRAPH_SIMPLE);
  hipStream_t st = static_cast<hipStream_t>(stream);

  // every check before the first enqueue
  const int es = cl_elem_size(dtype);
  ClCheck ck{C, P, es};
  ClArgs a = {};
  ClGramGeom gg = {};
  if (want_dx || want_dgb) {
    a.g = ck.add(grad_out, g_node_stride, g_pixel_stride);
    if (want_dx) a.out = ck.add(grad_x, gx_node_stride, gx_pixel_stride);
    if (want_dx && grad_x_base != nullptr) a.base = ck.add(grad_x_base, base_node_stride, base_pixel_stride);
    if (want_dgb) a.x = ck.add(x, x_node_stride, x_pixel_stride);
    if (ck.invalid) return hipErrorInvalidValue;
    if (mode != MRP_AGG_COPY_MEAN && num_edges > 0 && gb == nullptr) return hipErrorInvalidValue;
    if (want_dgb) {
      gg = cl_gram_geometry(num_graphs, max_nodes, C, P);
      if (gg.ws_bytes > 0 && (workspace == nullptr || workspace_bytes < gg.ws_bytes)) return hipErrorInvalidValue;
      if ((int64_t)num_graphs * gg.ncb * gg.nseg > 0x7fffffff) return hipErrorNotSupported;
    }
    if (ck.unsupported) return hipErrorNotSupported;
  }
  if (zero_dgb) {  // gamma/beta do not influence the output: their gradient is zero
    hipError_t e = hipMemsetAsync(grad_gb, 0, (size_t)num_edges * C * 2 * sizeof(float), st);
    if (e != hipSuccess) return e;
  }
  if (!want_dx && !want_dgb) return hipSuccess;

  const int nt = cl_nt_class(max_nodes);
  const int32_t kdeg = MRP_GRAPH_IS_REGULAR(graph_kind) ? MRP_GRAPH_REGULAR_K(graph_kind) : 0;
  a.kind = graph_kind == MRP_GRAPH_COMPLETE ? mrp::kClComplete : mrp::kClCsr;  // the backward's weights are dense
  a.gb = gb;
  a.dgb = grad_gb;
  a.ws = static_cast<float*>(workspace);
  a.indptr = indptr;
  a.src = src;
  a.eid = eid;
  a.goff = graph_off;
  a.C = C;
  a.P = P;
  a.mode = mode;
  a.logits = logits;
  a.kdeg = kdeg;
  a.nmax = max_nodes;
  a.agg_scale = agg_scale;
  a.self_scale = self_scale;

  if (want_dx) {
    const int vecw = 16 / es;
    // x is not read by the sweep: its alignment does not decide the vector path
    ClCheck cv{C, P, es};
    cv.add(grad_out, g_node_stride, g_pixel_stride);
    cv.add(grad_x, gx_node_stride, gx_pixel_stride);
    if (grad_x_base != nullptr) cv.add(grad_x_base, base_node_stride, base_pixel_stride);
    const bool vec = cv.vec && C % vecw == 0;
    const int minc = vec ? vecw : 1;
    int cb = std::max(std::min(64, cl_pow2_ceil(C)), minc);
    while (cb > minc && (int64_t)nt * nt * cb * 4 > 32 * 1024) cb /= 2;  // Wt[u][v][cb]: <= 32 KiB
    const size_t lds = (size_t)nt * nt * cb * 4;
    ClArgs d = a;
    d.cb = cb;
    d.ncb = (C + cb - 1) / cb;
    const int granule = mrp::kBlock / (cb / minc);
    const int64_t per_pixel = (int64_t)max_nodes * cb * es * 2;
    const int min_pixels = (int)std::max<int64_t>(granule, (4 * (int64_t)lds + per_pixel - 1) / per_pixel);
    const int64_t items = (int64_t)num_graphs * d.ncb;
    cl_segments(items, P, granule, min_pixels, d.nseg, d.seglen);
    const int64_t grid = items * d.nseg;
    if (grid > 0x7fffffff) return hipErrorNotSupported;
    hipError_t e;
    switch (dtype) {
      case MRP_DTYPE_F32: e = dispatch_dx_cl<float>(nt, vec, d, grid, lds, st); break;
      case MRP_DTYPE_BF16: e = dispatch_dx_cl<mrp::bf16_t>(nt, vec, d, grid, lds, st); break;
      default: e = dispatch_dx_cl<mrp::f16_t>(nt, vec, d, grid, lds, st); break;
    }
    if (e != hipSuccess) return e;
  }
  if (want_dgb) {
    ClArgs d = a;
    d.cb = 64;
    d.ncb = gg.ncb;
    d.nseg = gg.nseg;
    d.seglen = gg.seglen;
    // the staging loads are 16-byte pieces where x and grad_out allow them
    ClCheck cg{C, P, es};
    cg.add(x, x_node_stride, x_pixel_stride);
    cg.add(grad_out, g_node_stride, g_pixel_stride);
    const bool gvec = cg.vec && C % (16 / es) == 0;
    const int64_t items = (int64_t)num_graphs * gg.ncb;
    switch (dtype) {
      case MRP_DTYPE_F32: return dispatch_gram_cl<float>(nt, gvec, d, items, st);
      case MRP_DTYPE_BF16: return dispatch_gram_cl<mrp::bf16_t>(nt, gvec, d, items, st);
      default: return dispatch_gram_cl<mrp::f16_t>(nt, gvec, d, items, st);
    }
  }
  return hipSuccess;
}

}  // extern "C"
