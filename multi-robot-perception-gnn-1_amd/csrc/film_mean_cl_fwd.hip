// film_mean_cl_fwd.hip — mrp_film_mean_fwd_cl: the aggregation forward on pixel-major (channels-last)
// feature maps.  Kernels and design notes: film_mean_cl_kernels.hpp.
#include "film_mean_cl_kernels.hpp"

using namespace mrp_host;

namespace {

template <int NT, int VEC, typename T>
hipError_t launch_fwd_cl(const ClArgs& a, int64_t grid, size_t lds, hipStream_t st) {
  constexpr int PIX = NT * VEC <= 32 ? 2 : 1;  // x of PIX pixels in registers: at most 64 VGPRs
  if (a.kind == mrp::kClComplete)
    hipLaunchKernelGGL((mrp::film_fwd_cl<NT, VEC, PIX, true, T>), dim3((unsigned)grid), dim3(mrp::kBlock), lds, st, a);
  else
    hipLaunchKernelGGL((mrp::film_fwd_cl<NT, VEC, PIX, false, T>), dim3((unsigned)grid), dim3(mrp::kBlock), lds, st, a);
  return hipGetLastError();
}

template <typename T>
hipError_t dispatch_fwd_cl(int nt, bool vec, const ClArgs& a, int64_t grid, size_t lds, hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(T);
  switch (nt) {
    case 4: return vec ? launch_fwd_cl<4, V, T>(a, grid, lds, st) : launch_fwd_cl<4, 1, T>(a, grid, lds, st);
    case 8: return vec ? launch_fwd_cl<8, V, T>(a, grid, lds, st) : launch_fwd_cl<8, 1, T>(a, grid, lds, st);
    default: return vec ? launch_fwd_cl<16, V, T>(a, grid, lds, st) : launch_fwd_cl<16, 1, T>(a, grid, lds, st);
  }
}

}  // namespace

extern "C" int mrp_film_mean_fwd_cl(int32_t dtype, const void* x, int64_t x_node_stride, int64_t x_pixel_stride,
                                    const float* gb, const int32_t* indptr, const int32_t* src, const int32_t* eid,
                                    const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                                    int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P,
                                    int32_t mode_flags, void* out, int64_t out_node_stride, int64_t out_pixel_stride,
                                    const mrp_agg_epilogue_cl* ep, void* stream) {
  if (!cl_dtype_ok(dtype)) return hipErrorInvalidValue;
  const int32_t logits = (mode_flags & MRP_AGG_GB_LOGITS) ? 1 : 0;
  const int32_t mode = mode_flags & ~MRP_AGG_GB_LOGITS;
  if (!common_args_ok(indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P,
                      mode))
    return hipErrorInvalidValue;
  if (num_graphs == 0 || num_nodes == 0 || max_nodes == 0 || C == 0 || P == 0) return hipSuccess;
  const int es = cl_elem_size(dtype);
  ClCheck ck{C, P, es};
  ClArgs a = {};
  a.x = ck.add(x, x_node_stride, x_pixel_stride);
  a.out = ck.add(out, out_node_stride, out_pixel_stride);
  a.agg_scale = 1.f;
  if (ep != nullptr) {
    a.agg_scale = ep->agg_scale;
    a.self_scale = ep->self_scale;
    if (ep->x0 != nullptr) {
      a.x0 = ck.add(ep->x0, ep->x0_node_stride, ep->x0_pixel_stride);
      a.x0_scale = ep->x0_scale;
    }
    if (ep->xcopy != nullptr) a.xc = ck.add(ep->xcopy, ep->xcopy_node_stride, ep->xcopy_pixel_stride);
  }
  if (ck.invalid) return hipErrorInvalidValue;
  if (mode != MRP_AGG_COPY_MEAN && num_edges > 0 && gb == nullptr) return hipErrorInvalidValue;
  if (ck.unsupported) return hipErrorNotSupported;

  const int nt = cl_nt_class(max_nodes);
  const int vecw = 16 / es;
  const bool vec = ck.vec && C % vecw == 0;
  const int32_t kdeg = MRP_GRAPH_IS_REGULAR(graph_kind) ? MRP_GRAPH_REGULAR_K(graph_kind) : 0;
  a.kind = graph_kind == MRP_GRAPH_COMPLETE ? mrp::kClComplete
                                            : (kdeg >= 1 && kdeg <= 8 ? mrp::kClSlots : mrp::kClCsr);
  // slots of one graph: the LDS tile is [slot][cb] (gamma, beta) pairs
  int64_t slots = a.kind == mrp::kClComplete ? (int64_t)max_nodes * (max_nodes - 1)
                  : a.kind == mrp::kClSlots  ? (int64_t)max_nodes * kdeg
                                             : std::min<int64_t>((int64_t)max_nodes * max_nodes, num_edges);
  const int tables = nt == 4 ? mrp::ClTables<4>::kBytes : (nt == 8 ? mrp::ClTables<8>::kBytes : mrp::ClTables<16>::kBytes);
  // channels per workgroup: 64 (a pixel's row piece is 128 bytes of a 16-bit type, 256 of fp32), halved
  // until the tile leaves room for two workgroups per CU's 160 KiB (240 slots: 32 channels)
  const int minc = vec ? vecw : 1;
  int cb = std::max(std::min(64, cl_pow2_ceil(C)), minc);
  while (cb > minc && tables + slots * cb * 8 > 64 * 1024 - 256) cb /= 2;
  const size_t lds = (size_t)tables + (size_t)std::max<int64_t>(slots, 1) * cb * 8;
  if (lds > 64 * 1024) return hipErrorNotSupported;
  a.cb = cb;
  a.ncb = (C + cb - 1) / cb;
  const int lanes = cb / (vec ? vecw : 1);  // lanes per pixel
  const int pix = nt * (vec ? vecw : 1) <= 32 ? 2 : 1;
  const int granule = (mrp::kBlock / lanes) * pix;
  // a segment no shorter than a few tiles' worth of features, so the prologue's gamma/beta stay a
  // fraction of the bytes a workgroup moves
  const int64_t per_pixel = (int64_t)max_nodes * cb * es * 2;
  const int min_pixels = (int)std::max<int64_t>(granule, (4 * (int64_t)lds + per_pixel - 1) / per_pixel);
  const int64_t items = (int64_t)num_graphs * a.ncb;
  cl_segments(items, P, granule, min_pixels, a.nseg, a.seglen);
  const int64_t grid = items * a.nseg;
  if (grid > 0x7fffffff) return hipErrorNotSupported;
  a.gb = gb;
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
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case MRP_DTYPE_F32: return dispatch_fwd_cl<float>(nt, vec, a, grid, lds, st);
    case MRP_DTYPE_BF16: return dispatch_fwd_cl<mrp::bf16_t>(nt, vec, a, grid, lds, st);
    default: return dispatch_fwd_cl<mrp::f16_t>(nt, vec, a, grid, lds, st);
  }
}
