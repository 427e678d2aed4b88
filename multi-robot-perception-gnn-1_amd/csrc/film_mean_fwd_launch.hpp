// film_mean_fwd_launch.hpp — forward launch templates over the feature storage type T, included by
// film_mean_fwd.hip (float) and film_mean_fwd_{bf16,f16}.hip.  Kernels: film_mean_kernels.hpp.
#pragma once
#include "film_mean_kernels.hpp"

namespace mrp_host {

// Slice widths (elements of T) the forward is instantiated for.  float: 4 / 2 / 1 (16, 8, 4 bytes).
// 16-bit: 8 (graphs of <= 8 nodes) / 4 / 1 (16, 8, 2 bytes), and neither the compile-time k-NN(4) degree nor any MODE but the
// reference's own at 16-byte slices: the specialised variants only save ALU, the 16-bit sweep moves half
// the bytes, and every instantiation is build time.
template <typename T>
constexpr bool kHalfIo = sizeof(T) == 2;

template <typename T, int NT, int KMAX>
hipError_t launch_fwd_regular(const AggArgs& a, const Geometry& g, hipStream_t st) {
  const size_t lds = lds_fwd_regular<NT, KMAX>(g.cpb);
  if constexpr (kHalfIo<T>) {
    if (g.vec == 8 && NT <= 8) {
      if constexpr (NT <= 8) MRP_LAUNCH((mrp::film_fwd_regular<NT, KMAX, 8, 0, T>), lds);
    } else if (g.vec == 4)
      MRP_LAUNCH((mrp::film_fwd_regular<NT, KMAX, 4, 0, T>), lds);
    else if (g.vec == 1)
      MRP_LAUNCH((mrp::film_fwd_regular<NT, KMAX, 1, 0, T>), lds);
    else
      return hipErrorInvalidValue;
    return hipGetLastError();
  } else {
    // k-NN(4) in a mean mode (BASELINE configs[4]): compile-time degree, exact division by 4
    if constexpr (KMAX == 4) {
      if (g.vec == 4 && a.kdeg == 4 && a.mode != MRP_AGG_FILM_SUM) {
        MRP_LAUNCH((mrp::film_fwd_regular<NT, KMAX, 4, 4>), lds);
        return hipGetLastError();
      }
    }
    if (g.vec == 4)
      MRP_LAUNCH((mrp::film_fwd_regular<NT, KMAX, 4>), lds);
    else if (g.vec == 1)
      MRP_LAUNCH((mrp::film_fwd_regular<NT, KMAX, 1>), lds);
    else
      return hipErrorInvalidValue;
    return hipGetLastError();
  }
}

template <typename T, int NT, bool COMPLETE>
hipError_t launch_fwd_nt(const AggArgs& a, const Geometry& g, hipStream_t st) {
  if constexpr (!COMPLETE) {
    // per-edge-slot weights for uniform in-degree (k-NN frames)
    if (a.kdeg >= 1 && a.kdeg <= 4) return launch_fwd_regular<T, NT, 4>(a, g, st);
    if (a.kdeg >= 5 && a.kdeg <= 8) return launch_fwd_regular<T, NT, 8>(a, g, st);
  }
  const size_t lds = lds_fwd<NT>(g.cpb);
  if constexpr (kHalfIo<T>) {
    if constexpr (COMPLETE && NT >= 2 && NT <= 8) {
      if (g.vec == 8 && a.mode == MRP_AGG_FILM_MEAN) {
        MRP_LAUNCH((mrp::film_fwd<NT, 8, true, MRP_AGG_FILM_MEAN, T>), lds);
        return hipGetLastError();
      }
    }
    if (g.vec == 8 && NT <= 8) {
      if constexpr (NT <= 8) MRP_LAUNCH((mrp::film_fwd<NT, 8, COMPLETE, -1, T>), lds);
    } else if (g.vec == 4)
      MRP_LAUNCH((mrp::film_fwd<NT, 4, COMPLETE, -1, T>), lds);
    else if (g.vec == 1)
      MRP_LAUNCH((mrp::film_fwd<NT, 1, COMPLETE, -1, T>), lds);
    else
      return hipErrorInvalidValue;
    return hipGetLastError();
  } else {
    if constexpr (COMPLETE && NT >= 2 && NT <= 8) {
      // the reference's own configuration: mode and mean divisor compile-time (film_fwd MODE)
      if (g.vec == 4 && a.mode == MRP_AGG_FILM_MEAN) {
        MRP_LAUNCH((mrp::film_fwd<NT, 4, true, MRP_AGG_FILM_MEAN>), lds);
        return hipGetLastError();
      }
      if (g.vec == 2 && a.mode == MRP_AGG_FILM_MEAN) {
        MRP_LAUNCH((mrp::film_fwd<NT, 2, true, MRP_AGG_FILM_MEAN>), lds);
        return hipGetLastError();
      }
    }
    if (g.vec == 4)
      MRP_LAUNCH((mrp::film_fwd<NT, 4, COMPLETE>), lds);
    else if (g.vec == 2)
      MRP_LAUNCH((mrp::film_fwd<NT, 2, COMPLETE>), lds);
    else if (g.vec == 1)
      MRP_LAUNCH((mrp::film_fwd<NT, 1, COMPLETE>), lds);
    else
      return hipErrorInvalidValue;
    return hipGetLastError();
  }
}

template <typename T>
hipError_t dispatch_fwd(int nt, bool complete, const AggArgs& a, const Geometry& g, hipStream_t st) {
#define MRP_FWD_CASE(N) \
  case N: return complete ? launch_fwd_nt<T, N, true>(a, g, st) : launch_fwd_nt<T, N, false>(a, g, st);
  switch (nt) {
    MRP_FWD_CASE(1) MRP_FWD_CASE(2) MRP_FWD_CASE(3) MRP_FWD_CASE(4) MRP_FWD_CASE(5) MRP_FWD_CASE(6)
    MRP_FWD_CASE(7) MRP_FWD_CASE(8) MRP_FWD_CASE(9) MRP_FWD_CASE(10) MRP_FWD_CASE(11) MRP_FWD_CASE(12)
    MRP_FWD_CASE(13) MRP_FWD_CASE(14) MRP_FWD_CASE(15) MRP_FWD_CASE(16)
    default: return hipErrorInvalidValue;
  }
#undef MRP_FWD_CASE
}

// Widest slice (elements) every feature tensor of a call allows: P and the node strides multiples of
// it, the pointers aligned to its bytes.
struct SliceCheck {
  int64_t strides = 0;   // OR of P and the node strides
  uintptr_t ptrs = 0;    // OR of the pointers
  void add(const void* p, int64_t node_stride) {
    strides |= node_stride;
    ptrs |= reinterpret_cast<uintptr_t>(p);
  }
  bool ok(int vec, size_t elem) const { return strides % vec == 0 && ptrs % (vec * elem) == 0; }
};

// The forward behind mrp_film_mean_fwd{,_ex,_t} and mrp_film_mean_cat_fwd; x, out and the epilogue's
// x0 / xcopy hold elements of T, strides in elements.
template <typename T>
int film_fwd_impl(const T* x, int64_t x_node_stride, const float* gb, const int32_t* indptr, const int32_t* src,
                  const int32_t* eid, const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                  int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t mode_flags,
                  T* out, int64_t out_node_stride, const mrp_agg_epilogue* ep, void* stream) {
  T* xcopy = ep != nullptr ? reinterpret_cast<T*>(ep->xcopy) : nullptr;
  const int64_t xcopy_node_stride = ep != nullptr ? ep->xcopy_node_stride : 0;
  const T* x0 = ep != nullptr ? reinterpret_cast<const T*>(ep->x0) : nullptr;
  const int64_t x0_node_stride = ep != nullptr ? ep->x0_node_stride : 0;
  const int32_t logits = (mode_flags & MRP_AGG_GB_LOGITS) ? 1 : 0;
  const int32_t mode = mode_flags & ~MRP_AGG_GB_LOGITS;
  if (!common_args_ok(indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P,
                      mode))
    return hipErrorInvalidValue;
  if (num_graphs == 0 || num_nodes == 0 || max_nodes == 0 || C == 0 || P == 0) return hipSuccess;
  const int64_t plane = (int64_t)C * P;
  if (x == nullptr || out == nullptr || x_node_stride < plane || out_node_stride < plane)
    return hipErrorInvalidValue;
  if (mode != MRP_AGG_COPY_MEAN && num_edges > 0 && gb == nullptr) return hipErrorInvalidValue;
  if (xcopy != nullptr && xcopy_node_stride < plane) return hipErrorInvalidValue;
  if (x0 != nullptr && x0_node_stride < plane) return hipErrorInvalidValue;
  SliceCheck sc;
  sc.strides = P;
  sc.add(x, x_node_stride);
  sc.add(out, out_node_stride);
  if (xcopy != nullptr) sc.add(xcopy, xcopy_node_stride);
  if (x0 != nullptr) sc.add(x0, x0_node_stride);
  const int32_t kdeg = MRP_GRAPH_IS_REGULAR(graph_kind) ? MRP_GRAPH_REGULAR_K(graph_kind) : 0;
  const bool regular = kdeg >= 1 && kdeg <= 8;
  const Tuning& tu = tuning();
  int fvec, rvec;  // slice width of film_fwd / film_fwd_regular
  if constexpr (kHalfIo<T>) {
    // 16-byte slices of 8 elements (graphs of <= 8 nodes: beyond, 8 slices of 16 sources are 128 live
    // registers before the first product), else 8-byte slices of 4, else single elements
    fvec = rvec = (max_nodes <= 8 && sc.ok(8, sizeof(T))) ? 8 : (sc.ok(4, sizeof(T)) ? 4 : 1);
  } else {
    // 16-byte slices beat 8-byte ones at every measured size (tools/kernel_lab.hip product sweep)
    const bool vec4 = sc.ok(4, sizeof(T));
    fvec = vec4 ? (P < tu.fwd_vec2_below ? 2 : 4) : 1;
    rvec = vec4 ? 4 : 1;
  }
  Geometry g = regular ? make_geometry(C, P, rvec, tu.fwd_regular_lo, tu.fwd_regular_hi, tu.fwd_regular_cap)
                       : make_geometry(C, P, fvec, tu.fwd_lo, tu.fwd_hi, tu.fwd_cap);
  // COMPLETE graphs: one slice per lane, the plane split over ceil(PV / lpc) workgroups (their
  // prologue is one round of independent gamma/beta loads, hidden under the first slice).  CSR
  // graphs keep whole planes: their prologue walks the CSR (dependent loads) and a split repeats it
  // per segment (k-NN(4) N=16 C=1024 16x16: 304 us split vs 225 us whole)
  const int32_t pv = P / g.vec;
  const int32_t psplit = (graph_kind == MRP_GRAPH_COMPLETE || (regular && tu.fwd_regular_split))
                             ? (pv + g.lpc - 1) / g.lpc
                             : 1;
  g.grid = (int64_t)num_graphs * g.ncb * psplit;
  if (g.grid > 0x7fffffff) return hipErrorInvalidValue;
  AggArgs a = {};
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
  a.PV = P / g.vec;
  a.mode = mode;
  a.lpc = g.lpc;
  a.cpb = g.cpb;
  a.ncb = g.ncb;
  a.logits = logits;
  a.xc = xcopy;
  a.xcs = xcopy_node_stride;
  a.psplit = psplit;
  a.kdeg = kdeg;
  a.agg_scale = 1.f;
  if (ep != nullptr) {
    a.agg_scale = ep->agg_scale;
    a.self_scale = ep->self_scale;
    a.x0 = x0;
    a.x0s = x0_node_stride;
    a.x0_scale = ep->x0_scale;
    a.epi = (ep->agg_scale != 1.f || ep->self_scale != 0.f || x0 != nullptr) ? 1 : 0;
  }
  return dispatch_fwd<T>(max_nodes, graph_kind == MRP_GRAPH_COMPLETE, a, g, static_cast<hipStream_t>(stream));
}

// 16-bit entry points, one translation unit each (film_mean_fwd_{bf16,f16}.hip)
int film_fwd_bf16(const void* x, int64_t x_node_stride, const float* gb, const int32_t* indptr, const int32_t* src,
                  const int32_t* eid, const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                  int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t mode_flags,
                  void* out, int64_t out_node_stride, const mrp_agg_epilogue* ep, void* stream);
int film_fwd_f16(const void* x, int64_t x_node_stride, const float* gb, const int32_t* indptr, const int32_t* src,
                 const int32_t* eid, const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                 int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t mode_flags,
                 void* out, int64_t out_node_stride, const mrp_agg_epilogue* ep, void* stream);

}  // namespace mrp_host
