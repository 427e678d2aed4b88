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
  const size_t lds = g.lds;
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
  if (g.kernel == MRP_AGG_KERNEL_FILM_FWD_REGULAR) {
    // per-edge-slot weights for uniform in-degree (k-NN frames)
    if constexpr (!COMPLETE) {
      if (g.kmax == 4) return launch_fwd_regular<T, NT, 4>(a, g, st);
      if (g.kmax == 8) return launch_fwd_regular<T, NT, 8>(a, g, st);
    }
    return hipErrorInvalidValue;
  }
  if (g.kernel != MRP_AGG_KERNEL_FILM_FWD) return hipErrorInvalidValue;
  const size_t lds = g.lds;
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

// The forward's launch plan (film_mean_fwd.hip): validation, kernel choice, slice width, geometry, plane
// split and dynamic LDS for features of `elem` bytes per element.  No GPU call; the pointers are looked
// at for alignment and NULL only.  xelem: bytes per element of x where they differ from `elem` (1: the FP8
// messages of film_mean_fwd_q.hip; 0: x holds `elem`-byte elements like every other feature tensor).  Returns the code the entry points return before launching;
// g.kernel == MRP_AGG_KERNEL_NONE with hipSuccess: nothing to launch.  Behind both film_fwd_impl and
// mrp_film_mean_fwd_plan.
int film_fwd_plan(size_t elem, const void* x, int64_t x_node_stride, const float* gb, const int32_t* indptr,
                  const int32_t* src, const int32_t* eid, const int32_t* graph_off, int32_t num_graphs,
                  int32_t max_nodes, int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P,
                  int32_t mode_flags, void* out, int64_t out_node_stride, const mrp_agg_epilogue* ep, AggArgs& a,
                  Geometry& g, size_t xelem = 0);

// The forward behind mrp_film_mean_fwd{,_ex,_t} and mrp_film_mean_cat_fwd; x, out and the epilogue's
// x0 / xcopy hold elements of T, strides in elements.
template <typename T>
int film_fwd_impl(const T* x, int64_t x_node_stride, const float* gb, const int32_t* indptr, const int32_t* src,
                  const int32_t* eid, const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                  int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t mode_flags,
                  T* out, int64_t out_node_stride, const mrp_agg_epilogue* ep, void* stream) {
  AggArgs a = {};
  Geometry g;
  const int rc = film_fwd_plan(sizeof(T), x, x_node_stride, gb, indptr, src, eid, graph_off, num_graphs, max_nodes,
                               graph_kind, num_nodes, num_edges, C, P, mode_flags, out, out_node_stride, ep, a, g);
  if (rc != hipSuccess || g.kernel == MRP_AGG_KERNEL_NONE) return rc;
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
