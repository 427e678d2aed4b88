// film_mean_bwd_launch.hpp — backward launch templates, included by the film_mean_bwd_*.hip parts.
#pragma once
#include "film_mean_kernels.hpp"

namespace mrp_host {

template <int NT, bool COMPLETE, bool DXB>
hipError_t launch_bwd_ntb(const AggArgs& a_in, const Geometry& g, hipStream_t st) {
  if constexpr (NT <= 8) {
    const AggArgs& a = a_in;
    const size_t lds = g.lds;
    if (g.pre2) {  // exactly two slices per lane, both prefetched (film_bwd_plan)
      MRP_LAUNCH((mrp::film_bwd_fused<NT, NT, 4, COMPLETE, DXB, 1, true>), lds);
      return hipGetLastError();
    }
    if (g.vec == 4)
      MRP_LAUNCH((mrp::film_bwd_fused<NT, NT, 4, COMPLETE, DXB>), lds);
    else if (g.vec == 2)
      MRP_LAUNCH((mrp::film_bwd_fused<NT, NT, 2, COMPLETE, DXB>), lds);
    else
      MRP_LAUNCH((mrp::film_bwd_fused<NT, NT, 1, COMPLETE, DXB>), lds);
    return hipGetLastError();
  } else {
    if (a_in.want_dx) {
      const AggArgs& a = a_in;
      const size_t lds = g.lds_dx;
      if (g.vec == 4)
        MRP_LAUNCH((mrp::film_bwd_dx<NT, 4, COMPLETE, DXB>), lds);
      else if (g.vec == 2)
        MRP_LAUNCH((mrp::film_bwd_dx<NT, 2, COMPLETE, DXB>), lds);
      else
        MRP_LAUNCH((mrp::film_bwd_dx<NT, 1, COMPLETE, DXB>), lds);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
    if (a_in.want_dgb) {
      AggArgs a = a_in;
      a.want_dx = 0;
      const size_t lds = g.lds;
      if (g.vec == 4)
        MRP_LAUNCH((mrp::film_bwd_fused<NT, 4, 4, COMPLETE>), lds);
      else if (g.vec == 2)
        MRP_LAUNCH((mrp::film_bwd_fused<NT, 4, 2, COMPLETE>), lds);
      else
        MRP_LAUNCH((mrp::film_bwd_fused<NT, 4, 1, COMPLETE>), lds);
      return hipGetLastError();
    }
    return hipSuccess;
  }
}

// 16-bit features (T = mrp::bf16_t / mrp::f16_t): film_bwd_fused up to 8 nodes; beyond, film_bwd_mfma<..., T>
// where mrp_film_mean_bwd_t chose it (g.mfma_npb, launch_bwd_half_mfma) and else film_bwd_dx + the VB = 4
// Gram pass (no per-edge-slot kernel), slices of 4 elements (8 bytes) or 1, and no PRE2 variant: half of
// the fp32 instantiation set per dtype (1..8 nodes: 64 kernels against 128).
template <typename T, int NT, bool COMPLETE, bool DXB>
hipError_t launch_bwd_half_ntb(const AggArgs& a_in, const Geometry& g, hipStream_t st) {
  if constexpr (NT <= 8) {
    const AggArgs& a = a_in;
    const size_t lds = g.lds;
    if (g.vec == 4)
      MRP_LAUNCH((mrp::film_bwd_fused<NT, NT, 4, COMPLETE, DXB, 1, false, T>), lds);
    else
      MRP_LAUNCH((mrp::film_bwd_fused<NT, NT, 1, COMPLETE, DXB, 1, false, T>), lds);
    return hipGetLastError();
  } else {
    if (a_in.want_dx) {
      const AggArgs& a = a_in;
      const size_t lds = g.lds_dx;
      if (g.vec == 4)
        MRP_LAUNCH((mrp::film_bwd_dx<NT, 4, COMPLETE, DXB, T>), lds);
      else
        MRP_LAUNCH((mrp::film_bwd_dx<NT, 1, COMPLETE, DXB, T>), lds);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
    if (a_in.want_dgb) {
      AggArgs a = a_in;
      a.want_dx = 0;
      const size_t lds = g.lds;
      if (g.vec == 4)
        MRP_LAUNCH((mrp::film_bwd_fused<NT, 4, 4, COMPLETE, false, 1, false, T>), lds);
      else
        MRP_LAUNCH((mrp::film_bwd_fused<NT, 4, 1, COMPLETE, false, 1, false, T>), lds);
      return hipGetLastError();
    }
    return hipSuccess;
  }
}

// film_bwd_mfma<..., T> for graphs of 9..16 nodes, instantiated in film_mean_bwd_half_mfma.hip for
// mrp::bf16_t and mrp::f16_t (12 kernels each: COMPLETE / REGULAR KMAX 4, 8 x grad_x base x blocks per wave)
template <typename T>
hipError_t launch_bwd_half_mfma(bool complete, const AggArgs& a, const Geometry& g, hipStream_t st);

template <typename T, int NT>
hipError_t launch_bwd_half_nt(bool complete, const AggArgs& a, const Geometry& g, hipStream_t st) {
  if (g.kernel == MRP_AGG_KERNEL_FILM_BWD_MFMA) {
    if constexpr (NT > 8) return launch_bwd_half_mfma<T>(complete, a, g, st);
    return hipErrorInvalidValue;  // graphs of <= 8 nodes run film_bwd_fused
  }
  if (g.vec != 4 && g.vec != 1) return hipErrorInvalidValue;
  if (complete)
    return a.dxb ? launch_bwd_half_ntb<T, NT, true, true>(a, g, st) : launch_bwd_half_ntb<T, NT, true, false>(a, g, st);
  return a.dxb ? launch_bwd_half_ntb<T, NT, false, true>(a, g, st) : launch_bwd_half_ntb<T, NT, false, false>(a, g, st);
}

// One case of a 16-bit dispatch switch over the graph size.
#define MRP_HALF_NT_CASE(N)                                                                            \
  case N:                                                                                              \
    return dtype == MRP_DTYPE_BF16 ? launch_bwd_half_nt<mrp::bf16_t, N>(complete, a, g, st)            \
                                   : launch_bwd_half_nt<mrp::f16_t, N>(complete, a, g, st);

template <int NT, int KMAX, bool DXB>
hipError_t launch_bwd_regular(const AggArgs& a, const Geometry& g, hipStream_t st) {
  // VEC 4 would need 4*NT registers more per operand and spills; KMAX 8 only fits at VEC 1
  const size_t lds = g.lds;
  bool done = false;
  if constexpr (KMAX <= 4) {
    if (g.vec == 2) {
      MRP_LAUNCH((mrp::film_bwd_regular<NT, KMAX, 2, DXB>), lds);
      done = true;
    }
  }
  if (!done) MRP_LAUNCH((mrp::film_bwd_regular<NT, KMAX, 1, DXB>), lds);
  return hipGetLastError();
}

// film_bwd_mfma (mrp_film_mean_bwd_ex chose it and set g.mfma_npb, g.cpb = 4 x blocks per wave x
// channels per block)
template <bool COMPLETE, int NPB, int KMAX>
hipError_t launch_bwd_mfma_k(const AggArgs& a, const Geometry& g, hipStream_t st) {
  const size_t lds = g.lds;
  const int cpw = g.cpb / (4 * (16 / NPB));
  if (a.dxb) {
    if (cpw == 1)
      MRP_LAUNCH((mrp::film_bwd_mfma<COMPLETE, NPB, KMAX, true, 1>), lds);
    else
      MRP_LAUNCH((mrp::film_bwd_mfma<COMPLETE, NPB, KMAX, true, 2>), lds);
  } else {
    if (cpw == 1)
      MRP_LAUNCH((mrp::film_bwd_mfma<COMPLETE, NPB, KMAX, false, 1>), lds);
    else
      MRP_LAUNCH((mrp::film_bwd_mfma<COMPLETE, NPB, KMAX, false, 2>), lds);
  }
  return hipGetLastError();
}


template <int NT, bool COMPLETE>
hipError_t launch_bwd_mfma(const AggArgs& a, const Geometry& g, hipStream_t st) {
  if constexpr (COMPLETE) {
    if constexpr (NT > 8) return launch_bwd_mfma_k<true, 16, 1>(a, g, st);
    return hipErrorInvalidValue;  // complete graphs of <= 8 nodes run film_bwd_fused
  } else {
    if constexpr (NT > 8) {
      if (g.kmax == 4) return launch_bwd_mfma_k<false, 16, 4>(a, g, st);
      if (g.kmax == 8) return launch_bwd_mfma_k<false, 16, 8>(a, g, st);
    }
    return hipErrorInvalidValue;
  }
}

template <int NT, bool COMPLETE>
hipError_t launch_bwd_nt(const AggArgs& a, const Geometry& g, hipStream_t st) {
  // the kernel film_bwd_plan chose
  if (g.kernel == MRP_AGG_KERNEL_FILM_BWD_MFMA) return launch_bwd_mfma<NT, COMPLETE>(a, g, st);
  if (g.kernel == MRP_AGG_KERNEL_FILM_BWD_REGULAR) {
    // regular in-degree (k-NN): per-edge-slot Gram, one sweep
    if constexpr (NT > 8 && !COMPLETE) {
      if (g.kmax == 4)
        return a.dxb ? launch_bwd_regular<NT, 4, true>(a, g, st) : launch_bwd_regular<NT, 4, false>(a, g, st);
      if (g.kmax == 8)
        return a.dxb ? launch_bwd_regular<NT, 8, true>(a, g, st) : launch_bwd_regular<NT, 8, false>(a, g, st);
    }
    return hipErrorInvalidValue;
  }
  if (g.kernel != (NT <= 8 ? MRP_AGG_KERNEL_FILM_BWD_FUSED : MRP_AGG_KERNEL_FILM_BWD_DX_GRAM))
    return hipErrorInvalidValue;
  return a.dxb ? launch_bwd_ntb<NT, COMPLETE, true>(a, g, st) : launch_bwd_ntb<NT, COMPLETE, false>(a, g, st);
}

}  // namespace mrp_host
