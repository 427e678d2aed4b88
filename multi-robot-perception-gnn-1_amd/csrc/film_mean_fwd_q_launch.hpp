// film_mean_fwd_q_launch.hpp — launch templates of the FP8-message forward (mrp_film_mean_fwd_q) over the
// output storage type T, included by film_mean_fwd_q.hip (float) and film_mean_fwd_q_{bf16,f16}.hip.
// Kernels: film_fwd / film_fwd_regular of film_mean_kernels.hpp with TX = q8_t.
//
// Instantiation set per output type: the run-time-mode kernels, the format (E4M3 / E5M2) a wave-uniform switch
// inside the load, slice widths 8 (<= 8 nodes, 16-bit outputs) / 4 / 1 — plus the two specialisations whose
// only effect is to replace the mean's IEEE division (about 10 instructions per element, as much ALU as the
// FiLM terms themselves once the loads are a quarter of the bytes): the reference's own configuration
// (COMPLETE, film_mean, 2..8 nodes: MODE-specialised film_fwd at 8- and 4-element slices) and k-NN(4) in a
// mean mode (compile-time degree KC = 4 at 4-element slices).  Same bits either way (fast_math.hpp).
#pragma once
#include "film_mean_fwd_launch.hpp"

namespace mrp_host {

template <typename T, int NT, int KMAX>
hipError_t launch_fwd_q_regular(const AggArgs& a, const Geometry& g, hipStream_t st) {
  const size_t lds = g.lds;
  // k-NN(4) in a mean mode: compile-time degree, exact division by 4
  if constexpr (KMAX == 4) {
    if (g.vec == 4 && a.kdeg == 4 && a.mode != MRP_AGG_FILM_SUM) {
      MRP_LAUNCH((mrp::film_fwd_regular<NT, KMAX, 4, 4, T, mrp::q8_t>), lds);
      return hipGetLastError();
    }
  }
  if (g.vec == 8) {
    if constexpr (NT <= 8 && kHalfIo<T>)
      MRP_LAUNCH((mrp::film_fwd_regular<NT, KMAX, 8, 0, T, mrp::q8_t>), lds);
    else
      return hipErrorInvalidValue;
  } else if (g.vec == 4)
    MRP_LAUNCH((mrp::film_fwd_regular<NT, KMAX, 4, 0, T, mrp::q8_t>), lds);
  else if (g.vec == 1)
    MRP_LAUNCH((mrp::film_fwd_regular<NT, KMAX, 1, 0, T, mrp::q8_t>), lds);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

template <typename T, int NT, bool COMPLETE>
hipError_t launch_fwd_q_nt(const AggArgs& a, const Geometry& g, hipStream_t st) {
  if (g.kernel == MRP_AGG_KERNEL_FILM_FWD_REGULAR) {
    if constexpr (!COMPLETE) {
      if (g.kmax == 4) return launch_fwd_q_regular<T, NT, 4>(a, g, st);
      if (g.kmax == 8) return launch_fwd_q_regular<T, NT, 8>(a, g, st);
    }
    return hipErrorInvalidValue;
  }
  if (g.kernel != MRP_AGG_KERNEL_FILM_FWD) return hipErrorInvalidValue;
  const size_t lds = g.lds;
  if constexpr (COMPLETE && NT >= 2 && NT <= 8) {
    // the reference's own configuration: mode and mean divisor compile-time (film_fwd MODE)
    if (a.mode == MRP_AGG_FILM_MEAN && g.vec == 4) {
      MRP_LAUNCH((mrp::film_fwd<NT, 4, true, MRP_AGG_FILM_MEAN, T, mrp::q8_t>), lds);
      return hipGetLastError();
    }
    if constexpr (kHalfIo<T>) {
      if (a.mode == MRP_AGG_FILM_MEAN && g.vec == 8) {
        MRP_LAUNCH((mrp::film_fwd<NT, 8, true, MRP_AGG_FILM_MEAN, T, mrp::q8_t>), lds);
        return hipGetLastError();
      }
    }
  }
  if (g.vec == 8) {
    if constexpr (NT <= 8 && kHalfIo<T>)
      MRP_LAUNCH((mrp::film_fwd<NT, 8, COMPLETE, -1, T, mrp::q8_t>), lds);
    else
      return hipErrorInvalidValue;
  } else if (g.vec == 4)
    MRP_LAUNCH((mrp::film_fwd<NT, 4, COMPLETE, -1, T, mrp::q8_t>), lds);
  else if (g.vec == 1)
    MRP_LAUNCH((mrp::film_fwd<NT, 1, COMPLETE, -1, T, mrp::q8_t>), lds);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

template <typename T>
hipError_t dispatch_fwd_q(int nt, bool complete, const AggArgs& a, const Geometry& g, hipStream_t st) {
#define MRP_FWD_Q_CASE(N) \
  case N: return complete ? launch_fwd_q_nt<T, N, true>(a, g, st) : launch_fwd_q_nt<T, N, false>(a, g, st);
  switch (nt) {
    MRP_FWD_Q_CASE(1) MRP_FWD_Q_CASE(2) MRP_FWD_Q_CASE(3) MRP_FWD_Q_CASE(4) MRP_FWD_Q_CASE(5) MRP_FWD_Q_CASE(6)
    MRP_FWD_Q_CASE(7) MRP_FWD_Q_CASE(8) MRP_FWD_Q_CASE(9) MRP_FWD_Q_CASE(10) MRP_FWD_Q_CASE(11) MRP_FWD_Q_CASE(12)
    MRP_FWD_Q_CASE(13) MRP_FWD_Q_CASE(14) MRP_FWD_Q_CASE(15) MRP_FWD_Q_CASE(16)
    default: return hipErrorInvalidValue;
  }
#undef MRP_FWD_Q_CASE
}

// per-output-type dispatch, one translation unit each (they compile in parallel)
hipError_t dispatch_fwd_q_f32(int nt, bool complete, const AggArgs& a, const Geometry& g, hipStream_t st);
hipError_t dispatch_fwd_q_bf16(int nt, bool complete, const AggArgs& a, const Geometry& g, hipStream_t st);
hipError_t dispatch_fwd_q_f16(int nt, bool complete, const AggArgs& a, const Geometry& g, hipStream_t st);

}  // namespace mrp_host
