// film_mean_bwd_half_mfma.hip — the matrix-core backward (film_bwd_mfma) for 16-bit features, graphs of
// 9..16 nodes (see film_mean_bwd.hip and launch_bwd_half_nt).  A translation unit of its own so its 24
// kernels compile beside the others.
#include "film_mean_bwd_launch.hpp"

namespace mrp_host {

namespace {

// launch_bwd_mfma_k for storage type T, 16-node blocks (g.cpb = 4 x blocks per wave)
template <typename T, bool COMPLETE, int KMAX>
hipError_t launch_bwd_half_mfma_k(const AggArgs& a, const Geometry& g, hipStream_t st) {
  const size_t lds = g.lds;
  const int cpw = g.cpb / 4;
  if (a.dxb) {
    if (cpw == 1)
      MRP_LAUNCH((mrp::film_bwd_mfma<COMPLETE, 16, KMAX, true, 1, T>), lds);
    else
      MRP_LAUNCH((mrp::film_bwd_mfma<COMPLETE, 16, KMAX, true, 2, T>), lds);
  } else {
    if (cpw == 1)
      MRP_LAUNCH((mrp::film_bwd_mfma<COMPLETE, 16, KMAX, false, 1, T>), lds);
    else
      MRP_LAUNCH((mrp::film_bwd_mfma<COMPLETE, 16, KMAX, false, 2, T>), lds);
  }
  return hipGetLastError();
}

}  // namespace

template <typename T>
hipError_t launch_bwd_half_mfma(bool complete, const AggArgs& a, const Geometry& g, hipStream_t st) {
  if (g.mfma_npb != 16 || (g.cpb != 4 && g.cpb != 8)) return hipErrorInvalidValue;
  if (complete) return launch_bwd_half_mfma_k<T, true, 1>(a, g, st);
  if (g.kmax == 4) return launch_bwd_half_mfma_k<T, false, 4>(a, g, st);
  if (g.kmax == 8) return launch_bwd_half_mfma_k<T, false, 8>(a, g, st);
  return hipErrorInvalidValue;
}

template hipError_t launch_bwd_half_mfma<mrp::bf16_t>(bool, const AggArgs&, const Geometry&, hipStream_t);
template hipError_t launch_bwd_half_mfma<mrp::f16_t>(bool, const AggArgs&, const Geometry&, hipStream_t);

}  // namespace mrp_host
