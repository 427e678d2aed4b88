// film_mean_bwd_rows_mfma.hip — the matrix-core backward (film_bwd_mfma) in its CSR-row form: graphs of
// kind MRP_GRAPH_SIMPLE (no two CSR entries share a (source, destination) pair; range-limited and drop-out
// frames) of 9..16 nodes, fp32 / bf16 / fp16 features.  A translation unit of its own so its 12 kernels
// (3 dtypes x grad_x base x blocks per wave) compile beside the others.
#include "film_mean_bwd_launch.hpp"

namespace mrp_host {

namespace {

template <typename T>
hipError_t launch_bwd_rows_mfma(const AggArgs& a, const Geometry& g, hipStream_t st) {
  const size_t lds = g.lds;
  const int cpw = g.cpb / 4;
  if (a.dxb) {
    if (cpw == 1)
      MRP_LAUNCH((mrp::film_bwd_mfma<false, 16, 16, true, 1, T>), lds);
    else
      MRP_LAUNCH((mrp::film_bwd_mfma<false, 16, 16, true, 2, T>), lds);
  } else {
    if (cpw == 1)
      MRP_LAUNCH((mrp::film_bwd_mfma<false, 16, 16, false, 1, T>), lds);
    else
      MRP_LAUNCH((mrp::film_bwd_mfma<false, 16, 16, false, 2, T>), lds);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t dispatch_bwd_rows_mfma(int dtype, const AggArgs& a, const Geometry& g, hipStream_t st) {
  if (g.mfma_npb != 16 || g.kmax != 16 || (g.cpb != 4 && g.cpb != 8) || a.nmax <= 8) return hipErrorInvalidValue;
  if (dtype == MRP_DTYPE_F32) return launch_bwd_rows_mfma<float>(a, g, st);
  if (dtype == MRP_DTYPE_BF16) return launch_bwd_rows_mfma<mrp::bf16_t>(a, g, st);
  if (dtype == MRP_DTYPE_F16) return launch_bwd_rows_mfma<mrp::f16_t>(a, g, st);
  return hipErrorInvalidValue;
}

}  // namespace mrp_host
