// film_mean_bwd_half_9_12.hip — backward launches for 16-bit features, graphs of 9..12 nodes
// (see film_mean_bwd.hip and launch_bwd_half_ntb).
#include "film_mean_bwd_launch.hpp"

namespace mrp_host {

hipError_t dispatch_bwd_half_9_12(int dtype, int nt, bool complete, const AggArgs& a, const Geometry& g,
                                    hipStream_t st) {
  if (dtype != MRP_DTYPE_BF16 && dtype != MRP_DTYPE_F16) return hipErrorInvalidValue;
  switch (nt) {
    MRP_HALF_NT_CASE(9)
    MRP_HALF_NT_CASE(10)
    MRP_HALF_NT_CASE(11)
    MRP_HALF_NT_CASE(12)
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mrp_host
