// film_mean_bwd_half_13_16.hip — backward launches for 16-bit features, graphs of 13..16 nodes
// (see film_mean_bwd.hip and launch_bwd_half_ntb).
#include "film_mean_bwd_launch.hpp"

namespace mrp_host {

hipError_t dispatch_bwd_half_13_16(int dtype, int nt, bool complete, const AggArgs& a, const Geometry& g,
                                    hipStream_t st) {
  if (dtype != MRP_DTYPE_BF16 && dtype != MRP_DTYPE_F16) return hipErrorInvalidValue;
  switch (nt) {
    MRP_HALF_NT_CASE(13)
    MRP_HALF_NT_CASE(14)
    MRP_HALF_NT_CASE(15)
    MRP_HALF_NT_CASE(16)
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mrp_host
