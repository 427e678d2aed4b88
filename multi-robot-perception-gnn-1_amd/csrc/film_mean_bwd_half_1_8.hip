// film_mean_bwd_half_1_8.hip — backward launches for 16-bit features, graphs of 1..8 nodes
// (see film_mean_bwd.hip and launch_bwd_half_ntb).
#include "film_mean_bwd_launch.hpp"

namespace mrp_host {

hipError_t dispatch_bwd_half_1_8(int dtype, int nt, bool complete, const AggArgs& a, const Geometry& g,
                                    hipStream_t st) {
  if (dtype != MRP_DTYPE_BF16 && dtype != MRP_DTYPE_F16) return hipErrorInvalidValue;
  switch (nt) {
    MRP_HALF_NT_CASE(1)
    MRP_HALF_NT_CASE(2)
    MRP_HALF_NT_CASE(3)
    MRP_HALF_NT_CASE(4)
    MRP_HALF_NT_CASE(5)
    MRP_HALF_NT_CASE(6)
    MRP_HALF_NT_CASE(7)
    MRP_HALF_NT_CASE(8)
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mrp_host
