// film_mean_fwd_q_bf16.hip — the FP8-message forward's bf16-output instantiations (mrp_film_mean_fwd_q), a
// translation unit of their own so they compile beside the others (film_mean_fwd_q.hip).
#include "film_mean_fwd_q_launch.hpp"

namespace mrp_host {

hipError_t dispatch_fwd_q_bf16(int nt, bool complete, const AggArgs& a, const Geometry& g, hipStream_t st) {
  return dispatch_fwd_q<mrp::bf16_t>(nt, complete, a, g, st);
}

}  // namespace mrp_host
