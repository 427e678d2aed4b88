// film_max_bwd_bf16.hip — the max-pooled FiLM backward's launches for bf16 features (a translation unit of
// its own: it compiles beside film_max_bwd.hip and film_max_bwd_f16.hip).  Kernels: film_max_kernels.hpp.
#include "film_max_kernels.hpp"

namespace mrp_host {
hipError_t launch_max_bwd_bf16(const MaxArgs& m, const MaxBwdPlan& p, hipStream_t st) {
  return launch_max_bwd<mrp::bf16_t>(m, p, st);
}
}  // namespace mrp_host
