// film_wmean_bwd_f16.hip — the confidence-weighted FiLM backward's launches for f16 features (a translation
// unit of its own: it compiles beside film_wmean_bwd.hip).  Kernels: film_wmean_kernels.hpp.
#include "film_wmean_kernels.hpp"

namespace mrp_host {
hipError_t launch_wmean_bwd_f16(const WArgs& m, const WBwdPlan& p, hipStream_t st) {
  return launch_wmean_bwd<mrp::f16_t>(m, p, st);
}
}  // namespace mrp_host
