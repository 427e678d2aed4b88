// film_wattn_bwd_f16.hip — the f16 launches of the confidence-gated attention fusion's backward
// (film_wattn_bwd.hip plans; one translation unit per 16-bit type keeps the build parallel).
#include "film_attn_kernels.hpp"

namespace mrp_host {
hipError_t launch_wattn_bwd_f16(const WAttnArgs& m, int ck, int ks, size_t lds, int64_t grid, hipStream_t st) {
  return launch_attn_bwd<mrp::f16_t, true>(m, ck, ks, lds, grid, st);
}
}  // namespace mrp_host
