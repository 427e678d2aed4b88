// film_wattn_mh_bwd_bf16.hip — the bf16 launches of the multi-head backward of the confidence-gated attention fusion
// (film_wattn_bwd.hip plans; one translation unit per type keeps the build parallel).
#include "film_attn_kernels.hpp"

namespace mrp_host {
hipError_t launch_wattn_mh_bwd_bf16(const mrp::AttnMhArgs<true>& m, int ck, int ks, size_t lds, int64_t grid, int heads,
                                    hipStream_t st) {
  return launch_attn_bwd<mrp::bf16_t, true, true>(m, ck, ks, lds, grid, st, heads);
}
}  // namespace mrp_host
