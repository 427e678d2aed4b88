// film_attn_mh_bwd_f16.hip — the fp16 launches of the multi-head backward of the attention-pooled FiLM aggregation
// (film_attn_bwd.hip plans; one translation unit per type keeps the build parallel).
#include "film_attn_kernels.hpp"

namespace mrp_host {
hipError_t launch_attn_mh_bwd_f16(const mrp::AttnMhArgs<false>& m, int ck, int ks, size_t lds, int64_t grid, int heads,
                                  hipStream_t st) {
  return launch_attn_bwd<mrp::f16_t, false, true>(m, ck, ks, lds, grid, st, heads);
}
}  // namespace mrp_host
