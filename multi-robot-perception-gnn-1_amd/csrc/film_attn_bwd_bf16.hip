// film_attn_bwd_bf16.hip — the bf16 launches of the attention-pooled FiLM aggregation's backward
// (film_attn_bwd.hip plans; one translation unit per 16-bit type keeps the build parallel).
#include "film_attn_kernels.hpp"

namespace mrp_host {
hipError_t launch_attn_bwd_bf16(const AttnArgs& m, int ck, int ks, size_t lds, int64_t grid, hipStream_t st) {
  return launch_attn_bwd<mrp::bf16_t>(m, ck, ks, lds, grid, st);
}
}  // namespace mrp_host
