// film_wattn_fwd_q.hip — the gated launches of the FP8-message attention forward (film_attn_fwd_q.hip plans):
// film_attn_fwd (TX = q8_t) with WGT = true, single- and multi-head.  Kernels and design notes: film_attn_kernels.hpp.
#include "film_attn_kernels.hpp"

namespace mrp_host {

hipError_t launch_attn_fwd_q(int32_t dtype, const mrp::AttnQArgs<true, false>& m, int ks, size_t lds, int64_t grid,
                             int heads, hipStream_t st) {
  return launch_attn_fwd_q_dtype<true, false>(dtype, m, ks, lds, grid, heads, st);
}
hipError_t launch_attn_fwd_q(int32_t dtype, const mrp::AttnQArgs<true, true>& m, int ks, size_t lds, int64_t grid,
                             int heads, hipStream_t st) {
  return launch_attn_fwd_q_dtype<true, true>(dtype, m, ks, lds, grid, heads, st);
}

}  // namespace mrp_host
