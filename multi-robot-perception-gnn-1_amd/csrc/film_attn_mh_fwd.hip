// film_attn_mh_fwd.hip — the multi-head forward launches of the attention-pooled FiLM aggregation (film_attn_fwd.hip plans):
// film_attn_fwd with MH = true, grid = (graphs x tiles, heads).  Kernels and design notes:
// film_attn_kernels.hpp.
#include "film_attn_kernels.hpp"

namespace mrp_host {

namespace {
template <typename T>
hipError_t launch_mh_fwd(const mrp::AttnMhArgs<false>& m, int ks, size_t lds, int64_t grid, int heads, hipStream_t st) {
  const dim3 g((unsigned)grid, (unsigned)heads), block(mrp::kBlock);
  if (ks == 4)
    hipLaunchKernelGGL((mrp::film_attn_fwd<T, 4, false, true>), g, block, lds, st, m);
  else if (ks == 8)
    hipLaunchKernelGGL((mrp::film_attn_fwd<T, 8, false, true>), g, block, lds, st, m);
  else
    hipLaunchKernelGGL((mrp::film_attn_fwd<T, 16, false, true>), g, block, lds, st, m);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_attn_mh_fwd(int32_t dtype, const mrp::AttnMhArgs<false>& m, int ks, size_t lds, int64_t grid,
                              int heads, hipStream_t st) {
  switch (dtype) {
    case MRP_DTYPE_F32: return launch_mh_fwd<float>(m, ks, lds, grid, heads, st);
    case MRP_DTYPE_BF16: return launch_mh_fwd<mrp::bf16_t>(m, ks, lds, grid, heads, st);
    default: return launch_mh_fwd<mrp::f16_t>(m, ks, lds, grid, heads, st);
  }
}

}  // namespace mrp_host
