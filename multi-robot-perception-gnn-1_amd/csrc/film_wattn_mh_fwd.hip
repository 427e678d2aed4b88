// film_wattn_mh_fwd.hip — the multi-head forward launches of the confidence-gated attention fusion (film_wattn_fwd.hip plans):
// film_attn_fwd with MH = true and WGT = true, grid = (graphs x tiles, heads).  Kernels and design notes:
// film_attn_kernels.hpp.  Also film_attn_gw_reduce, the head sum of grad_w.
#include "film_attn_kernels.hpp"

namespace mrp {

// grad_w of the multi-head gated backward: the heads' partials (H, nodes, P) summed heads ascending, head 0's value
// first.  One thread per (node, pixel).
__global__ void __launch_bounds__(kBlock) film_attn_gw_reduce(const float* part, int heads, int nodes, int P,
                                                              float* gw, int64_t gwst) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t np = (int64_t)nodes * P;
  if (idx >= np) return;
  const int u = (int)(idx / P), p = (int)(idx - (int64_t)u * P);
  float r = part[idx];
  for (int k = 1; k < heads; ++k) r = __fadd_rn(r, part[(int64_t)k * np + idx]);
  gw[(int64_t)u * gwst + p] = r;
}

}  // namespace mrp

namespace mrp_host {

namespace {
template <typename T>
hipError_t launch_mh_fwd(const mrp::AttnMhArgs<true>& m, int ks, size_t lds, int64_t grid, int heads, hipStream_t st) {
  const dim3 g((unsigned)grid, (unsigned)heads), block(mrp::kBlock);
  if (ks == 4)
    hipLaunchKernelGGL((mrp::film_attn_fwd<T, 4, true, true>), g, block, lds, st, m);
  else if (ks == 8)
    hipLaunchKernelGGL((mrp::film_attn_fwd<T, 8, true, true>), g, block, lds, st, m);
  else
    hipLaunchKernelGGL((mrp::film_attn_fwd<T, 16, true, true>), g, block, lds, st, m);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_wattn_mh_fwd(int32_t dtype, const mrp::AttnMhArgs<true>& m, int ks, size_t lds, int64_t grid,
                              int heads, hipStream_t st) {
  switch (dtype) {
    case MRP_DTYPE_F32: return launch_mh_fwd<float>(m, ks, lds, grid, heads, st);
    case MRP_DTYPE_BF16: return launch_mh_fwd<mrp::bf16_t>(m, ks, lds, grid, heads, st);
    default: return launch_mh_fwd<mrp::f16_t>(m, ks, lds, grid, heads, st);
  }
}

hipError_t launch_attn_gw_reduce(const float* part, int heads, int32_t nodes, int32_t P, float* gw, int64_t gwst,
                                 hipStream_t st) {
  const int64_t blocks = ((int64_t)nodes * P + mrp::kBlock - 1) / mrp::kBlock;
  if (blocks <= 0) return hipSuccess;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mrp::film_attn_gw_reduce, dim3((unsigned)blocks), dim3(mrp::kBlock), 0, st, part, heads, nodes, P,
                     gw, gwst);
  return hipGetLastError();
}

}  // namespace mrp_host
