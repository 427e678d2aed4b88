// compress_half_common.hpp — what the node-major (compress_half.hip) and pixel-major
// (compress_half_cl.hip) bf16 / fp16 compress kernels share: the MFMA per type, the workgroup's tile and
// stage sizes, the LDS image layouts and the tile order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrp_ch {

typedef short s4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f8 __attribute__((ext_vector_type(8)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

struct BF16 {
  typedef __bf16 elem;
  typedef __bf16 v8 __attribute__((ext_vector_type(8)));
  typedef __bf16 v4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ f4 mma(u4 a, u4 b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};
struct F16 {
  typedef _Float16 elem;
  typedef _Float16 v8 __attribute__((ext_vector_type(8)));
  typedef _Float16 v4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ f4 mma(u4 a, u4 b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};

constexpr int TM = 256, TN = 128, BK = 32, THREADS = 512;
constexpr int A_BYTES = TM * BK * 2;  // 16 KiB: the stage's A operand (16 1-KiB pieces, or 256 64-byte rows)
constexpr int B_BYTES = BK * TN * 2;  // 8 KiB
constexpr int BUF_BYTES = A_BYTES + B_BYTES;
constexpr int LDS_BYTES = 2 * BUF_BYTES;  // 48 KiB

// byte offset of 16-byte chunk ch (8 columns) of row `row` in a [BK][TN] 16-bit image (compress_split.hip)
__device__ __forceinline__ uint32_t boff(int row, int ch) {
  return (uint32_t)(256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))));
}
// [row][4 chunks of 16 bytes], the chunks rotated by the row (compress_split.hip)
__device__ __forceinline__ uint32_t rowoff(int row, int chunk) {
  return (uint32_t)(64 * row + 16 * (chunk ^ ((row >> 2) & 3)));
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
}

__device__ __forceinline__ void tile_of(int t, int mtiles, int ntiles, int group, int& mt, int& nt) {
  const int gmax = group > 0 && group < mtiles ? group : mtiles;
  const int run = gmax * ntiles;
  const int g = t / run, first = g * gmax;
  const int gm = mtiles - first < gmax ? mtiles - first : gmax;
  const int rem = t - g * run;
  mt = first + rem % gm;
  nt = rem / gm;
}

}  // namespace mrp_ch
