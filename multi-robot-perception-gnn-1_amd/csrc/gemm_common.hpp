// gemm_common.hpp — what more than one of the GEMM translation units (compress_gemm.hip,
// compress_split.hip, encoder_bwd_split.hip, compress_split_cl.hip, compress_half.hip, compress_half_cl.hip,
// encoder_split.hip) uses: vector types, the buffer resource, the workgroup -> tile order, the 16-bit LDS
// image layouts, the launch of a kernel with dynamic LDS, the part-count dispatch, and the host side of the
// split-K weight gradients (planner, workspace placement, the sum of the partial tiles).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace mrp_gemm {

typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
typedef short s4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

// Buffer resource over `base` (raw, offsets in bytes, 2^31 - 1 bytes long)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
}

// Bijective block -> work-item remap: blocks orig, orig + 8, ... run on the same XCD (the dispatcher
// deals blocks round-robin over the 8 XCDs) and get consecutive ids, so tiles that share an operand
// share that XCD's L2 (cdna_hip_programming.md, XCD swizzle).
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
  const int q = nwg / 8, r = nwg % 8, xcd = orig % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / 8;
}

// Tile t of an mtiles x ntiles grid, in runs of `group` m-tiles walked m fastest (group <= 0: all of
// them, round 4's order).  An XCD runs ~32 consecutive tiles at once (the XCD-aware remap gives it a
// contiguous range), and they share its L2: with group 4 that window is 4 m-tiles x 8 column tiles,
// so the L2 misses per window are 4 row blocks of the packed operand plus 8 column blocks of the
// streamed one — at configs[3] (8 m-tiles x 32 column tiles) 42 MB per XCD against 59 MB for 8 x 4,
// and for its data gradient (16 m-tiles) 21 against 52 MB.
__device__ __forceinline__ void tile_of(int t, int mtiles, int ntiles, int group, int& mt, int& nt) {
  const int gmax = group > 0 && group < mtiles ? group : mtiles;
  const int run = gmax * ntiles;
  const int g = t / run, first = g * gmax;
  const int gm = mtiles - first < gmax ? mtiles - first : gmax;
  const int rem = t - g * run;
  mt = first + rem % gm;
  nt = rem / gm;
}

// byte offset of 16-byte chunk ch (8 columns) of row `row` in a [32 k][128 columns] 16-bit image
__device__ __forceinline__ uint32_t boff(int row, int ch) {
  return (uint32_t)(256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))));
}
// [row][32 k] 16-bit image: 64-byte rows of 4 chunks of 16 bytes, the chunks rotated by the row
__device__ __forceinline__ uint32_t rowoff(int row, int chunk) {
  return (uint32_t)(64 * row + 16 * (chunk ^ ((row >> 2) & 3)));
}

constexpr int64_t kOffMax = (int64_t)1 << 31;  // buffer offsets are 32-bit; keep every one below 2^31

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Launch kernel K with lds_bytes of dynamic LDS.  K is a template argument, so each kernel has its own
// instantiation and its dynamic-LDS attribute is set once per process, before its first launch.  Returns
// that call's error, else the launch's.
template <auto K, typename... A>
hipError_t launch_lds(int lds_bytes, dim3 grid, dim3 block, hipStream_t st, A... a) {
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL(K, grid, block, lds_bytes, st, a...);
  return hipGetLastError();
}

// f(std::integral_constant<int, parts>) for a part count the caller has validated (1..3): the run-time
// count of bf16 parts -> the compile-time NP of a kernel or launcher
template <class F>
auto dispatch_parts(int parts, F f) {
  if (parts == 3) return f(std::integral_constant<int, 3>{});
  if (parts == 2) return f(std::integral_constant<int, 2>{});
  return f(std::integral_constant<int, 1>{});
}

// compress_split.hip: the split-K planner of the 256 x 128-tile, 32-k-stage weight-gradient kernels
int nt_splits(int64_t tiles, int64_t ktot, int64_t M, int64_t N, int64_t* kchunk);

// compress_split.hip: out (M x N) = the sum over the nsplit partial tiles [split][M][N] of `part`, in a
// fixed order; outb (M, or null) = the same over the nsplitb row-sum partials [split][M] of partb
hipError_t split_sum(const float* part, int nsplit, int64_t M, int64_t N, float* out, const float* partb, int nsplitb,
                     float* outb, hipStream_t st);

// Where a weight gradient of ns splits of K puts its partial results.  One split writes gw / gbias
// themselves and needs no workspace; more write [split][M][N] tiles, then [split][M] row sums, into the
// workspace (`bytes` of it, 16-byte aligned) for split_sum.  err: hipErrorInvalidValue where that
// workspace is missing, short or misaligned.  outb is null where no gbias is wanted.  The workspace
// queries ask for `bytes` alone.
struct SplitK {
  int64_t bytes;
  hipError_t err;
  float* out;
  float* outb;
};
inline SplitK splitk_place(int ns, int64_t M, int64_t N, float* gw = nullptr, float* gbias = nullptr,
                           void* workspace = nullptr, int64_t workspace_bytes = 0) {
  SplitK p = {ns <= 1 ? 0 : ((int64_t)ns * M * N + (int64_t)ns * M) * 4, hipSuccess, gw, gbias};
  if (p.bytes == 0) return p;
  if (workspace == nullptr || workspace_bytes < p.bytes || !aligned16(workspace)) {
    p.err = hipErrorInvalidValue;
    return p;
  }
  float* ws = static_cast<float*>(workspace);
  p.out = ws;
  p.outb = gbias == nullptr ? nullptr : ws + (int64_t)ns * M * N;
  return p;
}

}  // namespace mrp_gemm
