// compress_half_common.hpp — what the node-major (compress_half.hip) and pixel-major
// (compress_half_cl.hip) bf16 / fp16 compress kernels share beyond gemm_common.hpp (vector types, rsrc,
// xcd_remap, tile_of, the LDS image offsets boff / rowoff, the split-K host helpers): the MFMA per type,
// the workgroup's tile and stage sizes, the weight-operand side of the forward / data-gradient kernels,
// the weight-gradient kernels' partial-tile store and the host tail of the two weight gradients.
// (plan_splits also plans the pixel-major fp32 weight gradient of compress_split_cl.hip: same tile, same stage.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_common.hpp"
#include "mrp_gnn.h"
#include "tuning.hpp"

namespace mrp_ch {

using namespace mrp_gemm;

typedef float f8 __attribute__((ext_vector_type(8)));

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

// the wave's 64 x 64 accumulators (4 x 4 tiles of 16 x 16) start at zero
__device__ __forceinline__ void zero_acc(f4 (&acc)[4][4]) {
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f4{0.f, 0.f, 0.f, 0.f};
}

// a lane's MFMA operand (eight k) from the two ds_read_b64_tr_b16 results that hold its k 0..3 and 4..7
__device__ __forceinline__ u4 join_tr(s4 k03, s4 k47) {
  const u2 lo = __builtin_bit_cast(u2, k03), hi = __builtin_bit_cast(u2, k47);
  return u4{lo.x, lo.y, hi.x, hi.y};
}

// The weight operand of gemm_nn_half and gemm_cl_half (wave w of 8, tile row mt; MB = M / 32 row blocks
// and KS = K / 16 steps in mrp_compress_pack_t's image `ap`).
// A stage is 16 LDS-DMA pieces of 1 KiB, pc = 2 mbl + ksl (local 32-row block, 16-k step), at the front
// of the stage's LDS buffer; wave w issues pc = w and w + 8.
// Fragments: lane (r16, qq) of a 16 x 16 tile holds k = 8 qq .. 8 qq + 7.  16-row block mi of the wave is
// half (mi & 1) of 32-row block 2 wm + (mi >> 1); the image holds 16-k steps in `pack`'s lane order (lane
// r + 32 h: row r, k 8 h ..), so the lane reads step qq >> 1, slot 16 (mi & 1) + r16 + 32 (qq & 1).
struct WeightSide {
  __amdgpu_buffer_rsrc_t ra;
  u4* lds;
  int w;
  uint32_t va[2], abase0;

  __device__ __forceinline__ WeightSide(const u4* ap, u4* lds_, int mt, int MB, int KS, int lane, int w_)
      : ra(rsrc(ap)), lds(lds_), w(w_) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pc = w + 8 * i;
      const int mbl = pc >> 1, ksl = pc & 1;
      const int mb = min(mt * (TM / 32) + mbl, MB - 1);  // blocks past M: any valid data, never stored
      va[i] = (uint32_t)((((int64_t)mb * KS + ksl) * 64 + lane) * 16);
    }
    const int r16 = lane & 15, qq = lane >> 4, wm = w >> 1;
    abase0 = (uint32_t)reinterpret_cast<uintptr_t>(reinterpret_cast<char*>(lds) + (r16 + 32 * (qq & 1)) * 16 +
                                                   (4 * wm + (qq >> 1)) * 1024);
  }
  // stage s's pieces into LDS buffer buf
  __device__ __forceinline__ void issue(int s, int buf) const {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, lds + (buf * BUF_BYTES + (w + 8 * i) * 1024) / 16, 16, va[i],
                                               (uint32_t)s * 2 * 1024, 0, 0);
  }
  // the wave's four row-block fragments from the buffer at byte offset bo
  __device__ __forceinline__ void read(uint32_t bo, u4 (&ar)[4]) const {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
      asm volatile("ds_read_b128 %0, %1 offset:%2"
                   : "=v"(ar[mi])
                   : "v"(abase0 + bo), "i"((mi >> 1) * 2048 + 256 * (mi & 1)));
  }
};

// A weight-gradient wave's fp32 partial tile into the split's M x N `out`.  Register r of lane (r16, qq)
// of tile (mi, ni): row 16 mi + 4 qq + r, column 16 ni + r16 of the wave's 64 x 64 at (m0, n0).
__device__ __forceinline__ void store_partial(const f4 (&acc)[4][4], float* out, int M, int N, int m0, int n0, int r16,
                                              int qq) {
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int n = n0 + 16 * ni + r16;
    if (n >= N) continue;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + 16 * mi + 4 * qq + r;
        if (m < M) out[(int64_t)m * N + n] = acc[mi][ni][r];
      }
  }
}

inline bool is_half(int32_t dtype) { return dtype == MRP_DTYPE_BF16 || dtype == MRP_DTYPE_F16; }

// launch a kernel's BF16 or F16 instantiation (dtype: is_half)
template <typename... P, typename... A>
hipError_t launch_t(int32_t dtype, void (*kb)(P...), void (*kf)(P...), dim3 grid, dim3 block, hipStream_t st, A... a) {
  hipLaunchKernelGGL(dtype == MRP_DTYPE_BF16 ? kb : kf, grid, block, 0, st, a...);
  return hipGetLastError();
}

// splits of K = nodes P in whole 32-k stages (the last one ragged where the kernel takes any P):
// gemm_common.hpp's planner on the stage count, or the count a knob forces (`forced` > 0, clamped so that
// no split is empty)
inline int plan_splits(int64_t M, int64_t N, int64_t ktot, int forced, int64_t* kchunk) {
  const int64_t tiles = ((M + TM - 1) / TM) * ((N + TN - 1) / TN);
  const int64_t stages = (ktot + BK - 1) / BK;
  if (forced <= 0) return nt_splits(tiles, stages * BK, M, N, kchunk);
  const int64_t per = (stages + forced - 1) / forced;
  *kchunk = per * BK;
  return (int)((stages + per - 1) / per);
}

// The tail of both weight-gradient entry points: plan the splits of K, place the partial results, launch
// the kernel and sum.  `a` (NTArgs or WArgs) arrives with its operands, n0, P and ktot set.
template <typename A>
hipError_t run_wgrad(int32_t dtype, void (*kb)(A), void (*kf)(A), A a, int forced, int64_t M, int64_t N, float* gw,
                     float* gbias, void* workspace, int64_t workspace_bytes, hipStream_t st) {
  a.M = (int32_t)M;
  a.N = (int32_t)N;
  a.mtiles = (int32_t)((M + TM - 1) / TM);
  a.ntiles = (int32_t)((N + TN - 1) / TN);
  const int ns = plan_splits(M, N, a.ktot, forced, &a.kchunk);
  const SplitK pl = splitk_place(ns, M, N, gw, gbias, workspace, workspace_bytes);
  if (pl.err != hipSuccess) return pl.err;
  a.out = pl.out;
  a.outb = pl.outb;
  const int64_t grid = (int64_t)a.mtiles * a.ntiles * ns;
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  a.group = mrp_host::tuning().nt_group;
  const hipError_t e = launch_t(dtype, kb, kf, dim3((unsigned)grid), dim3(THREADS), st, a);
  if (e != hipSuccess || ns <= 1) return e;
  return split_sum(pl.out, ns, M, N, gw, pl.outb, ns, gbias, st);
}

}  // namespace mrp_ch
