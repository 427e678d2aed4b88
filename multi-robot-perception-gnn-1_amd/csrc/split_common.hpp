// split_common.hpp — the split-bf16 arithmetic that the node-major (compress_split.hip) and pixel-major
// (compress_split_cl.hip) fp32 compress kernels share beyond gemm_common.hpp: the exact bf16 split of fp32
// operands, the partial products of one MFMA step into two accumulators, and the counted LDS waits of the
// fragment schedules.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_common.hpp"

namespace mrp_cs {

using namespace mrp_gemm;

__device__ __forceinline__ uint32_t cvt2(f2 x) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(x, bf2)); }
__device__ __forceinline__ f2 widen2(uint32_t p) {
  f2 r;
  r.x = __uint_as_float(p << 16);
  r.y = __uint_as_float(p & 0xffff0000u);
  return r;
}

// exact three-way split of two fp32 values: one dword (two bf16) per part
__device__ __forceinline__ void split2(f2 x, uint32_t& a, uint32_t& b, uint32_t& c) {
  a = cvt2(x);
  const f2 r1 = x - widen2(a);
  b = cvt2(r1);
  const f2 r2 = r1 - widen2(b);
  c = cvt2(r2);
}

// the first NP parts of the same split (NP 3: split2's; the parts a reduced form drops are never computed)
template <int NP>
__device__ __forceinline__ void splitp(f2 x, uint32_t (&p)[NP]) {
  p[0] = cvt2(x);
  if constexpr (NP > 1) {
    const f2 r1 = x - widen2(p[0]);
    p[1] = cvt2(r1);
    if constexpr (NP > 2) {
      const f2 r2 = r1 - widen2(p[1]);
      p[2] = cvt2(r2);
    }
  }
}

// The six partial products of one 16-k step into two accumulators: the five small ones (at most 2^-8
// of the product) into `lo`, a0 b0 into `hi`, summed once in the epilogue.  The bf16 MFMA rounds its
// sum into the accumulator to nearest, but where the accumulator is large against the products the
// low-order bits it drops are biased (tools/exp_split_dgrad.py: pixel sums of the data gradient 6x
// the fp32 GEMM's error with one accumulator); with a0 b0 alone in `hi` the long accumulator sees a
// sixth of the additions and the others happen 2^8 lower, and the bias falls to the fp32 GEMM's level.
struct Acc2 {
  f16v hi, lo;
};
// With NP parts kept the products are those with i + j < NP: six, three (a0 b1 and a1 b0 into `lo`) or
// a0 b0 alone (`lo` stays zero).
template <int NP>
__device__ __forceinline__ void mma6(const bf8 (&a)[NP], const bf8 (&b)[NP], Acc2& acc) {
  if constexpr (NP > 2) {
    acc.lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc.lo, 0, 0, 0);
    acc.lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc.lo, 0, 0, 0);
    acc.lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc.lo, 0, 0, 0);
  }
  if constexpr (NP > 1) {
    acc.lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc.lo, 0, 0, 0);
    acc.lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc.lo, 0, 0, 0);
  }
  acc.hi = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc.hi, 0, 0, 0);
}

// 16x16x32 form of the six partial products (four accumulator registers per 16 x 16 tile)
typedef float f4acc __attribute__((ext_vector_type(4)));
struct Acc2s {
  f4acc hi, lo;
};
template <int NP>
__device__ __forceinline__ void mma6_16(const bf8 (&a)[NP], const bf8 (&b)[NP], Acc2s& acc) {
  if constexpr (NP > 2) {
    acc.lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], acc.lo, 0, 0, 0);
    acc.lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], acc.lo, 0, 0, 0);
    acc.lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], acc.lo, 0, 0, 0);
  }
  if constexpr (NP > 1) {
    acc.lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], acc.lo, 0, 0, 0);
    acc.lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], acc.lo, 0, 0, 0);
  }
  acc.hi = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], acc.hi, 0, 0, 0);
}

// s_waitcnt lgkmcnt(N) with a compile-time count (the counter holds at most 15)
template <int N>
__device__ __forceinline__ void wait_lgkm() {
  static_assert(N >= 0, "lgkmcnt");
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N < 15 ? N : 15) : "memory");
}
// keep NP fragment registers behind the wait above them
template <int NP>
__device__ __forceinline__ void pin(u4 (&r)[NP]) {
#pragma unroll
  for (int p = 0; p < NP; ++p) asm volatile("" : "+v"(r[p]));
}

}  // namespace mrp_cs
