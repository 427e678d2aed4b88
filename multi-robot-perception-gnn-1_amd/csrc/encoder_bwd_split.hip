// encoder_bwd_split.hip — the edge encoder's backward (training path, encoder.py) on the bf16 matrix
// cores at fp32 accuracy, gfx950 (MI355X / CDNA4).  Its two GEMMs are NT products of k-contiguous rows,
// i.e. split_nt.hpp's product over one "node" of K pixels, all three bf16 parts kept:
//   dh^T (C x E)  = W2^T (C x 2C) . dz^T     (k = j: rows of W2^T and of dz)
//   dW2 (2C x C)  = dz^T (2C x E) . h         (k = e: rows of dz^T and of h^T; db2 = its row sums of dz^T)
// mrp_edge_encoder_bwd_split runs them one after the other on the compress weight gradient's kernel
// (nt_run, compress_split.hip); mrp_edge_encoder_bwd_fused runs the whole backward in three launches.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <map>
#include <mutex>
#include <vector>

#include "gemm_common.hpp"
#include "mrp_gnn.h"
#include "split_common.hpp"
#include "split_nt.hpp"
#include "tuning.hpp"

namespace mrp_cs {

// two independent NT products in one launch, on the default (16x16x32) form: workgroups [0, grid1) run
// a1, the rest a2, each product with its own XCD-aware tile order
__global__ void __launch_bounds__(512, 1) gemm_nt_dual_mf16(NTArgs a1, NTArgs a2, int grid1) {
  if ((int)blockIdx.x < grid1)
    gemm_nt_split_body<4>(a1, blockIdx.x, grid1);
  else
    gemm_nt_split_body<4>(a2, blockIdx.x - grid1, gridDim.x - grid1);
}

// the same with the first product's A operand pre-split (gemm_nt_psa_body: W2^T, packed once per weight
// version) — the split body re-split it once per column tile and call
__global__ void __launch_bounds__(512, 1) gemm_nt_dual_psa1(NTArgs a1, NTArgs a2, int grid1) {
  if ((int)blockIdx.x < grid1)
    gemm_nt_psa_body<3>(a1, blockIdx.x, grid1);
  else
    gemm_nt_split_body<4>(a2, blockIdx.x - grid1, gridDim.x - grid1);
}

constexpr int kNin = 9;

// dz (E x N2, row-major) -> the packed split image of dz^T (N2 x E, k = the edges; `pack`'s layout, the
// dW2 product's A operand, read by LDS-DMA) and db2's partials csum[eb][j] = sum of dz[e][j] over the
// 64-edge block eb in edge order (summed over the blocks in order by encoder_bwd_reduce).  64 x 64 tile
// through LDS as dz_transpose; lane -> (row j0 + (u & 63), edges 8 (u >> 6) ..): a wave's 32-row halves
// store 512 contiguous bytes per part.  E % 16 == 0.
__global__ void __launch_bounds__(256) dzT_pack(const float* __restrict__ dz, int E, int N2, u4* __restrict__ img,
                                                float* __restrict__ csum) {
  __shared__ float tile[64][65];
  const int j0 = blockIdx.x * 64, e0 = blockIdx.y * 64;
  const int c4 = threadIdx.x & 15, r0 = threadIdx.x >> 4;
  f4 v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = e0 + r0 + 16 * i, j = j0 + 4 * c4;
    v[i] = (e < E && j < N2) ? *reinterpret_cast<const f4*>(dz + (int64_t)e * N2 + j) : f4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) tile[r0 + 16 * i][4 * c4 + q] = v[i][q];
  __syncthreads();
  if (threadIdx.x < 64 && j0 + (int)threadIdx.x < N2) {
    float sum = 0.f;
    for (int e = 0; e < 64; ++e) sum += tile[e][threadIdx.x];
    csum[(int64_t)blockIdx.y * N2 + j0 + threadIdx.x] = sum;
  }
  const int64_t KS = E / 16;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int u = threadIdx.x + 256 * i;
    const int jl = u & 63, g8 = u >> 6;
    const int j = j0 + jl, e = e0 + 8 * g8;
    if (j >= N2 || e >= E) continue;
    u4 p0, p1, p2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f2 x;
      x.x = tile[8 * g8 + 2 * q][jl];
      x.y = tile[8 * g8 + 2 * q + 1][jl];
      uint32_t a0, a1, a2;
      split2(x, a0, a1, a2);
      p0[q] = a0, p1[q] = a1, p2[q] = a2;
    }
    const int64_t base = (((int64_t)(j >> 5) * KS + (e >> 4)) * 3) * 64 + (j & 31) + 32 * ((e >> 3) & 1);
    img[base] = p0;
    img[base + 64] = p1;
    img[base + 128] = p2;
  }
}

// both products with a pre-split A: W2^T's packed image and dz^T's (dzT_pack)
__global__ void __launch_bounds__(512, 1) gemm_nt_dual_psa2(NTArgs a1, NTArgs a2, int grid1) {
  if ((int)blockIdx.x < grid1)
    gemm_nt_psa_body<3>(a1, blockIdx.x, grid1);
  else
    gemm_nt_psa_body<3>(a2, blockIdx.x - grid1, gridDim.x - grid1);
}

struct EncPlan {
  int s1, s2;
  int64_t kc1, kc2;
  int t1, t2;  // tiles of each product
  int64_t off_dzT, off_p1, off_p2, off_p2b, bytes;
};

EncPlan enc_plan(int64_t E, int64_t C) {
  EncPlan pl{};
  const int64_t C2 = 2 * C;
  pl.t1 = (int)(((C + NTGeo<4>::TM - 1) / NTGeo<4>::TM) * ((E + TN - 1) / TN));       // dh^T: M = C, N = E
  pl.t2 = (int)(((C2 + NTGeo<4>::TM - 1) / NTGeo<4>::TM) * ((C + TN - 1) / TN));      // dW2: M = 2C, N = C
  const int64_t st1 = C2 / BK, st2 = E / BK;                                // 32-k split granules
  // Split counts: the makespan of the launch's workgroups dispatched in order (the a t1 units of the
  // first product, p1 stages each, then the b t2 of the second) onto 256 CUs one at a time (~2.8 us per
  // 32-k stage), plus the partial tiles written and read back at ~4 TB/s.  Round 4's estimate (rounds x
  // the longer split) missed that the second product's units start as soon as the first's free their CU:
  // round 5 (tools/ab_enc_splits.py) configs[2] (3, 3) 136.9 vs its (2, 1) 141.7 us, configs[1] (8, 7)
  // 30.0 vs (5, 4) 33.8, configs[3] (4, 1) 101.4 vs (8, 1) 106.2; the headline and configs[4] unchanged.
  // Memoised per shape (at most kMemo shapes; a full memo starts over).  A pair whose lower bound — its
  // first product's rounds, or all its work spread evenly over the CUs, plus its traffic — is no better
  // than the best found is not simulated: the full search is up to 32 x 32 pairs of b t2 heap steps
  // each (~5e5 at C = 2048), the pruned one a few percent of that.
  constexpr size_t kMemo = 64;
  static std::mutex mu;
  static std::map<std::pair<int64_t, int64_t>, std::pair<int, int>> memo;
  {
    std::lock_guard<std::mutex> lock(mu);
    auto it = memo.find({E, C});
    if (it != memo.end()) {
      pl.s1 = it->second.first;
      pl.s2 = it->second.second;
    } else {
      double best = 1e300;
      pl.s1 = pl.s2 = 1;
      std::vector<int64_t> slot(256);
      for (int a = 1; a <= 32; ++a)
        for (int b = 1; b <= 32; ++b) {
          const int64_t p1 = (st1 + a - 1) / a, p2 = (st2 + b - 1) / b;
          if ((st1 + p1 - 1) / p1 != a || (st2 + p2 - 1) / p2 != b) continue;  // no empty split
          const int64_t n1 = (int64_t)a * pl.t1, n2 = (int64_t)b * pl.t2;
          const int64_t q = n1 / 256, r = n1 % 256;
          const double traffic = ((double)a * C * E + (double)b * C2 * C) * 8.0 / 4.0e6;
          const int64_t lb = std::max<int64_t>((q + (r ? 1 : 0)) * p1, (n1 * p1 + n2 * p2 + 255) / 256);
          if ((double)lb * 2.8 + traffic >= best) continue;  // cannot beat the best: skip the simulation
          for (int i = 0; i < 256; ++i) slot[i] = (q + (i < r ? 1 : 0)) * p1;  // the first product round robin
          std::make_heap(slot.begin(), slot.end(), std::greater<int64_t>());
          int64_t span = (q + (r ? 1 : 0)) * p1;
          for (int64_t i = 0; i < n2; ++i) {  // the second product onto the earliest free CU
            std::pop_heap(slot.begin(), slot.end(), std::greater<int64_t>());
            slot.back() += p2;
            span = slot.back() > span ? slot.back() : span;
            std::push_heap(slot.begin(), slot.end(), std::greater<int64_t>());
          }
          const double cost = (double)span * 2.8 + traffic;
          if (cost < best) {
            best = cost;
            pl.s1 = a;
            pl.s2 = b;
          }
        }
      if (memo.size() >= kMemo) memo.clear();
      memo[{E, C}] = {pl.s1, pl.s2};
    }
  }
  // lab knobs enc_s1 / enc_s2 (0: the planner's): force a split count (the chunks cover K, none empty)
  if (mrp_host::tuning().enc_s1 > 0) pl.s1 = (int)(mrp_host::tuning().enc_s1 < st1 ? mrp_host::tuning().enc_s1 : st1);
  if (mrp_host::tuning().enc_s2 > 0) pl.s2 = (int)(mrp_host::tuning().enc_s2 < st2 ? mrp_host::tuning().enc_s2 : st2);
  pl.kc1 = ((st1 + pl.s1 - 1) / pl.s1) * BK;
  pl.kc2 = ((st2 + pl.s2 - 1) / pl.s2) * BK;
  pl.s1 = (int)((st1 * BK + pl.kc1 - 1) / pl.kc1);  // the splits the chunks give (no empty one)
  pl.s2 = (int)((st2 * BK + pl.kc2 - 1) / pl.kc2);
  auto al = [](int64_t v) { return (v + 63) / 64 * 64; };  // 256-byte segments
  int64_t o = 0;
  pl.off_dzT = o;
  o += al(C2 * E * 3 / 2);  // dz^T in fp32, or its packed split image (6 bytes per element)
  pl.off_p1 = o;
  o += al((int64_t)pl.s1 * C * E);
  pl.off_p2 = o;
  o += al((int64_t)pl.s2 * C2 * C);
  pl.off_p2b = o;
  const int64_t nb2 = (int64_t)pl.s2 > (E + 63) / 64 ? pl.s2 : (E + 63) / 64;  // db2 partials: splits or edge blocks
  o += al(nb2 * C2);
  pl.bytes = o * 4;
  return pl;
}

// blocks [0, nb1): one hidden unit each -> dW1 / db1; blocks [nb1, ...): 1024
// outputs of dW2 each (and, in the first 2C / 256 of them, 256 of db2)
__global__ void __launch_bounds__(256) encoder_bwd_reduce(const float* __restrict__ p1, int s1,
                                                          const float* __restrict__ hT, const float* __restrict__ pose,
                                                          int E, int C, float* __restrict__ dw1,
                                                          float* __restrict__ db1, int nb1,
                                                          const f4* __restrict__ p2, const float* __restrict__ p2b,
                                                          int s2, int s2b, f4* __restrict__ dw2, float* __restrict__ db2) {
  if ((int)blockIdx.x < nb1) {
    // one workgroup per hidden unit u: wave w's lanes walk edges 64 w + lane + 256 k, summing the dh^T
    // partials in split order, masking by the ReLU and accumulating d pose^T and d in registers; a
    // fixed lane butterfly per wave, the four waves' sums added in wave order, and dW1[u] / db1[u]
    // written directly (no per-edge-block partials, no final launch)
    __shared__ float wsum[4][kNin + 1];
    const int u = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t plane = (int64_t)C * E;
    const float* p1u = p1 + (int64_t)u * E;
    const float* hTu = hT + (int64_t)u * E;
    float acc[kNin + 1];
#pragma unroll
    for (int i = 0; i <= kNin; ++i) acc[i] = 0.f;
#pragma unroll 2
    for (int e = threadIdx.x; e < E; e += 256) {
      float dh;
      if (s1 <= 8) {  // every partial's load issued before the sums (clamped index, no branch per load)
        float pv[8];
#pragma unroll
        for (int sp = 0; sp < 8; ++sp) pv[sp] = p1u[(int64_t)(sp < s1 ? sp : s1 - 1) * plane + e];
        dh = pv[0];
#pragma unroll
        for (int sp = 1; sp < 8; ++sp) dh = sp < s1 ? dh + pv[sp] : dh;
      } else {
        dh = p1u[e];
        for (int sp = 1; sp < s1; ++sp) dh += p1u[(int64_t)sp * plane + e];
      }
      const float d = hTu[e] > 0.f ? dh : 0.f;
      const float* pr = pose + (int64_t)e * kNin;
#pragma unroll
      for (int i = 0; i < kNin; ++i) acc[i] = fmaf(d, pr[i], acc[i]);
      acc[kNin] += d;
    }
#pragma unroll
    for (int i = 0; i <= kNin; ++i)
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) acc[i] += __shfl_xor(acc[i], o, 64);
    if (lane <= kNin) {
      float v = acc[0];
#pragma unroll
      for (int i = 1; i <= kNin; ++i) v = lane == i ? acc[i] : v;
      wsum[w][lane] = v;
    }
    __syncthreads();
    if (threadIdx.x <= kNin) {
      const float v = ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + wsum[2][threadIdx.x]) + wsum[3][threadIdx.x];
      if (threadIdx.x < kNin)
        dw1[(int64_t)u * kNin + threadIdx.x] = v;
      else
        db1[u] = v;
    }
    return;
  }
  const int b = blockIdx.x - nb1;
  const int64_t n4 = (int64_t)2 * C * C / 4;
  const int64_t e4 = (int64_t)b * 256 + threadIdx.x;
  if (e4 < n4) {
    f4 v;
    if (s2 <= 8) {
      f4 pv[8];
#pragma unroll
      for (int sp = 0; sp < 8; ++sp) pv[sp] = p2[(int64_t)(sp < s2 ? sp : s2 - 1) * n4 + e4];
      v = pv[0];
#pragma unroll
      for (int sp = 1; sp < 8; ++sp) v = sp < s2 ? v + pv[sp] : v;
    } else {
      v = p2[e4];
      for (int sp = 1; sp < s2; ++sp) v += p2[(int64_t)sp * n4 + e4];
    }
    dw2[e4] = v;
  }
  const int64_t m = (int64_t)b * 256 + threadIdx.x;
  if (m < 2 * C) {
    float v = p2b[m];
    for (int sp = 1; sp < s2b; ++sp) v += p2b[(int64_t)sp * 2 * C + m];
    db2[m] = v;
  }
}

// The operands of the two products as NTArgs: one "node" whose P "pixels" are the product's whole K, both
// row ranges of B the same matrix.  The caller adds the outputs and the split (or leaves them to nt_run).
struct EncProducts {
  NTArgs dh, dw2;
};
EncProducts enc_products(const float* dz, const float* dzT, const float* w2T, const float* hT, int64_t E, int32_t C) {
  const int64_t C2 = 2 * (int64_t)C;
  EncProducts p = {};
  p.dh.g = w2T;  // dh^T (C x E) = W2^T (C x 2C) . dz^T: rows u, k = j
  p.dh.gs = C * C2;
  p.dh.s0 = p.dh.s1 = dz;  // rows e, k = j
  p.dh.s0s = p.dh.s1s = E * C2;
  p.dh.n0 = (int32_t)E;
  p.dh.P = (int32_t)C2;
  p.dw2.g = dzT;  // dW2 (2C x C) = dz^T (2C x E) . h: rows j, k = e; row sums = db2
  p.dw2.gs = C2 * E;
  p.dw2.s0 = p.dw2.s1 = hT;  // rows u, k = e
  p.dw2.s0s = p.dw2.s1s = (int64_t)C * E;
  p.dw2.n0 = C;
  p.dw2.P = (int32_t)E;
  return p;
}

}  // namespace mrp_cs

using namespace mrp_cs;

// The two GEMMs one after the other on the compress weight gradient's kernel (nt_run)
extern "C" int64_t mrp_edge_encoder_bwd_split_workspace(int32_t num_edges, int32_t C) {
  if (num_edges <= 0 || C <= 0 || num_edges % BK != 0 || C % 32 != 0) return 0;
  const int64_t a = nt_workspace(C, num_edges, 2 * (int64_t)C), b = nt_workspace(2 * (int64_t)C, C, num_edges);
  return a > b ? a : b;
}

extern "C" int mrp_edge_encoder_bwd_split(const float* dz, const float* dzT, const float* w2T, const float* hT,
                                          int32_t num_edges, int32_t C, float* dhT, float* dw2, float* db2,
                                          void* workspace, int64_t workspace_bytes, void* stream) {
  if (num_edges < 0 || C < 0) return hipErrorInvalidValue;
  if (db2 != nullptr && dw2 == nullptr) return hipErrorInvalidValue;  // db2 rides on the dW2 product
  if (num_edges == 0 || C == 0 || (dhT == nullptr && dw2 == nullptr)) return hipSuccess;
  if (num_edges % BK != 0 || C % 32 != 0) return hipErrorNotSupported;
  if ((dhT && (!dz || !w2T || !aligned16(dz) || !aligned16(w2T) || !aligned16(dhT))) ||
      (dw2 && (!dzT || !hT || !aligned16(dzT) || !aligned16(hT) || !aligned16(dw2))))
    return hipErrorInvalidValue;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t E = num_edges, C2 = 2 * (int64_t)C;
  const EncProducts p = enc_products(dz, dzT, w2T, hT, E, C);
  if (dhT) {
    const hipError_t e = nt_run(p.dh, C, E, 1, dhT, nullptr, workspace, workspace_bytes, st);
    if (e != hipSuccess) return e;
  }
  if (dw2) return nt_run(p.dw2, C2, C, 1, dw2, db2, workspace, workspace_bytes, st);  // row sums of dz^T = db2
  return hipSuccess;
}

// ------------------------------------------------------------------------------------------------
// The edge encoder's whole backward in three launches on one stream (training path, encoder.py):
//   1. dz^T                                     (mrp_edge_encoder_bwd_prep)
//   2. dh^T = W2^T dz^T and dW2 = dz^T h        one launch of both split-K NT products, splits chosen
//                                               jointly so the two fill one round of the chip
//   3. encoder_bwd_reduce: dW2 and db2 = the fixed-order sums of their partial tiles / row sums; and,
//      per hidden unit (one workgroup over all edges), dh^T summed from its partial tiles, masked by
//      [h^T > 0] (ReLU) and reduced against the pose rows into dW1 / db1 — dh^T never written.
//      (Round 4 first reduced per (4 units, 256 edges) into partials summed by a fourth launch: the
//      whole backward 46.2 -> 42.8 us at E = 1792, C = 512, tools/exp_enc_bwd.py.)
// ------------------------------------------------------------------------------------------------
extern "C" int64_t mrp_edge_encoder_bwd_fused_workspace(int32_t num_edges, int32_t C) {
  if (num_edges <= 0 || C <= 0 || num_edges % BK != 0 || C % 32 != 0) return 0;
  return enc_plan(num_edges, C).bytes;
}

extern "C" int mrp_edge_encoder_bwd_fused(const float* dz, const float* w2T, const void* w2T_packed, const float* hT,
                                          const float* pose, int32_t num_edges, int32_t C, float* dw1, float* db1,
                                          float* dw2, float* db2, void* workspace, int64_t workspace_bytes,
                                          void* stream) {
  if (num_edges < 0 || C < 0) return hipErrorInvalidValue;
  if (C == 0) return hipSuccess;
  if (!dw1 || !db1 || !dw2 || !db2) return hipErrorInvalidValue;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t E = num_edges, C2 = 2 * (int64_t)C;
  if (E == 0) {  // empty sums
    if (hipMemsetAsync(dw1, 0, (size_t)C * kNin * 4, st) != hipSuccess ||
        hipMemsetAsync(db1, 0, (size_t)C * 4, st) != hipSuccess ||
        hipMemsetAsync(dw2, 0, (size_t)C2 * C * 4, st) != hipSuccess || hipMemsetAsync(db2, 0, (size_t)C2 * 4, st) != hipSuccess)
      return hipErrorUnknown;
    return hipSuccess;
  }
  if (E % BK != 0 || C % 32 != 0) return hipErrorNotSupported;
  if (!dz || !w2T || !hT || !pose || !aligned16(dz) || !aligned16(w2T) || !aligned16(hT) || !aligned16(dw2))
    return hipErrorInvalidValue;
  const EncPlan pl = enc_plan(E, C);
  if (workspace == nullptr || !aligned16(workspace) || workspace_bytes < pl.bytes) return hipErrorInvalidValue;
  float* ws = static_cast<float*>(workspace);
  float* dzT = ws + pl.off_dzT;
  // W2^T's packed image (mrp_compress_split_pack(w2, C, 1, C, 2C)): the dh^T product reads its A by
  // LDS-DMA instead of splitting W2^T in every workgroup; and (enc_bwd_psa 2, the default) dz^T is
  // written as a packed image too (dzT_pack, with db2's partials), so the dW2 product reads both its
  // operands' A side pre-split.  enc_bwd_psa 0: both split in the kernel, 1: only W2^T pre-split.
  const int mode = mrp_host::tuning().enc_bwd_psa;
  const bool psa1 = w2T_packed != nullptr && aligned16(w2T_packed) && mode >= 1 && (int64_t)C * C2 * 6 < kOffMax;
  const bool psa2 = psa1 && mode >= 2 && C2 * E * 6 < kOffMax;
  hipError_t e;
  if (psa2) {
    hipLaunchKernelGGL(dzT_pack, dim3((unsigned)((C2 + 63) / 64), (unsigned)((E + 63) / 64)), dim3(256), 0, st, dz,
                       num_edges, (int)C2, reinterpret_cast<u4*>(dzT), ws + pl.off_p2b);
    e = hipGetLastError();
  } else {
    e = (hipError_t)mrp_edge_encoder_bwd_prep(dz, num_edges, C, dzT, E, stream);
  }
  if (e != hipSuccess) return e;
  using GN = NTGeo<4>;
  EncProducts p = enc_products(dz, dzT, w2T, hT, E, C);
  NTArgs &a1 = p.dh, &a2 = p.dw2;
  a1.out = ws + pl.off_p1;
  a1.outb = nullptr;
  a1.ktot = C2;
  a1.kchunk = pl.kc1;
  a1.M = C;
  a1.N = (int32_t)E;
  a1.mtiles = (int32_t)((C + GN::TM - 1) / GN::TM);
  a1.ntiles = (int32_t)((E + TN - 1) / TN);
  a1.ap = psa1 ? static_cast<const u4*>(w2T_packed) : nullptr;
  a2.out = ws + pl.off_p2;
  a2.outb = psa2 ? nullptr : ws + pl.off_p2b;  // psa2: db2's partials came from dzT_pack
  a2.ap = psa2 ? reinterpret_cast<const u4*>(dzT) : nullptr;
  a2.ktot = E;
  a2.kchunk = pl.kc2;
  a2.M = (int32_t)C2;
  a2.N = C;
  a2.mtiles = (int32_t)((C2 + GN::TM - 1) / GN::TM);
  a2.ntiles = (int32_t)((C + TN - 1) / TN);
  a1.group = a2.group = mrp_host::tuning().nt_group;
  const int grid1 = pl.t1 * pl.s1, grid2 = pl.t2 * pl.s2;
  const dim3 grid((unsigned)(grid1 + grid2)), block(GN::THREADS);
  e = psa2   ? launch_lds<gemm_nt_dual_psa2>(GN::LDS_BYTES, grid, block, st, a1, a2, grid1)
      : psa1 ? launch_lds<gemm_nt_dual_psa1>(GN::LDS_BYTES, grid, block, st, a1, a2, grid1)
             : launch_lds<gemm_nt_dual_mf16>(GN::LDS_BYTES, grid, block, st, a1, a2, grid1);
  if (e != hipSuccess) return e;
  const int nb1 = C;
  const int64_t nb2 = (C2 * C / 4 + 255) / 256;  // >= 2C / 256 blocks: db2 rides along
  hipLaunchKernelGGL(encoder_bwd_reduce, dim3((unsigned)(nb1 + nb2)), dim3(256), 0, st, ws + pl.off_p1, pl.s1, hT, pose,
                     num_edges, C, dw1, db1, nb1, reinterpret_cast<const f4*>(ws + pl.off_p2), ws + pl.off_p2b,
                     pl.s2, psa2 ? (int)((E + 63) / 64) : pl.s2, reinterpret_cast<f4*>(dw2), db2);
  return hipGetLastError();
}
