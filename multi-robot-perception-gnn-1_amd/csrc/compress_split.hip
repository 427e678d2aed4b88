// compress_split.hip — the GCN layer's 1x1 compress convolution (forward, data gradient and weight
// gradient) on the bf16 matrix cores at fp32 accuracy, gfx950 (MI355X / CDNA4).
//
// Reference (xjh19971/multi-robot-perception-gnn-1, dgl/model/models.py:163-165,181-184,186-189):
//     h = self.conv1(torch.cat((h, g_h), dim=1))       # nn.Conv2d(2C, C, kernel_size=1), fp32
// and its gradients in training (dgl/training.py:208-210).  Per node n, with P = H W pixels:
//     forward      y[n] = W [x[n]; a[n]] + b          M = C,  K = 2C (rows from x, then a)
//     data grad    [dx[n]; da[n]] = W^T dy[n]         M = 2C, K = C  (rows to dx, then da)
//     weight grad  dW = sum_n dy[n] [x[n]; a[n]]^T, db = sum_n, pixels dy[n]     K = nodes P
// Three products live here: (1) the NN product of the forward and the data gradient (Geo, pack,
// gemm_nn_split_body); (2) the NT product of the weight gradient with both operands split in the kernel
// (gemm_nt_split_w4_mf16 on split_nt.hpp's gemm_nt_split_body, split-K summed by split_sum_nt); (3) the
// same with dy split once beforehand (split_rows, gemm_nt_psa on split_nt.hpp's PsaBody, row_sums).  The
// edge encoder's backward builds its kernels from the same NT bodies in encoder_bwd_split.hip.
//
// The NN product is the same as compress_gemm.hip's gemm_nn (which runs it on the fp32 MFMA), here on
// v_mfma_f32_32x32x16_bf16 with the exact three-way bf16 split of encoder_split.hip: every fp32 operand
// x = x0 + x1 + x2 (+ < 2^-24 |x|), each product the sum of the six partial products a_i b_j with
// i + j <= 2, exact in the MFMA and summed in fp32 — as accurate as an fp32 GEMM (the omitted terms are
// below 2^-25 of the product; 6 roundings per 16 k against the fp32 MFMA's 16), at 192 MFMA cycles per
// 16 k instead of 512.
//
// Operands.  A (the weight, M x K) is split and laid out once per weight version by
// mrp_compress_split_pack in per-lane fragment order (16-byte unit ((mb KS + ks) 3 + p) 64 + lane holds
// lane (r, h)'s eight k = 16 ks + 8 h + j of row 32 mb + r, part p) and arrives by LDS-DMA.  B (the
// activations) is node-major NCHW: k = channel rows of P contiguous pixels, i.e. k-strided for the
// MFMA, which wants eight consecutive k per lane.  Each thread loads 16-byte row pieces of the next
// stage into registers, splits them, and stores the three bf16 parts row-major into LDS ([k][column],
// 256-byte rows, 16-byte chunks XOR-swizzled by the row: cdna_hip_programming.md T10 layout (b)); the
// MFMA fragments come back with ds_read_b64_tr_b16, which delivers four k of one column per lane
// (conflict-free on that layout).
//
// Workgroup: a (64 WMW) x 128 output tile of WMW x 2 waves of 64 x 64; K in stages of 32, two LDS
// buffers (A 12 WMW KiB + B 3 x 8 KiB each): stage s + 1's A is DMA'd and its B loaded into registers
// while stage s is multiplied; one barrier per stage.  Product forms: WMW = 4 (8 waves, two per SIMD,
// each B stage split once for 256 rows) on v_mfma_f32_16x16x32_bf16 (4 x 4 tiles of 16 x 16 per wave)
// where M % 256 == 0 — every reference configuration — else WMW = 2 on 32x32x16 (2 x 2 blocks of
// 32 x 32).  The weight gradient (below) runs the same structure on two activation operands, and with
// its dy operand split once (gemm_nt_psa).  Round 4's other forms are lab forms (tools/lab_forms.hip).
//
// Part count.  Every kernel of the compress takes a compile-time NP = 3 / 2 / 1: the bf16 parts kept per
// operand, with the partial products i + j < NP (six, three, one).  The reduced forms skip the dropped
// parts' conversions, LDS stores, fragment reads, weight-image pieces and MFMAs (mrp_compress_*_split_p;
// DESIGN.md §3.11); the numbers above are NP = 3's.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_common.hpp"
#include "mrp_gnn.h"
#include "split_common.hpp"
#include "split_nt.hpp"
#include "tuning.hpp"

namespace mrp_cs {

// TN, BK, the NT product's NTArgs / NTGeo and bodies, `using namespace mrp_gemm`: split_nt.hpp
constexpr int B_PART_BYTES = BK * TN * 2;  // one bf16 part of the B stage: 8 KiB

// Workgroup geometry: WMW x 2 waves of 64 x 64, TM = 64 WMW rows; NP = the bf16 parts kept per operand
// (3: six partial products; 2: three; 1: one — DESIGN.md §3.11).  A reduced form stages only its NP
// parts of either operand: the stage shrinks with NP.
template <int WMW, int NP = 3>
struct Geo {
  static constexpr int TM = 64 * WMW, NW = 2 * WMW, THREADS = 64 * NW;
  static constexpr int A_PIECES = (TM / 32) * (BK / 16) * NP;  // 1 KiB pieces per stage (2 NP per wave)
  static constexpr int A_BYTES = A_PIECES * 1024;
  static constexpr int BUF_BYTES = A_BYTES + NP * B_PART_BYTES;
  static constexpr int LDS_BYTES = 2 * BUF_BYTES;  // NP 3: 96 KiB (WMW 2), 144 KiB (WMW 4); x NP / 3
  static constexpr int BJ = BK * TN / 4 / THREADS;  // 16-byte B pieces per thread per stage
  static constexpr int KR = THREADS / 32;           // B rows per pass
};

// A (M x K) = w (row-major, M x K, stride lda) or w^T (w: K x M row-major, stride lda) -> packed parts
__global__ void __launch_bounds__(256) pack(const float* __restrict__ w, int64_t lda, int trans, int M, int K,
                                            u4* __restrict__ out) {
  const int KS = K / 16;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)(M / 32) * KS * 64) return;
  const int lane = (int)(t & 63);
  const int64_t g = t >> 6;  // mb * KS + ks
  const int ks = (int)(g % KS), mb = (int)(g / KS);
  const int m = 32 * mb + (lane & 31), k0 = 16 * ks + 8 * (lane >> 5);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = trans ? w[(int64_t)(k0 + j) * lda + m] : w[(int64_t)m * lda + k0 + j];
  u4 p0, p1, p2;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f2 x;
    x.x = v[2 * i];
    x.y = v[2 * i + 1];
    uint32_t e0, e1, e2;
    split2(x, e0, e1, e2);
    p0[i] = e0, p1[i] = e1, p2[i] = e2;
  }
  out[(g * 3 + 0) * 64 + lane] = p0;
  out[(g * 3 + 1) * 64 + lane] = p1;
  out[(g * 3 + 2) * 64 + lane] = p2;
}

struct Args {
  const u4* ap;  // packed A
  const float* b0;
  int64_t b0s;
  const float* b1;
  int64_t b1s;
  float* c0;
  int64_t c0s;
  float* c1;
  int64_t c1s;
  const float* bias;  // (M) or null
  int64_t ncols;      // nodes * P
  int32_t M, K, k0, m0, P, mtiles;
  int32_t group;  // tile order (tile_of)
};

template <int WMW, bool MF16 = false, int NP = 3>
__device__ __forceinline__ void gemm_nn_split_body(const Args& a) {
  using G = Geo<WMW, NP>;
  constexpr int TM = G::TM, NW = G::NW, A_PIECES = G::A_PIECES, A_BYTES = G::A_BYTES, BUF_BYTES = G::BUF_BYTES;
  extern __shared__ u4 lds[];
  char* ldsb = reinterpret_cast<char*>(lds);
  // XCD-aware tile order: the m tiles of one column tile run on one XCD and share its L2 (B is read
  // once from HBM per column tile)
  const int nwg = gridDim.x;
  const int id = xcd_remap(blockIdx.x, nwg);
  int mt, nt;
  tile_of(id, a.mtiles, nwg / a.mtiles, a.group, mt, nt);
  const int64_t nbase = (int64_t)nt * TN;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int KS = a.K / 16, nst = a.K / BK, ks0 = a.k0 / BK, MB = a.M / 32;

  // ---- A: LDS-DMA pieces pc = (mbl 2 + ksl) NP + p (local m block, 16-k step, part), pc = w + NW i.
  // The packed image always holds three parts per (block, step) as separate 1 KiB pieces: a reduced
  // form fetches the first NP of them and packs them densely in LDS.
  const __amdgpu_buffer_rsrc_t ra = rsrc(a.ap);
  uint32_t va[A_PIECES / NW];
#pragma unroll
  for (int i = 0; i < A_PIECES / NW; ++i) {
    const int pc = w + NW * i;
    const int mbl = pc / (2 * NP), kp = 3 * ((pc / NP) & 1) + pc % NP;  // kp = 3 ksl + p
    const int mb = min(mt * (TM / 32) + mbl, MB - 1);  // blocks past M: any valid data, never stored
    va[i] = (uint32_t)((((int64_t)mb * KS * 3 + kp) * 64 + lane) * 16);
  }
  auto issue_a = [&](int s, int buf) {
#pragma unroll
    for (int i = 0; i < A_PIECES / NW; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, lds + (buf * BUF_BYTES + (w + NW * i) * 1024) / 16, 16, va[i],
                                               (uint32_t)s * 6 * 1024, 0, 0);
  };

  // ---- B: thread t loads the 16-byte pieces (row (t >> 5) + KR j, columns 4 (t & 31) ..) of a stage
  const int fc = threadIdx.x & 31, kr = threadIdx.x >> 5;
  int64_t col = nbase + 4 * fc;
  if (col > a.ncols - 4) col = a.ncols - 4;  // columns past the end: any valid data, never stored
  const int64_t node = col / a.P, pix = col - node * a.P;
  const float* bp0 = a.b0 + node * a.b0s + pix + (int64_t)kr * a.P;
  const float* bp1 = a.b1 + node * a.b1s + pix + (int64_t)kr * a.P;
  f4 breg[G::BJ];
  auto load_b = [&](int s) {
    const float* p = s < ks0 ? bp0 + (int64_t)s * BK * a.P : bp1 + (int64_t)(s - ks0) * BK * a.P;
#pragma unroll
    for (int j = 0; j < G::BJ; ++j) breg[j] = *reinterpret_cast<const f4*>(p + (int64_t)G::KR * j * a.P);
  };
  auto store_b = [&](int buf) {  // split the registers' stage into the buffer's NP part images
    char* bimg = ldsb + buf * BUF_BYTES + A_BYTES;
#pragma unroll
    for (int j = 0; j < G::BJ; ++j) {
      f2 lo, hi;
      lo.x = breg[j].x, lo.y = breg[j].y, hi.x = breg[j].z, hi.y = breg[j].w;
      uint32_t l[NP], h[NP];
      splitp<NP>(lo, l);
      splitp<NP>(hi, h);
      const uint32_t o = boff(kr + G::KR * j, fc >> 1) + 8 * (fc & 1);
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        u2 v;
        v.x = l[p], v.y = h[p];
        *reinterpret_cast<u2*>(bimg + p * B_PART_BYTES + o) = v;
      }
    }
  };

  // ---- fragment reads of one 16-k step: A by row pieces (ds_read_b128), B by ds_read_b64_tr_b16
  const int g16 = lane >> 4, i16 = lane & 15, hh = lane >> 5;
  // tr read: lane 4q + p of its 16-lane group reads row r0 + q, columns c0 + 4p .. (c0 = 16 (g16 & 1))
  const int trq = i16 >> 2, trp = i16 & 3;
  auto read_step = [&](int buf, int ksl, bf8 (&af)[2][NP], bf8 (&bf)[2][NP]) {
    const char* base = ldsb + buf * BUF_BYTES;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int pc = ((2 * wm + mi) * 2 + ksl) * NP + p;
        af[mi][p] = __builtin_bit_cast(bf8, *reinterpret_cast<const u4*>(base + pc * 1024 + lane * 16));
      }
    const char* bimg = base + A_BYTES;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        s4 v[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int row = 16 * ksl + 8 * hh + 4 * t + trq;
          const int ch = (64 * wn + 32 * ni + 16 * (g16 & 1)) / 8 + (trp >> 1);
          const char* addr = bimg + p * B_PART_BYTES + boff(row, ch) + 8 * (trp & 1);
          v[t] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s4*)(reinterpret_cast<uintptr_t>(addr)));
        }
        u4 u;
        u.x = __builtin_bit_cast(uint32_t, __builtin_shufflevector(v[0], v[0], 0, 1));
        u.y = __builtin_bit_cast(uint32_t, __builtin_shufflevector(v[0], v[0], 2, 3));
        u.z = __builtin_bit_cast(uint32_t, __builtin_shufflevector(v[1], v[1], 0, 1));
        u.w = __builtin_bit_cast(uint32_t, __builtin_shufflevector(v[1], v[1], 2, 3));
        bf[ni][p] = __builtin_bit_cast(bf8, u);
      }
  };

  if constexpr (MF16) {
    // 16x16x32 products over the whole 32-k stage: lane (r16, qq) of a 16 x 16 tile holds k = 8 qq ..
    // 8 qq + 7.  A: 16-row block mi of the wave is half (mi & 1) of 32-row block 2 wm + (mi >> 1); the
    // packed image holds 16-k steps in the 32 x 32 x 16 lane order (lane r + 32 hh: row r, k 8 hh ..),
    // so the lane reads step qq >> 1, slot 16 (mi & 1) + r16 + 32 (qq & 1).  B: the transposing reads of
    // rows 8 qq + 4 t .. + 3 (t = 0, 1), columns 64 wn + 16 ni ...
    const int r16 = lane & 15, qq = lane >> 4;
    uint32_t tr16[4][2];  // byte address of read (ni, t) in buffer 0, part 0
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int t = 0; t < 2; ++t)
        tr16[ni][t] = (uint32_t)reinterpret_cast<uintptr_t>(
            ldsb + A_BYTES + boff(8 * qq + 4 * t + trq, (64 * wn + 16 * ni) / 8 + (trp >> 1)) + 8 * (trp & 1));
    const int aslot = (r16 + 32 * (qq & 1)) * 16;
    const uint32_t abase0 =
        (uint32_t)reinterpret_cast<uintptr_t>(ldsb + aslot + ((4 * wm + (qq >> 1)) * NP) * 1024);
    Acc2s acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mi][ni].hi[r] = acc[mi][ni].lo[r] = 0.f;
    issue_a(0, 0);
    load_b(0);
#pragma unroll 1
    for (int s = 0; s < nst; ++s) {
      const int buf = s & 1;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      store_b(buf);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      {  // (scope of the stage's fragments)
        // every fragment read by inline asm (the transposing-read builtin carries no memory operand, so
        // hipcc would wait for the LDS-DMA issued below, which fills the other buffer) with counted
        // waits, in the order the MFMAs need them: A row 0, B columns 0..3, then A row mi + 1 under row
        // mi's MFMAs (lgkmcnt holds at most 15).  2-3 % over one wait for all of them.  A row is NP
        // reads and a B column 2 NP, so every count below scales with NP.
        const uint32_t ab = abase0 + (uint32_t)(buf * BUF_BYTES);
        u4 ar[2][NP];
        s4 v[4][NP][2];
        auto read_a16 = [&](int mi, u4 (&r)[NP]) {
#pragma unroll
          for (int p = 0; p < NP; ++p)
            asm volatile("ds_read_b128 %0, %1 offset:%2"
                         : "=v"(r[p])
                         : "v"(ab), "i"((mi >> 1) * 2048 * NP + p * 1024 + 256 * (mi & 1)));
        };
        read_a16(0, ar[0]);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
          for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int t = 0; t < 2; ++t)
              asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
                           : "=v"(v[ni][p][t])
                           : "v"(tr16[ni][t] + (uint32_t)(buf * BUF_BYTES)), "i"(p * B_PART_BYTES));
        if (s + 1 < nst) {
          issue_a(s + 1, buf ^ 1);
          load_b(s + 1);
        }
        bf8 bf[4][NP];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          u4 (&cur)[NP] = ar[mi & 1];
          if (mi < 3) read_a16(mi + 1, ar[(mi + 1) & 1]);
          if (mi > 0) {
            if (mi < 3)
              wait_lgkm<NP>();  // row mi + 1's reads stay in flight
            else
              wait_lgkm<0>();
            pin<NP>(cur);
          }
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) {
            if (mi == 0) {
              // A row 0 and B columns 0..ni landed: younger are 2 NP (3 - ni) B reads and A row 1's NP
              // (NP 3: 21 -> 15, 15, 9, 3)
              if (ni == 0)
                wait_lgkm<7 * NP>();
              else if (ni == 1)
                wait_lgkm<5 * NP>();
              else if (ni == 2)
                wait_lgkm<3 * NP>();
              else
                wait_lgkm<NP>();
              if (ni == 0) pin<NP>(cur);
#pragma unroll
              for (int p = 0; p < NP; ++p) {
                asm volatile("" : "+v"(v[ni][p][0]), "+v"(v[ni][p][1]));
                u4 u;
                u.x = __builtin_bit_cast(uint32_t, __builtin_shufflevector(v[ni][p][0], v[ni][p][0], 0, 1));
                u.y = __builtin_bit_cast(uint32_t, __builtin_shufflevector(v[ni][p][0], v[ni][p][0], 2, 3));
                u.z = __builtin_bit_cast(uint32_t, __builtin_shufflevector(v[ni][p][1], v[ni][p][1], 0, 1));
                u.w = __builtin_bit_cast(uint32_t, __builtin_shufflevector(v[ni][p][1], v[ni][p][1], 2, 3));
                bf[ni][p] = __builtin_bit_cast(bf8, u);
              }
            }
            bf8 af[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) af[p] = __builtin_bit_cast(bf8, cur[p]);
            mma6_16<NP>(af, bf[ni], acc[mi][ni]);
            if (mi == 0 || ni == 3) __builtin_amdgcn_sched_barrier(0);  // keep each wait before its MFMAs
          }
        }
      }
    }
    // Epilogue.  Accumulator register r of lane (r16, qq) of tile (mi, ni): row 16 mi + 4 qq + r, column
    // 16 ni + r16.  Each store is one buffer_store_dword: the lane's byte offset (node, pixel, 4 qq rows)
    // is fixed per ni and the row's part (16 mi + r rows) is a scalar offset; a 16-row block lies on one
    // side of m0 (the launch requires m0 % 64 == 0), so its output tensor is picked per block.  Round 4's
    // per-element 64-bit addressing (an int64 division per column, a bias load and the side select per
    // element: ~1,800 VALU instructions per wave) cost 3-11 % of the kernel (tools/ab_gemm.py).
    const int mb0 = mt * TM + 64 * wm;
    uint32_t vo0[4], vo1[4];  // per ni: byte offset of (node, pixel, row 4 qq) in c0 / c1
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int64_t n = nbase + 64 * wn + 16 * ni + r16;
      const bool live = n < a.ncols;
      const uint32_t nn = (uint32_t)(live ? n : 0);  // the launch requires ncols < 2^31
      const uint32_t nd = nn / (uint32_t)a.P, px = nn - nd * (uint32_t)a.P;
      // columns past the end: an offset past the buffer's 2^31 - 1 bytes, so the store is dropped
      // (the range check covers the lane offset, not the scalar one)
      vo0[ni] = live ? 4u * ((uint32_t)((int64_t)nd * a.c0s) + px + (uint32_t)(4 * qq * a.P)) : 0x80000000u;
      vo1[ni] = live ? 4u * ((uint32_t)((int64_t)nd * a.c1s) + px + (uint32_t)(4 * qq * a.P)) : 0x80000000u;
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int mrow = mb0 + 16 * mi;  // the block's first row (wave-uniform)
      const bool side1 = mrow >= a.m0;
      const uint32_t srow = (uint32_t)(side1 ? mrow - a.m0 : mrow);
      const __amdgpu_buffer_rsrc_t rc = rsrc(side1 ? a.c1 : a.c0);
      f4 bv = {0.f, 0.f, 0.f, 0.f};
      if (a.bias != nullptr) {
        const float* bp = a.bias + mrow + 4 * qq;
        bv = {bp[0], bp[1], bp[2], bp[3]};
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t so = 4u * (srow + (uint32_t)r) * (uint32_t)a.P;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          float v = __fadd_rn(acc[mi][ni].hi[r], acc[mi][ni].lo[r]);
          if (a.bias != nullptr) v = __fadd_rn(v, bv[r]);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rc, side1 ? vo1[ni] : vo0[ni], so, 0);
        }
      }
    }
    return;
  }

  Acc2 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni].hi[r] = acc[mi][ni].lo[r] = 0.f;

  issue_a(0, 0);
  load_b(0);
#pragma unroll 1
  for (int s = 0; s < nst; ++s) {
    const int buf = s & 1;
    // stage s's B registers and A pieces (own) landed; its buffer was last read in stage s - 2
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    store_b(buf);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // stage s visible to every wave; every wave is past stage s - 1's reads
    if (s + 1 < nst) {
      issue_a(s + 1, buf ^ 1);
      load_b(s + 1);
    }
#pragma unroll
    for (int ksl = 0; ksl < 2; ++ksl) {
      bf8 af[2][NP], bf[2][NP];
      read_step(buf, ksl, af, bf);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) mma6<NP>(af[mi], bf[ni], acc[mi][ni]);
    }
  }

  // ---- epilogue: accumulator register r of lane (column l & 31, half hh) is row (r & 3) + 8 (r >> 2) + 4 hh
  const int mbase = mt * TM + 64 * wm;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int64_t n = nbase + 64 * wn + 32 * ni + (lane & 31);
    if (n >= a.ncols) continue;
    const int64_t nd = n / a.P, px = n - nd * a.P;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mbase + 32 * mi + (r & 3) + 8 * (r >> 2) + 4 * hh;
        if (m >= a.M) continue;
        float v = __fadd_rn(acc[mi][ni].hi[r], acc[mi][ni].lo[r]);
        if (a.bias != nullptr) v = __fadd_rn(v, a.bias[m]);
        float* dst = m < a.m0 ? a.c0 + nd * a.c0s + (int64_t)m * a.P + px
                              : a.c1 + nd * a.c1s + (int64_t)(m - a.m0) * a.P + px;
        *dst = v;
      }
  }
}

template <int NP>
__global__ void __launch_bounds__(256, 1) gemm_nn_split_w2(Args a) {
  gemm_nn_split_body<2, false, NP>(a);
}
template <int NP>
__global__ void __launch_bounds__(512, 1) gemm_nn_split_w4_mf16(Args a) {
  gemm_nn_split_body<4, true, NP>(a);
}

template <int WMW, int NP, void (*K)(Args)>
hipError_t launch_w(Args a, hipStream_t st) {
  using G = Geo<WMW, NP>;
  a.mtiles = (a.M + G::TM - 1) / G::TM;
  const int64_t grid = (int64_t)a.mtiles * ((a.ncols + TN - 1) / TN);
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  a.group = mrp_host::tuning().gemm_group;
  return launch_lds<K>(G::LDS_BYTES, dim3((unsigned)grid), dim3(G::THREADS), st, a);
}

// the 16x16x32 form's epilogue: 16-row blocks on one side of m0, 32-bit buffer offsets into c0 / c1
bool mf16_ok(const Args& a) {
  if (a.M % 256 != 0 || a.m0 % 64 != 0 || a.ncols >= kOffMax) return false;
  const int64_t nodes = a.ncols / a.P;
  const int64_t r0 = a.m0 < a.M ? a.m0 : a.M, r1 = a.M - r0;
  const int64_t e0 = ((nodes - 1) * a.c0s + r0 * a.P) * 4;
  const int64_t e1 = r1 > 0 ? ((nodes - 1) * a.c1s + r1 * a.P) * 4 : 0;
  return e0 < kOffMax && e1 < kOffMax;
}

template <int NP>
hipError_t launch(Args a, hipStream_t st) {
  if (a.K % BK != 0 || a.k0 % BK != 0 || a.M % 32 != 0 || a.P % 4 != 0) return hipErrorNotSupported;
  if ((int64_t)a.M * a.K * 6 >= kOffMax) return hipErrorNotSupported;
  // 256-row workgroups of 8 waves on 16x16x32 MFMAs (each B stage split once for 256 rows) when M is a
  // multiple of 256 (gemm_split 7), else 128-row workgroups of 4 waves on 32x32x16 MFMAs (2).  Round 4's
  // other forms — the 256-row 32x32x16 kernel and the pipelined 16-k-stage ones, 7-12 % slower than 7
  // at every config shape (the smaller MFMA holds a higher clock under the power limit) — are lab forms
  // now (tools/lab_forms.hip).
  int v = mrp_host::tuning().gemm_split;
  const bool mf16 = mf16_ok(a);
  if (v < 0) v = mf16 ? 7 : 2;
  if (v == 7 && mf16) return launch_w<4, NP, gemm_nn_split_w4_mf16<NP>>(a, st);
  return launch_w<2, NP, gemm_nn_split_w2<NP>>(a, st);
}

// ------------------------------------------------------------------------------------------------
// Weight gradient  dW = dy [x; agg]^T, db = the row sums of dy: the NT product of split_nt.hpp, whose
// bodies these kernels and the edge encoder's backward (encoder_bwd_split.hip) instantiate.
// ------------------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(512, 1) gemm_nt_split_w4_mf16(NTArgs a) {
  gemm_nt_split_body<4, NP>(a, blockIdx.x, gridDim.x);
}

// ------------------------------------------------------------------------------------------------
// Weight gradient with a pre-split A (round 5; split_nt 4, the default where C >= 1024).  The kernel
// above splits BOTH operands in every workgroup: A = dy (M = C rows) is re-split by every column tile
// (2C / 128 of them: 32 at configs[3]) and B = [x; agg] by every row tile (C / 256), three times the
// NN kernel's split work per MFMA (PMC r04: 1.59x its VALU instructions, MFMA busy 0.55 vs 0.66).
// Here dy is split ONCE, by split_rows, into `pack`'s fragment-ordered image (4 bytes read and 6
// written per element, plus the row sums db in fixed-order groups), and arrives by LDS-DMA exactly as
// the NN kernel's weight does; B is split in-kernel as before.  Per output the products and their
// order are gemm_nt_split_body<4, true>'s, so at the same split dW is bit-identical to it.
// ------------------------------------------------------------------------------------------------

// g (nodes, M, P), node stride gs -> the packed A image of the M x K matrix, k = node P + pixel
// (P % 16 == 0): unit ((mb KS + ks) 3 + p) 64 + lane holds lane (r = lane & 31, h = lane >> 5)'s
// k = 16 ks + 8 h .. + 7 of row 32 mb + r, part p — `pack`'s layout.  One wave per (row block mb,
// group of G 16-k steps); its row sums over the group go to rsum[m][group] (null: none), the two lanes
// of a row added in one fixed order.  NP < 3: the image holds NP parts per (block, step) — unit
// ((mb KS + ks) NP + p) 64 + lane, 2 NP bytes per element of g; the row sums are of the full fp32 g in
// every form.
template <int NP>
__global__ void __launch_bounds__(256) split_rows(const float* __restrict__ g, int64_t gs, int32_t M, int32_t P,
                                                  int64_t KS, int32_t G, int32_t ngroups, u4* __restrict__ out,
                                                  float* __restrict__ rsum) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int MB = M / 32;
  if (wv >= (int64_t)MB * ngroups) return;
  const int mb = (int)(wv % MB), grp = (int)(wv / MB);
  const int r = lane & 31, h = lane >> 5;
  const int64_t ks0 = (int64_t)grp * G;
  const int64_t ks1 = ks0 + G < KS ? ks0 + G : KS;
  int64_t nd = 16 * ks0 / P;  // the step's node and first pixel (P % 16 == 0: a step is within a node)
  int px = (int)(16 * ks0 - nd * P);
  const float* row = g + (int64_t)(32 * mb + r) * P + 8 * h;
  u4* o = out + ((int64_t)mb * KS * NP) * 64 + lane;
  float sum = 0.f;
#pragma unroll 2
  for (int64_t ks = ks0; ks < ks1; ++ks) {
    const float* src = row + nd * gs + px;
    const f4 v0 = *reinterpret_cast<const f4*>(src), v1 = *reinterpret_cast<const f4*>(src + 4);
    sum += ((v0.x + v0.y) + (v0.z + v0.w)) + ((v1.x + v1.y) + (v1.z + v1.w));
    u4 pp[NP];
    const f2 x[4] = {{v0.x, v0.y}, {v0.z, v0.w}, {v1.x, v1.y}, {v1.z, v1.w}};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint32_t e[NP];
      splitp<NP>(x[i], e);
#pragma unroll
      for (int p = 0; p < NP; ++p) pp[p][i] = e[p];
    }
    u4* d = o + ks * NP * 64;
#pragma unroll
    for (int p = 0; p < NP; ++p) __builtin_nontemporal_store(pp[p], d + 64 * p);
    px += 16;
    if (px == P) {
      px = 0;
      ++nd;
    }
  }
  if (rsum != nullptr) {
    const float other = __shfl_xor(sum, 32, 64);
    const float tot = h == 0 ? sum + other : other + sum;
    if (h == 0) rsum[(int64_t)(32 * mb + r) * ngroups + grp] = tot;  // [m][group]: a row's partials contiguous
  }
}

// out[m] = the sum of part[m][0 .. n) in a fixed order: one wave per row, lane l adding partials
// l, l + 64, .. in order, then a fixed xor butterfly (every lane ends with the same value)
__global__ void __launch_bounds__(64) row_sums(const float* __restrict__ part, int32_t n, int32_t M,
                                               float* __restrict__ out) {
  const int m = blockIdx.x, lane = threadIdx.x;
  if (m >= M) return;
  const float* p = part + (int64_t)m * n;
  float v = 0.f;
  for (int i = lane; i < n; i += 64) v += p[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) out[m] = v;
}

template <int NP>
__global__ void __launch_bounds__(512, 1) gemm_nt_psa(NTArgs a) {
  gemm_nt_psa_body<NP>(a, blockIdx.x, gridDim.x);
}

// out = sum over the splits of part (fixed order); outb = the same over nsplitb row-sum partials
__global__ void __launch_bounds__(256) split_sum_nt(const f4* __restrict__ part, int nsplit, int64_t n4,
                                                    f4* __restrict__ out, const float* __restrict__ partb,
                                                    int nsplitb, int32_t M, float* __restrict__ outb) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t e = tid; e < n4; e += stride) {
    f4 v = part[e];
    for (int s = 1; s < nsplit; ++s) v += part[(int64_t)s * n4 + e];
    out[e] = v;
  }
  if (outb != nullptr)
    for (int64_t m = tid; m < M; m += stride) {
      float v = partb[m];
      for (int s = 1; s < nsplitb; ++s) v += partb[(int64_t)s * M + m];
      outb[m] = v;
    }
}

}  // namespace mrp_cs

hipError_t mrp_gemm::split_sum(const float* part, int nsplit, int64_t M, int64_t N, float* out, const float* partb,
                               int nsplitb, float* outb, hipStream_t st) {
  const int64_t n4 = M * N / 4;
  const int64_t blocks = (n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048;
  hipLaunchKernelGGL(mrp_cs::split_sum_nt, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<const f4*>(part),
                     nsplit, n4, reinterpret_cast<f4*>(out), partb, nsplitb, (int32_t)M, outb);
  return hipGetLastError();
}

// Splits of K = Nt P (whole stages): the count minimising (rounds of one-per-CU workgroups) x
// (stages per split) plus the partial-tile traffic of the final sum.
int mrp_gemm::nt_splits(int64_t tiles, int64_t ktot, int64_t M, int64_t N, int64_t* kchunk) {
  const int64_t stages = ktot / mrp_cs::BK;
  int best = 1;
  double best_cost = 1e300;
  for (int s = 1; s <= 256; ++s) {
    const int64_t per = (stages + s - 1) / s;
    if ((stages + per - 1) / per != s) continue;  // some split would be empty
    const int64_t rounds = (tiles * s + 255) / 256;
    // one 32-k stage of a 256 x 128 workgroup (12.6 MFLOP of bf16 products on one CU, ~1.3 us at the
    // CU's peak) takes ~1.6 us; the split sum streams the partial tiles at ~4 TB/s plus a launch
    const double cost = (double)rounds * per * 1.6 + (s > 1 ? (double)M * N * 4.0 * (s + 1) / 4.0e6 + 4.0 : 0.0);
    if (cost < best_cost) {
      best_cost = cost;
      best = s;
    }
  }
  *kchunk = ((stages + best - 1) / best) * mrp_cs::BK;
  return best;
}

using namespace mrp_cs;

extern "C" int64_t mrp_compress_split_pack_bytes(int32_t M, int32_t K) {
  if (M <= 0 || K <= 0 || M % 32 != 0 || K % 16 != 0) return 0;
  return (int64_t)M * K * 6;
}

extern "C" int mrp_compress_split_pack(const float* w, int64_t ld, int32_t transpose, int32_t M, int32_t K,
                                       void* packed, void* stream) {
  if (M <= 0 || K <= 0 || ld <= 0) return hipErrorInvalidValue;
  if (M % 32 != 0 || K % 16 != 0) return hipErrorNotSupported;
  if (!w || !packed || !aligned16(packed)) return hipErrorInvalidValue;
  const int64_t threads = (int64_t)(M / 32) * (K / 16) * 64;
  hipLaunchKernelGGL(pack, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), w,
                     ld, transpose ? 1 : 0, M, K, static_cast<u4*>(packed));
  return hipGetLastError();
}

extern "C" int mrp_compress_fwd_split_p(const float* x, int64_t x_node_stride, const float* agg,
                                        int64_t agg_node_stride, int32_t num_nodes, int32_t C, int32_t P,
                                        const void* packed_w, const float* bias, float* y, int64_t y_node_stride,
                                        int32_t parts, void* stream) {
  if (parts < 1 || parts > 3) return hipErrorInvalidValue;
  if (num_nodes < 0 || C < 0 || P < 0) return hipErrorInvalidValue;
  if (num_nodes == 0 || C == 0 || P == 0) return hipSuccess;
  const int64_t plane = (int64_t)C * P;
  if (!x || !agg || !packed_w || !y || x_node_stride < plane || agg_node_stride < plane || y_node_stride < plane)
    return hipErrorInvalidValue;
  if (C % 32 != 0 || P % 4 != 0 || (x_node_stride & 3) || (agg_node_stride & 3) || !aligned16(x) || !aligned16(agg) ||
      !aligned16(packed_w))
    return hipErrorNotSupported;
  Args a = {};
  a.ap = static_cast<const u4*>(packed_w);
  a.b0 = x;
  a.b0s = x_node_stride;
  a.b1 = agg;
  a.b1s = agg_node_stride;
  a.c0 = y;
  a.c0s = y_node_stride;
  a.c1 = y;
  a.c1s = y_node_stride;
  a.bias = bias;
  a.ncols = (int64_t)num_nodes * P;
  a.M = C;
  a.K = 2 * C;
  a.k0 = C;
  a.m0 = C;
  a.P = P;
  return dispatch_parts(parts, [&](auto np) { return launch<decltype(np)::value>(a, static_cast<hipStream_t>(stream)); });
}

extern "C" int mrp_compress_fwd_split(const float* x, int64_t x_node_stride, const float* agg, int64_t agg_node_stride,
                                      int32_t num_nodes, int32_t C, int32_t P, const void* packed_w, const float* bias,
                                      float* y, int64_t y_node_stride, void* stream) {
  return mrp_compress_fwd_split_p(x, x_node_stride, agg, agg_node_stride, num_nodes, C, P, packed_w, bias, y,
                                  y_node_stride, 3, stream);
}

extern "C" int mrp_compress_bwd_data_split_p(const float* gy, int64_t gy_node_stride, int32_t num_nodes, int32_t C,
                                             int32_t P, const void* packed_wt, float* gx, int64_t gx_node_stride,
                                             float* gagg, int64_t gagg_node_stride, int32_t parts, void* stream) {
  if (parts < 1 || parts > 3) return hipErrorInvalidValue;
  if (num_nodes < 0 || C < 0 || P < 0) return hipErrorInvalidValue;
  if (num_nodes == 0 || C == 0 || P == 0) return hipSuccess;
  const int64_t plane = (int64_t)C * P;
  if (!gy || !packed_wt || !gx || !gagg || gy_node_stride < plane || gx_node_stride < plane ||
      gagg_node_stride < plane)
    return hipErrorInvalidValue;
  if (C % 32 != 0 || P % 4 != 0 || (gy_node_stride & 3) || !aligned16(gy) || !aligned16(packed_wt))
    return hipErrorNotSupported;
  Args a = {};
  a.ap = static_cast<const u4*>(packed_wt);
  a.b0 = gy;
  a.b0s = gy_node_stride;
  a.b1 = gy;
  a.b1s = gy_node_stride;
  a.c0 = gx;
  a.c0s = gx_node_stride;
  a.c1 = gagg;
  a.c1s = gagg_node_stride;
  a.bias = nullptr;
  a.ncols = (int64_t)num_nodes * P;
  a.M = 2 * C;
  a.K = C;
  a.k0 = C;
  a.m0 = C;
  a.P = P;
  return dispatch_parts(parts, [&](auto np) { return launch<decltype(np)::value>(a, static_cast<hipStream_t>(stream)); });
}

extern "C" int mrp_compress_bwd_data_split(const float* gy, int64_t gy_node_stride, int32_t num_nodes, int32_t C,
                                           int32_t P, const void* packed_wt, float* gx, int64_t gx_node_stride,
                                           float* gagg, int64_t gagg_node_stride, void* stream) {
  return mrp_compress_bwd_data_split_p(gy, gy_node_stride, num_nodes, C, P, packed_wt, gx, gx_node_stride, gagg,
                                       gagg_node_stride, 3, stream);
}

// (the two host functions split_nt.hpp declares: encoder_bwd_split.hip calls them too)
int64_t mrp_cs::nt_workspace(int64_t M, int64_t N, int64_t ktot) {
  const int64_t tiles = ((M + NTGeo<4>::TM - 1) / NTGeo<4>::TM) * ((N + TN - 1) / TN);
  int64_t kchunk;
  return splitk_place(nt_splits(tiles, ktot, M, N, &kchunk), M, N).bytes;
}

hipError_t mrp_cs::nt_run(NTArgs a, int64_t M, int64_t N, int32_t nodes, float* out, float* outb, void* workspace,
                          int64_t workspace_bytes, hipStream_t st, int parts) {
  using G = NTGeo<4>;
  a.mtiles = (int32_t)((M + G::TM - 1) / G::TM);
  a.ntiles = (int32_t)((N + TN - 1) / TN);
  a.ktot = (int64_t)nodes * a.P;
  const int ns = nt_splits((int64_t)a.mtiles * a.ntiles, a.ktot, M, N, &a.kchunk);
  const SplitK pl = splitk_place(ns, M, N, out, outb, workspace, workspace_bytes);
  if (pl.err != hipSuccess) return pl.err;
  a.out = pl.out;
  a.outb = pl.outb;
  a.M = (int32_t)M;
  a.N = (int32_t)N;
  const int64_t grid = (int64_t)a.mtiles * a.ntiles * ns;
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  // the 32-k-stage form on 16x16x32 MFMAs (split_nt 3; the compress weight gradient takes nt_run_psa
  // instead at 4, and at -1 where C >= 1024).  Round 4's 32x32x16 forms (the 32-k-stage one and the
  // pipelined 16-k-stage one), 4-5 % slower at every config shape, are lab forms (tools/lab_forms.hip).
  a.group = mrp_host::tuning().nt_group;
  const hipError_t e = dispatch_parts(parts, [&](auto np) {
    constexpr int NP = decltype(np)::value;
    return launch_lds<gemm_nt_split_w4_mf16<NP>>(NTGeo<4, NP>::LDS_BYTES, dim3((unsigned)grid), dim3(G::THREADS), st, a);
  });
  if (e != hipSuccess || ns == 1) return e;
  return split_sum(pl.out, ns, M, N, out, pl.outb, ns, outb, st);
}

namespace {
bool nt_split_ok(int32_t num_nodes, int32_t C, int32_t P) {
  return num_nodes > 0 && C > 0 && C % 64 == 0 && P % BK == 0;
}

// The pre-split-A weight gradient (split_rows + gemm_nt_psa): workspace = [partial tiles (splits > 1)]
// [dy's packed image, M K 6 bytes][row-sum group partials].  The default (split_nt -1) where C >= 1024
// and the image is addressable with 32-bit buffer offsets; forced by split_nt 4.  The GEMM alone runs
// 15-20 % faster than gemm_nt_split_w4_mf16 at every config shape (configs[3]: 281 vs 333 us,
// 244 TF/s); behind the data gradient in a training step (tools/exp_dy_image.py, HIP graph, the chip at
// its power limit) the pair gains 3 % at C = 1024 / 2048 (configs[4] 1278 vs 1320 us, [3] 626 vs
// 648), 1 % at C = 1280 and loses 4 % at C = 512 (the split pass moves 10 bytes per element of dy
// for a re-split factor of only 2C / 128 = 8 there).
struct PsaPlan {
  int ns, G, ngroups;
  int64_t kchunk, img_off, rs_off, bytes;
};

bool psa_ok(int64_t M, int64_t ktot) {
  const int v = mrp_host::tuning().split_nt;
  return ((v < 0 && M >= 1024) || v == 4) && M % 32 == 0 && ktot % BK == 0 && M * ktot * 6 < kOffMax;
}

PsaPlan psa_plan(int64_t M, int64_t N, int64_t ktot) {
  PsaPlan q{};
  const int64_t tiles = ((M + NTGeo<4>::TM - 1) / NTGeo<4>::TM) * ((N + TN - 1) / TN);
  q.ns = nt_splits(tiles, ktot, M, N, &q.kchunk);
  // split_rows: one wave per (32-row block, group of G 16-k steps), ~8192 waves
  const int64_t KS = ktot / 16, MB = M / 32;
  int64_t G = (KS * MB + 8191) / 8192;
  if (G < 1) G = 1;
  q.G = (int)G;
  q.ngroups = (int)((KS + G - 1) / G);
  auto al = [](int64_t v) { return (v + 255) / 256 * 256; };
  q.img_off = al(q.ns > 1 ? (int64_t)q.ns * M * N * 4 : 0);
  q.rs_off = al(q.img_off + M * ktot * 6);
  q.bytes = q.rs_off + (int64_t)q.ngroups * M * 4;
  return q;
}

// The pre-split-A GEMM proper: dW (+ db from rparts row-sum partials [M][nparts]) from dy's packed
// image `img` (split_rows' layout); the workspace holds the partial tiles when the plan splits K
hipError_t psa_gemm(NTArgs a, int64_t M, int64_t N, const u4* img, const float* rparts, int nparts, float* out,
                    float* outb, void* tiles_ws, hipStream_t st, int parts) {
  using G = NTGeo<4>;
  const PsaPlan q = psa_plan(M, N, a.ktot);
  a.ap = img;
  a.mtiles = (int32_t)((M + G::TM - 1) / G::TM);
  a.ntiles = (int32_t)((N + TN - 1) / TN);
  a.kchunk = q.kchunk;
  a.out = q.ns == 1 ? out : static_cast<float*>(tiles_ws);
  a.outb = nullptr;
  a.M = (int32_t)M;
  a.N = (int32_t)N;
  const int64_t grid = (int64_t)a.mtiles * a.ntiles * q.ns;
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  a.group = mrp_host::tuning().nt_group;
  hipError_t e = dispatch_parts(parts, [&](auto np) {
    constexpr int NP = decltype(np)::value;
    return launch_lds<gemm_nt_psa<NP>>(NTGeo<4, NP>::LDS_BYTES, dim3((unsigned)grid), dim3(G::THREADS), st, a);
  });
  if (e != hipSuccess) return e;
  if (outb != nullptr) {
    hipLaunchKernelGGL(row_sums, dim3((unsigned)M), dim3(64), 0, st, rparts, nparts, (int32_t)M, outb);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (q.ns == 1) return hipSuccess;
  return split_sum(static_cast<const float*>(tiles_ws), q.ns, M, N, out, nullptr, 0, nullptr, st);
}

// (the plan, and so the workspace layout and bound, is the same for every part count: a reduced form's
// image, 2 parts bytes per element, fills the front of the six-byte one's room)
hipError_t nt_run_psa(NTArgs a, int64_t M, int64_t N, int32_t nodes, float* out, float* outb, void* workspace,
                      int64_t workspace_bytes, hipStream_t st, int parts) {
  a.ktot = (int64_t)nodes * a.P;
  const PsaPlan q = psa_plan(M, N, a.ktot);
  if (workspace == nullptr || workspace_bytes < q.bytes || !aligned16(workspace)) return hipErrorInvalidValue;
  char* ws = static_cast<char*>(workspace);
  u4* img = reinterpret_cast<u4*>(ws + q.img_off);
  float* rs = reinterpret_cast<float*>(ws + q.rs_off);
  const int64_t waves = (M / 32) * q.ngroups;
  const dim3 sgrid((unsigned)((waves + 3) / 4));
  float* rsp = outb != nullptr ? rs : nullptr;
  dispatch_parts(parts, [&](auto np) {
    hipLaunchKernelGGL(split_rows<decltype(np)::value>, sgrid, dim3(256), 0, st, a.g, a.gs, (int32_t)M, a.P,
                       a.ktot / 16, q.G, q.ngroups, img, rsp);
  });
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return psa_gemm(a, M, N, img, rs, q.ngroups, out, outb, ws, st, parts);
}

}  // namespace

extern "C" int64_t mrp_compress_bwd_weight_split_workspace(int32_t num_nodes, int32_t C, int32_t P) {
  if (!nt_split_ok(num_nodes, C, P)) return 0;
  const int64_t ktot = (int64_t)num_nodes * P;
  if (psa_ok(C, ktot)) return psa_plan(C, 2 * (int64_t)C, ktot).bytes;
  return nt_workspace(C, 2 * (int64_t)C, ktot);
}

extern "C" int mrp_compress_bwd_weight_split_p(const float* gy, int64_t gy_node_stride, const float* x,
                                               int64_t x_node_stride, const float* agg, int64_t agg_node_stride,
                                               int32_t num_nodes, int32_t C, int32_t P, float* gw, float* gbias,
                                               void* workspace, int64_t workspace_bytes, int32_t parts,
                                               void* stream) {
  if (parts < 1 || parts > 3) return hipErrorInvalidValue;
  if (num_nodes < 0 || C < 0 || P < 0) return hipErrorInvalidValue;
  if (C == 0) return hipSuccess;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t M = C, N = 2 * (int64_t)C;
  if (gw == nullptr && gbias == nullptr) return hipSuccess;
  if (num_nodes == 0 || P == 0) {  // empty sum
    if (gw && hipMemsetAsync(gw, 0, M * N * 4, st) != hipSuccess) return hipErrorUnknown;
    if (gbias && hipMemsetAsync(gbias, 0, M * 4, st) != hipSuccess) return hipErrorUnknown;
    return hipSuccess;
  }
  const int64_t plane = (int64_t)C * P;
  if (!gy || !x || !agg || !gw || gy_node_stride < plane || x_node_stride < plane || agg_node_stride < plane)
    return hipErrorInvalidValue;
  if (!nt_split_ok(num_nodes, C, P) || (gy_node_stride & 3) || (x_node_stride & 3) || (agg_node_stride & 3) ||
      !aligned16(gy) || !aligned16(x) || !aligned16(agg) || !aligned16(gw))
    return hipErrorNotSupported;
  NTArgs a = {};
  a.g = gy;
  a.gs = gy_node_stride;
  a.s0 = x;
  a.s0s = x_node_stride;
  a.s1 = agg;
  a.s1s = agg_node_stride;
  a.n0 = C;
  a.P = P;
  if (psa_ok(M, (int64_t)num_nodes * P))
    return nt_run_psa(a, M, N, num_nodes, gw, gbias, workspace, workspace_bytes, st, parts);
  return nt_run(a, M, N, num_nodes, gw, gbias, workspace, workspace_bytes, st, parts);
}

extern "C" int mrp_compress_bwd_weight_split(const float* gy, int64_t gy_node_stride, const float* x,
                                             int64_t x_node_stride, const float* agg, int64_t agg_node_stride,
                                             int32_t num_nodes, int32_t C, int32_t P, float* gw, float* gbias,
                                             void* workspace, int64_t workspace_bytes, void* stream) {
  return mrp_compress_bwd_weight_split_p(gy, gy_node_stride, x, x_node_stride, agg, agg_node_stride, num_nodes, C, P,
                                         gw, gbias, workspace, workspace_bytes, 3, stream);
}
