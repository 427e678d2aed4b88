// split_nt.hpp — the split-bf16 NT product (both operands k-contiguous rows) as compress_split.hip (the
// compress weight gradient) and encoder_bwd_split.hip (the edge encoder's backward) both build kernels
// from it: the argument struct, the workgroup geometry, the two device bodies (gemm_nt_split_body splits
// both operands in the kernel; PsaBody reads its A operand pre-split by LDS-DMA) with the pieces the two
// share, and the host side that compress_split.hip defines for both units.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_common.hpp"
#include "split_common.hpp"

namespace mrp_cs {

// vector types, rsrc, xcd_remap, tile_of, the LDS image offsets boff / rowoff: gemm_common.hpp; the bf16
// split (split2 / splitp), the partial products (mma6 / mma6_16) and the counted waits: split_common.hpp
using namespace mrp_gemm;

constexpr int TN = 128, BK = 32;

// ------------------------------------------------------------------------------------------------
// Weight gradient  dW[m][n] = sum_k dy[m][k] S[n][k],  db[m] = sum_k dy[m][k],  k = (node, pixel):
// both operands are k-contiguous rows (a channel's P pixels of one node), so no transposing read is
// needed — each thread loads 16-byte row pieces of a stage (A = dy: TMW rows, B = [x; agg]: 128 rows,
// 32 pixels of one node), splits them and stores the three bf16 parts as [row][32 k] 64-byte rows (the
// row's four 16-byte chunks rotated by (row >> 2) & 3, so the fragment reads meet every bank once),
// from which a lane's eight consecutive k are one ds_read_b128.  K = Nt P is split over workgroups
// (whole stages, each within one node) into per-split partial tiles summed in a fixed order by
// split_sum_nt (deterministic); db from the fp32 dy pieces as loaded, per split.
// ------------------------------------------------------------------------------------------------
struct NTArgs {
  const float* g;  // dy (nodes, M, P), node stride gs
  int64_t gs;
  const float* s0;  // rows [0, n0) of B: x (nodes, n0, P)
  int64_t s0s;
  const float* s1;  // rows [n0, N): agg
  int64_t s1s;
  float* out;   // [split][M][N]
  float* outb;  // [split][M] or null
  int64_t ktot, kchunk;
  int32_t M, N, n0, P, mtiles, ntiles;
  const u4* ap;  // gemm_nt_psa: the pre-split image of g (split_rows), KS = ktot / 16 16-k steps per row block
  int32_t group;  // tile order (tile_of)
};

template <int WMW, int NP = 3>
struct NTGeo {
  static constexpr int TM = 64 * WMW, NW = 2 * WMW, THREADS = 64 * NW;
  static constexpr int ROWB = BK * 2;                                  // bytes per [row][32 k] bf16 row
  static constexpr int A_PART = TM * ROWB, B_PART = TN * ROWB;
  static constexpr int BUF_BYTES = NP * (A_PART + B_PART);
  static constexpr int LDS_BYTES = 2 * BUF_BYTES;                      // 144 KiB at WMW 4, NP 3 (x NP / 3)
  static constexpr int RPP = THREADS / 8;                              // rows per load pass (8 pieces a row)
  static constexpr int AJ = TM / RPP, BJ = TN / RPP;                   // A / B pieces per thread per stage
};

// ---- what the two bodies share ----------------------------------------------------------------------
// (The B operand's row offsets and stage walk, and the partial-tile store, stay written out in each body:
// as a struct, or a helper, they changed the k-loop or a branch of the compiled kernels —
// profiles/split_nt_device_code.md.)

// A workgroup's share of the product: split `split` of K (stages kbeg / BK .. + nst) of tile (mt, nt), the
// tiles of a split in the XCD-aware order (orig of nwg workgroups; TM rows per tile)
template <int TM>
struct NTTile {
  int split, mt, nt, mbase, nbase, nst;
  int64_t kbeg;
  __device__ __forceinline__ NTTile(const NTArgs& a, int orig, int nwg) {
    const int id = xcd_remap(orig, nwg);
    const int tiles = a.mtiles * a.ntiles;
    split = id / tiles;
    tile_of(id - split * tiles, a.mtiles, a.ntiles, a.group, mt, nt);
    mbase = mt * TM, nbase = nt * TN;
    kbeg = (int64_t)split * a.kchunk;
    const int64_t kend = kbeg + a.kchunk < a.ktot ? kbeg + a.kchunk : a.ktot;
    nst = kend > kbeg ? (int)((kend - kbeg) / BK) : 0;
  }
};

// a thread's 16-byte piece pc4 (4 k) of row `row` of a stage, split into the NP part images [row][32 k]
// at img, img + part_bytes, ..
template <int NP>
__device__ __forceinline__ void put(char* img, int part_bytes, int row, int pc4, const f4& v) {
  f2 lo, hi;
  lo.x = v.x, lo.y = v.y, hi.x = v.z, hi.y = v.w;
  uint32_t l[NP], h[NP];
  splitp<NP>(lo, l);
  splitp<NP>(hi, h);
  const uint32_t o = rowoff(row, pc4 >> 1) + 8 * (pc4 & 1);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    u2 u;
    u.x = l[p], u.y = h[p];
    *reinterpret_cast<u2*>(img + p * part_bytes + o) = u;
  }
}

__device__ __forceinline__ void zero_acc2(Acc2s (&acc)[4][4]) {
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[mi][ni].hi[r] = acc[mi][ni].lo[r] = 0.f;
}

// The products on v_mfma_f32_16x16x32_bf16 (the wave's 64 x 64 as 4 x 4 tiles of 16 x 16, one MFMA per
// 32 k), which holds a higher clock than the 32x32x16 shape under the chip's power limit
// (MI355X_MICROARCH.md, DVFS give-back item 7); the 32x32x16 forms are lab forms (tools/lab_forms.hip)
template <int WMW, int NP = 3>
__device__ __forceinline__ void gemm_nt_split_body(const NTArgs& a, int orig, int nwg) {
  using G = NTGeo<WMW, NP>;
  extern __shared__ u4 lds[];
  char* ldsb = reinterpret_cast<char*>(lds);
  const NTTile<G::TM> t(a, orig, nwg);
  const int split = t.split, nt = t.nt, mbase = t.mbase, nbase = t.nbase, nst = t.nst;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = w >> 1, wn = w & 1;

  // ---- loads: thread t -> piece (t & 7) (4 pixels) of rows (t >> 3) + RPP j
  const int pc4 = threadIdx.x & 7, r0 = threadIdx.x >> 3;
  int64_t aoff[G::AJ], boffs[G::BJ];  // row offsets within a node (elements), fixed
  bool bhi[G::BJ];
#pragma unroll
  for (int j = 0; j < G::AJ; ++j) aoff[j] = (int64_t)min(mbase + r0 + G::RPP * j, a.M - 1) * a.P + 4 * pc4;
#pragma unroll
  for (int j = 0; j < G::BJ; ++j) {
    const int n = min(nbase + r0 + G::RPP * j, a.N - 1);
    bhi[j] = n >= a.n0;
    boffs[j] = (int64_t)(bhi[j] ? n - a.n0 : n) * a.P + 4 * pc4;
  }
  f4 areg[G::AJ], breg[G::BJ];
  float rsum[G::AJ];
#pragma unroll
  for (int j = 0; j < G::AJ; ++j) rsum[j] = 0.f;
  // stages in order, k = (node ind, pixel ipx) advanced per stage (P % BK == 0: a stage never straddles
  // two nodes) — an int64 division per stage put ~80 scalar instructions between the barrier and the
  // stage's loads
  int64_t ind = t.kbeg / a.P;
  int ipx = (int)(t.kbeg - ind * a.P);
  auto load = [&]() {
    const float* gp = a.g + ind * a.gs + ipx;
    const float* xp = a.s0 + ind * a.s0s + ipx;
    const float* ap = a.s1 + ind * a.s1s + ipx;
#pragma unroll
    for (int j = 0; j < G::AJ; ++j) areg[j] = *reinterpret_cast<const f4*>(gp + aoff[j]);
#pragma unroll
    for (int j = 0; j < G::BJ; ++j) breg[j] = *reinterpret_cast<const f4*>((bhi[j] ? ap : xp) + boffs[j]);
    ipx += BK;
    if (ipx == a.P) {
      ipx = 0;
      ++ind;
    }
  };
  auto store = [&](int buf) {
    char* base = ldsb + buf * G::BUF_BYTES;
#pragma unroll
    for (int j = 0; j < G::AJ; ++j) {
      rsum[j] += (areg[j].x + areg[j].y) + (areg[j].z + areg[j].w);
      put<NP>(base, G::A_PART, r0 + G::RPP * j, pc4, areg[j]);
    }
#pragma unroll
    for (int j = 0; j < G::BJ; ++j) put<NP>(base + NP * G::A_PART, G::B_PART, r0 + G::RPP * j, pc4, breg[j]);
  };
  // lane (r16, q) reads k = 8 q .. 8 q + 7 (chunk q) of row r16 of a 16-row block
  const int r16 = lane & 15, q = lane >> 4;
  Acc2s acc[4][4];
  zero_acc2(acc);
  if (nst > 0) load();
#pragma unroll 1
  for (int s = 0; s < nst; ++s) {
    const int buf = s & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    store(buf);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (s + 1 < nst) load();
    const char* base = ldsb + buf * G::BUF_BYTES;
    const char* bb = base + NP * G::A_PART;
    bf8 bf[4][NP];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int p = 0; p < NP; ++p)
        bf[ni][p] = __builtin_bit_cast(bf8, *reinterpret_cast<const u4*>(bb + p * G::B_PART +
                                                                          rowoff(64 * wn + 16 * ni + r16, q)));
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      bf8 af[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p)
        af[p] = __builtin_bit_cast(bf8, *reinterpret_cast<const u4*>(base + p * G::A_PART +
                                                                      rowoff(64 * wm + 16 * mi + r16, q)));
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) mma6_16<NP>(af, bf[ni], acc[mi][ni]);
    }
  }
  float* out = a.out + (int64_t)split * a.M * a.N;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int n = nbase + 64 * wn + 16 * ni + r16;
    if (n >= a.N) continue;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mbase + 64 * wm + 16 * mi + 4 * q + r;
        if (m < a.M) out[(int64_t)m * a.N + n] = __fadd_rn(acc[mi][ni].hi[r], acc[mi][ni].lo[r]);
      }
  }
  if (a.outb != nullptr && nt == 0) {  // the column-tile-0 workgroups write the split's row sums
#pragma unroll
    for (int j = 0; j < G::AJ; ++j) {
      float v = rsum[j];  // the 8 threads of a row are 8 consecutive lanes (t & 7)
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      const int m = mbase + r0 + G::RPP * j;
      if (pc4 == 0 && m < a.M) a.outb[(int64_t)split * a.M + m] = v;
    }
  }
}

// The same product with a pre-split A: its packed image (split_rows, dzT_pack or `pack`) arrives by
// LDS-DMA exactly as the NN kernel's weight does; B is split in the kernel as above.  Per output the
// products and their order are gemm_nt_split_body<4>'s, so at the same split the result is bit-identical.
// NP: the parts kept of both operands; the image at a.ap holds NP parts per (block, step) (split_rows<NP>;
// NP 3: `pack`'s layout)
// (a static member of a class template, reached through the function template below: hipcc's host pass
// drops a function template's specialization with these inline-asm immediates when a non-template
// kernel names it — gemm_nt_psa<3>'s host stub went with it)
template <int NP>
struct PsaBody {
static __device__ __forceinline__ void run(const NTArgs& a, int orig, int nwg) {
  using G = NTGeo<4, NP>;
  constexpr int A_BYTES = 16 * NP * 1024;  // 256 rows x 32 k x NP parts: 16 NP 1-KiB pieces, 2 NP per wave
  constexpr int BP = G::B_PART, BUF = A_BYTES + NP * BP;  // NP 3: 72 KiB per buffer, two buffers
  extern __shared__ u4 lds[];
  char* ldsb = reinterpret_cast<char*>(lds);
  const NTTile<G::TM> t(a, orig, nwg);
  const int split = t.split, mt = t.mt, mbase = t.mbase, nbase = t.nbase, nst = t.nst;
  const int64_t kbeg = t.kbeg;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int64_t KS = a.ktot / 16;
  const int MB = a.M / 32;

  // ---- A: LDS-DMA pieces pc = (mbl 2 + ksl) NP + p of the stage, pc = w + 8 i
  const __amdgpu_buffer_rsrc_t ra = rsrc(a.ap);
  uint32_t va[2 * NP];
#pragma unroll
  for (int i = 0; i < 2 * NP; ++i) {
    const int pc = w + 8 * i;
    const int mbl = pc / (2 * NP), kp = pc % (2 * NP);  // kp = NP ksl + p
    const int mb = min(mt * 8 + mbl, MB - 1);  // blocks past M: any valid data, never stored
    va[i] = (uint32_t)((((int64_t)mb * KS + kbeg / 16) * NP + kp) * 64 + lane) * 16;
  }
  auto issue_a = [&](int s, int buf) {
#pragma unroll
    for (int i = 0; i < 2 * NP; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, lds + (buf * BUF + (w + 8 * i) * 1024) / 16, 16, va[i],
                                               (uint32_t)s * 2 * NP * 1024, 0, 0);
  };

  // ---- B: thread t -> piece (t & 7) (4 pixels) of rows (t >> 3) + 64 j of the stage
  const int pc4 = threadIdx.x & 7, r0 = threadIdx.x >> 3;
  int64_t boffs[G::BJ];
  bool bhi[G::BJ];
#pragma unroll
  for (int j = 0; j < G::BJ; ++j) {
    const int n = min(nbase + r0 + G::RPP * j, a.N - 1);
    bhi[j] = n >= a.n0;
    boffs[j] = (int64_t)(bhi[j] ? n - a.n0 : n) * a.P + 4 * pc4;
  }
  f4 breg[G::BJ];
  int64_t ind = kbeg / a.P;
  int ipx = (int)(kbeg - ind * a.P);
  auto load_b = [&]() {
    const float* xp = a.s0 + ind * a.s0s + ipx;
    const float* ap = a.s1 + ind * a.s1s + ipx;
#pragma unroll
    for (int j = 0; j < G::BJ; ++j) breg[j] = *reinterpret_cast<const f4*>((bhi[j] ? ap : xp) + boffs[j]);
    ipx += BK;
    if (ipx == a.P) {
      ipx = 0;
      ++ind;
    }
  };
  auto store_b = [&](int buf) {
    char* img = ldsb + buf * BUF + A_BYTES;
#pragma unroll
    for (int j = 0; j < G::BJ; ++j) put<NP>(img, BP, r0 + G::RPP * j, pc4, breg[j]);
  };

  // fragments: lane (r16, qq) holds k = 8 qq .. 8 qq + 7 of row r16 of a 16-row block.  A: 16-row block mi
  // of the wave is half (mi & 1) of 32-row block 2 wm + (mi >> 1); the packed image holds 16-k steps in the
  // 32 x 32 x 16 lane order, so the lane reads step qq >> 1, slot 16 (mi & 1) + r16 + 32 (qq & 1) (the NN
  // kernel's A reads).  B: chunk qq of row 64 wn + 16 ni + r16 of the [row][32 k] images.
  const int r16 = lane & 15, qq = lane >> 4;
  const uint32_t abase0 = (uint32_t)reinterpret_cast<uintptr_t>(ldsb + (r16 + 32 * (qq & 1)) * 16 +
                                                                 ((4 * wm + (qq >> 1)) * NP) * 1024);
  uint32_t bro[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
    bro[ni] = (uint32_t)reinterpret_cast<uintptr_t>(ldsb + A_BYTES + rowoff(64 * wn + 16 * ni + r16, qq));
  Acc2s acc[4][4];
  zero_acc2(acc);
  if (nst > 0) {
    issue_a(0, 0);
    load_b();
  }
#pragma unroll 1
  for (int s = 0; s < nst; ++s) {
    const int buf = s & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // stage s's B registers and own A pieces landed
    store_b(buf);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // stage s complete for every wave; every wave is past stage s - 1's reads
    {
      // every fragment read by inline asm with counted waits (a C++ LDS read beside the LDS-DMA issued
      // below would make hipcc wait for the DMA): A row 0, B columns 0..3, then A row mi + 1 under row
      // mi's MFMAs
      const uint32_t ab = abase0 + (uint32_t)(buf * BUF);
      u4 ar[2][NP], br[4][NP];
      auto read_a16 = [&](int mi, u4 (&rg)[NP]) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
          asm volatile("ds_read_b128 %0, %1 offset:%2"
                       : "=v"(rg[p])
                       : "v"(ab), "i"((mi >> 1) * 2048 * NP + p * 1024 + 256 * (mi & 1)));
      };
      read_a16(0, ar[0]);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int p = 0; p < NP; ++p)
          asm volatile("ds_read_b128 %0, %1 offset:%2"
                       : "=v"(br[ni][p])
                       : "v"(bro[ni] + (uint32_t)(buf * BUF)), "i"(p * BP));
      if (s + 1 < nst) {
        issue_a(s + 1, buf ^ 1);
        load_b();
      }
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
            // A row 0 and B columns 0..ni landed: younger are NP (3 - ni) B reads and A row 1's NP
            // (NP 3: 12, 9, 6, 3)
            if (ni == 0)
              wait_lgkm<4 * NP>();
            else if (ni == 1)
              wait_lgkm<3 * NP>();
            else if (ni == 2)
              wait_lgkm<2 * NP>();
            else
              wait_lgkm<NP>();
            if (ni == 0) pin<NP>(cur);
            pin<NP>(br[ni]);
          }
          bf8 af[NP], bfr[NP];
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            af[p] = __builtin_bit_cast(bf8, cur[p]);
            bfr[p] = __builtin_bit_cast(bf8, br[ni][p]);
          }
          mma6_16<NP>(af, bfr, acc[mi][ni]);
          if (mi == 0 || ni == 3) __builtin_amdgcn_sched_barrier(0);  // keep each wait before its MFMAs
        }
      }
    }
  }
  float* out = a.out + (int64_t)split * a.M * a.N;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int n = nbase + 64 * wn + 16 * ni + r16;
    if (n >= a.N) continue;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mbase + 64 * wm + 16 * mi + 4 * qq + r;
        if (m < a.M) out[(int64_t)m * a.N + n] = __fadd_rn(acc[mi][ni].hi[r], acc[mi][ni].lo[r]);
      }
  }
}
};
template <int NP>
__device__ __forceinline__ void gemm_nt_psa_body(const NTArgs& a, int orig, int nwg) {
  PsaBody<NP>::run(a, orig, nwg);
}

// compress_split.hip: workspace bytes of one NT product (split-K partial tiles, and their row sums)
int64_t nt_workspace(int64_t M, int64_t N, int64_t ktot);

// compress_split.hip: out (M x N) = sum_k g[m][k] s[n][k] (+ row sums of g into outb), k = (node, pixel)
// over `nodes` nodes of P pixels, on gemm_nt_split_w4_mf16; a.g/gs, a.s0/s0s, a.s1/s1s, a.n0, a.P set by
// the caller; parts = the bf16 parts kept (1..3)
hipError_t nt_run(NTArgs a, int64_t M, int64_t N, int32_t nodes, float* out, float* outb, void* workspace,
                  int64_t workspace_bytes, hipStream_t st, int parts = 3);

}  // namespace mrp_cs
