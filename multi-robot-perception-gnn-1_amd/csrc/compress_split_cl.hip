// compress_split_cl.hip — compress_split.hip's three products on pixel-major (torch.channels_last) fp32
// feature maps, gfx950 (MI355X / CDNA4).
//
// A pixel-major tensor is (pointer, node stride, pixel stride) in elements, as in compress_half_cl.hip:
// pixel row r = (node r / P, pixel r % P) is C contiguous channels at node * node_stride + pixel *
// pixel_stride.  Per pixel row r, everything fp32:
//     forward      y[r] = W [x[r]; a[r]] + b                    M = C,  K = 2C (k from x, then a)
//     data grad    [gx[r]; ga[r]] = W^T gy[r]                   M = 2C, K = C  (rows to gx, then ga)
//     weight grad  dW = sum_r gy[r] [x[r]; a[r]]^T, db = sum_r gy[r]
// The arithmetic is compress_split.hip's (split_common.hpp): the exact bf16 split of each fp32 operand,
// the partial products with i + j < NP, a0 b0 in its own accumulator, NP = 3 / 2 / 1 a template parameter.
//
// Forward / data gradient (gemm_cl_split<NP>): gemm_nt_psa's workgroup (compress_split.hip PsaBody: 8
// waves, a 256 x 128 tile as 4 x 2 waves of 4 x 4 v_mfma_f32_16x16x32_bf16 tiles, 32-k stages in two LDS
// buffers, one barrier per stage, the counted-lgkmcnt fragment schedule).  A is the packed weight image of
// mrp_compress_split_pack by LDS-DMA (a reduced form fetches its NP parts of the three).  B is 128 pixel
// rows x 32 k: the reduction index (channels) is contiguous, so thread t loads 8 k of row t >> 2 as two
// 16-byte pieces, splits them and stores one 16-byte piece per part into [row][32 k] images (rowoff's
// rotated chunks); the fragments come back by ds_read_b128 — no transposing read.  Pixels are rows: any P,
// a tile may cross node boundaries, rows past the end are loaded from the last row and never stored.  A
// lane's four accumulator registers are four consecutive channels of one pixel: the epilogue is one
// 16-byte store per (tile, lane) through a 64-bit address.
//
// Weight gradient (gemm_wg_cl_split<NP>): k is the pixel row, both operands are k-strided with channels
// contiguous.  A stage is 32 pixel rows x (256 gy channels | 128 [x; a] channels); each thread loads
// 16-byte pieces (4 channels of one row), splits them and stores 8 bytes per part into row-major
// [k][128 columns] images with gemm_nn_split_body's XOR swizzle (gy: two images per part); both operands'
// fragments come back through ds_read_b64_tr_b16.  72 KiB per buffer at NP = 3, two buffers.  A stage may
// cross a node boundary (each thread walks its own row's (node, pixel)); rows past the split's end are
// zero-filled.  K = nodes P is split over workgroups into fp32 partial tiles summed in a fixed order by
// split_sum (no atomics); db is the fp32 sum of the full gy in every mode, per split, formed in a fixed
// order by a few extra workgroups of the same launch (colsum_cl), then summed across the splits.

#include "compress_half_common.hpp"  // plan_splits
#include "mrp_gnn.h"
#include "split_common.hpp"
#include "tuning.hpp"

namespace mrp_cscl {

using namespace mrp_cs;

constexpr int TM = 256, TN = 128, BK = 32, THREADS = 512;

struct Args {
  const u4* ap;     // packed A (mrp_compress_split_pack's image: three 1 KiB pieces per (block, step))
  const float* b0;  // k < k0: node / pixel strides in elements
  int64_t b0n, b0p;
  const float* b1;  // k >= k0
  int64_t b1n, b1p;
  float* c0;  // output channels [0, m0)
  int64_t c0n, c0p;
  float* c1;  // output channels [m0, M)
  int64_t c1n, c1p;
  const float* bias;  // (M) or null
  int64_t nrows;      // nodes * P
  int32_t M, K, k0, m0, P, mtiles;
  int32_t group;  // tile order (tile_of)
};

template <int NP>
struct ClGeo {
  static constexpr int A_BYTES = 16 * NP * 1024;  // 256 rows x 32 k x NP parts: 16 NP 1-KiB pieces, 2 NP per wave
  static constexpr int B_PART = TN * BK * 2;      // one [128 rows][32 k] bf16 image: 8 KiB
  static constexpr int BUF = A_BYTES + NP * B_PART;
  static constexpr int LDS_BYTES = 2 * BUF;  // NP 3: 144 KiB, 2: 96 KiB, 1: 48 KiB
};

// (a static member of a class template, as compress_split.hip's PsaBody: hipcc's host pass drops a function
// template's specialization with these inline-asm immediates)
template <int NP>
struct ClBody {
static __device__ __forceinline__ void run(const Args& a) {
  using G = ClGeo<NP>;
  constexpr int A_BYTES = G::A_BYTES, BP = G::B_PART, BUF = G::BUF;
  extern __shared__ u4 lds[];
  char* ldsb = reinterpret_cast<char*>(lds);
  const int nwg = gridDim.x;
  const int id = xcd_remap(blockIdx.x, nwg);
  int mt, nt;
  tile_of(id, a.mtiles, nwg / a.mtiles, a.group, mt, nt);
  const int64_t nbase = (int64_t)nt * TN;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int KS = a.K / 16, nst = a.K / BK, ks0 = a.k0 / BK, MB = a.M / 32;

  // ---- A: LDS-DMA pieces pc = (mbl 2 + ksl) NP + p (local 32-row block, 16-k step, part), pc = w + 8 i.
  // The packed image holds three parts per (block, step): a reduced form fetches the first NP of them and
  // packs them densely in LDS (gemm_nn_split_body's A side).
  const __amdgpu_buffer_rsrc_t ra = rsrc(a.ap);
  uint32_t va[2 * NP];
#pragma unroll
  for (int i = 0; i < 2 * NP; ++i) {
    const int pc = w + 8 * i;
    const int mbl = pc / (2 * NP), kp = 3 * ((pc / NP) & 1) + pc % NP;  // kp = 3 ksl + p
    const int mb = min(mt * (TM / 32) + mbl, MB - 1);  // blocks past M: any valid data, never stored
    va[i] = (uint32_t)((((int64_t)mb * KS * 3 + kp) * 64 + lane) * 16);
  }
  auto issue_a = [&](int s, int buf) {
#pragma unroll
    for (int i = 0; i < 2 * NP; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, lds + (buf * BUF + (w + 8 * i) * 1024) / 16, 16, va[i],
                                               (uint32_t)s * 6 * 1024, 0, 0);
  };

  // ---- B: thread t owns (pixel row t >> 2, 8-k chunk t & 3) of a stage: two 16-byte loads
  const int pc4 = threadIdx.x & 3, prow = threadIdx.x >> 2;
  int64_t row = nbase + prow;
  if (row > a.nrows - 1) row = a.nrows - 1;  // rows past the end: any valid data, never stored
  const int64_t node = row / a.P, pix = row - node * a.P;
  const float* bp0 = a.b0 + node * a.b0n + pix * a.b0p + 8 * pc4;
  const float* bp1 = a.b1 + node * a.b1n + pix * a.b1p + 8 * pc4;
  f4 breg[2];
  auto load_b = [&](int s) {
    const float* p = s < ks0 ? bp0 + BK * s : bp1 + BK * (s - ks0);
    breg[0] = *reinterpret_cast<const f4*>(p);
    breg[1] = *reinterpret_cast<const f4*>(p + 4);
  };
  const uint32_t bst = A_BYTES + rowoff(prow, pc4);
  auto store_b = [&](int buf) {  // split the registers' 8 k into the buffer's NP part images
    char* img = ldsb + buf * BUF + bst;
    const f2 x[4] = {{breg[0].x, breg[0].y}, {breg[0].z, breg[0].w}, {breg[1].x, breg[1].y}, {breg[1].z, breg[1].w}};
    u4 pp[NP];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint32_t e[NP];
      splitp<NP>(x[i], e);
#pragma unroll
      for (int p = 0; p < NP; ++p) pp[p][i] = e[p];
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) *reinterpret_cast<u4*>(img + p * BP) = pp[p];
  };

  // fragments: lane (r16, qq) holds k = 8 qq .. 8 qq + 7 of row r16 of a 16-row block.  A: 16-row block mi
  // of the wave is half (mi & 1) of 32-row block 2 wm + (mi >> 1); the packed image holds 16-k steps in the
  // 32 x 32 x 16 lane order, so the lane reads step qq >> 1, slot 16 (mi & 1) + r16 + 32 (qq & 1).  B: chunk
  // qq of pixel row 64 wn + 16 ni + r16 of the [row][32 k] images.
  const int r16 = lane & 15, qq = lane >> 4;
  const uint32_t abase0 = (uint32_t)reinterpret_cast<uintptr_t>(ldsb + (r16 + 32 * (qq & 1)) * 16 +
                                                                 ((4 * wm + (qq >> 1)) * NP) * 1024);
  uint32_t bro[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
    bro[ni] = (uint32_t)reinterpret_cast<uintptr_t>(ldsb + A_BYTES + rowoff(64 * wn + 16 * ni + r16, qq));
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
        load_b(s + 1);
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
  // Epilogue.  Register r of lane (r16, qq) of tile (mi, ni): channel 16 mi + 4 qq + r of pixel row
  // 16 ni + r16 — the lane's four registers are four consecutive channels of one pixel: one 16-byte store.
  // A 16-channel block lies on one side of m0 (m0 % 16 == 0) and within M (M % 16 == 0).
  const int mb0 = mt * TM + 64 * wm;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int64_t n = nbase + 64 * wn + 16 * ni + r16;
    if (n >= a.nrows) continue;
    const uint32_t nn = (uint32_t)n;  // the launch requires nrows < 2^31
    const uint32_t nd = nn / (uint32_t)a.P, px = nn - nd * (uint32_t)a.P;
    float* p0 = a.c0 + (int64_t)nd * a.c0n + (int64_t)px * a.c0p + 4 * qq;
    float* p1 = a.c1 + (int64_t)nd * a.c1n + (int64_t)px * a.c1p + 4 * qq;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int mrow = mb0 + 16 * mi;  // the block's first channel (wave-uniform)
      if (mrow >= a.M) continue;
      f4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = __fadd_rn(acc[mi][ni].hi[r], acc[mi][ni].lo[r]);
      if (a.bias != nullptr) {
        const float* bp = a.bias + mrow + 4 * qq;
        const f4 bv = {bp[0], bp[1], bp[2], bp[3]};
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = __fadd_rn(v[r], bv[r]);
      }
      float* dst = mrow >= a.m0 ? p1 + (mrow - a.m0) : p0 + mrow;
      *reinterpret_cast<f4*>(dst) = v;
    }
  }
}
};

template <int NP>
__global__ void __launch_bounds__(THREADS, 1) gemm_cl_split(Args a) {
  ClBody<NP>::run(a);
}

// ------------------------------------------------------------------------------------------------
// Weight gradient  dW[m][n] = sum_r gy[r][m] S[r][n],  db[m] = sum_r gy[r][m],  r = (node, pixel)
// ------------------------------------------------------------------------------------------------
struct WArgs {
  const float* g;  // gy: pixel rows of M channels
  int64_t gn, gp;
  const float* s0;  // columns [0, n0): x
  int64_t s0n, s0p;
  const float* s1;  // columns [n0, N): agg
  int64_t s1n, s1p;
  float* out;   // [split][M][N]
  float* outb;  // [split][M] or null
  int64_t ktot, kchunk;
  int32_t M, N, n0, P, mtiles, ntiles;
  int32_t group;
  int32_t ndb;  // the launch's first ndb workgroups form db (colsum_cl): splits x 64-channel blocks, or 0
};

template <int NP>
struct WgGeo {
  static constexpr int IMG = BK * TN * 2;  // one [32 k][128 columns] bf16 image: 8 KiB
  static constexpr int A_PART = 2 * IMG, B_PART = IMG;  // gy: 256 channels = two images per part
  static constexpr int BUF = NP * (A_PART + B_PART);    // NP 3: 72 KiB
  static constexpr int LDS_BYTES = 2 * BUF;              // NP 3: 144 KiB, 2: 96 KiB, 1: 48 KiB
  static constexpr int AJ = 4, BJ = 2;  // 16-byte pieces per thread per stage: piece (t & 15) + 16 j of row t >> 4
};

// db: workgroup b of the launch's first a.ndb forms outb[split][64 cblk ..] = the fp32 sum of gy over the
// split's pixel rows.  Thread t adds piece t & 15 (4 channels) of rows (t >> 4), (t >> 4) + 32, .. in order;
// the 32 row lanes are then summed in order through LDS: one fixed order, whatever the part count.  (In the
// GEMM workgroups these sums would be 16 more live registers per thread beside the 128 accumulators.)
__device__ __forceinline__ void colsum_cl(const WArgs& a, int b, float* ldsf) {
  const int cb = (a.M + 63) / 64;
  const int split = b / cb, cblk = b - split * cb;
  const int64_t kbeg = (int64_t)split * a.kchunk;
  const int64_t kend = kbeg + a.kchunk < a.ktot ? kbeg + a.kchunk : a.ktot;
  const int piece = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int chn = min(64 * cblk + 4 * piece, a.M - 4);  // pieces past M: the last piece, never stored
  int64_t r = kbeg + rl;
  int64_t ind = r / a.P;
  int ipx = (int)(r - ind * a.P);
  const int qs = BK / a.P, rs = BK - qs * a.P;
  f4 v = {0.f, 0.f, 0.f, 0.f};
  for (; r < kend; r += BK) {
    v += *reinterpret_cast<const f4*>(a.g + ind * a.gn + (int64_t)ipx * a.gp + chn);
    ind += qs;
    ipx += rs;
    if (ipx >= a.P) {
      ipx -= a.P;
      ++ind;
    }
  }
  *reinterpret_cast<f4*>(ldsf + rl * 64 + 4 * piece) = v;
  __syncthreads();
  const int m = 64 * cblk + (int)threadIdx.x;
  if (threadIdx.x < 64 && m < a.M) {
    float s = ldsf[threadIdx.x];
    for (int k = 1; k < BK; ++k) s += ldsf[k * 64 + threadIdx.x];
    a.outb[(int64_t)split * a.M + m] = s;
  }
}

template <int NP>
__global__ void __launch_bounds__(THREADS, 1) gemm_wg_cl_split(WArgs a) {
  using G = WgGeo<NP>;
  extern __shared__ u4 lds[];
  char* ldsb = reinterpret_cast<char*>(lds);
  if ((int)blockIdx.x < a.ndb) {  // workgroup-uniform
    colsum_cl(a, blockIdx.x, reinterpret_cast<float*>(lds));
    return;
  }
  const int id = xcd_remap(blockIdx.x - a.ndb, gridDim.x - a.ndb);
  const int tiles = a.mtiles * a.ntiles;
  const int split = id / tiles, tid = id - split * tiles;
  int mt, nt;
  tile_of(tid, a.mtiles, a.ntiles, a.group, mt, nt);
  const int mbase = mt * TM, nbase = nt * TN;
  const int64_t kbeg = (int64_t)split * a.kchunk;
  const int64_t kend = kbeg + a.kchunk < a.ktot ? kbeg + a.kchunk : a.ktot;
  const int nst = kend > kbeg ? (int)((kend - kbeg + BK - 1) / BK) : 0;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = w >> 1, wn = w & 1;

  // ---- loads: thread t -> pixel row (t >> 4) of the stage, 16-byte pieces (4 channels) c4 = (t & 15) + 16 j:
  // gy channels mbase + 4 c4 (j < 4), S channels nbase + 4 c4 (j < 2; n0 % 4 == 0: a piece lies on one side
  // of n0).  Pieces past M / N: any valid data (the last piece), never stored.
  const int ch = threadIdx.x & 15, kr = threadIdx.x >> 4;
  // the thread's row walks 32 pixel rows per stage: (node, pixel) advance by (32 / P, 32 % P) with one carry
  // (the launch requires ktot < 2^31)
  int r = (int)kbeg + kr;
  int ind = r / a.P;
  int ipx = r - ind * a.P;
  const int kendi = (int)kend;
  const int qs = BK / a.P, rs = BK - qs * a.P;
  f4 areg[G::AJ], breg[G::BJ];
  auto load = [&]() {
    const f4 z = {0.f, 0.f, 0.f, 0.f};  // rows past the split's end: zero terms
#pragma unroll
    for (int j = 0; j < G::AJ; ++j) areg[j] = z;
#pragma unroll
    for (int j = 0; j < G::BJ; ++j) breg[j] = z;
    if (r < kendi) {
      const float* gp = a.g + (int64_t)ind * a.gn + (int64_t)ipx * a.gp;
      const float* xp = a.s0 + (int64_t)ind * a.s0n + (int64_t)ipx * a.s0p;
      const float* ap = a.s1 + (int64_t)ind * a.s1n + (int64_t)ipx * a.s1p;
#pragma unroll
      for (int j = 0; j < G::AJ; ++j)
        areg[j] = *reinterpret_cast<const f4*>(gp + min(mbase + 4 * (ch + 16 * j), a.M - 4));
#pragma unroll
      for (int j = 0; j < G::BJ; ++j) {
        const int ncol = min(nbase + 4 * (ch + 16 * j), a.N - 4);
        breg[j] = *reinterpret_cast<const f4*>(ncol >= a.n0 ? ap + (ncol - a.n0) : xp + ncol);
      }
    }
    r += BK;
    ind += qs;
    ipx += rs;
    if (ipx >= a.P) {
      ipx -= a.P;
      ++ind;
    }
  };
  // LDS offsets.  boff(row, chunk) = 256 row + 16 (chunk ^ sw(row)) with sw(row) = ((row & 3) << 2) |
  // ((row >> 2) & 3) XORs bit fields, so every offset a thread needs is one base with a constant XORed into
  // bits 4..7 and a constant added above them: one register per operand instead of one per access.  The
  // bases take the buffer's offset (a multiple of 8 KiB) inside the loop.
  // Stores: piece c4 of row kr -> image c4 >> 5 (= j >> 1), chunk (ch >> 1) | 8 (j & 1), half ch & 1.
  const uint32_t st0 = boff(kr, ch >> 1) + 8 * (ch & 1);
  auto put = [&](uint32_t o, int part_bytes, const f4& v) {
    f2 lo, hi;
    lo.x = v.x, lo.y = v.y, hi.x = v.z, hi.y = v.w;
    uint32_t l[NP], h[NP];
    splitp<NP>(lo, l);
    splitp<NP>(hi, h);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      u2 u;
      u.x = l[p], u.y = h[p];
      *reinterpret_cast<u2*>(ldsb + o + p * part_bytes) = u;
    }
  };
  auto store = [&](uint32_t sbase) {
#pragma unroll
    for (int j = 0; j < G::AJ; ++j) put((sbase ^ (128u * (j & 1))) + (j >> 1) * G::IMG, G::A_PART, areg[j]);
#pragma unroll
    for (int j = 0; j < G::BJ; ++j) put((sbase ^ (128u * j)) + NP * G::A_PART, G::B_PART, breg[j]);
  };
  // Fragments: lane (r16, qq) holds k = 8 qq .. 8 qq + 7 of row (A) / column (B) r16 of a 16-wide block: the
  // transposing reads of stage rows 8 qq + 4 t + trq (t = 0, 1), where lane 4 trq + trp of a 16-lane group
  // reads columns 4 trp .. of the block (gemm_wg_cl_half's addresses): chunk 8 b + 2 i + (trp >> 1), half
  // trp & 1, for block i of the wave's 64 (b = wm & 1 of image wm >> 1 for gy, wn for S).  With row & 3 = trq
  // and (row >> 2) & 3 = 2 (qq & 1) + t the offset of read (i, t) is (base ^ (32 i + 16 t)) + 1024 t.
  const int r16 = lane & 15, qq = lane >> 4;
  const int trq = r16 >> 2, trp = r16 & 3;
  const uint32_t rowpart = (uint32_t)(256 * (8 * qq + trq) + 8 * (trp & 1));
  const uint32_t swz = (uint32_t)((trq << 2) ^ (2 * (qq & 1)) ^ (trp >> 1));
  const uint32_t a0 = (rowpart + (uint32_t)((wm >> 1) * G::IMG)) | (16u * (swz ^ (uint32_t)(8 * (wm & 1))));
  const uint32_t b0 = (rowpart + (uint32_t)(NP * G::A_PART)) | (16u * (swz ^ (uint32_t)(8 * wn)));
  auto frag = [&](uint32_t base, int i, int part_off) {
    s4 v[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
      v[t] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(reinterpret_cast<uintptr_t>(
          ldsb + ((base ^ (uint32_t)(32 * i + 16 * t)) + (uint32_t)(1024 * t + part_off)))));
    u4 u;
    u.x = __builtin_bit_cast(uint32_t, __builtin_shufflevector(v[0], v[0], 0, 1));
    u.y = __builtin_bit_cast(uint32_t, __builtin_shufflevector(v[0], v[0], 2, 3));
    u.z = __builtin_bit_cast(uint32_t, __builtin_shufflevector(v[1], v[1], 0, 1));
    u.w = __builtin_bit_cast(uint32_t, __builtin_shufflevector(v[1], v[1], 2, 3));
    return __builtin_bit_cast(bf8, u);
  };
  Acc2s acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[mi][ni].hi[q] = acc[mi][ni].lo[q] = 0.f;
  if (nst > 0) load();
#pragma unroll 1
  for (int s = 0; s < nst; ++s) {
    const uint32_t bo = (uint32_t)((s & 1) * G::BUF);
    uint32_t sbase = st0 + bo, abase = a0 + bo, bbase = b0 + bo;
    asm volatile("" : "+v"(sbase), "+v"(abase), "+v"(bbase));  // formed here, not once per (access, buffer)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    store(sbase);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // stage s visible to every wave; every wave is past stage s - 1's reads
    if (s + 1 < nst) load();
    bf8 bf[4][NP];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int p = 0; p < NP; ++p) bf[ni][p] = frag(bbase, ni, p * G::B_PART);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      bf8 af[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) af[p] = frag(abase, mi, p * G::A_PART);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) mma6_16<NP>(af, bf[ni], acc[mi][ni]);
    }
  }
  // register q of lane (r16, qq) of tile (mi, ni): row 16 mi + 4 qq + q, column 16 ni + r16
  float* out = a.out + (int64_t)split * a.M * a.N;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int n = nbase + 64 * wn + 16 * ni + r16;
    if (n >= a.N) continue;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = mbase + 64 * wm + 16 * mi + 4 * qq + q;
        if (m < a.M) out[(int64_t)m * a.N + n] = __fadd_rn(acc[mi][ni].hi[q], acc[mi][ni].lo[q]);
      }
  }
}

bool native_on() { return mrp_host::tuning().compress_split_cl != 0; }

// a pixel-major fp32 operand of C channels: non-null, 16-byte aligned, strides whole 16-byte pieces,
// pixel stride >= C, node stride >= P pixel strides
bool operand_ok(const void* p, int64_t ns, int64_t ps, int32_t C, int32_t P) {
  return p != nullptr && aligned16(p) && (ns & 3) == 0 && (ps & 3) == 0 && ps >= C && ns >= (int64_t)P * ps;
}

hipError_t launch(Args a, int parts, hipStream_t st) {
  // 32-bit offsets: the packed image (LDS-DMA) and the pixel-row index
  if ((int64_t)a.M * a.K * 6 >= kOffMax || a.nrows >= kOffMax) return hipErrorNotSupported;
  a.mtiles = (a.M + TM - 1) / TM;
  const int64_t grid = (int64_t)a.mtiles * ((a.nrows + TN - 1) / TN);
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  a.group = mrp_host::tuning().gemm_group;
  return dispatch_parts(parts, [&](auto np) {
    constexpr int NP = decltype(np)::value;
    return launch_lds<gemm_cl_split<NP>>(ClGeo<NP>::LDS_BYTES, dim3((unsigned)grid), dim3(THREADS), st, a);
  });
}

}  // namespace mrp_cscl

using namespace mrp_cscl;

extern "C" int mrp_compress_fwd_split_cl(const float* x, int64_t x_node_stride, int64_t x_pixel_stride,
                                         const float* agg, int64_t agg_node_stride, int64_t agg_pixel_stride,
                                         int32_t num_nodes, int32_t C, int32_t P, const void* packed_w,
                                         const float* bias, float* y, int64_t y_node_stride, int64_t y_pixel_stride,
                                         int32_t parts, void* stream) {
  if (parts < 1 || parts > 3) return hipErrorInvalidValue;
  if (num_nodes < 0 || C < 0 || P < 0) return hipErrorInvalidValue;
  if (num_nodes == 0 || C == 0 || P == 0) return hipSuccess;
  if (!operand_ok(x, x_node_stride, x_pixel_stride, C, P) || !operand_ok(agg, agg_node_stride, agg_pixel_stride, C, P) ||
      !operand_ok(y, y_node_stride, y_pixel_stride, C, P) || !packed_w || !aligned16(packed_w))
    return hipErrorInvalidValue;
  if (C % 32 != 0 || !native_on()) return hipErrorNotSupported;
  Args a = {};
  a.ap = static_cast<const u4*>(packed_w);
  a.b0 = x;
  a.b0n = x_node_stride;
  a.b0p = x_pixel_stride;
  a.b1 = agg;
  a.b1n = agg_node_stride;
  a.b1p = agg_pixel_stride;
  a.c0 = a.c1 = y;
  a.c0n = a.c1n = y_node_stride;
  a.c0p = a.c1p = y_pixel_stride;
  a.bias = bias;
  a.nrows = (int64_t)num_nodes * P;
  a.M = C;
  a.K = 2 * C;
  a.k0 = C;
  a.m0 = C;
  a.P = P;
  return launch(a, parts, static_cast<hipStream_t>(stream));
}

extern "C" int mrp_compress_bwd_data_split_cl(const float* gy, int64_t gy_node_stride, int64_t gy_pixel_stride,
                                              int32_t num_nodes, int32_t C, int32_t P, const void* packed_wt,
                                              float* gx, int64_t gx_node_stride, int64_t gx_pixel_stride, float* gagg,
                                              int64_t gagg_node_stride, int64_t gagg_pixel_stride, int32_t parts,
                                              void* stream) {
  if (parts < 1 || parts > 3) return hipErrorInvalidValue;
  if (num_nodes < 0 || C < 0 || P < 0) return hipErrorInvalidValue;
  if (num_nodes == 0 || C == 0 || P == 0) return hipSuccess;
  if (!operand_ok(gy, gy_node_stride, gy_pixel_stride, C, P) || !operand_ok(gx, gx_node_stride, gx_pixel_stride, C, P) ||
      !operand_ok(gagg, gagg_node_stride, gagg_pixel_stride, C, P) || !packed_wt || !aligned16(packed_wt))
    return hipErrorInvalidValue;
  if (C % 32 != 0 || !native_on()) return hipErrorNotSupported;
  Args a = {};
  a.ap = static_cast<const u4*>(packed_wt);
  a.b0 = a.b1 = gy;
  a.b0n = a.b1n = gy_node_stride;
  a.b0p = a.b1p = gy_pixel_stride;
  a.c0 = gx;
  a.c0n = gx_node_stride;
  a.c0p = gx_pixel_stride;
  a.c1 = gagg;
  a.c1n = gagg_node_stride;
  a.c1p = gagg_pixel_stride;
  a.bias = nullptr;
  a.nrows = (int64_t)num_nodes * P;
  a.M = 2 * C;
  a.K = C;
  a.k0 = C;
  a.m0 = C;
  a.P = P;
  return launch(a, parts, static_cast<hipStream_t>(stream));
}

extern "C" int64_t mrp_compress_bwd_weight_split_cl_workspace(int32_t num_nodes, int32_t C, int32_t P) {
  if (num_nodes <= 0 || C <= 0 || P <= 0 || C % 32 != 0) return 0;
  const int64_t M = C, N = 2 * (int64_t)C;
  int64_t kchunk;
  const int ns = mrp_ch::plan_splits(M, N, (int64_t)num_nodes * P, mrp_host::tuning().split_cl_splits, &kchunk);
  return splitk_place(ns, M, N).bytes;
}

extern "C" int mrp_compress_bwd_weight_split_cl(const float* gy, int64_t gy_node_stride, int64_t gy_pixel_stride,
                                                const float* x, int64_t x_node_stride, int64_t x_pixel_stride,
                                                const float* agg, int64_t agg_node_stride, int64_t agg_pixel_stride,
                                                int32_t num_nodes, int32_t C, int32_t P, float* gw, float* gbias,
                                                void* workspace, int64_t workspace_bytes, int32_t parts,
                                                void* stream) {
  if (parts < 1 || parts > 3) return hipErrorInvalidValue;
  if (num_nodes < 0 || C < 0 || P < 0) return hipErrorInvalidValue;
  if (C == 0 || (gw == nullptr && gbias == nullptr)) return hipSuccess;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t M = C, N = 2 * (int64_t)C;
  if (num_nodes == 0 || P == 0) {  // empty sum
    if (gw && hipMemsetAsync(gw, 0, M * N * 4, st) != hipSuccess) return hipErrorUnknown;
    if (gbias && hipMemsetAsync(gbias, 0, M * 4, st) != hipSuccess) return hipErrorUnknown;
    return hipSuccess;
  }
  if (!operand_ok(gy, gy_node_stride, gy_pixel_stride, C, P) || !operand_ok(x, x_node_stride, x_pixel_stride, C, P) ||
      !operand_ok(agg, agg_node_stride, agg_pixel_stride, C, P) || !gw || !aligned16(gw))
    return hipErrorInvalidValue;
  if (C % 32 != 0 || !native_on()) return hipErrorNotSupported;
  WArgs a = {};
  a.g = gy;
  a.gn = gy_node_stride;
  a.gp = gy_pixel_stride;
  a.s0 = x;
  a.s0n = x_node_stride;
  a.s0p = x_pixel_stride;
  a.s1 = agg;
  a.s1n = agg_node_stride;
  a.s1p = agg_pixel_stride;
  a.n0 = C;
  a.P = P;
  a.ktot = (int64_t)num_nodes * P;
  if (a.ktot >= kOffMax - 2 * BK) return hipErrorNotSupported;  // the kernel's row index is an int past kend
  a.M = (int32_t)M;
  a.N = (int32_t)N;
  a.mtiles = (int32_t)((M + TM - 1) / TM);
  a.ntiles = (int32_t)((N + TN - 1) / TN);
  const int ns = mrp_ch::plan_splits(M, N, a.ktot, mrp_host::tuning().split_cl_splits, &a.kchunk);
  const SplitK pl = splitk_place(ns, M, N, gw, gbias, workspace, workspace_bytes);
  if (pl.err != hipSuccess) return pl.err;
  a.out = pl.out;
  a.outb = pl.outb;
  a.ndb = pl.outb != nullptr ? ns * (int32_t)((M + 63) / 64) : 0;
  const int64_t grid = (int64_t)a.mtiles * a.ntiles * ns + a.ndb;
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  a.group = mrp_host::tuning().nt_group;
  const hipError_t e = dispatch_parts(parts, [&](auto np) {
    constexpr int NP = decltype(np)::value;
    return launch_lds<gemm_wg_cl_split<NP>>(WgGeo<NP>::LDS_BYTES, dim3((unsigned)grid), dim3(THREADS), st, a);
  });
  if (e != hipSuccess || ns <= 1) return e;
  return split_sum(pl.out, ns, M, N, gw, pl.outb, ns, gbias, st);
}
