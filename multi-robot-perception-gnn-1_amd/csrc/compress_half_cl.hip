// compress_half_cl.hip — compress_half.hip's three products on pixel-major (torch.channels_last) bf16 /
// fp16 feature maps, gfx950 (MI355X / CDNA4).
//
// A pixel-major tensor is (pointer, node stride, pixel stride) in elements: pixel row r = (node r / P,
// pixel r % P) is C contiguous channels at node * node_stride + pixel * pixel_stride — a dense
// channels_last map has pixel stride C, either half of a channels_last 2C concatenation buffer 2C.  Per
// pixel row r, T = bf16 or fp16, parameters fp32:
//     forward      y[r] = T( W_T [x[r]; a[r]] + b )           M = C,  K = 2C (k from x, then a)
//     data grad    [gx[r]; ga[r]] = T( W_T^T gy[r] )          M = 2C, K = C  (rows to gx, then ga)
//     weight grad  dW = sum_r gy[r] [x[r]; a[r]]^T, db = sum_r gy[r]     fp32, never rounded to T
// The arithmetic contract, the workgroup (8 waves, a 256 x 128 output tile as 4 x 2 waves of 64 x 64),
// the 32-k stages in two LDS buffers with one barrier per stage, the tile order and the packed weight
// images (mrp_compress_pack_t's, by LDS-DMA) are compress_half.hip's.  What differs is the activation side:
//
// Forward / data gradient (gemm_cl_half): the activation's k (channels) is contiguous, so a lane's MFMA
// fragment is one 16-byte piece of a pixel row as loaded; the stage is [128 pixel rows][32 k] in
// gemm_nt_half's rotated 64-byte LDS rows, one ds_read_b128 per fragment, no transposing read.  Pixels are
// rows: any P (a 7 x 7 plane needs no padding), a tile may cross node boundaries, rows past the end are
// loaded from the last row and never stored.  With the weight as the MFMA's row operand a lane's four
// accumulator registers are four consecutive channels of one pixel; the epilogue transposes the wave's four
// 16-channel blocks across the four lanes of a pixel and stores 2 x 16 bytes per lane and column tile.
//
// Weight gradient (gemm_wg_cl_half): k is the pixel row, both operands are k-strided with channels
// contiguous, so both are staged as [32 pixel rows][128 channels] row-major images with gemm_nn_half's
// XOR swizzle (gy: two of them, 256 channels) and both operands' fragments come back through
// ds_read_b64_tr_b16.  A stage may cross a node boundary (each thread walks its own row's (node, pixel));
// rows past the split's end are zero-filled.  K = nodes P is split over workgroups into fp32 partial tiles
// summed in a fixed order by split_sum (deterministic, no atomics); db from the gy pieces widened to
// fp32, per split, reduced over the stage's 32 rows through LDS in a fixed order.

#include "compress_half_common.hpp"
#include "mrp_gnn.h"
#include "tuning.hpp"

namespace mrp_ccl {

using namespace mrp_ch;

struct Args {
  const u4* ap;    // packed A
  const char* b0;  // k < k0: node / pixel strides in elements
  int64_t b0n, b0p;
  const char* b1;  // k >= k0
  int64_t b1n, b1p;
  char* c0;  // output channels [0, m0)
  int64_t c0n, c0p;
  char* c1;  // output channels [m0, M)
  int64_t c1n, c1p;
  const float* bias;  // (M) or null
  int64_t nrows;      // nodes * P
  int32_t M, K, k0, m0, P, mtiles;
  int32_t group;  // tile order (tile_of)
};

template <typename T>
__global__ void __launch_bounds__(THREADS) gemm_cl_half(Args a) {
  __shared__ u4 lds[LDS_BYTES / 16];
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

  // ---- A: the packed weight by LDS-DMA, its fragments by ds_read_b128 (compress_half_common.hpp)
  const WeightSide wa(a.ap, lds, mt, MB, KS, lane, w);

  // ---- B: thread t loads the 16-byte piece (pixel row t >> 2, k 8 (t & 3) ..) of a stage
  const int pc4 = threadIdx.x & 3, prow = threadIdx.x >> 2;
  int64_t row = nbase + prow;
  if (row > a.nrows - 1) row = a.nrows - 1;  // rows past the end: any valid data, never stored
  const int64_t node = row / a.P, pix = row - node * a.P;
  const char* bp0 = a.b0 + 2 * (node * a.b0n + pix * a.b0p + 8 * pc4);
  const char* bp1 = a.b1 + 2 * (node * a.b1n + pix * a.b1p + 8 * pc4);
  u4 breg;
  auto load_b = [&](int s) {
    const char* p = s < ks0 ? bp0 + 2 * BK * s : bp1 + 2 * BK * (s - ks0);
    breg = *reinterpret_cast<const u4*>(p);
  };
  const uint32_t bst = A_BYTES + rowoff(prow, pc4);

  // ---- B fragments: lane (r16, qq) of a 16 x 16 tile holds k = 8 qq .. 8 qq + 7: chunk qq of pixel row
  // 64 wn + 16 ni + r16
  const int r16 = lane & 15, qq = lane >> 4;
  uint32_t bro[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
    bro[ni] = (uint32_t)reinterpret_cast<uintptr_t>(ldsb + A_BYTES + rowoff(64 * wn + 16 * ni + r16, qq));
  f4 acc[4][4];
  zero_acc(acc);

  wa.issue(0, 0);
  load_b(0);
#pragma unroll 1
  for (int s = 0; s < nst; ++s) {
    const int buf = s & 1;
    // stage s's B registers and own A pieces landed; its buffer was last read in stage s - 2
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *reinterpret_cast<u4*>(ldsb + buf * BUF_BYTES + bst) = breg;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // stage s visible to every wave; every wave is past stage s - 1's reads
    // fragment reads by inline asm (a C++ LDS read beside the LDS-DMA issued below would make hipcc wait
    // for the DMA, which fills the other buffer)
    const uint32_t bo = (uint32_t)(buf * BUF_BYTES);
    u4 ar[4], bf[4];
    wa.read(bo, ar);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) asm volatile("ds_read_b128 %0, %1" : "=v"(bf[ni]) : "v"(bro[ni] + bo));
    if (s + 1 < nst) {
      wa.issue(s + 1, buf ^ 1);
      load_b(s + 1);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(ar[i]), "+v"(bf[i]));
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = T::mma(ar[mi], bf[ni], acc[mi][ni]);  // channels x pixels
  }

  // Epilogue.  Register r of lane (r16, qq) of tile (mi, ni): channel 16 mi + 4 qq + r, pixel row 16 ni + r16:
  // the lane's four registers of a tile are 4 consecutive channels (8 bytes after the conversion).  Per
  // column tile ni the wave's four 16-channel blocks are transposed across the four lanes of a pixel, so
  // that lane (r16, qq) holds channels 64 wm + 16 qq .. + 15 of its pixel row and writes them as two 16-byte
  // stores: the four lanes of a pixel write 128 contiguous bytes (0.82-0.93 x the time of one 8-byte
  // store per tile).  A 16-channel block lies on one side of m0 (m0 % 16 == 0) and within M
  // (M % 16 == 0).
  const int mb0 = mt * TM + 64 * wm;
  const int mg = mb0 + 16 * qq;  // the lane's 16 channels after the transpose
  const bool glive = mg < a.M, gside1 = mg >= a.m0;
  const int gs = gside1 ? mg - a.m0 : mg;
  f4 bv[4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int mrow = mb0 + 16 * mi;
    bv[mi] = f4{0.f, 0.f, 0.f, 0.f};
    if (a.bias != nullptr && mrow < a.M) {
      const float* bp = a.bias + mrow + 4 * qq;
      bv[mi] = f4{bp[0], bp[1], bp[2], bp[3]};
    }
  }
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int64_t n = nbase + 64 * wn + 16 * ni + r16;
    const bool live = n < a.nrows;
    const uint32_t nn = (uint32_t)(live ? n : 0);
    const uint32_t nd = nn / (uint32_t)a.P, px = nn - nd * (uint32_t)a.P;
    u2 piece[4], grp[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      f4 v = acc[mi][ni];
      if (a.bias != nullptr) v = v + bv[mi];
      piece[mi] = __builtin_bit_cast(u2, __builtin_convertvector(v, typename T::v4));
      grp[mi] = piece[mi];
    }
    // round s: lane qq sends its piece of block (qq - s) & 3 and takes, from lane (qq + s) & 3 of its pixel,
    // that lane's piece of block qq: channels 16 qq + 4 ((qq + s) & 3) ..  Every lane takes part (blocks
    // past M and rows past the end carry values that are never stored).
#pragma unroll
    for (int s = 1; s < 4; ++s) {
      const int si = (qq - s) & 3, dj = (qq + s) & 3;
      const u2 snd = si == 0 ? piece[0] : si == 1 ? piece[1] : si == 2 ? piece[2] : piece[3];
      const int src = r16 + 16 * dj;
      const u2 rcv = {(uint32_t)__shfl((int)snd.x, src, 64), (uint32_t)__shfl((int)snd.y, src, 64)};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (dj == j) grp[j] = rcv;
    }
    // the lane's own piece of block qq belongs at position qq
    const u2 own = qq == 0 ? piece[0] : qq == 1 ? piece[1] : qq == 2 ? piece[2] : piece[3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (qq == j) grp[j] = own;
    if (live && glive) {
      char* p = (gside1 ? a.c1 + 2 * ((int64_t)nd * a.c1n + (int64_t)px * a.c1p)
                        : a.c0 + 2 * ((int64_t)nd * a.c0n + (int64_t)px * a.c0p)) + 2 * gs;
      *reinterpret_cast<u4*>(p) = u4{grp[0].x, grp[0].y, grp[1].x, grp[1].y};
      *reinterpret_cast<u4*>(p + 16) = u4{grp[2].x, grp[2].y, grp[3].x, grp[3].y};
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Weight gradient  dW[m][n] = sum_r gy[r][m] S[r][n],  db[m] = sum_r gy[r][m],  r = (node, pixel)
// ------------------------------------------------------------------------------------------------
struct WArgs {
  const char* g;  // gy: pixel rows of M channels
  int64_t gn, gp;
  const char* s0;  // columns [0, n0): x
  int64_t s0n, s0p;
  const char* s1;  // columns [n0, N): agg
  int64_t s1n, s1p;
  float* out;   // [split][M][N]
  float* outb;  // [split][M] or null
  int64_t ktot, kchunk;
  int32_t M, N, n0, P, mtiles, ntiles;
  int32_t group;
};

template <typename T>
__global__ void __launch_bounds__(THREADS) gemm_wg_cl_half(WArgs a) {
  __shared__ u4 lds[LDS_BYTES / 16];
  char* ldsb = reinterpret_cast<char*>(lds);
  const int id = xcd_remap(blockIdx.x, gridDim.x);
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
  const bool dob = a.outb != nullptr && nt == 0;  // the column-tile-0 workgroups form the split's db

  // ---- loads: thread t -> pixel row (t >> 4) of the stage, 16-byte piece (t & 15) (8 channels) of each of
  // the three 128-channel images: gy channels mbase + 8 ch .., mbase + 128 + 8 ch .., S channel nbase + 8 ch ..
  // Pieces past M / N: any valid data (the last piece), never stored.
  const int ch = threadIdx.x & 15, kr = threadIdx.x >> 4;
  const int64_t ao0 = 2 * (int64_t)min(mbase + 8 * ch, a.M - 8), ao1 = 2 * (int64_t)min(mbase + 128 + 8 * ch, a.M - 8);
  const int ncol = min(nbase + 8 * ch, a.N - 8);
  const bool bhi = ncol >= a.n0;
  const char* sb = (bhi ? a.s1 : a.s0) + 2 * (bhi ? ncol - a.n0 : ncol);
  const int64_t sn = bhi ? a.s1n : a.s0n, sp = bhi ? a.s1p : a.s0p;
  // the thread's row walks 32 pixel rows per stage: (node, pixel) advance by (32 / P, 32 % P) with one carry
  int64_t r = kbeg + kr;
  int64_t ind = r / a.P;
  int ipx = (int)(r - ind * a.P);
  const int qs = BK / a.P, rs = BK - qs * a.P;
  u4 areg0, areg1, breg;
  auto load = [&]() {
    areg0 = areg1 = breg = u4{0u, 0u, 0u, 0u};  // rows past the split's end: zero terms
    if (r < kend) {
      const char* gp = a.g + 2 * (ind * a.gn + (int64_t)ipx * a.gp);
      areg0 = *reinterpret_cast<const u4*>(gp + ao0);
      areg1 = *reinterpret_cast<const u4*>(gp + ao1);
      breg = *reinterpret_cast<const u4*>(sb + 2 * (ind * sn + (int64_t)ipx * sp));
    }
    r += BK;
    ind += qs;
    ipx += rs;
    if (ipx >= a.P) {
      ipx -= a.P;
      ++ind;
    }
  };
  f8 bs0 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, bs1 = bs0;
  const uint32_t st = boff(kr, ch);
  auto store = [&](int buf) {
    char* base = ldsb + buf * BUF_BYTES;
    if (dob) {
      bs0 += __builtin_convertvector(__builtin_bit_cast(typename T::v8, areg0), f8);
      bs1 += __builtin_convertvector(__builtin_bit_cast(typename T::v8, areg1), f8);
    }
    *reinterpret_cast<u4*>(base + st) = areg0;
    *reinterpret_cast<u4*>(base + B_BYTES + st) = areg1;
    *reinterpret_cast<u4*>(base + A_BYTES + st) = breg;
  };

  // ---- fragments: lane (r16, qq) holds k = 8 qq .. 8 qq + 7 of row (A) / column (B) r16 of a 16-wide block:
  // the transposing reads of stage rows 8 qq + 4 t .. + 3 (t = 0, 1), channels 16 i .. of the wave's 64
  const int r16 = lane & 15, qq = lane >> 4;
  const int trq = r16 >> 2, trp = r16 & 3;
  uint32_t atr[4][2], btr[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int krow = 8 * qq + 4 * t + trq;
      atr[i][t] = (uint32_t)reinterpret_cast<uintptr_t>(
          ldsb + (wm >> 1) * B_BYTES + boff(krow, (64 * (wm & 1) + 16 * i) / 8 + (trp >> 1)) + 8 * (trp & 1));
      btr[i][t] = (uint32_t)reinterpret_cast<uintptr_t>(
          ldsb + A_BYTES + boff(krow, (64 * wn + 16 * i) / 8 + (trp >> 1)) + 8 * (trp & 1));
    }
  f4 acc[4][4];
  zero_acc(acc);
  if (nst > 0) load();
#pragma unroll 1
  for (int s = 0; s < nst; ++s) {
    const int buf = s & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    store(buf);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const uint32_t bo = (uint32_t)(buf * BUF_BYTES);
    s4 av[4][2], bv[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int t = 0; t < 2; ++t) asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(av[i][t]) : "v"(atr[i][t] + bo));
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int t = 0; t < 2; ++t) asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(bv[i][t]) : "v"(btr[i][t] + bo));
    if (s + 1 < nst) load();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    u4 ar[4], br[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      asm volatile("" : "+v"(av[i][0]), "+v"(av[i][1]), "+v"(bv[i][0]), "+v"(bv[i][1]));
      ar[i] = join_tr(av[i][0], av[i][1]);
      br[i] = join_tr(bv[i][0], bv[i][1]);
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = T::mma(ar[mi], br[ni], acc[mi][ni]);
  }
  store_partial(acc, a.out + (int64_t)split * a.M * a.N, a.M, a.N, mbase + 64 * wm, nbase + 64 * wn, r16, qq);
  if (dob) {  // workgroup-uniform.  [32 stage rows][256 channels] fp32 in LDS, summed over the rows in order
    float* ldsf = reinterpret_cast<float*>(lds);
    __syncthreads();  // every wave is past its last fragment reads
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ldsf[kr * TM + 8 * ch + j] = bs0[j];
      ldsf[kr * TM + 128 + 8 * ch + j] = bs1[j];
    }
    __syncthreads();
    const int m = mbase + (int)threadIdx.x;
    if (threadIdx.x < TM && m < a.M) {
      float v = ldsf[threadIdx.x];
      for (int k = 1; k < BK; ++k) v += ldsf[k * TM + threadIdx.x];
      a.outb[(int64_t)split * a.M + m] = v;
    }
  }
}

bool native_on() { return mrp_host::tuning().compress_half_cl != 0; }

// a pixel-major operand of C channels: non-null, 16-byte aligned, strides whole 16-byte pieces,
// pixel stride >= C, node stride >= P pixel strides
bool operand_ok(const void* p, int64_t ns, int64_t ps, int32_t C, int32_t P) {
  return p != nullptr && aligned16(p) && (ns & 7) == 0 && (ps & 7) == 0 && ps >= C && ns >= (int64_t)P * ps;
}

hipError_t launch(int32_t dtype, Args a, hipStream_t st) {
  // 32-bit offsets: the packed image (LDS-DMA) and the pixel-row index
  if ((int64_t)a.M * a.K * 2 >= kOffMax || a.nrows >= kOffMax) return hipErrorNotSupported;
  a.mtiles = (a.M + TM - 1) / TM;
  const int64_t grid = (int64_t)a.mtiles * ((a.nrows + TN - 1) / TN);
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  a.group = mrp_host::tuning().gemm_group;
  return launch_t(dtype, gemm_cl_half<BF16>, gemm_cl_half<F16>, dim3((unsigned)grid), dim3(THREADS), st, a);
}

}  // namespace mrp_ccl

using namespace mrp_ccl;

extern "C" int mrp_compress_fwd_cl(int32_t dtype, const void* x, int64_t x_node_stride, int64_t x_pixel_stride,
                                   const void* agg, int64_t agg_node_stride, int64_t agg_pixel_stride,
                                   int32_t num_nodes, int32_t C, int32_t P, const void* packed_w, const float* bias,
                                   void* y, int64_t y_node_stride, int64_t y_pixel_stride, void* stream) {
  if (!is_half(dtype) || num_nodes < 0 || C < 0 || P < 0) return hipErrorInvalidValue;
  if (num_nodes == 0 || C == 0 || P == 0) return hipSuccess;
  if (!operand_ok(x, x_node_stride, x_pixel_stride, C, P) || !operand_ok(agg, agg_node_stride, agg_pixel_stride, C, P) ||
      !operand_ok(y, y_node_stride, y_pixel_stride, C, P) || !packed_w || !aligned16(packed_w))
    return hipErrorInvalidValue;
  if (C % 32 != 0 || !native_on()) return hipErrorNotSupported;
  Args a = {};
  a.ap = static_cast<const u4*>(packed_w);
  a.b0 = static_cast<const char*>(x);
  a.b0n = x_node_stride;
  a.b0p = x_pixel_stride;
  a.b1 = static_cast<const char*>(agg);
  a.b1n = agg_node_stride;
  a.b1p = agg_pixel_stride;
  a.c0 = a.c1 = static_cast<char*>(y);
  a.c0n = a.c1n = y_node_stride;
  a.c0p = a.c1p = y_pixel_stride;
  a.bias = bias;
  a.nrows = (int64_t)num_nodes * P;
  a.M = C;
  a.K = 2 * C;
  a.k0 = C;
  a.m0 = C;
  a.P = P;
  return launch(dtype, a, static_cast<hipStream_t>(stream));
}

extern "C" int mrp_compress_bwd_data_cl(int32_t dtype, const void* gy, int64_t gy_node_stride, int64_t gy_pixel_stride,
                                        int32_t num_nodes, int32_t C, int32_t P, const void* packed_wt, void* gx,
                                        int64_t gx_node_stride, int64_t gx_pixel_stride, void* gagg,
                                        int64_t gagg_node_stride, int64_t gagg_pixel_stride, void* stream) {
  if (!is_half(dtype) || num_nodes < 0 || C < 0 || P < 0) return hipErrorInvalidValue;
  if (num_nodes == 0 || C == 0 || P == 0) return hipSuccess;
  if (!operand_ok(gy, gy_node_stride, gy_pixel_stride, C, P) || !operand_ok(gx, gx_node_stride, gx_pixel_stride, C, P) ||
      !operand_ok(gagg, gagg_node_stride, gagg_pixel_stride, C, P) || !packed_wt || !aligned16(packed_wt))
    return hipErrorInvalidValue;
  if (C % 32 != 0 || !native_on()) return hipErrorNotSupported;
  Args a = {};
  a.ap = static_cast<const u4*>(packed_wt);
  a.b0 = a.b1 = static_cast<const char*>(gy);
  a.b0n = a.b1n = gy_node_stride;
  a.b0p = a.b1p = gy_pixel_stride;
  a.c0 = static_cast<char*>(gx);
  a.c0n = gx_node_stride;
  a.c0p = gx_pixel_stride;
  a.c1 = static_cast<char*>(gagg);
  a.c1n = gagg_node_stride;
  a.c1p = gagg_pixel_stride;
  a.bias = nullptr;
  a.nrows = (int64_t)num_nodes * P;
  a.M = 2 * C;
  a.K = C;
  a.k0 = C;
  a.m0 = C;
  a.P = P;
  return launch(dtype, a, static_cast<hipStream_t>(stream));
}

extern "C" int64_t mrp_compress_bwd_weight_cl_workspace(int32_t num_nodes, int32_t C, int32_t P) {
  if (num_nodes <= 0 || C <= 0 || P <= 0 || C % 32 != 0) return 0;
  const int64_t M = C, N = 2 * (int64_t)C;
  int64_t kchunk;
  const int ns = plan_splits(M, N, (int64_t)num_nodes * P, mrp_host::tuning().half_cl_splits, &kchunk);
  return splitk_place(ns, M, N).bytes;
}

extern "C" int mrp_compress_bwd_weight_cl(int32_t dtype, const void* gy, int64_t gy_node_stride,
                                          int64_t gy_pixel_stride, const void* x, int64_t x_node_stride,
                                          int64_t x_pixel_stride, const void* agg, int64_t agg_node_stride,
                                          int64_t agg_pixel_stride, int32_t num_nodes, int32_t C, int32_t P, float* gw,
                                          float* gbias, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!is_half(dtype) || num_nodes < 0 || C < 0 || P < 0) return hipErrorInvalidValue;
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
  a.g = static_cast<const char*>(gy);
  a.gn = gy_node_stride;
  a.gp = gy_pixel_stride;
  a.s0 = static_cast<const char*>(x);
  a.s0n = x_node_stride;
  a.s0p = x_pixel_stride;
  a.s1 = static_cast<const char*>(agg);
  a.s1n = agg_node_stride;
  a.s1p = agg_pixel_stride;
  a.n0 = C;
  a.P = P;
  a.ktot = (int64_t)num_nodes * P;
  return run_wgrad(dtype, gemm_wg_cl_half<BF16>, gemm_wg_cl_half<F16>, a, mrp_host::tuning().half_cl_splits, M, N, gw,
                   gbias, workspace, workspace_bytes, st);
}
