// compress_half.hip — the GCN layer's 1x1 compress convolution, its data gradient and its weight
// gradient on bf16 / fp16 feature maps, gfx950 (MI355X / CDNA4).
//
// Reference (xjh19971/multi-robot-perception-gnn-1, dgl/model/models.py:163-165,181-184,186-189):
//     h = self.conv1(torch.cat((h, g_h), dim=1))       # nn.Conv2d(2C, C, kernel_size=1)
// under torch.autocast the features are T = bf16 or fp16 and the parameters fp32.  Per node n, P = H W:
//     forward      y[n] = T( W_T [x[n]; a[n]] + b )           M = C,  K = 2C (rows from x, then a)
//     data grad    [gx[n]; ga[n]] = T( W_T^T gy[n] )          M = 2C, K = C  (rows to gx, then ga)
//     weight grad  dW = sum_n gy[n] [x[n]; a[n]]^T, db = sum gy   fp32, never rounded to T
// W_T is the fp32 weight rounded once to T (round to nearest even) when it is packed; products of two T
// values are exact in fp32, the sums are the MFMA's fp32 accumulator, the fp32 bias is added to the fp32
// sum, and the one rounding is the store's.
//
// These are compress_split.hip's kernels (gemm_nn_split_body<4, true> and gemm_nt_split_body<4>) with the
// three-way split removed: one v_mfma_f32_16x16x32_{bf16,f16} per product instead of six, one operand
// image instead of three, one accumulator set instead of hi + lo, half the bytes.  Same workgroup (8
// waves, a 256 x 128 output tile as 4 x 2 waves of 64 x 64), same 32-k stages in two LDS buffers with one
// barrier per stage, same XCD-aware tile_of order (gemm_common.hpp, with the image offsets boff and
// rowoff), same packed-weight layout (`pack`'s, 2 bytes per element, one part) arriving by LDS-DMA, same
// XOR-swizzled row-major activation image read back with ds_read_b64_tr_b16 (NN) and the same rotated
// [row][32 k] images read with ds_read_b128 (NT).
//
// NN epilogue: the MFMA's operand roles are the fp32 kernel's (weight rows x activation columns), so a
// lane's four accumulator registers are four channels of one pixel and each is one 2-byte
// buffer_store_short after the conversion to T.  The swapped form (activations as the MFMA's rows: four
// consecutive pixels per lane, one 8-byte store per tile, a quarter of the store instructions) was built
// and measured 2-8 % slower at every config shape (tools/lab_patches/half_nn_swapped.py).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compress_half_common.hpp"
#include "mrp_gnn.h"
#include "tuning.hpp"

namespace mrp_ch {  // types, tile sizes, the weight side, LDS layouts and the tile order: compress_half_common.hpp

// A (M x K) = w (row-major, stride lda) or w^T (w: K x M row-major, stride lda), rounded to T, in
// compress_split.hip's `pack` layout with one part: 16-byte unit (mb KS + ks) 64 + lane holds lane
// (r, h)'s eight k = 16 ks + 8 h + j of row 32 mb + r.
template <typename T>
__global__ void __launch_bounds__(256) pack_t(const float* __restrict__ w, int64_t lda, int trans, int M, int K,
                                              u4* __restrict__ out) {
  const int KS = K / 16;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)(M / 32) * KS * 64) return;
  const int lane = (int)(t & 63);
  const int64_t g = t >> 6;  // mb * KS + ks
  const int ks = (int)(g % KS), mb = (int)(g / KS);
  const int m = 32 * mb + (lane & 31), k0 = 16 * ks + 8 * (lane >> 5);
  typename T::v8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    v[j] = (typename T::elem)(trans ? w[(int64_t)(k0 + j) * lda + m] : w[(int64_t)m * lda + k0 + j]);
  out[t] = __builtin_bit_cast(u4, v);
}

struct Args {
  const u4* ap;  // packed A
  const char* b0;
  int64_t b0s;  // node strides in elements
  const char* b1;
  int64_t b1s;
  void* c0;
  int64_t c0s;
  void* c1;
  int64_t c1s;
  const float* bias;  // (M) or null
  int64_t ncols;      // nodes * P
  int32_t M, K, k0, m0, P, mtiles;
  int32_t group;  // tile order (tile_of)
};

template <typename T>
__global__ void __launch_bounds__(THREADS) gemm_nn_half(Args a) {
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

  // ---- B: thread t loads the 16-byte piece (row t >> 4, columns 8 (t & 15) ..) of a stage
  const int fc = threadIdx.x & 15, kr = threadIdx.x >> 4;
  int64_t col = nbase + 8 * fc;
  if (col > a.ncols - 8) col = a.ncols - 8;  // columns past the end: any valid data, never stored
  const int64_t node = col / a.P, pix = col - node * a.P;
  const char* bp0 = a.b0 + 2 * (node * a.b0s + pix + (int64_t)kr * a.P);
  const char* bp1 = a.b1 + 2 * (node * a.b1s + pix + (int64_t)kr * a.P);
  u4 breg;
  auto load_b = [&](int s) {
    const char* p = s < ks0 ? bp0 + 2 * ((int64_t)s * BK * a.P) : bp1 + 2 * ((int64_t)(s - ks0) * BK * a.P);
    breg = *reinterpret_cast<const u4*>(p);
  };
  const uint32_t bst = A_BYTES + boff(kr, fc);

  // ---- B fragments: lane (r16, qq) of a 16 x 16 tile holds k = 8 qq .. 8 qq + 7: the transposing reads of
  // rows 8 qq + 4 t .. + 3 (t = 0, 1), columns 64 wn + 16 ni ...
  const int r16 = lane & 15, qq = lane >> 4;
  const int trq = r16 >> 2, trp = r16 & 3;
  uint32_t tr16[4][2];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
#pragma unroll
    for (int t = 0; t < 2; ++t)
      tr16[ni][t] = (uint32_t)reinterpret_cast<uintptr_t>(
          ldsb + A_BYTES + boff(8 * qq + 4 * t + trq, (64 * wn + 16 * ni) / 8 + (trp >> 1)) + 8 * (trp & 1));
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
    u4 ar[4];
    s4 v[4][2];
    wa.read(bo, ar);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int t = 0; t < 2; ++t)
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v[ni][t]) : "v"(tr16[ni][t] + bo));
    if (s + 1 < nst) {
      wa.issue(s + 1, buf ^ 1);
      load_b(s + 1);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    u4 bf[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      asm volatile("" : "+v"(v[ni][0]), "+v"(v[ni][1]));
      bf[ni] = join_tr(v[ni][0], v[ni][1]);
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      asm volatile("" : "+v"(ar[mi]));
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = T::mma(ar[mi], bf[ni], acc[mi][ni]);  // channels x pixels
    }
  }

  // Epilogue.  Register r of lane (r16, qq) of tile (mi, ni): pixel column 16 ni + 4 qq + r, channel row
  // 16 mi + r16.  One buffer_store_dwordx2 per tile: the lane's byte offset (node, pixel, r16 rows) is fixed
  // per ni, the 16-row block's first row a scalar offset; a block lies on one side of m0 (m0 % 16 == 0) and
  // within M (M % 16 == 0).  Columns past the end get an offset past the buffer's 2^31 - 1 bytes (dropped).
  const int mb0 = mt * TM + 64 * wm;
  uint32_t vo0[4], vo1[4];  // per ni: byte offset of (node, pixel, row 4 qq) in c0 / c1
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int64_t n = nbase + 64 * wn + 16 * ni + r16;
    const bool live = n < a.ncols;
    const uint32_t nn = (uint32_t)(live ? n : 0);
    const uint32_t nd = nn / (uint32_t)a.P, px = nn - nd * (uint32_t)a.P;
    vo0[ni] = live ? 2u * ((uint32_t)((int64_t)nd * a.c0s) + px + (uint32_t)(4 * qq * a.P)) : 0x80000000u;
    vo1[ni] = live ? 2u * ((uint32_t)((int64_t)nd * a.c1s) + px + (uint32_t)(4 * qq * a.P)) : 0x80000000u;
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int mrow = mb0 + 16 * mi;
    if (mrow >= a.M) continue;
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
      const uint32_t so = 2u * (srow + (uint32_t)r) * (uint32_t)a.P;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        float v = acc[mi][ni][r];
        if (a.bias != nullptr) v = v + bv[r];
        const typename T::elem e = (typename T::elem)v;
        __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, e), rc, side1 ? vo1[ni] : vo0[ni], so, 0);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Weight gradient  dW[m][n] = sum_k dy[m][k] S[n][k],  db[m] = sum_k dy[m][k],  k = (node, pixel): both
// operands are k-contiguous rows of T (a channel's P pixels of one node), so eight consecutive k are
// one lane's fragment as loaded — 16-byte row pieces go through registers into [row][32 k] 64-byte LDS
// rows (chunks rotated by the row) and come back with one ds_read_b128 per fragment.  K = Nt P is split
// over workgroups (whole stages, each within one node: P % 32 == 0) into fp32 partial tiles summed in
// a fixed order by split_sum (deterministic); db from the dy pieces widened to fp32, per split.
// ------------------------------------------------------------------------------------------------
struct NTArgs {
  const char* g;  // dy (nodes, M, P), node stride gs (elements)
  int64_t gs;
  const char* s0;  // rows [0, n0) of B: x (nodes, n0, P)
  int64_t s0s;
  const char* s1;  // rows [n0, N): agg
  int64_t s1s;
  float* out;   // [split][M][N]
  float* outb;  // [split][M] or null
  int64_t ktot, kchunk;
  int32_t M, N, n0, P, mtiles, ntiles;
  int32_t group;
};

template <typename T>
__global__ void __launch_bounds__(THREADS) gemm_nt_half(NTArgs a) {
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
  const int nst = kend > kbeg ? (int)((kend - kbeg) / BK) : 0;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = w >> 1, wn = w & 1;

  // ---- loads: thread t -> piece (t & 3) (8 pixels) of A rows (t >> 2) + 128 j and of B row (t >> 2)
  const int pc8 = threadIdx.x & 3, r0 = threadIdx.x >> 2;
  int64_t aoff[2], boffs;
#pragma unroll
  for (int j = 0; j < 2; ++j) aoff[j] = 2 * ((int64_t)min(mbase + r0 + 128 * j, a.M - 1) * a.P + 8 * pc8);
  const int nrow = min(nbase + r0, a.N - 1);
  const bool bhi = nrow >= a.n0;
  boffs = 2 * ((int64_t)(bhi ? nrow - a.n0 : nrow) * a.P + 8 * pc8);
  u4 areg[2], breg;
  float rsum[2] = {0.f, 0.f};
  int64_t ind = kbeg / a.P;
  int ipx = (int)(kbeg - ind * a.P);
  auto load = [&]() {
    const char* gp = a.g + 2 * (ind * a.gs + ipx);
    const char* sp = bhi ? a.s1 + 2 * (ind * a.s1s + ipx) : a.s0 + 2 * (ind * a.s0s + ipx);
#pragma unroll
    for (int j = 0; j < 2; ++j) areg[j] = *reinterpret_cast<const u4*>(gp + aoff[j]);
    breg = *reinterpret_cast<const u4*>(sp + boffs);
    ipx += BK;
    if (ipx == a.P) {
      ipx = 0;
      ++ind;
    }
  };
  auto store = [&](int buf) {
    char* base = ldsb + buf * BUF_BYTES;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const f8 f = __builtin_convertvector(__builtin_bit_cast(typename T::v8, areg[j]), f8);
      rsum[j] += ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]));
      *reinterpret_cast<u4*>(base + rowoff(r0 + 128 * j, pc8)) = areg[j];
    }
    *reinterpret_cast<u4*>(base + A_BYTES + rowoff(r0, pc8)) = breg;
  };
  // lane (r16, qq) reads k = 8 qq .. 8 qq + 7 (chunk qq) of row r16 of a 16-row block
  const int r16 = lane & 15, qq = lane >> 4;
  uint32_t aro[4], bro[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    aro[i] = (uint32_t)reinterpret_cast<uintptr_t>(ldsb + rowoff(64 * wm + 16 * i + r16, qq));
    bro[i] = (uint32_t)reinterpret_cast<uintptr_t>(ldsb + A_BYTES + rowoff(64 * wn + 16 * i + r16, qq));
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
    u4 ar[4], br[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("ds_read_b128 %0, %1" : "=v"(ar[i]) : "v"(aro[i] + bo));
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("ds_read_b128 %0, %1" : "=v"(br[i]) : "v"(bro[i] + bo));
    if (s + 1 < nst) load();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(ar[i]), "+v"(br[i]));
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = T::mma(ar[mi], br[ni], acc[mi][ni]);
  }
  store_partial(acc, a.out + (int64_t)split * a.M * a.N, a.M, a.N, mbase + 64 * wm, nbase + 64 * wn, r16, qq);
  if (a.outb != nullptr && nt == 0) {  // the column-tile-0 workgroups write the split's row sums
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float v = rsum[j];  // the 4 threads of a row are 4 consecutive lanes (t & 3)
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      const int m = mbase + r0 + 128 * j;
      if (pc8 == 0 && m < a.M) a.outb[(int64_t)split * a.M + m] = v;
    }
  }
}

bool native_on() { return mrp_host::tuning().compress_half != 0; }

hipError_t launch_nn(int32_t dtype, Args a, hipStream_t st) {
  // 32-bit buffer offsets: the packed image, every output's node range and the column index
  if ((int64_t)a.M * a.K * 2 >= kOffMax || a.ncols >= kOffMax) return hipErrorNotSupported;
  const int64_t nodes = a.ncols / a.P;
  const int64_t r0 = a.m0 < a.M ? a.m0 : a.M, r1 = a.M - r0;
  if (((nodes - 1) * a.c0s + r0 * a.P) * 2 >= kOffMax || (r1 > 0 && ((nodes - 1) * a.c1s + r1 * a.P) * 2 >= kOffMax))
    return hipErrorNotSupported;
  a.mtiles = (a.M + TM - 1) / TM;
  const int64_t grid = (int64_t)a.mtiles * ((a.ncols + TN - 1) / TN);
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  a.group = mrp_host::tuning().gemm_group;
  return launch_t(dtype, gemm_nn_half<BF16>, gemm_nn_half<F16>, dim3((unsigned)grid), dim3(THREADS), st, a);
}

}  // namespace mrp_ch

using namespace mrp_ch;

extern "C" int64_t mrp_compress_pack_t_bytes(int32_t M, int32_t K) {
  if (M <= 0 || K <= 0 || M % 32 != 0 || K % 32 != 0) return 0;
  return (int64_t)M * K * 2;
}

extern "C" int mrp_compress_pack_t(int32_t dtype, const float* w, int64_t ld, int32_t transpose, int32_t M, int32_t K,
                                   void* packed, void* stream) {
  if (!is_half(dtype) || M < 0 || K < 0) return hipErrorInvalidValue;
  if (M == 0 || K == 0) return hipSuccess;
  if (!w || !packed || !aligned16(packed) || ld < (transpose ? M : K)) return hipErrorInvalidValue;
  if (M % 32 != 0 || K % 32 != 0) return hipErrorNotSupported;
  const int64_t threads = (int64_t)(M / 32) * (K / 16) * 64;
  return launch_t(dtype, pack_t<BF16>, pack_t<F16>, dim3((unsigned)((threads + 255) / 256)), dim3(256),
                  static_cast<hipStream_t>(stream), w, ld, transpose ? 1 : 0, M, K, static_cast<u4*>(packed));
}

extern "C" int mrp_compress_fwd_t(int32_t dtype, const void* x, int64_t x_node_stride, const void* agg,
                                  int64_t agg_node_stride, int32_t num_nodes, int32_t C, int32_t P,
                                  const void* packed_w, const float* bias, void* y, int64_t y_node_stride,
                                  void* stream) {
  if (!is_half(dtype) || num_nodes < 0 || C < 0 || P < 0) return hipErrorInvalidValue;
  if (num_nodes == 0 || C == 0 || P == 0) return hipSuccess;
  const int64_t plane = (int64_t)C * P;
  if (!x || !agg || !packed_w || !y || x_node_stride < plane || agg_node_stride < plane || y_node_stride < plane)
    return hipErrorInvalidValue;
  if (!aligned16(x) || !aligned16(agg) || !aligned16(packed_w) || !aligned16(y) || (x_node_stride & 7) ||
      (agg_node_stride & 7) || (y_node_stride & 7))
    return hipErrorInvalidValue;
  if (C % 32 != 0 || P % 8 != 0 || !native_on()) return hipErrorNotSupported;
  Args a = {};
  a.ap = static_cast<const u4*>(packed_w);
  a.b0 = static_cast<const char*>(x);
  a.b0s = x_node_stride;
  a.b1 = static_cast<const char*>(agg);
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
  return launch_nn(dtype, a, static_cast<hipStream_t>(stream));
}

extern "C" int mrp_compress_bwd_data_t(int32_t dtype, const void* gy, int64_t gy_node_stride, int32_t num_nodes,
                                       int32_t C, int32_t P, const void* packed_wt, void* gx, int64_t gx_node_stride,
                                       void* gagg, int64_t gagg_node_stride, void* stream) {
  if (!is_half(dtype) || num_nodes < 0 || C < 0 || P < 0) return hipErrorInvalidValue;
  if (num_nodes == 0 || C == 0 || P == 0) return hipSuccess;
  const int64_t plane = (int64_t)C * P;
  if (!gy || !packed_wt || !gx || !gagg || gy_node_stride < plane || gx_node_stride < plane ||
      gagg_node_stride < plane)
    return hipErrorInvalidValue;
  if (!aligned16(gy) || !aligned16(packed_wt) || !aligned16(gx) || !aligned16(gagg) || (gy_node_stride & 7) ||
      (gx_node_stride & 7) || (gagg_node_stride & 7))
    return hipErrorInvalidValue;
  if (C % 32 != 0 || P % 8 != 0 || !native_on()) return hipErrorNotSupported;
  Args a = {};
  a.ap = static_cast<const u4*>(packed_wt);
  a.b0 = static_cast<const char*>(gy);
  a.b0s = gy_node_stride;
  a.b1 = a.b0;
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
  return launch_nn(dtype, a, static_cast<hipStream_t>(stream));
}

extern "C" int64_t mrp_compress_bwd_weight_t_workspace(int32_t num_nodes, int32_t C, int32_t P) {
  if (num_nodes <= 0 || C <= 0 || P <= 0 || C % 32 != 0 || P % BK != 0) return 0;
  const int64_t M = C, N = 2 * (int64_t)C;
  int64_t kchunk;
  const int ns = plan_splits(M, N, (int64_t)num_nodes * P, mrp_host::tuning().half_nt_splits, &kchunk);
  return splitk_place(ns, M, N).bytes;
}

extern "C" int mrp_compress_bwd_weight_t(int32_t dtype, const void* gy, int64_t gy_node_stride, const void* x,
                                         int64_t x_node_stride, const void* agg, int64_t agg_node_stride,
                                         int32_t num_nodes, int32_t C, int32_t P, float* gw, float* gbias,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
  if (!is_half(dtype) || num_nodes < 0 || C < 0 || P < 0) return hipErrorInvalidValue;
  if (C == 0 || (gw == nullptr && gbias == nullptr)) return hipSuccess;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t M = C, N = 2 * (int64_t)C;
  if (num_nodes == 0 || P == 0) {  // empty sum
    if (gw && hipMemsetAsync(gw, 0, M * N * 4, st) != hipSuccess) return hipErrorUnknown;
    if (gbias && hipMemsetAsync(gbias, 0, M * 4, st) != hipSuccess) return hipErrorUnknown;
    return hipSuccess;
  }
  const int64_t plane = (int64_t)C * P;
  if (!gy || !x || !agg || !gw || gy_node_stride < plane || x_node_stride < plane || agg_node_stride < plane)
    return hipErrorInvalidValue;
  if (!aligned16(gy) || !aligned16(x) || !aligned16(agg) || !aligned16(gw) || (gy_node_stride & 7) ||
      (x_node_stride & 7) || (agg_node_stride & 7))
    return hipErrorInvalidValue;
  if (C % 32 != 0 || P % BK != 0 || !native_on()) return hipErrorNotSupported;
  NTArgs a = {};
  a.g = static_cast<const char*>(gy);
  a.gs = gy_node_stride;
  a.s0 = static_cast<const char*>(x);
  a.s0s = x_node_stride;
  a.s1 = static_cast<const char*>(agg);
  a.s1s = agg_node_stride;
  a.n0 = C;
  a.P = P;
  a.ktot = (int64_t)num_nodes * P;
  return run_wgrad(dtype, gemm_nt_half<BF16>, gemm_nt_half<F16>, a, mrp_host::tuning().half_nt_splits, M, N, gw, gbias,
                   workspace, workspace_bytes, st);
}
