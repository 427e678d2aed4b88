#pragma once
// film_attn_kernels.hpp — gfx950 kernels of the attention-pooled FiLM aggregation (mrp_film_attn_fwd / _bwd)
//
//   m_j[c,p]   = fl(fl(gamma_j[c] * x[u_j,c,p]) + beta_j[c])    j = 0, 1, ... over v's CSR row (edge-id order)
//   s_j[p]     = scale * sum_c x[v,c,p] * m_j[c,p]
//   a_j[p]     = softmax_j s_j[p]
//   out[v,c,p] = sum_j a_j[p] * m_j[c,p]
//
// The weights of a pixel need all C channels, so the decomposition is pixel-tile-major, unlike every other
// aggregation kernel here: a workgroup owns (graph, tile of kAttnTile = 64 pixels) for all channels and all of
// the graph's nodes.  Lane l of every wave owns pixel 64 tile + l (one element per access: a wave reads a
// contiguous 256-byte run of a (node, channel) plane in fp32, and no alignment or stride condition exists, so
// the geometry — and with it the order of every sum — depends on C, P and the graph only, never on the
// storage type or the pointers).  Wave w owns the destinations v = w, w + 4, w + 8, w + 12: their <= 16
// scores each (64 registers) stay in that wave's registers from the channel sweep through the softmax to the
// second sweep, so no score ever crosses a wave and the channel sum of a score is a single ascending chain.
//
// Channels are streamed in chunks: the workgroup stages x[u, c, tile] of all n nodes and the chunk's
// (gamma, beta) per slot in LDS (sigmoid applied once per slot and channel; the next chunk's loads are in
// flight in registers while the current one is computed: AttnChunk), then every wave reads the
// sources of its destinations' slots from LDS at a wave-uniform node index — the dynamic register index that
// costs film_max its select chains is an LDS address here.  A row's first KS slots (KS = 4, 8 or 16, from the
// graph kind's in-degree bound) are loaded from LDS in one batch and processed without a branch; slots past
// the row's end hold zeros and are discarded by selects.  (A wave-uniform branch per slot, the first form of
// these kernels, left every slot its own LDS round trip: 1.7 x slower in the forward at the headline shape.)
//
// Forward: sweep A accumulates s, the softmax runs in registers (v_exp_f32 on the max-subtracted score, an
// IEEE division by the sum), the weights go to attn (E, P); sweep B forms out.
// Backward: sweep A accumulates da_j = sum_c g[v] m_j, then ds_j = a_j (da_j - sum_k a_k da_k) with a read
// from attn; sweep B forms dm_j = a_j g[v] + scale ds_j x[v] per channel.  grad_x of the graph's nodes is
// accumulated in LDS, one lane-private partial per wave (a lane owns its pixel), and the four partials are
// summed in wave order; d gamma / d beta of a slot are reduced over the tile's 64 pixels by a fixed butterfly
// and, where a plane spans several tiles, written per tile to a workspace that film_attn_dgb_reduce sums in
// tile order.  No atomics anywhere.
//
// WGT = true instantiates the same kernels as the confidence-gated fusion (mrp_film_wattn_fwd / _bwd,
// film_wattn_*.hip): a sender map w[u, p] gates and weights the softmax.  A lane owns a pixel, so w is lane-private
// data: the graph's n x 64 weights are staged in LDS once per workgroup next to the row tables, "entry j delivered
// at this pixel" (w > 0) is a per-lane bit, and every place that discards a slot past the row's end with a
// wave-uniform select discards a silent entry with a per-lane one instead — a silent entry is never multiplied
// by zero.  The channel sweeps are unchanged (the silent slots' scores are formed and kept: grad_w needs their
// da_j); only the softmax step, the ds step and the selects differ.  grad_w[u, p] sums over the destinations in
// ascending order: the waves take turns, one destination at a time, on one lane-private LDS cell per (node,
// pixel) — at most 16 barriers per workgroup, one writer per element, no atomics.  WGT = false compiles the
// statements film_attn always had.
//
// MH = true instantiates the same kernels as the multi-head operators (mrp_film_attn_*_mh, mrp_film_wattn_*_mh,
// film_attn_mh_*.hip): the grid gains a head factor (blockIdx.y), and a workgroup rebases its argument block to
// its head — x, out, grad_out, grad_x and its base by head * Ch * P elements, gb / grad_gb / the grad_gb workspace
// by head * Ch channel columns, attn / rate by head * E * P, a.C = Ch — and then runs the single-head statements.
// Only the row stride of gb (the full C, gbC below) differs from a.C, so chunk boundaries count from the head's
// first channel and head k's bits are those of a single-head launch on the channel slice.  grad_w crosses heads:
// each head writes its in-workgroup sum to a partial (H, nodes, P) and film_attn_gw_reduce adds them, heads
// ascending.  MH = false compiles the statements the single-head kernels always had.

#include <type_traits>

#include "film_mean_kernels.hpp"

namespace mrp {

constexpr int kAttnSlots = MRP_FILM_ATTN_DEGREE;  // LDS slot stride per destination
constexpr int kAttnTile = 64;                     // pixels per workgroup: one per lane of a wave
constexpr int kAttnWaves = kBlock / 64;
constexpr int kAttnDpw = (MRP_MAX_NODES + kAttnWaves - 1) / kAttnWaves;  // destinations per wave
constexpr int kAttnFwdChunk = 8;  // channels staged at a time (forward: 16 n x and 16 n (gamma, beta) floats each)
// backward: + grad_out and 4 lane-private grad_x partials per (channel, node): 4 channels for <= 8 nodes, else 2
constexpr int kAttnBwdChunkSmall = 4, kAttnBwdChunk = 2;

struct AttnArgs {
  AggArgs a;         // the mean kernels' argument block (fwd: out = the aggregate; bwd: out = grad_x)
  int32_t complete;  // MRP_GRAPH_COMPLETE: slots and edge ids are arithmetic, every graph has a.nmax nodes
  int32_t ntile;     // pixel tiles per plane (grid = graphs x ntile)
  int32_t nnodes;    // film_attn_dgb_reduce: nodes of the batch
  float scale;
  float* attn;       // (E, P) softmax weights by edge id (fwd: written, bwd: read)
  float* ws;         // backward, ntile > 1: d gamma / d beta partials [ntile][E][C][2]
  int64_t E;
};

// The WGT kernels' argument block (film_attn's own kernels keep AttnArgs as it was).
struct WAttnArgs : AttnArgs {
  const float* w;    // (nodes, P) sender maps by source node, node stride wst
  int64_t wst;
  float* rate;       // (E, P) d a_j / d w_j up to the centring, by edge id (fwd: written if non-null, bwd: read)
  float* gw;         // backward: grad_w (nodes, P), node stride gwst; null: not wanted
  int64_t gwst;
};
template <bool WGT>
using AttnArgsOf = std::conditional_t<WGT, WAttnArgs, AttnArgs>;

// The MH kernels' argument block: a.C holds the channels of one head, gbC the channels of gb's rows.
template <bool WGT>
struct AttnMhArgs : AttnArgsOf<WGT> {
  int32_t gbC;   // C: the channel stride of gb, grad_gb and the grad_gb workspace
  int64_t gwhs;  // WGT backward: elements between two heads' grad_w partials (gw points at head 0's)
};
template <bool WGT, bool MH>
using AttnKernelArgs = std::conditional_t<MH, AttnMhArgs<WGT>, AttnArgsOf<WGT>>;

// MH: rebase the argument block to this workgroup's head (blockIdx.y): what a single-head launch on the head's
// channel slice would get.
template <typename T, bool WGT>
__device__ __forceinline__ void attn_head_rebase(AttnMhArgs<WGT>& m) {
  AggArgs& a = m.a;
  const int64_t k = blockIdx.y;
  const int64_t xoff = k * a.C * a.P, goff = k * a.C * 2, eoff = k * m.E * a.P;
  a.x = static_cast<const T*>(a.x) + xoff;
  if (a.g != nullptr) a.g = static_cast<const T*>(a.g) + xoff;
  if (a.out != nullptr) a.out = static_cast<T*>(a.out) + xoff;
  if (a.dxb != nullptr) a.dxb = static_cast<const T*>(a.dxb) + xoff;
  if (a.gb != nullptr) a.gb += goff;
  if (a.dgb != nullptr) a.dgb += goff;
  if (m.ws != nullptr) m.ws += goff;
  if (m.attn != nullptr) m.attn += eoff;
  if constexpr (WGT) {
    if (m.rate != nullptr) m.rate += eoff;
    if (m.gw != nullptr) m.gw += k * m.gwhs;
  }
}

// the channels of gb's rows
template <bool MH, typename Args>
__device__ __forceinline__ int attn_gb_channels(const Args& m) {
  if constexpr (MH)
    return m.gbC;
  else
    return m.a.C;
}

// LDS of one workgroup for graphs of up to nmax nodes and chunks of ck channels.
struct AttnLds {
  float* X;                    // [ck][nmax][64] the chunk's x, widened
  float2* W;                   // [ck][nmax * 16] (gamma, beta) per slot
  float* G;                    // backward: [ck][nmax][64] the chunk's grad_out, widened
  float* D;                    // backward: [4 waves][ck][nmax][64] grad_x partials
  unsigned long long* slot_u;  // [nmax] the row's local sources, 4 bits each, slot 0 lowest
  int* slot_e;                 // [nmax * 16] edge id, -1: no such slot
  int* rowlen;                 // [nmax]; WGT: followed by [nmax][64] the tile's sender weights (attn_wt)
  __device__ __forceinline__ AttnLds(void* smem, int nmax, int ck, bool bwd) {
    X = reinterpret_cast<float*>(smem);
    W = reinterpret_cast<float2*>(X + ck * nmax * kAttnTile);
    G = reinterpret_cast<float*>(W + ck * nmax * kAttnSlots);
    D = G + (bwd ? ck * nmax * kAttnTile : 0);
    slot_u = reinterpret_cast<unsigned long long*>(D + (bwd ? kAttnWaves * ck * nmax * kAttnTile : 0));
    slot_e = reinterpret_cast<int*>(slot_u + nmax);
    rowlen = slot_e + nmax * kAttnSlots;
  }
};

__device__ __forceinline__ float* attn_wt(const AttnLds& L, int nmax) {
  return reinterpret_cast<float*>(L.rowlen + nmax);
}

// WGT: the tile's weights of the graph's nodes into LDS (zeros past the plane's end: silent).  Wave w stages the
// nodes it stages x of.  Published by the barrier that ends attn_tables.
__device__ __forceinline__ void attn_stage_w(const WAttnArgs& m, const AttnLds& L, int node0, int n, int p, bool pin) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* Wt = attn_wt(L, m.a.nmax);
  for (int u = wave; u < n; u += kAttnWaves)
    Wt[u * kAttnTile + lane] = pin ? m.w[(int64_t)(node0 + u) * m.wst + p] : 0.f;
}

// Row lengths, sources and edge ids of the graph's rows (film_max's tables).  Ends with a barrier.
__device__ __forceinline__ void attn_tables(const AttnArgs& m, const AttnLds& L, int b, int node0, int n) {
  const AggArgs& a = m.a;
  for (int v = threadIdx.x; v < n; v += blockDim.x) {
    int beg = 0, deg = 0;
    if (m.complete) {
      deg = n - 1;
    } else {
      beg = a.kdeg > 0 ? (node0 + v) * a.kdeg : a.indptr[node0 + v];
      const int end = a.kdeg > 0 ? beg + a.kdeg : a.indptr[node0 + v + 1];
      deg = min(max(end - beg, 0), kAttnSlots);  // precondition: in-degree <= 16 (clamped: in-bounds anyway)
    }
    const int ebase = b * n * (n - 1);
    unsigned long long word = 0ull;
    for (int j = 0; j < kAttnSlots; ++j) {
      int u = 0, e = -1;
      if (j < deg) {
        if (m.complete) {
          u = j < v ? j : j + 1;  // v's in-edges in edge-id order: ascending source
          e = ebase + u * (n - 1) + (v < u ? v : v - 1);
        } else {
          u = a.src[beg + j] - node0;
          if ((unsigned)u >= (unsigned)n) u = 0;  // rejected on the host; keeps the LDS index in bounds
          e = a.eid[beg + j];
        }
      }
      word |= (unsigned long long)u << (4 * j);
      L.slot_e[v * kAttnSlots + j] = e;
    }
    L.slot_u[v] = word;
    L.rowlen[v] = deg;
  }
  __syncthreads();
}

// A chunk on its way from memory to LDS.  Wave w stages the planes of the nodes u = w, w + 4, w + 8, w + 12
// (its own destinations, so in the backward their grad_out comes along), thread t the (gamma, beta) of slot t.
// The loads of the next chunk are issued before the current chunk is computed and land in LDS after it: the
// memory latency lies under the arithmetic, and nothing waits on a load it has just issued.
template <int CK, bool BWD, typename T>
struct AttnChunk {
  T x[CK * kAttnDpw];  // as stored: widened when put (a conversion here would wait for the load it follows)
  T g[BWD ? CK * kAttnDpw : 1];
  T b[BWD ? CK * kAttnDpw : 1];  // grad_x_base of the nodes this wave writes
  float2 w[CK];
};

// Issue the loads of chunk [c0, c0 + CK) (zeros past C, past the graph's nodes and past the plane's end).
// my_e: the edge id of slot threadIdx.x (-1: none).  with_base (wave-uniform): also grad_x_base, which only the
// backward's second sweep reads.  MH: gbC is the channels of gb's rows (else a.C, read here as it always was).
template <int CK, bool BWD, typename T, bool MH = false>
__device__ __forceinline__ void attn_fetch(const AttnArgs& m, int node0, int n, int c0, int p, bool pin, int my_e,
                                           AttnChunk<CK, BWD, T>& r, bool with_base = false, int gbC = 0) {
  const AggArgs& a = m.a;
  const int wave = threadIdx.x >> 6;
  const int ck = min(CK, a.C - c0);  // <= 0 past the last chunk: nothing is loaded
  const T* xb = static_cast<const T*>(a.x) + (int64_t)node0 * a.xs + (int64_t)c0 * a.P + p;
  const T* gp = BWD ? static_cast<const T*>(a.g) + (int64_t)node0 * a.gs + (int64_t)c0 * a.P + p : nullptr;
  const T* bp = BWD && with_base && a.dxb != nullptr
                    ? static_cast<const T*>(a.dxb) + (int64_t)node0 * a.dxbs + (int64_t)c0 * a.P + p
                    : nullptr;
#pragma unroll
  for (int cl = 0; cl < CK; ++cl) {
#pragma unroll
    for (int i = 0; i < kAttnDpw; ++i) {
      const int u = wave + kAttnWaves * i;
      T xv = (T)0.f, gv = (T)0.f, bv = (T)0.f;
      if (cl < ck && u < n && pin) {
        xv = xb[(int64_t)u * a.xs + (int64_t)cl * a.P];
        if constexpr (BWD) {
          gv = gp[(int64_t)u * a.gs + (int64_t)cl * a.P];
          if (bp != nullptr) bv = bp[(int64_t)u * a.dxbs + (int64_t)cl * a.P];
        }
      }
      r.x[cl * kAttnDpw + i] = xv;
      if constexpr (BWD) {
        r.g[cl * kAttnDpw + i] = gv;
        r.b[cl * kAttnDpw + i] = bv;
      }
    }
    float2 w = make_float2(0.f, 0.f);
    if constexpr (MH) {
      if (cl < ck && my_e >= 0) w = *reinterpret_cast<const float2*>(a.gb + ((int64_t)my_e * gbC + c0 + cl) * 2);
    } else {
    if (cl < ck && my_e >= 0) w = *reinterpret_cast<const float2*>(a.gb + ((int64_t)my_e * a.C + c0 + cl) * 2);
    }
    r.w[cl] = w;
  }
}

// Put a fetched chunk into LDS, between the barrier that ends the previous chunk's reads and the one that
// publishes this one.  16-bit elements are widened here and the sigmoid of logits is applied here, once per
// (slot, channel).
template <int CK, bool BWD, typename T>
__device__ __forceinline__ void attn_put(const AttnArgs& m, const AttnLds& L, int n, int my_e,
                                         const AttnChunk<CK, BWD, T>& r) {
  const AggArgs& a = m.a;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
#pragma unroll
  for (int cl = 0; cl < CK; ++cl) {
#pragma unroll
    for (int i = 0; i < kAttnDpw; ++i) {
      const int u = wave + kAttnWaves * i;
      if (u < n) {
        L.X[(cl * a.nmax + u) * kAttnTile + lane] = (float)r.x[cl * kAttnDpw + i];
        if constexpr (BWD) L.G[(cl * a.nmax + u) * kAttnTile + lane] = (float)r.g[cl * kAttnDpw + i];
      }
    }
    if ((int)threadIdx.x < n * kAttnSlots) {
      float2 w = r.w[cl];
      if (a.logits && my_e >= 0) w = make_float2(sigmoidf(w.x), sigmoidf(w.y));
      L.W[cl * a.nmax * kAttnSlots + threadIdx.x] = w;
    }
  }
  __syncthreads();
}

// The wave-uniform description of destination v's row.
struct AttnRow {
  int deg;
  unsigned ulo, uhi;
  __device__ __forceinline__ AttnRow(const AttnLds& L, int v) {
    deg = __builtin_amdgcn_readfirstlane(L.rowlen[v]);
    const unsigned long long uw = L.slot_u[v];
    ulo = __builtin_amdgcn_readfirstlane((unsigned)uw);
    uhi = __builtin_amdgcn_readfirstlane((unsigned)(uw >> 32));
  }
  __device__ __forceinline__ int src(int jj) const { return ((jj < 8 ? ulo : uhi) >> (4 * (jj & 7))) & 15u; }
};

// The chunk-channel's (gamma, beta) and source value of a row's first KS slots, loaded from LDS in one batch
// with no branch in between (a branch per slot leaves every slot its own LDS round trip).  Slots past the
// row's end hold (0, 0) and source 0: their products are computed and discarded by the callers' selects.
template <int KS>
__device__ __forceinline__ void attn_slots(const float* Xc, const float2* Wc, const AttnRow& r, float2 (&w)[KS],
                                           float (&xu)[KS]) {
#pragma unroll
  for (int jj = 0; jj < KS; ++jj) {
    w[jj] = Wc[jj];
    xu[jj] = Xc[r.src(jj) * kAttnTile];
  }
}

// acc[i][j] += q_i[c,p] * m_j[c,p] over the chunk's ck channels for this wave's destinations; q is x[v] in the
// forward and grad_out[v] in the backward.  (Accumulators of slots past a row's end collect garbage, unread.)
template <bool BWD, int KS>
__device__ __forceinline__ void attn_scores(const AttnArgs& m, const AttnLds& L, int n, int ck,
                                            float (&acc)[kAttnDpw][KS]) {
  const AggArgs& a = m.a;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < kAttnDpw; ++i) {
    const int v = wave + kAttnWaves * i;
    if (v >= n) continue;  // wave-uniform
    const AttnRow r(L, v);
    for (int cl = 0; cl < ck; ++cl) {
      const float* Xc = L.X + cl * a.nmax * kAttnTile + lane;
      const float2* Wc = L.W + cl * a.nmax * kAttnSlots + v * kAttnSlots;
      const float q = BWD ? L.G[(cl * a.nmax + v) * kAttnTile + lane] : Xc[v * kAttnTile];
      float2 w[KS];
      float xu[KS];
      attn_slots<KS>(Xc, Wc, r, w, xu);
#pragma unroll
      for (int jj = 0; jj < KS; ++jj) {
        const float msg = __fadd_rn(__fmul_rn(w[jj].x, xu[jj]), w[jj].y);
        acc[i][jj] = __fmaf_rn(q, msg, acc[i][jj]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// FP8 messages, receiver side (film_attn_fwd with TX = q8_t).  The messages are x^[u,c,p] = fl32(s[u,c] * decode(xq[u,c,p])):
// codes of format a.qfmt (E4M3 / E5M2, never FNUZ) at a.x, node stride a.xs, with per-(source node, channel)
// scales a.xscale (rows of C, NULL: all 1).  The receiver's own features never crossed the link: the query of
// destination v is q[v,c,p] of type T, a second tensor.  Wave w stages exactly the nodes that are its own
// destinations and a lane owns its pixel, so the chunk's query values stay in that wave's registers (CK x
// kAttnDpw of them) and LDS holds what it always held.  From the staged plane on the statements are
// film_attn_fwd's.
// ---------------------------------------------------------------------------
template <bool WGT, bool MH>
struct AttnQArgs : AttnKernelArgs<WGT, MH> {
  const void* q;  // (nodes, C, P) own features of type T, node stride qs
  int64_t qs;
};
// film_attn_fwd's argument block for messages of type TX
template <bool WGT, bool MH, typename TX>
using AttnFwdArgs =
    std::conditional_t<std::is_same<TX, q8_t>::value, AttnQArgs<WGT, MH>, AttnKernelArgs<WGT, MH>>;

// MH: what a single-head launch on the head's channel slice of the codes, the scales and the query would get.
template <typename T, bool WGT>
__device__ __forceinline__ void attn_head_rebase_q(AttnQArgs<WGT, true>& m) {
  AggArgs& a = m.a;
  const int64_t k = blockIdx.y;
  const int64_t xoff = k * a.C * a.P, eoff = k * m.E * a.P;
  a.x = static_cast<const q8_t*>(a.x) + xoff;
  m.q = static_cast<const T*>(m.q) + xoff;
  a.out = static_cast<T*>(a.out) + xoff;
  if (a.gb != nullptr) a.gb += k * a.C * 2;
  if (a.xscale != nullptr) a.xscale += k * a.C;
  if (m.attn != nullptr) m.attn += eoff;
  if constexpr (WGT) {
    if (m.rate != nullptr) m.rate += eoff;
  }
}

// One code, decoded by load_frag's hardware conversions and multiplied once by its scale.
__device__ __forceinline__ float attn_decode(uint8_t code, int fmt, float s) {
  const f2 v = fmt == MRP_QDTYPE_E5M2 ? __builtin_amdgcn_cvt_pk_f32_bf8((int)code, false)
                                      : __builtin_amdgcn_cvt_pk_f32_fp8((int)code, false);
  return __fmul_rn(s, v.x);
}

template <int CK, typename T>
struct AttnChunkQ {
  uint8_t x[CK * kAttnDpw];  // codes as stored: decoded when put
  float sc[CK * kAttnDpw];   // their scales (wave-uniform)
  T q[CK * kAttnDpw];        // the query of the wave's destinations
  float2 w[CK];
};

// attn_fetch for codes.  QUERY: also the query values (sweep A alone reads them).  gbC: the channels of gb's and
// the scales' rows.
template <int CK, typename T, bool QUERY, typename Args>
__device__ __forceinline__ void attn_fetch_q(const Args& m, int node0, int n, int c0, int p, bool pin, int my_e,
                                             AttnChunkQ<CK, T>& r, int gbC) {
  const AggArgs& a = m.a;
  const int wave = threadIdx.x >> 6;
  const int wu = __builtin_amdgcn_readfirstlane(wave);  // the scales' addresses are scalar
  const int ck = min(CK, a.C - c0);  // <= 0 past the last chunk: nothing is loaded
  const q8_t* xb = static_cast<const q8_t*>(a.x) + (int64_t)node0 * a.xs + (int64_t)c0 * a.P + p;
  const T* qb = static_cast<const T*>(m.q) + (int64_t)node0 * m.qs + (int64_t)c0 * a.P + p;
  const float* sb = a.xscale != nullptr ? a.xscale + (int64_t)node0 * gbC + c0 : nullptr;
#pragma unroll
  for (int cl = 0; cl < CK; ++cl) {
#pragma unroll
    for (int i = 0; i < kAttnDpw; ++i) {
      const int u = wave + kAttnWaves * i;
      uint8_t xv = 0;
      T qv = (T)0.f;
      if (cl < ck && u < n && pin) {
        xv = xb[(int64_t)u * a.xs + (int64_t)cl * a.P].b;
        if constexpr (QUERY) qv = qb[(int64_t)u * m.qs + (int64_t)cl * a.P];
      }
      r.x[cl * kAttnDpw + i] = xv;
      r.q[cl * kAttnDpw + i] = qv;
      const int uu = wu + kAttnWaves * i;
      r.sc[cl * kAttnDpw + i] = (sb != nullptr && cl < ck && uu < n) ? sb[(int64_t)uu * gbC + cl] : 1.f;
    }
    float2 w = make_float2(0.f, 0.f);
    if (cl < ck && my_e >= 0) w = *reinterpret_cast<const float2*>(a.gb + ((int64_t)my_e * gbC + c0 + cl) * 2);
    r.w[cl] = w;
  }
}

// attn_put for codes: decoded and scaled here, once per (node, channel, pixel).
template <int CK, typename T, typename Args>
__device__ __forceinline__ void attn_put_q(const Args& m, const AttnLds& L, int n, int my_e,
                                           const AttnChunkQ<CK, T>& r) {
  const AggArgs& a = m.a;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
#pragma unroll
  for (int cl = 0; cl < CK; ++cl) {
#pragma unroll
    for (int i = 0; i < kAttnDpw; ++i) {
      const int u = wave + kAttnWaves * i;
      if (u < n)
        L.X[(cl * a.nmax + u) * kAttnTile + lane] =
            attn_decode(r.x[cl * kAttnDpw + i], a.qfmt, r.sc[cl * kAttnDpw + i]);
    }
    if ((int)threadIdx.x < n * kAttnSlots) {
      float2 w = r.w[cl];
      if (a.logits && my_e >= 0) w = make_float2(sigmoidf(w.x), sigmoidf(w.y));
      L.W[cl * a.nmax * kAttnSlots + threadIdx.x] = w;
    }
  }
  __syncthreads();
}

// attn_scores with the query in registers: acc[i][j] += q_i[c,p] * m_j[c,p], the same ascending chain.  A
// destination's CK query values are one register vector, the chunk channel a wave-uniform dynamic extract (as
// film_max's sources are): the channel loop stays rolled, as attn_scores' is.
template <int CK>
struct AttnQVec {
  typedef float type __attribute__((ext_vector_type(CK)));
};
template <int CK, int KS, typename Args>
__device__ __forceinline__ void attn_scores_q(const Args& m, const AttnLds& L, int n, int ck,
                                              const typename AttnQVec<CK>::type (&q)[kAttnDpw],
                                              float (&acc)[kAttnDpw][KS]) {
  const AggArgs& a = m.a;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < kAttnDpw; ++i) {
    const int v = wave + kAttnWaves * i;
    if (v >= n) continue;  // wave-uniform
    const AttnRow r(L, v);
    for (int cl = 0; cl < ck; ++cl) {
      const float* Xc = L.X + cl * a.nmax * kAttnTile + lane;
      const float2* Wc = L.W + cl * a.nmax * kAttnSlots + v * kAttnSlots;
      const float qv = q[i][cl];
      float2 w[KS];
      float xu[KS];
      attn_slots<KS>(Xc, Wc, r, w, xu);
#pragma unroll
      for (int jj = 0; jj < KS; ++jj) {
        const float msg = __fadd_rn(__fmul_rn(w[jj].x, xu[jj]), w[jj].y);
        acc[i][jj] = __fmaf_rn(qv, msg, acc[i][jj]);
      }
    }
  }
}

// Sum over the wave's 64 lanes, valid in lane 63: within rows of 16 by quad_perm, row_half_mirror and row_mirror,
// then row 0 into 1 and 2 into 3 (row_bcast15), then rows 0-1 into 2-3 (row_bcast31).  DPP only: no LDS round
// trip, a fixed order.
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_rows(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, ROWS, 0xf, false));
}
__device__ __forceinline__ float wave_sum63(float x) {
  x += dpp_mov<0xB1>(x);
  x += dpp_mov<0x4E>(x);
  x += dpp_mov<0x141>(x);
  x += dpp_mov<0x140>(x);
  x += dpp_rows<0x142, 0xA>(x);
  x += dpp_rows<0x143, 0xC>(x);
  return x;
}

// ---------------------------------------------------------------------------
// Forward.  Workgroup = graph x pixel tile.  KS: compiled slots per destination (4, 8 or 16; the launcher picks
// KS >= the graph kind's in-degree bound).
// ---------------------------------------------------------------------------
// TX: the storage type of the messages.  TX = T: they are x itself, and x[v] is also v's query (mrp_film_attn_fwd and
// its kin).  TX = q8_t: FP8 codes with per-(source node, channel) scales, and the query is a tensor of its own
// (a.x holds the codes, m.q the receiver's own features; T is their type and the output's: mrp_film_attn_fwd_q /
// mrp_film_wattn_fwd_q).
template <typename T, int KS, bool WGT = false, bool MH = false, typename TX = T>
__global__ void __launch_bounds__(kBlock) film_attn_fwd(AttnFwdArgs<WGT, MH, TX> m) {
  constexpr bool kQ = std::is_same<TX, q8_t>::value;
  if constexpr (MH) {
    if constexpr (kQ)
      attn_head_rebase_q<T, WGT>(m);
    else
      attn_head_rebase<T, WGT>(m);
  }
  const AggArgs& a = m.a;
  extern __shared__ float4 smem_f4[];
  const AttnLds L(smem_f4, a.nmax, kAttnFwdChunk, false);
  const int b = blockIdx.x / m.ntile;
  const int tile = blockIdx.x - b * m.ntile;
  const int node0 = m.complete ? b * a.nmax : a.goff[b];
  const int n = m.complete ? a.nmax : min(a.goff[b + 1] - node0, a.nmax);
  if (n <= 0) return;  // whole workgroup: empty graph
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p = tile * kAttnTile + lane;
  const bool pin = p < a.P;
  if constexpr (WGT) attn_stage_w(m, L, node0, n, p, pin);
  attn_tables(m, L, b, node0, n);
  constexpr int CK = kAttnFwdChunk;
  const int my_e = (int)threadIdx.x < n * kAttnSlots ? L.slot_e[threadIdx.x] : -1;
  std::conditional_t<kQ, AttnChunkQ<CK, T>, AttnChunk<CK, false, T>> next;
  if constexpr (kQ)
    attn_fetch_q<CK, T, true>(m, node0, n, 0, p, pin, my_e, next, attn_gb_channels<MH>(m));
  else
  attn_fetch<CK, false, T, MH>(m, node0, n, 0, p, pin, my_e, next, false, attn_gb_channels<MH>(m));

  float s[kAttnDpw][KS];
#pragma unroll
  for (int i = 0; i < kAttnDpw; ++i)
#pragma unroll
    for (int jj = 0; jj < KS; ++jj) s[i][jj] = 0.f;

  // sweep A: the scores, each an ascending chain over the channels
  for (int c0 = 0; c0 < a.C; c0 += CK) {
    if constexpr (kQ) {
      attn_put_q<CK, T>(m, L, n, my_e, next);
      typename AttnQVec<CK>::type q[kAttnDpw];  // this chunk's query values, kept while the next chunk is fetched
#pragma unroll
      for (int cl = 0; cl < CK; ++cl)
#pragma unroll
        for (int i = 0; i < kAttnDpw; ++i) q[i][cl] = (float)next.q[cl * kAttnDpw + i];
      if (c0 + CK < a.C)
        attn_fetch_q<CK, T, true>(m, node0, n, c0 + CK, p, pin, my_e, next, attn_gb_channels<MH>(m));
      else  // wraps: sweep B's first, which scores nothing
        attn_fetch_q<CK, T, false>(m, node0, n, 0, p, pin, my_e, next, attn_gb_channels<MH>(m));
      attn_scores_q<CK, KS>(m, L, n, min(CK, a.C - c0), q, s);
    } else {
    attn_put<CK, false, T>(m, L, n, my_e, next);
    attn_fetch<CK, false, T, MH>(m, node0, n, c0 + CK < a.C ? c0 + CK : 0, p, pin, my_e, next, false,
                                attn_gb_channels<MH>(m));  // wraps: sweep B's first
    attn_scores<false, KS>(m, L, n, min(CK, a.C - c0), s);
    }
  }

  // softmax over the row's entries, in registers; s becomes the weights
  constexpr float kLog2e = 1.4426950408889634f;
  unsigned dmask[kAttnDpw];  // WGT: bit j: entry j of destination i delivered at this lane's pixel
#pragma unroll
  for (int i = 0; i < kAttnDpw; ++i) dmask[i] = 0u;
#pragma unroll
  for (int i = 0; i < kAttnDpw; ++i) {
    const int v = wave + kAttnWaves * i;
    if (v >= n) continue;
    const int deg = __builtin_amdgcn_readfirstlane(L.rowlen[v]);
    float mx = -__builtin_inff();
    if constexpr (WGT) {
      // the gated softmax: max and sum over the delivered entries of this lane's pixel; u_j = exp(s_j - mx) for
      // every entry (a silent one's goes to rate only)
      const AttnRow r(L, v);
      const float* Wl = attn_wt(L, a.nmax) + lane;
      unsigned dl = 0u;
#pragma unroll
      for (int jj = 0; jj < KS; ++jj) {
        if (jj >= deg) continue;
        s[i][jj] = __fmul_rn(m.scale, s[i][jj]);
        const bool d = Wl[r.src(jj) * kAttnTile] > 0.f;  // false for a negative or NaN weight
        dl |= d ? 1u << jj : 0u;
        mx = d ? fmaxf(mx, s[i][jj]) : mx;
      }
      float z = 0.f;
#pragma unroll
      for (int jj = 0; jj < KS; ++jj) {
        if (jj >= deg) continue;
        s[i][jj] = __builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(s[i][jj], mx), kLog2e));
        const float t = __fmul_rn(Wl[r.src(jj) * kAttnTile], s[i][jj]);
        z = (dl >> jj) & 1u ? __fadd_rn(z, t) : z;
      }
      const bool zpos = dl != 0u && z > 0.f;  // nobody delivered: mx = -inf and the u_j mean nothing
#pragma unroll
      for (int jj = 0; jj < KS; ++jj) {
        if (jj >= deg) continue;
        const float u = s[i][jj];
        const float t = __fmul_rn(Wl[r.src(jj) * kAttnTile], u);
        s[i][jj] = zpos && ((dl >> jj) & 1u) ? __fdiv_rn(t, z) : 0.f;
        const int e = L.slot_e[v * kAttnSlots + jj];
        if (pin) {
          m.attn[(int64_t)e * a.P + p] = s[i][jj];
          if (m.rate != nullptr) m.rate[(int64_t)e * a.P + p] = zpos ? __fdiv_rn(u, z) : 0.f;
        }
      }
      dmask[i] = dl;
      continue;
    }
#pragma unroll
    for (int jj = 0; jj < KS; ++jj) {
      if (jj >= deg) continue;
      s[i][jj] = __fmul_rn(m.scale, s[i][jj]);
      mx = fmaxf(mx, s[i][jj]);
    }
    float sum = 0.f;
#pragma unroll
    for (int jj = 0; jj < KS; ++jj) {
      if (jj >= deg) continue;
      s[i][jj] = __builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(s[i][jj], mx), kLog2e));
      sum = __fadd_rn(sum, s[i][jj]);
    }
#pragma unroll
    for (int jj = 0; jj < KS; ++jj) {
      if (jj >= deg) continue;
      s[i][jj] = __fdiv_rn(s[i][jj], sum);
      const int e = L.slot_e[v * kAttnSlots + jj];
      if (pin) m.attn[(int64_t)e * a.P + p] = s[i][jj];
    }
  }

  // sweep B: out = sum_j a_j m_j in slot order
  for (int c0 = 0; c0 < a.C; c0 += CK) {
    const int ck = min(CK, a.C - c0);
    if constexpr (kQ) {
      attn_put_q<CK, T>(m, L, n, my_e, next);
      attn_fetch_q<CK, T, false>(m, node0, n, c0 + CK, p, pin, my_e, next, attn_gb_channels<MH>(m));
    } else {
    attn_put<CK, false, T>(m, L, n, my_e, next);
    attn_fetch<CK, false, T, MH>(m, node0, n, c0 + CK, p, pin, my_e, next, false, attn_gb_channels<MH>(m));
    }
#pragma unroll
    for (int i = 0; i < kAttnDpw; ++i) {
      const int v = wave + kAttnWaves * i;
      if (v >= n) continue;
      const AttnRow r(L, v);
      T* ob = static_cast<T*>(a.out) + (int64_t)(node0 + v) * a.os + (int64_t)c0 * a.P + p;
      for (int cl = 0; cl < ck; ++cl) {
        const float* Xc = L.X + cl * a.nmax * kAttnTile + lane;
        const float2* Wc = L.W + cl * a.nmax * kAttnSlots + v * kAttnSlots;
        float2 w[KS];
        float xu[KS];
        attn_slots<KS>(Xc, Wc, r, w, xu);
        Frag<1> o;
        if constexpr (WGT) {
          // fma onto -0 is the bare product, sign of zero included: the chain starts at the lane's first
          // delivered entry as film_attn's starts at slot 0
          o.v[0] = -0.f;
#pragma unroll
          for (int jj = 0; jj < KS; ++jj) {
            const float msg = __fadd_rn(__fmul_rn(w[jj].x, xu[jj]), w[jj].y);
            const float t = __fmaf_rn(s[i][jj], msg, o.v[0]);
            o.v[0] = (dmask[i] >> jj) & 1u ? t : o.v[0];  // a per-lane select: a silent entry is never multiplied
          }
          o.v[0] = dmask[i] != 0u ? o.v[0] : 0.f;  // nobody delivered (or an empty row): an exact zero
        } else {
        o.v[0] = 0.f;  // empty row: zeros
#pragma unroll
        for (int jj = 0; jj < KS; ++jj) {
          const float msg = __fadd_rn(__fmul_rn(w[jj].x, xu[jj]), w[jj].y);
          const float t = jj == 0 ? __fmul_rn(s[i][jj], msg) : __fmaf_rn(s[i][jj], msg, o.v[0]);
          o.v[0] = jj < r.deg ? t : o.v[0];  // a select, not a branch (wave-uniform)
        }
        }
        if (pin) store_frag<1, true>(ob + (int64_t)cl * a.P, o);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Backward.  Workgroup = graph x pixel tile; a.want_dx / a.want_dgb choose the outputs (the arithmetic of
// either is the same whether or not the other is wanted).  CK: channels per chunk; KS as in the forward.
// ---------------------------------------------------------------------------
template <typename T, int CK, int KS, bool WGT = false, bool MH = false>
__global__ void __launch_bounds__(kBlock) film_attn_bwd(AttnKernelArgs<WGT, MH> m) {
  if constexpr (MH) attn_head_rebase<T, WGT>(m);
  const AggArgs& a = m.a;
  extern __shared__ float4 smem_f4[];
  const AttnLds L(smem_f4, a.nmax, CK, true);
  const int b = blockIdx.x / m.ntile;
  const int tile = blockIdx.x - b * m.ntile;
  const int node0 = m.complete ? b * a.nmax : a.goff[b];
  const int n = m.complete ? a.nmax : min(a.goff[b + 1] - node0, a.nmax);
  if (n <= 0) return;  // whole workgroup
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p = tile * kAttnTile + lane;
  const bool pin = p < a.P;
  if constexpr (WGT) attn_stage_w(m, L, node0, n, p, pin);
  attn_tables(m, L, b, node0, n);
  const int my_e = (int)threadIdx.x < n * kAttnSlots ? L.slot_e[threadIdx.x] : -1;
  AttnChunk<CK, true, T> next;
  attn_fetch<CK, true, T, MH>(m, node0, n, 0, p, pin, my_e, next, false, attn_gb_channels<MH>(m));

  float ds[kAttnDpw][KS], at[kAttnDpw][KS];
#pragma unroll
  for (int i = 0; i < kAttnDpw; ++i)
#pragma unroll
    for (int jj = 0; jj < KS; ++jj) ds[i][jj] = at[i][jj] = 0.f;

  // sweep A: da_j = sum_c g[v] m_j
  for (int c0 = 0; c0 < a.C; c0 += CK) {
    attn_put<CK, true, T>(m, L, n, my_e, next);
    const bool last = c0 + CK >= a.C;  // then the fetch wraps to sweep B's first chunk, base included
    attn_fetch<CK, true, T, MH>(m, node0, n, last ? 0 : c0 + CK, p, pin, my_e, next, last,
                                   attn_gb_channels<MH>(m));
    attn_scores<true, KS>(m, L, n, min(CK, a.C - c0), ds);
  }
  unsigned dmask[kAttnDpw];  // WGT: bit j: entry j of destination i delivered at this lane's pixel
#pragma unroll
  for (int i = 0; i < kAttnDpw; ++i) dmask[i] = 0u;
  if constexpr (WGT) {
    // grad_w's cells, one per (node, pixel), in the grad_x partials' space (unused until sweep B)
    if (m.gw != nullptr) {
      for (int t = threadIdx.x; t < n * kAttnTile; t += blockDim.x) L.D[t] = 0.f;
      __syncthreads();
    }
  }
  // ds_j = a_j (da_j - sum_k a_k da_k), kept multiplied by scale (both of its uses are); zeros past the row's end
#pragma unroll
  for (int i = 0; i < kAttnDpw; ++i) {
    const int v = wave + kAttnWaves * i;
    const int deg = v < n ? __builtin_amdgcn_readfirstlane(L.rowlen[v]) : 0;
    float dot = 0.f;
    if constexpr (WGT) {
      // the sum runs over the delivered entries, ds of a silent entry is 0; the silent entries' da_j are kept
      // for grad_w
      const AttnRow r(L, v < n ? v : 0);
      unsigned dl = 0u;
#pragma unroll
      for (int jj = 0; jj < KS; ++jj) {
        if (jj >= deg) continue;
        const int e = L.slot_e[v * kAttnSlots + jj];
        at[i][jj] = pin ? m.attn[(int64_t)e * a.P + p] : 0.f;
        const bool d = attn_wt(L, a.nmax)[r.src(jj) * kAttnTile + lane] > 0.f;
        dl |= d ? 1u << jj : 0u;
        dot = d ? __fmaf_rn(at[i][jj], ds[i][jj], dot) : dot;
      }
      dmask[i] = dl;
      if (m.gw != nullptr) {
        // grad_w[u_j] += r_j (da_j - dbar), destinations ascending: v = 4 i + t is wave t's, the waves take turns
#pragma unroll
        for (int t = 0; t < kAttnWaves; ++t) {
          if (kAttnWaves * i + t >= n) continue;  // workgroup-uniform
          if (wave == t) {
#pragma unroll
            for (int jj = 0; jj < KS; ++jj) {
              if (jj >= deg) continue;
              const int e = L.slot_e[v * kAttnSlots + jj];
              const float rt = pin ? m.rate[(int64_t)e * a.P + p] : 0.f;
              float* cell = L.D + r.src(jj) * kAttnTile + lane;
              *cell = __fmaf_rn(rt, __fsub_rn(ds[i][jj], dot), *cell);
            }
          }
          __syncthreads();
        }
      }
#pragma unroll
      for (int jj = 0; jj < KS; ++jj)
        ds[i][jj] = (dl >> jj) & 1u ? __fmul_rn(m.scale, __fmul_rn(at[i][jj], __fsub_rn(ds[i][jj], dot))) : 0.f;
      continue;
    }
#pragma unroll
    for (int jj = 0; jj < KS; ++jj) {
      if (jj >= deg) continue;
      const int e = L.slot_e[v * kAttnSlots + jj];
      at[i][jj] = pin ? m.attn[(int64_t)e * a.P + p] : 0.f;
      dot = __fmaf_rn(at[i][jj], ds[i][jj], dot);
    }
#pragma unroll
    for (int jj = 0; jj < KS; ++jj)
      ds[i][jj] = jj < deg ? __fmul_rn(m.scale, __fmul_rn(at[i][jj], __fsub_rn(ds[i][jj], dot))) : 0.f;
  }

  if constexpr (WGT) {
    // grad_w of the nodes this wave stages (every node of the graph is written: zeros for one nobody hears);
    // sweep B's first barrier precedes the next write to these cells
    if (m.gw != nullptr && pin)
      for (int u = wave; u < n; u += kAttnWaves)
        m.gw[(int64_t)(node0 + u) * m.gwst + p] = L.D[u * kAttnTile + lane];
  }

  // sweep B
  const bool want_dx = a.want_dx != 0, want_dgb = a.want_dgb != 0;
  if constexpr (WGT) {
    if (!want_dx && !want_dgb) return;  // grad_w alone (whole workgroup): done
  }
  for (int c0 = 0; c0 < a.C; c0 += CK) {
    const int ck = min(CK, a.C - c0);
    attn_put<CK, true, T>(m, L, n, my_e, next);
    T base[CK * kAttnDpw];  // this chunk's grad_x_base, kept while the next chunk is fetched
#pragma unroll
    for (int t = 0; t < CK * kAttnDpw; ++t) base[t] = next.b[t];
    attn_fetch<CK, true, T, MH>(m, node0, n, c0 + CK, p, pin, my_e, next, true, attn_gb_channels<MH>(m));
    float* Dw = L.D + wave * CK * a.nmax * kAttnTile + lane;  // this lane's partials: [cl][u]
    if (want_dx) {
      // lane-private: written after the barriers that ended the previous chunk's sum, read by this lane only
      // until the barrier below
      for (int t = 0; t < ck * a.nmax; ++t) Dw[t * kAttnTile] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < kAttnDpw; ++i) {
      const int v = wave + kAttnWaves * i;
      if (v >= n) continue;
      const AttnRow r(L, v);
      for (int cl = 0; cl < ck; ++cl) {
        const int c = c0 + cl;
        const float* Xc = L.X + cl * a.nmax * kAttnTile + lane;
        const float2* Wc = L.W + cl * a.nmax * kAttnSlots + v * kAttnSlots;
        float* Dc = Dw + cl * a.nmax * kAttnTile;
        const float g = L.G[(cl * a.nmax + v) * kAttnTile + lane];
        const float xv = Xc[v * kAttnTile];
        float2 w[KS];
        float xu[KS];
        attn_slots<KS>(Xc, Wc, r, w, xu);
        float qacc = 0.f;  // the query path: scale sum_j ds_j m_j
#pragma unroll
        for (int jj = 0; jj < KS; ++jj) {
          // wave-uniform; selects, not branches (WGT: per lane, the delivered entries)
          const bool used = WGT ? ((dmask[i] >> jj) & 1u) != 0u : jj < r.deg;
          const float msg = __fadd_rn(__fmul_rn(w[jj].x, xu[jj]), w[jj].y);
          float dm = __fmaf_rn(ds[i][jj], xv, __fmul_rn(at[i][jj], g));  // key path + value path
          dm = used ? dm : 0.f;
          qacc = used ? __fmaf_rn(ds[i][jj], msg, qacc) : qacc;
          if (want_dx) {
            // (gamma, dm) = (0, 0) past the row's end: the partial of node 0 is rewritten unchanged
            float* Du = Dc + r.src(jj) * kAttnTile;
            if constexpr (WGT)
              *Du = used ? __fmaf_rn(w[jj].x, dm, *Du) : *Du;
            else
              *Du = __fmaf_rn(w[jj].x, dm, *Du);
          }
          if (want_dgb) {
            float2 rsum = make_float2(wave_sum63(used ? __fmul_rn(xu[jj], dm) : 0.f), wave_sum63(dm));
            if (lane == 63 && jj < r.deg) {
              const int e = L.slot_e[v * kAttnSlots + jj];
              const int64_t off = ((int64_t)e * attn_gb_channels<MH>(m) + c) * 2;
              if (m.ntile > 1) {
                *reinterpret_cast<float2*>(m.ws + (int64_t)tile * m.E * attn_gb_channels<MH>(m) * 2 + off) = rsum;
              } else {
                if (a.logits) rsum = sigmoid_backward(rsum, *reinterpret_cast<const float2*>(a.gb + off));
                *reinterpret_cast<float2*>(a.dgb + off) = rsum;
              }
            }
          }
        }
        if (want_dx) Dc[v * kAttnTile] = __fadd_rn(Dc[v * kAttnTile], qacc);
      }
    }
    if (want_dx) {
      __syncthreads();
      // grad_x of the chunk: the four waves' partials in wave order, then the base.  Wave w writes the nodes
      // it staged (u = w, w + 4, ...).
      T* ob = static_cast<T*>(a.out) + (int64_t)node0 * a.os + (int64_t)c0 * a.P + p;
#pragma unroll
      for (int cl = 0; cl < CK; ++cl) {
#pragma unroll
        for (int i = 0; i < kAttnDpw; ++i) {
          const int u = wave + kAttnWaves * i;
          if (cl >= ck || u >= n) continue;
          const float* Dp = L.D + (cl * a.nmax + u) * kAttnTile + lane;
          Frag<1> o;
          o.v[0] = Dp[0];
#pragma unroll
          for (int w = 1; w < kAttnWaves; ++w) o.v[0] = __fadd_rn(o.v[0], Dp[w * CK * a.nmax * kAttnTile]);
          if (a.dxb != nullptr) o.v[0] = __fadd_rn(o.v[0], (float)base[cl * kAttnDpw + i]);
          if (pin) store_frag<1, true>(ob + (int64_t)u * a.os + (int64_t)cl * a.P, o);
        }
      }
    }
  }
}

}  // namespace mrp

namespace mrp_host {

using mrp::AttnArgs;
using mrp::WAttnArgs;

inline int attn_tiles(int32_t P) { return (P + mrp::kAttnTile - 1) / mrp::kAttnTile; }

inline int attn_bwd_chunk(int max_nodes) { return max_nodes <= 8 ? mrp::kAttnBwdChunkSmall : mrp::kAttnBwdChunk; }

inline size_t lds_attn(int nmax, int ck, bool bwd, bool weighted = false) {
  return (size_t)ck * nmax * mrp::kAttnTile * 4 * (bwd ? 2 + mrp::kAttnWaves : 1) +
         (size_t)ck * nmax * mrp::kAttnSlots * 8 + (size_t)nmax * 8 + (size_t)nmax * mrp::kAttnSlots * 4 +
         (size_t)nmax * 4 + (weighted ? (size_t)nmax * mrp::kAttnTile * 4 : 0);
}

// bytes of the backward's grad_gb workspace
inline int64_t attn_workspace_bytes(int32_t num_edges, int32_t C, int32_t P) {
  const int nt = attn_tiles(P);
  return nt > 1 ? (int64_t)nt * num_edges * C * 2 * (int64_t)sizeof(float) : 0;
}

// The argument checks the two entry points share (film_max's, plus the scale).
inline bool attn_common_ok(int32_t dtype, int32_t flags, const int32_t* indptr, const int32_t* src, const int32_t* eid,
                           const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                           int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, float scale) {
  if (dtype != MRP_DTYPE_F32 && dtype != MRP_DTYPE_BF16 && dtype != MRP_DTYPE_F16) return false;
  if (flags != 0 && flags != MRP_AGG_GB_LOGITS) return false;
  if (!common_args_ok(indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P,
                      MRP_AGG_FILM_MEAN))
    return false;
  if (MRP_GRAPH_IS_REGULAR(graph_kind) && MRP_GRAPH_REGULAR_K(graph_kind) > MRP_FILM_ATTN_DEGREE) return false;
  return scale == scale && scale - scale == 0.f;  // finite
}

// compiled slots per destination for the in-degree bound a graph kind gives (COMPLETE: n - 1, REGULAR(k): k,
// else the operator's limit)
inline int attn_slots_for(int32_t graph_kind, int32_t max_nodes) {
  const int maxdeg = graph_kind == MRP_GRAPH_COMPLETE
                         ? max_nodes - 1
                         : (MRP_GRAPH_IS_REGULAR(graph_kind) ? MRP_GRAPH_REGULAR_K(graph_kind) : MRP_FILM_ATTN_DEGREE);
  return maxdeg <= 4 ? 4 : (maxdeg <= 8 ? 8 : 16);
}

hipError_t launch_attn_bwd_f32(const AttnArgs& m, int ck, int ks, size_t lds, int64_t grid, hipStream_t st);
hipError_t launch_attn_bwd_bf16(const AttnArgs& m, int ck, int ks, size_t lds, int64_t grid, hipStream_t st);
hipError_t launch_attn_bwd_f16(const AttnArgs& m, int ck, int ks, size_t lds, int64_t grid, hipStream_t st);
// the confidence-gated instantiations (film_wattn_bwd*.hip)
hipError_t launch_wattn_bwd_f32(const WAttnArgs& m, int ck, int ks, size_t lds, int64_t grid, hipStream_t st);
hipError_t launch_wattn_bwd_bf16(const WAttnArgs& m, int ck, int ks, size_t lds, int64_t grid, hipStream_t st);
hipError_t launch_wattn_bwd_f16(const WAttnArgs& m, int ck, int ks, size_t lds, int64_t grid, hipStream_t st);
// film_attn_dgb_reduce (film_attn_bwd.hip) over `blocks` workgroups
hipError_t launch_attn_dgb_reduce(const AttnArgs& m, int64_t blocks, hipStream_t st);

// the multi-head instantiations (film_attn_mh_bwd*.hip); grid = graphs x tiles, the head factor is heads
hipError_t launch_attn_mh_bwd_f32(const mrp::AttnMhArgs<false>& m, int ck, int ks, size_t lds, int64_t grid, int heads,
                                  hipStream_t st);
hipError_t launch_attn_mh_bwd_bf16(const mrp::AttnMhArgs<false>& m, int ck, int ks, size_t lds, int64_t grid,
                                   int heads, hipStream_t st);
hipError_t launch_attn_mh_bwd_f16(const mrp::AttnMhArgs<false>& m, int ck, int ks, size_t lds, int64_t grid, int heads,
                                  hipStream_t st);
hipError_t launch_wattn_mh_bwd_f32(const mrp::AttnMhArgs<true>& m, int ck, int ks, size_t lds, int64_t grid, int heads,
                                   hipStream_t st);
hipError_t launch_wattn_mh_bwd_bf16(const mrp::AttnMhArgs<true>& m, int ck, int ks, size_t lds, int64_t grid,
                                    int heads, hipStream_t st);
hipError_t launch_wattn_mh_bwd_f16(const mrp::AttnMhArgs<true>& m, int ck, int ks, size_t lds, int64_t grid, int heads,
                                   hipStream_t st);
// the multi-head forwards (film_attn_mh_fwd.hip)
hipError_t launch_attn_mh_fwd(int32_t dtype, const mrp::AttnMhArgs<false>& m, int ks, size_t lds, int64_t grid,
                              int heads, hipStream_t st);
hipError_t launch_wattn_mh_fwd(int32_t dtype, const mrp::AttnMhArgs<true>& m, int ks, size_t lds, int64_t grid,
                               int heads, hipStream_t st);
// film_attn_gw_reduce (film_attn_mh_fwd.hip): grad_w (nodes, P), node stride gwst, from the heads' partials
hipError_t launch_attn_gw_reduce(const float* part, int heads, int32_t nodes, int32_t P, float* gw, int64_t gwst,
                                 hipStream_t st);

// the FP8-message forwards (film_attn_fwd_q.hip: WGT = false, film_wattn_fwd_q.hip: WGT = true); heads = 1 for the
// single-head argument blocks
hipError_t launch_attn_fwd_q(int32_t dtype, const mrp::AttnQArgs<false, false>& m, int ks, size_t lds, int64_t grid,
                             int heads, hipStream_t st);
hipError_t launch_attn_fwd_q(int32_t dtype, const mrp::AttnQArgs<false, true>& m, int ks, size_t lds, int64_t grid,
                             int heads, hipStream_t st);
hipError_t launch_attn_fwd_q(int32_t dtype, const mrp::AttnQArgs<true, false>& m, int ks, size_t lds, int64_t grid,
                             int heads, hipStream_t st);
hipError_t launch_attn_fwd_q(int32_t dtype, const mrp::AttnQArgs<true, true>& m, int ks, size_t lds, int64_t grid,
                             int heads, hipStream_t st);

template <typename T, bool WGT, bool MH>
hipError_t launch_attn_fwd_q_t(const mrp::AttnQArgs<WGT, MH>& m, int ks, size_t lds, int64_t grid, int heads,
                               hipStream_t st) {
  const dim3 g((unsigned)grid, (unsigned)heads), block(mrp::kBlock);
  if (ks == 4)
    hipLaunchKernelGGL((mrp::film_attn_fwd<T, 4, WGT, MH, mrp::q8_t>), g, block, lds, st, m);
  else if (ks == 8)
    hipLaunchKernelGGL((mrp::film_attn_fwd<T, 8, WGT, MH, mrp::q8_t>), g, block, lds, st, m);
  else
    hipLaunchKernelGGL((mrp::film_attn_fwd<T, 16, WGT, MH, mrp::q8_t>), g, block, lds, st, m);
  return hipGetLastError();
}

template <bool WGT, bool MH>
hipError_t launch_attn_fwd_q_dtype(int32_t dtype, const mrp::AttnQArgs<WGT, MH>& m, int ks, size_t lds, int64_t grid,
                                   int heads, hipStream_t st) {
  switch (dtype) {
    case MRP_DTYPE_F32: return launch_attn_fwd_q_t<float, WGT, MH>(m, ks, lds, grid, heads, st);
    case MRP_DTYPE_BF16: return launch_attn_fwd_q_t<mrp::bf16_t, WGT, MH>(m, ks, lds, grid, heads, st);
    default: return launch_attn_fwd_q_t<mrp::f16_t, WGT, MH>(m, ks, lds, grid, heads, st);
  }
}

// The forward both FP8-message entry points share (film_attn_fwd_q.hip); weighted: mrp_film_wattn_fwd_q.
int attn_fwd_q(bool weighted, int32_t qdtype, const void* xq, int64_t xq_node_stride, const float* x_scale,
               int32_t dtype, const void* query, int64_t query_node_stride, const float* gb, const float* w,
               int64_t w_node_stride, const int32_t* indptr, const int32_t* src, const int32_t* eid,
               const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind, int32_t num_nodes,
               int32_t num_edges, int32_t C, int32_t P, int32_t flags, int32_t heads, void* out,
               int64_t out_node_stride, float scale, float* attn, float* rate, int64_t workspace_bytes, void* stream);

constexpr int kMaxGridY = 65535;  // the head factor of the grid

// heads of a multi-head call: >= 1 and a divisor of C (C = 0: any)
inline bool attn_heads_ok(int32_t C, int32_t heads) { return heads >= 1 && (C <= 0 || C % heads == 0); }

// bytes of the multi-head backward's grad_w partials (H, nodes, P)
inline int64_t attn_gw_partial_bytes(int32_t heads, int32_t num_nodes, int32_t P) {
  return heads > 1 ? (int64_t)heads * num_nodes * P * (int64_t)sizeof(float) : 0;
}

template <typename T, bool WGT = false, bool MH = false>
hipError_t launch_attn_bwd(const mrp::AttnKernelArgs<WGT, MH>& m, int ck, int ks, size_t lds, int64_t grid,
                           hipStream_t st, int heads = 1) {
  const dim3 g((unsigned)grid, (unsigned)heads), block(mrp::kBlock);
#define MRP_ATTN_BWD(CK, KS) hipLaunchKernelGGL((mrp::film_attn_bwd<T, CK, KS, WGT, MH>), g, block, lds, st, m)
  if (ck == mrp::kAttnBwdChunkSmall) {  // <= 8 nodes: in-degree <= 8 for every kind but CSR / SIMPLE rows
    if (ks == 4)
      MRP_ATTN_BWD(mrp::kAttnBwdChunkSmall, 4);
    else if (ks == 8)
      MRP_ATTN_BWD(mrp::kAttnBwdChunkSmall, 8);
    else
      MRP_ATTN_BWD(mrp::kAttnBwdChunkSmall, 16);
  } else {
    if (ks == 4)
      MRP_ATTN_BWD(mrp::kAttnBwdChunk, 4);
    else if (ks == 8)
      MRP_ATTN_BWD(mrp::kAttnBwdChunk, 8);
    else
      MRP_ATTN_BWD(mrp::kAttnBwdChunk, 16);
  }
#undef MRP_ATTN_BWD
  return hipGetLastError();
}

}  // namespace mrp_host
