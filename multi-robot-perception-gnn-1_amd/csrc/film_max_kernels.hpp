#pragma once
// film_max_kernels.hpp — gfx950 kernels of the max-pooled FiLM aggregation (mrp_film_max_fwd / _bwd)
//
//   m_j[c,p]   = fl(fl(gamma_j[c] * x[u_j,c,p]) + beta_j[c])    j = 0, 1, ... over v's CSR row (edge-id order)
//   out[v,c,p] = max_j m_j[c,p]                                  torch.max(mailbox, 1): the first maximal
//                                                                entry wins, the first NaN beats everything
//
// Unlike the mean kernels' dense N x N tiles (which sum parallel edges into one weight), everything here
// works per CSR entry ("slot"): slot (v, j) is v's j-th in-edge, its (gamma, beta) for the workgroup's
// channels, its local source (4 bits) and its edge id sit in LDS.  A destination has at most
// MRP_FILM_MAX_DEGREE = 16 slots.  As in film_fwd_regular, a lane owns a slice of one channel plane, holds
// that slice of all n sources in NT-wide register vectors, and x_u is a wave-uniform dynamic extract.
// That extract is not free.  Only 16-wide vectors are indexed through s_set_gpr_idx; for 4- and 8-wide ones
// the compiler emits a chain of scalar compares and v_cndmask selects per extracted element
// (film_max_fwd<8, 4, float> with 8-wide vectors: 1028 v_cndmask_b32 against 103 v_mul_f32 and 98 v_add_f32,
// no s_set_gpr_idx; with 16-wide ones: 132 v_cndmask_b32, 104 s_set_gpr_idx_on).  The forward therefore holds
// 16-wide vectors whatever NT, except at 8-element slices (16-bit features, <= 8 nodes: 128 registers).  The
// backward cannot: with 16-wide x and grad_x vectors the fused 8-node kernel spills (228 B/lane), so its
// extracts and its dynamic inserts stay select chains (film_max_bwd<8, 8, 8, true, 2, float>: 4084
// v_cndmask_b32, 2522 s_cselect_b64, 2378 s_cmp_eq_u32 against 1259 v_mul_f32), and it is bound by them, not
// by HBM; compile-time sources for COMPLETE graphs would remove them.
//
// The backward stores no argmax: it recomputes the winner from x, gamma and beta with the forward's own
// unfused arithmetic and comparison, so the selection matches the forward bit for bit.  Gradients follow
// torch's autograd of max: the winner's slot receives G, every other slot an exact zero, and each slot's
// term is gamma * sel (grad_x), x * sel (d gamma), sel (d beta) — a product with zero, not a skip, so
// non-finite operands propagate as they do in autograd.  No atomics: grad_x is accumulated in registers
// in slot order, d gamma / d beta as per-lane partial sums reduced by a fixed butterfly.

#include "film_mean_kernels.hpp"

namespace mrp {

constexpr int kMaxSlots = MRP_FILM_MAX_DEGREE;  // LDS slot stride per destination

struct MaxArgs {
  AggArgs a;         // the mean kernels' argument block (fwd: out = the aggregate; bwd: out = grad_x)
  int32_t complete;  // MRP_GRAPH_COMPLETE: slots and edge ids are arithmetic, every graph has a.nmax nodes
  int32_t nvb;       // backward: destination blocks per graph (grid = graphs x channel blocks x nvb)
};

// LDS of one workgroup: per channel the slots' (gamma, beta), then the channel-independent tables.
template <int NT>
struct MaxLds {
  static constexpr int NS = NT * kMaxSlots;
  static constexpr int WS = NS + 2;  // float2 per channel, padded 4 banks (as film_fwd_regular)
  float2* W;                         // [cpb][WS]
  int* slot_e;                       // [NS] edge id, -1: no such slot
  unsigned long long* slot_u;        // [NT] the row's local sources, 4 bits each, slot 0 lowest
  int* rowlen;                       // [NT]
  __device__ __forceinline__ MaxLds(void* smem, int cpb) {
    W = reinterpret_cast<float2*>(smem);
    slot_u = reinterpret_cast<unsigned long long*>(W + cpb * WS);
    slot_e = reinterpret_cast<int*>(slot_u + NT);
    rowlen = slot_e + NS;
  }
};

// The two prologue rounds.  Tables first (row lengths, sources, edge ids: the CSR walk's dependent loads),
// then one gamma/beta load per (channel, used slot).  Ends with the barrier that publishes the weights.
template <int NT>
__device__ __forceinline__ void max_prologue(const MaxArgs& m, const MaxLds<NT>& L, int b, int node0, int n, int c0) {
  const AggArgs& a = m.a;
  const int tid = threadIdx.x, nth = blockDim.x;
  for (int v = tid; v < NT; v += nth) {
    int beg = 0, deg = 0;
    if (v < n) {
      if (m.complete) {
        deg = n - 1;
      } else {
        beg = a.kdeg > 0 ? (node0 + v) * a.kdeg : a.indptr[node0 + v];
        const int end = a.kdeg > 0 ? beg + a.kdeg : a.indptr[node0 + v + 1];
        deg = min(max(end - beg, 0), kMaxSlots);  // precondition: in-degree <= 16 (clamped: in-bounds anyway)
      }
    }
    const int ebase = b * n * (n - 1);
    unsigned long long word = 0ull;
    for (int j = 0; j < kMaxSlots; ++j) {
      int u = 0, e = -1;
      if (j < deg) {
        if (m.complete) {
          u = j < v ? j : j + 1;  // v's in-edges in edge-id order: ascending source
          e = ebase + u * (n - 1) + (v < u ? v : v - 1);
        } else {
          u = a.src[beg + j] - node0;
          if ((unsigned)u >= (unsigned)n) u = 0;  // rejected on the host; keeps the register index in bounds
          e = a.eid[beg + j];
        }
      }
      word |= (unsigned long long)u << (4 * j);
      L.slot_e[v * kMaxSlots + j] = e;
    }
    L.slot_u[v] = word;
    L.rowlen[v] = deg;
  }
  __syncthreads();
  // slots in use per destination (wave-uniform bound of the item loop below)
  const int ksu = m.complete ? max(n - 1, 1) : (a.kdeg > 0 ? min(a.kdeg, kMaxSlots) : kMaxSlots);
  const int nitem = a.cpb * n * ksu;
  for (int t = tid; t < nitem; t += nth) {
    int cl, rest;
    split_channel(a, t, cl, rest);  // channel fastest: neighbouring lanes read neighbouring pairs
    const int v = rest / ksu, j = rest - v * ksu;
    const int slot = v * kMaxSlots + j;
    const int e = L.slot_e[slot];
    const int c = c0 + cl;
    float2 w = make_float2(0.f, 0.f);
    if (e >= 0 && c < a.C) {
      w = *reinterpret_cast<const float2*>(a.gb + ((int64_t)e * a.C + c) * 2);
      if (a.logits) w = make_float2(sigmoidf(w.x), sigmoidf(w.y));
    }
    L.W[cl * MaxLds<NT>::WS + slot] = w;
  }
  __syncthreads();
}

// torch.max's update: a message replaces the running maximum unless it is <= it, and nothing replaces a NaN.
__device__ __forceinline__ bool max_takes(float msg, float best) { return !(msg <= best) && best == best; }

template <int NT>
struct MaxVec {
  typedef float type __attribute__((ext_vector_type(NT <= 4 ? 4 : (NT <= 8 ? 8 : 16))));
};

// ---------------------------------------------------------------------------
// Forward.  Workgroup = graph x channel block x plane segment, as film_fwd.
// NT: compiled node capacity (4, 8 or 16); the graph's node count n <= NT is wave-uniform at run time.
// ---------------------------------------------------------------------------
// TX: the storage type of the gathered input x alone (out keeps T).  TX = q8_t: FP8 messages, widened and scaled in
// load_frag (a.qfmt, a.xscale) as in film_fwd; the arithmetic from there on is TX = T's (mrp_film_max_fwd_q).
template <int NT, int VEC, typename T, typename TX = T>
__global__ void __launch_bounds__(kBlock) film_max_fwd(MaxArgs m) {
  constexpr bool kQ = std::is_same<TX, q8_t>::value;
  const AggArgs& a = m.a;
  constexpr int WS = MaxLds<NT>::WS;
  extern __shared__ float4 smem_f4[];
  const MaxLds<NT> L(smem_f4, a.cpb);

  const int ps = a.psplit > 1 ? a.psplit : 1;
  const int item = blockIdx.x / ps;
  const int seg = blockIdx.x - item * ps;
  const int b = item / a.ncb;
  const int cb = item - b * a.ncb;
  const int seglen = (a.PV + ps - 1) / ps;
  const int jbeg = seg * seglen;
  const int jend = min(a.PV, jbeg + seglen);
  const int node0 = m.complete ? b * a.nmax : a.goff[b];
  const int n = m.complete ? a.nmax : min(a.goff[b + 1] - node0, NT);
  if (n <= 0) return;  // whole workgroup: empty graph
  const int c0 = cb * a.cpb;

  const int grp = threadIdx.x / a.lpc;
  const int li = threadIdx.x - grp * a.lpc;
  const int c = c0 + grp;
  const bool active = grp < a.cpb && c < a.C;
  const TX* xb = static_cast<const TX*>(a.x) + (int64_t)node0 * a.xs + (int64_t)c0 * a.P;
  T* ob = static_cast<T*>(a.out) + (int64_t)node0 * a.os + (int64_t)c0 * a.P;
  const uint32_t lane_plane = (uint32_t)grp * (uint32_t)a.P * (uint32_t)sizeof(T);
  const uint32_t lane_plane_x = (uint32_t)grp * (uint32_t)a.P * (uint32_t)sizeof(TX);
  // FP8 messages: the scales of this lane's channel for the graph's nodes, read once per workgroup
  float xsc[kQ ? NT : 1];
  if constexpr (kQ) {
#pragma unroll
    for (int u = 0; u < NT; ++u)
      xsc[u] = (active && u < n && a.xscale != nullptr) ? a.xscale[(int64_t)(node0 + u) * a.C + c] : 1.f;
  }

  // 16-wide register vectors whatever NT (up to 4-element slices: 64 registers): only those are indexed
  // through s_set_gpr_idx; an 8-wide vector's extract becomes a chain of 8 selects per element (header comment)
  typedef float vfw __attribute__((ext_vector_type(VEC <= 4 ? 16 : (NT <= 4 ? 4 : 8))));
  vfw xs[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) xs[k] = 0.f;
  auto load_slice = [&](int jj) {
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      if (u >= n) break;  // wave-uniform
      const TX* px = at_bytes(xb + (int64_t)u * a.xs, lane_plane_x + (uint32_t)jj * VEC * (uint32_t)sizeof(TX));
      Frag<VEC> f;
      if constexpr (kQ)
        f = load_frag<VEC, true>(px, a.qfmt, xsc[u]);
      else
        f = load_frag<VEC, true>(px);
#pragma unroll
      for (int k = 0; k < VEC; ++k) xs[k][u] = f.v[k];
    }
  };
  // the first slice's loads are in flight under the prologue's dependent loads
  int j = jbeg + li;
  if (active && j < jend) load_slice(j);
  max_prologue<NT>(m, L, b, node0, n, c0);
  if (!active) return;

  while (j < jend) {
    const uint32_t lane_off = lane_plane + (uint32_t)j * VEC * (uint32_t)sizeof(T);
#pragma unroll
    for (int v = 0; v < NT; ++v) {
      if (v >= n) break;
      int wbase = grp * WS + v * kMaxSlots;  // laundered: the weights stay in LDS (broadcast reads)
      asm volatile("" : "+v"(wbase));
      const float2* Wc = L.W + wbase;
      const int deg = __builtin_amdgcn_readfirstlane(L.rowlen[v]);
      const unsigned long long uw = L.slot_u[v];
      const unsigned ulo = __builtin_amdgcn_readfirstlane((unsigned)uw);
      const unsigned uhi = __builtin_amdgcn_readfirstlane((unsigned)(uw >> 32));
      Frag<VEC> best;
#pragma unroll
      for (int k = 0; k < VEC; ++k) best.v[k] = 0.f;  // empty row: zeros
#pragma unroll
      for (int jj = 0; jj < kMaxSlots; ++jj) {
        if (jj >= deg) break;  // wave-uniform
        const int u = ((jj < 8 ? ulo : uhi) >> (4 * (jj & 7))) & 15u;
        const float2 w = Wc[jj];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float msg = __fadd_rn(__fmul_rn(w.x, xs[k][u]), w.y);
          if (jj == 0 || max_takes(msg, best.v[k])) best.v[k] = msg;
        }
      }
      store_frag<VEC, true>(at_bytes(ob + (int64_t)v * a.os, lane_off), best);
    }
    j += a.lpc;
    if (j < jend) load_slice(j);
  }
}

// ---------------------------------------------------------------------------
// Backward.  Workgroup = graph x channel block x block of VB destinations [v0, v0 + VB); a lane sweeps its
// slices of the whole plane (no plane split: the d gamma / d beta sums of a slot end in one workgroup).
//   DGB  : per-lane partial sums of d gamma / d beta for the block's VB x KS slots (2 VB KS registers),
//          reduced over the plane's lanes at the end (lpc <= 64: one wave) and written by lane 0.
//   VB == NT: the block is the whole graph and grad_x (+ grad_x_base) is written too (a.want_dx).
// KS: compiled slots per destination (rows are clamped to it; the launcher picks KS >= the graph kind's
// in-degree bound).  The launcher keeps VB * KS <= 64 where DGB, so no instantiation spills.
// ---------------------------------------------------------------------------
template <int NT, int VB, int KS, bool DGB, int VEC, typename T>
__global__ void __launch_bounds__(kBlock, 2) film_max_bwd(MaxArgs m) {  // >= 2 waves per SIMD: <= 256 registers
  static_assert(KS <= kMaxSlots && VB <= NT, "slot and block bounds");
  const AggArgs& a = m.a;
  constexpr int WS = MaxLds<NT>::WS;
  constexpr bool DX = VB == NT;
  extern __shared__ float4 smem_f4[];
  const MaxLds<NT> L(smem_f4, a.cpb);

  const int item = blockIdx.x / m.nvb;
  const int v0 = (blockIdx.x - item * m.nvb) * VB;
  const int b = item / a.ncb;
  const int cb = item - b * a.ncb;
  const int node0 = m.complete ? b * a.nmax : a.goff[b];
  const int n = m.complete ? a.nmax : min(a.goff[b + 1] - node0, NT);
  if (n <= 0 || v0 >= n) return;  // whole workgroup
  const int c0 = cb * a.cpb;

  const int grp = threadIdx.x / a.lpc;
  const int li = threadIdx.x - grp * a.lpc;
  const int c = c0 + grp;
  const bool active = grp < a.cpb && c < a.C;
  const T* xb = static_cast<const T*>(a.x) + (int64_t)node0 * a.xs + (int64_t)c0 * a.P;
  const T* gbase = static_cast<const T*>(a.g) + (int64_t)node0 * a.gs + (int64_t)c0 * a.P;
  const uint32_t lane_plane = (uint32_t)grp * (uint32_t)a.P * (uint32_t)sizeof(T);
  const bool want_dx = DX && a.want_dx;

  typedef typename MaxVec<NT>::type vnt;
  vnt xs[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) xs[k] = 0.f;
  auto load_slice = [&](int jj) {
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      if (u >= n) break;
      const Frag<VEC> f = load_frag<VEC, true>(
          at_bytes(xb + (int64_t)u * a.xs, lane_plane + (uint32_t)jj * VEC * (uint32_t)sizeof(T)));
#pragma unroll
      for (int k = 0; k < VEC; ++k) xs[k][u] = f.v[k];
    }
  };
  int j = li;
  if (active && j < a.PV) load_slice(j);
  max_prologue<NT>(m, L, b, node0, n, c0);
  if (!active) return;

  float pg[DGB ? VB : 1][DGB ? KS : 1], pb[DGB ? VB : 1][DGB ? KS : 1];
  if constexpr (DGB) {
#pragma unroll
    for (int i = 0; i < VB; ++i)
#pragma unroll
      for (int jj = 0; jj < KS; ++jj) pg[i][jj] = pb[i][jj] = 0.f;
  }

  while (j < a.PV) {
    const uint32_t lane_off = lane_plane + (uint32_t)j * VEC * (uint32_t)sizeof(T);
    vnt dacc[DX ? VEC : 1];
    if constexpr (DX) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) dacc[k] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < VB; ++i) {
      const int v = v0 + i;
      if (v >= n) break;  // wave-uniform
      const Frag<VEC> G = load_frag<VEC, true>(at_bytes(gbase + (int64_t)v * a.gs, lane_off));
      int wbase = grp * WS + v * kMaxSlots;
      asm volatile("" : "+v"(wbase));
      const float2* Wc = L.W + wbase;
      // (the slot loops below skip, not leave, at the row's end: an early exit is merged with the loop's own
      // into a run-time trip count, the loop stays rolled, and the partial sums are then indexed in scratch)
      const int deg = __builtin_amdgcn_readfirstlane(L.rowlen[v]);
      const unsigned long long uw = L.slot_u[v];
      const unsigned ulo = __builtin_amdgcn_readfirstlane((unsigned)uw);
      const unsigned uhi = __builtin_amdgcn_readfirstlane((unsigned)(uw >> 32));
      // pass 1: the forward's selection, recomputed (same unfused message, same comparison)
      float best[VEC];
      int win[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        best[k] = 0.f;
        win[k] = 0;
      }
#pragma unroll
      for (int jj = 0; jj < KS; ++jj) {
        if (jj >= deg) continue;  // wave-uniform
        const int u = ((jj < 8 ? ulo : uhi) >> (4 * (jj & 7))) & 15u;
        const float2 w = Wc[jj];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float msg = __fadd_rn(__fmul_rn(w.x, xs[k][u]), w.y);
          if (jj == 0 || max_takes(msg, best[k])) {
            best[k] = msg;
            win[k] = jj;
          }
        }
      }
      // pass 2: every slot's terms in slot order; sel is G at the winner and an exact zero elsewhere
#pragma unroll
      for (int jj = 0; jj < KS; ++jj) {
        if (jj >= deg) continue;
        const int u = ((jj < 8 ? ulo : uhi) >> (4 * (jj & 7))) & 15u;
        const float2 w = Wc[jj];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float sel = win[k] == jj ? G.v[k] : 0.f;
          if constexpr (DX) {
            if (want_dx) dacc[k][u] = __fadd_rn(dacc[k][u], __fmul_rn(w.x, sel));
          }
          if constexpr (DGB) {
            pg[i][jj] = __fadd_rn(pg[i][jj], __fmul_rn(xs[k][u], sel));
            pb[i][jj] = __fadd_rn(pb[i][jj], sel);
          }
        }
      }
    }
    if constexpr (DX) {
      if (want_dx) {
        T* ob = static_cast<T*>(a.out) + (int64_t)node0 * a.os + (int64_t)c0 * a.P;
        const T* bb = a.dxb != nullptr ? static_cast<const T*>(a.dxb) + (int64_t)node0 * a.dxbs + (int64_t)c0 * a.P
                                       : nullptr;
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          if (u >= n) break;
          Frag<VEC> o;
#pragma unroll
          for (int k = 0; k < VEC; ++k) o.v[k] = dacc[k][u];
          if (bb != nullptr) {
            const Frag<VEC> base = load_frag<VEC, true>(at_bytes(bb + (int64_t)u * a.dxbs, lane_off));
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = __fadd_rn(o.v[k], base.v[k]);
          }
          store_frag<VEC, true>(at_bytes(ob + (int64_t)u * a.os, lane_off), o);
        }
      }
    }
    j += a.lpc;
    if (j < a.PV) load_slice(j);
  }

  if constexpr (DGB) {
    // the plane's lanes sit in one wave (lpc <= 64): a fixed butterfly, every lane ends with the sum
    with_lanes(a.lpc, [&](auto lanes) {
      constexpr int LN = decltype(lanes)::value;
#pragma unroll
      for (int i = 0; i < VB; ++i) {
        // (no early exits here: the cross-lane moves keep these loops from unrolling past one, and the
        // partial sums would then be indexed in scratch; unused slots hold zeros and are summed unstored)
        const int v = v0 + i;
        const int deg = v < n ? min(__builtin_amdgcn_readfirstlane(L.rowlen[v < NT ? v : 0]), KS) : 0;
#pragma unroll
        for (int jj = 0; jj < KS; ++jj) {
          float2 r = make_float2(group_sum<LN>(pg[i][jj]), group_sum<LN>(pb[i][jj]));
          if (li == 0 && jj < deg) {
            const int e = L.slot_e[v * kMaxSlots + jj];
            const int64_t off = ((int64_t)e * a.C + c) * 2;
            if (a.logits) r = sigmoid_backward(r, *reinterpret_cast<const float2*>(a.gb + off));
            *reinterpret_cast<float2*>(a.dgb + off) = r;
          }
        }
      }
    });
  }
}

}  // namespace mrp

namespace mrp_host {

using mrp::MaxArgs;

// compiled node capacity of a graph size
inline int max_bucket(int max_nodes) { return max_nodes <= 4 ? 4 : (max_nodes <= 8 ? 8 : 16); }

inline size_t lds_max(int nt, int cpb) {
  const int ns = nt * mrp::kMaxSlots;
  return (size_t)cpb * (ns + 2) * sizeof(float2) + (size_t)nt * 8 + (size_t)ns * 4 + (size_t)nt * 4;
}

// The backward's launches (film_max_bwd.hip plans, the per-dtype units launch).
struct MaxBwdPlan {
  Geometry g;        // vec, lpc, cpb, threads, ncb, lds
  int bucket = 0;    // NT
  int fused = 0;     // one launch writes both outputs (VB == NT with DGB)
  int ks = 0;        // fused / block pass: compiled slots per destination (8 or 16)
  int nvb = 1;       // block pass: destination blocks of 4
  int run_dx = 0;    // launch the grad_x-only kernel
  int run_dgb = 0;   // launch the destination-block kernel
};

hipError_t launch_max_bwd_f32(const MaxArgs& m, const MaxBwdPlan& p, hipStream_t st);
hipError_t launch_max_bwd_bf16(const MaxArgs& m, const MaxBwdPlan& p, hipStream_t st);
hipError_t launch_max_bwd_f16(const MaxArgs& m, const MaxBwdPlan& p, hipStream_t st);

// The launches of a plan for feature type T.
template <typename T>
hipError_t launch_max_bwd(MaxArgs m, const MaxBwdPlan& p, hipStream_t st) {
  const Geometry& g = p.g;
  const size_t lds = g.lds;
  const int64_t items = g.grid;  // graphs x channel blocks
#define MRP_MAX_BWD(NT, VB, KS, DGB, NVB)                                                                      \
  do {                                                                                                         \
    m.nvb = (NVB);                                                                                             \
    const dim3 grid((unsigned)(items * (NVB)));                                                                \
    if (g.vec == 4)                                                                                            \
      hipLaunchKernelGGL((mrp::film_max_bwd<NT, VB, KS, DGB, 4, T>), grid, dim3(g.threads), lds, st, m);       \
    else                                                                                                       \
      hipLaunchKernelGGL((mrp::film_max_bwd<NT, VB, KS, DGB, 1, T>), grid, dim3(g.threads), lds, st, m);       \
  } while (0)
  if (p.fused) {
    // 2-element slices at most: with 4 the partial sums, x slices and grad_x accumulators pass 256 registers
    m.nvb = 1;
    const dim3 grid((unsigned)items), block(g.threads);
    if (p.bucket == 4 && g.vec == 2)
      hipLaunchKernelGGL((mrp::film_max_bwd<4, 4, 16, true, 2, T>), grid, block, lds, st, m);
    else if (p.bucket == 4 && g.vec == 1)
      hipLaunchKernelGGL((mrp::film_max_bwd<4, 4, 16, true, 1, T>), grid, block, lds, st, m);
    else if (p.bucket == 8 && p.ks == 8 && g.vec == 2)
      hipLaunchKernelGGL((mrp::film_max_bwd<8, 8, 8, true, 2, T>), grid, block, lds, st, m);
    else if (p.bucket == 8 && p.ks == 8 && g.vec == 1)
      hipLaunchKernelGGL((mrp::film_max_bwd<8, 8, 8, true, 1, T>), grid, block, lds, st, m);
    else
      return hipErrorInvalidValue;
    return hipGetLastError();
  }
  if (p.run_dx) {
    if (p.bucket == 4)
      MRP_MAX_BWD(4, 4, 16, false, 1);
    else if (p.bucket == 8)
      MRP_MAX_BWD(8, 8, 16, false, 1);
    else
      MRP_MAX_BWD(16, 16, 16, false, 1);
  }
  if (p.run_dgb) {
    if (p.bucket == 8)
      MRP_MAX_BWD(8, 4, 16, true, p.nvb);
    else if (p.bucket == 16)
      MRP_MAX_BWD(16, 4, 16, true, p.nvb);
    else
      return hipErrorInvalidValue;
  }
#undef MRP_MAX_BWD
  return hipGetLastError();
}

}  // namespace mrp_host
