#pragma once
// film_wmean_kernels.hpp — gfx950 kernels of the confidence-weighted FiLM aggregation
// (mrp_film_wmean_fwd / _bwd): every sender u attaches a per-pixel map w[u,p] >= 0 to its feature map and
// the receiver averages, pixel by pixel, over what was delivered there.
//
//   m_{vu}[c,p] = fl(fl(Gamma[v][u][c] * x[u,c,p]) + Beta[v][u][c])     Gamma/Beta: the mean's dense tiles
//   acc[v,c,p]  = sum over v's sources u ascending  fl(acc + fl(w[u,p] * m_{vu}[c,p]))
//   D[v,p]      = sum over v's sources u ascending  fl(D + fl(cnt[v][u] * w[u,p]))   cnt: edges u -> v
//   out         = D > 0 ? acc / D : 0  (MEAN),  acc  (SUM)
//
// The arithmetic is the mean forward's (film_fwd) with one more product per message, on the same tiles in
// the same order, so w == 1 reproduces film_mean / film_sum bit for bit on every graph (fl(1 * m) = m, D the
// exact in-degree).  Like the mean, parallel edges u -> v are one tile entry (their gammas and betas summed in
// CSR order); with rows in ascending source order and no parallel edges this is the row-order sum of the
// header's definition.
//
// Three layouts:
//   * forward: the mean's.  Workgroup = graph x channel block x plane segment, a lane owns one channel and
//     slices of its plane, holds that slice of x and of w for the graph's nodes in registers; D is formed per
//     lane.  The w slices are the same for every channel group of the workgroup (cache hits after the first).
//   * grad_x and grad_w (film_wmean_bwd_xw): a lane owns a pixel slice and walks the workgroup's channels in
//     order, so grad_w's sum over channels is a register sum in channel order: no cross-lane step, no LDS
//     reduction.  A workgroup covers at most kWChanBlock channels (their tiles sit in LDS); with more channels
//     each block writes its partial to the workspace and film_wmean_dw_reduce adds them in block order.
//   * grad_gb (film_wmean_bwd_gb): the mean's again, per block of 4 destinations: per-lane partial sums of
//     every (destination, source) pair, one fixed butterfly over the plane's lanes, then each CSR entry of the
//     pair receives the pair's sums (parallel edges have equal gradients).
// No atomics, one writer per output element.  The backward recomputes `out` from its inputs.

#include "film_mean_kernels.hpp"

namespace mrp {

constexpr int kWChanBlock = 16;  // film_wmean_bwd_xw: channels per workgroup
constexpr int kWDestBlock = 4;   // film_wmean_bwd_gb: destinations per workgroup

struct WArgs {
  AggArgs a;         // the mean kernels' argument block (fwd: out = the aggregate; bwd: out = grad_x)
  const float* w;    // (num_nodes, P) sender maps, node stride ws
  int64_t ws;
  float* dw;         // bwd: grad_w, or the per-channel-block partials [ncb][num_nodes][P]
  int64_t dws;       // node stride of dw
  int64_t dwbs;      // channel-block stride of dw (0: grad_w itself)
  int32_t complete;  // MRP_GRAPH_COMPLETE: edge ids are arithmetic, every graph has a.nmax nodes
  int32_t mean;      // MRP_WAGG_MEAN (else MRP_WAGG_SUM)
  int32_t nvb;       // film_wmean_bwd_gb: destination blocks per graph
  int32_t nseg;      // film_wmean_bwd_xw: plane segments per (graph, channel block)
  int32_t want_dw;
};

// LDS of one workgroup: the mean forward's tiles [cpb][v][u], then the channel-independent tables.
template <int NT>
struct WLds {
  static constexpr int SZ = Tile<NT>::SZ;
  static constexpr int NTP = Tile<NT>::NTP;
  float* Ga;        // [cpb][SZ] sum of gamma over edges u -> v
  float* Gb;        // [cpb][SZ] sum of beta
  float* cnt;       // [NT][NTP] edges u -> v
  unsigned* emask;  // [NT] source bits of v
  float* extra;     // what follows (film_wmean_bwd_gb: the reduced sums)
  __device__ __forceinline__ WLds(void* smem, int cpb_tiles) {
    Ga = reinterpret_cast<float*>(smem);
    Gb = Ga + cpb_tiles * SZ;
    cnt = Gb + cpb_tiles * SZ;
    emask = reinterpret_cast<unsigned*>(cnt + NT * NTP);
    extra = reinterpret_cast<float*>(emask + NTP);
  }
};

// Prologue: tiles and tables of graph b.  Each (channel, destination) row is built by one thread walking the
// destination's in-edges in CSR order (COMPLETE: ascending source), as build_tiles_csr does, so the tile
// values are the mean's bits.  film = false: the tables only.  The caller's barrier publishes them.
template <int NT>
__device__ __forceinline__ void wmean_tiles(const WArgs& m, const WLds<NT>& L, int b, int node0, int n, int c0,
                                            bool film) {
  constexpr int SZ = Tile<NT>::SZ;
  constexpr int NTP = Tile<NT>::NTP;
  const AggArgs& a = m.a;
  const int tid = threadIdx.x, nth = blockDim.x;
  if (film) {
    for (int i = tid; i < a.cpb * SZ; i += nth) L.Ga[i] = L.Gb[i] = 0.f;
  }
  for (int i = tid; i < NT * NTP; i += nth) L.cnt[i] = 0.f;
  __syncthreads();
  for (int t = tid; t < a.cpb * NT; t += nth) {
    int cl, v;
    split_channel(a, t, cl, v);
    const int c = c0 + cl;
    const bool tab = cl == 0;
    const bool tiles = film && c < a.C;
    if (!tab && !tiles) continue;
    unsigned mask = 0u;
    if (v < n) {
      float* ga = L.Ga + cl * SZ + v * NTP;
      float* gbt = L.Gb + cl * SZ + v * NTP;
      float* cn = L.cnt + v * NTP;
      if (m.complete) {
        const int64_t ebase = (int64_t)b * n * (n - 1);
        for (int u = 0; u < n; ++u) {
          if (u == v) continue;
          if (tiles) {
            float2 g = *reinterpret_cast<const float2*>(a.gb + (complete_eid(ebase, n, u, v) * a.C + c) * 2);
            if (a.logits) g = make_float2(sigmoidf(g.x), sigmoidf(g.y));
            ga[u] = g.x;
            gbt[u] = g.y;
          }
          if (tab) cn[u] = 1.f;
          mask |= 1u << u;
        }
      } else {
        const int beg = a.kdeg > 0 ? (node0 + v) * a.kdeg : a.indptr[node0 + v];
        const int end = a.kdeg > 0 ? beg + a.kdeg : a.indptr[node0 + v + 1];
        for (int k = beg; k < end; ++k) {
          const int u = a.src[k] - node0;
          if ((unsigned)u >= (unsigned)n) continue;  // leaves the graph: rejected on the host, skipped here
          if (tiles) {
            float2 g = *reinterpret_cast<const float2*>(a.gb + ((int64_t)a.eid[k] * a.C + c) * 2);
            if (a.logits) g = make_float2(sigmoidf(g.x), sigmoidf(g.y));
            ga[u] += g.x;
            gbt[u] += g.y;
          }
          if (tab) cn[u] += 1.f;
          mask |= 1u << u;
        }
      }
    }
    if (tab) L.emask[v] = mask;
  }
}

// D[v] of one slice: the delivered weight, sources ascending (the same chain in every kernel).
template <int NT, int VEC>
__device__ __forceinline__ void wmean_norm(const float* cn, unsigned em, const float (&wv)[NT][VEC], float (&D)[VEC]) {
#pragma unroll
  for (int k = 0; k < VEC; ++k) D[k] = 0.f;
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    if (!((em >> u) & 1u)) continue;  // wave-uniform
    const float cu = cn[u];
#pragma unroll
    for (int k = 0; k < VEC; ++k) D[k] = __fadd_rn(D[k], __fmul_rn(cu, wv[u][k]));
  }
}

// A pixel nobody delivered to (D = 0) gives 0; a NaN in D stays one.
__device__ __forceinline__ float wmean_div(float num, float D) { return !(D <= 0.f) ? num / D : 0.f; }

// ---------------------------------------------------------------------------
// Forward.  Workgroup = graph x channel block x plane segment, as film_fwd.  NT: compiled node capacity
// (4, 8 or 16); the graph's node count n <= NT is wave-uniform at run time.
// ---------------------------------------------------------------------------
template <int NT, int VEC, typename T>
__global__ void __launch_bounds__(kBlock) film_wmean_fwd(WArgs m) {
  const AggArgs& a = m.a;
  constexpr int SZ = Tile<NT>::SZ;
  constexpr int NTP = Tile<NT>::NTP;
  extern __shared__ float4 smem_f4[];
  const WLds<NT> L(smem_f4, a.cpb);

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
  const T* xb = static_cast<const T*>(a.x) + (int64_t)node0 * a.xs + (int64_t)c0 * a.P;
  T* ob = static_cast<T*>(a.out) + (int64_t)node0 * a.os + (int64_t)c0 * a.P;
  const float* wb = m.w + (int64_t)node0 * m.ws;
  const uint32_t lane_plane = (uint32_t)grp * (uint32_t)a.P * (uint32_t)sizeof(T);

  float xv[NT][VEC], wv[NT][VEC];
#pragma unroll
  for (int u = 0; u < NT; ++u)
#pragma unroll
    for (int k = 0; k < VEC; ++k) xv[u][k] = wv[u][k] = 0.f;
  auto load_slice = [&](int jj) {
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      if (u < n) {  // wave-uniform
        const Frag<VEC> f = load_frag<VEC, true>(
            at_bytes(xb + (int64_t)u * a.xs, lane_plane + (uint32_t)jj * VEC * (uint32_t)sizeof(T)));
        const Frag<VEC> fw =
            load_frag<VEC, false>(at_bytes(wb + (int64_t)u * m.ws, (uint32_t)jj * VEC * (uint32_t)sizeof(float)));
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          xv[u][k] = f.v[k];
          wv[u][k] = fw.v[k];
        }
      }
    }
  };
  // the first slice's loads are in flight under the prologue's dependent loads
  int j = jbeg + li;
  if (active && j < jend) load_slice(j);
  wmean_tiles<NT>(m, L, b, node0, n, c0, true);
  __syncthreads();
  if (!active) return;

  unsigned emv[NT];
#pragma unroll
  for (int v = 0; v < NT; ++v) emv[v] = __builtin_amdgcn_readfirstlane(L.emask[v]);

  while (j < jend) {
    const uint32_t lane_off = lane_plane + (uint32_t)j * VEC * (uint32_t)sizeof(T);
    int tile = grp * SZ;  // laundered: the weights stay in LDS (broadcast reads), as in film_fwd
    asm volatile("" : "+v"(tile));
    const float* A = L.Ga + tile;
    const float* Bt = L.Gb + tile;
#pragma unroll
    for (int v = 0; v < NT; ++v) {
      if (v < n) {
        const unsigned em = emv[v];
        Frag<VEC> acc;
        float D[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = D[k] = 0.f;
#pragma unroll
        for (int u4 = 0; u4 < NTP; u4 += 4) {
          if (((em >> u4) & 15u) == 0u) continue;  // no source in this quad: skip its LDS reads
          const f4 wa = *reinterpret_cast<const f4*>(A + v * NTP + u4);
          const f4 wbt = *reinterpret_cast<const f4*>(Bt + v * NTP + u4);
          const f4 wc = *reinterpret_cast<const f4*>(L.cnt + v * NTP + u4);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int u = u4 + q;
            if (u >= NT) break;
            if (!((em >> u) & 1u)) continue;  // not a source of v: never touched
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
              const float msg = __fadd_rn(__fmul_rn(wa[q], xv[u][k]), wbt[q]);
              acc.v[k] = __fadd_rn(acc.v[k], __fmul_rn(wv[u][k], msg));
              D[k] = __fadd_rn(D[k], __fmul_rn(wc[q], wv[u][k]));
            }
          }
        }
        if (m.mean) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc.v[k] = wmean_div(acc.v[k], D[k]);
        }
        store_frag<VEC, true>(at_bytes(ob + (int64_t)v * a.os, lane_off), acc);
      }
    }
    j += a.lpc;
    if (j < jend) load_slice(j);
  }
}

// ---------------------------------------------------------------------------
// grad_x and grad_w.  Workgroup = graph x channel block (a.cpb <= kWChanBlock channels) x plane segment; a
// lane owns ONE slice of VEC pixels and walks the block's channels in order.  With Gh = grad_out / D (MEAN,
// 0 where D = 0) or grad_out (SUM):
//   grad_x[u,c,p] = w[u,p] * sum_v ascending Gamma[v][u][c] * Gh[v,c,p]               (+ grad_x_base)
//   grad_w[u,p]   = sum_c ascending sum_v ascending Gh[v,c,p] * (m_{vu}[c,p] - cnt[v][u] * out[v,c,p])
// (SUM: without the out term).  out is recomputed with the forward's arithmetic.
// ---------------------------------------------------------------------------
template <int NT, int VEC, typename T>
__global__ void __launch_bounds__(kBlock) film_wmean_bwd_xw(WArgs m) {
  const AggArgs& a = m.a;
  constexpr int SZ = Tile<NT>::SZ;
  constexpr int NTP = Tile<NT>::NTP;
  extern __shared__ float4 smem_f4[];
  const WLds<NT> L(smem_f4, a.cpb);

  const int item = blockIdx.x / m.nseg;
  const int seg = blockIdx.x - item * m.nseg;
  const int b = item / a.ncb;
  const int cb = item - b * a.ncb;
  const int node0 = m.complete ? b * a.nmax : a.goff[b];
  const int n = m.complete ? a.nmax : min(a.goff[b + 1] - node0, NT);
  if (n <= 0) return;  // whole workgroup
  const int c0 = cb * a.cpb;
  const int cend = min(a.C, c0 + a.cpb);
  const int j = seg * (int)blockDim.x + (int)threadIdx.x;
  const bool valid = j < a.PV;
  const int64_t poff = (int64_t)j * VEC;

  float wv[NT][VEC];
#pragma unroll
  for (int u = 0; u < NT; ++u) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) wv[u][k] = 0.f;
    if (valid && u < n) {
      const Frag<VEC> fw = load_frag<VEC, false>(m.w + (int64_t)(node0 + u) * m.ws + poff);
#pragma unroll
      for (int k = 0; k < VEC; ++k) wv[u][k] = fw.v[k];
    }
  }
  wmean_tiles<NT>(m, L, b, node0, n, c0, true);
  __syncthreads();
  if (!valid) return;

  unsigned emv[NT];
#pragma unroll
  for (int v = 0; v < NT; ++v) emv[v] = __builtin_amdgcn_readfirstlane(L.emask[v]);
  float Dv[NT][VEC];
#pragma unroll
  for (int v = 0; v < NT; ++v) wmean_norm<NT, VEC>(L.cnt + v * NTP, emv[v], wv, Dv[v]);

  const bool want_dx = a.want_dx != 0, want_dw = m.want_dw != 0;
  const bool need_out = want_dw && m.mean;
  float gw[NT][VEC];
#pragma unroll
  for (int u = 0; u < NT; ++u)
#pragma unroll
    for (int k = 0; k < VEC; ++k) gw[u][k] = 0.f;

  const T* xb = static_cast<const T*>(a.x) + (int64_t)node0 * a.xs + poff;
  const T* gbase = static_cast<const T*>(a.g) + (int64_t)node0 * a.gs + poff;
  for (int c = c0; c < cend; ++c) {
    const int64_t coff = (int64_t)c * a.P;
    const float* A = L.Ga + (c - c0) * SZ;
    const float* Bt = L.Gb + (c - c0) * SZ;
    float xv[NT][VEC], gv[NT][VEC], dacc[NT][VEC];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) xv[u][k] = gv[u][k] = dacc[u][k] = 0.f;
      if (u < n) {
        const Frag<VEC> f = load_frag<VEC, true>(xb + (int64_t)u * a.xs + coff);
        const Frag<VEC> g = load_frag<VEC, true>(gbase + (int64_t)u * a.gs + coff);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          xv[u][k] = f.v[k];
          gv[u][k] = g.v[k];
        }
      }
    }
#pragma unroll
    for (int v = 0; v < NT; ++v) {
      if (v < n) {
        const unsigned em = emv[v];
        float outv[VEC], gh[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) outv[k] = 0.f;
        if (need_out) {
#pragma unroll
          for (int u = 0; u < NT; ++u) {
            if (!((em >> u) & 1u)) continue;
            const float ga = A[v * NTP + u], gbv = Bt[v * NTP + u];
#pragma unroll
            for (int k = 0; k < VEC; ++k)
              outv[k] = __fadd_rn(outv[k], __fmul_rn(wv[u][k], __fadd_rn(__fmul_rn(ga, xv[u][k]), gbv)));
          }
#pragma unroll
          for (int k = 0; k < VEC; ++k) outv[k] = wmean_div(outv[k], Dv[v][k]);
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) gh[k] = m.mean ? wmean_div(gv[v][k], Dv[v][k]) : gv[v][k];
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          if (!((em >> u) & 1u)) continue;
          const float ga = A[v * NTP + u], gbv = Bt[v * NTP + u], cu = L.cnt[v * NTP + u];
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            dacc[u][k] = __fadd_rn(dacc[u][k], __fmul_rn(ga, gh[k]));
            if (want_dw) {
              const float msg = __fadd_rn(__fmul_rn(ga, xv[u][k]), gbv);
              gw[u][k] = __fadd_rn(gw[u][k], __fmul_rn(gh[k], __fadd_rn(msg, -__fmul_rn(cu, outv[k]))));
            }
          }
        }
      }
    }
    if (want_dx) {
      T* ob = static_cast<T*>(a.out) + (int64_t)node0 * a.os + poff + coff;
      const T* bb =
          a.dxb != nullptr ? static_cast<const T*>(a.dxb) + (int64_t)node0 * a.dxbs + poff + coff : nullptr;
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        if (u < n) {
          Frag<VEC> o;
#pragma unroll
          for (int k = 0; k < VEC; ++k) o.v[k] = __fmul_rn(wv[u][k], dacc[u][k]);
          if (bb != nullptr) {
            const Frag<VEC> base = load_frag<VEC, true>(bb + (int64_t)u * a.dxbs);
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = __fadd_rn(o.v[k], base.v[k]);
          }
          store_frag<VEC, true>(ob + (int64_t)u * a.os, o);
        }
      }
    }
  }
  if (want_dw) {
    float* db = m.dw + (int64_t)cb * m.dwbs + (int64_t)node0 * m.dws + poff;
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      if (u < n) {
        Frag<VEC> o;
#pragma unroll
        for (int k = 0; k < VEC; ++k) o.v[k] = gw[u][k];
        store_frag<VEC, false>(db + (int64_t)u * m.dws, o);
      }
    }
  }
}

// grad_w = the channel blocks' partials added in block order.  (A template so that only film_wmean_bwd.hip,
// which launches it, emits it.)
template <int UNUSED = 0>
__global__ void __launch_bounds__(kBlock) film_wmean_dw_reduce(const float* part, int32_t nblk, int64_t bs, float* dw,
                                                               int64_t dws, int64_t total, int32_t P) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= total) return;
  float s = part[i];
  for (int k = 1; k < nblk; ++k) s = __fadd_rn(s, part[(int64_t)k * bs + i]);
  const int64_t node = i / P;
  dw[node * dws + (i - node * P)] = s;
}

// ---------------------------------------------------------------------------
// grad_gb.  Workgroup = graph x channel block x block of kWDestBlock destinations; a lane owns one channel
// and sweeps its slices of the whole plane, as film_max_bwd's destination-block pass:
//   S[v][u] = (sum_p w[u,p] x[u,c,p] Gh[v,c,p], sum_p w[u,p] Gh[v,c,p])
// as per-lane partial sums, one fixed butterfly over the plane's lanes (lpc <= 64: one wave), then every CSR
// entry (u -> v) of the block's destinations is written from S[v][u].
// ---------------------------------------------------------------------------
template <int NT, int VEC, typename T>
__global__ void __launch_bounds__(kBlock) film_wmean_bwd_gb(WArgs m) {
  const AggArgs& a = m.a;
  constexpr int NTP = Tile<NT>::NTP;
  constexpr int VB = kWDestBlock;
  extern __shared__ float4 smem_f4[];
  const WLds<NT> L(smem_f4, 0);  // tables only
  float2* S = reinterpret_cast<float2*>(L.extra);  // [cpb][VB][NTP]

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
  const float* wb = m.w + (int64_t)node0 * m.ws;
  const uint32_t lane_plane = (uint32_t)grp * (uint32_t)a.P * (uint32_t)sizeof(T);

  float xv[NT][VEC], wv[NT][VEC];
#pragma unroll
  for (int u = 0; u < NT; ++u)
#pragma unroll
    for (int k = 0; k < VEC; ++k) xv[u][k] = wv[u][k] = 0.f;
  auto load_slice = [&](int jj) {
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      if (u < n) {
        const Frag<VEC> f = load_frag<VEC, true>(
            at_bytes(xb + (int64_t)u * a.xs, lane_plane + (uint32_t)jj * VEC * (uint32_t)sizeof(T)));
        const Frag<VEC> fw =
            load_frag<VEC, false>(at_bytes(wb + (int64_t)u * m.ws, (uint32_t)jj * VEC * (uint32_t)sizeof(float)));
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          xv[u][k] = f.v[k];
          wv[u][k] = fw.v[k];
        }
      }
    }
  };
  int j = li;
  if (active && j < a.PV) load_slice(j);
  wmean_tiles<NT>(m, L, b, node0, n, c0, false);
  __syncthreads();

  unsigned emv[VB];
#pragma unroll
  for (int i = 0; i < VB; ++i) emv[i] = __builtin_amdgcn_readfirstlane(L.emask[min(v0 + i, NT - 1)]);

  float pg[VB][NT], pb[VB][NT];
#pragma unroll
  for (int i = 0; i < VB; ++i)
#pragma unroll
    for (int u = 0; u < NT; ++u) pg[i][u] = pb[i][u] = 0.f;

  if (active) {
    while (j < a.PV) {
      const uint32_t lane_off = lane_plane + (uint32_t)j * VEC * (uint32_t)sizeof(T);
#pragma unroll
      for (int i = 0; i < VB; ++i) {
        const int v = v0 + i;
        if (v < n) {  // wave-uniform
          const Frag<VEC> G = load_frag<VEC, true>(at_bytes(gbase + (int64_t)v * a.gs, lane_off));
          const unsigned em = emv[i];
          float gh[VEC];
          if (m.mean) {
            float D[VEC];
            wmean_norm<NT, VEC>(L.cnt + v * NTP, em, wv, D);
#pragma unroll
            for (int k = 0; k < VEC; ++k) gh[k] = wmean_div(G.v[k], D[k]);
          } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) gh[k] = G.v[k];
          }
#pragma unroll
          for (int u = 0; u < NT; ++u) {
            if (!((em >> u) & 1u)) continue;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
              const float t = __fmul_rn(wv[u][k], gh[k]);
              pg[i][u] = __fadd_rn(pg[i][u], __fmul_rn(xv[u][k], t));
              pb[i][u] = __fadd_rn(pb[i][u], t);
            }
          }
        }
      }
      j += a.lpc;
      if (j < a.PV) load_slice(j);
    }
  }

  // the plane's lanes sit in one wave (lpc <= 64): a fixed butterfly, every lane ends with the sum
  with_lanes(a.lpc, [&](auto lanes) {
    constexpr int LN = decltype(lanes)::value;
#pragma unroll
    for (int i = 0; i < VB; ++i)
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        const float2 r = make_float2(group_sum<LN>(pg[i][u]), group_sum<LN>(pb[i][u]));
        if (active && li == 0) S[(grp * VB + i) * NTP + u] = r;
      }
  });
  __syncthreads();

  // one thread per (channel, destination): its row's entries, each from its pair's sums
  for (int t = threadIdx.x; t < a.cpb * VB; t += blockDim.x) {
    int cl, i;
    split_channel(a, t, cl, i);
    const int v = v0 + i, cc = c0 + cl;
    if (v >= n || cc >= a.C) continue;
    const float2* Sr = S + (cl * VB + i) * NTP;
    auto put = [&](int64_t e, int u) {
      const int64_t off = (e * a.C + cc) * 2;
      float2 r = Sr[u];
      if (a.logits) r = sigmoid_backward(r, *reinterpret_cast<const float2*>(a.gb + off));
      *reinterpret_cast<float2*>(a.dgb + off) = r;
    };
    if (m.complete) {
      const int64_t ebase = (int64_t)b * n * (n - 1);
      for (int u = 0; u < n; ++u)
        if (u != v) put(complete_eid(ebase, n, u, v), u);
    } else {
      const int beg = a.kdeg > 0 ? (node0 + v) * a.kdeg : a.indptr[node0 + v];
      const int end = a.kdeg > 0 ? beg + a.kdeg : a.indptr[node0 + v + 1];
      for (int k = beg; k < end; ++k) {
        const int u = a.src[k] - node0;
        if ((unsigned)u < (unsigned)n) put(a.eid[k], u);
      }
    }
  }
}

}  // namespace mrp

namespace mrp_host {

using mrp::WArgs;

// compiled node capacity of a graph size
inline int wmean_bucket(int max_nodes) { return max_nodes <= 4 ? 4 : (max_nodes <= 8 ? 8 : 16); }

inline size_t lds_wmean(int nt, int cpb_tiles) {
  const int ntp = (nt + 3) & ~3;
  return (size_t)(2 * cpb_tiles * (nt * ntp + 4) + nt * ntp + ntp) * sizeof(float);
}
inline size_t lds_wmean_gb(int nt, int cpb) {
  const int ntp = (nt + 3) & ~3;
  return lds_wmean(nt, 0) + (size_t)cpb * mrp::kWDestBlock * ntp * sizeof(float2);
}

// channel blocks of film_wmean_bwd_xw, and the bytes of their grad_w partials (0: one block, written directly)
inline int wmean_dw_blocks(int C) { return (C + mrp::kWChanBlock - 1) / mrp::kWChanBlock; }
inline int64_t wmean_workspace_bytes(int32_t num_nodes, int32_t C, int32_t P) {
  const int nb = wmean_dw_blocks(C);
  return nb > 1 ? (int64_t)nb * num_nodes * P * (int64_t)sizeof(float) : 0;
}

// The backward's launches (film_wmean_bwd.hip plans, the per-dtype units launch).
struct WBwdPlan {
  int bucket = 0;     // NT
  int vec = 1;        // 4 (graphs of <= 8 nodes, aligned operands) or 1
  int run_xw = 0;     // grad_x and / or grad_w
  int64_t grid_xw = 0;
  int threads_xw = 0, cpb_xw = 0, ncb_xw = 0, nseg = 1;
  size_t lds_xw = 0;
  int run_gb = 0;     // grad_gb
  Geometry g;         // film_wmean_bwd_gb: lpc, cpb, threads, ncb, grid (x nvb), lds
  int nvb = 1;
};

hipError_t launch_wmean_bwd_f32(const WArgs& m, const WBwdPlan& p, hipStream_t st);
hipError_t launch_wmean_bwd_bf16(const WArgs& m, const WBwdPlan& p, hipStream_t st);
hipError_t launch_wmean_bwd_f16(const WArgs& m, const WBwdPlan& p, hipStream_t st);

template <typename T>
hipError_t launch_wmean_bwd(WArgs m, const WBwdPlan& p, hipStream_t st) {
#define MRP_WMEAN_BWD(KERNEL, GRID, THREADS, LDS)                                              \
  do {                                                                                         \
    const dim3 grid((unsigned)(GRID)), block(THREADS);                                         \
    if (p.bucket == 4 && p.vec == 4)                                                           \
      hipLaunchKernelGGL((mrp::KERNEL<4, 4, T>), grid, block, LDS, st, m);                     \
    else if (p.bucket == 4)                                                                    \
      hipLaunchKernelGGL((mrp::KERNEL<4, 1, T>), grid, block, LDS, st, m);                     \
    else if (p.bucket == 8 && p.vec == 4)                                                      \
      hipLaunchKernelGGL((mrp::KERNEL<8, 4, T>), grid, block, LDS, st, m);                     \
    else if (p.bucket == 8)                                                                    \
      hipLaunchKernelGGL((mrp::KERNEL<8, 1, T>), grid, block, LDS, st, m);                     \
    else if (p.vec == 1)                                                                       \
      hipLaunchKernelGGL((mrp::KERNEL<16, 1, T>), grid, block, LDS, st, m);                    \
    else                                                                                       \
      return hipErrorInvalidValue;                                                             \
  } while (0)
  if (p.run_xw) {
    m.a.cpb = p.cpb_xw;
    m.a.ncb = p.ncb_xw;
    m.nseg = p.nseg;
    MRP_WMEAN_BWD(film_wmean_bwd_xw, p.grid_xw, p.threads_xw, p.lds_xw);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (p.run_gb) {
    m.a.cpb = p.g.cpb;
    m.a.ncb = p.g.ncb;
    m.a.lpc = p.g.lpc;
    m.nvb = p.nvb;
    MRP_WMEAN_BWD(film_wmean_bwd_gb, p.g.grid, p.g.threads, p.g.lds);
  }
#undef MRP_WMEAN_BWD
  return hipGetLastError();
}

}  // namespace mrp_host
