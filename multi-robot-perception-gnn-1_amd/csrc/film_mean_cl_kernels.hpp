#pragma once
// film_mean_cl_kernels.hpp — the FiLM-mean aggregation on pixel-major ("channels-last") feature maps.
//
// A feature tensor is (node, pixel, channel): node v's pixel p is a row of C contiguous elements at
// base + v * node_stride + p * pixel_stride (strides in elements; pixel_stride >= C, e.g. 2C for one
// half of a channels-last concatenation buffer).  gamma/beta are per channel and (E, C, 2) is already
// channel-contiguous, so here a lane owns a vector of channels of one pixel (16 bytes: 4 fp32 or 8
// 16-bit channels) instead of a slice of one channel plane, and the per-edge (gamma, beta) of the
// workgroup's channel block sit in LDS as [slot][channel] rows read per lane.
//
// The arithmetic is the node-major kernels' (film_mean_kernels.hpp), operation for operation:
//   forward   m = fl(fl(gamma x_u) + beta), acc = fl(acc + m) over the destination's slots, the mean a
//             correctly rounded division by the in-degree, then the epilogue of apply_epilogue;
//   grad_x    one fmaf chain per element: base (or 0), self_scale G[u], then Wt[u][v] G[v], v ascending;
//   grad_gb   s_v * sum_p G_v x_u and s_v * sum_p G_v in fp32 (fixed order: pixels of a wave ascending,
//             waves in order, plane segments in order).
// A destination's slots are what the node-major kernel of the same graph kind sums: the sources
// u != v ascending (COMPLETE), the CSR row in edge order (REGULAR(k), k <= 8: film_fwd_regular), or
// the distinct sources ascending with the gamma and beta of parallel edges added up first (any other
// CSR graph: film_fwd's dense tiles).
#include "film_mean_kernels.hpp"

namespace mrp {

struct ClTensor {
  const void* p;
  int64_t ns;  // node stride (elements)
  int64_t ps;  // pixel stride (elements)
};

constexpr int kClCsr = 0;       // dense tiles: parallel edges summed, sources ascending
constexpr int kClComplete = 1;  // arithmetic edge ids
constexpr int kClSlots = 2;     // REGULAR(k <= 8): one slot per edge in CSR order

struct ClArgs {
  ClTensor x, g, out, base, x0, xc;  // fwd: x, out, x0, xc;  bwd: g (grad_out), x, out (grad_x), base
  const float* gb;
  float* dgb;
  float* ws;  // Gram partials of the plane segments
  const int32_t* indptr;
  const int32_t* src;
  const int32_t* eid;
  const int32_t* goff;
  int32_t C, P, mode, logits, kind, kdeg, nmax;
  int32_t cb;      // channels per workgroup (a power of two)
  int32_t ncb;     // channel blocks per graph
  int32_t nseg;    // pixel segments per (graph, channel block)
  int32_t seglen;  // pixels per segment
  float agg_scale, self_scale, x0_scale;
};

template <int NT>
struct ClTables {
  static constexpr int kSlots = NT * (NT > 8 ? NT : 8);
  int sbeg[NT + 1];  // slot range of destination v: [sbeg[v], sbeg[v + 1])
  int cnt[NT];
  float deg[NT];
  unsigned mask[NT];
  int ssrc[kSlots];  // slot -> local source
  static constexpr int kBytes = (int)((sizeof(int) * (NT + 1 + NT + kSlots) + sizeof(float) * NT +
                                       sizeof(unsigned) * NT + 15) & ~(size_t)15);
};

template <int NT>
struct ClVec {
  typedef float type __attribute__((ext_vector_type(NT <= 4 ? 4 : (NT <= 8 ? 8 : 16))));
};

// workgroup -> (graph b, channel block, pixel segment), the graph's first node and node count
struct ClItem {
  int b, cbi, seg, node0, n, c0, pbeg, pend;
};
template <int NT>
__device__ __forceinline__ ClItem cl_item(const ClArgs& a) {
  ClItem it;
  const int item = blockIdx.x / a.nseg;
  it.seg = blockIdx.x - item * a.nseg;
  it.b = item / a.ncb;
  it.cbi = item - it.b * a.ncb;
  it.node0 = a.kind == kClComplete ? it.b * a.nmax : a.goff[it.b];
  it.n = a.kind == kClComplete ? a.nmax : min(a.goff[it.b + 1] - it.node0, NT);
  it.c0 = it.cbi * a.cb;
  it.pbeg = it.seg * a.seglen;
  it.pend = min(a.P, it.pbeg + a.seglen);
  return it;
}

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// CSR row of destination v (REGULAR(k): [k v, k (v + 1)), indptr is not read)
__device__ __forceinline__ void cl_row(const ClArgs& a, int node, int& beg, int& end) {
  beg = a.kdeg > 0 ? node * a.kdeg : a.indptr[node];
  end = a.kdeg > 0 ? beg + a.kdeg : a.indptr[node + 1];
}

__device__ __forceinline__ float2 cl_gb(const ClArgs& a, int64_t e, int c) {
  if (a.mode == MRP_AGG_COPY_MEAN) return make_float2(1.f, 0.f);
  float2 w = *reinterpret_cast<const float2*>(a.gb + (e * a.C + c) * 2);
  if (a.logits) w = make_float2(sigmoidf(w.x), sigmoidf(w.y));
  return w;
}

// reduce scale s_v of the backward (folded with the epilogue's agg_scale), as build_tiles_csr /
// complete_store form it
__device__ __forceinline__ float cl_scale(const ClArgs& a, int deg) {
  float s = 1.f;
  if (a.mode != MRP_AGG_FILM_SUM && deg > 0) s = 1.f / (float)deg;
  return s * a.agg_scale;
}

// VEC consecutive floats / float2 of an LDS row
template <int VEC>
__device__ __forceinline__ void lds_row(const float* p, float* w) {
  if constexpr (VEC % 4 == 0) {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
      const f4 t = *reinterpret_cast<const f4*>(p + 4 * q);
      w[4 * q] = t.x; w[4 * q + 1] = t.y; w[4 * q + 2] = t.z; w[4 * q + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) w[k] = p[k];
  }
}

// ---------------------------------------------------------------------------
// Forward.  Lane (pl, cv) owns channels [c0 + cv VEC, + VEC) of PIX pixels; x of all sources of those
// pixels sits in registers (indexed by the wave-uniform slot source), the slots' (gamma, beta) rows
// are read from LDS once per PIX pixels.
// ---------------------------------------------------------------------------
// COMPLETE: destination v's slots are the sources u != v ascending, slot v (n - 1) + (u < v ? u : u - 1):
// the sweep is unrolled over (v, u) with compile-time register indices (a run-time source index costs
// a register-relative move per element: the slot loop then issues more VALU than the HBM time holds).
template <int NT, int VEC, int PIX, bool COMPLETE, typename T>
__global__ void __launch_bounds__(kBlock) film_fwd_cl(ClArgs a) {
  typedef typename ClVec<NT>::type vnt;
  typedef ClTables<NT> Tb;
  extern __shared__ float4 smem_f4[];
  Tb* tb = reinterpret_cast<Tb*>(smem_f4);
  float2* gbt = reinterpret_cast<float2*>(reinterpret_cast<char*>(smem_f4) + Tb::kBytes);  // [slot][cb]

  const ClItem it = cl_item<NT>(a);
  const int n = it.n, node0 = it.node0;
  if (n <= 0) return;
  const int tid = threadIdx.x;
  const int lcb = __builtin_ctz((unsigned)a.cb);
  const int cbv = a.cb / VEC;  // lanes per pixel
  const int lcbv = __builtin_ctz((unsigned)cbv);
  const int cv = tid & (cbv - 1);
  const int pl = tid >> lcbv;
  const int ppb = kBlock >> lcbv;  // pixels per pass of the workgroup
  const int c = it.c0 + cv * VEC;
  const bool active = c < a.C;
  constexpr uint32_t ES = sizeof(T);

  const T* xb = static_cast<const T*>(a.x.p) + (int64_t)node0 * a.x.ns;
  T* ob = static_cast<T*>(const_cast<void*>(a.out.p)) + (int64_t)node0 * a.out.ns;

  vnt xv[PIX][VEC];
#pragma unroll
  for (int i = 0; i < PIX; ++i)
#pragma unroll
    for (int k = 0; k < VEC; ++k) xv[i][k] = (vnt)(0.f);
  auto load_pixels = [&](int p0) {
#pragma unroll
    for (int i = 0; i < PIX; ++i) {
      const int pi = p0 + i * ppb < it.pend ? p0 + i * ppb : p0;  // past the segment: a valid pixel, not stored
      const uint32_t off = ((uint32_t)pi * (uint32_t)a.x.ps + (uint32_t)c) * ES;
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        if (u < n) {
          const Frag<VEC> f = load_frag<VEC, true>(at_bytes(xb + (int64_t)u * a.x.ns, off));
#pragma unroll
          for (int k = 0; k < VEC; ++k) xv[i][k][u] = f.v[k];
        }
      }
    }
  };
  int p0 = it.pbeg + pl;
  // the first pixels' loads are issued before the prologue's dependent loads and LDS writes
  if (active && p0 < it.pend) load_pixels(p0);

  // prologue 1: slot counts, in-degrees and (CSR) neighbour masks per destination
  if (tid < NT) {
    const int v = tid;
    int cnt = 0, deg = 0;
    unsigned mask = 0u;
    if (v < n) {
      if (a.kind == kClComplete) {
        cnt = deg = n - 1;
      } else {
        int beg, end;
        cl_row(a, node0 + v, beg, end);
        deg = end - beg;
        if (a.kind == kClSlots) {
          cnt = deg;
        } else {
          for (int k = beg; k < end; ++k) {
            const int u = a.src[k] - node0;
            if ((unsigned)u < (unsigned)n) mask |= 1u << u;
          }
          cnt = __builtin_popcount(mask);
        }
      }
    }
    tb->cnt[v] = cnt;
    tb->deg[v] = (float)deg;
    tb->mask[v] = mask;
  }
  __syncthreads();
  // prologue 2: slot ranges and slot sources
  if (tid <= NT) {
    int s = 0;
    for (int i = 0; i < tid; ++i) s += tb->cnt[i];
    tb->sbeg[tid] = s;
    if (tid < n) {
      const int v = tid;
      if (a.kind == kClComplete) {
        for (int u = 0; u < n; ++u)
          if (u != v) tb->ssrc[s++] = u;
      } else if (a.kind == kClSlots) {
        int beg, end;
        cl_row(a, node0 + v, beg, end);
        for (int k = beg; k < end; ++k) {
          const int u = a.src[k] - node0;
          tb->ssrc[s++] = (unsigned)u < (unsigned)n ? u : 0;  // (rejected by the graph builder)
        }
      } else {
        const unsigned mask = tb->mask[v];
        for (int u = 0; u < NT; ++u)
          if ((mask >> u) & 1u) tb->ssrc[s++] = u;
      }
    }
  }
  __syncthreads();
  // prologue 3: the slots' (gamma, beta) rows, channel fastest (coalesced 8 cb-byte rows of gb)
  const int total = tb->sbeg[n];
  if (a.kind != kClCsr) {
    const int64_t ebase = (int64_t)it.b * n * (n - 1);
    for (int t = tid; t < total * a.cb; t += kBlock) {
      const int cl = t & (a.cb - 1), slot = t >> lcb;
      const int cc = it.c0 + cl;
      float2 w = make_float2(0.f, 0.f);
      if (cc < a.C) {
        int64_t e;
        if (a.kind == kClComplete) {
          const int v = slot / (n - 1), j = slot - v * (n - 1);
          e = complete_eid(ebase, n, j < v ? j : j + 1, v);
        } else {
          e = a.mode != MRP_AGG_COPY_MEAN ? a.eid[node0 * a.kdeg + slot] : 0;
        }
        w = cl_gb(a, e, cc);
      }
      gbt[t] = w;
    }
  } else {
    for (int t = tid; t < total * a.cb; t += kBlock) gbt[t] = make_float2(0.f, 0.f);
    __syncthreads();
    for (int t = tid; t < NT * a.cb; t += kBlock) {
      const int cl = t & (a.cb - 1), v = t >> lcb;
      const int cc = it.c0 + cl;
      if (v >= n || cc >= a.C) continue;
      int beg, end;
      cl_row(a, node0 + v, beg, end);
      const unsigned mask = tb->mask[v];
      const int s0 = tb->sbeg[v];
      for (int k = beg; k < end; ++k) {  // CSR order: parallel edges sum deterministically
        const int u = a.src[k] - node0;
        if ((unsigned)u >= (unsigned)n) continue;
        const float2 w = cl_gb(a, a.mode != MRP_AGG_COPY_MEAN ? a.eid[k] : 0, cc);
        float2* q = gbt + (s0 + __builtin_popcount(mask & ((1u << u) - 1u))) * a.cb + cl;
        q->x += w.x;
        q->y += w.y;
      }
    }
  }
  __syncthreads();
  if (!active) return;

  const bool mean = a.mode != MRP_AGG_FILM_SUM;
  const T* x0b = a.x0.p != nullptr ? static_cast<const T*>(a.x0.p) + (int64_t)node0 * a.x0.ns : nullptr;
  T* xcb = a.xc.p != nullptr ? static_cast<T*>(const_cast<void*>(a.xc.p)) + (int64_t)node0 * a.xc.ns : nullptr;
  while (p0 < it.pend) {
    // laundered: the unrolled COMPLETE sweep must re-read its rows per pixel, not hoist the tile
    int wo = cv * VEC;
    asm volatile("" : "+v"(wo));
    const float2* wl = gbt + wo;
    uint32_t ooff[PIX], x0off[PIX], xcoff[PIX];
    bool valid[PIX];
#pragma unroll
    for (int i = 0; i < PIX; ++i) {
      valid[i] = p0 + i * ppb < it.pend;
      const uint32_t pi = (uint32_t)(valid[i] ? p0 + i * ppb : p0);
      ooff[i] = (pi * (uint32_t)a.out.ps + (uint32_t)c) * ES;
      x0off[i] = (pi * (uint32_t)a.x0.ps + (uint32_t)c) * ES;
      xcoff[i] = (pi * (uint32_t)a.xc.ps + (uint32_t)c) * ES;
    }
#pragma unroll
    for (int v = 0; v < NT; ++v) {
      if (v >= n) break;
      float acc[PIX][VEC];
#pragma unroll
      for (int i = 0; i < PIX; ++i)
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[i][k] = 0.f;
      float d;
      if constexpr (COMPLETE) {
        d = (float)(n - 1);
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          if (u >= n) break;
          if (u == v) continue;
          const int s = v * (n - 1) + (u < v ? u : u - 1);
          float w[2 * VEC];
          lds_row<2 * VEC>(reinterpret_cast<const float*>(wl + s * a.cb), w);
#pragma unroll
          for (int i = 0; i < PIX; ++i)
#pragma unroll
            for (int k = 0; k < VEC; ++k)
              acc[i][k] = __fadd_rn(acc[i][k], __fadd_rn(__fmul_rn(w[2 * k], xv[i][k][u]), w[2 * k + 1]));
        }
      } else {
        const int s0 = uniform(tb->sbeg[v]), s1 = uniform(tb->sbeg[v + 1]);
        d = __builtin_bit_cast(float, uniform(__builtin_bit_cast(int, tb->deg[v])));
        for (int s = s0; s < s1; ++s) {
          const int u = uniform(tb->ssrc[s]);
          float w[2 * VEC];
          lds_row<2 * VEC>(reinterpret_cast<const float*>(wl + s * a.cb), w);
#pragma unroll
          for (int i = 0; i < PIX; ++i)
#pragma unroll
            for (int k = 0; k < VEC; ++k)
              acc[i][k] = __fadd_rn(acc[i][k], __fadd_rn(__fmul_rn(w[2 * k], xv[i][k][u]), w[2 * k + 1]));
        }
      }
#pragma unroll
      for (int i = 0; i < PIX; ++i) {
        if (mean && d > 0.f) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[i][k] = acc[i][k] / d;
        }
        if (a.agg_scale != 1.f) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[i][k] = __fmul_rn(a.agg_scale, acc[i][k]);
        }
        if (a.self_scale != 0.f) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[i][k] = __fadd_rn(acc[i][k], __fmul_rn(a.self_scale, xv[i][k][v]));
        }
        if (x0b != nullptr) {
          const Frag<VEC> z = load_frag<VEC, true>(at_bytes(x0b + (int64_t)v * a.x0.ns, x0off[i]));
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[i][k] = __fadd_rn(acc[i][k], __fmul_rn(a.x0_scale, z.v[k]));
        }
        if (valid[i]) {
          Frag<VEC> o;
#pragma unroll
          for (int k = 0; k < VEC; ++k) o.v[k] = acc[i][k];
          store_frag<VEC, true>(at_bytes(ob + (int64_t)v * a.out.ns, ooff[i]), o);
        }
      }
    }
    if (xcb != nullptr) {  // cat((x, aggregate), 1): x is in registers already
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        if (u >= n) break;
#pragma unroll
        for (int i = 0; i < PIX; ++i) {
          if (!valid[i]) continue;
          Frag<VEC> f;
#pragma unroll
          for (int k = 0; k < VEC; ++k) f.v[k] = xv[i][k][u];
          store_frag<VEC, true>(at_bytes(xcb + (int64_t)u * a.xc.ns, xcoff[i]), f);
        }
      }
    }
    p0 += ppb * PIX;
    if (p0 < it.pend) load_pixels(p0);
  }
}

// ---------------------------------------------------------------------------
// Backward, grad_x: the forward's lane layout; the dense transposed weights Wt[u][v] = s_v * (sum of
// gamma over the edges u -> v) of the channel block sit in LDS as [u][v][channel] rows.
// ---------------------------------------------------------------------------
template <int NT, int VEC, typename T>
__global__ void __launch_bounds__(kBlock) film_bwd_dx_cl(ClArgs a) {
  typedef typename ClVec<NT>::type vnt;
  extern __shared__ float4 smem_f4[];
  float* Wt = reinterpret_cast<float*>(smem_f4);  // [(u NT + v)][cb]

  const ClItem it = cl_item<NT>(a);
  const int n = it.n, node0 = it.node0;
  if (n <= 0) return;
  const int tid = threadIdx.x;
  const int lcb = __builtin_ctz((unsigned)a.cb);
  const int cbv = a.cb / VEC;
  const int lcbv = __builtin_ctz((unsigned)cbv);
  const int cv = tid & (cbv - 1);
  const int pl = tid >> lcbv;
  const int ppb = kBlock >> lcbv;
  const int c = it.c0 + cv * VEC;
  const bool active = c < a.C;
  const bool complete = a.kind == kClComplete;
  constexpr uint32_t ES = sizeof(T);

  const T* gbase = static_cast<const T*>(a.g.p) + (int64_t)node0 * a.g.ns;
  const T* bb = a.base.p != nullptr ? static_cast<const T*>(a.base.p) + (int64_t)node0 * a.base.ns : nullptr;
  T* ob = static_cast<T*>(const_cast<void*>(a.out.p)) + (int64_t)node0 * a.out.ns;

  // element k of every node's vector in one NT-wide value: a rolled node loop indexes registers, not scratch
  vnt gv[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) gv[k] = (vnt)(0.f);
  auto load_pixel = [&](int p) {
    const uint32_t off = ((uint32_t)p * (uint32_t)a.g.ps + (uint32_t)c) * ES;
#pragma unroll
    for (int v = 0; v < NT; ++v) {
      if (v < n) {
        const Frag<VEC> f = load_frag<VEC, false>(at_bytes(gbase + (int64_t)v * a.g.ns, off));
#pragma unroll
        for (int k = 0; k < VEC; ++k) gv[k][v] = f.v[k];
      }
    }
  };
  int p = it.pbeg + pl;
  if (active && p < it.pend) load_pixel(p);

  for (int t = tid; t < NT * NT * a.cb; t += kBlock) Wt[t] = 0.f;
  __syncthreads();
  for (int t = tid; t < NT * a.cb; t += kBlock) {
    const int cl = t & (a.cb - 1), v = t >> lcb;
    const int cc = it.c0 + cl;
    if (v >= n || cc >= a.C) continue;
    if (complete) {
      const float s = cl_scale(a, n - 1);
      const int64_t ebase = (int64_t)it.b * n * (n - 1);
      for (int u = 0; u < n; ++u)
        if (u != v) Wt[((u * NT + v) << lcb) + cl] = s * cl_gb(a, complete_eid(ebase, n, u, v), cc).x;
    } else {
      int beg, end;
      cl_row(a, node0 + v, beg, end);
      const float s = cl_scale(a, end - beg);
      for (int k = beg; k < end; ++k) {
        const int u = a.src[k] - node0;
        if ((unsigned)u >= (unsigned)n) continue;
        Wt[((u * NT + v) << lcb) + cl] += s * cl_gb(a, a.mode != MRP_AGG_COPY_MEAN ? a.eid[k] : 0, cc).x;
      }
    }
  }
  __syncthreads();
  if (!active) return;

  while (p < it.pend) {
    // the weights are re-read from LDS for every pixel: laundering the row offset stops the compiler
    // from hoisting the whole unrolled tile into registers (256 VGPRs at 8 nodes x 8 channels)
    int wo = cv * VEC;
    asm volatile("" : "+v"(wo));
    const float* wl = Wt + wo;
    const uint32_t ooff = ((uint32_t)p * (uint32_t)a.out.ps + (uint32_t)c) * ES;
    const uint32_t boff = ((uint32_t)p * (uint32_t)a.base.ps + (uint32_t)c) * ES;
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      if (u >= n) break;
      Frag<VEC> acc;
      if (bb != nullptr) {
        acc = load_frag<VEC, true>(at_bytes(bb + (int64_t)u * a.base.ns, boff));
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = 0.f;
      }
      if (a.self_scale != 0.f) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = fmaf(a.self_scale, gv[k][u], acc.v[k]);
      }
#pragma unroll
      for (int v = 0; v < NT; ++v) {
        if (v >= n) break;
        if (complete && v == u) continue;
        float w[VEC];
        lds_row<VEC>(wl + ((u * NT + v) << lcb), w);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.v[k] = fmaf(w[k], gv[k][v], acc.v[k]);
      }
      store_frag<VEC, true>(at_bytes(ob + (int64_t)u * a.out.ns, ooff), acc);
    }
    p += ppb;
    if (p < it.pend) load_pixel(p);
  }
}

// ---------------------------------------------------------------------------
// Backward, grad_gb.  A workgroup owns a graph x 64 channels x a pixel segment and stages the x and
// grad_out rows of a chunk of PC pixels into LDS in their storage type, as coalesced 16-byte pieces of
// the 64-channel rows (one element per access when pointers, strides or C do not allow vectors).  Then
// lane l of every wave reads channel l of each node and pixel from LDS (consecutive banks) and keeps the
// Gram D[v][u] = sum_p G_v x_u and S[v] = sum_p G_v of a block of VB destinations in registers.  Graphs
// of <= 8 nodes: one block, the four waves take every fourth pixel of the chunk and are summed in wave
// order through LDS.  9..16 nodes: four blocks of four destinations, one per wave, every wave walking
// the whole chunk — in LDS, so the blocking costs no global traffic.  A plane split over several
// workgroups (nseg > 1) leaves the partial sums in the workspace; film_gram_finish_cl adds them in
// segment order and writes grad_gb.
// ---------------------------------------------------------------------------
template <int NT>
struct ClGram {
  static constexpr int VB = NT <= 8 ? NT : 4;  // destinations per wave
  static constexpr int NB = NT / VB;           // destination blocks (1 or 4)
  static constexpr int PG = 4 / NB;            // pixel groups (waves per destination block)
  static constexpr int ROW = NT + 1;           // D[v][0..NT) and S[v]
};

// grad_gb of the edges into destinations [vb0, vb0 + VB) from the lane's sums
template <int NT, int VB>
__device__ __forceinline__ void gram_emit(const ClArgs& a, const ClItem& it, int c, int vb0,
                                          const typename ClVec<NT>::type* D, const float* S) {
  const int n = it.n, node0 = it.node0;
#pragma unroll
  for (int i = 0; i < VB; ++i) {
    const int v = vb0 + i;
    if (v >= n) break;
    if (a.kind == kClComplete) {
      const float s = cl_scale(a, n - 1);
      const int64_t ebase = (int64_t)it.b * n * (n - 1);
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        if (u >= n) break;
        if (u == v) continue;
        const int64_t off = (complete_eid(ebase, n, u, v) * a.C + c) * 2;
        float2 r = make_float2(s * D[i][u], s * S[i]);
        if (a.logits) r = sigmoid_backward(r, *reinterpret_cast<const float2*>(a.gb + off));
        *reinterpret_cast<float2*>(a.dgb + off) = r;
      }
    } else {
      int beg, end;
      cl_row(a, node0 + v, beg, end);
      beg = uniform(beg);
      end = uniform(end);
      const float s = cl_scale(a, end - beg);
      for (int k = beg; k < end; ++k) {
        const int u = uniform(a.src[k]) - node0;
        float2 r = make_float2(0.f, 0.f);
        if ((unsigned)u < (unsigned)n) r = make_float2(s * D[i][u], s * S[i]);
        const int64_t off = ((int64_t)uniform(a.eid[k]) * a.C + c) * 2;
        if (a.logits) r = sigmoid_backward(r, *reinterpret_cast<const float2*>(a.gb + off));
        *reinterpret_cast<float2*>(a.dgb + off) = r;
      }
    }
  }
}

template <int NT, bool VECP, typename T>
__global__ void __launch_bounds__(kBlock) film_bwd_gram_cl(ClArgs a) {
  typedef typename ClVec<NT>::type vnt;
  constexpr int VB = ClGram<NT>::VB, NB = ClGram<NT>::NB, PG = ClGram<NT>::PG, ROW = ClGram<NT>::ROW;
  constexpr int PC = NT <= 8 ? 8 : 4;   // pixels per staged chunk
  constexpr int ROWS = 2 * NT * PC;     // staged rows [tensor (x, grad_out)][node][pixel] of 64 channels
  constexpr int kStage = ROWS * 64 * (int)sizeof(T);
  constexpr int kRed = PG > 1 ? VB * ROW * 64 * (int)sizeof(float) : 0;
  __shared__ float4 smem4[((kStage > kRed ? kStage : kRed) + 15) / 16];
  T* st = reinterpret_cast<T*>(smem4);
  float* red = reinterpret_cast<float*>(smem4);  // after the sweep: the stage buffer is free

  const ClItem it = cl_item<NT>(a);
  const int n = it.n, node0 = it.node0;
  if (n <= 0) return;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int blk = wave % NB, pg = wave / NB;
  const int vb0 = blk * VB;
  const int c = it.c0 + lane;
  const bool act = c < a.C;
  const T* xb = static_cast<const T*>(a.x.p) + (int64_t)node0 * a.x.ns;
  const T* gbase = static_cast<const T*>(a.g.p) + (int64_t)node0 * a.g.ns;

  vnt D[VB];
  float S[VB];
#pragma unroll
  for (int i = 0; i < VB; ++i) {
    D[i] = (vnt)(0.f);
    S[i] = 0.f;
  }
  for (int pb = it.pbeg; pb < it.pend; pb += PC) {
    // row r = (tensor * NT + node) * PC + pixel
    auto row_src = [&](int r, int cc, bool& ok) -> const T* {
      const int p = r % PC, q = r / PC;
      const int node = q % NT, ten = q / NT;
      ok = node < n && pb + p < it.pend && cc < a.C;
      const int64_t ns = ten ? a.g.ns : a.x.ns, ps = ten ? a.g.ps : a.x.ps;
      return (ten ? gbase : xb) + (int64_t)node * ns + (int64_t)(pb + p) * ps + cc;
    };
    if constexpr (VECP) {
      constexpr int VW = 16 / (int)sizeof(T), LR = 64 / VW, ITEMS = ROWS * LR / kBlock;
      static_assert(ROWS * LR % kBlock == 0, "whole rounds of 16-byte pieces");
      f4 reg[ITEMS];
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {  // every load of the chunk issued before the first LDS write
        const int t = tid + i * kBlock;
        bool ok;
        const T* src = row_src(t / LR, it.c0 + (t % LR) * VW, ok);
        reg[i] = ok ? *reinterpret_cast<const f4*>(src) : (f4)(0.f);
      }
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        const int t = tid + i * kBlock;
        *reinterpret_cast<f4*>(st + (t / LR) * 64 + (t % LR) * VW) = reg[i];
      }
    } else {
      for (int t = tid; t < ROWS * 64; t += kBlock) {
        bool ok;
        const T* src = row_src(t >> 6, it.c0 + (t & 63), ok);
        st[t] = ok ? *src : (T)0.f;
      }
    }
    __syncthreads();
    if (act && vb0 < n) {
#pragma unroll
      for (int p = pg; p < PC; p += PG) {
        if (pb + p >= it.pend) break;
        float xr[NT], gr[VB];
#pragma unroll
        for (int u = 0; u < NT; ++u) xr[u] = u < n ? (float)st[(u * PC + p) * 64 + lane] : 0.f;
#pragma unroll
        for (int i = 0; i < VB; ++i) gr[i] = vb0 + i < n ? (float)st[((NT + vb0 + i) * PC + p) * 64 + lane] : 0.f;
#pragma unroll
        for (int i = 0; i < VB; ++i) {
          S[i] += gr[i];
#pragma unroll
          for (int u = 0; u < NT; ++u) D[i][u] = fmaf(gr[i], xr[u], D[i][u]);
        }
      }
    }
    __syncthreads();
  }
  if constexpr (PG > 1) {  // the pixel groups' partial sums, added in wave order
    for (int r = 1; r < PG; ++r) {
      if (pg == r) {
#pragma unroll
        for (int i = 0; i < VB; ++i) {
#pragma unroll
          for (int u = 0; u < NT; ++u) red[(i * ROW + u) * 64 + lane] = D[i][u];
          red[(i * ROW + NT) * 64 + lane] = S[i];
        }
      }
      __syncthreads();
      if (pg == 0) {
#pragma unroll
        for (int i = 0; i < VB; ++i) {
#pragma unroll
          for (int u = 0; u < NT; ++u) D[i][u] += red[(i * ROW + u) * 64 + lane];
          S[i] += red[(i * ROW + NT) * 64 + lane];
        }
      }
      __syncthreads();
    }
  }
  if (pg != 0 || !act) return;
  if (a.nseg > 1) {
    float* w = a.ws + ((int64_t)blockIdx.x * NT * ROW) * 64 + lane;  // blockIdx.x = item * nseg + seg
#pragma unroll
    for (int i = 0; i < VB; ++i) {
#pragma unroll
      for (int u = 0; u < NT; ++u) w[((vb0 + i) * ROW + u) * 64] = D[i][u];
      w[((vb0 + i) * ROW + NT) * 64] = S[i];
    }
    return;
  }
  gram_emit<NT, VB>(a, it, c, vb0, D, S);
}

// Second pass of a split plane: one workgroup per (graph, channel block), its four waves each taking
// NT / 4 destinations; a segment's partial sums are loaded as one batch of independent loads and added
// in segment order.
template <int NT>
__global__ void __launch_bounds__(kBlock) film_gram_finish_cl(ClArgs a) {
  typedef typename ClVec<NT>::type vnt;
  constexpr int VB = NT / 4, ROW = ClGram<NT>::ROW;
  ClItem it;
  it.b = blockIdx.x / a.ncb;
  it.cbi = blockIdx.x - it.b * a.ncb;
  it.seg = 0;
  it.node0 = a.kind == kClComplete ? it.b * a.nmax : a.goff[it.b];
  it.n = a.kind == kClComplete ? a.nmax : min(a.goff[it.b + 1] - it.node0, NT);
  it.c0 = it.cbi * a.cb;
  it.pbeg = it.pend = 0;
  if (it.n <= 0) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int vb0 = wave * VB;
  const int c = it.c0 + lane;
  if (c >= a.C || vb0 >= it.n) return;
  vnt D[VB];
  float S[VB];
#pragma unroll
  for (int i = 0; i < VB; ++i) {
    D[i] = (vnt)(0.f);
    S[i] = 0.f;
  }
  for (int seg = 0; seg < a.nseg; ++seg) {
    const float* w = a.ws + (((int64_t)blockIdx.x * a.nseg + seg) * NT * ROW) * 64 + lane;
    float t[VB][ROW];
#pragma unroll
    for (int i = 0; i < VB; ++i)
#pragma unroll
      for (int u = 0; u < ROW; ++u) t[i][u] = w[((vb0 + i) * ROW + u) * 64];
#pragma unroll
    for (int i = 0; i < VB; ++i) {
#pragma unroll
      for (int u = 0; u < NT; ++u) D[i][u] += t[i][u];
      S[i] += t[i][NT];
    }
  }
  gram_emit<NT, VB>(a, it, c, vb0, D, S);
}

}  // namespace mrp

// ---------------------------------------------------------------------------
// Host side shared by film_mean_cl_fwd.hip and film_mean_cl_bwd.hip.
// ---------------------------------------------------------------------------
namespace mrp_host {

using mrp::ClArgs;
using mrp::ClTensor;

inline int cl_elem_size(int32_t dtype) { return dtype == MRP_DTYPE_F32 ? 4 : 2; }
inline bool cl_dtype_ok(int32_t dtype) {
  return dtype == MRP_DTYPE_F32 || dtype == MRP_DTYPE_BF16 || dtype == MRP_DTYPE_F16;
}
// compile-time node capacity of the kernels: 4, 8 or 16
inline int cl_nt_class(int max_nodes) { return max_nodes <= 4 ? 4 : (max_nodes <= 8 ? 8 : 16); }
inline int cl_pow2_ceil(int v) {
  int p = 1;
  while (p < v) p *= 2;
  return p;
}

// Checks of one (pointer, node stride, pixel stride) triple, accumulated over a call's tensors.
struct ClCheck {
  int32_t C, P;
  int es;
  bool invalid = false;      // hipErrorInvalidValue
  bool unsupported = false;  // hipErrorNotSupported: a lane's 32-bit byte offset would not hold a node's span
  bool vec = true;           // every tensor allows 16-byte channel vectors
  ClTensor add(const void* p, int64_t ns, int64_t ps) {
    if (p == nullptr || ps < C || ns < (int64_t)P * ps) invalid = true;
    if (ps > 0 && (int64_t)P * ps * es >= ((int64_t)1 << 31)) unsupported = true;
    if ((reinterpret_cast<uintptr_t>(p) & 15u) != 0 || (ns * es) % 16 != 0 || (ps * es) % 16 != 0) vec = false;
    return ClTensor{p, ns, ps};
  }
};

// Pixel segments of a sweep: enough workgroups to fill the chip, none shorter than min_pixels
// (a multiple of `granule`, the pixels a workgroup takes per pass).
inline void cl_segments(int64_t items, int P, int granule, int min_pixels, int32_t& nseg, int32_t& seglen) {
  const int64_t want = std::max<int64_t>(1, (2048 + items - 1) / items);
  const int64_t most = std::max<int64_t>(1, P / std::max(min_pixels, 1));
  int64_t ns = std::min(want, most);
  int64_t len = (P + ns - 1) / ns;
  len = (len + granule - 1) / granule * granule;
  seglen = (int32_t)len;
  nseg = (int32_t)((P + len - 1) / len);
}

// Gram pass geometry: 64 channels per workgroup; the plane is split when the graphs and channel
// blocks alone do not fill the chip.  A function of the sizes only (the workspace query repeats it).
struct ClGramGeom {
  int32_t ncb, nseg, seglen;
  int64_t ws_bytes;
};
inline ClGramGeom cl_gram_geometry(int32_t num_graphs, int32_t max_nodes, int32_t C, int32_t P) {
  ClGramGeom g;
  g.ncb = (C + 63) / 64;
  cl_segments((int64_t)num_graphs * g.ncb, P, 4, 64, g.nseg, g.seglen);
  const int nt = cl_nt_class(max_nodes);
  g.ws_bytes = g.nseg > 1 ? (int64_t)num_graphs * g.ncb * g.nseg * nt * (nt + 1) * 64 * (int64_t)sizeof(float) : 0;
  return g;
}

}  // namespace mrp_host
