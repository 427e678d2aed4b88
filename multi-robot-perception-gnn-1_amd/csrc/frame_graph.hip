// frame_graph.hip — per-frame robot graphs built on the GPU (gfx950 / MI355X).
//
// Replaces the host-side graph construction of the reference's dataset path:
//   edge list   dgl/dataloader.py:88-95   every ordered pair i != j, i-major
//   edge feature dgl/dataloader.py:116-122 cal_relative_pose(pose_i, pose_j) per edge
//   relative pose dgl/utils.py:54-77     [t_j - t_i, first two columns of R(conj(q_i) q_j)]
// plus the k-NN(k) topology of the BASELINE configs (the reference builds complete graphs only):
// each destination v takes the k robots u != v nearest to it, |t_u - t_v| in float64 with ties to
// the lower index, listed in ascending u (the host builder `graph.knn_edges` in device form).
//
// One thread per (graph, destination robot): it selects v's in-edges, writes their relative poses,
// its CSR row (indptr, src, eid) and, for v == 0, its graph's node offset.  Work per batch is a few
// hundred threads: the point is to keep the per-batch host work (numpy loops, a host-to-device copy
// of the edge features) off the training step, not bandwidth.
//
// Arithmetic follows the reference's float32 numpy expression order exactly (compiled with
// -ffp-contract=off, no FMA contraction), so edge poses are bit-identical to the host path
// (`pose.relative_pose_batch` on float32 rows, itself pinned to the reference's own outputs).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mrp_gnn.h"

namespace mrp_graph {

constexpr int kThreads = 128;

// cal_relative_pose(p1 = source, p2 = destination), dgl/utils.py:69-77, float32.
__device__ __forceinline__ void relative_pose(const float* p1, const float* p2, float* out) {
  const float x1 = -p1[3], y1 = -p1[4], z1 = -p1[5], w1 = p1[6];  // conjugate of q1
  const float x2 = p2[3], y2 = p2[4], z2 = p2[5], w2 = p2[6];
  // q2 * q1^-1 in the reference's expansion, evaluated left to right
  const float x = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(w1, x2), __fmul_rn(x1, w2)), __fmul_rn(y1, z2)),
                            __fmul_rn(z1, y2));
  const float y = __fadd_rn(__fadd_rn(__fsub_rn(__fmul_rn(w1, y2), __fmul_rn(x1, z2)), __fmul_rn(y1, w2)),
                            __fmul_rn(z1, x2));
  const float z = __fadd_rn(__fsub_rn(__fadd_rn(__fmul_rn(w1, z2), __fmul_rn(x1, y2)), __fmul_rn(y1, x2)),
                            __fmul_rn(z1, w2));
  const float w = __fsub_rn(__fsub_rn(__fsub_rn(__fmul_rn(w1, w2), __fmul_rn(x1, x2)), __fmul_rn(y1, y2)),
                            __fmul_rn(z1, z2));
  out[0] = __fsub_rn(p2[0], p1[0]);
  out[1] = __fsub_rn(p2[1], p1[1]);
  out[2] = __fsub_rn(p2[2], p1[2]);
  // quat_to_so3 (dgl/utils.py:54-66), first six entries: a00 a10 a20 a01 a11 a21
  const float yy = __fmul_rn(y, y), zz = __fmul_rn(z, z), xx = __fmul_rn(x, x);
  out[3] = __fsub_rn(__fsub_rn(1.f, __fmul_rn(2.f, yy)), __fmul_rn(2.f, zz));
  out[4] = __fadd_rn(__fmul_rn(__fmul_rn(2.f, x), y), __fmul_rn(__fmul_rn(2.f, z), w));
  out[5] = __fsub_rn(__fmul_rn(__fmul_rn(2.f, x), z), __fmul_rn(__fmul_rn(2.f, y), w));
  out[6] = __fsub_rn(__fmul_rn(__fmul_rn(2.f, x), y), __fmul_rn(__fmul_rn(2.f, z), w));
  out[7] = __fsub_rn(__fsub_rn(1.f, __fmul_rn(2.f, xx)), __fmul_rn(2.f, zz));
  out[8] = __fadd_rn(__fmul_rn(__fmul_rn(2.f, y), z), __fmul_rn(__fmul_rn(2.f, x), w));
}

__device__ __forceinline__ void write_pose(float* edge_pose, int64_t e, const float* p) {
  if (edge_pose == nullptr) return;
#pragma unroll
  for (int i = 0; i < 9; ++i) edge_pose[e * 9 + i] = p[i];
}

__global__ void __launch_bounds__(kThreads) frame_graph_build(const float* __restrict__ poses, int B, int n, int k,
                                                             float* __restrict__ edge_pose, int32_t* __restrict__ indptr,
                                                             int32_t* __restrict__ src, int32_t* __restrict__ eid,
                                                             int32_t* __restrict__ goff) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nt = (int64_t)B * n;
  if (t >= nt) return;
  const int b = (int)(t / n);
  const int v = (int)(t - (int64_t)b * n);
  const int64_t node0 = (int64_t)b * n;
  const float* pv = poses + t * 7;
  if (goff != nullptr && v == 0) {
    goff[b] = (int32_t)node0;
    if (b == B - 1) goff[B] = (int32_t)nt;
  }
  float rel[9];
  if (k == 0) {
    // complete graph: in-edges of v are u = 0..n-1, u != v, at edge id b*n(n-1) + u(n-1) + (v<u ? v : v-1)
    const int64_t ebase = (int64_t)b * n * (n - 1);
    const int64_t row = ebase + (int64_t)v * (n - 1);  // CSR row start = v's rank among destinations
    if (indptr != nullptr) {
      indptr[t] = (int32_t)row;
      if (t == nt - 1) indptr[nt] = (int32_t)(nt * (n - 1));
    }
    int j = 0;
    for (int u = 0; u < n; ++u) {
      if (u == v) continue;
      const int64_t e = ebase + (int64_t)u * (n - 1) + (v < u ? v : v - 1);
      relative_pose(poses + (node0 + u) * 7, pv, rel);
      write_pose(edge_pose, e, rel);
      if (src != nullptr) src[row + j] = (int32_t)(node0 + u);
      if (eid != nullptr) eid[row + j] = (int32_t)e;
      ++j;
    }
    return;
  }
  // k-NN: k nearest sources by float64 Euclidean distance of the translations (numpy's
  // norm: sqrt((dx^2 + dy^2) + dz^2)), ties to the lower index
  double d[MRP_MAX_NODES];
  const double tvx = pv[0], tvy = pv[1], tvz = pv[2];
  for (int u = 0; u < n; ++u) {
    const float* pu = poses + (node0 + u) * 7;
    const double dx = __dsub_rn((double)pu[0], tvx);
    const double dy = __dsub_rn((double)pu[1], tvy);
    const double dz = __dsub_rn((double)pu[2], tvz);
    d[u] = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
  }
  unsigned chosen = 0u;
  for (int j = 0; j < k; ++j) {
    int best = -1;
    for (int u = 0; u < n; ++u) {
      if (u == v || ((chosen >> u) & 1u)) continue;
      if (best < 0 || d[u] < d[best]) best = u;  // strict: equal distance keeps the lower index
    }
    chosen |= 1u << best;
  }
  const int64_t row = t * k;
  if (indptr != nullptr) {
    indptr[t] = (int32_t)row;
    if (t == nt - 1) indptr[nt] = (int32_t)(nt * k);
  }
  int j = 0;
  for (int u = 0; u < n; ++u) {
    if (!((chosen >> u) & 1u)) continue;
    const int64_t e = row + j;  // edges are numbered destination-major, sources ascending
    relative_pose(poses + (node0 + u) * 7, pv, rel);
    write_pose(edge_pose, e, rel);
    if (src != nullptr) src[e] = (int32_t)(node0 + u);
    if (eid != nullptr) eid[e] = (int32_t)e;
    ++j;
  }
}

// ---------------------------------------------------------------------------
// Range-limited / drop-out frames (mrp_frame_graph_build_range): the in-degrees differ per robot, so the
// CSR row starts are a prefix sum over all B n destinations.  Three launches, no atomics (the sum is a
// fixed tree: the same bits every run) and nothing read back by the host:
//   range_rows   one thread per destination: its in-edge mask (16 bits) and every ordered pair's pose
//                row (the complete numbering, so the encoder's rows line up whatever edges exist);
//                the workgroup's exclusive scan of the in-degrees and its total
//   range_blocks one workgroup: exclusive scan of the workgroup totals, and indptr's terminator
//   range_fill   one thread per destination: its row start, src and eid from the mask
// Workspace (int32): [nt] masks, [nt] in-workgroup prefixes, [blocks] workgroup totals / offsets.
// ---------------------------------------------------------------------------
constexpr int kScan = 256;

// Exclusive scan of one value per thread over the workgroup (every thread calls it); total: the sum.
__device__ __forceinline__ int block_exclusive_scan(int v, int* sh, int& total) {
  const int i = threadIdx.x;
  sh[i] = v;
  __syncthreads();
  for (int d = 1; d < kScan; d <<= 1) {
    const int add = i >= d ? sh[i - d] : 0;
    __syncthreads();
    sh[i] += add;
    __syncthreads();
  }
  const int incl = sh[i];
  total = sh[kScan - 1];
  __syncthreads();
  return incl - v;
}

__global__ void __launch_bounds__(kScan) range_rows(const float* __restrict__ poses,
                                                    const uint8_t* __restrict__ active, int B, int n, int k,
                                                    double max_range, float* __restrict__ edge_pose,
                                                    int32_t* __restrict__ goff, int32_t* __restrict__ masks,
                                                    int32_t* __restrict__ prefix, int32_t* __restrict__ totals) {
  __shared__ int sh[kScan];
  const int64_t t = (int64_t)blockIdx.x * kScan + threadIdx.x;
  const int64_t nt = (int64_t)B * n;
  unsigned mask = 0u;
  if (t < nt) {
    const int b = (int)(t / n);
    const int v = (int)(t - (int64_t)b * n);
    const int64_t node0 = (int64_t)b * n;
    const float* pv = poses + t * 7;
    if (goff != nullptr && v == 0) {
      goff[b] = (int32_t)node0;
      if (b == B - 1) goff[B] = (int32_t)nt;
    }
    const int64_t ebase = (int64_t)b * n * (n - 1);
    const bool von = active == nullptr || active[t] != 0;
    double d[MRP_MAX_NODES];
    const double tvx = pv[0], tvy = pv[1], tvz = pv[2];
    unsigned cand = 0u;  // sources in range of v
    float rel[9];
    for (int u = 0; u < n; ++u) {
      if (u == v) continue;
      const float* pu = poses + (node0 + u) * 7;
      if (edge_pose != nullptr) {
        relative_pose(pu, pv, rel);
        write_pose(edge_pose, ebase + (int64_t)u * (n - 1) + (v < u ? v : v - 1), rel);
      }
      const double dx = __dsub_rn((double)pu[0], tvx);
      const double dy = __dsub_rn((double)pu[1], tvy);
      const double dz = __dsub_rn((double)pu[2], tvz);
      d[u] = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
      const bool uon = active == nullptr || active[node0 + u] != 0;
      if (von && uon && d[u] <= max_range) cand |= 1u << u;  // inclusive; false for a NaN distance
    }
    if (k > 0 && __popc(cand) > k) {
      // the k nearest of the candidates, ties to the lower index
      for (int j = 0; j < k; ++j) {
        int best = -1;
        for (int u = 0; u < n; ++u) {
          if (!((cand >> u) & 1u) || ((mask >> u) & 1u)) continue;
          if (best < 0 || d[u] < d[best]) best = u;
        }
        mask |= 1u << best;
      }
    } else {
      mask = cand;
    }
    masks[t] = (int32_t)mask;
  }
  int total;
  const int ex = block_exclusive_scan(__popc(mask), sh, total);
  if (t < nt) prefix[t] = ex;
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// One workgroup: the workgroup totals become exclusive offsets, chunk by chunk with a running carry.
__global__ void __launch_bounds__(kScan) range_blocks(int32_t* __restrict__ totals, int nblocks,
                                                      int32_t* __restrict__ indptr, int64_t nt) {
  __shared__ int sh[kScan];
  int carry = 0;
  for (int base = 0; base < nblocks; base += kScan) {
    const int i = base + (int)threadIdx.x;
    const int v = i < nblocks ? totals[i] : 0;
    int total;
    const int ex = block_exclusive_scan(v, sh, total);
    if (i < nblocks) totals[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0 && indptr != nullptr) indptr[nt] = carry;
}

__global__ void __launch_bounds__(kScan) range_fill(int B, int n, const int32_t* __restrict__ masks,
                                                    const int32_t* __restrict__ prefix,
                                                    const int32_t* __restrict__ offsets, int32_t* __restrict__ indptr,
                                                    int32_t* __restrict__ src, int32_t* __restrict__ eid) {
  const int64_t t = (int64_t)blockIdx.x * kScan + threadIdx.x;
  const int64_t nt = (int64_t)B * n;
  if (t >= nt) return;
  const int b = (int)(t / n);
  const int v = (int)(t - (int64_t)b * n);
  const int64_t node0 = (int64_t)b * n;
  const int64_t ebase = (int64_t)b * n * (n - 1);
  const unsigned mask = (unsigned)masks[t];
  int row = offsets[blockIdx.x] + prefix[t];
  if (indptr != nullptr) indptr[t] = row;
  for (int u = 0; u < n; ++u) {
    if (!((mask >> u) & 1u)) continue;
    if (src != nullptr) src[row] = (int32_t)(node0 + u);
    if (eid != nullptr) eid[row] = (int32_t)(ebase + (int64_t)u * (n - 1) + (v < u ? v : v - 1));
    ++row;
  }
}

}  // namespace mrp_graph

extern "C" int64_t mrp_frame_graph_build_range_workspace(int32_t num_graphs, int32_t n) {
  if (num_graphs <= 0 || n <= 0) return 0;
  const int64_t nt = (int64_t)num_graphs * n;
  const int64_t blocks = (nt + mrp_graph::kScan - 1) / mrp_graph::kScan;
  return (2 * nt + blocks) * (int64_t)sizeof(int32_t);
}

extern "C" int mrp_frame_graph_build_range(const float* poses, const uint8_t* active, int32_t num_graphs, int32_t n,
                                           int32_t knn_k, double max_range, float* edge_pose, int32_t* indptr,
                                           int32_t* src, int32_t* eid, int32_t* graph_off, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
  if (num_graphs < 0 || n < 0 || n > MRP_MAX_NODES || knn_k < 0) return hipErrorInvalidValue;
  if (knn_k > 0 && knn_k >= n) return hipErrorInvalidValue;
  if (!(max_range >= 0.0)) return hipErrorInvalidValue;  // negative or NaN
  const int64_t nt = (int64_t)num_graphs * n;
  const int64_t ne = nt * (n > 0 ? n - 1 : 0);
  if (nt >= 0x7fffffff || ne >= 0x7fffffff) return hipErrorInvalidValue;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (nt == 0) {
    if (graph_off != nullptr) {
      hipError_t e = hipMemsetAsync(graph_off, 0, sizeof(int32_t) * ((size_t)num_graphs + 1), st);
      if (e != hipSuccess) return e;
    }
    if (indptr != nullptr) return hipMemsetAsync(indptr, 0, sizeof(int32_t), st);
    return hipSuccess;
  }
  if (poses == nullptr || workspace == nullptr || (reinterpret_cast<uintptr_t>(workspace) & 3u) != 0 ||
      workspace_bytes < mrp_frame_graph_build_range_workspace(num_graphs, n))
    return hipErrorInvalidValue;
  const int blocks = (int)((nt + mrp_graph::kScan - 1) / mrp_graph::kScan);
  int32_t* masks = static_cast<int32_t*>(workspace);
  int32_t* prefix = masks + nt;
  int32_t* totals = prefix + nt;
  hipLaunchKernelGGL(mrp_graph::range_rows, dim3((unsigned)blocks), dim3(mrp_graph::kScan), 0, st, poses, active,
                     (int)num_graphs, (int)n, (int)knn_k, max_range, edge_pose, graph_off, masks, prefix, totals);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mrp_graph::range_blocks, dim3(1), dim3(mrp_graph::kScan), 0, st, totals, blocks, indptr, nt);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mrp_graph::range_fill, dim3((unsigned)blocks), dim3(mrp_graph::kScan), 0, st, (int)num_graphs,
                     (int)n, masks, prefix, totals, indptr, src, eid);
  return hipGetLastError();
}

extern "C" int mrp_frame_graph_build(const float* poses, int32_t num_graphs, int32_t n, int32_t knn_k,
                                     float* edge_pose, int32_t* indptr, int32_t* src, int32_t* eid,
                                     int32_t* graph_off, void* stream) {
  if (num_graphs < 0 || n < 0 || n > MRP_MAX_NODES || knn_k < 0) return hipErrorInvalidValue;
  if (knn_k > 0 && knn_k >= n) return hipErrorInvalidValue;  // k-NN needs k < n (knn_edges raises too)
  const int64_t nt = (int64_t)num_graphs * n;
  const int64_t ne = knn_k > 0 ? nt * knn_k : nt * (n > 0 ? n - 1 : 0);
  if (nt >= 0x7fffffff || ne >= 0x7fffffff) return hipErrorInvalidValue;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (nt == 0) {
    // no nodes: only the offsets (all zero) and the CSR terminator exist
    if (graph_off != nullptr && num_graphs >= 0) {
      hipError_t e = hipMemsetAsync(graph_off, 0, sizeof(int32_t) * ((size_t)num_graphs + 1), st);
      if (e != hipSuccess) return e;
    }
    if (indptr != nullptr) return hipMemsetAsync(indptr, 0, sizeof(int32_t), st);
    return hipSuccess;
  }
  if (poses == nullptr) return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((nt + mrp_graph::kThreads - 1) / mrp_graph::kThreads);
  hipLaunchKernelGGL(mrp_graph::frame_graph_build, dim3(blocks), dim3(mrp_graph::kThreads), 0, st, poses,
                     (int)num_graphs, (int)n, (int)knn_k, edge_pose, indptr, src, eid, graph_off);
  return hipGetLastError();
}
