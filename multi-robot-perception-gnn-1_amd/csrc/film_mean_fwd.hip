// film_mean_fwd.hip — forward launchers and C ABI (mrp_film_mean_fwd, mrp_film_mean_cat_fwd).
// Kernels and design notes: film_mean_kernels.hpp.
#include <cstring>
#include <unordered_map>

#include "film_mean_fwd_launch.hpp"

using namespace mrp_host;

// The streaming yardstick beside the aggregation rooflines (mrp_stream_copy): one nontemporal 16-byte
// load and store per thread per trip, grid-stride, 256 threads, one trip per thread where the grid
// allows (tools/copy_ceiling.hip's copy1, the best of round 1's copy sweep).
__global__ void __launch_bounds__(256) stream_copy(const mrp::f4* __restrict__ in, mrp::f4* __restrict__ out,
                                                   size_t n) {
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    __builtin_nontemporal_store(__builtin_nontemporal_load(in + i), out + i);
}

namespace mrp_host {
Tuning& tuning() {
  static Tuning t;
  return t;
}

int film_fwd_plan(size_t elem, const void* x, int64_t x_node_stride, const float* gb, const int32_t* indptr,
                  const int32_t* src, const int32_t* eid, const int32_t* graph_off, int32_t num_graphs,
                  int32_t max_nodes, int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P,
                  int32_t mode_flags, void* out, int64_t out_node_stride, const mrp_agg_epilogue* ep, AggArgs& a,
                  Geometry& g, size_t xelem) {
  g = Geometry();  // kernel = MRP_AGG_KERNEL_NONE until a launch is planned
  const bool half = elem == 2;  // 16-bit features (kHalfIo)
  const bool quant = xelem != 0 && xelem != elem;  // FP8 messages: x holds 1-byte codes
  void* xcopy = ep != nullptr ? ep->xcopy : nullptr;
  const int64_t xcopy_node_stride = ep != nullptr ? ep->xcopy_node_stride : 0;
  const void* x0 = ep != nullptr ? ep->x0 : nullptr;
  const int64_t x0_node_stride = ep != nullptr ? ep->x0_node_stride : 0;
  const int32_t logits = (mode_flags & MRP_AGG_GB_LOGITS) ? 1 : 0;
  const int32_t mode = mode_flags & ~MRP_AGG_GB_LOGITS;
  if (!common_args_ok(indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P,
                      mode))
    return hipErrorInvalidValue;
  if (num_graphs == 0 || num_nodes == 0 || max_nodes == 0 || C == 0 || P == 0) return hipSuccess;
  const int64_t plane = (int64_t)C * P;
  if (x == nullptr || out == nullptr || x_node_stride < plane || out_node_stride < plane)
    return hipErrorInvalidValue;
  if (mode != MRP_AGG_COPY_MEAN && num_edges > 0 && gb == nullptr) return hipErrorInvalidValue;
  if (xcopy != nullptr && xcopy_node_stride < plane) return hipErrorInvalidValue;
  if (x0 != nullptr && x0_node_stride < plane) return hipErrorInvalidValue;
  SliceCheck sc, scx;  // scx: the 1-byte input of the FP8 path, checked at its own element size
  sc.strides = scx.strides = P;
  (quant ? scx : sc).add(x, x_node_stride);
  sc.add(out, out_node_stride);
  if (xcopy != nullptr) sc.add(xcopy, xcopy_node_stride);
  if (x0 != nullptr) sc.add(x0, x0_node_stride);
  const int32_t kdeg = MRP_GRAPH_IS_REGULAR(graph_kind) ? MRP_GRAPH_REGULAR_K(graph_kind) : 0;
  const bool regular = kdeg >= 1 && kdeg <= 8;
  const Tuning& tu = tuning();
  int fvec, rvec;  // slice width of film_fwd / film_fwd_regular
  if (quant) {
    // the widest slice (elements) for which the codes (1 byte) and out / x0 (elem bytes) are both aligned:
    // 8 (<= 8 nodes, 16-bit outputs: an 8-byte load, 16-byte stores), 4 (a 4-byte load, 8- or 16-byte
    // stores), else single elements
    const bool ok8 = elem == 2 && max_nodes <= 8 && scx.ok(8, xelem) && sc.ok(8, elem);
    fvec = rvec = ok8 ? 8 : ((scx.ok(4, xelem) && sc.ok(4, elem)) ? 4 : 1);
  } else if (half) {
    // 16-byte slices of 8 elements (graphs of <= 8 nodes: beyond, 8 slices of 16 sources are 128 live
    // registers before the first product), else 8-byte slices of 4, else single elements
    fvec = rvec = (max_nodes <= 8 && sc.ok(8, elem)) ? 8 : (sc.ok(4, elem) ? 4 : 1);
  } else {
    // 16-byte slices beat 8-byte ones at every measured size (tools/kernel_lab.hip product sweep)
    const bool vec4 = sc.ok(4, elem);
    fvec = vec4 ? (P < tu.fwd_vec2_below ? 2 : 4) : 1;
    rvec = vec4 ? 4 : 1;
  }
  g = regular ? make_geometry(C, P, rvec, tu.fwd_regular_lo, tu.fwd_regular_hi, tu.fwd_regular_cap)
              : make_geometry(C, P, fvec, tu.fwd_lo, tu.fwd_hi, tu.fwd_cap);
  g.kernel = regular ? MRP_AGG_KERNEL_FILM_FWD_REGULAR : MRP_AGG_KERNEL_FILM_FWD;
  g.kmax = regular ? (kdeg <= 4 ? 4 : 8) : 0;
  // (at most 16 channels of 16-node tiles: 33 KiB, under kMaxDynamicLds at every setting)
  g.lds = regular ? lds_fwd_regular(max_nodes, g.kmax, g.cpb) : lds_fwd(max_nodes, g.cpb);
  // COMPLETE graphs: one slice per lane, the plane split over ceil(PV / lpc) workgroups (their
  // prologue is one round of independent gamma/beta loads, hidden under the first slice).  CSR
  // graphs keep whole planes: their prologue walks the CSR (dependent loads) and a split repeats it
  // per segment (k-NN(4) N=16 C=1024 16x16: 304 us split vs 225 us whole)
  const int32_t pv = P / g.vec;
  g.psplit = (graph_kind == MRP_GRAPH_COMPLETE || (regular && tu.fwd_regular_split)) ? (pv + g.lpc - 1) / g.lpc : 1;
  g.grid = (int64_t)num_graphs * g.ncb * g.psplit;
  if (g.grid > 0x7fffffff) return hipErrorInvalidValue;
  a = {};
  a.x = x;
  a.xs = x_node_stride;
  a.gb = gb;
  a.indptr = indptr;
  a.src = src;
  a.eid = eid;
  a.goff = graph_off;
  a.out = out;
  a.os = out_node_stride;
  a.C = C;
  a.P = P;
  a.PV = P / g.vec;
  a.mode = mode;
  a.lpc = g.lpc;
  a.cpb = g.cpb;
  a.ncb = g.ncb;
  a.logits = logits;
  a.xc = xcopy;
  a.xcs = xcopy_node_stride;
  a.psplit = g.psplit;
  a.kdeg = kdeg;
  a.agg_scale = 1.f;
  if (ep != nullptr) {
    a.agg_scale = ep->agg_scale;
    a.self_scale = ep->self_scale;
    a.x0 = x0;
    a.x0s = x0_node_stride;
    a.x0_scale = ep->x0_scale;
    a.epi = (ep->agg_scale != 1.f || ep->self_scale != 0.f || x0 != nullptr) ? 1 : 0;
  }
  return hipSuccess;
}

// A planner's result as the C ABI's mrp_agg_plan.
void fill_plan(const Geometry& g, int want_dx, int want_dgb, mrp_agg_plan* plan) {
  *plan = {};
  plan->kernel = g.kernel;
  if (g.kernel == MRP_AGG_KERNEL_NONE) return;
  plan->vec = g.vec;
  plan->lpc = g.lpc;
  plan->cpb = g.cpb;
  plan->threads = g.threads;
  plan->psplit = g.psplit;
  plan->ncb = g.ncb;
  plan->pre2 = g.pre2;
  plan->grid = g.grid;
  size_t lds = g.lds;
  if (g.kernel == MRP_AGG_KERNEL_FILM_BWD_DX_GRAM)  // the launches made: film_bwd_dx and / or the Gram pass
    lds = std::max(want_dx ? g.lds_dx : (size_t)0, want_dgb ? g.lds : (size_t)0);
  plan->lds_bytes = (int64_t)lds;
}
}  // namespace mrp_host

extern "C" {

int mrp_abi_version(void) { return 22; }

int mrp_tuning_set(const char* name, int32_t value) {
  if (name == nullptr) return hipErrorInvalidValue;
  Tuning& t = tuning();
  if (std::strcmp(name, "reset") == 0) {
    t = Tuning();
    return hipSuccess;
  }
  struct Knob {
    const char* name;
    int* field;
    int lo, hi;
  } knobs[] = {
      {"fwd_lo", &t.fwd_lo, 1, 256},
      {"fwd_hi", &t.fwd_hi, 1, 256},
      {"fwd_cap", &t.fwd_cap, 1, 16},
      {"fwd_vec2_below", &t.fwd_vec2_below, 0, 1 << 20},
      {"fwd_regular_split", &t.fwd_regular_split, 0, 1},
      {"fwd_regular_lo", &t.fwd_regular_lo, 1, 256},
      {"fwd_regular_hi", &t.fwd_regular_hi, 1, 256},
      {"fwd_regular_cap", &t.fwd_regular_cap, 1, 16},
      {"bwd_fused_lo", &t.bwd_fused_lo, 1, 256},
      {"bwd_fused_hi", &t.bwd_fused_hi, 1, 256},
      {"bwd_fused_cap", &t.bwd_fused_cap, 1, 64},
      {"bwd_pre2", &t.bwd_pre2, 0, 2},
      {"bwd_regular_vec", &t.bwd_regular_vec, 1, 2},
      {"bwd_regular_lanes", &t.bwd_regular_lanes, 1, 64},
      {"bwd_regular_mfma", &t.bwd_regular_mfma, 0, 1},
      {"bwd_complete_mfma", &t.bwd_complete_mfma, 0, 1},
      {"bwd_mfma_cpw", &t.bwd_mfma_cpw, 1, 2},
      {"bwd_half_mfma", &t.bwd_half_mfma, 0, 1},
      {"edge_split_v", &t.edge_split_v, -1, 3},
      {"edge_allx", &t.edge_allx, 0, 1},
      {"gemm_split", &t.gemm_split, -1, 7},
      {"split_nt", &t.split_nt, -1, 4},
      {"gemm_group", &t.gemm_group, 0, 64},
      {"nt_group", &t.nt_group, 0, 64},
      {"enc_bwd_psa", &t.enc_bwd_psa, 0, 2},
      {"enc_s1", &t.enc_s1, 0, 64},
      {"enc_s2", &t.enc_s2, 0, 64},
      {"compress_half", &t.compress_half, 0, 1},
      {"half_nt_splits", &t.half_nt_splits, 0, 256},
      {"compress_half_cl", &t.compress_half_cl, 0, 1},
      {"half_cl_splits", &t.half_cl_splits, 0, 256},
      {"compress_split_cl", &t.compress_split_cl, 0, 1},
      {"split_cl_splits", &t.split_cl_splits, 0, 256},
  };
  for (const Knob& k : knobs) {
    if (std::strcmp(name, k.name) == 0) {
      if (value < k.lo || value > k.hi) return hipErrorInvalidValue;
      // knobs that name kernels accept only the product's: gemm_split -1 (per shape), 2 or 7;
      // split_nt -1 (per shape), 3 or 4 (compress_split.hip; round 4's other forms: tools/lab_forms.hip)
      if (k.field == &t.gemm_split && value != -1 && value != 2 && value != 7) return hipErrorInvalidValue;
      if (k.field == &t.split_nt && value != -1 && value != 3 && value != 4) return hipErrorInvalidValue;
      if (k.field == &t.edge_split_v && value != -1 && value != 1 && value != 3) return hipErrorInvalidValue;
      *k.field = value;
      return hipSuccess;
    }
  }
  return hipErrorInvalidValue;
}

const char* mrp_error_string(int code) { return hipGetErrorString(static_cast<hipError_t>(code)); }

int mrp_stream_join(void* waiter, void* signaller) {
  if (waiter == signaller) return hipSuccess;
  // one event per signalling stream and host thread, re-recorded each call: a wait enqueued earlier
  // keeps the record it was enqueued behind
  thread_local std::unordered_map<void*, hipEvent_t> events;
  hipEvent_t& ev = events[signaller];
  if (ev == nullptr) {
    const hipError_t c = hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventReleaseToDevice);
    if (c != hipSuccess) {
      ev = nullptr;
      return c;
    }
  }
  hipError_t e = hipEventRecord(ev, static_cast<hipStream_t>(signaller));
  if (e == hipSuccess) e = hipStreamWaitEvent(static_cast<hipStream_t>(waiter), ev, 0);
  return e;
}

int mrp_stream_copy(const void* src, void* dst, int64_t bytes, void* stream) {
  if (bytes < 0 || (bytes % 16) != 0) return hipErrorInvalidValue;
  if (bytes == 0) return hipSuccess;
  if (!src || !dst || !aligned16(src) || !aligned16(dst)) return hipErrorInvalidValue;
  const size_t n = (size_t)bytes / 16;
  const size_t blocks = std::min<size_t>((n + 255) / 256, (size_t)1 << 30);
  hipLaunchKernelGGL(stream_copy, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const mrp::f4*>(src), static_cast<mrp::f4*>(dst), n);
  return hipGetLastError();
}

}  // extern "C"

extern "C" {

int mrp_film_mean_fwd(const float* x, int64_t x_node_stride, const float* gb, const int32_t* indptr,
                      const int32_t* src, const int32_t* eid, const int32_t* graph_off, int32_t num_graphs,
                      int32_t max_nodes, int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C,
                      int32_t P, int32_t mode_flags, float* out, int64_t out_node_stride, void* stream) {
  return film_fwd_impl<float>(x, x_node_stride, gb, indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind,
                       num_nodes, num_edges, C, P, mode_flags, out, out_node_stride, nullptr, stream);
}

int mrp_film_mean_fwd_ex(const float* x, int64_t x_node_stride, const float* gb, const int32_t* indptr,
                         const int32_t* src, const int32_t* eid, const int32_t* graph_off, int32_t num_graphs,
                         int32_t max_nodes, int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C,
                         int32_t P, int32_t mode_flags, float* out, int64_t out_node_stride,
                         const mrp_agg_epilogue* epilogue, void* stream) {
  return film_fwd_impl<float>(x, x_node_stride, gb, indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind,
                       num_nodes, num_edges, C, P, mode_flags, out, out_node_stride, epilogue, stream);
}

int mrp_film_mean_cat_fwd(const float* x, int64_t x_node_stride, const float* gb, const int32_t* indptr,
                          const int32_t* src, const int32_t* eid, const int32_t* graph_off, int32_t num_graphs,
                          int32_t max_nodes, int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C,
                          int32_t P, int32_t mode_flags, float* cat, int64_t cat_node_stride, void* stream) {
  if (cat == nullptr || cat_node_stride < 2 * (int64_t)C * P) return hipErrorInvalidValue;
  mrp_agg_epilogue ep = {1.f, 0.f, nullptr, 0, 0.f, cat, cat_node_stride};
  return film_fwd_impl<float>(x, x_node_stride, gb, indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind,
                       num_nodes, num_edges, C, P, mode_flags, cat + (int64_t)C * P, cat_node_stride, &ep, stream);
}

int mrp_film_mean_fwd_t(int32_t dtype, const void* x, int64_t x_node_stride, const float* gb, const int32_t* indptr,
                        const int32_t* src, const int32_t* eid, const int32_t* graph_off, int32_t num_graphs,
                        int32_t max_nodes, int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C,
                        int32_t P, int32_t mode_flags, void* out, int64_t out_node_stride,
                        const mrp_agg_epilogue* epilogue, void* stream) {
  switch (dtype) {
    case MRP_DTYPE_F32:
      return film_fwd_impl<float>(static_cast<const float*>(x), x_node_stride, gb, indptr, src, eid, graph_off,
                                  num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P, mode_flags,
                                  static_cast<float*>(out), out_node_stride, epilogue, stream);
    case MRP_DTYPE_BF16:
      return film_fwd_bf16(x, x_node_stride, gb, indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind,
                           num_nodes, num_edges, C, P, mode_flags, out, out_node_stride, epilogue, stream);
    case MRP_DTYPE_F16:
      return film_fwd_f16(x, x_node_stride, gb, indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind,
                          num_nodes, num_edges, C, P, mode_flags, out, out_node_stride, epilogue, stream);
    default: return hipErrorInvalidValue;
  }
}

int mrp_film_mean_fwd_plan(int32_t dtype, const void* x, int64_t x_node_stride, const float* gb,
                           const int32_t* indptr, const int32_t* src, const int32_t* eid, const int32_t* graph_off,
                           int32_t num_graphs, int32_t max_nodes, int32_t graph_kind, int32_t num_nodes,
                           int32_t num_edges, int32_t C, int32_t P, int32_t mode_flags, void* out,
                           int64_t out_node_stride, const mrp_agg_epilogue* epilogue, mrp_agg_plan* plan) {
  if (plan == nullptr) return hipErrorInvalidValue;
  if (dtype != MRP_DTYPE_F32 && dtype != MRP_DTYPE_BF16 && dtype != MRP_DTYPE_F16) return hipErrorInvalidValue;
  AggArgs a = {};
  Geometry g;
  const int rc = film_fwd_plan(dtype == MRP_DTYPE_F32 ? 4 : 2, x, x_node_stride, gb, indptr, src, eid, graph_off,
                               num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P, mode_flags, out,
                               out_node_stride, epilogue, a, g);
  if (rc == hipSuccess) fill_plan(g, 0, 0, plan);
  return rc;
}

}  // extern "C"
