// film_mean_bwd.hip — backward C ABI (mrp_film_mean_bwd).  The kernel launches are instantiated
// in film_mean_bwd_{1_8,9_12,13_16}.hip (split by graph size so they compile in parallel), for 16-bit
// features film_mean_bwd_half_{1_8,9_12,13_16,mfma}.hip, and film_mean_bwd_rows_mfma.hip (MRP_GRAPH_SIMPLE);
// kernels and design notes: film_mean_kernels.hpp.
#include "film_mean_kernels.hpp"

using namespace mrp_host;

namespace {

// Geometry of film_bwd_regular (N > 8, uniform in-degree k <= 8) for slice width vec.
// 1-element slices ask for twice the knob's lanes, at most 64: the kernel reduces a plane's Gram over one
// wave (with_lanes) and lane 0 alone stores it, so a plane on two waves would drop the second's partial.
Geometry regular_geometry(int C, int P, int vec) {
  const Tuning& tu = tuning();
  const int lanes = vec == 2 ? tu.bwd_regular_lanes : std::min(2 * tu.bwd_regular_lanes, 64);
  return make_geometry(C, P, vec, lanes, lanes, mrp::kMaxChanPerBlock);
}

hipError_t dispatch_bwd(int dtype, int nt, bool complete, const AggArgs& a, const Geometry& g, hipStream_t st) {
  // the CSR-row form of film_bwd_mfma (MRP_GRAPH_SIMPLE): film_mean_bwd_rows_mfma.hip, every dtype
  if (g.kernel == MRP_AGG_KERNEL_FILM_BWD_MFMA && g.kmax == 16) return dispatch_bwd_rows_mfma(dtype, a, g, st);
  if (dtype != MRP_DTYPE_F32) {  // 16-bit features: film_mean_bwd_half_*.hip
    if (nt >= 1 && nt <= 8) return dispatch_bwd_half_1_8(dtype, nt, complete, a, g, st);
    if (nt >= 9 && nt <= 12) return dispatch_bwd_half_9_12(dtype, nt, complete, a, g, st);
    if (nt >= 13 && nt <= 16) return dispatch_bwd_half_13_16(dtype, nt, complete, a, g, st);
    return hipErrorInvalidValue;
  }
  if (nt >= 1 && nt <= 8) return dispatch_bwd_1_8(nt, complete, a, g, st);
  if (nt >= 9 && nt <= 12) return dispatch_bwd_9_12(nt, complete, a, g, st);
  if (nt >= 13 && nt <= 16) return dispatch_bwd_13_16(nt, complete, a, g, st);
  return hipErrorInvalidValue;
}

int film_bwd_impl(int32_t dtype, const void* grad_out, int64_t g_node_stride, const void* x, int64_t x_node_stride,
                  const float* gb, const int32_t* indptr, const int32_t* src, const int32_t* eid,
                  const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                  int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t mode_flags, void* grad_x,
                  int64_t gx_node_stride, const void* grad_x_base, int64_t base_node_stride, float* grad_gb,
                  const mrp_agg_epilogue* ep, void* stream);

// The backward's launch plan: validation, kernel choice, slice width, geometry, the PRE2 condition, the
// matrix-core take-over and dynamic LDS.  No GPU call; the pointers are looked at for alignment and NULL
// only.  Returns the code the entry points return before launching; g.kernel == MRP_AGG_KERNEL_NONE with
// hipSuccess: nothing to launch.  zero_dgb: grad_gb is to be cleared first (gamma/beta without influence
// on the output).  Behind both film_bwd_impl and mrp_film_mean_bwd_plan.
int film_bwd_plan(int32_t dtype, const void* grad_out, int64_t g_node_stride, const void* x, int64_t x_node_stride,
                  const float* gb, const int32_t* indptr, const int32_t* src, const int32_t* eid,
                  const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                  int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t mode_flags, void* grad_x,
                  int64_t gx_node_stride, const void* grad_x_base, int64_t base_node_stride, float* grad_gb,
                  const mrp_agg_epilogue* ep, AggArgs& a, Geometry& g, bool& zero_dgb);

}  // namespace

extern "C" {

int mrp_film_mean_bwd_plan(int32_t dtype, const void* grad_out, int64_t g_node_stride, const void* x,
                           int64_t x_node_stride, const float* gb, const int32_t* indptr, const int32_t* src,
                           const int32_t* eid, const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                           int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P,
                           int32_t mode_flags, void* grad_x, int64_t gx_node_stride, const void* grad_x_base,
                           int64_t base_node_stride, float* grad_gb, const mrp_agg_epilogue* ep,
                           mrp_agg_plan* plan) {
  if (plan == nullptr) return hipErrorInvalidValue;
  if (dtype != MRP_DTYPE_F32 && dtype != MRP_DTYPE_BF16 && dtype != MRP_DTYPE_F16) return hipErrorInvalidValue;
  AggArgs a = {};
  Geometry g;
  bool zero_dgb = false;
  const int rc = film_bwd_plan(dtype, grad_out, g_node_stride, x, x_node_stride, gb, indptr, src, eid, graph_off,
                               num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P, mode_flags, grad_x,
                               gx_node_stride, grad_x_base, base_node_stride, grad_gb, ep, a, g, zero_dgb);
  if (rc == hipSuccess) fill_plan(g, a.want_dx, a.want_dgb, plan);
  return rc;
}

int mrp_film_mean_bwd(const float* grad_out, int64_t g_node_stride, const float* x, int64_t x_node_stride,
                      const float* gb, const int32_t* indptr, const int32_t* src, const int32_t* eid,
                      const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                      int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t mode_flags, float* grad_x,
                      int64_t gx_node_stride, const float* grad_x_base, int64_t base_node_stride, float* grad_gb,
                      void* stream) {
  return mrp_film_mean_bwd_ex(grad_out, g_node_stride, x, x_node_stride, gb, indptr, src, eid, graph_off, num_graphs,
                              max_nodes, graph_kind, num_nodes, num_edges, C, P, mode_flags, grad_x, gx_node_stride,
                              grad_x_base, base_node_stride, grad_gb, nullptr, nullptr, 0, stream);
}

// No backward kernel of this library version needs scratch (the plane-split k-NN backward that used
// it measured slower and is gone, round 3); kept so callers written against the workspace
// contract keep working.
int64_t mrp_film_mean_bwd_workspace(int32_t, int32_t, int32_t, int32_t, int32_t) { return 0; }

int mrp_film_mean_bwd_ex(const float* grad_out, int64_t g_node_stride, const float* x, int64_t x_node_stride,
                         const float* gb, const int32_t* indptr, const int32_t* src, const int32_t* eid,
                         const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                         int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t mode_flags,
                         float* grad_x, int64_t gx_node_stride, const float* grad_x_base, int64_t base_node_stride,
                         float* grad_gb, const mrp_agg_epilogue* ep, void* workspace, int64_t workspace_bytes,
                         void* stream) {
  (void)workspace;
  (void)workspace_bytes;
  return film_bwd_impl(MRP_DTYPE_F32, grad_out, g_node_stride, x, x_node_stride, gb, indptr, src, eid, graph_off,
                       num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P, mode_flags, grad_x,
                       gx_node_stride, grad_x_base, base_node_stride, grad_gb, ep, stream);
}

int mrp_film_mean_bwd_t(int32_t dtype, const void* grad_out, int64_t g_node_stride, const void* x,
                        int64_t x_node_stride, const float* gb, const int32_t* indptr, const int32_t* src,
                        const int32_t* eid, const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                        int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P,
                        int32_t mode_flags, void* grad_x, int64_t gx_node_stride, const void* grad_x_base,
                        int64_t base_node_stride, float* grad_gb, const mrp_agg_epilogue* ep, void* stream) {
  if (dtype != MRP_DTYPE_F32 && dtype != MRP_DTYPE_BF16 && dtype != MRP_DTYPE_F16) return hipErrorInvalidValue;
  return film_bwd_impl(dtype, grad_out, g_node_stride, x, x_node_stride, gb, indptr, src, eid, graph_off, num_graphs,
                       max_nodes, graph_kind, num_nodes, num_edges, C, P, mode_flags, grad_x, gx_node_stride,
                       grad_x_base, base_node_stride, grad_gb, ep, stream);
}

}  // extern "C"

namespace {

// The backward behind mrp_film_mean_bwd{,_ex,_t}.  grad_out, x, grad_x and grad_x_base hold elements of
// `dtype` (strides in elements); gb and grad_gb are fp32.
int film_bwd_impl(int32_t dtype, const void* grad_out, int64_t g_node_stride, const void* x, int64_t x_node_stride,
                  const float* gb, const int32_t* indptr, const int32_t* src, const int32_t* eid,
                  const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                  int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t mode_flags, void* grad_x,
                  int64_t gx_node_stride, const void* grad_x_base, int64_t base_node_stride, float* grad_gb,
                  const mrp_agg_epilogue* ep, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  AggArgs a = {};
  Geometry g;
  bool zero_dgb = false;
  const int rc = film_bwd_plan(dtype, grad_out, g_node_stride, x, x_node_stride, gb, indptr, src, eid, graph_off,
                               num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P, mode_flags, grad_x,
                               gx_node_stride, grad_x_base, base_node_stride, grad_gb, ep, a, g, zero_dgb);
  if (zero_dgb) {
    // gamma/beta do not influence the output: their gradient is zero.
    hipError_t e = hipMemsetAsync(grad_gb, 0, (size_t)num_edges * C * 2 * sizeof(float), st);
    if (e != hipSuccess) return e;
  }
  if (rc != hipSuccess || g.kernel == MRP_AGG_KERNEL_NONE) return rc;
  return dispatch_bwd(dtype, max_nodes, graph_kind == MRP_GRAPH_COMPLETE, a, g, st);
}

int film_bwd_plan(int32_t dtype, const void* grad_out, int64_t g_node_stride, const void* x, int64_t x_node_stride,
                  const float* gb, const int32_t* indptr, const int32_t* src, const int32_t* eid,
                  const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                  int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t mode_flags, void* grad_x,
                  int64_t gx_node_stride, const void* grad_x_base, int64_t base_node_stride, float* grad_gb,
                  const mrp_agg_epilogue* ep, AggArgs& a, Geometry& g, bool& zero_dgb) {
  g = Geometry();  // kernel = MRP_AGG_KERNEL_NONE until a launch is planned
  zero_dgb = false;
  const bool half = dtype != MRP_DTYPE_F32;  // 16-bit features
  const float agg_scale = ep != nullptr ? ep->agg_scale : 1.f;
  const float self_scale = ep != nullptr ? ep->self_scale : 0.f;
  const int32_t logits = (mode_flags & MRP_AGG_GB_LOGITS) ? 1 : 0;
  const int32_t mode = mode_flags & ~MRP_AGG_GB_LOGITS;
  if (!common_args_ok(indptr, src, eid, graph_off, num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P,
                      mode))
    return hipErrorInvalidValue;
  const bool copy = mode == MRP_AGG_COPY_MEAN;
  // MRP_GRAPH_SIMPLE: edge ids need not cover grad_gb's rows, and the rows no CSR entry names are zero
  const bool simple = graph_kind == MRP_GRAPH_SIMPLE;
  zero_dgb = grad_gb != nullptr && num_edges > 0 && C > 0 &&
             (copy || num_nodes == 0 || P == 0 || agg_scale == 0.f || simple);
  const bool want_dgb = grad_gb != nullptr && !copy && num_edges > 0 && agg_scale != 0.f;
  const bool want_dx = grad_x != nullptr;
  if (!want_dgb && !want_dx) return hipSuccess;
  if (num_graphs == 0 || num_nodes == 0 || max_nodes == 0 || C == 0 || P == 0) return hipSuccess;
  const int64_t plane = (int64_t)C * P;
  if (grad_out == nullptr || g_node_stride < plane) return hipErrorInvalidValue;
  if (want_dx && gx_node_stride < plane) return hipErrorInvalidValue;
  if (want_dx && grad_x_base != nullptr && base_node_stride < plane) return hipErrorInvalidValue;
  if (want_dgb && (x == nullptr || x_node_stride < plane)) return hipErrorInvalidValue;
  if (!copy && num_edges > 0 && gb == nullptr) return hipErrorInvalidValue;
  // 4-element slices: 16 bytes of fp32, 8 bytes of a 16-bit type
  auto slice_aligned = [half](const void* p) { return half ? aligned8(p) : aligned16(p); };
  bool vec4 = (P % 4 == 0) && (g_node_stride % 4 == 0) && slice_aligned(grad_out);
  if (want_dx) vec4 = vec4 && (gx_node_stride % 4 == 0) && slice_aligned(grad_x);
  if (want_dx && grad_x_base) vec4 = vec4 && (base_node_stride % 4 == 0) && slice_aligned(grad_x_base);
  if (want_dgb) vec4 = vec4 && (x_node_stride % 4 == 0) && slice_aligned(x);
  // 16-byte slices: with the DPP lane reduction they beat 8-byte slices (310 vs 322 us at B=32,
  // N=8, C=512, 32x32) despite 2 waves/SIMD instead of 3.  VEC=2 stays compiled for experiments.
  int vec = vec4 ? 4 : 1;
  const bool complete = graph_kind == MRP_GRAPH_COMPLETE;
  const bool sig_lds = complete && logits;  // the COMPLETE epilogue's per-slot sigmoid values in LDS
  const int kdeg = MRP_GRAPH_IS_REGULAR(graph_kind) ? MRP_GRAPH_REGULAR_K(graph_kind) : 0;
  int kernel;
  if (!half && max_nodes > 8 && kdeg >= 1 && kdeg <= 8) {
    // film_bwd_regular (fp32 features only; 16-bit ones that film_bwd_mfma below does not take run
    // film_bwd_dx + the Gram pass): 8-byte slices on 16 lanes per plane (367 us against 569 us on 64 lanes at
    // k-NN(4) N=16 C=1024 16x16): its prologue and lane reduction are amortised over more slices
    const Tuning& tu = tuning();
    vec = (vec4 && kdeg <= 4 && tu.bwd_regular_vec == 2) ? 2 : 1;
    g = regular_geometry(C, P, vec);
    kernel = MRP_AGG_KERNEL_FILM_BWD_REGULAR;
    g.kmax = kdeg <= 4 ? 4 : 8;
    g.lds = lds_regular(max_nodes, g.kmax, g.cpb);  // <= 27 KiB at 16 channels of 16 nodes
  } else if (max_nodes <= 8) {
    // film_bwd_fused: up to 128 lanes (two waves) per plane, two slices per lane: 283 vs 306 us at
    // 64 lanes at the bench size (tools/fwd_lab.hip backward sweep; 256 lanes: 297 us)
    const Tuning& tu = tuning();
    g = make_geometry(C, P, vec, tu.bwd_fused_lo, tu.bwd_fused_hi, tu.bwd_fused_cap);
    kernel = MRP_AGG_KERNEL_FILM_BWD_FUSED;
    // bwd_fused_cap = 64 on planes of 4 slices with the sigmoid values: 69 KiB at 64 channels
    while (g.cpb > 1 && lds_bwd(max_nodes, g.cpb, sig_lds, g.lpc) > kMaxDynamicLds) set_cpb(g, C, g.cpb / 2);
    g.lds = lds_bwd(max_nodes, g.cpb, sig_lds, g.lpc);
    // exactly two slices per lane: both prefetched (film_bwd_fused PRE2, fp32 16-byte slices only;
    // bwd_pre2 = 2: not with a grad_x base, whose instantiation then prefetches the base rows instead)
    const bool dxb = want_dx && grad_x_base != nullptr;
    g.pre2 = (!half && g.vec == 4 && P / g.vec == 2 * g.lpc && (tu.bwd_pre2 == 1 || (tu.bwd_pre2 == 2 && !dxb)))
                 ? 1
                 : 0;
  } else {
    g = make_geometry(C, P, vec, 64, 64, mrp::kMaxChanPerBlock);  // film_bwd_dx + Gram pass
    kernel = MRP_AGG_KERNEL_FILM_BWD_DX_GRAM;
    // the Gram pass of complete 16-node graphs with the sigmoid values: 66 KiB at 16 channels
    while (g.cpb > 1 && want_dgb && lds_bwd(max_nodes, g.cpb, sig_lds) > kMaxDynamicLds) set_cpb(g, C, g.cpb / 2);
    g.lds = lds_bwd(max_nodes, g.cpb, sig_lds);
    g.lds_dx = lds_dx(max_nodes, g.cpb);
  }
  // film_bwd_mfma: regular and simple graphs of 9..16 nodes and complete graphs, whole pixel groups of 64, 4-element
  // slices (vec4: 16-byte aligned fp32, 8-byte aligned 16-bit features; bwd_half_mfma = 0 keeps 16-bit
  // features on film_bwd_dx + the Gram pass)
  const bool mfma_kind = ((max_nodes > 8 && kdeg >= 1 && kdeg <= 8 && tuning().bwd_regular_mfma) ||
                          (simple && max_nodes > 8 && tuning().bwd_regular_mfma) ||  // the CSR-row form
                          (complete && max_nodes > 8 && tuning().bwd_complete_mfma)) &&
                         (!half || tuning().bwd_half_mfma);
  if (mfma_kind && vec4 && P % 64 == 0) {
    // per-lane row byte offsets are 32-bit: 15 node strides + two planes (a block's channel pair)
    const int64_t lim = (int64_t)1 << 32;
    const int64_t esz = half ? 2 : 4;
    const int64_t span = (int64_t)plane * esz + (int64_t)P * esz;
    bool fits = (int64_t)15 * g_node_stride * esz + span < lim;
    if (want_dx) fits = fits && (int64_t)15 * gx_node_stride * esz + span < lim;
    if (want_dx && grad_x_base) fits = fits && (int64_t)15 * base_node_stride * esz + span < lim;
    if (want_dgb) fits = fits && (int64_t)15 * x_node_stride * esz + span < lim;
    if (fits) {
      const int cpw = tuning().bwd_mfma_cpw >= 2 ? 2 : 1;  // instantiated: 1, 2
      g.mfma_npb = 16;
      g.vec = 4;
      g.lpc = 64;
      g.cpb = 4 * cpw * (16 / g.mfma_npb);  // 4 waves x blocks per wave x channels per block
      g.threads = 256;
      g.ncb = (C + g.cpb - 1) / g.cpb;
      kernel = MRP_AGG_KERNEL_FILM_BWD_MFMA;
      g.kmax = complete ? 1 : simple ? 16 : (kdeg <= 4 ? 4 : 8);  // film_bwd_mfma's KMAX (16: the CSR-row form)
      g.lds = lds_mfma(g.cpb, g.mfma_npb, g.kmax);
      g.lds_dx = 0;
      g.pre2 = 0;
    }
  }
  g.grid = (int64_t)num_graphs * g.ncb;
  if (g.grid > 0x7fffffff) return hipErrorInvalidValue;
  g.kernel = kernel;
  a = {};
  a.x = x;
  a.xs = x_node_stride;
  a.g = grad_out;
  a.gs = g_node_stride;
  a.gb = gb;
  a.indptr = indptr;
  a.src = src;
  a.eid = eid;
  a.goff = graph_off;
  a.out = grad_x;
  a.os = gx_node_stride;
  a.dgb = grad_gb;
  a.C = C;
  a.P = P;
  a.PV = P / g.vec;
  a.mode = mode;
  a.lpc = g.lpc;
  a.cpb = g.cpb;
  a.ncb = g.ncb;
  a.want_dx = want_dx ? 1 : 0;
  a.want_dgb = want_dgb ? 1 : 0;
  a.logits = logits;
  a.dxb = want_dx ? grad_x_base : nullptr;
  a.dxbs = base_node_stride;
  a.kdeg = kdeg;
  a.agg_scale = agg_scale;
  a.self_scale = self_scale;
  a.epi = (agg_scale != 1.f || self_scale != 0.f) ? 1 : 0;
  a.psplit = 1;
  a.nmax = max_nodes;
  return hipSuccess;
}

}  // namespace

