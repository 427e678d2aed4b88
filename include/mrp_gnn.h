/*
 * mrp_gnn.h — C ABI of the MI355X (gfx950) FiLM-mean message-passing library.
 *
 * This is the drop-in boundary for the GCN aggregation hot path of
 * xjh19971/multi-robot-perception-gnn-1.  The reference executes it as
 *
 *     g.edata['pose_gamma'], g.edata['pose_beta'] = edge_encoder(g.edata['pose'])
 *     g.update_all(edge_udf, node_udf)                 dgl/model/models.py:222-223
 *
 * with edge_udf  m_e   = gamma_e * x_src(e) + beta_e   dgl/model/models.py:210-211
 * and  node_udf  out_v = mean over v's mailbox          dgl/model/models.py:207-208
 * executed by DGL's update_all (gather -> message -> degree bucket -> reduce).
 *
 * Each entry point below replaces the DGL `update_all(edge_udf, node_udf)` call
 * (forward) or its autograd backward; the edge encoder stays a torch Linear stack
 * whose sigmoid output (E, 2C) is consumed *in place* as the interleaved (E, C, 2)
 * gamma/beta tensor that `edge.view(-1, C, 2)` exposes (dgl/model/models.py:154-155).
 *
 * Conventions
 *  - All pointers are device pointers owned by the caller; the library never
 *    allocates, frees or synchronises.  Work is enqueued on `stream`
 *    (a hipStream_t; NULL = the legacy default stream).
 *  - Node features are fp32, node-major: node v's C x P block (P = H*W) starts at
 *    x + v * x_node_stride, channel c's plane at + c * P, contiguous over P.
 *    x_node_stride >= C * P.  (A stride of 2*C*P writes straight into one half of
 *    the torch.cat((h, g_h), 1) buffer, dgl/model/models.py:182.)
 *  - The batched graph is a disjoint union of per-frame graphs (dgl.batch,
 *    dgl/training.py:57-58): graph b owns nodes [graph_off[b], graph_off[b+1]),
 *    at most MRP_MAX_NODES nodes, and every edge stays inside one graph.
 *    Edges are given as CSR by destination: the in-edges of node v occupy
 *    positions [indptr[v], indptr[v+1]) of `src` (global source node id) and
 *    `eid` (row of the (E, C, 2) gamma/beta tensor), in increasing edge-id order
 *    (DGL mailbox order).
 *  - Return value: 0 on success, otherwise a hipError_t value
 *    (hipErrorInvalidValue = 1 for bad shapes/arguments).  No exceptions cross
 *    the ABI.  Stateless and re-entrant.
 *  - Special values (tests/test_gpu_special_values.py).  A non-finite input stays visible — whatever the
 *    reference operation makes non-finite is non-finite here — and stays confined:
 *      aggregation forward: exactly the reference's set.  A non-neighbour, an edgeless node, a clamped
 *        load of a ragged batch are skipped, never multiplied by zero; xcopy carries x's bits, a NaN's
 *        payload included;
 *      aggregation backward: see mrp_film_mean_bwd (the graph, channel and pixel of the poisoned element);
 *      compress (all four families, every `parts`): a dense product — x or agg at (n, c, p) makes
 *        y[n, :, p] non-finite, gy at (n, o, p) makes gx[n, :, p] and gagg[n, :, p] non-finite, and in the
 *        weight gradient column c of gw (x, agg) or row o of gw and gbias[o] (gy); nothing else changes;
 *      edge encoder: pose[e, j] makes every logit of row e (and h[e, :] / hT[:, e] where the reference's
 *        is) non-finite — both ReLUs keep a NaN of either sign, as torch.relu does; no other row changes.
 *    An infinity may come back as NaN from the split-bf16 kernels.  The mean's division is the IEEE
 *    quotient for every sum: +0, subnormals, +-inf and NaN included (the fast division is used only for
 *    groups of sums with 2^-124 <= |s| < inf).  The fused sigmoid (MRP_AGG_GB_LOGITS) saturates: within
 *    (2.5 2^-23 + 2^-24 |z|) relative + 2^-126 absolute of the exact value for every z, exactly 1 from
 *    z = 20 + 24 ln 2 on, exactly 0 at z = -inf (the absolute term is one flushed subnormal: 1 / e^-z below
 *    about z = -87.3); its backward is exactly 0 at z = +-inf and |z| >= 104; a NaN logit stays in its own
 *    (edge, channel).  Every store to bf16 / fp16 is one round to nearest even of the fp32 result:
 *    overflow gives +-inf, results in T's subnormal range are kept, NaN stays NaN, -0 stays -0; bf16 / fp16
 *    subnormal operands are kept by the matrix cores.  The domain of the split-bf16 kernels is stated at
 *    mrp_compress_fwd_split.  FP8 messages (mrp_film_mean_fwd_q): an E4M3 NaN code (0x7f / 0xff) and an
 *    E5M2 inf / NaN code decode to fp32 NaN / inf and from there propagate as above — to the destinations
 *    that consume that source, at that channel and pixel, and to no other element; FP8 subnormal codes are
 *    decoded exactly (no flush), and the product with the scale is one fp32 rounding.  The same holds for
 *    mrp_film_max_fwd_q, mrp_film_attn_fwd_q and mrp_film_wattn_fwd_q: a NaN / inf code is a NaN / inf message
 *    element and reaches what it reaches in the fp32 operator on x^ (attention: every channel of that head
 *    at that pixel of the consuming destinations, no other head; a sender silent at a pixel is never read
 *    there); a non-finite query element acts as a non-finite x[v] does in mrp_film_attn_fwd, on v alone.
 */
#ifndef MRP_GNN_H
#define MRP_GNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRP_MAX_NODES 16

/* Graph kinds.  MRP_GRAPH_COMPLETE is the reference's only topology (dgl/dataloader.py:88-95):
 * every graph has exactly max_nodes nodes, edges are all ordered pairs u != v, numbered graph by
 * graph in i-major order (edge u->v of graph b is b*n*(n-1) + u*(n-1) + (v < u ? v : v-1)), and
 * node ids are graph by graph.  indptr/src/eid/graph_off are then not read (may be NULL).
 * MRP_GRAPH_CSR is any batch of disjoint graphs described by the CSR arrays.
 *
 * Preconditions the kernels rely on and do not check on the device (the library never reads
 * device memory on the host; RobotGraph.csr() establishes them, and breaking them gives wrong or
 * partially unwritten outputs rather than an error):
 *   - every graph b has graph_off[b+1] - graph_off[b] <= max_nodes nodes;
 *   - every edge's source lies in its destination's graph;
 *   - MRP_GRAPH_REGULAR(k): every node has exactly k in-edges, so node v's CSR row is
 *     [k*v, k*(v+1)) (indptr is then not read by the forward);
 *   - MRP_GRAPH_COMPLETE: the edge numbering below;
 *   - MRP_GRAPH_SIMPLE: no two CSR entries share a (source, destination) pair.
 *
 * MRP_GRAPH_SIMPLE is a batch described by the CSR arrays exactly as MRP_GRAPH_CSR, with that one
 * additional promise (a range-limited or drop-out frame has it by construction;
 * mrp_frame_graph_build_range builds such graphs).  Self-loops, graphs of fewer than max_nodes nodes
 * and nodes of in-degree 0 are allowed.  num_edges is the number of rows of gb / grad_gb and may
 * exceed indptr[num_nodes]: edge ids need not cover every row (src and eid hold at least
 * indptr[num_nodes] entries and must be non-NULL when num_edges > 0).  The backward writes every
 * grad_gb row that no CSR entry names as zeros.  Every entry point handles the kind as it handles
 * MRP_GRAPH_CSR (same kernels, same bits) except the NCHW backward of graphs with max_nodes 9..16,
 * which runs film_bwd_mfma in its CSR-row form where that kernel's conditions hold (P % 64 == 0,
 * aligned 4-element slices, 32-bit row offsets; knobs "bwd_regular_mfma", "bwd_half_mfma"): the weight
 * tile of a destination is then a plain scatter of its row, which is what the promise is for. */
enum mrp_graph_kind {
    MRP_GRAPH_CSR = 0,
    MRP_GRAPH_COMPLETE = 1,
    MRP_GRAPH_SIMPLE = 3 /* 2 is the low byte of MRP_GRAPH_REGULAR(k) */
};
/* MRP_GRAPH_REGULAR(k): a CSR graph in which every node has exactly k in-edges (k-NN graphs).  The
 * CSR arrays are read as for MRP_GRAPH_CSR; the backward for graphs of more than 8 nodes then keeps
 * one Gram accumulator per edge instead of per node pair (k <= 8).  num_edges must be k*num_nodes.
 * Node v's CSR row is then [k*v, k*(v+1)) by construction (CSR by destination, uniform degree), so
 * the forward does not read indptr. */
#define MRP_GRAPH_REGULAR(k) (((k) << 8) | 2)
#define MRP_GRAPH_IS_REGULAR(kind) (((kind) & 0xff) == 2)
#define MRP_GRAPH_REGULAR_K(kind) ((kind) >> 8)

/* Aggregation modes (the reference's UDF variants). */
enum mrp_agg_mode {
    MRP_AGG_FILM_MEAN = 0, /* mean_e(gamma_e*x_u + beta_e): models.py:207-211          */
    MRP_AGG_FILM_SUM = 1,  /* sum_e(gamma_e*x_u + beta_e)                              */
    MRP_AGG_COPY_MEAN = 2  /* mean_e(x_u), fn.copy_u('image','m'): models.py:225,
                              dgl_models.py:126 ("multi_view_dgl_mean_wofilm")         */
};

/* Flag OR-ed into `mode`: gb holds the edge encoder's pre-sigmoid logits z (the output of its
 * second Linear); the kernels apply gamma/beta = sigmoid(z) while building their tiles (forward)
 * and return d z = d gamma/beta * s (1 - s) (backward).  Fuses the encoder's Sigmoid
 * (dgl/model/models.py:150) into the aggregation. */
#define MRP_AGG_GB_LOGITS 0x100

/*
 * Forward: out[v] = reduce over in-edges e=(u->v) of (gamma_e (.) x[u] + beta_e).
 * Replaces g.update_all(edge_udf, node_udf), dgl/model/models.py:223.
 * Nodes with zero in-degree get zeros (DGL >= 0.5 zero-fill).
 *
 *   x          (num_nodes, C, P) fp32, node stride x_node_stride (elements)
 *   gb         (num_edges, C, 2) fp32 interleaved gamma/beta; may be NULL for COPY_MEAN
 *   indptr     (num_nodes + 1) int32, CSR by destination
 *   src, eid   (num_edges) int32
 *   graph_off  (num_graphs + 1) int32 node offsets of the batched graphs
 *   max_nodes  max_b (graph_off[b+1] - graph_off[b]), 0..MRP_MAX_NODES (host-known)
 *   graph_kind MRP_GRAPH_CSR, MRP_GRAPH_COMPLETE, MRP_GRAPH_SIMPLE or MRP_GRAPH_REGULAR(k) (see enum
 *              mrp_graph_kind)
 *   out        (num_nodes, C, P) fp32, node stride out_node_stride (elements)
 */
int mrp_film_mean_fwd(const float* x, int64_t x_node_stride,
                      const float* gb,
                      const int32_t* indptr, const int32_t* src, const int32_t* eid,
                      const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                      int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                      int32_t C, int32_t P, int32_t mode,
                      float* out, int64_t out_node_stride,
                      void* stream);

/*
 * torch.cat((x, update_all(...)), 1) in one pass (dgl/model/models.py:181-182, 186-188): as
 * mrp_film_mean_fwd, but `cat` is the (num_nodes, 2C, P) concatenation buffer (node stride
 * cat_node_stride >= 2*C*P): x is written to channels [0, C) and the aggregate to [C, 2C).  The
 * kernel stores the slices of x it already holds in registers, so x is read once instead of twice.
 */
int mrp_film_mean_cat_fwd(const float* x, int64_t x_node_stride,
                          const float* gb,
                          const int32_t* indptr, const int32_t* src, const int32_t* eid,
                          const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                          int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                          int32_t C, int32_t P, int32_t mode,
                          float* cat, int64_t cat_node_stride,
                          void* stream);

/*
 * Backward of mrp_film_mean_fwd (the autograd of models.py:207-211 through DGL's
 * gather/mailbox, which the reference gets from torch autograd).  With s_v the
 * reduce scale (1/deg v for the mean modes, 1 for SUM) and G = grad_out:
 *
 *   grad_x[u]      = sum_{e=(u->v)} s_v * gamma_e (.) G[v]          (gamma = 1 for COPY)
 *   grad_gb[e,c,0] = s_v * sum_p x[u,c,p] * G[v,c,p]                (d gamma_e)
 *   grad_gb[e,c,1] = s_v * sum_p G[v,c,p]                           (d beta_e)
 *
 * grad_x (node stride gx_node_stride) and grad_gb ((num_edges, C, 2), interleaved
 * like gb) may each be NULL to skip that output.  For COPY_MEAN grad_gb is zero-filled.
 * grad_x_base (node stride base_node_stride, may be NULL) is added to grad_x: the backward of
 * torch.cat((x, out), 1) (dgl/model/models.py:182) passes the first half of the concatenation's
 * gradient here and the second half as grad_out, so x's total gradient is one pass.
 * Deterministic: no atomics; each output element is written by exactly one lane.
 * Non-finite values: the transposed tiles are dense within a graph (a matrix-core kernel multiplies every
 * node pair of it), so a non-finite grad_out[v, c, p] may make grad_x non-finite at (any node of v's graph,
 * c, p) and grad_gb at (any edge of v's graph, c) — never outside them, and always wherever the formulas
 * above do; a non-finite x[u, c, p] leaves grad_x's bits unchanged and is confined in grad_gb to (the edges
 * of u's graph, c).  Some kernels are stricter ("Special values"); only this is promised.
 */
int mrp_film_mean_bwd(const float* grad_out, int64_t g_node_stride,
                      const float* x, int64_t x_node_stride,
                      const float* gb,
                      const int32_t* indptr, const int32_t* src, const int32_t* eid,
                      const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                      int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                      int32_t C, int32_t P, int32_t mode,
                      float* grad_x, int64_t gx_node_stride,
                      const float* grad_x_base, int64_t base_node_stride,
                      float* grad_gb,
                      void* stream);

/*
 * Epilogue of the aggregation, for the layer compositions around update_all.  With a = the
 * aggregate of destination v (as mrp_film_mean_fwd computes it), the forward writes
 *
 *   out[v] = agg_scale * a + self_scale * x[v] + x0_scale * x0[v]
 *
 * evaluated left to right in fp32 (each product rounded, then each sum; a scale of 1 is exact), and
 * if xcopy != NULL also stores x[v] at xcopy + v * xcopy_node_stride.  Uses:
 *   - plain aggregation:  {1, 0, NULL, 0, 0, NULL, 0} (what a NULL epilogue pointer means);
 *   - residual h = g_h + h (dgl/model/dgl_models.py:36-37): agg_scale 1, self_scale 1 — x[v] is
 *     already in registers, so this costs no traffic;
 *   - initial-feature mix (GCN2-style, (1 - alpha) * a + alpha * x0; not in the reference, parity
 *     unpinned): agg_scale 1 - alpha, x0 = the first layer's input, x0_scale alpha;
 *   - torch.cat((x, a), 1) (dgl/model/models.py:182): xcopy = the first half of the concatenation
 *     buffer (mrp_film_mean_cat_fwd is this with out = its second half).
 * The backward (mrp_film_mean_bwd_ex) reads agg_scale and self_scale: grad_out reaches the
 * aggregation scaled by agg_scale, and self_scale * grad_out[u] is added to grad_x[u].  The
 * gradient of x0 is x0_scale * grad_out (an elementwise product the caller forms); x0 and xcopy
 * are not read by the backward.
 * The typed entry points (mrp_film_mean_fwd_t) read x0 and write xcopy as elements of their `dtype`
 * (the pointers are declared float* here for the fp32 entry points; cast for the 16-bit types), with the
 * two node strides in elements of that type.
 */
typedef struct mrp_agg_epilogue {
    float agg_scale;
    float self_scale;
    const float* x0;
    int64_t x0_node_stride;
    float x0_scale;
    float* xcopy;
    int64_t xcopy_node_stride;
} mrp_agg_epilogue;

/* mrp_film_mean_fwd with an epilogue (NULL: plain).  x0 and xcopy rows use the node ids of x. */
int mrp_film_mean_fwd_ex(const float* x, int64_t x_node_stride,
                         const float* gb,
                         const int32_t* indptr, const int32_t* src, const int32_t* eid,
                         const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                         int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                         int32_t C, int32_t P, int32_t mode,
                         float* out, int64_t out_node_stride,
                         const mrp_agg_epilogue* epilogue,
                         void* stream);

/* mrp_film_mean_bwd for a forward run with `epilogue` (NULL: plain; see mrp_agg_epilogue).
 * workspace: reserved (NULL/0 allowed; mrp_film_mean_bwd_workspace returns 0): ABI 11's plane-split
 * k-NN backward that used it measured slower than whole planes and was removed in ABI 12. */
int mrp_film_mean_bwd_ex(const float* grad_out, int64_t g_node_stride,
                         const float* x, int64_t x_node_stride,
                         const float* gb,
                         const int32_t* indptr, const int32_t* src, const int32_t* eid,
                         const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                         int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                         int32_t C, int32_t P, int32_t mode,
                         float* grad_x, int64_t gx_node_stride,
                         const float* grad_x_base, int64_t base_node_stride,
                         float* grad_gb,
                         const mrp_agg_epilogue* epilogue,
                         void* workspace, int64_t workspace_bytes,
                         void* stream);

/*
 * Feature storage types of the typed entry points below.  Feature tensors (x, out, grad_out, grad_x,
 * grad_x_base, the epilogue's x0 and xcopy) hold elements of `dtype`, and every node stride counts
 * elements of `dtype`; gb (or its logits) and grad_gb are always fp32.  For the 16-bit types every
 * loaded element is widened exactly to fp32, the arithmetic is the fp32 kernels' own, operation for
 * operation, and every stored element is rounded once, to nearest even:
 *   mrp_film_mean_fwd_t(T, x) == T(mrp_film_mean_fwd_ex(float(x)))        bit for bit,
 * likewise grad_x for graphs of <= 8 nodes; xcopy receives x's bits unchanged.  Graphs of 9..16 nodes
 * (complete, or regular with in-degree <= 8) whose planes are whole groups of 64 pixels, with 8-byte
 * aligned pointers and node strides that are multiples of 4, run the matrix-core backward on 16-bit
 * features too: grad_x == T(fp32 grad_x) and grad_gb == the fp32 grad_gb, bit for bit.  Other shapes
 * of 9..16 nodes run film_bwd_dx + the film_bwd_fused Gram pass at 16 bits (no per-edge-slot kernel);
 * there grad_x, like grad_gb for <= 8 nodes, is summed in another order than the fp32 path's.
 * Slices are 16 bytes (8 elements; forward, <= 8 nodes), 8 bytes (4 elements) or one element, by the
 * alignment of the pointers, P and the node strides.
 */
enum mrp_dtype { MRP_DTYPE_F32 = 0, MRP_DTYPE_BF16 = 1, MRP_DTYPE_F16 = 2 };

/* mrp_film_mean_fwd_ex over a feature storage type.  MRP_DTYPE_F32 is mrp_film_mean_fwd_ex itself; an
 * unknown dtype returns hipErrorInvalidValue; zero sizes return success without a launch. */
int mrp_film_mean_fwd_t(int32_t dtype,
                        const void* x, int64_t x_node_stride,
                        const float* gb,
                        const int32_t* indptr, const int32_t* src, const int32_t* eid,
                        const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                        int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                        int32_t C, int32_t P, int32_t mode,
                        void* out, int64_t out_node_stride,
                        const mrp_agg_epilogue* epilogue,
                        void* stream);

/* mrp_film_mean_bwd_ex (without its reserved workspace) over a feature storage type: grad_out, x,
 * grad_x and grad_x_base hold `dtype`, grad_gb is fp32. */
int mrp_film_mean_bwd_t(int32_t dtype,
                        const void* grad_out, int64_t g_node_stride,
                        const void* x, int64_t x_node_stride,
                        const float* gb,
                        const int32_t* indptr, const int32_t* src, const int32_t* eid,
                        const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                        int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                        int32_t C, int32_t P, int32_t mode,
                        void* grad_x, int64_t gx_node_stride,
                        const void* grad_x_base, int64_t base_node_stride,
                        float* grad_gb,
                        const mrp_agg_epilogue* epilogue,
                        void* stream);

/* Bytes of workspace mrp_film_mean_bwd_ex can use for these graph/feature sizes (0: none needed;
 * always 0 since ABI 12). */
int64_t mrp_film_mean_bwd_workspace(int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                                    int32_t C, int32_t P);

/*
 * The aggregation on pixel-major ("channels-last") feature maps: what a backbone run with
 * memory_format=torch.channels_last hands over.  Node v's pixel p (P = H*W pixels) is a row of C
 * contiguous elements of `dtype` at
 *
 *     base + v * node_stride + p * pixel_stride          (strides in elements of `dtype`)
 *
 * with pixel_stride >= C (C for a dense channels-last tensor, 2C for either half of a channels-last
 * concatenation buffer) and node_stride >= P * pixel_stride.  Every feature tensor of these entry
 * points (x, out, grad_out, grad_x, grad_x_base, the epilogue's x0 and xcopy) is such a
 * (pointer, node_stride, pixel_stride) triple; each may have its own strides.  gb / grad_gb, the
 * graph arguments, C, P and mode are those of mrp_film_mean_fwd_t / mrp_film_mean_bwd_t.
 *
 * The arithmetic is the node-major entry points', operation for operation, so for every graph, mode,
 * epilogue and dtype
 *     mrp_film_mean_fwd_cl(x_cl) == mrp_film_mean_fwd_t(x_nchw)           as values, bit for bit,
 * and grad_x is the fmaf chain of the node-major backward for graphs of <= 8 nodes (base or 0, then
 * self_scale * G[u], then Wt[u][v] * G[v] for v ascending): bit-equal to it there.  grad_gb is summed
 * over the pixels in a fixed order of its own (deterministic; no atomics; every output element is
 * written by one lane).
 *
 * Return codes: hipErrorInvalidValue for an unknown dtype, a NULL pointer with work to do,
 * pixel_stride < C, node_stride < P * pixel_stride, max_nodes > MRP_MAX_NODES or a workspace smaller
 * than the query; hipErrorNotSupported when P * pixel_stride * sizeof(dtype) of a tensor reaches 2^31
 * (the kernels' per-lane byte offsets are 32 bits) or the launch grid would exceed 2^31 - 1
 * workgroups (the LDS tiles always fit: the channel block shrinks with the slot count); both are
 * decided on the host before anything is enqueued.  Zero sizes succeed without a launch.  No host
 * synchronisation: the entry points can be captured into a graph.
 *
 * Lanes access 16-byte channel vectors when every pointer is 16-byte aligned, C * sizeof(dtype) is a
 * multiple of 16 and every node and pixel stride is a multiple of 16 bytes; otherwise the same kernel
 * template runs with one element per access.
 */
typedef struct mrp_agg_epilogue_cl {
    float agg_scale;
    float self_scale;
    const void* x0;
    int64_t x0_node_stride;
    float x0_scale;
    void* xcopy;
    int64_t xcopy_node_stride;
    int64_t x0_pixel_stride;
    int64_t xcopy_pixel_stride;
} mrp_agg_epilogue_cl; /* mrp_agg_epilogue plus the two pixel strides */

int mrp_film_mean_fwd_cl(int32_t dtype,
                         const void* x, int64_t x_node_stride, int64_t x_pixel_stride,
                         const float* gb,
                         const int32_t* indptr, const int32_t* src, const int32_t* eid,
                         const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                         int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                         int32_t C, int32_t P, int32_t mode,
                         void* out, int64_t out_node_stride, int64_t out_pixel_stride,
                         const mrp_agg_epilogue_cl* epilogue,
                         void* stream);

/* Backward of mrp_film_mean_fwd_cl (see mrp_film_mean_bwd for the formulas; grad_x and grad_gb may
 * each be NULL; COPY_MEAN zero-fills grad_gb; x is read only when grad_gb is wanted).  The Gram of a
 * plane split over several workgroups is summed through `workspace` (>= the query's bytes, 4-byte
 * aligned; NULL / 0 allowed when the query returns 0) in segment order by a second launch. */
int mrp_film_mean_bwd_cl(int32_t dtype,
                         const void* grad_out, int64_t g_node_stride, int64_t g_pixel_stride,
                         const void* x, int64_t x_node_stride, int64_t x_pixel_stride,
                         const float* gb,
                         const int32_t* indptr, const int32_t* src, const int32_t* eid,
                         const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                         int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                         int32_t C, int32_t P, int32_t mode,
                         void* grad_x, int64_t gx_node_stride, int64_t gx_pixel_stride,
                         const void* grad_x_base, int64_t base_node_stride, int64_t base_pixel_stride,
                         float* grad_gb,
                         const mrp_agg_epilogue_cl* epilogue,
                         void* workspace, int64_t workspace_bytes,
                         void* stream);

/* Bytes of workspace mrp_film_mean_bwd_cl needs for these sizes (the same for every dtype); 0 when
 * grad_gb is not wanted (want_grad_gb == 0), for COPY_MEAN, and when no plane is split. */
int64_t mrp_film_mean_bwd_cl_workspace(int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                                       int32_t C, int32_t P, int32_t mode, int32_t want_grad_gb);

/*
 * The max-pooled FiLM aggregation (ABI 22, extended): node_udf = torch.max(mailbox, 1) in place of the
 * reference's torch.mean(mailbox, 1) (dgl/model/models.py:207-208).  An operator of its own: it is not a
 * value of enum mrp_agg_mode, and every mrp_film_mean_* entry point keeps rejecting mode 3.
 *
 * For destination v with CSR row [indptr[v], indptr[v+1]), entries j = 0, 1, ... in row order (edge-id
 * order, DGL's mailbox order), e_j the entry's edge id and u_j its source:
 *
 *   m_j[c,p]       = fl(fl(gamma_{e_j}[c] * x[u_j,c,p]) + beta_{e_j}[c])     no FMA contraction
 *   out[v,c,p]     = max_j m_j[c,p]                                          zeros when the row is empty
 *   w(v,c,p)       = the smallest j attaining that max                       the first maximal entry
 *   grad_x[u,c,p]  = sum over (v, j) with u_j = u of gamma_{e_j}[c] * sel_j(v,c,p)   (+ grad_x_base[u,c,p])
 *   grad_gb[e,c,0] = sum_p x[u,c,p] * sel_{j(e)}(v,c,p)
 *   grad_gb[e,c,1] = sum_p sel_{j(e)}(v,c,p)
 *   sel_j(v,c,p)   = grad_out[v,c,p] if j = w(v,c,p), else an exact 0
 *
 * which is torch.max(mailbox, 1) and its autograd.  Ties and NaN: on a tie the first maximal entry takes
 * the whole gradient (it is not split); a NaN message beats every number and the first NaN wins (torch's
 * update: a message replaces the running maximum unless it is <= it, and nothing replaces a NaN).  The
 * backward stores no argmax; it recomputes w from x, gamma and beta with the forward's own arithmetic.
 * With MRP_AGG_GB_LOGITS gamma/beta = sigmoid(z) formed in the kernel and grad_gb is d z, as for the mean.
 *
 * Every CSR entry is its own message: parallel edges u->v with different (gamma, beta) are two candidates,
 * and self-loops are allowed, under every graph kind (MRP_GRAPH_SIMPLE's promise is not needed here).
 * Every grad_gb row that no CSR entry names is written as zeros, for every graph kind; an entry that
 * never wins gets exact zeros (finite operands).  A node of in-degree 0 gets out = 0 and contributes
 * nothing to any gradient.
 *
 * Precondition, not checked on the device: every in-degree is <= MRP_FILM_MAX_DEGREE (a complete 16-node
 * graph has 15, with self-loops 16); MRP_GRAPH_REGULAR(k) with k above it is declined.
 *
 * 16-bit features: widened exactly on load, the fp32 arithmetic above unchanged, one round-to-nearest-even
 * at each store; gamma, beta and grad_gb stay fp32:  mrp_film_max_fwd(T, x) == T(mrp_film_max_fwd(float(x)))
 * bit for bit, likewise grad_x (on grad_out, x and grad_x_base widened) and grad_gb whenever the fp32 sums
 * are exact.
 *
 * Determinism: no atomics, one writer per output element, every sum in a fixed order.
 *
 * Non-finite values: max selects, it does not mix, so an input NaN or infinity is confined to its own
 * (destination, channel, pixel) of `out` — stricter than the mean backward's per-graph promise above.  In
 * the backward a slot that loses contributes gamma * 0, x * 0 and 0, as autograd does: a non-finite gamma
 * or x of a losing slot still reaches grad_x[u,c,p] / grad_gb[e,c,0] of that slot (0 * inf = NaN), and
 * nothing else.
 *
 * flags: 0 or MRP_AGG_GB_LOGITS.  grad_x or grad_gb may each be NULL to skip that output; with both NULL
 * the backward returns success without a launch.  Validation precedes any launch and matches the typed
 * mean entry points (sizes, strides, max_nodes > MRP_MAX_NODES, unknown kind, dtype or flags, inconsistent
 * COMPLETE counts, NULL pointers where there is work); empty work returns success.  No allocation, no
 * host synchronisation, capturable (a hipMemsetAsync of grad_gb precedes the kernels of non-COMPLETE
 * graphs).  out_node_stride / g_node_stride let the aggregate and its gradient be the second half of a
 * concatenation buffer, as above.
 */
#define MRP_FILM_MAX_DEGREE 16

int mrp_film_max_fwd(int32_t dtype,
                     const void* x, int64_t x_node_stride,
                     const float* gb,
                     const int32_t* indptr, const int32_t* src, const int32_t* eid,
                     const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                     int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                     int32_t C, int32_t P, int32_t flags,
                     void* out, int64_t out_node_stride,
                     void* stream);

int mrp_film_max_bwd(int32_t dtype,
                     const void* grad_out, int64_t g_node_stride,
                     const void* x, int64_t x_node_stride,
                     const float* gb,
                     const int32_t* indptr, const int32_t* src, const int32_t* eid,
                     const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                     int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                     int32_t C, int32_t P, int32_t flags,
                     void* grad_x, int64_t gx_node_stride,
                     const void* grad_x_base, int64_t base_node_stride,
                     float* grad_gb,
                     void* stream);

/*
 * The attention-pooled FiLM aggregation (ABI 22, extended): per-location attention fusion.  At every pixel
 * the receiver's feature vector is the query, each in-neighbour's FiLM message is key and value, and a
 * softmax over the row's entries weights them.  An operator of its own with its own kernels (pixel-tile-major:
 * a workgroup owns a graph and 64 pixels for all channels); the mean and max entry points are unchanged.
 *
 * For destination v with CSR row [indptr[v], indptr[v+1]), entries j = 0 .. d-1 in row order (edge-id
 * order, as mrp_film_max_*), e_j the entry's edge id and u_j its source:
 *
 *   m_j[c,p]   = fl(fl(gamma_{e_j}[c] * x[u_j,c,p]) + beta_{e_j}[c])          as film_max: no FMA contraction
 *   s_j[p]     = scale * sum_c x[v,c,p] * m_j[c,p]                           channels ascending, one chain
 *   a_j[p]     = exp(s_j[p] - max_k s_k[p]) / sum_k exp(s_k[p] - max_k)      softmax over the row's entries
 *   out[v,c,p] = sum_j a_j[p] * m_j[c,p]                                     slot order; zeros when d = 0
 *   attn[e_j,p] = a_j[p]                                                     (E, P) fp32, an output
 *
 * and the full autograd of it, the paths through the scores included.  With g = grad_out[v]:
 *
 *   da_j[p]   = sum_c g[c,p] * m_j[c,p]
 *   ds_j[p]   = a_j[p] * (da_j[p] - sum_k a_k[p] * da_k[p])
 *   dm_j[c,p] = a_j[p] * g[c,p] + scale * ds_j[p] * x[v,c,p]                 value path + key path
 *   grad_x[v,c,p]   += scale * sum_j ds_j[p] * m_j[c,p]                      query path
 *   grad_x[u_j,c,p] += gamma_{e_j}[c] * dm_j[c,p]                            (+ grad_x_base)
 *   grad_gb[e_j,c,0] = sum_p x[u_j,c,p] * dm_j[c,p]
 *   grad_gb[e_j,c,1] = sum_p dm_j[c,p]
 *
 * The backward reads attn as the forward wrote it and recomputes the messages, not the softmax.  With
 * MRP_AGG_GB_LOGITS gamma/beta = sigmoid(z) formed in the kernel and grad_gb is d z, as for the mean and max.
 * The caller chooses scale; 1/sqrt(C) is the usual one, 0 gives uniform weights 1/d.  The exponential is
 * v_exp_f32 on the max-subtracted score (about 1 ulp), the division is IEEE.
 *
 * Every CSR entry is its own message: parallel edges are separate candidates and self-loops are allowed (a
 * self-loop is how a node attends to itself), under every graph kind (MRP_GRAPH_SIMPLE's promise is not
 * needed).  Rows of attn and of grad_gb that no CSR entry names are written as zeros.  A node of in-degree 0
 * gets out = 0 and contributes nothing.
 *
 * Precondition, not checked on the device: every in-degree is <= MRP_FILM_ATTN_DEGREE;
 * MRP_GRAPH_REGULAR(k) with k above it is declined.
 *
 * 16-bit features: widened exactly on load; messages, scores, weights and every sum are fp32; one
 * round-to-nearest-even at each store; gamma, beta, attn and grad_gb stay fp32.  The order of every sum is a
 * function of C, P and the graph only, never of dtype, strides or alignment (every access is one element), so
 * mrp_film_attn_fwd(T, x) == T(mrp_film_attn_fwd(float(x))) bit for bit, attn is equal bit for bit, and
 * likewise grad_x (on grad_out, x and grad_x_base widened) and grad_gb.
 *
 * Determinism: no atomics, one writer per output element, every sum in a fixed order (scores: channels
 * ascending; out: slots ascending; grad_x: per wave of the workgroup the destinations v = w, w+4, ... in
 * slot order, then the four waves in order, then the base; grad_gb: a fixed 64-lane butterfly per pixel tile,
 * then the tiles in order).
 *
 * Non-finite values: a pixel's weights mix all channels of that pixel, so an input NaN or infinity at
 * (node, channel, pixel) may reach every channel of `out` and every weight at that pixel of the destinations
 * that receive the node (and of the node itself), and nothing at any other pixel or in any other graph.  In
 * the backward, grad_x is likewise confined to that pixel of that graph; grad_gb sums over pixels, so the
 * graph's grad_gb rows may all be affected.
 *
 * flags: 0 or MRP_AGG_GB_LOGITS.  grad_x or grad_gb may each be NULL to skip that output; with both NULL the
 * backward returns success without a launch.  Validation precedes any launch and matches mrp_film_max_*; in
 * addition hipErrorInvalidValue is returned for a non-finite scale, a NULL attn where there are edges, and a
 * workspace smaller than needed.  Empty work returns success (a forward without nodes or channels, C == 0,
 * writes a non-NULL attn as zeros: there is nothing to score).  No allocation, no host synchronisation,
 * capturable (hipMemsetAsync of attn / grad_gb precedes the kernels of non-COMPLETE graphs).
 * out_node_stride / g_node_stride let the aggregate and its gradient be the second half of a concatenation
 * buffer.
 *
 * mrp_film_attn_workspace(direction, ...) is the byte count `workspace` must hold (direction 0: forward,
 * always 0; else backward: the per-tile grad_gb partials where a plane spans several 64-pixel tiles, else 0).
 * It makes no GPU call.  The backward needs it only where grad_gb is wanted.
 */
#define MRP_FILM_ATTN_DEGREE 16

int mrp_film_attn_fwd(int32_t dtype,
                      const void* x, int64_t x_node_stride,
                      const float* gb,
                      const int32_t* indptr, const int32_t* src, const int32_t* eid,
                      const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                      int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                      int32_t C, int32_t P, int32_t flags,
                      void* out, int64_t out_node_stride,
                      float scale, float* attn,
                      void* workspace, int64_t workspace_bytes,
                      void* stream);

int mrp_film_attn_bwd(int32_t dtype,
                      const void* grad_out, int64_t g_node_stride,
                      const void* x, int64_t x_node_stride,
                      const float* gb,
                      const int32_t* indptr, const int32_t* src, const int32_t* eid,
                      const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                      int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                      int32_t C, int32_t P, int32_t flags,
                      void* grad_x, int64_t gx_node_stride,
                      const void* grad_x_base, int64_t base_node_stride,
                      float* grad_gb,
                      float scale, const float* attn,
                      void* workspace, int64_t workspace_bytes,
                      void* stream);

int64_t mrp_film_attn_workspace(int32_t direction, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                                int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P);

/*
 * The confidence-weighted FiLM aggregation (ABI 22, extended): every sender u attaches a per-pixel map
 * w[u,p] >= 0 to its feature map (where in the image it transmits), and the receiver averages, pixel by pixel,
 * over what was delivered there.  An operator of its own with its own kernels (the mean's channel-block-major
 * decomposition); every other entry point is unchanged.
 *
 *   x   (num_nodes, C, P) of `dtype`, node stride x_node_stride
 *   gb  (num_edges, C, 2) fp32 interleaved gamma/beta, or their logits with MRP_AGG_GB_LOGITS
 *   w   (num_nodes, P) fp32, node stride w_node_stride >= P, indexed by SOURCE node
 *   the graph arguments exactly as mrp_film_max_fwd (every kind, max_nodes <= MRP_MAX_NODES)
 *
 * Forward.  For destination v with row entries j in row order (edge-id order), e_j the edge and u_j the source:
 *
 *   m_j[c,p]   = fl(fl(gamma_{e_j}[c] * x[u_j,c,p]) + beta_{e_j}[c])        no FMA contraction (as the mean)
 *   acc[v,c,p] = sum_j in row order  fl(acc + fl(w[u_j,p] * m_j[c,p]))
 *   D[v,p]     = sum_j in row order  fl(D + w[u_j,p])
 *   out[v,c,p] = D[v,p] > 0 ? acc / D (IEEE division) : 0                    MRP_WAGG_MEAN
 *   out[v,c,p] = acc[v,c,p]                                                  MRP_WAGG_SUM
 *
 * An empty row, or a pixel at which every sender is silent, gives an exact 0 (the mean's zero fill).
 * Order of the sums: exactly the mean forward's, so that the two operators can be compared bit for bit.  The
 * kernels sum a destination's sources in ascending source order, and parallel edges u -> v are one term,
 * fl(w[u,p] * fl(fl(G x) + B)) with G, B the sums of the edges' gamma, beta in row order and
 * fl(cnt * w[u,p]) in D.  That is the row-order chain above whenever a row is in ascending source order
 * without parallel edges (complete i-major graphs, the k-NN and range builders): the condition under which
 * the mean itself keeps the reference's rounding order.  Consequences, for every graph:
 *   - w == 1 gives mrp_film_mean_fwd_t's bits in modes film_mean / film_sum (fl(1 * m) = m, D the in-degree);
 *   - a 0/1 map constant over each node's plane gives film_mean's bits on the graph without the silent
 *     robots' out-edges.
 *
 * Backward.  Gh[v,c,p] = grad_out / D where D > 0 and 0 elsewhere (MEAN), grad_out (SUM):
 *
 *   grad_x[u,c,p]  = w[u,p] * sum over (v,j) with u_j = u of gamma_{e_j}[c] * Gh[v,c,p]    (+ grad_x_base)
 *   grad_gb[e,c,0] = sum_p w[u,p] * x[u,c,p] * Gh[v,c,p]
 *   grad_gb[e,c,1] = sum_p w[u,p] * Gh[v,c,p]
 *   grad_w[u,p]    = sum over (v,j) with u_j = u, sum_c Gh[v,c,p] * (m_j[c,p] - out[v,c,p])   MEAN
 *   grad_w[u,p]    = sum over (v,j) with u_j = u, sum_c grad_out[v,c,p] * m_j[c,p]            SUM
 *
 * The backward recomputes `out` from x, gb and w with the forward's arithmetic; it takes no saved output.
 * With MRP_AGG_GB_LOGITS grad_gb is d logits.  grad_x, grad_gb and grad_w (fp32, node stride gw_node_stride
 * >= P) may each be NULL to skip that output; all NULL returns success without a launch.  grad_gb rows no CSR
 * entry names are written as zeros.  Sums: grad_x over destinations ascending; grad_gb per lane over its
 * slices, then a fixed butterfly over the plane's lanes; grad_w over channels ascending within a block of 16
 * channels (destinations ascending inside), the blocks' partials then added in block order from `workspace`.
 *
 * 16-bit features: widened exactly on load, the fp32 arithmetic above unchanged, one round-to-nearest-even at
 * each store of T; w, gamma/beta, grad_gb and grad_w stay fp32: fwd(T, x) == T(fwd(float(x))) bit for bit
 * (the per-element sums do not depend on slice width or geometry).
 *
 * Determinism: no atomics, one writer per output element, every sum in an order fixed by the shapes and the
 * graph.  No allocation, no host synchronisation, capturable (a hipMemsetAsync of grad_gb precedes the kernels
 * of non-COMPLETE graphs).  64-bit node offsets.
 *
 * Preconditions: w finite and >= 0.  Negative weights run the arithmetic above without an accuracy promise.  A
 * NaN or infinity in w[u,p] reaches `out` of the destinations that consume u, at pixel p, and nothing else.
 *
 * mrp_film_wmean_workspace is the byte count `workspace` must hold where grad_w is wanted: the per-block
 * partials (ceil(C / 16) x num_nodes x P floats) when C > 16, else 0.  It makes no GPU call.
 * Validation precedes any launch and matches mrp_film_max_*; in addition hipErrorInvalidValue is returned for a
 * NULL w with work to do, w_node_stride < P (gw_node_stride < P), an unknown wagg mode, and a workspace
 * smaller than needed.  Empty work returns success.  out_node_stride / g_node_stride let the aggregate and
 * its gradient be the second half of a concatenation buffer.
 */
enum mrp_wagg_mode { MRP_WAGG_MEAN = 0, MRP_WAGG_SUM = 1 };

int mrp_film_wmean_fwd(int32_t dtype,
                       const void* x, int64_t x_node_stride,
                       const float* gb,
                       const float* w, int64_t w_node_stride,
                       const int32_t* indptr, const int32_t* src, const int32_t* eid,
                       const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                       int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                       int32_t C, int32_t P, int32_t flags, int32_t wagg,
                       void* out, int64_t out_node_stride,
                       void* stream);

int mrp_film_wmean_bwd(int32_t dtype,
                       const void* grad_out, int64_t g_node_stride,
                       const void* x, int64_t x_node_stride,
                       const float* gb,
                       const float* w, int64_t w_node_stride,
                       const int32_t* indptr, const int32_t* src, const int32_t* eid,
                       const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                       int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                       int32_t C, int32_t P, int32_t flags, int32_t wagg,
                       void* grad_x, int64_t gx_node_stride,
                       const void* grad_x_base, int64_t base_node_stride,
                       float* grad_gb,
                       float* grad_w, int64_t gw_node_stride,
                       void* workspace, int64_t workspace_bytes,
                       void* stream);

int64_t mrp_film_wmean_workspace(int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                                 int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P);

/*
 * The confidence-gated attention fusion (ABI 22, extended): mrp_film_attn_* over what was delivered.  Every
 * sender u attaches a per-pixel map w[u,p] >= 0 (mrp_film_wmean_*'s: (num_nodes, P) fp32, node stride
 * w_node_stride >= P, indexed by SOURCE node); at each pixel the receiver attends over the senders that
 * delivered something there, each weighted by its confidence.  An operator of its own: the attention kernels
 * compiled with the gate (a lane owns a pixel, so w is lane-private and enters the softmax step only); every
 * other entry point is unchanged.  Everything not restated here is exactly mrp_film_attn_*: row order, every
 * graph kind, parallel edges, self-loops, in-degree <= MRP_FILM_ATTN_DEGREE, MRP_AGG_GB_LOGITS, scale, node
 * strides, 16-bit widening.
 *
 * For destination v, entries j of its CSR row in row order, e_j the edge, u_j the source, w_j[p] = w[u_j,p].
 * Entry j is DELIVERED at p iff w_j[p] > 0; a zero, negative or NaN weight compares false: a silent entry.
 *
 *   m_j[c,p], s_j[p]     as mrp_film_attn_fwd, bit for bit (same chains, same order)
 *   mx[p]   = max over delivered j of s_j[p]
 *   u_j[p]  = exp(s_j[p] - mx[p])             v_exp_f32 on the difference, for every entry of the row
 *   t_j[p]  = fl(w_j[p] * u_j[p])             delivered entries
 *   Z[p]    = sum of t_j over delivered j     row order, one chain
 *   a_j[p]  = fl(t_j / Z)   delivered j and Z > 0 (IEEE division); 0 for a silent j, Z == 0, an empty row
 *   r_j[p]  = fl(u_j / Z)   EVERY entry where Z > 0 (IEEE division);  0 where nobody delivered
 *   out[v,c,p]  = sum over delivered j, row order, of a_j * m_j: the bare product at the first delivered entry,
 *                 an fma chain after it (film_attn's chain, started there); an exact 0 where nobody delivered
 *   attn[e_j,p] = a_j[p]    (E, P) fp32, an output
 *   rate[e_j,p] = r_j[p]    (E, P) fp32, an output; may be NULL (inference): only grad_w needs it
 *
 * Silent entries are skipped by per-lane selects, never multiplied by zero: a silent sender's features, however
 * non-finite, reach out, attn, grad_x and grad_gb nowhere — only that sender's own rate and grad_w at that
 * pixel (and, as for film_attn, whatever that node receives itself: its features are its own row's query).
 * mx is taken over the delivered entries only, so a silent entry that outscores every delivered one by more
 * than the fp32 exponent range has rate = +inf, and grad_w follows IEEE from there; nothing is clamped.
 *
 * Backward, g = grad_out[v].  It reads attn and rate as the forward wrote them and recomputes the messages,
 * not the softmax:
 *
 *   da_j[p]  = sum_c g[c,p] * m_j[c,p]                   every entry, channels ascending
 *   dbar[p]  = sum over delivered k, row order, of a_k * da_k     (an fma chain from 0)
 *   ds_j[p]  = a_j * (da_j - dbar)                       0 for a silent j
 *   dm_j, grad_x (query, key and value paths, + grad_x_base), grad_gb: mrp_film_attn_bwd's formulas with these
 *            a and ds; silent entries contribute nothing (their grad_gb rows are zeros)
 *   grad_w[u,p] = sum over all (v, j) with u_j = u of r_j[p] * (da_j[p] - dbar[p])     an fma chain from 0,
 *            destinations ascending, then row order
 *
 * grad_w is the exact one-sided derivative: it includes the entries with w_j = 0, where it is in general not
 * zero (as mrp_film_wmean_bwd's), and is 0 where Z = 0.  grad_w (num_nodes, P) fp32 with node stride
 * gw_node_stride >= P; every node's row is written (zeros for a node nobody hears).  A workgroup owns all of a
 * graph's nodes at its 64 pixels, so the sum never crosses a workgroup: the waves take turns in destination
 * order on one LDS cell per (node, pixel).  No atomics, one writer per element.
 *
 * Consequences, bit for bit on finite operands:
 *   - w == 1 gives mrp_film_attn_fwd's out and attn (rate == attn) and mrp_film_attn_bwd's grad_x and grad_gb;
 *   - a 0/1 map constant over each node's plane gives mrp_film_attn_*'s out, attn, grad_x and grad_gb on the
 *     graph without the silent robots' out-edges (same E and edge ids, rows compacted); the removed edges'
 *     rows are zeros on both sides;
 *   - 16-bit features: fwd(T, x) == T(fwd(float(x))); attn, rate, grad_gb and grad_w are equal in fp32, and
 *     grad_x == T(fp32 grad_x) on widened operands.
 *
 * Determinism and the order of every other sum: mrp_film_attn_*'s.  Preconditions: those of mrp_film_attn_*,
 * and w < +inf.
 *
 * grad_x, grad_gb and grad_w may each be NULL to skip that output; all NULL returns success without a launch
 * (grad_w alone skips the second channel sweep).  Validation precedes any launch and is mrp_film_attn_*'s; in
 * addition hipErrorInvalidValue is returned for a NULL w with work to do, w_node_stride < P, gw_node_stride < P
 * with grad_w wanted, a non-NULL grad_w with a NULL rate (where there are edges), and a workspace smaller than
 * needed.  Empty work returns success (attn, rate, grad_gb and grad_w, where given, are zeros).  No
 * allocation, no host synchronisation, capturable (hipMemsetAsync of attn, rate / grad_gb precedes the kernels
 * of non-COMPLETE graphs: rows no CSR entry names are zeros).
 *
 * mrp_film_wattn_workspace(direction, ...) is mrp_film_attn_workspace's value: 0 for the forward; for the
 * backward the per-tile grad_gb partials where a plane spans several 64-pixel tiles (needed only where grad_gb
 * is wanted; grad_w needs none).  It makes no GPU call.
 */
int mrp_film_wattn_fwd(int32_t dtype,
                       const void* x, int64_t x_node_stride,
                       const float* gb,
                       const float* w, int64_t w_node_stride,
                       const int32_t* indptr, const int32_t* src, const int32_t* eid,
                       const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                       int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                       int32_t C, int32_t P, int32_t flags,
                       void* out, int64_t out_node_stride,
                       float scale, float* attn, float* rate,
                       void* workspace, int64_t workspace_bytes,
                       void* stream);

int mrp_film_wattn_bwd(int32_t dtype,
                       const void* grad_out, int64_t g_node_stride,
                       const void* x, int64_t x_node_stride,
                       const float* gb,
                       const float* w, int64_t w_node_stride,
                       const int32_t* indptr, const int32_t* src, const int32_t* eid,
                       const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                       int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                       int32_t C, int32_t P, int32_t flags,
                       void* grad_x, int64_t gx_node_stride,
                       const void* grad_x_base, int64_t base_node_stride,
                       float* grad_gb,
                       float scale, const float* attn, const float* rate,
                       float* grad_w, int64_t gw_node_stride,
                       void* workspace, int64_t workspace_bytes,
                       void* stream);

int64_t mrp_film_wattn_workspace(int32_t direction, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                                 int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P);

/*
 * Multi-head attention fusion (ABI 22, extended): mrp_film_attn_* and mrp_film_wattn_* with `heads` = H
 * independent channel groups, so that different channel groups can listen to different robots at the same
 * pixel.  Ch = C / H; head k owns channels [k Ch, (k+1) Ch).  The signatures are the single-head ones with
 * `int32_t heads` after `C, P, flags` (after `C, P` in the workspace queries); every other entry point is
 * unchanged.
 *
 * Per-head formulas: for every head k, m_j, s_j, a_j, out, da, ds, dm, grad_x and grad_gb are
 * mrp_film_attn_*'s formulas with "sum over c" meaning the head's Ch channels, ascending; for the gated form
 * mx, t_j, Z, r_j and dbar follow the same rule.  One `scale` serves all heads (the customary value is
 * 1 / sqrt(Ch)).
 *
 * Outputs: attn, and rate for the gated form, are (H, E, P) fp32, head-major: attn + k E P is exactly the
 * (E, P) array of a single-head call.  out, grad_x and grad_gb keep their shapes.
 *
 * Confidence maps: w (num_nodes, P) is shared by all heads (a sender's map says where it transmits, not which
 * channels).  grad_w[u,p] is the sum over heads, ascending, of the single-head grad_w chain of that head:
 * head 0's value first, then one fp32 add per further head.  No atomics, one writer per element (every head
 * writes a partial (H, num_nodes, P) in the workspace and a reduce pass adds them in head order).
 *
 * Bit-level contract, for every graph kind, flag, dtype, node stride and base: head k of the H-head call equals
 * mrp_film_attn_fwd / _bwd (or mrp_film_wattn_*) called with C = Ch; x, out, grad_out, grad_x and grad_x_base
 * offset by k Ch P elements with the same node strides; a contiguous copy of gb[:, k Ch : (k+1) Ch, :]; and
 * attn + k E P, rate + k E P — bit for bit in out, attn, rate, grad_x and grad_gb[:, k Ch : (k+1) Ch, :];
 * grad_w equals the ordered head sum above.  (Chunk boundaries of the channel sweeps count from the head's
 * first channel.)  The order of every sum is a function of Ch, P and the graph only.  The 16-bit contract
 * carries over unchanged: fwd(T, x) == T(fwd(float(x))), and attn, rate, grad_gb, grad_w are equal in fp32.
 * heads = 1 runs the single-head kernels: the bits of mrp_film_attn_* / mrp_film_wattn_*.
 *
 * Non-finite values: the containment tightens.  A NaN or infinity at (node, channel c, pixel p) reaches only
 * the channels of c's head at p in out and grad_x, and only attn + k E P and rate + k E P of that head
 * (grad_gb: the columns of that head; grad_w sums over heads, so its element at (node, p) may be affected).
 *
 * Validation precedes any launch: everything the single-head entry points reject is rejected, and
 * hipErrorInvalidValue is also returned for heads < 1, for C > 0 with C % heads != 0 and for heads > 65535.
 * Empty work returns success, with attn, rate (all heads), grad_gb and grad_w, where given, written as zeros.
 * For non-COMPLETE graphs the hipMemsetAsync of attn, rate and grad_gb covers all heads.
 *
 * Workspace: with heads = 1 both queries return the single-head queries' values.  mrp_film_attn_workspace_mh is
 * mrp_film_attn_workspace's value for every H (the per-tile grad_gb partials [tile][E][C][2] hold every head's
 * columns).  mrp_film_wattn_workspace_mh(direction != 0) adds heads * num_nodes * P * 4 bytes when heads > 1:
 * grad_w's per-head partials, placed after the grad_gb partials that the call needs (at the start where
 * grad_gb is not wanted or a plane is one tile); that space is needed only where grad_w is wanted.
 *
 * Large operands: every typed pointer is offset in 64-bit arithmetic (k Ch P, k E P and k num_nodes P are formed
 * in int64_t), so the spans may exceed 2^31 elements as for the single-head entry points: x, out, grad_out,
 * grad_x and grad_x_base span (num_nodes - 1) * stride + C * P elements, attn and rate H * E * P floats.
 */
int mrp_film_attn_fwd_mh(int32_t dtype,
                         const void* x, int64_t x_node_stride,
                         const float* gb,
                         const int32_t* indptr, const int32_t* src, const int32_t* eid,
                         const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                         int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                         int32_t C, int32_t P, int32_t flags, int32_t heads,
                         void* out, int64_t out_node_stride,
                         float scale, float* attn,
                         void* workspace, int64_t workspace_bytes,
                         void* stream);

int mrp_film_attn_bwd_mh(int32_t dtype,
                         const void* grad_out, int64_t g_node_stride,
                         const void* x, int64_t x_node_stride,
                         const float* gb,
                         const int32_t* indptr, const int32_t* src, const int32_t* eid,
                         const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                         int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                         int32_t C, int32_t P, int32_t flags, int32_t heads,
                         void* grad_x, int64_t gx_node_stride,
                         const void* grad_x_base, int64_t base_node_stride,
                         float* grad_gb,
                         float scale, const float* attn,
                         void* workspace, int64_t workspace_bytes,
                         void* stream);

int64_t mrp_film_attn_workspace_mh(int32_t direction, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                                   int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t heads);

int mrp_film_wattn_fwd_mh(int32_t dtype,
                          const void* x, int64_t x_node_stride,
                          const float* gb,
                          const float* w, int64_t w_node_stride,
                          const int32_t* indptr, const int32_t* src, const int32_t* eid,
                          const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                          int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                          int32_t C, int32_t P, int32_t flags, int32_t heads,
                          void* out, int64_t out_node_stride,
                          float scale, float* attn, float* rate,
                          void* workspace, int64_t workspace_bytes,
                          void* stream);

int mrp_film_wattn_bwd_mh(int32_t dtype,
                          const void* grad_out, int64_t g_node_stride,
                          const void* x, int64_t x_node_stride,
                          const float* gb,
                          const float* w, int64_t w_node_stride,
                          const int32_t* indptr, const int32_t* src, const int32_t* eid,
                          const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                          int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                          int32_t C, int32_t P, int32_t flags, int32_t heads,
                          void* grad_x, int64_t gx_node_stride,
                          const void* grad_x_base, int64_t base_node_stride,
                          float* grad_gb,
                          float scale, const float* attn, const float* rate,
                          float* grad_w, int64_t gw_node_stride,
                          void* workspace, int64_t workspace_bytes,
                          void* stream);

int64_t mrp_film_wattn_workspace_mh(int32_t direction, int32_t num_graphs, int32_t max_nodes, int32_t graph_kind,
                                    int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t heads);

/*
 * The layer's 1x1 compress convolution and its gradients, fp32 on the matrix cores (exact fp32
 * products, v_mfma_f32_32x32x2_f32), without the concatenation (dgl/model/models.py:163-165,181-184,
 * 186-189: h = conv(torch.cat((x, a), 1)) with conv = nn.Conv2d(2C, C, kernel_size=1)).  W is the
 * conv weight (C, 2C) row-major (nn.Conv2d's (C, 2C, 1, 1)); x and a are the two halves of the
 * concatenation as separate node-major tensors (any node strides, e.g. the two halves of one cat
 * buffer).  Requirements (else hipErrorNotSupported): C % 32 == 0, P % 4 == 0, node strides % 4 == 0,
 * every tensor 16-byte aligned, and the node range one workgroup reads addressable with 31-bit byte
 * offsets: for the forward and the data gradient (128 / P + 2) node strides of x / agg / gy plus one node's
 * K rows below 2^31 bytes (the offsets are relative to the column tile's first node, not to the tensor, and
 * the outputs are written through 64-bit addresses: the tensors themselves may span any number of GiB,
 * tests/test_gpu_large_span.py); the weight gradient splits K so that every split's node range fits
 * (at most 2^31 / (4 max node stride) - 2 nodes per split and at most 256 splits: a node stride that
 * leaves less than one node per split, or more nodes than 256 such splits hold, is declined).
 *
 * mrp_compress_fwd:       y[n] = W[:, :C] x[n] + W[:, C:] a[n] + bias      (bias (C) may be NULL)
 * mrp_compress_bwd_data:  gx[n] = W[:, :C]^T gy[n],  ga[n] = W[:, C:]^T gy[n]
 *                         wt = W^T (2C, C), from mrp_compress_weight_transpose
 * mrp_compress_bwd_weight: gw = sum_n gy[n] [x[n]; a[n]]^T (C, 2C),  gbias = sum_{n,p} gy (may be
 *                         NULL); split over the node-pixel axis into workspace (>=
 *                         mrp_compress_bwd_weight_workspace bytes for the largest of the three node
 *                         strides, 16-byte aligned; 0 = none needed), partial sums added in a fixed
 *                         order (deterministic).  Also needs P % 32 == 0 and C % 8 == 0.
 */
int mrp_compress_fwd(const float* x, int64_t x_node_stride, const float* a, int64_t a_node_stride,
                     int32_t num_nodes, int32_t C, int32_t P, const float* w, const float* bias,
                     float* y, int64_t y_node_stride, void* stream);
int mrp_compress_weight_transpose(const float* w, float* wt, int32_t C, void* stream);
int mrp_compress_bwd_data(const float* gy, int64_t gy_node_stride, int32_t num_nodes, int32_t C, int32_t P,
                          const float* wt, float* gx, int64_t gx_node_stride, float* ga, int64_t ga_node_stride,
                          void* stream);
int64_t mrp_compress_bwd_weight_workspace(int32_t num_nodes, int32_t C, int32_t P, int64_t max_node_stride);
int mrp_compress_bwd_weight(const float* gy, int64_t gy_node_stride, const float* x, int64_t x_node_stride,
                            const float* a, int64_t a_node_stride, int32_t num_nodes, int32_t C, int32_t P,
                            float* gw, float* gbias, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * The compress forward and data gradient on the bf16 matrix cores at fp32 accuracy
 * (compress_split.hip): the same products as mrp_compress_fwd / mrp_compress_bwd_data, each fp32
 * operand split exactly into three bf16 parts and each product the sum of the six partial products
 * whose omitted terms are below 2^-25 of it (error against float64 about an fp32 GEMM's: measured 0.3 to
 * 0.9 x torch's at K = 1024, bounded by 2 x in tests/test_gpu_split_fp32.py).
 * Domain (every split-bf16 kernel: compress, node-major and pixel-major, and the edge encoder): the accuracy
 * is relative to sum |a_k b_k| and independent of the operands' scale — scaling the operands by powers of two
 * scales the result bit for bit — as long as every non-zero bf16 part of every operand is a normal bf16 and
 * nothing overflows (tested for operands scaled by 2^-100 .. 2^100, products by 2^-110 .. 2^120); below
 * that the low parts are lost and the accuracy degrades towards bf16's.  A finite operand with
 * |x| >= 2^128 - 2^119 (0x7f7f8000) is outside the domain: it rounds to a bf16 infinity, its residual is
 * -inf, and every product that reads it is NaN (its output row or column; nothing else).  The
 * weight operand is split and laid out once per weight version:
 *   mrp_compress_split_pack_bytes(M, K)   bytes of a packed M x K operand (0 unless M % 32 == 0, K % 16 == 0)
 *   mrp_compress_split_pack(w, ld, transpose, M, K, packed)
 *                                         A = w (M x K row-major, row stride ld) or, transpose != 0,
 *                                         A = w^T (w: K x M row-major, row stride ld) -> packed (16-byte aligned)
 *   mrp_compress_fwd_split                y = W [x; agg] + b with packed = pack(w, 2C, 0, C, 2C)
 *   mrp_compress_bwd_data_split           [gx; gagg] = W^T gy with packed = pack(w, 2C, 1, 2C, C)
 * Arguments otherwise as mrp_compress_fwd / mrp_compress_bwd_data.  Requirements (else
 * hipErrorNotSupported): C % 32 == 0, P % 4 == 0, x / agg / gy 16-byte aligned with node strides % 4 == 0.
 * No span limit: operands and outputs are addressed with 64-bit node offsets (where an output's node range
 * passes 31-bit byte offsets the 128-row form, whose stores are 64-bit, runs instead of the 256-row one).
 */
int64_t mrp_compress_split_pack_bytes(int32_t M, int32_t K);
int mrp_compress_split_pack(const float* w, int64_t ld, int32_t transpose, int32_t M, int32_t K, void* packed,
                            void* stream);
int mrp_compress_fwd_split(const float* x, int64_t x_node_stride, const float* agg, int64_t agg_node_stride,
                           int32_t num_nodes, int32_t C, int32_t P, const void* packed_w, const float* bias, float* y,
                           int64_t y_node_stride, void* stream);
int mrp_compress_bwd_data_split(const float* gy, int64_t gy_node_stride, int32_t num_nodes, int32_t C, int32_t P,
                                const void* packed_wt, float* gx, int64_t gx_node_stride, float* gagg,
                                int64_t gagg_node_stride, void* stream);

/*
 * The compress weight gradient (mrp_compress_bwd_weight's products) on the split-bf16 matrix cores:
 * both operands are activations, split in the kernel on their way into LDS; K = num_nodes P split over
 * workgroups into partial tiles summed in a fixed order (deterministic).  Workspace: device buffer of
 * mrp_compress_bwd_weight_split_workspace(num_nodes, C, P) bytes (0: none needed).  Requirements (else
 * hipErrorNotSupported): C % 64 == 0, P % 32 == 0, 16-byte aligned operands, node strides % 4 == 0.
 */
int64_t mrp_compress_bwd_weight_split_workspace(int32_t num_nodes, int32_t C, int32_t P);
int mrp_compress_bwd_weight_split(const float* gy, int64_t gy_node_stride, const float* x, int64_t x_node_stride,
                                  const float* a, int64_t a_node_stride, int32_t num_nodes, int32_t C, int32_t P,
                                  float* gw, float* gbias, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * The three split-bf16 compress products with a selectable part count: the arguments of
 * mrp_compress_fwd_split / _bwd_data_split / _bwd_weight_split plus `parts` before `stream`.  A kernel
 * with `parts` = 3 / 2 / 1 keeps the first `parts` bf16 parts of each fp32 operand (x = x0 + x1 + x2, each
 * part the bf16 rounding of what the earlier ones left) and sums the partial products a_i b_j with
 * i + j < parts: six, three (a0 b0 + a0 b1 + a1 b0, "bf16x3") or one (bf16 operands).  The dropped
 * parts are not converted, not staged in LDS, not read and — for the packed weight image, whose parts
 * are separate 1 KiB pieces — not fetched; the image itself is mrp_compress_split_pack's three-part one
 * for every `parts` (no repack when the count changes).  a0 b0 accumulates alone, the other products in
 * a second fp32 accumulator, the two summed once at the end.
 * Error model, per term a_k b_k of a product (then fp32 accumulation of the partial sums as above):
 *   parts = 3: the omitted terms are below 2^-25 |a_k b_k| (the existing entry points' model);
 *   parts = 2: the dropped terms are a1 b1 and the two-part residuals (a - a0 - a1) b, a (b - b0 - b1):
 *              with a rounding unit of 2^-9 per bf16 part (|a1| <= 2^-9 |a|, residual <= 2^-18 |a|)
 *              at most (2^-18 + 2 x 2^-18 + higher orders) |a_k b_k| <= 3.1 x 2^-18 |a_k b_k|;
 *   parts = 1: |a - a0| <= 2^-9 |a| in both operands: at most 2.01 x 2^-9 |a_k b_k|.
 *   These are the bounds tests/test_gpu_compress_precision.py holds the kernels to against
 *   sum_k |a_k b_k|.  2^-9 is the rounding unit of a value just below a power of two; just above one a
 *   bf16 step is twice as wide (bf16 carries 8 significant bits: unit 2^-8), so a single term can reach
 *   2.01 x 2^-8 (parts = 1) and 3.1 x 2^-16 (parts = 2) of itself.  Over a sum the roundings do not
 *   align: measured errors are recorded in DESIGN.md §3.11.
 * gbias is the fp32 sum of the full gy for every `parts`, never of a truncated image.
 * Returns: `parts` outside {1, 2, 3}: hipErrorInvalidValue before anything else; zero sizes: success
 * without a launch (the weight gradient's empty sum zeroes its outputs as _bwd_weight_split does);
 * hipErrorNotSupported exactly where the existing entry point returns it; parts = 3 is the existing
 * entry point (bit-identical — the existing ones call these with 3).
 * mrp_compress_bwd_weight_split_workspace(num_nodes, C, P) is the workspace bound for every `parts`: a
 * reduced form never needs more (its pre-split image of gy takes 2 parts bytes per element of the six
 * the bound reserves, at the same offsets).
 */
int mrp_compress_fwd_split_p(const float* x, int64_t x_node_stride, const float* agg, int64_t agg_node_stride,
                             int32_t num_nodes, int32_t C, int32_t P, const void* packed_w, const float* bias,
                             float* y, int64_t y_node_stride, int32_t parts, void* stream);
int mrp_compress_bwd_data_split_p(const float* gy, int64_t gy_node_stride, int32_t num_nodes, int32_t C, int32_t P,
                                  const void* packed_wt, float* gx, int64_t gx_node_stride, float* gagg,
                                  int64_t gagg_node_stride, int32_t parts, void* stream);
int mrp_compress_bwd_weight_split_p(const float* gy, int64_t gy_node_stride, const float* x, int64_t x_node_stride,
                                    const float* a, int64_t a_node_stride, int32_t num_nodes, int32_t C, int32_t P,
                                    float* gw, float* gbias, void* workspace, int64_t workspace_bytes,
                                    int32_t parts, void* stream);

/*
 * The compress forward and both gradients on bf16 / fp16 feature maps (compress_half.hip; dtype is
 * MRP_DTYPE_BF16 or MRP_DTYPE_F16 = T, the storage type of x, agg, y, gy, gx and gagg; the parameters
 * and their gradients are fp32).  The same products as the _split entry points, one
 * v_mfma_f32_16x16x32_{bf16,f16} per product:
 *   mrp_compress_pack_t_bytes(M, K)   bytes of a packed M x K operand, 2 per element (0 unless
 *                                     M % 32 == 0 and K % 32 == 0)
 *   mrp_compress_pack_t               A = w (or w^T, as mrp_compress_split_pack) rounded once to T, round
 *                                     to nearest even -> packed (16-byte aligned)
 *   mrp_compress_fwd_t                y = T(W_T [x; agg] + bias): fp32 accumulation, the fp32 bias (C, may
 *                                     be NULL) added to the fp32 sum, one rounding at the store;
 *                                     packed = pack_t(w, 2C, 0, C, 2C)
 *   mrp_compress_bwd_data_t           [gx; gagg] = T(W_T^T gy), packed = pack_t(w, 2C, 1, 2C, C); gx and
 *                                     gagg are separate node-major outputs with their own node strides
 *   mrp_compress_bwd_weight_t         gw (C, 2C) = sum_n gy[n] [x[n]; agg[n]]^T and gbias (C, may be NULL)
 *                                     = sum gy, accumulated and stored in fp32 (never rounded to T);
 *                                     K = num_nodes P split over workgroups into fp32 partial tiles in
 *                                     workspace (mrp_compress_bwd_weight_t_workspace bytes, 16-byte
 *                                     aligned; 0: none needed), summed in a fixed order: deterministic
 * Before any launch: MRP_DTYPE_F32 or an unknown dtype, a NULL pointer with work to do, a node stride
 * below C P, a pointer that is not 16-byte aligned, a node stride that is not a multiple of 8 elements
 * or a workspace that is too small return hipErrorInvalidValue; zero sizes return success without a
 * launch (an empty weight-gradient sum zeroes gw / gbias).  Shapes the kernels do not tile return
 * hipErrorNotSupported: C % 32 != 0, P % 8 != 0 (forward, data gradient), P % 32 != 0 (weight
 * gradient), an output node range beyond 31-bit byte offsets (forward, data gradient: y, gx or gagg with
 * ((num_nodes - 1) node strides + C P) elements of 2 bytes reaching 2^31 bytes — their stores go through
 * 32-bit buffer offsets; nodes are independent, so a caller covers a wider output with one call per node
 * range that fits, as compress.py does; the operands x, agg, gy of all three entry points are read through
 * 64-bit addresses and may span any number of GiB, and the weight gradient has no span limit) — and every
 * shape while the tuning knob "compress_half" is 0.  No host synchronisation; stream-capturable.
 */
int64_t mrp_compress_pack_t_bytes(int32_t M, int32_t K);
int mrp_compress_pack_t(int32_t dtype, const float* w, int64_t ld, int32_t transpose, int32_t M, int32_t K,
                        void* packed, void* stream);
int mrp_compress_fwd_t(int32_t dtype, const void* x, int64_t x_node_stride, const void* agg, int64_t agg_node_stride,
                       int32_t num_nodes, int32_t C, int32_t P, const void* packed_w, const float* bias, void* y,
                       int64_t y_node_stride, void* stream);
int mrp_compress_bwd_data_t(int32_t dtype, const void* gy, int64_t gy_node_stride, int32_t num_nodes, int32_t C,
                            int32_t P, const void* packed_wt, void* gx, int64_t gx_node_stride, void* gagg,
                            int64_t gagg_node_stride, void* stream);
int64_t mrp_compress_bwd_weight_t_workspace(int32_t num_nodes, int32_t C, int32_t P);
int mrp_compress_bwd_weight_t(int32_t dtype, const void* gy, int64_t gy_node_stride, const void* x,
                              int64_t x_node_stride, const void* agg, int64_t agg_node_stride, int32_t num_nodes,
                              int32_t C, int32_t P, float* gw, float* gbias, void* workspace,
                              int64_t workspace_bytes, void* stream);

/*
 * The same three products on pixel-major (torch.channels_last) bf16 / fp16 feature maps
 * (compress_half_cl.hip).  Every feature tensor is a (pointer, node stride, pixel stride) triple in
 * elements, as the _cl aggregation entry points define it: pixel p of node n is C contiguous channels at
 * n * node_stride + p * pixel_stride — pixel stride C for a dense channels_last map, 2C for either half
 * of a channels_last concatenation buffer; node_stride >= P * pixel_stride, not necessarily equal.  The
 * arithmetic is the _t entry points': the weight rounded once to T when packed (the same
 * mrp_compress_pack_t images: pack_t(w, 2C, 0, C, 2C) for the forward, pack_t(w, 2C, 1, 2C, C) for the data
 * gradient), fp32 accumulation, the fp32 bias (may be NULL) added to the fp32 sum, one rounding at the
 * store; gw (C, 2C) and gbias (C, may be NULL) accumulated and stored in fp32.
 *   mrp_compress_fwd_cl                  y = T(W_T [x; agg] + bias) per pixel row
 *   mrp_compress_bwd_data_cl             [gx; gagg] = T(W_T^T gy): two pixel-major outputs with their own
 *                                        strides (e.g. the halves of one channels_last 2C buffer)
 *   mrp_compress_bwd_weight_cl           gw = sum gy [x; agg]^T, gbias = sum gy over all num_nodes P pixel
 *                                        rows, split into fp32 partial tiles in workspace
 *                                        (mrp_compress_bwd_weight_cl_workspace bytes, 16-byte aligned; 0:
 *                                        none needed) summed in a fixed order by a second launch: no
 *                                        atomics, two runs give the same bits
 * Pixels are rows: any P is tiled (no padding; a stage may cross a node boundary).  Before any launch:
 * MRP_DTYPE_F32 or an unknown dtype, a NULL pointer with work to do, a pointer that is not 16-byte
 * aligned, a node or pixel stride that is not a multiple of 8 elements, a pixel stride below C, a node
 * stride below P pixel strides or a workspace that is too small return hipErrorInvalidValue; zero sizes
 * return success without a launch (an empty weight-gradient sum zeroes gw / gbias).  C % 32 != 0, a
 * packed image or a pixel-row count beyond 31 bits — and every shape while the tuning knob
 * "compress_half_cl" is 0 — return hipErrorNotSupported.  mrp_compress_bwd_weight_cl needs gw whenever
 * it has work to do (gbias alone is not computed: gw == NULL with gbias != NULL is hipErrorInvalidValue;
 * both NULL is a no-op).  The knob is for callers of this C interface: compress.py does not consult it
 * (its own switch is compress.set_channels_last_compress) and raises on a declined pixel-major call.  No
 * host synchronisation; stream-capturable.
 */
int mrp_compress_fwd_cl(int32_t dtype, const void* x, int64_t x_node_stride, int64_t x_pixel_stride, const void* agg,
                        int64_t agg_node_stride, int64_t agg_pixel_stride, int32_t num_nodes, int32_t C, int32_t P,
                        const void* packed_w, const float* bias, void* y, int64_t y_node_stride,
                        int64_t y_pixel_stride, void* stream);
int mrp_compress_bwd_data_cl(int32_t dtype, const void* gy, int64_t gy_node_stride, int64_t gy_pixel_stride,
                             int32_t num_nodes, int32_t C, int32_t P, const void* packed_wt, void* gx,
                             int64_t gx_node_stride, int64_t gx_pixel_stride, void* gagg, int64_t gagg_node_stride,
                             int64_t gagg_pixel_stride, void* stream);
int64_t mrp_compress_bwd_weight_cl_workspace(int32_t num_nodes, int32_t C, int32_t P);
int mrp_compress_bwd_weight_cl(int32_t dtype, const void* gy, int64_t gy_node_stride, int64_t gy_pixel_stride,
                               const void* x, int64_t x_node_stride, int64_t x_pixel_stride, const void* agg,
                               int64_t agg_node_stride, int64_t agg_pixel_stride, int32_t num_nodes, int32_t C,
                               int32_t P, float* gw, float* gbias, void* workspace, int64_t workspace_bytes,
                               void* stream);

/*
 * The split-bf16 compress on pixel-major (torch.channels_last) fp32 feature maps (compress_split_cl.hip):
 * the _split_p entry points' three products with every feature tensor a (pointer, node stride, pixel
 * stride) triple in elements, as the _cl entry points above define it (pixel stride C for a dense
 * channels_last map, 2C for either half of a channels_last concatenation buffer; node_stride >=
 * P * pixel_stride).  The arithmetic is the _split_p block's: the exact bf16 split of each fp32 operand,
 * the partial products with i + j < parts (parts = 3: fp32 accuracy; 2 / 1: the reduced forms and their
 * per-term bounds stated there), a0 b0 in an accumulator of its own, fp32 accumulation and outputs; the
 * k order inside a product differs from the node-major kernels', so results agree with them to fp32
 * rounding, not bit for bit.  The packed weight images are mrp_compress_split_pack's, the same for
 * every `parts`: pack(w, 2C, 0, C, 2C) for the forward, pack(w, 2C, 1, 2C, C) for the data gradient.
 *   mrp_compress_fwd_split_cl            y = W [x; agg] + bias (C, may be NULL) per pixel row
 *   mrp_compress_bwd_data_split_cl       [gx; gagg] = W^T gy: two pixel-major outputs with their own
 *                                        strides (e.g. the halves of one channels_last 2C buffer)
 *   mrp_compress_bwd_weight_split_cl     gw (C, 2C) = sum gy [x; agg]^T and gbias (C, may be NULL) = sum gy
 *                                        over all num_nodes P pixel rows; K = num_nodes P is split over
 *                                        workgroups into fp32 partial tiles in workspace
 *                                        (mrp_compress_bwd_weight_split_cl_workspace bytes, 16-byte
 *                                        aligned; 0: none needed; the bound holds for every `parts`)
 *                                        summed in a fixed order by a second launch: no atomics, two runs
 *                                        give the same bits.  gbias is the fp32 sum of the full gy for
 *                                        every `parts`.
 * Pixels are rows: any P is tiled (no padding; a tile or stage may cross a node boundary).  Operands and
 * outputs are addressed through 64-bit arithmetic: no span limit, no per-node-range calls.  Returns, all
 * before any launch: `parts` outside {1, 2, 3}: hipErrorInvalidValue before anything else; a NULL pointer
 * with work to do, a pointer that is not 16-byte aligned, a node or pixel stride that is not a multiple of
 * 4 elements, a pixel stride below C, a node stride below P pixel strides, a workspace that is too small
 * or gw == NULL with gbias != NULL: hipErrorInvalidValue; zero sizes: success without a launch (an empty
 * weight-gradient sum zeroes gw / gbias; gw and gbias both NULL is a no-op); C % 32 != 0, a pixel-row
 * count or a packed image beyond 31 bits — and every shape while the tuning knob "compress_split_cl" is
 * 0 — hipErrorNotSupported.  The knob "split_cl_splits" forces the weight gradient's split-K count
 * (0 default = the planner's).  The error model otherwise is the _split_p block's.  No host
 * synchronisation; stream-capturable.
 */
int mrp_compress_fwd_split_cl(const float* x, int64_t x_node_stride, int64_t x_pixel_stride, const float* agg,
                              int64_t agg_node_stride, int64_t agg_pixel_stride, int32_t num_nodes, int32_t C,
                              int32_t P, const void* packed_w, const float* bias, float* y, int64_t y_node_stride,
                              int64_t y_pixel_stride, int32_t parts, void* stream);
int mrp_compress_bwd_data_split_cl(const float* gy, int64_t gy_node_stride, int64_t gy_pixel_stride,
                                   int32_t num_nodes, int32_t C, int32_t P, const void* packed_wt, float* gx,
                                   int64_t gx_node_stride, int64_t gx_pixel_stride, float* gagg,
                                   int64_t gagg_node_stride, int64_t gagg_pixel_stride, int32_t parts, void* stream);
int64_t mrp_compress_bwd_weight_split_cl_workspace(int32_t num_nodes, int32_t C, int32_t P);
int mrp_compress_bwd_weight_split_cl(const float* gy, int64_t gy_node_stride, int64_t gy_pixel_stride, const float* x,
                                     int64_t x_node_stride, int64_t x_pixel_stride, const float* agg,
                                     int64_t agg_node_stride, int64_t agg_pixel_stride, int32_t num_nodes, int32_t C,
                                     int32_t P, float* gw, float* gbias, void* workspace, int64_t workspace_bytes,
                                     int32_t parts, void* stream);

/*
 * First layer of the edge encoder, dgl/model/models.py:147-148:  h = relu(pose W1^T + b1).
 *   pose (num_edges, 9), w1 (C, 9) (nn.Linear weight layout), b1 (C) -> h (num_edges, C), fp32.
 * The second Linear is mrp_edge_logits_fwd and its Sigmoid is fused into the aggregation
 * (MRP_AGG_GB_LOGITS).
 */
int mrp_edge_hidden_fwd(const float* pose, const float* w1, const float* b1,
                        int32_t num_edges, int32_t C, float* h, void* stream);

/*
 * Second layer of the edge encoder before its Sigmoid, dgl/model/models.py:149:
 *   z = h W2^T + b2,  h (num_edges, C), w2 (2C, C) (nn.Linear weight layout), b2 (2C) -> z (num_edges, 2C)
 * fp32 on the matrix cores (exact fp32 products), the bias added in the epilogue.  z is the logits
 * tensor the aggregation reads with MRP_AGG_GB_LOGITS.  Requirements (else hipErrorNotSupported):
 * C % 32 == 0, h and w2 16-byte aligned, h and w2 under 2^31 bytes.
 */
int mrp_edge_logits_fwd(const float* h, int32_t num_edges, int32_t C, const float* w2, const float* b2,
                        float* z, void* stream);

/*
 * The edge encoder before its Sigmoid in one launch (dgl/model/models.py:146-149),
 *   z = relu(pose W1^T + b1) W2^T + b2     pose (num_edges, 9), w1 (C, 9), b1 (C), w2 (2C, C), b2 (2C),
 * at fp32 accuracy on the bf16 matrix cores (encoder_split.hip): every fp32 operand is
 * split exactly into three bf16 parts and each product is the sum of the six partial products whose
 * omitted terms are below 2^-25 of it (error against float64 about an fp32 GEMM's: measured 1.1 x torch's
 * at C = 1024, bounded by 2 x in tests/test_gpu_split_fp32.py); the hidden
 * layer is computed on the matrix cores too (b1 as a tenth input of value 1.0) and never written.
 * The weights are split and laid out once per weight version:
 *   mrp_edge_encoder_pack_bytes(C)  bytes of the packed image (0 if C <= 0 or C % 32 != 0)
 *   mrp_edge_encoder_pack           w1 (C, 9), b1 (C), w2 (2C, C) -> packed (16-byte aligned device buffer)
 *   mrp_edge_encoder_fwd_split      z = relu(pose W1^T + b1) W2^T + b2 from pose (E, 9), the packed image
 *                                   and b2 (2C, or NULL) -> z (E, 2C)
 * Requirements (else hipErrorNotSupported): C % 32 == 0 and a packed image below 2^31 bytes (the
 * kernel addresses it with 32-bit offsets: C <= 13344).  The z accumulation keeps the a0 b0 products
 * apart from the five small ones (two accumulators per output, summed once).  Used for inference;
 * training keeps h for its backward and runs mrp_edge_hidden_fwd + mrp_edge_logits_fwd.
 */
int64_t mrp_edge_encoder_pack_bytes(int32_t C);
int mrp_edge_encoder_pack(const float* w1, const float* b1, const float* w2, int32_t C, void* packed, void* stream);
int mrp_edge_encoder_fwd_split(const float* pose, const void* packed, const float* b2, int32_t num_edges, int32_t C,
                               float* z, void* stream);

/*
 * The encoder's training path on the split-bf16 matrix cores (replaces mrp_edge_hidden_fwd +
 * mrp_edge_logits_fwd forward and the two library GEMMs of the backward, dgl/model/models.py:146-149
 * under dgl/training.py:208-210's loss.backward(); the forward in encoder_split.hip, _bwd_prep / _bwd_t in
 * edge_encoder.hip, _bwd_split / _bwd_fused in encoder_bwd_split.hip):
 *   mrp_edge_encoder_fwd_split_train  as mrp_edge_encoder_fwd_split (shared-hidden form), and also
 *                                      h^T = relu(pose W1^T + b1)^T, (C, E) rows of hT_stride >= E floats
 *   mrp_edge_encoder_bwd_prep          dzT (2C, E) rows of dzT_stride >= E = dz^T (E % 4 == 0, C even,
 *                                      16-byte aligned, dzT_stride % 4 == 0; else hipErrorNotSupported)
 *   mrp_edge_encoder_bwd_split         dh^T (C, E) = W2^T dz^T and dW2 (2C, C) = dz^T h on the split-bf16
 *                                      weight-gradient kernel (either output may be NULL), with db2 (2C) =
 *                                      column sums of dz taken on the dW2 product (NULL, or dw2 non-NULL);
 *                                      w2T = W2^T (C, 2C) row-major; dzT and hT with row stride E;
 *                                      workspace: _split_workspace(E, C) bytes (0 if none is needed) —
 *                                      the two products may be issued as two calls on two streams, each
 *                                      with its own workspace
 *   mrp_edge_encoder_bwd_t             dpre = dh^T (.) [h^T > 0]: dw1 (C, 9) = dpre pose, db1 (C) = row sums
 *                                      (either may be NULL); workspace: _t_workspace(E, C) bytes
 *   mrp_edge_encoder_bwd_fused         the whole backward of the encoder's parameters in three launches
 *                                      on one stream: dz^T; dh^T and dW2 as ONE launch of both split-K
 *                                      products; a reduction that sums their partial tiles, applies the
 *                                      ReLU mask and forms dW1 / db1 (dh^T never written).  dw1, db1,
 *                                      dw2, db2 all required (no dpose); w2T_packed: NULL, or W2^T's
 *                                      packed split image (mrp_compress_split_pack(w2, C, 1, C, 2C), 16-byte
 *                                      aligned), which the dh^T product then reads instead of splitting
 *                                      w2T in every workgroup, and dz^T is then written as a packed image
 *                                      for the dW2 product too (same products, same order: dW1, db1 and
 *                                      dW2 bit-identical to the split form; db2 summed per 64-edge block);
 *                                      workspace: _fused_workspace(E, C) bytes
 *   mrp_edge_encoder_bwd_pose          the pose gradient (the encoder's input, wanted only when poses
 *                                      require grad): dpose (E, 9) = dpre^T W1 with dpre as for _bwd_t;
 *                                      any E, C; workspace: _pose_workspace(E, C) bytes (0: none needed)
 * Requirements of _bwd_split and _bwd_fused (else hipErrorNotSupported): E % 32 == 0, C % 32 == 0,
 * 16-byte aligned operands.  Shapes outside them run the same kernels on zero-padded operands
 * (encoder.py, EdgeEncoderPaddedFunction: E and C rounded up to 32, zero weight rows and columns, zero
 * gradient rows — every padded term a product with an exact zero).  All sums in a fixed order:
 * deterministic.
 */
int mrp_edge_encoder_fwd_split_train(const float* pose, const void* packed, const float* b2, int32_t num_edges,
                                     int32_t C, float* z, float* hT, int64_t hT_stride, void* stream);
int mrp_edge_encoder_bwd_prep(const float* dz, int32_t num_edges, int32_t C, float* dzT, int64_t dzT_stride,
                              void* stream);
int64_t mrp_edge_encoder_bwd_split_workspace(int32_t num_edges, int32_t C);
int mrp_edge_encoder_bwd_split(const float* dz, const float* dzT, const float* w2T, const float* hT,
                               int32_t num_edges, int32_t C, float* dhT, float* dw2, float* db2, void* workspace,
                               int64_t workspace_bytes, void* stream);
int64_t mrp_edge_encoder_bwd_fused_workspace(int32_t num_edges, int32_t C);
int mrp_edge_encoder_bwd_fused(const float* dz, const float* w2T, const void* w2T_packed, const float* hT,
                               const float* pose, int32_t num_edges, int32_t C, float* dw1, float* db1, float* dw2,
                               float* db2, void* workspace, int64_t workspace_bytes, void* stream);
int64_t mrp_edge_encoder_bwd_t_workspace(int32_t num_edges, int32_t C);
int mrp_edge_encoder_bwd_t(const float* dhT, int64_t dhT_stride, const float* hT, int64_t hT_stride,
                           const float* pose, int32_t num_edges, int32_t C, float* dw1, float* db1, void* workspace,
                           int64_t workspace_bytes, void* stream);
int64_t mrp_edge_encoder_bwd_pose_workspace(int32_t num_edges, int32_t C);
int mrp_edge_encoder_bwd_pose(const float* dhT, int64_t dhT_stride, const float* hT, int64_t hT_stride,
                              const float* w1, int32_t num_edges, int32_t C, float* dpose, void* workspace,
                              int64_t workspace_bytes, void* stream);

/*
 * Backward of the edge encoder's reductions (dgl/model/models.py:147-149), run after the two
 * library GEMMs of its backward (dh = dz W2, dW2 = dz^T h):
 *   db2[j]    = sum_e dz[e, j]                              (dz: (E, 2C), the logits' gradient that
 *                                                            mrp_film_mean_bwd writes with MRP_AGG_GB_LOGITS)
 *   dw1[k, i] = sum_e dh[e, k] * [h[e, k] > 0] * pose[e, i] (dh, h: (E, C); pose (E, 9); dw1 (C, 9))
 *   db1[k]    = sum_e dh[e, k] * [h[e, k] > 0]
 * workspace: device buffer of mrp_edge_encoder_bwd_workspace(E, C) bytes.  Outputs may be NULL.
 * Deterministic (fixed summation order, no atomics).
 */
int64_t mrp_edge_encoder_bwd_workspace(int32_t num_edges, int32_t C);
int mrp_edge_encoder_bwd(const float* dz, const float* dh, const float* h, const float* pose,
                         int32_t num_edges, int32_t C, float* db2, float* dw1, float* db1,
                         float* workspace, void* stream);

/*
 * Per-frame robot graphs built on the device (dgl/dataloader.py:88-122 with the relative pose of
 * dgl/utils.py:54-77), for a batch of num_graphs frames of n robots each (n <= MRP_MAX_NODES).
 *
 *   poses      (num_graphs * n, 7) fp32 rows (tx, ty, tz, qx, qy, qz, qw), graph by graph
 *   knn_k      0: complete graphs, the reference topology: all ordered pairs u != v, edges numbered
 *                 graph by graph i-major (the MRP_GRAPH_COMPLETE numbering), E = num_graphs*n*(n-1);
 *              k (1 <= k < n): k-NN graphs: destination v's sources are the k robots u != v with the
 *                 smallest |t_u - t_v| (float64, ties to the lower index), edges numbered
 *                 destination-major with sources ascending, E = num_graphs*n*k (MRP_GRAPH_REGULAR(k))
 *   edge_pose  (E, 9) fp32: cal_relative_pose(pose[src e], pose[dst e]), bit-identical to the
 *              reference's float32 arithmetic
 *   indptr     (num_graphs*n + 1), src (E), eid (E): CSR by destination, in-edges by increasing
 *              edge id; graph_off (num_graphs + 1) — the graph arguments of the aggregation calls
 * Any output pointer may be NULL to skip it.  Returns hipErrorInvalidValue for n > MRP_MAX_NODES,
 * k >= n or sizes beyond int32.
 */
int mrp_frame_graph_build(const float* poses, int32_t num_graphs, int32_t n, int32_t knn_k,
                          float* edge_pose, int32_t* indptr, int32_t* src, int32_t* eid,
                          int32_t* graph_off, void* stream);

/*
 * Range-limited / drop-out frames built on the device: graphs of kind MRP_GRAPH_SIMPLE.
 *
 *   poses      as above
 *   active     (num_graphs * n) bytes, nonzero = the robot takes part; NULL = all do
 *   knn_k      0: every robot in range; k (1 <= k < n): each destination keeps at most the k nearest
 *              of those (ties to the lower index)
 *   max_range  edge u->v exists iff u != v, both robots are active and d(u, v) <= max_range, with d the
 *              float64 distance of the translations, sqrt((dx^2 + dy^2) + dz^2) as in the k-NN rule;
 *              the comparison is inclusive, a NaN distance gives no edge, +inf means unlimited
 *   edge_pose  (num_graphs*n*(n-1), 9): every ordered pair's relative pose, present or not — the
 *              rows, numbering and bits of mrp_frame_graph_build(knn_k = 0)
 *   indptr     (num_graphs*n + 1); src, eid (capacity num_graphs*n*(n-1), indptr[num_graphs*n] used):
 *              the existing edges only, destination-major with sources ascending, eid = the complete
 *              graph's id b*n*(n-1) + u*(n-1) + (v < u ? v : v-1)
 *   graph_off  (num_graphs + 1): graph_off[b] = b*n — every robot stays a node; an inactive one has
 *              no edge in or out
 *   workspace  mrp_frame_graph_build_range_workspace(num_graphs, n) bytes of device memory, 4-byte
 *              aligned (the in-degrees' block totals of the prefix sum)
 * The aggregation calls then take num_edges = num_graphs*n*(n-1) (the rows of gb) and kind
 * MRP_GRAPH_SIMPLE.  Three launches on `stream`, no host read-back and no allocation: capturable, and
 * deterministic (the prefix sum is a fixed tree, no atomics).  Any output pointer may be NULL to skip it.
 * Returns hipErrorInvalidValue before any launch for n > MRP_MAX_NODES, knn_k < 0 or knn_k >= n (n > 0), a
 * NaN or negative max_range, a workspace that is NULL or too small, or sizes beyond int32.
 */
int mrp_frame_graph_build_range(const float* poses, const uint8_t* active, int32_t num_graphs, int32_t n,
                                int32_t knn_k, double max_range, float* edge_pose, int32_t* indptr,
                                int32_t* src, int32_t* eid, int32_t* graph_off, void* workspace,
                                int64_t workspace_bytes, void* stream);
int64_t mrp_frame_graph_build_range_workspace(int32_t num_graphs, int32_t n);

/* Experiment knobs of the launchers (kernel-lab sweeps; not needed for normal use; process-wide,
 * not thread-safe).  Returns hipErrorInvalidValue for an unknown name or a value out of range;
 * "reset" restores every default.  Geometry: "fwd_lo"/"fwd_hi"/"fwd_cap", "fwd_regular_*",
 * "bwd_fused_*", "bwd_regular_*" (the planners clamp what a kernel cannot run: at most 64 lanes per plane
 * in film_bwd_regular, channels per workgroup halved until the dynamic LDS fits 64 KiB; see
 * mrp_film_mean_fwd_plan below, which reports the geometry a setting gives); kernel choice:
 * "bwd_regular_mfma" (1, default: the matrix-core
 * backward for MRP_GRAPH_REGULAR graphs of 9..16 nodes), "bwd_complete_mfma" (1, default: the
 * matrix-core backward for complete graphs of 9..16 nodes too; those of <= 8 always run the VALU
 * one), "bwd_half_mfma" (1, default: 16-bit features run the matrix-core backward wherever the two
 * knobs before choose it for fp32; 0: film_bwd_dx + the Gram pass, as for shapes the kernel does not
 * take), "bwd_mfma_cpw" (channel blocks per wave of the matrix-core backward, 1 or 2), "bwd_pre2" (0
 * off, 1 on, 2 on unless a grad_x base is given), "fwd_regular_split" (0, default: whole planes).
 * Knobs that name a kernel accept only the kernels the library builds: "edge_split_v"
 * (mrp_edge_encoder_fwd_split: -1, default: per shape; 1 / 3: the hidden layer shared by a workgroup
 * of 4 / 8 waves); "gemm_split" (split-bf16 compress forward / data gradient: -1 per shape (7 where
 * M % 256 == 0, else 2), 2 = 128 rows / 4 waves on 32x32x16 MFMAs, 7 = 256 rows / 8 waves on 16x16x32
 * MFMAs); "split_nt" (split-bf16 weight gradient of mrp_compress_bwd_weight_split and
 * mrp_edge_encoder_bwd_split: -1 per shape, 3 = both operands split in the kernel on 16x16x32 MFMAs,
 * 4 = the compress weight gradient with dy split once (split_rows + gemm_nt_psa; the default where
 * C >= 1024)).  Round 4's other kernel forms are lab code (tools/lab_*.hip) since ABI 18.  Tile order
 * of the split-bf16 GEMMs: "gemm_group" (runs of this many 256-row tiles walked m fastest, so an XCD's
 * concurrent workgroups share row and column blocks in its L2; 4 default, 0 = all, 1..64) for the
 * forward / data gradient, "nt_group" (the same, default 0) for the weight gradient; "enc_bwd_psa"
 * (mrp_edge_encoder_bwd_fused given w2T_packed: 2 default = both products read their A operand
 * pre-split, dz^T written as a packed image; 1 = only W2^T's image; 0 = both split in the kernel);
 * "enc_s1" / "enc_s2" (its two products' split-K counts, 0 = the planner's); "compress_half" (1
 * default; 0 = the bf16 / fp16 compress entry points decline every shape, for A/B runs);
 * "half_nt_splits" (mrp_compress_bwd_weight_t's split-K count, 0 default = the planner's, 1..256);
 * "compress_half_cl" (1 default; 0 = the pixel-major compress entry points mrp_compress_*_cl decline
 * every shape, for A/B runs); "half_cl_splits" (mrp_compress_bwd_weight_cl's split-K count, 0 default =
 * the planner's, 1..256); "compress_split_cl" (1 default; 0 = the pixel-major fp32 entry points
 * mrp_compress_*_split_cl decline every shape) and "split_cl_splits"
 * (mrp_compress_bwd_weight_split_cl's split-K count, 0 default = the planner's, 1..256). */
int mrp_tuning_set(const char* name, int32_t value);

/*
 * The launch plan of the aggregation: what mrp_film_mean_fwd_t / mrp_film_mean_bwd_t would launch for
 * these arguments under the current knobs, computed by the very function the launch path calls and
 * without any GPU call (it works on a machine with no GPU).  tests/test_geometry_cpu.py walks the
 * geometry knobs over their accepted ranges through it and tools/sweep_geometry.py prints it beside
 * every timing.
 *
 * What the planners do beyond the knobs' values (so no accepted setting reaches a kernel outside its
 * requirements):
 *   - lanes per plane are a power of two <= P / vec; channels per workgroup fill at most 256 threads;
 *   - film_bwd_regular reduces a plane's partial sums over one wave: "bwd_regular_lanes" gives at most
 *     64 lanes per plane (1-element slices ask for twice the knob, capped at 64);
 *   - no launcher raises the 64 KiB limit of dynamic LDS: the channels per workgroup are halved until the
 *     kernel's request fits ("bwd_fused_cap" = 64 with logits on planes of 4 slices, and the Gram pass of
 *     complete 16-node graphs with logits at 16 channels, run 32 and 8 channels).  film_bwd_dx, launched
 *     before that Gram pass with the same geometry, runs the 8 channels with it (alone, when no gamma/beta
 *     gradient is wanted, it keeps its 16).
 */
enum mrp_agg_kernel {
  MRP_AGG_KERNEL_NONE = 0,             /* nothing to launch (empty sizes, no gradient wanted) */
  MRP_AGG_KERNEL_FILM_FWD = 1,         /* film_fwd */
  MRP_AGG_KERNEL_FILM_FWD_REGULAR = 2, /* film_fwd_regular (MRP_GRAPH_REGULAR(k), k <= 8) */
  MRP_AGG_KERNEL_FILM_BWD_FUSED = 3,   /* film_bwd_fused, one pass (graphs of <= 8 nodes) */
  MRP_AGG_KERNEL_FILM_BWD_DX_GRAM = 4, /* film_bwd_dx, then film_bwd_fused's 4-row Gram pass (> 8 nodes) */
  MRP_AGG_KERNEL_FILM_BWD_REGULAR = 5, /* film_bwd_regular (fp32, > 8 nodes, MRP_GRAPH_REGULAR(k), k <= 8) */
  MRP_AGG_KERNEL_FILM_BWD_MFMA = 6     /* film_bwd_mfma (9..16 nodes, P % 64 == 0, 4-element slices) */
};

typedef struct mrp_agg_plan {
  int32_t kernel;    /* enum mrp_agg_kernel */
  int32_t vec;       /* slice width in elements */
  int32_t lpc;       /* lanes per channel plane */
  int32_t cpb;       /* channels per workgroup */
  int32_t threads;   /* workgroup size = cpb * lpc (film_bwd_mfma: 256) */
  int32_t psplit;    /* forward: workgroups a plane is cut over (backward: 1) */
  int32_t ncb;       /* channel blocks per graph */
  int32_t pre2;      /* film_bwd_fused: the instantiation that prefetches both of a lane's two slices */
  int64_t grid;      /* workgroups = num_graphs * ncb * psplit */
  int64_t lds_bytes; /* dynamic LDS (MRP_AGG_KERNEL_FILM_BWD_DX_GRAM: the larger of its launches') */
} mrp_agg_plan;

/* The arguments of mrp_film_mean_fwd_t / mrp_film_mean_bwd_t without the stream.  Device pointers are
 * used for their alignment and for being NULL only, never dereferenced (`epilogue` is host memory and is
 * read).  Returns what the launch entry point would return before launching, with *plan filled on
 * success (kernel = MRP_AGG_KERNEL_NONE where the entry point returns success without a launch); a NULL
 * plan returns hipErrorInvalidValue. */
int mrp_film_mean_fwd_plan(int32_t dtype,
                           const void* x, int64_t x_node_stride,
                           const float* gb,
                           const int32_t* indptr, const int32_t* src, const int32_t* eid,
                           const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                           int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                           int32_t C, int32_t P, int32_t mode,
                           void* out, int64_t out_node_stride,
                           const mrp_agg_epilogue* epilogue,
                           mrp_agg_plan* plan);
int mrp_film_mean_bwd_plan(int32_t dtype,
                           const void* grad_out, int64_t g_node_stride,
                           const void* x, int64_t x_node_stride,
                           const float* gb,
                           const int32_t* indptr, const int32_t* src, const int32_t* eid,
                           const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                           int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                           int32_t C, int32_t P, int32_t mode,
                           void* grad_x, int64_t gx_node_stride,
                           const void* grad_x_base, int64_t base_node_stride,
                           float* grad_gb,
                           const mrp_agg_epilogue* epilogue,
                           mrp_agg_plan* plan);

/*
 * FP8 messages: the FiLM-mean forward on feature maps that arrive quantised to 8 bits (what a robot
 * sends over the radio link), read natively and widened exactly in registers.  Added to ABI 22 without a
 * new number (nothing existing changed; every other entry point still rejects these codes).
 *
 *   xq       (num_nodes, C, P) one OCP FP8 code per element: MRP_QDTYPE_E4M3 = torch.float8_e4m3fn (no
 *            infinities, NaN = 0x7f / 0xff, largest finite 448), MRP_QDTYPE_E5M2 = torch.float8_e5m2
 *            (IEEE-like, largest finite 57344).  Never the FNUZ encodings.  x_node_stride counts
 *            elements = bytes.
 *   x_scale  (num_nodes, C) contiguous fp32, one scale per (source node, channel); NULL: all 1.
 *   out      (num_nodes, C, P) of out_dtype (MRP_DTYPE_F32, _BF16 or _F16), node stride in its elements.
 *   the graph arguments, gb and mode (with MRP_AGG_GB_LOGITS) exactly as mrp_film_mean_fwd_t.
 *
 * Every loaded code is decoded exactly (subnormal codes included) and multiplied once by its scale,
 *     x^[u, c, p] = fl32(x_scale[u, c] * decode(xq[u, c, p])),
 * the scale is never folded into gamma, and from there on the arithmetic is the fp32 kernel's, operation
 * for operation, with one round to nearest even at the store: for every graph kind, mode and epilogue
 *     mrp_film_mean_fwd_q(xq, x_scale, out_dtype T) == T(mrp_film_mean_fwd_ex(x^))        bit for bit.
 * Epilogue: out[v] = agg_scale * a + x0_scale * x0[v] with x0 in out_dtype (residual: x0 = the layer's
 * own unquantised features, x0_scale 1; mix: agg_scale 1 - alpha, x0 = h0, x0_scale alpha).  A robot's own
 * features never cross the link, so the own-feature terms cannot come from xq: self_scale != 0 or a
 * non-NULL xcopy returns hipErrorInvalidValue.
 * Special values: the E4M3 NaN codes and the E5M2 inf / NaN codes propagate like any fp32 NaN / inf — to
 * the destinations that have that source as an in-neighbour, at that channel and pixel, and to no other
 * element; FP8 subnormal codes are decoded exactly; a non-finite scale acts on its (node, channel) alone.
 * Slices are 8 elements (graphs of <= 8 nodes, 16-bit outputs), 4, or 1: the widest for which xq (1-byte
 * elements) and out / x0 (2- or 4-byte elements) are both aligned and P and every node stride are
 * multiples of it.  fp32 outputs use 4 or 1 (16-byte stores, the fp32 kernel's width).
 * Span: as the typed entry point — node offsets are 64-bit, so xq and out may each span any number of
 * GiB (tests/test_gpu_fp8_messages.py places node blocks more than 2^32 bytes apart); the byte offsets
 * within one workgroup's channel block are 32-bit.  No span is declined.
 * Return codes, all before any launch: hipErrorInvalidValue for an unknown qdtype or out_dtype, a NULL
 * pointer with work to do, a node stride < C * P, max_nodes > MRP_MAX_NODES, an unknown graph kind or
 * mode flags, self_scale != 0 or xcopy != NULL.  Zero sizes succeed without a launch.  No host
 * synchronisation; stream-capturable.  mrp_film_mean_fwd_q_plan: the same arguments without the stream,
 * host only (no GPU call), reporting the plan the launcher acts on (as mrp_film_mean_fwd_plan).
 * Not provided: pixel-major FP8 inputs, FP8 outputs, a backward that reads FP8.  (The max and attention
 * reducers on FP8: mrp_film_max_fwd_q / mrp_film_attn_fwd_q / mrp_film_wattn_fwd_q below.)
 */
enum mrp_qdtype { MRP_QDTYPE_E4M3 = 0, MRP_QDTYPE_E5M2 = 1 };

int mrp_film_mean_fwd_q(int32_t qdtype,
                        const void* xq, int64_t x_node_stride,
                        const float* x_scale,
                        int32_t out_dtype,
                        const float* gb,
                        const int32_t* indptr, const int32_t* src, const int32_t* eid,
                        const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                        int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                        int32_t C, int32_t P, int32_t mode,
                        void* out, int64_t out_node_stride,
                        const mrp_agg_epilogue* epilogue,
                        void* stream);
int mrp_film_mean_fwd_q_plan(int32_t qdtype,
                             const void* xq, int64_t x_node_stride,
                             const float* x_scale,
                             int32_t out_dtype,
                             const float* gb,
                             const int32_t* indptr, const int32_t* src, const int32_t* eid,
                             const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                             int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                             int32_t C, int32_t P, int32_t mode,
                             void* out, int64_t out_node_stride,
                             const mrp_agg_epilogue* epilogue,
                             mrp_agg_plan* plan);

/*
 * FP8 messages for the max and attention reducers, receiver side.  Added to ABI 22 without a new number
 * (nothing existing changed).  A receiver holds its own features at full precision and is handed its
 * neighbours' feature maps as FP8 codes with scales (and, for the gated fusion, their confidence maps):
 *
 *   xq, xq_node_stride, x_scale, qdtype   the messages, exactly as mrp_film_mean_fwd_q's xq / x_scale:
 *            x^[u, c, p] = fl32(x_scale[u, c] * decode(xq[u, c, p])), x_scale (num_nodes, C) contiguous or
 *            NULL (all 1), strides in elements = bytes.
 *   query, query_node_stride, dtype       (attention only) the own features (num_nodes, C, P) of `dtype`
 *            (MRP_DTYPE_F32, _BF16 or _F16), which is also the type of out.  A robot's own maps never
 *            cross the link: x[v] scores the messages, x^[u] forms them, and the two are separate tensors.
 *   out_dtype                             (max only: it has no query) the type of out.
 *
 *   mrp_film_max_fwd_q    out[v, c, p] = max_j fl(fl(gamma_j[c] x^[u_j, c, p]) + beta_j[c]); everything else
 *                         as mrp_film_max_fwd.  == out_dtype(mrp_film_max_fwd(fp32 x^)) bit for bit.
 *   mrp_film_attn_fwd_q   mrp_film_attn_fwd_mh with the messages formed from x^ and the scores from
 *                         `query`: s_j[p] = scale * sum_c query[v, c, p] * m_j[c, p].  Everything else —
 *                         gb, the graph, flags, heads, scale, attn (heads, E, P), the workspace arguments
 *                         (the forward needs none) — as mrp_film_attn_fwd_mh; heads = 1 runs the
 *                         single-head kernels.  With query = x^ in fp32 the result is mrp_film_attn_fwd_mh(x^)'s
 *                         bit for bit, out and attn; a 16-bit query is widened exactly and out is rounded
 *                         once at the store, so T(query) gives T(the fp32 call on float(query)) with the same
 *                         attn.
 *   mrp_film_wattn_fwd_q  the same for mrp_film_wattn_fwd_mh: w, w_node_stride and rate as there.
 *   Under heads > 1, head k reads channels [k C / heads, (k + 1) C / heads) of xq, query and of x_scale's
 *   rows: its bits are those of a single-head call on the slices.
 *
 * Special values: as mrp_film_mean_fwd_q — an E4M3 NaN code or an E5M2 inf / NaN code is a NaN / inf message
 * element, and reaches what an fp32 NaN / inf at that place reaches in mrp_film_max_fwd / mrp_film_attn_fwd_mh
 * / mrp_film_wattn_fwd_mh: in the attention forms the outputs (all channels of that head) of the destinations
 * that consume that source at that pixel, no other head and no other pixel; a sender that is silent at a pixel
 * (w <= 0) is never read there, whatever its codes.
 * Return codes, all before any launch: hipErrorInvalidValue for an unknown qdtype, dtype or out_dtype; a NULL
 * xq, query, out (or gb / attn with num_edges > 0, or w) with work to do; a node stride < C * P (w: < P);
 * max_nodes > MRP_MAX_NODES or a REGULAR in-degree > 16 (CSR / SIMPLE rows longer than 16 are the
 * caller's to reject, as for mrp_film_attn_fwd); heads < 1 or not dividing C; an unknown graph kind or flags
 * other than 0 / MRP_AGG_GB_LOGITS; a non-finite scale; workspace_bytes < 0.  Zero sizes succeed without a
 * launch (attn and rate, where passed, are zeroed as in mrp_film_attn_fwd_mh).  No host synchronisation;
 * stream-capturable.  All offsets are 64-bit.
 * Not provided: a backward (training through FP8 attention needs the query / source split in the backward
 * kernels too), FP8 with mrp_film_wmean_fwd, pixel-major FP8, FP8 outputs, block scales.
 */
int mrp_film_max_fwd_q(int32_t qdtype,
                       const void* xq, int64_t xq_node_stride,
                       const float* x_scale,
                       int32_t out_dtype,
                       const float* gb,
                       const int32_t* indptr, const int32_t* src, const int32_t* eid,
                       const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                       int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                       int32_t C, int32_t P, int32_t flags,
                       void* out, int64_t out_node_stride,
                       void* stream);
int mrp_film_attn_fwd_q(int32_t qdtype,
                        const void* xq, int64_t xq_node_stride,
                        const float* x_scale,
                        int32_t dtype,
                        const void* query, int64_t query_node_stride,
                        const float* gb,
                        const int32_t* indptr, const int32_t* src, const int32_t* eid,
                        const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                        int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                        int32_t C, int32_t P, int32_t flags, int32_t heads,
                        void* out, int64_t out_node_stride,
                        float scale, float* attn,
                        void* workspace, int64_t workspace_bytes,
                        void* stream);
int mrp_film_wattn_fwd_q(int32_t qdtype,
                         const void* xq, int64_t xq_node_stride,
                         const float* x_scale,
                         int32_t dtype,
                         const void* query, int64_t query_node_stride,
                         const float* gb,
                         const float* w, int64_t w_node_stride,
                         const int32_t* indptr, const int32_t* src, const int32_t* eid,
                         const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                         int32_t graph_kind, int32_t num_nodes, int32_t num_edges,
                         int32_t C, int32_t P, int32_t flags, int32_t heads,
                         void* out, int64_t out_node_stride,
                         float scale, float* attn, float* rate,
                         void* workspace, int64_t workspace_bytes,
                         void* stream);

/* Library identification: ABI version (incremented on signature changes; 22 = this header: v21 plus
 * the typed aggregation entry points mrp_film_mean_fwd_t / mrp_film_mean_bwd_t (bf16 and fp16 feature
 * tensors, enum mrp_dtype) and, added since without a new number (nothing existing changed), the
 * typed compress entry points mrp_compress_pack_t_bytes / _pack_t / _fwd_t / _bwd_data_t /
 * _bwd_weight_t_workspace / _bwd_weight_t and the knobs "compress_half" / "half_nt_splits", and their
 * pixel-major forms mrp_compress_fwd_cl / _bwd_data_cl / _bwd_weight_cl_workspace / _bwd_weight_cl with the
 * knobs "compress_half_cl" / "half_cl_splits", and the part-count forms of the split-bf16 compress
 * mrp_compress_fwd_split_p / _bwd_data_split_p / _bwd_weight_split_p, and their pixel-major fp32 forms
 * mrp_compress_fwd_split_cl / _bwd_data_split_cl / _bwd_weight_split_cl_workspace / _bwd_weight_split_cl
 * with the knobs "compress_split_cl" / "split_cl_splits", and the host-only plan queries
 * mrp_film_mean_fwd_plan / mrp_film_mean_bwd_plan (enum mrp_agg_kernel, mrp_agg_plan), and the FP8-message
 * forwards mrp_film_mean_fwd_q / _q_plan, mrp_film_max_fwd_q, mrp_film_attn_fwd_q, mrp_film_wattn_fwd_q; 21: v19 plus
 * the streaming yardstick mrp_stream_copy, the device-scope stream join mrp_stream_join and the encoder's pose gradient (mrp_edge_encoder_bwd_pose
 * + workspace); 20: v19 plus a one-launch no-grad GCN layer
 * (mrp_gcn_fwd_fused), measured slower than the two launches it replaced and removed in 21
 * (tools/lab_patches/r06_fused_layer.patch); 19: v18 with
 * mrp_edge_encoder_bwd_fused taking W2^T's packed image (w2T_packed); 18: v17 without
 * mrp_edge_encoder_fwd (the fp32 one-launch encoder, superseded by mrp_edge_encoder_fwd_split) and
 * with fewer tuning knobs (only those that select kernels the library builds); 17: v16 plus
 * the split-bf16 training path of the edge encoder (mrp_edge_encoder_fwd_split_train, _bwd_prep,
 * _bwd_split, _bwd_t and their workspaces); 16: v15 plus
 * the split-bf16 weight gradient (mrp_compress_bwd_weight_split + workspace); 15: v14 plus
 * the split-bf16 compress forward / data gradient and their weight packing (mrp_compress_split_*,
 * mrp_compress_fwd_split, mrp_compress_bwd_data_split); 14: v13 plus
 * the split-bf16 edge encoder forward and its weight packing (mrp_edge_encoder_pack_bytes /
 * _pack / _fwd_split); 13: the
 * aggregation and epilogue entry points of v10, the matrix-core compress forward and gradients,
 * mrp_compress_fwd / _bwd_data / _bwd_weight of v12 (v11's forward-only fused and two-source
 * compress kernels, their weight packing and mrp_film_gate are gone), and the edge encoder's
 * second Linear and whole forward, mrp_edge_logits_fwd / mrp_edge_encoder_fwd). */
int mrp_abi_version(void);

/* The streaming yardstick the benchmark reports beside every aggregation roofline (ceiling_frac):
 * dst = src over `bytes` (a multiple of 16; 16-byte aligned pointers) as one nontemporal 16-byte load
 * and store per thread — the 1-read-1-write copy the HBM-bound kernels are measured against on the
 * same box in the same run.  Not part of the GCN path. */
int mrp_stream_copy(const void* src, void* dst, int64_t bytes, void* stream);

/* Stream join: work enqueued on `waiter` after this call waits for everything enqueued on `signaller`
 * before it — an event recorded with a device-scope release (no system-scope cache writeback: the
 * joined work is on the same device) that `waiter` waits on.  The inference encoder's stream joins the
 * caller's stream with it (encoder.py).  Returns a hipError_t. */
int mrp_stream_join(void* waiter, void* signaller);

/* Human-readable text for a return code (static storage). */
const char* mrp_error_string(int code);

#ifdef __cplusplus
}
#endif

#endif /* MRP_GNN_H */
