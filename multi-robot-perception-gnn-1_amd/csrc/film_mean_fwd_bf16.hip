// film_mean_fwd_bf16.hip — the forward's bf16 instantiations (mrp_film_mean_fwd_t), a translation unit of
// their own so they compile beside the fp32 ones (film_mean_fwd.hip).
#include "film_mean_fwd_launch.hpp"

namespace mrp_host {

int film_fwd_bf16(const void* x, int64_t x_node_stride, const float* gb, const int32_t* indptr, const int32_t* src,
                  const int32_t* eid, const int32_t* graph_off, int32_t num_graphs, int32_t max_nodes,
                  int32_t graph_kind, int32_t num_nodes, int32_t num_edges, int32_t C, int32_t P, int32_t mode_flags,
                  void* out, int64_t out_node_stride, const mrp_agg_epilogue* ep, void* stream) {
  return film_fwd_impl<mrp::bf16_t>(static_cast<const mrp::bf16_t*>(x), x_node_stride, gb, indptr, src, eid, graph_off,
                            num_graphs, max_nodes, graph_kind, num_nodes, num_edges, C, P, mode_flags,
                            static_cast<mrp::bf16_t*>(out), out_node_stride, ep, stream);
}

}  // namespace mrp_host
