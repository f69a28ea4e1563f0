// Internal (non-ABI) declarations: the views of the caller's buffers, dims, launch helpers.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/cgr_mpnn3d.h"
#include "layout.hpp"

namespace cgr {

void set_error(const std::string& msg);

#define HIP_RET(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      ::cgr::set_error(std::string("HIP error ") + hipGetErrorString(_e) + " at " + __FILE__ + \
                       ":" + std::to_string(__LINE__));                                       \
      return CGR_ERR_HIP;                                                                     \
    }                                                                                         \
  } while (0)

#define CGR_CHECK(cond, msg)           \
  do {                                 \
    if (!(cond)) {                     \
      ::cgr::set_error(msg);           \
      return CGR_ERR_INVALID_ARGUMENT; \
    }                                  \
  } while (0)

// Every launching entry point starts with this: hipGetLastError() is per thread and sticky, so an
// error left by an unrelated earlier HIP call (e.g. a caller's aborted stream capture) would
// otherwise be reported by our first post-launch check as if our launch had failed.
inline void clear_stale_hip_error() { (void)hipGetLastError(); }

// Views of the caller's buffers: every member is a region (layout.hpp), stated once in its
// layout function (capi.hip) and read here as the typed pointer it converts to.
// Index bookkeeping inside the arena (all int32).
struct IndexView {
  // zero block (zeroed each forward: a rider of the pack launch, or a memset with caller images):
  // deg_dst, deg_src, cursor, cursor2, graph_cnt, status, fcnt
  Reg<int> deg_dst, deg_src, cursor, cursor2, graph_cnt, status;
  Reg<int> fcnt;  // [N * column tiles] hub-segment tickets of the layer GEMMs (in the zero block)
  Reg<void> zero_block;
  Reg<uint64_t> rng;  // effective dropout key of this forward (read by every dropout kernel)
  Reg<int> perm, src_s, dst_s, rev_s, src_list, inv, src_c, dst_c, dst_ptr, src_ptr, graph_ptr,
      node_graph;
};

// split-bf16 weight images (gemm_b3.hpp), packed once per step by the forward or, the forward
// ones, by cgr_gnn_pack_images into a buffer of the caller's
struct Images {
  Reg<void> b3x;                  // [W0[:, :F]; W_n[:, :F]]   (x-GEMM; F > 0)
  Reg<void> b3rof;                // W_n[:, F:]                 (readout forward)
  Reg<void> b3rob;                // W_n[:, F:]^T diag(wf)      (readout backward)
  Reg<void> b3lf[CGR_MAX_DEPTH];  // W_l                        (layer forward)
  Reg<void> b3lb[CGR_MAX_DEPTH];  // W_l^T                      (layer backward)
};

// Forward-saved float state inside the arena.
struct FloatView : Images {
  Reg<float> fpart;  // [tiles, 2, BN] hub-segment partial sums of the layer GEMMs
  Reg<float> e_s;    // [E, Fep] sorted, zero padded edge_attr (Fe > 0)
  Reg<float> w0eT;   // [Fe, Hp] transposed edge-feature slice of edge_init.weight (Fe > 0)
  Reg<float> P;      // [N, Hp]  x @ W0[:, :F]^T (node-level half of edge init)
  Reg<float> Q;      // [N, Hp]  x @ W_n[:, :F]^T (x-part of the readout, beside graph prep)
  Reg<float> xp;     // [N, Fp]  x with rows padded to 4 floats (only when F % 4 != 0)
  Reg<float> h[CGR_MAX_DEPTH + 1];    // [E, Hp] h_0 .. h_D
  Reg<float> a[CGR_MAX_DEPTH + 1];    // [N, Hp] a_l = scatter_add(h_l, dst); a_D = readout s
  Reg<float> pre[CGR_MAX_DEPTH + 1];  // [E, Hp] pre-activations (non-ReLU only)
  Reg<float> zn;                      // [N, Hp] readout pre-activation (non-ReLU only)
  Reg<float> hn;                      // [N, Hp] readout activation
  Reg<float> g;                       // [B, Hp] pooled graph embeddings
  Reg<float> inv_deg;  // [N] 1 / max(in-degree, 1)   (mean aggregation only)
  Reg<float> inv_cnt;  // [B] 1 / max(graph nodes, 1) (mean pooling only)
  Reg<int> pool_arg;   // [B, Hp] max pooling's first arg-max node per column, -1: empty graph
};
struct ArenaView {
  IndexView idx;
  FloatView flt;
};

struct Dims {
  int64_t N, E, B;
  int F, Fe, Fep, Fp, H, Hp, D;  // Fp = round_up(F, 4)
  int act;
  int learnable_skip;
  int aggr, pool;  // enum cgr_aggregation / cgr_pooling
  // enum cgr_precision.  Every layout function and every launch decision reads the mode from
  // here and nowhere else: the NT GEMMs' variant and column tilings (nt_acc: x_cols,
  // readout_cols, layer_cols, image_cols) and the weight gradients' families (wgrad_candidates)
  int precision;
  bool nt_acc() const { return precision == CGR_PRECISION_FP32; }  // per-k-step accumulation
};

// Backward workspace.  dpre has one buffer per layer (no side->main wait before a buffer is
// rewritten; the edge-init backward sums dh0 from all of them); dm holds only the rows the fused
// layer-backward GEMM hands to the completer of a tile-crossing segment (ep_bwd.hpp).
struct WorkspaceView {
  Reg<float> dpre;  // D x [E, Hp], layer l at l * E * Hp
  Reg<float> dm, dh0, dzn, ds, Gs;
  // split-bf16 e-images (gemm_b3tn.hpp B3EImg) of the weight gradients' shared operand: dpre_l and
  // dzn on the side stream (one at a time), Gs on the caller's stream; the top layer's dpre,
  // written by its activation kernel on the caller's stream (img_top)
  Reg<void> img_side, img_main, img_top;
  // split-K slabs and bias slabs; count is the floats each holds: the backward checks the plan it
  // picked against it before every weight-gradient launch.  slab[2]: the side stream's
  // alternating pair (reductions folded into TNs); slab2: the node site's, on the caller's stream
  Reg<float> slab[2], bslab[2], slab2, bslab2;
  // 2 x [N, Hp] partial da sums of the dst segments that cross a row tile of the fused
  // layer-backward GEMM (ep_bwd.hpp), alternating by layer
  Reg<float> dag;
  // [N * column tiles] ticket counters of those segments, then one unpaired grid counter per
  // fused layer-backward launch
  Reg<int> cnt;
  // [row tiles * column tiles, 2, BN] partial sums of the segments over >= 3 row tiles
  Reg<float> part;
  // [F, input_grad_ldw(H)] the stacked, transposed x slices of edge_init / edge_to_node weights
  // (cgr_gnn_input_grads only)
  Reg<float> wxT;
  Reg<float> dsig_part;  // [D, bwd_dsig_slots] learnable-skip partial sums
};
inline int input_grad_ldw(int H) { return (2 * H + 3) & ~3; }
int bwd_dsig_slots(const Dims& d);
int bwd_seg_tiles(const Dims& d);
struct B3Cols;
// Column tilings of the NT GEMMs in d's precision mode (capi.hip): images are packed, sized and
// launched in these.  layer: the layer GEMMs, forward and fused backward; x: the x-GEMM's
// [P | Q]; readout: the node-row readout GEMMs, forward and backward; image: the
// batch-independent tiling of caller-packed images (cgr_gnn_pack_images) over n columns.
B3Cols layer_cols(const Dims& d);
B3Cols x_cols(const Dims& d);
B3Cols readout_cols(const Dims& d);
B3Cols image_cols(const Dims& d, int n);

// Forward variants.  Training (cgr_gnn_forward): every activation the backward reads is saved in
// the arena and the weight images are packed into it by each call.  Eval (cgr_gnn_predict): no
// saved activations -- h_1.. h_D alias a two-buffer ring and a_0 .. a_D a three-buffer ring (the
// fused layer epilogue zeroes the entries it accumulates two layers ahead, gnn_fwd.hip) -- and
// the forward weight images are packed into its arena by every call (the weights may have changed
// by any route: an optimizer writing through raw pointers, a replayed captured step), unless the
// caller hands pre-packed ones (cgr_gnn_pack_images) and vouches for their freshness.
// What a forward hands its caller, and so what cotangent its backward takes.  Fused
// (cgr_gnn_forward / _predict): y [B], the whole model.  Pooled (cgr_gnn_encode / _encode_predict,
// "headless"): the forward ends in the pool without the ffn head; its `y` argument is the caller's
// g_out [B, H].  Nodes (cgr_gnn_encode_nodes / _encode_nodes_predict): it ends after the readout
// GEMM; `y` is the caller's n_out [N, H], a copy of hn, and nothing of the pooling state (pool_arg,
// inv_cnt, g) is read or written, whatever d.pool says.  Below Fused there is no wf, so the
// readout-backward image is packed unscaled for every pooling mode and the backward reads a dzn
// materialised from the caller's dg [B, H] / dn [N, H].
enum class OutLevel : int { Fused = 0, Pooled = 1, Nodes = 2 };
struct FwdMode {
  bool eval = false;
  const void* images = nullptr;
  OutLevel level = OutLevel::Fused;
};
Dims make_dims(const cgr_gnn_config* cfg, int64_t N, int64_t E, int64_t B);
// The views over a buffer, one call each (capi.hip).  arena_view: the training arena's, or the
// eval (predict) arena's; image_view: a caller-packed image buffer's (only the forward images are
// present).
ArenaView arena_view(const Dims& d, bool eval, void* arena);
WorkspaceView workspace_view(const Dims& d, void* workspace);
Images image_view(const Dims& d, void* images);

// dropout threshold and scale of layer l (gnn_fwd.hip; oracle/dropout.py models it)
void dropout_consts(const float* dropout_p, int training, int l, uint32_t* thresh, float* scale);

struct PrepArgs {
  const int64_t* edge_index;
  const int64_t* batch;      // may be null (one graph)
  const int64_t* graph_ptr;  // may be null (derive from batch)
  const float* edge_attr;
  int64_t N, E, B;
  int64_t Fe, Fep;
  IndexView idx;
  float* e_s;
  // dropout key (folded into the first prep kernel): written to idx.rng when want_key
  bool want_key = false;
  uint64_t seed = 0;
  uint64_t* rng_counter = nullptr;
  // idx.zero_block already zeroed on this stream (a pack launch's rider, gnn_fwd.hip)
  bool zeroed = false;
};

}  // namespace cgr

int cgr_graph_prep_impl(const cgr::PrepArgs& a, hipStream_t st);
