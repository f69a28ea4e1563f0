/*
 * cgr_mpnn3d.h - C ABI of the MI355X-native CGR-MPNN-3D D-MPNN hot path (libcgr_mpnn3d.so).
 *
 * The reference (tobjec/CGR-MPNN-3D @ 2025-02-27) is pure Python; its hot path is the
 * ``GNN`` / ``DMPNNConv`` pair in ``cgr_mpnn_3D/models/GNN.py`` plus two PyTorch-Geometric
 * sum-scatters.  Each entry point below replaces one of those interfaces (file:line cited) and is
 * bound from Python by ``cgr_mpnn_3D/_amd/native.py`` (ctypes), which keeps the reference's
 * ``nn.Module`` surface so ``train.py`` / ``test.py`` drop in unchanged.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer argument named d_* / listed as "device" is
 *     device memory on the current HIP device; `stream` is a hipStream_t passed as void*
 *     (NULL = legacy default stream).  Calls only enqueue work: no allocation, no host sync, so
 *     they can be captured into a hipGraph.
 *   - fp32 data, row-major; int64 graph indices exactly as PyG produces them.
 *   - parameters / gradients are passed as a table of device pointers in the reference
 *     ``state_dict`` order (see CGR_PARAM_*), each tensor contiguous in the reference layout
 *     (nn.Linear weight = [out, in]).
 *   - return 0 on success, a CGR_ERR_* code otherwise; cgr_last_error() describes the failure
 *     (thread-local).  Python raises RuntimeError with that text.
 */
#ifndef CGR_MPNN3D_H
#define CGR_MPNN3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 9.  The headless entry points (cgr_gnn_encode, _encode_backward, _encode_input_grads,
 * _encode_predict) and the nodes-level ones (cgr_gnn_encode_nodes, _encode_nodes_backward,
 * _encode_nodes_input_grads, _encode_nodes_predict) were added within ABI 9: they change no
 * existing signature, struct or behaviour, so a binding written against the earlier ABI 9 keeps
 * working. */
#define CGR_ABI_VERSION 9
#define CGR_MAX_DEPTH 32

enum cgr_status {
  CGR_OK = 0,
  CGR_ERR_INVALID_ARGUMENT = 1,
  CGR_ERR_HIP = 2,
  CGR_ERR_UNSUPPORTED = 3,
};

/* activation_fn of GNN.__init__ (GNN.py:21, applied at GNN.py:86,127: any callable); train.py:284-292
 * offers F.relu / F.silu / F.gelu.  Codes 3-9 are further elementwise activations at torch's
 * default parameters (ELU alpha 1, leaky_relu slope 0.01, softplus beta 1 / threshold 20). */
enum cgr_activation {
  CGR_ACT_RELU = 0, CGR_ACT_SILU = 1, CGR_ACT_GELU = 2, CGR_ACT_TANH = 3, CGR_ACT_SIGMOID = 4,
  CGR_ACT_ELU = 5, CGR_ACT_LEAKY_RELU = 6, CGR_ACT_SOFTPLUS = 7, CGR_ACT_MISH = 8, CGR_ACT_SELU = 9
};

/* GNN.__init__(num_node_features, num_edge_features, depth, hidden_sizes, dropout_ps,
 *              activation_fn, aggr="add", pooling_fn=global_add_pool, use_learnable_skip)
 * (GNN.py:14-74).  The math of the reference requires one uniform hidden size (GNN.py:53-65). */
typedef struct cgr_gnn_config {
  int32_t num_node_features; /* F  (78 CGR + 768 MACE for CGR-MPNN-3D) */
  int32_t num_edge_features; /* Fe (14), may be 0 */
  int32_t hidden;            /* H  = hidden_sizes[i] for all i */
  int32_t depth;             /* D  (1 .. CGR_MAX_DEPTH) */
  int32_t activation;        /* enum cgr_activation */
  int32_t learnable_skip;    /* use_learnable_skip (GNN.py:71-74, :94-97) */
  int32_t aggregation;       /* enum cgr_aggregation: DMPNNConv(aggr=...) (GNN.py:22,63,119) */
  int32_t pooling;           /* enum cgr_pooling: pooling_fn (GNN.py:23,110) */
  int32_t precision;         /* enum cgr_precision (ABI 9; no reference counterpart) */
} cgr_gnn_config;

/* Arithmetic of the GNN kernels.  CGR_PRECISION_SPLIT (the default): the split-bf16 NT GEMMs add
 * every piece product into the matrix core's running sum, and widths up to 512 take their weight
 * gradients from two-piece split-bf16 operands -- predictions within the reference's fp32 at 1e-4,
 * some gradients outside it.  CGR_PRECISION_FP32: every 32-deep k step of an
 * NT GEMM is summed on its own and folded into the running sum with one fp32 add, and every weight
 * and bias gradient comes from fp32 rows on an fp32 TN kernel -- fp32-class against float64 at
 * every stage, slower.  The mode is part of the config: sizes, offsets, the
 * image layout of cgr_gnn_pack_images and every launch follow it, and cgr_gnn_backward /
 * cgr_gnn_input_grads refuse a config whose mode differs from the one `arena`'s forward ran in. */
enum cgr_precision { CGR_PRECISION_SPLIT = 0, CGR_PRECISION_FP32 = 1 };

/* aggr of GNN.__init__ / DMPNNConv (PyG MessagePassing): "add" (= "sum", the default) or "mean"
 * (the sum over a node's in-edges divided by their count, 0 for a node without in-edges) */
enum cgr_aggregation { CGR_AGGR_ADD = 0, CGR_AGGR_MEAN = 1 };
/* pooling_fn: global_add_pool (default), global_mean_pool (the graph's node sum divided by its
 * node count) or global_max_pool (per column the largest node value; with a `batch` its gradient
 * is shared evenly by the nodes holding it, as torch's scatter_reduce("amax", include_self=False)
 * backward does -- the zero `self` counted when the max is 0; with batch == NULL, x.max(dim=-2),
 * it goes to the first node holding it) */
enum cgr_pooling { CGR_POOL_ADD = 0, CGR_POOL_MEAN = 1, CGR_POOL_MAX = 2 };

/* One collated batch, the fields GNN.forward reads from a PyG Batch (GNN.py:77-82). */
typedef struct cgr_batch {
  const float* x;            /* device [N, F]  data.x */
  const int64_t* edge_index; /* device [2, E]  data.edge_index (row 0 = src, row 1 = dst) */
  const float* edge_attr;    /* device [E, Fe] data.edge_attr (NULL allowed when Fe == 0) */
  const int64_t* batch;      /* device [N]     data.batch, sorted graph id per node; NULL = one
                                graph (global_add_pool(h, None), GNN.py:110) */
  const int64_t* graph_ptr;  /* device [B+1]   Batch.ptr node offsets, or NULL (derived from
                                `batch` on the device) */
  int64_t num_nodes;         /* N */
  int64_t num_edges;         /* E (even: reverse edge of e is e ^ 1, GNN.py:136-138) */
  int64_t num_graphs;        /* B (1 when batch == NULL) */
} cgr_batch;

/* Parameter table order = reference state_dict order (GNN.py:53-74):
 *   [0] edge_init.weight [H, F+Fe]   [1] edge_init.bias [H]
 *   [2+2l] convs.l.lin.weight [H, H] [3+2l] convs.l.lin.bias [H]          l = 0..D-1
 *   [2+2D] edge_to_node.weight [H, F+H]  [3+2D] edge_to_node.bias [H]
 *   [4+2D] ffn.weight [1, H]         [5+2D] ffn.bias [1]
 *   [6+2D+l] skip_weights.l []       (only when learnable_skip)                              */
#define CGR_PARAM_EDGE_INIT_W 0
#define CGR_PARAM_EDGE_INIT_B 1
#define CGR_PARAM_CONV_W(l) (2 + 2 * (l))
#define CGR_PARAM_CONV_B(l) (3 + 2 * (l))
#define CGR_PARAM_E2N_W(D) (2 + 2 * (D))
#define CGR_PARAM_E2N_B(D) (3 + 2 * (D))
#define CGR_PARAM_FFN_W(D) (4 + 2 * (D))
#define CGR_PARAM_FFN_B(D) (5 + 2 * (D))
#define CGR_PARAM_SKIP(D, l) (6 + 2 * (D) + (l))

int cgr_abi_version(void);
const char* cgr_last_error(void);

/* number of entries of the parameter / gradient tables for `cfg` */
int cgr_gnn_num_params(const cgr_gnn_config* cfg);

/* Bytes of the per-forward arena (index bookkeeping + activations saved for backward) and of the
 * backward scratch workspace.  The caller owns both (e.g. torch.empty(uint8) on the device).
 *
 * The contract of every caller-owned buffer of the GNN entry points -- this arena and workspace,
 * the predict arena (cgr_gnn_predict_arena_bytes), the images of cgr_gnn_pack_images
 * (cgr_gnn_image_bytes), the gradient table's tensors, dx / dedge_attr and the outputs:
 *   - its contents on entry are arbitrary (another batch's arena, NaNs, anything): no result
 *     depends on them, the library writes whatever it later reads;
 *   - nothing outside the reported bytes (the size queries; the shapes of the outputs) is written;
 *   - the pad columns of the saved buffers (columns hidden .. Hp - 1 of the rows behind
 *     cgr_gnn_arena_offset / cgr_gnn_workspace_offset) are unspecified unless a buffer's
 *     description says otherwise; the bytes between a named region's end and the next region's
 *     256-byte-aligned start are left as they were.
 * tests/test_gpu_arena_contract.py holds every entry point to it. */
int64_t cgr_gnn_arena_bytes(const cgr_gnn_config* cfg, int64_t num_nodes, int64_t num_edges,
                            int64_t num_graphs);
int64_t cgr_gnn_workspace_bytes(const cgr_gnn_config* cfg, int64_t num_nodes, int64_t num_edges,
                                int64_t num_graphs);

/* Byte offset of a named arena buffer (introspection for tests/debugging).  "status" is the graph
 * prep's int32 status word: bit 0 an edge id outside [0, num_nodes), bit 1 an unsorted or
 * out-of-range batch vector, bit 2 edges not reverse-paired (src(e ^ 1) != dst(e) for some e;
 * informational: results stay exact, the backward takes its unpaired form), bit 4 (value 16) the
 * unpaired backward's completion timed out (see cgr_device_errors).  Names: "status", "rng",
 * "perm", "src_s", "dst_s", "rev_s", "src_list", "dst_ptr", "src_ptr", "graph_ptr",
 * "node_graph", "e_s", "P", "h", "a", "pre", "zn", "hn", "g"; `index` selects the layer for
 * "h" / "a" / "pre".  Returns -1 for an unknown or absent buffer. */
int64_t cgr_gnn_arena_offset(const cgr_gnn_config* cfg, int64_t num_nodes, int64_t num_edges,
                             int64_t num_graphs, const char* name, int32_t index);

/* Byte offset of a named backward-workspace buffer (introspection for tests/debugging; ABI 7).
 * Valid after cgr_gnn_backward has returned and its stream has been synchronised.  All buffers are
 * fp32 in sorted edge order (rows of "dpre" / "dpre0") or node order ("ds"), leading dimension
 * Hp = round_up(hidden, 4).  Names: "dpre" with `index` = conv layer l (0 .. depth-1): the
 * gradient at layer l's pre-activation; "dpre0": the gradient at the edge init's pre-activation
 * (written in place of the skip sum dh0); "ds": the gradient at the readout aggregate a_D,
 * already divided by the in-degree under mean aggregation (what the top layer gathers at dst);
 * "dzn_main": the gradient at the readout's pre-activation, node order, pad columns 0 -- valid
 * only where the backward materialises it in fp32 for the readout GEMM: after
 * cgr_gnn_encode_backward or cgr_gnn_encode_nodes_backward, and under max pooling.
 * Returns -1 for any other name: buffers that not every dispatch path materialises in fp32
 * ("dzn" as such, Gs, dm) are not exposed. */
int64_t cgr_gnn_workspace_offset(const cgr_gnn_config* cfg, int64_t num_nodes, int64_t num_edges,
                                 int64_t num_graphs, const char* name, int32_t index);

/* Index bookkeeping only (also run by cgr_gnn_forward): stable dst-sorted edge order, reverse
 * edge map, src/dst CSR, graph node ranges.  Replaces the implicit index handling of
 * GNN.py:85,132-138 and PyG's scatter/pool indexing (GNN.py:110,134). */
int cgr_graph_prep(const cgr_gnn_config* cfg, const cgr_batch* batch, void* arena, void* stream);

/* GNN.forward(data) -> [B] (GNN.py:76-110): edge init, `depth` fused D-MPNN layers
 * (gather -> MFMA GEMM -> bias/skip/act/dropout epilogue -> segmented reduce), edge->node
 * readout, add-pool and ffn.  Dropout (GNN.py:100-102) is applied when `training` != 0 and
 * dropout_p[l] > 0, from a counter-based RNG keyed by `seed` and, when `rng_counter` (device
 * uint64, may be NULL) is given, by its value, which the forward then increments on the device:
 * a captured graph replays with a fresh mask each time (the key is kept in the arena for the
 * backward).  Fills `arena` with what cgr_gnn_backward needs.  `y` device [B].
 * `training` is a bit set (other bits are rejected): CGR_TRAIN_DROPOUT = train-mode dropout
 * (module.training); CGR_TRAIN_FOR_BACKWARD = a backward will follow (the forward then also packs
 * the backward GEMMs' weight images into the arena; cgr_gnn_backward refuses an arena whose
 * forward did not set it).  Pass the same value to cgr_gnn_backward. */
#define CGR_TRAIN_DROPOUT 1
#define CGR_TRAIN_FOR_BACKWARD 2
int cgr_gnn_forward(const cgr_gnn_config* cfg, const float* const* params,
                    const cgr_batch* batch, const float* dropout_p, uint64_t seed,
                    uint64_t* rng_counter, int32_t training, void* arena, float* y,
                    void* stream);

/* Reverse mode of cgr_gnn_forward (what autograd runs for the reference: GNN.py:76-145 under
 * loss.backward(), trainer.py:142-143).  `dy` device [B] = dLoss/dy; writes every parameter
 * gradient into the table `grads` (same order and shapes as `params`, overwritten, not
 * accumulated).  `arena` must come from the matching forward call; `workspace` is scratch.
 *
 * `bucket_events` (NULL, or CGR_GRAD_BUCKETS(depth) hipEvent_t handles passed as void*): event b
 * is recorded on a stream of the backward as soon as every gradient of bucket b is final, so a
 * data-parallel caller can start bucket b's all-reduce while the rest of the backward runs
 * (trainer.py:138-144 has one device).  Buckets, in the order they become ready:
 *   0            edge_to_node.{weight,bias}, ffn.{weight,bias}
 *   1 + k        convs.(depth-1-k).lin.{weight,bias}            k = 0 .. depth-1
 *   depth + 1    edge_init.{weight,bias}, skip_weights.* (end of the backward, caller's stream) */
#define CGR_GRAD_BUCKETS(depth) ((depth) + 2)
int cgr_gnn_backward(const cgr_gnn_config* cfg, const float* const* params,
                     const cgr_batch* batch, const float* dropout_p, uint64_t seed,
                     int32_t training, const void* arena, const float* dy, float* const* grads,
                     void* workspace, void* const* bucket_events, void* stream);

/* Gradients with respect to the inputs (what autograd gives the reference for x / edge_attr
 * tensors that require grad: x enters through x[row] in edge_init, GNN.py:85-86, and through
 * cat([x, s]) in edge_to_node, GNN.py:105-106; edge_attr through edge_init only).  Call after
 * cgr_gnn_backward, on the same stream, with the same config / params / batch / arena / dy and
 * the SAME workspace (it reads the edge-init pre-activation gradient that backward left there).
 * dx: device [num_nodes, num_node_features] (NULL: skipped); dedge_attr: device
 * [num_edges, num_edge_features] in the caller's edge order (NULL: skipped); both overwritten,
 * fp32, 16-byte aligned.  Fails (nothing enqueued) unless `workspace` holds a successful
 * cgr_gnn_backward of `arena`'s latest forward (host-side record, no device sync). */
int cgr_gnn_input_grads(const cgr_gnn_config* cfg, const float* const* params,
                        const cgr_batch* batch, const void* arena, const float* dy,
                        void* workspace, float* dx, float* dedge_attr, void* stream);

/* Forward-only inference (test.py:85-113 and cli_tool/activation_energy_predictor.py:70-80 run
 * GNN.forward under torch.no_grad() in eval mode).  cgr_gnn_predict computes exactly what
 * cgr_gnn_forward computes for `y`, but keeps no activation for a backward (h_1 .. h_D share a
 * two-buffer ring and a_0 .. a_D a three-buffer one: its arena is ~half the training arena).
 * `images` NULL: the split-bf16 forward weight images are packed from `params` into the arena by
 * this call (one launch beside the graph bookkeeping; always current, whatever changed the weights
 * -- an optimizer writing through raw pointers, a replayed captured step).  Non-NULL: images
 * pre-packed by cgr_gnn_pack_images (cgr_gnn_image_bytes bytes, caller-owned), which the caller
 * must re-pack whenever the parameters change.  `training` may only hold CGR_TRAIN_DROPOUT
 * (module in train mode under no_grad).  Sizes: cgr_gnn_predict_arena_bytes. */
int64_t cgr_gnn_image_bytes(const cgr_gnn_config* cfg);
int cgr_gnn_pack_images(const cgr_gnn_config* cfg, const float* const* params, void* images,
                        void* stream);
int64_t cgr_gnn_predict_arena_bytes(const cgr_gnn_config* cfg, int64_t num_nodes,
                                    int64_t num_edges, int64_t num_graphs);
int cgr_gnn_predict(const cgr_gnn_config* cfg, const float* const* params,
                    const cgr_batch* batch, const float* dropout_p, uint64_t seed,
                    uint64_t* rng_counter, int32_t training, const void* images, void* arena,
                    float* y, void* stream);

/* The encoder without the ffn head (no reference entry point: the reference reaches the same
 * value with a forward hook on, or one line around, `self.pooling_fn(h, batch)`, GNN.py:110).
 * cgr_gnn_encode is cgr_gnn_forward up to and including the pooling: it fills `arena` the same way
 * (same layout, same dropout keying and counter advance) and writes the pooled graph embedding --
 * the learned reaction fingerprint -- to `g_out`, device [B, hidden] fp32 with row stride `hidden`
 * (no alignment required); no `y` is computed.  cgr_gnn_encode_backward is the reverse mode from a
 * general cotangent `dg`, device [B, hidden] fp32 contiguous, = dLoss/dg: every encoder gradient
 * of the table `grads`; cgr_gnn_encode_input_grads and cgr_gnn_encode_predict are the headless
 * forms of cgr_gnn_input_grads and cgr_gnn_predict.  All other arguments, the workspace, the
 * bucket events (bucket 0 then holds edge_to_node only) and the call order are those of the fused
 * calls.  The ffn.weight / ffn.bias entries of `params` and `grads` may be NULL and are never
 * read or written: any head (multi-target, an MLP) runs on g_out outside this library.
 * An arena remembers which forward filled it: cgr_gnn_backward / cgr_gnn_input_grads refuse an
 * arena of cgr_gnn_encode and cgr_gnn_encode_backward / _encode_input_grads one of
 * cgr_gnn_forward (nothing enqueued; cgr_last_error says why).  Both precision modes. */
int cgr_gnn_encode(const cgr_gnn_config* cfg, const float* const* params, const cgr_batch* batch,
                   const float* dropout_p, uint64_t seed, uint64_t* rng_counter, int32_t training,
                   void* arena, float* g_out, void* stream);
int cgr_gnn_encode_backward(const cgr_gnn_config* cfg, const float* const* params,
                            const cgr_batch* batch, const float* dropout_p, uint64_t seed,
                            int32_t training, const void* arena, const float* dg,
                            float* const* grads, void* workspace, void* const* bucket_events,
                            void* stream);
int cgr_gnn_encode_input_grads(const cgr_gnn_config* cfg, const float* const* params,
                               const cgr_batch* batch, const void* arena, const float* dg,
                               void* workspace, float* dx, float* dedge_attr, void* stream);
int cgr_gnn_encode_predict(const cgr_gnn_config* cfg, const float* const* params,
                           const cgr_batch* batch, const float* dropout_p, uint64_t seed,
                           uint64_t* rng_counter, int32_t training, const void* images,
                           void* arena, float* g_out, void* stream);

/* One level further down: the per-atom embedding hn = act(edge_to_node(cat[x, a_D])), the input
 * of `self.pooling_fn(h, batch)` (GNN.py:105-108), for atom-level attribution and targets and for
 * any readout the three native pools cannot express (attention, gated, set2set, a pool over the
 * reacting atoms only), which then runs on it outside this library.  The four calls mirror the
 * encode ones argument for argument.  cgr_gnn_encode_nodes is cgr_gnn_forward up to and including
 * the readout GEMM (same arena layout, dropout keying and counter advance) and writes `n_out`,
 * device [N, hidden] fp32 with row stride `hidden` (4-byte alignment; nothing outside [N, hidden]
 * is written).  cgr_gnn_encode_nodes_backward is the reverse mode from a general cotangent `dn`,
 * device [N, hidden] fp32 with row stride `hidden`, = dLoss/dhn; _encode_nodes_input_grads and
 * _encode_nodes_predict are the nodes forms of cgr_gnn_input_grads and cgr_gnn_predict.
 * cfg->pooling takes no part: it still sizes the arena, but no pooling state is read or written.
 * The ffn.weight / ffn.bias entries of `params` and `grads` may be NULL and are never read or
 * written.  An arena remembers the level of the forward that filled it -- the fused y, the pooled
 * g or the nodes -- and every backward / input-gradients entry refuses an arena of another level
 * (nothing enqueued; cgr_last_error names the call that belongs to the arena). */
int cgr_gnn_encode_nodes(const cgr_gnn_config* cfg, const float* const* params,
                         const cgr_batch* batch, const float* dropout_p, uint64_t seed,
                         uint64_t* rng_counter, int32_t training, void* arena, float* n_out,
                         void* stream);
int cgr_gnn_encode_nodes_backward(const cgr_gnn_config* cfg, const float* const* params,
                                  const cgr_batch* batch, const float* dropout_p, uint64_t seed,
                                  int32_t training, const void* arena, const float* dn,
                                  float* const* grads, void* workspace,
                                  void* const* bucket_events, void* stream);
int cgr_gnn_encode_nodes_input_grads(const cgr_gnn_config* cfg, const float* const* params,
                                     const cgr_batch* batch, const void* arena, const float* dn,
                                     void* workspace, float* dx, float* dedge_attr, void* stream);
int cgr_gnn_encode_nodes_predict(const cgr_gnn_config* cfg, const float* const* params,
                                 const cgr_batch* batch, const float* dropout_p, uint64_t seed,
                                 uint64_t* rng_counter, int32_t training, const void* images,
                                 void* arena, float* n_out, void* stream);

/* Sticky device-side conditions of `device` (no reference counterpart: the reference's autograd
 * cannot fail this way), read from pinned host memory the kernels write -- no device sync, so a
 * caller can poll it at every step.  A condition becomes visible once the kernel that raised it
 * has run.  Bits (cleared when `clear` != 0):
 *   CGR_DEVERR_UNPAIRED_TIMEOUT  a completer of the unpaired-edge backward (edges not
 *       reverse-paired, status bit 2) gave up waiting for the rest of its launch; the gradients
 *       of that backward are NaN-poisoned, never partial.  An error.
 *   CGR_DEVERR_UNPAIRED_SEEN  a backward ran the unpaired form (slower; informational).
 * Returns 0 before the device's first cgr_gnn_forward / _backward. */
#define CGR_DEVERR_UNPAIRED_SEEN 4
#define CGR_DEVERR_UNPAIRED_TIMEOUT 16
int32_t cgr_device_errors(int32_t device, int32_t clear);

/* Segmented sum, the sum-scatter primitive of the path (PyG propagate aggr="add", GNN.py:134;
 * global_add_pool, GNN.py:110) over a CSR: out[s, :] = sum_{j in [seg_ptr[s], seg_ptr[s+1])}
 * values[index ? index[j] : j, :].  width = row length in floats; ld_* = row strides (floats).
 * Deterministic (fixed summation order, no atomics). */
int cgr_segment_sum(const float* values, int64_t ld_values, const int32_t* index,
                    const int32_t* seg_ptr, int64_t num_segments, int64_t width, float* out,
                    int64_t ld_out, void* stream);

/* DMPNNConv.forward(edge_index, edge_attr) -> (a, h') (GNN.py:131-141), in the caller's edge
 * order: a[v] = sum_{dst(e)=v} h[e] (dim_size = N; aggregation CGR_AGGR_MEAN: divided by
 * max(in-degree, 1)), h'[e] = (a[src(e)] - h[e^1]) W^T + b.
 * `scratch` needs cgr_dmpnn_conv_scratch_bytes(N, E, H). */
int64_t cgr_dmpnn_conv_scratch_bytes(int64_t num_nodes, int64_t num_edges, int64_t hidden);
int cgr_dmpnn_conv_forward(const int64_t* edge_index, int64_t num_nodes, int64_t num_edges,
                           const float* h, int64_t hidden, const float* weight, const float* bias,
                           float* a_out, float* h_out, void* scratch, int32_t aggregation,
                           void* stream);
/* Reverse mode of cgr_dmpnn_conv_forward given dL/da (may be NULL) and dL/dh' (may be NULL):
 * writes dL/dh [E,H], dL/dW [H,H], dL/db [H].  `scratch` must hold the forward's bookkeeping
 * (same scratch buffer, untouched since the forward) plus cgr_dmpnn_conv_scratch_bytes. */
int cgr_dmpnn_conv_backward(const int64_t* edge_index, int64_t num_nodes, int64_t num_edges,
                            const float* h, int64_t hidden, const float* weight,
                            const float* grad_a, const float* grad_h_out, float* grad_h,
                            float* grad_weight, float* grad_bias, void* scratch,
                            int32_t aggregation, void* stream);

/* torch.optim.Adam(params, lr, betas, eps, weight_decay, amsgrad) step (train.py:117-119), fused
 * over every parameter tensor in one launch (+ one tiny launch for the step counter) instead of
 * the ~11 multi-tensor launches of torch's foreach path.  Per element, in the rounding order of
 * torch/optim/adam.py _multi_tensor_adam (hyper-parameters as Python doubles):
 *   g = grad (+ weight_decay * p);  m += (1 - b1) (g - m);  v = b2 v + (1 - b2) g^2;
 *   vmax = max(vmax, v) (amsgrad);  p -= lr / (1 - b1^t) * m / (sqrt(vmax or v) / sqrt(1 - b2^t) + eps)
 * with t = *step + 1 written back to *step: a per-tensor device float, like torch's state["step"]
 * (capturable=True), so a captured graph replays with the right bias corrections.  grad == NULL
 * skips a tensor and leaves its step (p.grad is None).  max_exp_avg_sq may be NULL when
 * amsgrad == 0.  Any number of tensors (launched in groups of CGR_ADAM_GROUP). */
#define CGR_ADAM_GROUP 32
typedef struct cgr_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* max_exp_avg_sq;
  float* step; /* device scalar */
  int64_t numel;
} cgr_adam_tensor;
int cgr_adam_step(const cgr_adam_tensor* tensors, int32_t num_tensors, double lr, double beta1,
                  double beta2, double eps, double weight_decay, int32_t amsgrad,
                  int32_t maximize, void* stream);
/* The same step with the learning rate read on the device (ABI 8): `lr` is a device fp32 scalar,
 * as torch.optim.Adam(lr=tensor, capturable=True) keeps it.  A scheduler that updates the scalar
 * in place (ExponentialLR of train.py:121) is then followed by a captured step's replays; the
 * kernel widens the value to double where cgr_adam_step uses its double argument, so an lr that
 * is exact in fp32 gives bit-identical updates on both entries. */
int cgr_adam_step_lr_ptr(const cgr_adam_tensor* tensors, int32_t num_tensors, const float* lr,
                         double beta1, double beta2, double eps, double weight_decay,
                         int32_t amsgrad, int32_t maximize, void* stream);

/* Global L2 gradient-norm clipping inside the step (added within ABI 9):
 * torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0) followed by the step above,
 * without the chain of foreach launches and without a host read.  One optimizer step is
 *   cgr_grad_sumsq once per tensor table (param group), each at its own offset of `partials`;
 *   cgr_adam_step_clip once per table, the first with num_partials = the sum of the counts.
 * cgr_grad_sumsq_partials: how many partials cgr_grad_sumsq writes for a table (host only; one per
 * block of the step kernel's decomposition; grad == NULL and numel <= 0 entries write none).
 * cgr_grad_sumsq: partials[b] = the fp32 sum of grad^2 over block b, in a fixed order; float4
 * loads where the gradient pointer is 16-byte aligned, scalar otherwise.  `capacity` is the
 * number of floats behind `partials`; a table that needs more is an error before any launch. */
int64_t cgr_grad_sumsq_partials(const cgr_adam_tensor* tensors, int32_t num_tensors);
int cgr_grad_sumsq(const cgr_adam_tensor* tensors, int32_t num_tensors, float* partials,
                   int64_t capacity, void* stream);
/* The step with the gradient scaled in registers by coef = min(1, max_norm / (norm + 1e-6))
 * before maximize and weight_decay apply (p.grad itself is not written: torch scales it in
 * place).  All pointers are device memory owned by the caller and static across steps:
 *   partials, num_partials: num_partials > 0 makes this call finalise the step's norm before its
 *     update: the step-count kernel sums the partials in a fixed order in double (no float
 *     atomics: identical gradient bits give identical norm bits), writes *grad_norm =
 *     (float)sqrt(sum), sets *gate = 1 if the sum is not finite (or the unpaired-backward timeout
 *     is flagged, as in cgr_adam_step), else 0, and adds 1 to *skipped_steps for a non-finite
 *     sum.  num_partials == 0: an earlier call of the same step did, and this one reads them.
 *   *gate != 0 skips the update: parameters, moments and *step stay as they were.
 *   max_norm: > 0 (infinity allowed: measured, never clipped); <= 0 = this table is not scaled,
 *     but still gated.
 *   lr_dev: NULL = the host value `lr`; else the device scalar of cgr_adam_step_lr_ptr. */
typedef struct cgr_adam_clip {
  const float* partials;
  int64_t num_partials;
  float* grad_norm;
  int32_t* gate;
  int64_t* skipped_steps;
  double max_norm;
} cgr_adam_clip;
int cgr_adam_step_clip(const cgr_adam_tensor* tensors, int32_t num_tensors, double lr,
                       const float* lr_dev, double beta1, double beta2, double eps,
                       double weight_decay, int32_t amsgrad, int32_t maximize,
                       const cgr_adam_clip* clip, void* stream);

/* On-device collation (replaces torch_geometric.loader.DataLoader / Batch.from_data_list in
 * trainer.py:105-118 over the per-reaction Data of ChemDataset.py:81-94).  The store holds every
 * graph of a dataset collated once on the device: graph g owns node rows [node_ptr[g],
 * node_ptr[g+1]) of x [*, F] and edges [edge_ptr[g], edge_ptr[g+1]) of edge_index [2,
 * num_edges_all] (global node ids) / edge_attr [*, Fe]; y [G] may be NULL.  For graph_ids[0..B)
 * (device) it writes exactly what Batch.from_data_list would: x_out [sum nodes, F], edge_index_out
 * [2, num_edges_out] re-based to the running node count, edge_attr_out, batch_out [sum nodes]
 * (= position in graph_ids), ptr_out [B+1], y_out [B].  The caller sizes the outputs (the counts
 * are known on the host from its copy of node_ptr / edge_ptr).  Bit-exact; one launch. */
int cgr_collate(const int64_t* graph_ids, int64_t num_ids, const int64_t* node_ptr,
                const int64_t* edge_ptr, const float* x, int64_t num_node_features,
                const int64_t* edge_index, int64_t num_edges_all, const float* edge_attr,
                int64_t num_edge_features, const float* y, float* x_out, int64_t* edge_index_out,
                int64_t num_edges_out, float* edge_attr_out, int64_t* batch_out, int64_t* ptr_out,
                float* y_out, void* stream);

/* Fixed-shape collation (ABI 8): cgr_collate's batch followed by one pad graph, so every batch
 * has the shapes node_cap / edge_cap (edge_cap even) whatever its graphs hold, and a captured
 * training step can replay over ragged batches.  Every argument the batch depends on is device
 * memory -- graph_ids [B], slot_weight [B] (the loss weight of each slot: 1 real, 0 filler) --
 * and the grid depends on B and the capacities only.  With N_real / E_real the node / edge sums
 * of the ids (reduced on the device):
 *   rows [0, N_real) / [0, E_real) of x_out [node_cap, F], edge_index_out [2, edge_cap] (row
 *     stride edge_cap), edge_attr_out [edge_cap, Fe], batch_out [node_cap] and ptr_out[0..B),
 *     y_out[0..B): exactly cgr_collate's output; mask_out[0..B) = slot_weight;
 *   the pad graph is slot B: P = node_cap - N_real nodes with x = 0, batch = B;
 *     ptr_out[B] = N_real, ptr_out[B+1] = node_cap, y_out[B] = 0, mask_out[B] = 0 (ptr_out has
 *     B + 2 entries, y_out / mask_out B + 1);
 *   pad edge pair j < (edge_cap - E_real) / 2: edge E_real + 2j = (a -> b), edge E_real + 2j + 1 =
 *     (b -> a) with a = N_real + j mod P, b = N_real + (j + 1) mod P, edge_attr = 0: reverse
 *     pairs (rev(e) = e ^ 1) like the real edges;
 *   info [4] int64 = N_real, E_real, status, 0.  Status bits: 1 = the batch does not fit
 *     (N_real + 2 > node_cap or E_real > edge_cap), 2 = edge_cap - E_real is odd, 4 = an id
 *     outside [0, num_graphs_all) (taken as an empty graph).  With bit 1 or 2 set the outputs
 *     inside the capacities are unspecified; nothing is ever written outside them.
 * The pad graph's loss weight is 0, so dy = 0 for slot B and it adds an exact 0 to every
 * gradient as long as its forward values are finite: the caller bounds the pad in-degree
 * (2 ceil(pairs / P)).  One launch. */
int cgr_collate_padded(const int64_t* graph_ids, const float* slot_weight, int64_t num_ids,
                       int64_t num_graphs_all, const int64_t* node_ptr, const int64_t* edge_ptr,
                       const float* x, int64_t num_node_features, const int64_t* edge_index,
                       int64_t num_edges_all, const float* edge_attr, int64_t num_edge_features,
                       const float* y, int64_t node_cap, int64_t edge_cap, float* x_out,
                       int64_t* edge_index_out, float* edge_attr_out, int64_t* batch_out,
                       int64_t* ptr_out, float* y_out, float* mask_out, int64_t* info,
                       void* stream);

/* Training loss (replaces torch.nn.MSELoss(reduction="sum") of train.py:120 as trainer.py:142-143
 * applies it; reduction_mean != 0 is MSELoss(reduction="mean")).  input, target: device [n] fp32.
 * forward: *loss (device scalar) = sum (input - target)^2 (/ n).  backward: grad_input =
 * 2 (input - target) grad_loss[0] (/ n), grad_target = -grad_input; either output may be NULL.
 * One launch each, deterministic. */
int cgr_mse_loss_forward(const float* input, const float* target, int64_t n,
                         int32_t reduction_mean, float* loss, void* stream);
int cgr_mse_loss_backward(const float* input, const float* target, const float* grad_loss,
                          int64_t n, int32_t reduction_mean, float* grad_input,
                          float* grad_target, void* stream);
/* The robust losses beside it (added within ABI 9), argument for argument the MSE pair, with
 * d = input - target:
 *   torch.nn.L1Loss: sum |d| (/ n); grad_input = sign(d) grad_loss[0] (/ n), 0 at d == 0.
 *   torch.nn.HuberLoss(delta), delta > 0: sum of d^2 / 2 where |d| < delta, else
 *     delta (|d| - delta / 2) (/ n); grad_input = d grad_loss[0] (/ n) where |d| <= delta, else
 *     delta sign(d) grad_loss[0] (/ n).
 * grad_target = -grad_input.  One launch each, deterministic. */
int cgr_l1_loss_forward(const float* input, const float* target, int64_t n,
                        int32_t reduction_mean, float* loss, void* stream);
int cgr_l1_loss_backward(const float* input, const float* target, const float* grad_loss,
                         int64_t n, int32_t reduction_mean, float* grad_input,
                         float* grad_target, void* stream);
int cgr_huber_loss_forward(const float* input, const float* target, int64_t n,
                           int32_t reduction_mean, double delta, float* loss, void* stream);
int cgr_huber_loss_backward(const float* input, const float* target, const float* grad_loss,
                            int64_t n, int32_t reduction_mean, double delta, float* grad_input,
                            float* grad_target, void* stream);

/* Attention pooling over atom embeddings (added within ABI 9; no reference counterpart: the
 * readout GNN.encode_nodes was added for, as one kernel each way).  A gated softmax over each
 * graph's atoms:
 *   s_v = x[v].weight + bias[0] ; alpha_v = exp(s_v - max_u s_u) / sum_u exp(s_u - max_u s_u)
 *   over the unmasked atoms u of v's graph (alpha_v = 0 for a masked atom) ; g[b] = sum_v alpha_v x[v]
 * x: device [N, H] fp32, row stride ldx >= H (floats).  Graph b's atoms are rows [ptr[b],
 * ptr[b + 1]) when ptr (device int64 [B + 1]) is given; else the rows whose id in batch (device
 * int64 [N], sorted ascending) is b, found by binary search inside the kernel; with neither,
 * B == 1 and the one graph is all N rows.  weight [H]; bias [1] or NULL; mask: device bytes [N],
 * nonzero = the atom takes part, or NULL.  Outputs: g [B, H] (row stride H), alpha [N].  Every
 * atom is expected to belong to one of the B graphs: alpha and dx rows of atoms outside all of
 * them are not written.
 * A graph without unmasked atoms gives a g row of +0.0 and alpha 0: nothing is divided by its zero
 * sum.  The maximum is subtracted, so scores of any magnitude are safe.  One workgroup per graph,
 * atoms summed in order: deterministic, and a graph's results depend on its own rows only.
 * forward: one launch.
 * backward, from dg [B, H] (row stride H) and the forward's alpha, with t_v = dg[b].x[v],
 *   c_b = sum_v alpha_v t_v, ds_v = alpha_v (t_v - c_b):
 *   dx[v] = alpha_v dg[b] + ds_v weight   [N, H], row stride H (masked atoms: exact zeros)
 *   dw    = sum_v ds_v x[v]               [H]
 * either may be NULL.  The bias has no gradient entry: the softmax is invariant to a shift of
 * every score, so d/d bias is exactly 0.  workspace: cgr_attention_pool_workspace_bytes(B, H)
 * bytes, 16-byte aligned, needed (and touched) only when dw is wanted: one dw partial per graph,
 * summed over the graphs in a fixed order by a second launch.
 * Refused before any launch: H <= 0, ldx < H, N or B out of range, B > 1 without batch and ptr,
 * NULL required pointers, a misaligned workspace. */
int64_t cgr_attention_pool_workspace_bytes(int64_t B, int64_t H);
int cgr_attention_pool_forward(const float* x, int64_t ldx, int64_t N, int64_t H,
                               const int64_t* batch, const int64_t* ptr, int64_t B,
                               const float* weight, const float* bias, const uint8_t* mask,
                               float* g, float* alpha, void* stream);
int cgr_attention_pool_backward(const float* x, int64_t ldx, int64_t N, int64_t H,
                                const int64_t* batch, const int64_t* ptr, int64_t B,
                                const float* weight, const float* alpha, const float* dg,
                                float* dx, float* dw, void* workspace, void* stream);

/* Mean-variance head on the pooled fingerprint (added within ABI 9; no reference counterpart: the
 * head of a heteroscedastic regression, one launch each way).  g: device [B, H] fp32, row stride
 * ldg >= H (floats), the output of cgr_gnn_encode or of the attention pool.
 *   mu[b] = g[b].w_mu + b_mu[0] ; raw[b] = g[b].w_var + b_var[0]
 *   var[b] = softplus(raw[b]) + min_var     (torch's softplus: beta 1, raw itself above 20)
 * w_mu, w_var [H]; b_mu, b_var [1] or NULL (= 0).  Outputs: out [B, 2] interleaved (out[b, 0] =
 * mu, out[b, 1] = var) and raw [B], what the backward reads (NULL: not stored).
 * backward, from dout [B, 2] and the forward's raw, with draw[b] = dout[b, 1] sigmoid(raw[b]) (1
 * above the threshold):
 *   dg[b] = dout[b, 0] w_mu + draw[b] w_var                       [B, H], row stride H
 *   dW    = (sum_b dout[b, 0] g[b], sum_b draw[b] g[b])           [2, H]
 *   db    = (sum_b dout[b, 0], sum_b draw[b])                     [2]
 * each may be NULL and is then not computed.  Every sum has a fixed shape and order (no atomics):
 * results are reproducible, and a row of out and of dg is the same bits whether its graph is
 * computed alone or in any batch.  No workspace.
 * Refused before any launch: H <= 0, ldg < H, B out of range, NULL required pointers (g, w_mu,
 * w_var; out; raw and dout in the backward), a min_var that is negative or not finite. */
int cgr_meanvar_head_forward(const float* g, int64_t ldg, int64_t B, int64_t H,
                             const float* w_mu, const float* b_mu, const float* w_var,
                             const float* b_var, double min_var, float* out, float* raw,
                             void* stream);
int cgr_meanvar_head_backward(const float* g, int64_t ldg, int64_t B, int64_t H,
                              const float* w_mu, const float* w_var, const float* raw,
                              const float* dout, float* dg, float* dW, float* db, void* stream);

/* torch.nn.GaussianNLLLoss (added within ABI 9).  mu and var are read with an element stride
 * (mu[i * mu_stride], var[i * var_stride]: 1 for contiguous tensors; 2 with var = mu + 1 for the
 * two columns of the head's out [n, 2] in place); target, weight: device [n] fp32, weight may be
 * NULL (= all 1).  With v = max(var, eps) and d = mu - target:
 *   *loss = sum_i w_i (0.5 (log v_i + d_i^2 / v_i) + (full ? 0.5 log 2 pi : 0))   (/ n)
 *   grad_mu = w (d / v) grad_loss[0] (/ n) ; grad_target = -grad_mu
 *   grad_var = w 0.5 (1 / v - d^2 / v^2) grad_loss[0] (/ n), evaluated at the clamped v and
 *     handed to var unchanged also where var < eps (torch's clamp is not differentiated)
 * grad_mu and grad_var are written at [i * grad_stride] (grad_var = grad_mu + 1, stride 2: one
 * [n, 2] tensor); each gradient may be NULL.  The mean divides by n whatever the weights are (as
 * torch's weighted losses do).  An element with w_i == 0 is skipped, not multiplied: it adds
 * nothing and its gradients are +0.0 whatever mu, var and target hold there (NaN, inf, var <= 0).
 * A negative var is not an error here (torch raises, at the price of a host sync).
 * One launch each, deterministic.  Refused before any launch: n < 0, a stride < 1, eps that is
 * not > 0 and finite, NULL required pointers. */
int cgr_gaussian_nll_loss_forward(const float* mu, int64_t mu_stride, const float* var,
                                  int64_t var_stride, const float* target, const float* weight,
                                  int64_t n, int32_t reduction_mean, int32_t full, double eps,
                                  float* loss, void* stream);
int cgr_gaussian_nll_loss_backward(const float* mu, int64_t mu_stride, const float* var,
                                   int64_t var_stride, const float* target, const float* weight,
                                   const float* grad_loss, int64_t n, int32_t reduction_mean,
                                   double eps, float* grad_mu, float* grad_var,
                                   int64_t grad_stride, float* grad_target, void* stream);

/* The weighted forms of the MSE / L1 / Huber pairs above (added within ABI 9): sum_i w_i l_i
 * (/ n), grad_input = w_i l_i' grad_loss[0] (/ n), grad_target = -grad_input, with the same terms
 * l_i.  weight: device [n] fp32, required (the unweighted losses are the entries above); delta is
 * read for CGR_LOSS_HUBER only.  An element with w_i == 0 is skipped, as in the Gaussian loss: it
 * adds nothing and its gradients are +0.0 whatever input and target hold there.  One launch each,
 * deterministic. */
enum cgr_weighted_loss { CGR_LOSS_MSE = 0, CGR_LOSS_L1 = 1, CGR_LOSS_HUBER = 2 };
int cgr_weighted_loss_forward(int32_t kind, const float* input, const float* target,
                              const float* weight, int64_t n, int32_t reduction_mean,
                              double delta, float* loss, void* stream);
int cgr_weighted_loss_backward(int32_t kind, const float* input, const float* target,
                               const float* weight, const float* grad_loss, int64_t n,
                               int32_t reduction_mean, double delta, float* grad_input,
                               float* grad_target, void* stream);

/* Instrumentation (no reference counterpart): per-kernel-class device time measured with HIP
 * events recorded on the launch stream around every launch of cgr_gnn_forward/_backward.
 * Off by default; do not enable while capturing a graph.  cgr_profile_collect() waits for the
 * recorded events; cgr_profile_report() writes "name count total_ms" lines and returns the
 * buffer size needed. */
int cgr_profile_enable(int32_t on);
int cgr_profile_collect(void);
void cgr_profile_reset(void);
int64_t cgr_profile_report(char* buf, int64_t len);

/* Diagnostic builds only (-DCGR_STAMPS, tools/stamp_lab.py): every split-bf16 NT GEMM workgroup
 * appends one 16 x uint64 record of shader-clock phase stamps to `buffer` (device, zeroed by the
 * caller; its first 16 bytes are the record counter) for at most `records` workgroups; NULL stops
 * recording.  The product build returns CGR_ERR_UNSUPPORTED. */
int cgr_debug_stamps(void* buffer, int64_t records);

/* Process diagnostics (no reference counterpart): on != 0 installs a SIGABRT handler that prints
 * the aborting thread's id, name and native backtrace to stderr, then passes the signal to the
 * handler installed before it (e.g. Python's faulthandler) or the default action; 0 restores
 * that handler.  Used by the multi-process / RCCL tests and the distributed bench, so an abort in
 * a runtime thread without Python frames still names its origin. */
int cgr_debug_abort_backtrace(int32_t on);

#ifdef __cplusplus
}
#endif

#endif /* CGR_MPNN3D_H */
