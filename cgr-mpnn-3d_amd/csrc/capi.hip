// C ABI of libcgr_mpnn3d.so (include/cgr_mpnn3d.h): validation, arena/workspace layout, error
// reporting.  No entry point allocates or synchronises; all work is enqueued on `stream`.
#include <string.h>

#include <algorithm>
#include <string>

#include "arena_book.hpp"
#include "dispatch.hpp"
#include "gnn_internal.hpp"
#include "kernels.hpp"
#include "streams.hpp"

namespace cgr {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

// what the last forward left in each arena, and which workspace holds its backward
static ArenaBook g_arenas;

// the calls of one output level and the names of its output and cotangent, for the messages
struct LevelCalls {
  const char *fwd, *bwd, *igr, *pred, *out, *up, *what;
};
static const LevelCalls& calls_of(OutLevel level) {
  static const LevelCalls k[3] = {
      {"cgr_gnn_forward", "cgr_gnn_backward", "cgr_gnn_input_grads", "cgr_gnn_predict", "y", "dy",
       "with the ffn head"},
      {"cgr_gnn_encode", "cgr_gnn_encode_backward", "cgr_gnn_encode_input_grads",
       "cgr_gnn_encode_predict", "g_out", "dg", "headless, no ffn head"},
      {"cgr_gnn_encode_nodes", "cgr_gnn_encode_nodes_backward", "cgr_gnn_encode_nodes_input_grads",
       "cgr_gnn_encode_nodes_predict", "n_out", "dn",
       "per-atom embeddings, no pooling or ffn head"}};
  return k[(int)level];
}
int gnn_forward_impl(const Dims& d, const float* const* params, const cgr_batch* b,
                     const float* dropout_p, uint64_t seed, uint64_t* rng_counter, int training,
                     void* arena, float* y, hipStream_t st, const FwdMode& mode);
hipError_t pack_forward_images(const Dims& d, const float* const* params, const Images& im,
                               hipStream_t st);
int gnn_backward_impl(const Dims& d, const float* const* params, const cgr_batch* b,
                      const float* dropout_p, uint64_t seed, int training, const void* arena,
                      const float* dy, float* const* grads, void* workspace,
                      hipEvent_t const* bucket_events, hipStream_t st, OutLevel level);
int gnn_input_grads_impl(const Dims& d, const float* const* params, const void* arena,
                         const float* dy, void* workspace, float* dx, float* de, hipStream_t st,
                         OutLevel level);

Dims make_dims(const cgr_gnn_config* cfg, int64_t N, int64_t E, int64_t B) {
  Dims d;
  d.N = N;
  d.E = E;
  d.B = B;
  d.F = cfg->num_node_features;
  d.Fe = cfg->num_edge_features;
  d.Fep = (int)round_up(d.Fe, 4);
  d.Fp = (int)round_up(d.F, 4);
  d.H = cfg->hidden;
  d.Hp = (int)round_up(d.H, 4);
  d.D = cfg->depth;
  d.act = cfg->activation;
  d.learnable_skip = cfg->learnable_skip ? 1 : 0;
  d.aggr = cfg->aggregation;
  d.pool = cfg->pooling;
  d.precision = cfg->precision;
  return d;
}

// ---- layouts: each function below states every region of one buffer once, in placement order,
// as a call on the placer (layout.hpp); the views, the byte totals and the offset queries all
// come from these statements.  A new region is a member of its view (gnn_internal.hpp) and one
// line here.

// The forward weight images in the column tilings given: one sizing rule for the training arena
// (which places each backward image behind its forward one: `bwd`), the eval arena and a
// caller-packed image buffer
template <class V>
static void image_regions(const Dims& d, const B3Cols& cx, const B3Cols& cr, const B3Cols& cl,
                          bool bwd, Images& im, V& v) {
  v(im.b3x, 16 * b3_img_u4(cx, d.F), d.F > 0);
  v(im.b3rof, 16 * b3_img_u4(cr, d.H));
  v(im.b3rob, 16 * b3_img_u4(cr, d.H), bwd);
  for (int l = 0; l < d.D; ++l) {
    v(im.b3lf[l], 16 * b3_img_u4(cl, d.H));
    v(im.b3lb[l], 16 * b3_img_u4(cl, d.H), bwd);
  }
}

// index bookkeeping, sorted edge features and the x-GEMM outputs: the prefix both arenas share
// (a predict arena's `status` is read at the training layout's offset)
template <class V>
static void prefix_regions(const Dims& d, ArenaView& a, V& v) {
  IndexView& i = a.idx;
  FloatView& f = a.flt;
  const size_t N = (size_t)d.N, E = (size_t)d.E, B = (size_t)d.B, Hp = (size_t)d.Hp;
  // the layer forward runs in layer_cols(d), or in image_cols(d, H) over caller-packed images
  // (predict)
  const B3Cols lc = layer_cols(d), dc = image_cols(d, d.H);
  // zero block: six int arrays back to back + the ticket counters of the layer GEMMs' hub
  // segments (EpLayerSeg, ep_fwd.hpp: zero on entry, reset by each completer), padded to a
  // multiple of 16 bytes
  v.packed(i.deg_dst, N);
  v.packed(i.deg_src, N);
  v.packed(i.cursor, N);
  v.packed(i.cursor2, N);
  v.packed(i.graph_cnt, B);
  v.packed(i.status, 4, "status");
  v.packed(i.fcnt, N * (size_t)std::max(lc.tiles, dc.tiles));
  v.block(i.zero_block, i.deg_dst, 16);
  v("rng", i.rng, 1);
  v("perm", i.perm, E);
  v("src_s", i.src_s, E);
  v("dst_s", i.dst_s, E);
  v("rev_s", i.rev_s, E);
  v("src_list", i.src_list, E);
  v(i.inv, E);
  v(i.src_c, E);
  v(i.dst_c, E);
  v("dst_ptr", i.dst_ptr, N + 1);
  v("src_ptr", i.src_ptr, N + 1);
  v("graph_ptr", i.graph_ptr, B + 1);
  v("node_graph", i.node_graph, N);
  v("e_s", f.e_s, E * (size_t)d.Fep, d.Fep != 0);
  v(f.w0eT, (size_t)d.Fe * Hp, d.Fe != 0);
  v("P", f.P, N * Hp);
  v("Q", f.Q, N * Hp);
  v(f.xp, N * (size_t)d.Fp, d.F % 4 != 0);
  v(f.inv_deg, N, d.aggr == CGR_AGGR_MEAN);
  v(f.inv_cnt, B, d.pool == CGR_POOL_MEAN);
  v(f.pool_arg, B * Hp, d.pool == CGR_POOL_MAX);
  // partial sums of the layer GEMMs' hub segments (over >= 3 row tiles), one slot pair per tile
  const size_t rt = (size_t)cdiv(d.E, b3nt_rows((int)d.E, d.H));
  v(f.fpart, rt * 2 * 16 * std::max((size_t)lc.tiles * lc.nf, (size_t)dc.tiles * dc.nf));
}

// training arena (cgr_gnn_forward and its kin): every activation the backward reads is saved
template <class V>
static size_t train_regions(const Dims& d, ArenaView& a, V& v) {
  FloatView& f = a.flt;
  const size_t N = (size_t)d.N, E = (size_t)d.E, B = (size_t)d.B, Hp = (size_t)d.Hp;
  prefix_regions(d, a, v);
  // the x-GEMM and the node-row readout GEMMs in their grid-filling column tilings
  image_regions(d, x_cols(d), readout_cols(d), layer_cols(d), true, f, v);
  for (int l = 0; l <= d.D; ++l) {
    v("h", f.h[l], E * Hp, true, l);
    v("a", f.a[l], N * Hp, true, l);
    v("pre", f.pre[l], E * Hp, d.act != CGR_ACT_RELU, l);
  }
  v("zn", f.zn, N * Hp, d.act != CGR_ACT_RELU);
  v("hn", f.hn, N * Hp);
  v("g", f.g, B * Hp);
  return v.off;
}

// eval arena (cgr_gnn_predict and its kin): h_1 .. h_D alias a two-buffer ring, a_0 .. a_D a
// three-buffer ring; the forward images are packed into it by every predict that is not handed
// pre-packed ones
template <class V>
static size_t eval_regions(const Dims& d, ArenaView& a, V& v) {
  FloatView& f = a.flt;
  const size_t N = (size_t)d.N, E = (size_t)d.E, B = (size_t)d.B, Hp = (size_t)d.Hp;
  prefix_regions(d, a, v);
  Reg<float> hr[2], ar[3];
  v(f.h[0], E * Hp);
  v(hr[0], E * Hp, d.D >= 2);
  v(hr[1], E * Hp);
  v(ar[0], N * Hp);
  v(ar[1], N * Hp);
  v(ar[2], N * Hp, d.D >= 2);
  for (int l = 0; l <= d.D; ++l) {
    if (l > 0) f.h[l] = hr[l & 1];
    f.a[l] = ar[l % 3];
  }
  v(f.hn, N * Hp);
  v(f.g, B * Hp);
  image_regions(d, x_cols(d), readout_cols(d), layer_cols(d), false, f, v);
  return v.off;
}

// caller-packed image buffer (cgr_gnn_pack_images): batch-independent tilings
template <class V>
static size_t image_buffer_regions(const Dims& d, Images& im, V& v) {
  image_regions(d, image_cols(d, 2 * d.H), image_cols(d, d.H), image_cols(d, d.H), false, im, v);
  return v.off;
}

ArenaView arena_view(const Dims& d, bool eval, void* arena) {
  ArenaView a;
  Placer<> v{static_cast<char*>(arena)};
  eval ? eval_regions(d, a, v) : train_regions(d, a, v);
  return a;
}

Images image_view(const Dims& d, void* images) {
  Images im;
  Placer<> v{static_cast<char*>(images)};
  image_buffer_regions(d, im, v);
  return im;
}
// column tiling of the layer GEMMs (forward and fused backward) over this batch's E rows: b3_cols
// when that fills the chip, else the narrower tiles of b3nt_cols (small batches: train.py's 32
// reactions run 60 -> 210 workgroups per layer GEMM)
// (every tiling in d's precision mode: the per-k-step accumulation variant of the NT kernel runs
// narrower tiles, gemm_b3.hpp kB3AccMaxNf)
B3Cols layer_cols(const Dims& d) { return b3nt_cols((int)d.E, d.H, d.nt_acc()); }
// the x-GEMM's and the readout GEMMs' grid-filling tilings over this batch's N rows
B3Cols x_cols(const Dims& d) { return b3nt_cols((int)d.N, 2 * d.H, d.nt_acc()); }
B3Cols readout_cols(const Dims& d) { return b3nt_cols((int)d.N, d.H, d.nt_acc()); }
// caller-packed images (cgr_gnn_pack_images) know no batch: b3_cols
B3Cols image_cols(const Dims& d, int n) { return b3_cols(n, d.nt_acc()); }

// row tiles x column tiles of the fused layer-backward GEMM (gnn_bwd.hip, ep_bwd.hpp)
int bwd_seg_tiles(const Dims& d) {
  return (int)cdiv(d.E, b3nt_rows((int)d.E, d.H)) * layer_cols(d).tiles;
}

// learnable-skip partial sums per layer: the top layer's activation kernel writes one per block,
// the fused layer-backward GEMM below it two per workgroup (its rows, the crossing segment that
// starts in its tile: ep_bwd.hpp)
int bwd_dsig_slots(const Dims& d) {
  return (int)std::max<int64_t>(2 * (int64_t)bwd_seg_tiles(d), layer_act_bwd_blocks(d.E, d.Hp));
}

// backward workspace (cgr_gnn_backward and its kin, then cgr_gnn_input_grads)
template <class V>
static size_t workspace_regions(const Dims& d, WorkspaceView& w, V& v) {
  const size_t N = (size_t)d.N, E = (size_t)d.E, Hp = (size_t)d.Hp;
  // public names: only what gnn_backward_impl leaves complete in fp32 on every path
  // (gnn_bwd.hip): Gs exists as an e-image alone on the split-bf16 paths, dm holds hand-off rows
  // only
  v.layers("dpre", w.dpre, E * Hp, d.D);  // one per layer (gnn_bwd.hip)
  v(w.dm, E * Hp);
  v("dpre0", w.dh0, E * Hp);  // dpre0 is written in place of dh0
  // "dzn_main": dzn [N, Hp] where the backward materialises it in fp32 on the caller's stream for
  // the readout NT -- below the fused level (cgr_gnn_encode_backward,
  // cgr_gnn_encode_nodes_backward) and under max pooling.  ("dzn" stays unknown: the fused add /
  // mean backward on the split-bf16 path never stores it.)
  v("dzn_main", w.dzn, N * Hp);
  v("ds", w.ds, N * Hp);
  v(w.Gs, N * Hp);
  // e-images: only where a site lists the split-bf16 family (not in CGR_PRECISION_FP32)
  bool eimg = false;
  for (WgSite s : {WgSite::Readout, WgSite::Layer, WgSite::Node}) {
    const WgCandidates c = wgrad_candidates(s, d);
    for (int i = 0; i < c.n; ++i) eimg = eimg || c.c[i].family == WgFamily::B3;
  }
  v(w.img_side, eimg ? b3_eimg_bytes(std::max(d.E, d.N), d.H) : 0);
  v(w.img_main, eimg ? b3_eimg_bytes(d.N, d.H) : 0);
  v(w.img_top, eimg ? b3_eimg_bytes(d.E, d.H) : 0);
  // split-K slabs: the largest over every family a site may pick for these dims (wgrad.hpp, the
  // table gnn_bwd.hip launches through).  The side-stream weight gradients (readout, layers, edge
  // features) run one after another and share `slab` (two, alternating: gnn_bwd.hip); the node
  // weight gradient runs beside them on the caller's stream: `slab2`.
  size_t slab = 0, bslab = 0, slab2 = 0, bslab2 = 0;
  auto fit = [&](WgSite s, size_t* sl, size_t* bs) {
    const WgCandidates c = wgrad_candidates(s, d);
    for (int i = 0; i < c.n; ++i) {
      *sl = std::max(*sl, c.c[i].slab_elems());
      *bs = std::max(*bs, c.c[i].bslab_elems());
    }
  };
  for (WgSite s : {WgSite::Readout, WgSite::Layer, WgSite::Edge}) fit(s, &slab, &bslab);
  fit(WgSite::Node, &slab2, &bslab2);
  for (int k = 0; k < 2; ++k) {
    v.floored(w.slab[k], slab);
    v.floored(w.bslab[k], bslab);
  }
  v.floored(w.slab2, slab2);
  v.floored(w.bslab2, bslab2);
  v(w.dag, 2 * N * Hp);  // two, alternating by layer
  v(w.cnt, N * (size_t)layer_cols(d).tiles + CGR_MAX_DEPTH);
  v(w.part, (size_t)bwd_seg_tiles(d) * 2 * (size_t)layer_cols(d).nf * 16);
  v(w.wxT, (size_t)d.F * (size_t)input_grad_ldw(d.H));
  v(w.dsig_part, (size_t)d.D * (size_t)bwd_dsig_slots(d));
  return v.off;
}

WorkspaceView workspace_view(const Dims& d, void* workspace) {
  WorkspaceView w;
  Placer<> v{static_cast<char*>(workspace)};
  workspace_regions(d, w, v);
  return w;
}
static int validate_config(const cgr_gnn_config* c) {
  CGR_CHECK(c != nullptr, "cgr: config is NULL");
  CGR_CHECK(c->num_node_features >= 0, "cgr: num_node_features must be >= 0");
  CGR_CHECK(c->num_edge_features >= 0, "cgr: num_edge_features must be >= 0");
  CGR_CHECK(c->hidden >= 1, "cgr: hidden size must be >= 1");
  CGR_CHECK(c->depth >= 1 && c->depth <= CGR_MAX_DEPTH, "cgr: depth must be in [1, 32]");
  CGR_CHECK(c->activation >= 0 && c->activation < ACT_COUNT, "cgr: unknown activation code");
  CGR_CHECK(c->aggregation == CGR_AGGR_ADD || c->aggregation == CGR_AGGR_MEAN,
            "cgr: unknown aggregation (CGR_AGGR_ADD, CGR_AGGR_MEAN)");
  CGR_CHECK(c->pooling == CGR_POOL_ADD || c->pooling == CGR_POOL_MEAN ||
                c->pooling == CGR_POOL_MAX,
            "cgr: unknown pooling (CGR_POOL_ADD, CGR_POOL_MEAN, CGR_POOL_MAX)");
  CGR_CHECK(c->precision == CGR_PRECISION_SPLIT || c->precision == CGR_PRECISION_FP32,
            "cgr: unknown precision (CGR_PRECISION_SPLIT, CGR_PRECISION_FP32)");
  return 0;
}

static int validate_batch(const cgr_gnn_config* c, const cgr_batch* b) {
  CGR_CHECK(b != nullptr, "cgr: batch is NULL");
  CGR_CHECK(b->num_nodes >= 1 && b->num_nodes < (1ll << 31), "cgr: num_nodes out of range");
  CGR_CHECK(b->num_edges >= 1 && b->num_edges < (1ll << 30),
            "cgr: num_edges must be >= 1 (the reference's flip/view needs edge pairs)");
  CGR_CHECK(b->num_edges % 2 == 0,
            "cgr: num_edges must be even: reverse edge of e is e^1 (GNN.py:136-138)");
  CGR_CHECK(b->num_graphs >= 1 && b->num_graphs <= b->num_nodes, "cgr: num_graphs out of range");
  CGR_CHECK(b->batch != nullptr || b->graph_ptr != nullptr || b->num_graphs == 1,
            "cgr: batch == NULL requires num_graphs == 1");
  CGR_CHECK(b->edge_index != nullptr, "cgr: edge_index is NULL");
  CGR_CHECK(c->num_node_features == 0 || b->x != nullptr, "cgr: x is NULL");
  CGR_CHECK(c->num_edge_features == 0 || b->edge_attr != nullptr, "cgr: edge_attr is NULL");
  return 0;
}

}  // namespace cgr

using namespace cgr;

extern "C" {

int cgr_abi_version(void) { return CGR_ABI_VERSION; }

const char* cgr_last_error(void) { return g_err.c_str(); }

int cgr_gnn_num_params(const cgr_gnn_config* cfg) {
  if (validate_config(cfg)) return -1;
  return 6 + 2 * cfg->depth + (cfg->learnable_skip ? cfg->depth : 0);
}

int64_t cgr_gnn_arena_bytes(const cgr_gnn_config* cfg, int64_t N, int64_t E, int64_t B) {
  if (validate_config(cfg)) return -1;
  ArenaView a;
  Placer<> v;
  return (int64_t)train_regions(make_dims(cfg, N, E, B), a, v);
}

int64_t cgr_gnn_workspace_bytes(const cgr_gnn_config* cfg, int64_t N, int64_t E, int64_t B) {
  if (validate_config(cfg)) return -1;
  WorkspaceView w;
  Placer<> v;
  return (int64_t)workspace_regions(make_dims(cfg, N, E, B), w, v);
}

// the offset queries: the names the region statements carry; -1 for any other name, an absent
// region or an index out of range
int64_t cgr_gnn_arena_offset(const cgr_gnn_config* cfg, int64_t N, int64_t E, int64_t B,
                             const char* name, int32_t index) {
  if (validate_config(cfg) || name == nullptr) return -1;
  ArenaView a;
  Placer<FindName> v{nullptr, {name, index}};
  train_regions(make_dims(cfg, N, E, B), a, v);
  return v.note.found;
}

int64_t cgr_gnn_workspace_offset(const cgr_gnn_config* cfg, int64_t N, int64_t E, int64_t B,
                                 const char* name, int32_t index) {
  if (validate_config(cfg) || name == nullptr) return -1;
  WorkspaceView w;
  Placer<FindName> v{nullptr, {name, index}};
  workspace_regions(make_dims(cfg, N, E, B), w, v);
  return v.note.found;
}

int cgr_graph_prep(const cgr_gnn_config* cfg, const cgr_batch* b, void* arena, void* stream) {
  clear_stale_hip_error();
  int rc = validate_config(cfg);
  if (rc) return rc;
  rc = validate_batch(cfg, b);
  if (rc) return rc;
  CGR_CHECK(arena != nullptr, "cgr: arena is NULL");
  const Dims d = make_dims(cfg, b->num_nodes, b->num_edges, b->num_graphs);
  const ArenaView av = arena_view(d, false, arena);
  PrepArgs pa{b->edge_index, b->batch, b->graph_ptr, b->edge_attr, d.N, d.E, d.B,
              d.Fe,          d.Fep,   av.idx,       av.flt.e_s};
  return cgr_graph_prep_impl(pa, (hipStream_t)stream);
}

// the ffn entries of a parameter / gradient table: NULL allowed below the fused level (the
// encode and encode_nodes calls)
static bool is_ffn_entry(const cgr_gnn_config* cfg, int i) {
  return i == CGR_PARAM_FFN_W(cfg->depth) || i == CGR_PARAM_FFN_B(cfg->depth);
}

// cgr_gnn_forward (y [B]) / cgr_gnn_encode (out = g_out [B, H]) / cgr_gnn_encode_nodes (out =
// n_out [N, H])
static int forward_entry(OutLevel level, const cgr_gnn_config* cfg, const float* const* params,
                         const cgr_batch* b, const float* dropout_p, uint64_t seed,
                         uint64_t* rng_counter, int32_t training, void* arena, float* out,
                         void* stream) {
  clear_stale_hip_error();
  int rc = validate_config(cfg);
  if (rc) return rc;
  rc = validate_batch(cfg, b);
  if (rc) return rc;
  const bool headless = level != OutLevel::Fused;
  CGR_CHECK(params != nullptr && arena != nullptr && out != nullptr,
            std::string("cgr: params / arena / ") + calls_of(level).out + " must not be NULL");
  CGR_CHECK((training & ~(CGR_TRAIN_DROPOUT | CGR_TRAIN_FOR_BACKWARD)) == 0,
            "cgr: unknown `training` bits (CGR_TRAIN_DROPOUT | CGR_TRAIN_FOR_BACKWARD)");
  const int np = cgr_gnn_num_params(cfg);
  for (int i = 0; i < np; ++i)
    CGR_CHECK(params[i] != nullptr || (headless && is_ffn_entry(cfg, i)),
              "cgr: NULL parameter pointer");
  const Dims d = make_dims(cfg, b->num_nodes, b->num_edges, b->num_graphs);
  g_arenas.note_forward(arena, -1);  // not usable by a backward unless the forward below succeeds
  FwdMode m;
  m.level = level;
  const int r = gnn_forward_impl(d, params, b, dropout_p, seed, rng_counter, training, arena, out,
                                 (hipStream_t)stream, m);
  if (r == 0) g_arenas.note_forward(arena, training, cfg->precision, level);
  return r;
}

int cgr_gnn_forward(const cgr_gnn_config* cfg, const float* const* params, const cgr_batch* b,
                    const float* dropout_p, uint64_t seed, uint64_t* rng_counter,
                    int32_t training, void* arena, float* y, void* stream) {
  return forward_entry(OutLevel::Fused, cfg, params, b, dropout_p, seed, rng_counter, training,
                       arena, y, stream);
}

int cgr_gnn_encode(const cgr_gnn_config* cfg, const float* const* params, const cgr_batch* b,
                   const float* dropout_p, uint64_t seed, uint64_t* rng_counter, int32_t training,
                   void* arena, float* g_out, void* stream) {
  return forward_entry(OutLevel::Pooled, cfg, params, b, dropout_p, seed, rng_counter, training,
                       arena, g_out, stream);
}

int cgr_gnn_encode_nodes(const cgr_gnn_config* cfg, const float* const* params,
                         const cgr_batch* b, const float* dropout_p, uint64_t seed,
                         uint64_t* rng_counter, int32_t training, void* arena, float* n_out,
                         void* stream) {
  return forward_entry(OutLevel::Nodes, cfg, params, b, dropout_p, seed, rng_counter, training,
                       arena, n_out, stream);
}

// cgr_gnn_backward (up = dy [B]) / cgr_gnn_encode_backward (up = dg [B, H]) /
// cgr_gnn_encode_nodes_backward (up = dn [N, H])
static int backward_entry(OutLevel level, const cgr_gnn_config* cfg, const float* const* params,
                          const cgr_batch* b, const float* dropout_p, uint64_t seed,
                          int32_t training, const void* arena, const float* up,
                          float* const* grads, void* workspace, void* const* bucket_events,
                          void* stream) {
  const bool headless = level != OutLevel::Fused;
  const std::string fn = calls_of(level).bwd, fwd = calls_of(level).fwd;
  clear_stale_hip_error();
  int rc = validate_config(cfg);
  if (rc) return rc;
  rc = validate_batch(cfg, b);
  if (rc) return rc;
  CGR_CHECK(params != nullptr && arena != nullptr && up != nullptr && grads != nullptr &&
                workspace != nullptr,
            std::string("cgr: params / arena / ") + calls_of(level).up +
                " / grads / workspace must not be NULL");
  CGR_CHECK((training & ~(CGR_TRAIN_DROPOUT | CGR_TRAIN_FOR_BACKWARD)) == 0,
            "cgr: unknown `training` bits (CGR_TRAIN_DROPOUT | CGR_TRAIN_FOR_BACKWARD)");
  const ArenaBook::Seen seen = g_arenas.seen(arena, workspace);
  const int ff = seen.flags;
  CGR_CHECK(ff >= 0 && (ff & CGR_TRAIN_FOR_BACKWARD),
            fn + ": `arena` was not filled by a successful " + fwd + " with "
            "CGR_TRAIN_FOR_BACKWARD set");
  const LevelCalls& own = calls_of(seen.level);  // the arena's own calls
  CGR_CHECK(seen.level == level,
            fn + ": `arena` was filled by " + own.fwd + " (" + own.what + "); its backward is " +
                own.bwd);
  CGR_CHECK((ff & CGR_TRAIN_DROPOUT) == (training & CGR_TRAIN_DROPOUT),
            fn + ": `training` dropout bit differs from the forward's");
  CGR_CHECK(seen.mode == cfg->precision,
            fn + ": the config's precision differs from the mode `arena`'s forward "
            "ran in");
  const int np = cgr_gnn_num_params(cfg);
  for (int i = 0; i < np; ++i) {
    if (headless && is_ffn_entry(cfg, i)) continue;  // never read or written
    CGR_CHECK(params[i] != nullptr, "cgr: NULL parameter pointer");
    CGR_CHECK(grads[i] != nullptr, "cgr: NULL gradient pointer");
  }
  const Dims d = make_dims(cfg, b->num_nodes, b->num_edges, b->num_graphs);
  if (bucket_events)
    for (int i = 0; i < CGR_GRAD_BUCKETS(cfg->depth); ++i)
      CGR_CHECK(bucket_events[i] != nullptr, fn + ": NULL bucket event");
  const int r = gnn_backward_impl(d, params, b, dropout_p, seed, training, arena, up, grads,
                                  workspace, reinterpret_cast<hipEvent_t const*>(bucket_events),
                                  (hipStream_t)stream, level);
  if (r == 0) g_arenas.note_backward(arena, workspace);
  return r;
}

int cgr_gnn_backward(const cgr_gnn_config* cfg, const float* const* params, const cgr_batch* b,
                     const float* dropout_p, uint64_t seed, int32_t training, const void* arena,
                     const float* dy, float* const* grads, void* workspace,
                     void* const* bucket_events, void* stream) {
  return backward_entry(OutLevel::Fused, cfg, params, b, dropout_p, seed, training, arena, dy,
                        grads, workspace, bucket_events, stream);
}

int cgr_gnn_encode_backward(const cgr_gnn_config* cfg, const float* const* params,
                            const cgr_batch* b, const float* dropout_p, uint64_t seed,
                            int32_t training, const void* arena, const float* dg,
                            float* const* grads, void* workspace, void* const* bucket_events,
                            void* stream) {
  return backward_entry(OutLevel::Pooled, cfg, params, b, dropout_p, seed, training, arena, dg,
                        grads, workspace, bucket_events, stream);
}

int cgr_gnn_encode_nodes_backward(const cgr_gnn_config* cfg, const float* const* params,
                                  const cgr_batch* b, const float* dropout_p, uint64_t seed,
                                  int32_t training, const void* arena, const float* dn,
                                  float* const* grads, void* workspace,
                                  void* const* bucket_events, void* stream) {
  return backward_entry(OutLevel::Nodes, cfg, params, b, dropout_p, seed, training, arena, dn,
                        grads, workspace, bucket_events, stream);
}

// cgr_gnn_input_grads (up = dy [B]) / cgr_gnn_encode_input_grads (up = dg [B, H]) /
// cgr_gnn_encode_nodes_input_grads (up = dn [N, H])
static int input_grads_entry(OutLevel level, const cgr_gnn_config* cfg,
                             const float* const* params, const cgr_batch* b, const void* arena,
                             const float* up, void* workspace, float* dx, float* dedge_attr,
                             void* stream) {
  const bool headless = level != OutLevel::Fused;
  const std::string fn = calls_of(level).igr, fwd = calls_of(level).fwd,
                    bwd = calls_of(level).bwd;
  clear_stale_hip_error();
  int rc = validate_config(cfg);
  if (rc) return rc;
  rc = validate_batch(cfg, b);
  if (rc) return rc;
  CGR_CHECK(params != nullptr && arena != nullptr && up != nullptr && workspace != nullptr,
            std::string("cgr: params / arena / ") + calls_of(level).up +
                " / workspace must not be NULL");
  const ArenaBook::Seen seen = g_arenas.seen(arena, workspace);
  const int ff = seen.flags;
  CGR_CHECK(ff >= 0 && (ff & CGR_TRAIN_FOR_BACKWARD),
            fn + ": `arena` was not filled by a successful " + fwd + " with "
            "CGR_TRAIN_FOR_BACKWARD set");
  const LevelCalls& own = calls_of(seen.level);  // the arena's own calls
  CGR_CHECK(seen.level == level,
            fn + ": `arena` was filled by " + own.fwd + " (" + own.what +
                "); its input gradients are " + own.igr);
  CGR_CHECK(seen.mode == cfg->precision,
            fn + ": the config's precision differs from the mode `arena`'s forward "
            "ran in");
  CGR_CHECK(seen.backward_here,
            fn + ": `workspace` does not hold a " + bwd + " of this `arena`'s "
            "latest forward (run the backward first, with the same arena and workspace)");
  CGR_CHECK(((uintptr_t)dx & 15) == 0 && ((uintptr_t)dedge_attr & 15) == 0,
            fn + ": dx / dedge_attr must be 16-byte aligned (or NULL)");
  const int np = cgr_gnn_num_params(cfg);
  for (int i = 0; i < np; ++i)
    CGR_CHECK(params[i] != nullptr || (headless && is_ffn_entry(cfg, i)),
              "cgr: NULL parameter pointer");
  const Dims d = make_dims(cfg, b->num_nodes, b->num_edges, b->num_graphs);
  return gnn_input_grads_impl(d, params, arena, up, workspace, dx, dedge_attr,
                              (hipStream_t)stream, level);
}

int cgr_gnn_input_grads(const cgr_gnn_config* cfg, const float* const* params,
                        const cgr_batch* b, const void* arena, const float* dy, void* workspace,
                        float* dx, float* dedge_attr, void* stream) {
  return input_grads_entry(OutLevel::Fused, cfg, params, b, arena, dy, workspace, dx,
                           dedge_attr, stream);
}

int cgr_gnn_encode_input_grads(const cgr_gnn_config* cfg, const float* const* params,
                               const cgr_batch* b, const void* arena, const float* dg,
                               void* workspace, float* dx, float* dedge_attr, void* stream) {
  return input_grads_entry(OutLevel::Pooled, cfg, params, b, arena, dg, workspace, dx,
                           dedge_attr, stream);
}

int cgr_gnn_encode_nodes_input_grads(const cgr_gnn_config* cfg, const float* const* params,
                                     const cgr_batch* b, const void* arena, const float* dn,
                                     void* workspace, float* dx, float* dedge_attr,
                                     void* stream) {
  return input_grads_entry(OutLevel::Nodes, cfg, params, b, arena, dn, workspace, dx, dedge_attr,
                           stream);
}

int64_t cgr_gnn_image_bytes(const cgr_gnn_config* cfg) {
  if (validate_config(cfg)) return -1;
  Images im;
  Placer<> v;
  return (int64_t)image_buffer_regions(make_dims(cfg, 1, 2, 1), im, v);
}

int cgr_gnn_pack_images(const cgr_gnn_config* cfg, const float* const* params, void* images,
                        void* stream) {
  clear_stale_hip_error();
  int rc = validate_config(cfg);
  if (rc) return rc;
  CGR_CHECK(params != nullptr && images != nullptr, "cgr: params / images must not be NULL");
  const int np = cgr_gnn_num_params(cfg);
  for (int i = 0; i < np; ++i) CGR_CHECK(params[i] != nullptr, "cgr: NULL parameter pointer");
  const Dims d = make_dims(cfg, 1, 2, 1);
  HIP_RET(pack_forward_images(d, params, image_view(d, images), (hipStream_t)stream));
  return 0;
}

int64_t cgr_gnn_predict_arena_bytes(const cgr_gnn_config* cfg, int64_t N, int64_t E, int64_t B) {
  if (validate_config(cfg)) return -1;
  ArenaView a;
  Placer<> v;
  return (int64_t)eval_regions(make_dims(cfg, N, E, B), a, v);
}

// cgr_gnn_predict (y [B]) / cgr_gnn_encode_predict (out = g_out [B, H]) /
// cgr_gnn_encode_nodes_predict (out = n_out [N, H])
static int predict_entry(OutLevel level, const cgr_gnn_config* cfg, const float* const* params,
                         const cgr_batch* b, const float* dropout_p, uint64_t seed,
                         uint64_t* rng_counter, int32_t training, const void* images,
                         void* arena, float* out, void* stream) {
  clear_stale_hip_error();
  int rc = validate_config(cfg);
  if (rc) return rc;
  rc = validate_batch(cfg, b);
  if (rc) return rc;
  const bool headless = level != OutLevel::Fused;
  CGR_CHECK(params != nullptr && arena != nullptr && out != nullptr,
            std::string("cgr: params / arena / ") + calls_of(level).out + " must not be NULL");
  CGR_CHECK((training & ~CGR_TRAIN_DROPOUT) == 0,
            std::string(calls_of(level).pred) +
                ": `training` may only hold CGR_TRAIN_DROPOUT (no backward follows)");
  const int np = cgr_gnn_num_params(cfg);
  for (int i = 0; i < np; ++i)
    CGR_CHECK(params[i] != nullptr || (headless && is_ffn_entry(cfg, i)),
              "cgr: NULL parameter pointer");
  const Dims d = make_dims(cfg, b->num_nodes, b->num_edges, b->num_graphs);
  FwdMode m;
  m.eval = true;
  m.images = images;
  m.level = level;
  g_arenas.note_forward(arena, -1);  // never a backward's arena
  return gnn_forward_impl(d, params, b, dropout_p, seed, rng_counter, training, arena, out,
                          (hipStream_t)stream, m);
}

int cgr_gnn_predict(const cgr_gnn_config* cfg, const float* const* params, const cgr_batch* b,
                    const float* dropout_p, uint64_t seed, uint64_t* rng_counter,
                    int32_t training, const void* images, void* arena, float* y, void* stream) {
  return predict_entry(OutLevel::Fused, cfg, params, b, dropout_p, seed, rng_counter, training,
                       images, arena, y, stream);
}

int cgr_gnn_encode_predict(const cgr_gnn_config* cfg, const float* const* params,
                           const cgr_batch* b, const float* dropout_p, uint64_t seed,
                           uint64_t* rng_counter, int32_t training, const void* images,
                           void* arena, float* g_out, void* stream) {
  return predict_entry(OutLevel::Pooled, cfg, params, b, dropout_p, seed, rng_counter, training,
                       images, arena, g_out, stream);
}

int cgr_gnn_encode_nodes_predict(const cgr_gnn_config* cfg, const float* const* params,
                                 const cgr_batch* b, const float* dropout_p, uint64_t seed,
                                 uint64_t* rng_counter, int32_t training, const void* images,
                                 void* arena, float* n_out, void* stream) {
  return predict_entry(OutLevel::Nodes, cfg, params, b, dropout_p, seed, rng_counter, training,
                       images, arena, n_out, stream);
}

int32_t cgr_device_errors(int32_t device, int32_t clear) {
  SideStreams* ss = side_streams_of(device);
  if (!ss || !ss->err_host) return 0;
  volatile int* w = ss->err_host;
  int32_t bits = 0;
  if (w[kDevErrUnpairedTimeout]) bits |= CGR_DEVERR_UNPAIRED_TIMEOUT;
  if (w[kDevErrUnpairedSeen]) bits |= CGR_DEVERR_UNPAIRED_SEEN;
  if (clear) {
    if (bits & CGR_DEVERR_UNPAIRED_TIMEOUT) w[kDevErrUnpairedTimeout] = 0;
    if (bits & CGR_DEVERR_UNPAIRED_SEEN) w[kDevErrUnpairedSeen] = 0;
  }
  return bits;
}

int cgr_segment_sum(const float* values, int64_t ld_values, const int32_t* index,
                    const int32_t* seg_ptr, int64_t num_segments, int64_t width, float* out,
                    int64_t ld_out, void* stream) {
  clear_stale_hip_error();
  CGR_CHECK(values != nullptr && seg_ptr != nullptr && out != nullptr,
            "cgr_segment_sum: NULL pointer");
  CGR_CHECK(num_segments >= 0 && width >= 0 && ld_values >= width && ld_out >= width,
            "cgr_segment_sum: bad sizes");
  HIP_RET(segment_sum(values, ld_values, index, seg_ptr, num_segments, width, out, ld_out,
                      (hipStream_t)stream));
  return 0;
}

// what the attention-pool pair shares: sizes, the segment source, the pointers both read
static int attn_pool_check(const char* what, const float* x, int64_t ldx, int64_t N, int64_t H,
                           const int64_t* batch, const int64_t* ptr, int64_t B,
                           const float* weight) {
  const std::string w(what);
  CGR_CHECK(H > 0 && H < (1ll << 30), w + ": H must be >= 1");
  CGR_CHECK(ldx >= H, w + ": ldx < H");
  CGR_CHECK(N >= 0 && N < (1ll << 31) && B >= 0 && B < (1ll << 31), w + ": N or B out of range");
  CGR_CHECK(B <= 1 || batch != nullptr || ptr != nullptr,
            w + ": B > 1 needs batch or ptr (neither = one graph)");
  CGR_CHECK(weight != nullptr && (N == 0 || x != nullptr), w + ": NULL pointer");
  return 0;
}

int64_t cgr_attention_pool_workspace_bytes(int64_t B, int64_t H) {
  if (B < 0 || H <= 0 || B >= (1ll << 31) || H >= (1ll << 30)) return -1;
  return B * round_up(H, 4) * (int64_t)sizeof(float);
}

int cgr_attention_pool_forward(const float* x, int64_t ldx, int64_t N, int64_t H,
                               const int64_t* batch, const int64_t* ptr, int64_t B,
                               const float* weight, const float* bias, const uint8_t* mask,
                               float* g, float* alpha, void* stream) {
  clear_stale_hip_error();
  const int rc = attn_pool_check("cgr_attention_pool_forward", x, ldx, N, H, batch, ptr, B, weight);
  if (rc) return rc;
  CGR_CHECK((B == 0 || g != nullptr) && (N == 0 || alpha != nullptr),
            "cgr_attention_pool_forward: NULL pointer");
  HIP_RET(attn_pool_fwd(x, ldx, N, (int)H, batch, ptr, B, weight, bias, mask, g, alpha,
                        (hipStream_t)stream));
  return 0;
}

int cgr_attention_pool_backward(const float* x, int64_t ldx, int64_t N, int64_t H,
                                const int64_t* batch, const int64_t* ptr, int64_t B,
                                const float* weight, const float* alpha, const float* dg,
                                float* dx, float* dw, void* workspace, void* stream) {
  clear_stale_hip_error();
  const int rc =
      attn_pool_check("cgr_attention_pool_backward", x, ldx, N, H, batch, ptr, B, weight);
  if (rc) return rc;
  CGR_CHECK((B == 0 || dg != nullptr) && (N == 0 || alpha != nullptr),
            "cgr_attention_pool_backward: NULL pointer");
  CGR_CHECK(dw == nullptr || B == 0 ||
                (workspace != nullptr && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0),
            "cgr_attention_pool_backward: dw needs a 16-byte aligned workspace "
            "(cgr_attention_pool_workspace_bytes)");
  if (B == 0 && dw)  // no graph: the sum over none
    HIP_RET(hipMemsetAsync(dw, 0, (size_t)H * sizeof(float), (hipStream_t)stream));
  HIP_RET(attn_pool_bwd(x, ldx, N, (int)H, batch, ptr, B, weight, alpha, dg, dx, dw,
                        static_cast<float*>(workspace), (hipStream_t)stream));
  return 0;
}

}  // extern "C"
