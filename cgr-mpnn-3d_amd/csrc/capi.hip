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
hipError_t pack_forward_images(const Dims& d, const float* const* params, const ImageLayout& IL,
                               void* images, hipStream_t st);
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

int bwd_seg_tiles(const Dims& d);

namespace {
struct Bump {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off = (size_t)round_up((int64_t)(off + bytes), (int64_t)kAlign);
    return o;
  }
};
constexpr size_t kNone = (size_t)-1;
}  // namespace

// index bookkeeping, sorted edge features and the x-GEMM outputs: shared by both layouts
static void layout_prefix(const Dims& d, ArenaLayout& L, Bump& b) {
  const size_t N = (size_t)d.N, E = (size_t)d.E, B = (size_t)d.B, Hp = (size_t)d.Hp;
  // zero block: six int arrays back to back, padded to a multiple of 16 bytes
  L.zero_block = b.off;
  L.deg_dst = b.off;
  L.deg_src = L.deg_dst + 4 * N;
  L.cursor = L.deg_src + 4 * N;
  L.cursor2 = L.cursor + 4 * N;
  L.graph_cnt = L.cursor2 + 4 * N;
  L.status = L.graph_cnt + 4 * B;
  // + the ticket counters of the layer GEMMs' hub segments (EpLayerSeg, ep_fwd.hpp: zero on entry, reset by
  // each completer)
  L.fcnt = L.status + 16;
  // the layer forward runs in layer_cols(d), or in image_cols(d, H) over caller-packed images
  // (predict)
  const B3Cols lc = layer_cols(d), dc = image_cols(d, d.H);
  const size_t fcnt_n = N * (size_t)std::max(lc.tiles, dc.tiles);
  L.zero_bytes = (size_t)round_up((int64_t)(4 * (4 * N + B) + 16 + 4 * fcnt_n), 16);
  b.take(L.zero_bytes);
  L.rng = b.take(8);
  L.perm = b.take(4 * E);
  L.src_s = b.take(4 * E);
  L.dst_s = b.take(4 * E);
  L.rev_s = b.take(4 * E);
  L.src_list = b.take(4 * E);
  L.inv = b.take(4 * E);
  L.src_c = b.take(4 * E);
  L.dst_c = b.take(4 * E);
  L.dst_ptr = b.take(4 * (N + 1));
  L.src_ptr = b.take(4 * (N + 1));
  L.graph_ptr = b.take(4 * (B + 1));
  L.node_graph = b.take(4 * N);
  L.e_s = d.Fep ? b.take(4 * E * (size_t)d.Fep) : kNone;
  L.w0eT = d.Fe ? b.take(4 * (size_t)d.Fe * Hp) : kNone;
  L.P = b.take(4 * N * Hp);
  L.Q = b.take(4 * N * Hp);
  L.xp = (d.F % 4 != 0) ? b.take(4 * N * (size_t)d.Fp) : kNone;
  L.inv_deg = d.aggr == CGR_AGGR_MEAN ? b.take(4 * N) : kNone;
  L.inv_cnt = d.pool == CGR_POOL_MEAN ? b.take(4 * B) : kNone;
  L.pool_arg = d.pool == CGR_POOL_MAX ? b.take(4 * B * Hp) : kNone;
  // partial sums of the layer GEMMs' hub segments (over >= 3 row tiles), one slot pair per tile
  const size_t rt = (size_t)cdiv(d.E, b3nt_rows((int)d.E, d.H));
  L.fpart = b.take(4 * rt * 2 * 16 *
                   std::max((size_t)lc.tiles * lc.nf, (size_t)dc.tiles * dc.nf));
}

ArenaLayout arena_layout(const Dims& d) {
  ArenaLayout L;
  memset(&L, 0xff, sizeof(L));
  Bump b;
  const size_t N = (size_t)d.N, E = (size_t)d.E, B = (size_t)d.B, Hp = (size_t)d.Hp;
  layout_prefix(d, L, b);
  L.b3x = d.F > 0 ? b.take(16 * b3_img_u4(x_cols(d), d.F)) : kNone;
  // the node-row readout GEMMs in their grid-filling column tiling (readout_cols)
  const B3Cols rc = readout_cols(d);
  L.b3rof = b.take(16 * b3_img_u4(rc, d.H));
  L.b3rob = b.take(16 * b3_img_u4(rc, d.H));
  for (int l = 0; l < d.D; ++l) {
    L.b3lf[l] = b.take(16 * b3_img_u4(layer_cols(d), d.H));
    L.b3lb[l] = b.take(16 * b3_img_u4(layer_cols(d), d.H));
  }
  for (int l = 0; l <= CGR_MAX_DEPTH; ++l) {
    L.h[l] = l <= d.D ? b.take(4 * E * Hp) : kNone;
    L.a[l] = l <= d.D ? b.take(4 * N * Hp) : kNone;
    L.pre[l] = (l <= d.D && d.act != CGR_ACT_RELU) ? b.take(4 * E * Hp) : kNone;
  }
  L.zn = d.act != CGR_ACT_RELU ? b.take(4 * N * Hp) : kNone;
  L.hn = b.take(4 * N * Hp);
  L.g = b.take(4 * B * Hp);
  L.bytes = b.off;
  L.off_index_begin = 0;
  return L;
}

ArenaLayout eval_arena_layout(const Dims& d) {
  ArenaLayout L;
  memset(&L, 0xff, sizeof(L));
  Bump b;
  const size_t N = (size_t)d.N, E = (size_t)d.E, B = (size_t)d.B, Hp = (size_t)d.Hp;
  layout_prefix(d, L, b);
  const size_t h0 = b.take(4 * E * Hp);
  const size_t hr[2] = {d.D >= 2 ? b.take(4 * E * Hp) : kNone, b.take(4 * E * Hp)};
  const size_t ar[3] = {b.take(4 * N * Hp), b.take(4 * N * Hp),
                        d.D >= 2 ? b.take(4 * N * Hp) : kNone};
  for (int l = 0; l <= CGR_MAX_DEPTH; ++l) {
    L.h[l] = l > d.D ? kNone : (l == 0 ? h0 : hr[l & 1]);
    L.a[l] = l > d.D ? kNone : ar[l % 3];
  }
  L.hn = b.take(4 * N * Hp);
  L.g = b.take(4 * B * Hp);
  // forward weight images, packed by every predict that is not handed pre-packed ones
  L.b3x = d.F > 0 ? b.take(16 * b3_img_u4(x_cols(d), d.F)) : kNone;
  L.b3rof = b.take(16 * b3_img_u4(readout_cols(d), d.H));
  for (int l = 0; l < d.D; ++l) L.b3lf[l] = b.take(16 * b3_img_u4(layer_cols(d), d.H));
  L.bytes = b.off;
  L.off_index_begin = 0;
  return L;
}

ImageLayout image_layout(const Dims& d) {
  ImageLayout I;
  Bump b;
  const B3Cols cx = image_cols(d, 2 * d.H), ch = image_cols(d, d.H);
  I.b3x = d.F > 0 ? b.take(16 * b3_img_u4(cx, d.F)) : kNone;
  I.b3rof = b.take(16 * b3_img_u4(ch, d.H));
  for (int l = 0; l < CGR_MAX_DEPTH; ++l) I.b3lf[l] = l < d.D ? b.take(16 * b3_img_u4(ch, d.H)) : kNone;
  I.bytes = b.off;
  return I;
}

static inline void* at(void* base, size_t off) {
  return off == kNone ? nullptr : static_cast<char*>(base) + off;
}

IndexView index_view(void* arena, const ArenaLayout& L) {
  IndexView v;
  v.deg_dst = (int*)at(arena, L.deg_dst);
  v.deg_src = (int*)at(arena, L.deg_src);
  v.cursor = (int*)at(arena, L.cursor);
  v.cursor2 = (int*)at(arena, L.cursor2);
  v.graph_cnt = (int*)at(arena, L.graph_cnt);
  v.status = (int*)at(arena, L.status);
  v.fcnt = (int*)at(arena, L.fcnt);
  v.fpart = (float*)at(arena, L.fpart);
  v.rng = (uint64_t*)at(arena, L.rng);
  v.zero_block = at(arena, L.zero_block);
  v.zero_bytes = L.zero_bytes;
  v.perm = (int*)at(arena, L.perm);
  v.src_s = (int*)at(arena, L.src_s);
  v.dst_s = (int*)at(arena, L.dst_s);
  v.rev_s = (int*)at(arena, L.rev_s);
  v.src_list = (int*)at(arena, L.src_list);
  v.inv = (int*)at(arena, L.inv);
  v.src_c = (int*)at(arena, L.src_c);
  v.dst_c = (int*)at(arena, L.dst_c);
  v.dst_ptr = (int*)at(arena, L.dst_ptr);
  v.src_ptr = (int*)at(arena, L.src_ptr);
  v.graph_ptr = (int*)at(arena, L.graph_ptr);
  v.node_graph = (int*)at(arena, L.node_graph);
  return v;
}

FloatView float_view(void* arena, const ArenaLayout& L, const Dims& d) {
  FloatView f;
  f.e_s = (float*)at(arena, L.e_s);
  f.w0eT = (float*)at(arena, L.w0eT);
  f.P = (float*)at(arena, L.P);
  f.Q = (float*)at(arena, L.Q);
  f.xp = (float*)at(arena, L.xp);
  f.inv_deg = (float*)at(arena, L.inv_deg);
  f.inv_cnt = (float*)at(arena, L.inv_cnt);
  f.pool_arg = (int*)at(arena, L.pool_arg);
  for (int l = 0; l <= CGR_MAX_DEPTH; ++l) {
    f.h[l] = (float*)at(arena, L.h[l]);
    f.a[l] = (float*)at(arena, L.a[l]);
    f.pre[l] = (float*)at(arena, L.pre[l]);
  }
  f.zn = (float*)at(arena, L.zn);
  f.hn = (float*)at(arena, L.hn);
  f.g = (float*)at(arena, L.g);
  f.b3x = at(arena, L.b3x);
  f.b3rof = at(arena, L.b3rof);
  f.b3rob = at(arena, L.b3rob);
  for (int l = 0; l < CGR_MAX_DEPTH; ++l) {
    f.b3lf[l] = l < d.D ? at(arena, L.b3lf[l]) : nullptr;
    f.b3lb[l] = l < d.D ? at(arena, L.b3lb[l]) : nullptr;
  }
  return f;
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

WorkspaceLayout workspace_layout(const Dims& d) {
  WorkspaceLayout W;
  Bump b;
  const size_t N = (size_t)d.N, E = (size_t)d.E, Hp = (size_t)d.Hp;
  W.dpre = b.take(4 * E * Hp * (size_t)d.D);  // one per layer (gnn_bwd.hip)
  W.dm = b.take(4 * E * Hp);
  W.dh0 = b.take(4 * E * Hp);
  W.dzn = b.take(4 * N * Hp);
  W.ds = b.take(4 * N * Hp);
  W.Gs = b.take(4 * N * Hp);
  // e-images: only where a site lists the split-bf16 family (not in CGR_PRECISION_FP32)
  bool eimg = false;
  for (WgSite s : {WgSite::Readout, WgSite::Layer, WgSite::Node}) {
    const WgCandidates w = wgrad_candidates(s, d);
    for (int i = 0; i < w.n; ++i) eimg = eimg || w.c[i].family == WgFamily::B3;
  }
  W.img_side = b.take(eimg ? b3_eimg_bytes(std::max(d.E, d.N), d.H) : 0);
  W.img_main = b.take(eimg ? b3_eimg_bytes(d.N, d.H) : 0);
  W.img_top = b.take(eimg ? b3_eimg_bytes(d.E, d.H) : 0);
  // split-K slabs: the largest over every family a site may pick for these dims (wgrad.hpp, the
  // table gnn_bwd.hip launches through).  The side-stream weight gradients (readout, layers, edge
  // features) run one after another and share `slab`; the node weight gradient runs beside them
  // on the caller's stream: `slab2`.
  auto fit = [&](WgSite s, size_t* slab, size_t* bslab) {
    const WgCandidates w = wgrad_candidates(s, d);
    for (int i = 0; i < w.n; ++i) {
      *slab = std::max(*slab, w.c[i].slab_elems());
      *bslab = std::max(*bslab, w.c[i].bslab_elems());
    }
  };
  for (WgSite s : {WgSite::Readout, WgSite::Layer, WgSite::Edge})
    fit(s, &W.slab_elems, &W.bslab_elems);
  fit(WgSite::Node, &W.slab2_elems, &W.bslab2_elems);
  W.slab = b.take(4 * std::max<size_t>(W.slab_elems, 1));
  W.bslab = b.take(4 * std::max<size_t>(W.bslab_elems, 1));
  W.slab_b = b.take(4 * std::max<size_t>(W.slab_elems, 1));  // alternating with slab (gnn_bwd.hip)
  W.bslab_b = b.take(4 * std::max<size_t>(W.bslab_elems, 1));
  W.slab2 = b.take(4 * std::max<size_t>(W.slab2_elems, 1));
  W.bslab2 = b.take(4 * std::max<size_t>(W.bslab2_elems, 1));
  W.dag = b.take(2 * 4 * N * Hp);  // two, alternating by layer
  // segment tickets, then one unpaired grid counter per fused layer-backward launch
  W.cnt = b.take(4 * (N * (size_t)layer_cols(d).tiles + CGR_MAX_DEPTH));
  W.part = b.take(4 * (size_t)bwd_seg_tiles(d) * 2 * (size_t)layer_cols(d).nf * 16);
  W.wxT = b.take(4 * (size_t)d.F * (size_t)input_grad_ldw(d.H));
  W.dsig_blocks = bwd_dsig_slots(d);
  W.dsig_part = b.take(4 * (size_t)d.D * (size_t)W.dsig_blocks);
  W.bytes = b.off;
  return W;
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
  return (int64_t)arena_layout(make_dims(cfg, N, E, B)).bytes;
}

int64_t cgr_gnn_workspace_bytes(const cgr_gnn_config* cfg, int64_t N, int64_t E, int64_t B) {
  if (validate_config(cfg)) return -1;
  return (int64_t)workspace_layout(make_dims(cfg, N, E, B)).bytes;
}

int64_t cgr_gnn_arena_offset(const cgr_gnn_config* cfg, int64_t N, int64_t E, int64_t B,
                             const char* name, int32_t index) {
  if (validate_config(cfg) || name == nullptr) return -1;
  const ArenaLayout L = arena_layout(make_dims(cfg, N, E, B));
  size_t o = (size_t)-1;
  const std::string n(name);
  const bool li = index >= 0 && index <= CGR_MAX_DEPTH;
  if (n == "status") o = L.status;
  if (n == "rng") o = L.rng;
  else if (n == "perm") o = L.perm;
  else if (n == "src_s") o = L.src_s;
  else if (n == "dst_s") o = L.dst_s;
  else if (n == "rev_s") o = L.rev_s;
  else if (n == "src_list") o = L.src_list;
  else if (n == "dst_ptr") o = L.dst_ptr;
  else if (n == "src_ptr") o = L.src_ptr;
  else if (n == "graph_ptr") o = L.graph_ptr;
  else if (n == "node_graph") o = L.node_graph;
  else if (n == "e_s") o = L.e_s;
  else if (n == "P") o = L.P;
  else if (n == "Q") o = L.Q;
  else if (n == "h" && li) o = L.h[index];
  else if (n == "a" && li) o = L.a[index];
  else if (n == "pre" && li) o = L.pre[index];
  else if (n == "zn") o = L.zn;
  else if (n == "hn") o = L.hn;
  else if (n == "g") o = L.g;
  return o == (size_t)-1 ? -1 : (int64_t)o;
}

int64_t cgr_gnn_workspace_offset(const cgr_gnn_config* cfg, int64_t N, int64_t E, int64_t B,
                                 const char* name, int32_t index) {
  if (validate_config(cfg) || name == nullptr) return -1;
  const Dims d = make_dims(cfg, N, E, B);
  const WorkspaceLayout W = workspace_layout(d);
  const std::string n(name);
  // only what gnn_backward_impl leaves complete in fp32 on every path (gnn_bwd.hip): dzn and Gs
  // exist as e-images alone on the split-bf16 paths, dm holds hand-off rows only
  if (n == "dpre" && index >= 0 && index < d.D)
    return (int64_t)(W.dpre + (size_t)index * 4 * (size_t)d.E * (size_t)d.Hp);
  if (n == "dpre0") return (int64_t)W.dh0;
  if (n == "ds") return (int64_t)W.ds;
  // "dzn_main": dzn [N, Hp] where the backward materialises it in fp32 on the caller's stream for
  // the readout NT -- below the fused level (cgr_gnn_encode_backward,
  // cgr_gnn_encode_nodes_backward) and under max pooling.  ("dzn" stays unknown: the fused add /
  // mean backward on the split-bf16 path never stores it.)
  if (n == "dzn_main") return (int64_t)W.dzn;
  return -1;
}

int cgr_graph_prep(const cgr_gnn_config* cfg, const cgr_batch* b, void* arena, void* stream) {
  clear_stale_hip_error();
  int rc = validate_config(cfg);
  if (rc) return rc;
  rc = validate_batch(cfg, b);
  if (rc) return rc;
  CGR_CHECK(arena != nullptr, "cgr: arena is NULL");
  const Dims d = make_dims(cfg, b->num_nodes, b->num_edges, b->num_graphs);
  const ArenaLayout L = arena_layout(d);
  const FloatView fv = float_view(arena, L, d);
  PrepArgs pa{b->edge_index, b->batch, b->graph_ptr, b->edge_attr, d.N, d.E, d.B,
              d.Fe,          d.Fep,   index_view(arena, L), fv.e_s};
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
  return (int64_t)image_layout(make_dims(cfg, 1, 2, 1)).bytes;
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
  HIP_RET(pack_forward_images(d, params, image_layout(d), images, (hipStream_t)stream));
  return 0;
}

int64_t cgr_gnn_predict_arena_bytes(const cgr_gnn_config* cfg, int64_t N, int64_t E, int64_t B) {
  if (validate_config(cfg)) return -1;
  return (int64_t)eval_arena_layout(make_dims(cfg, N, E, B)).bytes;
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

}  // extern "C"
