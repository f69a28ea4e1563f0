// Reverse mode of gnn_fwd.hip (the math is restated and pinned in
// oracle/dmpnn_numpy.py::backward).  Same gather -> MFMA GEMM -> segmented-reduce pattern as the
// forward with src and dst swapped; weight gradients are split-K TN GEMMs over the edge / node
// dimension reduced deterministically; the only atomics add the two partial sums of a segment
// that crosses a row tile onto zero (order-independent), so gradients are bitwise stable.
//
//   dwf = dy^T g ; dbf = sum dy ; dzn = dy[graph(v)] wf * act'(zn)        (ffn, pool, edge_to_node)
//   dW_n = dzn^T [x | s], db_n = colsum(dzn), ds = dzn W_n[:, F:]
//   dh_D = ds[dst]
//   for l = D-1 .. 0:
//     dpre_l = dh_{l+1} * mask * act'(pre_l) ; ds_l = sum dpre_l*h0
//     dW_l = dpre^T (a_l[src] - h_l[rev])  (message recomputed, never stored) ; db_l = colsum
//     dm = dpre W_l ; da = segsum_src(dm) ; dh_l = da[dst] - dm[rev] -> the next lower layer's
//     dpre, all in the dm GEMM's epilogue (EpLayerBwdSeg, ep_bwd.hpp: rows gathered through rev
//     so each dst segment's rows are the dm rows its node sums; dm and da never stored; segments
//     that cross a row tile completed in the same launch by their last contributor)
//   dh0 = sum_l s_l dpre_l (every layer's skip term) ; dpre0 = (dh0 + dh_0) * act'(pre0)
//   dW0[:, F:] = dpre0^T e ; db0 = colsum(dpre0) ; dW0[:, :F] = (segsum_src dpre0)^T x
//
// Streams: the critical path is act_bwd -> the fused dm GEMM per layer.
// Every weight-gradient TN GEMM (+ its slab reduction) only feeds the gradient outputs, so it runs
// on the side stream, forked right after its input is produced; every layer's dpre has a buffer
// of its own (the edge-init backward sums them into dh0), so the main stream waits for the side
// stream only at the very end.
//
// Weight gradients: wgrad.hpp's wgrad_pick says which TN family runs a site and with which plan
// (the table workspace_regions, capi.hip, sized the slabs from); each site names its operands once
// per family form and calls the `wgrad` helper below (slab check, launch, split-K reduction).
#include "dispatch.hpp"
#include "ep_bwd.hpp"
#include "epilogues.hpp"
#include "gnn_internal.hpp"
#include "kernels.hpp"
#include "profiling.hpp"
#include "streams.hpp"

namespace cgr {

// profile class of a weight gradient: the plain name for the split-bf16 e-image TN, "<name>[tnr]" /
// "<name>[f32]" for the fp32 families, so the family is visible in the per-class report (tests
// assert which family ran for a width, bench.py keys its roofline on the plain names)
static const char* wgrad_class(WgSite s, WgFamily f) {
#define CGR_WG_CLASS(name) {name, name "[tnr]", name "[f32]"}
  static const char* const cls[4][3] = {
      CGR_WG_CLASS("gemm_tn_wgrad_readout"), CGR_WG_CLASS("gemm_tn_wgrad_layer"),
      CGR_WG_CLASS("gemm_tn_wgrad_node"), CGR_WG_CLASS("gemm_tn_wgrad_edge")};
#undef CGR_WG_CLASS
  return cls[(int)s][(int)f];
}

// where a weight gradient's reduced slabs go (reduce_slabs, kernels.hpp): w[n, col_off + k] and
// bias[n] (nullptr: no bias sums wanted), the slab's pad columns [gap_at, gap_at + gap_len) skipped
struct WgDst {
  float* w;
  int64_t ld, col_off;
  float* bias;
  int gap_at = 0, gap_len = 0;
};

// a split-K reduction waiting for its launch: folded into the next side-stream split-bf16 TN
// (the launch-boundary reduce), or launched on its own (flush) before anything that would
// overwrite its slabs; its gradient bucket's event is recorded once it has run
struct PendingReduce {
  RedJob job{};  // job.slab == nullptr: none
  int bucket = -1;
};
int gnn_backward_impl(const Dims& d, const float* const* params, const cgr_batch* b,
                      const float* dropout_p, uint64_t seed, int training, const void* arena,
                      const float* dy, float* const* grads, void* workspace,
                      hipEvent_t const* bucket_events, hipStream_t st, OutLevel level) {
  const ArenaView av = arena_view(d, false, const_cast<void*>(arena));
  const IndexView& iv = av.idx;
  const FloatView& fv = av.flt;
  const WorkspaceView ws = workspace_view(d, workspace);
  // ws.slab / ws.bslab, the side stream's slab buffers, alternate: a TN writes one while the
  // previous weight gradient's slabs in the other are reduced in its prologue
  int sb = 0;  // buffer of the next side-stream TN
  // partial sums of tile-crossing segments, accumulated by layer l's fused backward GEMM: two
  // buffers, alternating by layer (a segment's completer zeroes its entries of the next one)
  auto dag_of = [&](int l) { return ws.dag + (l & 1) * (int64_t)d.N * d.Hp; };

  const int N = (int)d.N, E = (int)d.E, H = d.H, Hp = d.Hp, F = d.F, Fe = d.Fe, D = d.D;
  // dpre of layer l: a buffer per layer, so that writing dpre_{l-1} never waits for the side
  // stream's weight gradient of layer l+1 (a cross-queue edge on the critical chain of a
  // captured step: ~5 us each)
  auto dpre = [&](int l) { return ws.dpre + (int64_t)l * E * Hp; };

  SideStreams* ss = side_streams(st);
  if (!ss) return CGR_ERR_HIP;
  std::lock_guard<std::mutex> ss_lock(ss->mu);
  // instrumented (profiling) runs stay serial so per-kernel event times are isolated durations
  hipStream_t side = (prof_enabled() || single_stream()) ? st : ss->side;

  PendingReduce pend;
  auto retire = [&]() -> int {  // pend has run (folded into a TN, or launched)
    if (pend.job.slab && bucket_events && pend.bucket >= 0)
      HIP_RET(hipEventRecord(bucket_events[pend.bucket], side));
    pend = PendingReduce{};
    return 0;
  };
  // launch pend on its own (with `extra`, a job that runs in the same launch, if any)
  // max_blocks: the grid bound of the grouped reduce (kReduceMaxBlocks while the main chain runs
  // beside it; the backward's last one runs after the main chain has finished: unbounded)
  auto flush = [&](const RedJob* extra = nullptr, int max_blocks = kReduceMaxBlocks) -> int {
    RedJobs js{};
    if (pend.job.slab) js.j[js.n++] = pend.job;
    if (extra && extra->slab) js.j[js.n++] = *extra;
    if (js.n == 0) return 0;
    for (int i = 0; i < js.n; ++i) js.total += js.j[i].nblk;
    {
      ProfScope _p("splitk_reduce", side);
      HIP_RET(reduce_slabs_batched(js, max_blocks, side));
    }
    return retire();
  };
  // One weight gradient: the picked family's TN (operands as wgrad_launch takes them, wgrad.hpp)
  // into a slab pair checked to hold its plan, and its split-K reduction into o.  Side stream
  // (readout, layer, edge) into ws.slab[sb]: a split-bf16 TN reduces pend's slabs in its prologue
  // and leaves its own pending, an fp32 TN is followed by one launch for both; `bucket` is
  // complete then.  Node: caller's stream, slab2, reduced at once (flat after a split-bf16 TN:
  // this one ends the backward's main chain).
  auto wgrad = [&](auto site, const WgChoice& c, const void* img, const float* a, int vec,
                   auto&& make_b, const WgDst& o, int bucket,
                   int max_blocks = kReduceMaxBlocks) -> int {
    constexpr WgSite S = decltype(site)::value;
    constexpr bool own = S == WgSite::Node;
    const bool b3 = c.family == WgFamily::B3;
    hipStream_t ws_st = own ? st : side;
    const Reg<float>& sl = own ? ws.slab2 : ws.slab[sb];
    const Reg<float>& bsl = own ? ws.bslab2 : ws.bslab[sb];
    CGR_CHECK(c.slab_elems() <= sl.count && c.bslab_elems() <= bsl.count,
              "cgr: a weight-gradient plan exceeds the split-K slabs the workspace was sized for");
    {
      ProfScope _p(wgrad_class(S, c.family), ws_st);
      HIP_RET((wgrad_launch<S>(c, img, a, Hp, vec, make_b, sl, bsl, o.bias != nullptr, ws_st,
                               b3 && !own ? pend.job : RedJob{})));
    }
    if (own) {
      ProfScope _p("splitk_reduce", st);
      HIP_RET(reduce_slabs(sl, bsl, c.plan.splits, c.Nout, c.Kout, o.w, o.ld, o.col_off, o.bias, st,
                           o.gap_at, o.gap_len, b3));
      return 0;
    }
    RedJobs js{};  // (sized for the plan's split count)
    add_reduce_job(js, sl, bsl, c.plan.splits, c.Nout, c.Kout, o.w, o.ld, o.col_off, o.bias,
                   o.gap_at, o.gap_len);
    const RedJob mine = js.n ? js.j[0] : RedJob{};
    if (b3) {  // the TN took pend's job as its prologue; its own becomes pending
      if (const int rc = retire()) return rc;
      pend.job = mine;
      pend.bucket = bucket;
    } else {  // a TN that cannot fold: pend and its own reduction in one launch after it
      if (const int rc = flush(&mine, max_blocks)) return rc;
      if (bucket_events && bucket >= 0) HIP_RET(hipEventRecord(bucket_events[bucket], side));
    }
    sb ^= 1;
    return 0;
  };
  // x as the x-side weight gradients read it: in place, or the arena's padded copy (pad columns
  // zero) when F % 4 != 0; Fx columns of it are covered
  const float* xb = fv.xp ? fv.xp : b->x;
  const int64_t ldx = fv.xp ? d.Fp : F;
  const int Fx = (int)ldx;
  const bool x_aligned = ((uintptr_t)b->x & 15) == 0;

  // side: dwf, dbf; dzn; dW_n = dzn^T [x | s], db_n (forked before the main stream's readout NT:
  // deferring it behind a layer, or enqueuing the NT first, A/B -4..-14 %).  dzn is materialised
  // for the weight gradient only: the main stream's NT forms it inside the GEMM (LdActGradT).
  // the split-bf16 e-image TN takes dzn as the e-image the dzn kernel writes (dzn itself is
  // then never stored); the fp32 families read dzn
  const WgChoice ro = wgrad_pick(WgSite::Readout, d, x_aligned);
  const bool ro_b3 = ro.family == WgFamily::B3;
  // below the fused level (cgr_gnn_encode_backward: `dy` is dg [B, H], a general cotangent of the
  // pooled embedding; cgr_gnn_encode_nodes_backward: dn [N, H], one of the node embedding) the
  // upstream is neither a row nor a column factor, so every pooling mode takes max pooling's
  // route: dzn materialised on the main stream before the fork, the NT over the unscaled image;
  // no head gradients (the ffn entries of params / grads are not touched).  The nodes level has
  // no pool at all: the arena's pool_arg region, if cfg.pooling reserved one, was never written
  const bool fused = level == OutLevel::Fused;
  const bool max_pool = level != OutLevel::Nodes && fv.pool_arg != nullptr;  // CGR_POOL_MAX
  const bool dzn_main = max_pool || !fused;
  // dzn from the level's upstream (`dy` names dy [B], dg [B, H] or dn [N, H]; wf is read at the
  // fused level only): the TN's e-image, and fp32 where something reads it (the main stream's NT
  // under dzn_main, an fp32 weight-gradient family)
  const ReadoutUp up{level, dy, params[CGR_PARAM_FFN_W(D)]};
  auto form_dzn = [&](hipStream_t s) -> int {
    ProfScope _p(readout_act_bwd_class(level), s);
    HIP_RET(readout_act_bwd(up, iv.node_graph, fv.hn, fv.zn, N, H, Hp, d.act,
                            dzn_main || !ro_b3 ? ws.dzn : nullptr, ro_b3 ? ws.img_side : nullptr, s,
                            fv.inv_cnt, fv.pool_arg, fv.g));
    return 0;
  };
  auto side_readout = [&]() -> int {
    if (fused) {  // dwf = dy^T g, dbf: off the main chain (step A/B +0.8 %)
      ProfScope _p("head_bwd", side);
      HIP_RET(head_bwd(dy, fv.g, params[CGR_PARAM_FFN_W(D)], d.B, H, Hp, nullptr,
                       grads[CGR_PARAM_FFN_W(D)], grads[CGR_PARAM_FFN_B(D)], side));
    }
    // (dzn_main: dzn and its image came from the main stream, below)
    if (!dzn_main)
      if (const int rc = form_dzn(side)) return rc;
    // dW_n = dzn^T [x | s], db_n; bucket 0 (edge_to_node, ffn) is complete once its reduction
    // has run.  With x padded to Fp the reduce skips the pad columns.
    return wgrad(WgAt<WgSite::Readout>{}, ro, ws.img_side, ws.dzn, vec_for(xb, ldx, F),
                 [&](auto V) {
                   return LdConcat<decltype(V)::value>{xb, ldx, fv.a[D], Hp, Fx};
                 },
                 WgDst{grads[CGR_PARAM_E2N_W(D)], F + H, 0, grads[CGR_PARAM_E2N_B(D)], F, Fx - F},
                 0);
  };
  // main: ds = dzn W_n[:, F:] = diag(dy[graph]) act'(zn) (diag(wf) W_n[:, F:]) -- the row factor in
  // the epilogue, the column factor in the weight image (gnn_fwd.hip), act' in the A loader
  const bool acc = d.nt_acc();  // the NT launches' kernel variant (the images' tilings follow d)
  auto readout_nt = [&]() -> int {
    ProfScope _p("gemm_nt_readout_bwd", st);
    const float* m = d.act == ACT_RELU ? fv.hn : fv.zn;
    const b3_u4* img = static_cast<const b3_u4*>(fv.b3rob.p);
    if (dzn_main) {  // ds = dzn W_n[:, F:] with dzn materialised (its per-element arg-max mask is
                     // no row / column factor); the image is unscaled (gnn_fwd.hip)
      const EpStoreRowScale ep{ws.ds, Hp, N, H, nullptr, iv.node_graph, nullptr, fv.inv_deg};
      HIP_RET(launch_b3nt(LdPlain<4>{ws.dzn, Hp}, img, readout_cols(d), ep, N, H, H, st, acc));
      return 0;
    }
    // (mean pooling: dy / graph count; mean aggregation: ds / in-degree, for dh_D = ds[dst])
    const EpStoreRowScale ep{ws.ds, Hp, N, H, dy, iv.node_graph, fv.inv_cnt, fv.inv_deg};
    const B3Cols rc = readout_cols(d);  // the image's tiling (gnn_fwd.hip)
    // the activation derivative in the A loader, specialised per activation (main-loop code)
    if (d.act == ACT_RELU)
      HIP_RET(launch_b3nt(LdActGradT<ACT_RELU>{m, Hp, d.act}, img, rc, ep, N, H, H, st, acc));
    else if (d.act == ACT_SILU)
      HIP_RET(launch_b3nt(LdActGradT<ACT_SILU>{m, Hp, d.act}, img, rc, ep, N, H, H, st, acc));
    else
      HIP_RET(launch_b3nt(LdActGradT<-1>{m, Hp, d.act}, img, rc, ep, N, H, H, st, acc));
    return 0;
  };
  // capture order: fork, side work, then the main NT.  Enqueuing the NT first (the fork point
  // recorded before it, the side work after -- same dependencies) moves the NT onto the forward's
  // hardware queue in a captured graph but puts the first layer NT beside the readout TN: r05
  // same-box A/B 344.0k -> 341.0k reactions/s (3 runs each, profiles/r05_ro_first_ab.txt)
  if (dzn_main)  // dzn (fp32 for the NT, and the TN's e-image) before the fork
    if (const int rc = form_dzn(st)) return rc;
  if (side != st) HIP_RET(fork_to(ss, st, side));
  if (const int rc = side_readout()) return rc;
  if (const int rc = readout_nt()) return rc;

  // learnable-skip partial-sum slots per layer (bwd_dsig_slots)
  const int nb = bwd_dsig_slots(d);
  // row tile of the fused layer-backward GEMMs: crossing segments accumulate in dag
  const int seg_rows = b3nt_rows(E, H);
  const B3Cols lcols = layer_cols(d);  // the layer images' tiling (gnn_fwd.hip)
  const int seg_cols = lcols.tiles;
  const int seg_tiles = bwd_seg_tiles(d);
  const int spin = unpaired_spin_limit();  // CGR_UNPAIRED_SPIN_LIMIT (debug knob), per call
  auto layer_args = [&](int l) {
    uint32_t thresh;
    float scale;
    dropout_consts(dropout_p, training, l, &thresh, &scale);
    LayerBwdArgs la{};
    la.ds = ws.ds;
    la.dm = ws.dm;
    la.dst_s = iv.dst_s;
    la.rev_s = iv.rev_s;
    la.hnext = fv.h[l + 1];
    la.pre = fv.pre[l + 1];
    la.h0 = fv.h[0];
    la.sigma = d.learnable_skip ? params[CGR_PARAM_SKIP(D, l)] : nullptr;
    la.seed = iv.rng;  // the key the forward used (arena)
    la.thresh = thresh;
    la.scale = scale;
    la.layer = l;
    la.act = d.act;
    la.E = E;
    la.H = H;
    la.Hp = Hp;
    la.dpre = dpre(l);
    la.dsig_part = d.learnable_skip ? ws.dsig_part + (int64_t)l * nb : nullptr;
    return la;
  };
  // the top layer's weight gradient on the split-bf16 e-image TN takes dpre_{D-1}'s e-image from
  // the activation kernel that writes dpre_{D-1} (no e-image pass over it).  (The layers below
  // keep the e-image pass: written by the fused layer-backward GEMM's epilogue it cost each such
  // launch 10 us, step 0.755 -> 0.769 ms, profiles/r05_rejected_epilogue_eimage_*.  Against
  // the top layer's pass on the side stream: same-box A/B 341.6k vs 341.1k reactions/s,
  // profiles/r05_ab2_top_eimage_fused_vs_side.txt.)
  const WgChoice ly = wgrad_pick(WgSite::Layer, d, true);  // (no x operand)
  const bool top_b3 = D > 0 && ly.family == WgFamily::B3;
  if (D > 0) {  // top layer: dh_D = ds[dst]
    ProfScope _p("layer_act_bwd", st);
    LayerBwdArgs la = layer_args(D - 1);
    la.dag = dag_of(D - 1);
    la.cnt = ws.cnt;
    la.cnt_nodes = N;
    la.cnt_tiles = seg_cols;
    la.tile_rows = seg_rows;
    HIP_RET(layer_act_bwd(la, nb, top_b3 ? ws.img_top : nullptr, st));
  }
  auto edge_args = [&]() {
    LayerBwdArgs le{};
    le.dm = ws.dm;
    le.rev_s = iv.rev_s;
    le.h0 = fv.h[0];
    le.pre = fv.pre[0];
    le.act = d.act;
    le.E = E;
    le.H = H;
    le.Hp = Hp;
    le.dh0 = ws.dh0;
    le.dpre = ws.dh0;  // dpre0 is written in place of dh0 (the buffer it names)
    le.dpre_all = dpre(0);
    le.dpre_stride = (int64_t)E * Hp;
    le.nlayers = D;
    for (int k = 0; k < D; ++k) le.sig[k] = d.learnable_skip ? params[CGR_PARAM_SKIP(D, k)] : nullptr;
    return le;
  };
  // edge init: dpre0 = (dh0 + dh_0) * act'(pre0), dh0 summed from the layers' dpre buffers,
  // written to the dh0 buffer
  float* dpre0 = ws.dh0;
  for (int l = D - 1; l >= 0; --l) {
    float* dp = dpre(l);  // written by the previous iteration's fused kernel (or just above)
    // main: dm = dpre W_l.  The fork point is recorded before the NT is enqueued and the side
    // work after it: same dependencies, but a captured graph then keeps the main chain on one
    // hardware queue (A/B 1.283 -> 1.263 ms; DESIGN.md §9 "Stream order")
    hipEvent_t fork_ev = nullptr;
    if (side != st) HIP_RET(record_point(ss, st, &fork_ev));
    // dm = dpre_l W_l with the layer below's activation backward (or the edge init's) in the
    // epilogue: rows gathered through rev, dst segments summed in the tile (ep_bwd.hpp)
    const LayerBwdArgs lb = l > 0 ? layer_args(l - 1) : edge_args();
    {
      ProfScope _p("gemm_nt_layer_bwd_seg", st);
      const LdGatherRows al{dp, iv.rev_s, Hp};
      const b3_u4* img = static_cast<const b3_u4*>(fv.b3lb[l].p);
      float* dg = dag_of(l);
      float* dgn = l > 0 ? dag_of(l - 1) : nullptr;
      int* gcnt = ws.cnt + (int64_t)N * seg_cols + l;  // this launch's unpaired grid counter
      if (l > 0)
        HIP_RET(launch_b3nt(al, img, lcols,
                            EpLayerBwdSeg<false>{lb, ws.dm, iv.dst_s, iv.dst_ptr, iv.src_list,
                                                 iv.src_ptr, dg, dgn, ws.part, ws.cnt, iv.status,
                                                 E, H, N, seg_cols, gcnt, ss->dev_err, spin,
                                                 fv.inv_deg},
                            E, H, H, st, acc));
      else
        HIP_RET(launch_b3nt(al, img, lcols,
                            EpLayerBwdSeg<true>{lb, ws.dm, iv.dst_s, iv.dst_ptr, iv.src_list,
                                                iv.src_ptr, dg, dgn, ws.part, ws.cnt, iv.status,
                                                E, H, N, seg_cols, gcnt, ss->dev_err, spin,
                                                fv.inv_deg},
                            E, H, H, st, acc));
    }
    if (fork_ev) HIP_RET(hipStreamWaitEvent(side, fork_ev, 0));
    {  // side: dW_l = dpre^T m_l, db_l = colsum(dpre); the previous weight gradient's slabs are
       // reduced in the TN's prologue, this one's by the next TN (bucket D - l complete then)
      const void* img = l == D - 1 ? ws.img_top : ws.img_side;  // top layer: layer_act_bwd wrote it
      if (ly.family == WgFamily::B3 && l < D - 1) {
        ProfScope _p("eimage", side);
        HIP_RET(b3_eimage(dp, Hp, E, H, static_cast<b3_u4*>(ws.img_side.p), side));
      }
      const int rc = wgrad(WgAt<WgSite::Layer>{}, ly, img, dp, 4,
                           [&](auto) {
                             return LdGatherDiff<false>{fv.a[l], fv.h[l], iv.src_s, iv.rev_s, Hp};
                           },
                           WgDst{grads[CGR_PARAM_CONV_W(l)], H, 0, grads[CGR_PARAM_CONV_B(l)]},
                           D - l);
      if (rc) return rc;
    }
  }
  float* gW0 = grads[CGR_PARAM_EDGE_INIT_W];
  float* gb0 = grads[CGR_PARAM_EDGE_INIT_B];
  // tail: the fork point is recorded here and the side work (edge-feature TN) enqueued after the
  // main tail, as in the layer loop (A/B -0.8 %)
  hipEvent_t tail_ev = nullptr;
  if (side != st) HIP_RET(record_point(ss, st, &tail_ev));
  auto edge_tn = [&]() -> int {
    if (Fe > 0) {  // dW0[:, F:] = dpre0^T e, db0
      if (tail_ev) HIP_RET(hipStreamWaitEvent(side, tail_ev, 0));
      // reduced with the last layer's pending reduction in one launch (bucket D + 1 is recorded
      // at the join below), the last on the side stream: by then the main chain has ended (r05
      // trace: 13.5 us on 256 blocks for 1,300 logical ones, the step's tail), so it takes the GPU
      return wgrad(WgAt<WgSite::Edge>{}, wgrad_pick(WgSite::Edge, d, true), nullptr, dpre0, 4,
                   [&](auto) { return LdPlain<4>{fv.e_s, d.Fep}; }, WgDst{gW0, F + Fe, F, gb0}, -1,
                   1 << 20);
    }
    return flush();
  };
  if (!tail_ev) {
    const int rc = edge_tn();
    if (rc) return rc;
  }
  if (F > 0) {  // main: dW0[:, :F] = Gs^T x, Gs = segsum_src(dpre0) (own slab: beside the side
                // stream's work)
    const WgChoice nd = wgrad_pick(WgSite::Node, d, x_aligned);
    if (nd.family == WgFamily::B3) {  // Gs straight into the TN's e-image (never stored in fp32)
      ProfScope _p("segsum_src_bwd", st);
      HIP_RET(b3_segsum_eimage(dpre0, Hp, iv.src_list, iv.src_ptr, N, H,
                               static_cast<b3_u4*>(ws.img_main.p), st));
    } else {
      ProfScope _p("segsum_src_bwd", st);
      HIP_RET(segment_sum(dpre0, Hp, iv.src_list, iv.src_ptr, N, Hp, ws.Gs, Hp, st));
    }
    // db0 comes from the edge-feature TN when there is one
    const int rc = wgrad(WgAt<WgSite::Node>{}, nd, ws.img_main, ws.Gs, vec_for(xb, ldx, F),
                         [&](auto V) { return LdPlain<decltype(V)::value>{xb, ldx}; },
                         WgDst{gW0, F + Fe, 0, Fe > 0 ? nullptr : gb0, F, nd.Kout - F}, -1);
    if (rc) return rc;
  } else if (Fe == 0) {
    HIP_RET(hipMemsetAsync(gb0, 0, sizeof(float) * H, st));
  }
  if (tail_ev) {
    const int rc = edge_tn();
    if (rc) return rc;
  }

  if (d.learnable_skip) {
    ScalarReduceJobs sj{};
    for (int l = 0; l < D; ++l) {
      sj.out[l] = grads[CGR_PARAM_SKIP(D, l)];
      // the top layer's activation kernel fills all nb slots, the fused GEMMs two per workgroup
      sj.count[l] = l == D - 1 ? nb : 2 * seg_tiles;
    }
    sj.n = D;
    ProfScope _p("skip_grad_reduce", st);
    HIP_RET(reduce_partials(ws.dsig_part, nb, sj, st));
  }
  if (const int rc = flush()) return rc;  // (nothing left unless an edge TN was not run)
  // join: every gradient is complete when the main stream reaches here
  HIP_RET(depend(ss, side, st));
  if (bucket_events) HIP_RET(hipEventRecord(bucket_events[D + 1], st));
  return 0;
}

// Input gradients (autograd's x.grad / edge_attr.grad for the reference, GNN.py:85-86,105-106):
// x enters edge_init through x[src] and edge_to_node through [x | s], edge_attr edge_init only:
//   dq0 = dpre0 W0                     (q0 = [x[src] | e], GNN.py:86)
//   dx  = segsum_src(dpre0) W0[:, :F] + dzn W_n[:, :F]  = [Gs | dzn] [W0x ; W_nx]
//   de  = dpre0 W0[:, F:]              (rows back to the caller's edge order through perm)
// dpre0 is what gnn_backward_impl left in the workspace's dh0 buffer; Gs and dzn are re-formed
// in fp32 (the backward keeps them as e-images only) and the stacked weight slices transposed
// into wxT, so both products are one fp32 MFMA NT launch each (gemm.hpp), exact-fp32 products.
int gnn_input_grads_impl(const Dims& d, const float* const* params, const void* arena,
                         const float* dy, void* workspace, float* dx, float* de, hipStream_t st,
                         OutLevel level) {
  const ArenaView av = arena_view(d, false, const_cast<void*>(arena));
  const IndexView& iv = av.idx;
  const FloatView& fv = av.flt;
  const WorkspaceView ws = workspace_view(d, workspace);
  const float* dpre0 = ws.dh0;
  const int N = (int)d.N, E = (int)d.E, H = d.H, Hp = d.Hp, F = d.F, Fe = d.Fe, D = d.D;
  if (de && Fe > 0) {  // de = dpre0 W0e: B = W0[:, F:]^T, the forward's w0eT [Fe, Hp]
    ProfScope _p("input_grad_edge", st);
    const LdPlain<4> al{dpre0, Hp};
    const LdPlain<4> bl{fv.w0eT, Hp};
    const EpStorePermRows ep{de, Fe, E, Fe, iv.perm};
    HIP_RET(with_nt_rn(Fe, [&](auto RN) {
      return launch_gemm_nt<4, 1, decltype(RN)::value, 1>(al, bl, ep, E, Fe, H, st);
    }));
  }
  if (dx && F > 0) {
    const int ldw = input_grad_ldw(H);
    {
      ProfScope _p("input_grad_prep", st);
      HIP_RET(segment_sum(dpre0, Hp, iv.src_list, iv.src_ptr, N, H, ws.Gs, Hp, st));
      // `dy` is the level's upstream: dy [B], dg [B, H] or dn [N, H]; wf is read at Fused only
      const ReadoutUp up{level, dy, params[CGR_PARAM_FFN_W(D)]};
      HIP_RET(readout_act_bwd(up, iv.node_graph, fv.hn, fv.zn, N, H, Hp, d.act, ws.dzn, nullptr, st,
                              fv.inv_cnt, fv.pool_arg, fv.g));
      TransposeJobs tj{};  // wxT [F, ldw] = [W0[:, :F]^T | W_n[:, :F]^T]
      tj.job[0] = TransposeJob{params[CGR_PARAM_EDGE_INIT_W], F + Fe, 0, ws.wxT, ldw, H, F};
      tj.job[1] = TransposeJob{params[CGR_PARAM_E2N_W(D)], F + H, 0, ws.wxT + H, ldw, H, F};
      tj.n = 2;
      HIP_RET(transpose_batch(tj, st));
    }
    ProfScope _p("input_grad_node", st);
    const LdPlain<4> bl{ws.wxT, ldw};
    const EpStore ep{dx, F, N, F, nullptr};
    // [Gs | dzn] rows: the concat boundary H must not split a VEC-wide chunk
    HIP_RET(with_vec(H % 4 == 0 ? 4 : (H % 2 == 0 ? 2 : 1), [&](auto V) {
      const LdConcat<decltype(V)::value> al{ws.Gs, Hp, ws.dzn, Hp, H};
      return with_nt_rn(F, [&](auto RN) {
        return launch_gemm_nt<4, 1, decltype(RN)::value, 1>(al, bl, ep, N, F, 2 * H, st);
      });
    }));
  }
  return 0;
}

}  // namespace cgr
