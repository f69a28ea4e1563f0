// Weight gradients: every one is a split-K TN GEMM dW [Nout, Kout] = A^T B over R rows that any of
// three kernel families can run.  The one description of each site -- shape, candidate families in
// order of preference, each with its workgroup target, plan and feasibility -- that gnn_bwd.hip
// launches through and capi.hip sizes the split-K slabs through.  (Included by dispatch.hpp.)
//
//   site     Nout  Kout                            R   A       B
//   readout  H     Fx + H                          N   dzn     [x | s]
//   layer    H     H                               E   dpre_l  a_l[src] - h_l[rev]
//   node     H     Fx (F on the LDS-staged family) N   Gs      x
//   edge     H     Fe                              E   dpre0   e
// Fx = the x columns an x-side GEMM covers: F, or Fp when F % 4 != 0 (the arena's zero-padded
// copy xp is read then; the reduce skips the pad columns).
#pragma once

#include "gnn_internal.hpp"

namespace cgr {

// LDS-staged fp32 TN: floor(target / tiles) splits, 4 workgroups per CU (A/B: step-neutral vs
// 768, isolated weight gradient -20 %)
constexpr int kTnTargetWorkgroups = 1024;
// edge-feature weight gradient (K = 14) beside the node TN: fewer splits, fewer CUs taken from
// it (A/B 1024 -> 256 -0.3 %, 128 +0.4 %, 64 +2 %)
constexpr int kEdgeTnTargetWorkgroups = 256;
// Register-direct fp32 TN (gemm_tnr.hpp): fragments per lane 5 (H % 5 == 0: 80 x 80 tiles) or 4.
// Split targets: layer 512 (2 workgroups per CU: floor(512 / 25 tiles) = 20 splits), node 512,
// readout 256 (1 workgroup per CU beside the main-stream tail; A/B +0.5 %).
constexpr int kTnrLayerTarget = 512;
constexpr int kTnrNodeTarget = 512;
constexpr int kTnrReadoutTarget = 256;
// Split-bf16 TN (gemm_b3tn.hpp) workgroup targets (the layer's kB3TnTarget is beside its planner):
// readout beside the critical readout NT 112 (A/B +0.7 % vs 176, 64 -6 %), node (the backward's
// tail) 256 (+0.7 % vs 176, 352 -0.8 %)
constexpr int kB3TnReadoutTarget = 112;
constexpr int kB3TnNodeTarget = 256;

enum class WgSite { Readout, Layer, Node, Edge };
template <WgSite S>
using WgAt = std::integral_constant<WgSite, S>;  // a site as a compile-time argument
// split-bf16 e-image TN (gemm_b3tn.hpp), register-direct fp32 TN (gemm_tnr.hpp), LDS-staged fp32 TN
// (gemm.hpp): the order of preference at every site
enum class WgFamily { B3, Tnr, F32 };

// One family at one site.  `plan`: what the family's planner returned -- all three plan in TnPlan
// (gemm.hpp) and write the slab layout [splits][Nout][round_up(Kout, 4)], bias [splits][Nout].
struct WgChoice {
  WgFamily family;
  int target;  // workgroups the plan aims at
  int fa, fb;  // tnr fragment pair (0 otherwise)
  int Nout, Kout, R;
  TnPlan plan;
  bool feasible;         // the family covers this shape
  bool needs_aligned_x;  // ... but reads x in 16-byte units
  size_t slab_elems() const { return (size_t)plan.splits * Nout * (size_t)((Kout + 3) & ~3); }
  size_t bslab_elems() const { return (size_t)plan.splits * Nout; }
};

// LDS-staged fp32 TN of shape (Nout, Kout, R): covers every shape (also the standalone conv's)
inline WgChoice wg_f32(int Nout, int Kout, int R, int target = kTnTargetWorkgroups) {
  const TnPlan p = with_tn_shape(Nout, Kout, [&](auto W, auto RN) {
    return plan_tn<decltype(W)::value, 1, decltype(RN)::value, 1>(Nout, Kout, R, target);
  });
  return WgChoice{WgFamily::F32, target, 0, 0, Nout, Kout, R, p, true, false};
}
template <class AL, class BL>
inline hipError_t wg_f32_launch(const WgChoice& c, const AL& al, const BL& bl, float* slab,
                                float* bslab, bool want_bias, hipStream_t st) {
  return with_tn_shape(c.Nout, c.Kout, [&](auto W, auto RN) {
    return launch_gemm_tn<decltype(W)::value, 1, decltype(RN)::value, 1>(
        al, bl, c.plan, slab, bslab, c.Nout, c.Kout, c.R, want_bias, st);
  });
}

// register-direct fp32 TN: Nout % FA == 0 and Kout % FB == 0 (tnr_ok)
template <int FA, int FB>
inline WgChoice wg_tnr(int Nout, int Kout, int R, int target, bool x_side) {
  return WgChoice{WgFamily::Tnr, target, FA, FB, Nout, Kout, R,
                  plan_tnr<FA, FB>(Nout, Kout, R, target), tnr_ok<FA, FB>(Nout, Kout), x_side};
}
// split-bf16 e-image TN: Nout up to 32 fragments and B extents inside 32-bit element offsets
// (b3tni_ok; bl carries the B operand's leading dimensions, its pointers are not read)
template <class BL>
inline WgChoice wg_b3(const BL& bl, int Nout, int Kout, int R, int target, bool x_side) {
  return WgChoice{WgFamily::B3, target, 0, 0, Nout, Kout, R,
                  b3tn_plan(Nout, Kout, R, target), b3tni_ok(bl, Nout, R), x_side};
}

struct WgCandidates {
  WgChoice c[3];
  int n;  // 0: the site does not exist for these dims (node without F, edge without Fe)
};

// The families a site may run for these dims, most preferred first, feasible or not: the first
// feasible one runs (wgrad_pick), the slabs hold the largest of all of them (workspace_regions).
// x_side families read x (or xp) in 16-byte units: Fx % 4 == 0 always, the pointer is the caller's.
inline WgCandidates wgrad_candidates(WgSite s, const Dims& d) {
  const int H = d.H, N = (int)d.N, E = (int)d.E;
  const int64_t Hp = d.Hp;
  const int Fx = d.F % 4 ? d.Fp : d.F;
  WgCandidates w{};
  // CGR_PRECISION_FP32 leaves the split-bf16 family out at every site: the first feasible fp32
  // family runs, on fp32 rows (bias riders included), and no e-image is written or sized
  const bool fp32_only = d.precision == CGR_PRECISION_FP32;
  auto add = [&](const WgChoice& c) {
    if (!(fp32_only && c.family == WgFamily::B3)) w.c[w.n++] = c;
  };
  switch (s) {
    case WgSite::Readout:
      add(wg_b3(LdConcat<4>{nullptr, Fx, nullptr, Hp, Fx}, H, Fx + H, N, kB3TnReadoutTarget, true));
      add(wg_tnr<5, 4>(H, Fx + H, N, kTnrReadoutTarget, true));  // 80 x 64 tiles
      add(wg_f32(H, Fx + H, N));
      break;
    case WgSite::Layer:
      add(wg_b3(LdGatherDiff<false>{nullptr, nullptr, nullptr, nullptr, Hp}, H, H, E, kB3TnTarget,
                false));
      if (tnr_ok<5, 5>(H, H))
        add(wg_tnr<5, 5>(H, H, E, kTnrLayerTarget, false));
      else if (tnr_ok<4, 4>(H, H))
        add(wg_tnr<4, 4>(H, H, E, kTnrLayerTarget, false));
      add(wg_f32(H, H, E));
      break;
    case WgSite::Node:
      if (d.F == 0) break;
      add(wg_b3(LdPlain<4>{nullptr, Fx}, H, Fx, N, kB3TnNodeTarget, true));
      add(wg_tnr<5, 4>(H, Fx, N, kTnrNodeTarget, true));
      add(wg_f32(H, d.F, N));  // masks the columns past F itself: no pad columns in its slabs
      break;
    case WgSite::Edge:  // K = Fe = 14: the fp32 family only
      if (d.Fe > 0) add(wg_f32(H, d.Fe, E, kEdgeTnTargetWorkgroups));
      break;
  }
  return w;
}

// The family that runs: a pure function of the site, the dims and whether the caller's x is
// 16-byte aligned (it matters only when F % 4 == 0: otherwise xp, in the arena, is read).  The
// LDS-staged family ends every list and is always feasible.
inline WgChoice wgrad_pick(WgSite s, const Dims& d, bool x_aligned) {
  const WgCandidates w = wgrad_candidates(s, d);
  const bool ax = x_aligned || d.F % 4 != 0;
  for (int i = 0; i < w.n; ++i)
    if (w.c[i].feasible && (ax || !w.c[i].needs_aligned_x)) return w.c[i];
  return WgChoice{};
}

// Launch the picked family.  A [R, lda] fp32 (img: its e-image, which the split-bf16 family reads
// instead), B as the loader make_b(IC<V>) returns: V = vec on the LDS-staged family, 4 on the
// other two (16-byte rows: needs_aligned_x).  A site instantiates only the kernels it can pick.
template <WgSite S, class MakeB>
inline hipError_t wgrad_launch(const WgChoice& c, const void* img, const float* a, int64_t lda,
                               int vec, MakeB&& make_b, float* slab, float* bslab, bool want_bias,
                               hipStream_t st, const RedJob& prev = RedJob{}) {
  const TnPlan& p = c.plan;
  const LdPlain<4> al{a, lda};
  if (c.family == WgFamily::F32)
    return with_vec(vec, [&](auto V) {
      return wg_f32_launch(c, al, make_b(V), slab, bslab, want_bias, st);
    });
  if constexpr (S != WgSite::Edge) {
    const auto bl = make_b(IC<4>{});
    if (c.family == WgFamily::B3)
      return launch_b3tni(B3EImg{static_cast<const b3_u4*>(img), b3_eimg_cols(c.Nout)}, bl, p,
                          slab, bslab, c.Nout, c.Kout, c.R, want_bias, st, prev);
    if constexpr (S == WgSite::Layer) {
      if (c.fa == 5)
        return launch_gemm_tnr<5, 5>(al, bl, p, slab, bslab, c.Nout, c.Kout, c.R, want_bias, st);
      return launch_gemm_tnr<4, 4>(al, bl, p, slab, bslab, c.Nout, c.Kout, c.R, want_bias, st);
    } else {
      return launch_gemm_tnr<5, 4>(al, bl, p, slab, bslab, c.Nout, c.Kout, c.R, want_bias, st);
    }
  }
  return hipErrorInvalidValue;
}

}  // namespace cgr
