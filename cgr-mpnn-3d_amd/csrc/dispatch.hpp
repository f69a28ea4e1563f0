// Host-side tile / vector-width selection shared by forward, backward and workspace sizing.
//
// GEMM families (one per shape class, picked per call site by same-box A/B of the whole step,
// DESIGN.md §4):
//   gemm_b3.hpp   split-bf16 NT (every NT GEMM of the model)
//   gemm_b3tn.hpp split-bf16 e-image TN (layer / node / readout weight gradients whose output
//                 rows fit one workgroup)
//   gemm_tnr.hpp  register-direct fp32 TN (weight gradients of shapes the split TN does not cover)
//   gemm.hpp      LDS-staged fp32 NT / TN (standalone DMPNNConv, the edge-feature weight gradient
//                 with K = Fe = 14, and any remaining shape)
// What the three share is in gemm.hpp: the row loaders (an operand is described once, as an Ld*
// struct, whichever family reads it) and the weight gradients' plan type and split rule (TnPlan,
// tn_split).  Which TN family a weight gradient takes, with which workgroup target: wgrad.hpp (one
// table for the launch and for the slab sizing).
#pragma once

#include <stdint.h>

#include <type_traits>

#include "gemm.hpp"
#include "gemm_b3.hpp"
#include "gemm_b3tn.hpp"
#include "gemm_tnr.hpp"

namespace cgr {

template <int V>
using IC = std::integral_constant<int, V>;

// widest of {4, 2, 1} such that every row starts VEC-aligned (ld, pointer) and the VEC-wide
// chunk holding the last logical element stays inside the row (round_up(K, VEC) <= ld): the
// loaders read whole chunks and mask elements >= K
inline int vec_for(const void* p, int64_t ld, int64_t K) {
  const uintptr_t a = (uintptr_t)p;
  if (ld % 4 == 0 && (K + 3) / 4 * 4 <= ld && a % 16 == 0) return 4;
  if (ld % 2 == 0 && K % 2 == 0 && a % 8 == 0) return 2;
  return 1;
}

template <class F>
inline auto with_vec(int v, F&& f) {
  if (v == 4) return f(IC<4>{});
  if (v == 2) return f(IC<2>{});
  return f(IC<1>{});
}

// fp32 NT GEMM: 4 waves (BM = 64 rows), RN column fragments: 5 when the output width tiles by 80
// (H = 400 -> 5 tiles, no waste), else 4 (BN = 64).
template <class F>
inline auto with_nt_rn(int N, F&& f) {
  if (N % 80 == 0) return f(IC<5>{});
  return f(IC<4>{});
}

// fp32 TN GEMM: WAVES from the output-row count (= H), RN from the output-column count.
template <class F>
inline auto with_tn_shape(int Nout, int Kout, F&& f) {
  if (Nout % 80 == 0) {
    if (Kout <= 16) return f(IC<5>{}, IC<1>{});
    if (Kout % 80 == 0) return f(IC<5>{}, IC<5>{});
    return f(IC<5>{}, IC<4>{});
  }
  if (Kout <= 16) return f(IC<4>{}, IC<1>{});
  if (Kout % 80 == 0) return f(IC<4>{}, IC<5>{});
  return f(IC<4>{}, IC<4>{});
}

}  // namespace cgr

#include "wgrad.hpp"  // the weight-gradient sites: family choice, plans, slab sizes
