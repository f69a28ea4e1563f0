// Fused layer-forward epilogue (gemm_b3nt_kernel, a kTile epilogue): EpLayer whose GEMM also
// produces the layer's scatter-add a[v] = sum_{dst(e) = v} h'[e] (GNN.py:134) from its row tile
// (rows are dst-sorted): the "gather -> MLP -> segmented reduce" pass in one launch.
//
// Each segment's rows are summed in row order.  A segment inside the tile is stored; one crossing
// into one neighbouring tile is added atomically to a[v], which edge_init_segsum_fwd zeroed (two
// partials onto zero: p + q == q + p, deterministic); one over three or more row tiles (a hub
// node, in-degree > BM + 1) leaves its partial in a slot fixed by the data and its last
// contributor sums the slots in row-tile order -- deterministic for every in-degree
// (handoff.hpp; the backward twin is ep_bwd.hpp).
#pragma once

#include <type_traits>

#include "epilogues.hpp"
#include "handoff.hpp"
#include "stamps.hpp"

namespace cgr {

struct EpLayerSeg : EpLayer {
  static constexpr bool kTile = true;
  static constexpr bool kStarts = true;  // the segment pass walks the tile's start list
  const int* dst_s;  // [M] node of each (dst-sorted) row
  float* aout;       // [nodes, lda]; crossing / empty segments zeroed beforehand
  int64_t lda;
  float* znext;      // or null: [nodes, lda] whose crossing segments this GEMM zeroes (eval ring)
  // hub segments (over >= 3 row tiles: in-degree > rows per tile + 1), completed in fixed order
  // by their last contributor
  const int* dst_ptr;  // [nodes + 1] dst CSR of the sorted rows
  float* part;         // [tiles, 2, BN] their partial sums (slot_of)
  int* cnt;            // [nodes * tiles_n] tickets (zero on entry, left zero)
  int tiles_n;
  // apply4z that also returns the stored h (rows / columns outside: z unchanged)
  template <int A = -1>
  __device__ __forceinline__ float4 apply4z_h(int r, int c, float4 z, const Ctx& cx) const {
    if (r >= M || c >= N) return z;
    return this->template finish4<A>(r, c, z, cx);
  }

  // t: B3NtTile (gemm_b3.hpp); the accumulator tile in LDS already holds z: the addend went in
  // in the tail step (kAddend)
  template <class T>
  __device__ __forceinline__ void tile(const T t) const {  // by value: see B3NtTile
    using L = typename T::Lds;
    constexpr int BM = T::BM, BN = T::BN, NT = T::NT, LDC = T::LDC, C4 = BN / 4;
    const int m0 = t.m0, n0 = t.n0, tid = t.tid;
    const int tm = m0 / BM, tn = n0 / BN;
    const float* C = L::C(t.lds);
    const int* sd = L::sd(t.lds);
    const int nrow_t = min(BM, M - m0);
    // The tile's segment starts, in two halves (rows 0..63, rows 64..127); nh0 / nseg from the
    // mask: starts among rows < nrow_t (rows past the tile's count are sentinel starts)
    uint64_t mlo, mhi;
    L::load_mask(t.lds, mlo, mhi);
    const uint64_t klo = nrow_t >= 64 ? mlo : mlo & ((1ull << nrow_t) - 1);
    const uint64_t khi =
        nrow_t >= 128 ? mhi : (nrow_t > 64 ? mhi & ((1ull << (nrow_t - 64)) - 1) : 0);
    const int nh0 = __popcll(klo);
    const int nseg = nh0 + __popcll(khi);
    auto seg_start = [&](int j) { return L::starts(t.lds, j >= nh0)[j < nh0 ? j : j - nh0]; };
    // segment [r, e) x column group c4 of the tile: a[v] stored, or handed over (crossing)
    auto seg_out = [&](int r, int e, int c4, float4 a) {
      const int col = n0 + 4 * c4;
      const int v = sd[r + 1];
      float* dst = aout + (int64_t)v * lda + col;
      const bool head = r == 0 && sd[0] == v, tail = e == nrow_t && sd[nrow_t + 1] == v;
      if (tail && !head && znext)  // the tile where a crossing segment starts
        *reinterpret_cast<float4*>(znext + (int64_t)v * lda + col) = f4zero();
      if (head || tail)
        seg_hand_over<BM, BN>(dst, part, t.tile_id, tm, dst_ptr[v], dst_ptr[v + 1], c4, a);
      else
        st4_nt(dst, a);  // (common.hpp)
    };
    // ONE pass over (segment, column group) items -- each item applies its segment's rows in row
    // order (h stored) and sums them: no h write-back to LDS, no second pass behind a barrier.
    // The lanes of a wave take consecutive column groups of one or two segments, so they run the
    // same row count but at segment boundaries.  One loop per activation, chosen once.
    auto pass = [&](auto Ac) {
#pragma unroll
      for (int it = 0; it < T::EIT; ++it) {
        const int q = tid + NT * it;
        if (q >= nseg * C4) break;
        const int j = q / C4, c4 = q - j * C4, col = n0 + 4 * c4;
        if (col >= N) continue;
        const int r = seg_start(j), e = seg_end(mlo, mhi, r);
        float4 a = f4zero();
        for (int k = r; k < e; ++k)
          a = f4add(a, this->template apply4z_h<decltype(Ac)::value>(
                           m0 + k, col, *reinterpret_cast<const float4*>(&C[k * LDC + 4 * c4]),
                           t.cx));
        seg_out(r, e, c4, a);
      }
    };
    if (act == ACT_RELU) pass(std::integral_constant<int, ACT_RELU>{});
    else if (act == ACT_SILU) pass(std::integral_constant<int, ACT_SILU>{});
    else pass(std::integral_constant<int, -1>{});  // GELU and the rest
    CGR_STAMP(4);
    // hub segments: the last contributor sums the slots of every row tile in order
    const int vh = sd[0] == sd[1] ? sd[0] : -3;  // head segment's node, if any
    const int vt = sd[nrow_t] == sd[nrow_t + 1] ? sd[nrow_t] : -3;  // tail segment's node
    auto hub = [&](int v) { return v >= 0 && seg_tiles(dst_ptr[v], dst_ptr[v + 1], BM) >= 3; };
    const bool bh = hub(vh), bt = vt != vh && hub(vt);  // uniform over the workgroup
    if (bh || bt) {
      int* done = L::done(t.lds);
      ep_vm_drain();  // this wave's slot stores
      __syncthreads();
      if (tid == 0) seg_tickets<BM>(bh ? vh : -3, bt ? vt : -3, dst_ptr, cnt, tiles_n, tn, done);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int v = done[k];
        if (v < 0) continue;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // loads stay below the ticket
        const int t0 = dst_ptr[v] / BM, t1 = (dst_ptr[v + 1] - 1) / BM;
        for (int c4 = tid; c4 < C4; c4 += NT) {
          const int col = n0 + 4 * c4;
          if (col >= N) continue;
          *reinterpret_cast<float4*>(aout + (int64_t)v * lda + col) =
              seg_slot_sum<BN>(part, t0, t1, tiles_n, tn, c4);
        }
        if (tid == 0) cnt[(int64_t)v * tiles_n + tn] = 0;
      }
    }
  }
};

}  // namespace cgr
