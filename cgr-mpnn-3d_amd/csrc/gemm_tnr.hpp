// Register-direct TN GEMM for the weight gradients (gfx950, fp32 MFMA, no LDS in the main loop).
//
//   C[n, k] = sum_e A(e, n) * B(e, k)          (dW = dZ^T Q: A = dZ rows, B = Q rows)
//
// "Strided fragments": with the reduction index e as the MFMA k dimension, lane (fr, fg) of a
// v_mfma_f32_16x16x4_f32 supplies A(e = e0 + fg, m = fr) and B(e0 + fg, n = fr).  Output row
// fragment i of a wave tile is mapped to the rows n0 + FA * m + i (m = 0..15), so the FA
// consecutive values A(e, n0 + FA*fr .. + FA-1) that ONE lane loads with a 16-byte (+4-byte)
// load are exactly its operands for the FA row fragments; likewise FB column fragments.  A wave
// therefore streams its operands straight from L2 into registers, FA*FB MFMAs per 4 rows of e,
// with no LDS traffic and no barrier in the loop.
//
// Decomposition: a workgroup = 4 waves = one (16 FA x 16 FB) output tile and one split (row range)
// of e; the 4 waves take interleaved 4-row steps of the split and their partial tiles are combined
// through LDS in a fixed order ((w0 + w1) + (w2 + w3)) before the split's fp32 slab is written
// (same slab layout as gemm_tn_kernel, so reduce_slabs is shared).  Deterministic.
//
// Operands are the loaders of gemm.hpp (LdPlain, LdConcat, LdGatherDiff), the same objects the
// other two TN families take; how this kernel reads one is TnrSrc<L>, below.  Plans are TnPlan
// (gemm.hpp) by the shared split rule: at least 64 rows per split, 16-row granule (plan_tnr).
#pragma once

#include "common.hpp"
#include "gemm.hpp"

namespace cgr {

// F consecutive floats p[0 .. F-1] (4-byte aligned: gfx950 global loads need no 16-byte alignment)
template <int F>
__device__ __forceinline__ void tnr_ld(const float* __restrict__ p, float (&v)[F]) {
  if constexpr (F >= 4) {
    float4 q;
    __builtin_memcpy(&q, p, 16);
    v[0] = q.x;
    v[1] = q.y;
    v[2] = q.z;
    v[3] = q.w;
#pragma unroll
    for (int i = 4; i < F; ++i) v[i] = p[i];
  } else {
#pragma unroll
    for (int i = 0; i < F; ++i) v[i] = p[i];
  }
}

// Per operand kind (the loaders of gemm.hpp, described once per call site): idx() loads the row
// indices of row e (the gather's), fetch() issues the loads of F consecutive columns from c,
// combine() forms their fp32 values.  Rows and columns are in bounds (the kernel clamps them).
template <class L>
struct TnrSrc;
// plain rows: value(e, c) = base[e * ld + c]
template <int V>
struct TnrSrc<LdPlain<V>> {
  struct Idx {};
  static __device__ __forceinline__ Idx idx(const LdPlain<V>&, int) { return Idx{}; }
  template <int F>
  struct Raw {
    float v[F];
  };
  template <int F>
  static __device__ __forceinline__ void fetch(const LdPlain<V>& l, int e, const Idx&, int c,
                                               Raw<F>& r) {
    tnr_ld<F>(l.base + (int64_t)e * l.ld + c, r.v);
  }
  template <int F>
  static __device__ __forceinline__ void combine(const LdPlain<V>&, const Raw<F>& r,
                                                 float (&v)[F]) {
#pragma unroll
    for (int i = 0; i < F; ++i) v[i] = r.v[i];
  }
};

// message rows of a layer: value(e, c) = a[src[e], c] - h[rev[e], c]   (GNN.py:136-141)
template <bool X>
struct TnrSrc<LdGatherDiff<X>> {
  struct Idx {
    int s, r;
  };
  static __device__ __forceinline__ Idx idx(const LdGatherDiff<X>& l, int e) {
    return Idx{l.src[e], X ? (e ^ 1) : l.rev[e]};
  }
  template <int F>
  struct Raw {
    float va[F], vh[F];
  };
  template <int F>
  static __device__ __forceinline__ void fetch(const LdGatherDiff<X>& l, int, const Idx& x, int c,
                                               Raw<F>& r) {
    tnr_ld<F>(l.a + (int64_t)x.s * l.ld + c, r.va);
    tnr_ld<F>(l.h + (int64_t)x.r * l.ld + c, r.vh);
  }
  template <int F>
  static __device__ __forceinline__ void combine(const LdGatherDiff<X>&, const Raw<F>& r,
                                                 float (&v)[F]) {
#pragma unroll
    for (int i = 0; i < F; ++i) v[i] = r.va[i] - r.vh[i];
  }
};

// [x | s] rows of the readout (GNN.py:106): value(e, c) = c < F ? x[e, c] : s[e, c - F]; F % 4 == 0
// (x padded to 16-byte rows), so a lane's run of FB <= 4 columns never straddles the seam
template <int V>
struct TnrSrc<LdConcat<V>> {
  struct Idx {};
  static __device__ __forceinline__ Idx idx(const LdConcat<V>&, int) { return Idx{}; }
  template <int F_>
  struct Raw {
    float v[F_];
  };
  template <int F_>
  static __device__ __forceinline__ void fetch(const LdConcat<V>& l, int e, const Idx&, int c,
                                               Raw<F_>& r) {
    tnr_ld<F_>(c < l.F ? l.x + (int64_t)e * l.ldx + c : l.s + (int64_t)e * l.lds + (c - l.F), r.v);
  }
  template <int F_>
  static __device__ __forceinline__ void combine(const LdConcat<V>&, const Raw<F_>& r,
                                                 float (&v)[F_]) {
#pragma unroll
    for (int i = 0; i < F_; ++i) v[i] = r.v[i];
  }
};

constexpr int TNR_WAVES = 4;
// data loads 2 steps (8 rows) ahead of the MFMAs, row indices 3
constexpr int kTnrPf = 2;

template <int FA, int FB, class AL, class BL>
__global__ __launch_bounds__(TNR_WAVES * 64, 2) void gemm_tnr_kernel(
    AL al, BL bl, float* __restrict__ slab, float* __restrict__ bslab, int Nout, int Kout, int R,
    int rows_per_split, int tiles_k, int want_bias) {
  using SA = TnrSrc<AL>;
  using SB = TnrSrc<BL>;
  constexpr int TM = 16 * FA, TK = 16 * FB;
  __shared__ __attribute__((aligned(16))) float red[2][64 * FA * FB * 4];  // two partial tiles
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int tiles_n = (Nout + TM - 1) / TM;
  const int ntiles = tiles_n * tiles_k;
  // XCD-contiguous remap: the tiles of one split (same rows of A and B) share an XCD's L2
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int split = lin / ntiles, tile = lin - split * ntiles;
  const int tn = tile / tiles_k, tk = tile - tn * tiles_k;
  const int n0 = tn * TM, k0 = tk * TK;
  const int e_begin = split * rows_per_split;
  const int e_end = min(R, e_begin + rows_per_split);

  // this lane's FA rows of the tile, FB columns.  Nout % FA == 0 and Kout % FB == 0 (launcher
  // checks), so a lane's run is either fully valid or fully past the end; the latter is clamped in
  // bounds and only reaches outputs that are never stored
  const int na = min(n0 + FA * fr, Nout - FA);
  const int kb = min(k0 + FB * fr, Kout - FB);

  floatx4 acc[FA][FB];
#pragma unroll
  for (int i = 0; i < FA; ++i)
#pragma unroll
    for (int j = 0; j < FB; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  float bs[FA];
#pragma unroll
  for (int i = 0; i < FA; ++i) bs[i] = 0.f;

  // wave w takes steps w, w + 4, ... of 4 rows each; lane group fg row e = base + fg
  const int nrows = max(e_end - e_begin, 0);
  const int nsteps = (nrows + 3) >> 2;
  const int my_steps = nsteps > w ? (nsteps - w + TNR_WAVES - 1) / TNR_WAVES : 0;
  // step t of this wave -> row e (clamped to a valid row; ok = inside the split)
  auto row_of = [&](int t, bool& ok) {
    const int e = e_begin + 4 * (w + TNR_WAVES * t) + fg;
    ok = e < e_end;
    return ok ? e : (e_begin < R ? e_begin : 0);
  };
  // index rows (gathered sources) are loaded one step ahead of the data loads, which are one step
  // ahead of the MFMAs: no load waits on another load inside a step
  constexpr int NB = kTnrPf + 1;  // register sets: data kTnrPf steps ahead
  typename SA::template Raw<FA> ra[NB];
  typename SB::template Raw<FB> rb[NB];
  typename SA::Idx ia[NB];
  typename SB::Idx ib[NB];
  int er[NB];
  bool ok[NB], okn[NB];
  auto fetch_idx = [&](int t, int buf) {
    er[buf] = row_of(t, okn[buf]);
    ia[buf] = SA::idx(al, er[buf]);
    ib[buf] = SB::idx(bl, er[buf]);
  };
  auto fetch = [&](int buf) {  // data of the step whose indices sit in idx buffer buf
    ok[buf] = okn[buf];
    SA::template fetch<FA>(al, er[buf], ia[buf], na, ra[buf]);
    SB::template fetch<FB>(bl, er[buf], ib[buf], kb, rb[buf]);
  };
  auto compute = [&](int buf) {
    float av[FA], bv[FB];
    SA::template combine<FA>(al, ra[buf], av);
    SB::template combine<FB>(bl, rb[buf], bv);
#pragma unroll
    for (int i = 0; i < FA; ++i) av[i] = ok[buf] ? av[i] : 0.f;  // rows past the split: 0
#pragma unroll
    for (int i = 0; i < FA; ++i)
#pragma unroll
      for (int j = 0; j < FB; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < FA; ++i) bs[i] += av[i];
  };
  if (my_steps > 0) {
    // steps past my_steps re-read a valid row (never consumed)
    auto cl = [&](int t) { return t < my_steps ? t : my_steps - 1; };
    int t = 0;
    fetch_idx(0, 0);
    fetch_idx(cl(1), 1);
    fetch_idx(cl(2), 2);
    fetch(0);
    fetch(1);
    for (; t + 3 <= my_steps; t += 3) {
      fetch(2);
      fetch_idx(cl(t + 3), 0);
      compute(0);
      __builtin_amdgcn_sched_barrier(0);
      fetch(0);
      fetch_idx(cl(t + 4), 1);
      compute(1);
      __builtin_amdgcn_sched_barrier(0);
      fetch(1);
      fetch_idx(cl(t + 5), 2);
      compute(2);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (t < my_steps) compute(0);
    if (t + 1 < my_steps) compute(1);
  }

  // ---- fixed-order combine of the 4 waves' partial tiles: (w0 + w1) + (w2 + w3) ----
  constexpr int NV = FA * FB * 4;  // accumulator values per lane
  auto put = [&](float* dst) {
#pragma unroll
    for (int i = 0; i < FA; ++i)
#pragma unroll
      for (int j = 0; j < FB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[((i * FB + j) * 4 + r) * 64 + lane] = acc[i][j][r];
  };
  auto add = [&](const float* src) {
#pragma unroll
    for (int i = 0; i < FA; ++i) {
#pragma unroll
      for (int j = 0; j < FB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] += src[((i * FB + j) * 4 + r) * 64 + lane];
      __builtin_amdgcn_sched_barrier(0);  // bound the LDS values in flight (registers)
    }
  };
  (void)NV;
  if (w & 1) put(red[w >> 1]);
  __syncthreads();
  if (!(w & 1)) add(red[w >> 1]);
  __syncthreads();
  if (w == 2) put(red[0]);
  __syncthreads();
  if (w == 0) {
    add(red[0]);
    // slab [split][Nout][ldk]: element (n0 + FA*(4fg + r) + i, k0 + FB*fr + j)
    const int ldk = (Kout + 3) & ~3;
    float* out = slab + (int64_t)split * Nout * ldk;
    const int kc = k0 + FB * fr;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int i = 0; i < FA; ++i) {
        const int n = n0 + FA * (4 * fg + r) + i;
        if (n >= Nout) continue;
        float* o = out + (int64_t)n * ldk + kc;
        if (FB == 4 && kc + 4 <= Kout) {
          *reinterpret_cast<float4*>(o) =
              make_float4(acc[i][0][r], acc[i][1 % FB][r], acc[i][2 % FB][r], acc[i][3 % FB][r]);
        } else {
#pragma unroll
          for (int j = 0; j < FB; ++j)
            if (kc + j < Kout) o[j] = acc[i][j][r];
        }
      }
  }
  // bias column sums (tiles of the first column block): per lane sum over its rows, combined
  // over the lane groups and then the waves in fixed orders
  if (want_bias && tk == 0) {
#pragma unroll
    for (int i = 0; i < FA; ++i) {
      float v = bs[i];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      bs[i] = v;
    }
    __syncthreads();
    float* bred = red[0];
    if (fg == 0) {
#pragma unroll
      for (int i = 0; i < FA; ++i) bred[(w * FA + i) * 16 + fr] = bs[i];
    }
    __syncthreads();
    if (w == 0 && fg == 0) {
#pragma unroll
      for (int i = 0; i < FA; ++i) {
        const int n = n0 + FA * fr + i;
        const float v = (bred[(0 * FA + i) * 16 + fr] + bred[(1 * FA + i) * 16 + fr]) +
                        (bred[(2 * FA + i) * 16 + fr] + bred[(3 * FA + i) * 16 + fr]);
        if (n < Nout && n0 + FA * fr + i < n0 + TM) bslab[(int64_t)split * Nout + n] = v;
      }
    }
  }
}

// >= 64 rows (4 steps per wave) per split, splits start on 16-row boundaries
template <int FA, int FB>
inline TnPlan plan_tnr(int Nout, int Kout, int R, int target_wgs) {
  TnPlan p;
  p.tiles_n = (Nout + 16 * FA - 1) / (16 * FA);
  p.tiles_k = (Kout + 16 * FB - 1) / (16 * FB);
  tn_split(p, R, p.tiles_n * p.tiles_k, target_wgs, 64, 16);
  return p;
}

// requires Nout % FA == 0, Kout % FB == 0 (tnr_ok)
template <int FA, int FB>
inline bool tnr_ok(int Nout, int Kout) {
  return Nout >= FA && Kout >= FB && Nout % FA == 0 && Kout % FB == 0;
}
template <int FA, int FB, class AL, class BL>
inline hipError_t launch_gemm_tnr(const AL& al, const BL& bl, const TnPlan& p, float* slab,
                                  float* bslab, int Nout, int Kout, int R, bool want_bias,
                                  hipStream_t st) {
  hipLaunchKernelGGL((gemm_tnr_kernel<FA, FB, AL, BL>), dim3(p.tiles_n * p.tiles_k * p.splits),
                     dim3(TNR_WAVES * 64), 0, st, al, bl, slab, bslab, Nout, Kout, R,
                     p.rows_per_split, p.tiles_k, want_bias ? 1 : 0);
  return hipGetLastError();
}

}  // namespace cgr
