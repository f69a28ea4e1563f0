// Split-bf16 TN GEMM for the weight gradients on the bf16 matrix cores (gfx950
// v_mfma_f32_16x16x32_bf16): C[n, k] = sum_{e in split} A(e, n) B(e, k), fp32 partial slabs.
// A is read pre-split as an e-image (b3_eimage, b3_pack.hip), B is split while it is staged.
// Shares the fragment primitives (b3_u4, b3_cvt2, b3_split8, b3_sgb, b3_mfma, b3_kperm) with the
// NT kernel of gemm_b3.hpp and nothing else; plans are TnPlan (gemm.hpp), the site table wgrad.hpp.
#pragma once

#include "gemm_b3.hpp"

namespace cgr {

// Two-piece split (x = hi + lo, hi = bf16(x), lo = bf16(x - hi)) and three terms per product
// (lo.hi, hi.lo, hi.hi; the dropped lo.lo and the residuals are <= 2^-16 |ab| per product, and a
// weight gradient sums ~10^4 of them with independent signs: fp32-level error against the fp64
// oracle, profiles/r02_split_precision_experiment.txt "b3t").  The kernel (gemm_b3tni_kernel,
// below) takes A pre-split as an e-image and stages B transposed into LDS in the NT image
// geometry ([piece][column row][4 swizzled 16-byte chunks of 8 e-rows]: every fragment read one
// conflict-free ds_read_b128; column c stored at row sigma(c), a rotation inside its 16-column
// block, so a b128 store pass hits four 64-byte bank groups).  Plans (TnPlan, gemm.hpp): one
// workgroup per (split of the e rows, k-tile of tnk fragments), all Nout columns per workgroup
// (tiles_n = 1; the launcher takes the n-fragment count from Nout); at least 2 steps (64 rows) per
// split, splits start on 32-row boundaries.
inline TnPlan plan_b3tn(int Kout, int R, int tnk, int target_wgs) {
  TnPlan p;
  p.tiles_n = 1;
  p.tiles_k = (Kout + 16 * tnk - 1) / (16 * tnk);
  tn_split(p, R, p.tiles_k, target_wgs, 64, 32);
  return p;
}

// storage row of column c: rotate by its 4-group inside the 16-column block
__device__ __forceinline__ int b3tn_sigma(int c) {
  return (c & ~3) | (((c & 3) + ((c >> 2) & 3)) & 3);
}

// Per operand kind: idx() turns a row into the element rows its loads read (the gather's index
// loads), base()/off() address load i of a job (i < NL; 32-bit element offsets, b3tn_fits checks
// the extents), get() the fp32 value of row j (float4 = the job's 4 columns).  Rows past R read
// row 0 and columns past the operand column 0 (in bounds; discarded or zero-weighted).
template <class L>
struct B3TnSrc;
template <>
struct B3TnSrc<LdPlain<4>> {
  static constexpr int NL = 8;
  static __device__ __forceinline__ void idx(const LdPlain<4>&, int row, int (&ix)[2]) {
    ix[0] = ix[1] = row;
  }
  static __device__ __forceinline__ const float* base(const LdPlain<4>& l, int, int) {
    return l.base;
  }
  static __device__ __forceinline__ uint32_t off(const LdPlain<4>& l, const int (&ix)[2], int,
                                                 int col, int K) {
    return (uint32_t)ix[0] * (uint32_t)l.ld + (uint32_t)(col < K ? col : 0);
  }
  static __device__ __forceinline__ float4 get(const float4 (&v)[16], int j) { return v[j]; }
  static bool fits(const LdPlain<4>& l, int R) { return (double)R * l.ld < 4.0e9; }
};
template <>
struct B3TnSrc<LdConcat<4>> {  // [x | s] (F % 4 == 0)
  static constexpr int NL = 8;
  static __device__ __forceinline__ void idx(const LdConcat<4>&, int row, int (&ix)[2]) {
    ix[0] = ix[1] = row;
  }
  static __device__ __forceinline__ const float* base(const LdConcat<4>& l, int, int col) {
    return col < l.F ? l.x : l.s;
  }
  static __device__ __forceinline__ uint32_t off(const LdConcat<4>& l, const int (&ix)[2], int,
                                                 int col, int K) {
    return col < l.F ? (uint32_t)ix[0] * (uint32_t)l.ldx + (uint32_t)col
                     : (uint32_t)ix[0] * (uint32_t)l.lds + (uint32_t)(col < K ? col - l.F : 0);
  }
  static __device__ __forceinline__ float4 get(const float4 (&v)[16], int j) { return v[j]; }
  static bool fits(const LdConcat<4>& l, int R) {
    return (double)R * l.ldx < 4.0e9 && (double)R * l.lds < 4.0e9;
  }
};
template <bool X>
struct B3TnSrc<LdGatherDiff<X>> {  // a[src] - h[rev]: loads 0..7 the a rows, 8..15 the h rows
  static constexpr int NL = 16;
  static __device__ __forceinline__ void idx(const LdGatherDiff<X>& l, int row, int (&ix)[2]) {
    ix[0] = l.src[row];
    ix[1] = X ? (row ^ 1) : l.rev[row];
  }
  static __device__ __forceinline__ const float* base(const LdGatherDiff<X>& l, int h, int) {
    return h ? l.h : l.a;
  }
  static __device__ __forceinline__ uint32_t off(const LdGatherDiff<X>& l, const int (&ix)[2],
                                                 int h, int col, int K) {
    return (uint32_t)ix[h] * (uint32_t)l.ld + (uint32_t)(col < K ? col : 0);
  }
  static __device__ __forceinline__ float4 get(const float4 (&v)[16], int j) {
    return f4sub(v[j], v[8 + j]);
  }
  static bool fits(const LdGatherDiff<X>& l, int R) { return (double)R * l.ld < 4.0e9; }
};

// k fragments per workgroup: 5 (H = 400: 25 -> 5 tiles exactly); 4 for more than 25 n-fragments
// (H = 512: 32 -> 8 tiles), whose accumulators would not fit beside TNK = 5 (40 B of scratch)
inline int b3tn_tnk(int Nout) { return (Nout + 15) / 16 > 25 ? 4 : 5; }
// workgroups of the layer weight gradient (A/B in the step: 128 -0.8 %, 256 -1.1 % vs 176; the
// side stream shares the GPU with the main chain, fewer splits = smaller slabs)
constexpr int kB3TnTarget = 176;
inline TnPlan b3tn_plan(int Nout, int Kout, int R, int target = kB3TnTarget) {
  return plan_b3tn(Kout, R, b3tn_tnk(Nout), target);
}
// ------------------------------------------------------------------------------------------
// TN with the n-side operand as a pre-split e-image (weight gradients dW = A^T B whose A is
// shared by every k-tile: dpre, dzn, Gs)
// ------------------------------------------------------------------------------------------
// e-image of X [R rows, C cols] (R = the TN's reduction dimension): per 32-row step s and piece p
// (0 = hi = bf16(x), 1 = lo = bf16(x - hi)) a plane of `cimg` columns x 64 bytes, column c
// holding the pieces of rows 32 s .. 32 s + 31 in order; rows >= R and columns >= C are zero.
// Written once per matrix by b3_eimage (b3_pack.hip).  An MFMA A fragment (16 columns x 32 rows)
// is then one coalesced 1 KB global load per piece: lane (fr, fg) takes column fr, rows
// 8 fg .. 8 fg + 7 -- no transposition and no split inside the GEMM (the round-2 kernel re-staged
// and re-split the whole A operand in each of its tiles_k workgroups, 5 at H = 400: 83 % of its
// staging VALU, PMC 7.6 VALU per MFMA).
struct B3EImg {
  const b3_u4* img;  // 16-byte units: ((s * 2 + p) * cimg + c) * 4 + chunk
  int cimg;          // columns, a multiple of 16
};
inline int b3_eimg_cols(int C) { return (C + 15) / 16 * 16; }
inline size_t b3_eimg_bytes(int64_t R, int C) {
  return (size_t)((R + 31) / 32) * 2 * (size_t)b3_eimg_cols(C) * 64;
}
hipError_t b3_eimage(const float* x, int64_t ld, int64_t R, int C, b3_u4* img, hipStream_t st);
// e-image of G = segsum(X) over the CSR (idx, ptr) of R segments, G never stored (b3_pack.hip);
// X rows 16-byte aligned with ld >= round_up(C, 4)
hipError_t b3_segsum_eimage(const float* x, int64_t ld, const int* idx, const int* ptr, int64_t R,
                            int C, b3_u4* img, hipStream_t st);

// The producers that write an e-image themselves (b3_pack.hip: the segmented sum, the readout
// and the top layer's backward) work in blocks of one 32-row step x kImgCols columns through an
// LDS tile [32][kImgCols + 1]: b3_tile_put stores one thread's float4 (row r, column group c4,
// absolute column col; columns >= C as 0), and after a barrier b3_tile_to_eimage, thread =
// (column, 8-row chunk), chunk fastest, splits its 8 values and writes the chunk's slot in the
// two piece planes (k_b3_eimage's store pattern: a wave's stores cover 16 consecutive 64-byte
// slots).  256 threads per block.
constexpr int kImgCols = 64;

__device__ __forceinline__ void b3_tile_put(float (&tile)[32][kImgCols + 1], int r, int c4,
                                            int col, int C, const float4& v) {
  tile[r][4 * c4 + 0] = col + 0 < C ? v.x : 0.f;
  tile[r][4 * c4 + 1] = col + 1 < C ? v.y : 0.f;
  tile[r][4 * c4 + 2] = col + 2 < C ? v.z : 0.f;
  tile[r][4 * c4 + 3] = col + 3 < C ? v.w : 0.f;
}

__device__ __forceinline__ void b3_tile_to_eimage(const float (&tile)[32][kImgCols + 1], int64_t s,
                                                  int c0, int cimg, b3_u4* __restrict__ img) {
  const int q = threadIdx.x & 3, cl = threadIdx.x >> 2;  // 64 columns x 4 chunks
  const int c = c0 + cl;
  if (c >= cimg) return;
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = tile[8 * q + j][cl];
  b3_u4 pc[2];
  b3_split8<2>(f, pc);
  img[((s * 2 + 0) * cimg + c) * 4 + q] = pc[0];
  img[((s * 2 + 1) * cimg + c) * 4 + q] = pc[1];
}

// Workgroup = CW = 8 compute waves + SW staging waves (warp-specialised: a wave runs one role for
// the whole kernel, so the registers of the two roles are not live together).
//   * compute wave w: n-fragments w, w + CW, ... (RN of them, all TNK k-fragments each) plus RX
//     of the remaining (TNN % CW) x TNK products, dealt round-robin; its A fragments come straight
//     from the e-image, one step ahead of the MFMAs (two register sets, loop unrolled by 2).
//   * staging waves: the k-side operand B (TNK x 16 columns of the tile), split into hi / lo and
//     transposed into LDS in the NT image geometry (chunk c of a column = rows 8 c .. 8 c + 7 of
//     the step, the e-image's order); a job is 4 columns x 4 rows (one 8-byte half of a chunk
//     per column and piece), so the split's VALU is spread over SW = 3 waves on three SIMDs
//     (8-row jobs on 1.25 waves: lab 40 us);  its loads are issued two intervals before they are
//     staged (two register sets) and the gather's index loads one more interval ahead.
//   * one barrier per step: compute reads LDS buffer t & 1 while staging fills (t + 1) & 1.
//   * splits start on 32-row boundaries, so a split's last step reads only its own rows or the
//     image's zero rows: A is never masked; B rows past R read row 0 (finite, times zero A).
//   * bias (column sums of A) from the pieces, hi + lo per element: n-fragment f is summed by
//     the k-tile min(f / TNK, tiles_k - 1), inside the compute wave that loads f (the remainder
//     fragments by the wave holding their k-fragment-0 product).
template <int TNN, int TNK>
struct B3TniShape {
  static constexpr int CW = 8;
  static constexpr int BC = TNK * 16;
  static constexpr int JC = BC / 4;  // 4-column groups
  static constexpr int JB = JC * 8;  // staging jobs: 4 columns x 4 rows (half an 8-row chunk)
  static constexpr int SW = (JB + 63) / 64;
  static constexpr int NT = (CW + SW) * 64;
  static constexpr int RN = TNN / CW;
  static constexpr int REM = (TNN % CW) * TNK;
  static constexpr int RX = (REM + CW - 1) / CW;
  static constexpr int NA = RN + RX;        // A fragments a compute wave loads per step
  static constexpr int SU4 = 2 * BC * 4;    // b3_u4 per LDS stage buffer
  static constexpr size_t LDS_BYTES = (size_t)2 * SU4 * 16;
};

// prev (slab == null: none): the previous weight gradient's split-K slabs, reduced by this
// launch's threads before their own work (the launch-boundary reduce: no reduce launch, and the
// slab read overlaps other workgroups' main loops; prev's slabs are not this launch's)
template <int TNN, int TNK, class BL>
__global__ __launch_bounds__((B3TniShape<TNN, TNK>::NT)) void gemm_b3tni_kernel(
    B3EImg ai, BL bl, float* __restrict__ slab, float* __restrict__ bslab, int Nout, int Kout,
    int R, int rows_per_split, int tiles_k, int want_bias, RedJob prev) {
  typedef B3TnSrc<BL> TB;
  using S = B3TniShape<TNN, TNK>;
  constexpr int CW = S::CW, RN = S::RN, RX = S::RX, NA = S::NA, BC = S::BC, SU4 = S::SU4;
  constexpr int JB = S::JB;
  extern __shared__ b3_u4 b3_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fg = lane >> 4;
  CGR_STAMP_BEGIN();
#ifdef CGR_STAMPS
  // diagnostic: per step, the cycles a wave works and the cycles it waits at the step barrier, for
  // compute wave 0 (slots 1, 2) and staging wave 0 (slots 3, 4); slot 5 = main loop end
  unsigned long long st_work = 0, st_wait = 0, st_prev = 0, st_t = 0;
  const bool st_me = tid == 0 || tid == CW * 64;
#define TN_STAMP_PRE() do { if (st_me) { st_t = ::cgr::stamp_now(); st_work += st_t - st_prev; } } while (0)
#define TN_STAMP_POST() do { if (st_me) { st_prev = ::cgr::stamp_now(); st_wait += st_prev - st_t; } } while (0)
#define TN_STAMP_START() do { if (st_me) st_prev = ::cgr::stamp_now(); } while (0)
#else
#define TN_STAMP_PRE() ((void)0)
#define TN_STAMP_POST() ((void)0)
#define TN_STAMP_START() ((void)0)
#endif
  if (prev.slab) {
    const int64_t tot = reduce_items(prev);
    for (int64_t f = (int64_t)blockIdx.x * S::NT + tid; f < tot; f += (int64_t)gridDim.x * S::NT)
      reduce_slab_item(prev, f);
  }
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int split = lin / tiles_k, tkk = lin - split * tiles_k;
  const int k0 = tkk * TNK * 16;
  const int e_begin = split * rows_per_split;  // a multiple of 32
  const int e_end = min(R, e_begin + rows_per_split);
  const int nt = e_end > e_begin ? (e_end - e_begin + 31) / 32 : 0;

  // staging waves win the SIMD's issue arbitration against the compute wave they share it with
  // (static priority, no per-step flips: cdna_hip_programming.md T5; step A/B +0.5 %,
  // profiles/r03_fold_ab_cfg2.txt)
  if (w >= CW) __builtin_amdgcn_s_setprio(1);
  if (w >= CW) {
    // ================= staging waves: B of step t + 1 into LDS buffer (t + 1) & 1 =============
    // job (4-column group cg, 4-row group hc): rows 4 hc .. 4 hc + 3 of a step, half of the
    // 16-byte chunk hc / 2 of each column (the e-image's row order); lanes run column groups
    // fastest, so a load instruction covers ~3 rows x 320 contiguous bytes
    constexpr int JC = S::JC;
    const int q = tid - CW * 64;
    const bool act = q < JB;
    const int hc = act ? q / JC : 0;
    const int jcol = (act ? q - hc * JC : 0) * 4;  // first of the job's 4 columns in the tile
    const int gcol = k0 + jcol;
    const float* base0 = TB::base(bl, 0, gcol);
    const float* base1 = TB::base(bl, 1, gcol);
    // two register sets: rows j < 4 of a / plain rows in r[j], gathered h rows in r[8 + j]
    float4 raw0[16], raw1[16];
    uint32_t off[TB::NL];
    int ix[4][2];
    auto rowof = [&](int t, int j) {
      const int e = e_begin + t * 32 + 4 * hc + j;
      return e < R ? e : 0;
    };
    auto index = [&](int t) {  // the gather's index loads of step t
#pragma unroll
      for (int j = 0; j < 4; ++j) TB::idx(bl, rowof(t, j), ix[j]);
    };
    auto fetch = [&](float4 (&raw)[16]) {  // addresses from the last index(), then the loads
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int h = 0; h < TB::NL / 8; ++h) off[8 * h + j] = TB::off(bl, ix[j], h, gcol, Kout);
#pragma unroll
      for (int i = 0; i < 4; ++i) raw[i] = *reinterpret_cast<const float4*>(base0 + off[i]);
      if constexpr (TB::NL == 16) {
#pragma unroll
        for (int i = 8; i < 12; ++i) raw[i] = *reinterpret_cast<const float4*>(base1 + off[i]);
      }
    };
    typedef uint32_t u2v __attribute__((ext_vector_type(2)));
    auto put = [&](b3_u4* img, int t, float f0, float f1, float f2, float f3) {
      float a0, a1, a2, a3, c0, c1, c2, c3;
      const uint32_t h01 = b3_cvt2(f0, f1, a0, a1), h23 = b3_cvt2(f2, f3, a2, a3);
      const uint32_t l01 = b3_cvt2(f0 - a0, f1 - a1, c0, c1), l23 = b3_cvt2(f2 - a2, f3 - a3, c2, c3);
      const int row = b3tn_sigma(jcol + t);
      const int slot = (hc >> 1) ^ lds_swz(row);
      char* b = reinterpret_cast<char*>(img) + 8 * (hc & 1);
      *reinterpret_cast<u2v*>(b + (row * 4 + slot) * 16) = u2v{h01, h23};
      *reinterpret_cast<u2v*>(b + ((BC + row) * 4 + slot) * 16) = u2v{l01, l23};
    };
    auto stage = [&](const float4 (&raw)[16], int buf) {
      b3_u4* img = b3_lds + buf * SU4;
      float4 u[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] = TB::get(raw, j);
      if (act) {
        put(img, 0, u[0].x, u[1].x, u[2].x, u[3].x);
        put(img, 1, u[0].y, u[1].y, u[2].y, u[3].y);
        put(img, 2, u[0].z, u[1].z, u[2].z, u[3].z);
        put(img, 3, u[0].w, u[1].w, u[2].w, u[3].w);
      }
    };
    if (nt > 0) {
      index(0);
      fetch(raw0);  // step 0
      index(1);
      fetch(raw1);  // step 1
      index(2);
      stage(raw0, 0);
      fetch(raw0);  // step 2
      index(3);
      __syncthreads();
      TN_STAMP_START();
      // interval t (compute on step t): stage step t + 1, whose loads were issued two intervals
      // ago, then issue step t + 3's into the freed set (index loads one interval ahead of them)
      for (int t = 0; t < nt; t += 2) {
        if (t + 1 < nt) stage(raw1, 1);
        fetch(raw1);  // step t + 3
        index(t + 4);
        TN_STAMP_PRE();
        __syncthreads();
        TN_STAMP_POST();
        if (t + 1 >= nt) break;
        if (t + 2 < nt) stage(raw0, 0);
        fetch(raw0);  // step t + 4
        index(t + 5);
        TN_STAMP_PRE();
        __syncthreads();
        TN_STAMP_POST();
      }
    }
#ifdef CGR_STAMPS
    if (tid == CW * 64) {
      ::cgr::stamp_val(3, st_work);
      ::cgr::stamp_val(4, st_wait);
    }
#endif
    CGR_STAMP_END(0x4000 | TNN);
    return;
  }

  // ================= compute waves =================
  const int rrow = b3tn_sigma(fr);  // fragment reads: storage row of column fr of a block
  const int sw = fg ^ lds_swz(rrow);
  // this wave's A fragments: f < RN: n-fragment w + f CW; f >= RN: remainder product xq(f - RN)
  auto xq = [&](int x) {
    const int qq = w + x * CW;
    return qq < S::REM ? qq : 0;
  };
  auto frag_n = [&](int f) { return f < RN ? w + f * CW : RN * CW + xq(f - RN) / TNK; };
  // bias ownership (k-tile of n-fragment f) and, for remainder products, k-fragment 0 only
  bool own[NA];
#pragma unroll
  for (int f = 0; f < NA; ++f) {
    const int n = frag_n(f);
    const int tile = min(n / TNK, tiles_k - 1);
    own[f] = want_bias && tile == tkk && n < TNN &&
             (f < RN || (w + (f - RN) * CW < S::REM && xq(f - RN) % TNK == 0));
  }
  float bsum[NA];
#pragma unroll
  for (int f = 0; f < NA; ++f) bsum[f] = 0.f;
  const int s0 = e_begin / 32;
  auto aload = [&](int t, b3_u4 (&a)[NA][2]) {
    const int s = s0 + (t < nt ? t : nt - 1);
    const b3_u4* base = ai.img + (size_t)s * 2 * ai.cimg * 4;
#pragma unroll
    for (int f = 0; f < NA; ++f) {
      const int c = min(frag_n(f) * 16 + fr, ai.cimg - 1);  // fragments past the image: discarded
      a[f][0] = base[c * 4 + fg];
      a[f][1] = base[(ai.cimg + c) * 4 + fg];
    }
  };
  floatx4 acc[RN > 0 ? RN : 1][TNK], accx[RX > 0 ? RX : 1];
#pragma unroll
  for (int i = 0; i < RN; ++i)
#pragma unroll
    for (int j = 0; j < TNK; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int x = 0; x < RX; ++x) accx[x] = floatx4{0.f, 0.f, 0.f, 0.f};
  auto compute = [&](int buf, const b3_u4 (&a)[NA][2]) {
    const b3_u4* img = b3_lds + buf * SU4;
#pragma unroll
    for (int x = 0; x < RX; ++x) {
      const int rb = (xq(x) % TNK) * 16 + rrow;
      const b3_u4 xbh = img[rb * 4 + sw], xbl = img[(BC + rb) * 4 + sw];
      floatx4 c = accx[x];
      c = b3_mfma(a[RN + x][1], xbh, c);
      c = b3_mfma(a[RN + x][0], xbl, c);
      accx[x] = b3_mfma(a[RN + x][0], xbh, c);
    }
#pragma unroll
    for (int j = 0; j < TNK; ++j) {
      if constexpr (RN > 0) {
        const int row = j * 16 + rrow;
        const b3_u4 bh = img[row * 4 + sw], bl_ = img[(BC + row) * 4 + sw];
#pragma unroll
        for (int i = 0; i < RN; ++i) {
          floatx4 c = acc[i][j];
          c = b3_mfma(a[i][1], bh, c);
          c = b3_mfma(a[i][0], bl_, c);
          acc[i][j] = b3_mfma(a[i][0], bh, c);
        }
      }
    }
#pragma unroll
    for (int f = 0; f < NA; ++f)
      if (own[f]) {  // sum of hi + lo over the lane's 8 rows
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t h = a[f][0][k], l = a[f][1][k];
          s += (__uint_as_float(h << 16) + __uint_as_float(l << 16)) +
               (__uint_as_float(h & 0xffff0000u) + __uint_as_float(l & 0xffff0000u));
        }
        bsum[f] += s;
      }
  };
  if (nt > 0) {
    b3_u4 a0[NA][2], a1[NA][2];
    aload(0, a0);
    __syncthreads();  // B(0) staged
    TN_STAMP_START();
    for (int t = 0; t < nt; t += 2) {
      aload(t + 1, a1);
      __builtin_amdgcn_sched_barrier(0);
      compute(0, a0);
      TN_STAMP_PRE();
      __syncthreads();
      TN_STAMP_POST();
      if (t + 1 >= nt) break;
      aload(t + 2, a0);
      __builtin_amdgcn_sched_barrier(0);
      compute(1, a1);
      TN_STAMP_PRE();
      __syncthreads();
      TN_STAMP_POST();
    }
  }
#ifdef CGR_STAMPS
  if (tid == 0) {
    ::cgr::stamp_val(1, st_work);
    ::cgr::stamp_val(2, st_wait);
    ::cgr::stamp_val(5, ::cgr::stamp_now());
  }
#endif

  // ---- epilogue: accumulators straight to the slab (rows n = 16 nf + 4 fg + r, columns
  // k0 + 16 j + fr: 64 contiguous bytes per row and register) ----
  const int ldk = (Kout + 3) & ~3;
  float* out = slab + (int64_t)split * Nout * ldk;
  auto store = [&](int nf, int kf, const floatx4& c) {
    const int col = k0 + kf * 16 + fr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = nf * 16 + fg * 4 + r;
      if (row < Nout && col < Kout) out[(int64_t)row * ldk + col] = c[r];
    }
  };
#pragma unroll
  for (int i = 0; i < RN; ++i)
#pragma unroll
    for (int j = 0; j < TNK; ++j) store(w + i * CW, j, acc[i][j]);
#pragma unroll
  for (int x = 0; x < RX; ++x) {
    const int qq = w + x * CW;
    if (qq < S::REM) store(RN * CW + qq / TNK, qq % TNK, accx[x]);
  }
  if (want_bias) {
#pragma unroll
    for (int f = 0; f < NA; ++f) {
      float v = bsum[f];
      v += __shfl_xor(v, 16, 64);  // (g0 + g1), (g2 + g3)
      v += __shfl_xor(v, 32, 64);  // (g0 + g1) + (g2 + g3), the same in every group
      const int n = frag_n(f) * 16 + fr;
      if (own[f] && fg == 0 && n < Nout) bslab[(int64_t)split * Nout + n] = v;
    }
  }
  CGR_STAMP_END(0x4000 | TNN);
}
#undef TN_STAMP_PRE
#undef TN_STAMP_POST
#undef TN_STAMP_START

// splits of the e-image TN: rows_per_split a multiple of 32 (plan_b3tn rounds it)
template <int TNN, int TNK, class BL>
inline hipError_t launch_b3tni_t(const B3EImg& ai, const BL& bl, const TnPlan& p, float* slab,
                                 float* bslab, int Nout, int Kout, int R, bool want_bias,
                                 hipStream_t st, const RedJob& prev) {
  using S = B3TniShape<TNN, TNK>;
  auto kern = gemm_b3tni_kernel<TNN, TNK, BL>;
  static LdsLimit lim;
  const hipError_t e = lim.ensure(reinterpret_cast<const void*>(kern), (int)S::LDS_BYTES);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(p.tiles_k * p.splits), dim3(S::NT), S::LDS_BYTES, st, ai, bl,
                     slab, bslab, Nout, Kout, R, p.rows_per_split, p.tiles_k, want_bias ? 1 : 0,
                     prev);
  return hipGetLastError();
}

// the e-image TN covers Nout up to 32 fragments (H <= 512) and B operands whose extents fit the
// 32-bit element offsets; A = the e-image of an [R, >= Nout] matrix
template <class BL>
inline bool b3tni_ok(const BL& bl, int Nout, int R) {
  const int t = (Nout + 15) / 16;
  return t >= 1 && t <= 32 && B3TnSrc<BL>::fits(bl, R);
}

template <class BL>
inline hipError_t launch_b3tni(const B3EImg& ai, const BL& bl, const TnPlan& p, float* slab,
                               float* bslab, int Nout, int Kout, int R, bool want_bias,
                               hipStream_t st, const RedJob& prev = RedJob{}) {
  constexpr int TNK = 5;
  if (!b3tni_ok(bl, Nout, R) || p.rows_per_split % 32) return hipErrorInvalidValue;
  if (p.tiles_k != (Kout + 16 * b3tn_tnk(Nout) - 1) / (16 * b3tn_tnk(Nout)))
    return hipErrorInvalidValue;  // a plan from b3tn_plan
  // the smallest instantiated fragment count that covers Nout (25 at H = 400 and 32 at H = 512
  // exactly; extra fragments read the image's zero columns and are not stored)
  const int t = (Nout + 15) / 16;
  if (t <= 2) return launch_b3tni_t<2, TNK>(ai, bl, p, slab, bslab, Nout, Kout, R, want_bias, st, prev);
  if (t <= 4) return launch_b3tni_t<4, TNK>(ai, bl, p, slab, bslab, Nout, Kout, R, want_bias, st, prev);
  if (t <= 8) return launch_b3tni_t<8, TNK>(ai, bl, p, slab, bslab, Nout, Kout, R, want_bias, st, prev);
  if (t <= 16) return launch_b3tni_t<16, TNK>(ai, bl, p, slab, bslab, Nout, Kout, R, want_bias, st, prev);
  if (t <= 25) return launch_b3tni_t<25, TNK>(ai, bl, p, slab, bslab, Nout, Kout, R, want_bias, st, prev);
  return launch_b3tni_t<32, 4>(ai, bl, p, slab, bslab, Nout, Kout, R, want_bias, st, prev);
}

}  // namespace cgr
