// Mean-variance head on the pooled fingerprint (cgr_meanvar_head_forward / _backward):
//   mu[b] = g[b].w_mu + b_mu ; raw[b] = g[b].w_var + b_var ; var[b] = softplus(raw[b]) + min_var
// written interleaved, out[b] = (mu[b], var[b]), with torch's softplus (beta 1, threshold 20).
// Forward: one wave per row, its lanes over the columns, wave_sum -- a row's result depends on
// that row only.  Backward: the k_head_bwd shape (kernels.hip), a workgroup of 16 float4 column
// groups x 16 row phases: every thread writes the dg elements of its (rows, column group) and
// accumulates its dW share in row order, then the 16 phases are summed in phase order through
// LDS.  No atomics: every result is reproducible, and a row of out / dg is the same bits computed
// alone or inside any batch.
//
// Rows of g (stride ldg) and dg (stride H) are only 4-byte aligned when the stride is not a
// multiple of 4 (GNN.encode hands rows of stride H).  VEC: every base 16-byte aligned and H, ldg
// multiples of 4 -> float4 accesses; else element by element.  Both forms give a thread the same
// columns, so the results are the same bits in either.
#include "common.hpp"
#include "gnn_internal.hpp"

namespace cgr {

constexpr int kMvFwdThreads = 256;
constexpr int kMvFwdRows = kMvFwdThreads / 64;  // one wave per row
constexpr int kMvCols = 16;                     // float4 column groups of a backward workgroup
constexpr int kMvPhases = 16;                   // row phases of a backward workgroup
constexpr int kMvBwdThreads = kMvCols * kMvPhases;

__device__ __forceinline__ float mv_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
// d softplus / dx as torch's backward writes it: z / (z + 1) with z = exp(x), 1 past the threshold
__device__ __forceinline__ float mv_softplus_grad(float x) {
  const float z = expf(x);
  return x > 20.f ? 1.f : z / (z + 1.f);
}

template <bool VEC>
__global__ __launch_bounds__(kMvFwdThreads) void k_meanvar_fwd(
    const float* __restrict__ g, int64_t ldg, int64_t B, int H, const float* __restrict__ w_mu,
    const float* __restrict__ b_mu, const float* __restrict__ w_var,
    const float* __restrict__ b_var, float min_var, float* __restrict__ out,
    float* __restrict__ raw) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * kMvFwdRows + (threadIdx.x >> 6);
  if (b >= B) return;  // (uniform over the wave; no barrier follows)
  const float* row = g + b * ldg;
  float am = 0.f, av = 0.f;
  for (int k = 4 * lane; k < H; k += 256) {
    const float4 x = load4<VEC ? 4 : 1>(row + k, H - k);
    const float4 m = load4<VEC ? 4 : 1>(w_mu + k, H - k);
    const float4 v = load4<VEC ? 4 : 1>(w_var + k, H - k);
    am = fmaf(x.x, m.x, am);
    am = fmaf(x.y, m.y, am);
    am = fmaf(x.z, m.z, am);
    am = fmaf(x.w, m.w, am);
    av = fmaf(x.x, v.x, av);
    av = fmaf(x.y, v.y, av);
    av = fmaf(x.z, v.z, av);
    av = fmaf(x.w, v.w, av);
  }
  am = wave_sum(am);
  av = wave_sum(av);
  if (lane == 0) {
    const float r = av + (b_var ? b_var[0] : 0.f);
    out[2 * b] = am + (b_mu ? b_mu[0] : 0.f);
    out[2 * b + 1] = mv_softplus(r) + min_var;
    if (raw) raw[b] = r;
  }
}

// dg[b] = dout[b, 0] w_mu + draw[b] w_var with draw[b] = dout[b, 1] softplus'(raw[b]);
// dW[0] = sum_b dout[b, 0] g[b], dW[1] = sum_b draw[b] g[b] ;
// db = (sum_b dout[b, 0], sum_b draw[b]).  dg, dW, db each nullable (g is read only for dW).
template <bool VEC>
__global__ __launch_bounds__(kMvBwdThreads) void k_meanvar_bwd(
    const float* __restrict__ g, int64_t ldg, int64_t B, int H, const float* __restrict__ w_mu,
    const float* __restrict__ w_var, const float* __restrict__ raw,
    const float* __restrict__ dout, float* __restrict__ dg, float* __restrict__ dW,
    float* __restrict__ db) {
  __shared__ float4 red[2][kMvPhases][kMvCols];
  const int tx = threadIdx.x % kMvCols, ty = threadIdx.x / kMvCols;
  const int k = 4 * (blockIdx.x * kMvCols + tx);
  const float4 wm = load4<VEC ? 4 : 1>(w_mu + k, H - k), wv = load4<VEC ? 4 : 1>(w_var + k, H - k);
  float4 a0 = f4zero(), a1 = f4zero();
  float s0 = 0.f, s1 = 0.f;
  for (int64_t b = ty; b < B; b += kMvPhases) {
    const float d0 = dout[2 * b];
    const float d1 = dout[2 * b + 1] * mv_softplus_grad(raw[b]);
    s0 += d0;
    s1 += d1;
    if (k >= H) continue;
    if (dg) {
      const float4 r = make_float4(fmaf(d1, wv.x, d0 * wm.x), fmaf(d1, wv.y, d0 * wm.y),
                                   fmaf(d1, wv.z, d0 * wm.z), fmaf(d1, wv.w, d0 * wm.w));
      float* drow = dg + b * H;
      if constexpr (VEC) {
        *reinterpret_cast<float4*>(drow + k) = r;
      } else {
        const float rv[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (k + q < H) drow[k + q] = rv[q];
      }
    }
    if (dW) {
      const float4 x = load4<VEC ? 4 : 1>(g + b * ldg + k, H - k);
      a0 = make_float4(fmaf(d0, x.x, a0.x), fmaf(d0, x.y, a0.y), fmaf(d0, x.z, a0.z),
                       fmaf(d0, x.w, a0.w));
      a1 = make_float4(fmaf(d1, x.x, a1.x), fmaf(d1, x.y, a1.y), fmaf(d1, x.z, a1.z),
                       fmaf(d1, x.w, a1.w));
    }
  }
  if (dW) {
    red[0][ty][tx] = a0;
    red[1][ty][tx] = a1;
    __syncthreads();
    if (ty < 2 && k < H) {  // phase 0 sums dW[0]'s column group, phase 1 dW[1]'s
      float4 s = red[ty][0][tx];
#pragma unroll
      for (int p = 1; p < kMvPhases; ++p) s = f4add(s, red[ty][p][tx]);
      const float sv[4] = {s.x, s.y, s.z, s.w};
      float* wrow = dW + (int64_t)ty * H;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (k + q < H) wrow[k + q] = sv[q];
    }
  }
  if (db && blockIdx.x == 0) {  // (uniform over the workgroup)
    __syncthreads();
    if (tx == 0) red[0][ty][0] = make_float4(s0, s1, 0.f, 0.f);  // every tx summed the same rows
    __syncthreads();
    if (threadIdx.x == 0) {
      float t0 = red[0][0][0].x, t1 = red[0][0][0].y;
#pragma unroll
      for (int p = 1; p < kMvPhases; ++p) {
        t0 += red[0][p][0].x;
        t1 += red[0][p][0].y;
      }
      db[0] = t0;
      db[1] = t1;
    }
  }
}

static bool mv_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace cgr

using namespace cgr;

static int meanvar_check(const char* what, const float* g, int64_t ldg, int64_t B, int64_t H,
                         const float* w_mu, const float* w_var) {
  const std::string w(what);
  CGR_CHECK(H > 0 && H < (1ll << 30), w + ": H must be >= 1");
  CGR_CHECK(ldg >= H, w + ": ldg < H");
  CGR_CHECK(B >= 0 && B < (1ll << 31), w + ": B out of range");
  CGR_CHECK(w_mu != nullptr && w_var != nullptr && (B == 0 || g != nullptr), w + ": NULL pointer");
  return 0;
}

extern "C" int cgr_meanvar_head_forward(const float* g, int64_t ldg, int64_t B, int64_t H,
                                        const float* w_mu, const float* b_mu, const float* w_var,
                                        const float* b_var, double min_var, float* out,
                                        float* raw, void* stream) {
  clear_stale_hip_error();
  const int rc = meanvar_check("cgr_meanvar_head_forward", g, ldg, B, H, w_mu, w_var);
  if (rc) return rc;
  CGR_CHECK(min_var >= 0.0 && min_var <= 3.4028234e38,  // (false for NaN)
            "cgr_meanvar_head_forward: min_var must be >= 0 and finite");
  CGR_CHECK(B == 0 || out != nullptr, "cgr_meanvar_head_forward: NULL pointer");
  if (B == 0) return 0;
  const bool vec = H % 4 == 0 && ldg % 4 == 0 && mv_aligned16(g) && mv_aligned16(w_mu) &&
                   mv_aligned16(w_var);
  const dim3 grid((unsigned)cdiv(B, kMvFwdRows)), block(kMvFwdThreads);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL(k_meanvar_fwd<true>, grid, block, 0, st, g, ldg, B, (int)H, w_mu, b_mu,
                       w_var, b_var, (float)min_var, out, raw);
  else
    hipLaunchKernelGGL(k_meanvar_fwd<false>, grid, block, 0, st, g, ldg, B, (int)H, w_mu, b_mu,
                       w_var, b_var, (float)min_var, out, raw);
  HIP_RET(hipGetLastError());
  return 0;
}

extern "C" int cgr_meanvar_head_backward(const float* g, int64_t ldg, int64_t B, int64_t H,
                                         const float* w_mu, const float* w_var, const float* raw,
                                         const float* dout, float* dg, float* dW, float* db,
                                         void* stream) {
  clear_stale_hip_error();
  const int rc = meanvar_check("cgr_meanvar_head_backward", g, ldg, B, H, w_mu, w_var);
  if (rc) return rc;
  CGR_CHECK(B == 0 || (raw != nullptr && dout != nullptr),
            "cgr_meanvar_head_backward: NULL pointer");
  if (!dg && !dW && !db) return 0;
  const bool vec = H % 4 == 0 && ldg % 4 == 0 && mv_aligned16(g) && mv_aligned16(w_mu) &&
                   mv_aligned16(w_var) && (!dg || mv_aligned16(dg));
  // B == 0: the sums over no rows, exact zeros, from the same launch
  const dim3 grid((unsigned)cdiv(H, 4 * kMvCols)), block(kMvBwdThreads);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL(k_meanvar_bwd<true>, grid, block, 0, st, g, ldg, B, (int)H, w_mu, w_var,
                       raw, dout, dg, dW, db);
  else
    hipLaunchKernelGGL(k_meanvar_bwd<false>, grid, block, 0, st, g, ldg, B, (int)H, w_mu, w_var,
                       raw, dout, dg, dW, db);
  HIP_RET(hipGetLastError());
  return 0;
}
