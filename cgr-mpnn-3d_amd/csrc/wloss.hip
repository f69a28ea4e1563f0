// Losses with a per-element weight: torch.nn.GaussianNLLLoss (cgr_gaussian_nll_loss_*) and the
// weighted forms of MSE / L1 / Huber (cgr_weighted_loss_*), on the two launches of loss.hip: one
// workgroup sums in a fixed order, one elementwise backward.  The loss is sum_i w_i l_i (/ n for
// the mean).  An element of weight 0 is skipped, not multiplied: it adds nothing to the sum and
// its gradients are +0.0 whatever its input, target or variance hold (NaN, inf, var <= 0) -- a
// padded slot's nll(0, 0, var) is not 0, and 0 * NaN is NaN.
//
// The Gaussian term reads mu and var with an element stride and writes their gradients with one,
// so the two columns of a [n, 2] head output (and of its gradient) are used in place.
#include "common.hpp"
#include "gnn_internal.hpp"

namespace cgr {

constexpr int kWLossThreads = 256;

__device__ __forceinline__ float wloss_block_sum(float s) {
  __shared__ float red[kWLossThreads / 64];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
static_assert(kWLossThreads == 256, "wloss_block_sum combines four waves");

// 0.5 (log v + (mu - y)^2 / v) with v = max(var, eps), + 0.5 log 2 pi when `full`
__global__ __launch_bounds__(kWLossThreads) void k_gnll_fwd(
    const float* __restrict__ mu, int64_t mu_stride, const float* __restrict__ var,
    int64_t var_stride, const float* __restrict__ y, const float* __restrict__ weight, int64_t n,
    float eps, float full_const, float scale, float* __restrict__ loss) {
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kWLossThreads) {
    const float w = weight ? weight[i] : 1.f;
    if (w == 0.f) continue;
    const float v = fmaxf(var[i * var_stride], eps);
    const float d = mu[i * mu_stride] - y[i];
    const float term = 0.5f * (logf(v) + d * d / v) + full_const;
    s += weight ? w * term : term;
  }
  s = wloss_block_sum(s);
  if (threadIdx.x == 0) loss[0] = s * scale;
}

// dmu = c (mu - y) / v ; dy = -dmu ; dvar = c 0.5 (1 / v - (mu - y)^2 / v^2), at the clamped v and
// handed to var unchanged (torch's straight-through clamp); c = w grad_loss[0] (/ n)
__global__ __launch_bounds__(kWLossThreads) void k_gnll_bwd(
    const float* __restrict__ mu, int64_t mu_stride, const float* __restrict__ var,
    int64_t var_stride, const float* __restrict__ y, const float* __restrict__ weight,
    const float* __restrict__ g, int64_t n, float eps, float scale, float* __restrict__ dmu,
    float* __restrict__ dvar, int64_t grad_stride, float* __restrict__ dy) {
  const int64_t i = (int64_t)blockIdx.x * kWLossThreads + threadIdx.x;
  if (i >= n) return;
  const float w = weight ? weight[i] : 1.f;
  float gm = 0.f, gv = 0.f;
  if (w != 0.f) {
    const float c = weight ? w * (g[0] * scale) : g[0] * scale;
    const float v = fmaxf(var[i * var_stride], eps);
    const float d = mu[i * mu_stride] - y[i];
    const float q = d / v;
    gm = c * q;
    gv = c * (0.5f * (1.f / v - q * q));
  }
  if (dmu) dmu[i * grad_stride] = gm;
  if (dvar) dvar[i * grad_stride] = gv;
  if (dy) dy[i] = 0.f - gm;  // (+0.0 at weight 0)
}

// one term of torch's MSE / L1 / Huber kernels (kind: enum cgr_weighted_loss)
__device__ __forceinline__ float wloss_term(int kind, float d, float delta) {
  if (kind == 0) return d * d;
  const float a = fabsf(d);
  if (kind == 1) return a;
  return a < delta ? 0.5f * d * d : delta * (a - 0.5f * delta);
}
// its derivative in d: the unweighted kernels' case analysis (loss.hip)
__device__ __forceinline__ float wloss_dterm(int kind, float d, float delta) {
  if (kind == 0) return 2.f * d;
  if (kind == 1) return d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f * d;  // 0 * d: NaN stays NaN
  return d < -delta ? -delta : d > delta ? delta : d;
}

__global__ __launch_bounds__(kWLossThreads) void k_wloss_fwd(
    int kind, const float* __restrict__ y, const float* __restrict__ t,
    const float* __restrict__ weight, int64_t n, float delta, float scale,
    float* __restrict__ loss) {
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kWLossThreads) {
    const float w = weight[i];
    if (w == 0.f) continue;
    s += w * wloss_term(kind, y[i] - t[i], delta);
  }
  s = wloss_block_sum(s);
  if (threadIdx.x == 0) loss[0] = s * scale;
}

__global__ __launch_bounds__(kWLossThreads) void k_wloss_bwd(
    int kind, const float* __restrict__ y, const float* __restrict__ t,
    const float* __restrict__ weight, const float* __restrict__ g, int64_t n, float delta,
    float scale, float* __restrict__ dy, float* __restrict__ dt) {
  const int64_t i = (int64_t)blockIdx.x * kWLossThreads + threadIdx.x;
  if (i >= n) return;
  const float w = weight[i];
  const float v = w == 0.f ? 0.f : w * (g[0] * scale) * wloss_dterm(kind, y[i] - t[i], delta);
  if (dy) dy[i] = v;
  if (dt) dt[i] = 0.f - v;
}

}  // namespace cgr

using namespace cgr;

static bool finite_f32(double x) { return x >= -3.4028234e38 && x <= 3.4028234e38; }  // no NaN

static int gnll_check(const std::string& w, const float* mu, int64_t mu_stride, const float* var,
                      int64_t var_stride, const float* target, int64_t n, double eps) {
  CGR_CHECK(n >= 0 && n < (1ll << 38), w + ": n out of range");
  CGR_CHECK(mu_stride >= 1 && var_stride >= 1, w + ": strides must be >= 1");
  CGR_CHECK(eps > 0.0 && finite_f32(eps) && (float)eps > 0.f, w + ": eps must be > 0 and finite");
  CGR_CHECK(n == 0 || (mu && var && target), w + ": NULL pointer");
  return 0;
}

extern "C" int cgr_gaussian_nll_loss_forward(const float* mu, int64_t mu_stride, const float* var,
                                             int64_t var_stride, const float* target,
                                             const float* weight, int64_t n,
                                             int32_t reduction_mean, int32_t full, double eps,
                                             float* loss, void* stream) {
  clear_stale_hip_error();
  const int rc = gnll_check("cgr_gaussian_nll_loss_forward", mu, mu_stride, var, var_stride,
                            target, n, eps);
  if (rc) return rc;
  CGR_CHECK(loss != nullptr, "cgr_gaussian_nll_loss_forward: NULL pointer");
  const float scale = reduction_mean ? 1.f / (float)n : 1.f;  // n == 0: 0 * inf = nan, as torch
  hipLaunchKernelGGL(k_gnll_fwd, dim3(1), dim3(kWLossThreads), 0,
                     static_cast<hipStream_t>(stream), mu, mu_stride, var, var_stride, target,
                     weight, n, (float)eps, full ? 0.91893853320467274f : 0.f, scale, loss);
  HIP_RET(hipGetLastError());
  return 0;
}

extern "C" int cgr_gaussian_nll_loss_backward(const float* mu, int64_t mu_stride, const float* var,
                                              int64_t var_stride, const float* target,
                                              const float* weight, const float* grad_loss,
                                              int64_t n, int32_t reduction_mean, double eps,
                                              float* grad_mu, float* grad_var, int64_t grad_stride,
                                              float* grad_target, void* stream) {
  clear_stale_hip_error();
  const int rc = gnll_check("cgr_gaussian_nll_loss_backward", mu, mu_stride, var, var_stride,
                            target, n, eps);
  if (rc) return rc;
  CGR_CHECK(grad_loss != nullptr, "cgr_gaussian_nll_loss_backward: NULL pointer");
  CGR_CHECK(grad_stride >= 1, "cgr_gaussian_nll_loss_backward: strides must be >= 1");
  if (n == 0 || (!grad_mu && !grad_var && !grad_target)) return 0;
  hipLaunchKernelGGL(k_gnll_bwd, dim3((unsigned)cdiv(n, kWLossThreads)), dim3(kWLossThreads), 0,
                     static_cast<hipStream_t>(stream), mu, mu_stride, var, var_stride, target,
                     weight, grad_loss, n, (float)eps, reduction_mean ? 1.f / (float)n : 1.f,
                     grad_mu, grad_var, grad_stride, grad_target);
  HIP_RET(hipGetLastError());
  return 0;
}

static int wloss_check(const std::string& w, int32_t kind, const float* input,
                       const float* target, const float* weight, int64_t n, double delta) {
  CGR_CHECK(kind >= 0 && kind <= 2, w + ": kind must be 0 (mse), 1 (l1) or 2 (huber)");
  CGR_CHECK(n >= 0 && n < (1ll << 38), w + ": n out of range");
  CGR_CHECK(kind != 2 || (delta > 0.0 && finite_f32(delta) && (float)delta > 0.f),
            w + ": delta must be > 0 and finite");
  CGR_CHECK(n == 0 || (input && target && weight), w + ": NULL pointer");
  return 0;
}

extern "C" int cgr_weighted_loss_forward(int32_t kind, const float* input, const float* target,
                                         const float* weight, int64_t n, int32_t reduction_mean,
                                         double delta, float* loss, void* stream) {
  clear_stale_hip_error();
  const int rc = wloss_check("cgr_weighted_loss_forward", kind, input, target, weight, n, delta);
  if (rc) return rc;
  CGR_CHECK(loss != nullptr, "cgr_weighted_loss_forward: NULL pointer");
  const float scale = reduction_mean ? 1.f / (float)n : 1.f;  // n == 0: 0 * inf = nan, as torch
  hipLaunchKernelGGL(k_wloss_fwd, dim3(1), dim3(kWLossThreads), 0,
                     static_cast<hipStream_t>(stream), (int)kind, input, target, weight, n,
                     (float)delta, scale, loss);
  HIP_RET(hipGetLastError());
  return 0;
}

extern "C" int cgr_weighted_loss_backward(int32_t kind, const float* input, const float* target,
                                          const float* weight, const float* grad_loss, int64_t n,
                                          int32_t reduction_mean, double delta, float* grad_input,
                                          float* grad_target, void* stream) {
  clear_stale_hip_error();
  const int rc = wloss_check("cgr_weighted_loss_backward", kind, input, target, weight, n, delta);
  if (rc) return rc;
  CGR_CHECK(grad_loss != nullptr, "cgr_weighted_loss_backward: NULL pointer");
  if (n == 0 || (!grad_input && !grad_target)) return 0;
  hipLaunchKernelGGL(k_wloss_bwd, dim3((unsigned)cdiv(n, kWLossThreads)), dim3(kWLossThreads), 0,
                     static_cast<hipStream_t>(stream), (int)kind, input, target, weight,
                     grad_loss, n, (float)delta, reduction_mean ? 1.f / (float)n : 1.f,
                     grad_input, grad_target);
  HIP_RET(hipGetLastError());
  return 0;
}
