// The training step's loss, torch.nn.MSELoss(reduction="sum") as train.py:120 builds it and
// trainer.py:142-143 applies it to the model's predictions: forward and backward each one launch
// (torch: elementwise + reduce forward, fill + elementwise backward).  Deterministic: one
// workgroup sums in a fixed order.
#include "common.hpp"
#include "gnn_internal.hpp"

namespace cgr {

constexpr int kLossThreads = 256;

__global__ __launch_bounds__(kLossThreads) void k_mse_fwd(const float* __restrict__ y,
                                                          const float* __restrict__ t, int64_t n,
                                                          float scale, float* __restrict__ loss) {
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kLossThreads) {
    const float d = y[i] - t[i];
    s += d * d;
  }
  __shared__ float red[kLossThreads / 64];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = ((red[0] + red[1]) + (red[2] + red[3])) * scale;
}

// dy = scale2 (y - t) g  (scale2 = 2, or 2 / n for the mean); dt = -dy when requested
__global__ __launch_bounds__(kLossThreads) void k_mse_bwd(const float* __restrict__ y,
                                                          const float* __restrict__ t,
                                                          const float* __restrict__ g, int64_t n,
                                                          float scale2, float* __restrict__ dy,
                                                          float* __restrict__ dt) {
  const int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
  if (i >= n) return;
  const float v = scale2 * (y[i] - t[i]) * g[0];
  if (dy) dy[i] = v;
  if (dt) dt[i] = -v;
}

// torch.nn.L1Loss and torch.nn.HuberLoss(delta) on the same two launches: `delta` < 0 selects L1.
// One term, as torch's kernels write it (huber: |d| < delta ? d^2 / 2 : delta (|d| - delta / 2)).
__device__ __forceinline__ float robust_term(float d, float delta) {
  const float a = fabsf(d);
  if (delta < 0.f) return a;
  return a < delta ? 0.5f * d * d : delta * (a - 0.5f * delta);
}

__global__ __launch_bounds__(kLossThreads) void k_robust_fwd(const float* __restrict__ y,
                                                             const float* __restrict__ t,
                                                             int64_t n, float delta, float scale,
                                                             float* __restrict__ loss) {
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kLossThreads) s += robust_term(y[i] - t[i], delta);
  __shared__ float red[kLossThreads / 64];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = ((red[0] + red[1]) + (red[2] + red[3])) * scale;
}

// L1: dy = sign(d) (g / denom), 0 at d == 0.  Huber: dy = (norm d) g inside [-delta, delta],
// +-(norm delta) g outside (norm = 1 / denom; the operation order is torch's on both).  denom = 1
// or n (the mean); dt = -dy when requested
__global__ __launch_bounds__(kLossThreads) void k_robust_bwd(const float* __restrict__ y,
                                                             const float* __restrict__ t,
                                                             const float* __restrict__ g, int64_t n,
                                                             float delta, float denom,
                                                             float* __restrict__ dy,
                                                             float* __restrict__ dt) {
  const int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
  if (i >= n) return;
  const float d = y[i] - t[i];
  float v;
  if (delta < 0.f) {
    const float gs = g[0] / denom;
    v = d > 0.f ? gs : d < 0.f ? -gs : 0.f * gs;  // 0 * gs: a NaN gradient stays NaN, as torch
  } else {
    const float norm = 1.f / denom;
    v = d < -delta ? -norm * g[0] * delta : d > delta ? norm * g[0] * delta : norm * d * g[0];
  }
  if (dy) dy[i] = v;
  if (dt) dt[i] = -v;
}

}  // namespace cgr

using namespace cgr;

static int robust_forward(const char* what, const float* input, const float* target, int64_t n,
                          int32_t reduction_mean, float delta, float* loss, void* stream) {
  clear_stale_hip_error();
  CGR_CHECK(n >= 0 && loss && (n == 0 || (input && target)), std::string(what) + ": bad args");
  const float scale = reduction_mean ? 1.f / (float)n : 1.f;  // n == 0: 0 * inf = nan, as torch
  hipLaunchKernelGGL(k_robust_fwd, dim3(1), dim3(kLossThreads), 0,
                     static_cast<hipStream_t>(stream), input, target, n, delta, scale, loss);
  HIP_RET(hipGetLastError());
  return 0;
}

static int robust_backward(const char* what, const float* input, const float* target,
                           const float* grad_loss, int64_t n, int32_t reduction_mean, float delta,
                           float* grad_input, float* grad_target, void* stream) {
  clear_stale_hip_error();
  CGR_CHECK(n >= 0 && grad_loss && (n == 0 || (input && target)),
            std::string(what) + ": bad args");
  if (n == 0 || (!grad_input && !grad_target)) return 0;
  const int64_t blocks = (n + kLossThreads - 1) / kLossThreads;
  CGR_CHECK(blocks < (1LL << 31), std::string(what) + ": n too large");
  hipLaunchKernelGGL(k_robust_bwd, dim3((unsigned)blocks), dim3(kLossThreads), 0,
                     static_cast<hipStream_t>(stream), input, target, grad_loss, n, delta,
                     reduction_mean ? (float)n : 1.f, grad_input, grad_target);
  HIP_RET(hipGetLastError());
  return 0;
}

extern "C" int cgr_l1_loss_forward(const float* input, const float* target, int64_t n,
                                   int32_t reduction_mean, float* loss, void* stream) {
  return robust_forward("cgr_l1_loss_forward", input, target, n, reduction_mean, -1.f, loss,
                        stream);
}

extern "C" int cgr_l1_loss_backward(const float* input, const float* target,
                                    const float* grad_loss, int64_t n, int32_t reduction_mean,
                                    float* grad_input, float* grad_target, void* stream) {
  return robust_backward("cgr_l1_loss_backward", input, target, grad_loss, n, reduction_mean,
                         -1.f, grad_input, grad_target, stream);
}

// delta > 0 and finite in fp32 (a delta that rounds to 0 or to infinity would silently be L1-like
// or MSE / 2)
static bool huber_delta_ok(double delta) {
  const float f = (float)delta;
  return delta > 0.0 && f > 0.f && f <= 3.4028234e38f;
}

extern "C" int cgr_huber_loss_forward(const float* input, const float* target, int64_t n,
                                      int32_t reduction_mean, double delta, float* loss,
                                      void* stream) {
  CGR_CHECK(huber_delta_ok(delta), "cgr_huber_loss_forward: delta must be > 0 and finite");
  return robust_forward("cgr_huber_loss_forward", input, target, n, reduction_mean, (float)delta,
                        loss, stream);
}

extern "C" int cgr_huber_loss_backward(const float* input, const float* target,
                                       const float* grad_loss, int64_t n, int32_t reduction_mean,
                                       double delta, float* grad_input, float* grad_target,
                                       void* stream) {
  CGR_CHECK(huber_delta_ok(delta), "cgr_huber_loss_backward: delta must be > 0 and finite");
  return robust_backward("cgr_huber_loss_backward", input, target, grad_loss, n, reduction_mean,
                         (float)delta, grad_input, grad_target, stream);
}

extern "C" int cgr_mse_loss_forward(const float* input, const float* target, int64_t n,
                                    int32_t reduction_mean, float* loss, void* stream) {
  clear_stale_hip_error();
  CGR_CHECK(n >= 0 && loss && (n == 0 || (input && target)), "cgr_mse_loss_forward: bad args");
  const float scale = reduction_mean ? 1.f / (float)n : 1.f;  // n == 0: 0 * inf = nan, as torch
  hipLaunchKernelGGL(k_mse_fwd, dim3(1), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     input, target, n, scale, loss);
  HIP_RET(hipGetLastError());
  return 0;
}

extern "C" int cgr_mse_loss_backward(const float* input, const float* target,
                                     const float* grad_loss, int64_t n, int32_t reduction_mean,
                                     float* grad_input, float* grad_target, void* stream) {
  clear_stale_hip_error();
  CGR_CHECK(n >= 0 && grad_loss && (n == 0 || (input && target)),
            "cgr_mse_loss_backward: bad args");
  if (n == 0 || (!grad_input && !grad_target)) return 0;
  const float scale2 = reduction_mean ? 2.f / (float)n : 2.f;
  const int64_t blocks = (n + kLossThreads - 1) / kLossThreads;
  hipLaunchKernelGGL(k_mse_bwd, dim3((unsigned)blocks), dim3(kLossThreads), 0,
                     static_cast<hipStream_t>(stream), input, target, grad_loss, n, scale2,
                     grad_input, grad_target);
  HIP_RET(hipGetLastError());
  return 0;
}
