// Fused Adam / AMSGrad step (torch.optim.Adam as train.py:117-119 builds it) -- see cgr_adam_step
// in include/cgr_mpnn3d.h.  Memory-bound streaming: 5 reads + 4 writes of fp32 per element
// (amsgrad), float4 when every pointer of a tensor is 16-byte aligned, scalar otherwise.
// cgr_adam_step_clip adds global gradient-norm clipping (clip_grad_norm_ + step): one more
// streaming read of the gradients (k_grad_sumsq), the norm finalised by the step-count kernel.
#include <math.h>

#include "common.hpp"
#include "gnn_internal.hpp"
#include "streams.hpp"

namespace cgr {

struct AdamGroup {
  float* p[CGR_ADAM_GROUP];
  const float* g[CGR_ADAM_GROUP];
  float* m[CGR_ADAM_GROUP];
  float* v[CGR_ADAM_GROUP];
  float* vmax[CGR_ADAM_GROUP];
  float* step[CGR_ADAM_GROUP];
  int64_t numel[CGR_ADAM_GROUP];
  int32_t vec4[CGR_ADAM_GROUP];
  int32_t first_block[CGR_ADAM_GROUP + 1];
  int32_t n;
  // the timeout gate (streams.hpp adam_gate): `err` = the host-mapped error words, `gate` = the
  // device word the step-count kernel sets from them; both null = ungated
  const int* err;
  int* gate;
};

struct AdamHyper {
  double lr, b1, b2;
  float w1, b2f, w2, eps, wd;  // (float)(1 - b1), (float)b2, (float)(1 - b2), ... as torch casts
  int amsgrad, maximize;
  // lr as a device scalar (cgr_adam_step_lr_ptr: a scheduler updates it between replays of a
  // captured step); null = the host value `lr` above
  const float* lr_dev;
  // clipping (cgr_adam_step_clip, k_adam<true> only): the step's global gradient norm on the
  // device and this table's bound; max_norm <= 0 = not scaled
  const float* norm_dev;
  float max_norm;
};

constexpr int kAdamThreads = 256;
// one float4 per thread: 1.49 M parameters at cfg2 make ~1,460 blocks, every element's five loads
// in flight at once (r04's 16 elements per thread gave 91 blocks on 256 CUs: 15.4 us in the
// replayed step for 54 MB)
constexpr int kAdamElemsPerBlock = kAdamThreads * 4;

// t <- t + 1 for every tensor of the group (before k_adam reads it, same stream) -- unless an
// unpaired backward's completion timed out (its gradients are NaN): then the gate word tells
// k_adam to skip the step, and the parameters stay finite until the model's next forward raises
__global__ void k_adam_step_count(AdamGroup G) {
  __shared__ int poisoned;
  if (threadIdx.x == 0) {
    poisoned = G.err ? __hip_atomic_load(G.err + kDevErrUnpairedTimeout, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_SYSTEM) != 0
                     : 0;
    if (G.gate) G.gate[0] = poisoned;
  }
  __syncthreads();
  const int i = threadIdx.x;
  if (i < G.n && !poisoned) G.step[i][0] = G.step[i][0] + 1.f;
}

// The clipped step's norm (cgr_adam_step_clip).  Every block of k_grad_sumsq leaves one fp32 sum of
// squares, in the block decomposition of k_adam; k_adam_step_count_clip adds them up.  Nothing
// here is an atomic, and every order is fixed: identical gradient bits give identical norm bits.
struct NormGroup {
  const float* g[CGR_ADAM_GROUP];
  int64_t numel[CGR_ADAM_GROUP];
  int32_t vec4[CGR_ADAM_GROUP];
  int32_t first_block[CGR_ADAM_GROUP + 1];
  int32_t n;
  float* partials;  // [first_block[n]]: this launch's slice
};

struct ClipState {
  const float* partials;  // null: the norm and the gate of this step are already final
  int64_t num_partials;
  float* grad_norm;
  int* gate;
  int64_t* skipped;
};

constexpr int kNormFinalThreads = 256;

// streaming like k_adam (one float4 per thread, ~1,460 blocks at cfg2), 4 bytes read per element
__global__ __launch_bounds__(kAdamThreads) void k_grad_sumsq(NormGroup G) {
  const int b = blockIdx.x;
  int t = 0;
  while (t + 1 < G.n && G.first_block[t + 1] <= b) ++t;
  const int64_t n = G.numel[t];
  const float* Gr = G.g[t];
  const int64_t e = (int64_t)(b - G.first_block[t]) * kAdamElemsPerBlock + 4 * (int64_t)threadIdx.x;
  float s = 0.f;
  if (G.vec4[t] && e + 4 <= n) {
    const float4 g4 = *reinterpret_cast<const float4*>(Gr + e);
    s = (g4.x * g4.x + g4.y * g4.y) + (g4.z * g4.z + g4.w * g4.w);
  } else {
    for (int64_t k = e; k < n && k < e + 4; ++k) s = fmaf(Gr[k], Gr[k], s);
  }
  __shared__ float red[kAdamThreads / 64];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) G.partials[b] = (red[0] + red[1]) + (red[2] + red[3]);
}

// k_adam_step_count for a clipped step.  The launch that carries the partials first finalises the
// norm: thread i sums partials i, i + 256, ... in double, an LDS tree adds the 256 sums, and
// thread 0 writes the norm, the gate (a non-finite sum or the unpaired timeout: skip the step) and
// the skip count.  The later launches of the same step (further groups of CGR_ADAM_GROUP tensors,
// further param groups) only read the gate.
__global__ __launch_bounds__(kNormFinalThreads) void k_adam_step_count_clip(AdamGroup G,
                                                                            ClipState C) {
  __shared__ double red[kNormFinalThreads];
  __shared__ int skip;
  const int i = threadIdx.x;
  if (C.partials) {
    double s = 0.0;
    for (int64_t k = i; k < C.num_partials; k += kNormFinalThreads) s += (double)C.partials[k];
    red[i] = s;
    __syncthreads();
    for (int o = kNormFinalThreads / 2; o > 0; o >>= 1) {
      if (i < o) red[i] += red[i + o];
      __syncthreads();
    }
    if (i == 0) {
      const double total = red[0];
      const int bad = !(total <= 1.7976931348623157e308);  // inf or NaN
      const int poisoned = G.err ? __hip_atomic_load(G.err + kDevErrUnpairedTimeout,
                                                     __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_SYSTEM) != 0
                                 : 0;
      C.grad_norm[0] = (float)sqrt(total);
      if (bad) C.skipped[0] = C.skipped[0] + 1;
      skip = bad | poisoned;
      C.gate[0] = skip;
    }
  } else if (i == 0) {
    skip = C.gate[0];
  }
  __syncthreads();
  if (i < G.n && !skip) G.step[i][0] = G.step[i][0] + 1.f;
}

// torch _multi_tensor_adam order: lerp_ (weight < 0.5: m + w (g - m)), mul_(b2), addcmul_,
// maximum_, sqrt, div_(bc2_sqrt), add_(eps), addcdiv_(m, denom, -step_size).  kClip: the gradient
// is first scaled by the clip coefficient, rounded on its own as clip_grad_norm_'s g.mul_(coef) is
template <bool kClip>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float& vm,
                                          const AdamHyper& h, float neg_step_size,
                                          float bc2_sqrt, float coef) {
  if (kClip) g = __fmul_rn(g, coef);
  if (h.maximize) g = -g;
  if (h.wd != 0.f) g = fmaf(p, h.wd, g);          // grad.add(param, alpha=wd)
  m = fmaf(h.w1, g - m, m);
  v = fmaf(h.w2 * g, g, v * h.b2f);
  float vv = v;
  if (h.amsgrad) {
    vm = fmaxf(vm, v);
    vv = vm;
  }
  const float denom = sqrtf(vv) / bc2_sqrt + h.eps;
  p = fmaf(neg_step_size, m / denom, p);
}

template <bool kClip>
__global__ __launch_bounds__(kAdamThreads) void k_adam(AdamGroup G, AdamHyper h) {
  // the gradients are NaN-poisoned, or (kClip) their norm is not finite: no update (above)
  if (G.gate && G.gate[0]) return;
  const int b = blockIdx.x;
  int t = 0;
  while (t + 1 < G.n && G.first_block[t + 1] <= b) ++t;
  // the bias corrections once per block (double pow), broadcast through LDS
  __shared__ float sc[3];
  if (threadIdx.x == 0) {
    const double step = (double)G.step[t][0];
    const double bc1 = 1.0 - pow(h.b1, step);
    const double bc2 = 1.0 - pow(h.b2, step);
    const double lr = h.lr_dev ? (double)h.lr_dev[0] : h.lr;
    sc[0] = (float)(-(lr / bc1));
    sc[1] = (float)sqrt(bc2);
    // clip_grad_norm_: coef = clamp(max_norm / (total_norm + 1e-6), max=1), in fp32
    if (kClip) sc[2] = h.max_norm > 0.f ? fminf(h.max_norm / (h.norm_dev[0] + 1e-6f), 1.f) : 1.f;
  }
  __syncthreads();
  const float neg_step_size = sc[0], bc2_sqrt = sc[1];
  const float coef = kClip ? sc[2] : 1.f;
  const int64_t base = (int64_t)(b - G.first_block[t]) * kAdamElemsPerBlock;
  const int64_t n = G.numel[t];
  float* P = G.p[t];
  const float* Gr = G.g[t];
  float* M = G.m[t];
  float* V = G.v[t];
  float* VM = G.vmax[t];
  const int64_t e = base + 4 * (int64_t)threadIdx.x;
  if (G.vec4[t] && e + 4 <= n) {
    float4 p4 = *reinterpret_cast<const float4*>(P + e);
    const float4 g4 = *reinterpret_cast<const float4*>(Gr + e);
    float4 m4 = *reinterpret_cast<const float4*>(M + e);
    float4 v4 = *reinterpret_cast<const float4*>(V + e);
    float4 x4 = h.amsgrad ? *reinterpret_cast<const float4*>(VM + e) : v4;
    adam_elem<kClip>(p4.x, g4.x, m4.x, v4.x, x4.x, h, neg_step_size, bc2_sqrt, coef);
    adam_elem<kClip>(p4.y, g4.y, m4.y, v4.y, x4.y, h, neg_step_size, bc2_sqrt, coef);
    adam_elem<kClip>(p4.z, g4.z, m4.z, v4.z, x4.z, h, neg_step_size, bc2_sqrt, coef);
    adam_elem<kClip>(p4.w, g4.w, m4.w, v4.w, x4.w, h, neg_step_size, bc2_sqrt, coef);
    *reinterpret_cast<float4*>(P + e) = p4;
    *reinterpret_cast<float4*>(M + e) = m4;
    *reinterpret_cast<float4*>(V + e) = v4;
    if (h.amsgrad) *reinterpret_cast<float4*>(VM + e) = x4;
  } else {
    for (int64_t k = e; k < n && k < e + 4; ++k) {
      float vm = h.amsgrad ? VM[k] : 0.f;
      adam_elem<kClip>(P[k], Gr[k], M[k], V[k], vm, h, neg_step_size, bc2_sqrt, coef);
      if (h.amsgrad) VM[k] = vm;
    }
  }
}

}  // namespace cgr

using namespace cgr;

static int adam_step(const cgr_adam_tensor* tensors, int32_t num_tensors, double lr,
                     const float* lr_dev, double beta1, double beta2, double eps,
                     double weight_decay, int32_t amsgrad, int32_t maximize,
                     const cgr_adam_clip* clip, void* stream) {
  CGR_CHECK(num_tensors >= 0 && (num_tensors == 0 || tensors != nullptr),
            "cgr_adam_step: bad tensor table");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const AdamHyper h{lr,
                    beta1,
                    beta2,
                    (float)(1.0 - beta1),
                    (float)beta2,
                    (float)(1.0 - beta2),
                    (float)eps,
                    (float)weight_decay,
                    amsgrad ? 1 : 0,
                    maximize ? 1 : 0,
                    lr_dev,
                    clip ? clip->grad_norm : nullptr,
                    clip && clip->max_norm > 0.0 ? (float)clip->max_norm : 0.f};
  int dev = -1;
  SideStreams* ss = hipStreamGetDevice(st, &dev) == hipSuccess ? side_streams_of(dev) : nullptr;
  (void)hipGetLastError();
  // a clipped step gates on the caller's word (the norm's finite flag and the timeout together)
  const int* err = clip ? (ss ? ss->dev_err : nullptr) : ss && ss->adam_gate ? ss->dev_err : nullptr;
  int* gate = clip ? clip->gate : ss ? ss->adam_gate : nullptr;
  ClipState C{};
  if (clip) {
    C.partials = clip->num_partials > 0 ? clip->partials : nullptr;
    C.num_partials = clip->num_partials;
    C.grad_norm = clip->grad_norm;
    C.gate = clip->gate;
    C.skipped = clip->skipped_steps;
  }
  AdamGroup G{};
  G.err = err;
  G.gate = gate;
  auto flush = [&]() -> int {
    // (the launch that finalises the norm goes out even for a table without a single gradient)
    if (G.n == 0 && !C.partials) return 0;
    const int blocks = G.first_block[G.n];
    if (clip) {
      hipLaunchKernelGGL(k_adam_step_count_clip, dim3(1), dim3(kNormFinalThreads), 0, st, G, C);
      C.partials = nullptr;
    } else {
      hipLaunchKernelGGL(k_adam_step_count, dim3(1), dim3(64), 0, st, G);
    }
    HIP_RET(hipGetLastError());
    if (blocks > 0) {
      if (clip)
        hipLaunchKernelGGL(k_adam<true>, dim3(blocks), dim3(kAdamThreads), 0, st, G, h);
      else
        hipLaunchKernelGGL(k_adam<false>, dim3(blocks), dim3(kAdamThreads), 0, st, G, h);
      HIP_RET(hipGetLastError());
    }
    G = AdamGroup{};
    G.err = err;
    G.gate = gate;
    return 0;
  };
  for (int i = 0; i < num_tensors; ++i) {
    const cgr_adam_tensor& t = tensors[i];
    if (t.grad == nullptr || t.numel <= 0) continue;
    CGR_CHECK(t.param && t.exp_avg && t.exp_avg_sq && t.step && (!amsgrad || t.max_exp_avg_sq),
              "cgr_adam_step: NULL state pointer");
    const int64_t nb = (t.numel + kAdamElemsPerBlock - 1) / kAdamElemsPerBlock;
    CGR_CHECK(nb < (1 << 30), "cgr_adam_step: tensor too large");
    const int k = G.n;
    G.p[k] = t.param;
    G.g[k] = t.grad;
    G.m[k] = t.exp_avg;
    G.v[k] = t.exp_avg_sq;
    G.vmax[k] = t.max_exp_avg_sq;
    G.step[k] = t.step;
    G.numel[k] = t.numel;
    auto al = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    G.vec4[k] = al(t.param) && al(t.grad) && al(t.exp_avg) && al(t.exp_avg_sq) &&
                (!amsgrad || al(t.max_exp_avg_sq));
    G.first_block[k + 1] = G.first_block[k] + (int32_t)nb;
    CGR_CHECK((int64_t)G.first_block[k] + nb < (1LL << 31), "cgr_adam_step: too many blocks");
    G.n = k + 1;
    if (G.n == CGR_ADAM_GROUP) {
      const int rc = flush();
      if (rc) return rc;
    }
  }
  return flush();
}

extern "C" int cgr_adam_step(const cgr_adam_tensor* tensors, int32_t num_tensors, double lr,
                             double beta1, double beta2, double eps, double weight_decay,
                             int32_t amsgrad, int32_t maximize, void* stream) {
  clear_stale_hip_error();
  return adam_step(tensors, num_tensors, lr, nullptr, beta1, beta2, eps, weight_decay, amsgrad,
                   maximize, nullptr, stream);
}

extern "C" int cgr_adam_step_lr_ptr(const cgr_adam_tensor* tensors, int32_t num_tensors,
                                    const float* lr, double beta1, double beta2, double eps,
                                    double weight_decay, int32_t amsgrad, int32_t maximize,
                                    void* stream) {
  clear_stale_hip_error();
  CGR_CHECK(lr != nullptr, "cgr_adam_step_lr_ptr: NULL lr");
  return adam_step(tensors, num_tensors, 0.0, lr, beta1, beta2, eps, weight_decay, amsgrad,
                   maximize, nullptr, stream);
}

extern "C" int cgr_adam_step_clip(const cgr_adam_tensor* tensors, int32_t num_tensors, double lr,
                                  const float* lr_dev, double beta1, double beta2, double eps,
                                  double weight_decay, int32_t amsgrad, int32_t maximize,
                                  const cgr_adam_clip* clip, void* stream) {
  clear_stale_hip_error();
  CGR_CHECK(clip && clip->grad_norm && clip->gate && clip->skipped_steps && clip->num_partials >= 0 &&
                (clip->num_partials == 0 || clip->partials),
            "cgr_adam_step_clip: bad clip state");
  CGR_CHECK(!(clip->max_norm != clip->max_norm), "cgr_adam_step_clip: max_norm is NaN");
  return adam_step(tensors, num_tensors, lr, lr_dev, beta1, beta2, eps, weight_decay, amsgrad,
                   maximize, clip, stream);
}

// the partial count of one table entry: k_adam's block decomposition
static int64_t sumsq_blocks(const cgr_adam_tensor& t) {
  if (t.grad == nullptr || t.numel <= 0) return 0;
  return (t.numel + kAdamElemsPerBlock - 1) / kAdamElemsPerBlock;
}

extern "C" int64_t cgr_grad_sumsq_partials(const cgr_adam_tensor* tensors, int32_t num_tensors) {
  if (num_tensors < 0 || (num_tensors > 0 && tensors == nullptr)) {
    set_error("cgr_grad_sumsq_partials: bad tensor table");
    return -1;
  }
  int64_t total = 0;
  for (int i = 0; i < num_tensors; ++i) total += sumsq_blocks(tensors[i]);
  return total;
}

extern "C" int cgr_grad_sumsq(const cgr_adam_tensor* tensors, int32_t num_tensors,
                              float* partials, int64_t capacity, void* stream) {
  clear_stale_hip_error();
  const int64_t total = cgr_grad_sumsq_partials(tensors, num_tensors);
  CGR_CHECK(total >= 0, "cgr_grad_sumsq: bad tensor table");
  CGR_CHECK(total <= capacity && (total == 0 || partials),
            "cgr_grad_sumsq: the partials buffer is too small for this table");
  CGR_CHECK(total < (1LL << 31), "cgr_grad_sumsq: too many blocks");
  hipStream_t st = static_cast<hipStream_t>(stream);
  NormGroup G{};
  G.partials = partials;
  auto flush = [&]() -> int {
    if (G.n == 0) return 0;
    const int blocks = G.first_block[G.n];
    hipLaunchKernelGGL(k_grad_sumsq, dim3(blocks), dim3(kAdamThreads), 0, st, G);
    HIP_RET(hipGetLastError());
    float* next = G.partials + blocks;
    G = NormGroup{};
    G.partials = next;
    return 0;
  };
  for (int i = 0; i < num_tensors; ++i) {
    const int64_t nb = sumsq_blocks(tensors[i]);
    if (nb == 0) continue;
    const int k = G.n;
    G.g[k] = tensors[i].grad;
    G.numel[k] = tensors[i].numel;
    G.vec4[k] = ((uintptr_t)tensors[i].grad & 15) == 0;
    G.first_block[k + 1] = G.first_block[k] + (int32_t)nb;
    G.n = k + 1;
    if (G.n == CGR_ADAM_GROUP) {
      const int rc = flush();
      if (rc) return rc;
    }
  }
  return flush();
}
