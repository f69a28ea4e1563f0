// Attention pooling over atom embeddings (cgr_attention_pool_forward / _backward): a gated softmax
// over each graph's atoms,
//   s_v = x[v].w + b ; alpha_v = softmax_{graph(v), unmasked}(s)_v ; g[b] = sum_v alpha_v x[v].
// One workgroup per graph, as k_pool_head (kernels.hip): a graph's atoms are summed in atom order
// by one thread per float4 column group (16 atoms at a time as a fixed tree, the batches' sums
// in order with a compensated running sum), every cross-thread reduction has a fixed shape, and a
// workgroup reads nothing but its own graph's rows -- so a graph's g row, alpha and dx rows are
// the same bits pooled alone or inside any batch, and every result is reproducible.
//
// Rows of x (stride ldx), g, dg and dx (stride H) are only 4-byte aligned when the stride is not a
// multiple of 4 (GNN.encode_nodes hands rows of stride H).  VEC: every base 16-byte aligned and
// H, ldx multiples of 4 -> float4 accesses; else element by element.  Both forms give lane l of a
// wave the columns 4l .. 4l + 3 (+ 256 j), so a dot product is the same bits in either.
#include "common.hpp"
#include "gnn_internal.hpp"
#include "kernels.hpp"

namespace cgr {

constexpr int kAttnThreads = 256;
constexpr int kAttnWaves = kAttnThreads / 64;
constexpr int kAttnBatch = 16;  // atoms whose loads are in flight together (kPoolBatch)
constexpr int kAttnCap = 1024;  // ds_v of a chunk of atoms in LDS (backward)

// first index in the sorted ids [0, n) whose id is >= key
__device__ __forceinline__ int64_t lower_bound_id(const int64_t* __restrict__ ids, int64_t n,
                                                  int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ids[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// graph b's atoms [v0, v1): from ptr, else two searches in the sorted batch, else all N; clamped
// into [0, N] whatever the arrays hold
__device__ __forceinline__ void attn_segment(const int64_t* __restrict__ batch,
                                             const int64_t* __restrict__ ptr, int64_t N, int64_t b,
                                             int64_t& v0, int64_t& v1) {
  if (ptr) {
    v0 = ptr[b];
    v1 = ptr[b + 1];
  } else if (batch) {
    v0 = lower_bound_id(batch, N, b);
    v1 = lower_bound_id(batch, N, b + 1);
  } else {
    v0 = 0;
    v1 = N;
  }
  v0 = v0 < 0 ? 0 : (v0 > N ? N : v0);
  v1 = v1 < v0 ? v0 : (v1 > N ? N : v1);
}

template <bool VEC>
__device__ __forceinline__ float4 attn_ld4(const float* __restrict__ p, int valid) {
  return load4<VEC ? 4 : 1>(p, valid);
}

// columns [k, k + 4) of a row of stride-H storage (g, dx): never past column H
template <bool VEC>
__device__ __forceinline__ void attn_st4(float* __restrict__ row, int k, int H, const float4& v) {
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(row + k) = v;
  } else {
    const float tv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (k + q < H) row[k + q] = tv[q];
  }
}

// row . u over H columns by one wave (every lane returns the sum); explicit fmaf: the backward
// evaluates t_v at two sites and both must give the same bits
template <bool VEC>
__device__ __forceinline__ float attn_row_dot(const float* __restrict__ row,
                                              const float* __restrict__ u, int H, int lane) {
  float acc = 0.f;
  for (int k = 4 * lane; k < H; k += 256) {
    const float4 a = attn_ld4<VEC>(row + k, H - k), c = attn_ld4<VEC>(u + k, H - k);
    acc = fmaf(a.x, c.x, acc);
    acc = fmaf(a.y, c.y, acc);
    acc = fmaf(a.z, c.z, acc);
    acc = fmaf(a.w, c.w, acc);
  }
  return wave_sum(acc);
}

// sum_u wgt[u] x[u] over one batch of atoms as a fixed tree over its kAttnBatch slots (atoms u,
// u + 1 paired first); slots with gate[u] == 0 (weight-0 atoms, slots past the segment) add +0
__device__ __forceinline__ float4 attn_batch_sum(const float (&gate)[kAttnBatch],
                                                 const float (&wgt)[kAttnBatch],
                                                 const float4 (&x)[kAttnBatch]) {
  float4 p[kAttnBatch / 2];
#pragma unroll
  for (int j = 0; j < kAttnBatch / 2; ++j) {
    p[j] = gate[2 * j] != 0.f ? f4scale(x[2 * j], wgt[2 * j]) : f4zero();
    if (gate[2 * j + 1] != 0.f) {
      p[j].x = fmaf(wgt[2 * j + 1], x[2 * j + 1].x, p[j].x);
      p[j].y = fmaf(wgt[2 * j + 1], x[2 * j + 1].y, p[j].y);
      p[j].z = fmaf(wgt[2 * j + 1], x[2 * j + 1].z, p[j].z);
      p[j].w = fmaf(wgt[2 * j + 1], x[2 * j + 1].w, p[j].w);
    }
  }
#pragma unroll
  for (int n = kAttnBatch / 4; n >= 1; n >>= 1)
#pragma unroll
    for (int j = 0; j < n; ++j) p[j] = f4add(p[j], p[j + n]);
  return p[0];
}

// running sum of the batches' sums, compensated (Kahan): a segment of 1,500 atoms keeps the
// error of a short one.  Plain adds and subtracts only; the build has no reassociating fast-math.
struct AttnAcc {
  float4 s = f4zero(), c = f4zero();
  __device__ __forceinline__ void add(const float4& v) {
    const float4 y = f4sub(v, c);
    const float4 t = f4add(s, y);
    c = f4sub(f4sub(t, s), y);
    s = t;
  }
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// workgroup reductions through red[kAttnWaves]; the closing barrier frees red for the next one
__device__ __forceinline__ float attn_block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ float attn_block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return r;
}
static_assert(kAttnWaves == 4, "attn_block_sum / _max combine four waves");

// Forward.  alpha [N] doubles as the kernel's own scratch -- scores, then exponentials, then the
// weights -- for segments of any length; it is written and read back here, so it is neither const
// nor __restrict__ (such loads could go through the scalar cache, which does not see the vector
// stores).  A graph without unmasked atoms: alpha 0, g row +0.0, no division.
template <bool VEC>
__global__ __launch_bounds__(kAttnThreads) void k_attn_pool_fwd(
    const float* __restrict__ x, int64_t ldx, const int64_t* __restrict__ batch,
    const int64_t* __restrict__ ptr, int64_t N, int H, const float* __restrict__ w,
    const float* __restrict__ bias, const uint8_t* __restrict__ mask, float* alpha,
    float* __restrict__ g) {
  __shared__ float red[kAttnWaves];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int64_t v0, v1;
  attn_segment(batch, ptr, N, b, v0, v1);
  const float b0 = bias ? bias[0] : 0.f;

  // scores: each wave takes whole atoms, its lanes cover the columns
  for (int64_t v = v0 + wv; v < v1; v += kAttnWaves) {
    if (mask && !mask[v]) continue;
    const float s = attn_row_dot<VEC>(x + v * ldx, w, H, lane) + b0;
    if (lane == 0) alpha[v] = s;
  }
  __syncthreads();

  float m = -INFINITY;
  for (int64_t v = v0 + threadIdx.x; v < v1; v += kAttnThreads)
    if (!mask || mask[v]) m = fmaxf(m, alpha[v]);
  m = attn_block_max(m, red);

  // a thread reads back only what it wrote itself until the next barrier
  float sum = 0.f;
  for (int64_t v = v0 + threadIdx.x; v < v1; v += kAttnThreads) {
    const float e = (!mask || mask[v]) ? expf(alpha[v] - m) : 0.f;
    alpha[v] = e;
    sum += e;
  }
  const float S = attn_block_sum(sum, red);
  for (int64_t v = v0 + threadIdx.x; v < v1; v += kAttnThreads)
    alpha[v] = S == 0.f ? 0.f : alpha[v] / S;
  __syncthreads();

  // g[b] = sum_v alpha_v x[v]: one thread per float4 column group, atoms in order (the second
  // read of the segment's rows comes from L2); atoms of weight 0 take no part
  const int C4 = (H + 3) >> 2;
  for (int c = threadIdx.x; c < C4; c += kAttnThreads) {
    const int k = 4 * c;
    AttnAcc s;
    for (int64_t v = v0; v < v1; v += kAttnBatch) {
      float4 xr[kAttnBatch];
      float a[kAttnBatch];
#pragma unroll
      for (int u = 0; u < kAttnBatch; ++u) {
        const bool in = v + u < v1;
        a[u] = in ? alpha[v + u] : 0.f;
        xr[u] = in ? attn_ld4<VEC>(x + (v + u) * ldx + k, H - k) : f4zero();
      }
      s.add(attn_batch_sum(a, a, xr));
    }
    attn_st4<VEC>(g + b * H, k, H, s.s);
  }
}

// Backward of one graph from dg[b]:
//   t_v = dg[b].x[v] ; c = sum_v alpha_v t_v ; ds_v = alpha_v (t_v - c)
//   dx[v] = alpha_v dg[b] + ds_v w ; dwp[b] = sum_v ds_v x[v]   (this graph's share of dw)
// c first (one wave per atom, each wave's atoms in order, the four waves combined in a fixed
// order), then the atoms in chunks of kAttnCap: ds_v of the chunk into LDS (t_v evaluated again,
// the rows come from L2), then one thread per float4 column group writes the chunk's dx rows and
// accumulates dwp in atom order.  dwp rows have stride Hp = round_up(H, 4) (16-byte rows; the
// thread that owns a column group carries it across chunks through the row itself), an empty
// graph's row is zeros.  Atoms of weight 0 (masked) get dx rows of exact zeros.  dx, dwp nullable.
template <bool VEC>
__global__ __launch_bounds__(kAttnThreads) void k_attn_pool_bwd(
    const float* __restrict__ x, int64_t ldx, const int64_t* __restrict__ batch,
    const int64_t* __restrict__ ptr, int64_t N, int H, const float* __restrict__ w,
    const float* __restrict__ alpha, const float* __restrict__ dg, float* __restrict__ dx,
    float* dwp, int Hp) {
  __shared__ float red[kAttnWaves];
  __shared__ float ds_s[kAttnCap];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int64_t v0, v1;
  attn_segment(batch, ptr, N, b, v0, v1);
  const float* dgb = dg + b * H;
  const int C4 = (H + 3) >> 2;
  float* dwb = dwp ? dwp + b * Hp : nullptr;
  if (v1 <= v0) {  // (uniform over the workgroup)
    if (dwb)
      for (int c = threadIdx.x; c < C4; c += kAttnThreads)
        *reinterpret_cast<float4*>(dwb + 4 * c) = f4zero();
    return;
  }

  float cw = 0.f;
  for (int64_t v = v0 + wv; v < v1; v += kAttnWaves) {
    const float a = alpha[v];
    if (a == 0.f) continue;
    cw = fmaf(a, attn_row_dot<VEC>(x + v * ldx, dgb, H, lane), cw);
  }
  if (lane == 0) red[wv] = cw;
  __syncthreads();
  const float cb = (red[0] + red[1]) + (red[2] + red[3]);

  for (int64_t c0 = v0; c0 < v1; c0 += kAttnCap) {
    const int nc = (int)(v1 - c0 < kAttnCap ? v1 - c0 : kAttnCap);
    for (int i = wv; i < nc; i += kAttnWaves) {
      const int64_t v = c0 + i;
      const float a = alpha[v];
      const float t = a == 0.f ? 0.f : attn_row_dot<VEC>(x + v * ldx, dgb, H, lane);
      if (lane == 0) ds_s[i] = a == 0.f ? 0.f : a * (t - cb);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C4; c += kAttnThreads) {
      const int k = 4 * c;
      const float4 wk = attn_ld4<VEC>(w + k, H - k), dgk = attn_ld4<VEC>(dgb + k, H - k);
      AttnAcc acc;  // (the compensation starts over at a chunk boundary)
      if (dwb && c0 > v0) acc.s = *reinterpret_cast<const float4*>(dwb + k);
      for (int i = 0; i < nc; i += kAttnBatch) {
        float4 xr[kAttnBatch];
        float a[kAttnBatch], d[kAttnBatch];
#pragma unroll
        for (int u = 0; u < kAttnBatch; ++u) {
          const bool in = i + u < nc;
          a[u] = in ? alpha[c0 + i + u] : 0.f;
          d[u] = in ? ds_s[i + u] : 0.f;
          xr[u] = in && dwb ? attn_ld4<VEC>(x + (c0 + i + u) * ldx + k, H - k) : f4zero();
        }
#pragma unroll
        for (int u = 0; u < kAttnBatch; ++u) {
          float4 r = f4zero();
          if (a[u] != 0.f) {
            r.x = fmaf(d[u], wk.x, a[u] * dgk.x);
            r.y = fmaf(d[u], wk.y, a[u] * dgk.y);
            r.z = fmaf(d[u], wk.z, a[u] * dgk.z);
            r.w = fmaf(d[u], wk.w, a[u] * dgk.w);
          }
          if (dx && i + u < nc) attn_st4<VEC>(dx + (c0 + i + u) * H, k, H, r);
        }
        if (dwb) acc.add(attn_batch_sum(a, d, xr));
      }
      if (dwb) *reinterpret_cast<float4*>(dwb + k) = acc.s;
    }
    __syncthreads();  // ds_s is rewritten by the next chunk
  }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

hipError_t attn_pool_fwd(const float* x, int64_t ldx, int64_t N, int H, const int64_t* batch,
                         const int64_t* ptr, int64_t B, const float* w, const float* bias,
                         const uint8_t* mask, float* g, float* alpha, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  const bool vec = H % 4 == 0 && ldx % 4 == 0 && aligned16(x) && aligned16(w) && aligned16(g);
  if (vec)
    hipLaunchKernelGGL(k_attn_pool_fwd<true>, dim3((unsigned)B), dim3(kAttnThreads), 0, st, x,
                       ldx, batch, ptr, N, H, w, bias, mask, alpha, g);
  else
    hipLaunchKernelGGL(k_attn_pool_fwd<false>, dim3((unsigned)B), dim3(kAttnThreads), 0, st, x,
                       ldx, batch, ptr, N, H, w, bias, mask, alpha, g);
  return hipGetLastError();
}

hipError_t attn_pool_bwd(const float* x, int64_t ldx, int64_t N, int H, const int64_t* batch,
                         const int64_t* ptr, int64_t B, const float* w, const float* alpha,
                         const float* dg, float* dx, float* dw, float* dwp, hipStream_t st) {
  if (B <= 0 || (!dx && !dw)) return hipSuccess;
  const int Hp = (int)round_up(H, 4);
  const bool vec = H % 4 == 0 && ldx % 4 == 0 && aligned16(x) && aligned16(w) && aligned16(dg) &&
                   (!dx || aligned16(dx));
  if (!dw) dwp = nullptr;
  if (vec)
    hipLaunchKernelGGL(k_attn_pool_bwd<true>, dim3((unsigned)B), dim3(kAttnThreads), 0, st, x,
                       ldx, batch, ptr, N, H, w, alpha, dg, dx, dwp, Hp);
  else
    hipLaunchKernelGGL(k_attn_pool_bwd<false>, dim3((unsigned)B), dim3(kAttnThreads), 0, st, x,
                       ldx, batch, ptr, N, H, w, alpha, dg, dx, dwp, Hp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !dw) return e;
  // dw[h] = sum_b dwp[b, h], b = 0 .. B-1 in the slab reduction's fixed order
  return reduce_slabs(dwp, nullptr, (int)B, 1, H, dw, H, 0, nullptr, st);
}

}  // namespace cgr
