// The two kernels of the headless path (cgr_gnn_encode*, gnn_fwd.hip / gnn_bwd.hip): the pool
// without the ffn head and dzn from a general cotangent dg [B, H].  Each is the second-kernel form
// of one in kernels.hip / b3_pack.hip (k_pool_head, k_readout_bwd_img) and keeps that kernel's
// arithmetic and order to the letter -- tests/test_gpu_encode.py holds them to bitwise equality
// with the fused path.  They live in a translation unit of their own, linked last, so that the
// code objects of the fused path's kernels are byte for byte what they were without this file.
#include "bwd_rows.hpp"
#include "common.hpp"
#include "gemm_b3.hpp"
#include "gemm_b3tn.hpp"
#include "kernels.hpp"

namespace cgr {

// ------------------------------------------------------------------------------------------
// pool without head: one workgroup per graph, one thread per float4 column (k_pool_head's layout,
// summation order over a graph's nodes, max / first-arg / tie-count record and inv_cnt scaling)
// ------------------------------------------------------------------------------------------
constexpr int kPoolThreads = 128;
constexpr int kPoolBatch = 16;

// g [B, Hp] as k_pool_head writes it, and the caller's g_out [B, H] with row stride H: its rows
// are not 16-byte aligned when H % 4 != 0 and a row's last column group must not reach into the
// next row, so g_out is stored element by element
__global__ __launch_bounds__(kPoolThreads) void k_pool_only(const float* __restrict__ hn, int Hp,
                                                            const int* __restrict__ gptr, int H,
                                                            float* __restrict__ g,
                                                            float* __restrict__ g_out,
                                                            const float* __restrict__ inv_cnt,
                                                            int* __restrict__ pool_arg,
                                                            bool pool_first) {
  const int b = blockIdx.x;
  const int v0 = gptr[b], v1 = gptr[b + 1];
  const int C4 = Hp >> 2;
  const float gs = inv_cnt ? inv_cnt[b] : 1.f;  // global_mean_pool: the sum / node count
  for (int c = threadIdx.x; c < C4; c += kPoolThreads) {
    const float* col = hn + 4 * c;
    float4 s = f4zero();
    if (pool_arg) {  // global_max_pool: the largest value, its first node and its tie count
      float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      int arg[4] = {-1, -1, -1, -1}, cnt[4] = {0, 0, 0, 0};
      for (int v = v0; v < v1; ++v) {
        const float4 x = *reinterpret_cast<const float4*>(col + (int64_t)v * Hp);
        const float xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (xv[k] > m[k] || arg[k] < 0) {
            m[k] = xv[k];
            arg[k] = v;
            cnt[k] = 1;
          } else if (xv[k] == m[k]) {
            ++cnt[k];
          }
      }
      if (v1 <= v0) m[0] = m[1] = m[2] = m[3] = 0.f;  // (empty graph: 0, entry -1, never read)
      s = make_float4(m[0], m[1], m[2], m[3]);
      int rec[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)  // torch's amax backward also counts the zero `self` at a 0 max
        rec[k] = pool_first || arg[k] < 0 ? arg[k] : -(cnt[k] + (m[k] == 0.f ? 1 : 0));
      *reinterpret_cast<int4*>(pool_arg + (int64_t)b * Hp + 4 * c) =
          make_int4(rec[0], rec[1], rec[2], rec[3]);
    } else {
      for (int v = v0; v < v1; v += kPoolBatch) {
        float4 x[kPoolBatch];
#pragma unroll
        for (int u = 0; u < kPoolBatch; ++u)
          x[u] = v + u < v1 ? *reinterpret_cast<const float4*>(col + (int64_t)(v + u) * Hp)
                            : f4zero();
#pragma unroll
        for (int u = 0; u < kPoolBatch; ++u)
          if (v + u < v1) s = f4add(s, x[u]);
      }
    }
    if (inv_cnt) s = make_float4(s.x * gs, s.y * gs, s.z * gs, s.w * gs);
    *reinterpret_cast<float4*>(g + (int64_t)b * Hp + 4 * c) = s;
    const int n = 4 * c;
    const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (n + k < H) g_out[(int64_t)b * H + n + k] = sv[k];
  }
}

hipError_t pool_only_fwd(const float* hn, int Hp, const int* gptr, int64_t B, int H, float* g,
                         float* g_out, hipStream_t st, const float* inv_cnt, int* pool_arg,
                         bool pool_first) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pool_only, dim3(B), dim3(kPoolThreads), 0, st, hn, Hp, gptr, H, g, g_out,
                     inv_cnt, pool_arg, pool_first);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// dzn from dg: k_readout_bwd_img's block = one 32-row step x 64 columns, fp32 dzn (nullable)
// and / or its e-image (nullable) through the same LDS tile and store pattern
// ------------------------------------------------------------------------------------------
constexpr int kImgCols = 64;

// the upstream value of dzn[v, n] is dg[graph(v) * H + n] (fp32, row stride H, read element-wise;
// pad columns n >= H: 0) in place of dy[graph(v)] * wf[n]; then, in k_readout_bwd_img's order,
// the gscale (mean pooling) factor, the max-pool pick (first arg-max node, or shared ties), and
// ReLU's h > 0 or act_grad(zn): a rank-1 dg = dy (x) wf reproduces the fused max-pool bits
__global__ __launch_bounds__(256) void k_readout_bwd_img_dg(
    const float* __restrict__ dg, const int* __restrict__ node_graph,
    const float* __restrict__ hn, const float* __restrict__ zn, int64_t N, int H, int Hp, int act,
    float* __restrict__ dzn, int colblocks, int cimg, b3_u4* __restrict__ img,
    const float* __restrict__ gscale, const int* __restrict__ pool_arg,
    const float* __restrict__ gpool) {
  __shared__ float tile[32][kImgCols + 1];
  const int64_t s = blockIdx.x / colblocks;
  const int c0 = (int)(blockIdx.x - s * colblocks) * kImgCols;
  for (int it = threadIdx.x; it < 32 * (kImgCols / 4); it += blockDim.x) {
    const int r = it / (kImgCols / 4), c4 = it - r * (kImgCols / 4);
    const int64_t v = s * 32 + r;
    const int n = c0 + 4 * c4;
    float4 o = f4zero();
    if (v < N && n < Hp) {
      const int64_t off = v * Hp + n;
      const int gv = node_graph[v];
      const float* dgr = dg + (int64_t)gv * H;
      o.x = n < H ? dgr[n] : 0.f;
      o.y = n + 1 < H ? dgr[n + 1] : 0.f;
      o.z = n + 2 < H ? dgr[n + 2] : 0.f;
      o.w = n + 3 < H ? dgr[n + 3] : 0.f;
      if (gscale) {
        const float gsc = gscale[gv];
        o = make_float4(o.x * gsc, o.y * gsc, o.z * gsc, o.w * gsc);
      }
      if (pool_arg) {  // global_max_pool (the pool kernel's record, kernels.hpp)
        const int4 am = *reinterpret_cast<const int4*>(pool_arg + (int64_t)gv * Hp + n);
        const float4 h = *reinterpret_cast<const float4*>(hn + off);
        const float4 gm = *reinterpret_cast<const float4*>(gpool + (int64_t)gv * Hp + n);
        // the first arg-max node (>= 0), or every node holding the max sharing (-count)
        auto pick = [&](float ov, int a, float hv, float gmv) {
          if (a >= 0) return a == v ? ov : 0.f;
          return hv == gmv ? ov / (float)(-a) : 0.f;
        };
        o.x = pick(o.x, am.x, h.x, gm.x);
        o.y = pick(o.y, am.y, h.y, gm.y);
        o.z = pick(o.z, am.z, h.z, gm.z);
        o.w = pick(o.w, am.w, h.w, gm.w);
      }
      if (act == ACT_RELU) {
        const float4 h = *reinterpret_cast<const float4*>(hn + off);
        o.x = h.x > 0.f ? o.x : 0.f;
        o.y = h.y > 0.f ? o.y : 0.f;
        o.z = h.z > 0.f ? o.z : 0.f;
        o.w = h.w > 0.f ? o.w : 0.f;
      } else {
        const float4 z = *reinterpret_cast<const float4*>(zn + off);
        o.x *= act_grad(z.x, act);
        o.y *= act_grad(z.y, act);
        o.z *= act_grad(z.z, act);
        o.w *= act_grad(z.w, act);
      }
      if (dzn) *reinterpret_cast<float4*>(dzn + off) = o;
    }
    if (img) {  // (b3_pack.hip's b3_tile_put: columns >= H of the image are 0)
      tile[r][4 * c4 + 0] = n + 0 < H ? o.x : 0.f;
      tile[r][4 * c4 + 1] = n + 1 < H ? o.y : 0.f;
      tile[r][4 * c4 + 2] = n + 2 < H ? o.z : 0.f;
      tile[r][4 * c4 + 3] = n + 3 < H ? o.w : 0.f;
    }
  }
  if (!img) return;
  __syncthreads();
  // (b3_pack.hip's b3_tile_to_eimage: thread = (column, 8-row chunk), chunk fastest)
  const int q = threadIdx.x & 3, cl = threadIdx.x >> 2;
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

hipError_t readout_act_bwd_dg(const float* dg, const int* node_graph, const float* hn,
                              const float* zn, int64_t N, int H, int Hp, int act, float* dzn,
                              void* img, hipStream_t st, const float* gscale,
                              const int* pool_arg, const float* gpool) {
  if (N <= 0 || (!dzn && !img)) return hipSuccess;
  const int colblocks = (int)cdiv(Hp, kImgCols);
  const int64_t blocks = cdiv(N, 32) * colblocks;
  hipLaunchKernelGGL(k_readout_bwd_img_dg, dim3((unsigned)blocks), dim3(256), 0, st, dg,
                     node_graph, hn, zn, N, H, Hp, act, dzn, colblocks, b3_eimg_cols(H),
                     static_cast<b3_u4*>(img), gscale, pool_arg, gpool);
  return hipGetLastError();
}

}  // namespace cgr
