// The two kernels of the nodes level (cgr_gnn_encode_nodes*, gnn_fwd.hip / gnn_bwd.hip): the
// per-atom embedding hn handed out as n_out [N, H], and dzn from a cotangent dn [N, H] of it.
// Neither knows of graphs or pooling: no node_graph gather, no mean factor, no max-pool pick.
// Like encode_kernels.hip they live in a translation unit of their own, linked last, so that the
// code objects of every other kernel are byte for byte what they were without this file.
#include "bwd_rows.hpp"
#include "common.hpp"
#include "gemm_b3.hpp"
#include "gemm_b3tn.hpp"
#include "kernels.hpp"

namespace cgr {

// ------------------------------------------------------------------------------------------
// n_out [N, H] (row stride H) from hn [N, Hp]: one thread per float4 column group of hn.  n_out's
// rows are only 4-byte aligned when H % 4 != 0 and a row's last group must not reach into the
// next row (or past the buffer), so n_out is stored element by element, columns < H only
// ------------------------------------------------------------------------------------------
constexpr int kNodesOutThreads = 256;

__global__ __launch_bounds__(kNodesOutThreads) void k_nodes_out(const float* __restrict__ hn,
                                                                int Hp, int64_t N, int H,
                                                                float* __restrict__ n_out) {
  const int C4 = Hp >> 2;
  const int64_t t = (int64_t)blockIdx.x * kNodesOutThreads + threadIdx.x;
  if (t >= N * C4) return;
  const int64_t v = t / C4;
  const int n = 4 * (int)(t - v * C4);
  const float4 x = *reinterpret_cast<const float4*>(hn + v * Hp + n);
  const float xv[4] = {x.x, x.y, x.z, x.w};
  float* row = n_out + v * H;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (n + k < H) row[n + k] = xv[k];
}

hipError_t nodes_out_fwd(const float* hn, int Hp, int64_t N, int H, float* n_out,
                         hipStream_t st) {
  if (N <= 0) return hipSuccess;
  const int64_t blocks = cdiv(N * (Hp >> 2), kNodesOutThreads);
  hipLaunchKernelGGL(k_nodes_out, dim3((unsigned)blocks), dim3(kNodesOutThreads), 0, st, hn, Hp,
                     N, H, n_out);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// dzn from dn: k_readout_bwd_img's block = one 32-row step x 64 columns, fp32 dzn (nullable)
// and / or its e-image (nullable) through the same LDS tile and store pattern
// ------------------------------------------------------------------------------------------
constexpr int kImgCols = 64;

// dzn[v, n] = dn[v * H + n] * act'(zn[v, n]) (ReLU: hn[v, n] > 0 ? dn : 0); dn is fp32 with row
// stride H, read element-wise; pad columns n >= H of dzn and of the image are 0
__global__ __launch_bounds__(256) void k_nodes_bwd_img(
    const float* __restrict__ dn, const float* __restrict__ hn, const float* __restrict__ zn,
    int64_t N, int H, int Hp, int act, float* __restrict__ dzn, int colblocks, int cimg,
    b3_u4* __restrict__ img) {
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
      const float* dnr = dn + v * H;
      o.x = n < H ? dnr[n] : 0.f;
      o.y = n + 1 < H ? dnr[n + 1] : 0.f;
      o.z = n + 2 < H ? dnr[n + 2] : 0.f;
      o.w = n + 3 < H ? dnr[n + 3] : 0.f;
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

hipError_t nodes_act_bwd(const float* dn, const float* hn, const float* zn, int64_t N, int H,
                         int Hp, int act, float* dzn, void* img, hipStream_t st) {
  if (N <= 0 || (!dzn && !img)) return hipSuccess;
  const int colblocks = (int)cdiv(Hp, kImgCols);
  const int64_t blocks = cdiv(N, 32) * colblocks;
  hipLaunchKernelGGL(k_nodes_bwd_img, dim3((unsigned)blocks), dim3(256), 0, st, dn, hn, zn, N, H,
                     Hp, act, dzn, colblocks, b3_eimg_cols(H), static_cast<b3_u4*>(img));
  return hipGetLastError();
}

}  // namespace cgr
