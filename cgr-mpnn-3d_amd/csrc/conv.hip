// Standalone DMPNNConv (GNN.py:113-145) on the native kernels, in the caller's edge order:
//   a[v]  = sum_{dst(e) = v} h[e]                    (propagate, aggr="add", dim_size = N;
//                                                     aggr="mean": / max(in-degree, 1))
//   h'[e] = (a[src(e)] - h[e ^ 1]) W^T + b           (GNN.py:136-141)
// and its reverse mode.  GNN.forward never calls this (the fused path inlines the layer); it keeps
// the reference's public DMPNNConv usable on its own.
#include "dispatch.hpp"
#include "epilogues.hpp"
#include "gnn_internal.hpp"
#include "kernels.hpp"

namespace cgr {

int split_edges(const int64_t* ei, int E, int N, int* src_c, int* dst_c, hipStream_t st);
int csr_from_keys(const int* key, int n, int nb, int* deg, int* cursor, int* ptr, int* list,
                  hipStream_t st);

namespace {

struct ConvScratch {
  Reg<int> src_c, dst_c, perm, dst_ptr, src_perm, src_ptr, deg, cursor;
  Reg<float> h_p, a_p, dout_p, dm, da, wT, slab, bslab, inv_deg;
};

// the standalone conv's scratch: every region stated once (layout.hpp); returns the total bytes
size_t conv_regions(int64_t N, int64_t E, int64_t H, ConvScratch& s, Placer<>& v) {
  const size_t Hp = (size_t)round_up(H, 4);
  v(s.src_c, E);
  v(s.dst_c, E);
  v(s.perm, E);
  v(s.dst_ptr, N + 1);
  v(s.src_perm, E);
  v(s.src_ptr, N + 1);
  v(s.deg, N);
  v(s.cursor, N);
  v(s.h_p, E * Hp);
  v(s.a_p, N * Hp);
  v(s.dout_p, E * Hp);
  v(s.dm, E * Hp);
  v(s.da, N * Hp);
  v(s.wT, H * Hp);
  const WgChoice wg = wg_f32((int)H, (int)H, (int)E);  // dW = dout^T m (backward)
  v(s.slab, wg.slab_elems());
  v(s.bslab, wg.bslab_elems());
  v(s.inv_deg, N);
  return v.off;
}

ConvScratch conv_scratch(int64_t N, int64_t E, int64_t H, void* scratch) {
  ConvScratch s;
  Placer<> v{static_cast<char*>(scratch)};
  conv_regions(N, E, H, s, v);
  return s;
}

// da[v, :] += g[v, :H]  (g unpadded [N, H])
__global__ void k_add_rows(float* __restrict__ da, int64_t N, int H, int Hp,
                           const float* __restrict__ g) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * H) return;
  const int64_t v = t / H;
  const int c = (int)(t - v * H);
  da[v * Hp + c] += g[t];
}

// dh[e, :H] = da[dst(e)] (* inv_deg[dst(e)]: mean) - dm[e ^ 1]
__global__ void k_conv_dh(const float* __restrict__ da, const float* __restrict__ dm,
                          const int* __restrict__ dst_c, int64_t E, int H, int Hp,
                          float* __restrict__ dh, const float* __restrict__ inv_deg) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= E * H) return;
  const int64_t e = t / H;
  const int c = (int)(t - e * H);
  const int v = dst_c[e];
  const float s = inv_deg ? inv_deg[v] : 1.f;
  dh[t] = da[(int64_t)v * Hp + c] * s - dm[(e ^ 1) * Hp + c];
}

}  // namespace
}  // namespace cgr

using namespace cgr;

extern "C" {

int64_t cgr_dmpnn_conv_scratch_bytes(int64_t num_nodes, int64_t num_edges, int64_t hidden) {
  if (num_nodes < 1 || num_edges < 0 || hidden < 1) return -1;
  ConvScratch s;
  Placer<> v;
  return (int64_t)conv_regions(num_nodes, num_edges, hidden, s, v);
}

int cgr_dmpnn_conv_forward(const int64_t* edge_index, int64_t N, int64_t E, const float* h,
                           int64_t H, const float* weight, const float* bias, float* a_out,
                           float* h_out, void* scratch, int32_t aggregation, void* stream) {
  clear_stale_hip_error();
  CGR_CHECK(edge_index && h && weight && bias && a_out && h_out && scratch,
            "cgr_dmpnn_conv_forward: NULL pointer");
  CGR_CHECK(aggregation == CGR_AGGR_ADD || aggregation == CGR_AGGR_MEAN,
            "cgr_dmpnn_conv_forward: unknown aggregation");
  CGR_CHECK(N >= 1 && E >= 2 && E % 2 == 0 && H >= 1 && E < (1ll << 30) && N < (1ll << 31),
            "cgr_dmpnn_conv_forward: bad sizes (E must be even and > 0)");
  hipStream_t st = (hipStream_t)stream;
  const ConvScratch s = conv_scratch(N, E, H, scratch);
  const int Hp = (int)round_up(H, 4);
  int rc = split_edges(edge_index, (int)E, (int)N, s.src_c, s.dst_c, st);
  if (rc) return rc;
  rc = csr_from_keys(s.dst_c, (int)E, (int)N, s.deg, s.cursor, s.dst_ptr, s.perm, st);
  if (rc) return rc;
  rc = csr_from_keys(s.src_c, (int)E, (int)N, s.deg, s.cursor, s.src_ptr, s.src_perm, st);
  if (rc) return rc;
  HIP_RET(hipMemcpy2DAsync(s.h_p, Hp * 4, h, H * 4, H * 4, E, hipMemcpyDeviceToDevice, st));
  HIP_RET(segment_sum(s.h_p, Hp, s.perm, s.dst_ptr, N, Hp, s.a_p, Hp, st));
  if (aggregation == CGR_AGGR_MEAN) {  // the mean: a / max(in-degree, 1), kept for the backward
    HIP_RET(mean_scales(s.dst_ptr, N, nullptr, 0, s.inv_deg, nullptr, st));
    HIP_RET(scale_rows(s.a_p, Hp, N, s.inv_deg, st));
  }
  HIP_RET(hipMemcpy2DAsync(a_out, H * 4, s.a_p, Hp * 4, H * 4, N, hipMemcpyDeviceToDevice, st));
  const int vw = vec_for(weight, H, H);
  hipError_t e = with_vec(vw, [&](auto VW) {
    return with_nt_rn((int)H, [&](auto RN) {
      LdGatherDiff<true> al{s.a_p, s.h_p, s.src_c, nullptr, Hp};
      LdPlain<decltype(VW)::value> bl{weight, H};
      EpStore ep{h_out, H, (int)E, (int)H, bias};
      return launch_gemm_nt<4, 1, decltype(RN)::value, 1>(al, bl, ep, (int)E, (int)H, (int)H, st);
    });
  });
  HIP_RET(e);
  return 0;
}

int cgr_dmpnn_conv_backward(const int64_t* edge_index, int64_t N, int64_t E, const float* h,
                            int64_t H, const float* weight, const float* grad_a,
                            const float* grad_h_out, float* grad_h, float* grad_weight,
                            float* grad_bias, void* scratch, int32_t aggregation, void* stream) {
  clear_stale_hip_error();
  (void)edge_index;
  (void)h;
  CGR_CHECK(weight && grad_h && grad_weight && grad_bias && scratch,
            "cgr_dmpnn_conv_backward: NULL pointer");
  CGR_CHECK(aggregation == CGR_AGGR_ADD || aggregation == CGR_AGGR_MEAN,
            "cgr_dmpnn_conv_backward: unknown aggregation");
  CGR_CHECK(N >= 1 && E >= 2 && E % 2 == 0 && H >= 1, "cgr_dmpnn_conv_backward: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  const ConvScratch s = conv_scratch(N, E, H, scratch);
  const int Hp = (int)round_up(H, 4);
  if (grad_h_out) {
    HIP_RET(hipMemcpy2DAsync(s.dout_p, Hp * 4, grad_h_out, H * 4, H * 4, E, hipMemcpyDeviceToDevice,
                             st));
    // dW = dout^T m, db = colsum(dout)
    {
      LdPlain<4> al{s.dout_p, Hp};
      LdGatherDiff<true> bl{s.a_p, s.h_p, s.src_c, nullptr, Hp};
      const WgChoice wg = wg_f32((int)H, (int)H, (int)E);  // as conv_regions sized the slabs
      HIP_RET(wg_f32_launch(wg, al, bl, s.slab, s.bslab, true, st));
      HIP_RET(reduce_slabs(s.slab, s.bslab, wg.plan.splits, wg.Nout, wg.Kout, grad_weight, H, 0,
                           grad_bias, st));
    }
    TransposeJobs tj{};
    tj.job[0] = TransposeJob{weight, H, 0, s.wT, Hp, (int)H, (int)H};
    tj.n = 1;
    HIP_RET(transpose_batch(tj, st));
    hipError_t e = with_nt_rn((int)H, [&](auto RN) {
      LdPlain<4> al{s.dout_p, Hp};
      LdPlain<4> bl{s.wT, Hp};
      EpStore ep{s.dm, Hp, (int)E, (int)H, nullptr};
      return launch_gemm_nt<4, 1, decltype(RN)::value, 1>(al, bl, ep, (int)E, (int)H, (int)H, st);
    });
    HIP_RET(e);
    HIP_RET(segment_sum(s.dm, Hp, s.src_perm, s.src_ptr, N, Hp, s.da, Hp, st));
  } else {
    HIP_RET(hipMemsetAsync(grad_weight, 0, sizeof(float) * H * H, st));
    HIP_RET(hipMemsetAsync(grad_bias, 0, sizeof(float) * H, st));
    HIP_RET(hipMemsetAsync(s.dm, 0, sizeof(float) * E * Hp, st));
    HIP_RET(hipMemsetAsync(s.da, 0, sizeof(float) * N * Hp, st));
  }
  if (grad_a) {
    hipLaunchKernelGGL(k_add_rows, dim3(cdiv(N * H, 256)), dim3(256), 0, st, s.da, N, (int)H, Hp,
                       grad_a);
    HIP_RET(hipGetLastError());
  }
  hipLaunchKernelGGL(k_conv_dh, dim3(cdiv(E * H, 256)), dim3(256), 0, st, s.da, s.dm, s.dst_c, E,
                     (int)H, Hp, grad_h, aggregation == CGR_AGGR_MEAN ? s.inv_deg : nullptr);
  HIP_RET(hipGetLastError());
  return 0;
}

}  // extern "C"
