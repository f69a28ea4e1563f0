// On-device collation of a batch of reaction graphs from a device-resident graph store
// (replaces torch_geometric.loader.DataLoader / Batch.from_data_list as
// used by trainer.py:105-118 over the per-reaction Data of ChemDataset.py:81-94).
//
// The store is every graph of the dataset collated once (PyG layout): node rows of graph g are
// [node_ptr[g], node_ptr[g+1]) of x, its edges [edge_ptr[g], edge_ptr[g+1]) of edge_index /
// edge_attr with GLOBAL node ids.  Collating graph ids gid[0..B) gives exactly what
// Batch.from_data_list produces for those graphs in that order: node blocks concatenated, edge
// ids re-based to the running node count, batch[v] = position b, ptr = node offsets, y gathered.
//
// kCollateSlices workgroups per output graph: each sums the node / edge counts of the graphs
// before it (a block reduction over gid[0..b), O(B) reads -- no separate scan launch), then
// copies its slice of the graph's node rows (one contiguous block of x) and edge rows as 8-byte
// or 4-byte words, re-bases its edge ids, fills batch; slice 0 writes ptr and y.  Pure data
// movement: HBM-bound, bit-exact.
#include "gnn_internal.hpp"

namespace cgr {

constexpr int kCollateThreads = 256;
constexpr int kCollateSlices = 4;  // 4 workgroups per graph: ~1000 for a 256-graph batch

__device__ __forceinline__ int64_t block_sum_i64(int64_t v, int64_t* red) {
  // 256 threads = 4 waves
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const int64_t t = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return t;
}

// contiguous copy of n floats, src/dst offsets in floats; 8-byte words when both are 8-byte
// aligned, else 4-byte words
__device__ __forceinline__ void copy_floats(const float* __restrict__ src, float* __restrict__ dst,
                                            int64_t n, int slice) {
  // slice `slice` of kCollateSlices equal parts (even-sized, so 8-byte alignment is kept)
  const int64_t part = ((n + kCollateSlices - 1) / kCollateSlices + 1) & ~int64_t(1);
  const int64_t lo = min(n, part * slice);
  src += lo;
  dst += lo;
  n = min(n, lo + part) - lo;
  const bool al8 = (((uintptr_t)src | (uintptr_t)dst) & 7) == 0;
  if (al8) {
    const int64_t n2 = n >> 1;
    const float2* s2 = reinterpret_cast<const float2*>(src);
    float2* d2 = reinterpret_cast<float2*>(dst);
    int64_t i = threadIdx.x;
    for (; i + 3 * kCollateThreads < n2; i += 4 * kCollateThreads) {  // 4 loads in flight
      const float2 a = s2[i], b = s2[i + kCollateThreads], c = s2[i + 2 * kCollateThreads],
                   d = s2[i + 3 * kCollateThreads];
      d2[i] = a;
      d2[i + kCollateThreads] = b;
      d2[i + 2 * kCollateThreads] = c;
      d2[i + 3 * kCollateThreads] = d;
    }
    for (; i < n2; i += kCollateThreads) d2[i] = s2[i];
    if ((n & 1) && threadIdx.x == 0) dst[n - 1] = src[n - 1];
  } else {
    for (int64_t i = threadIdx.x; i < n; i += kCollateThreads) dst[i] = src[i];
  }
}

__global__ __launch_bounds__(kCollateThreads) void k_collate(
    const int64_t* __restrict__ gid, int64_t B, const int64_t* __restrict__ node_ptr,
    const int64_t* __restrict__ edge_ptr, const float* __restrict__ x, int64_t F,
    const int64_t* __restrict__ ei, int64_t E_all, const float* __restrict__ ea, int64_t Fe,
    const float* __restrict__ y, float* __restrict__ x_out, int64_t* __restrict__ ei_out,
    int64_t E_out, float* __restrict__ ea_out, int64_t* __restrict__ batch_out,
    int64_t* __restrict__ ptr_out, float* __restrict__ y_out) {
  __shared__ int64_t red[4];
  const int64_t b = blockIdx.x / kCollateSlices;
  const int slice = (int)(blockIdx.x % kCollateSlices);
  // offsets of this graph in the output = counts of the graphs before it
  int64_t pn = 0, pe = 0;
  for (int64_t i = threadIdx.x; i < b; i += kCollateThreads) {
    const int64_t g = gid[i];
    pn += node_ptr[g + 1] - node_ptr[g];
    pe += edge_ptr[g + 1] - edge_ptr[g];
  }
  const int64_t on = block_sum_i64(pn, red);
  const int64_t oe = block_sum_i64(pe, red);
  const int64_t g = gid[b];
  const int64_t n0 = node_ptr[g], nn = node_ptr[g + 1] - n0;
  const int64_t e0 = edge_ptr[g], ne = edge_ptr[g + 1] - e0;
  if (threadIdx.x == 0 && slice == 0) {
    ptr_out[b] = on;
    if (b == B - 1) ptr_out[B] = on + nn;
    if (y) y_out[b] = y[g];
  }
  copy_floats(x + n0 * F, x_out + on * F, nn * F, slice);
  if (Fe > 0) copy_floats(ea + e0 * Fe, ea_out + oe * Fe, ne * Fe, slice);
  const int t = slice * kCollateThreads + threadIdx.x, T = kCollateSlices * kCollateThreads;
  for (int64_t v = t; v < nn; v += T) batch_out[on + v] = b;
  const int64_t shift = on - n0;
  for (int64_t e = t; e < ne; e += T) {
    ei_out[oe + e] = ei[e0 + e] + shift;
    ei_out[E_out + oe + e] = ei[E_all + e0 + e] + shift;
  }
}

// ---- fixed-shape collation (cgr_collate_padded) ---------------------------------------------
// The same real region as k_collate, then one pad graph (slot B) that fills the outputs up to
// the capacities, so a captured training step can replay over ragged batches with frozen launch
// arguments.  Grid = B * kCollateSlices real workgroups + a pad-fill tail whose size depends on
// the capacities only.  Every write is bounded by the capacities on the device: a batch that
// does not fit sets info[2] and leaves the rest of the outputs unspecified, never out of range.

constexpr int kPadElemsPerBlock = kCollateThreads * 64;  // floats zeroed per pad workgroup (sizing)
constexpr int kPadBlocksMax = 512;

__host__ __device__ inline int64_t pad_blocks(int64_t N_cap, int64_t F, int64_t E_cap, int64_t Fe) {
  const int64_t work = N_cap * (F + 2) + E_cap * (Fe + 4);
  const int64_t nb = (work + kPadElemsPerBlock - 1) / kPadElemsPerBlock;
  return nb < 1 ? 1 : (nb > kPadBlocksMax ? kPadBlocksMax : nb);
}

// node / edge count of graph id g; an id outside [0, G) counts as an empty graph (flagged)
__device__ __forceinline__ bool graph_counts(int64_t g, int64_t G, const int64_t* node_ptr,
                                             const int64_t* edge_ptr, int64_t& nn, int64_t& ne) {
  if (g < 0 || g >= G) {
    nn = ne = 0;
    return false;
  }
  nn = node_ptr[g + 1] - node_ptr[g];
  ne = edge_ptr[g + 1] - edge_ptr[g];
  return true;
}

// zero n floats at p: thread t of T, 16-byte stores over the aligned middle
__device__ __forceinline__ void zero_floats(float* p, int64_t n, int64_t t, int64_t T) {
  int64_t head = (int64_t)((16 - ((uintptr_t)p & 15)) & 15) >> 2;
  if (head > n) head = n;
  const int64_t n4 = (n - head) >> 2;
  float4* p4 = reinterpret_cast<float4*>(p + head);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t i = t; i < n4; i += T) p4[i] = z;
  const int64_t tail0 = head + 4 * n4;
  if (t < head) p[t] = 0.f;
  if (t < n - tail0) p[tail0 + t] = 0.f;
}

enum : int64_t {
  kPadStatusOverflow = 1,  // N_real + 2 > N_cap or E_real > E_cap
  kPadStatusOddEdges = 2,  // E_cap - E_real is odd: the pad edges cannot be reverse pairs
  kPadStatusBadId = 4,     // a graph id outside [0, G) (treated as an empty graph)
};

__global__ __launch_bounds__(kCollateThreads) void k_collate_padded(
    const int64_t* __restrict__ gid, const float* __restrict__ slot_weight, int64_t B, int64_t G,
    const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ edge_ptr,
    const float* __restrict__ x, int64_t F, const int64_t* __restrict__ ei, int64_t E_all,
    const float* __restrict__ ea, int64_t Fe, const float* __restrict__ y, int64_t N_cap,
    int64_t E_cap, float* __restrict__ x_out, int64_t* __restrict__ ei_out,
    float* __restrict__ ea_out, int64_t* __restrict__ batch_out, int64_t* __restrict__ ptr_out,
    float* __restrict__ y_out, float* __restrict__ mask_out, int64_t* __restrict__ info) {
  __shared__ int64_t red[4];
  const int64_t real_blocks = B * kCollateSlices;
  if ((int64_t)blockIdx.x < real_blocks) {
    // ---- real region: k_collate's work for output slot b, bounded by the capacities
    const int64_t b = blockIdx.x / kCollateSlices;
    const int slice = (int)(blockIdx.x % kCollateSlices);
    int64_t pn = 0, pe = 0;
    for (int64_t i = threadIdx.x; i < b; i += kCollateThreads) {
      int64_t nn_i, ne_i;
      graph_counts(gid[i], G, node_ptr, edge_ptr, nn_i, ne_i);
      pn += nn_i;
      pe += ne_i;
    }
    const int64_t on = block_sum_i64(pn, red);
    const int64_t oe = block_sum_i64(pe, red);
    const int64_t g = gid[b];
    int64_t nn, ne;
    const bool valid = graph_counts(g, G, node_ptr, edge_ptr, nn, ne);
    if (threadIdx.x == 0 && slice == 0) {
      ptr_out[b] = on < N_cap ? on : N_cap;
      if (y) y_out[b] = valid ? y[g] : 0.f;
      mask_out[b] = slot_weight[b];
    }
    if (!valid || on + nn > N_cap || oe + ne > E_cap) return;  // uniform over the workgroup
    const int64_t n0 = node_ptr[g], e0 = edge_ptr[g];
    copy_floats(x + n0 * F, x_out + on * F, nn * F, slice);
    if (Fe > 0) copy_floats(ea + e0 * Fe, ea_out + oe * Fe, ne * Fe, slice);
    const int t = slice * kCollateThreads + threadIdx.x, T = kCollateSlices * kCollateThreads;
    for (int64_t v = t; v < nn; v += T) batch_out[on + v] = b;
    const int64_t shift = on - n0;
    for (int64_t e = t; e < ne; e += T) {
      ei_out[oe + e] = ei[e0 + e] + shift;
      ei_out[E_cap + oe + e] = ei[E_all + e0 + e] + shift;
    }
    return;
  }
  // ---- pad graph (slot B): every pad workgroup reduces over all B ids, then fills grid-stride
  const int64_t pb = (int64_t)blockIdx.x - real_blocks;
  const int64_t PB = (int64_t)gridDim.x - real_blocks;
  int64_t pn = 0, pe = 0, bad = 0;
  for (int64_t i = threadIdx.x; i < B; i += kCollateThreads) {
    int64_t nn_i, ne_i;
    if (!graph_counts(gid[i], G, node_ptr, edge_ptr, nn_i, ne_i)) bad = 1;
    pn += nn_i;
    pe += ne_i;
  }
  const int64_t N_real = block_sum_i64(pn, red);
  const int64_t E_real = block_sum_i64(pe, red);
  const int64_t any_bad = block_sum_i64(bad, red);
  int64_t status = any_bad ? kPadStatusBadId : 0;
  if (N_real + 2 > N_cap || E_real > E_cap) status |= kPadStatusOverflow;
  else if ((E_cap - E_real) & 1) status |= kPadStatusOddEdges;
  if (pb == 0 && threadIdx.x == 0) {
    info[0] = N_real;
    info[1] = E_real;
    info[2] = status;
    info[3] = 0;
    ptr_out[B] = N_real < N_cap ? N_real : N_cap;
    ptr_out[B + 1] = N_cap;
    if (y) y_out[B] = 0.f;
    mask_out[B] = 0.f;
  }
  if (status & (kPadStatusOverflow | kPadStatusOddEdges)) return;
  const int64_t t = pb * kCollateThreads + threadIdx.x, T = PB * kCollateThreads;
  const int64_t P = N_cap - N_real;         // >= 2
  const int64_t Ep = (E_cap - E_real) >> 1;  // pad edge pairs
  zero_floats(x_out + N_real * F, P * F, t, T);
  if (Fe > 0) zero_floats(ea_out + E_real * Fe, 2 * Ep * Fe, t, T);
  for (int64_t i = t; i < P; i += T) batch_out[N_real + i] = B;
  // pair j: edges (a -> b), (b -> a) along the ring of pad nodes: rev(e) = e ^ 1 as in real graphs
  for (int64_t j = t; j < Ep; j += T) {
    const int64_t a = N_real + j % P, b = N_real + (j + 1) % P;
    const int64_t e = E_real + 2 * j;
    ei_out[e] = a;
    ei_out[e + 1] = b;
    ei_out[E_cap + e] = b;
    ei_out[E_cap + e + 1] = a;
  }
}

}  // namespace cgr

using namespace cgr;

extern "C" int cgr_collate(const int64_t* graph_ids, int64_t num_ids, const int64_t* node_ptr,
                           const int64_t* edge_ptr, const float* x, int64_t num_node_features,
                           const int64_t* edge_index, int64_t num_edges_all,
                           const float* edge_attr, int64_t num_edge_features, const float* y,
                           float* x_out, int64_t* edge_index_out, int64_t num_edges_out,
                           float* edge_attr_out, int64_t* batch_out, int64_t* ptr_out,
                           float* y_out, void* stream) {
  clear_stale_hip_error();
  CGR_CHECK(num_ids >= 0, "cgr_collate: negative batch size");
  if (num_ids == 0) return 0;
  CGR_CHECK(graph_ids && node_ptr && edge_ptr && x && edge_index && x_out && edge_index_out &&
                batch_out && ptr_out,
            "cgr_collate: NULL pointer");
  CGR_CHECK(num_edge_features == 0 || (edge_attr && edge_attr_out),
            "cgr_collate: edge_attr pointers missing");
  CGR_CHECK(!y || y_out, "cgr_collate: y_out missing");
  CGR_CHECK(num_node_features >= 0 && num_edge_features >= 0 && num_edges_all >= 0 &&
                num_edges_out >= 0,
            "cgr_collate: bad sizes");
  CGR_CHECK(num_ids < (1LL << 28), "cgr_collate: too many graphs");
  hipLaunchKernelGGL(k_collate, dim3((unsigned)(num_ids * kCollateSlices)), dim3(kCollateThreads), 0,
                     (hipStream_t)stream, graph_ids, num_ids, node_ptr, edge_ptr, x,
                     num_node_features, edge_index, num_edges_all, edge_attr, num_edge_features,
                     y, x_out, edge_index_out, num_edges_out, edge_attr_out, batch_out, ptr_out,
                     y_out);
  HIP_RET(hipGetLastError());
  return 0;
}

extern "C" int cgr_collate_padded(const int64_t* graph_ids, const float* slot_weight,
                                  int64_t num_ids, int64_t num_graphs_all, const int64_t* node_ptr,
                                  const int64_t* edge_ptr, const float* x,
                                  int64_t num_node_features, const int64_t* edge_index,
                                  int64_t num_edges_all, const float* edge_attr,
                                  int64_t num_edge_features, const float* y, int64_t node_cap,
                                  int64_t edge_cap, float* x_out, int64_t* edge_index_out,
                                  float* edge_attr_out, int64_t* batch_out, int64_t* ptr_out,
                                  float* y_out, float* mask_out, int64_t* info, void* stream) {
  clear_stale_hip_error();
  CGR_CHECK(num_ids >= 1, "cgr_collate_padded: batch size must be at least 1");
  CGR_CHECK(graph_ids && slot_weight && node_ptr && edge_ptr && x && edge_index && x_out &&
                edge_index_out && batch_out && ptr_out && mask_out && info,
            "cgr_collate_padded: NULL pointer");
  CGR_CHECK(num_edge_features == 0 || (edge_attr && edge_attr_out),
            "cgr_collate_padded: edge_attr pointers missing");
  CGR_CHECK(!y || y_out, "cgr_collate_padded: y_out missing");
  CGR_CHECK(num_node_features >= 0 && num_edge_features >= 0 && num_edges_all >= 0 &&
                num_graphs_all >= 0,
            "cgr_collate_padded: bad sizes");
  CGR_CHECK(node_cap >= 2 && edge_cap >= 0 && (edge_cap & 1) == 0,
            "cgr_collate_padded: node_cap must be at least 2 and edge_cap even");
  CGR_CHECK(num_ids < (1LL << 28), "cgr_collate_padded: too many graphs");
  const int64_t blocks = num_ids * kCollateSlices +
                         pad_blocks(node_cap, num_node_features, edge_cap, num_edge_features);
  hipLaunchKernelGGL(k_collate_padded, dim3((unsigned)blocks), dim3(kCollateThreads), 0,
                     (hipStream_t)stream, graph_ids, slot_weight, num_ids, num_graphs_all,
                     node_ptr, edge_ptr, x, num_node_features, edge_index, num_edges_all,
                     edge_attr, num_edge_features, y, node_cap, edge_cap, x_out, edge_index_out,
                     edge_attr_out, batch_out, ptr_out, y_out, mask_out, info);
  HIP_RET(hipGetLastError());
  return 0;
}
