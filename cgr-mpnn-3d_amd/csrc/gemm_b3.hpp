// fp32 GEMMs on the bf16 matrix cores (gfx950 v_mfma_f32_16x16x32_bf16): three-piece split.
//
// An fp32 operand x is split x = p0 + p1 + p2 (+ r): p0 = bf16(x) (round to nearest even),
// p1 = bf16(x - p0), p2 = bf16(x - p0 - p1), every remainder exact in fp32, |r| <= 2^-24 |x|.
// A product a.b is the sum of the six piece products that can reach 2^-16 |ab| (p1p1, p0p2, p2p0,
// p0p1, p1p0, p0p0; dropped terms <= 2^-23 |ab|), each bf16 x bf16 product exact, all accumulated
// in fp32 by the MFMA.  The error is at the level of an fp32 GEMM's own rounding
// (tools/experiments/fp16_split_precision_sim.py, profiles/r02_split_precision_experiment.txt:
// gradients 2-4e-7 vs 4-14e-7 for a plain fp32 GEMM against the fp64 oracle).  The bf16 MFMA
// runs 16x the fp32 MFMA rate (MI355X_MICROARCH.md § Matrix cores), so six of them cost 3/8 of
// the matrix-core time of v_mfma_f32_16x16x4_f32; what bounds these kernels is operand delivery.
//
// NT: C[m, n] = sum_k A(m, k) B(n, k) (epilogue functors of epilogues.hpp).
//   * B (a weight matrix, small, read by every workgroup) is split ONCE per training step by
//     b3_pack (kernels: b3_pack.hip) into an *image*: per 32-deep k step ks and piece p a plane of
//     Nimg rows x 64 bytes; row n's 16-byte slot s holds the lane-group-c chunk c = s ^ lds_swz(n)
//     (8 bf16 of k = 32 ks + b3_kperm(c, j)).  A workgroup copies its column block of the plane
//     verbatim into LDS: the swizzle is baked into the image, so every B fragment read is one
//     conflict-free ds_read_b128 (the 64-byte-row geometry of gemm.hpp).
//   * A (the streamed, large operand: gathered messages, dpre, x, s, dzn) goes straight from
//     global memory into the lane's registers in MFMA fragment shape -- each A element belongs to
//     exactly one wave, so it is loaded once and split once (VALU), never staged through LDS.
//     The k permutation b3_kperm (lane group g holds k = 4g..4g+3 and 16+4g..16+4g+3) makes each
//     fragment load two float4s whose four lane groups cover 64 contiguous bytes of the row.
//   * workgroup = WAVES waves, wave w owns RF 16-row fragments and all NF 16-column fragments of
//     the tile (BM = 16 WAVES RF rows x BN = 16 NF columns); B goes through three LDS buffers, A
//     and B are loaded into registers two k steps ahead (unconditional in-bounds loads: no
//     vmcnt(0) merges), and each step's loads, LDS stores and A split are spread over its MFMAs,
//     which run over the column fragments in pairs.
//   * the last k step has nothing left to stage: an addend epilogue (EpLayer, EpLayerSeg,
//     EpReadoutQ) loads its addend (bias, skip term, Q) there, in MFMA layout, and adds it to the
//     accumulators before they leave the registers.
//   * epilogue: accumulators -> LDS [BM][BN+4] -> float4 row pieces, in one of three shapes.
//     Plain (EpSplit2, EpStoreRowScale, ...): one column group per thread, its constants and row
//     operands loaded before the accumulators go through LDS.  Addend-flat (EpLayer, EpReadoutQ):
//     the tile's pieces flat (piece tid + NT * pass, every lane busy).  Whole-tile (kTile): the
//     kernel builds the tile's dst-segment structure in LDS (B3NtEpiLds) and hands everything to
//     the functor's tile(), where the segment passes are described: ep_fwd.hpp, ep_bwd.hpp.
// (The weight gradients' TN kernel on the same primitives: gemm_b3tn.hpp.)
#pragma once

#include <type_traits>

#include "epilogues.hpp"
#include "gemm.hpp"
#include "handoff.hpp"
#include "reduce.hpp"
#include "stamps.hpp"

namespace cgr {

typedef __bf16 b3_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 b3_bf16x8 __attribute__((ext_vector_type(8)));
typedef float b3_floatx2 __attribute__((ext_vector_type(2)));
// 16-byte fragments / image chunks as a native vector (a HIP_vector_type uint4 copy lowers to a
// memcpy through a private alloca: scratch traffic and a vmcnt(0) right behind every load)
typedef uint32_t b3_u4 __attribute__((ext_vector_type(4)));

constexpr int B3_BK = 32;  // k per MFMA step

// element j (0..7) of lane group g holds k = b3_kperm(g, j) of a 32-deep step
__host__ __device__ constexpr int b3_kperm(int g, int j) {
  return j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4);
}

// 2 fp32 -> packed bf16x2 (RNE, v_cvt_pk_bf16_f32) and the two values it represents
__device__ __forceinline__ uint32_t b3_cvt2(float a, float b, float& fa, float& fb) {
  const uint32_t u =
      __builtin_bit_cast(uint32_t, __builtin_convertvector(b3_floatx2{a, b}, b3_bf16x2));
  fa = __uint_as_float(u << 16);
  fb = __uint_as_float(u & 0xffff0000u);
  return u;
}

// 8 fp32 -> P packed bf16x8 pieces (element 0 in the low half of word 0)
template <int P>
__device__ __forceinline__ void b3_split8(const float (&v)[8], b3_u4 (&out)[P]) {
  uint32_t w[P][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float a = v[2 * q], b = v[2 * q + 1];
#pragma unroll
    for (int i = 0; i < P; ++i) {
      float fa, fb;
      w[i][q] = b3_cvt2(a, b, fa, fb);
      a -= fa;
      b -= fb;
    }
  }
#pragma unroll
  for (int i = 0; i < P; ++i) out[i] = b3_u4{w[i][0], w[i][1], w[i][2], w[i][3]};
}

// sched_group_barrier with a count known only after unrolling (the builtin needs literals)
template <int MASK>
__device__ __forceinline__ void b3_sgb(int n) {
  switch (n) {
    case 1: __builtin_amdgcn_sched_group_barrier(MASK, 1, 0); break;
    case 2: __builtin_amdgcn_sched_group_barrier(MASK, 2, 0); break;
    case 3: __builtin_amdgcn_sched_group_barrier(MASK, 3, 0); break;
    case 4: __builtin_amdgcn_sched_group_barrier(MASK, 4, 0); break;
    case 5: __builtin_amdgcn_sched_group_barrier(MASK, 5, 0); break;
    case 6: __builtin_amdgcn_sched_group_barrier(MASK, 6, 0); break;
    case 7: __builtin_amdgcn_sched_group_barrier(MASK, 7, 0); break;
    case 8: __builtin_amdgcn_sched_group_barrier(MASK, 8, 0); break;
    default: break;
  }
}

__device__ __forceinline__ floatx4 b3_mfma(const b3_u4& a, const b3_u4& b, const floatx4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b3_bf16x8, a),
                                                 __builtin_bit_cast(b3_bf16x8, b), c, 0, 0, 0);
}

// One 32-deep step of a row fragment against a pair of column fragments, from three-piece
// fragments: accx += a.b and (two) accy += a.c, six piece products each, smallest terms first,
// the two chains alternating so that two independent accumulators are in flight.  A last, single
// column (!two) passes its own accumulator as accy, which is then left alone.
__device__ __forceinline__ void b3_mfma6x2(const b3_u4 (&a)[3], const b3_u4 (&b)[3],
                                           const b3_u4 (&c)[3], bool two, floatx4& accx,
                                           floatx4& accy) {
  floatx4 x = accx;
  floatx4 y = accy;
  x = b3_mfma(a[1], b[1], x);
  if (two) y = b3_mfma(a[1], c[1], y);
  x = b3_mfma(a[0], b[2], x);
  if (two) y = b3_mfma(a[0], c[2], y);
  x = b3_mfma(a[2], b[0], x);
  if (two) y = b3_mfma(a[2], c[0], y);
  x = b3_mfma(a[0], b[1], x);
  if (two) y = b3_mfma(a[0], c[1], y);
  x = b3_mfma(a[1], b[0], x);
  if (two) y = b3_mfma(a[1], c[0], y);
  x = b3_mfma(a[0], b[0], x);
  if (two) y = b3_mfma(a[0], c[0], y);
  accx = x;
  if (two) accy = y;
}

// ------------------------------------------------------------------------------------------
// B images
// ------------------------------------------------------------------------------------------
// column tiling of an NT GEMM with N output columns: tiles of nf 16-column fragments (nf from
// the instantiated set), image rows nimg = tiles * nf * 16 (rows >= N are zero)
struct B3Cols {
  int tiles, nf, nimg;
};
// the instantiated fragment counts per tile (launch_b3nt's switch).  acc: the per-k-step
// accumulation variant of the NT kernel (CGR_PRECISION_FP32) keeps a pair's step sums beside the
// running sums, so its tiles stop at kB3AccMaxNf fragment columns (at 11 and 13 it spills)
constexpr int kB3MaxNf = 13, kB3AccMaxNf = 8;
inline int b3_nf_snap(int nf, bool acc = false) {
  static const int sizes[] = {1, 2, 3, 4, 6, 7, 8, 11, 13};
  const int top = acc ? kB3AccMaxNf : kB3MaxNf;
  for (int s : sizes)
    if (s >= nf && s <= top) return s;
  return top;
}
inline B3Cols b3_cols(int N, bool acc = false) {
  const int nft = (N + 15) / 16;
  const int top = acc ? kB3AccMaxNf : kB3MaxNf;
  const int tiles = (nft + top - 1) / top;
  int nf = (nft + tiles - 1) / tiles;
  nf = b3_nf_snap(nf, acc);
  return B3Cols{tiles, nf, tiles * nf * 16};
}
inline int b3_nk(int K) { return (K + B3_BK - 1) / B3_BK; }
// b3_u4 elements of an image (3 pieces) in the column tiling c
inline size_t b3_img_u4(const B3Cols& c, int K) { return (size_t)b3_nk(K) * 3 * c.nimg * 4; }
inline size_t b3_img_u4(int N, int K) { return b3_img_u4(b3_cols(N), K); }

// one pack job: image rows [n_begin, n_begin + rows) from B(n, k) = src[n * ldn + k * ldk]
// (n < N real rows of this job, zero beyond; k < K real, zero beyond), times kscale[k] when set
struct B3PackJob {
  const float* src;
  int64_t ldn, ldk;
  b3_u4* img;
  int n_begin, rows, N, K, nimg, nk;
  const float* kscale;
};
constexpr int kMaxB3PackJobs = 24;  // per launch (kernel-argument size); b3_pack_all splits
struct B3PackJobs {
  B3PackJob job[kMaxB3PackJobs];
  int n;
};
// small independent jobs that ride in a pack launch (the forward start, gnn_fwd.hip: one launch
// per queue instead of three); each part is off when its pointer is null
struct B3PackRiders {
  // t_dst[c * t_ld_dst + r] = t_src[r * t_ld_src + c], r < t_rows, c < t_cols
  const float* t_src = nullptr;
  int64_t t_ld_src = 0;
  float* t_dst = nullptr;
  int64_t t_ld_dst = 0;
  int t_rows = 0, t_cols = 0;
  // z_u4 16-byte words of zeros at z_dst
  void* z_dst = nullptr;
  int64_t z_u4 = 0;
  // p_dst[r, :p_ld] = p_src[r, :p_F] then zeros, r < p_rows (pad_rows; p_ld % 4 == 0)
  const float* p_src = nullptr;
  float* p_dst = nullptr;
  int64_t p_rows = 0;
  int p_F = 0, p_ld = 0;
};
hipError_t b3_pack(const B3PackJobs& jobs, hipStream_t st, const B3PackRiders* riders = nullptr);
// append a job, launching the batch when it is full
inline hipError_t b3_pack_add(B3PackJobs& jobs, const B3PackJob& j, hipStream_t st) {
  if (jobs.n == kMaxB3PackJobs) {
    const hipError_t e = b3_pack(jobs, st);
    if (e != hipSuccess) return e;
    jobs.n = 0;
  }
  jobs.job[jobs.n++] = j;
  return hipSuccess;
}
// image job for B(n, k) = src[n * ldn + k * ldk], n < N, k < K, into an image of its own
inline B3PackJob b3_job(const float* src, int64_t ldn, int64_t ldk, int N, int K, void* img,
                        const B3Cols& c) {
  return B3PackJob{src, ldn, ldk, static_cast<b3_u4*>(img), 0, c.nimg, N, K, c.nimg, b3_nk(K)};
}
inline B3PackJob b3_job(const float* src, int64_t ldn, int64_t ldk, int N, int K, void* img) {
  return b3_job(src, ldn, ldk, N, K, img, b3_cols(N));
}

// ------------------------------------------------------------------------------------------
// NT kernel
// ------------------------------------------------------------------------------------------
// Optional traits of an epilogue functor EP, each detected: b3_ep_X<EP>::value is EP::kX where the
// functor declares it, else false.
#define B3_EP_TRAIT(name, member)                 \
  template <class EP, class = void>               \
  struct name : std::false_type {};               \
  template <class EP>                             \
  struct name<EP, std::void_t<decltype(EP::member)>> : std::bool_constant<EP::member> {}
// kTile: takes the whole accumulator tile and its dst-segment structure in LDS, ep.tile(B3NtTile)
// (EpLayerSeg: ep_fwd.hpp, EpLayerBwdSeg: ep_bwd.hpp); kStarts: such a functor that also wants the
// list of the tile's segment-start rows
B3_EP_TRAIT(b3_ep_tile, kTile);
B3_EP_TRAIT(b3_ep_starts, kStarts);
// kAddend: takes its addend (bias, skip term, Q, ...) into the accumulators in MFMA layout, its
// loads issued in the last k step (EpLayer, EpReadoutQ)
B3_EP_TRAIT(b3_ep_addend, kAddend);
// kAct: applies an activation `act`; the kernel switches on it once, outside its epilogue loop,
// and hands it to the functor as a template constant
B3_EP_TRAIT(b3_ep_act, kAct);
// kSideBlock: may carry one workgroup of independent work (EpSplit2: the graph bookkeeping beside
// the x-GEMM, prep_one.hpp): when ep.side_on, the launch has one extra, LAST workgroup (the tiles
// keep their XCD mapping) that runs ep.side(lds) instead of a tile, with the tile's LDS
B3_EP_TRAIT(b3_ep_side, kSideBlock);
#undef B3_EP_TRAIT

// The epilogue's LDS, over the dead stage buffers: its regions in order, each once, in 4-byte
// words.  (The words behind C belong to the whole-tile functors; kernels with static LDS cannot be
// given the full 160 KB dynamically, so they ride in the dynamic block.)
enum B3NtEpiRegion {
  kEpiC,       // the accumulator tile [BM][BN + 4]
  kEpiSd,      // BM + 2: dst of rows m0 - 1 .. m0 + BM, distinct negative sentinels outside [0, M)
  kEpiRed,     // 8: one reduction word per wave (EpLayerBwdSeg's block sums)
  kEpiMask,    // 4: segment-start mask (handoff.hpp) of rows 0..63, 64..127; then 1 spare word
  kEpiLate,    // 1: an unpaired completer gave up waiting (EpLayerBwdSeg)
  kEpiDone,    // 2: the nodes of the head / tail segment this workgroup completes, or -1
  kEpiStarts,  // BM + 1: the tile's segment-start rows, a half per 64 rows (EpLayerSeg)
  kEpiEnd
};
constexpr int b3nt_epi_off(int BM, int BN, int region) {  // first word of a region
  const int words[kEpiEnd] = {BM * (BN + 4), BM + 2, 8, 4 + 1, 1, 2, BM + 1};
  int o = 0;
  for (int r = 0; r < region; ++r) o += words[r];
  return o;
}
// Typed accessors for a BM x BN tile: static, on the block's address (the kernel's dynamic LDS).
// (A view object holding the address, handed on by reference, compiled the whole-tile kernels to
// 1-3 % more instructions and moved registers in the main loop of kernels that never use it.)
template <int BM_, int BN_>
struct B3NtEpiLds {
  static constexpr int BM = BM_, BN = BN_, LDC = BN + 4;
  template <int R>
  static constexpr int kOff = b3nt_epi_off(BM_, BN_, R);
  static constexpr int kSdWords = kOff<kEpiRed> - kOff<kEpiSd>;
  static_assert(BM == 64 || BM == 128, "segment mask: one or two 64-row words; two list halves");
  template <class T, int R>
  static __device__ __forceinline__ T* at(float* lds) { return (T*)(lds + kOff<R>); }
  static __device__ __forceinline__ float* C(float* lds) { return at<float, kEpiC>(lds); }
  static __device__ __forceinline__ int* sd(float* lds) { return at<int, kEpiSd>(lds); }
  template <int NT>
  static __device__ __forceinline__ float* red(float* lds) {
    static_assert(NT / 64 <= kOff<kEpiMask> - kOff<kEpiRed>, "reduction scratch: a word per wave");
    return at<float, kEpiRed>(lds);
  }
  static __device__ __forceinline__ uint32_t* mask(float* lds) { return at<uint32_t, kEpiMask>(lds); }
  // the mask as seg_first / seg_end take it (handoff.hpp)
  static __device__ __forceinline__ void load_mask(float* lds, uint64_t& mlo, uint64_t& mhi) {
    const uint32_t* m = mask(lds);
    mlo = m[0] | ((uint64_t)m[1] << 32);
    mhi = m[2] | ((uint64_t)m[3] << 32);
  }
  static __device__ __forceinline__ int* late(float* lds) { return at<int, kEpiLate>(lds); }
  static __device__ __forceinline__ int* done(float* lds) { return at<int, kEpiDone>(lds); }
  static __device__ __forceinline__ int* starts(float* lds, int half) {
    return at<int, kEpiStarts>(lds) + 64 * half;
  }
};

// dynamic LDS bytes of a BM x BN NT workgroup (B3NtShape::LDS_BYTES)
constexpr size_t b3nt_lds_bytes(int BM, int BN) {
  const size_t stage = (size_t)3 * (3 * BN * 4) * 16;
  const size_t epi = (size_t)b3nt_epi_off(BM, BN, kEpiEnd) * 4;
  return stage > epi ? stage : epi;
}

template <int WAVES, int RF, int NF>
struct B3NtShape {
  static constexpr int NT = WAVES * 64;
  static constexpr int BM = WAVES * 16 * RF, BN = NF * 16;
  static constexpr int BU4 = 3 * BN * 4;  // b3_u4 per B stage buffer (3 pieces x BN rows x 64 B)
  static constexpr int BPT = (BU4 + NT - 1) / NT;
  using Epi = B3NtEpiLds<BM, BN>;
  static constexpr int LDC = Epi::LDC;
  static constexpr size_t LDS_BYTES = b3nt_lds_bytes(BM, BN);
};

// What a whole-tile functor's tile() gets, BY VALUE (by reference the same kernels grew by 1 %):
// pv[it] = its pre4 of piece tid + NT * it of the tile's BM x BN / 4 float4 pieces (row q / C4,
// column group q % C4; not loaded for an addend functor), its context, the epilogue LDS block
// (layout Lds) and the tile's and the thread's place (tile_id = tm * tiles_n + tn)
template <class S, class EP, int EIT_>
struct B3NtTile {
  using Lds = typename S::Epi;
  static constexpr int BM = S::BM, BN = S::BN, NT = S::NT, LDC = S::LDC, EIT = EIT_;
  const typename EP::Pre (&pv)[EIT_];
  const typename EP::Ctx& cx;
  float* lds;
  int m0, n0, tile_id, tid;
};

// Pipeline (one barrier per k step, 3 LDS buffers for B):
//   iteration ks computes step ks from LDS buffer ks % 3 and A fragments afr[ks & 1], and stages
//   step ks+2's B block (registers -> buffer (ks+2) % 3, which step ks-1 read before the previous
//   barrier) and step ks+1's A fragments (split into afr[(ks+1) & 1]); it also issues the global
//   loads of A(ks+2) and B(ks+3), so every load has a full step to land.
//   A step runs over the column fragments in pairs (b3_mfma6x2): each pair's B fragments come from
//   a ring of registers read from LDS some fragments ahead, and each pair carries its share of
//   the step's loads, LDS stores and the A split between its MFMAs (sched_group_barrier).
//   Staging past the end writes a buffer nobody reads any more (unconditional, branch-free).
//   The last step (the tail) has nothing to stage: its load slots take the epilogue's addend.
//   Epilogue: the three shapes of the file header.
//   ACC (CGR_PRECISION_FP32): per-k-step accumulation.  The matrix core aligns every product of
//   an MFMA to its largest operand, the accumulator included, so the small pieces' products are
//   rounded at the ulp of the running sum.  With ACC a step's six piece products of a fragment go
//   into a zeroed accumulator (aligned to the step's own largest product) and one fp32 add folds
//   the step sum into the running sum.  The default (false) is the code path without it.
template <int WAVES, int RF, int NF, bool NOMASK, class AL, class EP, bool ACC = false>
__global__ __launch_bounds__(WAVES * 64) void gemm_b3nt_kernel(AL al, const b3_u4* __restrict__ Bimg,
                                                               int nimg, EP ep, int M, int N,
                                                               int K, int tiles_n) {
  using S = B3NtShape<WAVES, RF, NF>;
  constexpr int NT = S::NT, BM = S::BM, BN = S::BN, BU4 = S::BU4, BPT = S::BPT;
  extern __shared__ b3_u4 b3_lds[];
  int nwg = gridDim.x;
  if constexpr (b3_ep_side<EP>::value) {
    if (ep.side_on) {
      if (blockIdx.x == gridDim.x - 1) {
        ep.side(b3_lds);
        return;
      }
      --nwg;
    }
  }
  CGR_STAMP_BEGIN();
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fg = lane >> 4;
  const int tile = xcd_remap(blockIdx.x, nwg);
  const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int nk = (K + B3_BK - 1) / B3_BK;
  const int sw = fg ^ lds_swz(fr);  // lds_swz(16 j + fr) == lds_swz(fr)

  // ---- epilogue mapping ----
  constexpr int C4 = BN / 4;
  // the whole tile goes to the functor (EpLayerSeg: ep_fwd.hpp, EpLayerBwdSeg: ep_bwd.hpp)
  constexpr bool TILE = b3_ep_tile<EP>::value;
  constexpr bool ADD = b3_ep_addend<EP>::value;
  // Plain epilogues: one float4 column group per thread (its constants loaded once, in the
  // prologue), rows er0 + RPP * it
  constexpr int RPP = NT / C4;                // rows per pass
  constexpr int EIT = (BM + RPP - 1) / RPP;   // passes
  static_assert(RPP >= 1, "one row group per pass");
  const bool eact = tid < RPP * C4;
  const int ec4 = eact ? tid % C4 : 0, er0 = tid / C4;
  const int ecol = n0 + 4 * ec4;
  // Flat passes: epilogues without per-column constants (the addend forms, whose column terms
  // are already in the accumulators; the whole-tile functors) take item q = tid + NT * it of the
  // tile's BM x C4 float4 pieces, row q / C4, column group q % C4 -- every lane busy in every
  // pass (at BM 128 x 52 groups: 13 passes of 512 instead of 15 passes of 468 lanes)
  constexpr bool FLAT = TILE || ADD;
  constexpr int EITF = (BM * C4 + NT - 1) / NT;
  constexpr int EP_IT = FLAT ? EITF : EIT;
  // issued in the prologue behind the first operand loads, used after the main loop: the column
  // group's constants (bias, ...) and, for the whole-tile functors, this thread's row of the
  // tile's dst-segment structure (handoff.hpp)
  typename EP::Ctx cx;
  int sdv = 0;
  bool sstart = true;  // row tid starts a dst segment in the tile (handoff.hpp seg_*)
  auto epilogue_consts = [&]() {
    if constexpr (ADD)
      cx = ep.ctx_add();  // the column constants travel with the addend
    else
      cx = ep.ctx(ecol);
    if constexpr (TILE) {
      const int r = m0 - 1 + tid;
      const int d = ep.dst_s[min(max(r, 0), M - 1)];
      sdv = (r >= 0 && r < M) ? d : -1 - (r >= M);  // distinct sentinels outside [0, M)
      const int d1 = ep.dst_s[min(r + 1, M - 1)];    // row tid itself
      sstart = tid == 0 || r + 1 >= M || d1 != d;
    }
  };

  // ---- A: RF row fragments per lane, two float4 fetches per fragment per k step ----
  typename AL::Row arow[RF];
#pragma unroll
  for (int i = 0; i < RF; ++i) arow[i] = al.row(m0 + (w * RF + i) * 16 + fr, M);
  typedef typename AL::Raw ARaw[RF][2];
  // unconditional loads: k >= K reads in-bounds element 0 (the loaders clamp), never used
  auto fetchA = [&](ARaw& a, int ks) {
    const int kb = ks * B3_BK + 4 * fg;
#pragma unroll
    for (int i = 0; i < RF; ++i) {
      a[i][0] = al.fetch(arow[i], kb, K);
      a[i][1] = al.fetch(arow[i], kb + 16, K);
    }
  };
  auto splitA = [&](const ARaw& a, b3_u4 (&af)[RF][3], int ks) {
    const int kb = ks * B3_BK + 4 * fg;
#pragma unroll
    for (int i = 0; i < RF; ++i) {
      float4 u, v;
      if constexpr (NOMASK) {
        u = al.combine_nm(a[i][0]);
        v = al.combine_nm(a[i][1]);
      } else {
        u = al.combine(a[i][0], arow[i], kb, K);
        v = al.combine(a[i][1], arow[i], kb + 16, K);
      }
      const float f[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
      b3_split8<3>(f, af[i]);
    }
  };
  // ---- B: the tile's column block of one (ks, piece) plane is BN * 4 contiguous b3_u4 ----
  int boff[BPT], loff[BPT];
#pragma unroll
  for (int p = 0; p < BPT; ++p) {
    const int q = tid + p * NT;
    const int qq = q < BU4 ? q : BU4 - 1;
    const int piece = qq / (BN * 4), rem = qq - piece * (BN * 4);
    boff[p] = (piece * nimg + n0) * 4 + rem;
    loff[p] = q < BU4 ? q : -1;
  }
  typedef b3_u4 BRaw[BPT];
  auto fetchB = [&](BRaw& b, int ks) {  // steps past the end re-read the last plane (unused)
    const b3_u4* src = Bimg + (size_t)(ks < nk ? ks : nk - 1) * 3 * nimg * 4;
#pragma unroll
    for (int p = 0; p < BPT; ++p) b[p] = src[boff[p]];
  };
  auto storeB1 = [&](const BRaw& b, int p, int buf) {
    if (loff[p] >= 0) b3_lds[buf * BU4 + loff[p]] = b[p];
  };
  auto storeB = [&](const BRaw& b, int buf) {
#pragma unroll
    for (int p = 0; p < BPT; ++p)
      if (loff[p] >= 0) b3_lds[buf * BU4 + loff[p]] = b[p];
  };

  floatx4 acc[RF][NF];
#pragma unroll
  for (int i = 0; i < RF; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  // The addend of an addend epilogue, in MFMA layout; the tail step loads it.  The lane
  // coordinates of its loads are recomputed behind an opaque copy of the thread id: shared with
  // the prologue's, they would stay live across the main loop (spills)
  float arow_v[ADD ? RF : 1][ADD ? NF : 1][4];
  float acol_v[ADD ? NF : 1];
  int otid = 0;
  auto add_loads = [&](int j) {
    if constexpr (ADD) {
      const int ofr = otid & 15, ofg = (otid & 63) >> 4, ow = otid >> 6;
      const int col = n0 + j * 16 + ofr;
#pragma unroll
      for (int i = 0; i < RF; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          arow_v[i][j][r] = ep.add_row(m0 + (ow * RF + i) * 16 + ofg * 4 + r, col);
    }
  };

  // read-ahead depth: 4 fragment columns, 2 at 11 (4 spill the gathered-A kernels there)
  constexpr int LDA = NF == 11 ? 2 : (4 < NF ? 4 : NF - 1);
  constexpr int AV = (int)(sizeof(typename AL::Raw) / 16);  // VMEM instructions per A fetch unit
  constexpr int NAS = RF * 2;                               // A fetch units per step
  constexpr int NLS = NAS + BPT;                            // load slots per step
  constexpr int NP = (NF + 1) / 2;                          // MFMA pairs per step
  // One step: the MFMAs of step ks (LDS buffer cb, fragments afc), column groups in pairs, with
  // the step's other work spread over them -- the vector-memory path and the matrix pipe overlap
  // only when loads are interleaved with the MFMAs; issued as one burst per step they stall every
  // wave of the workgroup at once.
  //   A main step (kMain) stages: the global loads of the next raw set (A(ksa) -> ya,
  // B(ksb) -> yb), the LDS stores of the current set's B block (xb -> buffer wb) and the split of
  // its A fragments (xa -> afn, step ksn).
  //   The last step (kTail) has none of it left (the main steps load two steps ahead) and ignores
  // those arguments; for an addend epilogue it loads the addend instead, fragment column j beside
  // the MFMAs of pair j / 2, so its HBM traffic overlaps the matrix work instead of following it.
  // (A two-step tail that also splits A of the last step spilled 16-22 VGPRs on the gathered-A
  // kernels.)
  constexpr std::false_type kMain{};
  constexpr std::true_type kTail{};
  auto step = [&](auto TAILc, int cb, const b3_u4 (&afc)[RF][3], const BRaw& xb, int wb,
                  const ARaw& xa, b3_u4 (&afn)[RF][3], int ksn, ARaw& ya, int ksa, BRaw& yb,
                  int ksb) {
    constexpr bool TAIL = decltype(TAILc)::value;
    const b3_u4* Bs = b3_lds + cb * BU4;
    int kba = 0;
    const b3_u4* bsrc = nullptr;
    if constexpr (!TAIL) {
      kba = ksa * B3_BK + 4 * fg;
      bsrc = Bimg + (size_t)(ksb < nk ? ksb : nk - 1) * 3 * nimg * 4;
    }
    constexpr int RING = LDA + 2;
    b3_u4 bq[RING][3];
    auto rd = [&](int j) {
      const int o = (j * 16 + fr) * 4 + sw;
#pragma unroll
      for (int q = 0; q < 3; ++q)
        bq[j % RING][q] = Bs[q * BN * 4 + o];
    };
#pragma unroll
    for (int j = 0; j < LDA; ++j) rd(j);
    // the read-ahead is issued here, ahead of everything (else the scheduler fills each pair's
    // ds_read group with that pair's own reads and waits on them right away)
    __builtin_amdgcn_sched_barrier(0);
    // ACC: the previous pair's step sums; their adds are issued behind this pair's MFMAs, so
    // only two pairs' step sums are live
    floatx4 carx[ACC ? RF : 1], cary[ACC ? RF : 1];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int j = 2 * p;
      const bool two = j + 1 < NF;
      int nrd = 0;
      if (j + LDA < NF) {
        rd(j + LDA);
        nrd += 3;
      }
      if (two && j + 1 + LDA < NF) {
        rd(j + 1 + LDA);
        nrd += 3;
      }
      if constexpr (ACC) {
#pragma unroll
        for (int i = 0; i < RF; ++i) {
          floatx4 x = floatx4{0.f, 0.f, 0.f, 0.f}, y = x;
          b3_mfma6x2(afc[i], bq[j % RING], bq[(j + 1) % RING], two, x, y);
          if (p > 0) {
            acc[i][j - 2] += carx[i];
            acc[i][j - 1] += cary[i];  // every pair but the last has two columns
          }
          carx[i] = x;
          cary[i] = y;
        }
      } else {
#pragma unroll
        for (int i = 0; i < RF; ++i)
          b3_mfma6x2(afc[i], bq[j % RING], bq[(j + 1) % RING], two, acc[i][j],
                     acc[i][two ? j + 1 : j]);
      }
      constexpr int MQ = 4 * RF;  // a third of a pair's MFMAs
      if constexpr (!TAIL) {
        // this pair's share of the load slots and of the B stores
        int nvm = 0, nst = 0;
        const int s0 = p * NLS / NP, s1 = (p + 1) * NLS / NP;
#pragma unroll
        for (int s = 0; s < NLS; ++s)
          if (s >= s0 && s < s1) {
            if (s < NAS)
              ya[s >> 1][s & 1] = al.fetch(arow[s >> 1], kba + 16 * (s & 1), K);
            else
              yb[s - NAS] = bsrc[boff[s - NAS]];
            nvm += s < NAS ? AV : 1;
          }
        const int w0 = p * BPT / NP, w1 = (p + 1) * BPT / NP;
#pragma unroll
        for (int q = 0; q < BPT; ++q)
          if (q >= w0 && q < w1) {
            storeB1(xb, q, wb);
            ++nst;
          }
        if (p == NP / 2) splitA(xa, afn, ksn);
        b3_sgb<0x100>(nrd);                                    // ds_read
        if (two) b3_sgb<0x008>(MQ); else b3_sgb<0x008>(MQ / 2);  // MFMA
        b3_sgb<0x020>(nvm);                                    // global load
        if (two) b3_sgb<0x008>(MQ); else b3_sgb<0x008>(MQ / 2);
        b3_sgb<0x200>(nst);                                    // ds_write
        b3_sgb<0x008>(MQ);
      } else {
        int nvm = 0;
        if constexpr (ADD) {
          add_loads(j);
          if (two) add_loads(j + 1);
          nvm = (two ? 2 : 1) * 4 * RF;
        }
        b3_sgb<0x100>(nrd);
        if (two) b3_sgb<0x008>(MQ); else b3_sgb<0x008>(MQ / 2);
        b3_sgb<0x020>(nvm);
        if (two) b3_sgb<0x008>(2 * MQ); else b3_sgb<0x008>(MQ + MQ / 2);
      }
    }
    if constexpr (ACC) {  // the last pair's step sums
      constexpr int jl = 2 * (NP - 1);
#pragma unroll
      for (int i = 0; i < RF; ++i) {
        acc[i][jl] += carx[i];
        if constexpr (jl + 1 < NF) acc[i][jl + 1] += cary[i];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
  };

  {  // prologue: buffers 0, 1 <- B(0), B(1); afr0 <- A(0); raw set 0 <- A(1), B(2)
    ARaw a0, xa0, xa1;
    BRaw b0, b1, xb0, xb1;
    fetchA(a0, 0);
    fetchB(b0, 0);
    fetchB(b1, 1);
    fetchA(xa0, 1);
    fetchB(xb0, 2);
    b3_u4 afr0[RF][3], afr1[RF][3];
    storeB(b0, 0);
    storeB(b1, 1);
    splitA(a0, afr0, 0);
    __syncthreads();
    CGR_STAMP(1);
    epilogue_consts();  // after the prologue barrier: not waited for by it
    int cb = 0;  // LDS buffer of step ks (ks % 3)
    const int nmain = nk - 1;  // steps before the tail (the last step)
    for (int ks = 0; ks < nmain; ks += 2) {
      // even step: consume set 0 (A(ks+1), B(ks+2)), fill set 1 with A(ks+2), B(ks+3)
      step(kMain, cb, afr0, xb0, cb == 0 ? 2 : cb - 1, xa0, afr1, ks + 1, xa1, ks + 2, xb1, ks + 3);
      cb = cb == 2 ? 0 : cb + 1;
      if (ks + 1 >= nmain) break;
      // odd step: consume set 1 (A(ks+2), B(ks+3)), fill set 0 with A(ks+3), B(ks+4)
      step(kMain, cb, afr1, xb1, cb == 0 ? 2 : cb - 1, xa1, afr0, ks + 2, xa0, ks + 3, xb0, ks + 4);
      cb = cb == 2 ? 0 : cb + 1;
    }
    // tail: the last step uses fragment set nmain % 2 (split by the step before), moved into set
    // 0 so that the tail is one piece of code
    if (nmain & 1) {
#pragma unroll
      for (int i = 0; i < RF; ++i)
#pragma unroll
        for (int q = 0; q < 3; ++q) afr0[i][q] = afr1[i][q];
    }
    if constexpr (ADD) asm volatile("v_mov_b32 %0, %1" : "=v"(otid) : "v"(tid));
    step(kTail, cb, afr0, xb0, 0, xa0, afr1, 0, xa1, 0, xb1, 0);  // stages nothing: sets unused
  }

  CGR_STAMP(2);
  // ---- epilogue (the stage buffers are dead after the last barrier) ----
  ep.finish_ctx(cx);
  if constexpr (ADD) {  // the addend into the accumulators (the operation order of the apply)
#pragma unroll
    for (int j = 0; j < NF; ++j) acol_v[j] = ep.add_col(n0 + j * 16 + fr);  // L2-resident
#pragma unroll
    for (int i = 0; i < RF; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[i][j][r] = ep.add_apply(acc[i][j][r], arow_v[i][j][r], acol_v[j], cx);
  }
  typename EP::Pre pv[EP_IT];
  if constexpr (!ADD) {
#pragma unroll
    for (int it = 0; it < EP_IT; ++it) {
      if constexpr (TILE) {
        const int q = min(tid + NT * it, BM * C4 - 1);
        const int r = q / C4;
        pv[it] = ep.pre4(m0 + r, n0 + 4 * (q - r * C4));
      } else {
        pv[it] = ep.pre4(m0 + min(er0 + RPP * it, BM - 1), ecol);
      }
    }
  }
  float* const lds = reinterpret_cast<float*>(b3_lds);
  float* C = S::Epi::C(lds);
  if constexpr (TILE) {  // the tile's segment structure (in a helper this costs 9 kernels VGPRs)
    using L = typename S::Epi;
    static_assert(NT >= L::kSdWords, "sd: one dst per thread");
    uint32_t* smask = L::mask(lds);
    if (tid < L::kSdWords) L::sd(lds)[tid] = sdv;
    if (tid < BM) {
      const uint64_t b = __ballot(sstart);
      if ((tid & 63) == 0) {
        smask[2 * (tid >> 6)] = (uint32_t)b;
        smask[2 * (tid >> 6) + 1] = (uint32_t)(b >> 32);
      }
      if constexpr (b3_ep_starts<EP>::value) {
        // the start rows of this wave's 64 rows (below the tile's row count), in order, into half
        // tid / 64 of the start list (the halves' counts come from the mask)
        const bool real = sstart && tid < M - m0;
        const uint64_t rb = __ballot(real);
        if (real) L::starts(lds, tid >> 6)[__popcll(rb & ((1ull << (tid & 63)) - 1))] = tid;
      }
    }
    if (BM == 64 && tid == 0) smask[2] = smask[3] = 0xffffffffu;  // rows 64.. (none): starts
  }
#pragma unroll
  for (int i = 0; i < RF; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        C[((w * RF + i) * 16 + fg * 4 + r) * S::LDC + j * 16 + fr] = acc[i][j][r];
  __syncthreads();
  CGR_STAMP(3);
  if constexpr (TILE) {
    ep.tile(B3NtTile<S, EP, EP_IT>{pv, cx, lds, m0, n0, tile, tid});
  } else {
    auto apply_pass = [&](auto Ac) {
      if constexpr (ADD) {  // flat
#pragma unroll
        for (int it = 0; it < EP_IT; ++it) {
          const int q = tid + NT * it;
          if (q >= BM * C4) break;
          const int r = q / C4, c4 = q - r * C4, col = n0 + 4 * c4;
          const float4* cp = reinterpret_cast<const float4*>(&C[r * S::LDC + 4 * c4]);
          ep.template apply4z<decltype(Ac)::value>(m0 + r, col, *cp, cx);
        }
      } else {  // this thread's column group
#pragma unroll
        for (int it = 0; it < EIT; ++it) {
          const int r = er0 + RPP * it;
          if (eact && r < BM) {
            const float4* cp = reinterpret_cast<const float4*>(&C[r * S::LDC + 4 * ec4]);
            ep.apply4p(m0 + r, ecol, *cp, pv[it], cx);
          }
        }
      }
    };
    if constexpr (b3_ep_act<EP>::value) {  // one loop per activation, chosen once
      if (ep.act == ACT_RELU) apply_pass(std::integral_constant<int, ACT_RELU>{});
      else if (ep.act == ACT_SILU) apply_pass(std::integral_constant<int, ACT_SILU>{});
      else apply_pass(std::integral_constant<int, -1>{});  // GELU and the rest
    } else {
      apply_pass(std::integral_constant<int, -1>{});
    }
    CGR_STAMP(4);
  }
  // stamp_lab.py's tag bits: 1 = the forward's whole-tile functor (the one with a start list),
  // 2 = the backward's
  CGR_STAMP_END((TILE && !b3_ep_starts<EP>::value ? 2 : 0) | (b3_ep_starts<EP>::value ? 1 : 0) |
                (NF << 2) | (WAVES << 7));
}

template <int WAVES, int RF, int NF, bool NOMASK, bool ACC = false, class AL, class EP>
inline hipError_t launch_b3nt_t(const AL& al, const b3_u4* Bimg, int nimg, const EP& ep, int M,
                                int N, int K, int tiles_n, hipStream_t st) {
  using S = B3NtShape<WAVES, RF, NF>;
  auto kern = gemm_b3nt_kernel<WAVES, RF, NF, NOMASK, AL, EP, ACC>;
  static LdsLimit lim;
  // the dynamic bytes this launch asks for (a diagnostic build adds static LDS: stamps.hpp)
  const hipError_t e = lim.ensure(reinterpret_cast<const void*>(kern), (int)S::LDS_BYTES);
  if (e != hipSuccess) return e;
  const int tm = (M + S::BM - 1) / S::BM;
  int side = 0;
  if constexpr (b3_ep_side<EP>::value) {
    side = ep.side_on ? 1 : 0;
    // the caller checked b3nt_side_fits; a side workgroup needing more LDS than the tile is a bug
    if (side && ep.side_lds_bytes() > S::LDS_BYTES) return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(kern, dim3(tm * tiles_n + side), dim3(WAVES * 64), S::LDS_BYTES, st, al, Bimg,
                     nimg, ep, M, N, K, tiles_n);
  return hipGetLastError();
}

// workgroup rows: 8 waves (128 rows) when that still gives ~100+ workgroups (the node-row readout
// GEMMs at 120 x 8 waves beat 240 x 4 waves at one wave per SIMD: step A/B +0.8 %), else 4 (64 rows)
inline int b3nt_waves(int M, int N) {
  const int tiles_n = b3_cols(N).tiles;
  return ((M + 127) / 128) * tiles_n >= 96 ? 8 : 4;
}

// rows per workgroup tile of launch_b3nt for an M x N GEMM
inline int b3nt_rows(int M, int N) { return b3nt_waves(M, N) == 8 ? 128 : 64; }

// Column tiling of an M-row NT GEMM whose workgroups would leave CUs idle in b3_cols(N)'s tiling
// (the node-row readout GEMMs of a small batch: 60 row tiles x 2 at cfg2): more, narrower column
// tiles, chosen by a cost model of waves of workgroups x per-k-step cost, a step costing its
// MFMAs (nf fragment columns) plus fixed work worth kB3StepFixed columns (A fetch + split, B
// staging, the barrier: cfg2 layer GEMMs run 1.9 us per 13-column step against 1.3 us of MFMA).
// Every A row is then loaded and split once per column tile (more A traffic, all L2 hits).
// Images are packed in the tiling they are launched with (b3_job(..., cols)).
constexpr int kB3Cus = 256;
constexpr int kB3StepFixed = 6;
inline B3Cols b3nt_cols(int M, int N, bool acc = false) {
  const B3Cols c0 = b3_cols(N, acc);
  const int bm = b3nt_rows(M, N);
  const int tm = (M + bm - 1) / bm;
  const int nft = (N + 15) / 16;
  auto cost = [&](const B3Cols& c) {
    const int waves = (tm * c.tiles + kB3Cus - 1) / kB3Cus;
    return waves * (kB3StepFixed + c.nf);
  };
  B3Cols best = c0;
  int bc = cost(c0);
  for (int nf = c0.nf - 1; nf >= 2; --nf) {
    if (b3_nf_snap(nf, acc) != nf) continue;
    const int tiles = (nft + nf - 1) / nf;
    const B3Cols c{tiles, nf, tiles * nf * 16};
    const int k = cost(c);
    if (k < bc) best = c, bc = k;
  }
  return best;
}

// whether launch_b3nt(.., c, .., M, N, ..) can host a side workgroup of lds bytes on a CU no tile
// takes (one NT workgroup per CU: kB3Cus - 1 tiles at most)
inline bool b3nt_side_fits(int M, int N, const B3Cols& c, size_t lds) {
  const int bm = b3nt_rows(M, N);
  return (int64_t)((M + bm - 1) / bm) * c.tiles < kB3Cus && lds <= b3nt_lds_bytes(bm, c.nf * 16);
}

// C = A B^T with B given as its image (b3_pack of the same N, K in the column tiling c).
// M, N, K > 0.  acc: the per-k-step accumulation variant (c from b3_cols / b3nt_cols(.., true)).
template <class AL, class EP>
inline hipError_t launch_b3nt(const AL& al, const b3_u4* Bimg, const B3Cols& c, const EP& ep,
                              int M, int N, int K, hipStream_t st, bool acc = false) {
  if (M <= 0 || N <= 0) return hipSuccess;
  if (c.tiles * c.nf * 16 != c.nimg || c.nimg < N || b3_nf_snap(c.nf, acc) != c.nf)
    return hipErrorInvalidValue;
  const bool w8 = b3nt_waves(M, N) == 8;
  // unmasked A when K % 4 == 0: every fetched float4 is either all-valid or past K (clamped to
  // finite in-bounds data, multiplied by the image's zero rows)
  auto go = [&](auto NFc) -> hipError_t {
    constexpr int NF = decltype(NFc)::value;
    if (acc) {
      if constexpr (NF <= kB3AccMaxNf) {
        if (K % 4 == 0)
          return w8 ? launch_b3nt_t<8, 1, NF, true, true>(al, Bimg, c.nimg, ep, M, N, K, c.tiles, st)
                    : launch_b3nt_t<4, 1, NF, true, true>(al, Bimg, c.nimg, ep, M, N, K, c.tiles, st);
        return w8 ? launch_b3nt_t<8, 1, NF, false, true>(al, Bimg, c.nimg, ep, M, N, K, c.tiles, st)
                  : launch_b3nt_t<4, 1, NF, false, true>(al, Bimg, c.nimg, ep, M, N, K, c.tiles, st);
      }
      return hipErrorInvalidValue;
    }
    if (K % 4 == 0)
      return w8 ? launch_b3nt_t<8, 1, NF, true>(al, Bimg, c.nimg, ep, M, N, K, c.tiles, st)
                : launch_b3nt_t<4, 1, NF, true>(al, Bimg, c.nimg, ep, M, N, K, c.tiles, st);
    return w8 ? launch_b3nt_t<8, 1, NF, false>(al, Bimg, c.nimg, ep, M, N, K, c.tiles, st)
              : launch_b3nt_t<4, 1, NF, false>(al, Bimg, c.nimg, ep, M, N, K, c.tiles, st);
  };
  switch (c.nf) {
    case 1: return go(std::integral_constant<int, 1>{});
    case 2: return go(std::integral_constant<int, 2>{});
    case 3: return go(std::integral_constant<int, 3>{});
    case 4: return go(std::integral_constant<int, 4>{});
    case 6: return go(std::integral_constant<int, 6>{});
    case 7: return go(std::integral_constant<int, 7>{});
    case 8: return go(std::integral_constant<int, 8>{});
    case 11: return go(std::integral_constant<int, 11>{});
    case 13: return go(std::integral_constant<int, 13>{});
  }
  return hipErrorInvalidValue;
}
// ... in b3_cols(N)'s tiling
template <class AL, class EP>
inline hipError_t launch_b3nt(const AL& al, const b3_u4* Bimg, const EP& ep, int M, int N, int K,
                              hipStream_t st) {
  return launch_b3nt(al, Bimg, b3_cols(N), ep, M, N, K, st);
}

}  // namespace cgr
