// SFA channel/spatial attention stage as ONE operator (forward and backward), for gfx950.
//
// Reference: models/necks/mix.py:8-59 (channel_spatial_stage).  With x = cat[x_bev, x_voxel]:
//   s   = mean_hw(x)                         a = sigmoid(fc(s))                     (mix.py:41-44)
//   u   = a*x_bev + (1-a)*x_voxel                                                    (mix.py:46-50)
//   y1  = conv1(u)   z1 = relu(bn1(y1))   y2 = conv2(z1)   s2 = bn2(y2)              (mix.py:51)
//   out = sigmoid(s2)*(a*x_bev) + (1-sigmoid(s2))*((1-a)*x_voxel)                    (mix.py:52-58)
//
// The two 1x1 convolutions are (C x C) x (C x B*HW) GEMMs on NCHW data (six of them per forward + backward).  They run on the
// matrix cores with everything element-wise FUSED into the operand path, so no intermediate but y1 and y2 is ever stored.
// Precision per call (dhd_sfa_weights.gemm / storage_dtype, include/dhd_amd.h): bf16x3 (default), bf16x6, f32, or half storage.
// make_plan (host side, below) states which kernel family serves each precision and channel count.
// This file: the small dense pieces (channel mean -> fc -> a), BatchNorm statistics and coefficient tables, the fused blends,
// pw_wgrad3 + the deterministic partial reduction, and the host side of the operator for every storage type.
// Common structure of the GEMMs:
//   * forward / dgrad: the activation operand passes through a per-(sample,channel) affine prologue act(c0*in0 + c1*in1 + c2)
//     -- which is blend1 (in0,in1 = x_bev,x_voxel), BatchNorm+ReLU (in0 = y1) or BatchNorm-backward (in0,in1 = g,y); epilogue:
//     bias + BatchNorm batch statistics (forward), the ReLU mask from the pass bits the forward recorded (dgrad 2), whole-line
//     16-byte stores along the pixel axis (store_b128_guarded, sfa_mfma.h);
//   * weight gradient: pixels are the reduction dimension; per-worker partial matrices reduced by a second small kernel
//     (deterministic, no float atomics);
//   * BatchNorm gradient sums are per-plane streaming reductions with double-precision finalisation; the blends are fused with
//     the BatchNorm affine and the sigmoid.
// Forward reads x three times and y1/y2 twice; nothing is transposed, there is no NHWC detour.
// Backward, bf16x3 at C = 128 / 256 on float32 storage without cross-rank statistics (DHD_SFA_BWD_FOLD = 15, the default; T = one
// (B,C,H,W) tensor).  Both GEMMs of a layer apply the same BatchNorm-backward prologue gy = c0 g + c1 y + c2, and each layer runs
// them in ONE launch on pairs of CUs: gy is staged once per CU and never stored.  Layer 2 (sfa_gemm_pair.h) sums g1 where it is
// made; layer 1 (sfa_gemm_pair1.h) blends x into the weight gradient's operand, sums du (x_bev - x_voxel) where du is made and
// leaves g1 alone:
//   launch                          reads                          writes
//   blend2_bn_bwd                   x (2T), y2, gout               g2; BatchNorm-2 sums, go-part of dL/da
//   pw_pair (dgrad 2 + dW2)         g2, y2, y1                     g1; partials; sum g1, sum g1 (y1 - mu1) per pair-worker
//   wgrad_reduce, bn_backward_rows  partials, worker rows          dW2; BatchNorm-1 backward table, dgamma1, dbeta1
//   pw_pair1 (dgrad 1 + dW1)        g1, y1, x (2T)                 du; partials; sum du (x_bev - x_voxel) per (pair-worker, sample)
//   wgrad_reduce, fc_backward       partials, worker rows          dW1; dL/d(fc)
//   stage_gx                        y2, gout, du                   gx (2T)
// 14T of reads and 5T of writes (what the pairs' second CU reads again is not counted: it is the same tile at the same time).
// DHD_SFA_BWD_FOLD = 7 FOLDS layer 1 in two launches instead: the data gradient runs first and stores gy over g, the weight gradient
// reads that one tensor, and the load stream this frees carries the tensor a reduction pass of its own used to re-read:
//   pw_gemm_cu EPI 2, WB (dgrad 1)  g1, y1                         du, gy1 over g1
//   pw_wgrad3 FOLD 2 (dW1)          gy1, x (2T), du                partials; sum du (x_bev - x_voxel) per (worker, sample)
// 16T of reads and 6T of writes.  DHD_SFA_BWD_FOLD = 3 folds layer 2 as well:
//   pw_gemm_cu EPI 1, WB (dgrad 2)  g2, y2, pass bits              g1, gy2 over g2
//   pw_wgrad3 FOLD 1 (dW2)          gy2, y1, g1                    partials; sum g1, sum g1 (y1 - mu1) per worker
// 18T of reads and 7T of writes.  The unfolded flow (every other plan, the phase entry points, DHD_SFA_BWD_FOLD = 0) runs each
// weight gradient before its data gradient on the pair (g, y) and makes the sums in pair_sums (g1, y1) and blend1_da (x, du):
// 23T of reads, 5T of writes.
// Forward-only inference (dhd_sfa_stage_infer, running statistics, nothing kept for a backward): stage_infer below -- the forward's
// own launches, conv2 with BatchNorm-2 + sigmoid + blend in its epilogue (x three times, y1 twice), or under half storage both
// convolutions per pixel tile (sfa_half.h: sfa_onepass_h_kernel; x twice).
#include <stdlib.h>

#include <type_traits>

#include "sfa_gemm_cu.h"   // pw_gemm_cu: bf16x3 at C = 128 / 256; brings sfa_math.h (the stage's scalar expressions) and vec16.h
#include "sfa_gemm_pair.h" // pw_pair: data + weight gradient of conv2 on pairs of CUs
#include "sfa_gemm_pair1.h" // pw_pair1: the same for conv1, with the blend prologue and the dL/da sums
#include "sfa_half.h"      // pw_gemm_cuh / pw_wgrad_h / sfa_onepass_h: the GEMMs of half storage
#include "sfa_mfma.h"

using namespace dhd_sfa;

namespace {

constexpr int kEwBlock = 256;     // element-wise / reduction kernels
constexpr int kPlaneChunks = 4;   // blocks per (b, c) plane
constexpr int kPwBlock = 256;     // pw_gemm: 4 waves
constexpr int kPwStep = 16;       // input channels per weight image / pipeline step
constexpr int kWgBlock = 512;     // pw_wgrad: 8 waves
constexpr int kWgStride = 33;     // LDS row stride of a 32-pixel operand row (conflict-free column reads)
constexpr int kWgWorkers = 256;   // total pw_wgrad blocks (one per CU)
// The weight gradients' split of n steps (32 pixels each, sample after sample) over W workers, in ONE place for the kernel that
// works by it (pw_wgrad3_kernel) and the kernel that reads per-(worker, sample) rows back (fc_backward_kernel): worker w owns the
// steps [wg_first_step(n, w, W), wg_first_step(n, w + 1, W)), so step s belongs to worker wg_owner(n, s, W).
__host__ __device__ inline long long wg_first_step(long long n, long long w, long long W) { return n * w / W; }
__host__ __device__ inline int wg_owner(long long n, long long s, long long W) { return (int)(((s + 1) * W + n - 1) / n) - 1; }
struct WgFirstStep {   // the same partition for pw_pair_kernel (sfa_gemm_pair.h), whose workers are pairs of workgroups
  __host__ __device__ long long operator()(long long n, long long w, long long W) const { return wg_first_step(n, w, W); }
};
// operand blocks and workers per block of a weight-gradient launch (launch_wgrad) at c channels
inline int wgrad_blocks(int c) { const int ot = c == 128 ? 128 : 256; return (c / ot) * (c / ot); }
inline int wgrad_workers(int c) { const int nob = wgrad_blocks(c); return kWgWorkers / nob > 0 ? kWgWorkers / nob : 1; }
constexpr int kBwdFoldDefault = 15;  // DHD_SFA_BWD_FOLD when the environment does not say (bwd_fold_mode)

__device__ __forceinline__ float block_sum(float v, float* sm) {
  v = group_sum(v, DHD_WAVE);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sm[wv] = v;
  __syncthreads();
  float t = 0.f;
  for (int k = 0; k < (int)(blockDim.x / DHD_WAVE); ++k) t += sm[k];
  return t;
}

// ------------------------------------------------------------------------------------------------
// element-wise passes: one kernel per pass for every storage type TS (float, _Float16, __bf16)
// ------------------------------------------------------------------------------------------------
// A lane handles N = kVec16<TS> consecutive elements per vector: 16 bytes of the storage tensors (x, y1, y2, g2, g1, du), the
// same N elements of the I/O tensors (out, gout, gx; IoVec below).  float32 arithmetic, sfa_math.h's expressions.
//
// The storage types differ in THREE respects and nowhere else.  Each was a measured choice for its type; changing one is a
// performance change with a measurement of its own.
template <class TS> constexpr bool kHalfStorage = !std::is_same_v<TS, float>;
// 1. Cache policy.  Half storage streams every tensor non-temporally.  float32 storage leaves five accesses plain: the read of
//    y2 in blend2_bn and blend2_bn_bwd, the read of du in blend1_da, the store of g2, and both reads of pair_sums' tail iteration
//    (its main loop is non-temporal: 62 -> 52 us); everything else is non-temporal there too.
template <class TS> constexpr bool kStreamAll = kHalfStorage<TS>;
// 2. Vectors in flight per thread and stream in blend2_bn_bwd and stage_gx: two under half storage, one under float32 storage.
//    (plane_mean and pair_sums keep two, blend2_bn and blend1_da one, whatever the type.)
template <class TS> constexpr int kWideInFlight = kHalfStorage<TS> ? 2 : 1;
// 3. In-lane fold of the reductions in pair_sums and blend1_da: float32 storage sums a vector pairwise, (a+b)+(c+d), with plain
//    multiplies; half storage runs an fmaf chain over its eight elements (fold_sum, fold_dot below).
template <class TS> constexpr bool kFoldPairwise = !kHalfStorage<TS>;

// [lo, hi) in N-element vectors of this block's share of a plane of hw elements (hw % N == 0).
template <int N> __device__ __forceinline__ void chunk_range(int hw, int* lo, int* hi) {
  static_assert(N == 4 || N == 8, "16 bytes of float32 or of a half type");
  const int n = hw >> (N == 8 ? 3 : 2), per = (n + kPlaneChunks - 1) / kPlaneChunks;
  *lo = blockIdx.x * per;
  *hi = min(n, *lo + per);
}

// Vector i of N consecutive elements of an I/O tensor (dhd_sfa_weights.io_dtype) as float32, non-temporal: 16 bytes when the
// element is as wide as the storage type's, 8 bytes of a half type beside float32 storage (N = 4).  Widened exactly / rounded
// to nearest even; the 8-byte store converts element by element (vec16.h: the pairwise form is another instruction order).
template <class TO, int N> struct IoVec {
  static constexpr bool k16 = N == kVec16<TO>;
  static_assert(k16 || (N == 4 && sizeof(TO) == 2), "16 bytes, or four elements of a half type");
  using raw = std::conditional_t<k16, raw16<TO>, u32x2>;
  static __device__ __forceinline__ raw ld(const TO* base, size_t i) { return __builtin_nontemporal_load(reinterpret_cast<const raw*>(base) + i); }
  static __device__ __forceinline__ void widen(raw w, float* v) {
    if constexpr (k16) {
      widen16<TO>(w, v);
    } else {
      const f32x2 a = Pair<TO>::widen(w.x), b = Pair<TO>::widen(w.y);
      v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    }
  }
  static __device__ __forceinline__ void store(TO* base, size_t i, const float* v) {
    if constexpr (k16) {
      Vec16<TO, true>::store(base, i, v);
    } else {
      typedef TO t4 __attribute__((ext_vector_type(4)));
      const t4 h = {(TO)v[0], (TO)v[1], (TO)v[2], (TO)v[3]};
      __builtin_nontemporal_store(h, reinterpret_cast<t4*>(base) + i);
    }
  }
};

// sum of a vector's elements as a pairwise tree: (v0+v1)+(v2+v3), and for eight ((v0+v1)+(v2+v3))+((v4+v5)+(v6+v7))
template <int N> __device__ __forceinline__ float tree_sum(const float* v) {
  if constexpr (N == 4) return (v[0] + v[1]) + (v[2] + v[3]);
  else return tree_sum<N / 2>(v) + tree_sum<N / 2>(v + N / 2);
}

// acc + sum_j a[j]  and  acc + sum_j a[j]*d(j)  over one vector, in the storage type's order (kFoldPairwise)
template <class TS> __device__ __forceinline__ float fold_sum(float acc, const float* a) {
  if constexpr (kFoldPairwise<TS>) return acc + tree_sum<kVec16<TS>>(a);
#pragma unroll
  for (int j = 0; j < kVec16<TS>; ++j) acc += a[j];
  return acc;
}
template <class TS, class D> __device__ __forceinline__ float fold_dot(float acc, const float* a, D d) {
  if constexpr (kFoldPairwise<TS>) {
    static_assert(kVec16<TS> == 4, "the pairwise fold is written for four elements");
    return acc + ((a[0] * d(0) + a[1] * d(1)) + (a[2] * d(2) + a[3] * d(3)));
  }
#pragma unroll
  for (int j = 0; j < kVec16<TS>; ++j) acc = fmaf(a[j], d(j), acc);
  return acc;
}

// A thread's vectors lo + threadIdx.x, + kEwBlock, ... below hi: body(load(i), i) for each, with the loads of K (1 or 2) vectors
// requested before the first of them is used.
template <int K, class Load, class Body> __device__ __forceinline__ void for_each_vector(int lo, int hi, Load load, Body body) {
  int i = lo + threadIdx.x;
  if constexpr (K == 2) {
    for (; i + kEwBlock < hi; i += 2 * kEwBlock) {
      const auto u = load(i), w = load(i + kEwBlock);
      body(u, i);
      body(w, i + kEwBlock);
    }
    if (i < hi) body(load(i), i);
  } else {
    for (; i < hi; i += kEwBlock) body(load(i), i);
  }
}

// ------------------------------------------------------------------------------------------------
// small dense pieces: channel mean -> fc -> a, and its backward
// ------------------------------------------------------------------------------------------------

// channel means of x: a block's share of plane blockIdx.y
template <class TS>
__device__ __forceinline__ void plane_mean_block(const TS* __restrict__ x, float* __restrict__ part, int hw, float* sm) {
  constexpr int N = kVec16<TS>;
  using X = Vec16<TS, true>;
  const size_t plane = blockIdx.y;
  const TS* p = x + plane * hw;
  int lo, hi;
  chunk_range<N>(hw, &lo, &hi);
  float a0 = 0.f, a1 = 0.f;
  int i = lo + threadIdx.x;
  for (; i + kEwBlock < hi; i += 2 * kEwBlock) {
    float v[N], w[N];
    X::load(p, i, v);
    X::load(p, (size_t)i + kEwBlock, w);
    a0 += tree_sum<N>(v);
    a1 += tree_sum<N>(w);
  }
  if (i < hi) {
    float v[N];
    X::load(p, i, v);
    a0 += tree_sum<N>(v);
  }
  const float tot = block_sum(a0 + a1, sm);
  if (threadIdx.x == 0) part[plane * kPlaneChunks + blockIdx.x] = tot;
}

// the mean-only launch of the plans that pack their weight images in launches of their own (streamed / f32: float32 storage)
__global__ __launch_bounds__(kEwBlock) void plane_mean_kernel(const float* __restrict__ x, float* __restrict__ part, int hw) {
  __shared__ float sm[kEwBlock / DHD_WAVE];
  plane_mean_block(x, part, hw, sm);
}

// one block per sample: s = mean, h = relu(fc1 s), a = sigmoid(fc2 h); blend table (a, 1-a, 0).  The kernel is a
// chain of dependent L2 round trips on the stage's critical path, so each phase puts all its loads in flight at
// once: 16 waves x 4 rows of fc1 per pass, 16-byte loads of the fc2 rows.  (Round 3, tried: both weight matrices requested
// into registers before the first barrier -- 96 more registers in a 1024-thread block: 15.9 -> 20.5 us, reverted.)
constexpr int kFcBlock = 1024;
__global__ __launch_bounds__(kFcBlock) void fc_forward_kernel(const float* __restrict__ part, const float* __restrict__ w1,
                                                              const float* __restrict__ b1, const float* __restrict__ w2,
                                                              const float* __restrict__ b2, float* __restrict__ s,
                                                              float* __restrict__ hbuf, float* __restrict__ a,
                                                              float* __restrict__ tab, int c, int r, int hw,
                                                              int* __restrict__ ticks, int n_ticks) {
  extern __shared__ float sh[];  // s (2c) | h (r)
  if (blockIdx.x == 0)           // the arrival counters of this call's later kernels (SavedLayout::tick)
    for (int i = threadIdx.x; i < n_ticks; i += kFcBlock) ticks[i] = 0;
  float* ss = sh;
  float* hh = sh + 2 * c;
  const int b = blockIdx.x, c2 = 2 * c;
  for (int i = threadIdx.x; i < c2; i += kFcBlock) {
    const float* q = part + ((size_t)b * c2 + i) * kPlaneChunks;
    float v = ((q[0] + q[1]) + (q[2] + q[3])) / (float)hw;
    ss[i] = v;
    s[(size_t)b * c2 + i] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // four rows per wave and pass so that their loads are in flight together
  for (int j0 = wv * 4; j0 < r; j0 += 4 * (kFcBlock / DHD_WAVE)) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = lane; i < c2; i += DHD_WAVE) {
      const float sv = ss[i];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (j0 + q < r) acc[q] = fmaf(w1[(size_t)(j0 + q) * c2 + i], sv, acc[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float t = group_sum(acc[q], DHD_WAVE);
      if (lane == 0 && j0 + q < r) {
        const float v = fmaxf(t + b1[j0 + q], 0.f);
        hh[j0 + q] = v;
        hbuf[(size_t)b * r + j0 + q] = v;
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < c; k += kFcBlock) {
    float acc = b2[k];
    if ((r & 3) == 0) {
      const f32x4* wrow = reinterpret_cast<const f32x4*>(w2 + (size_t)k * r);
#pragma unroll 8
      for (int j = 0; j < (r >> 2); ++j) {
        const f32x4 wv4 = wrow[j];
        acc = fmaf(wv4.x, hh[4 * j], acc);
        acc = fmaf(wv4.y, hh[4 * j + 1], acc);
        acc = fmaf(wv4.z, hh[4 * j + 2], acc);
        acc = fmaf(wv4.w, hh[4 * j + 3], acc);
      }
    } else {
      for (int j = 0; j < r; ++j) acc = fmaf(w2[(size_t)k * r + j], hh[j], acc);
    }
    float v = sigmoidf_(acc);
    a[(size_t)b * c + k] = v;
    float* t = tab + (size_t)b * 3 * c;
    t[k] = v;
    t[c + k] = 1.0f - v;
    t[2 * c + k] = 0.f;
  }
}

// one block per sample: da (from the two partial sets) -> dpre2, dh, ds
__global__ __launch_bounds__(kEwBlock) void fc_backward_kernel(const float* __restrict__ da_p1, const float* __restrict__ da_p2,
                                                               const float* __restrict__ a, const float* __restrict__ hbuf,
                                                               const float* __restrict__ w1, const float* __restrict__ w2,
                                                               float* __restrict__ dpre2, float* __restrict__ dh,
                                                               float* __restrict__ ds, int c, int r, int fold_workers, int sps) {
  extern __shared__ float sh[];  // dpre2 (c) | dh (r) | partials (kEwBlock)
  float* sp = sh;
  float* sd = sh + c;
  const int b = blockIdx.x, c2 = 2 * c;
  // fold_workers > 0: da_p2 holds the rows of the folded conv1 weight gradient (pw_wgrad3_kernel, FOLD 2): row w + b from worker w
  // for sample b, for every worker from the owner of the sample's first step to the owner of its last
  const long long n = (long long)gridDim.x * sps;
  const int w_lo = fold_workers > 0 ? wg_owner(n, (long long)b * sps, fold_workers) : 0;
  const int w_hi = fold_workers > 0 ? wg_owner(n, (long long)(b + 1) * sps - 1, fold_workers) : -1;
  for (int k = threadIdx.x; k < c; k += kEwBlock) {
    float g = 0.f;
    if (fold_workers > 0) {
      for (int q = 0; q < kPlaneChunks; ++q) g += da_p1[((size_t)b * kPlaneChunks + q) * c + k];
      double g2 = 0.0;
      for (int w0 = w_lo; w0 <= w_hi; w0 += 32) {   // 32 rows in flight together; the sum keeps the order of the plain loop
        float v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = da_p2[(size_t)(min(w0 + u, w_hi) + b) * c + k];
#pragma unroll
        for (int u = 0; u < 32; ++u) g2 += w0 + u <= w_hi ? (double)v[u] : 0.0;
      }
      g += (float)g2;
    } else {
      for (int q = 0; q < kPlaneChunks; ++q)
        g += da_p1[((size_t)b * kPlaneChunks + q) * c + k] + da_p2[((size_t)b * kPlaneChunks + q) * c + k];
    }
    const float av = a[(size_t)b * c + k];
    const float v = g * av * (1.0f - av);
    sp[k] = v;
    dpre2[(size_t)b * c + k] = v;
  }
  __syncthreads();
  if (r <= kEwBlock && kEwBlock % r == 0) {
    // all threads: thread (group, j) sums k = group, group + groups, ...; partials through LDS
    float* pp = sh + c + r;  // groups * r partials
    const int groups = kEwBlock / r, j = threadIdx.x % r, grp = threadIdx.x / r;
    float acc = 0.f;
#pragma unroll 8
    for (int k = grp; k < c; k += groups) acc = fmaf(w2[(size_t)k * r + j], sp[k], acc);
    pp[grp * r + j] = acc;
    __syncthreads();
    if (threadIdx.x < r) {
      float t = 0.f;
      for (int q = 0; q < groups; ++q) t += pp[q * r + threadIdx.x];
      const float v = hbuf[(size_t)b * r + threadIdx.x] > 0.f ? t : 0.f;
      sd[threadIdx.x] = v;
      dh[(size_t)b * r + threadIdx.x] = v;
    }
  } else {
    for (int j = threadIdx.x; j < r; j += kEwBlock) {
      float acc = 0.f;
      for (int k = 0; k < c; ++k) acc = fmaf(w2[(size_t)k * r + j], sp[k], acc);
      const float v = hbuf[(size_t)b * r + j] > 0.f ? acc : 0.f;
      sd[j] = v;
      dh[(size_t)b * r + j] = v;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < c2; i += kEwBlock) {
    float acc = 0.f;
#pragma unroll 8
    for (int j = 0; j < r; ++j) acc = fmaf(w1[(size_t)j * c2 + i], sd[j], acc);
    ds[(size_t)b * c2 + i] = acc;
  }
}

// parameter gradients of the two Linear layers: one thread per output element.  Runs as extra block rows of
// stage_gx_kernel's launch (both only need fc_backward_kernel's results): one launch less on the stage's critical path.
struct FcGradJob {
  const float* dpre2;
  const float* dh;
  const float* hbuf;
  const float* s;
  float* gw1;
  float* gb1;
  float* gw2;
  float* gb2;
  int nb, r;
};
__device__ __forceinline__ void fc_param_grad_block(const FcGradJob& J, int block, int c) {
  const float* __restrict__ dpre2 = J.dpre2;
  const float* __restrict__ dh = J.dh;
  const float* __restrict__ hbuf = J.hbuf;
  const float* __restrict__ s = J.s;
  float* __restrict__ gw1 = J.gw1;
  float* __restrict__ gb1 = J.gb1;
  float* __restrict__ gw2 = J.gw2;
  float* __restrict__ gb2 = J.gb2;
  const int nb = J.nb, r = J.r;
  const int c2 = 2 * c;
  const int n_w1 = r * c2, n_w2 = c * r;
  int i = block * kEwBlock + threadIdx.x;
  if (i < n_w1) {
    const int j = i / c2, k = i % c2;
    float acc = 0.f;
    for (int b = 0; b < nb; ++b) acc = fmaf(dh[(size_t)b * r + j], s[(size_t)b * c2 + k], acc);
    gw1[i] = acc;
    return;
  }
  i -= n_w1;
  if (i < n_w2) {
    const int k = i / r, j = i % r;
    float acc = 0.f;
    for (int b = 0; b < nb; ++b) acc = fmaf(dpre2[(size_t)b * c + k], hbuf[(size_t)b * r + j], acc);
    gw2[i] = acc;
    return;
  }
  i -= n_w2;
  if (i < r) {
    float acc = 0.f;
    for (int b = 0; b < nb; ++b) acc += dh[(size_t)b * r + i];
    gb1[i] = acc;
    return;
  }
  i -= r;
  if (i < c) {
    float acc = 0.f;
    for (int b = 0; b < nb; ++b) acc += dpre2[(size_t)b * c + i];
    gb2[i] = acc;
  }
}

// ------------------------------------------------------------------------------------------------
// BatchNorm statistics
// ------------------------------------------------------------------------------------------------

// per plane chunk: sum (y - K), sum (y - K)^2 with K = y[0, ch, 0] (a sample of the channel, so the
// shifted sums do not cancel).  part: [(b*chunks + chunk)][2][c]
__global__ __launch_bounds__(kEwBlock) void moments_kernel(const float* __restrict__ y, float* __restrict__ part, int c, int hw) {
  __shared__ float sm[kEwBlock / DHD_WAVE];
  const int plane = blockIdx.y, b = plane / c, ch = plane % c;
  const float k = y[(size_t)ch * hw];
  const f32x4* p4 = reinterpret_cast<const f32x4*>(y + (size_t)plane * hw);
  int lo, hi;
  chunk_range<4>(hw, &lo, &hi);
  float s1 = 0.f, s2 = 0.f;
  for (int i = lo + threadIdx.x; i < hi; i += kEwBlock) {
    f32x4 v = p4[i];
    const float d0 = v.x - k, d1 = v.y - k, d2 = v.z - k, d3 = v.w - k;
    s1 += (d0 + d1) + (d2 + d3);
    s2 += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  s1 = block_sum(s1, sm);
  s2 = block_sum(s2, sm);
  if (threadIdx.x == 0) {
    float* q = part + ((size_t)(b * kPlaneChunks + blockIdx.x) * 2) * c;
    q[ch] = s1;
    q[c + ch] = s2;
  }
}

// Batch statistics -> mean, rstd, (scale, shift), prologue table (scale, 0, shift) per sample;
// running statistics updated like torch.nn.BatchNorm2d (biased variance normalises, unbiased feeds
// the running estimate).
__global__ __launch_bounds__(kEwBlock) void bn_train_finalize_kernel(const float* __restrict__ part, int n_part,
                                                                     const float* __restrict__ shift, int shift_stride,
                                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                     float* __restrict__ run_mean, float* __restrict__ run_var,
                                                                     float momentum, float eps, float* __restrict__ mean,
                                                                     float* __restrict__ rstd, float* __restrict__ scsh,
                                                                     float* __restrict__ tab, int nb, int c, int hw,
                                                                     long long* __restrict__ batches_tracked) {
  const int ch = blockIdx.x * kEwBlock + threadIdx.x;
  if (ch >= c) return;
  if (ch == 0 && batches_tracked) *batches_tracked += 1;   // nn.BatchNorm2d.num_batches_tracked
  double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
  for (int q = 0; q < n_part; ++q) {
    s1 += (double)part[((size_t)q * 2) * c + ch];
    s2 += (double)part[((size_t)q * 2 + 1) * c + ch];
  }
  const double n = (double)nb * (double)hw;
  const double md = s1 / n;
  double var = s2 / n - md * md;
  if (var < 0.0) var = 0.0;
  const double mu = (double)shift[(size_t)ch * shift_stride] + md;
  const float rs = (float)(1.0 / sqrt(var + (double)eps));
  mean[ch] = (float)mu;
  rstd[ch] = rs;
  const float sc = gamma[ch] * rs, shf = beta[ch] - (float)mu * sc;
  scsh[ch] = sc;
  scsh[c + ch] = shf;
  for (int b = 0; b < nb; ++b) {
    float* t = tab + (size_t)b * 3 * c;
    t[ch] = sc;
    t[c + ch] = 0.f;
    t[2 * c + ch] = shf;
  }
  if (run_mean) {
    const double unb = n > 1.0 ? var * n / (n - 1.0) : var;
    run_mean[ch] = (float)((1.0 - (double)momentum) * (double)run_mean[ch] + (double)momentum * mu);
    run_var[ch] = (float)((1.0 - (double)momentum) * (double)run_var[ch] + (double)momentum * unb);
  }
}

__device__ __forceinline__ void bn_eval_coef_channel(int ch, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     const float* __restrict__ run_mean, const float* __restrict__ run_var, float eps,
                                                     float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ scsh,
                                                     float* __restrict__ tab, int nb, int c) {
  const float rs = 1.0f / sqrtf(run_var[ch] + eps);
  mean[ch] = run_mean[ch];
  rstd[ch] = rs;
  const float sc = gamma[ch] * rs, shf = beta[ch] - run_mean[ch] * sc;
  scsh[ch] = sc;
  scsh[c + ch] = shf;
  for (int b = 0; b < nb; ++b) {
    float* t = tab + (size_t)b * 3 * c;
    t[ch] = sc;
    t[c + ch] = 0.f;
    t[2 * c + ch] = shf;
  }
}

__global__ __launch_bounds__(kEwBlock) void bn_eval_coef_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ run_mean, const float* __restrict__ run_var,
                                                                float eps, float* __restrict__ mean, float* __restrict__ rstd,
                                                                float* __restrict__ scsh, float* __restrict__ tab, int nb, int c) {
  const int ch = blockIdx.x * kEwBlock + threadIdx.x;
  if (ch >= c) return;
  bn_eval_coef_channel(ch, gamma, beta, run_mean, run_var, eps, mean, rstd, scsh, tab, nb, c);
}

// both layers' tables in one launch (forward-only inference: nothing lies between them); blockIdx.y = layer
struct BnEvalJob {
  const float *gamma, *beta, *run_mean, *run_var;
  float eps;
  float *mean, *rstd, *scsh, *tab;
};
__global__ __launch_bounds__(kEwBlock) void bn_eval_coef2_kernel(BnEvalJob j1, BnEvalJob j2, int nb, int c) {
  const int ch = blockIdx.x * kEwBlock + threadIdx.x;
  if (ch >= c) return;
  const BnEvalJob& j = blockIdx.y ? j2 : j1;
  bn_eval_coef_channel(ch, j.gamma, j.beta, j.run_mean, j.run_var, j.eps, j.mean, j.rstd, j.scsh, j.tab, nb, c);
}

// BatchNorm backward coefficients: dy = c0*g + c1*y + c2 (per channel), dgamma, dbeta, and the
// gradient of the bias of the convolution feeding this BatchNorm (sum of dy).
//   training: dy = gamma*rstd*(g - S1/n - (y-mu)*rstd^2*S2/n);  eval: dy = gamma*rstd*g
// COHERENT: the partial sums were written by other workgroups of the SAME launch (see BnTail): read them past the
// non-coherent cache levels.
// the channel's coefficients, dgamma, dbeta and bias gradient from its two sums s1 = sum g, s2 = sum g (y - mu)
__device__ __forceinline__ void bn_backward_coef_from_sums(double s1, double s2, int ch, const float* __restrict__ gamma,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           int training, float* __restrict__ tab, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, float* __restrict__ dbias, int nb, int c, int hw,
                                                           double* __restrict__ sums_out, const double* __restrict__ sums_in,
                                                           const double* __restrict__ loc_fwd, const float* __restrict__ shift) {
  const double n_loc = (double)nb * (double)hw;
  if (sums_out) {
    sums_out[ch] = s1; sums_out[c + ch] = s2;
    if (ch == 0) sums_out[2 * c] = n_loc;
    return;
  }
  const double n = sums_in ? sums_in[2 * c] : n_loc;
  const double g1 = sums_in ? sums_in[ch] : s1, g2 = sums_in ? sums_in[c + ch] : s2;
  const double rs = (double)rstd[ch], mu = (double)mean[ch], ga = (double)gamma[ch];
  if (dgamma) dgamma[ch] = (float)(rs * s2);
  if (dbeta) dbeta[ch] = (float)s1;
  double c0 = ga * rs, c1 = 0.0, c2 = 0.0, db = c0 * s1;
  if (training) {
    c1 = -ga * rs * rs * rs * g2 / n;
    c2 = -ga * rs * g1 / n - c1 * mu;
    db = 0.0;  // sum of dy over the (whole) batch vanishes identically
    if (sums_in) db = c0 * s1 + c1 * (loc_fwd[ch] + n_loc * (double)shift[ch]) + n_loc * c2;
  }
  if (dbias) dbias[ch] = (float)db;
  for (int b = 0; b < nb; ++b) {
    float* t = tab + (size_t)b * 3 * c;
    t[ch] = (float)c0;
    t[c + ch] = (float)c1;
    t[2 * c + ch] = (float)c2;
  }
}

template <bool COHERENT>
__device__ __forceinline__ void bn_backward_coef_channel(const float* __restrict__ part, int ch, const float* __restrict__ gamma,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         int training, float* __restrict__ tab, float* __restrict__ dgamma,
                                                         float* __restrict__ dbeta, float* __restrict__ dbias, int nb, int c, int hw,
                                                         double* __restrict__ sums_out, const double* __restrict__ sums_in,
                                                         const double* __restrict__ loc_fwd, const float* __restrict__ shift) {
  // Cross-rank statistics (nn.SyncBatchNorm): with `sums_out` only this rank's sums are written, [sum g][C] |
  // [sum g (y - mu)][C] | count, as doubles; with `sums_in` (their all-reduced values) the input-gradient coefficients use
  // the global sums and count, while dgamma / dbeta stay this rank's sums (the caller's DDP averages parameter gradients),
  // and the convolution-bias gradient is this rank's sum of dy, which no longer vanishes rank by rank:
  //   sum_local dy = c0 S1_local + c1 sum_local y + n_local c2,   sum_local y = loc_fwd[ch] + n_local shift[ch]  (the forward
  //   sums are those of y - shift).
  double s1 = 0.0, s2 = 0.0;
  if (COHERENT) {
    float v1[16], v2[16];   // in flight together; the sum keeps the order of the plain loop
    for (int q0 = 0; q0 < nb * kPlaneChunks; q0 += 16) {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int q = min(q0 + u, nb * kPlaneChunks - 1);
        v1[u] = __hip_atomic_load(part + ((size_t)q * 2) * c + ch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v2[u] = __hip_atomic_load(part + ((size_t)q * 2 + 1) * c + ch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (q0 + u < nb * kPlaneChunks) { s1 += (double)v1[u]; s2 += (double)v2[u]; }
    }
  } else {
    for (int q = 0; q < nb * kPlaneChunks; ++q) {
      s1 += (double)part[((size_t)q * 2) * c + ch];
      s2 += (double)part[((size_t)q * 2 + 1) * c + ch];
    }
  }
  bn_backward_coef_from_sums(s1, s2, ch, gamma, mean, rstd, training, tab, dgamma, dbeta, dbias, nb, c, hw, sums_out, sums_in, loc_fwd, shift);
}

struct BnRowsJob {
  const float* gamma;
  const float* mean;
  const float* rstd;
  float* tab;
  float* dgamma;
  float* dbeta;
  float* dbias;
  int training, nb, hw;
};

__global__ __launch_bounds__(kEwBlock) void bn_backward_coef_kernel(const float* __restrict__ part, const float* __restrict__ gamma,
                                                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                    int training, float* __restrict__ tab, float* __restrict__ dgamma,
                                                                    float* __restrict__ dbeta, float* __restrict__ dbias, int nb,
                                                                    int c, int hw, double* __restrict__ sums_out,
                                                                    const double* __restrict__ sums_in, const double* __restrict__ loc_fwd,
                                                                    const float* __restrict__ shift) {
  const int ch = blockIdx.x * kEwBlock + threadIdx.x;
  if (ch >= c) return;
  bn_backward_coef_channel<false>(part, ch, gamma, mean, rstd, training, tab, dgamma, dbeta, dbias, nb, c, hw, sums_out, sums_in,
                                  loc_fwd, shift);
}

// The same from the rows [n_rows][2][c] a folded weight-gradient kernel left (pw_wgrad3_kernel, FOLD 1: one row per worker).  A
// workgroup owns four channels, as in bn_stats_finalize_kernel: thread t sums rows t, t + 256, ... with one 16-byte load per sum,
// the 256 partial sums meet in LDS as doubles (fixed tree), threads 0-3 finalize one channel each.
__global__ __launch_bounds__(kEwBlock) void bn_backward_rows_kernel(const float* __restrict__ rows, int n_rows, BnRowsJob j, int c) {
  __shared__ double sm[kEwBlock][8];
  const int t = threadIdx.x, ch0 = 4 * blockIdx.x;
  const size_t row4 = (size_t)(2 * c) / 4;
  const f32x4* p1 = reinterpret_cast<const f32x4*>(rows + ch0);
  const f32x4* p2 = reinterpret_cast<const f32x4*>(rows + c + ch0);
  double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = t; i < n_rows; i += kEwBlock) {
    const f32x4 v1 = p1[(size_t)i * row4], v2 = p2[(size_t)i * row4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { a[e] += (double)v1[e]; a[4 + e] += (double)v2[e]; }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) sm[t][e] = a[e];
  __syncthreads();
  for (int s = kEwBlock / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int e = 0; e < 8; ++e) sm[t][e] += sm[t + s][e];
    }
    __syncthreads();
  }
  if (t >= 4) return;
  bn_backward_coef_from_sums(sm[0][t], sm[0][4 + t], ch0 + t, j.gamma, j.mean, j.rstd, j.training, j.tab, j.dgamma, j.dbeta, j.dbias, j.nb,
                             c, j.hw, nullptr, nullptr, nullptr, nullptr);
}

// The coefficient kernel above as the TAIL of the pass that produces its sums (one launch and ~7 us of latency chain less
// per BatchNorm backward).  The nb * kPlaneChunks workgroups of a channel count themselves in ticket[ch]; the one that
// arrives last computes the channel's coefficients in the plain kernel's summation order (bit-identical results) and leaves
// the counter at zero for the next launch.  Visibility across the eight XCDs (their L2s are not coherent with each other
// inside a kernel): the partial sums are written with agent-scope atomic stores (write-through), their acknowledgement is
// awaited (s_waitcnt) before the agent-scope ticket, and the last workgroup reads them with agent-scope atomic loads.  NOT
// with __threadfence(): an agent-scope release writes back the XCD's whole L2, and in a pass that is streaming 160 MB of
// results through it that made the pass 2.8x (blend2_bn_bwd 134 -> 375 us) and 4.7x (pair_sums 56 -> 262 us) slower.
// The counters live in the forward's `saved` block, which the forward zeroes.  ticket == nullptr (cross-rank statistics:
// the sums go through an all-reduce first): plain stores, no tail.
struct BnTail {
  int* ticket;
  const float* gamma;
  const float* mean;
  const float* rstd;
  float* tab;
  float* dgamma;
  float* dbeta;
  float* dbias;
  int training, nb, hw;
};
// thread 0 of a workgroup: its partial sums (row q of `part`) and, if it was the channel's last, the coefficients
__device__ __forceinline__ void bn_backward_publish(const BnTail& t, float* __restrict__ part, size_t q, int ch, int c, float s1,
                                                    float s2) {
  float* p1 = part + (q * 2) * c + ch;
  float* p2 = part + (q * 2 + 1) * c + ch;
  if (t.ticket == nullptr) {
    *p1 = s1;
    *p2 = s2;
    return;
  }
  __hip_atomic_store(p1, s1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(p2, s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (__hip_atomic_fetch_add(t.ticket + ch, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != t.nb * kPlaneChunks - 1) return;
  __hip_atomic_store(t.ticket + ch, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  bn_backward_coef_channel<true>(part, ch, t.gamma, t.mean, t.rstd, t.training, t.tab, t.dgamma, t.dbeta, t.dbias, t.nb, c, t.hw,
                                 nullptr, nullptr, nullptr, nullptr);
}

// sums for BatchNorm backward: S1 = sum g, S2 = sum g*(y - mean).  part: [(b*chunks+chunk)][2][c]
template <class TS>
__global__ __launch_bounds__(kEwBlock) void pair_sums_kernel(const TS* __restrict__ g, const TS* __restrict__ y,
                                                             const float* __restrict__ mean, float* __restrict__ part, int c, int hw,
                                                             BnTail tail) {
  constexpr int N = kVec16<TS>;
  using Main = Vec16<TS, true>;              // streamed once here
  using Tail = Vec16<TS, kStreamAll<TS>>;
  __shared__ float sm[kEwBlock / DHD_WAVE];
  const int plane = blockIdx.y, b = plane / c, ch = plane % c;
  const float mu = mean[ch];
  const TS* gp = g + (size_t)plane * hw;
  const TS* yp = y + (size_t)plane * hw;
  int lo, hi;
  chunk_range<N>(hw, &lo, &hi);
  float s1 = 0.f, s2 = 0.f, t1 = 0.f, t2 = 0.f;
  int i = lo + threadIdx.x;
  for (; i + kEwBlock < hi; i += 2 * kEwBlock) {   // two independent 16-byte vectors of either stream per thread
    float a[N], v[N], a2[N], v2[N];
    Main::load(gp, i, a);
    Main::load(yp, i, v);
    Main::load(gp, (size_t)i + kEwBlock, a2);
    Main::load(yp, (size_t)i + kEwBlock, v2);
    s1 = fold_sum<TS>(s1, a);
    s2 = fold_dot<TS>(s2, a, [&](int j) { return v[j] - mu; });
    t1 = fold_sum<TS>(t1, a2);
    t2 = fold_dot<TS>(t2, a2, [&](int j) { return v2[j] - mu; });
  }
  if (i < hi) {
    float a[N], v[N];
    Tail::load(gp, i, a);
    Tail::load(yp, i, v);
    s1 = fold_sum<TS>(s1, a);
    s2 = fold_dot<TS>(s2, a, [&](int j) { return v[j] - mu; });
  }
  s1 = block_sum(s1 + t1, sm);
  s2 = block_sum(s2 + t2, sm);
  if (threadIdx.x == 0) bn_backward_publish(tail, part, (size_t)(b * kPlaneChunks + blockIdx.x), ch, c, s1, s2);
}

// ------------------------------------------------------------------------------------------------
// fused blends
// ------------------------------------------------------------------------------------------------

// out = g*(a*xb) + (1-g)*((1-a)*xv),  g = sigmoid(sc*y2 + sh)
template <class TS, class TO>
__global__ __launch_bounds__(kEwBlock) void blend2_bn_kernel(const TS* __restrict__ x, const float* __restrict__ a1,
                                                             const TS* __restrict__ y2, const float* __restrict__ scsh,
                                                             TO* __restrict__ out, int c, int hw) {
  constexpr int N = kVec16<TS>;
  using X = Vec16<TS, true>;
  using Y2 = Vec16<TS, kStreamAll<TS>>;
  const int plane = blockIdx.y, b = plane / c, ch = plane % c;
  const float a = a1[plane], na = 1.0f - a, sc = scsh[ch], sh = scsh[c + ch];
  const TS* xb = x + ((size_t)b * 2 * c + ch) * hw;
  const TS* xv = x + ((size_t)b * 2 * c + c + ch) * hw;
  const TS* yp = y2 + (size_t)plane * hw;
  TO* op = out + (size_t)plane * hw;
  int lo, hi;
  chunk_range<N>(hw, &lo, &hi);
  for (int i = lo + threadIdx.x; i < hi; i += kEwBlock) {
    float p[N], q[N], s[N], r[N];
    X::load(xb, i, p);
    X::load(xv, i, q);
    Y2::load(yp, i, s);
#pragma unroll
    for (int j = 0; j < N; ++j) r[j] = blend_out(blend_gate(sc, s[j], sh), a, na, p[j], q[j]);
    IoVec<TO, N>::store(op, i, r);
  }
}

// g2 = dL/d s2 = go*(a*xb - (1-a)*xv)*g*(1-g), stored in TS; the BatchNorm-2 backward sums are those of the STORED g2 (float32
// storage: the value itself); the go-part of dL/da: sum go*(g*xb - (1-g)*xv).
// part: [(b*chunks+chunk)][2][c];  da_p1: [(b*chunks+chunk)][c]
template <class TS, class TO>
__global__ __launch_bounds__(kEwBlock) void blend2_bn_bwd_kernel(const TS* __restrict__ x, const float* __restrict__ a1,
                                                                 const TS* __restrict__ y2, const float* __restrict__ scsh,
                                                                 const float* __restrict__ mean, const TO* __restrict__ go,
                                                                 TS* __restrict__ g2, float* __restrict__ part,
                                                                 float* __restrict__ da_p1, int c, int hw, BnTail tail) {
  constexpr int N = kVec16<TS>;
  using X = Vec16<TS, true>;
  using Y2 = Vec16<TS, kStreamAll<TS>>;
  using G2 = Vec16<TS, kStreamAll<TS>>;
  using Go = IoVec<TO, N>;
  __shared__ float sm[kEwBlock / DHD_WAVE];
  const int plane = blockIdx.y, b = plane / c, ch = plane % c;
  const float a = a1[plane], na = 1.0f - a, sc = scsh[ch], sh = scsh[c + ch], mu = mean[ch];
  const TS* xb = x + ((size_t)b * 2 * c + ch) * hw;
  const TS* xv = x + ((size_t)b * 2 * c + c + ch) * hw;
  const TS* yp = y2 + (size_t)plane * hw;
  const TO* gp = go + (size_t)plane * hw;
  TS* rp = g2 + (size_t)plane * hw;
  int lo, hi;
  chunk_range<N>(hw, &lo, &hi);
  float s1 = 0.f, s2 = 0.f, sa = 0.f;
  struct In {
    raw16<TS> p, q, s;
    typename Go::raw o;
  };
  auto load = [&](int i) { return In{X::ld(xb, i), X::ld(xv, i), Y2::ld(yp, i), Go::ld(gp, i)}; };
  auto body = [&](const In& in, int i) {
    float p[N], q[N], s[N], o[N], r[N];
    widen16<TS>(in.p, p);
    widen16<TS>(in.q, q);
    widen16<TS>(in.s, s);
    Go::widen(in.o, o);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const float g = blend_gate(sc, s[j], sh);
      r[j] = blend_gate_grad(o[j], g, a, na, p[j], q[j]);
      sa = blend_da_add(sa, o[j], g, p[j], q[j]);
    }
    const raw16<TS> pk = narrow16<TS>(r);
    G2::st(rp, i, pk);
    widen16<TS>(pk, r);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      s1 += r[j];
      s2 = fmaf(r[j], s[j] - mu, s2);
    }
  };
  for_each_vector<kWideInFlight<TS>>(lo, hi, load, body);
  s1 = block_sum(s1, sm);
  s2 = block_sum(s2, sm);
  sa = block_sum(sa, sm);
  if (threadIdx.x == 0) {
    const size_t qi = (size_t)(b * kPlaneChunks + blockIdx.x);
    da_p1[qi * c + ch] = sa;
    bn_backward_publish(tail, part, qi, ch, c, s1, s2);
  }
}

// the du-part of dL/da: sum du*(xb - xv).   da_p2: [(b*chunks+chunk)][c]
template <class TS>
__global__ __launch_bounds__(kEwBlock) void blend1_da_kernel(const TS* __restrict__ x, const TS* __restrict__ du,
                                                             float* __restrict__ da_p2, int c, int hw) {
  constexpr int N = kVec16<TS>;
  using X = Vec16<TS, true>;
  using Du = Vec16<TS, kStreamAll<TS>>;
  __shared__ float sm[kEwBlock / DHD_WAVE];
  const int plane = blockIdx.y, b = plane / c, ch = plane % c;
  const TS* xb = x + ((size_t)b * 2 * c + ch) * hw;
  const TS* xv = x + ((size_t)b * 2 * c + c + ch) * hw;
  const TS* dp = du + (size_t)plane * hw;
  int lo, hi;
  chunk_range<N>(hw, &lo, &hi);
  float acc = 0.f;
  for (int i = lo + threadIdx.x; i < hi; i += kEwBlock) {
    float p[N], q[N], d[N];
    X::load(xb, i, p);
    X::load(xv, i, q);
    Du::load(dp, i, d);
    acc = fold_dot<TS>(acc, d, [&](int j) { return p[j] - q[j]; });
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) da_p2[(size_t)(b * kPlaneChunks + blockIdx.x) * c + ch] = acc;
}

// gx_bev = a*(go*g + du) + ds_bev/hw;  gx_vox = (1-a)*(go*(1-g) + du) + ds_vox/hw
template <class TS, class TO>
__global__ __launch_bounds__(kEwBlock) void stage_gx_kernel(const float* __restrict__ a1, const TS* __restrict__ y2,
                                                            const float* __restrict__ scsh, const TO* __restrict__ go,
                                                            const TS* __restrict__ du, const float* __restrict__ ds,
                                                            TO* __restrict__ gx, int c, int hw, int fc_rows, FcGradJob fc) {
  constexpr int N = kVec16<TS>;
  using S = Vec16<TS, true>;
  using Io = IoVec<TO, N>;
  if ((int)blockIdx.y < fc_rows) {   // the first block rows: the Linear layers' parameter gradients (dispatched first, no tail)
    fc_param_grad_block(fc, (int)blockIdx.y * kPlaneChunks + (int)blockIdx.x, c);
    return;
  }
  const int plane = (int)blockIdx.y - fc_rows, b = plane / c, ch = plane % c;
  const float a = a1[plane], na = 1.0f - a, sc = scsh[ch], sh = scsh[c + ch];
  const float kb = ds[(size_t)b * 2 * c + ch] / (float)hw, kv = ds[(size_t)b * 2 * c + c + ch] / (float)hw;
  const TS* yp = y2 + (size_t)plane * hw;
  const TO* gp = go + (size_t)plane * hw;
  const TS* dp = du + (size_t)plane * hw;
  TO* gb = gx + ((size_t)b * 2 * c + ch) * hw;
  TO* gv = gx + ((size_t)b * 2 * c + c + ch) * hw;
  int lo, hi;
  chunk_range<N>(hw, &lo, &hi);
  struct In {
    raw16<TS> s;
    typename Io::raw o;
    raw16<TS> d;
  };
  auto load = [&](int i) { return In{S::ld(yp, i), Io::ld(gp, i), S::ld(dp, i)}; };
  auto body = [&](const In& in, int i) {
    float s[N], o[N], d[N], rb[N], rv[N];
    widen16<TS>(in.s, s);
    Io::widen(in.o, o);
    widen16<TS>(in.d, d);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const float g = blend_gate(sc, s[j], sh);
      rb[j] = stage_gx_bev(a, o[j], g, d[j], kb);
      rv[j] = stage_gx_vox(na, o[j], g, d[j], kv);
    }
    Io::store(gb, i, rb);
    Io::store(gv, i, rv);
  };
  for_each_vector<kWideInFlight<TS>>(lo, hi, load, body);
}

#include "sfa_gemm_streamed.h"   // pw_gemm / pw_gemm6 / pw_wgrad / pw_wgrad6: the f32 reference point and bf16x6 at C = 512
#include "sfa_gemm_res.h"        // pw_gemm_res: bf16x3 at C = 512, bf16x6 at C = 128 / 256

// The forward's first launch: the channel means of x (blockIdx.y < n_planes) and, in rows of extra blocks, all FOUR weight
// images of the call -- conv1 / conv2 for the forward GEMMs and their transposes for the backward's data-gradient GEMMs, which
// round 2 packed in two separate launches (one per direction) on the critical path of either pass.
struct PackJob {
  const float* w[2];     // conv1, conv2
  u32x4* dst[4];         // conv1, conv2, conv1^T, conv2^T
  int c, cob, nt, blocks_each;
  int cu;                // images for pw_gemm_cu_kernel (sfa_gemm_cu.h: A fragments, one 32-channel tile after the other), else
                         // for pw_gemm_res (cob, nt).  float32 storage only: half storage has one kind of image, cuh_pack_weight
};

template <class TS>
__global__ __launch_bounds__(kEwBlock) void plane_mean_pack_kernel(const TS* __restrict__ x, float* __restrict__ part, int hw,
                                                                   int n_planes, PackJob job) {
  __shared__ float sm[kEwBlock / DHD_WAVE];
  if ((int)blockIdx.y < n_planes) { plane_mean_block(x, part, hw, sm); return; }
  const int pb = ((int)blockIdx.y - n_planes) * kPlaneChunks + (int)blockIdx.x;
  const int which = pb / job.blocks_each;
  if (which >= 4 || job.dst[which] == nullptr) return;   // (forward-only inference packs no transposes)
  if constexpr (kHalfStorage<TS>)
    cuh_pack_weight<TS>(job.w[which & 1], which >> 1, job.dst[which], job.c, (pb % job.blocks_each) * kEwBlock + (int)threadIdx.x);
  else if (job.cu) cu_pack_weight(job.w[which & 1], which >> 1, job.dst[which], job.c, (pb % job.blocks_each) * kEwBlock + (int)threadIdx.x);
  else pack_weight_res_block(job.w[which & 1], which >> 1, job.dst[which], job.c, job.cob, job.nt, pb % job.blocks_each);
}

// The GEMM epilogues' statistics rows [n][2][c] (n = samples x wave tiles: 5000 rows, 10 MB at B = 4) -> batch statistics and
// everything bn_train_finalize_kernel derives from them, in ONE launch (stat_reduce_kernel + bn_train_finalize_kernel took
// 9 + 7 us as two dependent launches).  A workgroup owns four channels: thread t sums rows t, t + 256, ... with two 16-byte
// loads per row (sum and sum of squares), the 256 partial sums meet in LDS as doubles, threads 0-3 finalize one channel each.
// Workgroup -> channel group is XCD-aware: the workgroups on one XCD (ids = x mod 8) take neighbouring channel groups, so that
// the 128-byte lines of a row are fetched into one L2 only.
__global__ __launch_bounds__(kEwBlock) void bn_stats_finalize_kernel(const float* __restrict__ part, int n,
                                                                     const float* __restrict__ shift, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, float* __restrict__ run_mean,
                                                                     float* __restrict__ run_var, float momentum, float eps,
                                                                     float* __restrict__ mean, float* __restrict__ rstd,
                                                                     float* __restrict__ scsh, float* __restrict__ tab, int nb, int c,
                                                                     int hw, double* __restrict__ sums_out, double* __restrict__ sums_out2,
                                                                     const double* __restrict__ sums_in, long long* __restrict__ batches_tracked) {
  // Cross-rank statistics (nn.SyncBatchNorm, dhd_sfa_stage_*_phase): with `sums_out` the kernel stops after the row
  // reduction and leaves this rank's shifted sums as doubles, [sum (y - shift)][C] | [sum (y - shift)^2][C] | count, in
  // sums_out and sums_out2; with `sums_in` it starts from such a vector (all-reduced by the caller) instead of the rows.
  __shared__ double sm[kEwBlock][8];
  const int nblk = gridDim.x, t = threadIdx.x;
  const int cg = nblk >= 8 ? (blockIdx.x & 7) * (nblk >> 3) + (blockIdx.x >> 3) : blockIdx.x;   // nblk is a multiple of 8 here
  const int ch0 = 4 * cg;
  const f32x4* p1 = reinterpret_cast<const f32x4*>(part + ch0);
  const f32x4* p2 = reinterpret_cast<const f32x4*>(part + c + ch0);
  const size_t row4 = (size_t)(2 * c) / 4;   // f32x4 units per row
  f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1, b1 = a1, b2 = a1;
  if (sums_in) n = 0;
  int i = t;
  for (; i + kEwBlock < n; i += 2 * kEwBlock) {
    a1 += p1[(size_t)i * row4];
    a2 += p2[(size_t)i * row4];
    b1 += p1[(size_t)(i + kEwBlock) * row4];
    b2 += p2[(size_t)(i + kEwBlock) * row4];
  }
  if (i < n) {
    a1 += p1[(size_t)i * row4];
    a2 += p2[(size_t)i * row4];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sm[t][e] = (double)a1[e] + (double)b1[e];
    sm[t][4 + e] = (double)a2[e] + (double)b2[e];
  }
  __syncthreads();
  for (int s = kEwBlock / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int e = 0; e < 8; ++e) sm[t][e] += sm[t + s][e];
    }
    __syncthreads();
  }
  if (t >= 4) return;
  const int ch = ch0 + t;
  double s1 = sm[0][t], s2 = sm[0][4 + t];
  double cnt = (double)nb * (double)hw;
  if (sums_out) {
    sums_out[ch] = s1; sums_out[c + ch] = s2;
    sums_out2[ch] = s1; sums_out2[c + ch] = s2;
    if (ch == 0) { sums_out[2 * c] = cnt; sums_out2[2 * c] = cnt; }
    return;
  }
  if (sums_in) { s1 = sums_in[ch]; s2 = sums_in[c + ch]; cnt = sums_in[2 * c]; }
  if (ch == 0 && batches_tracked) *batches_tracked += 1;   // nn.BatchNorm2d.num_batches_tracked (one kernel launch less per BatchNorm)
  const double md = s1 / cnt;
  double var = s2 / cnt - md * md;
  if (var < 0.0) var = 0.0;
  const double mu = (double)shift[ch] + md;
  const float rs = (float)(1.0 / sqrt(var + (double)eps));
  mean[ch] = (float)mu;
  rstd[ch] = rs;
  const float sc = gamma[ch] * rs, shf = beta[ch] - (float)mu * sc;
  scsh[ch] = sc;
  scsh[c + ch] = shf;
  for (int b = 0; b < nb; ++b) {
    float* q = tab + (size_t)b * 3 * c;
    q[ch] = sc;
    q[c + ch] = 0.f;
    q[2 * c + ch] = shf;
  }
  if (run_mean) {
    const double unb = cnt > 1.0 ? var * cnt / (cnt - 1.0) : var;
    run_mean[ch] = (float)((1.0 - (double)momentum) * (double)run_mean[ch] + (double)momentum * mu);
    run_var[ch] = (float)((1.0 - (double)momentum) * (double)run_var[ch] + (double)momentum * unb);
  }
}

// Weight gradient in the bf16x3 mode: G[co][ci] = sum_{b,p} A(co,p) * B(ci,p) with two bf16 parts per operand and the
// three products ah*bh + ah*bm + am*bh.  Same organisation as pw_wgrad6_kernel (items of 8 pixels are prologue'd and
// split ONCE by one thread and written to LDS in MFMA fragment order), but
//   * a step is 32 pixels = two MFMA k-steps: every channel row contributes one whole 128-byte line per step, so no line
//     is fetched twice -- the 16-pixel steps of the x6 kernel re-fetch the other half of each line one step later, after
//     the XCD's L2 has been turned over (PMC: 980 MB against 656 MB algorithmic) -- and there is one workgroup barrier
//     per 32 pixels instead of per 16.  Two parts instead of three make the 32-pixel double buffer fit in LDS (2 x 64 KB);
//   * the loads are line-coalesced: in one load instruction 8 adjacent lanes read the 8 four-pixel pieces of ONE row's
//     line (a wave instruction = 8 whole lines), instead of every lane reading 16 bytes of a different row (64 lines
//     touched per instruction, each line touched by four instructions).  An 8-pixel item is then assembled with one
//     lane-pair exchange (DPP quad_perm): of the rows loaded by instructions 2a and 2a+1, the even lane keeps its piece
//     of row 2a and takes its neighbour's, the odd lane does the same for row 2a+1.
//
// FOLD (stage_backward's folded flow; one operand block, c == OT): the data gradient that ran before this kernel left the
// BatchNorm-backward prologue's result in a0, so A is ONE input without a prologue, and the load stream that frees carries `aux`,
// a (nb, C, hw) tensor read at the B rows' addresses by the lanes that load them (before the pair exchange: 8 lanes = one row's
// line), for a per-row reduction a pass of its own used to make:
//   1  aux = g1, B = y1:            sum aux, sum aux*(y1 - mean[row]) (pair_sums_kernel's terms) -> fold_part[worker][2][c]
//   2  aux = du, B = x_bev|x_voxel: sum aux*(x_bev - x_voxel) per SAMPLE (blend1_da_kernel's term) -> fold_part[worker + sample][c]
//      (a worker's steps are contiguous, so worker + sample names each (worker, sample) pair that occurs exactly once)
// A and B are loaded non-temporally in this form and aux plainly: du is read once more by stage_gx right after the conv1 weight
// gradient, and with all four tensors loaded plainly the 4T of this kernel push it out of the last-level cache (stage_gx 128 ->
// 149 us, the step 16 us SLOWER than the unfolded flow; with the hint 47 us faster: LAB_NOTEBOOK R18).
// Per-thread accumulators over the worker's steps; the 8 lanes of a row meet in a fixed shuffle order: no atomics, the same bytes
// on every call.  The repeated last step (step_of) and pixel quads beyond the row's end add nothing.
template <int OT, bool A_TWO, bool B_TWO, bool B_RELU, int FOLD = 0>
__global__ __launch_bounds__(kWgBlock, 1) void pw_wgrad3_kernel(const float* __restrict__ a0, const float* __restrict__ a1,
                                                                const float* __restrict__ acoef, size_t a_bstride,
                                                                const float* __restrict__ b0, const float* __restrict__ b1,
                                                                const float* __restrict__ bcoef, size_t b_bstride,
                                                                float* __restrict__ partial, int c, int hw, int nb, int n_workers,
                                                                const float* __restrict__ aux = nullptr,
                                                                const float* __restrict__ aux_mean = nullptr,
                                                                float* __restrict__ fold_part = nullptr) {
  static_assert(FOLD == 0 || !A_TWO, "fold: A comes without a prologue");
  static_assert(FOLD != 1 || !B_TWO, "fold 1: B is y1");
  static_assert(FOLD != 2 || B_TWO, "fold 2: B is x_bev | x_voxel");
  constexpr int TA = OT / 64, TB = OT / 128;     // 32x32 tiles per wave
  constexpr int kTiles = OT / 32;                // 32-row tiles per operand
  constexpr int kOp = kTiles * 2 * 64;           // 16-byte units of one staged operand k-step: [tile][term][lane]
  constexpr int kBuf = 2 * 2 * kOp;              // [k-step 2][operand 2]
  constexpr int NJ = OT / 64;                    // load instructions per operand input and step (64 rows each)
  constexpr int NA = NJ / 2;                     // 8-pixel items per thread, operand and step
  extern __shared__ u32x4 ldsw[];                // [buf 2][k-step 2][operand 2][tile][term 2][lane]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int nob = c / OT;
  const int ob_co = (blockIdx.y / nob) * OT, ob_ci = (blockIdx.y % nob) * OT;
  const int wco = (wv >> 2) * (OT / 2), wci = (wv & 3) * (OT / 4);
  const int sps = (hw + 31) >> 5;                // steps per sample
  const long n_steps = (long)nb * sps;
  // worker w takes the contiguous range [n_steps w / n_workers, n_steps (w + 1) / n_workers).  (Tried: steps w, w + n_workers,
  // ... so that at any moment the workers together read one contiguous span of every channel row: 141 / 130 vs 133 / 128 us.)
  const int w_id = blockIdx.x;
  const int first = (int)wg_first_step(n_steps, w_id, n_workers);
  const int count = (int)wg_first_step(n_steps, w_id + 1, n_workers) - first;
  auto step_of = [&](int k) { return first + min(k, count - 1); };   // past the end: the last step again

  // loads: instruction j reads rows 64 j + 8 wv + (lane >> 3), four pixels 4 (lane & 7) ..
  const int ld_row = 8 * wv + (lane >> 3), ld_px = 4 * (lane & 7);
  // items after the pair exchange: row 64 (2a + odd) + ld_row, pixels 8 chunk .. 8 chunk + 7, chunk = (lane & 7) >> 1
  const int odd = lane & 1, chunk = (lane & 7) >> 1;
  const int it_ks = chunk >> 1, it_h = chunk & 1;   // MFMA k-step and lane half of the item

  f32x16 acc[TA][TB];
#pragma unroll
  for (int i = 0; i < TA; ++i)
#pragma unroll
    for (int j = 0; j < TB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  f32x4 raw[2][2][NJ];                           // [operand][input][load instruction]
  float cfa[NA][3], cfb[NA][3];                  // prologue coefficients of this thread's item rows (FOLD: cfa is unused)
  auto coef = [&](int op, int a, int q) {
    if constexpr (FOLD != 0) return cfb[a][q];   // A is staged as loaded: only B asks
    else return op ? cfb[a][q] : cfa[a][q];
  };
  int cur_b = -1;
  // FOLD: the auxiliary rows of load instruction j (row 64 j + ld_row, this lane's four pixels) and their running sums
  f32x4 rawx[FOLD ? NJ : 1];
  float fs1[FOLD ? NJ : 1], fs2[FOLD == 1 ? NJ : 1], fmu[FOLD == 1 ? NJ : 1];
  if constexpr (FOLD != 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      fs1[j] = 0.f;
      if constexpr (FOLD == 1) { fs2[j] = 0.f; fmu[j] = aux_mean[ob_ci + 64 * j + ld_row]; }
    }
  }
  // FOLD 2: the sums of sample bs are complete -> this worker's row of that sample
  auto fold_flush = [&](int bs) {
    if constexpr (FOLD == 2) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float v = fs1[j];
        v += __shfl_xor(v, 1, DHD_WAVE);
        v += __shfl_xor(v, 2, DHD_WAVE);
        v += __shfl_xor(v, 4, DHD_WAVE);
        if ((lane & 7) == 0) fold_part[(size_t)(blockIdx.x + bs) * c + ob_ci + 64 * j + ld_row] = v;
        fs1[j] = 0.f;
      }
    }
  };
  auto load_coefs = [&](int b) {
    if (FOLD == 2 && cur_b >= 0) fold_flush(cur_b);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int row = 64 * (2 * a + odd) + ld_row;
      [[maybe_unused]] const float* ca = FOLD == 0 ? acoef + (size_t)b * 3 * c + ob_co + row : nullptr;   // FOLD: A has no prologue
      const float* cb = bcoef + (size_t)b * 3 * c + ob_ci + row;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if constexpr (FOLD == 0) cfa[a][q] = ca[q * c];
        cfb[a][q] = cb[q * c];
      }
    }
    cur_b = b;
  };
  auto fetch = [&](int s) {
    const int b = s / sps, p = (s % sps) * 32 + ld_px;
    const size_t off = p < hw ? p : 0;
#pragma unroll
    for (int op = 0; op < 2; ++op) {
      const float* src0 = op ? b0 : a0;
      const float* src1 = op ? b1 : a1;
      const bool two = op ? B_TWO : A_TWO;
      const size_t base = (size_t)b * (op ? b_bstride : a_bstride) + (size_t)((op ? ob_ci : ob_co) + ld_row) * hw + off;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (FOLD != 0) {   // streamed once and not again in this backward: keep them out of the way of aux (header comment)
          raw[op][0][j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src0 + base + (size_t)(64 * j) * hw));
          if (two) raw[op][1][j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src1 + base + (size_t)(64 * j) * hw));
          continue;
        }
        raw[op][0][j] = *reinterpret_cast<const f32x4*>(src0 + base + (size_t)(64 * j) * hw);
        if (two) raw[op][1][j] = *reinterpret_cast<const f32x4*>(src1 + base + (size_t)(64 * j) * hw);
      }
    }
    if constexpr (FOLD != 0) {
      const size_t base = ((size_t)b * c + ob_ci + ld_row) * hw + off;
#pragma unroll
      for (int j = 0; j < NJ; ++j) rawx[j] = *reinterpret_cast<const f32x4*>(aux + base + (size_t)(64 * j) * hw);
    }
  };
  // neighbour lane's value (lanes 2k <-> 2k+1): DPP quad_perm [1,0,3,2]
  auto swap1 = [](float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xf, 0xf, true)); };
  // live (FOLD): the first staging of step s, not the last step over again
  auto stage = [&](int s, int buf, bool live) {
    const int b = s / sps, p = (s % sps) * 32 + 8 * chunk;
    if (b != cur_b) load_coefs(b);  // block-uniform, a few times per worker
    const bool in_lo = p < hw, in_hi = p + 4 < hw;
    if constexpr (FOLD != 0) {      // on the rows as loaded: pairwise over the four pixels, plain multiplies (float32 storage's fold)
      const bool ok = live && (s % sps) * 32 + ld_px < hw;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const f32x4 d = rawx[j], y = raw[1][0][j];
        if constexpr (FOLD == 1) {
          const float mu = fmu[j];
          const float t1 = (d.x + d.y) + (d.z + d.w);
          const float t2 = (d.x * (y.x - mu) + d.y * (y.y - mu)) + (d.z * (y.z - mu) + d.w * (y.w - mu));
          fs1[j] += ok ? t1 : 0.f;
          fs2[j] += ok ? t2 : 0.f;
        } else {
          const f32x4 v = raw[1][1][j];
          const float t1 = (d.x * (y.x - v.x) + d.y * (y.y - v.y)) + (d.z * (y.z - v.z) + d.w * (y.w - v.w));
          fs1[j] += ok ? t1 : 0.f;
        }
      }
    }
#pragma unroll
    for (int op = 0; op < 2; ++op) {
      const bool two = op ? B_TWO : A_TWO;
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const float k0 = coef(op, a, 0), k1 = coef(op, a, 1), k2 = coef(op, a, 2);
        const f32x2 k0v = {k0, k0}, k1v = {k1, k1}, k2v = {k2, k2};
        // assemble the item: [lo 4 pixels | hi 4 pixels] of this thread's row, per input
        float x[2][8];
#pragma unroll
        for (int in = 0; in < 2; ++in) {
          if (in == 1 && !two) continue;
          const f32x4 even_row = raw[op][in][2 * a], odd_row = raw[op][in][2 * a + 1];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float keep = odd ? odd_row[e] : even_row[e];
            const float recv = swap1(odd ? even_row[e] : odd_row[e]);
            x[in][e] = odd ? recv : keep;       // even lane holds the lower piece, odd lane the higher one
            x[in][4 + e] = odd ? keep : recv;
          }
        }
        u32x4 th, tm;
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) {
          const f32x2 x0 = {x[0][2 * jp], x[0][2 * jp + 1]};
          f32x2 t = (FOLD != 0 && op == 0) ? x0 : __builtin_elementwise_fma(k0v, x0, k2v);
          if (two) {
            const f32x2 x1 = {x[1][2 * jp], x[1][2 * jp + 1]};
            t = __builtin_elementwise_fma(k1v, x1, t);
          }
          if (op == 1 && B_RELU) { t.x = fmaxf(t.x, 0.f); t.y = fmaxf(t.y, 0.f); }
          if (!(jp < 2 ? in_lo : in_hi)) { t.x = 0.f; t.y = 0.f; }
          unsigned hh, mm;
          split2_hm(t.x, t.y, hh, mm);
          th[jp] = hh; tm[jp] = mm;
        }
        const int row = 64 * (2 * a + odd) + ld_row;
        u32x4* dst = ldsw + buf * kBuf + (it_ks * 2 + op) * kOp + (row >> 5) * 128 + (row & 31) + 32 * it_h;
        dst[0] = th;
        dst[64] = tm;
      }
    }
  };

  if (count > 0) {
    fetch(step_of(0));
    stage(step_of(0), 0, true);
    fetch(step_of(1));
  }
  __syncthreads();
  for (int k = 0; k < count; ++k) {
    const int buf = k & 1;
    // unconditional (indices clamped to the last step, whose re-staged copy nobody reads), see pw_wgrad6_kernel.
    // (tried: operand by operand -- stage A(s+1), request A(s+2), stage B(s+1), request B(s+2): no gain)
    stage(step_of(k + 1), buf ^ 1, k + 1 < count);
    fetch(step_of(k + 2));
    // keep the loads of step s + 2 ahead of this step's MFMAs (the scheduler sinks them to the end)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const u32x4* ta = ldsw + buf * kBuf + (ks * 2) * kOp + lane;
      const u32x4* tb = ta + kOp;
      u32x4 fb[TB][2];
#pragma unroll
      for (int j = 0; j < TB; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t) fb[j][t] = tb[(((wci >> 5) + j) * 2 + t) * 64];
#pragma unroll
      for (int i = 0; i < TA; ++i) {
        u32x4 fa[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) fa[t] = ta[(((wco >> 5) + i) * 2 + t) * 64];
        // terms: 0 = high, 1 = mid; smallest products first
#pragma unroll
        for (int j = 0; j < TB; ++j) acc[i][j] = mfma_bf16(fa[1], fb[j][0], acc[i][j]);
#pragma unroll
        for (int j = 0; j < TB; ++j) acc[i][j] = mfma_bf16(fa[0], fb[j][1], acc[i][j]);
#pragma unroll
        for (int j = 0; j < TB; ++j) acc[i][j] = mfma_bf16(fa[0], fb[j][0], acc[i][j]);
      }
    }
    __syncthreads();
  }

  float* po = partial + (size_t)blockIdx.x * c * c;
#pragma unroll
  for (int i = 0; i < TA; ++i)
#pragma unroll
    for (int j = 0; j < TB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int co = ob_co + wco + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
        const int ci = ob_ci + wci + 32 * j + r;
        po[(size_t)co * c + ci] = acc[i][j][e];
      }
  if constexpr (FOLD == 1) {        // one row [2][c] per worker (zeros from a worker without steps)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      float v1 = fs1[j], v2 = fs2[j];
#pragma unroll
      for (int m = 1; m < 8; m <<= 1) {
        v1 += __shfl_xor(v1, m, DHD_WAVE);
        v2 += __shfl_xor(v2, m, DHD_WAVE);
      }
      if ((lane & 7) == 0) {
        float* row = fold_part + (size_t)blockIdx.x * 2 * c + ob_ci + 64 * j + ld_row;
        row[0] = v1;
        row[c] = v2;
      }
    }
  }
  // the last sample's row; a worker without steps (fewer steps than workers) leaves a row of zeros for the sample its empty range
  // lies in, so that whoever sums a sample's rows need not know which workers had steps
  if (FOLD == 2) fold_flush(count > 0 ? cur_b : min(first / sps, nb - 1));
}

// gw[i] = sum over workers of partial[w][i].  A workgroup covers 64 consecutive elements x 4 worker phases: wave
// p sums workers p, p+4, ... with 16 loads in flight per lane, the four phase sums meet in LDS (fixed order:
// deterministic).  One thread per element with four loads in flight left the 64 MB of partials at 3 TB/s.
__global__ __launch_bounds__(kEwBlock) void wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ gw, int n,
                                                                int n_workers) {
  __shared__ float sm[kEwBlock];
  constexpr int kPhases = kEwBlock / DHD_WAVE;
  const int lane = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int i = blockIdx.x * DHD_WAVE + lane;
  float acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.f;
  if (i < n) {
    int w = ph;
    for (; w + 15 * kPhases < n_workers; w += 16 * kPhases) {
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[k] += partial[(size_t)(w + k * kPhases) * n + i];
    }
    for (; w < n_workers; w += kPhases) acc[0] += partial[(size_t)w * n + i];
  }
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < 16; k += 4) t += (acc[k] + acc[k + 1]) + (acc[k + 2] + acc[k + 3]);
  sm[threadIdx.x] = t;
  __syncthreads();
  if (ph == 0 && i < n) gw[i] = (sm[lane] + sm[DHD_WAVE + lane]) + (sm[2 * DHD_WAVE + lane] + sm[3 * DHD_WAVE + lane]);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------

constexpr int kTickWords = 64;                     // arrival counters besides the per-channel ones (see saved_layout)
constexpr int kResWaves = 8;                       // waves per resident workgroup
constexpr size_t kResTrBytes = (size_t)kResWaves * 16 * kResTrPitch * sizeof(float);  // store patches of the waves
constexpr size_t kLdsBytes = 160 * 1024;           // per-CU LDS of gfx950
constexpr size_t kResWeightMax = 128 * 1024;       // budget for the weight fragments
template <int N> using IntC = std::integral_constant<int, N>;

// (one sample of the input, 2 C hw floats, must stay below 4 GiB: the GEMMs address a sample through 32-bit buffer offsets)
inline bool stage_supported(int c, int hw) {
  return (c == 128 || (c > 0 && c % 256 == 0)) && hw > 0 && (hw & 3) == 0 && (size_t)2 * c * hw * sizeof(float) <= 0xFFFFFFFFull;
}

// C = 128 / 256 (the weight fragments of 32 channels x all K fit a wave's registers, one wave per 32 channels) and whole
// 16-byte vectors of the half type per plane
inline bool half_storage_supported(int c, int hw) { return (c == 128 || c == 256) && hw > 0 && (hw & 7) == 0 && stage_supported(c, hw); }

// Workspace layouts in BYTES, every section 256-byte aligned: the small float32 tables first, then the tensors in the storage
// type.  Besides the element size, the storage type sets the size of the weight images (float32 storage: f32 images take
// c^2 floats, bf16x6 images 1.5 c^2 -- room for 2 c^2 floats is kept; half storage: c^2 halves), of the ReLU pass bits and of
// the GEMM epilogues' statistics rows.
struct SavedLayout {
  size_t s, h, a1, tab_a, mean1, rstd1, scsh1, tab1, mean2, rstd2, scsh2, loc1, loc2, tick, wp1t, wp2t, mask, y1, y2, total;
};
inline SavedLayout saved_layout(int b, int c, int hw, int r, int storage) {
  const bool half = storage != DHD_F32;
  const size_t cc = (size_t)c * c, plane = (size_t)b * c * hw * (half ? 2 : 4);
  SavedLayout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  auto f = [&](size_t n) { return take(n * sizeof(float)); };
  L.s = f((size_t)b * 2 * c); L.h = f((size_t)b * r); L.a1 = f((size_t)b * c); L.tab_a = f((size_t)b * 3 * c);
  L.mean1 = f(c); L.rstd1 = f(c); L.scsh1 = f(2 * c); L.tab1 = f((size_t)b * 3 * c);
  L.mean2 = f(c); L.rstd2 = f(c); L.scsh2 = f(2 * c);
  // (2C + 1) doubles each: this rank's shifted sums + count (phased calls)
  L.loc1 = take((2 * (size_t)c + 1) * sizeof(double)); L.loc2 = take((2 * (size_t)c + 1) * sizeof(double));
  // arrival counters of the kernels that finish their own reductions (BnTail): [c] BatchNorm-2 backward | [c] BatchNorm-1
  // backward | kTickWords others; zeroed by the forward (fc_forward_kernel), left at zero by every kernel that uses them
  L.tick = f(2 * (size_t)c + kTickWords);
  // transposed weight images, packed by the forward for the backward
  L.wp1t = take(half ? 2 * cc : 8 * cc); L.wp2t = take(half ? 2 * cc : 8 * cc);
  // ReLU pass bits, one per activation: a word per (32 pixels, channel), [sample][wave tile][channel] (resident / streamed
  // kernels), 16-bit words in the staging lanes' order (cu kernels, sfa_gemm_cu.h: cu_mask_words), or cuh_mask_words (sfa_half.h)
  L.mask = take((half ? cuh_mask_words(b, c, hw) : (size_t)b * c * ((hw + 31) / 32)) * sizeof(unsigned));
  L.y1 = take(plane); L.y2 = take(plane);
  L.total = o;
  return L;
}

struct ScratchLayout {
  size_t wp1, wp2, part, stat_part, da1, da2, tab_g2, tab_g1, dpre2, dh, ds, mean_part, g2, g1, du, wpart, total;
};
inline ScratchLayout scratch_layout(int b, int c, int hw, int r, int storage) {
  const bool half = storage != DHD_F32;
  const size_t cc = (size_t)c * c, plane = (size_t)b * c * hw * (half ? 2 : 4);
  ScratchLayout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  auto f = [&](size_t n) { return take(n * sizeof(float)); };
  L.wp1 = take(half ? 2 * cc : 8 * cc); L.wp2 = take(half ? 2 * cc : 8 * cc);
  L.part = f((size_t)b * kPlaneChunks * 2 * c);
  // GEMM statistics rows: float32 storage a row per (sample, wave tile), or per wave of every launch (<= tiles + 63 each); half
  // storage one per workgroup of every launch (>= 8 samples per launch, <= 1024 CUs)
  L.stat_part = f((half ? (size_t)(b / 8 + 2) * 1024 : (size_t)b * ((hw + 31) / 32 + 64)) * 2 * c);
  L.da1 = f((size_t)b * kPlaneChunks * c); L.da2 = f((size_t)b * kPlaneChunks * c);
  L.tab_g2 = f((size_t)b * 3 * c); L.tab_g1 = f((size_t)b * 3 * c);
  L.dpre2 = f((size_t)b * c); L.dh = f((size_t)b * r); L.ds = f((size_t)b * 2 * c);
  L.mean_part = f((size_t)b * 2 * c * kPlaneChunks);
  L.g2 = take(plane); L.g1 = take(plane); L.du = take(plane);
  L.wpart = f((size_t)kWgWorkers * cc);
  L.total = o;
  return L;
}

inline int device_index() {
  int d = 0;
  (void)hipGetDevice(&d);
  return d < 0 || d >= 64 ? 0 : d;
}

int cu_count() {
  static int n[64] = {};
  const int dev = device_index();
  if (n[dev] == 0 && hipDeviceGetAttribute(&n[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n[dev] = -1;
  return n[dev];
}

// hipFuncSetAttribute is not a stream operation: doing it on every launch breaks stream capture (HIP graphs), so each kernel
// raises its dynamic-LDS limit once per device, on its first launch.  The flag belongs to the kernel (many share a signature).
template <auto Kern>
int lds_limit_once(size_t bytes) {
  static bool done[64] = {};
  const int dev = device_index();
  if (!done[dev]) {
    DHD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done[dev] = true;
  }
  return DHD_OK;
}
template <auto Kern, class... Args>
int launch_lds(dim3 grid, dim3 block, size_t shmem, size_t limit, hipStream_t st, Args... args) {
  if (int rc = lds_limit_once<Kern>(limit); rc != DHD_OK) return rc;
  hipLaunchKernelGGL(Kern, grid, block, shmem, st, args...);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

// 32-channel output tiles per resident workgroup: the largest of 4 / 2 / 1 whose fragments fit; 0 = does not fit
inline int res_cob(int c, int nt) {
  for (int cob = 4; cob >= 1; cob >>= 1)
    if (32 * cob <= c && (size_t)(c / 16) * cob * nt * 1024 <= kResWeightMax) return cob;
  return 0;
}

// The kernels of one call, chosen once per entry point by make_plan and passed to every launcher.
enum class Gemm { cu, cuh, res, streamed6, f32 };   // forward / data-gradient GEMMs
enum class Wgrad { w3, w6, f32, half };              // weight gradients
enum class Pack { cu, res, six, f32, cuh };          // weight images (cu / res / cuh: one launch with the channel means)
struct Plan {
  int storage;        // DHD_F32, or the half type every tensor of the stage is stored in
  Gemm gemm;
  Wgrad wgrad;
  Pack pack;
  int nt, cob;        // bf16 parts per operand (2: bf16x3, 3: bf16x6) and 32-channel tiles per resident workgroup (cu / res images)
  int cot;            // streamed6 / f32: 32-channel output tiles per workgroup
  bool fused_stats;   // training-mode BatchNorm sums come out of the GEMM epilogues (else moments_kernel)
};

// The precision of a call (dhd_sfa_weights.gemm / storage_dtype, include/dhd_amd.h) and the kernel family that serves it.
// Error codes in the order the entry points have always checked them.
int make_plan(const dhd_sfa_weights* w, int c, int hw, Plan* p) {
  *p = Plan{};
  switch (w->gemm) {
    // bf16x3 (default): bf16 MFMA on a two-way split of every float32 operand, three products per a*b, relative error
    // <= 3 * 2^-18 per product.  Measured against float64 at (2,512,200,200) the stage output is off by 2.2e-5 (bf16x6:
    // 1.2e-6, plain PyTorch fp32: 1.35e-6), well inside the 1e-3 bar of the path.
    case DHD_SFA_GEMM_DEFAULT: case DHD_SFA_GEMM_BF16X3: p->nt = 2; break;
    // bf16x6: exact three-way split, six products (float32-level accuracy)
    case DHD_SFA_GEMM_BF16X6: p->nt = 3; break;
    // f32: v_mfma_f32_32x32x2_f32, the float32 reference point of the precision table
    case DHD_SFA_GEMM_F32: p->nt = 0; break;
    default: return DHD_EINVAL;
  }
  if (w->io_dtype != DHD_F32 && w->io_dtype != DHD_F16 && w->io_dtype != DHD_BF16) return DHD_EINVAL;
  p->storage = w->storage_dtype;
  if (p->storage != DHD_F32) {
    // half storage (what an autocast region gets): x / y1 / y2 / g2 / g1 / du in fp16 or bf16 (== io_dtype), single half
    // products with float32 accumulation whatever the precision: pw_gemm_cuh / pw_wgrad_h (sfa_half.h), 64-pixel tiles
    if (p->storage != DHD_F16 && p->storage != DHD_BF16) return DHD_EINVAL;
    if (w->io_dtype != p->storage) return DHD_EINVAL;
    if (!half_storage_supported(c, hw)) return DHD_EUNSUPPORTED;
    p->gemm = Gemm::cuh; p->wgrad = Wgrad::half; p->pack = Pack::cuh;
    p->fused_stats = w->training != 0;
    return DHD_OK;
  }
  p->fused_stats = w->training && p->nt > 0;
  p->cob = p->nt > 0 ? res_cob(c, p->nt) : 0;
  p->cot = c % 256 == 0 ? 8 : 4;
  // weight gradients follow the precision alone: pw_wgrad3 (this file), pw_wgrad6 / pw_wgrad (sfa_gemm_streamed.h)
  p->wgrad = p->nt == 2 ? Wgrad::w3 : p->nt == 3 ? Wgrad::w6 : Wgrad::f32;
  if (p->nt == 2 && (c == 128 || c == 256)) {
    // bf16x3 at C = 128 / 256 (DHD-S / DHD-L: SFA(512, 256)): pw_gemm_cu (sfa_gemm_cu.h: one CU per pixel tile, weights in
    // registers, 8 waves x 32 channels or 4 waves).  C = 512 (1 MB of fragments) does not fit the register file of a CU.
    p->gemm = Gemm::cu; p->pack = Pack::cu;
  } else if ((p->nt == 2 && c == 512) || (p->nt == 3 && c <= 256)) {
    // weights resident in LDS (pw_gemm_res, sfa_gemm_res.h): bf16x6 at C = 128 (4 tiles per workgroup) / 256 (2), bf16x3 at
    // C = 512 (2): teams of 8 still beat the streamed form (2.85 vs 3.43 ms per stage at B = 3).  bf16x6 at C = 512 would need
    // teams of 16 (4.23 ms) and stays on the streamed kernels.
    p->gemm = Gemm::res; p->pack = Pack::res;
  } else if (p->nt > 0) {
    // weights streamed per pixel tile, bf16x6 operands (pw_gemm6 + its 128-channel tail launch, sfa_gemm_streamed.h): bf16x6 at
    // C >= 512 and bf16x3 at C >= 768 -- the latter has no streamed GEMM of its own, and keeps the bf16x3 weight gradient
    p->gemm = Gemm::streamed6; p->pack = Pack::six;
  } else {
    p->gemm = Gemm::f32; p->pack = Pack::f32;   // pw_gemm / pw_wgrad (sfa_gemm_streamed.h)
  }
  return DHD_OK;
}

// The four GEMMs of a call and, as template arguments, the variant of the kernels that serves each: conv1 (blend1 prologue over
// x_bev / x_voxel, bias epilogue), conv2 (BatchNorm + ReLU prologue, records the ReLU pass bits), the data gradients through
// conv2 (BatchNorm-backward prologue over g2 / y2, ReLU mask epilogue) and through conv1.  A weight gradient's second operand is
// the input of conv1 or conv2 and takes that GEMM's prologue.
// kConv2Blend (forward-only inference, cu / cuh kernels): conv2 whose epilogue goes on through BatchNorm-2, the sigmoid and the
// final blend and stores `out`; no y2, no pass bits, no statistics.
enum Op { kConv1, kConv2, kDgrad2, kDgrad1, kConv2Blend };
template <int OP>
struct Variant {
  static constexpr bool two = OP != kConv2 && OP != kConv2Blend;     // two inputs
  static constexpr bool relu = OP == kConv2 || OP == kConv2Blend;    // ReLU after the prologue
  // 0 forward (+bias), 1 dgrad with ReLU mask, 2 dgrad plain, 3 forward + blend epilogue
  static constexpr int epi = OP == kDgrad2 ? 1 : OP == kDgrad1 ? 2 : OP == kConv2Blend ? 3 : 0;
  static constexpr bool rec = OP == kConv2;     // records the ReLU pass bits
};
template <class F>
int with_op(Op op, F&& f) {
  switch (op) {
    case kConv1: return f(Variant<kConv1>{});
    case kConv2: return f(Variant<kConv2>{});
    case kDgrad2: return f(Variant<kDgrad2>{});
    case kDgrad1: return f(Variant<kDgrad1>{});
    case kConv2Blend: return f(Variant<kConv2Blend>{});
  }
  return DHD_EUNSUPPORTED;
}

// One forward / data-gradient GEMM: y = W . act(c0*in0 + c1*in1 + c2), per-(sample, channel) coefficients
template <class TS>
struct GemmCall {
  Op op;
  const TS* in0;
  const TS* in1;             // nullptr for conv2
  size_t in_bstride;
  int in_channels;
  const float* coef;
  const void* wp;            // packed weight image
  const float* bias;
  unsigned* mask;            // ReLU pass bits: written by conv2, read by dgrad 2
  float* stat_part;          // BatchNorm sums rows (fused statistics), or nullptr
  TS* y;
  const TS* aux;             // f32 dgrad 2: y1 and BatchNorm-1, the ReLU mask recomputed
  const float* aux_scsh;
  CuBlend blend;             // kConv2Blend: x, a, BatchNorm-2 scale / shift, out (y is unused)
  int out_dtype;             // kConv2Blend on float32 storage: element type of blend.out
  TS* wb;                    // data gradients of the cu kernels, float32 storage: in0 again, to take the prologue's result (or nullptr)
};

// One-CU-per-pixel-tile kernels: pw_gemm_cu (float32 storage, sfa_gemm_cu.h) and pw_gemm_cuh (half storage, sfa_half.h)
template <class TS>
int launch_gemm_cu(const GemmCall<TS>& g, int b, int c, int hw, hipStream_t st, int* stat_rows) {
  constexpr bool kHalf = !std::is_same<TS, float>::value;
  const int waves = c / 32;
  const bool blend = g.op == kConv2Blend;
  const int max_b = kHalf ? cuh_max_batch(c, waves, blend) : cu_max_batch(c, waves, blend);
  if (max_b < 1) return DHD_EUNSUPPORTED;
  const unsigned in_bytes = (unsigned)((size_t)g.in_channels * hw * sizeof(TS));
  const int nwt = kHalf ? (hw + kCuhTile - 1) / kCuhTile : (hw + 31) / 32;
  int cus = cu_count();
  if (cus <= 0) cus = 256;
  int rows_done = 0;
  for (int b0 = 0; b0 < b; b0 += max_b) {
    const int nb = b - b0 < max_b ? b - b0 : max_b;
    const long total = (long)nb * nwt;
    const int grid = (int)(total < cus ? total : cus);
    const size_t shmem = kHalf ? cuh_lds_bytes(c, waves, nb, blend) : cu_lds_bytes(c, waves, nb, blend);
    const TS* i0 = g.in0 + (size_t)b0 * g.in_bstride;
    const TS* i1 = g.in1 ? g.in1 + (size_t)b0 * g.in_bstride : nullptr;
    const float* cf = g.coef + (size_t)b0 * 3 * c;
    const u32x4* wp = static_cast<const u32x4*>(g.wp);
    unsigned* rm = g.mask ? g.mask + (kHalf ? cuh_mask_words(b0, c, hw) : cu_mask_words(b0, c, hw)) : nullptr;
    float* sp = g.stat_part ? g.stat_part + (size_t)rows_done * 2 * c : nullptr;
    rows_done += grid;                                   // one statistics row per workgroup
    TS* yo = g.y + (size_t)b0 * c * hw;
    CuBlend bl = g.blend;
    if (blend) {
      const size_t osz = kHalf ? sizeof(TS) : g.out_dtype == DHD_F32 ? 4 : 2;
      bl.x = static_cast<const TS*>(bl.x) + (size_t)b0 * 2 * c * hw;
      bl.a1 += (size_t)b0 * c;
      bl.out = static_cast<char*>(bl.out) + (size_t)b0 * c * hw * osz;
      if (kHalf) yo = static_cast<TS*>(bl.out);   // half storage: out is of the storage type and takes y's place
      else yo = static_cast<TS*>(g.blend.out);    // (unused; any valid address for the pipeline fill's dropped stores)
    }
    // EORD: with two inputs the epilogue goes before the staging (which waits for twice the loads), with one input after it --
    // measured either way (experiments/gemm_cu_bench.hip): 100 vs 107 us (conv1), 96 vs 97 (dgrad), 82 vs 76 (conv2).
    // float32: <KCN, WAVES, TWO_IN, RELU, EPI, RECORD, AUX = nt loads, R = 1, NACC = 1, ABL = 0, SAUX = 0, PP = ping-pong, BPF = 0,
    // EORD>, contiguous tile ranges
    const int rc = with_op(g.op, [&](auto v) {
      using V = decltype(v);
      auto run = [&](auto kcn) {
        constexpr int KCN = decltype(kcn)::value, WAVES = KCN / 2, EORD = V::two ? 1 : 0;
        if constexpr (kHalf) {
          return launch_lds<pw_gemm_cuh_kernel<TS, KCN, WAVES, V::two, V::relu, V::epi, V::rec, EORD>>(
              dim3(grid), dim3(WAVES * 64), shmem, kLdsBytes, st, i0, i1, g.in_bstride, in_bytes, cf, wp, g.bias, rm, sp, yo, hw, nb, bl);
        } else {
          auto go = [&](auto* to) {
            using TO = std::remove_pointer_t<decltype(to)>;
            if constexpr (V::epi == 1 || V::epi == 2) {
              if (g.wb != nullptr)   // the prologue's result goes back over in0
                return launch_lds<pw_gemm_cu_kernel<KCN, WAVES, V::two, V::relu, V::epi, V::rec, 2, 1, 1, 0, 0, true, 0, EORD, TO, true>>(
                    dim3(grid), dim3(WAVES * 64), shmem, kLdsBytes, st, i0, i1, g.in_bstride, in_bytes, cf, wp, g.bias, rm, sp, yo, hw, nb, 1,
                    bl, g.wb + (size_t)b0 * g.in_bstride);
            }
            return launch_lds<pw_gemm_cu_kernel<KCN, WAVES, V::two, V::relu, V::epi, V::rec, 2, 1, 1, 0, 0, true, 0, EORD, TO>>(
                dim3(grid), dim3(WAVES * 64), shmem, kLdsBytes, st, i0, i1, g.in_bstride, in_bytes, cf, wp, g.bias, rm, sp, yo, hw, nb, 1, bl,
                static_cast<float*>(nullptr));
          };
          if constexpr (V::epi == 3) {
            if (g.out_dtype == DHD_F16) return go((_Float16*)nullptr);
            if (g.out_dtype == DHD_BF16) return go((__bf16*)nullptr);
          }
          return go((float*)nullptr);
        }
      };
      return c == 256 ? run(IntC<16>{}) : run(IntC<8>{});
    });
    if (rc != DHD_OK) return rc;
  }
  if (stat_rows) *stat_rows = rows_done;
  return DHD_OK;
}

// Resident-weights kernels (pw_gemm_res): persistent workgroups, one per CU, teams of C / (32 COB) on one XCD.
int launch_gemm_res(const Plan& p, const GemmCall<float>& g, int b, int c, int hw, hipStream_t st, int* stat_rows) {
  int rows_done = 0;   // statistics rows written so far (bf16x3: one per wave of every launch; bf16x6: one per (sample, wave tile))
  const int groups = c / (32 * p.cob);
  const int nwt = (hw + 31) / 32;
  const size_t wbytes = (size_t)(c / 16) * p.cob * p.nt * 1024;
  const int max_b = (int)((kLdsBytes - wbytes - kResTrBytes - 64) / ((size_t)3 * c * sizeof(float)));  // samples whose tables fit next to the weights
  if (max_b < 1) return DHD_EUNSUPPORTED;
  const unsigned in_bytes = (unsigned)((size_t)g.in_channels * hw * sizeof(float));
  int cus = cu_count();
  if (cus <= 0) cus = 256;
  for (int b0 = 0; b0 < b; b0 += max_b) {
    const int nb = b - b0 < max_b ? b - b0 : max_b;
    const long total = (long)nb * nwt;
    int nteams = (cus / (8 * groups)) * 8;       // whole teams per XCD
    if (nteams < 8) nteams = 8;
    const int need = dhd_cdiv(total, kResWaves);
    if (need < nteams) nteams = dhd_cdiv(need, 8) * 8;
    const dim3 grid(nteams * groups);
    const size_t shmem = wbytes + (((size_t)nb * 3 * c + 3) & ~(size_t)3) * sizeof(float) + kResTrBytes;
    const float* i0 = g.in0 + (size_t)b0 * g.in_bstride;
    const float* i1 = g.in1 ? g.in1 + (size_t)b0 * g.in_bstride : nullptr;
    const float* cf = g.coef + (size_t)b0 * 3 * c;
    const u32x4* wp = static_cast<const u32x4*>(g.wp);
    unsigned* rm = g.mask ? g.mask + (size_t)b0 * nwt * c : nullptr;
    float* sp = g.stat_part ? g.stat_part + (size_t)rows_done * 2 * c : nullptr;
    rows_done += p.nt == 2 ? nteams : (int)total;
    float* yo = g.y + (size_t)b0 * c * hw;
    const int rc = with_op(g.op, [&](auto v) {
      using V = decltype(v);
      auto run = [&](auto nt, auto cob, auto kcn) {
        if constexpr (V::epi == 3) {   // the blend epilogue exists in the cu / cuh kernels only
          return (int)DHD_EUNSUPPORTED;
        } else {
          return launch_lds<pw_gemm_res_kernel<decltype(nt)::value, decltype(cob)::value, decltype(kcn)::value, V::two, V::relu, V::epi,
                                               kResWaves, 0, 4>>(grid, dim3(kResWaves * 64), shmem, kLdsBytes, st, i0, i1, g.in_bstride,
                                                                 in_bytes, cf, wp, g.bias, rm, sp, yo, c, hw, nb, groups, nteams);
        }
      };
      // (terms, tiles per workgroup) by channel count, as make_plan selects them
      if (p.nt == 3 && p.cob == 4 && c == 128) return run(IntC<3>{}, IntC<4>{}, IntC<8>{});
      if (p.nt == 3 && p.cob == 2 && c == 256) return run(IntC<3>{}, IntC<2>{}, IntC<16>{});
      if (p.nt == 2 && p.cob == 2 && c == 512) return run(IntC<2>{}, IntC<2>{}, IntC<32>{});
      return (int)DHD_EUNSUPPORTED;
    });
    if (rc != DHD_OK) return rc;
  }
  if (stat_rows) *stat_rows = rows_done;
  return DHD_OK;
}

// Streamed-weights kernels: pw_gemm6 (bf16x6 operands) or pw_gemm (f32), 128-pixel tiles, 32 COT output channels per workgroup
int launch_gemm_streamed(const Plan& p, const GemmCall<float>& g, int b, int c, int hw, hipStream_t st, int* stat_rows) {
  if (stat_rows) *stat_rows = b * ((hw + 31) / 32);   // a row per (sample, wave tile)
  const bool six = p.gemm == Gemm::streamed6;
  const int cot = p.cot;
  const int tps = dhd_cdiv(hw, 32 * (kPwBlock / DHD_WAVE));  // 128-pixel tiles per sample
  const unsigned in_bytes = (unsigned)((size_t)g.in_channels * hw * sizeof(float));  // one sample of in0 (and of in1, which follows it for x)
  const size_t shmem = six ? (size_t)2 * cot * 3 * 64 * 16 + (size_t)3 * c * sizeof(float) : (size_t)(2 * cot * 512 + 3 * c) * sizeof(float);
  const u32x4* wp = static_cast<const u32x4*>(g.wp);
  // Two 256-channel workgroups fit a CU (accumulators), so the tiles run in rounds of 2 x CUs.  With less
  // than two rounds of work (small batches) a partly filled round is a large share of the time: the tiles
  // beyond the full round go to a second launch of the 128-channel kernel instead (twice the workgroups,
  // three per CU, each about half as long), reading the same packed weights.  Measured -7 % (B = 1) and
  // -3 % (B = 2) on the stage; with more rounds the split gains nothing (B = 4: 1.715 vs 1.714 ms).
  int t_main = tps;
  if (six && cot == 8) {
    const int cus = cu_count();
    const long nrb = c / 256, n = (long)b * tps * nrb, slots = 2L * cus;
    if (cus > 0 && n < 2 * slots && n % slots != 0) {
      const int cand = (int)((n / slots) * slots / (b * nrb)) & ~7;
      if ((long)b * (tps - cand) * nrb * 2 <= 3L * cus) t_main = cand;
    }
  }
  const int t_tail8 = dhd_cdiv(tps - t_main, 8) * 8;  // whole groups of 8; surplus tiles exit at once
  const dim3 grid((t_main == tps ? dhd_cdiv(tps, 8) * 8 : t_main) * (c / (32 * cot)), b);
  const dim3 grid_tail(t_tail8 * (c / 128), b);
  const size_t shmem_tail = (size_t)2 * 4 * 3 * 64 * 16 + (size_t)3 * c * sizeof(float);
  return with_op(g.op, [&](auto v) {
    using V = decltype(v);
    auto run = [&](auto cot_c) {
      constexpr int COT = decltype(cot_c)::value;
      if constexpr (V::epi == 3) return (int)DHD_EUNSUPPORTED;   // the blend epilogue exists in the cu / cuh kernels only
      else {
      if (!six)
        return launch_lds<pw_gemm_kernel<COT, V::two, V::relu, V::epi>>(grid, dim3(kPwBlock), shmem, shmem, st, g.in0, g.in1, g.in_bstride,
                                                                        g.coef, static_cast<const float*>(g.wp), g.bias, g.aux, g.aux_scsh,
                                                                        g.y, c, hw);
      if (grid.x > 0) {
        const int rc = launch_lds<pw_gemm6_kernel<COT, V::two, V::relu, V::epi>>(grid, dim3(kPwBlock), shmem, shmem, st, g.in0, g.in1,
                                                                                 g.in_bstride, in_bytes, g.coef, wp, g.bias, g.mask,
                                                                                 g.stat_part, g.y, c, hw, 0, t_main, 0);
        if (rc != DHD_OK) return rc;
      }
      if (t_main < tps)
        return launch_lds<pw_gemm6_kernel<4, V::two, V::relu, V::epi>>(grid_tail, dim3(kPwBlock), shmem_tail, shmem_tail, st, g.in0,
                                                                       g.in1, g.in_bstride, in_bytes, g.coef, wp, g.bias, g.mask,
                                                                       g.stat_part, g.y, c, hw, t_main, tps, 1);
      return (int)DHD_OK;
      }
    };
    return cot == 8 ? run(IntC<8>{}) : run(IntC<4>{});
  });
}

template <class TS>
int launch_gemm(const Plan& p, const GemmCall<TS>& g, int b, int c, int hw, hipStream_t st, int* stat_rows = nullptr) {
  if constexpr (!std::is_same<TS, float>::value) {
    return launch_gemm_cu(g, b, c, hw, st, stat_rows);   // Gemm::cuh
  } else {
    if (p.gemm == Gemm::cu) return launch_gemm_cu(g, b, c, hw, st, stat_rows);
    if (p.gemm == Gemm::res) return launch_gemm_res(p, g, b, c, hw, st, stat_rows);
    return launch_gemm_streamed(p, g, b, c, hw, st, stat_rows);
  }
}

// Weight gradient gw = A . B^T over the pixels: A = BatchNorm-backward(a0, a1), B = the input of the GEMM `b_of` (conv1: blend1 of
// b0 / b1, conv2: BatchNorm + ReLU of b0).  Per-worker partial matrices, reduced deterministically by wgrad_reduce_kernel.
// (tried at C = 256 in the bf16x3 mode: 128 x 128 tiles, two workgroups per CU, operands read twice through L2: 233 / 189 us
// against 166 / 138 us for one 256 x 256 tile per CU)
// fold (Wgrad::w3 on float32 storage, C = 128 / 256): a0 holds the prologue's result already (the data gradient ran first with
// GemmCall::wb) and the kernel also reduces `aux` along the B rows into `rows` (pw_wgrad3_kernel, FOLD = mode).
struct WgradFold {
  int mode;            // 0 none, 1 BatchNorm-1 sums of aux = g1 (mean = mean1), 2 per-sample dL/da sums of aux = du
  const float* aux;
  const float* mean;
  float* rows;
};
template <class TS>
int launch_wgrad(const Plan& p, Op b_of, const TS* a0, const TS* a1, const float* acoef, size_t a_bs, const TS* b0, const TS* b1,
                 const float* bcoef, size_t b_bs, float* partial, float* gw, int b, int c, int hw, hipStream_t st,
                 WgradFold fold = WgradFold{0, nullptr, nullptr, nullptr}) {
  const int ot = c == 128 ? 128 : 256;
  const int nob = wgrad_blocks(c);
  const int workers = wgrad_workers(c);
  const dim3 grid(workers, nob), block(kWgBlock);
  const int rc = with_op(b_of, [&](auto v) {
    using V = decltype(v);
    auto run = [&](auto ot_c) {
      constexpr int OT = decltype(ot_c)::value;
      if constexpr (!std::is_same<TS, float>::value) {
        const size_t shmem = (size_t)2 * 4 * 2 * (OT / 32) * 64 * 16;
        return launch_lds<pw_wgrad_h_kernel<TS, OT, V::two, V::relu>>(grid, block, shmem, shmem, st, a0, a1, acoef, a_bs, b0, b1, bcoef,
                                                                     b_bs, partial, c, hw, b, workers);
      } else if (p.wgrad == Wgrad::w3) {
        const size_t shmem = (size_t)2 * 2 * 2 * (OT / 32) * 2 * 64 * 16;
        if (fold.mode != 0) {
          if (nob != 1 || fold.mode != (V::two ? 2 : 1)) return (int)DHD_EUNSUPPORTED;
          return launch_lds<pw_wgrad3_kernel<OT, false, V::two, V::relu, V::two ? 2 : 1>>(grid, block, shmem, shmem, st, a0, a1, acoef, a_bs, b0, b1,
                                                                                         bcoef, b_bs, partial, c, hw, b, workers, fold.aux,
                                                                                         fold.mean, fold.rows);
        }
        return launch_lds<pw_wgrad3_kernel<OT, true, V::two, V::relu>>(grid, block, shmem, shmem, st, a0, a1, acoef, a_bs, b0, b1, bcoef,
                                                                      b_bs, partial, c, hw, b, workers, static_cast<const float*>(nullptr),
                                                                      static_cast<const float*>(nullptr), static_cast<float*>(nullptr));
      } else if (p.wgrad == Wgrad::w6) {
        const size_t shmem = (size_t)2 * 2 * (OT / 32) * 3 * 64 * 16;
        return launch_lds<pw_wgrad6_kernel<OT, true, V::two, V::relu>>(grid, block, shmem, shmem, st, a0, a1, acoef, a_bs, b0, b1, bcoef,
                                                                      b_bs, partial, c, hw, b, workers);
      } else {
        const size_t shmem = (size_t)4 * OT * kWgStride * sizeof(float);
        return launch_lds<pw_wgrad_kernel<OT, true, V::two, V::relu>>(grid, block, shmem, shmem, st, a0, a1, acoef, a_bs, b0, b1, bcoef,
                                                                     b_bs, partial, c, hw, b, workers);
      }
    };
    return ot == 128 ? run(IntC<128>{}) : run(IntC<256>{});
  });
  if (rc != DHD_OK) return rc;
  const int n = c * c;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(dhd_cdiv(n, DHD_WAVE)), dim3(kEwBlock), 0, st, partial, gw, n, workers);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

// The channel means of x and the four weight images of a call: conv1 and conv2 (scratch), their transposes for the data
// gradients (saved).  dst: conv1, conv2, conv1^T, conv2^T.
template <class TS>
int launch_mean_pack(const Plan& p, const TS* x, const float* w1, const float* w2, void* const dst[4], float* mean_part, int b,
                     int c, int hw, hipStream_t st) {
  const int blocks_each = dhd_cdiv((c / 32) * (c / 16) * 64, kEwBlock);
  if (p.pack == Pack::cu || p.pack == Pack::res || p.pack == Pack::cuh) {   // one launch: the images in rows of extra blocks
    PackJob job;
    job.w[0] = w1; job.w[1] = w2;
    for (int i = 0; i < 4; ++i) job.dst[i] = static_cast<u32x4*>(dst[i]);
    job.c = c; job.nt = p.nt; job.cob = p.cob; job.cu = p.pack == Pack::cu ? 1 : 0;
    job.blocks_each = blocks_each;
    const dim3 grid(kPlaneChunks, b * 2 * c + dhd_cdiv(4 * blocks_each, kPlaneChunks));
    hipLaunchKernelGGL(plane_mean_pack_kernel<TS>, grid, dim3(kEwBlock), 0, st, x, mean_part, hw, b * 2 * c, job);
    DHD_LAUNCH_CHECK();
    return DHD_OK;
  }
  if constexpr (std::is_same_v<TS, float>) {
    hipLaunchKernelGGL(plane_mean_kernel, dim3(kPlaneChunks, b * 2 * c), dim3(kEwBlock), 0, st, x, mean_part, hw);
    DHD_LAUNCH_CHECK();
    for (int i = 0; i < 4; ++i) {   // the streamed / f32 forms pack one weight per launch
      const float* wi = i & 1 ? w2 : w1;
      if (p.pack == Pack::six)
        hipLaunchKernelGGL(pack_weight6_kernel, dim3(blocks_each), dim3(kEwBlock), 0, st, wi, i >> 1, static_cast<u32x4*>(dst[i]), c, p.cot);
      else
        hipLaunchKernelGGL(pack_weight_kernel, dim3(dhd_cdiv(c * c, kEwBlock)), dim3(kEwBlock), 0, st, wi, i >> 1, static_cast<float*>(dst[i]),
                           c, p.cot);
      DHD_LAUNCH_CHECK();
    }
    return DHD_OK;
  }
  return DHD_EINVAL;   // (make_plan gives half storage Pack::cuh)
}

// Forward in up to three phases, cut at the two BatchNorm statistics points.  sync == nullptr: all phases in one call with
// this call's own statistics.  sync != nullptr (nn.SyncBatchNorm): phases [lo, hi]; a phase that ends at a statistics point
// leaves this rank's sums in `sync` ((2C + 1) doubles: [sum (y - bias)][C] | [sum (y - bias)^2][C] | count), the next phase
// starts from the caller's all-reduced vector in the same place.
template <class TS, class TO>
int stage_forward(const Plan& p, const TS* x, const dhd_sfa_weights* w, TO* out, void* saved, void* scratch, int b, int c, int hw,
                  int lo, int hi, double* sync, hipStream_t st) {
  const int r = w->hidden;
  const SavedLayout S = saved_layout(b, c, hw, r, p.storage);
  const ScratchLayout T = scratch_layout(b, c, hw, r, p.storage);
  char* sv = static_cast<char*>(saved);
  char* sc = static_cast<char*>(scratch);
  auto SF = [&](size_t off) { return reinterpret_cast<float*>(sv + off); };
  auto TF = [&](size_t off) { return reinterpret_cast<float*>(sc + off); };
  TS* y1 = reinterpret_cast<TS*>(sv + S.y1);
  TS* y2 = reinterpret_cast<TS*>(sv + S.y2);
  float* stat_part = p.fused_stats ? TF(T.stat_part) : nullptr;
  const dim3 planes(kPlaneChunks, b * c), per_ch(dhd_cdiv(c, kEwBlock));
  const size_t cs = (size_t)c * hw;
  int stat_rows = 0, rc;
  struct Bn {
    const float *shift, *gamma, *beta;
    float *run_mean, *run_var;
    float momentum, eps;
    long long* batches;
    float *mean, *rstd, *scsh;
    double* loc;
  };
  const Bn bn1 = {w->conv1_b, w->bn1_w, w->bn1_b, w->bn1_mean, w->bn1_var, w->momentum1, w->eps1,
                  reinterpret_cast<long long*>(w->bn1_batches), SF(S.mean1), SF(S.rstd1), SF(S.scsh1), reinterpret_cast<double*>(sv + S.loc1)};
  const Bn bn2 = {w->conv2_b, w->bn2_w, w->bn2_b, w->bn2_mean, w->bn2_var, w->momentum2, w->eps2,
                  reinterpret_cast<long long*>(w->bn2_batches), SF(S.mean2), SF(S.rstd2), SF(S.scsh2), reinterpret_cast<double*>(sv + S.loc2)};
  // a phase that ends at a statistics point: this rank's sums only (also kept in `saved` for the backward's bias gradient)
  auto publish = [&](const Bn& n, float* tab) {
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(c / 4), dim3(kEwBlock), 0, st, TF(T.stat_part), stat_rows, n.shift, n.gamma, n.beta,
                       n.run_mean, n.run_var, n.momentum, n.eps, n.mean, n.rstd, n.scsh, tab, b, c, hw, sync, n.loc, nullptr, nullptr);
  };
  // the layer's coefficient tables: batch statistics (training) or the running ones
  auto coef = [&](const Bn& n, const TS* y, float* tab) {
    if (!w->training) {
      hipLaunchKernelGGL(bn_eval_coef_kernel, per_ch, dim3(kEwBlock), 0, st, n.gamma, n.beta, n.run_mean, n.run_var, n.eps, n.mean, n.rstd,
                         n.scsh, tab, b, c);
    } else if (p.fused_stats) {   // the GEMM epilogue left per-(sample, wave tile) sums shifted by the bias
      hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(c / 4), dim3(kEwBlock), 0, st, TF(T.stat_part), stat_rows, n.shift, n.gamma, n.beta,
                         n.run_mean, n.run_var, n.momentum, n.eps, n.mean, n.rstd, n.scsh, tab, b, c, hw, nullptr, nullptr, sync, n.batches);
    } else if constexpr (std::is_same<TS, float>::value) {   // f32 GEMMs: a statistics pass of their own
      hipLaunchKernelGGL(moments_kernel, planes, dim3(kEwBlock), 0, st, y, TF(T.part), c, hw);
      hipLaunchKernelGGL(bn_train_finalize_kernel, per_ch, dim3(kEwBlock), 0, st, TF(T.part), b * kPlaneChunks, y, hw, n.gamma, n.beta,
                         n.run_mean, n.run_var, n.momentum, n.eps, n.mean, n.rstd, n.scsh, tab, b, c, hw, n.batches);
    }
  };
  if (sync && !p.fused_stats) return DHD_EUNSUPPORTED;   // cross-rank statistics: training mode, bf16 GEMM precisions or half storage

  if (lo <= 0) {
    void* const dst[4] = {sc + T.wp1, sc + T.wp2, sv + S.wp1t, sv + S.wp2t};
    rc = launch_mean_pack(p, x, w->conv1_w, w->conv2_w, dst, TF(T.mean_part), b, c, hw, st);
    if (rc != DHD_OK) return rc;
    hipLaunchKernelGGL(fc_forward_kernel, dim3(b), dim3(kFcBlock), (size_t)(2 * c + r) * sizeof(float), st, TF(T.mean_part), w->fc1_w,
                       w->fc1_b, w->fc2_w, w->fc2_b, SF(S.s), SF(S.h), SF(S.a1), SF(S.tab_a), c, r, hw, reinterpret_cast<int*>(sv + S.tick),
                       2 * c + kTickWords);
    DHD_LAUNCH_CHECK();
    // y1 = conv1(blend1(x))
    rc = launch_gemm(p, GemmCall<TS>{kConv1, x, x + cs, 2 * cs, c, SF(S.tab_a), sc + T.wp1, w->conv1_b, nullptr, stat_part, y1},
                     b, c, hw, st, &stat_rows);
    if (rc != DHD_OK) return rc;
    if (sync) {
      publish(bn1, SF(S.tab1));
      DHD_LAUNCH_CHECK();
    }
  }
  if (hi <= 0) return DHD_OK;
  if (lo <= 1) {
    coef(bn1, y1, SF(S.tab1));
    DHD_LAUNCH_CHECK();
    // y2 = conv2(relu(bn1(y1)))
    rc = launch_gemm(p, GemmCall<TS>{kConv2, y1, nullptr, cs, c, SF(S.tab1), sc + T.wp2, w->conv2_b,
                                     reinterpret_cast<unsigned*>(sv + S.mask), stat_part, y2},
                     b, c, hw, st, &stat_rows);
    if (rc != DHD_OK) return rc;
    if (sync) {
      publish(bn2, TF(T.tab_g2));
      DHD_LAUNCH_CHECK();
    }
  }
  if (hi <= 1) return DHD_OK;
  coef(bn2, y2, TF(T.tab_g2));   // bn2 has no consumer GEMM in the forward: the table slot is a sink
  hipLaunchKernelGGL((blend2_bn_kernel<TS, TO>), planes, dim3(kEwBlock), 0, st, x, SF(S.a1), y2, SF(S.scsh2), out, c, hw);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

// DHD_SFA_BWD_FOLD = 0 | 1 | 2 | 3: the folded backward flow for no layer / layer 2 / layer 1 / both; + 4: layer 2 as ONE launch
// on pairs of CUs (pw_pair_kernel) in place of its two GEMMs, whatever bit 1 says; + 8: the same for layer 1 (pw_pair1_kernel),
// whatever bit 2 says.  Decimal 0 .. 15, anything else is the default (A/B switch, read once per process).  Default: see
// LAB_NOTEBOOK R18, R22, R26.
int bwd_fold_mode() {
  static const int mode = [] {
    const char* e = getenv("DHD_SFA_BWD_FOLD");
    if (e == nullptr || e[0] < '0' || e[0] > '9') return kBwdFoldDefault;
    if (e[1] == 0) return e[0] - '0';
    if (e[0] == '1' && e[1] >= '0' && e[1] <= '5' && e[2] == 0) return 10 + (e[1] - '0');
    return kBwdFoldDefault;
  }();
  return mode;
}

// Layer 2 of the backward in one launch (sfa_gemm_pair.h): g1, this call's conv2 weight gradient and the BatchNorm-1 sums per worker
int launch_pair(const PairArgs& a, float* gw, int c, hipStream_t st) {
  const size_t shmem = pair_lds_bytes(c);
  int rc;
  if (c == 256) rc = launch_lds<pw_pair_kernel<256, 2, WgFirstStep>>(dim3(kPairGrid), dim3(512), shmem, shmem, st, a);
  else if (c == 128) rc = launch_lds<pw_pair_kernel<128, 2, WgFirstStep>>(dim3(kPairGrid), dim3(256), shmem, shmem, st, a);
  else return DHD_EUNSUPPORTED;
  if (rc != DHD_OK) return rc;
  const int n = c * c;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(dhd_cdiv(n, DHD_WAVE)), dim3(kEwBlock), 0, st, a.partial, gw, n, kPairWorkers);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

// Layer 1 of the backward in one launch (sfa_gemm_pair1.h): du, this call's conv1 weight gradient and the du-part of dL/da per
// (pair-worker, sample)
int launch_pair1(const Pair1Args& a, float* gw, int c, hipStream_t st) {
  const size_t shmem = pair1_lds_bytes(c);
  int rc;
  if (c == 256) rc = launch_lds<pw_pair1_kernel<256, 2, WgFirstStep>>(dim3(kPairGrid), dim3(512), shmem, shmem, st, a);
  else if (c == 128) rc = launch_lds<pw_pair1_kernel<128, 2, WgFirstStep>>(dim3(kPairGrid), dim3(256), shmem, shmem, st, a);
  else return DHD_EUNSUPPORTED;
  if (rc != DHD_OK) return rc;
  const int n = c * c;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(dhd_cdiv(n, DHD_WAVE)), dim3(kEwBlock), 0, st, a.partial, gw, n, kPairWorkers);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

// Backward in up to three phases, cut where the two BatchNorm backward passes need their sums (sum g, sum g (y - mu)); `sync`
// as in stage_forward ((2C + 1) doubles: [sum g][C] | [sum g (y - mu)][C] | count).
template <class TS, class TO>
int stage_backward(const Plan& p, const TS* x, const dhd_sfa_weights* w, const void* saved, const TO* gout, TO* gx,
                   const dhd_sfa_grads* grads, void* scratch, int b, int c, int hw, int lo, int hi, double* sync, hipStream_t st) {
  const int r = w->hidden;
  const SavedLayout S = saved_layout(b, c, hw, r, p.storage);
  const ScratchLayout T = scratch_layout(b, c, hw, r, p.storage);
  char* sv = const_cast<char*>(static_cast<const char*>(saved));
  char* sc = static_cast<char*>(scratch);
  auto SF = [&](size_t off) { return reinterpret_cast<float*>(sv + off); };
  auto TF = [&](size_t off) { return reinterpret_cast<float*>(sc + off); };
  const TS* y1 = reinterpret_cast<const TS*>(sv + S.y1);
  const TS* y2 = reinterpret_cast<const TS*>(sv + S.y2);
  TS* g2 = reinterpret_cast<TS*>(sc + T.g2);
  TS* g1 = reinterpret_cast<TS*>(sc + T.g1);
  TS* du = reinterpret_cast<TS*>(sc + T.du);
  unsigned* mask = reinterpret_cast<unsigned*>(sv + S.mask);
  int* tick = reinterpret_cast<int*>(sv + S.tick);
  const dim3 planes(kPlaneChunks, b * c), per_ch(dhd_cdiv(c, kEwBlock));
  const size_t cs = (size_t)c * hw;
  int rc;
  // without cross-rank statistics the pass that makes a layer's sums finishes its own reduction (BnTail, on that layer's
  // arrival counters): no bn_backward_coef launch
  const BnTail tail2 = {sync ? nullptr : tick, w->bn2_w, SF(S.mean2), SF(S.rstd2), TF(T.tab_g2), grads->bn2_w, grads->bn2_b,
                        grads->conv2_b, w->training, b, hw};
  const BnTail tail1 = {sync ? nullptr : tick + c, w->bn1_w, SF(S.mean1), SF(S.rstd1), TF(T.tab_g1), grads->bn1_w, grads->bn1_b,
                        grads->conv1_b, w->training, b, hw};
  // with them: this rank's sums out at the end of a phase, the all-reduced ones in at the start of the next
  auto coef_out = [&](const BnTail& t) {
    hipLaunchKernelGGL(bn_backward_coef_kernel, per_ch, dim3(kEwBlock), 0, st, TF(T.part), t.gamma, t.mean, t.rstd, w->training, t.tab,
                       t.dgamma, t.dbeta, t.dbias, b, c, hw, sync, nullptr, nullptr, nullptr);
  };
  auto coef_in = [&](const BnTail& t, size_t loc, const float* bias) {
    hipLaunchKernelGGL(bn_backward_coef_kernel, per_ch, dim3(kEwBlock), 0, st, TF(T.part), t.gamma, t.mean, t.rstd, w->training, t.tab,
                       t.dgamma, t.dbeta, t.dbias, b, c, hw, nullptr, sync, reinterpret_cast<const double*>(sv + loc), bias);
  };
  if (sync && !p.fused_stats) return DHD_EUNSUPPORTED;
  // The folded flow (header comment): per layer, the data gradient first, leaving its prologue's result over g, then the weight
  // gradient on that one tensor, which also makes the sums pair_sums / blend1_da made in passes of their own.  The worker rows
  // live where scratch is dead: du's region during phase 1, g2's during phase 2.  Bit 4 of the switch: layer 2 as one launch on
  // pairs of CUs (launch_pair), under the same gate, its 128 worker rows in du's region too; bit 8: layer 1 likewise (launch_pair1),
  // its 128 + b rows at the head of g2's region.
  // The gate is `sync == nullptr`, not the entry point: the phase entry points keep the unfolded flow only because they always pass
  // a `sync`; a caller that cut the folded flow into phases would find gy, not g, in g2 / g1 between them.
  int fold = 0;
  const int fold_workers = wgrad_workers(c);   // the workers launch_wgrad gives the kernels whose rows are read back below
  if constexpr (std::is_same_v<TS, float>) {
    const size_t plane = (size_t)b * cs * sizeof(float);
    // one operand block per launch (all B rows in every worker), and the worker rows fit the dead regions
    if (p.gemm == Gemm::cu && p.wgrad == Wgrad::w3 && sync == nullptr && wgrad_blocks(c) == 1 && (size_t)fold_workers * 2 * c * sizeof(float) <= plane &&
        (size_t)(fold_workers + b) * c * sizeof(float) <= plane)
      fold = bwd_fold_mode();
  }
  float* rows1 = reinterpret_cast<float*>(du);   // [worker][2][c]: BatchNorm-1 sums
  float* rows2 = reinterpret_cast<float*>(g2);   // [worker + sample][c]: du-part of dL/da

  if (lo <= 0) {
    // g2 = dL/ds2, BatchNorm-2 sums, go-part of dL/da
    hipLaunchKernelGGL((blend2_bn_bwd_kernel<TS, TO>), planes, dim3(kEwBlock), 0, st, x, SF(S.a1), y2, SF(S.scsh2), SF(S.mean2), gout, g2, TF(T.part),
                       TF(T.da1), c, hw, tail2);
    if (sync) coef_out(tail2);
    DHD_LAUNCH_CHECK();
  }
  if (hi <= 0) return DHD_OK;
  if (lo <= 1) {
    if (sync) coef_in(tail2, S.loc2, w->conv2_b);
    DHD_LAUNCH_CHECK();
  }
  if (lo <= 1 && (fold & 4)) {
    if constexpr (std::is_same_v<TS, float>) {
      // g1 = (W2^T dy2) * [z1 > 0], dW2 = dy2 . z1^T and the BatchNorm-1 sums of g1 per worker; g2 stays as it is
      rc = launch_pair(PairArgs{g2, y2, TF(T.tab_g2), reinterpret_cast<const u32x4*>(sv + S.wp2t), y1, SF(S.scsh1), SF(S.mean1), g1, TF(T.wpart),
                                rows1, hw, b},
                       grads->conv2_w, c, st);
      if (rc != DHD_OK) return rc;
      const BnRowsJob j1 = {tail1.gamma, tail1.mean, tail1.rstd, tail1.tab, tail1.dgamma, tail1.dbeta, tail1.dbias, w->training, b, hw};
      hipLaunchKernelGGL(bn_backward_rows_kernel, dim3(c / 4), dim3(kEwBlock), 0, st, rows1, kPairWorkers, j1, c);
      DHD_LAUNCH_CHECK();
    }
  } else if (lo <= 1 && (fold & 1)) {
    if constexpr (std::is_same_v<TS, float>) {
      // g1 = (W2^T dy2) * [z1 > 0]; dy2 stays in g2
      rc = launch_gemm(p, GemmCall<TS>{kDgrad2, g2, y2, cs, c, TF(T.tab_g2), sv + S.wp2t, nullptr, mask, nullptr, g1, y1, SF(S.scsh1), CuBlend{}, 0, g2},
                       b, c, hw, st);
      if (rc != DHD_OK) return rc;
      // dW2 = dy2 . z1^T, and the BatchNorm-1 sums of g1 per worker
      rc = launch_wgrad<TS>(p, kConv2, g2, nullptr, nullptr, cs, y1, nullptr, SF(S.tab1), cs, TF(T.wpart), grads->conv2_w, b, c, hw, st,
                            WgradFold{1, g1, SF(S.mean1), rows1});
      if (rc != DHD_OK) return rc;
      const BnRowsJob j1 = {tail1.gamma, tail1.mean, tail1.rstd, tail1.tab, tail1.dgamma, tail1.dbeta, tail1.dbias, w->training, b, hw};
      hipLaunchKernelGGL(bn_backward_rows_kernel, dim3(c / 4), dim3(kEwBlock), 0, st, rows1, fold_workers, j1, c);
      DHD_LAUNCH_CHECK();
    }
  } else if (lo <= 1) {
    // dW2 = dy2 . z1^T
    rc = launch_wgrad<TS>(p, kConv2, g2, y2, TF(T.tab_g2), cs, y1, nullptr, SF(S.tab1), cs, TF(T.wpart), grads->conv2_w, b, c, hw, st);
    if (rc != DHD_OK) return rc;
    // g1 = (W2^T dy2) * [z1 > 0]
    rc = launch_gemm(p, GemmCall<TS>{kDgrad2, g2, y2, cs, c, TF(T.tab_g2), sv + S.wp2t, nullptr, mask, nullptr, g1, y1, SF(S.scsh1)},
                     b, c, hw, st);
    if (rc != DHD_OK) return rc;
    hipLaunchKernelGGL(pair_sums_kernel<TS>, planes, dim3(kEwBlock), 0, st, g1, y1, SF(S.mean1), TF(T.part), c, hw, tail1);
    if (sync) coef_out(tail1);
    DHD_LAUNCH_CHECK();
  }
  if (hi <= 1) return DHD_OK;
  if (sync) coef_in(tail1, S.loc1, w->conv1_b);
  DHD_LAUNCH_CHECK();
  if (fold & 8) {
    if constexpr (std::is_same_v<TS, float>) {
      // du = W1^T dy1, dW1 = dy1 . u^T and the du-part of dL/da per (pair-worker, sample); g1 stays as it is
      rc = launch_pair1(Pair1Args{g1, y1, TF(T.tab_g1), reinterpret_cast<const u32x4*>(sv + S.wp1t), x, SF(S.tab_a), du, TF(T.wpart), rows2, hw, b},
                        grads->conv1_w, c, st);
      if (rc != DHD_OK) return rc;
      hipLaunchKernelGGL(fc_backward_kernel, dim3(b), dim3(kEwBlock), (size_t)(c + r + kEwBlock) * sizeof(float), st, TF(T.da1), rows2,
                         SF(S.a1), SF(S.h), w->fc1_w, w->fc2_w, TF(T.dpre2), TF(T.dh), TF(T.ds), c, r, kPairWorkers, (hw + 31) / 32);
    }
  } else if (fold & 2) {
    if constexpr (std::is_same_v<TS, float>) {
      // du = W1^T dy1; dy1 stays in g1
      rc = launch_gemm(p, GemmCall<TS>{kDgrad1, g1, y1, cs, c, TF(T.tab_g1), sv + S.wp1t, nullptr, nullptr, nullptr, du, nullptr, nullptr, CuBlend{}, 0, g1},
                       b, c, hw, st);
      if (rc != DHD_OK) return rc;
      // dW1 = dy1 . u^T, and the du-part of dL/da per (worker, sample)
      rc = launch_wgrad<TS>(p, kConv1, g1, nullptr, nullptr, cs, x, x + cs, SF(S.tab_a), 2 * cs, TF(T.wpart), grads->conv1_w, b, c, hw, st,
                            WgradFold{2, du, nullptr, rows2});
      if (rc != DHD_OK) return rc;
      hipLaunchKernelGGL(fc_backward_kernel, dim3(b), dim3(kEwBlock), (size_t)(c + r + kEwBlock) * sizeof(float), st, TF(T.da1), rows2,
                         SF(S.a1), SF(S.h), w->fc1_w, w->fc2_w, TF(T.dpre2), TF(T.dh), TF(T.ds), c, r, fold_workers, (hw + 31) / 32);
    }
  } else {
    // dW1 = dy1 . u^T
    rc = launch_wgrad<TS>(p, kConv1, g1, y1, TF(T.tab_g1), cs, x, x + cs, SF(S.tab_a), 2 * cs, TF(T.wpart), grads->conv1_w, b, c, hw, st);
    if (rc != DHD_OK) return rc;
    // du = W1^T dy1
    rc = launch_gemm(p, GemmCall<TS>{kDgrad1, g1, y1, cs, c, TF(T.tab_g1), sv + S.wp1t, nullptr, nullptr, nullptr, du}, b, c, hw, st);
    if (rc != DHD_OK) return rc;
    hipLaunchKernelGGL(blend1_da_kernel<TS>, planes, dim3(kEwBlock), 0, st, x, du, TF(T.da2), c, hw);
    hipLaunchKernelGGL(fc_backward_kernel, dim3(b), dim3(kEwBlock), (size_t)(c + r + kEwBlock) * sizeof(float), st, TF(T.da1), TF(T.da2),
                       SF(S.a1), SF(S.h), w->fc1_w, w->fc2_w, TF(T.dpre2), TF(T.dh), TF(T.ds), c, r, 0, 0);
  }
  const int n_fc = r * 2 * c + c * r + r + c;
  const FcGradJob fcj = {TF(T.dpre2), TF(T.dh), SF(S.h), SF(S.s), grads->fc1_w, grads->fc1_b, grads->fc2_w, grads->fc2_b, b, r};
  const int fc_rows = dhd_cdiv(dhd_cdiv(n_fc, kEwBlock), kPlaneChunks);
  const dim3 planes_fc(kPlaneChunks, b * c + fc_rows);
  hipLaunchKernelGGL((stage_gx_kernel<TS, TO>), planes_fc, dim3(kEwBlock), 0, st, SF(S.a1), y2, SF(S.scsh2), gout, du, TF(T.ds), gx, c, hw, fc_rows, fcj);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

// Forward-only inference (dhd_sfa_stage_infer): running statistics, nothing kept for a backward.
//   UNFUSED   stage_forward itself, its `saved` layout placed at the head of `scratch`: every Plan
//   TWO_PASS  Gemm::cu / Gemm::cuh: mean + weight pack, fc, both BatchNorm tables, conv1 -> y1, conv2 + blend epilogue -> out
//   ONE_PASS  Gemm::cuh: mean + weight pack, fc, both BatchNorm tables, sfa_onepass_h_kernel (sfa_half.h) -> out; no y1
// Every form returns the bytes of stage_forward(training = 0): same kernels up to y1, and the blend epilogue applies
// blend2_bn_kernel's expression (sfa_math.h: blend_gate, blend_out) to the value the unfused conv2 would have stored.
inline bool infer_form_exists(const Plan& p, int form) {
  switch (form) {
    case DHD_SFA_INFER_AUTO: case DHD_SFA_INFER_UNFUSED: return true;
    case DHD_SFA_INFER_TWO_PASS: return p.gemm == Gemm::cu || p.gemm == Gemm::cuh;
    case DHD_SFA_INFER_ONE_PASS: return p.gemm == Gemm::cuh;
    default: return false;
  }
}
inline int infer_resolve(const Plan& p, int form) {
  if (form != DHD_SFA_INFER_AUTO) return form;
  // measured at (4, 2C, 200, 200), alternating windows (profiles/r7/sfa_infer*.json): one-pass beats two-pass by 6 us of 161 at
  // C = 256 and by 30 us of 105 at C = 128 in both half types (two-pass against itself: <= 0.3 us)
  if (infer_form_exists(p, DHD_SFA_INFER_ONE_PASS)) return DHD_SFA_INFER_ONE_PASS;
  return infer_form_exists(p, DHD_SFA_INFER_TWO_PASS) ? DHD_SFA_INFER_TWO_PASS : DHD_SFA_INFER_UNFUSED;
}

// scratch of the two-pass form: the two weight images, the small float32 tables, y1
struct InferLayout {
  size_t wp1, wp2, mean_part, s, h, a1, tab_a, mean1, rstd1, scsh1, tab1, mean2, rstd2, scsh2, tab2, y1, total;
};
inline InferLayout infer_layout(int b, int c, int hw, int r, int storage, bool with_y1) {
  const bool half = storage != DHD_F32;
  const size_t cc = (size_t)c * c;
  InferLayout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  auto f = [&](size_t n) { return take(n * sizeof(float)); };
  L.wp1 = take(half ? 2 * cc : 8 * cc); L.wp2 = take(half ? 2 * cc : 8 * cc);
  L.mean_part = f((size_t)b * 2 * c * kPlaneChunks);
  L.s = f((size_t)b * 2 * c); L.h = f((size_t)b * r); L.a1 = f((size_t)b * c); L.tab_a = f((size_t)b * 3 * c);
  L.mean1 = f(c); L.rstd1 = f(c); L.scsh1 = f(2 * c); L.tab1 = f((size_t)b * 3 * c);
  L.mean2 = f(c); L.rstd2 = f(c); L.scsh2 = f(2 * c); L.tab2 = f((size_t)b * 3 * c);   // tab2: bn2 feeds no GEMM prologue (a sink)
  L.y1 = take(with_y1 ? (size_t)b * c * hw * (half ? 2 : 4) : 0);
  L.total = o;
  return L;
}

inline size_t infer_scratch_total(const Plan& p, int form, int b, int c, int hw, int r) {
  const int f = infer_resolve(p, form);
  if (f != DHD_SFA_INFER_UNFUSED) return infer_layout(b, c, hw, r, p.storage, f == DHD_SFA_INFER_TWO_PASS).total;
  return saved_layout(b, c, hw, r, p.storage).total + scratch_layout(b, c, hw, r, p.storage).total;
}

// sfa_onepass_h_kernel: one workgroup per CU, contiguous tile ranges; as many samples per launch as have their tables in LDS
template <class TS>
int launch_onepass(const TS* x, const OnePassArgs& A, TS* out, int b, int c, int hw, hipStream_t st) {
  const int max_b = onepass_max_batch(c);
  if (max_b < 1) return DHD_EUNSUPPORTED;
  const int nwt = (hw + kCuhTile - 1) / kCuhTile;
  int cus = cu_count();
  if (cus <= 0) cus = 256;
  for (int b0 = 0; b0 < b; b0 += max_b) {
    const int nb = b - b0 < max_b ? b - b0 : max_b;
    const long total = (long)nb * nwt;
    const int grid = (int)(total < cus ? total : cus);
    OnePassArgs a = A;
    a.tab_a += (size_t)b0 * 3 * c;
    a.a1 += (size_t)b0 * c;
    const TS* xi = x + (size_t)b0 * 2 * c * hw;
    TS* oi = out + (size_t)b0 * c * hw;
    const size_t shmem = onepass_lds_bytes(c, nb);
    const int rc = c == 256 ? launch_lds<sfa_onepass_h_kernel<TS, 16>>(dim3(grid), dim3(kOnePassWaves * 64), shmem, kLdsBytes, st, xi, a, oi, hw, nb)
                            : launch_lds<sfa_onepass_h_kernel<TS, 8>>(dim3(grid), dim3(kOnePassWaves * 64), shmem, kLdsBytes, st, xi, a, oi, hw, nb);
    if (rc != DHD_OK) return rc;
  }
  return DHD_OK;
}

template <class TS, class TO>
int stage_infer(const Plan& p, const TS* x, const dhd_sfa_weights* w, TO* out, void* scratch, int b, int c, int hw, int form,
                hipStream_t st) {
  const int r = w->hidden;
  char* sc = static_cast<char*>(scratch);
  form = infer_resolve(p, form);
  if (form == DHD_SFA_INFER_UNFUSED)
    return stage_forward<TS, TO>(p, x, w, out, sc, sc + saved_layout(b, c, hw, r, p.storage).total, b, c, hw, 0, 2, nullptr, st);
  const InferLayout L = infer_layout(b, c, hw, r, p.storage, form == DHD_SFA_INFER_TWO_PASS);
  auto F = [&](size_t off) { return reinterpret_cast<float*>(sc + off); };
  TS* y1 = reinterpret_cast<TS*>(sc + L.y1);
  const size_t cs = (size_t)c * hw;
  void* const dst[4] = {sc + L.wp1, sc + L.wp2, nullptr, nullptr};
  int rc = launch_mean_pack(p, x, w->conv1_w, w->conv2_w, dst, F(L.mean_part), b, c, hw, st);
  if (rc != DHD_OK) return rc;
  hipLaunchKernelGGL(fc_forward_kernel, dim3(b), dim3(kFcBlock), (size_t)(2 * c + r) * sizeof(float), st, F(L.mean_part), w->fc1_w, w->fc1_b,
                     w->fc2_w, w->fc2_b, F(L.s), F(L.h), F(L.a1), F(L.tab_a), c, r, hw, static_cast<int*>(nullptr), 0);
  DHD_LAUNCH_CHECK();
  const BnEvalJob j1 = {w->bn1_w, w->bn1_b, w->bn1_mean, w->bn1_var, w->eps1, F(L.mean1), F(L.rstd1), F(L.scsh1), F(L.tab1)};
  const BnEvalJob j2 = {w->bn2_w, w->bn2_b, w->bn2_mean, w->bn2_var, w->eps2, F(L.mean2), F(L.rstd2), F(L.scsh2), F(L.tab2)};
  hipLaunchKernelGGL(bn_eval_coef2_kernel, dim3(dhd_cdiv(c, kEwBlock), 2), dim3(kEwBlock), 0, st, j1, j2, b, c);
  DHD_LAUNCH_CHECK();
  if (form == DHD_SFA_INFER_ONE_PASS) {
    if constexpr (std::is_same<TS, float>::value) {
      return DHD_EUNSUPPORTED;
    } else {
      const OnePassArgs A = {F(L.tab_a), F(L.tab1), w->conv1_b, w->conv2_b, F(L.a1), F(L.scsh2), reinterpret_cast<const u32x4*>(sc + L.wp1),
                             reinterpret_cast<const u32x4*>(sc + L.wp2)};
      return launch_onepass<TS>(x, A, reinterpret_cast<TS*>(out), b, c, hw, st);
    }
  }
  // y1 = conv1(blend1(x))
  rc = launch_gemm(p, GemmCall<TS>{kConv1, x, x + cs, 2 * cs, c, F(L.tab_a), sc + L.wp1, w->conv1_b, nullptr, nullptr, y1}, b, c, hw, st);
  if (rc != DHD_OK) return rc;
  // out = blend2(x, a, sigmoid(bn2(conv2(relu(bn1(y1))))))
  return launch_gemm(p, GemmCall<TS>{kConv2Blend, y1, nullptr, cs, c, F(L.tab1), sc + L.wp2, w->conv2_b, nullptr, nullptr, nullptr, nullptr,
                                     nullptr, CuBlend{x, F(L.a1), F(L.scsh2), out}, w->io_dtype},
                     b, c, hw, st);
}

// The driver instance of a call: storage type, and on float32 storage the I/O type
template <class F>
int with_types(const Plan& p, int io_dtype, F&& f) {
  if (p.storage == DHD_F16) return f((_Float16*)nullptr, (_Float16*)nullptr);
  if (p.storage == DHD_BF16) return f((__bf16*)nullptr, (__bf16*)nullptr);
  if (io_dtype == DHD_F16) return f((float*)nullptr, (_Float16*)nullptr);
  if (io_dtype == DHD_BF16) return f((float*)nullptr, (__bf16*)nullptr);
  return f((float*)nullptr, (float*)nullptr);
}

static int stage_forward_entry(const void* x, const dhd_sfa_weights* w, void* out, void* saved, void* scratch, int b, int c, int hw,
                               int lo, int hi, double* sync, void* stream) {
  if (!x || !w || !saved || !scratch || b <= 0 || (hi == 2 && !out)) return DHD_EINVAL;
  if (!dhd_aligned(16, x, out, saved, scratch)) return DHD_EINVAL;   // 16-byte vector accesses in every kernel of the stage
  if (!stage_supported(c, hw) || w->hidden <= 0) return DHD_EUNSUPPORTED;
  if (!w->fc1_w || !w->fc1_b || !w->fc2_w || !w->fc2_b || !w->conv1_w || !w->conv1_b || !w->bn1_w || !w->bn1_b || !w->conv2_w ||
      !w->conv2_b || !w->bn2_w || !w->bn2_b)
    return DHD_EINVAL;
  if (!w->training && (!w->bn1_mean || !w->bn1_var || !w->bn2_mean || !w->bn2_var)) return DHD_EINVAL;
  Plan p;
  if (int rc = make_plan(w, c, hw, &p); rc != DHD_OK) return rc;
  return with_types(p, w->io_dtype, [&](auto* ts, auto* to) {
    using TS = std::remove_pointer_t<decltype(ts)>;
    using TO = std::remove_pointer_t<decltype(to)>;
    return stage_forward<TS, TO>(p, static_cast<const TS*>(x), w, static_cast<TO*>(out), saved, scratch, b, c, hw, lo, hi, sync,
                                 dhd_stream(stream));
  });
}

static int stage_backward_entry(const void* x, const dhd_sfa_weights* w, const void* saved, const void* gout, void* gx,
                                const dhd_sfa_grads* grads, void* scratch, int b, int c, int hw, int lo, int hi, double* sync,
                                void* stream) {
  if (!x || !w || !saved || !gout || !grads || !scratch || b <= 0 || (hi == 2 && !gx)) return DHD_EINVAL;
  if (!dhd_aligned(16, x, saved, gout, gx, scratch)) return DHD_EINVAL;
  if (!stage_supported(c, hw) || w->hidden <= 0) return DHD_EUNSUPPORTED;
  if (!grads->fc1_w || !grads->fc1_b || !grads->fc2_w || !grads->fc2_b || !grads->conv1_w || !grads->conv1_b || !grads->bn1_w ||
      !grads->bn1_b || !grads->conv2_w || !grads->conv2_b || !grads->bn2_w || !grads->bn2_b)
    return DHD_EINVAL;
  Plan p;
  if (int rc = make_plan(w, c, hw, &p); rc != DHD_OK) return rc;
  return with_types(p, w->io_dtype, [&](auto* ts, auto* to) {
    using TS = std::remove_pointer_t<decltype(ts)>;
    using TO = std::remove_pointer_t<decltype(to)>;
    return stage_backward<TS, TO>(p, static_cast<const TS*>(x), w, saved, static_cast<const TO*>(gout), static_cast<TO*>(gx), grads,
                                  scratch, b, c, hw, lo, hi, sync, dhd_stream(stream));
  });
}

static int stage_infer_entry(const void* x, const dhd_sfa_weights* w, void* out, void* scratch, int b, int c, int hw, int form,
                             void* stream) {
  if (!x || !w || !out || !scratch || b <= 0 || form < DHD_SFA_INFER_AUTO || form > DHD_SFA_INFER_ONE_PASS) return DHD_EINVAL;
  if (!dhd_aligned(16, x, out, scratch)) return DHD_EINVAL;
  if (!stage_supported(c, hw) || w->hidden <= 0) return DHD_EUNSUPPORTED;
  if (!w->fc1_w || !w->fc1_b || !w->fc2_w || !w->fc2_b || !w->conv1_w || !w->conv1_b || !w->bn1_w || !w->bn1_b || !w->conv2_w ||
      !w->conv2_b || !w->bn2_w || !w->bn2_b)
    return DHD_EINVAL;
  if (w->training) return DHD_EINVAL;   // batch statistics belong to dhd_sfa_stage_forward
  if (!w->bn1_mean || !w->bn1_var || !w->bn2_mean || !w->bn2_var) return DHD_EINVAL;
  Plan p;
  if (int rc = make_plan(w, c, hw, &p); rc != DHD_OK) return rc;
  if (!infer_form_exists(p, form)) return DHD_EUNSUPPORTED;
  return with_types(p, w->io_dtype, [&](auto* ts, auto* to) {
    using TS = std::remove_pointer_t<decltype(ts)>;
    using TO = std::remove_pointer_t<decltype(to)>;
    return stage_infer<TS, TO>(p, static_cast<const TS*>(x), w, static_cast<TO*>(out), scratch, b, c, hw, form, dhd_stream(stream));
  });
}

// the Plan of a (storage type, precision) without a weights struct of the caller's
static int infer_plan(int c, int hw, int storage_dtype, int gemm, Plan* p) {
  dhd_sfa_weights w = {};
  w.gemm = gemm;
  w.storage_dtype = w.io_dtype = storage_dtype;
  if (!stage_supported(c, hw)) return DHD_EUNSUPPORTED;
  return make_plan(&w, c, hw, p);
}

}  // namespace

extern "C" {


int dhd_sfa_stage_supported(int c, int hw) { return stage_supported(c, hw) ? 1 : 0; }

size_t dhd_sfa_stage_saved_bytes(int b, int c, int hw, int hidden) {
  if (b <= 0 || hidden <= 0 || !stage_supported(c, hw)) return 0;
  return saved_layout(b, c, hw, hidden, DHD_F32).total;
}

size_t dhd_sfa_stage_scratch_bytes(int b, int c, int hw, int hidden) {
  if (b <= 0 || hidden <= 0 || !stage_supported(c, hw)) return 0;
  return scratch_layout(b, c, hw, hidden, DHD_F32).total;
}

int dhd_sfa_stage_half_storage_supported(int c, int hw) { return half_storage_supported(c, hw) ? 1 : 0; }

int dhd_sfa_stage_workspace_bytes(int b, int c, int hw, int hidden, int storage_dtype, size_t* saved_bytes, size_t* scratch_bytes) {
  if (b <= 0 || hidden <= 0 || !saved_bytes || !scratch_bytes) return DHD_EINVAL;
  if (storage_dtype == DHD_F32) {
    if (!stage_supported(c, hw)) return DHD_EUNSUPPORTED;
  } else {
    if (storage_dtype != DHD_F16 && storage_dtype != DHD_BF16) return DHD_EINVAL;
    if (!half_storage_supported(c, hw)) return DHD_EUNSUPPORTED;
  }
  *saved_bytes = saved_layout(b, c, hw, hidden, storage_dtype).total;
  *scratch_bytes = scratch_layout(b, c, hw, hidden, storage_dtype).total;
  return DHD_OK;
}

int dhd_sfa_stage_forward(const void* x, const dhd_sfa_weights* w, void* out, void* saved, void* scratch, int b, int c, int hw,
                          void* stream) {
  return stage_forward_entry(x, w, out, saved, scratch, b, c, hw, 0, 2, nullptr, stream);
}

int dhd_sfa_stage_backward(const void* x, const dhd_sfa_weights* w, const void* saved, const void* gout, void* gx,
                           const dhd_sfa_grads* grads, void* scratch, int b, int c, int hw, void* stream) {
  return stage_backward_entry(x, w, saved, gout, gx, grads, scratch, b, c, hw, 0, 2, nullptr, stream);
}

int dhd_sfa_stage_forward_phase(const void* x, const dhd_sfa_weights* w, void* out, void* saved, void* scratch, int b, int c, int hw,
                                int phase, double* sync_sums, void* stream) {
  if (phase < 0 || phase > 2 || !sync_sums || (reinterpret_cast<uintptr_t>(sync_sums) & 7)) return DHD_EINVAL;
  return stage_forward_entry(x, w, out, saved, scratch, b, c, hw, phase, phase, sync_sums, stream);
}

int dhd_sfa_stage_backward_phase(const void* x, const dhd_sfa_weights* w, const void* saved, const void* gout, void* gx,
                                 const dhd_sfa_grads* grads, void* scratch, int b, int c, int hw, int phase, double* sync_sums,
                                 void* stream) {
  if (phase < 0 || phase > 2 || !sync_sums || (reinterpret_cast<uintptr_t>(sync_sums) & 7)) return DHD_EINVAL;
  return stage_backward_entry(x, w, saved, gout, gx, grads, scratch, b, c, hw, phase, phase, sync_sums, stream);
}

int dhd_sfa_stage_infer_supported(int c, int hw, int storage_dtype, int gemm, int form) {
  Plan p;
  return infer_plan(c, hw, storage_dtype, gemm, &p) == DHD_OK && infer_form_exists(p, form) ? 1 : 0;
}

int dhd_sfa_stage_infer_scratch_bytes(int b, int c, int hw, int hidden, int storage_dtype, int gemm, int form, size_t* bytes) {
  if (b <= 0 || hidden <= 0 || !bytes || form < DHD_SFA_INFER_AUTO || form > DHD_SFA_INFER_ONE_PASS) return DHD_EINVAL;
  Plan p;
  if (int rc = infer_plan(c, hw, storage_dtype, gemm, &p); rc != DHD_OK) return rc;
  if (!infer_form_exists(p, form)) return DHD_EUNSUPPORTED;
  *bytes = infer_scratch_total(p, form, b, c, hw, hidden);
  return DHD_OK;
}

int dhd_sfa_stage_infer(const void* x, const dhd_sfa_weights* w, void* out, void* scratch, int b, int c, int hw, int form,
                        void* stream) {
  return stage_infer_entry(x, w, out, scratch, b, c, hw, form, stream);
}

}  // extern "C"
