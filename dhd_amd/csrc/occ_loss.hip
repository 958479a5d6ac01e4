// Occupancy-head losses of DHD's `predictor` in two streaming passes, for gfx950.
//
// Reference: models/dense_heads/occ_head.py:102-139 (predictor.loss) = class-balanced, camera-masked
// softmax cross entropy (models/losses/cross_entropy_loss.py:12-63) + sem_scal_loss_with_mask
// (models/losses/semkitti_loss.py:171-226) + geo_scal_loss_with_mask (:136-169), over
// M = B*200*200*16 voxels x 18 classes.  In eager PyTorch that is a softmax, ~17 masked gathers with a
// device->host sync each (`if torch.sum(..) > 0`), and their autograd mirror images.
//
// Every term is a function of a few global sums over the valid voxels v (camera mask & label != 255):
//   T_i = #{v: t_v = i}     P_i = sum_v p_vi     N_i = sum_{v: t_v = i} p_vi     CE = sum_v w_t (-log p_vt)
// (e.g. the specificity numerator sum (1-p_i)(1-[t=i]) = n_valid - P_i - T_i + N_i).  So:
//   pass 1 (occ_loss_sums)  reads logits/labels/mask once, softmax in registers, 56 block-reduced sums;
//   occ_loss_finalize       double-precision totals -> the three losses;
//   pass 2 (occ_loss_grad)  re-reads the logits, recomputes the softmax and writes
//                           dL/dz_k = valid p_k (a_k + b_k [t=k] - sum_j p_j a_j - p_t b_t) + ce (p_k - [t=k]),
//                           a_i = dL/dP_i, b_i = dL/dN_i evaluated per block from the stored totals.
// Edges.  No valid voxel (an empty camera mask, every label ignored): cross entropy and sem scal are 0 / 0 = NaN and geo scal is
// 3 x -log(1e-5), as the reference's formulas give; every gradient is 0.  `P_i > 0` (whether class i's precision term exists) is
// decided on the float32 sums, as in the reference: a class whose probability underflows in every valid voxel has none.  A
// logit of -inf is a probability of 0.  NaN: a NaN logit in a valid voxel makes all three losses NaN; an excluded voxel's
// logits are never read (the reference multiplies its cross entropy by 0 and would return NaN there).
// Traffic: 2 x 72 B read + 72 B written per voxel (+2 B labels/mask each pass); no (M,18) temporaries.
// Logit tiles go through LDS so that global accesses are 16-byte coalesced although a voxel's 18 logits
// are 72 contiguous bytes: a thread reads its voxel as nine conflict-free ds_read_b64.
#include "occ_loss_math.h"

namespace {

using dhd::f32x4;

// the softmax, inverse_sigmoid's steps, occ_loss_finalize and the gradient's coefficients: occ_loss_math.h, shared with occ_head.hip
constexpr int K = kLossK;          // classes (Occ3D-nuScenes: 17 semantic + free)
constexpr int kBlock = 256;        // one voxel per thread per tile
constexpr int kSums = kLossSums;   // T, P, N per class; CE; n_valid
constexpr int kMaxBlocks = 1024;
constexpr int kFinBlock = kLossFinBlock;

// copy tile [first voxel v0, n_in voxels) of the (M,18) matrix into LDS with 16-byte accesses
__device__ __forceinline__ void load_tile(const float* __restrict__ logits, long v0, int n_in, float* tile) {
  const f32x4* src = reinterpret_cast<const f32x4*>(logits + v0 * K);  // v0 is a multiple of kBlock: 16-byte aligned
  const int n4 = (n_in * K) >> 2, rest = (n_in * K) & 3;
  for (int i = threadIdx.x; i < n4; i += kBlock) reinterpret_cast<f32x4*>(tile)[i] = src[i];
  if (threadIdx.x < rest) tile[4 * n4 + threadIdx.x] = logits[v0 * K + 4 * n4 + threadIdx.x];
}

__global__ __launch_bounds__(kBlock) void occ_loss_sums(const float* __restrict__ logits, const uint8_t* __restrict__ labels,
                                                        const uint8_t* __restrict__ mask, const float* __restrict__ cw, long m,
                                                        int ignore, float* __restrict__ partial) {
  __shared__ float tile[kBlock * K];
  __shared__ float red[kBlock / DHD_WAVE][kSums];
  float accP[K], accN[K], accT[K], ce = 0.f, nv = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) accP[k] = accN[k] = accT[k] = 0.f;
  const long n_tiles = (m + kBlock - 1) / kBlock;
  for (long tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    const long v0 = tl * kBlock;
    const int n_in = (int)min((long)kBlock, m - v0);
    __syncthreads();
    load_tile(logits, v0, n_in, tile);
    __syncthreads();
    if ((int)threadIdx.x < n_in) {
      const long v = v0 + threadIdx.x;
      const int t = labels[v];
      const bool cam = mask[v] != 0;
      const bool valid = cam && t != ignore;
      if (valid) {
        Voxel x;
        softmax18(tile + threadIdx.x * K, t, x);
        nv += 1.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          accP[k] += x.p[k];
          if (k == t) {
            accN[k] += x.p[k];
            accT[k] += 1.f;
          }
        }
        if (t < K) ce += cw[t] * (x.lse - x.zt);
      }
    }
  }
  // block reduction of the 56 sums
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float a = wave_sum_bcast(accT[k]), b = wave_sum_bcast(accP[k]), c = wave_sum_bcast(accN[k]);
    if (lane == 0) {
      red[wv][k] = a;
      red[wv][K + k] = b;
      red[wv][2 * K + k] = c;
    }
  }
  {
    const float a = wave_sum_bcast(ce), b = wave_sum_bcast(nv);
    if (lane == 0) {
      red[wv][3 * K] = a;
      red[wv][3 * K + 1] = b;
    }
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    float s = 0.f;
    for (int w = 0; w < kBlock / DHD_WAVE; ++w) s += red[w][threadIdx.x];
    partial[(size_t)blockIdx.x * kSums + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(kBlock) void occ_loss_grad(const float* __restrict__ logits, const uint8_t* __restrict__ labels,
                                                        const uint8_t* __restrict__ mask, const float* __restrict__ cw, long m,
                                                        int ignore, int non_empty, const double* __restrict__ totals,
                                                        const float* __restrict__ gl, float* __restrict__ grad) {
  __shared__ float tile[kBlock * K];
  __shared__ float sa[K], sb[K], sce;
  // a_i = dL/dP_i, b_i = dL/dN_i from the totals and the upstream gradients gl[0..2]
  loss_coefficients(totals, gl, cw, non_empty, threadIdx.x, sa, sb, &sce);
  __syncthreads();
  float a[K], bq[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { a[k] = sa[k]; bq[k] = sb[k]; }
  const float ce_scale = sce;

  const long n_tiles = (m + kBlock - 1) / kBlock;
  for (long tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    const long v0 = tl * kBlock;
    const int n_in = (int)min((long)kBlock, m - v0);
    __syncthreads();
    load_tile(logits, v0, n_in, tile);
    __syncthreads();
    if ((int)threadIdx.x < n_in) {
      const long v = v0 + threadIdx.x;
      const int t = labels[v];
      const bool valid = mask[v] != 0 && t != ignore;
      float* row = tile + threadIdx.x * K;
      float d[K];
      if (valid) {
        Voxel x;
        softmax18(row, t, x);
        float bt = 0.f, wt = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (k == t) { bt = bq[k]; wt = cw[k]; }
        loss_grad18(x, t, a, bt, wt, ce_scale, d);
      } else {
#pragma unroll
        for (int k = 0; k < K; ++k) d[k] = 0.f;
      }
#pragma unroll
      for (int q = 0; q < K / 2; ++q) reinterpret_cast<float2*>(row)[q] = make_float2(d[2 * q], d[2 * q + 1]);
    }
    __syncthreads();
    {
      f32x4* dst = reinterpret_cast<f32x4*>(grad + v0 * K);
      const int n4 = (n_in * K) >> 2, rest = (n_in * K) & 3;
      for (int i = threadIdx.x; i < n4; i += kBlock) __builtin_nontemporal_store(reinterpret_cast<const f32x4*>(tile)[i], dst + i);
      if ((int)threadIdx.x < rest) grad[v0 * K + 4 * n4 + threadIdx.x] = tile[4 * n4 + threadIdx.x];
    }
  }
}

inline int n_blocks_for(long m) {
  const long tiles = (m + kBlock - 1) / kBlock;
  return (int)(tiles < kMaxBlocks ? tiles : kMaxBlocks);
}

}  // namespace

extern "C" {

size_t dhd_occ_loss_workspace_bytes(void) { return (size_t)kMaxBlocks * kSums * sizeof(float) + 64 * sizeof(double); }

int dhd_occ_loss_forward(const float* logits, const uint8_t* labels, const uint8_t* mask, const float* class_weight, int64_t n_voxels,
                         int n_classes, int ignore_index, int non_empty_idx, float* losses, void* workspace, void* stream) {
  if (!logits || !labels || !mask || !class_weight || !losses || !workspace || n_voxels <= 0) return DHD_EINVAL;
  if (n_classes != K || non_empty_idx < 0 || non_empty_idx >= K) return DHD_EUNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(logits) & 15) != 0) return DHD_EINVAL;
  hipStream_t st = dhd_stream(stream);
  float* partial = static_cast<float*>(workspace);
  double* totals = reinterpret_cast<double*>(partial + (size_t)kMaxBlocks * kSums);
  const int nb = n_blocks_for(n_voxels);
  hipLaunchKernelGGL(occ_loss_sums, dim3(nb), dim3(kBlock), 0, st, logits, labels, mask, class_weight, (long)n_voxels, ignore_index,
                     partial);
  hipLaunchKernelGGL(occ_loss_finalize, dim3(1), dim3(kFinBlock), 0, st, partial, nb, class_weight, non_empty_idx, totals, losses);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

int dhd_occ_loss_backward(const float* logits, const uint8_t* labels, const uint8_t* mask, const float* class_weight, int64_t n_voxels,
                          int n_classes, int ignore_index, int non_empty_idx, const float* grad_losses, const void* workspace,
                          float* grad_logits, void* stream) {
  if (!logits || !labels || !mask || !class_weight || !grad_losses || !workspace || !grad_logits || n_voxels <= 0) return DHD_EINVAL;
  if (n_classes != K || non_empty_idx < 0 || non_empty_idx >= K) return DHD_EUNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(logits) & 15) != 0 || (reinterpret_cast<uintptr_t>(grad_logits) & 15) != 0) return DHD_EINVAL;
  hipStream_t st = dhd_stream(stream);
  const float* partial = static_cast<const float*>(workspace);
  const double* totals = reinterpret_cast<const double*>(partial + (size_t)kMaxBlocks * kSums);
  hipLaunchKernelGGL(occ_loss_grad, dim3(n_blocks_for(n_voxels)), dim3(kBlock), 0, st, logits, labels, mask, class_weight,
                     (long)n_voxels, ignore_index, non_empty_idx, totals, grad_losses, grad_logits);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Evaluation side of the same logits: predictor.get_occ (occ_head.py:141-153: softmax -> argmax) and
// Metric_mIoU.hist_info (core/evaluation/occ_metrics.py:79-104: 18x18 confusion counts over the
// camera-visible voxels with a label in [0, 18)), in one pass over the (M,18) logits.
// argmax of the logits = argmax of their softmax (first maximum wins); the two can differ only where
// the two largest probabilities round to the same float.  Equal logits, +0 against -0 and a row of -inf give class 0 (the
// comparison is a strict >); which class a row with a NaN at k != 0 gets is unspecified.
// ------------------------------------------------------------------------------------------------
namespace {

__global__ __launch_bounds__(kBlock) void occ_argmax_hist(const float* __restrict__ logits, const uint8_t* __restrict__ labels,
                                                          const uint8_t* __restrict__ mask, long m, uint8_t* __restrict__ pred,
                                                          unsigned long long* __restrict__ hist) {
  __shared__ float tile[kBlock * K];
  __shared__ unsigned cnt[K * K];
  for (int i = threadIdx.x; i < K * K; i += kBlock) cnt[i] = 0;
  const long n_tiles = (m + kBlock - 1) / kBlock;
  for (long tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    const long v0 = tl * kBlock;
    const int n_in = (int)min((long)kBlock, m - v0);
    __syncthreads();
    load_tile(logits, v0, n_in, tile);
    __syncthreads();
    if ((int)threadIdx.x < n_in) {
      const float* row = tile + threadIdx.x * K;
      float best = row[0];
      int arg = 0;
#pragma unroll
      for (int k = 1; k < K; ++k) {
        const float z = row[k];
        if (z > best) { best = z; arg = k; }
      }
      const long v = v0 + threadIdx.x;
      if (pred) pred[v] = (uint8_t)arg;
      if (hist) {
        const int t = labels[v];
        if (t < K && (mask == nullptr || mask[v] != 0)) atomicAdd(&cnt[t * K + arg], 1u);
      }
    }
  }
  __syncthreads();
  if (hist)
    for (int i = threadIdx.x; i < K * K; i += kBlock)
      if (cnt[i]) atomicAdd(&hist[i], (unsigned long long)cnt[i]);
}

}  // namespace

extern "C" int dhd_occ_argmax_hist(const float* logits, const uint8_t* labels, const uint8_t* mask, int64_t n_voxels, int n_classes,
                                   uint8_t* pred, int64_t* hist, void* stream) {
  if (!logits || n_voxels <= 0 || (!pred && !hist) || (hist && !labels)) return DHD_EINVAL;
  if (n_classes != K) return DHD_EUNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(logits) & 15) != 0) return DHD_EINVAL;
  hipLaunchKernelGGL(occ_argmax_hist, dim3(n_blocks_for(n_voxels)), dim3(kBlock), 0, dhd_stream(stream), logits, labels, mask,
                     (long)n_voxels, pred, reinterpret_cast<unsigned long long*>(hist));
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}
