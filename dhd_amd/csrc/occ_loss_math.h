// The arithmetic the occupancy-head losses share between occ_loss.hip (the two streaming passes over logits in memory) and
// occ_head_loss.h (the same sums and the same gradient on logits that are still in the head's registers): the 18-way softmax,
// inverse_sigmoid's steps, the finalize launch (56 double totals -> three losses) and the coefficients a_i = dL/dP_i,
// b_i = dL/dN_i of the gradient.  occ_loss.hip's header comment derives the formulas.  Everything is in an anonymous namespace:
// each translation unit that includes this file has its own copy of the finalize kernel.
#pragma once
#include "vec16.h"

namespace {

constexpr int kLossK = 18;                  // classes (Occ3D-nuScenes: 17 semantic + free)
constexpr int kLossSums = 3 * kLossK + 2;   // T, P, N per class; CE; n_valid
constexpr int kLossFinBlock = 1024;         // finalize: 64 columns x 16 row phases

struct Voxel {
  float p[kLossK];
  float lse;   // log sum exp (shifted back)
  float zt;    // logit of the label (if t < K)
};

// the softmax of 18 logits held in registers
__device__ __forceinline__ void softmax18_vals(const float (&z)[kLossK], int t, Voxel& v) {
  float mx = z[0];
#pragma unroll
  for (int k = 1; k < kLossK; ++k) mx = fmaxf(mx, z[k]);
  float s = 0.f;
  v.zt = 0.f;
#pragma unroll
  for (int k = 0; k < kLossK; ++k) {
    if (k == t) v.zt = z[k];
    v.p[k] = __expf(z[k] - mx);
    s += v.p[k];
  }
  const float inv = 1.0f / s;
#pragma unroll
  for (int k = 0; k < kLossK; ++k) v.p[k] *= inv;
  v.lse = mx + __logf(s);
}

__device__ __forceinline__ void softmax18(const float* row, int t, Voxel& v) {
  float z[kLossK];
#pragma unroll
  for (int q = 0; q < kLossK / 2; ++q) {
    const float2 two = reinterpret_cast<const float2*>(row)[q];
    z[2 * q] = two.x;
    z[2 * q + 1] = two.y;
  }
  softmax18_vals(z, t, v);
}

// dL/dz_k of one valid voxel with label t from its softmax, the coefficients a, b (b_t and w_t already picked) and the
// cross-entropy scale: p_k (a_k + b_k [t = k] - sum_j p_j a_j - p_t b_t) + ce_scale w_t (p_k - [t = k])
template <class A>
__device__ __forceinline__ void loss_grad18(const Voxel& x, int t, const A& a, float bt, float wt, float ce_scale, float (&d)[kLossK]) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < kLossK; ++k) s = fmaf(x.p[k], a[k], s);
  float pt = 0.f;
#pragma unroll
  for (int k = 0; k < kLossK; ++k) if (k == t) pt = x.p[k];
  s = fmaf(pt, bt, s);
  const float cs = ce_scale * wt;
#pragma unroll
  for (int k = 0; k < kLossK; ++k) {
    const float hit = k == t ? 1.f : 0.f;
    d[k] = x.p[k] * (a[k] + hit * bt - s) + cs * (x.p[k] - hit);
  }
}

// inverse_sigmoid (semkitti_loss.py:8-16) moves the float32 value of x into [1e-5, 1-1e-5) by two `while` loops that step by
// 1e-5.  Which steps are taken is decided as the reference decides it, on float32 values against float32 thresholds: one step
// for x in [1-1e-5, 1) -- and TWO for x == 1.0f (a class every voxel of which is predicted with p = 1: 1.0f - 1e-5 rounds to
// float32(1 - 1e-5) itself, which is not below it) -- one step up for x < 1e-5.  The steps themselves are taken in double.  The
// loops are bounded (two steps down, one up: all that a ratio in [0, 1] can take); a NaN takes none and passes through.
__device__ __forceinline__ double inverse_sigmoid_arg(double ratio) {
  double x = (double)(float)ratio;
  for (int i = 0; i < 2 && (float)x >= 0.99999f; ++i) x -= 1e-5;
  if ((float)x < 1e-5f) x += 1e-5;
  return x;
}

// binary_cross_entropy_with_logits(inverse_sigmoid(x), 1) = -log(x')
__device__ __forceinline__ double nll_clamped(double x) { return -log(inverse_sigmoid_arg(x)); }

// derivative of nll_clamped(num/den) with respect to num and den
__device__ __forceinline__ void d_nll(double num, double den, double* d_num, double* d_den) {
  const double x = inverse_sigmoid_arg(num / den);
  *d_num = -1.0 / (x * den);
  *d_den = num / (x * den * den);
}

// partial (n_blocks, 56) float32 -> totals[0..55] = T, P, N, CE, n_valid (double);  losses[0..2] = cross entropy, sem scal, geo scal
__global__ __launch_bounds__(kLossFinBlock) void occ_loss_finalize(const float* __restrict__ partial, int n_blocks, const float* __restrict__ cw,
                                                                int non_empty, double* __restrict__ totals, float* __restrict__ losses) {
  constexpr int K = kLossK, kSums = kLossSums;
  __shared__ double tot[kSums];
  constexpr int kPh = kLossFinBlock / 64;
  __shared__ double ph[kPh][64];
  {
    // thread = (column, row phase): 16 phases x four independent accumulators keep the loads in flight
    const int col = threadIdx.x & 63, phase = threadIdx.x >> 6;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (col < kSums) {
      int b = phase;
      for (; b + 3 * kPh < n_blocks; b += 4 * kPh) {
        s0 += (double)partial[(size_t)b * kSums + col];
        s1 += (double)partial[(size_t)(b + kPh) * kSums + col];
        s2 += (double)partial[(size_t)(b + 2 * kPh) * kSums + col];
        s3 += (double)partial[(size_t)(b + 3 * kPh) * kSums + col];
      }
      for (; b < n_blocks; b += kPh) s0 += (double)partial[(size_t)b * kSums + col];
    }
    ph[phase][col] = (s0 + s1) + (s2 + s3);
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    double s = 0.0;
    for (int q = 0; q < kPh; ++q) s += ph[q][threadIdx.x];
    tot[threadIdx.x] = s;
    totals[threadIdx.x] = s;
  }
  __syncthreads();
  // per-class terms in parallel (each is up to three double-precision logs), then one thread adds them up
  __shared__ double term[K + 3];
  const double* T = tot;
  const double* P = tot + K;
  const double* N = tot + 2 * K;
  const double nv = tot[3 * K + 1];
  const int e = non_empty;
  if (threadIdx.x < K - 1) {
    const int i = threadIdx.x;
    double sem = 0.0;
    if (T[i] > 0.0) {
      if (P[i] > 0.0) sem += nll_clamped(N[i] / (P[i] + 1e-5));
      sem += nll_clamped(N[i] / (T[i] + 1e-5));
      const double neg = nv - T[i];
      if (neg > 0.0) sem += nll_clamped((nv - P[i] - T[i] + N[i]) / (neg + 1e-5));
    }
    term[i] = sem;
  } else if (threadIdx.x >= 64 && threadIdx.x < 67) {
    const double inter = (nv - T[e]) - (P[e] - N[e]);
    const int q = threadIdx.x - 64;
    term[K + q] = q == 0 ? nll_clamped(inter / ((nv - P[e]) + 1e-5))
                : q == 1 ? nll_clamped(inter / ((nv - T[e]) + 1e-5)) : nll_clamped(N[e] / (T[e] + 1e-5));
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double avg = 0.0, sem = 0.0, count = 0.0;
  for (int i = 0; i < K; ++i) avg += T[i] * (double)cw[i];
  for (int i = 0; i < K - 1; ++i) {
    sem += term[i];
    count += T[i] > 0.0 ? 1.0 : 0.0;
  }
  losses[0] = (float)(tot[3 * K] / avg);
  losses[1] = (float)(sem / count);
  losses[2] = (float)(term[K] + term[K + 1] + term[K + 2]);
}

// a_i = dL/dP_i -> sa[i], b_i = dL/dN_i -> sb[i] (threads 0..17) and the cross-entropy scale gl[0] / sum_i T_i w_i -> *sce
// (thread 0), from the stored totals and the upstream gradients gl[0..2].  The caller synchronises before it reads them.
__device__ __forceinline__ void loss_coefficients(const double* __restrict__ totals, const float* __restrict__ gl, const float* __restrict__ cw,
                                                  int non_empty, int tid, float* sa, float* sb, float* sce) {
  constexpr int K = kLossK;
  if (tid < K) {
    const int i = tid;
    const double* T = totals;
    const double* P = totals + K;
    const double* N = totals + 2 * K;
    const double nv = totals[3 * K + 1];
    double a = 0.0, b = 0.0;
    if (i < K - 1 && T[i] > 0.0) {
      double count = 0.0;
      for (int j = 0; j < K - 1; ++j) count += T[j] > 0.0 ? 1.0 : 0.0;
      const double g = (double)gl[1] / count;
      double dn, dd;
      if (P[i] > 0.0) {
        d_nll(N[i], P[i] + 1e-5, &dn, &dd);
        b += g * dn;
        a += g * dd;
      }
      d_nll(N[i], T[i] + 1e-5, &dn, &dd);
      b += g * dn;
      const double neg = nv - T[i];
      if (neg > 0.0) {
        d_nll(nv - P[i] - T[i] + N[i], neg + 1e-5, &dn, &dd);
        a -= g * dn;
        b += g * dn;
      }
    }
    if (i == non_empty) {
      const double g = (double)gl[2];
      const double inter = (nv - T[i]) - (P[i] - N[i]);
      double dn, dd;
      d_nll(inter, (nv - P[i]) + 1e-5, &dn, &dd);  // precision: inter and the denominator both fall with P
      a += g * (-dn - dd);
      b += g * dn;
      d_nll(inter, (nv - T[i]) + 1e-5, &dn, &dd);  // recall
      a -= g * dn;
      b += g * dn;
      d_nll(N[i], T[i] + 1e-5, &dn, &dd);          // specificity
      b += g * dn;
    }
    sa[i] = (float)a;
    sb[i] = (float)b;
  }
  if (tid == 0) {
    double avg = 0.0;
    for (int i = 0; i < K; ++i) avg += totals[i] * (double)cw[i];
    *sce = (float)((double)gl[0] / avg);
  }
}

}  // namespace
