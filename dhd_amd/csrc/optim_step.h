// The tail of the training step (dhd_amd/capi_optim/dhd_amd_optim.h): GradScaler.unscale_, clip_grad_norm_, AdamW.step, the
// half weight refresh and the weight EMA are five sweeps over the parameter set in torch (up to 16.5 passes over 147 M values for
// DHD-S); here they are one read of the gradients for the global norm and one sweep that reads g, p, m, v, ema and writes p, m,
// v, ema and the half copies.  Included by ema.hip behind ema1(), whose two roundings the EMA here repeats: the chunk walk is
// ema_update_kernel's.  Everything a replay of a captured step must see anew -- the loss scale, the clip coefficient, the step
// counts and what is derived from them, the EMA's decay pair -- is read from device memory.
#pragma once
// (The surface's header names "dhd_amd.h" as a caller with include/ on its path does, which this directory's build has not: the
// macros and structs it declares are repeated here, and tests/test_optim_capi.py holds the two to each other.)
#ifndef DHD_AMD_OPTIM_H
#define DHDW_OPTIM_CHUNK 65536
#define DHDW_OPTIM_RECORD_AT 0
#define DHDW_OPTIM_MULT_AT 16
#define DHDW_OPTIM_FOUND_AT 20
#define DHDW_OPTIM_PARTIALS_AT 64
typedef struct dhdw_optim_chunk {
  uint64_t p, g, exp_avg, exp_avg_sq, ema, half;
  int32_t len;
  int32_t group;
  int32_t half_dtype;
  int32_t slot;
} dhdw_optim_chunk;
typedef struct dhdw_optim_group {
  double lr, beta1, beta2, eps, weight_decay;
} dhdw_optim_group;
typedef struct dhdw_optim_tables {
  const dhdw_optim_chunk* chunks;
  const dhdw_optim_group* groups;
  const int32_t* slot_group;
  float* steps;
  float* slot_scalars;
  float* group_scalars;
  const float* decay_pair;
  float* scale;
  int32_t* growth_tracker;
  int32_t n_chunks, n_groups, n_slots;
  int32_t n_partials;
} dhdw_optim_tables;
extern "C" {
size_t dhdw_optim_workspace_bytes(int n_chunks);
int dhdw_optim_grad_norm(const dhdw_optim_tables* t, void* workspace, size_t workspace_bytes, void* stream);
int dhdw_optim_finalize(const dhdw_optim_tables* t, float max_norm, float growth_factor, float backoff_factor, int growth_interval,
                        void* workspace, size_t workspace_bytes, void* stream);
int dhdw_optim_adamw_update(const dhdw_optim_tables* t, const void* workspace, size_t workspace_bytes, void* stream);
}
#endif
#include "vec16.h"

namespace {

constexpr int kOptBlock = 256;

using dhd::f32x2;
using dhd::u32x2;

struct OptimWorkspace {
  float* record;      // {norm, coef, found_inf, scale}
  float* mult;        // inv_scale * coef
  int* found;
  double* partial;    // n_partials
  int* flag;          // n_partials
};

__host__ __device__ __forceinline__ OptimWorkspace optim_workspace(void* ws, int n_partials) {
  char* b = static_cast<char*>(ws);
  OptimWorkspace w;
  w.record = reinterpret_cast<float*>(b + DHDW_OPTIM_RECORD_AT);
  w.mult = reinterpret_cast<float*>(b + DHDW_OPTIM_MULT_AT);
  w.found = reinterpret_cast<int*>(b + DHDW_OPTIM_FOUND_AT);
  w.partial = reinterpret_cast<double*>(b + DHDW_OPTIM_PARTIALS_AT);
  w.flag = reinterpret_cast<int*>(w.partial + n_partials);
  return w;
}

// GradScaler.unscale_'s factor: the reciprocal taken in double, rounded to float32
__device__ __forceinline__ float optim_inv_scale(const float* scale) { return scale ? (float)(1.0 / (double)scale[0]) : 1.f; }

// Sum of the block's values in a fixed order (a tree over the thread index): the same bytes on every call.
__device__ __forceinline__ double optim_block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kOptBlock >> 1; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ double sq(float g, float inv) {
  const double x = (double)(g * inv);   // the unscaled gradient as float32, as unscale_ leaves it
  return x * x;
}

// partial[chunk] = sum (g * inv_scale)^2 in double, flag[chunk] = the sum is not finite (a float32 square cannot overflow a
// double, so that is: some element is Inf or NaN)
__global__ __launch_bounds__(kOptBlock) void optim_grad_sumsq(const dhdw_optim_chunk* __restrict__ chunks, const float* __restrict__ scale,
                                                              double* __restrict__ partial, int* __restrict__ flag) {
  __shared__ double red[kOptBlock];
  const int chunk = blockIdx.x;
  const uint64_t addr = chunks[chunk].g;
  const int n = chunks[chunk].len;
  const float inv = optim_inv_scale(scale);
  const float* __restrict__ g = reinterpret_cast<const float*>(addr);
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
  const int n4 = (addr & 15) == 0 ? n >> 2 : 0;
  double acc = 0.0;
  int i = threadIdx.x;
  for (; i + 3 * kOptBlock < n4; i += 4 * kOptBlock) {
    f32x4 a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = g4[i + q * kOptBlock];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc += (sq(a[q].x, inv) + sq(a[q].y, inv)) + (sq(a[q].z, inv) + sq(a[q].w, inv));
  }
  for (; i < n4; i += kOptBlock) {
    const f32x4 a = g4[i];
    acc += (sq(a.x, inv) + sq(a.y, inv)) + (sq(a.z, inv) + sq(a.w, inv));
  }
  for (int j = 4 * n4 + threadIdx.x; j < n; j += kOptBlock) acc += sq(g[j], inv);
  const double total = optim_block_sum(acc, red);
  if (threadIdx.x == 0) {
    partial[chunk] = total;
    flag[chunk] = !(fabs(total) <= 1.7976931348623157e308);
  }
}

// One workgroup.  The partials are added in a fixed order: thread t adds its run of consecutive partials in index order, thread 0
// adds the runs in index order.
__global__ __launch_bounds__(kOptBlock) void optim_finalize(dhdw_optim_tables t, float max_norm, float growth_factor, float backoff_factor,
                                                            int growth_interval, void* ws) {
  __shared__ double red[kOptBlock];
  __shared__ int s_found;
  const OptimWorkspace w = optim_workspace(ws, t.n_partials);
  const int tid = threadIdx.x;
  const int run = (t.n_partials + kOptBlock - 1) / kOptBlock;
  double acc = 0.0;
  int bad = 0;
  for (int i = tid * run; i < min((tid + 1) * run, t.n_partials); ++i) {
    acc += w.partial[i];
    bad |= w.flag[i];
  }
  red[tid] = acc;
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    double total = 0.0;
    for (int i = 0; i < kOptBlock; ++i) total += red[i];
    const float norm = (float)sqrt(total);
    const int found = bad || !(fabsf(norm) <= 3.402823466e38f);
    float coef = 1.f;
    if (max_norm >= 0.f) coef = (float)fmin(1.0, (double)max_norm / ((double)norm + 1e-6));   // torch's clip_grad_norm_
    float scale = 1.f;
    if (t.scale) {
      // torch._amp_update_scale_
      scale = t.scale[0];
      int tracker = t.growth_tracker[0];
      w.mult[0] = optim_inv_scale(t.scale) * coef;
      if (found) {
        scale *= backoff_factor;
        tracker = 0;
      } else if (++tracker == growth_interval) {
        const float grown = scale * growth_factor;
        if (fabsf(grown) <= 3.402823466e38f) scale = grown;
        tracker = 0;
      }
      t.scale[0] = scale;
      t.growth_tracker[0] = tracker;
    } else {
      w.mult[0] = coef;
    }
    w.record[0] = norm;
    w.record[1] = coef;
    w.record[2] = found ? 1.f : 0.f;
    w.record[3] = scale;
    w.found[0] = found;
    s_found = found;
  }
  __syncthreads();
  const bool found = s_found != 0;
  for (int g = tid; g < t.n_groups; g += kOptBlock) {
    const dhdw_optim_group h = t.groups[g];
    t.group_scalars[4 * g + 0] = (float)(1.0 - h.beta1);
    t.group_scalars[4 * g + 1] = (float)h.beta2;
    t.group_scalars[4 * g + 2] = (float)(1.0 - h.beta2);
    t.group_scalars[4 * g + 3] = (float)h.eps;
  }
  if (found) return;   // a skipped step: the counts and the scalars of the last step stay
  for (int s = tid; s < t.n_slots; s += kOptBlock) {
    const int g = t.slot_group[s];
    if (g < 0) continue;   // no gradient in this step: the tensor takes no part
    const dhdw_optim_group h = t.groups[g];
    const float step = t.steps[s] + 1.f;
    t.steps[s] = step;
    const double bc1 = 1.0 - pow(h.beta1, (double)step), bc2 = 1.0 - pow(h.beta2, (double)step);
    t.slot_scalars[4 * s + 0] = (float)(1.0 - h.lr * h.weight_decay);
    t.slot_scalars[4 * s + 1] = (float)(h.lr / bc1);
    t.slot_scalars[4 * s + 2] = (float)sqrt(bc2);
    t.slot_scalars[4 * s + 3] = 0.f;
  }
}

struct AdamScalars {
  float mult, decay, step_size, bc2_sqrt, omb1, b2, omb2, eps;
};

// torch's single-tensor AdamW on one element, one rounding per operation
__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, const AdamScalars& s) {
  g = g * s.mult;
  p = p * s.decay;
  m = m + (g - m) * s.omb1;
  v = v * s.b2 + s.omb2 * g * g;
  const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
  p = p - s.step_size * (m / denom);
}

__device__ __forceinline__ void adamw4(f32x4& p, f32x4 g, f32x4& m, f32x4& v, const AdamScalars& s) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float pk = p[k], mk = m[k], vk = v[k];
    adamw1(pk, g[k], mk, vk, s);
    p[k] = pk;
    m[k] = mk;
    v[k] = vk;
  }
}

__device__ __forceinline__ f32x4 ema4(f32x4 e, f32x4 p, float d, float omd) {
  f32x4 r;
  r.x = ema1(e.x, p.x, d, omd);
  r.y = ema1(e.y, p.y, d, omd);
  r.z = ema1(e.z, p.z, d, omd);
  r.w = ema1(e.w, p.w, d, omd);
  return r;
}

// the half image of p: what p.to(dtype) gives (round to nearest even; the hardware converts)
template <int H> __device__ __forceinline__ void store_half4(void* h, int i, f32x4 p) {
  if constexpr (H == DHD_F16) {
    reinterpret_cast<u32x2*>(h)[i] = u32x2{dhd::Pair<_Float16>::narrow(f32x2{p.x, p.y}), dhd::Pair<_Float16>::narrow(f32x2{p.z, p.w})};
  } else if constexpr (H == DHD_BF16) {
    reinterpret_cast<u32x2*>(h)[i] = u32x2{dhd::Pair<__bf16>::narrow(f32x2{p.x, p.y}), dhd::Pair<__bf16>::narrow(f32x2{p.z, p.w})};
  }
}
template <int H> __device__ __forceinline__ void store_half1(void* h, int j, float p) {
  if constexpr (H == DHD_F16) reinterpret_cast<_Float16*>(h)[j] = (_Float16)p;
  else if constexpr (H == DHD_BF16) reinterpret_cast<__bf16*>(h)[j] = (__bf16)p;
}

// One chunk of the sweep.  H: the half copy's dtype code (DHD_F32 = none), EMA: the chunk has an EMA copy.
template <int H, bool EMA>
__device__ __forceinline__ void adamw_chunk(const dhdw_optim_chunk& c, const AdamScalars& s, float d, float omd) {
  float* __restrict__ p = reinterpret_cast<float*>(c.p);
  const float* __restrict__ g = reinterpret_cast<const float*>(c.g);
  float* __restrict__ m = reinterpret_cast<float*>(c.exp_avg);
  float* __restrict__ v = reinterpret_cast<float*>(c.exp_avg_sq);
  float* __restrict__ e = reinterpret_cast<float*>(c.ema);
  void* h = reinterpret_cast<void*>(c.half);
  const int n = c.len;
  const uint64_t all = c.p | c.g | c.exp_avg | c.exp_avg_sq | (EMA ? c.ema : 0) | (H != DHD_F32 ? c.half : 0);
  const int n4 = (all & 15) == 0 ? n >> 2 : 0;
  f32x4* p4 = reinterpret_cast<f32x4*>(p);
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
  f32x4* m4 = reinterpret_cast<f32x4*>(m);
  f32x4* v4 = reinterpret_cast<f32x4*>(v);
  f32x4* e4 = reinterpret_cast<f32x4*>(e);
  int i = threadIdx.x;
  for (; i + 3 * kOptBlock < n4; i += 4 * kOptBlock) {
    f32x4 P[4], G[4], M[4], V[4], E[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = i + q * kOptBlock;
      P[q] = p4[k];
      G[q] = __builtin_nontemporal_load(g4 + k);
      M[q] = m4[k];
      V[q] = v4[k];
      if constexpr (EMA) E[q] = e4[k];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = i + q * kOptBlock;
      adamw4(P[q], G[q], M[q], V[q], s);
      p4[k] = P[q];
      m4[k] = M[q];
      v4[k] = V[q];
      if constexpr (EMA) e4[k] = ema4(E[q], P[q], d, omd);
      store_half4<H>(h, k, P[q]);
    }
  }
  for (; i < n4; i += kOptBlock) {
    f32x4 P = p4[i], M = m4[i], V = v4[i];
    const f32x4 G = __builtin_nontemporal_load(g4 + i);
    adamw4(P, G, M, V, s);
    p4[i] = P;
    m4[i] = M;
    v4[i] = V;
    if constexpr (EMA) e4[i] = ema4(e4[i], P, d, omd);
    store_half4<H>(h, i, P);
  }
  for (int j = 4 * n4 + threadIdx.x; j < n; j += kOptBlock) {
    float pj = p[j], mj = m[j], vj = v[j];
    adamw1(pj, g[j], mj, vj, s);
    p[j] = pj;
    m[j] = mj;
    v[j] = vj;
    if constexpr (EMA) e[j] = ema1(e[j], pj, d, omd);
    store_half1<H>(h, j, pj);
  }
}

// a skipped step: p, m and v stay; the EMA moves towards the unchanged p (ModelEMA.update after a skipped scaler.step) and the
// half copy is written again from it -- the same bytes where it was current, and current afterwards where it was not
template <int H>
__device__ __forceinline__ void skipped_chunk(const dhdw_optim_chunk& c, bool has_ema, float d, float omd) {
  const float* __restrict__ p = reinterpret_cast<const float*>(c.p);
  float* __restrict__ e = reinterpret_cast<float*>(c.ema);
  void* h = reinterpret_cast<void*>(c.half);
  const int n = c.len;
  const uint64_t all = c.p | (has_ema ? c.ema : 0) | (H != DHD_F32 ? c.half : 0);
  const int n4 = (all & 15) == 0 ? n >> 2 : 0;
  const f32x4* p4 = reinterpret_cast<const f32x4*>(p);
  f32x4* e4 = reinterpret_cast<f32x4*>(e);
  for (int i = threadIdx.x; i < n4; i += kOptBlock) {
    const f32x4 P = p4[i];
    if (has_ema) e4[i] = ema4(e4[i], P, d, omd);
    store_half4<H>(h, i, P);
  }
  for (int j = 4 * n4 + threadIdx.x; j < n; j += kOptBlock) {
    const float pj = p[j];
    if (has_ema) e[j] = ema1(e[j], pj, d, omd);
    store_half1<H>(h, j, pj);
  }
}

__global__ __launch_bounds__(kOptBlock) void optim_adamw_update(const dhdw_optim_chunk* __restrict__ chunks, const float* __restrict__ slot_scalars,
                                                                const float* __restrict__ group_scalars, const float* __restrict__ decay_pair,
                                                                const float* __restrict__ mult, const int* __restrict__ found) {
  const dhdw_optim_chunk c = chunks[blockIdx.x];
  const bool ema = c.ema != 0;
  float d = 0.f, omd = 0.f;
  if (ema) {
    d = decay_pair[0];
    omd = decay_pair[1];
  }
  const int half = c.half ? c.half_dtype : DHD_F32;
  if (found[0]) {   // uniform over the grid
    if (half == DHD_F16) skipped_chunk<DHD_F16>(c, ema, d, omd);
    else if (half == DHD_BF16) skipped_chunk<DHD_BF16>(c, ema, d, omd);
    else if (ema) skipped_chunk<DHD_F32>(c, ema, d, omd);
    return;
  }
  AdamScalars s;
  s.mult = mult[0];
  s.decay = slot_scalars[4 * c.slot + 0];
  s.step_size = slot_scalars[4 * c.slot + 1];
  s.bc2_sqrt = slot_scalars[4 * c.slot + 2];
  s.omb1 = group_scalars[4 * c.group + 0];
  s.b2 = group_scalars[4 * c.group + 1];
  s.omb2 = group_scalars[4 * c.group + 2];
  s.eps = group_scalars[4 * c.group + 3];
  if (ema) {
    if (half == DHD_F16) adamw_chunk<DHD_F16, true>(c, s, d, omd);
    else if (half == DHD_BF16) adamw_chunk<DHD_BF16, true>(c, s, d, omd);
    else adamw_chunk<DHD_F32, true>(c, s, d, omd);
  } else {
    if (half == DHD_F16) adamw_chunk<DHD_F16, false>(c, s, d, omd);
    else if (half == DHD_BF16) adamw_chunk<DHD_BF16, false>(c, s, d, omd);
    else adamw_chunk<DHD_F32, false>(c, s, d, omd);
  }
}

int optim_check(const dhdw_optim_tables* t, const void* ws, size_t bytes) {
  if (!t || !ws) return DHD_EINVAL;
  if (t->n_chunks < 0 || t->n_groups < 0 || t->n_slots < 0 || t->n_partials < t->n_chunks) return DHD_EINVAL;
  if (t->n_chunks > 0 && !t->chunks) return DHD_EINVAL;
  if (!dhd_aligned(16, t->chunks, ws)) return DHD_EINVAL;
  if (bytes < dhdw_optim_workspace_bytes(t->n_partials)) return DHD_ENOSPACE;
  return DHD_OK;
}

}  // namespace

extern "C" size_t dhdw_optim_workspace_bytes(int n_chunks) {
  if (n_chunks < 0) return 0;
  const size_t bytes = DHDW_OPTIM_PARTIALS_AT + (size_t)n_chunks * (sizeof(double) + sizeof(int));
  return (bytes + 15) & ~(size_t)15;
}

extern "C" int dhdw_optim_grad_norm(const dhdw_optim_tables* t, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = optim_check(t, workspace, workspace_bytes);
  if (rc != DHD_OK) return rc;
  if (t->scale && !t->growth_tracker) return DHD_EINVAL;
  if (t->n_chunks == 0) return DHD_OK;
  const OptimWorkspace w = optim_workspace(workspace, t->n_partials);
  hipLaunchKernelGGL(optim_grad_sumsq, dim3(t->n_chunks), dim3(kOptBlock), 0, dhd_stream(stream), t->chunks, t->scale, w.partial, w.flag);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

extern "C" int dhdw_optim_finalize(const dhdw_optim_tables* t, float max_norm, float growth_factor, float backoff_factor,
                                   int growth_interval, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = optim_check(t, workspace, workspace_bytes);
  if (rc != DHD_OK) return rc;
  if (max_norm != max_norm) return DHD_EINVAL;
  if (t->scale && !t->growth_tracker) return DHD_EINVAL;
  if (t->n_slots > 0 && (!t->groups || t->n_groups == 0 || !t->slot_group || !t->steps || !t->slot_scalars || !t->group_scalars))
    return DHD_EINVAL;
  if (t->n_groups > 0 && (!t->groups || !t->group_scalars)) return DHD_EINVAL;
  hipLaunchKernelGGL(optim_finalize, dim3(1), dim3(kOptBlock), 0, dhd_stream(stream), *t, max_norm, growth_factor, backoff_factor,
                     growth_interval, workspace);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

extern "C" int dhdw_optim_adamw_update(const dhdw_optim_tables* t, const void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = optim_check(t, workspace, workspace_bytes);
  if (rc != DHD_OK) return rc;
  if (t->n_chunks == 0) return DHD_OK;
  if (!t->groups || !t->slot_scalars || !t->group_scalars) return DHD_EINVAL;
  const OptimWorkspace w = optim_workspace(const_cast<void*>(workspace), t->n_partials);
  hipLaunchKernelGGL(optim_adamw_update, dim3(t->n_chunks), dim3(kOptBlock), 0, dhd_stream(stream), t->chunks, t->slot_scalars,
                     t->group_scalars, t->decay_pair, w.mult, w.found);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}
