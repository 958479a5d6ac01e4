// Half-storage form of the SFA stage operator (dhd_sfa_weights.storage_dtype): its element-wise passes.  Included by
// sfa_stage.hip inside its unnamed namespace, after the float32 stage's kernels and helpers (block_sum, BnTail, FcGradJob ...);
// the host side that launches them is sfa_stage.hip's, shared with the float32 storage.  GEMM kernels: sfa_half.h.
// Reference: models/necks/mix.py:37-59 under autocast (DHD-S.py:281).

// [lo, hi) in 8-element units of this block's share of a plane of hw elements (hw % 8 == 0)
__device__ __forceinline__ void chunk_range8(int hw, int* lo, int* hi) {
  const int n8 = hw >> 3, per = (n8 + kPlaneChunks - 1) / kPlaneChunks;
  *lo = blockIdx.x * per;
  *hi = min(n8, *lo + per);
}

struct PackJobH {
  const float* w[2];     // conv1, conv2
  u32x4* dst[4];         // conv1, conv2, conv1^T, conv2^T  (cuh_pack_weight)
  int c, blocks_each;
};

// channel means of x (block rows < n_planes) and, in rows of extra blocks, the four weight images of the call
template <class TS>
__global__ __launch_bounds__(kEwBlock) void plane_mean_pack_h_kernel(const TS* __restrict__ x, float* __restrict__ part, int hw,
                                                                     int n_planes, PackJobH job) {
  __shared__ float sm[kEwBlock / DHD_WAVE];
  if ((int)blockIdx.y >= n_planes) {
    const int pb = ((int)blockIdx.y - n_planes) * kPlaneChunks + (int)blockIdx.x;
    const int which = pb / job.blocks_each;
    if (which < 4 && job.dst[which] != nullptr)   // (forward-only inference packs no transposes)
      cuh_pack_weight<TS>(job.w[which & 1], which >> 1, job.dst[which], job.c, (pb % job.blocks_each) * kEwBlock + (int)threadIdx.x);
    return;
  }
  const size_t plane = blockIdx.y;
  const TS* p = x + plane * hw;
  int lo, hi;
  chunk_range8(hw, &lo, &hi);
  float a0 = 0.f, a1 = 0.f;
  int i = lo + threadIdx.x;
  for (; i + kEwBlock < hi; i += 2 * kEwBlock) {
    float v[8], w[8];
    ld8<TS>(p, i, v);
    ld8<TS>(p, i + kEwBlock, w);
    a0 += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    a1 += ((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7]));
  }
  if (i < hi) {
    float v[8];
    ld8<TS>(p, i, v);
    a0 += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  }
  const float tot = block_sum(a0 + a1, sm);
  if (threadIdx.x == 0) part[plane * kPlaneChunks + blockIdx.x] = tot;
}

// out = g*(a*xb) + (1-g)*((1-a)*xv),  g = sigmoid(sc*y2 + sh)
template <class TS>
__global__ __launch_bounds__(kEwBlock) void blend2_bn_h_kernel(const TS* __restrict__ x, const float* __restrict__ a1,
                                                               const TS* __restrict__ y2, const float* __restrict__ scsh,
                                                               TS* __restrict__ out, int c, int hw) {
  const int plane = blockIdx.y, b = plane / c, ch = plane % c;
  const float a = a1[plane], na = 1.0f - a, sc = scsh[ch], sh = scsh[c + ch];
  const TS* xb = x + ((size_t)b * 2 * c + ch) * hw;
  const TS* xv = x + ((size_t)b * 2 * c + c + ch) * hw;
  const TS* yp = y2 + (size_t)plane * hw;
  TS* op = out + (size_t)plane * hw;
  int lo, hi;
  chunk_range8(hw, &lo, &hi);
  for (int i = lo + threadIdx.x; i < hi; i += kEwBlock) {
    float p[8], q[8], s[8], r[8];
    ld8<TS>(xb, i, p);
    ld8<TS>(xv, i, q);
    ld8<TS>(yp, i, s);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float g = sigmoidf_(fmaf(sc, s[j], sh));
      r[j] = g * (a * p[j]) + (1.0f - g) * (na * q[j]);
    }
    st8<TS>(op, i, r);
  }
}

// g2 = dL/d s2 = go*(a*xb - (1-a)*xv)*g*(1-g), stored in TS; the BatchNorm-2 backward sums are those of the STORED g2;
// the go-part of dL/da: sum go*(g*xb - (1-g)*xv).   part: [(b*chunks+chunk)][2][c];  da_p1: [(b*chunks+chunk)][c]
template <class TS>
__global__ __launch_bounds__(kEwBlock) void blend2_bn_bwd_h_kernel(const TS* __restrict__ x, const float* __restrict__ a1,
                                                                   const TS* __restrict__ y2, const float* __restrict__ scsh,
                                                                   const float* __restrict__ mean, const TS* __restrict__ go,
                                                                   TS* __restrict__ g2, float* __restrict__ part,
                                                                   float* __restrict__ da_p1, int c, int hw, BnTail tail) {
  __shared__ float sm[kEwBlock / DHD_WAVE];
  const int plane = blockIdx.y, b = plane / c, ch = plane % c;
  const float a = a1[plane], na = 1.0f - a, sc = scsh[ch], sh = scsh[c + ch], mu = mean[ch];
  const TS* xb = x + ((size_t)b * 2 * c + ch) * hw;
  const TS* xv = x + ((size_t)b * 2 * c + c + ch) * hw;
  const TS* yp = y2 + (size_t)plane * hw;
  const TS* gp = go + (size_t)plane * hw;
  TS* rp = g2 + (size_t)plane * hw;
  int lo, hi;
  chunk_range8(hw, &lo, &hi);
  float s1 = 0.f, s2 = 0.f, sa = 0.f;
  auto body = [&](const u32x4 wp, const u32x4 wq, const u32x4 ws, const u32x4 wo, int i) {
    float p[8], q[8], s[8], o[8], r[8];
    widen16<TS>(wp, p);
    widen16<TS>(wq, q);
    widen16<TS>(ws, s);
    widen16<TS>(wo, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float g = sigmoidf_(fmaf(sc, s[j], sh));
      r[j] = o[j] * (a * p[j] - na * q[j]) * g * (1.0f - g);
      sa = fmaf(o[j], g * p[j] - (1.0f - g) * q[j], sa);
    }
    const u32x4 pk = narrow16<TS>(r);
    __builtin_nontemporal_store(pk, reinterpret_cast<u32x4*>(rp) + i);
    widen16<TS>(pk, r);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s1 += r[j];
      s2 = fmaf(r[j], s[j] - mu, s2);
    }
  };
  auto ldv = [](const TS* base, int i) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(base) + i); };
  int i = lo + threadIdx.x;
  for (; i + kEwBlock < hi; i += 2 * kEwBlock) {   // two 16-byte vectors of each of the four streams in flight per thread
    const u32x4 p0 = ldv(xb, i), q0 = ldv(xv, i), y0 = ldv(yp, i), o0 = ldv(gp, i);
    const u32x4 p1 = ldv(xb, i + kEwBlock), q1 = ldv(xv, i + kEwBlock), y1v = ldv(yp, i + kEwBlock), o1 = ldv(gp, i + kEwBlock);
    body(p0, q0, y0, o0, i);
    body(p1, q1, y1v, o1, i + kEwBlock);
  }
  if (i < hi) body(ldv(xb, i), ldv(xv, i), ldv(yp, i), ldv(gp, i), i);
  s1 = block_sum(s1, sm);
  s2 = block_sum(s2, sm);
  sa = block_sum(sa, sm);
  if (threadIdx.x == 0) {
    const size_t qi = (size_t)(b * kPlaneChunks + blockIdx.x);
    da_p1[qi * c + ch] = sa;
    bn_backward_publish(tail, part, qi, ch, c, s1, s2);
  }
}

// sums for BatchNorm backward: S1 = sum g, S2 = sum g*(y - mean)
template <class TS>
__global__ __launch_bounds__(kEwBlock) void pair_sums_h_kernel(const TS* __restrict__ g, const TS* __restrict__ y,
                                                               const float* __restrict__ mean, float* __restrict__ part, int c, int hw,
                                                               BnTail tail) {
  __shared__ float sm[kEwBlock / DHD_WAVE];
  const int plane = blockIdx.y, b = plane / c, ch = plane % c;
  const float mu = mean[ch];
  const TS* gp = g + (size_t)plane * hw;
  const TS* yp = y + (size_t)plane * hw;
  int lo, hi;
  chunk_range8(hw, &lo, &hi);
  float s1 = 0.f, s2 = 0.f, t1 = 0.f, t2 = 0.f;
  int i = lo + threadIdx.x;
  for (; i + kEwBlock < hi; i += 2 * kEwBlock) {
    float a[8], v[8], a2[8], v2[8];
    ld8<TS>(gp, i, a);
    ld8<TS>(yp, i, v);
    ld8<TS>(gp, i + kEwBlock, a2);
    ld8<TS>(yp, i + kEwBlock, v2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s1 += a[j];
      s2 = fmaf(a[j], v[j] - mu, s2);
      t1 += a2[j];
      t2 = fmaf(a2[j], v2[j] - mu, t2);
    }
  }
  if (i < hi) {
    float a[8], v[8];
    ld8<TS>(gp, i, a);
    ld8<TS>(yp, i, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s1 += a[j];
      s2 = fmaf(a[j], v[j] - mu, s2);
    }
  }
  s1 = block_sum(s1 + t1, sm);
  s2 = block_sum(s2 + t2, sm);
  if (threadIdx.x == 0) bn_backward_publish(tail, part, (size_t)(b * kPlaneChunks + blockIdx.x), ch, c, s1, s2);
}

// the du-part of dL/da: sum du*(xb - xv).   da_p2: [(b*chunks+chunk)][c]
template <class TS>
__global__ __launch_bounds__(kEwBlock) void blend1_da_h_kernel(const TS* __restrict__ x, const TS* __restrict__ du,
                                                               float* __restrict__ da_p2, int c, int hw) {
  __shared__ float sm[kEwBlock / DHD_WAVE];
  const int plane = blockIdx.y, b = plane / c, ch = plane % c;
  const TS* xb = x + ((size_t)b * 2 * c + ch) * hw;
  const TS* xv = x + ((size_t)b * 2 * c + c + ch) * hw;
  const TS* dp = du + (size_t)plane * hw;
  int lo, hi;
  chunk_range8(hw, &lo, &hi);
  float acc = 0.f;
  for (int i = lo + threadIdx.x; i < hi; i += kEwBlock) {
    float p[8], q[8], d[8];
    ld8<TS>(xb, i, p);
    ld8<TS>(xv, i, q);
    ld8<TS>(dp, i, d);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = fmaf(d[j], p[j] - q[j], acc);
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) da_p2[(size_t)(b * kPlaneChunks + blockIdx.x) * c + ch] = acc;
}

// gx_bev = a*(go*g + du) + ds_bev/hw;  gx_vox = (1-a)*(go*(1-g) + du) + ds_vox/hw
template <class TS>
__global__ __launch_bounds__(kEwBlock) void stage_gx_h_kernel(const float* __restrict__ a1, const TS* __restrict__ y2,
                                                              const float* __restrict__ scsh, const TS* __restrict__ go,
                                                              const TS* __restrict__ du, const float* __restrict__ ds,
                                                              TS* __restrict__ gx, int c, int hw, int fc_rows, FcGradJob fc) {
  if ((int)blockIdx.y < fc_rows) {   // the first block rows: the Linear layers' parameter gradients
    fc_param_grad_block(fc, (int)blockIdx.y * kPlaneChunks + (int)blockIdx.x, c);
    return;
  }
  const int plane = (int)blockIdx.y - fc_rows, b = plane / c, ch = plane % c;
  const float a = a1[plane], na = 1.0f - a, sc = scsh[ch], sh = scsh[c + ch];
  const float kb = ds[(size_t)b * 2 * c + ch] / (float)hw, kv = ds[(size_t)b * 2 * c + c + ch] / (float)hw;
  const TS* yp = y2 + (size_t)plane * hw;
  const TS* gp = go + (size_t)plane * hw;
  const TS* dp = du + (size_t)plane * hw;
  TS* gb = gx + ((size_t)b * 2 * c + ch) * hw;
  TS* gv = gx + ((size_t)b * 2 * c + c + ch) * hw;
  int lo, hi;
  chunk_range8(hw, &lo, &hi);
  auto body = [&](const u32x4 ws, const u32x4 wo, const u32x4 wd, int i) {
    float s[8], o[8], d[8], rb[8], rv[8];
    widen16<TS>(ws, s);
    widen16<TS>(wo, o);
    widen16<TS>(wd, d);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float g = sigmoidf_(fmaf(sc, s[j], sh));
      rb[j] = fmaf(a, fmaf(o[j], g, d[j]), kb);
      rv[j] = fmaf(na, fmaf(o[j], 1.0f - g, d[j]), kv);
    }
    st8<TS>(gb, i, rb);
    st8<TS>(gv, i, rv);
  };
  auto ldv = [](const TS* base, int i) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(base) + i); };
  int i = lo + threadIdx.x;
  for (; i + kEwBlock < hi; i += 2 * kEwBlock) {   // two vectors of each stream in flight per thread
    const u32x4 s0 = ldv(yp, i), o0 = ldv(gp, i), d0 = ldv(dp, i);
    const u32x4 s1 = ldv(yp, i + kEwBlock), o1 = ldv(gp, i + kEwBlock), d1 = ldv(dp, i + kEwBlock);
    body(s0, o0, d0, i);
    body(s1, o1, d1, i + kEwBlock);
  }
  if (i < hi) body(ldv(yp, i), ldv(gp, i), ldv(dp, i), i);
}
