// The temporal-stereo cost volume from the camera matrices (capi_stereo/dhd_amd_stereo_cv.h: dhdv_*), included at the end of
// deform.hip: the set of translation units is a closed list held by tests, and the kernels below are the kernels above them with
// two things changed.
//
//   1. The sampling position of hypothesis d at pixel (y, x) of view n is evaluated from the view's matrices and the three axes
//      of the separable frustum template (stereo_position) where lane_cell reads it from a (bn, D h, w, 2) grid that ~40 torch
//      launches wrote: the same float32 operation chain as DepthNet.gen_grid on the device, operation for operation (the library is
//      compiled without contraction and with correctly rounded division for this).  Lane l evaluates hypothesis d0 + l, 64
//      hypotheses at once, so the chain (about 250 instructions with its two correctly rounded divisions) costs about four
//      instructions per hypothesis, against ~50 of the hypothesis' own step.
//   2. The feature maps are read in their own type.  T = float: stereo_cost_volume_kernel / stereo_cost_volume_pair_kernel with
//      the same tap order, the same DPP tree and cv_softmax_store, so the same bytes.  T = _Float16 / __bf16: a 16-byte load is 8
//      channels, so a hypothesis needs half the lanes: up to 128 channels take 16 lanes (four hypotheses per step), up to 256 take
//      32 (two per step), more take the wave with one or two loads per lane.  Taps are widened to float32 (exact), the blend,
//      |diff| sums, the bias rule and the softmax are float32 as above, the result is rounded once.
//
// stereo_grid_kernel writes the positions themselves: the positions' own test, and the feed of dhd_stereo_cost_volume for
// feature shapes the fused kernels do not take.
#pragma once

// The constants of capi_stereo/dhd_amd_stereo_cv.h, restated: that header is compiled with include/ on the include path, which
// the library's own build does not have (tests/test_stereo_cv_capi.py holds the two sets of values equal).
#define DHDV_NCHW 0
#define DHDV_NHWC 1
#define DHDV_MAX_C 1024
#define DHDV_MAX_D 256

namespace dhd_stereo {

using dhd::f32x4;
using dhd::kVec16;
using dhd::raw16;
using dhd::Vec16;

struct Geom {
  const float *inv_post_rot, *post_trans, *combine, *trans, *intrins, *post_rots;   // (bn, 9) / (bn, 3)
  const float *u, *v, *dep;                                                         // (w), (h), (nd)
  float inv_w, inv_h;   // 1.0f / (wi - 1), 1.0f / (hi - 1): torch divides by a host scalar by multiplying with its reciprocal
};

// row `r` of the 3 x 3 matrix m applied to (a, b, c) as _mat_vec's Python sum() does: ((0 + m0 a) + m1 b) + m2 c
__device__ __forceinline__ float row3(const float* __restrict__ m, int r, float a, float b, float c) {
  return ((0.0f + m[3 * r] * a) + m[3 * r + 1] * b) + m[3 * r + 2] * c;
}

// the normalised sampling position of frustum point (u, v, dep) of view n in the adjacent image: gen_grid, see the C header
__device__ __forceinline__ void stereo_position(const Geom& g, int n, float u, float v, float dep, float& px, float& py) {
  const float* ipr = g.inv_post_rot + 9 * (size_t)n;
  const float* pt = g.post_trans + 3 * (size_t)n;
  const float* cb = g.combine + 9 * (size_t)n;
  const float* tr = g.trans + 3 * (size_t)n;
  const float* km = g.intrins + 9 * (size_t)n;
  const float* pr = g.post_rots + 9 * (size_t)n;
  const float p0 = u - pt[0], p1 = v - pt[1], p2 = dep - pt[2];
  float x = row3(ipr, 0, p0, p1, p2), y = row3(ipr, 1, p0, p1, p2), z = row3(ipr, 2, p0, p1, p2);
  x = x * z;
  y = y * z;
  const float cx = row3(cb, 0, x, y, z) + tr[0], cy = row3(cb, 1, x, y, z) + tr[1], cz = row3(cb, 2, x, y, z) + tr[2];
  const bool neg = cz < 1e-3f;
  const float ix = row3(km, 0, cx, cy, cz), iy = row3(km, 1, cx, cy, cz), iz = row3(km, 2, cx, cy, cz);
  const float qx = ix / iz, qy = iy / iz;
  const float fx = ((0.0f + pr[0] * qx) + pr[1] * qy) + pt[0];
  const float fy = ((0.0f + pr[3] * qx) + pr[4] * qy) + pt[1];
  px = neg ? -2.0f : fx * g.inv_w * 2.0f - 1.0f;
  py = neg ? -2.0f : fy * g.inv_h * 2.0f - 1.0f;
}

__global__ __launch_bounds__(kBlock) void stereo_grid_kernel(Geom g, float* __restrict__ grid, int h, int w, int nd, int total) {
  const int i = blockIdx.x * kBlock + threadIdx.x;   // ((n, d), y, x)
  if (i >= total) return;
  const int x = i % w, y = (i / w) % h, d = (i / (w * h)) % nd, n = i / (w * h * nd);
  float px, py;
  stereo_position(g, n, g.u[x], g.v[y], g.dep[d], px, py);
  reinterpret_cast<float2*>(grid)[i] = make_float2(px, py);
}

// the value a position has after gen_grid(...).to(T).float()
template <typename T> __device__ __forceinline__ float through(float v) { return (float)(T)v; }

// lane_cell with the position computed instead of read; what follows the position is lane_cell's
template <typename T>
__device__ __forceinline__ CellRegs lane_cell_geom(const Geom& g, int n, float u, float v, int d, int nd, int h, int w) {
  CellRegs r;
  float gx = 0.f, gy = 0.f;
  const bool have = d < nd;
  if (have) {
    stereo_position(g, n, u, v, g.dep[d], gx, gy);
    gx = through<T>(gx);
    gy = through<T>(gy);
  }
  const float px = (gx + 1.0f) * 0.5f * (float)(w - 1);   // align_corners=True
  const float py = (gy + 1.0f) * 0.5f * (float)(h - 1);
  const Tap tp = make_tap(py, px, h, w);
  r.idx[0] = have && tp.v00 ? tp.i00 : -1;
  r.idx[1] = have && tp.v01 ? tp.i01 : -1;
  r.idx[2] = have && tp.v10 ? tp.i10 : -1;
  r.idx[3] = have && tp.v11 ? tp.i11 : -1;
  r.wt[0] = tp.w00; r.wt[1] = tp.w01; r.wt[2] = tp.w10; r.wt[3] = tp.w11;
  return r;
}

// 16 bytes of channels as one (float) or two (half types) float4: vectors, not arrays of floats, so that a component picked by
// a run-time index stays a chain of selects on registers
template <typename T> struct Wide {
  static constexpr int NV = kVec16<T> / 4;
  f32x4 v[NV];
};
template <typename T> __device__ __forceinline__ raw16<T> raw_zero() {
  if constexpr (std::is_same_v<T, float>) return f32x4{0.f, 0.f, 0.f, 0.f};
  else return dhd::u32x4{0u, 0u, 0u, 0u};
}
template <typename T> __device__ __forceinline__ Wide<T> widen(raw16<T> w) {
  Wide<T> r;
  if constexpr (std::is_same_v<T, float>) {
    r.v[0] = w;
  } else {
    const dhd::f32x2 a = dhd::Pair<T>::widen(w[0]), b = dhd::Pair<T>::widen(w[1]), c = dhd::Pair<T>::widen(w[2]), d = dhd::Pair<T>::widen(w[3]);
    r.v[0] = f32x4{a.x, a.y, b.x, b.y};
    r.v[1] = f32x4{c.x, c.y, d.x, d.y};
  }
  return r;
}
template <typename T> __device__ __forceinline__ Wide<T> wide_zero() {
  Wide<T> r;
#pragma unroll
  for (int j = 0; j < Wide<T>::NV; ++j) r.v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  return r;
}
// s += wk * t, per component: one product and one sum, each rounded
template <typename T> __device__ __forceinline__ void blend(Wide<T>& s, float wk, const Wide<T>& t) {
#pragma unroll
  for (int j = 0; j < Wide<T>::NV; ++j) s.v[j] += wk * t.v[j];
}
// sum of |a - s| over the 16 bytes: pairs first, per float4 the order of the float32 kernels
template <typename T> __device__ __forceinline__ float abs_diff_sum(const Wide<T>& a, const Wide<T>& s) {
  float r[Wide<T>::NV];
#pragma unroll
  for (int j = 0; j < Wide<T>::NV; ++j) {
    const f32x4 df = a.v[j] - s.v[j];
    r[j] = (fabsf(df.x) + fabsf(df.y)) + (fabsf(df.z) + fabsf(df.w));
  }
  if constexpr (Wide<T>::NV == 1) return r[0];
  else return r[0] + r[1];
}
template <typename T> __device__ __forceinline__ float pick_wide(const Wide<T>& s, int comp) {
  if constexpr (Wide<T>::NV == 1) return pick(s.v[0], comp);
  else return pick(comp >= 4 ? s.v[1] : s.v[0], comp & 3);
}

// cv_softmax_store with the result rounded to T
template <typename T>
__device__ __forceinline__ void softmax_store(const float (&mine)[kCvMaxD / DHD_WAVE], T* __restrict__ out, int bn, int nd, int hw, int yx,
                                              int lane) {
  if constexpr (std::is_same_v<T, float>) {
    cv_softmax_store(mine, out, bn, nd, hw, yx, lane);
  } else {
    float mn = mine[0];
#pragma unroll
    for (int q = 1; q < kCvMaxD / DHD_WAVE; ++q) mn = fminf(mn, mine[q]);
    for (int m = 32; m > 0; m >>= 1) mn = fminf(mn, __shfl_xor(mn, m, DHD_WAVE));
    float e[kCvMaxD / DHD_WAVE], sum = 0.f;
#pragma unroll
    for (int q = 0; q < kCvMaxD / DHD_WAVE; ++q) {
      e[q] = mine[q] > 1.0e38f ? 0.f : __expf(mn - mine[q]);
      sum += e[q];
    }
    sum = wave_sum_bcast(sum);
    const float inv = 1.0f / sum;
    T* ob = out + (size_t)bn * nd * hw + yx;
#pragma unroll
    for (int q = 0; q < kCvMaxD / DHD_WAVE; ++q) {
      const int d = lane + 64 * q;
      if (d < nd) ob[(size_t)d * hw] = (T)(e[q] * inv);
    }
  }
}

// one hypothesis per step, all lanes on its channels: Q 16-byte channel groups per lane (stereo_cost_volume_kernel)
template <typename T, int Q>
__global__ __launch_bounds__(kBlock) void stereo_cv_wide_kernel(const T* __restrict__ prev, const T* __restrict__ curr, Geom geo, int c, int h,
                                                                int w, int nd, float bias, int flag_channel, T* __restrict__ out,
                                                                int n_pix) {
  constexpr int N = kVec16<T>;
  using V = Vec16<T, false>;
  const int lane = threadIdx.x & 63;
  const int pix = blockIdx.x * (kBlock / DHD_WAVE) + (threadIdx.x >> 6);  // (bn, y, x)
  if (pix >= n_pix) return;
  const int hw = h * w;
  const int bn = __builtin_amdgcn_readfirstlane(pix / hw), yx = pix % hw;
  const int cg = c / N;                        // 16-byte groups per pixel
  const T* pb = prev + (size_t)bn * hw * c;
  Wide<T> cur[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int g = lane + 64 * q;
    cur[q] = widen<T>(g < cg ? V::ld(curr + (size_t)pix * c, g) : raw_zero<T>());
  }
  const int flag_group = flag_channel / N, flag_comp = flag_channel % N;
  float mine[kCvMaxD / DHD_WAVE];  // cost of hypothesis d lives in lane d % 64, register d / 64
#pragma unroll
  for (int q = 0; q < kCvMaxD / DHD_WAVE; ++q) mine[q] = 3.0e38f;
  const float fu = geo.u[yx % w], fv = geo.v[yx / w];
  raw16<T> cache[4][Q];
  int cidx[4] = {-1, -1, -1, -1};
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int q = 0; q < Q; ++q) cache[k][q] = raw_zero<T>();
  for (int d0 = 0; d0 < nd; d0 += DHD_WAVE) {
    const CellRegs cell = lane_cell_geom<T>(geo, bn, fu, fv, d0 + lane, nd, h, w);
    const int nb = min(DHD_WAVE, nd - d0);
    for (int i = 0; i < nb; ++i) {
      int nidx[4];
      float wt[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        nidx[k] = __builtin_amdgcn_readlane(cell.idx[k], i);
        wt[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cell.wt[k]), i));
      }
      if (nidx[0] != cidx[0] || nidx[1] != cidx[1] || nidx[2] != cidx[2] || nidx[3] != cidx[3]) {
        raw16<T> nv[4][Q];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int want = nidx[k];
          if (want < 0) {
#pragma unroll
            for (int q = 0; q < Q; ++q) nv[k][q] = raw_zero<T>();
          } else if (want == cidx[0]) {
#pragma unroll
            for (int q = 0; q < Q; ++q) nv[k][q] = cache[0][q];
          } else if (want == cidx[1]) {
#pragma unroll
            for (int q = 0; q < Q; ++q) nv[k][q] = cache[1][q];
          } else if (want == cidx[2]) {
#pragma unroll
            for (int q = 0; q < Q; ++q) nv[k][q] = cache[2][q];
          } else if (want == cidx[3]) {
#pragma unroll
            for (int q = 0; q < Q; ++q) nv[k][q] = cache[3][q];
          } else {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
              const int g = lane + 64 * q;
              nv[k][q] = g < cg ? V::ld(pb + (size_t)want * c, g) : raw_zero<T>();
            }
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          cidx[k] = nidx[k];
#pragma unroll
          for (int q = 0; q < Q; ++q) cache[k][q] = nv[k][q];
        }
      }
      float acc = 0.f, flag = 1.f;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int g = lane + 64 * q;
        if (g >= cg) break;
        Wide<T> s = wide_zero<T>();
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (cidx[k] >= 0) blend<T>(s, wt[k], widen<T>(cache[k][q]));
        acc += abs_diff_sum<T>(cur[q], s);
        if (g == flag_group) flag = pick_wide<T>(s, flag_comp);
      }
      float tot = wave_sum_bcast(acc);
      if (bias != 0.f) {
        const float fv0 = __shfl(flag, flag_group & 63, DHD_WAVE);
        if (fv0 == 0.f) tot += bias;
      }
      if (lane == i) mine[d0 >> 6] = tot;
    }
  }
  softmax_store<T>(mine, out, bn, nd, hw, yx, lane);
}

// GROUP mode (at most G 16-byte channel groups): the 64 / G lane groups of the wave take 64 / G consecutive hypotheses per step.
// G = 32 is stereo_cost_volume_pair_kernel.
template <typename T, int G>
__global__ __launch_bounds__(kBlock) void stereo_cv_group_kernel(const T* __restrict__ prev, const T* __restrict__ curr, Geom geo, int c, int h,
                                                                 int w, int nd, float bias, int flag_channel, T* __restrict__ out,
                                                                 int n_pix) {
  constexpr int N = kVec16<T>, NH = DHD_WAVE / G;
  static_assert(G == 16 || G == 32, "a lane group is one or two DPP rows");
  using V = Vec16<T, false>;
  const int lane = threadIdx.x & 63, sub = lane / G, g = lane % G;
  const int pix = blockIdx.x * (kBlock / DHD_WAVE) + (threadIdx.x >> 6);
  if (pix >= n_pix) return;
  const int hw = h * w;
  const int bn = __builtin_amdgcn_readfirstlane(pix / hw), yx = pix % hw;
  const int cg = c / N;
  const bool live = g < cg;
  const T* pb = prev + (size_t)bn * hw * c + N * g;
  const Wide<T> cur = widen<T>(live ? V::ld(curr + (size_t)pix * c, g) : raw_zero<T>());
  const int flag_group = flag_channel / N, flag_comp = flag_channel % N;
  float mine[kCvMaxD / DHD_WAVE];
#pragma unroll
  for (int q = 0; q < kCvMaxD / DHD_WAVE; ++q) mine[q] = 3.0e38f;
  const float fu = geo.u[yx % w], fv = geo.v[yx / w];
  raw16<T> cache[4] = {raw_zero<T>(), raw_zero<T>(), raw_zero<T>(), raw_zero<T>()};
  int cidx[4] = {-1, -1, -1, -1};
  for (int d0 = 0; d0 < nd; d0 += DHD_WAVE) {
    const CellRegs cell = lane_cell_geom<T>(geo, bn, fu, fv, d0 + lane, nd, h, w);
    const int nb = min(DHD_WAVE, nd - d0);
    for (int i = 0; i < nb; i += NH) {
      const int src = i + sub;                  // the lane that holds this group's hypothesis (beyond nb: every index -1)
      Wide<T> s = wide_zero<T>();
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int want = __shfl(cell.idx[k], src, DHD_WAVE);
        const float wk = __shfl(cell.wt[k], src, DHD_WAVE);
        if (want != cidx[k]) {                   // per lane: the groups walk their own lines
          cache[k] = (want >= 0 && live) ? V::ld(pb + (size_t)want * c) : raw_zero<T>();
          cidx[k] = want;
        }
        if (want >= 0) blend<T>(s, wk, widen<T>(cache[k]));
      }
      float acc = live ? abs_diff_sum<T>(cur, s) : 0.f;
      // the first steps of wave_sum_bcast: the last lane of each group holds the group's sum
      acc = dpp_add<0xB1, 0xf>(acc);
      acc = dpp_add<0x4E, 0xf>(acc);
      acc = dpp_add<0x114, 0xf>(acc);
      acc = dpp_add<0x118, 0xf>(acc);
      if constexpr (G == 32) acc = dpp_add<0x142, 0xa>(acc);
      float tot[NH];
#pragma unroll
      for (int j = 0; j < NH; ++j) tot[j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), G * j + G - 1));
      if (bias != 0.f) {
        const float flag = pick_wide<T>(s, flag_comp);
#pragma unroll
        for (int j = 0; j < NH; ++j) {
          const float fj = __shfl(flag, G * j + (flag_group & (G - 1)), DHD_WAVE);
          if (fj == 0.f) tot[j] += bias;
        }
      }
#pragma unroll
      for (int j = 0; j < NH; ++j)
        if (lane == i + j && i + j < nb) mine[d0 >> 6] = tot[j];
    }
  }
  softmax_store<T>(mine, out, bn, nd, hw, yx, lane);
}

static inline bool dtype_ok(int dtype) { return dtype == DHD_F32 || dtype == DHD_F16 || dtype == DHD_BF16; }
static inline int elem_bytes(int dtype) { return dtype == DHD_F32 ? 4 : 2; }
static inline bool sizes_supported(int dtype, int bn, int c, int h, int w, int nd) {
  if (!dtype_ok(dtype) || bn < 1 || c < 1 || h < 1 || w < 1 || nd < 1) return false;
  const int per = 16 / elem_bytes(dtype);
  if (c % per != 0 || c > DHDV_MAX_C || nd > DHDV_MAX_D) return false;
  return (long)bn * h * w < (1L << 31) / nd;
}

template <typename T>
static void launch_cv(const T* prev, const T* curr, const Geom& geo, int bn, int c, int h, int w, int nd, float bias, int flag_channel, T* out,
                      hipStream_t st) {
  const long n_pix = (long)bn * h * w;
  const dim3 blocks(dhd_cdiv(n_pix, kBlock / DHD_WAVE)), threads(kBlock);
  const int cg = c / kVec16<T>;
#define DHDV_CV(K) hipLaunchKernelGGL(K, blocks, threads, 0, st, prev, curr, geo, c, h, w, nd, bias, flag_channel, out, (int)n_pix)
  if constexpr (std::is_same_v<T, float>) {     // dhd_stereo_cost_volume's choice
    const int q = (cg + DHD_WAVE - 1) / DHD_WAVE;
    if (cg <= 32) DHDV_CV((stereo_cv_group_kernel<T, 32>));
    else if (q <= 1) DHDV_CV((stereo_cv_wide_kernel<T, 1>));
    else if (q == 2) DHDV_CV((stereo_cv_wide_kernel<T, 2>));
    else if (q == 3) DHDV_CV((stereo_cv_wide_kernel<T, 3>));
    else DHDV_CV((stereo_cv_wide_kernel<T, 4>));
  } else {
    if (cg <= 16) DHDV_CV((stereo_cv_group_kernel<T, 16>));
    else if (cg <= 32) DHDV_CV((stereo_cv_group_kernel<T, 32>));
    else if (cg <= 64) DHDV_CV((stereo_cv_wide_kernel<T, 1>));
    else DHDV_CV((stereo_cv_wide_kernel<T, 2>));
  }
#undef DHDV_CV
}

}  // namespace dhd_stereo

extern "C" {

int dhdv_stereo_cv_supported(int dtype, int bn, int c, int h, int w, int n_depth) {
  return dhd_stereo::sizes_supported(dtype, bn, c, h, w, n_depth) ? 1 : 0;
}

size_t dhdv_stereo_cv_scratch_bytes(int dtype, int layout, int bn, int c, int h, int w) {
  if (layout != DHDV_NCHW || !dhd_stereo::sizes_supported(dtype, bn, c, h, w, 1)) return 0;
  const size_t one = ((size_t)bn * c * h * w * dhd_stereo::elem_bytes(dtype) + 15) / 16 * 16;
  return 2 * one;
}

int dhdv_stereo_grid(const float* inv_post_rot, const float* post_trans, const float* combine, const float* trans,
                     const float* intrins, const float* post_rots, const float* u, const float* v, const float* dep, float* grid,
                     int bn, int h, int w, int n_depth, int hi, int wi, void* stream) {
  using namespace dhd_stereo;
  if (!inv_post_rot || !post_trans || !combine || !trans || !intrins || !post_rots || !u || !v || !dep || !grid) return DHD_EINVAL;
  if (!dhd_aligned(4, inv_post_rot, post_trans, combine, trans, intrins, post_rots, u, v, dep) || !dhd_aligned(8, grid)) return DHD_EINVAL;
  if (bn < 1 || h < 1 || w < 1 || n_depth < 1 || hi < 2 || wi < 2) return DHD_EINVAL;
  if (n_depth > DHDV_MAX_D || (long)bn * h * w >= (1L << 31) / n_depth) return DHD_EUNSUPPORTED;
  const Geom geo = {inv_post_rot, post_trans, combine, trans, intrins, post_rots, u, v, dep, 1.0f / (float)(wi - 1), 1.0f / (float)(hi - 1)};
  const int total = bn * n_depth * h * w;
  hipLaunchKernelGGL(stereo_grid_kernel, dim3(dhd_cdiv(total, kBlock)), dim3(kBlock), 0, dhd_stream(stream), geo, grid, h, w, n_depth, total);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

int dhdv_stereo_cost_volume(const void* prev, const void* curr, void* out, int dtype, int layout, const float* inv_post_rot,
                            const float* post_trans, const float* combine, const float* trans, const float* intrins,
                            const float* post_rots, const float* u, const float* v, const float* dep, int bn, int c, int h, int w,
                            int n_depth, int hi, int wi, float bias, int flag_channel, void* scratch, size_t scratch_bytes,
                            void* stream) {
  using namespace dhd_stereo;
  if (!prev || !curr || !out || !inv_post_rot || !post_trans || !combine || !trans || !intrins || !post_rots || !u || !v || !dep)
    return DHD_EINVAL;
  if (!dhd_aligned(16, prev, curr, scratch) || !dhd_aligned(4, out, inv_post_rot, post_trans, combine, trans, intrins, post_rots, u, v, dep))
    return DHD_EINVAL;
  if (bn < 1 || c < 1 || h < 1 || w < 1 || n_depth < 1 || hi < 2 || wi < 2) return DHD_EINVAL;
  if ((layout != DHDV_NCHW && layout != DHDV_NHWC) || !sizes_supported(dtype, bn, c, h, w, n_depth) || flag_channel < 0 || flag_channel >= c)
    return DHD_EUNSUPPORTED;
  const size_t need = dhdv_stereo_cv_scratch_bytes(dtype, layout, bn, c, h, w);
  if (need > 0 && (!scratch || scratch_bytes < need)) return scratch ? DHD_ENOSPACE : DHD_EINVAL;
  const void *pl = prev, *cl = curr;
  if (layout == DHDV_NCHW) {     // [bn][c][h w] -> [bn][h w][c], each map once, in its own type
    char* s = static_cast<char*>(scratch);
    int rc = dhd_transpose_batched(prev, s, elem_bytes(dtype), bn, c, h * w, stream);
    if (rc == DHD_OK) rc = dhd_transpose_batched(curr, s + need / 2, elem_bytes(dtype), bn, c, h * w, stream);
    if (rc != DHD_OK) return rc;
    pl = s;
    cl = s + need / 2;
  }
  const Geom geo = {inv_post_rot, post_trans, combine, trans, intrins, post_rots, u, v, dep, 1.0f / (float)(wi - 1), 1.0f / (float)(hi - 1)};
  hipStream_t st = dhd_stream(stream);
  const int rc = dhd::with_dtype<dhd::NativeHalf>(dtype, [&](auto* p) {
    using T = std::remove_pointer_t<decltype(p)>;
    launch_cv<T>(static_cast<const T*>(pl), static_cast<const T*>(cl), geo, bn, c, h, w, n_depth, bias, flag_channel, static_cast<T*>(out), st);
    return DHD_OK;
  });
  if (rc != DHD_OK) return rc;
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

}  // extern "C"
