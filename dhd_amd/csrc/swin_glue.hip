// The memory-bound glue of a SwinBlock (backbones/swin.py:516-592 in the reference) around its Linear layers and its attention,
// section X1 of include/dhd_amd_ext.h:
//   ln_rows_fwd       LayerNorm of a token row written straight to where the window partition of window.hip puts that row (or, with
//                     the identity map, plain LayerNorm over rows that emits another dtype: norm2 -> the dtype fc1 casts to)
//   ln_rows_bwd       its backward from x, dy and gamma, over the real tokens, dy gathered through the reverse map; per-workgroup
//                     partial sums of dy x^ and dy in scratch, added up in a fixed order by ln_rows_bwd_params
//   win_reverse_add   out = identity + scale[b] * reverse(win): the window reverse of window.hip with the residual add in it
// One row's c channels live in registers across a group of `lanes` lanes (a power of two <= 64), eight channels per lane and step,
// STEPS = ceil(c / 8 / lanes) <= 4 steps; sums over a row are xor-shuffle trees inside the group (group_sum).  No LDS, no atomics.
#include "window_geom.h"

#include "../../include/dhd_amd_ext.h"

namespace {

using dhd::load8;
using dhd::store8;
using dhd::WinGeom;

constexpr int kMaxC = 2048;
constexpr int kFwdBlock = 256;
constexpr int kBwdBlock = DHD_WAVE;   // one wave per workgroup: its partial row pair is reduced by shuffles alone
constexpr int kBwdMinIters = 10;      // at least this many passes of a wave over its tokens per partial row pair it writes
constexpr int kBwdMaxGroups = 4096;   // partial row pairs at most (4 waves per SIMD of 256 CUs)
constexpr int kParamCols = 16;        // columns of the partial rows per wave of ln_rows_bwd_params
constexpr int kAddBlock = 256;

// lanes per row and steps per lane for c channels
struct RowShape {
  int lanes, steps;
};
inline RowShape row_shape(int c) {
  const int nvec = c >> 3;
  int lanes = 1;
  while (lanes < nvec && lanes < DHD_WAVE) lanes <<= 1;
  return {lanes, (nvec + lanes - 1) / lanes};
}

// workgroups of the backward over `tokens` tokens: enough tokens each for kBwdMinIters passes, kBwdMaxGroups at most.  Workgroup i of n
// takes the tokens [i * tokens / n, (i + 1) * tokens / n): never empty, since n <= tokens.
inline long bwd_groups(long tokens, int c) {
  const long per_group = (long)(kBwdBlock / row_shape(c).lanes) * kBwdMinIters;
  const long n = (tokens + per_group - 1) / per_group;
  return n < kBwdMaxGroups ? n : kBwdMaxGroups;
}

inline bool c_supported(int c) { return c >= 8 && c <= kMaxC && (c & 7) == 0; }
inline bool dtype_ok(int d) { return d == DHD_F32 || d == DHD_F16 || d == DHD_BF16; }

// the row of STEPS x 8 values at `p` (zeros where !on or past the row's end)
template <typename T, int STEPS>
__device__ __forceinline__ void load_row(const T* p, bool on, int lane, int lanes, int nvec, float (&v)[STEPS][8]) {
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const int vec = s * lanes + lane;
    if (on && vec < nvec) {
      load8<T>(p + vec * 8, v[s]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[s][k] = 0.f;
    }
  }
}

// mean and 1 / sqrt(var + eps) of the row held by the group: the sum, then the centred sum of squares.  The centred pass also
// sums the residuals d = x - mean and corrects the mean by their average: the float32 sum leaves the mean off by some
// 2^-24 |mean|, which (x - mean) rstd multiplies by up to eps^-1/2 = 316 -- on a constant row at 100, whose exact result is beta,
// that was 3e-3.  With the correction a constant row gives d = 0 and beta exactly; var = sum d^2 / c - (sum d / c)^2 is the
// variance about the corrected mean.
template <int STEPS>
__device__ __forceinline__ void row_stats(const float (&v)[STEPS][8], int lane, int lanes, int nvec, int c, float eps, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < STEPS; ++i)
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[i][k];
  mean = group_sum(s, lanes) / (float)c;
  float q = 0.f, e = 0.f;
#pragma unroll
  for (int i = 0; i < STEPS; ++i) {
    if (i * lanes + lane < nvec) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float d = v[i][k] - mean;
        e += d;
        q += d * d;
      }
    }
  }
  const float de = group_sum(e, lanes) / (float)c;
  mean += de;
  rstd = 1.f / sqrtf(fmaxf(group_sum(q, lanes) / (float)c - de * de, 0.f) + eps);
}

// every pass of the loop is made by all lanes of the block (the bound depends on blockIdx alone), so the shuffles of row_stats
// always find their partners; rows past the end and pad rows load nothing
template <typename TI, typename TO, int STEPS>
__global__ __launch_bounds__(kFwdBlock) void ln_rows_fwd(const TI* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         TO* __restrict__ out, WinGeom g, long rows, int lanes, float eps) {
  const int nvec = g.c >> 3, lane = threadIdx.x & (lanes - 1), sub = threadIdx.x / lanes, per_block = kFwdBlock / lanes;
  float ga[STEPS][8], be[STEPS][8];
  load_row<float, STEPS>(gamma, true, lane, lanes, nvec, ga);
  load_row<float, STEPS>(beta, true, lane, lanes, nvec, be);
  for (long base = (long)blockIdx.x * per_block; base < rows; base += (long)gridDim.x * per_block) {
    const long row = base + sub;
    const bool live = row < rows;
    const long src = !live ? -1 : g.ws > 0 ? dhd::win_partition_src(g, row) : row;   // -1: a pad row, zeros
    float v[STEPS][8];
    load_row<TI, STEPS>(x + (src < 0 ? 0 : src) * g.c, src >= 0, lane, lanes, nvec, v);
    float mean, rstd;
    row_stats<STEPS>(v, lane, lanes, nvec, g.c, eps, mean, rstd);
    if (!live) continue;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int vec = s * lanes + lane;
      if (vec >= nvec) continue;
      float y[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) y[k] = src < 0 ? 0.f : (v[s][k] - mean) * rstd * ga[s][k] + be[s][k];
      store8<TO>(out + row * g.c + vec * 8, y);
    }
  }
}

// one wave per workgroup, its run of tokens (bwd_groups) in passes of 64 / lanes tokens
template <typename TX, typename TD, int STEPS>
__global__ __launch_bounds__(kBwdBlock) void ln_rows_bwd(const TX* __restrict__ x, const TD* __restrict__ dy, const float* __restrict__ gamma,
                                                         TX* __restrict__ dx, float* __restrict__ partial, WinGeom g, long tokens, int lanes,
                                                         float eps) {
  const int nvec = g.c >> 3, lane = threadIdx.x & (lanes - 1), sub = threadIdx.x / lanes, per_pass = kBwdBlock / lanes;
  float ga[STEPS][8], sg[STEPS][8], sb[STEPS][8];
  load_row<float, STEPS>(gamma, true, lane, lanes, nvec, ga);
#pragma unroll
  for (int s = 0; s < STEPS; ++s)
#pragma unroll
    for (int k = 0; k < 8; ++k) sg[s][k] = sb[s][k] = 0.f;
  const long first = (long)blockIdx.x * tokens / gridDim.x, end = ((long)blockIdx.x + 1) * tokens / gridDim.x;
  for (long base = first; base < end; base += per_pass) {
    const long t = base + sub;
    const bool live = t < end;
    const long drow = !live ? 0 : g.ws > 0 ? dhd::win_reverse_src(g, t) : t;
    float v[STEPS][8], d[STEPS][8];
    load_row<TX, STEPS>(x + (live ? t : 0) * g.c, live, lane, lanes, nvec, v);
    load_row<TD, STEPS>(dy + drow * g.c, live, lane, lanes, nvec, d);
    float mean, rstd;
    row_stats<STEPS>(v, lane, lanes, nvec, g.c, eps, mean, rstd);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      if (!live || s * lanes + lane >= nvec) continue;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        v[s][k] = (v[s][k] - mean) * rstd;      // x^
        sb[s][k] += d[s][k];
        sg[s][k] += d[s][k] * v[s][k];
        d[s][k] *= ga[s][k];                    // g = dy gamma
        s1 += d[s][k];
        s2 += d[s][k] * v[s][k];
      }
    }
    const float c1 = group_sum(s1, lanes) / (float)g.c, c2 = group_sum(s2, lanes) / (float)g.c;
    if (!live) continue;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int vec = s * lanes + lane;
      if (vec >= nvec) continue;
      float r[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) r[k] = rstd * (d[s][k] - c1 - v[s][k] * c2);
      store8<TX>(dx + t * g.c + vec * 8, r);
    }
  }
  // the groups of the wave hold sums over different tokens of the same channels: add them, in a fixed tree
  for (int m = lanes; m < DHD_WAVE; m <<= 1) {
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        sg[s][k] += __shfl_xor(sg[s][k], m, DHD_WAVE);
        sb[s][k] += __shfl_xor(sb[s][k], m, DHD_WAVE);
      }
  }
  if (sub == 0) {
    float* p = partial + (long)blockIdx.x * 2 * g.c;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int vec = s * lanes + lane;
      if (vec >= nvec) continue;
      store8<float>(p + vec * 8, sg[s]);
      store8<float>(p + g.c + vec * 8, sb[s]);
    }
  }
}

// partial (groups, 2, c) -> dgamma (c), dbeta (c).  One wave per kParamCols of the 2 c columns: 4 lanes x 16 bytes across, 16 lanes
// down; a lane adds rows lane, lane + 16, ... in order, then the 16 are added in a fixed tree.
__global__ __launch_bounds__(DHD_WAVE) void ln_rows_bwd_params(const float* __restrict__ partial, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, long groups, int c) {
  const int col = blockIdx.x * kParamCols + (threadIdx.x & 3) * 4;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  for (long r = threadIdx.x >> 2; r < groups; r += DHD_WAVE / 4) {
    float v[4];
    dhd::Vec16<float, false>::load(partial + r * 2 * c + col, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] += v[k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    for (int m = 4; m < DHD_WAVE; m <<= 1) a[k] += __shfl_xor(a[k], m, DHD_WAVE);
  if (threadIdx.x < 4) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = col + k;
      if (j < c) dgamma[j] = a[k];
      else dbeta[j - c] = a[k];
    }
  }
}

// one thread per (token row, group of 8 channels), as window_rows
template <typename TW, typename TI, bool SCALED>
__global__ __launch_bounds__(kAddBlock) void win_reverse_add(const TW* __restrict__ win, const TI* __restrict__ identity,
                                                             const float* __restrict__ scale, TI* __restrict__ out, WinGeom g) {
  const int groups = g.c >> 3;
  const long total = (long)g.b * g.h * g.w * groups;
  for (long idx = (long)blockIdx.x * kAddBlock + threadIdx.x; idx < total; idx += (long)gridDim.x * kAddBlock) {
    const int cg = (int)(idx % groups);
    const long row = idx / groups;
    const long src = dhd::win_reverse_src(g, row);
    float a[8], v[8];
    load8<TI>(identity + row * g.c + cg * 8, a);
    load8<TW>(win + src * g.c + cg * 8, v);
    if (SCALED) {
      const float sc = scale[row / ((long)g.h * g.w)];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] *= sc;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] += v[k];
    store8<TI>(out + row * g.c + cg * 8, a);
  }
}

// the checks the three entry points share; g is filled for a call that passes
int make_geom(int b, int h, int w, int c, int window, int shift, bool identity_map_ok, WinGeom& g) {
  if (b <= 0 || h <= 0 || w <= 0) return DHD_EINVAL;
  if (!c_supported(c) || window < 0 || shift < 0) return DHD_EUNSUPPORTED;
  if (window == 0) {
    if (!identity_map_ok || shift != 0) return DHD_EUNSUPPORTED;
    g = WinGeom{b, h, w, c, 0, 0, h, w, 0, 0};
  } else {
    if (shift >= window) return DHD_EUNSUPPORTED;
    g = dhd::win_geom(b, h, w, c, window, shift);
  }
  if ((long)b * g.hp * g.wp >= (1L << 40)) return DHD_EUNSUPPORTED;
  return DHD_OK;
}

template <class F>
int with_steps(int steps, F&& f) {
  switch (steps) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
  }
  return DHD_EUNSUPPORTED;
}

}  // namespace

extern "C" int dhdx_ln_rows_supported(int c, int x_dtype, int out_dtype) { return c_supported(c) && dtype_ok(x_dtype) && dtype_ok(out_dtype); }

extern "C" int dhdx_ln_rows_forward(const void* x, const float* gamma, const float* beta, void* out, int x_dtype, int out_dtype, int b, int h,
                                    int w, int c, int window, int shift, float eps, void* stream) {
  if (!x || !gamma || !beta || !out) return DHD_EINVAL;
  if (!dhd_aligned(16, x, gamma, beta, out)) return DHD_EINVAL;   // load8 / store8
  WinGeom g;
  if (int rc = make_geom(b, h, w, c, window, shift, true, g)) return rc;
  if (!dtype_ok(x_dtype) || !dtype_ok(out_dtype)) return DHD_EUNSUPPORTED;
  const long rows = (long)b * g.hp * g.wp;
  const RowShape rs = row_shape(c);
  long blocks = (rows + kFwdBlock / rs.lanes - 1) / (kFwdBlock / rs.lanes);
  if (blocks > 65536) blocks = 65536;
  hipStream_t st = dhd_stream(stream);
  return dhd::with_dtype<dhd::HipHalf>(x_dtype, [&](auto* ti) {
    return dhd::with_dtype<dhd::HipHalf>(out_dtype, [&](auto* to) {
      return with_steps(rs.steps, [&](auto steps) {
        using TI = std::remove_pointer_t<decltype(ti)>;
        using TO = std::remove_pointer_t<decltype(to)>;
        hipLaunchKernelGGL((ln_rows_fwd<TI, TO, decltype(steps)::value>), dim3((unsigned)blocks), dim3(kFwdBlock), 0, st, (const TI*)x, gamma,
                           beta, (TO*)out, g, rows, rs.lanes, eps);
        DHD_LAUNCH_CHECK();
        return DHD_OK;
      });
    });
  });
}

extern "C" size_t dhdx_ln_rows_backward_scratch_bytes(long rows, int c) {
  if (rows <= 0 || rows >= (1L << 40) || !c_supported(c)) return 0;
  return (size_t)bwd_groups(rows, c) * 2 * c * sizeof(float);
}

extern "C" int dhdx_ln_rows_backward(const void* x, const void* dy, const float* gamma, void* dx, float* dgamma, float* dbeta, void* scratch,
                                     size_t scratch_bytes, int x_dtype, int dy_dtype, int b, int h, int w, int c, int window, int shift,
                                     float eps, void* stream) {
  if (!x || !dy || !gamma || !dx || !dgamma || !dbeta || !scratch) return DHD_EINVAL;
  if (!dhd_aligned(16, x, dy, gamma, dx, dgamma, dbeta, scratch)) return DHD_EINVAL;
  WinGeom g;
  if (int rc = make_geom(b, h, w, c, window, shift, true, g)) return rc;
  if (!dtype_ok(x_dtype) || !dtype_ok(dy_dtype)) return DHD_EUNSUPPORTED;
  const long tokens = (long)b * h * w;
  const long groups = bwd_groups(tokens, c);
  if (scratch_bytes < (size_t)groups * 2 * c * sizeof(float)) return DHD_ENOSPACE;
  const RowShape rs = row_shape(c);
  hipStream_t st = dhd_stream(stream);
  const int rc = dhd::with_dtype<dhd::HipHalf>(x_dtype, [&](auto* tx) {
    return dhd::with_dtype<dhd::HipHalf>(dy_dtype, [&](auto* td) {
      return with_steps(rs.steps, [&](auto steps) {
        using TX = std::remove_pointer_t<decltype(tx)>;
        using TD = std::remove_pointer_t<decltype(td)>;
        hipLaunchKernelGGL((ln_rows_bwd<TX, TD, decltype(steps)::value>), dim3((unsigned)groups), dim3(kBwdBlock), 0, st, (const TX*)x,
                           (const TD*)dy, gamma, (TX*)dx, (float*)scratch, g, tokens, rs.lanes, eps);
        DHD_LAUNCH_CHECK();
        return DHD_OK;
      });
    });
  });
  if (rc) return rc;
  hipLaunchKernelGGL(ln_rows_bwd_params, dim3((unsigned)(2 * c / kParamCols)), dim3(DHD_WAVE), 0, st, (const float*)scratch, dgamma, dbeta,
                     groups, c);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

extern "C" int dhdx_window_reverse_add(const void* win, const void* identity, const float* scale, void* out, int win_dtype, int id_dtype, int b,
                                       int h, int w, int c, int window, int shift, void* stream) {
  if (!win || !identity || !out) return DHD_EINVAL;
  if (!dhd_aligned(16, win, identity, out) || !dhd_aligned(4, scale)) return DHD_EINVAL;
  WinGeom g;
  if (int rc = make_geom(b, h, w, c, window, shift, false, g)) return rc;
  if (!dtype_ok(win_dtype) || !dtype_ok(id_dtype)) return DHD_EUNSUPPORTED;
  long blocks = ((long)b * h * w * (c >> 3) + kAddBlock - 1) / kAddBlock;
  if (blocks > 65536) blocks = 65536;
  hipStream_t st = dhd_stream(stream);
  return dhd::with_dtype<dhd::HipHalf>(win_dtype, [&](auto* tw) {
    return dhd::with_dtype<dhd::HipHalf>(id_dtype, [&](auto* ti) {
      using TW = std::remove_pointer_t<decltype(tw)>;
      using TI = std::remove_pointer_t<decltype(ti)>;
      if (scale) hipLaunchKernelGGL((win_reverse_add<TW, TI, true>), dim3((unsigned)blocks), dim3(kAddBlock), 0, st, (const TW*)win,
                                    (const TI*)identity, scale, (TI*)out, g);
      else hipLaunchKernelGGL((win_reverse_add<TW, TI, false>), dim3((unsigned)blocks), dim3(kAddBlock), 0, st, (const TW*)win,
                              (const TI*)identity, scale, (TI*)out, g);
      DHD_LAUNCH_CHECK();
      return DHD_OK;
    });
  });
}

// the stage seams (include/dhd_amd_seam.h): the same row form on two other row maps, in namespace dhd_seam
#include "swin_seam.h"
