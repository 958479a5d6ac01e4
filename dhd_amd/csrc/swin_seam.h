// The seams between the stages of a SwinTransformer (backbones/swin.py:79-241 in the reference), include/dhd_amd_seam.h.  Included by
// swin_glue.hip after its own kernels (no translation unit of its own: the list of translation units is a closed list held by
// tests/test_swin_ffn_capi.py); everything here lives in namespace dhd_seam, so nothing of swin_glue.hip is shadowed or changed.
//   merge_norm_fwd / _bwd   PatchMerging up to its Linear: the 2 x 2 gather into nn.Unfold's (c, kh, kw) channel order with the
//                           LayerNorm over the 4c gathered values in it.  A lane loads 16 bytes from each of the row's four source
//                           tokens and thereby holds a contiguous run of output channels (16 for float32 x, 32 for half x): the
//                           interleave is done in registers and both sides move as 16-byte vectors.  Sources past h or w are
//                           zeros that enter the statistics (the reference pads before this norm).
//   embed_norm_fwd / _bwd   PatchEmbed after its conv: LayerNorm over the channels of an NCHW map written as tokens.  A tile of
//                           pixels of one image is staged in LDS (float32, row stride tile + 1), the rows are normalised from
//                           there, and the backward puts dx back through the same tile.  Tiles never straddle an image.
//   seam_bwd_params         the partial rows (dy x^, dy) of either backward added up in a fixed order
// The rows are in the form of swin_glue.hip: a row in registers across a power-of-two group of lanes, the sum and then the
// centred sum of squares as xor-shuffle trees (group_sum), float32 throughout.  No atomics.
#pragma once
#include "window_geom.h"

#include "../../include/dhd_amd_seam.h"

namespace dhd_seam {
namespace {

using dhd::f32x2;
using dhd::kVec16;
using dhd::load8;
using dhd::Pair;
using dhd::store8;
using dhd::Vec16;

constexpr int kMergeMaxC = 512;       // 4c <= 2048
constexpr int kEmbedMaxC = 256;
constexpr int kBlock = 256;           // the forward kernels and the embed backward
constexpr int kBwdBlock = DHD_WAVE;   // merge backward: one wave per workgroup, its partial row pair is reduced by shuffles alone
constexpr int kBwdMinIters = 10;      // at least this many passes of a wave over its rows per partial row pair it writes
constexpr int kBwdMaxGroups = 4096;   // partial row pairs at most, merge
constexpr int kEmbedMinTiles = 4;     // tiles per workgroup of the embed backward at least (where there are that many)
constexpr int kEmbedMaxGroups = 2048; // partial row pairs at most, embed
constexpr int kParamCols = 16;        // columns of the partial rows per wave of seam_bwd_params

inline bool dtype_ok(int d) { return d == DHD_F32 || d == DHD_F16 || d == DHD_BF16; }
inline bool merge_c_ok(int c) { return c >= 8 && c <= kMergeMaxC && (c & 7) == 0; }
inline bool embed_c_ok(int c) { return c >= 8 && c <= kEmbedMaxC && (c & 7) == 0; }

struct RowShape {
  int lanes, steps;
};
// lanes per row (a power of two <= 64) and steps per lane for `units` 16-byte units
inline RowShape row_shape(int units) {
  int lanes = 1;
  while (lanes < units && lanes < DHD_WAVE) lanes <<= 1;
  return {lanes, (units + lanes - 1) / lanes};
}

// ---------------------------------------------------------------------------------------------------------------- merge

struct MergeGeom {
  int b, h, w, c, ho, wo;
};

// workgroups of the merge backward over `rows` output rows: sized for float32 x (the wider lane group), whatever x is, so that
// the scratch depends on (rows, c) alone.  Workgroup i of n takes the rows [i * rows / n, (i + 1) * rows / n): never empty.
inline long merge_bwd_groups(long rows, int c) {
  const long per_group = (long)(kBwdBlock / row_shape(c / 4).lanes) * kBwdMinIters;
  const long n = (rows + per_group - 1) / per_group;
  return n < kBwdMaxGroups ? n : kBwdMaxGroups;
}

// N contiguous floats <-> N elements of T, as 16-byte accesses
template <typename T, int N> __device__ __forceinline__ void load_run(const T* p, float* v) {
#pragma unroll
  for (int k = 0; k < N; k += kVec16<T>) Vec16<T, false>::load(p + k, v + k);
}
template <typename T, int N> __device__ __forceinline__ void store_run(T* p, const float* v) {
#pragma unroll
  for (int k = 0; k < N; k += kVec16<T>) Vec16<T, false>::store(p + k, v + k);
}

// The gathered row (bi, i, j) in source order: v[s][t * E + e] = x[bi, 2i + (t >> 1), 2j + (t & 1), (s lanes + lane) E + e], zeros
// where the source lies past h or w, where the unit lies past the row's end, or where !live.
template <typename TX, int STEPS>
__device__ __forceinline__ void merge_load(const TX* x, const MergeGeom& g, long bi, int i, int j, bool live, int lane, int lanes, int units,
                                           float (&v)[STEPS][4 * kVec16<TX>]) {
  constexpr int E = kVec16<TX>;
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const int u = s * lanes + lane;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int y = 2 * i + (t >> 1), xx = 2 * j + (t & 1);
      if (live && u < units && y < g.h && xx < g.w) {
        Vec16<TX, false>::load(x + ((bi * g.h + y) * g.w + xx) * g.c + u * E, v[s] + t * E);
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) v[s][t * E + e] = 0.f;
      }
    }
  }
}

// mean and 1 / sqrt(var + eps) over the n values of the row the group holds: the sum, then the centred sum of squares; the
// centred pass also sums the residuals and corrects the mean by their average (swin_glue.hip's row_stats says why: a constant row
// then gives exactly beta)
template <int STEPS, int N>
__device__ __forceinline__ void row_stats(const float (&v)[STEPS][N], int lane, int lanes, int units, int n, float eps, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < STEPS; ++i)
#pragma unroll
    for (int k = 0; k < N; ++k) s += v[i][k];
  mean = group_sum(s, lanes) / (float)n;
  float q = 0.f, e = 0.f;
#pragma unroll
  for (int i = 0; i < STEPS; ++i) {
    if (i * lanes + lane < units) {
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const float d = v[i][k] - mean;
        e += d;
        q += d * d;
      }
    }
  }
  const float de = group_sum(e, lanes) / (float)n;
  mean += de;
  rstd = 1.f / sqrtf(fmaxf(group_sum(q, lanes) / (float)n - de * de, 0.f) + eps);
}

// every pass of the loop is made by all lanes of the block (the bound depends on blockIdx alone), so the shuffles of row_stats
// always find their partners
template <typename TX, typename TO, int STEPS>
__global__ __launch_bounds__(kBlock) void merge_norm_fwd(const TX* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         TO* __restrict__ out, MergeGeom g, long rows, int lanes, float eps) {
  constexpr int E = kVec16<TX>, N = 4 * E;
  const int units = g.c / E, lane = threadIdx.x & (lanes - 1), sub = threadIdx.x / lanes, per_block = kBlock / lanes, n = 4 * g.c;
  float ga[STEPS][N], be[STEPS][N];
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const int u = s * lanes + lane;
    if (u < units) {
      load_run<float, N>(gamma + u * N, ga[s]);
      load_run<float, N>(beta + u * N, be[s]);
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k) ga[s][k] = be[s][k] = 0.f;
    }
  }
  for (long base = (long)blockIdx.x * per_block; base < rows; base += (long)gridDim.x * per_block) {
    const long row = base + sub;
    const bool live = row < rows;
    const int j = (int)(row % g.wo), i = (int)((row / g.wo) % g.ho);
    const long bi = row / ((long)g.wo * g.ho);
    float v[STEPS][N];
    merge_load<TX, STEPS>(x, g, bi, i, j, live, lane, lanes, units, v);
    float mean, rstd;
    row_stats<STEPS, N>(v, lane, lanes, units, n, eps, mean, rstd);
    if (!live) continue;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int u = s * lanes + lane;
      if (u >= units) continue;
      float y[N];
#pragma unroll
      for (int e = 0; e < E; ++e)
#pragma unroll
        for (int t = 0; t < 4; ++t) y[e * 4 + t] = (v[s][t * E + e] - mean) * rstd * ga[s][e * 4 + t] + be[s][e * 4 + t];
      store_run<TO, N>(out + row * n + (long)u * N, y);
    }
  }
}

// one wave per workgroup, its run of output rows (merge_bwd_groups) in passes of 64 / lanes rows
template <typename TX, typename TD, int STEPS>
__global__ __launch_bounds__(kBwdBlock) void merge_norm_bwd(const TX* __restrict__ x, const TD* __restrict__ dy, const float* __restrict__ gamma,
                                                            TX* __restrict__ dx, float* __restrict__ partial, MergeGeom g, long rows, int lanes,
                                                            float eps) {
  constexpr int E = kVec16<TX>, N = 4 * E;
  const int units = g.c / E, lane = threadIdx.x & (lanes - 1), sub = threadIdx.x / lanes, per_pass = kBwdBlock / lanes, n = 4 * g.c;
  float ga[STEPS][N], sg[STEPS][N], sb[STEPS][N];
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const int u = s * lanes + lane;
    if (u < units) load_run<float, N>(gamma + u * N, ga[s]);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      sg[s][k] = sb[s][k] = 0.f;
      if (u >= units) ga[s][k] = 0.f;
    }
  }
  const long first = (long)blockIdx.x * rows / gridDim.x, end = ((long)blockIdx.x + 1) * rows / gridDim.x;
  for (long base = first; base < end; base += per_pass) {
    const long row = base + sub;
    const bool live = row < end;
    const int j = (int)(row % g.wo), i = (int)((row / g.wo) % g.ho);
    const long bi = row / ((long)g.wo * g.ho);
    float v[STEPS][N], d[STEPS][N];
    merge_load<TX, STEPS>(x, g, bi, i, j, live, lane, lanes, units, v);
    float mean, rstd;
    row_stats<STEPS, N>(v, lane, lanes, units, n, eps, mean, rstd);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int u = s * lanes + lane;
      if (!live || u >= units) continue;
      load_run<TD, N>(dy + row * n + (long)u * N, d[s]);
      float xh[N];
#pragma unroll
      for (int e = 0; e < E; ++e)
#pragma unroll
        for (int t = 0; t < 4; ++t) xh[e * 4 + t] = (v[s][t * E + e] - mean) * rstd;      // x^ in the output's channel order
#pragma unroll
      for (int k = 0; k < N; ++k) {
        v[s][k] = xh[k];
        sb[s][k] += d[s][k];
        sg[s][k] += d[s][k] * xh[k];
        d[s][k] *= ga[s][k];                    // g = dy gamma
        s1 += d[s][k];
        s2 += d[s][k] * xh[k];
      }
    }
    const float c1 = group_sum(s1, lanes) / (float)n, c2 = group_sum(s2, lanes) / (float)n;
    if (!live) continue;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int u = s * lanes + lane;
      if (u >= units) continue;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int y = 2 * i + (t >> 1), xx = 2 * j + (t & 1);
        if (y >= g.h || xx >= g.w) continue;    // a pad source: part of the row's sums, no element of dx
        float r[E];
#pragma unroll
        for (int e = 0; e < E; ++e) r[e] = rstd * (d[s][e * 4 + t] - c1 - v[s][e * 4 + t] * c2);
        Vec16<TX, false>::store(dx + ((bi * g.h + y) * g.w + xx) * g.c + u * E, r);
      }
    }
  }
  // the groups of the wave hold sums over different rows of the same channels: add them, in a fixed tree
  for (int m = lanes; m < DHD_WAVE; m <<= 1) {
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
#pragma unroll
      for (int k = 0; k < N; ++k) {
        sg[s][k] += __shfl_xor(sg[s][k], m, DHD_WAVE);
        sb[s][k] += __shfl_xor(sb[s][k], m, DHD_WAVE);
      }
  }
  if (sub == 0) {
    float* p = partial + (long)blockIdx.x * 2 * n;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int u = s * lanes + lane;
      if (u >= units) continue;
      store_run<float, N>(p + u * N, sg[s]);
      store_run<float, N>(p + n + u * N, sb[s]);
    }
  }
}

// partial (groups, 2, n) -> dgamma (n), dbeta (n).  One wave per kParamCols of the 2 n columns: 4 lanes x 16 bytes across, 16 lanes
// down; a lane adds rows lane, lane + 16, ... in order, then the 16 are added in a fixed tree.
__global__ __launch_bounds__(DHD_WAVE) void seam_bwd_params(const float* __restrict__ partial, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, long groups, int n) {
  const int col = blockIdx.x * kParamCols + (threadIdx.x & 3) * 4;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  for (long r = threadIdx.x >> 2; r < groups; r += DHD_WAVE / 4) {
    float v[4];
    Vec16<float, false>::load(partial + r * 2 * n + col, v);
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
      if (j < n) dgamma[j] = a[k];
      else dbeta[j - n] = a[k];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- embed

// pixels per tile: the float32 tile of c x (tile + 1) stays under 34 KB, four workgroups to a CU
inline int embed_tile(int c) { return c <= 128 ? 64 : 32; }
inline size_t embed_lds_bytes(int c) { return (size_t)c * (embed_tile(c) + 1) * sizeof(float); }

// workgroups of the embed backward: from the token count alone (the scratch is asked for with it), at most one per tile that a
// map of that many tokens has at least -- b ceil(hw / tile) >= ceil(b hw / tile) -- so no workgroup is without a tile
inline long embed_bwd_groups(long tokens, int c) {
  const long per_group = (long)embed_tile(c) * kEmbedMinTiles;
  const long n = (tokens + per_group - 1) / per_group;
  return n < kEmbedMaxGroups ? n : kEmbedMaxGroups;
}

// one element <-> float, rounding as Vec16 rounds
template <class T> __device__ __forceinline__ float load1(const T* p) {
  if constexpr (std::is_same_v<T, float>) return *p;
  else return Pair<T>::widen((unsigned)*reinterpret_cast<const unsigned short*>(p)).x;
}
template <class T> __device__ __forceinline__ void store1(T* p, float v) {
  if constexpr (std::is_same_v<T, float>) *p = v;
  else *reinterpret_cast<unsigned short*>(p) = (unsigned short)(Pair<T>::narrow(f32x2{v, 0.f}) & 0xffffu);
}

// np pixels from p0 of the c channel planes at xb (each hw long) -> tile[ch * (P + 1) + p].  WIDE: hw is a multiple of the
// elements in 16 bytes, so every plane and every tile starts on a 16-byte boundary and np is a whole number of vectors.
template <typename T, bool WIDE>
__device__ __forceinline__ void stage_in(const T* xb, float* tile, int c, long hw, long p0, int np, int P) {
  const int S = P + 1;
  if constexpr (WIDE) {
    constexpr int E = kVec16<T>;
    const int chunks = P / E;
    for (int idx = threadIdx.x; idx < c * chunks; idx += kBlock) {
      const int ch = idx / chunks, p = (idx % chunks) * E;
      if (p >= np) continue;
      float f[E];
      Vec16<T, false>::load(xb + ch * hw + p0 + p, f);
#pragma unroll
      for (int e = 0; e < E; ++e) tile[ch * S + p + e] = f[e];
    }
  } else {
    for (int idx = threadIdx.x; idx < c * P; idx += kBlock) {
      const int ch = idx / P, p = idx % P;
      if (p < np) tile[ch * S + p] = load1<T>(xb + ch * hw + p0 + p);
    }
  }
}
template <typename T, bool WIDE>
__device__ __forceinline__ void stage_out(T* xb, const float* tile, int c, long hw, long p0, int np, int P) {
  const int S = P + 1;
  if constexpr (WIDE) {
    constexpr int E = kVec16<T>;
    const int chunks = P / E;
    for (int idx = threadIdx.x; idx < c * chunks; idx += kBlock) {
      const int ch = idx / chunks, p = (idx % chunks) * E;
      if (p >= np) continue;
      float f[E];
#pragma unroll
      for (int e = 0; e < E; ++e) f[e] = tile[ch * S + p + e];
      Vec16<T, false>::store(xb + ch * hw + p0 + p, f);
    }
  } else {
    for (int idx = threadIdx.x; idx < c * P; idx += kBlock) {
      const int ch = idx / P, p = idx % P;
      if (p < np) store1<T>(xb + ch * hw + p0 + p, tile[ch * S + p]);
    }
  }
}

// a workgroup per tile of P pixels of one image (grid-stride); a pixel's c channels across `lanes` <= 32 lanes, eight each
template <typename TX, typename TO, bool WIDE>
__global__ __launch_bounds__(kBlock) void embed_norm_fwd(const TX* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         TO* __restrict__ out, int c, long hw, int P, long tiles_per_image, long tiles, int lanes,
                                                         float eps) {
  extern __shared__ float tile[];
  const int S = P + 1, nvec = c >> 3, lane = threadIdx.x & (lanes - 1), sub = threadIdx.x / lanes, per_pass = kBlock / lanes;
  const bool mine = lane < nvec;
  float ga[1][8], be[1][8];
#pragma unroll
  for (int k = 0; k < 8; ++k) ga[0][k] = be[0][k] = 0.f;
  if (mine) {
    load8<float>(gamma + lane * 8, ga[0]);
    load8<float>(beta + lane * 8, be[0]);
  }
  for (long ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
    const long bi = ti / tiles_per_image, p0 = (ti % tiles_per_image) * P;
    const int np = (int)(hw - p0 < P ? hw - p0 : P);
    stage_in<TX, WIDE>(x + bi * c * hw, tile, c, hw, p0, np, P);
    __syncthreads();
    for (int pb = 0; pb < np; pb += per_pass) {
      const int p = pb + sub;
      const bool live = p < np;
      float v[1][8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[0][k] = live && mine ? tile[(lane * 8 + k) * S + p] : 0.f;
      float mean, rstd;
      row_stats<1, 8>(v, lane, lanes, nvec, c, eps, mean, rstd);
      if (!live || !mine) continue;
      float y[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) y[k] = (v[0][k] - mean) * rstd * ga[0][k] + be[0][k];
      store8<TO>(out + (bi * hw + p0 + p) * c + lane * 8, y);
    }
    __syncthreads();    // the next tile is staged over this one
  }
}

// workgroup i of n takes the tiles [i * tiles / n, (i + 1) * tiles / n); dx goes back through the tile
template <typename TX, typename TD, bool WIDE>
__global__ __launch_bounds__(kBlock) void embed_norm_bwd(const TX* __restrict__ x, const TD* __restrict__ dy, const float* __restrict__ gamma,
                                                         TX* __restrict__ dx, float* __restrict__ partial, int c, long hw, int P,
                                                         long tiles_per_image, long tiles, int lanes, float eps) {
  extern __shared__ float tile[];
  const int S = P + 1, nvec = c >> 3, lane = threadIdx.x & (lanes - 1), sub = threadIdx.x / lanes, per_pass = kBlock / lanes;
  const bool mine = lane < nvec;
  float ga[8], sg[8], sb[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) ga[k] = sg[k] = sb[k] = 0.f;
  if (mine) load8<float>(gamma + lane * 8, ga);
  const long first = (long)blockIdx.x * tiles / gridDim.x, end = ((long)blockIdx.x + 1) * tiles / gridDim.x;
  for (long ti = first; ti < end; ++ti) {
    const long bi = ti / tiles_per_image, p0 = (ti % tiles_per_image) * P;
    const int np = (int)(hw - p0 < P ? hw - p0 : P);
    stage_in<TX, WIDE>(x + bi * c * hw, tile, c, hw, p0, np, P);
    __syncthreads();
    for (int pb = 0; pb < np; pb += per_pass) {
      const int p = pb + sub;
      const bool live = p < np;
      float v[1][8], d[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        v[0][k] = live && mine ? tile[(lane * 8 + k) * S + p] : 0.f;
        d[k] = 0.f;
      }
      float mean, rstd;
      row_stats<1, 8>(v, lane, lanes, nvec, c, eps, mean, rstd);
      float s1 = 0.f, s2 = 0.f;
      if (live && mine) {
        load8<TD>(dy + (bi * hw + p0 + p) * c + lane * 8, d);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          v[0][k] = (v[0][k] - mean) * rstd;    // x^
          sb[k] += d[k];
          sg[k] += d[k] * v[0][k];
          d[k] *= ga[k];                        // g = dy gamma
          s1 += d[k];
          s2 += d[k] * v[0][k];
        }
      }
      const float c1 = group_sum(s1, lanes) / (float)c, c2 = group_sum(s2, lanes) / (float)c;
      if (!live || !mine) continue;
#pragma unroll
      for (int k = 0; k < 8; ++k) tile[(lane * 8 + k) * S + p] = rstd * (d[k] - c1 - v[0][k] * c2);   // over the x it read itself
    }
    __syncthreads();
    stage_out<TX, WIDE>(dx + bi * c * hw, tile, c, hw, p0, np, P);
    __syncthreads();
  }
  // the groups of a wave hold sums over different pixels of the same channels: add them in a fixed tree, then the four waves in order
  for (int m = lanes; m < DHD_WAVE; m <<= 1) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      sg[k] += __shfl_xor(sg[k], m, DHD_WAVE);
      sb[k] += __shfl_xor(sb[k], m, DHD_WAVE);
    }
  }
  const int wave = threadIdx.x / DHD_WAVE;
  if ((threadIdx.x & (DHD_WAVE - 1)) < lanes && mine) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      tile[wave * 2 * c + lane * 8 + k] = sg[k];
      tile[wave * 2 * c + c + lane * 8 + k] = sb[k];
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 2 * c; j += kBlock) {
    float a = tile[j];
    for (int w = 1; w < kBlock / DHD_WAVE; ++w) a += tile[w * 2 * c + j];
    partial[(long)blockIdx.x * 2 * c + j] = a;
  }
}

template <class F>
int with_steps(int steps, F&& f) {
  switch (steps) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
  }
  return DHD_EUNSUPPORTED;
}

// the checks the two merge entry points share; g is filled for a call that passes
int merge_geom(int b, int h, int w, int c, MergeGeom& g) {
  if (b <= 0 || h <= 0 || w <= 0) return DHD_EINVAL;
  if (!merge_c_ok(c)) return DHD_EUNSUPPORTED;
  g = MergeGeom{b, h, w, c, (h + 1) / 2, (w + 1) / 2};
  if ((long)b * h * w >= (1L << 40)) return DHD_EUNSUPPORTED;
  return DHD_OK;
}

int embed_geom(int b, int c, long hw) {
  if (b <= 0 || hw <= 0) return DHD_EINVAL;
  if (!embed_c_ok(c)) return DHD_EUNSUPPORTED;
  if (hw >= (1L << 40) || (long)b * hw >= (1L << 40)) return DHD_EUNSUPPORTED;
  return DHD_OK;
}

int launch_params(const float* scratch, float* dgamma, float* dbeta, long groups, int n, hipStream_t st) {
  hipLaunchKernelGGL(seam_bwd_params, dim3((unsigned)(2 * n / kParamCols)), dim3(DHD_WAVE), 0, st, scratch, dgamma, dbeta, groups, n);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

}  // namespace

extern "C" int dhds_merge_norm_supported(int c, int x_dtype, int out_dtype) { return merge_c_ok(c) && dtype_ok(x_dtype) && dtype_ok(out_dtype); }

extern "C" int dhds_merge_norm_forward(const void* x, const float* gamma, const float* beta, void* out, int x_dtype, int out_dtype, int b, int h,
                                       int w, int c, float eps, void* stream) {
  if (!x || !gamma || !beta || !out) return DHD_EINVAL;
  if (!dhd_aligned(16, x, gamma, beta, out)) return DHD_EINVAL;
  MergeGeom g;
  if (int rc = merge_geom(b, h, w, c, g)) return rc;
  if (!dtype_ok(x_dtype) || !dtype_ok(out_dtype)) return DHD_EUNSUPPORTED;
  const long rows = (long)b * g.ho * g.wo;
  hipStream_t st = dhd_stream(stream);
  return dhd::with_dtype<dhd::HipHalf>(x_dtype, [&](auto* ti) {
    using TI = std::remove_pointer_t<decltype(ti)>;
    const RowShape rs = row_shape(c / kVec16<TI>);
    long blocks = (rows + kBlock / rs.lanes - 1) / (kBlock / rs.lanes);
    if (blocks > 65536) blocks = 65536;
    return dhd::with_dtype<dhd::HipHalf>(out_dtype, [&](auto* to) {
      return with_steps(rs.steps, [&](auto steps) {
        using TO = std::remove_pointer_t<decltype(to)>;
        hipLaunchKernelGGL((merge_norm_fwd<TI, TO, decltype(steps)::value>), dim3((unsigned)blocks), dim3(kBlock), 0, st, (const TI*)x, gamma,
                           beta, (TO*)out, g, rows, rs.lanes, eps);
        DHD_LAUNCH_CHECK();
        return DHD_OK;
      });
    });
  });
}

extern "C" size_t dhds_merge_norm_backward_scratch_bytes(long out_rows, int c) {
  if (out_rows <= 0 || out_rows >= (1L << 40) || !merge_c_ok(c)) return 0;
  return (size_t)merge_bwd_groups(out_rows, c) * 2 * 4 * c * sizeof(float);
}

extern "C" int dhds_merge_norm_backward(const void* x, const void* dy, const float* gamma, void* dx, float* dgamma, float* dbeta, void* scratch,
                                        size_t scratch_bytes, int x_dtype, int dy_dtype, int b, int h, int w, int c, float eps, void* stream) {
  if (!x || !dy || !gamma || !dx || !dgamma || !dbeta || !scratch) return DHD_EINVAL;
  if (!dhd_aligned(16, x, dy, gamma, dx, dgamma, dbeta, scratch)) return DHD_EINVAL;
  MergeGeom g;
  if (int rc = merge_geom(b, h, w, c, g)) return rc;
  if (!dtype_ok(x_dtype) || !dtype_ok(dy_dtype)) return DHD_EUNSUPPORTED;
  const long rows = (long)b * g.ho * g.wo;
  const long groups = merge_bwd_groups(rows, c);
  if (scratch_bytes < (size_t)groups * 2 * 4 * c * sizeof(float)) return DHD_ENOSPACE;
  hipStream_t st = dhd_stream(stream);
  const int rc = dhd::with_dtype<dhd::HipHalf>(x_dtype, [&](auto* tx) {
    using TX = std::remove_pointer_t<decltype(tx)>;
    const RowShape rs = row_shape(c / kVec16<TX>);
    return dhd::with_dtype<dhd::HipHalf>(dy_dtype, [&](auto* td) {
      return with_steps(rs.steps, [&](auto steps) {
        using TD = std::remove_pointer_t<decltype(td)>;
        hipLaunchKernelGGL((merge_norm_bwd<TX, TD, decltype(steps)::value>), dim3((unsigned)groups), dim3(kBwdBlock), 0, st, (const TX*)x,
                           (const TD*)dy, gamma, (TX*)dx, (float*)scratch, g, rows, rs.lanes, eps);
        DHD_LAUNCH_CHECK();
        return DHD_OK;
      });
    });
  });
  if (rc) return rc;
  return launch_params((const float*)scratch, dgamma, dbeta, groups, 4 * c, st);
}

extern "C" int dhds_embed_norm_supported(int c, int x_dtype, int out_dtype) { return embed_c_ok(c) && dtype_ok(x_dtype) && dtype_ok(out_dtype); }

extern "C" int dhds_embed_norm_forward(const void* x, const float* gamma, const float* beta, void* out, int x_dtype, int out_dtype, int b, int c,
                                       long hw, float eps, void* stream) {
  if (!x || !gamma || !beta || !out) return DHD_EINVAL;
  if (!dhd_aligned(16, x, gamma, beta, out)) return DHD_EINVAL;
  if (int rc = embed_geom(b, c, hw)) return rc;
  if (!dtype_ok(x_dtype) || !dtype_ok(out_dtype)) return DHD_EUNSUPPORTED;
  const int P = embed_tile(c), lanes = row_shape(c >> 3).lanes;
  const long tiles_per_image = (hw + P - 1) / P, tiles = tiles_per_image * b;
  const long blocks = tiles < (1L << 20) ? tiles : (1L << 20);
  hipStream_t st = dhd_stream(stream);
  return dhd::with_dtype<dhd::HipHalf>(x_dtype, [&](auto* ti) {
    using TI = std::remove_pointer_t<decltype(ti)>;
    const bool wide = hw % kVec16<TI> == 0;
    return dhd::with_dtype<dhd::HipHalf>(out_dtype, [&](auto* to) {
      using TO = std::remove_pointer_t<decltype(to)>;
      if (wide) hipLaunchKernelGGL((embed_norm_fwd<TI, TO, true>), dim3((unsigned)blocks), dim3(kBlock), embed_lds_bytes(c), st, (const TI*)x,
                                   gamma, beta, (TO*)out, c, hw, P, tiles_per_image, tiles, lanes, eps);
      else hipLaunchKernelGGL((embed_norm_fwd<TI, TO, false>), dim3((unsigned)blocks), dim3(kBlock), embed_lds_bytes(c), st, (const TI*)x,
                              gamma, beta, (TO*)out, c, hw, P, tiles_per_image, tiles, lanes, eps);
      DHD_LAUNCH_CHECK();
      return DHD_OK;
    });
  });
}

extern "C" size_t dhds_embed_norm_backward_scratch_bytes(long tokens, int c) {
  if (tokens <= 0 || tokens >= (1L << 40) || !embed_c_ok(c)) return 0;
  return (size_t)embed_bwd_groups(tokens, c) * 2 * c * sizeof(float);
}

extern "C" int dhds_embed_norm_backward(const void* x, const void* dy, const float* gamma, void* dx, float* dgamma, float* dbeta, void* scratch,
                                        size_t scratch_bytes, int x_dtype, int dy_dtype, int b, int c, long hw, float eps, void* stream) {
  if (!x || !dy || !gamma || !dx || !dgamma || !dbeta || !scratch) return DHD_EINVAL;
  if (!dhd_aligned(16, x, dy, gamma, dx, dgamma, dbeta, scratch)) return DHD_EINVAL;
  if (int rc = embed_geom(b, c, hw)) return rc;
  if (!dtype_ok(x_dtype) || !dtype_ok(dy_dtype)) return DHD_EUNSUPPORTED;
  const long groups = embed_bwd_groups((long)b * hw, c);
  if (scratch_bytes < (size_t)groups * 2 * c * sizeof(float)) return DHD_ENOSPACE;
  const int P = embed_tile(c), lanes = row_shape(c >> 3).lanes;
  const long tiles_per_image = (hw + P - 1) / P, tiles = tiles_per_image * b;
  hipStream_t st = dhd_stream(stream);
  const int rc = dhd::with_dtype<dhd::HipHalf>(x_dtype, [&](auto* tx) {
    using TX = std::remove_pointer_t<decltype(tx)>;
    const bool wide = hw % kVec16<TX> == 0;
    return dhd::with_dtype<dhd::HipHalf>(dy_dtype, [&](auto* td) {
      using TD = std::remove_pointer_t<decltype(td)>;
      if (wide) hipLaunchKernelGGL((embed_norm_bwd<TX, TD, true>), dim3((unsigned)groups), dim3(kBlock), embed_lds_bytes(c), st, (const TX*)x,
                                   (const TD*)dy, gamma, (TX*)dx, (float*)scratch, c, hw, P, tiles_per_image, tiles, lanes, eps);
      else hipLaunchKernelGGL((embed_norm_bwd<TX, TD, false>), dim3((unsigned)groups), dim3(kBlock), embed_lds_bytes(c), st, (const TX*)x,
                              (const TD*)dy, gamma, (TX*)dx, (float*)scratch, c, hw, P, tiles_per_image, tiles, lanes, eps);
      DHD_LAUNCH_CHECK();
      return DHD_OK;
    });
  });
  if (rc) return rc;
  return launch_params((const float*)scratch, dgamma, dbeta, groups, c, st);
}

}  // namespace dhd_seam
