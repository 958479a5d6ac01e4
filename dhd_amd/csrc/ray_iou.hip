// RayIoU evaluation (core/evaluation/ray_metrics.py + lib/dvr/dvr.cu:70-319 of the reference): a voxel ray caster and the
// metric's counters, on the device.
//
// The reference's render_forward_cuda_kernel is the forward of a differentiable renderer: it records the whole path of a ray
// (four arrays of 1446 entries per thread) and then, in "test" phase, returns only the first occupied voxel on the path, or the
// last voxel inside the grid.  That result is O(1) state, so the walk here keeps the current candidate and stops at the first
// hit; every arithmetic operation of the traversal (double precision, no contraction: the Makefile's -ffp-contract=off) and
// every comparison is the published kernel's, in its order, so the two agree bit for bit on the same float32 inputs.
//
//   walk()                 one ray through one grid (Amanatides-Woo, strict-< axis cascade, bounded by kMaxStep)
//   ray_render_forward     the seam-level drop-in: float sigma (N,T,Z,Y,X), origins and end points in voxel units
//   ray_iou_bytes<O>       the product form: uint8 class grids (S,nx,ny,nz), (sample, origin in metres) pairs, both grids in
//                          one thread, labels, thresholds and int64 counters; per-ray results never leave the registers
#include <float.h>

#include "common.h"

namespace {

constexpr int kMaxStep = 1000;     // MAX_STEP of dvr.cu:13; no input makes a ray take more than kMaxStep + 1 iterations
constexpr int kMaxClasses = 32;
constexpr int kMaxThr = 4;
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;

struct Hit {
  int x, y, z;
  double d;        // ray parameter (voxel units) at which (x, y, z) is left
  bool entered;    // false: the ray never was inside the grid (the caller keeps the initial values)
};

// dvr.cu:113-307 with the path arrays folded away.  occ(x, y, z) is asked once per voxel inside the grid.
// A zero-length ray has NaN directions: every comparison below is false, z steps down, and the step bound ends the loop.
template <class Occ>
__device__ __forceinline__ Hit walk(double xo, double yo, double zo, double xe, double ye, double ze, int nx, int ny, int nz,
                                    const Occ& occ) {
  int vx = (int)xo, vy = (int)yo, vz = (int)zo;
  const double rx = xe - xo, ry = ye - yo, rz = ze - zo;
  const double len = sqrt(rx * rx + ry * ry + rz * rz);
  const double dx = rx / len, dy = ry / len, dz = rz / len;
  const int sx = (dx >= 0) ? 1 : -1, sy = (dy >= 0) ? 1 : -1, sz = (dz >= 0) ? 1 : -1;
  const double bx = vx + (sx < 0 ? 0 : 1), by = vy + (sy < 0 ? 0 : 1), bz = vz + (sz < 0 ? 0 : 1);
  double tx = (dx != 0) ? (bx - xo) / dx : DBL_MAX;
  double ty = (dy != 0) ? (by - yo) / dy : DBL_MAX;
  double tz = (dz != 0) ? (bz - zo) / dz : DBL_MAX;
  const double ddx = (dx != 0) ? sx / dx : DBL_MAX;
  const double ddy = (dy != 0) ? sy / dy : DBL_MAX;
  const double ddz = (dz != 0) ? sz / dz : DBL_MAX;

  Hit h = {0, 0, 0, 0.0, false};
  for (int step = 0; step <= kMaxStep; ++step) {
    const bool inside = (0 <= vx && vx < nx) && (0 <= vy && vy < ny) && (0 <= vz && vz < nz);
    if (!inside && h.entered) break;   // was inside, left: it does not come back
    const int cx = vx, cy = vy, cz = vz;
    double d;
    if (tx < ty) {
      if (tx < tz) { d = tx; vx += sx; tx += ddx; }
      else         { d = tz; vz += sz; tz += ddz; }
    } else {
      if (ty < tz) { d = ty; vy += sy; ty += ddy; }
      else         { d = tz; vz += sz; tz += ddz; }
    }
    if (inside) {
      h.entered = true;
      h.x = cx; h.y = cy; h.z = cz; h.d = d;     // last voxel inside, unless a hit ends the walk here
      if (occ(cx, cy, cz)) break;
    }
  }
  return h;
}

struct FloatSigma {   // (Z, Y, X) float, occupied where sigma > 0.5 (dvr.cu:274-275)
  const float* s;
  int ny, nx;
  __device__ __forceinline__ bool operator()(int x, int y, int z) const { return (double)s[((long)z * ny + y) * nx + x] > 0.5; }
};

struct ByteLabels {   // (nx, ny, nz) class ids, occupied where id < free_id (ray_metrics.py:88-91)
  const uint8_t* g;
  int ny, nz, free_id;
  __device__ __forceinline__ bool operator()(int x, int y, int z) const { return (int)g[((long)x * ny + y) * nz + z] < free_id; }
};

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ray_render_forward(const float* __restrict__ sigma, const float* __restrict__ origin,
                                                             const float* __restrict__ points, const float* __restrict__ tindex,
                                                             int t_sigma, int t_origin, int m, int nz, int ny, int nx,
                                                             float* __restrict__ pred_dist, float* __restrict__ gt_dist,
                                                             float* __restrict__ coord_index) {
  const int n = blockIdx.y;
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= m) return;
  const long ray = (long)n * m + c;
  float pd = -1.f, gd = -1.f, ix = 0.f, iy = 0.f, iz = 0.f;
  const float tf = tindex[ray];
  const int t = (tf >= 0.f && tf < (float)t_origin) ? (int)tf : -1;   // t < 0 (or NaN): padded ray
  if (t >= 0 && (t_sigma == 1 || t < t_sigma)) {
    const float* o = origin + ((long)n * t_origin + t) * 3;
    const float* e = points + ray * 3;
    const FloatSigma occ = {sigma + ((long)n * t_sigma + (t_sigma == 1 ? 0 : t)) * nz * ny * nx, ny, nx};
    const double xo = o[0], yo = o[1], zo = o[2], xe = e[0], ye = e[1], ze = e[2];
    const Hit h = walk(xo, yo, zo, xe, ye, ze, nx, ny, nz, occ);
    if (h.entered) {
      const double rx = xe - xo, ry = ye - yo, rz = ze - zo;
      pd = (float)h.d;
      gd = (float)sqrt(rx * rx + ry * ry + rz * rz);
      ix = (float)h.x; iy = (float)h.y; iz = (float)h.z;
    }
  }
  pred_dist[ray] = pd;
  gt_dist[ray] = gd;
  coord_index[ray * 3 + 0] = ix;
  coord_index[ray * 3 + 1] = iy;
  coord_index[ray * 3 + 2] = iz;
}

// ------------------------------------------------------------------------------------------------
struct IouParams {
  const uint8_t* pred;
  const uint8_t* gt;
  const int32_t* sample_id;
  const void* origins;
  const float* rays;
  unsigned long long* counts;
  int n_samples, nx, ny, nz, n_pairs, n_rays, free_id, n_classes, n_thr;
  float lower[3], voxel, thr[kMaxThr];
};

// ray_metrics.py:101-105: end point = ray + origin, then (p - offset) / scaler with float32 offset / scaler tensors, cast to
// float32.  O = double: torch promotes, the chain is float64 with the float32 constants widened, rounded once at the end.
// O = float: every operation is float32.
template <class O>
__device__ __forceinline__ void to_voxel_units(const O* org, const float* ray, const IouParams& p, double o[3], double e[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const O end = (O)ray[a] + org[a];
    o[a] = (double)(float)((org[a] - (O)p.lower[a]) / (O)p.voxel);
    e[a] = (double)(float)((end - (O)p.lower[a]) / (O)p.voxel);
  }
}

// ray_metrics.py:117,127: distance in metres (float32 product) and the label at coord_index; a ray that never entered keeps
// pred_dist = -1 and coord_index = (0, 0, 0).
__device__ __forceinline__ void label_and_dist(const Hit& h, const uint8_t* grid, const IouParams& p, int& label, float& dist) {
  const long idx = h.entered ? ((long)h.x * p.ny + h.y) * p.nz + h.z : 0;
  label = grid[idx];
  dist = (h.entered ? (float)h.d : -1.f) * p.voxel;
}

// calc_metrics (ray_metrics.py:138-172) for one ray per lane: class by class the wave counts its lanes with a ballot and one
// lane adds the sums to the block's LDS counters.  Called by whole waves (`valid` masks the lanes that have no ray).
__device__ __forceinline__ void count_wave(bool valid, int gl, int pl, float dp, float dg, const IouParams& p, unsigned* cnt) {
  valid = valid && gl != p.free_id;      // rays are evaluated where the ground truth is not free (:191)
  const float err = fabsf(dp - dg);
  const bool lane0 = (threadIdx.x & (DHD_WAVE - 1)) == 0;
  const unsigned long long classes = __ballot(valid);
  if (classes == 0) return;
  for (int c = 0; c < p.n_classes; ++c) {
    const bool g = valid && gl == c, q = valid && pl == c;
    const int ng = __popcll(__ballot(g)), nq = __popcll(__ballot(q));
    if (ng == 0 && nq == 0) continue;
    if (lane0) {
      if (ng) atomicAdd(&cnt[c], (unsigned)ng);
      if (nq) atomicAdd(&cnt[p.n_classes + c], (unsigned)nq);
    }
    if (__ballot(g && q) == 0) continue;
    for (int j = 0; j < p.n_thr; ++j) {
      const int nt = __popcll(__ballot(g && q && err < p.thr[j]));
      if (lane0 && nt) atomicAdd(&cnt[(2 + j) * p.n_classes + c], (unsigned)nt);
    }
  }
}

__device__ __forceinline__ void flush_counts(const unsigned* cnt, const IouParams& p) {
  __syncthreads();
  for (int i = threadIdx.x; i < (2 + p.n_thr) * p.n_classes; i += blockDim.x)
    if (cnt[i]) atomicAdd(&p.counts[i], (unsigned long long)cnt[i]);
}

// Work item w = pair * n_rays + ray, consecutive lanes take consecutive rays (one pitch ring = 360 consecutive azimuths:
// neighbouring lanes walk neighbouring paths and read neighbouring label bytes of a grid that stays in L2).  Occupancy is read as
// label bytes on purpose: walking 16-bit z columns packed into LDS measured 0.375 against 0.269 ms at 4 samples x 8 origins x
// 14 040 rays, because every workgroup first packs both grids of its sample (docs/LAB_NOTEBOOK.md, R8.1).
template <class O>
__global__ __launch_bounds__(kBlock) void ray_iou_bytes(const IouParams p) {
  __shared__ unsigned cnt[(2 + kMaxThr) * kMaxClasses];
  for (int i = threadIdx.x; i < (2 + kMaxThr) * kMaxClasses; i += kBlock) cnt[i] = 0;
  __syncthreads();
  const long total = (long)p.n_pairs * p.n_rays;
  const long cells = (long)p.nx * p.ny * p.nz;
  for (long w0 = (long)blockIdx.x * kBlock; w0 < total; w0 += (long)gridDim.x * kBlock) {   // block-uniform trip count
    const long w = w0 + threadIdx.x;
    bool valid = w < total;
    int gl = 0, pl = 0;
    float dp = 0.f, dg = 0.f;
    if (valid) {
      const int k = (int)(w / p.n_rays), r = (int)(w % p.n_rays);
      const int s = p.sample_id[k];
      valid = s >= 0 && s < p.n_samples;     // a pair that names no sample is skipped, never read through
      if (valid) {
        double o[3], e[3];
        to_voxel_units(static_cast<const O*>(p.origins) + (long)k * 3, p.rays + (long)r * 3, p, o, e);
        const uint8_t* gp = p.pred + s * cells;
        const uint8_t* gg = p.gt + s * cells;
        const Hit hp = walk(o[0], o[1], o[2], e[0], e[1], e[2], p.nx, p.ny, p.nz, ByteLabels{gp, p.ny, p.nz, p.free_id});
        const Hit hg = walk(o[0], o[1], o[2], e[0], e[1], e[2], p.nx, p.ny, p.nz, ByteLabels{gg, p.ny, p.nz, p.free_id});
        label_and_dist(hp, gp, p, pl, dp);
        label_and_dist(hg, gg, p, gl, dg);
      }
    }
    count_wave(valid, gl, pl, dp, dg, p, cnt);
  }
  flush_counts(cnt, p);
}

}  // namespace

extern "C" {

int dhd_ray_iou_supported(int nx, int ny, int nz, int n_classes, int n_thresholds) {
  if (nx < 1 || ny < 1 || nz < 1 || n_classes < 1 || n_thresholds < 1) return 0;
  if ((long)nx * ny * nz > 0x7fffffffL) return 0;
  return n_classes <= kMaxClasses && n_thresholds <= kMaxThr;
}

int dhd_ray_render_forward(const float* sigma, const float* origin, const float* points, const float* tindex, int n, int t_sigma,
                           int t_origin, int m, int nz, int ny, int nx, int phase, float* pred_dist, float* gt_dist,
                           float* coord_index, void* stream) {
  if (!sigma || !origin || !points || !tindex || !pred_dist || !gt_dist || !coord_index) return DHD_EINVAL;
  if (n < 1 || t_sigma < 1 || t_origin < 1 || m < 1 || nz < 1 || ny < 1 || nx < 1) return DHD_EINVAL;
  if (phase != DHD_RAY_PHASE_TEST && phase != DHD_RAY_PHASE_TRAIN) return DHD_EINVAL;
  if (phase == DHD_RAY_PHASE_TRAIN) return DHD_EUNSUPPORTED;
  if ((long)nx * ny * nz > 0x7fffffffL || n > 65535 || (long)n * m > 0x7fffffffL / 3) return DHD_EUNSUPPORTED;
  hipLaunchKernelGGL(ray_render_forward, dim3(dhd_cdiv(m, kBlock), n), dim3(kBlock), 0, dhd_stream(stream), sigma, origin, points,
                     tindex, t_sigma, t_origin, m, nz, ny, nx, pred_dist, gt_dist, coord_index);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

int dhd_ray_iou_accumulate(const uint8_t* pred, const uint8_t* gt, int n_samples, int nx, int ny, int nz, const int32_t* sample_id,
                           const void* origins, int n_pairs, int flags, const float* rays, int n_rays, const float* lower,
                           float voxel_size, int free_id, int n_classes, const float* thresholds, int n_thresholds,
                           int64_t* counts, void* stream) {
  if (!pred || !gt || !sample_id || !origins || !rays || !lower || !thresholds || !counts) return DHD_EINVAL;
  if (n_samples < 1 || nx < 1 || ny < 1 || nz < 1 || n_pairs < 1 || n_rays < 1 || n_classes < 1 || n_thresholds < 1)
    return DHD_EINVAL;
  if ((flags & ~DHD_RAY_ORIGIN_F64) != 0 || free_id < 0 || !(voxel_size > 0.f)) return DHD_EINVAL;
  const bool f64 = (flags & DHD_RAY_ORIGIN_F64) != 0;
  if ((reinterpret_cast<uintptr_t>(origins) & (f64 ? 7 : 3)) || (reinterpret_cast<uintptr_t>(counts) & 7) ||
      (reinterpret_cast<uintptr_t>(rays) & 3) || (reinterpret_cast<uintptr_t>(sample_id) & 3))
    return DHD_EINVAL;
  if (!dhd_ray_iou_supported(nx, ny, nz, n_classes, n_thresholds)) return DHD_EUNSUPPORTED;
  if ((long)nx * ny * nz * n_samples > (1L << 40) || (long)n_pairs * n_rays > (1L << 40)) return DHD_EUNSUPPORTED;

  IouParams p = {};
  p.pred = pred; p.gt = gt; p.sample_id = sample_id; p.origins = origins; p.rays = rays;
  p.counts = reinterpret_cast<unsigned long long*>(counts);
  p.n_samples = n_samples; p.nx = nx; p.ny = ny; p.nz = nz; p.n_pairs = n_pairs; p.n_rays = n_rays;
  p.free_id = free_id; p.n_classes = n_classes; p.n_thr = n_thresholds; p.voxel = voxel_size;
  for (int a = 0; a < 3; ++a) p.lower[a] = lower[a];
  for (int j = 0; j < n_thresholds; ++j) p.thr[j] = thresholds[j];
  hipStream_t st = dhd_stream(stream);

  const long want = ((long)n_pairs * n_rays + kBlock - 1) / kBlock;
  const int blocks = (int)(want < kMaxBlocks ? want : kMaxBlocks);
  if (f64) hipLaunchKernelGGL(ray_iou_bytes<double>, dim3(blocks), dim3(kBlock), 0, st, p);
  else     hipLaunchKernelGGL(ray_iou_bytes<float>, dim3(blocks), dim3(kBlock), 0, st, p);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

}  // extern "C"
