// Deformable convolution in training: the backward of deform_conv.hip's operator without column gradients (the dhdd_* surface,
// dhd_amd/capi_deform/dhd_amd_deform_train.h).  Included by deform_conv.hip after its kernels: Shape, the LDS tap table,
// load_corners / corner_values / blend, operand_of / mfma_parts and store_tiles are the forward's own.
//
// With col[c, t, p] = bilinear(x[c], pos(t, p)) and out = W col, the training path of depthnet.py keeps col from forward to
// backward, lets torch write dcol = W^T gout at the same size and reads it twice (col2im gather, col2offset).  Here neither exists:
//
//   deform_tap_sort_ct   one block per image: the <= 36 hw corner entries (source pixel, weight) grouped by (cell, tap), key =
//                        cell * 9 + t, then every segment put in ascending source order, so that the order of every sum below
//                        is a function of the offsets alone
//   deform_conv_bwd_dx_kernel    dx[cell, c] = sum_{t, o} W[o, c, t] G_t[cell, o],  G_t[cell, o] = sum over the entries e of segment
//                        (cell, t) of w_e gout[o, p_e]: the forward's GEMM again (rows c, reduction k = t O/g + o), whose B operand a lane
//                        gathers through the segment of its own cell from a channels_last gout in 16-byte runs, float32 sums
//   deform_conv_bwd_cols_kernel  dcol[(t, c), p] = sum_o W[o, c, t] gout[o, p] per 32-row tile in accumulator registers (A = W^T,
//                        rows k = t C/g + c; B = the lane's own pixel of gout, fetched once); from the corner runs of x of the
//                        tile's channels the two offset sums of the lane's pixel (dcol entering them rounded once to the GEMM type,
//                        as the column path's GEMM writes it) and, on request, the recomputed col values
//                        (the operand of dW, the bytes dhd_deform_im2col_t writes).  One block per (image, 128 pixels, group):
//                        with more than one group every group writes its own plane of partial offset gradients, and
//                        deform_doff_sum_kernel adds the planes in group order.  No atomics anywhere.
// float32 x: operands cut into bf16 high + residual, three products; fp16 / bf16 x: one product.  float32 accumulation.
#pragma once

namespace {

constexpr int kCtSortBlock = 1024;
// LDS of the sort: cnt[9 hw] | cur[9 hw] | part[kCtSortBlock] as int32 within 64 KiB
constexpr int kTrainMaxHW = (64 * 1024 / 4 - kCtSortBlock) / (2 * kTaps);     // 853 (the DHD-S map, 16 x 44, has 704)
constexpr int kCtRankRegs = 8;            // entries of a segment the ranking pass holds in registers

__global__ __launch_bounds__(kCtSortBlock) void deform_tap_sort_ct(const float* __restrict__ off, int* __restrict__ seg_start,
                                                                   uint2* __restrict__ unordered, uint2* __restrict__ entries, int h, int w,
                                                                   int pad, int dil) {
  extern __shared__ int sm[];
  const int hw = h * w, n = kTaps * hw, b = blockIdx.x, tid = threadIdx.x;
  int* cnt = sm;
  int* cur = sm + n;
  int* part = sm + 2 * n;
  for (int i = tid; i < n; i += kCtSortBlock) cnt[i] = 0;
  __syncthreads();
  const float* off_b = off + (size_t)b * 2 * kTaps * hw;
  for (int i = tid; i < n; i += kCtSortBlock) {
    const int t = i / hw;
    const dhd_deform::Tap tp = dhd_deform::tap_of(off_b, t, i % hw, h, w, 3, pad, dil);
    if (tp.v00) atomicAdd(cnt + tp.i00 * kTaps + t, 1);
    if (tp.v01) atomicAdd(cnt + tp.i01 * kTaps + t, 1);
    if (tp.v10) atomicAdd(cnt + tp.i10 * kTaps + t, 1);
    if (tp.v11) atomicAdd(cnt + tp.i11 * kTaps + t, 1);
  }
  __syncthreads();
  // exclusive scan of cnt: a contiguous chunk of segments per thread, then an inclusive scan of the chunk sums in LDS
  const int chunk = (n + kCtSortBlock - 1) / kCtSortBlock, lo = min(n, tid * chunk), hi = min(n, lo + chunk);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += cnt[i];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < kCtSortBlock; d <<= 1) {
    const int below = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += below;
    __syncthreads();
  }
  int* start_b = seg_start + (size_t)b * (n + 1);
  int run = part[tid] - sum;
  for (int i = lo; i < hi; ++i) {
    cur[i] = run;
    start_b[i] = run;
    run += cnt[i];
  }
  if (tid == kCtSortBlock - 1) start_b[n] = part[tid];
  __syncthreads();
  uint2* tmp_b = unordered + (size_t)b * 4 * n;
  for (int i = tid; i < n; i += kCtSortBlock) {
    const int t = i / hw, p = i % hw;
    const dhd_deform::Tap tp = dhd_deform::tap_of(off_b, t, p, h, w, 3, pad, dil);
    if (tp.v00) tmp_b[atomicAdd(cur + tp.i00 * kTaps + t, 1)] = make_uint2((unsigned)p, __float_as_uint(tp.w00));
    if (tp.v01) tmp_b[atomicAdd(cur + tp.i01 * kTaps + t, 1)] = make_uint2((unsigned)p, __float_as_uint(tp.w01));
    if (tp.v10) tmp_b[atomicAdd(cur + tp.i10 * kTaps + t, 1)] = make_uint2((unsigned)p, __float_as_uint(tp.w10));
    if (tp.v11) tmp_b[atomicAdd(cur + tp.i11 * kTaps + t, 1)] = make_uint2((unsigned)p, __float_as_uint(tp.w11));
  }
  __syncthreads();      // the block's own stores to `unordered` are read below
  // ascending source order within a segment: an entry's place is the number of entries of its segment with a smaller source
  // (a pixel reaches a cell through at most one of its four corners per tap, so the sources of a segment differ)
  uint2* ent_b = entries + (size_t)b * 4 * n;
  for (int seg = tid; seg < n; seg += kCtSortBlock) {
    const int e = cur[seg], s = e - cnt[seg], len = e - s;
    if (len <= kCtRankRegs) {             // the common case (4 on average): the segment in registers, its loads in flight together
      uint2 en[kCtRankRegs];
#pragma unroll
      for (int i = 0; i < kCtRankRegs; ++i) en[i] = i < len ? tmp_b[s + i] : make_uint2(0xffffffffu, 0u);   // never the smaller one
#pragma unroll
      for (int i = 0; i < kCtRankRegs; ++i) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < kCtRankRegs; ++j) rank += en[j].x < en[i].x ? 1 : 0;
        if (i < len) ent_b[s + rank] = en[i];
      }
    } else {
      for (int i = s; i < e; ++i) {
        const uint2 en = tmp_b[i];
        int rank = 0;
        for (int j = s; j < e; ++j) rank += tmp_b[j].x < en.x ? 1 : 0;
        ent_b[s + rank] = en;
      }
    }
  }
}

// the two weight streams of the backward, 1 KiB fragments in the order the waves read them (pack_weights_kernel's fragment form:
// lane (r, hh) holds A[row 32 m + r][k = 16 ks + 8 hh + j]); rows and k past the matrix are zero
//   MODE 0 (dx)    A[c][k = t O/g + o] = W[o, c, t],     fragments (g, ks, m, part)
//   MODE 1 (cols)  A[t C/g + c][k = o] = W[o, c, t],     fragments (g, m, ks, part)
template <class T, int MODE>
__global__ __launch_bounds__(kPackBlock) void pack_train_weights_kernel(const float* __restrict__ wgt, u32x4* __restrict__ stream, Shape s,
                                                                        int nks, int mt) {
  constexpr int P = kParts<T>;
  const long idx = (long)blockIdx.x * kPackBlock + threadIdx.x;
  const long n = (long)s.groups * nks * mt * P * 64;
  if (idx >= n) return;
  const int lane = (int)(idx & 63), r = lane & 31, hh = lane >> 5;
  long f = idx >> 6;
  const int part = (int)(f % P); f /= P;
  int m, ks, g;
  if constexpr (MODE == 0) {
    m = (int)(f % mt); f /= mt;
    ks = (int)(f % nks); g = (int)(f / nks);
  } else {
    ks = (int)(f % nks); f /= nks;
    m = (int)(f % mt); g = (int)(f / mt);
  }
  const int row = 32 * m + r, k0 = 16 * ks + 8 * hh;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = k0 + j;
    int t, c, o;
    if constexpr (MODE == 0) { t = k / s.og; o = k - t * s.og; c = row; }
    else { t = row / s.cg; c = row - t * s.cg; o = k; }
    v[j] = (t < kTaps && c < s.cg && o < s.og) ? wgt[((size_t)(g * s.og + o) * s.cg + c) * kTaps + t] : 0.f;
  }
  u32x4 parts[P];
  operand_of<T>(v, parts);
  stream[idx] = parts[part];
}

// MT: accumulator tiles of 32 input channels a wave keeps (1, 2 or 4 >= mt)
template <class T, bool OUT_NHWC, int MT>
__global__ __launch_bounds__(kBlock) void deform_conv_bwd_dx_kernel(const T* __restrict__ gout, const int* __restrict__ seg_start,
                                                                    const uint2* __restrict__ entries, const u32x4* __restrict__ stream,
                                                                    T* __restrict__ dx, Shape s, int tiles, int nks, int mt) {
  constexpr int P = kParts<T>;
  __shared__ int seg[kTaps * kPix + 1];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5, wave = tid >> 6;
  const int hw = s.h * s.w, n = kTaps * hw;
  const int g = blockIdx.x % s.groups;
  const int tile = (blockIdx.x / s.groups) % tiles, b = blockIdx.x / s.groups / tiles;
  const int p0 = tile * kPix;
  // the segment bounds of the block's cells are consecutive; a cell past the image gets an empty segment
  const int* start_b = seg_start + (size_t)b * (n + 1);
  for (int i = tid; i <= kTaps * kPix; i += kBlock) seg[i] = start_b[min(kTaps * p0 + i, n)];
  __syncthreads();
  if (p0 + wave * 32 >= hw) return;       // wave-uniform, after the only barrier
  const int px = wave * 32 + r;
  const bool live = p0 + px < hw;
  const T* gg = gout + (size_t)b * hw * s.o + (size_t)g * s.og;   // channels_last: pixel i, channel o at gg[i * O + o]
  const uint2* ent_b = entries + (size_t)b * 4 * n;
  const u32x4* wl = stream + (size_t)g * nks * mt * P * 64 + lane;

  f32x16 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[m][e] = 0.f;

  int t = 0, o0 = 8 * hh;       // (tap, first output channel) of this lane's 8 values of the k-step, advanced by 16 per step
  for (int ks = 0; ks < nks; ++ks) {
    while (o0 >= s.og && t < kTaps) { o0 -= s.og; ++t; }
    u32x4 wf[MT][P];
#pragma unroll
    for (int m = 0; m < MT; ++m)
      if (m < mt) {
#pragma unroll
        for (int q = 0; q < P; ++q) wf[m][q] = wl[(size_t)((ks * mt + m) * P + q) * 64];
      }
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (t < kTaps) {
      const int sb = seg[px * kTaps + t], se = seg[px * kTaps + t + 1];
      for (int i = sb; i < se; ++i) {     // ascending source pixel: the order of the sum
        const uint2 en = ent_b[i];
        const float wgt = __uint_as_float(en.y);
        const u32x4* src = reinterpret_cast<const u32x4*>(gg + (size_t)en.x * s.o + o0);
        u32x4 q[kRun<T>];
#pragma unroll
        for (int e = 0; e < kRun<T>; ++e) q[e] = src[e];
        float gv[8];
        widen_run<T>(q, gv);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = fmaf(wgt, gv[j], v[j]);
      }
    }
    o0 += 16;
    u32x4 xf[P];
    operand_of<T>(v, xf);
#pragma unroll
    for (int m = 0; m < MT; ++m)
      if (m < mt) acc[m] = mfma_parts<T>(wf[m], xf, acc[m]);
  }
  store_tiles<T, OUT_NHWC, MT>(acc, dx, b, hw, p0, px, live, hh, g, s.cg, s.c);
}

// NK: k-steps of 16 over O/g whose B fragments a lane keeps (1, 2, 4 or 8 >= nks)
template <class T, int NK>
__global__ __launch_bounds__(kBlock) void deform_conv_bwd_cols_kernel(const T* __restrict__ x, const T* __restrict__ gout,
                                                                      const float* __restrict__ off, const u32x4* __restrict__ stream,
                                                                      float* __restrict__ doff, size_t doff_group_stride,
                                                                      T* __restrict__ col, Shape s, int tiles, int nks, int mt) {
  constexpr int P = kParts<T>;
  __shared__ int4 tap_idx[kTaps * kPix];
  __shared__ float4 tap_wt[kTaps * kPix];
  __shared__ float2 tap_frac[kTaps * kPix];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5, wave = tid >> 6;
  const int hw = s.h * s.w;
  const int g = blockIdx.x % s.groups;
  const int tile = (blockIdx.x / s.groups) % tiles, b = blockIdx.x / s.groups / tiles;
  const int p0 = tile * kPix;
  const float* off_b = off + (size_t)b * 2 * kTaps * hw;
  // tap table of the block's pixels, as in the forward, with the fractional parts; a pixel past the image repeats the last one
  for (int i = tid; i < kTaps * kPix; i += kBlock) {
    const int t = i / kPix, p = min(p0 + i % kPix, hw - 1);
    const dhd_deform::Tap tp = dhd_deform::tap_of(off_b, t, p, s.h, s.w, 3, s.pad, s.dil);
    tap_idx[i] = make_int4(tp.v00 ? tp.i00 : -1, tp.v01 ? tp.i01 : -1, tp.v10 ? tp.i10 : -1, tp.v11 ? tp.i11 : -1);
    tap_wt[i] = make_float4(tp.w00, tp.w01, tp.w10, tp.w11);
    tap_frac[i] = make_float2(tp.ly, tp.lx);
  }
  __syncthreads();
  if (p0 + wave * 32 >= hw) return;       // wave-uniform, after the only barrier
  const int px = wave * 32 + r, p = p0 + px;
  const bool live = p < hw;
  const T* xg = x + (size_t)b * hw * s.c + (size_t)g * s.cg;
  const T* gp = gout + ((size_t)b * hw + min(p, hw - 1)) * s.o + (size_t)g * s.og;
  const u32x4* wl = stream + (size_t)g * mt * nks * P * 64 + lane;

  // B: the lane's own pixel of gout, every k-step, fetched once
  u32x4 bf[NK][P];
#pragma unroll
  for (int ks = 0; ks < NK; ++ks) {
    const int o0 = 16 * ks + 8 * hh;
    float gv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) gv[j] = 0.f;
    if (o0 < s.og) {
      const u32x4* src = reinterpret_cast<const u32x4*>(gp + o0);
      u32x4 q[kRun<T>];
#pragma unroll
      for (int e = 0; e < kRun<T>; ++e) q[e] = src[e];
      widen_run<T>(q, gv);
    }
    operand_of<T>(gv, bf[ks]);
  }

  float* d = doff + (size_t)g * doff_group_stride + (size_t)b * 2 * kTaps * hw;
  int tcur = -1;
  float gy = 0.f, gx = 0.f;
  // the sums of one tap are complete when the rows move on to the next: the two halves of the wave hold 4 channels of every 8
  auto flush = [&]() {
    if (tcur < 0) return;
    const float ty = gy + __shfl_xor(gy, 32, DHD_WAVE), tx = gx + __shfl_xor(gx, 32, DHD_WAVE);
    if (hh == 0 && live) {
      d[(size_t)(2 * tcur) * hw + p] = ty;
      d[(size_t)(2 * tcur + 1) * hw + p] = tx;
    }
  };
  for (int m = 0; m < mt; ++m) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks)
      if (ks < nks) {
        u32x4 wf[P];
#pragma unroll
        for (int q = 0; q < P; ++q) wf[q] = wl[(size_t)((m * nks + ks) * P + q) * 64];
        acc = mfma_parts<T>(wf, bf[ks], acc);
      }
    // register e: row 32 m + 8 (e >> 2) + 4 hh + (e & 3) = t C/g + c of dcol, pixel p; 8 rows share a tap (C/g is a multiple of 8)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row0 = 32 * m + 8 * q, t = row0 / s.cg, c8 = row0 - t * s.cg;
      if (t < kTaps) {                    // wave-uniform
        if (t != tcur) {
          flush();
          tcur = t;
          gy = gx = 0.f;
        }
        Corners<T> cr;
        load_corners<T>(xg, tap_idx, tap_wt, t, c8, px, s.c, true, cr);
        if (cr.valid & 15) {              // deform_col2offset's `inside`: a tap inside the image has a corner inside
          float xv[4][8];
#pragma unroll
          for (int i = 0; i < 4; ++i) corner_values<T>(cr, i, xv[i]);
          const float2 fr = tap_frac[t * kPix + px];
          const float ly = fr.x, lx = fr.y, hy = 1.0f - ly, hx = 1.0f - lx;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float v00 = hh ? xv[0][4 + i] : xv[0][i], v01 = hh ? xv[1][4 + i] : xv[1][i];
            const float v10 = hh ? xv[2][4 + i] : xv[2][i], v11 = hh ? xv[3][4 + i] : xv[3][i];
            // dcol as the column path's GEMM hands it to deform_col2offset: in the GEMM type, rounded once (float32: as it is)
            const float gv = (float)(T)acc[4 * q + i];
            gy = fmaf(gv, (v10 - v00) * hx + (v11 - v01) * lx, gy);
            gx = fmaf(gv, (v01 - v00) * hy + (v11 - v10) * ly, gx);
          }
        }
        if (col) {
          float v[8];
          blend<T>(cr, v);
          T* cb = col + (((size_t)b * s.c + (size_t)g * s.cg + c8 + 4 * hh) * kTaps + t) * hw + p;
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (live) cb[(size_t)i * kTaps * hw] = (T)(hh ? v[4 + i] : v[i]);
        }
      }
    }
  }
  flush();
}

// doffset = the groups' partial planes added in group order
__global__ __launch_bounds__(kPackBlock) void deform_doff_sum_kernel(const float* __restrict__ part, float* __restrict__ doff, long n, int groups) {
  const long i = (long)blockIdx.x * kPackBlock + threadIdx.x;
  if (i >= n) return;
  float v = part[i];
  for (int g = 1; g < groups; ++g) v += part[(size_t)g * n + i];
  doff[i] = v;
}

struct TrainPlan {
  Shape s;
  int nks_dx, mt_dx;       // dx: k-steps over 9 O/g, tiles of 32 input channels
  int nks_cols, mt_cols;   // cols: k-steps over O/g, tiles of 32 rows of (t, c)
  size_t at_stream_cols, at_starts, at_entries, at_unordered, at_doff, at_x, at_gout, total;
};

size_t up256(size_t n) { return (n + 255) / 256 * 256; }

TrainPlan make_train_plan(int b, int c, int o, int groups, int h, int w, int pad, int dil, int x_dtype, int x_layout, int g_layout) {
  TrainPlan pl;
  pl.s = make_shape(c, o, groups, h, w, pad, dil);
  const Shape& s = pl.s;
  pl.nks_dx = (kTaps * s.og + 15) / 16;
  pl.mt_dx = (s.cg + 31) / 32;
  pl.nks_cols = (s.og + 15) / 16;
  pl.mt_cols = (kTaps * s.cg + 31) / 32;
  const size_t parts = x_dtype == DHD_F32 ? 2 : 1, esz = x_dtype == DHD_F32 ? 4 : 2;
  const size_t hw = (size_t)h * w, n = kTaps * hw;
  size_t at = up256((size_t)groups * pl.nks_dx * pl.mt_dx * parts * 1024);
  pl.at_stream_cols = at; at += up256((size_t)groups * pl.mt_cols * pl.nks_cols * parts * 1024);
  pl.at_starts = at;      at += up256((size_t)b * (n + 1) * sizeof(int));
  pl.at_entries = at;     at += up256((size_t)b * 4 * n * sizeof(uint2));
  pl.at_unordered = at;   at += up256((size_t)b * 4 * n * sizeof(uint2));
  pl.at_doff = at;        at += groups > 1 ? up256((size_t)groups * b * 2 * kTaps * hw * sizeof(float)) : 0;
  pl.at_x = at;           at += x_layout == 0 ? up256((size_t)b * c * hw * esz) : 0;
  pl.at_gout = at;        at += g_layout == 0 ? up256((size_t)b * o * hw * esz) : 0;
  pl.total = at;
  return pl;
}

bool train_supported(int c, int o, int groups, int k, int h, int w, int x_dtype, int x_layout, int g_layout) {
  return shape_supported(c, o, groups, k, h, w) && (long)h * w <= kTrainMaxHW && precision_supported(x_dtype, x_layout, DHD_SFA_GEMM_DEFAULT) &&
         (g_layout == 0 || g_layout == 1);
}

template <class T>
int launch_backward(const void* x, int x_layout, const float* offset, const float* weight, const void* gout, int g_layout, void* dx,
                    float* doffset, void* col, int b, const TrainPlan& pl, void* scratch, void* stream) {
  hipStream_t st = dhd_stream(stream);
  const Shape& s = pl.s;
  char* base = static_cast<char*>(scratch);
  u32x4* stream_dx = reinterpret_cast<u32x4*>(base);
  u32x4* stream_cols = reinterpret_cast<u32x4*>(base + pl.at_stream_cols);
  int* starts = reinterpret_cast<int*>(base + pl.at_starts);
  uint2* entries = reinterpret_cast<uint2*>(base + pl.at_entries);
  uint2* unordered = reinterpret_cast<uint2*>(base + pl.at_unordered);
  const int hw = s.h * s.w;
  const long n_dx = (long)s.groups * pl.nks_dx * pl.mt_dx * kParts<T> * 64, n_cols = (long)s.groups * pl.mt_cols * pl.nks_cols * kParts<T> * 64;
  hipLaunchKernelGGL((pack_train_weights_kernel<T, 0>), dim3(dhd_cdiv(n_dx, kPackBlock)), dim3(kPackBlock), 0, st, weight, stream_dx, s,
                     pl.nks_dx, pl.mt_dx);
  hipLaunchKernelGGL((pack_train_weights_kernel<T, 1>), dim3(dhd_cdiv(n_cols, kPackBlock)), dim3(kPackBlock), 0, st, weight, stream_cols, s,
                     pl.nks_cols, pl.mt_cols);
  hipLaunchKernelGGL(deform_tap_sort_ct, dim3(b), dim3(kCtSortBlock), (2 * (size_t)kTaps * hw + kCtSortBlock) * sizeof(int), st, offset, starts,
                     unordered, entries, s.h, s.w, s.pad, s.dil);
  DHD_LAUNCH_CHECK();
  const T* xc = static_cast<const T*>(x);
  const T* gc = static_cast<const T*>(gout);
  if (x_layout == 0) {
    T* copy = reinterpret_cast<T*>(base + pl.at_x);
    const int rc = dhd_transpose_batched(x, copy, (int)sizeof(T), b, s.c, hw, stream);
    if (rc != DHD_OK) return rc;
    xc = copy;
  }
  if (g_layout == 0) {
    T* copy = reinterpret_cast<T*>(base + pl.at_gout);
    const int rc = dhd_transpose_batched(gout, copy, (int)sizeof(T), b, s.o, hw, stream);
    if (rc != DHD_OK) return rc;
    gc = copy;
  }
  const int tiles = dhd_cdiv(hw, kPix);
  const dim3 grid((unsigned)((long)b * tiles * s.groups));
  T* dxo = static_cast<T*>(dx);
  auto go_dx = [&](auto mt_tag) {
    constexpr int MT = decltype(mt_tag)::value;
    if (x_layout) hipLaunchKernelGGL((deform_conv_bwd_dx_kernel<T, true, MT>), grid, dim3(kBlock), 0, st, gc, starts, entries, stream_dx, dxo, s,
                                     tiles, pl.nks_dx, pl.mt_dx);
    else hipLaunchKernelGGL((deform_conv_bwd_dx_kernel<T, false, MT>), grid, dim3(kBlock), 0, st, gc, starts, entries, stream_dx, dxo, s, tiles,
                            pl.nks_dx, pl.mt_dx);
  };
  if (pl.mt_dx == 1) go_dx(std::integral_constant<int, 1>{});
  else if (pl.mt_dx == 2) go_dx(std::integral_constant<int, 2>{});
  else go_dx(std::integral_constant<int, kMaxMT>{});
  DHD_LAUNCH_CHECK();
  const long n_doff = (long)b * 2 * kTaps * hw;
  float* dpart = s.groups > 1 ? reinterpret_cast<float*>(base + pl.at_doff) : doffset;
  auto go_cols = [&](auto nk_tag) {
    constexpr int NK = decltype(nk_tag)::value;
    hipLaunchKernelGGL((deform_conv_bwd_cols_kernel<T, NK>), grid, dim3(kBlock), 0, st, xc, gc, offset, stream_cols, dpart, (size_t)n_doff,
                       static_cast<T*>(col), s, tiles, pl.nks_cols, pl.mt_cols);
  };
  if (pl.nks_cols == 1) go_cols(std::integral_constant<int, 1>{});
  else if (pl.nks_cols == 2) go_cols(std::integral_constant<int, 2>{});
  else if (pl.nks_cols <= 4) go_cols(std::integral_constant<int, 4>{});
  else go_cols(std::integral_constant<int, 8>{});
  DHD_LAUNCH_CHECK();
  if (s.groups > 1) {
    hipLaunchKernelGGL(deform_doff_sum_kernel, dim3(dhd_cdiv(n_doff, kPackBlock)), dim3(kPackBlock), 0, st, dpart, doffset, n_doff, s.groups);
    DHD_LAUNCH_CHECK();
  }
  return DHD_OK;
}

}  // namespace

extern "C" {

int dhdd_deform_conv_backward_supported(int c_in, int c_out, int groups, int k, int h, int w, int x_dtype, int x_layout, int g_layout) {
  return train_supported(c_in, c_out, groups, k, h, w, x_dtype, x_layout, g_layout) ? 1 : 0;
}

int dhdd_deform_conv_backward_scratch_bytes(int b, int c_in, int c_out, int groups, int k, int h, int w, int x_dtype, int x_layout,
                                            int g_layout, size_t* bytes) {
  if (bytes) *bytes = 0;
  if (!bytes || b <= 0 || c_in <= 0 || c_out <= 0 || groups <= 0 || h <= 0 || w <= 0 || !dtype_ok(x_dtype) || (x_layout != 0 && x_layout != 1) ||
      (g_layout != 0 && g_layout != 1))
    return DHD_EINVAL;
  if (c_in % groups || c_out % groups) return DHD_EINVAL;
  if (!train_supported(c_in, c_out, groups, k, h, w, x_dtype, x_layout, g_layout) || b > 65535) return DHD_EUNSUPPORTED;
  *bytes = make_train_plan(b, c_in, c_out, groups, h, w, 0, 1, x_dtype, x_layout, g_layout).total;
  return DHD_OK;
}

int dhdd_deform_conv_backward(const void* x, int x_dtype, int x_layout, const float* offset, const float* weight, const void* gout,
                              int g_layout, void* dx, float* doffset, void* col, int b, int c_in, int c_out, int groups, int h, int w, int k,
                              int pad, int dil, void* scratch, size_t scratch_bytes, void* stream) {
  if (!x || !offset || !weight || !gout || !dx || !doffset || !scratch) return DHD_EINVAL;
  if (b <= 0 || c_in <= 0 || c_out <= 0 || groups <= 0 || h <= 0 || w <= 0 || k <= 0 || pad < 0 || dil < 1) return DHD_EINVAL;
  if (!dtype_ok(x_dtype) || (x_layout != 0 && x_layout != 1) || (g_layout != 0 && g_layout != 1)) return DHD_EINVAL;
  if (c_in % groups || c_out % groups) return DHD_EINVAL;
  if (!train_supported(c_in, c_out, groups, k, h, w, x_dtype, x_layout, g_layout)) return DHD_EUNSUPPORTED;
  const long hw = (long)h * w, tiles = (hw + kPix - 1) / kPix;
  // 32-bit element indices on the device (hw <= 853, C/g and O/g <= 128); one block per (image, pixel tile, group)
  if (b > 65535 || b * hw * c_in >= (1L << 31) || b * hw * c_out >= (1L << 31) || (long)pad + 2L * dil + h + w >= (1L << 30) ||
      b * tiles * groups >= (1L << 31))
    return DHD_EUNSUPPORTED;
  const TrainPlan pl = make_train_plan(b, c_in, c_out, groups, h, w, pad, dil, x_dtype, x_layout, g_layout);
  if (scratch_bytes < pl.total) return DHD_ENOSPACE;
  // corner runs of x, runs of gout, the streams, a channels_last dx and the entry lists move as 8- and 16-byte vectors
  if (!dhd_aligned(16, x, gout, dx, col, scratch) || !dhd_aligned(4, offset, weight, doffset)) return DHD_EINVAL;
  return dhd::with_dtype<dhd::NativeHalf>(x_dtype, [&](auto* tp) {
    using T = std::remove_pointer_t<decltype(tp)>;
    return launch_backward<T>(x, x_layout, offset, weight, gout, g_layout, dx, doffset, col, b, pl, scratch, stream);
  });
}

}  // extern "C"
