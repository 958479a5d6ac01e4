// Deformable convolution at inference: bilinear gather + grouped MFMA GEMM in one kernel (section 15 of dhd_amd.h).
//
//   out[b, o, p] = sum_{c in group g, t < 9} W[o, c, t] * bilinear(x[b, c], tap position of (t, p))
//
// deform.hip writes the sampled columns (B, C*9, H*W) for a library GEMM because the backward pass needs them.  With nothing to
// differentiate they are pure traffic, and here they never exist in memory: the 8 consecutive-k values a lane contributes to
// the B operand of mfma_f32_32x32x16 are 8 consecutive channels of ONE tap of the lane's own pixel (k = t * C/g + c, C/g a
// multiple of 8), and in a channels_last x each of their four bilinear corners is one contiguous 16- or 32-byte run.  So a
// lane gathers, blends (the float32 arithmetic of deform_tap.h, the order of deform_im2col) and narrows its own operand in
// registers; LDS holds only the block's tap table (corner indices and weights of 9 taps x 128 pixels, computed once and shared
// by every k-step), not columns.
//
//   block = 4 waves = 128 consecutive pixels of one image x one group; wave = 32 pixels x all O/g output channels
//   A operand  the group's weights, re-ordered and split by pack_weights_kernel into `scratch` once per call in the order the
//              waves read them (1 KiB fragments, L2-resident after the first blocks); rows past O/g and k past 9 C/g are zero
//   B operand  built per k-step from the corner runs loaded one k-step ahead (as are the weight fragments)
//   C          up to 4 tiles of 32 output channels x 32 pixels, column (pixel) on the lane: an NCHW out is stored with
//              consecutive pixels on consecutive lanes, a channels_last out as 4 consecutive channels per lane
// float32 x: columns and weights cut into bf16 high + residual, three products (bf16x3); fp16 / bf16 x: the column rounded once
// to the type (what dhd_deform_im2col_t writes), weights rounded to it, one product.  Accumulation is float32.
// A dense NCHW x is transposed into `scratch` by the library's tiled transpose (layout.hip) first: per-plane 2- and 4-byte
// corner gathers measured 5-7x slower in deform.hip's kernels, and the transpose moves x once.
#include "deform_tap.h"
#include "sfa_mfma.h"

namespace {

using namespace dhd_sfa;

constexpr int kBlock = 256;
constexpr int kPix = kBlock / 64 * 32;     // pixels per block
constexpr int kTaps = 9;
constexpr int kMaxMT = 4;                  // O/g <= 128
constexpr int kPackBlock = 256;

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

template <class T> constexpr int kParts = std::is_same_v<T, float> ? 2 : 1;
template <class T> constexpr int kRun = 8 * (int)sizeof(T) / 16;   // 16-byte loads per corner run of 8 channels

template <class T> __device__ __forceinline__ f32x16 mfma16(u32x4 a, u32x4 b, f32x16 c) {
  if constexpr (std::is_same_v<T, _Float16>)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return mfma_bf16(a, b, c);
}

struct Shape {
  int c, o, groups, cg, og, h, w, pad, dil;
  int nks, mt;     // k-steps of 16 over K = 9 cg (zero-padded), tiles of 32 output channels
};

// fragment (g, ks, m, part) of the weight stream: lane (r, hh) holds A[row 32 m + r][k = 16 ks + 8 hh + j], k = t cg + c
template <class T>
__global__ __launch_bounds__(kPackBlock) void pack_weights_kernel(const float* __restrict__ wgt, u32x4* __restrict__ stream, Shape s) {
  constexpr int P = kParts<T>;
  const long idx = (long)blockIdx.x * kPackBlock + threadIdx.x;
  const long n = (long)s.groups * s.nks * s.mt * P * 64;
  if (idx >= n) return;
  const int lane = (int)(idx & 63), r = lane & 31, hh = lane >> 5;
  long f = idx >> 6;
  const int part = (int)(f % P); f /= P;
  const int m = (int)(f % s.mt); f /= s.mt;
  const int ks = (int)(f % s.nks), g = (int)(f / s.nks);
  const int row = 32 * m + r, k0 = 16 * ks + 8 * hh;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = k0 + j, t = k / s.cg, c = k - t * s.cg;
    v[j] = (row < s.og && t < kTaps) ? wgt[((size_t)(g * s.og + row) * s.cg + c) * kTaps + t] : 0.f;
  }
  u32x4 out;
#pragma unroll
  for (int jp = 0; jp < 4; ++jp) {
    if constexpr (std::is_same_v<T, float>) {
      unsigned hi, mid;
      split2_hm(v[2 * jp], v[2 * jp + 1], hi, mid);
      out[jp] = part ? mid : hi;
    } else {
      out[jp] = Pair<T>::narrow(f32x2{v[2 * jp], v[2 * jp + 1]});
    }
  }
  stream[idx] = out;
}

// the four corner runs of one k-step of one lane, as loaded, and what is needed to blend them
template <class T> struct Corners {
  u32x4 q[4][kRun<T>];
  f32x4 wt;
  int valid;       // bit i: corner i lies inside the image; bit 4: k is below 9 cg
};

template <class T>
__device__ __forceinline__ void load_corners(const T* __restrict__ xg, const int4* tap_idx, const float4* tap_wt, int t, int c0, int px,
                                             int c, bool k_live, Corners<T>& out) {
  const int4 idx = tap_idx[t * kPix + px];
  const float4 wt = tap_wt[t * kPix + px];
  out.wt = f32x4{wt.x, wt.y, wt.z, wt.w};
  const int id[4] = {idx.x, idx.y, idx.z, idx.w};
  out.valid = k_live ? 16 : 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool ok = id[i] >= 0 && k_live;
    out.valid |= ok ? 1 << i : 0;
    // a corner outside the image reads cell 0 of the image (inside the tensor) and is discarded below
    const u32x4* src = reinterpret_cast<const u32x4*>(xg + (size_t)(ok ? id[i] : 0) * c + c0);
#pragma unroll
    for (int e = 0; e < kRun<T>; ++e) out.q[i][e] = src[e];
  }
}

// 16 bytes of a run of consecutive elements, as loaded, as float32 (4 values, or 8 of a half type)
template <class T>
__device__ __forceinline__ void widen_quad(u32x4 q, float* xv) {
  if constexpr (std::is_same_v<T, float>) {
#pragma unroll
    for (int z = 0; z < 4; ++z) xv[z] = __uint_as_float(q[z]);
  } else {
#pragma unroll
    for (int z = 0; z < 4; ++z) {
      const f32x2 p = Pair<T>::widen(q[z]);
      xv[2 * z] = p.x;
      xv[2 * z + 1] = p.y;
    }
  }
}

// a run of 8 consecutive elements, as loaded, as float32
template <class T>
__device__ __forceinline__ void widen_run(const u32x4 (&q)[kRun<T>], float* xv) {
#pragma unroll
  for (int e = 0; e < kRun<T>; ++e) widen_quad<T>(q[e], xv + 4 * e);
}

// the 8 values of corner i of a lane's run as float32; a corner outside the image gives zeros
template <class T>
__device__ __forceinline__ void corner_values(const Corners<T>& cr, int i, float* xv) {
  const bool ok = (cr.valid >> i) & 1;
#pragma unroll
  for (int e = 0; e < kRun<T>; ++e) {
    u32x4 q = cr.q[i][e];
#pragma unroll
    for (int z = 0; z < 4; ++z) q[z] = ok ? q[z] : 0u;
    widen_quad<T>(q, xv + 4 * e);
  }
}

// 8 consecutive-k float32 values as the lane's MFMA operand: rounded once to a half type, or cut into bf16 high + residual
template <class T>
__device__ __forceinline__ void operand_of(const float* v, u32x4 (&xf)[kParts<T>]) {
#pragma unroll
  for (int jp = 0; jp < 4; ++jp) {
    if constexpr (kParts<T> == 2) {
      unsigned hi, mid;
      split2_hm(v[2 * jp], v[2 * jp + 1], hi, mid);
      xf[0][jp] = hi;
      xf[kParts<T> - 1][jp] = mid;
    } else {
      xf[0][jp] = Pair<T>::narrow(f32x2{v[2 * jp], v[2 * jp + 1]});
    }
  }
}

// acc += A B with both operands in kParts<T> parts: three products of a two-part split, smallest terms first, or one product
template <class T>
__device__ __forceinline__ f32x16 mfma_parts(const u32x4 (&a)[kParts<T>], const u32x4 (&b)[kParts<T>], f32x16 acc) {
  constexpr int P = kParts<T>;
  if constexpr (P == 2) {
    acc = mfma16<T>(a[P - 1], b[0], acc);
    acc = mfma16<T>(a[0], b[P - 1], acc);
  }
  return mfma16<T>(a[0], b[0], acc);
}

// the 8 sampled values of the lane, deform_im2col's chain: v = 0, then fmaf(weight, corner, v) over the valid corners in the
// order 00, 01, 10, 11.  A corner outside the image enters as fmaf(0, 0, v) = v.
template <class T>
__device__ __forceinline__ void blend(const Corners<T>& cr, float* v) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float xv[8];
    corner_values<T>(cr, i, xv);
    const float wi = cr.wt[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = fmaf(wi, xv[j], v[j]);
  }
  if (!(cr.valid & 16)) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
  }
}

// The accumulator tiles of a wave -- register e of tile m: channel 32 m + 8 (e >> 2) + 4 hh + (e & 3) of group g (n_g channels per
// group, n_all in all), pixel p0 + px of image b -- stored into a (B, n_all, hw) tensor: channels_last as 4 consecutive channels
// per lane, NCHW with consecutive pixels on consecutive lanes.
template <class T, bool OUT_NHWC, int MT>
__device__ __forceinline__ void store_tiles(const f32x16 (&acc)[MT], T* __restrict__ out, int b, int hw, int p0, int px, bool live, int hh,
                                            int g, int n_g, int n_all) {
  if constexpr (OUT_NHWC) {
    // the block's 128 pixels x n_all channels behind one descriptor (at most 256 KiB); offsets of stored lanes lie inside it
    T* ob = out + ((size_t)b * hw + p0) * n_all;
    const int rows = min(kPix, hw - p0);
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(ob, 0, (unsigned)((size_t)rows * n_all * sizeof(T)), 0x00020000);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int oc = 32 * m + 8 * q + 4 * hh;
        if (live && oc < n_g) {
          const int el = px * n_all + g * n_g + oc;
          if constexpr (std::is_same_v<T, float>) {
            const u32x4 w4 = {__float_as_uint(acc[m][4 * q]), __float_as_uint(acc[m][4 * q + 1]), __float_as_uint(acc[m][4 * q + 2]),
                              __float_as_uint(acc[m][4 * q + 3])};
            store_b128_guarded<0>(w4, ro, el * 4, 0);
          } else {
            u32x2 w2;
            w2[0] = Pair<T>::narrow(f32x2{acc[m][4 * q], acc[m][4 * q + 1]});
            w2[1] = Pair<T>::narrow(f32x2{acc[m][4 * q + 2], acc[m][4 * q + 3]});
            *reinterpret_cast<u32x2*>(ob + el) = w2;
          }
        }
      }
  } else {
    T* ob = out + ((size_t)b * n_all + (size_t)g * n_g) * hw + p0 + px;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int oc = 32 * m + 8 * (e >> 2) + 4 * hh + (e & 3);
        if (live && oc < n_g) ob[(size_t)oc * hw] = (T)acc[m][e];
      }
  }
}

// MT: accumulator tiles of 32 output channels a wave keeps (1, 2 or 4 >= s.mt)
template <class T, bool OUT_NHWC, int MT>
__global__ __launch_bounds__(kBlock) void deform_conv_kernel(const T* __restrict__ x, const float* __restrict__ off,
                                                             const u32x4* __restrict__ stream, T* __restrict__ out, Shape s, int tiles) {
  constexpr int P = kParts<T>;
  __shared__ int4 tap_idx[kTaps * kPix];
  __shared__ float4 tap_wt[kTaps * kPix];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5, wave = tid >> 6;
  const int hw = s.h * s.w;
  const int g = blockIdx.x % s.groups;
  const int tile = (blockIdx.x / s.groups) % tiles, b = blockIdx.x / s.groups / tiles;
  const int p0 = tile * kPix;
  const float* off_b = off + (size_t)b * 2 * kTaps * hw;
  // tap table of the block's pixels; a pixel past the image repeats the last one and is never stored
  for (int i = tid; i < kTaps * kPix; i += kBlock) {
    const int t = i / kPix, p = min(p0 + i % kPix, hw - 1);
    const dhd_deform::Tap tp = dhd_deform::tap_of(off_b, t, p, s.h, s.w, 3, s.pad, s.dil);
    tap_idx[i] = make_int4(tp.v00 ? tp.i00 : -1, tp.v01 ? tp.i01 : -1, tp.v10 ? tp.i10 : -1, tp.v11 ? tp.i11 : -1);
    tap_wt[i] = make_float4(tp.w00, tp.w01, tp.w10, tp.w11);
  }
  __syncthreads();
  if (p0 + wave * 32 >= hw) return;       // wave-uniform, after the only barrier
  const int px = wave * 32 + r, p = p0 + px;
  const bool live = p < hw;
  const T* xg = x + (size_t)b * hw * s.c + (size_t)g * s.cg;      // channels_last: cell i, channel ch at xg[i * c + ch]
  const u32x4* wl = stream + (size_t)g * s.nks * s.mt * P * 64 + lane;

  f32x16 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[m][e] = 0.f;

  // One k-step's operands: the lane's corner runs and the weight fragments.  Two sets, A and B, alternate: while one is
  // blended and multiplied the other is in flight, both its gathers and its weights (with the weight fragments
  // loaded in the iteration that uses them, and four accumulator tiles for every O/g, a call took 77 us against 62 us at
  // (24, 256, 16, 44) in fp16 channels_last: an L2 round trip per k-step, and two waves per SIMD instead of three).
  struct Operands {
    Corners<T> cr;
    u32x4 wf[MT][P];
  };
  // (tap, first channel) of this lane's 8 values of the next k-step to load, advanced by 16 per step
  int t = 0, c0 = 8 * hh;
  auto fetch = [&](int ks, Operands& op) {
    while (c0 >= s.cg && t < kTaps) { c0 -= s.cg; ++t; }
    const bool k_live = t < kTaps;
    load_corners<T>(xg, tap_idx, tap_wt, k_live ? t : kTaps - 1, k_live ? c0 : 0, px, s.c, k_live, op.cr);
    c0 += 16;
#pragma unroll
    for (int m = 0; m < MT; ++m)
      if (m < s.mt) {
#pragma unroll
        for (int q = 0; q < P; ++q) op.wf[m][q] = wl[(size_t)((ks * s.mt + m) * P + q) * 64];
      }
  };
  auto multiply = [&](const Operands& op) {
    float v[8];
    blend<T>(op.cr, v);
    u32x4 xf[P];
    operand_of<T>(v, xf);
#pragma unroll
    for (int m = 0; m < MT; ++m)
      if (m < s.mt) acc[m] = mfma_parts<T>(op.wf[m], xf, acc[m]);
  };
  Operands opa, opb;
  fetch(0, opa);
  for (int ks = 0; ks < s.nks; ks += 2) {
    if (ks + 1 < s.nks) fetch(ks + 1, opb);
    multiply(opa);
    if (ks + 1 < s.nks) {
      if (ks + 2 < s.nks) fetch(ks + 2, opa);
      multiply(opb);
    }
  }

  store_tiles<T, OUT_NHWC, MT>(acc, out, b, hw, p0, px, live, hh, g, s.og, s.o);
}

bool dtype_ok(int d) { return d == DHD_F32 || d == DHD_F16 || d == DHD_BF16; }

bool precision_supported(int x_dtype, int layout, int gemm) {
  if (layout != 0 && layout != 1) return false;
  if (x_dtype == DHD_F32) return gemm == DHD_SFA_GEMM_DEFAULT || gemm == DHD_SFA_GEMM_BF16X3;
  if (x_dtype == DHD_F16 || x_dtype == DHD_BF16) return gemm == DHD_SFA_GEMM_DEFAULT;   // gemm selects float32 arithmetic only
  return false;
}

bool shape_supported(int c, int o, int groups, int k, int h, int w) {
  if (c <= 0 || o <= 0 || groups <= 0 || h <= 0 || w <= 0 || k != 3 || c % groups || o % groups) return false;
  const int cg = c / groups, og = o / groups;
  if (cg % 8 || og % 8 || cg > 128 || og > 128) return false;
  const long hw = (long)h * w;
  return hw * c < (1L << 31) && hw * o < (1L << 31);
}

Shape make_shape(int c, int o, int groups, int h, int w, int pad, int dil) {
  Shape s;
  s.c = c; s.o = o; s.groups = groups; s.cg = c / groups; s.og = o / groups; s.h = h; s.w = w; s.pad = pad; s.dil = dil;
  s.nks = (kTaps * s.cg + 15) / 16;
  s.mt = (s.og + 31) / 32;
  return s;
}

// scratch: the weight stream, rounded up to 256 bytes, then the channels_last copy of an NCHW x
size_t stream_bytes(const Shape& s, int x_dtype) {
  const size_t n = (size_t)s.groups * s.nks * s.mt * (x_dtype == DHD_F32 ? 2 : 1) * 1024;
  return (n + 255) / 256 * 256;
}
size_t scratch_total(const Shape& s, int b, int x_dtype, int layout) {
  const size_t esz = x_dtype == DHD_F32 ? 4 : 2;
  const size_t copy = layout == 0 ? ((size_t)b * s.c * s.h * s.w * esz + 15) / 16 * 16 : 0;
  return stream_bytes(s, x_dtype) + copy;
}

template <class T>
int launch(const void* x, int layout, const float* offset, const float* weight, void* out, int b, const Shape& s, void* scratch,
           size_t wbytes, void* stream) {
  hipStream_t st = dhd_stream(stream);
  u32x4* wstream = static_cast<u32x4*>(scratch);
  const long n_pack = (long)s.groups * s.nks * s.mt * kParts<T> * 64;
  hipLaunchKernelGGL(pack_weights_kernel<T>, dim3(dhd_cdiv(n_pack, kPackBlock)), dim3(kPackBlock), 0, st, weight, wstream, s);
  DHD_LAUNCH_CHECK();
  const T* xc = static_cast<const T*>(x);
  if (layout == 0) {
    T* copy = reinterpret_cast<T*>(static_cast<char*>(scratch) + wbytes);
    const int rc = dhd_transpose_batched(x, copy, (int)sizeof(T), b, s.c, s.h * s.w, stream);
    if (rc != DHD_OK) return rc;
    xc = copy;
  }
  const int tiles = dhd_cdiv((long)s.h * s.w, kPix);
  const dim3 grid((unsigned)((long)b * tiles * s.groups));
  T* o = static_cast<T*>(out);
  auto go = [&](auto mt_tag) {
    constexpr int MT = decltype(mt_tag)::value;
    if (layout) hipLaunchKernelGGL((deform_conv_kernel<T, true, MT>), grid, dim3(kBlock), 0, st, xc, offset, wstream, o, s, tiles);
    else hipLaunchKernelGGL((deform_conv_kernel<T, false, MT>), grid, dim3(kBlock), 0, st, xc, offset, wstream, o, s, tiles);
  };
  if (s.mt == 1) go(std::integral_constant<int, 1>{});
  else if (s.mt == 2) go(std::integral_constant<int, 2>{});
  else go(std::integral_constant<int, kMaxMT>{});
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

}  // namespace

#include "deform_conv_train.h"

extern "C" {

int dhd_deform_conv_infer_supported(int c_in, int c_out, int groups, int k, int h, int w, int x_dtype, int layout, int gemm) {
  return shape_supported(c_in, c_out, groups, k, h, w) && precision_supported(x_dtype, layout, gemm) ? 1 : 0;
}

int dhd_deform_conv_infer_scratch_bytes(int b, int c_in, int c_out, int groups, int k, int h, int w, int x_dtype, int layout,
                                        size_t* bytes) {
  if (!bytes || b <= 0 || c_in <= 0 || c_out <= 0 || groups <= 0 || h <= 0 || w <= 0 || !dtype_ok(x_dtype) || (layout != 0 && layout != 1))
    return DHD_EINVAL;
  if (c_in % groups || c_out % groups) return DHD_EINVAL;
  if (!shape_supported(c_in, c_out, groups, k, h, w)) return DHD_EUNSUPPORTED;
  *bytes = scratch_total(make_shape(c_in, c_out, groups, h, w, 0, 1), b, x_dtype, layout);
  return DHD_OK;
}

int dhd_deform_conv_infer(const void* x, int x_dtype, int layout, const float* offset, const float* weight, void* out, int b, int c_in,
                          int c_out, int groups, int h, int w, int k, int pad, int dil, int gemm, void* scratch, size_t scratch_bytes,
                          void* stream) {
  if (!x || !offset || !weight || !out || !scratch) return DHD_EINVAL;
  if (b <= 0 || c_in <= 0 || c_out <= 0 || groups <= 0 || h <= 0 || w <= 0 || k <= 0 || pad < 0 || dil < 1) return DHD_EINVAL;
  if (!dtype_ok(x_dtype) || (layout != 0 && layout != 1) || gemm < DHD_SFA_GEMM_DEFAULT || gemm > DHD_SFA_GEMM_BF16X3) return DHD_EINVAL;
  if (c_in % groups || c_out % groups) return DHD_EINVAL;
  if (!dhd_deform_conv_infer_supported(c_in, c_out, groups, k, h, w, x_dtype, layout, gemm)) return DHD_EUNSUPPORTED;
  const long hw = (long)h * w, tiles = (hw + kPix - 1) / kPix;
  // flat element indices of offset (18 planes) in 32 bits on the device; one block per (image, pixel tile, group)
  if (b * hw * c_in >= (1L << 31) || b * hw * c_out >= (1L << 31) || b * hw * 2 * kTaps >= (1L << 31) || (long)pad + 2L * dil + h + w >= (1L << 30) ||
      b * tiles * groups >= (1L << 31))
    return DHD_EUNSUPPORTED;
  const Shape s = make_shape(c_in, c_out, groups, h, w, pad, dil);
  if (scratch_bytes < scratch_total(s, b, x_dtype, layout)) return DHD_ENOSPACE;
  // x's corner runs, the weight stream and a channels_last out move as 16-byte vectors; offset and weight are read by element
  if (!dhd_aligned(16, x, out, scratch) || !dhd_aligned(4, offset, weight)) return DHD_EINVAL;
  const size_t wbytes = stream_bytes(s, x_dtype);
  return dhd::with_dtype<dhd::NativeHalf>(x_dtype, [&](auto* tp) {
    using T = std::remove_pointer_t<decltype(tp)>;
    return launch<T>(x, layout, offset, weight, out, b, s, scratch, wbytes, stream);
  });
}

}  // extern "C"
