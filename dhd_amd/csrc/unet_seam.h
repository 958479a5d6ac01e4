// The seams of the UNets (capi_unet/dhd_amd_unet_seam.h), included at the end of upsample.hip: the 2 x 2 max pooling of `_Down`
// without an index tensor, and ConvTranspose2d(2, stride 2) + pad + cat of `_Up` as one kernel that writes into the concatenated
// tensor, with the backward of both.
//
// Pooling.  THE RULE lives in pool_winner() and nowhere else; forward and backward both call it.  The backward has one thread per
// 2 x 2 cell of the INPUT (cells of a dropped row / column included), which writes the cell's elements of gx exactly once.
//
// Up seam.  Product P = Wp X^T with Wp the packed weight (row n = q cout + co, q = 2 dy + dx; cin contiguous) as the A operand
// of v_mfma_f32_16x16x32 and 16 x1 pixels as the B operand: both fragments are 16 consecutive bytes of a row whose k runs
// contiguously, so they are read straight from global memory (the weight from L2, x1 once per column tile) and no LDS stage
// exists.  The result fragment holds 4 consecutive ROWS per lane; row r of fragment f is given the product row
// base + 8 (r >> 2) + 4 f + (r & 3), so that the two fragments of a lane are 8 consecutive channels of one pixel: one 16-byte
// store (two for float32) through store_b128_guarded, whose descriptor covers exactly the output tensor.  A workgroup is 4
// waves = DHDN_UP_ROWS pixels x DHDN_UP_COLS product rows, a wave 32 x 32.  float32 tensors multiply as three bf16 products.
// The copy of x2 and the zero border are a grid-stride loop of 16-byte vectors over the whole grid, in the same launch.
// The backward is the same kernel shape with Wb (row ci; n contiguous) as A and the gathered gradient as B; the workgroups of
// column tile 0 also write the gathered operand G and a partial row of dbias (fixed order, no atomics).
#pragma once
#include "sfa_mfma.h"

// The constants of capi_unet/dhd_amd_unet_seam.h, restated: that header is compiled with include/ on the include path, which
// the library's own build does not have (tests/test_unet_seam_capi.py holds the two sets of values equal).
#define DHDN_NCHW 0
#define DHDN_NHWC 1
#define DHDN_UP_ROWS 32
#define DHDN_UP_COLS 128

namespace dhd_unet {

using namespace dhd_sfa;

constexpr int kBlock = 256;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

// ------------------------------------------------------------------------------------------------ elements of a 16-byte vector
template <class T> using Raw = std::conditional_t<std::is_same_v<T, float>, float, unsigned short>;
template <class T> struct Arr { Raw<T> e[kVec16<T>]; };

template <class T> __device__ __forceinline__ float raw_f(Raw<T> r) {
  if constexpr (std::is_same_v<T, float>) return r;
  else if constexpr (std::is_same_v<T, _Float16>) return (float)__builtin_bit_cast(_Float16, r);
  else return __uint_as_float((unsigned)r << 16);
}
// 0 + g in torch's accumulation: the bits of g, a negative zero becomes +0
template <class T> __device__ __forceinline__ Raw<T> grad_bits(Raw<T> g) {
  if constexpr (std::is_same_v<T, float>) return g + 0.f;
  else return g == (unsigned short)0x8000u ? (unsigned short)0 : g;
}

// THE RULE of N1: the winner of a window scanned (0,0), (0,1), (1,0), (1,1)
__device__ __forceinline__ int pool_winner(float a, float b, float c, float d) {
  float m = -__builtin_inff();
  int w = 0;
  if (a > m || __builtin_isnan(a)) { m = a; w = 0; }
  if (b > m || __builtin_isnan(b)) { m = b; w = 1; }
  if (c > m || __builtin_isnan(c)) { m = c; w = 2; }
  if (d > m || __builtin_isnan(d)) { m = d; w = 3; }
  return w;
}

// the winner's element, as a chain of selects (a nested conditional becomes an indexed read of a table in private memory)
template <class R> __device__ __forceinline__ R pool_pick(int win, R a, R b, R c, R d) {
  R r = a;
  r = win == 1 ? b : r;
  r = win == 2 ? c : r;
  r = win == 3 ? d : r;
  return r;
}

inline int grid_for(long work) {
  const long b = (work + kBlock - 1) / kBlock;
  return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

// ------------------------------------------------------------------------------------------------ pooling, channels_last
template <class T>
__global__ __launch_bounds__(kBlock) void pool_fwd_nhwc(const T* __restrict__ x, T* __restrict__ y, int B, int C, int H, int W) {
  constexpr int N = kVec16<T>;
  using V = Vec16<T, false>;
  const int nv = C / N, Ho = H / 2, Wo = W / 2;
  const long total = (long)B * Ho * Wo * nv;
  for (long idx = (long)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (long)gridDim.x * kBlock) {
    const int v = (int)(idx % nv);
    const long pix = idx / nv;
    const int j = (int)(pix % Wo), i = (int)((pix / Wo) % Ho);
    const long b = pix / ((long)Wo * Ho);
    const T* p = x + ((b * H + 2 * i) * W + 2 * j) * (long)C + v * N;
    Arr<T> in[4];
    in[0] = __builtin_bit_cast(Arr<T>, V::ld(p));
    in[1] = __builtin_bit_cast(Arr<T>, V::ld(p + C));
    in[2] = __builtin_bit_cast(Arr<T>, V::ld(p + (long)W * C));
    in[3] = __builtin_bit_cast(Arr<T>, V::ld(p + (long)W * C + C));
    Arr<T> o;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const int win = pool_winner(raw_f<T>(in[0].e[k]), raw_f<T>(in[1].e[k]), raw_f<T>(in[2].e[k]), raw_f<T>(in[3].e[k]));
      o.e[k] = pool_pick(win, in[0].e[k], in[1].e[k], in[2].e[k], in[3].e[k]);
    }
    V::st(y + pix * C + v * N, 0, __builtin_bit_cast(raw16<T>, o));
  }
}

template <class T>
__global__ __launch_bounds__(kBlock) void pool_bwd_nhwc(const T* __restrict__ x, const T* __restrict__ gy, T* __restrict__ gx, int B, int C,
                                                        int H, int W) {
  constexpr int N = kVec16<T>;
  using V = Vec16<T, false>;
  const int nv = C / N, Ho = H / 2, Wo = W / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const long total = (long)B * Hc * Wc * nv;
  for (long idx = (long)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (long)gridDim.x * kBlock) {
    const int v = (int)(idx % nv);
    const long cell = idx / nv;
    const int j = (int)(cell % Wc), i = (int)((cell / Wc) % Hc);
    const long b = cell / ((long)Wc * Hc);
    const long at = ((b * H + 2 * i) * W + 2 * j) * (long)C + v * N;     // element (2 i, 2 j) of the cell: always inside
    Arr<T> o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int k = 0; k < N; ++k) o[q].e[k] = 0;
    if (i < Ho && j < Wo) {                                              // a whole window
      const T* p = x + at;
      Arr<T> in[4];
      in[0] = __builtin_bit_cast(Arr<T>, V::ld(p));
      in[1] = __builtin_bit_cast(Arr<T>, V::ld(p + C));
      in[2] = __builtin_bit_cast(Arr<T>, V::ld(p + (long)W * C));
      in[3] = __builtin_bit_cast(Arr<T>, V::ld(p + (long)W * C + C));
      const Arr<T> g = __builtin_bit_cast(Arr<T>, V::ld(gy + ((b * Ho + i) * Wo + j) * (long)C + v * N));
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const int win = pool_winner(raw_f<T>(in[0].e[k]), raw_f<T>(in[1].e[k]), raw_f<T>(in[2].e[k]), raw_f<T>(in[3].e[k]));
        const Raw<T> gb = grad_bits<T>(g.e[k]);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q].e[k] = win == q ? gb : (Raw<T>)0;
      }
    }
    const bool right = 2 * j + 1 < W, below = 2 * i + 1 < H;
    V::st(gx + at, 0, __builtin_bit_cast(raw16<T>, o[0]));
    if (right) V::st(gx + at + C, 0, __builtin_bit_cast(raw16<T>, o[1]));
    if (below) V::st(gx + at + (long)W * C, 0, __builtin_bit_cast(raw16<T>, o[2]));
    if (right && below) V::st(gx + at + (long)W * C + C, 0, __builtin_bit_cast(raw16<T>, o[3]));
  }
}

// ------------------------------------------------------------------------------------------------ pooling, NCHW (single elements)
template <class T>
__global__ __launch_bounds__(kBlock) void pool_fwd_nchw(const T* __restrict__ x, T* __restrict__ y, long planes, int H, int W) {
  const Raw<T>* xr = reinterpret_cast<const Raw<T>*>(x);
  Raw<T>* yr = reinterpret_cast<Raw<T>*>(y);
  const int Ho = H / 2, Wo = W / 2;
  const long total = planes * Ho * Wo;
  for (long idx = (long)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (long)gridDim.x * kBlock) {
    const int j = (int)(idx % Wo), i = (int)((idx / Wo) % Ho);
    const long pl = idx / ((long)Wo * Ho);
    const Raw<T>* p = xr + (pl * H + 2 * i) * W + 2 * j;
    const Raw<T> a = p[0], b = p[1], c = p[W], d = p[W + 1];
    const int win = pool_winner(raw_f<T>(a), raw_f<T>(b), raw_f<T>(c), raw_f<T>(d));
    yr[idx] = pool_pick(win, a, b, c, d);
  }
}

template <class T>
__global__ __launch_bounds__(kBlock) void pool_bwd_nchw(const T* __restrict__ x, const T* __restrict__ gy, T* __restrict__ gx, long planes,
                                                        int H, int W) {
  const Raw<T>* xr = reinterpret_cast<const Raw<T>*>(x);
  const Raw<T>* gr = reinterpret_cast<const Raw<T>*>(gy);
  Raw<T>* o = reinterpret_cast<Raw<T>*>(gx);
  const int Ho = H / 2, Wo = W / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const long total = planes * Hc * Wc;
  for (long idx = (long)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (long)gridDim.x * kBlock) {
    const int j = (int)(idx % Wc), i = (int)((idx / Wc) % Hc);
    const long pl = idx / ((long)Wc * Hc);
    const long at = (pl * H + 2 * i) * W + 2 * j;
    int win = -1;
    Raw<T> gb = 0;
    if (i < Ho && j < Wo) {
      const Raw<T>* p = xr + at;
      win = pool_winner(raw_f<T>(p[0]), raw_f<T>(p[1]), raw_f<T>(p[W]), raw_f<T>(p[W + 1]));
      gb = grad_bits<T>(gr[(pl * Ho + i) * Wo + j]);
    }
    const bool right = 2 * j + 1 < W, below = 2 * i + 1 < H;
    o[at] = win == 0 ? gb : (Raw<T>)0;
    if (right) o[at + 1] = win == 1 ? gb : (Raw<T>)0;
    if (below) o[at + W] = win == 2 ? gb : (Raw<T>)0;
    if (right && below) o[at + W + 1] = win == 3 ? gb : (Raw<T>)0;
  }
}

inline bool dtype_ok(int d) { return d == DHD_F32 || d == DHD_F16 || d == DHD_BF16; }
inline int esize(int d) { return d == DHD_F32 ? 4 : 2; }

inline bool pool_ok(int dtype, int layout, int b, int c, int h, int w) {
  if (!dtype_ok(dtype) || (layout != DHDN_NCHW && layout != DHDN_NHWC) || b < 1 || c < 1 || h < 2 || w < 2) return false;
  if (layout == DHDN_NHWC && c % 8) return false;
  return (long)b * c * h * w < (1L << 40);
}

inline int pool_run(bool bwd, const void* x, const void* gy, void* out, int dtype, int layout, int b, int c, int h, int w, void* stream) {
  if (!x || !out || (bwd && !gy)) return DHD_EINVAL;
  if (!dhd_aligned(layout == DHDN_NHWC ? 16 : esize(dtype), x, gy, out)) return DHD_EINVAL;
  if (b < 1 || c < 1 || h < 1 || w < 1) return DHD_EINVAL;
  if (!pool_ok(dtype, layout, b, c, h, w)) return DHD_EUNSUPPORTED;
  hipStream_t st = dhd_stream(stream);
  return with_dtype<NativeHalf>(dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    const long cells = bwd ? (long)b * ((h + 1) / 2) * ((w + 1) / 2) : (long)b * (h / 2) * (w / 2);
    if (layout == DHDN_NHWC) {
      const int blocks = grid_for(cells * (c / kVec16<T>));
      if (bwd) hipLaunchKernelGGL(pool_bwd_nhwc<T>, dim3(blocks), dim3(kBlock), 0, st, (const T*)x, (const T*)gy, (T*)out, b, c, h, w);
      else hipLaunchKernelGGL(pool_fwd_nhwc<T>, dim3(blocks), dim3(kBlock), 0, st, (const T*)x, (T*)out, b, c, h, w);
    } else {
      const int blocks = grid_for(cells * c);
      if (bwd) hipLaunchKernelGGL(pool_bwd_nchw<T>, dim3(blocks), dim3(kBlock), 0, st, (const T*)x, (const T*)gy, (T*)out, (long)b * c, h, w);
      else hipLaunchKernelGGL(pool_fwd_nchw<T>, dim3(blocks), dim3(kBlock), 0, st, (const T*)x, (T*)out, (long)b * c, h, w);
    }
    DHD_LAUNCH_CHECK();
    return (int)DHD_OK;
  });
}

// ------------------------------------------------------------------------------------------------ the up seam
struct UpGeom {
  int B, Cin, Cout, C2, h, w, H, W, top, left;
};

template <class T> constexpr int kParts = std::is_same_v<T, float> ? 2 : 1;

template <class T> __device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
  if constexpr (std::is_same_v<T, _Float16>)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// 8 consecutive k of a tensor row as operand words: the row's own 16 bytes, or the high and mid bf16 parts of 8 floats
template <class T> struct Frag { u32x4 part[kParts<T>]; };
template <class T> __device__ __forceinline__ Frag<T> tensor_frag(const T* p) {
  Frag<T> f;
  if constexpr (std::is_same_v<T, float>) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    unsigned hi[4], mid[4];
    split2_hm(a[0], a[1], hi[0], mid[0]);
    split2_hm(a[2], a[3], hi[1], mid[1]);
    split2_hm(b[0], b[1], hi[2], mid[2]);
    split2_hm(b[2], b[3], hi[3], mid[3]);
    f.part[0] = u32x4{hi[0], hi[1], hi[2], hi[3]};
    f.part[1] = u32x4{mid[0], mid[1], mid[2], mid[3]};
  } else {
    f.part[0] = *reinterpret_cast<const u32x4*>(p);
  }
  return f;
}
// the packed weight: 16-bit operands, part 1 (float32 tensors only) `part_stride` elements behind part 0
template <class T> __device__ __forceinline__ Frag<T> weight_frag(const unsigned short* p, size_t part_stride) {
  Frag<T> f;
#pragma unroll
  for (int s = 0; s < kParts<T>; ++s) f.part[s] = *reinterpret_cast<const u32x4*>(p + s * part_stride);
  return f;
}
// acc += a b: one product, or high x mid + mid x high + high x high
template <class T> __device__ __forceinline__ f32x4 product(const Frag<T>& a, const Frag<T>& b, f32x4 acc) {
  if constexpr (std::is_same_v<T, float>) {
    acc = mfma16<T>(a.part[0], b.part[1], acc);
    acc = mfma16<T>(a.part[1], b.part[0], acc);
  }
  return mfma16<T>(a.part[0], b.part[0], acc);
}

// a lane's 8 consecutive results (two fragments of 4) -> one 16-byte store, two for float32; byte_off of the first
template <class T>
__device__ __forceinline__ void store8(const float* v, __amdgpu_buffer_rsrc_t rsrc, int byte_off) {
  if constexpr (std::is_same_v<T, float>) {
    store_b128_guarded<0>(u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])}, rsrc, byte_off, 0);
    store_b128_guarded<0>(u32x4{__float_as_uint(v[4]), __float_as_uint(v[5]), __float_as_uint(v[6]), __float_as_uint(v[7])}, rsrc, byte_off + 16, 0);
  } else {
    store_b128_guarded<0>(narrow16<T>(v), rsrc, byte_off, 0);
  }
}

// the weight (cin, cout, 2, 2) of TW -> 16-bit MFMA operands of T's products, through an LDS tile of 32 ci x 16 co x 4 q.
//   BWD == false:  wp[part][q cout + co][ci]      BWD == true:  wb[part][ci][q cout + co]
template <class TW, class T, bool BWD>
__global__ __launch_bounds__(kBlock) void pack_weight(const TW* __restrict__ wgt, unsigned short* __restrict__ dst, int Cin, int Cout) {
  __shared__ float tile[32][65];
  const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 16, NC = 4 * Cout;
  const Raw<TW>* src = reinterpret_cast<const Raw<TW>*>(wgt);
  for (int e = threadIdx.x; e < 32 * 64; e += kBlock) {
    const int ci = e >> 6, r = e & 63;                                   // r = 4 co + q: 64 consecutive source elements
    tile[ci][r] = raw_f<TW>(src[((size_t)(ci0 + ci) * Cout + co0) * 4 + r]);
  }
  __syncthreads();
  const size_t part_stride = (size_t)NC * Cin;
  for (int e = threadIdx.x; e < 32 * 64; e += kBlock) {
    int ci, co, q;
    size_t at;
    if constexpr (BWD) {
      co = e & 15, q = (e >> 4) & 3, ci = e >> 6;
      at = (size_t)(ci0 + ci) * NC + q * Cout + co0 + co;
    } else {
      ci = e & 31, co = (e >> 5) & 15, q = e >> 9;
      at = (size_t)(q * Cout + co0 + co) * Cin + ci0 + ci;
    }
    const float v = tile[ci][4 * co + q];
    if constexpr (std::is_same_v<T, float>) {
      unsigned h, m;
      split2_hm(v, 0.f, h, m);
      dst[at] = (unsigned short)h;
      dst[at + part_stride] = (unsigned short)m;
    } else {
      dst[at] = (unsigned short)Pair<T>::narrow(f32x2{v, 0.f});
    }
  }
}

// The 16-byte vectors of the concatenated tensor that the product does not write: channels 0 .. C2 from / to the dense x2-shaped
// tensor (FWD: out <- x2; else gx2 <- gout), and in the forward the zero border of channels C2 .. C2 + Cout.
template <class T, bool FWD>
__device__ __forceinline__ void skip_half(const T* __restrict__ from, T* __restrict__ to, const UpGeom& g) {
  constexpr int N = kVec16<T>;
  using V = Vec16<T, false>;
  const int Ct = g.C2 + g.Cout, nvt = Ct / N, nv2 = g.C2 / N;
  const long nwg = (long)gridDim.x * gridDim.y, wg = (long)blockIdx.y * gridDim.x + blockIdx.x;
  if (!FWD && !to) return;
  const bool border = FWD && (g.H != 2 * g.h || g.W != 2 * g.w);
  const int nv = border ? nvt : nv2;                                     // vectors looked at per pixel
  const long total = (long)g.B * g.H * g.W * nv;
  for (long idx = wg * kBlock + threadIdx.x; idx < total; idx += nwg * kBlock) {
    const int cv = (int)(idx % nv);
    const long pix = idx / nv;
    if (cv < nv2) {
      if constexpr (FWD) V::st(to + pix * Ct + cv * N, 0, V::ld(from + pix * g.C2 + cv * N));
      else V::st(to + pix * g.C2 + cv * N, 0, V::ld(from + pix * Ct + cv * N));
    } else {
      const int ox = (int)(pix % g.W), oy = (int)((pix / g.W) % g.H);
      if (oy < g.top || oy >= g.top + 2 * g.h || ox < g.left || ox >= g.left + 2 * g.w) {
        raw16<T> z;
#pragma unroll
        for (int k = 0; k < 4; ++k) z[k] = 0;
        V::st(to + pix * Ct + cv * N, 0, z);
      }
    }
  }
}

// element offset of channel C2 of output pixel (2 y + top, 2 x + left) of x1 pixel p
__device__ __forceinline__ long out_base(int p, const UpGeom& g) {
  const int hw = g.h * g.w, b = p / hw, rem = p - b * hw, y = rem / g.w, x = rem - y * g.w;
  return (((long)b * g.H + 2 * y + g.top) * g.W + 2 * x + g.left) * (long)(g.C2 + g.Cout) + g.C2;
}

template <class T>
__global__ __launch_bounds__(kBlock) void up_cat_fwd(const T* __restrict__ x1, const T* __restrict__ x2, const unsigned short* __restrict__ wp,
                                                     const float* __restrict__ bias, T* __restrict__ out, UpGeom g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g4 = lane >> 4;
  const int R = g.B * g.h * g.w, NC = 4 * g.Cout, Ct = g.C2 + g.Cout, Cin = g.Cin;
  const int p0 = blockIdx.x * DHDN_UP_ROWS, nb = blockIdx.y * DHDN_UP_COLS + wave * 32;
  if (nb < NC) {                                                         // wave-uniform; 4 cout is a multiple of 32
    const size_t part_stride = (size_t)NC * Cin;
    const unsigned short* wa[2];
    const T* xb[2];
    int pix[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) wa[f] = wp + (size_t)(nb + (r >> 2) * 8 + f * 4 + (r & 3)) * Cin + 8 * g4;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      pix[t] = p0 + 16 * t + r;
      xb[t] = x1 + (size_t)min(pix[t], R - 1) * Cin + 8 * g4;             // a row past the end reads the last row and stores nothing
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int f = 0; f < 2; ++f) acc[t][f] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < Cin; k0 += 32) {
      Frag<T> a[2], b[2];
#pragma unroll
      for (int f = 0; f < 2; ++f) a[f] = weight_frag<T>(wa[f] + k0, part_stride);
#pragma unroll
      for (int t = 0; t < 2; ++t) b[t] = tensor_frag<T>(xb[t] + k0);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int f = 0; f < 2; ++f) acc[t][f] = product<T>(a[f], b[t], acc[t][f]);
    }
    // this lane: channels n8 .. n8 + 8 of the product, all of one quadrant (cout is a multiple of 16)
    const int n8 = nb + 8 * g4, q = n8 / g.Cout, co = n8 - q * g.Cout;
    float bv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) bv[k] = bias ? bias[co + k] : 0.f;
    const __amdgpu_buffer_rsrc_t ro =
        __builtin_amdgcn_make_buffer_rsrc(out, 0, (unsigned)((size_t)g.B * g.H * g.W * Ct * sizeof(T)), 0x00020000);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (pix[t] < R) {
        const long at = out_base(pix[t], g) + ((long)(q >> 1) * g.W + (q & 1)) * Ct + co;
        float v[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v[k] = acc[t][0][k] + bv[k];
          v[4 + k] = acc[t][1][k] + bv[4 + k];
        }
        store8<T>(v, ro, (int)(at * (long)sizeof(T)));
      }
    }
  }
  skip_half<T, true>(x2, out, g);
}

// gx1 = G Wb^T; column tile 0 also writes G (gop) and the workgroup's partial row of dbias (partial), either may be null
template <class T>
__global__ __launch_bounds__(kBlock) void up_cat_bwd(const T* __restrict__ gout, const unsigned short* __restrict__ wb, T* __restrict__ gx1,
                                                     T* __restrict__ gx2, T* __restrict__ gop, float* __restrict__ partial, UpGeom g) {
  __shared__ float sums[kBlock * 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g4 = lane >> 4;
  const int R = g.B * g.h * g.w, NC = 4 * g.Cout, Ct = g.C2 + g.Cout, Cin = g.Cin;
  const int p0 = blockIdx.x * DHDN_UP_ROWS, cb = blockIdx.y * DHDN_UP_COLS + wave * 32;
  if (cb < Cin) {                                                        // wave-uniform; cin is a multiple of 32
    const size_t part_stride = (size_t)NC * Cin;
    const unsigned short* wa[2];
    const T* gb[2];
    int pix[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) wa[f] = wb + (size_t)(cb + (r >> 2) * 8 + f * 4 + (r & 3)) * NC + 8 * g4;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      pix[t] = p0 + 16 * t + r;
      gb[t] = gout + out_base(min(pix[t], R - 1), g);
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int f = 0; f < 2; ++f) acc[t][f] = f32x4{0.f, 0.f, 0.f, 0.f};
    int q = 0, co = 8 * g4;                                              // k0 + 8 g4 = q cout + co
    for (int k0 = 0; k0 < NC; k0 += 32) {
      while (co >= g.Cout) { co -= g.Cout; ++q; }
      const long off = ((long)(q >> 1) * g.W + (q & 1)) * Ct + co;
      Frag<T> a[2], b[2];
#pragma unroll
      for (int f = 0; f < 2; ++f) a[f] = weight_frag<T>(wa[f] + k0, part_stride);
#pragma unroll
      for (int t = 0; t < 2; ++t) b[t] = tensor_frag<T>(gb[t] + off);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int f = 0; f < 2; ++f) acc[t][f] = product<T>(a[f], b[t], acc[t][f]);
      co += 32;
    }
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(gx1, 0, (unsigned)((size_t)R * Cin * sizeof(T)), 0x00020000);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (pix[t] < R) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v[k] = acc[t][0][k];
          v[4 + k] = acc[t][1][k];
        }
        store8<T>(v, ro, (int)(((long)pix[t] * Cin + cb + 8 * g4) * (long)sizeof(T)));
      }
    }
  }
  if (blockIdx.y == 0 && (gop || partial)) {                             // block-uniform
    constexpr int N = kVec16<T>;
    using V = Vec16<T, false>;
    const int nv = g.Cout / N, L = kBlock / nv;                          // nv <= 128: at least two pixel lanes
    const int cv = threadIdx.x % nv, pl = threadIdx.x / nv;
    float s[N];
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = 0.f;
    if (pl < L) {
      for (int j = pl; j < 4 * DHDN_UP_ROWS; j += L) {                   // (pixel of the tile, quadrant)
        const int p = p0 + (j >> 2), qq = j & 3;
        if (p >= R) break;
        const raw16<T> w16 = V::ld(gout + out_base(p, g) + ((long)(qq >> 1) * g.W + (qq & 1)) * Ct + cv * N);
        if (gop) V::st(gop + (size_t)p * NC + qq * g.Cout + cv * N, 0, w16);
        float v[N];
        widen16<T>(w16, v);
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] += v[k];
      }
#pragma unroll
      for (int k = 0; k < N; ++k) sums[pl * g.Cout + cv * N + k] = s[k];
    }
    __syncthreads();
    if (partial) {
      for (int c = threadIdx.x; c < g.Cout; c += kBlock) {
        float tot = 0.f;
        for (int l = 0; l < L; ++l) tot += sums[l * g.Cout + c];
        partial[(size_t)blockIdx.x * g.Cout + c] = tot;
      }
    }
  }
  skip_half<T, false>(gout, gx2, g);
}

// dbias[co] = sum of the partial rows in index order: 16 channels per workgroup, 16 row lanes, then the lanes in order
__global__ __launch_bounds__(kBlock) void up_cat_dbias(const float* __restrict__ partial, float* __restrict__ dbias, int rows, int Cout) {
  __shared__ float s[16][17];
  const int c = threadIdx.x & 15, l = threadIdx.x >> 4, co = blockIdx.x * 16 + c;
  float tot = 0.f;
  for (int rt = l; rt < rows; rt += 16) tot += partial[(size_t)rt * Cout + co];
  s[l][c] = tot;
  __syncthreads();
  if (l == 0) {
    float v = 0.f;
    for (int k = 0; k < 16; ++k) v += s[k][c];
    dbias[co] = v;
  }
}

inline bool upcat_ok(int dtype, int layout, int b, int cin, int cout, int c2, int h, int w, int H, int W) {
  if (!dtype_ok(dtype) || layout != DHDN_NHWC || b < 1 || h < 1 || w < 1) return false;
  if (cin < 32 || cin > 1024 || cin % 32 || cout < 16 || cout > 512 || cout % 16 || c2 < 8 || c2 % 8) return false;
  if (H < 2L * h || W < 2L * w) return false;
  const long lim = 1L << 31, e = esize(dtype);
  return (long)b * H * W * (c2 + cout) * e < lim && (long)b * h * w * cin * e < lim && (long)b * h * w * 4 * cout * e < lim;
}

inline int up_row_tiles(int b, int h, int w) { return (int)(((long)b * h * w + DHDN_UP_ROWS - 1) / DHDN_UP_ROWS); }
inline size_t up_pack_bytes(int dtype, int cin, int cout) { return (size_t)(dtype == DHD_F32 ? 2 : 1) * 4 * cout * cin * 2; }

inline UpGeom up_geom(int b, int cin, int cout, int c2, int h, int w, int H, int W) {
  return UpGeom{b, cin, cout, c2, h, w, H, W, (H - 2 * h) / 2, (W - 2 * w) / 2};
}

template <class T, bool BWD>
int up_pack(const void* weight, int wdtype, void* dst, int cin, int cout, hipStream_t st) {
  return with_dtype<NativeHalf>(wdtype, [&](auto* tw) {
    using TW = std::remove_pointer_t<decltype(tw)>;
    hipLaunchKernelGGL((pack_weight<TW, T, BWD>), dim3(cin / 32, cout / 16), dim3(kBlock), 0, st, (const TW*)weight, (unsigned short*)dst, cin, cout);
    DHD_LAUNCH_CHECK();
    return (int)DHD_OK;
  });
}

}  // namespace dhd_unet

extern "C" {

int dhdn_max_pool2_supported(int dtype, int layout, int b, int c, int h, int w) { return dhd_unet::pool_ok(dtype, layout, b, c, h, w) ? 1 : 0; }

int dhdn_max_pool2_forward(const void* x, void* y, int dtype, int layout, int b, int c, int h, int w, void* stream) {
  return dhd_unet::pool_run(false, x, nullptr, y, dtype, layout, b, c, h, w, stream);
}

int dhdn_max_pool2_backward(const void* x, const void* grad_y, void* grad_x, int dtype, int layout, int b, int c, int h, int w, void* stream) {
  return dhd_unet::pool_run(true, x, grad_y, grad_x, dtype, layout, b, c, h, w, stream);
}

int dhdn_up_cat_supported(int dtype, int layout, int b, int cin, int cout, int c2, int h, int w, int H, int W) {
  return dhd_unet::upcat_ok(dtype, layout, b, cin, cout, c2, h, w, H, W) ? 1 : 0;
}

size_t dhdn_up_cat_scratch_bytes(int dtype, int b, int cin, int cout, int h, int w, int backward) {
  using namespace dhd_unet;
  if (!upcat_ok(dtype, DHDN_NHWC, b, cin, cout, 8, h, w, 2 * h, 2 * w)) return 0;
  size_t n = up_pack_bytes(dtype, cin, cout);
  if (backward) n += (size_t)up_row_tiles(b, h, w) * cout * sizeof(float);
  return (n + 15) / 16 * 16;
}

int dhdn_up_cat_forward(const void* x1, const void* x2, const void* weight, int wdtype, const float* bias, void* out, void* scratch,
                        size_t scratch_bytes, int dtype, int layout, int b, int cin, int cout, int c2, int h, int w, int H, int W,
                        void* stream) {
  using namespace dhd_unet;
  if (!x1 || !x2 || !weight || !out || !scratch) return DHD_EINVAL;
  if (!dhd_aligned(16, x1, x2, weight, out, scratch) || !dhd_aligned(4, bias)) return DHD_EINVAL;
  if (b < 1 || cin < 1 || cout < 1 || c2 < 1 || h < 1 || w < 1 || H < 1 || W < 1) return DHD_EINVAL;
  if (!dtype_ok(wdtype) || !upcat_ok(dtype, layout, b, cin, cout, c2, h, w, H, W)) return DHD_EUNSUPPORTED;
  if (scratch_bytes < dhdn_up_cat_scratch_bytes(dtype, b, cin, cout, h, w, 0)) return DHD_ENOSPACE;
  const UpGeom g = up_geom(b, cin, cout, c2, h, w, H, W);
  hipStream_t st = dhd_stream(stream);
  return with_dtype<NativeHalf>(dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    const int rc = up_pack<T, false>(weight, wdtype, scratch, cin, cout, st);
    if (rc != DHD_OK) return rc;
    const dim3 grid(up_row_tiles(b, h, w), (4 * cout + DHDN_UP_COLS - 1) / DHDN_UP_COLS);
    hipLaunchKernelGGL(up_cat_fwd<T>, grid, dim3(kBlock), 0, st, (const T*)x1, (const T*)x2, (const unsigned short*)scratch, bias, (T*)out, g);
    DHD_LAUNCH_CHECK();
    return (int)DHD_OK;
  });
}

int dhdn_up_cat_backward(const void* grad_out, const void* weight, int wdtype, void* grad_x1, void* grad_x2, void* g_operand,
                         float* dbias, void* scratch, size_t scratch_bytes, int dtype, int layout, int b, int cin, int cout, int c2,
                         int h, int w, int H, int W, void* stream) {
  using namespace dhd_unet;
  if (!grad_out || !weight || !grad_x1 || !scratch) return DHD_EINVAL;
  if (!dhd_aligned(16, grad_out, weight, grad_x1, grad_x2, g_operand, scratch) || !dhd_aligned(4, dbias)) return DHD_EINVAL;
  if (b < 1 || cin < 1 || cout < 1 || c2 < 1 || h < 1 || w < 1 || H < 1 || W < 1) return DHD_EINVAL;
  if (!dtype_ok(wdtype) || !upcat_ok(dtype, layout, b, cin, cout, c2, h, w, H, W)) return DHD_EUNSUPPORTED;
  if (scratch_bytes < dhdn_up_cat_scratch_bytes(dtype, b, cin, cout, h, w, 1)) return DHD_ENOSPACE;
  const UpGeom g = up_geom(b, cin, cout, c2, h, w, H, W);
  hipStream_t st = dhd_stream(stream);
  return with_dtype<NativeHalf>(dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    const int rc = up_pack<T, true>(weight, wdtype, scratch, cin, cout, st);
    if (rc != DHD_OK) return rc;
    const int rows = up_row_tiles(b, h, w);
    float* partial = dbias ? reinterpret_cast<float*>(static_cast<char*>(scratch) + up_pack_bytes(dtype, cin, cout)) : nullptr;
    const dim3 grid(rows, (cin + DHDN_UP_COLS - 1) / DHDN_UP_COLS);
    hipLaunchKernelGGL(up_cat_bwd<T>, grid, dim3(kBlock), 0, st, (const T*)grad_out, (const unsigned short*)scratch, (T*)grad_x1, (T*)grad_x2,
                       (T*)g_operand, partial, g);
    DHD_LAUNCH_CHECK();
    if (dbias) {
      hipLaunchKernelGGL(up_cat_dbias, dim3(cout / 16), dim3(kBlock), 0, st, (const float*)partial, dbias, rows, cout);
      DHD_LAUNCH_CHECK();
    }
    return (int)DHD_OK;
  });
}

}  // extern "C"
