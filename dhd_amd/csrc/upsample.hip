// Bilinear up-sampling with align_corners = True -- nn.Upsample(scale_factor, 'bilinear', align_corners=True) of FPN_LSS
// (necks/lss_fpn.py:27,43) and of the UNets' decoder (backbones/unet.py:86) -- for NCHW and channels_last tensors,
// float32 / float16 / bfloat16.
//   forward : every output element interpolates its four neighbours with torch's index arithmetic
//             (UpSample.cuh: scale = (in - 1) / (out - 1), src = scale * dst, i0 = (int)src, lambda = src - i0) in float32 and rounds once.
//   backward: GATHER form -- one thread per input element (NCHW) or per 16-byte channel vector of an input pixel (channels_last)
//             adds the contributions of the <= (2 s + 2)^2 output pixels that read it, float32 accumulation, one writer per
//             element: no atomics, no memset, deterministic (torch's kernels scatter with atomics, in half precision for half
//             tensors, and its channels_last backward takes 2.3 ms where this one takes the time of reading the gradient once).
#include "vec16.h"

namespace {

constexpr int kUpBlock = 256;

// 16-byte vectors (channels_last kernels), plain access; the NCHW kernels read and write single elements
template <typename T> struct Num : dhd::Vec16<T, false> {
  static __device__ __forceinline__ float get(const T* p) {
    if constexpr (std::is_same_v<T, __half>) return __half2float(*p);
    else if constexpr (std::is_same_v<T, __hip_bfloat16>) return __uint_as_float((unsigned)*reinterpret_cast<const unsigned short*>(p) << 16);
    else return *p;
  }
  static __device__ __forceinline__ void put(T* p, float v) {
    if constexpr (std::is_same_v<T, __half>) *p = __float2half_rn(v);
    else if constexpr (std::is_same_v<T, __hip_bfloat16>) *reinterpret_cast<unsigned short*>(p) = (unsigned short)dhd::bf16_rne(v);
    else *p = v;
  }
};

struct Geom {
  int n, c, hin, win, hout, wout;
  float rh, rw;   // (in - 1) / (out - 1), 0 for out == 1
};

// source cell of output index o: i0 = (int)(r o), the neighbour i0 + ip (ip = 0 on the last cell), lambda of the neighbour
__device__ __forceinline__ void src_cell(float r, int o, int in, int* i0, int* ip, float* l1) {
  const float f = r * (float)o;
  *i0 = (int)f;
  *ip = *i0 < in - 1 ? 1 : 0;
  *l1 = f - (float)*i0;
}

// first output index whose source cell is >= i (i0 is monotonic in o); `out` if there is none
__device__ __forceinline__ int first_out(float r, int i, int out) {
  if (i <= 0) return 0;
  if (r <= 0.f) return out;
  int o = (int)((float)i / r);
  o = min(max(o, 0), out);
  while (o > 0 && (int)(r * (float)(o - 1)) >= i) --o;
  while (o < out && (int)(r * (float)o) < i) ++o;
  return o;
}

// the outputs that read input index i along one axis are [lo, lo + cnt): those whose cell is i - 1 or i
__device__ __forceinline__ int tap_range(float r, int i, int out, int* lo) {
  *lo = first_out(r, i - 1, out);
  return first_out(r, i + 1, out) - *lo;
}
// ... and output o reads it with weight (cell == i) (1 - l1) + (cell + ip == i) l1
__device__ __forceinline__ float tap_weight(float r, int o, int in, int i) {
  int i0, ip; float l1;
  src_cell(r, o, in, &i0, &ip, &l1);
  return (i0 == i ? 1.f - l1 : 0.f) + (i0 + ip == i ? l1 : 0.f);
}

// ------------------------------------------------------------------ NCHW
template <typename T>
__global__ __launch_bounds__(kUpBlock) void up_fwd_nchw(const T* __restrict__ x, T* __restrict__ y, Geom g) {
  const long total = (long)g.n * g.c * g.hout * g.wout;
  for (long idx = (long)blockIdx.x * kUpBlock + threadIdx.x; idx < total; idx += (long)gridDim.x * kUpBlock) {
    const int w2 = (int)(idx % g.wout), h2 = (int)((idx / g.wout) % g.hout);
    const long plane = idx / ((long)g.wout * g.hout);
    int h1, hp, w1, wp; float hl, wl;
    src_cell(g.rh, h2, g.hin, &h1, &hp, &hl);
    src_cell(g.rw, w2, g.win, &w1, &wp, &wl);
    const T* p = x + (plane * g.hin + h1) * g.win + w1;
    const float a = Num<T>::get(p), b = Num<T>::get(p + wp), c = Num<T>::get(p + (long)hp * g.win), d = Num<T>::get(p + (long)hp * g.win + wp);
    const float h0 = 1.f - hl, w0 = 1.f - wl;
    Num<T>::put(y + idx, h0 * (w0 * a + wl * b) + hl * (w0 * c + wl * d));
  }
}

template <typename T>
__global__ __launch_bounds__(kUpBlock) void up_bwd_nchw(const T* __restrict__ gy, T* __restrict__ gx, Geom g) {
  const long total = (long)g.n * g.c * g.hin * g.win;
  for (long idx = (long)blockIdx.x * kUpBlock + threadIdx.x; idx < total; idx += (long)gridDim.x * kUpBlock) {
    const int w1 = (int)(idx % g.win), h1 = (int)((idx / g.win) % g.hin);
    const long plane = idx / ((long)g.win * g.hin);
    int hlo, wlo;
    const int nh = tap_range(g.rh, h1, g.hout, &hlo), nw = tap_range(g.rw, w1, g.wout, &wlo);
    const T* p = gy + (plane * g.hout + hlo) * g.wout + wlo;
    float acc = 0.f;
    for (int a = 0; a < nh; ++a) {
      float row = 0.f;
      for (int b = 0; b < nw; ++b) row = fmaf(tap_weight(g.rw, wlo + b, g.win, w1), Num<T>::get(p + (long)a * g.wout + b), row);
      acc = fmaf(tap_weight(g.rh, hlo + a, g.hin, h1), row, acc);
    }
    Num<T>::put(gx + idx, acc);
  }
}

// ------------------------------------------------------------------ channels_last: [n][h][w][c], one 16-byte vector per thread
template <typename T>
__global__ __launch_bounds__(kUpBlock) void up_fwd_nhwc(const T* __restrict__ x, T* __restrict__ y, Geom g) {
  constexpr int N = Num<T>::N;
  const int V = g.c / N;
  const long total = (long)g.n * g.hout * g.wout * V;
  for (long idx = (long)blockIdx.x * kUpBlock + threadIdx.x; idx < total; idx += (long)gridDim.x * kUpBlock) {
    const int v = (int)(idx % V);
    const long pix = idx / V;
    const int w2 = (int)(pix % g.wout), h2 = (int)((pix / g.wout) % g.hout);
    const long img = pix / ((long)g.wout * g.hout);
    int h1, hp, w1, wp; float hl, wl;
    src_cell(g.rh, h2, g.hin, &h1, &hp, &hl);
    src_cell(g.rw, w2, g.win, &w1, &wp, &wl);
    const T* p = x + (((img * g.hin + h1) * g.win + w1) * (long)g.c) + v * N;
    float a[N], b[N], c[N], d[N], o[N];
    Num<T>::load(p, a);
    Num<T>::load(p + (long)wp * g.c, b);
    Num<T>::load(p + (long)hp * g.win * g.c, c);
    Num<T>::load(p + ((long)hp * g.win + wp) * g.c, d);
    const float h0 = 1.f - hl, w0 = 1.f - wl;
#pragma unroll
    for (int k = 0; k < N; ++k) o[k] = h0 * (w0 * a[k] + wl * b[k]) + hl * (w0 * c[k] + wl * d[k]);
    Num<T>::store(y + pix * g.c + v * N, o);
  }
}

template <typename T>
__global__ __launch_bounds__(kUpBlock) void up_bwd_nhwc(const T* __restrict__ gy, T* __restrict__ gx, Geom g) {
  constexpr int N = Num<T>::N;
  const int V = g.c / N;
  const long total = (long)g.n * g.hin * g.win * V;
  for (long idx = (long)blockIdx.x * kUpBlock + threadIdx.x; idx < total; idx += (long)gridDim.x * kUpBlock) {
    const int v = (int)(idx % V);
    const long pix = idx / V;
    const int w1 = (int)(pix % g.win), h1 = (int)((pix / g.win) % g.hin);
    const long img = pix / ((long)g.win * g.hin);
    int hlo, wlo;
    const int nh = tap_range(g.rh, h1, g.hout, &hlo), nw = tap_range(g.rw, w1, g.wout, &wlo);
    const T* p = gy + ((img * g.hout + hlo) * g.wout + wlo) * (long)g.c + v * N;
    float acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.f;
    for (int a = 0; a < nh; ++a) {
      const float wa = tap_weight(g.rh, hlo + a, g.hin, h1);
      for (int b = 0; b < nw; ++b) {
        float t[N];
        Num<T>::load(p + ((long)a * g.wout + b) * g.c, t);
        const float wgt = wa * tap_weight(g.rw, wlo + b, g.win, w1);
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] = fmaf(wgt, t[k], acc[k]);
      }
    }
    Num<T>::store(gx + pix * g.c + v * N, acc);
  }
}

inline bool up_ok(int dtype, int layout, int n, int c, int hin, int win, int hout, int wout) {
  if (dtype < 0 || dtype > 2 || layout < 0 || layout > 1 || n <= 0 || c <= 0 || hin <= 0 || win <= 0) return false;
  if (hout < hin || wout < win) return false;                              // up-sampling only
  if ((long)hout > 8L * hin || (long)wout > 8L * win) return false;         // the gather of backward visits (2 s + 1)^2 outputs
  if (layout == 1 && c % (dtype == 0 ? 4 : 8)) return false;
  return (long)n * c * hout * wout < (1L << 40);
}

inline Geom make_geom(int n, int c, int hin, int win, int hout, int wout) {
  Geom g{n, c, hin, win, hout, wout, 0.f, 0.f};
  g.rh = hout > 1 ? (float)(hin - 1) / (float)(hout - 1) : 0.f;
  g.rw = wout > 1 ? (float)(win - 1) / (float)(wout - 1) : 0.f;
  return g;
}

inline int up_blocks(long work) {
  const long b = (work + kUpBlock - 1) / kUpBlock;
  return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

template <typename T>
int up_run(bool bwd, const T* in, T* out, int layout, const Geom& g, hipStream_t st) {
  const long plane = bwd ? (long)g.hin * g.win : (long)g.hout * g.wout;
  if (layout == 0) {
    const int blocks = up_blocks((long)g.n * g.c * plane);
    if (bwd) hipLaunchKernelGGL(up_bwd_nchw<T>, dim3(blocks), dim3(kUpBlock), 0, st, in, out, g);
    else hipLaunchKernelGGL(up_fwd_nchw<T>, dim3(blocks), dim3(kUpBlock), 0, st, in, out, g);
  } else {
    const int blocks = up_blocks((long)g.n * plane * (g.c / Num<T>::N));
    if (bwd) hipLaunchKernelGGL(up_bwd_nhwc<T>, dim3(blocks), dim3(kUpBlock), 0, st, in, out, g);
    else hipLaunchKernelGGL(up_fwd_nhwc<T>, dim3(blocks), dim3(kUpBlock), 0, st, in, out, g);
  }
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

int up_dispatch(bool bwd, const void* in, void* out, int dtype, int layout, int n, int c, int hin, int win, int hout, int wout, void* stream) {
  if (!in || !out) return DHD_EINVAL;
  // channels_last rows move as 16-byte vectors; the NCHW kernels access single elements
  if (!dhd_aligned(layout == 1 ? 16 : (dtype == DHD_F32 ? 4 : 2), in, out)) return DHD_EINVAL;
  if (!up_ok(dtype, layout, n, c, hin, win, hout, wout)) return DHD_EUNSUPPORTED;
  const Geom g = make_geom(n, c, hin, win, hout, wout);
  hipStream_t st = dhd_stream(stream);
  return dhd::with_dtype<dhd::HipHalf>(dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    return up_run<T>(bwd, (const T*)in, (T*)out, layout, g, st);
  });
}

}  // namespace

extern "C" {

int dhd_upsample_bilinear_supported(int dtype, int layout, int n, int c, int hin, int win, int hout, int wout) {
  return up_ok(dtype, layout, n, c, hin, win, hout, wout) ? 1 : 0;
}

int dhd_upsample_bilinear_forward(const void* x, int dtype, int layout, int n, int c, int hin, int win, int hout, int wout, void* y,
                                  void* stream) {
  return up_dispatch(false, x, y, dtype, layout, n, c, hin, win, hout, wout, stream);
}

int dhd_upsample_bilinear_backward(const void* grad_y, int dtype, int layout, int n, int c, int hin, int win, int hout, int wout,
                                   void* grad_x, void* stream) {
  return up_dispatch(true, grad_y, grad_x, dtype, layout, n, c, hin, win, hout, wout, stream);
}

}  // extern "C"

// the seams of the UNets' other decoder form (ConvTranspose2d) and of their encoder: the dhdn_* surface
#include "unet_seam.h"
