// Swin FFN at inference: LayerNorm -> Linear -> GELU -> Linear -> residual add in one kernel (include/dhd_amd_ffn.h).
//
//   out[row] = x[row] + W2 . gelu(W1 . LN(x[row]; gamma, beta, eps) + b1) + b2          exact (erf) GELU, hidden = 4 C
//
// Reference: models/backbones/swin.py:569-592 (SwinBlock: norm2 + FFN with identity) at eval time.  Neither the normalised rows nor
// the two (rows x 4C) hidden tensors exist in memory.
//
// The form is occ_head.hip's.  One wave owns 32 rows from the load of x to the store of out; the waves of a block share nothing.
// Both GEMMs put the WEIGHTS on the MFMA A operand (rows = output units) and the tokens on the B operand (column = lane & 31):
//   * a lane loads the channels 16 ks + 8 h + j (h = lane >> 5, j < 8) of its row for every k-step ks: half a row.  The two
//     halves of a row meet once per LayerNorm sum (lane ^ 32); normalised, rounded (or split) they ARE the B fragments of GEMM-1
//     and stay in registers for all C / 8 hidden tiles,
//   * a 32-unit hidden tile comes out of GEMM-1 with its row on the lane and its units in the 16 registers, which after GELU and
//     the rounding (or split) is the B operand of two k-steps of GEMM-2: element j of lane half h of k-step s is unit
//     8 (2 s + (j >> 2)) + 4 h + (j & 3) of the tile, and W2's k order is permuted to match when it is packed,
//   * W2's rows are permuted so that register 8 s + j of output tile n is channel 32 n + 16 s + 8 h + j: the channels the lane
//     loaded for k-step 2 n + s.  The residual add and the store of out are therefore 16-byte vectors in x's own layout.
// The weights reach a wave as one linear stream of 1 KiB fragments (16 bytes per lane) in the order of their use, prepared in
// `scratch` by pack_stream_kernel once per call and L2-resident after the first waves; a ring of R fragments is loaded ahead of
// the MFMAs that consume them.  Per hidden tile t the stream holds
//   4 fragments     b1 of the tile as float32, register e of fragment f = b1[32 t + 8 f + 4 h + e]
//   C / 16 * P      GEMM-1, k-step ks, part p: W1[32 t + r][16 ks + 8 h + j]
//   C / 16 * P      GEMM-2, k-step s, output tile n, part p: W2[out_ch(r, n)][hid_unit(t, s, h, j)]
// with P = 2 bf16 parts (high, residual) of a float32 weight (mm_dtype float32: three products per step, as sfa / occ_head), or
// P = 1 weight rounded to the half type (one product, float32 accumulation).
//
// Rows are independent: a row lives in one MFMA column (two lanes), nothing is reduced across columns, nothing is atomic.
#include "sfa_mfma.h"

#include "../../include/dhd_amd_ffn.h"

namespace {

using namespace dhd_sfa;

constexpr int kBlock = 256;                 // 4 waves = 128 rows; one wave per SIMD (the kernel needs more than 256 registers)
constexpr int kRowsPerBlock = kBlock / 64 * 32;
constexpr int kPackBlock = 256;
constexpr long kMaxRows = 1L << 37;         // grid.x = rows / 128 stays below 2^31

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

template <class M> constexpr int kParts = std::is_same_v<M, float> ? 2 : 1;

// the largest ring of at most 20 fragments (80 registers) whose length divides the fragments of a hidden tile: static positions
constexpr int ring_size(int n) {
  for (int r = 20; r > 1; --r)
    if (n % r == 0) return r;
  return 1;
}

template <class M, int C> struct Geo {
  static constexpr int P = kParts<M>;
  static constexpr int KS = C / 16;          // k-steps of GEMM-1 = (output tile, k-step) pairs of GEMM-2 per hidden tile
  static constexpr int NT = C / 32;          // output tiles of GEMM-2
  static constexpr int HT = C / 8;           // hidden tiles: 4 C / 32
  static constexpr int N = 4 + 2 * KS * P;   // fragments per hidden tile: 20 / 36 (C = 128), 36 / 68 (C = 256)
  static constexpr int R = ring_size(N);     // 20 / 18, 18 / 17
  static constexpr size_t kStreamBytes = (size_t)HT * N * 1024;
  // The ring runs R fragments ahead of its consumer to the very end, so the last refills read past the last fragment.  Their
  // address is carried in the scalar offset of the buffer load, which the hardware range check does not look at: the bytes must
  // exist.  `scratch` therefore ends with R KiB that are read and never used (nor written: any bit pattern will do).
  static constexpr size_t kScratchBytes = kStreamBytes + (size_t)R * 1024;
};

// channel of MFMA row r of output tile n, and hidden unit of element j of lane half h of k-step s of hidden tile t
__host__ __device__ constexpr int out_ch(int r, int n) { return 32 * n + 16 * (r >> 4) + 8 * ((r >> 2) & 1) + 4 * ((r >> 3) & 1) + (r & 3); }
__host__ __device__ constexpr int hid_unit(int t, int s, int h, int j) { return 32 * t + 8 * (2 * s + (j >> 2)) + 4 * h + (j & 3); }

template <class M> __device__ __forceinline__ f32x16 mfma16(u32x4 a, u32x4 b, f32x16 c) {
  if constexpr (std::is_same_v<M, _Float16>)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return mfma_bf16(a, b, c);
}

// eight consecutive-k values -> the fragment words: part 0 / 1 of the bf16 split of float32, or the values rounded to M
template <class M> __device__ __forceinline__ void make_parts(const float* v, u32x4 (&w)[kParts<M>]) {
#pragma unroll
  for (int jp = 0; jp < 4; ++jp) {
    if constexpr (std::is_same_v<M, float>) {
      unsigned h, m;
      split2_hm(v[2 * jp], v[2 * jp + 1], h, m);
      w[0][jp] = h;
      w[kParts<M> - 1][jp] = m;
    } else {
      w[0][jp] = Pair<M>::narrow(f32x2{v[2 * jp], v[2 * jp + 1]});
    }
  }
}

// one thread per (hidden tile, fragment, lane): 16 bytes of the stream
template <class M, int C>
__global__ __launch_bounds__(kPackBlock) void pack_stream_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                                                 const float* __restrict__ w2, u32x4* __restrict__ stream) {
  using G = Geo<M, C>;
  constexpr int P = G::P, N = G::N, KS = G::KS, NT = G::NT, H = 4 * C;
  const int idx = blockIdx.x * kPackBlock + threadIdx.x;
  if (idx >= G::HT * N * 64) return;
  const int lane = idx & 63, r = lane & 31, h = lane >> 5;
  const int f = (idx >> 6) % N, t = (idx >> 6) / N;
  float v[8];
  u32x4 parts[P];
  u32x4 out;
  if (f < 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = __float_as_uint(b1[32 * t + 8 * f + 4 * h + e]);
  } else if (f < 4 + KS * P) {
    const int ks = (f - 4) / P, part = (f - 4) % P;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w1[(size_t)(32 * t + r) * C + 16 * ks + 8 * h + j];
    make_parts<M>(v, parts);
    out = part ? parts[P - 1] : parts[0];
  } else {
    const int g = f - 4 - KS * P;
    const int part = g % P, n = (g / P) % NT, s = g / (P * NT);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w2[(size_t)out_ch(r, n) * H + hid_unit(t, s, h, j)];
    make_parts<M>(v, parts);
    out = part ? parts[P - 1] : parts[0];
  }
  stream[idx] = out;
}

// GELU(x) = x Phi(x) with the exact (erf) Phi, as max(x, 0) - |x| erfc(|x| / sqrt 2) / 2, branch-free on the hardware rcp and
// exp2: the library erff costs several times the MFMAs it sits between.  erfc(z) = poly(t) exp(-z^2), t = 1 / (1 + p z), is
// Abramowitz & Stegun 7.1.26 (absolute error of erf below 1.5e-7 for every z), so the absolute error of the GELU is below
// 0.75e-7 |x| plus float32 rounding, and in the erfc form it vanishes with the value in the negative tail instead of leaving
// 1 - erf's cancellation there.  |x| is clamped to 14 inside the second term (erfc(9.9) < 2e-44: the term is 0 there) so that
// +inf gives inf and not inf - inf * 0.  A NaN goes through: the first term is a select that keeps it.
__device__ __forceinline__ float gelu_erf(float x) {
  constexpr float kRsqrt2 = 0.707106769084930419921875f, kLog2e = 1.44269502162933349609375f;
  const float ax = fminf(fabsf(x), 14.f);
  const float z = ax * kRsqrt2;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.f));
  const float poly = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
  const float e = __builtin_amdgcn_exp2f(-(z * z) * kLog2e);
  return (x < 0.f ? 0.f : x) - (0.5f * ax) * (poly * e);
}

// The 8 channels 16 ks + 8 h + j of a row as they lie in memory: 2 vectors of float32, 1 of a half type.
template <class X> constexpr int kRawVecs = 8 * sizeof(X) / 16;

template <class X> __device__ __forceinline__ void load_raw(const X* row, int ks, u32x4 (&raw)[kRawVecs<X>]) {
  const u32x4* q = reinterpret_cast<const u32x4*>(row + 16 * ks);
#pragma unroll
  for (int w = 0; w < kRawVecs<X>; ++w) raw[w] = q[w];
}

template <class X> __device__ __forceinline__ void widen8(const u32x4 (&raw)[kRawVecs<X>], float* v) {
  if constexpr (std::is_same_v<X, float>) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = __uint_as_float(raw[j >> 2][j & 3]);
  } else {
#pragma unroll
    for (int jp = 0; jp < 4; ++jp) {
      const f32x2 p = Pair<X>::widen(raw[0][jp]);
      v[2 * jp] = p.x;
      v[2 * jp + 1] = p.y;
    }
  }
}

__device__ __forceinline__ float sum8(const float* s) { return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7])); }

// KEEP: the row's own bytes stay in registers from the first load to the residual add; otherwise the epilogue loads them again
// (the one combination whose registers do not hold them: C = 256 with the two-part float32 operands).
// S: what multiplies the branch before the residual add.  NoScale (inference: nothing, and nothing is compiled for it) or the
// per-image factor of the training forward (swin_ffn_train.h).
struct NoScale {
  static constexpr bool kOn = false;
};

template <class X, class M, int C, bool KEEP, class S>
__global__ __launch_bounds__(kBlock) void swin_ffn_kernel(const X* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const u32x4* __restrict__ stream,
                                                          const float* __restrict__ b2, X* __restrict__ out, long rows, float eps,
                                                          S scale) {
  using G = Geo<M, C>;
  constexpr int P = G::P, N = G::N, R = G::R, KS = G::KS, NT = G::NT, HT = G::HT, RW = kRawVecs<X>;
  static_assert(N % R == 0, "the ring position of a fragment must not depend on the hidden tile");
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const long p0 = ((long)blockIdx.x * (kBlock / 64) + (tid >> 6)) * 32;   // wave-uniform
  if (p0 >= rows) return;
  const bool live = p0 + r < rows;   // a lane past the last row computes on the last row and stores nothing
  const long p = live ? p0 + r : rows - 1;
  float f = 1.f;
  if constexpr (S::kOn) f = scale.factor[p / scale.rows_per_image];   // the row's image; applied in float32 in the epilogue
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(stream), 0, (unsigned)G::kScratchBytes, 0x00020000);
  // the ring: fragment i of tile t sits in ring[i % R]; its slot is refilled with fragment i + R as soon as it is consumed
  // (the refills of the last fragments read the padding behind the stream, see kScratchBytes)
  u32x4 ring[R];
  const int lane_off = lane * 16;
  static_for<R>([&](auto i) { ring[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, i * 1024, 0); });

  const X* xrow = x + (size_t)p * C + 8 * h;
  u32x4 raw[KS][RW];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) load_raw<X>(xrow, ks, raw[ks]);

  // LayerNorm statistics in float32: mean, then the centred sum of squares (a second pass over registers); each sum is eight
  // strided partial sums, a fixed tree over them and the other half of the row (lane ^ 32)
  float mean = 0.f, rstd = 1.f;
  const bool ln = gamma != nullptr;   // uniform over the launch
  if (ln) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      float v[8];
      widen8<X>(raw[ks], v);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += v[j];
    }
    float tot = sum8(s);
    tot += __shfl_xor(tot, 32, DHD_WAVE);
    mean = tot * (1.f / C);
    // the centred pass also sums the residuals and corrects the mean by their average: the rounding of the float32 sum, some
    // 2^-24 |mean|, is otherwise multiplied by rstd (316 on a constant row, whose exact xn is beta)
    float q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, e[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      float v[8];
      widen8<X>(raw[ks], v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = v[j] - mean;
        e[j] += d;
        q[j] = fmaf(d, d, q[j]);
      }
    }
    float var = sum8(q), de = sum8(e);
    var += __shfl_xor(var, 32, DHD_WAVE);
    de += __shfl_xor(de, 32, DHD_WAVE);
    de *= 1.f / C;
    mean += de;
    rstd = 1.f / sqrtf(fmaxf(var * (1.f / C) - de * de, 0.f) + eps);
  }

  // the B fragments of GEMM-1: xf[ks][part] = normalised elements 16 ks + 8 h + j of the row
  u32x4 xf[KS][P];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    if (!ln && std::is_same_v<X, M> && !std::is_same_v<X, float>) {
      xf[ks][0] = raw[ks][0];   // a half row that the half GEMM reads as it lies
    } else {
      float v[8];
      widen8<X>(raw[ks], v);
      if (ln) {
        const f32x4* gp = reinterpret_cast<const f32x4*>(gamma + 16 * ks + 8 * h);
        const f32x4* bp = reinterpret_cast<const f32x4*>(beta + 16 * ks + 8 * h);
        const f32x4 g0 = gp[0], g1 = gp[1], c0 = bp[0], c1 = bp[1];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ((v[j] - mean) * rstd) * (j < 4 ? g0[j & 3] : g1[j & 3]) + (j < 4 ? c0[j & 3] : c1[j & 3]);
      }
      make_parts<M>(v, xf[ks]);   // rounded once to the type fc1 reads, as nn.LayerNorm + autocast (or a half model) do
    }
  }

  f32x16 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[n][e] = 0.f;

  for (int t = 0; t < HT; ++t) {
    const int base = t * (N * 1024);
    // take fragment I out of the ring and refill its slot
    auto take = [&](auto I) {
      constexpr int i = decltype(I)::value;
      const u32x4 v = ring[i % R];
      ring[i % R] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, base + (i + R) * 1024, 0);
      // The refill stays HERE: left alone, the scheduler sinks every load to just above its use to save registers, and the
      // wave then sits out one L2 round trip per fragment.
      __builtin_amdgcn_sched_barrier(0);
      return v;
    };
    // hidden tile, starting from its bias
    f32x16 hid;
    static_for<4>([&](auto F) {
      const u32x4 v = take(F);
#pragma unroll
      for (int e = 0; e < 4; ++e) hid[4 * F + e] = __uint_as_float(v[e]);
    });
    static_for<KS>([&](auto KSI) {
      constexpr int ks = decltype(KSI)::value;
      if constexpr (P == 2) {
        const u32x4 wh = take(std::integral_constant<int, 4 + 2 * ks>{});
        const u32x4 wm = take(std::integral_constant<int, 4 + 2 * ks + 1>{});
        hid = mfma16<M>(wm, xf[ks][0], hid);   // smallest terms first
        hid = mfma16<M>(wh, xf[ks][P - 1], hid);
        hid = mfma16<M>(wh, xf[ks][0], hid);
      } else {
        hid = mfma16<M>(take(std::integral_constant<int, 4 + ks>{}), xf[ks][0], hid);
      }
    });
    // GELU in float32, then the operand parts of the two k-steps of GEMM-2
    u32x4 hf[2][P];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float a[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = gelu_erf(hid[8 * s + j]);
      make_parts<M>(a, hf[s]);
    }
    static_for<2 * NT>([&](auto GI) {
      constexpr int g = decltype(GI)::value, s = g / NT, n = g % NT, i0 = 4 + KS * P + g * P;
      if constexpr (P == 2) {
        const u32x4 wh = take(std::integral_constant<int, i0>{});
        const u32x4 wm = take(std::integral_constant<int, i0 + 1>{});
        acc[n] = mfma16<M>(wm, hf[s][0], acc[n]);
        acc[n] = mfma16<M>(wh, hf[s][P - 1], acc[n]);
        acc[n] = mfma16<M>(wh, hf[s][0], acc[n]);
      } else {
        acc[n] = mfma16<M>(take(std::integral_constant<int, i0>{}), hf[s][0], acc[n]);
      }
    });
  }

  // register 8 s + j of tile n = channel 16 (2 n + s) + 8 h + j of this lane's row: x's own layout
  X* orow = out + (size_t)p * C + 8 * h;
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int ks = 2 * n + s;
      float xv[8], o[8];
      if constexpr (KEEP) {
        widen8<X>(raw[ks], xv);
      } else {
        u32x4 again[RW];
        load_raw<X>(xrow, ks, again);
        widen8<X>(again, xv);
      }
      const f32x4* bp = reinterpret_cast<const f32x4*>(b2 + 16 * ks + 8 * h);
      const f32x4 c0 = bp[0], c1 = bp[1];
      if constexpr (S::kOn) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = xv[j] + f * (acc[n][8 * s + j] + (j < 4 ? c0[j & 3] : c1[j & 3]));
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = xv[j] + (acc[n][8 * s + j] + (j < 4 ? c0[j & 3] : c1[j & 3]));
      }
      if (live) {
        raw16<X>* q = reinterpret_cast<raw16<X>*>(orow + 16 * ks);
#pragma unroll
        for (int w = 0; w < RW; ++w) q[w] = narrow16<X>(o + w * kVec16<X>);
      }
    }
}

bool shape_supported(int c, int hidden) { return (c == 128 || c == 256) && hidden == 4 * c; }

bool dtype_code(int d) { return d == DHD_F32 || d == DHD_F16 || d == DHD_BF16; }

// the residual stream in float32 with any GEMM type (a block under autocast), or a half model in its own type
bool precision_supported(int x_dtype, int mm_dtype) {
  return dtype_code(x_dtype) && dtype_code(mm_dtype) && (x_dtype == DHD_F32 || x_dtype == mm_dtype);
}

size_t scratch_bytes(int c, int mm_dtype) {
  if (c == 128) return mm_dtype == DHD_F32 ? Geo<float, 128>::kScratchBytes : Geo<__bf16, 128>::kScratchBytes;
  return mm_dtype == DHD_F32 ? Geo<float, 256>::kScratchBytes : Geo<__bf16, 256>::kScratchBytes;
}

template <class X, class M, int C, class S = NoScale>
int launch(const void* x, const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2, const float* b2,
           void* out, void* scratch, long rows, float eps, hipStream_t st, S scale = S{}) {
  using G = Geo<M, C>;
  constexpr bool keep = !(C == 256 && std::is_same_v<M, float>);
  u32x4* stream = static_cast<u32x4*>(scratch);
  constexpr int n_pack = G::HT * G::N * 64;
  hipLaunchKernelGGL((pack_stream_kernel<M, C>), dim3(dhd_cdiv(n_pack, kPackBlock)), dim3(kPackBlock), 0, st, w1, b1, w2, stream);
  DHD_LAUNCH_CHECK();
  hipLaunchKernelGGL((swin_ffn_kernel<X, M, C, keep, S>), dim3(dhd_cdiv(rows, kRowsPerBlock)), dim3(kBlock), 0, st,
                     static_cast<const X*>(x), gamma, beta, stream, b2, static_cast<X*>(out), rows, eps, scale);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

}  // namespace

extern "C" {

int dhdf_swin_ffn_supported(int c, int hidden, int x_dtype, int mm_dtype) {
  return shape_supported(c, hidden) && precision_supported(x_dtype, mm_dtype) ? 1 : 0;
}

size_t dhdf_swin_ffn_scratch_bytes(int c, int hidden, int mm_dtype) {
  if (!shape_supported(c, hidden) || !dtype_code(mm_dtype)) return 0;
  return scratch_bytes(c, mm_dtype);
}

int dhdf_swin_ffn_infer(const void* x, const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2,
                        const float* b2, void* out, void* scratch, size_t scratch_size, int x_dtype, int mm_dtype, long rows, int c,
                        int hidden, float eps, void* stream) {
  if (!x || !w1 || !b1 || !w2 || !b2 || !out || !scratch || rows <= 0) return DHD_EINVAL;
  if ((gamma == nullptr) != (beta == nullptr)) return DHD_EINVAL;   // the LayerNorm is there or it is not
  if (!dhd_aligned(16, x, gamma, beta, w1, b1, w2, b2, out, scratch)) return DHD_EINVAL;
  if (!dhdf_swin_ffn_supported(c, hidden, x_dtype, mm_dtype) || rows > kMaxRows) return DHD_EUNSUPPORTED;
  if (scratch_size < scratch_bytes(c, mm_dtype)) return DHD_ENOSPACE;
  hipStream_t st = dhd_stream(stream);
  return dhd::with_dtype<dhd::NativeHalf>(x_dtype, [&](auto* xp) {
    using X = std::remove_pointer_t<decltype(xp)>;
    return dhd::with_dtype<dhd::NativeHalf>(mm_dtype, [&](auto* mp) {
      using M = std::remove_pointer_t<decltype(mp)>;
      if constexpr (std::is_same_v<X, float> || std::is_same_v<X, M>) {
        return c == 128 ? launch<X, M, 128>(x, gamma, beta, w1, b1, w2, b2, out, scratch, rows, eps, st)
                        : launch<X, M, 256>(x, gamma, beta, w1, b1, w2, b2, out, scratch, rows, eps, st);
      } else {
        return (int)DHD_EUNSUPPORTED;
      }
    });
  });
}

}  // extern "C"

// the kernel family for C = 512 and 1024 and its dhdg_* entry points, on the helpers above
#include "swin_ffn_wide.h"

// the training pair for C = 128 and 256 (forward with a per-image factor, recompute backward) and its dhdt_* entry points
#include "swin_ffn_train.h"

// the training pair for C = 512 in the wide family's form and its dhdu_* entry points, on both of the above
#include "swin_ffn_wide_train.h"
