// Swin FFN at inference for C = 512 and 1024 (include/dhd_amd_ffn_wide.h): the same formula, rounding points and GELU as
// swin_ffn.hip, which includes this file after its own helpers (gelu_erf, make_parts, mfma16, load_raw, widen8, ring_size and the
// dtype predicates are used as they are), in a form whose weights are shared by a whole workgroup.
//
// Why a second form: in the one-wave-per-32-rows kernel a lane holds C / 2 accumulators and (C / 4) P operand registers, which is
// the whole register file at C = 512 with P = 2 and more than it at C = 1024, and every wave streams every weight byte.  Here
//   * a workgroup of 4 waves owns T rows: with one half part 96 at C = 512 and 64 at C = 1024 (the most whose tile and chunk
//     buffers fit the 160 KiB LDS: the weight stream is rows / T x packed bytes out of L2 / Infinity Cache, and at 64 rows
//     C = 512 measured 10 % slower), 32 with the two bf16 parts of float32.  Each wave normalises
//     T / 4 of them (one row at a time over the 64 lanes, float32 statistics by a fixed xor butterfly) and writes the operand
//     parts into an LDS tile [part][row][C] whose rows are padded by 16 bytes: lane (r, h) reads the 16 bytes of row r at
//     k = 16 ks + 8 h with ds_read_b128, bank 4 r + const (mod 64), which is conflict-free in each of the instruction's four
//     16-lane groups,
//   * the hidden dimension is walked in chunks of HC units (128; 256 at C = 512 in float32).  GEMM-1: wave w computes the unit
//     tiles [UTW w, UTW (w + 1)) of the chunk (UTW = HC / 128) for all T rows, W1 fragments on the MFMA A operand, the tile on
//     B.  Bias is the initial accumulator; GELU and the one rounding follow in float32, and the chunk goes to an LDS buffer
//     [part][row][HC] (rows padded by 16 bytes as well), double-buffered where the LDS allows it (C = 512: one barrier per
//     chunk), single at C = 1024 (two barriers),
//   * GEMM-2: wave w owns the output channels [w C / 4, (w + 1) C / 4): C / 128 tiles x T / 32 row tiles of accumulators, W2
//     fragments of its channel slice on A, the hidden chunk from LDS on B.  W2's rows are permuted inside a 32-channel tile by
//     out_ch (as the narrow kernel) so that a lane ends with 8 consecutive channels of its row per register octet: the residual
//     add and the store are 16-byte vectors in x's own layout.  x is read a second time for that add.
// So a weight byte is fetched once per workgroup.  Each wave reads its own linear stream of 1 KiB fragments, laid out by
// pack_wide_kernel as [wave][chunk][fragment] in the order of use, through the same ring of R fragments as the narrow kernel:
//   4 UTW           b1 of the wave's unit tiles, register e of fragment 4 ut + f = b1[unit0 + 32 ut + 8 f + 4 h + e]
//   KS UTW P        GEMM-1, k-step ks, unit tile ut, part p: W1[unit0 + 32 ut + r][16 ks + 8 h + j]
//   HC / 16 MT P    GEMM-2, k-step s, channel tile m, part p: W2[out_ch(r, MT w + m)][HC chunk + 16 s + 8 h + j]
// The ring reads R fragments past the end of a wave's stream: the next wave's, or for the last wave R KiB of padding that scratch
// includes.  Rows are independent (a row is one MFMA column and one LayerNorm pass), nothing is atomic.
#pragma once

#include "../../include/dhd_amd_ffn_wide.h"

namespace {

constexpr int kWideWaves = 4;
constexpr int kWideBlock = 64 * kWideWaves;
constexpr long kWideMaxRows = 1L << 36;     // grid.x = rows / 32 stays below 2^31

template <class M, int C> struct WGeo {
  static constexpr int P = kParts<M>;
  static constexpr int T = P == 2 ? 32 : C == 512 ? 96 : 64;     // rows of a workgroup
  static constexpr int HC = C == 512 && P == 2 ? 256 : 128;      // hidden units of a chunk
  static constexpr int NBUF = C == 512 ? 2 : 1;     // hidden chunk buffers in LDS
  static constexpr int UTW = HC / (32 * kWideWaves);// unit tiles of a wave per chunk
  static constexpr int RT = T / 32;                 // row tiles
  static constexpr int MT = C / (32 * kWideWaves);  // channel tiles of a wave
  static constexpr int KS = C / 16;                 // k-steps of GEMM-1
  static constexpr int HS = HC / 16;                // k-steps of GEMM-2 per chunk
  static constexpr int NCH = 4 * C / HC;            // chunks
  static constexpr int NB = 4 * UTW;                // bias fragments
  static constexpr int N1 = KS * UTW * P;
  static constexpr int N = NB + N1 + HS * MT * P;   // fragments per (wave, chunk): 68 / 264 (C = 512), 132 / 260 (C = 1024)
  static constexpr int R = ring_size(N);            // 17 / 12, 12 / 20
  static constexpr int XS = 2 * C + 16;             // bytes of a tile row
  static constexpr int HB = 2 * HC + 16;            // bytes of a hidden-chunk row
  static constexpr int kTileBytes = P * T * XS;
  static constexpr int kHidBytes = P * T * HB;      // one buffer
  static constexpr int kLdsBytes = kTileBytes + NBUF * kHidBytes;   // 152 064 / 134 144 (C = 512), 149 504 (C = 1024)
  static constexpr size_t kWaveBytes = (size_t)NCH * N * 1024;
  static constexpr size_t kStreamBytes = kWideWaves * kWaveBytes;
  static constexpr size_t kScratchBytes = kStreamBytes + (size_t)R * 1024;   // the last wave's read-ahead (read, never used)
  static_assert(N % R == 0 && kLdsBytes <= 160 * 1024 && kScratchBytes < (1u << 31), "geometry");
};

// four consecutive-k values -> two fragment words per part
template <class M> __device__ __forceinline__ void make_parts4(const float* v, u32x2 (&w)[kParts<M>]) {
#pragma unroll
  for (int jp = 0; jp < 2; ++jp) {
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

// one thread per (wave, chunk, fragment, lane): 16 bytes of the stream
template <class M, int C>
__global__ __launch_bounds__(kPackBlock) void pack_wide_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                                               const float* __restrict__ w2, u32x4* __restrict__ stream) {
  using G = WGeo<M, C>;
  constexpr int P = G::P, N = G::N, UTW = G::UTW, MT = G::MT, H = 4 * C;
  const int idx = blockIdx.x * kPackBlock + threadIdx.x;
  if (idx >= kWideWaves * G::NCH * N * 64) return;
  const int lane = idx & 63, r = lane & 31, h = lane >> 5;
  const int q = idx >> 6, f = q % N, t = (q / N) % G::NCH, w = q / (N * G::NCH);
  const int unit0 = G::HC * t + 32 * UTW * w;
  float v[8];
  u32x4 parts[P];
  u32x4 out;
  if (f < G::NB) {
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = __float_as_uint(b1[unit0 + 32 * (f >> 2) + 8 * (f & 3) + 4 * h + e]);
  } else if (f < G::NB + G::N1) {
    const int g = f - G::NB, part = g % P, ut = (g / P) % UTW, ks = g / (P * UTW);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w1[(size_t)(unit0 + 32 * ut + r) * C + 16 * ks + 8 * h + j];
    make_parts<M>(v, parts);
    out = part ? parts[P - 1] : parts[0];
  } else {
    const int g = f - G::NB - G::N1, part = g % P, m = (g / P) % MT, s = g / (P * MT);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w2[(size_t)out_ch(r, MT * w + m) * H + G::HC * t + 16 * s + 8 * h + j];
    make_parts<M>(v, parts);
    out = part ? parts[P - 1] : parts[0];
  }
  stream[idx] = out;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, DHD_WAVE);
  return v;
}

template <class M> __device__ __forceinline__ f32x16 mfma_parts(const u32x4 (&w)[kParts<M>], const u32x4 (&b)[kParts<M>], f32x16 c) {
  constexpr int P = kParts<M>;
  if constexpr (P == 2) {
    c = mfma16<M>(w[P - 1], b[0], c);   // smallest terms first
    c = mfma16<M>(w[0], b[P - 1], c);
  }
  return mfma16<M>(w[0], b[0], c);
}

// S: what multiplies the branch before the residual add, as in swin_ffn_kernel: NoScale (inference: nothing, and nothing is
// compiled for it) or the per-image factor of the training forward (swin_ffn_wide_train.h).
template <class X, class M, int C, class S = NoScale>
__global__ __launch_bounds__(kWideBlock) void swin_ffn_wide_kernel(const X* __restrict__ x, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, const u32x4* __restrict__ stream,
                                                                   const float* __restrict__ b2, X* __restrict__ out, long rows,
                                                                   float eps, S scale) {
  using G = WGeo<M, C>;
  constexpr int P = G::P, T = G::T, N = G::N, R = G::R, KS = G::KS, HS = G::HS, UTW = G::UTW, RT = G::RT, MT = G::MT, RW = kRawVecs<X>;
  constexpr int NV = C / 512;   // 8-channel vectors of a row per lane in the LayerNorm pass
  __shared__ __attribute__((aligned(16))) unsigned char lds[G::kLdsBytes];
  unsigned char* const tile = lds;
  unsigned char* const hidb = lds + G::kTileBytes;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long p0 = (long)blockIdx.x * T;   // < rows: the grid is cdiv(rows, T)
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(stream)) + w * G::kWaveBytes, 0,
      (unsigned)(G::kScratchBytes - w * G::kWaveBytes), 0x00020000);
  u32x4 ring[R];
  const int lane_off = lane * 16;
  static_for<R>([&](auto i) { ring[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, i * 1024, 0); });

  // ---- LayerNorm: wave w normalises the rows [w T / 4, (w + 1) T / 4) of the tile, a row past the last one as the last one
  {
    const bool ln = gamma != nullptr;   // uniform over the launch
    float gv[NV][8], bv[NV][8];
    if (ln) {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const f32x4* gp = reinterpret_cast<const f32x4*>(gamma + 512 * k + 8 * lane);
        const f32x4* bp = reinterpret_cast<const f32x4*>(beta + 512 * k + 8 * lane);
        const f32x4 g0 = gp[0], g1 = gp[1], c0 = bp[0], c1 = bp[1];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          gv[k][j] = j < 4 ? g0[j & 3] : g1[j & 3];
          bv[k][j] = j < 4 ? c0[j & 3] : c1[j & 3];
        }
      }
    }
#pragma unroll 2
    for (int i = 0; i < T / kWideWaves; ++i) {
      const int rl = w * (T / kWideWaves) + i;
      const long p = p0 + rl < rows ? p0 + rl : rows - 1;
      const X* xrow = x + (size_t)p * C + 8 * lane;
      float v[NV][8];
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        u32x4 raw[RW];
        load_raw<X>(xrow, 32 * k, raw);   // channels 512 k + 8 lane + j
        widen8<X>(raw, v[k]);
      }
      if (ln) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) s += sum8(v[k]);
        float mean = wave_sum(s) * (1.f / C);
        // the centred pass also sums the residuals and corrects the mean by their average (swin_ffn.hip says why)
        float q = 0.f, e = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          float d[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) d[j] = v[k][j] - mean;
          e += sum8(d);
#pragma unroll
          for (int j = 0; j < 8; ++j) d[j] *= d[j];
          q += sum8(d);
        }
        const float de = wave_sum(e) * (1.f / C);
        mean += de;
        const float rstd = 1.f / sqrtf(fmaxf(wave_sum(q) * (1.f / C) - de * de, 0.f) + eps);
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
          for (int j = 0; j < 8; ++j) v[k][j] = ((v[k][j] - mean) * rstd) * gv[k][j] + bv[k][j];
      }
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        u32x4 parts[P];
        make_parts<M>(v[k], parts);   // rounded once to the type fc1 reads
#pragma unroll
        for (int part = 0; part < P; ++part)
          *reinterpret_cast<u32x4*>(tile + (part * T + rl) * G::XS + (512 * k + 8 * lane) * 2) = parts[part];
      }
    }
  }
  __syncthreads();

  f32x16 acc[MT][RT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][rt][e] = 0.f;

  // this lane's B-operand addresses: row r of row tile 0, k = 8 h
  const unsigned char* const xb = tile + r * G::XS + 16 * h;
  const int hrow = r * G::HB;

  for (int t = 0; t < G::NCH; ++t) {
    const int base = t * (N * 1024);
    auto take = [&](auto I) {   // fragment I of the chunk out of the ring, its slot refilled (see swin_ffn_kernel)
      constexpr int i = decltype(I)::value;
      const u32x4 v = ring[i % R];
      ring[i % R] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, base + (i + R) * 1024, 0);
      __builtin_amdgcn_sched_barrier(0);
      return v;
    };
    unsigned char* const hb = hidb + (G::NBUF == 2 ? (t & 1) * G::kHidBytes : 0);

    // ---- GEMM-1: the wave's unit tiles x all rows, starting from the bias
    f32x16 hid[UTW][RT];
    static_for<G::NB>([&](auto F) {
      constexpr int f = decltype(F)::value;
      const u32x4 v = take(F);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int e = 0; e < 4; ++e) hid[f >> 2][rt][4 * (f & 3) + e] = __uint_as_float(v[e]);
    });
    u32x4 bx[2][RT][P];
    auto load_x = [&](auto KSI, u32x4 (&b)[RT][P]) {
      constexpr int ks = decltype(KSI)::value;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int part = 0; part < P; ++part)
          b[rt][part] = *reinterpret_cast<const u32x4*>(xb + (part * T + 32 * rt) * G::XS + 32 * ks);
    };
    load_x(std::integral_constant<int, 0>{}, bx[0]);
    static_for<KS>([&](auto KSI) {
      constexpr int ks = decltype(KSI)::value;
      if constexpr (ks + 1 < KS) load_x(std::integral_constant<int, ks + 1>{}, bx[(ks + 1) & 1]);   // one k-step ahead of its use
      static_for<UTW>([&](auto UT) {
        constexpr int ut = decltype(UT)::value, i0 = G::NB + (ks * UTW + ut) * P;
        u32x4 wf[P];
        wf[0] = take(std::integral_constant<int, i0>{});
        if constexpr (P == 2) wf[P - 1] = take(std::integral_constant<int, i0 + P - 1>{});
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) hid[ut][rt] = mfma_parts<M>(wf, bx[ks & 1][rt], hid[ut][rt]);
      });
    });

    // ---- GELU in float32, rounded once, into the chunk buffer: register 4 f + e is unit 8 f + 4 h + e of the tile
#pragma unroll
    for (int ut = 0; ut < UTW; ++ut)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          float a[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) a[e] = gelu_erf(hid[ut][rt][4 * f + e]);
          u32x2 hp[P];
          make_parts4<M>(a, hp);
#pragma unroll
          for (int part = 0; part < P; ++part)
            *reinterpret_cast<u32x2*>(hb + (part * T + 32 * rt) * G::HB + hrow + (32 * (UTW * w + ut) + 8 * f + 4 * h) * 2) = hp[part];
        }
    __syncthreads();

    // ---- GEMM-2: the wave's channel slice x all rows over the chunk's units
    u32x4 bh[2][RT][P];
    auto load_h = [&](auto SI, u32x4 (&b)[RT][P]) {
      constexpr int s = decltype(SI)::value;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int part = 0; part < P; ++part)
          b[rt][part] = *reinterpret_cast<const u32x4*>(hb + (part * T + 32 * rt) * G::HB + hrow + 16 * h + 32 * s);
    };
    load_h(std::integral_constant<int, 0>{}, bh[0]);
    static_for<HS>([&](auto SI) {
      constexpr int s = decltype(SI)::value;
      if constexpr (s + 1 < HS) load_h(std::integral_constant<int, s + 1>{}, bh[(s + 1) & 1]);
      static_for<MT>([&](auto MI) {
        constexpr int m = decltype(MI)::value, i0 = G::NB + G::N1 + (s * MT + m) * P;
        u32x4 wf[P];
        wf[0] = take(std::integral_constant<int, i0>{});
        if constexpr (P == 2) wf[P - 1] = take(std::integral_constant<int, i0 + P - 1>{});
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[m][rt] = mfma_parts<M>(wf, bh[s & 1][rt], acc[m][rt]);
      });
    });
    if constexpr (G::NBUF == 1) __syncthreads();   // the one buffer is read out before the next chunk overwrites it
  }

  // ---- b2 and the residual add: register 8 s + j of tile (m, rt) = channel 32 (MT w + m) + 16 s + 8 h + j of row 32 rt + r
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const bool live = p0 + 32 * rt + r < rows;   // a lane past the last row computed on the last row and stores nothing
    const long p = live ? p0 + 32 * rt + r : rows - 1;
    const X* xrow = x + (size_t)p * C + 8 * h;
    X* orow = out + (size_t)p * C + 8 * h;
    float f = 1.f;
    if constexpr (S::kOn) f = scale.factor[p / scale.rows_per_image];   // the row's image; applied in float32
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int ks = 2 * (MT * w + m) + s;
        u32x4 raw[RW];
        float xv[8], o[8];
        load_raw<X>(xrow, ks, raw);
        widen8<X>(raw, xv);
        const f32x4* bp = reinterpret_cast<const f32x4*>(b2 + 16 * ks + 8 * h);
        const f32x4 c0 = bp[0], c1 = bp[1];
        if constexpr (S::kOn) {
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = xv[j] + f * (acc[m][rt][8 * s + j] + (j < 4 ? c0[j & 3] : c1[j & 3]));
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = xv[j] + (acc[m][rt][8 * s + j] + (j < 4 ? c0[j & 3] : c1[j & 3]));
        }
        if (live) {
          raw16<X>* q = reinterpret_cast<raw16<X>*>(orow + 16 * ks);
#pragma unroll
          for (int v = 0; v < RW; ++v) q[v] = narrow16<X>(o + v * kVec16<X>);
        }
      }
  }
}

bool wide_shape_supported(int c, int hidden) { return (c == 512 || c == 1024) && hidden == 4 * c; }

size_t wide_scratch_bytes(int c, int mm_dtype) {
  if (c == 512) return mm_dtype == DHD_F32 ? WGeo<float, 512>::kScratchBytes : WGeo<__bf16, 512>::kScratchBytes;
  return mm_dtype == DHD_F32 ? WGeo<float, 1024>::kScratchBytes : WGeo<__bf16, 1024>::kScratchBytes;
}

template <class X, class M, int C, class S = NoScale>
int wide_launch(const void* x, const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2,
                const float* b2, void* out, void* scratch, long rows, float eps, hipStream_t st, S scale = S{}) {
  using G = WGeo<M, C>;
  u32x4* stream = static_cast<u32x4*>(scratch);
  constexpr int n_pack = kWideWaves * G::NCH * G::N * 64;
  hipLaunchKernelGGL((pack_wide_kernel<M, C>), dim3(dhd_cdiv(n_pack, kPackBlock)), dim3(kPackBlock), 0, st, w1, b1, w2, stream);
  DHD_LAUNCH_CHECK();
  hipLaunchKernelGGL((swin_ffn_wide_kernel<X, M, C, S>), dim3(dhd_cdiv(rows, (long)G::T)), dim3(kWideBlock), 0, st,
                     static_cast<const X*>(x), gamma, beta, stream, b2, static_cast<X*>(out), rows, eps, scale);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

}  // namespace

extern "C" {

int dhdg_swin_ffn_wide_supported(int c, int hidden, int x_dtype, int mm_dtype) {
  return wide_shape_supported(c, hidden) && precision_supported(x_dtype, mm_dtype) ? 1 : 0;
}

size_t dhdg_swin_ffn_wide_scratch_bytes(int c, int hidden, int mm_dtype) {
  if (!wide_shape_supported(c, hidden) || !dtype_code(mm_dtype)) return 0;
  return wide_scratch_bytes(c, mm_dtype);
}

int dhdg_swin_ffn_wide_infer(const void* x, const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2,
                             const float* b2, void* out, void* scratch, size_t scratch_size, int x_dtype, int mm_dtype, long rows,
                             int c, int hidden, float eps, void* stream) {
  if (!x || !w1 || !b1 || !w2 || !b2 || !out || !scratch || rows <= 0) return DHD_EINVAL;
  if ((gamma == nullptr) != (beta == nullptr)) return DHD_EINVAL;   // the LayerNorm is there or it is not
  if (!dhd_aligned(16, x, gamma, beta, w1, b1, w2, b2, out, scratch)) return DHD_EINVAL;
  if (!dhdg_swin_ffn_wide_supported(c, hidden, x_dtype, mm_dtype) || rows > kWideMaxRows) return DHD_EUNSUPPORTED;
  if (scratch_size < wide_scratch_bytes(c, mm_dtype)) return DHD_ENOSPACE;
  hipStream_t st = dhd_stream(stream);
  return dhd::with_dtype<dhd::NativeHalf>(x_dtype, [&](auto* xp) {
    using X = std::remove_pointer_t<decltype(xp)>;
    return dhd::with_dtype<dhd::NativeHalf>(mm_dtype, [&](auto* mp) {
      using M = std::remove_pointer_t<decltype(mp)>;
      if constexpr (std::is_same_v<X, float> || std::is_same_v<X, M>) {
        return c == 512 ? wide_launch<X, M, 512>(x, gamma, beta, w1, b1, w2, b2, out, scratch, rows, eps, st)
                        : wide_launch<X, M, 1024>(x, gamma, beta, w1, b1, w2, b2, out, scratch, rows, eps, st);
      } else {
        return (int)DHD_EUNSUPPORTED;
      }
    });
  });
}

}  // extern "C"
