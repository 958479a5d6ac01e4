// Swin FFN in training for C = 128 and 256 (include/dhd_amd_ffn_train.h): the forward of swin_ffn.hip with a per-image factor on
// the branch (DropPath), and a backward that recomputes the hidden tile instead of reading a saved one.  swin_ffn.hip includes this
// file after its own helpers: Geo's constants, make_parts, mfma16, out_ch, hid_unit, ring_size, load_raw / widen8, sum8 and the
// dtype predicates are used as they are, and the forward IS swin_ffn_kernel with the per-image factor as its S.
//
//   out = x + s[row / rows_per_image] (W2 . gelu(W1 . xn + b1) + b2),   xn = LN(x; gamma, beta, eps)
//
// Backward, for g = dout and gs = s g.  The form is the forward's: one wave owns 32 rows from the loads to the store of dx, the
// weights are on the MFMA A operand and the tokens on B (column = lane & 31), nothing goes through LDS between the GEMMs.  A lane
// holds the channels 16 ks + 8 h + j of its row; xn and gs, each rounded once to the GEMM type M (or split in two bf16 parts for
// float32), are B fragments as they lie.  Per hidden tile t of 32 units:
//   h_t  = W1_t . xn + b1                    the forward's GEMM-1
//   da_t = W2[:, t]^T . gs                   A rows are the units 32 t + r, k runs over the channels 16 ks + 8 h + j: the result has
//                                            h_t's register layout (register e = unit 8 (e >> 2) + 4 h + (e & 3) of the tile)
//   a_t = gelu(h_t), dh_t = da_t gelu'(h_t)  float32, in registers; gelu'(x) = Phi(x) + x phi(x) from the terms of gelu_erf
//   dxn += W1[t, :]^T . dh_t                 A rows are out_ch(r, n), k is hid_unit(t, s, h, j): dxn lands in x's own layout, as
//                                            the forward's GEMM-2 output does
// The weight stream (pack_train_kernel, once per call, nothing cached) holds per hidden tile
//   4 fragments     b1 of the tile as float32, register e of fragment f = b1[32 t + 8 f + 4 h + e]
//   C / 16 * P      h:   k-step ks, part p: W1[32 t + r][16 ks + 8 h + j]
//   C / 16 * P      da:  k-step ks, part p: W2[16 ks + 8 h + j][32 t + r]
//   C / 16 * P      dxn: k-step s, output tile n, part p: W1[hid_unit(t, s, h, j)][out_ch(r, n)]
// and is read through the forward's ring.  With float32 GEMMs every product is the three bf16 products of the forward, smallest
// terms first.
//
// Epilogue, float32: x is loaded again (the registers that held it carry dxn by then), x^ = (x - mean) rstd, dx^ = dxn gamma,
//   dx = g + rstd (dx^ - mean(dx^) - x^ mean(dx^ x^))
// rounded once to x's type and stored as 16-byte vectors.  dgamma = sum_rows dxn x^ and dbeta = sum_rows dxn: the 32 rows of a
// wave are added by a butterfly that halves the register count with every exchange (16 values -> 1 per lane in 16 shuffles), the
// four waves of a workgroup in a fixed order through LDS, and the per-workgroup rows in scratch by a second launch in a fixed
// order.  No atomics: the same bytes in give the same bytes out.
//
// The weight gradients are reductions over rows and stay with the caller's GEMMs; on request the kernel writes their operands
// xn (rows, C), act = a (rows, 4C) and dhid = dh (rows, 4C), dense, in M.  A lane holds 4 consecutive units per register quad: 16
// bytes of float32, stored as they lie; of a half type two quads are paired with the other half of the row (lane ^ 32, one
// v_permlane32_swap per word) into one 16-byte store.
//
// One wave per SIMD, up to 512 registers, no scratch memory in any instantiation.  C = 256 with float32 GEMMs does not hold xn, gs
// and dxn in two parts each: that one instantiation keeps dxn and makes the B fragments of the h and da GEMMs again per k-step of
// every tile (BKEEP below).
#pragma once

#include "../../include/dhd_amd_ffn_train.h"

namespace {

template <class M, int C> struct TGeo {
  static constexpr int P = kParts<M>;
  static constexpr int KS = C / 16, NT = C / 32, HT = C / 8;
  static constexpr int N = 4 + 3 * KS * P;   // fragments per hidden tile: 28 / 52 (C = 128), 52 / 100 (C = 256)
  // 14 / 13, 13 / 10: beside the two-part operands of C = 256 the ring is kept at 40 registers
  static constexpr int R = C == 256 && P == 2 ? 10 : ring_size(N);
  static constexpr size_t kStreamBytes = (size_t)HT * N * 1024;
  static constexpr size_t kPackedBytes = kStreamBytes + (size_t)R * 1024;   // with the read-ahead's padding, as Geo::kScratchBytes
};

// act and dhid in a half type: 16 bytes per lane after a lane ^ 32 exchange (1, measured 2.5 - 4 % faster over forward + backward),
// or 8 bytes per lane as the quads lie (0: the form it was measured against)
#ifndef DHD_FFN_TRAIN_EXCHANGE_STORES
#define DHD_FFN_TRAIN_EXCHANGE_STORES 1
#endif
constexpr bool kExchangeStores = DHD_FFN_TRAIN_EXCHANGE_STORES;
constexpr int kParamBlock = 256;   // dgamma / dbeta: 16 lanes down the partial rows x 16 columns

// one thread per (hidden tile, fragment, lane): 16 bytes of the backward's stream
template <class M, int C>
__global__ __launch_bounds__(kPackBlock) void pack_train_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                                                const float* __restrict__ w2, u32x4* __restrict__ stream) {
  using G = TGeo<M, C>;
  constexpr int P = G::P, N = G::N, KS = G::KS, NT = G::NT, H = 4 * C, B = KS * P;
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
    stream[idx] = out;
    return;
  }
  const int g = (f - 4) % B, part = g % P;
  if (f < 4 + B) {
    const int ks = g / P;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w1[(size_t)(32 * t + r) * C + 16 * ks + 8 * h + j];
  } else if (f < 4 + 2 * B) {
    const int ks = g / P;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w2[(size_t)(16 * ks + 8 * h + j) * H + 32 * t + r];
  } else {
    const int n = (g / P) % NT, s = g / (P * NT);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w1[(size_t)hid_unit(t, s, h, j) * C + out_ch(r, n)];
  }
  make_parts<M>(v, parts);
  out = part ? parts[P - 1] : parts[0];
  stream[idx] = out;
}

// a = GELU(x) as gelu_erf gives it (the same t, poly, e and clamp), d = GELU'(x) = Phi(x) + x phi(x) from the same terms:
// Phi(x) = erfc(|x| / sqrt 2) / 2 for x < 0 and 1 minus that otherwise, phi(x) = e / sqrt(2 pi).  Absolute error of Phi below
// 0.75e-7; past the clamp e is below 3e-43 and x is taken as +-14, so +-inf give 1 and 0 and not inf * 0.  A NaN goes through
// both: a by gelu_erf's select, d by the select of the clamp.
__device__ __forceinline__ void gelu_erf_grad(float x, float& a, float& d) {
  constexpr float kRsqrt2 = 0.707106769084930419921875f, kLog2e = 1.44269502162933349609375f, kRsqrt2Pi = 0.3989422804014327f;
  const float ax = fminf(fabsf(x), 14.f);
  const float z = ax * kRsqrt2;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.f));
  const float poly = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
  const float e = __builtin_amdgcn_exp2f(-(z * z) * kLog2e);
  const float pe = poly * e;
  a = (x < 0.f ? 0.f : x) - (0.5f * ax) * pe;
  const float Phi = x < 0.f ? 0.5f * pe : 1.f - 0.5f * pe;
  const float xs = fabsf(x) > 14.f ? copysignf(14.f, x) : x;
  d = fmaf(xs, e * kRsqrt2Pi, Phi);
}

// 4 consecutive values rounded to M, stored as they lie: 16 bytes of float32, 8 of a half type
template <class M> __device__ __forceinline__ void store4(M* dst, const float* v) {
  if constexpr (std::is_same_v<M, float>) {
    *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
    *reinterpret_cast<u32x2*>(dst) = u32x2{Pair<M>::narrow(f32x2{v[0], v[1]}), Pair<M>::narrow(f32x2{v[2], v[3]})};
  }
}

// Two neighbouring register quads of a half type (units 8 k + 4 h + (0..3) and 8 (k + 1) + 4 h + (0..3) of a row that the lanes
// r and r + 32 share) after one half exchange per word (v_permlane32_swap): the lower lane holds units 8 k .. 8 k + 7, the upper
// lane 8 (k + 1) .. 8 (k + 1) + 7 -- 16 contiguous bytes each.  Every lane of the wave must take part.
template <class M> __device__ __forceinline__ u32x4 pair_quads(const float* v) {
  unsigned w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = Pair<M>::narrow(f32x2{v[2 * i], v[2 * i + 1]});
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const auto sw = __builtin_amdgcn_permlane32_swap(w[i], w[2 + i], false, false);
    w[i] = sw[0];
    w[2 + i] = sw[1];
  }
  return u32x4{w[0], w[1], w[2], w[3]};
}

// One step of the column sums: the lanes r and r ^ MASK share their 2 N values, each keeps the sums of N of them.
template <int MASK, int N> __device__ __forceinline__ void fold_step(float* v, int r) {
  const bool up = (r & MASK) != 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float keep = up ? v[i + N] : v[i];
    const float send = up ? v[i] : v[i + N];
    v[i] = keep + __shfl_xor(send, MASK, DHD_WAVE);
  }
}
// v[0..16) added over the 32 lanes that share lane >> 5; lane r returns the total of v[r >> 1].  a + b is b + a bit for bit, so
// both lanes of an exchange hold the same sums and the order of the additions is fixed.
__device__ __forceinline__ float col_sums16(float* v, int r) {
  fold_step<16, 8>(v, r);
  fold_step<8, 4>(v, r);
  fold_step<4, 2>(v, r);
  fold_step<2, 1>(v, r);
  return v[0] + __shfl_xor(v[0], 1, DHD_WAVE);
}

// the per-image factor of the forward: swin_ffn_kernel's S
struct ImageScale {
  static constexpr bool kOn = true;
  const float* factor;
  long rows_per_image;
};

template <class X, class M, int C>
__global__ __launch_bounds__(kBlock) void swin_ffn_bwd_kernel(const X* __restrict__ x, const X* __restrict__ dout,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const u32x4* __restrict__ stream, const float* __restrict__ scale,
                                                              long rows_per_image, X* __restrict__ dx, float* __restrict__ partial,
                                                              M* __restrict__ xn_out, M* __restrict__ act_out, M* __restrict__ dhid_out,
                                                              long rows, float eps) {
  using G = TGeo<M, C>;
  constexpr int P = G::P, N = G::N, R = G::R, KS = G::KS, NT = G::NT, HT = G::HT, RW = kRawVecs<X>, H = 4 * C;
  static_assert(N % R == 0, "the ring position of a fragment must not depend on the hidden tile");
  __shared__ float red[kBlock / 64][2 * C];   // per wave: sum_rows dxn x^ (C), sum_rows dxn (C)
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const long p0 = ((long)blockIdx.x * (kBlock / 64) + (tid >> 6)) * 32;   // wave-uniform
  float* myred = red[tid >> 6];
  if (p0 >= rows) {   // a wave past the last row adds nothing
    for (int i = lane; i < 2 * C; i += 64) myred[i] = 0.f;
  } else {
    const bool live = p0 + r < rows;   // a lane past the last row computes on the last row, stores nothing and adds nothing
    const long p = live ? p0 + r : rows - 1;
    const bool ops = xn_out != nullptr;   // uniform over the launch: all three operand tensors or none
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(stream), 0, (unsigned)G::kPackedBytes, 0x00020000);
    u32x4 ring[R];
    const int lane_off = lane * 16;
    static_for<R>([&](auto i) { ring[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, i * 1024, 0); });

    const X* xrow = x + (size_t)p * C + 8 * h;
    const X* grow = dout + (size_t)p * C + 8 * h;
    float mean, rstd;
    // BKEEP: xn and gs stay in registers for all hidden tiles.  C = 256 with the two-part float32 operands has no room for them
    // beside dxn: there the h and da GEMMs load their B fragment again for every k-step of every tile and normalise (scale) and
    // split it anew -- out of L2, and little VALU work beside the three MFMAs it feeds.
    constexpr bool BKEEP = !(C == 256 && std::is_same_v<M, float>);
    u32x4 xf[BKEEP ? KS : 1][P], gf[BKEEP ? KS : 1][P];
    u32x4 raw[KS][RW];   // the row as loaded: for the statistics and the first xn, dead after them
    {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) load_raw<X>(xrow, ks, raw[ks]);
      // the forward's statistics, operation for operation
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
      mean += de;   // the forward's correction of the mean by the residuals' average
      rstd = 1.f / sqrtf(fmaxf(var * (1.f / C) - de * de, 0.f) + eps);
    }
    // xn, rounded once to M: the B fragments of the h GEMM, and the operand of dW1
    // (`off` is 0: inside the tile loop a value the compiler cannot see through, or the loads would be hoisted out of the loop
    // and the registers they were meant to free would hold them again)
    auto make_xn = [&](const u32x4 (&xraw)[RW], int ks, u32x4 (&parts)[P], bool store, int off) {
      float v[8];
      widen8<X>(xraw, v);
      const f32x4* gp = reinterpret_cast<const f32x4*>(gamma + off + 16 * ks + 8 * h);
      const f32x4* bp = reinterpret_cast<const f32x4*>(beta + off + 16 * ks + 8 * h);
      const f32x4 g0 = gp[0], g1 = gp[1], c0 = bp[0], c1 = bp[1];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = ((v[j] - mean) * rstd) * (j < 4 ? g0[j & 3] : g1[j & 3]) + (j < 4 ? c0[j & 3] : c1[j & 3]);
      make_parts<M>(v, parts);
      if (store) {
        raw16<M>* o = reinterpret_cast<raw16<M>*>(xn_out + (size_t)p * C + 8 * h + 16 * ks);
#pragma unroll
        for (int w = 0; w < kRawVecs<M>; ++w) o[w] = narrow16<M>(v + w * kVec16<M>);
      }
    };
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) make_xn(raw[ks], ks, xf[BKEEP ? ks : 0], ops && live, 0);
    // gs = s g in float32, rounded once to M: the B fragments of the da GEMM
    const float sc = scale ? scale[p / rows_per_image] : 1.f;
    auto make_gs = [&](int ks, u32x4 (&parts)[P], int off) {
      u32x4 graw[RW];
      float v[8];
      load_raw<X>(grow + off, ks, graw);
      widen8<X>(graw, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= sc;
      make_parts<M>(v, parts);
    };
    if constexpr (BKEEP) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) make_gs(ks, gf[ks], 0);
    }

    f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[n][e] = 0.f;

    M* arow = act_out + (size_t)p * H + 4 * h;
    M* drow = dhid_out + (size_t)p * H + 4 * h;
    for (int t = 0; t < HT; ++t) {
      const int base = t * (N * 1024);
      auto take = [&](auto I) {   // fragment I out of the ring, its slot refilled at once (see swin_ffn_kernel)
        constexpr int i = decltype(I)::value;
        const u32x4 v = ring[i % R];
        ring[i % R] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, base + (i + R) * 1024, 0);
        __builtin_amdgcn_sched_barrier(0);
        return v;
      };
      // three products of the two-part operands, smallest terms first, or the one product of the rounded ones
      auto gemm_step = [&](auto I0, const u32x4 (&b)[P], f32x16 c) {
        constexpr int i0 = decltype(I0)::value;
        if constexpr (P == 2) {
          const u32x4 wh = take(std::integral_constant<int, i0>{});
          const u32x4 wm = take(std::integral_constant<int, i0 + 1>{});
          c = mfma16<M>(wm, b[0], c);
          c = mfma16<M>(wh, b[P - 1], c);
          return mfma16<M>(wh, b[0], c);
        } else {
          return mfma16<M>(take(std::integral_constant<int, i0>{}), b[0], c);
        }
      };
      int tz = 0;   // zero, opaque per tile: what keeps the reloads of the !BKEEP form inside the loop
      if constexpr (!BKEEP) asm volatile("" : "+v"(tz));
      f32x16 hid, da;
      static_for<4>([&](auto F) {
        const u32x4 v = take(F);
#pragma unroll
        for (int e = 0; e < 4; ++e) hid[4 * F + e] = __uint_as_float(v[e]);
      });
#pragma unroll
      for (int e = 0; e < 16; ++e) da[e] = 0.f;
      static_for<KS>([&](auto KSI) {
        constexpr int ks = decltype(KSI)::value;
        if constexpr (!BKEEP) {
          u32x4 xraw[RW];
          load_raw<X>(xrow + tz, ks, xraw);
          make_xn(xraw, ks, xf[0], false, tz);
        }
        hid = gemm_step(std::integral_constant<int, 4 + ks * P>{}, xf[BKEEP ? ks : 0], hid);
      });
      static_for<KS>([&](auto KSI) {
        constexpr int ks = decltype(KSI)::value;
        if constexpr (!BKEEP) make_gs(ks, gf[0], tz);
        da = gemm_step(std::integral_constant<int, 4 + (KS + ks) * P>{}, gf[BKEEP ? ks : 0], da);
      });
      float a[16], d[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        gelu_erf_grad(hid[e], a[e], d[e]);
        d[e] *= da[e];
      }
      if constexpr (kExchangeStores && !std::is_same_v<M, float>) {
        if (ops) {
#pragma unroll
          for (int m = 0; m < 2; ++m) {   // quads 2 m and 2 m + 1 -> units 32 t + 16 m + 8 h + (0..7): one 16-byte store
            const u32x4 wa = pair_quads<M>(a + 8 * m), wd = pair_quads<M>(d + 8 * m);
            if (live) {
              *reinterpret_cast<u32x4*>(arow - 4 * h + 32 * t + 16 * m + 8 * h) = wa;
              *reinterpret_cast<u32x4*>(drow - 4 * h + 32 * t + 16 * m + 8 * h) = wd;
            }
          }
        }
      } else if (ops && live) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {   // register quad q = units 32 t + 8 q + 4 h + (0..3)
          store4<M>(arow + 32 * t + 8 * q, a + 4 * q);
          store4<M>(drow + 32 * t + 8 * q, d + 4 * q);
        }
      }
      u32x4 df[2][P];
#pragma unroll
      for (int s = 0; s < 2; ++s) make_parts<M>(d + 8 * s, df[s]);
      static_for<2 * NT>([&](auto GI) {
        constexpr int g = decltype(GI)::value, s = g / NT, n = g % NT;
        acc[n] = gemm_step(std::integral_constant<int, 4 + (2 * KS + g) * P>{}, df[s], acc[n]);
      });
    }

    // register 8 s + j of tile n = d xn of channel 16 (2 n + s) + 8 h + j of this lane's row.  First pass: the parameter sums,
    // dx^ = dxn gamma in place of dxn, and the two row means.
    float s1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, s2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int ks = 2 * n + s;
        u32x4 raw[RW];
        float xh[8], cs[16];
        load_raw<X>(xrow, ks, raw);
        widen8<X>(raw, xh);
        const f32x4* gp = reinterpret_cast<const f32x4*>(gamma + 16 * ks + 8 * h);
        const f32x4 g0 = gp[0], g1 = gp[1];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          xh[j] = (xh[j] - mean) * rstd;
          const float dn = acc[n][8 * s + j];
          cs[j] = live ? dn * xh[j] : 0.f;
          cs[8 + j] = live ? dn : 0.f;
          const float dh = dn * (j < 4 ? g0[j & 3] : g1[j & 3]);
          acc[n][8 * s + j] = dh;
          s1[j] += dh;
          s2[j] = fmaf(dh, xh[j], s2[j]);
        }
        const float total = col_sums16(cs, r);   // of cs[r >> 1]: dgamma's term of channel j for r < 16, dbeta's from there
        if ((r & 1) == 0) myred[(r >> 4) * C + 16 * ks + 8 * h + ((r >> 1) & 7)] = total;
      }
    float m1 = sum8(s1), m2 = sum8(s2);
    m1 += __shfl_xor(m1, 32, DHD_WAVE);
    m2 += __shfl_xor(m2, 32, DHD_WAVE);
    m1 *= 1.f / C;
    m2 *= 1.f / C;
    X* dxrow = dx + (size_t)p * C + 8 * h;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int ks = 2 * n + s;
        u32x4 raw[RW], graw[RW];
        float xh[8], gv[8], o[8];
        load_raw<X>(xrow, ks, raw);
        load_raw<X>(grow, ks, graw);
        widen8<X>(raw, xh);
        widen8<X>(graw, gv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xhat = (xh[j] - mean) * rstd;
          o[j] = gv[j] + rstd * ((acc[n][8 * s + j] - m1) - xhat * m2);
        }
        if (live) {
          raw16<X>* q = reinterpret_cast<raw16<X>*>(dxrow + 16 * ks);
#pragma unroll
          for (int w = 0; w < RW; ++w) q[w] = narrow16<X>(o + w * kVec16<X>);
        }
      }
  }
  __syncthreads();
  // the workgroup's partial row: its four waves in a fixed order
  float* prow = partial + (size_t)blockIdx.x * (2 * C);
  for (int i = tid; i < 2 * C; i += kBlock) prow[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// partial (groups, 2 C) -> dgamma (C), dbeta (C).  A workgroup owns 16 columns: 16 lanes walk down the rows, each adding every
// 16th row in order, then lane 0 of a column adds the 16 sums in order.
__global__ __launch_bounds__(kParamBlock) void swin_ffn_bwd_params(const float* __restrict__ partial, float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta, int groups, int c) {
  __shared__ float sums[16][17];
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4, col = blockIdx.x * 16 + cl;
  float a = 0.f;
#pragma unroll 4
  for (int g = rl; g < groups; g += 16) a += partial[(size_t)g * (2 * c) + col];
  sums[rl][cl] = a;
  __syncthreads();
  if (rl == 0) {
    float t = sums[0][cl];
    for (int i = 1; i < 16; ++i) t += sums[i][cl];
    if (col < c) dgamma[col] = t;
    else dbeta[col - c] = t;
  }
}

// every combination of the inference family
bool train_supported(int c, int hidden, int x_dtype, int mm_dtype) { return shape_supported(c, hidden) && precision_supported(x_dtype, mm_dtype); }

size_t train_packed_bytes(int c, int mm_dtype) {
  if (c == 128) return mm_dtype == DHD_F32 ? TGeo<float, 128>::kPackedBytes : TGeo<__bf16, 128>::kPackedBytes;
  return mm_dtype == DHD_F32 ? TGeo<float, 256>::kPackedBytes : TGeo<__bf16, 256>::kPackedBytes;
}

template <class X, class M, int C>
int train_backward(const void* x, const void* dout, const float* gamma, const float* beta, const float* w1, const float* b1,
                   const float* w2, const float* scale, long rows_per_image, void* dx, float* dgamma, float* dbeta, void* xn, void* act,
                   void* dhid, void* scratch, long rows, float eps, hipStream_t st) {
  using G = TGeo<M, C>;
  u32x4* stream = static_cast<u32x4*>(scratch);
  float* partial = reinterpret_cast<float*>(static_cast<char*>(scratch) + G::kPackedBytes);
  constexpr int n_pack = G::HT * G::N * 64;
  const int groups = dhd_cdiv(rows, kRowsPerBlock);
  hipLaunchKernelGGL((pack_train_kernel<M, C>), dim3(dhd_cdiv(n_pack, kPackBlock)), dim3(kPackBlock), 0, st, w1, b1, w2, stream);
  DHD_LAUNCH_CHECK();
  hipLaunchKernelGGL((swin_ffn_bwd_kernel<X, M, C>), dim3(groups), dim3(kBlock), 0, st, static_cast<const X*>(x),
                     static_cast<const X*>(dout), gamma, beta, stream, scale, rows_per_image, static_cast<X*>(dx), partial,
                     static_cast<M*>(xn), static_cast<M*>(act), static_cast<M*>(dhid), rows, eps);
  DHD_LAUNCH_CHECK();
  hipLaunchKernelGGL(swin_ffn_bwd_params, dim3(2 * C / 16), dim3(kParamBlock), 0, st, partial, dgamma, dbeta, groups, C);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

// f.template operator()<X, M, C>() for the element types of the two dtype codes and the C of a supported call
template <class F> int train_dispatch(int x_dtype, int mm_dtype, int c, F&& f) {
  return dhd::with_dtype<dhd::NativeHalf>(x_dtype, [&](auto* xp) {
    using X = std::remove_pointer_t<decltype(xp)>;
    return dhd::with_dtype<dhd::NativeHalf>(mm_dtype, [&](auto* mp) {
      using M = std::remove_pointer_t<decltype(mp)>;
      if constexpr (std::is_same_v<X, float> || std::is_same_v<X, M>) {
        return c == 128 ? f(xp, mp, std::integral_constant<int, 128>{}) : f(xp, mp, std::integral_constant<int, 256>{});
      } else {
        return (int)DHD_EUNSUPPORTED;
      }
    });
  });
}

}  // namespace

extern "C" {

int dhdt_swin_ffn_supported(int c, int hidden, int x_dtype, int mm_dtype) { return train_supported(c, hidden, x_dtype, mm_dtype) ? 1 : 0; }

size_t dhdt_swin_ffn_forward_scratch_bytes(int c, int hidden, int mm_dtype) {
  if (!shape_supported(c, hidden) || !dtype_code(mm_dtype)) return 0;
  return scratch_bytes(c, mm_dtype);
}

size_t dhdt_swin_ffn_backward_scratch_bytes(long rows, int c, int hidden, int mm_dtype) {
  if (!shape_supported(c, hidden) || !dtype_code(mm_dtype) || rows <= 0 || rows > kMaxRows) return 0;
  return train_packed_bytes(c, mm_dtype) + (size_t)dhd_cdiv(rows, kRowsPerBlock) * 2 * c * sizeof(float);
}

int dhdt_swin_ffn_forward(const void* x, const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2,
                          const float* b2, const float* scale, long rows_per_image, void* out, void* scratch, size_t scratch_size,
                          int x_dtype, int mm_dtype, long rows, int c, int hidden, float eps, void* stream) {
  if (!x || !gamma || !beta || !w1 || !b1 || !w2 || !b2 || !out || !scratch || rows <= 0) return DHD_EINVAL;
  if (!dhd_aligned(16, x, gamma, beta, w1, b1, w2, b2, scale, out, scratch)) return DHD_EINVAL;
  if (scale && (rows_per_image <= 0 || rows % rows_per_image != 0)) return DHD_EINVAL;
  if (!train_supported(c, hidden, x_dtype, mm_dtype) || rows > kMaxRows) return DHD_EUNSUPPORTED;
  if (scratch_size < scratch_bytes(c, mm_dtype)) return DHD_ENOSPACE;
  hipStream_t st = dhd_stream(stream);
  return train_dispatch(x_dtype, mm_dtype, c, [&](auto* xp, auto* mp, auto cc) {
    using X = std::remove_pointer_t<decltype(xp)>;
    using M = std::remove_pointer_t<decltype(mp)>;
    constexpr int C = decltype(cc)::value;
    // without a factor this IS the inference operator: the same two launches, the same bytes
    if (!scale) return launch<X, M, C>(x, gamma, beta, w1, b1, w2, b2, out, scratch, rows, eps, st);
    return launch<X, M, C, ImageScale>(x, gamma, beta, w1, b1, w2, b2, out, scratch, rows, eps, st, ImageScale{scale, rows_per_image});
  });
}

int dhdt_swin_ffn_backward(const void* x, const void* dout, const float* gamma, const float* beta, const float* w1, const float* b1,
                           const float* w2, const float* scale, long rows_per_image, void* dx, float* dgamma, float* dbeta, void* xn,
                           void* act, void* dhid, void* scratch, size_t scratch_size, int x_dtype, int mm_dtype, long rows, int c,
                           int hidden, float eps, void* stream) {
  if (!x || !dout || !gamma || !beta || !w1 || !b1 || !w2 || !dx || !dgamma || !dbeta || !scratch || rows <= 0) return DHD_EINVAL;
  if ((xn == nullptr) != (act == nullptr) || (xn == nullptr) != (dhid == nullptr)) return DHD_EINVAL;   // the operands: all or none
  if (!dhd_aligned(16, x, dout, gamma, beta, w1, b1, w2, scale, dx, dgamma, dbeta, xn, act, dhid, scratch)) return DHD_EINVAL;
  if (scale && (rows_per_image <= 0 || rows % rows_per_image != 0)) return DHD_EINVAL;
  if (!train_supported(c, hidden, x_dtype, mm_dtype) || rows > kMaxRows) return DHD_EUNSUPPORTED;
  if (scratch_size < dhdt_swin_ffn_backward_scratch_bytes(rows, c, hidden, mm_dtype)) return DHD_ENOSPACE;
  hipStream_t st = dhd_stream(stream);
  return train_dispatch(x_dtype, mm_dtype, c, [&](auto* xp, auto* mp, auto cc) {
    using X = std::remove_pointer_t<decltype(xp)>;
    using M = std::remove_pointer_t<decltype(mp)>;
    constexpr int C = decltype(cc)::value;
    return train_backward<X, M, C>(x, dout, gamma, beta, w1, b1, w2, scale, rows_per_image, dx, dgamma, dbeta, xn, act, dhid, scratch,
                                   rows, eps, st);
  });
}

}  // extern "C"
