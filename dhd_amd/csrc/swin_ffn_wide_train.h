// Swin FFN in training for C = 512 (dhd_amd/include/dhd_amd_ffn_wide_train.h): the wide family's forward with the per-image
// factor of DropPath on the branch, and a recompute backward in the wide family's form.  swin_ffn.hip includes this file after
// swin_ffn_wide.h and swin_ffn_train.h: gelu_erf_grad, pair_quads, store4, col_sums16, ImageScale and swin_ffn_bwd_params of the
// narrow training pair, make_parts4, mfma_parts, wave_sum, the ring and the tile pitches of the wide family, and make_parts, mfma16,
// out_ch, load_raw / widen8 and the dtype predicates of swin_ffn.hip are used as they are.
//
// Forward: swin_ffn_wide_kernel with ImageScale as its S, on the inference operator's weight stream and scratch size.
//
// Backward, for g = dout and gs = s g (what include/dhd_amd_ffn_train.h section T1 defines).  A workgroup of 4 waves owns T rows: 64
// with one half part, 32 with the two bf16 parts of float32.
//   * Prologue: wave w normalises the rows [w T / 4, (w + 1) T / 4), one row at a time over the 64 lanes with the forward's
//     statistics, operation for operation.  xn, rounded once to the GEMM type (or split), goes into the LDS tile [part][row][C] of
//     the forward and -- on request -- to memory as the operand of dW1; gs = s g, the float32 product rounded once, into a second
//     tile of the same shape; mean and rstd of the row into LDS.
//   * Per hidden chunk of HC = 128 units wave w owns the unit tile [32 w, 32 (w + 1)) of the chunk for all T rows:
//       h  = W1 . xn + b1         W1 fragments on the MFMA A operand, the xn tile on B: the forward's GEMM-1
//       da = W2^T . gs            A rows are the units, k runs over the channels, the gs tile on B: h's register layout
//       a = gelu(h), dh = da gelu'(h)        float32, in registers; on request a and dh go to memory as 16-byte vectors
//     dh, rounded once (or split), goes to the LDS chunk buffer [part][row][HC]; then
//       dxn += W1^T . dh          wave w owns the channels [w C / 4, (w + 1) C / 4): the forward's GEMM-2 with W1^T for W2
//     One chunk buffer (two do not fit beside two tiles): the barrier before the write waits for the readers of the chunk before,
//     which have the h and da GEMMs of this chunk behind them by then; the barrier after it publishes the chunk.
//   * Epilogue, float32: x^ = (x - mean) rstd from x read again, dx^ = dxn gamma.  A row's channels are spread over the four
//     waves: each wave adds its 128 channels of dx^ and dx^ x^ (two lanes per row), writes the two sums to LDS, and after a
//     barrier every lane adds the four waves' sums in a fixed order.  dx = g + rstd (dx^ - mean(dx^) - x^ mean(dx^ x^)), rounded
//     once, 16-byte stores in x's own layout.
//   * dgamma / dbeta: the T rows of a workgroup are added per channel by the narrow kernel's butterfly (col_sums16), the wave
//     that owns a channel writes the workgroup's partial row in scratch, and swin_ffn_bwd_params adds the rows in a fixed order.
// No atomics.  A row past the last one computes on the last row, stores nothing and adds nothing.
//
// The weight stream (pack_wide_train_kernel, once per call): per wave and chunk, unit0 = HC t + 32 w,
//   4               b1, register e of fragment f = b1[unit0 + 8 f + 4 h + e]
//   C / 16 * P      h:   k-step ks, part p: W1[unit0 + r][16 ks + 8 h + j]
//   C / 16 * P      da:  k-step ks, part p: W2[16 ks + 8 h + j][unit0 + r]
//   HC / 16 * MT P  dxn: k-step s, channel tile m, part p: W1[HC t + 16 s + 8 h + j][out_ch(r, MT w + m)]
#pragma once

// (The surface's header is not included here: it names "dhd_amd.h" as a caller with both include directories on its path does,
// and this build has no include path.  tests/test_swin_ffn_wide_train_capi.py holds the definitions below to its declarations.)

namespace {

template <class M, int C> struct WTGeo {
  static constexpr int P = kParts<M>;
  static constexpr int T = P == 2 ? 32 : 64;        // rows of a workgroup
  static constexpr int HC = 32 * kWideWaves;        // hidden units of a chunk: one unit tile per wave
  static constexpr int RT = T / 32;                 // row tiles
  static constexpr int MT = C / (32 * kWideWaves);  // channel tiles of a wave
  static constexpr int KS = C / 16;                 // k-steps of the h and da GEMMs
  static constexpr int HS = HC / 16;                // k-steps of the dxn GEMM per chunk
  static constexpr int NCH = 4 * C / HC;            // chunks
  static constexpr int NB = 4;                      // bias fragments
  static constexpr int NG = KS * P;                 // fragments of the h GEMM, and of the da GEMM
  static constexpr int N = NB + 2 * NG + HS * MT * P;   // fragments per (wave, chunk): 100 / 196
  static constexpr int R = ring_size(N);            // 20 / 14
  static constexpr int XS = WGeo<M, C>::XS;         // bytes of a tile row
  static constexpr int HB = 2 * HC + 16;            // bytes of a chunk row
  static constexpr int kTileBytes = P * T * XS;     // one of the two tiles
  static constexpr int kHidBytes = P * T * HB;
  static constexpr int kStatBytes = T * 2 * 4;      // mean, rstd per row
  static constexpr int kRedBytes = T * kWideWaves * 2 * 4;   // per row and wave: sum dx^, sum dx^ x^
  static constexpr int kLdsBytes = 2 * kTileBytes + kHidBytes + kStatBytes + kRedBytes;   // 153 088 with either GEMM type
  static constexpr size_t kWaveBytes = (size_t)NCH * N * 1024;
  static constexpr size_t kStreamBytes = kWideWaves * kWaveBytes;
  static constexpr size_t kPackedBytes = kStreamBytes + (size_t)R * 1024;   // the last wave's read-ahead (read, never used)
  static_assert(C == 512 && N % R == 0 && kLdsBytes <= 160 * 1024 && kPackedBytes < (1u << 31), "geometry");
};

// one thread per (wave, chunk, fragment, lane): 16 bytes of the backward's stream
template <class M, int C>
__global__ __launch_bounds__(kPackBlock) void pack_wide_train_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                                                     const float* __restrict__ w2, u32x4* __restrict__ stream) {
  using G = WTGeo<M, C>;
  constexpr int P = G::P, N = G::N, MT = G::MT, H = 4 * C;
  const int idx = blockIdx.x * kPackBlock + threadIdx.x;
  if (idx >= kWideWaves * G::NCH * N * 64) return;
  const int lane = idx & 63, r = lane & 31, h = lane >> 5;
  const int q = idx >> 6, f = q % N, t = (q / N) % G::NCH, w = q / (N * G::NCH);
  const int unit0 = G::HC * t + 32 * w;
  float v[8];
  u32x4 parts[P];
  u32x4 out;
  if (f < G::NB) {
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = __float_as_uint(b1[unit0 + 8 * f + 4 * h + e]);
    stream[idx] = out;
    return;
  }
  if (f < G::NB + G::NG) {
    const int g = f - G::NB, ks = g / P;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w1[(size_t)(unit0 + r) * C + 16 * ks + 8 * h + j];
  } else if (f < G::NB + 2 * G::NG) {
    const int g = f - G::NB - G::NG, ks = g / P;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w2[(size_t)(16 * ks + 8 * h + j) * H + unit0 + r];
  } else {
    const int g = f - G::NB - 2 * G::NG, m = (g / P) % MT, s = g / (P * MT);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w1[(size_t)(G::HC * t + 16 * s + 8 * h + j) * C + out_ch(r, MT * w + m)];
  }
  const int part = (f - G::NB) % P;   // NG and HS MT P are multiples of P
  make_parts<M>(v, parts);
  out = part ? parts[P - 1] : parts[0];
  stream[idx] = out;
}

template <class X, class M, int C>
__global__ __launch_bounds__(kWideBlock) void swin_ffn_wide_bwd_kernel(const X* __restrict__ x, const X* __restrict__ dout,
                                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                       const u32x4* __restrict__ stream, const float* __restrict__ scale,
                                                                       long rows_per_image, X* __restrict__ dx, float* __restrict__ partial,
                                                                       M* __restrict__ xn_out, M* __restrict__ act_out,
                                                                       M* __restrict__ dhid_out, long rows, float eps) {
  using G = WTGeo<M, C>;
  constexpr int P = G::P, T = G::T, N = G::N, R = G::R, KS = G::KS, HS = G::HS, RT = G::RT, MT = G::MT, RW = kRawVecs<X>, H = 4 * C;
  static_assert(C == 512, "a lane holds 8 channels of a row in the LayerNorm pass");
  __shared__ __attribute__((aligned(16))) unsigned char lds[G::kLdsBytes];
  unsigned char* const xt = lds;                         // xn
  unsigned char* const gt = lds + G::kTileBytes;         // gs
  unsigned char* const hb = lds + 2 * G::kTileBytes;     // the chunk of dh
  float* const stat = reinterpret_cast<float*>(hb + G::kHidBytes);
  float* const red = stat + 2 * T;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long p0 = (long)blockIdx.x * T;   // < rows: the grid is cdiv(rows, T)
  const bool ops = xn_out != nullptr;     // uniform over the launch: all three operand tensors or none
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(stream)) + w * G::kWaveBytes, 0,
      (unsigned)(G::kPackedBytes - w * G::kWaveBytes), 0x00020000);
  u32x4 ring[R];
  const int lane_off = lane * 16;
  static_for<R>([&](auto i) { ring[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, i * 1024, 0); });

  // ---- prologue: wave w normalises the rows [w T / 4, (w + 1) T / 4) of the tile and scales their gradient
  {
    float gv[8], bv[8];
    {
      const f32x4* gp = reinterpret_cast<const f32x4*>(gamma + 8 * lane);
      const f32x4* bp = reinterpret_cast<const f32x4*>(beta + 8 * lane);
      const f32x4 g0 = gp[0], g1 = gp[1], c0 = bp[0], c1 = bp[1];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        gv[j] = j < 4 ? g0[j & 3] : g1[j & 3];
        bv[j] = j < 4 ? c0[j & 3] : c1[j & 3];
      }
    }
#pragma unroll 2
    for (int i = 0; i < T / kWideWaves; ++i) {
      const int rl = w * (T / kWideWaves) + i;
      const bool live = p0 + rl < rows;   // wave-uniform
      const long p = live ? p0 + rl : rows - 1;
      u32x4 raw[RW];
      float v[8], d[8];
      load_raw<X>(x + (size_t)p * C + 8 * lane, 0, raw);   // channels 8 lane + j
      widen8<X>(raw, v);
      // the wide forward's statistics, operation for operation
      float mean = wave_sum(sum8(v)) * (1.f / C);
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = v[j] - mean;
      const float de = wave_sum(sum8(d)) * (1.f / C);
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] *= d[j];
      mean += de;   // the forward's correction of the mean by the residuals' average
      const float rstd = 1.f / sqrtf(fmaxf(wave_sum(sum8(d)) * (1.f / C) - de * de, 0.f) + eps);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = ((v[j] - mean) * rstd) * gv[j] + bv[j];
      u32x4 parts[P];
      make_parts<M>(v, parts);   // rounded once to the type fc1 reads
#pragma unroll
      for (int part = 0; part < P; ++part) *reinterpret_cast<u32x4*>(xt + (part * T + rl) * G::XS + 16 * lane) = parts[part];
      if (ops && live) {
        raw16<M>* o = reinterpret_cast<raw16<M>*>(xn_out + (size_t)p * C + 8 * lane);
#pragma unroll
        for (int q = 0; q < kRawVecs<M>; ++q) o[q] = narrow16<M>(v + q * kVec16<M>);
      }
      if (lane == 0) {
        stat[2 * rl] = mean;
        stat[2 * rl + 1] = rstd;
      }
      // gs = s g in float32, rounded once to the GEMM type
      const float sc = scale ? scale[p / rows_per_image] : 1.f;
      load_raw<X>(dout + (size_t)p * C + 8 * lane, 0, raw);
      widen8<X>(raw, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= sc;
      make_parts<M>(v, parts);
#pragma unroll
      for (int part = 0; part < P; ++part) *reinterpret_cast<u32x4*>(gt + (part * T + rl) * G::XS + 16 * lane) = parts[part];
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

  // this lane's B-operand offsets: row r of row tile 0, k = 8 h
  const int xoff = r * G::XS + 16 * h;
  const int hrow = r * G::HB;
  long prow[RT];     // this lane's row of every row tile, a row past the last one as the last one
  bool plive[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    plive[rt] = p0 + 32 * rt + r < rows;
    prow[rt] = plive[rt] ? p0 + 32 * rt + r : rows - 1;
  }

  for (int t = 0; t < G::NCH; ++t) {
    const int base = t * (N * 1024);
    auto take = [&](auto I) {   // fragment I of the chunk out of the ring, its slot refilled (see swin_ffn_kernel)
      constexpr int i = decltype(I)::value;
      const u32x4 v = ring[i % R];
      ring[i % R] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, base + (i + R) * 1024, 0);
      __builtin_amdgcn_sched_barrier(0);
      return v;
    };
    const int unit0 = G::HC * t + 32 * w;

    // ---- h = W1 . xn + b1 and da = W2^T . gs: the wave's unit tile x all rows
    f32x16 hid[RT], da[RT];
    static_for<G::NB>([&](auto F) {
      constexpr int f = decltype(F)::value;
      const u32x4 v = take(F);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int e = 0; e < 4; ++e) hid[rt][4 * f + e] = __uint_as_float(v[e]);
    });
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int e = 0; e < 16; ++e) da[rt][e] = 0.f;
    auto gemm_tile = [&](const unsigned char* tile, auto I0, f32x16 (&c)[RT]) {
      constexpr int i0 = decltype(I0)::value;
      u32x4 bx[2][RT][P];
      auto load_b = [&](auto KSI, u32x4 (&b)[RT][P]) {
        constexpr int ks = decltype(KSI)::value;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int part = 0; part < P; ++part)
            b[rt][part] = *reinterpret_cast<const u32x4*>(tile + xoff + (part * T + 32 * rt) * G::XS + 32 * ks);
      };
      load_b(std::integral_constant<int, 0>{}, bx[0]);
      static_for<KS>([&](auto KSI) {
        constexpr int ks = decltype(KSI)::value;
        if constexpr (ks + 1 < KS) load_b(std::integral_constant<int, ks + 1>{}, bx[(ks + 1) & 1]);   // one k-step ahead of its use
        u32x4 wf[P];
        wf[0] = take(std::integral_constant<int, i0 + ks * P>{});
        if constexpr (P == 2) wf[P - 1] = take(std::integral_constant<int, i0 + ks * P + P - 1>{});
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) c[rt] = mfma_parts<M>(wf, bx[ks & 1][rt], c[rt]);
      });
    };
    gemm_tile(xt, std::integral_constant<int, G::NB>{}, hid);
    gemm_tile(gt, std::integral_constant<int, G::NB + G::NG>{}, da);

    // ---- a = gelu(h), dh = da gelu'(h) in float32: register 4 f + e is unit unit0 + 8 f + 4 h + e of row 32 rt + r
    u32x2 dparts[RT][4][P];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      float a[16], d[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        gelu_erf_grad(hid[rt][e], a[e], d[e]);
        d[e] *= da[rt][e];
      }
      if (ops) {
        M* arow = act_out + (size_t)prow[rt] * H + unit0;
        M* drow = dhid_out + (size_t)prow[rt] * H + unit0;
        if constexpr (!std::is_same_v<M, float>) {
#pragma unroll
          for (int m = 0; m < 2; ++m) {   // quads 2 m and 2 m + 1 -> units unit0 + 16 m + 8 h + (0..7): one 16-byte store
            const u32x4 wa = pair_quads<M>(a + 8 * m), wd = pair_quads<M>(d + 8 * m);
            if (plive[rt]) {
              *reinterpret_cast<u32x4*>(arow + 16 * m + 8 * h) = wa;
              *reinterpret_cast<u32x4*>(drow + 16 * m + 8 * h) = wd;
            }
          }
        } else if (plive[rt]) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {   // register quad q = units unit0 + 8 q + 4 h + (0..3)
            store4<M>(arow + 8 * q + 4 * h, a + 4 * q);
            store4<M>(drow + 8 * q + 4 * h, d + 4 * q);
          }
        }
      }
#pragma unroll
      for (int f = 0; f < 4; ++f) make_parts4<M>(d + 4 * f, dparts[rt][f]);
    }
    __syncthreads();   // the chunk before is read out
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int part = 0; part < P; ++part)
          *reinterpret_cast<u32x2*>(hb + (part * T + 32 * rt) * G::HB + hrow + (32 * w + 8 * f + 4 * h) * 2) = dparts[rt][f][part];
    __syncthreads();

    // ---- dxn += W1^T . dh: the wave's channel slice x all rows over the chunk's units
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
        constexpr int m = decltype(MI)::value, i0 = G::NB + 2 * G::NG + (s * MT + m) * P;
        u32x4 wf[P];
        wf[0] = take(std::integral_constant<int, i0>{});
        if constexpr (P == 2) wf[P - 1] = take(std::integral_constant<int, i0 + P - 1>{});
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[m][rt] = mfma_parts<M>(wf, bh[s & 1][rt], acc[m][rt]);
      });
    });
  }

  // ---- epilogue.  Register 8 s + j of tile (m, rt) = d xn of channel 16 ks + 8 h + j, ks = 2 (MT w + m) + s, of row 32 rt + r.
  // First pass: the parameter sums, dx^ = dxn gamma in place of dxn, and the wave's share of the two row sums.
  float mean[RT], rstd[RT], s1[RT][8], s2[RT][8];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    mean[rt] = stat[2 * (32 * rt + r)];
    rstd[rt] = stat[2 * (32 * rt + r) + 1];
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[rt][j] = s2[rt][j] = 0.f;
  }
  float* prt = partial + (size_t)blockIdx.x * (2 * C);
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int ks = 2 * (MT * w + m) + s;
      const f32x4* gp = reinterpret_cast<const f32x4*>(gamma + 16 * ks + 8 * h);
      const f32x4 g0 = gp[0], g1 = gp[1];
      float cs[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) cs[j] = 0.f;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        u32x4 raw[RW];
        float xh[8];
        load_raw<X>(x + (size_t)prow[rt] * C + 8 * h, ks, raw);
        widen8<X>(raw, xh);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          xh[j] = (xh[j] - mean[rt]) * rstd[rt];
          const float dn = acc[m][rt][8 * s + j];
          cs[j] += plive[rt] ? dn * xh[j] : 0.f;
          cs[8 + j] += plive[rt] ? dn : 0.f;
          const float dh = dn * (j < 4 ? g0[j & 3] : g1[j & 3]);
          acc[m][rt][8 * s + j] = dh;
          s1[rt][j] += dh;
          s2[rt][j] = fmaf(dh, xh[j], s2[rt][j]);
        }
      }
      const float total = col_sums16(cs, r);   // of cs[r >> 1]: dgamma's term of channel j for r < 16, dbeta's from there
      if ((r & 1) == 0) prt[(r >> 4) * C + 16 * ks + 8 * h + ((r >> 1) & 7)] = total;
    }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    float m1 = sum8(s1[rt]), m2 = sum8(s2[rt]);
    m1 += __shfl_xor(m1, 32, DHD_WAVE);
    m2 += __shfl_xor(m2, 32, DHD_WAVE);
    if (h == 0) {
      red[((32 * rt + r) * kWideWaves + w) * 2] = m1;
      red[((32 * rt + r) * kWideWaves + w) * 2 + 1] = m2;
    }
  }
  __syncthreads();
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const float* q = red + (32 * rt + r) * kWideWaves * 2;   // the four waves in a fixed order
    const float m1 = (((q[0] + q[2]) + q[4]) + q[6]) * (1.f / C), m2 = (((q[1] + q[3]) + q[5]) + q[7]) * (1.f / C);
    const X* xrow = x + (size_t)prow[rt] * C + 8 * h;
    const X* grow = dout + (size_t)prow[rt] * C + 8 * h;
    X* dxrow = dx + (size_t)prow[rt] * C + 8 * h;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int ks = 2 * (MT * w + m) + s;
        u32x4 raw[RW], graw[RW];
        float xh[8], gv[8], o[8];
        load_raw<X>(xrow, ks, raw);
        load_raw<X>(grow, ks, graw);
        widen8<X>(raw, xh);
        widen8<X>(graw, gv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xhat = (xh[j] - mean[rt]) * rstd[rt];
          o[j] = gv[j] + rstd[rt] * ((acc[m][rt][8 * s + j] - m1) - xhat * m2);
        }
        if (plive[rt]) {
          raw16<X>* q16 = reinterpret_cast<raw16<X>*>(dxrow + 16 * ks);
#pragma unroll
          for (int v = 0; v < RW; ++v) q16[v] = narrow16<X>(o + v * kVec16<X>);
        }
      }
  }
}

bool wide_train_supported(int c, int hidden, int x_dtype, int mm_dtype) {
  return c == 512 && hidden == 4 * c && precision_supported(x_dtype, mm_dtype);
}

size_t wide_train_packed_bytes(int mm_dtype) {
  return mm_dtype == DHD_F32 ? WTGeo<float, 512>::kPackedBytes : WTGeo<__bf16, 512>::kPackedBytes;
}

long wide_train_groups(long rows, int mm_dtype) {
  return dhd_cdiv(rows, (long)(mm_dtype == DHD_F32 ? WTGeo<float, 512>::T : WTGeo<__bf16, 512>::T));
}

template <class X, class M, int C>
int wide_train_backward(const void* x, const void* dout, const float* gamma, const float* beta, const float* w1, const float* b1,
                        const float* w2, const float* scale, long rows_per_image, void* dx, float* dgamma, float* dbeta, void* xn,
                        void* act, void* dhid, void* scratch, long rows, float eps, hipStream_t st) {
  using G = WTGeo<M, C>;
  u32x4* stream = static_cast<u32x4*>(scratch);
  float* partial = reinterpret_cast<float*>(static_cast<char*>(scratch) + G::kPackedBytes);
  constexpr int n_pack = kWideWaves * G::NCH * G::N * 64;
  const long groups = dhd_cdiv(rows, (long)G::T);
  hipLaunchKernelGGL((pack_wide_train_kernel<M, C>), dim3(dhd_cdiv(n_pack, kPackBlock)), dim3(kPackBlock), 0, st, w1, b1, w2, stream);
  DHD_LAUNCH_CHECK();
  hipLaunchKernelGGL((swin_ffn_wide_bwd_kernel<X, M, C>), dim3(groups), dim3(kWideBlock), 0, st, static_cast<const X*>(x),
                     static_cast<const X*>(dout), gamma, beta, stream, scale, rows_per_image, static_cast<X*>(dx), partial,
                     static_cast<M*>(xn), static_cast<M*>(act), static_cast<M*>(dhid), rows, eps);
  DHD_LAUNCH_CHECK();
  hipLaunchKernelGGL(swin_ffn_bwd_params, dim3(2 * C / 16), dim3(kParamBlock), 0, st, partial, dgamma, dbeta, (int)groups, C);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

// f(X*, M*) for the element types of the two dtype codes of a supported call
template <class F> int wide_train_dispatch(int x_dtype, int mm_dtype, F&& f) {
  return dhd::with_dtype<dhd::NativeHalf>(x_dtype, [&](auto* xp) {
    using X = std::remove_pointer_t<decltype(xp)>;
    return dhd::with_dtype<dhd::NativeHalf>(mm_dtype, [&](auto* mp) {
      using M = std::remove_pointer_t<decltype(mp)>;
      if constexpr (std::is_same_v<X, float> || std::is_same_v<X, M>) {
        return f(xp, mp);
      } else {
        return (int)DHD_EUNSUPPORTED;
      }
    });
  });
}

}  // namespace

extern "C" {

int dhdu_swin_ffn_wide_supported(int c, int hidden, int x_dtype, int mm_dtype) {
  return wide_train_supported(c, hidden, x_dtype, mm_dtype) ? 1 : 0;
}

size_t dhdu_swin_ffn_wide_forward_scratch_bytes(int c, int hidden, int mm_dtype) {
  if (!(c == 512 && hidden == 4 * c) || !dtype_code(mm_dtype)) return 0;
  return wide_scratch_bytes(c, mm_dtype);
}

size_t dhdu_swin_ffn_wide_backward_scratch_bytes(long rows, int c, int hidden, int mm_dtype) {
  if (!(c == 512 && hidden == 4 * c) || !dtype_code(mm_dtype) || rows <= 0 || rows > kWideMaxRows) return 0;
  return wide_train_packed_bytes(mm_dtype) + (size_t)wide_train_groups(rows, mm_dtype) * 2 * c * sizeof(float);
}

int dhdu_swin_ffn_wide_forward(const void* x, const float* gamma, const float* beta, const float* w1, const float* b1,
                               const float* w2, const float* b2, const float* scale, long rows_per_image, void* out, void* scratch,
                               size_t scratch_size, int x_dtype, int mm_dtype, long rows, int c, int hidden, float eps, void* stream) {
  if (!x || !gamma || !beta || !w1 || !b1 || !w2 || !b2 || !out || !scratch || rows <= 0) return DHD_EINVAL;
  if (!dhd_aligned(16, x, gamma, beta, w1, b1, w2, b2, scale, out, scratch)) return DHD_EINVAL;
  if (scale && (rows_per_image <= 0 || rows % rows_per_image != 0)) return DHD_EINVAL;
  if (!wide_train_supported(c, hidden, x_dtype, mm_dtype) || rows > kWideMaxRows) return DHD_EUNSUPPORTED;
  if (scratch_size < wide_scratch_bytes(c, mm_dtype)) return DHD_ENOSPACE;
  hipStream_t st = dhd_stream(stream);
  return wide_train_dispatch(x_dtype, mm_dtype, [&](auto* xp, auto* mp) {
    using X = std::remove_pointer_t<decltype(xp)>;
    using M = std::remove_pointer_t<decltype(mp)>;
    // without a factor this IS the wide inference operator: the same two launches, the same bytes
    if (!scale) return wide_launch<X, M, 512>(x, gamma, beta, w1, b1, w2, b2, out, scratch, rows, eps, st);
    return wide_launch<X, M, 512, ImageScale>(x, gamma, beta, w1, b1, w2, b2, out, scratch, rows, eps, st, ImageScale{scale, rows_per_image});
  });
}

int dhdu_swin_ffn_wide_backward(const void* x, const void* dout, const float* gamma, const float* beta, const float* w1,
                                const float* b1, const float* w2, const float* scale, long rows_per_image, void* dx, float* dgamma,
                                float* dbeta, void* xn, void* act, void* dhid, void* scratch, size_t scratch_size, int x_dtype,
                                int mm_dtype, long rows, int c, int hidden, float eps, void* stream) {
  if (!x || !dout || !gamma || !beta || !w1 || !b1 || !w2 || !dx || !dgamma || !dbeta || !scratch || rows <= 0) return DHD_EINVAL;
  if ((xn == nullptr) != (act == nullptr) || (xn == nullptr) != (dhid == nullptr)) return DHD_EINVAL;   // the operands: all or none
  if (!dhd_aligned(16, x, dout, gamma, beta, w1, b1, w2, scale, dx, dgamma, dbeta, xn, act, dhid, scratch)) return DHD_EINVAL;
  if (scale && (rows_per_image <= 0 || rows % rows_per_image != 0)) return DHD_EINVAL;
  if (!wide_train_supported(c, hidden, x_dtype, mm_dtype) || rows > kWideMaxRows) return DHD_EUNSUPPORTED;
  if (scratch_size < dhdu_swin_ffn_wide_backward_scratch_bytes(rows, c, hidden, mm_dtype)) return DHD_ENOSPACE;
  hipStream_t st = dhd_stream(stream);
  return wide_train_dispatch(x_dtype, mm_dtype, [&](auto* xp, auto* mp) {
    using X = std::remove_pointer_t<decltype(xp)>;
    using M = std::remove_pointer_t<decltype(mp)>;
    return wide_train_backward<X, M, 512>(x, dout, gamma, beta, w1, b1, w2, scale, rows_per_image, dx, dgamma, dbeta, xn, act, dhid,
                                          scratch, rows, eps, st);
  });
}

}  // extern "C"
