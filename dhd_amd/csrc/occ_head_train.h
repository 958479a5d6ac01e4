// Occupancy head in training (dhd_amd/capi/dhd_amd_occ_train.h): the backward of occ_head.hip's predicter MLP, recomputing the
// hidden tile instead of reading a saved one.  occ_head.hip includes this file after its own helpers: the constants, kParts,
// mfma16, pack_part, hid_unit, softplus and load_x are used as they are.  The forward in training IS dhd_occ_head_infer with
// pred = NULL and logits set: no kernel of its own, nothing of hidden size saved.
//
//   logits[cell] = W2 . softplus(W1 . x[cell] + b1) + b2,      g = dL/dlogits (float32, in the logits' cell order)
//
// The form is the forward's: one wave owns 32 cells of one sample from the loads to the store of their dx, the weights are on
// the MFMA A operand and the cells on B (column = lane & 31), nothing goes through LDS between the GEMMs.  A lane holds the
// channels 16 ks + 8 h + j of its cell's x and the logit columns 16 ks + 8 h + j of its cell's g; each, rounded once to the GEMM
// type T (or split in two bf16 parts for float32), is a B fragment as it lies.  Per hidden tile t of 32 units:
//   h_t  = W1_t . x + b1                      the forward's GEMM-1
//   da_t = W2[:, t]^T . g                     A rows are the units 32 t + r, k runs over the 288 logit columns (18 k-steps): the
//                                             result has h_t's register layout (register e = unit 8 (e >> 2) + 4 h + (e & 3))
//   a_t = softplus(h_t), dh_t = da_t s(h_t)   float32, in registers; s = sigmoid from softplus's own e = exp(-|h|)
//   dx  += W1[t, :]^T . dh_t                  A rows are dx_ch(r, n), k is hid_unit(t, s, h, j): dx lands in x's own layout
//                                             (register 8 s + j of tile n = channel 16 (2 n + s) + 8 h + j)
// The weight stream (pack_train_stream_kernel, once per call, nothing cached) holds per hidden tile
//   4 fragments     b1 of the tile as float32, register e of fragment f = b1[32 t + 8 f + 4 h + e]
//   16 * P          h:   k-step ks, part p: W1[32 t + r][16 ks + 8 h + j]
//   18 * P          da:  k-step ks, part p: W2[16 ks + 8 h + j][32 t + r]
//   2 * 8 * P       dx:  k-step s, output tile n, part p: W1[hid_unit(t, s, h, j)][dx_ch(r, n)]
// and is read through the forward's ring, with the forward's padding behind it (kScratchBytes).  With float32 GEMMs every
// product is the three bf16 products of the forward, smallest terms first.
//
// dx is rounded once to x's type and stored in x's layout: 16-byte vectors along the channels of a channels_last x, one element
// per channel of an NCHW x (32 consecutive cells per store instruction).  db1 = sum_cells dh and db2 = sum_cells g (float32, of
// the unrounded values): the 32 cells of a wave are added by a butterfly that halves the register count with every exchange,
// the four waves of a workgroup in a fixed order through LDS, and the per-workgroup rows of 800 floats in scratch by a second
// launch in a fixed order.  No atomics: the same bytes in give the same bytes out.
//
// The weight gradients are reductions over cells and stay with the caller's GEMMs; on request the kernel writes their operands
//   act  (cells, 512) = a,  in T, in the LOGITS' cell order (b, ix, iy): dW2 = g^T . act
//   dhid (cells, 512) = dh, in T, in x's PIXEL order (b, iy, ix):        dW1 = dhid^T . x
//   ghalf (cells, 288) = g rounded once to a half T, in g's own order (with float32 GEMMs g itself is the operand)
// A lane holds 4 consecutive units per register quad: 16 bytes of float32, stored as they lie; of a half type two quads are
// paired with the other half of the cell (lane ^ 32, one v_permlane32_swap per word) into one 16-byte store.  All of them are
// plain global stores under the lane's own predicate: no buffer store, so nothing for store_b128_guarded to guard.
//
// A lane past the sample computes on the sample's last cell, as in the forward; its g is taken as zero, its terms of db1 and
// db2 are selected to zero (not multiplied: the last cell may hold a NaN), and it stores no operand row and no dx.
//
// One wave per SIMD, up to 512 registers, no private memory in any instantiation:
//   half GEMMs (f16, bf16; NCHW and channels_last)   KEEP: the x fragments (64 registers) and the g fragments (72) stay in
//                                                    registers for all 16 tiles beside dx (128) and the ring (18 fragments)
//   float32 GEMMs (NCHW and channels_last)           RELOAD: two bf16 parts of each do not fit beside dx; dx is kept and the B
//                                                    fragments of the h and da GEMMs are loaded and split again per k-step of
//                                                    every tile (out of L2), as swin_ffn_train.h's BKEEP = false does
#pragma once
// (../capi/dhd_amd_occ_train.h declares the entry points at the end of this file; like swin_ffn_wide_train.h's header it names
// dhd_amd.h without a directory and is not included here: tests/test_occ_head_train_capi.py holds the two to each other.)

namespace {

constexpr int kGS = kCols / 16;            // 18 k-steps of the da GEMM
constexpr int kXT = kC / 32;               // 8 output tiles of the dx GEMM
constexpr int kSums = kHidden + kCols;     // 800: db1, then db2
constexpr int kParamBlock = 256;           // db1 / db2: 16 lanes down the partial rows x 16 columns

template <class T> constexpr int kTrainFrags = 4 + (kKS + kGS + 2 * kXT) * kParts<T>;   // fragments per hidden tile: 104 / 54
template <class T> constexpr int kTrainRing = std::is_same_v<T, float> ? 13 : 18;       // divides kTrainFrags<T>
template <class T> constexpr size_t kTrainStreamBytes = (size_t)kHT * kTrainFrags<T> * 1024;
template <class T> constexpr size_t kTrainPackedBytes = kTrainStreamBytes<T> + (size_t)kTrainRing<T> * 1024;   // as kScratchBytes

// channel of x of MFMA row r of output tile n of the dx GEMM: register 8 s + j of lane half h is channel 16 (2 n + s) + 8 h + j
__host__ __device__ constexpr int dx_ch(int r, int n) { return 32 * n + 16 * (r >> 4) + 8 * ((r >> 2) & 1) + 4 * ((r >> 3) & 1) + (r & 3); }

// one thread per (hidden tile, fragment, lane): 16 bytes of the backward's stream
template <class T>
__global__ __launch_bounds__(kPackBlock) void pack_train_stream_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                                                       const float* __restrict__ w2, u32x4* __restrict__ stream) {
  constexpr int P = kParts<T>, N = kTrainFrags<T>;
  const int idx = blockIdx.x * kPackBlock + threadIdx.x;
  if (idx >= kHT * N * 64) return;
  const int lane = idx & 63, r = lane & 31, h = lane >> 5;
  const int f = (idx >> 6) % N, t = (idx >> 6) / N;
  float v[8];
  u32x4 out;
  if (f < 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = __float_as_uint(b1[32 * t + 8 * f + 4 * h + e]);
    stream[idx] = out;
    return;
  }
  int part;
  if (f < 4 + kKS * P) {
    const int ks = (f - 4) / P;
    part = (f - 4) % P;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w1[(size_t)(32 * t + r) * kC + 16 * ks + 8 * h + j];
  } else if (f < 4 + (kKS + kGS) * P) {
    const int g = f - 4 - kKS * P, ks = g / P;
    part = g % P;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w2[(size_t)(16 * ks + 8 * h + j) * kHidden + 32 * t + r];
  } else {
    const int g = f - 4 - (kKS + kGS) * P, n = (g / P) % kXT, s = g / (P * kXT);
    part = g % P;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w1[(size_t)hid_unit(t, s, h, j) * kC + dx_ch(r, n)];
  }
  stream[idx] = pack_part<T>(v, part);
}

// a = softplus(x) as the forward gives it, s = its derivative, the logistic function, from the same e = exp(-|x|): 1 / (1 + e)
// for x >= 0 and e / (1 + e) below (1 ulp of the hardware rcp on top of e's 2).  torch's rule holds: above the threshold of 20
// the derivative is 1 (1 + exp(-20) rounds to 1 anyway; the select says so).  |x| is clamped as in softplus, so +-inf give 1 and
// 0.  A NaN goes through both: a by softplus's select, s by the select below (fminf would have clamped it away).
__device__ __forceinline__ void softplus_grad(float x, float& a, float& s) {
  constexpr float kLog2eHi = 1.44269502162933349609375f, kLog2eLo = 1.92596299e-8f, kLn2 = 0.693147182464599609375f;
  a = softplus(x);
  const float m = -fminf(fabsf(x), 100.f);   // softplus's own terms, operation for operation: one copy after inlining
  const float hi = m * kLog2eHi;
  const float lo = fmaf(m, kLog2eLo, fmaf(m, kLog2eHi, -hi));
  const float eh = __builtin_amdgcn_exp2f(hi);
  const float e = fmaf(eh, lo * kLn2, eh);
  const float rc = __builtin_amdgcn_rcpf(1.f + e);
  const float sg = x > 20.f ? 1.f : (x < 0.f ? e * rc : rc);
  s = x != x ? x : sg;
}

// eight consecutive-k values -> the B fragment parts
template <class T> __device__ __forceinline__ void make_parts(const float* v, u32x4 (&parts)[kParts<T>]) {
#pragma unroll
  for (int p = 0; p < kParts<T>; ++p) parts[p] = pack_part<T>(v, p);
}

// 4 consecutive values rounded to T, stored as they lie: 16 bytes of float32, 8 of a half type
template <class T> __device__ __forceinline__ void store4(T* dst, const float* v) {
  if constexpr (std::is_same_v<T, float>) {
    *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
    *reinterpret_cast<u32x2*>(dst) = u32x2{Pair<T>::narrow(f32x2{v[0], v[1]}), Pair<T>::narrow(f32x2{v[2], v[3]})};
  }
}

// Two neighbouring register quads of a half type (units 8 k + 4 h + (0..3) and 8 (k + 1) + 4 h + (0..3) of a cell that the lanes
// r and r + 32 share) after one half exchange per word (v_permlane32_swap): the lower lane holds units 8 k .. 8 k + 7, the upper
// lane 8 (k + 1) .. 8 (k + 1) + 7 -- 16 contiguous bytes each.  Every lane of the wave must take part.  (swin_ffn_train.h's.)
template <class T> __device__ __forceinline__ u32x4 pair_quads(const float* v) {
  unsigned w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = Pair<T>::narrow(f32x2{v[2 * i], v[2 * i + 1]});
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
// both lanes of an exchange hold the same sums and the order of the additions is fixed.  (swin_ffn_train.h's.)
__device__ __forceinline__ float col_sums16(float* v, int r) {
  fold_step<16, 8>(v, r);
  fold_step<8, 4>(v, r);
  fold_step<4, 2>(v, r);
  fold_step<2, 1>(v, r);
  return v[0] + __shfl_xor(v[0], 1, DHD_WAVE);
}

// The x fragment of one k-step, for the RELOAD form: load_x's loads and splits for k-step ks alone.  voff is load_x's per-lane
// byte offset (plus a zero the compiler cannot see through, which keeps the loads inside the tile loop).
template <class T, bool NHWC>
__device__ __forceinline__ void load_x_step(__amdgpu_buffer_rsrc_t rx, int voff, int ks, int hw, u32x4 (&parts)[kParts<T>]) {
  static_assert(std::is_same_v<T, float>, "only the float32 instantiations reload");
  float v[8];
  if constexpr (NHWC) {
    const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(rx, voff, ks * 64, 0);
    const u32x4 b = __builtin_amdgcn_raw_buffer_load_b128(rx, voff, ks * 64 + 16, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = __uint_as_float(a[j]);
      v[4 + j] = __uint_as_float(b[j]);
    }
  } else {
    const int row = hw * 4;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, voff, (16 * ks + j) * row, 0));
  }
  make_parts<T>(v, parts);
}

template <class T, bool NHWC>
__global__ __launch_bounds__(kBlock) void occ_head_bwd_kernel(const T* __restrict__ x, const u32x4* __restrict__ stream,
                                                              const float* __restrict__ glogits, int dy, int dx, T* __restrict__ dx_out,
                                                              float* __restrict__ partial, T* __restrict__ act_out,
                                                              T* __restrict__ dhid_out, T* __restrict__ ghalf_out) {
  constexpr int P = kParts<T>, N = kTrainFrags<T>, R = kTrainRing<T>, E = sizeof(T);
  constexpr bool KEEP = P == 1;   // see the header comment: the half instantiations keep x and g, the float32 ones reload them
  static_assert(N % R == 0, "the ring position of a fragment must not depend on the hidden tile");
  __shared__ float red[kBlock / 64][kSums];   // per wave: sum_cells dh (512), sum_cells g (288)
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, hw = dy * dx;
  const int p0 = (blockIdx.x * (kBlock / 64) + (tid >> 6)) * 32;   // wave-uniform
  float* myred = red[tid >> 6];
  if (p0 >= hw) {   // a wave past the sample adds nothing
    for (int i = lane; i < kSums; i += 64) myred[i] = 0.f;
  } else {
    const bool live = p0 + r < hw;   // a lane past the sample computes on its last cell, stores nothing and adds nothing
    const int p = live ? p0 + r : hw - 1;
    const int iy = p / dx, ix = p - iy * dx;
    const size_t cell = ((size_t)b * dx + ix) * dy + iy;   // the logits' order: the reference's permute(0, 3, 2, 1)
    const size_t pixel = (size_t)b * hw + p;               // x's order
    const bool ops = act_out != nullptr;                   // uniform over the launch: act and dhid, or neither
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(x + (size_t)b * kC * hw), 0,
                                                                        (unsigned)((size_t)kC * hw * sizeof(T)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(stream), 0, (unsigned)kTrainPackedBytes<T>, 0x00020000);
    u32x4 ring[R];
    const int lane_off = lane * 16;
    static_for<R>([&](auto i) { ring[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, i * 1024, 0); });

    u32x4 xf[KEEP ? kKS : 1][P], gf[KEEP ? kGS : 1][P];
    if constexpr (KEEP) {
      load_x<T, NHWC>(rx, p, h, hw, xf);
      // an NCHW x arrives as 256 two-byte loads: they are packed into their 64 registers before the loads of g are issued
      __builtin_amdgcn_sched_barrier(0);
    }
    const int xoff = NHWC ? (p * kC + 8 * h) * E : (p + 8 * h * hw) * E;   // load_x's per-lane offset

    // g: the logit columns 16 ks + 8 h + j of this lane's cell, zero in a lane past the sample.  One pass over all of it for
    // db2, ghalf and (KEEP) the B fragments of the da GEMM.
    const float* grow = glogits + cell * kCols + 8 * h;
    auto load_g = [&](int ks, float* v, int off) {
      const f32x4* gp = reinterpret_cast<const f32x4*>(grow + off + 16 * ks);
      const f32x4 g0 = gp[0], g1 = gp[1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = live ? g0[j] : 0.f;
        v[4 + j] = live ? g1[j] : 0.f;
      }
    };
#pragma unroll
    for (int m = 0; m < kGS / 2; ++m) {
      float v[16];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int ks = 2 * m + s;
        load_g(ks, v + 8 * s, 0);
        if constexpr (KEEP) {
          make_parts<T>(v + 8 * s, gf[ks]);
          if (ghalf_out && live) *reinterpret_cast<u32x4*>(ghalf_out + cell * kCols + 8 * h + 16 * ks) = gf[ks][0];
        }
      }
      const float total = col_sums16(v, r);   // of v[r >> 1]: column 16 (2 m + (i >> 3)) + 8 h + (i & 7), i = r >> 1
      if ((r & 1) == 0) myred[kHidden + 16 * (2 * m + (r >> 4)) + 8 * h + ((r >> 1) & 7)] = total;
    }

    f32x16 acc[kXT];
#pragma unroll
    for (int n = 0; n < kXT; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[n][e] = 0.f;

    T* arow = act_out + cell * kHidden;
    T* drow = dhid_out + pixel * kHidden;
    for (int t = 0; t < kHT; ++t) {
      const int base = t * (N * 1024);
      auto take = [&](auto I) {   // fragment I out of the ring, its slot refilled at once (see occ_head_kernel)
        constexpr int i = decltype(I)::value;
        const u32x4 v = ring[i % R];
        ring[i % R] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, base + (i + R) * 1024, 0);
        __builtin_amdgcn_sched_barrier(0);
        return v;
      };
      // three products of the two-part operands, smallest terms first, or the one product of the rounded ones
      auto gemm_step = [&](auto I0, const u32x4 (&bf)[P], f32x16 c) {
        constexpr int i0 = decltype(I0)::value;
        if constexpr (P == 2) {
          const u32x4 wh = take(std::integral_constant<int, i0>{});
          const u32x4 wm = take(std::integral_constant<int, i0 + 1>{});
          c = mfma16<T>(wm, bf[0], c);
          c = mfma16<T>(wh, bf[P - 1], c);
          return mfma16<T>(wh, bf[0], c);
        } else {
          return mfma16<T>(take(std::integral_constant<int, i0>{}), bf[0], c);
        }
      };
      int tz = 0;   // zero, opaque per tile: what keeps the reloads of the RELOAD form inside the loop
      if constexpr (!KEEP) asm volatile("" : "+v"(tz));
      f32x16 hid, da;
      static_for<4>([&](auto F) {
        const u32x4 v = take(F);
#pragma unroll
        for (int e = 0; e < 4; ++e) hid[4 * F + e] = __uint_as_float(v[e]);
      });
#pragma unroll
      for (int e = 0; e < 16; ++e) da[e] = 0.f;
      static_for<kKS>([&](auto KSI) {
        constexpr int ks = decltype(KSI)::value;
        if constexpr (!KEEP) load_x_step<T, NHWC>(rx, xoff + tz, ks, hw, xf[0]);
        hid = gemm_step(std::integral_constant<int, 4 + ks * P>{}, xf[KEEP ? ks : 0], hid);
      });
      static_for<kGS>([&](auto KSI) {
        constexpr int ks = decltype(KSI)::value;
        if constexpr (!KEEP) {
          float v[8];
          load_g(ks, v, tz);
          make_parts<T>(v, gf[0]);
        }
        da = gemm_step(std::integral_constant<int, 4 + (kKS + ks) * P>{}, gf[KEEP ? ks : 0], da);
      });
      float a[16], d[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float sg;
        softplus_grad(hid[e], a[e], sg);
        d[e] = da[e] * sg;
      }
      if constexpr (!std::is_same_v<T, float>) {
        if (ops) {
#pragma unroll
          for (int m = 0; m < 2; ++m) {   // quads 2 m and 2 m + 1 -> units 32 t + 16 m + 8 h + (0..7): one 16-byte store
            const u32x4 wa = pair_quads<T>(a + 8 * m), wd = pair_quads<T>(d + 8 * m);
            if (live) {
              *reinterpret_cast<u32x4*>(arow + 32 * t + 16 * m + 8 * h) = wa;
              *reinterpret_cast<u32x4*>(drow + 32 * t + 16 * m + 8 * h) = wd;
            }
          }
        }
      } else if (ops && live) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {   // register quad q = units 32 t + 8 q + 4 h + (0..3)
          store4<T>(arow + 32 * t + 8 * q + 4 * h, a + 4 * q);
          store4<T>(drow + 32 * t + 8 * q + 4 * h, d + 4 * q);
        }
      }
      u32x4 df[2][P];
#pragma unroll
      for (int s = 0; s < 2; ++s) make_parts<T>(d + 8 * s, df[s]);
      // db1's terms of this tile, in place: d is dead after its fragments are made
#pragma unroll
      for (int e = 0; e < 16; ++e) d[e] = live ? d[e] : 0.f;
      const float total = col_sums16(d, r);   // of d[r >> 1]: unit 32 t + 8 (i >> 2) + 4 h + (i & 3), i = r >> 1
      if ((r & 1) == 0) myred[32 * t + 8 * (r >> 3) + 4 * h + ((r >> 1) & 3)] = total;
      static_for<2 * kXT>([&](auto GI) {
        constexpr int g = decltype(GI)::value, s = g / kXT, n = g % kXT;
        acc[n] = gemm_step(std::integral_constant<int, 4 + (kKS + kGS + g) * P>{}, df[s], acc[n]);
      });
    }

    // register 8 s + j of tile n = dx of channel 16 (2 n + s) + 8 h + j of this lane's cell
    if (live) {
      if constexpr (NHWC) {
        T* orow = dx_out + pixel * kC + 8 * h;
#pragma unroll
        for (int n = 0; n < kXT; ++n)
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = acc[n][8 * s + j];
            raw16<T>* q = reinterpret_cast<raw16<T>*>(orow + 16 * (2 * n + s));
#pragma unroll
            for (int w = 0; w < 8 / kVec16<T>; ++w) q[w] = narrow16<T>(o + w * kVec16<T>);
          }
      } else {
        T* ocol = dx_out + ((size_t)b * kC + 8 * h) * hw + p;
#pragma unroll
        for (int n = 0; n < kXT; ++n)
#pragma unroll
          for (int e = 0; e < 16; ++e) ocol[(size_t)(16 * (2 * n + (e >> 3)) + (e & 7)) * hw] = (T)acc[n][e];
      }
    }
  }
  __syncthreads();
  // the workgroup's partial row: its four waves in a fixed order
  float* prow = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kSums;
  for (int i = tid; i < kSums; i += kBlock) prow[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// partial (groups, 800) -> db1 (512), db2 (288).  A workgroup owns 16 columns: 16 lanes walk down the rows, each adding every
// 16th row in order, then lane 0 of a column adds the 16 sums in order.
__global__ __launch_bounds__(kParamBlock) void occ_head_bwd_params(const float* __restrict__ partial, float* __restrict__ db1,
                                                                   float* __restrict__ db2, int groups) {
  __shared__ float sums[16][17];
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4, col = blockIdx.x * 16 + cl;
  float a = 0.f;
#pragma unroll 4
  for (int g = rl; g < groups; g += 16) a += partial[(size_t)g * kSums + col];
  sums[rl][cl] = a;
  __syncthreads();
  if (rl == 0) {
    float t = sums[0][cl];
    for (int i = 1; i < 16; ++i) t += sums[i][cl];
    if (col < kHidden) db1[col] = t;
    else db2[col - kHidden] = t;
  }
}

size_t train_packed_bytes(int x_dtype) { return x_dtype == DHD_F32 ? kTrainPackedBytes<float> : kTrainPackedBytes<__bf16>; }

// one sample of x behind a 32-bit buffer descriptor, byte offsets in an int; grid.y (dhd_occ_head_infer's limits)
bool train_size_supported(int b, int dy, int dx) { return (size_t)dy * dx <= ((size_t)1 << 30) / (kC * 4) && b <= 65535; }

int train_groups(int b, int dy, int dx) { return b * dhd_cdiv((long)dy * dx, kCellsPerBlock); }

template <class T, bool NHWC>
int launch_backward(const void* x, const dhd_occ_head_weights* w, int b, int dy, int dx, const float* glogits, void* dx_out, float* db1,
                    float* db2, void* act, void* dhid, void* ghalf, void* scratch, hipStream_t st) {
  u32x4* stream = static_cast<u32x4*>(scratch);
  float* partial = reinterpret_cast<float*>(static_cast<char*>(scratch) + kTrainPackedBytes<T>);
  constexpr int n_pack = kHT * kTrainFrags<T> * 64;
  hipLaunchKernelGGL(pack_train_stream_kernel<T>, dim3(dhd_cdiv(n_pack, kPackBlock)), dim3(kPackBlock), 0, st, w->w1, w->b1, w->w2, stream);
  DHD_LAUNCH_CHECK();
  hipLaunchKernelGGL((occ_head_bwd_kernel<T, NHWC>), dim3(dhd_cdiv((long)dy * dx, kCellsPerBlock), b), dim3(kBlock), 0, st,
                     static_cast<const T*>(x), stream, glogits, dy, dx, static_cast<T*>(dx_out), partial, static_cast<T*>(act),
                     static_cast<T*>(dhid), static_cast<T*>(ghalf));
  DHD_LAUNCH_CHECK();
  hipLaunchKernelGGL(occ_head_bwd_params, dim3(kSums / 16), dim3(kParamBlock), 0, st, partial, db1, db2, train_groups(b, dy, dx));
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

}  // namespace

extern "C" {

int dhdo_occ_head_backward_supported(int c, int hidden, int dz, int n_classes, int x_dtype, int layout) {
  return dhd_occ_head_infer_supported(c, hidden, dz, n_classes, x_dtype, layout, DHD_SFA_GEMM_DEFAULT);
}

int dhdo_occ_head_backward_scratch_bytes(const dhd_occ_head_weights* w, int x_dtype, int b, int dy, int dx, size_t* bytes) {
  if (!w || !bytes) return DHD_EINVAL;
  *bytes = 0;
  if (b <= 0 || dy <= 0 || dx <= 0) return DHD_EINVAL;
  if (x_dtype != DHD_F32 && x_dtype != DHD_F16 && x_dtype != DHD_BF16) return DHD_EINVAL;
  if (!shape_supported(w->c, w->hidden, w->dz, w->n_classes) || !precision_supported(x_dtype, 0, w->gemm)) return DHD_EUNSUPPORTED;
  if (!train_size_supported(b, dy, dx)) return DHD_EUNSUPPORTED;
  *bytes = train_packed_bytes(x_dtype) + (size_t)train_groups(b, dy, dx) * kSums * sizeof(float);
  return DHD_OK;
}

int dhdo_occ_head_backward(const void* x, int x_dtype, int layout, const dhd_occ_head_weights* w, int b, int dy, int dx,
                           const float* glogits, void* dx_out, float* db1, float* db2, void* act, void* dhid, void* ghalf, void* scratch,
                           size_t scratch_bytes, void* stream) {
  if (!x || !w || !w->w1 || !w->b1 || !w->w2 || !glogits || !dx_out || !db1 || !db2 || !scratch || b <= 0 || dy <= 0 || dx <= 0)
    return DHD_EINVAL;
  if (x_dtype != DHD_F32 && x_dtype != DHD_F16 && x_dtype != DHD_BF16) return DHD_EINVAL;
  if ((act == nullptr) != (dhid == nullptr)) return DHD_EINVAL;          // the two hidden operands: both or neither
  if (ghalf && (x_dtype == DHD_F32 || !act)) return DHD_EINVAL;          // with float32 GEMMs glogits itself is the operand
  if (!dhd_aligned(16, x, w->w1, w->b1, w->w2, glogits, dx_out, db1, db2, act, dhid, ghalf, scratch)) return DHD_EINVAL;
  if (!dhd_occ_head_infer_supported(w->c, w->hidden, w->dz, w->n_classes, x_dtype, layout, w->gemm)) return DHD_EUNSUPPORTED;
  if (!train_size_supported(b, dy, dx)) return DHD_EUNSUPPORTED;
  if (scratch_bytes < train_packed_bytes(x_dtype) + (size_t)train_groups(b, dy, dx) * kSums * sizeof(float)) return DHD_ENOSPACE;
  hipStream_t st = dhd_stream(stream);
  return dhd::with_dtype<dhd::NativeHalf>(x_dtype, [&](auto* tp) {
    using T = std::remove_pointer_t<decltype(tp)>;
    return layout ? launch_backward<T, true>(x, w, b, dy, dx, glogits, dx_out, db1, db2, act, dhid, ghalf, scratch, st)
                  : launch_backward<T, false>(x, w, b, dy, dx, glogits, dx_out, db1, db2, act, dhid, ghalf, scratch, st);
  });
}

}  // extern "C"
