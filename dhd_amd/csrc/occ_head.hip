// Occupancy head at inference: predicter MLP -> class map in one kernel (section 14 of dhd_amd.h).
//
//   logits[cell][z*18 + k] = W2 . softplus(W1 . x[cell] + b1) + b2,   pred[cell][z] = first-maximum argmax_k
//
// Reference: models/dense_heads/occ_head.py:84-100 (predictor.forward after final_conv) and :141-153 (get_occ); the histogram is
// Metric_mIoU.hist_info as in occ_loss.hip.  Neither the (cells x 512) hidden nor the (cells x 288) logits exist in memory.
//
// One wave owns 32 BEV cells from the load of x to the store of their 16 class bytes; the waves of a block share nothing but
// the LDS histogram.  Both GEMMs put the WEIGHTS on the MFMA A operand (rows = output units) and the cells on the B operand
// (column = lane & 31), so that
//   * x is split once into B fragments that stay in registers for all 16 hidden tiles,
//   * a 32-unit hidden tile comes out of GEMM-1 with its cell on the lane and its units in the 16 registers, which after bias,
//     Softplus and the split IS the B operand of two k-steps of GEMM-2 (no lane movement, no LDS): element j of lane half h of
//     k-step s is unit 8 (2s + (j >> 2)) + 4h + (j & 3) of the tile, and W2's k order is permuted to match when it is packed,
//   * W2's rows are permuted so that lane half h of a cell ends with z = 8h .. 8h+7 complete: register e of output tile n is
//     logit column 144 h + 16 n + e, and the 18-way argmax per z is register-only.
// The weights reach a wave as one linear stream of 1 KiB fragments (16 bytes per lane) in the order of their use, prepared in
// `scratch` by pack_stream_kernel once per call and L2-resident after the first waves; a ring of kRing fragments is loaded
// ahead of the MFMAs that consume them.  Per hidden tile t the stream holds
//   4 fragments     b1 of the tile as float32, register e of fragment f = b1[32 t + 8 f + 4 h + e]
//   16 * P          GEMM-1, k-step ks, part p: W1[32 t + r][16 ks + 8 h + j]
//   2 * 9 * P       GEMM-2, k-step s, output tile n, part p: W2[col(r, n)][unit(t, s, h, j)]
// with P = 2 bf16 parts (high, residual) of a float32 weight, or P = 1 weight rounded to the half type of x.
#include "sfa_mfma.h"
#include "occ_loss_math.h"

namespace {

using namespace dhd_sfa;

constexpr int kC = 256, kHidden = 512, kDz = 16, kClasses = 18;
constexpr int kCols = kDz * kClasses;      // 288 logits per cell
constexpr int kNT = kCols / 32;            // 9 output tiles of GEMM-2
constexpr int kHT = kHidden / 32;          // 16 hidden tiles
constexpr int kKS = kC / 16;               // 16 k-steps of GEMM-1
constexpr int kBlock = 256;                // 4 waves = 128 cells; one wave per SIMD (the kernel needs more than 256 registers)
constexpr int kCellsPerBlock = kBlock / 64 * 32;
constexpr int kPackBlock = 256;

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

template <class T> constexpr int kParts = std::is_same_v<T, float> ? 2 : 1;
template <class T> constexpr int kFrags = 4 + (kKS + 2 * kNT) * kParts<T>;   // fragments per hidden tile: 72 / 38
template <class T> constexpr int kRing = std::is_same_v<T, float> ? 18 : 19; // divides kFrags<T>: static ring positions
template <class T> constexpr size_t kStreamBytes = (size_t)kHT * kFrags<T> * 1024;
// The ring runs kRing fragments ahead of its consumer to the very end, so the last refills read past the last fragment.  Their
// address is carried in the scalar offset of the buffer load, which the hardware range check does not look at: the bytes must
// exist.  `scratch` therefore ends with kRing KiB that are read and never used (nor written: any bit pattern will do).
template <class T> constexpr size_t kScratchBytes = kStreamBytes<T> + (size_t)kRing<T> * 1024;

// logit column of MFMA row r of output tile n, and hidden unit of element j of lane half h of k-step s of hidden tile t
__host__ __device__ constexpr int out_col(int r, int n) { return 144 * ((r >> 2) & 1) + 16 * n + 4 * (r >> 3) + (r & 3); }
__host__ __device__ constexpr int hid_unit(int t, int s, int h, int j) { return 32 * t + 8 * (2 * s + (j >> 2)) + 4 * h + (j & 3); }

template <class T> __device__ __forceinline__ f32x16 mfma16(u32x4 a, u32x4 b, f32x16 c) {
  if constexpr (std::is_same_v<T, _Float16>)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return mfma_bf16(a, b, c);
}

// eight consecutive-k weights -> the fragment words of part `part`
template <class T> __device__ __forceinline__ u32x4 pack_part(const float* v, int part) {
  u32x4 w;
#pragma unroll
  for (int jp = 0; jp < 4; ++jp) {
    if constexpr (std::is_same_v<T, float>) {
      unsigned h, m;
      split2_hm(v[2 * jp], v[2 * jp + 1], h, m);
      w[jp] = part ? m : h;
    } else {
      w[jp] = Pair<T>::narrow(f32x2{v[2 * jp], v[2 * jp + 1]});
    }
  }
  return w;
}

// one thread per (hidden tile, fragment, lane): 16 bytes of the stream
template <class T>
__global__ __launch_bounds__(kPackBlock) void pack_stream_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                                                 const float* __restrict__ w2, u32x4* __restrict__ stream) {
  constexpr int P = kParts<T>, N = kFrags<T>;
  const int idx = blockIdx.x * kPackBlock + threadIdx.x;
  if (idx >= kHT * N * 64) return;
  const int lane = idx & 63, r = lane & 31, h = lane >> 5;
  const int f = (idx >> 6) % N, t = (idx >> 6) / N;
  float v[8];
  u32x4 out;
  if (f < 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = __float_as_uint(b1[32 * t + 8 * f + 4 * h + e]);
  } else if (f < 4 + kKS * P) {
    const int ks = (f - 4) / P, part = (f - 4) % P;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w1[(size_t)(32 * t + r) * kC + 16 * ks + 8 * h + j];
    out = pack_part<T>(v, part);
  } else {
    const int g = f - 4 - kKS * P;
    const int part = g % P, n = (g / P) % kNT, s = g / (P * kNT);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w2[(size_t)out_col(r, n) * kHidden + hid_unit(t, s, h, j)];
    out = pack_part<T>(v, part);
  }
  stream[idx] = out;
}

// Softplus (beta 1) as max(x, 0) + log1p(exp(-|x|)), branch-free on the hardware exp2 / log2 / rcp (1 ulp each): the library
// expf + log1pf pair costs ~135 instructions per value, more VALU time than the MFMAs it sits between.  torch's rule (the
// value itself above 20) holds to the last bit: exp(-20) = 2e-9 is below half an ulp of 20.
//   e = exp(-|x|):  the exponent -|x| log2(e) is carried in two floats (product error recovered by fma), ~2 ulp
//   log1p(e), 0 <= e <= 1:  e < 2^-5: the alternating series to e^5 (truncation < e^5 / 6 = 5e-9 relative);
//                           else log(u) e / (u - 1) with u = fl(1 + e), which cancels the rounding of 1 + e
// |x| is clamped to 100 (e = 0 there) so that +-inf give inf / 0 and not inf - inf.  A NaN goes through as torch's does: the
// first term is a select that keeps it (fmaxf would return the 0), and the second term is finite.
__device__ __forceinline__ float softplus(float x) {
  constexpr float kLog2eHi = 1.44269502162933349609375f, kLog2eLo = 1.92596299e-8f, kLn2 = 0.693147182464599609375f;
  const float a = -fminf(fabsf(x), 100.f);
  const float hi = a * kLog2eHi;
  const float lo = fmaf(a, kLog2eLo, fmaf(a, kLog2eHi, -hi));
  const float eh = __builtin_amdgcn_exp2f(hi);
  const float e = fmaf(eh, lo * kLn2, eh);
  const float u = 1.f + e;
  const float big = (__builtin_amdgcn_logf(u) * kLn2) * (e * __builtin_amdgcn_rcpf(u - 1.f));
  const float small = e * fmaf(-e, fmaf(-e, fmaf(-e, fmaf(-e, 0.2f, 0.25f), 1.f / 3.f), 0.5f), 1.f);
  return (x < 0.f ? 0.f : x) + (e < 0.03125f ? small : big);
}

// x fragments of one wave: xf[ks][part] = elements 16 ks + 8 h + j of cell p.  `rx` spans one sample and p must lie inside it:
// the channel term travels in the scalar offset, which the buffer range check does not cover.
template <class T, bool NHWC>
__device__ __forceinline__ void load_x(__amdgpu_buffer_rsrc_t rx, int p, int h, int hw, u32x4 (&xf)[kKS][kParts<T>]) {
  constexpr int E = sizeof(T);
  if constexpr (NHWC) {
    const int voff = (p * kC + 8 * h) * E;
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) {
      if constexpr (std::is_same_v<T, float>) {
        const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(rx, voff, ks * 64, 2);
        const u32x4 b = __builtin_amdgcn_raw_buffer_load_b128(rx, voff, ks * 64 + 16, 2);
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) {
          const u32x4 q = jp < 2 ? a : b;
          unsigned hi, mid;
          split2_hm(__uint_as_float(q[2 * (jp & 1)]), __uint_as_float(q[2 * (jp & 1) + 1]), hi, mid);
          xf[ks][0][jp] = hi;
          xf[ks][1][jp] = mid;
        }
      } else {
        xf[ks][0] = __builtin_amdgcn_raw_buffer_load_b128(rx, voff, ks * 32, 2);
      }
    }
  } else {
    const int voff = (p + 8 * h * hw) * E;
    const int row = hw * E;
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) {
      if constexpr (std::is_same_v<T, float>) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, voff, (16 * ks + j) * row, 2));
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) {
          unsigned hi, mid;
          split2_hm(v[2 * jp], v[2 * jp + 1], hi, mid);
          xf[ks][0][jp] = hi;
          xf[ks][1][jp] = mid;
        }
      } else {
        unsigned v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rx, voff, (16 * ks + j) * row, 2);
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) xf[ks][0][jp] = v[2 * jp] | (v[2 * jp + 1] << 16);
      }
    }
  }
}

// the loss epilogue of occ_head_kernel<T, NHWC, true> (occ_head_loss.h)
__device__ __forceinline__ void loss_terms(const f32x16 (&acc)[kNT], u32x2 lab, u32x2 msk, const float* __restrict__ cw, int ignore,
                                           float (&sum)[kLossSums]);
__device__ __forceinline__ void loss_row(float (&sum)[kLossSums], float (*red)[kLossSums], float* __restrict__ row);

// LOSS (occ_head_loss.h): beside the logits, the workgroup's row of the 56 loss sums of its valid voxels -> loss_partial; labels
// and mask are then required, class_weight and ignore are the loss's.  Without it the three trailing arguments are not read.
template <class T, bool NHWC, bool LOSS = false>
__global__ __launch_bounds__(kBlock) void occ_head_kernel(const T* __restrict__ x, const u32x4* __restrict__ stream,
                                                          const float* __restrict__ b2, int dy, int dx, uint8_t* __restrict__ pred,
                                                          float* __restrict__ logits, const uint8_t* __restrict__ labels,
                                                          const uint8_t* __restrict__ mask, unsigned long long* __restrict__ hist,
                                                          const float* __restrict__ class_weight, int ignore,
                                                          float* __restrict__ loss_partial) {
  constexpr int P = kParts<T>, N = kFrags<T>, R = kRing<T>;
  static_assert(N % R == 0, "the ring position of a fragment must not depend on the hidden tile");
  __shared__ unsigned cnt[kClasses * kClasses];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, hw = dy * dx;
  const int p0 = (blockIdx.x * (kBlock / 64) + (tid >> 6)) * 32;   // wave-uniform
  if (hist) {
    for (int i = tid; i < kClasses * kClasses; i += kBlock) cnt[i] = 0;
    __syncthreads();
  }
  [[maybe_unused]] float lsum[LOSS ? kLossSums : 1];
  if constexpr (LOSS) {
#pragma unroll
    for (int i = 0; i < kLossSums; ++i) lsum[i] = 0.f;   // a wave or a lane past the sample adds nothing
  }
  if (p0 < hw) {
    const int p = p0 + r;
    const bool live = p < hw;   // a lane past the sample computes on the sample's last cell and stores nothing
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(x + (size_t)b * kC * hw), 0,
                                                                        (unsigned)((size_t)kC * hw * sizeof(T)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(stream), 0, (unsigned)kScratchBytes<T>, 0x00020000);
    // the ring: fragment i of tile t sits in ring[i % R]; its slot is refilled with fragment i + R as soon as it is consumed
    // (the refills of the last fragments read the padding behind the stream, see kScratchBytes)
    u32x4 ring[R];
    const int lane_off = lane * 16;
    static_for<R>([&](auto i) { ring[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, i * 1024, 0); });

    u32x4 xf[kKS][P];
    load_x<T, NHWC>(rx, live ? p : hw - 1, h, hw, xf);

    f32x16 acc[kNT];
#pragma unroll
    for (int n = 0; n < kNT; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[n][e] = 0.f;

    for (int t = 0; t < kHT; ++t) {
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
      static_for<kKS>([&](auto KS) {
        constexpr int ks = decltype(KS)::value;
        if constexpr (P == 2) {
          const u32x4 wh = take(std::integral_constant<int, 4 + 2 * ks>{});
          const u32x4 wm = take(std::integral_constant<int, 4 + 2 * ks + 1>{});
          hid = mfma16<T>(wm, xf[ks][0], hid);   // smallest terms first
          hid = mfma16<T>(wh, xf[ks][P - 1], hid);
          hid = mfma16<T>(wh, xf[ks][0], hid);
        } else {
          hid = mfma16<T>(take(std::integral_constant<int, 4 + ks>{}), xf[ks][0], hid);
        }
      });
      // Softplus in float32, then the operand parts of the two k-steps of GEMM-2
      u32x4 hf[2][P];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) {
          const float a = softplus(hid[8 * s + 2 * jp]), c = softplus(hid[8 * s + 2 * jp + 1]);
          if constexpr (P == 2) {
            unsigned hi, mid;
            split2_hm(a, c, hi, mid);
            hf[s][0][jp] = hi;
            hf[s][P - 1][jp] = mid;
          } else {
            hf[s][0][jp] = Pair<T>::narrow(f32x2{a, c});
          }
        }
      static_for<2 * kNT>([&](auto G) {
        constexpr int g = decltype(G)::value, s = g / kNT, n = g % kNT, i0 = 4 + kKS * P + g * P;
        if constexpr (P == 2) {
          const u32x4 wh = take(std::integral_constant<int, i0>{});
          const u32x4 wm = take(std::integral_constant<int, i0 + 1>{});
          acc[n] = mfma16<T>(wm, hf[s][0], acc[n]);
          acc[n] = mfma16<T>(wh, hf[s][P - 1], acc[n]);
          acc[n] = mfma16<T>(wh, hf[s][0], acc[n]);
        } else {
          acc[n] = mfma16<T>(take(std::integral_constant<int, i0>{}), hf[s][0], acc[n]);
        }
      });
    }

    // register e of tile n = logit 144 h + 16 n + e of this lane's cell: z = 8 h + j / 18, class j % 18 with j = 16 n + e
    const float* bias = b2 + 144 * h;
#pragma unroll
    for (int n = 0; n < kNT; ++n)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 bq = *reinterpret_cast<const f32x4*>(bias + 16 * n + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[n][4 * q + e] += bq[e];
      }
    if (live) {
      const int iy = p / dx, ix = p - iy * dx;
      const size_t cell = ((size_t)b * dx + ix) * dy + iy;   // the reference's permute(0, 3, 2, 1)
      int arg[8];
#pragma unroll
      for (int z = 0; z < 8; ++z) {
        float best = acc[(18 * z) >> 4][(18 * z) & 15];
        arg[z] = 0;
#pragma unroll
        for (int k = 1; k < kClasses; ++k) {
          const float v = acc[(18 * z + k) >> 4][(18 * z + k) & 15];
          if (v > best) { best = v; arg[z] = k; }
        }
      }
      const size_t vox = cell * kDz + 8 * h;
      if (pred) {
        u32x2 w;
        w[0] = arg[0] | (arg[1] << 8) | (arg[2] << 16) | (arg[3] << 24);
        w[1] = arg[4] | (arg[5] << 8) | (arg[6] << 16) | (arg[7] << 24);
        *reinterpret_cast<u32x2*>(pred + vox) = w;
      }
      if (logits) {
        f32x4* lo = reinterpret_cast<f32x4*>(logits + cell * kCols + 144 * h);
#pragma unroll
        for (int n = 0; n < kNT; ++n)
#pragma unroll
          for (int q = 0; q < 4; ++q) lo[4 * n + q] = f32x4{acc[n][4 * q], acc[n][4 * q + 1], acc[n][4 * q + 2], acc[n][4 * q + 3]};
      }
      if (hist) {
        const u32x2 lab = *reinterpret_cast<const u32x2*>(labels + vox);
        u32x2 msk = {0x01010101u, 0x01010101u};
        if (mask) msk = *reinterpret_cast<const u32x2*>(mask + vox);
#pragma unroll
        for (int z = 0; z < 8; ++z) {
          const int tl = (lab[z >> 2] >> (8 * (z & 3))) & 255, m = (msk[z >> 2] >> (8 * (z & 3))) & 255;
          if (tl < kClasses && m != 0) atomicAdd(&cnt[tl * kClasses + arg[z]], 1u);
        }
      }
      if constexpr (LOSS)
        loss_terms(acc, *reinterpret_cast<const u32x2*>(labels + vox), *reinterpret_cast<const u32x2*>(mask + vox), class_weight, ignore, lsum);
    }
  }
  if constexpr (LOSS) {
    __shared__ float lred[kBlock / 64][kLossSums];
    loss_row(lsum, lred, loss_partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kLossSums);
  }
  if (hist) {
    __syncthreads();
    for (int i = tid; i < kClasses * kClasses; i += kBlock)
      if (cnt[i]) atomicAdd(&hist[i], (unsigned long long)cnt[i]);
  }
}

bool shape_supported(int c, int hidden, int dz, int n_classes) { return c == kC && hidden == kHidden && dz == kDz && n_classes == kClasses; }

bool precision_supported(int x_dtype, int layout, int gemm) {
  if (layout != 0 && layout != 1) return false;
  if (x_dtype == DHD_F32) return gemm == DHD_SFA_GEMM_DEFAULT || gemm == DHD_SFA_GEMM_BF16X3;
  if (x_dtype == DHD_F16 || x_dtype == DHD_BF16) return gemm == DHD_SFA_GEMM_DEFAULT;   // gemm selects float32 arithmetic only
  return false;
}

size_t scratch_bytes(int x_dtype) { return x_dtype == DHD_F32 ? kScratchBytes<float> : kScratchBytes<__bf16>; }

template <class T, bool NHWC>
int launch(const void* x, const dhd_occ_head_weights* w, int b, int dy, int dx, uint8_t* pred, float* logits, const uint8_t* labels,
           const uint8_t* mask, int64_t* hist, void* scratch, hipStream_t st) {
  u32x4* stream = static_cast<u32x4*>(scratch);
  constexpr int n_pack = kHT * kFrags<T> * 64;
  hipLaunchKernelGGL(pack_stream_kernel<T>, dim3(dhd_cdiv(n_pack, kPackBlock)), dim3(kPackBlock), 0, st, w->w1, w->b1, w->w2, stream);
  DHD_LAUNCH_CHECK();
  hipLaunchKernelGGL((occ_head_kernel<T, NHWC>), dim3(dhd_cdiv((long)dy * dx, kCellsPerBlock), b), dim3(kBlock), 0, st,
                     static_cast<const T*>(x), stream, w->b2, dy, dx, pred, logits, labels, mask,
                     reinterpret_cast<unsigned long long*>(hist), (const float*)nullptr, 0, (float*)nullptr);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

}  // namespace

extern "C" {

int dhd_occ_head_infer_supported(int c, int hidden, int dz, int n_classes, int x_dtype, int layout, int gemm) {
  return shape_supported(c, hidden, dz, n_classes) && precision_supported(x_dtype, layout, gemm) ? 1 : 0;
}

int dhd_occ_head_infer_scratch_bytes(const dhd_occ_head_weights* w, int x_dtype, size_t* bytes) {
  if (!w || !bytes) return DHD_EINVAL;
  if (x_dtype != DHD_F32 && x_dtype != DHD_F16 && x_dtype != DHD_BF16) return DHD_EINVAL;
  if (!shape_supported(w->c, w->hidden, w->dz, w->n_classes) || !precision_supported(x_dtype, 0, w->gemm)) return DHD_EUNSUPPORTED;
  *bytes = scratch_bytes(x_dtype);
  return DHD_OK;
}

int dhd_occ_head_infer(const void* x, int x_dtype, int layout, const dhd_occ_head_weights* w, int b, int dy, int dx, uint8_t* pred,
                       float* logits, const uint8_t* labels, const uint8_t* mask, int64_t* hist, void* scratch, void* stream) {
  if (!x || !w || !w->w1 || !w->b1 || !w->w2 || !w->b2 || !scratch || b <= 0 || dy <= 0 || dx <= 0) return DHD_EINVAL;
  if ((!pred && !logits) || (hist && !labels)) return DHD_EINVAL;
  if (x_dtype != DHD_F32 && x_dtype != DHD_F16 && x_dtype != DHD_BF16) return DHD_EINVAL;
  if (!dhd_occ_head_infer_supported(w->c, w->hidden, w->dz, w->n_classes, x_dtype, layout, w->gemm)) return DHD_EUNSUPPORTED;
  // one sample of x behind a 32-bit buffer descriptor, byte offsets in an int; grid.y
  if ((size_t)dy * dx > ((size_t)1 << 30) / (kC * 4) || b > 65535) return DHD_EUNSUPPORTED;
  const uintptr_t align = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(scratch) | reinterpret_cast<uintptr_t>(w->b2) |
                          reinterpret_cast<uintptr_t>(logits);
  if ((align & 15) != 0 || (reinterpret_cast<uintptr_t>(pred) & 7) != 0) return DHD_EINVAL;
  if (hist && (((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(mask)) & 7) != 0)) return DHD_EINVAL;
  hipStream_t st = dhd_stream(stream);
  return dhd::with_dtype<dhd::NativeHalf>(x_dtype, [&](auto* tp) {
    using T = std::remove_pointer_t<decltype(tp)>;
    return layout ? launch<T, true>(x, w, b, dy, dx, pred, logits, labels, mask, hist, scratch, st)
                  : launch<T, false>(x, w, b, dy, dx, pred, logits, labels, mask, hist, scratch, st);
  });
}

}  // extern "C"

// the training half: the recompute backward and its dhdo_* entry points (the forward in training is dhd_occ_head_infer itself)
#include "occ_head_train.h"
// the head and its three losses as one operator: the forward's loss epilogue, the backward with the loss gradient, dhdl_*
#include "occ_head_loss.h"
