// Occupancy head and its three losses in training as one operator (dhd_amd/capi_occ_loss/dhd_amd_occ_head_loss.h): the loss sums
// as an epilogue of occ_head.hip's forward, and the loss gradient as a prologue of occ_head_train.h's backward.  occ_head.hip
// includes this file after occ_head_train.h: its helpers and that file's (make_parts, col_sums16, softplus_grad, pair_quads,
// store4, load_x_step, occ_head_bwd_params) are used as they are; the loss arithmetic is occ_loss_math.h's, shared with
// occ_loss.hip.  Neither occ_loss_sums nor occ_loss_grad runs, and the float32 dL/dlogits of the half types never exists.
//
// Forward: occ_head_kernel<T, NHWC, true>.  A lane ends with 8 whole voxels of its cell in registers (register e of tile n =
// logit 144 h + 16 n + e); with their 8 label and 8 mask bytes it adds its terms of T_i, P_i, N_i, CE and n_valid, a voxel that is
// masked out or ignored by a select (its logits may be NaN).  56 sums per lane -> the wave (a fixed butterfly) -> the four waves
// in order through LDS -> one row per workgroup in scratch -> occ_loss_finalize (double totals, the three losses).  No atomics.
//
// Backward: occ_head_loss_bwd_kernel.  The da GEMM sums over the 288 logit columns in the order 144 h + 8 ks + j, so lane half h
// holds the columns of its own 8 voxels: g = dL/dlogits is computed from the saved logits, the labels and the totals in the
// lane's registers (occ_loss_grad's closed form, coefficients per workgroup in double) and is the B operand as it lies.
//   half GEMMs     KEEP: g goes into the 72 fragment registers; ghalf is written on request for dW2 = g^T act
//   float32 GEMMs  RELOAD: g is written once to a float32 (cells, 288) buffer -- dW2's operand -- and the per-tile reloads read
//                  back what the same lane wrote
// Everything after the prologue is occ_head_bwd_kernel's tile loop; the kernels have names of their own because the set of
// occ_head_bwd_kernel / pack_train_stream_kernel instantiations is a closed list.
#pragma once

namespace {

// The backward's stream with the da block in voxel order: k-step ks, part p: W2[144 h + 8 ks + j][32 t + r].
template <class T>
__global__ __launch_bounds__(kPackBlock) void pack_loss_stream_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
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
    for (int j = 0; j < 8; ++j) v[j] = w2[(size_t)(144 * h + 8 * ks + j) * kHidden + 32 * t + r];
  } else {
    const int g = f - 4 - (kKS + kGS) * P, n = (g / P) % kXT, s = g / (P * kXT);
    part = g % P;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w1[(size_t)hid_unit(t, s, h, j) * kC + dx_ch(r, n)];
  }
  stream[idx] = pack_part<T>(v, part);
}

// v[0..8) added over the 32 lanes that share lane >> 5; lane r returns the total of v[r >> 2] (col_sums16's steps, one fewer)
__device__ __forceinline__ float col_sums8(float* v, int r) {
  fold_step<16, 4>(v, r);
  fold_step<8, 2>(v, r);
  fold_step<4, 1>(v, r);
  const float t = v[0] + __shfl_xor(v[0], 2, DHD_WAVE);
  return t + __shfl_xor(t, 1, DHD_WAVE);
}

// the forward's epilogue: this lane's terms of the 56 sums from its 8 voxels (acc after the bias, see occ_head_kernel)
__device__ __forceinline__ void loss_terms(const f32x16 (&acc)[kNT], u32x2 lab, u32x2 msk, const float* __restrict__ cw, int ignore,
                                           float (&sum)[kLossSums]) {
  constexpr int K = kLossK;
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    const int t = (lab[z >> 2] >> (8 * (z & 3))) & 255, m = (msk[z >> 2] >> (8 * (z & 3))) & 255;
    const bool valid = m != 0 && t != ignore;
    float lz[K];
#pragma unroll
    for (int k = 0; k < K; ++k) lz[k] = acc[(18 * z + k) >> 4][(18 * z + k) & 15];
    Voxel v;
    softmax18_vals(lz, t, v);
    sum[3 * K + 1] += valid ? 1.f : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const bool hit = valid && k == t;
      sum[K + k] += valid ? v.p[k] : 0.f;
      sum[2 * K + k] += hit ? v.p[k] : 0.f;
      sum[k] += hit ? 1.f : 0.f;
    }
    const float ce = cw[t < K ? t : 0] * (v.lse - v.zt);
    sum[3 * K] += valid && t < K ? ce : 0.f;
  }
}

// the 56 sums of a workgroup: every wave by wave_sum_bcast's fixed butterfly, the four waves in order -> row[0..55]
__device__ __forceinline__ void loss_row(float (&sum)[kLossSums], float (*red)[kLossSums], float* __restrict__ row) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int i = 0; i < kLossSums; ++i) {
    const float s = wave_sum_bcast(sum[i]);
    if (lane == 0) red[wv][i] = s;
  }
  __syncthreads();
  if (tid < kLossSums) row[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

template <class T, bool NHWC>
__global__ __launch_bounds__(kBlock) void occ_head_loss_bwd_kernel(const T* __restrict__ x, const u32x4* __restrict__ stream,
                                                                   const float* __restrict__ logits, const uint8_t* __restrict__ labels,
                                                                   const uint8_t* __restrict__ mask, const float* __restrict__ cw,
                                                                   const double* __restrict__ totals, const float* __restrict__ gl,
                                                                   int ignore, int non_empty, int dy, int dx, T* __restrict__ dx_out,
                                                                   float* __restrict__ partial, T* __restrict__ act_out,
                                                                   T* __restrict__ dhid_out, T* gout) {
  constexpr int P = kParts<T>, N = kTrainFrags<T>, E = sizeof(T), K = kLossK;
  constexpr bool KEEP = P == 1;   // half: g stays in registers; float32: g goes to gout and is reloaded per tile
  // The ring of a half NCHW x is 9 fragments deep, not 18: with 18 the allocator is one register short of 512 and puts a
  // fragment of g into private memory.  (The padding behind the stream is kTrainRing's, which covers the shorter read-ahead.)
  constexpr int R = KEEP && !NHWC ? 9 : kTrainRing<T>;
  static_assert(R <= kTrainRing<T>, "the read-ahead past the stream's end must stay inside its padding");
  static_assert(N % R == 0, "the ring position of a fragment must not depend on the hidden tile");
  __shared__ float red[kBlock / 64][kSums];   // per wave: sum_cells dh (512), sum_cells g (288)
  __shared__ float sa[K], sb[K], scw[K], sce;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, hw = dy * dx;
  const int p0 = (blockIdx.x * (kBlock / 64) + (tid >> 6)) * 32;   // wave-uniform
  float* myred = red[tid >> 6];
  loss_coefficients(totals, gl, cw, non_empty, tid, sa, sb, &sce);
  if (tid < K) scw[tid] = cw[tid];
  __syncthreads();
  if (p0 >= hw) {   // a wave past the sample adds nothing
    for (int i = lane; i < kSums; i += 64) myred[i] = 0.f;
  } else {
    const bool live = p0 + r < hw;   // a lane past the sample computes on its last cell, stores nothing and adds nothing
    const int p = live ? p0 + r : hw - 1;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(x + (size_t)b * kC * hw), 0,
                                                                        (unsigned)((size_t)kC * hw * sizeof(T)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(stream), 0, (unsigned)kTrainPackedBytes<T>, 0x00020000);
    u32x4 ring[R];
    const int lane_off = lane * 16;
    static_for<R>([&](auto i) { ring[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, i * 1024, 0); });

    u32x4 xf[KEEP ? kKS : 1][P], gf[KEEP ? kGS : 1][P];
    const int xoff = NHWC ? (p * kC + 8 * h) * E : (p + 8 * h * hw) * E;   // load_x's per-lane offset
    const int iy = p / dx, ix = p - iy * dx;
    const size_t cell = ((size_t)b * dx + ix) * dy + iy;   // the logits' order: the reference's permute(0, 3, 2, 1)
    const size_t pixel = (size_t)b * hw + p;               // x's order
    const bool ops = act_out != nullptr;                   // uniform over the launch: act and dhid, or neither

    // g of this lane's 8 voxels: columns 144 h + 18 z + k of its cell, exact zeros where the voxel is masked out or ignored
    // and in a lane past the sample.  Two voxels are 36 floats, nine 16-byte loads.
    const size_t col0 = cell * kCols + 144 * h;
    {
      float a[K];
#pragma unroll
      for (int k = 0; k < K; ++k) a[k] = sa[k];
      const float ce_scale = sce;
      const u32x2 lab = *reinterpret_cast<const u32x2*>(labels + cell * kDz + 8 * h);
      const u32x2 msk = *reinterpret_cast<const u32x2*>(mask + cell * kDz + 8 * h);
      // four voxels at a time (72 columns = nine k-steps): their g, then its fragments, its stores and its terms of db2
      static_for<2>([&](auto G4) {
        constexpr int g4 = decltype(G4)::value;
        float g[72];
        static_for<2>([&](auto Q) {
          constexpr int q = 2 * g4 + decltype(Q)::value;
          float lz[2][K];
          const f32x4* src = reinterpret_cast<const f32x4*>(logits + col0 + 36 * q);
#pragma unroll
          for (int i = 0; i < 9; ++i) {
            const f32x4 v = src[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) lz[(4 * i + e) / K][(4 * i + e) % K] = v[e];
          }
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const int z = 2 * q + s;
            const int t = (lab[z >> 2] >> (8 * (z & 3))) & 255, m = (msk[z >> 2] >> (8 * (z & 3))) & 255;
            const bool valid = live && m != 0 && t != ignore;
            const int tc = t < K ? t : 0;
            Voxel v;
            softmax18_vals(lz[s], t, v);
            float d[K];
            loss_grad18(v, t, a, t < K ? sb[tc] : 0.f, t < K ? scw[tc] : 0.f, ce_scale, d);
#pragma unroll
            for (int k = 0; k < K; ++k) g[18 * (z - 4 * g4) + k] = valid ? d[k] : 0.f;
          }
        });
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          const int ks = 9 * g4 + i;
          if constexpr (KEEP) {
            make_parts<T>(g + 8 * i, gf[ks]);
            if (gout && live) *reinterpret_cast<u32x4*>(gout + col0 + 8 * ks) = gf[ks][0];
          } else if (live) {
            f32x4* dst = reinterpret_cast<f32x4*>(gout + col0 + 8 * ks);
            dst[0] = f32x4{g[8 * i], g[8 * i + 1], g[8 * i + 2], g[8 * i + 3]};
            dst[1] = f32x4{g[8 * i + 4], g[8 * i + 5], g[8 * i + 6], g[8 * i + 7]};
          }
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          const float total = col_sums8(g + 8 * i, r);   // of column 144 h + 8 ks + (r >> 2); g is dead afterwards
          if ((r & 3) == 0) myred[kHidden + 144 * h + 8 * (9 * g4 + i) + (r >> 2)] = total;
        }
        __builtin_amdgcn_sched_barrier(0);   // the second four voxels after the first: 72 live values of g, not 144
      });
    }
    if constexpr (KEEP) {
      // x after g: an NCHW x arrives as 256 two-byte loads, and the 64 registers they are packed into are not live above
      load_x<T, NHWC>(rx, p, h, hw, xf);
      __builtin_amdgcn_sched_barrier(0);
    }
    // the float32 g of the RELOAD form: columns 144 h + 8 ks + j, what this lane stored above
    auto load_g = [&](int ks, float* v, int off) {
      const f32x4* gp = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(gout) + col0 + off + 8 * ks);
      const f32x4 g0 = gp[0], g1 = gp[1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = live ? g0[j] : 0.f;
        v[4 + j] = live ? g1[j] : 0.f;
      }
    };

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
  float* prow = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kSums;
  for (int i = tid; i < kSums; i += kBlock) prow[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

constexpr size_t kLossRowBytes = kLossSums * sizeof(float);
constexpr size_t kLossWorkspaceBytes = kLossSums * sizeof(double);   // the 56 totals: every byte written by the forward

template <class T> constexpr size_t kFwdPartialOffset = (kScratchBytes<T> + 15) / 16 * 16;

size_t loss_forward_scratch(int x_dtype, int b, int dy, int dx) {
  const size_t packed = x_dtype == DHD_F32 ? kFwdPartialOffset<float> : kFwdPartialOffset<__bf16>;
  return packed + (size_t)train_groups(b, dy, dx) * kLossRowBytes;
}

size_t loss_backward_scratch(int x_dtype, int b, int dy, int dx) {
  return train_packed_bytes(x_dtype) + (size_t)train_groups(b, dy, dx) * kSums * sizeof(float);
}

template <class T, bool NHWC>
int launch_loss_forward(const void* x, const dhd_occ_head_weights* w, int b, int dy, int dx, const uint8_t* labels, const uint8_t* mask,
                        const float* cw, int ignore, int non_empty, float* logits, float* losses, void* workspace, void* scratch,
                        hipStream_t st) {
  u32x4* stream = static_cast<u32x4*>(scratch);
  float* partial = reinterpret_cast<float*>(static_cast<char*>(scratch) + kFwdPartialOffset<T>);
  constexpr int n_pack = kHT * kFrags<T> * 64;
  hipLaunchKernelGGL(pack_stream_kernel<T>, dim3(dhd_cdiv(n_pack, kPackBlock)), dim3(kPackBlock), 0, st, w->w1, w->b1, w->w2, stream);
  DHD_LAUNCH_CHECK();
  hipLaunchKernelGGL((occ_head_kernel<T, NHWC, true>), dim3(dhd_cdiv((long)dy * dx, kCellsPerBlock), b), dim3(kBlock), 0, st,
                     static_cast<const T*>(x), stream, w->b2, dy, dx, (uint8_t*)nullptr, logits, labels, mask,
                     (unsigned long long*)nullptr, cw, ignore, partial);
  DHD_LAUNCH_CHECK();
  hipLaunchKernelGGL(occ_loss_finalize, dim3(1), dim3(kLossFinBlock), 0, st, partial, train_groups(b, dy, dx), cw, non_empty,
                     static_cast<double*>(workspace), losses);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

template <class T, bool NHWC>
int launch_loss_backward(const void* x, const dhd_occ_head_weights* w, int b, int dy, int dx, const float* logits, const uint8_t* labels,
                         const uint8_t* mask, const float* cw, int ignore, int non_empty, const float* gl, const void* workspace,
                         void* dx_out, float* db1, float* db2, void* act, void* dhid, void* g, void* scratch, hipStream_t st) {
  u32x4* stream = static_cast<u32x4*>(scratch);
  float* partial = reinterpret_cast<float*>(static_cast<char*>(scratch) + kTrainPackedBytes<T>);
  constexpr int n_pack = kHT * kTrainFrags<T> * 64;
  hipLaunchKernelGGL(pack_loss_stream_kernel<T>, dim3(dhd_cdiv(n_pack, kPackBlock)), dim3(kPackBlock), 0, st, w->w1, w->b1, w->w2, stream);
  DHD_LAUNCH_CHECK();
  hipLaunchKernelGGL((occ_head_loss_bwd_kernel<T, NHWC>), dim3(dhd_cdiv((long)dy * dx, kCellsPerBlock), b), dim3(kBlock), 0, st,
                     static_cast<const T*>(x), stream, logits, labels, mask, cw, static_cast<const double*>(workspace), gl, ignore,
                     non_empty, dy, dx, static_cast<T*>(dx_out), partial, static_cast<T*>(act), static_cast<T*>(dhid), static_cast<T*>(g));
  DHD_LAUNCH_CHECK();
  hipLaunchKernelGGL(occ_head_bwd_params, dim3(kSums / 16), dim3(kParamBlock), 0, st, partial, db1, db2, train_groups(b, dy, dx));
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

bool loss_args_supported(int ignore_index, int non_empty_idx) {
  return ignore_index >= 0 && ignore_index <= 255 && non_empty_idx >= 0 && non_empty_idx < kLossK;
}

}  // namespace

extern "C" {

int dhdl_occ_head_loss_supported(int c, int hidden, int dz, int n_classes, int x_dtype, int layout) {
  return dhd_occ_head_infer_supported(c, hidden, dz, n_classes, x_dtype, layout, DHD_SFA_GEMM_DEFAULT);
}

size_t dhdl_occ_head_loss_workspace_bytes(void) { return kLossWorkspaceBytes; }

int dhdl_occ_head_loss_scratch_bytes(const dhd_occ_head_weights* w, int x_dtype, int b, int dy, int dx, size_t* forward_bytes,
                                     size_t* backward_bytes) {
  if (forward_bytes) *forward_bytes = 0;
  if (backward_bytes) *backward_bytes = 0;
  if (!w || !forward_bytes || !backward_bytes) return DHD_EINVAL;
  if (b <= 0 || dy <= 0 || dx <= 0) return DHD_EINVAL;
  if (x_dtype != DHD_F32 && x_dtype != DHD_F16 && x_dtype != DHD_BF16) return DHD_EINVAL;
  if (!shape_supported(w->c, w->hidden, w->dz, w->n_classes) || !precision_supported(x_dtype, 0, w->gemm)) return DHD_EUNSUPPORTED;
  if (w->gemm != DHD_SFA_GEMM_DEFAULT || !train_size_supported(b, dy, dx)) return DHD_EUNSUPPORTED;
  *forward_bytes = loss_forward_scratch(x_dtype, b, dy, dx);
  *backward_bytes = loss_backward_scratch(x_dtype, b, dy, dx);
  return DHD_OK;
}

int dhdl_occ_head_loss_forward(const void* x, int x_dtype, int layout, const dhd_occ_head_weights* w, int b, int dy, int dx,
                               const uint8_t* labels, const uint8_t* mask, const float* class_weight, int ignore_index,
                               int non_empty_idx, float* logits, float* losses, void* workspace, void* scratch, size_t scratch_bytes,
                               void* stream) {
  if (!x || !w || !w->w1 || !w->b1 || !w->w2 || !w->b2 || !labels || !mask || !class_weight || !logits || !losses || !workspace ||
      !scratch || b <= 0 || dy <= 0 || dx <= 0)
    return DHD_EINVAL;
  if (x_dtype != DHD_F32 && x_dtype != DHD_F16 && x_dtype != DHD_BF16) return DHD_EINVAL;
  if (!dhd_aligned(16, x, w->w1, w->b1, w->w2, w->b2, logits, workspace, scratch) || !dhd_aligned(8, labels, mask) ||
      !dhd_aligned(4, class_weight, losses))
    return DHD_EINVAL;
  if (!dhd_occ_head_infer_supported(w->c, w->hidden, w->dz, w->n_classes, x_dtype, layout, w->gemm) || w->gemm != DHD_SFA_GEMM_DEFAULT)
    return DHD_EUNSUPPORTED;
  if (!loss_args_supported(ignore_index, non_empty_idx) || !train_size_supported(b, dy, dx)) return DHD_EUNSUPPORTED;
  if (scratch_bytes < loss_forward_scratch(x_dtype, b, dy, dx)) return DHD_ENOSPACE;
  hipStream_t st = dhd_stream(stream);
  return dhd::with_dtype<dhd::NativeHalf>(x_dtype, [&](auto* tp) {
    using T = std::remove_pointer_t<decltype(tp)>;
    return layout ? launch_loss_forward<T, true>(x, w, b, dy, dx, labels, mask, class_weight, ignore_index, non_empty_idx, logits, losses,
                                                 workspace, scratch, st)
                  : launch_loss_forward<T, false>(x, w, b, dy, dx, labels, mask, class_weight, ignore_index, non_empty_idx, logits, losses,
                                                  workspace, scratch, st);
  });
}

int dhdl_occ_head_loss_backward(const void* x, int x_dtype, int layout, const dhd_occ_head_weights* w, int b, int dy, int dx,
                                const float* logits, const uint8_t* labels, const uint8_t* mask, const float* class_weight,
                                int ignore_index, int non_empty_idx, const float* grad_losses, const void* workspace, void* dx_out,
                                float* db1, float* db2, void* act, void* dhid, void* g, void* scratch, size_t scratch_bytes, void* stream) {
  if (!x || !w || !w->w1 || !w->b1 || !w->w2 || !logits || !labels || !mask || !class_weight || !grad_losses || !workspace || !dx_out ||
      !db1 || !db2 || !scratch || b <= 0 || dy <= 0 || dx <= 0)
    return DHD_EINVAL;
  if (x_dtype != DHD_F32 && x_dtype != DHD_F16 && x_dtype != DHD_BF16) return DHD_EINVAL;
  if ((act == nullptr) != (dhid == nullptr)) return DHD_EINVAL;          // the two hidden operands: both or neither
  if (x_dtype == DHD_F32 ? !g : (g && !act)) return DHD_EINVAL;          // float32: g is the kernel's own operand; half: ghalf beside act
  if (!dhd_aligned(16, x, w->w1, w->b1, w->w2, logits, workspace, dx_out, db1, db2, act, dhid, g, scratch) || !dhd_aligned(8, labels, mask) ||
      !dhd_aligned(4, class_weight, grad_losses))
    return DHD_EINVAL;
  if (!dhd_occ_head_infer_supported(w->c, w->hidden, w->dz, w->n_classes, x_dtype, layout, w->gemm) || w->gemm != DHD_SFA_GEMM_DEFAULT)
    return DHD_EUNSUPPORTED;
  if (!loss_args_supported(ignore_index, non_empty_idx) || !train_size_supported(b, dy, dx)) return DHD_EUNSUPPORTED;
  if (scratch_bytes < loss_backward_scratch(x_dtype, b, dy, dx)) return DHD_ENOSPACE;
  hipStream_t st = dhd_stream(stream);
  return dhd::with_dtype<dhd::NativeHalf>(x_dtype, [&](auto* tp) {
    using T = std::remove_pointer_t<decltype(tp)>;
    return layout ? launch_loss_backward<T, true>(x, w, b, dy, dx, logits, labels, mask, class_weight, ignore_index, non_empty_idx,
                                                  grad_losses, workspace, dx_out, db1, db2, act, dhid, g, scratch, st)
                  : launch_loss_backward<T, false>(x, w, b, dy, dx, logits, labels, mask, class_weight, ignore_index, non_empty_idx,
                                                   grad_losses, workspace, dx_out, db1, db2, act, dhid, g, scratch, st);
  });
}

}  // extern "C"
