// SFA backward, layer 2: the data gradient AND the weight gradient of conv2 in one persistent kernel on PAIRS of compute units
// ("pair" kernel; bf16x3, float32 storage, C = 128 / 256).
//
// Reference: models/necks/mix.py:51 (spacial_leanring: conv1x1 - BN - ReLU - conv1x1 - BN), its backward through conv2.
//
// Both GEMMs of the layer consume gy = c0 g + c1 y + c2 (the BatchNorm-2 backward prologue):
//   g1[ci][p]   = (sum_co W[co][ci] gy[co][p]) * [z1[ci][p] > 0]          k = co      (pw_gemm_cu_kernel EPI 1)
//   dW[co][ci] += sum_p gy[co][p] z1[ci][p],  z1 = relu(sc1 y1 + sh1)     k = pixel   (pw_wgrad3_kernel)
// In the folded flow (sfa_stage.hip) gy passes from the first launch to the second through memory and the second re-reads g1
// for the BatchNorm-1 sums: 7T of traffic where the layer needs g, y, y1 in and g1 out (4T).  One CU cannot hold both products
// at C = 256 (256 KB of weight fragments + 256 KB of accumulators against 512 KB of registers), two CUs can: the CUs of a pair
// walk the SAME 32-pixel steps, each stages the whole gy tile, and CU `half` keeps
//   * the MFMA A fragments of W^T for its C/2 rows ci of the data gradient (v_mfma_f32_16x16x32_bf16: a wave owns 16 rows for all
//     K: C/32 k-steps x 2 parts x 4 = 64 VGPRs at C = 256, and two 16 x 16 accumulators = 8),
//   * the accumulators of dW[:, its C/2 columns ci] (v_mfma_f32_32x32x16_bf16: C/64 tiles of 32 x 32 per wave = 64 VGPRs).
// The two CUs share nothing but read-only inputs: no flags, no waiting on each other; where they run (blocks b and b + 8 land on
// one XCD in practice, so the partner's read of the tile is an L2 hit) decides speed only.
//
// A workgroup has C/32 waves (512 threads at C = 256; 256 at C = 128, where the same form needs no more).  Per step:
//   stage    lane (g, q) of wave wv holds rows 32 wv + 4 g + j (j < 4) of g and y, pixels 4 q .. 4 q + 3 (one 16-byte load each: 8
//            lanes = one 128-byte line), applies the prologue in pw_gemm_cu_kernel's order of operations, cuts the result into two
//            bf16 parts ONCE and writes it to two LDS images in MFMA fragment order:
//              D image (B operand of the data gradient) unit [k-step 32][part][pixel half nt][lane = 16 kq + n], pixel 4 q + e at
//              (nt, n) = (e >> 1, q + 8 (e & 1)); a lane's 4 rows of one pixel are the 8 bytes (g & 1) of unit kq = g >> 1;
//              A image (A operand of the weight gradient) unit [k-step 16 kk][co tile][part][lane = m' + 32 h], pixel quad q at
//              (kk, h) = (q >> 2, (q >> 1) & 1), bytes 8 (q & 1); row m of the tile sits at m' = m ^ (2 kk + h);
//            and its two rows ci of y1 (rows 16 wv + g + 8 k of the CU's half) as z1 into the
//              B image unit [kk][ci tile][part][lane = m' + 32 h], m' = m ^ ((2 kk + h) << 1).
//            Every 16-lane group of a ds_write_b64 covers one aligned 128-byte span, and every ds_read_b128 reads the 64 units of
//            one [..][lane] block, permuted inside aligned groups of 4 (8) units: no bank conflicts by the rules of
//            MI355X_MICROARCH.md (tests/test_sfa_pair_map.py simulates all five access patterns).
//   compute  3 (C/32) 2 MFMAs 16x16x32 for the data gradient and 3 (C/64) 2 MFMAs 32x32x16 for the weight gradient per wave.
//   epilogue the wave's 16 x 32 result goes through a wave-private patch so that lane (g, q) sees pixels 4 q .. of rows g and
//            g + 8 of the wave's 16 -- the rows and pixels whose raw y1 it holds from the staging: the ReLU pass bit is
//            recomputed from y1 with the forward's own expression (no mask read), g1 is stored in whole lines, and sum g1,
//            sum g1 (y1 - mu1) are kept per lane over the worker's steps.
// Two LDS barriers per step (the images are single-buffered: 80 KB + patches at C = 256); the loads of step s + 1 are issued as
// soon as the staging of step s has read its raw rows and are in flight during its MFMAs and epilogue.  cu_lds_barrier, not __syncthreads: see sfa_gemm_cu.h.
// At the end a CU writes its C x C/2 columns of the worker's partial matrix and its half of the worker's row [2][C] in
// pw_wgrad3_kernel's FOLD 1 format, so wgrad_reduce_kernel and bn_backward_rows_kernel serve unchanged with 128 workers.
// No atomics, fixed orders: the same bytes on every call.
#pragma once
#include "sfa_gemm_cu.h"

namespace dhd_sfa {

constexpr int kPairWorkers = 128;   // pairs of workgroups = workers of the step partition (wg_first_step)
constexpr int kPairGrid = 2 * kPairWorkers;
constexpr int kPairPatchPitch = 36;   // floats per row of a wave's 16 x 32 patch

// Workgroup -> (worker, half of the input channels ci).  Workgroups b and b + 8 form a pair: equal blockIdx % 8 (one XCD under
// round-robin dispatch) and equal blockIdx / 16.
struct PairSlot { int worker, half; };
__host__ __device__ inline PairSlot pair_slot(int block) {
  PairSlot s;
  s.worker = (block >> 4) * 8 + (block & 7);
  s.half = (block >> 3) & 1;
  return s;
}

// 16-byte unit of the three LDS images (counted from the image's start) and the byte inside it, for the WRITER of
//   D: rows co .. co + 3 (co % 4 == 0) of pixel p;  A: pixels 4 q .. 4 q + 3 of row co;  B: pixels 4 q .. of row ci (of the half)
// and for the READER lane of a fragment.  c: channels.
__host__ __device__ inline int pair_d_write(int co, int p, int part) {
  const int q = p >> 2, e = p & 3;
  return (((((co >> 5) * 2 + part) * 2 + (e >> 1)) * 64 + 16 * ((co >> 3) & 3) + q + 8 * (e & 1)) << 4) + 8 * ((co >> 2) & 1);
}
__host__ __device__ inline int pair_d_read(int ks, int part, int nt, int lane) { return ((((ks * 2 + part) * 2 + nt) * 64) + lane) << 4; }
__host__ __device__ inline int pair_a_write(int c, int co, int q, int part) {
  const int kk = q >> 2, h = (q >> 1) & 1;
  return ((((kk * (c / 32) + (co >> 5)) * 2 + part) * 64 + ((co & 31) ^ (2 * kk + h)) + 32 * h) << 4) + 8 * (q & 1);
}
__host__ __device__ inline int pair_a_read(int c, int kk, int tile, int part, int lane) {
  return (((kk * (c / 32) + tile) * 2 + part) * 64 + (lane ^ (2 * kk + (lane >> 5)))) << 4;
}
__host__ __device__ inline int pair_b_write(int c, int ci, int q, int part) {
  const int kk = q >> 2, h = (q >> 1) & 1;
  return ((((kk * (c / 64) + (ci >> 5)) * 2 + part) * 64 + ((ci & 31) ^ ((2 * kk + h) << 1)) + 32 * h) << 4) + 8 * (q & 1);
}
__host__ __device__ inline int pair_b_read(int c, int kk, int tile, int part, int lane) {
  return (((kk * (c / 64) + tile) * 2 + part) * 64 + (lane ^ ((2 * kk + (lane >> 5)) << 1))) << 4;
}

// dynamic LDS of a workgroup: D image + A image + B image + one patch per wave
// + the prologue table [3][c]
inline size_t pair_lds_bytes(int c) {
  return (size_t)128 * c + 128 * c + 64 * c + (size_t)(c / 32) * 16 * kPairPatchPitch * sizeof(float) + (size_t)3 * c * sizeof(float);
}

struct PairArgs {
  const float* g;       // (nb, C, hw) gradient entering the BatchNorm backward (g2)
  const float* y;       // (nb, C, hw) that BatchNorm's input (y2)
  const float* coef;    // [3][C] BatchNorm-backward table c0 | c1 | c2 (the same for every sample: bn_backward_coef_from_sums)
  const u32x4* wp;      // cu_pack_weight image of W^T (rows ci, k = co): the data gradient's own image
  const float* b;       // (nb, C, hw) y1
  const float* b_scsh;  // [2][C] BatchNorm-1 scale | shift (the forward's prologue table)
  const float* b_mean;  // [C] BatchNorm-1 batch mean
  float* out;           // (nb, C, hw) g1
  float* partial;       // [kPairWorkers][C][C] weight-gradient partial matrices
  float* rows;          // [kPairWorkers][2][C] sum g1 | sum g1 (y1 - mean)
  int hw, nb;
};

__device__ __forceinline__ f32x4 mfma16_bf16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// FirstStep: wg_first_step of sfa_stage.hip (the partition the row readers use), passed as a type so that this header stands alone
// AUX: cache policy of the loads of g, y and y1 (2: non-temporal, the product's; plain loads make the partner's reads L2 hits --
// 495 MB fetched per launch instead of 670 at (4, 256, 200 x 200) -- without making the kernel faster, and cost the step's other
// kernels 20 us: LAB_NOTEBOOK R22.1)
template <int C, int AUX, class FirstStep>
__global__ __launch_bounds__(2 * C, 1) void pw_pair_kernel(PairArgs a) {
  static_assert(C == 128 || C == 256, "C/32 waves, C/64 weight-gradient tiles per wave");
  constexpr int KS = C / 32, KCN = C / 16, HALF = C / 2;
  constexpr int TCO = C / 32, TCI = C / 64;                    // 32-row tiles of dW: rows co, columns ci of the half
  constexpr int TA = C / 128, TB = 2, WCI = TCI / TB;          // tiles per wave, waves along ci
  constexpr int DIMG = 128 * C, AIMG = 128 * C, BIMG = 64 * C;
  extern __shared__ __attribute__((aligned(16))) unsigned char pair_lds[];
  unsigned char* const dimg = pair_lds;
  unsigned char* const aimg = pair_lds + DIMG;
  unsigned char* const bimg = pair_lds + DIMG + AIMG;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 3, q = lane & 7;
  float* const patch = reinterpret_cast<float*>(pair_lds + DIMG + AIMG + BIMG) + wv * (16 * kPairPatchPitch);
  const PairSlot slot = pair_slot((int)blockIdx.x);
  const int cib = slot.half * HALF;                            // first channel ci of this CU's half
  const int hw = a.hw, sps = (hw + 31) >> 5;
  const long long n_steps = (long long)a.nb * sps;
  const int first = (int)FirstStep{}(n_steps, slot.worker, kPairWorkers);
  const int count = (int)FirstStep{}(n_steps, slot.worker + 1, kPairWorkers) - first;
  const int row_bytes = hw * 4;
  const unsigned in_bytes = (unsigned)((size_t)C * hw * sizeof(float));

  // ---- W^T fragments -> registers: lane = (row r of the wave's 16, k quarter kq), gathered from the 32x32x16 image ----------
  u32x4 wh[KS], wm[KS];
  {
    const int row = cib + 16 * wv + (lane & 15), kq = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const u32x4* src = a.wp + ((size_t)((row >> 5) * KCN + 2 * ks + (kq >> 1)) * 2) * 64 + (row & 31) + 32 * (kq & 1);
      wh[ks] = src[0];
      wm[ks] = src[64];
    }
  }
  // ---- per-lane constants ---------------------------------------------------------------------------------------------------
  const int co0 = 32 * wv + 4 * g;                             // staged rows co0 .. co0 + 3 of g, y
  // the prologue table lives in LDS and is read per step (12 registers less than keeping the lane's rows resident)
  float* const cf_lds = reinterpret_cast<float*>(pair_lds + DIMG + AIMG + BIMG) + (C / 32) * (16 * kPairPatchPitch);
  for (int i = tid; i < 3 * C; i += 2 * C) cf_lds[i] = a.coef[i];
  float bsc[2], bsh[2], bmu[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int ch = cib + 16 * wv + g + 8 * k;                  // staged rows of y1 == the rows of g1 this lane stores
    bsc[k] = a.b_scsh[ch];
    bsh[k] = a.b_scsh[C + ch];
    bmu[k] = a.b_mean[ch];
  }
  const int lda_voff = (co0 * hw + 4 * q) * 4;
  const int ldb_voff = ((cib + 16 * wv + g) * hw + 4 * q) * 4;
  int aw[4], bw[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) aw[j] = pair_a_write(C, co0 + j, q, 0);
#pragma unroll
  for (int k = 0; k < 2; ++k) bw[k] = pair_b_write(C, 16 * wv + g + 8 * k, q, 0);
  const int dw = pair_d_write(co0, 4 * q, 0);
  const int a_rd = (lane ^ (lane >> 5)) << 4, b_rd = (lane ^ ((lane >> 5) << 1)) << 4;   // k-step 0; k-step 1: ^ 2 (^ 4) units

  f32x16 acc[TA][TB];
#pragma unroll
  for (int i = 0; i < TA; ++i)
#pragma unroll
    for (int j = 0; j < TB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  float s1[2] = {0.f, 0.f}, s2[2] = {0.f, 0.f};

  f32x4 rg[4], ry[4], rb[2];
  auto issue = [&](int s) {
    const int b = s / sps, p0 = (s - b * sps) * 32;
    const __amdgpu_buffer_rsrc_t sg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.g + (size_t)b * C * hw), 0, in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t sy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.y + (size_t)b * C * hw), 0, in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t sb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.b + (size_t)b * C * hw), 0, in_bytes, 0x00020000);
    // a pixel quad beyond the row's end (last step of a sample, hw % 32 != 0) re-reads quad 0: it is staged as zeros
    const bool okq = p0 + 4 * q < hw;
    const int va = okq ? lda_voff : lda_voff - 16 * q, vb = okq ? ldb_voff : ldb_voff - 16 * q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      rg[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(sg, va, j * row_bytes + p0 * 4, AUX));
      ry[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(sy, va, j * row_bytes + p0 * 4, AUX));
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) rb[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(sb, vb, 8 * k * row_bytes + p0 * 4, AUX));
  };

  __builtin_amdgcn_s_waitcnt(0x0F70);                          // vmcnt(0): weights and tables are complete before the loop (sfa_gemm_cu.h)
  cu_lds_barrier();                                            // publishes the prologue table
  if (count > 0) {                                             // workgroup-uniform
    issue(first);
    {   // as many (dropped) stores as an epilogue issues, so that the wait counts at the loop's head agree with the back edge's
      const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(a.out, 0, 16, 0x00020000);
      store_b128_guarded<0>(u32x4{0u, 0u, 0u, 0u}, ro, 0x7ffffff0, 0);
      store_b128_guarded<0>(u32x4{0u, 0u, 0u, 0u}, ro, 0x7ffffff0, 0);
    }
  }
  for (int it = 0; it < count; ++it) {
    const int s = first + it;
    const int b = s / sps, p0 = (s - b * sps) * 32;
    const bool okq = p0 + 4 * q < hw;
    // ---- stage: prologue, one split, three images ------------------------------------------------------------------------
    // First everything that reads the raw rows, then the next step's loads into the registers that frees: their issue (which can
    // block behind the texture-address queue) then overlaps the other waves' splits and LDS stores, not the MFMAs
    float v[4][4];                                             // [pixel e][row j]
    {
      const f32x4 c0 = *reinterpret_cast<const f32x4*>(cf_lds + co0);
      const f32x4 c1 = *reinterpret_cast<const f32x4*>(cf_lds + C + co0);
      const f32x4 c2 = *reinterpret_cast<const f32x4*>(cf_lds + 2 * C + co0);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float tv = fmaf(c0[j], rg[j][e], c2[j]);
          tv = fmaf(c1[j], ry[j][e], tv);
          v[e][j] = okq ? tv : 0.f;
        }
    }
    f32x4 yk[2];
    unsigned pass[2];
    float z[2][4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      yk[k] = rb[k];
      pass[k] = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float zr = fmaxf(fmaf(bsc[k], rb[k][e], bsh[k]), 0.f);   // the forward's prologue: z > 0 <=> its recorded pass bit
        pass[k] |= min(__float_as_uint(zr), 1u) << e;
        z[k][e] = okq ? zr : 0.f;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    issue(first + min(it + 1, count - 1));                     // past the end: the last step again, never staged
    __builtin_amdgcn_sched_barrier(0);
    unsigned h01[4], m01[4], h23[4], m23[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      split2_hm(v[e][0], v[e][1], h01[e], m01[e]);
      split2_hm(v[e][2], v[e][3], h23[e], m23[e]);
      const int off = dw + (((e >> 1) * 64 + 8 * (e & 1)) << 4);
      *reinterpret_cast<u32x2*>(dimg + off) = u32x2{h01[e], h23[e]};
      *reinterpret_cast<u32x2*>(dimg + off + 2048) = u32x2{m01[e], m23[e]};
    }
    {   // the same bf16 values, paired along the pixels: row j's quad from the row-pair words
      constexpr unsigned LO = 0x05040100u, HI = 0x07060302u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned* hs = j < 2 ? h01 : h23;
        const unsigned* ms = j < 2 ? m01 : m23;
        const unsigned sel = (j & 1) ? HI : LO;
        const u32x2 hq = {__builtin_amdgcn_perm(hs[1], hs[0], sel), __builtin_amdgcn_perm(hs[3], hs[2], sel)};
        const u32x2 mq = {__builtin_amdgcn_perm(ms[1], ms[0], sel), __builtin_amdgcn_perm(ms[3], ms[2], sel)};
        *reinterpret_cast<u32x2*>(aimg + aw[j]) = hq;
        *reinterpret_cast<u32x2*>(aimg + aw[j] + 1024) = mq;
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      unsigned zh01, zm01, zh23, zm23;
      split2_hm(z[k][0], z[k][1], zh01, zm01);
      split2_hm(z[k][2], z[k][3], zh23, zm23);
      *reinterpret_cast<u32x2*>(bimg + bw[k]) = u32x2{zh01, zh23};
      *reinterpret_cast<u32x2*>(bimg + bw[k] + 1024) = u32x2{zm01, zm23};
    }
    cu_lds_barrier();

    // ---- data gradient: D[ci of the wave's 16][pixel] over all co ---------------------------------------------------------
    f32x4 dacc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const u32x4 bh = *reinterpret_cast<const u32x4*>(dimg + pair_d_read(ks, 0, nt, lane));
        const u32x4 bm = *reinterpret_cast<const u32x4*>(dimg + pair_d_read(ks, 1, nt, lane));
        dacc[nt] = mfma16_bf16(wm[ks], bh, dacc[nt]);          // smallest terms first
        dacc[nt] = mfma16_bf16(wh[ks], bm, dacc[nt]);
        dacc[nt] = mfma16_bf16(wh[ks], bh, dacc[nt]);
      }
    // ---- weight gradient: dW[co tiles of the wave][ci tiles of the wave] += gy z1^T over the step's 32 pixels -------------------
    {
      const int wco = wv / WCI, wci = wv % WCI;
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        u32x4 fb[TB][2];
#pragma unroll
        for (int j = 0; j < TB; ++j)
#pragma unroll
          for (int t = 0; t < 2; ++t) fb[j][t] = *reinterpret_cast<const u32x4*>(bimg + ((((k2 * TCI + TB * wci + j) * 2 + t) * 64) << 4) + (b_rd ^ (k2 << 6)));
#pragma unroll
        for (int i = 0; i < TA; ++i) {
          u32x4 fa[2];
#pragma unroll
          for (int t = 0; t < 2; ++t) fa[t] = *reinterpret_cast<const u32x4*>(aimg + ((((k2 * TCO + TA * wco + i) * 2 + t) * 64) << 4) + (a_rd ^ (k2 << 5)));
#pragma unroll
          for (int j = 0; j < TB; ++j) acc[i][j] = mfma_bf16(fa[1], fb[j][0], acc[i][j]);
#pragma unroll
          for (int j = 0; j < TB; ++j) acc[i][j] = mfma_bf16(fa[0], fb[j][1], acc[i][j]);
#pragma unroll
          for (int j = 0; j < TB; ++j) acc[i][j] = mfma_bf16(fa[0], fb[j][0], acc[i][j]);
        }
      }
    }
    // ---- epilogue: patch transposition, ReLU mask, g1 in whole lines, BatchNorm-1 sums ----------------------------------------
    {
      const int col = lane & 15, prow = 4 * (lane >> 4);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) patch[(prow + i) * kPairPatchPitch + 4 * (col & 7) + 2 * nt + (col >> 3)] = dacc[nt][i];
      const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)b * C * hw, 0, in_bytes, 0x00020000);
      const int voff = okq ? ldb_voff : 0x7ffffff0;            // beyond the buffer's range: the store is dropped
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        f32x4 o = *reinterpret_cast<const f32x4*>(patch + (g + 8 * k) * kPairPatchPitch + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = __int_as_float(__float_as_int(o[e]) & __builtin_amdgcn_sbfe((int)pass[k], e, 1));
        const f32x4 y1 = yk[k];
        const float mu = bmu[k];
        const float t1 = (o.x + o.y) + (o.z + o.w);
        const float t2 = (o.x * (y1.x - mu) + o.y * (y1.y - mu)) + (o.z * (y1.z - mu) + o.w * (y1.w - mu));
        s1[k] += okq ? t1 : 0.f;
        s2[k] += okq ? t2 : 0.f;
        store_b128_guarded<0>(__builtin_bit_cast(u32x4, o), ro, voff, 8 * k * row_bytes + p0 * 4);
      }
    }
    cu_lds_barrier();
  }

  // ---- this CU's columns of the worker's partial matrix (zeros from a worker without steps) and its half of the worker's row ----
  {
    const int wco = wv / WCI, wci = wv % WCI;
    float* po = a.partial + (size_t)slot.worker * C * C;
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
      for (int j = 0; j < TB; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int co = 32 * (TA * wco + i) + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
          const int ci = cib + 32 * (TB * wci + j) + (lane & 31);
          po[(size_t)co * C + ci] = acc[i][j][e];
        }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    float v1 = s1[k], v2 = s2[k];
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
      v1 += __shfl_xor(v1, m, DHD_WAVE);
      v2 += __shfl_xor(v2, m, DHD_WAVE);
    }
    if (q == 0) {
      float* row = a.rows + (size_t)slot.worker * 2 * C + cib + 16 * wv + g + 8 * k;
      row[0] = v1;
      row[C] = v2;
    }
  }
}

}  // namespace dhd_sfa
