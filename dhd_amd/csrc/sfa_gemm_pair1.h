// SFA backward, layer 1: the data gradient AND the weight gradient of conv1 in one persistent kernel on PAIRS of compute units
// (bf16x3, float32 storage, C = 128 / 256).  The plan is pw_pair_kernel's (sfa_gemm_pair.h: 256 workgroups, pair_slot, 128
// pair-workers over the 32-pixel steps, the three single-buffered LDS images and their maps, two LDS barriers per step, no flags,
// no atomics, fixed summation orders); what differs is what the layer feeds it and what it leaves behind.
//
// Reference: models/necks/mix.py:46-51 (u = a x_bev + (1 - a) x_voxel, conv1x1 - BN), the backward through conv1.
//
// Both GEMMs of the layer consume gy1 = c0 g1 + c1 y1 + c2 (the BatchNorm-1 backward prologue):
//   du[ci][p]   = sum_co W1[co][ci] gy1[co][p]                                  k = co      (pw_gemm_cu_kernel EPI 2)
//   dW1[co][ci] += sum_p gy1[co][p] u[ci][p],  u = a x_bev + (1 - a) x_voxel    k = pixel   (pw_wgrad3_kernel)
// and the channel attention's gradient needs  sum_p du[ci][p] (x_bev - x_voxel)[ci][p]  per sample (blend1_da_kernel's term).
// In the folded flow gy1 passes from the first launch to the second through memory (written over g1, read back) and the second
// re-reads du: 6T read + 2T written where the layer needs g1, y1, x (2T) in and du out.  Here a CU of a pair stages the whole gy1
// tile (D and A images), the rows of u of ITS half of the input channels ci (B image), keeps x_bev - x_voxel of the rows and
// pixels whose du it will see after the patch transposition, stores du in whole lines and sums du (x_bev - x_voxel) per lane.
// g1 is NOT written: it stays the gradient layer 2 made.
//
// The blend coefficients a | 1 - a are per SAMPLE: the CU's half of them lies in LDS ([C/2][2] floats) and is refreshed, under the
// step's second barrier, whenever the worker's next step belongs to another sample; at the same moment the lane sums of the
// finished sample go out as the worker's row of that sample, in pw_wgrad3_kernel's FOLD 2 format with 128 workers: row
// worker + sample, [C] floats, each CU its half of the channels (fc_backward_kernel reads them with fold_workers = kPairWorkers).
// A worker without steps writes a row of zeros for the sample its empty range lies in.  The C x C/2 columns of the worker's partial
// matrix go where pw_pair_kernel puts them (wgrad_reduce_kernel over 128 matrices).
#pragma once
#include "sfa_gemm_pair.h"

namespace dhd_sfa {

// dynamic LDS of a workgroup: pw_pair_kernel's + the blend coefficients [c / 2][2] of the current sample
inline size_t pair1_lds_bytes(int c) { return pair_lds_bytes(c) + (size_t)c * sizeof(float); }

struct Pair1Args {
  const float* g;       // (nb, C, hw) gradient entering the BatchNorm-1 backward (g1)
  const float* y;       // (nb, C, hw) that BatchNorm's input (y1)
  const float* coef;    // [3][C] BatchNorm-backward table c0 | c1 | c2 (the same for every sample: bn_backward_coef_from_sums)
  const u32x4* wp;      // cu_pack_weight image of W1^T (rows ci, k = co): the data gradient's own image
  const float* x;       // (nb, 2C, hw) x_bev | x_voxel
  const float* tab_a;   // [nb][3][C] a | 1 - a | 0 (fc_forward_kernel)
  float* out;           // (nb, C, hw) du
  float* partial;       // [kPairWorkers][C][C] weight-gradient partial matrices
  float* rows;          // [kPairWorkers + nb][C]: row worker + sample = sum du (x_bev - x_voxel) over the worker's steps of the sample
  int hw, nb;
};

// FirstStep: wg_first_step of sfa_stage.hip, as in pw_pair_kernel.  AUX: cache policy of the loads of g1 and y1, which BOTH CUs of
// a pair read, XAUX: of the loads of x, of which a CU reads its own half (2: non-temporal).  SAUX: that of the du stores (0: plain
// -- stage_gx reads du in the next big launch).  All were measured on the whole step, not on the kernel: LAB_NOTEBOOK R26.1.
template <int C, int AUX, class FirstStep, int SAUX = 0, int XAUX = AUX>
__global__ __launch_bounds__(2 * C, 1) void pw_pair1_kernel(Pair1Args a) {
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
  const unsigned x_bytes = (unsigned)((size_t)2 * C * hw * sizeof(float));

  // ---- W1^T fragments -> registers: lane = (row r of the wave's 16, k quarter kq), gathered from the 32x32x16 image ----------
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
  const int co0 = 32 * wv + 4 * g;                             // staged rows co0 .. co0 + 3 of g1, y1
  float* const cf_lds = reinterpret_cast<float*>(pair_lds + DIMG + AIMG + BIMG) + (C / 32) * (16 * kPairPatchPitch);
  float* const ab_lds = cf_lds + 3 * C;                        // [HALF][2]: a | 1 - a of the current sample, this CU's half
  for (int i = tid; i < 3 * C; i += 2 * C) cf_lds[i] = a.coef[i];
  // the blend coefficients of sample b (workgroup-uniform call; the caller's barrier publishes them)
  auto load_ab = [&](int b) {
    if (tid < HALF) {
      const float* t = a.tab_a + (size_t)b * 3 * C + cib + tid;
      *reinterpret_cast<f32x2*>(ab_lds + 2 * tid) = f32x2{t[0], t[C]};
    }
  };
  load_ab(min(first / sps, a.nb - 1));
  const int lda_voff = (co0 * hw + 4 * q) * 4;
  const int ldb_voff = ((cib + 16 * wv + g) * hw + 4 * q) * 4; // rows of x_bev staged == rows of du stored (k: + 8 rows)
  // one base per image: row co0 + j of the A image lies at aw0 ^ (j << 4) (co0 % 4 == 0 and the map's XOR term is below 4), row
  // + 8 of the B image at bw0 ^ 128 (g < 8, the XOR term below 8).  The XOR is an opaque instruction where it is used: hipcc
  // would otherwise keep all six addresses in registers, and the kernel has none to spare at C = 256.
  const int aw0 = pair_a_write(C, co0, q, 0), bw0 = pair_b_write(C, 16 * wv + g, q, 0);
  auto xor_c = [](int v, auto cc) {
    int r;
    asm("v_xor_b32 %0, %1, %2" : "=v"(r) : "n"(decltype(cc)::value), "v"(v));
    return r;
  };
  const int dw = pair_d_write(co0, 4 * q, 0);
  const int a_rd = (lane ^ (lane >> 5)) << 4, b_rd = (lane ^ ((lane >> 5) << 1)) << 4;   // k-step 0; k-step 1: ^ 2 (^ 4) units

  f32x16 acc[TA][TB];
#pragma unroll
  for (int i = 0; i < TA; ++i)
#pragma unroll
    for (int j = 0; j < TB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  float fs[2] = {0.f, 0.f};                                    // sum du (x_bev - x_voxel) of the current sample, rows g + 8 k
  // the sums of sample bs are complete -> this CU's half of the worker's row of that sample (8 lanes of a row, fixed order)
  auto flush = [&](int bs) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      float v = fs[k];
      v += __shfl_xor(v, 1, DHD_WAVE);
      v += __shfl_xor(v, 2, DHD_WAVE);
      v += __shfl_xor(v, 4, DHD_WAVE);
      if (q == 0) a.rows[(size_t)(slot.worker + bs) * C + cib + 16 * wv + g + 8 * k] = v;
      fs[k] = 0.f;
    }
  };

  f32x4 rg[4], ry[4], rxb[2], rxv[2];
  auto issue = [&](int s) {
    const int b = s / sps, p0 = (s - b * sps) * 32;
    const __amdgpu_buffer_rsrc_t sg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.g + (size_t)b * C * hw), 0, in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t sy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.y + (size_t)b * C * hw), 0, in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t sx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x + (size_t)b * 2 * C * hw), 0, x_bytes, 0x00020000);
    // a pixel quad beyond the row's end (last step of a sample, hw % 32 != 0) re-reads quad 0: it is staged as zeros
    const bool okq = p0 + 4 * q < hw;
    const int va = okq ? lda_voff : lda_voff - 16 * q, vb = okq ? ldb_voff : ldb_voff - 16 * q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      rg[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(sg, va, j * row_bytes + p0 * 4, AUX));
      ry[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(sy, va, j * row_bytes + p0 * 4, AUX));
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      rxb[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(sx, vb, 8 * k * row_bytes + p0 * 4, XAUX));
      rxv[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(sx, vb, (C + 8 * k) * row_bytes + p0 * 4, XAUX));
    }
  };

  __builtin_amdgcn_s_waitcnt(0x0F70);                          // vmcnt(0): weights and tables are complete before the loop (sfa_gemm_cu.h)
  cu_lds_barrier();                                            // publishes the prologue table and the first sample's blend coefficients
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
    const int s_next = first + min(it + 1, count - 1);         // past the end: the last step again, never staged
    const bool okq = p0 + 4 * q < hw;
    // ---- stage: prologue, one split, three images ------------------------------------------------------------------------
    // First everything that reads the raw rows, then the next step's loads into the registers that frees (pw_pair_kernel)
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
    f32x4 xd[2];                                               // x_bev - x_voxel of rows g + 8 k: the epilogue's factor
    float u[2][4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const f32x2 ab = *reinterpret_cast<const f32x2*>(ab_lds + 2 * (16 * wv + g + 8 * k));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float tu = fmaf(ab.x, rxb[k][e], 0.f);                 // pw_wgrad3_kernel's prologue: fma(a, x_bev, 0), then fma(1 - a, x_voxel, .)
        tu = fmaf(ab.y, rxv[k][e], tu);
        u[k][e] = okq ? tu : 0.f;
        xd[k][e] = rxb[k][e] - rxv[k][e];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    issue(s_next);
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
      static_for<4>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const unsigned* hs = j < 2 ? h01 : h23;
        const unsigned* ms = j < 2 ? m01 : m23;
        const unsigned sel = (j & 1) ? HI : LO;
        const u32x2 hq = {__builtin_amdgcn_perm(hs[1], hs[0], sel), __builtin_amdgcn_perm(hs[3], hs[2], sel)};
        const u32x2 mq = {__builtin_amdgcn_perm(ms[1], ms[0], sel), __builtin_amdgcn_perm(ms[3], ms[2], sel)};
        const int aw = xor_c(aw0, std::integral_constant<int, (j << 4)>{});
        *reinterpret_cast<u32x2*>(aimg + aw) = hq;
        *reinterpret_cast<u32x2*>(aimg + aw + 1024) = mq;
      });
    }
    static_for<2>([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      unsigned uh01, um01, uh23, um23;
      split2_hm(u[k][0], u[k][1], uh01, um01);
      split2_hm(u[k][2], u[k][3], uh23, um23);
      const int bw = xor_c(bw0, std::integral_constant<int, (k << 7)>{});
      *reinterpret_cast<u32x2*>(bimg + bw) = u32x2{uh01, uh23};
      *reinterpret_cast<u32x2*>(bimg + bw + 1024) = u32x2{um01, um23};
    });
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
    // ---- weight gradient: dW[co tiles of the wave][ci tiles of the wave] += gy u^T over the step's 32 pixels -----------------
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
    // ---- epilogue: patch transposition, du in whole lines, the sample's sum du (x_bev - x_voxel) ------------------------------
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
        const f32x4 o = *reinterpret_cast<const f32x4*>(patch + (g + 8 * k) * kPairPatchPitch + 4 * q);
        const f32x4 d = xd[k];
        const float t1 = (o.x * d.x + o.y * d.y) + (o.z * d.z + o.w * d.w);   // pw_wgrad3_kernel FOLD 2's pairwise form
        fs[k] += okq ? t1 : 0.f;
        store_b128_guarded<SAUX>(__builtin_bit_cast(u32x4, o), ro, voff, 8 * k * row_bytes + p0 * 4);
      }
    }
    // the next step belongs to another sample (workgroup-uniform): this sample's row goes out, the next one's coefficients come in
    const int b_next = s_next / sps;
    if (b_next != b) {
      flush(b);
      load_ab(b_next);
    }
    cu_lds_barrier();
  }

  // ---- this CU's columns of the worker's partial matrix (zeros from a worker without steps) and its half of the last row ----
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
  // the last sample's row; a worker without steps leaves a row of zeros for the sample its empty range lies in (pw_wgrad3_kernel)
  flush(count > 0 ? (first + count - 1) / sps : min(first / sps, a.nb - 1));
}

}  // namespace dhd_sfa
