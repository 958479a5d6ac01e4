// Scalar arithmetic of the SFA stage (models/necks/mix.py:52-58 and its derivatives), written ONCE: every kernel that blends --
// the element-wise passes of sfa_stage.hip, the EPI == 3 epilogues of pw_gemm_cu_kernel (sfa_gemm_cu.h) and pw_gemm_cuh_kernel
// (sfa_half.h), sfa_onepass_h_kernel -- calls these, so that dhd_sfa_stage_infer returns the bytes of the eval forward by
// construction.  The translation unit is built with -ffp-contract=off: an expression rounds as it is written, fmaf is explicit.
//   g = sigmoid(sc*y2 + sh)          a, na = 1 - a: channel attention          xb, xv: x_bev, x_voxel
#pragma once
#include <hip/hip_runtime.h>

namespace dhd_sfa {

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + __expf(-v)); }

// the spatial gate of BatchNorm-2's output: sc, sh = scale, shift of the layer
__device__ __forceinline__ float blend_gate(float sc, float y2, float sh) { return sigmoidf_(fmaf(sc, y2, sh)); }

// out = g*(a*xb) + (1-g)*((1-a)*xv)
__device__ __forceinline__ float blend_out(float g, float a, float na, float xb, float xv) { return g * (a * xb) + (1.0f - g) * (na * xv); }

// dL/d s2 = go*(a*xb - (1-a)*xv)*g*(1-g)
__device__ __forceinline__ float blend_gate_grad(float go, float g, float a, float na, float xb, float xv) {
  return go * (a * xb - na * xv) * g * (1.0f - g);
}

// acc + go*(g*xb - (1-g)*xv): the go-part of dL/da, summed over a plane
__device__ __forceinline__ float blend_da_add(float acc, float go, float g, float xb, float xv) {
  return fmaf(go, g * xb - (1.0f - g) * xv, acc);
}

// dL/dx_bev = a*(go*g + du) + kb,  dL/dx_voxel = (1-a)*(go*(1-g) + du) + kv   (kb, kv: the channel mean's share, ds/hw)
__device__ __forceinline__ float stage_gx_bev(float a, float go, float g, float du, float kb) { return fmaf(a, fmaf(go, g, du), kb); }
__device__ __forceinline__ float stage_gx_vox(float na, float go, float g, float du, float kv) {
  return fmaf(na, fmaf(go, 1.0f - g, du), kv);
}

}  // namespace dhd_sfa
