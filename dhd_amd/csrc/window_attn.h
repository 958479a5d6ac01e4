// What the forward (window_attn.hip) and the backward (window_attn_bwd.hip) of the Swin window attention share: the limits, the
// 16 x 16 x 32 MFMA with its fragment map, and the operand words of a token's 8 channels / of two probabilities.
#pragma once
#include <type_traits>

#include "sfa_mfma.h"

namespace dhd_window_attn {

using namespace dhd_sfa;

constexpr int kHeadDim = 32;
constexpr int kMaxN = 144;
constexpr int kMaxTiles = kMaxN / 16;         // key / query tiles of 16
constexpr int kMaxPairs = (kMaxTiles + 1) / 2;
constexpr int kMaxKeys2 = kMaxPairs * 32;     // keys of the V^T image
constexpr int kMaxTable = 23 * 23;            // (2 Wh - 1)(2 Ww - 1) with Wh Ww <= 144 is largest at 12 x 12
constexpr int kWaves = 3;
constexpr int kBlock = kWaves * 64;
constexpr int kVtStride = kMaxKeys2 + 4;      // halves per channel row of V^T: 328 bytes, 8-byte aligned, rows on different banks
// Blocks are handed to the XCDs in pairs of consecutive (window, head) items.  With an even head count and a half qkv the pair is
// heads 2k, 2k + 1 of one window, whose 64-byte rows share every 128-byte line; with an odd head count pairs straddle windows,
// and a float32 head is a full line already.  Speed only.
constexpr int kHeadsPerXcd = 2;

template <class T> constexpr int kParts = std::is_same_v<T, float> ? 2 : 1;

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

// D (16 x 16) += A (16 x 32) B (32 x 16); lane l holds A[l & 15][8 (l >> 4) + j], B[8 (l >> 4) + j][l & 15], D[4 (l >> 4) + r][l & 15]
template <class T> __device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
  if constexpr (std::is_same_v<T, _Float16>)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// 8 consecutive channels of one token as MFMA operand words: part 0 (and the bf16 remainder, part 1, of a float32 tensor)
template <class T> struct Frag { u32x4 part[kParts<T>]; };

template <class T> __device__ __forceinline__ Frag<T> zero_frag() {
  Frag<T> f;
#pragma unroll
  for (int p = 0; p < kParts<T>; ++p) f.part[p] = u32x4{0u, 0u, 0u, 0u};
  return f;
}

template <class T> __device__ __forceinline__ Frag<T> load_frag(const T* p) {
  Frag<T> f;
  if constexpr (std::is_same_v<T, float>) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    unsigned hi[4], mid[4];
    split2_hm(a[0], a[1], hi[0], mid[0]);
    split2_hm(a[2], a[3], hi[1], mid[1]);
    split2_hm(b[0], b[1], hi[2], mid[2]);
    split2_hm(b[2], b[3], hi[3], mid[3]);
    f.part[0] = u32x4{hi[0], hi[1], hi[2], hi[3]};
    f.part[1] = u32x4{mid[0], mid[1], mid[2], mid[3]};
  } else {
    f.part[0] = *reinterpret_cast<const u32x4*>(p);
  }
  return f;
}

// two probabilities -> one operand word per part
template <class T> __device__ __forceinline__ void pack_p(float a, float b, unsigned& h, unsigned& m) {
  if constexpr (std::is_same_v<T, float>) split2_hm(a, b, h, m);
  else h = Pair<T>::narrow(f32x2{a, b});
}

inline bool dtype_ok(int dtype) { return dtype == DHD_F32 || dtype == DHD_F16 || dtype == DHD_BF16; }
inline bool gemm_ok(int gemm) { return gemm >= DHD_SFA_GEMM_DEFAULT && gemm <= DHD_SFA_GEMM_BF16X3; }

// the support table of sections 16 and 17 of include/dhd_amd.h
inline int shape_supported(int wh, int ww, int nh, int head_dim, int dtype, int gemm) {
  if (head_dim != kHeadDim || wh < 1 || ww < 1 || wh > kMaxN || ww > kMaxN || wh * ww > kMaxN || nh < 1) return 0;
  if (!dtype_ok(dtype) || !gemm_ok(gemm)) return 0;
  if (dtype == DHD_F32 ? (gemm != DHD_SFA_GEMM_DEFAULT && gemm != DHD_SFA_GEMM_BF16X3) : gemm != DHD_SFA_GEMM_DEFAULT) return 0;
  return (long)wh * ww * 3 * nh * kHeadDim < (1L << 31) ? 1 : 0;      // one window's qkv
}

}  // namespace dhd_window_attn
