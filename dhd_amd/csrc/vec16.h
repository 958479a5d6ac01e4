// Typed 16-byte access and dtype dispatch, shared by every operator of libdhd_amd.so that has a half-precision path.
//
// Device side: Pair<T> converts one 32-bit word of two T to two floats and back (registers only); widen16 / narrow16 do the
// same for 16 bytes = kVec16<T> elements, Vec16<T, NT> adds the memory access (NT: non-temporal or plain).  Widening is exact;
// narrowing rounds to nearest even.  For bfloat16 there are two roundings, and the element SPELLING selects it:
//   __hip_bfloat16  the integer formula bf16_rne (PyTorch's float -> bfloat16 for finite values; the carry can turn a
//                   NaN into Inf or, past the sign bit, into zero)
//   __bf16          the hardware convert (v_cvt_pk_bf16_f32; NaN stays NaN)
// They agree on every finite input and differ on NaN only.  Who uses what:
//
//   operator                                  spelling                    access             bfloat16 rounding
//   batchnorm.hip                             __half / __hip_bfloat16     non-temporal       integer formula
//   window.hip                                __half / __hip_bfloat16     plain              integer formula
//   upsample.hip                              __half / __hip_bfloat16     plain              integer formula
//   sfa_half.h (storage)                      _Float16 / __bf16           non-temporal       hardware convert
//   sfa_stage.hip element-wise (storage)      float / _Float16 / __bf16   per tensor (its    hardware convert
//                                                                         policy block)
//   sfa_stage.hip IoVec (edge tensors)        float / _Float16 / __bf16   non-temporal, 16 B hardware convert
//                                                                         or 8 B (half I/O on float32 storage)
//   mghs_pool.hip (dense views)               _Float16 / __bf16           non-temporal       hardware convert
//   deform.hip, mghs_softmax.hip (scalars)    _Float16 / __bf16           plain, per element hardware convert ((T)v)
//
// sfa_stage.hip's 8-byte IoVec store and mghs_pool.hip's pack_vox convert element by element ((T)v, the same hardware convert) instead of through
// Pair<T>::narrow: the pairwise form compiles to the same instructions in another order, and their kernels keep the order they have.
//
// Host side: with_dtype maps a DHD_F32 / DHD_F16 / DHD_BF16 code of the C ABI to an element type of either spelling.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <type_traits>

#include "common.h"

namespace dhd {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// float -> bfloat16 bits, round to nearest even by integer arithmetic
__device__ __forceinline__ unsigned bf16_rne(float f) {
  const unsigned u = __float_as_uint(f);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// two floats <-> a word of two bfloat16 (the first in the low half); the hardware convert
__device__ __forceinline__ unsigned pack_bf16(f32x2 v) { return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2)); }
__device__ __forceinline__ f32x2 unpack_bf16(unsigned p) {
  f32x2 r = {__uint_as_float(p << 16), __uint_as_float(p & 0xffff0000u)};
  return r;
}

template <class T> struct Pair;
template <> struct Pair<__half> {
  static __device__ __forceinline__ f32x2 widen(unsigned w) {
    const __half2 h = *reinterpret_cast<const __half2*>(&w);
    return f32x2{__low2float(h), __high2float(h)};
  }
  static __device__ __forceinline__ unsigned narrow(f32x2 v) {
    const __half2 h = __floats2half2_rn(v.x, v.y);
    return *reinterpret_cast<const unsigned*>(&h);
  }
};
template <> struct Pair<__hip_bfloat16> {
  static __device__ __forceinline__ f32x2 widen(unsigned w) { return unpack_bf16(w); }
  static __device__ __forceinline__ unsigned narrow(f32x2 v) { return bf16_rne(v.x) | (bf16_rne(v.y) << 16); }
};
template <> struct Pair<_Float16> {
  static __device__ __forceinline__ f32x2 widen(unsigned w) {
    const f16x2 h = __builtin_bit_cast(f16x2, w);
    return f32x2{(float)h.x, (float)h.y};
  }
  static __device__ __forceinline__ unsigned narrow(f32x2 v) { return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2)); }
};
template <> struct Pair<__bf16> {
  static __device__ __forceinline__ f32x2 widen(unsigned w) { return unpack_bf16(w); }
  static __device__ __forceinline__ unsigned narrow(f32x2 v) { return pack_bf16(v); }
};

// the value a float becomes when it is stored as T and read back
template <class T> __device__ __forceinline__ f32x2 round2(f32x2 v) {
  if constexpr (std::is_same_v<T, float>) return v;
  else return Pair<T>::widen(Pair<T>::narrow(v));
}

// 16 bytes of T in registers (f32x4 of float, u32x4 of a half type) <-> kVec16<T> floats
template <class T> constexpr int kVec16 = 16 / sizeof(T);
template <class T> using raw16 = std::conditional_t<std::is_same_v<T, float>, f32x4, u32x4>;
template <class T> __device__ __forceinline__ void widen16(raw16<T> w, float* v) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (std::is_same_v<T, float>) {
      v[i] = w[i];
    } else {
      const f32x2 p = Pair<T>::widen(w[i]);
      v[2 * i] = p.x;
      v[2 * i + 1] = p.y;
    }
  }
}
template <class T> __device__ __forceinline__ raw16<T> narrow16(const float* v) {
  raw16<T> w;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (std::is_same_v<T, float>) w[i] = v[i];
    else w[i] = Pair<T>::narrow(f32x2{v[2 * i], v[2 * i + 1]});
  }
  return w;
}

// 16-byte loads and stores of T (p 16-byte aligned), non-temporal (NT) or plain
template <class T, bool NT> struct Vec16 {
  static constexpr int N = kVec16<T>;
  // vector i of p, the 16 bytes as they are (widen16 them where they are used) ...
  static __device__ __forceinline__ raw16<T> ld(const T* p, size_t i = 0) {
    const raw16<T>* q = reinterpret_cast<const raw16<T>*>(p) + i;
    if constexpr (NT) return __builtin_nontemporal_load(q);
    else return *q;
  }
  static __device__ __forceinline__ void st(T* p, size_t i, raw16<T> w) {
    raw16<T>* q = reinterpret_cast<raw16<T>*>(p) + i;
    if constexpr (NT) __builtin_nontemporal_store(w, q);
    else *q = w;
  }
  // ... and as kVec16<T> floats
  static __device__ __forceinline__ void load(const T* p, size_t i, float* v) { widen16<T>(ld(p, i), v); }
  static __device__ __forceinline__ void load(const T* p, float* v) { load(p, 0, v); }
  static __device__ __forceinline__ void store(T* p, size_t i, const float* v) { st(p, i, narrow16<T>(v)); }
  static __device__ __forceinline__ void store(T* p, const float* v) { store(p, 0, v); }
};

// Host: the element type of a dtype code of the C ABI, in HIP's spelling (these appear in the mangled names of the batchnorm,
// window and upsample kernels) or the compiler's (SFA, MGHS, deform, softmax).
struct HipHalf { using f16 = __half; using bf16 = __hip_bfloat16; };
struct NativeHalf { using f16 = _Float16; using bf16 = __bf16; };

// f(p) with p a null pointer to the element type: `using T = std::remove_pointer_t<decltype(p)>`.  Two codes: nest two calls.
template <class Spelling, class F>
int with_dtype(int dtype, F&& f) {
  switch (dtype) {
    case DHD_F32: return f((float*)nullptr);
    case DHD_F16: return f((typename Spelling::f16*)nullptr);
    case DHD_BF16: return f((typename Spelling::bf16*)nullptr);
  }
  return DHD_EINVAL;
}

}  // namespace dhd
