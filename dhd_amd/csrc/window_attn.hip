// Swin window attention at inference (section 16 of include/dhd_amd.h): from the qkv projection's output (W, N, 3, nh, 32),
// as it lies, to the tensor `proj` reads, (W, N, nh * 32), in one launch.  The scores, the probabilities, the expanded
// relative-position bias / shift mask and the permuted q / k / v never reach memory.
//
// One workgroup of three waves per (window, head).  The head's K rows go to LDS as they are, V goes there transposed
// ([channel][key], written in pairs of keys), the head's column of the bias table, the keys' table offsets and their region
// ids beside them.  A wave then owns 16 queries at a time:
//   S^T = K Q^T   one v_mfma_f32_16x16x32 per 16 keys (K = 32 = the head dimension).  The orientation puts the query on the
//                 lane and the keys in the accumulator registers, so
//   softmax       is a reduction over registers and two cross-lane steps (lanes l, l ^ 16, l ^ 32 share a query), float32, and
//   O^T = V^T P^T takes the probabilities of two key tiles as its B operand without moving them: lane (query, g) holds the keys
//                 16 t + 4 g + r of tile t, so element j of the fragment is key 16 t0 + 4 g + j (j < 4) or 16 t1 + 4 g + j - 4,
//                 and the A operand reads V^T in that same key order (two 8-byte LDS reads).
// N is padded to a multiple of 16 (32 for the second product) in LDS only: padded rows are written as zeros, never loaded, their
// scores are -inf (weight exactly 0), and padded queries are never stored.
// float32 qkv: every operand is cut into two bf16 parts (sfa_mfma.h split2_hm), three products per a*b, also for P.
#include "window_attn.h"

namespace {

using namespace dhd_window_attn;

template <class T> struct Lds {
  unsigned short k[kParts<T>][kMaxN * kHeadDim];          // [key][channel], rows of 64 bytes
  unsigned short vt[kParts<T>][kHeadDim * kVtStride];     // [channel][key]
  float table[(kMaxTable + 3) / 4 * 4];                   // the head's column of the bias table (what follows stays 16-byte aligned)
  unsigned short kidx[kMaxKeys2];                         // y (2 Ww - 1) + x of a key
  unsigned char region[kMaxKeys2];
};

struct Shape {
  int items, nw, n, ww, nh, tab_len, q0;   // q0 = (Wh - 1)(2 Ww - 1) + Ww - 1
  float scale;
};

template <class T>
__global__ __launch_bounds__(kBlock) void window_attn_kernel(const T* __restrict__ qkv, const float* __restrict__ table,
                                                              const unsigned char* __restrict__ regions, T* __restrict__ out, Shape s) {
  constexpr int P = kParts<T>;
  __shared__ __attribute__((aligned(16))) Lds<T> lds;
  const int item = xcd_grouped_tile(blockIdx.x, kHeadsPerXcd);
  if (item >= s.items) return;
  const int w = item / s.nh, h = item - w * s.nh;
  const int n = s.n, nt = (n + 15) >> 4, np = (nt + 1) >> 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned row_stride = 3u * s.nh * kHeadDim;                 // elements from one token's q to the next token's
  const T* base = qkv + (unsigned)w * n * row_stride + (unsigned)h * kHeadDim;

  // ---- stage the head: bias column, key offsets and regions, K, V^T --------------------------------------------------------
  for (int i = tid; i < s.tab_len; i += kBlock) lds.table[i] = table[(unsigned)i * s.nh + h];
  for (int j = tid; j < np * 32; j += kBlock) {
    const bool real = j < n;
    lds.kidx[j] = real ? (unsigned short)((j / s.ww) * (2 * s.ww - 1) + j % s.ww) : 0;
    lds.region[j] = real && regions ? regions[(unsigned)(w % s.nw) * n + j] : 0;
  }
  for (int c = tid; c < nt * 64; c += kBlock) {                      // K: (key, 8 channels) -> 16 bytes per part
    const int key = c >> 2, cg = c & 3;
    const Frag<T> f = key < n ? load_frag<T>(base + (unsigned)key * row_stride + s.nh * kHeadDim + cg * 8) : zero_frag<T>();
#pragma unroll
    for (int p = 0; p < P; ++p) *reinterpret_cast<u32x4*>(&lds.k[p][key * kHeadDim + cg * 8]) = f.part[p];
  }
  for (int c = tid; c < np * 64; c += kBlock) {                      // V^T: (two keys, 8 channels) -> 8 words per part
    const int key = (c >> 2) * 2, cg = c & 3;
    const T* src = base + (unsigned)key * row_stride + 2 * s.nh * kHeadDim + cg * 8;
    const Frag<T> a = key < n ? load_frag<T>(src) : zero_frag<T>();
    const Frag<T> b = key + 1 < n ? load_frag<T>(src + row_stride) : zero_frag<T>();
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned lo = (a.part[p][e >> 1] >> (16 * (e & 1))) & 0xffffu, hi = (b.part[p][e >> 1] >> (16 * (e & 1))) & 0xffffu;
        *reinterpret_cast<unsigned*>(&lds.vt[p][(cg * 8 + e) * kVtStride + key]) = lo | (hi << 16);
      }
    }
  }
  __syncthreads();

  const int col = lane & 15, g = lane >> 4;
  for (int qt = wave; qt < nt; qt += kWaves) {
    const int qi = qt * 16 + col, qc = min(qi, n - 1);              // a padded query computes on zeros and is not stored
    const Frag<T> q = qi < n ? load_frag<T>(base + (unsigned)qi * row_stride + g * 8) : zero_frag<T>();
    const int qidx = (qc / s.ww) * (2 * s.ww - 1) + qc % s.ww + s.q0;
    const unsigned qreg = lds.region[qc];

    // ---- S^T = K Q^T, then the scores of this lane's query against keys 16 t + 4 g + r ------------------------------------
    float sc[kMaxTiles][4];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < kMaxTiles; ++t) {
      if (t < nt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int off = (t * 16 + col) * kHeadDim + g * 8;
        const u32x4 k0 = *reinterpret_cast<const u32x4*>(&lds.k[0][off]);
        acc = mfma16<T>(k0, q.part[0], acc);
        if constexpr (P == 2) {
          const u32x4 k1 = *reinterpret_cast<const u32x4*>(&lds.k[1][off]);
          acc = mfma16<T>(k0, q.part[1], acc);
          acc = mfma16<T>(k1, q.part[0], acc);
        }
        const int j0 = t * 16 + g * 4;
        const u32x2 kx = *reinterpret_cast<const u32x2*>(&lds.kidx[j0]);
        const unsigned rg = *reinterpret_cast<const unsigned*>(&lds.region[j0]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ki = (kx[r >> 1] >> (16 * (r & 1))) & 0xffff;
          float v = acc[r] * s.scale + lds.table[qidx - ki];
          if (((rg >> (8 * r)) & 0xffu) != qreg) v -= 100.f;
          if (j0 + r >= n) v = -INFINITY;
          sc[t][r] = v;
          mx = fmaxf(mx, v);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[t][r] = -INFINITY;
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, DHD_WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, 32, DHD_WAVE));     // finite: key 0 is always real

    // ---- exponentials (float32 sum), O^T = V^T P^T over pairs of key tiles -------------------------------------------------
    float sum = 0.f;
    f32x4 o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int pp = 0; pp < kMaxPairs; ++pp) {
      if (pp < np) {
        float e[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          e[r] = __expf(sc[2 * pp][r] - mx);
          e[4 + r] = 2 * pp + 1 < kMaxTiles ? __expf(sc[(2 * pp + 1) % kMaxTiles][r] - mx) : 0.f;
        }
        unsigned wh[4], wm[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          sum += e[2 * i] + e[2 * i + 1];
          pack_p<T>(e[2 * i], e[2 * i + 1], wh[i], wm[i]);
        }
        const u32x4 ph = {wh[0], wh[1], wh[2], wh[3]}, pm = {wm[0], wm[1], wm[2], wm[3]};
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const int off = (ct * 16 + col) * kVtStride + pp * 32 + g * 4;
          u32x4 v0;
          const u32x2 a0 = *reinterpret_cast<const u32x2*>(&lds.vt[0][off]), a1 = *reinterpret_cast<const u32x2*>(&lds.vt[0][off + 16]);
          v0 = u32x4{a0[0], a0[1], a1[0], a1[1]};
          o[ct] = mfma16<T>(v0, ph, o[ct]);
          if constexpr (P == 2) {
            const u32x2 b0 = *reinterpret_cast<const u32x2*>(&lds.vt[1][off]), b1 = *reinterpret_cast<const u32x2*>(&lds.vt[1][off + 16]);
            o[ct] = mfma16<T>(v0, pm, o[ct]);
            o[ct] = mfma16<T>(u32x4{b0[0], b0[1], b1[0], b1[1]}, ph, o[ct]);
          }
        }
      }
    }
    sum += __shfl_xor(sum, 16, DHD_WAVE);
    sum += __shfl_xor(sum, 32, DHD_WAVE);
    const float inv = 1.f / sum;

    // ---- lane (query, g) holds channels 16 ct + 4 g + r of its query -------------------------------------------------------
    if (qi < n) {
      T* dst = out + ((unsigned)w * n + qi) * (unsigned)(s.nh * kHeadDim) + h * kHeadDim + g * 4;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const f32x4 y = o[ct] * inv;
        if constexpr (std::is_same_v<T, float>) {
          *reinterpret_cast<f32x4*>(dst + ct * 16) = y;
        } else {
          *reinterpret_cast<u32x2*>(dst + ct * 16) = u32x2{Pair<T>::narrow(f32x2{y[0], y[1]}), Pair<T>::narrow(f32x2{y[2], y[3]})};
        }
      }
    }
  }
}

}  // namespace

extern "C" {

int dhd_window_attn_infer_supported(int wh, int ww, int nh, int head_dim, int dtype, int gemm) {
  return shape_supported(wh, ww, nh, head_dim, dtype, gemm);
}

int dhd_window_attn_infer(const void* qkv, int dtype, const float* table, const uint8_t* regions, void* out, int windows, int nw,
                          int wh, int ww, int nh, int head_dim, float scale, int gemm, void* stream) {
  if (!qkv || !table || !out) return DHD_EINVAL;
  if (windows <= 0 || nw <= 0 || wh <= 0 || ww <= 0 || nh <= 0 || head_dim <= 0 || windows % nw) return DHD_EINVAL;
  if (!dtype_ok(dtype) || !gemm_ok(gemm)) return DHD_EINVAL;
  if (!dhd_aligned(16, qkv, out) || !dhd_aligned(4, table)) return DHD_EINVAL;
  if (!dhd_window_attn_infer_supported(wh, ww, nh, head_dim, dtype, gemm)) return DHD_EUNSUPPORTED;
  const long n = (long)wh * ww;
  if ((double)windows * n * 3 * nh * kHeadDim >= 2147483648.0) return DHD_EUNSUPPORTED;   // element offsets in 32 bits on the device
  Shape s;
  s.items = windows * nh;
  s.nw = nw;
  s.n = (int)n;
  s.ww = ww;
  s.nh = nh;
  s.tab_len = (2 * wh - 1) * (2 * ww - 1);
  s.q0 = (wh - 1) * (2 * ww - 1) + ww - 1;
  s.scale = scale;
  const dim3 grid((unsigned)xcd_grouped_blocks(s.items, kHeadsPerXcd));
  return dhd::with_dtype<dhd::NativeHalf>(dtype, [&](auto* tp) {
    using T = std::remove_pointer_t<decltype(tp)>;
    hipLaunchKernelGGL(window_attn_kernel<T>, grid, dim3(kBlock), 0, dhd_stream(stream), static_cast<const T*>(qkv), table, regions,
                       static_cast<T*>(out), s);
    DHD_LAUNCH_CHECK();
    return (int)DHD_OK;
  });
}

}  // extern "C"
