// Backward of the Swin window attention (section 17 of include/dhd_amd.h): from qkv (W, N, 3, nh, 32) and dout (W, N, nh * 32),
// both as they lie, to dqkv in qkv's layout and the gradient of the relative-position table.  The forward (window_attn.hip)
// saves nothing but its inputs: the scores and the softmax statistics are recomputed here, and delta_i = sum_j P_ij dP_ij comes
// from P and dP in registers, so neither `out` nor a log-sum-exp is needed.
//
// One workgroup of three waves per (run of windows, head); per window two passes, each shaped like the forward, over the same LDS:
//   pass A  the query on the lane, the keys in the accumulator registers (the forward's orientation).  LDS: K rows, V rows, K^T.
//           S^T = K Q^T and dP^T = V dO^T per key tile; row maximum, 1 / row sum and delta per query (kept in LDS for pass B);
//           dS^T = P^T o (dP^T - delta); dQ^T = scale K^T dS^T, with two key tiles of dS^T as the B operand where they lie.
//   pass B  the key on the lane, the queries in the registers.  LDS: Q rows, dO rows, Q^T, dO^T.
//           S = Q K^T and dP = dO V^T per query tile, P from the stored statistics, dS; dV^T = dO^T P and dK^T = scale Q^T dS
//           with two query tiles as the B operand.  A wave finishes its 16 keys' dK and dV alone.
// Pass B evaluates the scores again with the operand roles exchanged (Q rows x K fragment instead of K rows x Q fragment): in
// float32 the cross terms of the three bf16 products come in the other order, so its P can differ from pass A's in the last
// bits, and dQ (pass A's P) and dK / dV (pass B's P, normalised with pass A's maximum and sum) rest on slightly different P.
// Every element of dqkv is written by exactly one lane: no atomics, a fixed summation order, the same bytes from every call.
// dtable: pass A adds its float32 dS (before any rounding) into an LDS copy of the head's table column with LDS float atomics,
// one copy per wave; the workgroup adds its three copies in a fixed order and writes the column once, as one partial row of the
// scratch buffer, and a second launch adds the partial rows in a fixed order.  No global atomics.  A copy is written by one wave
// only, whose query tiles and atomic instructions come in program order, so the only order left open is that of the lanes of ONE
// instruction that hit the same offset, which the LDS takes in a fixed order: dtable has been the same bytes from every call
// wherever it was compared (tests/test_gpu_swin_composed.py: 8 tables, plain, repeated and under checkpointing).  With one copy
// shared by the three waves the order depended on their timing and the last one or two bits changed from run to run.
// Precisions as in the forward: float32 operands cut into two bf16 parts (three products per a * b, also for P and dS); half
// operands one product, P and dS rounded once to the type; scores, softmax, delta and dS arithmetic in float32.
#include "window_attn.h"

namespace {

using namespace dhd_window_attn;

constexpr int kMaxChunks = 512;               // runs of windows per head: the rows of the dtable partials

template <class T> struct LdsBwd {
  unsigned short rows[2][kParts<T>][kMaxN * kHeadDim];    // [token][channel], rows of 64 bytes.  Pass A: K, V.  Pass B: Q, dO
  unsigned short tr[2][kParts<T>][kHeadDim * kVtStride];  // [channel][token].  Pass A: K^T, -.  Pass B: Q^T, dO^T
  float table[(kMaxTable + 3) / 4 * 4];                   // the head's column of the bias table
  float dtab[kWaves][(kMaxTable + 3) / 4 * 4];            // its gradient, over the windows of this workgroup: one copy per wave
  float mx[kMaxN], inv[kMaxN], delta[kMaxN];              // per query: row maximum, 1 / row sum, sum_j P dP
  unsigned short kidx[kMaxKeys2];                         // y (2 Ww - 1) + x of a token
  unsigned char region[kMaxKeys2];
};

struct BwdShape {
  int items, chunks, wpc, windows, nw, n, ww, nh, tab_len, q0;   // items = chunks * nh; wpc windows per chunk
  float scale;
};

// `nt` tiles of 16 tokens x 32 channels of one head -> rows; tokens >= n are zeros
template <class T>
__device__ __forceinline__ void stage_rows(unsigned short (*dst)[kMaxN * kHeadDim], const T* src, unsigned stride, int n, int nt, int tid) {
  for (int c = tid; c < nt * 64; c += kBlock) {
    const int tok = c >> 2, cg = c & 3;
    const Frag<T> f = tok < n ? load_frag<T>(src + (unsigned)tok * stride + cg * 8) : zero_frag<T>();
#pragma unroll
    for (int p = 0; p < kParts<T>; ++p) *reinterpret_cast<u32x4*>(&dst[p][tok * kHeadDim + cg * 8]) = f.part[p];
  }
}

// the same, transposed: (two tokens, 8 channels) -> 8 words per part; `np` pairs of tiles
template <class T>
__device__ __forceinline__ void stage_transposed(unsigned short (*dst)[kHeadDim * kVtStride], const T* src, unsigned stride, int n, int np, int tid) {
  for (int c = tid; c < np * 64; c += kBlock) {
    const int tok = (c >> 2) * 2, cg = c & 3;
    const T* s = src + (unsigned)tok * stride + cg * 8;
    const Frag<T> a = tok < n ? load_frag<T>(s) : zero_frag<T>();
    const Frag<T> b = tok + 1 < n ? load_frag<T>(s + stride) : zero_frag<T>();
#pragma unroll
    for (int p = 0; p < kParts<T>; ++p) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned lo = (a.part[p][e >> 1] >> (16 * (e & 1))) & 0xffffu, hi = (b.part[p][e >> 1] >> (16 * (e & 1))) & 0xffffu;
        *reinterpret_cast<unsigned*>(&dst[p][(cg * 8 + e) * kVtStride + tok]) = lo | (hi << 16);
      }
    }
  }
}

// one 16 x 16 tile of rows (tile t) x fragment^T
template <class T>
__device__ __forceinline__ f32x4 rows_times_frag(const unsigned short (*rows)[kMaxN * kHeadDim], int t, int col, int g, const Frag<T>& f) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int off = (t * 16 + col) * kHeadDim + g * 8;
  const u32x4 r0 = *reinterpret_cast<const u32x4*>(&rows[0][off]);
  acc = mfma16<T>(r0, f.part[0], acc);
  if constexpr (kParts<T> == 2) {
    const u32x4 r1 = *reinterpret_cast<const u32x4*>(&rows[1][off]);
    acc = mfma16<T>(r0, f.part[1], acc);
    acc = mfma16<T>(r1, f.part[0], acc);
  }
  return acc;
}

// o[ct] += image[channels 16 ct ..][tokens of pair pp, in the order of the packed words] x (8 values per lane: x[0..3] of tile
// 2 pp, x[4..7] of tile 2 pp + 1, tokens 4 g + r of each)
template <class T>
__device__ __forceinline__ void transposed_times_pair(const unsigned short (*img)[kHeadDim * kVtStride], int pp, int col, int g, const float* x,
                                                      f32x4* o) {
  unsigned wh[4], wm[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 4; ++i) pack_p<T>(x[2 * i], x[2 * i + 1], wh[i], wm[i]);
  const u32x4 ph = {wh[0], wh[1], wh[2], wh[3]}, pm = {wm[0], wm[1], wm[2], wm[3]};
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int off = (ct * 16 + col) * kVtStride + pp * 32 + g * 4;
    const u32x2 a0 = *reinterpret_cast<const u32x2*>(&img[0][off]), a1 = *reinterpret_cast<const u32x2*>(&img[0][off + 16]);
    const u32x4 v0 = {a0[0], a0[1], a1[0], a1[1]};
    o[ct] = mfma16<T>(v0, ph, o[ct]);
    if constexpr (kParts<T> == 2) {
      const u32x2 b0 = *reinterpret_cast<const u32x2*>(&img[1][off]), b1 = *reinterpret_cast<const u32x2*>(&img[1][off + 16]);
      o[ct] = mfma16<T>(v0, pm, o[ct]);
      o[ct] = mfma16<T>(u32x4{b0[0], b0[1], b1[0], b1[1]}, ph, o[ct]);
    }
  }
}

// lane (token, g) holds channels 16 ct + 4 g + r of its token
template <class T> __device__ __forceinline__ void store_channels(T* dst, const f32x4* o, float mul) {
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const f32x4 y = o[ct] * mul;
    if constexpr (std::is_same_v<T, float>) {
      *reinterpret_cast<f32x4*>(dst + ct * 16) = y;
    } else {
      *reinterpret_cast<u32x2*>(dst + ct * 16) = u32x2{Pair<T>::narrow(f32x2{y[0], y[1]}), Pair<T>::narrow(f32x2{y[2], y[3]})};
    }
  }
}

template <class T>
__global__ __launch_bounds__(kBlock) void window_attn_bwd_kernel(const T* __restrict__ qkv, const T* __restrict__ dout,
                                                                  const float* __restrict__ table, const unsigned char* __restrict__ regions,
                                                                  T* __restrict__ dqkv, float* __restrict__ partial, BwdShape s) {
  __shared__ __attribute__((aligned(16))) LdsBwd<T> lds;
  const int item = xcd_grouped_tile(blockIdx.x, kHeadsPerXcd);
  if (item >= s.items) return;
  const int chunk = item / s.nh, h = item - chunk * s.nh;
  const int n = s.n, nt = (n + 15) >> 4, np = (nt + 1) >> 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const unsigned row_stride = 3u * s.nh * kHeadDim, do_stride = (unsigned)s.nh * kHeadDim;
  const unsigned k_off = do_stride, v_off = 2 * do_stride;            // from a token's q to its k and v

  for (int i = tid; i < s.tab_len; i += kBlock) {
    lds.table[i] = table[(unsigned)i * s.nh + h];
#pragma unroll
    for (int v = 0; v < kWaves; ++v) lds.dtab[v][i] = 0.f;
  }
  for (int j = tid; j < kMaxKeys2; j += kBlock) lds.kidx[j] = j < n ? (unsigned short)((j / s.ww) * (2 * s.ww - 1) + j % s.ww) : 0;

  const int w_end = min(s.windows, (chunk + 1) * s.wpc);
  for (int w = chunk * s.wpc; w < w_end; ++w) {
    const unsigned tok0 = (unsigned)w * n;
    const T* base = qkv + tok0 * row_stride + (unsigned)h * kHeadDim;          // q of token 0
    const T* dbase = dout + tok0 * do_stride + (unsigned)h * kHeadDim;
    T* gbase = dqkv + tok0 * row_stride + (unsigned)h * kHeadDim;

    // ---- pass A: K rows, V rows, K^T ----------------------------------------------------------------------------------------
    __syncthreads();                                                            // the previous window's pass B has read its images
    for (int j = tid; j < kMaxKeys2; j += kBlock) lds.region[j] = j < n && regions ? regions[(unsigned)(w % s.nw) * n + j] : 0;
    stage_rows<T>(lds.rows[0], base + k_off, row_stride, n, nt, tid);
    stage_rows<T>(lds.rows[1], base + v_off, row_stride, n, nt, tid);
    stage_transposed<T>(lds.tr[0], base + k_off, row_stride, n, np, tid);
    __syncthreads();

    for (int qt = wave; qt < nt; qt += kWaves) {
      const int qi = qt * 16 + col, qc = min(qi, n - 1);              // a padded query computes on zeros and is not stored
      const Frag<T> q = qi < n ? load_frag<T>(base + (unsigned)qi * row_stride + g * 8) : zero_frag<T>();
      const Frag<T> d = qi < n ? load_frag<T>(dbase + (unsigned)qi * do_stride + g * 8) : zero_frag<T>();
      const int qidx = lds.kidx[qc] + s.q0;
      const unsigned qreg = lds.region[qc];

      float sc[kMaxTiles][4], dp[kMaxTiles][4];                       // of this lane's query against keys 16 t + 4 g + r
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < kMaxTiles; ++t) {
        if (t < nt) {
          const f32x4 acc = rows_times_frag<T>(lds.rows[0], t, col, g, q);
          const f32x4 dacc = rows_times_frag<T>(lds.rows[1], t, col, g, d);
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
            dp[t][r] = dacc[r];                                       // 0 for a padded key: its V row is zeros
            mx = fmaxf(mx, v);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) { sc[t][r] = -INFINITY; dp[t][r] = 0.f; }
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, DHD_WAVE));
      mx = fmaxf(mx, __shfl_xor(mx, 32, DHD_WAVE));     // finite: key 0 is always real

      float sum = 0.f, dl = 0.f;
#pragma unroll
      for (int t = 0; t < kMaxTiles; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __expf(sc[t][r] - mx);        // 0 for a padded key
          sc[t][r] = e;
          sum += e;
          dl = fmaf(e, dp[t][r], dl);
        }
      }
      sum += __shfl_xor(sum, 16, DHD_WAVE);
      sum += __shfl_xor(sum, 32, DHD_WAVE);
      dl += __shfl_xor(dl, 16, DHD_WAVE);
      dl += __shfl_xor(dl, 32, DHD_WAVE);
      const float inv = 1.f / sum, delta = dl * inv;
      if (g == 0) {                                     // also for padded queries of the last tile (finite; pass B gives them weight 0)
        lds.mx[qi] = mx;
        lds.inv[qi] = inv;
        lds.delta[qi] = delta;
      }

      // ---- dS^T, its sum per table offset, dQ^T = scale K^T dS^T over pairs of key tiles -------------------------------------
      f32x4 o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int pp = 0; pp < kMaxPairs; ++pp) {
        if (pp < np) {
          float ds[8];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int t = 2 * pp + u;
            if (t < kMaxTiles && t < nt) {
              const int j0 = t * 16 + g * 4;
              const u32x2 kx = *reinterpret_cast<const u32x2*>(&lds.kidx[j0]);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float x = sc[t % kMaxTiles][r] * inv * (dp[t % kMaxTiles][r] - delta);
                ds[4 * u + r] = x;
                const int ki = (kx[r >> 1] >> (16 * (r & 1))) & 0xffff;
                if (qi < n && j0 + r < n) atomicAdd(&lds.dtab[wave][qidx - ki], x);
              }
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r) ds[4 * u + r] = 0.f;
            }
          }
          transposed_times_pair<T>(lds.tr[0], pp, col, g, ds, o);
        }
      }
      if (qi < n) store_channels<T>(gbase + (unsigned)qi * row_stride + g * 4, o, s.scale);
    }

    // ---- pass B: Q rows, dO rows, Q^T, dO^T -----------------------------------------------------------------------------------
    __syncthreads();
    stage_rows<T>(lds.rows[0], base, row_stride, n, nt, tid);
    stage_rows<T>(lds.rows[1], dbase, do_stride, n, nt, tid);
    stage_transposed<T>(lds.tr[0], base, row_stride, n, np, tid);
    stage_transposed<T>(lds.tr[1], dbase, do_stride, n, np, tid);
    __syncthreads();

    for (int kt = wave; kt < nt; kt += kWaves) {
      const int kj = kt * 16 + col, kc = min(kj, n - 1);              // a padded key computes on zeros and is not stored
      const Frag<T> kf = kj < n ? load_frag<T>(base + k_off + (unsigned)kj * row_stride + g * 8) : zero_frag<T>();
      const Frag<T> vf = kj < n ? load_frag<T>(base + v_off + (unsigned)kj * row_stride + g * 8) : zero_frag<T>();
      const int kidx = (int)lds.kidx[kc] - s.q0;
      const unsigned kreg = lds.region[kc];
      f32x4 dv[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, dk[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int pp = 0; pp < kMaxPairs; ++pp) {
        if (pp < np) {
          float p[8], ds[8];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int t = 2 * pp + u;
            if (t < kMaxTiles && t < nt) {
              const f32x4 acc = rows_times_frag<T>(lds.rows[0], t, col, g, kf);     // queries 16 t + 4 g + r against this lane's key
              const f32x4 dacc = rows_times_frag<T>(lds.rows[1], t, col, g, vf);
              const int i0 = t * 16 + g * 4;
              const u32x2 qx = *reinterpret_cast<const u32x2*>(&lds.kidx[i0]);
              const unsigned rg = *reinterpret_cast<const unsigned*>(&lds.region[i0]);
              const f32x4 m4 = *reinterpret_cast<const f32x4*>(&lds.mx[i0]), inv4 = *reinterpret_cast<const f32x4*>(&lds.inv[i0]),
                          del4 = *reinterpret_cast<const f32x4*>(&lds.delta[i0]);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int qi = (qx[r >> 1] >> (16 * (r & 1))) & 0xffff;
                float v = acc[r] * s.scale + lds.table[qi - kidx];
                if (((rg >> (8 * r)) & 0xffu) != kreg) v -= 100.f;
                const float pr = i0 + r < n && kj < n ? __expf(v - m4[r]) * inv4[r] : 0.f;
                p[4 * u + r] = pr;
                ds[4 * u + r] = pr * (dacc[r] - del4[r]);
              }
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r) p[4 * u + r] = ds[4 * u + r] = 0.f;
            }
          }
          transposed_times_pair<T>(lds.tr[1], pp, col, g, p, dv);
          transposed_times_pair<T>(lds.tr[0], pp, col, g, ds, dk);
        }
      }
      if (kj < n) {
        T* dst = gbase + (unsigned)kj * row_stride + g * 4;
        store_channels<T>(dst + k_off, dk, s.scale);
        store_channels<T>(dst + v_off, dv, 1.f);
      }
    }
  }

  __syncthreads();
  float* row = partial + ((unsigned)chunk * s.nh + h) * (unsigned)s.tab_len;
  static_assert(kWaves == 3, "the sum of the per-wave copies below is written out for three waves");
  for (int i = tid; i < s.tab_len; i += kBlock) row[i] = (lds.dtab[0][i] + lds.dtab[1][i]) + lds.dtab[2][i];
}

// dtable[r, h] = the partial rows of head h added in the order of the chunks
__global__ __launch_bounds__(256) void window_attn_dtable_kernel(const float* __restrict__ partial, float* __restrict__ dtable, int chunks, int nh,
                                                                  int tab_len) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= nh * tab_len) return;
  const int h = o / tab_len, r = o - h * tab_len;
  const unsigned step = (unsigned)nh * tab_len;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int c = 0;
  for (; c + 4 <= chunks; c += 4) {
    a0 += partial[(unsigned)c * step + o];
    a1 += partial[(unsigned)(c + 1) * step + o];
    a2 += partial[(unsigned)(c + 2) * step + o];
    a3 += partial[(unsigned)(c + 3) * step + o];
  }
  for (; c < chunks; ++c) a0 += partial[(unsigned)c * step + o];
  dtable[(unsigned)r * nh + h] = (a0 + a1) + (a2 + a3);
}

int chunk_rows(int windows) { return windows < kMaxChunks ? windows : kMaxChunks; }

}  // namespace

extern "C" {

int dhd_window_attn_backward_supported(int wh, int ww, int nh, int head_dim, int dtype, int gemm) {
  return shape_supported(wh, ww, nh, head_dim, dtype, gemm);
}

size_t dhd_window_attn_backward_scratch_bytes(int windows, int wh, int ww, int nh) {
  if (windows <= 0 || wh <= 0 || ww <= 0 || nh <= 0 || (long)wh * ww > kMaxN) return 0;
  return (size_t)chunk_rows(windows) * nh * ((2L * wh - 1) * (2L * ww - 1)) * sizeof(float);
}

int dhd_window_attn_backward(const void* qkv, const void* dout, int dtype, const float* table, const uint8_t* regions, void* dqkv,
                             float* dtable, void* scratch, size_t scratch_bytes, int windows, int nw, int wh, int ww, int nh, int head_dim,
                             float scale, int gemm, void* stream) {
  if (!qkv || !dout || !table || !dqkv || !dtable || !scratch) return DHD_EINVAL;
  if (windows <= 0 || nw <= 0 || wh <= 0 || ww <= 0 || nh <= 0 || head_dim <= 0 || windows % nw) return DHD_EINVAL;
  if (!dtype_ok(dtype) || !gemm_ok(gemm)) return DHD_EINVAL;
  if (!dhd_aligned(16, qkv, dout, dqkv) || !dhd_aligned(4, table, dtable, scratch)) return DHD_EINVAL;
  if (!shape_supported(wh, ww, nh, head_dim, dtype, gemm)) return DHD_EUNSUPPORTED;
  const long n = (long)wh * ww;
  if ((double)windows * n * 3 * nh * kHeadDim >= 2147483648.0) return DHD_EUNSUPPORTED;   // element offsets in 32 bits on the device
  if (scratch_bytes < dhd_window_attn_backward_scratch_bytes(windows, wh, ww, nh)) return DHD_ENOSPACE;
  BwdShape s;
  s.wpc = (windows + kMaxChunks - 1) / kMaxChunks;
  s.chunks = (windows + s.wpc - 1) / s.wpc;          // <= chunk_rows(windows)
  s.items = s.chunks * nh;
  s.windows = windows;
  s.nw = nw;
  s.n = (int)n;
  s.ww = ww;
  s.nh = nh;
  s.tab_len = (2 * wh - 1) * (2 * ww - 1);
  s.q0 = (wh - 1) * (2 * ww - 1) + ww - 1;
  s.scale = scale;
  float* partial = static_cast<float*>(scratch);
  const dim3 grid((unsigned)xcd_grouped_blocks(s.items, kHeadsPerXcd));
  return dhd::with_dtype<dhd::NativeHalf>(dtype, [&](auto* tp) {
    using T = std::remove_pointer_t<decltype(tp)>;
    hipLaunchKernelGGL(window_attn_bwd_kernel<T>, grid, dim3(kBlock), 0, dhd_stream(stream), static_cast<const T*>(qkv),
                       static_cast<const T*>(dout), table, regions, static_cast<T*>(dqkv), partial, s);
    DHD_LAUNCH_CHECK();
    hipLaunchKernelGGL(window_attn_dtable_kernel, dim3((unsigned)dhd_cdiv((long)nh * s.tab_len, 256)), dim3(256), 0, dhd_stream(stream), partial,
                       dtable, s.chunks, nh, s.tab_len);
    DHD_LAUNCH_CHECK();
    return (int)DHD_OK;
  });
}

}  // extern "C"
