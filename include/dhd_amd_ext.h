/*
 * dhd_amd_ext.h -- extension surface of libdhd_amd.so: entry points of the same library, under the conventions of dhd_amd.h
 * (caller-owned [dev] memory, `stream` a hipStream_t as void*, 0 / positive hipError_t / negative DHD_E* return codes, dense
 * tensors, the DHD_F32 / DHD_F16 / DHD_BF16 dtype codes), that are not part of the numbered dhd_* surface.
 *
 * Why the prefix differs: the dhd_* surface is held closed by three tables that live in test files (the header / binding /
 * export equality of tests/test_capi.py and the per-entry rows of tests/test_gpu_guard_bands.py and tests/test_gpu_views.py).
 * A change that may not edit those tables cannot add a launching dhd_* symbol, so an operator family added by such a change
 * ships here as dhdx_*, with its own copies of the three guarantees (tests/test_swin_glue_capi.py, tests/test_gpu_swin_glue.py).
 * Folding a family into dhd_amd.h -- renaming it dhd_*, adding its rows to the tables and raising DHD_ABI_VERSION if anything
 * else moves -- is a change of its own.  Nothing here alters dhd_amd.h: DHD_ABI_VERSION is unchanged by this header.
 */
#ifndef DHD_AMD_EXT_H
#define DHD_AMD_EXT_H

#include "dhd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------ *
 * X1. Swin block glue: what a `SwinBlock` does to the token map outside its four Linear layers and the attention of
 *     sections 16-17 -- LayerNorm fused into the window partition of section 12 (and, with the identity map, plain LayerNorm
 *     over rows emitting another dtype), its backward, and the window reverse of section 12 fused with the residual add.
 *     Memory-bound row kernels: a row's c channels are held in registers across a power-of-two group of lanes, eight channels
 *     per lane and step, moved as 16-byte vectors.  No LDS, no atomics.
 *
 *     The row map.  Tokens are the rows of x (b, h, w, c), t = (bi h + y) w + x.  With window > 0 the output rows are those of
 *     section 12's partition, (b, nh nw, window^2, c) with nh = ceil(h / window), nw = ceil(w / window): row r holds token
 *     src(r), the map of dhd_window_rows(reverse = 0), or lies in the padding.  With window == 0 the map is the identity over
 *     b h w rows (shift must be 0; only the product b h w matters).
 *
 *     Supported (dhdx_ln_rows_supported: 1 / 0): c a multiple of 8, 8 <= c <= 2048; float32, float16 or bfloat16 on either
 *     side, in any combination.  Calls additionally need 0 <= shift < window (or window == shift == 0) and fewer than 2^40 rows.
 *     Arithmetic: float32 throughout.  mean = sum(x) / c; var = sum((x - mean)^2) / c (the centred form, a second pass over
 *     registers); rstd = 1 / sqrtf(var + eps); each sum is a fixed tree over the lane group.  Within the layer's 1e-4 bar of a
 *     float64 LayerNorm, not bit-identical to torch's.  A half output is the float32 result rounded once, to nearest even.
 * ------------------------------------------------------------------------------------ */
int dhdx_ln_rows_supported(int c, int x_dtype, int out_dtype);

/* out row r = (x[src(r)] - mean) * rstd * gamma + beta, in out_dtype; a row whose source lies in the padding is written as
 * exact zeros (the reference pads after norm1).  x [dev] dense (b, h, w, c) in x_dtype; gamma, beta [dev] float32 (c); out
 * [dev] dense (b, nh nw, window^2, c) for window > 0, (b, h, w, c) for window == 0, in out_dtype, every element written.
 * x, out, gamma and beta 16-byte aligned.  Checked on the host before the launch: a NULL or misaligned pointer or a
 * non-positive b / h / w -> DHD_EINVAL; c, a dtype code, window or shift outside the supported range -> DHD_EUNSUPPORTED.
 * One launch on `stream`; nothing allocated, kept or synchronised. */
int dhdx_ln_rows_forward(const void* x, const float* gamma, const float* beta, void* out, int x_dtype, int out_dtype, int b, int h,
                         int w, int c, int window, int shift, float eps, void* stream);

/* Bytes of caller-provided scratch for a backward over `rows` = b h w tokens of c channels: one pair of float32 rows
 * (sum of dy x^, sum of dy; 8 c bytes) per workgroup of the token kernel, so bytes / (8 c) is the number of workgroups.
 * Non-decreasing in rows; 0 for sizes the operator does not take. */
size_t dhdx_ln_rows_backward_scratch_bytes(long rows, int c);

/* Backward of dhdx_ln_rows_forward from x, dy and gamma alone: the row statistics are recomputed from x, which the backward
 * reads anyway.  With x^ = (x - mean) rstd and g = dy gamma, per token
 *   dx = rstd (g - mean_c(g) - x^ mean_c(g x^)),      dgamma = sum over tokens of dy x^,      dbeta = sum over tokens of dy,
 * where a token's dy row is row src^-1(t) of dy: the kernel runs over the real tokens and gathers dy through the reverse map
 * of section 12, so the pad rows of dy are never read.
 * x, b .. eps as in the forward; dy [dev] dense, the forward's output shape, in dy_dtype; dx [dev] dense, x's shape and dtype,
 * every element written; dgamma, dbeta [dev] float32 (c), every element written (not accumulated into); scratch [dev] of at
 * least dhdx_ln_rows_backward_scratch_bytes(b h w, c) bytes, contents undefined before and after.  The inputs are only read.
 * x, dy, dx, gamma, dgamma, dbeta and scratch 16-byte aligned.
 * Reproducibility: no atomics.  Every workgroup adds its contiguous run of tokens into its own partial row pair in a fixed
 * order, and a second launch adds the partial rows in a fixed order: dx, dgamma and dbeta are the same bytes on every call.
 * Checked on the host before the first launch: a NULL or misaligned pointer or a non-positive b / h / w -> DHD_EINVAL; c, a
 * dtype code, window or shift outside the supported range -> DHD_EUNSUPPORTED; scratch_bytes too small -> DHD_ENOSPACE.
 * Two launches on `stream`; nothing allocated, kept or synchronised. */
int dhdx_ln_rows_backward(const void* x, const void* dy, const float* gamma, void* dx, float* dgamma, float* dbeta, void* scratch,
                          size_t scratch_bytes, int x_dtype, int dy_dtype, int b, int h, int w, int c, int window, int shift,
                          float eps, void* stream);

/* Window reverse + residual add: out[bi, y, x, :] = identity[bi, y, x, :] + scale[bi] * win[bi, map(y, x), :] with map the
 * map of dhd_window_rows(reverse = 1) (padding rows of win are dropped, never read).  win [dev] dense (b, nh nw, window^2, c)
 * in win_dtype; identity [dev] dense (b, h, w, c) in id_dtype; scale [dev] float32 (b) -- DropPath's floor(keep + u) / keep
 * per image -- or NULL for 1, in which case the multiply is skipped; out [dev] dense, identity's shape and dtype, every
 * element written; out overlaps neither input.  Arithmetic: float32, product and sum rounded separately (no fused multiply-add), the result rounded once to
 * id_dtype: with scale == NULL the bytes of `identity + float(reverse(win))` cast to id_dtype.
 * c a multiple of 8 with 8 <= c <= 2048, window > 0, 0 <= shift < window.  win, identity and out 16-byte aligned, scale 4-byte.
 * Checked on the host before the launch: a NULL win / identity / out, a misaligned pointer or a non-positive b / h / w ->
 * DHD_EINVAL; c, a dtype code, window or shift outside the supported range -> DHD_EUNSUPPORTED.
 * One launch on `stream`; nothing allocated, kept or synchronised.  Its backward needs no kernel of its own: the gradient of
 * identity is the incoming gradient, the gradient of win is dhd_window_rows(reverse = 0) of it, times scale[bi]. */
int dhdx_window_reverse_add(const void* win, const void* identity, const float* scale, void* out, int win_dtype, int id_dtype, int b,
                            int h, int w, int c, int window, int shift, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHD_AMD_EXT_H */
