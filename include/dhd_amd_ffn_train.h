/*
 * dhd_amd_ffn_train.h -- the Swin FFN training surface of libdhd_amd.so: entry points of the same library, under the conventions
 * of dhd_amd.h (caller-owned [dev] memory, `stream` a hipStream_t as void*, 0 / positive hipError_t / negative DHD_E* return
 * codes, dense tensors, the DHD_F32 / DHD_F16 / DHD_BF16 dtype codes).
 *
 * Why a header and a prefix of its own: every other surface of the library is a closed list held by a table that lives in a
 * test file.  A change that may not edit those tables ships its family beside them as dhdt_*, with its own copies of the
 * guarantees (tests/test_swin_ffn_train_capi.py, tests/test_gpu_swin_ffn_train.py).  Nothing here alters another header:
 * DHD_ABI_VERSION is unchanged by this header.
 */
#ifndef DHD_AMD_FFN_TRAIN_H
#define DHD_AMD_FFN_TRAIN_H

#include "dhd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------ *
 * T1. Swin FFN in training: the second half of a `SwinBlock` with its DropPath, forward and backward.  For tokens x (rows, c)
 *     that are `rows / rows_per_image` images of `rows_per_image` rows each, and one float32 factor s per image:
 *
 *       xn  = LN(x; gamma, beta, eps)
 *       out = x + s[row / rows_per_image] (W2 . gelu(W1 . xn + b1) + b2)          exact (erf) GELU, hidden = 4 c
 *
 *     s is DropPath's draw, floor(keep + rand) / keep; scale == NULL means s = 1.  The factor is applied in float32 to the whole
 *     branch, before the residual add and the one rounding to x_dtype.  With scale == NULL the forward gives the bytes of the
 *     inference operator of the same library.  Nothing is saved by the forward: the backward takes x and recomputes.
 *
 *     The backward, for g = dout and gs = s g, per hidden tile in registers: h = W1 . xn + b1 again, da = W2^T . gs,
 *     a = gelu(h), dh = da gelu'(h) with gelu'(x) = Phi(x) + x phi(x) from the same erfc terms as the GELU, dxn += W1^T . dh;
 *     then the LayerNorm backward in float32 with x^ = (x - mean) rstd and dx^ = dxn gamma:
 *
 *       dx     = g + rstd (dx^ - mean(dx^) - x^ mean(dx^ x^))        rounded once to x_dtype
 *       dgamma = sum over rows of dxn x^,   dbeta = sum over rows of dxn
 *
 *     x is read three times and dout twice (the registers that held them carry the products in between).  The weight gradients
 *     are reductions over rows and are not computed here; on request the backward writes their operands
 *       xn (rows, c), act = a (rows, hidden), dhid = dh (rows, hidden)         dense, in mm_dtype, each rounded once to it
 *     so that dW1 = dhid^T . xn, db1 = sum dhid, dW2 = gs^T . act, db2 = sum gs.  With all three pointers NULL none is written
 *     (a frozen stage: only dx, dgamma, dbeta).
 *
 *     mm_dtype is what the GEMMs run in, as in the inference operator: DHD_F32 is three bf16 MFMA products of the two-part
 *     splits of both operands, smallest terms first; DHD_F16 / DHD_BF16 one product of operands rounded to that type.  float32
 *     accumulation; statistics, biases, GELU and its derivative, the factor and the LayerNorm backward are float32.
 *     Supported (dhdt_swin_ffn_supported: 1 / 0): c in {128, 256} with hidden == 4 c; x_dtype float32 with any mm_dtype, or
 *     x_dtype == mm_dtype.  The LayerNorm is required: gamma and beta are never NULL.  For c = 256 with mm_dtype float32 the
 *     registers of a wave do not hold xn and gs beside dxn: the backward loads x and dout again for every hidden tile (out of L2).
 *     Rows are independent in out, dx, xn, act and dhid: a NaN or infinity in a row of x or dout stays in that row (dgamma and
 *     dbeta are sums over all rows).  No atomics: two calls on the same bytes give the same bytes in every output.
 * ------------------------------------------------------------------------------------ */
int dhdt_swin_ffn_supported(int c, int hidden, int x_dtype, int mm_dtype);

/* Bytes of caller-provided scratch of a forward call: the weight stream of the inference operator.  0 for sizes or dtype codes
 * the operator does not take. */
size_t dhdt_swin_ffn_forward_scratch_bytes(int c, int hidden, int mm_dtype);

/* x [dev] dense (rows, c) in x_dtype; gamma, beta [dev] float32 (c); w1 [dev] float32 (hidden, c), b1 [dev] float32 (hidden),
 * w2 [dev] float32 (c, hidden), b2 [dev] float32 (c): nn.Linear's layouts; scale [dev] float32 (rows / rows_per_image) or NULL
 * (then rows_per_image is not looked at); out [dev] dense (rows, c) in x_dtype, every element written, overlapping no input;
 * scratch [dev] of at least dhdt_swin_ffn_forward_scratch_bytes(c, hidden, mm_dtype) bytes, contents undefined before and after
 * (the weights are laid out into it on every call: nothing is cached).  Every pointer 16-byte aligned.  1 <= rows <= 2^37.
 * Checked on the host before the first launch: a NULL (but scale) or misaligned pointer, rows <= 0, or with a scale
 * rows_per_image <= 0 or rows % rows_per_image != 0 -> DHD_EINVAL; c, hidden, a dtype code or a combination outside the
 * supported set, or rows > 2^37 -> DHD_EUNSUPPORTED; scratch_bytes too small -> DHD_ENOSPACE.
 * Two launches on `stream`; nothing allocated, kept or synchronised. */
int dhdt_swin_ffn_forward(const void* x, const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2,
                          const float* b2, const float* scale, long rows_per_image, void* out, void* scratch, size_t scratch_bytes,
                          int x_dtype, int mm_dtype, long rows, int c, int hidden, float eps, void* stream);

/* Bytes of caller-provided scratch of a backward call on `rows` rows: the backward's weight stream (b1 and three blocks of MFMA
 * fragments per hidden tile, plus what the read-ahead touches past its end) and one row of 2 c float32 partial sums per
 * workgroup of 128 rows.  0 for sizes, dtype codes or row counts the operator does not take. */
size_t dhdt_swin_ffn_backward_scratch_bytes(long rows, int c, int hidden, int mm_dtype);

/* x, dout [dev] dense (rows, c) in x_dtype; the parameters and scale as in the forward (b2 has no part in the backward);
 * dx [dev] dense (rows, c) in x_dtype; dgamma, dbeta [dev] float32 (c); xn [dev] (rows, c), act, dhid [dev] (rows, hidden) in
 * mm_dtype, all three given or all three NULL; every element of every output given is written, and no output overlaps an input
 * or another output; scratch [dev] of at least dhdt_swin_ffn_backward_scratch_bytes(rows, c, hidden, mm_dtype) bytes, contents
 * undefined before and after.  Every pointer 16-byte aligned.  1 <= rows <= 2^37.
 * Checked on the host before the first launch: a NULL (but scale and the operand triple) or misaligned pointer, one or two of
 * xn / act / dhid NULL, rows <= 0, or with a scale rows_per_image <= 0 or rows % rows_per_image != 0 -> DHD_EINVAL; outside the
 * supported set or rows > 2^37 -> DHD_EUNSUPPORTED; scratch_bytes too small -> DHD_ENOSPACE.
 * Three launches on `stream` (the weight stream, the operator, the parameter sums); nothing allocated, kept or synchronised. */
int dhdt_swin_ffn_backward(const void* x, const void* dout, const float* gamma, const float* beta, const float* w1, const float* b1,
                           const float* w2, const float* scale, long rows_per_image, void* dx, float* dgamma, float* dbeta, void* xn,
                           void* act, void* dhid, void* scratch, size_t scratch_bytes, int x_dtype, int mm_dtype, long rows, int c,
                           int hidden, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHD_AMD_FFN_TRAIN_H */
