/*
 * dhd_amd_ffn_wide_train.h -- the Swin FFN training surface of libdhd_amd.so for C = 512: entry points of the same library, under
 * the conventions of dhd_amd.h (caller-owned [dev] memory, `stream` a hipStream_t as void*, 0 / positive hipError_t / negative
 * DHD_E* return codes, dense tensors, the DHD_F32 / DHD_F16 / DHD_BF16 dtype codes).
 *
 * Why a header of its own, and why here: every other surface of the library is a closed list held by a table that lives in a
 * test file, and the listing of include/ itself is such a list (its six headers are named by two tests).  A change that may not
 * edit those tables ships its family beside them as dhdu_*, in the package's own include directory, with its own copies of the
 * guarantees (tests/test_swin_ffn_wide_train_capi.py, tests/test_gpu_swin_ffn_wide_train.py).  Compile with both directories on
 * the include path.  Nothing here alters another header: DHD_ABI_VERSION is unchanged by this header.
 */
#ifndef DHD_AMD_FFN_WIDE_TRAIN_H
#define DHD_AMD_FFN_WIDE_TRAIN_H

#include "dhd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------ *
 * U1. Swin FFN in training at C = 512 (DHD-L's stage 2): what dhd_amd_ffn_train.h section T1 defines, formula for formula and
 *     rounding point for rounding point,
 *
 *       xn  = LN(x; gamma, beta, eps)
 *       out = x + s[row / rows_per_image] (W2 . gelu(W1 . xn + b1) + b2)          exact (erf) GELU, hidden = 4 c
 *       dx  = g + rstd (dx^ - mean(dx^) - x^ mean(dx^ x^)),  dgamma = sum_rows dxn x^,  dbeta = sum_rows dxn
 *
 *     in the form of the wide inference family: a workgroup of four waves owns T rows (64 with half GEMMs, 32 with float32
 *     GEMMs), the normalised rows and the scaled gradient gs = s g live in two tiles of its local memory, and every weight byte
 *     is fetched once per workgroup.  The forward is the wide inference kernel with the per-image factor applied in float32 to
 *     the whole branch before the residual add and the one rounding: with scale == NULL it gives the bytes of the wide inference
 *     operator.  The backward recomputes the hidden chunk by chunk (h = W1 . xn + b1, da = W2^T . gs, dh = da gelu'(h),
 *     dxn += W1^T . dh) and on request writes the weight-gradient operands
 *       xn (rows, c), act = gelu(h) (rows, hidden), dhid = dh (rows, hidden)       dense, in mm_dtype, each rounded once to it
 *     so that dW1 = dhid^T . xn, db1 = sum dhid, dW2 = gs^T . act, db2 = sum gs.  With all three pointers NULL none is written.
 *
 *     mm_dtype as in T1: DHD_F32 is three bf16 MFMA products of the two-part splits, smallest terms first; DHD_F16 / DHD_BF16
 *     one product of operands rounded to that type.  float32 accumulation; statistics, biases, GELU and its derivative, the
 *     factor and the LayerNorm backward are float32.
 *     Supported (dhdu_swin_ffn_wide_supported: 1 / 0): c == 512 with hidden == 2048; x_dtype float32 with any mm_dtype, or
 *     x_dtype == mm_dtype.  The LayerNorm is required: gamma and beta are never NULL.  c = 1024 has no training operator.
 *     Rows are independent in out, dx, xn, act and dhid: a NaN or infinity in a row of x or dout stays in that row (dgamma and
 *     dbeta are sums over all rows).  No atomics: two calls on the same bytes give the same bytes in every output.
 * ------------------------------------------------------------------------------------ */
int dhdu_swin_ffn_wide_supported(int c, int hidden, int x_dtype, int mm_dtype);

/* Bytes of caller-provided scratch of a forward call: the weight stream of the wide inference operator.  0 for sizes or dtype
 * codes the operator does not take. */
size_t dhdu_swin_ffn_wide_forward_scratch_bytes(int c, int hidden, int mm_dtype);

/* x [dev] dense (rows, c) in x_dtype; gamma, beta [dev] float32 (c); w1 [dev] float32 (hidden, c), b1 [dev] float32 (hidden),
 * w2 [dev] float32 (c, hidden), b2 [dev] float32 (c): nn.Linear's layouts; scale [dev] float32 (rows / rows_per_image) or NULL
 * (then rows_per_image is not looked at); out [dev] dense (rows, c) in x_dtype, every element written, overlapping no input;
 * scratch [dev] of at least dhdu_swin_ffn_wide_forward_scratch_bytes(c, hidden, mm_dtype) bytes, contents undefined before and
 * after (the weights are laid out into it on every call: nothing is cached).  Every pointer 16-byte aligned.  1 <= rows <= 2^36.
 * Checked on the host before the first launch: a NULL (but scale) or misaligned pointer, rows <= 0, or with a scale
 * rows_per_image <= 0 or rows % rows_per_image != 0 -> DHD_EINVAL; c, hidden, a dtype code or a combination outside the
 * supported set, or rows > 2^36 -> DHD_EUNSUPPORTED; scratch_bytes too small -> DHD_ENOSPACE.
 * Two launches on `stream`; nothing allocated, kept or synchronised. */
int dhdu_swin_ffn_wide_forward(const void* x, const float* gamma, const float* beta, const float* w1, const float* b1,
                               const float* w2, const float* b2, const float* scale, long rows_per_image, void* out, void* scratch,
                               size_t scratch_bytes, int x_dtype, int mm_dtype, long rows, int c, int hidden, float eps, void* stream);

/* Bytes of caller-provided scratch of a backward call on `rows` rows: the backward's weight stream (per wave and hidden chunk b1
 * and three blocks of MFMA fragments, plus what the read-ahead touches past its end) and one row of 2 c float32 partial sums per
 * workgroup of T rows.  0 for sizes, dtype codes or row counts the operator does not take. */
size_t dhdu_swin_ffn_wide_backward_scratch_bytes(long rows, int c, int hidden, int mm_dtype);

/* x, dout [dev] dense (rows, c) in x_dtype; the parameters and scale as in the forward (b2 has no part in the backward);
 * dx [dev] dense (rows, c) in x_dtype; dgamma, dbeta [dev] float32 (c); xn [dev] (rows, c), act, dhid [dev] (rows, hidden) in
 * mm_dtype, all three given or all three NULL; every element of every output given is written, and no output overlaps an input
 * or another output; scratch [dev] of at least dhdu_swin_ffn_wide_backward_scratch_bytes(rows, c, hidden, mm_dtype) bytes,
 * contents undefined before and after.  Every pointer 16-byte aligned.  1 <= rows <= 2^36.
 * Checked on the host before the first launch: a NULL (but scale and the operand triple) or misaligned pointer, one or two of
 * xn / act / dhid NULL, rows <= 0, or with a scale rows_per_image <= 0 or rows % rows_per_image != 0 -> DHD_EINVAL; outside the
 * supported set or rows > 2^36 -> DHD_EUNSUPPORTED; scratch_bytes too small -> DHD_ENOSPACE.
 * Three launches on `stream` (the weight stream, the operator, the parameter sums); nothing allocated, kept or synchronised. */
int dhdu_swin_ffn_wide_backward(const void* x, const void* dout, const float* gamma, const float* beta, const float* w1,
                                const float* b1, const float* w2, const float* scale, long rows_per_image, void* dx, float* dgamma,
                                float* dbeta, void* xn, void* act, void* dhid, void* scratch, size_t scratch_bytes, int x_dtype,
                                int mm_dtype, long rows, int c, int hidden, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHD_AMD_FFN_WIDE_TRAIN_H */
