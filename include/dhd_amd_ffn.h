/*
 * dhd_amd_ffn.h -- the Swin FFN surface of libdhd_amd.so: entry points of the same library, under the conventions of dhd_amd.h
 * (caller-owned [dev] memory, `stream` a hipStream_t as void*, 0 / positive hipError_t / negative DHD_E* return codes, dense
 * tensors, the DHD_F32 / DHD_F16 / DHD_BF16 dtype codes).
 *
 * Why a header and a prefix of its own: the dhd_* surface (dhd_amd.h) and the dhdx_* surface (dhd_amd_ext.h) are both closed
 * lists held by tables that live in test files (tests/test_capi.py, tests/test_swin_glue_capi.py).  A change that may not edit
 * those tables ships its family beside them as dhdf_*, with its own copies of the guarantees (tests/test_swin_ffn_capi.py,
 * tests/test_gpu_swin_ffn.py).  Nothing here alters dhd_amd.h or dhd_amd_ext.h: DHD_ABI_VERSION is unchanged by this header.
 */
#ifndef DHD_AMD_FFN_H
#define DHD_AMD_FFN_H

#include "dhd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------ *
 * F1. Swin FFN at inference: the second half of a `SwinBlock` (norm2, fc1, GELU, fc2, residual add) as one forward-only
 *     operator.  For tokens x (rows, c):
 *
 *       out = x + W2 . gelu(W1 . LN(x; gamma, beta, eps) + b1) + b2          exact (erf) GELU, hidden = 4 c
 *
 *     x is read once (twice for c = 256 with mm_dtype float32, see below) and out written once; the normalised rows and both
 *     (rows, hidden) tensors never reach memory.  With gamma == beta == NULL the LayerNorm is skipped: x + fc2(gelu(fc1(x))).
 *
 *     Two dtype codes.  x_dtype is the storage type of x and out.  mm_dtype is what the two Linear layers run in:
 *       DHD_F32            every product as three bf16 MFMA products of the two-part splits of both operands (bf16x3, as the
 *                          other float32 GEMMs of the library), float32 accumulation
 *       DHD_F16 / DHD_BF16 one MFMA product of operands rounded to that type, float32 accumulation; the LayerNorm output is
 *                          rounded once to it, the hidden activations once after the GELU
 *     Supported (dhdf_swin_ffn_supported: 1 / 0): c in {128, 256} with hidden == 4 c; (x_dtype, mm_dtype) with x_dtype float32
 *     and any mm_dtype (a block under autocast: the residual stream is float32), or x_dtype == mm_dtype (a half model).
 *     Arithmetic outside the products is float32: LayerNorm statistics (mean, then the centred sum of squares; rstd = 1 /
 *     sqrtf(var + eps)), biases, GELU (max(x, 0) - |x| erfc(|x| / sqrt 2) / 2 with erfc to 1.5e-7 absolute) and the residual
 *     add; the result is rounded once to x_dtype, to nearest even.
 *     Rows are independent: a row's result depends on no other row of the call, so a NaN or infinity stays in its row.  No
 *     atomics: two calls on the same bytes give the same bytes.
 * ------------------------------------------------------------------------------------ */
int dhdf_swin_ffn_supported(int c, int hidden, int x_dtype, int mm_dtype);

/* Bytes of caller-provided scratch of a call: the two weight matrices and b1 laid out as the stream of MFMA fragments the
 * kernel reads, plus the fragments its read-ahead touches past the end of the stream (read, never used, never written).
 * 0 for sizes or dtype codes the operator does not take. */
size_t dhdf_swin_ffn_scratch_bytes(int c, int hidden, int mm_dtype);

/* x [dev] dense (rows, c) in x_dtype; gamma, beta [dev] float32 (c), or both NULL for no LayerNorm; w1 [dev] float32 (hidden, c),
 * b1 [dev] float32 (hidden), w2 [dev] float32 (c, hidden), b2 [dev] float32 (c): nn.Linear's layouts; out [dev] dense (rows, c)
 * in x_dtype, every element written, overlapping no input; scratch [dev] of at least dhdf_swin_ffn_scratch_bytes(c, hidden,
 * mm_dtype) bytes, contents undefined before and after (the weights are laid out into it on every call: nothing is cached
 * across calls).  The inputs are only read.  Every pointer 16-byte aligned.  1 <= rows <= 2^37.
 * For c = 256 with mm_dtype float32 the registers of a wave do not hold the row beside both operands' parts, and the residual
 * add loads x a second time.
 * Checked on the host before the first launch: a NULL or misaligned pointer (gamma and beta: one of them NULL), or rows <= 0
 * -> DHD_EINVAL; c, hidden, a dtype code or a combination outside the supported set, or rows > 2^37 -> DHD_EUNSUPPORTED;
 * scratch_bytes too small -> DHD_ENOSPACE.
 * Two launches on `stream` (the weight stream, the operator); nothing allocated, kept or synchronised. */
int dhdf_swin_ffn_infer(const void* x, const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2,
                        const float* b2, void* out, void* scratch, size_t scratch_bytes, int x_dtype, int mm_dtype, long rows, int c,
                        int hidden, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHD_AMD_FFN_H */
