/*
 * dhd_amd_ffn_wide.h -- the wide Swin FFN surface of libdhd_amd.so: entry points of the same library, under the conventions of
 * dhd_amd.h (caller-owned [dev] memory, `stream` a hipStream_t as void*, 0 / positive hipError_t / negative DHD_E* return codes,
 * dense tensors, the DHD_F32 / DHD_F16 / DHD_BF16 dtype codes).
 *
 * Why a header and a prefix of its own: the dhd_*, dhdx_* and dhdf_* surfaces (dhd_amd.h, dhd_amd_ext.h, dhd_amd_ffn.h) are
 * closed lists held by tables that live in test files; dhdf_swin_ffn_supported(512, 2048, ...) is pinned at 0 there.  The kernel
 * family for c = 512 and 1024 therefore ships beside them as dhdg_*, with its own copies of the guarantees
 * (tests/test_swin_ffn_wide_capi.py, tests/test_gpu_swin_ffn_wide.py).  Nothing here alters the other three headers:
 * DHD_ABI_VERSION is unchanged by this header.
 */
#ifndef DHD_AMD_FFN_WIDE_H
#define DHD_AMD_FFN_WIDE_H

#include "dhd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------ *
 * G1. Swin FFN at inference for the wide stages: the operator of dhd_amd_ffn.h, section F1, for c in {512, 1024}.  For tokens
 *     x (rows, c):
 *
 *       out = x + W2 . gelu(W1 . LN(x; gamma, beta, eps) + b1) + b2          exact (erf) GELU, hidden = 4 c
 *
 *     x is read twice (once for the LayerNorm, once for the residual add) and out written once, in 16-byte accesses; the
 *     normalised rows and both (rows, hidden) tensors never reach memory.  With gamma == beta == NULL the LayerNorm is skipped:
 *     x + fc2(gelu(fc1(x))).
 *
 *     Two dtype codes.  x_dtype is the storage type of x and out.  mm_dtype is what the two Linear layers run in:
 *       DHD_F32            every product as three bf16 MFMA products of the two-part splits of both operands (bf16x3, as the
 *                          other float32 GEMMs of the library), float32 accumulation
 *       DHD_F16 / DHD_BF16 one MFMA product of operands rounded to that type, float32 accumulation; the LayerNorm output is
 *                          rounded once to it, the hidden activations once after the GELU; pre-activations are never rounded
 *     Supported (dhdg_swin_ffn_wide_supported: 1 / 0): c in {512, 1024} with hidden == 4 c; (x_dtype, mm_dtype) with x_dtype
 *     float32 and any mm_dtype (a block under autocast: the residual stream is float32), or x_dtype == mm_dtype (a half model).
 *     Arithmetic outside the products is float32: LayerNorm statistics (mean, then the centred sum of squares; rstd = 1 /
 *     sqrtf(var + eps)), biases, GELU (the same function as F1: max(x, 0) - |x| erfc(|x| / sqrt 2) / 2 with erfc to 1.5e-7
 *     absolute) and the residual add; the result is rounded once to x_dtype, to nearest even.
 *     A workgroup owns 96 or 64 rows (mm_dtype a half type, c = 512 or 1024) or 32 rows (float32) and shares the weights among
 *     them; rows are still independent: a row's result depends on no other row of the call, so a NaN or infinity stays in
 *     its row.  No atomics: two calls on the same bytes give the same bytes.
 * ------------------------------------------------------------------------------------ */
int dhdg_swin_ffn_wide_supported(int c, int hidden, int x_dtype, int mm_dtype);

/* Bytes of caller-provided scratch of a call: the two weight matrices and b1 laid out as the four per-wave streams of MFMA
 * fragments the kernel reads, plus the fragments the last wave's read-ahead touches past the end (read, never used, never
 * written).  0 for sizes or dtype codes the operator does not take. */
size_t dhdg_swin_ffn_wide_scratch_bytes(int c, int hidden, int mm_dtype);

/* x [dev] dense (rows, c) in x_dtype; gamma, beta [dev] float32 (c), or both NULL for no LayerNorm; w1 [dev] float32 (hidden, c),
 * b1 [dev] float32 (hidden), w2 [dev] float32 (c, hidden), b2 [dev] float32 (c): nn.Linear's layouts; out [dev] dense (rows, c)
 * in x_dtype, every element written, overlapping no input; scratch [dev] of at least dhdg_swin_ffn_wide_scratch_bytes(c, hidden,
 * mm_dtype) bytes, contents undefined before and after (the weights are laid out into it on every call: nothing is cached
 * across calls).  The inputs are only read; nothing is read beyond x's last row.  Every pointer 16-byte aligned.
 * 1 <= rows <= 2^36.
 * Checked on the host before the first launch, in this order: a NULL or misaligned pointer (gamma and beta: one of them NULL),
 * or rows <= 0 -> DHD_EINVAL; c, hidden, a dtype code or a combination outside the supported set, or rows > 2^36 ->
 * DHD_EUNSUPPORTED; scratch_bytes too small -> DHD_ENOSPACE.
 * Two launches on `stream` (the weight streams, the operator); nothing allocated, kept or synchronised. */
int dhdg_swin_ffn_wide_infer(const void* x, const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2,
                             const float* b2, void* out, void* scratch, size_t scratch_bytes, int x_dtype, int mm_dtype, long rows,
                             int c, int hidden, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHD_AMD_FFN_WIDE_H */
