/*
 * dhd_amd_seam.h -- the stage seams of the Swin backbone: entry points of libdhd_amd.so under the conventions of dhd_amd.h
 * (caller-owned [dev] memory, `stream` a hipStream_t as void*, 0 / positive hipError_t / negative DHD_E* return codes, dense
 * tensors, the DHD_F32 / DHD_F16 / DHD_BF16 dtype codes), outside the numbered dhd_* surface.
 *
 * Why a header and a prefix of its own: for the reason dhd_amd_ext.h gives.  The tables of the existing surfaces are closed
 * lists held by test files, each with the exact set of names of its prefix; a family added beside them ships under a new prefix
 * with its own copies of the guarantees (tests/test_swin_seam_capi.py, tests/test_gpu_swin_seam.py).  Nothing here alters
 * dhd_amd.h: DHD_ABI_VERSION is unchanged by this header.
 */
#ifndef DHD_AMD_SEAM_H
#define DHD_AMD_SEAM_H

#include "dhd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------ *
 * S1. Patch merging up to its Linear layer: the 2 x 2 neighbourhood gather (stride 2) with the LayerNorm over the gathered
 *     4c values in it.  x is the token map (b, h, w, c); output row r = (bi, i, j), i < ho = ceil(h / 2), j < wo = ceil(w / 2),
 *     has 4c channels, channel k = 4 cc + 2 kh + kw holding x[bi, 2i + kh, 2j + kw, cc] -- nn.Unfold's (c, kh, kw) order, so
 *     the weight of the Linear that follows is used as it stands.  A source past h or w is an exact zero, and that zero ENTERS
 *     the row's statistics: the reference pads before this norm (unlike the window form of dhd_amd_ext.h, which pads after).
 *
 *     Supported (dhds_merge_norm_supported: 1 / 0): c a multiple of 8, 8 <= c <= 512 (4c <= 2048); float32, float16 or
 *     bfloat16 on either side, in any combination.  Calls additionally need fewer than 2^40 tokens.
 *     Arithmetic: float32 throughout, as section X1 of dhd_amd_ext.h states it.  mean = sum / 4c; var = the centred sum of
 *     squares over registers / 4c; rstd = 1 / sqrtf(var + eps); every sum is a fixed tree over a lane group.  Within the
 *     layer's 1e-4 bar of a float64 LayerNorm, not bit-identical to torch's.  A half result is the float32 result rounded
 *     once, to nearest even.  A lane loads 16 bytes from each of a row's four sources and stores the contiguous run of output
 *     channels they interleave to: 16-byte accesses on both sides.  No LDS, no atomics.
 * ------------------------------------------------------------------------------------ */
int dhds_merge_norm_supported(int c, int x_dtype, int out_dtype);

/* out row r = (gather(x)[r] - mean) * rstd * gamma + beta, in out_dtype.  x [dev] dense (b, h, w, c) in x_dtype; gamma, beta
 * [dev] float32 (4c); out [dev] dense (b, ho wo, 4c) in out_dtype, every element written.  x, out, gamma and beta 16-byte
 * aligned.  Checked on the host before the launch: a NULL or misaligned pointer or a non-positive b / h / w -> DHD_EINVAL; c
 * or a dtype code outside the supported range -> DHD_EUNSUPPORTED.
 * One launch on `stream`; nothing allocated, kept or synchronised.  Reproducible: the same bytes on every call. */
int dhds_merge_norm_forward(const void* x, const float* gamma, const float* beta, void* out, int x_dtype, int out_dtype, int b, int h,
                            int w, int c, float eps, void* stream);

/* Bytes of caller-provided scratch for a backward over `out_rows` = b ho wo output rows of 4c channels: one pair of float32
 * rows (sum of dy x^, sum of dy; 32 c bytes) per workgroup of the row kernel.  Non-decreasing in out_rows; 0 for sizes the
 * operator does not take. */
size_t dhds_merge_norm_backward_scratch_bytes(long out_rows, int c);

/* Backward of dhds_merge_norm_forward from x, dy and gamma alone; the row statistics are recomputed from x.  With x^ the
 * normalised gathered row and g = dy gamma, per output row
 *   d(gathered) = rstd (g - mean(g) - x^ mean(g x^)),      dgamma = sum over rows of dy x^,      dbeta = sum over rows of dy,
 * the means over all 4c values, zeros of the padding included.  Every real token is a source of exactly one output row, so
 * dx is written once per element with plain stores; pad sources have no element of dx and are skipped.
 * x, b .. eps as in the forward; dy [dev] dense (b, ho wo, 4c) in dy_dtype; dx [dev] dense, x's shape and dtype, every element
 * written; dgamma, dbeta [dev] float32 (4c), every element written (not accumulated into); scratch [dev] of at least
 * dhds_merge_norm_backward_scratch_bytes(b ho wo, c) bytes, contents undefined before and after.  The inputs are only read.
 * x, dy, dx, gamma, dgamma, dbeta and scratch 16-byte aligned.
 * Reproducibility: no atomics.  Every workgroup adds its contiguous run of rows into its own partial row pair in a fixed
 * order, and a second launch adds the partial rows in a fixed order: dx, dgamma and dbeta are the same bytes on every call.
 * Checked on the host before the first launch: a NULL or misaligned pointer or a non-positive b / h / w -> DHD_EINVAL; c or a
 * dtype code outside the supported range -> DHD_EUNSUPPORTED; scratch_bytes too small -> DHD_ENOSPACE.
 * Two launches on `stream`; nothing allocated, kept or synchronised. */
int dhds_merge_norm_backward(const void* x, const void* dy, const float* gamma, void* dx, float* dgamma, float* dbeta, void* scratch,
                             size_t scratch_bytes, int x_dtype, int dy_dtype, int b, int h, int w, int c, float eps, void* stream);

/* ------------------------------------------------------------------------------------ *
 * S2. Patch embedding after its convolution: LayerNorm over the channels of an NCHW map, written as the token map.  x is the
 *     convolution's output as it lies, dense (b, c, hw); out is (b, hw, c).  The transposition happens inside the kernel: a
 *     tile of 64 (c <= 128) or 32 pixels of one image is staged in LDS in float32 and the rows are normalised from there; no
 *     intermediate tensor is written to memory.  Tiles never straddle an image; the last tile of an image is partial.
 *     Channel planes are read (and, in the backward, written) as 16-byte vectors where hw is a multiple of the elements in
 *     16 bytes of x_dtype, element by element otherwise; the token side always moves as 16-byte vectors.
 *
 *     Supported (dhds_embed_norm_supported: 1 / 0): c a multiple of 8, 8 <= c <= 256; float32, float16 or bfloat16 on either
 *     side, in any combination.  Calls additionally need fewer than 2^40 tokens.  Arithmetic as in S1, over c values.
 * ------------------------------------------------------------------------------------ */
int dhds_embed_norm_supported(int c, int x_dtype, int out_dtype);

/* out[bi, p, :] = (x[bi, :, p] - mean) * rstd * gamma + beta, in out_dtype.  x [dev] dense (b, c, hw) in x_dtype; gamma, beta
 * [dev] float32 (c); out [dev] dense (b, hw, c) in out_dtype, every element written.  x, out, gamma and beta 16-byte aligned.
 * Checked on the host before the launch: a NULL or misaligned pointer or a non-positive b / hw -> DHD_EINVAL; c or a dtype
 * code outside the supported range -> DHD_EUNSUPPORTED.
 * One launch on `stream`; nothing allocated, kept or synchronised.  Reproducible: the same bytes on every call. */
int dhds_embed_norm_forward(const void* x, const float* gamma, const float* beta, void* out, int x_dtype, int out_dtype, int b, int c,
                            long hw, float eps, void* stream);

/* Bytes of caller-provided scratch for a backward over `tokens` = b hw tokens of c channels: one pair of float32 rows (8 c
 * bytes) per workgroup.  Non-decreasing in tokens; 0 for sizes the operator does not take. */
size_t dhds_embed_norm_backward_scratch_bytes(long tokens, int c);

/* Backward of dhds_embed_norm_forward from x, dy and gamma alone, the statistics recomputed: the formulas of S1 over c values.
 * x, b .. eps as in the forward; dy [dev] dense (b, hw, c) in dy_dtype; dx [dev] dense (b, c, hw), x's layout and dtype, every
 * element written (through the LDS tile, as x was read); dgamma, dbeta [dev] float32 (c), every element written; scratch [dev]
 * of at least dhds_embed_norm_backward_scratch_bytes(b hw, c) bytes, contents undefined before and after.  The inputs are only
 * read.  x, dy, dx, gamma, dgamma, dbeta and scratch 16-byte aligned.
 * Reproducibility: no atomics.  Every workgroup adds its contiguous run of tiles into its own partial row pair in a fixed
 * order, and a second launch adds the partial rows in a fixed order: dx, dgamma and dbeta are the same bytes on every call.
 * Checked on the host before the first launch: a NULL or misaligned pointer or a non-positive b / hw -> DHD_EINVAL; c or a
 * dtype code outside the supported range -> DHD_EUNSUPPORTED; scratch_bytes too small -> DHD_ENOSPACE.
 * Two launches on `stream`; nothing allocated, kept or synchronised. */
int dhds_embed_norm_backward(const void* x, const void* dy, const float* gamma, void* dx, float* dgamma, float* dbeta, void* scratch,
                             size_t scratch_bytes, int x_dtype, int dy_dtype, int b, int c, long hw, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHD_AMD_SEAM_H */
