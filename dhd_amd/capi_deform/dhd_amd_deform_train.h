/*
 * dhd_amd_deform_train.h -- the deformable convolution's training surface of libdhd_amd.so: entry points of the same library,
 * under the conventions of dhd_amd.h (caller-owned [dev] memory, `stream` a hipStream_t as void*, 0 / positive hipError_t /
 * negative DHD_E* return codes, the DHD_F32 / DHD_F16 / DHD_BF16 dtype codes, section 15's operator).
 *
 * Why a header, a prefix and a directory of its own: the reason dhd_amd_occ_train.h gives.  Every other surface of the library is
 * a closed list held by a table that lives in a test file, and the listings of include/, dhd_amd/include/ and dhd_amd/capi/ are
 * such lists too.  A change that may not edit them ships its family beside them as dhdd_*, with its own copies of the guarantees
 * (tests/test_deform_conv_train_capi.py, tests/test_gpu_deform_conv_train.py).  Compile with include/ on the include path.
 * Nothing here alters another header: DHD_ABI_VERSION is unchanged by this header.
 */
#ifndef DHD_AMD_DEFORM_TRAIN_H
#define DHD_AMD_DEFORM_TRAIN_H

#include "dhd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------ *
 * D1. Deformable convolution (DCN v1, 3 x 3, stride 1, one deformable group) in training.
 *
 *       col[c, t, p] = bilinear(x[c], position of tap t of pixel p),      out[o, p] = sum_{c in group, t} W[o, c, t] col[c, t, p]
 *
 *     The forward in training is dhd_deform_conv_infer: the same launches, the same bytes, nothing of column size is kept.  The
 *     backward takes x, the offsets, W and g = dL/dout and computes, without the column gradient dcol = W^T g ever being in memory:
 *
 *       dx[c, cell]     = sum_{t, o} W[o, c, t] G_t[o, cell],   G_t[o, cell] = sum over the corner entries (p, w) of tap t that touch
 *                         the cell of w g[o, p], entries in ascending p                      in x_dtype and x's layout, rounded once
 *       doffset[2t, p], doffset[2t+1, p] = sum over all channels of dcol[c, t, p] d bilinear / d(row, column), the expression and
 *                         the `inside` rule of the column path's offset kernel; dcol enters rounded once to x_dtype, as the column
 *                         path's GEMM writes it (float32: as accumulated)                                            float32
 *
 *     The weight gradient is a reduction over pixels and is not computed here; on request the backward writes its operand:
 *       col (b, c_in * 9, h * w), rows c * 9 + t, in x_dtype: the bytes dhd_deform_im2col_t writes from the same x, so that
 *       dW[o, (c, t)] = sum over images and pixels of g[o, p] col[(c, t), p]
 *
 *     float32 x: three bf16 MFMA products of two-part splits, smallest terms first; half x: one product in its own type.  float32
 *     accumulation; positions, bilinear weights and their derivatives are float32.  A NaN or infinity in a pixel of g stays in the
 *     cells its taps touch (dx) and in that pixel's entries (doffset).  No atomics on results: two calls on the same bytes give
 *     the same bytes in every output.
 * ------------------------------------------------------------------------------------ */

/* 1 / 0: the set of dhd_deform_conv_infer_supported with the default GEMM mode (k = 3, C/g and O/g multiples of 8 up to 128, ...),
 * h * w <= 853 (the (cell, tap) sort of one image works in 64 KiB of LDS), x_layout and g_layout 0 (dense NCHW) or 1 (channels_last). */
int dhdd_deform_conv_backward_supported(int c_in, int c_out, int groups, int k, int h, int w, int x_dtype, int x_layout, int g_layout);

/* Bytes of caller-provided scratch of a backward call: the two weight streams, the segment bounds and two copies of the entry
 * lists (b * 36 * h * w entries of 8 bytes each), with more than one group the groups' partial offset gradients, and the
 * channels_last copy of an NCHW x and of an NCHW g.  *bytes is 0 whenever the return code is not 0: bytes NULL, a non-positive
 * size, channel counts the groups do not divide, a bad dtype or layout code -> DHD_EINVAL; a shape outside the supported set or
 * b > 65535 -> DHD_EUNSUPPORTED. */
int dhdd_deform_conv_backward_scratch_bytes(int b, int c_in, int c_out, int groups, int k, int h, int w, int x_dtype, int x_layout,
                                            int g_layout, size_t* bytes);

/* x [dev] (b, c_in, h, w) in x_dtype, dense NCHW (x_layout 0) or channels_last (1); offset [dev] float32 (b, 18, h, w), weight
 * [dev] float32 (c_out, c_in / groups, 3, 3), as in section 15; gout [dev] (b, c_out, h, w) in x_dtype, dense NCHW (g_layout 0) or
 * channels_last (1); dx [dev] of x's shape, dtype and layout; doffset [dev] float32 of offset's shape; col [dev] (b, c_in * 9,
 * h * w) in x_dtype, or NULL: then it is not written.  Every element of every output given is written once, and no output
 * overlaps an input or another output; scratch [dev] of at least dhdd_deform_conv_backward_scratch_bytes(...) bytes, contents
 * undefined before and after.  x, gout, dx, col and scratch 16-byte aligned; offset, weight and doffset 4-byte aligned.
 * Checked on the host before the first launch, in this order: a NULL pointer (but col), a non-positive size, pad < 0, dil < 1, a
 * bad dtype or layout code, channel counts the groups do not divide -> DHD_EINVAL; a shape outside the supported set or
 * b > 65535 -> DHD_EUNSUPPORTED; scratch_bytes too small -> DHD_ENOSPACE; a misaligned pointer -> DHD_EINVAL.
 * Launches on `stream`: the two weight streams, the sort, a transpose per NCHW input, the two operators, with more than one group
 * the sum of the partial offset gradients; nothing allocated, kept or synchronised. */
int dhdd_deform_conv_backward(const void* x, int x_dtype, int x_layout, const float* offset, const float* weight, const void* gout,
                              int g_layout, void* dx, float* doffset, void* col, int b, int c_in, int c_out, int groups, int h, int w, int k,
                              int pad, int dil, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHD_AMD_DEFORM_TRAIN_H */
