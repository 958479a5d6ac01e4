/*
 * dhd_amd_occ_train.h -- the occupancy head's training surface of libdhd_amd.so: entry points of the same library, under the
 * conventions of dhd_amd.h (caller-owned [dev] memory, `stream` a hipStream_t as void*, 0 / positive hipError_t / negative
 * DHD_E* return codes, the DHD_F32 / DHD_F16 / DHD_BF16 dtype codes, dhd_occ_head_weights of section 14).
 *
 * Why a header, a prefix and a directory of its own: every other surface of the library is a closed list held by a table that
 * lives in a test file, and the listings of include/ and of dhd_amd/include/ are such lists too.  A change that may not edit
 * them ships its family beside them as dhdo_*, with its own copies of the guarantees (tests/test_occ_head_train_capi.py,
 * tests/test_gpu_occ_head_train.py).  Compile with include/ on the include path.  Nothing here alters another header:
 * DHD_ABI_VERSION is unchanged by this header.
 */
#ifndef DHD_AMD_OCC_TRAIN_H
#define DHD_AMD_OCC_TRAIN_H

#include "dhd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------ *
 * O1. Occupancy head in training: the predicter MLP of section 14, per BEV cell,
 *
 *       logits[cell] = W2 . softplus(W1 . x[cell] + b1) + b2            c = 256, hidden = 512, dz * n_classes = 16 * 18
 *
 *     The forward in training is dhd_occ_head_infer with pred == NULL and logits set: the same launches, the same bytes, and
 *     nothing of hidden size is kept.  The backward takes x, the parameters and g = dL/dlogits and recomputes, per hidden tile in
 *     registers: h = W1 . x + b1 again, da = W2^T . g, a = softplus(h), dh = da s(h) with s the logistic function from
 *     softplus's own exp(-|h|) (1 above torch's threshold of 20, 1 / 0 at +-inf, a NaN goes through), dx += W1^T . dh.
 *
 *       dx  = W1^T . dh           in x_dtype and in x's layout, rounded once
 *       db1 = sum over cells of dh,   db2 = sum over cells of g           float32, of the unrounded values
 *
 *     The weight gradients are reductions over cells and are not computed here; on request the backward writes their operands,
 *     dense, in the GEMM type, each rounded once to it:
 *       act  (cells, hidden) = a    in the LOGITS' cell order (b, ix, iy), so that dW2 = g^T . act
 *       dhid (cells, hidden) = dh   in x's PIXEL order (b, iy, ix), so that dW1 = dhid^T . x  (channels_last: one product on a
 *                                   view of x; NCHW: a product per sample, summed)
 *       ghalf (cells, 288)   = g    rounded to a half GEMM type, in g's own order; with float32 GEMMs g itself is the operand
 *     With act and dhid NULL none is written (a frozen head: only dx, db1, db2).
 *
 *     The GEMM type follows x as in section 14: float32 x -> three bf16 MFMA products of two-part splits, smallest terms first;
 *     half x -> one product in its own type.  float32 accumulation; biases, Softplus and its derivative are float32.
 *     Cells are independent in dx, act, dhid and ghalf: a NaN or infinity in a cell of x or g stays in that cell (db1 and db2
 *     are sums over all cells).  No atomics: two calls on the same bytes give the same bytes in every output.
 * ------------------------------------------------------------------------------------ */

/* 1 / 0: the set of dhd_occ_head_infer_supported with the default GEMM mode. */
int dhdo_occ_head_backward_supported(int c, int hidden, int dz, int n_classes, int x_dtype, int layout);

/* Bytes of caller-provided scratch of a backward call on (b, 256, dy, dx): the backward's weight stream (b1 and three blocks of
 * MFMA fragments per hidden tile, plus what the read-ahead touches past its end) and one row of 800 float32 partial sums per
 * workgroup of 128 cells of a sample.  *bytes is 0 whenever the return code is not 0: w or bytes NULL, a non-positive size or a
 * bad dtype code -> DHD_EINVAL; a head, a dtype or a size outside the supported set -> DHD_EUNSUPPORTED.  Only w's integer
 * members are looked at. */
int dhdo_occ_head_backward_scratch_bytes(const dhd_occ_head_weights* w, int x_dtype, int b, int dy, int dx, size_t* bytes);

/* x [dev] (b, 256, dy, dx) in x_dtype, dense NCHW (layout 0) or channels_last (layout 1); w: the parameters as in section 14
 * (b2 has no part in the backward and may be NULL); glogits [dev] float32 (b, dx, dy, 16, 18), dense: the reference's
 * permute(0, 3, 2, 1) cell order, what dhd_occ_loss_backward writes; dx_out [dev] of x's shape, dtype and layout; db1 [dev]
 * float32 (512), db2 [dev] float32 (288); act, dhid [dev] (b * dy * dx, 512) in x_dtype, both given or both NULL; ghalf [dev]
 * (b * dy * dx, 288) in x_dtype or NULL, and NULL when x_dtype is DHD_F32 or act is NULL.  Every element of every output given
 * is written, and no output overlaps an input or another output; scratch [dev] of at least
 * dhdo_occ_head_backward_scratch_bytes(...) bytes, contents undefined before and after.  Every pointer 16-byte aligned.
 * Checked on the host before the first launch: a NULL (but b2 and the operands) or misaligned pointer, a non-positive size, a
 * bad dtype code, one of act / dhid without the other, ghalf with float32 or without act -> DHD_EINVAL; a head, layout or gemm
 * mode outside the supported set, one sample of more than 2^30 bytes as float32 (dy * dx > 2^20) or b > 65535 ->
 * DHD_EUNSUPPORTED; scratch_bytes too small -> DHD_ENOSPACE.
 * Three launches on `stream` (the weight stream, the operator, the bias sums); nothing allocated, kept or synchronised. */
int dhdo_occ_head_backward(const void* x, int x_dtype, int layout, const dhd_occ_head_weights* w, int b, int dy, int dx,
                           const float* glogits, void* dx_out, float* db1, float* db2, void* act, void* dhid, void* ghalf,
                           void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHD_AMD_OCC_TRAIN_H */
