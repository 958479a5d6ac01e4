/*
 * dhd_amd_occ_head_loss.h -- the occupancy head and its three losses in training as one operator of libdhd_amd.so: entry points
 * of the same library, under the conventions of dhd_amd.h (caller-owned [dev] memory, `stream` a hipStream_t as void*, 0 /
 * positive hipError_t / negative DHD_E* return codes, the DHD_F32 / DHD_F16 / DHD_BF16 dtype codes, dhd_occ_head_weights of
 * section 14).
 *
 * Why a header, a prefix and a directory of its own: the reason dhd_amd_occ_train.h gives.  Every other surface of the library is
 * a closed list held by a table that lives in a test file, and the listings of include/, dhd_amd/include/, dhd_amd/capi/ and
 * dhd_amd/capi_deform/ are such lists too, so the family ships beside them as dhdl_*, with its own copies of the guarantees
 * (tests/test_occ_head_loss_capi.py, tests/test_gpu_occ_head_loss.py).  Compile with include/ on the include path.  Nothing
 * here alters another header: DHD_ABI_VERSION is unchanged by this header.
 */
#ifndef DHD_AMD_OCC_HEAD_LOSS_H
#define DHD_AMD_OCC_HEAD_LOSS_H

#include "dhd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------ *
 * L1. Occupancy head + losses: the predicter MLP of section 14 and the three losses of dhd_occ_loss_forward on its logits,
 *
 *       logits[cell] = W2 . softplus(W1 . x[cell] + b1) + b2            c = 256, hidden = 512, dz * n_classes = 16 * 18
 *       losses[0..2] = class-balanced camera-masked cross entropy, sem scal, geo scal of the (b * dx * dy * 16, 18) logits
 *
 *     The forward is dhd_occ_head_infer's kernel writing the same float32 logits, byte for byte; while a lane still holds its 8
 *     voxels in registers it adds their terms of the 56 sums every loss is a function of (T_i, P_i, N_i, CE, n_valid over the
 *     valid voxels: mask != 0 and label != ignore_index).  A voxel that is not valid takes no part by a select: its logits may
 *     be NaN.  One row of 56 float32 per workgroup, then one launch that adds the rows in double and evaluates the losses with
 *     dhd_occ_loss_forward's formulas and edges (no valid voxel: NaN, NaN, 3 x -log(1e-5)).  The logits are not read again.
 *
 *     The backward is dhdo_occ_head_backward with g = dL/dlogits computed in the kernel instead of read: from the saved logits,
 *     the labels, the mask, the totals of the forward and the three upstream gradients,
 *       g_k = p_k (a_k + b_k [t = k] - sum_j p_j a_j - p_t b_t) + ce_scale w_t (p_k - [t = k])        exact 0 off the valid voxels
 *     with a_i = dL/dP_i, b_i = dL/dN_i and ce_scale from the totals in double, as dhd_occ_loss_backward has them.  dx, db1, db2,
 *     act and dhid are as in dhd_amd_occ_train.h.  g itself: a half x_dtype keeps it in registers and writes it, rounded once,
 *     only on request (dW2 = g^T . act); with DHD_F32 it is written once as float32 -- dW2's operand -- and read back per hidden
 *     tile by the lane that wrote it.  No atomics: two calls on the same bytes give the same bytes in every output.
 * ------------------------------------------------------------------------------------ */

/* 1 / 0: the set of dhd_occ_head_infer_supported with the default GEMM mode. */
int dhdl_occ_head_loss_supported(int c, int hidden, int dz, int n_classes, int x_dtype, int layout);

/* Bytes of the workspace the forward fills and the backward reads: the 56 totals in double. */
size_t dhdl_occ_head_loss_workspace_bytes(void);

/* Bytes of caller-provided scratch of a forward and of a backward call on (b, 256, dy, dx): the weight stream of each, and one
 * row of partial sums per workgroup of 128 cells of a sample (56 float32 forward, 800 backward).  Both are 0 whenever the return
 * code is not 0: a NULL pointer, a non-positive size or a bad dtype code -> DHD_EINVAL; a head, a dtype, a gemm mode or a size
 * outside the supported set -> DHD_EUNSUPPORTED.  Only w's integer members are looked at. */
int dhdl_occ_head_loss_scratch_bytes(const dhd_occ_head_weights* w, int x_dtype, int b, int dy, int dx, size_t* forward_bytes,
                                     size_t* backward_bytes);

/* x [dev] (b, 256, dy, dx) in x_dtype, dense NCHW (layout 0) or channels_last (layout 1); w: the parameters as in section 14;
 * labels, mask [dev] uint8 (b, dx, dy, 16), 8-byte aligned; class_weight [dev] float32 (18); logits [dev] float32
 * (b, dx, dy, 16, 18), every element written; losses [dev] float32 (3); workspace [dev] of dhdl_occ_head_loss_workspace_bytes()
 * bytes, to be handed to the backward unchanged; scratch [dev] of at least the forward bytes, contents undefined before and after.
 * x, the parameters, logits, workspace and scratch 16-byte aligned.
 * Checked on the host before the first launch: a NULL or misaligned pointer, a non-positive size, a bad dtype code ->
 * DHD_EINVAL; a head, layout or gemm mode outside the supported set, ignore_index outside [0, 255], non_empty_idx outside
 * [0, 18), dy * dx > 2^20 or b > 65535 -> DHD_EUNSUPPORTED; scratch_bytes too small -> DHD_ENOSPACE.
 * Three launches on `stream` (the weight stream, the operator, the totals); nothing allocated, kept or synchronised. */
int dhdl_occ_head_loss_forward(const void* x, int x_dtype, int layout, const dhd_occ_head_weights* w, int b, int dy, int dx,
                               const uint8_t* labels, const uint8_t* mask, const float* class_weight, int ignore_index,
                               int non_empty_idx, float* logits, float* losses, void* workspace, void* scratch, size_t scratch_bytes,
                               void* stream);

/* The inputs of the forward (b2 may be NULL), its logits and its workspace; grad_losses [dev] float32 (3): dL/dlosses[0..2], read
 * on the device (a loss scale arrives through it, and the call can be captured into a graph); dx_out [dev] of x's shape, dtype
 * and layout; db1 [dev] float32 (512), db2 [dev] float32 (288); act, dhid [dev] (b * dy * dx, 512) in x_dtype, both given or both
 * NULL; g [dev] (b * dy * dx, 288) in x_dtype: required with DHD_F32 (the kernel's own operand; scratch to the caller when the
 * weights are frozen), optional with a half type and then only beside act.  Every element of every output given is written.
 * Checked on the host before the first launch as in the forward, and: one of act / dhid without the other, g missing with
 * DHD_F32, g without act with a half type -> DHD_EINVAL.
 * Three launches on `stream` (the weight stream, the operator, the bias sums); nothing allocated, kept or synchronised. */
int dhdl_occ_head_loss_backward(const void* x, int x_dtype, int layout, const dhd_occ_head_weights* w, int b, int dy, int dx,
                                const float* logits, const uint8_t* labels, const uint8_t* mask, const float* class_weight,
                                int ignore_index, int non_empty_idx, const float* grad_losses, const void* workspace, void* dx_out,
                                float* db1, float* db2, void* act, void* dhid, void* g, void* scratch, size_t scratch_bytes,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHD_AMD_OCC_HEAD_LOSS_H */
