/*
 * dhd_amd_stereo_cv.h -- the temporal-stereo cost volume of DepthNet computed from the camera matrices, as operators of
 * libdhd_amd.so: the sampling positions of `gen_grid` are evaluated inside the kernel, and the feature maps are read in their
 * own type (float32, float16 or bfloat16) where they lie.  Entry points of the same library, under the conventions of
 * dhd_amd.h (caller-owned [dev] memory, `stream` a hipStream_t as void*, 0 / positive hipError_t / negative DHD_E* return
 * codes, the DHD_F32 / DHD_F16 / DHD_BF16 dtype codes).
 *
 * Why a header, a prefix and a directory of its own: the reason dhd_amd_occ_train.h gives.  Every other surface of the library is
 * a closed list held by a table that lives in a test file, and so are the listings of the directories that hold the other
 * headers, so the family ships beside them as dhdv_*, with its own copies of the guarantees (tests/test_stereo_cv_capi.py,
 * tests/test_gpu_stereo_cv.py).  Compile with include/ on the include path.  Nothing here alters another header:
 * DHD_ABI_VERSION is unchanged by this header, and dhd_stereo_cost_volume (dhd_amd.h) is unchanged.
 */
#ifndef DHD_AMD_STEREO_CV_H
#define DHD_AMD_STEREO_CV_H

#include "dhd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* layout codes of the (bn, c, h, w) feature maps */
#define DHDV_NCHW 0 /* dense NCHW: re-laid once, in its own type, into `scratch` (dhd_transpose_batched) */
#define DHDV_NHWC 1 /* torch.channels_last: [bn][h][w][c] in memory, read where it lies */

/* limits of the fused kernels */
#define DHDV_MAX_C 1024
#define DHDV_MAX_D 256

/* ------------------------------------------------------------------------------------ *
 * THE POSITION.  For view n (of bn), frustum point (u, v, dep) = (u[x], v[y], dep[d]) and the adjacent image of hi x wi pixels,
 * in float32, every product, sum and quotient rounded (no fused multiply-add), `M p` meaning (0 + m0 p0 + m1 p1) + m2 p2 per
 * row, left to right:
 *
 *     p = (u, v, dep) - post_trans[n]
 *     (x, y, z) = inv_post_rot[n] p;   x = x z;  y = y z
 *     (x, y, z) = combine[n] (x, y, z) + trans[n]                 combine = rots inverse(intrins), trans: of k2s_sensor
 *     neg = z < 1e-3f
 *     (x, y, z) = intrins[n] (x, y, z);   x = x / z;  y = y / z
 *     (x, y) = post_rots[n][:2, :2] (x, y) + post_trans[n][:2]
 *     px = x * (1.0f / (wi - 1)) * 2 - 1,   py = y * (1.0f / (hi - 1)) * 2 - 1;   (px, py) = (-2, -2) where neg
 *
 * It is DepthNet.gen_grid as torch's device kernels evaluate it (a division by a Python scalar is a multiplication by its
 * float32 reciprocal there), bit for bit.  The six view arrays are float32, dense: inv_post_rot, combine, intrins, post_rots
 * (bn, 3, 3) row-major, post_trans and trans (bn, 3); the inverses and `combine` are the caller's.  u (w), v (h) and dep
 * (n_depth) are the axes of the separable frustum template, float32.
 * ------------------------------------------------------------------------------------ */

/* 1 where dhdv_stereo_cost_volume takes the sizes, else 0: c a multiple of 8 (of 4 for DHD_F32) up to DHDV_MAX_C, n_depth up
 * to DHDV_MAX_D, bn n_depth h w below 2^31. */
int dhdv_stereo_cv_supported(int dtype, int bn, int c, int h, int w, int n_depth);

/* Bytes of scratch of one dhdv_stereo_cost_volume call (a multiple of 16): both maps re-laid for DHDV_NCHW, 0 for DHDV_NHWC
 * and where the arguments are not supported. */
size_t dhdv_stereo_cv_scratch_bytes(int dtype, int layout, int bn, int c, int h, int w);

/* grid (bn, n_depth * h, w, 2) float32, 8-byte aligned: the positions above, (px, py) interleaved, as gen_grid returns them.
 * NULL or misaligned pointer, a size < 1, hi or wi < 2 -> DHD_EINVAL; n_depth > DHDV_MAX_D or bn n_depth h w >= 2^31 ->
 * DHD_EUNSUPPORTED.  One launch. */
int dhdv_stereo_grid(const float* inv_post_rot, const float* post_trans, const float* combine, const float* trans,
                     const float* intrins, const float* post_rots, const float* u, const float* v, const float* dep, float* grid,
                     int bn, int h, int w, int n_depth, int hi, int wi, void* stream);

/* out (bn, n_depth, h, w) dense, of `dtype` = softmax over n_depth of -cost,
 *     cost[n, d, y, x] = sum_c | curr[n, c, y, x] - bilinear(prev[n, c], position(n, x, y, d)) |   (+ bias where the sample of
 *                        channel `flag_channel` came back exactly 0; skipped for bias == 0)
 * with the position rounded once through `dtype` (what gen_grid(...).to(dtype) does), align_corners = True, zero padding.
 * prev, curr: (bn, c, h, w) of `dtype` in `layout`, 16-byte aligned.  Sampling, the channel sum, the bias rule and the softmax are
 * float32; the result is rounded once.  DHD_F32: the arithmetic, its order and so the bytes of dhd_stereo_cost_volume on
 * gen_grid's positions.  Half types: a lane holds 8 channels; up to 128 channels take 16 lanes per hypothesis (four hypotheses
 * per step), up to 256 take 32, more take the whole wave; the channel sum is a DPP reduction inside the lane group.  No atomics:
 * two calls on the same bytes give the same bytes.
 *
 * NULL or misaligned pointer (scratch may be NULL where no scratch is needed), a size < 1, hi or wi < 2 -> DHD_EINVAL (the
 * pointer test comes first); not supported, an unknown dtype or layout, flag_channel outside 0 .. c - 1 -> DHD_EUNSUPPORTED;
 * scratch_bytes below dhdv_stereo_cv_scratch_bytes -> DHD_ENOSPACE.  One launch, three for DHDV_NCHW. */
int dhdv_stereo_cost_volume(const void* prev, const void* curr, void* out, int dtype, int layout, const float* inv_post_rot,
                            const float* post_trans, const float* combine, const float* trans, const float* intrins,
                            const float* post_rots, const float* u, const float* v, const float* dep, int bn, int c, int h, int w,
                            int n_depth, int hi, int wi, float bias, int flag_channel, void* scratch, size_t scratch_bytes,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHD_AMD_STEREO_CV_H */
