/*
 * dhd_amd_unet_seam.h -- what a UNet does between its 3 x 3 convolutions, as operators of libdhd_amd.so: the 2 x 2 max pooling
 * of `_Down` without an index tensor, and the transposed 2 x 2 convolution, padding and concatenation of `_Up` in one launch.
 * Entry points of the same library, under the conventions of dhd_amd.h (caller-owned [dev] memory, `stream` a hipStream_t as
 * void*, 0 / positive hipError_t / negative DHD_E* return codes, the DHD_F32 / DHD_F16 / DHD_BF16 dtype codes).
 *
 * Why a header, a prefix and a directory of its own: the reason dhd_amd_occ_train.h gives.  Every other surface of the library is
 * a closed list held by a table that lives in a test file, and so are the listings of the directories that hold the other
 * headers, so the family ships beside them as dhdn_*, with its own copies of the guarantees (tests/test_unet_seam_capi.py,
 * tests/test_gpu_unet_seam.py).  Compile with include/ on the include path.  Nothing here alters another header:
 * DHD_ABI_VERSION is unchanged by this header.
 */
#ifndef DHD_AMD_UNET_SEAM_H
#define DHD_AMD_UNET_SEAM_H

#include "dhd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* layout codes of a (b, c, h, w) map */
#define DHDN_NCHW 0
#define DHDN_NHWC 1 /* torch.channels_last: [b][h][w][c] in memory */

/* ------------------------------------------------------------------------------------ *
 * N1. MaxPool2d(2): y (b, c, h / 2, w / 2) of x (b, c, h, w), in x's dtype and layout.  A last odd row / column is dropped.
 *
 *     THE RULE (both kernels): scan the window in the order (0,0), (0,1), (1,0), (1,1), starting from the first element with
 *     max = -inf; an element v replaces the running maximum when  v > max || isnan(v).  So ties keep the first element, an
 *     all -inf window keeps (0,0), and the last NaN of a window wins.  It is torch's rule: values and gradient routing are those
 *     of F.max_pool2d bit for bit -- on the CPU in both layouts and on the device, with one exception measured on the MI355X:
 *     torch's channels_last device kernels hand the gradient of an all -inf window to no element at all.
 *
 *     forward   one launch; y is the winner's bits.  Nothing but x is needed later: no index tensor exists.
 *     backward  one launch; recomputes the winner from x and writes EVERY element of gx exactly once: gy at the winner (as
 *               0 + gy, torch's accumulation: a negative zero becomes +0), zero elsewhere, zero in a dropped row / column.
 *               No zero-fill pass and no atomics, so two calls on the same bytes give the same bytes.
 *
 *     DHDN_NHWC moves 16-byte channel vectors: c a multiple of 16 / sizeof(element), i.e. 8 for the half types (and 8 is what
 *     the entry points ask of float32 too), pointers 16-byte aligned.  DHDN_NCHW accesses single elements: any c, pointers
 *     aligned to the element.  h, w >= 2; fewer than 2^40 elements.
 * ------------------------------------------------------------------------------------ */

/* 1 where the two entry points below take the arguments, else 0. */
int dhdn_max_pool2_supported(int dtype, int layout, int b, int c, int h, int w);

/* NULL or misaligned pointer, b, c, h or w < 1 -> DHD_EINVAL (the pointer test comes first); otherwise not supported ->
 * DHD_EUNSUPPORTED.  One launch on `stream`; nothing allocated, kept or synchronised. */
int dhdn_max_pool2_forward(const void* x, void* y, int dtype, int layout, int b, int c, int h, int w, void* stream);
int dhdn_max_pool2_backward(const void* x, const void* grad_y, void* grad_x, int dtype, int layout, int b, int c, int h, int w,
                            void* stream);

/* ------------------------------------------------------------------------------------ *
 * N2. The up seam: out = cat([x2, pad(conv_transpose2d(x1, weight, bias, stride = 2))], 1).
 *
 *       x1      (b, cin, h, w)          DHDN_NHWC, `dtype`
 *       x2      (b, c2, H, W)           DHDN_NHWC, `dtype`;  H >= 2 h, W >= 2 w
 *       weight  (cin, cout, 2, 2)       dense, of `wdtype` (any of the three codes); packed into MFMA operand order by a launch
 *                                       of its own in every call (into `scratch`)
 *       bias    float32 (cout) or NULL
 *       out     (b, c2 + cout, H, W)    DHDN_NHWC, `dtype`
 *
 *     pads: top = (H - 2 h) / 2, left = (W - 2 w) / 2, the rest after; the padded border of channels c2 .. c2 + cout is zero
 *     (no bias there).  Output pixel (2 y + dy + top, 2 x + dx + left), channel c2 + co, is
 *     bias[co] + sum_ci x1[y, x, ci] weight[ci, co, dy, dx]: a (pixels x cin) (cin x 4 cout) product on the MFMA
 *     (v_mfma_f32_16x16x32) with float32 accumulation, the bias added in float32, one rounding on the way out.  DHD_F32 tensors
 *     multiply as three bfloat16 products (high x high, high x mid, mid x high of the exact splits of sfa_mfma.h).  The epilogue
 *     writes into the concatenated tensor; the same launch copies x2 into channels 0 .. c2 and writes the border.  Neither the
 *     up-sampled nor the padded tensor exists.
 *
 *     backward: grad_out (b, c2 + cout, H, W) is read where it lies.
 *       grad_x1  (b, cin, h, w) = G W^T on the MFMA, G the (pixels x 4 cout) operand gathered from the four output pixels of
 *                each x1 pixel (column q cout + co, q = 2 dy + dx)
 *       grad_x2  (b, c2, H, W) dense, or NULL: not written
 *       g_operand  G itself, (b h w, 4 cout) row-major in `dtype`, the operand of the caller's weight-gradient GEMM
 *                (dweight[ci, co, dy, dx] = sum_p x1[p, ci] G[p, q cout + co]), or NULL: not written
 *       dbias    float32 (cout), or NULL: per-workgroup partial rows in `scratch`, added in index order by a second launch
 *     No atomics: two calls on the same bytes give the same bytes.
 *
 *     Supported: the three dtype codes, DHDN_NHWC only, cin a multiple of 32 in 32 .. 1024, cout a multiple of 16 in 16 .. 512,
 *     c2 a multiple of 8 (>= 8), every tensor below 2^31 bytes.  All tensor pointers 16-byte aligned.
 * ------------------------------------------------------------------------------------ */

/* x1 pixels per workgroup (the row tile) and columns of the product per workgroup (the column tile: of 4 cout in the forward,
 * of cin in the backward).  The grid is ceil(b h w / ROWS) x ceil(columns / COLS). */
#define DHDN_UP_ROWS 32
#define DHDN_UP_COLS 128

int dhdn_up_cat_supported(int dtype, int layout, int b, int cin, int cout, int c2, int h, int w, int H, int W);

/* Bytes of scratch of one call (a multiple of 16): the packed weight, and for backward != 0 the partial rows of dbias behind
 * it.  0 where the shape is not supported. */
size_t dhdn_up_cat_scratch_bytes(int dtype, int b, int cin, int cout, int h, int w, int backward);

/* NULL or misaligned x1, x2, weight, out or scratch, misaligned bias, a size < 1 -> DHD_EINVAL (pointers first); not supported
 * -> DHD_EUNSUPPORTED; scratch_bytes below dhdn_up_cat_scratch_bytes(..., 0) -> DHD_ENOSPACE.  Two launches on `stream`. */
int dhdn_up_cat_forward(const void* x1, const void* x2, const void* weight, int wdtype, const float* bias, void* out, void* scratch,
                        size_t scratch_bytes, int dtype, int layout, int b, int cin, int cout, int c2, int h, int w, int H, int W,
                        void* stream);

/* As above with grad_out, weight, grad_x1 and scratch required, grad_x2, g_operand and dbias optional, and scratch_bytes held
 * to dhdn_up_cat_scratch_bytes(..., 1).  Two launches, three with dbias. */
int dhdn_up_cat_backward(const void* grad_out, const void* weight, int wdtype, void* grad_x1, void* grad_x2, void* g_operand,
                         float* dbias, void* scratch, size_t scratch_bytes, int dtype, int layout, int b, int cin, int cout, int c2,
                         int h, int w, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHD_AMD_UNET_SEAM_H */
