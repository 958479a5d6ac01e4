// The sampling position of one deformable-convolution tap and its four bilinear corners, in the float32 arithmetic every
// kernel of deform.hip and deform_conv.hip shares: position = integer base + offset, the `inside` test of mmcv's
// deformable_im2col, corners outside the image contribute 0.  One definition, so that the columns deform_im2col writes and
// the columns deform_conv.hip multiplies without writing them are the same numbers by construction.
#pragma once
#include <hip/hip_runtime.h>

namespace dhd_deform {

struct Tap {
  int i00, i01, i10, i11;   // flat indices into the H*W plane (valid ones only are used)
  float w00, w01, w10, w11; // bilinear weights, 0 for corners outside the image
  float ly, lx;             // fractional parts
  bool v00, v01, v10, v11, inside;
};

__device__ __forceinline__ Tap make_tap(float py, float px, int h, int w) {
  Tap t;
  t.inside = py > -1.0f && px > -1.0f && py < (float)h && px < (float)w;
  const float fy = floorf(py), fx = floorf(px);
  const int y0 = (int)fy, x0 = (int)fx, y1 = y0 + 1, x1 = x0 + 1;
  t.ly = py - fy;
  t.lx = px - fx;
  const float hy = 1.0f - t.ly, hx = 1.0f - t.lx;
  t.v00 = t.inside && y0 >= 0 && x0 >= 0;
  t.v01 = t.inside && y0 >= 0 && x1 <= w - 1;
  t.v10 = t.inside && y1 <= h - 1 && x0 >= 0;
  t.v11 = t.inside && y1 <= h - 1 && x1 <= w - 1;
  t.i00 = y0 * w + x0; t.i01 = y0 * w + x1; t.i10 = y1 * w + x0; t.i11 = y1 * w + x1;
  t.w00 = t.v00 ? hy * hx : 0.f;
  t.w01 = t.v01 ? hy * t.lx : 0.f;
  t.w10 = t.v10 ? t.ly * hx : 0.f;
  t.w11 = t.v11 ? t.ly * t.lx : 0.f;
  return t;
}

__device__ __forceinline__ Tap tap_of(const float* __restrict__ off_b, int t, int p, int h, int w, int k, int pad, int dil) {
  const int hw = h * w;
  const int y = p / w, x = p % w, ky = t / k, kx = t % k;
  const float py = (float)(y + ky * dil - pad) + off_b[(size_t)(2 * t) * hw + p];
  const float px = (float)(x + kx * dil - pad) + off_b[(size_t)(2 * t + 1) * hw + p];
  return make_tap(py, px, h, w);
}

}  // namespace dhd_deform
