// The index maps of the Swin shifted-window partition and its reverse (window.hip's header comment has the formulas), shared by
// window.hip (the row gathers) and swin_glue.hip (LayerNorm into the gather, reverse + residual add).
#pragma once
#include "vec16.h"

namespace dhd {

// eight consecutive elements <-> float registers, as 16-byte accesses
template <typename T> __device__ __forceinline__ void load8(const T* p, float (&v)[8]) {
  using V = Vec16<T, false>;
#pragma unroll
  for (int k = 0; k < 8; k += V::N) V::load(p + k, v + k);
}
template <typename T> __device__ __forceinline__ void store8(T* p, const float (&v)[8]) {
  using V = Vec16<T, false>;
#pragma unroll
  for (int k = 0; k < 8; k += V::N) V::store(p + k, v + k);
}

struct WinGeom {
  int b, h, w, c, ws, shift, hp, wp, nh, nw;
};

// the geometry of a (b, h, w, c) token map cut into windows of `window` (> 0) after a cyclic shift
static inline WinGeom win_geom(int b, int h, int w, int c, int window, int shift) {
  WinGeom g{b, h, w, c, window, shift, 0, 0, 0, 0};
  g.nh = (h + window - 1) / window;
  g.nw = (w + window - 1) / window;
  g.hp = g.nh * window;
  g.wp = g.nw * window;
  return g;
}

// partition: the token row that window row `row` of (b, nh*nw, ws*ws) holds, -1 where it lies in the padding
__device__ __forceinline__ long win_partition_src(const WinGeom& g, long row) {
  const int ws2 = g.ws * g.ws;
  const int i = (int)(row % ws2);
  const long win = row / ws2;
  const int wx = (int)(win % g.nw), wy = (int)((win / g.nw) % g.nh);
  const long bi = win / ((long)g.nw * g.nh);
  int y = wy * g.ws + i / g.ws + g.shift, x = wx * g.ws + i % g.ws + g.shift;
  if (y >= g.hp) y -= g.hp;
  if (x >= g.wp) x -= g.wp;
  return (y < g.h && x < g.w) ? (bi * g.h + y) * g.w + x : -1;
}

// reverse: the window row that token row `row` of (b, h, w) comes back from (never padding)
__device__ __forceinline__ long win_reverse_src(const WinGeom& g, long row) {
  const int x = (int)(row % g.w), y = (int)((row / g.w) % g.h);
  const long bi = row / ((long)g.w * g.h);
  int py = y - g.shift, px = x - g.shift;
  if (py < 0) py += g.hp;
  if (px < 0) px += g.wp;
  return (((bi * g.nh + py / g.ws) * g.nw + px / g.ws) * g.ws + py % g.ws) * g.ws + px % g.ws;
}

}  // namespace dhd
