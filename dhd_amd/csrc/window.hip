// Shifted-window partition / reverse of the Swin backbone (DHD-L: backbones/swin.py:448-513 in the reference's ShiftWindowMSA.forward)
// as ONE gather each way.  The reference pads the (B, H, W, C) token map to multiples of the window, rolls it by -shift, and cuts it into
// windows (three copies of the activation: F.pad, torch.roll, permute + reshape); after attention it undoes the three (three more).
// Both directions are permutations of token rows (plus zero rows for the padding), so each is a row copy through an index map:
//   partition: out[b][wy][wx][iy][ix][:] = in[b][y][x][:]  with (y, x) = ((wy ws + iy + shift) mod Hp, (wx ws + ix + shift) mod Wp), 0 outside H x W
//   reverse  : out[b][y][x][:] = win[b][wy][wx][iy][ix][:] with (wy ws + iy, wx ws + ix) = ((y - shift) mod Hp, (x - shift) mod Wp)
// Each is also the other's transpose (the gradient of one is the other applied to the gradient).  The element type may change on the
// way (float32 LayerNorm output -> the autocast dtype the qkv projection would cast to anyway; half gradients -> float32).
#include "window_geom.h"

namespace {

using dhd::WinGeom;

constexpr int kWinBlock = 256;

// one thread per (row, group of 8 channels); rows of the OUTPUT are walked in order, the source row comes from the index map
template <typename TI, typename TO, bool REVERSE>
__global__ __launch_bounds__(kWinBlock) void window_rows(const TI* __restrict__ in, TO* __restrict__ out, WinGeom g) {
  const int groups = g.c >> 3;
  const long rows = REVERSE ? (long)g.b * g.h * g.w : (long)g.b * g.hp * g.wp;
  const long total = rows * groups;
  for (long idx = (long)blockIdx.x * kWinBlock + threadIdx.x; idx < total; idx += (long)gridDim.x * kWinBlock) {
    const int cg = (int)(idx % groups);
    const long row = idx / groups;
    const long src = REVERSE ? dhd::win_reverse_src(g, row) : dhd::win_partition_src(g, row);   // source row, -1 = zeros
    float v[8];
    if (src < 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = 0.f;
    } else {
      dhd::load8<TI>(in + src * g.c + cg * 8, v);
    }
    dhd::store8<TO>(out + row * g.c + cg * 8, v);
  }
}

template <typename TI, typename TO>
int window_launch(const void* in, void* out, const WinGeom& g, int reverse, hipStream_t st) {
  const long rows = reverse ? (long)g.b * g.h * g.w : (long)g.b * g.hp * g.wp;
  long blocks = (rows * (g.c >> 3) + kWinBlock - 1) / kWinBlock;
  if (blocks > 65536) blocks = 65536;
  if (reverse) hipLaunchKernelGGL((window_rows<TI, TO, true>), dim3((unsigned)blocks), dim3(kWinBlock), 0, st, (const TI*)in, (TO*)out, g);
  else hipLaunchKernelGGL((window_rows<TI, TO, false>), dim3((unsigned)blocks), dim3(kWinBlock), 0, st, (const TI*)in, (TO*)out, g);
  DHD_LAUNCH_CHECK();
  return DHD_OK;
}

}  // namespace

extern "C" int dhd_window_rows(const void* in, void* out, int in_dtype, int out_dtype, int b, int h, int w, int c, int window, int shift,
                               int reverse, void* stream) {
  if (!in || !out) return DHD_EINVAL;
  if (!dhd_aligned(16, in, out)) return DHD_EINVAL;   // load8 / store8
  if (in_dtype < 0 || in_dtype > 2 || out_dtype < 0 || out_dtype > 2 || b <= 0 || h <= 0 || w <= 0 || c <= 0 || (c & 7) || window <= 0 ||
      shift < 0 || shift >= window)
    return DHD_EUNSUPPORTED;
  const WinGeom g = dhd::win_geom(b, h, w, c, window, shift);
  if ((long)b * g.hp * g.wp >= (1L << 40)) return DHD_EUNSUPPORTED;
  hipStream_t st = dhd_stream(stream);
  return dhd::with_dtype<dhd::HipHalf>(in_dtype, [&](auto* ti) {
    return dhd::with_dtype<dhd::HipHalf>(out_dtype, [&](auto* to) {
      return window_launch<std::remove_pointer_t<decltype(ti)>, std::remove_pointer_t<decltype(to)>>(in, out, g, reverse, st);
    });
  });
}
