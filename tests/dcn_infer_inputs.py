"""Inputs, float64 reference and error bounds of the dhd_deform_conv_infer tests (no GPU needed here).

Inputs are seeded randn (x, offsets x scale); the weight is DCN's default init (uniform in +-1 / sqrt(9 C)).  The reference R is
oracle/dcn_oracle.py in float64 on the STORED values of x (x rounded to the precision under test) and the float32 offsets and
weights.  Everything is computed once per (case, precision) and handed out read-only."""
import functools

import numpy as np
import torch

from oracle import dcn_oracle

PRECISIONS = {'f32_bf16x3': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}
LAYOUTS = ('nchw', 'channels_last')

# (B, C, O, groups, H, W, dilation, offset scale)
CASES = {
    'dhds_2x256x16x44': (2, 256, 256, 4, 16, 44, 1, 0.5),        # production channels and map
    'g13_2x32x6x10': (2, 32, 32, 4, 6, 10, 1, 3.0),              # G13's HeightNet: K and M padded, partial pixel tile
    'g1_3x64to128x7x9_dil2': (3, 64, 128, 1, 7, 9, 2, 3.0),      # groups = 1, O != C, dilation 2, 63 pixels
    'one_cell_1x256x1x1': (1, 256, 256, 4, 1, 1, 1, 0.5),
    'outside_2x128to64x5x70': (2, 128, 64, 4, 5, 70, 1, 40.0),   # nearly every tap outside, W no multiple of the tile
    'c512_1x512x8x12': (1, 512, 512, 4, 8, 12, 1, 0.5),          # C / g = 128
}

E_F32 = 1e-4     # the bound test_dcn_hip_sampling_vs_grid_sample_formulation holds this layer's output to


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> x float32 (B, C, H, W), offset float32 (B, 18, H, W), weight float32 (O, C / g, 3, 3): CPU tensors, not to be written."""
    b, c, o, g, h, w, dil, scale = CASES[case]
    gen = torch.Generator().manual_seed(9000 + sorted(CASES).index(case))
    x = torch.randn(b, c, h, w, generator=gen)
    offset = torch.randn(b, 18, h, w, generator=gen) * scale
    bound = 1.0 / (c * 9) ** 0.5
    weight = (torch.rand(o, c // g, 3, 3, generator=gen) * 2 - 1) * bound
    return x, offset, weight


def stored_x(case, prec):
    """x as the precision under test stores it (float32 values of the rounded tensor)."""
    return inputs(case)[0].to(PRECISIONS[prec])


@functools.lru_cache(maxsize=None)
def _columns(case, prec):
    b, c, o, g, h, w, dil, scale = CASES[case]
    x, offset, _ = inputs(case)
    xs = stored_x(case, prec).double().numpy()
    return dcn_oracle.deform_im2col(xs, offset.numpy(), 3, dil, dil)       # (B, C * 9, H * W) float64; pad = dil


def _product(case, col, weight64):
    b, c, o, g, h, w, dil, scale = CASES[case]
    wg = weight64.reshape(g, o // g, (c // g) * 9)
    return np.matmul(wg[None], col.reshape(b, g, (c // g) * 9, h * w)).reshape(b, o, h, w)


@functools.lru_cache(maxsize=None)
def reference(case, prec):
    """R: dcn_oracle.deform_conv2d's value (its columns times the float64 weight), float64 torch tensor (B, O, H, W)."""
    return torch.from_numpy(_product(case, _columns(case, prec), inputs(case)[2].double().numpy()))


@functools.lru_cache(maxsize=None)
def bound(case, prec):
    """E of |y - R| <= E max(1, |R|max).  float32: 1e-4.  Half: 2 E0, E0 = max |R - chain| with the chain = the oracle's columns of
    the half-rounded x rounded to the half type, the weights rounded to it, a float64 product, the result rounded to the type."""
    if prec == 'f32_bf16x3':
        return E_F32
    dt = PRECISIONS[prec]
    col = torch.from_numpy(_columns(case, prec)).to(dt).double().numpy()
    wgt = inputs(case)[2].to(dt).double().numpy()
    chain = torch.from_numpy(_product(case, col, wgt)).to(dt).double()
    return 2 * float((reference(case, prec) - chain).abs().max())


def scale_of(ref):
    return max(1.0, float(ref.abs().max()))
