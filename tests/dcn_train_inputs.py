"""Inputs, float64 twin and bars of the deform_conv (DCN in training) tests (no GPU needed here).

The cases are dcn_infer_inputs.CASES, by import, and two more: `pileup` (every tap of every pixel lands within one cell of
(2, 3): one long (cell, tap) segment per tap and many empty ones) and `zero_offset` (all offsets 0: DCN's initial state, where
the operator is the plain convolution).  gout is seeded randn.  The twin is oracle.dcn_oracle.deform_conv2d_backward in float64
on the STORED values: x and gout rounded to the precision under test, the float32 offsets and weights.

The offset gradient has a kink where a sampling coordinate is integral (the floor moves to the next cell) and at the validity
edges -1, H and W, which are integral too; the kernels place taps in float32.  So every random offset whose coordinate lies
within KINK of an integer is moved by +NUDGE, and `assert_no_kinks` shows that none is left: float32 and float64 then floor to
the same cell and the twin is unambiguous.  `zero_offset` is exempt: its coordinates are exactly integral in both arithmetics,
and its doffset is compared with today's HIP path instead.

Everything is computed once per (case, precision) and handed out read-only."""
import functools

import numpy as np
import torch

import dcn_infer_inputs as DI
from oracle import dcn_oracle

PRECISIONS = DI.PRECISIONS
LAYOUTS = DI.LAYOUTS
E_F32 = DI.E_F32          # the project's bar for this layer: |y - twin| <= E_F32 max(1, |twin|max)
HALF_FACTOR = 1.5         # half types: at most this times the error of today's path (and never held below the float32 bar)
KINK, NUDGE = 1e-3, 0.01

# (B, C, O, groups, H, W, dilation, offset scale)
CASES = dict(DI.CASES)
CASES['pileup'] = (1, 32, 32, 4, 6, 10, 1, None)
CASES['zero_offset'] = (2, 64, 64, 4, 5, 9, 1, 0.0)
assert list(CASES)[:6] == ['dhds_2x256x16x44', 'g13_2x32x6x10', 'g1_3x64to128x7x9_dil2', 'one_cell_1x256x1x1', 'outside_2x128to64x5x70',
                           'c512_1x512x8x12']
TENSORS = ('dx', 'doffset', 'dw')


def _base(h, w, dil):
    """Integer part of the sampling coordinates, (9, H, W) rows and columns, for pad = dil."""
    ii, jj = np.divmod(np.arange(9), 3)
    rows = (np.arange(h)[None, :, None] - dil + (ii * dil)[:, None, None]) + np.zeros((1, 1, w), np.int64)
    cols = (np.arange(w)[None, None, :] - dil + (jj * dil)[:, None, None]) + np.zeros((1, h, 1), np.int64)
    return rows, cols


def coordinates(case, offset, dtype=np.float64):
    """(B, 9, 2, H, W) sampling coordinates (row, column) of `offset` in the arithmetic `dtype`: base + offset."""
    b, c, o, g, h, w, dil, scale = CASES[case]
    rows, cols = _base(h, w, dil)
    off = offset.numpy().astype(dtype).reshape(b, 9, 2, h, w)
    return np.stack((rows.astype(dtype)[None] + off[:, :, 0], cols.astype(dtype)[None] + off[:, :, 1]), 2)


def kinks(case, offset):
    """Number of sampling coordinates within KINK of an integer, in float32 or in float64 arithmetic."""
    n = 0
    for dt in (np.float32, np.float64):
        co = coordinates(case, offset, dt).astype(np.float64)
        n += int((np.abs(co - np.round(co)) < KINK).sum())
    return n


def assert_no_kinks(case):
    if CASES[case][7] == 0.0:
        return
    assert kinks(case, inputs(case)[1]) == 0, case


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> x (B, C, H, W), offset (B, 18, H, W), weight (O, C / g, 3, 3), gout (B, O, H, W): float32 CPU tensors, not to be written."""
    b, c, o, g, h, w, dil, scale = CASES[case]
    if case in DI.CASES:
        x, offset, weight = DI.inputs(case)
        gen = torch.Generator().manual_seed(9100 + sorted(CASES).index(case))
    else:
        gen = torch.Generator().manual_seed(9100 + sorted(CASES).index(case))
        x = torch.randn(b, c, h, w, generator=gen)
        bound = 1.0 / (c * 9) ** 0.5
        weight = (torch.rand(o, c // g, 3, 3, generator=gen) * 2 - 1) * bound
        if scale is None:       # pileup: coordinate = (2, 3) + uniform(-1, 1)
            rows, cols = _base(h, w, dil)
            target = torch.rand(b, 9, 2, h, w, generator=gen) * 2 - 1
            target[:, :, 0] += 2.0 - torch.from_numpy(rows).float()[None]
            target[:, :, 1] += 3.0 - torch.from_numpy(cols).float()[None]
            offset = target.reshape(b, 18, h, w).contiguous()
        else:
            offset = torch.zeros(b, 18, h, w)
    gout = torch.randn(b, o, h, w, generator=gen)
    if scale != 0.0:
        offset = offset.clone()
        for dt in (np.float32, np.float64):     # move what lies at a kink, in either arithmetic
            co = coordinates(case, offset, dt).astype(np.float64)
            near = torch.from_numpy(np.abs(co - np.round(co)) < KINK).reshape(offset.shape)
            offset[near] += NUDGE
    return x, offset, weight, gout


def stored(case, prec):
    """(x, gout) as the precision under test stores them."""
    x, _, _, gout = inputs(case)
    return x.to(PRECISIONS[prec]), gout.to(PRECISIONS[prec])


@functools.lru_cache(maxsize=None)
def twin(case, prec):
    """{'out', 'dx', 'doffset', 'dw'}: float64 torch tensors from oracle.dcn_oracle on the stored values."""
    b, c, o, g, h, w, dil, scale = CASES[case]
    _, offset, weight, _ = inputs(case)
    xs, gs = (t.double().numpy() for t in stored(case, prec))
    out = dcn_oracle.deform_conv2d(xs, offset.numpy(), weight.numpy(), dil, dil, g)
    dx, doff, dw = dcn_oracle.deform_conv2d_backward(gs, xs, offset.numpy(), weight.numpy(), dil, dil, g)
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in (('out', out), ('dx', dx), ('doffset', doff), ('dw', dw))}


def scale_of(ref):
    return max(1.0, float(ref.abs().max()))


def rel_error(y, ref):
    """max |y - ref| / max(1, |ref|max), in float64 on the CPU."""
    return float((y.detach().cpu().double() - ref).abs().max()) / scale_of(ref)


def bar(prec, today_error):
    """The bound on rel_error of one tensor: float32 -> E_F32; a half type -> HALF_FACTOR x today's path's error on the same
    inputs, and the float32 bar where today's error is below it."""
    if prec == 'f32_bf16x3':
        return E_F32
    return HALF_FACTOR * today_error if today_error >= E_F32 else E_F32


class FixedOffset(torch.nn.Module):
    """Stands in for DCN.conv_offset: hands out the case's offsets (a leaf that collects their gradient)."""

    def __init__(self, offset):
        super().__init__()
        self.offset = offset

    def forward(self, x):
        return self.offset


def dcn_module(case, weight, offset, device='cpu', dtype=torch.float32):
    """A DCN of the case's shape with `weight` and with conv_offset replaced by the fixed `offset`."""
    from dhd_amd.depthnet import DCN
    b, c, o, g, h, w, dil, scale = CASES[case]
    m = DCN(c, o, 3, padding=dil, dilation=dil, groups=g).to(device=device, dtype=dtype)
    with torch.no_grad():
        m.weight.copy_(weight)
    m.conv_offset = FixedOffset(offset)
    return m
