"""Inputs, shape grid and float64 twins of the UNet seam operators (dhd_amd/unet_seam.py), shared by tests/test_unet_seam_inputs.py
(CPU) and tests/test_gpu_unet_seam.py (GPU).  A helper module, not a conftest.

The pooling rule, restated (pool_rule): scan the 2 x 2 window in the order (0,0), (0,1), (1,0), (1,1) from max = -inf, winner the
first element; an element replaces the running maximum when v > max or isnan(v).

The up seam's twin is torch's own conv_transpose2d + pad + cat in float64 on the CPU with its autograd (twin), computed once per
(case, precision) from the values the operator is given (rounded to the precision's dtype first) and never modified."""
import functools

import torch
import torch.nn.functional as F

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = {'f32': F32, 'f16': F16, 'bf16': BF16}
BAR = 1e-4

# ------------------------------------------------------------------------------------------------ pooling
# (B, C, H, W): one window; odd H and W with rows of 7 (misaligned NCHW rows); even; odd H, one output column
POOL_SHAPES = [(2, 8, 2, 2), (2, 24, 5, 7), (1, 40, 6, 4), (3, 72, 9, 2)]


def pool_input(shape, dtype, seed=0):
    """relu(randn): about half the elements are zero, so whole windows tie; plus a gradient for the output."""
    gen = torch.Generator().manual_seed(100 + seed + sum(shape))
    x = torch.relu(torch.randn(shape, generator=gen)).to(dtype)
    gy = torch.randn(shape[0], shape[1], shape[2] // 2, shape[3] // 2, generator=gen).to(dtype)
    return x, gy


def pool_edge_input(dtype):
    """(1, 8, 4, 24): twelve windows per channel, the first row of windows holding the edge values: a four-way tie, zeros, one
    NaN first / last, two NaNs, +inf, +inf against NaN, all -inf, -inf with one finite; the second row of windows random."""
    nan, inf = float('nan'), float('inf')
    wins = [(1., 1., 1., 1.), (0., 0., 0., 0.), (nan, 2., 3., 4.), (1., 2., 3., nan), (nan, 5., nan, 1.), (1., inf, 2., 3.),
            (inf, nan, 1., 2.), (-inf, -inf, -inf, -inf), (-inf, -inf, -3., -inf), (inf, inf, 1., inf), (nan, nan, nan, nan), (-0., 0., -0., 0.)]
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(1, 8, 4, 24, generator=gen)
    for c in range(8):
        for j, w in enumerate(wins):
            w = w[c % 4:] + w[:c % 4]                    # rotate per channel: every edge value visits every position
            x[0, c, 0, 2 * j], x[0, c, 0, 2 * j + 1], x[0, c, 1, 2 * j], x[0, c, 1, 2 * j + 1] = w
    gy = torch.randn(1, 8, 2, 12, generator=gen)
    return x.to(dtype), gy.to(dtype)


def pool_rule(x):
    """-> (values, winner 0..3) of every whole 2 x 2 window of x (B, C, H, W) by the rule above, on any device."""
    B, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    xs = [x[:, :, di:2 * Ho:2, dj:2 * Wo:2] for di in (0, 1) for dj in (0, 1)]
    m = torch.full_like(xs[0], float('-inf'))
    win = torch.zeros(xs[0].shape, dtype=torch.long, device=x.device)
    for k, v in enumerate(xs):
        take = (v > m) | torch.isnan(v)
        m = torch.where(take, v, m)
        win = torch.where(take, torch.full_like(win, k), win)
    return m, win


def pool_rule_grad(x, gy):
    """The gradient the rule routes: 0 + gy at the winner of each window, zero elsewhere and in a dropped row / column."""
    B, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    _, win = pool_rule(x)
    gx = torch.zeros_like(x)
    for k, (di, dj) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        gx[:, :, di:2 * Ho:2, dj:2 * Wo:2] = torch.where(win == k, gy + torch.zeros_like(gy), torch.zeros_like(gy))
    return gx


def bits(t):
    """The tensor's bytes as integers: equality that tells NaNs and signed zeros apart."""
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same_but_nan_payload(a, b):
    """Equal bits, except that any NaN equals any NaN: torch.where on the CPU does not keep a half NaN's payload, so the restated
    rule is held to this; the operators are held to bits()."""
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (torch.isnan(a) & torch.isnan(b))).all())


# ------------------------------------------------------------------------------------------------ the up seam
# name: (B, Cin, Cout, C2, h, w, H, W).  The kernel's row tile is 32 x1 pixels; its column tile 128 columns: of 4 Cout in the
# forward (Cout = 16 / 32 / 48: half a tile, one tile, one and a half), of Cin in the backward (96 / 128 / 160).
UP_CASES = {
    'c32_3x5':          (1, 32, 16, 8, 3, 5, 6, 10),        # pads (0, 0)
    'c64_4x4_pad11':    (2, 64, 32, 32, 4, 4, 9, 9),        # pads (1, 1): nothing before, one after
    'c160_9x8_pad32':   (3, 160, 80, 48, 9, 8, 21, 18),     # pads (3, 2); Cout != C2; 216 rows: 7 row tiles, the last ragged
    'window_c128':      (1, 128, 64, 64, 2, 2, 4, 5),       # a single window; pads (0, 1)
    'window_c1024':     (1, 1024, 512, 512, 2, 2, 4, 4),    # the deepest level's channels
    'map_1x1':          (2, 32, 16, 8, 1, 1, 2, 2),
    'rows_31':          (1, 32, 16, 8, 1, 31, 2, 62),
    'rows_32':          (2, 32, 16, 8, 4, 4, 8, 8),
    'rows_33':          (3, 32, 16, 8, 1, 11, 2, 22),
    'cols_192_cin96':   (1, 96, 48, 8, 3, 5, 7, 10),        # pads (1, 0)
}


def up_inputs(case, prec):
    """x1, x2 (channels_last), weight, bias and the gradient of the output, in the precision's dtype (bias float32)."""
    B, Cin, Cout, C2, h, w, H, W = UP_CASES[case]
    dt = DTYPES[prec]
    gen = torch.Generator().manual_seed(7 + sum(UP_CASES[case]))
    r = lambda *s: torch.randn(*s, generator=gen)
    v = dict(x1=r(B, Cin, h, w), x2=r(B, C2, H, W), weight=r(Cin, Cout, 2, 2) / (Cin ** 0.5), bias=r(Cout) * 0.5, gout=r(B, C2 + Cout, H, W))
    out = {k: t.to(dt) for k, t in v.items()}
    out['bias'] = v['bias']
    for k in ('x1', 'x2', 'gout'):
        out[k] = out[k].contiguous(memory_format=torch.channels_last)
    return out


def up_reference(x1, x2, weight, bias):
    """`_Up.forward` up to its double convolution, in whatever dtype and device the tensors have."""
    y = F.conv_transpose2d(x1, weight, bias, stride=2)
    dy, dx = x2.size(2) - y.size(2), x2.size(3) - y.size(3)
    return torch.cat([x2, F.pad(y, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])], dim=1)


@functools.lru_cache(maxsize=None)
def twin(case, prec):
    """-> dict(out, gx1, gx2, gweight, gbias) in float64 from the precision's values."""
    v = up_inputs(case, prec)
    x1, x2, wgt, b = (v[k].double().contiguous().requires_grad_() for k in ('x1', 'x2', 'weight', 'bias'))
    out = up_reference(x1, x2, wgt, b)
    out.backward(v['gout'].double())
    return dict(out=out.detach(), gx1=x1.grad, gx2=x2.grad, gweight=wgt.grad, gbias=b.grad)


def up_einsum(x1, x2, weight, bias):
    """The same map written out: out[b, C2 + o, 2y + i + top, 2x + j + left] = bias[o] + sum_c x1[b, c, y, x] weight[c, o, i, j]."""
    B, Cin, h, w = x1.shape
    _, C2, H, W = x2.shape
    Cout = weight.shape[1]
    top, left = (H - 2 * h) // 2, (W - 2 * w) // 2
    out = torch.zeros(B, C2 + Cout, H, W, dtype=x1.dtype)
    out[:, :C2] = x2
    q = torch.einsum('bcyx,coij->boyixj', x1, weight) + bias.view(1, -1, 1, 1, 1, 1)
    out[:, C2:, top:top + 2 * h, left:left + 2 * w] = q.reshape(B, Cout, 2 * h, 2 * w)
    return out


def scale_of(t):
    return max(1.0, float(t.abs().max()))
