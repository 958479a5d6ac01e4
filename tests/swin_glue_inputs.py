"""Seeded inputs and the float64 twin of the Swin glue operators (dhd_amd/swin_glue.py), shared by tests/test_swin_glue_capi.py
and tests/test_gpu_swin_glue.py (a helper module of the tests, not a conftest).

The twin is torch on the CPU in float64 and does, literally and in this order, what the reference's block does around its
attention: `F.layer_norm`, `F.pad`, `torch.roll`, permute + reshape -- and on the way back reshape + permute, `torch.roll`, the
crop, and the residual add.  Its gradients are autograd's.  Everything is computed once per (case, precision) and cached; the
cached tensors are never modified.

Precisions name what the operator is handed: 'f32' float32 in and out, 'f32_bf16' / 'f32_f16' float32 in with a half result
(and therefore a half incoming gradient), 'bf16' bfloat16 in and out.  A half input or gradient is the seeded float32 tensor
rounded to that type; the twin is fed exactly those stored values, so its result is the exact function of what the operator read.
"""
import functools

import torch
import torch.nn.functional as F

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
EPS = 1e-5

# name -> (B, H, W, ws, shift, C); ws == 0: the identity map over (B, H, C) rows (W unused)
CASES = {
    'pad_shift_c96': (2, 10, 15, 7, 3, 96),         # padding on both axes, the seam, C not a power of two
    'ws12_c128': (2, 24, 36, 12, 6, 128),           # DHD-L's window; 1728 tokens: several workgroups of the backward, the last ragged
    'noshift_c8': (3, 5, 9, 4, 0, 8),               # one vector per row, odd row count
    'one_window_c1024': (1, 3, 5, 7, 0, 1024),      # a window that is mostly padding, a wide row (two steps per lane)
    'one_token_cmax': (1, 1, 1, 1, 0, 2048),        # the largest advertised C (four steps per lane)
    'rows_c96': (2, 37, 1, 0, 0, 96),               # the identity map: norm2's form
}
WINDOW_CASES = tuple(k for k, v in CASES.items() if v[3] > 0)

# name -> (x dtype, result dtype = dtype of the incoming gradient)
PRECISIONS = {'f32': (F32, F32), 'f32_bf16': (F32, BF16), 'f32_f16': (F32, F16), 'bf16': (BF16, BF16)}


def window_arg(case):
    B, H, W, ws, sh, C = CASES[case]
    return (H, W, ws, sh) if ws else None


def out_shape(case):
    B, H, W, ws, sh, C = CASES[case]
    return (B, -(-H // ws) * -(-W // ws), ws * ws, C) if ws else (B, H, C)


def _gen(case, salt):
    return torch.Generator().manual_seed(1000 * (list(CASES).index(case) + 1) + salt)


@functools.lru_cache(maxsize=None)
def inputs(case, prec):
    """-> dict of CPU tensors in the dtypes the operator is handed: x (B, H * W, C), gamma, beta (float32), dy (the result's shape,
    its dtype), win (the result's shape and dtype: windows to reverse), scale (float32 (B,): 0 and 1 / 0.9)."""
    B, H, W, ws, sh, C = CASES[case]
    xdt, odt = PRECISIONS[prec]
    tokens = H * W if ws else H
    x = (torch.randn(B, tokens, C, generator=_gen(case, 1)) * 1.5 + 0.5).to(xdt)
    gamma = 1.0 + 0.2 * torch.randn(C, generator=_gen(case, 2))
    beta = 0.1 * torch.randn(C, generator=_gen(case, 3))
    dy = torch.randn(out_shape(case), generator=_gen(case, 4)).to(odt)
    win = torch.randn(out_shape(case), generator=_gen(case, 5)).to(odt)
    scale = torch.tensor([0.0 if i % 2 else 1 / 0.9 for i in range(B)], dtype=F32)
    if B == 1:
        scale = torch.tensor([1 / 0.9], dtype=F32)
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, win=win, scale=scale)


# ------------------------------------------------------------------------------------------------ the twin

def partition64(t, H, W, ws, sh):
    """(B, H * W, C) -> (B, nW, ws * ws, C): F.pad, torch.roll, permute + reshape (ShiftWindowMSA.forward's CPU branch)."""
    B, L, C = t.shape
    t = t.view(B, H, W, C)
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    if pad_r or pad_b:
        t = F.pad(t, (0, 0, 0, pad_r, 0, pad_b))
    Hp, Wp = H + pad_b, W + pad_r
    if sh > 0:
        t = torch.roll(t, shifts=(-sh, -sh), dims=(1, 2))
    nh, nw = Hp // ws, Wp // ws
    return t.view(B, nh, ws, nw, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, nh * nw, ws * ws, C)


def reverse64(win, H, W, ws, sh):
    """(B, nW, ws * ws, C) -> (B, H * W, C): the inverse, in the inverse order."""
    B, C = win.shape[0], win.shape[-1]
    nh, nw = -(-H // ws), -(-W // ws)
    t = win.view(B, nh, nw, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, nh * ws, nw * ws, C)
    if sh > 0:
        t = torch.roll(t, shifts=(sh, sh), dims=(1, 2))
    return t[:, :H, :W].contiguous().view(B, H * W, C)


def ln_rows64(x, gamma, beta, case):
    B, H, W, ws, sh, C = CASES[case]
    y = F.layer_norm(x, (C,), gamma, beta, EPS)
    return partition64(y, H, W, ws, sh) if ws else y


def reverse_add64(win, identity, scale, case):
    B, H, W, ws, sh, C = CASES[case]
    r = reverse64(win, H, W, ws, sh)
    return identity + (r if scale is None else scale.view(-1, 1, 1) * r)


def pad_rows(case):
    """bool (B, nW, ws * ws): the rows of the partition that lie in the padding."""
    B, H, W, ws, sh, C = CASES[case]
    ones = torch.ones(B, H * W, 1, dtype=torch.float64)
    return partition64(ones, H, W, ws, sh)[..., 0] == 0


@functools.lru_cache(maxsize=None)
def ln_twin(case, prec):
    """-> (Y64, dx64, dgamma64, dbeta64) of the LayerNorm-rows operator on the stored inputs."""
    v = inputs(case, prec)
    x, g, b = (v[k].double().requires_grad_() for k in ('x', 'gamma', 'beta'))
    y = ln_rows64(x, g, b, case)
    dx, dg, db = torch.autograd.grad(y, (x, g, b), v['dy'].double())
    return y.detach(), dx, dg, db


@functools.lru_cache(maxsize=None)
def reverse_add_twin(case, prec, scaled):
    """-> (out64, dwin64, didentity64) of reverse + add on the stored inputs: win, the case's x as identity, reverse_add_gout as
    the incoming gradient; with `scaled` the case's scale, else none."""
    v = inputs(case, prec)
    win, ident = v['win'].double().requires_grad_(), v['x'].double().requires_grad_()
    out = reverse_add64(win, ident, v['scale'].double() if scaled else None, case)
    dwin, dident = torch.autograd.grad(out, (win, ident), reverse_add_gout(case, prec).double())
    return out.detach(), dwin, dident


@functools.lru_cache(maxsize=None)
def reverse_add_gout(case, prec):
    """The incoming gradient of reverse + add: identity's shape and dtype."""
    v = inputs(case, prec)
    return torch.randn(v['x'].shape, generator=_gen(case, 6)).to(v['x'].dtype)


def scale_of(t):
    return max(1.0, float(t.abs().max()))
