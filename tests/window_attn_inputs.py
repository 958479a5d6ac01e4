"""Inputs, float64 reference and error bounds of the dhd_window_attn_infer tests (no GPU needed here).

Inputs are seeded: randn q, k, v (scores have std ~ 1 at scale = 32^-0.5; one case scales q by 3 for scores up to ~ +-15), the
bias table randn * 0.5 so that the bias matters, regions from swin.shift_window_regions of the case's padded map.  The
reference R is the formula of section 16 of the header in float64 on the STORED values (qkv rounded to the precision under
test; the table stays float32).  Everything is computed once per (case, precision) and handed out read-only.

Bounds, |y - R| <= E max(1, |R|max):
  float32 (bf16x3)   E = 1e-4, the project's float32 layer bar (E_F32 of dcn_infer_inputs.py).
  fp16 / bf16        E = 2 E0, E0 = max |R - chain| with the chain = scores and softmax in float64 on the rounded inputs, P
                     rounded to the half type, the float64 P V rounded to the half type.  The factor 2 covers summation order
                     and the variant that rounds the unnormalised exponentials and divides afterwards."""
import functools

import numpy as np
import torch

PRECISIONS = {'f32_bf16x3': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}
HEAD_DIM = 32
SCALE = HEAD_DIM ** -0.5
E_F32 = 1e-4

# (Wh, Ww), padded map (H, W) or None for `windows` windows without regions, shift, B, heads, q scale
CASES = {
    'ws12_24x36_shift6_b2_nh4': ((12, 12), (24, 36), 6, 2, 4, 1.0),      # N = 144: no padding; corner window with four regions; w mod nW
    'ws7_21x14_shift3_nh3': ((7, 7), (21, 14), 3, 1, 3, 1.0),            # N = 49 padded to 64; odd head count
    'ws7_one_window_plain': ((7, 7), None, 0, 1, 1, 1.0),                # regions = NULL
    'ws4_8x8_shift2_b2_nh2': ((4, 4), (8, 8), 2, 2, 2, 1.0),             # N = 16: a single key tile
    'win3x5_nonsquare_nh2': ((3, 5), None, 0, 2, 2, 1.0),                # N = 15, Wh != Ww: a swapped y / x in the bias index shows
    'ws12_one_window_nh32': ((12, 12), None, 0, 1, 32, 1.0),             # stage-3 head count
    'ws12_24x36_shift6_q3': ((12, 12), (24, 36), 6, 2, 4, 3.0),          # scores up to ~ +-15
}
NEIGHBOUR_CASES = ('ws7_21x14_shift3_nh3', 'ws7_one_window_plain')       # N = 49: padded rows inside the kernel


def geometry(case):
    """-> (Wh, Ww, N, B, nW, nh)"""
    (wh, ww), hw, shift, b, nh, _ = CASES[case]
    nw = 1 if hw is None else (hw[0] // wh) * (hw[1] // ww)
    return wh, ww, wh * ww, b, nw, nh


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> qkv float32 (B, nW, N, 3 * nh * 32), table float32 ((2 Wh - 1)(2 Ww - 1), nh), regions uint8 (nW, N) or None: CPU
    tensors, not to be written."""
    from dhd_amd.swin import shift_window_regions
    (_, _), hw, shift, _, _, qscale = CASES[case]
    wh, ww, n, b, nw, nh = geometry(case)
    gen = torch.Generator().manual_seed(16000 + sorted(CASES).index(case))
    qkv = torch.randn(b, nw, n, 3, nh, HEAD_DIM, generator=gen)
    qkv[:, :, :, 0] *= qscale
    table = torch.randn((2 * wh - 1) * (2 * ww - 1), nh, generator=gen) * 0.5
    regions = None if hw is None else shift_window_regions(hw[0], hw[1], wh, shift, 'cpu')
    assert regions is None or (regions.dtype == torch.uint8 and tuple(regions.shape) == (nw, n))
    return qkv.reshape(b, nw, n, 3 * nh * HEAD_DIM), table, regions


def stored_qkv(case, prec):
    """qkv as the precision under test stores it."""
    return inputs(case)[0].to(PRECISIONS[prec])


def additive_term(case):
    """float64 (nW, nh, N, N): the bias looked up from the table plus -100 between different regions."""
    wh, ww, n, b, nw, nh = geometry(case)
    _, table, regions = inputs(case)
    ys, xs = np.divmod(np.arange(n), ww)
    index = (ys[:, None] - ys[None, :] + wh - 1) * (2 * ww - 1) + (xs[:, None] - xs[None, :] + ww - 1)       # [i, j]
    bias = table.double().numpy()[index.reshape(-1)].reshape(n, n, nh).transpose(2, 0, 1)                    # (nh, N, N)
    add = np.broadcast_to(bias[None], (nw, nh, n, n)).copy()
    if regions is not None:
        r = regions.numpy().astype(np.int64)
        add += np.where(r[:, :, None] != r[:, None, :], -100.0, 0.0)[:, None]
    return add


@functools.lru_cache(maxsize=None)
def _probabilities(case, prec):
    """float64 softmax (B, nW, nh, N, N) and v (B, nW, nh, N, 32) of the stored qkv."""
    wh, ww, n, b, nw, nh = geometry(case)
    x = stored_qkv(case, prec).double().numpy().reshape(b, nw, n, 3, nh, HEAD_DIM)
    q, k, v = (x[:, :, :, i].transpose(0, 1, 3, 2, 4) for i in range(3))                                    # (B, nW, nh, N, 32)
    s = SCALE * np.matmul(q, k.transpose(0, 1, 2, 4, 3)) + additive_term(case)[None]
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    return p / p.sum(-1, keepdims=True), v


def _to_out(o):
    b, nw, nh, n, d = o.shape
    return torch.from_numpy(np.ascontiguousarray(o.transpose(0, 1, 3, 2, 4)).reshape(b, nw, n, nh * d))


@functools.lru_cache(maxsize=None)
def reference(case, prec):
    """R: float64 torch tensor (B, nW, N, nh * 32)."""
    p, v = _probabilities(case, prec)
    return _to_out(np.matmul(p, v))


@functools.lru_cache(maxsize=None)
def bound(case, prec):
    if prec == 'f32_bf16x3':
        return E_F32
    dt = PRECISIONS[prec]
    p, v = _probabilities(case, prec)
    p = torch.from_numpy(p).to(dt).double().numpy()
    chain = _to_out(np.matmul(p, v)).to(dt).double()
    return 2 * float((reference(case, prec) - chain).abs().max())


def scale_of(ref):
    return max(1.0, float(ref.abs().max()))
