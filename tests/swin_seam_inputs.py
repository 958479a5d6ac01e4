"""Seeded inputs and the float64 twin of the Swin seam operators (dhd_amd/swin_seam.py), shared by tests/test_swin_seam_capi.py
and tests/test_gpu_swin_seam.py (a helper module of the tests, not a conftest).

The twin is torch on the CPU in float64.  For the merge it is, literally, today's code: the `F.pad` and the
`reshape.permute.reshape` of `PatchMerging.forward`, then `F.layer_norm` over 4C.  For the embed it is
`flatten(2).transpose(1, 2)` and `F.layer_norm` over C.  Gradients are autograd's.  Everything is computed once per
(kind, case, precision) and cached; the cached tensors are never modified.

Precisions name what the operator is handed: 'f32' float32 in and out, 'f32_bf16' / 'f32_f16' float32 in with a half result
(and therefore a half incoming gradient), 'bf16' bfloat16 in and out, and for the embed 'bf16_f32', a bfloat16 conv output with a
float32 result (what nn.LayerNorm emits under autocast).  A half input or gradient is the seeded float32 tensor rounded to that
type; the twin is fed exactly those stored values, so its result is the exact function of what the operator read.
"""
import functools

import torch
import torch.nn.functional as F

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
EPS = 1e-5

# name -> (B, H, W, C)
MERGE_CASES = {
    'odd_both_c8': (2, 5, 7, 8),            # padding on both axes; the narrowest row (4C = 32)
    'even_c96': (2, 6, 10, 96),             # 4C = 384, not a power of two
    'odd_h_c128': (1, 9, 12, 128),          # DHD-L's stage-0 width; one axis padded
    'one_token_c256': (1, 1, 1, 256),       # three of four sources in the padding
    'cmax': (1, 2, 3, 512),                 # 4C = 2048, the advertised limit
    'many_rows_c32': (3, 40, 44, 32),       # 1320 output rows: several backward workgroups, the last ragged
}
# name -> (B, C, H, W)
EMBED_CASES = {
    'tiny_c8': (2, 8, 3, 5),                # 15 pixels: less than one tile; misaligned planes
    'c96': (1, 96, 7, 19),                  # 133 pixels: ragged tail; C not a power of two
    'two_images_c128': (2, 128, 9, 33),     # 297 pixels per image: tiles at an image's end
    'cmax': (1, 256, 4, 17),                # the advertised limit
    'aligned_c128': (1, 128, 8, 16),        # the wide-access path
}
CASES = {'merge': MERGE_CASES, 'embed': EMBED_CASES}

# name -> (x dtype, result dtype = dtype of the incoming gradient)
PRECISIONS = {'f32': (F32, F32), 'f32_bf16': (F32, BF16), 'f32_f16': (F32, F16), 'bf16': (BF16, BF16)}
EMBED_PRECISIONS = dict(PRECISIONS, bf16_f32=(BF16, F32))


def precisions(kind):
    return EMBED_PRECISIONS if kind == 'embed' else PRECISIONS


def grid(kind):
    return [(c, p) for c in CASES[kind] for p in precisions(kind)]


def x_shape(kind, case):
    if kind == 'merge':
        B, H, W, C = MERGE_CASES[case]
        return (B, H * W, C)
    return EMBED_CASES[case]


def norm_len(kind, case):
    return 4 * MERGE_CASES[case][3] if kind == 'merge' else EMBED_CASES[case][1]


def out_shape(kind, case):
    if kind == 'merge':
        B, H, W, C = MERGE_CASES[case]
        return (B, -(-H // 2) * -(-W // 2), 4 * C)
    B, C, H, W = EMBED_CASES[case]
    return (B, H * W, C)


def _gen(kind, case, salt):
    return torch.Generator().manual_seed(100000 * (1 + (kind == 'embed')) + 1000 * (list(CASES[kind]).index(case) + 1) + salt)


@functools.lru_cache(maxsize=None)
def inputs(kind, case, prec):
    """-> dict of CPU tensors in the dtypes the operator is handed: x (merge: (B, H * W, C) tokens; embed: (B, C, H, W)), gamma,
    beta (float32, the normalised length), dy (the result's shape, its dtype)."""
    xdt, odt = precisions(kind)[prec]
    n = norm_len(kind, case)
    x = (torch.randn(x_shape(kind, case), generator=_gen(kind, case, 1)) * 1.5 + 0.5).to(xdt)
    gamma = 1.0 + 0.2 * torch.randn(n, generator=_gen(kind, case, 2))
    beta = 0.1 * torch.randn(n, generator=_gen(kind, case, 3))
    dy = torch.randn(out_shape(kind, case), generator=_gen(kind, case, 4)).to(odt)
    return dict(x=x, gamma=gamma, beta=beta, dy=dy)


# ------------------------------------------------------------------------------------------------ the twin

def merge64(x, gamma, beta, H, W):
    """PatchMerging.forward up to the input of `reduction` (stride 2), as it stands."""
    B, L, C = x.shape
    s = 2
    x = x.view(B, H, W, C)
    if H % s or W % s:
        x = F.pad(x, (0, 0, 0, W % s, 0, H % s))
    Hp, Wp = x.shape[1] // s, x.shape[2] // s
    x = x[:, :Hp * s, :Wp * s].reshape(B, Hp, s, Wp, s, C).permute(0, 1, 3, 5, 2, 4).reshape(B, Hp * Wp, C * s * s)
    return F.layer_norm(x, (4 * C,), gamma, beta, EPS)


def embed64(x, gamma, beta):
    """PatchEmbed.forward after the projection."""
    return F.layer_norm(x.flatten(2).transpose(1, 2), (x.shape[1],), gamma, beta, EPS)


def call64(kind, case, x, gamma, beta):
    if kind == 'merge':
        B, H, W, C = MERGE_CASES[case]
        return merge64(x, gamma, beta, H, W)
    return embed64(x, gamma, beta)


@functools.lru_cache(maxsize=None)
def twin(kind, case, prec):
    """-> (Y64, dx64, dgamma64, dbeta64) of the operator on the stored inputs."""
    v = inputs(kind, case, prec)
    x, g, b = (v[k].double().requires_grad_() for k in ('x', 'gamma', 'beta'))
    y = call64(kind, case, x, g, b)
    dx, dg, db = torch.autograd.grad(y, (x, g, b), v['dy'].double())
    return y.detach(), dx, dg, db


def scale_of(t):
    return max(1.0, float(t.abs().max()))
