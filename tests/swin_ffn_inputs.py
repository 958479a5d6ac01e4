"""Seeded inputs and the float64 twin of the Swin FFN operator (dhd_amd/swin_ffn.py), shared by tests/test_swin_ffn_capi.py and
tests/test_gpu_swin_ffn.py (a helper module of the tests, not a conftest).

The twin is torch on the CPU in float64 and does, literally and in this order, what the second half of the reference's block
does: `F.layer_norm` -> `F.linear` -> `F.gelu` (exact) -> `F.linear` -> the residual add.  It is fed the stored values the operator
reads: x in its storage type (the seeded float32 tensor rounded to it), every parameter in float32.  Everything is computed once
per case and cached; the cached tensors are never modified.

Precisions name (x dtype, GEMM dtype): 'f32' all float32 (bf16x3 products), 'f32_bf16' / 'f32_f16' a float32 residual stream
under autocast, 'bf16' / 'f16' a half model."""
import functools

import torch
import torch.nn.functional as F

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
EPS = 1e-5

# the tails of a 32-row wave tile and of a 128-row workgroup; 300 is three workgroups, the last ragged
ROWS = (1, 31, 33, 127, 129, 300)
CHANNELS = (128, 256)
PRECISIONS = {'f32': (F32, F32), 'f32_bf16': (F32, BF16), 'f32_f16': (F32, F16), 'bf16': (BF16, BF16), 'f16': (F16, F16)}

# name -> (rows, C, LayerNorm?, tails?)
CASES = {}
for _c in CHANNELS:
    for _i, _r in enumerate(ROWS):
        CASES[f'r{_r}_c{_c}_ln'] = (_r, _c, True, False)
    for _r in (33, 300):
        CASES[f'r{_r}_c{_c}_plain'] = (_r, _c, False, False)          # FFN.forward(x) with identity None
    CASES[f'r129_c{_c}_tails'] = (129, _c, True, True)               # pre-activations that reach +-12: both GELU tails
TAIL = 12.0


def _gen(case, salt):
    return torch.Generator().manual_seed(1000 * (list(CASES).index(case) + 1) + salt)


@functools.lru_cache(maxsize=None)
def inputs(case, prec):
    """-> dict of CPU tensors as the operator is handed them: x (rows, C) in its storage type; gamma, beta (C) or None; w1 (4C, C),
    b1 (4C), w2 (C, 4C), b2 (C) in float32 (in a half model: in x's type).  Weights ~ N(0, 1 / fan_in) so that outputs are O(1); in a `tails` case w1 and b1 are
    scaled so that the largest pre-activation magnitude is TAIL (checked by the capi test on the twin)."""
    rows, C, ln, tails = CASES[case]
    xdt, _ = PRECISIONS[prec]
    H = 4 * C
    x = (torch.randn(rows, C, generator=_gen(case, 1)) * 1.5 + 0.5).to(xdt)
    gamma = 1.0 + 0.2 * torch.randn(C, generator=_gen(case, 2)) if ln else None
    beta = 0.1 * torch.randn(C, generator=_gen(case, 3)) if ln else None
    w1 = torch.randn(H, C, generator=_gen(case, 4)) / C ** 0.5
    b1 = 0.1 * torch.randn(H, generator=_gen(case, 5))
    w2 = torch.randn(C, H, generator=_gen(case, 6)) / H ** 0.5
    b2 = 0.1 * torch.randn(C, generator=_gen(case, 7))
    if tails:
        pre = pre_activation64(x, gamma, beta, w1, b1)
        k = TAIL / float(pre.abs().max())
        w1, b1 = (w1 * k).float(), (b1 * k).float()
    v = dict(x=x, gamma=gamma, beta=beta, w1=w1, b1=b1, w2=w2, b2=b2)
    if xdt != F32:      # a half model stores half parameters: the operator reads them as .float(), the twin reads the same values
        v = {k: (None if t is None else t.to(xdt)) for k, t in v.items()}
    return v


# ------------------------------------------------------------------------------------------------ the twin

def pre_activation64(x, gamma, beta, w1, b1):
    h = x.double()
    if gamma is not None:
        h = F.layer_norm(h, (h.shape[-1],), gamma.double(), beta.double(), EPS)
    return F.linear(h, w1.double(), b1.double())


def ffn64(x, gamma, beta, w1, b1, w2, b2):
    """layer_norm -> linear -> gelu (exact) -> linear -> add, in float64 on what was stored."""
    h = F.gelu(pre_activation64(x, gamma, beta, w1, b1))
    return x.double() + F.linear(h, w2.double(), b2.double())


@functools.lru_cache(maxsize=None)
def twin(case, prec):
    v = inputs(case, prec)
    return ffn64(v['x'], v['gamma'], v['beta'], v['w1'], v['b1'], v['w2'], v['b2'])


def parent(v, xdt, mdt, device_type):
    """Today's module formulation on the tensors `v` in the same dtypes: torch layer_norm / linear / gelu / linear / add, under
    autocast where the GEMM dtype differs from x's (a half model's parameters are already of its type)."""
    x = v['x']
    if xdt != mdt:
        with torch.autocast(device_type, dtype=mdt):
            h = x if v['gamma'] is None else F.layer_norm(x, (x.shape[-1],), v['gamma'], v['beta'], EPS)
            return x + F.linear(F.gelu(F.linear(h, v['w1'], v['b1'])), v['w2'], v['b2'])
    h = x if v['gamma'] is None else F.layer_norm(x, (x.shape[-1],), v['gamma'], v['beta'], EPS)
    return x + F.linear(F.gelu(F.linear(h, v['w1'], v['b1'])), v['w2'], v['b2'])


def scale_of(ref):
    return max(1.0, float(ref.abs().max()))
