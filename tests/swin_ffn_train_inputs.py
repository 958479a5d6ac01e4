"""Seeded inputs and the float64 autograd twin of the Swin FFN training operator (dhd_amd.swin_ffn), shared by
tests/test_swin_ffn_train_capi.py and tests/test_gpu_swin_ffn_train.py (a helper module of the tests, not a conftest).

The twin is torch autograd on the CPU in float64 over the literal module formulation, `F.layer_norm` -> `F.linear` -> `F.gelu`
(exact) -> `F.linear` -> the per-image factor -> the residual add, applied to the stored values the operator reads: x and dout
in their storage type, every parameter as stored, the factors as float32.  It gives out and the gradients of x and of the seven
parameters for the seeded dout.  Everything is computed once per (case, precision, scale setting) and cached; the cached tensors
are never modified.

Precisions name (x dtype, GEMM dtype) as in swin_ffn_inputs.py."""
import functools

import torch
import torch.nn.functional as F

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
EPS = 1e-5

# the tails of a 32-row wave tile and of a 128-row workgroup; 300 is three workgroups, the last ragged
ROWS = (1, 33, 129, 300)
CHANNELS = (128, 256)
PRECISIONS = {'f32': (F32, F32), 'f32_bf16': (F32, BF16), 'f32_f16': (F32, F16), 'bf16': (BF16, BF16), 'f16': (F16, F16)}
TAIL = 12.0

# name -> (rows, C, tails?)
CASES = {}
for _c in CHANNELS:
    for _r in ROWS:
        CASES[f'r{_r}_c{_c}'] = (_r, _c, False)
    CASES[f'r129_c{_c}_tails'] = (129, _c, True)          # pre-activations that reach +-12: gelu' in both tails

# scale settings: None, or 3 images of 100 rows with a dropped one in the middle (keep = 0.9), at rows = 300 only
SCALES = {'none': None, 'drop': (1 / 0.9, 0.0, 1 / 0.9)}
TENSORS = ('out', 'dx', 'dgamma', 'dbeta', 'dw1', 'db1', 'dw2', 'db2')
PARAMS = ('gamma', 'beta', 'w1', 'b1', 'w2', 'b2')


def scale_settings(case):
    return ('none', 'drop') if CASES[case][0] == 300 else ('none',)


GRID = [(c, p, s) for c in CASES for p in PRECISIONS for s in scale_settings(c)]


def _gen(case, salt):
    return torch.Generator().manual_seed(7000 * (list(CASES).index(case) + 1) + salt)


def scale_tensor(name):
    """The per-image factors as the operator is handed them: float32 (images,), or None."""
    return None if SCALES[name] is None else torch.tensor(SCALES[name], dtype=F32)


@functools.lru_cache(maxsize=None)
def inputs(case, prec):
    """-> dict of CPU tensors as the operator is handed them: x, dout (rows, C) in the storage type; gamma, beta (C), w1 (4C, C),
    b1 (4C), w2 (C, 4C), b2 (C) in float32 (in a half model: in x's type).  Weights ~ N(0, 1 / fan_in); in a `tails` case w1 and
    b1 are scaled so that the largest pre-activation magnitude is TAIL."""
    rows, C, tails = CASES[case]
    xdt, _ = PRECISIONS[prec]
    H = 4 * C
    x = (torch.randn(rows, C, generator=_gen(case, 1)) * 1.5 + 0.5).to(xdt)
    gamma = 1.0 + 0.2 * torch.randn(C, generator=_gen(case, 2))
    beta = 0.1 * torch.randn(C, generator=_gen(case, 3))
    w1 = torch.randn(H, C, generator=_gen(case, 4)) / C ** 0.5
    b1 = 0.1 * torch.randn(H, generator=_gen(case, 5))
    w2 = torch.randn(C, H, generator=_gen(case, 6)) / H ** 0.5
    b2 = 0.1 * torch.randn(C, generator=_gen(case, 7))
    dout = torch.randn(rows, C, generator=_gen(case, 8)).to(xdt)
    if tails:
        pre = F.linear(F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), EPS), w1.double(), b1.double())
        k = TAIL / float(pre.abs().max())
        w1, b1 = (w1 * k).float(), (b1 * k).float()
    v = dict(x=x, gamma=gamma, beta=beta, w1=w1, b1=b1, w2=w2, b2=b2, dout=dout)
    if xdt != F32:      # a half model stores half parameters: the operator reads them as .float(), the twin reads the same values
        v = {k: t.to(xdt) for k, t in v.items()}
    return v


def formulation(x, gamma, beta, w1, b1, w2, b2, scale):
    """The literal module formulation in the dtypes it is handed (and under whatever autocast is active)."""
    h = F.layer_norm(x, (x.shape[-1],), gamma, beta, EPS)
    branch = F.linear(F.gelu(F.linear(h, w1, b1)), w2, b2)
    if scale is not None:
        images = scale.numel()
        branch = (branch.view(images, -1, x.shape[-1]) * scale.to(branch.dtype).view(images, 1, 1)).view(x.shape)
    return x + branch


def _collect(out, leaves):
    got = {'out': out.detach(), 'dx': leaves['x'].grad}
    got.update({'d' + k: leaves[k].grad for k in PARAMS})
    return got


@functools.lru_cache(maxsize=None)
def twin(case, prec, scale_name):
    """-> dict of float64 CPU tensors: out, dx, dgamma, dbeta, dw1, db1, dw2, db2."""
    v = inputs(case, prec)
    leaves = {k: v[k].double().requires_grad_() for k in ('x',) + PARAMS}
    s = scale_tensor(scale_name)
    out = formulation(leaves['x'], *(leaves[k] for k in PARAMS), None if s is None else s.double())
    out.backward(v['dout'].double())
    return _collect(out, leaves)


def parent(v, xdt, mdt, scale, device_type):
    """Today's module formulation with torch autograd on the tensors `v` in the same dtypes (under autocast where the GEMM dtype
    differs from x's) -> the same dict as the twin, in the dtypes torch gives."""
    leaves = {k: v[k].detach().clone().requires_grad_() for k in ('x',) + PARAMS}
    with torch.autocast(device_type, dtype=mdt, enabled=xdt != mdt):
        out = formulation(leaves['x'], *(leaves[k] for k in PARAMS), scale)
    out.backward(v['dout'].to(out.dtype))
    return _collect(out, leaves)


def scale_of(ref):
    return max(1.0, float(ref.abs().max()))
