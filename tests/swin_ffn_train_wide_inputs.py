"""Seeded inputs and the float64 autograd twin of the Swin FFN training operator at C = 512 (dhd_amd.swin_ffn through the wide
training family, csrc/swin_ffn_wide_train.h), shared by tests/test_swin_ffn_wide_train_capi.py and
tests/test_gpu_swin_ffn_wide_train.py (a helper module of the tests, not a conftest).

The twin is the one of tests/swin_ffn_train_inputs.py -- torch autograd on the CPU in float64 over the literal module formulation
applied to the stored values the operator reads -- and its pieces (`formulation`, `parent`, `scale_tensor`, `scale_of`,
`_collect`) are imported from there, not copied.  Everything is computed once per (case, precision, scale setting) and cached;
the cached tensors are never modified."""
import functools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from swin_ffn_train_inputs import (BF16, EPS, F16, F32, PARAMS, PRECISIONS, SCALES, TAIL, TENSORS, _collect, formulation, parent,  # noqa: E402,F401
                                   scale_of, scale_tensor)

C = 512
# one row; the tail of a 32-row wave tile; the tail of a workgroup of 32, 64 or 96 rows; several ragged workgroups
ROWS = (1, 33, 129, 300)

# name -> (rows, tails?)
CASES = {f'r{_r}_c{C}': (_r, False) for _r in ROWS}
CASES[f'r129_c{C}_tails'] = (129, True)               # pre-activations that reach +-12: gelu' in both tails


def scale_settings(case):
    """'drop' (3 images of 100 rows, the middle one dropped) at rows = 300 only."""
    return ('none', 'drop') if CASES[case][0] == 300 else ('none',)


GRID = [(c, p, s) for c in CASES for p in PRECISIONS for s in scale_settings(c)]


def _gen(case, salt):
    return torch.Generator().manual_seed(9000 * (list(CASES).index(case) + 1) + salt)


@functools.lru_cache(maxsize=None)
def inputs(case, prec):
    """-> dict of CPU tensors as the operator is handed them: x, dout (rows, 512) in the storage type; gamma, beta (512),
    w1 (2048, 512), b1 (2048), w2 (512, 2048), b2 (512) in float32 (in a half model: in x's type).  Weights ~ N(0, 1 / fan_in); in
    the `tails` case w1 and b1 are scaled so that the largest pre-activation magnitude is TAIL."""
    rows, tails = CASES[case]
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


@functools.lru_cache(maxsize=None)
def twin(case, prec, scale_name):
    """-> dict of float64 CPU tensors: out, dx, dgamma, dbeta, dw1, db1, dw2, db2."""
    v = inputs(case, prec)
    leaves = {k: v[k].double().requires_grad_() for k in ('x',) + PARAMS}
    s = scale_tensor(scale_name)
    out = formulation(leaves['x'], *(leaves[k] for k in PARAMS), None if s is None else s.double())
    out.backward(v['dout'].double())
    return _collect(out, leaves)
