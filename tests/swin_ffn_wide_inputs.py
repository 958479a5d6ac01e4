"""Seeded inputs and the float64 twin of the wide Swin FFN operator (C = 512 and 1024: csrc/swin_ffn_wide.h), shared by
tests/test_swin_ffn_wide_capi.py and tests/test_gpu_swin_ffn_wide.py (a helper module of the tests, not a conftest).

Built the way tests/swin_ffn_inputs.py builds its cases, and on its functions: the twin (`ffn64`), the parent formulation, the
precisions and the tail scale are imported from there, not restated.  Everything is computed once per case and cached; the cached
tensors are never modified.

Rows.  A workgroup owns 32 rows with float32 GEMMs and, with half GEMMs, 96 rows at C = 512 and 64 at C = 1024; a wave normalises
a quarter of them and an MFMA column tile is 32: 1, 31, 33, 63, 65, 95, 97 are both sides of a 32-, a 64- and a 96-row tile, 129 is
more than one workgroup of every size, 200 is more than two (three, six) with a ragged last one.  The hidden dimension is walked
in chunks of 128 or 256 units (16 or 32 chunks at C = 512, 32 at C = 1024), each wave owning a quarter of the output channels, so
every case crosses chunk and channel-slice boundaries."""
import functools

import torch

from swin_ffn_inputs import EPS, PRECISIONS, TAIL, ffn64, parent, pre_activation64, scale_of  # noqa: F401

F32 = torch.float32
ROWS = (1, 31, 33, 63, 65, 95, 97, 129, 200)
CHANNELS = (512, 1024)

# name -> (rows, C, LayerNorm?, tails?)
CASES = {}
for _c in CHANNELS:
    for _r in ROWS:
        CASES[f'r{_r}_c{_c}_ln'] = (_r, _c, True, False)
    for _r in (33, 200):
        CASES[f'r{_r}_c{_c}_plain'] = (_r, _c, False, False)          # FFN.forward(x) with identity None
    CASES[f'r129_c{_c}_tails'] = (129, _c, True, True)               # pre-activations that reach +-12: both GELU tails


def _gen(case, salt):
    return torch.Generator().manual_seed(77000 + 1000 * (list(CASES).index(case) + 1) + salt)


@functools.lru_cache(maxsize=None)
def _inputs32(case):
    """The float32 tensors of a case; the half-model precisions round these."""
    rows, C, ln, tails = CASES[case]
    H = 4 * C
    x = torch.randn(rows, C, generator=_gen(case, 1)) * 1.5 + 0.5
    gamma = 1.0 + 0.2 * torch.randn(C, generator=_gen(case, 2)) if ln else None
    beta = 0.1 * torch.randn(C, generator=_gen(case, 3)) if ln else None
    w1 = torch.randn(H, C, generator=_gen(case, 4)) / C ** 0.5
    b1 = 0.1 * torch.randn(H, generator=_gen(case, 5))
    w2 = torch.randn(C, H, generator=_gen(case, 6)) / H ** 0.5
    b2 = 0.1 * torch.randn(C, generator=_gen(case, 7))
    return dict(x=x, gamma=gamma, beta=beta, w1=w1, b1=b1, w2=w2, b2=b2)


@functools.lru_cache(maxsize=None)
def _inputs_as(case, xdt):
    tails = CASES[case][3]
    v = dict(_inputs32(case))
    v['x'] = v['x'].to(xdt)
    if tails:
        pre = pre_activation64(v['x'], v['gamma'], v['beta'], v['w1'], v['b1'])
        k = TAIL / float(pre.abs().max())
        v['w1'], v['b1'] = (v['w1'] * k).float(), (v['b1'] * k).float()
    if xdt != F32:      # a half model stores half parameters: the operator reads them as .float(), the twin reads the same values
        v = {k: (None if t is None else t.to(xdt)) for k, t in v.items()}
    return v


def inputs(case, prec):
    """-> dict of CPU tensors as the operator is handed them: x (rows, C) in its storage type; gamma, beta (C) or None; w1 (4C, C),
    b1 (4C), w2 (C, 4C), b2 (C) in float32 (in a half model: in x's type).  Weights ~ N(0, 1 / fan_in) so that outputs are O(1);
    in a `tails` case w1 and b1 are scaled so that the largest pre-activation magnitude is TAIL on the stored x.  The three
    precisions with float32 tokens share their tensors (and their twin): only the GEMM type differs."""
    return _inputs_as(case, PRECISIONS[prec][0])


@functools.lru_cache(maxsize=None)
def _twin_as(case, xdt):
    v = _inputs_as(case, xdt)
    return ffn64(v['x'], v['gamma'], v['beta'], v['w1'], v['b1'], v['w2'], v['b2'])


def twin(case, prec):
    return _twin_as(case, PRECISIONS[prec][0])
