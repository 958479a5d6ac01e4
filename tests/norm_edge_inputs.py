"""Inputs, float64 references and bounds of the normalisation kernels' value-edge tests: the training BatchNorm of
csrc/batchnorm.hip (both layouts) and the LayerNorm-bearing Swin operators (csrc/swin_glue.hip, swin_seam.h, swin_ffn.hip).  No GPU is needed
here: test_norm_edge_inputs.py checks on the CPU that every regime is what its name says after rounding to the storage type,
test_gpu_norm_edges.py runs the kernels on them.

Every kernel that computes a mean and a variance was tested on `randn * s + m` with |m| / s <= 2 only, where any variance formula
looks right.  The regimes below put ONE property at its edge per channel (BatchNorm) or per row (LayerNorm): an offset far larger
than the spread, a first element -- the one a one-pass kernel is tempted to take its shift from -- that is 0 or an outlier, a
constant or nearly constant channel (rstd reaches eps^-1/2 = 316 and the exact result is beta), and the sparse / bimodal maps of
a BEV grid.  One regime per channel of the same tensor with `plain` channels between them: one launch covers them all, and the
`plain` channels must come out bit for bit as in an all-`plain` tensor of the same shape.

Everything is seeded, computed once (functools.lru_cache) and handed out to be read, not written.  References are float64 on the
CPU on the STORED values (x and g rounded to the storage type, then widened); BatchNorm's is written out from the formulas, the
LayerNorm operators' are the float64 twins of swin_glue_inputs / swin_seam_inputs / swin_ffn*_inputs fed the new x.  The bound is the project's rule,
value_edge_inputs.bound: the operator's bar where the float32 torch formulation ("the mirror", run by the GPU test on the same
device) is itself within the bar of float64, else 4 x the mirror's error -- per tensor AND per channel / per row regime, so that a
large channel cannot hide a wrong small one."""
import functools

import torch

from value_edge_inputs import bound  # noqa: F401  (the one bound rule; re-exported to the tests)

DTYPES = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}
EPS = 1e-5

# --------------------------------------------------------------------------- A. BatchNorm channels

NEAR_CONSTANT_C = 1.9              # `c + 1e-3 |c| z`: var = 3.6e-6 < eps; just below a power of two, where a half type is finest
# the regime of each channel, repeated over the channels of wider tensors.  `offset_r`'s r depends on the storage type (OFFSET_R)
PERIOD = ('plain', 'offset_r', 'first_zero_30', 'first_outlier_100', 'constant_0', 'first_zero_100', 'constant_0.37',
          'first_outlier_1000', 'near_constant', 'constant_-2.5', 'first_zero_300', 'constant_100.3', 'sparse',
          'constant_first_zero', 'bimodal', 'tiny')
FAMILIES = ('plain', 'offset', 'first_zero', 'first_outlier', 'constant', 'constant_first_zero', 'near_constant', 'sparse',
            'bimodal', 'tiny')
# An offset at which `r + z` keeps 16 distinct values in the type also in a channel of 48 elements: float16 has steps of 0.125 in
# [128, 256) and of 0.5 / 1 around 1000; bfloat16 has steps of 0.125 in [16, 32) and of 0.5 in [64, 128).
OFFSET_R = {'f32': 1000.0, 'f16': 200.0, 'bf16': 30.0}
# Regimes a storage type cannot hold (fewer than 16 distinct values per channel after rounding; test_norm_edge_inputs.py checks
# that each entry is needed and that nothing else is missing).  Their channels carry `plain` instead.
#   bfloat16 (8 significant bits): `300 + z` has steps of 2, `100 + z` steps of 0.5 (16 values at best, fewer in small channels);
#   `1.9 (1 + 1e-3 z)` has steps of 2^-7 = 4 sigma; `5 + 0.05 z` steps of 2^-5 (13 values).  float16: `1.9 (1 + 1e-3 z)` has steps
#   of 2^-10 (about 15 values in 80 000 samples).
ABSENT = {'f32': (), 'f16': ('near_constant',), 'bf16': ('first_zero_100', 'first_zero_300', 'near_constant', 'bimodal')}
MIN_DISTINCT = 16
GAMMA_ZERO_AT, GAMMA_NEGATIVE_AT = PERIOD.index('constant_0'), PERIOD.index('bimodal')     # in the first period only

BN_BARS = {'f32': 2e-5, 'f16': 2e-3, 'bf16': 1.6e-2}      # of test_batchnorm2d_training_vs_torch; x 4 for dgamma / dbeta in halves
BN_SHAPES = {
    'nchw': ((2, 16, 200, 200),      # several plane chunks, the two-stream loop and its tail
             (3, 16, 16, 44),        # one short chunk, the tail loop only
             (1, 16, 4, 4)),         # cnt = 16
    'nhwc': ((6, 64, 32, 88),
             (2, 24, 6, 10),         # row lanes do not fill the workgroup
             (2, 2048, 4, 6)),       # two column groups; the regimes repeat over the channels
}
BN_CASES = tuple((layout, shape, dt) for layout in BN_SHAPES for shape in BN_SHAPES[layout] for dt in DTYPES)


def family(regime):
    for f in sorted(FAMILIES, key=len, reverse=True):
        if regime == f or regime.startswith(f + '_'):
            return f
    raise KeyError(regime)


def regime_of_channel(ch, dtype_name):
    r = PERIOD[ch % len(PERIOD)]
    return 'plain' if r in ABSENT[dtype_name] else r


def channel_regimes(c, dtype_name):
    return [regime_of_channel(ch, dtype_name) for ch in range(c)]


def regime_values(regime, z, gen, dtype_name='f32'):
    """The regime's channel (or row) from the standard normal z (cnt,), float64, BEFORE rounding to the storage type.  Element 0
    is "the first": sample 0, first pixel (a row's channel 0)."""
    cnt = z.numel()
    z = z.double()
    fam = family(regime)
    num = lambda: float(regime.rsplit('_', 1)[1])
    if fam == 'plain':
        return 3.0 + 1.7 * z
    if fam == 'offset':
        return OFFSET_R[dtype_name] + z
    if fam == 'first_zero':
        v = num() + z
        v[0] = 0.0
        return v
    if fam == 'first_outlier':
        v = z.clone()
        v[0] = num()
        return v
    if fam == 'constant_first_zero':
        v = torch.full_like(z, -2.5)
        v[0] = 0.0
        return v
    if fam == 'constant':
        return torch.full_like(z, num())
    if fam == 'near_constant':
        return NEAR_CONSTANT_C * (1.0 + 1e-3 * z)
    if fam in ('sparse', 'bimodal'):       # exact zeros but for a seeded subset that never holds the first element
        share, mu, sd = (0.001, 5.0, 3.0) if fam == 'sparse' else (0.3, 5.0, 0.05)
        k = min(cnt - 1, max(2, int(round(share * cnt))))
        at = torch.randperm(cnt - 1, generator=gen)[:k] + 1
        v = torch.zeros_like(z)
        v[at] = mu + sd * z[at]
        return v
    if fam == 'tiny':
        return 1e-4 * z
    raise KeyError(regime)


def _seed(layout, shape):
    return 5100 + 7 * sum(shape) + (layout == 'nhwc')


@functools.lru_cache(maxsize=None)
def bn_case(layout, shape, dtype_name, all_plain=False):
    """-> dict of CPU tensors, logical (n, c, h, w) and dense NCHW (the GPU test moves x, g and res into the layout): 'x', 'g',
    'res' in the storage type; 'gamma', 'beta', 'running_mean', 'running_var' float32; 'x_ideal' float64 (before rounding);
    'regimes' (the name per channel).  `all_plain`: the same noise with `plain` in every channel -- its x, g and res agree with
    the mixed tensor's bit for bit in the channels that are `plain` there."""
    n, c, h, w = shape
    dt = DTYPES[dtype_name]
    gen = torch.Generator().manual_seed(_seed(layout, shape))
    z = torch.randn(n, c, h, w, generator=gen)
    zg = torch.randn(n, c, h, w, generator=gen)
    res = torch.randn(n, c, h, w, generator=gen).to(dt)
    gamma = torch.rand(c, generator=gen) + 0.5
    gamma[GAMMA_ZERO_AT], gamma[GAMMA_NEGATIVE_AT] = 0.0, -0.8
    beta = torch.randn(c, generator=gen)
    rm, rv = torch.randn(c, generator=gen), torch.rand(c, generator=gen) + 0.5
    regimes = ['plain'] * c if all_plain else channel_regimes(c, dtype_name)
    ideal = torch.empty(n, c, h, w, dtype=torch.float64)
    for ch, r in enumerate(regimes):
        rgen = torch.Generator().manual_seed(_seed(layout, shape) + 31 * ch + 1)
        ideal[:, ch] = regime_values(r, z[:, ch].reshape(-1), rgen, dtype_name).view(n, h, w)
    x = ideal.to(dt)
    # g = 0.5 xhat + z': correlated with x, so that c1 of gx = c0 g + c1 x + c2 is of order rstd (an uncorrelated g leaves it ~ 0
    # and the backward's cancellation would never show)
    xd = x.double()
    mean = xd.mean((0, 2, 3), keepdim=True)
    var = ((xd - mean) ** 2).mean((0, 2, 3), keepdim=True)
    g = (0.5 * (xd - mean) / torch.sqrt(var + EPS) + zg.double()).to(dt)
    return dict(x=x, g=g, res=res, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, x_ideal=ideal, regimes=regimes)


def channel_err(t, t64):
    """max |t - t64| / max(1, max |t64|) per channel of (n, c, h, w) tensors -> (c,) float64."""
    t, t64 = t.detach().double().cpu(), t64.double()
    return (t - t64).abs().amax((0, 2, 3)) / t64.abs().amax((0, 2, 3)).clamp(min=1.0)


@functools.lru_cache(maxsize=None)
def bn_stats64(layout, shape, dtype_name, all_plain=False):
    """-> mean, biased var, rstd (c,) and xhat (n, c, h, w) of the stored x, float64."""
    x = bn_case(layout, shape, dtype_name, all_plain)['x'].double()
    mean = x.mean((0, 2, 3))
    xc = x - mean.view(1, -1, 1, 1)
    var = (xc * xc).mean((0, 2, 3))
    rstd = 1.0 / torch.sqrt(var + EPS)
    return mean, var, rstd, xc * rstd.view(1, -1, 1, 1)


def bn_reference(layout, shape, dtype_name, mode='plain', mask=None, all_plain=False):
    """Training BatchNorm written out in float64 -> dict: 'pre' (the normalised, scaled and shifted x, plus the residual in mode
    'add'), 'y', 'gx', 'gres' (mode 'add'), 'dgamma', 'dbeta', 'mean', 'var'.  Modes 'relu' and 'add' put max(0, .) behind it;
    `mask` (bool, where the output is positive) replaces the reference's own sign decision -- the caller passes the operator's
    where the pre-activation is within rounding of zero."""
    v = bn_case(layout, shape, dtype_name, all_plain)
    n, c, h, w = shape
    cnt = n * h * w
    mean, var, rstd, xhat = bn_stats64(layout, shape, dtype_name, all_plain)
    col = lambda t: t.double().view(1, -1, 1, 1)
    pre = xhat * col(v['gamma']) + col(v['beta'])
    if mode == 'add':
        pre = pre + v['res'].double()
    g = v['g'].double()
    if mode == 'plain':
        y = pre
    else:
        mask = pre > 0 if mask is None else mask.cpu()
        y, g = pre * mask, g * mask
    dbeta, dgamma = g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))
    gx = col(v['gamma']) * col(rstd) * (g - col(dbeta) / cnt - xhat * col(dgamma) / cnt)
    return dict(pre=pre, y=y, gx=gx, gres=g if mode == 'add' else None, dgamma=dgamma, dbeta=dbeta, mean=mean, var=var, cnt=cnt)


def running64(rm, rv, mean, var, cnt, factor):
    """The running statistics after one step (the variance enters unbiased), float64."""
    unbiased = var * (cnt / (cnt - 1.0) if cnt > 1 else 1.0)
    return (1.0 - factor) * rm.double() + factor * mean, (1.0 - factor) * rv.double() + factor * unbiased


def bn_mirror(x, g, res, gamma, beta, rm, rv, factor, mode, mask):
    """The float32 torch formulation, on the device the tensors live on: F.batch_norm on the widened stored values and autograd.
    -> dict like bn_reference's (float32), plus 'running_mean' / 'running_var' (updated copies)."""
    import torch.nn.functional as F
    x = x.detach().float().requires_grad_()
    res = res.detach().float().requires_grad_() if mode == 'add' else None
    gamma, beta = gamma.detach().clone().requires_grad_(), beta.detach().clone().requires_grad_()
    rm, rv = rm.clone(), rv.clone()
    pre = F.batch_norm(x, rm, rv, gamma, beta, True, factor, EPS)
    if mode == 'add':
        pre = pre + res
    y = pre if mode == 'plain' else pre * mask
    y.backward(g.float())
    return dict(y=y.detach(), gx=x.grad, gres=res.grad if res is not None else None, dgamma=gamma.grad, dbeta=beta.grad,
                running_mean=rm, running_var=rv)


# --------------------------------------------------------------------------- the summation model of the one-pass kernel

def model_nchw_error(x, first_value_shift=True, centred=False, blocks=4, threads=256, vec=4):
    """A NumPy model of the NCHW forward on ONE channel x (n, hw) float32 -> error of y / max(1, |y|max) against float64, with
    gamma = 1, beta = 0.  Per plane `blocks` workgroups of `threads` threads; a thread adds its vectors' (x - shift) and
    (x - shift)^2 in float32 in the order the kernel visits them, a workgroup adds its threads in a tree, the finalize is double.
    first_value_shift: shift = x[0, 0] (the kernel before the fix), else the median of x[0, 0], x[0, hw / 2], x[0, hw - 1];
    centred: y = (x - mean) * scale + beta instead of x * scale + (beta - mean * scale)."""
    import numpy as np
    x = np.asarray(x, np.float32)
    n, hw = x.shape
    shift = x[0, 0] if first_value_shift else np.float32(np.median([x[0, 0], x[0, hw // 2], x[0, hw - 1]]))
    nvec = hw // vec
    per = -(-nvec // blocks)
    s1 = s2 = 0.0
    for plane in range(n):
        for b in range(blocks):
            lo, hi = b * per, min(nvec, (b + 1) * per)
            steps = -(-(hi - lo) // threads)
            d = np.zeros((steps * threads, vec), np.float32)
            d[:hi - lo] = (x[plane, lo * vec:hi * vec] - shift).reshape(-1, vec)
            d = d.reshape(steps, threads, vec).transpose(1, 0, 2).reshape(threads, steps * vec)      # a thread's elements in its order
            a1 = np.add.accumulate(d, axis=1, dtype=np.float32)[:, -1]
            a2 = np.add.accumulate((d.astype(np.float64) ** 2).astype(np.float32), axis=1, dtype=np.float32)[:, -1]
            while a1.size > 1:
                a1, a2 = a1[0::2] + a1[1::2], a2[0::2] + a2[1::2]
            s1, s2 = s1 + float(a1[0]), s2 + float(a2[0])
    cnt = float(n * hw)
    m = s1 / cnt
    var, mean = max(s2 / cnt - m * m, 0.0), float(shift) + m
    rstd = 1.0 / np.sqrt(var + EPS)
    x64 = x.astype(np.float64)
    if centred:
        y = ((x - np.float32(mean)).astype(np.float64) * float(np.float32(rstd))).astype(np.float32)
    else:
        y = (x64 * float(np.float32(rstd)) + float(np.float32(-mean * rstd))).astype(np.float32)
    mean64 = x64.mean()
    y64 = (x64 - mean64) / np.sqrt(((x64 - mean64) ** 2).mean() + EPS)
    return float(np.abs(y - y64).max() / max(1.0, np.abs(y64).max()))


# The rows of the issue's table: name -> (channel from z (n, hw) float64, modelled error of today's kernel)
MODEL_ROWS = {
    'plain': (lambda z: 3 + 1.7 * z, 9e-8),
    'offset_1000': (lambda z: 1000 + z, 1.2e-5),
    'first_zero_30': (lambda z: _first(30 + z, 0.0), 1.2e-5),
    'first_zero_100': (lambda z: _first(100 + z, 0.0), 1.2e-4),
    'first_outlier_100': (lambda z: _first(z, 100.0), 7e-5),
    'first_outlier_1000': (lambda z: _first(z, 1000.0), 8e-4),
    'constant_100.3': (lambda z: 100.3 + 0 * z, 1.9e-3),
    'constant_100.3_first_zero': (lambda z: _first(100.3 + 0 * z, 0.0), 9e-3),
}


def _first(v, value):
    v = v.clone()
    v.view(-1)[0] = value
    return v


@functools.lru_cache(maxsize=None)
def model_channel(name):
    z = torch.randn(2, 200 * 200, generator=torch.Generator().manual_seed(77), dtype=torch.float64)
    return MODEL_ROWS[name][0](z).float().numpy()


# --------------------------------------------------------------------------- B. LayerNorm rows

# The row regimes: BatchNorm's list with channel 0 of the row as "the first" element (the offset row goes up to the storage type's
# OFFSET_R), `one_massive_channel` (z with one channel at 1e3: the residual-stream pattern of trained transformers), and rows at
# +-6e4 -- what a float16 producer hands over: their squares overflow the half type but not the float32 the kernel must square
# in.  The operators take no float16 x; the rows ride in the 'f32_f16' precision (float32 x, float16 result and gradient).
# Each regime fills ROWS_PER_REGIME consecutive rows, over and over until the operator's rows are filled.
LN_REGIMES = tuple(PERIOD) + ('one_massive_channel',)
LN_F16_EXTRA = ('large_6e4', 'large_-6e4')
LN_STORE = {'f32': 'f32', 'f32_f16': 'f32', 'bf16': 'bf16'}        # precision -> the type x is stored in
ROWS_PER_REGIME = 2
LN_BAR = 1e-4                      # the layer bar of test_gpu_swin_glue.py / _seam.py / _ffn*.py
LN_UNIT = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}     # one more rounding of a half result
FFN_MARGIN = 1.5                   # of test_gpu_swin_ffn*.py: a half GEMM precision is held to 1.5 x the parent's own error


def ln_regimes(prec):
    """The row regimes a precision runs."""
    regs = tuple(r for r in LN_REGIMES if r not in ABSENT[LN_STORE[prec]])
    return regs + (LN_F16_EXTRA if prec == 'f32_f16' else ())


def ln_row_values(regime, z, gen, store_name):
    if regime == 'one_massive_channel':
        v = z.double().clone()
        v[z.numel() // 3] = 1e3
        return v
    if regime.startswith('large_'):
        return float(regime.split('_')[1]) + 8.0 * z.double()
    return regime_values(regime, z, gen, store_name)


@functools.lru_cache(maxsize=None)
def ln_rows(rows, C, prec, seed):
    """-> x (rows, C) float64 before rounding, and the regime name of every row."""
    gen = torch.Generator().manual_seed(6100 + seed)
    z = torch.randn(rows, C, generator=gen)
    regs = ln_regimes(prec)
    names = tuple(regs[(i // ROWS_PER_REGIME) % len(regs)] for i in range(rows))
    x = torch.stack([ln_row_values(names[i], z[i], torch.Generator().manual_seed(6100 + seed + 13 * i + 1), LN_STORE[prec])
                     for i in range(rows)])
    return x, names


def _noise(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(6900 + seed), dtype=torch.float64)


def group_err(t, t64, names):
    """max |t - t64| / max(1, max |t64|) over the rows of each regime.  t, t64: (..., C) with as many rows as names; a name of None
    (a row of window padding) is left out.  -> {regime: error}"""
    C = t64.shape[-1]
    t, t64 = t.detach().double().cpu().reshape(-1, C), t64.double().reshape(-1, C)
    assert t.shape == t64.shape and t.shape[0] == len(names)
    out = {}
    for r in dict.fromkeys(n for n in names if n is not None):
        sel = torch.tensor([n == r for n in names])
        out[r] = float((t[sel] - t64[sel]).abs().max() / max(1.0, float(t64[sel].abs().max())))
    return out


# ---- swin_glue: layer_norm_rows, plain and into windows

GLUE_CASES = ('ws12_c128', 'rows_c96')         # C = 128 into 12 x 12 windows (shifted); the identity map (the module's plain case)
GLUE_PRECISIONS = ('f32', 'bf16', 'f32_f16')


@functools.lru_cache(maxsize=None)
def glue_case(case, prec):
    """swin_glue_inputs' case with the row regimes as x and dy = 0.5 xhat + z' -> dict: x, dy, gamma, beta as the operator is
    handed them; names_in / names_out per row of x / of the result (None: window padding); Y, DX, DG, DB float64 from the
    module's own twin (ln_rows64 + autograd) on the stored values."""
    import swin_glue_inputs as SG
    B, H, W, ws, sh, C = SG.CASES[case]
    tokens = H * W if ws else H
    xdt, odt = SG.PRECISIONS[prec]
    v = SG.inputs(case, prec)
    ideal, names = ln_rows(B * tokens, C, prec, seed=list(SG.CASES).index(case))
    x = ideal.view(B, tokens, C).to(xdt)
    one, zero = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    xhat = SG.ln_rows64(x.double(), one, zero, case)
    dy = (0.5 * xhat + _noise(xhat.shape, 1)).to(odt)
    ids = torch.arange(1, B * tokens + 1, dtype=torch.float64).view(B, tokens, 1)
    out_ids = SG.partition64(ids, H, W, ws, sh) if ws else ids
    names_out = tuple(None if i == 0 else names[int(i) - 1] for i in out_ids.reshape(-1).tolist())
    xl, gl, bl = (t.double().requires_grad_() for t in (x, v['gamma'], v['beta']))
    Y = SG.ln_rows64(xl, gl, bl, case)
    DX, DG, DB = torch.autograd.grad(Y, (xl, gl, bl), dy.double())
    return dict(x=x, dy=dy, gamma=v['gamma'], beta=v['beta'], names_in=names, names_out=names_out, ideal=ideal, Y=Y.detach(), DX=DX,
                DG=DG, DB=DB)


# ---- swin_seam: patch_merge_norm (the norm over 4C), patch_embed_norm

# (kind, case of swin_seam_inputs, batch): the batch is this module's, so that every operator gets 33 rows or more
SEAM_CASES = (('merge', 'even_c96', 3), ('merge', 'odd_h_c128', 2), ('embed', 'two_images_c128', 1))
SEAM_PRECISIONS = ('f32', 'bf16', 'f32_f16')


def merge_gather(t, H, W):
    """(B, H W, C) -> (B, ceil(H / 2) ceil(W / 2), 4 C): the rearrangement of PatchMerging (zero padding to even sides; element
    c * 4 + 2 i + j of a result row is channel c of the token at offset (i, j) of its 2 x 2 block), without the norm."""
    B, L, C = t.shape
    t = torch.nn.functional.pad(t.view(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
    Hp, Wp = t.shape[1] // 2, t.shape[2] // 2
    return t.reshape(B, Hp, 2, Wp, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, Hp * Wp, 4 * C)


def seam_rows(kind, t, case):
    """A tensor of x's shape as the (B, rows, normalised length) rows the operator normalises."""
    import swin_seam_inputs as SS
    if kind == 'merge':
        _, H, W, _ = SS.MERGE_CASES[case]
        return merge_gather(t, H, W)
    return t.flatten(2).transpose(1, 2)


@functools.lru_cache(maxsize=None)
def seam_case(kind, case, batch, prec):
    """swin_seam_inputs' case (its gamma, beta, H, W, C; `batch` images) with the row regimes in the rows the operator normalises
    -> dict like glue_case's; x in the operator's own shape ((B, H W, C) tokens / (B, C, H, W) maps).  A merged row at an odd edge
    keeps zeros where its block lies in the padding."""
    import swin_seam_inputs as SS
    xdt, odt = SS.precisions(kind)[prec]
    v = SS.inputs(kind, case, prec)
    n = SS.norm_len(kind, case)
    seed = 50 + list(SS.CASES[kind]).index(case) + 10 * (kind == 'embed')
    if kind == 'merge':
        _, H, W, C = SS.MERGE_CASES[case]
        shape = (batch, H * W, C)
    else:
        _, C, H, W = SS.EMBED_CASES[case]
        shape = (batch, C, H, W)
    where = seam_rows(kind, torch.arange(1, batch * H * W * C + 1, dtype=torch.float64).view(shape), case)      # 0: padding
    rows = where.shape[0] * where.shape[1]
    ideal, names = ln_rows(rows, n, prec, seed)
    flat = torch.zeros(batch * H * W * C + 1, dtype=torch.float64)
    flat[where.reshape(-1).long()] = ideal.reshape(-1)
    x = flat[1:].view(shape).to(xdt)
    one, zero = torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    xhat = SS.call64(kind, case, x.double(), one, zero)
    dy = (0.5 * xhat + _noise(xhat.shape, seed)).to(odt)
    xl, gl, bl = (t.double().requires_grad_() for t in (x, v['gamma'], v['beta']))
    Y = SS.call64(kind, case, xl, gl, bl)
    DX, DG, DB = torch.autograd.grad(Y, (xl, gl, bl), dy.double())
    return dict(x=x, dy=dy, gamma=v['gamma'], beta=v['beta'], names_in=names, names_out=names, ideal=ideal, Y=Y.detach(), DX=DX, DG=DG, DB=DB)


# ---- the four Swin FFN families: LayerNorm -> MLP -> residual

FFN_ROWS = 40
# (family, input module, case whose weights are used)
FFN_CASES = (('infer', 'swin_ffn_inputs', 'r33_c128_ln'), ('infer_wide', 'swin_ffn_wide_inputs', 'r33_c512_ln'),
             ('train', 'swin_ffn_train_inputs', 'r33_c128'), ('train_wide', 'swin_ffn_train_wide_inputs', 'r33_c512'))
FFN_PRECISIONS = ('f32', 'bf16')
FFN_TENSORS = ('out', 'dx', 'dgamma', 'dbeta', 'dw1', 'db1', 'dw2', 'db2')


@functools.lru_cache(maxsize=None)
def ffn_case(family, prec):
    """The input module's case with FFN_ROWS rows of the row regimes as x (and, in training, dout = 0.5 xhat + z') -> dict:
    'v' the operator's tensors (every weight the module's own), 'names', 'ref' {tensor: float64} from the module's twin
    (ffn64 / formulation + autograd with scale_name = 'none'), 'module'."""
    import importlib
    modname, case = {f: (m, c) for f, m, c in FFN_CASES}[family]
    M = importlib.import_module(modname)
    xdt, mdt = M.PRECISIONS[prec]
    v = dict(M.inputs(case, prec))
    C = v['w1'].shape[1]
    ideal, names = ln_rows(FFN_ROWS, C, prec, seed=90 + [f for f, _, _ in FFN_CASES].index(family))
    v['x'] = ideal.to(xdt)
    if family.startswith('train'):
        xd = v['x'].double()
        xhat = torch.nn.functional.layer_norm(xd, (C,), None, None, EPS)
        v['dout'] = (0.5 * xhat + _noise(xd.shape, 7)).to(xdt)
        leaves = {k: v[k].double().requires_grad_() for k in ('x',) + M.PARAMS}
        out = M.formulation(leaves['x'], *(leaves[k] for k in M.PARAMS), None)
        out.backward(v['dout'].double())
        ref = M._collect(out, leaves)
    else:
        ref = {'out': M.ffn64(v['x'], v['gamma'], v['beta'], v['w1'], v['b1'], v['w2'], v['b2'])}
    return dict(v=v, names=names, ideal=ideal, ref=ref, module=M, xdt=xdt, mdt=mdt)
