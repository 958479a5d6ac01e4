"""Conditions on the inputs of test_gpu_norm_edges.py (norm_edge_inputs.py), checked on the CPU: after rounding to the storage
type every regime is still what its name says, the table of regimes a storage type cannot hold is exactly the set that fails that
check, the float64 references alone stay inside what the GPU test assumes, and a NumPy model of the one-pass shifted sums shows
why the regimes exist."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_edge_inputs as N


def _ratio(v):
    v = v.double()
    return float(v.mean().abs() / v.std(unbiased=False).clamp(min=1e-300))


def _holds(regime, stored, ideal):
    """Does the stored channel / row keep the regime?  At least 16 distinct values -- or a quarter of what was drawn, where fewer than
    64 elements carry noise (a 4 x 4 plane, the non-zero share of a sparse map) -- and |mean| / std within a factor 2 of the
    unrounded channel's."""
    fam = N.family(regime)
    if fam in ('constant', 'constant_first_zero'):
        return True
    drawn = int((ideal != 0).sum()) if fam in ('sparse', 'bimodal') else ideal.numel()
    if len(torch.unique(stored)) < min(N.MIN_DISTINCT, drawn // 4):
        return False
    want, got = _ratio(ideal), _ratio(stored)
    return abs(got - want) < 0.05 if want < 0.1 else want / 2 <= got <= 2 * want


def _fresh_channel(regime, cnt, dt, seed):
    gen = torch.Generator().manual_seed(seed)
    ideal = N.regime_values(regime, torch.randn(cnt, generator=gen), gen, dt)
    return ideal.to(N.DTYPES[dt]), ideal


@pytest.mark.parametrize('dt', list(N.DTYPES))
def test_absent_table_is_exactly_what_the_storage_type_cannot_hold(dt):
    """Every regime of the period, at every BatchNorm channel size and LayerNorm row length: the ones that lose their 16 distinct
    values or their |mean| / std in the type are the ones the table names -- no more (nothing is dropped silently) and no fewer."""
    sizes = sorted({s[0] * s[2] * s[3] for shapes in N.BN_SHAPES.values() for s in shapes} | {96, 128, 384, 512})
    failing = set()
    for regime in N.PERIOD:
        for cnt in sizes:
            stored, ideal = _fresh_channel(regime, cnt, dt, 40 + cnt)
            if not _holds(regime, stored, ideal):
                failing.add(regime)
    print(dt, 'cannot hold', sorted(failing), '| table', N.ABSENT[dt])
    assert failing == set(N.ABSENT[dt])
    gone = set(N.FAMILIES) - {N.family(r) for r in N.channel_regimes(len(N.PERIOD), dt)}
    assert len(gone) <= {'f32': 0, 'f16': 1, 'bf16': 2}[dt], gone
    print(dt, 'channels run', N.channel_regimes(len(N.PERIOD), dt))
    for prec, store in N.LN_STORE.items():
        if store == dt:
            print(prec, 'rows run', N.ln_regimes(prec))


@pytest.mark.parametrize('layout,shape,dt', N.BN_CASES)
def test_batchnorm_channels_are_what_their_names_say(layout, shape, dt):
    v = N.bn_case(layout, shape, dt)
    x, regimes = v['x'], v['regimes']
    n, c, h, w = shape
    mean, var, rstd, xhat = N.bn_stats64(layout, shape, dt)
    assert set(regimes) == set(N.channel_regimes(len(N.PERIOD), dt)) and regimes.count('plain') >= c // 16
    for ch, r in enumerate(regimes):
        col, fam = x[:, ch].reshape(-1), N.family(r)
        assert _holds(r, col, v['x_ideal'][:, ch].reshape(-1)), (ch, r)
        first = float(col[0])
        if fam in ('first_zero', 'constant_first_zero', 'sparse', 'bimodal'):
            assert first == 0.0
        if fam == 'first_outlier':
            assert first == float(r.rsplit('_', 1)[1])
        if fam == 'offset':
            assert abs(first - N.OFFSET_R[dt]) < 5 and N.OFFSET_R[dt] / 2 < _ratio(col) < 2 * N.OFFSET_R[dt]
        if fam == 'first_zero':            # every other element sits at the offset
            assert float(col[1:].double().mean()) > 0.9 * float(r.rsplit('_', 1)[1])
        if fam == 'constant':
            assert float(var[ch]) == 0.0 and float(mean[ch]) == first and len(torch.unique(col)) == 1
        if fam == 'constant_first_zero':
            assert len(torch.unique(col[1:])) == 1 and float(col[1]) == -2.5 and 0 < float(var[ch]) < 6.25
        if fam in ('near_constant', 'tiny'):
            assert float(var[ch]) < N.EPS
        if fam == 'sparse':
            assert 2 <= int((col != 0).sum()) <= max(2, 0.002 * col.numel())
        if fam == 'bimodal':
            assert 0.25 < float((col != 0).double().mean()) < 0.35
    # around the regimes: gamma has one zero and one negative entry; g is correlated with xhat (c1 of the backward ~ rstd)
    assert int((v['gamma'] == 0).sum()) == 1 and int((v['gamma'] < 0).sum()) == 1
    if n * h * w >= 2000:                  # mean(g xhat) = 0.5 var / (var + eps) + noise of order cnt^-1/2
        corr, want = (v['g'].double() * xhat).mean((0, 2, 3)), 0.5 * var / (var + N.EPS)
        assert bool((corr > 0.8 * want - 0.05).all()), (corr, want)
        assert sum(float(q) > 0.3 for q in corr) >= c // 2
    # channel isolation has something to compare: the all-plain tensor agrees bit for bit in the plain channels
    alone = N.bn_case(layout, shape, dt, all_plain=True)
    plain = [ch for ch, r in enumerate(regimes) if r == 'plain']
    assert all(torch.equal(v[k][:, plain], alone[k][:, plain]) for k in ('x', 'g', 'res')) and set(alone['regimes']) == {'plain'}


@pytest.mark.parametrize('layout,shape,dt', [c for c in N.BN_CASES if c[2] == 'f32'])
def test_float32_mirror_on_the_cpu_is_close_to_float64(layout, shape, dt):
    """F.batch_norm in float32 on the CPU against the float64 formulas: within 4 x the bar in every regime except `near_constant`
    and `constant_100.3`, where (x - mean) rstd carries the rounding of the float32 mean, 2^-25 |c|, times rstd: the order
    2^-24 |c| rstd (1.9 x 270 and 100 x 316 -> 3e-5 and 2e-3) is the most it may be off."""
    v = N.bn_case(layout, shape, dt)
    ref = N.bn_reference(layout, shape, dt)
    mir = N.bn_mirror(v['x'], v['g'], None, v['gamma'], v['beta'], v['running_mean'], v['running_var'], 0.1, 'plain', None)
    rstd = N.bn_stats64(layout, shape, dt)[2]
    for name in ('y', 'gx'):
        err = N.channel_err(mir[name], ref[name])
        for ch, r in enumerate(v['regimes']):
            limit = 4 * N.BN_BARS[dt]
            if r in ('near_constant', 'constant_100.3'):
                limit = 2.0 ** -24 * abs(float(ref['mean'][ch])) * float(rstd[ch]) * 2 * (2 if name == 'gx' else 1)
            assert float(err[ch]) <= limit, (name, ch, r, float(err[ch]), limit)
        print(layout, shape, name, {r: f'{float(err[ch]):.2g}' for ch, r in enumerate(v['regimes'][:16])})
    rm, rv = N.running64(v['running_mean'], v['running_var'], ref['mean'], ref['var'], ref['cnt'], 0.1)
    assert torch.allclose(mir['running_mean'].double(), rm, atol=1e-5, rtol=1e-5)
    assert torch.allclose(mir['running_var'].double(), rv, atol=1e-5, rtol=1e-4)


def test_reference_formulas_are_autograd_of_float64_batch_norm():
    """The written-out float64 reference against torch's own float64 batch_norm and autograd, all three modes."""
    layout, shape, dt = 'nhwc', (2, 24, 6, 10), 'f32'
    v = N.bn_case(layout, shape, dt)
    for mode in ('plain', 'relu', 'add'):
        ref = N.bn_reference(layout, shape, dt, mode)
        x, ga, be = (v[k].double().requires_grad_() for k in ('x', 'gamma', 'beta'))
        res = v['res'].double().requires_grad_()
        pre = F.batch_norm(x, None, None, ga, be, True, 0.0, N.EPS) + (res if mode == 'add' else 0)
        y = pre if mode == 'plain' else torch.relu(pre)
        y.backward(v['g'].double())
        assert torch.allclose(ref['y'], y.detach(), atol=1e-11, rtol=0)
        live = [ch for ch, r in enumerate(v['regimes']) if N.family(r) != 'constant']       # autograd's own rounding x rstd = 316
        assert torch.allclose(ref['gx'][:, live], x.grad[:, live], atol=1e-9, rtol=1e-9)
        assert torch.allclose(ref['gx'], x.grad, atol=1e-6, rtol=0)
        assert torch.allclose(ref['dgamma'], ga.grad, atol=1e-8) and torch.allclose(ref['dbeta'], be.grad, atol=1e-10)
        if mode == 'add':
            assert torch.equal(ref['gres'], res.grad)


@pytest.mark.parametrize('name', list(N.MODEL_ROWS))
def test_summation_model_reproduces_the_orders_of_the_one_pass_kernel(name):
    """Why the regimes exist: a model of the float32 sums of (x - x_first) and (x - x_first)^2 with var = s2 / cnt - m^2 and
    y = x * scale + (beta - mean * scale) on a (2, 1, 200, 200) channel loses what the table says, to the order of magnitude;
    with the shift taken as the median of three elements and y = (x - mean) * scale + beta every row is back at the float32
    mirror's level (the constant channel: exactly beta)."""
    x = N.model_channel(name)
    want = N.MODEL_ROWS[name][1]
    one_pass = N.model_nchw_error(x)
    fixed = N.model_nchw_error(x, first_value_shift=False, centred=True)
    print(f'{name}: first-value shift, uncentred output {one_pass:.3g} (table {want:.3g}); median-of-three shift, centred output {fixed:.3g}')
    assert 0.1 * want <= one_pass <= 10 * want
    if name.startswith('constant'):
        assert fixed <= 1e-7
    else:
        assert fixed <= 2e-5


# --------------------------------------------------------------------------- B. LayerNorm rows

@pytest.mark.parametrize('prec', list(N.LN_STORE))
@pytest.mark.parametrize('C', [96, 128, 384, 512])
def test_layernorm_rows_are_what_their_names_say(prec, C):
    x, names = N.ln_rows(40, C, prec, seed=C)
    stored = x.to(N.DTYPES[N.LN_STORE[prec]])
    assert set(names) == set(N.ln_regimes(prec)) and len(names) >= 33
    assert ('large_6e4' in names) == (prec == 'f32_f16')
    for i, r in enumerate(names):
        row = stored[i]
        if r == 'one_massive_channel':
            assert float(row.abs().max()) == 1e3 == float(row[C // 3]) and float(row.double().abs().median()) < 1.5
            continue
        if r.startswith('large_'):      # finite in float16, the squares are not; float32 holds them
            assert bool(torch.isfinite(row.half()).all()) and bool(torch.isinf(row.half() * row.half()).all())
            assert bool(torch.isfinite(row.float() ** 2).all())
            continue
        assert _holds(r, row, x[i]), (i, r)
        fam = N.family(r)
        if fam in ('first_zero', 'constant_first_zero', 'sparse', 'bimodal'):
            assert float(row[0]) == 0.0
        if fam == 'first_outlier':
            assert float(row[0]) == float(r.rsplit('_', 1)[1])
        if fam == 'constant':
            assert float(row.double().var(unbiased=False)) == 0.0


def _regime_rows_are_the_ideal(d, rows):
    """The rows the operator normalises are the regimes' rows (rounded to the storage type), wherever no padding intervenes."""
    ideal = d['ideal'].to(rows.dtype).double()
    return (rows.double().reshape(ideal.shape) == ideal).all(-1)


@pytest.mark.parametrize('case', N.GLUE_CASES)
@pytest.mark.parametrize('prec', N.GLUE_PRECISIONS)
def test_glue_cases_carry_the_regimes(case, prec):
    d = N.glue_case(case, prec)
    assert bool(_regime_rows_are_the_ideal(d, d['x']).all()) and len(d['names_in']) >= 33
    assert set(n for n in d['names_out'] if n) == set(N.ln_regimes(prec)) and tuple(d['Y'].shape) == tuple(d['dy'].shape)
    const = [i for i, n in enumerate(d['names_in']) if n.startswith('constant')]
    assert bool(torch.isfinite(d['DX']).all()) and float(d['DX'].reshape(len(d['names_in']), -1)[const].abs().max()) > 100     # rstd = 316


@pytest.mark.parametrize('kind,case,batch', N.SEAM_CASES)
@pytest.mark.parametrize('prec', N.SEAM_PRECISIONS)
def test_seam_cases_carry_the_regimes(kind, case, batch, prec):
    d = N.seam_case(kind, case, batch, prec)
    rows = N.seam_rows(kind, d['x'], case)
    same = _regime_rows_are_the_ideal(d, rows)
    assert len(d['names_in']) >= 33 and d['Y'].shape[0] * d['Y'].shape[1] == len(d['names_in'])
    assert float(same.double().mean()) > (0.75 if 'odd' in case else 0.999)        # an odd side: the last block row is half padding
    assert set(d['names_in']) == set(N.ln_regimes(prec))
    # the rearrangement written out in seam_rows is the module's: normalising its rows gives the twin's result
    import swin_seam_inputs as SS
    n = rows.shape[-1]
    again = F.layer_norm(rows.double(), (n,), d['gamma'].double(), d['beta'].double(), SS.EPS)
    assert torch.equal(again, d['Y'])


@pytest.mark.parametrize('family', [f for f, _, _ in N.FFN_CASES])
@pytest.mark.parametrize('prec', N.FFN_PRECISIONS)
def test_ffn_cases_carry_the_regimes(family, prec):
    d = N.ffn_case(family, prec)
    v = d['v']
    assert bool(_regime_rows_are_the_ideal(d, v['x']).all()) and v['x'].shape[0] >= 33
    assert set(d['names']) == set(N.ln_regimes(prec)) and all(bool(torch.isfinite(t).all()) for t in d['ref'].values())
    assert v['w1'].shape == (4 * v['x'].shape[1], v['x'].shape[1]) and ('dout' in v) == family.startswith('train')
