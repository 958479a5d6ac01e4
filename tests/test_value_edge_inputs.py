"""Conditions on the inputs of test_gpu_value_edges.py (value_edge_inputs.py), checked on the CPU: every regime reaches the
branch it was built for, no ratio of the occupancy losses sits where float32 and float64 may legitimately part, and the float32
torch formulations agree with the float64 references -- their error per regime is printed; it is the "reference alone" error
that decides the bound of a kernel wherever float32 itself cannot meet the operator's bar."""
import numpy as np
import pytest
import torch

import value_edge_inputs as V


# --------------------------------------------------------------------------- A. occupancy losses

def _ratios(regime):
    return torch.cat([V.occ_reference(r, m)['ratios'] for r, m in V.OCC_CASES if r == regime])


def test_occupancy_regimes_reach_their_branches():
    sat, conf, wrong = _ratios('saturated'), _ratios('confident'), _ratios('confidently_wrong')
    assert int((sat >= 1 - 1e-5).sum()) >= 1 and int((wrong < 1e-5).sum()) >= 1
    # 8 * onehot + randn gives p_t ~ 0.98: the ratios of `confident` approach the clamp (it is `saturated` that reaches it)
    assert float(conf.max()) > 0.97 and int((conf >= 1 - 1e-5).sum()) == 0
    # x == 1.0 in float32 (two steps of inverse_sigmoid) and x in [1 - 1e-5, 1) (one step) both occur
    down = V.inverse_sigmoid_steps(sat)[0]
    assert int((down == 2).sum()) >= 1 and int((down == 1).sum()) >= 1
    even = V.occ_reference('saturated_even', 4097)['ratios']
    assert len(even) == 6 and bool((V.inverse_sigmoid_steps(even)[0] == 2).all())      # sem and geo each 3 x -log(1 - 2e-5)
    assert all(abs(float(l) - 3 * -np.log(1 - 2e-5)) < 1e-7 for l in V.occ_reference('saturated_even', 4097)['losses'][1:])
    for m in V.OCC_SIZES:
        z, t, cam = V.occ_case('underflow', m)
        valid = cam & (t != V.IGNORE)
        p32 = torch.softmax(z, 1)[valid]
        assert float(p32[:, V.UNDERFLOW_CLASS].sum()) == 0.0                       # P_i == 0 in float32 ...
        assert float(V.occ_reference('underflow', m)['P'][V.UNDERFLOW_CLASS]) > 0   # ... and not in float64
        if m > 1:
            assert int((t[valid] == V.UNDERFLOW_CLASS).sum()) >= 2                  # with T_i > 0: the `P_i > 0` test decides
    for m in V.OCC_SIZES:
        z, t, cam = V.occ_case('neg_inf', m)
        assert bool(torch.isinf(z[:, V.NEG_INF_CLASS]).all()) and int((t == V.NEG_INF_CLASS).sum()) == 0
        z, t, cam = V.occ_case('one_valid_voxel', m)
        assert int((cam & (t != V.IGNORE)).sum()) == 1
        z, t, cam = V.occ_case('empty_mask', m)
        assert int(cam.sum()) == 0
        z, t, cam = V.occ_case('all_ignored', m)
        assert bool((t == V.IGNORE).all()) and (m == 1 or int(cam.sum()) > 0)
        z, t, cam = V.occ_case('absent_classes', m)
        assert all(int((t == c).sum()) == 0 for c in V.ABSENT)
        z, t, cam = V.occ_case('huge', 4097)
        assert float(z.abs().max()) > 3e4
    assert float(V.occ_reference('huge', 4097)['losses'][0]) > 1e4                  # CE ~ 1.8e4


@pytest.mark.parametrize('regime,m', V.OCC_CASES)
def test_no_occupancy_ratio_sits_on_a_threshold(regime, m):
    """Within 1e-6 of 1e-5 or 1 - 1e-5 float32 and float64 may take different branches of inverse_sigmoid, and within a float32
    rounding of 1 - 2^-25 (x rounds to 1.0 above it: two steps, below it: one) a different number of steps.  No ratio of any
    case lies there; the second band is 5e-9 wide, many times the error of a ratio of double-precision totals."""
    r = V.occ_reference(regime, m)['ratios']
    assert float((r - 1e-5).abs().min()) > 1e-6 and float((r - (1 - 1e-5)).abs().min()) > 1e-6
    assert not bool(((r - (1 - 2.0 ** -25)).abs() < 5e-9).any())
    assert bool(((r >= 0) & (r <= 1)).all())


@pytest.mark.parametrize('regime,m', V.OCC_CASES)
def test_float32_mirrors_agree_with_the_float64_losses(regime, m):
    """dhd_amd.detector's CrossEntropyLoss / sem_scal / geo_scal in float32 against the float64 twin written from the reference
    formulas, and the twin against the numpy oracle where that is defined.  The one regime in which float32 cannot follow
    float64 is `underflow`: P_i = 0 in float32 skips the precision term of class i, 1e-87 n in float64 does not and adds
    -log(1e-5) / #classes to sem scal (the reference, in float32, skips it)."""
    from oracle import mghs_oracle as O
    ref = V.occ_reference(regime, m)
    z, t, cam = V.occ_case(regime, m)
    print(f'{regime} m={m}: float64 losses {[float(x) for x in ref["losses"]]}, float32 mirror error '
          f'{[float(e) for e in ref["loss_err"]]} (bounds {ref["loss_bound"]}), gradient |G|max {float(ref["grad"].abs().max()):.3g} '
          f'mirror error {ref["grad_err"]:.3g} (bound {ref["grad_bound"]:.3g})')
    nan = torch.isnan(ref['losses'])
    assert torch.equal(nan, torch.isnan(ref['mirror_losses']))
    if regime in ('empty_mask', 'all_ignored'):
        assert nan.tolist() == [True, True, False]
        assert abs(float(ref['losses'][2]) - 3 * -np.log(1e-5)) < 1e-6            # (NaN, NaN, 34.5388)
    else:
        assert not bool(nan.any())
    for i in range(3):
        if nan[i] or (regime == 'underflow' and i == 1 and m > 1):
            continue
        assert float(ref['loss_err'][i]) <= 2e-5 * max(1.0, abs(float(ref['losses'][i]))), (i, ref['loss_err'])
    if regime == 'underflow' and m > 1:
        n_present = int((torch.bincount(t[cam & (t != V.IGNORE)].long(), minlength=256)[:17] > 0).sum())
        assert abs(float(ref['loss_err'][1]) - -np.log(1e-5) / n_present) < 1e-4
    assert ref['grad_err'] <= 1e-4 * float(ref['grad'].abs().max()) + 1e-9
    assert bool(torch.isfinite(ref['grad']).all()) and bool(torch.isfinite(ref['mirror_grad']).all())
    if not bool(nan.any()) and regime != 'huge':                                     # the oracle takes log(p): inf at p = 0
        o = O.occ_losses(z.numpy(), t.numpy(), cam.numpy(), V.class_weights().numpy())
        assert max(abs(float(a) - float(b)) for a, b in zip(o, ref['losses'])) < 1e-6


# --------------------------------------------------------------------------- B. bin labels

@pytest.mark.parametrize('name', list(V.LABEL_CASES))
def test_bin_label_placements_straddle_every_boundary(name):
    c, (dref, href) = V.label_case(name), V.label_reference(name)
    neck = V.label_neck(name)
    for ref, k_of, n_bins, zero_boundary in ((dref, c['d_k'], neck.D, None), (href, c['h_k'], neck.H, 10)):
        for k in range(1, n_bins + 2):
            got = set(ref[torch.from_numpy(k_of == k)].tolist())
            below, above = k - 1, (k if k <= n_bins else 0)                          # g == n_bins + 1: "no label"
            if zero_boundary == k:
                # the boundary value is 0.0 (height bin 10 starts at -1 + 10 * 0.1): a 0 in the map means "no point", and its
                # float32 neighbours are denormals that vanish in v - offset, so nothing can be placed below this boundary
                assert got == {0, above}, (name, k, got)
                continue
            assert {below, above} <= got, (name, k, got)
        got = set(ref[torch.from_numpy(k_of == 0)].tolist())                         # below the first bin and in it: both "no label"
        assert got == {0}
    assert int(c['d_k'].max()) == neck.D + 1 and int(c['h_k'].max()) == neck.H + 1
    neg, zero, big = (int(w) for w in c['special'])
    assert [int(dref[w]) for w in (neg, zero, big)] == [0, 0, 0] and [int(href[w]) for w in (neg, zero, big)] == [0, 0, 0]
    n_cam, fh, fw = V.LABEL_FEATURE_MAP
    ds = V.LABEL_CASES[name][1]
    win = lambda a, w: a[0, w // (fh * fw), ((w // fw) % fh) * ds:((w // fw) % fh + 1) * ds, (w % fw) * ds:(w % fw + 1) * ds]
    assert float(win(c['gt_depth'], neg).min()) < 0 and int((win(c['gt_depth'], neg) != 0).sum()) == 1
    assert int((win(c['gt_depth'], zero) != 0).sum()) == 0 and float(win(c['gt_depth'], big).max()) == 1e5
    assert int((dref > 0).sum()) > 1000 and int((href > 0).sum()) > 1000


# --------------------------------------------------------------------------- C. bin BCE

def test_bin_bce_inputs_reach_the_clamps():
    zeros = ones = hundreds = 0
    for kind, c in V.BCE_CASES:
        pred, bins, fg = V.bce_case(kind, c)
        ref = V.bce_reference(kind, c)
        p_fg = pred.permute(0, 2, 3, 1).reshape(-1, c)[fg > 0]
        zeros += int((p_fg == 0).sum())
        ones += int((p_fg == 1).sum())
        hundreds += int((ref['terms'] == 100.0).sum())
        assert bool(((pred >= 0) & (pred <= 1)).all())
        print(f'{kind} C={c}: loss {ref["loss"]:.6g} float32 formula error {ref["loss_err"]:.3g} (bound {ref["loss_bound"]:.3g}), '
              f'|G|max {float(ref["grad"].abs().max()):.3g} error {ref["grad_err"]:.3g} (bound {ref["grad_bound"]:.3g})')
        assert ref['loss_err'] <= 1e-5 * max(1.0, abs(ref['loss'])) and np.isfinite(ref['loss'])
    assert zeros >= 10 and ones >= 10 and hundreds >= 1
    for c in V.BCE_CHANNELS:
        assert int((V.bce_case('no_foreground', c)[2] > 0).sum()) == 0 and int((V.bce_case('one_foreground', c)[2] > 0).sum()) == 1
        assert float(V.bce_reference('zeros_ones', c)['grad'].abs().max()) >= 1e11            # (p - y) / 1e-12 at p = 0, y = 1
        assert float(V.bce_case('tiny', c)[0].min()) == np.float32(1e-30)
        assert float(V.bce_case('near_one', c)[0].max()) == 1.0 - 2.0 ** -24
    pred, bins, fg = V.bce_case('stride', 3)
    assert pred[:, 0].numel() == 66156 > V.BCE_GRID_STRIDE
    assert int((fg[V.BCE_GRID_STRIDE:] > 0).sum()) >= 3 and 0.01 < float((fg > 0).float().mean()) < 0.03


# --------------------------------------------------------------------------- D, E. head and argmax rows

@pytest.mark.parametrize('dtype_name', list(V.HEAD_DTYPES))
@pytest.mark.parametrize('shape', list(V.HEAD_SHAPES))
def test_head_inputs_hold_their_edges(shape, dtype_name):
    dt = V.HEAD_DTYPES[dtype_name]
    big = torch.finfo(dt).max
    bn, d, c, hb, extra, fh, fw = V.HEAD_SHAPES[shape]
    x_d, hl = V.head_case('largest', shape, dtype_name)[:2]
    assert x_d.dtype == dt and float(x_d[:, :d].float().max()) == big and float(x_d[:, :d].float().min()) == -big
    ref = V.head_reference('largest', shape, dtype_name)
    assert bool(torch.isfinite(ref['depth']).all()) and int((ref['depth'] == 0.5).sum()) >= 2 and int((ref['depth'] == 1).sum()) >= 1
    ref = V.head_reference('neg_inf', shape, dtype_name)
    assert bool(torch.isfinite(ref['depth']).all()) and bool((ref['depth'][:, d // 2] == 0).all())
    ref = V.head_reference('two_maxima', shape, dtype_name)
    assert bool((ref['height'].max(1).values == 0.5).all()) and bool((ref['height'].sum(1) - 1).abs().max() < 1e-12)
    assert bool(ref['band_clear'].all())
    ref = V.head_reference('all_equal', shape, dtype_name)
    assert bool((ref['height'] == 1.0 / hb).all()) and bool(ref['band_clear'].all())
    ref = V.head_reference('nan_rows', shape, dtype_name)
    nan_d = torch.isnan(ref['depth']).any(1)
    assert int(nan_d.sum()) == 3 and bool(torch.isnan(ref['depth']).all(1).eq(nan_d).all())
    # torch's own softmax agrees on which rows are NaN
    assert torch.equal(torch.isnan(torch.softmax(V.head_case('nan_rows', shape, dtype_name)[0][:, :d].float(), 1)), torch.isnan(ref['depth']))


def test_argmax_rows():
    z, t, cam = V.argmax_case()
    pred, hist = V.argmax_reference(z, t, cam)
    assert tuple(pred[:8]) == V.ARGMAX_EXPECTED and tuple(pred[9:17]) == V.ARGMAX_EXPECTED
    assert hist.sum() == int((cam & (t != V.IGNORE)).sum()) and z.shape[0] > 2 * 256
    b2 = V.argmax_head_bias().view(16, V.N_CLS)
    assert tuple(np.argmax(b2.double().numpy(), 1)) == V.ARGMAX_EXPECTED * 2
