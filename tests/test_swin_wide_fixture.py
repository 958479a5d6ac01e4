"""Fixture G20 (tests/swin_wide_inputs.py): the reference's Swin backbone at DHD-L's widths -- embed 128, heads 4 / 8 / 16 / 32,
window 12, four stages -- in float64, against this repository's port on the CPU.  G10 has head dimension 8 and widths 16 / 32 / 64;
this one has the sizes the HIP operators run at, so what tests/test_gpu_swin_composed.py holds them to is the reference's result
and not a twin written beside the kernels.

Bound.  Both sides are float64 and compute the same expression; they differ in the order of summation only (SDPA against
materialised scores, the 2 x 2 gather by reshape against nn.Unfold), so every recorded tensor is held to 1e-9 max(1, |ref|max):
the float64 rounding floor (2^-53, a few thousand terms per sum, some twenty layers) with margin.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_wide_inputs as SW  # noqa: E402
from conftest import GOLDEN  # noqa: E402

TOL = 1e-9
_cache = {}


def fixture():
    if 'g' not in _cache:
        _cache['g'] = SW.load(GOLDEN)
    return _cache['g']


def port():
    """(state keys, state SHA, record of the port's float64 run on the CPU), made once."""
    if 'port' not in _cache:
        from dhd_amd.swin import SwinTransformer
        threads = torch.get_num_threads()
        torch.set_num_threads(min(threads, 8))
        try:
            net = SwinTransformer(**SW.ARGS).eval().double()
            sha = SW.set_state(net)
            _cache['port'] = (list(net.state_dict()), sha, {k: v for k, v in net.state_dict().items() if 'relative_position_index' in k},
                              SW.record(net))
        finally:
            torch.set_num_threads(threads)
    return _cache['port']


def _compare(got, ref, what):
    """Every entry of ref that is a number array, within TOL max(1, |ref|max); -> the worst ratio error / bound."""
    worst = 0.0
    for k, r in ref.items():
        if r.dtype.kind != 'f':
            continue
        assert k in got, f'{what}: {k} missing'
        a = np.asarray(got[k])
        assert a.shape == r.shape and a.dtype == np.float64, (what, k, a.shape, r.shape)
        bound = TOL * max(1.0, float(np.abs(r).max()))
        err = float(np.abs(a - r).max())
        worst = max(worst, err / bound)
        assert err <= bound, f'{what}: {k}: max error {err:.3e} > {bound:.3e}'
    return worst


def _as_stored(rec):
    """The record as the generator stores it: the stereo output, the stage-0 map and the stage-0-only path are one tensor in the
    reference, kept once as out0."""
    rec = dict(rec)
    rec.pop('map0'), rec.pop('stage0')
    return rec


def test_fixture_is_what_it_says():
    g = fixture()
    assert [tuple(g[f'out{i}'].shape) for i in range(3)] == list(SW.OUT_SHAPES)
    assert [tuple(g[f'map{i}'].shape) for i in (1, 2, 3)] == [(2, h * w, c) for (h, w), c in zip(SW.MAPS[1:], SW.WIDTHS[1:])]
    assert tuple(g['x_grad'].shape) == SW.X_SHAPE and len(g['score_max']) == 8
    assert all(v.dtype == np.float64 for k, v in g.items() if k.startswith(('out', 'map', 'x_grad', 'grad.', 'gnorm.', 'gproj.')))
    import hashlib
    assert hashlib.sha256(np.ascontiguousarray(SW.x_input()).tobytes()).hexdigest() == str(g['x_sha'])
    for path in os.listdir(GOLDEN):
        if path.startswith(SW.STEM):
            assert os.path.getsize(os.path.join(GOLDEN, path)) <= 1 << 20, path


def test_port_against_the_reference_fixture():
    g = fixture()
    keys, sha, index, rec = port()
    assert keys == [str(k) for k in g['state_keys']]                         # same keys in the same order: checkpoints load
    assert sha == str(g['state_sha'])
    for k, v in index.items():
        assert np.array_equal(v.numpy(), g['state.' + k]), k                 # the bias lookup tables themselves, 12 x 12 windows
    names = [k[6:] for k in g if k.startswith('gnorm.')]
    assert len(names) == len([k for k in rec if k.startswith('gnorm.')]) and all('gproj.' + n in g for n in names)
    worst = _compare(_as_stored(rec), g, 'port')
    # the three tensors the fixture keeps once
    B, C, H, W = g['out0'].shape
    for k, a in (('stage0', rec['stage0']), ('map0', rec['map0'].reshape(B, H, W, C).transpose(0, 3, 1, 2))):
        err = float(np.abs(a - g['out0']).max())
        assert err <= TOL * max(1.0, float(np.abs(g['out0']).max())), (k, err)
    print(f'port against G20: worst error / bound {worst:.3e} over {sum(v.dtype.kind == "f" for v in g.values())} tensors')


def test_softmax_guard():
    """A cap on the input's quality, for the reference's run and the port's: in every block the largest score that enters a
    softmax (scale q k^T + bias, the mask aside) lies between 2 and 20 -- neither flat, where bias table and mask would not
    matter, nor saturated, where one key would hide every error in the others."""
    for what, s in (('reference', fixture()['score_max']), ('port', port()[3]['score_max'])):
        print(what, 'largest score per block:', np.round(s, 2))
        assert len(s) == 8 and float(s.min()) > 2.0 and float(s.max()) < 20.0, (what, s)


def test_generator_reproduces_the_fixture(tmp_path):
    """Where the reference is present, `make_golden.py g20` gives the committed fixture again (a process of its own: the generator
    installs stand-ins for third-party packages into sys.modules)."""
    code = ('import os, sys\n'
            f'sys.path.insert(0, {GOLDEN!r})\n'
            'import make_golden as M\n'
            'if not os.path.isdir(M.REF):\n'
            '    sys.exit(77)\n'
            f'M.write_g20({str(tmp_path)!r})\n')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    if r.returncode == 77:
        pytest.skip('the reference is not on this machine')
    assert r.returncode == 0, r.stderr[-2000:]
    new, g = SW.load(str(tmp_path)), fixture()
    assert sorted(new) == sorted(g)
    for k in g:
        if g[k].dtype.kind != 'f':
            assert np.array_equal(new[k], g[k]), k
    _compare(new, g, 'regenerated')
