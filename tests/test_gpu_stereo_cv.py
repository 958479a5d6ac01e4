"""The stereo cost volume from the camera matrices (dhd_amd/stereo_cv.py, csrc/stereo_cv.h) on the GPU, against today's path on
the same tensors: `gen_grid` (about forty torch launches) + `_hip_cost_volume` (float32 and NHWC copies + dhd_stereo_cost_volume).

  positions   bit for bit gen_grid's                                      float32   bit for bit today's bytes
  half types  |got - ref| <= 1e-4 + 2 eps_T |ref|, columns sum to 1       layouts   the same bytes whatever the memory
  module      G8 through DepthNet.calculate_cost_volumn                   routing   off: today's calls; c = 12: grid kernel
  bounds      nothing outside the buffers, a second call the same bytes

Inputs: tests/stereo_cv_inputs.py (tests/test_stereo_cv_inputs.py holds their conditions without a GPU).  Maps are 8 x 22."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import guarded_alloc as G  # noqa: E402
import stereo_cv_inputs as inp  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
UNIT_ROUNDOFF = {F16: 2.0 ** -11, BF16: 2.0 ** -8}      # half an ulp of 1: 11 and 8 significant bits
H, W = 8, 22
CAL_KEYS = ('post_rots', 'post_trans', 'intrins', 'k2s_sensor')


@functools.lru_cache(maxsize=None)
def _metas(kind, n_depth, frustum_dtype=F32, small=False):
    return inp.metas(kind, n_depth, 'cuda', frustum_dtype, inp.SMALL_INPUT_SIZE if small else inp.INPUT_SIZE)


@functools.lru_cache(maxsize=None)
def _features(c, dtype, h=H, w=W):
    return tuple(t.cuda() for t in inp.features(c, h, w, dtype))


@functools.lru_cache(maxsize=None)
def _net(n_depth, bias):
    return inp.depthnet(n_depth, bias)


def _flag(c):
    return (c // 4 - 1) * 4


def _gen_grid(m, hi=None, wi=None):
    B, N, _ = m['post_trans'].shape
    D, h, w, _ = m['frustum'].shape
    return _net(D, 0.0).gen_grid(m, B, N, D, h, w, hi or h * 4, wi or w * 4)


@functools.lru_cache(maxsize=None)
def _today(kind, n_depth, c, dtype, bias):
    """Today's path on the shared tensors: gen_grid, rounded through the features' dtype, + _hip_cost_volume.  Computed once."""
    m = _metas(kind, n_depth)
    prev, curr = _features(c, dtype)
    return _net(n_depth, bias)._hip_cost_volume(prev, curr, _gen_grid(m).to(dtype), n_depth, _flag(c))


def _fused(kind, n_depth, c, dtype, bias, prev=None, curr=None):
    import dhd_amd
    m = _metas(kind, n_depth)
    if prev is None:
        prev, curr = _features(c, dtype)
    return dhd_amd.stereo_cost_volume(prev, curr, m['frustum'], *[m[k] for k in CAL_KEYS], bias, _flag(c))


# ------------------------------------------------------------------------------------------------ 1. positions

@pytest.mark.parametrize('kind', inp.CALIBRATIONS)
@pytest.mark.parametrize('n_depth', [12, 70, 130])
def test_positions_are_gen_grids_bits(gpu, kind, n_depth):
    import dhd_amd
    m = _metas(kind, n_depth)
    ref = _gen_grid(m)
    got = dhd_amd.stereo_sampling_grid(m['frustum'], *[m[k] for k in CAL_KEYS], H * 4, W * 4)
    differ = int((got.view(torch.int32) != ref.view(torch.int32)).sum())
    inside, marked, outside = inp.shares(ref)
    print(f'{kind} D={n_depth}: {differ} of {ref.numel()} words differ; inside {inside:.3f} marked {marked:.3f} outside {outside:.3f}')
    assert got.shape == ref.shape == (2, n_depth * H, W, 2) and got.dtype == F32
    assert torch.equal(got, ref)


@pytest.mark.parametrize('kind', inp.CALIBRATIONS)
def test_positions_of_the_small_map(gpu, kind):
    import dhd_amd
    m = _metas(kind, 12, F32, True)
    hi, wi = inp.SMALL_INPUT_SIZE
    ref = _gen_grid(m, hi, wi)
    got = dhd_amd.stereo_sampling_grid(m['frustum'], *[m[k] for k in CAL_KEYS], hi, wi)
    assert got.shape == (2, 12 * 5, 7, 2) and torch.equal(got, ref)


@pytest.mark.parametrize('dtype', [BF16, F16])
def test_positions_from_a_half_frustum(gpu, dtype):
    """A frustum template in a half type is promoted to float32 by gen_grid's first subtraction; the axes are converted the same."""
    import dhd_amd
    m = _metas('b', 70, dtype)
    assert m['frustum'].dtype == dtype
    ref = _gen_grid(m)
    got = dhd_amd.stereo_sampling_grid(m['frustum'], *[m[k] for k in CAL_KEYS], H * 4, W * 4)
    assert ref.dtype == F32 and torch.equal(got, ref)
    assert not torch.equal(ref, _gen_grid(_metas('b', 70)))       # the rounded template is another template


# ------------------------------------------------------------------------------------------------ 2. float32: today's bytes

@pytest.mark.parametrize('c', [16, 128, 132, 520])
@pytest.mark.parametrize('bias', [0.0, 5.0])
@pytest.mark.parametrize('kind,n_depth', [('a', 12), ('b', 70)])
def test_float32_is_todays_bytes(gpu, c, bias, kind, n_depth):
    ref = _today(kind, n_depth, c, F32, bias)
    got = _fused(kind, n_depth, c, F32, bias)
    assert got.shape == ref.shape == (2, n_depth, H, W) and got.dtype == F32
    print(f'c={c} bias={bias} {kind} D={n_depth}: max |diff| {float((got - ref).abs().max()):.3e}, max p {float(ref.max()):.3f}')
    assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------ 3. half types

HALF_CASES = [(8, 12, 'a'), (8, 130, 'b'), (64, 65, 'b'), (128, 88, 'a'), (128, 130, 'c'), (136, 12, 'b'), (256, 88, 'b'), (264, 65, 'a'),
              (520, 12, 'c'), (520, 130, 'b')]


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('c,n_depth,kind', HALF_CASES)
def test_half_types_against_todays_path_on_the_same_tensors(gpu, dtype, c, n_depth, kind):
    """Both paths see the same float32 values (a half widens exactly) and the same rounded positions; the channel sums run in
    another order (the project's 1e-4 bar) and each output is rounded once (2 eps_T |ref|: today's path rounds too)."""
    eps = UNIT_ROUNDOFF[dtype]
    ref = _today(kind, n_depth, c, dtype, 5.0)
    prev, curr = (t.contiguous(memory_format=torch.channels_last) for t in _features(c, dtype))
    got = _fused(kind, n_depth, c, dtype, 5.0, prev, curr)
    assert got.shape == ref.shape == (2, n_depth, H, W) and got.dtype == ref.dtype == dtype
    g, r = got.double(), ref.double()
    excess = ((g - r).abs() - (1e-4 + 2 * eps * r.abs())).max().item()
    colsum = (g.sum(1) - 1).abs().max().item()
    print(f'{dtype} c={c} D={n_depth} {kind}: max |diff| {float((g - r).abs().max()):.3e}, over the bar by {excess:.3e}; '
          f'column sums off by {colsum:.3e} (bar {n_depth * eps:.3e}); max p {float(r.max()):.3f}')
    assert torch.isfinite(got).all()
    assert excess <= 0
    assert colsum <= n_depth * eps


# ------------------------------------------------------------------------------------------------ 4. layouts

@pytest.mark.parametrize('dtype,c', [(F32, 132), (F16, 128), (BF16, 264)])
def test_layouts_give_the_same_bytes(gpu, dtype, c, monkeypatch):
    from dhd_amd import _stereo_cv
    layouts = []
    real = _stereo_cv.call
    monkeypatch.setattr(_stereo_cv, 'call', lambda name, *a: (layouts.append(a[4]) if name == 'dhdv_stereo_cost_volume' else None, real(name, *a))[1])
    prev, curr = _features(c, dtype)
    base = _fused('b', 70, c, dtype, 5.0)                                                      # dense NCHW
    cl = [t.contiguous(memory_format=torch.channels_last) for t in (prev, curr)]
    views = [t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for t in (prev, curr)]     # NHWC memory behind a permuted view
    mixed = [cl[0], curr]

    def offset(t, nhwc):
        """the same values at a storage offset of one element: the address is no multiple of 16"""
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:]
        if nhwc:
            v = flat.view(t.shape[0], t.shape[2], t.shape[3], t.shape[1]).permute(0, 3, 1, 2)
        else:
            v = flat.view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 != 0 and torch.equal(v, t)
        return v

    runs = [('channels_last', cl, _stereo_cv.NHWC), ('permuted view', views, _stereo_cv.NHWC), ('one of each', mixed, _stereo_cv.NCHW),
            ('offset NCHW', [offset(t, False) for t in (prev, curr)], _stereo_cv.NCHW),
            ('offset NHWC', [offset(t, True) for t in (prev, curr)], _stereo_cv.NCHW),
            ('strided', [torch.cat([t, t], 1)[:, :c] for t in (prev, curr)], _stereo_cv.NCHW)]
    assert layouts == [_stereo_cv.NCHW]
    for name, (p, q), want in runs:
        got = _fused('b', 70, c, dtype, 5.0, p, q)
        assert layouts[-1] == want, name
        assert torch.equal(got, base), name


# ------------------------------------------------------------------------------------------------ 5. G8 through the module

def test_g8_through_the_module_with_the_switch_on(gpu, monkeypatch):
    import dhd_amd
    from dhd_amd import _stereo_cv, stereo_cv
    g = inp.g8()
    d = g['frustum'].shape[0]
    dn = inp.depthnet(d, float(g['bias']))
    t = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    metas = dict(k2s_sensor=t(g['k2s_sensor']), intrins=t(g['intrins']), post_rots=t(g['post_rots']), post_trans=t(g['post_trans']),
                 frustum=t(g['frustum']), cv_feat_list=[t(g['prev']), t(g['curr'])])
    calls, real = [], _stereo_cv.call
    monkeypatch.setattr(_stereo_cv, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    monkeypatch.setattr(stereo_cv, 'ROUTED', {k: True for k in stereo_cv.ROUTED})
    assert dn.use_hip_cost_volume and dhd_amd.fused_stereo_cost_volume(dn) == [dn]
    cv = dn.calculate_cost_volumn(metas)
    assert calls == ['dhdv_stereo_cost_volume']
    np.testing.assert_allclose(cv.cpu().numpy(), g['cost_volume'], rtol=2e-4, atol=2e-6)


# ------------------------------------------------------------------------------------------------ 6. routing

def _module_run(dn, kind, n_depth, c, dtype, frustum=None):
    m = dict(_metas(kind, n_depth))
    if frustum is not None:
        m['frustum'] = frustum
    m['cv_feat_list'] = list(_features(c, dtype))
    return dn.calculate_cost_volumn(m)


def test_routing(gpu, monkeypatch):
    import dhd_amd
    from dhd_amd import _lib, _stereo_cv, stereo_cv
    for dtype, c in ((F32, 16), (BF16, 128), (BF16, 12)):      # the shared references, before the calls are counted
        _today('b', 70, c, dtype, 5.0)
    calls, real_call = [], _stereo_cv.call
    monkeypatch.setattr(_stereo_cv, 'call', lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    checked, real_check = [], _lib.check
    monkeypatch.setattr(_lib, 'check', lambda rc, what: (checked.append(what), real_check(rc, what))[1])
    dn = inp.depthnet(70, 5.0)
    # the switch off (the default): today's bytes, today's calls
    assert 'DHD_STEREO_CV' in os.environ or dn.fused_cost_volume is False
    dhd_amd.fused_stereo_cost_volume(dn, False)
    for dtype, c in ((F32, 16), (BF16, 128)):
        assert torch.equal(_module_run(dn, 'b', 70, c, dtype), _today('b', 70, c, dtype, 5.0))
    assert calls == [] and not [w for w in checked if w.startswith('dhdv')] and checked.count('dhd_stereo_cost_volume') == 2
    # on, but nothing routed: today's path
    dhd_amd.fused_stereo_cost_volume(dn, True)
    monkeypatch.setattr(stereo_cv, 'ROUTED', {k: False for k in stereo_cv.ROUTED})
    assert torch.equal(_module_run(dn, 'b', 70, 128, BF16), _today('b', 70, 128, BF16, 5.0)) and calls == []
    # on and routed: the operator
    monkeypatch.setattr(stereo_cv, 'ROUTED', {k: True for k in stereo_cv.ROUTED})
    assert torch.equal(_module_run(dn, 'b', 70, 16, F32), _today('b', 70, 16, F32, 5.0)) and calls == ['dhdv_stereo_cost_volume']
    # on, 12 half channels (no 16-byte groups of 8): the grid kernel feeds today's kernel -- the same positions, so the same bytes
    del calls[:], checked[:]
    assert torch.equal(_module_run(dn, 'b', 70, 12, BF16), _today('b', 70, 12, BF16, 5.0))
    assert calls == ['dhdv_stereo_grid'] and checked.count('dhd_stereo_cost_volume') == 1
    # on, a frustum that is not separable: today's path
    del calls[:], checked[:]
    broken = _metas('b', 70)['frustum'].clone()
    broken[5, 3, 7, 0] += 0.25
    dn0 = inp.depthnet(70, 5.0)
    assert dn0.fused_cost_volume is False or 'DHD_STEREO_CV' in os.environ
    dhd_amd.fused_stereo_cost_volume(dn0, False)
    ref = _module_run(dn0, 'b', 70, 128, BF16, broken)
    del calls[:], checked[:]
    got = _module_run(dn, 'b', 70, 128, BF16, broken)
    assert torch.equal(got, ref) and not torch.equal(ref, _today('b', 70, 128, BF16, 5.0))
    assert calls == [] and checked.count('dhd_stereo_cost_volume') == 1


# ------------------------------------------------------------------------------------------------ 7. bounds and repeatability

@pytest.mark.parametrize('dtype,c,nhwc', [(F32, 132, False), (BF16, 128, False), (F16, 264, True), (BF16, 8, True)])
def test_nothing_outside_the_buffers_and_a_second_call_gives_the_same_bytes(gpu, dtype, c, nhwc, monkeypatch):
    import dhd_amd
    m = _metas('b', 130)
    prev, curr = _features(c, dtype)
    if nhwc:
        prev, curr = (t.contiguous(memory_format=torch.channels_last) for t in (prev, curr))
    plain = _fused('b', 130, c, dtype, 5.0, prev, curr)
    again = _fused('b', 130, c, dtype, 5.0, prev, curr)
    assert torch.equal(plain, again)
    grid = dhd_amd.stereo_sampling_grid(m['frustum'], *[m[k] for k in CAL_KEYS], H * 4, W * 4)
    for fill in (0xFF, 0x00):
        with G.guarded(monkeypatch, fill) as ledger:
            got = _fused('b', 130, c, dtype, 5.0, prev, curr)
            got_grid = dhd_amd.stereo_sampling_grid(m['frustum'], *[m[k] for k in CAL_KEYS], H * 4, W * 4)
            ledger.check()
            got, got_grid = got.clone(), got_grid.clone()
        ours = [e for e in ledger.sites_under(G.PRODUCT_ROOT) if 'stereo_cv.py' in e.site or 'mghs_op.py' in e.site]
        print(f'{dtype} c={c} nhwc={nhwc} [fill {fill:#04x}]: {len(ledger)} guarded allocations, {ledger.total_bytes()} bytes, guards intact')
        assert len(ours) == len(ledger) == (2 if nhwc else 3), [e.site for e in ledger.entries]      # out, grid [, scratch]
        assert torch.equal(got, plain) and torch.equal(got_grid, grid), fill
