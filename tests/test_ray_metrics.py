"""RayIoU without a GPU: the host half of dhd_amd.ray_metrics, golden G19 (the reference's own Python, see
tests/golden/make_golden_rayiou.py) against the float64 twin, the twin against an independent brute-force ray caster, and the
argument checks of the two C entry points that run before any launch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rayiou_twin as twin  # noqa: E402

KEYS = ('RayIoU', 'RayIoU@1', 'RayIoU@2', 'RayIoU@4')


def g19_samples(g):
    """-> list of (pred (200,200,16) u8, gt, origins (1,T,3) in the recorded dtype)."""
    out = []
    for i in range(3):
        gt = g[f'gt{i}']
        pred = gt.copy().reshape(-1)
        pred[g[f'pred{i}_index']] = g[f'pred{i}_value']
        out.append((pred.reshape(gt.shape), gt, g[f'origins{i}']))
    return out


def test_ray_set_is_the_references_bit_for_bit():
    from dhd_amd import generate_lidar_rays
    rays = generate_lidar_rays()
    ref = golden('g19_rayiou')['rays']
    assert rays.dtype == np.float32 and rays.shape == (14040, 3) == ref.shape
    assert np.array_equal(rays.view(np.uint32), ref.view(np.uint32))
    assert np.abs(np.linalg.norm(rays.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_twin_reproduces_g19():
    """The twin's caster is the stub the fixture was made with, so this pins the reference's Python half (voxel-unit conversion
    for float64 and float32 origin tensors, the float32 distance product, label lookup, validity mask, counters, means) and
    guards the twin against drift."""
    g = golden('g19_rayiou')
    samples = g19_samples(g)
    assert [s[2].dtype for s in samples] == [np.float64, np.float64, np.float32]
    pairs, never = [], 0
    for i, (pred, gt, org) in enumerate(samples):
        pl, pd, _ = twin.sample(pred, org[0], g['rays'])
        gl, gd, _ = twin.sample(gt, org[0], g['rays'])
        assert np.array_equal(gl, g[f'label{i}'][:, 0]) and np.array_equal(pl, g[f'label{i}'][:, 1])
        assert np.array_equal(gd.view(np.uint32), g[f'dist{i}'][:, 0].view(np.uint32))
        assert np.array_equal(pd.view(np.uint32), g[f'dist{i}'][:, 1].view(np.uint32))
        never += int((gd == np.float32(-1) * np.float32(0.4)).sum())
        pairs.append((pl, pd, gl, gd))
    assert never > 1000          # the far origin: rays that run out of steps keep distance -0.4 and the label of voxel (0,0,0)
    cnt = twin.counters(pairs)
    assert cnt.dtype == np.int64 and np.array_equal(cnt, g['counts'])
    res, _ = twin.metrics(cnt)
    for k in KEYS:
        assert abs(res[k] - float(g['result_' + k])) < 1e-12


def test_host_metric_arithmetic_matches_g19():
    from dhd_amd.ray_metrics import metrics_from_counts
    g = golden('g19_rayiou')
    res = metrics_from_counts(g['counts'])
    for k in KEYS:
        assert abs(res[k] - float(g['result_' + k])) < 1e-12
    assert res['per_class'].shape == (3, 17)
    empty = metrics_from_counts(np.zeros((5, 18), dtype=np.int64))     # 0 / 0 = NaN per class, as in the reference
    assert np.isnan(empty['RayIoU'])


def test_twin_against_brute_force():
    """Independent of the stepping algorithm: on a ragged 37 x 23 x 5 grid at 4 % occupancy, for each of four origins (inside,
    near a corner, above, beside the grid) and all 14 040 rays, the hit voxel must be the occupied voxel whose slab the ray
    enters first and the distance that slab's exit parameter, to 1e-11 (at most 65 additions at magnitude <= 64 in float64).
    Rays within 1e-9 voxel of a tie in either method are set aside; they may be at most 0.1 % of the rays."""
    rays = golden('g19_rayiou')['rays']
    rng = np.random.RandomState(7)
    occ = rng.rand(37, 23, 5) < 0.04
    origins = np.array([[17.3, 11.6, 2.4], [0.4, 0.7, 0.2], [20.2, 9.9, 11.5], [-6.3, 12.4, 2.7]], dtype=np.float32)
    for o in origins:
        e = (rays.astype(np.float64) * 70 + o).astype(np.float32)       # end points beyond the grid in every direction
        c = twin.cast(occ, o, e)
        hit, vox, far, margin = twin.brute_force(occ, o, e)
        band = (c['margin'] < 1e-9) | (margin < 1e-9)
        print('origin', o, 'tie band', int(band.sum()), 'hits', int(hit.sum()))
        assert band.sum() <= 14
        ok = ~band
        twin_hit = c['entered'] & occ[np.where(c['entered'], c['coord'][:, 0], 0), np.where(c['entered'], c['coord'][:, 1], 0),
                                      np.where(c['entered'], c['coord'][:, 2], 0)]
        assert np.array_equal(twin_hit[ok], hit[ok])
        both = ok & hit
        assert both.sum() > 100             # the comparison has something to look at
        assert np.array_equal(c['coord'][both], vox[both])
        err = np.abs(c['dist'][both] - far[both]).max()
        print('max |exit - slab exit|', err)
        assert err < 1e-11
        # a ray that hits nothing ends in a free voxel inside the grid (the last one on its way), or never entered
        miss = ok & ~hit & c['entered']
        assert not occ[c['coord'][miss, 0], c['coord'][miss, 1], c['coord'][miss, 2]].any()


def test_entry_points_validate_before_any_launch():
    from dhd_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(64)
    f3 = (C.c_float * 3)(-40, -40, -1)
    thr = (C.c_float * 4)(1, 2, 4, 8)
    acc = lambda **kw: lib.dhd_ray_iou_accumulate(*[{**dict(pred=one, gt=one, s=1, nx=200, ny=200, nz=16, sid=one, org=one, k=2, flags=1,
                                                          rays=one, n_rays=14040, lower=f3, voxel=0.4, free=17, nc=18, thr=thr, nt=3,
                                                          counts=one, stream=None), **kw}[n]
                                                   for n in ('pred', 'gt', 's', 'nx', 'ny', 'nz', 'sid', 'org', 'k', 'flags', 'rays', 'n_rays',
                                                             'lower', 'voxel', 'free', 'nc', 'thr', 'nt', 'counts', 'stream')])
    for name in ('pred', 'gt', 'sid', 'org', 'rays', 'lower', 'thr', 'counts'):
        assert acc(**{name: None}) == -1, name
    for name in ('s', 'nx', 'ny', 'nz', 'k', 'n_rays', 'nc', 'nt'):
        assert acc(**{name: -1}) == -1 and acc(**{name: 0}) == -1, name
    assert acc(free=-1) == -1 and acc(flags=8) == -1 and acc(voxel=0.0) == -1
    assert acc(org=C.c_void_p(68)) == -1 and acc(counts=C.c_void_p(68)) == -1       # misaligned double origins / int64 counters
    assert acc(nc=33) == -3 and acc(nt=5) == -3 and acc(nx=1 << 16, ny=1 << 16) == -3
    assert lib.dhd_ray_iou_supported(200, 200, 16, 18, 3) == 1 and lib.dhd_ray_iou_supported(37, 23, 5, 32, 4) == 1
    assert lib.dhd_ray_iou_supported(200, 200, 16, 33, 3) == 0 and lib.dhd_ray_iou_supported(200, 200, 16, 18, 5) == 0
    assert lib.dhd_ray_iou_supported(0, 200, 16, 18, 3) == 0 and lib.dhd_ray_iou_supported(2048, 2048, 512, 18, 3) == 0

    rf = lambda **kw: lib.dhd_ray_render_forward(*[{**dict(sigma=one, origin=one, points=one, tindex=one, n=1, ts=1, to=1, m=100, nz=16,
                                                         ny=200, nx=200, phase=0, pd=one, gd=one, ci=one, stream=None), **kw}[n]
                                                  for n in ('sigma', 'origin', 'points', 'tindex', 'n', 'ts', 'to', 'm', 'nz', 'ny', 'nx',
                                                            'phase', 'pd', 'gd', 'ci', 'stream')])
    for name in ('sigma', 'origin', 'points', 'tindex', 'pd', 'gd', 'ci'):
        assert rf(**{name: None}) == -1, name
    for name in ('n', 'ts', 'to', 'm', 'nz', 'ny', 'nx'):
        assert rf(**{name: -1}) == -1 and rf(**{name: 0}) == -1, name
    assert rf(phase=1) == -3 and rf(phase=2) == -1          # "train" is refused, anything else is no phase
    assert lib.dhd_abi_version() == 6


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the behaviour without a GPU')
def test_no_gpu_is_an_error_not_a_fallback():
    import dhd_amd
    from dhd_amd import _lib
    g = golden('g19_rayiou')
    pred, gt, org = g19_samples(g)[0]
    with pytest.raises(_lib.DhdError):
        dhd_amd.RayIoU().add_batch(pred, gt, org)
    with pytest.raises(_lib.DhdError):
        dhd_amd.calc_rayiou([pred], [gt], [org])
    z = torch.zeros(1, 1, 16, 200, 200)
    with pytest.raises(_lib.DhdError):
        dhd_amd.render_forward(z, torch.zeros(1, 1, 3), torch.ones(1, 4, 3), torch.zeros(1, 4), [1, 16, 200, 200], 'test')
    with pytest.raises(_lib.DhdError):
        dhd_amd.render_forward(z, torch.zeros(1, 1, 3), torch.ones(1, 4, 3), torch.zeros(1, 4), [1, 16, 200, 200], 'eval')
