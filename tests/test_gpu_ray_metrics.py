"""RayIoU on the MI355X: the HIP ray caster against the float64 twin (tests/rayiou_twin.py), and the fused counter kernel
against golden G19, the record of the reference's own Python (tests/golden/make_golden_rayiou.py).

The caster's bar is identity: the kernel and the twin read the same float32 inputs and perform the same IEEE double operations
in the same order under the same strict comparisons, so coord_index is equal and pred_dist bit-identical on every ray, rays on
exact ties included."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rayiou_twin as twin  # noqa: E402
from test_ray_metrics import KEYS, g19_samples  # noqa: E402

pytestmark = pytest.mark.gpu


def _render_and_compare(gpu, occ, origins_vox, ends_vox):
    """occ (nx,ny,nz) bool; origins_vox (T,3), ends_vox (T,M,3) float32: one call with T origins, a static grid and two padded
    rays, against one twin cast per origin.  Returns (rays compared, rays on an exact tie)."""
    import dhd_amd
    t_n, m = ends_vox.shape[:2]
    sigma = torch.from_numpy(np.ascontiguousarray(occ.transpose(2, 1, 0))).float()[None, None].to(gpu)
    tindex = np.repeat(np.arange(t_n, dtype=np.float32), m)
    points = ends_vox.reshape(-1, 3)
    pad = np.array([5, t_n * m - 7])
    tindex[pad] = -1
    nz, ny, nx = sigma.shape[2:]
    pd, gd, ci = dhd_amd.render_forward(sigma, torch.from_numpy(origins_vox)[None].to(gpu), torch.from_numpy(points)[None].to(gpu),
                                        torch.from_numpy(tindex)[None].to(gpu), [1, nz, ny, nx], 'test')
    assert pd.shape == (1, t_n * m) and gd.shape == (1, t_n * m) and ci.shape == (1, t_n * m, 3) and pd.dtype == torch.float32
    pd, gd, ci = pd[0].cpu().numpy(), gd[0].cpu().numpy(), ci[0].cpu().numpy()
    ties = 0
    for t in range(t_n):
        c = twin.cast(occ, origins_vox[t], ends_vox[t])
        e = c['entered']
        r = ends_vox[t].astype(np.float64) - origins_vox[t].astype(np.float64)
        length = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2])
        want_pd = np.where(e, c['dist'], -1.0).astype(np.float32)
        want_gd = np.where(e, length, -1.0).astype(np.float32)
        want_ci = np.where(e[:, None], c['coord'], 0).astype(np.float32)
        padded = np.isin(np.arange(t * m, (t + 1) * m), pad)
        want_pd[padded], want_gd[padded], want_ci[padded] = -1, -1, 0
        sl = slice(t * m, (t + 1) * m)
        n_coord = int((ci[sl] != want_ci).any(1).sum())
        n_dist = int((pd[sl].view(np.uint32) != want_pd.view(np.uint32)).sum())
        n_gt = int((gd[sl].view(np.uint32) != want_gd.view(np.uint32)).sum())
        ties += int((c['margin'] == 0).sum())
        print(f'origin {origins_vox[t]}: {m} rays, entered {int(e.sum())}, exact ties {int((c["margin"] == 0).sum())}, '
              f'coord mismatches {n_coord}, pred_dist bit mismatches {n_dist}, gt_dist bit mismatches {n_gt}')
        assert n_coord == 0 and n_dist == 0 and n_gt == 0
    return t_n * m, ties


def test_render_forward_is_the_twin_on_g19(gpu):
    g = golden('g19_rayiou')
    rays = g['rays']
    total = ties = 0
    for pred, gt, org in g19_samples(g):
        vox = [twin.to_voxel_units(o, rays, (-40.0, -40.0, -1.0), 0.4) for o in org[0]]
        o = np.stack([v[0] for v in vox])
        e = np.stack([v[1] for v in vox])
        for sem in (pred, gt):
            n, k = _render_and_compare(gpu, sem < 17, o, e)
            total, ties = total + n, ties + k
    print(f'{total} rays, {ties} on an exact tie')
    assert ties > 0          # the quarter-voxel origins put rays on exact ties; they are held to identity too


def test_render_forward_is_the_twin_on_a_ragged_grid(gpu):
    rays = golden('g19_rayiou')['rays']
    occ = np.random.RandomState(7).rand(37, 23, 5) < 0.04
    o = np.array([[17.3, 11.6, 2.4], [0.4, 0.7, 0.2], [20.2, 9.9, 11.5], [-6.3, 12.4, 2.7], [-0.5, 3.2, 1.1]], dtype=np.float32)
    e = np.stack([(rays.astype(np.float64) * 70 + p).astype(np.float32) for p in o])
    _render_and_compare(gpu, occ, o, e)


def test_render_forward_refuses_train_and_bad_shapes(gpu):
    import dhd_amd
    from dhd_amd import _lib
    z = torch.zeros(1, 1, 16, 200, 200, device=gpu)
    args = (torch.zeros(1, 1, 3, device=gpu), torch.ones(1, 4, 3, device=gpu), torch.zeros(1, 4, device=gpu))
    with pytest.raises(_lib.DhdError, match='UNSUPPORTED'):
        dhd_amd.render_forward(z, *args, [1, 16, 200, 200], 'train')
    with pytest.raises(_lib.DhdError):
        dhd_amd.render_forward(z, *args, [1, 16, 100, 200], 'test')
    # a zero-length ray (end point = origin: NaN directions, every comparison false) steps down in z and out of the grid
    pd, _, ci = dhd_amd.render_forward(z, torch.full((1, 1, 3), 3.5, device=gpu), torch.full((1, 4, 3), 3.5, device=gpu),
                                       torch.zeros(1, 4, device=gpu), [1, 16, 200, 200], 'test')
    torch.cuda.synchronize()
    assert ci.min() >= 0 and ci[..., 2].max() < 16


def _g19_counts(g, which):
    return twin.counters((g[f'label{i}'][:, 1].astype(np.int64), g[f'dist{i}'][:, 1], g[f'label{i}'][:, 0].astype(np.int64),
                          g[f'dist{i}'][:, 0]) for i in which)


def test_accumulate_gives_g19_counters(gpu):
    import dhd_amd
    g = golden('g19_rayiou')
    samples = g19_samples(g)
    assert np.array_equal(_g19_counts(g, (0, 1, 2)), g['counts'])

    one = dhd_amd.RayIoU()
    one.add_batch(np.stack([s[0] for s in samples]), np.stack([s[1] for s in samples]), [s[2] for s in samples])
    assert one.counts.dtype == torch.int64 and one.counts.is_cuda and one.counts.shape == (5, 18)
    got = one.counts.cpu().numpy()
    print('gt_cnt', got[0], '\npred_cnt', got[1], '\ntp_cnt', got[2:], '\ndifference from G19', np.abs(got - g['counts']).sum())
    assert np.array_equal(got, g['counts'])
    res = one.count()
    for k in KEYS:
        print(k, res[k], float(g['result_' + k]))
        assert abs(res[k] - float(g['result_' + k])) < 1e-12
    assert res['per_class'].shape == (3, 17)

    # float64 origins (samples 0, 1) and float32 origins (sample 2), each against the reference's per-ray record
    for which in ((0, 1), (2,)):
        m = dhd_amd.RayIoU()
        for i in which:                                   # one sample per call: calls accumulate
            m.add_batch(samples[i][0], samples[i][1], samples[i][2])
        assert np.array_equal(m.counts.cpu().numpy(), _g19_counts(g, which)), which
    # the same origin values in the other precision take the other arithmetic chain: checked against the twin
    pred, gt, org = samples[2]
    o64 = org[0].astype(np.float64)[:1]
    m = dhd_amd.RayIoU()
    m.add_batch(pred, gt, o64)
    pl, pd, _ = twin.sample(pred, o64, g['rays'])
    gl, gd, _ = twin.sample(gt, o64, g['rays'])
    assert np.array_equal(m.counts.cpu().numpy(), twin.counters([(pl, pd, gl, gd)]))

    # sample order does not matter; two calls give the one-call result
    rev = dhd_amd.RayIoU()
    rev.add_batch(np.stack([s[0] for s in samples[::-1]]), np.stack([s[1] for s in samples[::-1]]), [s[2] for s in samples[::-1]])
    assert torch.equal(rev.counts, one.counts)
    two = dhd_amd.RayIoU()
    two.add_batch(samples[0][0], samples[0][1], samples[0][2])
    two.add_batch(torch.from_numpy(np.stack([s[0] for s in samples[1:]])).to(gpu), torch.from_numpy(np.stack([s[1] for s in samples[1:]])),
                  [torch.from_numpy(s[2]) for s in samples[1:]])
    assert torch.equal(two.counts, one.counts)


def test_accumulate_on_a_ragged_grid_with_other_classes(gpu):
    """37 x 23 x 5 voxels of 0.5 m, 6 classes, 4 thresholds: the form for grids that are not Occ3D's, against the twin."""
    import dhd_amd
    rays = golden('g19_rayiou')['rays']
    rng = np.random.RandomState(11)
    gt = np.where(rng.rand(37, 23, 5) < 0.05, rng.randint(0, 5, (37, 23, 5)), 5).astype(np.uint8)
    gt[:, :, 0] = 3
    pred = np.where(rng.rand(37, 23, 5) < 0.1, rng.randint(0, 6, (37, 23, 5)), gt).astype(np.uint8)
    names = ('a', 'b', 'c', 'd', 'e', 'free')
    thr = (0.5, 1, 2, 3)
    org = np.array([[9.1, 6.2, 1.3], [1.0, 11.0, 2.2], [14.0, 3.0, 4.0]])
    kw = dict(lower=(0.0, 0.0, 0.0), voxel=0.5, free_id=5)
    for dt in (np.float64, np.float32):
        m = dhd_amd.RayIoU(pc_range=(0, 0, 0, 18.5, 11.5, 2.5), voxel_size=0.5, class_names=names, thresholds=thr)
        assert m.grid == (37, 23, 5)
        m.add_batch(pred, gt, org.astype(dt))
        pl, pd, _ = twin.sample(pred, org.astype(dt), rays, **kw)
        gl, gd, _ = twin.sample(gt, org.astype(dt), rays, **kw)
        want = twin.counters([(pl, pd, gl, gd)], n_classes=6, free_id=5, thresholds=thr)
        assert want[0].sum() > 10000
        assert np.array_equal(m.counts.cpu().numpy(), want), dt
        assert set(m.count()) == {'RayIoU', 'RayIoU@0.5', 'RayIoU@1', 'RayIoU@2', 'RayIoU@3', 'per_class'}


def test_device_pred_of_occ_argmax_hist_goes_in_as_it_is(gpu):
    import dhd_amd
    from dhd_amd.occ_loss import occ_argmax_hist
    g = golden('g19_rayiou')
    _, gt, org = g19_samples(g)[0]
    gen = torch.Generator().manual_seed(3)
    logits = torch.randn(200 * 200 * 16, 18, generator=gen)
    logits[torch.arange(logits.shape[0]), torch.from_numpy(gt.reshape(-1).astype(np.int64))] += 3.0      # mostly right
    pred_dev, _ = occ_argmax_hist(logits.to(gpu))
    a = dhd_amd.RayIoU()
    a.device = gpu
    assert a._grids(pred_dev, 'pred').data_ptr() == pred_dev.data_ptr()        # no copy
    a.add_batch(pred_dev, gt, org)
    b = dhd_amd.RayIoU()
    b.add_batch(pred_dev.cpu().numpy().reshape(200, 200, 16), gt, org)
    assert a.counts[0].sum() > 0 and torch.equal(a.counts, b.counts)


def test_calc_rayiou_returns_the_references_numbers(gpu):
    import dhd_amd
    g = golden('g19_rayiou')
    samples = g19_samples(g)
    res = dhd_amd.calc_rayiou([s[0].reshape(-1) for s in samples], [s[1] for s in samples], [torch.from_numpy(s[2]) for s in samples])
    assert set(res) == set(KEYS)
    for k in KEYS:
        assert abs(res[k] - float(g['result_' + k])) < 1e-12, (k, res[k])
