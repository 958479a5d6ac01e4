"""Float64 numpy restatement of the RayIoU pipeline (helper of the ray-metric tests, not a test): the voxel traversal of the
published ray caster, the conversion of origins and rays to voxel units for float64 and float32 origins, labels, counters and the
final means.  Written from the algorithm; every ray of a call advances in lock step, one numpy operation per scalar
operation of the per-ray loop, in the same order, so a device kernel that performs the same IEEE operations gives the same bits.

cast() also reports, per ray, the number of loop iterations and the tie margin: the smallest gap between the two lowest
boundary parameters (tMax) met on the way.  A ray with margin 0 sits on an exact tie, where only the comparison order decides
which voxel comes next."""
import numpy as np

MAX_STEP = 1000
DBL_MAX = np.finfo(np.float64).max


def cast(occ, origin, points):
    """occ (nx,ny,nz) bool; origin (3,), points (M,3) float32 voxel units ->
    dict(coord (M,3) int64, dist (M,) float64, entered (M,) bool, steps (M,) int64, margin (M,) float64)."""
    nx, ny, nz = occ.shape
    n = np.array([nx, ny, nz])
    o = np.asarray(origin, dtype=np.float32).astype(np.float64).reshape(1, 3)
    e = np.asarray(points, dtype=np.float32).astype(np.float64)
    m = e.shape[0]
    with np.errstate(all='ignore'):
        v = np.broadcast_to(np.trunc(o).astype(np.int64), (m, 3)).copy()
        r = e - o
        length = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2])
        d = r / length[:, None]
        step = np.where(d >= 0, 1, -1).astype(np.int64)
        bound = (v + (step > 0)).astype(np.float64)
        nz_dir = d != 0
        t = np.where(nz_dir, (bound - o) / d, DBL_MAX)
        dt = np.where(nz_dir, step / d, DBL_MAX)

        coord = np.zeros((m, 3), dtype=np.int64)
        dist = np.zeros(m)
        entered = np.zeros(m, dtype=bool)
        steps = np.zeros(m, dtype=np.int64)
        margin = np.full(m, np.inf)
        active = np.ones(m, dtype=bool)
        for _ in range(MAX_STEP + 1):
            inside = np.all((v >= 0) & (v < n), axis=1)
            active &= ~(~inside & entered)
            if not active.any():
                break
            steps += active
            cur = v.copy()
            tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
            x_lt_y = tx < ty
            axis = np.where(x_lt_y, np.where(tx < tz, 0, 2), np.where(ty < tz, 1, 2))
            rows = np.arange(m)
            left_at = t[rows, axis]
            ts = np.sort(t, axis=1)
            gap = ts[:, 1] - ts[:, 0]
            margin = np.where(active & (gap < margin), gap, margin)
            adv = active
            v[rows[adv], axis[adv]] += step[rows[adv], axis[adv]]
            t[rows[adv], axis[adv]] += dt[rows[adv], axis[adv]]
            rec = active & inside
            entered |= rec
            coord[rec] = cur[rec]
            dist[rec] = left_at[rec]
            hit = np.zeros(m, dtype=bool)
            hit[rec] = occ[cur[rec, 0], cur[rec, 1], cur[rec, 2]]
            active &= ~hit
    return dict(coord=coord, dist=dist, entered=entered, steps=steps, margin=margin)


def to_voxel_units(origin, rays, lower, voxel):
    """origin (3,) float32 or float64 metres, rays (M,3) float32, lower (3,) and voxel as float32 -> origin, end points in
    voxel units, float32.  The arithmetic runs in the origin's dtype (float32 constants widened exactly), rounded once."""
    dt = origin.dtype
    assert dt in (np.float32, np.float64) and rays.dtype == np.float32
    lower = np.asarray(lower, dtype=np.float32).astype(dt)
    voxel = np.float32(voxel).astype(dt)
    end = rays.astype(dt) + origin[None, :]
    return ((origin - lower) / voxel).astype(np.float32), ((end - lower) / voxel).astype(np.float32)


def render(sem, origin, rays, lower=(-40.0, -40.0, -1.0), voxel=0.4, free_id=17):
    """One origin through one class grid (nx,ny,nz) -> label (M,) int64, dist (M,) float32 metres, and cast()'s dict."""
    o, e = to_voxel_units(origin, rays, lower, voxel)
    c = cast(sem < free_id, o, e)
    dist = np.where(c['entered'], c['dist'].astype(np.float32), np.float32(-1.0)).astype(np.float32) * np.float32(voxel)
    xyz = np.where(c['entered'][:, None], c['coord'], 0)
    return sem[xyz[:, 0], xyz[:, 1], xyz[:, 2]].astype(np.int64), dist, c


def sample(sem, origins, rays, **kw):
    """All origins (T,3) of one sample -> label (T*M,), dist (T*M,), total loop iterations."""
    parts = [render(sem, o, rays, **kw) for o in origins]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), sum(int(p[2]['steps'].sum()) for p in parts)


def counters(pairs, n_classes=18, free_id=17, thresholds=(1, 2, 4)):
    """pairs: iterable of (pred_label, pred_dist, gt_label, gt_dist) -> int64 (2 + n_thr, n_classes): gt | pred | tp[j]."""
    out = np.zeros((2 + len(thresholds), n_classes), dtype=np.int64)
    for pl, pd, gl, gd in pairs:
        keep = gl != free_id
        pl, pd, gl, gd = pl[keep], pd[keep], gl[keep], gd[keep]
        err = np.abs(pd - gd)
        assert err.dtype == np.float32
        out[0] += np.bincount(gl[gl < n_classes], minlength=n_classes)
        out[1] += np.bincount(pl[pl < n_classes], minlength=n_classes)
        for j, thr in enumerate(thresholds):
            ok = (pl == gl) & (err < thr) & (gl < n_classes)
            out[2 + j] += np.bincount(gl[ok], minlength=n_classes)
    return out


def metrics(cnt, thresholds=(1, 2, 4)):
    c = cnt.astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        iou = (c[2:] / (c[0] + c[1] - c[2:]))[:, :-1]
        out = {'RayIoU': float(np.nanmean(iou))}
        for j, thr in enumerate(thresholds):
            out[f'RayIoU@{thr}'] = float(np.nanmean(iou[j]))
    return out, iou


def brute_force(occ, origin, points):
    """Independent check of cast(): no stepping.  For every occupied voxel and every ray the slab test gives the entry and exit
    parameters; the hit is the occupied voxel of smallest entry.  For small grids (memory: rays x occupied voxels).
    -> hit (M,) bool, coord (M,3), exit (M,) float64, margin (M,) = gap between the two smallest entries."""
    o = np.asarray(origin, dtype=np.float32).astype(np.float64)
    e = np.asarray(points, dtype=np.float32).astype(np.float64)
    r = e - o[None]
    d = r / np.sqrt((r * r).sum(1))[:, None]
    vox = np.argwhere(occ)
    lo = vox.astype(np.float64)[None] - o[None, None]          # (1,V,3): slab faces relative to the origin
    hi = lo + 1.0
    with np.errstate(all='ignore'):
        dd = d[:, None, :]
        t0, t1 = lo / dd, hi / dd
        near, far = np.minimum(t0, t1), np.maximum(t0, t1)
        # a ray parallel to an axis is inside that slab for every parameter or for none
        within = (lo <= 0) & (hi > 0)
        near = np.where(dd == 0, np.where(within, -np.inf, np.inf), near).max(2)
        far = np.where(dd == 0, np.where(within, np.inf, -np.inf), far).min(2)
    near = np.where((near < far) & (far > 0), near, np.inf)
    two = np.sort(near, axis=1)[:, :2]
    k = near.argmin(1)
    rows = np.arange(e.shape[0])
    with np.errstate(invalid='ignore'):
        margin = np.where(np.isfinite(two[:, 1]), two[:, 1] - two[:, 0], np.inf)
    return np.isfinite(two[:, 0]), vox[k], far[rows, k], margin
