"""RayIoU (core/evaluation/ray_metrics.py of the reference) on the MI355X: the voxel ray caster the reference JIT-compiles
from lib/dvr/dvr.cu, and the metric's counters, as HIP kernels (csrc/ray_iou.hip).

    render_forward(...)    the reference's dvr.render_forward: bind it in place of the JIT module
    RayIoU                 the metric as an accumulator: add_batch() per step, counts on the device, count() at the end
    calc_rayiou(...)       ray_metrics.main under the name datasets/nuscenes_dataset_occ.py imports it by

There is no CPU path: without a GPU every entry point that casts a ray raises DhdError."""
import ctypes as C
import math
import warnings

import numpy as np
import torch

from . import _lib
from .trace import traced

OCC_CLASS_NAMES = ('others', 'barrier', 'bicycle', 'bus', 'car', 'construction_vehicle', 'motorcycle', 'pedestrian',
                   'traffic_cone', 'trailer', 'truck', 'driveable_surface', 'other_flat', 'sidewalk', 'terrain', 'manmade',
                   'vegetation', 'free')
PC_RANGE = (-40.0, -40.0, -1.0, 40.0, 40.0, 5.4)
VOXEL_SIZE = 0.4


def generate_lidar_rays():
    """(14040, 3) float32 unit vectors: 39 pitch rings x 360 azimuths (ray_metrics.py:56-79; the ten lowest rings look at
    ground distances 1..10 lidar heights, the rest continue with the last spacing until past the upper edge of the nuScenes
    lidar's field of view, 0.21 rad).  Evaluated value by value in float64 as the reference does, so the float32 results
    are its bits."""
    pitch = [-(math.pi / 2 - math.atan(k + 1)) for k in range(10)]
    while pitch[-1] < 0.21:
        pitch.append(pitch[-1] + (pitch[-1] - pitch[-2]))
    out = np.empty((len(pitch), 360, 3), dtype=np.float32)
    for i, p in enumerate(pitch):
        for j, deg in enumerate(np.arange(0, 360, 1)):
            az = np.deg2rad(deg)
            out[i, j] = (np.cos(p) * np.cos(az), np.cos(p) * np.sin(az), np.sin(p))
    return out.reshape(-1, 3)


def _gpu():
    if not torch.cuda.is_available():
        raise _lib.DhdError('ray casting runs only as a HIP kernel on the GPU, and none is available (there is no CPU path)')
    return torch.device('cuda', torch.cuda.current_device())


@traced('dhd.ray_render_forward')
def render_forward(sigma, origin, points, tindex, grid=None, phase='test'):
    """dvr.render_forward of the reference (lib/dvr/dvr.cu:329-388): sigma (N,T,Z,Y,X), origin (N,T',3) and points (N,M,3) in
    voxel units, tindex (N,M) -> (pred_dist (N,M), gt_dist (N,M), coord_index (N,M,3)), float32 on sigma's device.
    `grid` = [T, Z, Y, X] is accepted for the signature's sake and checked against sigma; phase 'train' is refused."""
    if phase not in _lib.RAY_PHASE:
        raise _lib.DhdError(f'render_forward: unknown phase {phase!r}')
    for name, t in (('sigma', sigma), ('origin', origin), ('points', points), ('tindex', tindex)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.DhdError(f'render_forward: {name} must be a GPU tensor (there is no CPU path)')
    if sigma.dim() != 5 or origin.dim() != 3 or points.dim() != 3 or tindex.dim() != 2 or origin.shape[2] != 3 or points.shape[2] < 3:
        raise _lib.DhdError('render_forward: expected sigma (N,T,Z,Y,X), origin (N,T,3), points (N,M,3), tindex (N,M)')
    n, t_sigma, nz, ny, nx = sigma.shape
    m = points.shape[1]
    if origin.shape[0] != n or points.shape[0] != n or tuple(tindex.shape) != (n, m):
        raise _lib.DhdError('render_forward: inconsistent batch / ray counts')
    if grid is not None and tuple(int(g) for g in grid)[1:] != (nz, ny, nx):
        raise _lib.DhdError(f'render_forward: grid {list(grid)} does not describe sigma {tuple(sigma.shape)}')
    dev = sigma.device
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    sigma, origin, points, tindex = f(sigma), f(origin), f(points[..., :3]), f(tindex)
    with torch.cuda.device(dev):
        pred_dist = torch.empty(n, m, dtype=torch.float32, device=dev)
        gt_dist = torch.empty(n, m, dtype=torch.float32, device=dev)
        coord = torch.empty(n, m, 3, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().dhd_ray_render_forward(_lib.ptr(sigma), _lib.ptr(origin), _lib.ptr(points), _lib.ptr(tindex), n, t_sigma,
                                                      origin.shape[1], m, nz, ny, nx, _lib.RAY_PHASE[phase], _lib.ptr(pred_dist),
                                                      _lib.ptr(gt_dist), _lib.ptr(coord), _lib.stream_ptr(dev)),
                   'dhd_ray_render_forward')
    return pred_dist, gt_dist, coord


def _key(thr):
    return f'RayIoU@{int(thr) if float(thr).is_integer() else thr}'


class RayIoU:
    """The metric as an accumulator, like the mIoU histogram of occ_argmax_hist: `counts` is a device int64 tensor
    (2 + len(thresholds), n_classes) = gt_cnt | pred_cnt | tp_cnt[j] that add_batch() adds into and that can be summed across
    ranks; nothing per ray leaves the kernel and nothing reaches the host before count()."""

    def __init__(self, pc_range=PC_RANGE, voxel_size=VOXEL_SIZE, class_names=OCC_CLASS_NAMES, thresholds=(1, 2, 4), device=None):
        self.pc_range = tuple(float(v) for v in pc_range)
        self.voxel_size = float(voxel_size)
        self.class_names = tuple(class_names)
        self.thresholds = tuple(thresholds)
        self.grid = tuple(int(round((self.pc_range[3 + a] - self.pc_range[a]) / self.voxel_size)) for a in range(3))
        self.n_classes = len(self.class_names)
        self.free_id = self.n_classes - 1
        self.device = torch.device(device) if device is not None else None
        self.counts = None
        self._rays = None

    def _setup(self, dev):
        if self.counts is None:
            lib = _lib.load()
            if not lib.dhd_ray_iou_supported(*self.grid, self.n_classes, len(self.thresholds)):
                raise _lib.DhdError(f'RayIoU: grid {self.grid}, {self.n_classes} classes, {len(self.thresholds)} thresholds: '
                                    + _lib._ERRORS[-3])
            self.device = dev
            self.counts = torch.zeros(2 + len(self.thresholds), self.n_classes, dtype=torch.int64, device=dev)
            self._rays = torch.from_numpy(generate_lidar_rays()).to(dev)
        elif dev != self.device:
            raise _lib.DhdError(f'RayIoU: counters live on {self.device}, this batch on {dev}')

    def _grids(self, sem, name):
        """-> (S, nx, ny, nz) uint8 on the device; a device uint8 tensor is used where it is."""
        cells = self.grid[0] * self.grid[1] * self.grid[2]
        if not isinstance(sem, torch.Tensor):
            sem = np.asarray(sem)
            if sem.dtype == object or (sem.ndim >= 1 and sem.size % cells):
                raise _lib.DhdError(f'RayIoU: {name} does not hold whole {self.grid} grids')
            sem = torch.from_numpy(np.ascontiguousarray(sem.astype(np.uint8, copy=False)))
        if sem.numel() == 0 or sem.numel() % cells:
            raise _lib.DhdError(f'RayIoU: {name} does not hold whole {self.grid} grids')
        if sem.dtype != torch.uint8:
            sem = sem.to(torch.uint8)
        return sem.to(self.device).contiguous().view(-1, *self.grid)

    @staticmethod
    def _origins(o):
        """One sample's origins (T,3) or (1,T,3), numpy or torch, float32 or float64 -> numpy (T,3) of that dtype."""
        o = o.detach().cpu().numpy() if isinstance(o, torch.Tensor) else np.asarray(o)
        if o.dtype not in (np.float32, np.float64):
            raise _lib.DhdError(f'RayIoU: lidar origins must be float32 or float64, not {o.dtype}')
        if o.ndim == 3 and o.shape[0] == 1:
            o = o[0]
        if o.ndim != 2 or o.shape[1] != 3 or o.shape[0] == 0:
            raise _lib.DhdError(f'RayIoU: lidar origins of a sample are (T,3) or (1,T,3), got {o.shape}')
        return o

    @traced('dhd.ray_iou')
    def add_batch(self, sem_pred, sem_gt, lidar_origins):
        """sem_pred, sem_gt: class ids of one sample (nx,ny,nz) or a batch (S,nx,ny,nz) (flattened forms too), numpy or torch.
        lidar_origins: one sample: (T,3) / (1,T,3); a batch: a sequence of S such.  float64 origins take the reference's
        float64 arithmetic (what its dataset hands over), float32 origins its float32 arithmetic."""
        dev = self.device
        if isinstance(sem_pred, torch.Tensor) and sem_pred.is_cuda:
            dev = sem_pred.device
        elif dev is None:
            dev = _gpu()
        if dev.type != 'cuda' or not torch.cuda.is_available():
            raise _lib.DhdError('RayIoU runs only as a HIP kernel on the GPU (there is no CPU path)')
        self._setup(dev)
        pred, gt = self._grids(sem_pred, 'sem_pred'), self._grids(sem_gt, 'sem_gt')
        if pred.shape != gt.shape:
            raise _lib.DhdError(f'RayIoU: {pred.shape[0]} predictions, {gt.shape[0]} ground truths')
        s = pred.shape[0]
        if isinstance(lidar_origins, (list, tuple)) or (lidar_origins.ndim == 3 and s > 1):
            per_sample = [self._origins(o) for o in lidar_origins]     # a sequence, or an (S,T,3) array
        else:
            per_sample = [self._origins(lidar_origins)]
        if len(per_sample) != s:
            raise _lib.DhdError(f'RayIoU: {s} samples, origins for {len(per_sample)}')
        lib = _lib.load()
        lower = (C.c_float * 3)(*self.pc_range[:3])
        thr = (C.c_float * len(self.thresholds))(*self.thresholds)
        with torch.cuda.device(dev):
            for dt, flag in ((np.float64, _lib.RAY_ORIGIN_F64), (np.float32, 0)):
                ids = [i for i, o in enumerate(per_sample) for _ in range(len(o)) if o.dtype == dt]
                if not ids:
                    continue
                org = torch.from_numpy(np.concatenate([o for o in per_sample if o.dtype == dt])).to(dev)
                sid = torch.tensor(ids, dtype=torch.int32).to(dev)
                _lib.check(lib.dhd_ray_iou_accumulate(_lib.ptr(pred), _lib.ptr(gt), s, *self.grid, _lib.ptr(sid), _lib.ptr(org), len(ids),
                                                      flag, _lib.ptr(self._rays), self._rays.shape[0], lower, self.voxel_size,
                                                      self.free_id, self.n_classes, thr, len(self.thresholds),
                                                      _lib.ptr(self.counts), _lib.stream_ptr(dev)),
                           'dhd_ray_iou_accumulate')
        return self.counts

    def count(self):
        """ray_metrics.py:168-172,199-228: IoU_j = tp_j / (gt + pred - tp_j) over the classes but the last (free), RayIoU@j their
        nanmean, RayIoU the nanmean over all.  -> {'RayIoU', 'RayIoU@1', ..., 'per_class': (n_thresholds, n_classes - 1) array}."""
        if self.counts is None:
            raise _lib.DhdError('RayIoU.count(): nothing was added')
        c = self.counts.cpu().numpy().astype(np.float64)
        return metrics_from_counts(c, self.thresholds)


def metrics_from_counts(counts, thresholds=(1, 2, 4)):
    """Host arithmetic of the metric on a (2 + n_thresholds, n_classes) counter array (e.g. summed over ranks)."""
    c = np.asarray(counts, dtype=np.float64)
    gt, pred, tp = c[0], c[1], c[2:]
    with np.errstate(invalid='ignore', divide='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)       # nanmean of classes that never occur
        iou = (tp / (gt + pred - tp))[:, :-1]
        out = {'RayIoU': np.nanmean(iou)}
        for j, thr in enumerate(thresholds):
            out[_key(thr)] = np.nanmean(iou[j])
    out['per_class'] = iou
    return out


def calc_rayiou(sem_pred_list, sem_gt_list, lidar_origin_list, **kwargs):
    """ray_metrics.main: per-sample class grids and lidar origins -> {'RayIoU', 'RayIoU@1', 'RayIoU@2', 'RayIoU@4'}, with the
    per-class table printed.  Samples go to the device in batches of 8."""
    metric = RayIoU(**kwargs)
    n = len(sem_pred_list)
    if n == 0 or len(sem_gt_list) != n or len(lidar_origin_list) != n:
        raise _lib.DhdError('calc_rayiou: the three lists must have the same, non-zero length')
    _gpu()
    cells = metric.grid[0] * metric.grid[1] * metric.grid[2]
    flat = lambda seq: np.stack([np.asarray(g.cpu() if isinstance(g, torch.Tensor) else g).reshape(cells) for g in seq])
    for i in range(0, n, 8):
        metric.add_batch(flat(sem_pred_list[i:i + 8]), flat(sem_gt_list[i:i + 8]), list(lidar_origin_list[i:i + 8]))
    res = metric.count()
    table = res.pop('per_class')
    keys = [_key(t) for t in metric.thresholds]
    print(' | '.join(['class'.ljust(22)] + keys))
    for name, row in zip(metric.class_names[:-1], table.T):
        print(' | '.join([name.ljust(22)] + [f'{v:.3f}'.rjust(len(k)) for v, k in zip(row, keys)]))
    print(' | '.join(['MEAN'.ljust(22)] + [f'{res[k]:.3f}'.rjust(len(k)) for k in keys]))
    return res
