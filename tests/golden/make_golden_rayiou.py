"""Golden G19: RayIoU as the reference's own Python computes it (projects/mmdet3d_plugin/core/evaluation/ray_metrics.py:
generate_lidar_rays, process_one_sample, main), run on the CPU.  Its CUDA half (lib/dvr/dvr.cu, JIT-compiled with nvcc at
import) cannot run here, so torch.utils.cpp_extension.load is replaced by an object whose render_forward is the float64
restatement in tests/rayiou_twin.py; prettytable (not installed) is stubbed and Tensor.cuda is the identity.

    python tests/golden/make_golden_rayiou.py [reference root]     -> tests/golden/g19_rayiou.npz

Runs only where the reference checkout exists; the fixture it writes is data (ray set, scenes, origins, per-ray results,
counters, the final dict).  Scenes are stored as the ground-truth grid plus the voxels where the prediction differs."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rayiou_twin as twin  # noqa: E402

GRID = (200, 200, 16)
FREE = 17


class _Dvr:
    @staticmethod
    def render_forward(sigma, origin, points, tindex, grid, phase):
        assert phase == 'test' and sigma.shape[:2] == (1, 1) and origin.shape == (1, 1, 3) and float(tindex.abs().max()) == 0
        occ = sigma[0, 0].permute(2, 1, 0).numpy() > 0.5
        c = twin.cast(occ, origin[0, 0].numpy(), points[0].numpy())
        e = c['entered']
        r = points[0].numpy().astype(np.float64) - origin[0, 0].numpy().astype(np.float64)
        gt = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2])
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32)))[None]
        return f(np.where(e, c['dist'], -1.0)), f(np.where(e, gt, -1.0)), f(np.where(e[:, None], c['coord'], 0))


class _Table:
    def __init__(self, *a, **k):
        self.rows = []

    def add_row(self, row, **k):
        self.rows.append(row)

    def __str__(self):
        return '\n'.join(str(r) for r in self.rows)


def load_reference(root):
    import torch.utils.cpp_extension as ext
    ext.load = lambda *a, **k: _Dvr
    sys.modules['prettytable'] = types.SimpleNamespace(PrettyTable=_Table)
    torch.Tensor.cuda = lambda self, *a, **k: self
    path = os.path.join(root, 'projects', 'mmdet3d_plugin', 'core', 'evaluation', 'ray_metrics.py')
    spec = importlib.util.spec_from_file_location('reference_ray_metrics', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_scene(seed):
    """Ground plane, ~1 % clutter, and a prediction that differs from the ground truth in ~1.5 % of the voxels."""
    rng = np.random.RandomState(seed)
    gt = np.full(GRID, FREE, dtype=np.uint8)
    gt[:, :, :2] = 11
    gt[60:140, 90:110, 1] = 13
    clutter = rng.rand(*GRID) < 0.01
    gt[clutter] = rng.randint(0, 17, size=int(clutter.sum()))
    pred = gt.copy()
    noise = rng.rand(*GRID) < 0.015
    pred[noise] = rng.randint(0, 18, size=int(noise.sum()))
    return pred, gt


# per sample: dtype of the origin tensor, origins (metres)
SAMPLES = [
    (np.float64, [[0.9858, 0.0, 1.8402],          # the nuScenes lidar: y lands exactly on a voxel face
                  [2.1, -3.3, 0.9]]),            # quarter-voxel position: exact tMax ties on diagonal rays
    (np.float64, [[-10.3, 5.7, 7.0],              # above the grid: enters from outside
                  [4.0, 4.0, -1.0 + 0.4 * 316]]),  # 300 voxels above it: runs out of steps, never enters
    (np.float32, [[0.9858, 0.0, 1.8402],
                  [-6.1, 8.5, 0.5]]),
]


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    ref = load_reference(root)
    rays = ref.generate_lidar_rays()
    out = {'rays': rays}
    preds, gts, origins = [], [], []
    for i, (dt, org) in enumerate(SAMPLES):
        pred, gt = make_scene(100 + i)
        o = torch.from_numpy(np.asarray(org, dtype=dt)[None])
        preds.append(pred.reshape(-1)); gts.append(gt); origins.append(o)
        out[f'gt{i}'] = gt
        diff = np.flatnonzero(pred.reshape(-1) != gt.reshape(-1)).astype(np.int32)
        out[f'pred{i}_index'], out[f'pred{i}_value'] = diff, pred.reshape(-1)[diff]
        out[f'origins{i}'] = o.numpy()
        rt = torch.from_numpy(rays)
        pp, pg = ref.process_one_sample(pred, rt, o), ref.process_one_sample(gt, rt, o)
        assert pp.dtype == np.float32 and pp.shape == (len(org) * len(rays), 2)
        out[f'label{i}'] = np.stack([pg[:, 0], pp[:, 0]], 1).astype(np.uint8)      # columns: ground truth, prediction
        out[f'dist{i}'] = np.stack([pg[:, 1], pp[:, 1]], 1)
    res = ref.main(preds, gts, origins)
    cnt = twin.counters((out[f'label{i}'][:, 1].astype(np.int64), out[f'dist{i}'][:, 1], out[f'label{i}'][:, 0].astype(np.int64),
                         out[f'dist{i}'][:, 0]) for i in range(len(SAMPLES)))
    mine, _ = twin.metrics(cnt)
    for k, v in res.items():
        assert abs(mine[k] - v) < 1e-12, (k, mine[k], v)     # the counters below are the ones behind the reference's dict
        out['result_' + k] = np.float64(v)
    out['counts'] = cnt
    path = os.path.join(HERE, 'g19_rayiou.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes', res)


if __name__ == '__main__':
    main()
