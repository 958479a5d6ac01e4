"""RayIoU at the Occ3D size: S = 4 samples, T = 8 float64 lidar origins each, 14 040 rays, prediction and ground-truth grid.
45 add_batch calls (20 of them between device events) and 10 render_forward calls of one origin; run it under
`rocprofv3 --kernel-trace --stats` for the kernel times (profiles/r8/ray_iou.txt).  --steps: also count the traversal's loop
iterations for the same inputs with the float64 twin (tests/rayiou_twin.py; about two minutes of CPU time)."""
import json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dhd_amd
import rayiou_twin as twin

def scene(seed):
    rng = np.random.RandomState(seed)
    gt = np.full((200, 200, 16), 17, np.uint8); gt[:, :, :2] = 11
    cl = rng.rand(200, 200, 16) < 0.01; gt[cl] = rng.randint(0, 17, int(cl.sum()))
    for _ in range(30):
        x, y = rng.randint(0, 180, 2); gt[x:x + rng.randint(2, 20), y:y + rng.randint(2, 20), 2:rng.randint(4, 12)] = rng.randint(0, 17)
    pred = gt.copy(); nz = rng.rand(200, 200, 16) < 0.015; pred[nz] = rng.randint(0, 18, int(nz.sum()))
    return pred, gt

S, T = 4, 8
dev = torch.device('cuda', 0)
sc = [scene(s) for s in range(S)]
pred = torch.from_numpy(np.stack([p for p, _ in sc])).to(dev); gt = torch.from_numpy(np.stack([g for _, g in sc])).to(dev)
rng = np.random.RandomState(5)
org = np.array([0.9858, 0.0, 1.8402]) + np.concatenate([rng.uniform(-4, 4, (S * T, 2)), rng.uniform(-0.05, 0.05, (S * T, 1))], 1)
origins = [org[s * T:(s + 1) * T] for s in range(S)]
m = dhd_amd.RayIoU()
for _ in range(25):
    m.add_batch(pred, gt, origins)
torch.cuda.synchronize()
ev = []
for _ in range(20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); m.add_batch(pred, gt, origins); e1.record(); torch.cuda.synchronize(); ev.append(e0.elapsed_time(e1))
# the seam-level caster on the same rays of sample 0 / origin 0
rays = dhd_amd.generate_lidar_rays()
o, e = twin.to_voxel_units(org[0], rays, (-40.0, -40.0, -1.0), 0.4)
sigma = (gt[0] < 17).permute(2, 1, 0).float()[None, None].contiguous()
for _ in range(10):
    dhd_amd.render_forward(sigma, torch.from_numpy(o)[None, None].to(dev), torch.from_numpy(e)[None].to(dev), torch.zeros(1, len(rays), device=dev), [1, 16, 200, 200], 'test')
torch.cuda.synchronize()
steps = 0
if '--steps' in sys.argv:
    for s in range(S):
        for sem in sc[s]:
            steps += twin.sample(sem, origins[s], rays)[2]
print(json.dumps(dict(S=S, T=T, rays=len(rays), add_batch_event_ms_median=float(np.median(ev)), add_batch_event_ms_min=float(min(ev)),
                      twin_loop_iterations_all=int(steps), device=torch.cuda.get_device_name(0))))
