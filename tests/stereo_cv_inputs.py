"""Inputs of the stereo cost volume tests (a helper module, not a test): three calibrations derived from golden G8, frustum
templates from `create_frustum`, and seeded feature maps.  tests/test_stereo_cv_inputs.py holds, without a GPU, the conditions that
make them worth running: enough positions inside the adjacent image, enough behind its camera, some outside it."""
import math
import os
import types

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g8_stereo.npz')
INPUT_SIZE, DOWNSAMPLE = (32, 88), 4                       # stereo resolution 8 x 22, G8's
DEPTH_CFG = {12: (1.0, 45.0, 44.0 / 12), 65: (1.0, 66.0, 1.0), 70: (1.0, 36.0, 0.5), 88: (1.0, 45.0, 0.5), 130: (1.0, 66.0, 0.5)}
SMALL_INPUT_SIZE = (20, 28)                                # the 5 x 7 map
CALIBRATIONS = ('a', 'b', 'c')

_g8 = None


def g8():
    global _g8
    if _g8 is None:
        with np.load(GOLDEN) as f:
            _g8 = {k: f[k] for k in f.files}
    return _g8


def calibration(kind):
    """kind 'a': G8's as recorded.  'b': k2s_sensor[0, 1, 2, 3] -= 6, so the hypotheses nearer than ~6 m lie behind the adjacent
    camera of view 1.  'c': a horizontal flip and a 5 degree rotation about the image centre on top of G8's post_rots, with the
    post_trans that goes with it.  -> dict of float32 CPU tensors."""
    g = g8()
    cal = {k: g[k].copy() for k in ('k2s_sensor', 'intrins', 'post_rots', 'post_trans')}
    if kind == 'b':
        cal['k2s_sensor'][0, 1, 2, 3] -= 6.0
    elif kind == 'c':
        a = math.radians(5.0)
        rot = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]], np.float64)
        aug = np.eye(3)
        aug[:2, :2] = rot @ np.diag([-1.0, 1.0])
        centre = np.array([(INPUT_SIZE[1] - 1) / 2.0, (INPUT_SIZE[0] - 1) / 2.0, 0.0])
        shift = centre - aug @ centre
        for n in range(cal['post_rots'].shape[1]):
            pr, pt = cal['post_rots'][0, n].astype(np.float64), cal['post_trans'][0, n].astype(np.float64)
            cal['post_rots'][0, n] = (aug @ pr).astype(np.float32)
            cal['post_trans'][0, n] = (aug @ pt + shift).astype(np.float32)
    elif kind != 'a':
        raise ValueError(kind)
    return {k: torch.from_numpy(v) for k, v in cal.items()}


def frustum(n_depth, input_size=INPUT_SIZE):
    """(D, H, W, 3) float32 template of MGHS.create_frustum for the depth config that gives D = n_depth."""
    from dhd_amd.lss_heightmap import MGHS
    holder = types.SimpleNamespace(sid=False)
    f = MGHS.create_frustum(holder, DEPTH_CFG[n_depth], input_size, DOWNSAMPLE).contiguous()
    assert f.shape[0] == n_depth == holder.D
    return f


def metas(kind, n_depth, device='cpu', frustum_dtype=torch.float32, input_size=INPUT_SIZE):
    m = {k: v.to(device) for k, v in calibration(kind).items()}
    m['frustum'] = frustum(n_depth, input_size).to(device=device, dtype=frustum_dtype)
    return m


def features(c, h, w, dtype=torch.float32, bn=2, seed=0):
    """prev, curr (bn, c, h, w) CPU maps of `dtype`: normal values scaled so that the costs of the hypotheses stay comparable (a
    cost volume that is not one-hot)."""
    gen = torch.Generator().manual_seed(1000 * seed + c)
    scale = 16.0 / c
    return tuple((torch.randn(bn, c, h, w, generator=gen) * scale).to(dtype) for _ in range(2))


def depthnet(n_depth, bias):
    from dhd_amd.depthnet import DepthNet
    return DepthNet(32, 32, 16, n_depth, use_dcn=False, aspp_mid_channels=16, stereo=True, bias=bias)


def cpu_grid(m, hi=None, wi=None):
    """gen_grid on the CPU -> (B N, D, H, W, 2)."""
    B, N, _ = m['post_trans'].shape
    D, H, W, _ = m['frustum'].shape
    grid = depthnet(D, 0.0).gen_grid(m, B, N, D, H, W, hi or H * 4, wi or W * 4)
    return grid.view(B * N, D, H, W, 2)


def shares(grid):
    """-> (inside, marked, outside) shares of the positions of a (..., 2) grid: inside the image (both coordinates in [-1, 1]),
    carrying the behind-the-camera marker (-2, -2), and with all four bilinear taps outside an (H, W) map of any size (a pixel
    coordinate <= -1 or >= size: certain beyond |coordinate| > 1 + 2 / (size - 1), taken here at the 5-wide map's 1.5)."""
    g = grid.reshape(-1, 2)
    inside = ((g >= -1) & (g <= 1)).all(-1).float().mean().item()
    marked = (g == -2).all(-1).float().mean().item()
    outside = (g.abs() > 1.5).any(-1).float().mean().item()
    return inside, marked, outside


def separable(f):
    D, H, W, _ = f.shape
    u, v, d = f[0, 0, :, 0], f[0, :, 0, 1], f[:, 0, 0, 2]
    return (torch.equal(f[..., 0], u.view(1, 1, W).expand(D, H, W)) and torch.equal(f[..., 1], v.view(1, H, 1).expand(D, H, W))
            and torch.equal(f[..., 2], d.view(D, 1, 1).expand(D, H, W)))
