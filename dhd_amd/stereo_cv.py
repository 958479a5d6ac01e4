"""The temporal-stereo cost volume of DepthNet from the camera matrices (csrc/stereo_cv.h, capi_stereo/dhd_amd_stereo_cv.h):

  stereo_sampling_grid   the (BN, D H, W, 2) float32 sampling grid of `gen_grid` in one launch, bit for bit
  stereo_cost_volume     gen_grid + `_hip_cost_volume` in one operator: lane l of a wave evaluates the position of hypothesis
                         d0 + l from the view's matrices, the feature maps are read in their own type (float32, float16,
                         bfloat16) where they lie when their memory is NHWC, and the result is written in that type.  Neither
                         the grid nor a float32 / NHWC copy of the features exists.

float32 results are today's bytes (same positions, same tap order, same reduction tree, same softmax).  Half results are within
1e-4 + 2 eps |ref| of today's path on the same half tensors: both see the same float32 values and the same rounded positions, a
lane sums 8 channels where today's sums 4, and the result is rounded once.  `_LiftNetBase.fused_cost_volume` is opt-in and routed
by measurement (ROUTED).  The entry points are reached through _stereo_cv.call(name, ...) / _stereo_cv.value(name, ...)."""
import weakref

import torch

from . import _lib, _stereo_cv
from .trace import traced

_F32, _F16, _BF16 = torch.float32, torch.float16, torch.bfloat16

# Which (channel class, dtype) entries `calculate_cost_volumn` routes to the operator: those where the whole fused path, from the
# metas to the cost volume, beat the whole of today's path by more than the larger min-max spread of the two
# (experiments/stereo_cv_bench.py -> profiles/r28/stereo_cv.json).  The channel class is the kernel family a channel count takes:
# 'c128' up to 128 channels, 'c256' up to 256, 'c512' up to 512, 'c1024' above.  An entry that was not measured is False and stays
# with today's path; the operator itself still takes it when called directly.  12 views, D = 88, medians in us per call, fused
# against today's whole path, dense NCHW maps | channels_last maps (the larger spread in brackets), and the kernels alone:
#   c128 (DHD-L, 128 @ 128 x 352):  float32 4700 / 11875 (78) | 4438 / 12391 (141), kernels 4193 / 4153 (262): a tie
#                                   bf16    4118 / 12200 (81) | 3971 / 12729 (76),  kernels 3786 / 4031 (151)
#                                   fp16    4202 / 12193 (73) | 4052 / 12723 (75),  kernels 3911 / 4098 (187)
#   c256 (DHD-M, 256 @ 64 x 176):   float32 2091 / 3670 (70)  | 1958 / 3937 (58),   kernels 1716 / 1686 (7): a loss of 30 us
#                                   bf16    1743 / 3770 (64)  | 1679 / 4027 (51),   kernels 1402 / 1679 (11)
#                                   fp16    1756 / 3736 (67)  | 1689 / 4016 (82),   kernels 1445 / 1680 (14)
# The whole path wins everywhere it was measured: what it saves is gen_grid's launches and the copies, not tap bytes.
ROUTED = {(cls, dt): False for cls in ('c128', 'c256', 'c512', 'c1024') for dt in (_F32, _F16, _BF16)}
for _cls in ('c128', 'c256'):
    for _dt in (_F32, _F16, _BF16):
        ROUTED[(_cls, _dt)] = True
del _cls, _dt


def channel_class(c):
    return 'c128' if c <= 128 else 'c256' if c <= 256 else 'c512' if c <= 512 else 'c1024'


def stereo_cv_routed(c, dtype):
    """True when the measurement routed this (channel class, dtype) to the operator (ROUTED)."""
    return bool(ROUTED.get((channel_class(c), dtype), False))


_axes_cache = {}     # id(frustum) -> (weakref, version, axes or None)


def frustum_axes(frustum):
    """(u, v, dep) float32 axis vectors of a separable (D, H, W, 3) frustum template -- frustum[d, y, x] == (u[x], v[y], dep[d]),
    what `create_frustum` builds -- or None where it is not separable.  Checked once per frustum object (one host
    synchronisation, so an object first seen while a HIP graph is being captured counts as not separable)."""
    if not (torch.is_tensor(frustum) and frustum.dim() == 4 and frustum.shape[-1] == 3 and frustum.numel() > 0):
        return None
    hit = _axes_cache.get(id(frustum))
    if hit is not None and hit[0]() is frustum and hit[1] == frustum._version:
        return hit[2]
    if frustum.is_cuda and torch.cuda.is_current_stream_capturing():
        return None
    u, v, dep = frustum[0, 0, :, 0], frustum[0, :, 0, 1], frustum[:, 0, 0, 2]
    D, H, W, _ = frustum.shape
    same = (torch.equal(frustum[..., 0], u.view(1, 1, W).expand(D, H, W)) and torch.equal(frustum[..., 1], v.view(1, H, 1).expand(D, H, W))
            and torch.equal(frustum[..., 2], dep.view(D, 1, 1).expand(D, H, W)))
    axes = tuple(a.float().contiguous() for a in (u, v, dep)) if same else None
    key = id(frustum)
    _axes_cache[key] = (weakref.ref(frustum, lambda _, key=key: _axes_cache.pop(key, None)), frustum._version, axes)
    return axes


def _view_arrays(post_rots, post_trans, intrins, k2s_sensor):
    """The six float32 view arrays of the C surface, from the expressions of `gen_grid` (so under autocast `combine` is the same
    rounded product gen_grid multiplies with), on (B, N, 3, 3) tensors: capturable."""
    from .detector import small_inverse   # torch.inverse, or a closed form while a HIP graph is being captured
    inv_post = small_inverse(post_rots)
    rots = k2s_sensor[:, :, :3, :3].contiguous()
    trans = k2s_sensor[:, :, :3, 3].contiguous()
    combine = rots.matmul(small_inverse(intrins))
    return tuple(t.float().contiguous() for t in (inv_post, post_trans, combine, trans, intrins, post_rots))


def _metas_ok(*metas):
    return all(torch.is_tensor(t) and t.is_cuda and t.dtype == _F32 for t in metas)


def stereo_sampling_grid(frustum, post_rots, post_trans, intrins, k2s_sensor, hi, wi):
    """`DepthNet.gen_grid` in one launch: the (B N, D H, W, 2) float32 sampling grid of the stereo frustum `frustum` (D, H, W, 3;
    separable, any float dtype) in the adjacent frame's image of hi x wi pixels, bit for bit what gen_grid returns on the device.
    post_rots, intrins (B, N, 3, 3), post_trans (B, N, 3), k2s_sensor (B, N, 4, 4): float32 GPU tensors."""
    if not _metas_ok(post_rots, post_trans, intrins, k2s_sensor) or not (torch.is_tensor(frustum) and frustum.is_cuda):
        raise _lib.DhdError('stereo_sampling_grid: float32 calibration tensors and a frustum on the GPU: dhd_amd runs only as HIP kernels')
    axes = frustum_axes(frustum)
    if axes is None:
        raise _lib.DhdError('stereo_sampling_grid: the frustum template is not separable into (u, v, depth) axes')
    return _grid(axes, _view_arrays(post_rots, post_trans, intrins, k2s_sensor), frustum.shape, hi, wi)


@traced('dhd.stereo_cv.grid')
def _grid(axes, views, fshape, hi, wi):
    D, H, W, _ = fshape
    bn = views[0].shape[0] * views[0].shape[1]
    dev = views[0].device
    with torch.cuda.device(dev):
        grid = torch.empty((bn, D * H, W, 2), dtype=_F32, device=dev)
        _stereo_cv.call('dhdv_stereo_grid', *[_lib.ptr(t) for t in views], *[_lib.ptr(a) for a in axes], _lib.ptr(grid), bn, H, W, D,
                        int(hi), int(wi), _lib.stream_ptr(dev))
    return grid


def stereo_cv_supported(prev, curr, frustum, post_rots, post_trans, intrins, k2s_sensor):
    """True when `stereo_cost_volume` takes the call: prev, curr (B N, C, H, W) GPU maps of one dtype (float32, float16 or
    bfloat16) with C a multiple of 8 (of 4 in float32) up to 1024; a separable (D, H, W, 3) frustum with D <= 256; float32
    calibration tensors on the GPU; fewer than 2^31 cost cells."""
    if not (torch.is_tensor(prev) and torch.is_tensor(curr) and prev.is_cuda and curr.is_cuda and curr.dim() == 4
            and prev.shape == curr.shape and prev.dtype == curr.dtype and curr.dtype in _lib.DTYPE_CODE and curr.numel() > 0):
        return False
    if not _metas_ok(post_rots, post_trans, intrins, k2s_sensor) or not (torch.is_tensor(frustum) and frustum.is_cuda and frustum.dim() == 4):
        return False
    bn, c, h, w = curr.shape
    D, H, W, _ = frustum.shape
    if (H, W) != (h, w) or post_trans.shape[0] * post_trans.shape[1] != bn:
        return False
    if not _stereo_cv.value('dhdv_stereo_cv_supported', _lib.DTYPE_CODE[curr.dtype], bn, c, h, w, D):
        return False
    return frustum_axes(frustum) is not None


def _nhwc_in_place(x):
    """True where the kernels can read the (bn, c, h, w) map where it lies: its memory is dense [bn][h][w][c], 16-byte aligned."""
    return x.permute(0, 2, 3, 1).is_contiguous() and x.data_ptr() % 16 == 0


def _features(prev, curr):
    """-> prev, curr, layout code.  Both maps with NHWC memory: read in place.  Otherwise dense NCHW, which the entry point
    re-lays once in the maps' own type; any other view gets .contiguous() (and a copy where it is misaligned) first."""
    if _nhwc_in_place(prev) and _nhwc_in_place(curr):
        return prev, curr, _stereo_cv.NHWC
    return _lib.dense16(prev), _lib.dense16(curr), _stereo_cv.NCHW


@traced('dhd.stereo_cv')
def _cost_volume(prev, curr, axes, views, D, hi, wi, bias, flag_channel):
    prev, curr, layout = _features(prev.detach(), curr.detach())
    bn, c, h, w = curr.shape
    dev = curr.device
    code = _lib.dtype_code(curr.dtype)
    with torch.cuda.device(dev):
        out = torch.empty((bn, D, h, w), dtype=curr.dtype, device=dev)
        nbytes = _stereo_cv.value('dhdv_stereo_cv_scratch_bytes', code, layout, bn, c, h, w)
        # the re-laid pair is a tensor of this call, not pooled scratch: 277 MB at the DHD-L size, and a pool keeps one per stream for
        # the life of the process (measured: + 1.68 GB at the peak of a captured DHD-L step), where today's copies are freed at once
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        _stereo_cv.call('dhdv_stereo_cost_volume', _lib.ptr(prev), _lib.ptr(curr), _lib.ptr(out), code, layout, *[_lib.ptr(t) for t in views],
                        *[_lib.ptr(a) for a in axes], bn, c, h, w, D, int(hi), int(wi), float(bias), int(flag_channel), _lib.ptr(scratch),
                        nbytes, _lib.stream_ptr(dev))
    return out


def stereo_cost_volume(prev, curr, frustum, post_rots, post_trans, intrins, k2s_sensor, bias, flag_channel):
    """softmax over the D hypotheses of -cost, cost[n, d, y, x] = sum_c |curr[n, c, y, x] - sample(prev[n, c], position)| (+ bias
    where the sample of channel `flag_channel` is exactly 0), the position of hypothesis d at pixel (y, x) being gen_grid's for an
    adjacent image of (4 H, 4 W) pixels, rounded once through the features' dtype: what `calculate_cost_volumn` computes through
    gen_grid and `_hip_cost_volume`, as one operator, (B N, D, H, W) in the features' dtype.  prev, curr: (B N, C, H, W) GPU maps of
    float32, float16 or bfloat16; channels_last tensors and permuted views with NHWC memory are read where they lie, dense NCHW
    maps are re-laid once in their own type into a scratch tensor of the call.  No gradient (the cost volume is computed under no_grad).  No
    atomics: two calls give the same bytes.  Works under graph capture once the frustum object has been seen."""
    for name, t in (('prev', prev), ('curr', curr)):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.DhdError(f'stereo_cost_volume: {name} must live on the GPU: dhd_amd runs only as HIP kernels '
                                f'(got {getattr(t, "device", type(t))})')
    if not stereo_cv_supported(prev, curr, frustum, post_rots, post_trans, intrins, k2s_sensor):
        raise _lib.DhdError(f'stereo_cost_volume: no operator for maps {tuple(prev.shape)} of {prev.dtype} / {tuple(curr.shape)} of '
                            f'{curr.dtype} with a frustum {tuple(frustum.shape)} (see stereo_cv_supported)')
    h, w = curr.shape[2:]
    return _cost_volume(prev, curr, frustum_axes(frustum), _view_arrays(post_rots, post_trans, intrins, k2s_sensor), frustum.shape[0],
                        h * 4, w * 4, bias, flag_channel)


def module_cost_volume(net, metas, prev, curr, D, hi, wi, flag_channel):
    """What `calculate_cost_volumn` does with `fused_cost_volume` on: the operator where the call is supported and routed; the grid
    kernel in place of gen_grid's torch chain, feeding today's kernel, where only the feature shape is not supported; None (today's
    code) otherwise."""
    cal = (metas['post_rots'], metas['post_trans'], metas['intrins'], metas['k2s_sensor'])
    frustum = metas['frustum']
    if not (_metas_ok(*cal) and torch.is_tensor(frustum) and frustum.is_cuda and frustum.dim() == 4 and tuple(frustum.shape[1:3]) == tuple(curr.shape[2:])):
        return None
    axes = frustum_axes(frustum)
    if axes is None:
        return None
    if stereo_cv_supported(prev, curr, frustum, *cal):
        if not stereo_cv_routed(curr.shape[1], curr.dtype):
            return None
        return _cost_volume(prev, curr, axes, _view_arrays(*cal), D, hi, wi, net.bias, flag_channel)
    if D > _stereo_cv.MAX_D or curr.shape[0] * D * curr.shape[2] * curr.shape[3] >= 2 ** 31:
        return None
    grid = _grid(axes, _view_arrays(*cal), frustum.shape, hi, wi).to(curr.dtype)
    return net._hip_cost_volume(prev, curr, grid, D, flag_channel)
