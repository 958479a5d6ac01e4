"""The stereo cost volume of the temporal DepthNet at the sizes DHD-L and DHD-M run it: the whole of today's path -- gen_grid's
torch chain, the (BN, D H, W, 2) grid, float32 and NHWC copies of both feature maps, dhd_stereo_cost_volume, the cast back --
against the whole fused path (dhd_amd/stereo_cv.py, csrc/stereo_cv.h), both from the metas to the cost volume through
`DepthNet.calculate_cost_volumn`, switch off and on.

Sizes: DHD-L, 12 views, c = 128, 128 x 352, D = 88, golden G16's calibration; DHD-M (dhd_m_model_cfg: 256 x 704 images, ResNet-50
stage-1 features), 12 views, c = 256, 64 x 176, D = 88, the same calibration with the image resize halved.  Dtypes: float32,
bfloat16, float16 feature maps (what the backbone hands over under autocast).  Layouts: dense NCHW maps (the operator re-lays them
once in their own type) and channels_last maps (read in place).

Protocol (that of experiments/unet_seam_bench.py): one process, the same tensors, the two paths in alternating windows of
`--calls` calls between device events, median / min / max us per call over `--windows` windows.  `wins`: the fused median beats
today's by more than the larger min-max spread of the two.  `kernel_only`: dhd_stereo_cost_volume on a prepared float32 NHWC pair
and grid against dhdv_stereo_cost_volume on prepared channels_last maps and view arrays.  `peak_bytes`: what one warmed call holds
at its peak on top of what was allocated before it.  `max_abs_diff`: between the two results at full size; `positions_that_differ`:
32-bit words of stereo_sampling_grid that are not gen_grid's (must be 0).

One JSON record (--out).  Needs a GPU: no fallback.

    python experiments/stereo_cv_bench.py --out profiles/r28/stereo_cv.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_ffn_infer_bench as NB  # noqa: E402  (puts the repository root on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dhd_amd  # noqa: E402
from dhd_amd import _lib, _stereo_cv, mghs_op, stereo_cv  # noqa: E402
from dhd_amd.depthnet import DepthNet  # noqa: E402
from dhd_amd.lss_heightmap import MGHS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NAME = {F32: 'float32', F16: 'float16', BF16: 'bfloat16'}
SIZES = {'dhd-l': dict(c=128, input_size=(512, 1408), resize=1.0), 'dhd-m': dict(c=256, input_size=(256, 704), resize=0.5)}
DEPTH = (1.0, 45.0, 0.5)
BIAS = 5.0


def make_metas(size, dev):
    import types
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'g16_stereo_dhdl.npz')) as g:
        cal = {k: torch.from_numpy(g[k].copy()) for k in ('k2s_sensor', 'intrins', 'post_rots', 'post_trans')}
    s = SIZES[size]['resize']
    cal['post_rots'][..., :2, :] *= s
    cal['post_trans'][..., :2] *= s
    frustum = MGHS.create_frustum(types.SimpleNamespace(sid=False), DEPTH, SIZES[size]['input_size'], 4).contiguous()
    metas = {k: v.to(dev) for k, v in cal.items()}
    metas['frustum'] = frustum.to(dev)
    return metas


def measure(paths, calls, windows):
    for fn in paths.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(windows):
        for k, fn in paths.items():
            times[k].append(NB.window(fn, calls))
    rec = {k: NB.summary(ts) for k, ts in times.items()}
    spread = max(rec[k]['max_us'] - rec[k]['min_us'] for k in paths)
    rec['larger_spread_us'] = round(spread, 1)
    rec['speedup'] = round(rec['today']['median_us'] / rec['fused']['median_us'], 2)
    rec['wins'] = bool(rec['today']['median_us'] - rec['fused']['median_us'] > spread)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--sizes', default='dhd-l,dhd-m')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda')
    record = {'protocol': f'12 views, D = 88; alternating windows of {args.calls} calls, {args.windows} windows, median / min / max us per call',
              'cases': [], 'routed': [], 'not_routed': []}
    stereo_cv.ROUTED.update({k: True for k in stereo_cv.ROUTED})       # the fused module path is what is being measured
    for size in args.sizes.split(','):
        metas = make_metas(size, dev)
        D, H, W, _ = metas['frustum'].shape
        B, N, _ = metas['post_trans'].shape
        c = SIZES[size]['c']
        cal = [metas[k] for k in ('post_rots', 'post_trans', 'intrins', 'k2s_sensor')]
        today_net, fused_net = (DepthNet(32, 32, 16, D, use_dcn=False, aspp_mid_channels=16, stereo=True, bias=BIAS) for _ in range(2))
        dhd_amd.fused_stereo_cost_volume(today_net, False)
        dhd_amd.fused_stereo_cost_volume(fused_net, True)
        ref_grid = today_net.gen_grid(metas, B, N, D, H, W, H * 4, W * 4)
        got_grid = dhd_amd.stereo_sampling_grid(metas['frustum'], *cal, H * 4, W * 4)
        differ = int((ref_grid.view(torch.int32) != got_grid.view(torch.int32)).sum())
        inside = float(((ref_grid >= -1) & (ref_grid <= 1)).all(-1).float().mean())
        del got_grid
        for dt in (F32, BF16, F16):
            torch.manual_seed(5)
            flag = (c // 4 - 1) * 4
            nchw = [(0.5 * torch.randn(B * N, c, H, W, device=dev)).to(dt) for _ in range(2)]
            rec = dict(size=size, dtype=NAME[dt], views=B * N, c=c, h=H, w=W, d=D, positions_that_differ=differ,
                       share_of_positions_inside=round(inside, 3))
            for layout in ('nchw', 'channels_last'):
                feats = nchw if layout == 'nchw' else [t.contiguous(memory_format=torch.channels_last) for t in nchw]
                m = dict(metas, cv_feat_list=feats)
                paths = {'today': lambda m=m: today_net.calculate_cost_volumn(m), 'fused': lambda m=m: fused_net.calculate_cost_volumn(m)}
                with torch.no_grad():
                    r = measure(paths, args.calls, args.windows)
                    r['peak_bytes'] = {k: NB.peak_bytes(fn) for k, fn in paths.items()}
                    a, b = paths['today'](), paths['fused']()
                    r['max_abs_diff'] = float((a.float() - b.float()).abs().max())
                    r['max_probability'] = float(a.float().max())
                    del a, b
                rec['whole_path_' + layout] = r
            # the kernels alone, on prepared operands
            prev32, curr32 = (mghs_op._nchw_to_nhwc(t.float().contiguous()) for t in nchw)
            grid = ref_grid.to(dt).float().contiguous()
            cl = [t.contiguous(memory_format=torch.channels_last) for t in nchw]
            views, axes = stereo_cv._view_arrays(*cal), stereo_cv.frustum_axes(metas['frustum'])
            out32 = torch.empty((B * N, D, H, W), dtype=F32, device=dev)
            out = torch.empty((B * N, D, H, W), dtype=dt, device=dev)
            lib, st = _lib.load(), _lib.stream_ptr(dev)

            def todays_kernel():
                _lib.check(lib.dhd_stereo_cost_volume(_lib.ptr(prev32), _lib.ptr(curr32), _lib.ptr(grid), B * N, c, H, W, D, BIAS, flag,
                                                      _lib.ptr(out32), st), 'dhd_stereo_cost_volume')

            def fused_kernel():
                _stereo_cv.call('dhdv_stereo_cost_volume', _lib.ptr(cl[0]), _lib.ptr(cl[1]), _lib.ptr(out), _lib.dtype_code(dt), _stereo_cv.NHWC,
                                *[_lib.ptr(t) for t in views], *[_lib.ptr(a) for a in axes], B * N, c, H, W, D, H * 4, W * 4, BIAS, flag,
                                None, 0, st)
            rec['kernel_only'] = measure({'today': todays_kernel, 'fused': fused_kernel}, args.calls, args.windows)
            rec['routed'] = bool(rec['whole_path_nchw']['wins'] and rec['whole_path_channels_last']['wins'])
            record['routed' if rec['routed'] else 'not_routed'].append([stereo_cv.channel_class(c), NAME[dt]])
            record['cases'].append(rec)
            print(json.dumps(rec), flush=True)
            del prev32, curr32, grid, cl, out32, out, nchw
            torch.cuda.empty_cache()
        del ref_grid, metas
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
