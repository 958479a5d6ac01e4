"""The seams of DHD-S's three voxel encoders (UNet, bilinear=False), 4 images: the operators of dhd_amd/unet_seam.py
(csrc/unet_seam.h) against today's calls, forward and forward + backward, at the UNet's own shapes in channels_last.

Pool: the inputs of the four `_Down`s, 64 @ 200 x 200, 128 @ 100 x 100, 256 @ 50 x 50, 512 @ 25 x 25; today's call is
F.max_pool2d(x, 2).  Up: the four `_Up`s, x1 1024 @ 12 x 12 / 512 @ 25 x 25 / 256 @ 50 x 50 / 128 @ 100 x 100 with the skip tensor
of half the channels at 25 / 50 / 100 / 200; today's calls are conv_transpose2d + F.pad + torch.cat.  Dtypes: float32, and half
tensors under fp16 / bf16 autocast with a float32 weight, as inside the UNet under autocast.  The fused forward + backward
includes the weight-pack launches and torch's weight-gradient GEMM.

Protocol (that of experiments/swin_seam_bench.py): one process, the same tensors, fused and today's path in alternating windows
of `--calls` calls between device events, median / min / max us per call over `--windows` windows.  An entry is `routed` only
where the fused median beats today's by more than the larger min-max spread of the two, forward and forward + backward both.
`achieved_fraction`: the forward's bytes (inputs read once, outputs written once) over the fused median, as a fraction of
6.3 TB/s.  `peak_bytes`: what one warmed forward + backward holds at its peak on top of what was allocated before it.

One JSON record (--out).  Needs a GPU: no fallback.

    python experiments/unet_seam_bench.py --out profiles/r25/unet_seam.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_ffn_infer_bench as NB  # noqa: E402  (puts the repository root on sys.path)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dhd_amd import unet_seam  # noqa: E402

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
B = 4
CL = torch.channels_last
POOLS = [(64, 200), (128, 100), (256, 50), (512, 25)]                   # C, H = W of the input
UPS = [(1024, 12, 25), (512, 25, 50), (256, 50, 100), (128, 100, 200)]   # Cin, h = w of x1, H = W of x2
PRECISIONS = {'f32': (F32, None), 'fp16_autocast': (F16, F16), 'bf16_autocast': (BF16, BF16)}   # tensor dtype, autocast dtype
NAME = {F32: 'float32', F16: 'float16', BF16: 'bfloat16'}
ACHIEVABLE = 6.3e12


def todays_up(x1, x2, w, b):
    y = F.conv_transpose2d(x1, w, b, stride=2)
    dy, dx = x2.size(2) - y.size(2), x2.size(3) - y.size(3)
    return torch.cat([x2, F.pad(y, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])], dim=1)


def make_case(kind, shape, dt, act, dev):
    torch.manual_seed(11)
    r = lambda *s: torch.randn(*s, device=dev)
    if kind == 'pool':
        C, H = shape
        x = torch.relu(r(B, C, H, H)).to(dt).contiguous(memory_format=CL).requires_grad_()
        leaves = (x,)
        fwd = {'today': lambda: F.max_pool2d(x, 2), 'fused': lambda: unet_seam.max_pool2x2(x)}
        out_shape = (B, C, H // 2, H // 2)
        nbytes = (x.numel() + B * C * (H // 2) ** 2) * x.element_size()
    else:
        Cin, h, H = shape
        x1 = r(B, Cin, h, h).to(dt).contiguous(memory_format=CL).requires_grad_()
        x2 = r(B, Cin // 2, H, H).to(dt).contiguous(memory_format=CL).requires_grad_()
        w = (r(Cin, Cin // 2, 2, 2) / Cin ** 0.5).requires_grad_()
        b = (0.1 * r(Cin // 2)).requires_grad_()
        leaves = (x1, x2, w, b)
        fwd = {'today': lambda: todays_up(x1, x2, w, b), 'fused': lambda: unet_seam.conv_transpose2x2_cat(x1, x2, w, b)}
        out_shape = (B, Cin, H, H)
        nbytes = (x1.numel() + x2.numel() + B * Cin * H * H) * x1.element_size() + w.numel() * w.element_size()
    dy = r(*out_shape).to(dt).contiguous(memory_format=CL)

    def ctx():
        return torch.autocast('cuda', dtype=act) if act is not None else torch.autocast('cuda', enabled=False)

    def forward(f):
        def g():
            with torch.no_grad(), ctx():
                return f()
        return g

    def both(f):
        def g():
            with ctx():
                y = f()
            return torch.autograd.grad(y, leaves, dy)
        return g
    paths = {'forward': {k: forward(f) for k, f in fwd.items()}, 'forward_backward': {k: both(f) for k, f in fwd.items()}}
    return paths, dict(shape=list(shape), dtype=NAME[dt], forward_bytes=nbytes)


def measure(paths, calls, windows):
    for fn in paths.values():
        for _ in range(3):
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
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda')
    record = {'protocol': f'{B} images, channels_last; alternating windows of {args.calls} calls, {args.windows} windows, median / min / max us per call',
              'cases': [], 'routed': [], 'not_routed': []}
    for kind, shapes in (('pool', POOLS), ('up', UPS)):
        for shape in shapes:
            for prec, (dt, act) in PRECISIONS.items():
                paths, info = make_case(kind, shape, dt, act, dev)
                rec = dict(kind=kind, precision=prec, **info)
                for what in ('forward', 'forward_backward'):
                    rec[what] = measure(paths[what], args.calls, args.windows)
                rec['peak_bytes'] = {k: NB.peak_bytes(fn) for k, fn in paths['forward_backward'].items()}
                rec['achieved_fraction'] = round(info['forward_bytes'] / (rec['forward']['fused']['median_us'] * 1e-6) / ACHIEVABLE, 3)
                rec['routed'] = bool(rec['forward']['wins'] and rec['forward_backward']['wins'])
                key = [kind, shape[0], NAME[dt], 'nhwc']
                record['routed' if rec['routed'] else 'not_routed'].append(key)
                record['cases'].append(rec)
                print(json.dumps(rec), flush=True)
                del paths
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
