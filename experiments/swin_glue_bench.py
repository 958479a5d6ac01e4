"""The three glue pieces of a SwinBlock, fused (dhd_amd/swin_glue.py) against the path they replace, at DHD-L's stage shapes.

12 images (2 x 6 views of 512 x 1408); token maps 128 x 352, 64 x 176, 32 x 88, 16 x 44 with C = 128, 256, 512, 1024; window 12, plain
and shifted by 6; float32, and the dtypes of a bf16 autocast region (float32 residual stream, bfloat16 windows and fc1 input).
Per piece, forward alone and forward + backward (torch.autograd.grad of everything that has a gradient, nothing accumulated):

  norm1_partition   today: F.layer_norm (float32 out, as autocast runs it) -> _WindowRows partition into the window dtype
                    fused: layer_norm_rows(..., window=...)
  reverse_add       today: x + _WindowRows reverse(win)                      fused: window_reverse_add(win, x, ...)
  norm2_cast        today: F.layer_norm -> .to(the dtype fc1 casts to)       fused: layer_norm_rows(..., out_dtype)

Both paths run in ONE process on the same tensors, alternating per window: device events, every shape warmed, --windows windows of
--calls calls each; median, min and max per path.  `fused_faster_beyond_spread` compares the two medians against the larger min-max
spread of the two paths in this process.  Bytes are counted from shapes here (the least each path can move: every tensor read or
written once per kernel that touches it), and `hbm_share` is the fused path's bytes over its median time over 6.3 TB/s, the
achievable HBM rate of the MI355X.  One JSON record (--out).  Needs a GPU: no fallback.

    python experiments/swin_glue_bench.py --out profiles/r12/swin_glue.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from dhd_amd.swin import _WindowRows
from dhd_amd.swin_glue import layer_norm_rows, window_reverse_add

WS, SHIFT, B, EPS = 12, 6, 12, 1e-5
HBM = 6.3e12
STAGES = {0: ((128, 352), 128), 1: ((64, 176), 256), 2: ((32, 88), 512), 3: ((16, 44), 1024)}
PRECISIONS = {'f32': torch.float32, 'bf16_autocast': torch.bfloat16}       # the window / fc1-input dtype; the token map is float32


def make_case(stage, cdt, shift, dev):
    """-> {piece: {mode: {path: fn}}}, {piece: {mode: {path: bytes}}}"""
    (H, W), C = STAGES[stage]
    nw = -(-H // WS) * -(-W // WS)
    T, R, s = B * H * W, B * nw * WS * WS, torch.empty(0, dtype=cdt).element_size()
    torch.manual_seed(7 + stage)
    x = (torch.randn(B, H * W, C, device=dev) * 1.5 + 0.5).requires_grad_()
    gamma = (1 + 0.2 * torch.randn(C, device=dev)).requires_grad_()
    beta = (0.1 * torch.randn(C, device=dev)).requires_grad_()
    win = torch.randn(B, nw, WS * WS, C, device=dev).to(cdt).requires_grad_()
    dwin = torch.randn(B, nw, WS * WS, C, device=dev).to(cdt)        # gradient of the windows
    dtok = torch.randn(B, H * W, C, device=dev)                      # gradient of a float32 token map
    dcast = dtok.to(cdt)                                             # gradient of fc1's input
    geom = (H, W, WS, shift)

    def grad(f, wrt, g):
        return lambda: torch.autograd.grad(f(), wrt, g)

    def nograd(f):
        def run():
            with torch.no_grad():
                return f()
        return run

    def n1_today():
        return _WindowRows.apply(F.layer_norm(x, (C,), gamma, beta, EPS).view(B, H, W, C), H, W, WS, shift, False, cdt)

    def n1_fused():
        return layer_norm_rows(x, gamma, beta, EPS, cdt, geom)

    def ra_today():
        return x + _WindowRows.apply(win, H, W, WS, shift, True, win.dtype).view(B, H * W, C)

    def ra_fused():
        return window_reverse_add(win, x, H, W, WS, shift)

    def n2_today():
        return F.layer_norm(x, (C,), gamma, beta, EPS).to(cdt)

    def n2_fused():
        return layer_norm_rows(x, gamma, beta, EPS, cdt)

    p3 = (x, gamma, beta)
    runs = {
        'norm1_partition': {'fwd': {'today': nograd(n1_today), 'fused': nograd(n1_fused)},
                            'fwd_bwd': {'today': grad(n1_today, p3, dwin), 'fused': grad(n1_fused, p3, dwin)}},
        'reverse_add': {'fwd': {'today': nograd(ra_today), 'fused': nograd(ra_fused)},
                        'fwd_bwd': {'today': grad(ra_today, (win, x), dtok), 'fused': grad(ra_fused, (win, x), dtok)}},
        'norm2_cast': {'fwd': {'today': nograd(n2_today), 'fused': nograd(n2_fused)},
                       'fwd_bwd': {'today': grad(n2_today, p3, dcast), 'fused': grad(n2_fused, p3, dcast)}},
    }
    tc, rc = T * C, R * C
    cast = 0 if s == 4 else 1      # float32: .to() is the tensor itself, no pass
    fwd = {
        'norm1_partition': {'today': (4 + 4) * tc + 4 * tc + s * rc, 'fused': 4 * tc + s * rc},
        'reverse_add': {'today': (s + s) * tc + (4 + s + 4) * tc, 'fused': (s + 4 + 4) * tc},
        'norm2_cast': {'today': (4 + 4) * tc + cast * (4 + s) * tc, 'fused': (4 + s) * tc},
    }
    bwd = {   # on top of the forward
        # today: the reverse gather of dwin into float32, then torch's LayerNorm backward (x, dy in, dx out); fused: x, dy in, dx out
        'norm1_partition': {'today': (s + 4) * tc + 3 * 4 * tc, 'fused': (4 + s + 4) * tc},
        # the add's backward hands its gradient through; the reverse's backward is the partition of it (both paths)
        'reverse_add': {'today': 4 * tc + s * rc, 'fused': 4 * tc + s * rc},
        'norm2_cast': {'today': cast * (s + 4) * tc + 3 * 4 * tc, 'fused': (4 + s + 4) * tc},
    }
    nbytes = {p: {'fwd': fwd[p], 'fwd_bwd': {k: fwd[p][k] + bwd[p][k] for k in fwd[p]}} for p in fwd}
    return runs, nbytes, dict(tokens=T, window_rows=R, channels=C)


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls   # us per call


def peak_bytes(fn):
    """Peak bytes a warmed call holds on top of what was allocated before it (its results included)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--stages', type=int, nargs='+', default=[0, 1, 2, 3])
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('swin_glue_bench: no GPU')
    dev = torch.device('cuda', 0)
    record = {'window': WS, 'shift': SHIFT, 'images': B, 'calls_per_window': args.calls, 'windows': args.windows, 'time': 'us per call',
              'hbm_rate': HBM, 'device': torch.cuda.get_device_name(0), 'cases': {}}
    for stage in args.stages:
        for pname, cdt in PRECISIONS.items():
            for shift in (0, SHIFT):
                runs, nbytes, shape = make_case(stage, cdt, shift, dev)
                for piece, modes in runs.items():
                    for mode, paths in modes.items():
                        for fn in paths.values():
                            for _ in range(3):
                                fn()
                        torch.cuda.synchronize()
                        times = {k: [] for k in paths}
                        for _ in range(args.windows):
                            for k, fn in paths.items():
                                times[k].append(window(fn, args.calls))
                        rec = {k: {'median_us': round(statistics.median(ts), 1), 'min_us': round(min(ts), 1), 'max_us': round(max(ts), 1),
                                   'bytes': nbytes[piece][mode][k], 'peak_bytes': peak_bytes(paths[k])} for k, ts in times.items()}
                        rec.update(shape)
                        rec['hbm_share'] = round(rec['fused']['bytes'] / (rec['fused']['median_us'] * 1e-6) / HBM, 3)
                        rec['speedup'] = round(rec['today']['median_us'] / rec['fused']['median_us'], 2)
                        spread = max(rec[k]['max_us'] - rec[k]['min_us'] for k in paths)
                        rec['larger_spread_us'] = round(spread, 1)
                        rec['fused_faster_beyond_spread'] = bool(rec['today']['median_us'] - rec['fused']['median_us'] > spread)
                        key = f"stage{stage}_{pname}_{'shifted' if shift else 'plain'}_{piece}_{mode}"
                        record['cases'][key] = rec
                        print(key, json.dumps(rec), flush=True)
                del runs
                torch.cuda.empty_cache()
    record['not_faster_beyond_spread'] = sorted(k for k, v in record['cases'].items() if not v['fused_faster_beyond_spread'])
    record['fused_faster_in_every_case'] = not record['not_faster_beyond_spread']
    print(json.dumps({k: v for k, v in record.items() if k != 'cases'}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
