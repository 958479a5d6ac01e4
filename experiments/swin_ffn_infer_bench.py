"""The second half of a SwinBlock at inference, fused (dhd_amd/swin_ffn.py) against the two forms it replaces, at DHD-L's stage shapes,
and the whole Swin backbone with the switch off / on.

12 images (2 x 6 views of 512 x 1408); token maps 128 x 352, 64 x 176, 32 x 88, 16 x 44 with C = 128, 256, 512, 1024, hidden 4C; a float32
residual stream under bf16 autocast, under fp16 autocast, and in float32 without autocast.  Per (stage, precision), no_grad:

  today        x + ffn(norm2(x)): nn.LayerNorm and the FFN module as SwinBlock.forward calls them
  today_glue   the same with fused_glue's norm2: ffn(layer_norm_rows(x, ..., the dtype fc1 reads), identity=x)
  fused        swin_ffn_infer(x, ...), its weight-pack launch included (where the operator takes the shape: C = 128, 256)

All paths run in ONE process on the same tensors, alternating per window: device events, every shape warmed, --windows windows of
--calls calls each; median, min and max per path.  `routed` is the routing rule of the pull request: the fused median beats BOTH
parents' medians by more than the larger min-max spread of the paths compared.  FLOPs are counted from shapes (2 x 2 x rows x C x 4C),
`tflops` is that over the fused median -- a whole-call rate, pack launch included, not a kernel's share of peak.  Peak bytes are the
caching allocator's, above what was resident before a warmed call.

Then the backbone: SwinTransformer of DHD-L at 12 x 3 x 512 x 1408, no_grad, bf16 autocast, fused_inference and fused_swin_glue on on both
sides, fused_swin_ffn off / on alternating, two runs each (with the routing table as committed, and -- `forced` -- with every entry
the operator takes switched on, which is what tells whether the table's entries pay off end to end).

One JSON record (--out).  Needs a GPU: no fallback.

    python experiments/swin_ffn_infer_bench.py --out profiles/r13/swin_ffn_infer.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

import dhd_amd
from dhd_amd import swin_ffn
from dhd_amd.swin import FFN, SwinTransformer
from dhd_amd.swin_glue import layer_norm_rows

B, EPS = 12, 1e-5
STAGES = {0: ((128, 352), 128), 1: ((64, 176), 256), 2: ((32, 88), 512), 3: ((16, 44), 1024)}
PRECISIONS = {'bf16_autocast': torch.bfloat16, 'fp16_autocast': torch.float16, 'f32': torch.float32}   # the GEMM dtype; the token map is float32


def make_case(stage, mdt, dev):
    (H, W), C = STAGES[stage]
    rows = B * H * W
    torch.manual_seed(7 + stage)
    x = torch.randn(B, H * W, C, device=dev) * 1.5 + 0.5
    norm = nn.LayerNorm(C, eps=EPS).to(dev).eval()
    ffn = FFN(C, 4 * C).to(dev).eval()
    with torch.no_grad():
        norm.weight.add_(0.2 * torch.randn(C, device=dev))
        norm.bias.add_(0.1 * torch.randn(C, device=dev))
    fc1, fc2 = ffn.layers[0][0], ffn.layers[1]
    auto = mdt != torch.float32

    def run(f):
        def g():
            with torch.no_grad(), torch.autocast('cuda', dtype=mdt if auto else torch.bfloat16, enabled=auto):
                return f()
        return g

    paths = {'today': run(lambda: ffn(norm(x), identity=x)),
             'today_glue': run(lambda: ffn(layer_norm_rows(x, norm.weight, norm.bias, EPS, mdt), identity=x))}
    if swin_ffn.swin_ffn_shape_supported(x, 4 * C, mdt):
        paths['fused'] = run(lambda: swin_ffn.swin_ffn_infer(x, norm.weight, norm.bias, EPS, fc1.weight, fc1.bias, fc2.weight, fc2.bias, mdt))
    return paths, dict(rows=rows, channels=C, hidden=4 * C, flop=2 * 2 * rows * C * 4 * C)


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls   # us per call


def peak_bytes(fn):
    """Peak bytes a warmed call holds on top of what was allocated before it (its result included)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def summary(ts):
    return {'median_us': round(statistics.median(ts), 1), 'min_us': round(min(ts), 1), 'max_us': round(max(ts), 1)}


def backbone(dev, forced, runs, steps):
    torch.manual_seed(3)
    net = SwinTransformer(pretrain_img_size=224, patch_size=4, window_size=12, mlp_ratio=4, embed_dims=128, depths=[2, 2, 18, 2],
                          num_heads=[4, 8, 16, 32], strides=(4, 2, 2, 2), out_indices=(2, 3), drop_path_rate=0.1, return_stereo_feat=True,
                          with_cp=False).to(dev).eval()
    net.init_weights()
    dhd_amd.fused_inference(net)
    dhd_amd.fused_swin_glue(net)
    img = torch.randn(B, 3, 512, 1408, device=dev)
    table = dict(swin_ffn.ROUTED)
    if forced:
        swin_ffn.ROUTED = {k: True for k in table}

    def fwd():
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            return net(img)
    times, outs = {'off': [], 'on': []}, {}
    try:
        for on in (False, True):
            dhd_amd.fused_swin_ffn(net, on)
            for _ in range(2):
                outs[on] = fwd()
        torch.cuda.synchronize()
        for _ in range(runs):
            for on in (False, True):
                dhd_amd.fused_swin_ffn(net, on)
                times['on' if on else 'off'].append(window(fwd, steps) / 1e3)
    finally:
        swin_ffn.ROUTED = table
    eff = {k: True for k in table} if forced else table
    blocks = sum(eff.get((b.norm2.normalized_shape[0], torch.float32, torch.bfloat16), False) for b in dhd_amd.fused_swin_ffn(net, False))
    diff = max(float((a.float() - b.float()).abs().max()) for a, b in zip(outs[True], outs[False]))
    scale = max(float(b.float().abs().max()) for b in outs[False])
    return {'ms_per_forward': {k: [round(t, 2) for t in v] for k, v in times.items()}, 'blocks_on_the_operator': int(blocks), 'of_blocks': 24,
            'max_abs_diff_on_vs_off': diff, 'max_abs_output': scale}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--stages', type=int, nargs='+', default=[0, 1, 2, 3])
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--backbone-runs', type=int, default=2)
    ap.add_argument('--backbone-steps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('swin_ffn_infer_bench: no GPU')
    dev = torch.device('cuda', 0)
    record = {'images': B, 'calls_per_window': args.calls, 'windows': args.windows, 'time': 'us per call',
              'device': torch.cuda.get_device_name(0), 'cases': {}}
    for stage in args.stages:
        for pname, mdt in PRECISIONS.items():
            paths, shape = make_case(stage, mdt, dev)
            for fn in paths.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in paths}
            for _ in range(args.windows):
                for k, fn in paths.items():
                    times[k].append(window(fn, args.calls))
            rec = {k: dict(summary(ts), peak_bytes=peak_bytes(paths[k])) for k, ts in times.items()}
            rec.update(shape)
            if 'fused' in paths:
                spread = max(rec[k]['max_us'] - rec[k]['min_us'] for k in paths)
                best_parent = min(rec['today']['median_us'], rec['today_glue']['median_us'])
                rec['larger_spread_us'] = round(spread, 1)
                rec['speedup_over_best_parent'] = round(best_parent / rec['fused']['median_us'], 2)
                rec['tflops'] = round(shape['flop'] / (rec['fused']['median_us'] * 1e-6) / 1e12, 1)
                rec['routed'] = bool(best_parent - rec['fused']['median_us'] > spread)
                a, p = paths['fused'](), paths['today']()
                rec['max_abs_diff_fused_vs_today'] = float((a - p).abs().max())
            else:
                rec['routed'] = False
                rec['fused'] = 'no operator for this C: today\'s path'
            key = f'stage{stage}_{pname}'
            record['cases'][key] = rec
            print(key, json.dumps(rec), flush=True)
            del paths
            torch.cuda.empty_cache()
    record['routed'] = sorted(k for k, v in record['cases'].items() if v['routed'])
    record['stay_with_torch'] = sorted(k for k, v in record['cases'].items() if not v['routed'])
    if args.backbone_runs > 0:
        for name, forced in (('backbone_table_as_committed', False), ('backbone_every_supported_entry_forced', True)):
            record[name] = backbone(dev, forced, args.backbone_runs, args.backbone_steps)
            print(name, json.dumps(record[name]), flush=True)
            torch.cuda.empty_cache()
    print(json.dumps({k: v for k, v in record.items() if k != 'cases'}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
