"""The second half of a SwinBlock in training at C = 512, fused (dhd_amd.swin_ffn through the wide training family: the wide forward
with the DropPath factor, recompute HIP backward) against the two forms it replaces with torch autograd, at DHD-L's stage-2 shape.

12 images (2 x 6 views of 512 x 1408); token maps 32 x 88 with C = 512: 33 792 rows, hidden 2048, DropPath active (keep 0.9, one
fixed draw shared by all paths so that they do the same work).  Cases: float32 tokens under bf16 autocast, under fp16 autocast and
in float32, and tokens in the autocast type (what patch merging hands the stage) under bf16 and under fp16 autocast.  The paths,
`forward`, `step`, the windows and the `routed` rule are those of experiments/swin_ffn_train_bench.py, whose functions this script
uses: all paths in ONE process on the same tensors, alternating per window, device events, median, min and max per path; `step` is
forward + backward with both weight packs and torch's four weight-gradient reductions included; `routed` is True where the fused
step median beats BOTH parents' step medians by more than the largest min-max spread of the three.

One JSON record (--out).  Needs a GPU: no fallback.

    python experiments/swin_ffn_train_wide_bench.py --out profiles/r17/swin_ffn_train_wide.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import swin_ffn_train_bench as NB
from dhd_amd import swin_ffn

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# name -> (stage, token dtype, GEMM dtype)
CASES = {'stage2_bf16_autocast': (2, F32, BF16), 'stage2_fp16_autocast': (2, F32, F16), 'stage2_f32': (2, F32, F32),
         'stage2_bf16_tokens': (2, BF16, BF16), 'stage2_fp16_tokens': (2, F16, F16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES))
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('swin_ffn_train_wide_bench: no GPU')
    dev = torch.device('cuda', 0)
    record = {'images': NB.B, 'calls_per_window': args.calls, 'windows': args.windows, 'time': 'us per call',
              'device': torch.cuda.get_device_name(0), 'cases': {}}
    for key in args.cases:
        stage, xdt, mdt = CASES[key]
        forwards, steps, shape = NB.make_case(stage, xdt, mdt, dev, swin_ffn.swin_ffn_train_wide_shape_supported)
        assert 'fused' in steps, key
        rec = dict(shape, forward=NB.measure(forwards, args.windows, args.calls), step=NB.measure(steps, args.windows, args.calls))
        for k, fn in steps.items():
            rec['step'][k]['peak_bytes'] = NB.peak_bytes(fn)
        s = rec['step']
        spread = max(s[k]['max_us'] - s[k]['min_us'] for k in s)
        best_parent = min(s['today']['median_us'], s['today_glue']['median_us'])
        rec['largest_spread_us'] = round(spread, 1)
        rec['step_speedup_over_best_parent'] = round(best_parent / s['fused']['median_us'], 2)
        rec['forward_speedup_over_best_parent'] = round(min(rec['forward']['today']['median_us'], rec['forward']['today_glue']['median_us'])
                                                        / rec['forward']['fused']['median_us'], 2)
        rec['routed'] = bool(best_parent - s['fused']['median_us'] > spread)
        a, p = steps['fused'](), steps['today']()
        rec['max_abs_diff_dx_fused_vs_today'] = float((a[0].float() - p[0].float()).abs().max())
        record['cases'][key] = rec
        print(key, json.dumps(rec), flush=True)
        del forwards, steps, a, p
        torch.cuda.empty_cache()
    record['routed'] = sorted(k for k, v in record['cases'].items() if v['routed'])
    record['stay_with_torch'] = sorted(k for k, v in record['cases'].items() if not v['routed'])
    print(json.dumps({k: v for k, v in record.items() if k != 'cases'}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
