"""The second half of a SwinBlock in training, fused (dhd_amd.swin_ffn: forward with the DropPath factor, recompute HIP backward)
against the two forms it replaces with torch autograd, at DHD-L's stage-0 and stage-1 shapes.

12 images (2 x 6 views of 512 x 1408); token maps 128 x 352 with C = 128 and 64 x 176 with C = 256, hidden 4C, DropPath active
(keep 0.9, one fixed draw shared by all paths so that they do the same work).  Cases: stage 0 with float32 tokens under bf16
autocast, under fp16 autocast, and in float32; stage 1 with float32 tokens and with tokens in the autocast type (what patch merging
hands the stage) under bf16 and under fp16 autocast.  Per case, with grad:

  today        x + drop_path(ffn(norm2(x))): nn.LayerNorm and the FFN module as SwinBlock.forward calls them, torch autograd
  today_glue   the same with fused_glue's norm2 (layer_norm_rows into the dtype fc1 reads), torch autograd + its HIP backward
  fused        swin_ffn(x, ..., scale): both weight-pack launches and the four torch weight-gradient GEMMs / sums included

`forward` is the forward alone (grad enabled: the parents save what their backward needs), `step` is forward + backward through
torch.autograd.grad for x and the six parameters.  All paths run in ONE process on the same tensors, alternating per window: device
events, every shape warmed, --windows windows of --calls calls each; median, min and max per path.  `routed` is ROUTED_TRAIN's
rule: the fused step median beats BOTH parents' step medians by more than the largest min-max spread of the three.  Peak bytes are
the caching allocator's over a warmed step, above what was resident before it.

One JSON record (--out).  Needs a GPU: no fallback.

    python experiments/swin_ffn_train_bench.py --out profiles/r16/swin_ffn_train.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

from dhd_amd import swin_ffn
from dhd_amd.swin import FFN
from dhd_amd.swin_glue import layer_norm_rows, swin_glue_supported

B, EPS, KEEP = 12, 1e-5, 0.9
STAGES = {0: ((128, 352), 128), 1: ((64, 176), 256), 2: ((32, 88), 512)}      # stage 2: swin_ffn_train_wide_bench.py's
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# name -> (stage, token dtype, GEMM dtype)
CASES = {'stage0_bf16_autocast': (0, F32, BF16), 'stage0_fp16_autocast': (0, F32, F16), 'stage0_f32': (0, F32, F32),
         'stage1_bf16_autocast': (1, F32, BF16), 'stage1_fp16_autocast': (1, F32, F16),
         'stage1_bf16_tokens': (1, BF16, BF16), 'stage1_fp16_tokens': (1, F16, F16)}


def make_case(stage, xdt, mdt, dev, supported=swin_ffn.swin_ffn_train_shape_supported):
    """`supported`: the predicate of the training family that takes the stage's C."""
    (H, W), C = STAGES[stage]
    rows = B * H * W
    torch.manual_seed(7 + stage)
    x = (torch.randn(B, H * W, C, device=dev) * 1.5 + 0.5).to(xdt).requires_grad_()
    dout = torch.randn(B, H * W, C, device=dev).to(xdt)
    norm = nn.LayerNorm(C, eps=EPS).to(dev).train()
    ffn = FFN(C, 4 * C).to(dev).train()
    with torch.no_grad():
        norm.weight.add_(0.2 * torch.randn(C, device=dev))
        norm.bias.add_(0.1 * torch.randn(C, device=dev))
    fc1, fc2 = ffn.layers[0][0], ffn.layers[1]
    kept = (KEEP + torch.rand((B, 1, 1), device=dev)).floor()
    scale = kept.view(-1).float().div(KEEP)
    auto = mdt != F32
    leaves = [x, norm.weight, norm.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias]

    def drop(t):                                      # DropPath.forward on a fixed draw
        return t.div(KEEP) * kept.to(t.dtype)

    forms = {'today': lambda: x + drop(ffn.layers(norm(x)))}
    glue = swin_glue_supported(x, plain_ln_to=mdt)       # as SwinBlock._forward_glue asks: where there is no cast to fuse, torch's norm2
    forms['today_glue'] = (lambda: x + drop(ffn.layers(layer_norm_rows(x, norm.weight, norm.bias, EPS, mdt)))) if glue else forms['today']
    if supported(x, 4 * C, mdt):
        forms['fused'] = lambda: swin_ffn.swin_ffn(x, norm.weight, norm.bias, EPS, fc1.weight, fc1.bias, fc2.weight, fc2.bias, mdt, scale)

    def forward(f):
        def g():
            with torch.autocast('cuda', dtype=mdt if auto else BF16, enabled=auto):
                return f()
        return g

    def step(f):
        fwd = forward(f)

        def g():
            return torch.autograd.grad(fwd(), leaves, dout)
        return g
    return ({k: forward(f) for k, f in forms.items()}, {k: step(f) for k, f in forms.items()},
            dict(rows=rows, channels=C, hidden=4 * C, tokens=str(xdt), gemms=str(mdt), dropped_images=int(B - kept.sum()), today_glue_is='layer_norm_rows' if glue else 'nn.LayerNorm, as today'))


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


def measure(paths, windows, calls):
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(windows):
        for k, fn in paths.items():
            times[k].append(window(fn, calls))
    return {k: summary(ts) for k, ts in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES))
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('swin_ffn_train_bench: no GPU')
    dev = torch.device('cuda', 0)
    record = {'images': B, 'calls_per_window': args.calls, 'windows': args.windows, 'time': 'us per call',
              'device': torch.cuda.get_device_name(0), 'cases': {}}
    for key in args.cases:
        stage, xdt, mdt = CASES[key]
        forwards, steps, shape = make_case(stage, xdt, mdt, dev)
        rec = dict(shape, forward=measure(forwards, args.windows, args.calls), step=measure(steps, args.windows, args.calls))
        for k, fn in steps.items():
            rec['step'][k]['peak_bytes'] = peak_bytes(fn)
        if 'fused' in steps:
            s = rec['step']
            spread = max(s[k]['max_us'] - s[k]['min_us'] for k in s)
            best_parent = min(s['today']['median_us'], s['today_glue']['median_us'])
            rec['largest_spread_us'] = round(spread, 1)
            rec['step_speedup_over_best_parent'] = round(best_parent / s['fused']['median_us'], 2)
            rec['routed'] = bool(best_parent - s['fused']['median_us'] > spread)
            a, p = steps['fused'](), steps['today']()
            rec['max_abs_diff_dx_fused_vs_today'] = float((a[0].float() - p[0].float()).abs().max())
        else:
            rec['routed'] = False
            rec['fused'] = 'no operator for this combination: today\'s path'
        record['cases'][key] = rec
        print(key, json.dumps(rec), flush=True)
        del forwards, steps
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
