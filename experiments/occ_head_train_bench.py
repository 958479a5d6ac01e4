"""The occupancy head's predicter in training, fused (dhd_amd.occ_head.occ_head_train: the inference operator writing float32
logits as the forward, recompute HIP backward) against today's path with torch autograd, on final_conv's output at the DHD-S
training shape (4, 256, 200, 200).

Cases: {float32, fp16 autocast, bf16 autocast} x {NCHW, channels_last}; under autocast x is in the autocast type, as final_conv
hands it over.  Per case, with grad for x and the four parameters:

  today   predicter(x.permute(0, 3, 2, 1)) as predictor.forward calls it, then .float() as the loss reads it; backward from the
          same float32 glogits by torch autograd
  fused   occ_head_train(x, ...): both weight-pack launches and the two torch weight-gradient GEMMs included

`forward` is the forward alone (grad enabled: today's path saves what its backward needs), `step` is forward + backward through
torch.autograd.grad.  Both paths run in ONE process on the same tensors, alternating per window: device events, both warmed,
--windows windows of --calls calls each; median, min and max per path.  `routed` is ROUTED_TRAIN's rule: the fused step median
beats today's by more than the larger min-max spread of the two.  `peak_bytes` is the caching allocator's peak over a warmed
step above what was resident before it; `held_bytes` is what a forward leaves allocated for its backward (its result included).

One JSON record (--out).  Needs a GPU: no fallback.

    python experiments/occ_head_train_bench.py --out profiles/r20/occ_head_train.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn as nn

from dhd_amd import occ_head
from swin_ffn_train_bench import measure, peak_bytes

SHAPE = (4, 256, 200, 200)
DZ, N_CLS = 16, 18
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# name -> (dtype of x = the GEMM type, channels_last)
CASES = {'f32_nchw': (F32, False), 'f32_channels_last': (F32, True), 'fp16_autocast_nchw': (F16, False),
         'fp16_autocast_channels_last': (F16, True), 'bf16_autocast_nchw': (BF16, False), 'bf16_autocast_channels_last': (BF16, True)}


def make_case(dt, channels_last, dev):
    b, c, dy, dx = SHAPE
    torch.manual_seed(7)
    x = torch.randn(SHAPE, device=dev).to(dt)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_()
    predicter = nn.Sequential(nn.Linear(c, 2 * c), nn.Softplus(), nn.Linear(2 * c, N_CLS * DZ)).to(dev).train()
    lin1, lin2 = predicter[0], predicter[2]
    glogits = torch.randn(b, dx, dy, DZ, N_CLS, device=dev) * (torch.rand(b, dx, dy, DZ, 1, device=dev) >= 0.3)
    leaves = [x, lin1.weight, lin1.bias, lin2.weight, lin2.bias]
    auto = dt != F32
    forms = {'today': lambda: predicter(x.permute(0, 3, 2, 1)).view(b, dx, dy, DZ, N_CLS).float(),
             'fused': lambda: occ_head.occ_head_train(x, lin1.weight, lin1.bias, lin2.weight, lin2.bias, DZ)}

    def forward(f):
        def g():
            with torch.autocast('cuda', dtype=dt if auto else BF16, enabled=auto):
                return f()
        return g

    def step(f):
        fwd = forward(f)

        def g():
            return torch.autograd.grad(fwd(), leaves, glogits)
        return g
    return {k: forward(f) for k, f in forms.items()}, {k: step(f) for k, f in forms.items()}


def held_bytes(fn):
    """Bytes a warmed forward leaves allocated while its result is alive: the result and what autograd keeps for the backward."""
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - before
    del out
    return held


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES))
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('occ_head_train_bench: no GPU')
    dev = torch.device('cuda', 0)
    record = {'shape': list(SHAPE), 'calls_per_window': args.calls, 'windows': args.windows, 'time': 'us per call',
              'device': torch.cuda.get_device_name(0), 'cases': {}}
    for key in args.cases:
        dt, cl = CASES[key]
        forwards, steps = make_case(dt, cl, dev)
        rec = dict(x_dtype=str(dt), layout='channels_last' if cl else 'NCHW', forward=measure(forwards, args.windows, args.calls),
                   step=measure(steps, args.windows, args.calls))
        for k in steps:
            rec['step'][k]['peak_bytes'] = peak_bytes(steps[k])
            rec['forward'][k]['held_bytes'] = held_bytes(forwards[k])
        s = rec['step']
        spread = max(s[k]['max_us'] - s[k]['min_us'] for k in s)
        rec['largest_spread_us'] = round(spread, 1)
        rec['step_speedup_over_today'] = round(s['today']['median_us'] / s['fused']['median_us'], 2)
        rec['routed'] = bool(s['today']['median_us'] - s['fused']['median_us'] > spread)
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
