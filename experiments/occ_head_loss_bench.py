"""The occupancy head's predicter and its three losses in training as one operator (dhd_amd.occ_head.occ_head_losses: the loss
sums in the head's forward kernel, the gradient of the logits inside the head's backward kernel) against the parent path,
occ_head_train + occ_loss.occ_losses, on final_conv's output at the DHD-S training shape (4, 256, 200, 200) with a 70 % camera
mask.

Cases: {float32, fp16 autocast, bf16 autocast} x {NCHW, channels_last}; under autocast x is in the autocast type, as final_conv
hands it over.  Per case, with grad for x and the four parameters:

  parent  occ_losses(occ_head_train(x, ...), labels, mask, class_weight): five launches over the float32 logits
  fused   occ_head_losses(x, ..., labels, mask, class_weight)

each with both weight-pack launches and the two torch weight-gradient GEMMs.  `forward` is the forward alone (grad enabled),
`step` is forward + backward of the weighted sum of the three losses through torch.autograd.grad.  Both paths run in ONE process
on the same tensors, alternating per window: device events, both warmed, --windows windows of --calls calls each; median, min
and max per path.  `routed` is ROUTED_LOSS's rule: the fused step median beats the parent's by more than the larger min-max
spread of the two.  `peak_bytes` is the caching allocator's peak over a warmed step above what was resident before it;
`held_bytes` is what a forward leaves allocated for its backward (its result included).

One JSON record (--out).  Needs a GPU: no fallback.

    python experiments/occ_head_loss_bench.py --out profiles/r23/occ_head_loss.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import torch.nn as nn

from dhd_amd import occ_head, occ_loss
from dhd_amd.detector import NUSC_CLASS_FREQUENCIES
from occ_head_train_bench import BF16, CASES, DZ, F32, N_CLS, SHAPE, held_bytes
from swin_ffn_train_bench import measure, peak_bytes

LOSS_WEIGHTS = (0.7, 1.3, 2.0)


def make_case(dt, channels_last, dev):
    b, c, dy, dx = SHAPE
    torch.manual_seed(7)
    x = torch.randn(SHAPE, device=dev).to(dt)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_()
    predicter = nn.Sequential(nn.Linear(c, 2 * c), nn.Softplus(), nn.Linear(2 * c, N_CLS * DZ)).to(dev).train()
    lin1, lin2 = predicter[0], predicter[2]
    params = [lin1.weight, lin1.bias, lin2.weight, lin2.bias]
    labels = torch.randint(0, N_CLS, (b, dx, dy, DZ), device=dev).to(torch.uint8)
    labels[torch.rand(labels.shape, device=dev) < 0.01] = 255
    mask = (torch.rand(labels.shape, device=dev) < 0.7).to(torch.uint8)
    cw = torch.from_numpy((1 / np.log(NUSC_CLASS_FREQUENCIES[:N_CLS] + 0.001)).astype(np.float32)).to(dev)
    up = torch.tensor(LOSS_WEIGHTS, device=dev)
    leaves = [x] + params
    auto = dt != F32
    forms = {'parent': lambda: torch.stack(occ_loss.occ_losses(occ_head.occ_head_train(x, *params, DZ).view(-1, N_CLS), labels, mask, cw)),
             'fused': lambda: torch.stack(occ_head.occ_head_losses(x, *params, labels, mask, cw, dz=DZ))}

    def forward(f):
        def g():
            with torch.autocast('cuda', dtype=dt if auto else BF16, enabled=auto):
                return f()
        return g

    def step(f):
        fwd = forward(f)

        def g():
            return torch.autograd.grad(fwd(), leaves, up)
        return g
    return {k: forward(f) for k, f in forms.items()}, {k: step(f) for k, f in forms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES))
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('occ_head_loss_bench: no GPU')
    dev = torch.device('cuda', 0)
    record = {'shape': list(SHAPE), 'camera_mask': 0.7, 'calls_per_window': args.calls, 'windows': args.windows, 'time': 'us per call',
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
        rec['step_speedup_over_parent'] = round(s['parent']['median_us'] / s['fused']['median_us'], 3)
        rec['routed'] = bool(s['parent']['median_us'] - s['fused']['median_us'] > spread)
        a, p = steps['fused'](), steps['parent']()
        rec['max_abs_diff_dx_fused_vs_parent'] = float((a[0].float() - p[0].float()).abs().max())
        rec['losses'] = {k: [float(t) for t in forwards[k]().detach()] for k in forwards}
        record['cases'][key] = rec
        print(key, json.dumps(rec), flush=True)
        del forwards, steps, a, p
        torch.cuda.empty_cache()
    record['routed'] = sorted(k for k, v in record['cases'].items() if v['routed'])
    record['stay_with_parent'] = sorted(k for k, v in record['cases'].items() if not v['routed'])
    print(json.dumps({k: v for k, v in record.items() if k != 'cases'}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
