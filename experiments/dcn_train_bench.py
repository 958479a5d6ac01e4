"""DCN in training, fused (dhd_amd.deform_conv: the inference operator as the forward, the HIP backward without column gradients)
against today's path (depthnet._DeformIm2col + torch.matmul with torch autograd), at (24, 256, 256, groups 4, 16, 44): both DCN
layers of DHD-S at batch size 4 see this shape.

Cases: {float32, fp16 autocast, bf16 autocast} x {NCHW, channels_last}; under autocast x is in the autocast type.  Per case,
with grad for x, the offsets and the weight, on the same tensors:

  today   DCN.forward with the switch off (the float32 staging copy of x, im2col, matmul; backward by torch autograd through
          dhd_deform_col2im_t)
  fused   deform_conv(x, offset, weight, ...): the weight packs of the forward and of the backward and torch's dW GEMM included

The offsets are a fixed float32 tensor handed to both (the 3 x 3 offset convolution in front is the same in both paths and is
left out).  `forward` is the forward alone (grad enabled: today's path saves what its backward needs), `step` is forward +
backward through torch.autograd.grad.  Both paths run in ONE process, alternating per window: device events, both warmed,
--windows windows of --calls calls each; median, min and max per path.  `routed` is ROUTED_TRAIN's rule: the fused step median
beats today's by more than the larger min-max spread of the two.  `peak_bytes` is the caching allocator's peak over a warmed
step above what was resident before it; `held_bytes` is what a forward leaves allocated for its backward (its result included).

One JSON record (--out).  Needs a GPU: no fallback.

    python experiments/dcn_train_bench.py --out profiles/r21/dcn_train.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import dhd_amd
from dhd_amd.depthnet import DCN
from occ_head_train_bench import held_bytes
from swin_ffn_train_bench import measure, peak_bytes

B, C, O, GROUPS, H, W = 24, 256, 256, 4, 16, 44
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# name -> (dtype of x = the GEMM type, channels_last)
CASES = {'f32_nchw': (F32, False), 'f32_channels_last': (F32, True), 'fp16_autocast_nchw': (F16, False),
         'fp16_autocast_channels_last': (F16, True), 'bf16_autocast_nchw': (BF16, False), 'bf16_autocast_channels_last': (BF16, True)}


class _Fixed(torch.nn.Module):
    def __init__(self, offset):
        super().__init__()
        self.offset = offset

    def forward(self, x):
        return self.offset


def make_case(dt, channels_last, dev):
    torch.manual_seed(7)
    x = torch.randn(B, C, H, W, device=dev).to(dt)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_()
    offset = (torch.randn(B, 18, H, W, device=dev) * 0.5).requires_grad_()
    m = DCN(C, O, groups=GROUPS).to(dev).train()
    m.fused_train = False
    m.conv_offset = _Fixed(offset)
    gout = torch.randn(B, O, H, W, device=dev).to(dt)
    gout_cl = gout.contiguous(memory_format=torch.channels_last)      # the gradient arrives in the layout of the output
    leaves = [x, offset, m.weight]
    auto = dt != F32
    forms = {'today': lambda: m(x), 'fused': lambda: dhd_amd.deform_conv(x, offset, m.weight, 1, 1, GROUPS)}

    def forward(f):
        def g():
            with torch.autocast('cuda', dtype=dt if auto else BF16, enabled=auto):
                return f()
        return g

    def step(f):
        fwd = forward(f)

        def g():
            out = fwd()
            return torch.autograd.grad(out, leaves, gout if out.is_contiguous() else gout_cl)
        return g
    return {k: forward(f) for k, f in forms.items()}, {k: step(f) for k, f in forms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES))
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dcn_train_bench: no GPU')
    dev = torch.device('cuda', 0)
    record = {'shape': [B, C, O, GROUPS, H, W], 'calls_per_window': args.calls, 'windows': args.windows, 'time': 'us per call',
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
    record['stay_with_todays_path'] = sorted(k for k, v in record['cases'].items() if not v['routed'])
    print(json.dumps({k: v for k, v in record.items() if k != 'cases'}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
