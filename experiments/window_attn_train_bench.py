"""Forward + backward of the Swin window attention in training: dhd_amd.window_attn against the formulation it replaces.

At DHD-L's four stage shapes (B = 2 x 6 views of 512 x 1408, 12 x 12 windows: 3960 / 1080 / 288 / 96 windows of 4 / 8 / 16 / 32
heads), for float32 (bf16x3), fp16 and bf16 qkv, plain and shifted blocks, in ONE process and alternating per window on the same
qkv tensor (the qkv projection's output), table, mask and output gradient:
(a) dhd_amd.window_attn: qkv as it lies -> the tensor `proj` reads, and its fused backward -> (dqkv, dtable);
(b) the parent's core exactly as WindowMSA.forward runs it (the operand permute, the bias / mask expansion and its cast,
F.scaled_dot_product_attention, the output transpose) and torch's autograd backward through all of it.
What is timed is torch.autograd.grad(forward(qkv, table), (qkv, table), dout): one forward + one backward, nothing accumulated.
Device events, both warmed, windows of --calls calls, --windows windows each; median and min-max per path, the peak bytes each path
allocates on top of its inputs, and the largest gradient difference.  One JSON record (--out).  Needs a GPU: no fallback.

    python experiments/window_attn_train_bench.py --out profiles/r11/window_attn_train.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from dhd_amd.swin import WindowMSA, shift_window_mask, shift_window_regions
from dhd_amd.window_attn import window_attn

PRECISIONS = {'f32_bf16x3': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}
WS, SHIFT, B = 12, 6, 12
# stage -> (padded map, heads): 128 x 352, 64 x 176, 32 x 88, 16 x 44 token maps padded up to the window
STAGES = {0: ((132, 360), 4), 1: ((72, 180), 8), 2: ((36, 96), 16), 3: ((24, 48), 32)}


def make_case(stage, dtype, shifted, dev):
    (hp, wp), nh = STAGES[stage]
    nw, n, c = (hp // WS) * (wp // WS), WS * WS, nh * 32
    torch.manual_seed(11 + stage)
    msa = WindowMSA(c, nh, (WS, WS)).to(dev).train()
    with torch.no_grad():
        msa.relative_position_bias_table.normal_(0, 0.5)
    qkv = torch.randn(B, nw, n, 3 * c, device=dev).to(dtype).requires_grad_()
    dout = torch.randn(B, nw, n, c, device=dev).to(dtype)
    mask = shift_window_mask(hp, wp, WS, SHIFT, dev) if shifted else None
    regions = shift_window_regions(hp, wp, WS, SHIFT, dev) if shifted else None
    table, index, scale = msa.relative_position_bias_table, msa.relative_position_index, msa.scale

    def fused():
        out = window_attn(qkv, table, (WS, WS), nh, scale, regions=regions)
        return torch.autograd.grad(out, (qkv, table), dout)

    def parent():      # WindowMSA.forward between its two Linear layers, line for line, and autograd through it
        q = qkv.view(B, nw, n, 3, nh, 32).permute(3, 0, 1, 4, 2, 5).reshape(3, B, nw * nh, n, 32)
        bias = table[index.view(-1)].view(n, n, -1).permute(2, 0, 1)
        bias = bias.unsqueeze(0).expand(nw, nh, n, n) if mask is None else bias.unsqueeze(0) + mask.unsqueeze(1)
        out = F.scaled_dot_product_attention(q[0], q[1], q[2], attn_mask=bias.reshape(1, nw * nh, n, n).to(q.dtype), dropout_p=0., scale=scale)
        out = out.view(B, nw, nh, n, 32).transpose(2, 3).reshape(B, nw, n, c)
        return torch.autograd.grad(out, (qkv, table), dout)
    return {'fused': fused, 'parent': parent}, (qkv, dout, mask, regions, msa), B * nw


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
        raise SystemExit('window_attn_train_bench: no GPU')
    dev = torch.device('cuda', 0)
    record = {'window': WS, 'shift': SHIFT, 'images': B, 'calls_per_window': args.calls, 'windows': args.windows,
              'timed': 'forward + backward, us per call', 'device': torch.cuda.get_device_name(0), 'cases': {}}
    for stage in args.stages:
        for name, dtype in PRECISIONS.items():
            for shifted in (False, True):
                runs, keep, n_windows = make_case(stage, dtype, shifted, dev)
                for fn in runs.values():
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                times = {k: [] for k in runs}
                for _ in range(args.windows):
                    for k, fn in runs.items():
                        times[k].append(window(fn, args.calls))
                rec = {k: {'median_us': round(statistics.median(ts), 1), 'min_us': round(min(ts), 1), 'max_us': round(max(ts), 1),
                           'peak_bytes': peak_bytes(runs[k])} for k, ts in times.items()}
                rec['attention_windows'], rec['heads'] = n_windows, STAGES[stage][1]
                rec['speedup'] = round(rec['parent']['median_us'] / rec['fused']['median_us'], 2)
                spread = max(rec[k]['max_us'] - rec[k]['min_us'] for k in runs)
                rec['larger_spread_us'] = round(spread, 1)
                rec['fused_faster_beyond_spread'] = bool(rec['parent']['median_us'] - rec['fused']['median_us'] > spread)
                a, p = runs['fused'](), runs['parent']()
                for i, g in enumerate(('dqkv', 'dtable')):
                    rec[f'max_abs_diff_{g}'] = float((a[i].float() - p[i].float()).abs().max())
                    rec[f'max_abs_parent_{g}'] = float(p[i].float().abs().max())
                key = f"stage{stage}_{name}_{'shifted' if shifted else 'plain'}"
                record['cases'][key] = rec
                print(key, json.dumps(rec), flush=True)
                del runs, keep, a, p
                torch.cuda.empty_cache()
    record['slower_cases'] = sorted(k for k, v in record['cases'].items() if v['speedup'] <= 1.0)
    record['fused_faster_in_every_case'] = not record['slower_cases']
    print(json.dumps(record))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
