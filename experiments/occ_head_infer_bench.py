"""The fused occupancy head of inference (dhd_occ_head_infer) against the module formulation it replaces.

At (B, 256, 200, 200) for B = 1 and 4, for float32 (bf16x3), fp16 and bf16 x in NCHW and channels_last, in ONE process and
alternating per window on the same final_conv output: (a) dhd_amd.occ_head_infer -> class grid, (b) the parent's path: torch
`predicter` on the permuted tensor (under autocast for a half x, as the detector runs it) -> float32 logits ->
occ_loss.occ_argmax_hist -> class grid.  Device events, both warmed, windows of --calls calls, --windows windows each; median and
min-max per path, the peak bytes each path allocates on top of its inputs, and whether the two class grids agree.  One JSON
record (--out).  Needs a GPU: no fallback.

    python experiments/occ_head_infer_bench.py --out profiles/r8/occ_head_infer.json
    python experiments/occ_head_infer_bench.py --trace-only fp16     # a few calls of both paths, for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from dhd_amd.detector import predictor
from dhd_amd.occ_head import occ_head_infer
from dhd_amd.occ_loss import occ_argmax_hist

PRECISIONS = {'f32_bf16x3': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}
LAYOUTS = ('nchw', 'channels_last')


def make_case(b, h, w, dtype, layout, dev):
    torch.manual_seed(7)
    head = predictor(256, 256, 16, num_classes=18).to(dev).eval()
    with torch.no_grad():
        for lin in (head.predicter[0], head.predicter[2]):
            lin.weight.mul_(3.0)
            lin.bias.uniform_(-0.5, 0.5)
    x = torch.randn(b, 256, h, w, device=dev).to(dtype)
    if layout == 'channels_last':
        x = x.contiguous(memory_format=torch.channels_last)
    lin1, lin2 = head.predicter[0], head.predicter[2]
    params = [p.detach() for p in (lin1.weight, lin1.bias, lin2.weight, lin2.bias)]

    def fused():
        return occ_head_infer(x, *params, dz=16)

    def parent():
        with torch.no_grad(), torch.autocast('cuda', dtype=dtype, enabled=dtype != torch.float32):
            logits = head.predicter(x.permute(0, 3, 2, 1))
        pred, _ = occ_argmax_hist(logits.float())
        return pred.view(b, w, h, 16)
    return {'fused': fused, 'parent': parent}, (head, x)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--hw', type=int, nargs=2, default=[200, 200])
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace-only', default=None, help='run 3 calls of both paths of this precision (B = 4, both layouts) and exit')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('occ_head_infer_bench: no GPU')
    dev = torch.device('cuda', 0)
    h, w = args.hw
    record = {'hw': args.hw, 'calls_per_window': args.calls, 'windows': args.windows, 'device': torch.cuda.get_device_name(0),
              'cases': {}}
    for b in ([4] if args.trace_only else args.batches):
        for name in ([args.trace_only] if args.trace_only else list(PRECISIONS)):
            for layout in LAYOUTS:
                runs, keep = make_case(b, h, w, PRECISIONS[name], layout, dev)
                for fn in runs.values():
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                if args.trace_only:
                    continue
                times = {k: [] for k in runs}
                for _ in range(args.windows):
                    for k, fn in runs.items():
                        times[k].append(window(fn, args.calls))
                rec = {k: {'median_us': round(statistics.median(ts), 1), 'min_us': round(min(ts), 1), 'max_us': round(max(ts), 1),
                           'peak_bytes': peak_bytes(runs[k])} for k, ts in times.items()}
                rec['speedup'] = round(rec['parent']['median_us'] / rec['fused']['median_us'], 2)
                rec['class_grid_agreement'] = round(float((runs['fused']() == runs['parent']()).float().mean()), 5)
                record['cases'][f'b{b}_{name}_{layout}'] = rec
                print(f'b{b}_{name}_{layout}', json.dumps(rec), flush=True)
                del runs, keep
                torch.cuda.empty_cache()
    if args.trace_only:
        return
    print(json.dumps(record))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
