"""The fused deformable convolution of inference (dhd_deform_conv_infer) against the formulation it replaces.

At (B, 256, 16, 44) for B = 24 and 6, 256 -> 256 channels, groups = 4 (the DCN of the DHD-S HeightNet), for float32 (bf16x3), fp16
and bf16 x in NCHW and channels_last, in ONE process and alternating per window on the same x, offsets and weight:
(a) dhd_amd.deform_conv_infer; (b) the parent's path exactly as DCN.forward runs it: the float32 NCHW staging copy of x,
_DeformIm2col (the column matrix in the compute dtype) and torch.matmul with the weight, under autocast for a half x.  Device
events, both warmed, windows of --calls calls, --windows windows each; median and min-max per path, the peak bytes each path
allocates on top of its inputs, and max |a - b|.  One JSON record (--out).  Needs a GPU: no fallback.

    python experiments/dcn_infer_bench.py --out profiles/r9/dcn_infer.json
    python experiments/dcn_infer_bench.py --trace-only fp16     # a few calls of both paths, for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from dhd_amd.deform_conv import deform_conv_infer
from dhd_amd.depthnet import DCN, _DeformIm2col

PRECISIONS = {'f32_bf16x3': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}
LAYOUTS = ('nchw', 'channels_last')
C, O, GROUPS, K = 256, 256, 4, 3


def make_case(b, h, w, dtype, layout, dev):
    torch.manual_seed(11)
    weight = DCN(C, O, groups=GROUPS).weight.detach().to(dev)          # the layer's default init
    x = torch.randn(b, C, h, w, device=dev).to(dtype)
    if layout == 'channels_last':
        x = x.contiguous(memory_format=torch.channels_last)
    offset = torch.randn(b, 2 * K * K, h, w, device=dev) * 0.5

    def fused():
        return deform_conv_infer(x, offset, weight, padding=1, dilation=1, groups=GROUPS)

    def parent():      # DCN.forward's HIP branch, line for line, with the offsets given
        with torch.no_grad(), torch.autocast('cuda', dtype=dtype, enabled=dtype != torch.float32):
            wgt = weight.reshape(GROUPS, O // GROUPS, (C // GROUPS) * K * K)
            col = _DeformIm2col.apply(x, offset, K, 1, 1, dtype)
            out = torch.matmul(wgt, col.view(b, GROUPS, (C // GROUPS) * K * K, h * w))
            return out.reshape(b, O, h, w)
    return {'fused': fused, 'parent': parent}, (x, offset, weight)


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls   # us per call


def peak_bytes(fn):
    """Peak bytes a warmed call holds on top of what was allocated before it (its result included; pooled scratch is not: it
    is allocated once and listed separately)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def scratch_bytes(b, h, w, dtype, layout):
    import ctypes
    from dhd_amd import _lib
    n = ctypes.c_size_t()
    _lib.call('dhd_deform_conv_infer_scratch_bytes', b, C, O, GROUPS, K, h, w, _lib.DTYPE_CODE[dtype], int(layout == 'channels_last'), ctypes.byref(n))
    return n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[24, 6])
    ap.add_argument('--hw', type=int, nargs=2, default=[16, 44])
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace-only', default=None, help='run 3 calls of both paths of this precision (B = 24, both layouts) and exit')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dcn_infer_bench: no GPU')
    dev = torch.device('cuda', 0)
    h, w = args.hw
    record = {'shape': [C, O, GROUPS, h, w], 'calls_per_window': args.calls, 'windows': args.windows,
              'device': torch.cuda.get_device_name(0), 'cases': {}}
    for b in ([24] if args.trace_only else args.batches):
        for name in ([args.trace_only] if args.trace_only else list(PRECISIONS)):
            for layout in LAYOUTS:
                dtype = PRECISIONS[name]
                runs, keep = make_case(b, h, w, dtype, layout, dev)
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
                rec['fused']['pooled_scratch_bytes'] = scratch_bytes(b, h, w, dtype, layout)
                rec['speedup'] = round(rec['parent']['median_us'] / rec['fused']['median_us'], 2)
                spread = max(rec[k]['max_us'] - rec[k]['min_us'] for k in runs)
                rec['larger_spread_us'] = round(spread, 1)
                rec['fused_faster_beyond_spread'] = bool(rec['parent']['median_us'] - rec['fused']['median_us'] > spread)
                a, p = runs['fused'](), runs['parent']()
                rec['max_abs_diff'] = float((a.float() - p.float()).abs().max())
                rec['max_abs_parent'] = float(p.float().abs().max())
                record['cases'][f'b{b}_{name}_{layout}'] = rec
                print(f'b{b}_{name}_{layout}', json.dumps(rec), flush=True)
                del runs, keep, a, p
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
