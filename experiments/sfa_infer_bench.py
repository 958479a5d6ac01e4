"""Forward-only inference operator of the SFA stage (dhd_sfa_stage_infer) against the eval-mode forward it replaces.

At (4, 512, 200, 200), for fp16 storage, bf16 storage and float32 bf16x3, through the C ABI, in ONE process and alternating per
window: (a) dhd_sfa_stage_forward(training = 0), (b) UNFUSED, (c) TWO_PASS, (d) ONE_PASS where it exists -- plus a second (a)
and a second (c) slot in the same rotation, which give the spread of a form against itself.  Device events, every form warmed,
windows of --calls calls, --windows windows each; median and min-max per form.  One JSON record (--out) with the medians, the
algorithmic HBM bytes computed from the shapes, and bytes / time as a share of the 8 TB/s peak; the transient allocation of
one module call with and without the inference operator goes into the same record.  Needs a GPU: no fallback.

    python experiments/sfa_infer_bench.py --out profiles/r7/sfa_infer.json
    python experiments/sfa_infer_bench.py --trace-only fp16     # a few calls of every form, for rocprofv3 --kernel-trace --stats
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from dhd_amd import _lib
from dhd_amd.mix import _stage_params, _stage_weights, channel_spatial_stage

PEAK = 8.0e12
FORMS = {'unfused': 1, 'two_pass': 2, 'one_pass': 3}
PRECISIONS = {'fp16': (torch.float16, torch.float16), 'bf16': (torch.bfloat16, torch.bfloat16), 'f32_bf16x3': (None, torch.float32)}


def algorithmic_bytes(b, c, hw, esz, out_esz):
    """HBM bytes of the (B,C,H,W)-sized tensor passes (weights, tables and pass bits left out); x_b and x_v are 2 planes."""
    plane = b * c * hw
    x = 2 * plane * esz
    return {
        'forward_eval': 3 * x + 4 * plane * esz + plane * out_esz,     # x three times, y1 w+r, y2 w+r, out
        'unfused': 3 * x + 4 * plane * esz + plane * out_esz,
        'two_pass': 3 * x + 2 * plane * esz + plane * out_esz,         # x three times, y1 w+r, out
        'one_pass': 2 * x + plane * out_esz,
    }


def make_case(name, b, c, h, w, dev):
    storage, io = PRECISIONS[name]
    torch.manual_seed(7)
    st = channel_spatial_stage(2 * c).to(dev)
    with torch.no_grad():
        for bn in (st.spacial_leanring[1], st.spacial_leanring[4]):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
    st.eval()
    st.gemm = 'bf16x3'
    x = (torch.randn(b, 2 * c, h, w, device=dev) * 0.7 + 0.1).to(storage or torch.float32)
    wts, ps = _stage_weights(st, _stage_params(st), io, storage is not None)
    lib = _lib.load()
    hw = h * w
    stream = _lib.stream_ptr(dev)
    out = torch.empty((b, c, h, w), dtype=io, device=dev)
    ns, nt = C.c_size_t(), C.c_size_t()
    _lib.check(lib.dhd_sfa_stage_workspace_bytes(b, c, hw, wts.hidden, wts.storage_dtype, C.byref(ns), C.byref(nt)), 'workspace')
    saved = torch.empty(ns.value, dtype=torch.uint8, device=dev)
    scratch = torch.empty(nt.value, dtype=torch.uint8, device=dev)
    keep = [st, x, ps, wts, out, saved, scratch]

    def forward_eval():
        _lib.check(lib.dhd_sfa_stage_forward(_lib.ptr(x), C.byref(wts), _lib.ptr(out), _lib.ptr(saved), _lib.ptr(scratch), b, c, hw, stream),
                   'dhd_sfa_stage_forward')
    runs = {'forward_eval': forward_eval}
    for fname, form in FORMS.items():
        if not lib.dhd_sfa_stage_infer_supported(c, hw, wts.storage_dtype, wts.gemm, form):
            continue
        n = C.c_size_t()
        _lib.check(lib.dhd_sfa_stage_infer_scratch_bytes(b, c, hw, wts.hidden, wts.storage_dtype, wts.gemm, form, C.byref(n)), 'scratch')
        sc = torch.empty(n.value, dtype=torch.uint8, device=dev)
        keep.append(sc)

        def run(form=form, sc=sc):
            _lib.check(lib.dhd_sfa_stage_infer(_lib.ptr(x), C.byref(wts), _lib.ptr(out), _lib.ptr(sc), b, c, hw, form, stream),
                       'dhd_sfa_stage_infer')
        runs[fname] = run
    esz = x.element_size()
    return runs, algorithmic_bytes(b, c, hw, esz, out.element_size()), keep, (st, x)


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls   # us per call


def module_transient(st, x):
    """Bytes a module call allocates beyond what it returns to the allocator, scratch pool warm."""
    res = {}
    for infer in (True, False):
        st.infer = infer
        with torch.no_grad():
            st(x)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            o = st(x)
            torch.cuda.synchronize()
            res['infer' if infer else 'training_operator'] = torch.cuda.max_memory_allocated() - before
            del o
    st.infer = True
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=4, default=[4, 512, 200, 200])
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace-only', default=None, help='run 5 calls of every form of this precision and exit')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sfa_infer_bench: no GPU')
    dev = torch.device('cuda', 0)
    b, c2, h, w = args.shape
    c = c2 // 2
    record = {'shape': args.shape, 'calls_per_window': args.calls, 'windows': args.windows, 'peak_bytes_per_s': PEAK,
              'device': torch.cuda.get_device_name(0), 'precisions': {}}
    for name in ([args.trace_only] if args.trace_only else list(PRECISIONS)):
        runs, nbytes, keep, (st, x) = make_case(name, b, c, h, w, dev)
        for fn in runs.values():          # every form warmed
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        if args.trace_only:
            return
        # the rotation: (a) (b) (c) [(d)] (a') (c'), one window each, repeated
        slots = [(k, k) for k in runs] + [('forward_eval#2', 'forward_eval'), ('two_pass#2', 'two_pass')]
        slots = [s for s in slots if s[1] in runs]
        times = {s[0]: [] for s in slots}
        for _ in range(args.windows):
            for label, key in slots:
                times[label].append(window(runs[key], args.calls))
        rec = {}
        for label, ts in times.items():
            key = label.split('#')[0]
            med = statistics.median(ts)
            rec[label] = {'median_us': round(med, 2), 'min_us': round(min(ts), 2), 'max_us': round(max(ts), 2),
                          'algorithmic_bytes': nbytes[key], 'share_of_peak': round(nbytes[key] / (med * 1e-6) / PEAK, 4)}
        rec['spread_us'] = {k: round(abs(rec[k]['median_us'] - rec[k + '#2']['median_us']), 2) for k in ('forward_eval', 'two_pass')
                            if k + '#2' in rec}
        rec['module_transient_bytes'] = module_transient(st, x)
        record['precisions'][name] = rec
        print(name, json.dumps(rec), flush=True)
        del runs, keep, st, x
        torch.cuda.empty_cache()
    line = json.dumps(record)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
