"""A/B of one environment switch over whole bench.py runs: the same bench.py command, one fresh process per run, alternating
without / with the switch set to 1, --runs runs each; the JSON result line of every run goes into one record (--out).

With --peak every run goes through a small driver that runs bench.py as __main__ in its own process (bench.py itself is
untouched) and prints torch's peak allocated bytes of the whole run after it; the figure is recorded per run.  With
--force-table MODULE.NAME the driver first sets every entry of that routing table (a dict of bools) to True, in every run of
both settings: what the switch would do if the measurement had routed everything.

A run that does not end with exit status 0 and a result line ends the script with that status: nothing more is started on the
GPU after a run that failed.

    python experiments/env_switch_ab.py --switch DHD_SWIN_GLUE --also DHD_WINDOW_ATTN_TRAIN=1 --out profiles/r12/e2e_dhdl_bf16_swin_glue_ab.json \\
        -- --gpus 1 --workload e2e --model dhd-l --amp bf16 --batch 2 --steps 6 --warmup 3
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# bench.py as __main__ (with --gpus 1 it runs in this process), then the caching allocator's peak
PEAK_DRIVER = ('import importlib, json, os, runpy, sys, torch\n'
               'force, sys.argv = sys.argv[1], sys.argv[2:]\n'
               'if force != "-":\n'
               '    sys.path.insert(0, os.path.dirname(sys.argv[0]))\n'
               '    table = getattr(importlib.import_module(force.rsplit(".", 1)[0]), force.rsplit(".", 1)[1])\n'
               '    table.update({k: True for k in table})\n'
               'try:\n'
               '    runpy.run_path(sys.argv[0], run_name="__main__")\n'
               'finally:\n'
               '    print(json.dumps({"peak_allocated_bytes": torch.cuda.max_memory_allocated()}))\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--switch', required=True, help='the environment variable that is absent / 1')
    ap.add_argument('--also', action='append', default=[], metavar='NAME=VALUE', help='set in every run')
    ap.add_argument('--runs', type=int, default=2, help='runs of each setting')
    ap.add_argument('--timeout', type=float, default=420.0, help='seconds per run')
    ap.add_argument('--peak', action='store_true', help='record the peak allocated bytes of every run')
    ap.add_argument('--force-table', default=None, metavar='MODULE.NAME', help='a routing table whose every entry is True in every run')
    ap.add_argument('--out', default=None)
    ap.add_argument('bench', nargs=argparse.REMAINDER, help='-- followed by the arguments of bench.py')
    args = ap.parse_args()
    bench = [a for a in args.bench if a != '--'] if args.bench[:1] == ['--'] else args.bench
    fixed = dict(kv.split('=', 1) for kv in args.also)
    record = {'command': 'bench.py ' + ' '.join(bench) + f', alternating without / with {args.switch}=1 in the environment, one process per run',
              'environment': fixed, 'runs': []}
    if args.force_table:
        record['forced_table'] = args.force_table
    for order in range(1, 2 * args.runs + 1):
        on = order % 2 == 0
        env = {k: v for k, v in os.environ.items() if k != args.switch}
        env.update(fixed)
        if on:
            env[args.switch] = '1'
        head = [sys.executable, '-c', PEAK_DRIVER, args.force_table or '-'] if args.peak or args.force_table else [sys.executable]
        out = subprocess.run(head + [os.path.join(ROOT, 'bench.py')] + bench, env=env, capture_output=True, text=True, timeout=args.timeout)
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
        peak = json.loads(lines.pop()) if len(head) > 1 and lines and 'peak_allocated_bytes' in lines[-1] else {}
        if out.returncode != 0 or not lines:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            raise SystemExit(out.returncode or 1)
        res = json.loads(lines[-1])
        run = dict({'order': order, args.switch: '1' if on else None}, **peak)
        run.update({k: res[k] for k in ('samples_per_s', 'ms_per_step', 'steps', 'warmup', 'dtype', 'hip_graph') if k in res})
        record['runs'].append(run)
        print(json.dumps(run), flush=True)
    for on in (None, '1'):
        ms = [r['ms_per_step'] for r in record['runs'] if r[args.switch] == on and 'ms_per_step' in r]
        if ms:
            record['with' if on else 'without'] = {'ms_per_step_mean': round(sum(ms) / len(ms), 2), 'spread_ms': round(max(ms) - min(ms), 2)}
            peaks = [r['peak_allocated_bytes'] for r in record['runs'] if r[args.switch] == on and 'peak_allocated_bytes' in r]
            if peaks:
                record['with' if on else 'without']['peak_allocated_bytes'] = max(peaks)
    print(json.dumps(record))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
