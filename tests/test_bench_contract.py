"""The driver's contract with bench.py (one JSON line, named fields), checked on the GPU with a short run."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_fields(gpu):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--full',
                          '--no-e2e', '--cpu-samples', '1', '--repeats', '3', '--fresh-procs', '1'], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
              'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 1 and d['higher_is_better'] is True
    assert d['unit'] == 'samples/s' and d['scaling'] == 'weak' and d['vs_baseline'] is None and d['dtype'] == 'f32'
    assert 'workload' in d['config'] and 'model' not in d['config']
    assert abs(d['value'] - 4 * 3 / (d['ms_per_step'] * 3e-3)) < 1e-6 * d['value']
    # the protocol of the timed region: R repeats of the K-step loop, the headline is the median loop; per-part statistics; the
    # same again from a fresh process
    assert d['repeats'] == 3 and len(d['ms_per_step_all']) == 3 and d['ms_per_step_min'] <= d['ms_per_step'] <= d['ms_per_step_max']
    for part in ('writer_ms', 'mghs_bwd_ms', 'sfa_fwd_ms', 'sfa_bwd_ms'):
        st = d['parts'][part]
        assert 0 < st['min'] <= st['median'] <= st['max']
    assert abs(d['roofline']['launch_ms'] - d['parts']['writer_ms']['median']) < 1e-12
    fp = d['fresh_processes']
    assert len(fp) == 1 and 'error' not in fp[0] and fp[0]['repeats'] == 3 and fp[0]['ms_per_step']['median'] > 0
    assert set(d['event_samples_dropped']) == {'dropped', 'total'} and d['event_samples_dropped']['dropped'] <= 0.1 * d['event_samples_dropped']['total'] + 1
    for name in ('roofline', 'roofline_bwd', 'roofline_operator', 'roofline_sfa_stage'):
        r = d[name]
        assert r['bound'] == 'hbm' and r['unit'] == 'GB/s' and r['peak'] == 8000.0
        frac = r['frac_effective'] if name == 'roofline_bwd' else r['frac']   # (algorithmic bytes over time; frac_hbm = counter bytes)
        assert abs(frac - r['achieved'] / r['peak']) < 1e-9 and 0.02 < frac < 1.0, (name, frac)
        if name == 'roofline_bwd':
            assert 'frac' not in r and (r['frac_hbm'] is None or 0.02 < r['frac_hbm'] < 1.0)
        assert r['traffic'] is None or r['traffic'] > 0
    c = d['cpu_baseline']
    assert c['kind'] == 'port' and c['unit'] == 'samples/s' and c['cores'] >= 1 and c['value'] > 0 and 'sample' in c
    assert d['value'] > 50 * c['value']            # sanity: the GPU path is not the CPU twin


HEADLINE = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
            'data', 'config')


@pytest.mark.gpu
def test_plain_bench_times_the_given_steps_once_and_dumps_the_last_step(gpu, tmp_path):
    """A plain run (no --full): W warm-ups, ONE loop of exactly K steps, the headline line and nothing else; --dump-outputs
    writes the last timed step's results as float .npy files (at most 64 MB), the same arrays from run to run."""
    import numpy as np
    runs = []
    for k in range(2):
        d = tmp_path / f'run{k}'
        t0 = time.perf_counter()
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '5', '--warmup', '2',
                              '--dump-outputs', str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        wall = time.perf_counter() - t0
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1
        line = json.loads(lines[0])
        for key in HEADLINE:
            assert key in line, key
        assert line['steps'] == 5 and line['warmup'] == 2 and line['repeats'] == 1 and line['dtype'] == 'f32'
        assert line['unit'] == 'samples/s' and line['higher_is_better'] is True
        assert abs(line['value'] - 4 * 5 / (line['ms_per_step'] * 5e-3)) < 1e-6 * line['value']
        assert 0 < line['ms_per_step'] * 5e-3 < wall
        for key in ('roofline', 'cpu_baseline', 'e2e', 'fresh_processes', 'hotpath_amp', 'roofline_operator', 'roofline_dhdl', 'parts'):
            assert key not in line, key
        files = sorted(f.name for f in d.iterdir())
        arrays = {f[:-4]: np.load(d / f) for f in files}
        assert all(f.endswith('.npy') for f in files)
        assert {'mghs_out0', 'mghs_out3', 'mghs_depth_grad', 'mghs_feat_grad', 'sfa_out', 'sfa_x_grad'} <= set(arrays)
        assert all(v.dtype in (np.float32, np.float64) and v.size > 0 and np.isfinite(v).all() for v in arrays.values())
        assert sum(os.path.getsize(d / f) for f in files) <= 64 * 2**20
        runs.append(arrays)
    a, b = runs
    assert set(a) == set(b)
    for name in a:
        assert a[name].shape == b[name].shape, name
        np.testing.assert_allclose(a[name], b[name], rtol=1e-4, atol=1e-5 * max(1.0, float(np.abs(b[name]).max())), err_msg=name)


def test_plain_and_full_run_arguments():
    """--repeats defaults to one loop in a plain run and to seven with --full; a counter pass and a fresh-process child are
    forms of the full measurement; --dump-outputs belongs to the hot path."""
    sys.path.insert(0, ROOT)
    import bench
    argv = sys.argv
    try:
        for args, full, repeats in (([], False, 1), (['--full'], True, 7), (['--repeats', '3'], False, 3),
                                    (['--pmc-pass'], True, 1), (['--child', '--repeats', '2'], True, 2)):
            sys.argv = ['bench.py', '--steps', '4'] + args
            a = bench.parse()
            assert (a.full, a.repeats, a.steps) == (full, repeats, 4), args
        sys.argv = ['bench.py', '--workload', 'e2e', '--dump-outputs', 'x']
        with pytest.raises(SystemExit):
            bench.parse()
    finally:
        sys.argv = argv


def test_dump_outputs_writes_a_fixed_sample_of_large_arrays(tmp_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    n = bench.DUMP_SAMPLE + 12345
    x = torch.arange(n, dtype=torch.float64) * 0.5
    arrays = dict(big=x, small=torch.arange(7, dtype=torch.float16), grad=torch.ones(3, 2))
    nbytes = bench.dump_outputs(arrays, str(tmp_path / 'a'))
    bench.dump_outputs(arrays, str(tmp_path / 'b'))
    big = np.load(tmp_path / 'a' / 'big.npy')
    assert big.dtype == np.float64 and big.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(big) > 0) and big[-1] <= 0.5 * (n - 1)
    assert np.array_equal(big, np.load(tmp_path / 'b' / 'big.npy'))          # the same positions every run
    small = np.load(tmp_path / 'a' / 'small.npy')
    assert small.dtype == np.float32 and np.array_equal(small, np.arange(7, dtype=np.float32))
    assert np.load(tmp_path / 'a' / 'grad.npy').shape == (6,)
    assert nbytes == 8 * bench.DUMP_SAMPLE + 4 * 7 + 4 * 6


@pytest.mark.gpu
def test_bench_refuses_more_ranks_than_gpus(gpu):
    import torch
    n = torch.cuda.device_count() + 1
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', str(n), '--steps', '1', '--warmup', '0'],
                         capture_output=True, text=True, timeout=300, cwd=ROOT,
                         env={k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')})
    assert out.returncode != 0 and 'GPU(s) are visible' in (out.stderr + out.stdout)


def test_committed_pmc_summary_is_reported_only_for_the_kernel_sources_it_was_collected_from():
    """bench.py reports `traffic` only while profiles/<round>/pmc_summary.json carries the hash of the kernel sources the
    library is built from; after a kernel edit without a fresh counter pass (profiles/collect.sh on the GPU box) the field
    must read null -- never a stale number."""
    import glob
    import warnings
    sys.path.insert(0, ROOT)
    import bench
    sha = bench.kernel_source_sha256()
    current = [f for f in glob.glob(os.path.join(ROOT, 'profiles', '*', 'pmc_summary.json'))
               if json.load(open(f)).get('source_sha256') == sha]
    if not current:
        warnings.warn('profiles/*/pmc_summary.json is stale for the current kernel sources: `traffic` reads null until '
                      'profiles/collect.sh has run on the GPU box')
        assert bench.pmc_traffic('mghs_stream_fwd', 4) is None and bench.sfa_forward_traffic(4) is None
        return
    assert bench.pmc_traffic('mghs_stream_fwd', 4) is not None
    both = [bench.pmc_traffic(k, 4) for k in ('mghs_stream_bwd', 'mghs_pixel_bwd')]
    assert None not in both
    fwd = bench.sfa_forward_traffic(4)
    assert fwd is not None and 4 * 328e6 < fwd < 2 * 4 * 328e6     # algorithmic 328 MB per sample


def test_event_mean_leaves_out_host_stalls():
    """bench.event_mean: an interval between two HIP events also contains the time the stream sat idle while the host was
    paused (a 36-39 ms garbage collection between an event and the next launch made a 26 us kernel read 1.9 ms); samples above
    three times the median are dropped, everything else is a plain mean."""
    sys.path.insert(0, ROOT)
    import bench

    class Ev:
        def __init__(self, t):
            self.t = t

        def elapsed_time(self, other):
            return other.t - self.t

    pairs = [(Ev(0.0), Ev(0.026)) for _ in range(19)] + [(Ev(0.0), Ev(38.0))]
    assert abs(bench.event_mean(pairs) - 0.026) < 1e-12
    pairs = [(Ev(0.0), Ev(t)) for t in (0.10, 0.12, 0.14, 0.29)]      # ordinary spread: nothing dropped
    assert abs(bench.event_mean(pairs) - 0.1625) < 1e-12
    import gc
    was = gc.isenabled()
    with bench.no_gc():
        assert not gc.isenabled()
    assert gc.isenabled() == was
