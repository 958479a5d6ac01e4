"""The pair kernel of the SFA backward's layer 1 (dhd_amd/csrc/sfa_gemm_pair1.h: pw_pair1_kernel), on the CPU.

  * the header's two instantiations build for gfx950 without private memory, within two waves per SIMD at C = 256, and the LDS
    plan (pw_pair_kernel's images, patches and prologue table + the current sample's blend coefficients) stays within 160 KB;
  * the two XOR identities the kernel derives its LDS write addresses from hold for sfa_gemm_pair.h's maps (mirrored in
    test_sfa_pair_map.py, which holds the mirrors against the header);
  * the dL/da rows: the kernel names the row of (worker, sample) `worker + sample` (pw_wgrad3_kernel's FOLD 2 format with W = 128
    workers) and fc_backward_kernel sums, for sample b, the rows w + b of the workers w_lo .. w_hi = wg_owner(first step of b) ..
    wg_owner(last step of b).  Mirrored here for the GPU test's shapes: every pair that occurs -- a worker with steps in the
    sample, or a worker without steps and the sample its empty range lies in -- gets exactly one row, and the rows a sample's
    sum reads are exactly the rows of the pairs of that sample whose worker lies in [w_lo, w_hi]: all workers with steps in it, and
    every worker without steps in between (whose row of zeros must therefore exist)."""
import os
import re
import subprocess

import pytest

import sfa_bwd_pair1_worker as W1
import test_sfa_pair_map as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'dhd_amd', 'csrc')
WORKERS = 128


def first_step(n, w):
    return n * w // WORKERS


def wg_owner(n, s):
    """csrc/sfa_stage.hip: the worker whose range [first_step(w), first_step(w + 1)) holds step s"""
    return ((s + 1) * WORKERS + n - 1) // n - 1


def written_rows(b, hw):
    """{(worker, sample): row} as pw_pair1_kernel writes them: a flush per sample of the worker's steps, or one row of zeros"""
    sps = (hw + 31) // 32
    n = b * sps
    rows = {}
    for w in range(WORKERS):
        first, end = first_step(n, w), first_step(n, w + 1)
        samples = sorted({s // sps for s in range(first, end)}) if end > first else [min(first // sps, b - 1)]
        for smp in samples:
            assert (w, smp) not in rows
            rows[w, smp] = w + smp
    return rows


@pytest.mark.parametrize('shape', W1.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_every_worker_sample_pair_has_one_row_and_a_samples_sum_reads_its_own(shape):
    c, b, h, w = shape
    hw = h * w
    sps = (hw + 31) // 32
    n = b * sps
    rows = written_rows(b, hw)
    assert len(set(rows.values())) == len(rows)                      # exactly one row per pair
    assert max(rows.values()) < WORKERS + b                          # inside [kPairWorkers + nb][c]
    by_row = {r: pair for pair, r in rows.items()}
    with_steps = {(wg_owner(n, s), s // sps) for s in range(n)}
    assert all(first_step(n, wk) <= s < first_step(n, wk + 1) for s in range(n) for wk in (wg_owner(n, s),))
    assert with_steps <= set(rows)
    seen = set()
    for smp in range(b):
        w_lo, w_hi = wg_owner(n, smp * sps), wg_owner(n, (smp + 1) * sps - 1)
        for wk in range(w_lo, w_hi + 1):
            assert by_row.get(wk + smp) == (wk, smp), (smp, wk)       # written, and by this worker for this sample
            seen.add((wk, smp))
    assert with_steps <= seen                                        # no step's contribution is left out
    assert all(pair in with_steps or first_step(n, pair[0]) == first_step(n, pair[0] + 1) for pair in seen)


def test_the_shapes_hold_workers_with_one_two_and_three_samples_and_without_steps():
    kinds = set()
    for c, b, h, w in W1.SHAPES:
        for _, samples in W1.worker_samples(b, h, w):
            kinds.add(len(samples))
    assert kinds == {0, 1, 2, 3}
    assert dict(W1.worker_samples(*W1.THREE_SAMPLES[1:]))[2] == [4, 5, 6]


@pytest.mark.parametrize('c', (128, 256))
def test_write_addresses_follow_from_one_base_by_xor(c):
    """row co0 + j (co0 % 4 == 0) of the A image at a_write(co0) ^ (j << 4); row ci + 8 (ci % 16 < 8) of the B image at
    b_write(ci) ^ 128"""
    for part in range(2):
        for q in range(8):
            for co0 in range(0, c, 4):
                for j in range(4):
                    assert M.a_write(c, co0 + j, q, part) == M.a_write(c, co0, q, part) ^ (j << 4)
            for ci in range(c // 2):
                if ci % 16 < 8:
                    assert M.b_write(c, ci + 8, q, part) == M.b_write(c, ci, q, part) ^ 128


def test_pair1_kernel_builds_for_gfx950_without_private_memory(tmp_path):
    """both instantiations: ScratchSize 0, at most 256 registers (two waves per SIMD at C = 256), the LDS plan within 160 KB"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    (tmp_path / 'pair1.hip').write_text(
        '#include "sfa_gemm_pair1.h"\nusing namespace dhd_sfa;\n'
        'struct FS { __host__ __device__ long long operator()(long long n, long long w, long long W) const { return n * w / W; } };\n'
        'template __global__ void dhd_sfa::pw_pair1_kernel<256, 2, FS>(Pair1Args);\n'
        'template __global__ void dhd_sfa::pw_pair1_kernel<128, 2, FS>(Pair1Args);\n')
    p = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-I', CSRC, '-I', os.path.join(ROOT, 'include'),
                        '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c', str(tmp_path / 'pair1.hip'), '-o', str(tmp_path / 'pair1.o')],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    blocks = re.findall(r'Function Name: (\S*pw_pair1_kernel\S*).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)', p.stderr, re.S)
    assert len(blocks) == 2, p.stderr[-2000:]
    for name, vgprs, agprs, scratch in blocks:
        print(name, 'VGPRs', vgprs, 'AGPRs', agprs, 'scratch', scratch)
        assert int(scratch) == 0, (name, scratch)
        assert int(vgprs) + int(agprs) <= 256, (name, vgprs, agprs)
    for c in (128, 256):
        assert 128 * c + 128 * c + 64 * c + (c // 32) * 16 * 36 * 4 + 3 * c * 4 + c * 4 <= 160 * 1024
