"""The pair kernel of the SFA backward (dhd_amd/csrc/sfa_gemm_pair.h: pw_pair_kernel), on the CPU.

  * pair_slot and the three LDS image maps are pure functions: mirrored here in Python, and the mirrors are held against the
    header's own text compiled as a host program (with wg_first_step cut out of sfa_stage.hip);
  * every (32-pixel step, half of the input channels) is owned by exactly one workgroup, and the two workgroups of a pair have
    equal blockIdx % 8;
  * the writers of an image cover every byte exactly once, and a reader lane finds the MFMA operand element it must hold
    (v_mfma_f32_16x16x32_bf16 B operand for the D image, v_mfma_f32_32x32x16_bf16 A / B operands for the A / B images; the two
    weight-gradient images agree on the pixel order along k);
  * the five access patterns touch every bank at most once per lane group (ds_write_b64: 4 x 16 contiguous lanes, bank =
    (addr / 4) mod 32; ds_read_b128: 4 groups of 16 lanes, bank = (addr / 4) mod 64; MI355X_MICROARCH.md, LDS);
  * the header's two instantiations build for gfx950 without private memory, within two waves per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'dhd_amd', 'csrc')
HEADER = os.path.join(CSRC, 'sfa_gemm_pair.h')
WORKERS, GRID = 128, 256
SHAPES = ((128, 3, 36, 40), (256, 2, 52, 60), (128, 2, 20, 28), (256, 6, 12, 20), (128, 3, 64, 64), (128, 3, 100, 100), (256, 3, 60, 60))


# ---- the mirrors ---------------------------------------------------------------------------------------------------------------
def pair_slot(block):
    return (block >> 4) * 8 + (block & 7), (block >> 3) & 1


def first_step(n, w, workers=WORKERS):
    return n * w // workers


def d_write(co, p, part):
    q, e = p >> 2, p & 3
    return (((((co >> 5) * 2 + part) * 2 + (e >> 1)) * 64 + 16 * ((co >> 3) & 3) + q + 8 * (e & 1)) << 4) + 8 * ((co >> 2) & 1)


def d_read(ks, part, nt, lane):
    return ((((ks * 2 + part) * 2 + nt) * 64) + lane) << 4


def a_write(c, co, q, part):
    kk, h = q >> 2, (q >> 1) & 1
    return ((((kk * (c // 32) + (co >> 5)) * 2 + part) * 64 + ((co & 31) ^ (2 * kk + h)) + 32 * h) << 4) + 8 * (q & 1)


def a_read(c, kk, tile, part, lane):
    return (((kk * (c // 32) + tile) * 2 + part) * 64 + (lane ^ (2 * kk + (lane >> 5)))) << 4


def b_write(c, ci, q, part):
    kk, h = q >> 2, (q >> 1) & 1
    return ((((kk * (c // 64) + (ci >> 5)) * 2 + part) * 64 + ((ci & 31) ^ ((2 * kk + h) << 1)) + 32 * h) << 4) + 8 * (q & 1)


def b_read(c, kk, tile, part, lane):
    return (((kk * (c // 64) + tile) * 2 + part) * 64 + (lane ^ ((2 * kk + (lane >> 5)) << 1))) << 4


# ---- ownership -----------------------------------------------------------------------------------------------------------------
def test_pairs_share_an_xcd_slot_and_cover_both_halves():
    by_worker = {}
    for block in range(GRID):
        w, h = pair_slot(block)
        by_worker.setdefault(w, []).append((h, block))
    assert sorted(by_worker) == list(range(WORKERS))
    for w, members in by_worker.items():
        assert sorted(h for h, _ in members) == [0, 1]
        (_, b0), (_, b1) = sorted(members)
        assert b0 % 8 == b1 % 8 and b0 // 16 == b1 // 16 and b1 == b0 + 8


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_every_step_and_half_is_owned_exactly_once(shape):
    c, b, h, w = shape
    n = b * ((h * w + 31) // 32)
    owned = {}
    for block in range(GRID):
        worker, half = pair_slot(block)
        for s in range(first_step(n, worker), first_step(n, worker + 1)):
            owned[s, half] = owned.get((s, half), 0) + 1
    assert sorted(owned) == [(s, half) for s in range(n) for half in (0, 1)]
    assert set(owned.values()) == {1}


def straddling(b, h, w):
    sps = (h * w + 31) // 32
    n = b * sps
    return [(k, first_step(n, k), first_step(n, k + 1)) for k in range(WORKERS)
            if first_step(n, k + 1) > first_step(n, k) and first_step(n, k) // sps != (first_step(n, k + 1) - 1) // sps]


def test_the_shapes_exercise_what_their_table_says():
    """steps per shape, workers that straddle a sample boundary, idle workers -- with the kernel's own partition"""
    steps = {s: s[1] * ((s[2] * s[3] + 31) // 32) for s in SHAPES}
    assert [steps[s] for s in SHAPES] == [135, 196, 36, 48, 384, 939, 339]
    assert [k for k, _, _ in straddling(3, 64, 64)] == [42, 85]
    assert [k for k, _, _ in straddling(3, 100, 100)] == [42, 85] and (100 * 100) % 32 != 0
    assert (85, 225, 227) in straddling(3, 60, 60) and (60 * 60) % 32 != 0
    assert steps[(128, 2, 20, 28)] < WORKERS and steps[(256, 6, 12, 20)] < WORKERS


# ---- the images ----------------------------------------------------------------------------------------------------------------
def stage_lanes(c):
    """(wave, lane, g, q) of a workgroup of c / 32 waves"""
    for wv in range(c // 32):
        for lane in range(64):
            yield wv, lane, lane >> 3, lane & 7


@pytest.mark.parametrize('c', (128, 256))
def test_d_image_holds_the_data_gradients_b_operand(c):
    """writer: lane (g, q) of wave wv, rows co = 32 wv + 4 g .. + 3 of pixel 4 q + e, 8 bytes per part; reader: lane l of k-step ks
    holds gy[co = 32 ks + 8 (l >> 4) + j][pixel of column l & 15 of pixel half nt], j = 0..7 in byte order"""
    img = {}
    for wv, lane, g, q in stage_lanes(c):
        for e in range(4):
            for part in range(2):
                at = d_write(32 * wv + 4 * g, 4 * q + e, part)
                for j in range(4):
                    for byte in range(2):
                        key = at + 2 * j + byte
                        assert key not in img
                        img[key] = (32 * wv + 4 * g + j, 4 * q + e, part)
    assert sorted(img) == list(range(128 * c))
    for ks in range(c // 32):
        for part in range(2):
            for nt in range(2):
                for lane in range(64):
                    at = d_read(ks, part, nt, lane)
                    col = lane & 15
                    pixel = 4 * (col & 7) + 2 * nt + (col >> 3)      # the epilogue's patch column of MFMA column `col`
                    for j in range(8):
                        assert img[at + 2 * j] == (32 * ks + 8 * (lane >> 4) + j, pixel, part)


@pytest.mark.parametrize('c', (128, 256))
def test_weight_gradient_images_hold_both_operands_in_one_pixel_order(c):
    a_img, b_img = {}, {}
    for wv, lane, g, q in stage_lanes(c):
        for part in range(2):
            for j in range(4):                                        # A: rows co of g, y
                co = 32 * wv + 4 * g + j
                at = a_write(c, co, q, part)
                for e in range(4):
                    assert at + 2 * e not in a_img
                    a_img[at + 2 * e] = (co, 4 * q + e, part)
            for k in range(2):                                        # B: rows ci of y1, of this CU's half
                ci = 16 * wv + g + 8 * k
                at = b_write(c, ci, q, part)
                for e in range(4):
                    assert at + 2 * e not in b_img
                    b_img[at + 2 * e] = (ci, 4 * q + e, part)
    assert sorted(a_img) == list(range(0, 128 * c, 2)) and sorted(b_img) == list(range(0, 64 * c, 2))
    for kk in range(2):
        for part in range(2):
            for lane in range(64):
                pixels = [16 * kk + 8 * (lane >> 5) + j for j in range(8)]
                for tile in range(c // 32):
                    at = a_read(c, kk, tile, part, lane)
                    assert [a_img[at + 2 * j] for j in range(8)] == [(32 * tile + (lane & 31), p, part) for p in pixels]
                for tile in range(c // 64):
                    at = b_read(c, kk, tile, part, lane)
                    assert [b_img[at + 2 * j] for j in range(8)] == [(32 * tile + (lane & 31), p, part) for p in pixels]


@pytest.mark.parametrize('c', (128, 256))
def test_every_lds_access_of_the_step_is_bank_conflict_free(c):
    g0 = [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27]
    g1 = [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]
    read_groups = [g0, g1, [x + 32 for x in g0], [x + 32 for x in g1]]

    def free(addrs, words, mod):
        banks = [(a // 4 + w) % mod for a in addrs for w in range(words)]
        return len(banks) == len(set(banks))

    for wv in range(c // 32):
        for l0 in range(0, 64, 16):
            lanes = [(lane >> 3, lane & 7) for lane in range(l0, l0 + 16)]
            for part in range(2):
                for e in range(4):
                    assert free([d_write(32 * wv + 4 * g, 4 * q + e, part) for g, q in lanes], 2, 32), ('D write', wv, l0, e)
                for j in range(4):
                    assert free([a_write(c, 32 * wv + 4 * g + j, q, part) for g, q in lanes], 2, 32), ('A write', wv, l0, j)
                for k in range(2):
                    assert free([b_write(c, 16 * wv + g + 8 * k, q, part) for g, q in lanes], 2, 32), ('B write', wv, l0, k)
    for grp in read_groups:
        for part in range(2):
            for ks in range(c // 32):
                for nt in range(2):
                    assert free([d_read(ks, part, nt, lane) for lane in grp], 4, 64), ('D read', ks, nt)
            for kk in range(2):
                for tile in range(c // 32):
                    assert free([a_read(c, kk, tile, part, lane) for lane in grp], 4, 64), ('A read', kk, tile)
                for tile in range(c // 64):
                    assert free([b_read(c, kk, tile, part, lane) for lane in grp], 4, 64), ('B read', kk, tile)


# ---- the mirrors against the header ---------------------------------------------------------------------------------------------
def test_the_mirrors_are_the_header(tmp_path):
    src = open(HEADER).read()
    m = re.search(r'struct PairSlot \{[^}]*\};\n.*?__host__ __device__ inline int pair_b_read\(.*?\n\}\n', src, re.S)
    assert m, 'pair_slot .. pair_b_read not found in sfa_gemm_pair.h'
    stage = open(os.path.join(CSRC, 'sfa_stage.hip')).read()
    fs = re.search(r'__host__ __device__ inline long long wg_first_step\(.*?\}\n', stage)
    assert fs, 'wg_first_step not found in sfa_stage.hip'
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    args = [cxx] if cxx else [os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-x', 'c++']
    prog = ('#include <cstdio>\n#define __host__\n#define __device__\n' + fs.group(0) + m.group(0) +
            'int main() {\n'
            '  for (int b = 0; b < 256; ++b) { PairSlot s = pair_slot(b); printf("%d %d\\n", s.worker, s.half); }\n'
            '  for (long long n = 0; n < 1000; n += 37) for (int w = 0; w <= 128; ++w) printf("%lld\\n", wg_first_step(n, w, 128));\n'
            '  for (int c = 128; c <= 256; c += 128) for (int part = 0; part < 2; ++part) {\n'
            '    for (int co = 0; co < c; co += 4) for (int p = 0; p < 32; ++p) printf("%d\\n", pair_d_write(co, p, part));\n'
            '    for (int ks = 0; ks < c / 32; ++ks) for (int nt = 0; nt < 2; ++nt) for (int l = 0; l < 64; ++l) printf("%d\\n", pair_d_read(ks, part, nt, l));\n'
            '    for (int r = 0; r < c; ++r) for (int q = 0; q < 8; ++q) printf("%d\\n", pair_a_write(c, r, q, part));\n'
            '    for (int r = 0; r < c / 2; ++r) for (int q = 0; q < 8; ++q) printf("%d\\n", pair_b_write(c, r, q, part));\n'
            '    for (int kk = 0; kk < 2; ++kk) for (int l = 0; l < 64; ++l) {\n'
            '      for (int t = 0; t < c / 32; ++t) printf("%d\\n", pair_a_read(c, kk, t, part, l));\n'
            '      for (int t = 0; t < c / 64; ++t) printf("%d\\n", pair_b_read(c, kk, t, part, l));\n'
            '    }\n'
            '  }\n  return 0;\n}\n')
    (tmp_path / 'pair.cpp').write_text(prog)
    exe = str(tmp_path / 'pair')
    subprocess.run(args + ['-O1', str(tmp_path / 'pair.cpp'), '-o', exe], check=True, capture_output=True, timeout=120)
    got = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split('\n')
    want = ['%d %d' % pair_slot(b) for b in range(256)]
    want += [str(first_step(n, w)) for n in range(0, 1000, 37) for w in range(129)]
    for c in (128, 256):
        for part in range(2):
            want += [str(d_write(co, p, part)) for co in range(0, c, 4) for p in range(32)]
            want += [str(d_read(ks, part, nt, l)) for ks in range(c // 32) for nt in range(2) for l in range(64)]
            want += [str(a_write(c, r, q, part)) for r in range(c) for q in range(8)]
            want += [str(b_write(c, r, q, part)) for r in range(c // 2) for q in range(8)]
            for kk in range(2):
                for l in range(64):
                    want += [str(a_read(c, kk, t, part, l)) for t in range(c // 32)]
                    want += [str(b_read(c, kk, t, part, l)) for t in range(c // 64)]
    assert got[:-1] == want and got[-1] == ''


def test_pair_kernel_builds_for_gfx950_without_private_memory(tmp_path):
    """both instantiations: ScratchSize 0, at most 256 registers (two waves per SIMD at C = 256), the LDS plan within 160 KB"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    (tmp_path / 'pair.hip').write_text(
        '#include "sfa_gemm_pair.h"\nusing namespace dhd_sfa;\n'
        'struct FS { __host__ __device__ long long operator()(long long n, long long w, long long W) const { return n * w / W; } };\n'
        'template __global__ void dhd_sfa::pw_pair_kernel<256, 2, FS>(PairArgs);\n'
        'template __global__ void dhd_sfa::pw_pair_kernel<128, 2, FS>(PairArgs);\n')
    p = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-I', CSRC, '-I', os.path.join(ROOT, 'include'),
                        '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c', str(tmp_path / 'pair.hip'), '-o', str(tmp_path / 'pair.o')],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    blocks = re.findall(r'Function Name: (\S*pw_pair_kernel\S*).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)', p.stderr, re.S)
    assert len(blocks) == 2, p.stderr[-2000:]
    for name, vgprs, agprs, scratch in blocks:
        assert int(scratch) == 0, (name, scratch)
        assert int(vgprs) + int(agprs) <= 256, (name, vgprs, agprs)
    for c in (128, 256):
        assert 128 * c + 128 * c + 64 * c + (c // 32) * 16 * 36 * 4 + 3 * c * 4 <= 160 * 1024
