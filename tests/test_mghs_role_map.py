"""role_of_group (dhd_amd/csrc/mghs_layout.h): which role a group of 8 consecutive workgroups of a merged MGHS launch plays
(DHD_MGHS_BY_GRID: a streaming role and a point role in one launch, mghs_fwd_bands_g0sums).  On the CPU: the function is pure,
so it is mirrored here in Python, and the mirror is held against the header's own text compiled as a host program.

For counts including 0 of either role: every stream group and every point group is named exactly once, in increasing order;
the point groups lie evenly among the stream groups; a group's 8 workgroups keep blockIdx & 7 = 0..7 in the index the bodies
are given."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'dhd_amd', 'csrc', 'mghs_layout.h')
COUNTS = [(s, p) for s in (0, 1, 2, 3, 7, 8, 50, 1600) for p in (0, 1, 2, 5, 33, 182) if s + p > 0]


def role_of_group(g, n_stream, n_point):
    """The mirror: (point?, index among the groups of its role)."""
    n = n_stream + n_point
    before, upto = g * n_point // n, (g + 1) * n_point // n
    return (1, before) if upto > before else (0, g - before)


@pytest.mark.parametrize('n_stream,n_point', COUNTS)
def test_every_group_of_either_role_is_named_exactly_once(n_stream, n_point):
    roles = [role_of_group(g, n_stream, n_point) for g in range(n_stream + n_point)]
    assert [i for p, i in roles if p] == list(range(n_point))
    assert [i for p, i in roles if not p] == list(range(n_stream))


@pytest.mark.parametrize('n_stream,n_point', COUNTS)
def test_point_groups_lie_evenly_among_the_stream_groups(n_stream, n_point):
    """Among the first g groups there are floor(g * n_point / n) point groups: never more than one off the even share, so both
    kinds are being started from the first group of the launch to the last."""
    n = n_stream + n_point
    seen = 0
    for g in range(n):
        assert seen == g * n_point // n
        assert abs(seen - g * n_point / n) < 1
        seen += role_of_group(g, n_stream, n_point)[0]
    assert seen == n_point


def test_workgroups_of_a_group_keep_their_xcd():
    """The merged kernel hands the streaming body (index << 3) | (blockIdx & 7).  A point body is written for workgroups of
    kBlock threads, of which a merged workgroup holds k: part `part` of it gets ((k * index + part) << 3) | (blockIdx & 7).  The 8
    workgroups of a group stay one per XCD (x = 0..7), and every body index is produced exactly once."""
    n_stream, n_point, k = 5, 3, 2
    stream, point = [], []
    for block in range((n_stream + n_point) * 8):
        grp, x = block >> 3, block & 7
        is_point, index = role_of_group(grp, n_stream, n_point)
        if is_point:
            for part in range(k):
                b = ((k * index + part) << 3) | x
                assert b & 7 == x
                point.append(b)
        else:
            b = (index << 3) | x
            assert b & 7 == x
            stream.append(b)
    assert sorted(stream) == list(range(n_stream * 8))
    assert sorted(point) == list(range(k * n_point * 8))


def test_the_mirror_is_the_header(tmp_path):
    """The struct and the function are cut out of mghs_layout.h and compiled as host code; the program prints every group's
    role for the counts above."""
    src = open(HEADER).read()
    m = re.search(r'struct RoleSlot \{[^}]*\};\n__host__ __device__ inline RoleSlot role_of_group\(.*?\n\}\n', src, re.S)
    assert m, 'role_of_group not found in mghs_layout.h'
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    args = [cxx] if cxx else [os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-x', 'c++']
    prog = ('#include <cstdio>\n#include <cstdlib>\n#define __host__\n#define __device__\n' + m.group(0) +
            'int main(int argc, char** argv) {\n'
            '  for (int a = 1; a + 1 < argc; a += 2) {\n'
            '    const int s = atoi(argv[a]), p = atoi(argv[a + 1]);\n'
            '    for (int g = 0; g < s + p; ++g) { RoleSlot r = role_of_group(g, s, p); printf("%d %d %d %d %d\\n", s, p, g, r.point, r.index); }\n'
            '  }\n  return 0;\n}\n')
    (tmp_path / 'role.cpp').write_text(prog)
    exe = str(tmp_path / 'role')
    subprocess.run(args + ['-O1', str(tmp_path / 'role.cpp'), '-o', exe], check=True, capture_output=True, timeout=120)
    out = subprocess.run([exe] + [str(v) for c in COUNTS for v in c], check=True, capture_output=True, text=True, timeout=60).stdout
    got = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    want = [(s, p, g) + role_of_group(g, s, p) for s, p in COUNTS for g in range(s + p)]
    assert got == want
