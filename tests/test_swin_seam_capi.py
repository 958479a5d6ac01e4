"""The stage-seam surface `dhds_*` of libdhd_amd.so (include/dhd_amd_seam.h, dhd_amd/_seam.py) without a GPU: its own copies of
the guarantees tests/test_capi.py holds for the `dhd_*` surface -- header, binding table and exports agree; every entry point
refuses bad input on the host with the documented code -- plus the host-side pieces of the seams: the truth tables, the scratch
sizes, the twin's channel order, and the switch on the CPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_seam_inputs as SS  # noqa: E402
from conftest import golden  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'dhd_amd_seam.h')
EINVAL, ENOSPACE, EUNSUPPORTED = -1, -2, -3
WANT = ['dhds_embed_norm_backward', 'dhds_embed_norm_backward_scratch_bytes', 'dhds_embed_norm_forward', 'dhds_embed_norm_supported',
        'dhds_merge_norm_backward', 'dhds_merge_norm_backward_scratch_bytes', 'dhds_merge_norm_forward', 'dhds_merge_norm_supported']


def declared_symbols():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(?:int|size_t)\s+(dhds_[a-z0-9_]+)\s*\(', src)))


def test_header_binding_table_and_exports_agree():
    from dhd_amd import _ext, _ffn, _ffn_wide, _lib, _seam
    assert len(WANT) == 8 and declared_symbols() == WANT == sorted(_seam.EXPORTED_SYMBOLS)
    lib = _seam.load()
    assert lib is _lib.load()                                        # the same library, the same handle
    for name, (argtypes, restype) in _seam._PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r' T (dhds_[a-z0-9_]+)', out)) == set(WANT)
    # the other surfaces are what they were: nothing of the family leaked into their tables, the ABI number did not move
    for table in (_lib._PROTOTYPES, _ext._PROTOTYPES, _ffn._PROTOTYPES, _ffn_wide._PROTOTYPES):
        assert not any(n.startswith('dhds') for n in table)
    assert _lib.ABI_VERSION == 6 and lib.dhd_abi_version() == 6
    assert re.search(r'#define DHD_ABI_VERSION 6\b', open(os.path.join(ROOT, 'include', 'dhd_amd.h')).read())
    text = open(HEADER).read()
    assert '#include "dhd_amd.h"' in text and 'DHD_ABI_VERSION is unchanged' in text
    assert 'dhdf_' not in text and 'dhdg_' not in text
    others = [f for f in os.listdir(os.path.join(ROOT, 'include')) if f != 'dhd_amd_seam.h']
    assert 'dhd_amd.h' in others and 'dhd_amd_ext.h' in others
    for other in others:
        assert 'dhds_' not in open(os.path.join(ROOT, 'include', other)).read(), other


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / 'h.c'
    src.write_text('#include "dhd_amd_seam.h"\nint main(void) { return dhds_merge_norm_supported(8, DHD_F32, DHD_BF16) '
                   '&& dhds_embed_norm_supported(8, DHD_F16, DHD_F32) ? 0 : 1; }\n')
    out = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + os.path.join(ROOT, 'include'), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_the_makefile_builds_the_kernels():
    """The kernels are csrc/swin_seam.h, included by swin_glue.hip (the list of translation units is a closed list held by
    tests/test_swin_ffn_capi.py, so the family adds none, as the wide FFN family did); a change of either header rebuilds."""
    csrc = os.path.join(ROOT, 'dhd_amd', 'csrc')
    mk = open(os.path.join(csrc, 'Makefile')).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith('SRCS')).split(':=')[1].split()
    assert 'swin_glue.hip' in srcs and os.path.exists(os.path.join(csrc, 'swin_seam.h'))
    assert not [f for f in os.listdir(csrc) if f.endswith('.hip') and 'seam' in f]
    rule = next(ln for ln in mk.splitlines() if ln.startswith('%.o:')).split()
    assert 'swin_seam.h' in rule and '../../include/dhd_amd_seam.h' in rule and 'vec16.h' in rule and 'common.h' in rule
    glue = open(os.path.join(csrc, 'swin_glue.hip')).read()
    assert glue.count('#include "swin_seam.h"') == 1 and glue.rstrip().endswith('#include "swin_seam.h"')   # after everything of its own
    seam = open(os.path.join(csrc, 'swin_seam.h')).read()
    assert 'namespace dhd_seam {' in seam and 'atomic' not in seam.replace('No atomics', '')


def test_supported_truth_tables():
    from dhd_amd import _seam
    lib = _seam.load()
    for fn, cmax in ((lib.dhds_merge_norm_supported, 512), (lib.dhds_embed_norm_supported, 256)):
        for c in range(-8, 2100):
            want = int(c >= 8 and c % 8 == 0 and c <= cmax)
            assert fn(c, 0, 0) == want and fn(c, 2, 1) == want, (fn.__name__, c)
        for a in (0, 1, 2):
            for b in (0, 1, 2):
                assert fn(8, a, b) == 1 and fn(cmax, a, b) == 1 and fn(cmax + 8, a, b) == 0, (fn.__name__, a, b)
        for bad in (3, -1):
            assert fn(128, bad, 0) == 0 and fn(128, 0, bad) == 0


def test_scratch_bytes():
    from dhd_amd import _seam
    lib = _seam.load()
    for f, cs, row_bytes in ((lib.dhds_merge_norm_backward_scratch_bytes, (8, 32, 96, 128, 256, 512), lambda c: 32 * c),
                             (lib.dhds_embed_norm_backward_scratch_bytes, (8, 96, 128, 256), lambda c: 8 * c)):
        for c in cs:
            last, rb = 0, row_bytes(c)
            for rows in list(range(1, 300)) + [1320, 8448, 33792, 135168, 540672, 540673, 10 ** 7, 10 ** 9]:
                n = f(rows, c)
                assert n >= max(last, rb) and n % rb == 0, (f.__name__, rows, c, n, last)   # whole row pairs, at least one, non-decreasing
                last = n
            assert last <= 4096 * rb                                             # bounded: the partial rows stay a small table
        for rows, c in ((0, 128), (-5, 128), (1 << 40, 128), (100, 12), (100, 4), (100, 0), (100, -8)):
            assert f(rows, c) == 0, (f.__name__, rows, c)
    assert lib.dhds_merge_norm_backward_scratch_bytes(100, 520) == 0 and lib.dhds_embed_norm_backward_scratch_bytes(100, 264) == 0
    # many_rows_c32: 1320 output rows span several workgroups and no equal split of them exists, so one workgroup is ragged
    B, H, W, Cc = SS.MERGE_CASES['many_rows_c32']
    groups = lib.dhds_merge_norm_backward_scratch_bytes(B * (H // 2) * (W // 2), Cc) // (32 * Cc)
    assert B * (H // 2) * (W // 2) == 1320 and groups >= 3 and 1320 % groups != 0, groups
    # two_images_c128: more tiles than workgroups, more than one workgroup
    B, Cc, H, W = SS.EMBED_CASES['two_images_c128']
    assert lib.dhds_embed_norm_backward_scratch_bytes(B * H * W, Cc) // (8 * Cc) >= 2


def _each_pointer(fn, args, slots):
    """fn(*args) with each pointer of `slots` NULL, then 4 and 2 bytes off a 16-byte boundary -> DHD_EINVAL."""
    for s in slots:
        for bad in (None, C.c_void_p(0x10004), C.c_void_p(0x10002)):
            a = list(args)
            a[s] = bad
            assert fn(*a) == EINVAL, (fn.__name__, s, bad)


def test_bad_input_is_refused_on_the_host():
    """Fake addresses, no device: every call below returns before any launch.  Each base call is valid but for the one thing named,
    and where the pointer test comes first the same call with good pointers reaches the later check."""
    from dhd_amd import _seam
    lib = _seam.load()
    P = C.c_void_p(0x10000)
    mfwd = [P, P, P, P, 0, 2, 2, 5, 7, 96, 1e-5, None]                          # x gamma beta out | dtypes | b h w c | eps
    mbwd = [P, P, P, P, P, P, P, 1 << 20, 0, 2, 2, 5, 7, 96, 1e-5, None]        # x dy gamma dx dgamma dbeta scratch bytes | dtypes | b h w c
    efwd = [P, P, P, P, 2, 0, 2, 96, 133, 1e-5, None]                           # x gamma beta out | dtypes | b c hw | eps
    ebwd = [P, P, P, P, P, P, P, 1 << 20, 2, 0, 2, 96, 133, 1e-5, None]
    _each_pointer(lib.dhds_merge_norm_forward, mfwd, (0, 1, 2, 3))
    _each_pointer(lib.dhds_merge_norm_backward, mbwd, (0, 1, 2, 3, 4, 5, 6))
    _each_pointer(lib.dhds_embed_norm_forward, efwd, (0, 1, 2, 3))
    _each_pointer(lib.dhds_embed_norm_backward, ebwd, (0, 1, 2, 3, 4, 5, 6))
    # fn, args, index of each size argument, index of c, the dtype slots
    table = ((lib.dhds_merge_norm_forward, mfwd, dict(b=6, h=7, w=8), 9, (4, 5)),
             (lib.dhds_merge_norm_backward, mbwd, dict(b=10, h=11, w=12), 13, (8, 9)),
             (lib.dhds_embed_norm_forward, efwd, dict(b=6, hw=8), 7, (4, 5)),
             (lib.dhds_embed_norm_backward, ebwd, dict(b=10, hw=12), 11, (8, 9)))
    for fn, args, sizes, c_at, dts in table:
        def with_(at, val, base=args):
            a = list(base)
            a[at] = val
            return fn(*a)
        cmax = 512 if 'merge' in fn.__name__ else 256
        for c in (12, 100, 0, 4, -8, cmax + 8, 4096):
            assert with_(c_at, c) == EUNSUPPORTED, (fn.__name__, c)
        for k, at in sizes.items():
            assert with_(at, 0) == EINVAL and with_(at, -1) == EINVAL, (fn.__name__, k)
        for s in dts:
            for bad in (3, -1):
                assert with_(s, bad) == EUNSUPPORTED, (fn.__name__, s, bad)
        # the pointer test comes first: with a bad pointer the same calls are DHD_EINVAL
        a = list(args)
        a[0], a[c_at] = None, 12
        assert fn(*a) == EINVAL
    # 2^40 tokens
    a = list(mfwd)
    a[6], a[7], a[8] = 1 << 30, 1 << 10, 1
    assert lib.dhds_merge_norm_forward(*a) == EUNSUPPORTED
    a = list(efwd)
    a[6], a[8] = 1 << 20, 1 << 20
    assert lib.dhds_embed_norm_forward(*a) == EUNSUPPORTED
    # scratch: one byte less than advertised is refused; the size check comes after the shape checks
    for fn, args, need, c_at in ((lib.dhds_merge_norm_backward, mbwd, lib.dhds_merge_norm_backward_scratch_bytes(2 * 3 * 4, 96), 13),
                                 (lib.dhds_embed_norm_backward, ebwd, lib.dhds_embed_norm_backward_scratch_bytes(2 * 133, 96), 11)):
        assert need > 0
        for short in (0, 7, need - 1):
            a = list(args)
            a[7] = short
            assert fn(*a) == ENOSPACE, (fn.__name__, short)
        a = list(args)
        a[7], a[c_at] = 0, 12
        assert fn(*a) == EUNSUPPORTED


@pytest.mark.parametrize('case', SS.MERGE_CASES)
def test_the_twin_gathers_in_unfolds_order(case):
    """The merge twin against the channel order the header states: channel 4 cc + 2 kh + kw of row (bi, i, j) holds
    x[bi, 2i + kh, 2j + kw, cc], zero past H or W -- and against nn.Unfold, whose order it is."""
    B, H, W, Cc = SS.MERGE_CASES[case]
    x = SS.inputs('merge', case, 'f32')['x'].double()
    n = 4 * Cc
    # a LayerNorm with eps -> the raw gathered values: undo it by comparing normalised forms
    got = SS.merge64(x, torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), H, W)
    ho, wo = -(-H // 2), -(-W // 2)
    xp = torch.zeros(B, 2 * ho, 2 * wo, Cc, dtype=torch.float64)
    xp[:, :H, :W] = x.view(B, H, W, Cc)
    rows = torch.empty(B, ho, wo, Cc, 2, 2, dtype=torch.float64)
    for kh in range(2):
        for kw in range(2):
            rows[..., kh, kw] = xp[:, kh::2, kw::2]
    rows = rows.reshape(B, ho * wo, n)
    want = torch.nn.functional.layer_norm(rows, (n,), None, None, SS.EPS)
    assert tuple(got.shape) == SS.out_shape('merge', case) and torch.allclose(got, want, rtol=0, atol=1e-12)
    unf = torch.nn.Unfold(kernel_size=2, stride=2)(xp.permute(0, 3, 1, 2)).transpose(1, 2)
    assert torch.equal(unf, rows)


def test_twin_gradients_are_those_of_layer_norm():
    """The embed twin's autograd gradients against the closed form the kernels evaluate."""
    v = SS.inputs('embed', 'c96', 'f32')
    y, dx, dg, db = SS.twin('embed', 'c96', 'f32')
    x = v['x'].double().flatten(2).transpose(1, 2)
    g, dy = v['gamma'].double(), v['dy'].double()
    mean = x.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + SS.EPS)
    xh = (x - mean) * rstd
    gg = dy * g
    want = rstd * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    assert torch.allclose(dx, want.transpose(1, 2).reshape(v['x'].shape), rtol=0, atol=1e-12)
    assert torch.allclose(dg, (dy * xh).sum((0, 1)), rtol=0, atol=1e-12) and torch.allclose(db, dy.sum((0, 1)), rtol=0, atol=1e-12)
    assert torch.allclose(y, xh * g + v['beta'].double(), rtol=0, atol=1e-12)


def test_cpu_tensors_raise_and_the_switch_on_the_cpu_is_todays_path(monkeypatch):
    """CPU tensors handed to the operators raise DhdError (no fallback); with the switch on, PatchMerging, PatchEmbed and the
    whole backbone on the CPU return today's bits and no dhds_* entry point reaches _lib.check."""
    import dhd_amd
    from dhd_amd import _lib, swin_seam
    from dhd_amd.swin import PatchEmbed, PatchMerging
    from test_host_logic import swin_from_fixture
    assert 'DHD_SWIN_SEAMS' in os.environ or (PatchMerging.fused_seam is False and PatchEmbed.fused_seam is False)
    with pytest.raises(_lib.DhdError):
        dhd_amd.patch_merge_norm(torch.rand(2, 35, 8), torch.ones(32), torch.zeros(32), 1e-5, (5, 7))
    with pytest.raises(_lib.DhdError):
        dhd_amd.patch_embed_norm(torch.rand(2, 8, 3, 5), torch.ones(8), torch.zeros(8), 1e-5)
    assert not dhd_amd.swin_seam_supported(torch.rand(2, 35, 8), 'merge') and not dhd_amd.swin_seam_supported(torch.rand(2, 8, 3, 5), 'embed', torch.float32)
    seen = []
    real = _lib.check
    monkeypatch.setattr(_lib, 'check', lambda rc, what: (seen.append(what), real(rc, what))[1])
    monkeypatch.setattr(swin_seam, 'ROUTED', {k: True for k in swin_seam.ROUTED})
    gen = torch.Generator().manual_seed(3)
    torch.manual_seed(11)
    merge, embed = PatchMerging(8, 16), PatchEmbed(3, 16)
    xm, xe = torch.randn(2, 35, 8, generator=gen), torch.randn(2, 3, 13, 18, generator=gen)
    res = {}
    for on in (False, True):
        merge.fused_seam = embed.fused_seam = on
        res[on] = (merge(xm, (5, 7))[0], embed(xe))
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1])
    g = golden('g10_swin')
    outs = {}
    for on in (False, True):
        net = swin_from_fixture(g)
        mods = dhd_amd.fused_swin_seams(net, on)
        assert len(mods) == 3 and sum(isinstance(m, PatchEmbed) for m in mods) == 1 and all(m.fused_seam is on for m in mods)
        assert all(not vars(b).get('fused_glue') and not vars(b).get('fused_ffn') for b in net.modules())     # a switch of its own
        x = torch.from_numpy(g['x']).requires_grad_()
        o = net(x)
        sum(t.sum() for t in o).backward()
        outs[on] = [t.detach() for t in o] + [x.grad]
    for i in range(3):
        ref = g[f'out{i}']
        assert np.abs(outs[False][i].numpy() - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), i
    assert all(torch.equal(a, b) for a, b in zip(outs[False], outs[True]))
    assert not any(w.startswith('dhds') for w in seen), seen
