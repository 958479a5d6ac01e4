"""The stereo cost volume surface `dhdv_*` of libdhd_amd.so (dhd_amd/capi_stereo/dhd_amd_stereo_cv.h, dhd_amd/_stereo_cv.py)
without a GPU: its own copies of the guarantees tests/test_capi.py holds for the `dhd_*` surface -- header, binding table and
exports agree; every entry point refuses bad input on the host with the documented code -- plus the truth table, the scratch
sizes, the build wiring and the switch on the CPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPI = os.path.join(ROOT, 'dhd_amd', 'capi_stereo')
HEADER = os.path.join(CAPI, 'dhd_amd_stereo_cv.h')
CSRC = os.path.join(ROOT, 'dhd_amd', 'csrc')
EINVAL, ENOSPACE, EUNSUPPORTED = -1, -2, -3
WANT = ['dhdv_stereo_cost_volume', 'dhdv_stereo_cv_scratch_bytes', 'dhdv_stereo_cv_supported', 'dhdv_stereo_grid']
CTYPE = {'int': C.c_int, 'size_t': C.c_size_t, 'float': C.c_float}


def _prototypes():
    """name -> (argtypes, restype) as the header declares them."""
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r'\b(int|size_t)\s+(dhdv_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        types = []
        for a in args.split(','):
            a = a.strip()
            types.append(C.c_void_p if '*' in a else CTYPE[re.sub(r'\s+\w+$', '', a).replace('const ', '').strip()])
        out[name] = (types, CTYPE[ret])
    return out


def test_header_binding_table_and_exports_agree():
    from dhd_amd import _ext, _lib, _optim, _seam, _stereo_cv, _unet_seam
    protos = _prototypes()
    assert len(WANT) == 4 and sorted(protos) == WANT == sorted(_stereo_cv.EXPORTED_SYMBOLS)
    for name, (argtypes, restype) in _stereo_cv._PROTOTYPES.items():
        assert (argtypes, restype) == protos[name], name                 # the table is the header, argument by argument
    lib = _stereo_cv.load()
    assert lib is _lib.load()                                            # the same library, the same handle
    for name, (argtypes, restype) in _stereo_cv._PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r' T (dhdv_[a-z0-9_]+)', out)) == set(WANT)
    for table in (_lib._PROTOTYPES, _ext._PROTOTYPES, _seam._PROTOTYPES, _optim._PROTOTYPES, _unet_seam._PROTOTYPES):
        assert not any(n.startswith('dhdv') for n in table)
    assert _lib.ABI_VERSION == 6 and lib.dhd_abi_version() == 6
    text = open(HEADER).read()
    assert '#include "dhd_amd.h"' in text and 'DHD_ABI_VERSION is unchanged' in text
    assert os.listdir(CAPI) == ['dhd_amd_stereo_cv.h']
    # the constants: header, kernels and binding state the same values
    kern = open(os.path.join(CSRC, 'stereo_cv.h')).read()
    for name, val in (('DHDV_NCHW', _stereo_cv.NCHW), ('DHDV_NHWC', _stereo_cv.NHWC), ('DHDV_MAX_C', _stereo_cv.MAX_C),
                      ('DHDV_MAX_D', _stereo_cv.MAX_D)):
        for src in (text, kern):
            assert re.search(rf'#define {name} {val}\b', src), name


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / 'h.c'
    src.write_text('#include "dhd_amd_stereo_cv.h"\nint main(void) { return dhdv_stereo_cv_supported(DHD_F16, 2, 128, 8, 22, DHDV_MAX_D) '
                   '&& dhdv_stereo_cv_scratch_bytes(DHD_F32, DHDV_NCHW, 1, 32, 16, 1) > 0 ? 0 : 1; }\n')
    out = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + os.path.join(ROOT, 'include'),
                          '-I' + CAPI, str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_the_makefile_builds_the_kernels():
    """The kernels are csrc/stereo_cv.h, included at the end of deform.hip behind the kernels they are variants of (the set of
    translation units is a closed list held by other tests, so the family adds none); a change of either header rebuilds."""
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith('SRCS')).split(':=')[1].split()
    assert len(srcs) == 22 and 'deform.hip' in srcs and not [f for f in os.listdir(CSRC) if f.endswith('.hip') and 'stereo' in f]
    rule = next(ln for ln in mk.splitlines() if ln.startswith('%.o:')).split()
    assert 'stereo_cv.h' in rule and '../capi_stereo/dhd_amd_stereo_cv.h' in rule and 'vec16.h' in rule and 'deform_tap.h' in rule
    flags = mk.split('HIPFLAGS ?=')[1].split('SRCS')[0]
    assert '-ffp-contract=off' in flags and '-fhip-fp32-correctly-rounded-divide-sqrt' in flags     # the positions are gen_grid's bits
    dh = open(os.path.join(CSRC, 'deform.hip')).read()
    assert dh.count('#include "stereo_cv.h"') == 1 and dh.rstrip().endswith('#include "stereo_cv.h"')     # after everything of its own
    kern = open(os.path.join(CSRC, 'stereo_cv.h')).read()
    assert 'namespace dhd_stereo {' in kern and kern.count('void stereo_position(') == 1 and 'fmaf' not in kern
    assert not re.search(r'atomic', kern.replace('No atomics', ''))


def test_supported_truth_table_and_scratch_bytes():
    from dhd_amd import _stereo_cv
    lib = _stereo_cv.load()
    sup, scratch = lib.dhdv_stereo_cv_supported, lib.dhdv_stereo_cv_scratch_bytes
    for c in range(-8, 1100):
        assert sup(0, 2, c, 8, 22, 12) == int(1 <= c <= 1024 and c % 4 == 0), c
        for dt in (1, 2):
            assert sup(dt, 2, c, 8, 22, 12) == int(1 <= c <= 1024 and c % 8 == 0), (dt, c)
    for dt in (0, 1, 2):
        for d in range(-1, 300):
            assert sup(dt, 2, 64, 8, 22, d) == int(1 <= d <= 256), d
        assert sup(dt, 0, 64, 8, 22, 12) == 0 and sup(dt, 2, 64, 0, 22, 12) == 0 and sup(dt, 2, 64, 8, 0, 12) == 0
        # bn D h w against 2^31: 12 x 88 x 128 x 352 = 47.6 M cells is the DHD-L size
        assert sup(dt, 12, 128, 128, 352, 88) == 1
        assert sup(dt, 1 << 11, 64, 1 << 10, 1 << 2, 1 << 8) == 0 and sup(dt, (1 << 11) - 1, 64, 1 << 10, 1 << 2, 1 << 8) == 1
    assert sup(3, 2, 64, 8, 22, 12) == 0 and sup(-1, 2, 64, 8, 22, 12) == 0
    for dt, size in ((0, 4), (1, 2), (2, 2)):
        for bn, c, h, w in ((2, 64, 8, 22), (1, 8, 5, 7), (12, 128, 128, 352), (3, 520, 3, 3)):
            one = -(-bn * c * h * w * size // 16) * 16
            assert scratch(dt, 0, bn, c, h, w) == 2 * one and scratch(dt, 1, bn, c, h, w) == 0
        assert scratch(dt, 0, 2, 12 if size == 2 else 6, 8, 22) == 0 and scratch(dt, 2, 2, 64, 8, 22) == 0
    assert scratch(3, 0, 2, 64, 8, 22) == 0


def test_bad_input_is_refused_on_the_host():
    """Fake addresses, no device: every call below returns before any launch."""
    from dhd_amd import _stereo_cv
    lib = _stereo_cv.load()
    P = C.c_void_p(0x10000)
    # six view arrays, u v dep, grid | bn h w n_depth hi wi | stream
    ga = [P] * 10 + [2, 8, 22, 12, 32, 88, None]
    # prev curr out | dtype layout | six view arrays, u v dep | bn c h w n_depth hi wi | bias flag_channel | scratch bytes stream
    ca = [P, P, P, 1, 1] + [P] * 9 + [2, 64, 8, 22, 12, 32, 88, 5.0, 60, P, 1 << 24, None]

    def with_(fn, args, at, val):
        a = list(args)
        a[at] = val
        return fn(*a)

    grid, cv = lib.dhdv_stereo_grid, lib.dhdv_stereo_cost_volume
    for s in range(10):
        for bad in (None, C.c_void_p(0x10002)):
            assert with_(grid, ga, s, bad) == EINVAL, (s, bad)
    assert with_(grid, ga, 9, C.c_void_p(0x10004)) == EINVAL            # the grid is written as float2
    for s in range(10, 16):
        assert with_(grid, ga, s, 0) == EINVAL and with_(grid, ga, s, -1) == EINVAL, s
    assert with_(grid, ga, 14, 1) == EINVAL and with_(grid, ga, 15, 1) == EINVAL     # hi - 1, wi - 1 divide
    assert with_(grid, ga, 13, 257) == EUNSUPPORTED and with_(grid, ga, 10, 1 << 24) == EUNSUPPORTED
    a = list(ga)
    a[0], a[13] = None, 257
    assert grid(*a) == EINVAL                                                # the pointer test comes first

    for s in (0, 1, 2) + tuple(range(5, 14)):
        for bad in (None, C.c_void_p(0x10002)):
            assert with_(cv, ca, s, bad) == EINVAL, (s, bad)
    for s in (0, 1):
        assert with_(cv, ca, s, C.c_void_p(0x10008)) == EINVAL            # 16-byte channel groups
    assert with_(cv, ca, 23, C.c_void_p(0x10008)) == EINVAL
    for s in range(14, 21):
        assert with_(cv, ca, s, 0) == EINVAL and with_(cv, ca, s, -1) == EINVAL, s
    assert with_(cv, ca, 19, 1) == EINVAL and with_(cv, ca, 20, 1) == EINVAL
    for dt in (0, 1, 2):
        a = list(ca)
        a[3] = dt
        for c in (12 if dt else 6, 1032):
            a[15], a[22] = c, 0
            assert cv(*a) == EUNSUPPORTED, (dt, c)
        a[15], a[22] = 64, 60
        assert with_(cv, a, 18, 257) == EUNSUPPORTED and with_(cv, a, 14, 1 << 24) == EUNSUPPORTED
        assert with_(cv, a, 22, 64) == EUNSUPPORTED and with_(cv, a, 22, -1) == EUNSUPPORTED
    assert with_(cv, ca, 3, 3) == EUNSUPPORTED and with_(cv, ca, 3, -1) == EUNSUPPORTED and with_(cv, ca, 4, 2) == EUNSUPPORTED
    a = list(ca)
    a[0], a[15] = None, 12
    assert cv(*a) == EINVAL                                                  # the pointer test comes first
    # scratch: none needed where the maps are read in place; one byte short is refused, after the shape checks
    a = list(ca)
    a[23], a[24] = None, 0
    a[15] = 12
    assert cv(*a) == EUNSUPPORTED
    need = lib.dhdv_stereo_cv_scratch_bytes(1, 0, 2, 64, 8, 22)
    assert need == 2 * 2 * 64 * 8 * 22 * 2
    for short in (0, 15, need - 1):
        a = list(ca)
        a[4], a[24] = 0, short
        assert cv(*a) == ENOSPACE, short
    a = list(ca)
    a[4], a[23] = 0, None
    assert cv(*a) == EINVAL


def test_cpu_tensors_raise_and_the_switch_on_the_cpu_is_todays_path(monkeypatch):
    """CPU tensors handed to the operators raise DhdError (no fallback); with the switch off, and with it on and every entry
    routed, a DepthNet on the CPU returns today's bits and no dhdv_* entry point reaches _lib.check."""
    import dhd_amd
    import stereo_cv_inputs as inp
    from dhd_amd import _lib, stereo_cv
    from dhd_amd.depthnet import _LiftNetBase
    assert 'DHD_STEREO_CV' in os.environ or _LiftNetBase.fused_cost_volume is False
    m = inp.metas('a', 12)
    prev, curr = inp.features(16, 8, 22)
    cal = (m['post_rots'], m['post_trans'], m['intrins'], m['k2s_sensor'])
    with pytest.raises(_lib.DhdError):
        dhd_amd.stereo_cost_volume(prev, curr, m['frustum'], *cal, 5.0, 12)
    with pytest.raises(_lib.DhdError):
        dhd_amd.stereo_sampling_grid(m['frustum'], *cal, 32, 88)
    assert not dhd_amd.stereo_cv_supported(prev, curr, m['frustum'], *cal)
    assert set(stereo_cv.ROUTED) == {(cls, dt) for cls in ('c128', 'c256', 'c512', 'c1024')
                                     for dt in (torch.float32, torch.float16, torch.bfloat16)}
    assert all(isinstance(v, bool) for v in stereo_cv.ROUTED.values())
    assert [stereo_cv.channel_class(c) for c in (8, 128, 132, 256, 264, 512, 520, 1024)] == ['c128', 'c128', 'c256', 'c256', 'c512', 'c512',
                                                                                            'c1024', 'c1024']
    seen, real = [], _lib.check
    monkeypatch.setattr(_lib, 'check', lambda rc, what: (seen.append(what), real(rc, what))[1])
    monkeypatch.setattr(stereo_cv, 'ROUTED', {k: True for k in stereo_cv.ROUTED})
    dn = inp.depthnet(12, 5.0)
    m['cv_feat_list'] = [prev, curr]
    outs = {}
    for on in (False, True):
        mods = dhd_amd.fused_stereo_cost_volume(dn, on)
        assert mods == [dn] and dn.fused_cost_volume is on
        outs[on] = dn.calculate_cost_volumn(m)
    assert torch.equal(outs[False], outs[True])
    assert not any(w.startswith('dhdv') for w in seen), seen
    # the frustum axes: separable templates give (u, v, dep) in float32, anything else None
    u, v, dep = stereo_cv.frustum_axes(m['frustum'])
    assert torch.equal(u, m['frustum'][0, 0, :, 0]) and torch.equal(v, m['frustum'][0, :, 0, 1]) and torch.equal(dep, m['frustum'][:, 0, 0, 2])
    half = m['frustum'].to(torch.bfloat16)
    assert all(a.dtype == torch.float32 and torch.equal(a, b.float()) for a, b in
               zip(stereo_cv.frustum_axes(half), (half[0, 0, :, 0], half[0, :, 0, 1], half[:, 0, 0, 2])))
    broken = m['frustum'].clone()
    broken[3, 2, 5, 1] += 1.0
    assert stereo_cv.frustum_axes(broken) is None and stereo_cv.frustum_axes(m['frustum'][..., :2]) is None
