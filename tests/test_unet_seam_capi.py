"""The UNet-seam surface `dhdn_*` of libdhd_amd.so (dhd_amd/capi_unet/dhd_amd_unet_seam.h, dhd_amd/_unet_seam.py) without a GPU:
its own copies of the guarantees tests/test_capi.py holds for the `dhd_*` surface -- header, binding table and exports agree;
every entry point refuses bad input on the host with the documented code -- plus the truth tables, the scratch sizes, the build
wiring and the switch on the CPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPI = os.path.join(ROOT, 'dhd_amd', 'capi_unet')
HEADER = os.path.join(CAPI, 'dhd_amd_unet_seam.h')
CSRC = os.path.join(ROOT, 'dhd_amd', 'csrc')
EINVAL, ENOSPACE, EUNSUPPORTED = -1, -2, -3
WANT = ['dhdn_max_pool2_backward', 'dhdn_max_pool2_forward', 'dhdn_max_pool2_supported', 'dhdn_up_cat_backward', 'dhdn_up_cat_forward',
        'dhdn_up_cat_scratch_bytes', 'dhdn_up_cat_supported']
CTYPE = {'int': C.c_int, 'size_t': C.c_size_t}


def _prototypes():
    """name -> (argtypes, restype) as the header declares them."""
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r'\b(int|size_t)\s+(dhdn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        types = []
        for a in args.split(','):
            a = a.strip()
            types.append(C.c_void_p if '*' in a else CTYPE[re.sub(r'\s+\w+$', '', a).replace('const ', '').strip()])
        out[name] = (types, CTYPE[ret])
    return out


def test_header_binding_table_and_exports_agree():
    from dhd_amd import _ext, _lib, _optim, _seam, _unet_seam
    protos = _prototypes()
    assert len(WANT) == 7 and sorted(protos) == WANT == sorted(_unet_seam.EXPORTED_SYMBOLS)
    for name, (argtypes, restype) in _unet_seam._PROTOTYPES.items():
        assert (argtypes, restype) == protos[name], name                 # the table is the header, argument by argument
    lib = _unet_seam.load()
    assert lib is _lib.load()                                            # the same library, the same handle
    for name, (argtypes, restype) in _unet_seam._PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r' T (dhdn_[a-z0-9_]+)', out)) == set(WANT)
    for table in (_lib._PROTOTYPES, _ext._PROTOTYPES, _seam._PROTOTYPES, _optim._PROTOTYPES):
        assert not any(n.startswith('dhdn') for n in table)
    assert _lib.ABI_VERSION == 6 and lib.dhd_abi_version() == 6
    text = open(HEADER).read()
    assert '#include "dhd_amd.h"' in text and 'DHD_ABI_VERSION is unchanged' in text
    assert os.listdir(CAPI) == ['dhd_amd_unet_seam.h']
    # the constants: header, kernels and binding state the same values
    kern = open(os.path.join(CSRC, 'unet_seam.h')).read()
    for name, val in (('DHDN_NCHW', _unet_seam.NCHW), ('DHDN_NHWC', _unet_seam.NHWC), ('DHDN_UP_ROWS', _unet_seam.UP_ROWS),
                      ('DHDN_UP_COLS', _unet_seam.UP_COLS)):
        for src in (text, kern):
            assert re.search(rf'#define {name} {val}\b', src), name


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / 'h.c'
    src.write_text('#include "dhd_amd_unet_seam.h"\nint main(void) { return dhdn_max_pool2_supported(DHD_F16, DHDN_NHWC, 1, 8, 2, 2) '
                   '&& dhdn_up_cat_scratch_bytes(DHD_F32, 1, 32, 16, 1, 1, 1) > 0 ? 0 : 1; }\n')
    out = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + os.path.join(ROOT, 'include'),
                          '-I' + CAPI, str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_the_makefile_builds_the_kernels():
    """The kernels are csrc/unet_seam.h, included at the end of upsample.hip (the set of translation units is a closed list held
    by other tests, so the family adds none); a change of either header rebuilds."""
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith('SRCS')).split(':=')[1].split()
    assert len(srcs) == 22 and 'upsample.hip' in srcs and not [f for f in os.listdir(CSRC) if f.endswith('.hip') and 'unet' in f]
    rule = next(ln for ln in mk.splitlines() if ln.startswith('%.o:')).split()
    assert 'unet_seam.h' in rule and '../capi_unet/dhd_amd_unet_seam.h' in rule and 'sfa_mfma.h' in rule and 'vec16.h' in rule
    up = open(os.path.join(CSRC, 'upsample.hip')).read()
    assert up.count('#include "unet_seam.h"') == 1 and up.rstrip().endswith('#include "unet_seam.h"')     # after everything of its own
    kern = open(os.path.join(CSRC, 'unet_seam.h')).read()
    assert 'namespace dhd_unet {' in kern and 'store_b128_guarded' in kern and kern.count('pool_winner(float') == 1
    assert not re.search(r'atomic', kern.replace('no atomics', ''))


def test_supported_truth_tables():
    from dhd_amd import _unet_seam
    lib = _unet_seam.load()
    for dt in (0, 1, 2):
        for c in range(-8, 80):
            assert lib.dhdn_max_pool2_supported(dt, 1, 2, c, 5, 7) == int(c >= 8 and c % 8 == 0), c
            assert lib.dhdn_max_pool2_supported(dt, 0, 2, c, 5, 7) == int(c >= 1), c
        for h, w, ok in ((2, 2, 1), (1, 2, 0), (2, 1, 0), (3, 3, 1), (0, 4, 0)):
            assert lib.dhdn_max_pool2_supported(dt, 0, 1, 8, h, w) == ok and lib.dhdn_max_pool2_supported(dt, 1, 1, 8, h, w) == ok
    assert lib.dhdn_max_pool2_supported(3, 0, 1, 8, 4, 4) == 0 and lib.dhdn_max_pool2_supported(0, 2, 1, 8, 4, 4) == 0
    assert lib.dhdn_max_pool2_supported(0, 0, 1 << 20, 1 << 10, 1 << 6, 1 << 6) == 0                 # 2^42 elements
    up = lib.dhdn_up_cat_supported
    for dt in (0, 1, 2):
        for cin in range(0, 1100, 8):
            assert up(dt, 1, 2, cin, 16, 8, 3, 5, 6, 10) == int(32 <= cin <= 1024 and cin % 32 == 0), cin
        for cout in range(0, 560, 8):
            assert up(dt, 1, 2, 32, cout, 8, 3, 5, 6, 10) == int(16 <= cout <= 512 and cout % 16 == 0), cout
        for c2 in range(0, 64, 4):
            assert up(dt, 1, 2, 32, 16, c2, 3, 5, 6, 10) == int(c2 >= 8 and c2 % 8 == 0), c2
        assert up(dt, 0, 2, 32, 16, 8, 3, 5, 6, 10) == 0                                               # NCHW: today's path
        assert up(dt, 1, 2, 32, 16, 8, 3, 5, 5, 10) == 0 and up(dt, 1, 2, 32, 16, 8, 3, 5, 6, 9) == 0  # x2 smaller than 2 x x1
        assert up(dt, 1, 2, 32, 16, 8, 3, 5, 9, 12) == 1
    assert up(3, 1, 2, 32, 16, 8, 3, 5, 6, 10) == 0
    assert up(0, 1, 64, 1024, 512, 512, 100, 100, 200, 200) == 0 and up(1, 1, 4, 128, 64, 64, 100, 100, 200, 200) == 1   # 2^31 bytes


def test_scratch_bytes():
    from dhd_amd import _unet_seam
    f = _unet_seam.load().dhdn_up_cat_scratch_bytes
    for dt, parts in ((0, 2), (1, 1), (2, 1)):
        for b, cin, cout, h, w in ((1, 32, 16, 1, 1), (4, 1024, 512, 12, 12), (4, 128, 64, 100, 100), (3, 160, 80, 9, 8)):
            pack = parts * 4 * cout * cin * 2
            tiles = -(-b * h * w // _unet_seam.UP_ROWS)
            assert f(dt, b, cin, cout, h, w, 0) == pack and f(dt, b, cin, cout, h, w, 1) == pack + -(-tiles * cout * 4 // 16) * 16
    assert f(1, 1, 40, 16, 1, 1, 0) == 0 and f(1, 1, 32, 24, 1, 1, 1) == 0 and f(3, 1, 32, 16, 1, 1, 0) == 0 and f(1, 0, 32, 16, 1, 1, 0) == 0


def test_bad_input_is_refused_on_the_host():
    """Fake addresses, no device: every call below returns before any launch."""
    from dhd_amd import _unet_seam
    lib = _unet_seam.load()
    P = C.c_void_p(0x10000)
    pf = [P, P, 1, 1, 2, 8, 5, 7, None]                                        # x y | dtype layout b c h w
    pb = [P, P, P, 1, 1, 2, 8, 5, 7, None]
    uf = [P, P, P, 0, P, P, P, 1 << 24, 1, 1, 2, 32, 16, 8, 3, 5, 6, 10, None]     # x1 x2 w wdtype bias out scratch bytes | dtype layout b cin cout c2 h w H W
    ub = [P, P, 0, P, P, P, P, P, 1 << 24, 1, 1, 2, 32, 16, 8, 3, 5, 6, 10, None]  # gout w wdtype gx1 gx2 gop dbias scratch bytes | ...
    table = ((lib.dhdn_max_pool2_forward, pf, (0, 1), range(4, 8), 5, (2,), 3),
             (lib.dhdn_max_pool2_backward, pb, (0, 1, 2), range(5, 9), 6, (3,), 4),
             (lib.dhdn_up_cat_forward, uf, (0, 1, 2, 5, 6), range(10, 18), 11, (3, 8), 9),
             (lib.dhdn_up_cat_backward, ub, (0, 1, 3, 7), range(11, 19), 12, (2, 9), 10))
    for fn, args, ptrs, sizes, c_at, dts, layout_at in table:
        def with_(at, val):
            a = list(args)
            a[at] = val
            return fn(*a)
        for s in ptrs:
            for bad in (None, C.c_void_p(0x10004), C.c_void_p(0x10002)):
                assert with_(s, bad) == EINVAL, (fn.__name__, s, bad)
        for s in sizes:
            assert with_(s, 0) == EINVAL and with_(s, -1) == EINVAL, (fn.__name__, s)
        assert with_(c_at, 12) == EUNSUPPORTED, fn.__name__
        for s in dts:
            for bad in (3, -1):
                assert with_(s, bad) == EUNSUPPORTED, (fn.__name__, s, bad)
        assert with_(layout_at, 2) == EUNSUPPORTED
        a = list(args)                                                            # the pointer test comes first
        a[0], a[c_at] = None, 12
        assert fn(*a) == EINVAL
    # optional pointers may be NULL but not misaligned
    for at in (4, 5, 6):
        a = list(ub)
        a[at] = C.c_void_p(0x10002)
        assert lib.dhdn_up_cat_backward(*a) == EINVAL
    a = list(uf)
    a[4] = C.c_void_p(0x10002)
    assert lib.dhdn_up_cat_forward(*a) == EINVAL
    # the up seam takes channels_last only; scratch one byte short is refused, after the shape checks
    a = list(uf)
    a[9] = 0
    assert lib.dhdn_up_cat_forward(*a) == EUNSUPPORTED
    for fn, args, at, bwd in ((lib.dhdn_up_cat_forward, uf, 7, 0), (lib.dhdn_up_cat_backward, ub, 8, 1)):
        need = lib.dhdn_up_cat_scratch_bytes(1, 2, 32, 16, 3, 5, bwd)
        assert need > 0
        for short in (0, 7, need - 1):
            a = list(args)
            a[at] = short
            assert fn(*a) == ENOSPACE, (fn.__name__, short)
        a = list(args)
        a[at], a[11 + bwd] = 0, 40
        assert fn(*a) == EUNSUPPORTED


def test_cpu_tensors_raise_and_the_switch_on_the_cpu_is_todays_path(monkeypatch):
    """CPU tensors handed to the operators raise DhdError (no fallback); with the switch on and every entry routed, a UNet on the
    CPU returns today's bits and no dhdn_* entry point reaches _lib.check."""
    import dhd_amd
    from dhd_amd import _lib, unet_seam
    from dhd_amd.detector import UNet, _Down, _Up
    assert 'DHD_UNET_SEAMS' in os.environ or (_Down.fused_seam is False and _Up.fused_seam is False)
    with pytest.raises(_lib.DhdError):
        dhd_amd.max_pool2x2(torch.rand(2, 8, 4, 4))
    with pytest.raises(_lib.DhdError):
        dhd_amd.conv_transpose2x2_cat(torch.rand(1, 32, 2, 2), torch.rand(1, 8, 4, 4), torch.rand(32, 16, 2, 2))
    assert not dhd_amd.unet_seam_supported(torch.rand(2, 8, 4, 4), 'pool')
    assert not dhd_amd.unet_seam_supported(torch.rand(1, 32, 2, 2), 'up', torch.rand(1, 8, 4, 4), torch.rand(32, 16, 2, 2))
    with pytest.raises(ValueError):
        dhd_amd.unet_seam_supported(torch.rand(2, 8, 4, 4), 'down')
    assert set(k[0] for k in unet_seam.ROUTED) == {'pool', 'up'} and all(isinstance(v, bool) for v in unet_seam.ROUTED.values())
    seen, real = [], _lib.check
    monkeypatch.setattr(_lib, 'check', lambda rc, what: (seen.append(what), real(rc, what))[1])
    monkeypatch.setattr(unet_seam, 'ROUTED', {k: True for k in unet_seam.ROUTED})
    torch.manual_seed(3)
    net = UNet(8, 4)
    x = torch.randn(2, 8, 32, 32)
    outs = {}
    for on in (False, True):
        mods = dhd_amd.fused_unet_seams(net, on)
        assert len(mods) == 8 and all(m.fused_seam is on for m in mods)
        net.zero_grad()
        xi = x.clone().requires_grad_()
        net(xi).sum().backward()
        outs[on] = [xi.grad.clone()] + [p.grad.clone() for p in net.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(outs[False], outs[True]))
    assert not any(w.startswith('dhdn') for w in seen), seen
