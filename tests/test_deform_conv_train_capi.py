"""The deformable convolution's training surface `dhdd_*` of libdhd_amd.so (dhd_amd/capi_deform/dhd_amd_deform_train.h,
dhd_amd/_deform_train.py) without a GPU: header, binding table and exports agree and leave the other surfaces alone; the entry
points refuse bad input on the host with the documented code; the predicate at the edges of the shape family; the switch is off
and sets only itself; the backward kernels use no private memory."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
CAPI = os.path.join(ROOT, 'dhd_amd', 'capi_deform')
CSRC = os.path.join(ROOT, 'dhd_amd', 'csrc')
HEADER = os.path.join(CAPI, 'dhd_amd_deform_train.h')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
EINVAL, ENOSPACE, EUNSUPPORTED = -1, -2, -3
WANT = ['dhdd_deform_conv_backward', 'dhdd_deform_conv_backward_scratch_bytes', 'dhdd_deform_conv_backward_supported']
MAX_HW = 853                                                 # (64 KiB / 4 - 1024) // 18: the (cell, tap) sort's LDS


def _declarations():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\bint\s+(dhdd_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src)}


def test_header_binding_table_and_exports_agree():
    from dhd_amd import _deform_train, _ext, _ffn, _ffn_train, _ffn_wide, _ffn_wide_train, _lib, _occ_train, _seam
    decl = _declarations()
    assert sorted(decl) == WANT == sorted(_deform_train.EXPORTED_SYMBOLS)
    lib = _deform_train.load()
    assert lib is _lib.load()                                        # the same library, the same handle
    for name, (argtypes, restype) in _deform_train._PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
        assert len(argtypes) == len(decl[name].split(',')), name     # as many parameters as the header declares
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r' T (dhdd_[a-z0-9_]+)', out)) == set(WANT)
    for other in (_lib, _ext, _ffn, _ffn_wide, _seam, _ffn_train, _ffn_wide_train, _occ_train):
        assert not any(n.startswith('dhdd') for n in other._PROTOTYPES), other.__name__
    assert _lib.ABI_VERSION == 6 and lib.dhd_abi_version() == 6      # the ABI number did not move
    text = open(HEADER).read()
    assert '#include "dhd_amd.h"' in text and 'DHD_ABI_VERSION is unchanged' in text
    assert os.listdir(CAPI) == ['dhd_amd_deform_train.h']


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / 'h.c'
    src.write_text('#include "dhd_amd_deform_train.h"\n'
                   'int main(void) { return dhdd_deform_conv_backward_supported(256, 256, 4, 3, 16, 44, DHD_F16, 1, 1) ? 0 : 1; }\n')
    out = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + INCLUDE, '-I' + CAPI, str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_the_makefile_keeps_its_translation_units_and_knows_the_headers():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith('SRCS')).split(':=')[1].split()
    assert 'deform_conv.hip' in srcs and len(srcs) == 22             # a header of deform_conv.hip, not a translation unit
    rule = next(ln for ln in mk.splitlines() if ln.startswith('%.o:')).split()
    assert 'deform_conv_train.h' in rule and '../capi_deform/dhd_amd_deform_train.h' in rule
    assert '#include "deform_conv_train.h"' in open(os.path.join(CSRC, 'deform_conv.hip')).read()


def test_supported_set_at_the_edges_of_the_shape_family():
    from dhd_amd import _deform_train, _lib
    lib = _deform_train.load()
    sup = lib.dhdd_deform_conv_backward_supported
    #            c_in c_out groups k  h   w   dtype x_layout g_layout
    assert sup(256, 256, 4, 3, 16, 44, 1, 0, 0) == 1
    for dt in (-1, 0, 1, 2, 3):
        for xl in (-1, 0, 1, 2):
            for gl in (-1, 0, 1, 2):
                want = int(dt in (0, 1, 2) and xl in (0, 1) and gl in (0, 1))
                assert sup(256, 256, 4, 3, 16, 44, dt, xl, gl) == want, (dt, xl, gl)
    # the inference operator's family: k = 3, C/g and O/g multiples of 8 up to 128
    for c, o, g, k, want in ((8, 8, 1, 3, 1), (128, 128, 1, 3, 1), (512, 512, 4, 3, 1), (136, 128, 1, 3, 0), (128, 136, 1, 3, 0), (12, 12, 1, 3, 0),
                             (32, 36, 4, 3, 0), (32, 32, 3, 3, 0), (32, 32, 4, 5, 0), (32, 32, 4, 1, 0), (0, 32, 4, 3, 0), (32, 32, 0, 3, 0)):
        assert sup(c, o, g, k, 6, 10, 0, 0, 0) == want, (c, o, g, k)
        assert want <= lib.dhd_deform_conv_infer_supported(c, o, g, k, 6, 10, 0, 0, 0)
    # the map: at most MAX_HW cells, which includes DHD-S's 16 x 44
    for h, w, want in ((1, 1, 1), (16, 44, 1), (1, MAX_HW, 1), (MAX_HW, 1, 1), (1, MAX_HW + 1, 0), (27, 32, 0), (0, 4, 0), (4, -1, 0)):
        assert sup(32, 32, 4, 3, h, w, 1, 1, 0) == want, (h, w)
    assert 16 * 44 <= MAX_HW


def test_scratch_bytes():
    from dhd_amd import _deform_train
    lib = _deform_train.load()
    n = C.c_size_t(77)

    def size(b, c, o, g, k, h, w, dt, xl, gl):
        n.value = 77
        rc = lib.dhdd_deform_conv_backward_scratch_bytes(b, c, o, g, k, h, w, dt, xl, gl, C.byref(n))
        assert (rc == 0) == (n.value != 0)                           # zero bytes whenever it is an error
        return rc, n.value
    base = (2, 32, 32, 4, 3, 6, 10)
    rc, cl = size(*base, 1, 1, 1)
    assert rc == 0 and cl % 256 == 0
    # the entry lists alone: two copies of b * 36 * hw entries of 8 bytes, and b * (9 hw + 1) segment bounds
    assert cl >= 2 * 2 * 36 * 60 * 8 + 2 * (9 * 60 + 1) * 4
    # an NCHW x or gout adds its channels_last copy; float32 doubles the weight streams and the copies
    x_copy = size(*base, 1, 0, 1)[1] - cl
    g_copy = size(*base, 1, 1, 0)[1] - cl
    assert x_copy == g_copy == 2 * 32 * 60 * 2 and size(*base, 1, 0, 0)[1] == cl + x_copy + g_copy
    assert size(*base, 2, 1, 1)[1] == cl and size(*base, 0, 1, 1)[1] > cl and size(*base, 0, 0, 1)[1] - size(*base, 0, 1, 1)[1] == 2 * x_copy
    # one group: no partial offset gradients
    assert size(2, 32, 32, 1, 3, 6, 10, 1, 1, 1)[1] < cl + 4 * 2 * 18 * 60 * 4
    for bad in ((0,) + base[1:], base[:1] + (0,) + base[2:], base[:5] + (0, 10), base[:6] + (-1,), base[:3] + (0,) + base[4:], (2, 32, 32, 3, 3, 6, 10)):
        assert size(*bad, 1, 1, 1) == (EINVAL, 0), bad
    for dt, xl, gl in ((-1, 1, 1), (3, 1, 1), (1, 2, 1), (1, 1, -1)):
        assert size(*base, dt, xl, gl) == (EINVAL, 0)
    for unsupported in ((2, 32, 32, 4, 5, 6, 10), (2, 12, 12, 1, 3, 6, 10), (2, 32, 32, 4, 3, 1, MAX_HW + 1), (65536, 32, 32, 4, 3, 6, 10)):
        assert size(*unsupported, 1, 1, 1) == (EUNSUPPORTED, 0), unsupported
    assert size(65535, 32, 32, 4, 3, 1, 1, 1, 1, 1)[0] == 0
    assert lib.dhdd_deform_conv_backward_scratch_bytes(*base, 1, 1, 1, None) == EINVAL


def test_bad_input_is_refused_on_the_host():
    """Fake addresses, no device: every call below returns before any launch.  Each base call is valid but for the one thing named."""
    from dhd_amd import _deform_train
    lib = _deform_train.load()
    fn = lib.dhdd_deform_conv_backward
    P = C.c_void_p(0x10000)
    need = C.c_size_t()
    assert lib.dhdd_deform_conv_backward_scratch_bytes(2, 32, 32, 4, 3, 6, 10, 1, 0, 1, C.byref(need)) == 0
    #       x  dtype layout offset weight gout g_layout dx doffset col | b c_in c_out groups h  w  k pad dil | scratch bytes stream
    base = [P, 1, 0, P, P, P, 1, P, P, P, 2, 32, 32, 4, 6, 10, 3, 1, 1, P, need.value, None]
    i_bytes = 20
    vec16, vec4, optional = (0, 5, 7, 9, 19), (3, 4, 8), (9,)

    def call(**kw):
        a = list(base)
        for k, val in kw.items():
            a[int(k[1:])] = val
        return fn(*a)
    for s in vec16 + vec4:
        if s not in optional:
            assert call(**{f'a{s}': None}) == EINVAL, s
    for s in vec16:
        for bad in (0x10004, 0x10008, 0x10002):
            assert call(**{f'a{s}': C.c_void_p(bad)}) == EINVAL, (s, bad)
    for s in vec4:
        assert call(**{f'a{s}': C.c_void_p(0x10002)}) == EINVAL, s
    assert call(a9=None, a20=need.value - 1) == ENOSPACE                 # col may be NULL: the call gets as far as the size check
    for i in (10, 11, 12, 13, 14, 15, 16):
        for bad in (0, -1):
            assert call(**{f'a{i}': bad}) == EINVAL, (i, bad)
    assert call(a17=-1) == EINVAL and call(a18=0) == EINVAL
    for dt in (-1, 3):
        assert call(a1=dt) == EINVAL
    for i in (2, 6):
        for layout in (-1, 2):
            assert call(**{f'a{i}': layout}) == EINVAL, (i, layout)
    assert call(a13=3) == EINVAL                                         # groups that do not divide the channels
    assert call(a16=5, a17=2) == EUNSUPPORTED and call(a11=12, a12=12, a13=1) == EUNSUPPORTED
    assert call(a14=1, a15=MAX_HW + 1, a20=1 << 40) == EUNSUPPORTED and call(a10=65536, a20=1 << 40) == EUNSUPPORTED
    for short in (0, 1024, need.value - 1):
        assert call(a20=short) == ENOSPACE, short
    # a NULL pointer before the shape, the shape before the size, the size before the alignment (dhd_deform_conv_infer's order)
    assert call(a0=None, a16=5) == EINVAL and call(a16=5, a20=0) == EUNSUPPORTED
    assert call(a0=C.c_void_p(0x10004), a20=0) == ENOSPACE


def test_no_cpu_path_and_cpu_tensors_keep_the_module_formulation(monkeypatch):
    import dhd_amd
    from dhd_amd import deform_conv as DC
    from dhd_amd.depthnet import DCN
    x, offset, weight = torch.randn(2, 32, 6, 10), torch.randn(2, 18, 6, 10), torch.randn(32, 8, 3, 3)
    with pytest.raises(dhd_amd._lib.DhdError):                           # no fallback: the operator is HIP only
        dhd_amd.deform_conv(x, offset, weight, groups=4)
    assert not DC.deform_conv_train_supported(x, weight, 4) and not DC.deform_conv_train_routed(x, weight, 4)
    assert dhd_amd.deform_conv_train_supported is DC.deform_conv_train_supported and callable(dhd_amd.deform_conv_infer)
    # with the switch on and the table saying yes to everything, CPU tensors take today's path: every bit, every gradient
    monkeypatch.setattr(DC, 'deform_conv', lambda *a, **k: (_ for _ in ()).throw(AssertionError('the fused operator was reached')))
    monkeypatch.setattr(DC, 'ROUTED_TRAIN', {k: True for k in DC.ROUTED_TRAIN})
    torch.manual_seed(3)
    m = DCN(32, 32, groups=4)
    with torch.no_grad():
        m.conv_offset.bias.normal_(0, 1.0)

    def step():
        m.zero_grad(set_to_none=True)
        xl = x.clone().requires_grad_()
        out = m(xl)
        out.square().sum().backward()
        return [out.detach(), xl.grad] + [p.grad.clone() for p in m.parameters()]
    assert 'fused_train' not in vars(m)
    want = step()
    assert dhd_amd.fused_dcn_training(m) == [m] and m.fused_train is True and not m._train_applies(x)
    got = step()
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert dhd_amd.fused_dcn_training(m, False) == [m] and m.fused_train is False and m.fused_infer is False and m.use_hip is True
    assert len(DC.ROUTED_TRAIN) == 6 and all(isinstance(on, bool) for on in DC.ROUTED_TRAIN.values())
    assert set(DC.ROUTED_TRAIN) == {(dt, layout) for dt in (torch.float32, torch.float16, torch.bfloat16) for layout in (0, 1)}


def test_the_switch_is_off_and_the_environment_variable_sets_the_class_default():
    from dhd_amd.depthnet import DCN
    assert 'DHD_DCN_TRAIN' in os.environ or DCN.fused_train is False
    code = 'from dhd_amd.depthnet import DCN as D; print(D.fused_train, D.fused_infer, D.use_hip)'
    for value, want in ((None, 'False False True'), ('1', 'True False True')):
        env = {k: v for k, v in os.environ.items() if k != 'DHD_DCN_TRAIN'}
        if value is not None:
            env['DHD_DCN_TRAIN'] = value
        out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT, env=env)
        assert out.returncode == 0 and out.stdout.split('\n')[0] == want, (value, out.stdout, out.stderr[-800:])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_the_backward_kernels_use_no_private_memory(tmp_path):
    """deform_conv.hip compiled to gfx950 assembly with the Makefile's flags: every instantiation of the backward's kernels (dx for
    3 types x 2 layouts x 3 tile counts, cols for 3 types x 4 k-step counts, the two stream packers per type, the sort, the sum
    of the partial offset gradients) reports a private segment of 0 bytes."""
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    flags = re.search(r'^HIPFLAGS \?= (.*?)(?<!\\)$', mk, flags=re.S | re.M).group(1).replace('\\\n', ' ').replace('$(ARCH)', 'gfx950').split()
    flags = [f for f in flags if f not in ('-fPIC', '-Wall')]
    out = tmp_path / 'deform_conv.s'
    subprocess.run([HIPCC] + flags + ['--cuda-device-only', '-S', os.path.join(CSRC, 'deform_conv.hip'), '-o', str(out)], check=True,
                   capture_output=True, timeout=900)
    meta = re.findall(r'\.name:\s+(\S+)\n(?:(?!\.name:).)*?\.private_segment_fixed_size:\s+(\d+)', open(out).read(), flags=re.S)
    keys = ('deform_conv_bwd_dx_kernel', 'deform_conv_bwd_cols_kernel', 'pack_train_weights_kernel', 'deform_tap_sort_ct', 'deform_doff_sum_kernel')
    new = {n: int(p) for n, p in meta if any(k in n for k in keys)}
    count = {k: len([n for n in new if k in n]) for k in keys}
    assert count == dict(zip(keys, (18, 12, 6, 1, 1))), count
    assert all(p == 0 for p in new.values()), {n: p for n, p in new.items() if p}
