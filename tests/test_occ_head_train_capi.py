"""The occupancy head's training surface `dhdo_*` of libdhd_amd.so (dhd_amd/capi/dhd_amd_occ_train.h, dhd_amd/_occ_train.py)
without a GPU: header, binding table and exports agree and leave the other surfaces alone; the entry points refuse bad input on
the host with the documented code; the switch is off and sets only itself; the backward kernels use no private memory; and the
inputs the GPU tests measure against are what they are said to be."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_head_train_inputs as OT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
CAPI = os.path.join(ROOT, 'dhd_amd', 'capi')
CSRC = os.path.join(ROOT, 'dhd_amd', 'csrc')
HEADER = os.path.join(CAPI, 'dhd_amd_occ_train.h')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
EINVAL, ENOSPACE, EUNSUPPORTED = -1, -2, -3
WANT = ['dhdo_occ_head_backward', 'dhdo_occ_head_backward_scratch_bytes', 'dhdo_occ_head_backward_supported']
ROW = 800 * 4                                               # one workgroup's partial sums: db1 (512) and db2 (288) as float32


def _declarations():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\bint\s+(dhdo_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src)}


def _weights(c=256, hidden=512, dz=16, n_classes=18, gemm=0, ptr=0x10000):
    from dhd_amd import _lib
    w = _lib.OccHeadWeights()
    w.w1 = w.b1 = w.w2 = w.b2 = ptr
    w.c, w.hidden, w.dz, w.n_classes, w.gemm = c, hidden, dz, n_classes, gemm
    return w


def test_header_binding_table_and_exports_agree():
    from dhd_amd import _ext, _ffn, _ffn_train, _ffn_wide, _ffn_wide_train, _lib, _occ_train, _seam
    decl = _declarations()
    assert sorted(decl) == WANT == sorted(_occ_train.EXPORTED_SYMBOLS)
    lib = _occ_train.load()
    assert lib is _lib.load()                                        # the same library, the same handle
    for name, (argtypes, restype) in _occ_train._PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
        assert len(argtypes) == len(decl[name].split(',')), name     # as many parameters as the header declares
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r' T (dhdo_[a-z0-9_]+)', out)) == set(WANT)
    # the other surfaces are what they were: the family is in none of their tables, and the ABI number did not move
    for other in (_lib, _ext, _ffn, _ffn_wide, _seam, _ffn_train, _ffn_wide_train):
        assert not any(n.startswith('dhdo') for n in other._PROTOTYPES), other.__name__
    assert (len(_ext._PROTOTYPES), len(_ffn._PROTOTYPES), len(_ffn_wide._PROTOTYPES), len(_seam._PROTOTYPES),
            len(_ffn_train._PROTOTYPES), len(_ffn_wide_train._PROTOTYPES)) == (5, 3, 3, 8, 5, 5)
    assert _lib.ABI_VERSION == 6 and lib.dhd_abi_version() == 6
    assert re.search(r'#define DHD_ABI_VERSION 6\b', open(os.path.join(INCLUDE, 'dhd_amd.h')).read())
    text = open(HEADER).read()
    assert '#include "dhd_amd.h"' in text and 'DHD_ABI_VERSION is unchanged' in text
    assert not any(p in text for p in ('dhds_', 'dhdg_', 'dhdf_', 'dhdx_', 'dhdt_', 'dhdu_'))
    # both pinned listings are as they were, and the new directory holds the one header
    assert sorted(os.listdir(INCLUDE)) == ['dhd_amd.h', 'dhd_amd_ext.h', 'dhd_amd_ffn.h', 'dhd_amd_ffn_train.h', 'dhd_amd_ffn_wide.h',
                                           'dhd_amd_seam.h']
    assert os.listdir(os.path.join(ROOT, 'dhd_amd', 'include')) == ['dhd_amd_ffn_wide_train.h']
    assert os.listdir(CAPI) == ['dhd_amd_occ_train.h']
    for d in (INCLUDE, os.path.join(ROOT, 'dhd_amd', 'include')):
        for other in os.listdir(d):
            assert 'dhdo_' not in open(os.path.join(d, other)).read(), other


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / 'h.c'
    src.write_text('#include "dhd_amd_occ_train.h"\n'
                   'int main(void) { return dhdo_occ_head_backward_supported(256, 512, 16, 18, DHD_F32, 0) ? 0 : 1; }\n')
    out = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + INCLUDE, '-I' + CAPI, str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_the_makefile_keeps_its_translation_units_and_knows_the_headers():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith('SRCS')).split(':=')[1].split()
    assert 'occ_head.hip' in srcs and len(srcs) == 22                # a header of occ_head.hip, not a translation unit
    rule = next(ln for ln in mk.splitlines() if ln.startswith('%.o:')).split()
    assert 'occ_head_train.h' in rule and '../capi/dhd_amd_occ_train.h' in rule
    assert os.path.exists(os.path.join(CSRC, 'occ_head_train.h'))
    assert '#include "occ_head_train.h"' in open(os.path.join(CSRC, 'occ_head.hip')).read()


def test_supported_set_is_the_inference_operators():
    from dhd_amd import _lib, _occ_train
    lib = _occ_train.load()
    _lib.load()
    heads = ((256, 512, 16, 18), (256, 512, 16, 17), (256, 512, 8, 18), (128, 512, 16, 18), (256, 1024, 16, 18), (512, 512, 16, 18), (0, 0, 0, 0))
    for c, hidden, dz, n in heads:
        for dt in (-1, 0, 1, 2, 3):
            for layout in (-1, 0, 1, 2):
                want = lib.dhd_occ_head_infer_supported(c, hidden, dz, n, dt, layout, 0)
                assert lib.dhdo_occ_head_backward_supported(c, hidden, dz, n, dt, layout) == want, (c, hidden, dz, n, dt, layout)
                assert want == int((c, hidden, dz, n) == (256, 512, 16, 18) and dt in (0, 1, 2) and layout in (0, 1))


def test_scratch_bytes():
    from dhd_amd import _occ_train
    lib = _occ_train.load()
    n = C.c_size_t(77)
    w = _weights()

    def size(dt, b, dy, dx, wts=w):
        n.value = 77
        rc = lib.dhdo_occ_head_backward_scratch_bytes(C.byref(wts), dt, b, dy, dx, C.byref(n))
        assert (rc == 0) == (n.value != 0)                           # zero bytes whenever it is an error
        return rc, n.value
    for dt in (0, 1, 2):
        rc, one = size(dt, 1, 1, 1)
        assert rc == 0
        # the stream: b1 and three blocks of fragments (W1, W2, W1 again) in the GEMM type -- two bf16 parts of a float32
        assert one >= 512 * 4 + (2 * 256 * 512 + 288 * 512) * (4 if dt == 0 else 2) + ROW and (one - ROW) % 1024 == 0
        # one 800-float row per workgroup of 128 cells of a sample
        for b, dy, dx, groups in ((1, 8, 16, 1), (1, 1, 129, 2), (1, 12, 11, 2), (2, 7, 9, 2), (3, 20, 28, 15), (4, 200, 200, 4 * 313)):
            assert size(dt, b, dy, dx) == (0, one + (groups - 1) * ROW), (dt, b, dy, dx)
    assert size(1, 3, 20, 28) == size(2, 3, 20, 28) and size(0, 3, 20, 28)[1] > size(1, 3, 20, 28)[1]
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)):
        assert size(0, *bad) == (EINVAL, 0)
    for dt in (-1, 3):
        assert size(dt, 1, 1, 1) == (EINVAL, 0)
    assert size(0, 65536, 1, 1) == (EUNSUPPORTED, 0) and size(0, 1, 1025, 1024) == (EUNSUPPORTED, 0) and size(0, 1, 1024, 1024)[0] == 0
    for wts in (_weights(c=128), _weights(hidden=256), _weights(dz=8), _weights(n_classes=17), _weights(gemm=1), _weights(gemm=2)):
        assert size(0, 1, 1, 1, wts) == (EUNSUPPORTED, 0)
    assert lib.dhdo_occ_head_backward_scratch_bytes(None, 0, 1, 1, 1, C.byref(n)) == EINVAL
    assert lib.dhdo_occ_head_backward_scratch_bytes(C.byref(w), 0, 1, 1, 1, None) == EINVAL


def test_bad_input_is_refused_on_the_host():
    """Fake addresses, no device: every call below returns before any launch.  Each base call is valid but for the one thing named."""
    from dhd_amd import _occ_train
    lib = _occ_train.load()
    fn = lib.dhdo_occ_head_backward
    P = C.c_void_p(0x10000)
    w = _weights()
    need = C.c_size_t()
    assert lib.dhdo_occ_head_backward_scratch_bytes(C.byref(w), 1, 3, 20, 28, C.byref(need)) == 0
    #       x  dtype layout w         b  dy  dx | glogits dx_out db1 db2 act dhid ghalf scratch | bytes stream
    base = [P, 1, 0, C.byref(w), 3, 20, 28, P, P, P, P, P, P, P, P, need.value, None]
    i_w, i_b, i_bytes = 3, 4, 15
    required, optional = (0, 7, 8, 9, 10, 14), (11, 12, 13)

    def call(**kw):
        a = list(base)
        for k, val in kw.items():
            a[int(k[1:])] = val
        return fn(*a)
    for s in required + optional:
        for bad in (None, C.c_void_p(0x10004), C.c_void_p(0x10002)):
            if bad is None and s in optional:
                continue
            assert call(**{f'a{s}': bad}) == EINVAL, (s, bad)
    assert call(a3=None) == EINVAL
    for member in ('w1', 'b1', 'w2'):
        for bad in (0, 0x10004):
            wb = _weights()
            setattr(wb, member, bad)
            assert call(a3=C.byref(wb)) == EINVAL, (member, bad)
    wb = _weights()
    wb.b2 = 0                                                        # b2 has no part in the backward
    assert call(a3=C.byref(wb), a15=need.value - 1) == ENOSPACE
    # the operands: act and dhid together; ghalf only beside them and only with a half type
    assert call(a11=None) == EINVAL and call(a12=None) == EINVAL
    assert call(a11=None, a12=None) == EINVAL                        # ... ghalf without act
    assert call(a11=None, a12=None, a13=None, a15=need.value - 1) == ENOSPACE
    assert call(a13=None, a15=need.value - 1) == ENOSPACE
    assert call(a1=0, a15=1 << 30) == EINVAL                         # ghalf with float32
    assert call(a1=0, a13=None, a15=need.value) == ENOSPACE          # (the float32 stream is the larger one)
    for i in (4, 5, 6):
        for bad in (0, -1):
            assert call(**{f'a{i}': bad}) == EINVAL, (i, bad)
    for dt in (-1, 3):
        assert call(a1=dt) == EINVAL
    for layout in (-1, 2):
        assert call(a2=layout) == EUNSUPPORTED
    for wts in (_weights(c=128), _weights(hidden=256), _weights(dz=8), _weights(n_classes=17), _weights(gemm=1)):
        assert call(a3=C.byref(wts)) == EUNSUPPORTED
    assert call(a4=65536, a15=1 << 40) == EUNSUPPORTED
    assert call(a5=1025, a6=1024, a15=1 << 40) == EUNSUPPORTED       # one sample past the 32-bit buffer descriptor
    # the pointer test comes first, the size check last
    assert call(a0=None, a3=C.byref(_weights(c=128))) == EINVAL
    for short in (0, 1024, need.value - 1):
        assert call(a15=short) == ENOSPACE, short
    assert call(a15=0, a3=C.byref(_weights(c=128))) == EUNSUPPORTED


def test_no_cpu_path_and_cpu_tensors_keep_the_module_formulation(monkeypatch):
    import dhd_amd
    from dhd_amd import occ_head
    from dhd_amd.detector import predictor
    v = OT.inputs('partial_wave', 'f32')
    with pytest.raises(dhd_amd._lib.DhdError):                       # no fallback: the operator is HIP only
        dhd_amd.occ_head_train(v['x'], v['w1'], v['b1'], v['w2'], v['b2'])
    assert not occ_head.train_supported(v['x'], v['w1'], v['w2']) and not occ_head.train_routed(v['x'], v['w1'], v['w2'])
    # with the switch on and the table saying yes to everything, CPU tensors take today's path: every bit, every gradient
    monkeypatch.setattr(occ_head, 'occ_head_train', lambda *a, **k: (_ for _ in ()).throw(AssertionError('the fused operator was reached')))
    monkeypatch.setattr(occ_head, 'ROUTED_TRAIN', {k: True for k in occ_head.ROUTED_TRAIN})
    head = OT.module_head()
    feats = OT.module_inputs()[0]

    def step(h):
        h.zero_grad(set_to_none=True)
        x = feats.clone().requires_grad_()
        out = h(x)
        out.square().sum().backward()
        return [out.detach(), x.grad] + [p.grad.clone() for p in h.parameters()]
    assert 'fused_train' not in vars(head)
    want = step(head)
    assert len(dhd_amd.fused_occ_head_training(head)) == 1 and head.fused_train is True and not head._train_applies(feats)
    got = step(head)
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert dhd_amd.fused_occ_head_training(head, False) == [head] and head.fused_train is False
    del head.fused_train
    assert len(occ_head.ROUTED_TRAIN) == 6 and all(isinstance(on, bool) for on in occ_head.ROUTED_TRAIN.values())
    assert set(occ_head.ROUTED_TRAIN) == {(dt, layout) for dt in (torch.float32, torch.float16, torch.bfloat16) for layout in (0, 1)}
    assert predictor.fused_infer is False and callable(dhd_amd.occ_head_infer)


def test_the_switch_is_off_and_the_environment_variable_sets_the_class_default():
    from dhd_amd.detector import predictor
    assert 'DHD_OCC_HEAD_TRAIN' in os.environ or predictor.fused_train is False
    code = 'from dhd_amd.detector import predictor as P; print(P.fused_train, P.fused_infer)'
    for value, want in ((None, 'False False'), ('1', 'True False')):
        env = {k: v for k, v in os.environ.items() if k != 'DHD_OCC_HEAD_TRAIN'}
        if value is not None:
            env['DHD_OCC_HEAD_TRAIN'] = value
        out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT, env=env)
        assert out.returncode == 0 and out.stdout.split('\n')[0] == want, (value, out.stdout, out.stderr[-800:])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_the_backward_kernels_use_no_private_memory(tmp_path):
    """occ_head.hip compiled to gfx950 assembly with the Makefile's flags: every instantiation of the backward's kernels (the
    operator for 3 types x 2 layouts, the stream packer, the bias sums) reports a private segment of 0 bytes."""
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    flags = re.search(r'^HIPFLAGS \?= (.*?)(?<!\\)$', mk, flags=re.S | re.M).group(1).replace('\\\n', ' ').replace('$(ARCH)', 'gfx950').split()
    flags = [f for f in flags if f not in ('-fPIC', '-Wall')]
    out = tmp_path / 'occ_head.s'
    subprocess.run([HIPCC] + flags + ['--cuda-device-only', '-S', os.path.join(CSRC, 'occ_head.hip'), '-o', str(out)], check=True,
                   capture_output=True, timeout=900)
    meta = re.findall(r'\.name:\s+(\S+)\n(?:(?!\.name:).)*?\.private_segment_fixed_size:\s+(\d+)', open(out).read(), flags=re.S)
    new = {n: int(p) for n, p in meta if any(k in n for k in ('occ_head_bwd_kernel', 'occ_head_bwd_params', 'pack_train_stream_kernel'))}
    assert len([n for n in new if 'occ_head_bwd_kernel' in n]) == 6 and len(new) == 10, sorted(new)
    assert all(p == 0 for p in new.values()), {n: p for n, p in new.items() if p}


def test_the_inputs_are_what_they_are_said_to_be():
    assert sorted(OT.SHAPES.values()) == [(1, 1, 1), (1, 12, 11), (2, 7, 9), (3, 20, 28)] and len(OT.GRID) == 24
    for case, shape in OT.SHAPES.items():
        g = OT.make_glogits(shape)
        b, dy, dx = shape
        assert g.dtype == torch.float32 and tuple(g.shape) == (b, dx, dy, OT.DZ, OT.N_CLS)
        dead = (g == 0).all(-1)
        assert bool(((g == 0).any(-1) == dead).all())                # whole voxels, nothing else
        if dead.numel() >= 1000:
            assert 0.25 < float(dead.double().mean()) < 0.35
    # the twin against torch's own float32 autograd over the same formulation: float32 rounding apart
    ref, got = OT.twin('partial_wave', 'f32'), OT.chain(OT.inputs('partial_wave', 'f32'), torch.float32, 'cpu')
    for k in OT.TENSORS:
        assert ref[k].dtype == torch.float64 and float((got[k].double() - ref[k]).abs().max()) <= 5e-5 * OT.scale_of(ref[k]), k
    # fp16 at module level: the loss scale keeps the gradient of the logits in fp16's normal range, the unscaled loss does not
    scale = OT.fp16_loss_scale()
    assert OT.starved_fraction(scale) < 0.01 <= OT.starved_fraction(scale / 2) and scale == 2.0 ** round(torch.log2(torch.tensor(scale)).item())
    m = OT.module_twin()
    assert m['losses'].dtype == torch.float64 and bool(torch.isfinite(m['losses']).all()) and float((m['glogits'] == 0).double().mean()) > 0.2
