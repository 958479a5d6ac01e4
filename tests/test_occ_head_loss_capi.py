"""The occupancy head + losses surface `dhdl_*` of libdhd_amd.so (dhd_amd/capi_occ_loss/dhd_amd_occ_head_loss.h,
dhd_amd/_occ_loss_head.py) without a GPU: header, binding table and exports agree and leave the other surfaces alone; the entry
points refuse bad input on the host with the documented code; the switch is off and sets only itself; the new kernels use no
private memory; and the inputs the GPU tests measure against are what they are said to be."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_head_loss_inputs as OL  # noqa: E402
import occ_head_train_inputs as OT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
CAPI = os.path.join(ROOT, 'dhd_amd', 'capi_occ_loss')
CSRC = os.path.join(ROOT, 'dhd_amd', 'csrc')
HEADER = os.path.join(CAPI, 'dhd_amd_occ_head_loss.h')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
EINVAL, ENOSPACE, EUNSUPPORTED = -1, -2, -3
WANT = ['dhdl_occ_head_loss_backward', 'dhdl_occ_head_loss_forward', 'dhdl_occ_head_loss_scratch_bytes', 'dhdl_occ_head_loss_supported',
        'dhdl_occ_head_loss_workspace_bytes']
FWD_ROW, BWD_ROW = 56 * 4, 800 * 4                          # one workgroup's partial sums, forward and backward


def _declarations():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(?:int|size_t)\s+(dhdl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src)}


def _weights(c=256, hidden=512, dz=16, n_classes=18, gemm=0, ptr=0x10000):
    from dhd_amd import _lib
    w = _lib.OccHeadWeights()
    w.w1 = w.b1 = w.w2 = w.b2 = ptr
    w.c, w.hidden, w.dz, w.n_classes, w.gemm = c, hidden, dz, n_classes, gemm
    return w


def test_header_binding_table_and_exports_agree():
    from dhd_amd import _deform_train, _ext, _ffn, _ffn_train, _ffn_wide, _ffn_wide_train, _lib, _occ_loss_head, _occ_train, _seam
    decl = _declarations()
    assert sorted(decl) == WANT == sorted(_occ_loss_head.EXPORTED_SYMBOLS)
    lib = _occ_loss_head.load()
    assert lib is _lib.load()                                        # the same library, the same handle
    for name, (argtypes, restype) in _occ_loss_head._PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
        params = [p for p in decl[name].split(',') if p.strip() != 'void']
        assert len(argtypes) == len(params), name                    # as many parameters as the header declares
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r' T (dhdl_[a-z0-9_]+)', out)) == set(WANT)
    for other in (_lib, _ext, _ffn, _ffn_wide, _seam, _ffn_train, _ffn_wide_train, _occ_train, _deform_train):
        assert not any(n.startswith('dhdl') for n in other._PROTOTYPES), other.__name__
    assert _lib.ABI_VERSION == 6 and lib.dhd_abi_version() == 6
    text = open(HEADER).read()
    assert '#include "dhd_amd.h"' in text and 'DHD_ABI_VERSION is unchanged' in text
    assert os.listdir(CAPI) == ['dhd_amd_occ_head_loss.h']
    assert lib.dhdl_occ_head_loss_workspace_bytes() == 56 * 8


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / 'h.c'
    src.write_text('#include "dhd_amd_occ_head_loss.h"\n'
                   'int main(void) { return dhdl_occ_head_loss_supported(256, 512, 16, 18, DHD_F32, 0) ? 0 : 1; }\n')
    out = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + INCLUDE, '-I' + CAPI, str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_the_makefile_knows_the_headers():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    rule = next(ln for ln in mk.splitlines() if ln.startswith('%.o:')).split()
    for h in ('occ_head_loss.h', 'occ_loss_math.h', '../capi_occ_loss/dhd_amd_occ_head_loss.h'):
        assert h in rule, h
    text = open(os.path.join(CSRC, 'occ_head.hip')).read()
    assert text.index('#include "occ_head_train.h"') < text.index('#include "occ_head_loss.h"')
    assert '#include "occ_loss_math.h"' in text and '#include "occ_loss_math.h"' in open(os.path.join(CSRC, 'occ_loss.hip')).read()


def test_supported_set_is_the_inference_operators():
    from dhd_amd import _occ_loss_head
    lib = _occ_loss_head.load()
    for c, hidden, dz, n in ((256, 512, 16, 18), (256, 512, 16, 17), (256, 512, 8, 18), (128, 512, 16, 18), (256, 1024, 16, 18), (0, 0, 0, 0)):
        for dt in (-1, 0, 1, 2, 3):
            for layout in (-1, 0, 1, 2):
                want = lib.dhd_occ_head_infer_supported(c, hidden, dz, n, dt, layout, 0)
                assert lib.dhdl_occ_head_loss_supported(c, hidden, dz, n, dt, layout) == want, (c, hidden, dz, n, dt, layout)


def test_scratch_bytes():
    from dhd_amd import _occ_loss_head, _occ_train
    lib = _occ_loss_head.load()
    _occ_train.load()
    f, b = C.c_size_t(77), C.c_size_t(77)
    w = _weights()

    def size(dt, n, dy, dx, wts=w):
        f.value = b.value = 77
        rc = lib.dhdl_occ_head_loss_scratch_bytes(C.byref(wts), dt, n, dy, dx, C.byref(f), C.byref(b))
        assert (rc == 0) == (f.value != 0) == (b.value != 0)         # zero bytes whenever it is an error
        return rc, f.value, b.value
    for dt in (0, 1, 2):
        rc, f1, b1 = size(dt, 1, 1, 1)
        infer, train = C.c_size_t(), C.c_size_t()
        assert rc == 0 and lib.dhd_occ_head_infer_scratch_bytes(C.byref(w), dt, C.byref(infer)) == 0
        assert lib.dhdo_occ_head_backward_scratch_bytes(C.byref(w), dt, 1, 1, 1, C.byref(train)) == 0
        assert f1 == infer.value + FWD_ROW and b1 == train.value     # the inference stream + one row; the training backward's
        for n, dy, dx, groups in ((1, 8, 16, 1), (1, 1, 129, 2), (1, 12, 11, 2), (2, 7, 9, 2), (3, 20, 28, 15), (4, 200, 200, 4 * 313)):
            assert size(dt, n, dy, dx) == (0, f1 + (groups - 1) * FWD_ROW, b1 + (groups - 1) * BWD_ROW), (dt, n, dy, dx)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)):
        assert size(0, *bad) == (EINVAL, 0, 0)
    for dt in (-1, 3):
        assert size(dt, 1, 1, 1) == (EINVAL, 0, 0)
    assert size(0, 65536, 1, 1)[0] == EUNSUPPORTED and size(0, 1, 1025, 1024)[0] == EUNSUPPORTED and size(0, 1, 1024, 1024)[0] == 0
    for wts in (_weights(c=128), _weights(hidden=256), _weights(dz=8), _weights(n_classes=17), _weights(gemm=1), _weights(gemm=3)):
        assert size(0, 1, 1, 1, wts) == (EUNSUPPORTED, 0, 0)
    assert lib.dhdl_occ_head_loss_scratch_bytes(None, 0, 1, 1, 1, C.byref(f), C.byref(b)) == EINVAL
    assert lib.dhdl_occ_head_loss_scratch_bytes(C.byref(w), 0, 1, 1, 1, None, C.byref(b)) == EINVAL and b.value == 0
    assert lib.dhdl_occ_head_loss_scratch_bytes(C.byref(w), 0, 1, 1, 1, C.byref(f), None) == EINVAL and f.value == 0


def _caller(fn, base):
    def call(**kw):
        a = list(base)
        for k, val in kw.items():
            a[int(k[1:])] = val
        return fn(*a)
    return call


def test_the_forward_refuses_bad_input_on_the_host():
    """Fake addresses, no device: every call below returns before any launch.  Each base call is valid but for the one thing named."""
    from dhd_amd import _occ_loss_head
    lib = _occ_loss_head.load()
    P = C.c_void_p(0x10000)
    w = _weights()
    f, b = C.c_size_t(), C.c_size_t()
    assert lib.dhdl_occ_head_loss_scratch_bytes(C.byref(w), 1, 3, 20, 28, C.byref(f), C.byref(b)) == 0
    #       x  dtype layout w      b  dy  dx | labels mask cw | ignore non_empty | logits losses workspace scratch | bytes stream
    base = [P, 1, 0, C.byref(w), 3, 20, 28, P, P, P, 255, 17, P, P, P, P, f.value, None]
    call = _caller(lib.dhdl_occ_head_loss_forward, base)
    short = dict(a16=f.value - 1)
    for s, aligns in ((0, 16), (7, 8), (8, 8), (9, 4), (12, 16), (13, 4), (14, 16), (15, 16)):
        assert call(**{f'a{s}': None}) == EINVAL, s
        assert call(**{f'a{s}': C.c_void_p(0x10000 + aligns // 2)}) == EINVAL, s
        assert call(**{f'a{s}': C.c_void_p(0x10000 + aligns)}, **short) == ENOSPACE, s
    assert call(a3=None) == EINVAL
    for member in ('w1', 'b1', 'w2', 'b2'):
        for bad in (0, 0x10004):
            wb = _weights()
            setattr(wb, member, bad)
            assert call(a3=C.byref(wb)) == EINVAL, (member, bad)
    for i in (4, 5, 6):
        for bad in (0, -1):
            assert call(**{f'a{i}': bad}) == EINVAL, (i, bad)
    for dt in (-1, 3):
        assert call(a1=dt) == EINVAL
    for layout in (-1, 2):
        assert call(a2=layout) == EUNSUPPORTED
    for wts in (_weights(c=128), _weights(hidden=256), _weights(dz=8), _weights(n_classes=17), _weights(gemm=1)):
        assert call(a3=C.byref(wts)) == EUNSUPPORTED
    assert call(a1=0, a3=C.byref(_weights(gemm=3)), a16=1 << 30) == EUNSUPPORTED      # the default GEMM mode only
    for ignore in (-1, 256):
        assert call(a10=ignore) == EUNSUPPORTED
    for non_empty in (-1, 18):
        assert call(a11=non_empty) == EUNSUPPORTED
    assert call(a10=0, a11=0, **short) == ENOSPACE
    assert call(a4=65536, a16=1 << 40) == EUNSUPPORTED and call(a5=1025, a6=1024, a16=1 << 40) == EUNSUPPORTED
    assert call(a0=None, a3=C.byref(_weights(c=128))) == EINVAL                       # the pointer test first, the size check last
    for n in (0, 1024, f.value - 1):
        assert call(a16=n) == ENOSPACE, n
    assert call(a16=0, a3=C.byref(_weights(c=128))) == EUNSUPPORTED


def test_the_backward_refuses_bad_input_on_the_host():
    from dhd_amd import _occ_loss_head
    lib = _occ_loss_head.load()
    P = C.c_void_p(0x10000)
    w = _weights()
    f, b = C.c_size_t(), C.c_size_t()
    assert lib.dhdl_occ_head_loss_scratch_bytes(C.byref(w), 1, 3, 20, 28, C.byref(f), C.byref(b)) == 0
    #       0  1     2      3          4  5   6  | 7      8      9    10 | 11     12        | 13          14        15     16  17  18  19   20 21
    #       x  dtype layout w          b  dy  dx | logits labels mask cw | ignore non_empty | grad_losses workspace dx_out db1 db2 act dhid g  scratch | bytes stream
    base = [P, 1, 0, C.byref(w), 3, 20, 28, P, P, P, P, 255, 17, P, P, P, P, P, P, P, P, P, b.value, None]
    call = _caller(lib.dhdl_occ_head_loss_backward, base)
    short = dict(a22=b.value - 1)
    for s, aligns in ((0, 16), (7, 16), (8, 8), (9, 8), (10, 4), (13, 4), (14, 16), (15, 16), (16, 16), (17, 16), (21, 16)):
        assert call(**{f'a{s}': None}) == EINVAL, s
        assert call(**{f'a{s}': C.c_void_p(0x10000 + aligns // 2)}) == EINVAL, s
        assert call(**{f'a{s}': C.c_void_p(0x10000 + aligns)}, **short) == ENOSPACE, s
    for s in (18, 19, 20):
        assert call(**{f'a{s}': C.c_void_p(0x10008)}) == EINVAL, s
    wb = _weights()
    wb.b2 = 0                                                        # b2 has no part in the backward
    assert call(a3=C.byref(wb), **short) == ENOSPACE
    for member in ('w1', 'b1', 'w2'):
        wb = _weights()
        setattr(wb, member, 0)
        assert call(a3=C.byref(wb)) == EINVAL, member
    # the operands: act and dhid together; g optional beside them with a half type, required with float32
    assert call(a18=None) == EINVAL and call(a19=None) == EINVAL
    assert call(a18=None, a19=None) == EINVAL                        # ... g without act
    assert call(a18=None, a19=None, a20=None, **short) == ENOSPACE and call(a20=None, **short) == ENOSPACE
    assert call(a1=0, a20=None, a22=1 << 30) == EINVAL               # float32 without g
    assert call(a1=0, a18=None, a19=None, a22=b.value) == ENOSPACE   # float32, frozen weights: g is scratch (the float32 stream is larger)
    for i in (4, 5, 6):
        for bad in (0, -1):
            assert call(**{f'a{i}': bad}) == EINVAL, (i, bad)
    for dt in (-1, 3):
        assert call(a1=dt) == EINVAL
    for layout in (-1, 2):
        assert call(a2=layout) == EUNSUPPORTED
    for wts in (_weights(c=128), _weights(hidden=256), _weights(dz=8), _weights(n_classes=17), _weights(gemm=1)):
        assert call(a3=C.byref(wts)) == EUNSUPPORTED
    for ignore in (-1, 256):
        assert call(a11=ignore) == EUNSUPPORTED
    for non_empty in (-1, 18):
        assert call(a12=non_empty) == EUNSUPPORTED
    assert call(a4=65536, a22=1 << 40) == EUNSUPPORTED and call(a5=1025, a6=1024, a22=1 << 40) == EUNSUPPORTED
    for n in (0, 1024, b.value - 1):
        assert call(a22=n) == ENOSPACE, n
    assert call(a22=0, a3=C.byref(_weights(c=128))) == EUNSUPPORTED


def test_no_cpu_path_and_the_switch_sets_only_itself(monkeypatch):
    import dhd_amd
    from dhd_amd import occ_head
    from dhd_amd.detector import DHD, predictor
    import types
    v = OT.inputs('partial_wave', 'f32')
    sem, cam = OL.labels('partial_wave')
    with pytest.raises(dhd_amd._lib.DhdError):                       # no fallback: the operator is HIP only
        dhd_amd.occ_head_losses(v['x'], v['w1'], v['b1'], v['w2'], v['b2'], sem, cam, OL.class_weights())
    assert not occ_head.loss_supported(v['x'], v['w1'], v['w2']) and not occ_head.loss_routed(v['x'], v['w1'], v['w2'])
    assert set(occ_head.ROUTED_LOSS) == set(occ_head.ROUTED_TRAIN) and all(isinstance(on, bool) for on in occ_head.ROUTED_LOSS.values())
    # with the switch on and the table saying yes to everything, CPU tensors take today's two calls: every bit
    monkeypatch.setattr(occ_head, 'occ_head_losses', lambda *a, **k: (_ for _ in ()).throw(AssertionError('the fused operator was reached')))
    monkeypatch.setattr(occ_head, 'ROUTED_LOSS', {k: True for k in occ_head.ROUTED_LOSS})
    head = OT.module_head()
    feats, sem, cam = OT.module_inputs()
    net = types.SimpleNamespace(occ_head=head, mixed_feats=lambda f: f[0], occ_logits=lambda f: head(f[0]))

    def step():
        head.zero_grad(set_to_none=True)
        x = feats.clone().requires_grad_()
        out = DHD.forward_occ_train(net, [x], sem, cam)
        sum(out.values()).backward()
        return [out[k].detach() for k in ('loss_occ', 'loss_voxel_sem_scal', 'loss_voxel_geo_scal')] + [x.grad] + [p.grad.clone() for p in head.parameters()]
    assert 'fused_loss' not in vars(head)
    want = step()
    before = dict(vars(head))
    assert dhd_amd.fused_occ_head_loss(head) == [head] and head.fused_loss is True and not head._loss_applies(feats)
    assert {k for k in vars(head) if k not in before} == {'fused_loss'}
    got = step()
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert dhd_amd.fused_occ_head_loss(head, False) == [head] and head.fused_loss is False
    del head.fused_loss
    assert predictor.fused_infer is False and 'predictor' in dhd_amd.fused_occ_head_loss.__doc__


def test_the_switch_is_off_and_the_environment_variable_sets_the_class_default():
    from dhd_amd.detector import predictor
    assert 'DHD_OCC_HEAD_LOSS' in os.environ or predictor.fused_loss is False
    code = 'from dhd_amd.detector import predictor as P; print(P.fused_loss, P.fused_train)'
    for value, want in ((None, 'False False'), ('1', 'True False')):
        env = {k: v for k, v in os.environ.items() if k not in ('DHD_OCC_HEAD_LOSS', 'DHD_OCC_HEAD_TRAIN')}
        if value is not None:
            env['DHD_OCC_HEAD_LOSS'] = value
        out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT, env=env)
        assert out.returncode == 0 and out.stdout.split('\n')[0] == want, (value, out.stdout, out.stderr[-800:])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_the_new_kernels_use_no_private_memory(tmp_path):
    """occ_head.hip compiled to gfx950 assembly with the Makefile's flags: every instantiation of the forward with the loss sums,
    of the backward with the loss gradient (3 types x 2 layouts each), of its stream packer and the finalize launch reports a
    private segment of 0 bytes and at most 512 registers."""
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    flags = re.search(r'^HIPFLAGS \?= (.*?)(?<!\\)$', mk, flags=re.S | re.M).group(1).replace('\\\n', ' ').replace('$(ARCH)', 'gfx950').split()
    flags = [f for f in flags if f not in ('-fPIC', '-Wall')]
    out = tmp_path / 'occ_head.s'
    subprocess.run([HIPCC] + flags + ['--cuda-device-only', '-S', os.path.join(CSRC, 'occ_head.hip'), '-o', str(out)], check=True,
                   capture_output=True, timeout=900)
    meta = re.findall(r'\.name:\s+(\S+)\n(?:(?!\.name:).)*?\.private_segment_fixed_size:\s+(\d+)(?:(?!\.name:).)*?\.vgpr_count:\s+(\d+)',
                      open(out).read(), flags=re.S)
    fwd = {n: (int(p), int(r)) for n, p, r in meta if re.search(r'occ_head_kernelI\w+?Lb[01]ELb1EEEv', n)}
    bwd = {n: (int(p), int(r)) for n, p, r in meta if 'occ_head_loss_bwd_kernel' in n}
    rest = {n: (int(p), int(r)) for n, p, r in meta if 'pack_loss_stream_kernel' in n or 'occ_loss_finalize' in n}
    assert (len(fwd), len(bwd), len(rest)) == (6, 6, 4), (sorted(fwd), sorted(bwd), sorted(rest))
    for n, (private, regs) in {**fwd, **bwd, **rest}.items():
        print(n[:70], 'private', private, 'registers', regs)
        assert private == 0 and regs <= 512, n


def test_the_inputs_are_what_they_are_said_to_be():
    for case, (b, dy, dx) in OT.SHAPES.items():
        sem, cam = OL.labels(case)
        assert sem.dtype == torch.uint8 and cam.dtype == torch.bool and tuple(sem.shape) == tuple(cam.shape) == (b, dx, dy, OT.DZ)
        valid = cam & (sem != OL.IGNORE)
        assert not bool((sem == OL.ABSENT).any()) and bool(valid.any())
        assert set(sem.unique().tolist()) <= set(range(OT.N_CLS)) | {OL.IGNORE}
        if b > 1:
            assert not bool(valid[OL.EMPTY_SAMPLE].any()) and bool(cam[OL.EMPTY_SAMPLE].any()) and all(bool(valid[i].any()) for i in range(b) if i != OL.EMPTY_SAMPLE)
        if sem.numel() >= 1000:
            rest = cam if b == 1 else cam[[i for i in range(b) if i != OL.EMPTY_SAMPLE]]
            assert 0.65 < float(rest.double().mean()) < 0.75 and bool((sem == OL.IGNORE).any())
    # the twin's losses are finite and its gradients are not all zero; the weights are the unequal ones
    t = OL.twin('partial_wave', 'f32')
    assert OL.WEIGHTS == (0.7, 1.3, 2.0) and t['losses'].dtype == torch.float64 and bool(torch.isfinite(t['losses']).all())
    assert all(t[k].dtype == torch.float64 and float(t[k].abs().max()) > 0 for k in OT.TENSORS)
    # float32 torch autograd over the same formulation agrees with the twin, float32 rounding apart
    v = OT.inputs('partial_wave', 'f32')
    leaves = {k: v[k].clone().requires_grad_() for k in ('x',) + OT.PARAMS}
    logits = OT.formulation(*(leaves[k] for k in ('x',) + OT.PARAMS))
    losses = OL.losses_f64(logits.double(), 'partial_wave')
    sum(w * l for w, l in zip(OL.WEIGHTS, losses)).backward()
    for k in OT.TENSORS:
        g = leaves['x'].grad if k == 'dx' else leaves[k[1:]].grad
        assert float((g.double() - t[k]).abs().max()) <= 5e-5 * OT.scale_of(t[k]), k
