"""The Swin FFN training surface `dhdu_*` of libdhd_amd.so for C = 512 (dhd_amd/include/dhd_amd_ffn_wide_train.h,
dhd_amd/_ffn_wide_train.py) without a GPU: header, binding table and exports agree and leave the other surfaces alone; the entry
points refuse bad input on the host with the documented code; and the host-side pieces of the routing -- the switch that is off,
what it sets and what it leaves alone, and the float64 autograd twin the GPU tests measure against."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_ffn_train_wide_inputs as SW  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
OWN_INCLUDE = os.path.join(ROOT, 'dhd_amd', 'include')
HEADER = os.path.join(OWN_INCLUDE, 'dhd_amd_ffn_wide_train.h')
CSRC = os.path.join(ROOT, 'dhd_amd', 'csrc')
EINVAL, ENOSPACE, EUNSUPPORTED = -1, -2, -3
WANT = ['dhdu_swin_ffn_wide_backward', 'dhdu_swin_ffn_wide_backward_scratch_bytes', 'dhdu_swin_ffn_wide_forward',
        'dhdu_swin_ffn_wide_forward_scratch_bytes', 'dhdu_swin_ffn_wide_supported']
COMBOS = ((0, 0), (0, 1), (0, 2), (1, 1), (2, 2))          # (x_dtype, mm_dtype) codes: DHD_F32 0, DHD_F16 1, DHD_BF16 2
MAX_ROWS = 1 << 36                                         # the wide family's row limit


def _declarations(header, prefix):
    """{name: number of parameters} of the functions a header declares."""
    src = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return {name: len(params.split(',')) for name, params in re.findall(r'\b(?:int|size_t)\s+(%s[a-z0-9_]+)\s*\(([^)]*)\)' % prefix, src)}


def test_header_binding_table_and_exports_agree():
    from dhd_amd import _ext, _ffn, _ffn_train, _ffn_wide, _ffn_wide_train, _lib, _seam
    declared = _declarations(HEADER, 'dhdu_')
    assert sorted(declared) == WANT == sorted(_ffn_wide_train.EXPORTED_SYMBOLS)
    lib = _ffn_wide_train.load()
    assert lib is _lib.load() and lib is _ffn_train.load()           # the same library, the same handle
    for name, (argtypes, restype) in _ffn_wide_train._PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
        assert len(argtypes) == declared[name], name                 # the header is not compiled into the library: held here
    # argument for argument the dhdt_* five
    narrow = _declarations(os.path.join(INCLUDE, 'dhd_amd_ffn_train.h'), 'dhdt_')
    for name, (argtypes, restype) in _ffn_wide_train._PROTOTYPES.items():
        twin = name.replace('dhdu_swin_ffn_wide', 'dhdt_swin_ffn')
        assert _ffn_train._PROTOTYPES[twin] == (argtypes, restype) and narrow[twin] == declared[name], name
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r' T (dhdu_[a-z0-9_]+)', out)) == set(WANT)
    # the other surfaces are what they were: the family is in none of their tables, and the ABI number did not move
    for other in (_lib, _ext, _ffn, _ffn_wide, _seam, _ffn_train):
        assert not any(n.startswith('dhdu') for n in other._PROTOTYPES), other.__name__
    assert (len(_ext._PROTOTYPES), len(_ffn._PROTOTYPES), len(_ffn_wide._PROTOTYPES), len(_seam._PROTOTYPES), len(_ffn_train._PROTOTYPES)) == (5, 3, 3, 8, 5)
    assert _lib.ABI_VERSION == 6 and lib.dhd_abi_version() == 6
    assert re.search(r'#define DHD_ABI_VERSION 6\b', open(os.path.join(INCLUDE, 'dhd_amd.h')).read())
    text = open(HEADER).read()
    assert '#include "dhd_amd.h"' in text and 'DHD_ABI_VERSION is unchanged' in text
    assert not any(p in text for p in ('dhds_', 'dhdg_', 'dhdf_', 'dhdx_', 'dhdt_'))
    # include/ still lists its six headers and none of them names the family; the new header is the only one beside the package
    assert sorted(os.listdir(INCLUDE)) == ['dhd_amd.h', 'dhd_amd_ext.h', 'dhd_amd_ffn.h', 'dhd_amd_ffn_train.h', 'dhd_amd_ffn_wide.h',
                                           'dhd_amd_seam.h']
    for other in os.listdir(INCLUDE):
        assert 'dhdu_' not in open(os.path.join(INCLUDE, other)).read(), other
    assert os.listdir(OWN_INCLUDE) == ['dhd_amd_ffn_wide_train.h']


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / 'h.c'
    src.write_text('#include "dhd_amd_ffn_wide_train.h"\nint main(void) { return dhdu_swin_ffn_wide_supported(512, 2048, DHD_F32, DHD_BF16) ? 0 : 1; }\n')
    out = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + INCLUDE, '-I' + OWN_INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_the_makefile_keeps_its_translation_units_and_knows_the_headers():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith('SRCS')).split(':=')[1].split()
    assert 'swin_ffn.hip' in srcs and len(srcs) == 22                # a header of swin_ffn.hip, not a translation unit
    assert not [f for f in os.listdir(CSRC) if f.endswith('.hip') and ('wide' in f or 'seam' in f)]
    rule = next(ln for ln in mk.splitlines() if ln.startswith('%.o:')).split()
    assert 'swin_ffn_wide_train.h' in rule and '../include/dhd_amd_ffn_wide_train.h' in rule
    assert all(h in rule for h in ('swin_ffn_train.h', '../../include/dhd_amd_ffn_train.h', 'swin_ffn_wide.h', '../../include/dhd_amd_ffn_wide.h'))
    assert all(os.path.exists(os.path.join(CSRC, h)) for h in rule[2:])
    hip = open(os.path.join(CSRC, 'swin_ffn.hip')).read()
    at = [hip.index(f'#include "{h}"') for h in ('swin_ffn_wide.h', 'swin_ffn_train.h', 'swin_ffn_wide_train.h')]
    assert at[2] > at[1] and at[2] > at[0]                           # after the two headers whose helpers it reuses
    own = open(os.path.join(CSRC, 'swin_ffn_wide_train.h')).read()
    assert 'gelu_erf_grad(' in own and not re.search(r'float\s+gelu_erf\w*\s*\(', own) and not re.search(r'void\s+gelu_erf_grad\s*\(', own)
    for helper in ('make_parts', 'mfma16', 'mfma_parts', 'ring_size', 'pair_quads', 'col_sums16'):
        assert not re.search(r'\b%s\s*\([^;{]*\)\s*\{' % helper, own), helper      # used, not defined again


def test_supported_set_and_scratch_bytes():
    from dhd_amd import _ffn_train, _ffn_wide, _ffn_wide_train
    lib = _ffn_wide_train.load()
    _ffn_wide.load()
    _ffn_train.load()
    c = 512
    for a in (0, 1, 2):
        for b in (0, 1, 2):
            assert lib.dhdu_swin_ffn_wide_supported(c, 4 * c, a, b) == int((a, b) in COMBOS), (a, b)
    for m in (0, 1, 2):
        f, b1, b300 = (lib.dhdu_swin_ffn_wide_forward_scratch_bytes(c, 4 * c, m), lib.dhdu_swin_ffn_wide_backward_scratch_bytes(1, c, 4 * c, m),
                       lib.dhdu_swin_ffn_wide_backward_scratch_bytes(300, c, 4 * c, m))
        assert f == lib.dhdg_swin_ffn_wide_scratch_bytes(c, 4 * c, m) > 0        # the forward runs on the inference operator's stream
        # the backward's stream: three matrices' worth of fragments in the GEMM type and b1; then one row of 2 c floats per workgroup
        assert b1 >= 3 * c * 4 * c * (4 if m == 0 else 2) + 4 * 4 * c + 2 * c * 4
        t = 32 if m == 0 else 64                                                 # rows of a workgroup
        assert b300 - b1 == (-(-300 // t) - 1) * (2 * c * 4) and (b1 - 2 * c * 4) % 1024 == 0, m
    assert lib.dhdu_swin_ffn_wide_backward_scratch_bytes(300, c, 4 * c, 1) == lib.dhdu_swin_ffn_wide_backward_scratch_bytes(300, c, 4 * c, 2)
    for rows in (0, -1, MAX_ROWS + 1):
        assert lib.dhdu_swin_ffn_wide_backward_scratch_bytes(rows, c, 4 * c, 2) == 0
    assert lib.dhdu_swin_ffn_wide_backward_scratch_bytes(MAX_ROWS, c, 4 * c, 2) > 0
    for c2, hidden in ((128, 512), (256, 1024), (1024, 4096), (512, 1024), (512, 4096), (768, 3072), (0, 0), (-512, -2048), (512, -2048)):
        for a, b in COMBOS:
            assert lib.dhdu_swin_ffn_wide_supported(c2, hidden, a, b) == 0, (c2, hidden)
        assert lib.dhdu_swin_ffn_wide_forward_scratch_bytes(c2, hidden, 2) == 0 and lib.dhdu_swin_ffn_wide_backward_scratch_bytes(300, c2, hidden, 2) == 0
    for bad in (3, -1):
        assert lib.dhdu_swin_ffn_wide_supported(512, 2048, bad, 0) == 0 and lib.dhdu_swin_ffn_wide_supported(512, 2048, 0, bad) == 0
        assert lib.dhdu_swin_ffn_wide_forward_scratch_bytes(512, 2048, bad) == 0 and lib.dhdu_swin_ffn_wide_backward_scratch_bytes(300, 512, 2048, bad) == 0
    # the neighbours accept and reject what they did: the narrow training family no C = 512, the wide inference family both wide sizes
    assert lib.dhdt_swin_ffn_supported(512, 2048, 0, 2) == 0 and lib.dhdt_swin_ffn_supported(128, 512, 0, 2) == 1
    assert lib.dhdg_swin_ffn_wide_supported(512, 2048, 0, 2) == 1 and lib.dhdg_swin_ffn_wide_supported(1024, 4096, 0, 2) == 1


def _bases(lib):
    P = C.c_void_p(0x10000)
    fneed, bneed = lib.dhdu_swin_ffn_wide_forward_scratch_bytes(512, 2048, 2), lib.dhdu_swin_ffn_wide_backward_scratch_bytes(300, 512, 2048, 2)
    #      x gamma beta w1 b1 w2 b2 scale | rpi | out scratch | bytes | x_dtype mm_dtype | rows c hidden | eps | stream
    fwd = [P, P, P, P, P, P, P, P, 100, P, P, fneed, 0, 2, 300, 512, 2048, 1e-5, None]
    #      x dout gamma beta w1 b1 w2 scale | rpi | dx dgamma dbeta xn act dhid scratch | bytes | x_dtype mm_dtype | rows c hidden | eps | stream
    bwd = [P, P, P, P, P, P, P, P, 100, P, P, P, P, P, P, P, bneed, 0, 2, 300, 512, 2048, 1e-5, None]
    return fwd, bwd


# per entry point: the pointer slots that must not be NULL, all pointer slots, and the slots of scale, rows_per_image, scratch bytes, x_dtype
SLOTS = {'dhdu_swin_ffn_wide_forward': (tuple(range(7)) + (9, 10), tuple(range(8)) + (9, 10), 7, 8, 11, 12),
         'dhdu_swin_ffn_wide_backward': (tuple(range(7)) + (9, 10, 11, 15), tuple(range(8)) + tuple(range(9, 16)), 7, 8, 16, 17)}


@pytest.mark.parametrize('name', sorted(SLOTS))
def test_bad_input_is_refused_on_the_host(name):
    """Fake addresses, no device: every call below returns before any launch.  Each base call is valid but for the one thing named."""
    from dhd_amd import _ffn_wide_train
    lib = _ffn_wide_train.load()
    fn = getattr(lib, name)
    base = _bases(lib)[name.endswith('backward')]
    required, pointers, i_scale, i_rpi, i_bytes, i_xd = SLOTS[name]
    i_md, i_rows, i_c, i_hidden = i_xd + 1, i_xd + 2, i_xd + 3, i_xd + 4
    need = base[i_bytes]
    for s in pointers:
        for bad in (None, C.c_void_p(0x10004), C.c_void_p(0x10002)):
            if bad is None and s not in required:
                continue
            a = list(base)
            a[s] = bad
            assert fn(*a) == EINVAL, (s, bad)
    if name.endswith('backward'):                         # the operand triple: all three or none
        for gone in ((12,), (13,), (14,), (12, 13), (12, 14), (13, 14)):
            a = list(base)
            for s in gone:
                a[s] = None
            assert fn(*a) == EINVAL, gone
    for rows in (0, -1):
        a = list(base)
        a[i_rows] = rows
        assert fn(*a) == EINVAL
    for rpi in (0, -100, 7, 301, 600):                    # with a scale: a positive divisor of rows
        a = list(base)
        a[i_rpi] = rpi
        assert fn(*a) == EINVAL, rpi
    for c, hidden in ((96, 384), (512, 1024), (128, 512), (256, 1024), (1024, 4096), (0, 0), (512, 4096)):
        a = list(base)
        a[i_c], a[i_hidden] = c, hidden
        assert fn(*a) == EUNSUPPORTED, (c, hidden)
    for xd, md in ((3, 0), (0, 3), (-1, 0), (0, -1), (1, 2), (2, 1), (1, 0), (2, 0)):      # a code, or a combination, outside the set
        a = list(base)
        a[i_xd], a[i_md] = xd, md
        a[i_bytes] = 1 << 26
        assert fn(*a) == EUNSUPPORTED, (xd, md)
    a = list(base)
    a[i_rows], a[i_rpi] = MAX_ROWS + 1, 1
    assert fn(*a) == EUNSUPPORTED
    # the pointer test comes first, the size check last
    a = list(base)
    a[0], a[i_c] = None, 96
    assert fn(*a) == EINVAL
    for short in (0, 1024, need - 1):
        a = list(base)
        a[i_bytes] = short
        assert fn(*a) == ENOSPACE, short
    a = list(base)
    a[i_bytes], a[i_c], a[i_hidden] = 0, 96, 384
    assert fn(*a) == EUNSUPPORTED
    # without a scale rows_per_image is not looked at: the call gets as far as the size check
    a = list(base)
    a[i_scale], a[i_rpi], a[i_bytes] = None, 0, need - 1
    assert fn(*a) == ENOSPACE


def _block(c=512, hidden=None, **kw):
    from dhd_amd.swin import SwinBlock
    torch.manual_seed(3)
    return SwinBlock(c, c // 32, hidden or 4 * c, window_size=4, shift=False, **kw)


def test_the_switch_is_off_and_sets_only_itself():
    import dhd_amd
    from dhd_amd.swin import PatchMerging, SwinBlock, WindowMSA
    assert 'DHD_SWIN_FFN_TRAIN_WIDE' in os.environ or SwinBlock.fused_ffn_train_wide is False      # off unless the environment asks
    before = SwinBlock.fused_ffn_train_wide
    net = nn.Sequential(_block(128), nn.Identity(), _block(128), PatchMerging(128, 256))

    def state():
        return [(type(m).__name__, sorted((k, v) for k, v in vars(m).items() if k.startswith('fused_'))) for m in net.modules()]
    clean = state()
    blocks = dhd_amd.fused_swin_ffn_training_wide(net)
    assert len(blocks) == 2 and all(isinstance(b, SwinBlock) and b.fused_ffn_train_wide is True for b in blocks)
    # exactly that attribute on exactly the blocks: every other module and every other switch is as it was
    assert [(n, [kv for kv in s if kv[0] != 'fused_ffn_train_wide']) for n, s in state()] == clean
    assert all(vars(m).get('fused_ffn_train_wide') is (True if isinstance(m, SwinBlock) else None) for m in net.modules())
    assert SwinBlock.fused_ffn_train_wide is before and _block(128).fused_ffn_train_wide is before    # instances, not the class
    assert all(b.fused_ffn_train_wide is False for b in dhd_amd.fused_swin_ffn_training_wide(net, False))
    # the other switches set what they set before and do not reach this one
    for fn, cls, attr in ((dhd_amd.fused_training, WindowMSA, 'fused_train'), (dhd_amd.fused_swin_ffn, SwinBlock, 'fused_ffn'),
                          (dhd_amd.fused_swin_glue, SwinBlock, 'fused_glue'), (dhd_amd.fused_inference, WindowMSA, 'fused_infer'),
                          (dhd_amd.fused_swin_seams, PatchMerging, 'fused_seam'), (dhd_amd.fused_swin_ffn_training, SwinBlock, 'fused_ffn_train')):
        snap = state()
        switched = fn(net)
        assert switched and all(isinstance(m, cls) and getattr(m, attr) is True for m in switched)
        assert [(n, [kv for kv in s if kv[0] != attr]) for n, s in state()] == [(n, [kv for kv in s if kv[0] != attr]) for n, s in snap]
        assert all(b.fused_ffn_train_wide is False for b in blocks)
    assert callable(dhd_amd.swin_ffn_train_wide_supported) and callable(dhd_amd.swin_ffn_train_supported)


def test_the_environment_variable_sets_the_class_default():
    code = 'from dhd_amd.swin import SwinBlock as B; print(B.fused_ffn_train_wide, B.fused_ffn_train, B.fused_ffn, B.fused_glue)'
    names = ('DHD_SWIN_FFN_TRAIN_WIDE', 'DHD_SWIN_FFN_TRAIN', 'DHD_SWIN_FFN', 'DHD_SWIN_GLUE')
    for set_, want in ((None, 'False False False False'), ('DHD_SWIN_FFN_TRAIN_WIDE', 'True False False False'),
                       ('DHD_SWIN_FFN_TRAIN', 'False True False False')):
        env = {k: v for k, v in os.environ.items() if k not in names}
        if set_ is not None:
            env[set_] = '1'
        out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT, env=env)
        assert out.returncode == 0 and out.stdout.split('\n')[0] == want, (set_, out.stdout, out.stderr[-800:])


@pytest.mark.parametrize('mode', ('train', 'eval'))
def test_on_cpu_tensors_the_flag_changes_nothing(monkeypatch, mode):
    """The operator is stubbed to raise and the routing table says yes to everything: on CPU tensors the output and every
    gradient of a SwinBlock(512, 16, 2048) are today's, bit for bit, with the same random draws."""
    import dhd_amd
    from dhd_amd import swin_ffn

    def boom(*a, **k):
        raise AssertionError('the fused operator was reached')
    monkeypatch.setattr(swin_ffn, 'swin_ffn', boom)
    monkeypatch.setattr(swin_ffn, 'ROUTED_TRAIN_WIDE', {k: True for k in swin_ffn.ROUTED_TRAIN_WIDE})
    block = _block(drop_path_rate=0.5)
    assert block.norm2.normalized_shape == (512,) and block.ffn.layers[0][0].out_features == 2048
    block.train(mode == 'train')
    x = torch.randn(2, 5 * 7, 512, generator=torch.Generator().manual_seed(4))

    def step():
        torch.manual_seed(9)
        block.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_()
        out = block(xg, (5, 7))
        out.square().sum().backward()
        return [out.detach(), xg.grad] + [p.grad for p in block.parameters()], torch.get_rng_state()
    want, rng = step()
    dhd_amd.fused_swin_ffn_training_wide(block)
    assert block.fused_ffn_train_wide is True and not block._ffn_train_wide_applies(x)
    got, rng_on = step()
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)) and torch.equal(rng, rng_on)
    from dhd_amd.swin_ffn import swin_ffn_train_wide_shape_supported, swin_ffn_train_wide_supported
    assert not swin_ffn_train_wide_shape_supported(x, 2048) and not swin_ffn_train_wide_supported(x, 2048)
    monkeypatch.undo()
    with pytest.raises(dhd_amd._lib.DhdError):                               # no fallback: the operator is HIP only
        dhd_amd.swin_ffn(x, torch.ones(512), torch.zeros(512), 1e-5, torch.zeros(2048, 512), torch.zeros(2048), torch.zeros(512, 2048), torch.zeros(512))


def test_the_routing_tables_name_only_what_their_operators_take():
    from dhd_amd import _ffn_train, _ffn_wide_train, _lib, swin_ffn
    lib = _ffn_wide_train.load()
    _ffn_train.load()
    assert sorted((c, _lib.DTYPE_CODE[x], _lib.DTYPE_CODE[m]) for c, x, m in swin_ffn.ROUTED_TRAIN_WIDE) == sorted((512, a, b) for a, b in COMBOS)
    for (c, xdt, mdt), on in swin_ffn.ROUTED_TRAIN_WIDE.items():
        assert isinstance(on, bool)
        assert lib.dhdu_swin_ffn_wide_supported(c, 4 * c, _lib.DTYPE_CODE[xdt], _lib.DTYPE_CODE[mdt]) == 1, (c, xdt, mdt)
    # the narrow table is what it was: its 10 keys, none of them C = 512
    assert len(swin_ffn.ROUTED_TRAIN) == 10 and sorted({c for c, _, _ in swin_ffn.ROUTED_TRAIN}) == [128, 256]
    for (c, xdt, mdt) in swin_ffn.ROUTED_TRAIN:
        assert lib.dhdt_swin_ffn_supported(c, 4 * c, _lib.DTYPE_CODE[xdt], _lib.DTYPE_CODE[mdt]) == 1
        assert lib.dhdu_swin_ffn_wide_supported(c, 4 * c, _lib.DTYPE_CODE[xdt], _lib.DTYPE_CODE[mdt]) == 0


@pytest.mark.parametrize('case,sname', (('r33_c512', 'none'), ('r300_c512', 'drop'), ('r129_c512_tails', 'none')))
def test_the_twin_agrees_with_the_float32_module_formulation(case, sname):
    """The twin against torch's own float32 autograd over the same formulation on the CPU: float32 rounding apart; the grid holds
    what the issue lists; the tails case reaches both tails of gelu'."""
    rows, tails = SW.CASES[case]
    v, s = SW.inputs(case, 'f32'), SW.scale_tensor(sname)
    got, ref = SW.parent(v, torch.float32, torch.float32, s, 'cpu'), SW.twin(case, 'f32', sname)
    for k in SW.TENSORS:
        err = float((got[k].double() - ref[k]).abs().max())
        print(f'{case} [{sname}] {k}: max |float32 - twin| = {err:.3e}')
        assert ref[k].dtype == torch.float64 and tuple(ref[k].shape) == tuple(got[k].shape)
        assert err <= 5e-5 * SW.scale_of(ref[k]), k
    if sname == 'drop':                                    # the dropped image: out is x and dx is dout
        assert torch.equal(ref['out'][100:200], v['x'][100:200].double()) and torch.equal(ref['dx'][100:200], v['dout'][100:200].double())
    if tails:
        import torch.nn.functional as F
        pre = F.linear(F.layer_norm(v['x'].double(), (512,), v['gamma'].double(), v['beta'].double(), SW.EPS), v['w1'].double(), v['b1'].double())
        assert abs(float(pre.abs().max()) - SW.TAIL) < 1e-4 and float(pre.min()) < -8 and float(pre.max()) > 8
    assert sorted({r for r, _ in SW.CASES.values()}) == [1, 33, 129, 300] and len(SW.GRID) == 30
    import swin_ffn_train_inputs as ST
    assert all(getattr(SW, n) is getattr(ST, n) for n in ('formulation', 'parent', 'scale_tensor', 'scale_of', '_collect'))
