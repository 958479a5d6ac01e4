"""The Swin FFN surface `dhdf_*` of libdhd_amd.so (include/dhd_amd_ffn.h, dhd_amd/_ffn.py) without a GPU: its own copies of the
guarantees tests/test_capi.py and tests/test_swin_glue_capi.py hold for the other two surfaces -- header, binding table and
exports agree; the entry point refuses bad input on the host with the documented code -- plus the host-side pieces of the
routing: the switch that is off, what it leaves alone, and the float64 twin the GPU tests measure against."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_ffn_inputs as SF  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'dhd_amd_ffn.h')
EINVAL, ENOSPACE, EUNSUPPORTED = -1, -2, -3
WANT = ['dhdf_swin_ffn_infer', 'dhdf_swin_ffn_scratch_bytes', 'dhdf_swin_ffn_supported']
COMBOS = ((0, 0), (0, 1), (0, 2), (1, 1), (2, 2))          # (x_dtype, mm_dtype) codes: DHD_F32 0, DHD_F16 1, DHD_BF16 2


def declared_symbols():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(?:int|size_t)\s+(dhdf_[a-z0-9_]+)\s*\(', src)))


def test_header_binding_table_and_exports_agree():
    from dhd_amd import _ext, _ffn, _lib
    assert declared_symbols() == WANT == sorted(_ffn.EXPORTED_SYMBOLS)
    lib = _ffn.load()
    assert lib is _lib.load() and lib is _ext.load()                 # the same library, the same handle
    for name, (argtypes, restype) in _ffn._PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r' T (dhdf_[a-z0-9_]+)', out)) == set(WANT)
    # the other two surfaces are what they were: nothing of the family leaked into their tables, the ABI number did not move
    assert not any(n.startswith('dhdf') for n in _lib._PROTOTYPES) and not any(n.startswith('dhdf') for n in _ext._PROTOTYPES)
    assert len(_ext._PROTOTYPES) == 5 and all(n.startswith('dhdx_') for n in _ext._PROTOTYPES)
    assert all(n.startswith('dhd_') for n in _lib._PROTOTYPES)
    assert _lib.ABI_VERSION == 6 and lib.dhd_abi_version() == 6
    assert re.search(r'#define DHD_ABI_VERSION 6\b', open(os.path.join(ROOT, 'include', 'dhd_amd.h')).read())
    assert '#include "dhd_amd.h"' in open(HEADER).read()
    for other in ('dhd_amd.h', 'dhd_amd_ext.h'):
        assert 'dhdf_' not in open(os.path.join(ROOT, 'include', other)).read()


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / 'h.c'
    src.write_text('#include "dhd_amd_ffn.h"\nint main(void) { return dhdf_swin_ffn_supported(128, 512, DHD_F32, DHD_BF16) ? 0 : 1; }\n')
    out = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + os.path.join(ROOT, 'include'), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_the_makefile_builds_the_translation_unit():
    mk = open(os.path.join(ROOT, 'dhd_amd', 'csrc', 'Makefile')).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith('SRCS')).split(':=')[1].split()
    assert 'swin_ffn.hip' in srcs and os.path.exists(os.path.join(ROOT, 'dhd_amd', 'csrc', 'swin_ffn.hip'))
    assert 'swin_glue.hip' in srcs and 'occ_head.hip' in srcs and len(srcs) == 22        # everything that was there is there
    rule = next(ln for ln in mk.splitlines() if ln.startswith('%.o:'))
    assert 'dhd_amd_ffn.h' in rule and 'dhd_amd_ext.h' in rule and 'window_geom.h' in rule and 'dhd_amd.h' in rule


def test_supported_set_and_scratch_bytes():
    from dhd_amd import _ffn
    lib = _ffn.load()
    for c in (128, 256):
        for a in (0, 1, 2):
            for b in (0, 1, 2):
                assert lib.dhdf_swin_ffn_supported(c, 4 * c, a, b) == int((a, b) in COMBOS), (c, a, b)
        for m in (0, 1, 2):
            n = lib.dhdf_swin_ffn_scratch_bytes(c, 4 * c, m)
            # at least the two matrices in the GEMM type (two bf16 parts of a float32 weight) and b1; whole 1 KiB fragments
            assert n >= 2 * c * 4 * c * (4 if m == 0 else 2) + 4 * 4 * c and n % 1024 == 0, (c, m, n)
        assert lib.dhdf_swin_ffn_scratch_bytes(c, 4 * c, 1) == lib.dhdf_swin_ffn_scratch_bytes(c, 4 * c, 2)
    for c, hidden in ((128, 256), (128, 1024), (256, 512), (96, 384), (64, 256), (0, 0), (-128, -512), (512, 2048), (1024, 4096)):
        assert lib.dhdf_swin_ffn_supported(c, hidden, 0, 0) == 0, (c, hidden)
        assert lib.dhdf_swin_ffn_scratch_bytes(c, hidden, 0) == 0, (c, hidden)      # 0 for sizes the operator does not take
    for bad in (3, -1):
        assert lib.dhdf_swin_ffn_supported(128, 512, bad, 0) == 0 and lib.dhdf_swin_ffn_supported(128, 512, 0, bad) == 0
        assert lib.dhdf_swin_ffn_scratch_bytes(128, 512, bad) == 0


def test_bad_input_is_refused_on_the_host():
    """Fake addresses, no device: every call below returns before any launch.  Each base call is valid but for the one thing named."""
    from dhd_amd import _ffn
    lib = _ffn.load()
    fn = lib.dhdf_swin_ffn_infer
    P = C.c_void_p(0x10000)
    need = lib.dhdf_swin_ffn_scratch_bytes(128, 512, 2)
    #       x gamma beta w1 b1 w2 b2 out scratch | bytes | x_dtype mm_dtype | rows c hidden | eps | stream
    base = [P, P, P, P, P, P, P, P, P, need, 0, 2, 300, 128, 512, 1e-5, None]
    for s in range(9):
        for bad in (None, C.c_void_p(0x10004), C.c_void_p(0x10002)):
            a = list(base)
            a[s] = bad
            assert fn(*a) == EINVAL, (s, bad)          # gamma or beta alone NULL: the LayerNorm is there or it is not
    for rows in (0, -1):
        a = list(base)
        a[12] = rows
        assert fn(*a) == EINVAL
    for c, hidden in ((96, 384), (128, 256), (512, 2048), (1024, 4096), (0, 0), (256, 512)):
        a = list(base)
        a[13], a[14] = c, hidden
        assert fn(*a) == EUNSUPPORTED, (c, hidden)
    for xd, md in ((3, 0), (0, 3), (-1, 0), (0, -1), (1, 2), (2, 1), (1, 0), (2, 0)):      # a code, or a combination, outside the set
        a = list(base)
        a[10], a[11] = xd, md
        a[9] = 1 << 24
        assert fn(*a) == EUNSUPPORTED, (xd, md)
    a = list(base)
    a[12] = (1 << 37) + 1
    assert fn(*a) == EUNSUPPORTED
    # the pointer test comes first, the size check last
    a = list(base)
    a[0], a[13] = None, 96
    assert fn(*a) == EINVAL
    for short in (0, 1024, need - 1):
        a = list(base)
        a[9] = short
        assert fn(*a) == ENOSPACE, short
    a = list(base)
    a[9], a[13], a[14] = 0, 96, 384
    assert fn(*a) == EUNSUPPORTED
    for xd, md in COMBOS:                                # every combination asks for its own scratch size
        a = list(base)
        a[10], a[11] = xd, md
        a[9] = lib.dhdf_swin_ffn_scratch_bytes(128, 512, md) - 1
        assert fn(*a) == ENOSPACE, (xd, md)


def _block(c=128, hidden=None):
    from dhd_amd.swin import SwinBlock
    torch.manual_seed(3)
    return SwinBlock(c, c // 32, hidden or 4 * c, window_size=4, shift=False).eval()


def test_the_switch_is_off_and_sets_instances():
    import dhd_amd
    from dhd_amd.swin import SwinBlock
    assert 'DHD_SWIN_FFN' in os.environ or SwinBlock.fused_ffn is False      # off unless the environment asks
    before = SwinBlock.fused_ffn
    net = nn.Sequential(_block(), nn.Identity(), _block())
    blocks = dhd_amd.fused_swin_ffn(net)
    assert len(blocks) == 2 and all(isinstance(b, SwinBlock) and b.fused_ffn is True and 'fused_ffn' in vars(b) for b in blocks)
    assert SwinBlock.fused_ffn is before and _block().fused_ffn is before    # instances, not the class
    assert all(b.fused_ffn is False for b in dhd_amd.fused_swin_ffn(net, False))
    # fused_inference does not reach it
    dhd_amd.fused_inference(net)
    assert all(b.fused_ffn is False for b in blocks)
    assert callable(dhd_amd.swin_ffn_infer) and callable(dhd_amd.swin_ffn_supported)


def test_with_the_switch_on_cpu_and_grad_inputs_take_todays_path(monkeypatch):
    """The operator is stubbed to raise, and the routing table says yes to everything: a CPU input, and an input that requires
    grad, are still today's two lines, bit for bit."""
    import dhd_amd
    from dhd_amd import swin_ffn
    from dhd_amd.swin import SwinBlock

    def boom(*a, **k):
        raise AssertionError('the fused operator was reached')
    monkeypatch.setattr(swin_ffn, 'swin_ffn_infer', boom)
    monkeypatch.setattr(swin_ffn, 'ROUTED', {k: True for k in swin_ffn.ROUTED})
    block = _block()
    x = torch.randn(2, 13 * 19, 128, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        want = block(x, (13, 19))
    want_grad = block(x.clone().requires_grad_(), (13, 19)).detach()          # (SDPA may pick another kernel when it saves for backward)
    dhd_amd.fused_swin_ffn(block)
    assert block.fused_ffn is True and not block._ffn_applies(x)
    with torch.no_grad():
        assert torch.equal(block(x, (13, 19)), want)                         # a CPU tensor
    xg = x.clone().requires_grad_()
    out = block(xg, (13, 19))                                                # grad enabled, parameters require grad
    assert torch.equal(out.detach(), want_grad) and out.requires_grad
    out.sum().backward()
    assert xg.grad is not None and block.ffn.layers[1].weight.grad is not None
    block.train()
    assert not block._ffn_applies(x)
    from dhd_amd.swin_ffn import swin_ffn_shape_supported
    assert not swin_ffn_shape_supported(x, 512)
    with pytest.raises(dhd_amd._lib.DhdError):                               # no fallback: the operator is HIP only
        dhd_amd.swin_ffn_infer(x, None, None, 1e-5, torch.zeros(512, 128), torch.zeros(512), torch.zeros(128, 512), torch.zeros(128))


def test_the_routing_table_names_only_what_the_operator_takes():
    from dhd_amd import _ffn, _lib, swin_ffn
    lib = _ffn.load()
    assert len(swin_ffn.ROUTED) == 10
    for (c, xdt, mdt), on in swin_ffn.ROUTED.items():
        assert isinstance(on, bool)
        assert lib.dhdf_swin_ffn_supported(c, 4 * c, _lib.DTYPE_CODE[xdt], _lib.DTYPE_CODE[mdt]) == 1, (c, xdt, mdt)


@pytest.mark.parametrize('case', ('r33_c128_ln', 'r300_c256_plain', 'r129_c128_tails', 'r129_c256_tails'))
def test_the_twin_agrees_with_the_float32_module_formulation(case):
    """The twin against torch's own float32 modules (nn.LayerNorm, FFN) on the CPU: float32 rounding of a 4C-long sum apart."""
    from dhd_amd.swin import FFN
    rows, c, ln, tails = SF.CASES[case]
    v = SF.inputs(case, 'f32')
    ffn = FFN(c, 4 * c).eval()
    norm = nn.LayerNorm(c, eps=SF.EPS)
    with torch.no_grad():
        ffn.layers[0][0].weight.copy_(v['w1']); ffn.layers[0][0].bias.copy_(v['b1'])       # noqa: E702
        ffn.layers[1].weight.copy_(v['w2']); ffn.layers[1].bias.copy_(v['b2'])             # noqa: E702
        if ln:
            norm.weight.copy_(v['gamma']); norm.bias.copy_(v['beta'])                      # noqa: E702
        got = ffn(norm(v['x']), identity=v['x']) if ln else ffn(v['x'])
    ref = SF.twin(case, 'f32')
    err = float((got.double() - ref).abs().max())
    print(f'{case}: max |module - twin| = {err:.3e}')
    assert tuple(ref.shape) == (rows, c) and ref.dtype == torch.float64
    assert err <= 2e-5 * SF.scale_of(ref)
    assert torch.equal(SF.parent(v, torch.float32, torch.float32, 'cpu'), got)
    if tails:
        pre = SF.pre_activation64(v['x'], v['gamma'], v['beta'], v['w1'], v['b1'])
        assert abs(float(pre.abs().max()) - SF.TAIL) < 1e-4 and float(pre.min()) < -8 and float(pre.max()) > 8     # both tails
    assert 1.0 < float(ref.abs().max()) < 16.0                                # outputs are O(1)
