"""The wide Swin FFN surface `dhdg_*` of libdhd_amd.so (include/dhd_amd_ffn_wide.h, dhd_amd/_ffn_wide.py) without a GPU: the
counterpart of tests/test_swin_ffn_capi.py -- header, binding table and exports agree; the entry point refuses bad input on the
host with the documented code in the documented order -- plus the host-side pieces of the routing: the second table, what the
switch leaves alone at C = 512, and the float64 twin the GPU tests measure against."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_ffn_wide_inputs as SW  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'dhd_amd_ffn_wide.h')
CSRC = os.path.join(ROOT, 'dhd_amd', 'csrc')
EINVAL, ENOSPACE, EUNSUPPORTED = -1, -2, -3
WANT = ['dhdg_swin_ffn_wide_infer', 'dhdg_swin_ffn_wide_scratch_bytes', 'dhdg_swin_ffn_wide_supported']
COMBOS = ((0, 0), (0, 1), (0, 2), (1, 1), (2, 2))          # (x_dtype, mm_dtype) codes: DHD_F32 0, DHD_F16 1, DHD_BF16 2


def declared_symbols():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(?:int|size_t)\s+(dhdg_[a-z0-9_]+)\s*\(', src)))


def test_header_binding_table_and_exports_agree():
    from dhd_amd import _ext, _ffn, _ffn_wide, _lib
    assert declared_symbols() == WANT == sorted(_ffn_wide.EXPORTED_SYMBOLS)
    lib = _ffn_wide.load()
    assert lib is _lib.load() and lib is _ext.load() and lib is _ffn.load()          # the same library, the same handle
    for name, (argtypes, restype) in _ffn_wide._PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
    # argument for argument the dhdf_ three
    narrow = {n.replace('dhdf_swin_ffn', 'dhdg_swin_ffn_wide'): p for n, p in _ffn._PROTOTYPES.items()}
    assert narrow == _ffn_wide._PROTOTYPES
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r' T (dhdg_[a-z0-9_]+)', out)) == set(WANT)
    # the three older surfaces are what they were
    for table in (_lib._PROTOTYPES, _ext._PROTOTYPES, _ffn._PROTOTYPES):
        assert not any('dhdg' in n for n in table)
    assert len(_ffn._PROTOTYPES) == 3 and len(_ext._PROTOTYPES) == 5
    assert _lib.ABI_VERSION == 6 and lib.dhd_abi_version() == 6
    assert '#include "dhd_amd.h"' in open(HEADER).read()
    for other in ('dhd_amd.h', 'dhd_amd_ext.h', 'dhd_amd_ffn.h'):
        assert 'dhdg_' not in open(os.path.join(ROOT, 'include', other)).read()


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / 'h.c'
    src.write_text('#include "dhd_amd_ffn_wide.h"\nint main(void) { return dhdg_swin_ffn_wide_supported(512, 2048, DHD_F32, DHD_BF16) ? 0 : 1; }\n')
    out = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + os.path.join(ROOT, 'include'), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_the_kernels_live_in_a_header_of_swin_ffn_hip():
    assert os.path.exists(os.path.join(CSRC, 'swin_ffn_wide.h'))
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    rule = next(ln for ln in mk.splitlines() if ln.startswith('%.o:'))
    assert 'swin_ffn_wide.h' in rule.split() and 'dhd_amd_ffn_wide.h' in rule and 'dhd_amd_ffn.h' in rule
    hip = open(os.path.join(CSRC, 'swin_ffn.hip')).read()
    assert '#include "swin_ffn_wide.h"' in hip
    assert hip.index('#include "swin_ffn_wide.h"') > hip.index('float gelu_erf(')          # after the helpers it reuses
    wide = open(os.path.join(CSRC, 'swin_ffn_wide.h')).read()
    assert 'gelu_erf(' in wide and not re.search(r'float\s+gelu_erf\s*\(', wide)            # one GELU, not a copy
    assert not [f for f in os.listdir(CSRC) if f.endswith('.hip') and 'wide' in f]         # no new translation unit


def test_supported_set_and_scratch_bytes():
    from dhd_amd import _ffn, _ffn_wide
    lib = _ffn_wide.load()
    _ffn.load()
    for c in (512, 1024):
        for a in (0, 1, 2):
            for b in (0, 1, 2):
                assert lib.dhdg_swin_ffn_wide_supported(c, 4 * c, a, b) == int((a, b) in COMBOS), (c, a, b)
        for m in (0, 1, 2):
            n = lib.dhdg_swin_ffn_wide_scratch_bytes(c, 4 * c, m)
            # at least the two matrices in the GEMM type (two bf16 parts of a float32 weight) and b1; whole 1 KiB fragments
            assert n >= 2 * c * 4 * c * (4 if m == 0 else 2) + 4 * 4 * c and n % 1024 == 0, (c, m, n)
        assert lib.dhdg_swin_ffn_wide_scratch_bytes(c, 4 * c, 1) == lib.dhdg_swin_ffn_wide_scratch_bytes(c, 4 * c, 2)
        # the narrow surface still does not take these
        assert lib.dhdf_swin_ffn_supported(c, 4 * c, 0, 0) == 0 and lib.dhdf_swin_ffn_scratch_bytes(c, 4 * c, 0) == 0
    for c, hidden in ((128, 512), (256, 1024), (512, 1024), (1024, 2048), (512, 4096), (768, 3072), (2048, 8192), (0, 0), (-512, -2048),
                      (512, -2048), (-1024, 4096)):
        for a, b in COMBOS:
            assert lib.dhdg_swin_ffn_wide_supported(c, hidden, a, b) == 0, (c, hidden)
        assert lib.dhdg_swin_ffn_wide_scratch_bytes(c, hidden, 0) == 0, (c, hidden)      # 0 for sizes the operator does not take
    for bad in (3, -1):
        assert lib.dhdg_swin_ffn_wide_supported(512, 2048, bad, 0) == 0 and lib.dhdg_swin_ffn_wide_supported(512, 2048, 0, bad) == 0
        assert lib.dhdg_swin_ffn_wide_scratch_bytes(512, 2048, bad) == 0


def test_bad_input_is_refused_on_the_host():
    """Fake addresses, no device: every call below returns before any launch.  Each base call is valid but for the one thing named."""
    from dhd_amd import _ffn_wide
    lib = _ffn_wide.load()
    fn = lib.dhdg_swin_ffn_wide_infer
    P = C.c_void_p(0x10000)
    need = lib.dhdg_swin_ffn_wide_scratch_bytes(512, 2048, 2)
    #       x gamma beta w1 b1 w2 b2 out scratch | bytes | x_dtype mm_dtype | rows c hidden | eps | stream
    base = [P, P, P, P, P, P, P, P, P, need, 0, 2, 300, 512, 2048, 1e-5, None]
    for s in range(9):
        for bad in (None, C.c_void_p(0x10004), C.c_void_p(0x10002)):
            a = list(base)
            a[s] = bad
            assert fn(*a) == EINVAL, (s, bad)          # gamma or beta alone NULL: the LayerNorm is there or it is not
    for rows in (0, -1):
        a = list(base)
        a[12] = rows
        assert fn(*a) == EINVAL
    for c, hidden in ((128, 512), (256, 1024), (512, 1024), (768, 3072), (2048, 8192), (0, 0), (-512, -2048)):
        a = list(base)
        a[13], a[14] = c, hidden
        assert fn(*a) == EUNSUPPORTED, (c, hidden)
    for xd, md in ((3, 0), (0, 3), (-1, 0), (0, -1), (1, 2), (2, 1), (1, 0), (2, 0)):      # a code, or a combination, outside the set
        a = list(base)
        a[10], a[11] = xd, md
        a[9] = 1 << 26
        assert fn(*a) == EUNSUPPORTED, (xd, md)
    a = list(base)
    a[12] = (1 << 36) + 1
    assert fn(*a) == EUNSUPPORTED
    # the pointer test comes first, the size check last
    a = list(base)
    a[0], a[13] = None, 96
    assert fn(*a) == EINVAL
    a = list(base)
    a[12], a[13], a[9] = 0, 96, 0
    assert fn(*a) == EINVAL
    for short in (0, 1024, need - 1):
        a = list(base)
        a[9] = short
        assert fn(*a) == ENOSPACE, short
    a = list(base)
    a[9], a[13], a[14] = 0, 768, 3072
    assert fn(*a) == EUNSUPPORTED
    for c in (512, 1024):
        for xd, md in COMBOS:                            # every combination asks for its own scratch size
            a = list(base)
            a[10], a[11], a[13], a[14] = xd, md, c, 4 * c
            a[9] = lib.dhdg_swin_ffn_wide_scratch_bytes(c, 4 * c, md) - 1
            assert fn(*a) == ENOSPACE, (c, xd, md)


def test_the_routing_tables_name_only_what_their_family_takes():
    from dhd_amd import _ffn_wide, _lib, swin_ffn
    lib = _ffn_wide.load()
    assert len(swin_ffn.ROUTED_WIDE) == 10 and len(swin_ffn.ROUTED) == 10
    assert {k[0] for k in swin_ffn.ROUTED_WIDE} == {512, 1024} and {k[0] for k in swin_ffn.ROUTED} == {128, 256}
    for (c, xdt, mdt), on in swin_ffn.ROUTED_WIDE.items():
        assert isinstance(on, bool)
        assert lib.dhdg_swin_ffn_wide_supported(c, 4 * c, _lib.DTYPE_CODE[xdt], _lib.DTYPE_CODE[mdt]) == 1, (c, xdt, mdt)


def test_with_the_switch_on_cpu_grad_and_train_take_todays_path(monkeypatch):
    """The operator is stubbed to raise, and both routing tables say yes to everything: at C = 512 a CPU input, an input that
    requires grad, and a block in train mode are still today's two lines, bit for bit."""
    import dhd_amd
    from dhd_amd import swin_ffn
    from dhd_amd.swin import SwinBlock

    def boom(*a, **k):
        raise AssertionError('the fused operator was reached')
    monkeypatch.setattr(swin_ffn, 'swin_ffn_infer', boom)
    monkeypatch.setattr(swin_ffn, 'ROUTED', {k: True for k in swin_ffn.ROUTED})
    monkeypatch.setattr(swin_ffn, 'ROUTED_WIDE', {k: True for k in swin_ffn.ROUTED_WIDE})
    torch.manual_seed(3)
    block = SwinBlock(512, 16, 2048, window_size=4, shift=False).eval()
    x = torch.randn(2, 8 * 12, 512, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        want = block(x, (8, 12))
    want_grad = block(x.clone().requires_grad_(), (8, 12)).detach()           # (SDPA may pick another kernel when it saves for backward)
    block.train()
    want_train = block(x, (8, 12)).detach()
    block.eval()
    dhd_amd.fused_swin_ffn(block)
    assert block.fused_ffn is True and not block._ffn_applies(x)
    with torch.no_grad():
        assert torch.equal(block(x, (8, 12)), want)                          # a CPU tensor
    xg = x.clone().requires_grad_()
    out = block(xg, (8, 12))                                                 # grad enabled, parameters require grad
    assert torch.equal(out.detach(), want_grad) and out.requires_grad
    out.sum().backward()
    assert xg.grad is not None and block.ffn.layers[1].weight.grad is not None
    block.train()
    assert not block._ffn_applies(x)
    assert torch.equal(block(x, (8, 12)).detach(), want_train)
    assert not swin_ffn.swin_ffn_shape_supported(x, 2048) and not swin_ffn.swin_ffn_supported(x, 2048)
    monkeypatch.undo()
    with pytest.raises(dhd_amd._lib.DhdError):                               # no fallback: the operator is HIP only
        dhd_amd.swin_ffn_infer(x, None, None, 1e-5, torch.zeros(2048, 512), torch.zeros(2048), torch.zeros(512, 2048), torch.zeros(512))


@pytest.mark.parametrize('case', ('r33_c512_ln', 'r31_c1024_ln', 'r129_c512_tails', 'r129_c1024_tails'))
def test_the_twin_agrees_with_the_float32_module_formulation(case):
    """The twin against torch's own float32 modules (nn.LayerNorm, FFN) on the CPU: float32 rounding of a 4C-long sum apart."""
    from dhd_amd import _ffn_wide
    from dhd_amd.swin import FFN
    rows, c, ln, tails = SW.CASES[case]
    assert _ffn_wide.value('dhdg_swin_ffn_wide_supported', c, 4 * c, 0, 0) == 1          # a shape the operator takes
    v = SW.inputs(case, 'f32')
    ffn = FFN(c, 4 * c).eval()
    norm = nn.LayerNorm(c, eps=SW.EPS)
    with torch.no_grad():
        ffn.layers[0][0].weight.copy_(v['w1']); ffn.layers[0][0].bias.copy_(v['b1'])       # noqa: E702
        ffn.layers[1].weight.copy_(v['w2']); ffn.layers[1].bias.copy_(v['b2'])             # noqa: E702
        norm.weight.copy_(v['gamma']); norm.bias.copy_(v['beta'])                          # noqa: E702
        got = ffn(norm(v['x']), identity=v['x'])
    ref = SW.twin(case, 'f32')
    err = float((got.double() - ref).abs().max())
    print(f'{case}: max |module - twin| = {err:.3e}')
    assert ln and tuple(ref.shape) == (rows, c) and ref.dtype == torch.float64
    assert err <= 2e-5 * SW.scale_of(ref)
    assert torch.equal(SW.parent(v, torch.float32, torch.float32, 'cpu'), got)
    if tails:
        pre = SW.pre_activation64(v['x'], v['gamma'], v['beta'], v['w1'], v['b1'])
        assert abs(float(pre.abs().max()) - SW.TAIL) < 1e-4 and float(pre.min()) < -8 and float(pre.max()) > 8     # both tails
    assert 1.0 < float(ref.abs().max()) < 16.0                                # outputs are O(1)

