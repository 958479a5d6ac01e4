"""dhd_deform_conv_infer* without a GPU: the ABI surface, the support table, the scratch formula, the host-side refusals (fake
addresses, no device touched), and the Python switches around it."""
import ctypes as C
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('dhd_deform_conv_infer_supported', 'dhd_deform_conv_infer_scratch_bytes', 'dhd_deform_conv_infer')
EINVAL, ENOSPACE, EUNSUPPORTED = -1, -2, -3
F32, F16, BF16 = 0, 1, 2


def _lib():
    from dhd_amd import _lib
    return _lib, _lib.load()


def test_symbols_are_exported_and_bound_and_the_abi_is_still_6():
    _l, lib = _lib()
    for name in NAMES:
        assert name in _l.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    header = open(os.path.join(ROOT, 'include', 'dhd_amd.h')).read()
    assert all(re.search(r'\bint\s+%s\s*\(' % n, header) for n in NAMES)
    assert lib.dhd_abi_version() == 6 == _l.ABI_VERSION and '#define DHD_ABI_VERSION 6' in header


def test_support_table():
    _l, lib = _lib()
    sup = lib.dhd_deform_conv_infer_supported
    # the five channel configurations the operator must take: (c_in, c_out, groups)
    for c, o, g in ((256, 256, 4), (512, 512, 4), (64, 64, 1), (128, 128, 1), (32, 32, 4)):
        for dt in (F32, F16, BF16):
            for layout in (0, 1):
                assert sup(c, o, g, 3, 16, 44, dt, layout, 0) == 1, (c, o, g, dt, layout)
        assert sup(c, o, g, 3, 16, 44, F32, 0, _l.SFA_GEMM['bf16x3']) == 1
    assert sup(64, 128, 1, 3, 7, 9, F32, 1, 0) == 1 and sup(128, 64, 4, 3, 5, 70, BF16, 0, 0) == 1
    assert sup(256, 256, 4, 5, 16, 44, F32, 0, 0) == 0                       # k = 5
    assert sup(16, 16, 4, 3, 16, 44, F32, 0, 0) == 0                         # C / g = 4
    assert sup(136, 136, 1, 3, 16, 44, F32, 0, 0) == 0                       # C / g = 136
    assert sup(12, 12, 4, 3, 16, 44, F32, 0, 0) == 0 and sup(256, 250, 4, 3, 16, 44, F32, 0, 0) == 0
    assert sup(256, 256, 4, 3, 16, 44, F32, 0, _l.SFA_GEMM['bf16x6']) == 0 and sup(256, 256, 4, 3, 16, 44, F32, 0, _l.SFA_GEMM['f32']) == 0
    assert sup(256, 256, 4, 3, 16, 44, F16, 0, _l.SFA_GEMM['bf16x3']) == 0   # gemm selects float32 arithmetic only
    assert sup(256, 256, 4, 3, 16, 44, 3, 0, 0) == 0 and sup(256, 256, 4, 3, 16, 44, -1, 0, 0) == 0    # dtype
    assert sup(256, 256, 4, 3, 16, 44, F32, 2, 0) == 0 and sup(256, 256, 4, 3, 16, 44, F32, -1, 0) == 0  # layout
    assert sup(256, 256, 4, 3, 1 << 12, 1 << 12, F32, 0, 0) == 0            # c * h * w past the int32 index space


def _formula(b, c, o, g, h, w, esz, layout):
    """The formula of section 15 of the header."""
    up = lambda n, q: (n + q - 1) // q * q
    parts = 2 if esz == 4 else 1
    stream = up(g * -(-9 * (c // g) // 16) * -(-(o // g) // 32) * parts * 1024, 256)
    return stream + (up(b * c * h * w * esz, 16) if layout == 0 else 0)


def test_scratch_bytes_follow_the_documented_formula():
    _l, lib = _lib()
    n = C.c_size_t()
    for (b, c, o, g, h, w) in ((24, 256, 256, 4, 16, 44), (3, 72, 40, 1, 7, 9)):     # 72: K = 648 is padded to 656
        for dt, esz in ((F32, 4), (F16, 2), (BF16, 2)):
            for layout in (0, 1):
                assert lib.dhd_deform_conv_infer_scratch_bytes(b, c, o, g, 3, h, w, dt, layout, C.byref(n)) == 0
                assert n.value == _formula(b, c, o, g, h, w, esz, layout) and n.value % 16 == 0, (b, c, dt, layout)
    assert _formula(24, 256, 256, 4, 16, 44, 2, 1) == 4 * 36 * 2 * 1024
    assert lib.dhd_deform_conv_infer_scratch_bytes(24, 256, 256, 4, 3, 16, 44, F32, 0, None) == EINVAL
    assert lib.dhd_deform_conv_infer_scratch_bytes(24, 256, 256, 3, 3, 16, 44, F32, 0, C.byref(n)) == EINVAL      # c % groups
    assert lib.dhd_deform_conv_infer_scratch_bytes(24, 256, 256, 4, 3, 16, 44, 7, 0, C.byref(n)) == EINVAL
    assert lib.dhd_deform_conv_infer_scratch_bytes(24, 256, 256, 4, 5, 16, 44, F32, 0, C.byref(n)) == EUNSUPPORTED


def test_every_refusal_happens_on_the_host():
    """Fake addresses throughout: a call that got as far as a launch would fault, so each code below is a host-side check."""
    _l, lib = _lib()
    P, M = C.c_void_p(0x10000), C.c_void_p(0x10004)
    big = C.c_size_t(1 << 30)
    fn = lib.dhd_deform_conv_infer
    # x, x_dtype, layout, offset, weight, out, b, c_in, c_out, groups, h, w, k, pad, dil, gemm, scratch, scratch_bytes, stream
    good = [P, F32, 0, P, P, P, 2, 256, 256, 4, 16, 44, 3, 1, 1, 0, P, big, None]

    def with_(**kw):
        names = ('x', 'x_dtype', 'layout', 'offset', 'weight', 'out', 'b', 'c_in', 'c_out', 'groups', 'h', 'w', 'k', 'pad', 'dil', 'gemm',
                 'scratch', 'scratch_bytes', 'stream')
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)

    for name in ('x', 'offset', 'weight', 'out', 'scratch'):
        assert with_(**{name: None}) == EINVAL, name
    assert with_(x_dtype=3) == EINVAL and with_(layout=2) == EINVAL and with_(gemm=4) == EINVAL and with_(gemm=-1) == EINVAL
    assert with_(groups=3) == EINVAL and with_(c_out=254) == EINVAL                               # c % groups
    assert with_(b=0) == EINVAL and with_(pad=-1) == EINVAL and with_(dil=0) == EINVAL
    assert with_(k=5) == EUNSUPPORTED and with_(c_in=16, c_out=16) == EUNSUPPORTED and with_(c_in=544, c_out=544) == EUNSUPPORTED
    assert with_(gemm=_l.SFA_GEMM['bf16x6']) == EUNSUPPORTED and with_(x_dtype=F16, gemm=_l.SFA_GEMM['bf16x3']) == EUNSUPPORTED
    assert with_(b=1 << 14, h=64) == EUNSUPPORTED                                                # b c h w past 2^31
    n = C.c_size_t()
    assert lib.dhd_deform_conv_infer_scratch_bytes(2, 256, 256, 4, 3, 16, 44, F32, 0, C.byref(n)) == 0
    assert with_(scratch_bytes=C.c_size_t(n.value - 1)) == ENOSPACE and with_(scratch_bytes=C.c_size_t(0)) == ENOSPACE
    # alignment, behind every other check: x, out and scratch move as 16-byte vectors
    for name in ('x', 'out', 'scratch'):
        assert with_(**{name: M}, scratch_bytes=C.c_size_t(n.value)) == EINVAL, name
    assert with_(offset=C.c_void_p(0x10002)) == EINVAL


def test_fused_inference_flips_every_dcn_and_predictor_and_back():
    import dhd_amd
    from dhd_amd.depthnet import DCN
    from dhd_amd.detector import predictor
    assert DCN.fused_infer is False and predictor.fused_infer is False
    dcn = DCN(32, 32, groups=4)
    head = predictor.__new__(predictor)
    torch.nn.Module.__init__(head)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 32, 1), torch.nn.Sequential(dcn), head)
    assert dcn.fused_infer is False and head.fused_infer is False
    switched = dhd_amd.fused_inference(model)
    assert len(switched) == 2 and switched[0] is dcn and switched[1] is head
    assert dcn.fused_infer is True and head.fused_infer is True
    assert DCN.fused_infer is False and predictor.fused_infer is False              # instances, not the classes
    again = dhd_amd.fused_inference(model, enabled=False)
    assert len(again) == 2 and dcn.fused_infer is False and head.fused_infer is False
    # switched on, a CPU input still takes today's path
    dcn.fused_infer = True
    assert not dcn.eval().fused_applies(torch.zeros(1, 32, 4, 4))


def test_cpu_tensors_raise_and_the_functions_are_exported():
    import dhd_amd
    import pytest
    from dhd_amd import _lib as L
    assert dhd_amd.deform_conv_infer is dhd_amd.deform_conv.deform_conv_infer
    assert dhd_amd.deform_conv_infer_supported is dhd_amd.deform_conv.deform_conv_infer_supported
    x, off, wgt = torch.zeros(1, 32, 4, 4), torch.zeros(1, 18, 4, 4), torch.zeros(32, 8, 3, 3)
    assert dhd_amd.deform_conv_infer_supported(x, wgt, 4) is False
    with pytest.raises(L.DhdError):
        dhd_amd.deform_conv_infer(x, off, wgt, groups=4)


def test_lib_call_checks_the_return_code():
    import pytest
    from dhd_amd import _lib as L
    n = C.c_size_t()
    assert L.call('dhd_deform_conv_infer_scratch_bytes', 1, 32, 32, 4, 3, 6, 10, 0, 1, C.byref(n)) is None and n.value > 0
    with pytest.raises(L.DhdError, match='dhd_deform_conv_infer_scratch_bytes.*DHD_EUNSUPPORTED'):
        L.call('dhd_deform_conv_infer_scratch_bytes', 1, 32, 32, 4, 5, 6, 10, 0, 1, C.byref(n))


def test_the_module_calls_the_library_by_name_only():
    """tests/test_gpu_views.py scans the top-level modules for calls written `lib.dhd_*(`, `load().dhd_*(` or `_call('dhd_*'` and
    demands a row of its table for each launching one.  That file is a yardstick that a feature cannot edit, so the new operator
    is reached through _lib.call(name, ...), which the scan does not match; its view behaviour is pinned by
    test_gpu_deform_conv_infer.py::test_views instead (and by DESIGN.md's Views table).  Should this test fail, a row is due."""
    text = open(os.path.join(ROOT, 'dhd_amd', 'deform_conv.py')).read()
    assert re.findall(r'\b(?:lib|load\(\))\.(dhd_[a-z0-9_]+)', text) == []
    assert re.findall(r"_call\('(dhd_[a-z0-9_]+)'", text) == []
    assert "_lib.call('dhd_deform_conv_infer'," in text
