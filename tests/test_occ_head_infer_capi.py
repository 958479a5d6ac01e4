"""dhd_occ_head_infer, the fused occupancy head of inference (predicter MLP -> class map): everything that can be asked
without a GPU -- the symbols, which configurations exist, the scratch size, host-side validation, and the fall-back of
predictor.predict_occ on CPU tensors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import torch

from conftest import ROOT
from test_capi import declared_symbols

SYMBOLS = ('dhd_occ_head_infer', 'dhd_occ_head_infer_scratch_bytes', 'dhd_occ_head_infer_supported')
F32, F16, BF16 = 0, 1, 2
NCHW, NHWC = 0, 1
EINVAL, EUNSUPPORTED = -1, -3


def _weights(_lib, c=256, hidden=512, dz=16, n_classes=18, gemm=0, null=()):
    """A struct whose pointers are never dereferenced (validation happens before any launch)."""
    w = _lib.OccHeadWeights()
    for n in ('w1', 'b1', 'w2', 'b2'):
        setattr(w, n, None if n in null else 0x10000)
    w.c, w.hidden, w.dz, w.n_classes, w.gemm = c, hidden, dz, n_classes, gemm
    return w


def test_abi_stays_6_and_the_three_symbols_are_declared_bound_and_exported():
    from dhd_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 6 and lib.dhd_abi_version() == 6
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r' T (dhd_[a-z0-9_]+)', out))
    for name in SYMBOLS:
        assert name in declared_symbols() and name in _lib.EXPORTED_SYMBOLS and name in exported, name
        assert getattr(lib, name) is not None
    import dhd_amd
    assert dhd_amd.occ_head_infer is dhd_amd.occ_head.occ_head_infer


def test_supported_configurations():
    from dhd_amd import _lib
    sup = _lib.load().dhd_occ_head_infer_supported
    for dtype in (F32, F16, BF16):
        for layout in (NCHW, NHWC):
            assert sup(256, 512, 16, 18, dtype, layout, 0) == 1, (dtype, layout)
            assert sup(256, 512, 16, 17, dtype, layout, 0) == 0 and sup(256, 512, 16, 19, dtype, layout, 0) == 0
    assert sup(256, 512, 16, 18, F32, NCHW, _lib.SFA_GEMM['bf16x3']) == 1         # the default, by its own name
    assert sup(128, 512, 16, 18, F32, NCHW, 0) == 0 and sup(256, 256, 16, 18, F32, NCHW, 0) == 0 and sup(256, 512, 8, 18, F32, NCHW, 0) == 0
    assert sup(256, 512, 16, 18, 5, NCHW, 0) == 0 and sup(256, 512, 16, 18, F32, 2, 0) == 0 and sup(256, 512, 16, 18, F32, NCHW, 9) == 0


def test_scratch_bytes():
    from dhd_amd import _lib
    size = _lib.load().dhd_occ_head_infer_scratch_bytes
    n = C.c_size_t(0)
    for dtype in (F32, F16, BF16):
        assert size(C.byref(_weights(_lib)), dtype, C.byref(n)) == 0
        assert n.value > 0 and n.value % 16 == 0 and n.value <= 4 << 20, (dtype, n.value)   # weight images only: nothing per cell
    assert size(None, F32, C.byref(n)) == EINVAL and size(C.byref(_weights(_lib)), F32, None) == EINVAL
    assert size(C.byref(_weights(_lib)), 7, C.byref(n)) == EINVAL
    assert size(C.byref(_weights(_lib, n_classes=17)), F32, C.byref(n)) == EUNSUPPORTED


def test_argument_validation_happens_on_the_host():
    from dhd_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(0x10000)
    ok = _weights(_lib)

    def call(x=one, dtype=F32, layout=NCHW, w=ok, b=4, dy=200, dx=200, pred=one, logits=None, labels=None, mask=None, hist=None,
             scratch=one):
        return lib.dhd_occ_head_infer(x, dtype, layout, None if w is None else C.byref(w), b, dy, dx, pred, logits, labels, mask, hist,
                                      scratch, None)
    assert call(x=None) == EINVAL and call(w=None) == EINVAL and call(scratch=None) == EINVAL
    for n in ('w1', 'b1', 'w2', 'b2'):
        assert call(w=_weights(_lib, null=(n,))) == EINVAL, n
    assert call(b=0) == EINVAL and call(dy=0) == EINVAL and call(dx=-1) == EINVAL
    assert call(pred=None, logits=None) == EINVAL                                  # nothing to write
    assert call(hist=one) == EINVAL                                                # a histogram needs labels
    assert call(scratch=C.c_void_p(0x10008)) == EINVAL and call(x=C.c_void_p(0x10004)) == EINVAL   # 16-byte alignment
    assert call(dtype=3) == EINVAL
    assert call(w=_weights(_lib, n_classes=17)) == EUNSUPPORTED and call(w=_weights(_lib, c=128)) == EUNSUPPORTED
    assert call(w=_weights(_lib, gemm=_lib.SFA_GEMM['f32'])) == EUNSUPPORTED and call(layout=2) == EUNSUPPORTED
    assert call(dtype=F16, w=_weights(_lib, gemm=_lib.SFA_GEMM['bf16x3'])) == EUNSUPPORTED   # gemm names float32 arithmetic only


def test_predict_occ_on_cpu_tensors_falls_back_to_the_module_formulation():
    from occ_head_inputs import make_head, make_x
    head = make_head()
    x = make_x((2, 7, 9))
    labels = torch.randint(0, 19, (2, 9, 7, 16), generator=torch.Generator().manual_seed(5)).to(torch.uint8)
    labels[labels == 18] = 255
    mask = torch.rand(2, 9, 7, 16, generator=torch.Generator().manual_seed(6)) < 0.7
    try:
        for flag in (False, True):
            type(head).fused_infer = flag
            with torch.no_grad():
                assert not head.fused_applies(x)
                want = head.get_occ(head.forward(x))
                got = head.predict_occ(x)
                dev = head.predict_occ(x, to_host=False)
                occ, hist, lg = head.predict_occ(x, labels=labels, mask_camera=mask, return_logits=True)
                assert torch.equal(lg, head.forward(x))
            assert isinstance(got, list) and len(got) == 2 and got[0].dtype == np.uint8 and got[0].shape == (9, 7, 16)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)) and all(np.array_equal(a, b) for a, b in zip(occ, want))
            assert torch.is_tensor(dev) and dev.dtype == torch.uint8 and np.array_equal(dev.numpy(), np.stack(want))
            t, p = labels.reshape(-1).long(), torch.from_numpy(np.stack(want)).reshape(-1).long()
            keep = (t < 18) & mask.reshape(-1)
            assert torch.equal(hist, torch.bincount(t[keep] * 18 + p[keep], minlength=324).view(18, 18)) and hist.sum() > 500
    finally:
        type(head).fused_infer = False
    assert type(head).fused_infer is False                                         # the default stays the parent's path


def test_the_new_product_code_never_imports_the_oracle():
    for rel in ('dhd_amd/occ_head.py', 'dhd_amd/csrc/occ_head.hip', 'dhd_amd/detector.py', 'dhd_amd/__init__.py'):
        assert 'oracle' not in open(os.path.join(ROOT, rel)).read(), rel
