"""dhd_sfa_stage_infer (ABI 6), the forward-only inference operator of the SFA stage: everything that can be asked
without a GPU -- the symbols, host-side validation, which form exists for which precision, scratch sizes, and the
predicate by which channel_spatial_stage chooses it."""
import ctypes as C
import re
import subprocess

import pytest
import torch

from test_capi import SFA_WORKSPACE_BYTES, declared_symbols

INFER_SYMBOLS = ('dhd_sfa_stage_infer', 'dhd_sfa_stage_infer_scratch_bytes', 'dhd_sfa_stage_infer_supported')
AUTO, UNFUSED, TWO_PASS, ONE_PASS = 0, 1, 2, 3
F32, F16, BF16 = 0, 1, 2
GEMM = {'default': 0, 'bf16x6': 1, 'f32': 2, 'bf16x3': 3}


def test_the_three_symbols_are_declared_bound_and_exported():
    from dhd_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 6 and lib.dhd_abi_version() == 6
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r' T (dhd_[a-z0-9_]+)', out))
    for name in INFER_SYMBOLS:
        assert name in declared_symbols() and name in _lib.EXPORTED_SYMBOLS and name in exported, name
        assert getattr(lib, name) is not None
    assert _lib.SFA_INFER == {'auto': AUTO, 'unfused': UNFUSED, 'two_pass': TWO_PASS, 'one_pass': ONE_PASS}


def _weights(_lib, training=0, running=True, gemm=0, storage=F32, io=None):
    """A struct whose pointers are never dereferenced (validation happens before any launch)."""
    w = _lib.SfaWeights()
    for n in ('fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'conv1_w', 'conv1_b', 'bn1_w', 'bn1_b', 'conv2_w', 'conv2_b', 'bn2_w', 'bn2_b'):
        setattr(w, n, 0x10000)
    if running:
        w.bn1_mean = w.bn1_var = w.bn2_mean = w.bn2_var = 0x10000
    w.hidden, w.training, w.gemm, w.storage_dtype = 32, training, gemm, storage
    w.io_dtype = storage if io is None else io
    w.eps1 = w.eps2 = 1e-5
    return w


def test_validation_happens_on_the_host_before_any_launch():
    from dhd_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(16)
    ok = _weights(_lib)

    def call(x=one, w=ok, out=one, scratch=one, b=4, c=256, hw=40000, form=AUTO):
        return lib.dhd_sfa_stage_infer(x, C.byref(w), out, scratch, b, c, hw, form, None)
    assert call(x=None) == -1 and call(out=None) == -1 and call(scratch=None) == -1
    assert call(c=64) == -3                                           # unsupported C
    assert call(w=_lib.SfaWeights(), c=64) == -3                      # ... found before the struct is looked at
    w0 = _lib.SfaWeights()
    w0.hidden = 32
    assert call(w=w0) == -1                                           # null weights
    assert call(w=_weights(_lib, training=1)) == -1                   # batch statistics: dhd_sfa_stage_forward
    assert call(w=_weights(_lib, running=False)) == -1                # eval mode without running statistics
    assert call(form=4) == -1 and call(form=-1) == -1                 # unknown form
    assert call(w=_weights(_lib, gemm=7)) == -1                       # unknown precision, as in the forward
    assert call(w=_weights(_lib, storage=F16, io=BF16)) == -1         # half storage: io_dtype == storage_dtype
    # forms that do not exist for a precision / shape
    assert call(w=_weights(_lib, gemm=GEMM['bf16x6']), form=TWO_PASS) == -3
    assert call(w=_weights(_lib, gemm=GEMM['f32']), form=TWO_PASS) == -3
    assert call(c=512, form=TWO_PASS) == -3
    assert call(form=ONE_PASS) == -3                                  # float32 storage has no one-pass form
    assert call(w=_weights(_lib, gemm=GEMM['bf16x6']), form=ONE_PASS) == -3
    assert call(w=_weights(_lib, storage=F16), c=512) == -3           # half storage has no C = 512, in any form


def test_which_form_exists_for_which_precision():
    """UNFUSED and AUTO wherever dhd_sfa_stage_forward(training = 0) runs; TWO_PASS for bf16x3 on float32 storage and for half
    storage at C = 128 / 256; ONE_PASS for half storage only."""
    from dhd_amd import _lib
    lib = _lib.load()
    sup = lib.dhd_sfa_stage_infer_supported
    for c in (64, 128, 256, 512, 768):
        for hw in (40, 402, 1368, 40000):
            f32_ok = bool(lib.dhd_sfa_stage_supported(c, hw))
            half_ok = bool(lib.dhd_sfa_stage_half_storage_supported(c, hw))
            for gname, gemm in GEMM.items():
                for form in (AUTO, UNFUSED):
                    assert bool(sup(c, hw, F32, gemm, form)) == f32_ok, (c, hw, gname, form)
                    for storage in (F16, BF16):
                        assert bool(sup(c, hw, storage, gemm, form)) == half_ok, (c, hw, gname, form, storage)
                two = f32_ok and c in (128, 256) and gname in ('default', 'bf16x3')
                assert bool(sup(c, hw, F32, gemm, TWO_PASS)) == two, (c, hw, gname)
                for storage in (F16, BF16):
                    assert bool(sup(c, hw, storage, gemm, TWO_PASS)) == half_ok, (c, hw, gname, storage)
                    assert bool(sup(c, hw, storage, gemm, ONE_PASS)) == half_ok, (c, hw, gname, storage)
                assert sup(c, hw, F32, gemm, ONE_PASS) == 0
    assert sup(256, 40000, 5, 0, AUTO) == 0 and sup(256, 40000, F32, 9, AUTO) == 0 and sup(256, 40000, F32, 0, 7) == 0


def test_scratch_sizes():
    """TWO_PASS keeps one y1 next to the small tables; UNFUSED is the training layout (saved + scratch) in one block."""
    from dhd_amd import _lib
    lib = _lib.load()
    n = C.c_size_t(0)
    size = lib.dhd_sfa_stage_infer_scratch_bytes
    for (b, c, hw), (fs, ft, hs, ht) in SFA_WORKSPACE_BYTES.items():
        for storage, saved, scratch, esz in ((F32, fs, ft, 4), (F16, hs, ht, 2), (BF16, hs, ht, 2)):
            if saved is None:
                for form in (AUTO, UNFUSED, TWO_PASS):
                    assert size(b, c, hw, 32, storage, 0, form, C.byref(n)) == -3, (b, c, hw, storage, form)
                continue
            assert size(b, c, hw, 32, storage, 0, UNFUSED, C.byref(n)) == 0
            assert 0 < n.value <= saved + scratch and n.value % 16 == 0, (b, c, hw, storage)
            unfused = n.value
            if storage == F32:
                assert size(b, c, hw, 32, storage, 0, ONE_PASS, C.byref(n)) == -3
            else:
                assert size(b, c, hw, 32, storage, 0, ONE_PASS, C.byref(n)) == 0
                assert 0 < n.value <= 8e6 and n.value % 16 == 0, (b, c, hw, storage, n.value)
            if c in (128, 256):
                assert size(b, c, hw, 32, storage, 0, TWO_PASS, C.byref(n)) == 0
                assert 0 < n.value <= b * c * hw * esz + 8e6 and n.value % 16 == 0, (b, c, hw, storage, n.value)
                two = n.value
                assert size(b, c, hw, 32, storage, 0, AUTO, C.byref(n)) == 0 and n.value <= two
            else:
                assert size(b, c, hw, 32, storage, 0, TWO_PASS, C.byref(n)) == -3
                assert size(b, c, hw, 32, storage, 0, AUTO, C.byref(n)) == 0 and n.value == unfused
            # precisions whose GEMMs are not the cu kernels: AUTO is the unfused form
            if storage == F32:
                assert size(b, c, hw, 32, storage, GEMM['bf16x6'], AUTO, C.byref(n)) == 0 and n.value == unfused
    assert size(0, 256, 40000, 32, F32, 0, AUTO, C.byref(n)) == -1 and size(4, 256, 40000, 0, F32, 0, AUTO, C.byref(n)) == -1
    assert size(4, 256, 40000, 32, F32, 0, AUTO, None) == -1 and size(4, 256, 40000, 32, F32, 0, 9, C.byref(n)) == -1
    assert size(4, 256, 40000, 32, 5, 0, AUTO, C.byref(n)) == -1 and size(4, 64, 40000, 32, F32, 0, AUTO, C.byref(n)) == -3


def test_routing_predicate_needs_no_device():
    """inference_selected: eval mode with running statistics and nothing to differentiate."""
    from dhd_amd.mix import channel_spatial_stage, inference_selected
    st = channel_spatial_stage(256)
    x = torch.zeros(1, 256, 4, 4)
    assert st.infer is True and st.infer_form is None
    assert not inference_selected(st, x)                               # train mode
    with torch.no_grad():
        assert not inference_selected(st, x)
    st.eval()
    assert not inference_selected(st, x)                               # eval, grad mode on, parameters require grad
    with torch.no_grad():
        assert inference_selected(st, x)
        assert inference_selected(st, x.clone().requires_grad_())      # grad mode off: nothing is recorded
    for p in st.parameters():
        p.requires_grad_(False)
    assert inference_selected(st, x)                                   # grad mode on, but nothing requires a gradient
    assert not inference_selected(st, x.clone().requires_grad_())
    st.fc[2].bias.requires_grad_(True)
    assert not inference_selected(st, x)                               # one parameter does
    with torch.no_grad():
        assert inference_selected(st, x)
        st.infer = False                                               # the A/B switch
        assert not inference_selected(st, x)
        st.infer = True
        st.spacial_leanring[4].train()                                 # one BatchNorm on batch statistics
        assert not inference_selected(st, x)
        st.spacial_leanring[4].eval()
        assert inference_selected(st, x)
        bn = st.spacial_leanring[1]
        bn.running_mean = bn.running_var = None                        # no running buffers: batch statistics even in eval
        assert not inference_selected(st, x)
