"""C-ABI surface checks that need no GPU: the library loads, exports every symbol the header
declares, validates arguments before touching the device, and the package fails loudly
(instead of falling back) when the library or the GPU is missing."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'dhd_amd.h')


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(?:int|size_t)\s+(dhd_[a-z0-9_]+)\s*\(', src)))


def test_header_and_binding_table_agree():
    from dhd_amd import _lib
    assert declared_symbols() == sorted(_lib.EXPORTED_SYMBOLS)


def test_library_loads_and_exports_every_declared_symbol():
    from dhd_amd import _lib
    lib = _lib.load()
    assert os.path.samefile(_lib.LIB_PATH, os.path.join(ROOT, 'dhd_amd', 'csrc', 'libdhd_amd.so'))
    for name in declared_symbols():
        assert getattr(lib, name) is not None, name
    assert lib.dhd_abi_version() == _lib.ABI_VERSION
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r' T (dhd_[a-z0-9_]+)', out))
    assert exported == set(declared_symbols()), exported ^ set(declared_symbols())


def test_sfa_stage_shape_support_and_validation():
    """dhd_sfa_stage_*: supported channel counts, sizes, and argument checks that run before any launch."""
    from dhd_amd import _lib
    lib = _lib.load()
    assert lib.dhd_sfa_stage_supported(256, 40000) == 1 and lib.dhd_sfa_stage_supported(128, 400) == 1
    assert lib.dhd_sfa_stage_supported(512, 40000) == 1
    assert lib.dhd_sfa_stage_supported(64, 40000) == 0 and lib.dhd_sfa_stage_supported(256, 402) == 0
    # a sample is addressed through 32-bit buffer offsets: 2*C*hw*4 bytes must stay below 4 GiB
    assert lib.dhd_sfa_stage_supported(512, 1 << 21) == 0 and lib.dhd_sfa_stage_supported(512, (1 << 20) - 4) == 1
    assert lib.dhd_sfa_stage_saved_bytes(4, 64, 40000, 8) == 0
    saved = lib.dhd_sfa_stage_saved_bytes(4, 256, 40000, 32)
    # y1 + y2 (2 x 164 MB) + one pass bit per activation (5 MB) + small tables
    assert 2 * 4 * 256 * 40000 * 4 < saved < 2 * 4 * 256 * 40000 * 4 + 8e6
    assert lib.dhd_sfa_stage_scratch_bytes(4, 256, 40000, 32) > 3 * 4 * 256 * 40000 * 4
    w, g = _lib.SfaWeights(), _lib.SfaGrads()
    one = C.c_void_p(16)
    assert lib.dhd_sfa_stage_forward(None, C.byref(w), one, one, one, 4, 256, 40000, None) == -1
    assert lib.dhd_sfa_stage_forward(one, C.byref(w), one, one, one, 4, 64, 40000, None) == -3   # unsupported C
    w.hidden = 32
    assert lib.dhd_sfa_stage_forward(one, C.byref(w), one, one, one, 4, 256, 40000, None) == -1  # null weights
    assert lib.dhd_sfa_stage_backward(one, C.byref(w), one, one, one, C.byref(g), one, 4, 256, 40000, None) == -1
    # the GEMM precision is a per-call field (dhd_sfa_weights.gemm), not a process-wide switch
    assert not hasattr(lib, 'dhd_sfa_set_gemm_mode') and not hasattr(lib, 'dhd_mghs_set_deterministic')
    assert _lib.SFA_GEMM == {'default': 0, 'bf16x6': 1, 'f32': 2, 'bf16x3': 3}


# (b, C, hw) -> saved / scratch bytes of float32 storage, then of half storage (fp16 and bf16 alike; None: unsupported), as the
# library returned them before its host side was rewritten.  hw = 40 and 1368 are not multiples of 32 or 64.  hidden = 32.
SFA_WORKSPACE_BYTES = {
    (1, 128, 40): (318976, 17185536, 101888, 18987776),
    (1, 128, 1368): (1699840, 19267328, 803328, 20007680),
    (1, 128, 40000): (41876992, 79842048, 21200384, 49677056),
    (4, 128, 40): (459008, 17623552, 180480, 19130880),
    (4, 128, 1368): (5982464, 25950720, 2986240, 23210496),
    (4, 128, 40000): (166691072, 268249600, 84574464, 141888000),
    (9, 128, 40): (692736, 18353920, 311808, 20418304),
    (9, 128, 1368): (13120512, 37090048, 6624768, 29597440),
    (9, 128, 40000): (374714880, 582262528, 190198272, 296621824),
    (1, 256, 40): (1161216, 68449536, 333824, 71660800),
    (1, 256, 1368): (3922944, 72613120, 1736704, 73700608),
    (1, 256, 40000): (84277248, 193762560, 42530816, 133039360),
    (4, 256, 40): (1441024, 69325312, 490752, 71946752),
    (4, 256, 1368): (12487936, 85979648, 6102272, 80105984),
    (4, 256, 40000): (333905152, 570577408, 169278720, 317460992),
    (9, 256, 40): (1907712, 70785280, 752640, 74520832),
    (9, 256, 1368): (26763264, 108257536, 13378560, 92879104),
    (9, 256, 40000): (749952000, 1198602496, 380525568, 626927872),
    (1, 512, 40): (4418560, 273213696, None, None),
    (1, 512, 1368): (9942016, 281540864, None, None),
    (1, 512, 40000): (170650624, 523839744, None, None),
    (4, 512, 40): (4977920, 274964992, None, None),
    (4, 512, 1368): (27071744, 308273664, None, None),
    (4, 512, 40000): (669906176, 1277469184, None, None),
    (9, 512, 40): (5910528, 277884160, None, None),
    (9, 512, 1368): (55621632, 352828672, None, None),
    (9, 512, 40000): (1501999104, 2533518592, None, None),
    (1, 768, 40): (9773056, 614292736, None, None),
    (1, 768, 1368): (18058240, 626783488, None, None),
    (1, 768, 40000): (259121152, 990231808, None, None),
    (4, 768, 40): (10611968, 616919552, None, None),
    (4, 768, 1368): (43752704, 666882560, None, None),
    (4, 768, 40000): (1008004352, 2120675840, None, None),
    (9, 768, 40): (12010496, 621297920, None, None),
    (9, 768, 1368): (86577152, 733714688, None, None),
    (9, 768, 40000): (2256143360, 4004749568, None, None),
}


def test_sfa_stage_workspace_bytes_are_pinned():
    """dhd_sfa_stage_workspace_bytes / _saved_bytes / _scratch_bytes: captured graphs and caches are sized from them, so a layout
    change must be deliberate."""
    from dhd_amd import _lib
    lib = _lib.load()
    s, t = C.c_size_t(0), C.c_size_t(0)
    for (b, c, hw), (fs, ft, hs, ht) in SFA_WORKSPACE_BYTES.items():
        assert lib.dhd_sfa_stage_workspace_bytes(b, c, hw, 32, 0, C.byref(s), C.byref(t)) == 0
        assert (s.value, t.value) == (fs, ft), (b, c, hw)
        assert (lib.dhd_sfa_stage_saved_bytes(b, c, hw, 32), lib.dhd_sfa_stage_scratch_bytes(b, c, hw, 32)) == (fs, ft), (b, c, hw)
        for storage in (1, 2):   # DHD_F16, DHD_BF16
            rc = lib.dhd_sfa_stage_workspace_bytes(b, c, hw, 32, storage, C.byref(s), C.byref(t))
            if hs is None:
                assert rc == -3, (b, c, hw, storage)
            else:
                assert rc == 0 and (s.value, t.value) == (hs, ht), (b, c, hw, storage)
        assert lib.dhd_sfa_stage_workspace_bytes(b, c, hw, 32, 5, C.byref(s), C.byref(t)) == -1


def test_library_is_a_gfx950_code_object():
    from dhd_amd import _lib
    blob = open(_lib.LIB_PATH, 'rb').read()
    assert b'gfx950' in blob and b'gfx90a' not in blob and b'sm_' not in blob


def test_argument_validation_happens_on_the_host():
    from dhd_amd import _lib
    lib = _lib.load()
    n, m = C.c_size_t(0), C.c_size_t(0)
    d = _lib.MghsDesc()
    assert lib.dhd_mghs_workspace_bytes(C.byref(d), C.byref(n), C.byref(m)) == -1  # all-zero desc
    d.batch, d.n_cams, d.n_depth, d.fh, d.fw, d.channels, d.n_grids = 1, 6, 44, 16, 44, 64, 4
    for g, nz in zip(range(4), (1, 4, 4, 8)):
        d.grid[g].n[0], d.grid[g].n[1], d.grid[g].n[2] = 200, 200, nz
    assert lib.dhd_mghs_workspace_bytes(C.byref(d), C.byref(n), C.byref(m)) == 0
    state, scratch = n.value, m.value
    # state (what backward needs, held by autograd): slot prefix (V words) + slot -> voxel (2P) + per-point slots (2P) = 5.7 MB
    assert 5.0e6 < state < 6.5e6
    # scratch (shared per stream): counters / keys / sorted lists (~2V + 10P words = 13 MB) + the compact table sized for the
    # most slots the index rules allow: min(V0, P) + min(V1 + V2 + V3, P) = 40 000 + 185 856 rows x 256 B = 58 MB
    assert 6.5e7 < scratch < 8.0e7
    d.batch = 4
    assert lib.dhd_mghs_workspace_bytes(C.byref(d), C.byref(n), C.byref(m)) == 0
    assert 3.9 * state < n.value < 4.1 * state and 3.9 * scratch < m.value < 4.1 * scratch
    d.n_grids = 5
    assert lib.dhd_mghs_workspace_bytes(C.byref(d), C.byref(n), C.byref(m)) == -1
    d.n_grids = 4
    d.flags = 8                                                                     # unknown flag bit (1, 2, 4 are defined)
    assert lib.dhd_mghs_workspace_bytes(C.byref(d), C.byref(n), C.byref(m)) == -1
    d.flags = _lib.MGHS_DETERMINISTIC | _lib.MGHS_FEAT_GRAD_NCHW
    assert lib.dhd_mghs_workspace_bytes(C.byref(d), C.byref(n), C.byref(m)) == 0
    assert lib.dhd_mghs_prepare(C.byref(d), None, None, None, None) == -1
    assert lib.dhd_mghs_lift(C.byref(d), None, None, 65, None, None, None, None, None, None, None) == -1
    assert lib.dhd_hbm_calibrate(None, 1024, 0, None) == -1 and lib.dhd_hbm_calibrate(C.c_void_p(4096), 1000, 1, None) == -1
    assert lib.dhd_bev_pool_v2_forward(None, None, None, None, None, None, None, None, 64, 10, None) == -1
    assert lib.dhd_bev_pool_v2_forward(None, None, None, None, None, None, None, None, 64, 0, None) == 0  # nothing to do
    # fused operator: sizes on the host, shapes it does not take, missing workspace
    fs, fc = C.c_size_t(), C.c_size_t()
    assert lib.dhd_bev_pool_v2_fused_workspace_bytes(64, 4, 1, 200, 200, 81205, C.byref(fs), C.byref(fc)) == 0
    assert fs.value >= 4 * (160001 + 81206) and fs.value % 256 == 0 and fc.value >= 4 * (2 * 160000 + 64 * 81206)
    assert lib.dhd_bev_pool_v2_fused_workspace_bytes(80, 4, 1, 200, 200, 10, C.byref(fs), C.byref(fc)) == -1      # C != 64
    assert lib.dhd_bev_pool_v2_fused_workspace_bytes(64, 4, 1, 202, 200, 10, C.byref(fs), C.byref(fc)) == -3     # Dy % 4
    assert lib.dhd_bev_pool_v2_fused_workspace_bytes(64, 4, 1, 200, 260, 10, C.byref(fs), C.byref(fc)) == -3     # Dx > 256
    assert lib.dhd_bev_pool_v2_fused_workspace_bytes(64, 4, 1, 200, 200, 10, None, None) == -1
    assert lib.dhd_bev_pool_v2_fused_forward(*([None] * 8), 64, 10, 4, 1, 200, 200, None, 0, 0, None, 0, None) == -1
    assert lib.dhd_bev_pool_v2_fused_backward(*([None] * 10), 64, 10, 10, 4, 1, 200, 200, None, 0, None, 0, None) == -1
    assert lib.dhd_sfa_channel_mean(None, None, 1, 512, 40000, None) == -1
    assert lib.dhd_height_band(None, 6, 65, 16, 44, None, None, None, None) == -1
    assert lib.dhd_ema_update(None, None, None, 5, 0.5, 0.5, None) == -1
    assert lib.dhd_bn_supported(1, 24, 64, 128 * 352) == 1 and lib.dhd_bn_supported(1, 4, 64, 2500) == 0 and lib.dhd_bn_supported(0, 4, 64, 2500) == 1
    assert lib.dhd_bn_supported(0, 70000, 1, 64) == 0 and lib.dhd_bn_workspace_bytes(24, 64, 45056) == (24 * 16 * 2 * 64 + 3 * 64) * 4
    assert lib.dhd_bn_train_forward(None, 0, 2, 8, 64, None, None, None, None, 0.1, 1e-5, None, None, None, None, None) == -1
    assert lib.dhd_ema_update(None, None, None, 0, 0.5, 0.5, None) == 0  # empty state
    d.batch = 1 << 20
    assert lib.dhd_mghs_workspace_bytes(C.byref(d), C.byref(n), C.byref(m)) == -3  # beyond the int32 index space
    # a dtype code outside DHD_F32 / DHD_F16 / DHD_BF16 is refused by every entry point that takes one, before any launch (all other
    # arguments valid, pointers never dereferenced).  The return codes are those of the library before the dtype dispatch moved
    # into csrc/vec16.h.  Left out because the earlier library reaches a launch with them: dhd_mghs_forward_views (gathers before it
    # looks at the views; dhd_mghs_forward_stream_views is the same check without the gather) and dhd_mghs_softmax_backward with
    # g_xd == NULL (xd_dtype is not read then).
    P = C.c_void_p(0x10000)
    d1 = _lib.MghsDesc()
    d1.batch, d1.n_cams, d1.n_depth, d1.fh, d1.fw, d1.channels, d1.n_grids = 1, 1, 4, 4, 11, 64, 1
    d1.grid[0].n[0], d1.grid[0].n[1], d1.grid[0].n[2] = 8, 8, 1
    assert lib.dhd_mghs_workspace_bytes(C.byref(d1), C.byref(n), C.byref(m)) == 0
    ws = _lib.MghsWorkspace(0x10000, n.value, 0x4000000, m.value)
    views = (_lib.TensorView * _lib.DHD_MAX_GRIDS)()
    views[0].ptr, views[0].batch_stride, views[0].z_stride, views[0].channel_stride = 0x8000000, 64 * 64, 64 * 64, 64
    for bad in (3, -1):
        assert lib.dhd_bn_train_forward(P, bad, 2, 8, 64, None, None, None, None, 0.1, 1e-5, P, P, P, P, None) == -3
        assert lib.dhd_bn_train_backward(P, P, bad, 2, 8, 64, None, P, P, P, None, None, P, None) == -3
        assert lib.dhd_bn_nhwc_train_forward(P, None, bad, 128, 8, 0, None, None, None, None, 0.1, 1e-5, P, P, P, P, P, None) == -3
        assert lib.dhd_bn_nhwc_train_backward(P, None, P, bad, 128, 8, 0, None, P, P, None, P, None, None, None, P, None) == -3
        assert lib.dhd_upsample_bilinear_forward(P, bad, 0, 1, 8, 4, 4, 8, 8, P, None) == -3
        assert lib.dhd_upsample_bilinear_backward(P, bad, 1, 1, 8, 4, 4, 8, 8, P, None) == -3
        assert lib.dhd_window_rows(P, P, bad, 0, 1, 7, 7, 8, 7, 0, 0, None) == -3                       # input code
        assert lib.dhd_window_rows(P, P, 0, bad, 1, 7, 7, 8, 7, 0, 1, None) == -3                       # output code
        assert lib.dhd_deform_im2col_t(P, 0, P, P, bad, 1, 4, 5, 5, 3, 1, 1, None) == -1                # column code
        assert lib.dhd_deform_im2col_t(P, bad, P, P, 0, 1, 4, 5, 5, 3, 1, 1, None) == -1                # image code
        assert lib.dhd_deform_col2im_t(P, bad, P, 0, P, P, P, 1, 4, 5, 5, 3, 1, 1, P, 1 << 20, None) == -3
        assert lib.dhd_deform_col2im_t(P, 0, P, bad, P, P, P, 1, 4, 5, 5, 3, 1, 1, P, 1 << 20, None) == -1
        assert lib.dhd_mghs_softmax_forward(P, bad, 0, 12, None, 0, 0, 0, 2, 44, 4, 8, 0, None, None, P, P, None, None, None) == -1
        assert lib.dhd_mghs_softmax_forward(P, 0, 0, 12, P, bad, 0, 8, 2, 44, 4, 8, 8, None, None, P, P, P, None, None) == -1
        assert lib.dhd_mghs_softmax_backward(None, None, None, None, None, 2, 44, 4, 8, 0, P, bad, 0, 12, None, 0, 0, 0, None) == -1
        assert lib.dhd_mghs_softmax_backward(None, None, None, None, None, 2, 44, 4, 8, 8, P, 0, 0, 12, P, bad, 0, 8, None) == -1
        views[0].dtype = bad
        assert lib.dhd_mghs_forward_stream_views(C.byref(d1), P, P, C.byref(views), C.byref(ws), None) == -1
        assert lib.dhd_mghs_backward_views(C.byref(d1), P, P, C.byref(views), P, P, C.byref(ws), None) == -1
    # a mixed pair the deform kernels are not built for (half image, other half columns), and a half view on the generic MGHS path
    assert lib.dhd_deform_im2col_t(P, 1, P, P, 2, 1, 4, 5, 5, 3, 1, 1, None) == -1
    d1.channels, views[0].dtype = 32, 1
    assert lib.dhd_mghs_workspace_bytes(C.byref(d1), C.byref(n), C.byref(m)) == 0
    ws = _lib.MghsWorkspace(0x10000, n.value, 0x4000000, m.value)
    assert lib.dhd_mghs_backward_views(C.byref(d1), P, P, C.byref(views), P, P, C.byref(ws), None) == -3


def test_no_silent_fallback_without_gpu_or_library():
    from dhd_amd import _lib, bev_pool_v2, SFA
    from dhd_amd import mghs_op
    z = torch.zeros(0, dtype=torch.int32)
    with pytest.raises(_lib.DhdError):
        bev_pool_v2(torch.rand(1, 1, 2, 2, 2), torch.rand(1, 1, 2, 2, 4), z, z, z, (1, 1, 3, 3, 4), z, z)
    with pytest.raises(_lib.DhdError):
        SFA(32, 16)(torch.rand(1, 32, 5, 5))
    with pytest.raises(_lib.DhdError):
        mghs_op.height_band(torch.rand(2, 65, 4, 11), [0.1 * i for i in range(65)], [0, 1, 2, 3])
    from dhd_amd import label_loss, occ_loss
    from dhd_amd.depthnet import _DeformIm2col
    with pytest.raises(_lib.DhdError):
        occ_loss.occ_losses(torch.rand(10, 18), torch.zeros(10, dtype=torch.uint8), torch.ones(10, dtype=torch.uint8), torch.ones(18))
    with pytest.raises(_lib.DhdError):
        occ_loss.occ_argmax_hist(torch.rand(10, 18))
    with pytest.raises(_lib.DhdError):
        label_loss.bin_labels(torch.rand(1, 2, 32, 32), torch.rand(1, 2, 32, 32), 16, [1.0, 45.0, 1.0], 44, -1.0, 0.1, 65)
    with pytest.raises(_lib.DhdError):
        label_loss.points_to_maps(torch.rand(2, 100, 4), 64, 176)
    with pytest.raises(_lib.DhdError):
        _DeformIm2col.apply(torch.rand(1, 4, 5, 5), torch.zeros(1, 18, 5, 5), 3, 1, 1)
    code = ("import os, sys; sys.path.insert(0, %r); os.environ['DHD_AMD_LIB'] = '/nonexistent/libdhd_amd.so'\n"
            "from dhd_amd import _lib\n"
            "try:\n    _lib.load()\nexcept _lib.DhdError as e:\n    print('LOUD', e)\n" % ROOT)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert 'LOUD' in out.stdout and 'no CPU or PyTorch fallback' in out.stdout


def test_product_code_never_imports_the_oracle():
    for base, _, files in os.walk(os.path.join(ROOT, 'dhd_amd')):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                text = open(os.path.join(base, f)).read()
                assert 'oracle' not in text.replace('oracle-free', ''), os.path.join(base, f)


def test_workspace_alignment_is_checked_on_the_host():
    """The MGHS kernels access the carved workspace arrays as 16-byte vectors: a misaligned base is refused."""
    from dhd_amd import _lib
    lib = _lib.load()
    d = _lib.MghsDesc()
    d.batch, d.n_cams, d.n_depth, d.fh, d.fw, d.channels, d.n_grids = 1, 1, 4, 4, 11, 64, 1
    d.grid[0].n[0], d.grid[0].n[1], d.grid[0].n[2] = 8, 8, 1
    n, m = C.c_size_t(0), C.c_size_t(0)
    assert lib.dhd_mghs_workspace_bytes(C.byref(d), C.byref(n), C.byref(m)) == 0 and n.value > 0 and m.value > 0
    cal = _lib.Calib()
    for f, _ in _lib.Calib._fields_:
        setattr(cal, f, 0x20000)
    for state, scratch, rc in ((0x10004, 0x40000, -1), (0x10000, 0x40004, -1)):
        ws = _lib.MghsWorkspace(state, n.value, scratch, m.value)
        assert lib.dhd_mghs_prepare(C.byref(d), C.byref(cal), None, C.byref(ws), None) == rc
    ws = _lib.MghsWorkspace(0x10000, n.value - 1, 0x40000, m.value)       # too small
    assert lib.dhd_mghs_prepare(C.byref(d), C.byref(cal), None, C.byref(ws), None) == -2


def test_tensor_alignment_is_checked_on_the_host():
    """Every entry point whose kernels move a caller's tensor as 16-byte vectors (csrc/vec16.h; 4-byte pairs in layout.hip) refuses a
    misaligned pointer with DHD_EINVAL before any launch: fake addresses, no device touched.  Each call is otherwise valid, and
    where a later host check exists the same call with the aligned address reaches it (-3), so the -1 is the alignment test's."""
    from dhd_amd import _lib
    lib = _lib.load()
    P, M = C.c_void_p(0x10000), C.c_void_p(0x10004)     # 16-byte aligned / 4 bytes off
    H = C.c_void_p(0x10002)                             # 2 bytes off: a one-element offset of a half tensor

    def each(fn, args, slots, later=None):
        """fn(*args) with the pointer at each of `slots` replaced by a misaligned one -> -1; `later`: (slot, value, code) of a
        host check behind the alignment test that the aligned call reaches."""
        for s in slots:
            for bad in (M, H):
                a = list(args)
                a[s] = bad
                assert fn(*a) == -1, (fn.__name__, s, bad.value)
        if later is not None:
            a = list(args)
            a[later[0]] = later[1]
            assert fn(*a) == later[2], fn.__name__
            a[slots[0]] = M
            assert fn(*a) == -1, fn.__name__

    # SFA stage: x, out, saved, scratch / gout, gx (the parameters are read element by element)
    w, g = _lib.SfaWeights(), _lib.SfaGrads()
    for f, _ in _lib.SfaWeights._fields_[:16]:
        setattr(w, f, 0x20000)
    for f, _ in _lib.SfaGrads._fields_:
        setattr(g, f, 0x20000)
    w.hidden = 16
    S = C.c_void_p(0x30000)   # sync_sums
    each(lib.dhd_sfa_stage_forward, [P, C.byref(w), P, P, P, 2, 128, 64, None], (0, 2, 3, 4), later=(6, 64, -3))
    each(lib.dhd_sfa_stage_backward, [P, C.byref(w), P, P, P, C.byref(g), P, 2, 128, 64, None], (0, 2, 3, 4, 6), later=(8, 64, -3))
    each(lib.dhd_sfa_stage_forward_phase, [P, C.byref(w), P, P, P, 2, 128, 64, 2, S, None], (0, 2, 3, 4), later=(6, 64, -3))
    each(lib.dhd_sfa_stage_backward_phase, [P, C.byref(w), P, P, P, C.byref(g), P, 2, 128, 64, 2, S, None], (0, 2, 3, 4, 6), later=(8, 64, -3))
    each(lib.dhd_sfa_stage_infer, [P, C.byref(w), P, P, 2, 128, 64, 0, None], (0, 2, 3), later=(5, 64, -3))
    # BatchNorm, NCHW and channels_last: x, y, grad_y, grad_x, residual, grad_residual
    each(lib.dhd_bn_train_forward, [P, 0, 2, 8, 64, None, None, None, None, 0.1, 1e-5, P, P, P, P, None], (0, 11), later=(1, 3, -3))
    each(lib.dhd_bn_train_backward, [P, P, 0, 2, 8, 64, None, P, P, P, None, None, P, None], (0, 1, 9), later=(2, 3, -3))
    each(lib.dhd_bn_nhwc_train_forward, [P, P, 0, 128, 8, 2, None, None, None, None, 0.1, 1e-5, P, P, P, P, P, None], (0, 1, 12),
         later=(2, 3, -3))
    each(lib.dhd_bn_nhwc_train_backward, [P, P, P, 0, 128, 8, 2, None, P, P, P, P, P, None, None, P, None], (0, 1, 2, 11, 12),
         later=(3, 3, -3))
    # bilinear up-sampling: channels_last rows are vectors; the NCHW kernels are scalar and take any element-aligned address
    each(lib.dhd_upsample_bilinear_forward, [P, 0, 1, 1, 8, 4, 4, 8, 8, P, None], (0, 9), later=(1, 3, -3))
    each(lib.dhd_upsample_bilinear_backward, [P, 0, 1, 1, 8, 4, 4, 8, 8, P, None], (0, 9), later=(1, 3, -3))
    assert lib.dhd_upsample_bilinear_forward(M, 0, 0, 1, 8, 4, 4, 2, 8, M, None) == -3     # NCHW float32 at 4 bytes off: passes on to the
    assert lib.dhd_upsample_bilinear_forward(H, 1, 0, 1, 8, 4, 4, 2, 8, H, None) == -3     # shape check (down-sampling); half at 2 bytes too
    assert lib.dhd_upsample_bilinear_forward(H, 0, 0, 1, 8, 4, 4, 8, 8, P, None) == -1     # float32 at 2 bytes off
    # window partition / reverse
    each(lib.dhd_window_rows, [P, P, 0, 2, 1, 7, 7, 8, 7, 0, 0, None], (0, 1), later=(7, 12, -3))
    # layout: 4-byte elements and the 2-byte pair kernel (even rows and cols) need 4-byte alignment; the scalar 2-byte kernel does not
    for eb, rows, cols, bad in ((4, 7, 9, H), (2, 8, 10, H)):
        assert lib.dhd_transpose_batched(bad, P, eb, 0, rows, cols, None) == -1 and lib.dhd_transpose_batched(P, bad, eb, 0, rows, cols, None) == -1
        assert lib.dhd_transpose_batched(P, P, eb, 0, rows, cols, None) == -3              # (batch 0: the check behind it)
    assert lib.dhd_transpose_batched(H, H, 2, 0, 7, 10, None) == -3                        # odd rows: element accesses only
    # stereo cost volume: 16-byte channel groups of prev / curr, one float2 per sampling position
    each(lib.dhd_stereo_cost_volume, [P, P, P, 2, 16, 6, 10, 8, 5.0, 12, P, None], (0, 1), later=(4, 18, -3))
    assert lib.dhd_stereo_cost_volume(P, P, M, 2, 16, 6, 10, 8, 5.0, 12, P, None) == -1
    # MGHS on the compact path (C = 64): a context row and the pooled tensors move as 16-byte vectors
    d = _lib.MghsDesc()
    d.batch, d.n_cams, d.n_depth, d.fh, d.fw, d.channels, d.n_grids = 1, 1, 4, 4, 11, 64, 1
    d.grid[0].n[0], d.grid[0].n[1], d.grid[0].n[2] = 8, 8, 1
    n, m = C.c_size_t(0), C.c_size_t(0)
    assert lib.dhd_mghs_workspace_bytes(C.byref(d), C.byref(n), C.byref(m)) == 0
    ws = _lib.MghsWorkspace(0x100000, n.value, 0x4000000, m.value)
    good, bad = (C.c_void_p * _lib.DHD_MAX_GRIDS)(0x8000000), (C.c_void_p * _lib.DHD_MAX_GRIDS)(0x8000004)
    assert lib.dhd_mghs_forward_gather(C.byref(d), P, M, C.byref(ws), None) == -1
    assert lib.dhd_mghs_forward(C.byref(d), P, M, C.byref(good), C.byref(ws), None) == -1
    assert lib.dhd_mghs_forward_stream(C.byref(d), P, M, C.byref(good), C.byref(ws), None) == -1
    assert lib.dhd_mghs_forward_stream(C.byref(d), P, P, C.byref(bad), C.byref(ws), None) == -1
    assert lib.dhd_mghs_backward(C.byref(d), P, M, C.byref(good), P, P, C.byref(ws), None) == -1
    assert lib.dhd_mghs_backward(C.byref(d), P, P, C.byref(good), P, M, C.byref(ws), None) == -1
    assert lib.dhd_mghs_backward(C.byref(d), P, P, C.byref(bad), P, P, C.byref(ws), None) == -1


def _build_c_example(tmp_path):
    """examples/capi_kat.c with plain gcc (C11): the header is C, the only other dependency is the HIP runtime's host API."""
    exe = str(tmp_path / 'capi_kat')
    lib_dir = os.path.join(ROOT, 'dhd_amd', 'csrc')
    cmd = ['gcc', '-std=c11', '-O2', '-Wall', '-Werror', '-D__HIP_PLATFORM_AMD__', os.path.join(ROOT, 'examples', 'capi_kat.c'),
           '-I' + os.path.join(ROOT, 'include'), '-I/opt/rocm/include', '-L' + lib_dir, '-ldhd_amd', '-L/opt/rocm/lib', '-lamdhip64', '-lm',
           '-Wl,-rpath,' + lib_dir, '-Wl,-rpath,/opt/rocm/lib', '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return exe


def test_header_is_plain_c_and_the_c_example_links(tmp_path):
    """include/dhd_amd.h compiles as strict C99 (no C++ or torch types anywhere in the ABI) and a C host program written
    against it links to libdhd_amd.so with gcc alone -- the form a binding in the reference's own extension style would
    take."""
    src = tmp_path / 'h.c'
    src.write_text('#include "dhd_amd.h"\nint main(void) { return dhd_abi_version() == DHD_ABI_VERSION ? 0 : 1; }\n')
    out = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + os.path.join(ROOT, 'include'), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    _build_c_example(tmp_path)


@pytest.mark.gpu
def test_c_example_reproduces_the_reference_known_answer_test(gpu, tmp_path):
    """The reference's in-file KAT (ops/bev_pool_v2/bev_pool.py:163-194) from a plain C program: hipMalloc'd buffers, its own
    stream, forward + device regrouping + backward through the C ABI, no Python and no torch in the process."""
    exe = _build_c_example(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'KAT ok' in out.stdout, (out.stdout + out.stderr)[-2000:]
