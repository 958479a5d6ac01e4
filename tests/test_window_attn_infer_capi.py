"""dhd_window_attn_infer* without a GPU: the ABI surface, the support table, the host-side refusals (fake addresses, no device
touched), the Python switches around it and the region ids the operator reads instead of the shift mask."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('dhd_window_attn_infer_supported', 'dhd_window_attn_infer')
EINVAL, EUNSUPPORTED = -1, -3
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
    mk = open(os.path.join(ROOT, 'dhd_amd', 'csrc', 'Makefile')).read()
    assert 'window_attn.hip' in next(ln for ln in mk.splitlines() if ln.startswith('SRCS'))


def test_support_table():
    _l, lib = _lib()
    sup = lib.dhd_window_attn_infer_supported
    G = _l.SFA_GEMM
    # wh, ww, nh, head_dim, dtype, gemm
    for dt in (F32, F16, BF16):
        for wh, ww in ((12, 12), (7, 7), (4, 4), (3, 5), (1, 1), (1, 144), (144, 1), (9, 16)):
            for nh in (1, 3, 4, 8, 16, 32):
                assert sup(wh, ww, nh, 32, dt, 0) == 1, (wh, ww, nh, dt)
    assert sup(12, 12, 4, 32, F32, G['bf16x3']) == 1
    for hd in (8, 16, 31, 33, 64, 0, -32):                                  # head dimension 32 only
        assert sup(12, 12, 4, hd, F16, 0) == 0, hd
    assert sup(13, 13, 4, 32, F16, 0) == 0 and sup(12, 13, 4, 32, F16, 0) == 0 and sup(1, 145, 4, 32, F16, 0) == 0    # N = 169, 156, 145
    assert sup(0, 12, 4, 32, F16, 0) == 0 and sup(12, -1, 4, 32, F16, 0) == 0 and sup(12, 12, 0, 32, F16, 0) == 0
    assert sup(1 << 16, 1 << 16, 4, 32, F16, 0) == 0                        # wh * ww wraps to 0 in 32 bits
    assert sup(12, 12, 4, 32, 3, 0) == 0 and sup(12, 12, 4, 32, -1, 0) == 0      # dtype
    assert sup(12, 12, 4, 32, F32, G['bf16x6']) == 0 and sup(12, 12, 4, 32, F32, G['f32']) == 0
    assert sup(12, 12, 4, 32, F32, 4) == 0 and sup(12, 12, 4, 32, F32, -1) == 0
    for dt in (F16, BF16):                                                  # gemm selects float32 arithmetic only
        for g in ('bf16x3', 'bf16x6', 'f32'):
            assert sup(12, 12, 4, 32, dt, G[g]) == 0
    # N * 3 * nh * 32 < 2^31 for one window: 144 * 96 * nh
    nh_max = ((1 << 31) - 1) // (144 * 96)
    assert sup(12, 12, nh_max, 32, F16, 0) == 1 and sup(12, 12, nh_max + 1, 32, F16, 0) == 0


def test_every_refusal_happens_on_the_host():
    """Fake addresses throughout: a call that got as far as a launch would fault, so each code below is a host-side check."""
    _l, lib = _lib()
    P, M = C.c_void_p(0x10000), C.c_void_p(0x10004)
    fn = lib.dhd_window_attn_infer
    names = ('qkv', 'dtype', 'table', 'regions', 'out', 'windows', 'nw', 'wh', 'ww', 'nh', 'head_dim', 'scale', 'gemm', 'stream')
    good = [P, F16, P, P, P, 12, 6, 12, 12, 4, 32, 32 ** -0.5, 0, None]

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)

    for name in ('qkv', 'table', 'out'):
        assert with_(**{name: None}) == EINVAL, name
    for name in ('windows', 'nw', 'wh', 'ww', 'nh', 'head_dim'):
        assert with_(**{name: 0}) == EINVAL and with_(**{name: -1}) == EINVAL, name
    assert with_(windows=13) == EINVAL and with_(nw=5) == EINVAL                       # windows % nw
    assert with_(dtype=3) == EINVAL and with_(dtype=-1) == EINVAL and with_(gemm=4) == EINVAL and with_(gemm=-1) == EINVAL
    assert with_(qkv=M) == EINVAL and with_(out=M) == EINVAL and with_(qkv=C.c_void_p(0x10008)) == EINVAL      # 16-byte vectors
    assert with_(table=C.c_void_p(0x10002)) == EINVAL and with_(table=C.c_void_p(0x10001)) == EINVAL              # 4-byte elements
    assert with_(head_dim=16) == EUNSUPPORTED and with_(head_dim=64) == EUNSUPPORTED
    assert with_(wh=13, ww=13) == EUNSUPPORTED and with_(wh=12, ww=13) == EUNSUPPORTED
    assert with_(gemm=_l.SFA_GEMM['bf16x3']) == EUNSUPPORTED                         # half dtypes take the default only
    assert with_(dtype=F32, gemm=_l.SFA_GEMM['bf16x6']) == EUNSUPPORTED and with_(dtype=F32, gemm=_l.SFA_GEMM['f32']) == EUNSUPPORTED
    # windows * N * 3 * nh * 32 < 2^31: 144 * 384 * windows at nh = 4
    w_max = ((1 << 31) - 1) // (144 * 384)
    w_max -= w_max % 6
    assert with_(windows=w_max + 6) == EUNSUPPORTED and with_(windows=1 << 30, nw=1) == EUNSUPPORTED
    assert with_(nh=(1 << 31) // (144 * 96) + 1) == EUNSUPPORTED


def _small_swin():
    from dhd_amd.swin import SwinTransformer
    return SwinTransformer(embed_dims=32, patch_size=4, window_size=4, depths=(2, 2), num_heads=(1, 2), strides=(4, 2),
                           out_indices=(0, 1), drop_path_rate=0., with_cp=False)


def test_fused_inference_flips_every_window_msa_and_back():
    import dhd_amd
    from dhd_amd.swin import WindowMSA
    assert WindowMSA.fused_infer is False
    net = _small_swin()
    mods = [m for m in net.modules() if isinstance(m, WindowMSA)]
    assert len(mods) == 4 and all(m.fused_infer is False for m in mods)
    switched = dhd_amd.fused_inference(net)
    assert len(switched) == 4 and all(a is b for a, b in zip(switched, mods)) and all(m.fused_infer is True for m in mods)
    assert WindowMSA.fused_infer is False and 'fused_infer' in mods[0].__dict__       # instances, not the class
    again = dhd_amd.fused_inference(net, enabled=False)
    assert len(again) == 4 and all(m.fused_infer is False for m in mods) and WindowMSA.fused_infer is False
    assert 'WindowMSA' in dhd_amd.fused_inference.__doc__


def test_a_cpu_input_keeps_todays_path(monkeypatch):
    import dhd_amd
    from dhd_amd import window_attn
    net = _small_swin().eval()
    x = torch.randn(1, 3, 24, 40, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        today = net(x)
    dhd_amd.fused_inference(net)

    def boom(*a, **k):
        raise AssertionError('the fused operator was reached on a CPU input')
    monkeypatch.setattr(window_attn, 'window_attn_infer', boom)
    msa = net.stages[0].blocks[1].attn.w_msa
    assert msa.fused_infer and not msa.fused_applies(torch.zeros(1, 2, 16, 32))
    with torch.no_grad():
        out = net(x)
    assert all(torch.equal(a, b) for a, b in zip(out, today))
    # forward(x, mask) keeps working for callers that pass only a mask
    win, mask = torch.randn(2, 3, 16, 32), torch.zeros(3, 16, 16)
    with torch.no_grad():
        assert torch.equal(msa(win, mask), msa(win, mask, regions=None)) and msa(win).shape == win.shape


def test_cpu_tensors_raise_and_the_functions_are_exported():
    import dhd_amd
    from dhd_amd import _lib as L
    assert dhd_amd.window_attn_infer is dhd_amd.window_attn.window_attn_infer
    assert dhd_amd.window_attn_infer_supported is dhd_amd.window_attn.window_attn_infer_supported
    qkv, table = torch.zeros(1, 1, 16, 96), torch.zeros(49, 1)
    assert dhd_amd.window_attn_infer_supported(qkv, (4, 4), 1) is False
    with pytest.raises(L.DhdError):
        dhd_amd.window_attn_infer(qkv, table, (4, 4), 1, 32 ** -0.5)
    text = open(os.path.join(ROOT, 'dhd_amd', 'window_attn.py')).read()
    assert "@traced('dhd.swin.attn.infer')" in text and "_lib.call('dhd_window_attn_infer'," in text
    assert re.findall(r'\b(?:lib|load\(\))\.(dhd_[a-z0-9_]+)', text) == []          # reached by name only, as deform_conv.py is


@pytest.mark.parametrize('geom', [(24, 36, 12, 6), (21, 14, 7, 3), (8, 8, 4, 2)])
def test_regions_reproduce_the_shift_mask(geom):
    from dhd_amd.swin import shift_window_mask, shift_window_regions
    H, W, ws, sh = geom
    mask = shift_window_mask(H, W, ws, sh, 'cpu')
    reg = shift_window_regions(H, W, ws, sh, 'cpu')
    nw = (H // ws) * (W // ws)
    assert reg.dtype == torch.uint8 and tuple(reg.shape) == (nw, ws * ws) and reg.is_contiguous() and int(reg.max()) == 8
    assert mask.dtype == torch.float32 and tuple(mask.shape) == (nw, ws * ws, ws * ws)
    r = reg.long()
    differ = r.unsqueeze(1) != r.unsqueeze(2)                  # [w, i, j]: regions of tokens j and i differ
    assert torch.equal(mask, torch.where(differ, torch.tensor(-100.0), torch.tensor(0.0)))
    assert bool(differ.any()) and bool((mask.diagonal(dim1=1, dim2=2) == 0).all())


def test_the_reference_and_bounds_of_the_gpu_tests():
    """window_attn_inputs.py against torch's own attention in float64 on one shifted case, and the size of its half bounds."""
    import torch.nn.functional as F
    import window_attn_inputs as I
    case = 'ws7_21x14_shift3_nh3'
    wh, ww, n, b, nw, nh = I.geometry(case)
    qkv, table, regions = I.inputs(case)
    q, k, v = qkv.double().view(b, nw, n, 3, nh, 32).permute(3, 0, 1, 4, 2, 5)
    add = torch.from_numpy(I.additive_term(case))
    out = F.scaled_dot_product_attention(q, k, v, attn_mask=add[None], scale=I.SCALE).transpose(2, 3).reshape(b, nw, n, nh * 32)
    assert float((out - I.reference(case, 'f32_bf16x3')).abs().max()) < 1e-12
    assert I.bound(case, 'f32_bf16x3') == 1e-4
    assert 2e-4 < I.bound(case, 'fp16') < 4e-3 and 2e-3 < I.bound(case, 'bf16') < 4e-2
