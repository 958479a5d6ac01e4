"""dhd_window_attn_backward* without a GPU: the ABI surface, the support table, the host-side refusals (fake addresses, no device
touched), the float64 gradients the GPU tests compare against pinned to autograd through WindowMSA.forward, and the Python
switches of the training route."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('dhd_window_attn_backward_supported', 'dhd_window_attn_backward_scratch_bytes', 'dhd_window_attn_backward')
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
    assert all(re.search(r'\b(?:int|size_t)\s+%s\s*\(' % n, header) for n in NAMES)
    assert lib.dhd_abi_version() == 6 == _l.ABI_VERSION and '#define DHD_ABI_VERSION 6' in header
    mk = open(os.path.join(ROOT, 'dhd_amd', 'csrc', 'Makefile')).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith('SRCS')).split()
    assert 'window_attn_bwd.hip' in srcs and 'window_attn.hip' in srcs


def test_support_table_equals_the_forwards():
    """On the grid of arguments of test_window_attn_infer_capi.test_support_table."""
    _l, lib = _lib()
    fwd, bwd = lib.dhd_window_attn_infer_supported, lib.dhd_window_attn_backward_supported
    G = _l.SFA_GEMM
    nh_max = ((1 << 31) - 1) // (144 * 96)
    grid = [(wh, ww, nh, 32, dt, 0) for dt in (F32, F16, BF16)
            for wh, ww in ((12, 12), (7, 7), (4, 4), (3, 5), (1, 1), (1, 144), (144, 1), (9, 16)) for nh in (1, 3, 4, 8, 16, 32)]
    grid += [(12, 12, 4, 32, F32, G['bf16x3'])]
    grid += [(12, 12, 4, hd, F16, 0) for hd in (8, 16, 31, 33, 64, 0, -32)]
    grid += [(13, 13, 4, 32, F16, 0), (12, 13, 4, 32, F16, 0), (1, 145, 4, 32, F16, 0), (0, 12, 4, 32, F16, 0), (12, -1, 4, 32, F16, 0),
             (12, 12, 0, 32, F16, 0), (1 << 16, 1 << 16, 4, 32, F16, 0), (12, 12, 4, 32, 3, 0), (12, 12, 4, 32, -1, 0),
             (12, 12, 4, 32, F32, G['bf16x6']), (12, 12, 4, 32, F32, G['f32']), (12, 12, 4, 32, F32, 4), (12, 12, 4, 32, F32, -1)]
    grid += [(12, 12, 4, 32, dt, G[g]) for dt in (F16, BF16) for g in ('bf16x3', 'bf16x6', 'f32')]
    grid += [(12, 12, nh_max, 32, F16, 0), (12, 12, nh_max + 1, 32, F16, 0)]
    got = [bwd(*a) for a in grid]
    assert got == [fwd(*a) for a in grid]
    assert set(got) == {0, 1} and bwd(12, 12, 4, 32, F16, 0) == 1 and bwd(13, 13, 4, 32, F16, 0) == 0 and bwd(12, 12, 4, 16, F16, 0) == 0


def test_scratch_bytes_is_positive_and_monotone_in_windows():
    _l, lib = _lib()
    fn = lib.dhd_window_attn_backward_scratch_bytes
    for wh, ww, nh in ((12, 12, 4), (7, 7, 3), (3, 5, 2), (12, 12, 32)):
        sizes = [fn(w, wh, ww, nh) for w in (1, 2, 3, 7, 96, 288, 511, 512, 513, 1080, 3960, 100000)]
        assert all(s > 0 and s % 4 == 0 for s in sizes), sizes
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1], sizes
        assert sizes[0] >= (2 * wh - 1) * (2 * ww - 1) * nh * 4            # at least one partial row per head


def test_every_refusal_happens_on_the_host():
    """Fake addresses throughout: a call that got as far as a launch would fault, so each code below is a host-side check."""
    _l, lib = _lib()
    P, M = C.c_void_p(0x10000), C.c_void_p(0x10004)
    fn = lib.dhd_window_attn_backward
    names = ('qkv', 'dout', 'dtype', 'table', 'regions', 'dqkv', 'dtable', 'scratch', 'scratch_bytes', 'windows', 'nw', 'wh', 'ww', 'nh',
             'head_dim', 'scale', 'gemm', 'stream')
    need = lib.dhd_window_attn_backward_scratch_bytes(12, 12, 12, 4)
    good = [P, P, F16, P, P, P, P, P, need, 12, 6, 12, 12, 4, 32, 32 ** -0.5, 0, None]

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)

    for name in ('qkv', 'dout', 'table', 'dqkv', 'dtable', 'scratch'):
        assert with_(**{name: None}) == EINVAL, name
    for name in ('windows', 'nw', 'wh', 'ww', 'nh', 'head_dim'):
        assert with_(**{name: 0}) == EINVAL and with_(**{name: -1}) == EINVAL, name
    assert with_(windows=13) == EINVAL and with_(nw=5) == EINVAL                       # windows % nw
    assert with_(dtype=3) == EINVAL and with_(dtype=-1) == EINVAL and with_(gemm=4) == EINVAL and with_(gemm=-1) == EINVAL
    for name in ('qkv', 'dout', 'dqkv'):                                               # 16-byte vectors
        assert with_(**{name: M}) == EINVAL and with_(**{name: C.c_void_p(0x10008)}) == EINVAL, name
    for name in ('table', 'dtable', 'scratch'):                                        # 4-byte elements
        assert with_(**{name: C.c_void_p(0x10002)}) == EINVAL and with_(**{name: C.c_void_p(0x10001)}) == EINVAL, name
    assert with_(head_dim=16) == EUNSUPPORTED and with_(head_dim=64) == EUNSUPPORTED
    assert with_(wh=13, ww=13) == EUNSUPPORTED and with_(wh=12, ww=13) == EUNSUPPORTED and with_(wh=1, ww=145) == EUNSUPPORTED   # N = 145
    assert with_(gemm=_l.SFA_GEMM['bf16x3']) == EUNSUPPORTED                         # half dtypes take the default only
    assert with_(dtype=F32, gemm=_l.SFA_GEMM['bf16x6']) == EUNSUPPORTED and with_(dtype=F32, gemm=_l.SFA_GEMM['f32']) == EUNSUPPORTED
    w_max = ((1 << 31) - 1) // (144 * 384)                                           # windows * N * 3 * nh * 32 < 2^31
    w_max -= w_max % 6
    huge = 1 << 40
    assert with_(windows=w_max + 6, scratch_bytes=huge) == EUNSUPPORTED and with_(windows=1 << 30, nw=1, scratch_bytes=huge) == EUNSUPPORTED
    assert with_(nh=(1 << 31) // (144 * 96) + 1, scratch_bytes=huge) == EUNSUPPORTED
    assert with_(scratch_bytes=need - 1) == ENOSPACE and with_(scratch_bytes=0) == ENOSPACE
    assert with_(windows=18, scratch_bytes=need) == ENOSPACE                        # sized for 12 windows


@pytest.mark.parametrize('case', ['ws7_21x14_shift3_nh3', 'win3x5_nonsquare_nh2'])
def test_the_reference_gradients_are_autograd_through_the_module(case):
    """G of window_attn_train_inputs.py against torch's float64 autograd through WindowMSA.forward (today's SDPA path, on the CPU,
    float64 module and inputs): qkv enters through a forward hook on the qkv Linear, proj is the identity, to 1e-9 relative."""
    import window_attn_train_inputs as T
    from dhd_amd.swin import WindowMSA
    wh, ww, n, b, nw, nh = T.geometry(case)
    qkv, table, regions = T.inputs(case)
    m = WindowMSA(32 * nh, nh, (wh, ww)).double().train()
    assert m.scale == T.SCALE and m.fused_train is False
    with torch.no_grad():
        m.relative_position_bias_table.copy_(table.double())
    m.proj = torch.nn.Identity()
    leaf = T.stored_qkv(case, 'f32_bf16x3').double().requires_grad_()
    m.qkv.register_forward_hook(lambda mod, args, out: leaf)
    mask = None
    if regions is not None:
        r = regions.long()
        mask = torch.where(r.unsqueeze(1) != r.unsqueeze(2), -100.0, 0.0).double()       # [w, i, j], as shift_window_mask
    out = m(torch.zeros(b, nw, n, 32 * nh, dtype=torch.float64), mask)
    (out * T.stored_dout(case, 'f32_bf16x3').double()).sum().backward()
    G = T.gradients(case, 'f32_bf16x3')
    for name, got, ref in (('dqkv', leaf.grad, G[0]), ('dtable', m.relative_position_bias_table.grad, G[1])):
        err = float((got - ref).abs().max()) / T.scale_of(ref)
        assert got.shape == ref.shape and err <= 1e-9, (name, err)
    assert float(G[1].abs().max()) > 1.0 and float(G[0].abs().max()) > 0.5           # neither is trivially small


def test_half_bounds_have_the_size_of_one_rounding():
    """The bounds of the GPU tests of dhd_amd.window_attn are neither vacuous nor loose; dout is seeded and stable."""
    import window_attn_train_inputs as T
    from dhd_amd.window_attn import window_attn_supported
    assert window_attn_supported(T.stored_qkv('ws7_21x14_shift3_nh3', 'bf16'), (7, 7), 3) is False      # a CPU tensor
    case = 'ws7_21x14_shift3_nh3'
    assert T.bound_dqkv(case, 'f32_bf16x3') == 1e-4 == T.bound_dtable(case, 'bf16')
    assert 2e-4 < T.bound_dqkv(case, 'fp16') < 2e-2 and 2e-3 < T.bound_dqkv(case, 'bf16') < 1e-1
    d = T.stored_dout(case, 'bf16')
    assert d.dtype == torch.bfloat16 and tuple(d.shape) == tuple(T.stored_qkv(case, 'bf16').shape[:-1]) + (96,)
    assert torch.equal(T.stored_dout(case, 'bf16'), d)


def _small_swin():
    from dhd_amd.swin import SwinTransformer
    return SwinTransformer(embed_dims=32, patch_size=4, window_size=4, depths=(2, 2), num_heads=(1, 2), strides=(4, 2),
                           out_indices=(0, 1), drop_path_rate=0., with_cp=False)


def test_fused_training_flips_exactly_the_window_msa_modules():
    import dhd_amd
    from dhd_amd.swin import WindowMSA
    assert 'DHD_WINDOW_ATTN_TRAIN' not in os.environ and WindowMSA.fused_train is False     # off without the environment variable
    net = _small_swin()
    mods = [m for m in net.modules() if isinstance(m, WindowMSA)]
    before = {id(m): dict(m.__dict__) for m in net.modules()}
    switched = dhd_amd.fused_training(net)
    assert len(switched) == 4 and all(a is b for a, b in zip(switched, mods)) and all(m.fused_train is True for m in mods)
    assert WindowMSA.fused_train is False and all(m.fused_infer is False for m in mods)
    for m in net.modules():                                                                 # nothing else changed anywhere
        now = dict(m.__dict__)
        if isinstance(m, WindowMSA):
            assert now.pop('fused_train') is True
        assert now.keys() == before[id(m)].keys() and all(now[k] is before[id(m)][k] for k in now)
    again = dhd_amd.fused_training(net, on=False)
    assert len(again) == 4 and all(m.fused_train is False for m in mods)
    assert 'WindowMSA' in dhd_amd.fused_training.__doc__


def test_the_environment_variable_sets_the_class_default():
    import subprocess
    import sys
    code = 'from dhd_amd.swin import WindowMSA; print(WindowMSA.fused_train, WindowMSA.fused_infer)'
    env = dict(os.environ, DHD_WINDOW_ATTN_TRAIN='1', PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True)
    assert out.stdout.split() == ['True', 'False'], out.stderr[-500:]


def test_on_cpu_tensors_the_flag_changes_nothing(monkeypatch):
    import dhd_amd
    from dhd_amd import window_attn
    net = _small_swin().train()
    x = torch.randn(1, 3, 24, 40, generator=torch.Generator().manual_seed(1))

    def grads():
        net.zero_grad()
        outs = net(x)
        sum(o.square().sum() for o in outs).backward()
        return [o.detach() for o in outs] + [p.grad.clone() for p in net.parameters() if p.grad is not None]
    today = grads()
    with torch.no_grad():
        today_no_grad = net(x)
    dhd_amd.fused_training(net)

    def boom(*a, **k):
        raise AssertionError('the fused operator was reached on a CPU input')
    monkeypatch.setattr(window_attn, 'window_attn', boom)
    monkeypatch.setattr(window_attn, 'window_attn_infer', boom)
    got = grads()
    assert len(got) == len(today) and all(torch.equal(a, b) for a, b in zip(got, today))
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(net(x), today_no_grad))


def test_cpu_tensors_raise_and_the_function_is_exported():
    import dhd_amd
    from dhd_amd import _lib as L
    assert callable(dhd_amd.window_attn) and dhd_amd.window_attn.window_attn is not None
    assert dhd_amd.window_attn_supported is dhd_amd.window_attn.window_attn_supported
    qkv, table = torch.zeros(1, 1, 16, 96, requires_grad=True), torch.zeros(49, 1)
    assert dhd_amd.window_attn_supported(qkv, (4, 4), 1) is False
    with pytest.raises(L.DhdError):
        dhd_amd.window_attn(qkv, table, (4, 4), 1, 32 ** -0.5)
    text = open(os.path.join(ROOT, 'dhd_amd', 'window_attn.py')).read()
    assert "@traced('dhd.swin.attn.train')" in text and "_lib.call('dhd_window_attn_backward'," in text
    assert re.findall(r'\b(?:lib|load\(\))\.(dhd_[a-z0-9_]+)', text) == []
