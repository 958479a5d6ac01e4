"""The UNet seam operators (dhd_amd/unet_seam.py, csrc/unet_seam.h) on the GPU: the pooling against torch bit for bit, the up seam
against the float64 twin of tests/unet_seam_inputs.py, both inside `_Down` / `_Up` / `UNet` and the G17 fixture, on views, under
graph capture and inside guard bands.  Routing is forced with monkeypatch.

Bounds.  Pooling: none, every byte is torch's.  Up seam, float32: the project's layer bar |y - Y64| <= 1e-4 max(1, |Y64|max) on
the output, gx1, gx2, dbias and dweight.  Up seam, half types: the error against the twin is at most 1.5 x the error torch's own
three calls make in the same dtype on the same tensors (the project's bar for a half path).  The x2 half of the output and gx2
are copies: bit-equal to their sources.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as G  # noqa: E402
import unet_seam_inputs as US  # noqa: E402
from conftest import golden  # noqa: E402
from test_gpu_views import Case  # noqa: E402

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
CL = torch.channels_last
pytestmark = pytest.mark.gpu


def _sync():
    """Wait for the device; after a device error nothing more is started in this module."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'GPU fault, stopping the module: {e}', returncode=3)


def _recorder(monkeypatch):
    """The names that reach dhd_amd._lib.check: every dhdn_* launch goes through it."""
    from dhd_amd import _lib, _unet_seam
    _unet_seam.load()
    seen, real = [], _lib.check

    def check(rc, what):
        seen.append(what)
        return real(rc, what)
    monkeypatch.setattr(_lib, 'check', check)
    return seen


class _Everything(dict):
    """A routing table that routes every entry."""

    def get(self, key, default=None):
        return True


def _route_all(monkeypatch):
    from dhd_amd import unet_seam
    monkeypatch.setattr(unet_seam, 'ROUTED', _Everything())


def _err(got, ref64):
    return float((got.detach().cpu().double() - ref64).abs().max())


# ------------------------------------------------------------------------------------------------ 1. pooling

def _pool_both(x, gy, fn):
    x = x.clone().requires_grad_()
    y = fn(x)
    y.backward(gy)
    _sync()
    return y.detach(), x.grad


@pytest.mark.parametrize('fmt', [torch.contiguous_format, CL], ids=['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype', [F32, F16, BF16], ids=['f32', 'f16', 'bf16'])
@pytest.mark.parametrize('shape', US.POOL_SHAPES, ids=str)
def test_pool_is_torchs_bit_for_bit(gpu, shape, dtype, fmt):
    import dhd_amd
    x, gy = (t.to(gpu).contiguous(memory_format=fmt) for t in US.pool_input(shape, dtype))
    y, gx = _pool_both(x, gy, dhd_amd.max_pool2x2)
    yt, gxt = _pool_both(x, gy, lambda t: F.max_pool2d(t, 2))
    assert y.dtype == dtype and y.shape == yt.shape and y.stride() == yt.stride() and gx.stride() == x.stride()
    assert torch.equal(US.bits(y), US.bits(yt)) and torch.equal(US.bits(gx), US.bits(gxt))
    B, C, H, W = shape
    assert int((y == 0).sum()) > 0 or H * W <= 4                                            # ties were there
    assert not bool(US.bits(gx[:, :, 2 * (H // 2):]).any()) and not bool(US.bits(gx[:, :, :, 2 * (W // 2):]).any())   # dropped: +0
    _, again = _pool_both(x, gy, dhd_amd.max_pool2x2)
    assert torch.equal(US.bits(again), US.bits(gx))


@pytest.mark.parametrize('fmt', [torch.contiguous_format, CL], ids=['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype', [F32, F16, BF16], ids=['f32', 'f16', 'bf16'])
def test_pool_edge_values_are_torchs_on_device_and_on_the_cpu(gpu, dtype, fmt):
    """NaN, two NaNs, +inf, all -inf, four-way ties, signed zeros.  The edge-value windows are held to torch on the CPU: values
    and gradient bit for bit (a NaN equals a NaN: torch's CPU kernel does not keep a bfloat16 NaN's payload).  Torch on the device
    is the same everywhere but in one place: its channels_last kernels hand the gradient of an all -inf window to NO element
    (measured here: 8 of 768 gradient elements, all three dtypes), where torch on the CPU and torch's NCHW device kernel hand it
    to element (0,0), which is the rule the operator states.  Those windows are left out of the device comparison, and only
    there and only in channels_last."""
    import dhd_amd
    xc, gc = (t.contiguous(memory_format=fmt) for t in US.pool_edge_input(dtype))
    x, gy = xc.to(gpu), gc.to(gpu)
    y, gx = _pool_both(x, gy, dhd_amd.max_pool2x2)
    xr = xc.clone().requires_grad_()
    yc = F.max_pool2d(xr, 2)
    yc.backward(gc)
    assert US.same_but_nan_payload(y.cpu(), yc.detach()) and US.same_but_nan_payload(gx.cpu(), xr.grad)
    yt, gxt = _pool_both(x, gy, lambda t: F.max_pool2d(t, 2))
    assert torch.equal(US.bits(y), US.bits(yt))
    differs = US.bits(gx) != US.bits(gxt)
    print(f'edge values [{dtype}, {fmt}]: gradient elements that differ from torch on the device: {int(differs.sum())} of {gx.numel()}')
    if fmt == CL:
        all_minus_inf = (F.max_pool2d(x.float(), 2) == float('-inf')).repeat_interleave(2, 2).repeat_interleave(2, 3)
        assert int(all_minus_inf.sum()) == 8 * 4 and not bool((differs & ~all_minus_inf).any())
    else:
        assert not bool(differs.any())
    assert int(torch.isnan(y).sum()) >= 40 and int((y == float('-inf')).sum()) == 8


def test_pool_unsupported_channels_take_todays_path(gpu, monkeypatch):
    import dhd_amd
    from dhd_amd import _lib
    from dhd_amd.detector import _Down
    _route_all(monkeypatch)
    x = torch.relu(torch.randn(2, 12, 6, 6, device=gpu)).contiguous(memory_format=CL)
    assert not dhd_amd.unet_seam_supported(x, 'pool') and dhd_amd.unet_seam_supported(x.contiguous(), 'pool')
    with pytest.raises(_lib.DhdError):
        dhd_amd.max_pool2x2(x)
    torch.manual_seed(1)
    m = _Down(12, 16).to(gpu).to(memory_format=CL)
    m.fused_seam = False
    ref = m(x)
    seen = _recorder(monkeypatch)
    m.fused_seam = True
    got = m(x)
    _sync()
    assert torch.equal(got, ref) and not any(w.startswith('dhdn') for w in seen)


# ------------------------------------------------------------------------------------------------ 2. the up seam

UP_GRID = [pytest.param(c, p, id=f'{c}-{p}') for c in US.UP_CASES for p in ('f32', 'f16', 'bf16')]


def _up_run(v, op, need_w=True, c=None):
    """Forward and backward of `op` on the tensors of v; c (test_gpu_views.Case) presents x1 or the gradient as a view."""
    c = c or Case(None, 'fresh')
    x1, x2 = c.inp('x1', v['x1'], grad=True), c.inp('x2', v['x2'], grad=True)
    w, b = v['weight'].clone().requires_grad_(need_w), v['bias'].clone().requires_grad_(need_w)
    out = op(x1, x2, w, b)
    c.grad('gout', out).backward(v['gout'])
    _sync()
    return dict(out=out.detach(), gx1=x1.grad, gx2=x2.grad, gweight=w.grad, gbias=b.grad)


def _torch_up(x1, x2, w, b):
    return US.up_reference(x1, x2, w, b.to(w.dtype))


@pytest.mark.parametrize('case,prec', UP_GRID)
def test_up_seam_against_the_float64_twin(gpu, case, prec):
    import dhd_amd
    v = {k: t.to(gpu) for k, t in US.up_inputs(case, prec).items()}
    got = _up_run(v, dhd_amd.conv_transpose2x2_cat)
    t = US.twin(case, prec)
    B, Cin, Cout, C2, h, w, H, W = US.UP_CASES[case]
    dt = US.DTYPES[prec]
    assert got['out'].shape == (B, C2 + Cout, H, W) and got['out'].dtype == dt and got['out'].is_contiguous(memory_format=CL)
    assert got['gx1'].shape == v['x1'].shape and got['gx1'].dtype == dt and got['gx2'].dtype == dt and got['gweight'].dtype == dt
    assert got['gweight'].shape == (Cin, Cout, 2, 2) and got['gbias'].shape == (Cout,) and got['gbias'].dtype == F32
    # the copies
    assert torch.equal(US.bits(got['out'][:, :C2]), US.bits(v['x2'])) and torch.equal(US.bits(got['gx2']), US.bits(v['gout'][:, :C2]))
    top, left = (H - 2 * h) // 2, (W - 2 * w) // 2
    border = torch.ones(H, W, dtype=torch.bool, device=gpu)
    border[top:top + 2 * h, left:left + 2 * w] = False
    assert not bool(US.bits(got['out'][:, C2:])[:, :, border].any())                                   # +0, no bias
    errs = {k: _err(got[k], t[k]) for k in ('out', 'gx1', 'gx2', 'gbias', 'gweight')}
    if prec == 'f32':
        print(f'{case} [f32]: ' + ', '.join(f'{k} {e:.2e} / {US.BAR * US.scale_of(t[k]):.2e}' for k, e in errs.items()))
        for k, e in errs.items():
            assert e <= US.BAR * US.scale_of(t[k]), (k, e)
    else:
        tv = dict(v, bias=v['bias'])
        ref = _up_run(tv, _torch_up)
        terr = {k: _err(ref[k], t[k]) for k in errs}
        print(f'{case} [{prec}]: ' + ', '.join(f'{k} {errs[k]:.2e} vs torch {terr[k]:.2e} (ratio {errs[k] / terr[k] if terr[k] else float(errs[k] > 0):.2f})'
                                              for k in errs))
        for k in errs:
            assert errs[k] <= 1.5 * terr[k], (k, errs[k], terr[k])
    again = _up_run(v, dhd_amd.conv_transpose2x2_cat)
    assert all(torch.equal(US.bits(again[k]), US.bits(got[k])) for k in got)


def test_a_frozen_layer_writes_no_operand(gpu, monkeypatch):
    import dhd_amd
    from dhd_amd import _unet_seam
    v = {k: t.to(gpu) for k, t in US.up_inputs('c64_4x4_pad11', 'bf16').items()}
    calls, real = [], _unet_seam.call
    monkeypatch.setattr(_unet_seam, 'call', lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    live = _up_run(v, dhd_amd.conv_transpose2x2_cat, need_w=True)
    frozen = _up_run(v, dhd_amd.conv_transpose2x2_cat, need_w=False)
    bwd = [a for n, a in calls if n == 'dhdn_up_cat_backward']
    assert len(bwd) == 2 and bwd[0][5].value and bwd[0][6].value                 # g_operand and dbias given ...
    assert not bwd[1][5].value and not bwd[1][6].value                           # ... and NULL with the layer frozen
    assert frozen['gweight'] is None and frozen['gbias'] is None
    assert torch.equal(frozen['gx1'], live['gx1']) and torch.equal(frozen['gx2'], live['gx2']) and torch.equal(frozen['out'], live['out'])


def test_up_seam_refuses_what_it_does_not_cover(gpu):
    import dhd_amd
    from dhd_amd import _lib
    v = {k: t.to(gpu) for k, t in US.up_inputs('c32_3x5', 'f32').items()}
    assert dhd_amd.unet_seam_supported(v['x1'], 'up', v['x2'], v['weight'])
    assert not dhd_amd.unet_seam_supported(v['x1'].contiguous(), 'up', v['x2'].contiguous(), v['weight'])          # NCHW maps
    assert not dhd_amd.unet_seam_supported(v['x1'], 'up', v['x2'].half(), v['weight'])                            # two dtypes
    assert not dhd_amd.unet_seam_supported(v['x1'], 'up', v['x2'][:, :, :5], v['weight'])                         # x2 smaller
    with pytest.raises(_lib.DhdError):
        dhd_amd.conv_transpose2x2_cat(v['x1'].contiguous(), v['x2'].contiguous(), v['weight'])


# ------------------------------------------------------------------------------------------------ 3. modules

def _module_run(m, inputs, autocast=None):
    m.zero_grad()
    xs = [t.clone().requires_grad_() for t in inputs]
    with torch.autocast('cuda', dtype=autocast, enabled=autocast is not None):
        y = m(*xs)
    gen = torch.Generator().manual_seed(9)
    y.float().backward(torch.randn(y.shape, generator=gen).to(y.device))
    _sync()
    return [y.detach().float()] + [x.grad.float() for x in xs] + [p.grad.float() for p in m.parameters()]


def _module_twin(m, inputs):
    import copy
    m64 = copy.deepcopy(m).cpu().double()
    m64.fused_seam = False
    for s in m64.modules():
        if hasattr(s, 'fused_seam'):
            s.fused_seam = False
    return [t.double() for t in _module_run(m64, [t.cpu().double().contiguous() for t in inputs])]


def _same_where_today_repeats(got, today, again):
    """got == today bit for bit on every tensor that today's path itself reproduces from run to run (MIOpen's convolutions need
    not: on this stack a UNet's forward differs in the last bits between two runs of the same module on the same input, and the
    weight gradients are added up with atomics); -> how many tensors were not comparable.  What the calls were is held by the
    recorder beside it."""
    stable = [torch.equal(a, b) for a, b in zip(today, again)]
    assert all(torch.equal(a, b) for a, b, ok in zip(got, today, stable) if ok)
    print(f'tensors today\'s path does not repeat: {len(stable) - sum(stable)} of {len(stable)}')
    return len(stable) - sum(stable)


def _switch(m, on):
    for s in m.modules():
        if hasattr(type(s), 'fused_seam'):
            s.fused_seam = on


def _modules(gpu):
    from dhd_amd.detector import UNet, _Down, _Up
    gen = torch.Generator().manual_seed(21)
    r = lambda *s: torch.randn(*s, generator=gen).to(gpu).contiguous(memory_format=CL)
    torch.manual_seed(5)
    return {'down': (_Down(32, 64), [r(2, 32, 11, 10)]),
            'up': (_Up(64, 32, False), [r(2, 64, 5, 4), r(2, 32, 11, 9)]),
            'unet': (UNet(32, 16), [r(2, 32, 40, 40)])}


@pytest.mark.parametrize('name', ['down', 'up', 'unet'])
def test_modules_against_the_float64_twin(gpu, monkeypatch, name):
    m, inputs = _modules(gpu)[name]
    m = m.to(gpu).to(memory_format=CL)
    twin = _module_twin(m, inputs)
    _switch(m, False)
    today = _module_run(m, inputs)
    _route_all(monkeypatch)
    seen = _recorder(monkeypatch)
    _switch(m, True)
    got = _module_run(m, inputs)
    n = {'down': (1, 1, 0, 0), 'up': (0, 0, 1, 1), 'unet': (4, 4, 4, 4)}[name]
    assert tuple(seen.count(k) for k in ('dhdn_max_pool2_forward', 'dhdn_max_pool2_backward', 'dhdn_up_cat_forward', 'dhdn_up_cat_backward')) == n
    rel = lambda a, t: float((a.cpu().double() - t).norm() / t.norm().clamp_min(1e-30))
    e_got = [_err(a, t) / US.scale_of(t) for a, t in zip(got, twin)]
    e_today = [_err(a, t) / US.scale_of(t) for a, t in zip(today, twin)]
    print(f'{name} [f32]: worst scaled error {max(e_got):.2e} (today {max(e_today):.2e}), output {e_got[0]:.2e}')
    assert e_got[0] <= US.BAR                                                   # the output: the layer bar
    # gradients pass ReLUs and pooling windows that a 1e-6 difference flips: held to the bar where today's path meets it too
    if name == 'unet':
        # ~20 ReLU / pooling layers and train-mode BatchNorm over 8 values at the deepest level: a last-bit difference in the
        # forward flips units, and each flip moves the back-propagated signal by that unit's whole contribution (the reasoning
        # of test_voxel_logits.check_gradients, whose bound this is): relative L2 below 3e-2, or 1.5 x today's where today's
        # path itself is further from the twin
        r_got, r_today = [rel(a, t) for a, t in zip(got, twin)], [rel(a, t) for a, t in zip(today, twin)]
        print(f'unet [f32]: worst relative L2 {max(r_got):.2e} (today {max(r_today):.2e})')
        assert all(a <= max(3e-2, 1.5 * b) for a, b in zip(r_got, r_today))
    else:
        for a, b in zip(e_got, e_today):
            assert a <= max(US.BAR, 1.5 * b)
    if name == 'down':                                                          # pooling alone: today's bits
        _switch(m, False)
        assert _same_where_today_repeats(got, today, _module_run(m, inputs)) <= 2 and torch.equal(got[0], today[0]) and torch.equal(got[1], today[1])
        _switch(m, True)
    for dt in (BF16, F16):
        # inside a UNet under autocast both operands of `_Up` arrive in the autocast dtype (they are outputs of convolutions)
        ins = [t.to(dt) for t in inputs] if name == 'up' else inputs
        _switch(m, False)
        today = _module_run(m, ins, dt)
        _switch(m, True)
        del seen[:]
        got = _module_run(m, ins, dt)
        assert tuple(seen.count(k) for k in ('dhdn_max_pool2_forward', 'dhdn_max_pool2_backward', 'dhdn_up_cat_forward', 'dhdn_up_cat_backward')) == n
        # a whole UNet's gradients pass unit flips (above): the largest single element of a gradient is decided by which units
        # flipped, so there the error is measured as the relative L2 distance to the twin; one seam: the largest element
        measure = rel if name == 'unet' else (lambda a, t: _err(a, t) / US.scale_of(t))
        e_got, e_today = [measure(a, t) for a, t in zip(got, twin)], [measure(a, t) for a, t in zip(today, twin)]
        print(f'{name} [{dt} autocast]: largest ratio {max(a / b for a, b in zip(e_got, e_today) if b):.2f}')
        print(f'{name} [{dt} autocast]: ratios of the error to today\'s ' + ' '.join(f'{a / b if b else 0:.2f}' for a, b in zip(e_got, e_today)))
        assert got[0].shape == today[0].shape and all(a <= 1.5 * b for a, b in zip(e_got, e_today))


def test_switch_off_unrouted_and_unsupported_are_todays_path(gpu, monkeypatch):
    """Switch off; switch on with the table empty; switch on, everything routed, but shapes the operators do not take (NCHW
    maps for the up seam, 12 channels in channels_last for the pool): today's calls, today's bits, no dhdn_* launch."""
    from dhd_amd import unet_seam
    from dhd_amd.detector import UNet
    torch.manual_seed(2)
    net = UNet(32, 16).to(gpu).to(memory_format=CL)
    x = torch.randn(2, 32, 32, 32, device=gpu).contiguous(memory_format=CL)
    _switch(net, False)
    _module_run(net, [x])                                                       # (the first call searches MIOpen's solvers)
    ref = _module_run(net, [x])
    seen = _recorder(monkeypatch)
    again = _module_run(net, [x])
    assert not any(w.startswith('dhdn') for w in seen)
    _switch(net, True)
    monkeypatch.setattr(unet_seam, 'ROUTED', {k: False for k in unet_seam.ROUTED})
    got = _module_run(net, [x])
    _same_where_today_repeats(got, ref, again)
    assert not any(w.startswith('dhdn') for w in seen)
    _route_all(monkeypatch)
    nchw = UNet(32, 16).to(gpu)
    nchw.load_state_dict(net.state_dict())
    _switch(nchw, False)
    ref, again = _module_run(nchw, [x.contiguous()]), _module_run(nchw, [x.contiguous()])
    assert not any(w.startswith('dhdn') for w in seen)
    _switch(nchw, True)
    got = _module_run(nchw, [x.contiguous()])
    _same_where_today_repeats(got, ref, again)
    assert seen.count('dhdn_max_pool2_forward') == 4 and 'dhdn_up_cat_forward' not in seen     # NCHW: the pool has it, the up seam not


def test_checkpointing_a_unet_changes_nothing(gpu, monkeypatch):
    from dhd_amd.detector import UNet
    _route_all(monkeypatch)
    torch.manual_seed(4)
    net = UNet(32, 16).to(gpu).to(memory_format=CL)
    _switch(net, True)
    x = torch.randn(2, 32, 32, 32, device=gpu).contiguous(memory_format=CL)
    plain, repeat = _module_run(net, [x]), _module_run(net, [x])

    class Ckpt(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, t):
            return checkpoint(self.inner, t, use_reentrant=False)
    _same_where_today_repeats(_module_run(Ckpt(net), [x]), plain, repeat)


# ------------------------------------------------------------------------------------------------ 4. graph capture

def _capture(fn, arg, other):
    """One capture and replay of fn(arg) against eager, then a replay on other inputs copied into place."""
    ref1, ref2 = fn(arg).clone(), fn(other).clone()
    _sync()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(arg)
    torch.cuda.current_stream().wait_stream(s)
    _sync()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = fn(arg)
    graph.replay()
    _sync()
    assert torch.equal(cap, ref1)
    arg.copy_(other)
    graph.replay()
    _sync()
    assert torch.equal(cap, ref2) and not torch.equal(ref1, ref2)


def test_graph_capture_of_each_wrapper(gpu):
    import dhd_amd
    with torch.no_grad():
        x, _ = US.pool_input((2, 24, 5, 7), BF16)
        x = x.to(gpu).contiguous(memory_format=CL)
        _capture(dhd_amd.max_pool2x2, x.clone(), x.flip(0).flip(-1).contiguous(memory_format=CL))
        v = {k: t.to(gpu) for k, t in US.up_inputs('c160_9x8_pad32', 'bf16').items()}
        _capture(lambda t: dhd_amd.conv_transpose2x2_cat(t, v['x2'], v['weight'], v['bias']), v['x1'].clone(),
                 v['x1'].flip(0).flip(-1).contiguous(memory_format=CL))


# ------------------------------------------------------------------------------------------------ 5. views

def _pool_run(v, c):
    import dhd_amd
    x = c.inp('x', v['x'], grad=True)
    y = dhd_amd.max_pool2x2(x)
    c.grad('gy', y).backward(v['gy'])
    _sync()
    return dict(y=y.detach(), gx=x.grad)


VIEWS = ([pytest.param('pool', t, how, id=f'pool-{t}-{how}') for t in ('x', 'gy') for how in ('offset_elem', 'nhwc_offset_elem', 'inner_step2')]
         # (an NCHW view of x1 / x2 is not a channels_last map: unsupported by design, see the refusal test)
         + [pytest.param('up', t, how, id=f'up-{t}-{how}') for t, hows in (('x1', ('nhwc_offset_elem',)), ('x2', ('nhwc_offset_elem',)),
                                                                            ('gout', ('nhwc_offset_elem', 'inner_step2'))) for how in hows])


@pytest.mark.parametrize('op,target,how', VIEWS)
def test_views(gpu, op, target, how):
    import dhd_amd
    if op == 'pool':
        x, gy = US.pool_input((2, 24, 5, 7), BF16)
        fmt = CL if how.startswith('nhwc') else torch.contiguous_format
        v = dict(x=x.to(gpu).contiguous(memory_format=fmt), gy=gy.to(gpu).contiguous(memory_format=fmt))
        run = lambda c: _pool_run(v, c)
    else:
        v = {k: t.to(gpu) for k, t in US.up_inputs('c64_4x4_pad11', 'bf16').items()}
        run = lambda c: _up_run(v, dhd_amd.conv_transpose2x2_cat, c=c)
    fresh = run(Case(None, 'fresh'))
    c = Case(target, how)
    got = run(c)
    assert len(c.parents) == 1
    for k, ref in fresh.items():
        assert got[k].shape == ref.shape and got[k].dtype == ref.dtype and torch.equal(US.bits(got[k]), US.bits(ref)), k
    assert c.untouched(), 'a parent buffer changed: the view was written to, or something wrote outside it'


# ------------------------------------------------------------------------------------------------ 6. guard bands

GUARDED = ([pytest.param('pool', s, p, id=f'pool-{s}-{p}') for s in US.POOL_SHAPES for p in ('nchw', 'nhwc')]
           + [pytest.param('up', c, p, id=f'up-{c}-{p}') for c in US.UP_CASES for p in ('f32', 'bf16')])


@pytest.mark.parametrize('op,case,prec', GUARDED)
def test_inside_guard_bands(gpu, monkeypatch, op, case, prec):
    """Plain, then with every buffer the wrappers allocate between two 4096-byte guard bands at its exact size, every byte 0xFF,
    then 0x00: no guard byte changes, the runs agree, and nothing uninitialised is read (0xFF is NaN in every float type)."""
    import dhd_amd
    if op == 'pool':
        fmt = CL if prec == 'nhwc' else torch.contiguous_format
        x, gy = US.pool_input(case, F16)
        v = dict(x=x.to(gpu).contiguous(memory_format=fmt), gy=gy.to(gpu).contiguous(memory_format=fmt))
        run, n = (lambda: _pool_run(v, Case(None, 'fresh'))), 2                  # y; gx
    else:
        v = {k: t.to(gpu) for k, t in US.up_inputs(case, prec).items()}
        run, n = (lambda: _up_run(v, dhd_amd.conv_transpose2x2_cat)), 7          # out, scratch; gx1, gx2, g_operand, dbias, scratch
    plain = run()
    for fill in (0xFF, 0x00):
        with G.guarded(monkeypatch, fill) as ledger:
            got = run()
            ledger.check()
            got = {k: t.detach().clone() for k, t in got.items()}
        ours = [e for e in ledger.sites_under(G.PRODUCT_ROOT) if 'unet_seam.py' in e.site or 'mghs_op.py' in e.site]
        print(f'{op} {case} [{prec}, fill {fill:#04x}]: {len(ledger)} guarded allocations, {ledger.total_bytes()} bytes, guards intact')
        assert len(ours) == len(ledger) == n, [e.site for e in ledger.entries]
        for k, ref in plain.items():
            assert int((torch.isfinite(ref) & ~torch.isfinite(got[k])).sum()) == 0, (k, fill)
            assert torch.equal(got[k], ref), (k, fill)


# ------------------------------------------------------------------------------------------------ 7. golden G17

def test_voxel_logits_with_the_seams_on(gpu, monkeypatch):
    """G17 in channels_last (the layout the step runs in and the one the up seam takes) with every seam routed: the float32 logits
    stay within the 1e-3 bar of the reference's recorded logits (the parent commit measures 2.6e-5 without the seams)."""
    import dhd_amd
    import test_voxel_logits as TV
    g = golden('g17_voxel_logits')
    _route_all(monkeypatch)
    seen = _recorder(monkeypatch)
    real = TV.build_model

    def build(gg):
        model, dims = real(gg)
        assert len(dhd_amd.fused_unet_seams(model, True)) == 24                  # three UNets, four seams of each kind each
        return model, dims
    monkeypatch.setattr(TV, 'build_model', build)
    model, lg, dgrad, fgrad = TV._run_product(gpu, g, 'train', channels_last=True)
    err = TV.check_logits(lg, g, 'train', 1e-3)
    TV.check_gradients(g, 'train', dgrad, fgrad, dict(model.named_parameters()))
    print(f'G17 train channels_last, UNet seams on: max logit error {err:.2e} (the parent commit, seams off: 2.6e-5)')
    assert seen.count('dhdn_max_pool2_forward') == 12 and seen.count('dhdn_up_cat_forward') == 12
    assert seen.count('dhdn_max_pool2_backward') == 12 and seen.count('dhdn_up_cat_backward') == 12
