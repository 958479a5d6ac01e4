"""dhd_amd.deform_conv on the GPU: DCN's fused forward and its HIP backward without column gradients, against
oracle/dcn_oracle.py in float64 (the twin of dcn_train_inputs.py), against today's path (DCN with the switch off) and through
DCN.forward in a small conv stack.

Bars, per tensor G of (dx, doffset, dW), on rel = max |y - twin| / max(1, |twin|max):
  float32 x (bf16x3)   rel <= 1e-4 (E_F32, the project's bar for this layer)
  fp16 / bf16 x        rel <= 1.5 x the same figure of today's path on the same stored inputs under autocast; where today's figure
                       is below 1e-4, the float32 bar
Measured figures are printed by test_gradients_against_the_float64_twin and recorded in docs/LAB_NOTEBOOK.md."""
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dcn_train_inputs as TI
from dcn_train_inputs import CASES, LAYOUTS, PRECISIONS

pytestmark = pytest.mark.gpu

CL = torch.channels_last
case_prec_layout = lambda f: pytest.mark.parametrize('case', list(CASES))(
    pytest.mark.parametrize('prec', list(PRECISIONS))(pytest.mark.parametrize('layout', LAYOUTS)(f)))

_DEV, _FUSED, _TODAY = {}, {}, {}


@pytest.fixture(scope='module', autouse=True)
def _release_what_the_module_cached():
    """The inputs and results shared among the tests above live until the module ends; then they and the allocator's cached
    blocks are released, so that the tests that follow start from the allocator state they would have without this file."""
    yield
    for cache in (_DEV, _FUSED, _TODAY):
        cache.clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def same_bytes(u, v):
    """Equal bit for bit (an integer view of the same element size keeps any strides)."""
    as_int = {2: torch.int16, 4: torch.int32}
    return u.shape == v.shape and u.dtype == v.dtype and torch.equal(u.view(as_int[u.element_size()]), v.view(as_int[v.element_size()]))


def _fmt(layout):
    return CL if layout == 'channels_last' else torch.contiguous_format


def device_inputs(case, prec, layout, gpu):
    """(x, offset, weight, gout) on the device, x and gout in the precision and layout under test; made once, only read."""
    key = (case, prec, layout, str(gpu))
    if key not in _DEV:
        _, offset, weight, _ = TI.inputs(case)
        x, gout = (t.to(gpu).contiguous(memory_format=_fmt(layout)) for t in TI.stored(case, prec))
        _DEV[key] = (x, offset.to(gpu), weight.to(gpu), gout)
    return _DEV[key]


def step(case, x, offset, weight, gout):
    """One forward + backward of deform_conv on leaves made of the arguments -> {'out', 'dx', 'doffset', 'dw'}."""
    import dhd_amd
    b, c, o, g, h, w, dil, scale = CASES[case]
    xl, ol, wl = (t.detach().requires_grad_() for t in (x, offset, weight))
    out = dhd_amd.deform_conv(xl, ol, wl, padding=dil, dilation=dil, groups=g)
    out.backward(gout)
    torch.cuda.synchronize()
    return {'out': out.detach(), 'dx': xl.grad, 'doffset': ol.grad, 'dw': wl.grad}


def fused(case, prec, layout, gpu):
    key = (case, prec, layout, str(gpu))
    if key not in _FUSED:
        _FUSED[key] = step(case, *device_inputs(case, prec, layout, gpu))
    return _FUSED[key]


def backward(case, prec, layout, gpu, want_col=True):
    """(dx, doffset, col) of one deform_conv_backward call."""
    from dhd_amd import deform_conv as DC
    b, c, o, g, h, w, dil, scale = CASES[case]
    x, offset, weight, gout = device_inputs(case, prec, layout, gpu)
    res = DC.deform_conv_backward(x, offset, weight, gout, dil, dil, g, want_col=want_col)
    torch.cuda.synchronize()
    return res


def today(case, prec, gpu):
    """Today's path on the same stored inputs: DCN with the switch off (under autocast for a half type), NCHW."""
    key = (case, prec, str(gpu))
    if key not in _TODAY:
        x, offset, weight, gout = device_inputs(case, prec, 'nchw', gpu)
        off = offset.detach().clone().requires_grad_()
        m = TI.dcn_module(case, weight, off, device=gpu)
        m.fused_train = False
        xl = x.detach().clone().requires_grad_()
        with torch.autocast('cuda', dtype=PRECISIONS[prec], enabled=prec != 'f32_bf16x3'):
            out = m(xl)
        assert out.dtype == PRECISIONS[prec]
        out.backward(gout)
        torch.cuda.synchronize()
        _TODAY[key] = {'out': out.detach(), 'dx': xl.grad, 'doffset': off.grad, 'dw': m.weight.grad}
    return _TODAY[key]


@case_prec_layout
def test_forward_is_the_inference_operator(gpu, case, prec, layout):
    import dhd_amd
    b, c, o, g, h, w, dil, scale = CASES[case]
    x, offset, weight, gout = device_inputs(case, prec, layout, gpu)
    want = dhd_amd.deform_conv_infer(x, offset, weight, padding=dil, dilation=dil, groups=g)
    got = fused(case, prec, layout, gpu)['out']
    assert got.dtype == x.dtype and got.stride() == want.stride() and torch.equal(got, want)


@case_prec_layout
def test_col_operand_is_what_im2col_writes(gpu, case, prec, layout):
    from dhd_amd import _lib
    b, c, o, g, h, w, dil, scale = CASES[case]
    x = device_inputs(case, prec, layout, gpu)[0]
    offset = device_inputs(case, prec, layout, gpu)[1]
    col = backward(case, prec, layout, gpu)[2]
    xn = x.contiguous()
    want = torch.full((b, c * 9, h * w), float('nan'), dtype=x.dtype, device=gpu)
    code = _lib.dtype_code(x.dtype)
    assert _lib.load().dhd_deform_im2col_t(_lib.ptr(xn), code, _lib.ptr(offset), _lib.ptr(want), code, b, c, h, w, 3, dil, dil,
                                           _lib.stream_ptr(x.device)) == 0
    torch.cuda.synchronize()
    assert col.dtype == x.dtype and col.shape == want.shape and same_bytes(col, want)
    assert backward(case, prec, layout, gpu, want_col=False)[2] is None


@case_prec_layout
def test_gradients_against_the_float64_twin(gpu, case, prec, layout):
    tw = TI.twin(case, prec)
    got = fused(case, prec, layout, gpu)
    x = device_inputs(case, prec, layout, gpu)[0]
    assert got['dx'].dtype == x.dtype and got['dx'].stride() == x.stride()
    assert got['doffset'].dtype == torch.float32 and got['dw'].dtype == torch.float32
    base = today(case, prec, gpu) if prec != 'f32_bf16x3' else None
    failed = []
    for k in TI.TENSORS:
        if case == 'zero_offset' and k == 'doffset':
            continue            # every coordinate is integral: test_zero_offsets_against_the_plain_convolution
        assert got[k].shape == tw[k].shape and bool(torch.isfinite(got[k]).all()), k
        err = TI.rel_error(got[k], tw[k])
        terr = TI.rel_error(base[k], tw[k]) if base is not None else 0.0
        E = TI.bar(prec, terr)
        print(f'deform_conv {prec} {layout} {case} {k}: rel error {err:.3e}, today {terr:.3e}, bar {E:.3e}')
        if err > E:
            failed.append((k, err, E))
    assert not failed, failed


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('layout', LAYOUTS)
def test_zero_offsets_against_the_plain_convolution(gpu, prec, layout):
    """DCN's initial state: out, dx and dW against float64 F.conv2d autograd on the stored values; doffset, whose coordinates are
    all integral, against today's HIP path (same dtypes, same inputs) within the float32 bar: the operator forms the offset sums
    from dcol rounded once to the GEMM type, as the column path's GEMM hands it to deform_col2offset (measured difference 5.4e-6 in
    float32, 2.3e-7 in fp16, 1.3e-7 in bf16)."""
    case = 'zero_offset'
    b, c, o, g, h, w, dil, scale = CASES[case]
    xs, gs = (t.double() for t in TI.stored(case, prec))
    xs.requires_grad_()
    wd = TI.inputs(case)[2].double().requires_grad_()
    ref_out = F.conv2d(xs, wd, padding=dil, dilation=dil, groups=g)
    ref_out.backward(gs)
    got = fused(case, prec, layout, gpu)
    base = today(case, prec, gpu)
    for k, ref in (('out', ref_out.detach()), ('dx', xs.grad), ('dw', wd.grad)):
        err, terr = TI.rel_error(got[k], ref), TI.rel_error(base[k], ref)
        E = TI.bar(prec, terr)
        print(f'deform_conv zero offsets {prec} {layout} {k}: rel error vs conv2d {err:.3e}, today {terr:.3e}, bar {E:.3e}')
        assert err <= E, (k, err, E)
    err = TI.rel_error(got['doffset'], base['doffset'].cpu().double())
    tw = TI.twin(case, prec)['doffset']
    print(f'deform_conv zero offsets {prec} {layout} doffset: rel difference to today\'s path {err:.3e}, bar {TI.E_F32:.1e}; against the '
          f'float64 twin: the operator {TI.rel_error(got["doffset"], tw):.3e}, today\'s path {TI.rel_error(base["doffset"], tw):.3e}')
    assert err <= TI.E_F32, err


@case_prec_layout
def test_two_calls_give_the_same_bytes(gpu, case, prec, layout):
    a = backward(case, prec, layout, gpu)
    b = backward(case, prec, layout, gpu)
    for name, u, v in zip(('dx', 'doffset', 'col'), a, b):
        assert u.data_ptr() != v.data_ptr() and same_bytes(u, v), name
    first = fused(case, prec, layout, gpu)
    assert torch.equal(a[0], first['dx']) and torch.equal(a[1], first['doffset'])


@pytest.mark.parametrize('case', ['g13_2x32x6x10', 'g1_3x64to128x7x9_dil2', 'one_cell_1x256x1x1', 'outside_2x128to64x5x70'])
@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('layout', LAYOUTS)
def test_inside_guard_bands(gpu, monkeypatch, case, prec, layout):
    """dx, doffset, col and the pooled scratch (at exactly the advertised size) between guard bands, at the partial-tile cases and at
    H * W = 1: the bands are intact, and the results are those of the unguarded call."""
    from guarded_alloc import guarded
    want = backward(case, prec, layout, gpu)
    with guarded(monkeypatch, fill=0xFF) as ledger:
        got = backward(case, prec, layout, gpu)
        ledger.check()
        sites = [e.site for e in ledger.entries]
        assert len(ledger) >= 4 and any('mghs_op.py' in s for s in sites) and sum('deform_conv.py' in s for s in sites) >= 3, sites
    for u, v in zip(got, want):
        assert same_bytes(u, v)


def _touched_cells(case, image, p):
    """Cells the taps of pixel `p` of `image` touch, and which taps lie inside, from the float64 coordinates."""
    b, c, o, g, h, w, dil, scale = CASES[case]
    co = TI.coordinates(case, TI.inputs(case)[1])[image].reshape(9, 2, h * w)[:, :, p]
    cells, inside = set(), []
    for t in range(9):
        py, px = co[t]
        ok = -1 < py < h and -1 < px < w
        inside.append(ok)
        if ok:
            y0, x0 = int(np.floor(py)), int(np.floor(px))
            cells |= {yy * w + xx for yy in (y0, y0 + 1) for xx in (x0, x0 + 1) if 0 <= yy < h and 0 <= xx < w}
    return cells, inside


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('layout', LAYOUTS)
def test_a_nan_in_gout_stays_where_its_taps_reach(gpu, prec, layout):
    """One NaN at (image 1, output channel 9, pixel 27) of gout: dx is NaN exactly in the cells that pixel's taps touch, in the
    channels of the output channel's group, of that image; doffset exactly in that pixel's entries of the taps inside the image."""
    from dhd_amd import deform_conv as DC
    case = 'g13_2x32x6x10'
    b, c, o, g, h, w, dil, scale = CASES[case]
    x, offset, weight, gout = device_inputs(case, prec, layout, gpu)
    image, och, p = 1, 9, 27
    gn = gout.clone(memory_format=torch.preserve_format)
    gn[image, och, p // w, p % w] = float('nan')
    dx, doff, col = DC.deform_conv_backward(x, offset, weight, gn, dil, dil, g)
    torch.cuda.synchronize()
    cells, inside = _touched_cells(case, image, p)
    assert cells and any(inside)
    want_dx = torch.zeros(b, c, h * w, dtype=torch.bool)
    grp = och // (o // g)
    want_dx[image, grp * (c // g):(grp + 1) * (c // g), sorted(cells)] = True
    want_doff = torch.zeros(b, 18, h * w, dtype=torch.bool)
    for t in range(9):
        if inside[t]:
            want_doff[image, 2 * t:2 * t + 2, p] = True
    assert torch.equal(torch.isnan(dx).cpu().reshape(b, c, h * w), want_dx)
    assert torch.equal(torch.isnan(doff).cpu().reshape(b, 18, h * w), want_doff)
    assert bool(torch.isfinite(col).all())
    clean = backward(case, prec, layout, gpu)
    keep = ~want_dx.reshape(dx.shape).to(gpu)
    assert torch.equal(dx[keep], clean[0][keep])


VIEWS = [('x', k) for k in ('offset_elem', 'channel_slice', 'nhwc_offset_elem')] + [('gout', k) for k in ('offset_elem', 'channel_slice',
                                                                                                         'nhwc_offset_elem')]


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('target,kind', VIEWS)
def test_views(gpu, prec, target, kind):
    """x or gout as a strided or 16-byte-misaligned view carved out of a poisoned parent (test_gpu_views.present): the dense call's
    bytes in every result (the wrapper copies the view into its own layout and the same kernels run), the parent untouched."""
    from test_gpu_views import present
    case = 'g13_2x32x6x10'
    x, offset, weight, gout = device_inputs(case, prec, 'nchw', gpu)
    args = dict(x=x, offset=offset, weight=weight, gout=gout)
    dense = dict(args)
    if kind.startswith('nhwc'):
        dense[target] = args[target].contiguous(memory_format=CL)
    want = step(case, **dense)
    view, parent = present(args[target], kind)
    snap = parent.view(torch.uint8).clone()
    args[target] = view
    got = step(case, **args)
    for k in ('out', 'dx', 'doffset', 'dw'):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(parent.view(torch.uint8), snap), 'a parent buffer changed'


# --------------------------------------------------------------------------- the module route

def _stack(gpu, k=3):
    """A HeightNet-like stack in small: conv, DCN (32 channels, 4 groups, live offsets), conv."""
    from dhd_amd.depthnet import DCN
    torch.manual_seed(11)
    net = torch.nn.Sequential(torch.nn.Conv2d(16, 32, 3, padding=1), DCN(32, 32, k, padding=k // 2, groups=4), torch.nn.Conv2d(32, 8, 1))
    with torch.no_grad():
        net[1].conv_offset.weight.normal_(0, 0.05)
        net[1].conv_offset.bias.normal_(0, 1.0)
    return net.to(gpu)


def _recorder(monkeypatch):
    """-> the names of the training surface's entry points as they are called, and 'im2col' for today's sampling kernel."""
    from dhd_amd import _deform_train, _lib
    seen = []
    real_call, real_check = _deform_train.call, _lib.check

    def call(name, *a):
        seen.append(name)
        return real_call(name, *a)

    def check(rc, what):
        if what == 'dhd_deform_im2col_t':
            seen.append('im2col')
        return real_check(rc, what)
    monkeypatch.setattr(_deform_train, 'call', call)
    monkeypatch.setattr(_lib, 'check', check)
    return seen


def _route_everything(monkeypatch):
    from dhd_amd import deform_conv as DC
    monkeypatch.setattr(DC, 'ROUTED_TRAIN', {k: True for k in DC.ROUTED_TRAIN})


def _module_step(net, x, gout, autocast=None, ckpt=False):
    from torch.utils.checkpoint import checkpoint
    net.zero_grad(set_to_none=True)
    xl = x.detach().clone().requires_grad_()
    with torch.autocast('cuda', dtype=autocast or torch.float16, enabled=autocast is not None):
        out = checkpoint(net, xl, use_reentrant=False) if ckpt else net(xl)
    out.backward(gout.to(out.dtype))
    torch.cuda.synchronize()
    return [out.detach(), xl.grad] + [p.grad.clone() for p in net.parameters()]


def _module_inputs(gpu, h=6, w=10):
    gen = torch.Generator().manual_seed(12)
    return torch.randn(2, 16, h, w, generator=gen).to(gpu), torch.randn(2, 8, h, w, generator=gen).to(gpu)


def _close(got, want, E):
    return all(float((a.double() - b.double()).abs().max()) <= E * max(1.0, float(b.double().abs().max())) for a, b in zip(got, want))


def _todays_path_again(got, want):
    """The forward's bytes; the gradients within the float32 bar only, because today's backward orders its cell sums by LDS atomics
    and does not repeat its own bytes from one call to the next."""
    return torch.equal(got[0], want[0]) and _close(got[1:], want[1:], TI.E_F32)


def test_module_route_in_train_mode_and_under_checkpoint(gpu, monkeypatch):
    """Switch on, train mode, float32: the operator is reached (forward and backward), no column matrix is written, and the
    output and the gradients of the input and of every parameter are within the float32 bar of the switch off; under
    torch.utils.checkpoint the same bytes as without it; with the switch off the calls of the parent and its forward's bytes (its
    backward does not repeat its own bytes: _todays_path_again)."""
    import dhd_amd
    _route_everything(monkeypatch)
    net = _stack(gpu).train()
    x, gout = _module_inputs(gpu)
    seen = _recorder(monkeypatch)
    assert net[1].fused_train is False
    off = _module_step(net, x, gout)
    assert seen == ['im2col'], seen
    assert dhd_amd.fused_dcn_training(net) == [net[1]] and net[1].fused_train is True and net[1]._train_applies(x.new_empty(2, 32, 6, 10))
    del seen[:]
    on = _module_step(net, x, gout)
    assert seen.count('dhdd_deform_conv_backward') == 1 and 'im2col' not in seen, seen
    assert len(on) == len(off) == 9 and _close(on, off, TI.E_F32)
    del seen[:]
    ck = _module_step(net, x, gout, ckpt=True)
    assert seen.count('dhdd_deform_conv_backward') == 1 and all(torch.equal(a, b) for a, b in zip(ck, on))
    net.eval()
    with torch.no_grad():
        assert torch.equal(net(x), on[0])                     # eval mode, no grad: the same operator
    assert dhd_amd.fused_dcn_training(net, False) == [net[1]] and net[1].fused_train is False
    net.train()
    del seen[:]
    again = _module_step(net, x, gout)
    assert seen == ['im2col'] and _todays_path_again(again, off)


def test_module_route_under_fp16_autocast(gpu, monkeypatch):
    """Both paths see the same fp16 offsets and round the same quantities to fp16 at different points (today: col, dcol, dx; the
    operator: the gathered gout sums, col, dx).  A rounding is at most 2^-11 relative and a gradient passes at most three per
    path, six in the difference, so 6 x 2^-11 max(1, |today|max) bounds it; the convolutions around are the same in both."""
    import dhd_amd
    _route_everything(monkeypatch)
    net = _stack(gpu).train()
    x, gout = _module_inputs(gpu)
    off = _module_step(net, x, gout, autocast=torch.float16)
    dhd_amd.fused_dcn_training(net)
    seen = _recorder(monkeypatch)
    on = _module_step(net, x, gout, autocast=torch.float16)
    assert seen.count('dhdd_deform_conv_backward') == 1 and 'im2col' not in seen, seen
    assert [t.dtype for t in on] == [t.dtype for t in off] and on[0].dtype == torch.float16
    assert _close(on, off, 6 * 2.0 ** -11)


def test_module_route_inside_a_graph_capture(gpu, monkeypatch):
    """Forward and backward captured once on one stream, replayed on fresh contents of the static input: the eager results."""
    import dhd_amd
    _route_everything(monkeypatch)
    net = _stack(gpu).train()
    dhd_amd.fused_dcn_training(net)
    x, gout = _module_inputs(gpu)
    x2 = x * 0.5 + 0.25
    ref1, ref2 = _module_step(net, x, gout), _module_step(net, x2, gout)
    static = x.clone().requires_grad_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            net.zero_grad(set_to_none=True)
            static.grad = None
            net(static).backward(gout)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    net.zero_grad(set_to_none=True)
    static.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net(static)
        out.backward(gout)
    for xs, ref in ((x, ref1), (x2, ref2)):
        with torch.no_grad():
            static.copy_(xs)
        g.replay()
        torch.cuda.synchronize()
        got = [out.detach(), static.grad] + [p.grad for p in net.parameters()]
        assert all(torch.equal(a, b) for a, b in zip(got, ref))
    assert not torch.equal(ref1[0], ref2[0])


@pytest.mark.parametrize('why', ['map_over_the_limit', 'k5', 'not_routed'])
def test_an_unsupported_call_takes_todays_path(gpu, monkeypatch, why):
    import dhd_amd
    if why != 'not_routed':
        _route_everything(monkeypatch)
    else:
        from dhd_amd import deform_conv as DC
        monkeypatch.setattr(DC, 'ROUTED_TRAIN', {k: False for k in DC.ROUTED_TRAIN})
    net = _stack(gpu, k=5 if why == 'k5' else 3).train()
    h, w = (27, 32) if why == 'map_over_the_limit' else (6, 10)        # 864 cells: over 853
    x, gout = _module_inputs(gpu, h, w)
    off = _module_step(net, x, gout)
    dhd_amd.fused_dcn_training(net)
    assert not net[1]._train_applies(x.new_empty(2, 32, h, w))
    seen = _recorder(monkeypatch)
    on = _module_step(net, x, gout)
    assert seen == ['im2col'] and _todays_path_again(on, off)
    if why == 'map_over_the_limit':
        assert net[1]._train_applies(x.new_empty(2, 32, 1, 853)) and not net[1]._train_applies(x.new_empty(2, 32, 1, 854))


def test_nothing_of_column_size_is_held_between_forward_and_backward(gpu):
    """8 x 256 x 16 x 44 in fp16: the bytes held after the forward above the state before it are at most bytes(x) + bytes(offset)
    + bytes(out) + 64 KiB; today's path exceeds that by the column matrix."""
    import dhd_amd
    from dhd_amd.depthnet import DCN
    b, c, h, w = 8, 256, 16, 44
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(b, c, h, w, generator=gen).to(gpu).half()
    offset = (torch.randn(b, 18, h, w, generator=gen) * 0.5).to(gpu)
    m = DCN(c, c, groups=4).to(gpu)
    m.conv_offset = TI.FixedOffset(offset)
    budget = x.numel() * 2 + offset.numel() * 4 + b * c * h * w * 2 + 64 * 1024
    col_bytes = b * c * 9 * h * w * 2

    def held(run):
        for _ in range(2):                                    # the pooled scratch and the library's handles exist before
            out = run()
            out.float().sum().backward()
            del out
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(gpu)
        out = run()
        torch.cuda.synchronize()
        after = torch.cuda.memory_allocated(gpu)
        del out
        return after - before
    fused_held = held(lambda: dhd_amd.deform_conv(x.detach().requires_grad_(), offset, m.weight, 1, 1, 4))
    with torch.autocast('cuda', dtype=torch.float16):
        today_held = held(lambda: m(x.detach().requires_grad_()))
    print(f'held after the forward: fused {fused_held} bytes, today {today_held} bytes, budget {budget}, column matrix {col_bytes}')
    assert fused_held <= budget and today_held >= budget + col_bytes
