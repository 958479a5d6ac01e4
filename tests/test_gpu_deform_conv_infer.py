"""dhd_deform_conv_infer on the GPU: the fused deformable convolution of inference against oracle/dcn_oracle.py in float64,
through the C ABI, through dhd_amd.deform_conv_infer and through DCN.forward / HeightNet on the G13 fixture.

Inputs, reference and bounds: dcn_infer_inputs.py.  One bound per precision, |y - R| <= E max(1, |R|max):
  float32 x (bf16x3)   E = 1e-4, the bar test_dcn_hip_sampling_vs_grid_sample_formulation holds this layer's output to
  fp16 / bf16 x        E = 2 E0, E0 = max |R - chain| computed on the CPU (columns and weights rounded to the half type, float64
                       product, result rounded); the factor 2 covers summation order and single-ulp column flips.
Measured errors are printed by test_against_the_float64_oracle and recorded in docs/LAB_NOTEBOOK.md."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from dcn_infer_inputs import CASES, LAYOUTS, PRECISIONS, bound, inputs, reference, scale_of, stored_x

pytestmark = pytest.mark.gpu

CL = torch.channels_last
case_prec_layout = lambda f: pytest.mark.parametrize('case', list(CASES))(
    pytest.mark.parametrize('prec', list(PRECISIONS))(pytest.mark.parametrize('layout', LAYOUTS)(f)))

_DEV = {}


def device_inputs(case, prec, layout, gpu):
    """(x in the precision and layout under test, offset, weight) on the device, made once and only read."""
    key = (case, prec, layout, str(gpu))
    if key not in _DEV:
        _, offset, weight = inputs(case)
        x = stored_x(case, prec).to(gpu)
        if layout == 'channels_last':
            x = x.contiguous(memory_format=CL)
        _DEV[key] = (x, offset.to(gpu), weight.to(gpu))
    return _DEV[key]


def run(case, x, offset, weight, **kw):
    from dhd_amd import deform_conv_infer
    b, c, o, g, h, w, dil, scale = CASES[case]
    return deform_conv_infer(x, offset, weight, padding=dil, dilation=dil, groups=g, **kw)


def run_capi(case, x, offset, weight, fill=0xCD):
    """Through the C ABI with a scratch of exactly the advertised size and `out` pre-filled with NaN."""
    from dhd_amd import _lib
    lib = _lib.load()
    b, c, o, g, h, w, dil, scale = CASES[case]
    layout = int(not x.is_contiguous())
    code = _lib.DTYPE_CODE[x.dtype]
    n = C.c_size_t()
    assert lib.dhd_deform_conv_infer_scratch_bytes(b, c, o, g, 3, h, w, code, layout, C.byref(n)) == 0 and n.value % 16 == 0
    scratch = torch.full((n.value,), fill, dtype=torch.uint8, device=x.device)
    out = torch.full((b, o, h, w), float('nan'), dtype=x.dtype, device=x.device)
    if layout:
        out = out.contiguous(memory_format=CL)
    rc = lib.dhd_deform_conv_infer(_lib.ptr(x), code, layout, _lib.ptr(offset), _lib.ptr(weight), _lib.ptr(out), b, c, o, g, h, w, 3, dil, dil,
                                   0, _lib.ptr(scratch), n.value, _lib.stream_ptr(x.device))
    torch.cuda.synchronize()
    assert rc == 0
    return out


def within(y, ref, E):
    return float((y.detach().cpu().double() - ref).abs().max()) / scale_of(ref), E


@case_prec_layout
def test_against_the_float64_oracle(gpu, case, prec, layout):
    """Every element written (out starts as NaN) and within E of the float64 reference; the same bytes whatever the scratch held,
    from a second call and through the Python wrapper; the inputs are only read."""
    x, offset, weight = device_inputs(case, prec, layout, gpu)
    keep = [t.clone() for t in (x, offset, weight)]
    ref, E = reference(case, prec), bound(case, prec)
    y = run_capi(case, x, offset, weight)
    assert y.dtype == x.dtype and y.shape == ref.shape
    assert y.is_contiguous(memory_format=CL) if layout == 'channels_last' else y.is_contiguous()
    assert bool(torch.isfinite(y).all())
    err, _ = within(y, ref, E)
    print(f'deform_conv_infer {prec} {layout} {case}: max |y - float64| / max(1, |R|max) = {err:.3e}, bound E = {E:.3e}')
    assert err <= E, (err, E)
    assert torch.equal(run_capi(case, x, offset, weight, fill=0x00), y)
    pooled = run(case, x, offset, weight)
    assert torch.equal(pooled, y) and pooled.stride() == y.stride() and pooled.dtype == x.dtype
    assert all(torch.equal(a, b) for a, b in zip((x, offset, weight), keep))


@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('prec', list(PRECISIONS))
def test_both_layouts_agree(gpu, case, prec):
    ref, E = reference(case, prec), bound(case, prec)
    a = run(case, *device_inputs(case, prec, 'nchw', gpu))
    b = run(case, *device_inputs(case, prec, 'channels_last', gpu))
    assert a.is_contiguous() and b.is_contiguous(memory_format=CL)
    err = float((a.double() - b.double()).abs().max()) / scale_of(ref)
    assert err <= E, (err, E)


@pytest.mark.parametrize('case', ['g13_2x32x6x10', 'g1_3x64to128x7x9_dil2', 'dhds_2x256x16x44'])
@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('layout', LAYOUTS)
def test_zero_offsets_give_the_plain_convolution(gpu, case, prec, layout):
    b, c, o, g, h, w, dil, scale = CASES[case]
    x, offset, weight = device_inputs(case, prec, layout, gpu)
    ref = F.conv2d(stored_x(case, prec).double(), inputs(case)[2].double(), padding=dil, dilation=dil, groups=g)
    y = run(case, x, torch.zeros_like(offset), weight)
    err, E = within(y, ref, bound(case, prec))
    print(f'deform_conv_infer zero offsets {prec} {layout} {case}: error vs conv2d {err:.3e}, bound E = {E:.3e}')
    assert err <= E, (err, E)


VIEW_CASE = 'g13_2x32x6x10'
VIEWS = ([('x', k) for k in ('offset16', 'offset_elem', 'channel_slice', 'nhwc', 'nhwc_offset_elem')] +
         [('offset', k) for k in ('offset_elem', 'channel_slice')] + [('weight', 'offset_elem')])


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('target,kind', VIEWS)
def test_views(gpu, prec, target, kind):
    """One tensor shown as a view carved out of a poisoned parent (test_gpu_views.present), the others fresh: the fresh run's
    result -- identical where x keeps its layout (the wrapper copies the view and the same kernels run), within the bound for a
    channels_last x against the NCHW fresh run -- and every byte of the parent, values and poison, as it was."""
    from test_gpu_views import present
    x, offset, weight = device_inputs(VIEW_CASE, prec, 'nchw', gpu)
    fresh = run(VIEW_CASE, x, offset, weight)
    args = dict(x=x, offset=offset, weight=weight)
    view, parent = present(args[target], kind)
    snap = parent.view(torch.uint8).clone()
    args[target] = view
    got = run(VIEW_CASE, **args)
    torch.cuda.synchronize()
    assert got.shape == fresh.shape and got.dtype == fresh.dtype and bool(torch.isfinite(got).all())
    if kind.startswith('nhwc'):
        assert got.is_contiguous(memory_format=CL)
        ref, E = reference(VIEW_CASE, prec), bound(VIEW_CASE, prec)
        assert float((got.double() - fresh.double()).abs().max()) / scale_of(ref) <= E
    else:
        assert got.is_contiguous() and torch.equal(got, fresh)
    assert torch.equal(parent.view(torch.uint8), snap), 'a parent buffer changed'


# --------------------------------------------------------------------------- the module path

def _recorder(monkeypatch):
    """-> list of the names that reach _lib.call (the new operator's only way into the library) followed by the `what` of every
    _lib.check (how the older wrappers report an entry point), as 'call:<name>' / 'check:<name>'."""
    from dhd_amd import _lib
    seen = []
    real_call, real_check = _lib.call, _lib.check

    def call(name, *a):
        seen.append('call:' + name)
        return real_call(name, *a)

    def check(rc, what):
        seen.append('check:' + what)
        return real_check(rc, what)
    monkeypatch.setattr(_lib, 'call', call)
    monkeypatch.setattr(_lib, 'check', check)
    return seen


def _height_case(gpu):
    from test_host_logic import _g13_case
    g, net, x, mlp = _g13_case('height', gpu)
    return g, net, x.detach(), mlp


def test_heightnet_routes_through_the_fused_operator(gpu, monkeypatch):
    """HeightNet with G13's parameters, eval mode, no_grad, fused_inference(net): within the GPU tolerance of the fixture (5e-4, as
    check_g13 is called on the GPU); dhd_deform_conv_infer reached once, dhd_deform_im2col_t not at all."""
    import numpy as np
    import dhd_amd
    g, net, x, mlp = _height_case(gpu)
    net.eval()
    switched = dhd_amd.fused_inference(net)
    assert len(switched) == 1 and switched[0].fused_infer is True
    seen = _recorder(monkeypatch)
    with torch.no_grad():
        out = net(x, mlp)
    torch.cuda.synchronize()
    assert seen.count('call:dhd_deform_conv_infer') == 1 and 'check:dhd_deform_im2col_t' not in seen, seen
    ref = g['height.eval.out']
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print(f'G13 HeightNet eval with the fused DCN: max error {err:.2e} (atol {5e-4 * max(1.0, np.abs(ref).max()):.2e})')
    np.testing.assert_allclose(out.cpu().numpy(), ref, atol=5e-4 * max(1.0, np.abs(ref).max()), rtol=1e-3)


@pytest.mark.parametrize('how', ['default_switch', 'train_mode', 'requires_grad'])
def test_heightnet_keeps_todays_path(gpu, monkeypatch, how):
    """fused_infer at its default, train mode, or an input that requires grad under enabled grad: the fused entry point is not
    reached and the output equals today's path bit for bit."""
    import dhd_amd
    _, net, x, mlp = _height_case(gpu)
    net.train(how == 'train_mode')
    for mod in net.modules():              # ASPP's Dropout(0.5) off, as the fixture was recorded
        if isinstance(mod, torch.nn.Dropout):
            mod.eval()
    with torch.no_grad():
        today = net(x, mlp)                # every switch off: the parent's path
    if how != 'default_switch':
        dhd_amd.fused_inference(net)
    seen = _recorder(monkeypatch)
    if how == 'requires_grad':
        out = net(x.clone().requires_grad_(), mlp)
    else:
        with torch.no_grad():              # train mode: batch statistics, so the moved running statistics do not matter
            out = net(x, mlp)
    torch.cuda.synchronize()
    assert 'call:dhd_deform_conv_infer' not in seen and seen.count('check:dhd_deform_im2col_t') == 1, seen
    assert torch.equal(out.detach(), today)


def test_an_unsupported_layer_falls_back(gpu, monkeypatch):
    from dhd_amd.depthnet import DCN
    torch.manual_seed(5)
    m = DCN(12, 12, groups=4).to(gpu).eval()
    with torch.no_grad():
        m.conv_offset.bias.normal_(0, 1.0)
    x = torch.randn(2, 12, 5, 7, device=gpu)
    with torch.no_grad():
        today = m(x)
        m.fused_infer = True
        assert not m.fused_applies(x)
        seen = _recorder(monkeypatch)
        out = m(x)
    assert 'call:dhd_deform_conv_infer' not in seen and seen.count('check:dhd_deform_im2col_t') == 1
    assert torch.equal(out, today)


def test_autocast_fp16_channels_last_returns_what_todays_path_returns(gpu, monkeypatch):
    from dhd_amd.depthnet import DCN
    torch.manual_seed(6)
    m = DCN(32, 32, groups=4).to(gpu).eval()
    with torch.no_grad():
        m.conv_offset.bias.normal_(0, 1.0)
    x = torch.randn(2, 32, 6, 10, device=gpu).contiguous(memory_format=CL)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):
        today = m(x)
        m.fused_infer = True
        assert m.fused_applies(x)
        seen = _recorder(monkeypatch)
        out = m(x)
    assert seen.count('call:dhd_deform_conv_infer') == 1
    assert out.dtype == today.dtype == torch.float16 and out.shape == today.shape and out.stride() == today.stride()
    # both are fp16 products of the same half columns: a few ulps of the output apart
    assert float((out.float() - today.float()).abs().max()) <= 4 * 2 ** -11 * max(1.0, float(today.float().abs().max()))


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('layout', LAYOUTS)
def test_call_is_graph_capturable(gpu, prec, layout):
    """One capture and replay of the wrapper gives the eager bytes, also on fresh contents of the static input: scratch comes
    from the pool (warmed on a side stream), nothing is allocated or synchronised inside the call."""
    case = 'g13_2x32x6x10'
    x, offset, weight = device_inputs(case, prec, layout, gpu)
    x = x.clone(memory_format=torch.preserve_format)
    x2 = (x.float() * 0.5 + 0.25).to(x.dtype).contiguous(memory_format=CL if layout == 'channels_last' else torch.contiguous_format)
    assert x2.stride() == x.stride()
    ref1, ref2 = run(case, x, offset, weight).clone(), run(case, x2, offset, weight).clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(case, x, offset, weight)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = run(case, x, offset, weight)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, ref1)
    x.copy_(x2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, ref2) and not torch.equal(ref1, ref2)
