"""The Swin seam operators (dhd_amd/swin_seam.py, csrc/swin_seam.h) on the GPU: against the float64 twin of
tests/swin_seam_inputs.py, inside `PatchMerging` / `PatchEmbed` / `SwinTransformer` on the G10 fixture, on views, and inside
guard bands.

Bounds.  Float32 results are held to the project's layer bar, |y - Y64| <= 1e-4 max(1, |Y64|max).  A half result of the forward
needs no tolerance: it must equal the operator's own float32 result cast to that type.  Where dx is stored in a half type the
stored value is the float32 result rounded once more, so its bound adds one unit roundoff of that type relative to the exact
value, u = 2^-8 (bfloat16) or 2^-11 (float16), plus 2^-25 for float16, half the spacing of its subnormals.  Under bf16 autocast a
module is held to 1.5 x the error today's autocast path makes on the same inputs against float64.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as G  # noqa: E402
import swin_seam_inputs as SS  # noqa: E402
from conftest import golden  # noqa: E402
from test_gpu_views import Case  # noqa: E402  (present() behind Case.inp / Case.grad: tensors carved out of poisoned parents)

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
UNIT = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}
TINY = {F32: 0.0, F16: 2.0 ** -25, BF16: 0.0}
BAR = 1e-4
pytestmark = pytest.mark.gpu
GRID = [pytest.param(k, c, p, id=f'{k}-{c}-{p}') for k in ('merge', 'embed') for c, p in SS.grid(k)]


def _sync():
    """Wait for the device; after a device error nothing more is started in this module."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'GPU fault, stopping the module: {e}', returncode=3)


def _on(gpu, kind, case, prec):
    return {k: t.to(gpu) for k, t in SS.inputs(kind, case, prec).items()}


def _err(got, ref64):
    return float((got.detach().cpu().double() - ref64).abs().max())


def _op(kind, case, x, gamma, beta, out_dtype=None):
    import dhd_amd
    if kind == 'merge':
        B, H, W, C = SS.MERGE_CASES[case]
        return dhd_amd.patch_merge_norm(x, gamma, beta, SS.EPS, (H, W), out_dtype)
    return dhd_amd.patch_embed_norm(x, gamma, beta, SS.EPS, out_dtype)


def _recorder(monkeypatch):
    """The names that reach dhd_amd._lib.check: every dhds_* call goes through it."""
    from dhd_amd import _lib, _seam
    _seam.load()
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
    from dhd_amd import swin_seam
    monkeypatch.setattr(swin_seam, 'ROUTED', _Everything())


# ------------------------------------------------------------------------------------------------ 1. forward

@pytest.mark.parametrize('kind,case,prec', GRID)
def test_forward_against_the_float64_twin(gpu, kind, case, prec):
    v, (xdt, odt) = _on(gpu, kind, case, prec), SS.precisions(kind)[prec]
    y32 = _op(kind, case, v['x'], v['gamma'], v['beta'], F32)
    _sync()
    Y64 = SS.twin(kind, case, prec)[0]
    err = _err(y32, Y64)
    print(f'{kind} {case} [{prec}]: max |y - Y64| = {err:.3e}, bound {BAR * SS.scale_of(Y64):.3e}')
    assert tuple(y32.shape) == SS.out_shape(kind, case) and y32.dtype == F32 and y32.is_contiguous()
    assert err <= BAR * SS.scale_of(Y64)
    if odt != F32:
        y = _op(kind, case, v['x'], v['gamma'], v['beta'], odt)
        _sync()
        assert y.dtype == odt and torch.equal(y, y32.to(odt))
    if xdt == odt:                                                           # the default result dtype is x's
        assert _op(kind, case, v['x'], v['gamma'], v['beta']).dtype == xdt
    if kind == 'merge':                                                      # the (B, H, W, C) spelling of the same map
        B, H, W, C = SS.MERGE_CASES[case]
        assert torch.equal(_op(kind, case, v['x'].view(B, H, W, C), v['gamma'], v['beta'], F32), y32)


# ------------------------------------------------------------------------------------------------ 2. backward

def _grads(v, kind, case, prec, dy):
    x, g, b = (v[k].clone().requires_grad_() for k in ('x', 'gamma', 'beta'))
    y = _op(kind, case, x, g, b, SS.precisions(kind)[prec][1])
    y.backward(dy)
    _sync()
    return x.grad, g.grad, b.grad


@pytest.mark.parametrize('kind,case,prec', GRID)
def test_backward_against_the_twins_autograd(gpu, kind, case, prec):
    v, (xdt, odt) = _on(gpu, kind, case, prec), SS.precisions(kind)[prec]
    dx, dg, db = _grads(v, kind, case, prec, v['dy'])
    _, DX, DG, DB = SS.twin(kind, case, prec)
    assert dx.dtype == xdt and dx.shape == v['x'].shape and dg.dtype == F32 and db.dtype == F32 and dg.shape == db.shape == v['gamma'].shape
    assert dx.stride() == v['x'].stride()
    print(f'{kind} {case} [{prec}]: max |dx - DX| = {_err(dx, DX):.3e} (|DX|max {float(DX.abs().max()):.3e}), |dgamma - DG| = {_err(dg, DG):.3e} '
          f'(|DG|max {float(DG.abs().max()):.3e}), |dbeta - DB| = {_err(db, DB):.3e} (|DB|max {float(DB.abs().max()):.3e})')
    assert _err(dg, DG) <= BAR * SS.scale_of(DG) and _err(db, DB) <= BAR * SS.scale_of(DB)
    if xdt == F32:
        assert _err(dx, DX) <= BAR * SS.scale_of(DX)
    else:       # dx is stored in x's half type: the float32 result, rounded once more
        assert bool(((dx.cpu().double() - DX).abs() <= BAR * SS.scale_of(DX) + UNIT[xdt] * DX.abs() + TINY[xdt]).all())
    # no atomics: a second run gives the same bytes
    again = _grads(v, kind, case, prec, v['dy'])
    assert all(torch.equal(a, b) for a, b in zip((dx, dg, db), again))


# ------------------------------------------------------------------------------------------------ 3. modules

def _merge_module(gpu, C=32, **kw):
    from dhd_amd.swin import PatchMerging
    torch.manual_seed(7)
    m = PatchMerging(C, 2 * C, **kw)
    if isinstance(m.norm, nn.LayerNorm) and m.norm.elementwise_affine:
        with torch.no_grad():
            m.norm.weight.add_(0.2 * torch.randn_like(m.norm.weight))
            m.norm.bias.add_(0.1 * torch.randn_like(m.norm.bias))
    return m.to(gpu)


def _embed_module(gpu, C=32, **kw):
    from dhd_amd.swin import PatchEmbed
    torch.manual_seed(8)
    m = PatchEmbed(3, C, **kw)
    if isinstance(m.norm, nn.LayerNorm) and m.norm.elementwise_affine:
        with torch.no_grad():
            m.norm.weight.add_(0.2 * torch.randn_like(m.norm.weight))
            m.norm.bias.add_(0.1 * torch.randn_like(m.norm.bias))
    return m.to(gpu)


def _module_io(which):
    """-> (x, args after x, incoming gradient) on the CPU in float32: 9 x 13 tokens (padding on both axes) / an 18 x 26 image
    (padded to 20 x 28 by the patch size: 5 x 7 pixels, planes that start off a 16-byte boundary)."""
    gen = torch.Generator().manual_seed(21)
    if which == 'merge':
        return torch.randn(2, 9 * 13, 32, generator=gen) * 1.5 + 0.5, ((9, 13),), torch.randn(2, 5 * 7, 64, generator=gen)
    return torch.randn(2, 3, 18, 26, generator=gen), (), torch.randn(2, 5 * 7, 32, generator=gen)


def _run_module(m, x, args, gy):
    x = x.clone().requires_grad_()
    m.zero_grad()
    y = m(x, *args)
    y = y[0] if isinstance(y, tuple) else y
    y.backward(gy)
    lin = m.reduction if hasattr(m, 'reduction') else m.projection
    return dict(out=y.detach(), x_grad=x.grad, norm_w=m.norm.weight.grad.clone(), norm_b=m.norm.bias.grad.clone(), lin_w=lin.weight.grad.clone())


@pytest.mark.parametrize('which', ['merge', 'embed'])
def test_module_against_its_float64_twin(gpu, monkeypatch, which):
    _route_all(monkeypatch)
    m = (_merge_module if which == 'merge' else _embed_module)(gpu)
    m.fused_seam = True
    twin = copy.deepcopy(m).cpu().double()
    twin.fused_seam = False
    x, args, gy = _module_io(which)
    seen = _recorder(monkeypatch)
    got = _run_module(m, x.to(gpu), args, gy.to(gpu))
    _sync()
    assert seen.count(f'dhds_{which}_norm_forward') == 1 and seen.count(f'dhds_{which}_norm_backward') == 1
    ref = _run_module(twin, x.double(), args, gy.double())
    for k in ref:
        err = _err(got[k], ref[k])
        print(f'{which} module {k}: max error {err:.3e}, bound {BAR * SS.scale_of(ref[k]):.3e}')
        assert got[k].shape == ref[k].shape and err <= BAR * SS.scale_of(ref[k]), k
    # eval mode takes the same route
    del seen[:]
    m.eval()
    with torch.no_grad():
        y = m(x.to(gpu), *args)
    _sync()
    assert seen == [f'dhds_{which}_norm_forward'] and torch.equal(y[0] if isinstance(y, tuple) else y, got['out'])


@pytest.mark.parametrize('which', ['merge', 'embed'])
def test_module_under_bf16_autocast(gpu, monkeypatch, which):
    """Shape and dtype are today's; the error against float64 is at most 1.5 x the error of today's autocast path on the same
    inputs."""
    _route_all(monkeypatch)
    m = (_merge_module if which == 'merge' else _embed_module)(gpu)
    twin = copy.deepcopy(m).cpu().double()
    x, args, gy = _module_io(which)
    ref = _run_module(twin, x.double(), args, gy.double())
    res = {}
    seen = _recorder(monkeypatch)
    for on in (False, True):
        m.fused_seam = on
        with torch.autocast('cuda', dtype=BF16):
            xg = x.to(gpu).requires_grad_()
            m.zero_grad()
            y = m(xg, *args)
            y = y[0] if isinstance(y, tuple) else y
        y.backward(gy.to(gpu).to(y.dtype))
        _sync()
        res[on] = dict(out=y.detach(), x_grad=xg.grad, norm_w=m.norm.weight.grad.clone(), norm_b=m.norm.bias.grad.clone())
        assert (f'dhds_{which}_norm_forward' in seen) == on and (f'dhds_{which}_norm_backward' in seen) == on
    assert res[True]['out'].dtype == res[False]['out'].dtype == (BF16 if which == 'merge' else F32)
    for k in res[True]:
        a, b = res[True][k], res[False][k]
        ea, eb = _err(a, ref[k]), _err(b, ref[k])
        print(f'{which} module, bf16 autocast, {k}: error {ea:.3e} fused, {eb:.3e} today')
        assert a.shape == b.shape and a.dtype == b.dtype and ea <= 1.5 * eb, k


# ------------------------------------------------------------------------------------------------ 4. the whole backbone, G10

def _g10(gpu, on, **kw):
    import dhd_amd
    from test_host_logic import swin_from_fixture
    g = golden('g10_swin')
    net = swin_from_fixture(g, **kw).to(gpu)
    dhd_amd.fused_swin_seams(net, on)
    return g, net


def _g10_step(g, net, gpu):
    from dhd_amd import synthetic as syn
    x = torch.from_numpy(g['x']).to(gpu).requires_grad_()
    outs = net(x)
    ws = [torch.from_numpy(syn.hash_signed(2000 + i, tuple(o.shape))).to(gpu) for i, o in enumerate(outs)]
    sum((o * w).sum() for o, w in zip(outs, ws)).backward()
    _sync()
    return [o.detach() for o in outs], x.grad


def test_g10_with_the_switch_on(gpu, monkeypatch):
    """SwinTransformer on G10 within the bound tests/test_detector.py holds it to on the GPU (5e-5 relative to the maximum), through
    the four launching entry points: one embed and two merges, forward and backward."""
    _route_all(monkeypatch)
    g, net = _g10(gpu, True)
    seen = _recorder(monkeypatch)
    outs, xg = _g10_step(g, net, gpu)
    for i, o in enumerate(outs):
        ref = g[f'out{i}']
        err = np.abs(o.cpu().numpy() - ref).max()
        print(f'G10 out{i}: max error {err:.3e}, bound {5e-5 * max(1.0, np.abs(ref).max()):.3e}')
        assert err <= 5e-5 * max(1.0, np.abs(ref).max()), i
    err = np.abs(xg.cpu().numpy() - g['x_grad']).max()
    print(f'G10 x_grad: max error {err:.3e}, bound {5e-5 * np.abs(g["x_grad"]).max():.3e}')
    assert err <= 5e-5 * np.abs(g['x_grad']).max()
    assert seen.count('dhds_embed_norm_forward') == 1 and seen.count('dhds_merge_norm_forward') == 2
    assert seen.count('dhds_embed_norm_backward') == 1 and seen.count('dhds_merge_norm_backward') == 2
    assert not any(n.startswith(('dhdx', 'dhdf', 'dhdg')) for n in seen)     # a switch of its own
    del seen[:]
    with torch.no_grad():
        again = net(torch.from_numpy(g['x']).to(gpu))
    _sync()
    assert [n for n in seen if n.startswith('dhds')] == ['dhds_embed_norm_forward', 'dhds_merge_norm_forward', 'dhds_merge_norm_forward']
    assert all(torch.equal(a, b) for a, b in zip(again, outs))


# ------------------------------------------------------------------------------------------------ 5. every other call is today's path

def test_switch_off_is_todays_path(gpu, monkeypatch):
    from dhd_amd.swin import PatchEmbed, PatchMerging
    _route_all(monkeypatch)
    g, off = _g10(gpu, False)
    seen = _recorder(monkeypatch)
    got = _g10_step(g, off, gpu)
    assert not any(n.startswith('dhds') for n in seen)
    monkeypatch.setattr(PatchMerging, 'fused_seam', False)
    monkeypatch.setattr(PatchEmbed, 'fused_seam', False)
    from test_host_logic import swin_from_fixture
    never = swin_from_fixture(g).to(gpu)                                      # a model nobody switched
    assert not any('fused_seam' in vars(b) for b in never.modules())
    ref = _g10_step(g, never, gpu)
    assert all(torch.equal(a, b) for a, b in zip(got[0], ref[0])) and torch.equal(got[1], ref[1])


def _bits_of_both(m, x, args, gy, seen):
    res = {}
    for on in (False, True):
        m.fused_seam = on
        xg = x.clone().requires_grad_()
        m.zero_grad()
        y = m(xg, *args)
        y = y[0] if isinstance(y, tuple) else y
        y.backward(gy)
        _sync()
        res[on] = [y.detach(), xg.grad] + [p.grad.clone() for p in m.parameters()]
    assert not any(n.startswith('dhds') for n in seen), seen
    assert all(torch.equal(a, b) for a, b in zip(res[False], res[True]))


def test_an_unrouted_entry_is_todays_path(gpu, monkeypatch):
    from dhd_amd import swin_seam
    monkeypatch.setattr(swin_seam, 'ROUTED', {})
    seen = _recorder(monkeypatch)
    for which, make in (('merge', _merge_module), ('embed', _embed_module)):
        x, args, gy = _module_io(which)
        _bits_of_both(make(gpu), x.to(gpu), args, gy.to(gpu), seen)
    monkeypatch.setattr(swin_seam, 'ROUTED', {('merge', 32, F32, F32): False, ('embed', 32, F32, F32): False})
    for which, make in (('merge', _merge_module), ('embed', _embed_module)):
        x, args, gy = _module_io(which)
        _bits_of_both(make(gpu), x.to(gpu), args, gy.to(gpu), seen)


def test_an_unsupported_call_is_todays_path(gpu, monkeypatch):
    _route_all(monkeypatch)
    seen = _recorder(monkeypatch)
    gen = torch.Generator().manual_seed(33)
    rn = lambda *s: torch.randn(*s, generator=gen).to(gpu)
    # stride 3: 9 x 13 tokens -> 3 x 5 rows of 9C (13 % 3 = 1: padded, then cropped, as today)
    _bits_of_both(_merge_module(gpu, 8, stride=3), rn(2, 9 * 13, 8), ((9, 13),), rn(2, 3 * 4, 16), seen)
    # C = 12: no multiple of 8
    _bits_of_both(_merge_module(gpu, 12), rn(2, 9 * 13, 12), ((9, 13),), rn(2, 5 * 7, 24), seen)
    _bits_of_both(_embed_module(gpu, 12), rn(2, 3, 18, 26), (), rn(2, 5 * 7, 12), seen)
    # no norm
    _bits_of_both(_merge_module(gpu, 32, norm=False), rn(2, 9 * 13, 32), ((9, 13),), rn(2, 5 * 7, 64), seen)
    _bits_of_both(_embed_module(gpu, 32, norm=False), rn(2, 3, 18, 26), (), rn(2, 5 * 7, 32), seen)
    # a norm without affine parameters, and one without a bias
    for kw in (dict(elementwise_affine=False), dict(bias=False)):
        m = _merge_module(gpu, 32)
        m.norm = nn.LayerNorm(128, **kw).to(gpu)
        _bits_of_both(m, rn(2, 9 * 13, 32), ((9, 13),), rn(2, 5 * 7, 64), seen)
        e = _embed_module(gpu, 32)
        e.norm = nn.LayerNorm(32, **kw).to(gpu)
        _bits_of_both(e, rn(2, 3, 18, 26), (), rn(2, 5 * 7, 32), seen)
    # and the control: the same modules as they come do take the operators
    _route_all(monkeypatch)
    m = _merge_module(gpu, 32)
    m.fused_seam = True
    m(rn(2, 9 * 13, 32), (9, 13))
    e = _embed_module(gpu, 32)
    e.fused_seam = True
    e(rn(2, 3, 18, 26))
    _sync()
    assert seen[-2:] == ['dhds_merge_norm_forward', 'dhds_embed_norm_forward']


def test_swin_seam_supported(gpu):
    from dhd_amd import swin_seam_supported
    tok = torch.empty(2, 35, 128, device=gpu)
    img = torch.empty(2, 128, 5, 7, device=gpu)
    assert swin_seam_supported(tok, 'merge') and swin_seam_supported(tok, 'merge', BF16) and swin_seam_supported(tok.to(F16), 'merge', F32)
    assert swin_seam_supported(img, 'embed') and swin_seam_supported(img.to(BF16), 'embed', F32)
    assert swin_seam_supported(torch.empty(1, 4, 512, device=gpu), 'merge') and not swin_seam_supported(torch.empty(1, 4, 520, device=gpu), 'merge')
    assert swin_seam_supported(torch.empty(1, 256, 2, 2, device=gpu), 'embed') and not swin_seam_supported(torch.empty(1, 264, 2, 2, device=gpu), 'embed')
    assert not swin_seam_supported(torch.empty(2, 35, 12, device=gpu), 'merge') and not swin_seam_supported(tok.cpu(), 'merge')
    assert not swin_seam_supported(tok.double(), 'merge') and not swin_seam_supported(tok, 'merge', torch.float64)
    assert not swin_seam_supported(tok, 'embed') and not swin_seam_supported(torch.empty(0, 128, 5, 7, device=gpu), 'embed')
    with pytest.raises(ValueError):
        swin_seam_supported(tok, 'norm')


def test_a_channels_last_map_goes_to_layer_norm_rows_as_it_lies(gpu, monkeypatch):
    """patch_embed_norm on a map that is dense in channels_last memory: its token view is contiguous, so the existing row
    operator takes it where it lies -- no copy, and not the kernel of this family."""
    import dhd_amd
    kind, case, prec = 'embed', 'two_images_c128', 'f32_bf16'
    v = _on(gpu, kind, case, prec)
    x = v['x'].contiguous(memory_format=torch.channels_last)
    assert not x.is_contiguous()
    seen = _recorder(monkeypatch)
    made = []
    real = dhd_amd._lib.dense16

    def dense16(t, *a, **k):
        out = real(t, *a, **k)
        made.append((t.data_ptr(), out))
        return out
    monkeypatch.setattr(dhd_amd._lib, 'dense16', dense16)
    y = dhd_amd.patch_embed_norm(x, v['gamma'], v['beta'], SS.EPS, F32)
    _sync()
    assert seen == ['dhdx_ln_rows_forward']
    assert any(src == x.data_ptr() and out.data_ptr() == x.data_ptr() for src, out in made)      # read where it lies
    Y64 = SS.twin(kind, case, prec)[0]
    assert _err(y, Y64) <= BAR * SS.scale_of(Y64)


# ------------------------------------------------------------------------------------------------ 6. checkpointing

def test_checkpointing_a_stage_with_a_merge_changes_nothing(gpu, monkeypatch):
    from torch.utils.checkpoint import checkpoint
    _route_all(monkeypatch)
    g, net = _g10(gpu, True)
    stage = net.stages[0]
    assert stage.downsample is not None and stage.downsample.fused_seam
    gen = torch.Generator().manual_seed(5)
    x0 = torch.randn(2, 13 * 19, 16, generator=gen).to(gpu)
    gy = torch.randn(2, 7 * 10, 32, generator=gen).to(gpu)
    seen = _recorder(monkeypatch)
    res = []
    for cp in (False, True):
        x = x0.clone().requires_grad_()
        stage.zero_grad()
        out = checkpoint(stage, x, (13, 19), use_reentrant=False) if cp else stage(x, (13, 19))
        assert out[1] == (7, 10)
        out[0].backward(gy)
        _sync()
        n = stage.downsample.norm
        res.append((out[0].detach(), x.grad, n.weight.grad.clone(), n.bias.grad.clone(), stage.downsample.reduction.weight.grad.clone()))
    assert seen.count('dhds_merge_norm_forward') == 3 and seen.count('dhds_merge_norm_backward') == 2     # the recomputation is the third
    assert all(torch.equal(a, b) for a, b in zip(*res))


# ------------------------------------------------------------------------------------------------ 7. graph capture

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
    with torch.no_grad():
        for kind, case in (('merge', 'odd_h_c128'), ('embed', 'two_images_c128')):
            v = _on(gpu, kind, case, 'f32_bf16')
            _capture(lambda x: _op(kind, case, x, v['gamma'], v['beta'], BF16), v['x'].clone(), v['x'].flip(0 if kind == 'embed' else 1).flip(-1).contiguous())


# ------------------------------------------------------------------------------------------------ 8. views

VIEW_CASES = {'merge': 'even_c96', 'embed': 'c96'}
VIEW_PREC = 'f32_bf16'
VIEWS = [pytest.param(k, t, kind, id=f'{k}-{t}-{kind}') for k in ('merge', 'embed')
         for t, kinds in (('x', ('offset_elem', 'inner_step2')), ('dy', ('offset_elem', 'inner_step2', 'expanded'))) for kind in kinds]
_fresh = {}


def _seam_run(c, v, kind, case, prec, const=()):
    """Forward and backward; c (test_gpu_views.Case) presents x or dy as a view."""
    dy = torch.full_like(v['dy'], 0.5) if 'dy' in const else v['dy']
    x, gam, bet = c.inp('x', v['x'], grad=True), v['gamma'].clone().requires_grad_(), v['beta'].clone().requires_grad_()
    y = _op(kind, case, x, gam, bet, SS.precisions(kind)[prec][1])
    c.grad('dy', y).backward(dy)
    _sync()
    return dict(y=y.detach(), dx=x.grad, dgamma=gam.grad, dbeta=bet.grad)


@pytest.mark.parametrize('kind,target,how', VIEWS)
def test_views(gpu, kind, target, how):
    case = VIEW_CASES[kind]
    v = _on(gpu, kind, case, VIEW_PREC)
    const = (target,) if how == 'expanded' else ()
    if (kind, const) not in _fresh:
        _fresh[kind, const] = _seam_run(Case(None, 'fresh'), v, kind, case, VIEW_PREC, const)
    c = Case(target, how)
    got = _seam_run(c, v, kind, case, VIEW_PREC, const)
    assert len(c.parents) == 1                                                # the tensor was presented as a view
    for k, ref in _fresh[kind, const].items():
        assert got[k].shape == ref.shape and got[k].dtype == ref.dtype and torch.equal(got[k], ref), k
    assert c.untouched(), 'a parent buffer changed: the view was written to, or something wrote outside it'
    for name, t in c.shown.items():
        if t.requires_grad:
            assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == t.dtype, name


# ------------------------------------------------------------------------------------------------ 9. guard bands

GUARDED = ([pytest.param(k, c, 'f32_bf16', id=f'{k}-{c}-f32_bf16') for k in ('merge', 'embed') for c in SS.CASES[k]]
           + [pytest.param(k, c, 'bf16', id=f'{k}-{c}-bf16') for k in ('merge', 'embed') for c in SS.CASES[k]])


@pytest.mark.parametrize('kind,case,prec', GUARDED)
def test_inside_guard_bands(gpu, monkeypatch, kind, case, prec):
    """Plain, then with every buffer the wrappers allocate between two 4096-byte guard bands at its exact size, every byte 0xFF,
    then 0x00: no guard byte changes, the three runs agree, and nothing uninitialised is read (0xFF is NaN in every float type)."""
    v = _on(gpu, kind, case, prec)
    snap = {k: t.clone() for k, t in v.items()}
    plain = _seam_run(Case(None, 'fresh'), v, kind, case, prec)
    for fill in (0xFF, 0x00):
        with G.guarded(monkeypatch, fill) as ledger:
            got = _seam_run(Case(None, 'fresh'), v, kind, case, prec)
            ledger.check()
            got = {k: t.detach().clone() for k, t in got.items()}
        inside = ledger.sites_under(G.PRODUCT_ROOT)
        ours = [e for e in inside if 'swin_seam.py' in e.site]
        print(f'{kind} {case} [{prec}, fill {fill:#04x}]: {len(ledger)} guarded allocations, {ledger.total_bytes()} bytes, guards intact')
        assert len(inside) == len(ledger) == len(ours) == 5                   # out; dx, dgamma, dbeta, scratch
        for k, ref in plain.items():
            assert int((torch.isfinite(ref) & ~torch.isfinite(got[k])).sum()) == 0, (k, fill)
            assert torch.equal(got[k], ref), (k, fill)
    for k, s in snap.items():
        assert torch.equal(v[k], s), f'input {k} changed'
