"""The Swin glue operators (dhd_amd/swin_glue.py, csrc/swin_glue.hip) on the GPU: against the float64 twin of
tests/swin_glue_inputs.py, inside `SwinBlock` / `SwinTransformer` on the G10 fixture, on views, and inside guard bands.

Bounds.  Float32 results are held to the project's layer bar, |y - Y64| <= 1e-4 max(1, |Y64|max).  A half result of the forward
needs no tolerance: it must equal the operator's own float32 result cast to that type.  Where a gradient is stored in a half type
(dx for bfloat16 x, dwin for half windows) the stored value is the float32 result rounded once more, so its bound adds one unit
roundoff of that type relative to the exact value, u = 2^-8 (bfloat16: 8 significant bits) or 2^-11 (float16: 11 bits), plus
2^-25 for float16, half the spacing of its subnormals (a gradient smaller than 2^-14 is rounded on that grid).
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as G  # noqa: E402
import swin_glue_inputs as SG  # noqa: E402
from conftest import golden  # noqa: E402
from test_gpu_views import Case  # noqa: E402  (present() behind Case.inp / Case.grad: tensors carved out of poisoned parents)

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
UNIT = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}
TINY = {F32: 0.0, F16: 2.0 ** -25, BF16: 0.0}
BAR = 1e-4
pytestmark = pytest.mark.gpu
GRID = [pytest.param(c, p, id=f'{c}-{p}') for c in SG.CASES for p in SG.PRECISIONS]
WGRID = [pytest.param(c, p, id=f'{c}-{p}') for c in SG.WINDOW_CASES for p in SG.PRECISIONS]


def _sync():
    """Wait for the device; after a device error nothing more is started in this module."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'GPU fault, stopping the module: {e}', returncode=3)


def _on(gpu, case, prec):
    return {k: t.to(gpu) for k, t in SG.inputs(case, prec).items()}


def _err(got, ref64):
    return float((got.detach().cpu().double() - ref64).abs().max())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _recorder(monkeypatch):
    """The names that reach dhd_amd._lib.check: every dhd_* call of swin.py and every dhdx_* call goes through it."""
    from dhd_amd import _ext, _lib
    _ext.load()
    seen, real = [], _lib.check

    def check(rc, what):
        seen.append(what)
        return real(rc, what)
    monkeypatch.setattr(_lib, 'check', check)
    return seen


# ------------------------------------------------------------------------------------------------ 1. forward

@pytest.mark.parametrize('case,prec', GRID)
def test_forward_against_the_float64_twin(gpu, case, prec):
    from dhd_amd import layer_norm_rows
    v, (xdt, odt) = _on(gpu, case, prec), SG.PRECISIONS[prec]
    win = SG.window_arg(case)
    y32 = layer_norm_rows(v['x'], v['gamma'], v['beta'], SG.EPS, F32, win)
    _sync()
    Y64 = SG.ln_twin(case, prec)[0]
    err = _err(y32, Y64)
    print(f'{case} [{prec}]: max |y - Y64| = {err:.3e}, bound {BAR * SG.scale_of(Y64):.3e}')
    assert tuple(y32.shape) == SG.out_shape(case) and y32.dtype == F32
    assert err <= BAR * SG.scale_of(Y64)
    pad = SG.pad_rows(case).to(gpu) if win else None
    if win:
        assert bool((_bits(y32)[pad] == 0).all())                           # exact zeros, not -0 and not beta
        assert bool((y32[~pad].abs().sum(-1) > 0).all())
    if odt != F32:
        y = layer_norm_rows(v['x'], v['gamma'], v['beta'], SG.EPS, odt, win)
        _sync()
        assert y.dtype == odt and torch.equal(y, y32.to(odt))
        if win:
            assert bool((_bits(y)[pad] == 0).all())
    if xdt == odt:                                                           # the default result dtype is x's
        assert layer_norm_rows(v['x'], v['gamma'], v['beta'], SG.EPS, window=win).dtype == xdt


# ------------------------------------------------------------------------------------------------ 2. backward

def _ln_grads(v, case, prec, dy):
    from dhd_amd import layer_norm_rows
    x, g, b = (v[k].clone().requires_grad_() for k in ('x', 'gamma', 'beta'))
    y = layer_norm_rows(x, g, b, SG.EPS, SG.PRECISIONS[prec][1], SG.window_arg(case))
    y.backward(dy)
    _sync()
    return x.grad, g.grad, b.grad


@pytest.mark.parametrize('case,prec', GRID)
def test_backward_against_the_twins_autograd(gpu, case, prec):
    v, (xdt, odt) = _on(gpu, case, prec), SG.PRECISIONS[prec]
    dx, dg, db = _ln_grads(v, case, prec, v['dy'])
    _, DX, DG, DB = SG.ln_twin(case, prec)
    assert dx.dtype == xdt and dx.shape == v['x'].shape and dg.dtype == F32 and db.dtype == F32 and dg.shape == db.shape == v['gamma'].shape
    print(f'{case} [{prec}]: max |dx - DX| = {_err(dx, DX):.3e} (|DX|max {float(DX.abs().max()):.3e}), |dgamma - DG| = {_err(dg, DG):.3e} '
          f'(|DG|max {float(DG.abs().max()):.3e}), |dbeta - DB| = {_err(db, DB):.3e} (|DB|max {float(DB.abs().max()):.3e})')
    assert _err(dg, DG) <= BAR * SG.scale_of(DG) and _err(db, DB) <= BAR * SG.scale_of(DB)
    if xdt == F32:
        assert _err(dx, DX) <= BAR * SG.scale_of(DX)
    else:       # dx is stored in x's half type: the float32 result, rounded once more
        assert bool(((dx.cpu().double() - DX).abs() <= BAR * SG.scale_of(DX) + UNIT[xdt] * DX.abs() + TINY[xdt]).all())
    # no atomics: a second run gives the same bytes
    again = _ln_grads(v, case, prec, v['dy'])
    assert all(torch.equal(a, b) for a, b in zip((dx, dg, db), again))
    # the pad rows of dy are never read
    if SG.window_arg(case):
        pad = SG.pad_rows(case).to(gpu)
        dy = v['dy'].clone()
        dy[pad] = float('nan')
        assert bool(pad.any()) == bool(torch.isnan(dy).any())
        poisoned = _ln_grads(v, case, prec, dy)
        assert all(torch.equal(a, b) for a, b in zip((dx, dg, db), poisoned))


# ------------------------------------------------------------------------------------------------ 3. reverse + add

@pytest.mark.parametrize('case,prec', WGRID)
def test_reverse_add(gpu, case, prec):
    from dhd_amd import window_reverse_add
    from dhd_amd.swin import _WindowRows
    v = _on(gpu, case, prec)
    B, H, W, ws, sh, C = SG.CASES[case]
    win, ident, gout = v['win'], v['x'], SG.reverse_add_gout(case, prec).to(gpu)
    out = window_reverse_add(win, ident, H, W, ws, sh)
    _sync()
    ref = (ident + _WindowRows.apply(win, H, W, ws, sh, True, win.dtype).view(B, H * W, C).float()).to(ident.dtype)
    assert out.shape == ident.shape and out.dtype == ident.dtype and torch.equal(out, ref)
    for scaled in (False, True):
        O64, DW, DI = SG.reverse_add_twin(case, prec, scaled)
        w_, i_ = win.clone().requires_grad_(), ident.clone().requires_grad_()
        o = window_reverse_add(w_, i_, H, W, ws, sh, v['scale'] if scaled else None)
        o.backward(gout)
        _sync()
        # two float32 roundings (the product, the sum), and one more where identity's type is a half type
        moved = (O64 - ident.cpu().double()).abs()                           # |scale * reverse(win)|
        bound = 2 * UNIT[F32] * (ident.cpu().double().abs() + moved) + (UNIT[ident.dtype] * O64.abs() + TINY[ident.dtype] if ident.dtype != F32 else 0)
        assert bool(((o.detach().cpu().double() - O64).abs() <= bound).all()), _err(o, O64)
        # identity's gradient is the incoming gradient; win's is its partition in win's dtype (one rounding where the type narrows)
        # times scale (one more)
        assert torch.equal(i_.grad, gout) and torch.equal(i_.grad.cpu().double(), DI)
        roundings = (gout.dtype != win.dtype) + scaled
        assert w_.grad.dtype == win.dtype and w_.grad.shape == win.shape
        assert bool(((w_.grad.cpu().double() - DW).abs() <= roundings * (1.01 * UNIT[win.dtype] * DW.abs() + TINY[win.dtype])).all()), _err(w_.grad, DW)
        if scaled and B > 1:
            assert bool((w_.grad[1] == 0).all()) and torch.equal(o.detach()[1], ident[1])      # scale 0: the dropped image


# ------------------------------------------------------------------------------------------------ 4./5. inside the model, G10

def _g10(gpu, on, **kw):
    import dhd_amd
    from test_host_logic import swin_from_fixture
    g = golden('g10_swin')
    net = swin_from_fixture(g, **kw).to(gpu)
    dhd_amd.fused_swin_glue(net, on)
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
    the three new entry points; a forward without grad cuts and reverses no window through dhd_window_rows."""
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
    assert {'dhdx_ln_rows_forward', 'dhdx_ln_rows_backward', 'dhdx_window_reverse_add'} <= set(seen)
    # per block norm1 and the add; norm2 of a small float32 map has no cast to fuse and is routed to torch (swin_glue_supported)
    assert seen.count('dhdx_ln_rows_forward') == 6 and seen.count('dhdx_window_reverse_add') == 6
    assert seen.count('dhdx_ln_rows_backward') == 6 and seen.count('dhd_window_rows') == 6               # the add's backward: a partition
    del seen[:]
    with torch.no_grad():
        again = net(torch.from_numpy(g['x']).to(gpu))
    _sync()
    assert 'dhd_window_rows' not in seen and seen.count('dhdx_ln_rows_forward') == 6
    assert all(torch.equal(a, b) for a, b in zip(again, outs))


def test_one_block_against_todays_block_in_float64(gpu):
    """A shifted SwinBlock of G10 (13 x 19 tokens, window 4: padding on both axes) with the switch on, output and input gradient,
    against the same block's unfused formulation on the CPU in float64."""
    g, net = _g10(gpu, True)
    block = net.stages[0].blocks[1]
    assert block.attn.shift_size > 0 and block.fused_glue
    twin = copy.deepcopy(block).cpu().double()
    twin.fused_glue = False
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 13 * 19, 16, generator=gen)
    gy = torch.randn(2, 13 * 19, 16, generator=gen)
    xa, xb = x.to(gpu).requires_grad_(), x.double().requires_grad_()
    ya, yb = block(xa, (13, 19)), twin(xb, (13, 19))
    ya.backward(gy.to(gpu))
    yb.backward(gy.double())
    _sync()
    for name, a, b in (('out', ya, yb), ('x_grad', xa.grad, xb.grad), ('norm1.weight.grad', block.norm1.weight.grad, twin.norm1.weight.grad),
                       ('norm2.bias.grad', block.norm2.bias.grad, twin.norm2.bias.grad)):
        err, top = _err(a, b.detach()), float(b.detach().abs().max())
        print(f'block {name}: max error {err:.3e}, bound {5e-5 * max(1.0, top):.3e}')
        assert err <= 5e-5 * max(1.0, top), name


def test_under_bf16_autocast(gpu, monkeypatch):
    """The windows WindowMSA receives are the float32 LayerNorm rows rounded once to bfloat16, and the block's output keeps the
    dtype it has today."""
    from dhd_amd import layer_norm_rows
    g, net = _g10(gpu, True)
    _, plain = _g10(gpu, False)
    took = {}
    for name, m in (('on', net), ('off', plain)):
        block = m.stages[0].blocks[1]
        block.register_forward_pre_hook(lambda mod, args, name=name: took.__setitem__(name + '_in', (args[0].detach().clone(), args[1])))
        block.register_forward_hook(lambda mod, args, out, name=name: took.__setitem__(name + '_out', out.detach()))
        block.attn.w_msa.register_forward_pre_hook(lambda mod, args, name=name: took.__setitem__(name + '_win', args[0].detach().clone()))
    x = torch.from_numpy(g['x']).to(gpu)
    seen = _recorder(monkeypatch)
    with torch.no_grad(), torch.autocast('cuda', dtype=BF16):
        outs = net(x)
        assert seen.count('dhdx_ln_rows_forward') == 12      # norm2 as well: it emits the bfloat16 fc1 reads
        ref = plain(x)
    _sync()
    block = net.stages[0].blocks[1]
    x_in, (H, W) = took['on_in']
    want = layer_norm_rows(x_in, block.norm1.weight, block.norm1.bias, block.norm1.eps, F32,
                           (H, W, block.attn.window_size, block.attn.shift_size)).to(BF16)
    assert took['on_win'].dtype == BF16 and torch.equal(took['on_win'], want)
    assert took['on_out'].dtype == took['off_out'].dtype == F32 and took['on_win'].dtype == took['off_win'].dtype
    assert all(a.dtype == b.dtype and a.shape == b.shape for a, b in zip(outs, ref))


def test_switch_off_is_todays_path(gpu, monkeypatch):
    from dhd_amd.swin import SwinBlock
    g, off = _g10(gpu, False)
    seen = _recorder(monkeypatch)
    got = _g10_step(g, off, gpu)
    assert not any(n.startswith('dhdx') for n in seen) and seen.count('dhd_window_rows') == 24
    monkeypatch.setattr(SwinBlock, 'fused_glue', False)
    from test_host_logic import swin_from_fixture
    never = swin_from_fixture(g).to(gpu)                                      # a model nobody switched
    assert not any('fused_glue' in vars(b) for b in never.modules())
    ref = _g10_step(g, never, gpu)
    assert all(torch.equal(a, b) for a, b in zip(got[0], ref[0])) and torch.equal(got[1], ref[1])


def test_a_small_layer_norm_with_nothing_to_fuse_is_routed_to_torch(gpu):
    """swin_glue_supported(x, plain_ln_to=dtype): the identity-map form into the dtype nn.LayerNorm emits anyway (x's, or float32
    under autocast) on a map below PLAIN_LN_MIN_NUMEL elements goes to today's path (the measurement that decided it is in
    dhd_amd/swin_glue.py); everything else is taken -- under bf16 autocast every norm2, whatever the stage's token dtype."""
    from dhd_amd.swin_glue import PLAIN_LN_MIN_NUMEL, swin_glue_supported
    small = torch.empty(2, 64, 128, device=gpu)
    big = torch.empty(1, PLAIN_LN_MIN_NUMEL // 1024, 1024, device=gpu)
    assert swin_glue_supported(small) and swin_glue_supported(small, plain_ln_to=BF16) and not swin_glue_supported(small, plain_ln_to=F32)
    assert swin_glue_supported(big, plain_ln_to=F32) and swin_glue_supported(big[:, 1:], plain_ln_to=F32) is False
    assert not swin_glue_supported(small.to(BF16), plain_ln_to=BF16)
    with torch.autocast('cuda', dtype=BF16):
        assert swin_glue_supported(small, plain_ln_to=BF16) and swin_glue_supported(small.to(BF16), plain_ln_to=BF16)
        assert not swin_glue_supported(small, plain_ln_to=F32)
    assert not swin_glue_supported(torch.empty(2, 64, 12, device=gpu)) and not swin_glue_supported(small.cpu())


# ------------------------------------------------------------------------------------------------ 6. determinism and capture

def test_checkpointing_changes_nothing(gpu):
    g, a = _g10(gpu, True)
    _, b = _g10(gpu, True)
    for st in b.stages:
        st.with_cp = True
    (oa, ga), (ob, gb) = _g10_step(g, a, gpu), _g10_step(g, b, gpu)
    assert all(torch.equal(p, q) for p, q in zip(oa, ob)) and torch.equal(ga, gb)
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    for k in pa:
        if '.norm1.' in k or '.norm2.' in k:
            assert pa[k].grad is not None and torch.equal(pa[k].grad, pb[k].grad), k


def test_droppath_draws_what_it_drew(gpu):
    """Training with an active DropPath: the fused route draws the same random tensor with the same call, so the generator ends
    in the same state, and the same images are dropped: the step agrees with the unfused one to the G10 bound."""
    res = {}
    for on in (False, True):
        g, net = _g10(gpu, on)
        net.train()
        assert net.stages[2].blocks[1].attn.drop.drop_prob > 0
        torch.manual_seed(1234)
        torch.cuda.manual_seed(1234)
        outs, xg = _g10_step(g, net, gpu)
        res[on] = (outs, xg, torch.cuda.get_rng_state(gpu).clone())
    assert torch.equal(res[False][2], res[True][2])
    for a, b in zip(res[True][0] + [res[True][1]], res[False][0] + [res[False][1]]):
        assert _err(a, b.cpu().double()) <= 5e-5 * SG.scale_of(b)


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
    from dhd_amd import layer_norm_rows, window_reverse_add
    case, prec = 'ws12_c128', 'f32_bf16'
    v = _on(gpu, case, prec)
    B, H, W, ws, sh, C = SG.CASES[case]
    with torch.no_grad():
        _capture(lambda x: layer_norm_rows(x, v['gamma'], v['beta'], SG.EPS, BF16, (H, W, ws, sh)), v['x'].clone(), v['x'].flip(1).contiguous())
        _capture(lambda x: layer_norm_rows(x, v['gamma'], v['beta'], SG.EPS, BF16), v['x'].clone(), v['x'].flip(1).contiguous())
        _capture(lambda w: window_reverse_add(w, v['x'], H, W, ws, sh, v['scale']), v['win'].clone(), v['win'].flip(2).contiguous())


# ------------------------------------------------------------------------------------------------ 7. views

VIEW_CASE, VIEW_PREC = 'pad_shift_c96', 'f32_bf16'
VIEWS = [pytest.param(t, k, id=f'{t}-{k}') for t, kinds in (('x', ('offset_elem', 'inner_step2')), ('dy', ('offset_elem', 'inner_step2', 'expanded')),
                                                             ('win', ('offset_elem', 'inner_step2')), ('identity', ('offset_elem', 'inner_step2')),
                                                             ('gout', ('offset_elem', 'expanded')))
         for k in kinds]
_fresh = {}


def _glue_run(c, v, case, prec, const=()):
    """Both operators forward and backward; c (test_gpu_views.Case) presents one of x, dy, win, identity, gout as a view."""
    from dhd_amd import layer_norm_rows, window_reverse_add
    B, H, W, ws, sh, C = SG.CASES[case]
    dy = torch.full_like(v['dy'], 0.5) if 'dy' in const else v['dy']
    x, gam, bet = c.inp('x', v['x'], grad=True), v['gamma'].clone().requires_grad_(), v['beta'].clone().requires_grad_()
    y = layer_norm_rows(x, gam, bet, SG.EPS, SG.PRECISIONS[prec][1], SG.window_arg(case))
    c.grad('dy', y).backward(dy)
    res = dict(y=y.detach(), dx=x.grad, dgamma=gam.grad, dbeta=bet.grad)
    if ws:
        gout = v['gout'] if 'gout' not in const else torch.full_like(v['gout'], 0.5)
        win, ident = c.inp('win', v['win'], grad=True), c.inp('identity', v['x'], grad=True)
        out = window_reverse_add(win, ident, H, W, ws, sh, v['scale'])
        c.grad('gout', out).backward(gout)
        res.update(out=out.detach(), dwin=win.grad, didentity=ident.grad)
    _sync()
    return res


@pytest.mark.parametrize('target,kind', VIEWS)
def test_views(gpu, target, kind):
    v = _on(gpu, VIEW_CASE, VIEW_PREC)
    v['gout'] = SG.reverse_add_gout(VIEW_CASE, VIEW_PREC).to(gpu)
    const = (target,) if kind == 'expanded' else ()
    if const not in _fresh:
        _fresh[const] = _glue_run(Case(None, 'fresh'), v, VIEW_CASE, VIEW_PREC, const)
    case = Case(target, kind)
    got = _glue_run(case, v, VIEW_CASE, VIEW_PREC, const)
    assert len(case.parents) == 1                                             # the tensor was presented as a view
    for k, ref in _fresh[const].items():
        assert got[k].shape == ref.shape and got[k].dtype == ref.dtype and torch.equal(got[k], ref), k
    assert case.untouched(), 'a parent buffer changed: the view was written to, or something wrote outside it'
    for name, t in case.shown.items():
        if t.requires_grad:
            assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == t.dtype, name


# ------------------------------------------------------------------------------------------------ 8. guard bands

GUARDED = [pytest.param(c, 'f32_bf16', id=f'{c}-f32_bf16') for c in SG.CASES] + [pytest.param('ws12_c128', 'bf16', id='ws12_c128-bf16'),
                                                                                   pytest.param('one_token_cmax', 'f32', id='one_token_cmax-f32')]


@pytest.mark.parametrize('case,prec', GUARDED)
def test_inside_guard_bands(gpu, monkeypatch, case, prec):
    """Plain, then with every buffer the wrappers allocate between two 4096-byte guard bands at its exact size, every byte 0xFF,
    then 0x00: no guard byte changes, the three runs agree, and nothing uninitialised is read (0xFF is NaN in every float type)."""
    v = _on(gpu, case, prec)
    v['gout'] = SG.reverse_add_gout(case, prec).to(gpu)
    snap = {k: t.clone() for k, t in v.items()}
    plain = _glue_run(Case(None, 'fresh'), v, case, prec)
    for fill in (0xFF, 0x00):
        with G.guarded(monkeypatch, fill) as ledger:
            got = _glue_run(Case(None, 'fresh'), v, case, prec)
            ledger.check()
            got = {k: t.detach().clone() for k, t in got.items()}
        inside = ledger.sites_under(G.PRODUCT_ROOT)
        ours = [e for e in inside if 'swin_glue.py' in e.site]
        print(f'{case} [{prec}, fill {fill:#04x}]: {len(ledger)} guarded allocations, {ledger.total_bytes()} bytes, guards intact')
        # out; dx, dgamma, dbeta, scratch; reverse + add's out -- and the partition of its backward, allocated in swin.py
        assert len(inside) == len(ledger) and len(ours) == (6 if SG.window_arg(case) else 5) and len(ledger) == len(ours) + bool(SG.window_arg(case))
        for k, ref in plain.items():
            assert int((torch.isfinite(ref) & ~torch.isfinite(got[k])).sum()) == 0, (k, fill)
            assert torch.equal(got[k], ref), (k, fill)
    for k, s in snap.items():
        assert torch.equal(v[k], s), f'input {k} changed'
