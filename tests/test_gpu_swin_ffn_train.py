"""The Swin FFN training operator (dhd_amd.swin_ffn, csrc/swin_ffn_train.h) on the GPU: forward and every gradient against the
float64 autograd twin of tests/swin_ffn_train_inputs.py at every case, dtype combination and scale setting; a dropped image,
repeatability, row independence, guard bands, the NULL operand triple, the routed SwinBlock and the composed backbone.

Bars.  GEMMs in float32 (bf16x3): out within 1e-4 max(1, |ref|max) of the twin and each gradient within 1e-4 max(1, |G|max) of its
own twin tensor, the project's layer bar.  GEMMs in a half type: the parent formulation (torch autograd over layer_norm / linear
/ gelu / linear / scale / add in the same dtypes on the same tensors) is run in the same test and its error against the twin
taken tensor by tensor; the fused error may be at most 1.5 x that, the project's existing margin."""
import copy
import os
import sys

import pytest
import torch
from torch.utils.checkpoint import checkpoint

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as G  # noqa: E402
import swin_ffn_train_inputs as ST  # noqa: E402

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
BAR, MARGIN = 1e-4, 1.5
pytestmark = pytest.mark.gpu
GRID = [pytest.param(c, p, s, id=f'{c}-{p}-{s}') for c, p, s in ST.GRID]
FWD, BWD = 'dhdt_swin_ffn_forward', 'dhdt_swin_ffn_backward'


def _sync():
    """Wait for the device; after a device error nothing more is started in this module."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'GPU fault, stopping the module: {e}', returncode=3)


def _on(gpu, case, prec):
    return {k: t.to(gpu) for k, t in ST.inputs(case, prec).items()}


def _scale(gpu, name):
    s = ST.scale_tensor(name)
    return None if s is None else s.to(gpu)


def _err(got, ref64):
    return float((got.detach().cpu().double() - ref64).abs().max())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _step(v, mdt, scale):
    """Forward and backward of the operator on fresh leaves -> the twin's dict."""
    import dhd_amd
    leaves = {k: v[k].detach().clone().requires_grad_() for k in ('x',) + ST.PARAMS}
    out = dhd_amd.swin_ffn(leaves['x'], leaves['gamma'], leaves['beta'], ST.EPS, leaves['w1'], leaves['b1'], leaves['w2'], leaves['b2'], mdt, scale)
    _sync()
    out.backward(v['dout'])
    _sync()
    return ST._collect(out, leaves)


def _backward(v, mdt, scale, operands=True, x=None, dout=None):
    from dhd_amd.swin_ffn import swin_ffn_backward
    got = swin_ffn_backward(v['x'] if x is None else x, v['dout'] if dout is None else dout, v['gamma'], v['beta'], ST.EPS, v['w1'], v['b1'],
                            v['w2'], mdt, scale, operands)
    _sync()
    return dict(zip(('dx', 'dgamma', 'dbeta', 'xn', 'act', 'dhid'), got))


def _recorder(monkeypatch):
    """The names that reach dhd_amd._lib.check: every entry point of every family goes through it."""
    from dhd_amd import _ffn, _ffn_train, _lib
    _ffn.load()
    _ffn_train.load()
    seen, real = [], _lib.check

    def check(rc, what):
        seen.append(what)
        return real(rc, what)
    monkeypatch.setattr(_lib, 'check', check)
    return seen


def _route_everything(monkeypatch):
    """The routing table as if every entry had won its measurement: these tests are about the route, not about which sizes take it."""
    from dhd_amd import swin_ffn
    monkeypatch.setattr(swin_ffn, 'ROUTED_TRAIN', {k: True for k in swin_ffn.ROUTED_TRAIN})


# ------------------------------------------------------------------------------------------------ 1. against the twin

@pytest.mark.parametrize('case,prec,sname', GRID)
def test_operator_against_the_float64_twin(gpu, case, prec, sname):
    from dhd_amd import swin_ffn_infer
    v, (xdt, mdt), scale = _on(gpu, case, prec), ST.PRECISIONS[prec], _scale(gpu, sname)
    got, ref = _step(v, mdt, scale), ST.twin(case, prec, sname)
    if scale is None:                                                          # without a factor: the inference operator's bytes
        infer = swin_ffn_infer(v['x'], v['gamma'], v['beta'], ST.EPS, v['w1'], v['b1'], v['w2'], v['b2'], mdt)
        _sync()
        assert _same(got['out'], infer)
    par = None
    if mdt != F32:
        par = ST.parent(v, xdt, mdt, scale, 'cuda')
        _sync()
    failures = []
    for k in ST.TENSORS:
        want_dt = xdt if k in ('out', 'dx') else v[k[1:]].dtype
        assert got[k].dtype == want_dt and tuple(got[k].shape) == tuple(ref[k].shape), k
        err, size = _err(got[k], ref[k]), ST.scale_of(ref[k])
        if par is None:
            print(f'{case} [{prec}, {sname}] {k}: max |fused - twin| = {err:.3e}, bound {BAR * size:.3e}')
            ok = err <= BAR * size
        else:
            perr = _err(par[k], ref[k])
            print(f'{case} [{prec}, {sname}] {k}: max |fused - twin| = {err:.3e}, parent {perr:.3e}, ratio {err / perr if perr else float("inf"):.3f} (bound {MARGIN})')
            assert par[k].dtype == want_dt
            if k == 'db2' and v['x'].shape[0] == 1 and xdt == mdt:
                ok = perr == 0 and err == 0      # one row of a half model: db2 IS the stored dout row, no arithmetic on either side
            else:
                ok = perr > 0 and err <= MARGIN * perr
        if not ok:
            failures.append(k)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ 2. a dropped image

@pytest.mark.parametrize('case,prec', [('r300_c128', 'f32'), ('r300_c128', 'f32_bf16'), ('r300_c256', 'f32_f16'), ('r300_c256', 'bf16')])
def test_a_dropped_image_passes_its_gradient_through(gpu, case, prec):
    from dhd_amd.swin_ffn import _scaled_grad
    v, (xdt, mdt), scale = _on(gpu, case, prec), ST.PRECISIONS[prec], _scale(gpu, 'drop')
    got = _backward(v, mdt, scale)
    dropped = slice(100, 200)
    assert _same(got['dx'][dropped], v['dout'][dropped])                      # dx == dout, bit for bit
    assert not _same(got['dx'][:100], v['dout'][:100])
    gs = _scaled_grad(v['dout'], scale, mdt)
    assert bool((got['dhid'][dropped] == 0).all()) and bool((gs[dropped] == 0).all())
    assert bool((got['dhid'][:100] != 0).any()) and bool((gs[200:] != 0).any())
    # the forward leaves the dropped image's tokens as they are
    import dhd_amd
    out = dhd_amd.swin_ffn(v['x'], v['gamma'], v['beta'], ST.EPS, v['w1'], v['b1'], v['w2'], v['b2'], mdt, scale)
    _sync()
    assert _same(out[dropped], v['x'][dropped]) and not _same(out[:100], v['x'][:100])


# ------------------------------------------------------------------------------------------------ 3. / 4. repeatability, rows

ROWS_GRID = [('r129_c128', 'f32_bf16', 'none'), ('r300_c128', 'f32', 'drop'), ('r300_c256', 'f32_f16', 'none'), ('r129_c256', 'bf16', 'none'),
             ('r300_c256', 'f32', 'drop')]


@pytest.mark.parametrize('case,prec,sname', ROWS_GRID)
def test_calls_repeat_and_rows_are_independent(gpu, case, prec, sname):
    v, (xdt, mdt), scale = _on(gpu, case, prec), ST.PRECISIONS[prec], _scale(gpu, sname)
    rows = v['x'].shape[0]
    base = _backward(v, mdt, scale)
    again = _backward(v, mdt, scale)
    assert all(_same(again[k], base[k]) for k in base), [k for k in base if not _same(again[k], base[k])]
    gen = torch.Generator().manual_seed(13)
    per_row = ('dx', 'xn', 'act', 'dhid')
    for which in ('x', 'dout'):
        for keep in (0, 31, 32, rows - 1):                                    # both ends of a wave tile, the last row of the call
            t = (torch.randn(v[which].shape, generator=gen) * 3).to(xdt).to(gpu)
            t[(keep + 1) % rows, 3] = float('inf')
            t[(keep + 2) % rows, ::2] = float('-inf')
            t[(keep + 3) % rows, 5] = float('nan')
            t[(keep + 4) % rows] = float('nan')                               # a whole row of NaN next door
            t[keep] = v[which][keep]
            # the row under test keeps its own x and dout; every other row differs in `which`
            got = _backward(v, mdt, scale, **{which: t})
            assert all(_same(got[k][keep], base[k][keep]) for k in per_row), (which, keep)
    # a NaN row poisons itself and nothing else in the per-row outputs
    x = v['x'].clone()
    x[40, 7] = float('nan')
    got = _backward(v, mdt, scale, x=x)
    others = torch.arange(rows, device=gpu) != 40
    assert all(_same(got[k][others], base[k][others]) for k in per_row)
    assert bool(torch.isnan(got['dx'][40]).all())


# ------------------------------------------------------------------------------------------------ 5. guard bands

GUARDED = [pytest.param(f'r{r}_c{c}', p, s, id=f'r{r}_c{c}-{p}-{s}') for r, c, p, s in
           ((1, 128, 'f32_bf16', 'none'), (33, 128, 'f32', 'none'), (129, 128, 'bf16', 'none'), (300, 128, 'f32_f16', 'drop'),
            (1, 256, 'f16', 'none'), (33, 256, 'f32_bf16', 'none'), (129, 256, 'f32', 'none'), (300, 256, 'bf16', 'drop'))]


@pytest.mark.parametrize('case,prec,sname', GUARDED)
def test_inside_guard_bands(gpu, monkeypatch, case, prec, sname):
    """Plain, then with every buffer of the two entry points (out and the forward's scratch; dx, dgamma, dbeta, xn, act, dhid and
    the backward's scratch) between two 4096-byte guard bands at its exact advertised size, every byte 0xFF, then 0x00: no guard
    byte changes, and the three runs agree -- every advertised byte of every output is written and nothing uninitialised is used
    (0xFF is NaN in every float type)."""
    from dhd_amd import _ffn_train, _lib
    from dhd_amd.swin_ffn import _forward
    v, (xdt, mdt), scale = _on(gpu, case, prec), ST.PRECISIONS[prec], _scale(gpu, sname)
    rows, c = v['x'].shape
    xs, ms, mc = v['x'].element_size(), torch.empty(0, dtype=mdt).element_size(), _lib.DTYPE_CODE[mdt]

    def run():
        out = _forward(v['x'], v['gamma'], v['beta'], ST.EPS, v['w1'], v['b1'], v['w2'], v['b2'], mdt, scale)
        _sync()
        return dict(_backward(v, mdt, scale), out=out)
    plain = run()
    want = sorted([rows * c * xs, _ffn_train.value('dhdt_swin_ffn_forward_scratch_bytes', c, 4 * c, mc),
                   rows * c * xs, 4 * c, 4 * c, rows * c * ms, rows * 4 * c * ms, rows * 4 * c * ms,
                   _ffn_train.value('dhdt_swin_ffn_backward_scratch_bytes', rows, c, 4 * c, mc)])
    for fill in (0xFF, 0x00):
        with G.guarded(monkeypatch, fill) as ledger:
            got = run()
            ledger.check()
            got = {k: t.detach().clone() for k, t in got.items()}
        ours = [e for e in ledger.sites_under(G.PRODUCT_ROOT) if 'swin_ffn.py' in e.site]
        print(f'{case} [{prec}, {sname}, fill {fill:#04x}]: {len(ledger)} guarded allocations, {ledger.total_bytes()} bytes, guards intact')
        assert len(ours) == len(ledger) == 9 and sorted(e.nbytes for e in ours) == want
        for k, t in got.items():
            assert bool(torch.isfinite(t).all()) and _same(t, plain[k]), (k, fill)


# ------------------------------------------------------------------------------------------------ 6. the NULL operand triple

@pytest.mark.parametrize('case,prec,sname', ROWS_GRID)
def test_without_the_operands_the_gradients_are_the_same_bytes(gpu, case, prec, sname):
    v, (xdt, mdt), scale = _on(gpu, case, prec), ST.PRECISIONS[prec], _scale(gpu, sname)
    full, bare = _backward(v, mdt, scale), _backward(v, mdt, scale, operands=False)
    assert bare['xn'] is None and bare['act'] is None and bare['dhid'] is None
    assert all(_same(bare[k], full[k]) for k in ('dx', 'dgamma', 'dbeta'))


# ------------------------------------------------------------------------------------------------ 7. the routed block

HW = (24, 24)


def _block(gpu, drop_path=0.5, ffn_drop=0.):
    from dhd_amd.swin import SwinBlock
    torch.manual_seed(41)
    block = SwinBlock(128, 4, 512, window_size=12, drop_rate=ffn_drop, drop_path_rate=drop_path).train()
    with torch.no_grad():                                                     # parameters that are not at their initial values
        for n in (block.norm1, block.norm2):
            n.weight.add_(0.2 * torch.randn(128))
            n.bias.add_(0.1 * torch.randn(128))
        block.attn.w_msa.relative_position_bias_table.normal_(0, 0.5)
        for lin in (block.ffn.layers[0][0], block.ffn.layers[1]):
            lin.bias.normal_(0, 0.1)
    x = torch.randn(2, HW[0] * HW[1], 128, generator=torch.Generator().manual_seed(42)) * 1.5
    w = torch.randn(2, HW[0] * HW[1], 128, generator=torch.Generator().manual_seed(43))
    return block.to(gpu), x.to(gpu), w.to(gpu)


def _train_step(block, x, w, auto, seed, cp=False):
    """One step at a fixed RNG state -> (out, x.grad, {name: grad}, the RNG state after it)."""
    torch.cuda.manual_seed(seed)
    block.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_()
    with torch.autocast('cuda', dtype=auto or BF16, enabled=auto is not None):
        out = checkpoint(block, xg, HW, use_reentrant=False) if cp else block(xg, HW)
    (out.float() * w).sum().backward()
    _sync()
    return out.detach(), xg.grad, {n: p.grad for n, p in block.named_parameters() if p.grad is not None}, torch.cuda.get_rng_state()


@pytest.mark.parametrize('auto', (None, BF16, F16), ids=('f32', 'bf16_autocast', 'f16_autocast'))
def test_swin_block_takes_the_route_in_training(gpu, monkeypatch, auto):
    """A 2-image 24 x 24 map in train mode with drop_path 0.5: the switch changes which operator runs and nothing of the random
    stream; gradients are held to the bars of (1) against a float64 copy of the block driven by the same draws."""
    import dhd_amd
    _route_everything(monkeypatch)
    block, x, w = _block(gpu)
    seen = _recorder(monkeypatch)
    seeds = [s for s in range(60, 80)]
    # a seed whose draws drop one image in the FFN's DropPath and keep the other: found from today's path, not from the fused one
    outs = {}
    dhd_amd.fused_swin_ffn_training(block, False)
    pick = None
    for seed in seeds:
        torch.cuda.manual_seed(seed)
        torch.rand((2, 1, 1), dtype=auto or F32, device=gpu)                    # the attention's DropPath draws first
        kept = (0.5 + torch.rand((2, 1, 1), dtype=auto or F32, device=gpu)).floor().view(-1).tolist()
        if sorted(kept) == [0.0, 1.0]:
            pick = seed
            break
    assert pick is not None
    for on in (False, True):
        assert len(dhd_amd.fused_swin_ffn_training(block, on)) == 1
        del seen[:]
        outs[on] = _train_step(block, x, w, auto, pick)
        assert (seen.count(FWD), seen.count(BWD)) == ((1, 1) if on else (0, 0)), seen
    assert torch.equal(outs[True][3], outs[False][3])                          # the RNG state after the step
    # the same images are dropped: the dropped image's tokens pass through the second half of the block untouched either way
    assert outs[True][0].dtype == outs[False][0].dtype == F32
    # the float64 reference on the same draws: torch.rand in float64 would draw differently, so the two masks are replayed
    torch.cuda.manual_seed(pick)
    draws = iter([(0.5 + torch.rand((2, 1, 1), dtype=auto or F32, device=gpu)).floor().double().cpu() for _ in range(2)])
    from dhd_amd.swin import DropPath
    ref_block = copy.deepcopy(block).cpu().double()
    xr = x.double().cpu().requires_grad_()
    with monkeypatch.context() as m:
        m.setattr(DropPath, 'forward', lambda self, t: t.div(0.5) * next(draws))
        (ref_block(xr, HW) * w.double().cpu()).sum().backward()
    ref = dict({n: p.grad for n, p in ref_block.named_parameters() if p.grad is not None}, x=xr.grad)
    failures = []
    for n, r in ref.items():
        on, off = (outs[k][1] if n == 'x' else outs[k][2][n] for k in (True, False))
        e_on, e_off, diff, size = _err(on, r), _err(off, r), _err(on, off.double().cpu()), ST.scale_of(off)
        print(f'block [{auto}] {n}: fused {e_on:.3e}, today {e_off:.3e} against float64; |fused - today| {diff:.3e}, bar {BAR * size:.3e}')
        # float32: the layer bar against today's path; autocast: 1.5 x what today's path is off by against float64
        if not (diff <= BAR * size if auto is None else e_on <= MARGIN * e_off):
            failures.append(n)
    assert not failures, failures


@pytest.mark.parametrize('auto', (None, BF16), ids=('f32', 'bf16_autocast'))
def test_checkpointing_gives_the_bits_of_the_unchecked_run(gpu, monkeypatch, auto):
    import dhd_amd
    _route_everything(monkeypatch)
    block, x, w = _block(gpu)
    dhd_amd.fused_swin_ffn_training(block)
    seen = _recorder(monkeypatch)
    plain = _train_step(block, x, w, auto, 7)
    assert (seen.count(FWD), seen.count(BWD)) == (1, 1)
    del seen[:]
    cp = _train_step(block, x, w, auto, 7, cp=True)
    assert (seen.count(FWD), seen.count(BWD)) == (2, 1)                        # the no-grad pass and the recomputation
    assert _same(cp[0], plain[0]) and _same(cp[1], plain[1]) and torch.equal(cp[3], plain[3])
    assert cp[2].keys() == plain[2].keys() and all(_same(cp[2][n], g) for n, g in plain[2].items())


def test_frozen_parameters_flag_off_and_active_dropout(gpu, monkeypatch):
    import dhd_amd
    from dhd_amd import swin_ffn as module
    _route_everything(monkeypatch)
    block, x, w = _block(gpu)
    seen = _recorder(monkeypatch)
    # flag off: no call of the family, today's bits (two runs of today's path agree, and the flag-off block is today's path)
    today = _train_step(block, x, w, None, 5)
    assert not any(n.startswith('dhdt_') for n in seen)
    dhd_amd.fused_swin_ffn_training(block)
    full = _train_step(block, x, w, None, 5)
    dhd_amd.fused_swin_ffn_training(block, False)
    off = _train_step(block, x, w, None, 5)
    assert _same(off[0], today[0]) and _same(off[1], today[1]) and all(_same(off[2][n], g) for n, g in today[2].items())
    # norm2 and the FFN frozen: the backward still runs (without the operands) and the input gradient is unchanged
    dhd_amd.fused_swin_ffn_training(block)
    for p in (*block.norm2.parameters(), *block.ffn.parameters()):
        p.requires_grad_(False)
    wanted = []
    real = module.swin_ffn_backward
    monkeypatch.setattr(module, 'swin_ffn_backward', lambda *a, **k: (wanted.append(k.get('operands')), real(*a, **k))[1])
    del seen[:]
    frozen = _train_step(block, x, w, None, 5)
    assert (seen.count(FWD), seen.count(BWD)) == (1, 1) and wanted == [False]
    assert _same(frozen[1], full[1]) and _same(frozen[0], full[0])
    assert not any(n.startswith(('norm2', 'ffn')) for n in frozen[2])
    # the route in eval mode and without grad
    block.eval()
    del seen[:]
    with torch.no_grad():
        block(x, HW)
    _sync()
    assert seen.count(FWD) == 1
    # an active ffn_drop keeps torch
    wet, x2, w2 = _block(gpu, ffn_drop=0.1)
    dhd_amd.fused_swin_ffn_training(wet)
    del seen[:]
    _train_step(wet, x2, w2, None, 5)
    assert not any(n.startswith('dhdt_') for n in seen) and not wet._ffn_train_applies(x2)
    wet.eval()                                                                 # inactive in eval mode: the route
    assert wet._ffn_train_applies(x2)


# ------------------------------------------------------------------------------------------------ 8. composed

def test_composed_backbone_gradients(gpu, monkeypatch):
    """G20's gradient run of tests/test_gpu_swin_composed.py (eval mode with grad) with fused_training, the glue, the seams and
    this switch on: stages 0 and 1 show four forward and four backward calls of the operator, and every recorded tensor stays
    within the composed test's own bound, n x 1e-4 x max(1, |R|max), each FFN call counting as one more fused call."""
    import collections

    import numpy as np

    import dhd_amd
    import test_gpu_swin_composed as TC
    TC._route_all(monkeypatch)
    _route_everything(monkeypatch)
    g, x = TC._g(), TC._x(gpu)
    forward, backward, per_stage = TC._grad_tables()
    forward = [(lab, [m for n in names for m in ((n, FWD) if n == TC.ADD and lab in ('stage0', 'stage1') else (n,))]) for lab, names in forward]
    backward = backward + collections.Counter({BWD: 4})
    per_stage = {s: n + (2 if s in (0, 1) else 0) for s, n in per_stage.items()}
    TC._probes(TC._net(gpu))
    net = TC._switch(TC._net(gpu), glue=True, seams=True, train=True)
    assert len(dhd_amd.fused_swin_ffn_training(net)) == 8
    seen = _recorder(monkeypatch)
    from dhd_amd import _ext, _ffn_wide, _seam
    for m in (_ext, _ffn_wide, _seam):
        m.load()
    outs, xg, grads = TC._grad_step(net, x)
    calls = list(seen)
    nf = len(TC._flat(forward))
    assert calls[:nf] == TC._flat(forward), calls[:nf]
    assert collections.Counter(calls[nf:]) == backward, collections.Counter(calls[nf:])
    failures = []
    for i, o in enumerate(outs):
        k = f'out{i}'
        n = TC._calls_upto(forward, TC.LABEL_OF[k])
        e = float((o.double().cpu() - torch.from_numpy(g[k])).abs().max())
        b = n * BAR * max(1.0, float(np.abs(g[k]).max()))
        print(f'  {k:<8} {e:.3e}     {n:>3}    {b:.3e}')
        if e > b:
            failures.append(k)
    worst = {}
    for name, kind, e, scale in TC._grad_errors(grads, xg):
        n = TC._grad_calls(name, forward, per_stage)
        b = n * BAR * scale
        key = (kind, 'stage ' + name.split('.')[1] if name and name.startswith('stages') else 'other')
        if key not in worst or e / b > worst[key][0]:
            worst[key] = (e / b, name, e, n, b)
        if e > b:
            failures.append((kind, name))
    for (kind, where), (r, name, e, n, b) in sorted(worst.items()):
        print(f'  worst {kind} in {where}: {name}: {e:.3e}     {n:>3}    {b:.3e}')
    assert not failures, failures
