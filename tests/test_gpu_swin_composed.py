"""The whole Swin backbone at DHD-L's widths with every HIP switch on, against fixture G20, the reference's own float64 run
(tests/swin_wide_inputs.py): window attention (fused_inference / fused_training), the block glue (fused_swin_glue), the FFN at
C = 128 / 256 and at C = 512 / 1024 (fused_swin_ffn) and the stage seams (fused_swin_seams) composed, which is what a user gets
from the four environment switches plus fused_inference(net).  The module-level tests hold each operator to a twin written beside
it, on G10 none of attention and FFN can run (head dimension 8, widths 16 / 32 / 64); here the reference checks them, and the
hand-overs between them: windows in the GEMM dtype into the attention, the residual from reverse + add into the FFN, bf16 tokens
out of a merge into a block that routes through the glue, a 3 x 5 map padded to one 12 x 12 window, odd sizes at every merge,
checkpointed blocks, and the stage-0-only path of the stereo frame.

The float32 bound.  The project's bar for one operator is 1e-4 max(1, |R|max).  A tensor downstream of n fused operator calls is
held to that bar accumulated linearly, n x 1e-4 x max(1, |R|max), R the fixture's tensor (for a gradient, the reference
gradient), n counted from the expected-calls table below (the window copies of dhd_window_rows are exact and do not count).  It is
a condition derived from the per-layer bar, not a measurement; each test prints the fused error, the error of today's float32
path on the same GPU, and the bound.  Where the fixture holds only the norm and a projection of a gradient G of N elements, the
element bound e is taken with |G|max replaced by its lower estimate ||G|| / sqrt(N) (no looser), and the two numbers are held to
what e implies: | ||g|| - ||G|| | <= ||g - G|| <= sqrt(N) e, and |<g - G, w>| <= sqrt(N) e ||w|| (Cauchy-Schwarz).

Under autocast the fused path is held to 1.5 x the error today's autocast path makes against the fixture, in the same test.
"""
import collections
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_wide_inputs as SW  # noqa: E402
from conftest import GOLDEN  # noqa: E402

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
BAR = 1e-4
pytestmark = pytest.mark.gpu

EMBED, MERGE = 'dhds_embed_norm_forward', 'dhds_merge_norm_forward'
LN, ADD, ROWS = 'dhdx_ln_rows_forward', 'dhdx_window_reverse_add', 'dhd_window_rows'
ATTN, NARROW, WIDE = 'dhd_window_attn_infer', 'dhdf_swin_ffn_infer', 'dhdg_swin_ffn_wide_infer'
EMBED_B, MERGE_B, LN_B, ATTN_B = 'dhds_embed_norm_backward', 'dhds_merge_norm_backward', 'dhdx_ln_rows_backward', 'dhd_window_attn_backward'
FAMILY = dict(attn=('dhd_window_attn',), glue=('dhdx_',), ffn=('dhdf_', 'dhdg_'), seams=('dhds_',))

# What one forward in eval mode without grad calls with every switch on and every routing table routed, in order: per block norm1
# into the windows, the attention, reverse + add, and the second half of the block as one operator.
EXPECTED_ALL_ON = (
    ('embed', [EMBED]),
    ('stage0', [LN, ATTN, ADD, NARROW, LN, ATTN, ADD, NARROW]),              # 24 x 34 tokens of 128: 12 windows, the second block shifted
    ('merge0', [MERGE]),
    ('stage1', [LN, ATTN, ADD, NARROW, LN, ATTN, ADD, NARROW]),              # 12 x 17 of 256: 4 windows
    ('merge1', [MERGE]),
    ('stage2', [LN, ATTN, ADD, WIDE, LN, ATTN, ADD, WIDE]),                  # 6 x 9 of 512: 1 window
    ('merge2', [MERGE]),                                                     # C = 512: the shipped routing leaves this one to torch
    ('stage3', [LN, ATTN, ADD, WIDE, LN, ATTN, ADD, WIDE]),                  # 3 x 5 of 1024: 1 window
)
# The gradient run (fused_training, glue and seams; eval mode with grad): the forward per block is norm1 into the windows, the
# attention and reverse + add (norm2 and the FFN are torch's: the map is small and float32, fused_swin_ffn's operator is for
# inference, and the training operator's switch, fused_swin_ffn_training, is not set here: tests/test_gpu_swin_ffn_train.py and
# tests/test_gpu_swin_train_step.py set it); the backward per block is the window partition of the gradient (reverse + add),
# the attention's and norm1's.
EXPECTED_GRAD_FORWARD = tuple((label, [n for n in names if n not in (NARROW, WIDE)]) for label, names in EXPECTED_ALL_ON)
EXPECTED_GRAD_BACKWARD = {'embed': [EMBED_B], 'merge': [MERGE_B], 'stage': [ROWS, ATTN_B, LN_B, ROWS, ATTN_B, LN_B]}


def _expected(off=None, shipped=False, first_stage_only=False):
    """The table with one switch off, and / or with the routing tables as shipped (float32)."""
    table = []
    for label, names in EXPECTED_ALL_ON:
        if (off == 'seams' and label.startswith(('embed', 'merge'))) or (shipped and label == 'merge2'):
            names = []
        if off == 'attn':
            names = [n for n in names if n != ATTN]
        if off == 'ffn':
            names = [n for n in names if n not in (NARROW, WIDE)]
        if off == 'glue':                                                    # the windows are cut and put back by dhd_window_rows
            names = [ROWS if n in (LN, ADD) else n for n in names]
        table.append((label, list(names)))
        if first_stage_only and label == 'merge0':                           # forward_first_stage runs the whole stage, its merge included
            break
    return table


def _flat(table):
    return [n for _, names in table for n in names]


def _calls_upto(table, label):
    """The fused operator calls upstream of what `label` emits."""
    n = 0
    for lab, names in table:
        n += sum(x != ROWS for x in names)
        if lab == label:
            return n
    raise KeyError(label)


def _sync():
    """Wait for the device; after a device error nothing more is started in this module."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'GPU fault, stopping the module: {e}', returncode=3)


# ------------------------------------------------------------------------------------------------ shared: fixture, weights, today's path

_cache = {}


def _g():
    if 'g' not in _cache:
        _cache['g'] = SW.load(GOLDEN)
    return _cache['g']


def _state():
    """The float32 state of the G20 network, made once (36.3 M hashes); every value is exactly the fixture's."""
    if 'state' not in _cache:
        from dhd_amd.swin import SwinTransformer
        net = SwinTransformer(**SW.ARGS)
        assert SW.set_state(net) == str(_g()['state_sha'])
        _cache['state'] = {k: v.clone() for k, v in net.state_dict().items()}
    return _cache['state']


def _net(gpu, **kw):
    from dhd_amd.swin import SwinTransformer
    net = SwinTransformer(**{**SW.ARGS, **kw}).eval()
    net.load_state_dict(_state())
    return net.to(gpu)


def _switch(net, attn=False, glue=False, ffn=False, seams=False, train=False):
    import dhd_amd
    dhd_amd.fused_inference(net, attn)
    dhd_amd.fused_training(net, train)
    dhd_amd.fused_swin_glue(net, glue)
    dhd_amd.fused_swin_ffn(net, ffn)
    dhd_amd.fused_swin_seams(net, seams)
    return net


ALL_ON = dict(attn=True, glue=True, ffn=True, seams=True)


def _x(gpu, dtype=F32):
    return torch.from_numpy(SW.x_input()).to(gpu, dtype)


def _recorder(monkeypatch):
    """The names that reach dhd_amd._lib.check: every entry point of the five families and dhd_window_rows go through it."""
    from dhd_amd import _ext, _ffn, _ffn_wide, _lib, _seam
    for m in (_ext, _ffn, _ffn_wide, _seam):
        m.load()
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
    from dhd_amd import swin_ffn, swin_seam
    monkeypatch.setattr(swin_seam, 'ROUTED', _Everything())
    monkeypatch.setattr(swin_ffn, 'ROUTED', _Everything())
    monkeypatch.setattr(swin_ffn, 'ROUTED_WIDE', _Everything())


def _refs():
    """The fixture's forward tensors by the names _infer gives them."""
    g = _g()
    B, C, H, W = g['out0'].shape
    refs = {f'out{i}': g[f'out{i}'] for i in range(3)}
    refs['map0'] = np.ascontiguousarray(g['out0'].transpose(0, 2, 3, 1)).reshape(B, H * W, C)      # kept once in the fixture, as out0
    refs.update({f'map{i}': g[f'map{i}'] for i in (1, 2, 3)})
    refs['stage0'] = g['out0']
    return refs


LABEL_OF = dict(out0='stage0', map0='stage0', stage0='stage0', map1='stage1', map2='stage2', out1='stage2', map3='stage3', out2='stage3')


def _infer(net, x, seen=None):
    """One forward without grad -> ({name: tensor}, the calls of net(x), the calls of forward_first_stage(x))."""
    with torch.no_grad():
        if seen is not None:
            del seen[:]
        outs, maps = SW.forward_with_maps(net, x)
        _sync()
        full = list(seen) if seen is not None else None
        if seen is not None:
            del seen[:]
        first = net.forward_first_stage(x)
        _sync()
    got = {f'out{i}': o for i, o in enumerate(outs)}
    got.update({f'map{i}': m for i, m in enumerate(maps)})
    got['stage0'] = first
    return got, full, (list(seen) if seen is not None else None)


def _errors(got, refs=None):
    refs = refs or _refs()
    return {k: float(np.abs(got[k].detach().double().cpu().numpy() - r).max()) for k, r in refs.items()}


def _today(gpu):
    """Errors of today's float32 path (every switch off) on this GPU against the fixture, and its tensors; made once."""
    if 'today' not in _cache:
        got, _, _ = _infer(_switch(_net(gpu)), _x(gpu))
        _cache['today'] = (_errors(got), got)
    return _cache['today']


def _hold(errs, table, today, what):
    """Print fused error | today's error | bound for every tensor, then assert the bound."""
    refs, rows = _refs(), []
    for k, e in errs.items():
        n = _calls_upto(table, LABEL_OF[k])
        rows.append((k, e, today[k], n, n * BAR * max(1.0, float(np.abs(refs[k]).max()))))
    print(f'\n{what}\n  tensor   fused error   today         calls  bound')
    for k, e, t, n, b in rows:
        print(f'  {k:<8} {e:.3e}     {t:.3e}     {n:>3}    {b:.3e}' + ('   (more than 10 x today)' if e > 10 * t else ''))
    for k, e, t, n, b in rows:
        assert e <= b, f'{what}: {k}: error {e:.3e} > bound {b:.3e}'


# ------------------------------------------------------------------------------------------------ 1. inference, float32, everything on

@pytest.mark.parametrize('routing', ['shipped', 'all_routed'])
def test_inference_float32_everything_on(gpu, monkeypatch, routing):
    if routing == 'all_routed':
        _route_all(monkeypatch)
    table = _expected(shipped=routing == 'shipped')
    today, _ = _today(gpu)
    net, x = _switch(_net(gpu), **ALL_ON), _x(gpu)
    seen = _recorder(monkeypatch)
    got, full, first = _infer(net, x, seen)
    assert full == _flat(table), (full, _flat(table))
    assert first == _flat(_expected(shipped=routing == 'shipped', first_stage_only=True)), first
    for fam, stems in FAMILY.items():                                        # no family is silently not reached
        assert any(n.startswith(stems) for n in full), fam
    assert NARROW in full and WIDE in full
    for k, shape in zip(('out0', 'out1', 'out2'), SW.OUT_SHAPES):
        assert tuple(got[k].shape) == shape and got[k].dtype == F32
    _hold(_errors(got), table, today, f'inference, float32, everything on, routing {routing}')
    again, _, _ = _infer(net, x)
    assert all(torch.equal(again[k], got[k]) for k in got)                   # a second call returns the same bits


# ------------------------------------------------------------------------------------------------ 2. leave one out

@pytest.mark.parametrize('off', ['attn', 'glue', 'ffn', 'seams'])
def test_leave_one_out(gpu, monkeypatch, off):
    _route_all(monkeypatch)
    table = _expected(off=off)
    today, _ = _today(gpu)
    net = _switch(_net(gpu), **{**ALL_ON, off: False})
    seen = _recorder(monkeypatch)
    got, full, first = _infer(net, _x(gpu), seen)
    assert not any(n.startswith(FAMILY[off]) for n in full + first), (off, full)
    assert full == _flat(table), (full, _flat(table))
    assert first == _flat(_expected(off=off, first_stage_only=True)), first
    _hold(_errors(got), table, today, f'inference, float32, everything on but {off}')


# ------------------------------------------------------------------------------------------------ 3. switched off is today's path

def test_switched_off_is_todays_path(gpu, monkeypatch):
    from dhd_amd.swin import PatchEmbed, PatchMerging, SwinBlock, WindowMSA
    _route_all(monkeypatch)
    x = _x(gpu)
    net = _switch(_net(gpu), train=True, **ALL_ON)
    seen = _recorder(monkeypatch)
    _infer(net, x, seen)
    _switch(net)                                                             # everything off again
    got, full, first = _infer(net, x, seen)
    assert not any(n.startswith(s) for stems in FAMILY.values() for s in stems for n in full + first), full
    for cls, names in ((WindowMSA, ('fused_infer', 'fused_train')), (SwinBlock, ('fused_glue', 'fused_ffn')),
                       (PatchEmbed, ('fused_seam',)), (PatchMerging, ('fused_seam',))):
        for name in names:
            monkeypatch.setattr(cls, name, False)                            # whatever the environment says
    never = _net(gpu)                                                        # a model nobody touched
    assert not any(k.startswith('fused_') for m in never.modules() for k in vars(m))
    ref, _, _ = _infer(never, x)
    assert all(torch.equal(got[k], ref[k]) for k in ref)


# ------------------------------------------------------------------------------------------------ 4. autocast

@pytest.mark.parametrize('dtype', [BF16, F16], ids=['bf16', 'fp16'])
def test_autocast_everything_on(gpu, monkeypatch, dtype):
    """Each output within 1.5 x the error of today's autocast path against the float64 fixture, in today's dtypes; with the
    routing tables as shipped (what a user gets) and with every entry routed."""
    x, refs = _x(gpu), _refs()
    seen = _recorder(monkeypatch)
    with torch.autocast('cuda', dtype=dtype):
        base, full, _ = _infer(_switch(_net(gpu)), x, seen)
    assert not any(n.startswith(s) for stems in FAMILY.values() for s in stems for n in full), full
    eb = _errors(base, refs)
    net = _switch(_net(gpu), **ALL_ON)
    for routing in ('shipped', 'all_routed'):
        if routing == 'all_routed':
            _route_all(monkeypatch)
        with torch.autocast('cuda', dtype=dtype):
            got, full, _ = _infer(net, x, seen)
        ea = _errors(got, refs)
        print(f'\nautocast {dtype}, everything on, routing {routing}: ' + ', '.join(f'{n} x {c}' for n, c in sorted(collections.Counter(full).items()))
              + '\n  tensor   fused error   today')
        for k in refs:
            print(f'  {k:<8} {ea[k]:.3e}     {eb[k]:.3e}')
        for fam, stems in FAMILY.items():
            assert any(n.startswith(stems) for n in full), (fam, routing)
        for k in refs:
            assert got[k].shape == base[k].shape and got[k].dtype == base[k].dtype, k
        for k in ('out0', 'out1', 'out2'):
            assert ea[k] <= 1.5 * eb[k], f'{routing}: {k}: {ea[k]:.3e} fused against {eb[k]:.3e} today'


# ------------------------------------------------------------------------------------------------ 5. gradients, float32

def _probes(net):
    """{parameter name: (the fixture's probe vector as a float64 CPU tensor)}; 36.3 M hashes, made once."""
    if 'probes' not in _cache:
        index = {k: j for j, k in enumerate(net.state_dict())}
        _cache['probes'] = {n: torch.from_numpy(SW.grad_probe(index[n], tuple(p.shape))) for n, p in net.named_parameters()}
    return _cache['probes']


def _grad_step(net, x):
    x = x.clone().requires_grad_()
    net.zero_grad(set_to_none=True)
    outs = net(x)
    SW.backward_of(outs)
    _sync()
    return [o.detach() for o in outs], x.grad, {n: p.grad for n, p in net.named_parameters()}


def _grad_calls(name, forward, backward_of_stage):
    """The fused calls upstream of the gradient of parameter `name` (None: the input): the forward up to where the parameter's
    output norm reads, or all of it, plus the backward from the loss down to the parameter's stage."""
    nf = {lab: _calls_upto(forward, lab) for lab, _ in forward}
    if name is not None and name.startswith('norm'):                         # norm2 / norm3: the output norms
        return nf[f'stage{name[4]}']
    stage = -1 if name is None or name.startswith('patch_embed') else int(name.split('.')[1])
    return nf['stage3'] + sum(n for s, n in backward_of_stage.items() if s >= stage)


def _grad_tables():
    forward = [(lab, list(names)) for lab, names in EXPECTED_GRAD_FORWARD]
    backward = collections.Counter()
    per_stage = {}
    for s in (3, 2, 1, 0):
        names = EXPECTED_GRAD_BACKWARD['stage'] + (EXPECTED_GRAD_BACKWARD['merge'] if s < 3 else [])
        backward.update(names)
        per_stage[s] = sum(n != ROWS for n in names)
    backward.update(EXPECTED_GRAD_BACKWARD['embed'])
    per_stage[-1] = 1
    return forward, backward, per_stage


def _grad_errors(grads, xg):
    """-> rows (name, kind, error, bound scale): the input gradient and every whole gradient against the fixture element by
    element; for every other parameter the norm and the projection, with the factor their bound has over the element bound."""
    g = _g()
    rows = [(None, 'x_grad', float((xg.double().cpu() - torch.from_numpy(g['x_grad'])).abs().max()), max(1.0, float(np.abs(g['x_grad']).max())))]
    net_probes = _cache['probes']
    for name, gr in grads.items():
        gr = gr.double().cpu()
        if 'grad.' + name in g:
            R = torch.from_numpy(g['grad.' + name])
            rows.append((name, 'grad', float((gr - R).abs().max()), max(1.0, float(R.abs().max()))))
            continue
        N, w = gr.numel(), net_probes[name]
        e = max(1.0, float(g['gnorm.' + name]) / math.sqrt(N))
        rows.append((name, 'gnorm', abs(float(gr.norm()) - float(g['gnorm.' + name])), e * math.sqrt(N)))
        rows.append((name, 'gproj', abs(float((gr * w).sum()) - float(g['gproj.' + name])), e * math.sqrt(N) * float(w.norm())))
    return rows


def test_gradients_float32(gpu, monkeypatch):
    """Eval mode with grad (DropPath is the identity and the fixture applies): fused_training, the glue and the seams on.  No FFN
    operator records a call: the inference one does not run where something is differentiated, and the training one
    (fused_swin_ffn_training) is left off here; test_composed_backbone_gradients of tests/test_gpu_swin_ffn_train.py is this test
    with it on, and tests/test_gpu_swin_train_step.py holds the train-mode step with every switch on."""
    _route_all(monkeypatch)
    g, x = _g(), _x(gpu)
    forward, backward, per_stage = _grad_tables()
    base = _net(gpu)
    _probes(base)
    t_outs, t_xg, t_grads = _grad_step(_switch(base), x)                      # today's path, for the table
    today = {(n, k): e for n, k, e, _ in _grad_errors(t_grads, t_xg)}
    del t_grads
    net = _switch(_net(gpu), glue=True, seams=True, train=True)
    seen = _recorder(monkeypatch)
    outs, xg, grads = _grad_step(net, x)
    calls = list(seen)
    nf = len(_flat(forward))
    assert calls[:nf] == _flat(forward), calls[:nf]
    assert collections.Counter(calls[nf:]) == backward, collections.Counter(calls[nf:])
    assert not any(n.startswith(FAMILY['ffn']) for n in calls)
    print('\ngradients, float32: fused_training + glue + seams\n  tensor   fused error   today         calls  bound')
    failures = []
    for i, (o, t) in enumerate(zip(outs, t_outs)):
        k = f'out{i}'
        n = _calls_upto(forward, LABEL_OF[k])
        e, et = (float((v.double().cpu() - torch.from_numpy(g[k])).abs().max()) for v in (o, t))
        b = n * BAR * max(1.0, float(np.abs(g[k]).max()))
        print(f'  {k:<8} {e:.3e}     {et:.3e}     {n:>3}    {b:.3e}')
        if e > b:
            failures.append(k)
    worst = {}
    for name, kind, e, scale in _grad_errors(grads, xg):
        n = _grad_calls(name, forward, per_stage)
        b = n * BAR * scale
        if kind == 'x_grad' or 'relative_position_bias_table' in name or name.startswith(('patch_embed', 'norm')):
            print(f'  {kind} {name or ""}: {e:.3e}     {today[name, kind]:.3e}     {n:>3}    {b:.3e}')
        key = (kind, 'stage ' + name.split('.')[1] if name and name.startswith('stages') else 'other')
        if key not in worst or e / b > worst[key][0]:
            worst[key] = (e / b, name, e, today[name, kind], n, b)
        if e > b:
            failures.append((kind, name))
    for (kind, where), (r, name, e, et, n, b) in sorted(worst.items()):
        print(f'  worst {kind} in {where}: {name}: {e:.3e}     {et:.3e}     {n:>3}    {b:.3e}')
    assert not failures, failures


def test_with_cp_is_bit_identical(gpu, monkeypatch):
    """The same gradient step with with_cp=True, as DHD-L sets it: every block runs twice (the recomputation), and the outputs and
    all gradients are held to the bits of the with_cp=False run, and of that run repeated.  torch's convolution is asked for its
    deterministic weight gradient in all three runs; it is not the code under test.

    This test found the one thing the composed runs changed in the operators: dhd_window_attn_backward added dtable into ONE LDS
    copy shared by its three waves, and the eight bias-table gradients differed by one or two units in the last place (6.0e-08 to
    1.9e-06 on gradients of 1.2 to 10.1) between any two runs, checkpointed or not.  Each wave now has its own copy."""
    _route_all(monkeypatch)
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    x = _x(gpu)
    _, backward, _ = _grad_tables()
    seen = _recorder(monkeypatch)
    plain = _switch(_net(gpu), glue=True, seams=True, train=True)
    outs, xg, grads = _grad_step(plain, x)
    grads = {n: t.clone() for n, t in grads.items()}
    assert seen.count(LN) == 8 and seen.count(ATTN) == 8 and seen.count(ADD) == 8
    _, _, again = _grad_step(plain, x)                                       # the control: the same model a second time
    twice = [n for n in grads if not torch.equal(again[n], grads[n])]
    for n in twice:
        print(f'  with_cp=False twice: {n}: max difference {float((again[n] - grads[n]).abs().max()):.3e} of {float(grads[n].abs().max()):.3e}')
    del again
    cp = _switch(_net(gpu, with_cp=True), glue=True, seams=True, train=True)
    del seen[:]
    c_outs, c_xg, c_grads = _grad_step(cp, x)
    assert seen.count(LN) == 16 and seen.count(ATTN) == 16 and seen.count(ADD) == 16      # every block ran twice
    assert collections.Counter(n for n in seen if n.endswith('backward')) == collections.Counter({k: v for k, v in backward.items() if k != ROWS})
    assert all(torch.equal(a, b) for a, b in zip(c_outs, outs)) and torch.equal(c_xg, xg)
    differ = [n for n in grads if not torch.equal(c_grads[n], grads[n])]
    for n in differ:
        print(f'  with_cp: {n}: max difference {float((c_grads[n] - grads[n]).abs().max()):.3e} of {float(grads[n].abs().max()):.3e}')
    assert not differ, differ
    assert not twice, twice


# ------------------------------------------------------------------------------------------------ 6. train mode draws

def test_train_mode_draws(gpu, monkeypatch):
    """net.train() with drop_path_rate 0.1, with fused_training, the glue, the seams and fused_swin_ffn_training on.  Two runs from
    one seed give the same bits, and the switched-off model leaves the generator where the switched-on one does: DropPath's
    draws are the same in number.  That the result is right is held by tests/test_gpu_swin_train_step.py."""
    import dhd_amd
    _route_all(monkeypatch)
    x = _x(gpu)
    states, runs = {}, []
    seen = _recorder(monkeypatch)
    for on in (True, True, False):
        net = _switch(_net(gpu), glue=on, seams=on, train=on).train()
        assert len(dhd_amd.fused_swin_ffn_training(net, on)) == 8
        torch.cuda.manual_seed(1234)
        del seen[:]
        outs, xg, _ = _grad_step(net, x)
        states.setdefault(on, []).append(torch.cuda.get_rng_state(gpu))
        assert (ATTN_B in seen and LN_B in seen and MERGE_B in seen and 'dhdt_swin_ffn_backward' in seen) == on, seen
        assert any(n.startswith(('dhd_window_attn', 'dhdx_', 'dhds_', 'dhdt_')) for n in seen) == on, seen
        if on:
            runs.append(outs + [xg])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert torch.equal(states[True][0], states[True][1]) and torch.equal(states[True][0], states[False][0])
    torch.cuda.manual_seed(1234)
    assert not torch.equal(torch.cuda.get_rng_state(gpu), states[True][0])   # and draws there were
