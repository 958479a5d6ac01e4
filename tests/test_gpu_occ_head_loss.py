"""The occupancy head and its three losses as one operator on the GPU (dhd_amd.occ_head_losses, csrc/occ_head_loss.h): the losses
against occ_losses_f64 on the operator's own logits (2e-5 max(1, |loss|), the bar of occ_losses), the logits against
occ_head_train's bytes, the gradients against the float64 twin of tests/occ_head_loss_inputs.py at the project's bars (float32:
1e-4 max(1, |G|max); half: at most 1.5 x the error of occ_head_train + occ_losses on the same inputs), the module route, the
edges, and reproducibility, checkpointing, graph capture, guard bands and views."""
import copy
import math
import os
import sys
import types

import pytest
import torch
from torch.utils.checkpoint import checkpoint

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as G  # noqa: E402
import occ_head_loss_inputs as OL  # noqa: E402
import occ_head_train_inputs as OT  # noqa: E402

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
BAR, MARGIN, LOSS_BAR = 1e-4, 1.5, 2e-5
pytestmark = pytest.mark.gpu
GRID = [pytest.param(s, p, l, id=f'{s}-{p}-{l}') for s, p, l in OT.GRID]
SMALL = [pytest.param('tails', p, l, id=f'tails-{p}-{l}') for p in OT.PRECISIONS for l in OT.LAYOUTS]
NO_VALID = (float('nan'), float('nan'), 3 * -math.log(1e-5))


def _sync():
    """Wait for the device; after a device error nothing more is started in this module."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'GPU fault, stopping the module: {e}', returncode=3)


def _on(gpu, case, prec, layout):
    v = {k: t.to(gpu) for k, t in OT.inputs(case, prec).items() if k != 'glogits'}
    v['x'] = OT.in_layout(v['x'], layout)
    sem, cam = OL.labels(case)
    v.update(sem=sem.to(gpu), cam=cam.to(gpu), cw=OL.class_weights().to(gpu))
    return v


def _err(got, ref64):
    return float((got.detach().cpu().double() - ref64).abs().max())


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _weighted(losses, scale=1.0):
    return sum(w * l for w, l in zip(OL.WEIGHTS, losses)) * scale


def _step(v, fused=True, scale=1.0, grads=(True,) * 5, **over):
    """Forward and backward of w . losses on fresh leaves, through the operator or through occ_head_train + occ_losses."""
    import dhd_amd
    from dhd_amd import occ_loss
    a = dict(v, **over)
    leaves = {k: a[k].detach().clone().requires_grad_(g) for k, g in zip(('x',) + OT.PARAMS, grads)}
    leaves['x'] = a['x'].detach().requires_grad_(grads[0])
    args = [leaves[k] for k in ('x',) + OT.PARAMS]
    if fused:
        losses = dhd_amd.occ_head_losses(*args, a['sem'], a['cam'], a['cw'], dz=OT.DZ)
    else:
        logits = dhd_amd.occ_head_train(*args, OT.DZ)
        losses = occ_loss.occ_losses(logits.reshape(-1, OT.N_CLS), a['sem'], a['cam'], a['cw'])
    _sync()
    _weighted(losses, scale).backward()
    _sync()
    out = {'losses': torch.stack([l.detach() for l in losses]), 'dx': leaves['x'].grad}
    out.update({'d' + k: leaves[k].grad for k in OT.PARAMS})
    return {k: t if t is None or k == 'losses' else t / scale for k, t in out.items()}


def _forward(v, **over):
    from dhd_amd.occ_head import occ_head_loss_forward
    a = dict(v, **over)
    lab, msk = a['sem'].reshape(-1).to(torch.uint8), a['cam'].reshape(-1).to(torch.uint8)
    logits, losses, ws = occ_head_loss_forward(a['x'], a['w1'], a['b1'], a['w2'], a['b2'], lab, msk, a['cw'], OT.DZ)
    _sync()
    return logits, losses, ws, lab, msk


def _backward(v, operands=True, gl=OL.WEIGHTS):
    from dhd_amd.occ_head import occ_head_loss_backward
    logits, losses, ws, lab, msk = _forward(v)
    g = torch.tensor(gl, dtype=F32, device=v['x'].device)
    got = occ_head_loss_backward(v['x'], logits, lab, msk, v['cw'], ws, g, v['w1'], v['b1'], v['w2'], OT.DZ, operands=operands)
    _sync()
    out = dict(zip(('dx', 'db1', 'db2', 'act', 'dhid', 'g'), got))
    out.update(logits=logits, losses=losses, ws=ws)
    return out


def _route_everything(monkeypatch):
    from dhd_amd import occ_head
    monkeypatch.setattr(occ_head, 'ROUTED_LOSS', {k: True for k in occ_head.ROUTED_LOSS})
    monkeypatch.setattr(occ_head, 'ROUTED_TRAIN', {k: True for k in occ_head.ROUTED_TRAIN})


# ------------------------------------------------------------------------------------------------ 1. the losses and the logits

@pytest.mark.parametrize('case,prec,layout', GRID)
def test_losses_against_float64_on_the_operators_own_logits(gpu, case, prec, layout):
    import dhd_amd
    v = _on(gpu, case, prec, layout)
    logits, losses, _, _, _ = _forward(v)
    with torch.no_grad():
        want_logits = dhd_amd.occ_head_train(v['x'], v['w1'], v['b1'], v['w2'], v['b2'], OT.DZ)
        api = dhd_amd.occ_head_losses(v['x'], v['w1'], v['b1'], v['w2'], v['b2'], v['sem'], v['cam'], v['cw'], dz=OT.DZ)
    _sync()
    assert logits.dtype == F32 and torch.equal(logits, want_logits)          # the saved logits: occ_head_train's, byte for byte
    assert _same(torch.stack(api), losses)
    ref = torch.stack([l.detach() for l in OL.losses_f64(logits.cpu().double(), case)])
    for name, got, want in zip(OL.LOSSES, losses.cpu().double(), ref):
        err, bound = abs(float(got - want)), LOSS_BAR * max(1.0, abs(float(want)))
        print(f'{case} [{prec}, {layout}] {name}: fused {float(got):.7f}, float64 {float(want):.7f}, error {err:.3e}, bound {bound:.3e}')
        assert bool(torch.isfinite(want)) and err <= bound, name


# ------------------------------------------------------------------------------------------------ 2. the gradients

@pytest.mark.parametrize('case,prec,layout', GRID)
def test_gradients_against_the_float64_twin(gpu, case, prec, layout):
    v, dt = _on(gpu, case, prec, layout), OT.PRECISIONS[prec]
    got, ref = _step(v), OL.twin(case, prec)
    par = None if dt == F32 else _step(v, fused=False)
    assert got['dx'].stride() == v['x'].stride() and got['dx'].dtype == dt
    failures = []
    for k in OT.TENSORS:
        assert tuple(got[k].shape) == tuple(ref[k].shape) and got[k].dtype == (dt if k == 'dx' else F32), k
        err, size = _err(got[k], ref[k]), OT.scale_of(ref[k])
        if par is None:
            print(f'{case} [{prec}, {layout}] {k}: max |fused - twin| = {err:.3e}, bound {BAR * size:.3e}')
            ok = err <= BAR * size
        else:
            perr = _err(par[k], ref[k])
            print(f'{case} [{prec}, {layout}] {k}: max |fused - twin| = {err:.3e}, parent {perr:.3e}, ratio {err / perr if perr else float("inf"):.3f} (bound {MARGIN})')
            ok = perr > 0 and err <= MARGIN * perr
        if not ok:
            failures.append(k)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ 3. module level

def _drive(head, feats, sem, cam):
    """DHD.forward_occ_train on a stand-in whose only parts are the ones it uses."""
    from dhd_amd.detector import DHD
    net = types.SimpleNamespace(occ_head=head, mixed_feats=lambda f: f[0], occ_logits=lambda f: head(f[0]))
    return DHD.forward_occ_train(net, [feats], sem, cam)


def _module_step(gpu, auto, loss_on, cp=False, conv=True, direct=False):
    head = copy.deepcopy(OT.module_head()).to(gpu)
    if not conv:
        head.final_conv = torch.nn.Identity()
    head.fused_train, head.fused_loss = True, loss_on
    feats, sem, cam = (t.to(gpu) for t in OT.module_inputs())
    x = feats.clone().requires_grad_()
    with torch.autocast('cuda', dtype=auto, enabled=auto is not None):
        if direct:
            losses = head.loss(head(x), sem, cam)
        elif cp:
            losses = checkpoint(lambda t: _drive(head, t, sem, cam), x, use_reentrant=False)
        else:
            losses = _drive(head, x, sem, cam)
        total = sum(losses.values())
    _sync()
    total.backward()
    _sync()
    assert list(losses) == ['loss_occ', 'loss_voxel_sem_scal', 'loss_voxel_geo_scal']
    out = {'losses': torch.stack([losses[k].detach().float() for k in losses]), 'dfeats': x.grad}
    out.update({'d' + n: p.grad for n, p in head.named_parameters()})
    return out


NEW = ('dhdl_occ_head_loss_forward', 'dhdl_occ_head_loss_backward')
OLD = ('dhd_occ_loss_forward', 'dhd_occ_loss_backward')


@pytest.mark.parametrize('auto', (None, BF16), ids=('f32', 'bf16_autocast'))
def test_forward_occ_train_takes_the_route_with_the_switch_on(gpu, monkeypatch, auto):
    from dhd_amd import _lib
    _route_everything(monkeypatch)
    seen, real = [], _lib.check
    monkeypatch.setattr(_lib, 'check', lambda rc, what: (seen.append(what), real(rc, what))[1])
    ref = OT.module_twin()
    got = _module_step(gpu, auto, True)
    assert [seen.count(n) for n in NEW + OLD] == [1, 1, 0, 0] and 'dhdo_occ_head_backward' not in seen
    seen.clear()
    par = _module_step(gpu, auto, False)
    assert [seen.count(n) for n in NEW + OLD] == [0, 0, 1, 1] and seen.count('dhdo_occ_head_backward') == 1
    failures = []
    for k in [k for k in ref if k != 'glogits']:
        err, perr, size = _err(got[k], ref[k]), _err(par[k], ref[k]), OT.scale_of(ref[k])
        bound = BAR * size if auto is None else MARGIN * perr
        print(f'module [{auto or F32}] {k}: max |fused - twin| = {err:.3e}, today {perr:.3e}, bound {bound:.3e}')
        if not err <= bound:
            failures.append(k)
    assert not failures, failures


@pytest.mark.parametrize('auto', (None, BF16), ids=('f32', 'bf16_autocast'))
def test_with_the_switch_off_or_not_routed_todays_two_calls_run_bit_for_bit(gpu, monkeypatch, auto):
    """final_conv is the identity here: bytes are compared, and the library convolution is not reproducible from call to call."""
    from dhd_amd import _lib, occ_head
    seen, real = [], _lib.check
    monkeypatch.setattr(_lib, 'check', lambda rc, what: (seen.append(what), real(rc, what))[1])
    today = _module_step(gpu, auto, False, conv=False, direct=True)
    seen.clear()
    off = _module_step(gpu, auto, False, conv=False)
    assert [seen.count(n) for n in NEW + OLD] == [0, 0, 1, 1]
    seen.clear()
    monkeypatch.setattr(occ_head, 'ROUTED_LOSS', {k: False for k in occ_head.ROUTED_LOSS})
    unrouted = _module_step(gpu, auto, True, conv=False)                        # the switch on, the table saying no
    assert [seen.count(n) for n in NEW + OLD] == [0, 0, 1, 1]
    for k in today:
        assert torch.equal(off[k], today[k]) and torch.equal(unrouted[k], today[k]), k


@pytest.mark.parametrize('auto', (None, BF16), ids=('f32', 'bf16_autocast'))
def test_checkpointing_gives_the_bits_of_the_unchecked_run(gpu, monkeypatch, auto):
    from dhd_amd import _lib
    _route_everything(monkeypatch)
    seen, real = [], _lib.check
    monkeypatch.setattr(_lib, 'check', lambda rc, what: (seen.append(what), real(rc, what))[1])
    a = _module_step(gpu, auto, True, conv=False)
    assert [seen.count(n) for n in NEW] == [1, 1]
    seen.clear()
    b = _module_step(gpu, auto, True, cp=True, conv=False)
    assert [seen.count(n) for n in NEW] == [2, 1]
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ 4. edges

@pytest.mark.parametrize('prec,layout', [('f32', 'nchw'), ('f16', 'nhwc'), ('bf16', 'nchw')])
def test_no_valid_voxel_gives_the_reference_losses_and_zero_gradients(gpu, prec, layout):
    v = _on(gpu, 'tails', prec, layout)
    for name, over in (('empty mask', dict(cam=torch.zeros_like(v['cam']))), ('all ignored', dict(sem=torch.full_like(v['sem'], OL.IGNORE)))):
        got = _step(v, **over)
        l = got['losses'].cpu().tolist()
        assert math.isnan(l[0]) and math.isnan(l[1]) and abs(l[2] - NO_VALID[2]) <= LOSS_BAR * NO_VALID[2], (name, l)
        for k in OT.TENSORS:
            assert not bool(got[k].any()), (name, k)


@pytest.mark.parametrize('prec,layout', [('f32', 'nhwc'), ('bf16', 'nchw')])
def test_a_nan_counts_only_in_a_valid_voxel(gpu, prec, layout):
    v = _on(gpu, 'tails', prec, layout)
    bi, iy, ix = 0, 13, 27
    x = v['x'].clone()
    x[bi, 100, iy, ix] = float('nan')
    cam = v['cam'].clone()
    cam[bi, ix, iy] = False                                                     # every voxel of that cell masked out
    clean = _forward(v, cam=cam)[1]
    hidden = _forward(v, x=x, cam=cam)[1]
    assert bool(torch.isfinite(hidden).all()) and _same(hidden, clean)
    cam[bi, ix, iy, 3] = True
    sem = v['sem'].clone()
    sem[bi, ix, iy, 3] = 2
    assert bool(torch.isnan(_forward(v, x=x, cam=cam, sem=sem)[1]).all())


@pytest.mark.parametrize('case,prec,layout', SMALL)
def test_frozen_parameters_write_no_operand_and_the_same_dx(gpu, monkeypatch, case, prec, layout):
    from dhd_amd import occ_head
    v = _on(gpu, case, prec, layout)
    with_ops, without = _backward(v, True), _backward(v, False)
    assert without['act'] is None and without['dhid'] is None and (without['g'] is None) == (prec != 'f32')
    assert all(with_ops[k] is not None for k in ('act', 'dhid', 'g'))
    for k in ('dx', 'db1', 'db2'):
        assert _same(with_ops[k], without[k]), k
    wanted, real = [], occ_head.occ_head_loss_backward
    monkeypatch.setattr(occ_head, 'occ_head_loss_backward', lambda *a, **k: (wanted.append(k.get('operands')), real(*a, **k))[1])
    for grads, want in (((True, False, True, False, True), False), ((True, True, False, False, False), True),
                        ((False, False, False, True, False), True), ((True, False, False, False, False), False)):
        got = _step(v, grads=grads)
        assert wanted.pop() is want and not wanted
        assert [got[k] is not None for k in OT.TENSORS] == list(grads)
        if grads[0]:
            assert _same(got['dx'], with_ops['dx'])


def test_the_fp16_loss_scale_arrives_through_the_upstream_gradient(gpu):
    v, ref, scale = _on(gpu, 'tails', 'f16', 'nchw'), OL.twin('tails', 'f16'), OT.fp16_loss_scale()
    plain, scaled, par = _step(v), _step(v, scale=scale), _step(v, fused=False, scale=scale)
    failures = []
    for k in OT.TENSORS:
        err, perr, uerr = _err(scaled[k], ref[k]), _err(par[k], ref[k]), _err(plain[k], ref[k])
        print(f'fp16, loss scale {scale:g}, {k}: scaled {err:.3e}, unscaled {uerr:.3e}, parent scaled {perr:.3e}, ratio {err / perr if perr else float("inf"):.3f}')
        if not (perr > 0 and err <= MARGIN * perr and bool(torch.isfinite(scaled[k]).all())):
            failures.append(k)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ 5. reproducibility and plumbing

@pytest.mark.parametrize('case,prec,layout', SMALL)
def test_two_calls_give_the_same_bytes(gpu, case, prec, layout):
    v = _on(gpu, case, prec, layout)
    a, b = _backward(v), _backward(v)
    for k in a:
        assert _same(a[k], b[k]), k
        assert k in ('ws',) or a[k] is None or bool(torch.isfinite(a[k]).all()), k


@pytest.mark.parametrize('case,prec,layout', SMALL + [pytest.param('one_cell', 'bf16', 'nchw', id='one_cell-bf16-nchw')])
def test_inside_guard_bands(gpu, monkeypatch, case, prec, layout):
    """Every buffer the wrappers allocate (forward: scratch, logits, losses, workspace; backward: dx, db1, db2, act, dhid, g,
    scratch) between two guard bands at its advertised size, every byte 0xFF: no guard byte changes and the runs agree."""
    v = _on(gpu, case, prec, layout)
    before = {k: t.clone() for k, t in v.items()}
    plain = _backward(v)
    with G.guarded(monkeypatch, 0xFF) as ledger:
        got = _backward(v)
        ledger.check()
        got = {k: None if t is None else t.detach().clone() for k, t in got.items()}
    ours = [e for e in ledger.sites_under(G.PRODUCT_ROOT) if 'occ_head.py' in e.site]
    print(f'{case} [{prec}, {layout}]: {len(ledger)} guarded allocations, {ledger.total_bytes()} bytes, guards intact')
    assert len(ours) == 11
    for k, t in got.items():
        assert _same(t, plain[k]), k
    for k, t in v.items():
        assert _same(t, before[k]), k


@pytest.mark.parametrize('prec,layout', [('f32', 'nchw'), ('bf16', 'nhwc'), ('f16', 'nchw')])
def test_strided_offset_and_misaligned_views_give_the_dense_result(gpu, prec, layout):
    v = _on(gpu, 'two_groups', prec, layout)
    want = _step(v)
    x, sem, cam = v['x'], v['sem'], v['cam']
    big = OT.in_layout(torch.zeros(x.shape[0] + 1, x.shape[1], x.shape[2] + 2, x.shape[3] + 3, dtype=x.dtype, device=gpu), layout)
    big[1:, :, 1:-1, 2:-1] = x
    flat = torch.zeros(x.numel() + 1, dtype=x.dtype, device=gpu)
    flat[1:] = x.reshape(-1) if layout == 'nchw' else x.permute(0, 2, 3, 1).reshape(-1)
    mis = flat[1:].view(x.shape) if layout == 'nchw' else flat[1:].view(x.shape[0], x.shape[2], x.shape[3], x.shape[1]).permute(0, 3, 1, 2)

    def strided(t):
        wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=gpu)
        wide[..., ::2] = t
        return wide[..., ::2]

    def offset(t):
        buf = torch.zeros(t.numel() + 3, dtype=t.dtype, device=gpu)
        buf[3:] = t.reshape(-1)
        return buf[3:].view(t.shape)
    for name, over in (('strided', dict(x=big[1:, :, 1:-1, 2:-1], sem=strided(sem), cam=strided(cam))),
                       ('misaligned', dict(x=mis, sem=offset(sem), cam=offset(cam)))):
        assert all(torch.equal(over[k], v[k]) for k in over) and (name != 'misaligned' or all(t.data_ptr() % 8 for t in over.values()))
        got = _step(v, **over)
        for k in got:
            assert torch.equal(got[k], want[k]), (name, k)


@pytest.mark.parametrize('prec,layout', [('f32', 'nchw'), ('bf16', 'nhwc')])
def test_forward_and_backward_captured_into_one_graph(gpu, prec, layout):
    import dhd_amd
    v = _on(gpu, 'partial_wave', prec, layout)
    want = _step(v)
    leaves = [v[k].detach().clone().requires_grad_() for k in ('x',) + OT.PARAMS]
    up = torch.tensor(OL.WEIGHTS, dtype=F32, device=gpu)

    def run():
        losses = torch.stack(dhd_amd.occ_head_losses(*leaves, v['sem'], v['cam'], v['cw'], dz=OT.DZ))
        return (losses,) + torch.autograd.grad(losses, leaves, up)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    _sync()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for t in outs:
        t.zero_()
    graph.replay()
    _sync()
    for k, t in zip(('losses',) + OT.TENSORS, outs):
        assert torch.equal(t, want[k]), k
