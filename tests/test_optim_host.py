"""dhd_amd.optim without a GPU: the CPU path of FusedAdamW holds the semantics of the fused step (the same mathematics through
torch ops) against clip_grad_norm_ + torch.optim.AdamW + ModelEMA.update, the state dict moves between the two classes in both
directions, a non-finite gradient skips the step while the EMA advances, the loss-scale rule is torch._amp_update_scale_'s,
the chunk table is planned as the kernels expect it, and build_optimizer reads the reference's config dicts."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

import dhd_amd
from dhd_amd import _optim
from dhd_amd.optim import CHUNK, DynamicLossScale, FusedAdamW, build_optimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_step_inputs as OS  # noqa: E402

GOLDEN_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g18_configs.json')
MAX_NORM = 5.0


class Net(nn.Module):
    """Two Linear layers and a BatchNorm (buffers: the EMA's tensors that no optimizer owns), one frozen parameter and one that
    never gets a gradient."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.a = nn.Linear(7, 5)
        self.bn = nn.BatchNorm1d(5)
        self.b = nn.Linear(5, 3)
        self.frozen = nn.Parameter(torch.randn(4), requires_grad=False)
        self.unused = nn.Parameter(torch.randn(6))


def _grads(net, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    for n, p in net.named_parameters():
        if p.requires_grad and n != 'unused':
            p.grad = torch.randn(p.shape, generator=g) * scale


def _groups(net):
    rest = [p for n, p in net.named_parameters() if p.requires_grad and not n.startswith('a.')]
    return [dict(params=list(net.a.parameters()), lr=3e-3, weight_decay=0.0), dict(params=rest)]


HYPERS = [dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0), dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)]


def _trainable(net):
    return [p for p in net.parameters() if p.requires_grad]


def _twin(net, max_norm):
    return OS.Twin64(_trainable(net), [0 if n.startswith('a.') else 1 for n, p in net.named_parameters() if p.requires_grad], HYPERS, max_norm)


def _err(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def test_cpu_path_equals_clip_adamw_and_ema_over_three_steps():
    """Three steps with clipping active, two groups, an EMA: after every step p, exp_avg, exp_avg_sq and the norm are within
    the bar of optim_step_inputs against the float64 twin, E_torch being clip_grad_norm_ + AdamW(foreach=False) on the same
    gradients.  The tensors no optimizer owns (buffers, the frozen parameter) go through ModelEMA's own expression and have
    the same bits as after ModelEMA.update; the EMA of the parameters is held bit for bit further down, against a run of the
    same optimizer without ema= followed by ModelEMA.update."""
    ours, theirs = Net(), Net()
    twin = _twin(ours, MAX_NORM)
    ema_o, ema_t = dhd_amd.ModelEMA(ours, updates=100), dhd_amd.ModelEMA(theirs, updates=100)
    opt = FusedAdamW(_groups(ours), lr=2e-3, weight_decay=1e-2, max_norm=MAX_NORM, ema=ema_o, model=ours)
    ref = torch.optim.AdamW(_groups(theirs), lr=2e-3, weight_decay=1e-2, foreach=False)
    for it in range(3):
        _grads(ours, it, 4.0)
        _grads(theirs, it, 4.0)
        with torch.no_grad():
            ours.bn.running_mean += 0.1 * (it + 1)       # a buffer moves: the EMA follows it through update_rest
            theirs.bn.running_mean += 0.1 * (it + 1)
        twin.step([p.grad for p in _trainable(ours)])
        opt.step()
        norm = torch.nn.utils.clip_grad_norm_([p for p in theirs.parameters() if p.grad is not None], MAX_NORM)
        ref.step()
        ema_t.update(None, theirs)
        rec = opt.last_record()
        assert float(norm) > MAX_NORM and rec['coef'] < 1.0 and not rec['found_inf'] and opt.grad_norm() == rec['norm']
        OS.check_bar(f'step {it}', (opt, _trainable(ours)), (ref, _trainable(theirs)), twin, rec['norm'], float(norm))
        assert ema_o.updates == ema_t.updates == 101 + it
    assert torch.equal(ours.frozen, theirs.frozen) and torch.equal(ours.unused, theirs.unused)
    assert ours.unused not in opt.state and all(float(opt.state[p]['step']) == 3 for p in ours.a.parameters())
    assert torch.equal(ema_o.ema.bn.running_mean, ema_t.ema.bn.running_mean) and torch.equal(ema_o.ema.frozen, ema_t.ema.frozen)
    assert torch.equal(ema_o.ema.bn.num_batches_tracked, ema_t.ema.bn.num_batches_tracked)
    # the EMA arithmetic itself, bit for bit: a run without ema= followed by ModelEMA.update
    a, b = Net(), Net()
    ema_a, ema_b = dhd_amd.ModelEMA(a, updates=7), dhd_amd.ModelEMA(b, updates=7)
    opt_a = FusedAdamW(_groups(a), max_norm=MAX_NORM, ema=ema_a, model=a)
    opt_b = FusedAdamW(_groups(b), max_norm=MAX_NORM)
    for it in range(3):
        _grads(a, it, 4.0)
        _grads(b, it, 4.0)
        opt_a.step()
        opt_b.step()
        ema_b.update(None, b)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    assert all(torch.equal(x, y) for x, y in zip(ema_a.ema.state_dict().values(), ema_b.ema.state_dict().values()))


def test_without_clipping_and_without_ema_the_step_is_adamw():
    ours, theirs = Net(), Net()
    twin = _twin(ours, None)
    opt = FusedAdamW(_groups(ours), lr=2e-3, weight_decay=1e-2)
    ref = torch.optim.AdamW(_groups(theirs), lr=2e-3, weight_decay=1e-2, foreach=False)
    for it in range(3):
        _grads(ours, it)
        _grads(theirs, it)
        twin.step([p.grad for p in _trainable(ours)])
        opt.step()
        ref.step()
        assert opt.last_record()['coef'] == 1.0
        OS.check_bar(f'step {it}', (opt, _trainable(ours)), (ref, _trainable(theirs)), twin)


def test_state_dict_round_trip_both_ways_with_a_further_step():
    ours, theirs = Net(), Net()
    opt = FusedAdamW(_groups(ours), lr=2e-3, weight_decay=1e-2, max_norm=MAX_NORM)
    ref = torch.optim.AdamW(_groups(theirs), lr=2e-3, weight_decay=1e-2, foreach=False)
    twin = _twin(ours, MAX_NORM)

    def both(it):
        _grads(ours, it)
        _grads(theirs, it)
        twin.step([p.grad for p in _trainable(ours)])
        opt.step()
        torch.nn.utils.clip_grad_norm_([p for p in theirs.parameters() if p.grad is not None], MAX_NORM)
        ref.step()
    both(0)
    both(1)
    sd = opt.state_dict()
    assert set(sd) == {'state', 'param_groups'} and set(sd['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'}
    assert set(sd['param_groups'][0]) == set(ref.state_dict()['param_groups'][0])
    assert sd['state'][0]['step'].dtype == torch.float32 and sd['state'][0]['step'].device.type == 'cpu' and float(sd['state'][0]['step']) == 2
    # ours -> torch's: a fresh AdamW continues from our state as from its own
    fresh_ref = torch.optim.AdamW(_groups(theirs), lr=1.0, foreach=False)
    fresh_ref.load_state_dict(copy.deepcopy(sd))
    ref = fresh_ref
    # torch's -> ours
    fresh = FusedAdamW(_groups(ours), lr=1.0, max_norm=MAX_NORM)
    fresh.load_state_dict(copy.deepcopy(ref.state_dict()))
    opt = fresh
    assert opt.param_groups[0]['lr'] == 3e-3 and opt.param_groups[1]['lr'] == 2e-3
    both(2)
    assert all(float(opt.state[p]['step']) == 3 for p in ours.a.parameters())
    OS.check_bar('after the round trip', (opt, _trainable(ours)), (ref, _trainable(theirs)), twin)
    with pytest.raises(ValueError):
        bad = copy.deepcopy(ref.state_dict())
        bad['param_groups'][0]['amsgrad'] = True
        FusedAdamW(_groups(ours)).load_state_dict(bad)


@pytest.mark.parametrize('poison', [float('inf'), float('nan')])
def test_a_non_finite_gradient_skips_the_step_and_the_ema_advances(poison):
    net = Net()
    ema, twin = dhd_amd.ModelEMA(net, updates=50), dhd_amd.ModelEMA(net, updates=50)
    scale = DynamicLossScale(init_scale=1024., growth_interval=2)
    opt = FusedAdamW(_groups(net), lr=2e-3, max_norm=MAX_NORM, ema=ema, model=net, loss_scale=scale)
    loss = scale.scale(torch.tensor(2.0))
    assert float(loss) == 2048.0
    _grads(net, 0, 1024.0)
    opt.step()
    assert not opt.last_record()['found_inf'] and scale.get_scale() == 1024.0
    twin.update(None, net)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    state = {p: {k: v.clone() for k, v in st.items()} for p, st in opt.state.items()}
    _grads(net, 1, 1024.0)
    net.b.weight.grad[1, 2] = poison
    opt.step()
    rec = opt.last_record()
    assert rec['found_inf'] and rec['scale'] == 512.0 and scale.get_scale() == 512.0 and scale.state_dict()['_growth_tracker'] == 0
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    assert all(torch.equal(st[k], state[p][k]) for p, st in opt.state.items() for k in st)
    twin.update(None, net)                      # what ModelEMA.update after a skipped scaler.step does today
    assert ema.updates == twin.updates == 52
    assert all(torch.equal(a, b) for a, b in zip(ema.ema.state_dict().values(), twin.ema.state_dict().values()))
    # two clean steps: the scale grows after growth_interval = 2
    for it, want in ((2, 512.0), (3, 1024.0)):
        _grads(net, it, 512.0)
        opt.step()
        assert not opt.last_record()['found_inf'] and scale.get_scale() == want
    assert all(float(opt.state[p]['step']) == 3 for p in net.a.parameters())


def test_the_scale_rule_is_amp_update_scale():
    rule = getattr(torch, '_amp_update_scale_')
    ours = DynamicLossScale(init_scale=2.0 ** 10, growth_factor=3.0, backoff_factor=0.25, growth_interval=3, device='cpu')
    s, tracker = torch.full((), 2.0 ** 10), torch.zeros((), dtype=torch.int32)
    for found in (0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0):
        ours._host_update(bool(found))
        rule(s, tracker, torch.tensor(float(found)), 3.0, 0.25, 3)
        assert ours.get_scale() == float(s) and ours.state_dict()['_growth_tracker'] == int(tracker)
    big = DynamicLossScale(init_scale=3e38, growth_interval=1, device='cpu')
    big._host_update(False)
    assert big.get_scale() == float(torch.tensor(3e38))                   # growth that would overflow is not taken
    sd = ours.state_dict()
    assert set(sd) == set(torch.amp.GradScaler('cpu').state_dict())
    other = DynamicLossScale()
    other.load_state_dict(sd)
    assert other.state_dict() == sd
    with pytest.raises(ValueError):
        DynamicLossScale(growth_factor=1.0)


def test_what_is_not_supported_raises():
    p = [nn.Parameter(torch.zeros(3))]
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(norm_type=1), dict(norm_type=float('inf')), dict(max_norm=-1.0),
               dict(ema=object()), dict(lr=-1.0), dict(betas=(1.0, 0.9))):
        with pytest.raises(ValueError):
            FusedAdamW(p, **kw)
    opt = FusedAdamW(p)
    opt.param_groups[0]['lr'] = torch.tensor(1e-3)
    p[0].grad = torch.ones(3)
    with pytest.raises(ValueError):
        opt.step()


class _Fake:
    """What chunk planning looks at of a tensor: address, size, strides, dtype."""

    def __init__(self, addr, n, dtype=torch.float32):
        self.addr, self.n, self.dtype = addr, n, dtype

    def data_ptr(self):
        return self.addr

    def numel(self):
        return self.n


def test_chunk_rows():
    """Lengths, offsets, groups and slots of the table, against the loop ModelEMA's _ChunkTable is."""
    sizes = [1, 3, CHUNK - 1, CHUNK, CHUNK + 1, 200001, 0, 3 * CHUNK]
    entries = []
    for i, n in enumerate(sizes):
        base = 0x100000000 * (i + 1)
        ema = None if i % 2 else _Fake(base + 0x40000000, n)
        half = None if i % 3 else (None, _Fake(base + 0x50000000, n, torch.float16 if i % 2 else torch.bfloat16))
        entries.append((i % 2, 10 + i, _Fake(base, n), _Fake(base + 0x10000000, n), _Fake(base + 0x20000000, n), _Fake(base + 0x30000000, n),
                        ema, half))
    rows = FusedAdamW.chunk_rows(entries)
    assert rows.dtype == _optim.CHUNK_DTYPE and rows.flags['C_CONTIGUOUS']
    want = []
    for gi, slot, p, g, m, v, e, h in entries:
        for off in range(0, p.n, CHUNK):
            want.append((p.addr + 4 * off, g.addr + 4 * off, m.addr + 4 * off, v.addr + 4 * off, 0 if e is None else e.addr + 4 * off,
                         0 if h is None else h[1].addr + 2 * off, min(CHUNK, p.n - off), gi, 0 if h is None else {torch.float16: 1, torch.bfloat16: 2}[h[1].dtype], slot))
    assert [tuple(int(x) for x in r) for r in rows.tolist()] == want and len(want) == 1 + 1 + 1 + 1 + 2 + 4 + 0 + 3
    assert int(rows['len'].sum()) == sum(sizes) and rows['len'].min() >= 1 and rows['len'].max() == CHUNK
    assert len(FusedAdamW.chunk_rows([])) == 0


def test_planning_the_fallback_set():
    """On CPU tensors plan() sorts as it does on the GPU: dense in the parameter's own layout with gradient, state and copies
    -> the table; anything else -> the torch path."""
    torch.manual_seed(0)
    flat = torch.randn(40)
    ps = [nn.Parameter(torch.randn(5)),                                                      # 0 plain
          nn.Parameter(torch.randn(8, 4, 3, 3).contiguous(memory_format=torch.channels_last)),    # 1 channels_last, gradient too
          nn.Parameter(torch.randn(8, 4, 3, 3).contiguous(memory_format=torch.channels_last)),    # 2 channels_last, contiguous gradient
          nn.Parameter(flat[1:13].view(3, 4)),                                               # 3 one element into a buffer: dense
          nn.Parameter(torch.randn(6, 4)[:, ::2]),                                           # 4 strided
          nn.Parameter(torch.randn(4, 4)),                                                   # 5 transposed gradient
          nn.Parameter(torch.randn(3))]                                                      # 6 no gradient
    for i, p in enumerate(ps[:6]):
        p.grad = torch.randn(p.shape)
    ps[1].grad = torch.randn(8, 4, 3, 3).contiguous(memory_format=torch.channels_last)
    ps[5].grad = torch.randn(4, 4).t()
    opt = FusedAdamW(ps)
    active = [(gi, slot, p) for gi, slot, p in opt._slots() if p.grad is not None]
    assert [slot for _, slot, _ in active] == [0, 1, 2, 3, 4, 5]
    table, fallback = opt.plan(active, {}, {})
    assert [e[1] for e in table] == [0, 1, 3] and [e[1] for e in fallback] == [2, 4, 5]
    assert opt.state[ps[1]]['exp_avg'].stride() == ps[1].stride()                           # the state takes the parameter's layout
    # strides of dimensions of size 1 address nothing: an (O, I, 1, 1) weight in either convention with a gradient in the other
    cl = lambda: torch.empty(6, 4, 1, 1, memory_format=torch.channels_last).normal_()       # strides (4, 1, 4, 4)
    one = [nn.Parameter(torch.randn(6, 4, 1, 1)), nn.Parameter(cl())]
    one[0].grad = cl()
    one[1].grad = torch.randn(6, 4, 1, 1)
    assert one[0].stride() != one[0].grad.stride() and one[1].stride() != one[1].grad.stride()
    o1 = FusedAdamW(one)
    assert [len(x) for x in o1.plan([(0, 0, one[0]), (0, 1, one[1])], {}, {})] == [2, 0]
    # an EMA copy or a half copy in another layout sends the tensor to the torch path as well
    e = {id(ps[1]): torch.zeros(8, 4, 3, 3)}
    assert [x[1] for x in opt.plan(active, e, {})[1]] == [1, 2, 4, 5]
    with pytest.raises(dhd_amd._lib.DhdError):
        opt.plan(active, {id(ps[0]): torch.zeros(5, dtype=torch.float64)}, {})
    # ... and the torch path computes the same update whatever the strides
    ref = [nn.Parameter(p.detach().clone()) for p in ps]
    for p, q in zip(ps, ref):
        q.grad = None if p.grad is None else p.grad.clone()
    opt.step()
    torch.optim.AdamW(ref, foreach=False).step()
    assert all(_err(p, q) <= 2 ** -21 for p, q in zip(ps, ref))


def test_the_key_changes_only_when_an_address_or_a_layout_does():
    ps = [nn.Parameter(torch.randn(5)), nn.Parameter(torch.randn(2, 3))]
    opt = FusedAdamW(ps)
    for p in ps:
        p.grad = torch.randn(p.shape)
        opt._init_state(p, 0)
    active = [(0, i, p) for i, p in enumerate(ps)]
    k0 = opt._key(active, {}, {})
    for p in ps:
        p.grad.mul_(2.0)                        # values change, addresses stay
    assert opt._key(active, {}, {}) == k0
    keep = ps[1].grad                           # (kept alive: the allocator must not hand the same block out again)
    ps[1].grad = torch.randn(2, 3)              # zero_grad(set_to_none=True) + backward: a new tensor
    assert opt._key(active, {}, {}) != k0
    ps[1].grad = keep
    assert opt._key(active, {}, {}) == k0
    assert opt._key(active, {id(ps[0]): torch.zeros(5)}, {}) != k0 and opt._key(active[:1], {}, {}) != k0
    opt.state[ps[0]]['exp_avg'] = torch.zeros(5)
    assert opt._key(active, {}, {}) != k0


def test_build_optimizer_on_the_reference_config():
    from dhd_amd.config import Config, _wrap
    with open(GOLDEN_CFG) as f:
        rec = json.load(f, object_hook=lambda d: tuple(d['__tuple__']) if set(d) == {'__tuple__'} else d)['DHD-S']
    cfg = Config(_wrap(rec))
    assert dict(cfg.optimizer) == dict(type='AdamW', lr=2e-4, weight_decay=1e-2)
    assert {k: dict(v) for k, v in dict(cfg.optimizer_config).items()} == dict(grad_clip=dict(max_norm=5, norm_type=2))
    net = Net()
    plain = build_optimizer(net, cfg.optimizer, cfg.optimizer_config)
    assert type(plain) is torch.optim.AdamW and plain.defaults['lr'] == 2e-4 and plain.defaults['weight_decay'] == 1e-2
    n_trainable = sum(p.requires_grad for p in net.parameters())
    assert len(plain.param_groups[0]['params']) == n_trainable
    ema = dhd_amd.ModelEMA(net)
    fused = build_optimizer(net, cfg.optimizer, cfg.optimizer_config, fused=True, ema=ema)
    assert type(fused) is FusedAdamW is dhd_amd.FusedAdamW and fused.max_norm == 5.0 and fused.model is net and fused.ema is ema
    assert fused.defaults['lr'] == 2e-4 and fused.defaults['weight_decay'] == 1e-2 and fused.defaults['betas'] == (0.9, 0.999)
    assert len(fused.param_groups[0]['params']) == n_trainable and dict(cfg.optimizer)['type'] == 'AdamW'     # the dict is not consumed
    assert build_optimizer(net, cfg.optimizer, None, fused=True).max_norm is None
    with pytest.raises(ValueError):
        build_optimizer(net, dict(type='SGD', lr=0.1))
    with pytest.raises(ValueError):
        build_optimizer(net, cfg.optimizer, dict(grad_clip=dict(max_norm=5, norm_type=1)), fused=True)
    assert dhd_amd.DynamicLossScale is DynamicLossScale and dhd_amd.build_optimizer is build_optimizer
