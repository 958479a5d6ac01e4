"""FusedAdamW on the GPU (dhd_amd/optim.py over csrc/optim_step.h): one small state that holds every path of the three kernels --

  * flat tensors of 1, 3, 4, 5, 1023, 4095, 4096, 4097, 65 535, 65 536, 65 537 and 200 001 elements: the 16-byte tail, the
    unrolled loop's 4096-element stride and the chunk boundary on both sides;
  * a channels_last (8, 4, 3, 3) weight whose gradient is channels_last too (the table), and one whose gradient is contiguous
    (the torch path with device scalars);
  * a parameter, and separately a gradient, an EMA tensor and a half copy, that start one element into a flat buffer (the
    kernels' single-element path);
  * a parameter whose grad is None, a frozen parameter and a buffer (the EMA's own sweep);
  * two groups with different lr and weight decay

-- against the float64 twin and the bar of optim_step_inputs, and bit for bit where the issue says bits: the EMA against
ModelEMA.update, the half copies against p.to(dtype), a skipped step, a captured step against eager steps, two identical runs,
and one pass inside guard bands."""
import math
import os
import sys

import pytest
import torch
from torch import nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as G  # noqa: E402
import optim_step_inputs as OS  # noqa: E402

ME = os.path.abspath(__file__)
SIZES = (1, 3, 4, 5, 1023, 4095, 4096, 4097, 65535, 65536, 65537, 200001)
MAX_NORM = 5.0
LRS = (3e-3, 1e-3)
ENTRIES = ('dhdw_optim_grad_norm', 'dhdw_optim_finalize', 'dhdw_optim_adamw_update')


def _new(gpu, values, offset=0, channels_last=False):
    """`values` (a CPU tensor) in fresh device memory obtained through torch.empty -- inside guard bands in the guarded test --
    starting `offset` elements into its buffer."""
    if channels_last:
        t = torch.empty(values.shape, dtype=values.dtype, device=gpu, memory_format=torch.channels_last)
    else:
        t = torch.empty(values.numel() + offset, dtype=values.dtype, device=gpu)[offset:].view(values.shape)
    t.copy_(values)
    return t


class Model(nn.Module):
    def __init__(self, gpu, seed=0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        r = lambda *shape: torch.randn(shape, generator=gen)
        self.flat = nn.ParameterList([nn.Parameter(_new(gpu, r(n))) for n in SIZES])
        self.off = nn.Parameter(_new(gpu, r(4099), offset=1))          # the parameter itself one element into a buffer
        self.goff = nn.Parameter(_new(gpu, r(4099)))                   # ... its gradient
        self.eoff = nn.Parameter(_new(gpu, r(777)))                    # ... its EMA copy
        self.conv = nn.Conv2d(4, 8, 3, bias=False)
        self.conv.weight = nn.Parameter(_new(gpu, r(8, 4, 3, 3), channels_last=True))
        self.conv2 = nn.Conv2d(4, 8, 3, bias=False)                    # channels_last weight, contiguous gradient: the torch path
        self.conv2.weight = nn.Parameter(_new(gpu, r(8, 4, 3, 3), channels_last=True))
        self.lin = nn.Linear(33, 17)
        self.lin.weight, self.lin.bias = nn.Parameter(_new(gpu, r(17, 33))), nn.Parameter(_new(gpu, r(17)))
        self.hoff = nn.Linear(40, 25, bias=False)                      # ... its half copy
        self.hoff.weight = nn.Parameter(_new(gpu, r(25, 40)))
        self.none = nn.Parameter(_new(gpu, r(7)))                      # never gets a gradient
        self.frozen = nn.Parameter(_new(gpu, r(9)), requires_grad=False)
        self.register_buffer('running', _new(gpu, r(5)))

    def trainable(self):
        return [p for p in self.parameters() if p.requires_grad]

    def groups(self, wd):
        flat = list(self.flat)
        rest = [p for p in self.trainable() if not any(p is q for q in flat)]
        return [dict(params=flat, lr=LRS[0], weight_decay=wd), dict(params=rest, lr=LRS[1], weight_decay=5e-3)]

    def group_of(self):
        return [0 if any(p is q for q in self.flat) else 1 for p in self.trainable()]

    def grad_values(self, seed, scale):
        """Per trainable parameter the gradient of step `seed` as a CPU tensor, None for `none`."""
        gen = torch.Generator().manual_seed(1000 + seed)
        return [None if p is self.none else torch.randn(p.shape, generator=gen) * scale for p in self.trainable()]

    def set_grads(self, values, plain=False):
        """Fresh gradient tensors, as after zero_grad(set_to_none=True) and a backward.  plain: all of them aligned and in the
        parameter's layout (the torch reference's copy)."""
        gpu = self.goff.device
        for p, v in zip(self.trainable(), values):
            if v is None:
                p.grad = None
            elif p is self.conv.weight or (plain and p is self.conv2.weight):
                p.grad = _new(gpu, v, channels_last=True)
            else:
                p.grad = _new(gpu, v, offset=1 if (p is self.goff and not plain) else 0)


def _hypers(wd):
    return [dict(lr=LRS[0], betas=(0.9, 0.999), eps=1e-8, weight_decay=wd), dict(lr=LRS[1], betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-3)]


class Run:
    """A Model with a FusedAdamW over it and, on request, the EMA (one EMA tensor moved one element into a buffer), the half
    cache (one copy moved likewise) and the loss scale."""

    def __init__(self, gpu, wd=1e-2, max_norm=MAX_NORM, ema=False, half=None, scale=None, updates=300):
        import dhd_amd
        self.model = Model(gpu)
        self.ema = self.cache = None
        if ema:
            self.ema = dhd_amd.ModelEMA(self.model, updates=updates)
            self.ema.ema.eoff.data = _new(gpu, self.ema.ema.eoff.detach().cpu(), offset=1)
        if half is not None:
            self.cache = dhd_amd.HalfWeightCache(self.model, half)
            assert len(self.cache) == 4
            self.model.hoff._dhd_w16 = _new(gpu, self.model.hoff._dhd_w16.cpu(), offset=1)
        self.scale = scale
        self.opt = dhd_amd.FusedAdamW(self.model.groups(wd), max_norm=max_norm, ema=self.ema if ema == 'fused' else None, model=self.model,
                                      half_cache=self.cache, loss_scale=scale)
        self.fused_ema = ema == 'fused'

    def step(self, seed, grad_scale, poison=None):
        values = self.model.grad_values(seed, grad_scale)
        if poison is not None:
            at = next(i for i, p in enumerate(self.model.trainable()) if p is self.model.flat[7])
            values[at].view(-1)[4000] = poison         # one element of the 4097-element tensor: the tail of the unrolled loop
        self.model.set_grads(values)
        self.opt.step()
        if self.ema is not None and not self.fused_ema:
            self.ema.update(None, self.model)
        return values

    def bytes(self):
        """Every tensor the step may write, as bytes: parameters, buffers, state, the EMA's state, the half copies."""
        out = {'model.' + k: v for k, v in self.model.state_dict().items()}
        for i, p in enumerate(self.model.trainable()):
            for k, v in self.opt.state.get(p, {}).items():
                out[f'state{i}.{k}'] = v
        if self.ema is not None:
            out.update({'ema.' + k: v for k, v in self.ema.ema.state_dict().items()})
        if self.cache is not None:
            out.update({f'half{i}': m._dhd_w16 for i, m in enumerate(self.cache.modules)})
        return {k: v.detach().clone().contiguous().view(-1).view(torch.uint8).cpu() for k, v in out.items()}


def _same(a, b, keys=None):
    assert set(a) == set(b)
    return [k for k in (keys or a) if not torch.equal(a[k], b[k])]


@pytest.mark.gpu
@pytest.mark.parametrize('wd', [0.0, 1e-2])
@pytest.mark.parametrize('grad_scale', [1.0, 1e-3], ids=['clipped', 'not_clipped'])
def test_three_steps_against_the_float64_twin(gpu, wd, grad_scale):
    """p, exp_avg, exp_avg_sq and the norm after each of three steps: E_fused <= 1.5 E_torch + 2^-23 against the float64 twin,
    E_torch from clip_grad_norm_ + AdamW(foreach=True) on the same device with the same gradients."""
    run = Run(gpu, wd=wd)
    ref_model = Model(gpu)
    ref = torch.optim.AdamW(ref_model.groups(wd), foreach=True)
    twin = OS.Twin64(run.model.trainable(), run.model.group_of(), _hypers(wd), MAX_NORM)
    assert run.opt.rebuilds == 0
    for it in range(3):
        values = run.step(it, grad_scale)
        ref_model.set_grads(values, plain=True)
        norm = torch.nn.utils.clip_grad_norm_([p for p in ref_model.parameters() if p.grad is not None], MAX_NORM)
        ref.step()
        twin.step(values)
        rec = run.opt.last_record()
        assert (rec['norm'] > MAX_NORM) == (grad_scale == 1.0) == (rec['coef'] < 1.0) and not rec['found_inf']
        OS.check_bar(f'wd {wd} grads x{grad_scale} step {it}', (run.opt, run.model.trainable()), (ref, ref_model.trainable()), twin,
                     rec['norm'], float(norm))
    assert run.opt.rebuilds == 3                                  # fresh gradient tensors every step: a rebuild every step
    assert [e[2] is run.model.conv2.weight for e in run.opt._table.fallback] == [True]
    assert run.model.none not in run.opt.state and torch.equal(run.model.frozen, ref_model.frozen)
    steps = {float(run.opt.state[p]['step']) for p in run.model.trainable() if p is not run.model.none}
    assert steps == {3.0}
    # gradients that stay in place: no rebuild
    run.opt.step()
    assert run.opt.rebuilds == 3


@pytest.mark.gpu
def test_the_ema_is_bit_equal_to_model_ema_update(gpu):
    """ema= against a run without it followed by ModelEMA.update: parameters, state and every EMA tensor bit for bit -- the
    tensors in the table, the one on the torch path, the one a buffer offset puts on the single-element path, the buffer and
    the frozen and gradient-less parameters that ModelEMA.update_rest sweeps."""
    a, b = Run(gpu, ema='fused'), Run(gpu, ema='after')
    for it in range(3):
        a.step(it, 1.0)
        b.step(it, 1.0)
        with torch.no_grad():
            a.model.running += 0.25
            b.model.running += 0.25
    assert a.ema.updates == b.ema.updates == 303
    assert _same(a.bytes(), b.bytes()) == []
    start = Model(gpu).state_dict()
    for k in ('flat.0', 'flat.11', 'off', 'goff', 'eoff', 'conv.weight', 'conv2.weight', 'lin.bias', 'running'):
        assert not torch.equal(a.ema.ema.state_dict()[k], start[k]), k          # ... and they did move


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['fp16', 'bf16'])
def test_half_copies_are_the_rounded_parameters_and_routed_layers_take_them(gpu, dtype):
    from dhd_amd import amp_weights
    run = Run(gpu, half=dtype)
    run.step(0, 1.0)
    run.step(1, 1e-3)
    for m in run.cache.modules:
        assert m._dhd_w16.dtype == dtype and torch.equal(m._dhd_w16, m.weight.to(dtype)), type(m).__name__
    assert not torch.equal(run.model.lin._dhd_w16, Model(gpu).lin.weight.to(dtype))                  # (the weights did move)
    assert run.model.hoff._dhd_w16.data_ptr() % 16 == 2 and run.model.conv2 in run.cache.modules      # the offset copy, the torch path's copy
    x = torch.randn(6, 33, device=gpu)
    with torch.autocast('cuda', dtype=dtype):
        assert amp_weights._half_of(run.model.lin, x) is not None                                     # the copy is current: the layer is routed
        y = run.model.lin(x)
        want = F.linear(x.to(dtype), run.model.lin._dhd_w16, run.model.lin.bias.to(dtype))
        assert amp_weights._half_of(run.model.conv2, torch.randn(1, 4, 5, 5, device=gpu)) is not None
    assert y.dtype == dtype and torch.equal(y, want)
    with torch.no_grad():
        run.model.lin.weight.mul_(2.0)                 # anyone else's update: the copy is stale, the layer falls back
    with torch.autocast('cuda', dtype=dtype):
        assert amp_weights._half_of(run.model.lin, x) is None


@pytest.mark.gpu
@pytest.mark.parametrize('poison', [float('inf'), float('nan')], ids=['inf', 'nan'])
def test_a_non_finite_gradient_skips_the_step(gpu, poison):
    """p, m, v, the half copies and the step counts keep their bytes, the EMA advances as ModelEMA.update does after a skipped
    scaler.step, the scale is halved; after growth_interval = 2 clean steps it doubles."""
    import dhd_amd
    runs = []
    for how in ('fused', 'after'):
        scale = dhd_amd.DynamicLossScale(init_scale=1024.0, growth_interval=2)
        run = Run(gpu, ema=how, half=torch.float16, scale=scale)
        assert float(scale.scale(torch.ones((), device=gpu))) == 1024.0
        run.step(0, 1024.0)
        rec = run.opt.last_record()
        assert not rec['found_inf'] and rec['scale'] == 1024.0 and abs(rec['norm'] - math.sqrt(sum(SIZES))) < 0.05 * rec['norm']
        before = run.bytes()
        run.step(1, 1024.0, poison=poison)
        rec = run.opt.last_record()
        assert rec['found_inf'] and rec['scale'] == 512.0 and scale.get_scale() == 512.0 and scale.state_dict()['_growth_tracker'] == 0
        after = run.bytes()
        changed = _same(before, after)
        assert changed and all(k.startswith('ema.') for k in changed), changed     # nothing but the EMA moved
        assert {'ema.flat.11', 'ema.eoff', 'ema.conv2.weight', 'ema.running'} <= set(changed)
        assert {float(run.opt.state[p]['step']) for p in run.model.trainable() if p is not run.model.none} == {1.0}
        for it, want in ((2, 512.0), (3, 1024.0)):
            run.step(it, 512.0)
            assert not run.opt.last_record()['found_inf'] and scale.get_scale() == want
        runs.append(run)
    assert runs[0].ema.updates == runs[1].ema.updates == 304
    assert _same(runs[0].bytes(), runs[1].bytes()) == []


@pytest.mark.gpu
def test_a_captured_step_follows_the_learning_rate_and_equals_eager_steps(gpu):
    """One warm-up step, the capture, three replays with new gradients and another lr each time, against the same four steps
    run eagerly: every byte.  The step counts, the clip coefficient, the loss scale and the EMA's decay are read on the device;
    the lr reaches the replay through advance()."""
    import dhd_amd
    from dhd_amd.graph import GraphedStep
    lrs = [(3e-3, 1e-3), (2e-3, 5e-4), (1e-3, 2e-3), (7e-4, 1e-4)]

    def make():
        run = Run(gpu, ema='fused', half=torch.bfloat16, scale=dhd_amd.DynamicLossScale(init_scale=8.0, growth_interval=3))
        run.model.set_grads(run.model.grad_values(0, 8.0))
        return run

    def load(run, it):
        for p, v in zip(run.model.trainable(), run.model.grad_values(it, 8.0)):
            if v is not None:
                p.grad.copy_(v)
        for group, lr in zip(run.opt.param_groups, lrs[it]):
            group['lr'] = lr

    eager, graphed = make(), make()
    for it in range(4):
        load(eager, it)
        eager.opt.step()
    load(graphed, 0)
    step = GraphedStep(lambda: graphed.opt.step(), warmup=1, before_replay=[graphed.opt.advance], emas=[graphed.ema])
    assert graphed.ema.captured and graphed.opt.rebuilds == 1
    for it in range(1, 4):
        load(graphed, it)
        step()
    torch.cuda.synchronize()
    assert graphed.ema.updates == eager.ema.updates == 304 and graphed.opt.rebuilds == 1
    assert _same(eager.bytes(), graphed.bytes()) == []
    assert eager.opt.last_record() == graphed.opt.last_record() and eager.opt.last_record()['scale'] == 16.0
    assert {float(graphed.opt.state[p]['step']) for p in graphed.model.trainable() if p is not graphed.model.none} == {4.0}


@pytest.mark.gpu
def test_the_learning_rate_of_each_replay_is_its_own_with_the_host_running_ahead(gpu):
    """Static gradients on the device, eight replays issued back to back behind a queue of matrix products, another lr before
    each and no synchronisation in between: the host is replays ahead of the device when the uploads run, and every replay must
    still step with the lr advance() was given for it -- the bytes of the same eight steps run eagerly one by one."""
    import dhd_amd
    from dhd_amd.graph import GraphedStep
    lrs = [(3e-3 / (1 + it), 1e-3 * (1 + it)) for it in range(9)]

    def make():
        run = Run(gpu, ema='fused', half=torch.float16)
        run.model.set_grads(run.model.grad_values(0, 1.0))
        return run

    def set_lr(run, it):
        for group, lr in zip(run.opt.param_groups, lrs[it]):
            group['lr'] = lr

    eager, graphed = make(), make()
    for it in range(9):
        set_lr(eager, it)
        eager.opt.step()
        torch.cuda.synchronize()
    set_lr(graphed, 0)
    step = GraphedStep(lambda: graphed.opt.step(), warmup=1, before_replay=[graphed.opt.advance], emas=[graphed.ema])
    big = torch.randn(8192, 8192, device=gpu)
    torch.cuda.synchronize()
    for _ in range(12):
        big @ big                                   # tens of milliseconds of queue: the replays below wait behind it
    for it in range(1, 9):
        set_lr(graphed, it)
        step()
    torch.cuda.synchronize()
    assert _same(eager.bytes(), graphed.bytes()) == []


@pytest.mark.gpu
def test_a_whole_captured_step_with_the_gradients_kept_in_place(gpu):
    """The whole-step form: zero_grad(set_to_none=False), a backward and the step in one captured function.  The gradients stay
    where the warm-up's backward put them, so the table of the warm-up serves the capture and the replays; three replays with new
    inputs against the same steps run eagerly: every byte.  (With set_to_none=True the gradients of the capture would be new
    tensors and step() raises: the table is not rebuilt while a stream captures.)"""
    import dhd_amd
    from dhd_amd.graph import GraphedStep

    def make():
        run = Run(gpu, ema='fused', half=torch.float16, scale=dhd_amd.DynamicLossScale(init_scale=4.0, growth_interval=2))
        used = [p for p in run.model.trainable() if p is not run.model.none]
        coef = [torch.empty_like(p) for p in used]

        def step_fn():
            run.opt.zero_grad(set_to_none=False)
            loss = sum((p * c).sum() for p, c in zip(used, coef))
            run.scale.scale(loss).backward()
            run.opt.step()
            return loss

        def load(it):
            gen = torch.Generator().manual_seed(50 + it)
            for c in coef:
                c.copy_(torch.randn(c.shape, generator=gen))
        return run, step_fn, load

    eager, eager_fn, eager_load = make()
    for it in range(4):
        eager_load(it)
        eager_fn()
    graphed, fn, load = make()
    load(0)
    step = GraphedStep(fn, warmup=1, before_replay=[graphed.opt.advance], emas=[graphed.ema])
    assert graphed.opt.rebuilds == 1                               # the warm-up's; the capture found the same addresses
    for it in range(1, 4):
        load(it)
        step()
    torch.cuda.synchronize()
    assert graphed.opt.rebuilds == 1 and graphed.ema.updates == eager.ema.updates == 304
    assert _same(eager.bytes(), graphed.bytes()) == []
    assert eager.opt.last_record() == graphed.opt.last_record() and eager.opt.last_record()['scale'] == 16.0


@pytest.mark.gpu
@pytest.mark.parametrize('poison', [None, float('inf')], ids=['stepped', 'skipped'])
def test_a_stale_half_copy_is_current_after_any_step(gpu, poison):
    """A weight changed in place behind the cache's back (load_state_dict without refresh()): the copy is stale and the layer
    falls back.  After the next step -- also a skipped one, which writes half = round(p) from the unchanged p -- the copy is the
    rounded weight and the layer is routed again."""
    import dhd_amd
    from dhd_amd import amp_weights
    run = Run(gpu, half=torch.float16, scale=dhd_amd.DynamicLossScale(init_scale=2.0))
    run.step(0, 2.0)
    with torch.no_grad():
        for m in run.cache.modules:
            m.weight.add_(0.5)
    x = torch.randn(6, 33, device=gpu)
    with torch.autocast('cuda', dtype=torch.float16):
        assert amp_weights._half_of(run.model.lin, x) is None
    weights = [m.weight.detach().clone() for m in run.cache.modules]
    run.step(1, 2.0, poison=poison)
    assert run.opt.last_record()['found_inf'] == (poison is not None)
    for m, w in zip(run.cache.modules, weights):
        assert torch.equal(m.weight, w) == (poison is not None)
        assert torch.equal(m._dhd_w16, m.weight.to(torch.float16)), type(m).__name__
    with torch.autocast('cuda', dtype=torch.float16):
        assert amp_weights._half_of(run.model.lin, x) is not None and amp_weights._half_of(run.model.conv2, torch.randn(1, 4, 5, 5, device=gpu)) is not None


@pytest.mark.gpu
def test_two_identical_runs_give_identical_bytes(gpu):
    runs = [Run(gpu, ema='fused', half=torch.float16) for _ in range(2)]
    for run in runs:
        for it in range(2):
            run.step(it, 1.0)
    assert _same(runs[0].bytes(), runs[1].bytes()) == []
    assert runs[0].opt.last_record() == runs[1].opt.last_record()


def _spy(monkeypatch):
    """The entry points a run reaches through the library handle."""
    from dhd_amd import _lib
    seen, real = [], _lib.load()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def call(*a):
                seen.append(name)
                return fn(*a)
            return call
    monkeypatch.setattr(_lib, '_lib', Spy())
    return seen


@pytest.mark.gpu
def test_one_step_inside_guard_bands(gpu, monkeypatch):
    """Every buffer of the step -- parameters, gradients, moments, EMA and half copies moved into guarded memory, the tables and
    the workspace -- between guard bands, at both fill values: the guards stay intact, the three launching entry points are
    reached, and the results are the plain run's bytes (the fill is never read)."""
    import dhd_amd

    def one():
        run = Run(gpu, ema='fused', half=torch.float16, scale=dhd_amd.DynamicLossScale(init_scale=4.0))
        for v, m in run.ema.pairs(run.model):          # the EMA's parameters are deep copies torch allocated: move them under guard
            if isinstance(v, nn.Parameter):
                off = 1 if m is run.model.eoff else 0
                v.data = _new(gpu, v.detach().cpu(), offset=off, channels_last=v.dim() == 4)
        for m in run.cache.modules:
            if m is not run.model.hoff:
                m._dhd_w16 = _new(gpu, m._dhd_w16.cpu(), channels_last=m._dhd_w16.dim() == 4)
        run.step(0, 4.0)
        run.step(1, 4.0)
        torch.cuda.synchronize()
        return run
    plain = one().bytes()
    for fill in (0x00, 0xFF):
        with monkeypatch.context() as mp:
            seen = _spy(mp)
            with G.guarded(mp, fill, roots=(G.PRODUCT_ROOT, ME)) as ledger:
                run = one()
                ledger.check()
                got = run.bytes()
        inside = ledger.sites_under(G.PRODUCT_ROOT)
        print(f'fill {fill:#04x}: {len(ledger)} guarded allocations ({len(inside)} inside dhd_amd/), {ledger.total_bytes()} bytes; guards intact')
        assert inside and len(ledger) > len(inside) > 20
        assert set(ENTRIES) <= set(seen), sorted(set(ENTRIES) - set(seen))
        assert _same(plain, got) == []
