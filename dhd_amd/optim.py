"""The tail of the training step as one operator: unscale, clip, AdamW, the weight EMA and the half weight copies.

Between `loss.backward()` and the next forward the step protocol of the reference configs runs `GradScaler.unscale_`,
`clip_grad_norm_(..., 5)` (optimizer_config.grad_clip), `AdamW.step`, `HalfWeightCache.refresh()` and `ModelEMA.update`: five
sweeps over the parameter set, up to 16.5 passes over its 147 M values for DHD-S.  `FusedAdamW.step()` is three launches of
csrc/optim_step.h (dhd_amd/capi_optim/dhd_amd_optim.h) over one chunk table: the gradients are read once for the global norm, a
one-workgroup launch turns the partial sums into the clip coefficient, the step counts and the loss-scale rule, and one sweep
reads g, p, m, v, ema and writes p, m, v, ema and the half copies.  Everything that changes from step to step lives in device
memory, so the step can be captured into a HIP graph (`GraphedStep(before_replay=[opt.advance], emas=[ema])`) after one eager
step, as long as gradients, state and copies stay where that step found them (the table is not rebuilt while a stream captures:
a whole captured step keeps its gradients in place with `zero_grad(set_to_none=False)`); nothing synchronises but `grad_norm()` / `last_record()` / `state_dict()`.

The arithmetic is torch's single-tensor AdamW in float32, one rounding per operation, on g' = g * (inv_scale * coef): within the
bar of torch's own float32 path against float64 (tests/test_gpu_optim_step.py), not bit-identical to it.  The EMA is
`ModelEMA.update`'s two roundings and the half copies are `p.to(dtype)`: both bit-identical.  A step with a non-finite gradient
is skipped whole (p, m, v and the step counts keep their bytes; the half copies are written again from the unchanged p, so they
are current afterwards whatever they were before) while the EMA still advances, as `scaler.step` followed
by `ModelEMA.update` does today -- also without a loss scale, where torch would write NaN into the parameters.

CPU tensors, and GPU tensors that are not dense in one layout with their gradient, state and copies, take the same mathematics
through torch ops (`_update_tensors`), so the class works without a GPU; a GPU tensor that the table covers never does."""
import ctypes as C

import numpy as np
import torch

from . import _lib, _optim

CHUNK = _optim.CHUNK


class DynamicLossScale:
    """GradScaler's dynamic loss scale with its state where `FusedAdamW` reads and updates it: `scale(loss)` multiplies by a
    device scalar, the optimizer's sweep divides it out of the gradients, and its one-workgroup launch applies
    `torch._amp_update_scale_`'s rule (found_inf: scale * backoff_factor; growth_interval clean steps in a row: scale *
    growth_factor).  There is no unscale_/step/update protocol: pass the object as `FusedAdamW(loss_scale=...)`.  The state is
    placed on the device of the first loss (or `device=`); `state_dict()` has GradScaler's keys and synchronises."""

    def __init__(self, init_scale=65536., growth_factor=2., backoff_factor=.5, growth_interval=2000, device=None):
        if growth_factor <= 1.0 or not 0.0 < backoff_factor < 1.0 or growth_interval < 1:
            raise ValueError('DynamicLossScale: growth_factor > 1, 0 < backoff_factor < 1 and growth_interval >= 1')
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._init = (float(init_scale), 0)
        self._scale = self._growth_tracker = None
        if device is not None:
            self.to(device)

    def to(self, device):
        """Place (or move) the state on `device`."""
        scale, tracker = self._init if self._scale is None else (self._scale.item(), self._growth_tracker.item())
        self._scale = torch.zeros((), dtype=torch.float32, device=device).fill_(scale)
        self._growth_tracker = torch.zeros((), dtype=torch.int32, device=device).fill_(tracker)
        return self

    def scale(self, loss):
        if self._scale is None:
            self.to(loss.device)
        return loss * self._scale

    def get_scale(self):
        return self._init[0] if self._scale is None else float(self._scale.item())

    def state_dict(self):
        return {'scale': self.get_scale(), 'growth_factor': self.growth_factor, 'backoff_factor': self.backoff_factor,
                'growth_interval': self.growth_interval,
                '_growth_tracker': self._init[1] if self._scale is None else int(self._growth_tracker.item())}

    def load_state_dict(self, state):
        self.growth_factor, self.backoff_factor = float(state['growth_factor']), float(state['backoff_factor'])
        self.growth_interval = int(state['growth_interval'])
        self._init = (float(state['scale']), int(state['_growth_tracker']))
        if self._scale is not None:
            self._scale.fill_(self._init[0])
            self._growth_tracker.fill_(self._init[1])

    def _host_update(self, found_inf):
        """torch._amp_update_scale_ on CPU state, in float32."""
        scale, tracker = np.float32(self._scale.item()), int(self._growth_tracker.item())
        if found_inf:
            scale, tracker = scale * np.float32(self.backoff_factor), 0
        else:
            tracker += 1
            if tracker == self.growth_interval:
                with np.errstate(over='ignore'):
                    grown = scale * np.float32(self.growth_factor)
                scale, tracker = (grown if np.isfinite(grown) else scale), 0
        self._scale.fill_(float(scale))
        self._growth_tracker.fill_(tracker)


def _dense_layout(t):
    """`t` fills its memory without gaps in one of the two layouts the parameters of the models here have."""
    return t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))


def _same_order(t, p):
    """`t` lies in memory in the order `p` does: equal strides in every dimension longer than 1 (the stride of a dimension of
    size 1 addresses nothing: an (O, I, 1, 1) weight and its gradient may disagree there and still be the same bytes in order)."""
    return t.shape == p.shape and all(a == b for n, a, b in zip(p.shape, t.stride(), p.stride()) if n != 1)


def _update_tensors(p, g, m, v, e, h, mult, decay, step_size, bc2_sqrt, omb1, b2, omb2, eps, d, omd, found):
    """The sweep's mathematics on one tensor through torch ops, operation for operation (csrc/optim_step.h: adamw1, ema1).  The
    scalars are Python floats and `found` a bool (CPU), or 0-dim device tensors (a GPU tensor outside the chunk table)."""
    g = g * mult
    p_new = p * decay
    m_new = m + (g - m) * omb1
    v_new = v * b2 + omb2 * g * g
    p_new = p_new - step_size * (m_new / (v_new.sqrt() / bc2_sqrt + eps))
    if torch.is_tensor(found):
        p_new, m_new, v_new = torch.where(found, p, p_new), torch.where(found, m, m_new), torch.where(found, v, v_new)
        found = False
    if not found:
        p.copy_(p_new)
        m.copy_(m_new)
        v.copy_(v_new)
    if h is not None:      # also on a skipped step: the copy is then current whatever it was before
        h.copy_(p)
    if e is not None:      # ModelEMA.update's expression
        e *= d
        e += omd * p


class _Table:
    """What one set of addresses needs on the device: the chunk rows, the slot -> group map and the argument struct."""

    def __init__(self):
        self.key = None
        self.n_chunks = self.n_partials = 0
        self.chunk_rows = None      # numpy, kept for the tests and the pinned upload
        self.fallback = []
        self.kernel_params = []


class FusedAdamW(torch.optim.Optimizer):
    """`torch.optim.AdamW` (decoupled weight decay) with gradient unscaling, global-norm clipping (`max_norm`, the L2 norm over
    all parameters of all groups, as `clip_grad_norm_`), the weight EMA (`ema=`: a ModelEMA, with `model=` the model it
    follows) and the half weight copies (`half_cache=`: a HalfWeightCache) in the same sweep.  `loss_scale=`: a DynamicLossScale.

    Param groups are supported; `amsgrad`, `maximize` and a `norm_type` other than 2 raise ValueError; parameters whose `grad`
    is None are skipped.  `state_dict()` / `load_state_dict()` have torch.optim.AdamW's layout (`step`, `exp_avg`, `exp_avg_sq`
    per parameter and its param-group keys), so state moves between the two classes in either direction.  With `ema=` do not call
    `ModelEMA.update` as well: `step()` runs the whole update (the tensors the optimizer does not own through
    `ModelEMA.update_rest`).  With `half_cache=` do not call `refresh()`.  All parameters that have a gradient must live on
    one device."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None, ema=None, half_cache=None,
                 loss_scale=None, *, model=None, norm_type=2, amsgrad=False, maximize=False):
        if amsgrad or maximize:
            raise ValueError('FusedAdamW: amsgrad and maximize are not supported')
        if float(norm_type) != 2.0:
            raise ValueError('FusedAdamW: gradient clipping by the L2 norm only (norm_type=2)')
        if max_norm is not None and not float(max_norm) >= 0.0:
            raise ValueError('FusedAdamW: max_norm must be None or >= 0')
        if ema is not None and model is None:
            raise ValueError('FusedAdamW: ema= needs model=, the model the ModelEMA follows')
        # torch.optim.AdamW's own defaults and checks (lr, eps, betas, weight_decay ranges), so that the param groups carry every
        # key its step() reads after a load_state_dict of ours
        defaults = dict(torch.optim.AdamW([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay).defaults)
        defaults.update(foreach=None, fused=None, capturable=False)
        super().__init__(params, defaults)
        self.max_norm = None if max_norm is None else float(max_norm)
        self.ema, self.model, self.half_cache, self.loss_scale = ema, model, half_cache, loss_scale
        self.rebuilds = 0                     # how often the device table was (re)built
        self._table = _Table()
        self._dev = None                      # device-resident state: see _device_state()
        self._hyper = None                    # the hyper-parameters last uploaded
        self._record = None                   # the step record of the CPU path

    # ------------------------------------------------------------------------------------------------ hyper-parameters

    def _check_groups(self):
        for group in self.param_groups:
            if group.get('amsgrad') or group.get('maximize'):
                raise ValueError('FusedAdamW: amsgrad and maximize are not supported')
            if torch.is_tensor(group['lr']):
                raise ValueError('FusedAdamW: lr must be a float (the table on the device is what a captured step reads)')

    def _hyper_rows(self):
        return [(float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay']))
                for g in self.param_groups]

    def advance(self):
        """Upload the hyper-parameter table if a scheduler (or anyone) changed a group's lr, betas, eps or weight_decay since the
        last upload.  `step()` calls it; around a captured step it must run before every replay:
        `GraphedStep(before_replay=[opt.advance], emas=[ema])`."""
        rows = self._hyper_rows()
        if self._dev is None or rows == self._hyper or torch.cuda.is_current_stream_capturing():
            return      # (while a graph is captured nothing is uploaded: the replays' advance() does it)
        self._check_groups()
        # a pageable source, as ModelEMA._set_decay_dev: the runtime stages it when the copy is issued, so a later advance() --
        # the host runs replays ahead of the device -- cannot change what an earlier upload delivers
        image = torch.from_numpy(np.array(rows, dtype=np.float64).reshape(-1).view(np.uint8))
        self._dev['groups'].copy_(image, non_blocking=True)
        self._hyper = rows

    # ------------------------------------------------------------------------------------------------ state

    def _slots(self):
        """(group index, slot, parameter) of every parameter: a slot is the parameter's position over all groups."""
        out = []
        for gi, group in enumerate(self.param_groups):
            for p in group['params']:
                out.append((gi, len(out), p))
        return out

    def _device_state(self, device, n_slots):
        """Device memory that outlives a table: the step counts (state['step'] of a GPU parameter is a view of one element), the
        scalars derived from them, the hyper-parameter table, and the workspace."""
        dv = self._dev
        n_groups = len(self.param_groups)
        if dv is not None and dv['device'] == device and dv['n_slots'] == n_slots and dv['n_groups'] == n_groups:
            return dv
        if dv is not None and dv['device'] != device:
            raise ValueError(f'FusedAdamW: parameters on {dv["device"]} and on {device}; one device only')
        new = dict(device=device, n_slots=n_slots, n_groups=n_groups,
                   steps=torch.zeros(n_slots, dtype=torch.float32, device=device),
                   slot_scalars=torch.zeros((n_slots, 4), dtype=torch.float32, device=device),
                   group_scalars=torch.zeros((n_groups, 4), dtype=torch.float32, device=device),
                   groups=torch.zeros(n_groups * _optim.GROUP_DTYPE.itemsize, dtype=torch.uint8, device=device),
                   decay_pair=torch.zeros(2, dtype=torch.float32, device=device), workspace=None)
        if dv is not None:      # a param group was added: the counts move over
            n = min(n_slots, dv['n_slots'])
            new['steps'][:n].copy_(dv['steps'][:n])
        for _, slot, p in self._slots():
            st = self.state.get(p)
            if st and p.is_cuda:
                if dv is None:
                    new['steps'][slot].copy_(st['step'])
                st['step'] = new['steps'][slot]
        self._dev, self._hyper, self._table.key = new, None, None
        return new

    def _init_state(self, p, slot):
        st = self.state[p]
        if not st:
            st['step'] = self._dev['steps'][slot] if p.is_cuda else torch.zeros((), dtype=torch.float32)
            st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def state_dict(self):
        """torch.optim.AdamW's layout; `step` comes out as a float32 scalar on the CPU, as torch keeps it (synchronises)."""
        sd = super().state_dict()
        sd['state'] = {k: {n: (t.detach().to('cpu', copy=True) if n == 'step' else t) for n, t in st.items()} for k, st in sd['state'].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._check_groups()
        slots = self._slots()
        gpu = [p for _, _, p in slots if p.is_cuda]
        if gpu:
            self._dev = None
            self._device_state(gpu[0].device, len(slots))          # the loaded counts move into the device array
        for _, slot, p in slots:
            st = self.state.get(p)
            if not st:
                continue
            if not p.is_cuda:
                st['step'] = torch.as_tensor(st['step'], dtype=torch.float32).reshape(()).clone()
            for n in ('exp_avg', 'exp_avg_sq'):
                if st[n].stride() != p.stride() or st[n].dtype != p.dtype:      # the sweep walks p's layout
                    st[n] = torch.empty_like(p, memory_format=torch.preserve_format).copy_(st[n])
        self._table.key = None

    # ------------------------------------------------------------------------------------------------ the step

    def _copies(self):
        """id(parameter) -> its EMA tensor, and -> (module, half copy) of the cache."""
        emas = {id(m): v for v, m in self.ema.pairs(self.model)} if self.ema is not None else {}
        halves = {id(m.weight): (m, m._dhd_w16) for m in self.half_cache.modules} if self.half_cache is not None else {}
        return emas, halves

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        slots = self._slots()
        active = [(gi, slot, p) for gi, slot, p in slots if p.grad is not None]
        if any(p.grad.is_sparse for _, _, p in active):
            raise RuntimeError('FusedAdamW does not support sparse gradients')
        devices = {p.device for _, _, p in active}
        if len(devices) > 1:
            raise ValueError(f'FusedAdamW: parameters with a gradient on {sorted(map(str, devices))}; one device only')
        if devices and next(iter(devices)).type == 'cuda':
            self._step_gpu(slots, active, next(iter(devices)))
        else:
            self._step_cpu(active)
        return loss

    # ---- CPU: host logic with the kernels' mathematics (the CPU tests hold the semantics)

    def _step_cpu(self, active):
        self._check_groups()
        ls = self.loss_scale
        if ls is not None and ls._scale is None:
            ls.to('cpu')
        inv = np.float32(1.0 / float(ls._scale.item())) if ls is not None else np.float32(1.0)
        total = 0.0
        for _, _, p in active:
            total += float((p.grad * float(inv)).double().pow(2).sum())
        norm = np.float32(np.sqrt(total))
        found = not bool(np.isfinite(norm))
        coef = np.float32(1.0)
        if self.max_norm is not None:
            coef = np.float32(min(1.0, self.max_norm / (float(norm) + 1e-6))) if not found else np.float32(np.nan)
        mult = float(inv * coef)
        if ls is not None:
            ls._host_update(found)
        d = self.ema.begin_update() if self.ema is not None else 0.0
        emas, halves = self._copies()
        for gi, slot, p in active:
            group = self.param_groups[gi]
            st = self._init_state(p, slot)
            lr, (b1, b2), eps, wd = float(group['lr']), group['betas'], float(group['eps']), float(group['weight_decay'])
            if not found:
                st['step'] += 1
            step = float(st['step'])
            bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
            _update_tensors(p, p.grad, st['exp_avg'], st['exp_avg_sq'], emas.get(id(p)), halves.get(id(p), (None, None))[1], mult,
                            1.0 - lr * wd, lr / bc1 if not found else 0.0, bc2 ** 0.5 if not found else 1.0, 1.0 - b1, b2, 1.0 - b2, eps,
                            d, 1.0 - d, found)
        if self.ema is not None:
            self.ema.update_rest(self.model, {id(p) for _, _, p in active if id(p) in emas}, d)
        self._stamp(p for _, _, p in active)
        self._record = dict(norm=float(norm), coef=float(coef), found_inf=found, scale=ls.get_scale() if ls is not None else 1.0)

    # ---- GPU

    def plan(self, active, emas, halves):
        """Sort the parameters that have a gradient into the chunk table (everything dense in the parameter's own layout) and the
        fallback set (torch ops); returns (table entries, fallback entries) of (group, slot, p, g, m, v, ema, (module, half))."""
        table, fallback = [], []
        for gi, slot, p in active:
            st = self._init_state(p, slot)
            g, m, v, e, mh = p.grad, st['exp_avg'], st['exp_avg_sq'], emas.get(id(p)), halves.get(id(p))
            h = mh[1] if mh is not None else None
            if any(t.dtype != torch.float32 for t in (p, g, m, v)) or (e is not None and e.dtype != torch.float32):
                raise _lib.DhdError('FusedAdamW: GPU parameters, gradients, state and EMA copies must be float32')
            if any(t is not None and (t.device != p.device or t.shape != p.shape) for t in (g, m, v, e, h)):
                raise _lib.DhdError('FusedAdamW: a gradient, state tensor or copy differs from its parameter in device or shape')
            same = _dense_layout(p) and all(t is None or _same_order(t, p) for t in (g, m, v, e, h))
            (table if same or p.numel() == 0 else fallback).append((gi, slot, p, g, m, v, e, mh))
        return table, fallback

    @staticmethod
    def chunk_rows(entries):
        """The rows of dhdw_optim_chunk for `entries`, vectorised: a numpy array of _optim.CHUNK_DTYPE."""
        n = len(entries)
        numel = np.fromiter((e[2].numel() for e in entries), dtype=np.int64, count=n)
        ptrs = np.array([[e[2].data_ptr(), e[3].data_ptr(), e[4].data_ptr(), e[5].data_ptr(), 0 if e[6] is None else e[6].data_ptr(),
                          0 if e[7] is None else e[7][1].data_ptr()] for e in entries], dtype=np.uint64).reshape(n, 6)
        n_ch = (numel + CHUNK - 1) // CHUNK
        owner = np.repeat(np.arange(n), n_ch)
        k = np.arange(int(n_ch.sum()), dtype=np.int64) - np.repeat(np.cumsum(n_ch) - n_ch, n_ch)    # chunk number inside its tensor
        rows = np.zeros(len(owner), dtype=_optim.CHUNK_DTYPE)
        off = (k * CHUNK).astype(np.uint64)
        for j, name in enumerate(('p', 'g', 'exp_avg', 'exp_avg_sq', 'ema', 'half')):
            base = ptrs[owner, j]
            rows[name] = np.where(base != 0, base + off * np.uint64(2 if name == 'half' else 4), np.uint64(0))
        rows['len'] = np.minimum(CHUNK, numel[owner] - k * CHUNK)
        rows['group'] = np.fromiter((e[0] for e in entries), dtype=np.int32, count=n)[owner]
        rows['slot'] = np.fromiter((e[1] for e in entries), dtype=np.int32, count=n)[owner]
        rows['half_dtype'] = np.fromiter((0 if e[7] is None else _lib.dtype_code(e[7][1].dtype) for e in entries), dtype=np.int32, count=n)[owner]
        return rows

    def _key(self, active, emas, halves):
        key = []
        for _, _, p in active:
            st, g, e, mh = self.state.get(p) or {}, p.grad, emas.get(id(p)), halves.get(id(p))
            key.append((p.data_ptr(), g.data_ptr(), p.stride(), g.stride(),
                        st['exp_avg'].data_ptr() if st else 0, st['exp_avg_sq'].data_ptr() if st else 0,
                        e.data_ptr() if e is not None else 0, mh[1].data_ptr() if mh is not None else 0))
        return key

    def _rebuild(self, slots, active, emas, halves, device, key):
        if torch.cuda.is_current_stream_capturing():
            # e.g. zero_grad(set_to_none=True) and a backward inside the captured function: the gradients of the capture are new
            # tensors.  The table is not rebuilt while a stream captures (its upload would be a copy node bound to a host image)
            raise _lib.DhdError('FusedAdamW: the addresses of the gradients, state or copies changed while a graph is being captured; '
                                'keep the gradients in place (zero_grad(set_to_none=False)) and run one eager step before the capture')
        dv = self._device_state(device, len(slots))
        entries, fallback = self.plan(active, emas, halves)
        rows = self.chunk_rows(entries)
        t = self._table = _Table()
        t.key, t.chunk_rows, t.fallback = key, rows, fallback
        t.kernel_params = [e[2] for e in entries]
        t.n_chunks, t.n_partials = len(rows), len(rows) + len(fallback)
        slot_group = np.full(len(slots), -1, dtype=np.int32)
        for gi, slot, _ in active:
            slot_group[slot] = gi
        # one host image -> one device buffer: [chunk rows | slot_group], through a fresh pinned tensor per upload (the caching
        # host allocator keeps it from being reused before the copy has run)
        image = np.concatenate([rows.view(np.uint8).reshape(-1), slot_group.view(np.uint8)])
        size = max(image.size, 16)
        t.host = torch.empty(size, dtype=torch.uint8).pin_memory()
        t.host.numpy()[:image.size] = image
        t.dev = torch.empty(size, dtype=torch.uint8, device=device)
        t.dev.copy_(t.host, non_blocking=True)
        ws_bytes = _optim.value('dhdw_optim_workspace_bytes', t.n_partials)
        if dv['workspace'] is None or dv['workspace'].numel() < ws_bytes:
            dv['workspace'] = torch.zeros(ws_bytes, dtype=torch.uint8, device=device)
        ws = dv['workspace']
        t.ws_bytes = ws_bytes
        t.record = ws[_optim.RECORD_AT:_optim.RECORD_AT + 16].view(torch.float32)
        t.mult = ws[_optim.MULT_AT:_optim.MULT_AT + 4].view(torch.float32)[0]
        t.found = ws[_optim.FOUND_AT:_optim.FOUND_AT + 4].view(torch.int32)[0]
        t.partials = ws[_optim.PARTIALS_AT:_optim.PARTIALS_AT + 8 * t.n_partials].view(torch.float64)
        t.flags = ws[_optim.PARTIALS_AT + 8 * t.n_partials:_optim.PARTIALS_AT + 12 * t.n_partials].view(torch.int32)
        ls = self.loss_scale
        t.args = _optim.Tables(chunks=t.dev.data_ptr(), groups=dv['groups'].data_ptr(), slot_group=t.dev.data_ptr() + rows.nbytes,
                               steps=dv['steps'].data_ptr(), slot_scalars=dv['slot_scalars'].data_ptr(),
                               group_scalars=dv['group_scalars'].data_ptr(),
                               decay_pair=(self.ema._decay_dev[device] if self.ema is not None else dv['decay_pair']).data_ptr(),
                               scale=ls._scale.data_ptr() if ls is not None else None,
                               growth_tracker=ls._growth_tracker.data_ptr() if ls is not None else None,
                               n_chunks=t.n_chunks, n_groups=len(self.param_groups), n_slots=len(slots), n_partials=t.n_partials)
        self.rebuilds += 1
        return t

    def _step_gpu(self, slots, active, device):
        ls = self.loss_scale
        if ls is not None:
            if ls._scale is None:
                ls.to(device)
            if ls._scale.device != device:
                raise ValueError(f'FusedAdamW: the loss scale lives on {ls._scale.device}, the parameters on {device}')
        with torch.cuda.device(device):
            d = self.ema.begin_update([device]) if self.ema is not None else 0.0
            emas, halves = self._copies()
            self._device_state(device, len(slots))
            for _, slot, p in active:
                self._init_state(p, slot)
            key = self._key(active, emas, halves)
            t = self._table
            if key != t.key:
                t = self._rebuild(slots, active, emas, halves, device, key)
            dv = self._dev
            self.advance()
            stream = _lib.stream_ptr(device)
            args, ws = C.byref(t.args), _lib.ptr(dv['workspace'])
            inv = (1.0 / ls._scale.double()).float() if ls is not None and t.fallback else None
            for j, e in enumerate(t.fallback):     # the partial sums of the tensors outside the table, where the finalize launch reads them
                g = e[3] if inv is None else e[3] * inv
                total = g.double().pow(2).sum()
                t.partials[t.n_chunks + j].copy_(total)
                t.flags[t.n_chunks + j].copy_(~torch.isfinite(total))
            _optim.call('dhdw_optim_grad_norm', args, ws, t.ws_bytes, stream)
            _optim.call('dhdw_optim_finalize', args, -1.0 if self.max_norm is None else self.max_norm,
                        ls.growth_factor if ls is not None else 1.0, ls.backoff_factor if ls is not None else 1.0,
                        ls.growth_interval if ls is not None else 0, ws, t.ws_bytes, stream)
            _optim.call('dhdw_optim_adamw_update', args, ws, t.ws_bytes, stream)
            if t.fallback:
                pair = self.ema._decay_dev[device] if self.ema is not None else dv['decay_pair']
                found = t.found != 0
                for gi, slot, p, g, m, v, e, mh in t.fallback:
                    ss, gs = dv['slot_scalars'][slot], dv['group_scalars'][gi]
                    _update_tensors(p, g, m, v, e, None if mh is None else mh[1], t.mult, ss[0], ss[1], ss[2], gs[0], gs[1], gs[2], gs[3],
                                    pair[0], pair[1], found)
            if self.ema is not None:
                self.ema.update_rest(self.model, {id(p) for _, _, p in active if id(p) in emas}, d)
            if t.kernel_params:
                torch.autograd.graph.increment_version(t.kernel_params)     # the launch wrote them behind autograd's back
            self._stamp(p for _, _, p in active)

    def _stamp(self, params):
        """The half copies of the updated weights are current: `_half_of` compares this key."""
        if self.half_cache is None:
            return
        updated = {id(p) for p in params}
        for m in self.half_cache.modules:
            w = m.weight
            if id(w) in updated:
                m._dhd_w16_key = (w.data_ptr(), w._version)

    # ------------------------------------------------------------------------------------------------ the record

    def last_record(self):
        """{norm, coef, found_inf, scale} of the last step: the gradients' global L2 norm after unscaling, the clip coefficient,
        whether the step was skipped, the loss scale after the rule.  Reads device memory: synchronises."""
        if self._table.key is not None:
            norm, coef, found, scale = self._table.record.tolist()
            return dict(norm=norm, coef=coef, found_inf=bool(found), scale=scale)
        return self._record

    def grad_norm(self):
        """The global gradient norm of the last step, what `clip_grad_norm_` returns (synchronises)."""
        rec = self.last_record()
        return None if rec is None else rec['norm']


def build_optimizer(model, optimizer_cfg, optimizer_config=None, fused=False, **kw):
    """The optimizer of the reference's config dicts, unchanged: `optimizer = dict(type='AdamW', lr=2e-4, weight_decay=1e-2)` and
    `optimizer_config = dict(grad_clip=dict(max_norm=5, norm_type=2))`.  fused=False: `torch.optim.AdamW` over the parameters
    that require a gradient (clipping stays the caller's, as it is today).  fused=True: `FusedAdamW` with the grad_clip of
    `optimizer_config` as its `max_norm`; **kw goes to the constructor (ema=, half_cache=, loss_scale=)."""
    cfg = dict(optimizer_cfg)
    if cfg.pop('type') != 'AdamW':
        raise ValueError(f"build_optimizer: type='AdamW' only, got {optimizer_cfg['type']!r}")
    if cfg.pop('paramwise_cfg', None):
        raise ValueError('build_optimizer: paramwise_cfg is not supported')
    params = [p for p in model.parameters() if p.requires_grad]
    if not fused:
        return torch.optim.AdamW(params, **cfg, **kw)
    clip = dict((optimizer_config or {}).get('grad_clip') or {})
    if clip:
        kw.setdefault('max_norm', clip.pop('max_norm'))
        kw.setdefault('norm_type', clip.pop('norm_type', 2))
        if clip:
            raise ValueError(f'build_optimizer: grad_clip keys {sorted(clip)} are not supported')
    if kw.get('ema') is not None:
        kw.setdefault('model', model)
    return FusedAdamW(params, **cfg, **kw)
