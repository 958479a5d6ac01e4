"""The tail of the training step on its own, and a whole DHD-S fp16 step with either tail.

  python experiments/optim_step_bench.py tail [--model dhd-s] [--out profiles/r24/optim_step.json]
  python experiments/optim_step_bench.py e2e  [--out profiles/r24/e2e_dhds_fp16_optim_step_ab.json]   (one process; run it twice)
  python experiments/optim_step_bench.py once --setting fp16      (one fused tail and nothing else: for a kernel trace)

tail: the parameter list of build_detector(<model cfg>) with gradients in place; today's calls in bench.py's order (unscale_,
clip_grad_norm_, fused capturable AdamW, HalfWeightCache.refresh, ModelEMA.update) against FusedAdamW.step on the SAME tensors in
the same process, for float32 / fp16 (loss scale + half cache) / bf16 (half cache), eager and captured.  Windows of `--iters`
tails alternate between the two arms; a window is timed by device events around it with a synchronise before and after; the
figure is the median over the windows with the min-max spread.  Bytes are counted from the shapes (the model of the issue: one
read of g, then g, p, m, v, ema read and p, m, v, ema and the half copies written).  Host time: perf_counter around the calls
of an eager tail with an empty queue, with the table reused and with a forced rebuild.

e2e: bench.py's EndToEnd (its model, inputs and layout) with this script's own copy of its step protocol under GraphedStep, the
torch tail against the fused tail: two models built alike, one captured step each, alternating window by window; a window in
which the arm's loss scale changed (a skipped step) is not counted.  The fused arm keeps its gradients in place
(zero_grad(set_to_none=False)), because FusedAdamW does not rebuild its table inside a capture."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dhd_amd  # noqa: E402
from dhd_amd.graph import GraphedStep  # noqa: E402

HBM = 6.3e12   # bytes/s the micro-architecture guide calls achievable


def _window(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _alternate(arms, iters, rounds):
    got = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            got[k].append(_window(fn, iters))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), windows=len(v), iters=iters) for k, v in got.items()}


def _host(fn, n):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    torch.cuda.synchronize()
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), n=n)


def build_model(name, dev):
    from dhd_amd.detector import dhd_l_model_cfg, dhd_s_model_cfg
    torch.manual_seed(0)
    model = dhd_amd.build_detector({'dhd-s': dhd_s_model_cfg, 'dhd-l': dhd_l_model_cfg}[name]()).to(dev).train()
    model.use_channels_last(True, None)
    return model


class Tails:
    """Both tails over one model.  setting: 'fp32' | 'fp16' | 'bf16'."""

    def __init__(self, model, setting, capturable):
        self.model, self.setting = model, setting
        self.params = [p for p in model.parameters() if p.requires_grad]
        gen = torch.Generator(device=self.params[0].device).manual_seed(1)
        for p in self.params:
            p.grad = torch.empty_like(p).normal_(0.0, 1e-3, generator=gen)
        self.ema = dhd_amd.ModelEMA(model, 0.9990, updates=10560)
        half = {'fp16': torch.float16, 'bf16': torch.bfloat16}.get(setting)
        self.cache = dhd_amd.HalfWeightCache(model, half) if half is not None else None
        # scale 1 on both arms: the gradients are unscaled in place by torch's arm every tail, and must not drift to zero
        self.scaler = torch.amp.GradScaler('cuda', init_scale=1.0, growth_interval=10 ** 9) if setting == 'fp16' else None
        self.scale = dhd_amd.DynamicLossScale(init_scale=1.0, growth_interval=10 ** 9) if setting == 'fp16' else None
        if self.scaler is not None:
            self.scaler.scale(torch.zeros((), device=self.params[0].device))     # GradScaler makes its state on the first scale()
        self.torch_opt = torch.optim.AdamW(self.params, lr=2e-4, weight_decay=1e-2, fused=True, capturable=capturable)
        self.fused_opt = dhd_amd.FusedAdamW(self.params, lr=2e-4, weight_decay=1e-2, max_norm=5.0, ema=self.ema, model=model,
                                            half_cache=self.cache, loss_scale=self.scale)

    def torch_tail(self):
        if self.scaler is not None:
            self.scaler._per_optimizer_states.clear()     # a tail without a backward: let unscale_ run again
            self.scaler.unscale_(self.torch_opt)
            torch.nn.utils.clip_grad_norm_(self.params, 5.0)
            self.scaler.step(self.torch_opt)
            self.scaler.update()
        else:
            torch.nn.utils.clip_grad_norm_(self.params, 5.0)
            self.torch_opt.step()
        if self.cache is not None:
            self.cache.refresh()
        self.ema.update(None, self.model)

    def fused_tail(self):
        self.fused_opt.step()

    def close(self):
        if self.cache is not None:
            self.cache.remove()       # the next Tails over the same model routes the layers again
        for p in self.params:
            p.grad = None

    def bytes(self):
        n = sum(p.numel() for p in self.params)
        n_half = sum(h.numel() for h in self.cache.halves) if self.cache is not None else 0
        n_state = sum(v.numel() for v in self.ema.ema.state_dict().values() if v.dtype.is_floating_point)
        fused = 4 * n * 10 + 2 * n_half + 12 * (n_state - n)                      # + the EMA's own sweep of what the optimizer does not own
        today = 4 * n * ((2 if self.scaler is not None else 0) + 3 + 7) + (4 + 2) * n_half + 12 * n_state
        return dict(parameters=n, tensors=len(self.params), half_copy_elements=n_half, ema_state_elements=n_state,
                    fused_model_bytes=fused, today_model_bytes=today)


def tail(args):
    dev = torch.device('cuda', 0)
    model = build_model(args.model, dev)
    out = dict(model=args.model, device=torch.cuda.get_device_name(0), hbm_bytes_per_s=HBM, protocol=__doc__.split('\n\n')[2], settings={})
    for setting in args.settings.split(','):
        rec = {}
        for mode in ('eager', 'captured'):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t = Tails(model, setting, capturable=mode == 'captured')
            rec['counts'] = t.bytes()
            for _ in range(3):
                t.torch_tail()
                t.fused_tail()
            if mode == 'eager':
                arms = {'torch': t.torch_tail, 'fused': t.fused_tail}
                rec['host_ms_fused_table_reused'] = _host(t.fused_tail, 20)

                def rebuilt():
                    t.fused_opt._table.key = None
                    t.fused_tail()
                rec['host_ms_fused_table_rebuilt'] = _host(rebuilt, 10)
                rec['host_ms_torch'] = _host(t.torch_tail, 20)
            else:
                g_torch = GraphedStep(t.torch_tail, warmup=1, emas=[t.ema])
                g_fused = GraphedStep(t.fused_tail, warmup=1, before_replay=[t.fused_opt.advance], emas=[t.ema])
                arms = {'torch': g_torch, 'fused': g_fused}
            res = _alternate(arms, args.iters, args.rounds)
            for k, r in res.items():
                b = rec['counts']['fused_model_bytes' if k == 'fused' else 'today_model_bytes']
                r['model_bytes'] = b
                r['bytes_per_s'] = b / (r['median_ms'] * 1e-3)
                r['fraction_of_hbm'] = r['bytes_per_s'] / HBM
            res['speedup_fused_over_torch'] = res['torch']['median_ms'] / res['fused']['median_ms']
            res['floor_ms_at_hbm'] = rec['counts']['fused_model_bytes'] / HBM * 1e3
            res['peak_allocated_bytes_over_model'] = torch.cuda.max_memory_allocated() - base
            rec[mode] = res
            print(setting, mode, json.dumps(res), flush=True)
            t.close()
            del t, arms
            if mode == 'captured':
                del g_torch, g_fused
        out['settings'][setting] = rec
        print(setting, 'counts', json.dumps(rec['counts']), flush=True)
    _write(args.out, out)


def once(args):
    dev = torch.device('cuda', 0)
    t = Tails(build_model(args.model, dev), args.setting, capturable=False)
    for _ in range(5):
        t.fused_tail()
    torch.cuda.synchronize()
    print('once', args.setting, json.dumps(t.fused_opt.last_record()))


def e2e(args):
    """bench.py's model, inputs and layout; this script's copy of its step protocol (bench.py: EndToEnd._eager_step)."""
    import bench
    dev = torch.device('cuda', 0)
    # one model per arm, built alike: each arm is then the benchmark's own training run, and its loss scale settles as there
    e = bench.EndToEnd(dev, args.batch, 0, 1, 'fp16', model='dhd-s', ema=True, graph=True)
    f = bench.EndToEnd(dev, args.batch, 0, 1, 'fp16', model='dhd-s', ema=True, graph=True)
    # the synthetic batch does not train stably at the configs' lr under fp16: both arms start at the scale they settle at and
    # step with a tenth of the lr, so that neither skips steps while it is timed (the hyper-parameters do not change the work)
    torch_opt = e.opt
    for group in torch_opt.param_groups:
        group['lr'] = args.lr if not torch.is_tensor(group['lr']) else group['lr'].fill_(args.lr)
    scaler = torch.amp.GradScaler('cuda', init_scale=args.init_scale)
    scale = dhd_amd.DynamicLossScale(init_scale=args.init_scale)
    fused_opt = dhd_amd.FusedAdamW(f.params, lr=args.lr, weight_decay=1e-2, max_norm=5.0, ema=f.ema, model=f.model, half_cache=f.wcache,
                                   loss_scale=scale)
    params = e.params + f.params

    def forward(b):
        with torch.autocast('cuda', dtype=torch.float16):
            return sum(b.model(return_loss=True, **b.kw).values())

    def torch_step():
        torch_opt.zero_grad(set_to_none=True)
        loss = forward(e)
        scaler.scale(loss).backward()
        scaler.unscale_(torch_opt)
        torch.nn.utils.clip_grad_norm_(e.params, 5.0)
        scaler.step(torch_opt)
        scaler.update()
        e.wcache.refresh()
        e.ema.update(None, e.model)
        return loss

    def fused_step():
        # the gradients stay in place (FusedAdamW does not rebuild its table inside a capture): a zeroing pass and accumulating
        # instead of adopting the first gradient, which the torch arm does not pay
        fused_opt.zero_grad(set_to_none=False)
        loss = forward(f)
        scale.scale(loss).backward()
        fused_opt.step()
        return loss

    arms = {'torch_tail': GraphedStep(torch_step, warmup=3, emas=[e.ema]),
            'fused_tail': GraphedStep(fused_step, warmup=3, before_replay=[fused_opt.advance], emas=[f.ema])}
    res_settle = []
    for _ in range(args.settle):          # both loss scales start at 65536 and settle over the first replays; synchronises
        losses = {k: float(fn().detach()) for k, fn in arms.items()}
        res_settle.append(dict(losses, torch_scale=scaler.get_scale(), fused=fused_opt.last_record()))
    # a window counts only if no step in it was skipped by either arm (a skipped step is cheaper in the fused sweep: it moves the
    # EMA alone): both scales are read before and after, and with growth_interval = 2000 a change is a skipped step
    windows = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            before = (scaler.get_scale(), scale.get_scale())
            ms = _window(fn, args.iters)
            windows[k].append(dict(ms=ms, clean=before == (scaler.get_scale(), scale.get_scale())))
    res = {}
    for k, w in windows.items():
        clean = [x['ms'] for x in w if x['clean']]
        res[k] = dict(median_ms=statistics.median(clean) if clean else None, min_ms=min(clean, default=None), max_ms=max(clean, default=None),
                      clean_windows=len(clean), windows=len(w), iters=args.iters, all_ms=[round(x['ms'], 3) for x in w])
    if res['torch_tail']['median_ms'] and res['fused_tail']['median_ms']:
        res['speedup_fused_over_torch'] = res['torch_tail']['median_ms'] / res['fused_tail']['median_ms']
    res['settling'] = res_settle
    res['table'] = dict(chunks=fused_opt._table.n_chunks, torch_path_tensors=len(fused_opt._table.fallback))
    res['fused_record'] = fused_opt.last_record()
    res['torch_scale'] = scaler.get_scale()
    res['parameters_finite'] = all(bool(torch.isfinite(p).all()) for p in params)
    res['rebuilds'] = fused_opt.rebuilds
    out = dict(model='dhd-s', amp='fp16', batch=args.batch, lr=args.lr, init_scale=args.init_scale, device=torch.cuda.get_device_name(0), result=res)
    print('e2e', json.dumps(res), flush=True)
    prev = json.load(open(args.out)) if os.path.exists(args.out) else dict(processes=[])
    prev['processes'].append(out)
    _write(args.out, prev)


def _write(path, obj):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(obj, f, indent=1)
        f.write('\n')
    print('wrote', path)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['tail', 'e2e', 'once'])
    ap.add_argument('--model', default='dhd-s')
    ap.add_argument('--settings', default='fp32,fp16,bf16')
    ap.add_argument('--setting', default='fp16')
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--out', default=None)
    ap.add_argument('--settle', type=int, default=24)
    ap.add_argument('--lr', type=float, default=2e-5)
    ap.add_argument('--init-scale', type=float, default=1024.0)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'r24', 'optim_step.json' if a.what == 'tail' else 'e2e_dhds_fp16_optim_step_ab.json')
    {'tail': tail, 'e2e': e2e, 'once': once}[a.what](a)
