"""Shared by tests/test_optim_host.py and tests/test_gpu_optim_step.py (a helper module, not a conftest): the float64 twin of the
optimizer step and the bar the fused step is held to.

The twin is torch's single-tensor AdamW (torch/optim/adam.py, `_single_tensor_adam` with decoupled weight decay) behind
`clip_grad_norm_`'s expressions, written out in float64.  For each of p, exp_avg, exp_avg_sq (over all tensors together) and the
norm, E = max|x - x64| / max|x64|; the bar is E_fused <= 1.5 * E_torch + 2^-23 with E_torch measured on the same inputs through
torch's own float32 path: the project's 1.5x rule for operators that are not bit-identical, plus one rounding of the stored
result."""
import math

import torch

QUANTITIES = ('p', 'exp_avg', 'exp_avg_sq')


class Twin64:
    """params: float32 tensors (their values are the start); group_of[i]: index into hypers; hypers: dicts with lr, betas, eps,
    weight_decay; max_norm: None or the clip threshold."""

    def __init__(self, params, group_of, hypers, max_norm):
        self.p = [p.detach().double().cpu().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.steps = [0] * len(self.p)
        self.group_of, self.hypers, self.max_norm = list(group_of), hypers, max_norm
        self.norm = None

    def step(self, grads, inv_scale=1.0):
        """grads: per parameter a tensor or None (skipped, as torch skips it)."""
        gs = [None if g is None else g.detach().double().cpu() * inv_scale for g in grads]
        self.norm = math.sqrt(sum(float((g * g).sum()) for g in gs if g is not None))
        coef = 1.0 if self.max_norm is None else min(1.0, self.max_norm / (self.norm + 1e-6))
        for i, g in enumerate(gs):
            if g is None:
                continue
            h = self.hypers[self.group_of[i]]
            lr, (b1, b2), eps, wd = h['lr'], h['betas'], h['eps'], h['weight_decay']
            g = g * coef
            self.steps[i] += 1
            t = self.steps[i]
            self.p[i] = self.p[i] * (1.0 - lr * wd)
            self.m[i] = self.m[i] + (g - self.m[i]) * (1.0 - b1)
            self.v[i] = self.v[i] * b2 + (1.0 - b2) * g * g
            denom = self.v[i].sqrt() / math.sqrt(1.0 - b2 ** t) + eps
            self.p[i] = self.p[i] - (lr / (1.0 - b1 ** t)) * (self.m[i] / denom)
        return self.norm

    def quantity(self, name):
        return {'p': self.p, 'exp_avg': self.m, 'exp_avg_sq': self.v}[name]


def error(tensors, twins):
    """E over a set of tensors: max|x - x64| / max|x64|, both maxima over all of them (None entries: no state, skipped)."""
    num = den = 0.0
    for x, x64 in zip(tensors, twins):
        if x is None:
            continue
        x = x.detach().double().cpu()
        num = max(num, float((x - x64).abs().max()))
        den = max(den, float(x64.abs().max()))
    return num / den if den else num


def state_of(opt, params, name):
    """The tensors of quantity `name` for `params` in order, out of an optimizer (None where it holds no state)."""
    if name == 'p':
        return list(params)
    return [opt.state[p][name] if p in opt.state and opt.state[p] else None for p in params]


def check_bar(label, fused, torch32, twin, norm_fused=None, norm_torch=None):
    """fused, torch32: (optimizer, params).  Prints every figure, then asserts the bar; returns the figures."""
    figures = {}
    for q in QUANTITIES:
        figures[q] = (error(state_of(*fused, q), twin.quantity(q)), error(state_of(*torch32, q), twin.quantity(q)))
    if norm_fused is not None:
        figures['norm'] = (abs(norm_fused - twin.norm) / twin.norm, abs(norm_torch - twin.norm) / twin.norm)
    for q, (ef, et) in figures.items():
        print(f'{label}: {q}: E_fused {ef:.3e}  E_torch {et:.3e}  ratio {ef / et if et else float("inf"):.3f}  bar {1.5 * et + 2 ** -23:.3e}')
    for q, (ef, et) in figures.items():
        assert ef <= 1.5 * et + 2 ** -23, (label, q, ef, et)
    return figures
