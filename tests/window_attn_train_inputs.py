"""Inputs, float64 gradients and error bounds of the dhd_window_attn_backward tests (no GPU needed here).

The cases, qkv, table and regions are those of window_attn_inputs.py, unchanged.  Added here: a seeded dout per case (randn,
rounded to the precision under test) and G = (dqkv, dtable), the gradients of section 17 of the header in float64 on the STORED
values (qkv and dout rounded to the precision under test; the table stays float32).  Computed once per (case, precision) and
handed out read-only.

Bounds, |g - G| <= E max(1, |G|max) per gradient tensor:
  float32 (bf16x3)        E = E_F32 = 1e-4, the project's float32 layer bar.
  dtable, all precisions  the same 1e-4: it is accumulated and stored in float32 from the unrounded dS.
  dqkv in fp16 / bf16     E = 2 E0, E0 = max |G - chain| with the chain = float64 arithmetic with P and dS rounded to the half
                          type where the products consume them (P for dV; dS for dQ and dK) and dQ, dK, dV rounded to the half
                          type at the end.  The factor 2 covers summation order and where exactly the kernel rounds."""
import functools

import numpy as np
import torch

import window_attn_inputs as I
from window_attn_inputs import CASES, E_F32, HEAD_DIM, NEIGHBOUR_CASES, PRECISIONS, SCALE, additive_term, geometry, inputs, scale_of, stored_qkv  # noqa: F401


@functools.lru_cache(maxsize=None)
def _dout32(case):
    wh, ww, n, b, nw, nh = geometry(case)
    gen = torch.Generator().manual_seed(17000 + sorted(CASES).index(case))
    return torch.randn(b, nw, n, nh * HEAD_DIM, generator=gen)


def stored_dout(case, prec):
    """dout (B, nW, N, nh * 32) as the precision under test stores it."""
    return _dout32(case).to(PRECISIONS[prec])


def relative_index(case):
    """int64 (N, N): the table row of the pair (query i, key j)."""
    wh, ww, n, b, nw, nh = geometry(case)
    ys, xs = np.divmod(np.arange(n), ww)
    return (ys[:, None] - ys[None, :] + wh - 1) * (2 * ww - 1) + (xs[:, None] - xs[None, :] + ww - 1)


def _heads_first(x, b, nw, n, nh):
    return x.reshape(b, nw, n, nh, HEAD_DIM).transpose(0, 1, 3, 2, 4)                   # (B, nW, nh, N, 32)


def _to_qkv(dq, dk, dv):
    b, nw, nh, n, d = dq.shape
    x = np.stack([dq, dk, dv], axis=0).transpose(1, 2, 4, 0, 3, 5)                      # (B, nW, N, 3, nh, 32)
    return torch.from_numpy(np.ascontiguousarray(x).reshape(b, nw, n, 3 * nh * d))


@functools.lru_cache(maxsize=None)
def _terms(case, prec):
    """float64 q, k, v, dO (B, nW, nh, N, 32), P and dS (B, nW, nh, N, N) of the stored inputs."""
    wh, ww, n, b, nw, nh = geometry(case)
    x = stored_qkv(case, prec).double().numpy().reshape(b, nw, n, 3, nh, HEAD_DIM)
    q, k, v = (x[:, :, :, i].transpose(0, 1, 3, 2, 4) for i in range(3))
    p, v2 = I._probabilities(case, prec)
    assert np.array_equal(v, v2)
    do = _heads_first(stored_dout(case, prec).double().numpy(), b, nw, n, nh)
    dp = np.matmul(do, v.transpose(0, 1, 2, 4, 3))
    ds = p * (dp - (p * dp).sum(-1, keepdims=True))
    return q, k, v, do, p, ds


@functools.lru_cache(maxsize=None)
def gradients(case, prec):
    """G: float64 torch tensors dqkv (B, nW, N, 3 * nh * 32) and dtable ((2 Wh - 1)(2 Ww - 1), nh)."""
    wh, ww, n, b, nw, nh = geometry(case)
    q, k, v, do, p, ds = _terms(case, prec)
    dq = SCALE * np.matmul(ds, k)
    dk = SCALE * np.matmul(ds.transpose(0, 1, 2, 4, 3), q)
    dv = np.matmul(p.transpose(0, 1, 2, 4, 3), do)
    rows = (2 * wh - 1) * (2 * ww - 1)
    per_head = ds.sum((0, 1)).reshape(nh, n * n)
    index = relative_index(case).reshape(-1)
    dtable = np.stack([np.bincount(index, weights=per_head[h], minlength=rows) for h in range(nh)], axis=1)
    return _to_qkv(dq, dk, dv), torch.from_numpy(dtable)


@functools.lru_cache(maxsize=None)
def bound_dqkv(case, prec):
    if prec == 'f32_bf16x3':
        return E_F32
    dt = PRECISIONS[prec]
    rnd = lambda a: torch.from_numpy(a).to(dt).double().numpy()
    q, k, v, do, p, ds = _terms(case, prec)
    pr, dsr = rnd(p), rnd(ds)
    chain = _to_qkv(SCALE * np.matmul(dsr, k), SCALE * np.matmul(dsr.transpose(0, 1, 2, 4, 3), q), np.matmul(pr.transpose(0, 1, 2, 4, 3), do))
    chain = chain.to(dt).double()
    return 2 * float((gradients(case, prec)[0] - chain).abs().max())


def bound_dtable(case, prec):
    return E_F32
