"""dhd_window_attn_backward on the GPU: the fused backward of the Swin window attention against the float64 gradients, through the
C ABI, through dhd_amd.window_attn + autograd and through SwinBlockSequence under activation checkpointing.

Inputs, reference gradients and bounds: window_attn_train_inputs.py.  |g - G| <= E max(1, |G|max) per gradient tensor:
  float32 qkv (bf16x3)     E = 1e-4, the project's float32 layer bar
  dtable, every precision  E = 1e-4 (accumulated and stored in float32 from the unrounded dS)
  dqkv in fp16 / bf16      E = 2 E0, E0 = max |G - chain| computed on the CPU (P and dS rounded to the half type where the products
                           consume them, dQ / dK / dV rounded at the end); the factor 2 covers summation order and where exactly
                           the kernel rounds.
dqkv is reproducible bit for bit; dtable is accumulated with LDS float atomics and the header gives no guarantee for its low
bits, so here dtable is compared within its bound and never byte for byte (tests/test_gpu_swin_composed.py compares its bytes).
Measured errors are printed by test_against_the_float64_gradients; docs/LAB_NOTEBOOK.md (R11.1) is where they are recorded."""
import copy

import pytest
import torch

from window_attn_train_inputs import (CASES, NEIGHBOUR_CASES, PRECISIONS, SCALE, bound_dqkv, bound_dtable, geometry, gradients, inputs,
                                      scale_of, stored_dout, stored_qkv)

pytestmark = pytest.mark.gpu

case_prec = lambda f: pytest.mark.parametrize('case', list(CASES))(pytest.mark.parametrize('prec', list(PRECISIONS))(f))

_DEV = {}


def device_inputs(case, prec, gpu):
    """(qkv and dout in the precision under test, table, regions or None) on the device, made once and only read."""
    key = (case, prec, str(gpu))
    if key not in _DEV:
        _, table, regions = inputs(case)
        _DEV[key] = (stored_qkv(case, prec).to(gpu), stored_dout(case, prec).to(gpu), table.to(gpu), None if regions is None else regions.to(gpu))
    return _DEV[key]


def capi(case, qkv, dout, table, regions, dqkv, dtable=None):
    """The C entry point on the tensors as they lie (qkv, dout and dqkv may be dense slices of larger parents); dtable and the
    scratch are fresh, dtable pre-filled with NaN.  -> (dqkv, dtable)"""
    from dhd_amd import _lib
    wh, ww, n, b, nw, nh = geometry(case)
    assert qkv.is_contiguous() and dout.is_contiguous() and dqkv.is_contiguous()
    lib = _lib.load()
    windows = qkv.numel() // (n * 96 * nh)
    if dtable is None:
        dtable = torch.full(tuple(table.shape), float('nan'), dtype=torch.float32, device=qkv.device)
    nbytes = lib.dhd_window_attn_backward_scratch_bytes(windows, wh, ww, nh)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=qkv.device)
    rc = lib.dhd_window_attn_backward(_lib.ptr(qkv), _lib.ptr(dout), _lib.DTYPE_CODE[qkv.dtype], _lib.ptr(table), _lib.ptr(regions), _lib.ptr(dqkv),
                                      _lib.ptr(dtable), _lib.ptr(scratch), nbytes, windows, nw, wh, ww, nh, 32, SCALE, 0,
                                      _lib.stream_ptr(qkv.device))
    torch.cuda.synchronize()
    assert rc == 0, rc
    return dqkv, dtable


def run_capi(case, qkv, dout, table, regions):
    """Through the C ABI with dqkv and dtable pre-filled with NaN."""
    return capi(case, qkv, dout, table, regions, torch.full_like(qkv, float('nan')))


def rel_err(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max()) / scale_of(ref)


@case_prec
def test_against_the_float64_gradients(gpu, case, prec):
    """Every element of dqkv and dtable written (both start as NaN), finite and within the bounds; a second call writes the same
    dqkv bytes (and a dtable within its bound: the header does not claim its low bits); the inputs are only read."""
    qkv, dout, table, regions = device_inputs(case, prec, gpu)
    ins = (qkv, dout, table) + (() if regions is None else (regions,))
    keep = [t.clone() for t in ins]
    (G_qkv, G_tab), E_qkv, E_tab = gradients(case, prec), bound_dqkv(case, prec), bound_dtable(case, prec)
    dqkv, dtable = run_capi(case, qkv, dout, table, regions)
    assert dqkv.dtype == qkv.dtype and dqkv.shape == G_qkv.shape and dtable.dtype == torch.float32 and dtable.shape == G_tab.shape
    assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(dtable).all())
    e_qkv, e_tab = rel_err(dqkv, G_qkv), rel_err(dtable, G_tab)
    parts = dqkv.cpu().double().view(-1, 3, qkv.shape[-1] // 3) - G_qkv.view(-1, 3, qkv.shape[-1] // 3)
    print(f'window_attn_backward {prec} {case}: dqkv err {e_qkv:.3e} (bound {E_qkv:.3e}, |G|max {float(G_qkv.abs().max()):.2f}; '
          f'dq / dk / dv abs {float(parts[:, 0].abs().max()):.3e} / {float(parts[:, 1].abs().max()):.3e} / {float(parts[:, 2].abs().max()):.3e}), '
          f'dtable err {e_tab:.3e} (bound {E_tab:.1e}, |G|max {float(G_tab.abs().max()):.2f})')
    assert e_qkv <= E_qkv, (e_qkv, E_qkv)
    assert e_tab <= E_tab, (e_tab, E_tab)
    again, tab_again = run_capi(case, qkv, dout, table, regions)
    assert torch.equal(again.view(torch.uint8), dqkv.view(torch.uint8))
    assert rel_err(tab_again, G_tab) <= E_tab
    assert all(torch.equal(a, b) for a, b in zip(ins, keep))


@pytest.mark.parametrize('case', NEIGHBOUR_CASES)
@pytest.mark.parametrize('prec', list(PRECISIONS))
def test_neighbouring_windows_are_neither_read_nor_written(gpu, case, prec):
    """qkv and dout are the dense slices [1:-1] of parents whose first and last windows are NaN, dqkv sits inside a NaN-filled
    parent: the fresh run's bytes, the poison as it was, the input parents byte-identical afterwards.  N = 49 is padded to 64
    inside the kernel: a kernel that loaded padded rows from the next window would carry its NaN into dtable or dqkv, one that
    stored padded rows would overwrite the poison."""
    qkv, dout, table, regions = device_inputs(case, prec, gpu)
    fresh, fresh_tab = run_capi(case, qkv, dout, table, regions)

    def parent_of(t):
        flat = t.reshape(-1, t.shape[-2], t.shape[-1])
        p = torch.full((flat.shape[0] + 2,) + tuple(flat.shape[1:]), float('nan'), dtype=t.dtype, device=gpu)
        p[1:-1] = flat
        return p
    qparent, dparent = parent_of(qkv), parent_of(dout)
    gparent = torch.full_like(qparent, float('nan'))
    snaps = [p.view(torch.uint8).clone() for p in (qparent, dparent)]
    got, got_tab = capi(case, qparent[1:-1], dparent[1:-1], table, regions, gparent[1:-1])
    assert got.data_ptr() == gparent[1].data_ptr() and all(p[1].data_ptr() % 16 == 0 for p in (qparent, dparent, gparent))
    assert torch.equal(got.reshape(fresh.shape).view(torch.uint8), fresh.view(torch.uint8))
    assert bool(torch.isfinite(got_tab).all()) and rel_err(got_tab, gradients(case, prec)[1]) <= bound_dtable(case, prec)
    assert all(torch.equal(p.view(torch.uint8), s) for p, s in zip((qparent, dparent), snaps))
    assert bool(torch.isnan(gparent[0]).all()) and bool(torch.isnan(gparent[-1]).all())


@pytest.mark.parametrize('prec', list(PRECISIONS))
def test_uniform_attention_has_exact_gradients(gpu, prec):
    """q = 0, a zero table, no regions, N = 16: every probability is 1 / 16.  With small-integer V and dout, dV is the mean over
    the queries of dout (multiples of 1 / 16 below 4) and dK is 0, both exactly in every precision.  dS = (dP - rowmean(dP)) / 16
    is a multiple of 2^-8 (exact in float32 and as two bf16 parts, rounded once in the half types), so dQ = scale dS K is
    compared to within two roundings of the format; dtable sums dS per offset."""
    from dhd_amd import window_attn
    dt = PRECISIONS[prec]
    gen = torch.Generator().manual_seed(6)
    nh, n, w = 2, 16, 3
    qkv = torch.randn(w, n, 3, nh, 32, generator=gen)
    qkv[:, :, 0] = 0
    qkv[:, :, 2] = torch.randint(-3, 4, (w, n, nh, 32), generator=gen).float()
    qkv = qkv.to(dt)
    dout = torch.randint(-3, 4, (w, n, nh, 32), generator=gen).float()
    k, v, do = qkv[:, :, 1].double(), qkv[:, :, 2].double(), dout.double()
    dp = torch.einsum('wihc,wjhc->whij', do, v)
    ds = (dp - dp.mean(-1, keepdim=True)) / n
    dq = SCALE * torch.einsum('whij,wjhc->wihc', ds, k)
    dv = do.mean(1, keepdim=True).expand(w, n, nh, 32)
    x = qkv.reshape(w, n, 96 * nh).to(gpu).requires_grad_()
    table = torch.zeros(49, nh, device=gpu, requires_grad=True)
    window_attn(x, table, (4, 4), nh, SCALE).backward(dout.reshape(w, n, nh * 32).to(gpu).to(dt))
    g = x.grad.cpu().double().view(w, n, 3, nh, 32)
    assert x.grad.dtype == dt and table.grad.dtype == torch.float32
    assert torch.equal(g[:, :, 2], dv), 'dV is not the exact mean of dout'
    assert torch.equal(g[:, :, 1], torch.zeros_like(dv)), 'dK is not exactly 0'
    eps = {'f32_bf16x3': 2.0 ** -16, 'fp16': 2.0 ** -11, 'bf16': 2.0 ** -8}[prec]
    assert float((g[:, :, 0] - dq).abs().max()) <= 2 * eps * max(1.0, float(dq.abs().max()))
    index = torch.arange(n).view(4, 4)
    rel = ((index // 4).view(-1, 1) - (index // 4).view(1, -1) + 3) * 7 + (index % 4).view(-1, 1) - (index % 4).view(1, -1) + 3
    ref = torch.zeros(49, nh, dtype=torch.float64).index_add_(0, rel.reshape(-1), ds.sum(0).permute(1, 2, 0).reshape(n * n, nh))
    assert float((table.grad.cpu().double() - ref).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max()))


VIEW_CASE = 'ws7_21x14_shift3_nh3'


def _autograd(case, qkv, dout, table, regions, table_dtype=torch.float32):
    from dhd_amd import window_attn
    wh, ww, n, b, nw, nh = geometry(case)
    x, t = qkv.detach().clone().requires_grad_(), table.detach().to(table_dtype).requires_grad_()
    out = window_attn(x, t, (wh, ww), nh, SCALE, regions=regions)
    out.backward(dout)
    torch.cuda.synchronize()
    return out.detach(), x.grad, t.grad


@pytest.mark.parametrize('case', ['ws12_24x36_shift6_b2_nh4', VIEW_CASE, 'win3x5_nonsquare_nh2'])
@pytest.mark.parametrize('prec', list(PRECISIONS))
def test_autograd_gives_the_c_abi_bytes(gpu, case, prec):
    """window_attn(...).backward(dout): the forward is window_attn_infer's, dqkv is the C-ABI run's bytes, dtable is within its bound
    (not byte-compared: LDS float atomics) and comes back in the parameter's dtype and shape."""
    from dhd_amd import window_attn_infer
    qkv, dout, table, regions = device_inputs(case, prec, gpu)
    wh, ww, n, b, nw, nh = geometry(case)
    fresh, _ = run_capi(case, qkv, dout, table, regions)
    out, dqkv, dtable = _autograd(case, qkv, dout, table, regions)
    assert torch.equal(out, window_attn_infer(qkv, table, (wh, ww), nh, SCALE, regions=regions))
    assert dqkv.dtype == qkv.dtype and dqkv.shape == qkv.shape and torch.equal(dqkv.view(torch.uint8), fresh.view(torch.uint8))
    assert dtable.dtype == torch.float32 and dtable.shape == table.shape
    assert rel_err(dtable, gradients(case, prec)[1]) <= bound_dtable(case, prec)
    if prec != 'f32_bf16x3':                          # a parameter kept in the half type gets its gradient in that type
        _, dq2, dt2 = _autograd(case, qkv, dout, table.to(qkv.dtype).float(), regions, table_dtype=qkv.dtype)
        assert dt2.dtype == qkv.dtype and dt2.shape == table.shape and bool(torch.isfinite(dt2).all())


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('kind', ['offset16', 'offset_elem', 'inner_step2'])
def test_a_strided_or_misaligned_dout_is_copied(gpu, prec, kind):
    """dout shown as a view carved out of a poisoned parent (test_gpu_views.present): the fresh run's dqkv bytes, and every byte of
    the parent, values and poison, as it was."""
    from test_gpu_views import present
    qkv, dout, table, regions = device_inputs(VIEW_CASE, prec, gpu)
    _, fresh, _ = _autograd(VIEW_CASE, qkv, dout, table, regions)
    view, parent = present(dout, kind)
    snap = parent.view(torch.uint8).clone()
    _, got, got_tab = _autograd(VIEW_CASE, qkv, view, table, regions)
    assert got.is_contiguous() and torch.equal(got.view(torch.uint8), fresh.view(torch.uint8))
    assert rel_err(got_tab, gradients(VIEW_CASE, prec)[1]) <= bound_dtable(VIEW_CASE, prec)
    assert torch.equal(parent.view(torch.uint8), snap), 'a parent buffer changed'


# --------------------------------------------------------------------------- the module path

def _recorder(monkeypatch):
    """-> list of the names that reach _lib.call (the operator's only way into the library)."""
    from dhd_amd import _lib
    seen = []
    real_call = _lib.call

    def call(name, *a):
        seen.append(name)
        return real_call(name, *a)
    monkeypatch.setattr(_lib, 'call', call)
    return seen


FWD, BWD = 'dhd_window_attn_infer', 'dhd_window_attn_backward'
_SEQ = {}


def _sequence(gpu):
    """SwinBlockSequence of two blocks (plain + shifted, window 7, 3 heads, with_cp=True) on a 21 x 14 map, B = 2, with randomised
    tables; the float32 module on the GPU (train mode), its input, the gradient of its output, and the same step's output and
    parameter gradients from a float64 copy on the CPU.  Made once; tests work on copies of the module."""
    if 'm' not in _SEQ:
        from dhd_amd.swin import SwinBlockSequence, WindowMSA
        torch.manual_seed(21)
        m = SwinBlockSequence(96, 3, 192, 2, window_size=7, with_cp=True).train()
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, WindowMSA):
                    mod.relative_position_bias_table.normal_(0, 0.5)
        x, g = torch.randn(2, 21 * 14, 96), torch.randn(2, 21 * 14, 96)
        m64 = copy.deepcopy(m).double()
        x64 = x.double().requires_grad_()
        out64 = m64(x64, (21, 14), {})[0]
        out64.backward(g.double())
        ref = [out64.detach(), x64.grad] + [p.grad for p in m64.parameters()]
        _SEQ.update(m=m.to(gpu), x=x.to(gpu), g=g.to(gpu), ref=ref, names=['out', 'dx'] + [k for k, _ in m64.named_parameters()])
    return copy.deepcopy(_SEQ['m']), _SEQ['x'], _SEQ['g'], _SEQ['ref'], _SEQ['names']


def _step(m, x, g, autocast=None):
    """One forward + backward from the module's state -> [out, dx, every parameter gradient]"""
    m.zero_grad()
    x = x.detach().clone().requires_grad_()
    with torch.autocast('cuda', dtype=autocast, enabled=autocast is not None):
        out = m(x, (21, 14), {})[0]
    out.backward(g.to(out.dtype))
    torch.cuda.synchronize()
    return [out.detach(), x.grad] + [p.grad for p in m.parameters()]


def test_block_sequence_float32_matches_todays_path(gpu, monkeypatch):
    """Train mode, activation checkpointing, the same state: with fused_train the backward entry point is reached once per block
    and the forward twice (the checkpoint re-runs it), with it off neither attention entry point; output and every parameter
    gradient agree within the float32 bound."""
    import dhd_amd
    m, x, g, _, names = _sequence(gpu)
    seen = _recorder(monkeypatch)
    today = _step(m, x, g)
    assert FWD not in seen and BWD not in seen, seen
    assert len(dhd_amd.fused_training(m)) == 2
    del seen[:]
    got = _step(m, x, g)
    assert seen.count(BWD) == 2 and seen.count(FWD) == 4, seen
    assert len(got) == len(today) == len(names)
    for name, a, b in zip(names, got, today):
        err = float((a.double() - b.double()).abs().max()) / max(1.0, float(b.abs().max()))
        print(f'SwinBlockSequence float32 fused_train vs today, {name}: {err:.3e}')
        assert a.shape == b.shape and a.dtype == b.dtype and err <= 1e-4, (name, err)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_block_sequence_under_autocast_is_no_worse_than_todays_path(gpu, monkeypatch, dtype):
    """Both paths round qkv and proj alike; the fused one keeps the bias and its gradient in float32.  Per tensor (output, input
    gradient, every parameter gradient) its distance to the float64 step is at most 2 x the distance of today's autocast path to
    the same float64 step."""
    import dhd_amd
    m, x, g, ref, names = _sequence(gpu)
    today = _step(m, x, g, autocast=dtype)
    dhd_amd.fused_training(m)
    seen = _recorder(monkeypatch)
    got = _step(m, x, g, autocast=dtype)
    assert seen.count(BWD) == 2 and seen.count(FWD) == 4, seen
    for name, a, b, r in zip(names, got, today, ref):
        e_new, e_old = (float((t.cpu().double() - r).abs().max()) for t in (a, b))
        print(f'SwinBlockSequence autocast {dtype} {name}: error vs float64 fused {e_new:.3e}, today {e_old:.3e}')
        assert a.shape == b.shape and a.dtype == b.dtype and e_new <= 2 * e_old, (name, e_new, e_old)


def test_no_grad_forward_in_training_mode_takes_the_operator(gpu, monkeypatch):
    import dhd_amd
    m, x, g, _, _ = _sequence(gpu)
    with torch.no_grad():
        today = m(x, (21, 14), {})[0]
    dhd_amd.fused_training(m)
    seen = _recorder(monkeypatch)
    with torch.no_grad():
        out = m(x, (21, 14), {})[0]
    torch.cuda.synchronize()
    assert m.training and seen.count(FWD) == 2 and BWD not in seen, seen
    err = float((out.double() - today.double()).abs().max()) / max(1.0, float(today.abs().max()))
    assert out.shape == today.shape and err <= 1e-4, err


def test_dropout_and_head_dimension_keep_sdpa(gpu, monkeypatch):
    """Attention dropout p > 0 in train mode, and a head dimension the kernel does not have, fall through to SDPA with the flag on;
    the same module in eval mode takes the operator."""
    from dhd_amd.swin import WindowMSA
    torch.manual_seed(3)
    x = torch.randn(1, 2, 49, 64, device=gpu)
    seen = _recorder(monkeypatch)
    drop = WindowMSA(64, 2, (7, 7), attn_drop_rate=0.1).to(gpu).train()
    drop.fused_train = True
    drop(x).sum().backward()
    assert FWD not in seen and BWD not in seen, seen
    drop.eval()
    drop(x).sum().backward()
    assert seen.count(FWD) == 1 and seen.count(BWD) == 1, seen
    del seen[:]
    hd16 = WindowMSA(64, 4, (7, 7)).to(gpu).train()
    hd16.fused_train = True
    hd16(x).sum().backward()
    torch.cuda.synchronize()
    assert FWD not in seen and BWD not in seen, seen


def _peak_case(gpu, batch):
    from dhd_amd.swin import WindowMSA, shift_window_mask, shift_window_regions
    torch.manual_seed(4)
    m = WindowMSA(128, 4, (12, 12)).to(gpu).train()
    x = torch.randn(batch, 6, 144, 128, device=gpu)
    return m, x, shift_window_mask(24, 36, 12, 6, gpu), shift_window_regions(24, 36, 12, 6, gpu)


def test_peak_allocation_is_lower_with_the_operator(gpu):
    """One WindowMSA forward + backward at the N = 144 case (6 windows of 12 x 12, 4 heads, shifted), 16 images: peak allocation
    above the resident state, flag on against flag off.  The batch is 16 and not the 2 of the numerical case because the peak of
    a whole step also contains what torch takes around the Linear layers: the sum over rows for the qkv bias gradient allocates
    a temporary inside the call, the same on both paths (21 MB at 2 images, 48 MiB from 8 images on, on the MI355X; on a device
    where the reduction is split differently it is not taken).  At 2 and at 8 images it is larger than everything the
    attention allocates and the two peaks are the same number; at 16 images today's path holds 98 MB around SDPA's backward,
    the operator at most dqkv + that temporary = 72 MB, and the temporary no longer decides."""
    m, x, mask, regions = _peak_case(gpu, 16)

    def peak():
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(gpu)
        base = torch.cuda.memory_allocated(gpu)
        m(x, mask, regions=regions).sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(gpu) - base
    peak()                                     # warm-up: library handles and cached workspaces are allocated once
    off = peak()
    m.fused_train = True
    peak()
    on = peak()
    print(f'WindowMSA N = 144, 16 images, forward + backward, peak allocation above the resident state: today {off} B, fused_train {on} B')
    assert on < off, (on, off)


def test_the_attention_allocates_less_with_the_operator(gpu):
    """The same module at 2 images (the numerical case): the peak of the forward, what the graph holds between forward and backward, and the peak of the
    backward up to the qkv Linear's (measured by differentiating to qkv: the attention and proj only) are each lower with the
    flag on -- the permuted operands, the expanded bias and what SDPA saves do not exist."""
    m, x, mask, regions = _peak_case(gpu, 2)

    def figures():
        got = {}

        def grab(mod, args, out):
            got['qkv'] = out
        handle = m.qkv.register_forward_hook(grab)
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(gpu)
        base = torch.cuda.memory_allocated(gpu)
        out = m(x, mask, regions=regions)
        handle.remove()
        torch.cuda.synchronize()
        forward_peak, held = torch.cuda.max_memory_allocated(gpu) - base, torch.cuda.memory_allocated(gpu) - base
        grads = torch.autograd.grad(out.sum(), (got.pop('qkv'), m.relative_position_bias_table))
        torch.cuda.synchronize()
        return forward_peak, held, torch.cuda.max_memory_allocated(gpu) - base, grads
    figures()
    off = figures()[:3]
    m.fused_train = True
    figures()
    on = figures()[:3]
    print(f'WindowMSA N = 144, bytes above the resident state (forward peak, held after forward, peak up to dqkv): today {off}, fused_train {on}')
    assert all(a < b for a, b in zip(on, off)), (on, off)
