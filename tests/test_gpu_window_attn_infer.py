"""dhd_window_attn_infer on the GPU: the fused Swin window attention of inference against the float64 formula, through the C ABI,
through dhd_amd.window_attn_infer and through WindowMSA / ShiftWindowMSA / SwinTransformer.

Inputs, reference and bounds: window_attn_inputs.py.  One bound per precision, |y - R| <= E max(1, |R|max):
  float32 qkv (bf16x3)   E = 1e-4, the project's float32 layer bar
  fp16 / bf16 qkv        E = 2 E0, E0 = max |R - chain| computed on the CPU (float64 softmax rounded to the half type, float64
                         P V rounded to it); the factor 2 covers summation order and rounding the unnormalised exponentials.
Measured errors are printed by test_against_the_float64_reference and recorded in docs/LAB_NOTEBOOK.md."""
import copy

import pytest
import torch

from window_attn_inputs import CASES, NEIGHBOUR_CASES, PRECISIONS, SCALE, bound, geometry, inputs, reference, scale_of, stored_qkv

pytestmark = pytest.mark.gpu

case_prec = lambda f: pytest.mark.parametrize('case', list(CASES))(pytest.mark.parametrize('prec', list(PRECISIONS))(f))

_DEV = {}


def device_inputs(case, prec, gpu):
    """(qkv in the precision under test, table, regions or None) on the device, made once and only read."""
    key = (case, prec, str(gpu))
    if key not in _DEV:
        _, table, regions = inputs(case)
        _DEV[key] = (stored_qkv(case, prec).to(gpu), table.to(gpu), None if regions is None else regions.to(gpu))
    return _DEV[key]


def run(case, qkv, table, regions, **kw):
    from dhd_amd import window_attn_infer
    wh, ww, n, b, nw, nh = geometry(case)
    return window_attn_infer(qkv, table, (wh, ww), nh, SCALE, regions=regions, **kw)


def capi(case, qkv, table, regions, out):
    """The C entry point on the tensors as they lie (qkv and out may be dense slices of larger parents)."""
    from dhd_amd import _lib
    wh, ww, n, b, nw, nh = geometry(case)
    assert qkv.is_contiguous() and out.is_contiguous()
    rc = _lib.load().dhd_window_attn_infer(_lib.ptr(qkv), _lib.DTYPE_CODE[qkv.dtype], _lib.ptr(table), _lib.ptr(regions), _lib.ptr(out),
                                           qkv.numel() // (n * 96 * nh), nw, wh, ww, nh, 32, SCALE, 0, _lib.stream_ptr(qkv.device))
    torch.cuda.synchronize()
    assert rc == 0
    return out


def run_capi(case, qkv, table, regions):
    """Through the C ABI with `out` pre-filled with NaN."""
    return capi(case, qkv, table, regions, torch.full(tuple(qkv.shape[:-1]) + (qkv.shape[-1] // 3,), float('nan'), dtype=qkv.dtype, device=qkv.device))


@case_prec
def test_against_the_float64_reference(gpu, case, prec):
    """Every element written (out starts as NaN), finite and within E of the float64 reference; the same bytes from a second call
    and through the Python wrapper; the inputs are only read."""
    qkv, table, regions = device_inputs(case, prec, gpu)
    keep = [t.clone() for t in (qkv, table) + (() if regions is None else (regions,))]
    ref, E = reference(case, prec), bound(case, prec)
    y = run_capi(case, qkv, table, regions)
    assert y.dtype == qkv.dtype and y.shape == ref.shape
    assert bool(torch.isfinite(y).all())
    err = float((y.cpu().double() - ref).abs().max()) / scale_of(ref)
    print(f'window_attn_infer {prec} {case}: max |y - float64| / max(1, |R|max) = {err:.3e}, bound E = {E:.3e}, |R|max = {float(ref.abs().max()):.2f}')
    assert err <= E, (err, E)
    assert torch.equal(run_capi(case, qkv, table, regions), y)
    wrapped = run(case, qkv, table, regions)
    assert torch.equal(wrapped, y) and wrapped.is_contiguous() and wrapped.dtype == qkv.dtype
    assert all(torch.equal(a, b) for a, b in zip((qkv, table) + (() if regions is None else (regions,)), keep))


@pytest.mark.parametrize('case', NEIGHBOUR_CASES)
@pytest.mark.parametrize('prec', list(PRECISIONS))
def test_neighbouring_windows_are_neither_read_nor_written(gpu, case, prec):
    """qkv is the dense slice [1:-1] of a parent whose first and last windows are NaN, out sits inside a NaN-filled parent: the
    fresh run's bytes, and the parents' poison as it was.  N = 49 is padded to 64 inside the kernel: a kernel that loaded padded V
    rows or padded queries from the next window, or stored padded rows, fails here.  A padded K row read from the neighbour would
    not show (its scores are replaced by -inf before use); that the kernel writes zeros there is read off its source."""
    qkv, table, regions = device_inputs(case, prec, gpu)
    fresh = run_capi(case, qkv, table, regions)
    flat = qkv.reshape(-1, qkv.shape[-2], qkv.shape[-1])
    qparent = torch.full((flat.shape[0] + 2,) + tuple(flat.shape[1:]), float('nan'), dtype=qkv.dtype, device=gpu)
    qparent[1:-1] = flat
    oparent = torch.full((flat.shape[0] + 2, flat.shape[1], flat.shape[2] // 3), float('nan'), dtype=qkv.dtype, device=gpu)
    qsnap = qparent.view(torch.uint8).clone()
    got = capi(case, qparent[1:-1], table, regions, oparent[1:-1])
    assert got.data_ptr() == oparent[1].data_ptr() and got.data_ptr() % 16 == 0 and qparent[1].data_ptr() % 16 == 0
    assert torch.equal(got.reshape(fresh.shape), fresh)
    assert torch.equal(qparent.view(torch.uint8), qsnap)
    assert bool(torch.isnan(oparent[0]).all()) and bool(torch.isnan(oparent[-1]).all())


@pytest.mark.parametrize('prec', list(PRECISIONS))
def test_uniform_attention_is_the_exact_mean_of_v(gpu, prec):
    """q = 0, a zero table, no regions: every probability is 1 / 16, and with small-integer V every output row is the exact mean
    of V (multiples of 1 / 16 below 4: exact in every precision)."""
    from dhd_amd import window_attn_infer
    gen = torch.Generator().manual_seed(5)
    nh, n, w = 2, 16, 3
    qkv = torch.randn(w, n, 3, nh, 32, generator=gen)
    qkv[:, :, 0] = 0
    qkv[:, :, 2] = torch.randint(-3, 4, (w, n, nh, 32), generator=gen).float()
    mean = qkv[:, :, 2].double().mean(1, keepdim=True).expand(w, n, nh, 32).reshape(w, n, nh * 32)
    y = window_attn_infer(qkv.reshape(w, n, 96 * nh).to(gpu).to(PRECISIONS[prec]), torch.zeros(49, nh, device=gpu), (4, 4), nh, SCALE)
    assert y.dtype == PRECISIONS[prec] and torch.equal(y.cpu().double(), mean)


VIEW_CASE = 'ws7_21x14_shift3_nh3'


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('kind', ['offset16', 'offset_elem', 'inner_step2'])
def test_views_of_qkv(gpu, prec, kind):
    """qkv shown as a view carved out of a poisoned parent (test_gpu_views.present): the fresh run's bytes (the wrapper copies a
    view the kernel cannot read where it lies), and every byte of the parent, values and poison, as it was."""
    from test_gpu_views import present
    qkv, table, regions = device_inputs(VIEW_CASE, prec, gpu)
    fresh = run(VIEW_CASE, qkv, table, regions)
    view, parent = present(qkv, kind)
    snap = parent.view(torch.uint8).clone()
    got = run(VIEW_CASE, view, table, regions)
    torch.cuda.synchronize()
    assert got.is_contiguous() and got.dtype == fresh.dtype and torch.equal(got, fresh)
    assert torch.equal(parent.view(torch.uint8), snap), 'a parent buffer changed'


# --------------------------------------------------------------------------- the module path

def _recorder(monkeypatch):
    """-> list of the names that reach _lib.call (the new operator's only way into the library) followed by the `what` of every
    _lib.check (how the older wrappers report an entry point), as 'call:<name>' / 'check:<name>'."""
    from dhd_amd import _lib
    seen = []
    real_call, real_check = _lib.call, _lib.check

    def call(name, *a):
        seen.append('call:' + name)
        return real_call(name, *a)

    def check(rc, what):
        seen.append('check:' + what)
        return real_check(rc, what)
    monkeypatch.setattr(_lib, 'call', call)
    monkeypatch.setattr(_lib, 'check', check)
    return seen


ENTRY = 'call:dhd_window_attn_infer'
_MSA = {}


def _msa_case(gpu):
    """ShiftWindowMSA(64, 2, 7, shift 3) with a randomised table on a 13 x 19 map (padded to 14 x 21), B = 2; the module (eval, on
    the GPU), its input, and the same module's float64 result on the CPU.  Made once; tests work on copies of the module."""
    if 'm' not in _MSA:
        from dhd_amd.swin import ShiftWindowMSA
        torch.manual_seed(11)
        m = ShiftWindowMSA(64, 2, 7, shift_size=3).eval()
        with torch.no_grad():
            m.w_msa.relative_position_bias_table.normal_(0, 0.5)
        x = torch.randn(2, 13 * 19, 64)
        with torch.no_grad():
            ref = copy.deepcopy(m).double()(x.double(), (13, 19))
        _MSA.update(m=m.to(gpu), x=x.to(gpu), ref=ref)
    return copy.deepcopy(_MSA['m']), _MSA['x'], _MSA['ref']


def test_module_float32_against_float64(gpu, monkeypatch):
    m, x, ref = _msa_case(gpu)
    m.w_msa.fused_infer = True
    seen = _recorder(monkeypatch)
    with torch.no_grad():
        out = m(x, (13, 19), {})
    torch.cuda.synchronize()
    assert seen.count(ENTRY) == 1, seen
    err = float((out.cpu().double() - ref).abs().max()) / scale_of(ref)
    print(f'ShiftWindowMSA float32, fused: max error vs float64 / max(1, |ref|max) = {err:.3e}')
    assert out.dtype == torch.float32 and err <= 1e-4, err


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_module_under_autocast_is_no_worse_than_todays_path(gpu, monkeypatch, dtype):
    """Both paths round qkv and proj alike and the fused one keeps the bias in float32: its error against the float64 module is
    at most 2 x the error of today's path (switch off) against the same reference; the 2 is for summation order."""
    m, x, ref = _msa_case(gpu)
    masks = {}
    with torch.no_grad(), torch.autocast('cuda', dtype=dtype):
        today = m(x, (13, 19), masks)
        m.w_msa.fused_infer = True
        seen = _recorder(monkeypatch)
        out = m(x, (13, 19), masks)
    torch.cuda.synchronize()
    assert seen.count(ENTRY) == 1 and out.dtype == today.dtype == dtype and out.shape == today.shape
    assert sorted(len(k) for k in masks) == [5, 6]                   # the mask and, under its own key, the regions
    e_new, e_old = (float((t.cpu().double() - ref).abs().max()) for t in (out, today))
    print(f'ShiftWindowMSA autocast {dtype}: error vs float64 fused {e_new:.3e}, today {e_old:.3e}')
    assert e_new <= 2 * e_old, (e_new, e_old)


def _small_swin(gpu):
    from dhd_amd.swin import SwinTransformer, WindowMSA
    torch.manual_seed(12)
    net = SwinTransformer(embed_dims=32, patch_size=4, window_size=4, depths=(2, 2), num_heads=(1, 2), strides=(4, 2),
                          out_indices=(0, 1), drop_path_rate=0., with_cp=False)
    net.init_weights()
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, WindowMSA):
                mod.relative_position_bias_table.normal_(0, 0.5)
            elif isinstance(mod, torch.nn.Linear):
                mod.weight.normal_(0, mod.in_features ** -0.5)
    return net.to(gpu).eval(), torch.randn(2, 3, 40, 56, device=gpu)


def test_small_swin_reaches_the_operator_once_per_block(gpu, monkeypatch):
    import dhd_amd
    net, x = _small_swin(gpu)
    with torch.no_grad():
        today = net(x)
    assert len(dhd_amd.fused_inference(net)) == 4
    seen = _recorder(monkeypatch)
    with torch.no_grad():
        outs = net(x)
    torch.cuda.synchronize()
    assert seen.count(ENTRY) == 4, seen
    for o, t in zip(outs, today):
        err = float((o.double() - t.double()).abs().max()) / max(1.0, float(t.abs().max()))
        print(f'small SwinTransformer, fused vs today: {err:.3e}')
        assert o.shape == t.shape and err <= 1e-4, err


@pytest.mark.parametrize('how', ['default_switch', 'train_mode', 'requires_grad'])
def test_todays_path_stays(gpu, monkeypatch, how):
    """The switch at its default, train mode, or an input that requires grad under enabled grad: the entry point is not reached
    and the output equals today's path bit for bit."""
    m, x, _ = _msa_case(gpu)
    m.train(how == 'train_mode')

    def go():
        if how == 'requires_grad':
            return m(x.clone().requires_grad_(), (13, 19), {}).detach()
        with torch.no_grad():
            return m(x, (13, 19), {})
    today = go()                               # the switch off: the parent's path
    if how != 'default_switch':
        m.w_msa.fused_infer = True
    seen = _recorder(monkeypatch)
    out = go()
    torch.cuda.synchronize()
    assert ENTRY not in seen and seen.count('check:dhd_window_rows') == 2, seen
    assert torch.equal(out.detach(), today)


def test_head_dimension_8_falls_back(gpu, monkeypatch):
    """The G10 fixture's Swin (head dimension 8): with the switch on it takes today's path, bit for bit."""
    import dhd_amd
    from conftest import golden
    from test_host_logic import swin_from_fixture
    g = golden('g10_swin')
    net = swin_from_fixture(g).to(gpu)
    x = torch.from_numpy(g['x']).to(gpu)
    with torch.no_grad():
        today = net(x)
    assert len(dhd_amd.fused_inference(net)) == 6
    seen = _recorder(monkeypatch)
    with torch.no_grad():
        outs = net(x)
    torch.cuda.synchronize()
    assert ENTRY not in seen
    assert len(outs) == len(today) and all(torch.equal(a, b) for a, b in zip(outs, today))


@pytest.mark.parametrize('prec', list(PRECISIONS))
def test_call_is_graph_capturable(gpu, prec):
    """One capture and replay of the wrapper gives the eager bytes, also on fresh contents of the static qkv: nothing but `out` is
    allocated and nothing is synchronised inside the call."""
    case = 'ws7_21x14_shift3_nh3'
    qkv, table, regions = device_inputs(case, prec, gpu)
    qkv = qkv.clone()
    qkv2 = (qkv.float() * 0.5 + 0.25).to(qkv.dtype)
    ref1, ref2 = run(case, qkv, table, regions).clone(), run(case, qkv2, table, regions).clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(case, qkv, table, regions)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = run(case, qkv, table, regions)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, ref1)
    qkv.copy_(qkv2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, ref2) and not torch.equal(ref1, ref2)
