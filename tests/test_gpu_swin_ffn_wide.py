"""The wide Swin FFN operator (C = 512 and 1024: dhd_amd/swin_ffn.py, csrc/swin_ffn_wide.h) on the GPU: against the float64 twin of
tests/swin_ffn_wide_inputs.py at every case and dtype combination, row independence, repeatability, guard bands, views, the routed
SwinBlock, graph capture and the peak allocation.  The counterpart of tests/test_gpu_swin_ffn.py.

Bars (the project's own).  GEMMs in float32 (bf16x3): max error <= 1e-4 max(1, |out|max), the layer bar: the narrow kernel measured
6.4e-5 at |out|max 10.4 against a bound of 1.04e-3, and a 4 x longer sum keeps that inside even if the error grew linearly (an
argument, not a measurement).  GEMMs in a half type: the parent formulation (torch layer_norm / linear / gelu / linear / add in
the same dtypes on the same tensors) is run in the same test and its error against the twin taken; the fused error may be at most
1.5 x that -- its rounding points are a subset of the parent's (the pre-activations are never rounded), and the margin covers a
maximum taken over a different accumulation order."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as G  # noqa: E402
import swin_ffn_wide_inputs as SW  # noqa: E402

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
BAR, MARGIN = 1e-4, 1.5
WIDE, NARROW = 'dhdg_swin_ffn_wide_infer', 'dhdf_swin_ffn_infer'
pytestmark = pytest.mark.gpu
GRID = [pytest.param(c, p, id=f'{c}-{p}') for c in SW.CASES for p in SW.PRECISIONS]


def _sync():
    """Wait for the device; after a device error nothing more is started in this module."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'GPU fault, stopping the module: {e}', returncode=3)


def _on(gpu, case, prec):
    return {k: (None if t is None else t.to(gpu)) for k, t in SW.inputs(case, prec).items()}


def _run(v, mdt, x=None):
    from dhd_amd import swin_ffn_infer
    out = swin_ffn_infer(v['x'] if x is None else x, v['gamma'], v['beta'], SW.EPS, v['w1'], v['b1'], v['w2'], v['b2'], mdt)
    _sync()
    return out


def _err(got, ref64):
    return float((got.detach().cpu().double() - ref64).abs().max())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _recorder(monkeypatch):
    """The names that reach dhd_amd._lib.check: every entry point that returns a code goes through it."""
    from dhd_amd import _ffn, _ffn_wide, _lib
    _ffn.load()
    _ffn_wide.load()
    seen, real = [], _lib.check

    def check(rc, what):
        seen.append(what)
        return real(rc, what)
    monkeypatch.setattr(_lib, 'check', check)
    return seen


def _route(monkeypatch, wide=True):
    """Both routing tables as if every entry had won its measurement (or the wide one as if none had): these tests are about the
    route, not about which sizes take it."""
    from dhd_amd import swin_ffn
    monkeypatch.setattr(swin_ffn, 'ROUTED', {k: True for k in swin_ffn.ROUTED})
    monkeypatch.setattr(swin_ffn, 'ROUTED_WIDE', {k: wide for k in swin_ffn.ROUTED_WIDE})


# ------------------------------------------------------------------------------------------------ 1. against the twin

@pytest.mark.parametrize('case,prec', GRID)
def test_operator_against_the_float64_twin(gpu, case, prec):
    v, (xdt, mdt) = _on(gpu, case, prec), SW.PRECISIONS[prec]
    out = _run(v, mdt)
    ref = SW.twin(case, prec)
    assert tuple(out.shape) == tuple(ref.shape) and out.dtype == xdt and out.data_ptr() != v['x'].data_ptr()
    err, scale = _err(out, ref), SW.scale_of(ref)
    if mdt == F32:
        print(f'{case} [{prec}]: max |out - twin| = {err:.3e}, bound {BAR * scale:.3e}')
        assert err <= BAR * scale
    else:
        par = SW.parent(v, xdt, mdt, 'cuda')
        _sync()
        perr = _err(par, ref)
        print(f'{case} [{prec}]: max |out - twin| = {err:.3e}, parent {perr:.3e}, ratio {err / perr:.3f} (bound {MARGIN})')
        assert par.dtype == xdt and perr > 0
        assert err <= MARGIN * perr


# ------------------------------------------------------------------------------------------------ 2. rows, repeatability

@pytest.mark.parametrize('case,prec', [('r129_c512_ln', 'f32_bf16'), ('r200_c512_ln', 'f32'), ('r200_c1024_plain', 'f32_f16'),
                                       ('r129_c1024_ln', 'bf16'), ('r65_c1024_ln', 'f32')])
def test_rows_are_independent_and_calls_repeat(gpu, case, prec):
    v, (xdt, mdt) = _on(gpu, case, prec), SW.PRECISIONS[prec]
    rows = v['x'].shape[0]
    base = _run(v, mdt)
    assert _same(_run(v, mdt), base)                                          # two calls, the same bytes
    gen = torch.Generator().manual_seed(11)
    # both ends of a wave's LayerNorm rows (8, 16 or 24), of an MFMA row tile (32), of a workgroup tile (32, 64 or 96), the last row
    for keep in sorted(k for k in {0, 7, 8, 15, 16, 23, 24, 31, 32, 63, 64, 95, 96, rows - 1} if k < rows):
        x = (torch.randn(v['x'].shape, generator=gen) * 50).to(xdt).to(gpu)
        x[(keep + 1) % rows, 3] = float('inf')
        x[(keep + 2) % rows, ::2] = float('-inf')
        x[(keep + 3) % rows, 5] = float('nan')
        x[(keep + 4) % rows] = float('nan')                                   # a whole row of NaN next door, in the same tile or the next
        x[(keep - 1) % rows] = float('nan')
        x[keep] = v['x'][keep]
        got = _run(v, mdt, x)
        assert _same(got[keep], base[keep]), keep
    # a NaN row poisons itself and nothing else
    x = v['x'].clone()
    x[40, 7] = float('nan')
    got = _run(v, mdt, x)
    others = torch.arange(rows, device=gpu) != 40
    assert _same(got[others], base[others]) and bool(torch.isnan(got[40]).all())
    # a single row of the call is the row alone
    alone = _run(v, mdt, v['x'][50:51].clone())
    assert _same(alone[0], base[50])


# ------------------------------------------------------------------------------------------------ 3. guard bands

GUARDED = [pytest.param(f'r{r}_c{c}_ln', p, id=f'r{r}_c{c}-{p}') for r, c, p in
           ((1, 512, 'f32_bf16'), (33, 512, 'f32'), (129, 512, 'bf16'), (200, 512, 'f32_f16'), (63, 512, 'f16'),
            (1, 1024, 'f32'), (31, 1024, 'f16'), (65, 1024, 'f32_bf16'), (200, 1024, 'f32'), (129, 1024, 'bf16'))]


@pytest.mark.parametrize('case,prec', GUARDED)
def test_inside_guard_bands(gpu, monkeypatch, case, prec):
    """Plain, then with the two buffers the wrapper allocates (out, scratch) between two 4096-byte guard bands at their exact sizes,
    every byte 0xFF, then 0x00: no guard byte changes, the three runs agree (every element of out is written, nothing
    uninitialised is used: 0xFF is NaN in every float type), and the inputs are what they were."""
    from dhd_amd import _ffn_wide, _lib
    v, (xdt, mdt) = _on(gpu, case, prec), SW.PRECISIONS[prec]
    rows, c = v['x'].shape
    snap = {k: t.clone() for k, t in v.items() if t is not None}
    plain = _run(v, mdt)
    need = _ffn_wide.value('dhdg_swin_ffn_wide_scratch_bytes', c, 4 * c, _lib.DTYPE_CODE[mdt])
    for fill in (0xFF, 0x00):
        with G.guarded(monkeypatch, fill) as ledger:
            got = _run(v, mdt)
            ledger.check()
            got = got.detach().clone()
        ours = [e for e in ledger.sites_under(G.PRODUCT_ROOT) if 'swin_ffn.py' in e.site]
        print(f'{case} [{prec}, fill {fill:#04x}]: {len(ledger)} guarded allocations, {ledger.total_bytes()} bytes, guards intact')
        assert len(ours) == len(ledger) == 2 and sorted(e.nbytes for e in ours) == sorted((rows * c * v['x'].element_size(), need))
        assert bool(torch.isfinite(got).all()) and _same(got, plain), fill
    for k, s in snap.items():
        assert _same(v[k], s), f'input {k} changed'


# ------------------------------------------------------------------------------------------------ 4. views

@pytest.mark.parametrize('kind', ('strided_tokens', 'offset_4_bytes', 'channel_slice', 'batched'))
def test_views_give_the_dense_calls_bytes(gpu, kind):
    case, prec = 'r129_c512_ln', 'f32_bf16'
    v, (xdt, mdt) = _on(gpu, case, prec), SW.PRECISIONS[prec]
    x = v['x']
    rows, c = x.shape
    dense = _run(v, mdt)
    if kind == 'strided_tokens':
        parent = torch.full((2 * rows, c), float('nan'), device=gpu)
        parent[::2] = x
        view = parent[::2]
    elif kind == 'offset_4_bytes':
        parent = torch.full((rows * c + 1,), float('nan'), device=gpu)
        parent[1:] = x.reshape(-1)
        view = parent[1:].view(rows, c)
        assert view.data_ptr() % 16 == 4
    elif kind == 'channel_slice':
        parent = torch.full((rows, c + 32), float('nan'), device=gpu)
        parent[:, 8:8 + c] = x
        view = parent[:, 8:8 + c]
    else:
        parent = x.clone()
        view = parent.view(3, 43, c)                                         # (..., C): the result has the view's shape
    before = parent.clone()
    assert kind == 'batched' or not (view.is_contiguous() and view.data_ptr() % 16 == 0)
    got = _run(v, mdt, view)
    assert got.shape == view.shape and got.is_contiguous() and _same(got.reshape(rows, c), dense)
    assert _same(parent.nan_to_num(7.0), before.nan_to_num(7.0))             # the view was only read


# ------------------------------------------------------------------------------------------------ 5. the route

HW = (8, 12)


def _block(gpu, shift, c=512, heads=16):
    from dhd_amd.swin import SwinBlock
    torch.manual_seed(41 + int(shift))
    block = SwinBlock(c, heads, 4 * c, window_size=4, shift=shift).eval()
    with torch.no_grad():                                                     # parameters that are not at their initial values
        for n in (block.norm1, block.norm2):
            n.weight.add_(0.2 * torch.randn(c))
            n.bias.add_(0.1 * torch.randn(c))
        block.attn.w_msa.relative_position_bias_table.normal_(0, 0.5)
        for lin in (block.ffn.layers[0][0], block.ffn.layers[1]):
            lin.bias.normal_(0, 0.1)
    x = torch.randn(2, HW[0] * HW[1], c, generator=torch.Generator().manual_seed(42)) * 1.5
    block.fused_glue = False                                                  # whatever the environment says: norm2 runs as a module
    return block.to(gpu), x.to(gpu)


def _second_half64(block, mid):
    """The block's second half in float64 on the tokens `mid` the first half produced: x + ffn(norm2(x))."""
    b = copy.deepcopy(block).double().cpu()
    m = mid.detach().cpu().double()
    with torch.no_grad():
        return b.ffn(b.norm2(m), identity=m)


@pytest.mark.parametrize('shift', (False, True), ids=('plain', 'shifted'))
@pytest.mark.parametrize('mode', ('f32', 'bf16_autocast'))
def test_swin_block_takes_the_route(gpu, monkeypatch, shift, mode):
    """SwinBlock(512, 16, 2048, window_size=4) on 2 images of 8 x 12 tokens, eval + no_grad, both tables all-True.  The first half of
    the block is the same code with the switch on and off; the tokens that enter the second half are taken from a hook on norm2
    in the switch-off run, and the second half of both runs is held against a float64 run of it on those tokens."""
    import dhd_amd
    _route(monkeypatch)
    block, x = _block(gpu, shift)
    auto = mode.startswith('bf16')
    seen = _recorder(monkeypatch)
    mids = []
    hook = block.norm2.register_forward_hook(lambda mod, args, out: mids.append(args[0].detach().clone()))
    outs = {}
    for on in (False, True):
        dhd_amd.fused_swin_ffn(block, on)
        del seen[:], mids[:]
        with torch.no_grad(), torch.autocast('cuda', dtype=BF16, enabled=auto):
            outs[on] = block(x, HW)
        _sync()
        assert seen.count(WIDE) == int(on) and NARROW not in seen, (on, seen)
        assert len(mids) == int(not on)                                       # norm2 as a module ran on today's path only
        assert outs[on].dtype == F32 and outs[on].shape == x.shape
        if not on:
            mid = mids[0]
    hook.remove()
    ref = _second_half64(block, mid)
    e_on, e_off, scale = _err(outs[True], ref), _err(outs[False], ref), SW.scale_of(ref)
    print(f'block [{mode}, shift {shift}]: fused {e_on:.3e}, today {e_off:.3e}, scale {scale:.2f}')
    if auto:
        assert e_on <= MARGIN * e_off
    else:
        assert e_on <= BAR * scale
    # with ROUTED_WIDE all-False the switch changes nothing: today's bytes, no operator
    _route(monkeypatch, wide=False)
    del seen[:]
    with torch.no_grad(), torch.autocast('cuda', dtype=BF16, enabled=auto):
        unrouted = block(x, HW)
    _sync()
    assert block.fused_ffn is True and WIDE not in seen and NARROW not in seen and _same(unrouted, outs[False])


def test_a_narrow_block_still_reaches_the_narrow_family(gpu, monkeypatch):
    import dhd_amd
    _route(monkeypatch)
    block, x = _block(gpu, False, c=128, heads=4)
    dhd_amd.fused_swin_ffn(block)
    seen = _recorder(monkeypatch)
    with torch.no_grad():
        block(x, HW)
    _sync()
    assert seen.count(NARROW) == 1 and WIDE not in seen


# ------------------------------------------------------------------------------------------------ 6. graph capture

def test_graph_capture(gpu):
    """Captured on a single stream (no branches), replayed twice -- the second time on other inputs copied into place."""
    case, prec = 'r200_c512_ln', 'f32_bf16'
    v, (xdt, mdt) = _on(gpu, case, prec), SW.PRECISIONS[prec]
    arg, other = v['x'].clone(), v['x'].flip(0).contiguous()
    with torch.no_grad():
        ref1, ref2 = _run(v, mdt, arg).clone(), _run(v, mdt, other).clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            _run(v, mdt, arg)
        torch.cuda.current_stream().wait_stream(s)
        _sync()
        from dhd_amd import swin_ffn_infer
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = swin_ffn_infer(arg, v['gamma'], v['beta'], SW.EPS, v['w1'], v['b1'], v['w2'], v['b2'], mdt)
        graph.replay()
        _sync()
        assert _same(cap, ref1)
        arg.copy_(other)
        graph.replay()
        _sync()
        assert _same(cap, ref2) and not _same(ref1, ref2)


# ------------------------------------------------------------------------------------------------ 7. peak allocation

def _peak(fn):
    """Peak bytes a warmed call holds on top of what was allocated before it (its result included)."""
    fn()
    _sync()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    _sync()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def test_peak_allocation(gpu):
    """2048 x 512 tokens under bf16 autocast: the fused call holds its result and its scratch; the parent holds the hidden tensor
    twice (fc1's output and GELU's) at its peak."""
    from dhd_amd import _ffn_wide
    rows, c = 2048, 512
    gen = torch.Generator().manual_seed(31)
    v = dict(x=torch.randn(rows, c, generator=gen), gamma=1 + 0.2 * torch.randn(c, generator=gen), beta=0.1 * torch.randn(c, generator=gen),
             w1=torch.randn(4 * c, c, generator=gen) / c ** 0.5, b1=0.1 * torch.randn(4 * c, generator=gen),
             w2=torch.randn(c, 4 * c, generator=gen) / (4 * c) ** 0.5, b2=0.1 * torch.randn(c, generator=gen))
    v = {k: t.to(gpu) for k, t in v.items()}
    out_bytes, hidden_bytes = rows * c * 4, rows * 4 * c * 2
    scratch = _ffn_wide.value('dhdg_swin_ffn_wide_scratch_bytes', c, 4 * c, 2)
    with torch.no_grad():
        fused = _peak(lambda: _run(v, BF16))
        parent = _peak(lambda: SW.parent(v, F32, BF16, 'cuda'))
    print(f'peak above resident: fused {fused} bytes (out {out_bytes} + scratch {scratch}), parent {parent} bytes (hidden tensor {hidden_bytes})')
    assert fused <= out_bytes + scratch + (1 << 20)
    assert parent >= 2 * hidden_bytes
