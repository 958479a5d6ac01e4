"""The normalisation kernels on offset, outlier and constant data, against float64 (inputs, references and the bound rule:
norm_edge_inputs.py; that the inputs are what their names say: test_norm_edge_inputs.py).

  csrc/batchnorm.hip     training BatchNorm, NCHW and channels_last (+ ReLU / residual epilogues), through
                         dhd_amd.batchnorm.BatchNorm2d and once more through the C ABI
  csrc/swin_glue.hip     layer_norm_rows, norm into windows
  csrc/swin_seam.h       patch_merge_norm, patch_embed_norm
  csrc/swin_ffn.hip      the inline norm2 of swin_ffn_infer and swin_ffn (training), C = 128 and the wide family at C = 512

Errors are max |t - t64| / max(1, max |t64|) per tensor and per channel (BatchNorm) or per row regime (LayerNorm).  The bound is
the bar the operator already has where the float32 torch formulation, run here on the same device on the same stored values, is
within that bar of float64, else 4 x that formulation's own error (value_edge_inputs.bound).  Every case prints the kernel's
error, the mirror's error and the bound per regime before it asserts."""
import pytest
import torch
import torch.nn.functional as F

import norm_edge_inputs as N

pytestmark = pytest.mark.gpu

NAN = float('nan')


def _bound(bar, mirror_err):
    """value_edge_inputs.bound, element-wise on tensors."""
    out = torch.empty_like(mirror_err)
    for i in range(mirror_err.numel()):
        out.view(-1)[i] = N.bound(float(bar.view(-1)[i]) if torch.is_tensor(bar) else bar, float(mirror_err.view(-1)[i]))
    return out


class _Report:
    """Collects (tensor, regime, kernel error, mirror error, bound) of every channel, prints the worst channel of each regime and
    fails at the end if any channel was out of its bound."""

    def __init__(self, title, regimes):
        self.title, self.regimes, self.rows, self.bad = title, regimes, [], []

    def add(self, name, err, mirror, bnd):
        for r in dict.fromkeys(self.regimes):
            sel = [i for i, q in enumerate(self.regimes) if q == r]
            i = max(sel, key=lambda j: float(err[j]) / float(bnd[j]) if float(err[j]) == float(err[j]) else float('inf'))
            self.rows.append((name, r, float(err[i]), float(mirror[i]), float(bnd[i])))
        ok = err <= bnd
        for i in (~ok).nonzero().view(-1).tolist():
            self.bad.append((name, self.regimes[i], i, float(err[i]), float(mirror[i]), float(bnd[i])))

    def finish(self):
        print(self.title)
        for name, r, e, m, b in self.rows:
            print(f'  {name:13s} {r:20s} kernel {e:9.3g}  mirror {m:9.3g}  bound {b:9.3g}{"   <-- OUT" if not e <= b else ""}')
        assert not self.bad, f'{self.title}: out of bound (tensor, regime, channel, kernel, mirror, bound): {self.bad}'


# --------------------------------------------------------------------------- A. BatchNorm

def _lay(t, layout, gpu):
    t = t.to(gpu)
    return t.contiguous(memory_format=torch.channels_last) if layout == 'nhwc' else t.contiguous()


def _module_steps(gpu, layout, shape, dt, mode, all_plain=False):
    """Two training steps of BatchNorm2d (routing forced to the HIP operator), the second with momentum=None -> per step a dict
    of y, gx, gres, dgamma, dbeta, running_mean, running_var (clones) and num_batches_tracked."""
    from dhd_amd.batchnorm import BatchNorm2d
    AlwaysHip = type('AlwaysHipBN', (BatchNorm2d,), dict(_routing=(0, 1 << 30, 0)))   # no size threshold
    v = N.bn_case(layout, shape, dt, all_plain)
    c = shape[1]
    bn = AlwaysHip(c, momentum=0.1).to(gpu).train()
    with torch.no_grad():
        bn.weight.copy_(v['gamma']); bn.bias.copy_(v['beta'])
        bn.running_mean.copy_(v['running_mean']); bn.running_var.copy_(v['running_var'])
    steps = []
    for step in range(2):
        if step == 1:
            bn.momentum = None                      # cumulative average: factor = 1 / num_batches_tracked = 1 / 2
        x = _lay(v['x'], layout, gpu).requires_grad_()
        res = _lay(v['res'], layout, gpu).requires_grad_() if mode == 'add' else None
        g = _lay(v['g'], layout, gpu)
        assert bn._nhwc_ok(x) if layout == 'nhwc' else bn._hip_ok(x)
        y = bn(x, relu=mode == 'relu', residual=res)
        assert y.dtype == x.dtype and y.stride() == x.stride()
        y.backward(g)
        steps.append(dict(y=y.detach(), gx=x.grad, gres=res.grad if res is not None else None, dgamma=bn.weight.grad.clone(),
                          dbeta=bn.bias.grad.clone(), running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
                          tracked=int(bn.num_batches_tracked)))
        bn.zero_grad()
    return steps


def _capi_step(gpu, layout, shape, dt, mode, factor):
    """One forward + backward through the C ABI on buffers the test owns: outputs pre-filled with NaN, the workspace with 0xCD,
    every input compared with its clone afterwards."""
    from dhd_amd import _lib
    lib = _lib.load()
    v = N.bn_case(layout, shape, dt)
    n, c, h, w = shape
    x, g = _lay(v['x'], layout, gpu), _lay(v['g'], layout, gpu)
    res = _lay(v['res'], layout, gpu) if mode == 'add' else None
    gamma, beta = v['gamma'].to(gpu), v['beta'].to(gpu)
    rm, rv = v['running_mean'].to(gpu), v['running_var'].to(gpu)
    nan_like = lambda t: torch.full_like(t, NAN)
    nan_c = lambda k=1: torch.full((k * c,), NAN, dtype=torch.float32, device=gpu)
    y, gx, gres = nan_like(x), nan_like(x), nan_like(x) if mode == 'add' else None
    mean, rstd, affine, dgamma, dbeta = nan_c(), nan_c(), nan_c(2), nan_c(), nan_c()
    code, st = _lib.dtype_code(x.dtype), _lib.stream_ptr(gpu)
    clones = [t.clone() for t in (x, g, gamma, beta)] + ([res.clone()] if res is not None else [])
    with torch.cuda.device(gpu):
        if layout == 'nchw':
            ws = torch.full((lib.dhd_bn_workspace_bytes(n, c, h * w),), 0xCD, dtype=torch.uint8, device=gpu)
            _lib.check(lib.dhd_bn_train_forward(_lib.ptr(x), code, n, c, h * w, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(rm), _lib.ptr(rv),
                                                factor, N.EPS, _lib.ptr(y), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(ws), st),
                       'dhd_bn_train_forward')
            ws.fill_(0xCD)
            _lib.check(lib.dhd_bn_train_backward(_lib.ptr(x), _lib.ptr(g), code, n, c, h * w, _lib.ptr(gamma), _lib.ptr(mean), _lib.ptr(rstd),
                                                 _lib.ptr(gx), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(ws), st), 'dhd_bn_train_backward')
        else:
            rows, flags = n * h * w, {'plain': 0, 'relu': 1, 'add': 2}[mode]
            ws = torch.full((lib.dhd_bn_nhwc_workspace_bytes(rows, c),), 0xCD, dtype=torch.uint8, device=gpu)
            _lib.check(lib.dhd_bn_nhwc_train_forward(_lib.ptr(x), _lib.ptr(res), code, rows, c, flags, _lib.ptr(gamma), _lib.ptr(beta),
                                                     _lib.ptr(rm), _lib.ptr(rv), factor, N.EPS, _lib.ptr(y), _lib.ptr(mean), _lib.ptr(rstd),
                                                     _lib.ptr(affine), _lib.ptr(ws), st), 'dhd_bn_nhwc_train_forward')
            ws.fill_(0xCD)
            _lib.check(lib.dhd_bn_nhwc_train_backward(_lib.ptr(x), _lib.ptr(y), _lib.ptr(g), code, rows, c, flags, _lib.ptr(gamma),
                                                      _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(affine), _lib.ptr(gx), _lib.ptr(gres),
                                                      _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(ws), st), 'dhd_bn_nhwc_train_backward')
    torch.cuda.synchronize()
    for t, cl in zip([x, g, gamma, beta] + ([res] if res is not None else []), clones):
        bits = torch.int32 if t.dtype == torch.float32 else torch.int16
        assert torch.equal(t.view(bits), cl.view(bits)), 'an input was written'
    return dict(y=y, gx=gx, gres=gres, dgamma=dgamma, dbeta=dbeta, running_mean=rm, running_var=rv, save_mean=mean, save_rstd=rstd)


def _check_steps(gpu, title, layout, shape, dt, mode, steps, factors):
    """Every tensor of every step, per channel, within bound(bar, mirror error) of float64."""
    v = N.bn_case(layout, shape, dt)
    bar = N.BN_BARS[dt]
    pbar = bar * (1 if dt == 'f32' else 4)
    rep = _Report(title, v['regimes'])
    x, g = _lay(v['x'], layout, gpu), _lay(v['g'], layout, gpu)
    res = _lay(v['res'], layout, gpu) if mode == 'add' else None
    gamma, beta = v['gamma'].to(gpu), v['beta'].to(gpu)
    rm32, rv32 = v['running_mean'].to(gpu), v['running_var'].to(gpu)
    rm64, rv64 = v['running_mean'].double(), v['running_var'].double()
    for k, (out, factor) in enumerate(zip(steps, factors)):
        tag = f'step{k} '
        mask = out['y'].float() > 0 if mode != 'plain' else None
        ref = N.bn_reference(layout, shape, dt, mode, None if mask is None else mask.cpu())
        mir = N.bn_mirror(x, g, res, gamma, beta, rm32, rv32, factor, mode, mask)
        rm32, rv32 = mir['running_mean'], mir['running_var']
        rm64, rv64 = N.running64(rm64, rv64, ref['mean'], ref['var'], ref['cnt'], factor)
        assert bool(torch.isfinite(out['y'].float()).all()) and bool(torch.isfinite(out['gx'].float()).all())
        for name in ('y', 'gx') + (('gres',) if mode == 'add' else ()):
            m = N.channel_err(mir[name], ref[name])
            bnd = _bound(bar, m)
            rep.add(tag + name, N.channel_err(out[name], ref[name]), m, bnd)
            if name == 'y' and mode != 'plain':
                # the sign of a pre-activation within 2 x bound x scale of zero is the operator's; everywhere else it is checked
                scale = ref['pre'].abs().amax((0, 2, 3)).clamp(min=1.0)
                sure = ref['pre'].abs() > (2 * bnd * scale).view(1, -1, 1, 1)
                assert bool((mask.cpu() == (ref['pre'] > 0))[sure].all()), 'ReLU mask differs where the sign is certain'
        for name in ('dgamma', 'dbeta'):
            e = lambda t: (t.double().cpu() - ref[name]).abs() / ref[name].abs().clamp(min=1.0)
            m = e(mir[name])
            rep.add(tag + name, e(out[name]), m, _bound(pbar, m))
        for name, r64, rtol in (('running_mean', rm64, 1e-5), ('running_var', rv64, 1e-4)):
            e = lambda t: (t.double().cpu() - r64).abs()
            tol = 1e-5 + rtol * r64.abs()                                 # allclose(atol=1e-5, rtol) of the existing tests
            m = e(mir[name])
            rep.add(tag + name, e(out[name]), m, _bound(tol, m))
        if 'tracked' in out:
            assert out['tracked'] == k + 1
        # a constant channel: exactly beta
        const = [i for i, r in enumerate(v['regimes']) if N.family(r) == 'constant']
        stored = N.DTYPES[dt]
        want = beta.view(1, -1, 1, 1).expand(shape)
        if mode == 'add':
            want = want + res.float()
        if mode != 'plain':
            want = want.clamp(min=0)
        exact = torch.equal(out['y'][:, const].float(), want.to(stored)[:, const].float())
        worst = float((out['y'][:, const].float() - want[:, const]).abs().max())
        print(f'  {tag}constant channels: y == beta{" (+ residual, ReLU)" if mode != "plain" else ""} exactly: {exact} (largest difference {worst:.3g})')
        if dt == 'f32' or mode != 'add':      # (a half sum beta + residual is rounded once by the kernel, twice here)
            rep.bad += [] if exact else [('y == beta on constant channels', 'constant', -1, worst, 0.0, 0.0)]
    rep.finish()


def _bn_modes(layout):
    return ('plain', 'relu', 'add') if layout == 'nhwc' else ('plain',)


BN_GRID = [(layout, shape, dt, mode) for layout, shape, dt in N.BN_CASES for mode in _bn_modes(layout)]
_bn_id = lambda p: '-'.join(['x'.join(map(str, q)) if isinstance(q, tuple) else str(q) for q in p])


@pytest.mark.parametrize('case', BN_GRID, ids=_bn_id)
def test_batchnorm_module_on_edge_channels_vs_float64(gpu, case):
    """BatchNorm2d, two steps (the second with momentum=None): y, gx, the residual gradient, dgamma, dbeta and both running
    statistics per channel within bound(bar, mirror error) of float64; num_batches_tracked; constant channels give y == beta
    exactly; the `plain` channels are bit-identical to those of an all-`plain` tensor (no channel leaks into another)."""
    layout, shape, dt, mode = case
    steps = _module_steps(gpu, layout, shape, dt, mode)
    _check_steps(gpu, f'BatchNorm2d {layout} {shape} {dt} {mode}', layout, shape, dt, mode, steps, (0.1, 0.5))
    plain = [i for i, r in enumerate(N.bn_case(layout, shape, dt)['regimes']) if r == 'plain']
    alone = _module_steps(gpu, layout, shape, dt, mode, all_plain=True)
    for a, b in zip(steps, alone):
        for name in ('y', 'gx') + (('gres',) if mode == 'add' else ()):
            assert torch.equal(a[name][:, plain], b[name][:, plain]), f'{name}: a plain channel depends on its neighbours'
        for name in ('dgamma', 'dbeta', 'running_mean', 'running_var'):
            assert torch.equal(a[name][plain], b[name][plain]), f'{name}: a plain channel depends on its neighbours'


@pytest.mark.parametrize('case', BN_GRID, ids=_bn_id)
def test_batchnorm_c_abi_on_edge_channels_vs_float64(gpu, case):
    """The same tensors through dhd_bn_train_forward / _backward and dhd_bn_nhwc_train_forward / _backward: every output element
    is written (they start as NaN: the checks against float64 would fail on one that was left), no input is, and the saved
    statistics are finite."""
    layout, shape, dt, mode = case
    out = _capi_step(gpu, layout, shape, dt, mode, 0.1)
    _check_steps(gpu, f'C ABI {layout} {shape} {dt} {mode}', layout, shape, dt, mode, [out], (0.1,))
    assert bool(torch.isfinite(out['save_mean']).all()) and bool(torch.isfinite(out['save_rstd']).all())


# --------------------------------------------------------------------------- B. LayerNorm

F32 = torch.float32


def _rule(bar, mirror):
    return {r: N.bound(bar, m) for r, m in mirror.items()}


def _ln_report(title, rows):
    """rows: (tensor, regime, kernel error, mirror error, bound).  Prints them all, then fails on the ones out of bound."""
    print(title)
    bad = []
    for name, r, e, m, b in rows:
        out = not e <= b
        print(f'  {name:7s} {r:20s} kernel {e:9.3g}  mirror {m:9.3g}  bound {b:9.3g}{"   <-- OUT" if out else ""}')
        if out:
            bad.append((name, r, e, m, b))
    assert not bad, f'{title}: out of bound (tensor, regime, kernel, mirror, bound): {bad}'


def _ln_check(title, d, op, mirror_op, rows_of, xdt, odt, gpu):
    """A LayerNorm operator `op(x, gamma, beta, out_dtype)` on the case d against its float64 twin, forward and backward, per row
    regime; `mirror_op(x, gamma, beta)` is the float32 torch formulation, `rows_of(t)` turns a tensor of x's shape into the rows
    that names_in names."""
    x, dy, gamma, beta = (d[k].to(gpu) for k in ('x', 'dy', 'gamma', 'beta'))
    rows = []
    # forward: the float32 result; a half result is that result rounded once
    y32 = op(x, gamma, beta, F32)
    torch.cuda.synchronize()
    assert y32.dtype == F32 and tuple(y32.shape) == tuple(d['Y'].shape)
    xm, gm, bm = x.float().clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    ym = mirror_op(xm, gm, bm)
    mdx, mdg, mdb = torch.autograd.grad(ym, (xm, gm, bm), dy.float())
    e, m = N.group_err(y32, d['Y'], d['names_out']), N.group_err(ym, d['Y'], d['names_out'])
    rows += [('y', r, e[r], m[r], N.bound(N.LN_BAR, m[r])) for r in e]
    if odt != F32:
        y = op(x, gamma, beta, odt)
        assert y.dtype == odt and torch.equal(y, y32.to(odt))
    # backward
    xl, gl, bl = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    op(xl, gl, bl, odt).backward(dy)
    torch.cuda.synchronize()
    assert xl.grad.dtype == xdt and xl.grad.shape == x.shape
    DXr, dxr, mdxr = rows_of(d['DX']), rows_of(xl.grad.double().cpu()), rows_of(mdx.double().cpu())
    e, m = N.group_err(dxr, DXr, d['names_in']), N.group_err(mdxr, DXr, d['names_in'])
    # dx in x's half type is the float32 result rounded once more: one unit roundoff of that type on top
    rows += [('dx', r, e[r], m[r], N.bound(N.LN_BAR, m[r]) + N.LN_UNIT[xdt]) for r in e]
    for name, got, mir, ref in (('dgamma', gl.grad, mdg, d['DG']), ('dbeta', bl.grad, mdb, d['DB'])):
        err = lambda t: float((t.double().cpu() - ref).abs().max() / max(1.0, float(ref.abs().max())))
        rows.append((name, 'all rows', err(got), err(mir), N.bound(N.LN_BAR, err(mir))))
    assert bool(torch.isfinite(y32).all()) and bool(torch.isfinite(xl.grad.float()).all())
    _ln_report(title, rows)


@pytest.mark.parametrize('prec', N.GLUE_PRECISIONS)
@pytest.mark.parametrize('case', N.GLUE_CASES)
def test_layer_norm_rows_on_edge_rows_vs_float64(gpu, case, prec):
    """layer_norm_rows (plain and into windows), forward and backward, every row regime within bound(1e-4, mirror error) of the
    module's float64 twin."""
    import swin_glue_inputs as SG
    from dhd_amd import layer_norm_rows
    d = N.glue_case(case, prec)
    xdt, odt = SG.PRECISIONS[prec]
    win = SG.window_arg(case)
    _ln_check(f'layer_norm_rows {case} [{prec}]', d, lambda x, g, b, o: layer_norm_rows(x, g, b, SG.EPS, o, win),
              lambda x, g, b: SG.ln_rows64(x, g, b, case), lambda t: t, xdt, odt, gpu)


@pytest.mark.parametrize('prec', N.SEAM_PRECISIONS)
@pytest.mark.parametrize('kind,case,batch', N.SEAM_CASES)
def test_seam_norms_on_edge_rows_vs_float64(gpu, kind, case, batch, prec):
    """patch_merge_norm (the norm over 4C) and patch_embed_norm with the regimes in the rows they normalise."""
    import dhd_amd
    import swin_seam_inputs as SS
    d = N.seam_case(kind, case, batch, prec)
    xdt, odt = SS.precisions(kind)[prec]
    if kind == 'merge':
        _, H, W, _ = SS.MERGE_CASES[case]
        op = lambda x, g, b, o: dhd_amd.patch_merge_norm(x, g, b, SS.EPS, (H, W), o)
    else:
        op = lambda x, g, b, o: dhd_amd.patch_embed_norm(x, g, b, SS.EPS, o)
    _ln_check(f'patch_{kind}_norm {case} x{batch} [{prec}]', d, op, lambda x, g, b: SS.call64(kind, case, x, g, b),
              lambda t: N.seam_rows(kind, t, case), xdt, odt, gpu)


@pytest.mark.parametrize('prec', N.FFN_PRECISIONS)
@pytest.mark.parametrize('family', [f for f, _, _ in N.FFN_CASES])
def test_swin_ffn_on_edge_rows_vs_float64(gpu, family, prec):
    """The four FFN families (inline norm2): 'f32' within bound(1e-4, the parent formulation's error) of the module's float64
    twin, 'bf16' within 1.5 x the parent's own error -- the modules' bounds -- per row regime for out and dx, per tensor for the
    parameter gradients."""
    import dhd_amd
    d = N.ffn_case(family, prec)
    M, xdt, mdt = d['module'], d['xdt'], d['mdt']
    v = {k: (None if t is None else t.to(gpu)) for k, t in d['v'].items()}
    train = family.startswith('train')
    if train:
        leaves = {k: v[k].detach().clone().requires_grad_() for k in ('x',) + M.PARAMS}
        out = dhd_amd.swin_ffn(leaves['x'], leaves['gamma'], leaves['beta'], M.EPS, leaves['w1'], leaves['b1'], leaves['w2'], leaves['b2'], mdt, None)
        out.backward(v['dout'])
        got = M._collect(out, leaves)
        par = M.parent(v, xdt, mdt, None, 'cuda')
    else:
        got = {'out': dhd_amd.swin_ffn_infer(v['x'], v['gamma'], v['beta'], M.EPS, v['w1'], v['b1'], v['w2'], v['b2'], mdt)}
        par = {'out': M.parent(v, xdt, mdt, 'cuda')}
    torch.cuda.synchronize()
    limit = (lambda m: N.bound(N.LN_BAR, m)) if mdt == F32 else (lambda m: N.bound(N.FFN_MARGIN * m, m))
    rows = []
    for k in (N.FFN_TENSORS if train else ('out',)):
        ref = d['ref'][k]
        assert got[k].dtype == par[k].dtype and tuple(got[k].shape) == tuple(ref.shape) and bool(torch.isfinite(got[k].float()).all()), k
        if k in ('out', 'dx'):
            e, m = N.group_err(got[k], ref, d['names']), N.group_err(par[k], ref, d['names'])
            rows += [(k, r, e[r], m[r], limit(m[r])) for r in e]
        else:
            err = lambda t: float((t.double().cpu() - ref).abs().max() / max(1.0, float(ref.abs().max())))
            rows.append((k, 'all rows', err(got[k]), err(par[k]), limit(err(par[k]))))
    _ln_report(f'swin_ffn {family} [{prec}]', rows)
