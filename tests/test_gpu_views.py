"""Every HIP operator on strided, offset and misaligned views of its inputs and of the gradients it is handed back.

The parity tests feed the operators freshly allocated dense tensors.  A model that slices, concatenates, permutes or expands
around them hands over views: a dense tensor at an odd storage offset (2 or 4 bytes off a 16-byte boundary), a channel slice,
a strided or channels_last tensor, and -- from `.sum().backward()` -- a gradient whose strides are all zero.  DESIGN.md
("Views: what each operator does with a tensor that is not dense and aligned") says what each operator does with those;
ROWS below is the checkable form of that table.

present(values, kind) carves a tensor equal to `values` out of a larger buffer filled with poison (all-ones bytes: NaN in every
float type, -1 / 255 in the integer types) with at least 64 bytes of poison on either side, so that a wrapper which ignores
strides or offset reads poison -- inside the allocation -- and a kernel that writes outside the view changes a poison byte.
A gradient is presented by an identity autograd node on the operator's output whose backward returns present(g, kind).

One case = one operator, one tensor presented in one layout, everything else fresh.  It asserts
  1. the same outputs, gradients and updated buffers as with fresh tensors: torch.equal where the wrapper copies the view and
     the same deterministic kernels run, the tolerance of the operator's existing parity test where it documents another path
     (each row names that test in `src`);
  2. every byte of every parent buffer, values and poison, is what it was; gradients have the shape and dtype of the input as
     presented;
  3. the C entry points that were called (the names that reach dhd_amd._lib.check, and every call through the library
     handle) are the ones the row expects: all of `entries` for fresh tensors, and the row's `path` for the view.
"""
import collections
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import small_dhds_cfg  # noqa: E402

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
CL = torch.channels_last
PAD = 64   # bytes of poison on either side of every view

DENSE = ('offset16', 'offset_elem', 'channel_slice', 'inner_step2')
NHWC = ('nhwc', 'nhwc_offset_elem')
FLAT = ('offset16', 'offset_elem', 'inner_step2')            # 1-D tensors
GRAD = DENSE + ('expanded',)


# --------------------------------------------------------------------------------------------- presenting a tensor

def _strides(shape, fmt=None):
    return torch.empty(shape, device='meta').stride() if fmt is None else torch.empty(shape, device='meta', memory_format=fmt).stride()


def present(values, kind):
    """-> (tensor equal to `values` laid out as `kind`, parent buffer or None for 'fresh')."""
    v = values.detach()
    if kind == 'fresh':
        return v.clone(), None
    es, shape = v.element_size(), tuple(v.shape)
    pad = PAD // es
    if kind in ('offset16', 'offset_elem'):
        strides, start, span = _strides(shape), pad + (kind == 'offset_elem'), v.numel()
    elif kind in ('nhwc', 'nhwc_offset_elem'):
        strides, start, span = _strides(shape, CL), pad + (kind == 'nhwc_offset_elem'), v.numel()
    elif kind == 'channel_slice':            # parent[:, 3:3 + C] of an (N, C + 5, ...) parent
        parent = (shape[0], shape[1] + 5) + shape[2:]
        strides = _strides(parent)
        start, span = pad + 3 * strides[1], int(np.prod(parent))
    elif kind == 'inner_step2':              # parent[..., ::2]
        parent = shape[:-1] + (2 * shape[-1],)
        strides = _strides(parent)[:-1] + (2,)
        start, span = pad, int(np.prod(parent))
    elif kind == 'expanded':                 # zero strides over a full-size parent: what sum().backward() hands over
        assert v.numel() > 0 and bool((v == v.reshape(-1)[0]).all()), 'expanded presents constant values only'
        strides, start, span = (0,) * v.dim(), pad, v.numel()
    else:
        raise KeyError(kind)
    buf = torch.empty(pad + 1 + span + pad, dtype=v.dtype, device=v.device)
    buf.view(torch.uint8).fill_(255)
    view = torch.as_strided(buf, shape, strides, start)
    if kind == 'expanded':
        buf[start] = v.reshape(-1)[0]
    else:
        view.copy_(v)
    lo, hi = buf.data_ptr(), buf.data_ptr() + buf.numel() * es
    assert view.data_ptr() - PAD >= lo and view.data_ptr() + v.numel() * es + PAD <= hi     # the parent-buffer rule
    if kind in ('offset16', 'offset_elem', 'nhwc', 'nhwc_offset_elem'):
        assert (view.data_ptr() % 16 != 0) == kind.endswith('offset_elem') and view.data_ptr() != buf.data_ptr()
    assert torch.equal(view, v) and view.dtype == v.dtype
    return view, buf


class _PresentGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, case):
        ctx.case = case
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        return ctx.case._present(g), None


class Case:
    """What a row's `run` uses to hand its tensors over: inp() for an input, grad() for the gradient of an output."""

    def __init__(self, target, kind):
        self.target, self.kind, self.parents, self.shown = target, kind, [], {}

    def _present(self, values):
        view, buf = present(values, self.kind)
        if buf is not None:
            self.parents.append((buf, buf.view(torch.uint8).clone()))
        return view

    def inp(self, name, values, grad=False):
        v = self._present(values) if name == self.target else values.detach().clone()
        self.shown[name] = v
        return v.requires_grad_() if grad else v

    def grad(self, name, y):
        return _PresentGrad.apply(y, self) if name == self.target else y

    def untouched(self):
        return all(torch.equal(buf.view(torch.uint8), snap) for buf, snap in self.parents)


def _record(monkeypatch):
    """The C entry points a run goes through: the `what` of every dhd_amd._lib.check and every call through the library handle
    (bev_pool_v2 only calls check on failure)."""
    from dhd_amd import _lib
    seen = []
    real_check, real_lib = _lib.check, _lib.load()

    def check(rc, what):
        seen.append(('check', what))
        return real_check(rc, what)

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real_lib, name)

            def call(*a):
                seen.append(('call', name))
                return fn(*a)
            return call
    monkeypatch.setattr(_lib, 'check', check)
    monkeypatch.setattr(_lib, '_lib', Spy())
    return seen


# --------------------------------------------------------------------------------------------- the table

class Row:
    """name; values(gpu) -> dict of plain tensors; run(case, values) -> dict of result tensors; present: target -> kinds;
    entries: C entry points a fresh run must go through (`watch`: further names whose call count is compared);
    path(target, kind) -> {entry: calls} where the view changes the fresh run's counts, else None;
    tol(target, kind) -> None (torch.equal with the fresh run) or the tolerance of `src`; close(key, got, ref, tol) the form of
    that test's assertion; ref64(values, got) -> the float64 torch formulation, compared where tol is not None;
    fresh_keys(target, kind) -> result keys compared with the fresh run (None = all); const: target -> value keys made constant
    for 'expanded'; raises(target, kind) -> the raw-layout helpers that refuse a view."""

    def __init__(self, name, values, run, present, entries, src='', watch=(), path=None, tol=None, close=None, ref64=None,
                 fresh_keys=None, const=None, raises=None):
        self.name, self.values, self.run, self.present, self.entries, self.src = name, values, run, present, tuple(entries), src
        self.watch = tuple(entries) + tuple(watch)
        self.path = path or (lambda t, k: None)
        self.tol = tol or (lambda t, k: None)
        self.close = close or _rel_close
        self.ref64, self.const = ref64, const or {}
        self.fresh_keys = fresh_keys or (lambda t, k: None)
        self.raises = raises or (lambda t, k: False)


def _rel_close(key, got, ref, tol):
    """|got - ref| <= tol * max(1, |ref|_max): the form of the BatchNorm, DCN and bev_pool parity assertions."""
    if got.numel() == 0:
        return True
    err = float((got.double() - ref.double()).abs().max())
    return err <= tol * max(1.0, float(ref.double().abs().max()))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, gpu, dtype=F32, scale=1.0, shift=0.0, fmt=None):
    t = (torch.randn(shape, generator=_gen(seed)) * scale + shift).to(gpu).to(dtype)
    return t if fmt is None else t.contiguous(memory_format=fmt)


ROWS = []


# ---- SFA stage (mix): training and inference, float32 and half storage ----------------------------------------------

def _sfa_row(dtype, train):
    b = 2 if dtype == F32 else 1                      # 2C = 256 input, 8x8; (128, 1, 8, 8) with half storage

    def values(gpu):
        return dict(x=_randn((b, 256, 8, 8), 11, gpu, dtype), g=_randn((b, 128, 8, 8), 12, gpu, dtype))

    def run(c, v):
        from dhd_amd.mix import channel_spatial_stage, fused_stage_supported, inference_selected
        torch.manual_seed(0)
        st = channel_spatial_stage(256)
        sp = st.spacial_leanring
        with torch.no_grad():
            for bn in (sp[1], sp[4]):
                bn.running_mean.uniform_(-0.2, 0.2)
                bn.running_var.uniform_(0.5, 1.5)
        st = st.to(v['x'].device).train(train)
        x = c.inp('x', v['x'], grad=train)
        assert fused_stage_supported(st, x)
        if not train:
            with torch.no_grad():
                assert inference_selected(st, x)
                return dict(y=st(x))
        y = st(x)
        c.grad('g', y).backward(v['g'])
        out = dict(y=y.detach(), gx=x.grad)
        out.update({'d_' + n: p.grad for n, p in st.named_parameters()})
        out.update({'buf_' + n: t for n, t in st.named_buffers()})
        return out

    tag = ('train' if train else 'infer') + ('_f32' if dtype == F32 else '_f16_half_storage')
    pres = dict(x=('fresh',) + DENSE + NHWC)
    if train:
        pres['g'] = GRAD + NHWC
    return Row('sfa_' + tag, values, run, pres,
               ('dhd_sfa_stage_forward', 'dhd_sfa_stage_backward') if train else ('dhd_sfa_stage_infer',),
               src='copy, same kernels: test_sfa_stage_is_bit_reproducible_and_precision_is_per_instance', const=dict(g=['g']))


ROWS += [_sfa_row(F32, True), _sfa_row(F16, True), _sfa_row(F32, False), _sfa_row(F16, False)]


def _sfa_generic_row():
    """C = 16: the fused stage does not exist, the section-3 kernels run around library convolutions (_AttentionStage)."""
    def values(gpu):
        return dict(x=_randn((2, 32, 5, 8), 13, gpu), g=_randn((2, 16, 5, 8), 14, gpu))

    def run(c, v):
        from dhd_amd.mix import channel_spatial_stage, fused_stage_supported
        torch.manual_seed(0)
        st = channel_spatial_stage(32).to(v['x'].device).train()
        x = c.inp('x', v['x'], grad=True)
        assert not fused_stage_supported(st, x)
        y = st(x)
        c.grad('g', y).backward(v['g'])
        out = dict(y=y.detach(), gx=x.grad)
        out.update({'d_' + n: p.grad for n, p in st.named_parameters()})
        return out

    def close(key, got, ref, tol_):      # test_sfa_vs_reference, the same stage: output 2e-5 / 1e-4, gradients 2e-4 (x max |ref|) / 1e-3
        a, b = got.cpu().numpy(), ref.cpu().numpy()
        if key == 'y':
            return bool(np.allclose(a, b, atol=2e-5, rtol=1e-4))
        return bool(np.allclose(a, b, atol=2e-4 * (1.0 if key == 'gx' else max(1.0, float(np.abs(b).max()))), rtol=1e-3))

    # the blend backward sums dL/da1 with float atomics (csrc/sfa.hip): two fresh runs differ in the last bits of every gradient,
    # so every case of this row compares at the bar of the stage's parity test
    return Row('sfa_generic_c16', values, run, dict(x=('fresh',) + DENSE, g=GRAD),
               ('dhd_sfa_channel_mean', 'dhd_sfa_blend1', 'dhd_sfa_blend2', 'dhd_sfa_blend2_backward', 'dhd_sfa_blend1_backward',
                'dhd_sfa_mean_backward'), tol=lambda t, k: 1.0, close=close, src='test_sfa_vs_reference', const=dict(g=['g']))


ROWS.append(_sfa_generic_row())


# ---- BatchNorm2d: NCHW kernels and channels_last kernels with the fused ReLU / residual -------------------------------

_BN_TOL = {F32: 2e-5, F16: 2e-3, BF16: 1.6e-2}    # test_batchnorm2d_training_vs_torch / _channels_last_fused_vs_torch


def _bn_params(bn, c):
    g = _gen(5)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.5)
        bn.running_mean.copy_(torch.randn(c, generator=g))
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return bn


def _bn_close(dtype, nhwc):
    def close(key, got, ref, tol):
        if key == 'rm':
            return torch.allclose(got.double(), ref.double(), atol=1e-5, rtol=1e-5)
        if key == 'rv':
            return torch.allclose(got.double(), ref.double(), atol=1e-5, rtol=1e-4)
        mult = {'gx': 2 if nhwc else 1, 'gw': 1 if dtype == F32 else 4, 'gb': 1 if dtype == F32 else 4}.get(key, 1)
        return _rel_close(key, got, ref, tol * mult)
    return close


def _bn_row(shape, dtype, nhwc, mode):
    n, ch, h, w = shape
    fmt = CL if nhwc else None

    def values(gpu):
        return dict(x=_randn(shape, 21, gpu, dtype, 1.7, 0.4, fmt), res=_randn(shape, 22, gpu, dtype, fmt=fmt),
                    g=_randn(shape, 23, gpu, dtype, fmt=fmt))

    def run(c, v):
        from dhd_amd.batchnorm import BatchNorm2d
        cls = BatchNorm2d if nhwc else type('AlwaysHipBN', (BatchNorm2d,), dict(_routing=(0, 1 << 30, 0)))   # no size threshold
        bn = _bn_params(cls(ch), ch).to(v['x'].device).train()
        x = c.inp('x', v['x'], grad=True)
        r = c.inp('res', v['res'], grad=True) if mode == 'add' else None
        y = bn(x, relu=mode == 'relu', residual=r)
        c.grad('g', y).backward(v['g'])
        out = dict(y=y.detach(), gx=x.grad, gw=bn.weight.grad, gb=bn.bias.grad, rm=bn.running_mean, rv=bn.running_var)
        if r is not None:
            out['gres'] = r.grad
        return out

    def ref64(v, got):
        """torch's BatchNorm2d + add + relu in float64 on the same (rounded) inputs; the ReLU takes the operator's own decision
        where the pre-activation is within rounding of zero, as test_batchnorm2d_channels_last_fused_vs_torch does."""
        bn = _bn_params(torch.nn.BatchNorm2d(ch), ch).double().to(v['x'].device).train()
        x = v['x'].double().requires_grad_()
        r = v['res'].double().requires_grad_() if mode == 'add' else None
        pre = bn(x) if r is None else bn(x) + r
        if mode == 'plain':
            y = pre
        else:
            mask = got['y'].double() > 0
            sure = pre.detach().abs() > 2 * _BN_TOL[dtype] * max(1.0, float(pre.detach().abs().max()))
            assert bool((mask == (pre.detach() > 0))[sure].all())
            y = pre * mask
        y.backward(v['g'].double())
        out = dict(y=y.detach(), gx=x.grad, gw=bn.weight.grad, gb=bn.bias.grad, rm=bn.running_mean, rv=bn.running_var)
        if r is not None:
            out['gres'] = r.grad
        return out

    fwd, bwd = ('dhd_bn_nhwc_train_forward', 'dhd_bn_nhwc_train_backward') if nhwc else ('dhd_bn_train_forward', 'dhd_bn_train_backward')
    # the documented torch path: a view of x that is not dense in the kernel's layout, or dense at an odd storage offset
    # (a channel slice of a ONE-image NCHW batch is dense, at a 16-byte aligned start here: the kernels take it)
    x_to_torch = (('offset_elem', 'inner_step2', 'nhwc_offset_elem') + (('channel_slice',) if n > 1 or nhwc else ())
                  + (('offset16',) if nhwc else ()))
    res_unfused = ('nhwc_offset_elem', 'channel_slice')      # channels_last: the residual is added by torch after the kernel

    def path(t, k):
        return {fwd: 0, bwd: 0} if t == 'x' and k in x_to_torch else None

    def tol(t, k):
        other = (t == 'x' and k in x_to_torch) or (nhwc and t == 'res' and k in res_unfused)
        return _BN_TOL[dtype] if other else None

    def fresh_keys(t, k):
        # with a ReLU behind another path, elements within rounding of zero may fall on either side: their gradients are
        # checked against the float64 formulation with the operator's own mask, the fresh run vouches for what does not depend on it
        return ('y', 'rm', 'rv') if tol(t, k) is not None and mode != 'plain' else None

    if nhwc:
        pres = dict(x=('fresh', 'nhwc', 'nhwc_offset_elem', 'channel_slice', 'offset16'))
        if mode == 'add':
            pres['res'] = ('nhwc',) + res_unfused
        pres['g'] = NHWC + GRAD
    else:
        pres = dict(x=('fresh',) + DENSE)
        if mode == 'add':
            pres['res'] = DENSE + NHWC      # added by torch after the kernel: any view
        else:
            pres['g'] = GRAD + NHWC         # (behind the torch tail of 'add' the operator never sees the caller's gradient)
    name = 'bn_%s_%s_%s_%s' % ('nhwc' if nhwc else 'nchw', 'x'.join(map(str, shape)), str(dtype)[6:], mode)
    return Row(name, values, run, pres, (fwd, bwd), path=path, tol=tol, close=_bn_close(dtype, nhwc), ref64=ref64, fresh_keys=fresh_keys,
               const=dict(g=['g']), src='test_batchnorm2d_channels_last_fused_vs_torch' if nhwc else 'test_batchnorm2d_training_vs_torch')


ROWS += [_bn_row((1, 5, 4, 4), F32, False, 'plain'), _bn_row((1, 5, 4, 4), F32, False, 'add'),
         _bn_row((24, 16, 8, 22), F16, False, 'plain'), _bn_row((24, 16, 8, 22), F16, False, 'add'),
         _bn_row((3, 8, 5, 7), F32, True, 'relu'), _bn_row((3, 8, 5, 7), F32, True, 'add'),
         _bn_row((2, 24, 6, 10), F16, True, 'relu'), _bn_row((2, 24, 6, 10), F16, True, 'add')]


# ---- detector.Upsample -----------------------------------------------------------------------------------------------

_UP_EPS = {F32: 2.0 ** -23, F16: 2.0 ** -10, BF16: 2.0 ** -7}     # test_bilinear_upsample_forward_backward_vs_float64


def _up_row(shape, size, dtype, nhwc):
    fmt = CL if nhwc else None

    def values(gpu):
        return dict(x=_randn(shape, 31, gpu, dtype, fmt=fmt), g=_randn(shape[:2] + size, 32, gpu, dtype, fmt=fmt))

    def run(c, v):
        from dhd_amd.detector import Upsample
        x = c.inp('x', v['x'], grad=True)
        y = Upsample(size=size, mode='bilinear', align_corners=True)(x)
        c.grad('g', y).backward(v['g'])
        return dict(y=y.detach(), gx=x.grad)

    def ref64(v, got):
        x = v['x'].double().requires_grad_()
        y = torch.nn.functional.interpolate(x, size=size, mode='bilinear', align_corners=True)
        y.backward(v['g'].double())
        return dict(y=y.detach(), gx=x.grad)

    def close(key, got, ref, tol):
        eps = _UP_EPS[dtype]
        d = (got.double() - ref.double()).abs()
        if key == 'y':
            return bool((d <= (0.5 * eps + 2e-5) * ref.double().abs().clamp_min(1.0) + 1e-30).all())
        return float(d.max()) <= (eps + 4e-5) * float(ref.double().abs().max())

    # every view is copied into the layout it is dense in (else NCHW) and the library's kernels run; a view that ends up in the
    # row's other layout runs the other layout's kernel, held to the parity test's bar against float64 and the fresh run
    other_kernel = NHWC if not nhwc else DENSE

    def tol(t, k):
        return 1.0 if t == 'x' and k in other_kernel else None

    pres = dict(x=('fresh',) + DENSE + NHWC, g=GRAD + NHWC)
    name = 'upsample_%s_%s_%s' % ('nhwc' if nhwc else 'nchw', 'x'.join(map(str, shape)), str(dtype)[6:])
    return Row(name, values, run, pres, ('dhd_upsample_bilinear_forward', 'dhd_upsample_bilinear_backward'), tol=tol,
               close=close, ref64=ref64, const=dict(g=['g']), src='test_bilinear_upsample_forward_backward_vs_float64')


ROWS += [_up_row((2, 8, 9, 13), (18, 26), F32, False), _up_row((3, 24, 1, 6), (4, 6), F16, False),
         _up_row((3, 24, 1, 6), (4, 6), F32, True), _up_row((2, 8, 9, 13), (18, 26), BF16, True)]


# ---- Swin window partition and reverse ---------------------------------------------------------------------------------

def _window_row(B, H, W, C, ws, sh, dtype, out_dtype):
    nh, nw = -(-H // ws), -(-W // ws)

    def values(gpu):
        return dict(x=_randn((B, H, W, C), 41, gpu, dtype), gw=_randn((B, nh * nw, ws * ws, C), 42, gpu, out_dtype),
                    w=_randn((B, nh * nw, ws * ws, C), 43, gpu, dtype), gy=_randn((B, H, W, C), 44, gpu, out_dtype))

    def run(c, v):
        from dhd_amd.swin import _WindowRows
        x, w = c.inp('x', v['x'], grad=True), c.inp('w', v['w'], grad=True)
        win = _WindowRows.apply(x, H, W, ws, sh, False, out_dtype)
        c.grad('gw', win).backward(v['gw'])
        y = _WindowRows.apply(w, H, W, ws, sh, True, out_dtype)
        c.grad('gy', y).backward(v['gy'])
        return dict(win=win.detach(), gx=x.grad, y=y.detach(), gw=w.grad)

    name = 'window_%s_%s_to_%s' % ('x'.join(map(str, (B, H, W, C, ws, sh))), str(dtype)[6:], str(out_dtype)[6:])
    return Row(name, values, run, dict(x=('fresh',) + DENSE, w=DENSE, gw=GRAD, gy=GRAD), ('dhd_window_rows',),
               const=dict(gw=['gw'], gy=['gy']), src='copy, same kernel: test_swin_window_rows_equal_pad_roll_partition')


ROWS += [_window_row(2, 14, 21, 32, 7, 3, F32, F32), _window_row(2, 14, 21, 32, 7, 3, F32, BF16), _window_row(1, 5, 9, 16, 4, 2, BF16, BF16)]


# ---- layout.to_layout, both directions ---------------------------------------------------------------------------------

def _layout_row(shape, dtype, to_cl):
    src_fmt, dst_fmt = (None, CL) if to_cl else (CL, None)

    def values(gpu):
        return dict(x=_randn(shape, 51, gpu, dtype, 100.0, fmt=src_fmt), g=_randn(shape, 52, gpu, dtype, fmt=dst_fmt))

    def run(c, v):
        from dhd_amd.layout import to_layout
        x = c.inp('x', v['x'], grad=True)
        y = to_layout(x, torch.channels_last if to_cl else torch.contiguous_format)
        assert y.is_contiguous(memory_format=torch.channels_last if to_cl else torch.contiguous_format)
        c.grad('g', y).backward(v['g'])
        return dict(y=y.detach(), gx=x.grad)

    src_dense = ('offset16',) if to_cl else ('nhwc',)             # dense in the source format and aligned: the kernel
    dst_dense = ('nhwc',) if to_cl else ('offset16',)

    def path(t, k):
        # fresh: one transpose forward, one backward.  A view that is not (dense in its format and aligned) takes torch's copy; a
        # gradient that already has the producer's layout is returned as it is
        if k == 'fresh' or (t == 'x' and k in src_dense) or (t == 'g' and k in dst_dense):
            return None
        if not to_cl and t == 'x' and k == 'channel_slice':    # its gradient is wanted in NCHW, which the incoming one already is
            return {'dhd_transpose_batched': 0}
        return {'dhd_transpose_batched': 1}

    if to_cl:
        pres = dict(x=('fresh',) + DENSE, g=NHWC + GRAD)
    else:
        pres = dict(x=('fresh',) + NHWC + ('channel_slice',), g=GRAD + NHWC)
    name = 'layout_%s_%s_%s' % ('to_nhwc' if to_cl else 'to_nchw', 'x'.join(map(str, shape)), str(dtype)[6:])
    return Row(name, values, run, pres, ('dhd_transpose_batched',), path=path, const=dict(g=['g']),
               src='a pure copy on every path: test_layout_conversion_is_a_pure_copy_in_both_directions')


ROWS += [_layout_row((3, 7, 5, 9), F32, True), _layout_row((3, 7, 5, 9), F32, False),
         _layout_row((2, 64, 20, 28), F16, True), _layout_row((2, 64, 20, 28), F16, False)]


# ---- mghs_op.depth_height_head -----------------------------------------------------------------------------------------

def _head_row(bn, d, c_, hb, extra, fh, fw, dtype, nhwc):
    fmt = CL if nhwc else None
    hr = [round(-1.0 + 0.1 * i, 1) for i in range(hb)]
    mr = [-1.0, hr[hb // 4], hr[hb // 2], hr[-1]]

    def values(gpu):
        hl = _randn((bn, hb + extra, fh, fw), 62, gpu, dtype, 3.0)
        hl[:, 3] = hl[:, 7]
        return dict(xd=_randn((bn, d + c_ + extra, fh, fw), 61, gpu, dtype, 3.0, fmt=fmt), hl=hl.contiguous(memory_format=fmt or torch.contiguous_format),
                    gd=_randn((bn, d, fh, fw), 63, gpu), gf=_randn((bn, c_, fh, fw), 64, gpu), gh=_randn((bn, hb, fh, fw), 65, gpu))

    def run(c, v):
        from dhd_amd import mghs_op
        xd, hl = c.inp('xd', v['xd'], grad=True), c.inp('hl', v['hl'], grad=True)
        depth, feat, height, band = mghs_op.depth_height_head(xd, hl, d, c_, hr, mr)
        torch.autograd.backward([c.grad('gd', depth), c.grad('gf', feat), c.grad('gh', height)], [v['gd'], v['gf'], v['gh']])
        return dict(depth=depth.detach(), feat=feat.detach(), height=height.detach(), band=band, gxd=xd.grad, ghl=hl.grad)

    kinds = (NHWC + ('channel_slice', 'offset16')) if nhwc else DENSE + NHWC
    name = 'depth_height_head_%s_%s_%s' % ('x'.join(map(str, (bn, d, c_, hb, extra, fh, fw))), str(dtype)[6:], 'nhwc' if nhwc else 'nchw')
    return Row(name, values, run, dict(xd=('fresh',) + kinds, hl=kinds, gd=GRAD, gf=GRAD, gh=GRAD),
               ('dhd_mghs_softmax_forward', 'dhd_mghs_softmax_backward'), const=dict(gd=['gd'], gf=['gf'], gh=['gh']),
               src='scalar kernels read the view where it lies: test_depth_height_head_one_launch_vs_torch')


ROWS += [_head_row(5, 88, 32, 17, 3, 7, 9, F32, False), _head_row(5, 88, 32, 17, 3, 7, 9, F16, True),
         _head_row(2, 9, 8, 65, 0, 1, 3, BF16, False), _head_row(2, 9, 8, 65, 0, 1, 3, F32, True)]


# ---- view transform: mghs_pool, mghs_lift_pool and the raw-layout helpers ----------------------------------------------

def _vt_inputs(gpu, channels):
    from dhd_amd import synthetic as syn
    from test_gpu_parity import T, device_calib, make_plan
    cfg = small_dhds_cfg()
    cfg['out_channels'] = channels
    n_cams = 3
    calib_np = syn.make_calibration(70 + channels, 1, n_cams, cfg['input_size'])
    depth, feat, hidx = syn.lift_inputs(80 + channels, 1, n_cams, 44, 4, 11, channels, 65)
    plan, axes = make_plan(cfg, 1, n_cams, channels=channels)
    plan_det = type(plan)(1, n_cams, plan.desc.n_depth, plan.desc.fh, plan.desc.fw, channels, plan.grids, deterministic=True)
    calib, keep = device_calib(calib_np, axes, gpu)
    height = T(syn.height_probs_from_index(hidx, len(cfg['height_range'])), gpu)
    return cfg, plan_det, calib, keep, T(depth, gpu), T(feat, gpu), height


def _vt_row(channels, lift, out_dtype):
    """depth (B*N, D, fH, fW), tran_feat -- presented as the reference forms it, a channel slice of the depth net's output --
    and the height distribution, deterministic mode; C = 64 is the compact path, with half outputs."""
    state = {}

    def values(gpu):
        cfg, plan, calib, keep, depth, feat, height = _vt_inputs(gpu, channels)
        state.update(cfg=cfg, plan=plan, calib=calib, keep=keep)
        v = dict(depth=depth, feat=feat, height=height)
        for k, s in enumerate(plan.out_shapes()):
            v['g%d' % k] = _randn(tuple(s), 90 + k, gpu, out_dtype)
        return v

    def run(c, v):
        from dhd_amd import mghs_op
        cfg, plan, calib = state['cfg'], state['plan'], state['calib']
        depth, feat = c.inp('depth', v['depth'], grad=True), c.inp('feat', v['feat'], grad=True)
        height = c.inp('height', v['height'])
        if lift:
            outs = mghs_op.mghs_lift_pool(plan, calib, height, cfg['height_range'], cfg['mask_range'], depth, feat, out_dtype=out_dtype)
        else:
            band = mghs_op.height_band(height, cfg['height_range'], cfg['mask_range'])
            outs = mghs_op.mghs_pool(plan, calib, band, depth, feat, out_dtype=out_dtype)
        torch.autograd.backward([c.grad('g%d' % k, o) for k, o in enumerate(outs)], [v['g%d' % k] for k in range(len(outs))])
        res = {'out%d' % k: o.detach() for k, o in enumerate(outs)}
        res.update(gdepth=depth.grad, gfeat=feat.grad)
        return res

    def close(key, got, ref, tol_):      # test_view_transform_small_vs_reference: gradients atol 2e-5, rtol 1e-5
        if key.startswith('out'):
            return torch.equal(got, ref)      # deterministic mode
        return bool(np.allclose(got.float().cpu().numpy(), ref.float().cpu().numpy(), atol=2e-5, rtol=1e-5))

    # off the compact path (C != 64) the backward adds into feat_grad with float atomics: two fresh runs differ in its last bits
    tol = (lambda t, k: 1.0) if channels != 64 else None
    pres = dict(depth=('fresh',) + DENSE, feat=DENSE, height=DENSE, g0=GRAD, g2=GRAD)
    entries = ('dhd_mghs_lift',) if lift else ('dhd_height_band', 'dhd_mghs_prepare', 'dhd_feat_nchw_to_nhwc')
    name = 'mghs_%s_c%d_%s' % ('lift_pool' if lift else 'pool', channels, str(out_dtype)[6:])
    return Row(name, values, run, pres, entries + ('dhd_mghs_forward_views', 'dhd_mghs_backward_views'), tol=tol, close=close,
               const=dict(g0=['g0'], g2=['g2']),
               src='test_view_transform_small_vs_reference' if channels != 64 else 'copy, same kernels, deterministic mode: test_deterministic_mode_makes_the_forward_bit_reproducible')


ROWS += [_vt_row(8, False, F32), _vt_row(8, True, F32), _vt_row(64, True, F32), _vt_row(64, True, F16)]


def _vt_helpers_row():
    """The helpers that take raw layouts: a dense view is handled (the compact path's 16-byte rows are the library's check: C = 8
    here, the generic path), a strided view is refused with DhdError -- never read as if it were dense."""
    state = {}

    def values(gpu):
        cfg, plan, calib, keep, depth, feat, height = _vt_inputs(gpu, 8)
        state.update(cfg=cfg, plan=plan, calib=calib, keep=keep)
        from dhd_amd import mghs_op
        v = dict(depth=depth, feat=feat, height=height, feat_nhwc=feat.permute(0, 2, 3, 1).contiguous())
        for k, s in enumerate(plan.out_shapes()):
            v['g%d' % k] = _randn(tuple(s), 90 + k, gpu)
        return v

    def run(c, v):
        from dhd_amd import mghs_op
        cfg, plan, calib = state['cfg'], state['plan'], state['calib']
        height = c.inp('height', v['height'])
        band = mghs_op.height_band(height, cfg['height_range'], cfg['mask_range'])
        rank, _ = mghs_op.voxel_index(plan, calib, 1)
        nhwc = mghs_op._nchw_to_nhwc(c.inp('feat', v['feat']))
        back = mghs_op._nhwc_to_nchw(c.inp('feat_nhwc', v['feat_nhwc']))
        ws = plan.new_workspace(v['depth'].device)
        band2, fl = mghs_op.lift(plan, calib, height, cfg['height_range'], cfg['mask_range'], c.inp('tran_feat', v['feat']), ws)
        depth = c.inp('depth', v['depth'])
        fn = c.inp('pool_feat', fl)
        outs = mghs_op.pool_forward(plan, depth, fn, ws)
        outs2 = mghs_op.pool_forward_phases(plan, depth, fn, ws)
        gs = [c.inp('g%d' % k, v['g%d' % k]) for k in range(len(outs))]
        dg, fg = mghs_op.pool_backward(plan, depth, fn, gs, ws)
        res = dict(band=band, band2=band2, rank=rank, nhwc=nhwc, back=back, fl=fl, dg=dg, fg=fg)
        res.update({'out%d' % k: o for k, o in enumerate(outs)})
        res.update({'phase%d' % k: o for k, o in enumerate(outs2)})
        return res

    dense = ('offset16', 'offset_elem')
    strided = ('channel_slice', 'inner_step2')
    pres = dict(height=('fresh',) + DENSE, feat=dense + strided, feat_nhwc=dense + strided, tran_feat=dense + strided, depth=dense + strided,
                pool_feat=dense + strided, g1=dense + ('inner_step2',))    # (one sample: a channel slice of a pooled tensor is dense)
    return Row('mghs_raw_layout_helpers_c8', values, run, pres,
               ('dhd_height_band', 'dhd_mghs_voxel_index', 'dhd_feat_nchw_to_nhwc', 'dhd_feat_nhwc_to_nchw', 'dhd_mghs_lift', 'dhd_mghs_forward',
                'dhd_mghs_forward_gather', 'dhd_mghs_forward_stream', 'dhd_mghs_backward'),
               raises=lambda t, k: (t != 'height' and k in strided) or (t == 'g1' and k == 'offset_elem'),
               # C = 8 is off the compact path: its backward adds into feat_grad with float atomics (two fresh runs differ)
               tol=lambda t, k: 1.0,
               close=lambda key, got, ref, tol_: (bool(np.allclose(got.cpu().numpy(), ref.cpu().numpy(), atol=2e-5, rtol=1e-5))
                                                  if key in ('fg', 'dg') else torch.equal(got, ref)),
               src='test_view_transform_small_vs_reference (gradients atol 2e-5, rtol 1e-5); everything else identical')


ROWS.append(_vt_helpers_row())


# ---- bev_pool_v2: three-step and fused ---------------------------------------------------------------------------------

def _bev_row(channels, fused):
    B, N, D, fh, fw = 2, 2, 44, 8, 22
    shape = (B, 1, 40, 48, channels)

    def values(gpu):
        from dhd_amd import synthetic as syn
        from test_gpu_parity import T, _ragged_lists
        rd, rf, rb, st, ln = _ragged_lists(5, B, N, D, fh, fw, 1, 40, 48)
        return dict(depth=T(syn.hash_signed(170, (B, N, D, fh, fw)), gpu), feat=T(syn.hash_signed(171, (B, N, fh, fw, channels)), gpu),
                    rd=T(rd, gpu), rf=T(rf, gpu), rb=T(rb, gpu), st=T(st, gpu), ln=T(ln, gpu), rb64=T(rb, gpu).long(),
                    g=T(syn.hash_signed(172, (B, channels, 1, 40, 48)), gpu))

    def run(c, v):
        import importlib
        bp = importlib.import_module('dhd_amd.bev_pool_v2')      # (the package exports the function under the module's name)
        bp.clear_caches()
        depth, feat = c.inp('depth', v['depth'], grad=True), c.inp('feat', v['feat'], grad=True)
        rb = c.inp('rb64', v['rb64']) if c.target == 'rb64' else c.inp('rb', v['rb'])
        out = bp.bev_pool_v2(depth, feat, c.inp('rd', v['rd']), c.inp('rf', v['rf']), rb, shape, c.inp('st', v['st']), c.inp('ln', v['ln']),
                             fused=fused)
        c.grad('g', out).backward(v['g'])
        bp.clear_caches()
        return dict(out=out.detach(), gdepth=depth.grad, gfeat=feat.grad)

    def tol(t, k):
        # three-step entry points: a misaligned feat / out_grad takes the scalar kernels (another summation order);
        # the fused wrapper copies, so the same kernels run
        return 3e-5 if (not fused and k == 'offset_elem' and t in ('feat', 'g')) else None

    def close(key, got, ref, tol_):
        return bool(np.allclose(got.cpu().numpy(), ref.cpu().numpy(), atol=tol_ if key != 'gdepth' else 1e-5, rtol=1e-5))

    pres = dict(depth=('fresh',) + DENSE, feat=DENSE, rd=FLAT, rf=FLAT, rb=FLAT, rb64=FLAT, st=FLAT, ln=FLAT, g=GRAD)
    entries = ('dhd_bev_pool_v2_fused_forward', 'dhd_bev_pool_v2_fused_backward') if fused else ('dhd_bev_pool_v2_forward', 'dhd_bev_pool_v2_backward')
    return Row('bev_pool_v2_%s_c%d' % ('fused' if fused else 'three_step', channels), values, run, pres, entries, tol=tol, close=close,
               const=dict(g=['g']), src='test_bev_pool_v2_operator_ragged_intervals (atol 3e-5 / 1e-5, rtol 1e-5)')


ROWS += [_bev_row(8, False), _bev_row(20, False), _bev_row(64, False), _bev_row(64, True)]


# ---- occupancy losses, argmax + histogram, occupancy head at inference -------------------------------------------------

def _occ_values(m, gpu):
    gen = _gen(m)
    z = (3.0 * torch.randn(m, 18, generator=gen)).to(gpu)
    t = torch.randint(0, 18, (m,), generator=gen)
    t[t == 5] = 4
    t[::97] = 255
    t[0], t[1] = 3, 17
    cam = (torch.rand(m, generator=gen) < 0.4)
    cam[:2] = True
    from dhd_amd.detector import NUSC_CLASS_FREQUENCIES
    cw = torch.from_numpy((1 / np.log(NUSC_CLASS_FREQUENCIES + 0.001)).astype(np.float32)).to(gpu)
    return dict(z=z, t=t.to(gpu), t8=t.to(torch.uint8).to(gpu), cam=cam.to(torch.uint8).to(gpu), cw=cw,
                g=torch.tensor([0.7, 1.3, 2.0], device=gpu))


def _occ_loss_row(m):
    def run(c, v):
        from dhd_amd.occ_loss import _OccLosses, occ_losses
        z = c.inp('z', v['z'], grad=True)
        t = c.inp('t8', v['t8']) if c.target == 't8' else c.inp('t', v['t'])
        cam, cw = c.inp('cam', v['cam']), c.inp('cw', v['cw'])
        if c.target == 'g':       # the (3,) gradient reaches the node as it is only through the node itself
            losses = _OccLosses.apply(z, t.to(torch.uint8), cam, cw, 255, 17)
            c.grad('g', losses).backward(v['g'])
        else:
            losses = torch.stack(occ_losses(z, t, cam, cw))
            losses.backward(v['g'])
        return dict(losses=losses.detach(), gz=z.grad)

    def values(gpu):
        return _occ_values(m, gpu)

    return Row('occ_losses_m%d' % m, values, run,
               dict(z=('fresh',) + DENSE, t=FLAT, t8=FLAT, cam=FLAT, cw=FLAT, g=FLAT + ('expanded',)),
               ('dhd_occ_loss_forward', 'dhd_occ_loss_backward'), const=dict(g=['g']),
               src='copy, same kernels (block sums in a fixed order): test_occ_losses_vs_torch_autograd')


def _occ_hist_row(m):
    def run(c, v):
        from dhd_amd.occ_loss import occ_argmax_hist
        t = c.inp('t8', v['t8']) if c.target == 't8' else c.inp('t', v['t'])
        pred, hist = occ_argmax_hist(c.inp('z', v['z']), t, c.inp('cam', v['cam']))
        return dict(pred=pred, hist=hist)

    return Row('occ_argmax_hist_m%d' % m, lambda gpu: _occ_values(m, gpu), run, dict(z=('fresh',) + DENSE, t=FLAT, t8=FLAT, cam=FLAT),
               ('dhd_occ_argmax_hist',), src='integer results: test_occ_argmax_and_confusion_histogram_vs_oracle')


ROWS += [_occ_loss_row(255), _occ_loss_row(4097), _occ_hist_row(255), _occ_hist_row(4097)]


def _occ_head_row(dtype, nhwc):
    shape = (1, 1, 1)    # the smallest shape of tests/occ_head_inputs.py

    def values(gpu):
        import occ_head_inputs as I
        w1, b1, w2, b2 = I.head_params(I.make_head(), gpu)
        x = I.make_x(shape).to(gpu).to(dtype)
        lab = torch.randint(0, 18, (1, 1, 1, 16), generator=_gen(3)).to(torch.uint8).to(gpu)
        return dict(x=x.contiguous(memory_format=CL) if nhwc else x, w1=w1, b1=b1, w2=w2, b2=b2, lab=lab, cam=torch.ones_like(lab))

    def run(c, v):
        from dhd_amd.occ_head import occ_head_infer
        names = ('w1', 'b1', 'w2', 'b2')
        if c.target == 'flat_params':      # the four parameters as views of ONE flat buffer, as a flattened optimiser state has them
            sizes = [v[n].numel() for n in names]
            flat = c.inp('flat_params', torch.cat([torch.zeros(1, device=v['x'].device)] + [v[n].reshape(-1) for n in names]))
            ps, at = [], 1
            for n, s in zip(names, sizes):
                ps.append(flat[at:at + s].view(v[n].shape))
                at += s
        else:
            ps = [c.inp(n, v[n]) for n in names]
        pred, hist, logits = occ_head_infer(c.inp('x', v['x']), *ps, labels=c.inp('lab', v['lab']), mask_camera=c.inp('cam', v['cam']),
                                            return_logits=True)
        return dict(pred=pred, hist=hist, logits=logits)

    kinds = ('fresh',) + (NHWC if nhwc else ('offset16', 'offset_elem')) + ('channel_slice',)
    return Row('occ_head_infer_%s_%s' % (str(dtype)[6:], 'nhwc' if nhwc else 'nchw'), values, run,
               dict(x=kinds, flat_params=('offset16', 'offset_elem'), b2=FLAT, w2=('offset_elem',), lab=('offset_elem', 'inner_step2'),
                    cam=('offset_elem',)),
               ('dhd_occ_head_infer',), src='copy, same kernel: test_gpu_occ_head_infer.py')


ROWS += [_occ_head_row(F32, False), _occ_head_row(F16, True)]


# ---- label_loss: fg_bce, bin_labels, points_to_maps ---------------------------------------------------------------------

def _fg_bce_row():
    bn, ch, h, w = 2, 9, 4, 11

    def values(gpu):
        g = _gen(71)
        pred = torch.softmax(torch.randn(bn, ch, h, w, generator=g), 1).to(gpu)
        b = torch.randint(0, ch + 1, (bn * h * w,), generator=g)
        fg = torch.randint(0, 3, (bn * h * w,), generator=g)
        return dict(pred=pred, b16=b.to(torch.int16).to(gpu), fg16=fg.to(torch.int16).to(gpu), b64=b.to(gpu), fg64=fg.to(gpu),
                    g=torch.tensor(1.7, device=gpu))

    def run(c, v):
        from dhd_amd import label_loss
        pred = c.inp('pred', v['pred'], grad=True)
        wide = c.target in ('b64', 'fg64')
        b = c.inp('b64', v['b64']) if wide else c.inp('b16', v['b16'])
        fg = c.inp('fg64', v['fg64']) if wide else c.inp('fg16', v['fg16'])
        loss = label_loss.fg_bce(pred, b, fg, 3.0)
        c.grad('g', loss).backward(v['g'])
        return dict(loss=loss.detach(), gpred=pred.grad)

    return Row('fg_bce_2x9x4x11', values, run,
               dict(pred=('fresh',) + DENSE + NHWC, b16=FLAT, fg16=FLAT, b64=FLAT, fg64=('fresh',) + FLAT, g=('offset_elem',)),
               ('dhd_bin_bce_forward', 'dhd_bin_bce_backward'), src='copy / conversion, same kernels: test_height_and_depth_loss_vs_torch_mirror_full_size')


def _bin_labels_row():
    def values(gpu):
        g = _gen(72)
        sel = torch.rand(1, 2, 64, 48, generator=g) < 0.05
        return dict(gd=(torch.rand(1, 2, 64, 48, generator=g) * 50.0 * sel).to(gpu), gh=((torch.rand(1, 2, 64, 48, generator=g) * 7.4 - 1.5) * sel).to(gpu))

    def run(c, v):
        from dhd_amd import label_loss
        out = {}
        for sid in (False, True):
            d, h = label_loss.bin_labels(c.inp('gd', v['gd']), c.inp('gh', v['gh']), 16, [1.0, 45.0, 1.0], 44, -1.0, 0.1, 65, sid=sid)
            out.update({'d%d' % sid: d, 'h%d' % sid: h})
        return out

    return Row('bin_labels_1x2x64x48', values, run, dict(gd=('fresh',) + DENSE, gh=DENSE), ('dhd_sparse_bin_labels', 'dhd_sparse_bin_labels_sid'),
               src='integer results: test_height_loss_labels_and_value_vs_reference_golden')


def _points_row():
    def values(gpu):
        g = _gen(73)
        n = 700
        pts = torch.stack([torch.rand(2, n, generator=g) * 190 - 8, torch.rand(2, n, generator=g) * 76 - 7, torch.rand(2, n, generator=g) * 60.0,
                           torch.randn(2, n, generator=g) * 5.0], -1)
        return dict(pts=pts.to(gpu))

    def run(c, v):
        from dhd_amd.label_loss import points_to_maps
        dm, hm = points_to_maps(c.inp('pts', v['pts']), 64, 176, 2)
        return dict(dm=dm, hm=hm)

    return Row('points_to_maps_2x700', values, run, dict(pts=('fresh',) + DENSE), ('dhd_points_to_maps',),
               src='z-buffer minimum, order-independent: test_rasterise_points_vs_oracle_and_reference_golden')


ROWS += [_fg_bce_row(), _bin_labels_row(), _points_row()]


# ---- DCN module and _DeformIm2col --------------------------------------------------------------------------------------

def _dcn_module_row():
    b, ch, h, w, dil = 2, 10, 7, 9, 2

    def values(gpu):
        return dict(x=_randn((b, ch, h, w), 81, gpu), g=_randn((b, 2 * ch, h, w), 82, gpu))

    def run(c, v):
        from dhd_amd.depthnet import DCN
        torch.manual_seed(ch + h)
        m = DCN(ch, 2 * ch, kernel_size=3, padding=dil, dilation=dil, groups=1)
        with torch.no_grad():
            m.conv_offset.weight.normal_(0, 0.15)
            m.conv_offset.bias.normal_(0, 3.0)
        m = m.to(v['x'].device)
        x = c.inp('x', v['x'], grad=True)
        y = m(x)
        c.grad('g', y).backward(v['g'])
        out = dict(y=y.detach(), gx=x.grad)
        out.update({'d_' + n: p.grad for n, p in m.named_parameters()})
        return out

    def close(key, got, ref, tol_):      # test_dcn_hip_sampling_vs_grid_sample_formulation: 1e-4 / 2e-4 / 5e-4
        return _rel_close(key, got, ref, {'y': 1e-4, 'gx': 2e-4}.get(key, 5e-4))

    # the gather form of col2im sums a cell's corner entries in the arrival order of its counting atomics: the gradients of
    # two runs differ in the last bits whatever the layout, so every case of this row compares at the sampling test's bar
    return Row('dcn_module_2x10x7x9_dil2', values, run, dict(x=('fresh',) + DENSE + NHWC, g=GRAD), ('dhd_deform_im2col_t', 'dhd_deform_col2im_t'),
               tol=lambda t, k: 1.0, close=close, const=dict(g=['g']), src='test_dcn_hip_sampling_vs_grid_sample_formulation')


def _deform_row(col_dtype):
    b, ch, h, w, k = 3, 16, 16, 44, 3

    def values(gpu):
        return dict(x=_randn((b, ch, h, w), 83, gpu), off=_randn((b, 2 * k * k, h, w), 84, gpu, scale=0.5),
                    g=_randn((b, ch * k * k, h * w), 85, gpu, col_dtype))

    def run(c, v):
        from dhd_amd.depthnet import _DeformIm2col
        x, off = c.inp('x', v['x'], grad=True), c.inp('off', v['off'], grad=True)
        col = _DeformIm2col.apply(x, off, k, 1, 1, col_dtype)
        c.grad('g', col).backward(v['g'])
        return dict(col=col.detach(), gx=x.grad, goff=off.grad)

    def close(key, got, ref, tol_):      # test_dcn_gather_col2im_vs_atomic_form_and_typed_columns: dx 2e-5, col and doffset identical
        return _rel_close(key, got, ref, 2e-5) if key == 'gx' else torch.equal(got, ref)

    return Row('deform_im2col_3x16x16x44_cols_' + str(col_dtype)[6:], values, run, dict(x=('fresh',) + DENSE + NHWC, off=DENSE, g=FLAT + ('channel_slice', 'expanded')),
               ('dhd_deform_im2col_t', 'dhd_deform_col2im_t'), tol=lambda t, kk: 1.0, close=close, const=dict(g=['g']),
               src='test_dcn_gather_col2im_vs_atomic_form_and_typed_columns')


ROWS += [_dcn_module_row(), _deform_row(F32), _deform_row(F16)]


# ---- stereo cost volume ------------------------------------------------------------------------------------------------

def _stereo_row():
    bn, ch, h, w, d = 2, 16, 6, 10, 8

    def values(gpu):
        grid = torch.rand(bn, d * h, w, 2, generator=_gen(93)) * 2.6 - 1.3
        grid[0, :w] = -2.0
        return dict(prev=_randn((bn, ch, h, w), 91, gpu), curr=_randn((bn, ch, h, w), 92, gpu), grid=grid.to(gpu))

    def run(c, v):
        from dhd_amd.depthnet import DepthNet
        torch.manual_seed(1)
        dn = DepthNet(32, 32, 16, d, use_dcn=False, aspp_mid_channels=16, stereo=True, bias=5.0)
        return dict(cv=dn._hip_cost_volume(c.inp('prev', v['prev']), c.inp('curr', v['curr']), c.inp('grid', v['grid']), d, (ch // 4 - 1) * 4))

    return Row('stereo_cost_volume_2x16x6x10x8', values, run, dict(prev=('fresh',) + DENSE + NHWC, curr=DENSE, grid=DENSE),
               ('dhd_stereo_cost_volume', 'dhd_feat_nchw_to_nhwc'), src='copy, same kernel: test_stereo_cost_volume_vs_grid_sample_formulation')


ROWS.append(_stereo_row())


# ---- RayIoU.add_batch and render_forward ---------------------------------------------------------------------------------

def _ray_row():
    nx, ny, nz = 37, 23, 5

    def values(gpu):
        rs = np.random.RandomState(7)
        stack = torch.from_numpy(rs.randint(0, 18, size=(2, 2, nx, ny, nz)).astype(np.uint8))
        stack[rs.rand(2, 2, nx, ny, nz) < 0.9] = 17                     # mostly free
        org = torch.tensor([[7.3, 4.6, 1.0], [0.4, 0.7, 0.2], [8.2, 3.9, 1.5]], dtype=torch.float64)
        occ = torch.from_numpy((rs.rand(1, 1, nz, ny, nx) < 0.04).astype(np.float32))
        o_vox = torch.tensor([[[17.3, 11.6, 2.4], [0.4, 0.7, 0.2]]])
        dirs = torch.nn.functional.normalize(torch.randn(64, 3, generator=_gen(9)), dim=1)
        pts = (o_vox[0].repeat_interleave(64, 0) + dirs.repeat(2, 1) * 70)[None]
        tindex = torch.arange(2, dtype=torch.float32).repeat_interleave(64)[None]
        return dict(pred=stack[0].to(gpu), gt=stack[1].to(gpu), org64=org.to(gpu), org32=org.float().to(gpu), sigma=occ.to(gpu),
                    origin=o_vox.to(gpu), pts=pts.to(gpu), tindex=tindex.to(gpu))

    def run(c, v):
        import dhd_amd
        # pred / gt: slices of a stacked batch; origins: three columns of a wider (n, 3 + 5) array (present's channel_slice),
        # float64 and float32 (each takes the reference's arithmetic of that precision: two sets of counters)
        pred, gt = c.inp('pred', v['pred']), c.inp('gt', v['gt'])
        m, m32 = (dhd_amd.RayIoU(pc_range=(0.0, 0.0, 0.0, nx * 0.4, ny * 0.4, nz * 0.4), voxel_size=0.4) for _ in range(2))
        org, org32 = c.inp('org64', v['org64']), c.inp('org32', v['org32'])
        m.add_batch(pred, gt, [org, org])
        m32.add_batch(pred, gt, [org32, org32])
        pd, gd, ci = dhd_amd.render_forward(c.inp('sigma', v['sigma']), c.inp('origin', v['origin']), c.inp('pts', v['pts']),
                                            c.inp('tindex', v['tindex']), [1, nz, ny, nx], 'test')
        return dict(counts=m.counts, counts32=m32.counts, pd=pd, gd=gd, ci=ci)

    return Row('rayiou_37x23x5', values, run,
               dict(pred=('fresh',) + DENSE, gt=DENSE, org64=('channel_slice', 'offset_elem'), org32=('channel_slice', 'offset_elem'),
                    sigma=DENSE, origin=DENSE, pts=DENSE, tindex=DENSE),
               ('dhd_ray_iou_accumulate', 'dhd_ray_render_forward'), src='integer counters, double-precision walk: test_gpu_ray_metrics.py')


ROWS.append(_ray_row())


# ---- EMA update: parameters that are views into one flat buffer at odd offsets ----------------------------------------

def _ema_row():
    sizes = [1, 3, 64, 1023, 5000, 0]

    def values(gpu):
        from dhd_amd import synthetic as syn
        total = sum(n + 1 for n in sizes)
        return dict(flat=torch.from_numpy(syn.hash_signed(300, (total,))).to(gpu), step=torch.from_numpy(syn.hash_signed(301, (total,))).to(gpu))

    def run(c, v):
        from dhd_amd.ema import ModelEMA
        def net_of(flat):
            net = torch.nn.Module()
            net.p = torch.nn.ParameterList()
            at = 1                                # every parameter starts one element after the previous one's end: odd offsets
            for n in sizes:
                net.p.append(torch.nn.Parameter(flat[at:at + n]))
                at += n + 1
            return net
        ema = ModelEMA(net_of(c.inp('flat', v['flat'])), decay=0.999, updates=100)     # the EMA copy keeps the views' layout
        ema.update(None, net_of(c.inp('flat', v['flat'] + v['step'])))                 # the model after a step, laid out alike
        return {'ema%d' % i: p.detach().clone() for i, p in enumerate(ema.ema.p)}

    # a strided parameter is not something a launch over linear chunks can walk: the reference's own expression through torch
    # (the one-element parameter is dense whatever its stride, so the launch still happens: the path does not change)
    return Row('ema_flat_buffer_views', values, run, dict(flat=('fresh',) + FLAT), ('dhd_ema_update',),
               src='element-wise, the same two roundings on either path: test_ema_update_ragged_state_vs_oracle')


ROWS.append(_ema_row())


# --------------------------------------------------------------------------------------------- the test

CASES = [pytest.param(row, target, kind, id='%s-%s-%s' % (row.name, target, kind))
         for row in ROWS for target, kinds in row.present.items() for kind in kinds]

_values, _fresh = {}, {}


def _row_values(row, gpu, target, kind):
    if row.name not in _values:
        _values[row.name] = row.values(gpu)
    v = _values[row.name]
    const = row.const.get(target, ()) if kind == 'expanded' else ()
    if const:
        v = dict(v)
        for k in const:
            v[k] = torch.full_like(v[k], 0.5)
    return v, tuple(const)


def _watched(row, seen):
    return collections.Counter(name for how, name in seen if how == 'call' and name in row.watch)


def _fresh_run(row, gpu, v, const, monkeypatch):
    key = (row.name, const)
    if key not in _fresh:
        with monkeypatch.context() as mp:
            seen = _record(mp)
            out = row.run(Case(None, 'fresh'), v)
            torch.cuda.synchronize()
        calls = _watched(row, seen)
        checked = {name for how, name in seen if how == 'check'}
        for e in row.entries:     # the module must not compare torch with torch
            assert calls[e] > 0, f'{row.name}: a fresh run does not reach {e}: {dict(calls)}'
        _fresh[key] = ({k: t.detach().clone() for k, t in out.items()}, calls, checked)
    return _fresh[key]


def test_the_table_covers_every_function_that_hands_a_pointer_to_the_library():
    """Every function of dhd_amd/ that passes a tensor pointer to the library (`_lib.ptr(` or `.data_ptr()` next to a library
    call) belongs to an operator with a row here; the C entry points the rows watch are the checkable form of that.  The
    spellings of a library call: `lib.dhd_x(`, `load().dhd_x(`, `_call('dhd_x'`, `_lib.call('dhd_x'` and `_lib.value('dhd_x'`."""
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dhd_amd')
    called = set()
    for f in os.listdir(root):
        if f.endswith('.py') and f != '_lib.py':
            called |= set(re.findall(r'\b(?:lib|load\(\))\.(dhd_[a-z0-9_]+)', open(os.path.join(root, f)).read()))
            called |= set(re.findall(r"(?:_call|\bcall|\bvalue)\(\s*'(dhd_[a-z0-9_]+)'", open(os.path.join(root, f)).read()))
    launching = {n for n in called if not n.endswith(('_supported', '_bytes')) and n != 'dhd_abi_version'}
    assert {'dhd_window_attn_infer', 'dhd_window_attn_backward', 'dhd_deform_conv_infer'} <= launching      # the _lib.call spelling is seen
    watched = {e for row in ROWS for e in row.watch}
    # not operators on caller tensors: calibration stream of bench.py, test-only introspection, graph-capture twin of dhd_ema_update,
    # the cross-rank phases of the SFA stage (two ranks: test_fused_sfa_stage_under_syncbatchnorm_two_ranks), static-rig lift
    exempt = {'dhd_hbm_calibrate', 'dhd_mghs_debug_keys', 'dhd_mghs_stats', 'dhd_ema_update_dev', 'dhd_sfa_stage_forward_phase',
              'dhd_sfa_stage_backward_phase', 'dhd_mghs_lift_static', 'dhd_bev_pool_v2_regroup', 'dhd_deform_col2im', 'dhd_deform_im2col'}
    # shown on views by a test of their own, which carves the tensor out of a poisoned parent with present() as the rows here do
    exempt |= {'dhd_deform_conv_infer',        # test_gpu_deform_conv_infer.py::test_views
               'dhd_window_attn_backward',     # test_gpu_window_attn_train.py::test_a_strided_or_misaligned_dout_is_copied
               'dhd_window_attn_infer'}        # test_gpu_window_attn_infer.py::test_views_of_qkv
    assert launching - watched - exempt == set(), sorted(launching - watched - exempt)



@pytest.mark.gpu
@pytest.mark.parametrize('row,target,kind', CASES)
def test_operator_on_a_view(gpu, monkeypatch, row, target, kind):
    from dhd_amd import _lib
    v, const = _row_values(row, gpu, target, kind)
    ref, ref_calls, _ = _fresh_run(row, gpu, v, const, monkeypatch)
    case = Case(target, kind)
    seen = _record(monkeypatch)
    if row.raises(target, kind):
        with pytest.raises(_lib.DhdError):
            row.run(case, v)
        torch.cuda.synchronize()
        print(f'{row.name} [{target} as {kind}]: refused with DhdError, as the table expects')
        assert case.untouched()
        return
    try:
        got = row.run(case, v)
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device fault poisons the process: nothing more is started on the GPU
        if 'HIP error' in str(e) or 'illegal memory access' in str(e):
            pytest.exit(f'{row.name} [{target} as {kind}]: GPU fault, stopping the module: {e}', returncode=3)
        raise
    calls = _watched(row, seen)
    expected = collections.Counter(ref_calls)
    override = row.path(target, kind)
    if override:
        for name, n in override.items():
            expected[name] = n
    expected = +expected
    tol = row.tol(target, kind)
    print(f'{row.name} [{target} as {kind}]: path {dict(calls)}; expected {dict(expected)}; '
          f'{"torch.equal with the fresh run" if tol is None else "tolerance of " + row.src}')
    # 1. the same results
    keys = row.fresh_keys(target, kind) or tuple(ref)
    assert set(got) == set(ref)
    for k in keys:
        a, b = got[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if tol is None:
            assert torch.equal(a, b), (k, float((a.double() - b.double()).abs().max()) if a.numel() else 0.0)
        else:
            assert row.close(k, a, b, tol), (k, float((a.double() - b.double()).abs().max()))
    if tol is not None and row.ref64 is not None:
        r64 = row.ref64(v, got)
        for k in r64:
            assert row.close(k, got[k], r64[k], tol), ('float64', k, float((got[k].double() - r64[k]).abs().max()))
    # 2. memory: values and poison untouched; gradients in the shape and dtype of the input as presented
    assert case.untouched(), 'a parent buffer changed: the view was written to, or something wrote outside it'
    for name, t in case.shown.items():
        if t.requires_grad:
            assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == t.dtype, name
    # 3. the path taken
    assert calls == expected, (dict(calls), dict(expected))
