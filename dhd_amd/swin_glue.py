"""The memory-bound glue of a Swin block as HIP operators (csrc/swin_glue.hip, section X1 of include/dhd_amd_ext.h):

  layer_norm_rows      LayerNorm written straight into the shifted-window partition (norm1 -> windows in one pass), or, without
                       a window, LayerNorm over rows that emits another dtype (norm2 -> the dtype fc1 casts its input to)
  window_reverse_add   identity + scale[b] * reverse(windows): the window reverse with the residual add and DropPath's
                       per-image factor in it

Both are differentiable.  layer_norm_rows saves x, weight and bias and nothing else: its backward recomputes the row statistics
from x, gathers the incoming gradient through the reverse map over the real tokens (pad rows are never read), and sums the
weight and bias gradients without atomics, so dx, dweight and dbias are reproducible bit for bit.  window_reverse_add's backward
is the existing window partition of the incoming gradient.  The statistics are float32 (mean, then the centred sum of squares):
within the layer's 1e-4 bar of a float64 LayerNorm, not torch's bits, which is why `SwinBlock.fused_glue` is opt-in.

The entry points are reached through _ext.call(name, ...) / _ext.value(name, ...)."""
import torch

from . import _ext, _lib
from .trace import traced


# Below this many elements a LayerNorm with no cast to fuse stays with torch: at DHD-L's stage 2 / 3 maps in float32 (17.3 M / 8.7 M
# elements) the identity-map form moves the bytes torch's LayerNorm moves and measured 135.8 against 130.4 us and 81.3 against
# 74.2 us forward + backward (profiles/r12/swin_glue.json), while at stage 1 (34.6 M) it wins 214.6 against 412.5 us.
PLAIN_LN_MIN_NUMEL = 1 << 25


def swin_glue_supported(x, plain_ln_to=None):
    """True when the operators here take the token map `x` (..., C): a GPU tensor of float32, float16 or bfloat16 whose channel
    count the kernels hold in registers (a multiple of 8 from 8 to 2048).  With `plain_ln_to` the question is about the
    identity-map LayerNorm into that dtype (norm2 -> what fc1 reads): where nn.LayerNorm itself emits that dtype here (x's
    dtype, or float32 inside an autocast region) there is no cast to fuse, and a small map is routed to today's path
    (PLAIN_LN_MIN_NUMEL)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() >= 2 and x.dtype in _lib.DTYPE_CODE and x.numel() > 0):
        return False
    if plain_ln_to is not None and x.numel() < PLAIN_LN_MIN_NUMEL:
        todays = torch.float32 if torch.is_autocast_enabled() else x.dtype
        if plain_ln_to == todays:
            return False
    code = _lib.DTYPE_CODE[x.dtype]
    return bool(_ext.value('dhdx_ln_rows_supported', x.shape[-1], code, code))


def _row_geometry(x, window):
    """(b, h, w, window, shift, output shape) of a call on x (..., C)."""
    C = x.shape[-1]
    if window is None:
        if x.dim() < 2:
            raise _lib.DhdError(f'layer_norm_rows: x {tuple(x.shape)} is not (..., rows, C)')
        return x.numel() // (x.shape[-2] * C), x.shape[-2], 1, 0, 0, tuple(x.shape)
    H, W, ws, shift = window
    B = x.shape[0]
    if x.numel() != B * H * W * C:
        raise _lib.DhdError(f'layer_norm_rows: x {tuple(x.shape)} is not a (B, {H} x {W}, C) token map')
    return B, H, W, ws, shift, (B, -(-H // ws) * -(-W // ws), ws * ws, C)


def _affine(p, C, name):
    p = p.detach().float().contiguous()
    if tuple(p.shape) != (C,):
        raise _lib.DhdError(f'layer_norm_rows: {name} must have shape ({C},), got {tuple(p.shape)}')
    return _lib.dense16(p)


class _LayerNormRows(torch.autograd.Function):
    """out = LN(x) through the row map; saves x (the dense tensor the kernel read), weight and bias."""

    @staticmethod
    @traced('dhd.swin.glue.ln')
    def forward(ctx, x, weight, bias, eps, out_dtype, window):
        x = _lib.dense16(x.detach())
        C, dev = x.shape[-1], x.device
        b, h, w, ws, shift, shape = _row_geometry(x, window)
        gamma, beta = _affine(weight, C, 'weight'), _affine(bias, C, 'bias')
        with torch.cuda.device(dev):
            out = torch.empty(shape, dtype=out_dtype, device=dev)
            _ext.call('dhdx_ln_rows_forward', _lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(out), _lib.dtype_code(x.dtype),
                      _lib.dtype_code(out_dtype), b, h, w, C, ws, shift, float(eps), _lib.stream_ptr(dev))
        ctx.save_for_backward(x, weight, bias)
        ctx.args = (eps, window)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @traced('dhd.swin.glue.ln.backward')
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        eps, window = ctx.args
        C, dev = x.shape[-1], x.device
        b, h, w, ws, shift, _ = _row_geometry(x, window)
        dy = _lib.dense16(dy)       # a strided, expanded or misaligned gradient is copied; x was saved dense
        gamma = _affine(weight, C, 'weight')
        with torch.cuda.device(dev):
            dx = torch.empty_like(x)
            dgamma = torch.empty(C, dtype=torch.float32, device=dev)
            dbeta = torch.empty(C, dtype=torch.float32, device=dev)
            nbytes = _ext.value('dhdx_ln_rows_backward_scratch_bytes', b * h * w, C)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _ext.call('dhdx_ln_rows_backward', _lib.ptr(x), _lib.ptr(dy), _lib.ptr(gamma), _lib.ptr(dx), _lib.ptr(dgamma), _lib.ptr(dbeta),
                      _lib.ptr(scratch), nbytes, _lib.dtype_code(x.dtype), _lib.dtype_code(dy.dtype), b, h, w, C, ws, shift, float(eps),
                      _lib.stream_ptr(dev))
        return dx, dgamma.to(weight.dtype), dbeta.to(bias.dtype), None, None, None


def layer_norm_rows(x, weight, bias, eps, out_dtype=None, window=None):
    """LayerNorm over the last axis of x (..., C) with float32 `weight` and `bias` (C,), written through a row map.

    window = (H, W, ws, shift): x is a (B, H * W, C) or (B, H, W, C) token map and the result is the (B, nW, ws * ws, C) windows
    of the padded, cyclically shifted map, as `ShiftWindowMSA` cuts them -- rows that lie in the padding are exact zeros (the
    reference pads after the norm).  window = None: the result has x's shape.  out_dtype (default x's) may be any of float32,
    float16, bfloat16; a half result is the float32 result rounded once.  Differentiable in x, weight and bias; works under
    torch.autocast (the dtypes are the caller's, nothing is cast behind its back) and under checkpoint(use_reentrant=False).
    A view the kernels cannot read where it lies is copied first.  The forward allocates the result; the backward dx, the two
    parameter gradients and its scratch, all from the caching allocator."""
    if not (x.is_cuda and weight.is_cuda and bias.is_cuda):
        raise _lib.DhdError(f'layer_norm_rows: x, weight and bias must live on the GPU (got {x.device}, {weight.device}, {bias.device})')
    window = None if window is None else tuple(int(v) for v in window)
    return _LayerNormRows.apply(x, weight, bias, float(eps), out_dtype or x.dtype, window)


class _WindowReverseAdd(torch.autograd.Function):
    @staticmethod
    @traced('dhd.swin.glue.reverse_add')
    def forward(ctx, win, identity, H, W, ws, shift, scale):
        win, ident = _lib.dense16(win.detach()), _lib.dense16(identity.detach())
        B, C, dev = ident.shape[0], ident.shape[-1], ident.device
        nw = -(-H // ws) * -(-W // ws)
        if ident.numel() != B * H * W * C or win.numel() != B * nw * ws * ws * C or win.shape[-1] != C:
            raise _lib.DhdError(f'window_reverse_add: win {tuple(win.shape)} and identity {tuple(ident.shape)} do not fit '
                                f'{H} x {W} tokens in windows of {ws}')
        if scale is not None:
            scale = scale.detach().reshape(-1)
            if scale.dtype != torch.float32 or scale.numel() != B or not scale.is_cuda:
                raise _lib.DhdError(f'window_reverse_add: scale must be float32 ({B},) on the GPU')
            scale = scale.contiguous()
        with torch.cuda.device(dev):
            out = torch.empty(ident.shape, dtype=ident.dtype, device=dev)
            _ext.call('dhdx_window_reverse_add', _lib.ptr(win), _lib.ptr(ident), _lib.ptr(scale), _lib.ptr(out), _lib.dtype_code(win.dtype),
                      _lib.dtype_code(ident.dtype), B, H, W, C, ws, shift, _lib.stream_ptr(dev))
        ctx.save_for_backward(scale)
        ctx.args = (H, W, ws, shift, win.dtype, tuple(win.shape))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @traced('dhd.swin.glue.reverse_add.backward')
    def backward(ctx, g):
        from .swin import _WindowRows
        scale, = ctx.saved_tensors
        H, W, ws, shift, win_dtype, win_shape = ctx.args
        dwin = None
        if ctx.needs_input_grad[0]:
            dwin = _WindowRows.apply(g.reshape(g.shape[0], H, W, g.shape[-1]), H, W, ws, shift, False, win_dtype).view(win_shape)
            if scale is not None:
                dwin.mul_(scale.view(-1, 1, 1, 1))
        return dwin, g, None, None, None, None, None


def window_reverse_add(win, identity, H, W, ws, shift, scale=None):
    """identity + scale[b] * reverse(win): win (B, nW, ws * ws, C) windows as `layer_norm_rows(..., window=...)` lays them out,
    identity the (B, H * W, C) or (B, H, W, C) token map they are added to, scale float32 (B,) or None for 1 (DropPath's
    floor(keep + u) / keep per image).  The result has identity's shape and dtype; the sum is taken in float32 and rounded once,
    and with scale None it is bit-identical to `identity + reverse(win).float()` in identity's dtype.  Differentiable in win and
    identity (not in scale): identity's gradient is the incoming gradient itself, win's the window partition of it in win's
    dtype, times scale[b]."""
    if not (win.is_cuda and identity.is_cuda):
        raise _lib.DhdError(f'window_reverse_add: win and identity must live on the GPU (got {win.device}, {identity.device})')
    return _WindowReverseAdd.apply(win, identity, int(H), int(W), int(ws), int(shift), scale)
