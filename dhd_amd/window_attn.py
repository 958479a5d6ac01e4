"""Swin window attention at inference as one HIP operator (csrc/window_attn.hip, section 16 of include/dhd_amd.h): from the
qkv projection's output, as it lies, to the tensor the output projection reads.  The (3, B, windows x heads, N, d) operand copy,
the expanded (windows x heads, N, N) bias / mask and the transposed copy of the result that `WindowMSA.forward` makes around
`F.scaled_dot_product_attention` do not exist; the kernel reads the relative-position table and the region ids of the shifted
map and does the index arithmetic itself.  `window_attn_infer` is forward only (no autograd node); `window_attn` is the same forward
with the fused HIP backward (csrc/window_attn_bwd.hip, section 17) behind it, for training.

The entry points are reached through _lib.call(name, ...), the one spelling of a library call by name."""
import sys
import types

import torch

from . import _lib
from .trace import traced

HEAD_DIM = 32


def _gemm_code(gemm):
    return _lib.SFA_GEMM[gemm or 'default']


def window_attn_shape_supported(window_size, num_heads, dtype, numel, gemm=None, backward=False):
    """True when the library has a kernel for this window, head count and dtype, and `numel` elements of qkv are within its
    32-bit index space; with backward=True, when it also has the backward.  No tensor is needed to ask."""
    wh, ww = window_size
    if dtype not in _lib.DTYPE_CODE or numel >= 1 << 31:
        return False
    name = 'dhd_window_attn_backward_supported' if backward else 'dhd_window_attn_infer_supported'
    return bool(_lib.value(name, wh, ww, num_heads, HEAD_DIM, _lib.DTYPE_CODE[dtype], _gemm_code(gemm)))


def _qkv_supported(qkv, window_size, num_heads, gemm, backward):
    wh, ww = window_size
    if not (torch.is_tensor(qkv) and qkv.is_cuda and qkv.dim() >= 2):
        return False
    if wh < 1 or ww < 1 or num_heads < 1 or qkv.shape[-2] != wh * ww or qkv.shape[-1] != 3 * num_heads * HEAD_DIM:
        return False
    return window_attn_shape_supported(window_size, num_heads, qkv.dtype, qkv.numel(), gemm, backward)


def window_attn_infer_supported(qkv, window_size, num_heads, gemm=None):
    """True when window_attn_infer takes this call: a GPU tensor (..., N, 3 * num_heads * 32) of a dtype, and a window, that the
    kernel has."""
    return _qkv_supported(qkv, window_size, num_heads, gemm, False)


def window_attn_supported(qkv, window_size, num_heads, gemm=None):
    """True when window_attn takes this call, forward and backward."""
    return _qkv_supported(qkv, window_size, num_heads, gemm, True)


@traced('dhd.swin.attn.infer')
def window_attn_infer(qkv, table, window_size, num_heads, scale, regions=None, gemm=None):
    """qkv (..., nW, N, 3 * num_heads * 32) float32 / float16 / bfloat16, the output of the qkv projection for windows
    (..., nW, N, C); table ((2 Wh - 1)(2 Ww - 1), num_heads), the relative-position bias table; regions uint8 (nW, N) from
    swin.shift_window_regions, or None for unshifted windows.  Returns out (..., nW, N, num_heads * 32) in qkv's dtype.  A view
    the kernel cannot read where it lies -- strided, or dense at an address that is not a multiple of 16 bytes -- is copied
    first; the table is used as a float32 dense tensor.  The only allocation is `out`."""
    if not (qkv.is_cuda and table.is_cuda and (regions is None or regions.is_cuda)):
        raise _lib.DhdError(f'window_attn_infer: qkv, table and regions must live on the GPU (got {qkv.device}, {table.device})')
    wh, ww = window_size
    n, c = wh * ww, num_heads * HEAD_DIM
    if qkv.dim() < 3 or qkv.shape[-2] != n or qkv.shape[-1] != 3 * c:
        raise _lib.DhdError(f'window_attn_infer: qkv {tuple(qkv.shape)} is not (..., nW, {n}, {3 * c})')
    qkv = _lib.dense16(qkv.detach())
    table = _lib.require_gpu_tensor(table.detach().float().contiguous(), torch.float32, 'relative-position bias table')
    if tuple(table.shape) != ((2 * wh - 1) * (2 * ww - 1), num_heads):
        raise _lib.DhdError('window_attn_infer: inconsistent shapes of table and window')
    windows = qkv.numel() // (n * 3 * c)
    nw = qkv.shape[-3]
    if regions is not None:
        regions = regions.detach()
        if regions.dtype != torch.uint8 or tuple(regions.shape) != (nw, n):
            raise _lib.DhdError(f'window_attn_infer: regions must be uint8 ({nw}, {n}), got {regions.dtype} {tuple(regions.shape)}')
        regions = regions.contiguous()
    dev = qkv.device
    with torch.cuda.device(dev):
        out = torch.empty(tuple(qkv.shape[:-1]) + (c,), dtype=qkv.dtype, device=dev)
        _lib.call('dhd_window_attn_infer', _lib.ptr(qkv), _lib.dtype_code(qkv.dtype), _lib.ptr(table), _lib.ptr(regions), _lib.ptr(out),
                  windows, nw, wh, ww, num_heads, HEAD_DIM, float(scale), _gemm_code(gemm), _lib.stream_ptr(dev))
    return out


class _WindowAttn(torch.autograd.Function):
    """out = window_attn_infer(qkv, ...); saves its inputs and nothing else, the backward recomputes the softmax.  What is saved of
    qkv is the dense tensor the kernel read: qkv itself, or the one copy of a strided or misaligned view, which the backward
    reads again instead of copying a second time."""

    @staticmethod
    def forward(ctx, qkv, table, regions, window_size, num_heads, scale, gemm):
        qkv = _lib.dense16(qkv.detach())
        out = window_attn_infer(qkv, table, window_size, num_heads, scale, regions=regions, gemm=gemm)
        ctx.save_for_backward(qkv, table, regions)
        ctx.args = (window_size, num_heads, scale, gemm)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @traced('dhd.swin.attn.train')
    def backward(ctx, dout):
        qkv, table, regions = ctx.saved_tensors
        (wh, ww), nh, scale, gemm = ctx.args
        n, c = wh * ww, nh * HEAD_DIM
        dout = _lib.dense16(dout.to(qkv.dtype))       # a strided or misaligned gradient is copied; qkv was saved dense
        tab = table.detach().float().contiguous()
        if regions is not None:
            regions = regions.detach().contiguous()
        windows, nw, dev = qkv.numel() // (n * 3 * c), qkv.shape[-3], qkv.device
        with torch.cuda.device(dev):
            dqkv = torch.empty_like(qkv)
            dtable = torch.empty(tab.shape, dtype=torch.float32, device=dev)
            nbytes = _lib.value('dhd_window_attn_backward_scratch_bytes', windows, wh, ww, nh)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.call('dhd_window_attn_backward', _lib.ptr(qkv), _lib.ptr(dout), _lib.dtype_code(qkv.dtype), _lib.ptr(tab), _lib.ptr(regions),
                      _lib.ptr(dqkv), _lib.ptr(dtable), _lib.ptr(scratch), nbytes, windows, nw, wh, ww, nh, HEAD_DIM, float(scale),
                      _gemm_code(gemm), _lib.stream_ptr(dev))
        return dqkv, dtable.to(table.dtype).view(table.shape), None, None, None, None, None


@traced('dhd.swin.attn.train')
def window_attn(qkv, table, window_size, num_heads, scale, regions=None, gemm=None):
    """window_attn_infer with a backward: the same arguments and the same result, differentiable in `qkv` and `table`.  The
    forward is the inference operator and saves qkv, table and regions and nothing else; the backward is one call of
    dhd_window_attn_backward, which recomputes the softmax and returns dqkv in qkv's dtype and layout (what the qkv Linear's
    backward consumes, no permute back) and dtable in the table's dtype and shape.  dqkv is reproducible bit for bit, and so
    is dtable as far as tested (LDS float atomics into one copy per wave, see csrc/window_attn_bwd.hip).  Works under
    torch.autocast (half qkv, float32 table) and under checkpoint(..., use_reentrant=False).  The backward allocates dqkv, dtable and its scratch from the caching allocator."""
    return _WindowAttn.apply(qkv, table, regions, tuple(window_size), num_heads, scale, gemm)


class _CallableModule(types.ModuleType):
    """`dhd_amd.window_attn` names this module and, as the package's public interface, the function of the same name: calling the
    module calls the function, so `dhd_amd.window_attn(qkv, ...)` and `dhd_amd.window_attn.window_attn_infer` both hold."""
    __call__ = staticmethod(window_attn)


sys.modules[__name__].__class__ = _CallableModule
