"""Deformable convolution at inference as one HIP operator (csrc/deform_conv.hip, section 15 of include/dhd_amd.h): the
bilinear sampling of `DCN` and the grouped product with its weight in one kernel.  The column matrix (B, C * 9, H * W) that
the training path writes for its backward pass (depthnet._DeformIm2col, 78-155 MB at the DHD-S HeightNet size) does not exist;
x is read where it lies, NCHW or channels_last, float32 / float16 / bfloat16, and `out` comes back in the same dtype and
memory format.  deform_conv_infer is forward only, with no autograd node; deform_conv below is the same forward with a HIP
backward (csrc/deform_conv_train.h).

The entry points are reached through _lib.call(name, ...), the one spelling of a library call by name."""
import ctypes as C
import sys
import types

import torch

from . import _deform_train, _lib
from .trace import traced


def _layout_of(x):
    """0 = NCHW, 1 = channels_last, None = neither (the caller makes it contiguous)."""
    if x.is_contiguous():
        return 0
    if x.is_contiguous(memory_format=torch.channels_last):
        return 1
    return None


def _gemm_code(gemm):
    return _lib.SFA_GEMM[gemm or 'default']


def deform_conv_infer_supported(x, weight, groups, gemm=None):
    """True when deform_conv_infer takes this call: a GPU tensor (B, C, H, W) of a dtype, and a 3x3 weight (O, C / groups, 3, 3) of
    channel counts, that the kernel has."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in _lib.DTYPE_CODE and weight.dim() == 4):
        return False
    c, (o, cg, kh, kw) = x.shape[1], weight.shape
    if kh != kw or groups < 1 or c % groups or o % groups or cg * groups != c:
        return False
    layout = _layout_of(x)
    fn = getattr(_lib.load(), 'dhd_deform_conv_infer_supported')
    return bool(fn(c, o, groups, kh, max(x.shape[2], 1), max(x.shape[3], 1), _lib.DTYPE_CODE[x.dtype], 0 if layout is None else layout,
                   _gemm_code(gemm)))


@traced('dhd.dcn.infer')
def deform_conv_infer(x, offset, weight, padding=1, dilation=1, groups=1, gemm=None):
    """x (B, C, H, W) float32 / float16 / bfloat16, NCHW or channels_last; offset (B, 18, H, W), channel 2t = dy and 2t + 1 = dx
    of tap t; weight (O, C / groups, 3, 3).  Returns out (B, O, H, W) in x's dtype and memory format.  A view the kernel cannot
    read where it lies -- strided, or dense at an address that is not a multiple of 16 bytes -- is copied first; offset and
    weight are used as float32 dense tensors.  Scratch comes from the pool; nothing is kept between calls."""
    if not (x.is_cuda and offset.is_cuda and weight.is_cuda):
        raise _lib.DhdError(f'deform_conv_infer: x, offset and weight must live on the GPU (got {x.device}, {offset.device}, {weight.device})')
    x = x.detach()
    layout = _layout_of(x)
    if layout is None:
        x, layout = x.contiguous(), 0
    if x.data_ptr() % 16:     # 16-byte corner runs: a dense view at an odd storage offset is copied, in its layout
        x = x.clone(memory_format=torch.preserve_format)
    b, c, h, w = x.shape
    weight = _lib.require_gpu_tensor(weight.detach().float().contiguous(), torch.float32, 'DCN weight')
    offset = _lib.require_gpu_tensor(offset.detach().float().contiguous(), torch.float32, 'DCN offsets')
    o, cg, k, _ = weight.shape
    if cg * groups != c or tuple(offset.shape) != (b, 2 * k * k, h, w):
        raise _lib.DhdError('deform_conv_infer: inconsistent shapes of x, offset and weight')
    code = _lib.dtype_code(x.dtype)
    dev = x.device
    with torch.cuda.device(dev):
        nscratch = C.c_size_t()
        _lib.call('dhd_deform_conv_infer_scratch_bytes', b, c, o, groups, k, h, w, code, layout, C.byref(nscratch))
        from .mghs_op import scratch_pool
        scratch = scratch_pool.get(dev, nscratch.value, 'deform_conv')
        out = torch.empty((b, o, h, w), dtype=x.dtype, device=dev,
                          memory_format=torch.channels_last if layout else torch.contiguous_format)
        _lib.call('dhd_deform_conv_infer', _lib.ptr(x), code, layout, _lib.ptr(offset), _lib.ptr(weight), _lib.ptr(out), b, c, o, groups,
                  h, w, k, padding, dilation, _gemm_code(gemm), _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr(dev))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Training: the inference operator as the forward, a HIP backward without column gradients (csrc/deform_conv_train.h)

# Which (x dtype, layout) entries `DCN.fused_train` routes to `deform_conv` (layout 0 = NCHW, 1 = channels_last): True only where
# forward + backward, the weight packs and torch's dW GEMM included, beat today's path (depthnet._DeformIm2col + torch.matmul) by
# more than the larger min-max spread of the two at (24, 256, 256, g = 4, 16, 44) (experiments/dcn_train_bench.py ->
# profiles/r21/dcn_train.json).  Medians in us per forward + backward, fused against today (larger min-max spread of the two);
# x under autocast is in the autocast type:
#   float32        NCHW 738 against 911 (17),  channels_last 711 against 932 (17)
#   fp16 autocast  NCHW 503 against 610 (21),  channels_last 505 against 639 (12)
#   bf16 autocast  NCHW 496 against 610 (16),  channels_last 501 against 637 (14)
# The forward alone: 126 / 113 / 79 / 68 / 77 / 65 against 201 / 225 / 152 / 177 / 152 / 177.  Every entry wins by more than the
# spread; most of the margin is the forward's: the two backward launches, the sort and the dW GEMM together take 424 us where
# today's backward takes 458 (fp16 NCHW, by subtraction).  Held between forward and backward on top of x: the output alone, 16.5 MiB in
# float32 and 8.2 MiB in half, against 179 and 106 MiB; peak of one step 198 against 342 MiB and 99 against 187 MiB.
ROUTED_TRAIN = {
    (torch.float32, 0): True, (torch.float32, 1): True,
    (torch.float16, 0): True, (torch.float16, 1): True,
    (torch.bfloat16, 0): True, (torch.bfloat16, 1): True,
}


def _train_layout(x):
    """The layout deform_conv runs x in: its own where it is dense, else NCHW (deform_conv_infer's rule)."""
    layout = _layout_of(x)
    return 0 if layout is None else layout


def deform_conv_train_supported(x, weight, groups):
    """True when `deform_conv` itself takes this call: what deform_conv_infer takes with the default GEMM mode, on a map of at most
    853 cells (the backward sorts one image's taps by (cell, tap) in LDS; DHD-S's 16 x 44 has 704)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in _lib.DTYPE_CODE and torch.is_tensor(weight) and weight.dim() == 4):
        return False
    c, (o, cg, kh, kw) = x.shape[1], weight.shape
    if kh != kw or groups < 1 or c % groups or o % groups or cg * groups != c:
        return False
    return bool(_deform_train.value('dhdd_deform_conv_backward_supported', c, o, groups, kh, max(x.shape[2], 1), max(x.shape[3], 1),
                                    _lib.DTYPE_CODE[x.dtype], _train_layout(x), 0))


def deform_conv_train_routed(x, weight, groups):
    """True when a `DCN` with `fused_train` on sends `x` (in its compute dtype) to `deform_conv`: the operator takes it and the
    measurement routed that (dtype, layout) to it (ROUTED_TRAIN)."""
    return deform_conv_train_supported(x, weight, groups) and ROUTED_TRAIN.get((x.dtype, _train_layout(x)), False)


def deform_conv_backward(x, offset, weight, gout, padding=1, dilation=1, groups=1, want_col=True):
    """One dhdd_deform_conv_backward call on dense, 16-byte aligned GPU tensors: x (B, C, H, W) and gout (B, O, H, W) of one dtype,
    each NCHW or channels_last; offset (B, 18, H, W) and weight (O, C / groups, 3, 3) float32 -> (dx, doffset, col): dx in x's dtype
    and layout, doffset float32, and with `want_col` the operand of dW, col (B, C * 9, H * W) in x's dtype -- the bytes
    dhd_deform_im2col_t writes -- else None (the kernel then does not write it).  Scratch comes from the pool."""
    b, c, h, w = x.shape
    o, cg, k, _ = weight.shape
    xl, gl = _layout_of(x), _layout_of(gout)
    if xl is None or gl is None or gout.dtype != x.dtype or tuple(gout.shape) != (b, o, h, w):
        raise _lib.DhdError('deform_conv_backward: x and gout must be dense, NCHW or channels_last, of one dtype, and gout of the output shape')
    code, dev = _lib.dtype_code(x.dtype), x.device
    with torch.cuda.device(dev):
        nscratch = C.c_size_t()
        _deform_train.call('dhdd_deform_conv_backward_scratch_bytes', b, c, o, groups, k, h, w, code, xl, gl, C.byref(nscratch))
        from .mghs_op import scratch_pool
        scratch = scratch_pool.get(dev, nscratch.value, 'deform_conv_bwd')
        dx = torch.empty_like(x)                              # preserve_format: x's own layout
        doffset = torch.empty_like(offset)
        col = torch.empty((b, c * k * k, h * w), dtype=x.dtype, device=dev) if want_col else None
        _deform_train.call('dhdd_deform_conv_backward', _lib.ptr(x), code, xl, _lib.ptr(offset), _lib.ptr(weight), _lib.ptr(gout), gl,
                           _lib.ptr(dx), _lib.ptr(doffset), _lib.ptr(col), b, c, o, groups, h, w, k, padding, dilation, _lib.ptr(scratch),
                           scratch.numel(), _lib.stream_ptr(dev))
    return dx, doffset, col


class _DeformConvTrain(torch.autograd.Function):
    """out = W . bilinear columns of x; saves the dense x, the float32 offsets and the weight, and nothing of column size."""

    @staticmethod
    def forward(ctx, x, offset, weight, padding, dilation, groups):
        xd = x.detach()
        layout = _train_layout(xd)
        xd = _lib.dense16(xd, torch.channels_last if layout else torch.contiguous_format)
        off = offset.detach().float().contiguous()
        wgt = weight.detach().float().contiguous()
        out = deform_conv_infer(xd, off, wgt, padding, dilation, groups)
        ctx.save_for_backward(xd, off, wgt)
        ctx.args = (padding, dilation, groups, offset.dtype, weight.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @traced('dhd.dcn.train')
    def backward(ctx, gout):
        x, off, wgt = ctx.saved_tensors
        padding, dilation, groups, off_dtype, w_dtype = ctx.args
        need = ctx.needs_input_grad
        g = gout.to(x.dtype)
        gl = _layout_of(g)                                    # a strided or misaligned gradient is copied
        g = _lib.dense16(g, torch.channels_last if gl == 1 else torch.contiguous_format)
        with torch.autocast('cuda', enabled=False):
            dx, doff, col = deform_conv_backward(x, off, wgt, g, padding, dilation, groups, want_col=need[2])
            dw = None
            if need[2]:
                b, c, h, w = x.shape
                o = wgt.shape[0]
                # dW[g, o, (c, t)] = sum over images and pixels of gout col: one product per image in the GEMM type, summed in float32
                per = torch.matmul(g.reshape(b, groups, o // groups, h * w), col.view(b, groups, (c // groups) * 9, h * w).transpose(-1, -2))
                dw = (per[0].float() if b == 1 else per.sum(0, dtype=torch.float32)).reshape(wgt.shape).to(w_dtype)
        return dx if need[0] else None, doff.to(off_dtype) if need[1] else None, dw, None, None, None


def deform_conv(x, offset, weight, padding=1, dilation=1, groups=1):
    """Deformable convolution (DCN v1, 3 x 3, stride 1, one deformable group), differentiable in x, offset and weight: x (B, C, H, W)
    float32 / float16 / bfloat16, NCHW or channels_last; offset (B, 18, H, W); weight (O, C / groups, 3, 3).  Returns out
    (B, O, H, W) in x's dtype and memory format -- the bytes of deform_conv_infer.

    The forward saves the dense x, the offsets and the weight as float32, and nothing of column size.  The backward is one
    dhdd_deform_conv_backward call: dx in x's dtype and layout, doffset, and -- where the weight wants a gradient -- the recomputed
    columns in x's dtype, from which torch's GEMM takes dW, summed over the batch in float32.  The column gradient never exists.
    The GEMMs run in x's type (float32: bf16x3 split products; a half type: its own, float32 accumulation).  No atomics on
    results: a repeated call gives the same bytes.  Works under torch.autocast (x selects the type), under checkpoint and inside a
    captured HIP graph once the scratch pool holds the call's size.  HIP only: a CPU tensor or an unsupported shape raises DhdError."""
    if not (torch.is_tensor(x) and x.is_cuda and torch.is_tensor(offset) and offset.is_cuda and torch.is_tensor(weight) and weight.is_cuda):
        raise _lib.DhdError('deform_conv: x, offset and weight must live on the GPU: dhd_amd runs only as HIP kernels')
    if not deform_conv_train_supported(x, weight, groups):
        raise _lib.DhdError(f'deform_conv: no operator for x {tuple(x.shape)} of {x.dtype} with weight {tuple(weight.shape)} in {groups} groups')
    return _DeformConvTrain.apply(x, offset, weight, padding, dilation, groups)


class _CallableModule(types.ModuleType):
    """`dhd_amd.deform_conv` names this module and, as the package's public interface, the function of the same name: calling the
    module calls the function, so `dhd_amd.deform_conv(x, ...)` and `dhd_amd.deform_conv.deform_conv_infer` both hold."""
    __call__ = staticmethod(deform_conv)


sys.modules[__name__].__class__ = _CallableModule
