"""Deformable convolution at inference as one HIP operator (csrc/deform_conv.hip, section 15 of include/dhd_amd.h): the
bilinear sampling of `DCN` and the grouped product with its weight in one kernel.  The column matrix (B, C * 9, H * W) that
the training path writes for its backward pass (depthnet._DeformIm2col, 78-155 MB at the DHD-S HeightNet size) does not exist;
x is read where it lies, NCHW or channels_last, float32 / float16 / bfloat16, and `out` comes back in the same dtype and
memory format.  Forward only: no autograd node.

The entry points are reached through _lib.call(name, ...), the one spelling of a library call by name."""
import ctypes as C

import torch

from . import _lib
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
