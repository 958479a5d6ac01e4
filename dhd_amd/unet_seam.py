"""What a `UNet` does between its 3 x 3 convolutions, as HIP operators (csrc/unet_seam.h, capi_unet/dhd_amd_unet_seam.h):

  max_pool2x2             nn.MaxPool2d(2) of `_Down` without an index tensor: the backward recomputes the winner of each window
                          from x (alive anyway: it is the skip tensor) and writes every element of the gradient once
  conv_transpose2x2_cat   `_Up` with bilinear=False up to its double convolution: cat([x2, pad(conv_transpose2d(x1, w, b, 2))], 1)
                          in one launch that writes the concatenated tensor; neither the up-sampled nor the padded tensor exists

The pooling is torch's bit for bit, forward and backward (see max_pool2x2 for the one window where torch's own kernels disagree
with each other).  The up seam is a float32-accumulated MFMA product rounded once:
within the layer's bar of a float64 evaluation, not torch's bits, which is why `_Down.fused_seam` / `_Up.fused_seam` are opt-in
and routed by measurement.  The entry points are reached through _unet_seam.call(name, ...) / _unet_seam.value(name, ...)."""
import torch

from . import _lib, _unet_seam
from .trace import traced

_F32, _F16, _BF16 = torch.float32, torch.float16, torch.bfloat16

# Which (kind, channels, dtype, layout) entries the modules route to the operators: those where the operator beat today's calls,
# forward and forward + backward both, by more than the larger min-max spread of the two, at DHD-S's own shapes, 4 images
# (experiments/unet_seam_bench.py -> profiles/r25/unet_seam.json).  kind 'pool': channels of x; kind 'up': channels of x1.  The
# dtype is the one the seam computes in (the autocast dtype under autocast).  Medians in us per call, fused against today's
# calls, forward | forward + backward (the larger spread in brackets):
#   pool, every size and dtype: 20-22 / 13-17 (1-4) | 176-211 / 73-95 (5-85): a LOSS.  Every figure is the host's, not the
#     kernels': the times do not move between 64 @ 200 x 200 and 512 @ 25 x 25.  An autograd.Function and two ctypes calls cost
#     more on the host than torch's built-in node.  Not routed.
#   up 1024 @ 12 x 12:  float32 72 / 84 (7) | 375 / 274 (116);  fp16 43 / 61 (26) | 178 / 202 (123);  bf16 44 / 71 (58) | 164 / 210 (45)
#   up  512 @ 25 x 25:  float32 56 / 79 (9) | 172 / 236 (12);   fp16 42 / 60 (19) | 162 / 183 (10);   bf16 42 / 57 (3)  | 161 / 204 (9)
#   up  256 @ 50 x 50:  float32 50 / 89 (3) | 178 / 255 (5);    fp16 41 / 57 (3)  | 162 / 180 (6);    bf16 42 / 58 (4)  | 195 / 215 (64)
#   up  128 @ 100 x 100: float32 52 / 113 (2) | 268 / 274 (4);  fp16 41 / 77 (4)  | 227 / 184 (4);    bf16 40 / 77 (4)  | 227 / 210 (1)
# The up seam's forward wins at every size; forward + backward loses at 128 @ 100 x 100 in the half types (the gathered operand
# of the weight-gradient GEMM is 20 MB written and read again) and is inside the spread elsewhere.  An entry that is not listed
# was not measured and stays with torch; the operators themselves still take it when called directly.
ROUTED = {}
for _c in (64, 128, 256, 512):
    for _dt in (_F32, _F16, _BF16):
        ROUTED[('pool', _c, _dt, 'nhwc')] = False
for _c in (128, 256, 512, 1024):
    for _dt in (_F32, _F16, _BF16):
        ROUTED[('up', _c, _dt, 'nhwc')] = False
for _key in (('up', 512, _F32, 'nhwc'), ('up', 512, _BF16, 'nhwc'), ('up', 256, _F32, 'nhwc'), ('up', 256, _F16, 'nhwc'),
             ('up', 128, _F32, 'nhwc')):
    ROUTED[_key] = True
del _c, _dt, _key


def _nhwc(x):
    """True where the map's channels are the innermost axis in memory (a channels_last tensor or a view of one)."""
    return x.dim() == 4 and x.shape[1] > 1 and x.stride(1) == 1


def _fmt(nhwc):
    return torch.channels_last if nhwc else torch.contiguous_format


def _compute_dtype(x):
    return torch.get_autocast_dtype('cuda') if torch.is_autocast_enabled() and x.is_cuda else x.dtype


def unet_seam_supported(x, kind, x2=None, weight=None):
    """True when the operator of `kind` takes the tensors.  'pool': x a GPU map (B, C, H, W) of float32, float16 or bfloat16 with
    H, W >= 2, NCHW or channels_last (then C a multiple of 8).  'up': x the low map x1 (B, Cin, h, w) and x2 (B, C2, H, W) both
    channels_last on the GPU, H >= 2h and W >= 2w, weight (Cin, Cout, 2, 2); Cin a multiple of 32 up to 1024, Cout a multiple of
    16 up to 512, C2 a multiple of 8; x2 of the dtype the seam computes in (x1's, or the autocast dtype under autocast)."""
    if kind not in ('pool', 'up'):
        raise ValueError(f"unet_seam_supported: kind is 'pool' or 'up', not {kind!r}")
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.numel() > 0 and x.dtype in _lib.DTYPE_CODE):
        return False
    if kind == 'pool':
        B, C, H, W = x.shape
        return bool(_unet_seam.value('dhdn_max_pool2_supported', _lib.DTYPE_CODE[x.dtype], int(_nhwc(x)), B, C, H, W))
    if not (torch.is_tensor(x2) and torch.is_tensor(weight) and x2.is_cuda and weight.is_cuda and x2.dim() == 4 and weight.dim() == 4):
        return False
    dt = _compute_dtype(x)
    if dt not in _lib.DTYPE_CODE or x2.dtype != dt or weight.dtype not in _lib.DTYPE_CODE:
        return False
    (B, Cin, h, w), (B2, C2, H, W) = x.shape, x2.shape
    if B2 != B or tuple(weight.shape[:1] + weight.shape[2:]) != (Cin, 2, 2) or not (_nhwc(x) and _nhwc(x2)):
        return False
    return bool(_unet_seam.value('dhdn_up_cat_supported', _lib.DTYPE_CODE[dt], _unet_seam.NHWC, B, Cin, weight.shape[1], C2, h, w, H, W))


def unet_seam_routed(x, kind):
    """True when the measurement routed this (kind, channels, dtype, layout) to the operator (ROUTED)."""
    dt = x.dtype if kind == 'pool' else _compute_dtype(x)
    return bool(ROUTED.get((kind, x.shape[1], dt, 'nhwc' if _nhwc(x) else 'nchw'), False))


class _MaxPool2x2(torch.autograd.Function):
    """y = max over 2 x 2 windows; saves x (the dense tensor the kernel read) and nothing else."""

    @staticmethod
    @traced('dhd.unet.pool')
    def forward(ctx, x):
        nhwc = _nhwc(x)
        x = _lib.dense16(x.detach(), _fmt(nhwc))
        B, C, H, W = x.shape
        dev = x.device
        with torch.cuda.device(dev):
            y = torch.empty((B, C, H // 2, W // 2), dtype=x.dtype, device=dev, memory_format=_fmt(nhwc))
            _unet_seam.call('dhdn_max_pool2_forward', _lib.ptr(x), _lib.ptr(y), _lib.dtype_code(x.dtype), int(nhwc), B, C, H, W,
                            _lib.stream_ptr(dev))
        ctx.save_for_backward(x)
        ctx.nhwc = nhwc
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    @traced('dhd.unet.pool.backward')
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        nhwc = ctx.nhwc
        B, C, H, W = x.shape
        dev = x.device
        gy = _lib.dense16(gy, _fmt(nhwc))       # any view of a gradient
        with torch.cuda.device(dev):
            gx = torch.empty_like(x)
            _unet_seam.call('dhdn_max_pool2_backward', _lib.ptr(x), _lib.ptr(gy), _lib.ptr(gx), _lib.dtype_code(x.dtype), int(nhwc), B, C, H, W,
                            _lib.stream_ptr(dev))
        return gx


def max_pool2x2(x):
    """F.max_pool2d(x, 2) for a GPU map (B, C, H, W) of float32, float16 or bfloat16, NCHW or channels_last (C a multiple of 8),
    in x's dtype and layout; a last odd row / column is dropped.  Values and gradient are torch's bit for bit (ties keep the first
    element of the window in row-major order, a NaN wins; the gradient of an all -inf window goes to its first element, as torch
    does on the CPU and in NCHW on the device, where torch's channels_last device kernels drop it).  No index tensor: only x is kept for the backward, which recomputes the
    winners and writes each element of the gradient once, without a zero-fill pass and without atomics.  Works under autocast,
    checkpoint and graph capture; a view the kernels cannot read where it lies is copied first."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.DhdError(f'max_pool2x2: x must live on the GPU: dhd_amd runs only as HIP kernels (got {getattr(x, "device", type(x))})')
    if not unet_seam_supported(x, 'pool'):
        raise _lib.DhdError(f'max_pool2x2: no operator for a map {tuple(x.shape)} of {x.dtype} with strides {x.stride()}')
    return _MaxPool2x2.apply(x)


def _geom(x1, x2_shape, cout):
    B, Cin, h, w = x1.shape
    return (_lib.dtype_code(x1.dtype), _unet_seam.NHWC, B, Cin, cout, x2_shape[1], h, w, x2_shape[2], x2_shape[3])


class _ConvTranspose2x2Cat(torch.autograd.Function):
    """out = cat([x2, pad(conv_transpose2d(x1, weight, bias, stride=2))], 1); saves x1 and weight, not x2 and not the output."""

    @staticmethod
    @traced('dhd.unet.up')
    def forward(ctx, x1, x2, weight, bias):
        from .mghs_op import scratch_pool
        x1 = _lib.dense16(x1.detach(), torch.channels_last)
        x2 = _lib.dense16(x2.detach(), torch.channels_last)
        w = _lib.dense16(weight.detach())
        b = None if bias is None else _lib.dense16(bias.detach().float())
        cout, dev = w.shape[1], x1.device
        geom = _geom(x1, x2.shape, cout)
        with torch.cuda.device(dev):
            out = torch.empty((x2.shape[0], x2.shape[1] + cout, x2.shape[2], x2.shape[3]), dtype=x1.dtype, device=dev,
                              memory_format=torch.channels_last)
            nbytes = _unet_seam.value('dhdn_up_cat_scratch_bytes', geom[0], geom[2], geom[3], cout, geom[6], geom[7], 0)
            scratch = scratch_pool.get(dev, nbytes, 'unet_up')
            _unet_seam.call('dhdn_up_cat_forward', _lib.ptr(x1), _lib.ptr(x2), _lib.ptr(w), _lib.dtype_code(w.dtype), _lib.ptr(b), _lib.ptr(out),
                            _lib.ptr(scratch), nbytes, *geom, _lib.stream_ptr(dev))
        ctx.save_for_backward(x1, weight)
        ctx.x2_shape = tuple(x2.shape)
        ctx.bias_dtype = None if bias is None else bias.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @traced('dhd.unet.up.backward')
    def backward(ctx, gout):
        from .mghs_op import scratch_pool
        x1, weight = ctx.saved_tensors
        need_x2, need_w, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.bias_dtype is not None and ctx.needs_input_grad[3]
        gout = _lib.dense16(gout, torch.channels_last)
        w = _lib.dense16(weight.detach())
        cout, dev = w.shape[1], x1.device
        geom = _geom(x1, ctx.x2_shape, cout)
        B, Cin, h, wd = x1.shape
        with torch.cuda.device(dev):
            gx1 = torch.empty_like(x1)
            gx2 = torch.empty(ctx.x2_shape, dtype=x1.dtype, device=dev, memory_format=torch.channels_last) if need_x2 else None
            gop = torch.empty((B * h * wd, 4 * cout), dtype=x1.dtype, device=dev) if need_w else None
            dbias = torch.empty(cout, dtype=torch.float32, device=dev) if need_b else None
            nbytes = _unet_seam.value('dhdn_up_cat_scratch_bytes', geom[0], geom[2], geom[3], cout, geom[6], geom[7], 1)
            scratch = scratch_pool.get(dev, nbytes, 'unet_up_bwd')
            _unet_seam.call('dhdn_up_cat_backward', _lib.ptr(gout), _lib.ptr(w), _lib.dtype_code(w.dtype), _lib.ptr(gx1), _lib.ptr(gx2),
                            _lib.ptr(gop), _lib.ptr(dbias), _lib.ptr(scratch), nbytes, *geom, _lib.stream_ptr(dev))
        gw = None
        if need_w:      # the reduction over all pixels stays with torch's GEMM, on the operand the kernel wrote
            gw = torch.mm(x1.permute(0, 2, 3, 1).reshape(B * h * wd, Cin).t(), gop)
            gw = gw.view(Cin, 4, cout).permute(0, 2, 1).reshape(Cin, cout, 2, 2).to(weight.dtype)
        return gx1, gx2, gw, (dbias.to(ctx.bias_dtype) if need_b else None)


def conv_transpose2x2_cat(x1, x2, weight, bias=None):
    """cat([x2, F.pad(F.conv_transpose2d(x1, weight, bias, stride=2), pads)], 1) as `_Up.forward` computes it, for channels_last
    GPU maps x1 (B, Cin, h, w) and x2 (B, C2, H, W) with H >= 2h, W >= 2w and weight (Cin, Cout, 2, 2): the pads are diff // 2
    before and the rest after, the border zero (no bias there).  Under torch.autocast x1 is cast to the autocast dtype, as the
    module's convolution does; x2 must have the dtype the seam computes in.  One launch writes the (B, C2 + Cout, H, W)
    channels_last result -- the product on the MFMA with float32 accumulation (float32 tensors as three bfloat16 products), the
    bias added in float32, one rounding, x2 copied beside it -- after a launch that packs the weight.  Differentiable in all four
    inputs: the backward reads the gradient once, writes x2's gradient dense, x1's through the MFMA, the bias gradient from
    per-workgroup partial rows in a fixed order (no atomics), and, only where the weight requires a gradient, the gathered
    operand of torch's weight-gradient GEMM.  Saves x1 and weight.  Works under checkpoint and graph capture (scratch comes from
    the pool); a view the kernels cannot read where it lies is copied first."""
    for name, t in (('x1', x1), ('x2', x2), ('weight', weight)):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.DhdError(f'conv_transpose2x2_cat: {name} must live on the GPU: dhd_amd runs only as HIP kernels '
                                f'(got {getattr(t, "device", type(t))})')
    if not unet_seam_supported(x1, 'up', x2, weight):
        raise _lib.DhdError(f'conv_transpose2x2_cat: no operator for x1 {tuple(x1.shape)} of {x1.dtype}, x2 {tuple(x2.shape)} of {x2.dtype}, '
                            f'weight {tuple(weight.shape)} (channels_last maps of one dtype; see unet_seam_supported)')
    dt = _compute_dtype(x1)
    return _ConvTranspose2x2Cat.apply(x1.to(dt), x2, weight, bias)
