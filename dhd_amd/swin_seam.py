"""The seams between the stages of the Swin backbone as HIP operators (csrc/swin_seam.h, include/dhd_amd_seam.h):

  patch_merge_norm   what `PatchMerging` does before its Linear: the 2 x 2 gather into nn.Unfold's channel order with the
                     LayerNorm over the 4C gathered values in it, emitting the dtype the Linear reads
  patch_embed_norm   what `PatchEmbed` does after its conv: LayerNorm over the channels of the NCHW map, written as tokens; the
                     transposition happens inside the kernel

Both are differentiable and save x, weight and bias and nothing else: the backward recomputes the row statistics from x and
sums the weight and bias gradients without atomics, so dx, dweight and dbias are reproducible bit for bit.  The statistics are
float32 (mean, then the centred sum of squares): within the layer's 1e-4 bar of a float64 LayerNorm, not torch's bits, which is
why `PatchMerging.fused_seam` / `PatchEmbed.fused_seam` are opt-in.

The entry points are reached through _seam.call(name, ...) / _seam.value(name, ...)."""
import torch

from . import _lib, _seam
from .trace import traced

_F32, _F16, _BF16 = torch.float32, torch.float16, torch.bfloat16

# Which (kind, C, x dtype, result dtype) entries the modules route to the operators: those where the fused path beat today's
# path, forward and forward + backward both, by more than the larger min-max spread of the two at DHD-L's map of that C, 12
# images (experiments/swin_seam_bench.py -> profiles/r15/swin_seam.json).  Medians in us per call, fused against today's path,
# forward | forward + backward (the larger spread in brackets):
#   merge, C = 128, 128 x 352:  float32 135 / 303 (50) | 419 / 816 (74);  bf16 autocast 82 / 377 (64) | 335 / 955 (3);
#                               fp16 autocast 80 / 369 (24) | 337 / 960 (9);  bf16 tokens 116 / 418 (14) | 342 / 1060 (7)
#   merge, C = 256, 64 x 176:   float32 74 / 118 (8) | 265 / 368 (10);  bf16 autocast 40 / 157 (10) | 269 / 430 (54);
#                               fp16 autocast 40 / 160 (4) | 248 / 431 (131);  bf16 tokens 61 / 178 (10) | 257 / 480 (43)
#   merge, C = 512, 32 x 88:    float32 39 / 54 (5) | 252 / 204 (35);  bf16 autocast 38 / 69 (15) | 243 / 230 (28);
#                               fp16 autocast 29 / 70 (9) | 241 / 230 (26);  bf16 tokens 36 / 84 (5) | 259 / 255 (34)
#   embed, C = 128, 128 x 352:  float32 137 / 907 (20) | 407 / 2146 (12);  bf16 conv output 104 / 977 (4) | 360 / 2276 (62);
#                               fp16 conv output 125 / 983 (17) | 336 / 2281 (32)
# At C = 512 the forward wins but forward + backward does not (the backward's time barely falls with the map, about 210 us at
# 8 448 rows against 255 us at 135 168; its fixed part was not profiled): False, the stage-2 merge stays with torch.  An entry that is not listed (fp16 tokens, other channel counts) was not
# measured and stays with torch as well; the operators themselves still take it when called directly.
ROUTED = {
    ('merge', 128, _F32, _F32): True, ('merge', 128, _F32, _BF16): True, ('merge', 128, _F32, _F16): True, ('merge', 128, _BF16, _BF16): True,
    ('merge', 256, _F32, _F32): True, ('merge', 256, _F32, _BF16): True, ('merge', 256, _F32, _F16): True, ('merge', 256, _BF16, _BF16): True,
    ('merge', 512, _F32, _F32): False, ('merge', 512, _F32, _BF16): False, ('merge', 512, _F32, _F16): False, ('merge', 512, _BF16, _BF16): False,
    ('embed', 128, _F32, _F32): True, ('embed', 128, _BF16, _F32): True, ('embed', 128, _F16, _F32): True,
}


def swin_seam_supported(x, kind, out_dtype=None):
    """True when the operator of `kind` ('merge': x a token map (..., C); 'embed': x an NCHW map (B, C, H, W)) takes x and emits
    `out_dtype` (default x's): a GPU tensor of float32, float16 or bfloat16, C a multiple of 8, up to 512 for 'merge' (4C <= 2048)
    and up to 256 for 'embed'."""
    if kind not in ('merge', 'embed'):
        raise ValueError(f"swin_seam_supported: kind is 'merge' or 'embed', not {kind!r}")
    if not (torch.is_tensor(x) and x.is_cuda and x.numel() > 0 and x.dtype in _lib.DTYPE_CODE):
        return False
    out_dtype = out_dtype or x.dtype
    if out_dtype not in _lib.DTYPE_CODE or x.dim() < (4 if kind == 'embed' else 2) or (kind == 'embed' and x.dim() != 4):
        return False
    C = x.shape[1] if kind == 'embed' else x.shape[-1]
    return bool(_seam.value(f'dhds_{kind}_norm_supported', C, _lib.DTYPE_CODE[x.dtype], _lib.DTYPE_CODE[out_dtype]))


def swin_seam_routed(x, kind, out_dtype=None):
    """True when the measurement routed this (kind, C, x dtype, result dtype) to the operator (ROUTED)."""
    C = x.shape[1] if kind == 'embed' else x.shape[-1]
    return bool(ROUTED.get((kind, C, x.dtype, out_dtype or x.dtype), False))


def _affine(p, n, name, op):
    p = p.detach().float().contiguous()
    if tuple(p.shape) != (n,):
        raise _lib.DhdError(f'{op}: {name} must have shape ({n},), got {tuple(p.shape)}')
    return _lib.dense16(p)


def _backward_call(kind, x, dy, weight, n, rows, dims, eps):
    """dx, dgamma, dbeta of either operator: x dense as the forward read it, dy made dense, n the normalised length."""
    dev = x.device
    dy = _lib.dense16(dy)       # a strided, expanded or misaligned gradient is copied; x was saved dense
    gamma = _affine(weight, n, 'weight', f'patch_{kind}_norm')
    with torch.cuda.device(dev):
        dx = torch.empty_like(x)
        dgamma = torch.empty(n, dtype=torch.float32, device=dev)
        dbeta = torch.empty(n, dtype=torch.float32, device=dev)
        nbytes = _seam.value(f'dhds_{kind}_norm_backward_scratch_bytes', rows, n // 4 if kind == 'merge' else n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _seam.call(f'dhds_{kind}_norm_backward', _lib.ptr(x), _lib.ptr(dy), _lib.ptr(gamma), _lib.ptr(dx), _lib.ptr(dgamma), _lib.ptr(dbeta),
                   _lib.ptr(scratch), nbytes, _lib.dtype_code(x.dtype), _lib.dtype_code(dy.dtype), *dims, float(eps), _lib.stream_ptr(dev))
    return dx, dgamma, dbeta


class _PatchMergeNorm(torch.autograd.Function):
    """out = LN(gather(x)); saves x (the dense tensor the kernel read), weight and bias."""

    @staticmethod
    @traced('dhd.swin.seam.merge')
    def forward(ctx, x, weight, bias, eps, hw_shape, out_dtype):
        x = _lib.dense16(x.detach())
        (H, W), B, C, dev = hw_shape, x.shape[0], x.shape[-1], x.device
        if x.dim() not in (3, 4) or x.numel() != B * H * W * C:
            raise _lib.DhdError(f'patch_merge_norm: x {tuple(x.shape)} is not a (B, {H} x {W}, C) token map')
        gamma, beta = _affine(weight, 4 * C, 'weight', 'patch_merge_norm'), _affine(bias, 4 * C, 'bias', 'patch_merge_norm')
        with torch.cuda.device(dev):
            out = torch.empty((B, -(-H // 2) * -(-W // 2), 4 * C), dtype=out_dtype, device=dev)
            _seam.call('dhds_merge_norm_forward', _lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(out), _lib.dtype_code(x.dtype),
                       _lib.dtype_code(out_dtype), B, H, W, C, float(eps), _lib.stream_ptr(dev))
        ctx.save_for_backward(x, weight, bias)
        ctx.args = (eps, hw_shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @traced('dhd.swin.seam.merge.backward')
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        eps, (H, W) = ctx.args
        B, C = x.shape[0], x.shape[-1]
        dx, dgamma, dbeta = _backward_call('merge', x, dy, weight, 4 * C, B * -(-H // 2) * -(-W // 2), (B, H, W, C), eps)
        return dx, dgamma.to(weight.dtype), dbeta.to(bias.dtype), None, None, None


def patch_merge_norm(x, weight, bias, eps, hw_shape, out_dtype=None):
    """The input of `PatchMerging.reduction`: x a (B, H * W, C) or (B, H, W, C) token map with hw_shape = (H, W); the result is
    (B, ceil(H / 2) * ceil(W / 2), 4C), row (i, j) the LayerNorm (weight, bias of length 4C, float32 statistics) of the 2 x 2
    neighbourhood x[2i : 2i + 2, 2j : 2j + 2] in nn.Unfold's channel order 4 c + 2 kh + kw.  A neighbour past H or W is a zero
    that enters the statistics, as in the reference, which pads before this norm.  out_dtype (default x's) may be any of
    float32, float16, bfloat16; a half result is the float32 result rounded once.  Differentiable in x, weight and bias; works
    under torch.autocast (the dtypes are the caller's), under checkpoint(use_reentrant=False) and under graph capture.  A view
    the kernels cannot read where it lies is copied first.  The forward allocates the result; the backward dx, the two parameter
    gradients and its scratch, all from the caching allocator."""
    if not (torch.is_tensor(x) and x.is_cuda and weight.is_cuda and bias.is_cuda):
        raise _lib.DhdError(f'patch_merge_norm: x, weight and bias must live on the GPU: dhd_amd runs only as HIP kernels '
                            f'(got {x.device}, {weight.device}, {bias.device})')
    out_dtype = out_dtype or x.dtype
    if not swin_seam_supported(x, 'merge', out_dtype):
        raise _lib.DhdError(f'patch_merge_norm: no operator for tokens {tuple(x.shape)} of {x.dtype} into {out_dtype}')
    return _PatchMergeNorm.apply(x, weight, bias, float(eps), tuple(int(v) for v in hw_shape), out_dtype)


class _PatchEmbedNorm(torch.autograd.Function):
    """out = LN over the channels of x (B, C, H, W), as tokens; saves x (the dense NCHW tensor the kernel read), weight and bias."""

    @staticmethod
    @traced('dhd.swin.seam.embed')
    def forward(ctx, x, weight, bias, eps, out_dtype):
        x = _lib.dense16(x.detach())
        B, C, H, W = x.shape
        dev = x.device
        gamma, beta = _affine(weight, C, 'weight', 'patch_embed_norm'), _affine(bias, C, 'bias', 'patch_embed_norm')
        with torch.cuda.device(dev):
            out = torch.empty((B, H * W, C), dtype=out_dtype, device=dev)
            _seam.call('dhds_embed_norm_forward', _lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(out), _lib.dtype_code(x.dtype),
                       _lib.dtype_code(out_dtype), B, C, H * W, float(eps), _lib.stream_ptr(dev))
        ctx.save_for_backward(x, weight, bias)
        ctx.eps = eps
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @traced('dhd.swin.seam.embed.backward')
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        B, C, H, W = x.shape
        dx, dgamma, dbeta = _backward_call('embed', x, dy, weight, C, B * H * W, (B, C, H * W), ctx.eps)
        return dx, dgamma.to(weight.dtype), dbeta.to(bias.dtype), None, None


def patch_embed_norm(x, weight, bias, eps, out_dtype=None):
    """`x.flatten(2).transpose(1, 2)` followed by LayerNorm (weight, bias of length C, float32 statistics) for x (B, C, H, W), the
    patch convolution's output as it lies: the result is the (B, H * W, C) token map in out_dtype (default x's; any of float32,
    float16, bfloat16; a half result is the float32 result rounded once).  The transposition happens inside the kernel, through
    LDS: no intermediate tensor is written.  Where x is dense in channels_last memory its token view is already contiguous and
    goes to `layer_norm_rows` as it lies, without a copy and without the kernel here.  Differentiable in x, weight and bias
    (dx has x's layout and dtype); works under torch.autocast, under checkpoint(use_reentrant=False) and under graph capture.
    Any other view is made dense first.  The forward allocates the result; the backward dx, the two parameter gradients and its
    scratch, all from the caching allocator."""
    if not (torch.is_tensor(x) and x.is_cuda and weight.is_cuda and bias.is_cuda):
        raise _lib.DhdError(f'patch_embed_norm: x, weight and bias must live on the GPU: dhd_amd runs only as HIP kernels '
                            f'(got {x.device}, {weight.device}, {bias.device})')
    out_dtype = out_dtype or x.dtype
    if not swin_seam_supported(x, 'embed', out_dtype):
        raise _lib.DhdError(f'patch_embed_norm: no operator for a map {tuple(x.shape)} of {x.dtype} into {out_dtype}')
    if not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last):
        from .swin_glue import layer_norm_rows
        B, C, H, W = x.shape
        return layer_norm_rows(x.permute(0, 2, 3, 1).reshape(B, H * W, C), weight, bias, eps, out_dtype)
    return _PatchEmbedNorm.apply(x, weight, bias, float(eps), out_dtype)
