"""The second half of a Swin block at inference as one HIP operator (csrc/swin_ffn.hip, include/dhd_amd_ffn.h for C = 128 and
256; csrc/swin_ffn_wide.h, include/dhd_amd_ffn_wide.h for C = 512 and 1024):

    swin_ffn_infer(x, norm_weight, norm_bias, eps, w1, b1, w2, b2) = x + fc2(gelu(fc1(layer_norm(x))))

x is read once (the wide family: twice) and the result written once; the normalised rows and the two (tokens x 4C) hidden tensors never exist.  Forward
only: nothing is saved and nothing is differentiable, which is why `SwinBlock.fused_ffn` routes to it only in eval mode with
nothing to differentiate.  The entry points are reached through _ffn.call(name, ...) / _ffn.value(name, ...), or the same two
of _ffn_wide: the functions here dispatch on C to the family that takes it.

In training the same half, with its DropPath, is `swin_ffn` (csrc/swin_ffn_train.h, include/dhd_amd_ffn_train.h for C = 128 and
256; csrc/swin_ffn_wide_train.h, dhd_amd/include/dhd_amd_ffn_wide_train.h for C = 512): an autograd function whose forward saves
the tokens and nothing of the hidden tensors and whose backward recomputes them in one HIP call, `SwinBlock.fused_ffn_train`'s
route (`SwinBlock.fused_ffn_train_wide`'s at C = 512).  C = 1024 has no training operator."""
import sys
import types

import torch

from . import _ffn, _ffn_train, _ffn_wide, _ffn_wide_train, _lib
from .trace import traced

_F32, _F16, _BF16 = torch.float32, torch.float16, torch.bfloat16

# Which (C, x dtype, GEMM dtype) entries `swin_ffn_supported` routes to the operator: those where the fused call, weight pack
# included, beat BOTH parent forms (torch's norm2 + FFN, and the same with fused_glue's norm2) by more than the run-to-run spread
# of any of the three at DHD-L's stage shape of that C (experiments/swin_ffn_infer_bench.py -> profiles/r13/swin_ffn_infer.json).
# Medians in us per call, fused against the better parent (largest min-max spread of the three paths):
#   C = 128, 540 672 rows: bf16 autocast 479 against 787 (28), fp16 autocast 474 against 798 (33), float32 590 against 1833 (45)
#   C = 256, 135 168 rows: bf16 autocast 296 against 460 (103), fp16 autocast 301 against 450 (73), float32 528 against 1447 (86)
# The half-model combinations (half tokens) were not measured: False, they stay with torch; the operator itself still takes them
# when called directly.
ROUTED = {
    (128, _F32, _BF16): True, (128, _F32, _F16): True, (128, _F32, _F32): True,
    (256, _F32, _BF16): True, (256, _F32, _F16): True, (256, _F32, _F32): True,
    (128, _BF16, _BF16): False, (128, _F16, _F16): False, (256, _BF16, _BF16): False, (256, _F16, _F16): False,
}

# The same rule for the wide family (C = 512, 1024: DHD-L's stages 2 and 3), measured at 33 792 x 512 and 8 448 x 1024 by
# experiments/swin_ffn_wide_bench.py -> profiles/r14/swin_ffn_wide_infer.json.  Medians in us per call, fused against the better
# parent (largest min-max spread of the three paths); "bf16 tokens" is the residual stream in the autocast type under autocast,
# which is what DHD-L's backbone hands these stages (PatchMerging's Linear returns the autocast type):
#   C = 512, 33 792 rows: bf16 autocast 253 against 300 (31), fp16 autocast 259 against 304 (31), float32 533 against 1248 (88),
#                         bf16 tokens 236 against 288 (20), fp16 tokens 246 against 287 (23)
#   C = 1024, 8 448 rows: bf16 autocast 247 against 222 (38), fp16 autocast 247 against 228 (22), float32 734 against 1203 (76),
#                         bf16 tokens 238 against 216 (19), fp16 tokens 241 against 220 (32)
# At C = 1024 the half GEMMs lose (132 workgroups of 64 rows on 256 CUs): False, they stay with torch; the operator itself still
# takes them when called directly.  A half model without autocast shares the half-token entries and was not timed on its own.
ROUTED_WIDE = {
    (512, _F32, _BF16): True, (512, _F32, _F16): True, (512, _F32, _F32): True,
    (1024, _F32, _BF16): False, (1024, _F32, _F16): False, (1024, _F32, _F32): True,
    (512, _BF16, _BF16): True, (512, _F16, _F16): True, (1024, _BF16, _BF16): False, (1024, _F16, _F16): False,
}

_WIDE = (512, 1024)


def _family(C):
    """(binding, entry-point stem, routing table) of the kernel family that takes C channels."""
    if C in _WIDE:
        return _ffn_wide, 'dhdg_swin_ffn_wide', ROUTED_WIDE
    return _ffn, 'dhdf_swin_ffn', ROUTED


def swin_ffn_shape_supported(x, hidden, mm_dtype=None):
    """True when the operator itself takes the tokens `x` (..., C) with `hidden` units in `mm_dtype` (default x's dtype): a GPU
    tensor, C in {128, 256, 512, 1024}, hidden == 4 C, and float32 tokens with any GEMM dtype or half tokens with their own."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() >= 1 and x.numel() > 0):
        return False
    mm_dtype = mm_dtype or x.dtype
    if x.dtype not in _lib.DTYPE_CODE or mm_dtype not in _lib.DTYPE_CODE:
        return False
    binding, stem, _ = _family(x.shape[-1])
    return bool(binding.value(stem + '_supported', x.shape[-1], int(hidden), _lib.DTYPE_CODE[x.dtype], _lib.DTYPE_CODE[mm_dtype]))


def swin_ffn_supported(x, hidden, mm_dtype=None):
    """True when a `SwinBlock` with `fused_ffn` on sends the tokens `x` (..., C) to the operator: the operator takes them
    (swin_ffn_shape_supported) and the measurement routed that (C, dtype combination) to it (ROUTED, ROUTED_WIDE)."""
    if not swin_ffn_shape_supported(x, hidden, mm_dtype):
        return False
    return _family(x.shape[-1])[2].get((x.shape[-1], x.dtype, mm_dtype or x.dtype), False)


def _param(p, shape, name):
    if p is None:
        return None
    if not p.is_cuda:
        raise _lib.DhdError(f'swin_ffn_infer: {name} must live on the GPU (got {p.device})')
    if tuple(p.shape) != shape:
        raise _lib.DhdError(f'swin_ffn_infer: {name} must have shape {shape}, got {tuple(p.shape)}')
    return _lib.dense16(p.detach().float())


@traced('dhd.swin.ffn.infer')
def swin_ffn_infer(x, norm_weight, norm_bias, eps, w1, b1, w2, b2, mm_dtype=None):
    """x + fc2(gelu(fc1(layer_norm(x)))) for tokens x (..., C): norm_weight, norm_bias (C,) the LayerNorm's affine parameters
    (both None: no LayerNorm, `FFN.forward(x)`), w1 (4C, C), b1 (4C,), w2 (C, 4C), b2 (C,) the two Linear layers, exact (erf) GELU.
    Returns a new tensor of x's shape and dtype.

    mm_dtype (default x's dtype) is what the two Linear layers run in: float32 (bf16x3 split products) or a half type (one
    product, float32 accumulation; the LayerNorm output and the GELU output each rounded once to it) -- under autocast pass the
    autocast dtype with float32 tokens.  Statistics, biases, GELU and the residual add are float32.  Parameters of another dtype
    are read as `.float()`, which is exact.  A non-contiguous or misaligned view of x is made dense first.  The weights are laid
    out into scratch from torch's allocator on every call; nothing is cached.  Forward only, HIP only: a CPU tensor or an
    unsupported size raises DhdError."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.DhdError(f'swin_ffn_infer: x must live on the GPU: dhd_amd runs only as HIP kernels (got {getattr(x, "device", None)})')
    mm_dtype = mm_dtype or x.dtype
    C = x.shape[-1]
    hidden = w1.shape[0]
    if not swin_ffn_shape_supported(x, hidden, mm_dtype):
        raise _lib.DhdError(f'swin_ffn_infer: no operator for tokens {tuple(x.shape)} of {x.dtype}, hidden {hidden}, GEMMs in {mm_dtype}')
    if (norm_weight is None) != (norm_bias is None):
        raise _lib.DhdError('swin_ffn_infer: norm_weight and norm_bias are given together or not at all')
    binding, stem, _ = _family(C)
    dev = x.device
    x = _lib.dense16(x.detach())
    gamma, beta = _param(norm_weight, (C,), 'norm_weight'), _param(norm_bias, (C,), 'norm_bias')
    w1, b1 = _param(w1, (hidden, C), 'w1'), _param(b1, (hidden,), 'b1')
    w2, b2 = _param(w2, (C, hidden), 'w2'), _param(b2, (C,), 'b2')
    xc, mc = _lib.dtype_code(x.dtype), _lib.dtype_code(mm_dtype)
    with torch.cuda.device(dev):
        out = torch.empty(x.shape, dtype=x.dtype, device=dev)
        nbytes = binding.value(stem + '_scratch_bytes', C, hidden, mc)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        binding.call(stem + '_infer', _lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2),
                     _lib.ptr(b2), _lib.ptr(out), _lib.ptr(scratch), nbytes, xc, mc, x.numel() // C, C, hidden, float(eps),
                     _lib.stream_ptr(dev))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Training: forward with the DropPath factor, recompute backward (C = 128 and 256; C = 512 through the wide training family)

# Which (C, x dtype, GEMM dtype) entries `swin_ffn_train_supported` routes to `swin_ffn`, by ROUTED's rule applied to forward +
# backward (both weight packs and the torch weight-gradient GEMMs included) against both parents with torch autograd at DHD-L's
# stage shapes, 12 images, DropPath active (experiments/swin_ffn_train_bench.py -> profiles/r16/swin_ffn_train.json).  Medians in
# us per forward + backward, fused against today / today with fused_glue's norm2 (largest min-max spread of the three paths):
#   C = 128, 540 672 rows: bf16 autocast 3982 against 5838 / 4577 (59), fp16 autocast 4016 against 5823 / 4540 (44),
#                          float32 5494 against 8944 / 7827 (40)
#   C = 256, 135 168 rows: bf16 autocast 2164 against 2558 / 2256 (9), fp16 autocast 2176 against 2551 / 2247 (79),
#                          bf16 tokens 2050 against 2493 / 2148 (12), fp16 tokens 2051 against 2502 / 2148 (85)
# "bf16 tokens" is the residual stream in the autocast type, which is what patch merging hands DHD-L's stage 1 under autocast.
# fp16 autocast at C = 256 wins by 71 us, less than that run's spread (one slow window of the glue parent): False by the rule.
# Not measured, False: C = 256 in float32 (the form that loads x and dout again per hidden tile), C = 128 with half tokens.  The
# operator itself takes every entry when called directly.
ROUTED_TRAIN = {
    (128, _F32, _BF16): True, (128, _F32, _F16): True, (128, _F32, _F32): True,
    (256, _F32, _BF16): True, (256, _F32, _F16): False, (256, _F32, _F32): False,
    (128, _BF16, _BF16): False, (128, _F16, _F16): False, (256, _BF16, _BF16): True, (256, _F16, _F16): True,
}


def swin_ffn_train_shape_supported(x, hidden, mm_dtype=None):
    """True when `swin_ffn` itself takes the tokens `x` (..., C) with `hidden` units in `mm_dtype` (default x's dtype): a GPU
    tensor, C in {128, 256}, hidden == 4 C, float32 tokens with any GEMM dtype or half tokens with their own."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() >= 1 and x.numel() > 0):
        return False
    mm_dtype = mm_dtype or x.dtype
    if x.dtype not in _lib.DTYPE_CODE or mm_dtype not in _lib.DTYPE_CODE:
        return False
    return bool(_ffn_train.value('dhdt_swin_ffn_supported', x.shape[-1], int(hidden), _lib.DTYPE_CODE[x.dtype], _lib.DTYPE_CODE[mm_dtype]))


def swin_ffn_train_supported(x, hidden, mm_dtype=None):
    """True when a `SwinBlock` with `fused_ffn_train` on sends the tokens `x` (..., C) to `swin_ffn`: the operator takes them
    (swin_ffn_train_shape_supported) and the measurement routed that (C, dtype combination) to it (ROUTED_TRAIN)."""
    if not swin_ffn_train_shape_supported(x, hidden, mm_dtype):
        return False
    return ROUTED_TRAIN.get((x.shape[-1], x.dtype, mm_dtype or x.dtype), False)


# The wide training family (C = 512: DHD-L's stage 2, csrc/swin_ffn_wide_train.h), `SwinBlock.fused_ffn_train_wide`'s table, by
# ROUTED_TRAIN's rule: an entry is True only where forward + backward beat both parents by more than the largest min-max spread
# of the three paths at 33 792 x 512, 12 images, DropPath active (experiments/swin_ffn_train_wide_bench.py ->
# profiles/r17/swin_ffn_train_wide.json).  Medians in us per forward + backward, fused against today / today with fused_glue's
# norm2 (largest min-max spread of the three paths); with half tokens there is no cast for the glue's norm2 to fuse, so both
# parents are the same code there and their difference is run-to-run noise:
#   bf16 autocast 1342 against 1408 / 1347 (45), fp16 autocast 1370 against 1404 / 1356 (66), float32 2617 against 3817 / 3808 (33),
#   bf16 tokens 1342 against 1420 / 1383 (52), fp16 tokens 1349 against 1422 / 1391 (42)
# The forward alone wins everywhere (251 / 258 / 567 / 251 / 259 against 335 / 332 / 1312 / 378 / 369 for the better parent); with
# half GEMMs the backward gives that back: 528 workgroups of 64 rows are 2.06 rounds on 256 CUs.  float32 wins by 1191 us.  fp16
# tokens win by 42.2 us against a spread of 41.8: True by the rule, by the narrowest of margins.  bf16 tokens -- what DHD-L's
# backbone hands stage 2 under bf16 autocast -- win by 41 us, less than that run's spread: False, as are the two autocast forms
# with float32 tokens (a tie, and a loss of 14 us to the glue parent).  The operator itself takes every entry when called directly.
# (Under checkpointing a block's forward runs twice, which this rule counts once: with every entry forced the DHD-L bf16 step is
# 235.0 against 236.6 ms, profiles/r17/e2e_dhdl_bf16_swin_ffn_train_wide_forced_ab.json.  The table follows the rule.)
ROUTED_TRAIN_WIDE = {
    (512, _F32, _BF16): False, (512, _F32, _F16): False, (512, _F32, _F32): True,
    (512, _BF16, _BF16): False, (512, _F16, _F16): True,
}


def swin_ffn_train_wide_shape_supported(x, hidden, mm_dtype=None):
    """True when `swin_ffn`'s wide family takes the tokens `x` (..., C) with `hidden` units in `mm_dtype` (default x's dtype): a
    GPU tensor, C == 512, hidden == 2048, float32 tokens with any GEMM dtype or half tokens with their own."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() >= 1 and x.numel() > 0):
        return False
    mm_dtype = mm_dtype or x.dtype
    if x.dtype not in _lib.DTYPE_CODE or mm_dtype not in _lib.DTYPE_CODE:
        return False
    return bool(_ffn_wide_train.value('dhdu_swin_ffn_wide_supported', x.shape[-1], int(hidden), _lib.DTYPE_CODE[x.dtype],
                                      _lib.DTYPE_CODE[mm_dtype]))


def swin_ffn_train_wide_supported(x, hidden, mm_dtype=None):
    """True when a `SwinBlock` with `fused_ffn_train_wide` on sends the tokens `x` (..., C) to `swin_ffn`: the wide family takes
    them (swin_ffn_train_wide_shape_supported) and the measurement routed that dtype combination to it (ROUTED_TRAIN_WIDE)."""
    if not swin_ffn_train_wide_shape_supported(x, hidden, mm_dtype):
        return False
    return ROUTED_TRAIN_WIDE.get((x.shape[-1], x.dtype, mm_dtype or x.dtype), False)


def _train_family(C):
    """(binding, entry-point stem) of the training family that takes C channels."""
    if C == 512:
        return _ffn_wide_train, 'dhdu_swin_ffn_wide'
    return _ffn_train, 'dhdt_swin_ffn'


def _f32(p):
    return _lib.dense16(p.detach().float())


def _scaled_grad(dout, scale, mm_dtype):
    """gs (rows, C): the gradient times its image's factor, the float32 product rounded once to the GEMM dtype, as the kernel
    forms its own."""
    C = dout.shape[-1]
    g = dout.reshape(-1, C)
    if scale is None:
        return g.to(mm_dtype)
    return (g.float().view(scale.numel(), -1, C) * scale.view(-1, 1, 1)).to(mm_dtype).view(-1, C)


def swin_ffn_backward(x, dout, norm_weight, norm_bias, eps, w1, b1, w2, mm_dtype=None, scale=None, operands=True):
    """One dhdt_swin_ffn_backward (C = 512: dhdu_swin_ffn_wide_backward) call on dense, aligned GPU tensors: x, dout (..., C) of
    one dtype, the parameters as swin_ffn takes them (b2 has no part), scale float32 (images,) or None -> (dx, dgamma, dbeta, xn,
    act, dhid): dx in x's dtype and shape, dgamma and dbeta float32 (C,), and with `operands` the weight-gradient operands xn (rows, C), act and dhid (rows, 4C) in
    mm_dtype, else three None (the kernel then writes none of them).  Allocates its outputs and its scratch; nothing is cached."""
    mm_dtype = mm_dtype or x.dtype
    C, hidden = x.shape[-1], w1.shape[0]
    rows, dev = x.numel() // C, x.device
    xc, mc = _lib.dtype_code(x.dtype), _lib.dtype_code(mm_dtype)
    binding, stem = _train_family(C)
    with torch.cuda.device(dev):
        dx = torch.empty_like(x)
        dgamma = torch.empty(C, dtype=torch.float32, device=dev)
        dbeta = torch.empty(C, dtype=torch.float32, device=dev)
        xn = act = dhid = None
        if operands:
            xn = torch.empty((rows, C), dtype=mm_dtype, device=dev)
            act = torch.empty((rows, hidden), dtype=mm_dtype, device=dev)
            dhid = torch.empty((rows, hidden), dtype=mm_dtype, device=dev)
        nbytes = binding.value(stem + '_backward_scratch_bytes', rows, C, hidden, mc)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        held = [_f32(p) for p in (norm_weight, norm_bias, w1, b1, w2)]      # a half model's float32 copies live until the call is made
        binding.call(stem + '_backward', _lib.ptr(x), _lib.ptr(dout), *(_lib.ptr(p) for p in held), _lib.ptr(scale),
                     rows // scale.numel() if scale is not None else 0, _lib.ptr(dx), _lib.ptr(dgamma), _lib.ptr(dbeta),
                     _lib.ptr(xn), _lib.ptr(act), _lib.ptr(dhid), _lib.ptr(scratch), nbytes, xc, mc, rows, C, hidden, float(eps),
                     _lib.stream_ptr(dev))
    return dx, dgamma, dbeta, xn, act, dhid


def _forward(x, norm_weight, norm_bias, eps, w1, b1, w2, b2, mm_dtype, scale):
    """One dhdt_swin_ffn_forward (C = 512: dhdu_swin_ffn_wide_forward) call on a dense, aligned x."""
    C, hidden = x.shape[-1], w1.shape[0]
    rows, dev = x.numel() // C, x.device
    xc, mc = _lib.dtype_code(x.dtype), _lib.dtype_code(mm_dtype)
    binding, stem = _train_family(C)
    with torch.cuda.device(dev):
        out = torch.empty(x.shape, dtype=x.dtype, device=dev)
        nbytes = binding.value(stem + '_forward_scratch_bytes', C, hidden, mc)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        held = [_f32(p) for p in (norm_weight, norm_bias, w1, b1, w2, b2)]  # a half model's float32 copies live until the call is made
        binding.call(stem + '_forward', _lib.ptr(x), *(_lib.ptr(p) for p in held), _lib.ptr(scale),
                     rows // scale.numel() if scale is not None else 0, _lib.ptr(out), _lib.ptr(scratch), nbytes, xc, mc, rows,
                     C, hidden, float(eps), _lib.stream_ptr(dev))
    return out


class _SwinFFN(torch.autograd.Function):
    """out = x + scale * ffn(norm2(x)); saves the dense x, the parameters and scale, and nothing else: the backward recomputes
    the hidden tile by tile in dhdt_swin_ffn_backward (C = 512: chunk by chunk in dhdu_swin_ffn_wide_backward) and leaves the
    four weight-gradient reductions to torch's GEMMs."""

    @staticmethod
    def forward(ctx, x, norm_weight, norm_bias, w1, b1, w2, b2, scale, eps, mm_dtype):
        xd = _lib.dense16(x.detach())
        out = _forward(xd, norm_weight, norm_bias, eps, w1, b1, w2, b2, mm_dtype, scale)
        ctx.save_for_backward(xd, norm_weight, norm_bias, w1, b1, w2, b2, scale)
        ctx.args = (float(eps), mm_dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @traced('dhd.swin.ffn.train')
    def backward(ctx, dout):
        x, norm_weight, norm_bias, w1, b1, w2, b2, scale = ctx.saved_tensors
        eps, mm_dtype = ctx.args
        need = ctx.needs_input_grad
        dout = _lib.dense16(dout.to(x.dtype))      # a strided or misaligned gradient is copied; x was saved dense
        with torch.autocast('cuda', enabled=False):
            # no weight or bias wants a gradient: the kernel writes none of their operands
            dx, dgamma, dbeta, xn, act, dhid = swin_ffn_backward(x, dout, norm_weight, norm_bias, eps, w1, b1, w2, mm_dtype, scale,
                                                                 operands=any(need[3:7]))
            dw1 = db1 = dw2 = db2 = None
            if need[3]:
                dw1 = (dhid.t() @ xn).to(w1.dtype)
            if need[4]:
                db1 = dhid.sum(0, dtype=torch.float32).to(b1.dtype)
            if need[5] or need[6]:
                gs = _scaled_grad(dout, scale, mm_dtype)
                if need[5]:
                    dw2 = (gs.t() @ act).to(w2.dtype)
                if need[6]:
                    db2 = gs.sum(0, dtype=torch.float32).to(b2.dtype)
        return (dx if need[0] else None, dgamma.to(norm_weight.dtype) if need[1] else None, dbeta.to(norm_bias.dtype) if need[2] else None,
                dw1, db1, dw2, db2, None, None, None)


def swin_ffn(x, norm_weight, norm_bias, eps, w1, b1, w2, b2, mm_dtype=None, scale=None):
    """x + scale * fc2(gelu(fc1(layer_norm(x)))) for tokens x (..., C), differentiable in x and the seven parameters.  The
    arguments are swin_ffn_infer's (the LayerNorm is required here); `scale`, float32 with one factor per image (x.shape[0] of
    them: DropPath's floor(keep + rand) / keep), multiplies the branch in float32 before the residual add; None means 1, and
    then the forward returns swin_ffn_infer's bytes.

    C = 128 and 256 run the dhdt_* family, C = 512 the dhdu_* family; C = 1024 has no training operator.
    The forward saves the dense x, the parameters and scale.  The backward is one backward call of the family, which recomputes
    the hidden tile by tile and returns dx, dgamma, dbeta and -- where a weight or bias wants a gradient -- the operands xn, act
    and dhid in mm_dtype, from which torch's GEMMs take dW1 = dhid^T @ xn, db1 = sum dhid, dW2 = gs^T @ act, db2 = sum gs (gs the
    scaled gradient in mm_dtype), each cast to its parameter's dtype.  No atomics: a repeated call gives the same bytes.  Works
    under torch.autocast (pass the autocast dtype as mm_dtype) and under checkpoint(..., use_reentrant=False).  HIP only: a CPU
    tensor or an unsupported size raises DhdError."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.DhdError(f'swin_ffn: x must live on the GPU: dhd_amd runs only as HIP kernels (got {getattr(x, "device", None)})')
    mm_dtype = mm_dtype or x.dtype
    C, hidden = x.shape[-1], w1.shape[0]
    if not (swin_ffn_train_shape_supported(x, hidden, mm_dtype) or swin_ffn_train_wide_shape_supported(x, hidden, mm_dtype)):
        raise _lib.DhdError(f'swin_ffn: no operator for tokens {tuple(x.shape)} of {x.dtype}, hidden {hidden}, GEMMs in {mm_dtype}')
    for p, shape, name in ((norm_weight, (C,), 'norm_weight'), (norm_bias, (C,), 'norm_bias'), (w1, (hidden, C), 'w1'),
                           (b1, (hidden,), 'b1'), (w2, (C, hidden), 'w2'), (b2, (C,), 'b2')):
        if not (torch.is_tensor(p) and p.is_cuda and tuple(p.shape) == shape):
            raise _lib.DhdError(f'swin_ffn: {name} must be a GPU tensor of shape {shape}')
    if scale is not None:
        if not (scale.is_cuda and scale.numel() > 0 and (x.numel() // C) % scale.numel() == 0):
            raise _lib.DhdError(f'swin_ffn: scale must hold one factor per image of x on the GPU, got {tuple(scale.shape)} for {tuple(x.shape)}')
        scale = _lib.dense16(scale.detach().float().reshape(-1))
    return _SwinFFN.apply(x, norm_weight, norm_bias, w1, b1, w2, b2, scale, eps, mm_dtype)


class _CallableModule(types.ModuleType):
    """`dhd_amd.swin_ffn` names this module and, as the package's public interface, the function of the same name: calling the
    module calls the function, so `dhd_amd.swin_ffn(x, ...)` and `dhd_amd.swin_ffn.swin_ffn_infer` both hold."""
    __call__ = staticmethod(swin_ffn)


sys.modules[__name__].__class__ = _CallableModule
