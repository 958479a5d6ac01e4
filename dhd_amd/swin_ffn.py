"""The second half of a Swin block at inference as one HIP operator (csrc/swin_ffn.hip, include/dhd_amd_ffn.h for C = 128 and
256; csrc/swin_ffn_wide.h, include/dhd_amd_ffn_wide.h for C = 512 and 1024):

    swin_ffn_infer(x, norm_weight, norm_bias, eps, w1, b1, w2, b2) = x + fc2(gelu(fc1(layer_norm(x))))

x is read once (the wide family: twice) and the result written once; the normalised rows and the two (tokens x 4C) hidden tensors never exist.  Forward
only: nothing is saved and nothing is differentiable, which is why `SwinBlock.fused_ffn` routes to it only in eval mode with
nothing to differentiate.  The entry points are reached through _ffn.call(name, ...) / _ffn.value(name, ...), or the same two
of _ffn_wide: the functions here dispatch on C to the family that takes it."""
import torch

from . import _ffn, _ffn_wide, _lib
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
