"""The occupancy head at inference as one HIP operator (csrc/occ_head.hip, section 14 of include/dhd_amd.h):
predictor.forward after final_conv (models/dense_heads/occ_head.py:84-100: Linear -> Softplus -> Linear per BEV cell) and
get_occ (:141-153) in one kernel that writes the uint8 class grid, and on request the mIoU histogram and the float32 logits.
The (cells, 512) hidden and the (cells, 288) logits of the module formulation never reach memory.

In training the same MLP is `occ_head_train` (csrc/occ_head_train.h, capi/dhd_amd_occ_train.h): an autograd function whose
forward is the inference operator writing float32 logits, saving x and the parameters and nothing of hidden size, and whose
backward recomputes the hidden tile by tile in one HIP call -- `predictor.fused_train`'s route.  `occ_head_losses`
(csrc/occ_head_loss.h, capi_occ_loss/dhd_amd_occ_head_loss.h) is that function with the head's three losses inside: the loss sums
ride in the forward kernel and the loss gradient in the backward kernel -- `predictor.fused_loss`'s route."""
import ctypes as C

import torch

from . import _lib, _occ_loss_head, _occ_train
from .occ_loss import NUM_CLASSES
from .trace import traced


def _layout_of(x):
    """0 = NCHW, 1 = channels_last, None = neither (the caller makes it contiguous)."""
    if x.is_contiguous():
        return 0
    if x.is_contiguous(memory_format=torch.channels_last):
        return 1
    return None


def supported(x, w1, w2, dz=16, gemm=None):
    """True when occ_head_infer takes this call: a GPU tensor (B, C, Dy, Dx) of a dtype, and weights of a shape, that the kernel has."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in _lib.DTYPE_CODE and w1.dim() == 2 and w2.dim() == 2):
        return False
    if w1.shape[1] != x.shape[1] or w2.shape[1] != w1.shape[0] or w2.shape[0] % dz:
        return False
    layout = _layout_of(x)
    return bool(_lib.load().dhd_occ_head_infer_supported(x.shape[1], w1.shape[0], dz, w2.shape[0] // dz, _lib.DTYPE_CODE[x.dtype],
                                                        0 if layout is None else layout, _lib.SFA_GEMM[gemm or 'default']))


def _f32(t, name):
    return _lib.require_gpu_tensor(t.detach().float().contiguous(), torch.float32, name)


@traced('dhd.occ_head.infer')
def occ_head_infer(x, w1, b1, w2, b2, dz=16, labels=None, mask_camera=None, hist=None, return_logits=False, gemm=None):
    """x: final_conv's output (B, C, Dy, Dx), float32 / float16 / bfloat16, NCHW or channels_last; w1 (hidden, C), b1, w2
    (dz * n_classes, hidden), b2: the predicter's parameters.  Returns pred, a device uint8 tensor (B, Dx, Dy, dz) -- the class
    map in the reference's orientation -- or, when labels are given or return_logits is set, (pred, hist, logits) with None
    for what was not asked for.  hist (18, 18) int64 is accumulated into when given (rows = ground truth, columns = prediction;
    labels / mask_camera (B, Dx, Dy, dz) as in occ_loss.occ_argmax_hist); logits are (B, Dx, Dy, dz, n_classes) float32.
    No autograd node, nothing kept between calls; scratch comes from the pool."""
    if not x.is_cuda:
        raise _lib.DhdError(f'occ_head_infer: x must live on the GPU (got {x.device})')
    x = x.detach()
    layout = _layout_of(x)
    if layout is None:
        x, layout = x.contiguous(), 0
    if x.data_ptr() % 16:     # 16-byte loads of x: a dense view at an odd storage offset is copied, in its layout
        x = x.clone(memory_format=torch.preserve_format)
    b, c, dy, dx = x.shape
    if hist is not None and labels is None:
        raise _lib.DhdError('occ_head_infer: hist needs labels (nothing would be counted)')
    w1, b1, w2, b2 = _f32(w1, 'predicter[0].weight'), _f32(b1, 'predicter[0].bias'), _f32(w2, 'predicter[2].weight'), _f32(b2, 'predicter[2].bias')
    if b2.data_ptr() % 16:    # read as float4; a parameter that is a view of a flat buffer may sit anywhere
        b2 = b2.clone()
    n_cls = w2.shape[0] // dz
    if w1.shape[1] != c or b1.numel() != w1.shape[0] or w2.shape != (dz * n_cls, w1.shape[0]) or b2.numel() != w2.shape[0]:
        raise _lib.DhdError('occ_head_infer: inconsistent parameter shapes')
    wts = _lib.OccHeadWeights()
    wts.w1, wts.b1, wts.w2, wts.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    wts.c, wts.hidden, wts.dz, wts.n_classes, wts.gemm = c, w1.shape[0], dz, n_cls, _lib.SFA_GEMM[gemm or 'default']
    code = _lib.dtype_code(x.dtype)
    lib = _lib.load()
    dev = x.device
    with torch.cuda.device(dev):
        nscratch = C.c_size_t()
        _lib.check(lib.dhd_occ_head_infer_scratch_bytes(C.byref(wts), code, C.byref(nscratch)), 'dhd_occ_head_infer_scratch_bytes')
        from .mghs_op import scratch_pool
        scratch = scratch_pool.get(dev, nscratch.value, 'occ_head')
        pred = torch.empty(b, dx, dy, dz, dtype=torch.uint8, device=dev)
        logits = torch.empty(b, dx, dy, dz, n_cls, dtype=torch.float32, device=dev) if return_logits else None
        lab = msk = None
        if labels is not None:
            lab = labels.reshape(-1).to(device=dev, dtype=torch.uint8).contiguous()
            msk = None if mask_camera is None else mask_camera.reshape(-1).to(device=dev, dtype=torch.uint8).contiguous()
            # labels and mask are read 8 voxels at a time
            lab = lab.clone() if lab.data_ptr() % 8 else lab
            msk = msk.clone() if msk is not None and msk.data_ptr() % 8 else msk
            if lab.numel() != pred.numel() or (msk is not None and msk.numel() != pred.numel()):
                raise _lib.DhdError('occ_head_infer: labels / mask_camera must have one element per voxel')
            if hist is None:
                hist = torch.zeros(n_cls, n_cls, dtype=torch.int64, device=dev)
            else:
                _lib.require_gpu_tensor(hist, torch.int64, 'hist')
        _lib.check(lib.dhd_occ_head_infer(_lib.ptr(x), code, layout, C.byref(wts), b, dy, dx, _lib.ptr(pred), _lib.ptr(logits),
                                          _lib.ptr(lab), _lib.ptr(msk), _lib.ptr(hist) if lab is not None else None,
                                          _lib.ptr(scratch), _lib.stream_ptr(dev)), 'dhd_occ_head_infer')
    if labels is None and not return_logits:
        return pred
    return pred, (hist if labels is not None else None), logits


# ---------------------------------------------------------------------------------------------------------------------------
# Training: the inference operator as the forward, recompute HIP backward

# Which (x dtype, layout) entries `predictor.fused_train` routes to `occ_head_train` (layout 0 = NCHW, 1 = channels_last): by
# swin_ffn.ROUTED_TRAIN's rule, True only where forward + backward, both weight packs and the torch weight-gradient GEMMs
# included, beat today's path (predicter(x), .float(), autograd from the same float32 glogits) by more than the larger min-max
# spread of the two paths at (4, 256, 200, 200) (experiments/occ_head_train_bench.py -> profiles/r20/occ_head_train.json).
# Medians in us per forward + backward, fused against today (larger min-max spread of the two); x under autocast is in the
# autocast type, as final_conv hands it over:
#   float32        NCHW 3100 against 4155 (166),  channels_last 3776 against 4020 (68)
#   fp16 autocast  NCHW 1357 against 2605 (57),   channels_last 1606 against 2443 (29)
#   bf16 autocast  NCHW 1332 against 2591 (41),   channels_last 1575 against 2431 (22)
# The forward alone: 356 / 373 / 250 / 254 / 256 / 250 against 1297 / 1168 / 977 / 814 / 970 / 811.  Held between forward and
# backward on top of x: 176 MiB, the float32 logits, against 957 MiB in float32 and 723 MiB under autocast; peak of one step
# 963 against 1342 MiB and 659 against 1192 MiB.  Every entry wins by more than the spread; float32 channels_last by the
# narrowest margin (244 us).  The channels_last steps are slower than the NCHW ones in every type; where that time goes (the
# kernel or the dW1 GEMM on the view of x) was not measured.
ROUTED_TRAIN = {
    (torch.float32, 0): True, (torch.float32, 1): True,
    (torch.float16, 0): True, (torch.float16, 1): True,
    (torch.bfloat16, 0): True, (torch.bfloat16, 1): True,
}


def train_supported(x, w1, w2, dz=16):
    """True when `occ_head_train` itself takes this call: a GPU tensor (B, 256, Dy, Dx) with at least one cell, float32 / float16 /
    bfloat16, and weights of the head the kernel has (hidden 512, dz * n_classes = 16 * 18) -- the inference operator's set."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.numel() > 0 and x.dtype in _lib.DTYPE_CODE):
        return False
    if not (torch.is_tensor(w1) and torch.is_tensor(w2) and w1.dim() == 2 and w2.dim() == 2):
        return False
    if w1.shape[1] != x.shape[1] or w2.shape[1] != w1.shape[0] or w2.shape[0] % dz:
        return False
    return bool(_occ_train.value('dhdo_occ_head_backward_supported', x.shape[1], w1.shape[0], dz, w2.shape[0] // dz,
                                 _lib.DTYPE_CODE[x.dtype], _train_layout(x)))


def train_routed(x, w1, w2, dz=16):
    """True when a `predictor` with `fused_train` on sends final_conv's output `x` to `occ_head_train`: the operator takes it
    (train_supported) and the measurement routed that (dtype, layout) to it (ROUTED_TRAIN)."""
    if not train_supported(x, w1, w2, dz):
        return False
    return ROUTED_TRAIN.get((x.dtype, _train_layout(x)), False)


def _weights(w1, b1, w2, b2, c, dz):
    """(dhd_occ_head_weights, the float32 tensors it points to): a half model's float32 copies live until the call is made.
    b2 may be None (the backward does not read it)."""
    held = [None if p is None else _lib.dense16(p.detach().float()) for p in (w1, b1, w2, b2)]
    wts = _lib.OccHeadWeights()
    wts.w1, wts.b1, wts.w2, wts.b2 = (None if p is None else p.data_ptr() for p in held)
    wts.c, wts.hidden, wts.dz, wts.n_classes, wts.gemm = c, w1.shape[0], dz, w2.shape[0] // dz, _lib.SFA_GEMM['default']
    return wts, held


def _train_layout(x):
    """The layout occ_head_train runs x in: its own where it is dense; a view that is neither keeps the order of its strides
    (channels innermost: channels_last, else NCHW) when it is made dense."""
    layout = _layout_of(x)
    if layout is None:
        layout = 1 if x.stride(1) == 1 and x.shape[1] > 1 else 0
    return layout


def _dense_in_layout(x):
    """(x dense and 16-byte aligned in _train_layout's layout, the layout code)."""
    layout = _train_layout(x)
    return _lib.dense16(x, torch.channels_last if layout else torch.contiguous_format), layout


def _forward_logits(x, layout, w1, b1, w2, b2, dz):
    """One dhd_occ_head_infer call with pred = NULL on a dense, aligned x: the float32 logits (B, Dx, Dy, dz, n_classes)."""
    b, c, dy, dx = x.shape
    code, dev = _lib.dtype_code(x.dtype), x.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        wts, held = _weights(w1, b1, w2, b2, c, dz)
        nbytes = C.c_size_t()
        _lib.check(lib.dhd_occ_head_infer_scratch_bytes(C.byref(wts), code, C.byref(nbytes)), 'dhd_occ_head_infer_scratch_bytes')
        scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        logits = torch.empty(b, dx, dy, dz, wts.n_classes, dtype=torch.float32, device=dev)
        _lib.check(lib.dhd_occ_head_infer(_lib.ptr(x), code, layout, C.byref(wts), b, dy, dx, None, _lib.ptr(logits), None, None, None,
                                          _lib.ptr(scratch), _lib.stream_ptr(dev)), 'dhd_occ_head_infer')
    return logits


def occ_head_backward(x, glogits, w1, b1, w2, dz=16, operands=True):
    """One dhdo_occ_head_backward call on dense, aligned GPU tensors: x (B, 256, Dy, Dx) NCHW or channels_last, glogits float32
    (B, Dx, Dy, dz, n_classes), the parameters as occ_head_train takes them (b2 has no part) -> (dx, db1, db2, act, dhid, ghalf):
    dx in x's dtype and layout, db1 (512,) and db2 (288,) float32, and with `operands` the weight-gradient operands in x's dtype --
    act (cells, 512) in the logits' cell order, dhid (cells, 512) in x's pixel order, and for a half x ghalf (cells, 288), glogits
    rounded once -- else three None (the kernel then writes none of them).  Allocates its outputs and its scratch; nothing is cached."""
    b, c, dy, dx = x.shape
    layout = _layout_of(x)
    if layout is None:
        raise _lib.DhdError('occ_head_backward: x must be dense, NCHW or channels_last')
    code, dev, cells = _lib.dtype_code(x.dtype), x.device, b * dy * dx
    hidden, cols = w1.shape[0], w2.shape[0]
    with torch.cuda.device(dev):
        wts, held = _weights(w1, b1, w2, None, c, dz)
        dxo = torch.empty_like(x)                           # preserve_format: x's own layout
        db1 = torch.empty(hidden, dtype=torch.float32, device=dev)
        db2 = torch.empty(cols, dtype=torch.float32, device=dev)
        act = dhid = ghalf = None
        if operands:
            act = torch.empty((cells, hidden), dtype=x.dtype, device=dev)
            dhid = torch.empty((cells, hidden), dtype=x.dtype, device=dev)
            if x.dtype != torch.float32:
                ghalf = torch.empty((cells, cols), dtype=x.dtype, device=dev)
        nbytes = C.c_size_t()
        _occ_train.call('dhdo_occ_head_backward_scratch_bytes', C.byref(wts), code, b, dy, dx, C.byref(nbytes))
        scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        _occ_train.call('dhdo_occ_head_backward', _lib.ptr(x), code, layout, C.byref(wts), b, dy, dx, _lib.ptr(glogits), _lib.ptr(dxo),
                        _lib.ptr(db1), _lib.ptr(db2), _lib.ptr(act), _lib.ptr(dhid), _lib.ptr(ghalf), _lib.ptr(scratch), nbytes.value,
                        _lib.stream_ptr(dev))
    return dxo, db1, db2, act, dhid, ghalf


class _OccHeadTrain(torch.autograd.Function):
    """logits = W2 . softplus(W1 . x + b1) + b2 per BEV cell; saves the dense x and the parameters and nothing else: the backward
    recomputes the hidden tile by tile in dhdo_occ_head_backward and leaves the two weight-gradient reductions to torch's GEMMs."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, dz):
        xd, layout = _dense_in_layout(x.detach())
        logits = _forward_logits(xd, layout, w1, b1, w2, b2, dz)
        ctx.save_for_backward(xd, w1, b1, w2, b2)
        ctx.dz = dz
        return logits

    @staticmethod
    @torch.autograd.function.once_differentiable
    @traced('dhd.occ_head.train')
    def backward(ctx, glogits):
        x, w1, b1, w2, b2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = _lib.dense16(glogits.float())                   # a strided or misaligned gradient is copied; x was saved dense
        with torch.autocast('cuda', enabled=False):
            # no weight wants a gradient: the kernel writes none of their operands
            dx, db1, db2, act, dhid, ghalf = occ_head_backward(x, g, w1, b1, w2, ctx.dz, operands=need[1] or need[3])
            dw1 = dw2 = None
            if need[1]:
                b, c, dy, dxs = x.shape
                if x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
                    dw1 = dhid.t() @ x.permute(0, 2, 3, 1).reshape(-1, c)          # a view: x's pixels are dhid's rows
                else:                                                               # NCHW: one product per sample, summed
                    per = torch.bmm(dhid.view(b, dy * dxs, -1).transpose(1, 2), x.reshape(b, c, dy * dxs).transpose(1, 2))
                    dw1 = per[0] if b == 1 else per.sum(0, dtype=torch.float32)
                dw1 = dw1.to(w1.dtype)
            if need[3]:
                gm = ghalf if ghalf is not None else g.view(-1, w2.shape[0])
                dw2 = (gm.t() @ act).to(w2.dtype)
        return (dx if need[0] else None, dw1, db1.to(b1.dtype) if need[2] else None, dw2, db2.to(b2.dtype) if need[4] else None, None)


def occ_head_train(x, w1, b1, w2, b2, dz=16):
    """The predicter MLP on final_conv's output, differentiable in x and the four parameters: x (B, 256, Dy, Dx), float32 /
    float16 / bfloat16, NCHW or channels_last; w1 (512, 256), b1, w2 (dz * 18, 512), b2.  Returns the logits (B, Dx, Dy, dz, 18) in
    float32 -- the bytes of occ_head_infer(..., return_logits=True), in the reference's permute(0, 3, 2, 1) orientation, what
    occ_loss.occ_losses reads without a cast.

    The GEMMs run in x's type (float32: bf16x3 split products; a half type: its own, float32 accumulation), so under autocast
    final_conv's half output selects the half kernels; parameters of another dtype are read as `.float()`.  The forward saves the
    dense x and the parameters, and nothing of hidden size.  The backward is one dhdo_occ_head_backward call, which recomputes
    the hidden tile by tile and returns dx in x's dtype and layout, db1, db2 and -- where a weight wants a gradient -- the operands
    act, dhid (and ghalf) in x's dtype, from which torch's GEMMs take dW2 = g^T @ act and dW1 = dhid^T @ x, each cast to its
    parameter's dtype.  No atomics: a repeated call gives the same bytes.  Works under torch.autocast, under
    checkpoint(..., use_reentrant=False) and inside a captured HIP graph (no host synchronisation, scratch from torch's
    allocator).  HIP only: a CPU tensor or an unsupported shape raises DhdError."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.DhdError(f'occ_head_train: x must live on the GPU: dhd_amd runs only as HIP kernels (got {getattr(x, "device", None)})')
    if not train_supported(x, w1, w2, dz):
        raise _lib.DhdError(f'occ_head_train: no operator for x {tuple(x.shape)} of {x.dtype} with weights {tuple(w1.shape)}, '
                            f'{tuple(w2.shape)} and dz {dz}')
    for p, shape, name in ((w1, (512, 256), 'w1'), (b1, (512,), 'b1'), (w2, (dz * NUM_CLASSES, 512), 'w2'), (b2, (dz * NUM_CLASSES,), 'b2')):
        if not (torch.is_tensor(p) and p.is_cuda and tuple(p.shape) == shape):
            raise _lib.DhdError(f'occ_head_train: {name} must be a GPU tensor of shape {shape}')
    return _OccHeadTrain.apply(x, w1, b1, w2, b2, dz)


# ---------------------------------------------------------------------------------------------------------------------------
# Training: the head and its three losses as one operator (csrc/occ_head_loss.h, capi_occ_loss/dhd_amd_occ_head_loss.h)

# Which (x dtype, layout) entries `predictor.fused_loss` routes to `occ_head_losses` (layout 0 = NCHW, 1 = channels_last): by
# ROUTED_TRAIN's rule, True only where forward + backward of head and losses, the weight packs and the torch weight-gradient
# GEMMs included, beat occ_head_train + occ_loss.occ_losses by more than the larger min-max spread of the two paths at
# (4, 256, 200, 200) with a 70 % camera mask (experiments/occ_head_loss_bench.py -> profiles/r23/occ_head_loss.json).
# Medians in us per forward + backward, fused against the parent path (larger min-max spread of the two):
#   float32        NCHW 3352 against 3310 (13),   channels_last 4010 against 3926 (19)
#   fp16 autocast  NCHW 1465 against 1462 (52),   channels_last 1668 against 1700 (28)
#   bf16 autocast  NCHW 1465 against 1466 (42),   channels_last 1675 against 1704 (35)
# The forward alone: 410 / 429 / 285 / 284 / 281 / 282 against 405 / 432 / 276 / 278 / 274 / 279.  The two loss passes the operator
# removes cost the parent path about 110 us of a step, and the softmax epilogue and prologue cost the fused kernels as much: one
# entry wins by more than the spread (fp16 channels_last, by 32 us), bf16 channels_last wins by less (29 against 35), the NCHW
# half entries tie and float32 loses (it writes and re-reads the same float32 g, with the softmax on top).  Held between forward
# and backward: 176 MiB either way; peak of a step 659 MiB either way under autocast, 1138 against 962 MiB in float32 (g is
# allocated beside act and dhid instead of before them).
ROUTED_LOSS = {
    (torch.float32, 0): False, (torch.float32, 1): False,
    (torch.float16, 0): False, (torch.float16, 1): True,
    (torch.bfloat16, 0): False, (torch.bfloat16, 1): False,
}


def loss_supported(x, w1, w2, dz=16):
    """True when `occ_head_losses` itself takes this call: occ_head_train's set (train_supported)."""
    if not train_supported(x, w1, w2, dz):
        return False
    return bool(_occ_loss_head.value('dhdl_occ_head_loss_supported', x.shape[1], w1.shape[0], dz, w2.shape[0] // dz,
                                     _lib.DTYPE_CODE[x.dtype], _train_layout(x)))


def loss_routed(x, w1, w2, dz=16):
    """True when a `predictor` with `fused_loss` on sends final_conv's output `x` to `occ_head_losses`."""
    if not loss_supported(x, w1, w2, dz):
        return False
    return ROUTED_LOSS.get((x.dtype, _train_layout(x)), False)


def _voxel_bytes(t, n, name):
    """labels / mask as the kernels read them: uint8, one per voxel, dense and aligned."""
    t = _lib.dense16(t.reshape(-1).to(torch.uint8))
    if t.numel() != n:
        raise _lib.DhdError(f'occ_head_losses: {name} must have one element per voxel ({n}), got {t.numel()}')
    return t


def occ_head_loss_forward(x, w1, b1, w2, b2, labels, mask, cw, dz=16, ignore_index=255, non_empty_idx=17):
    """One dhdl_occ_head_loss_forward call on dense, aligned GPU tensors: x (B, 256, Dy, Dx) NCHW or channels_last, the
    parameters, labels and mask uint8 (B * Dx * Dy * dz,), cw float32 (18,) -> (logits (B, Dx, Dy, dz, 18) float32, losses (3,)
    float32, workspace).  Allocates its outputs and its scratch; nothing is cached."""
    b, c, dy, dx = x.shape
    layout = _layout_of(x)
    if layout is None:
        raise _lib.DhdError('occ_head_loss_forward: x must be dense, NCHW or channels_last')
    code, dev = _lib.dtype_code(x.dtype), x.device
    with torch.cuda.device(dev):
        wts, held = _weights(w1, b1, w2, b2, c, dz)
        fwd, bwd = C.c_size_t(), C.c_size_t()
        _occ_loss_head.call('dhdl_occ_head_loss_scratch_bytes', C.byref(wts), code, b, dy, dx, C.byref(fwd), C.byref(bwd))
        scratch = torch.empty(fwd.value, dtype=torch.uint8, device=dev)
        logits = torch.empty(b, dx, dy, dz, wts.n_classes, dtype=torch.float32, device=dev)
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        ws = torch.empty(_occ_loss_head.value('dhdl_occ_head_loss_workspace_bytes'), dtype=torch.uint8, device=dev)
        _occ_loss_head.call('dhdl_occ_head_loss_forward', _lib.ptr(x), code, layout, C.byref(wts), b, dy, dx, _lib.ptr(labels),
                            _lib.ptr(mask), _lib.ptr(cw), ignore_index, non_empty_idx, _lib.ptr(logits), _lib.ptr(losses), _lib.ptr(ws),
                            _lib.ptr(scratch), fwd.value, _lib.stream_ptr(dev))
    return logits, losses, ws


def occ_head_loss_backward(x, logits, labels, mask, cw, ws, glosses, w1, b1, w2, dz=16, ignore_index=255, non_empty_idx=17,
                           operands=True):
    """One dhdl_occ_head_loss_backward call: the forward's inputs, logits and workspace and glosses (3,) float32 on the device
    -> (dx, db1, db2, act, dhid, g) as occ_head_backward returns them, g in ghalf's place: for a float32 x always the float32
    dL/dlogits (the kernel's own operand), for a half x dL/dlogits rounded once, with `operands` only."""
    b, c, dy, dx = x.shape
    layout = _layout_of(x)
    if layout is None:
        raise _lib.DhdError('occ_head_loss_backward: x must be dense, NCHW or channels_last')
    code, dev, cells = _lib.dtype_code(x.dtype), x.device, b * dy * dx
    hidden, cols = w1.shape[0], w2.shape[0]
    with torch.cuda.device(dev):
        wts, held = _weights(w1, b1, w2, None, c, dz)
        dxo = torch.empty_like(x)
        db1 = torch.empty(hidden, dtype=torch.float32, device=dev)
        db2 = torch.empty(cols, dtype=torch.float32, device=dev)
        act = dhid = g = None
        if operands:
            act = torch.empty((cells, hidden), dtype=x.dtype, device=dev)
            dhid = torch.empty((cells, hidden), dtype=x.dtype, device=dev)
        if operands or x.dtype == torch.float32:
            g = torch.empty((cells, cols), dtype=x.dtype, device=dev)
        fwd, bwd = C.c_size_t(), C.c_size_t()
        _occ_loss_head.call('dhdl_occ_head_loss_scratch_bytes', C.byref(wts), code, b, dy, dx, C.byref(fwd), C.byref(bwd))
        scratch = torch.empty(bwd.value, dtype=torch.uint8, device=dev)
        _occ_loss_head.call('dhdl_occ_head_loss_backward', _lib.ptr(x), code, layout, C.byref(wts), b, dy, dx, _lib.ptr(logits),
                            _lib.ptr(labels), _lib.ptr(mask), _lib.ptr(cw), ignore_index, non_empty_idx, _lib.ptr(glosses), _lib.ptr(ws),
                            _lib.ptr(dxo), _lib.ptr(db1), _lib.ptr(db2), _lib.ptr(act), _lib.ptr(dhid), _lib.ptr(g), _lib.ptr(scratch),
                            bwd.value, _lib.stream_ptr(dev))
    return dxo, db1, db2, act, dhid, g


class _OccHeadLosses(torch.autograd.Function):
    """The three losses of the predicter MLP's logits; saves the dense x, the parameters, the float32 logits, the uint8 labels and
    mask, the class weights and the workspace of totals.  The backward is one dhdl_occ_head_loss_backward call and torch's two
    weight-gradient GEMMs on the operands it writes, as in _OccHeadTrain.backward."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, labels, mask, cw, dz, ignore_index, non_empty_idx):
        xd, layout = _dense_in_layout(x.detach())
        logits, losses, ws = occ_head_loss_forward(xd, w1, b1, w2, b2, labels, mask, cw, dz, ignore_index, non_empty_idx)
        ctx.save_for_backward(xd, w1, b1, w2, b2, logits, labels, mask, cw, ws)
        ctx.args = (dz, ignore_index, non_empty_idx)
        return losses

    @staticmethod
    @torch.autograd.function.once_differentiable
    @traced('dhd.occ_head.losses')
    def backward(ctx, glosses):
        x, w1, b1, w2, b2, logits, labels, mask, cw, ws = ctx.saved_tensors
        need = ctx.needs_input_grad
        gl = glosses.float().contiguous()
        with torch.autocast('cuda', enabled=False):
            dx, db1, db2, act, dhid, g = occ_head_loss_backward(x, logits, labels, mask, cw, ws, gl, w1, b1, w2, *ctx.args,
                                                                operands=need[1] or need[3])
            dw1 = dw2 = None
            if need[1]:
                b, c, dy, dxs = x.shape
                if x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
                    dw1 = dhid.t() @ x.permute(0, 2, 3, 1).reshape(-1, c)          # a view: x's pixels are dhid's rows
                else:                                                               # NCHW: one product per sample, summed
                    per = torch.bmm(dhid.view(b, dy * dxs, -1).transpose(1, 2), x.reshape(b, c, dy * dxs).transpose(1, 2))
                    dw1 = per[0] if b == 1 else per.sum(0, dtype=torch.float32)
                dw1 = dw1.to(w1.dtype)
            if need[3]:
                dw2 = (g.t() @ act).to(w2.dtype)
        return (dx if need[0] else None, dw1, db1.to(b1.dtype) if need[2] else None, dw2, db2.to(b2.dtype) if need[4] else None,
                None, None, None, None, None, None)


def occ_head_losses(x, w1, b1, w2, b2, labels, mask_camera, class_weight, dz=16, ignore_index=255, non_empty_idx=17):
    """(loss_occ, loss_voxel_sem_scal, loss_voxel_geo_scal) before the head's weight_* factors, of the predicter MLP on
    final_conv's output: occ_loss.occ_losses(occ_head_train(x, ...), labels, mask_camera, class_weight) as one operator,
    differentiable in x and the four parameters.  x (B, 256, Dy, Dx) float32 / float16 / bfloat16, NCHW or channels_last;
    labels / mask_camera (B, Dx, Dy, dz) of any integer or bool dtype (converted to uint8 once); class_weight (18,).

    The forward writes the float32 logits (occ_head_train's bytes) and, from the registers that hold them, the 56 sums the losses
    are functions of; the backward computes dL/dlogits in the head's backward kernel from the saved logits, the labels and the
    totals, so neither of occ_loss's two passes runs and no float32 gradient of the logits exists for a half x.  Saved between
    forward and backward: x, the parameters, the logits, the uint8 labels and mask, and 448 bytes of totals.  The upstream
    gradient is read on the device: a loss scale costs nothing, and forward + backward can be captured into a HIP graph.  Works
    under torch.autocast and checkpoint(..., use_reentrant=False).  No atomics: a repeated call gives the same bytes.  HIP only:
    a CPU tensor or an unsupported shape raises DhdError."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.DhdError(f'occ_head_losses: x must live on the GPU: dhd_amd runs only as HIP kernels (got {getattr(x, "device", None)})')
    if not loss_supported(x, w1, w2, dz):
        raise _lib.DhdError(f'occ_head_losses: no operator for x {tuple(x.shape)} of {x.dtype} with weights {tuple(w1.shape)}, '
                            f'{tuple(w2.shape)} and dz {dz}')
    for p, shape, name in ((w1, (512, 256), 'w1'), (b1, (512,), 'b1'), (w2, (dz * NUM_CLASSES, 512), 'w2'), (b2, (dz * NUM_CLASSES,), 'b2')):
        if not (torch.is_tensor(p) and p.is_cuda and tuple(p.shape) == shape):
            raise _lib.DhdError(f'occ_head_losses: {name} must be a GPU tensor of shape {shape}')
    n = x.shape[0] * x.shape[2] * x.shape[3] * dz
    labels = _voxel_bytes(labels.to(x.device), n, 'labels')
    mask = _voxel_bytes(mask_camera.to(x.device), n, 'mask_camera')
    cw = _lib.dense16(class_weight.detach().to(device=x.device, dtype=torch.float32))
    if cw.numel() != NUM_CLASSES:
        raise _lib.DhdError(f'occ_head_losses: class_weight must have {NUM_CLASSES} elements')
    out = _OccHeadLosses.apply(x, w1, b1, w2, b2, labels, mask, cw, dz, int(ignore_index), int(non_empty_idx))
    return out[0], out[1], out[2]
