"""The occupancy head at inference as one HIP operator (csrc/occ_head.hip, section 14 of include/dhd_amd.h):
predictor.forward after final_conv (models/dense_heads/occ_head.py:84-100: Linear -> Softplus -> Linear per BEV cell) and
get_occ (:141-153) in one kernel that writes the uint8 class grid, and on request the mIoU histogram and the float32 logits.
The (cells, 512) hidden and the (cells, 288) logits of the module formulation never reach memory."""
import ctypes as C

import torch

from . import _lib
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
