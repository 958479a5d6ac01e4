"""dhd_amd -- MI355X (gfx950) implementation of DHD's height-decoupled LSS view transform.

Host-side mirror of the reference's plugin surface for this path
(projects/mmdet3d_plugin: ops/bev_pool_v2, models/necks/lss_heightmap.py, models/necks/mix.py),
over the C ABI of csrc/libdhd_amd.so (include/dhd_amd.h).  Importing the package does not need
a GPU; calling any operator does, and fails loudly without the HIP library.
"""
from .registry import NECKS, BACKBONES, HEADS, DETECTORS, HOOKS, build_neck, build_backbone, build_head, build_detector, build_hook  # noqa: F401
from .bev_pool_v2 import bev_pool_v2, QuickCumsumCuda  # noqa: F401
from .lss_heightmap import MGHS, MGHS_Depth, MGHS_Stereo  # noqa: F401
from .mix import SFA, channel_spatial_stage  # noqa: F401
from .depthnet import HeightNet, DepthNet  # noqa: F401
from .detector import DHD  # noqa: F401  (also registers ResNet, CustomFPN, CustomResNet, FPN_LSS, UNet, Identity, predictor)
from .swin import SwinTransformer  # noqa: F401
from .ema import ModelEMA, MEGVIIEMAHook, SyncbnControlHook, SequentialControlHook  # noqa: F401
from .config import Config  # noqa: F401
from .checkpoint import load_checkpoint, load_state_dict, save_checkpoint  # noqa: F401
from .amp_weights import HalfWeightCache  # noqa: F401
from .optim import FusedAdamW, DynamicLossScale, build_optimizer  # noqa: F401
from .occ_head import occ_head_infer, occ_head_train, occ_head_losses  # noqa: F401
from . import deform_conv  # noqa: F401  (the module, callable as its function deform_conv)
from .deform_conv import deform_conv_infer, deform_conv_infer_supported, deform_conv_train_supported  # noqa: F401
from . import window_attn  # noqa: F401  (the module, callable as its function window_attn)
from .window_attn import window_attn_infer, window_attn_infer_supported, window_attn_supported  # noqa: F401
from .swin_glue import layer_norm_rows, window_reverse_add, swin_glue_supported  # noqa: F401
from . import swin_ffn  # noqa: F401  (the module, callable as its function swin_ffn)
from .swin_ffn import swin_ffn_infer, swin_ffn_supported, swin_ffn_train_supported, swin_ffn_train_wide_supported  # noqa: F401
from .swin_seam import patch_merge_norm, patch_embed_norm, swin_seam_supported  # noqa: F401
from .unet_seam import max_pool2x2, conv_transpose2x2_cat, unet_seam_supported, unet_seam_routed  # noqa: F401
from .stereo_cv import stereo_sampling_grid, stereo_cost_volume, stereo_cv_supported, stereo_cv_routed  # noqa: F401
from .ray_metrics import RayIoU, calc_rayiou, generate_lidar_rays, render_forward  # noqa: F401

__version__ = '0.1.0'


def fused_inference(model, enabled=True):
    """The one switch for the inference operators whose results are within their bars but not bit-identical to the module
    formulation: sets `fused_infer` on every occupancy head (`predictor`), every `DCN` and every Swin `WindowMSA` of `model` and
    returns the modules it switched.  They take their fused operator only in eval mode with nothing to differentiate, and only
    where it has the shape (window attention: head dimension 32, at most 144 tokens per window; under autocast it keeps the
    relative-position bias in float32 where the module formulation rounds it to the half type).  The second half of a Swin block
    has a switch of its own, `fused_swin_ffn`, which this one does not set."""
    from .depthnet import DCN
    from .detector import predictor
    from .swin import WindowMSA
    switched = [m for m in model.modules() if isinstance(m, (DCN, predictor, WindowMSA))]
    for m in switched:
        m.fused_infer = bool(enabled)
    return switched


def fused_training(model, on=True):
    """The training sibling of fused_inference: sets `fused_train` on every Swin `WindowMSA` of `model` and returns the modules it
    switched.  With it the attention between the two Linear layers runs as `window_attn` -- the fused forward on qkv as it lies
    and its fused HIP backward -- in train and eval mode, with or without grad, wherever the operator has the shape (head
    dimension 32, at most 144 tokens per window, a GPU tensor) and attention dropout is inactive; every other call keeps SDPA.
    Within the layer's bar of SDPA, not bit-identical; under autocast the relative-position bias and its gradient stay float32."""
    from .swin import WindowMSA
    switched = [m for m in model.modules() if isinstance(m, WindowMSA)]
    for m in switched:
        m.fused_train = bool(on)
    return switched


def fused_swin_glue(model, on=True):
    """Sets `fused_glue` on every `SwinBlock` of `model` and returns the blocks it switched.  With it a block's LayerNorms, window
    partition / reverse, DropPath and first residual add run as the operators of swin_glue.py (norm1 into the windows, reverse +
    add, norm2 into the dtype fc1 reads) wherever the windows are cut on the GPU, both norms are affine over the channels and
    the channel count is a multiple of 8 up to 2048; every other call keeps today's path.  The attention inside the windows and
    its own switches (fused_inference, fused_training) are untouched.  Within the layer's bar of torch's LayerNorm, not
    bit-identical; the random stream of an active DropPath is unchanged."""
    from .swin import SwinBlock
    switched = [m for m in model.modules() if isinstance(m, SwinBlock)]
    for m in switched:
        m.fused_glue = bool(on)
    return switched


def fused_swin_ffn(model, on=True):
    """Sets `fused_ffn` on every `SwinBlock` of `model` and returns the blocks it switched.  With it the second half of a block --
    norm2, fc1, GELU, fc2 and the residual add -- runs as the one operator of swin_ffn.py in eval mode with nothing to
    differentiate, wherever the operator has the shape (C = 128, 256, 512 or 1024 with mlp_ratio 4, a GPU tensor, two biased Linear
    layers around an exact GELU, an affine norm2) and the measurement routed that size and dtype to it (swin_ffn.ROUTED,
    swin_ffn.ROUTED_WIDE); every other
    call keeps today's path bit for bit.  It is a switch of its own and not part of fused_inference; it composes with
    fused_inference and fused_swin_glue.  Within the layer's bar of the module formulation, not bit-identical."""
    from .swin import SwinBlock
    switched = [m for m in model.modules() if isinstance(m, SwinBlock)]
    for m in switched:
        m.fused_ffn = bool(on)
    return switched


def fused_swin_ffn_training(model, on=True):
    """Sets `fused_ffn_train` on every `SwinBlock` of `model` and returns the blocks it switched.  With it the second half of a
    block -- norm2, fc1, GELU, fc2, DropPath and the residual add -- runs as `swin_ffn`, the fused forward and its recompute HIP
    backward, in train and eval mode, with or without grad, wherever the operator has the shape (C = 128 or 256 with mlp_ratio 4,
    a GPU tensor, two biased Linear layers around an exact GELU, an affine norm2), the FFN's dropout is inactive and the
    measurement routed that size and dtype to it (swin_ffn.ROUTED_TRAIN); every other call keeps today's path bit for bit.  The
    random stream of an active DropPath is unchanged.  It is a switch of its own: the other fused_* switches do not set it and
    it sets none of theirs.  Within the layer's bar of the module formulation, not bit-identical."""
    from .swin import SwinBlock
    switched = [m for m in model.modules() if isinstance(m, SwinBlock)]
    for m in switched:
        m.fused_ffn_train = bool(on)
    return switched


def fused_swin_ffn_training_wide(model, on=True):
    """Sets `fused_ffn_train_wide` on every `SwinBlock` of `model` and returns the blocks it switched: fused_swin_ffn_training's
    route at C = 512 (DHD-L's stage 2) through the wide training family -- the wide forward with DropPath's factor and its
    recompute HIP backward -- under the same conditions, wherever the measurement routed that dtype combination to it
    (swin_ffn.ROUTED_TRAIN_WIDE); every other call keeps today's path bit for bit.  The random stream of an active DropPath is
    unchanged.  It is a switch of its own: fused_swin_ffn_training does not set it and it does not set that one, so a model with
    only the other switches on makes the calls it made before.  C = 1024 has no training operator."""
    from .swin import SwinBlock
    switched = [m for m in model.modules() if isinstance(m, SwinBlock)]
    for m in switched:
        m.fused_ffn_train_wide = bool(on)
    return switched


def fused_occ_head_training(model, on=True):
    """Sets `fused_train` on every occupancy head (`predictor`) of `model` and returns the heads it switched.  With it the head's
    predicter -- Linear, Softplus, Linear per BEV cell -- runs as `occ_head_train`, the fused forward that writes float32 logits
    and its recompute HIP backward, in train and eval mode, with or without grad, wherever the operator has the shape (256
    channels, 512 hidden units, 16 x 18 logits, a GPU tensor) and the measurement routed that dtype and layout to it
    (occ_head.ROUTED_TRAIN); every other call keeps today's path bit for bit.  It is a switch of its own: fused_inference and
    `predict_occ` are untouched and it sets none of the other switches.  Within the layer's bar of the module formulation, not
    bit-identical; under autocast the logits come out in float32 where the module formulation hands the loss a half tensor to cast."""
    from .detector import predictor
    switched = [m for m in model.modules() if isinstance(m, predictor)]
    for m in switched:
        m.fused_train = bool(on)
    return switched


def fused_occ_head_loss(model, on=True):
    """Sets `fused_loss` on every occupancy head (`predictor`) of `model` and returns the heads it switched.  With it
    `DHD.forward_occ_train` takes `predictor.forward_loss`: final_conv, then the predicter and the three losses as one operator,
    `occ_head_losses` -- the loss sums ride in the head's forward kernel and the gradient of the logits is computed inside the
    head's backward kernel -- wherever the operator has the shape and the measurement routed that dtype and layout to it
    (occ_head.ROUTED_LOSS); every other call keeps today's two calls bit for bit.  It is a switch of its own: it sets none of
    the other switches, and `predictor.forward` and `predictor.loss` are untouched.  Within the bars of occ_head_train and
    occ_losses, not bit-identical to them."""
    from .detector import predictor
    switched = [m for m in model.modules() if isinstance(m, predictor)]
    for m in switched:
        m.fused_loss = bool(on)
    return switched


def fused_dcn_training(model, on=True):
    """Sets `fused_train` on every `DCN` of `model` and returns the modules it switched.  With it the deformable convolution of the
    HeightNet / DepthNet stacks runs as `deform_conv` -- the fused forward of the inference operator and its HIP backward, which
    neither keeps the column matrix nor writes its gradient -- in train and eval mode, with or without grad, wherever the operator
    has the shape (3 x 3, C / groups and O / groups multiples of 8 up to 128, a map of at most 853 cells, a GPU tensor) and the
    measurement routed that dtype and layout to it (deform_conv.ROUTED_TRAIN); every other call keeps today's path bit for bit.  It
    is a switch of its own: fused_inference is untouched and it sets none of the other switches.  Within the layer's bar of
    today's path, not bit-identical."""
    from .depthnet import DCN
    switched = [m for m in model.modules() if isinstance(m, DCN)]
    for m in switched:
        m.fused_train = bool(on)
    return switched


def fused_swin_seams(model, on=True):
    """Sets `fused_seam` on every `PatchMerging` and `PatchEmbed` of `model` and returns the modules it switched.  With it the seam
    at a stage boundary runs as an operator of swin_seam.py, in train and eval mode: patch merging's 2 x 2 gather, LayerNorm over
    4C and cast to the dtype `reduction` reads as `patch_merge_norm` (stride 2, C a multiple of 8 up to 512, an affine norm with a
    bias), and patch embedding's transposition of the conv output and LayerNorm as `patch_embed_norm` (C a multiple of 8 up to
    256) -- wherever the tensor is on the GPU and the measurement routed that size and dtype to the operator
    (swin_seam.ROUTED); every other call keeps today's path bit for bit.  It is a switch of its own: the other fused_* switches
    do not set it and it sets none of theirs.  Within the layer's bar of torch's LayerNorm, not bit-identical."""
    from .swin import PatchEmbed, PatchMerging
    switched = [m for m in model.modules() if isinstance(m, (PatchEmbed, PatchMerging))]
    for m in switched:
        m.fused_seam = bool(on)
    return switched


def fused_unet_seams(model, on=True):
    """Sets `fused_seam` on every `_Down` and `_Up` of the UNets of `model` and returns the modules it switched.  With it the
    MaxPool2d(2) of `_Down` runs as `max_pool2x2` -- no index tensor, the backward recomputes the winners from the skip tensor --
    and ConvTranspose2d + pad + cat of `_Up` (bilinear=False) as `conv_transpose2x2_cat`, one launch that writes the concatenated
    tensor, in train and eval mode, with or without grad, wherever the tensors are on the GPU, the operator has the shape
    (unet_seam_supported) and the measurement routed that channel count, dtype and layout to it (unet_seam.ROUTED); every other
    call, and `_Up` with bilinear=True, keeps today's path bit for bit.  It is a switch of its own: it sets none of the other
    switches.  The pooling is torch's bit for bit; the up seam is within the layer's bar of today's path, not bit-identical."""
    from .detector import _Down, _Up
    switched = [m for m in model.modules() if isinstance(m, (_Down, _Up))]
    for m in switched:
        m.fused_seam = bool(on)
    return switched


def fused_stereo_cost_volume(model, on=True):
    """Sets `fused_cost_volume` on every HeightNet / DepthNet of `model` and returns the modules it switched.  With it
    `calculate_cost_volumn` (the temporal DepthNet of DHD-M and DHD-L) runs as `stereo_cost_volume`: the sampling positions of
    `gen_grid` are evaluated inside the kernel from the camera matrices, and the stereo features are read in their own dtype
    (float32, float16, bfloat16), in place where their memory is NHWC -- wherever the call is supported (stereo_cv_supported) and
    the measurement routed that channel class and dtype to it (stereo_cv.ROUTED).  A feature shape the operator does not take, with
    a separable frustum, gets its grid from `stereo_sampling_grid` and keeps today's kernel; every other call keeps today's path bit
    for bit.  float32 results are today's bytes; half results are within 1e-4 + 2 eps |ref| of today's.  It is a switch of its
    own: it sets none of the other switches."""
    from .depthnet import _LiftNetBase
    switched = [m for m in model.modules() if isinstance(m, _LiftNetBase)]
    for m in switched:
        m.fused_cost_volume = bool(on)
    return switched
