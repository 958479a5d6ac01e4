"""The shared input definition of the occupancy-head training tests (test_occ_head_train_capi.py, test_gpu_occ_head_train.py): the
head and the x of occ_head_inputs.py, a gradient of the logits as the loss kernel writes it, the float64 autograd twin and the
same-dtype chain the half bars are stated against.  Everything here is computed once per (shape, precision) and never modified."""
import functools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_head_inputs as OH  # noqa: E402

C, HIDDEN, DZ, N_CLS, COLS = OH.C, OH.HIDDEN, OH.DZ, OH.N_CLS, OH.DZ * OH.N_CLS

# (B, Dy, Dx): the smallest shapes that reach every way the kernel can go wrong
SHAPES = {
    'one_cell': (1, 1, 1),          # one live lane (pair)
    'partial_wave': (2, 7, 9),      # one partial wave per sample
    'two_groups': (1, 12, 11),      # two workgroups, the second with one live lane group
    'tails': (3, 20, 28),           # Dy != Dx, 15 workgroups of partial rows, a tail in every sample
}
PRECISIONS = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}      # the dtype of x = the GEMM type
LAYOUTS = ('nchw', 'nhwc')
GRID = [(s, p, l) for s in SHAPES for p in PRECISIONS for l in LAYOUTS]
PARAMS = ('w1', 'b1', 'w2', 'b2')
TENSORS = ('dx', 'dw1', 'db1', 'dw2', 'db2')


@functools.lru_cache(maxsize=None)
def make_glogits(shape, seed=5):
    """(B, Dy, Dx) -> dL/dlogits (B, Dx, Dy, DZ, N_CLS) float32 on the CPU: N(0, 1) with whole voxels zeroed at random (about 30 %),
    as the voxels outside the camera mask are."""
    b, dy, dx = shape
    gen = torch.Generator().manual_seed(seed + 1000 * b + 10 * dy + dx)
    g = torch.randn(b, dx, dy, DZ, N_CLS, generator=gen)
    keep = torch.rand(b, dx, dy, DZ, 1, generator=gen) >= 0.3
    return g * keep


@functools.lru_cache(maxsize=None)
def inputs(case, prec):
    """x (B, C, Dy, Dx) in the precision's dtype (NCHW, dense), the float32 parameters, glogits: CPU tensors, shared, read-only."""
    shape = SHAPES[case]
    w1, b1, w2, b2 = OH.head_params(OH.make_head())
    return dict(x=OH.make_x(shape).to(PRECISIONS[prec]), w1=w1, b1=b1, w2=w2, b2=b2, glogits=make_glogits(shape))


def in_layout(x, layout):
    """x dense in `layout`: the same values, NCHW or channels_last strides."""
    return x.contiguous(memory_format=torch.channels_last) if layout == 'nhwc' else x.contiguous()


def scale_of(t):
    return max(1.0, float(t.abs().max()))


def _collect(logits, leaves):
    out = {'logits': logits.detach(), 'dx': leaves['x'].grad}
    out.update({'d' + k: leaves[k].grad for k in PARAMS})
    return out


def formulation(x, w1, b1, w2, b2, r=lambda t: t):
    """The module formulation on x (B, C, Dy, Dx): permute(0, 3, 2, 1), Linear, Softplus, Linear -> (B, Dx, Dy, DZ, N_CLS); `r`
    rounds where an autocast region rounds (autocast_chain_logits of occ_head_inputs.py)."""
    h = r(F.linear(r(OH.cells_of(x)), r(w1), r(b1)))
    h = r(F.softplus(h))
    lg = r(F.linear(h, r(w2), r(b2)))
    return lg.view(*lg.shape[:3], DZ, N_CLS)


@functools.lru_cache(maxsize=None)
def twin(case, prec):
    """float64 autograd on the CPU through F.linear / F.softplus, from x as the operator reads it (rounded to the precision's
    dtype) and the float32 parameters -> logits, dx (B, C, Dy, Dx), dw1, db1, dw2, db2, all float64."""
    v = inputs(case, prec)
    leaves = {k: v[k].double().requires_grad_() for k in ('x',) + PARAMS}
    logits = formulation(*(leaves[k] for k in ('x',) + PARAMS))
    logits.backward(v['glogits'].double())
    return _collect(logits, leaves)


def chain(v, dtype, device):
    """torch autograd over the same formulation in the same dtypes: operands rounded to `dtype`, float32 accumulation, every
    intermediate rounded (forward and, through the casts' own backward, the gradients), the logits cast to float32 before
    glogits comes back -- what an autocast region computes for a half x and float32 parameters.  float32: plain autograd."""
    r = (lambda t: t) if dtype == torch.float32 else (lambda t: t.to(dtype).float())
    leaves = {k: v[k].to(device).float().requires_grad_() for k in ('x',) + PARAMS}
    logits = formulation(*(leaves[k] for k in ('x',) + PARAMS), r=r)
    logits.backward(v['glogits'].to(device))
    return _collect(logits, leaves)


# ---------------------------------------------------------------------------------------------------------------------------
# module level: predictor.forward -> loss -> backward

MODULE_SHAPE = (2, 7, 9)                                    # (B, Dy, Dx): one partial wave per sample
F16_MIN_NORMAL = 2.0 ** -14


@functools.lru_cache(maxsize=None)
def module_head(seed=7):
    """A predictor whose loss is defined (class-balanced, camera-masked), with occ_head_inputs' scaling of the two Linear layers."""
    from dhd_amd.detector import predictor
    torch.manual_seed(seed)
    head = predictor(C, C, DZ, num_classes=N_CLS, class_balance=True)
    with torch.no_grad():
        for lin in (head.predicter[0], head.predicter[2]):
            lin.weight.mul_(3.0)
            lin.bias.uniform_(-0.5, 0.5)
    return head.train()


@functools.lru_cache(maxsize=None)
def module_inputs(seed=11):
    """img_feats (B, C, Dy, Dx) float32, voxel_semantics (B, Dx, Dy, DZ) uint8 in [0, 18), mask_camera of the same shape (70 % set)."""
    b, dy, dx = MODULE_SHAPE
    gen = torch.Generator().manual_seed(seed)
    feats = torch.randn(b, C, dy, dx, generator=gen)
    sem = torch.randint(0, N_CLS, (b, dx, dy, DZ), generator=gen).to(torch.uint8)
    cam = torch.rand(b, dx, dy, DZ, generator=gen) < 0.7
    return feats, sem, cam


@functools.lru_cache(maxsize=None)
def module_twin():
    """The float64 twin on the CPU of head.forward -> head.loss -> backward of the sum of the three losses.  The loss's torch
    formulation casts to float32 inside, so its float64 spelling, occ_losses_f64 of value_edge_inputs.py, stands for it.
    -> dict: 'losses' (3,) float64, 'glogits' (dL/dlogits), 'dfeats', and 'd<name>' for every parameter of the head."""
    import copy
    import value_edge_inputs as VE
    head = copy.deepcopy(module_head()).double()
    feats, sem, cam = module_inputs()
    x = feats.double().requires_grad_()
    logits = head(x)
    logits.retain_grad()
    losses, _, _ = VE.occ_losses_f64(logits.reshape(-1, N_CLS), sem.reshape(-1).long(), cam.reshape(-1), head.cls_weights)
    sum(losses).backward()
    out = {'losses': torch.stack([l.detach() for l in losses]), 'glogits': logits.grad, 'dfeats': x.grad}
    out.update({'d' + n: p.grad for n, p in head.named_parameters()})
    return out


def starved_fraction(scale):
    """The share of the twin's non-zero glogits that, times `scale`, fall below fp16's smallest normal."""
    g = module_twin()['glogits'].abs()
    g = g[g > 0]
    return float((g * scale < F16_MIN_NORMAL).double().mean())


@functools.lru_cache(maxsize=None)
def fp16_loss_scale():
    """The smallest power of two, as a GradScaler would hold, with fewer than 1 % of the twin's non-zero glogits starved."""
    for k in range(0, 25):
        if starved_fraction(2.0 ** k) < 0.01:
            return 2.0 ** k
    raise AssertionError('no scale up to 2^24 keeps the gradient of the logits in fp16')
