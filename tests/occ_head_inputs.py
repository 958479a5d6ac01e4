"""The shared input definition of the occupancy-head inference tests (test_occ_head_infer_capi.py, test_gpu_occ_head_infer.py):
a predictor(256, 256, 16, num_classes=18) whose two Linear weights are scaled x3 and whose biases are uniform(-0.5, 0.5), fed
x ~ N(0, 1) as final_conv's output.  On 4096 cells the float64 logits have std 2.3 and every one of the 18 classes wins
somewhere, so an argmax test cannot pass on a constant map."""
import functools

import torch
import torch.nn.functional as F

C, HIDDEN, DZ, N_CLS = 256, 512, 16, 18


@functools.lru_cache(maxsize=None)
def make_head(seed=0):
    from dhd_amd.detector import predictor
    torch.manual_seed(seed)
    head = predictor(C, C, DZ, num_classes=N_CLS)
    with torch.no_grad():
        for lin in (head.predicter[0], head.predicter[2]):
            lin.weight.mul_(3.0)
            lin.bias.uniform_(-0.5, 0.5)
    return head.eval()


def head_params(head, device=None):
    lin1, lin2 = head.predicter[0], head.predicter[2]
    return [p.detach().to(device) if device is not None else p.detach() for p in (lin1.weight, lin1.bias, lin2.weight, lin2.bias)]


@functools.lru_cache(maxsize=None)
def make_x(shape, seed=2):
    """(B, Dy, Dx) -> x (B, C, Dy, Dx) float32, NCHW, on the CPU.  The seed is one for which none of the 16 voxels of the
    single-cell case (1, 1, 1) has a float64 top-2 margin inside fp16's near-tie band (with seed 1 one voxel has: 6.25 % of that
    grid, above the 5 % at which the class-map test calls itself vacuous); a property of the float64 reference alone."""
    b, dy, dx = shape
    return torch.randn(b, C, dy, dx, generator=torch.Generator().manual_seed(seed + 1000 * b + 10 * dy + dx))


def cells_of(x):
    """(B, C, Dy, Dx) -> (B, Dx, Dy, C): the reference's permute(0, 3, 2, 1)."""
    return x.permute(0, 3, 2, 1)


@functools.lru_cache(maxsize=None)
def reference_logits(shape):
    """float64 torch on the CPU of W2 . softplus(W1 . x + b1) + b2 -> (B, Dx, Dy, DZ, N_CLS)."""
    w1, b1, w2, b2 = (p.double() for p in head_params(make_head()))
    v = cells_of(make_x(shape)).double()
    lg = F.linear(F.softplus(F.linear(v, w1, b1)), w2, b2)
    return lg.view(*lg.shape[:3], DZ, N_CLS)


@functools.lru_cache(maxsize=None)
def autocast_chain_logits(shape, dtype):
    """What an autocast region computes: operands rounded to `dtype`, float32 accumulation, Linear-1's output rounded, Softplus
    in float32, rounded, Linear-2, rounded (returned as float32)."""
    r = lambda t: t.to(dtype).float()
    w1, b1, w2, b2 = (r(p) for p in head_params(make_head()))
    v = r(cells_of(make_x(shape)))
    h = r(F.linear(v, w1, b1))
    h = r(F.softplus(h))
    lg = r(F.linear(h, w2, b2))
    return lg.view(*lg.shape[:3], DZ, N_CLS)


def first_argmax(logits):
    """First-maximum argmax over the last axis, as uint8 (torch.argmax does not promise which maximum it returns)."""
    m = logits.max(-1, keepdim=True).values
    idx = torch.arange(logits.shape[-1], device=logits.device).expand_as(logits)
    return torch.where(logits == m, idx, logits.shape[-1]).min(-1).values.to(torch.uint8)
