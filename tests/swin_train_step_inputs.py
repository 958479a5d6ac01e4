"""The Swin training step as DHD-L runs it -- train mode with DropPath drawing, checkpointed blocks, autocast -- against float64.

The reference is a float64 CPU copy of dhd_amd.swin.SwinTransformer with G20's weights, input and loss (tests/swin_wide_inputs.py),
run in train mode.  torch.rand in float64 on the CPU draws other numbers than the GPU's generator does in float32 or a half type,
so the reference does not draw: the per-image masks floor(keep + u) of the run under test are recorded once on today's path
(`record_masks`) and replayed into the float64 network (`replay`).  A DropPath of rate 0 draws nothing and takes no mask, as in
DropPath.forward.

drop_path_rate is 0.5: the eight blocks have rates 0, 1/14, ..., 1/2, so block 0 draws nothing and the other seven draw twice
each (the attention's DropPath, then the FFN's): 14 masks per step, in the order the modules run."""
import contextlib

import torch

import swin_wide_inputs as SW

DROP_PATH_RATE = 0.5
ARGS = {**SW.ARGS, 'drop_path_rate': DROP_PATH_RATE}
DRAWS = 14


def net(with_cp=False, **kw):
    """A SwinTransformer at G20's sizes with drop_path_rate 0.5 (float32, on the CPU, in train mode, weights not set)."""
    from dhd_amd.swin import SwinTransformer
    return SwinTransformer(**{**ARGS, 'with_cp': with_cp, **kw}).train()


def drop_paths(model):
    """[(name, module)] of the DropPath modules that draw in train mode, in the order a forward runs them: per block the
    attention's, then the FFN's."""
    from dhd_amd.swin import SwinBlock
    found = []
    for name, block in model.named_modules():
        if isinstance(block, SwinBlock):
            for sub, dp in (('attn.drop', block.attn.drop), ('ffn.dropout_layer', block.ffn.dropout_layer)):
                if dp.drop_prob != 0.:
                    found.append((f'{name}.{sub}', dp))
    return found


@contextlib.contextmanager
def record_masks(model):
    """Within the block every DropPath of the process runs DropPath.forward's own expression and appends its mask.floor() to the
    list this yields.  Meant for today's path (every switch off, with_cp=False: a checkpointed block would draw, and record,
    twice); a step of `model` appends len(drop_paths(model)) masks."""
    from dhd_amd.swin import DropPath
    masks, real = [], DropPath.forward

    def forward(self, x):
        if self.drop_prob == 0. or not self.training:
            return x
        keep = 1 - self.drop_prob
        mask = keep + torch.rand((x.shape[0],) + (1,) * (x.dim() - 1), dtype=x.dtype, device=x.device)
        masks.append(mask.floor())
        return x.div(keep) * mask.floor()

    DropPath.forward = forward
    try:
        yield masks
    finally:
        DropPath.forward = real


@contextlib.contextmanager
def replay(net64, masks):
    """Within the block every drawing DropPath returns x.div(keep) * next(masks) instead of drawing; yields a one-element list that
    holds how many masks were taken.  `masks` is any iterable of tensors that broadcast against (B, 1, 1) in net64's dtype."""
    from dhd_amd.swin import DropPath
    it, taken, real = iter(masks), [0], DropPath.forward

    def forward(self, x):
        if self.drop_prob == 0. or not self.training:
            return x
        taken[0] += 1
        return x.div(1 - self.drop_prob) * next(it).to(x)

    DropPath.forward = forward
    try:
        yield taken
    finally:
        DropPath.forward = real


def step(model, x, autocast=None):
    """One forward and backward of G20's loss on x (a leaf is made of it) -> (outs, x.grad, {name: grad}), all detached."""
    x = x.detach().clone().requires_grad_()
    model.zero_grad(set_to_none=True)
    with torch.autocast(x.device.type, dtype=autocast or torch.bfloat16, enabled=autocast is not None):
        outs = model(x)
    SW.backward_of(outs)
    return [o.detach() for o in outs], x.grad, {n: p.grad for n, p in model.named_parameters()}


def reference_step(masks, state=None, threads=8):
    """The float64 step on the CPU with `masks` replayed -> (outs, x_grad, {name: grad}, masks taken); at most `threads` threads.
    `state` is a float32 state dict that already holds G20's weights (every value is a float32 number, so widening is exact), which
    saves hashing them again."""
    had = torch.get_num_threads()
    torch.set_num_threads(min(had, threads))
    try:
        net64 = net().double()
        if state is None:
            SW.set_state(net64)
        else:
            net64.load_state_dict({k: v.detach().cpu().double() if v.dtype.is_floating_point else v.cpu() for k, v in state.items()})
        with replay(net64, masks) as taken:
            outs, xg, grads = step(net64, torch.from_numpy(SW.x_input()))
        return outs, xg, grads, taken[0]
    finally:
        torch.set_num_threads(had)
