"""Fixture G20: the Swin backbone at DHD-L's widths (embed 128, heads 4 / 8 / 16 / 32, window 12, four stages of two blocks, one
plain and one shifted), run by the reference's models/backbones/swin.py in float64.  What the generator
(tests/golden/make_golden.py g20) and the tests share lives here: the constructor arguments, the weight rule, the input, the loss,
the one function that runs a network and records what the fixture holds, and the reader / writer of the fixture's files.

Nothing here imports the reference: `record` takes any module with the reference's structure (patch_embed, drop_after_pos,
stages[i] returning (x_down, down_hw, x, hw), norm{i}, WindowMSA modules named `w_msa`), which both the reference's
SwinTransformer and dhd_amd.swin.SwinTransformer have.

The 36.3 M weights are not stored; they are a pure function of integer hashes (`set_state`), and the fixture stores the SHA-256
of the float64 state.  Every value is a float32 number (the rule is evaluated in float32 and widened), so a float32 copy of the
network carries the fixture's weights exactly.

The token maps are 24 x 34 -> 12 x 17 -> 6 x 9 -> 3 x 5: window padding in every stage, an odd size at every merge, 12 / 4 / 1 / 1
windows per image, region boundaries inside the shifted blocks of stages 0 and 1.

Files.  No file of the repository exceeds 1 MiB, and the fixture is about 5 MB of float64 that does not compress, so it is
written as g20_swin_dhdl.npz (the small entries) plus g20_swin_dhdl.<k>.npz shards; an array too large for one shard is cut
along its first axis into `name@i` pieces.  `load` puts them back together.
"""
import glob
import hashlib
import math
import os

import numpy as np
import torch

from dhd_amd import synthetic as syn

ARGS = dict(embed_dims=128, patch_size=4, window_size=12, depths=(2, 2, 2, 2), num_heads=(4, 8, 16, 32), strides=(4, 2, 2, 2),
            out_indices=(2, 3), drop_path_rate=0.1, with_cp=False, return_stereo_feat=True)
X_SHAPE = (2, 3, 96, 136)
MAPS = ((24, 34), (12, 17), (6, 9), (3, 5))
WIDTHS = (128, 256, 512, 1024)
OUT_SHAPES = ((2, 128, 24, 34), (2, 512, 6, 9), (2, 1024, 3, 5))
FULL_GRAD_MAX = 65536          # parameters up to this many elements have their whole gradient in the fixture, the Linear weights
                               # excepted (`full_grad`): bias tables, norms, biases and the patch conv, 0.5 MB; the Linear weights
                               # under the limit would add another 4.2 MB.  Every parameter has its norm and a projection.
STEM = 'g20_swin_dhdl'
SHARD_BYTES = 1000000          # under the repository's limit of 1 MiB per file, zip overhead included


# ------------------------------------------------------------------------------------------------ weights, input, loss

def state_value(j, key, shape):
    """The value of the floating-point state entry `key` (the j-th of state_dict()) as float64 holding float32 numbers."""
    h = syn.hash_signed(1000 + j, tuple(shape))
    if 'relative_position_bias_table' in key:
        v = h
    elif len(shape) >= 2:
        v = h * np.float32(math.sqrt(3.0 / int(np.prod(shape[1:]))))          # fan_in = v[0].numel(): uniform-like variance 1 / fan_in
    elif key.endswith('weight'):
        v = np.float32(1.0) + np.float32(0.25) * h                           # the norms
    else:
        v = np.float32(0.25) * h
    assert v.dtype == np.float32
    return v.astype(np.float64)


def set_state(net):
    """Fill the floating-point state of `net` (any dtype) by the rule; -> SHA-256 of the concatenated float64 values in
    state_dict() order."""
    sha = hashlib.sha256()
    with torch.no_grad():
        for j, (k, v) in enumerate(net.state_dict().items()):
            if not v.dtype.is_floating_point:
                continue
            a = state_value(j, k, tuple(v.shape))
            sha.update(a.tobytes())
            v.copy_(torch.from_numpy(a))
    return sha.hexdigest()


def x_input():
    return syn.hash_signed(1999, X_SHAPE).astype(np.float64)


def loss_weight(i, shape):
    return syn.hash_signed(2000 + i, tuple(shape)).astype(np.float64)


def grad_probe(j, shape):
    return syn.hash_signed(3000 + j, tuple(shape)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ one recorded run

def scores_of(msa, x):
    """max |scale q k^T + relative-position bias| of a WindowMSA for the windows x (..., N, C): what enters the softmax, the shift
    mask left out (-100 there by construction)."""
    N, C = x.shape[-2:]
    nh = msa.num_heads
    with torch.no_grad():
        qkv = msa.qkv(x.reshape(-1, N, C)).view(-1, N, 3, nh, C // nh)
        s = torch.einsum('wihd,wjhd->whij', qkv[:, :, 0], qkv[:, :, 1]) * msa.scale
        bias = msa.relative_position_bias_table[msa.relative_position_index.reshape(-1)].view(N, N, nh).permute(2, 0, 1)
        return float((s + bias.unsqueeze(0)).abs().max())


def first_stage(net, x):
    """The stage-0-only path of the extra stereo frame (detectors/bevstereo4d.py:41-54), restated on the modules."""
    if hasattr(net, 'forward_first_stage'):
        return net.forward_first_stage(x)
    tok = net.patch_embed(x)
    _, _, o0, hw0 = net.stages[0](net.drop_after_pos(tok), (net.patch_embed.DH, net.patch_embed.DW))
    return o0.view(-1, *hw0, net.num_features[0]).permute(0, 3, 1, 2).contiguous()


def forward_with_maps(net, x):
    """-> (outs, [the un-normalised (B, L, C) token map after each stage])."""
    maps, hooks = [], [s.register_forward_hook(lambda m, a, out: maps.append(out[2].detach())) for s in net.stages]
    try:
        outs = net(x)
    finally:
        for h in hooks:
            h.remove()
    return outs, maps


def backward_of(outs):
    sum((o * torch.from_numpy(loss_weight(i, o.shape)).to(o)).sum() for i, o in enumerate(outs)).backward()


def full_grad(name, p):
    return p.numel() <= FULL_GRAD_MAX and (p.dim() != 2 or 'relative_position_bias_table' in name)


def grad_summaries(net):
    """-> {key: value} for every parameter in named_parameters() order, j its index in state_dict(): gnorm.<name>, gproj.<name>
    (float64 scalars), and grad.<name> whole where `full_grad`."""
    index = {k: j for j, k in enumerate(net.state_dict())}
    out = {}
    for name, p in net.named_parameters():
        g = p.grad.detach().double().cpu().numpy()
        out['gnorm.' + name] = np.array(np.sqrt((g * g).sum()))
        out['gproj.' + name] = np.array((g * grad_probe(index[name], g.shape)).sum())
        if full_grad(name, p):
            out['grad.' + name] = g
    return out


def record(net):
    """Run `net` (float64, eval mode, weights set) forward and backward on the CPU; -> the entries of the fixture."""
    g = {}
    smax, hooks = [], [m.register_forward_pre_hook(lambda m, a: smax.append(scores_of(m, a[0].detach())))
                       for n, m in net.named_modules() if n.endswith('w_msa')]
    x = torch.from_numpy(x_input()).requires_grad_()
    outs, maps = forward_with_maps(net, x)
    for h in hooks:
        h.remove()
    backward_of(outs)
    for i, o in enumerate(outs):
        g[f'out{i}'] = o.detach().numpy()
    for i, m in enumerate(maps):
        g[f'map{i}'] = m.numpy()
    g['x_grad'] = x.grad.numpy()
    g['score_max'] = np.array(smax)
    g.update(grad_summaries(net))
    with torch.no_grad():
        g['stage0'] = first_stage(net, x.detach()).numpy()
    return g


# ------------------------------------------------------------------------------------------------ the fixture's files

def save(directory, g):
    """Write g as STEM.npz + STEM.<k>.npz, none above SHARD_BYTES."""
    pieces = []
    for k, a in g.items():
        a = np.asarray(a)
        n = -(-a.nbytes // (SHARD_BYTES - 4096)) if a.nbytes > SHARD_BYTES - 4096 else 1
        if n == 1:
            pieces.append((k, a))
        else:
            assert a.shape[0] >= n, k
            pieces += [(f'{k}@{i}', c) for i, c in enumerate(np.array_split(a, n, axis=0))]
    shards, room = [{}], SHARD_BYTES
    for k, a in sorted(pieces, key=lambda p: -p[1].nbytes):              # first fit, largest first
        need = a.nbytes + 512 + 2 * len(k)
        for s in shards:
            if s.setdefault('__used__', 0) + need <= room:
                s[k] = a
                s['__used__'] += need
                break
        else:
            shards.append({k: a, '__used__': need})
    shards.sort(key=lambda s: s['__used__'])                             # the smallest entries end up in STEM.npz
    for old in glob.glob(os.path.join(directory, STEM + '*.npz')):
        os.remove(old)
    for i, s in enumerate(shards):
        s.pop('__used__')
        path = os.path.join(directory, STEM + ('.npz' if i == 0 else f'.{i}.npz'))
        np.savez_compressed(path, **s)
        assert os.path.getsize(path) <= 1 << 20, path


def load(directory):
    """-> {name: array} of the whole fixture."""
    parts = {}
    for path in sorted(glob.glob(os.path.join(directory, STEM + '*.npz'))):
        with np.load(path) as z:
            for k in z.files:
                parts[k] = z[k]
    g, cut = {}, {}
    for k, a in parts.items():
        if '@' in k:
            name, i = k.rsplit('@', 1)
            cut.setdefault(name, {})[int(i)] = a
        else:
            g[k] = a
    for name, d in cut.items():
        g[name] = np.concatenate([d[i] for i in range(len(d))], axis=0)
    return g
