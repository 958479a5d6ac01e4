"""One process of tests/test_gpu_sfa_bwd_fold.py: the SFA stage's training step at the module's shapes under the DHD_SFA_BWD_FOLD
value this process was started with (the library reads the switch once per process).

    python tests/sfa_bwd_fold_worker.py OUT.pt

Per shape: forward + backward twice (same bytes?), once more inside guard bands (tests/guarded_alloc.py), and the pieces of
`saved` / `scratch` the g-buffer check needs.  Everything goes to OUT.pt; this file asserts nothing about values itself beyond
the guard bands."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = ((128, 3, 36, 40),    # whole tiles
          (256, 2, 52, 60),    # 97.5 tiles per sample: a partial last tile
          (128, 2, 20, 28),    # 36 tiles, far fewer than workgroups: idle workgroups, repeated tiles
          (256, 6, 12, 20),    # the GEMM launcher splits the batch 4 + 2; 48 steps: most weight-gradient workers have none
          # more steps (32 pixels each, sample after sample) than the 256 weight-gradient workers, three samples, and a sample
          # boundary INSIDE a worker's range (straddling_workers below; the test asserts it): that worker flushes a dL/da row per
          # sample, and the summing kernel meets a worker that belongs to two samples
          (128, 3, 64, 64),    # 384 steps of whole tiles: worker 85 owns steps 127-128 across the boundary at 128
          (128, 3, 100, 100))  # 939 steps, 312.5 per sample: workers 85 (311-314) and 170 (623-626) straddle, behind a partial step
K_WORKERS = 256                # csrc/sfa_stage.hip: kWgWorkers
K_CHUNKS = 4                   # kPlaneChunks


def straddling_workers(b, h, w, workers=K_WORKERS):
    """[(worker, first step, end step)] of the weight-gradient workers whose steps belong to more than one sample: worker k owns
    the steps [n k // W, n (k + 1) // W) of the n = b * ceil(hw / 32) steps (csrc/sfa_stage.hip: wg_first_step)."""
    sps = (h * w + 31) // 32
    n = b * sps
    out = []
    for k in range(workers):
        first, end = n * k // workers, n * (k + 1) // workers
        if end > first and first // sps != (end - 1) // sps:
            out.append((k, first, end))
    return out


def inputs(c, b, h, w):
    """Stage (train mode, non-trivial BatchNorm state, bf16x3), x and the output gradient: CPU generator, the same in every process."""
    from dhd_amd.mix import channel_spatial_stage
    torch.manual_seed(1000 * c + h)
    st = channel_spatial_stage(2 * c)
    with torch.no_grad():
        for bn in (st.spacial_leanring[1], st.spacial_leanring[4]):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
    st.train()
    st.gemm = 'bf16x3'
    x = torch.randn(b, 2 * c, h, w) * 0.7 + 0.1
    g = torch.randn(b, c, h, w)
    return st, x, g


def scratch_offsets(b, c, hw, r):
    """scratch_layout (csrc/sfa_stage.hip) for float32 storage: byte offsets of the sections the check reads, and the total."""
    o, off = 0, {}

    def take(name, nbytes):
        nonlocal o
        off[name] = o
        o += (nbytes + 255) & ~255
    cc, plane = c * c, b * c * hw * 4
    take('wp1', 8 * cc); take('wp2', 8 * cc)
    take('part', 4 * b * K_CHUNKS * 2 * c)
    take('stat_part', 4 * b * ((hw + 31) // 32 + 64) * 2 * c)
    take('da1', 4 * b * K_CHUNKS * c); take('da2', 4 * b * K_CHUNKS * c)
    take('tab_g2', 4 * b * 3 * c); take('tab_g1', 4 * b * 3 * c)
    take('dpre2', 4 * b * c); take('dh', 4 * b * r); take('ds', 4 * b * 2 * c)
    take('mean_part', 4 * b * 2 * c * K_CHUNKS)
    take('g2', plane); take('g1', plane); take('du', plane)
    take('wpart', 4 * K_WORKERS * cc)
    off['total'] = o
    return off


def step(st, x, g, dev):
    import copy
    st = copy.deepcopy(st).to(dev)
    xd = x.to(dev).requires_grad_()
    out = st(xd)
    out.backward(g.to(dev), retain_graph=True)
    res = {'out': out.detach().clone(), 'gx': xd.grad.clone()}
    res.update({'d_' + k: p.grad.clone() for k, p in st.named_parameters()})
    return res, out


def main(out_path):
    import ctypes as C
    import guarded_alloc as G
    from dhd_amd import _lib, mix
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    results = {'fold': os.environ.get('DHD_SFA_BWD_FOLD', '')}
    for c, b, h, w in SHAPES:
        hw = h * w
        st, x, g = inputs(c, b, h, w)
        assert mix.fused_stage_supported(st.to(dev), x.to(dev))
        st = st.cpu()
        first, out = step(st, x, g, dev)
        torch.cuda.synchronize()
        # the workspaces of that call: `saved` from the autograd node, scratch from the pool (grow-only, one per device and stream)
        r = st.fc[0].weight.shape[0]
        off = scratch_offsets(b, c, hw, r)
        nsaved, nscratch = C.c_size_t(), C.c_size_t()
        _lib.check(lib.dhd_sfa_stage_workspace_bytes(b, c, hw, r, 0, C.byref(nsaved), C.byref(nscratch)), 'dhd_sfa_stage_workspace_bytes')
        assert off['total'] == nscratch.value, (off['total'], nscratch.value)
        saved = out.grad_fn.saved_tensors[1]
        assert saved.dtype == torch.uint8 and saved.numel() == nsaved.value
        scratch = mix._stage_scratch(dev, nscratch.value).view(torch.uint8)
        plane = b * c * hw * 4
        pa = (plane + 255) & ~255

        def f32(buf, at, n):
            return buf[at:at + 4 * n].clone().view(torch.float32)
        pieces = {'y1': f32(saved, nsaved.value - 2 * pa, b * c * hw).view(b, c, hw), 'y2': f32(saved, nsaved.value - pa, b * c * hw).view(b, c, hw),
                  'g2': f32(scratch, off['g2'], b * c * hw).view(b, c, hw), 'g1': f32(scratch, off['g1'], b * c * hw).view(b, c, hw),
                  'tab_g2': f32(scratch, off['tab_g2'], b * 3 * c).view(b, 3, c), 'tab_g1': f32(scratch, off['tab_g1'], b * 3 * c).view(b, 3, c)}
        del out, saved
        second, _ = step(st, x, g, dev)
        same = all(torch.equal(first[k].view(torch.uint8), second[k].view(torch.uint8)) for k in first)
        # once more with every buffer the wrapper allocates (out, saved, scratch, gradients) between guard bands, NaN-filled
        mp = pytest.MonkeyPatch()
        try:
            with G.guarded(mp, fill=0xFF) as ledger:
                third, _ = step(st, x, g, dev)
                torch.cuda.synchronize()
                ledger.check()
                n_guarded = len(ledger)
        finally:
            mp.undo()
        same_guarded = all(torch.equal(first[k].view(torch.uint8), third[k].view(torch.uint8)) for k in first)
        results[(c, b, h, w)] = dict(res={k: v.cpu() for k, v in first.items()}, pieces={k: v.cpu() for k, v in pieces.items()},
                                    same=same, same_guarded=same_guarded, n_guarded=n_guarded)
    torch.save(results, out_path)


if __name__ == '__main__':
    main(sys.argv[1])
