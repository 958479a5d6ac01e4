"""One process of tests/test_gpu_sfa_bwd_pair1.py: the SFA stage's training step at the module's shapes under the DHD_SFA_BWD_FOLD
value this process was started with (the library reads the switch once per process).

    python tests/sfa_bwd_pair1_worker.py OUT.pt

tests/sfa_bwd_pair_worker.py's run (its shapes, inputs, step and guard bands) with one more shape and one more piece of scratch:
`du` as the layer-1 kernels stored it.  Everything goes to OUT.pt; this file asserts nothing about values itself beyond the guard
bands."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import sfa_bwd_fold_worker as F  # noqa: E402
import sfa_bwd_pair_worker as P  # noqa: E402

THREE_SAMPLES = (128, 300, 4, 8)    # 300 one-step samples over 128 pair-workers: most workers own steps of two or three samples
SHAPES = P.SHAPES + (THREE_SAMPLES,)
PAIR_WORKERS = P.PAIR_WORKERS


def worker_samples(b, h, w, workers=PAIR_WORKERS):
    """[(worker, [samples of its steps])] with the kernels' partition (csrc/sfa_stage.hip: wg_first_step)."""
    sps = (h * w + 31) // 32
    n = b * sps
    return [(k, sorted({s // sps for s in range(n * k // workers, n * (k + 1) // workers)})) for k in range(workers)]


def main(out_path):
    import ctypes as C
    import guarded_alloc as G
    from dhd_amd import _lib, mix
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    results = {'fold': os.environ.get('DHD_SFA_BWD_FOLD', '')}
    for c, b, h, w in SHAPES:
        hw = h * w
        st, x, g = F.inputs(c, b, h, w)
        assert mix.fused_stage_supported(st.to(dev), x.to(dev))
        st = st.cpu()
        first, out = F.step(st, x, g, dev)
        torch.cuda.synchronize()
        r = st.fc[0].weight.shape[0]
        off = F.scratch_offsets(b, c, hw, r)
        nsaved, nscratch = C.c_size_t(), C.c_size_t()
        _lib.check(lib.dhd_sfa_stage_workspace_bytes(b, c, hw, r, 0, C.byref(nsaved), C.byref(nscratch)), 'dhd_sfa_stage_workspace_bytes')
        assert off['total'] == nscratch.value, (off['total'], nscratch.value)   # scratch_layout keeps its byte sizes
        saved = out.grad_fn.saved_tensors[1]
        assert saved.dtype == torch.uint8 and saved.numel() == nsaved.value
        scratch = mix._stage_scratch(dev, nscratch.value).view(torch.uint8)
        pa = (b * c * hw * 4 + 255) & ~255

        def f32(buf, at, n):
            return buf[at:at + 4 * n].clone().view(torch.float32)
        pieces = {'y1': f32(saved, nsaved.value - 2 * pa, b * c * hw).view(b, c, hw),
                  'g1': f32(scratch, off['g1'], b * c * hw).view(b, c, hw), 'du': f32(scratch, off['du'], b * c * hw).view(b, c, hw),
                  'tab_g1': f32(scratch, off['tab_g1'], b * 3 * c).view(b, 3, c)}
        del out, saved
        second, _ = F.step(st, x, g, dev)
        same = all(torch.equal(first[k].view(torch.uint8), second[k].view(torch.uint8)) for k in first)
        mp = pytest.MonkeyPatch()
        try:
            with G.guarded(mp, fill=0xFF) as ledger:
                third, _ = F.step(st, x, g, dev)
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
