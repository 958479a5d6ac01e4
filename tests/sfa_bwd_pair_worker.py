"""One process of tests/test_gpu_sfa_bwd_pair.py: the SFA stage's training step at the module's shapes under the DHD_SFA_BWD_FOLD
value this process was started with (the library reads the switch once per process).

    python tests/sfa_bwd_pair_worker.py OUT.pt

Per shape: forward + backward twice (same bytes?), once more inside guard bands (tests/guarded_alloc.py), and the pieces of
`saved` / `scratch` the g-buffer checks need.  Inputs, the step and the scratch layout are tests/sfa_bwd_fold_worker.py's.
Everything goes to OUT.pt; this file asserts nothing about values itself beyond the guard bands."""
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

SHAPES = ((128, 3, 36, 40),     # 135 steps of whole tiles
          (256, 2, 52, 60),     # 196 steps, a partial last tile per sample
          (128, 2, 20, 28),     # 36 steps: most pair-workers have none
          (256, 6, 12, 20),     # 48 steps
          (128, 3, 64, 64),     # 384 steps: pair-workers 42 and 85 straddle a sample boundary
          (128, 3, 100, 100),   # 939 steps: the same behind a partial step
          (256, 3, 60, 60))     # 339 steps: pair-worker 85 owns steps 225-226 across the boundary at 226, partial last step, C = 256
PAIR_WORKERS = 128              # csrc/sfa_gemm_pair.h: kPairWorkers


def straddling_workers(b, h, w):
    return F.straddling_workers(b, h, w, PAIR_WORKERS)


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
        # saved_layout (csrc/sfa_stage.hip): s | h | a1 | tab_a | mean1 | rstd1 | scsh1 ..., every section 256-byte aligned
        at_scsh1 = sum((4 * n + 255) & ~255 for n in (b * 2 * c, b * r, b * c, b * 3 * c, c, c))
        pieces = {'y1': f32(saved, nsaved.value - 2 * pa, b * c * hw).view(b, c, hw), 'y2': f32(saved, nsaved.value - pa, b * c * hw).view(b, c, hw),
                  'g2': f32(scratch, off['g2'], b * c * hw).view(b, c, hw), 'g1': f32(scratch, off['g1'], b * c * hw).view(b, c, hw),
                  'tab_g2': f32(scratch, off['tab_g2'], b * 3 * c).view(b, 3, c), 'tab_g1': f32(scratch, off['tab_g1'], b * 3 * c).view(b, 3, c),
                  'scsh1': f32(saved, at_scsh1, 2 * c).view(2, c)}
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
