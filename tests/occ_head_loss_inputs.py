"""The shared input definition of the occupancy head + losses tests (test_gpu_occ_head_loss.py, test_occ_head_loss_capi.py): the
head, the x and the shapes of occ_head_train_inputs.py, labels and a camera mask for them, and the float64 twin of
head -> three losses -> weighted sum -> backward.  Everything here is computed once per (shape, precision) and never modified."""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_head_train_inputs as OT  # noqa: E402
import value_edge_inputs as VE  # noqa: E402

ABSENT = 7                          # the class nobody is labelled with
IGNORE = 255
WEIGHTS = VE.LOSS_WEIGHTS           # (0.7, 1.3, 2.0): dL/dloss of (cross entropy, sem scal, geo scal)
EMPTY_SAMPLE = 1                    # in the shapes with more than one sample: the sample without a valid voxel
LOSSES = ('ce', 'sem', 'geo')


@functools.lru_cache(maxsize=None)
def labels(case, seed=23):
    """(sem uint8 (B, Dx, Dy, DZ), cam bool of the same shape): the 18 classes but ABSENT, about 3 % ignored, 70 % camera-visible;
    in a shape with several samples, sample EMPTY_SAMPLE has no valid voxel (its first half masked out, its second half ignored)."""
    b, dy, dx = OT.SHAPES[case]
    gen = torch.Generator().manual_seed(seed + 1000 * b + 10 * dy + dx)
    sem = torch.randint(0, OT.N_CLS, (b, dx, dy, OT.DZ), generator=gen)
    sem[sem == ABSENT] = OT.N_CLS - 1
    sem[torch.rand(sem.shape, generator=gen) < 0.03] = IGNORE
    cam = torch.rand(sem.shape, generator=gen) < 0.7
    if b > 1:
        cam[EMPTY_SAMPLE, : dx // 2 + 1] = False
        sem[EMPTY_SAMPLE, dx // 2 + 1:] = IGNORE
    return sem.to(torch.uint8), cam


def class_weights():
    return VE.class_weights()


def losses_f64(logits64, case):
    """occ_losses_f64 on (cells, 18) float64 logits with the case's labels -> (ce, sem, geo), differentiable."""
    sem, cam = labels(case)
    return VE.occ_losses_f64(logits64.reshape(-1, OT.N_CLS), sem.reshape(-1).long(), cam.reshape(-1), class_weights())[0]


@functools.lru_cache(maxsize=None)
def twin(case, prec):
    """float64 autograd on the CPU of head -> losses -> sum_i WEIGHTS[i] loss_i, from x as the operator reads it and the float32
    parameters -> 'losses' (3,), 'logits', dx, dw1, db1, dw2, db2, all float64."""
    v = OT.inputs(case, prec)
    leaves = {k: v[k].double().requires_grad_() for k in ('x',) + OT.PARAMS}
    logits = OT.formulation(*(leaves[k] for k in ('x',) + OT.PARAMS))
    losses = losses_f64(logits, case)
    sum(w * l for w, l in zip(WEIGHTS, losses)).backward()
    out = OT._collect(logits, leaves)
    out['losses'] = torch.stack([l.detach() for l in losses])
    return out
