"""The pair kernel of the SFA backward's layer 1 (csrc/sfa_gemm_pair1.h, DHD_SFA_BWD_FOLD bit 8): conv1's data gradient du, its
weight gradient and the du-part of dL/da per (pair-worker, sample) in one launch on pairs of compute units; g1 is not written.

The switch is read once per process, so each value runs in ONE fresh process (tests/sfa_bwd_pair1_worker.py, all shapes, bf16x3,
train mode): 7 (pair layer 2 + folded layer 1, the yardstick), 15 (both layers as pair kernels), 13 (the same without the fold
bit: bit 8 decides whatever bit 2 says) and 5 (pair layer 2 + unfolded layer 1, which leaves g1 as layer 2 made it).  The shapes
are sfa_bwd_pair_worker's plus (128, 300, 4, 8), where workers own steps of THREE samples: the per-sample blend coefficients are
reloaded and a dL/da row is flushed twice inside such a worker.  This module compares what the processes saved:
  1. gx and the 12 parameter gradients against the float64 oracle, with test_gpu_sfa_bwd_fold's bounds and tie allowance;
  2. each tensor's error <= 1.5 x switch 7's error + 1e-6 scale (same mathematics, another summation order);
  3. two calls, and a call inside NaN-filled guard bands, give the same bytes;
  4. du as stored, against a float64 evaluation of the product the bf16x3 mode defines, sum_co (Wh gh + Wh gm + Wm gh) with
     h = bf16(v), m = bf16(v - h) (csrc/sfa_mfma.h: split2_hm), on gy1 = fma(c1, y1, fma(c0, g1, c2)) from the run's own g1, y1
     and tab_g1: within 1e-6 scale, the bound layer 2's g1 is held to.  The distance to the plain float64 product is printed and
     bounded by the format's own worst case, 3 x 2^-18 sum_co |W| |gy|, element by element;
  5. g1 after a value-15 (13) call is, byte for byte, g1 after a value-5 call;
  6. the forward's `out` does not depend on the switch."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sfa_bwd_pair1_worker as W  # noqa: E402
from test_gpu_parity import GEMM_MODES  # noqa: E402
import test_gpu_sfa_bwd_fold as FOLD  # noqa: E402

pytestmark = pytest.mark.gpu
F = GEMM_MODES['bf16x3']
FOLDS = ('7', '15', '13', '5')
PAIR1 = ('15', '13')


def test_a_worker_of_the_extra_shape_owns_steps_of_three_samples():
    c, b, h, w = W.THREE_SAMPLES
    assert (h * w + 31) // 32 == 1
    per_worker = dict(W.worker_samples(b, h, w))
    assert per_worker[2] == [4, 5, 6]
    assert max(len(v) for v in per_worker.values()) == 3 and min(len(v) for v in per_worker.values()) == 2


@pytest.fixture(scope='module')
def runs(gpu, tmp_path_factory):
    """{switch value: what the worker process saved}"""
    d = tmp_path_factory.mktemp('sfa_bwd_pair1')
    out = {}
    for fold in FOLDS:
        path = str(d / ('fold%s.pt' % fold))
        env = dict(os.environ, DHD_SFA_BWD_FOLD=fold)
        p = subprocess.run([sys.executable, os.path.join(HERE, 'sfa_bwd_pair1_worker.py'), path], env=env, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, (fold, p.stdout[-2000:], p.stderr[-4000:])
        out[fold] = torch.load(path, weights_only=False)
        assert out[fold]['fold'] == fold
    return out


_refs = {}


def reference(shape, gpu):
    """test_gpu_sfa_bwd_fold.reference at this module's shapes (its worker's inputs are this worker's), once per shape"""
    if shape not in _refs:
        _refs[shape] = FOLD.reference(shape, gpu)
    return _refs[shape]


@pytest.mark.parametrize('shape', W.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_pair1_backward_vs_float64_oracle(gpu, runs, shape):
    ref, tie = reference(shape, gpu)
    errs = {}
    for fold in ('7',) + PAIR1:
        res = runs[fold][shape]['res']
        for k, want in ref.items():
            got = res[k].double().reshape(want.shape)
            scale = max(1.0, want.abs().max().item())
            tol = (1e-4 if k == 'gx' else 5e-4) * F
            excess = ((got - want).abs() - 1.01 * tie[k].reshape(want.shape)).max().item()
            errs[fold, k] = (got - want).abs().max().item(), scale
            print('fold', fold, shape, k, 'max error %.3e excess %.3e bound %.3e' % (errs[fold, k][0], excess, tol * scale))
            assert excess <= tol * scale, (fold, k, excess, tol * scale)
    for fold in PAIR1:
        for k in ref:
            (e, scale), (e7, _) = errs[fold, k], errs['7', k]
            assert e <= 1.5 * e7 + 1e-6 * scale, (fold, k, e, e7, scale)


@pytest.mark.parametrize('shape', W.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_pair1_backward_is_reproducible_and_stays_inside_its_buffers(runs, shape):
    for fold in FOLDS:
        r = runs[fold][shape]
        assert r['same'], (fold, 'two calls differ')
        assert r['n_guarded'] > 0 and r['same_guarded'], (fold, 'the guarded, NaN-filled call differs')
    for fold in FOLDS[1:]:   # the forward does not depend on the switch
        assert torch.equal(runs['7'][shape]['res']['out'], runs[fold][shape]['res']['out'])
    # bit 8 decides, whatever bit 2 says: the same launches, the same bytes
    for k, v in runs['15'][shape]['res'].items():
        assert torch.equal(v.view(torch.uint8), runs['13'][shape]['res'][k].view(torch.uint8)), k


@pytest.mark.parametrize('shape', W.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_du_is_the_data_gradient_of_gy1_and_g1_is_left_alone(runs, shape):
    c, b, h, w = shape
    p5 = runs['5'][shape]['pieces']
    st, _, _ = W.F.inputs(c, b, h, w)
    w1 = st.spacial_leanring[0].weight.detach().double().reshape(c, c)      # [co][ci]

    def split(v):                                           # split2_hm: two round-to-nearest-even cuts, the residual exact in float32
        hi = v.float().bfloat16().float()
        return hi.double(), (v.float() - hi).bfloat16().double()
    wh, wm = split(w1)
    for fold in PAIR1:
        p = runs[fold][shape]['pieces']
        for k in ('y1', 'tab_g1', 'g1'):                    # 5.: g1 is the gradient layer 2 made (and so are the sums taken from it)
            assert torch.equal(p[k].view(torch.uint8), p5[k].view(torch.uint8)), (fold, k)
        t = p['tab_g1'].double()
        # the staging's two fused multiply-adds: each exact in float64 up to its one rounding, then cut to float32
        gy = (t[:, 1, :, None] * p['y1'].double() + (t[:, 0, :, None] * p['g1'].double() + t[:, 2, :, None]).float().double()).float()
        gh, gm = split(gy)
        gy = gy.double()
        want = torch.einsum('oi,bop->bip', wh, gh) + torch.einsum('oi,bop->bip', wh, gm) + torch.einsum('oi,bop->bip', wm, gh)
        plain = torch.einsum('oi,bop->bip', w1, gy)
        got = p['du'].double()
        scale = plain.abs().max().item()
        d, d_plain = (got - want).abs().max().item(), (got - plain).abs().max().item()
        print('du fold', fold, shape, 'vs the three-product formula %.3e, vs the plain product %.3e, scale %.3e: ratios %.3e %.3e' %
              (d, d_plain, scale, d / scale, d_plain / scale))
        assert d <= 1e-6 * scale, (fold, d, scale)
        worst = 3 * 2.0 ** -18 * torch.einsum('oi,bop->bip', w1.abs(), gy.abs()) + 1e-6 * scale
        assert ((got - plain).abs() <= worst).all(), fold
    # the folded layer 1 is what the check can tell apart: it leaves gy1, not g1, behind
    p7 = runs['7'][shape]['pieces']
    assert (p7['g1'].double() - p5['g1'].double()).abs().max().item() > 1e-3 * p5['g1'].abs().max().item()
