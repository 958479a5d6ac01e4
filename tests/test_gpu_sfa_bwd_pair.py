"""The pair kernel of the SFA backward (csrc/sfa_gemm_pair.h, DHD_SFA_BWD_FOLD bit 4): layer 2's data gradient, weight gradient
and BatchNorm-1 sums in one launch on pairs of compute units, 128 pair-workers over the 32-pixel steps.

The switch is read once per process, so each value runs in ONE fresh process (tests/sfa_bwd_pair_worker.py, all shapes, bf16x3,
train mode): 3 (the folded flow, the yardstick), 7 (pair kernel for layer 2, folded layer 1) and 5 (pair kernel for layer 2,
unfolded layer 1, which leaves g1 and g2 as the pair kernel met and made them).  A pair form of layer 1 (bit 8) does not exist,
so 11 and 15 are not run.  This module compares what the processes saved:
  1. gx and the 12 parameter gradients against the float64 oracle, with test_gpu_sfa_bwd_fold's bounds and tie allowance;
  2. each tensor's error <= 1.5 x the fold-3 error + 1e-6 scale (same mathematics, another summation order);
  3. two calls, and a call inside NaN-filled guard bands, give the same bytes;
  4. g1 as the pair kernel stored it.  NOT byte-equal to the folded flow's: the pair kernel's data gradient runs on
     v_mfma_f32_16x16x32_bf16 (k-steps of 32 channels, 16 output rows per wave) where pw_gemm_cu_kernel runs 32x32x16, another
     order of the float32 additions.  So: against a float64 evaluation from fold 3's stored gy2 (the samples of g2 behind its
     dL/da rows), the conv2 weight and y1, within 1e-6 scale.  The evaluation is of the product the bf16x3 mode defines,
     sum_co (Wh gh + Wh gm + Wm gh) [z1 > 0] with h = bf16(v), m = bf16(v - h) (csrc/sfa_mfma.h: split2_hm), so that what is left
     is the float32 accumulation alone (measured: 2.4e-7 .. 4.2e-7 scale).  Against the PLAIN float64 product sum_co W gy no bf16x3 data
     gradient can stay within 1e-6 scale: the mode drops Wm gm and the third parts, up to 3 x 2^-18 per product; measured for
     this kernel 4.8e-6 .. 7.0e-6 scale over the seven shapes.  That figure is printed, and bounded by the format's own worst
     case, 3 x 2^-18 sum_co |W| |gy|, element by element;
  5. g2 is still g, not gy, after a pair-flow call: fold 3's table applied to it gives fold 3's g2, and it is far from it itself;
  6. the forward's `out` does not depend on the switch."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sfa_bwd_pair_worker as W  # noqa: E402
from test_gpu_parity import GEMM_MODES  # noqa: E402  (_TIE, _plain_stage: through test_gpu_sfa_bwd_fold.reference)
import test_gpu_sfa_bwd_fold as FOLD  # noqa: E402

pytestmark = pytest.mark.gpu
F = GEMM_MODES['bf16x3']
FOLDS = ('3', '7', '5')
PAIR = ('7', '5')
FOLD_WORKERS = 256   # workers of the folded layer 1, whose dL/da rows lie at the head of g2's region after folds 3 and 7


def test_the_partition_over_128_pair_workers_is_what_the_shapes_claim():
    have = {s: W.straddling_workers(*s[1:]) for s in W.SHAPES}
    assert [k for k, _, _ in have[(128, 3, 64, 64)]] == [42, 85]
    assert [k for k, _, _ in have[(128, 3, 100, 100)]] == [42, 85] and (100 * 100) % 32 != 0
    assert (85, 225, 227) in have[(256, 3, 60, 60)] and 3 * ((60 * 60 + 31) // 32) == 339 and (60 * 60) % 32 != 0
    assert [s[1] * ((s[2] * s[3] + 31) // 32) for s in W.SHAPES] == [135, 196, 36, 48, 384, 939, 339]
    assert sum(1 for s in W.SHAPES if s[1] * ((s[2] * s[3] + 31) // 32) < W.PAIR_WORKERS) == 2


@pytest.fixture(scope='module')
def runs(gpu, tmp_path_factory):
    """{switch value: what the worker process saved}"""
    d = tmp_path_factory.mktemp('sfa_bwd_pair')
    out = {}
    for fold in FOLDS:
        path = str(d / ('fold%s.pt' % fold))
        env = dict(os.environ, DHD_SFA_BWD_FOLD=fold)
        p = subprocess.run([sys.executable, os.path.join(HERE, 'sfa_bwd_pair_worker.py'), path], env=env, capture_output=True, text=True,
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
def test_pair_backward_vs_float64_oracle(gpu, runs, shape):
    ref, tie = reference(shape, gpu)
    errs = {}
    for fold in FOLDS:
        res = runs[fold][shape]['res']
        for k, want in ref.items():
            got = res[k].double().reshape(want.shape)
            scale = max(1.0, want.abs().max().item())
            tol = (1e-4 if k == 'gx' else 5e-4) * F
            excess = ((got - want).abs() - 1.01 * tie[k].reshape(want.shape)).max().item()
            errs[fold, k] = (got - want).abs().max().item(), scale
            print('fold', fold, shape, k, 'max error %.3e excess %.3e bound %.3e' % (errs[fold, k][0], excess, tol * scale))
            assert excess <= tol * scale, (fold, k, excess, tol * scale)
    for fold in PAIR:
        for k in ref:
            (e, scale), (e3, _) = errs[fold, k], errs['3', k]
            assert e <= 1.5 * e3 + 1e-6 * scale, (fold, k, e, e3, scale)


@pytest.mark.parametrize('shape', W.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_pair_backward_is_reproducible_and_stays_inside_its_buffers(runs, shape):
    for fold in FOLDS:
        r = runs[fold][shape]
        assert r['same'], (fold, 'two calls differ')
        assert r['n_guarded'] > 0 and r['same_guarded'], (fold, 'the guarded, NaN-filled call differs')
    for fold in PAIR:   # the forward does not depend on the switch
        assert torch.equal(runs['3'][shape]['res']['out'], runs[fold][shape]['res']['out'])


@pytest.mark.parametrize('shape', W.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_g1_is_the_masked_data_gradient_of_fold_3s_gy2(runs, shape):
    c, b, h, w = shape
    hw = h * w
    p3, p5 = runs['3'][shape]['pieces'], runs['5'][shape]['pieces']
    for k in ('y1', 'y2', 'tab_g2', 'scsh1'):
        assert torch.equal(p3[k], p5[k]), k
    first = -(-(FOLD_WORKERS + b) * c // (c * hw))        # samples of fold 3's g2 that its dL/da rows reach into
    assert first < b
    st, _, _ = W.F.inputs(c, b, h, w)
    w2 = st.spacial_leanring[3].weight.detach().double().reshape(c, c)      # [co][ci]
    gy2 = p3['g2'][first:].double()
    z1 = p3['scsh1'][0].double()[None, :, None] * p3['y1'][first:].double() + p3['scsh1'][1].double()[None, :, None]
    def split(v):                                           # split2_hm: two round-to-nearest-even cuts, the residual exact in float32
        hi = v.float().bfloat16().float()
        return hi.double(), (v.float() - hi).bfloat16().double()
    (wh, wm), (gh, gm) = split(w2), split(gy2)
    mask = z1 > 0
    want = (torch.einsum('oi,bop->bip', wh, gh) + torch.einsum('oi,bop->bip', wh, gm) + torch.einsum('oi,bop->bip', wm, gh)) * mask
    plain = torch.einsum('oi,bop->bip', w2, gy2) * mask
    got = p5['g1'][first:].double()
    scale = plain.abs().max().item()
    d, d_plain = (got - want).abs().max().item(), (got - plain).abs().max().item()
    print('g1', shape, 'vs the three-product formula %.3e, vs the plain product %.3e, scale %.3e: ratios %.3e %.3e' %
          (d, d_plain, scale, d / scale, d_plain / scale))
    assert torch.equal(got == 0, want == 0)   # the ReLU mask: float32 fmaf and this float64 expression agree in sign
    assert d <= 1e-6 * scale, (d, scale)
    worst = 3 * 2.0 ** -18 * torch.einsum('oi,bop->bip', w2.abs(), gy2.abs()) + 1e-6 * scale
    assert ((got - plain).abs() <= worst).all()


@pytest.mark.parametrize('shape', W.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_g2_is_still_g_after_a_pair_flow_call(runs, shape):
    c, b, h, w = shape
    p3 = runs['3'][shape]['pieces']
    t = p3['tab_g2'].double()
    for fold, lo in (('5', 0), ('7', (FOLD_WORKERS + b) * c)):            # fold 7: the folded layer 1 left its dL/da rows at the head
        p = runs[fold][shape]['pieces']
        assert torch.equal(p['tab_g2'], p3['tab_g2']) and torch.equal(p['y2'], p3['y2'])
        skip = max(lo, (FOLD_WORKERS + b) * c)                             # fold 3's own rows
        assert skip < p['g2'].numel() // 2
        gy = t[:, 0, :, None] * p['g2'].double() + t[:, 1, :, None] * p['y2'].double() + t[:, 2, :, None]
        scale = gy.abs().max().item()
        d = (gy - p3['g2'].double()).flatten()[skip:].abs().max().item()
        assert d <= 1e-6 * max(scale, 1e-30), (fold, d, scale)
        assert (p['g2'].double() - p3['g2'].double()).flatten()[skip:].abs().max().item() > 1e-3 * scale, (fold, 'g2 cannot be told from gy2')
    # with nothing folded behind it the pair flow leaves ALL of g2 alone: the same bytes as the head-less part of fold 7's
    lo = (FOLD_WORKERS + b) * c
    assert torch.equal(runs['5'][shape]['pieces']['g2'].flatten()[lo:], runs['7'][shape]['pieces']['g2'].flatten()[lo:])
