"""The folded SFA backward (csrc/sfa_stage.hip, DHD_SFA_BWD_FOLD): per layer the data gradient runs first and leaves its
BatchNorm-backward prologue's result over g, the weight gradient reads that one tensor and also makes the sums that pair_sums /
blend1_da made in passes of their own.

The switch is read once per process, so folds 0 and 3 each run in ONE fresh process (tests/sfa_bwd_fold_worker.py, all shapes,
bf16x3, train mode); this module compares what they saved:
  * gx and the 12 parameter gradients against the float64 oracle (oracle/mghs_oracle.sfa_stage), within test_sfa_stage_vs_torch's
    tolerances (tol_x = 1e-4 f, tol_p = 5e-4 f, f = 20) and with its tie handling: the element-wise difference between two
    float64 evaluations of the same formula (test_gpu_parity._plain_stage) whose ReLU gradient is cut at +tie and -tie is granted
    on top -- zero unless a pre-ReLU activation within the GEMM's rounding of zero touches the element;
  * fold-on error <= 1.5 x fold-off error + 1e-6 scale per tensor (same mathematics, another summation order);
  * two calls give the same bytes, and so does a call inside guard bands with NaN-filled workspaces (nothing outside
    saved / scratch / outputs is written, nothing unwritten is read);
  * after the data gradients the g buffers hold c0 g + c1 y + c2 applied exactly ONCE (a repeated last tile or an idle
    workgroup that stored would apply it to its own output): g and the tables from the processes' scratch, the expression in
    torch float64.  With fold 3 the head of g2's region holds the per-(worker, sample) dL/da rows by then and is left out."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sfa_bwd_fold_worker as W  # noqa: E402
from test_gpu_parity import GEMM_MODES, _TIE, _plain_stage  # noqa: E402

pytestmark = pytest.mark.gpu
F = GEMM_MODES['bf16x3']
PARAMS = ('fc.0.weight', 'fc.0.bias', 'fc.2.weight', 'fc.2.bias', 'spacial_leanring.0.weight', 'spacial_leanring.0.bias',
          'spacial_leanring.1.weight', 'spacial_leanring.1.bias', 'spacial_leanring.3.weight', 'spacial_leanring.3.bias',
          'spacial_leanring.4.weight', 'spacial_leanring.4.bias')
ORACLE_KEYS = ('fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'conv1_w', 'conv1_b', 'bn1_w', 'bn1_b', 'conv2_w', 'conv2_b', 'bn2_w', 'bn2_b')


def test_some_shapes_have_workers_that_straddle_samples():
    """The per-(worker, sample) dL/da rows are only exercised where a weight-gradient worker's steps belong to two samples (a flush
    inside the worker, two rows from it, a worker shared by two samples in the summing kernel).  Computed with the kernels' own
    partition, so the claim cannot go stale: two of the shapes have such workers, one of them behind a partial last step, and
    one shape has fewer steps than workers (workers without steps)."""
    have = {s: W.straddling_workers(*s[1:]) for s in W.SHAPES}
    assert sum(1 for v in have.values() if v) >= 2, have
    assert any(v and (s[2] * s[3]) % 32 != 0 for s, v in have.items()), have
    assert any(s[1] * ((s[2] * s[3] + 31) // 32) < W.K_WORKERS for s in W.SHAPES)


@pytest.fixture(scope='module')
def runs(gpu, tmp_path_factory):
    """{fold: what the worker process saved} for folds 0 and 3."""
    d = tmp_path_factory.mktemp('sfa_bwd_fold')
    out = {}
    for fold in ('0', '3'):
        path = str(d / ('fold%s.pt' % fold))
        env = dict(os.environ, DHD_SFA_BWD_FOLD=fold)
        p = subprocess.run([sys.executable, os.path.join(HERE, 'sfa_bwd_fold_worker.py'), path], env=env, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, (fold, p.stdout[-2000:], p.stderr[-4000:])
        out[fold] = torch.load(path, weights_only=False)
        assert out[fold]['fold'] == fold
    return out


_refs = {}


def reference(shape, gpu):
    """(oracle gx, oracle parameter gradients by module name, tie allowance per tensor) -- computed once per shape."""
    if shape not in _refs:
        from oracle import mghs_oracle as O
        c, b, h, w = shape
        st, x, g = W.inputs(c, b, h, w)
        n = lambda t: t.detach().cpu().numpy()
        sp = st.spacial_leanring
        bnp = lambda m: (n(m.weight), n(m.bias), n(m.running_mean), n(m.running_var))
        _, dx, grads = O.sfa_stage(n(x), n(st.fc[0].weight), n(st.fc[0].bias), n(st.fc[2].weight), n(st.fc[2].bias), n(sp[0].weight),
                                   n(sp[0].bias), bnp(sp[1]), n(sp[3].weight), n(sp[3].bias), bnp(sp[4]), eps=sp[1].eps, training=True,
                                   out_grad=n(g))
        ref = {'gx': torch.from_numpy(np.asarray(dx, np.float64))}
        for name, key in zip(PARAMS, ORACLE_KEYS):
            ref['d_' + name] = torch.from_numpy(np.asarray(grads[key], np.float64))
        # the tie allowance: the same formula in float64 with the ReLU gradient cut at +tie and at -tie
        import copy
        cut = []
        for margin in (_TIE * F, -_TIE * F):
            m = copy.deepcopy(st).double().to(gpu).train()
            xd = x.double().to(gpu).requires_grad_()
            _plain_stage(m, xd, margin).backward(g.double().to(gpu))
            cut.append(dict([('gx', xd.grad.cpu())] + [('d_' + k, p.grad.cpu()) for k, p in m.named_parameters()]))
        tie = {k: (cut[0][k] - cut[1][k]).abs() for k in cut[0]}
        _refs[shape] = ref, tie
    return _refs[shape]


@pytest.mark.parametrize('shape', W.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_folded_backward_vs_float64_oracle(gpu, runs, shape):
    ref, tie = reference(shape, gpu)
    errs = {}
    for fold in ('0', '3'):
        res = runs[fold][shape]['res']
        for k, want in ref.items():
            got = res[k].double().reshape(want.shape)
            scale = max(1.0, want.abs().max().item())
            tol = (1e-4 if k == 'gx' else 5e-4) * F
            excess = ((got - want).abs() - 1.01 * tie[k].reshape(want.shape)).max().item()
            errs[fold, k] = (got - want).abs().max().item(), scale
            print('fold', fold, shape, k, 'max error %.3e excess %.3e bound %.3e' % (errs[fold, k][0], excess, tol * scale))
            assert excess <= tol * scale, (fold, k, excess, tol * scale)
    for k in ref:
        (e3, scale), (e0, _) = errs['3', k], errs['0', k]
        assert e3 <= 1.5 * e0 + 1e-6 * scale, (k, e3, e0, scale)


@pytest.mark.parametrize('shape', W.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_folded_backward_is_reproducible_and_stays_inside_its_buffers(runs, shape):
    for fold in ('0', '3'):
        r = runs[fold][shape]
        assert r['same'], (fold, 'two calls differ')
        assert r['n_guarded'] > 0 and r['same_guarded'], (fold, 'the guarded, NaN-filled call differs')
    # the forward does not depend on the switch
    assert torch.equal(runs['0'][shape]['res']['out'], runs['3'][shape]['res']['out'])


@pytest.mark.parametrize('shape', W.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_g_buffers_hold_the_prologue_result_exactly_once(runs, shape):
    c, b, h, w = shape
    p0, p3 = runs['0'][shape]['pieces'], runs['3'][shape]['pieces']
    # without the fold the g buffers are what the passes before the GEMMs wrote; the forward's y and the BatchNorm-2 table (made
    # by blend2_bn_bwd in either flow) are the same bytes in both processes
    for k in ('y1', 'y2', 'tab_g2'):
        assert torch.equal(p0[k], p3[k]), k
    skip = (W.K_WORKERS + b) * c        # floats of g2's region that hold the dL/da rows after the fold-3 call
    for g, y, tab in (('g2', 'y2', 'tab_g2'), ('g1', 'y1', 'tab_g1')):
        t = p3[tab].double()            # the folded call's own table (its BatchNorm-1 sums come in another order)
        want = t[:, 0, :, None] * p0[g].double() + t[:, 1, :, None] * p3[y].double() + t[:, 2, :, None]
        got = p3[g].double()
        lo = skip if g == 'g2' else 0
        assert lo < got.numel() // 2
        d = (got - want).flatten()[lo:].abs().max().item()
        scale = want.abs().max().item()
        # once: float32 rounding of two fused multiply-adds; twice would be off by the size of the values themselves
        assert d <= 1e-6 * max(scale, 1e-30), (g, d, scale)
        assert (p0[g].double() - want).flatten()[lo:].abs().max().item() > 1e-3 * scale, (g, 'the check cannot tell g from its prologue result')
