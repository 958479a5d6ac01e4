"""The replay harness of tests/swin_train_step_inputs.py on the CPU: what tests/test_gpu_swin_train_step.py takes as its float64
reference is wired to the right DropPath modules in the right order, and recording the masks of a run does not change the run."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_train_step_inputs as TS  # noqa: E402
import swin_wide_inputs as SW  # noqa: E402
from conftest import GOLDEN  # noqa: E402

TOL = 1e-9


def test_rates_and_order_of_the_draws():
    net = TS.net()
    found = TS.drop_paths(net)
    assert len(found) == TS.DRAWS
    rates = [dp.drop_prob for _, dp in found]
    assert np.allclose(rates, [k / 14 for k in range(1, 8) for _ in (0, 1)], atol=1e-7) and rates[-1] == 0.5
    assert [n.rsplit('.', 2)[-2] for n, _ in found] == ['attn', 'ffn'] * 7
    b0 = net.stages[0].blocks[0]
    assert b0.attn.drop.drop_prob == 0. and b0.ffn.dropout_layer.drop_prob == 0.          # block 0 draws nothing
    assert TS.net(with_cp=True).stages[2].with_cp and not net.stages[2].with_cp


def test_replay_of_keep_reproduces_the_eval_mode_fixture():
    """Every replayed mask equal to its module's keep: x.div(keep) * keep is x to an ulp, so the train-mode float64 run must give
    G20's eval-mode run -- outputs, input gradient and every recorded gradient, norm and projection -- to 1e-9 |ref|max.  A mask
    handed to the wrong module (another keep) or a module left drawing would be off in the first digit."""
    g = SW.load(GOLDEN)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(threads, 8))
    try:
        net = TS.net().double()
        assert SW.set_state(net) == str(g['state_sha']) and net.training
        keeps = [torch.full((2, 1, 1), 1 - dp.drop_prob, dtype=torch.float64) for _, dp in TS.drop_paths(net)]
        gen = torch.get_rng_state()
        with TS.replay(net, keeps) as taken:
            outs, xg, _ = TS.step(net, torch.from_numpy(SW.x_input()))
        assert taken[0] == TS.DRAWS == len(keeps)
        assert torch.equal(torch.get_rng_state(), gen)                                      # the replay draws nothing
    finally:
        torch.set_num_threads(threads)
    got = {f'out{i}': o.numpy() for i, o in enumerate(outs)}
    got['x_grad'] = xg.numpy()
    got.update(SW.grad_summaries(net))
    worst, n = 0.0, 0
    for k, r in g.items():
        if not k.startswith(('out', 'x_grad', 'grad.', 'gnorm.', 'gproj.')):
            continue
        a = np.asarray(got[k])
        assert a.shape == r.shape and a.dtype == np.float64, k
        err, size = float(np.abs(a - r).max()), float(np.abs(r).max())
        worst, n = max(worst, err / size), n + 1
        assert err <= TOL * size, f'{k}: {err:.3e} of {size:.3e}'
    print(f'train mode with keep replayed against G20: worst relative error {worst:.3e} over {n} entries')
    assert n == 4 + 2 * len(list(net.named_parameters())) + sum(SW.full_grad(k, p) for k, p in net.named_parameters())


def test_recording_is_transparent():
    """One float32 train step on the CPU from one seed, with and without record_masks: the same bits and the same generator state
    afterwards; 14 masks of zeros and ones, and (2, 1, 1) each.  torch's deterministic algorithms are asked for: the bias tables'
    gradient (an index_put that accumulates) otherwise differs in the last place between any two runs on several threads."""
    net = TS.net()                                                                         # torch's initial weights: the two runs share them
    x = torch.from_numpy(SW.x_input()).float()
    runs, was = [], torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        for record in (False, True):
            torch.manual_seed(77)
            if record:
                with TS.record_masks(net) as masks:
                    res = TS.step(net, x)
            else:
                res = TS.step(net, x)
            runs.append((res, torch.get_rng_state()))
    finally:
        torch.use_deterministic_algorithms(was)
    (a, sa), (b, sb) = runs
    assert all(torch.equal(p, q) for p, q in zip(a[0], b[0])) and torch.equal(a[1], b[1])
    assert a[2].keys() == b[2].keys() and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    assert torch.equal(sa, sb)
    torch.manual_seed(77)
    assert not torch.equal(torch.get_rng_state(), sa)                                      # and draws there were
    assert len(masks) == TS.DRAWS and all(tuple(m.shape) == (2, 1, 1) and m.dtype == torch.float32 for m in masks)
    assert all(bool(((m == 0) | (m == 1)).all()) for m in masks) and any(bool((m == 0).any()) for m in masks)
    from dhd_amd.swin import DropPath
    assert DropPath.forward.__qualname__ == 'DropPath.forward'                             # the patch is gone
