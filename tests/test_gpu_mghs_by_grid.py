"""MGHS pooling by grid (csrc/mghs_pool.hip, DHD_MGHS_BY_GRID): the point work of one grid shares a launch with the streaming
of another.  Forward, with grid 0's sums by the sorted gather: band sums, then {band writer || grid-0 sums}, then the grid-0
writer.  The backward by grid and the forward with grid 0's sums by pixel column were measured slower than the plain flow
and are not in the library: bit 2 of the switch changes nothing, 32-row maps keep the plain flow under every value; the
cases for them below hold whatever the library does with the switch.

The switch is read once per process, so switches 0 and 3 each run in ONE fresh process (tests/mghs_by_grid_worker.py, every
case); this module compares what they saved:
  * deterministic grouping (16 x 12 maps, grid 0 by the sorted gather): all pooled tensors and both gradients are the same bytes
    under either switch -- every voxel and every pixel is summed by the same code in the same order;
  * default grouping: the backward is the same bytes (it has no atomics and does not depend on the entries' order); the
    forward of either switch stays within atol = rtol = 1e-5 of the float64 pooling of the same points, the bound of the
    small-shape oracle tests (test_gpu_parity.test_view_transform_*), and has the same non-zero pattern.  That covers the 32 x 12
    maps, whose grid-0 sums are made by pixel column with atomics in arrival order;
  * deterministic mode: two calls give the same bytes;
  * edges -- every pixel in one band (two band grids receive nothing), no point in grid 0, a two-grid descriptor, float16 /
    bfloat16 tensor views: as above, and a third call with every output pre-filled with NaN between guard bands gives the same
    bytes again and leaves the guards alone (nothing outside is written, every element is written);
  * dhd_mghs_forward / dhd_mghs_backward on plain pointers equal the view entry points, and the phase entry points
    (dhd_mghs_forward_gather + dhd_mghs_forward_stream), which keep the two-launch flow, return the bytes of switch 0."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mghs_by_grid_worker as W  # noqa: E402

pytestmark = pytest.mark.gpu
OUTS = ('out0', 'out1', 'out2', 'out3')
GRADS = ('depth_grad', 'feat_grad')
DET = [n for n, c in W.CASES.items() if c[2]]
DEFAULT_ORDER = [n for n, c in W.CASES.items() if not c[2]]


@pytest.fixture(scope='module')
def runs(gpu, tmp_path_factory):
    """{switch: what the worker process saved} for switches 0 and 3."""
    d = tmp_path_factory.mktemp('mghs_by_grid')
    out = {}
    for switch in ('0', '3'):
        path = str(d / ('switch%s.pt' % switch))
        env = dict(os.environ, DHD_MGHS_BY_GRID=switch)
        env.pop('DHD_MGHS_DETERMINISTIC', None)
        p = subprocess.run([sys.executable, os.path.join(HERE, 'mghs_by_grid_worker.py'), path], env=env, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, (switch, p.stdout[-2000:], p.stderr[-4000:])
        out[switch] = torch.load(path, weights_only=False)
        assert out[switch]['switch'] == switch
    return out


def bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def keys_of(res):
    return [k for k in OUTS if k in res]


def test_the_cases_reach_what_they_are_meant_to(runs):
    """Kept points per grid as the library counts them: every band of the plain cases receives points, and the edge cases are
    the edges they claim to be."""
    k = {n: runs['0'][n]['kept'] for n in W.CASES}
    for n in ('sorted_b1', 'sorted_b3', 'columns_b1', 'columns_b3', 'half_f16'):
        assert len(k[n]) == 4 and min(k[n]) > 0, (n, k[n])
    assert k['one_band_only'][1] == 0 and k['one_band_only'][3] == 0 and k['one_band_only'][2] > 0
    assert k['one_band_only_columns'][1] == 0 and k['one_band_only_columns'][3] == 0 and k['one_band_only_columns'][2] > 0
    assert k['no_point_in_grid0'][0] == 0 and min(k['no_point_in_grid0'][1:]) > 0
    assert len(k['two_grids']) == 2 and min(k['two_grids']) > 0
    for n in W.CASES:
        assert runs['3'][n]['kept'] == k[n], n


@pytest.mark.parametrize('name', DET)
def test_deterministic_grouping_same_bytes_under_either_switch(runs, name):
    a, b = runs['0'][name], runs['3'][name]
    for k in keys_of(a['res']) + list(GRADS):
        assert bytes_equal(a['res'][k], b['res'][k]), (name, k)
        assert not torch.isnan(b['res'][k].float()).any(), (name, k)
    assert a['res']['depth_grad'].abs().sum() > 0 and a['res']['feat_grad'].abs().sum() > 0
    for sw in ('0', '3'):
        assert runs[sw][name]['same'], (sw, name, 'two calls differ')


@pytest.mark.parametrize('name', list(W.CASES))
def test_forward_against_the_float64_pooling_and_backward_bytes(runs, name):
    """Either switch, either grouping: the float32 sums within 1e-5 + 1e-5 |v| of the float64 sums of the same points (half
    outputs: of their rounding to the output type, plus half an ulp), zero exactly where no point lands; the backward of switch 3
    is the backward of switch 0 bit for bit."""
    odt = W.CASES[name][5]
    eps = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[odt]
    for sw in ('0', '3'):
        r = runs[sw][name]
        for k, want in zip(keys_of(r['res']), r['ref']):
            got = r['res'][k].double()
            err = (got - want).abs()
            bound = 1e-5 + (1e-5 + 1.01 * eps) * want.abs()
            print(name, 'switch', sw, k, 'max error %.3e, max of error / bound %.3f, non-zero %d' % (err.max().item(), (err / bound).max().item(),
                                                                                         int((want != 0).sum())))
            assert bool((err <= bound).all()), (name, sw, k, err.max().item())
            assert torch.equal(got != 0, want != 0) or odt != torch.float32, (name, sw, k)
    for k in GRADS:
        assert bytes_equal(runs['0'][name]['res'][k], runs['3'][name]['res'][k]), (name, k)


@pytest.mark.parametrize('name', list(W.CASES))
def test_nan_prefilled_outputs_between_guard_bands(runs, name):
    """The worker's third call ran with every buffer the wrappers allocate filled with 0xFF bytes (NaN in all three types)
    between guard bands, and checked the guards.  Every element was written: no NaN is left; and the gradients -- with
    deterministic grouping the pooled tensors too -- are the bytes of the plain call."""
    for sw in ('0', '3'):
        r = runs[sw][name]
        assert r['n_guarded'] >= 6, (sw, name, r['n_guarded'])        # four (or two) pooled tensors, two gradients, the workspaces
        for k, v in r['guarded'].items():
            assert not torch.isnan(v.float()).any(), (sw, name, k)
        for k in list(GRADS) + (keys_of(r['res']) if W.CASES[name][2] else []):
            assert bytes_equal(r['guarded'][k], runs['0'][name]['res'][k]), (sw, name, k)


@pytest.mark.parametrize('name', [n for n in DET if W.CASES[n][5] == torch.float32])
def test_plain_pointer_and_phase_entry_points(runs, name):
    """dhd_mghs_forward / dhd_mghs_backward follow the switch like the view entry points and give their bytes; the phase entry
    points keep today's flow under switch 3 and give the bytes of switch 0."""
    base = runs['0'][name]['res']
    for sw in ('0', '3'):
        raw = runs[sw][name]['raw']
        for i, k in enumerate(keys_of(base)):
            assert bytes_equal(raw['whole_out%d' % i], base[k]), (sw, name, k)
            assert bytes_equal(raw['phases_out%d' % i], base[k]), (sw, name, k)
        assert bytes_equal(raw['raw_depth_grad'], base['depth_grad']), (sw, name)
        # the node returns the context gradient as (B N, C, fH, fW), the raw entry point as (B N, fH, fW, C)
        assert bytes_equal(raw['raw_feat_grad'].permute(0, 3, 1, 2).contiguous(), base['feat_grad']), (sw, name)


@pytest.mark.parametrize('name', [n for n in DEFAULT_ORDER if W.CASES[n][5] == torch.float32])
def test_plain_pointer_backward_with_default_grouping(runs, name):
    base = runs['0'][name]['res']
    raw = runs['3'][name]['raw']
    assert bytes_equal(raw['raw_depth_grad'], base['depth_grad']), name
    assert bytes_equal(raw['raw_feat_grad'].permute(0, 3, 1, 2).contiguous(), base['feat_grad']), name
