"""The inputs of tests/test_gpu_stereo_cv.py (tests/stereo_cv_inputs.py), checked without a GPU: the conditions under which a
pass of the GPU tests means something."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stereo_cv_inputs as inp  # noqa: E402


def test_cpu_gen_grid_on_g8_is_the_recorded_grid_bit_for_bit():
    g = inp.g8()
    m = inp.calibration('a')
    m['frustum'] = torch.from_numpy(g['frustum'])
    grid = inp.cpu_grid(m)
    assert np.array_equal(grid.reshape(g['grid'].shape).numpy(), g['grid'])
    # the template create_frustum builds for G8's depth config is G8's recorded frustum up to the last bit of its axes (numpy's
    # linspace / arange there, torch's here)
    assert torch.allclose(inp.frustum(12), m['frustum'], rtol=1e-6, atol=0)


def test_calibration_a_has_most_positions_inside_the_image():
    inside, marked, outside = inp.shares(inp.cpu_grid(inp.metas('a', 12)))
    print('a: inside %.3f marked %.3f outside %.3f' % (inside, marked, outside))
    assert inside >= 0.5


def test_calibration_b_puts_near_hypotheses_of_view_1_behind_the_camera():
    inside, marked, outside = inp.shares(inp.cpu_grid(inp.metas('b', 12))[1])
    print('b, view 1: inside %.3f marked %.3f outside %.3f' % (inside, marked, outside))
    assert inside >= 0.25 and marked >= 0.10


@pytest.mark.parametrize('kind', inp.CALIBRATIONS)
@pytest.mark.parametrize('n_depth', sorted(inp.DEPTH_CFG))
def test_every_case_samples_inside_and_outside_the_image(kind, n_depth):
    """Some position of every case has all four taps outside the map, so the flag channel samples exactly 0 there (the bias
    rule is exercised), and a fair share lies inside (the taps are exercised)."""
    inside, marked, outside = inp.shares(inp.cpu_grid(inp.metas(kind, n_depth)))
    assert outside > 0 and inside >= 0.25, (inside, marked, outside)


@pytest.mark.parametrize('kind', inp.CALIBRATIONS)
def test_the_small_map_samples_inside_and_outside_the_image(kind):
    m = inp.metas(kind, 12, input_size=inp.SMALL_INPUT_SIZE)
    assert tuple(m['frustum'].shape) == (12, 5, 7, 3)
    inside, marked, outside = inp.shares(inp.cpu_grid(m))
    assert outside > 0 and inside > 0.02, (inside, marked, outside)


def test_calibration_c_is_a_flip_and_a_rotation_that_keeps_the_image_centre():
    a, c = inp.calibration('a'), inp.calibration('c')
    centre = torch.tensor([(inp.INPUT_SIZE[1] - 1) / 2.0, (inp.INPUT_SIZE[0] - 1) / 2.0])
    for n in range(2):
        ra, rc = a['post_rots'][0, n, :2, :2].double(), c['post_rots'][0, n, :2, :2].double()
        assert torch.det(ra) * torch.det(rc) < 0                                   # the flip
        aug = rc @ torch.inverse(ra)
        assert abs(abs(float(torch.det(aug))) - 1) < 1e-5
        assert abs(float(torch.atan2(-aug[1, 0], -aug[0, 0])) - np.radians(5.0)) < 1e-5  # rot(5 deg) @ diag(-1, 1)
        # a point that G8's augmentation sends to the image centre still lands there
        p = torch.inverse(ra) @ (centre.double() - a['post_trans'][0, n, :2].double())
        assert torch.allclose(rc @ p + c['post_trans'][0, n, :2].double(), centre.double(), atol=1e-3)
    assert torch.equal(a['intrins'], c['intrins']) and torch.equal(a['k2s_sensor'], c['k2s_sensor'])


def test_every_frustum_is_separable_and_has_its_depth_count():
    for n_depth in inp.DEPTH_CFG:
        f = inp.frustum(n_depth)
        assert tuple(f.shape) == (n_depth, 8, 22, 3) and inp.separable(f)
        for dt in (torch.float16, torch.bfloat16):
            assert inp.separable(f.to(dt))
    assert inp.separable(inp.frustum(12, inp.SMALL_INPUT_SIZE))
    broken = inp.frustum(12).clone()
    broken[3, 2, 5, 0] += 0.5
    assert not inp.separable(broken)


def test_features_are_seeded_and_keep_the_cost_volume_from_being_one_hot():
    p1, c1 = inp.features(64, 8, 22)
    p2, c2 = inp.features(64, 8, 22)
    assert torch.equal(p1, p2) and torch.equal(c1, c2) and not torch.equal(p1, c1)
    m = inp.metas('a', 12)
    dn = inp.depthnet(12, 5.0)
    dn.use_hip_cost_volume = False
    m['cv_feat_list'] = [p1, c1]
    cv = dn.calculate_cost_volumn(m)
    assert float(cv.max()) < 0.9 and abs(float(cv.sum()) - 2 * 8 * 22) < 1e-2
