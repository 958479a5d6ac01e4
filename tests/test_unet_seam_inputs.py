"""The helpers of tests/unet_seam_inputs.py on the CPU: the pooling rule against F.max_pool2d (values, indices and autograd, both
layouts, the edge values), the up seam's float64 twin against a plain einsum restatement, and the shape grid's own claims."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_seam_inputs as US  # noqa: E402

LAYOUTS = [torch.contiguous_format, torch.channels_last]


def _torch_pool(x, gy):
    x = x.clone().requires_grad_()
    y, idx = F.max_pool2d(x, 2, return_indices=True)
    y.backward(gy)
    return y.detach(), idx, x.grad


@pytest.mark.parametrize('fmt', LAYOUTS, ids=['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype', [US.F32, US.BF16], ids=['f32', 'bf16'])
def test_the_rule_is_torchs_on_the_edge_values(dtype, fmt):
    """Four-way ties, windows of zeros, one and two NaNs, +inf, all -inf: values, indices and the routed gradient are identical."""
    x, gy = US.pool_edge_input(dtype)
    x, gy = x.contiguous(memory_format=fmt), gy.contiguous(memory_format=fmt)
    y, idx, gx = _torch_pool(x, gy)
    m, win = US.pool_rule(x)
    W = x.shape[3]
    i, j = torch.meshgrid(torch.arange(m.shape[2]), torch.arange(m.shape[3]), indexing='ij')
    flat = (2 * i + win // 2) * W + 2 * j + win % 2
    assert US.same_but_nan_payload(m, y) and torch.equal(flat, idx)
    assert US.same_but_nan_payload(US.pool_rule_grad(x, gy), gx)
    # what the edge windows are there for
    assert int(torch.isnan(y).sum()) >= 8 * 5 and int((y == float('-inf')).sum()) == 8 and int((y == float('inf')).sum()) >= 8 * 2
    assert bool((win[0, :, 0, 0] == 0).all()) and bool((win[0, :, 0, 7] == 0).all())        # a tie and all -inf keep the first


@pytest.mark.parametrize('fmt', LAYOUTS, ids=['nchw', 'nhwc'])
@pytest.mark.parametrize('shape', US.POOL_SHAPES, ids=str)
def test_the_rule_is_torchs_after_a_relu(shape, fmt):
    x, gy = US.pool_input(shape, US.F32)
    x, gy = x.contiguous(memory_format=fmt), gy.contiguous(memory_format=fmt)
    y, _, gx = _torch_pool(x, gy)
    assert torch.equal(US.pool_rule(x)[0], y) and torch.equal(US.pool_rule_grad(x, gy), gx)
    assert int((y == 0).sum()) > 0 or shape[2] * shape[3] <= 4                              # whole windows tie at zero
    B, C, H, W = shape
    assert bool((gx[:, :, 2 * (H // 2):] == 0).all()) and bool((gx[:, :, :, 2 * (W // 2):] == 0).all())


@pytest.mark.parametrize('case', US.UP_CASES)
def test_the_twin_is_the_einsum(case):
    v = US.up_inputs(case, 'f32')
    x1, x2, wgt, b = (v[k].double().requires_grad_() for k in ('x1', 'x2', 'weight', 'bias'))
    out = US.up_einsum(x1, x2, wgt, b)
    t = US.twin(case, 'f32')
    assert out.shape == t['out'].shape and torch.allclose(out, t['out'], rtol=0, atol=1e-12)
    out.backward(v['gout'].double())
    for k, g in (('gx1', x1.grad), ('gx2', x2.grad), ('gweight', wgt.grad), ('gbias', b.grad)):
        assert torch.allclose(g, t[k], rtol=0, atol=1e-11 * US.scale_of(t[k])), k
    C2 = x2.shape[1]
    assert torch.equal(t['out'][:, :C2], x2.detach()) and torch.equal(t['gx2'], v['gout'][:, :C2].double())


def test_the_grid_covers_what_it_says():
    pads, maps, batches, rows, cols_f, cols_b = set(), set(), set(), set(), set(), set()
    for B, Cin, Cout, C2, h, w, H, W in US.UP_CASES.values():
        assert Cin % 32 == 0 and Cout % 16 == 0 and C2 % 8 == 0 and H >= 2 * h and W >= 2 * w
        pads.add((H - 2 * h, W - 2 * w)); maps.add((h, w)); batches.add(B); rows.add(B * h * w); cols_f.add(4 * Cout); cols_b.add(Cin)
    assert {(0, 0), (1, 1), (0, 1), (3, 2)} <= pads and {(1, 1), (3, 5), (4, 4), (9, 8)} <= maps and batches == {1, 2, 3}
    assert {31, 32, 33} <= rows and {64, 128, 192} <= cols_f and {96, 128, 160} <= cols_b
    assert {(32, 16, 8), (64, 32, 32), (160, 80, 48), (128, 64, 64), (1024, 512, 512)} <= {c[1:4] for c in US.UP_CASES.values()}
