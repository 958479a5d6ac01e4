"""The inputs the deform_conv tests measure against are what dcn_train_inputs.py says they are (no GPU)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_infer_inputs as DI  # noqa: E402
import dcn_train_inputs as TI  # noqa: E402


def test_the_cases_are_the_inference_cases_and_two_more():
    assert list(TI.CASES)[:len(DI.CASES)] == list(DI.CASES) and all(TI.CASES[k] == v for k, v in DI.CASES.items())
    assert TI.CASES['pileup'][:7] == (1, 32, 32, 4, 6, 10, 1) and TI.CASES['zero_offset'][:7] == (2, 64, 64, 4, 5, 9, 1)
    for case in DI.CASES:
        x, offset, weight, gout = TI.inputs(case)
        xi, oi, wi = DI.inputs(case)
        assert x is xi and weight is wi and gout.shape == (x.shape[0], weight.shape[0]) + x.shape[2:]
        moved = offset != oi
        assert float(moved.float().mean()) < 0.02 and bool(((offset - oi)[moved] - TI.NUDGE).abs().max() < 1e-5 if moved.any() else True)
    assert not bool(TI.inputs('zero_offset')[1].any())


@pytest.mark.parametrize('case', list(TI.CASES))
def test_no_sampling_coordinate_is_left_at_a_kink(case):
    TI.assert_no_kinks(case)
    if case != 'zero_offset':
        assert TI.kinks(case, TI.inputs(case)[1]) == 0
    if case in DI.CASES and case not in ('one_cell_1x256x1x1',):
        assert TI.kinks(case, DI.inputs(case)[1]) > 0          # the helper had something to move


def test_pileup_lands_within_one_cell_of_its_target():
    co = TI.coordinates('pileup', TI.inputs('pileup')[1])
    assert float(abs(co[:, :, 0] - 2.0).max()) < 1.0 + 2 * TI.NUDGE and float(abs(co[:, :, 1] - 3.0).max()) < 1.0 + 2 * TI.NUDGE


@pytest.mark.parametrize('case', ['g13_2x32x6x10', 'g1_3x64to128x7x9_dil2', 'outside_2x128to64x5x70', 'pileup', 'zero_offset'])
def test_the_twin_is_float64_autograd_through_the_grid_sample_formulation(case):
    """dx and dW of the twin against float64 autograd through DCN's grid_sample formulation (CPU tensors take it), to 1e-10.  (A
    map with H or W of 1 is left out: the formulation's normalisation divides by max(W - 1, 1).)"""
    x, offset, weight, gout = TI.inputs(case)
    tw = TI.twin(case, 'f32_bf16x3')
    m = TI.dcn_module(case, weight.double(), offset.double(), dtype=torch.float64)
    xd = x.double().requires_grad_()
    out = m(xd)
    out.backward(gout.double())
    assert float((out.detach() - tw['out']).abs().max()) <= 1e-10
    assert float((xd.grad - tw['dx']).abs().max()) <= 1e-10 and float((m.weight.grad - tw['dw']).abs().max()) <= 1e-10


def test_at_zero_offsets_the_twin_is_the_plain_convolution():
    b, c, o, g, h, w, dil, scale = TI.CASES['zero_offset']
    x, offset, weight, gout = TI.inputs('zero_offset')
    for prec in TI.PRECISIONS:
        xs, gs = (t.double() for t in TI.stored('zero_offset', prec))
        xs.requires_grad_()
        wd = weight.double().requires_grad_()
        out = F.conv2d(xs, wd, padding=dil, dilation=dil, groups=g)
        out.backward(gs)
        tw = TI.twin('zero_offset', prec)
        for got, k in ((out.detach(), 'out'), (xs.grad, 'dx'), (wd.grad, 'dw')):
            assert float((got - tw[k]).abs().max()) <= 1e-10, (prec, k)


def test_the_bar():
    assert TI.bar('f32_bf16x3', 0.5) == TI.E_F32 == 1e-4 and TI.bar('fp16', 1e-3) == 1.5e-3 and TI.bar('bf16', 1e-6) == TI.E_F32
