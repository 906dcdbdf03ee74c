"""Pins tests/distill_ref.py (the restatement the GPU tests of the distillation kernels compare against) to F.kl_div, to a
hand-worked value and to the properties of the formulas.  CPU only."""
import math

import pytest
import torch
from torch.nn import functional as F

from tests import distill_ref as R

TAUS = (1.0, 4.0, 0.5)


def inputs(shape=(2, 5, 3, 4), seed=11):
    g = torch.Generator().manual_seed(seed)
    return 2.0 * torch.randn(*shape, generator=g, dtype=torch.float64), 2.0 * torch.randn(*shape, generator=g, dtype=torch.float64)


@pytest.mark.parametrize('tau', TAUS)
def test_pixel_kind_is_kl_div_over_the_class_axis(tau):
    s, t = inputs()
    B, C, h, w = s.shape
    want = F.kl_div(F.log_softmax(s / tau, 1), F.softmax(t / tau, 1), reduction='sum') * tau ** 2 / (B * h * w)
    got = R.distillation_loss(s, t, tau, 'pixel')
    assert abs(float(got) - float(want)) <= 1e-13 * abs(float(want))


@pytest.mark.parametrize('tau', TAUS)
def test_channel_kind_is_kl_div_over_the_rows_of_positions(tau):
    s, t = inputs()
    B, C, h, w = s.shape
    rs, rt = s.reshape(B * C, h * w), t.reshape(B * C, h * w)
    want = F.kl_div(F.log_softmax(rs / tau, 1), F.softmax(rt / tau, 1), reduction='sum') * tau ** 2 / (B * C)
    got = R.distillation_loss(s, t, tau, 'channel')
    assert abs(float(got) - float(want)) <= 1e-13 * abs(float(want))


@pytest.mark.parametrize('tau', TAUS)
def test_hand_worked_value(tau):
    """C = 2, one pixel, s = (0, 0), t = (tau ln 3, 0): p = (3/4, 1/4), q = (1/2, 1/2),
    loss = tau^2 (3/4 ln 1.5 + 1/4 ln 0.5) = 0.1308120 tau^2."""
    s = torch.zeros(1, 2, 1, 1, dtype=torch.float64)
    t = torch.tensor([tau * math.log(3.0), 0.0], dtype=torch.float64).view(1, 2, 1, 1)
    want = tau ** 2 * (0.75 * math.log(1.5) + 0.25 * math.log(0.5))
    assert abs(want / tau ** 2 - 0.1308120) < 5e-8
    assert abs(float(R.distillation_loss(s, t, tau, 'pixel')) - want) <= 1e-14 * tau ** 2
    # the same two numbers as the two positions of one plane
    got = R.distillation_loss(s.view(1, 1, 2, 1), t.view(1, 1, 2, 1), tau, 'channel')
    assert abs(float(got) - want) <= 1e-14 * tau ** 2
    _, g = R.loss_and_grad(s, t, torch.float64, tau, 'pixel')
    assert torch.allclose(g.flatten(), torch.tensor([-0.25, 0.25], dtype=torch.float64) * tau, rtol=1e-13, atol=0)


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('tau', TAUS)
def test_gradient_is_the_closed_form_and_its_rows_sum_to_zero(kind, tau):
    s, t = inputs()
    _, g = R.loss_and_grad(s, t, torch.float64, tau, kind)
    assert torch.allclose(g, R.grad_closed_form(s, t, tau, kind), rtol=1e-11, atol=1e-15)
    rows = g.sum(1) if kind == 'pixel' else g.flatten(2).sum(2)
    assert float(rows.abs().max()) <= 1e-15
    assert float(g.abs().max()) > 1e-3


@pytest.mark.parametrize('kind', R.KINDS)
def test_identical_inputs_give_zero(kind):
    s, _ = inputs()
    loss, g = R.loss_and_grad(s, s.clone(), torch.float64, 4.0, kind)
    # the value and the closed-form gradient exactly; autograd's chain through log_softmax to a few f64 roundings
    assert float(loss) == 0.0 and float(g.abs().max()) <= 1e-15
    assert float(R.grad_closed_form(s, s.clone(), 4.0, kind).abs().max()) == 0.0


def test_teacher_is_a_constant():
    s, t = inputs()
    s.requires_grad_(True)
    t.requires_grad_(True)
    R.distillation_loss(s, t, 2.0, 'pixel').backward()
    assert t.grad is None and s.grad is not None


def test_units():
    assert R.units((2, 19, 8, 16), 'pixel') == (256, 19) and R.units((2, 19, 8, 16), 'channel') == (38, 128)
