"""tests/wce_ref.py against torch: the restatement of the class-weighted, label-smoothed cross-entropy equals
F.cross_entropy(..., weight=, ignore_index=, label_smoothing=) in f64, its closed-form gradient equals autograd's, out-of-range
labels behave as ignored, an empty denominator gives nan with a zero gradient, and a two-pixel case worked by hand."""
import math

import pytest
import torch
from torch.nn import functional as F

from tests import wce_ref as R

C = 7
COMBOS = pytest.mark.parametrize('weighted,eps', [(True, 0.0), (False, 0.1), (True, 0.1)], ids=['w', 'eps', 'w_eps'])


def inputs(seed=11, out_of_range=False):
    g = torch.Generator().manual_seed(seed)
    x = 2.0 * torch.randn(2, C, 6, 8, generator=g, dtype=torch.float64)
    t = torch.randint(0, C, (2, 6, 8), generator=g)
    t[torch.rand(2, 6, 8, generator=g) < 0.15] = 255
    if out_of_range:
        flat = t.view(-1)
        flat[[2, 30, 61]] = -1
        flat[[9, 44]] = 300
    w = torch.rand(C, generator=g, dtype=torch.float64) * 49 + 1
    w[3] = 0.0
    return x, t, w


def torch_loss_and_grad(x, t, w, eps, low_size=None):
    x = x.detach().clone().requires_grad_(True)
    z = x if low_size is None else F.interpolate(x, size=tuple(t.shape[-2:]), mode='bilinear', align_corners=True)
    loss = F.cross_entropy(z, t, weight=w, ignore_index=255, label_smoothing=eps)
    loss.backward()
    return loss.detach(), x.grad


@COMBOS
def test_restatement_equals_torch_in_f64(weighted, eps):
    x, t, w = inputs()
    w = w if weighted else None
    want, want_grad = torch_loss_and_grad(x, t, w, eps)
    got, got_grad = R.loss_and_grad(R.wce_loss, x, t, torch.float64, w, 255, eps)
    assert abs(float(got) / float(want) - 1) <= 1e-12
    assert float((got_grad - want_grad).abs().max()) <= 1e-12 * float(want_grad.abs().max())
    closed = R.wce_grad_closed_form(x, t, w, 255, eps)
    assert float((closed - want_grad).abs().max()) <= 1e-12 * float(want_grad.abs().max())


@COMBOS
def test_upsampled_restatement_equals_torch_in_f64(weighted, eps):
    x, _, w = inputs()
    w = w if weighted else None
    g = torch.Generator().manual_seed(5)
    t = torch.randint(0, C, (2, 24, 32), generator=g)
    t[torch.rand(2, 24, 32, generator=g) < 0.15] = 255
    want, want_grad = torch_loss_and_grad(x, t, w, eps, low_size=True)
    got, got_grad = R.loss_and_grad(R.upsampled_wce_loss, x, t, torch.float64, w, 255, eps)
    assert abs(float(got) / float(want) - 1) <= 1e-12
    assert float((got_grad - want_grad).abs().max()) <= 1e-12 * float(want_grad.abs().max())
    closed = R.upsampled_wce_grad_closed_form(x, t, w, 255, eps)
    assert float((closed - want_grad).abs().max()) <= 1e-12 * float(want_grad.abs().max())


@COMBOS
def test_out_of_range_labels_behave_as_ignored(weighted, eps):
    x, t, w = inputs(out_of_range=True)
    w = w if weighted else None
    assert int((t == -1).sum()) == 3 and int((t == 300).sum()) == 2
    clean = t.clone()
    clean[(t < 0) | (t >= C)] = 255               # torch raises on the labels themselves
    want, want_grad = torch_loss_and_grad(x, clean, w, eps)
    got, got_grad = R.loss_and_grad(R.wce_loss, x, t, torch.float64, w, 255, eps)
    assert abs(float(got) / float(want) - 1) <= 1e-12
    assert float((got_grad - want_grad).abs().max()) <= 1e-12 * float(want_grad.abs().max())
    assert float(got_grad.movedim(1, -1)[(t < 0) | (t >= C)].abs().max()) == 0.0


def test_empty_denominator_gives_nan_and_a_zero_gradient():
    x, t, w = inputs()
    every_ignored = torch.full_like(t, 255)
    only_weightless = torch.where(t == 255, t, torch.full_like(t, 3))        # w[3] == 0
    for target in (every_ignored, only_weightless):
        for eps in (0.0, 0.1):
            assert math.isnan(float(R.wce_loss(x, target, w, 255, eps)))
            assert math.isnan(float(F.cross_entropy(x, target, weight=w, ignore_index=255, label_smoothing=eps)))
            assert float(R.wce_grad_closed_form(x, target, w, 255, eps).abs().max()) == 0.0
    assert math.isnan(float(R.wce_loss(x, every_ignored, None, 255, 0.1)))


def test_two_pixels_by_hand():
    """C = 2, w = (1, 3).  Pixel 1: x = (0, 0), t = 0: lse = ln 2.  Pixel 2: x = (ln 3, 0), t = 1: lse = ln 4, p = (3/4, 1/4).
    eps = 0:   den = 4, loss = (1 ln 2 + 3 ln 4) / 4 = 7 ln 2 / 4.
    eps = 0.2: pixel 1: 0.8 ln 2 + 0.1 (1 ln 2 + 3 ln 2) = 1.2 ln 2;  pixel 2: 0.8 * 3 ln 4 + 0.1 (1 (ln 4 - ln 3) + 3 ln 4)
               = 5.6 ln 2 - 0.1 ln 3;  loss = (6.8 ln 2 - 0.1 ln 3) / 4.
    Gradient of pixel 2 at eps = 0.2: s = 0.8 * 3 + 0.2 * 4 / 2 = 2.8, hot = (0.1 * 1, 2.4 + 0.1 * 3) = (0.1, 2.7):
               (2.8 * 3/4 - 0.1, 2.8 / 4 - 2.7) / 4 = (0.5, -0.5)."""
    x = torch.tensor([[[[0.0, math.log(3.0)]], [[0.0, 0.0]]]], dtype=torch.float64)        # (1, 2, 1, 2)
    t = torch.tensor([[[0, 1]]])
    w = torch.tensor([1.0, 3.0], dtype=torch.float64)
    ln2, ln3 = math.log(2.0), math.log(3.0)
    assert abs(float(R.wce_loss(x, t, w, 255, 0.0)) - 7 * ln2 / 4) <= 1e-14
    assert abs(float(R.wce_loss(x, t, w, 255, 0.2)) - (6.8 * ln2 - 0.1 * ln3) / 4) <= 1e-14
    g = R.wce_grad_closed_form(x, t, w, 255, 0.2)
    assert torch.allclose(g[0, :, 0, 1], torch.tensor([0.5, -0.5], dtype=torch.float64), atol=1e-14)
    # pixel 1: s = 0.8 + 0.4 = 1.2, hot = (0.8 + 0.1, 0.3): (0.6 - 0.9, 0.6 - 0.3) / 4
    assert torch.allclose(g[0, :, 0, 0], torch.tensor([-0.075, 0.075], dtype=torch.float64), atol=1e-14)
