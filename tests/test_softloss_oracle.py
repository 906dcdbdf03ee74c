"""The checker of the focal / Dice tests (tests/softloss_ref.py) against the reference's own focal numbers
(tests/golden/focal.npz, written by tests/golden/make_focal_golden.py), against the closed-form gradients the HIP kernels
evaluate (csrc/softloss.hip), and against values worked by hand.  CPU only."""
import os

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from tests import cases, softloss_ref as R

GAMMAS = (2.0, 0.5)


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return cases.load_npz(os.path.join(golden_dir, 'focal.npz'))


def _random_case(seed, B=2, C=6, H=4, W=8, gain=3.0):
    g = torch.Generator().manual_seed(seed)
    logits = gain * torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < 0.1] = 255
    target.view(-1)[[1, 9]] = -1
    target.view(-1)[[4]] = 300
    return logits, target


def test_fixture_is_what_its_docstring_says(fixture):
    t = fixture['target']
    assert fixture['logits'].shape == (1, 7, 16, 24) and fixture['logits'].dtype == np.float32
    assert 0.05 < (t == 255).mean() < 0.15
    assert sorted(set(np.unique(t)) - {255}) == list(range(7))
    assert sorted(k for k in fixture if k.endswith('/loss')) == ['gamma0.5/loss', 'gamma2.0/loss']


@pytest.mark.parametrize('gamma', GAMMAS)
def test_focal_restatement_reproduces_the_reference(fixture, gamma):
    """variant='reference' in f32: the reference's loss within 1e-6 relative, its gradient within rel_err 1e-6 (the two
    differ in how q is formed: sum of the other classes here, 1 - s_t there)."""
    logits, target = torch.from_numpy(fixture['logits']), torch.from_numpy(fixture['target'])
    loss, grad = R.loss_and_grad(R.focal_loss, logits, target, torch.float32, 0.25, gamma, 255, 'reference')
    want_loss, want_grad = float(fixture['gamma%s/loss' % gamma]), fixture['gamma%s/grad' % gamma]
    d_loss, d_grad = abs(float(loss) / want_loss - 1), cases.rel_err(grad.numpy(), want_grad)
    print('focal fixture gamma %s: loss %.7f rel %.2e, grad rel_err %.2e' % (gamma, want_loss, d_loss, d_grad))
    assert d_loss <= 1e-6
    assert d_grad <= 1e-6
    loss64, _ = R.loss_and_grad(R.focal_loss, logits, target, torch.float64, 0.25, gamma, 255, 'reference')
    assert abs(float(loss64) / want_loss - 1) < 1e-5


@pytest.mark.parametrize('variant', R.FOCAL_VARIANTS)
@pytest.mark.parametrize('gamma', [0.0, 0.5, 1.0, 2.0])
@pytest.mark.parametrize('ignore', [255, None])
def test_focal_autograd_equals_the_closed_form(variant, gamma, ignore):
    for seed in range(3):
        logits, target = _random_case(seed)
        _, grad = R.loss_and_grad(R.focal_loss, logits, target, torch.float64, 0.25, gamma, ignore, variant)
        want = R.focal_grad_closed_form(logits, target, 0.25, gamma, ignore, variant)
        assert cases.rel_err(grad.numpy(), want.numpy()) <= 1e-12
        assert float(grad.abs().max()) > 0


@pytest.mark.parametrize('smooth', [1.0, 0.0])
@pytest.mark.parametrize('ignore', [255, None])
def test_dice_autograd_equals_the_closed_form(smooth, ignore):
    for seed in range(3):
        logits, target = _random_case(seed)
        if seed == 2:
            target[target == 3] = 4                       # an absent class
        _, grad = R.loss_and_grad(R.dice_loss, logits, target, torch.float64, 6, smooth, ignore)
        want = R.dice_grad_closed_form(logits, target, 6, smooth, ignore)
        assert cases.rel_err(grad.numpy(), want.numpy()) <= 1e-12
        assert float(grad.abs().max()) > 0


def test_dice_hand_worked_case():
    """1x2x1x8, class-0 probabilities 1/2 1/4 3/4 1/2 1/8 7/8 1/2 1/4, labels 0 1 0 1 1 0 255 0, ignore 255, smooth 1.
    Over the 7 valid pixels: sum p_0 = 13/4, sum p_1 = 15/4, counts 4 and 3, I_0 = 1/2 + 3/4 + 7/8 + 1/4 = 19/8,
    I_1 = 3/4 + 1/2 + 7/8 = 17/8.  dice_0 = (19/4 + 1) / (29/4 + 1) = 23/33, dice_1 = (17/4 + 1) / (27/4 + 1) = 21/31,
    loss = 1 - (23/33 + 21/31) / 2 = 320/1023."""
    p0 = torch.tensor([1 / 2, 1 / 4, 3 / 4, 1 / 2, 1 / 8, 7 / 8, 1 / 2, 1 / 4], dtype=torch.float64)
    logits = torch.log(torch.stack([p0, 1 - p0])).reshape(1, 2, 1, 8)
    target = torch.tensor([0, 1, 0, 1, 1, 0, 255, 0]).reshape(1, 1, 8)
    assert abs(float(R.dice_loss(logits, target, 2, 1.0, 255)) - 320 / 1023) <= 1e-14
    assert abs(float(R.dice_loss(logits.float(), target, 2, 1.0, 255)) - 320 / 1023) <= 1e-6
    # smooth = 0: 1 - (19/29 + 17/27) / 2 = 1 - 503/783 = 280/783
    assert abs(float(R.dice_loss(logits, target, 2, 0.0, 255)) - 280 / 783) <= 1e-14


@pytest.mark.parametrize('smooth', [1.0, 0.0])
def test_dice_with_every_pixel_ignored(smooth):
    logits = torch.randn(1, 4, 4, 8, dtype=torch.float64)
    for target in (torch.full((1, 4, 8), 255), torch.full((1, 4, 8), -1), torch.full((1, 4, 8), 4)):
        loss, grad = R.loss_and_grad(R.dice_loss, logits, target, torch.float64, 4, smooth, 255)
        assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0
        assert float(R.dice_grad_closed_form(logits, target, 4, smooth, 255).abs().max()) == 0.0
    loss, grad = R.loss_and_grad(R.focal_loss, logits, torch.full((1, 4, 8), 255), torch.float64, 0.25, 2.0, 255, 'reference')
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


def test_dice_counts_an_absent_class():
    """A class no valid pixel carries still enters the mean over C: its term is 1 - smooth / (sum p_c + smooth)."""
    logits, target = _random_case(5)
    target[target == 2] = 1
    p = F.softmax(logits, 1)
    valid = R.valid_mask(target, 6, 255)
    s2 = float(p[:, 2][valid].sum())
    full = float(R.dice_loss(logits, target, 6, 1.0, 255))
    others = [c for c in range(6) if c != 2]
    # the same loss from the per-class terms, class 2 by its closed form
    terms = []
    for c in others:
        pc, fg = p[:, c][valid], (target[valid] == c).double()
        terms.append(1 - (2 * float((pc * fg).sum()) + 1) / (float(pc.sum() + fg.sum()) + 1))
    terms.append(1 - 1 / (s2 + 1))
    assert abs(full - sum(terms) / 6) <= 1e-14


def test_lin_at_gamma_zero_is_alpha_times_cross_entropy():
    logits, target = _random_case(3)
    for alpha in (0.25, 1.0):
        loss, grad = R.loss_and_grad(R.focal_loss, logits, target, torch.float64, alpha, 0.0, 255, 'lin')
        x = logits.clone().requires_grad_(True)
        t = torch.where(R.valid_mask(target, 6, 255), target, torch.full_like(target, 255))   # out-of-range labels -> ignored
        ce = alpha * F.cross_entropy(x, t, ignore_index=255)
        ce.backward()
        assert abs(float(loss) / float(ce.detach()) - 1) <= 1e-14
        assert cases.rel_err(grad.numpy(), x.grad.numpy()) <= 1e-13


def test_reference_variant_weights_with_exp_of_the_published_weight():
    """One pixel, two classes, p_t = 1/4: q = 3/4, gamma = 2 -> lin 9/16 * log 4 * alpha, reference exp(9/16) * log 4 * alpha."""
    logits = torch.log(torch.tensor([1 / 4, 3 / 4], dtype=torch.float64)).reshape(1, 2, 1, 1).repeat(1, 1, 1, 8)
    target = torch.zeros(1, 1, 8, dtype=torch.int64)
    lin = float(R.focal_loss(logits, target, 0.25, 2.0, None, 'lin'))
    ref = float(R.focal_loss(logits, target, 0.25, 2.0, None, 'reference'))
    assert abs(lin - 0.25 * 9 / 16 * np.log(4)) <= 1e-15
    assert abs(ref - 0.25 * np.exp(9 / 16) * np.log(4)) <= 1e-15
