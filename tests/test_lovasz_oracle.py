"""The checker of the Lovasz-Softmax tests (tests/lovasz_ref.py) against the reference's own numbers
(tests/golden/lovasz.npz, written by tests/golden/make_lovasz_golden.py), and the closed-form Lovasz weights the HIP
kernel evaluates against the cumsum form the reference evaluates.  CPU only."""
import os

import numpy as np
import pytest
import torch

from tests import cases, lovasz_ref as R


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return cases.load_npz(os.path.join(golden_dir, 'lovasz.npz'))


def test_fixture_is_what_its_docstring_says(fixture):
    t = fixture['target']
    assert fixture['logits'].shape == (1, 7, 16, 24) and fixture['logits'].dtype == np.float32
    assert (t == 5).sum() == 0 and 0.05 < (t == 255).mean() < 0.15
    assert sorted(set(np.unique(t)) - {255}) == [0, 1, 2, 3, 4, 6]


@pytest.mark.parametrize('name,ignore', [('ignore255', 255), ('ignore_none', None)])
def test_restatement_reproduces_the_reference(fixture, name, ignore):
    """variant='reference' in f32: the reference's loss bit for bit, its gradient within 1e-6."""
    logits, target = torch.from_numpy(fixture['logits']), torch.from_numpy(fixture['target'])
    loss, grad = R.loss_and_grad(logits, target, 7, ignore, 'reference', torch.float32)
    assert loss.numpy().astype(np.float32).tobytes() == fixture[name + '/loss'].tobytes(), (float(loss), float(fixture[name + '/loss']))
    assert cases.rel_err(grad.numpy(), fixture[name + '/grad']) <= 1e-6
    # and the f64 mode is the same function: it agrees with the f32 one to f32 rounding
    loss64, _ = R.loss_and_grad(logits, target, 7, ignore, 'reference', torch.float64)
    assert abs(float(loss64) / float(loss) - 1) < 1e-5


def _sorted_flags(seed, n, frac):
    g = torch.Generator().manual_seed(seed)
    fg = (torch.rand(n, generator=g) < frac).double()
    fg[int(torch.randint(0, n, (1,), generator=g))] = 1.0        # at least one foreground element
    return fg


@pytest.mark.parametrize('variant', R.VARIANTS)
@pytest.mark.parametrize('n,frac', [(1, 1.0), (2, 0.5), (7, 0.3), (1000, 0.05), (4097, 0.5), (20000, 0.001)])
def test_closed_form_weights_equal_the_cumsum_form(variant, n, frac):
    """g_r in closed form from integers == the cumsum form in f64, for both variants.  Bound: the cumsum form subtracts two
    Jaccard values of size <= 1, each a few f64 roundings -> absolute 1e-14; the closed form has no cancellation."""
    for seed in range(3):
        fg = _sorted_flags(seed, n, frac)
        want = R.lovasz_weights(fg.clone(), variant)
        got = R.closed_form_weights(fg, variant)
        assert got.dtype == torch.float64 and want.dtype == torch.float64
        assert float((got - want).abs().max()) <= 1e-14
    for first in (0.0, 1.0):                                     # both kinds of rank 0
        fg = _sorted_flags(7, max(n, 2), frac)
        fg[0] = first
        fg[-1] = 1.0
        assert float((R.closed_form_weights(fg, variant) - R.lovasz_weights(fg.clone(), variant)).abs().max()) <= 1e-14


def test_berman_weights_are_nonnegative_and_sum_to_the_last_jaccard():
    fg = _sorted_flags(3, 500, 0.2)
    g = R.closed_form_weights(fg, 'berman')
    assert (g >= 0).all() and abs(float(g.sum()) - 1.0) < 1e-12   # J of the full set is 1 - 0/U = 1


@pytest.mark.parametrize('ignore', [255, None])
def test_berman_loss_is_in_the_unit_interval(fixture, ignore):
    logits, target = torch.from_numpy(fixture['logits']), torch.from_numpy(fixture['target'])
    for gain in (0.0, 1.0, 10.0):
        loss, _ = R.loss_and_grad(gain * logits, target, 7, ignore, 'berman', torch.float64)
        assert 0.0 <= float(loss) <= 1.0
    ref_loss, _ = R.loss_and_grad(logits, target, 7, ignore, 'reference', torch.float64)
    assert float(ref_loss) > 1.0                                  # the reference's weighting grows with the pixel count


def test_stable_sort_changes_nothing_without_ties(fixture):
    logits, target = torch.from_numpy(fixture['logits']), torch.from_numpy(fixture['target'])
    assert R.tie_free(logits, target, 7, 255)
    for variant in R.VARIANTS:
        a = R.loss_and_grad(logits, target, 7, 255, variant, torch.float64, stable=False)
        b = R.loss_and_grad(logits, target, 7, 255, variant, torch.float64, stable=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_no_class_present_gives_zero():
    logits = torch.randn(1, 4, 4, 8)
    target = torch.full((1, 4, 8), 255)
    loss, grad = R.loss_and_grad(logits, target, 4, 255, 'reference', torch.float64)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0
