"""CPU (no GPU): the float64 restatement of the multi-scale + flip fusion (tests/msflip_ref.py) against stock torch, and the
derived score margin against float32 torch and against the top-2 gaps of the test inputs."""
import pytest
import torch
import torch.nn.functional as F

from tests import msflip_ref as R

MODES = ('softmax', 'logits')


@pytest.fixture(scope='module')
def maps():
    return R.make_maps()


def _margin(lows, average, size=R.OUT):
    zmax = max(float(low.abs().max()) for low in lows)
    return R.margin(len(lows), lows[0].shape[1], zmax, [tuple(low.shape[-2:]) for low in lows], size, average)


@pytest.mark.parametrize('average', MODES)
def test_single_plain_map_is_interpolate_argmax(maps, average):
    low = maps[0][4]                                          # 8 x 16
    score, pred = R.scores([low], [False], R.OUT, average)
    up = F.interpolate(low.double(), size=R.OUT, mode='bilinear', align_corners=True)
    assert torch.equal(pred, up.argmax(1))                    # softmax is monotone: the same arg-max in both modes
    if average == 'logits':
        assert torch.equal(score, up)


@pytest.mark.parametrize('average', MODES)
def test_flipped_map_of_mirrored_input_gives_mirrored_scores(maps, average):
    lows, flips = maps
    plain, _ = R.scores(lows, flips, R.OUT, average)
    # upsample(flip(low)) is flip(upsample(low)) up to the rounding of the mirrored weights (l0 <-> l1), a few float64 ulps:
    # mirroring every map mirrors the scores ...
    mirrored, _ = R.scores([low.flip(-1) for low in lows], flips, R.OUT, average)
    assert torch.allclose(mirrored, plain.flip(-1), rtol=0, atol=1e-12)
    # ... and a map computed from the mirrored input and flagged `flip` scores like the plain map of the plain input
    one, _ = R.scores([lows[6].flip(-1)], [True], R.OUT, average)
    ref, _ = R.scores([lows[6]], [False], R.OUT, average)
    assert torch.allclose(one, ref, rtol=0, atol=1e-12)
    both, _ = R.scores([low.flip(-1) for low in lows], [not f for f in flips], R.OUT, average)
    assert torch.allclose(both, plain, rtol=0, atol=1e-12)


@pytest.mark.parametrize('average', MODES)
def test_float32_torch_stays_inside_the_margin(maps, average):
    lows, flips = maps
    s64, _ = R.scores(lows, flips, R.OUT, average)
    s32, _ = R.scores(lows, flips, R.OUT, average, dtype=torch.float32)
    err = float((s32.double() - s64).abs().max())
    m = _margin(lows, average)
    print('%s: float32 torch max |score - f64| = %.3e, margin %.3e' % (average, err, m))
    assert err <= m


@pytest.mark.parametrize('average', MODES)
def test_margin_excludes_at_most_one_percent_of_the_pixels(maps, average):
    lows, flips = maps
    s64, _ = R.scores(lows, flips, R.OUT, average)
    m = _margin(lows, average)
    # both the best and the runner-up score may be off by the margin, so the cap is held at twice it (it then holds at the margin too)
    share = float((R.top2_gap(s64) <= 2 * m).double().mean())
    print('%s: margin %.3e, share of pixels with gap <= 2 margin: %.4f' % (average, m, share))
    assert 2 * m <= 1e-3                                   # the band stays inside the range the gap statistics were taken in
    assert share <= 0.01


def test_coordinate_error_is_zero_for_identity_and_small_otherwise():
    assert R.coord_error(40, 40) == 0.0 and R.coord_error(1, 72) == 0.0 and R.coord_error(10, 33) == 0.0   # 9/32 is exact
    for n_in, n_out in ((5, 40), (9, 72), (18, 70), (10, 34)):
        e = R.coord_error(n_in, n_out)
        assert 0.0 < e <= 2 * R.U * (n_in - 1)               # never above the two-rounding bound


def test_confusion_restatement_skips_ignored_and_out_of_range():
    pred = torch.tensor([0, 1, 2, 1, 0])
    target = torch.tensor([0, 255, 2, 7, 1])
    cm = R.confusion(pred, target, 3)
    assert cm.sum() == 3 and cm[0, 0] == 1 and cm[2, 2] == 1 and cm[1, 0] == 1
