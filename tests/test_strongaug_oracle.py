"""tests/strongaug_ref.py (the float64 restatement of tssa.strong_augment and its tolerance) against hand-worked pixels for each step
and against scipy's mirrored correlation; tssa.gaussian_taps and tssa.StrongAugment (host code: no GPU); and, for every case of
tests/test_gpu_strongaug.py, the discriminating power of the tolerance (each of four wrong restatements -- taps of radius R - 1,
clamped instead of mirrored borders, the contrast mean taken before brightness, the hue shift negated -- leaves the true one by more
than 4x the tolerance somewhere in every sample where it can show) and the share of elements the first-order hue bound does not
cover (at most 1 %)."""
import numpy as np
import pytest

import torch_semantic_segmentation_amd as tssa
from torch_semantic_segmentation_amd import ops
from tests import strongaug_ref as R

TILE = ops.STRONGAUG_TILE
IDS = R.case_ids(TILE)


def one(x3, color, sigma=0.0, mean=None, std=None):
    """a constant-colour 9x16 sample through the restatement"""
    x = np.broadcast_to(np.asarray(x3, np.float64).reshape(1, 3, 1, 1), (1, 3, 9, 16)).copy()
    rad, taps = tssa.gaussian_taps(sigma)
    out, tol, _ = R.batch(x, np.asarray([list(color) + [0, 0, 0]], np.float32), [rad], [taps], mean, std)
    return out[0], tol[0]


def test_identity_is_none():
    out, tol = one((0.2, 0.4, 0.6), (0, 2.0, 0.5, 0.5, 0.25))
    assert out is None and tol is None


def test_brightness_by_hand():
    out, tol = one((0.2, 0.4, 0.6), (1, 2.0, 1, 1, 0))                   # (0.4, 0.8, 1.2 -> 1)
    assert np.allclose(out[:, 3, 5], [0.4, 0.8, 1.0], atol=1e-15) and tol.max() < 1e-5
    out, _ = one((0.2, 0.4, 0.6), (1, 0.0, 1, 1, 0))
    assert (out == 0).all()


def test_contrast_by_hand():
    # after brightness 2: (0.4, 0.8, 1.0), grey m = 0.299 0.4 + 0.587 0.8 + 0.114 = 0.7032; fc = 0.5: m + (u - m) / 2
    out, _ = one((0.2, 0.4, 0.6), (1, 2.0, 0.5, 1, 0))
    m = float(np.float32(0.7032))
    assert np.allclose(out[:, 0, 0], [(0.4 + m) / 2, (0.8 + m) / 2, (1.0 + m) / 2], atol=1e-15)
    out, _ = one((0.2, 0.4, 0.6), (1, 2.0, 0.0, 1, 0))                   # fc = 0: the whole sample is m, equal channels
    assert (out == m).all()
    # a two-valued image: m is the mean over the pixels, not the pixel's own grey value
    x = np.zeros((1, 3, 9, 16))
    x[0, :, :, 8:] = 1.0
    out, _, _ = R.batch(x, np.asarray([[1, 1, 2.0, 1, 0, 0, 0, 0]], np.float32), [0], [tssa.gaussian_taps(0)[1]])
    assert (out[0][:, :, :8] == 0.0).all() and np.allclose(out[0][:, :, 8:], 1.0, atol=1e-15)       # 0.5 + 2 (0 - 0.5) = -0.5 -> 0; 1.5 -> 1
    out, _, _ = R.batch(x, np.asarray([[1, 1, 0.5, 1, 0, 0, 0, 0]], np.float32), [0], [tssa.gaussian_taps(0)[1]])
    assert np.allclose(out[0][:, :, :8], 0.25) and np.allclose(out[0][:, :, 8:], 0.75)


def test_saturation_by_hand():
    g = 0.299 * 0.2 + 0.587 * 0.4 + 0.114 * 0.6                          # 0.3630
    out, _ = one((0.2, 0.4, 0.6), (1, 1, 1, 0.0, 0))
    assert np.allclose(out[:, 1, 1], [g, g, g], atol=1e-15) and (out[0] == out[1]).all() and (out[1] == out[2]).all()
    out, _ = one((0.2, 0.4, 0.6), (1, 1, 1, 2.0, 0))                     # g + 2 (u - g) = 2u - g
    assert np.allclose(out[:, 1, 1], [0.4 - g, 0.8 - g, 1.2 - g], atol=1e-15)


def test_hue_by_hand():
    third = float(np.float32(1.0 / 3.0))
    out, _ = one((1.0, 0.0, 0.0), (1, 1, 1, 1, third))                   # red turned by a third: green
    assert np.allclose(out[:, 2, 2], [0.0, 1.0, 0.0], atol=1e-6)
    out, _ = one((1.0, 0.0, 0.0), (1, 1, 1, 1, -third))                  # and the other way: blue
    assert np.allclose(out[:, 2, 2], [0.0, 0.0, 1.0], atol=1e-6)
    for dh in (0.5, -0.5):                                               # half a turn either way: cyan
        out, _ = one((1.0, 0.0, 0.0), (1, 1, 1, 1, dh))
        assert np.allclose(out[:, 2, 2], [0.0, 1.0, 1.0], atol=1e-15)
    out, _ = one((0.3, 0.3, 0.3), (1, 1, 1, 1, 0.25))                    # grey has no hue
    assert np.allclose(out, 0.3, atol=1e-15)
    out, _ = one((0.2, 0.4, 0.6), (1, 1, 1, 1, 0.0))
    assert np.allclose(out[:, 0, 0], [0.2, 0.4, 0.6], atol=1e-15)


def test_normalisation_round_trip_by_hand():
    mean, std = R.IMAGENET_MEAN, R.IMAGENET_STD
    x3 = [(v - m) / s for v, m, s in zip((0.2, 0.4, 0.6), mean, std)]
    out, tol = one(x3, (1, 2.0, 1, 1, 0), mean=mean, std=std)
    want = [(v - m) / s for v, m, s in zip((0.4, 0.8, 1.0), mean, std)]
    assert np.allclose(out[:, 4, 4], want, atol=1e-6) and tol.max() < 1e-5 / min(std)      # the raw bound over std


def test_blur_by_hand():
    rad, taps = tssa.gaussian_taps(0.6)
    assert rad == 2
    w = taps.astype(np.float64)
    x = np.zeros((1, 3, 9, 16))
    x[0, 0, 4, 8] = 1.0                       # an impulse in the interior: the outer product of the taps
    x[0, 1, 0, 0] = 1.0                       # one in the corner: the mirrored taps fold back onto it
    out, _, _ = R.batch(x, np.asarray([[0, 1, 1, 1, 0, 0, 0, 0]], np.float32), [rad], [taps])
    o = out[0]
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            assert np.isclose(o[0, 4 + dy, 8 + dx], w[abs(dy)] * w[abs(dx)], atol=1e-17)
    assert o[0, 4, 11] == 0.0
    # output (0,0) reads input (0,0) with w0; output (0,1) reads it with w1 (k = -1); output (0,2) with w2 (k = -2);
    # mirroring never reads index 0 twice (-1 -> 1, -2 -> 2)
    assert np.isclose(o[1, 0, 0], w[0] * w[0]) and np.isclose(o[1, 0, 1], w[0] * w[1]) and np.isclose(o[1, 1, 2], w[1] * w[2])
    assert o[1, 0, 3] == 0.0
    # an impulse at column 1 is read twice by output column 0: k = +1 and k = -1 -> refl(-1) = 1
    x = np.zeros((1, 3, 9, 16))
    x[0, 2, 4, 1] = 1.0
    o = R.batch(x, np.asarray([[0, 1, 1, 1, 0, 0, 0, 0]], np.float32), [rad], [taps])[0][0]
    assert np.isclose(o[2, 4, 0], w[0] * 2 * w[1]) and np.isclose(o[2, 4, 15], 0.0)
    x = np.zeros((1, 3, 9, 16))
    x[0, 2, 4, 14] = 1.0                      # W -> W - 2: output 15 reads 14 at k = -1 and at k = +1
    o = R.batch(x, np.asarray([[0, 1, 1, 1, 0, 0, 0, 0]], np.float32), [rad], [taps])[0][0]
    assert np.isclose(o[2, 4, 15], w[0] * 2 * w[1])


def test_blur_against_scipy():
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(5)
    a = rng.random((3, 11, 24))
    for sigma in (0.3, 1.15, 8.0 / 3.0):
        rad, taps = tssa.gaussian_taps(sigma)
        full = np.concatenate([taps[rad:0:-1], taps[:rad + 1]]).astype(np.float64)
        for axis in (1, 2):
            if a.shape[axis] <= rad:
                continue
            want = ndimage.correlate1d(a, full, axis=axis, mode='mirror')
            assert np.allclose(R.blur_axis(a, taps, rad, axis), want, rtol=0, atol=1e-15)


def test_gaussian_taps():
    for sigma, rad in ((0.0, 0), (0.15, 1), (1.0 / 3.0, 1), (1.15, 4), (8.0 / 3.0, 8)):
        r, taps = tssa.gaussian_taps(sigma)
        assert r == rad and taps.dtype == np.float32 and taps.shape == (12,) and (taps[r + 1:] == 0).all() and (taps[:r + 1] > 0).all()
        assert (np.diff(taps[:r + 1]) < 0).all()                                       # falls with |k|: symmetric by construction
        total = float(taps[0]) + 2.0 * float(taps[1:].astype(np.float64).sum())
        assert abs(total - 1.0) <= (2 * r + 1) * 2.0 ** -24                            # one float32 rounding (of a value < 1) per tap
        if r:
            k = np.arange(r + 1, dtype=np.float64)
            e = np.exp(-k * k / (2 * sigma * sigma))
            assert np.array_equal(taps[:r + 1], (e / (e[0] + 2 * e[1:].sum())).astype(np.float32))
    assert tssa.gaussian_taps(0.0)[1][0] == 1.0
    for bad in (-0.1, 2.7, float('nan')):
        with pytest.raises(ValueError):
            tssa.gaussian_taps(bad)


def test_draw_ranges_and_errors():
    sa = tssa.StrongAugment(color_p=0.7, brightness=0.4, contrast=1.5, saturation=0.25, hue=0.1, blur_p=0.6, sigma=(0.2, 2.0))
    color, radius, taps = sa.draw(4000, np.random.default_rng(3))
    assert color.shape == (4000, 8) and color.dtype == np.float32 and radius.dtype == np.int32 and taps.shape == (4000, 12)
    assert set(np.unique(color[:, 0])) == {0.0, 1.0} and 0.66 < color[:, 0].mean() < 0.74
    assert color[:, 1].min() >= np.float32(0.6) and color[:, 1].max() <= np.float32(1.4) and color[:, 1].std() > 0.2
    assert color[:, 2].min() >= 0.0 and color[:, 2].max() <= 2.5 and color[:, 2].max() > 2.3        # max(0, 1 - 1.5) = 0
    assert np.abs(color[:, 4]).max() <= np.float32(0.1) and (color[:, 5:] == 0).all()
    assert 0.36 < (radius == 0).mean() < 0.44 and radius.max() == 6 and radius[radius > 0].min() == 1     # ceil(3 * 0.2), ceil(3 * 2)
    assert (taps[radius == 0, 0] == 1).all()
    again = sa.draw(4000, np.random.default_rng(3))
    assert all(np.array_equal(a, b) for a, b in zip((color, radius, taps), again))
    d = tssa.StrongAugment()
    assert (d.color_p, d.brightness, d.contrast, d.saturation, d.hue, d.blur_p, d.sigma) == (0.8, 0.25, 0.25, 0.25, 0.25, 0.5, (0.15, 1.15))
    none = tssa.StrongAugment(color_p=0.0, blur_p=0.0).draw(16, np.random.default_rng(0))
    assert (none[0][:, 0] == 0).all() and (none[1] == 0).all()
    for kw in (dict(brightness=-0.1), dict(contrast=-1), dict(saturation=float('inf')), dict(hue=0.6), dict(hue=-0.1), dict(sigma=(0.1, 2.7)),
               dict(sigma=(-0.1, 1.0)), dict(sigma=(1.0, 0.5)), dict(color_p=1.5), dict(blur_p=-0.1), dict(std=(1, 0, 1)), dict(mean=(0, 0))):
        with pytest.raises(ValueError):
            tssa.StrongAugment(**kw)


def _feature_on(variant, color, rad):
    apply, fb, fc, fs, dh = (float(v) for v in color[:5])
    if variant in ('radius-1', 'clamp'):
        return rad > 0
    if variant == 'm-before':
        return apply != 0 and fb != 1.0 and fc != 1.0
    return apply != 0 and 0.0 < abs(dh) < 0.5 and fb * fc * fs > 0         # +-0.5 is the same turn either way; no chroma, no hue


@pytest.mark.parametrize('case_id', IDS)
def test_discriminating_power(case_id):
    c = R.case(case_id, TILE)
    out, tol, _ = R.reference(case_id, TILE)
    seen = 0
    for variant in R.VARIANTS:
        wrong = R.reference(case_id, TILE, variant)[0]
        for b in range(3):
            if not _feature_on(variant, c['color'][b], int(c['radius'][b])):
                continue
            seen += 1
            ratio = float((np.abs(wrong[b] - out[b]) / tol[b]).max())
            assert ratio > 4.0, (case_id, variant, b, ratio)
    assert seen > 0 or c['identity']


@pytest.mark.parametrize('case_id', IDS)
def test_fallback_share(case_id):
    share = R.fallback_share(case_id, TILE)
    assert share <= 0.01, (case_id, share)
    out, tol, _ = R.reference(case_id, TILE)
    for o, t in zip(out, tol):
        assert (o is None) == (t is None)
        if o is not None:
            assert np.isfinite(o).all() and np.isfinite(t).all() and (t > 0).all()


def test_exactly_grey_and_black_pixels_follow_the_definition():
    """without mean / std the planted pixels keep D = 0 exactly: equal channels out of the colour steps, and a tight bound there"""
    cid = 'mixed-23x40-f32-raw'
    c = R.case(cid, TILE)
    out, tol, fb = R.reference(cid, TILE)
    b = [i for i in range(3) if c['color'][i][0] != 0 and c['radius'][i] == 0][0]
    assert (out[b][0, 3:5, 5:7] == out[b][1, 3:5, 5:7]).all() and (out[b][1, 3:5, 5:7] == out[b][2, 3:5, 5:7]).all()
    assert not fb[b][3:5, 5:7].any() and not fb[b][6:8, 9:11].any() and tol[b][:, 3:5, 5:7].max() < 2e-6
    assert (out[b][:, 6:8, 9:11] >= 0).all()
