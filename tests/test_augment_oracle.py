"""CPU (no GPU): pins tests/augment_ref.py, the restatement the GPU tests of tss_augment_batch_u8 compare against, and the host
side of the feature (TrainAugment.draw, argument checks)."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

from tests import augment_ref as R

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
H, W = 20, 36


def source(seed=0, B=2, C=3, h=H, w=W):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (B, C, h, w)).astype(np.uint8)
    tgt = rng.randint(0, 19, (B, h, w)).astype(np.uint8)
    tgt[rng.rand(B, h, w) < 0.1] = 255
    return img, tgt


def test_identity_scale_is_slice_plus_normalize_exactly():
    img, tgt = source()
    mean, std = IMAGENET
    rows = [[H, W, 0, 0, 0, 0], [H, W, 12, 20, 0, 0]]
    x, y = R.augment(img, tgt, rows, (8, 16), mean, std)
    sc, sh = R.constants(3, mean, std)
    for b, (oy, ox) in enumerate([(0, 0), (12, 20)]):
        want = img[b, :, oy:oy + 8, ox:ox + 16].astype(np.float64) * sc[:, None, None] + sh[:, None, None]
        assert np.array_equal(x[b], want)
        assert np.array_equal(y[b], tgt[b, oy:oy + 8, ox:ox + 16].astype(np.int64))
    # the constants are the float32 ones of the C entry: (x / 255 - mean) / std to float32 accuracy
    plain = (img[0, :, :8, :16] / 255.0 - np.array(mean)[:, None, None]) / np.array(std)[:, None, None]
    assert np.abs(x[0] - plain).max() < 1e-6
    x1, _ = R.augment(img, None, rows, (8, 16))
    assert np.array_equal(x1[0], img[0, :, :8, :16].astype(np.float64) * float(np.float32(1) / np.float32(255)))


@pytest.mark.parametrize('size', [(20, 36), (40, 72), (10, 18), (27, 49), (40, 18)])
def test_flip_is_an_exact_mirror(size):
    img, tgt = source(1)
    Hs, Ws = size
    oy, ox = min(2, Hs - 8), min(2, Ws - 16)
    x0, y0 = R.augment(img, tgt, [[Hs, Ws, oy, ox, 0, 0]] * 2, (8, 16), *IMAGENET)
    x1, y1 = R.augment(img, tgt, [[Hs, Ws, oy, ox, 1, 0]] * 2, (8, 16), *IMAGENET)
    assert np.array_equal(x1, x0[..., ::-1]) and np.array_equal(y1, y0[..., ::-1])


def test_constant_image_stays_constant_for_every_scale():
    img = np.full((1, 3, H, W), 137, np.uint8)
    sc, sh = R.constants(3, *IMAGENET)
    for Hs, Ws in [(20, 36), (40, 72), (10, 18), (27, 49), (40, 18), (13, 71)]:
        x, _ = R.augment(img, None, [[Hs, Ws, Hs - 8, Ws - 16, 0, 0]], (8, 16), *IMAGENET)
        want = 137.0 * sc + sh
        assert np.abs(x[0] - want[:, None, None]).max() <= 1e-13, (Hs, Ws)


@pytest.mark.parametrize('size', [(27, 49), (40, 72), (10, 18)])
def test_bilinear_stage_is_interpolate_align_corners_false(size):
    """Independent check of the half-pixel and edge convention: the whole resized plane, in grey levels, float64."""
    img, _ = source(2, B=1, C=1)
    Hs, Ws = size
    got = R.sample_bilinear(img[0, 0], np.arange(Hs), np.arange(Ws), Hs, Ws)
    want = F.interpolate(torch.from_numpy(img.astype(np.float64)), size=(Hs, Ws), mode='bilinear', align_corners=False)[0, 0].numpy()
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-9


@pytest.mark.parametrize('size', [(40, 72), (10, 18)])
def test_nearest_stage_is_interpolate_nearest_at_exact_ratios(size):
    _, tgt = source(3, B=1)
    Hs, Ws = size
    got = R.sample_nearest(tgt[0], np.arange(Hs), np.arange(Ws), Hs, Ws)
    want = F.interpolate(torch.from_numpy(tgt.astype(np.float64))[None], size=(Hs, Ws), mode='nearest')[0, 0].numpy()
    assert np.array_equal(got, want.astype(tgt.dtype))


def test_linear_taps_floor_and_clamp_at_the_edges():
    i0, i1, w = R.linear_taps(np.arange(72), 36, 72)            # x2: n = -36 at X = 0 -> x0 = -1 (clamped), weight 3/4
    assert (i0[0], i1[0], w[0]) == (0, 0, 0.75) and (i0[1], i1[1], w[1]) == (0, 1, 0.25)
    assert (i0[-1], i1[-1]) == (35, 35) and i0.min() == 0 and i1.max() == 35
    i0, i1, w = R.linear_taps(np.arange(36), 36, 36)
    assert np.array_equal(i0, np.arange(36)) and not w.any()
    assert np.array_equal(R.nearest_index(np.arange(18), 36, 18), 2 * np.arange(18))


def test_tolerance_is_the_derived_bound():
    out = np.zeros((1, 3, 1, 1))
    out[0, :, 0, 0] = (2.0, -1.0, 0.0)
    tol = R.image_tolerance(out, *IMAGENET)
    sc, _ = R.constants(3, *IMAGENET)
    want = 14 * 2.0 ** -24 * 255 * sc + 2.0 ** -24 * np.abs(out[0, :, 0, 0])
    assert np.allclose(tol[0, :, 0, 0], want, rtol=1e-15)
    assert 3.5e-6 < tol.max() < 4.0e-6                          # 1 / std = 4.46: 14 u / std, plus u |out|


def test_draw_bounds_determinism_and_checks():
    import torch_semantic_segmentation_amd as tssa
    aug = tssa.TrainAugment((512, 768), scale_range=(0.5, 2.0), flip_p=0.5)
    SH, SW = 1024, 2048
    rows = aug.draw(10000, (SH, SW), generator=torch.Generator().manual_seed(7))
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (10000, 6) and not rows.is_cuda
    Hs, Ws, oy, ox, flip, pad = rows.long().unbind(1)
    assert (Hs >= 512).all() and (Hs <= 2048).all() and (Ws >= 768).all() and (Ws <= 4096).all()
    assert (oy >= 0).all() and (oy <= Hs - 512).all() and (ox >= 0).all() and (ox <= Ws - 768).all()
    assert ((flip == 0) | (flip == 1)).all() and not pad.any()
    assert 0.45 < flip.double().mean() < 0.55                   # Bernoulli(0.5) over 10 000 draws: 10 sigma
    assert Hs.min() < 560 and Hs.max() > 2000                   # the whole scale range is drawn from
    assert (oy == Hs - 512).any() and (oy == 0).any()           # both ends of the origin range are reachable
    assert ((Ws - 2 * Hs).abs() <= 1).all()                     # one factor for both axes
    again = aug.draw(10000, (SH, SW), generator=torch.Generator().manual_seed(7))
    assert torch.equal(rows, again)
    assert not torch.equal(rows, aug.draw(10000, (SH, SW), generator=torch.Generator().manual_seed(8)))
    same = tssa.TrainAugment((512, 768), scale_range=(1, 1)).draw(64, (SH, SW), generator=torch.Generator().manual_seed(0))
    assert (same[:, 0] == SH).all() and (same[:, 1] == SW).all()
    assert tssa.TrainAugment((8, 16), flip_p=0.0).draw(100, (20, 36))[:, 4].sum() == 0
    assert tssa.TrainAugment((8, 16), flip_p=1.0).draw(100, (20, 36))[:, 4].sum() == 100
    with pytest.raises(ValueError, match='smaller than'):
        tssa.TrainAugment((512, 768), scale_range=(0.3, 2.0)).draw(4, (SH, SW))     # 307 x 614 < the crop
    with pytest.raises(ValueError):
        tssa.TrainAugment((512, 768), scale_range=(0.5, 2.0)).draw(4, (1000, 2048))  # 500 < 512
    with pytest.raises(ValueError):
        tssa.TrainAugment((512, 770))                                                # width not a multiple of 8
    with pytest.raises(ValueError):
        tssa.TrainAugment((512, 768), scale_range=(1.0, 5.0)).draw(1, (SH, SW))      # 10240 > 8192


def test_parameter_rows_are_validated_where_they_enter():
    from torch_semantic_segmentation_amd import ops
    good = torch.tensor([[20, 36, 12, 20, 1, 0]], dtype=torch.int32)
    ops.check_augment_params(good, (20, 36), (8, 16))
    for bad in ([20, 36, 13, 20, 0, 0], [20, 36, 0, 21, 0, 0], [7, 36, 0, 0, 0, 0], [20, 15, 0, 0, 0, 0], [20, 36, -1, 0, 0, 0],
                [20, 36, 0, 0, 2, 0], [9000, 36, 0, 0, 0, 0]):
        with pytest.raises(ValueError):
            ops.check_augment_params(torch.tensor([bad], dtype=torch.int32), (20, 36), (8, 16))
    with pytest.raises(ValueError):
        ops.check_augment_params(good.long(), (20, 36), (8, 16))


def test_augment_batch_has_no_cpu_fallback():
    import torch_semantic_segmentation_amd as tssa
    rows = torch.tensor([[20, 36, 0, 0, 0, 0]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match='HIP path only'):
        tssa.augment_batch(torch.zeros(1, 3, 20, 36, dtype=torch.uint8), torch.zeros(1, 20, 36, dtype=torch.uint8), rows, (8, 16))
    with pytest.raises(RuntimeError, match='HIP path only'):
        tssa.augment_batch(None, torch.zeros(1, 20, 36, dtype=torch.uint8), rows, (8, 16))
