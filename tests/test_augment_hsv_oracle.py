"""CPU (no GPU): pins tests/augment_hsv_ref.py, the restatement the GPU tests of tss_augment_batch_u8_ex compare against, by known
values that depend on no kernel; and the host side of the feature (TrainAugment.draw_color, the colour-row and table checks)."""
import numpy as np
import pytest
import torch

from tests import augment_hsv_ref as HR

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def random_blends(seed=0, n=4096):
    """float64 [3, n] blends as the kernel meets them: convex combinations of four uint8 texels per channel."""
    rng = np.random.RandomState(seed)
    texels = rng.randint(0, 256, (4, 3, n)).astype(np.float64)
    wx, wy = rng.rand(n), rng.rand(n)
    w = np.stack([(1 - wx) * (1 - wy), wx * (1 - wy), (1 - wx) * wy, wx * wy])
    return (texels * w[:, None, :]).sum(0)


def shift(rgb, dh=0, ds=0, dv=0):
    return np.stack(HR.hsv_shift(rgb[0], rgb[1], rgb[2], dh, ds, dv))


def pixel(r, g, b, **kw):
    return shift(np.array([[r], [g], [b]], dtype=np.float64), **kw)[:, 0].tolist()


def test_zero_shift_is_the_identity():
    rgb = random_blends()
    assert np.abs(shift(rgb) - rgb).max() < 1e-9
    bytes_ = np.random.RandomState(1).randint(0, 256, (3, 4096)).astype(np.float64)      # ties and exact sector boundaries
    assert np.abs(shift(bytes_) - bytes_).max() < 1e-9


def test_half_turns_of_the_hue_are_the_identity():
    rgb = random_blends(2)
    for ds, dv in ((0, 0), (30, -20), (-30, 20)):
        base = shift(rgb, 0, ds, dv)
        assert np.abs(shift(rgb, 180, ds, dv) - base).max() < 1e-9
        assert np.abs(shift(rgb, -180, ds, dv) - base).max() < 1e-9


def test_primaries_rotate_into_each_other():
    assert pixel(255, 0, 0, dh=60) == [0, 255, 0]
    assert pixel(255, 0, 0, dh=120) == [0, 0, 255]
    assert pixel(0, 255, 0, dh=60) == [0, 0, 255]
    assert pixel(0, 0, 255, dh=60) == [255, 0, 0]                # 120 + 60 wraps to 0
    assert pixel(255, 0, 0, dh=-60) == [0, 0, 255]               # 0 - 60 wraps to 120
    assert pixel(255, 0, 0, dh=30) == [255, 255, 0]              # yellow: the end of sector 0


def test_saturation_and_value_shifts():
    rgb = random_blends(3)
    V = rgb.max(0)
    grey = shift(rgb, ds=-255)
    assert np.array_equal(grey, np.stack([V, V, V]))             # S' = 0: p = q = t = V exactly
    assert np.abs(shift(rgb, dv=255).max(0) - 255.0).max() == 0  # V' saturates at 255
    assert np.abs(shift(rgb, dv=-255)).max() == 0                # V' = 0: black
    got = shift(rgb, dv=20)
    assert np.abs(got.max(0) - np.minimum(V + 20, 255)).max() < 1e-9
    # a grey pixel has hue 0: ds = +51 (S' = 51 = 0.2 * 255) tints it red, (V, 0.8 V, 0.8 V)
    for v in (1.0, 100.0, 137.25, 255.0):
        assert np.allclose(pixel(v, v, v, ds=51), [v, 0.8 * v, 0.8 * v], rtol=1e-15, atol=0)
    assert pixel(90.5, 90.5, 90.5, dh=17, dv=0) == [90.5, 90.5, 90.5]        # hue alone leaves grey alone, exactly
    for dv in (0, -1, -255):                                     # black stays black (S = 0 by definition at V = 0)
        assert pixel(0, 0, 0, dh=20, ds=30, dv=dv) == [0, 0, 0]
    assert pixel(0, 0, 0, dv=10) == [10, 10, 10]


def test_apply_flag_and_the_whole_restatement():
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, (2, 3, 12, 20)).astype(np.uint8)
    tgt = rng.randint(0, 256, (2, 12, 20)).astype(np.uint8)
    rows = [[18, 31, 3, 5, 1, 0], [12, 20, 0, 0, 0, 0]]
    lut = rng.randint(0, 20, 256)
    lut[rng.rand(256) < 0.3] = 255
    plain_x, plain_y = HR.R.augment(img, tgt, rows, (8, 16), *IMAGENET)
    x, y = HR.augment(img, tgt, rows, (8, 16), *IMAGENET, color=[[0, 20, 30, -20], [0, -180, 255, 255]], label_map=lut)
    assert np.array_equal(x, plain_x)                            # apply = 0 ignores the shifts
    assert np.array_equal(y, lut[plain_y]) and y.dtype == np.int64
    x, y = HR.augment(img, tgt, rows, (8, 16), *IMAGENET, color=[[1, 0, 0, 0], [1, 20, 30, -20]])
    assert np.abs(x[0] - plain_x[0]).max() < 1e-9 / 0.224 and np.abs(x[1] - plain_x[1]).max() > 0.05
    assert np.array_equal(y, plain_y)
    x, _ = HR.augment(img.transpose(0, 2, 3, 1), None, rows, (8, 16), color=[[1, 7, 8, 9], [1, 20, 30, -20]], image_hwc=True)
    x2, _ = HR.augment(img, None, rows, (8, 16), color=[[1, 7, 8, 9], [1, 20, 30, -20]])
    assert np.array_equal(x, x2)


def test_tolerance_is_the_derived_bound_and_holds_for_a_float32_evaluation():
    """The bound's value at one hand-computed pixel, its specialisations, and a float32 evaluation of the same formula from the
    same (float32-rounded) blends inside it everywhere (that evaluation differs from float64 by about 1e-4 grey levels)."""
    u, e = 2.0 ** -24, 13 * 2.0 ** -24 * 255
    grey = np.zeros((1, 3, 1, 1))
    grey[0, :, 0, 0] = (200.0, 100.0, 50.0)                      # V = 200, m = 50, D = 150, S = 191.25
    tol = HR.hsv_tolerance(grey, [[1, 20, 30, 20]])[0, :, 0, 0]
    V2, S2 = 220.0, 221.25
    d_s = ((255 / 200) * (1 + 50 / 200) * e + 3 * u * 191.25 + 510 * u) / 255 + u
    d_h = 2 * e / 150 + 40 * u
    d_grey = e + 510 * u + V2 * (S2 / 255 * d_h + d_s) + 4 * u * V2
    out = np.array(HR.hsv_shift(200.0, 100.0, 50.0, 20, 30, 20)) / 255
    sc = float(np.float32(1) / np.float32(255))
    assert np.allclose(tol, sc * (d_grey + 255 * u) + u * out, rtol=1e-12)
    assert 60 * u < tol.max() < 130 * u                          # a few dozen u 255 grey levels (here / 255), not percent-level
    # apply = 0: augment_ref.image_tolerance itself
    assert np.array_equal(HR.hsv_tolerance(grey, [[0, 20, 30, 20]]), HR.R.image_tolerance(grey * sc))
    # ds = dv = 0: finite at exact grey and exact black, no 1 / D and no 1 / V
    flat = np.zeros((1, 3, 1, 3))
    flat[0, :, 0, 0], flat[0, :, 0, 1], flat[0, :, 0, 2] = 77.0, 0.0, (1e-3, 0.0, 0.0)
    assert HR.hsv_tolerance(flat, [[1, 0, 0, 0]]).max() < 80 * u
    assert np.isinf(HR.hsv_tolerance(flat, [[1, 0, 5, 0]])[0, :, 0, 0]).all()        # grey with ds > 0: discontinuous
    assert np.isinf(HR.hsv_tolerance(flat, [[1, 0, 0, 5]])[0, :, 0, 1]).all()        # black with dv > 0
    rgb = random_blends(5, 20000)
    D, V = rgb.max(0) - rgb.min(0), rgb.max(0)
    keep = (D >= 8) & (V >= 8)
    assert keep.mean() > 0.95
    for dh, ds, dv in [(20, 30, 20), (-20, -30, -20), (20, -30, 20), (-20, 30, -20), (180, 0, 0), (0, 255, 0), (0, 0, 255), (0, -255, -255)]:
        want = shift(rgb, dh, ds, dv)
        got = np.stack(HR.hsv_shift(*rgb.astype(np.float32), dh, ds, dv, dtype=np.float32))
        assert got.dtype == np.float32
        tol = HR.hsv_tolerance(rgb.reshape(1, 3, 1, -1), [[1, dh, ds, dv]])[0, :, 0] / sc        # in grey levels
        err = np.abs(got - want)
        assert (err[:, keep] <= tol[:, keep]).all(), (dh, ds, dv, float((err[:, keep] / tol[:, keep]).max()))


def test_draw_color_bounds_determinism_and_unchanged_geometry_rows():
    import torch_semantic_segmentation_amd as tssa
    aug = tssa.TrainAugment((512, 768), hsv_p=0.5)
    rows = aug.draw_color(10000, generator=torch.Generator().manual_seed(7))
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (10000, 4) and not rows.is_cuda
    apply, dh, ds, dv = rows.long().unbind(1)
    assert ((apply == 0) | (apply == 1)).all() and 0.45 < apply.double().mean() < 0.55
    for col, lim in ((dh, 20), (ds, 30), (dv, 20)):              # albumentations' default limits, both ends reached
        assert col.min() == -lim and col.max() == lim and abs(col.double().mean()) < 1.0
    assert torch.equal(rows, aug.draw_color(10000, generator=torch.Generator().manual_seed(7)))
    assert not torch.equal(rows, aug.draw_color(10000, generator=torch.Generator().manual_seed(8)))
    off = tssa.TrainAugment((512, 768))
    assert off.hsv_p == 0.0 and off.label_map is None and off.draw_color(1000)[:, 0].sum() == 0
    assert tssa.TrainAugment((8, 16), hsv_p=1.0).draw_color(100)[:, 0].sum() == 100
    wide = tssa.TrainAugment((8, 16), hsv_p=1.0, hue_shift_limit=180, sat_shift_limit=255, val_shift_limit=0).draw_color(5000)
    assert wide[:, 1].abs().max() > 170 and wide[:, 2].abs().max() > 240 and not wide[:, 3].any()
    # draw() is what it was: the same rows for the same seed whatever the new arguments, and as the first draw of a pair
    old = tssa.TrainAugment((512, 768), scale_range=(0.5, 2.0), flip_p=0.5).draw(64, (1024, 2048), generator=torch.Generator().manual_seed(3))
    # recorded from the commit before draw_color existed
    assert old[:3].tolist() == [[564, 1129, 15, 279, 1, 0], [1672, 3344, 706, 512, 1, 0], [1134, 2268, 485, 279, 0, 0]]
    g = torch.Generator().manual_seed(3)
    new = tssa.TrainAugment((512, 768), scale_range=(0.5, 2.0), flip_p=0.5, hsv_p=0.5, label_map=list(range(256)))
    assert torch.equal(new.draw(64, (1024, 2048), generator=g), old)
    first = new.draw_color(64, generator=g)
    g2 = torch.Generator().manual_seed(3)
    new.draw(64, (1024, 2048), generator=g2)
    assert torch.equal(new.draw_color(64, generator=g2), first)
    with pytest.raises(ValueError):
        tssa.TrainAugment((8, 16), hsv_p=1.5)
    with pytest.raises(ValueError):
        tssa.TrainAugment((8, 16), hue_shift_limit=181)
    with pytest.raises(ValueError):
        tssa.TrainAugment((8, 16), label_map=list(range(255)))


def test_colour_rows_and_tables_are_validated_where_they_enter():
    from torch_semantic_segmentation_amd import ops
    ops.check_color_params(torch.tensor([[1, 180, -255, 255], [0, -180, 255, -255]], dtype=torch.int32))
    for bad in ([2, 0, 0, 0], [-1, 0, 0, 0], [1, 181, 0, 0], [1, -181, 0, 0], [1, 0, 256, 0], [0, 0, 0, -256]):
        with pytest.raises(ValueError):
            ops.check_color_params(torch.tensor([bad], dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.check_color_params(torch.zeros((2, 4), dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.check_color_params(torch.zeros((2, 6), dtype=torch.int32))
    lut = ops.label_lut([255] * 7 + list(range(249)))
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256,) and lut[:8].tolist() == [255] * 7 + [0]
    assert torch.equal(ops.label_lut(np.arange(256)), torch.arange(256, dtype=torch.uint8))
    assert ops.label_lut(lut) is lut
    for bad in (list(range(255)), [256] + [0] * 255, [-1] + [0] * 255, torch.zeros(256), torch.zeros((2, 128), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ops.label_lut(bad)
    with pytest.raises(RuntimeError, match='HIP path only'):
        ops.remap_labels(torch.zeros((1, 4, 4), dtype=torch.uint8), list(range(256)))
