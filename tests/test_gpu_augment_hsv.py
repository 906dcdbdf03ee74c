"""GPU: tss_augment_batch_u8_ex and tss_remap_labels_u8 (csrc/augment.hip) -- the train augmentation's gather kernel with
HueSaturationValue on the blended pixel and the label table in the same launch -- against the float64 restatement
tests/augment_hsv_ref.py (pinned by tests/test_augment_hsv_oracle.py): the image within the DERIVED elementwise bound
augment_hsv_ref.hsv_tolerance, labels equal.  Every test: B = 3, source 24 x 40, crop 16 x 32, geometry rows that upscale (37 x 61),
sit at the minimum scale (16 x 32) and at identity (24 x 40), flip 0 and 1, independent uniform random bytes per channel."""
import functools

import numpy as np
import pytest
import torch

from tests import augment_hsv_ref as HR
from tests import cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
B, H, W, CH, CW = 3, 24, 40, 16, 32
U = HR.U

# (Hs, Ws, oy, ox, flip, 0): upscale at its maximal / zero origin, the minimum scale (one origin), identity
GEOMETRY = ([[37, 61, 21, 29, 0, 0], [16, 32, 0, 0, 1, 0], [24, 40, 8, 8, 0, 0]],
            [[37, 61, 0, 0, 1, 0], [16, 32, 0, 0, 0, 0], [24, 40, 3, 5, 1, 0]])
# the limits of albumentations' defaults in all sign combinations, one extreme row per shift and sign, one interior row
COLOR = ([[1, a * 20, b * 30, c * 20] for a in (1, -1) for b in (1, -1) for c in (1, -1)]
         + [[1, 180, 0, 0], [1, -180, 0, 0], [1, 0, 255, 0], [1, 0, -255, 0], [1, 0, 0, 255], [1, 0, 0, -255], [1, 7, -13, 11]])
BATCHES = len(COLOR) // B                                        # 5 calls of 3 samples


def geometry(k):
    """Rows of call k: the two row sets in turn, rotated so that every colour row meets another geometry."""
    rows = GEOMETRY[k % 2]
    return rows[k % B:] + rows[:k % B]


@functools.lru_cache(maxsize=None)
def source(planted=False):
    """uint8 CHW image, labels (random bytes, 255 among them) and a non-injective table with entries equal to 255; seeded,
    shared, never modified.  planted: exactly grey and exactly black 2 x 2 texel patches inside the identity rows' crop windows."""
    rng = np.random.RandomState(77)
    img = rng.randint(0, 256, (B, 3, H, W)).astype(np.uint8)
    tgt = rng.randint(0, 256, (B, H, W)).astype(np.uint8)
    tgt[:, 0, :4] = 255
    lut = rng.randint(0, 19, 256).astype(np.uint8)
    lut[rng.rand(256) < 0.25] = 255
    lut[255] = 255
    if planted:
        img[:, :, 10:12, 12:14] = 77
        img[:, :, 12:14, 20:22] = 0
    for a in (img, tgt, lut):
        a.setflags(write=False)
    return img, tgt, lut


@functools.lru_cache(maxsize=None)
def blends(k, planted=False):
    g = HR.blend(source(planted)[0], geometry(k), (CH, CW))
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def reference(k, norm):
    """(float64 image, tolerance) of call k: colour rows COLOR[3k : 3k+3] on geometry(k)."""
    mean, std = IMAGENET if norm else (None, None)
    color = COLOR[B * k:B * k + B]
    return HR.normalize(HR.shift_blend(blends(k), color), mean, std), HR.hsv_tolerance(blends(k), color, mean, std)


def to_dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)      # a contiguous copy: the shared arrays are read-only


def device_image(img, hwc):
    return to_dev(img.transpose(0, 2, 3, 1) if hwc else img)


def rows_t(rows):
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize('hwc', [True, False])
def test_null_pointers_and_unapplied_rows_are_the_plain_entry_bit_for_bit(hwc):
    import ctypes
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import _native as N
    img, tgt, _ = source()
    dimg, dtgt = device_image(img, hwc), to_dev(tgt)
    m3, s3 = (ctypes.c_float * 3)(*IMAGENET[0]), (ctypes.c_float * 3)(*IMAGENET[1])
    for k in range(2):
        p = rows_t(geometry(k)).to(DEV)
        x0, y0 = tssa.augment_batch(dimg, dtgt, p, (CH, CW), *IMAGENET, image_hwc=hwc)
        x1 = torch.full_like(x0, float('nan'))
        y1 = torch.full_like(y0, -1)
        N.call('tss_augment_batch_u8_ex', N.ptr(dimg), int(hwc), m3, s3, N.ptr(x1), N.ptr(dtgt), N.ptr(y1), N.ptr(p), None, None,
               B, 3, H, W, CH, CW, N.stream())
        assert torch.equal(x1, x0) and torch.equal(y1, y0)
        off = rows_t([[0, 20, -30, 20], [0, -180, 255, -255], [0, 0, 0, 0]])
        x2, y2 = tssa.augment_batch(dimg, dtgt, p, (CH, CW), *IMAGENET, image_hwc=hwc, color=off)
        assert torch.equal(x2, x0) and torch.equal(y2, y0)
    # one channel: no colour rows there, the table alone goes through the same kernel
    grey1 = to_dev(img[:, :1].transpose(0, 2, 3, 1) if hwc else img[:, :1])
    x0, y0 = tssa.augment_batch(grey1, dtgt, rows_t(geometry(0)), (CH, CW), image_hwc=hwc)
    x1, y1 = tssa.augment_batch(grey1, dtgt, rows_t(geometry(0)), (CH, CW), image_hwc=hwc, label_map=list(range(256)))
    assert torch.equal(x1, x0) and torch.equal(y1, y0)


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('hwc', [True, False])
def test_shifted_batch_vs_restatement(hwc, norm):
    """Every pixel with D >= 8 and V >= 8 grey levels (float64 reference) within hsv_tolerance; the others (at most 5 %: a
    condition) finite and inside the range of a normalized grey level."""
    import torch_semantic_segmentation_amd as tssa
    img, tgt, _ = source()
    mean, std = IMAGENET if norm else (None, None)
    dimg = device_image(img, hwc)
    sc, sh = HR.R.constants(3, mean, std)
    lo, hi = np.minimum(sh, 255.0 * sc + sh), np.maximum(sh, 255.0 * sc + sh)
    slack = 2.0 * U * np.maximum(np.abs(lo), np.abs(hi))
    for k in range(BATCHES):
        want, tol = reference(k, norm)
        x, y = tssa.augment_batch(dimg, None, rows_t(geometry(k)), (CH, CW), mean, std, image_hwc=hwc, color=rows_t(COLOR[B * k:B * k + B]))
        assert y is None and x.dtype == torch.float32 and tuple(x.shape) == (B, 3, CH, CW)
        got = x.double().cpu().numpy()
        D, V = HR.conditioning(blends(k))
        keep = np.broadcast_to(((D >= 8) & (V >= 8))[:, None], got.shape)
        left = 1.0 - keep.mean()
        err = np.abs(got - want)
        worst = np.where(keep, err / tol, 0.0)
        print('call %d rows %s: left out %.2f %%, max error %.3e, bound there %.3e, max error / bound %.3f'
              % (k, COLOR[B * k:B * k + B], 100 * left, err[keep].max(), tol.flat[worst.argmax()], worst.max()))
        assert left <= 0.05
        assert (err[keep] <= tol[keep]).all(), (k, float(worst.max()))
        assert np.isfinite(got).all()
        assert (got >= (lo - slack)[None, :, None, None]).all() and (got <= (hi + slack)[None, :, None, None]).all()


@pytest.mark.parametrize('hwc', [True, False])
def test_zero_shift_round_trip(hwc):
    """apply = 1 with (0, 0, 0) against the plain output at ALL pixels, within the bound at ds = dv = 0 (no 1 / D, no 1 / V);
    exactly grey blends (planted grey and black texel patches) come back bit for bit."""
    import torch_semantic_segmentation_amd as tssa
    img, _, _ = source(planted=True)
    dimg = device_image(img, hwc)
    zero = [[1, 0, 0, 0]] * B
    for k in range(2):
        for mean, std in ((None, None), IMAGENET):
            grey = blends(k, planted=True)
            tol = HR.hsv_tolerance(grey, zero, mean, std)
            assert np.isfinite(tol).all()
            p = rows_t(geometry(k))
            plain, _ = tssa.augment_batch(dimg, None, p, (CH, CW), mean, std, image_hwc=hwc)
            x, _ = tssa.augment_batch(dimg, None, p, (CH, CW), mean, std, image_hwc=hwc, color=rows_t(zero))
            err = np.abs(x.double().cpu().numpy() - plain.double().cpu().numpy())
            print('rows %d: max round-trip error %.3e, bound there %.3e' % (k, err.max(), tol.flat[(err / tol).argmax()]))
            assert (err <= tol).all(), float((err / tol).max())
            assert (np.abs(x.double().cpu().numpy() - HR.normalize(grey, mean, std)) <= tol).all()
            D, V = HR.conditioning(grey)
            flat, black = (D == 0) & (V > 0), V == 0
            assert flat.sum() >= 4 and black.sum() >= 4
            same = torch.from_numpy(np.broadcast_to((D == 0)[:, None], err.shape).copy()).to(DEV)
            assert torch.equal(x[same], plain[same])


def test_label_table():
    import torch_semantic_segmentation_amd as tssa
    img, tgt, lut = source()
    assert len(set(lut.tolist())) < 256 and (lut == 255).sum() > 1
    dtgt, dlut = to_dev(tgt), to_dev(lut)
    for k in range(2):
        _, want = HR.augment(None, tgt, geometry(k), (CH, CW), label_map=lut)
        _, y = tssa.augment_batch(None, dtgt, rows_t(geometry(k)), (CH, CW), label_map=dlut)
        assert y.dtype == torch.int64 and np.array_equal(y.cpu().numpy(), want)
        x, y2 = tssa.augment_batch(device_image(img, True), dtgt, rows_t(geometry(k)), (CH, CW), image_hwc=True,
                                   color=rows_t(COLOR[:B]), label_map=lut.tolist())
        assert torch.equal(y2, y)
    rng = np.random.RandomState(5)
    for shape in ((2, 17, 23), (5, 41, 53)):                    # 782 = 97 x 8 + 6: one block and a tail; 10865: six blocks, tail 1
        raw = rng.randint(0, 256, shape).astype(np.uint8)
        raw.flat[-8:] = 255
        got = tssa.remap_labels(to_dev(raw), lut.tolist())
        assert got.dtype == torch.int64 and tuple(got.shape) == shape
        assert np.array_equal(got.cpu().numpy(), lut.astype(np.int64)[raw])
    out = torch.full((2, 17, 24), -1, dtype=torch.int64, device=DEV)
    raw = rng.randint(0, 256, (2, 17, 24)).astype(np.uint8)     # no tail
    assert tssa.remap_labels(to_dev(raw), dlut, out=out) is out
    assert np.array_equal(out.cpu().numpy(), lut.astype(np.int64)[raw])


def test_argument_errors():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import _native as N
    img, tgt, lut = source()
    dtgt = to_dev(tgt)
    one = to_dev(img[:, :1])
    p, c = rows_t(geometry(0)), rows_t(COLOR[:B])
    with pytest.raises(ValueError, match='3-channel'):
        tssa.augment_batch(one, dtgt, p, (CH, CW), color=c)
    with pytest.raises(ValueError, match='3-channel'):
        tssa.augment_batch(None, dtgt, p, (CH, CW), color=c)
    x = torch.full((B, 1, CH, CW), -7.0, dtype=torch.float32, device=DEV)
    dp, dc = p.to(DEV), c.to(DEV)
    rc = N.lib().tss_augment_batch_u8_ex(N.ptr(one), 0, None, None, N.ptr(x), None, None, N.ptr(dp), N.ptr(dc), None,
                                         B, 1, H, W, CH, CW, N.stream())
    assert rc == -2                                              # TSS_ERR_SHAPE: colour rows with one channel
    torch.cuda.synchronize()
    assert (x == -7.0).all()
    dimg = device_image(img, False)
    for bad in ([1, 181, 0, 0], [1, 0, -256, 0], [1, 0, 0, 256], [2, 0, 0, 0]):
        with pytest.raises(ValueError):
            tssa.augment_batch(dimg, dtgt, p, (CH, CW), color=rows_t([bad] * B))
    with pytest.raises(ValueError):
        tssa.augment_batch(dimg, dtgt, p, (CH, CW), color=c[:2])
    with pytest.raises(ValueError):
        tssa.augment_batch(dimg, dtgt, p, (CH, CW), color=c.long())
    with pytest.raises(ValueError):
        tssa.augment_batch(dimg, dtgt, p, (CH, CW), label_map=lut.tolist()[:255])
    with pytest.raises(ValueError):
        tssa.remap_labels(dtgt, list(range(257)))
    with pytest.raises(ValueError):
        tssa.remap_labels(dtgt.long(), lut.tolist())


def test_one_captured_graph_serves_every_draw():
    import torch_semantic_segmentation_amd as tssa
    img, tgt, lut = source()
    dimg, dtgt, dlut = device_image(img, True), to_dev(tgt), to_dev(lut)
    draws = [(rows_t(geometry(k)), rows_t(COLOR[B * k:B * k + B])) for k in (0, 3)]
    p, c = draws[0][0].to(DEV), draws[0][1].to(DEV)
    out = (torch.zeros((B, 3, CH, CW), dtype=torch.float32, device=DEV), torch.zeros((B, CH, CW), dtype=torch.int64, device=DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up outside the capture
        tssa.augment_batch(dimg, dtgt, p, (CH, CW), *IMAGENET, image_hwc=True, out=out, color=c, label_map=dlut)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tssa.augment_batch(dimg, dtgt, p, (CH, CW), *IMAGENET, image_hwc=True, out=out, color=c, label_map=dlut)
    seen = []
    for rows, color in draws:
        p.copy_(rows)
        c.copy_(color)
        graph.replay()
        torch.cuda.synchronize()
        ex, ey = tssa.augment_batch(dimg, dtgt, rows, (CH, CW), *IMAGENET, image_hwc=True, color=color, label_map=dlut)
        assert torch.equal(out[0], ex) and torch.equal(out[1], ey)
        seen.append(out[0].clone())
    assert not torch.equal(seen[0], seen[1])


@pytest.mark.parametrize('use_graph', [False, True])
def test_pipeline_draws_colour_rows_and_maps_labels(use_graph):
    """engine.HostBatchPipeline(augment=TrainAugment(hsv_p=1, label_map=...)): what the (captured) step read is augment_batch of
    the staged frame with the rows that draw() and then draw_color() give from an identically seeded generator."""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    g = torch.Generator().manual_seed(5)
    Bp, SH, SW, ch, cw = 2, 96, 160, 64, 128
    mean, std = IMAGENET
    lut = source()[2]
    batches = [(torch.randint(0, 256, (Bp, SH, SW, 3), generator=g, dtype=torch.uint8),
                torch.randint(0, 256, (Bp, SH, SW), generator=g, dtype=torch.uint8)) for _ in range(3)]
    aug = tssa.TrainAugment((ch, cw), scale_range=(0.8, 2.0), flip_p=0.5, mean=mean, std=std, hsv_p=1.0, label_map=lut.tolist())
    twin = torch.Generator().manual_seed(11)
    rows = []
    for _ in batches:
        geo = aug.draw(Bp, (SH, SW), generator=twin)
        rows.append((geo, aug.draw_color(Bp, generator=twin)))
    assert all(bool(c[:, 0].all()) for _, c in rows) and len({tuple(c.flatten().tolist()) for _, c in rows}) == 3
    torch.manual_seed(0)
    m = cases.product_model('fastscnn').to(DEV)
    cases.zero_dropout(m)
    tr = E.Trainer(m, E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5), tssa.CrossEntropyLoss(ignore_index=255), use_graph=use_graph)
    ex = torch.empty((Bp, 3, ch, cw), dtype=torch.float32)
    ey = torch.empty((Bp, ch, cw), dtype=torch.int64)
    with pytest.raises(ValueError, match='3-channel'):
        E.HostBatchPipeline(tr, ex[:, :1], ey, wire='u8', image_hwc=True, device=DEV, augment=aug, source_size=(SH, SW))
    pipe = E.HostBatchPipeline(tr, ex, ey, wire='u8', image_hwc=True, device=DEV, augment=aug, source_size=(SH, SW),
                               generator=torch.Generator().manual_seed(11))
    assert len(pipe.color) == 2 and tuple(pipe.color[0].shape) == (Bp, 4) and pipe.color[0].dtype == torch.int32
    losses = []
    for k, (img, tgt) in enumerate(batches):
        pipe.put(img.pin_memory(), tgt.pin_memory())
        losses.append(pipe.step().item())
        slot = k % 2
        assert torch.equal(pipe.params[slot].cpu(), rows[k][0]) and torch.equal(pipe.color[slot].cpu(), rows[k][1])
        wx, wy = tssa.augment_batch(img.to(DEV), tgt.to(DEV), rows[k][0], (ch, cw), mean, std, image_hwc=True, color=rows[k][1],
                                    label_map=lut.tolist())
        assert torch.equal(pipe.decoded[0], wx) and torch.equal(pipe.decoded[1], wy)
        assert set(np.unique(wy.cpu().numpy()).tolist()) <= set(range(19)) | {255}
    assert all(np.isfinite(v) for v in losses)
    pipe.close()
    assert pipe.color == [] and pipe._lut is None
