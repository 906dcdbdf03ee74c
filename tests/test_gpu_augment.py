"""GPU: tss_augment_batch_u8 (csrc/augment.hip) -- random scale, crop, flip, Normalize and ToTensor of a uint8 batch in one gather
kernel -- against the float64 restatement tests/augment_ref.py (pinned by tests/test_augment_oracle.py): the image within the
DERIVED elementwise bound augment_ref.image_tolerance (14 float32 roundings), the labels equal.  Parameter rows are written by hand
so that the edges are hit.  Then the kernel at the top of the (captured) train step, through engine.HostBatchPipeline."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import augment_ref as R
from tests import cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
H, W, CH, CW = 20, 36, 8, 16

# name -> rows (Hs, Ws, oy, ox, flip, 0), one sample each
GEOMETRY = {
    'identity': [[20, 36, 0, 0, 0, 0], [20, 36, 12, 20, 0, 0]],            # zero weights, maximal origin
    'x2': [[40, 72, 0, 0, 0, 0], [40, 72, 32, 56, 0, 0]],                  # n < 0 and the floor at top / left, clamp at bottom / right
    'half': [[10, 18, 2, 2, 0, 0]],                                        # texel skipping, nearest stride
    'non_dyadic': [[27, 49, 3, 5, 0, 0]],                                  # inexact weights, remainder arithmetic
    'anisotropic': [[40, 18, 30, 2, 0, 0], [10, 72, 1, 50, 1, 0]],         # horizontal and vertical paths independent
    'per_sample': [[20, 36, 5, 7, 0, 0], [40, 72, 32, 56, 1, 0], [27, 49, 3, 5, 1, 0]],   # per-sample rows, flip with a crop origin
}
VARIANTS = [(hwc, C, norm) for hwc in (True, False) for C in (3, 1) for norm in (False, True)]


@functools.lru_cache(maxsize=None)
def source(B, C, h=H, w=W):
    """uint8 CHW image and labels (all of 0..18 and 255 present), seeded; shared by the tests, never modified."""
    rng = np.random.RandomState(100 * B + C)
    img = rng.randint(0, 256, (B, C, h, w)).astype(np.uint8)
    tgt = rng.randint(0, 19, (B, h, w)).astype(np.uint8)
    tgt[rng.rand(B, h, w) < 0.1] = 255
    tgt[:, 0, :20] = np.arange(20)
    tgt[:, 0, 19] = 255
    img.setflags(write=False)
    tgt.setflags(write=False)
    return img, tgt


@functools.lru_cache(maxsize=None)
def reference(name, C, norm):
    rows = GEOMETRY[name]
    img, tgt = source(len(rows), C)
    mean, std = IMAGENET if norm else (None, None)
    return R.augment(img, tgt, rows, (CH, CW), mean, std)


def check(got_x, got_y, want_x, want_y, mean, std, what):
    if want_x is not None:
        err = np.abs(got_x.double().cpu().numpy() - want_x)
        tol = R.image_tolerance(want_x, mean, std)
        print('%s: max image error %.3e, bound at that element %.3e' % (what, err.max(), tol.flat[err.argmax()]))
        assert got_x.dtype == torch.float32 and (err <= tol).all(), (what, float((err / tol).max()))
    if want_y is not None:
        assert got_y.dtype == torch.int64 and np.array_equal(got_y.cpu().numpy(), want_y), what


def to_dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)  # a contiguous copy: the shared arrays are read-only


def device_image(img, hwc):
    return to_dev(img.transpose(0, 2, 3, 1) if hwc else img)


@pytest.mark.parametrize('hwc,C,norm', VARIANTS)
@pytest.mark.parametrize('name', sorted(GEOMETRY))
def test_augment_batch_vs_restatement(name, hwc, C, norm):
    import torch_semantic_segmentation_amd as tssa
    rows = GEOMETRY[name]
    img, tgt = source(len(rows), C)
    mean, std = IMAGENET if norm else (None, None)
    if C == 1 and norm:
        mean, std = mean[:1], std[:1]
    want_x, want_y = reference(name, C, norm)
    x, y = tssa.augment_batch(device_image(img, hwc), to_dev(tgt), torch.tensor(rows, dtype=torch.int32),
                              (CH, CW), mean=mean, std=std, image_hwc=hwc)
    assert tuple(x.shape) == (len(rows), C, CH, CW) and tuple(y.shape) == (len(rows), CH, CW)
    check(x, y, want_x, want_y, mean, std, (name, hwc, C, norm))
    got_labels = set(np.unique(y.cpu().numpy()).tolist())
    assert got_labels <= set(np.unique(tgt).tolist())                       # pass-through: no label is invented


def test_identity_is_the_decode_entry_bit_for_bit():
    """At Hs = H, Ws = W every weight is 0: the crop equals tss_decode_batch_u8 of the same region exactly."""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import _native as N
    img, tgt = source(2, 3)
    mean, std = IMAGENET
    x, y = tssa.augment_batch(device_image(img, False), to_dev(tgt),
                              torch.tensor(GEOMETRY['identity'], dtype=torch.int32), (CH, CW), mean=mean, std=std)
    crop = np.stack([img[0, :, 0:8, 0:16], img[1, :, 12:20, 20:36]])
    full = torch.empty((2, 3, CH, CW), dtype=torch.float32, device=DEV)
    N.call('tss_decode_batch_u8', N.ptr(to_dev(crop)), 0, (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std),
           N.ptr(full), None, None, 2, 3, CH * CW, N.stream())
    assert torch.equal(x, full)
    assert torch.equal(y.cpu(), torch.from_numpy(np.stack([tgt[0, 0:8, 0:16], tgt[1, 12:20, 20:36]]).astype(np.int64)))


def test_labels_pass_through_unchanged():
    """All of 0..18 and 255 reach the output at identity scale (row 0 of the source holds them); nothing else appears."""
    import torch_semantic_segmentation_amd as tssa
    _, tgt = source(1, 3)
    wide = np.ascontiguousarray(tgt[:, :, :32])
    _, y = tssa.augment_batch(None, to_dev(wide), torch.tensor([[20, 32, 0, 0, 1, 0]], dtype=torch.int32), (8, 32))
    assert set(np.unique(y.cpu().numpy()).tolist()) >= set(range(19)) | {255}
    assert np.array_equal(y.cpu().numpy()[0], wide[0, :8, ::-1].astype(np.int64))


@pytest.mark.parametrize('half', ['image', 'target'])
def test_optional_halves_through_the_c_entry(half):
    """image = NULL / target = NULL: the other half is written, the missing one's output is not touched."""
    from torch_semantic_segmentation_amd import _native as N
    rows = GEOMETRY['per_sample']
    img, tgt = source(3, 3)
    want_x, want_y = reference('per_sample', 3, True)
    mean, std = IMAGENET
    x = torch.full((3, 3, CH, CW), -7.0, dtype=torch.float32, device=DEV)
    y = torch.full((3, CH, CW), -7, dtype=torch.int64, device=DEV)
    p = torch.tensor(rows, dtype=torch.int32).to(DEV)
    dimg, dtgt = device_image(img, True), to_dev(tgt)
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    if half == 'image':
        N.call('tss_augment_batch_u8', N.ptr(dimg), 1, m3, s3, N.ptr(x), None, None, N.ptr(p), 3, 3, H, W, CH, CW, N.stream())
        check(x, None, want_x, None, mean, std, half)
        assert (y == -7).all()
    else:
        N.call('tss_augment_batch_u8', None, 1, m3, s3, None, N.ptr(dtgt), N.ptr(y), N.ptr(p), 3, 3, H, W, CH, CW, N.stream())
        check(None, y, None, want_y, mean, std, half)
        assert (x == -7.0).all()


@pytest.mark.parametrize('hwc', [True, False])
def test_many_blocks_and_a_ragged_last_block(hwc):
    """Source 70 x 530 -> crop 64 x 520 of a 93 x 707 scaled image, B = 2: 8320 thread groups = 32 full blocks and one of 128
    threads (the grid covers every group; the kernel has no stride loop)."""
    import torch_semantic_segmentation_amd as tssa
    img, tgt = source(2, 3, 70, 530)
    rows = [[93, 707, 29, 187, 0, 0], [93, 707, 0, 0, 1, 0]]
    mean, std = IMAGENET
    want_x, want_y = R.augment(img, tgt, rows, (64, 520), mean, std)
    x = torch.full((2, 3, 64, 520), float('nan'), dtype=torch.float32, device=DEV)
    y = torch.full((2, 64, 520), -1, dtype=torch.int64, device=DEV)
    rx, ry = tssa.augment_batch(device_image(img, hwc), to_dev(tgt), torch.tensor(rows, dtype=torch.int32),
                                (64, 520), mean=mean, std=std, image_hwc=hwc, out=(x, y))
    assert rx is x and ry is y
    check(x, y, want_x, want_y, mean, std, ('large', hwc))


def test_argument_errors_launch_nothing():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import _native as N
    lib = N.lib()
    img, tgt = source(1, 3)
    dimg, dtgt = device_image(img, False), to_dev(tgt)
    p = torch.tensor([[20, 36, 0, 0, 0, 0]], dtype=torch.int32).to(DEV)
    x = torch.full((3 * CH * CW + 8,), -7.0, dtype=torch.float32, device=DEV)
    y = torch.full((CH * CW + 8,), -7, dtype=torch.int64, device=DEV)

    def rc(image_out, target_out, C, cw):
        return lib.tss_augment_batch_u8(N.ptr(dimg), 0, None, None, image_out, N.ptr(dtgt), target_out, N.ptr(p), 1, C, H, W, CH, cw,
                                        N.stream())
    assert rc(x.data_ptr(), y.data_ptr(), 3, 12) == -2                      # TSS_ERR_SHAPE: crop width not a multiple of 8
    assert rc(x.data_ptr(), y.data_ptr(), 4, CW) == -2                      # TSS_ERR_SHAPE: four channels
    assert rc(x.data_ptr(), y.data_ptr(), 3, 8200) == -2                    # TSS_ERR_SHAPE: past 8192
    assert rc(x[1:].data_ptr(), y.data_ptr(), 3, CW) == -3                  # TSS_ERR_ALIGN: image_out + 4 bytes
    assert rc(x.data_ptr(), y[1:].data_ptr(), 3, CW) == -3                  # TSS_ERR_ALIGN: target_out + 8 bytes
    torch.cuda.synchronize()
    assert (x == -7.0).all() and (y == -7).all()
    assert rc(x.data_ptr(), y.data_ptr(), 3, CW) == 0                       # the same call with good arguments does launch
    assert not (x[:3 * CH * CW] == -7.0).any() and not (y[:CH * CW] == -7).any()
    rows = torch.tensor([[20, 36, 0, 0, 0, 0]], dtype=torch.int32)
    with pytest.raises(ValueError):
        tssa.augment_batch(dimg, dtgt, rows, (CH, 12))
    with pytest.raises(ValueError):
        tssa.augment_batch(torch.zeros((1, 4, H, W), dtype=torch.uint8, device=DEV), dtgt, rows, (CH, CW))
    with pytest.raises(ValueError):
        tssa.augment_batch(dimg, dtgt, rows, (CH, CW), out=(x[1:1 + 3 * CH * CW].view(1, 3, CH, CW), None))
    with pytest.raises(ValueError):                                         # a CPU row that leaves the scaled image
        tssa.augment_batch(dimg, dtgt, torch.tensor([[20, 36, 13, 0, 0, 0]], dtype=torch.int32), (CH, CW))
    with pytest.raises(ValueError):
        tssa.augment_batch(dimg, dtgt, rows.long(), (CH, CW))


@pytest.mark.parametrize('use_graph', [False, True])
def test_pipeline_augments_at_the_top_of_the_step(use_graph):
    """engine.HostBatchPipeline(wire='u8', augment=...): the loader ships full uint8 frames, put() draws the rows, and the
    (captured) step augments on the device.  Twin: the same rows redrawn from the same seed on the CPU, the restatement's output
    (cast to float32) through the plain f32 wire.  Loss tolerances as tests/test_gpu_models.py's u8-vs-f32 comparison, for the
    same reason: inputs a few float32 roundings apart, amplified by train-mode steps (first step tight, later steps loose)."""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    g = torch.Generator().manual_seed(5)
    B, SH, SW, ch, cw = 2, 96, 160, 64, 128
    mean, std = IMAGENET
    batches = []
    for _ in range(4):
        img = torch.randint(0, 256, (B, SH, SW, 3), generator=g, dtype=torch.uint8)
        tgt = torch.randint(0, 19, (B, SH, SW), generator=g, dtype=torch.uint8)
        tgt[torch.rand(B, SH, SW, generator=g) < 0.05] = 255
        batches.append((img, tgt))
    aug = tssa.TrainAugment((ch, cw), scale_range=(0.8, 2.0), flip_p=0.5, mean=mean, std=std)
    gen = torch.Generator().manual_seed(11)
    rows = [aug.draw(B, (SH, SW), generator=gen) for _ in range(6)]
    assert len({tuple(r.flatten().tolist()) for r in rows}) == 6            # every step has rows of its own
    refs = [R.augment(i.numpy(), t.numpy(), r.numpy(), (ch, cw), mean, std, image_hwc=True) for (i, t), r in zip(batches, rows)]

    def make():
        torch.manual_seed(0)
        m = cases.product_model('fastscnn').to(DEV)
        cases.zero_dropout(m)
        opt = E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
        return E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=255), use_graph=use_graph)

    def run(pipe, feed, after_step=None):
        got = []
        pipe.put(*feed[0])
        for k, nxt in enumerate(feed[1:]):
            pipe.put(*nxt)
            got.append(pipe.step().item())
            if after_step:
                after_step(k)
        got.append(pipe.step().item())
        if after_step:
            after_step(len(feed) - 1)
        return got

    ex = torch.from_numpy(refs[0][0]).float()
    ey = torch.from_numpy(refs[0][1])
    twin = E.HostBatchPipeline(make(), ex, ey, wire='f32', device=DEV)
    want = run(twin, [(torch.from_numpy(x).float().pin_memory(), torch.from_numpy(y).pin_memory()) for x, y in refs])

    tr = make()
    with pytest.raises(ValueError):
        E.HostBatchPipeline(tr, ex, ey, wire='f32', augment=aug, source_size=(SH, SW), device=DEV)
    with pytest.raises(ValueError):                                         # 0.5 x 96 < 64: RandomCrop would raise
        E.HostBatchPipeline(tr, ex, ey, wire='u8', image_hwc=True, device=DEV, source_size=(SH, SW),
                            augment=tssa.TrainAugment((ch, cw), scale_range=(0.5, 2.0)))
    pipe = E.HostBatchPipeline(tr, ex, ey, wire='u8', image_hwc=True, device=DEV, augment=aug, source_size=(SH, SW),
                               generator=torch.Generator().manual_seed(11))
    assert tuple(pipe.stage[0][0].shape) == (B, SH, SW, 3) and tuple(pipe.decoded[0].shape) == (B, 3, ch, cw)
    decoded = []
    got = run(pipe, [(i.pin_memory(), t.pin_memory()) for i, t in batches],
              after_step=lambda k: decoded.append((pipe.decoded[0].clone(), pipe.decoded[1].clone())))
    for k, ((dx, dy), (rx, ry)) in enumerate(zip(decoded, refs)):           # what the step read, against the restatement
        check(dx, dy, rx, ry, mean, std, ('pipeline step', k))
    print('losses', got, want)
    assert abs(got[0] / want[0] - 1) < 2e-5 and np.allclose(got, want, rtol=3e-3), (got, want)
    # the SAME batch twice more, with the next two row sets of the generator: the (captured) step re-reads the device rows
    pipe.put(batches[0][0].pin_memory(), batches[0][1].pin_memory())
    pipe.step()
    first = pipe.decoded[0].clone()
    pipe.put(batches[0][0].pin_memory(), batches[0][1].pin_memory())
    pipe.step()
    second = pipe.decoded[0].clone()
    assert not torch.equal(first, second)
    for k, got_x in ((4, first), (5, second)):
        rx, _ = R.augment(batches[0][0].numpy(), None, rows[k].numpy(), (ch, cw), mean, std, image_hwc=True)
        check(got_x, None, rx, None, mean, std, ('same batch, rows', k))
    pipe.close()
