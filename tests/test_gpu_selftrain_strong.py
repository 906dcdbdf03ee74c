"""tssa.SelfTraining(strong=tssa.StrongAugment(...)), set up as tests/test_gpu_selftrain_trainer.py (FastSCNN in bf16 on
synthetic_batch(2, 64, 128) plus a second seeded batch as the unlabelled frames): three captured steps equal three eager steps on
bits -- losses, parameters, the average, x_all, y_all -- with ClassMix + strong and with mix=None + strong (FixMatch's pair); after a
step the unlabelled half of x_all equals, on bits, tssa.strong_augment of the mixed half that tests/selftrain_ref.py builds, with the
rows in last_rows; y_all's half is the mix's target; the labelled half is untouched."""
import functools

import numpy as np
import pytest
import torch

from tests import selftrain_ref as R, strongaug_ref as SR
from tests import test_gpu_selftrain_trainer as T

pytestmark = pytest.mark.gpu
DEV = T.DEV
MEAN, STD = SR.IMAGENET_MEAN, SR.IMAGENET_STD


def run(use_graph, mix, steps=3):
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    x, y, xu = T.batches()
    m = T.student()
    opt = E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
    ema = E.ModelEMA(m, opt, T.DECAY)
    teacher = T.student()
    tr = E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=T.IGN), use_graph=use_graph, ema=ema)
    strong = tssa.StrongAugment(mean=MEAN, std=STD, color_p=0.9, blur_p=0.9, sigma=(0.5, 2.5))
    st = tssa.SelfTraining(tr, teacher, 19, threshold=0.5, mix=mix, seed=11, strong=strong)
    st.set_threshold(T.median_confidence())
    losses, rows = [], []
    for _ in range(steps):
        losses.append(st.step(x, y, xu).clone())
        rows.append(st.last_rows)
    assert bool(tr._graphs) == use_graph
    return {'losses': torch.stack(losses).cpu(), 'm': m, 'ema': ema, 'st': st, 'teacher': teacher, 'rows': rows}


@functools.lru_cache(maxsize=None)
def eager(mix):
    return run(False, mix)


@pytest.mark.parametrize('mix', ['classmix', None])
def test_three_steps_captured_equal_eager(mix):
    e, g = eager(mix), run(True, mix)
    print('selftrain strong', mix, 'losses', e['losses'].tolist(), 'radii', [r[4].tolist() for r in e['rows']])
    assert bool(torch.isfinite(e['losses']).all()) and float(e['losses'][1]) != float(e['losses'][0])
    assert torch.equal(e['losses'], g['losses'])
    T.same_bits(T.snapshot(e['m']), T.snapshot(g['m']))
    T.same_bits(T.snapshot(e['ema'].module), T.snapshot(g['ema'].module))
    assert torch.equal(e['st'].x_all, g['st'].x_all) and torch.equal(e['st'].y_all, g['st'].y_all)
    for a, b in zip(e['rows'], g['rows']):
        assert len(a) == 6 and all(np.array_equal(p, q) for p, q in zip(a, b))
    # the rows of the three steps differ, and some step jitters and some step blurs: one graph served every draw
    assert not np.array_equal(e['rows'][0][3], e['rows'][1][3])
    assert any(r[3][:, 0].any() for r in e['rows']) and any(r[4].any() for r in e['rows'])


@pytest.mark.parametrize('mix', ['classmix', None])
def test_unlabelled_half_equals_strong_augment_of_the_mixed_half(mix):
    import torch_semantic_segmentation_amd as tssa
    r = eager(mix)
    st, (x, y, xu) = r['st'], T.batches()
    B, H, W = 2, 64, 128
    lab, _, kept = tssa.upsample_pseudo_labels(T.teacher_low(r['teacher'], xu), st.threshold, size=(H, W))
    assert torch.equal(kept, st.last_kept) and torch.equal(lab, st.pseudo)
    lab = lab.cpu().numpy()
    partner, keys, boxes, color, radius, taps = st.last_rows
    assert color.shape == (B, 8) and radius.shape == (B,) and taps.shape == (B, 12)
    if mix == 'classmix':
        want_i, want_t = R.mix_batch(R.bits_of(xu), lab, partner, sel=R.classmix_select(lab, keys, 19))
    else:
        want_i, want_t = R.mix_batch(R.bits_of(xu), lab, partner, boxes=boxes)
        assert np.array_equal(want_i, R.bits_of(xu))
    assert np.array_equal(R.bits_of(st.mixed), want_i)
    mixed = torch.from_numpy(want_i).view(xu.dtype).to(DEV)
    want_x = tssa.strong_augment(mixed, color, radius, taps, mean=MEAN, std=STD)
    assert np.array_equal(R.bits_of(st.x_all[B:]), R.bits_of(want_x))
    assert color[:, 0].any() or radius.any()
    assert not np.array_equal(R.bits_of(want_x), want_i)                      # a real augmentation in the last step
    assert np.array_equal(st.y_all[B:].cpu().numpy(), want_t)
    assert torch.equal(st.x_all[:B], x) and torch.equal(st.y_all[:B], y)


def test_argument_checks():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    m = T.student()
    tr = E.Trainer(m, E.FlatAdamW(m.parameters(), lr=1e-3), tssa.CrossEntropyLoss(ignore_index=T.IGN))
    with pytest.raises(ValueError):
        tssa.SelfTraining(tr, T.student(), 19, strong='jitter')
    x, y, xu = T.batches()
    with pytest.raises(ValueError):                                           # H = 8 < 9
        tssa.SelfTraining(tr, T.student(), 19, strong=tssa.StrongAugment()).step(x[:, :, :8], y[:, :8], xu[:, :, :8])
