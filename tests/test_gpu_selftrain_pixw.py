"""tssa.SelfTraining(pixel_weighting='confidence'): every pseudo-labelled pixel's loss weighted by the teacher's confidence (csrc/pixwce.hip),
on the tiny model and shapes of tests/test_gpu_selftrain_weight.py (FastSCNN in bf16 on synthetic_batch(2, 64, 128), ClassMix, the initial
teacher's median confidence as the threshold).  Three captured steps equal three eager steps on bits, alone and with unsup_weight=0.5 on
top; w_all[B:] is mix_plane (the numpy restatement) of the teacher's confidence as the public operator returns it, with the rows the step
drew, and w_all[:B] is ones; pixel_weighting=None is the SelfTraining of before on bits; the argument checks."""
import numpy as np
import pytest
import torch

from tests import pixwce_ref, selftrain_ref
from tests.test_gpu_selftrain_trainer import DECAY, DEV, IGN, batches, median_confidence, same_bits, snapshot, student, teacher_low

pytestmark = pytest.mark.gpu
NOT_GIVEN = object()


def run(use_graph, pixel_weighting=NOT_GIVEN, unsup_weight=None, mix='classmix', steps=3, norm='weight'):
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    x, y, xu = batches()
    m = student()
    opt = E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
    ema = E.ModelEMA(m, opt, DECAY)
    tr = E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=IGN), use_graph=use_graph, ema=ema)
    kw = {} if pixel_weighting is NOT_GIVEN else dict(pixel_weighting=pixel_weighting, pixel_norm=norm)
    if unsup_weight is not None:
        kw['unsup_weight'] = unsup_weight
    teacher = student()
    st = tssa.SelfTraining(tr, teacher, 19, threshold=0.5, mix=mix, seed=11, **kw)
    st.set_threshold(median_confidence())
    losses, snaps = [], []
    for _ in range(steps):
        losses.append(st.step(x, y, xu).clone())
        snaps.append(snapshot(m))
    assert bool(tr._graphs) == use_graph and len(tr._graphs) <= 1
    return {'losses': torch.stack(losses).cpu(), 'snaps': snaps, 'st': st, 'tr': tr, 'teacher': teacher}


@pytest.mark.parametrize('unsup_weight', [None, 0.5])
def test_three_captured_steps_equal_three_eager_steps(unsup_weight):
    e, g = run(False, 'confidence', unsup_weight), run(True, 'confidence', unsup_weight)
    print('selftrain confidence, lambda', unsup_weight, 'losses', e['losses'].tolist())
    assert bool(torch.isfinite(e['losses']).all()) and float(e['losses'][1]) != float(e['losses'][0])
    assert torch.equal(e['losses'], g['losses'])
    for a, b in zip(e['snaps'], g['snaps']):
        same_bits(a, b)
    assert torch.equal(e['st'].w_all, g['st'].w_all)
    assert e['tr'].loss_fn.pixel_weight.data_ptr() == e['st'].w_all.data_ptr()
    # the map weighs in: another loss than the same run without it
    assert not torch.equal(e['losses'], run(False, None, unsup_weight)['losses'])
    if unsup_weight is not None:
        terms = e['st'].last_group_loss.cpu()
        assert (terms > 0).all() and abs(float(e['losses'][-1]) - float(terms.double().sum())) <= float(np.spacing(np.float32(float(e['losses'][-1]))))


@pytest.mark.parametrize('mix', ['classmix', 'cutmix', None])
def test_the_map_equals_the_restatement(mix):
    import torch_semantic_segmentation_amd as tssa
    r = run(False, 'confidence', mix=mix, steps=2 if mix is not None else 1)
    st, (x, y, xu) = r['st'], batches()
    B, H, W = 2, 64, 128
    lab, conf, _ = tssa.upsample_pseudo_labels(teacher_low(r['teacher'], xu), st.threshold, size=(H, W), want_confidence=True)
    assert torch.equal(lab, st.pseudo) and torch.equal(conf, st.conf)
    partner, keys, boxes = st.last_rows[:3]
    lab = lab.cpu().numpy()
    if mix == 'classmix':
        want = pixwce_ref.mix_plane(selftrain_ref.bits_of(conf), lab, partner, sel=selftrain_ref.classmix_select(lab, keys, 19))
    else:
        want = pixwce_ref.mix_plane(selftrain_ref.bits_of(conf), lab, partner, boxes=boxes)
    assert np.array_equal(selftrain_ref.bits_of(st.w_all[B:]), want)
    assert bool((st.w_all[:B] == 1.0).all())
    c = conf.cpu()
    assert 0.05 < float(c.min()) < float(c.max()) <= 1.0               # the arg-max class holds at least 1 / 19 = 0.0526
    if mix is None:
        assert np.array_equal(want, selftrain_ref.bits_of(conf))
    else:
        assert not np.array_equal(want, selftrain_ref.bits_of(conf))


def test_no_weighting_is_the_self_training_of_before():
    for use_graph in (False, True):
        a, b = run(use_graph, None), run(use_graph)
        assert torch.equal(a['losses'], b['losses'])
        for p, q in zip(a['snaps'], b['snaps']):
            same_bits(p, q)
        assert a['tr'].loss_fn.pixel_weight is None and not hasattr(a['st'], 'w_all')


def test_threshold_zero_is_pure_soft_weighting():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    x, y, xu = batches()
    m = student()
    tr = E.Trainer(m, E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5), tssa.CrossEntropyLoss(ignore_index=IGN))
    st = tssa.SelfTraining(tr, student(), 19, threshold=0.0, mix=None, pixel_weighting='confidence', pixel_norm='pixels')
    loss = st.step(x, y, xu)
    assert bool(torch.isfinite(loss)) and st.last_kept.cpu().tolist() == [64 * 128] * 2 and bool((st.y_all[2:] != IGN).all())


def test_argument_checks():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    m = student()
    opt = E.FlatAdamW(m.parameters(), lr=1e-3)
    tr = E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=IGN))
    for kw in (dict(pixel_weighting='conf'), dict(pixel_weighting='confidence', pixel_norm='mean')):
        with pytest.raises(ValueError):
            tssa.SelfTraining(tr, student(), 19, **kw)
    with pytest.raises(ValueError):
        tssa.SelfTraining(E.Trainer(m, opt, tssa.OHEMLoss(ignore_index=IGN)), student(), 19, pixel_weighting='confidence')
    with pytest.raises(ValueError):
        tssa.SelfTraining(E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=IGN), fuse_head_loss=False), student(), 19,
                          pixel_weighting='confidence')
    with pytest.raises(ValueError):
        tssa.SelfTraining(E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=IGN, label_smoothing=0.1)), student(), 19,
                          pixel_weighting='confidence')
