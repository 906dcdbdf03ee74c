"""tssa.SelfTraining over engine.Trainer: FastSCNN in bf16 on synthetic_batch(2, 64, 128) plus a second seeded batch as the unlabelled
frames, set up as tests/test_gpu_ema_trainer.py sets its runs up (whose docstring says why bit-for-bit statements about whole steps need
bf16 activations).  Three steps captured equal three steps eager on bits -- losses, parameters, the average -- with ClassMix, with
CutMix and with the trainer's own average as the teacher; the mixed half of the 2B batch the student saw equals the restatement
(tests/selftrain_ref.py) built from the pseudo-labels the public operator returns for the teacher's own forward_lowres; and a plain
Trainer, run before and after self-training steps in one process, keeps its bits (SelfTraining leaves no state behind in the
library or the package; engine.Trainer itself is not edited)."""
import functools

import numpy as np
import pytest
import torch

from oracle.recipe import formula_state, synthetic_batch
from tests import cases, selftrain_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DECAY = 0.9
IGN = 255


def student():
    import torch_semantic_segmentation_amd as tssa
    m = cases.product_model('fastscnn')
    m.load_state_dict(formula_state(m), strict=True)
    cases.zero_dropout(m)
    return tssa.set_compute_dtype(m.to(DEV), torch.bfloat16)


def batches():
    x, y = synthetic_batch(2, 64, 128)
    xu, _ = synthetic_batch(2, 64, 128, seed=4321)
    return x.to(DEV), y.to(DEV), xu.to(DEV)


def snapshot(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


def same_bits(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def teacher_low(teacher, xu, frozen=True):
    from torch_semantic_segmentation_amd import engine as E, ops
    with torch.no_grad(), E.EvalPrep(teacher, frozen=frozen):
        return ops.to_nhwc(ops.materialize(teacher.forward_lowres(xu)))


@functools.lru_cache(maxsize=None)
def median_confidence():
    """the threshold of the runs: the median confidence of the initial teacher on the unlabelled frames, so that about half is kept"""
    import torch_semantic_segmentation_amd as tssa
    xu = batches()[2]
    t = student().eval()
    _, conf, _ = tssa.upsample_pseudo_labels(teacher_low(t, xu), 0.0, size=tuple(xu.shape[-2:]), want_confidence=True)
    return float(conf.median())


def run(use_graph, mix, mean_teacher=False, steps=3):
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    x, y, xu = batches()
    m = student()
    opt = E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
    ema = E.ModelEMA(m, opt, DECAY)
    teacher = ema.module if mean_teacher else student()
    tr = E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=IGN), use_graph=use_graph, ema=ema)
    st = tssa.SelfTraining(tr, teacher, 19, threshold=0.5, mix=mix, seed=11)
    st.set_threshold(median_confidence())
    losses, kept = [], []
    for _ in range(steps):
        losses.append(st.step(x, y, xu).clone())
        kept.append(st.last_kept.clone())
    assert bool(tr._graphs) == use_graph
    assert st._teacher_prep.frozen == (not mean_teacher)
    return {'losses': torch.stack(losses).cpu(), 'kept': torch.stack(kept).cpu(), 'm': m, 'ema': ema, 'st': st, 'teacher': teacher, 'tr': tr}


@functools.lru_cache(maxsize=None)
def eager(mix, mean_teacher=False):
    return run(False, mix, mean_teacher)


@pytest.mark.parametrize('mix,mean_teacher', [('classmix', False), ('cutmix', False), ('classmix', True)])
def test_three_steps_captured_equal_eager(mix, mean_teacher):
    e, g = eager(mix, mean_teacher), run(True, mix, mean_teacher)
    print('selftrain', mix, mean_teacher, 'losses', e['losses'].tolist(), 'kept', e['kept'].tolist())
    assert bool(torch.isfinite(e['losses']).all()) and float(e['losses'][1]) != float(e['losses'][0])
    assert torch.equal(e['losses'], g['losses']) and torch.equal(e['kept'], g['kept'])
    same_bits(snapshot(e['m']), snapshot(g['m']))
    same_bits(snapshot(e['ema'].module), snapshot(g['ema'].module))
    assert torch.equal(e['st'].x_all, g['st'].x_all) and torch.equal(e['st'].y_all, g['st'].y_all)
    n = 64 * 128
    # the threshold is the INITIAL teacher's median confidence: about half of the first step's pixels (a teacher that moves grows
    # more confident from step to step, so nothing is said about the later ones)
    assert ((e['kept'][0] > 0.2 * n) & (e['kept'][0] < 0.8 * n)).all() and (e['kept'] > 0).all() and (e['kept'] < n).all()
    if mean_teacher:                       # the teacher moved: other pseudo-labels than the frozen teacher's from the second step on
        f = eager(mix, False)
        assert torch.equal(e['kept'][0], f['kept'][0]) and not torch.equal(e['kept'][1:], f['kept'][1:])


@pytest.mark.parametrize('mix', ['classmix', 'cutmix', None])
def test_mixed_half_equals_the_restatement(mix):
    """the second half of x_all / y_all after the last step, from the pseudo-labels of the public operator on the (frozen) teacher's own
    forward_lowres, the rows the step drew, and the numpy restatement of the pick and the select"""
    import torch_semantic_segmentation_amd as tssa
    r = eager(mix) if mix is not None else run(False, None, steps=1)
    st, (x, y, xu) = r['st'], batches()
    B, H, W = 2, 64, 128
    lab, _, kept = tssa.upsample_pseudo_labels(teacher_low(r['teacher'], xu), st.threshold, size=(H, W))
    assert torch.equal(kept, st.last_kept) and torch.equal(lab, st.pseudo)
    lab = lab.cpu().numpy()
    assert 0.2 < (lab != IGN).mean() < 0.8          # a frozen teacher: the share of the first step at every step
    partner, keys, boxes = st.last_rows
    assert partner.tolist() == ([1, 0] if mix is not None else [0, 1])
    if mix == 'classmix':
        sel = R.classmix_select(lab, keys, 19)
        assert np.array_equal(st.sel.cpu().numpy(), sel) and sel.sum() > 0
        want_i, want_t = R.mix_batch(R.bits_of(xu), lab, partner, sel=sel)
    else:
        if mix == 'cutmix':
            area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) / float(H * W)
            assert ((area > 0.2) & (area < 0.55)).all() and (boxes[:, 2] <= H).all() and (boxes[:, 3] <= W).all() and (boxes >= 0).all()
        want_i, want_t = R.mix_batch(R.bits_of(xu), lab, partner, boxes=boxes)
    assert np.array_equal(R.bits_of(st.x_all[B:]), want_i) and np.array_equal(st.y_all[B:].cpu().numpy(), want_t)
    assert torch.equal(st.x_all[:B], x) and torch.equal(st.y_all[:B], y)
    if mix is None:
        assert np.array_equal(want_i, R.bits_of(xu)) and np.array_equal(want_t, lab.astype(np.int64))
    else:
        assert not np.array_equal(want_i, R.bits_of(xu)) and not np.array_equal(want_i, R.bits_of(xu)[partner])      # a real mix


def test_plain_trainer_keeps_its_bits():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E

    def plain(use_graph):
        x, y, _ = batches()
        m = student()
        tr = E.Trainer(m, E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5), tssa.CrossEntropyLoss(ignore_index=IGN), use_graph=use_graph)
        return torch.stack([tr.step_async(x, y).clone() for _ in range(3)]).cpu(), snapshot(m)

    before = plain(False)
    run(True, 'classmix', steps=1)
    for after in (plain(False), plain(True)):
        assert torch.equal(before[0], after[0])
        same_bits(before[1], after[1])


def test_argument_checks():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    m = student()
    tr = E.Trainer(m, E.FlatAdamW(m.parameters(), lr=1e-3), tssa.CrossEntropyLoss(ignore_index=IGN))
    with pytest.raises(ValueError):
        tssa.SelfTraining(tr, student(), 19, mix='mixup')
    with pytest.raises(ValueError):
        tssa.SelfTraining(tr, student(), 19, ignore_index=18)
    with pytest.raises(NotImplementedError):
        tssa.SelfTraining(tr, torch.nn.Conv2d(3, 19, 1), 19)
    x, y, xu = batches()
    with pytest.raises(ValueError):
        tssa.SelfTraining(tr, student(), 19).step(x, y, xu[:1])
