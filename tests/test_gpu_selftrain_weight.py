"""tssa.SelfTraining(unsup_weight=...): L = L_sup + lambda L_unsup from one head pass (per-sample loss groups, csrc/groupce.hip), on
the tiny model and shapes of tests/test_gpu_selftrain_trainer.py (FastSCNN in bf16 on synthetic_batch(2, 64, 128), ClassMix, the
initial teacher's median confidence as the threshold).  Three captured steps equal three eager steps on bits; unsup_weight=None is the
SelfTraining of before on bits; set_unsup_weight between replays of ONE captured graph moves the step (the prologue's kernel reads
lambda from device memory); the two terms of last_group_loss add up to the loss; 'kept_share' equals the host restatement of
tss_selftrain_weights (tests/groupce_ref.py) on the read-back last_kept; a trainer whose loss is not CrossEntropyLoss is refused."""
import functools

import numpy as np
import pytest
import torch

from tests import groupce_ref as R
from tests.test_gpu_selftrain_trainer import DECAY, DEV, IGN, batches, median_confidence, same_bits, snapshot, student

pytestmark = pytest.mark.gpu
NOT_GIVEN = object()


def run(use_graph, unsup_weight=NOT_GIVEN, weighting='mean', steps=3, schedule=None):
    """`steps` ClassMix steps; schedule: {step index: lambda set before that step}"""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    x, y, xu = batches()
    m = student()
    opt = E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
    ema = E.ModelEMA(m, opt, DECAY)
    tr = E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=IGN), use_graph=use_graph, ema=ema)
    kw = {} if unsup_weight is NOT_GIVEN else dict(unsup_weight=unsup_weight, unsup_weighting=weighting)
    st = tssa.SelfTraining(tr, student(), 19, threshold=0.5, mix='classmix', seed=11, **kw)
    st.set_threshold(median_confidence())
    grouped = unsup_weight is not NOT_GIVEN and unsup_weight is not None
    losses, terms, snaps = [], [], []
    for i in range(steps):
        if schedule and i in schedule:
            st.set_unsup_weight(schedule[i])
        losses.append(st.step(x, y, xu).clone())
        if grouped:
            terms.append(st.last_group_loss.clone())
        snaps.append(snapshot(m))
    assert bool(tr._graphs) == use_graph and len(tr._graphs) <= 1
    return {'losses': torch.stack(losses).cpu(), 'terms': torch.stack(terms).cpu() if terms else None, 'snaps': snaps, 'st': st, 'tr': tr}


@functools.lru_cache(maxsize=None)
def eager_half():
    return run(False, 0.5)


def test_three_captured_steps_equal_three_eager_steps():
    e, g = eager_half(), run(True, 0.5)
    print('selftrain lambda=0.5 losses', e['losses'].tolist(), 'terms', e['terms'].tolist())
    assert bool(torch.isfinite(e['losses']).all()) and float(e['losses'][1]) != float(e['losses'][0])
    assert torch.equal(e['losses'], g['losses']) and torch.equal(e['terms'], g['terms'])
    for a, b in zip(e['snaps'], g['snaps']):
        same_bits(a, b)
    assert (e['terms'] > 0).all(), 'both terms carry a loss (about half of the pseudo-labels are kept)'
    st = e['st']
    assert st.group.cpu().tolist() == [0, 0, 1, 1] and st.weight.cpu().tolist() == [1.0, 1.0, 0.5, 0.5]
    # L_sup + lambda L_unsup is another loss than the mean over all 2B samples
    assert not torch.equal(e['losses'], run(False, None)['losses'])


def test_the_two_terms_add_up_to_the_loss():
    e = eager_half()
    for loss, terms in zip(e['losses'], e['terms']):
        ulp = float(np.spacing(np.float32(abs(float(loss)))))
        diff = abs(float(loss) - float(terms.double().sum()))
        print('selftrain loss %.9g terms %s diff %.3g ulp' % (float(loss), terms.tolist(), diff / ulp))
        assert diff <= ulp


def test_no_weight_is_the_self_training_of_before():
    for use_graph in (False, True):
        a, b = run(use_graph, None), run(use_graph)
        assert torch.equal(a['losses'], b['losses'])
        for p, q in zip(a['snaps'], b['snaps']):
            same_bits(p, q)
        assert a['tr'].loss_fn.sample_group is None and not hasattr(a['st'], 'group')


def test_set_unsup_weight_reaches_a_captured_step():
    """lambda 0.5, 0.5, then 0 for the third step: one captured graph replayed after set_unsup_weight(0.0) against an eager run that
    had the weight 0 for that step -- and that step is another one than with 0.5"""
    g = run(True, 0.5, schedule={2: 0.0})
    e = run(False, 0.5, schedule={2: 0.0})
    assert torch.equal(g['losses'], e['losses']) and torch.equal(g['terms'], e['terms'])
    same_bits(g['snaps'][2], e['snaps'][2])
    assert float(g['terms'][2][1]) == 0.0 and g['st'].weight.cpu().tolist() == [1.0, 1.0, 0.0, 0.0]
    half = eager_half()
    same_bits(g['snaps'][1], half['snaps'][1])
    assert float(g['losses'][2]) != float(half['losses'][2])
    with pytest.raises(AssertionError):
        same_bits(g['snaps'][2], half['snaps'][2])
    # a weight of 0 from the start: the supervised term alone drives the step
    z = run(True, 0.0, steps=1)
    assert float(z['terms'][0][1]) == 0.0 and float(z['losses'][0]) == float(z['terms'][0][0])


def test_kept_share_equals_the_host_restatement():
    for use_graph in (False, True):
        r = run(use_graph, 0.7, weighting='kept_share', steps=2)
        st = r['st']
        kept = st.last_kept.cpu().tolist()
        group, weight = R.selftrain_weights(kept, 64 * 128, 0.7, 1)
        assert np.array_equal(st.group.cpu().numpy(), group)
        assert np.array_equal(st.weight.cpu().numpy().view(np.uint32), weight.view(np.uint32)), (st.weight.cpu().tolist(), weight.tolist(), kept)
        assert 0.0 < float(weight[2]) < 0.7


def test_argument_checks():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    m = student()
    opt = E.FlatAdamW(m.parameters(), lr=1e-3)
    with pytest.raises(ValueError):
        tssa.SelfTraining(E.Trainer(m, opt, tssa.OHEMLoss(ignore_index=IGN)), student(), 19, unsup_weight=0.5)
    tr = E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=IGN))
    with pytest.raises(ValueError):
        tssa.SelfTraining(E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=IGN), fuse_head_loss=False), student(), 19, unsup_weight=0.5)
    for kw in (dict(unsup_weight=-1.0), dict(unsup_weight=float('nan')), dict(unsup_weight=0.5, unsup_weighting='share')):
        with pytest.raises(ValueError):
            tssa.SelfTraining(tr, student(), 19, **kw)
    with pytest.raises(ValueError):
        tssa.SelfTraining(tr, student(), 19).set_unsup_weight(0.5)
    tssa.SelfTraining(E.Trainer(m, opt, tssa.OHEMLoss(ignore_index=IGN)), student(), 19)          # without a weight: as before
