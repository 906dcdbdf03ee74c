"""engine.ModelEMA under engine.Trainer(ema=...): FastSCNN in bf16 on synthetic_batch(2, 64, 128), as tests/test_gpu_distill_trainer.py
(whose docstring says why bit-for-bit statements about whole steps need bf16 activations).

The average is rebuilt on the host from snapshots of the student taken after every step, with the float32 restatement of the
kernel's three roundings (tests/ema_ref.py: lerp32, omd32); everything is compared on bits."""
import functools

import numpy as np
import pytest
import torch

from oracle.recipe import formula_state, synthetic_batch
from tests import cases, ema_ref as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DECAY = 0.9


def student():
    import torch_semantic_segmentation_amd as tssa
    m = cases.product_model('fastscnn')
    m.load_state_dict(formula_state(m), strict=True)
    cases.zero_dropout(m)
    return tssa.set_compute_dtype(m.to(DEV), torch.bfloat16)


def batch():
    x, y = synthetic_batch(2, 64, 128)
    return x.to(DEV), y.to(DEV)


def snapshot(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


def advance(avg, snap, k, decay=DECAY, warmup=False):
    """The restated average after update k: floating-point tensors by the three roundings, integer ones copied."""
    omd = M.omd32(k, decay, warmup)
    return {name: (M.lerp32(avg[name], v, omd) if v.dtype == np.float32 else v.copy()) for name, v in snap.items()}


def same_bits(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def adamw(m):
    from torch_semantic_segmentation_amd import engine as E
    return E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)


def ema_run(use_graph, steps=3, mean_teacher=False, with_ema=True):
    """`steps` trainer steps; returns losses, the student's snapshot after every step (the initial one first) and the objects."""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    x, y = batch()
    m = student()
    opt = adamw(m)
    kw = {}
    ema = None
    if with_ema:
        ema = E.ModelEMA(m, opt, DECAY)
        kw['ema'] = ema
    if mean_teacher:
        kw.update(teacher=ema.module, distill_loss=tssa.DistillationLoss(4.0, 'channel'), distill_weight=3.0)
    tr = E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=255), use_graph=use_graph, **kw)
    snaps, losses = [snapshot(m)], []
    for _ in range(steps):
        losses.append(tr.step_async(x, y).clone())
        snaps.append(snapshot(m))
    assert bool(tr._graphs) == use_graph
    return {'losses': torch.stack(losses).cpu(), 'snaps': snaps, 'm': m, 'opt': opt, 'ema': ema, 'tr': tr}


@functools.lru_cache(maxsize=None)
def eager3():
    return ema_run(False)


def test_three_steps_against_snapshots_eager_and_captured():
    eager, graph = eager3(), ema_run(True)
    for run in (eager, graph):
        ema, m = run['ema'], run['m']
        avg = run['snaps'][0]
        for k, snap in enumerate(run['snaps'][1:]):
            avg = advance(avg, snap, k)
        got = snapshot(ema.module)
        same_bits(got, avg)                                  # parameters (step kernel), running statistics and counters (rows kernel)
        nbt = [k for k in got if k.endswith('num_batches_tracked')]
        assert nbt and all(got[k] == 3 and got[k] == run['snaps'][-1][k] for k in nbt)
        moved = [k for k in got if k.endswith('running_mean') or k.endswith('weight')]
        assert all(got[k].tobytes() != run['snaps'][-1][k].tobytes() for k in moved)     # an average, not a copy of the student
        assert ema.num_updates == 3 and run['opt'].ema_updates == 3
        assert not ema.module.training and not any(mod.training for mod in ema.module.modules())
        assert all(not p.requires_grad and p.grad is None for p in ema.module.parameters())
        assert ema.module.compute_dtype == torch.bfloat16
        mine = {t.untyped_storage().data_ptr() for t in ema.module.state_dict().values()}
        theirs = {t.untyped_storage().data_ptr() for t in m.state_dict().values()} | {run['opt'].flat_grad.untyped_storage().data_ptr()}
        assert not (mine & theirs)
        held = {p.untyped_storage().data_ptr() for p in ema.module.parameters()}
        assert held == {ema.ema_flat.untyped_storage().data_ptr()}                      # every parameter a view into ONE buffer
    assert bool(torch.isfinite(eager['losses']).all()) and float(eager['losses'][1]) != float(eager['losses'][0])
    assert torch.equal(eager['losses'], graph['losses'])
    same_bits(eager['snaps'][-1], graph['snaps'][-1])
    same_bits(snapshot(eager['ema'].module), snapshot(graph['ema'].module))


def test_without_ema_trains_as_before_and_with_it_the_same():
    """Trainer built as today (no ema argument) against the run with the average attached: losses and parameters, bit for bit."""
    without, with_ema = ema_run(False, with_ema=False), eager3()
    assert without['tr'].ema is None and without['opt'].ema_flat is None
    assert torch.equal(without['losses'], with_ema['losses'])
    same_bits(without['snaps'][-1], with_ema['snaps'][-1])


def test_mean_teacher_captured_eager_hand_assembled_and_not_stale():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    eager, graph = ema_run(False, mean_teacher=True), ema_run(True, mean_teacher=True)
    assert eager['tr']._teacher_prep is not None and not eager['tr']._teacher_prep.frozen
    assert torch.equal(eager['losses'], graph['losses'])
    same_bits(eager['snaps'][-1], graph['snaps'][-1])
    same_bits(snapshot(eager['ema'].module), snapshot(graph['ema'].module))

    # by hand: a separately built teacher receives the restated average before each step; a Trainer built for that step alone takes
    # today's frozen path, i.e. a fresh EvalPrep of exactly these weights
    x, y = batch()
    m, t = student(), student()
    opt = adamw(m)
    kd, ce = tssa.DistillationLoss(4.0, 'channel'), tssa.CrossEntropyLoss(ignore_index=255)
    avg, losses = snapshot(m), []
    for k in range(3):
        t.load_state_dict({name: torch.from_numpy(v) for name, v in avg.items()}, strict=True)
        tr = E.Trainer(m, opt, ce, teacher=t, distill_loss=kd, distill_weight=3.0)
        losses.append(tr.step_async(x, y).clone())
        assert tr._teacher_prep.frozen
        avg = advance(avg, snapshot(m), k)
    print('mean teacher losses', eager['losses'].tolist(), 'by hand', [float(v) for v in losses])
    assert torch.equal(torch.stack(losses).cpu(), eager['losses'])
    same_bits(snapshot(m), eager['snaps'][-1])
    same_bits(avg, snapshot(eager['ema'].module))

    # a frozen snapshot of the initial weights as the teacher: the same first step, other losses from the second on
    m, t = student(), student()
    tr = E.Trainer(m, adamw(m), ce, teacher=t, distill_loss=kd, distill_weight=3.0)
    frozen = torch.stack([tr.step_async(x, y).clone() for _ in range(3)]).cpu()
    print('frozen teacher losses', frozen.tolist())
    assert torch.equal(frozen[0], eager['losses'][0])
    assert float(frozen[1]) != float(eager['losses'][1]) and float(frozen[2]) != float(eager['losses'][2])


def test_evaluators_and_resume():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    x, y = batch()
    ce = tssa.CrossEntropyLoss(ignore_index=255)
    m = student()
    opt = adamw(m)
    ema = E.ModelEMA(m, opt, DECAY, warmup=True)
    tr = E.Trainer(m, opt, ce, ema=ema)
    for _ in range(3):
        tr.step_async(x, y)
    saved = {'m': {k: v.clone() for k, v in m.state_dict().items()}, 'opt': opt.state_dict(), 'ema': ema.state_dict()}
    assert saved['opt']['flat']['ema_state'][0] == 3 and saved['ema']['num_updates'] == 3
    loss4 = tr.step_async(x, y).clone()

    m2 = student()
    opt2 = adamw(m2)
    ema2 = E.ModelEMA(m2, opt2, DECAY, warmup=True)
    m2.load_state_dict(saved['m'])
    opt2.load_state_dict(saved['opt'])
    ema2.load_state_dict(saved['ema'])
    assert ema2.num_updates == 3 and opt2.ema_updates == 3
    loss4b = E.Trainer(m2, opt2, ce, ema=ema2).step_async(x, y).clone()
    assert torch.equal(loss4, loss4b)
    same_bits(snapshot(m), snapshot(m2))
    same_bits(snapshot(ema.module), snapshot(ema2.module))
    assert {p.untyped_storage().data_ptr() for p in ema2.module.parameters()} == {ema2.ema_flat.untyped_storage().data_ptr()}

    # the averaged model under the evaluators, against a freshly built model that was handed its state_dict
    fresh = student()
    fresh.load_state_dict(ema.module.state_dict(), strict=True)
    for make in (lambda mod: E.Evaluator(mod, num_classes=19),
                 lambda mod: E.MultiScaleEvaluator(mod, num_classes=19, scales=(0.5, 1.0), flip=True)):
        got, want = make(ema.module).run([(x, y)]), make(fresh).run([(x, y)])
        assert got['miou'] == want['miou'] and got['accuracy'] == want['accuracy'] and 0.0 <= got['miou'] <= 1.0
        assert torch.equal(got['iou'], want['iou']) and torch.equal(got['dice'], want['dice'])
    assert not ema.module.training

    target = student()
    ema.copy_to(target)
    same_bits(snapshot(target), snapshot(ema.module))


def test_stock_optimizer_is_one_rows_launch_over_everything():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    x, y = batch()
    m = student()
    opt = torch.optim.SGD(m.parameters(), lr=1e-2, momentum=0.9)
    ema = E.ModelEMA(m, opt, DECAY, warmup=True)
    assert not ema.flat and ema.table.shape == (len(m.state_dict()), 4)              # one row per parameter and buffer, one launch
    assert set(ema.table[:, 3].tolist()) == {E.EMA_LERP_F32, E.EMA_COPY_I64}
    tr = E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=255), ema=ema)
    assert not tr.flat
    avg = snapshot(m)
    for k in range(3):
        tr.step_async(x, y)
        avg = advance(avg, snapshot(m), k, warmup=True)
    same_bits(snapshot(ema.module), avg)
    assert ema.num_updates == 3
    weights = [k for k in avg if k.endswith('weight')]
    assert weights and all(avg[k].tobytes() != snapshot(m)[k].tobytes() for k in weights[:4])     # an average, not a copy
