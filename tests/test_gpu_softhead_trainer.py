"""engine.Trainer with FocalLoss / DiceLoss built with fused_head=True: FastSCNN on synthetic_batch(2, 64, 128), the loss taken by
tssa.upsample_focal_loss / upsample_dice_loss on model.forward_lowres(x) (tests/test_gpu_softhead.py pins the operators).

The first-loss comparison against the unfused trainer runs both models in f32, where the two routes differ by rounding only (bound:
the loss bound of tests/test_gpu_softhead.py, relative 2e-5); with bf16 activations the unfused route rounds the full-resolution
logits to bf16, a tensor the fused route never forms.  The bit-for-bit statements run in bf16, the benchmark's arithmetic, as in
tests/test_gpu_wce.py::test_trainer_three_captured_steps_equal_three_eager_steps."""
import pytest
import torch

from tests.test_gpu_distill_trainer import batch, teacher
from tests.test_gpu_wce import student, trainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WHICH = pytest.mark.parametrize('which', ['focal', 'dice'])


def loss_module(which, fused_head=True):
    import torch_semantic_segmentation_amd as tssa
    if which == 'focal':
        return tssa.FocalLoss(ignore_index=255, fused_head=fused_head)
    return tssa.DiceLoss(19, ignore_index=255, fused_head=fused_head)


def f32_student():
    from oracle.recipe import formula_state
    from tests import cases
    m = cases.product_model('fastscnn')
    m.load_state_dict(formula_state(m), strict=True)
    cases.zero_dropout(m)
    return m.to(DEV)


@WHICH
def test_first_eager_loss_matches_the_unfused_trainer(which):
    x, y = batch()
    fused, unfused = trainer(f32_student(), loss_module(which)), trainer(f32_student(), loss_module(which, False))
    assert fused.fuse_head_loss and not unfused.fuse_head_loss
    a, b = float(fused.step_async(x, y)), float(unfused.step_async(x, y))
    print('%s first loss fused %.7f unfused %.7f rel %.2e' % (which, a, b, abs(a / b - 1)))
    assert b > 0 and abs(a / b - 1) <= 2e-5


@WHICH
def test_eager_step_is_the_fused_operator_on_the_lowres_logits(which):
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    x, y = batch()
    tr = trainer(student(), loss_module(which))
    assert tr.fuse_head_loss
    got = tr.step_async(x, y)
    m2 = student()
    m2.train()
    shadows = ops.WeightShadows(m2)
    shadows.refresh()
    with shadows:
        low = ops.materialize(m2.forward_lowres(x)).detach()
    if which == 'focal':
        want = tssa.upsample_focal_loss(low, y, scale_factor=m2.logit_scale, ignore_index=255)
    else:
        want = tssa.upsample_dice_loss(low, y, 19, scale_factor=m2.logit_scale, ignore_index=255)
    assert torch.equal(got, want) and float(want) > 0


def run_steps(which, use_graph, steps=3):
    x, y = batch()
    m = student()
    tr = trainer(m, loss_module(which), use_graph=use_graph)
    assert tr.fuse_head_loss
    losses = [tr.step_async(x, y).clone() for _ in range(steps)]
    assert bool(tr._graphs) == use_graph
    return torch.stack(losses).cpu(), torch.cat([p.detach().flatten() for p in m.parameters()]).cpu()


@WHICH
def test_three_captured_steps_equal_three_eager_steps(which):
    eager, graph = run_steps(which, False), run_steps(which, True)
    print('%s losses eager %s graph %s' % (which, eager[0].tolist(), graph[0].tolist()))
    assert bool(torch.isfinite(eager[0]).all()) and float(eager[0][1]) != float(eager[0][0])
    assert torch.equal(eager[0], graph[0])
    assert torch.equal(eager[1], graph[1])


@WHICH
def test_fused_head_false_keeps_the_unfused_route(which):
    tr = trainer(student(), loss_module(which, False))
    assert not tr.fuse_head_loss
    from torch_semantic_segmentation_amd import engine as E
    m = student()
    tr = E.Trainer(m, E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5), loss_module(which), fuse_head_loss=False)
    assert not tr.fuse_head_loss


@WHICH
def test_one_step_with_a_teacher_runs_and_is_finite(which):
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    x, y = batch()
    m = student()
    tr = E.Trainer(m, E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5), loss_module(which), teacher=teacher(),
                   distill_loss=tssa.DistillationLoss(4.0, 'pixel'), distill_weight=3.0)
    assert tr.fuse_head_loss
    with_teacher = tr.step_async(x, y)
    alone = trainer(student(), loss_module(which)).step_async(x, y)
    print('%s step loss with teacher %.6f, head loss alone %.6f' % (which, float(with_teacher), float(alone)))
    assert bool(torch.isfinite(with_teacher)) and float(with_teacher) > float(alone) > 0
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_dice_with_more_than_24_classes_runs_through_the_operators_fallback():
    """DiceLoss(fused_head=True) at 25 classes: the Trainer still takes the low-resolution route; upsample_dice_loss falls back."""
    from oracle.recipe import formula_state
    from tests import cases
    import torch_semantic_segmentation_amd as tssa
    m = cases.product_model('fastscnn', 3, 25)
    m.load_state_dict(formula_state(m), strict=True)
    cases.zero_dropout(m)
    m.to(DEV)
    tssa.set_compute_dtype(m, torch.bfloat16)
    x, y = batch()
    tr = trainer(m, tssa.DiceLoss(25, ignore_index=255, fused_head=True))
    assert tr.fuse_head_loss
    loss = tr.step_async(x, y)
    assert bool(torch.isfinite(loss)) and float(loss) > 0
