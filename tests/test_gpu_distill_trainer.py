"""engine.Trainer(teacher=..., distill_loss=..., distill_weight=...): a FastSCNN student distilled from a second, differently
seeded FastSCNN on synthetic_batch(2, 64, 128).  The distillation term is tssa.distillation_loss (tests/test_gpu_distill.py) on
the two forward_lowres maps; these tests pin how the Trainer assembles it and that the teacher stays frozen.

Both models compute in bf16, the benchmark's arithmetic: there a Trainer step is bit-reproducible (two eager runs, and an eager against
a captured run, give the same bits with or without a teacher), which the bit-for-bit statements below rest on.  With f32 activations
the step of this package is not reproducible from run to run even without a teacher (measured on an MI355X: parameters of two
identical eager 3-step runs differ by up to 1.2e-3), so nothing bit-exact can be asked of a whole step there."""
import pytest
import torch

from oracle.recipe import formula_state, synthetic_batch
from tests import cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def bf16(m):
    import torch_semantic_segmentation_amd as tssa
    tssa.set_compute_dtype(m, torch.bfloat16)
    return m


def student():
    m = cases.product_model('fastscnn')
    m.load_state_dict(formula_state(m), strict=True)
    cases.zero_dropout(m)
    return bf16(m.to(DEV))


def teacher():
    torch.manual_seed(4711)
    m = cases.product_model('fastscnn')
    with torch.no_grad():                     # running statistics away from their (0, 1) defaults
        for mod in m.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                mod.running_mean.normal_(0.0, 0.1)
                mod.running_var.uniform_(0.5, 1.5)
    cases.zero_dropout(m)
    return bf16(m.to(DEV)).train()            # handed over in train mode: the Trainer puts it in eval()


def batch():
    x, y = synthetic_batch(2, 64, 128)
    return x.to(DEV), y.to(DEV)


def trainer(m, t, loss_fn, distill, weight=1.0, use_graph=False):
    from torch_semantic_segmentation_amd import engine as E
    opt = E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
    return E.Trainer(m, opt, loss_fn, use_graph=use_graph, teacher=t, distill_loss=distill, distill_weight=weight)


def frozen_state(t):
    return {k: v.detach().clone() for k, v in list(t.named_parameters()) + list(t.named_buffers())}


def assert_teacher_untouched(t, before):
    now = dict(list(t.named_parameters()) + list(t.named_buffers()))
    assert set(now) == set(before)
    for k, v in before.items():
        assert torch.equal(now[k].detach(), v), k
    assert not t.training and not any(mod.training for mod in t.modules())
    assert all(p.grad is None for p in t.parameters())


@pytest.mark.parametrize('head,kind', [('ce', 'channel'), ('ohem', 'pixel')])
def test_eager_step_loss_is_head_loss_plus_weighted_distillation(head, kind):
    """The step's loss equals, bit for bit, the sum assembled by hand from the same operators on a copy of the two models."""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E, ops
    x, y = batch()
    loss_fn = tssa.CrossEntropyLoss(ignore_index=255) if head == 'ce' else tssa.OHEMLoss(ignore_index=255)
    m, t = student(), teacher()
    before = frozen_state(t)
    tr = trainer(m, t, loss_fn, tssa.DistillationLoss(4.0, kind), weight=3.0)
    assert tr.fuse_head_loss
    got = tr.step_async(x, y)
    assert_teacher_untouched(t, before)
    assert all(p.data_ptr() != q.data_ptr() for g in tr.optimizer.param_groups for p in g['params'] for q in t.parameters())

    m2, t2 = student(), teacher().eval()
    m2.train()
    with torch.no_grad(), E.EvalPrep(t2):
        t_low = ops.materialize(t2.forward_lowres(x))
    shadows = ops.WeightShadows(m2)
    shadows.refresh()
    with shadows:                             # gradients enabled, as in the step: the model takes other kernels without them
        low = ops.materialize(m2.forward_lowres(x)).detach()
    if head == 'ce':
        head_loss = tssa.upsample_cross_entropy(low, y, scale_factor=m2.logit_scale, ignore_index=255)
    else:
        head_loss = ops.upsample_ohem_loss(low, y, scale_factor=m2.logit_scale, ignore_index=255, thresh_loss=loss_fn.thresh_loss,
                                           numel_frac=loss_fn.numel_frac)
    kd = tssa.distillation_loss(low, t_low, 4.0, kind)
    want = head_loss + 3.0 * kd
    print('%s + 3 x %s: head %.6f kd %.6f step %.6f' % (head, kind, float(head_loss), float(kd), float(got)))
    assert float(kd) > 0 and float(head_loss) > 0
    assert torch.equal(got, want)


def run_steps(use_graph, weight=3.0, with_teacher=True, steps=3):
    import torch_semantic_segmentation_amd as tssa
    x, y = batch()
    m = student()
    t = teacher() if with_teacher else None
    before = frozen_state(t) if with_teacher else None
    tr = trainer(m, t, tssa.CrossEntropyLoss(ignore_index=255), tssa.DistillationLoss(4.0, 'channel') if with_teacher else None,
                 weight=weight, use_graph=use_graph)
    losses = [tr.step_async(x, y).clone() for _ in range(steps)]
    assert bool(tr._graphs) == use_graph
    if with_teacher:
        assert_teacher_untouched(t, before)
    return torch.stack(losses).cpu(), torch.cat([p.detach().flatten() for p in m.parameters()]).cpu()


def test_three_captured_steps_equal_three_eager_steps_and_leave_the_teacher_alone():
    eager, graph = run_steps(False), run_steps(True)
    print('losses eager %s graph %s' % (eager[0].tolist(), graph[0].tolist()))
    assert bool(torch.isfinite(eager[0]).all()) and float(eager[0][1]) != float(eager[0][0])
    assert torch.equal(eager[0], graph[0])
    assert torch.equal(eager[1], graph[1])


def test_zero_weight_trains_as_without_a_teacher():
    """distill_weight = 0: the gradient that reaches the low-resolution logits is head + 0 * (finite distillation gradient),
    an exact addition of (signed) zeros, so one step leaves the same parameters, bit for bit, as a Trainer with no teacher."""
    with_t, without = run_steps(False, weight=0.0, steps=1), run_steps(False, with_teacher=False, steps=1)
    assert torch.equal(with_t[0], without[0])
    assert torch.equal(with_t[1], without[1])


def test_constructor_rejections():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    x, y = batch()
    ce, kd = tssa.CrossEntropyLoss(ignore_index=255), tssa.DistillationLoss(4.0, 'channel')
    with pytest.raises(ValueError):
        trainer(student(), teacher(), ce, None)
    with pytest.raises(ValueError):
        trainer(student(), None, ce, kd)
    with pytest.raises(NotImplementedError):
        trainer(student(), torch.nn.Conv2d(3, 19, 1).to(DEV), ce, kd)
    wide = bf16(cases.product_model('fastscnn', 3, 21).to(DEV))         # 21 classes against the student's 19
    tr = trainer(student(), wide, ce, kd)
    with pytest.raises(NotImplementedError):
        tr.step_async(x, y)
    m = student()
    assert E.create_segmentation_trainer(m, E.FlatAdamW(m.parameters(), lr=1e-3), ce, DEV, teacher=teacher(), distill_loss=kd,
                                         distill_weight=2.0).distill_weight == 2.0
