"""GPU: engine.Trainer on a 66-class FastSCNN (bf16, 2 x 3 x 64 x 128): the fused head + loss takes the class-chunked kernels of
csrc/widehead.hip, eagerly and from a captured graph, for the weighted + smoothed cross-entropy and for OHEM; and the first step
against the explicit unfused composition (upsample_logits + the planar loss) on the same low-resolution logits, within the bounds
of tests/test_gpu_wce.py (loss: relative 2e-5; gradients that pass through bf16 storage: cases.rel_err <= 2e-2)."""
import pytest
import torch

from oracle.recipe import formula_state, synthetic_batch
from tests import cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 0.1
C = 66


def student():
    import torch_semantic_segmentation_amd as tssa
    m = cases.product_model('fastscnn', 3, C)
    m.load_state_dict(formula_state(m), strict=True)
    cases.zero_dropout(m)
    m.to(DEV)
    tssa.set_compute_dtype(m, torch.bfloat16)
    return m


def batch():
    x, y = synthetic_batch(2, 64, 128)
    pos = torch.arange(y.numel()).view_as(y)
    y = torch.where(y == 255, y, (y * 7 + pos) % C)          # labels in [0, 66), the 255s of the synthetic batch kept
    assert int((y == 255).sum()) > 0 and int(y[y != 255].max()) == C - 1
    return x.to(DEV), y.to(DEV)


def make_loss(kind, y):
    import torch_semantic_segmentation_amd as tssa
    if kind == 'ohem':
        return tssa.OHEMLoss(ignore_index=255, thresh_loss=4.0, numel_frac=0.05)
    w = tssa.enet_class_weights(tssa.label_histogram(y, C, ignore_index=255))
    return tssa.CrossEntropyLoss(255, weight=w, label_smoothing=EPS).to(DEV)


def run_steps(kind, use_graph, steps=3):
    from torch_semantic_segmentation_amd import engine as E
    x, y = batch()
    m = student()
    tr = E.Trainer(m, E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5), make_loss(kind, y), use_graph=use_graph)
    assert tr.fuse_head_loss
    losses = [tr.step_async(x, y).clone() for _ in range(steps)]
    assert bool(tr._graphs) == use_graph
    return torch.stack(losses).cpu(), torch.cat([p.detach().flatten() for p in m.parameters()]).cpu()


@pytest.mark.parametrize('kind', ['ce', 'ohem'])
def test_three_captured_steps_equal_three_eager_steps(kind):
    eager, graph = run_steps(kind, False), run_steps(kind, True)
    print('%s losses eager %s graph %s' % (kind, eager[0].tolist(), graph[0].tolist()))
    assert bool(torch.isfinite(eager[0]).all()) and float(eager[0][1]) != float(eager[0][0])
    assert torch.equal(eager[0], graph[0])
    assert torch.equal(eager[1], graph[1])


@pytest.mark.parametrize('kind', ['ce', 'ohem'])
def test_first_step_against_the_unfused_composition(kind):
    """The trainer's first loss is the fused operator on the model's low-resolution logits (bit for bit); that operator and the
    unfused composition, each followed by the classifier's backward, agree on the loss and on the classifier's gradients."""
    from torch_semantic_segmentation_amd import engine as E, ops
    x, y = batch()
    loss_fn = make_loss(kind, y)
    m0 = student()
    tr = E.Trainer(m0, E.FlatAdamW(m0.parameters(), lr=1e-3, weight_decay=1e-5), loss_fn, use_graph=False)
    assert tr.fuse_head_loss
    got = tr.step_async(x, y).clone()

    def step(fused):
        m = student()
        m.train()
        shadows = ops.WeightShadows(m)
        shadows.refresh()
        with shadows:
            low = m.forward_lowres(x)
            if fused and kind == 'ohem':
                loss = ops.upsample_ohem_loss(low, y, scale_factor=m.logit_scale, ignore_index=255, thresh_loss=loss_fn.thresh_loss,
                                              numel_frac=loss_fn.numel_frac)
            elif fused:
                loss = ops.upsample_cross_entropy(low, y, scale_factor=m.logit_scale, ignore_index=255, weight=loss_fn.weight,
                                                  label_smoothing=EPS)
            else:       # the explicit composition, in f32 from the same bf16 low-resolution logits
                loss = loss_fn(ops.upsample_logits(ops.materialize(low).float(), scale_factor=m.logit_scale), y)
            loss.backward()
        grads = {n: p.grad.detach().float().cpu() for n, p in m.classifier.named_parameters() if p.grad is not None}
        assert grads
        return loss.detach().cpu(), grads

    (lf, gf), (lu, gu) = step(True), step(False)
    assert torch.equal(got.cpu(), lf)
    print('%s: trainer %.6f fused %.6f unfused %.6f' % (kind, float(got), float(lf), float(lu)))
    assert abs(float(lf) / float(lu) - 1) <= 2e-5
    # The classifier's gradient as ONE tensor (cases.rel_err is a whole-tensor metric), and every tensor on its own except two: the
    # shift of a BatchNorm that a convolution and another train-mode BatchNorm follow has an analytically zero gradient (that
    # BatchNorm removes every per-channel mean), so what either path computes for it is the rounding of the bf16 low-resolution
    # gradient summed over the pixels (4e-6 where the other tensors are 1e-3 .. 5e-2) -- printed, and bounded on the whole gradient's scale.
    flat = lambda g: torch.cat([g[n].flatten() for n in sorted(g)]).numpy()      # noqa: E731
    for n in sorted(gu):
        print('  classifier.%-12s max |fused - unfused| %.3e, max |unfused| %.3e' % (n, float((gf[n] - gu[n]).abs().max()), float(gu[n].abs().max())))
        if not n.endswith('.1.bias'):         # every tensor but those shifts (blocks 0 and 1: depthwise, BN '.1', 1x1, BN '.3') also on its own
            assert cases.rel_err(gf[n].numpy(), gu[n].numpy()) <= 2e-2, n
    d = cases.rel_err(flat(gf), flat(gu))
    print('  classifier, all parameters: rel %.2e' % d)
    assert d <= 2e-2
