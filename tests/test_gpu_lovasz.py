"""tssa.LovaszSoftmaxLoss / lovasz_softmax_loss (csrc/lovasz.hip) against the f64 restatement of the reference's formula
(tests/lovasz_ref.py, pinned to the reference's own numbers by tests/test_lovasz_oracle.py), both weightings.

Bounds.  Loss: relative 1e-5 (the f32 loss tolerance of test_cross_entropy_fwd_bwd), f32 and bf16 logits alike (bf16
inputs are bf16-exact and the restatement reads the same values).  Gradient, f32 logits: the restatement's own f32-vs-f64
distance d_ref on that input, times 3 (the convention of the bf16 kernel tests), floor 2e-5 (test_ohem_loss_matches_
reference_formula); d_ref varies by orders of magnitude with how many near-equal errors swap ranks in f32, so it is
measured per input.  Gradient, bf16 logits: 2e-2 (stored in bf16), as for CE and OHEM.  Distances are cases.rel_err.
Inputs are built on the CPU from fixed seeds; every case is asserted tie-free in f64 first (the tie rule has its own test).
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle.recipe import formula_state, synthetic_batch
from tests import cases, lovasz_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

#            B, C,  H,   W, ignore_index, fraction of label 255, absent class, gain
CASES = {
    'ignore10':     (2, 19, 32, 64, 255, 0.10, None, 2.0),
    'ignore_none':  (2, 19, 32, 64, None, 0.10, None, 1.0),      # labels 255 stay in the set: background of every class
    'absent_class': (2, 5, 48, 80, 255, 0.10, 3, 2.0),           # 7680 pixels: 2 sort tiles, the second ragged
    'four_tiles':   (1, 19, 96, 160, 255, 0.10, None, 3.0),      # 15360 pixels = 3.75 tiles of 4096
    'few_kept':     (2, 19, 32, 64, 255, 0.995, None, 2.0),
}


@functools.lru_cache(maxsize=None)
def case_input(name, bf16):
    B, C, H, W, ignore, frac, absent, gain = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 100)
    logits = gain * torch.randn(B, C, H, W, generator=g)
    if bf16:
        logits = logits.bfloat16().float()
    target = torch.randint(0, C, (B, H, W), generator=g)
    if absent is not None:
        target[target == absent] = (absent + 1) % C
    target[torch.rand(B, H, W, generator=g) < frac] = 255
    return logits, target


@functools.lru_cache(maxsize=None)
def case_reference(name, bf16, variant):
    """(f64 loss, f64 gradient, d_ref) of the restatement; computed once, never modified."""
    B, C, H, W, ignore, frac, absent, gain = CASES[name]
    logits, target = case_input(name, bf16)
    assert R.tie_free(logits, target, C, ignore)
    l64, g64 = R.loss_and_grad(logits, target, C, ignore, variant, torch.float64)
    _, g32 = R.loss_and_grad(logits, target, C, ignore, variant, torch.float32)
    return float(l64), g64.numpy(), cases.rel_err(g32.numpy(), g64.numpy())


def hip_loss_and_grad(logits, target, C, ignore, variant, dtype=torch.float32, scale=None):
    import torch_semantic_segmentation_amd as tssa
    x = logits.to(DEV).to(dtype).requires_grad_(True)
    loss = tssa.lovasz_softmax_loss(x, target.to(DEV), C, ignore_index=ignore, variant=variant)
    (loss if scale is None else scale * loss).backward()
    return loss.detach().cpu(), x.grad.detach().float().cpu()


@pytest.mark.parametrize('variant', R.VARIANTS)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('name', list(CASES))
def test_loss_and_gradient_vs_f64_restatement(name, dtype, variant):
    B, C, H, W, ignore, frac, absent, gain = CASES[name]
    bf16 = dtype == torch.bfloat16
    logits, target = case_input(name, bf16)
    want_loss, want_grad, d_ref = case_reference(name, bf16, variant)
    if absent is not None:
        assert (target == absent).sum() == 0
    if ignore is None:
        assert (target == 255).sum() > 0
    loss, grad = hip_loss_and_grad(logits, target, C, ignore, variant, dtype)
    d_loss = abs(float(loss) / want_loss - 1)
    d_grad = cases.rel_err(grad.numpy(), want_grad)
    bound = 2e-2 if bf16 else max(2e-5, 3 * d_ref)
    print('lovasz %-12s %-4s %-9s loss %.6f rel %.2e | grad d_ref %.2e hip %.2e bound %.2e'
          % (name, 'bf16' if bf16 else 'f32', variant, want_loss, d_loss, d_ref, d_grad, bound))
    assert torch.isfinite(grad).all()
    assert d_loss <= 1e-5
    assert d_grad <= bound


@pytest.mark.parametrize('key,ignore', [('ignore255', 255), ('ignore_none', None)])
def test_fixture_input_reproduces_the_recorded_reference(golden_dir, key, ignore):
    """The reference's own f32 loss and gradient (tests/golden/lovasz.npz), default variant."""
    g = cases.load_npz(os.path.join(golden_dir, 'lovasz.npz'))
    logits, target = torch.from_numpy(g['logits']), torch.from_numpy(g['target'])
    assert R.tie_free(logits, target, 7, ignore)
    _, g64 = R.loss_and_grad(logits, target, 7, ignore, 'reference', torch.float64)
    d_ref = cases.rel_err(g[key + '/grad'], g64.numpy())
    loss, grad = hip_loss_and_grad(logits, target, 7, ignore, 'reference')
    d_loss = abs(float(loss) / float(g[key + '/loss']) - 1)
    d_grad = cases.rel_err(grad.numpy(), g[key + '/grad'])
    print('lovasz fixture %s: loss rel %.2e | grad d_ref %.2e hip-vs-recorded %.2e' % (key, d_loss, d_ref, d_grad))
    assert d_loss <= 1e-5
    assert d_grad <= max(2e-5, 3 * d_ref)


@pytest.mark.parametrize('variant', R.VARIANTS)
def test_exact_ties_follow_ascending_pixel_index(variant):
    """Rows 8..15 of every image repeat rows 0..7 (logits and labels): thousands of exactly equal errors per class.  The
    stable sort orders them by flat pixel index, which is what the f64 restatement with a stable sort does."""
    B, C, H, W = 2, 19, 32, 64
    logits, target = (t.clone() for t in case_input('ignore10', False))
    logits[:, :, 8:16] = logits[:, :, 0:8]
    target[:, 8:16] = target[:, 0:8]
    assert not R.tie_free(logits, target, C, 255)
    l64, g64 = R.loss_and_grad(logits, target, C, 255, variant, torch.float64, stable=True)
    _, g32 = R.loss_and_grad(logits, target, C, 255, variant, torch.float32, stable=True)
    d_ref = cases.rel_err(g32.numpy(), g64.numpy())
    loss, grad = hip_loss_and_grad(logits, target, C, 255, variant)
    d_loss, d_grad = abs(float(loss) / float(l64) - 1), cases.rel_err(grad.numpy(), g64.numpy())
    print('lovasz ties %-9s loss rel %.2e | grad d_ref %.2e hip %.2e' % (variant, d_loss, d_ref, d_grad))
    assert d_loss <= 1e-5
    assert d_grad <= max(2e-5, 3 * d_ref)
    loss2, grad2 = hip_loss_and_grad(logits, target, C, 255, variant)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_all_ignored_target_gives_zero_loss_and_zero_gradient(dtype):
    logits, _ = case_input('ignore10', False)
    target = torch.full((2, 32, 64), 255)
    for variant in R.VARIANTS:
        loss, grad = hip_loss_and_grad(logits, target, 19, 255, variant, dtype)
        assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


@pytest.mark.parametrize('name', ['ignore10', 'four_tiles'])
def test_two_calls_are_bit_identical(name):
    B, C, H, W, ignore, *_ = CASES[name]
    logits, target = case_input(name, False)
    for variant in R.VARIANTS:
        a = hip_loss_and_grad(logits, target, C, ignore, variant)
        b = hip_loss_and_grad(logits, target, C, ignore, variant)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_classes_sorted_in_chunks_give_the_same_bits():
    """At 8x19x1024x2048 the classes are sorted a few at a time (bounded sort buffers); the same path at a small size:
    chunks of 4 classes (the last one ragged: 19 = 4*4 + 3) and of 1 against all 19 at once."""
    from torch_semantic_segmentation_amd import ops
    B, C, H, W, ignore, *_ = CASES['four_tiles']
    logits, target = case_input('four_tiles', False)
    assert ops.lovasz_chunk_classes == 0
    want = hip_loss_and_grad(logits, target, C, ignore, 'reference')
    try:
        for chunk in (4, 1):
            ops.lovasz_chunk_classes = chunk
            got = hip_loss_and_grad(logits, target, C, ignore, 'reference')
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), chunk
    finally:
        ops.lovasz_chunk_classes = 0


def test_grad_out_is_honoured():
    B, C, H, W, ignore, *_ = CASES['ignore10']
    logits, target = case_input('ignore10', False)
    loss, grad = hip_loss_and_grad(logits, target, C, ignore, 'reference')
    loss7, grad7 = hip_loss_and_grad(logits, target, C, ignore, 'reference', scale=0.7)
    assert torch.equal(loss, loss7)
    # the scale enters before the one rounding to f32: 0.7f * grad differs by an ulp or two
    assert cases.rel_err(grad7.numpy(), 0.7 * grad.double().numpy()) <= 1e-6
    want_loss, want_grad, d_ref = case_reference('ignore10', False, 'reference')
    assert cases.rel_err(grad7.numpy(), 0.7 * want_grad) <= max(2e-5, 3 * d_ref)


def test_module_defaults_and_argument_errors():
    import torch_semantic_segmentation_amd as tssa
    m = tssa.LovaszSoftmaxLoss(19)
    assert (m.num_classes, m.ignore_index, m.variant) == (19, -100, 'reference')
    logits, target = case_input('ignore10', False)
    x, t = logits.to(DEV), target.to(DEV)
    want = tssa.lovasz_softmax_loss(x, t, 19, ignore_index=255)
    assert torch.equal(tssa.LovaszSoftmaxLoss(19, 255)(x, t), want)
    assert torch.equal(tssa.LovaszSoftmaxFn.apply(x, t, 255, 'reference'), want)
    with pytest.raises(ValueError):
        tssa.lovasz_softmax_loss(x, t, 18, ignore_index=255)
    with pytest.raises(ValueError):
        tssa.LovaszSoftmaxLoss(20, 255)(x, t)
    with pytest.raises(ValueError):
        tssa.lovasz_softmax_loss(x, t, 19, variant='jaccard')
    with pytest.raises(NotImplementedError):
        tssa.lovasz_softmax_loss(x[:, :, :3, :5].contiguous(), t[:, :3, :5].contiguous(), 19)


def test_trainer_runs_the_lovasz_loss_eagerly_and_as_a_captured_graph():
    """Trainer(model, opt, LovaszSoftmaxLoss) takes the unfused model(x) -> loss_fn path; the step (sort, scan, gradient)
    is captured in a HIP graph and gives the eager trajectory (bound: test_flat_adamw_and_graph_replay_match_eager's)."""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    x, y = synthetic_batch(2, 64, 128)
    x, y = x.to(DEV), y.to(DEV)
    results = []
    for use_graph in (False, True):
        m = cases.product_model('fastscnn')
        m.load_state_dict(formula_state(m), strict=True)
        cases.zero_dropout(m)
        m.to(DEV)
        opt = E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
        tr = E.Trainer(m, opt, tssa.LovaszSoftmaxLoss(19, 255), use_graph=use_graph)
        assert not tr.fuse_head_loss
        results.append([tr.step_async(x, y).item() for _ in range(2)])
        assert bool(tr._graphs) == use_graph and tr.use_graph == use_graph
    assert np.isfinite(results[0]).all() and np.isfinite(results[1]).all()
    assert results[0][0] > 0 and results[0][1] != results[0][0]
    assert np.allclose(results[1], results[0], rtol=1e-3), results
