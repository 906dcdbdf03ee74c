"""tssa.FocalLoss / focal_loss and tssa.DiceLoss / dice_loss (csrc/softloss.hip) against the f64 restatements of
tests/softloss_ref.py (pinned to the reference's own focal numbers and to hand-worked values by tests/test_softloss_oracle.py).

Bounds: those of tests/test_gpu_lovasz.py.  Loss: relative 1e-5, f32 and bf16 logits alike (bf16 inputs are bf16-exact and
the restatement reads the same values).  Gradient, f32 logits: max(2e-5, 3 d_ref), d_ref the restatement's own f32-vs-f64
distance on that input (where the f32 restatement is not finite, at saturated pixels, the floor 2e-5 alone).  Gradient,
bf16 logits: 2e-2 (stored in bf16).  Distances are cases.rel_err.  Inputs are built on the CPU from fixed seeds; every
case carries about 10 % labels 255 and a handful of out-of-range labels (-1, 300) that must behave as ignored.
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle.recipe import formula_state, synthetic_batch
from tests import cases, softloss_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ALPHA = 0.25
GAMMAS = (0.0, 0.5, 2.0)
DTYPES = pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])

#            B,  C,  H,  W, fraction of label 255, absent class
CASES = {
    'sub_wave':    (2, 19, 8, 24, 0.10, None),      # 24 pixel groups per image: less than one wave
    'two_blocks':  (1, 5, 48, 80, 0.10, 3),         # 480 pixel groups: two blocks, the second ragged; class 3 absent
    'odd_batch':   (3, 21, 16, 40, 0.10, None),     # odd batch, more than 20 classes
    'two_classes': (2, 2, 8, 8, 0.10, None),        # the smallest class count
    'few_valid':   (2, 19, 32, 64, 0.995, None),
}


@functools.lru_cache(maxsize=None)
def case_input(name, bf16):
    B, C, H, W, frac, absent = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 300)
    logits = 2.0 * torch.randn(B, C, H, W, generator=g)
    if bf16:
        logits = logits.bfloat16().float()
    target = torch.randint(0, C, (B, H, W), generator=g)
    if absent is not None:
        target[target == absent] = (absent + 1) % C
    target[torch.rand(B, H, W, generator=g) < frac] = 255
    flat = target.view(-1)
    flat[[3, 17, 40]] = -1
    flat[[5, 29]] = 300
    return logits, target


def reference(fn, logits, target, *args):
    """(f64 loss, f64 gradient, d_ref) of a restatement; d_ref is None where the f32 restatement is not finite."""
    l64, g64 = R.loss_and_grad(fn, logits, target, torch.float64, *args)
    _, g32 = R.loss_and_grad(fn, logits, target, torch.float32, *args)
    d_ref = cases.rel_err(g32.numpy(), g64.numpy()) if bool(torch.isfinite(g32).all()) else None
    return float(l64), g64.numpy(), d_ref


@functools.lru_cache(maxsize=None)
def focal_reference(name, bf16, gamma, variant):
    return reference(R.focal_loss, *case_input(name, bf16), ALPHA, gamma, 255, variant)


@functools.lru_cache(maxsize=None)
def dice_reference(name, bf16, smooth):
    return reference(R.dice_loss, *case_input(name, bf16), CASES[name][1], smooth, 255)


def grad_bound(bf16, d_ref):
    if bf16:
        return 2e-2
    return 2e-5 if d_ref is None else max(2e-5, 3 * d_ref)


def hip_focal(logits, target, gamma, variant, dtype=torch.float32, ignore=255, scale=None, alpha=ALPHA):
    import torch_semantic_segmentation_amd as tssa
    x = logits.to(DEV).to(dtype).requires_grad_(True)
    loss = tssa.focal_loss(x, target.to(DEV), alpha=alpha, gamma=gamma, ignore_index=ignore, variant=variant)
    (loss if scale is None else scale * loss).backward()
    return loss.detach().cpu(), x.grad.detach().float().cpu()


def hip_dice(logits, target, C, smooth, dtype=torch.float32, ignore=255, scale=None):
    import torch_semantic_segmentation_amd as tssa
    x = logits.to(DEV).to(dtype).requires_grad_(True)
    loss = tssa.dice_loss(x, target.to(DEV), C, smooth=smooth, ignore_index=ignore)
    (loss if scale is None else scale * loss).backward()
    return loss.detach().cpu(), x.grad.detach().float().cpu()


def check(tag, got, want, bf16):
    (loss, grad), (want_loss, want_grad, d_ref) = got, want
    d_loss = abs(float(loss) / want_loss - 1)
    d_grad = cases.rel_err(grad.numpy(), want_grad)
    bound = grad_bound(bf16, d_ref)
    print('%s loss %.6f rel %.2e | grad d_ref %s hip %.2e bound %.2e'
          % (tag, want_loss, d_loss, 'n/a' if d_ref is None else '%.2e' % d_ref, d_grad, bound))
    assert torch.isfinite(grad).all()
    assert d_loss <= 1e-5
    assert d_grad <= bound


@pytest.mark.parametrize('variant', R.FOCAL_VARIANTS)
@pytest.mark.parametrize('gamma', GAMMAS)
@DTYPES
@pytest.mark.parametrize('name', list(CASES))
def test_focal_loss_and_gradient_vs_f64_restatement(name, dtype, gamma, variant):
    bf16 = dtype == torch.bfloat16
    logits, target = case_input(name, bf16)
    assert (target == 255).sum() > 0 and (target == -1).sum() == 3 and (target == 300).sum() == 2
    got = hip_focal(logits, target, gamma, variant, dtype)
    check('focal %-11s %-4s g%.1f %-9s' % (name, 'bf16' if bf16 else 'f32', gamma, variant), got,
          focal_reference(name, bf16, gamma, variant), bf16)


@pytest.mark.parametrize('smooth', [1.0, 0.0])
@DTYPES
@pytest.mark.parametrize('name', list(CASES))
def test_dice_loss_and_gradient_vs_f64_restatement(name, dtype, smooth):
    bf16 = dtype == torch.bfloat16
    B, C, H, W, frac, absent = CASES[name]
    logits, target = case_input(name, bf16)
    if absent is not None:
        assert (target == absent).sum() == 0
    got = hip_dice(logits, target, C, smooth, dtype)
    check('dice  %-11s %-4s smooth %.0f' % (name, 'bf16' if bf16 else 'f32', smooth), got, dice_reference(name, bf16, smooth), bf16)


@pytest.mark.parametrize('gamma', [2.0, 0.5])
def test_focal_fixture_reproduces_the_recorded_reference(golden_dir, gamma):
    """The reference's own f32 loss and gradient (tests/golden/focal.npz), default variant."""
    g = cases.load_npz(os.path.join(golden_dir, 'focal.npz'))
    logits, target = torch.from_numpy(g['logits']), torch.from_numpy(g['target'])
    want_loss, want_grad = float(g['gamma%s/loss' % gamma]), g['gamma%s/grad' % gamma]
    _, g64 = R.loss_and_grad(R.focal_loss, logits, target, torch.float64, ALPHA, gamma, 255, 'reference')
    d_ref = cases.rel_err(want_grad, g64.numpy())
    loss, grad = hip_focal(logits, target, gamma, 'reference')
    d_loss, d_grad = abs(float(loss) / want_loss - 1), cases.rel_err(grad.numpy(), want_grad)
    print('focal fixture gamma %s: loss rel %.2e | grad d_ref %.2e hip-vs-recorded %.2e' % (gamma, d_loss, d_ref, d_grad))
    assert d_loss <= 1e-5
    assert d_grad <= max(2e-5, 3 * d_ref)


@functools.lru_cache(maxsize=None)
def saturated_input():
    """'sub_wave' with three pixel groups rewritten: the target's logit 40 and 200 above the other classes, and 40 below."""
    logits, target = (t.clone() for t in case_input('sub_wave', False))
    B, C, H, W = logits.shape
    logits = 0.5 * logits
    for row, delta in ((1, 40.0), (2, 200.0), (3, -40.0)):
        t = target[0, row]
        ok = (t >= 0) & (t < C)
        assert int(ok.sum()) >= 16
        cols = torch.nonzero(ok).flatten()
        logits[0, t[cols], row, cols] += delta
    return logits, target


@pytest.mark.parametrize('variant', R.FOCAL_VARIANTS)
@pytest.mark.parametrize('gamma', [0.5, 1.0, 2.0])
def test_focal_saturated_pixels_have_a_finite_and_correct_gradient(gamma, variant):
    logits, target = saturated_input()
    want = reference(R.focal_loss, logits, target, ALPHA, gamma, 255, variant)
    assert np.isfinite(want[1]).all()
    got = hip_focal(logits, target, gamma, variant)
    check('focal saturated g%.1f %-9s' % (gamma, variant), got, want, False)


@DTYPES
def test_all_ignored_target_gives_zero_loss_and_zero_gradient(dtype):
    logits, _ = case_input('sub_wave', False)
    for target in (torch.full((2, 8, 24), 255), torch.full((2, 8, 24), -1)):
        for variant in R.FOCAL_VARIANTS:
            loss, grad = hip_focal(logits, target, 2.0, variant, dtype)
            assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0
        for smooth in (1.0, 0.0):
            loss, grad = hip_dice(logits, target, 19, smooth, dtype)
            assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


@pytest.mark.parametrize('name', ['sub_wave', 'two_blocks'])
def test_two_calls_are_bit_identical(name):
    C = CASES[name][1]
    logits, target = case_input(name, False)
    for fn in (lambda: hip_focal(logits, target, 2.0, 'reference'), lambda: hip_focal(logits, target, 0.5, 'lin'),
               lambda: hip_dice(logits, target, C, 1.0)):
        a, b = fn(), fn()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_block_cap_changes_the_grid_not_the_result():
    """480 pixel groups: the default grid is two blocks (two partial rows).  Capped at 1 block the kernels take two
    grid-stride trips and write one row; capped at 3 the cap is not reached.  Every setting meets the bounds against the f64
    restatement, and the capped results agree with the default's to the summation order (loss 1e-6, gradient 1e-6)."""
    from torch_semantic_segmentation_amd import ops
    name = 'two_blocks'
    C = CASES[name][1]
    logits, target = case_input(name, False)
    lib = ops.N.lib()
    assert ops.softloss_max_blocks == 0
    B, _, H, W = logits.shape
    row = 3 * C * 8
    coef = lib.tss_dice_workspace_bytes(B, C, H * W, 1) - row
    assert lib.tss_dice_workspace_bytes(B, C, H * W, 0) == coef + 2 * row        # the coefficients come out of two rows
    assert lib.tss_dice_workspace_bytes(B, C, H * W, 3) == coef + 2 * row
    assert lib.tss_focal_workspace_bytes(B, H * W, 0) == 2 * 16 and lib.tss_focal_workspace_bytes(B, H * W, 1) == 16
    base_f, base_d = hip_focal(logits, target, 2.0, 'reference'), hip_dice(logits, target, C, 1.0)
    try:
        for cap in (1, 3):
            ops.softloss_max_blocks = cap
            got_f, got_d = hip_focal(logits, target, 2.0, 'reference'), hip_dice(logits, target, C, 1.0)
            check('focal cap %d' % cap, got_f, focal_reference(name, False, 2.0, 'reference'), False)
            check('dice  cap %d' % cap, got_d, dice_reference(name, False, 1.0), False)
            for got, base in ((got_f, base_f), (got_d, base_d)):
                assert abs(float(got[0]) / float(base[0]) - 1) <= 1e-6
                assert cases.rel_err(got[1].numpy(), base[1].numpy()) <= 1e-6
    finally:
        ops.softloss_max_blocks = 0


def test_grad_out_is_honoured():
    name = 'sub_wave'
    logits, target = case_input(name, False)
    for run, want in ((lambda s: hip_focal(logits, target, 2.0, 'reference', scale=s), focal_reference(name, False, 2.0, 'reference')),
                      (lambda s: hip_dice(logits, target, 19, 1.0, scale=s), dice_reference(name, False, 1.0))):
        loss, grad = run(None)
        loss7, grad7 = run(0.7)
        assert torch.equal(loss, loss7)
        # the scale enters before the one rounding to f32: 0.7f * grad differs by an ulp or two
        assert cases.rel_err(grad7.numpy(), 0.7 * grad.double().numpy()) <= 1e-6
        assert cases.rel_err(grad7.numpy(), 0.7 * want[1]) <= grad_bound(False, want[2])


def test_alpha_scales_the_focal_loss():
    logits, target = case_input('sub_wave', False)
    a, b = hip_focal(logits, target, 2.0, 'lin', alpha=0.25), hip_focal(logits, target, 2.0, 'lin', alpha=1.0)
    assert abs(float(b[0]) / (4 * float(a[0])) - 1) <= 1e-6
    assert cases.rel_err(b[1].numpy(), 4 * a[1].double().numpy()) <= 1e-6


def test_ignore_index_none_keeps_every_in_range_pixel():
    """The labels 255 are out of range for 19 classes, so they stay out with ignore_index=None too; an in-range
    ignore_index drops that class's pixels, None keeps them."""
    logits, target = case_input('sub_wave', False)
    for ignore in (None, 4):
        want = reference(R.focal_loss, logits, target, ALPHA, 2.0, ignore, 'reference')
        check('focal ignore %s' % ignore, hip_focal(logits, target, 2.0, 'reference', ignore=ignore), want, False)
        want = reference(R.dice_loss, logits, target, 19, 1.0, ignore)
        check('dice  ignore %s' % ignore, hip_dice(logits, target, 19, 1.0, ignore=ignore), want, False)


@functools.lru_cache(maxsize=None)
def many_class_input(bf16):
    """2x50x48x48: 576 pixel groups (three blocks by default, the third ragged), 50 classes = three register sweeps of 24."""
    g = torch.Generator().manual_seed(77)
    logits = 2.0 * torch.randn(2, 50, 48, 48, generator=g)
    if bf16:
        logits = logits.bfloat16().float()
    target = torch.randint(0, 50, (2, 48, 48), generator=g)
    target[torch.rand(2, 48, 48, generator=g) < 0.1] = 255
    return logits, target


@functools.lru_cache(maxsize=None)
def many_class_reference(bf16):
    return reference(R.dice_loss, *many_class_input(bf16), 50, 1.0, 255)


@pytest.mark.parametrize('cap', [0, 1, 2])
@DTYPES
def test_dice_with_more_classes_than_one_register_sweep(dtype, cap):
    """C = 50: the per-class sums take three sweeps of 24 classes, the last one ragged, the lse read back on the second and
    third.  Default grid: three partial rows; capped at 1 block: three grid-stride trips per sweep and one row; at 2: two
    rows, the first block with two trips."""
    from torch_semantic_segmentation_amd import ops
    bf16 = dtype == torch.bfloat16
    logits, target = many_class_input(bf16)
    lib = ops.N.lib()
    rows = {0: 3, 1: 1, 2: 2}[cap]
    assert lib.tss_dice_workspace_bytes(2, 50, 48 * 48, cap) == 512 + rows * 3 * 50 * 8
    assert ops.softloss_max_blocks == 0
    try:
        ops.softloss_max_blocks = cap
        got = hip_dice(logits, target, 50, 1.0, dtype)
    finally:
        ops.softloss_max_blocks = 0
    check('dice  C=50 %-4s cap %d' % ('bf16' if bf16 else 'f32', cap), got, many_class_reference(bf16), bf16)


def test_module_defaults_and_argument_errors():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    m = tssa.FocalLoss()
    assert (m.alpha, m.gamma, m.ignore_index, m.variant) == (0.25, 2.0, None, 'reference')
    d = tssa.DiceLoss(19)
    assert (d.num_classes, d.smooth, d.ignore_index) == (19, 1.0, -100)
    logits, target = case_input('sub_wave', False)
    x, t = logits.to(DEV), target.to(DEV)
    want = tssa.focal_loss(x, t, ignore_index=255)
    assert torch.equal(tssa.FocalLoss(ignore_index=255)(x, t), want)
    assert torch.equal(tssa.FocalFn.apply(x, t, 0.25, 2.0, 255, 'reference'), want)
    assert torch.equal(tssa.FocalLoss()(x, t), tssa.focal_loss(x, t, ignore_index=None))
    want = tssa.dice_loss(x, t, 19, ignore_index=255)
    assert torch.equal(tssa.DiceLoss(19, ignore_index=255)(x, t), want)
    assert torch.equal(tssa.DiceFn.apply(x, t, 1.0, 255), want)
    with pytest.raises(ValueError):
        tssa.focal_loss(x, t, variant='berman')
    with pytest.raises(ValueError):
        tssa.FocalLoss(variant='published')
    with pytest.raises(ValueError):
        tssa.focal_loss(x, t, gamma=-0.5)
    with pytest.raises(ValueError):
        tssa.dice_loss(x, t, 18)
    with pytest.raises(ValueError):
        tssa.DiceLoss(20)(x, t)
    with pytest.raises(NotImplementedError):
        tssa.dice_loss(torch.zeros(1, 257, 2, 8, device=DEV), torch.zeros(1, 2, 8, dtype=torch.int64, device=DEV), 257)
    for fn in (lambda a, b: tssa.focal_loss(a, b), lambda a, b: tssa.dice_loss(a, b, 19)):
        with pytest.raises(NotImplementedError):
            fn(x[:, :, :3, :5].contiguous(), t[:, :3, :5].contiguous())
    # the C side refuses the same arguments with TSS_ERR_SHAPE (-2) before it launches anything
    lib, ptr = ops.N.lib(), ops.N.ptr
    B, C, H, W = x.shape
    lse, coef = torch.empty(B, H, W, device=DEV), torch.empty(B, H, W, device=DEV)
    ws, out = torch.empty(4096, dtype=torch.uint8, device=DEV), torch.empty(2, device=DEV)
    st = ops.N.stream()
    assert lib.tss_focal_fwd(ptr(x), ptr(t), ptr(lse), ptr(coef), ptr(ws), ptr(out[0:1]), ptr(out[1:2]), B, C, H * W, 255, 1,
                             0.25, -0.5, 0, 0, 0, st) == -2
    assert lib.tss_focal_fwd(ptr(x), ptr(t), ptr(lse), ptr(coef), ptr(ws), ptr(out[0:1]), ptr(out[1:2]), B, C, H * W, 255, 1,
                             0.25, 2.0, 2, 0, 0, st) == -2
    assert lib.tss_dice_fwd(ptr(x), ptr(t), ptr(lse), ptr(ws), ptr(out[0:1]), B, 257, H * W, 255, 1, 1.0, 0, 0, st) == -2
    assert lib.tss_dice_workspace_bytes(B, 257, H * W, 0) == 0 and lib.tss_dice_workspace_bytes(B, 256, H * W, 0) > 0
    assert lib.tss_dice_fwd(ptr(x), ptr(t), ptr(lse), ptr(ws), ptr(out[0:1]), B, C, H * W + 4, 255, 1, 1.0, 0, 0, st) == -2


@pytest.mark.parametrize('which', ['focal', 'dice'])
def test_trainer_runs_the_loss_eagerly_and_as_a_captured_graph(which):
    """Trainer(model, opt, FocalLoss / DiceLoss) takes the unfused model(x) -> loss_fn path; the step is captured in a HIP
    graph and gives the eager trajectory (bound: test_flat_adamw_and_graph_replay_match_eager's)."""
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
        loss_fn = tssa.FocalLoss(ignore_index=255) if which == 'focal' else tssa.DiceLoss(19, ignore_index=255)
        tr = E.Trainer(m, opt, loss_fn, use_graph=use_graph)
        assert not tr.fuse_head_loss
        results.append([tr.step_async(x, y).item() for _ in range(2)])
        assert bool(tr._graphs) == use_graph and tr.use_graph == use_graph
    assert np.isfinite(results[0]).all() and np.isfinite(results[1]).all()
    assert results[0][0] > 0 and results[0][1] != results[0][0]
    assert np.allclose(results[1], results[0], rtol=1e-3), results
