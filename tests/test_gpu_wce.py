"""Class weights and label smoothing in tssa.cross_entropy (planar kernels, tss_cross_entropy_{fwd,bwd}_ex) and in
tssa.upsample_cross_entropy (the fused head, tss_upsample_ce_fwd_ex) against the f64 restatement of tests/wce_ref.py, which
tests/test_wce_oracle.py pins to F.cross_entropy.

Inputs.  Planar: the cases of tests/test_gpu_softloss.py (sub-wave, two blocks with a ragged second, odd batch with 21 classes, two
classes, almost nothing valid), same seeds.  Fused: the shapes of tests/test_gpu_ops.py::test_fused_upsample_cross_entropy_matches_unfused
that reach a code path each (FUSED below).  Labels carry about 10 % of 255 and a handful of -1 / 300.  Weights: tssa.enet_class_weights
of tssa.label_histogram of the case's own labels (1.4 for a class that fills the image to 50.5 for an absent one), class 1 then set to
exactly 0; the last class is absent from the labels (remapped to class 0) wherever there are more than two classes -- with two classes an
absent class next to a weightless one would leave no pixel that counts, which test_empty_denominator covers.
Combinations: (w, 0), (None, 0.1), (w, 0.1), f32 and bf16; bf16 inputs are bf16-exact and the restatement reads the same values.

Bounds (those of tests/test_gpu_softloss.py and tests/test_gpu_ops.py).  Loss: relative 2e-5.  Gradient, f32: cases.rel_err <=
max(2e-5, 3 d_ref), d_ref the restatement's own f32-vs-f64 distance on that input.  Gradient, bf16: 2e-2 (stored in bf16).
"""
import functools

import pytest
import torch

from oracle.recipe import formula_state, synthetic_batch
from tests import cases, wce_ref as R
from tests.test_gpu_softloss import CASES, case_input

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 0.1
DTYPES = pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
COMBOS = pytest.mark.parametrize('weighted,eps', [(True, 0.0), (False, EPS), (True, EPS)], ids=['w', 'eps', 'w_eps'])

#          low-res shape,    scale   path reached
FUSED = {
    'base':       ((2, 19, 8, 16), 8),      # CP = 20
    'edge':       ((1, 19, 5, 7), 8),       # lanes past the image edge, odd rows
    'few_class':  ((2, 5, 6, 4), 4),        # pad classes in play
    'cp24':       ((1, 21, 40, 33), 8),     # CP = 24 instance, two strips with an 8-lane second, several bands
    'bands':      ((3, 19, 70, 36), 2),     # several bands, odd batch
    'scale1':     ((1, 19, 9, 300), 1),     # a flush every row, rB == rA at the end
}


# an output that is no multiple of the map and nearly equal to it: the row tap moves on almost every output row, 32 of 256 lanes in use
NEAR = ((1, 19, 15, 29), (16, 32))


def drop_last_class(target, C):
    if C > 2:
        target[target == C - 1] = 0
    return target


def class_weights(target, C):
    """The ENet weights of the labels' own histogram, by the package's device functions; class 1 weightless."""
    import torch_semantic_segmentation_amd as tssa
    counts = tssa.label_histogram(target.to(DEV), C, ignore_index=255)
    w = tssa.enet_class_weights(counts).cpu()
    assert w.dtype == torch.float32 and w.shape == (C,)
    if C > 2:
        assert int(counts[C - 1]) == 0 and float(w.max()) > 50.0
    assert 1.0 < float(w.min()) and int(counts.sum()) > 0
    w[1] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def planar_input(name, bf16):
    logits, target = case_input(name, bf16)
    C = CASES[name][1]
    target = drop_last_class(target.clone(), C)
    assert (target == 255).sum() > 0 and (target == -1).sum() == 3 and (target == 300).sum() == 2
    return logits, target, class_weights(target, C)


def labelled_input(shape, size, seed, bf16):
    """(low-resolution logits, labels of `size` with about 10 % of 255, three -1 and two 300, class weights) from one seed."""
    B, C, h, w = shape
    H, W = size
    g = torch.Generator().manual_seed(seed)
    low = 2.0 * torch.randn(B, C, h, w, generator=g)
    if bf16:
        low = low.bfloat16().float()
    target = torch.randint(0, C, (B, H, W), generator=g)
    target = drop_last_class(target, C)
    target[torch.rand(B, H, W, generator=g) < 0.10] = 255
    flat = target.view(-1)
    flat[[3, 17, 40]] = -1
    flat[[5, 29]] = 300
    return low, target, class_weights(target, C)


@functools.lru_cache(maxsize=None)
def fused_input(name, bf16):
    (B, C, h, w), scale = FUSED[name]
    return labelled_input((B, C, h, w), (h * scale, w * scale), sorted(FUSED).index(name) + 900, bf16)


@functools.lru_cache(maxsize=None)
def near_input(bf16):
    return labelled_input(NEAR[0], NEAR[1], 960, bf16)


def reference(fn, x, target, w, eps):
    """(f64 loss, f64 gradient, d_ref) of a restatement."""
    l64, g64 = R.loss_and_grad(fn, x, target, torch.float64, w, 255, eps)
    _, g32 = R.loss_and_grad(fn, x, target, torch.float32, w, 255, eps)
    d_ref = cases.rel_err(g32.numpy(), g64.numpy()) if bool(torch.isfinite(g32).all()) else None
    return float(l64), g64.numpy(), d_ref


@functools.lru_cache(maxsize=None)
def planar_reference(name, bf16, weighted, eps):
    logits, target, w = planar_input(name, bf16)
    return reference(R.wce_loss, logits, target, w if weighted else None, eps)


@functools.lru_cache(maxsize=None)
def fused_reference(name, bf16, weighted, eps):
    low, target, w = fused_input(name, bf16)
    return reference(R.upsampled_wce_loss, low, target, w if weighted else None, eps)


def grad_bound(bf16, d_ref):
    if bf16:
        return 2e-2
    return 2e-5 if d_ref is None else max(2e-5, 3 * d_ref)


def hip_planar(logits, target, w, eps, dtype=torch.float32, scale=None):
    import torch_semantic_segmentation_amd as tssa
    x = logits.to(DEV).to(dtype).requires_grad_(True)
    loss = tssa.cross_entropy(x, target.to(DEV), 255, weight=None if w is None else w.to(DEV), label_smoothing=eps)
    (loss if scale is None else scale * loss).backward()
    return loss.detach().cpu(), x.grad.detach().float().cpu()


def hip_fused(low, target, w, eps, scale_factor, dtype=torch.float32, scale=None, size=None):
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    a = ops.to_nhwc(low.to(DEV).to(dtype)).clone().requires_grad_(True)
    loss = tssa.upsample_cross_entropy(a, target.to(DEV), scale_factor=scale_factor, size=size, ignore_index=255,
                                       weight=None if w is None else w.to(DEV), label_smoothing=eps)
    (loss if scale is None else scale * loss).backward()
    return loss.detach().cpu(), a.grad.detach().float().cpu()


def check(tag, got, want, bf16):
    (loss, grad), (want_loss, want_grad, d_ref) = got, want
    d_loss = abs(float(loss) / want_loss - 1)
    d_grad = cases.rel_err(grad.numpy(), want_grad)
    bound = grad_bound(bf16, d_ref)
    print('%s loss %.6f rel %.2e | grad d_ref %s hip %.2e bound %.2e'
          % (tag, want_loss, d_loss, 'n/a' if d_ref is None else '%.2e' % d_ref, d_grad, bound))
    assert torch.isfinite(grad).all()
    assert d_loss <= 2e-5
    assert d_grad <= bound


def tag_of(kind, name, bf16, weighted, eps):
    return '%s %-11s %-4s %s eps %.1f' % (kind, name, 'bf16' if bf16 else 'f32', 'w' if weighted else '-', eps)


@COMBOS
@DTYPES
@pytest.mark.parametrize('name', list(CASES))
def test_planar_loss_and_gradient_vs_f64_restatement(name, dtype, weighted, eps):
    bf16 = dtype == torch.bfloat16
    logits, target, w = planar_input(name, bf16)
    got = hip_planar(logits, target, w if weighted else None, eps, dtype)
    check(tag_of('planar', name, bf16, weighted, eps), got, planar_reference(name, bf16, weighted, eps), bf16)


@COMBOS
@DTYPES
@pytest.mark.parametrize('name', list(FUSED))
def test_fused_loss_and_gradient_vs_f64_restatement(name, dtype, weighted, eps):
    bf16 = dtype == torch.bfloat16
    low, target, w = fused_input(name, bf16)
    got = hip_fused(low, target, w if weighted else None, eps, FUSED[name][1], dtype)
    check(tag_of('fused ', name, bf16, weighted, eps), got, fused_reference(name, bf16, weighted, eps), bf16)


@pytest.mark.parametrize('weighted,eps', [(False, 0.0), (True, 0.0), (False, EPS), (True, EPS)], ids=['plain', 'w', 'eps', 'w_eps'])
@DTYPES
def test_fused_output_nearly_the_map_size_vs_f64_restatement(dtype, weighted, eps):
    bf16 = dtype == torch.bfloat16
    low, target, w = near_input(bf16)
    assert (target == 255).sum() > 0 and (target == -1).sum() == 3 and (target == 300).sum() == 2
    got = hip_fused(low, target, w if weighted else None, eps, None, dtype, size=NEAR[1])
    want = reference(R.upsampled_wce_loss, low, target, w if weighted else None, eps)
    check(tag_of('fused ', 'near', bf16, weighted, eps), got, want, bf16)


@pytest.mark.parametrize('name', ['sub_wave', 'two_blocks', 'odd_batch'])
def test_planar_unit_weights_agree_with_the_unweighted_kernels(name):
    logits, target, w = planar_input(name, False)
    want = planar_reference(name, False, False, 0.0)
    plain = hip_planar(logits, target, None, 0.0)
    ones = hip_planar(logits, target, torch.ones_like(w), 0.0)
    check('planar plain %s' % name, plain, want, False)
    check('planar ones  %s' % name, ones, want, False)
    assert abs(float(ones[0]) / float(plain[0]) - 1) <= 2e-5
    assert cases.rel_err(ones[1].numpy(), plain[1].numpy()) <= grad_bound(False, want[2])


@pytest.mark.parametrize('name', ['base', 'few_class', 'cp24', 'scale1'])
def test_fused_unit_weights_agree_with_the_unweighted_kernel(name):
    low, target, w = fused_input(name, False)
    want = fused_reference(name, False, False, 0.0)
    plain = hip_fused(low, target, None, 0.0, FUSED[name][1])
    ones = hip_fused(low, target, torch.ones_like(w), 0.0, FUSED[name][1])
    check('fused plain %s' % name, plain, want, False)
    check('fused ones  %s' % name, ones, want, False)
    assert abs(float(ones[0]) / float(plain[0]) - 1) <= 2e-5
    assert cases.rel_err(ones[1].numpy(), plain[1].numpy()) <= grad_bound(False, want[2])


@pytest.mark.parametrize('name', ['sub_wave', 'two_blocks'])
def test_planar_defaults_call_the_old_entries_bit_for_bit(name):
    """weight=None, label_smoothing=0 through the Python API == tss_cross_entropy_fwd / _bwd called directly.  (At most two blocks add
    into the zeroed f64 accumulator, and a + b == b + a: the old entries' atomics cannot reorder anything here.)"""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import _native as N
    logits, target, _ = planar_input(name, False)
    x, t = logits.to(DEV).requires_grad_(True), target.to(DEV)
    loss = tssa.cross_entropy(x, t, 255, weight=None, label_smoothing=0.0)
    (0.7 * loss).backward()
    assert torch.equal(tssa.CrossEntropyLoss(255)(x.detach(), t), loss.detach())
    B, C, H, W = logits.shape
    xd = x.detach()
    lse, acc, scal = torch.empty(B, H, W, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV), torch.empty(2, device=DEV)
    N.call('tss_cross_entropy_fwd', N.ptr(xd), N.ptr(t), N.ptr(lse), N.ptr(acc), N.ptr(scal[0:1]), N.ptr(scal[1:2]), B, C, H * W, 255,
           N.dtype_code(xd.dtype), N.stream())
    d, gout = torch.empty_like(xd), torch.tensor([0.7], device=DEV)
    N.call('tss_cross_entropy_bwd', N.ptr(xd), N.ptr(t), N.ptr(lse), N.ptr(scal[1:2]), N.ptr(gout), N.ptr(d), B, C, H * W, 255,
           N.dtype_code(xd.dtype), N.stream())
    assert torch.equal(scal[0], loss.detach()) and torch.equal(d, x.grad)


@DTYPES
@pytest.mark.parametrize('name', ['base', 'cp24'])
def test_fused_defaults_call_the_old_entry_bit_for_bit(name, dtype):
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import _native as N, ops
    low, target, _ = fused_input(name, dtype == torch.bfloat16)
    (B, C, h, w), scale = FUSED[name]
    H, W = h * scale, w * scale
    a, t = ops.to_nhwc(low.to(DEV).to(dtype)).clone().requires_grad_(True), target.to(DEV)
    loss = tssa.upsample_cross_entropy(a, t, scale_factor=scale, ignore_index=255, weight=None, label_smoothing=0.0)
    (0.7 * loss).backward()
    ad = ops.to_nhwc(a.detach())
    ws = torch.empty(N.lib().tss_upsample_ce_ws(B, C, h, w, H, W), device=DEV)
    scal = torch.empty(2, device=DEV)
    N.call('tss_upsample_ce_fwd', N.ptr(ad), ad.stride(3), N.ptr(t), N.ptr(ws), N.ptr(scal[0:1]), N.ptr(scal[1:2]),
           B, C, h, w, H, W, 255, N.dtype_code(ad.dtype), N.stream())
    out = torch.empty((B, h, w, ad.stride(3)), dtype=ad.dtype, device=DEV)
    gout = torch.tensor([0.7], device=DEV)
    N.call('tss_upsample_ce_bwd', N.ptr(ws), N.ptr(scal[1:2]), N.ptr(gout), N.ptr(out), ad.stride(3), B, C, h, w, H, W,
           N.dtype_code(ad.dtype), N.stream())
    assert torch.equal(scal[0], loss.detach()) and torch.equal(out.permute(0, 3, 1, 2)[:, :C], a.grad)


@pytest.mark.parametrize('eps', [0.0, EPS])
def test_scaling_the_weights_by_four_changes_nothing(eps):
    """4 w is exact in f32 and the loss is homogeneous of degree 0 in w: the same bounds against the same reference, and the two
    evaluations agree with each other within them."""
    for kind, name in (('planar', 'two_blocks'), ('planar', 'odd_batch'), ('fused', 'base'), ('fused', 'cp24')):
        if kind == 'planar':
            x, target, w = planar_input(name, False)
            want = planar_reference(name, False, True, eps)
            one, four = hip_planar(x, target, w, eps), hip_planar(x, target, 4 * w, eps)
        else:
            x, target, w = fused_input(name, False)
            want = fused_reference(name, False, True, eps)
            one, four = hip_fused(x, target, w, eps, FUSED[name][1]), hip_fused(x, target, 4 * w, eps, FUSED[name][1])
        check('%s %s 4w eps %.1f' % (kind, name, eps), four, want, False)
        assert abs(float(four[0]) / float(one[0]) - 1) <= 2e-5
        assert cases.rel_err(four[1].numpy(), one[1].numpy()) <= grad_bound(False, want[2])


@COMBOS
def test_two_evaluations_are_bit_identical(weighted, eps):
    for name in ('sub_wave', 'two_blocks', 'odd_batch'):
        logits, target, w = planar_input(name, False)
        a, b = (hip_planar(logits, target, w if weighted else None, eps, scale=0.7) for _ in range(2))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for name in ('base', 'cp24', 'bands'):
        low, target, w = fused_input(name, False)
        a, b = (hip_fused(low, target, w if weighted else None, eps, FUSED[name][1], scale=0.7) for _ in range(2))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@COMBOS
@DTYPES
@pytest.mark.parametrize('name', list(FUSED))
def test_fused_pass_writes_every_workspace_element_that_the_gather_reads(name, dtype, weighted, eps):
    """Through the C ABI with a NaN-filled workspace and a NaN-filled gradient: finite, equal to the autograd path, pad channels 0."""
    from torch_semantic_segmentation_amd import _native as N, ops
    low, target, w = fused_input(name, dtype == torch.bfloat16)
    (B, C, h, wd), scale = FUSED[name]
    H, W = h * scale, wd * scale
    want_loss, want_grad = hip_fused(low, target, w if weighted else None, eps, scale, dtype, scale=0.7)
    ad, t = ops.to_nhwc(low.to(DEV).to(dtype)), target.to(DEV)          # the padded pitch (a clone would drop it)
    wdev = w.to(DEV) if weighted else None
    ws = torch.full((N.lib().tss_upsample_ce_ws(B, C, h, wd, H, W),), float('nan'), device=DEV)
    scal = torch.full((2,), float('nan'), device=DEV)
    N.call('tss_upsample_ce_fwd_ex', N.ptr(ad), ad.stride(3), N.ptr(t), N.ptr(wdev), eps, N.ptr(ws), N.ptr(scal[0:1]), N.ptr(scal[1:2]),
           B, C, h, wd, H, W, 255, N.dtype_code(ad.dtype), N.stream())
    out = torch.full((B, h, wd, ad.stride(3)), float('nan'), dtype=ad.dtype, device=DEV)
    gout = torch.tensor([0.7], device=DEV)
    N.call('tss_upsample_ce_bwd', N.ptr(ws), N.ptr(scal[1:2]), N.ptr(gout), N.ptr(out), ad.stride(3), B, C, h, wd, H, W,
           N.dtype_code(ad.dtype), N.stream())
    assert torch.isfinite(out.float()).all() and torch.isfinite(scal).all()
    assert torch.equal(scal[0].cpu(), want_loss)
    assert torch.equal(out.permute(0, 3, 1, 2)[:, :C].float().cpu(), want_grad)
    assert (out[..., C:] == 0).all()


@pytest.mark.parametrize('eps', [0.0, EPS])
@DTYPES
def test_empty_denominator_gives_nan_and_a_zero_gradient(dtype, eps):
    """No valid pixel, and valid pixels whose class weight is 0 (class 1), planar and fused."""
    bf16 = dtype == torch.bfloat16
    logits, target, w = planar_input('sub_wave', bf16)
    low, ftarget, fw = fused_input('base', bf16)
    for fill in (255, 1):
        t = torch.where(target == 255, target, torch.full_like(target, fill))
        loss, grad = hip_planar(logits, t, w, eps, dtype)
        assert torch.isnan(loss) and float(grad.abs().max()) == 0.0
        t = torch.where(ftarget == 255, ftarget, torch.full_like(ftarget, fill))
        loss, grad = hip_fused(low, t, fw, eps, 8, dtype)
        assert torch.isnan(loss) and float(grad.abs().max()) == 0.0
    if eps > 0:
        loss, grad = hip_planar(logits, torch.full_like(target, 255), None, eps, dtype)
        assert torch.isnan(loss) and float(grad.abs().max()) == 0.0
        loss, grad = hip_fused(low, torch.full_like(ftarget, 255), None, eps, 8, dtype)
        assert torch.isnan(loss) and float(grad.abs().max()) == 0.0


def test_fallback_outside_the_fused_envelope_passes_both_arguments_on():
    """C = 26 > 24: upsample_cross_entropy takes upsample_logits + the planar kernels, with the weights and the smoothing."""
    g = torch.Generator().manual_seed(41)
    low = 2.0 * torch.randn(1, 26, 4, 8, generator=g)
    target = torch.randint(0, 26, (1, 8, 16), generator=g)
    target[torch.rand(1, 8, 16, generator=g) < 0.1] = 255
    w = torch.rand(26, generator=g) * 49 + 1
    want = reference(R.upsampled_wce_loss, low, target, w, EPS)
    check('fallback C=26', hip_fused(low, target, w, EPS, 2), want, False)


def test_module_buffer_and_argument_errors():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import _native as N, ops
    logits, target, w = planar_input('sub_wave', False)
    x, t = logits.to(DEV), target.to(DEV)
    m = tssa.CrossEntropyLoss(255)
    assert (m.ignore_index, m.weight, m.label_smoothing) == (255, None, 0.0) and 'weight' in m._buffers
    m = tssa.CrossEntropyLoss(255, weight=w.double().repeat_interleave(2)[::2], label_smoothing=EPS)     # f64, strided: kept as f32 (C,)
    assert m.weight.dtype == torch.float32 and m.weight.shape == (19,) and m.weight.is_contiguous() and not m.weight.is_cuda
    assert 'weight' in dict(m.named_buffers()) and not m.weight.requires_grad
    m = m.to(DEV)
    assert m.weight.is_cuda
    assert torch.equal(m(x, t), tssa.cross_entropy(x, t, 255, weight=w.to(DEV), label_smoothing=EPS))
    for bad in (dict(weight=w[:18].to(DEV)), dict(weight=w), dict(label_smoothing=-0.1), dict(label_smoothing=1.5),
                dict(weight=torch.arange(19, device=DEV))):
        with pytest.raises(ValueError):
            tssa.cross_entropy(x, t, 255, **bad)
        with pytest.raises(ValueError):
            tssa.upsample_cross_entropy(ops.to_nhwc(x), torch.zeros(2, 16, 48, dtype=torch.int64, device=DEV), scale_factor=2,
                                        ignore_index=255, **bad)
    with pytest.raises(ValueError):
        tssa.CrossEntropyLoss(255, label_smoothing=2.0)
    with pytest.raises(ValueError):
        tssa.CrossEntropyLoss(255, weight=torch.arange(19))
    # the C side: more than 24 classes are outside the fused pass, a smoothing outside [0, 1] outside every new entry
    lib, ptr, st = N.lib(), N.ptr, N.stream()
    big = torch.zeros(1, 4, 8, 32, device=DEV)
    tt = torch.zeros(1, 8, 16, dtype=torch.int64, device=DEV)
    ws, scal = torch.empty(4096, device=DEV), torch.empty(2, device=DEV)
    assert lib.tss_upsample_ce_fwd_ex(ptr(big), 32, ptr(tt), None, 0.0, ptr(ws), ptr(scal[0:1]), ptr(scal[1:2]), 1, 25, 4, 8, 8, 16, 255,
                                      0, st) == -2
    assert lib.tss_upsample_ce_fwd_ex(ptr(big), 32, ptr(tt), None, 1.5, ptr(ws), ptr(scal[0:1]), ptr(scal[1:2]), 1, 19, 4, 8, 8, 16, 255,
                                      0, st) == -2
    B, C, H, W = x.shape
    lse, rows = torch.empty(B, H, W, device=DEV), torch.empty(64, 2, dtype=torch.float64, device=DEV)
    assert lib.tss_cross_entropy_ex_rows(B, H * W) == 1 and lib.tss_cross_entropy_ex_rows(B, H * W + 4) == 0
    assert lib.tss_cross_entropy_fwd_ex(ptr(x), ptr(t), None, -0.5, ptr(lse), ptr(rows), ptr(scal[0:1]), ptr(scal[1:2]), B, C, H * W, 255,
                                        0, st) == -2
    assert lib.tss_cross_entropy_bwd_ex(ptr(x), ptr(t), None, 0.1, ptr(lse), ptr(scal[1:2]), None, ptr(torch.empty_like(x)), B, C,
                                        H * W + 4, 255, 0, st) == -2


# ----------------------------------------------------------------------------- Trainer (FastSCNN, bf16, 2 x 3 x 64 x 128)

def student():
    import torch_semantic_segmentation_amd as tssa
    m = cases.product_model('fastscnn')
    m.load_state_dict(formula_state(m), strict=True)
    cases.zero_dropout(m)
    m.to(DEV)
    tssa.set_compute_dtype(m, torch.bfloat16)
    return m


def batch():
    x, y = synthetic_batch(2, 64, 128)
    return x.to(DEV), y.to(DEV)


def weighted_loss(y):
    import torch_semantic_segmentation_amd as tssa
    w = tssa.enet_class_weights(tssa.label_histogram(y, 19, ignore_index=255))
    return tssa.CrossEntropyLoss(255, weight=w, label_smoothing=EPS).to(DEV)


def trainer(m, loss_fn, use_graph=False):
    from torch_semantic_segmentation_amd import engine as E
    opt = E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
    return E.Trainer(m, opt, loss_fn, use_graph=use_graph)


def test_trainer_eager_step_is_the_fused_weighted_head_loss():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    x, y = batch()
    loss_fn = weighted_loss(y)
    tr = trainer(student(), loss_fn)
    assert tr.fuse_head_loss
    got = tr.step_async(x, y)
    m2 = student()
    m2.train()
    shadows = ops.WeightShadows(m2)
    shadows.refresh()
    with shadows:
        low = ops.materialize(m2.forward_lowres(x)).detach()
    want = tssa.upsample_cross_entropy(low, y, scale_factor=m2.logit_scale, ignore_index=255, weight=loss_fn.weight, label_smoothing=EPS)
    plain = tssa.upsample_cross_entropy(low, y, scale_factor=m2.logit_scale, ignore_index=255)
    print('step %.6f by hand %.6f unweighted %.6f' % (float(got), float(want), float(plain)))
    assert torch.equal(got, want) and float(want) > 0 and float(want) != float(plain)


def run_steps(use_graph, zero_class_after=None, steps=3):
    x, y = batch()
    m = student()
    loss_fn = weighted_loss(y)
    tr = trainer(m, loss_fn, use_graph=use_graph)
    assert tr.fuse_head_loss
    losses = []
    for i in range(steps):
        if i == zero_class_after:
            with torch.no_grad():
                loss_fn.weight[int(y[(y >= 0) & (y < 19)].flatten()[0])] *= 0          # in place: the captured step reads this buffer
        losses.append(tr.step_async(x, y).clone())
    assert bool(tr._graphs) == use_graph
    return torch.stack(losses).cpu(), torch.cat([p.detach().flatten() for p in m.parameters()]).cpu()


def test_trainer_three_captured_steps_equal_three_eager_steps():
    eager, graph = run_steps(False), run_steps(True)
    print('losses eager %s graph %s' % (eager[0].tolist(), graph[0].tolist()))
    assert bool(torch.isfinite(eager[0]).all()) and float(eager[0][1]) != float(eager[0][0])
    assert torch.equal(eager[0], graph[0])
    assert torch.equal(eager[1], graph[1])


def test_trainer_weight_update_between_replays_needs_no_recapture():
    """The weight of a class that is present goes to 0, in place, between the second and the third replay: the replayed loss is the
    one an eager trainer gives after the same update, and not the one of an untouched weight."""
    untouched = run_steps(False)
    eager, graph = run_steps(False, zero_class_after=2), run_steps(True, zero_class_after=2)
    print('losses untouched %s eager %s graph %s' % (untouched[0].tolist(), eager[0].tolist(), graph[0].tolist()))
    assert torch.equal(eager[0][:2], untouched[0][:2]) and float(eager[0][2]) != float(untouched[0][2])
    assert torch.equal(graph[0], eager[0])
    assert torch.equal(graph[1], eager[1])


def test_trainer_unfused_weighted_loss_is_captured_like_the_eager_step():
    """fuse_head_loss=False: model(x) -> the planar weighted kernels, forward and backward inside the captured step.  f32 model, the
    bound of tests/test_gpu_softloss.py::test_trainer_runs_the_loss_eagerly_and_as_a_captured_graph."""
    import numpy as np
    from torch_semantic_segmentation_amd import engine as E
    x, y = batch()
    results = []
    for use_graph in (False, True):
        m = cases.product_model('fastscnn')
        m.load_state_dict(formula_state(m), strict=True)
        cases.zero_dropout(m)
        m.to(DEV)
        tr = E.Trainer(m, E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5), weighted_loss(y), use_graph=use_graph,
                       fuse_head_loss=False)
        assert not tr.fuse_head_loss
        results.append([tr.step_async(x, y).item() for _ in range(2)])
        assert bool(tr._graphs) == use_graph
    assert np.isfinite(results[0]).all() and np.isfinite(results[1]).all()
    assert results[0][0] > 0 and results[0][1] != results[0][0]
    assert np.allclose(results[1], results[0], rtol=1e-3), results
