"""GPU: tssa.upsample_focal_loss and tssa.upsample_dice_loss (csrc/softhead.hip, the MODE 5 instance of csrc/widehead.hip): the focal
and the soft Dice loss of the bilinearly upsampled logits, computed from the low-resolution logits.

Reference (imported, not restated): tests/softloss_ref.py's focal_loss / dice_loss applied to tests/wce_ref.py's upsample of the
low-resolution logits, run in f64 through softloss_ref.loss_and_grad, and once in f32 for d_ref (tests/test_gpu_softloss.py's
`reference`).  Bounds, by tests/test_gpu_wce.py's `check`: loss relative 2e-5; gradient w.r.t. the low-resolution logits, f32:
cases.rel_err <= max(2e-5, 3 d_ref), the floor alone where the f32 restatement is not finite; bf16: 2e-2.

Geometries of the register kernels: the FUSED table of tests/test_gpu_wce.py with its fused_input (CP 20 and 24 instances, lanes past
the image edge, two strips, several bands, scale 1 with rB == rA at the end, pad classes), plus EXTRA below: two classes, 99.5 % of
the labels ignored, one class absent, an output size that is no multiple of the map (15 x 29 -> 16 x 32).
Wide route: c25, c33, edge, strips, scale1, c256 of tests/test_gpu_widehead.py's WIDE.
Labels as there: about 10 % of 255, three -1, two 300.  Every call is made twice and must give the same bits.
"""
import functools

import pytest
import torch

from tests import cases, softloss_ref as R, wce_ref as U
from tests.test_gpu_softloss import reference, saturated_input
from tests.test_gpu_wce import FUSED, check, fused_input
from tests.test_gpu_widehead import WIDE, wide_input

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ALPHA = 0.25
GAMMAS = (0.0, 0.5, 2.0)
DTYPES = pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])

#             low-res shape, scale, fraction of label 255, absent class
EXTRA = {
    'tiny':      ((2, 2, 4, 4), 2, 0.10, None),       # the smallest class count
    'few_valid': ((2, 19, 8, 16), 8, 0.995, None),    # almost nothing counts
    'absent':    ((1, 5, 6, 9), 4, 0.10, 3),          # class 3 absent; 36 columns: lanes past the edge
    # an output SIZE, no multiple of the map and nearly equal to it; the name sorts last, so the seeds of the cases above stay
    'uneven':    ((1, 19, 15, 29), (16, 32), 0.10, None),
}
REGISTER = list(FUSED) + list(EXTRA)
WIDE_NAMES = ['c25', 'c33', 'edge', 'strips', 'scale1', 'c256']


@functools.lru_cache(maxsize=None)
def head_input(name, bf16):
    """(low-resolution logits, labels, scale) of a register-path case."""
    if name in FUSED:
        low, target, _ = fused_input(name, bf16)
        return low, target, FUSED[name][1]
    (B, C, h, w), scale, frac, absent = EXTRA[name]
    g = torch.Generator().manual_seed(sorted(EXTRA).index(name) + 2900)
    low = 2.0 * torch.randn(B, C, h, w, generator=g)
    if bf16:
        low = low.bfloat16().float()
    H, W = scale if isinstance(scale, tuple) else (h * scale, w * scale)
    target = torch.randint(0, C, (B, H, W), generator=g)
    if absent is not None:
        target[target == absent] = (absent + 1) % C
    target[torch.rand(B, H, W, generator=g) < frac] = 255
    flat = target.view(-1)
    flat[[3, 17, 40]] = -1
    flat[[5, 29]] = 300
    return low, target, scale


@functools.lru_cache(maxsize=None)
def wide_head_input(name, bf16):
    low, target, _ = wide_input(name, bf16)
    return low, target, WIDE[name][1]


def up_focal(low, target, *args):
    return R.focal_loss(U.upsample(low, tuple(target.shape[-2:])), target, *args)


def up_dice(low, target, *args):
    return R.dice_loss(U.upsample(low, tuple(target.shape[-2:])), target, *args)


@functools.lru_cache(maxsize=None)
def focal_reference(name, bf16, gamma, variant, wide=False, ignore=255):
    low, target, _ = (wide_head_input if wide else head_input)(name, bf16)
    return reference(up_focal, low, target, ALPHA, gamma, ignore, variant)


@functools.lru_cache(maxsize=None)
def dice_reference(name, bf16, smooth, ignore=255):
    low, target, _ = head_input(name, bf16)
    return reference(up_dice, low, target, low.shape[1], smooth, ignore)


def nhwc(low, dtype):
    from torch_semantic_segmentation_amd import ops
    return ops.to_nhwc(low.to(DEV).to(dtype))


def out_size(scale):
    """the operators' size / scale_factor arguments of a case's scale (an output size where it is a tuple)"""
    return {'size': scale} if isinstance(scale, tuple) else {'scale_factor': scale}


def hip_focal(low, target, scale, gamma, variant, dtype=torch.float32, ignore=255, gscale=None, alpha=ALPHA):
    import torch_semantic_segmentation_amd as tssa
    a = nhwc(low, dtype).clone().requires_grad_(True)
    loss = tssa.upsample_focal_loss(a, target.to(DEV), alpha=alpha, gamma=gamma, ignore_index=ignore, variant=variant, **out_size(scale))
    (loss if gscale is None else gscale * loss).backward()
    return loss.detach().cpu(), a.grad.detach().float().cpu()


def hip_dice(low, target, scale, smooth, dtype=torch.float32, ignore=255, gscale=None):
    import torch_semantic_segmentation_amd as tssa
    a = nhwc(low, dtype).clone().requires_grad_(True)
    loss = tssa.upsample_dice_loss(a, target.to(DEV), low.shape[1], smooth=smooth, ignore_index=ignore, **out_size(scale))
    (loss if gscale is None else gscale * loss).backward()
    return loss.detach().cpu(), a.grad.detach().float().cpu()


def same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ----------------------------------------------------------------------------- 1. register path vs f64

@DTYPES
@pytest.mark.parametrize('name', REGISTER)
def test_focal_register_path_vs_f64_restatement(name, dtype):
    bf16 = dtype == torch.bfloat16
    low, target, scale = head_input(name, bf16)
    assert low.shape[1] <= 24 and (target == 255).sum() > 0 and (target == -1).sum() == 3 and (target == 300).sum() == 2
    for gamma in GAMMAS:
        for variant in R.FOCAL_VARIANTS:
            got = hip_focal(low, target, scale, gamma, variant, dtype)
            check('focal %-9s %-4s g%.1f %-9s' % (name, 'bf16' if bf16 else 'f32', gamma, variant), got,
                  focal_reference(name, bf16, gamma, variant), bf16)
            assert same_bits(got, hip_focal(low, target, scale, gamma, variant, dtype))


@DTYPES
@pytest.mark.parametrize('name', REGISTER)
def test_dice_register_path_vs_f64_restatement(name, dtype):
    bf16 = dtype == torch.bfloat16
    low, target, scale = head_input(name, bf16)
    if name == 'absent':
        assert (target == 3).sum() == 0
    for smooth in (1.0, 0.0):
        got = hip_dice(low, target, scale, smooth, dtype)
        check('dice  %-9s %-4s smooth %.0f' % (name, 'bf16' if bf16 else 'f32', smooth), got, dice_reference(name, bf16, smooth), bf16)
        assert same_bits(got, hip_dice(low, target, scale, smooth, dtype))


# ----------------------------------------------------------------------------- 2. focal, wide route vs f64

@DTYPES
@pytest.mark.parametrize('name', WIDE_NAMES)
def test_focal_wide_route_vs_f64_restatement(name, dtype):
    bf16 = dtype == torch.bfloat16
    low, target, scale = wide_head_input(name, bf16)
    assert low.shape[1] > 24
    for gamma in GAMMAS:
        for variant in R.FOCAL_VARIANTS:
            got = hip_focal(low, target, scale, gamma, variant, dtype)
            check('focal wide %-7s %-4s g%.1f %-9s' % (name, 'bf16' if bf16 else 'f32', gamma, variant), got,
                  focal_reference(name, bf16, gamma, variant, True), bf16)
            assert same_bits(got, hip_focal(low, target, scale, gamma, variant, dtype))


# ----------------------------------------------------------------------------- 3. saturated pixels

@functools.lru_cache(maxsize=None)
def saturated_low(C):
    """Low-resolution logits at scale 1 (the map is the image): tests/test_gpu_softloss.py's saturated_input for 19 classes; for
    more, the same construction -- logits halved, then three rows of pixels with the target's logit 40 and 200 above the other
    classes, and 40 below."""
    if C == 19:
        return saturated_input()
    g = torch.Generator().manual_seed(3100 + C)
    logits = torch.randn(2, C, 8, 24, generator=g)
    target = torch.randint(0, C, (2, 8, 24), generator=g)
    target[torch.rand(2, 8, 24, generator=g) < 0.10] = 255
    flat = target.view(-1)
    flat[[3, 17, 40]] = -1
    flat[[5, 29]] = 300
    for row, delta in ((1, 40.0), (2, 200.0), (3, -40.0)):
        t = target[0, row]
        cols = torch.nonzero((t >= 0) & (t < C)).flatten()
        assert len(cols) >= 16
        logits[0, t[cols], row, cols] += delta
    return logits, target


@pytest.mark.parametrize('variant', R.FOCAL_VARIANTS)
@pytest.mark.parametrize('gamma', [0.5, 1.0, 2.0])
@pytest.mark.parametrize('C', [19, 30], ids=['register', 'wide'])
def test_focal_saturated_pixels_have_a_finite_and_correct_gradient(C, gamma, variant):
    import numpy as np
    low, target = saturated_low(C)
    want = reference(up_focal, low, target, ALPHA, gamma, 255, variant)
    assert np.isfinite(want[1]).all()
    got = hip_focal(low, target, 1, gamma, variant)
    check('focal saturated C=%d g%.1f %-9s' % (C, gamma, variant), got, want, False)


# ----------------------------------------------------------------------------- 4. workspace coverage, through the C ABI

def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device=DEV)


def gather(N, ws, scale, C, geom, ad, wide):
    B, h, wd, H, W = geom
    out = nan(B, h, wd, ad.stride(3), dtype=ad.dtype)
    gout = torch.tensor([0.7], device=DEV)
    N.call('tss_upsample_ce%s_bwd' % ('_wide' if wide else ''), N.ptr(ws), N.ptr(scale), N.ptr(gout), N.ptr(out), ad.stride(3), B, C, h, wd,
           H, W, N.dtype_code(ad.dtype), N.stream())
    return out


def assert_abi_result(out, loss, C, want):
    assert torch.isfinite(out.float()).all() and torch.isfinite(loss).all()
    assert torch.equal(loss.reshape(()).cpu(), want[0])
    assert torch.equal(out.permute(0, 3, 1, 2)[:, :C].float().cpu(), want[1])
    assert (out[..., C:] == 0).all()


@DTYPES
@pytest.mark.parametrize('name', list(FUSED))
def test_register_passes_write_every_workspace_element_that_the_gather_reads(name, dtype):
    """NaN-filled workspaces and a NaN-filled gradient buffer: finite, the bits of the autograd path, pad channels exactly 0."""
    from torch_semantic_segmentation_amd import _native as N
    low, target, scale = head_input(name, dtype == torch.bfloat16)
    B, C, h, wd = low.shape
    H, W = h * scale, wd * scale
    ad, t = nhwc(low, dtype), target.to(DEV)
    code, ldl, st = N.dtype_code(ad.dtype), ad.stride(3), N.stream()
    want = hip_focal(low, target, scale, 2.0, 'reference', dtype, gscale=0.7)
    ws, scal = nan(N.lib().tss_upsample_ce_ws(B, C, h, wd, H, W)), nan(2)
    N.call('tss_upsample_focal_fwd', N.ptr(ad), ldl, N.ptr(t), N.ptr(ws), N.ptr(scal[0:1]), N.ptr(scal[1:2]), B, C, h, wd, H, W, 255, 1,
           ALPHA, 2.0, 0, code, st)
    assert_abi_result(gather(N, ws, scal[1:2], C, (B, h, wd, H, W), ad, False), scal[0], C, want)
    want = hip_dice(low, target, scale, 1.0, dtype, gscale=0.7)
    nd = N.lib().tss_upsample_dice_ws(B, C, h, wd, H, W)
    assert nd > 0
    dws, loss, ws = nan(nd), nan(1), nan(N.lib().tss_upsample_ce_ws(B, C, h, wd, H, W))
    N.call('tss_upsample_dice_fwd', N.ptr(ad), ldl, N.ptr(t), N.ptr(dws), N.ptr(loss), B, C, h, wd, H, W, 255, 1, 1.0, code, st)
    assert torch.isfinite(dws[:48]).all() and (dws[C:24] == 0).all() and (dws[24 + C:48] == 0).all()
    N.call('tss_upsample_dice_grad', N.ptr(ad), ldl, N.ptr(t), N.ptr(dws), N.ptr(ws), B, C, h, wd, H, W, 255, 1, code, st)
    assert_abi_result(gather(N, ws, torch.ones(1, device=DEV), C, (B, h, wd, H, W), ad, False), loss, C, want)


@DTYPES
@pytest.mark.parametrize('name', WIDE_NAMES)
def test_wide_route_writes_every_workspace_element_that_the_gather_reads(name, dtype):
    from torch_semantic_segmentation_amd import _native as N
    low, target, scale = wide_head_input(name, dtype == torch.bfloat16)
    B, C, h, wd = low.shape
    H, W = h * scale, wd * scale
    ad, t = nhwc(low, dtype), target.to(DEV)
    code, ldl, st = N.dtype_code(ad.dtype), ad.stride(3), N.stream()
    want = hip_focal(low, target, scale, 0.5, 'lin', dtype, gscale=0.7)
    n = B * H * W
    pix, rows, scal = nan(B, H, W), nan(N.lib().tss_focal_coef_rows(n), 2, dtype=torch.float64), nan(2)
    N.call('tss_upsample_pixel_ce_wide', N.ptr(ad), ldl, N.ptr(t), N.ptr(pix), B, C, h, wd, H, W, 255, code, st)
    N.call('tss_focal_coef_from_ce', N.ptr(pix), N.ptr(t), N.ptr(rows), N.ptr(scal[0:1]), N.ptr(scal[1:2]), n, C, 255, 1, ALPHA, 0.5, 1, st)
    assert torch.isfinite(pix).all() and (pix[(t < 0) | (t >= C)] == 0).all()
    ws = nan(N.lib().tss_upsample_ce_wide_ws(B, C, h, wd, H, W))
    N.call('tss_upsample_coef_grad_wide', N.ptr(ad), ldl, N.ptr(t), N.ptr(pix), N.ptr(ws), B, C, h, wd, H, W, 255, code, st)
    assert_abi_result(gather(N, ws, scal[1:2], C, (B, h, wd, H, W), ad, True), scal[0], C, want)


# ----------------------------------------------------------------------------- 5. degenerate and scaling cases

def routes():
    """(name, run(target, dtype, **kw) -> (loss, grad), labels) for the three routes at a small geometry each."""
    low, target, scale = head_input('base', False)
    wlow, wtarget, wscale = wide_head_input('c25', False)
    return [('focal', lambda t, dtype=torch.float32, **kw: hip_focal(low, t, scale, 2.0, 'reference', dtype, **kw), target),
            ('focal wide', lambda t, dtype=torch.float32, **kw: hip_focal(wlow, t, wscale, 2.0, 'lin', dtype, **kw), wtarget),
            ('dice', lambda t, dtype=torch.float32, **kw: hip_dice(low, t, scale, 1.0, dtype, **kw), target)]


@DTYPES
def test_all_ignored_target_gives_zero_loss_and_zero_gradient(dtype):
    for name, run, target in routes():
        for fill in (255, -1):
            loss, grad = run(torch.full_like(target, fill), dtype)
            assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0, name
    low, target, scale = head_input('base', False)
    loss, grad = hip_dice(low, torch.full_like(target, 255), scale, 0.0, dtype)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


def test_ignore_index_none_keeps_every_in_range_pixel():
    """Label 255 is out of range for these class counts, so it stays out with ignore_index=None too; an in-range ignore_index drops
    that class's pixels, None keeps them."""
    low, target, scale = head_input('base', False)
    wlow, wtarget, wscale = wide_head_input('c25', False)
    for ignore in (None, 4):
        want = reference(up_focal, low, target, ALPHA, 2.0, ignore, 'reference')
        check('focal ignore %s' % ignore, hip_focal(low, target, scale, 2.0, 'reference', ignore=ignore), want, False)
        want = reference(up_focal, wlow, wtarget, ALPHA, 2.0, ignore, 'lin')
        check('focal wide ignore %s' % ignore, hip_focal(wlow, wtarget, wscale, 2.0, 'lin', ignore=ignore), want, False)
        want = reference(up_dice, low, target, 19, 1.0, ignore)
        check('dice ignore %s' % ignore, hip_dice(low, target, scale, 1.0, ignore=ignore), want, False)
    none, in_range = (hip_focal(low, target, scale, 2.0, 'reference', ignore=i)[0] for i in (None, 4))
    assert torch.equal(none, hip_focal(low, target, scale, 2.0, 'reference', ignore=255)[0]) and not torch.equal(none, in_range)


def test_grad_out_scales_the_gradient_linearly():
    for name, run, target in routes():
        one, scaled = run(target), run(target, gscale=0.7)
        assert torch.equal(one[0], scaled[0]), name
        assert cases.rel_err(scaled[1].numpy(), 0.7 * one[1].double().numpy()) <= 4 * 2.0 ** -24, name     # one product more, one rounding


def test_alpha_scales_the_focal_loss_linearly():
    """alpha enters the finalize kernel as a factor of the f64 sums; 4 is a power of two, so loss and gradient are exact multiples up
    to the one rounding to f32."""
    for name, run, target in routes()[:2]:
        a, b = run(target, alpha=0.25), run(target, alpha=1.0)
        assert abs(float(b[0]) / (4 * float(a[0])) - 1) <= 2.0 ** -23, name
        assert cases.rel_err(b[1].numpy(), 4 * a[1].double().numpy()) <= 4 * 2.0 ** -24, name


# ----------------------------------------------------------------------------- 6. envelope

def test_outside_the_envelope_the_operators_return_the_unfused_composition():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(47)
    for C, fused, planar in ((25, lambda a, t: tssa.upsample_dice_loss(a, t, 25, scale_factor=2, ignore_index=255),
                              lambda x, t: tssa.dice_loss(x, t, 25, ignore_index=255)),
                             (257, lambda a, t: tssa.upsample_focal_loss(a, t, scale_factor=2, ignore_index=255),
                              lambda x, t: tssa.focal_loss(x, t, ignore_index=255))):
        low = (2.0 * torch.randn(1, C, 4, 8, generator=g)).to(DEV)
        target = torch.randint(0, C, (1, 8, 16), generator=g)
        target[torch.rand(1, 8, 16, generator=g) < 0.1] = 255
        target = target.to(DEV)
        a, b = (ops.to_nhwc(low).clone().requires_grad_(True) for _ in range(2))
        got, want = fused(a, target), planar(ops.upsample_logits(b, size=(8, 16)), target)
        got.backward()
        want.backward()
        assert float(want.detach()) > 0 and torch.equal(got.detach(), want.detach()) and torch.equal(a.grad, b.grad), C
    # an output smaller than the map: the same rule
    low = (2.0 * torch.randn(1, 19, 8, 16, generator=g)).to(DEV)
    target = torch.randint(0, 19, (1, 4, 8), generator=g).to(DEV)
    assert torch.equal(tssa.upsample_focal_loss(low, target, size=(4, 8)), tssa.focal_loss(ops.upsample_logits(low, size=(4, 8)), target))
    assert torch.equal(tssa.upsample_dice_loss(low, target, 19, size=(4, 8)), tssa.dice_loss(ops.upsample_logits(low, size=(4, 8)), target, 19))


def test_argument_errors_and_refused_shapes():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import _native as N
    low, target, scale = head_input('base', False)
    a, t = nhwc(low, torch.float32), target.to(DEV)
    for bad in (dict(gamma=-0.5), dict(variant='berman')):
        with pytest.raises(ValueError):
            tssa.upsample_focal_loss(a, t, scale_factor=scale, **bad)
    with pytest.raises(ValueError):
        tssa.upsample_dice_loss(a, t, 19, scale_factor=scale, smooth=-1.0)
    with pytest.raises(ValueError):
        tssa.upsample_dice_loss(a, t, 18, scale_factor=scale)
    for fn in (lambda tt: tssa.upsample_focal_loss(a, tt, scale_factor=scale), lambda tt: tssa.upsample_dice_loss(a, tt, 19, scale_factor=scale)):
        with pytest.raises(RuntimeError):
            fn(t.int())
        with pytest.raises(RuntimeError):
            fn(t[:, :-1])
    # the C side answers TSS_ERR_SHAPE (-2) before it launches anything
    lib, ptr, st = N.lib(), N.ptr, N.stream()
    big = torch.zeros(1, 4, 8, 264, device=DEV)
    tt = torch.zeros(1, 8, 16, dtype=torch.int64, device=DEV)
    ws, scal = torch.empty(1 << 16, device=DEV), torch.empty(2, device=DEV)
    rows = torch.empty(64, 2, dtype=torch.float64, device=DEV)
    focal = lambda C, ldl, h, H, gamma, variant: lib.tss_upsample_focal_fwd(ptr(big), ldl, ptr(tt), ptr(ws), ptr(scal[0:1]), ptr(scal[1:2]),
                                                                            1, C, h, 8, H, 16, 255, 1, 0.25, gamma, variant, 0, st)
    dice = lambda C, ldl, h, H, smooth: lib.tss_upsample_dice_fwd(ptr(big), ldl, ptr(tt), ptr(ws), ptr(scal[0:1]), 1, C, h, 8, H, 16, 255, 1,
                                                                  smooth, 0, st)
    assert focal(19, 24, 4, 8, 2.0, 0) == 0 and dice(19, 24, 4, 8, 1.0) == 0
    assert focal(25, 32, 4, 8, 2.0, 0) == -2 and focal(0, 24, 4, 8, 2.0, 0) == -2 and dice(25, 32, 4, 8, 1.0) == -2
    assert focal(19, 24, 4, 3, 2.0, 0) == -2 and dice(19, 24, 4, 3, 1.0) == -2                     # H < h
    assert focal(19, 24, 4, 8, -0.5, 0) == -2 and focal(19, 24, 4, 8, 2.0, 2) == -2 and dice(19, 24, 4, 8, -1.0) == -2
    assert lib.tss_upsample_dice_grad(ptr(big), 32, ptr(tt), ptr(ws), ptr(ws), 1, 25, 4, 8, 8, 16, 255, 1, 0, st) == -2
    assert lib.tss_upsample_dice_ws(1, 25, 4, 8, 8, 16) == 0 and lib.tss_upsample_dice_ws(1, 24, 4, 8, 8, 16) > 0
    assert lib.tss_upsample_dice_ws(1, 19, 4, 8, 3, 16) == 0
    coef = lambda C, gamma, variant: lib.tss_focal_coef_from_ce(ptr(ws), ptr(tt), ptr(rows), ptr(scal[0:1]), ptr(scal[1:2]), 128, C, 255, 1,
                                                                0.25, gamma, variant, st)
    assert coef(66, 2.0, 1) == 0 and coef(66, -0.5, 0) == -2 and coef(66, 2.0, 2) == -2 and coef(0, 2.0, 0) == -2
    assert lib.tss_focal_coef_rows(0) == 0 and lib.tss_focal_coef_rows(128) == 1 and lib.tss_focal_coef_rows(1025) == 2
    grad = lambda C, ldl, h, H: lib.tss_upsample_coef_grad_wide(ptr(big), ldl, ptr(tt), ptr(ws), ptr(ws), 1, C, h, 8, H, 16, 255, 0, st)
    assert grad(257, 264, 4, 8) == -2 and grad(66, 72, 4, 3) == -2
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 7. peak memory

@pytest.mark.parametrize('loss,C', [('focal', 19), ('focal', 66), ('dice', 19)])
def test_peak_memory_stays_below_half_the_full_resolution_logits(loss, C):
    """low = (1, C, 16, 32), scale 8, f32: forward + backward may raise the peak by less than half of B C H W 4 bytes (the method of
    tests/test_gpu_widehead.py's test of the same name)."""
    from torch_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(1)
    low = ops.to_nhwc(torch.randn(1, C, 16, 32, generator=g).to(DEV)).clone().requires_grad_(True)
    target = torch.randint(0, C, (1, 128, 256), generator=g).to(DEV)
    full = 1 * C * 128 * 256 * 4
    if loss == 'focal':
        fn = lambda: ops.upsample_focal_loss(low, target, scale_factor=8, ignore_index=255)
    else:
        fn = lambda: ops.upsample_dice_loss(low, target, C, scale_factor=8, ignore_index=255)
    fn().backward()          # warm: one-time buffers
    low.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    fn().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print('%s C=%d: peak rise %.2f MB, full-resolution logits %.2f MB' % (loss, C, rise / 1e6, full / 1e6))
    assert rise < full / 2
