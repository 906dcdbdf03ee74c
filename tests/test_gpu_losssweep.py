"""What the shared class-plane sweep (csrc/losssweep.h) guarantees across the losses built on it: the same per-pixel
log-sum-exp bits from every forward that saves one, and one validity rule (a pixel counts iff target != ignore_index and
0 <= target < C).  Inputs are built on the CPU from fixed seeds."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """logits (float32, CPU) and a target mixing valid labels with 255 (the ignore index), -1, C and 300."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(B * 1000 + H)
    logits = 3.0 * torch.randn(B, C, H, W, generator=g)
    target = torch.randint(0, C, (B, H, W), generator=g)
    flat = target.view(-1)
    flat[[0, 9, 10]] = 255
    flat[[2, 17]] = -1
    flat[[5, 23]] = C
    flat[[7, 12]] = 300
    return logits, target


@DTYPES
@pytest.mark.parametrize('shape', [(3, 19, 1, 8), (2, 19, 4, 8)], ids=['group_per_image', 'four_groups_per_image'])
def test_every_forward_saves_the_same_lse(shape, dtype):
    """tss_cross_entropy_fwd, tss_ohem_fwd and tss_dice_fwd write bit-identical per-pixel lse arrays for the same logits (the
    focal forward is not in the list: its log1pf branch is a different formula by design)."""
    from torch_semantic_segmentation_amd import _native as N
    call, ptr, stream = N.call, N.ptr, N.stream
    B, C, H, W = shape
    logits, target = _inputs(shape)
    x, t = logits.to(DEV).to(dtype), target.to(DEV)
    code = N.dtype_code(dtype)

    def f32(*s):
        return torch.zeros(s, dtype=torch.float32, device=DEV)

    lse_ce, lse_ohem, lse_dice = f32(B, H, W), f32(B, H, W), f32(B, H, W)
    scal = f32(2)
    acc = torch.zeros(2, dtype=torch.float64, device=DEV)
    call('tss_cross_entropy_fwd', ptr(x), ptr(t), ptr(lse_ce), ptr(acc), ptr(scal[0:1]), ptr(scal[1:2]), B, C, H * W, 255, code, stream())
    pix, res = f32(B, H, W), f32(5)
    ws = torch.zeros(N.lib().tss_ohem_workspace_bytes(), dtype=torch.uint8, device=DEV)
    call('tss_ohem_fwd', ptr(x), ptr(t), ptr(lse_ohem), ptr(pix), ptr(ws), ptr(res[0:1]), ptr(res[1:5]), B, C, H * W, 255,
         0.35667494393873245, int(B * H * W * 0.05), code, stream())
    dws = torch.zeros(N.lib().tss_dice_workspace_bytes(B, C, H * W, 0), dtype=torch.uint8, device=DEV)
    loss = f32(1)
    call('tss_dice_fwd', ptr(x), ptr(t), ptr(lse_dice), ptr(dws), ptr(loss), B, C, H * W, 255, 1, 1.0, 0, code, stream())
    ref = torch.logsumexp(x.float(), dim=1)
    assert torch.allclose(lse_ce, ref, rtol=1e-5, atol=1e-5)          # an lse at all, not three equal arrays of anything
    assert torch.equal(lse_ce.view(torch.int32), lse_ohem.view(torch.int32))
    assert torch.equal(lse_ce.view(torch.int32), lse_dice.view(torch.int32))


@DTYPES
@pytest.mark.parametrize('loss', ['cross_entropy', 'ohem_loss', 'focal_loss', 'dice_loss'])
def test_one_validity_rule(loss, dtype):
    """Labels 255 (ignored), -1, C and 300 are dropped by every loss alike: the gradient is exactly zero at those pixels in all C
    planes, and it is not all-zero over the kept ones.  (Lovasz-Softmax is not in the list: by its documented rule an
    out-of-range label is background, not dropped.)"""
    import torch_semantic_segmentation_amd as tssa
    shape = (2, 19, 4, 8)
    C = shape[1]
    logits, target = _inputs(shape)
    x = logits.to(DEV).to(dtype).requires_grad_(True)
    t = target.to(DEV)
    fn = {'cross_entropy': lambda: tssa.cross_entropy(x, t, ignore_index=255),
          'ohem_loss': lambda: tssa.ohem_loss(x, t, ignore_index=255),
          'focal_loss': lambda: tssa.focal_loss(x, t, ignore_index=255),
          'dice_loss': lambda: tssa.dice_loss(x, t, C, ignore_index=255)}[loss]
    fn().backward()
    kept = (t != 255) & (t >= 0) & (t < C)
    assert 0 < int(kept.sum()) < kept.numel() and int((~kept).sum()) == 9
    grad = x.grad.float().movedim(1, -1)                                # [B, H, W, C]
    assert bool(torch.isfinite(grad).all())
    assert int((grad[~kept] != 0).sum()) == 0
    assert int((grad[kept] != 0).sum()) > 0
