"""Non-GPU: the public surface of the fused focal / Dice head (csrc/softhead.hip): the operators are exported, the loss modules
take fused_head (default off), the Trainer's choice of route follows it, the header declares the entries and their workspace
queries answer on the host."""
import inspect

import torch


def test_operators_are_exported_from_the_package():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    assert tssa.upsample_focal_loss is ops.upsample_focal_loss and tssa.upsample_dice_loss is ops.upsample_dice_loss
    p = inspect.signature(tssa.upsample_focal_loss).parameters
    assert list(p) == ['low', 'target', 'scale_factor', 'size', 'alpha', 'gamma', 'ignore_index', 'variant']
    assert (p['alpha'].default, p['gamma'].default, p['ignore_index'].default, p['variant'].default) == (0.25, 2.0, -100, 'reference')
    p = inspect.signature(tssa.upsample_dice_loss).parameters
    assert list(p) == ['low', 'target', 'num_classes', 'scale_factor', 'size', 'smooth', 'ignore_index']
    assert (p['smooth'].default, p['ignore_index'].default) == (1.0, -100)


def test_loss_modules_take_fused_head_and_default_to_off():
    import torch_semantic_segmentation_amd as tssa
    f, d = tssa.FocalLoss(), tssa.DiceLoss(19)
    assert f.fused_head is False and d.fused_head is False
    assert (f.alpha, f.gamma, f.ignore_index, f.variant) == (0.25, 2.0, None, 'reference')
    assert (d.num_classes, d.smooth, d.ignore_index) == (19, 1.0, -100)
    assert tssa.FocalLoss(ignore_index=255, fused_head=True).fused_head is True
    assert tssa.DiceLoss(19, ignore_index=255, fused_head=True).fused_head is True


class _LowresModel(torch.nn.Module):
    logit_scale = 8

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 19, 1)

    def forward_lowres(self, x):
        return self.conv(x)


def test_trainer_fuses_these_losses_only_on_request():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    m = _LowresModel()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    for on, off in ((tssa.FocalLoss(fused_head=True), tssa.FocalLoss()), (tssa.DiceLoss(19, fused_head=True), tssa.DiceLoss(19))):
        assert E.Trainer(m, opt, on).fuse_head_loss
        assert not E.Trainer(m, opt, off).fuse_head_loss
        assert not E.Trainer(m, opt, on, fuse_head_loss=False).fuse_head_loss
        assert not E.Trainer(torch.nn.Conv2d(3, 19, 1), opt, on).fuse_head_loss          # no forward_lowres
    assert E.Trainer(m, opt, tssa.CrossEntropyLoss(255)).fuse_head_loss


def test_header_declares_the_entries_and_the_workspace_queries_answer():
    from torch_semantic_segmentation_amd import _native as N
    decls = N.parse_header()
    for name in ('tss_upsample_focal_fwd', 'tss_focal_coef_rows', 'tss_focal_coef_from_ce', 'tss_upsample_coef_grad_wide',
                 'tss_upsample_dice_ws', 'tss_upsample_dice_fwd', 'tss_upsample_dice_grad'):
        assert name in decls, name
    lib = N.lib()
    # 8x19x128x256 -> 1024x2048: 8 strips x 32 bands x 8 images = 2048 blocks, a row of 3 x 19 doubles each, 64 floats of coefficients
    assert lib.tss_upsample_dice_ws(8, 19, 128, 256, 1024, 2048) == 64 + 2048 * 3 * 19 * 2
    assert lib.tss_upsample_dice_ws(8, 25, 128, 256, 1024, 2048) == 0 and lib.tss_upsample_dice_ws(8, 19, 128, 256, 64, 2048) == 0
    assert lib.tss_focal_coef_rows(8 * 1024 * 2048) == 4096 and lib.tss_focal_coef_rows(0) == 0
