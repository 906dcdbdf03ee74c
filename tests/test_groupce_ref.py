"""Non-GPU: tests/groupce_ref.py pinned against hand-worked cases, the host validation of per-sample loss groups (it runs before any
device access, so it needs no GPU), and the public surface of the feature."""
import inspect
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import groupce_ref as R

IGN = 255


def _inputs(B=4, C=5, h=3, w=4, H=7, W=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    low = torch.randn((B, C, h, w), generator=g, dtype=torch.float64)
    t = torch.randint(0, C, (B, H, W), generator=g)
    t[torch.rand((B, H, W), generator=g) < 0.1] = IGN
    return low, t


def test_one_group_reproduces_the_mean():
    low, t = _inputs()
    for cw, eps in ((None, 0.0), (torch.tensor([0.5, 1.0, 2.0, 0.0, 1.5], dtype=torch.float64), 0.0), (None, 0.125)):
        x = low.clone().requires_grad_(True)
        z = F.interpolate(x, size=t.shape[-2:], mode='bilinear', align_corners=True)
        want = F.cross_entropy(z, t, weight=cw, ignore_index=IGN, label_smoothing=eps)
        gwant, = torch.autograd.grad(want * 0.7, x)
        want = want.detach()
        r = R.grouped_ce(low, t, [2, 2, 2, 2], class_weight=cw, label_smoothing=eps, grad_out=0.7)
        assert abs(r['loss'] - float(want)) <= 1e-13 * abs(float(want))
        assert float((r['grad'] - gwant).abs().max()) <= 1e-13
        assert r['group_loss'].tolist() == [0.0, 0.0, r['loss'], 0.0]
        assert torch.allclose(r['scale'], torch.full((4,), 1.0 / float(r['n'].sum()), dtype=torch.float64), rtol=1e-15, atol=0)


def test_two_groups_by_hand():
    """identity size, two classes, logits (0, ln 3): p = (1/4, 3/4), so a pixel of class 1 costs ln(4/3) and one of class 0 ln 4.
    Sample 0 (group 0, lambda 1): 4 pixels of class 1.  Sample 1 (group 1, lambda 0.5): 2 of class 0, 1 of class 1, 1 ignored.
        L_0 = ln(4/3),  L_1 = 0.5 (2 ln 4 + ln(4/3)) / 3,  scale = (1/4, 0.5/3)"""
    low = torch.zeros((2, 2, 2, 2), dtype=torch.float64)
    low[:, 1] = math.log(3.0)
    t = torch.tensor([[[1, 1], [1, 1]], [[0, 0], [1, IGN]]])
    r = R.grouped_ce(low, t, [0, 1], [1.0, 0.5])
    L0, L1 = math.log(4 / 3), 0.5 * (2 * math.log(4) + math.log(4 / 3)) / 3
    assert abs(float(r['group_loss'][0]) - L0) < 1e-15 and abs(float(r['group_loss'][1]) - L1) < 1e-15
    assert abs(r['loss'] - (L0 + L1)) < 1e-15
    assert r['n'].tolist() == [4.0, 3.0] and r['scale'].tolist() == [0.25, 0.5 / 3]
    # d CE / d z_c = p_c - [c == t]: sample 0's pixels carry (1/4) (1/4, -1/4) each, the ignored pixel of sample 1 nothing
    assert torch.allclose(r['grad'][0, 0], torch.full((2, 2), 0.25 * 0.25, dtype=torch.float64), rtol=1e-14, atol=0)
    assert torch.allclose(r['grad'][1, :, 0, 0], torch.tensor([-0.75, 0.75], dtype=torch.float64) * 0.5 / 3, rtol=1e-14, atol=0)
    assert r['grad'][1, :, 1, 1].tolist() == [0.0, 0.0]
    # uniform logits: every valid pixel costs ln C whatever the counts are, and lambda scales the term
    low, t = _inputs(seed=3)
    r = R.grouped_ce(torch.zeros_like(low), t, [0, 1, 0, 1], [1.0, 0.5, 1.0, 0.5])
    assert abs(r['loss'] - 1.5 * math.log(5)) < 1e-14


def test_an_all_ignored_group_gives_zero():
    low, t = _inputs(seed=1)
    t[1] = IGN
    t[3] = -1                 # out of range: ignored too
    r = R.grouped_ce(low, t, [0, 1, 0, 1], [1.0, 0.5, 1.0, 0.5])
    solo = R.grouped_ce(low[[0, 2]], t[[0, 2]], [0, 0])
    assert float(r['group_loss'][1]) == 0.0 and r['scale'][[1, 3]].tolist() == [0.0, 0.0]
    assert abs(r['loss'] - solo['loss']) < 1e-15 and math.isfinite(r['loss'])
    assert float(r['grad'][[1, 3]].abs().max()) == 0.0 and not torch.isnan(r['grad']).any()
    assert torch.equal(r['grad'][[0, 2]], solo['grad'])
    # every group empty: the loss is 0, not nan
    t[:] = IGN
    r = R.grouped_ce(low, t, [0, 1, 0, 1])
    assert r['loss'] == 0.0 and float(r['grad'].abs().max()) == 0.0


def test_selftrain_weights_by_hand():
    g, w = R.selftrain_weights([10, 30], 100, 0.5, 0)
    assert g.tolist() == [0, 0, 1, 1] and g.dtype == np.int32 and w.dtype == np.float32 and w.tolist() == [1.0, 1.0, 0.5, 0.5]
    g, w = R.selftrain_weights([10, 30], 100, 0.5, 1)               # share 40 / 200 = 0.2, times 0.5
    assert g.tolist() == [0, 0, 1, 1] and w.tolist() == [1.0, 1.0, float(np.float32(0.1)), float(np.float32(0.1))]
    assert R.selftrain_weights([0, 0, 0], 64, 2.0, 1)[1].tolist() == [1.0] * 3 + [0.0] * 3
    assert R.selftrain_weights([64, 64, 64], 64, 0.3, 1)[1][3:].tolist() == [float(np.float32(0.3))] * 3     # everything kept: lam itself
    # rounded once: float32(lam) enters in float64
    lam = np.float32(0.7)
    assert R.selftrain_weights([5, 6], 9, 0.7, 1)[1][2] == np.float32(np.float64(lam) * 11.0 / 18.0)


def test_host_validation_raises_before_any_device_access():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    g, w = tssa.check_sample_groups([0, 1, 0], [1.0, 0.5, 0], 3)
    assert g.dtype == np.int32 and g.tolist() == [0, 1, 0] and w.dtype == np.float32 and w.tolist() == [1.0, 0.5, 0.0]
    assert tssa.check_sample_groups(torch.tensor([2, 2, 2]), None, 3)[1] is None
    bad = (([0, 1], None), ([0, 1, 3], None), ([0, -1, 1], None), ([0.0, 1.0, 1.0], None), ([[0, 1, 1]], None),
           ([0, 1, 1], [1.0, 1.0]), ([0, 1, 1], [1.0, -0.5, 1.0]), ([0, 1, 1], [1.0, float('nan'), 1.0]),
           ([0, 1, 1], [1.0, float('inf'), 1.0]))
    for group, weight in bad:
        with pytest.raises(ValueError):
            ops.check_sample_groups(group, weight, 3)
    # through the operator, on host tensors: the ValueError comes before anything asks for the device
    low, t = torch.zeros((3, 5, 2, 2)), torch.zeros((3, 4, 4), dtype=torch.int64)
    for group, weight in bad:
        with pytest.raises(ValueError):
            tssa.upsample_cross_entropy(low, t, size=(4, 4), sample_group=group, sample_weight=weight)
    with pytest.raises(ValueError):           # more classes than the fused head takes: no unfused route
        tssa.upsample_cross_entropy(torch.zeros((3, 257, 2, 2)), t, size=(4, 4), sample_group=[0, 0, 1])
    with pytest.raises(ValueError):           # an output smaller than the map
        tssa.upsample_cross_entropy(torch.zeros((3, 5, 8, 8)), t, size=(4, 4), sample_group=[0, 0, 1])
    with pytest.raises(ValueError):           # rows without groups
        tssa.upsample_cross_entropy(low, t, size=(4, 4), sample_weight=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        tssa.CrossEntropyLoss(ignore_index=IGN).set_sample_groups([0, 5, 1])


def test_public_surface():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import _native as N, ops
    p = inspect.signature(tssa.upsample_cross_entropy).parameters
    assert list(p) == ['low', 'target', 'scale_factor', 'size', 'ignore_index', 'weight', 'label_smoothing', 'sample_group',
                       'sample_weight', 'group_loss_out']
    assert all(p[k].default is None for k in ('sample_group', 'sample_weight', 'group_loss_out'))
    assert tssa.UpsampleGroupedCrossEntropyFn is ops.UpsampleGroupedCrossEntropyFn
    ce = tssa.CrossEntropyLoss(ignore_index=IGN)
    assert ce.sample_group is None and ce.sample_weight is None and ce.group_loss_out is None
    assert 'sample_group' not in ce.state_dict()
    ce.clear_sample_groups()
    p = inspect.signature(tssa.SelfTraining.__init__).parameters
    assert p['unsup_weight'].default is None and p['unsup_weighting'].default == 'mean'
    decls = N.parse_header()
    for name in ('tss_upsample_ce_group_finalize', 'tss_upsample_ce_bwd_rows', 'tss_upsample_ce_wide_bwd_rows', 'tss_selftrain_weights',
                 'tss_upsample_ce_group_max_batch'):
        assert name in decls, name
    assert N.lib().tss_upsample_ce_group_max_batch() == ops.GROUP_MAX_BATCH
