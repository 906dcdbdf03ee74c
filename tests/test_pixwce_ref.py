"""Non-GPU: tests/pixwce_ref.py pinned against hand-worked cases, against tests/groupce_ref.py for a map of ones and against
torch.mean(ce * omega); its HeadRef helper against its own autograd; the numpy restatement of mix_plane; the host validation of the map
(it runs before any device access) and the public surface of the feature."""
import inspect
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import groupce_ref as G
from tests import pixwce_ref as R

IGN = 255


def _inputs(B=4, C=5, h=3, w=4, H=7, W=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    low = torch.randn((B, C, h, w), generator=g, dtype=torch.float64)
    t = torch.randint(0, C, (B, H, W), generator=g)
    t[torch.rand((B, H, W), generator=g) < 0.1] = IGN
    om = torch.randint(0, 17, (B, H, W), generator=g).double() / 8
    return low, t, om


def test_the_three_norms_by_hand():
    """identity size 2x2, two classes, logits (0, ln 3): p = (1/4, 3/4); a pixel of class 1 costs a = ln(4/3), one of class 0 b = ln 4.
    One sample: labels (1, 0 / 1, ignored), omega (2, 0.5 / 0, 7), class weights (w0, w1) = (3, 0.5):
        k = (1, 1.5, 0, -), numerator = a + 1.5 b;  D: 'weight' 2.5, 'valid' 0.5 + 3 + 0.5 = 4, 'pixels' 4 (the ignored one included)
    and without class weights k = (2, 0.5, 0, -), numerator 2 a + 0.5 b;  D: 2.5, 3, 4"""
    low = torch.zeros((1, 2, 2, 2), dtype=torch.float64)
    low[:, 1] = math.log(3.0)
    t = torch.tensor([[[1, 0], [1, IGN]]])
    om = torch.tensor([[[2.0, 0.5], [0.0, 7.0]]], dtype=torch.float64)
    a, b = math.log(4 / 3), math.log(4.0)
    cw = torch.tensor([3.0, 0.5], dtype=torch.float64)
    for norm, D in (('weight', 2.5), ('valid', 4.0), ('pixels', 4.0)):
        r = R.pixel_weighted_ce(low, t, om, class_weight=cw, norm=norm)
        assert abs(r['loss'] - (a + 1.5 * b) / D) < 1e-15 and r['n'].tolist() == [D], norm
        # d loss / d z = k (p - onehot) / D: pixel (0, 0) class 1 with k = 1, pixel (0, 1) class 0 with k = 1.5, the others nothing
        assert torch.allclose(r['grad'][0, :, 0, 0], torch.tensor([0.25, -0.25], dtype=torch.float64) / D, rtol=1e-14, atol=0)
        assert torch.allclose(r['grad'][0, :, 0, 1], torch.tensor([-0.75, 0.75], dtype=torch.float64) * 1.5 / D, rtol=1e-14, atol=0)
        assert r['grad'][0, :, 1, 0].tolist() == [0.0, 0.0] and r['grad'][0, :, 1, 1].tolist() == [0.0, 0.0]
    for norm, D in (('weight', 2.5), ('valid', 3.0), ('pixels', 4.0)):
        r = R.pixel_weighted_ce(low, t, om, norm=norm)
        assert abs(r['loss'] - (2 * a + 0.5 * b) / D) < 1e-15 and r['n'].tolist() == [D], norm
    # a nan under an ignored pixel is never looked at
    om[0, 1, 1] = float('nan')
    assert math.isfinite(R.pixel_weighted_ce(low, t, om)['loss'])


def test_a_map_of_ones_restates_the_grouped_loss():
    low, t, _ = _inputs()
    ones = torch.ones(t.shape, dtype=torch.float64)
    cw = torch.tensor([0.5, 1.0, 2.0, 0.0, 1.5], dtype=torch.float64)
    for weight in (None, cw):
        for group, lam in (([0, 0, 0, 0], None), ([0, 1, 0, 1], [1.0, 0.5, 1.0, 0.5]), ([3, 0, 3, 0], [0.3, 2.0, 0.3, 2.0])):
            want = G.grouped_ce(low, t, group, lam, class_weight=weight, grad_out=0.7)
            for norm in ('valid', 'weight'):
                r = R.pixel_weighted_ce(low, t, ones, class_weight=weight, norm=norm, group=group, weight=lam, grad_out=0.7)
                assert abs(r['loss'] - want['loss']) <= 1e-14 * abs(want['loss'])
                assert torch.allclose(r['group_loss'], want['group_loss'], rtol=1e-14, atol=0)
                assert torch.allclose(r['grad'], want['grad'], rtol=1e-13, atol=1e-16) and torch.equal(r['n'], want['n'])
    # group=None is one group of weight 1
    a, b = R.pixel_weighted_ce(low, t, ones), G.grouped_ce(low, t, [0, 0, 0, 0])
    assert abs(a['loss'] - b['loss']) <= 1e-15 and a['group_loss'].tolist()[1:] == [0.0, 0.0, 0.0]


def test_pixels_is_the_mean_of_the_weighted_map():
    low, t, om = _inputs(seed=2)
    t = torch.where(t == IGN, torch.zeros_like(t), t)          # nothing ignored
    x = low.clone().requires_grad_(True)
    z = F.interpolate(x, size=t.shape[-2:], mode='bilinear', align_corners=True)
    want = torch.mean(F.cross_entropy(z, t, reduction='none') * om)
    gwant, = torch.autograd.grad(want, x)
    want = want.detach()
    r = R.pixel_weighted_ce(low, t, om, norm='pixels')
    assert abs(r['loss'] - float(want)) <= 1e-14 * abs(float(want)) and float((r['grad'] - gwant).abs().max()) <= 1e-14
    # with ignored pixels the denominator still counts them
    low, t, om = _inputs(seed=2)
    r = R.pixel_weighted_ce(low, t, om, norm='pixels')
    assert r['n'].tolist() == [63.0] * 4 and abs(r['loss'] - float(r['S'].sum()) / 252.0) < 1e-15


def test_an_empty_denominator_gives_zero():
    low, t, om = _inputs(seed=1)
    zero = torch.zeros_like(om)
    r = R.pixel_weighted_ce(low, t, zero)
    assert r['loss'] == 0.0 and float(r['grad'].abs().max()) == 0.0 and r['group_loss'].tolist() == [0.0] * 4
    om[1] = 0.0
    r = R.pixel_weighted_ce(low, t, om, group=[0, 1, 2, 3])
    assert float(r['group_loss'][1]) == 0.0 and float(r['grad'][1].abs().max()) == 0.0 and not torch.isnan(r['grad']).any()
    # 'valid': the zero-weight sample still counts in the denominator, its numerator is 0
    r = R.pixel_weighted_ce(low, t, om, norm='valid', group=[0, 1, 2, 3])
    assert float(r['n'][1]) > 0 and float(r['group_loss'][1]) == 0.0 and float(r['scale'][1]) > 0


def test_head_ref_helper_agrees_with_autograd():
    from tests import exact as X
    g = X.case_gen(7)
    x, labels = X.head_logits((2, 5, 3, 4), g), X.head_labels(2, 7, 9, 5, g, IGN)
    om = torch.randint(0, 17, (2, 7, 9), generator=g).double() / 8
    cw = torch.tensor([0.5, 1.0, 2.0, 0.0, 1.5], dtype=torch.float64)
    for norm in R.NORMS:
        for weight in (None, cw):
            ref = R.head_ref(x, labels, om, weight, norm, IGN, grad_out=0.7)
            r = R.pixel_weighted_ce(x, labels, om, class_weight=weight, norm=norm, grad_out=0.7)
            assert abs(ref.loss - r['loss']) <= 1e-13 * abs(r['loss']) and abs(ref.den - float(r['n'].sum())) <= 1e-12
            assert float((ref.g - r['grad']).abs().max()) <= 1e-14
            assert bool((ref.A >= ref.g.abs() - 1e-15).all()) and ref.S >= abs(ref.loss) * ref.den - 1e-12


def test_mix_plane_restatement():
    labels = np.array([[[0, 1, 2, 3]], [[3, 2, 1, 0]]], dtype=np.uint8)
    plane = np.arange(8, dtype=np.int32).reshape(2, 1, 4)
    sel = np.zeros((2, 256), dtype=np.uint8)
    sel[0, [1, 3]] = 1
    sel[1, 2] = 1
    out = R.mix_plane(plane, labels, [1, 0], sel=sel)
    assert out.tolist() == [[[4, 1, 6, 3]], [[0, 5, 2, 3]]]
    out = R.mix_plane(plane, labels, [1, 1], boxes=[[0, 1, 1, 3], [0, 0, 0, 0]])
    assert out.tolist() == [[[4, 1, 2, 7]], [[4, 5, 6, 7]]]


def test_host_validation_raises_before_any_device_access():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    cpu = torch.device('cpu')
    om = torch.ones((3, 4, 4))
    ops.check_pixel_weight(om, (3, 4, 4), cpu)
    for bad in (om.double(), om[:2], om[:, :, :3], om.transpose(1, 2), om.numpy(), None, 1.0):      # dtype, shape, strides, no tensor
        with pytest.raises(ValueError):
            ops.check_pixel_weight(bad, (3, 4, 4), cpu)
    with pytest.raises(ValueError):                                           # a map that lives elsewhere than the logits
        ops.check_pixel_weight(om, (3, 4, 4), torch.device('cuda', 0))
    with pytest.raises(ValueError):
        ops.check_pixel_weight(om, (3, 4, 4), cpu, 'mean')
    low, t = torch.zeros((3, 5, 2, 2)), torch.zeros((3, 4, 4), dtype=torch.int64)
    call = lambda **kw: tssa.upsample_pixel_weighted_cross_entropy(low, t, om, size=(4, 4), **kw)
    for kw in (dict(pixel_norm='mean'), dict(label_smoothing=0.1), dict(sample_weight=[1.0, 1.0, 1.0]), dict(sample_group=[0, 1, 3])):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):           # more classes than the fused head takes: no unfused route
        tssa.upsample_pixel_weighted_cross_entropy(torch.zeros((3, 257, 2, 2)), t, om, size=(4, 4))
    with pytest.raises(ValueError):           # an output smaller than the map
        tssa.upsample_pixel_weighted_cross_entropy(torch.zeros((3, 5, 8, 8)), t, om, size=(4, 4))
    ce = tssa.CrossEntropyLoss(ignore_index=IGN)
    for bad, norm in ((om, 'weight'), (om.numpy(), 'weight')):           # a host map
        with pytest.raises(ValueError):
            ce.set_pixel_weight(bad, norm)
    with pytest.raises(ValueError):
        ce.set_pixel_weight(om, 'mean')
    with pytest.raises(ValueError):
        tssa.CrossEntropyLoss(ignore_index=IGN, label_smoothing=0.1).set_pixel_weight(om)


def test_public_surface():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import _native as N, ops
    p = inspect.signature(tssa.upsample_pixel_weighted_cross_entropy).parameters
    assert list(p) == ['low', 'target', 'pixel_weight', 'scale_factor', 'size', 'ignore_index', 'weight', 'label_smoothing', 'pixel_norm',
                       'sample_group', 'sample_weight', 'group_loss_out'] and p['pixel_norm'].default == 'weight'
    assert tssa.upsample_pixel_weighted_cross_entropy is ops.upsample_pixel_weighted_cross_entropy
    assert 'pixel_weight' not in inspect.signature(tssa.upsample_cross_entropy).parameters      # the plain function keeps its parameters
    assert tssa.UpsamplePixelWeightedCrossEntropyFn is ops.UpsamplePixelWeightedCrossEntropyFn
    assert ops.PIXEL_NORMS == {'weight': 0, 'valid': 1, 'pixels': 2}
    ce = tssa.CrossEntropyLoss(ignore_index=IGN)
    assert ce.pixel_weight is None and ce.pixel_norm == 'weight' and 'pixel_weight' not in ce.state_dict()
    ce.clear_pixel_weight()
    p = inspect.signature(tssa.SelfTraining.__init__).parameters
    assert p['pixel_weighting'].default is None and p['pixel_norm'].default == 'weight'
    assert list(inspect.signature(tssa.mix_plane).parameters) == ['plane', 'labels', 'partner', 'sel', 'boxes', 'out']
    assert 'out_confidence' in inspect.signature(tssa.upsample_pseudo_labels).parameters
    decls = N.parse_header()
    for name in ('tss_upsample_ce_pixw_fwd', 'tss_upsample_ce_pixw_coef_wide', 'tss_mix_plane'):
        assert name in decls, name
    assert hasattr(N.lib(), 'tss_upsample_ce_pixw_fwd')
