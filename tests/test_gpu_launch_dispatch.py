"""GPU: the dtype dispatch of the C entry points that the other suites reach in one dtype only (or in one of several
dtype pairs): each case runs the public operator in float32 and in bfloat16 and compares with the plain torch formula
on the same inputs, so a wrong template instance or pointer cast in either branch shows.

Bounds.  float32: the bound of the operator's existing test (cited per case).  bfloat16: the bound of the operator's
existing bf16 test where there is one (the upsampled cross-entropy / OHEM / argmax family).  bilinear, upsample_logits,
adaptive_avg_pool, resize_image and gate are held elementwise, in both dtypes and at the C ABI, by
tests/test_gpu_resample_exact.py (bit for bit or to a derived bound on dyadic operands); the norm-wise bf16 bound used for them
here is derived from the number format: the kernels compute in f32 from the bf16 inputs and round every output element
once, so an element is off by at most half a bf16 ulp, which is 2**-8 relative (8 significand bits), and so is the
relative L2 error (one rounding typically gives about 1.1e-3; a wrong instance or cast gives O(1)).  BF16 below adds the
operator's f32 bound to that.  The reference of a bf16 case is the f32 formula on the same bf16 values.  (The upsampled
cross-entropy / OHEM / argmax family already runs in both dtypes and both class-register instances in test_gpu_ops.py;
its C = 19 and C = 21 cases are repeated here at 8x8 -> 32x32 with the bounds of those tests.)
"""
import pytest
import torch
import torch.nn.functional as F

from tests import cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = [torch.float32, torch.bfloat16]
BF16 = 2.0 ** -8 + 1e-5


def rel(a, b):
    return cases.rel_err(a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy())


def bound(dtype, f32_bound):
    return f32_bound if dtype == torch.float32 else BF16


def sliced(B, C, H, W, dtype, seed):
    """An NHWC activation of C channels that is a channel slice of a wider buffer (pitch 2C != C)."""
    from torch_semantic_segmentation_amd import ops
    torch.manual_seed(seed)
    wide = ops.new_nhwc(B, 2 * C, H, W, dtype, DEV)
    wide.copy_(torch.randn(B, 2 * C, H, W, device=DEV))
    x = wide[:, :C]
    assert ops.ld(x) == 2 * C
    return x


@pytest.mark.parametrize('dtype', DTYPES)
def test_bilinear_both_dtypes(dtype):
    """tss_bilinear_nhwc_fwd / _bwd; f32 bound 1e-5 as test_gpu_ops.py::test_bilinear_nhwc_fwd_bwd."""
    from torch_semantic_segmentation_amd import ops
    x = sliced(2, 16, 8, 8, dtype, 11)
    cot = torch.randn(2, 16, 12, 20, device=DEV).to(dtype)
    a = x.detach().requires_grad_(True)
    ya = ops.bilinear(a, size=(12, 20))
    ya.backward(cot)
    b = x.detach().float().requires_grad_(True)
    yb = F.interpolate(b, size=(12, 20), mode='bilinear', align_corners=True)
    yb.backward(cot.float())
    assert ya.dtype == dtype and a.grad.dtype == dtype
    assert rel(ya, yb) < bound(dtype, 1e-5) and rel(a.grad, b.grad) < bound(dtype, 1e-5)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [19, 21])
def test_upsample_logits_both_dtypes(C, dtype):
    """tss_upsample_head_fwd / _bwd (8 x 8 -> 32 x 32: the class-vector kernel); f32 bound 1e-5 as
    test_gpu_ops.py::test_upsample_head_fwd_bwd."""
    from torch_semantic_segmentation_amd import ops
    torch.manual_seed(12)
    low = torch.randn(2, C, 8, 8, device=DEV).to(dtype)
    cot = torch.randn(2, C, 32, 32, device=DEV).to(dtype)
    a = ops.to_nhwc(low).clone().requires_grad_(True)
    ya = ops.upsample_logits(a, size=(32, 32))
    ya.backward(cot)
    b = low.float().clone().requires_grad_(True)
    yb = F.interpolate(b, size=(32, 32), mode='bilinear', align_corners=True)
    yb.backward(cot.float())
    assert ya.dtype == dtype
    assert rel(ya, yb) < bound(dtype, 1e-5) and rel(a.grad, b.grad) < bound(dtype, 1e-5)


@pytest.mark.parametrize('dtype', DTYPES)
def test_adaptive_pool_both_dtypes(dtype):
    """tss_adaptive_pool_fwd / _bwd; f32 bound 1e-5 as test_gpu_ops.py::test_adaptive_pool_fwd_bwd."""
    from torch_semantic_segmentation_amd import ops
    x = sliced(2, 16, 8, 8, dtype, 13)
    cot = torch.randn(2, 16, 3, 3, device=DEV).to(dtype)
    a = x.detach().requires_grad_(True)
    ya = ops.adaptive_avg_pool(a, 3)
    ya.backward(cot)
    b = x.detach().float().requires_grad_(True)
    yb = F.adaptive_avg_pool2d(b, 3)
    yb.backward(cot.float())
    assert rel(ya, yb) < bound(dtype, 1e-5) and rel(a.grad, b.grad) < bound(dtype, 1e-5)


@pytest.mark.parametrize('out_dtype', DTYPES)
@pytest.mark.parametrize('in_dtype', DTYPES)
def test_resize_image_every_dtype_pair(in_dtype, out_dtype):
    """tss_bilinear_planar_fwd, its four (input, output) instances; f32 bound 1e-5 as
    test_gpu_ops.py::test_resize_image_matches_interpolate, a bf16 output adds its one rounding."""
    from torch_semantic_segmentation_amd import ops
    torch.manual_seed(14)
    x = torch.randn(2, 3, 8, 8, device=DEV).to(in_dtype)
    y = ops.resize_image(x, size=(12, 20), out_dtype=out_dtype)
    ref = F.interpolate(x.float(), size=(12, 20), mode='bilinear', align_corners=True)
    assert y.dtype == out_dtype and y.shape == ref.shape
    assert rel(y, ref) < bound(out_dtype, 1e-5)


def lowres_case(C, dtype, seed):
    torch.manual_seed(seed)
    low = (2 * torch.randn(2, C, 8, 8, device=DEV)).to(dtype)
    target = torch.randint(0, C, (2, 32, 32), device=DEV)
    target[1, 5, 7] = 255                                  # one ignored pixel
    return low, target


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [19, 21])
def test_argmax_confusion_both_dtypes(C, dtype):
    """tss_argmax_confusion and tss_upsample_argmax_confusion (20- and 24-register instance): exact, as
    test_gpu_ops.py::test_argmax_confusion_matches_torch (the full-resolution one is float32 only there)."""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    low, target = lowres_case(C, dtype, 15)
    full = F.interpolate(low.float(), size=(32, 32), mode='bilinear', align_corners=True).to(dtype)
    pred, cm = tssa.argmax_confusion(full, target, ignore_index=255)
    ref = full.float().argmax(1)
    valid = target != 255
    assert (pred.long() == ref).all()
    assert (cm == torch.bincount(target[valid] * C + ref[valid], minlength=C * C).view(C, C)).all()
    # the fused head: mismatch fraction against the argmax of the f32 interpolation at most 1e-4 (f32) / 5e-3 (bf16) and the
    # matrix of its own predictions exactly, as test_gpu_ops.py::test_fused_upsample_argmax_confusion_matches_unfused
    pred_u, cm_u = tssa.upsample_argmax_confusion(ops.to_nhwc(low), target, size=(32, 32), ignore_index=255)
    up = F.interpolate(low.float(), size=(32, 32), mode='bilinear', align_corners=True)
    assert (pred_u.long() != up.argmax(1)).float().mean().item() <= (1e-4 if dtype == torch.float32 else 5e-3)
    assert (cm_u == torch.bincount(target[valid] * C + pred_u.long()[valid], minlength=C * C).view(C, C)).all()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [19, 21])
def test_upsample_cross_entropy_and_ohem_both_dtypes(C, dtype):
    """tss_upsample_ce_fwd / _bwd, tss_upsample_pixel_ce, tss_upsample_ohem_grad.  Cross-entropy: bounds 2e-5 (f32) and
    2e-2 (bf16) as test_gpu_ops.py::test_fused_upsample_cross_entropy_matches_unfused."""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    low, target = lowres_case(C, dtype, 16)
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    b = low.float().clone().requires_grad_(True)
    up = F.interpolate(b, size=(32, 32), mode='bilinear', align_corners=True)
    lb = F.cross_entropy(up, target, ignore_index=255)
    lb.backward()
    a = ops.to_nhwc(low).clone().requires_grad_(True)
    la = tssa.upsample_cross_entropy(a, target, size=(32, 32), ignore_index=255)
    la.backward()
    assert abs(la.item() / lb.item() - 1) < tol and rel(a.grad, b.grad) < tol
    # the same head under OHEM, threshold branch; bounds 5e-5 (f32) and 1e-2 (bf16) as
    # test_gpu_ops.py::test_upsample_ohem_from_lowres_logits_matches_the_unfused_pair, reference: the oracle's formula
    from oracle.recipe import ohem
    tol = 5e-5 if dtype == torch.float32 else 1e-2
    c = low.float().clone().requires_grad_(True)
    lc = ohem(F.interpolate(c, size=(32, 32), mode='bilinear', align_corners=True), target, ignore_index=255,
              thresh_loss=0.35667494393873245, numel_frac=0.05)
    lc.backward()
    a2 = ops.to_nhwc(low).clone().requires_grad_(True)
    lo = ops.upsample_ohem_loss(a2, target, size=(32, 32), ignore_index=255, thresh_loss=0.35667494393873245, numel_frac=0.05)
    lo.backward()
    assert abs(lo.item() / lc.item() - 1) < tol and rel(a2.grad, c.grad) < tol


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('add_one', [False, True])
def test_gate_both_dtypes(add_one, dtype):
    """tss_gate_fwd / tss_gate_bwd: x * (sigmoid(a) + add_one), a = one value per image and channel.  f32: max |diff| <=
    1e-3 max |ref| + 2e-4, the criterion of test_gpu_zoo.py::test_pspnet_head_matches_reference, the only test that reaches
    the gate (bise_arm / bise_ffm, float32 only).  bf16: one rounding per output element on top of that relative 1e-3."""
    import numpy as np
    from torch_semantic_segmentation_amd import ops
    x = sliced(2, 16, 8, 8, dtype, 17)
    att = ops.new_nhwc(2, 16, 1, 1, dtype, DEV)
    att.copy_(torch.randn(2, 16, 1, 1, device=DEV))
    cot = torch.randn(2, 16, 8, 8, device=DEV).to(dtype)
    xa, aa = x.detach().requires_grad_(True), att.detach().requires_grad_(True)
    ya = ops.gate(xa, aa, add_one=add_one)
    ya.backward(cot)
    xb, ab = x.detach().float().requires_grad_(True), att.detach().float().requires_grad_(True)
    yb = xb * (torch.sigmoid(ab) + (1.0 if add_one else 0.0))
    yb.backward(cot.float())
    assert ya.dtype == dtype and xa.grad.dtype == dtype and aa.grad.dtype == dtype
    for got, want in ((ya, yb), (xa.grad, xb.grad), (aa.grad, ab.grad)):
        if dtype == torch.float32:
            g, w = got.detach().cpu().double().numpy(), want.detach().cpu().double().numpy()
            assert np.abs(g - w).max() <= 1e-3 * np.abs(w).max() + 2e-4
        else:
            assert rel(got, want) < 2.0 ** -8 + 1e-3


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [19, 21])
def test_upsample_head_bwd_cols_alone_equals_the_two_pass_backward(C, dtype):
    """tss_upsample_head_bwd_cols (no Python caller): the column pass of tss_upsample_head_bwd on its own.  Run on the f32
    row buffer that tss_upsample_head_bwd left, it is the same kernel on the same input: bit equality."""
    from torch_semantic_segmentation_amd import _native as N
    torch.manual_seed(18)
    B, h, w, H, W = 2, 8, 8, 32, 32
    ldl = (C + 7) // 8 * 8
    dy = torch.randn(B, C, H, W, device=DEV).to(dtype)
    tmp = torch.empty(B * C * h * W, dtype=torch.float32, device=DEV)
    both = torch.zeros(B, h, w, ldl, dtype=dtype, device=DEV)
    cols = torch.zeros(B, h, w, ldl, dtype=dtype, device=DEV)
    code = N.dtype_code(dtype)
    N.call('tss_upsample_head_bwd', N.ptr(dy), None, N.ptr(tmp), N.ptr(both), ldl, B, C, h, w, H, W, code, N.stream())
    N.call('tss_upsample_head_bwd_cols', N.ptr(tmp), N.ptr(cols), ldl, B, C, h, w, W, code, N.stream())
    assert float(both.float().abs().max()) > 0 and torch.equal(both, cols)
    # and the pair is the gradient of the interpolation (f32 bound of test_gpu_ops.py::test_upsample_head_fwd_bwd, BF16 rule above)
    low = torch.zeros(B, C, h, w, device=DEV, requires_grad=True)
    F.interpolate(low, size=(H, W), mode='bilinear', align_corners=True).backward(dy.float())
    assert rel(cols.permute(0, 3, 1, 2)[:, :C], low.grad) < bound(dtype, 1e-5)


@pytest.mark.parametrize('dtype', DTYPES)
def test_concat_slice_and_split_glue_both_dtypes(dtype):
    """tss_copy_nhwc (concat), tss_pad_channels (gradient of channel_slice) and tss_cat2_add (gradient of split_fork): copies
    and one addition rounded once, bit-exact in both dtypes as test_gpu_zoo_exact.py::
    test_channel_shuffle_cat2_add_pad_channels_are_bit_exact asserts for them in bfloat16."""
    from torch_semantic_segmentation_amd import ops
    x, y = sliced(2, 16, 8, 8, dtype, 19), sliced(2, 8, 8, 8, dtype, 20)
    assert torch.equal(ops.concat([x, y]), torch.cat([x, y], 1))
    # channel_slice: the gradient is the incoming one padded with zero channels
    z = sliced(2, 16, 8, 8, dtype, 21).detach().requires_grad_(True)
    g = sliced(2, 8, 8, 8, dtype, 22)
    ops.channel_slice(z, 8).backward(g)
    assert z.grad.dtype == dtype and torch.equal(z.grad[:, :8], g) and not z.grad[:, 8:].any()
    # split_fork: cat(g_left, g_right) + g_skip, computed in f32 and rounded once
    s = sliced(2, 16, 8, 8, dtype, 23).detach().requires_grad_(True)
    left, right, skip = ops.split_fork(s)
    gl, gr, gs = sliced(2, 8, 8, 8, dtype, 24), sliced(2, 8, 8, 8, dtype, 25), sliced(2, 16, 8, 8, dtype, 26)
    torch.autograd.backward([left, right, skip], [gl, gr, gs])
    assert s.grad.dtype == dtype and torch.equal(s.grad, (torch.cat([gl, gr], 1).float() + gs.float()).to(dtype))
