"""GPU: the fused head, its losses and the evaluators for 24 < C <= 256 classes (csrc/widehead.hip, the tss_*_wide entries).

References (imported, not restated): tests/wce_ref.py in f64 for the cross-entropy, tests/msflip_ref.py for the arg-max kernels,
the unfused HIP pair and the torch formula for OHEM.  Helpers and bounds are those of tests/test_gpu_wce.py (loss: relative 2e-5;
gradient, f32: cases.rel_err <= max(2e-5, 3 d_ref); gradient, bf16: 2e-2), tests/test_gpu_msflip.py (`check`) and
tests/test_gpu_ops.py (the OHEM test).

Class counts: 25 (first past the register kernels; a one-class ragged chunk at 16 classes per chunk would be 17 and 33: 33 is in),
32 (two whole chunks), 66 (Mapillary, pitch 72), 130 (nine chunks, the last ragged), 256 (the limit); for the counters also 96 and
97, the last count whose C x C counters sit in LDS and the first that counts with 64-bit atomics on the matrix.
Labels as in tests/test_gpu_wce.py: about 10 % of 255, three -1, two 300, the last class absent, class 1 of weight exactly 0.

The multi-scale kernel performs, per score, exactly the roundings that msflip_ref.margin counts for the register kernel: the
maximum is taken over all classes before any exponential (a walk of its own), the sum adds the C exponentials in class order from 0,
the score is exp(z - m) * (1 / s) and the maps are added in list order.  No term is added to the margin.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import cases, msflip_ref as M, wce_ref as R
from tests.test_gpu_msflip import DTYPES as MS_DTYPES, check as ms_check, fused as ms_fused, inputs as ms_inputs
from tests.test_gpu_wce import check, class_weights, drop_last_class, hip_fused, reference, tag_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 0.1
DTYPES = pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
COMBOS = pytest.mark.parametrize('weighted,eps', [(True, 0.0), (False, EPS), (True, EPS), (False, 0.0)], ids=['w', 'eps', 'w_eps', 'plain'])

#          low-res shape,     scale   path reached
WIDE = {
    'c25':     ((2, 25, 8, 16), 8),       # first count past the register kernels: chunks of 16 + 9
    'edge':    ((1, 66, 5, 7), 8),        # lanes past the image edge, odd rows; last chunk holds two classes
    'strips':  ((1, 66, 4, 33), 8),       # two strips with an 8-lane second
    'bands':   ((3, 66, 70, 36), 2),      # several bands, odd batch
    'scale1':  ((1, 130, 9, 300), 1),     # a flush every row, rB == rA at the end; nine chunks
    'c256':    ((1, 256, 6, 4), 4),       # the limit: sixteen whole chunks
    'c33':     ((1, 33, 5, 7), 4),        # a one-class ragged chunk
    'c32':     ((2, 32, 6, 4), 4),        # whole chunks only, pitch == C
}


@functools.lru_cache(maxsize=None)
def wide_input(name, bf16):
    (B, C, h, w), scale = WIDE[name]
    g = torch.Generator().manual_seed(sorted(WIDE).index(name) + 1900)
    low = 2.0 * torch.randn(B, C, h, w, generator=g)
    if bf16:
        low = low.bfloat16().float()
    H, W = h * scale, w * scale
    target = torch.randint(0, C, (B, H, W), generator=g)
    target = drop_last_class(target, C)
    target[torch.rand(B, H, W, generator=g) < 0.10] = 255
    flat = target.view(-1)
    flat[[3, 17, 40]] = -1
    flat[[5, 29]] = 300
    return low, target, class_weights(target, C)


@functools.lru_cache(maxsize=None)
def wide_reference(name, bf16, weighted, eps):
    low, target, w = wide_input(name, bf16)
    return reference(R.upsampled_wce_loss, low, target, w if weighted else None, eps)


# ----------------------------------------------------------------------------- 1. cross-entropy

@COMBOS
@DTYPES
@pytest.mark.parametrize('name', list(WIDE))
def test_wide_loss_and_gradient_vs_f64_restatement(name, dtype, weighted, eps):
    bf16 = dtype == torch.bfloat16
    low, target, w = wide_input(name, bf16)
    got = hip_fused(low, target, w if weighted else None, eps, WIDE[name][1], dtype)
    check(tag_of('wide', name, bf16, weighted, eps), got, wide_reference(name, bf16, weighted, eps), bf16)
    again = hip_fused(low, target, w if weighted else None, eps, WIDE[name][1], dtype)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])          # the same bits on every run


@COMBOS
@DTYPES
@pytest.mark.parametrize('name', list(WIDE))
def test_wide_pass_writes_every_workspace_element_that_the_gather_reads(name, dtype, weighted, eps):
    """Through the C ABI with a NaN-filled workspace and a NaN-filled gradient: finite, the bits of the autograd path, pad channels 0."""
    from torch_semantic_segmentation_amd import _native as N, ops
    low, target, w = wide_input(name, dtype == torch.bfloat16)
    (B, C, h, wd), scale = WIDE[name]
    H, W = h * scale, wd * scale
    want_loss, want_grad = hip_fused(low, target, w if weighted else None, eps, scale, dtype, scale=0.7)
    ad, t = ops.to_nhwc(low.to(DEV).to(dtype)), target.to(DEV)
    assert ad.stride(3) % 8 == 0 and ad.stride(3) >= C
    wdev = w.to(DEV) if weighted else None
    nws = N.lib().tss_upsample_ce_wide_ws(B, C, h, wd, H, W)
    assert nws > 0
    ws = torch.full((nws,), float('nan'), device=DEV)
    scal = torch.full((2,), float('nan'), device=DEV)
    N.call('tss_upsample_ce_wide_fwd', N.ptr(ad), ad.stride(3), N.ptr(t), N.ptr(wdev), eps, N.ptr(ws), N.ptr(scal[0:1]), N.ptr(scal[1:2]),
           B, C, h, wd, H, W, 255, N.dtype_code(ad.dtype), N.stream())
    out = torch.full((B, h, wd, ad.stride(3)), float('nan'), dtype=ad.dtype, device=DEV)
    gout = torch.tensor([0.7], device=DEV)
    N.call('tss_upsample_ce_wide_bwd', N.ptr(ws), N.ptr(scal[1:2]), N.ptr(gout), N.ptr(out), ad.stride(3), B, C, h, wd, H, W,
           N.dtype_code(ad.dtype), N.stream())
    assert torch.isfinite(out.float()).all() and torch.isfinite(scal).all()
    assert torch.equal(scal[0].cpu(), want_loss)
    assert torch.equal(out.permute(0, 3, 1, 2)[:, :C].float().cpu(), want_grad)
    assert (out[..., C:] == 0).all()


@pytest.mark.parametrize('name', ['c25', 'bands', 'scale1'])
def test_wide_grad_out_scales_the_gradient_linearly(name):
    low, target, w = wide_input(name, False)
    one = hip_fused(low, target, w, EPS, WIDE[name][1])
    scaled = hip_fused(low, target, w, EPS, WIDE[name][1], scale=0.7)
    assert torch.equal(one[0], scaled[0])
    assert cases.rel_err(scaled[1].numpy(), 0.7 * one[1].double().numpy()) <= 4 * 2.0 ** -24       # one product more, one rounding


@pytest.mark.parametrize('eps', [0.0, EPS])
@DTYPES
def test_wide_empty_denominator_gives_nan_and_a_zero_gradient(dtype, eps):
    """No valid pixel, and valid pixels whose class weight is 0 (class 1): what the register kernels give."""
    low, target, w = wide_input('edge', dtype == torch.bfloat16)
    for fill in (255, 1):
        t = torch.where(target == 255, target, torch.full_like(target, fill))
        loss, grad = hip_fused(low, t, w, eps, 8, dtype)
        assert torch.isnan(loss) and float(grad.abs().max()) == 0.0
    loss, grad = hip_fused(low, torch.full_like(target, 255), None, eps, 8, dtype)
    assert torch.isnan(loss) and float(grad.abs().max()) == 0.0


# ----------------------------------------------------------------------------- 2. chunk boundaries

@functools.lru_cache(maxsize=None)
def hot_input(C, hot):
    """Integer-valued logits in [-20, 0], class `hot` at +60 everywhere; labels as wide_input."""
    g = torch.Generator().manual_seed(77 + C + hot)
    low = -torch.randint(0, 21, (1, C, 5, 7), generator=g).float()
    low[:, hot] = 60.0
    target = torch.randint(0, C, (1, 40, 56), generator=g)
    target[torch.rand(1, 40, 56, generator=g) < 0.10] = 255
    return low, target


@pytest.mark.parametrize('eps', [0.0, EPS])
@pytest.mark.parametrize('where', ['last', 'first'])
@pytest.mark.parametrize('C', [25, 66, 130])
def test_hot_class_at_a_chunk_boundary(C, where, eps):
    """The running maximum jumps by 60 in the ragged last chunk (or sits in the first one and every later chunk is rescaled to nothing)."""
    low, target = hot_input(C, C - 1 if where == 'last' else 0)
    want = reference(R.upsampled_wce_loss, low, target, None, eps)
    check('hot %s C=%d eps %.1f' % (where, C, eps), hip_fused(low, target, None, eps, 8), want, False)


def tie_low(C=66):
    g = torch.Generator().manual_seed(5)
    low = torch.randint(-20, 1, (2, C, 5, 9), generator=g).float()
    low[:, 3] = 7.0
    low[:, 40] = low[:, 3]
    return low


def test_argmax_ties_across_chunks_go_to_the_lowest_index():
    """Planes 3 and 40 (chunks 0 and 2) are equal and the per-pixel maximum: 3 everywhere, in all three arg-max functions."""
    import torch_semantic_segmentation_amd as tssa
    low = tie_low()
    for dtype in (torch.float32, torch.bfloat16):
        pred, _ = tssa.upsample_argmax_confusion(low.to(DEV, dtype), scale_factor=8)
        assert int(pred.min()) == 3 and int(pred.max()) == 3
        for average in ('softmax', 'logits'):
            pred, _ = tssa.multiscale_argmax_confusion([low.to(DEV, dtype), low[:, :, :3, :4].to(DEV, dtype)], [False, True], size=(33, 70),
                                                       average=average)
            assert int(pred.min()) == 3 and int(pred.max()) == 3
        planar = F.interpolate(low, scale_factor=4, mode='nearest').to(DEV, dtype).contiguous()     # 20 x 36: whole 8-pixel groups
        pred, _ = tssa.argmax_confusion(planar)
        assert int(pred.min()) == 3 and int(pred.max()) == 3


# ----------------------------------------------------------------------------- 3. OHEM

def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('case', ['threshold', 'top_n', 'many_ignored'])
@pytest.mark.parametrize('geom', [(2, 66, 16, 32, 8), (1, 66, 9, 13, 4), (3, 130, 12, 20, 8)])
def test_wide_upsample_ohem_matches_the_formula_and_the_unfused_pair(geom, case, dtype):
    """tests/test_gpu_ops.py::test_upsample_ohem_from_lowres_logits_matches_the_unfused_pair at 66 and 130 classes: its cases, its bounds."""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    from oracle.recipe import ohem
    torch.manual_seed(23)
    B, C, h, w, scale = geom
    H, W = h * scale, w * scale
    gain, frac = (3.0, 0.05) if case == 'threshold' else (0.05, 0.01)
    low = (gain * torch.randn(B, C, h, w, device=DEV)).to(dtype)
    target = torch.randint(0, C, (B, H, W), device=DEV)
    # the top-n branch needs the n-th loss below the threshold: ln C plus a little at near-uniform logits
    thresh = 0.35667494393873245 if case == 'threshold' else float(torch.log(torch.tensor(float(C)))) + 0.66
    target[torch.rand(B, H, W, device=DEV) < (0.995 if case == 'many_ignored' else 0.1)] = 255
    assert (B * H * W) % 8 == 0

    def fused():
        a = low.clone().requires_grad_(True)
        la = ops.upsample_ohem_loss(a, target, scale_factor=scale, ignore_index=255, thresh_loss=thresh, numel_frac=frac)
        (0.7 * la).backward()
        return la.detach().clone(), a.grad.clone()
    la, ga = fused()
    b = low.float().clone().requires_grad_(True)
    up = F.interpolate(b, scale_factor=scale, mode='bilinear', align_corners=True)
    lb = ohem(up, target, ignore_index=255, thresh_loss=thresh, numel_frac=frac)
    (0.7 * lb).backward()
    per = F.cross_entropy(up.detach(), target, ignore_index=255, reduction='none').flatten()
    nth = torch.sort(per, descending=True)[0][int(per.numel() * frac)].item()
    assert (nth > thresh) == (case == 'threshold')
    tol = 5e-5 if dtype == torch.float32 else 1e-2
    print('ohem C=%d %s %s: loss rel %.2e grad rel %.2e' % (C, case, dtype, abs(la.item() / lb.item() - 1), rel(ga, b.grad)))
    assert abs(la.item() / lb.item() - 1) < tol, (la.item(), lb.item())
    assert rel(ga, b.grad) < tol
    if (dtype == torch.float32 or case == 'threshold') and W % 8 == 0:
        c = low.clone().requires_grad_(True)
        lc = tssa.OHEMLoss(ignore_index=255, thresh_loss=thresh, numel_frac=frac)(ops.upsample_logits(c, scale_factor=scale), target)
        (0.7 * lc).backward()
        assert abs(la.item() / lc.item() - 1) < (5e-5 if dtype == torch.float32 else 2e-2)
        assert rel(ga, c.grad) < (5e-5 if dtype == torch.float32 else 3e-2)
    l2, g2 = fused()
    assert torch.equal(g2, ga) and abs(l2.item() - la.item()) <= 1e-6 * abs(la.item())


# ----------------------------------------------------------------------------- 4. arg-max + confusion

def labels(shape, C, seed):
    g = torch.Generator().manual_seed(seed)
    target = torch.randint(0, C, shape, generator=g)
    target[torch.rand(shape, generator=g) < 0.1] = 255
    target[0, 0, :5] = C                                   # out of range: skipped like ignore_index
    target[-1, -1, -3:] = -2
    return target


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('C,h,w,scale', [(66, 5, 9, 8), (256, 6, 4, 4), (96, 3, 40, 8), (97, 3, 40, 8)])
def test_wide_upsample_argmax_confusion(C, h, w, scale, dtype):
    import torch_semantic_segmentation_amd as tssa
    size = (h * scale, w * scale)
    low = (torch.randn(2, C, h, w, generator=torch.Generator().manual_seed(C)) * 4).bfloat16().float()
    score, want = M.scores([low], [False], size, 'logits')
    m = M.margin(1, C, float(low.abs().max()), [(h, w)], size, 'logits')
    decided = M.top2_gap(score) > m
    target = labels((2,) + size, C, 3)
    td = target.to(DEV)
    pred, cm = tssa.upsample_argmax_confusion(low.to(DEV, MS_DTYPES[dtype]), td, scale_factor=scale)
    assert pred.dtype == torch.uint8 and cm.dtype == torch.int64 and tuple(cm.shape) == (C, C)
    wrong = int(((pred.cpu().long() != want) & decided).sum())
    print('upsample argmax C=%d %s: margin %.3e undecided %.4f wrong %d' % (C, dtype, m, 1 - float(decided.double().mean()), wrong))
    assert wrong == 0 and float(decided.double().mean()) >= 0.99
    counts = M.confusion(pred.cpu(), target, C)
    assert torch.equal(cm.cpu(), counts) and int(cm.sum()) == int(((target >= 0) & (target < C) & (target != 255)).sum())
    pred2, cm2 = tssa.upsample_argmax_confusion(low.to(DEV, MS_DTYPES[dtype]), td, scale_factor=scale, confusion=cm.clone(), want_pred=False)
    assert pred2 is None and torch.equal(cm2.cpu(), 2 * counts)


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('C', [65, 96, 97, 256])
def test_wide_planar_argmax_confusion_is_exact(C, dtype):
    """Integer-valued logits without ties (a permutation of 0 .. C-1 per pixel, exact in bf16): torch.argmax, bit for bit."""
    import torch_semantic_segmentation_amd as tssa
    g = torch.Generator().manual_seed(C)
    B, H, W = 3, 9, 40                                     # 360 pixels per image: 45 groups, two blocks' worth over the batch
    logits = torch.rand(B, H, W, C, generator=g).argsort(-1).permute(0, 3, 1, 2).float().contiguous()
    target = labels((B, H, W), C, 4)
    pred, cm = tssa.argmax_confusion(logits.to(DEV, MS_DTYPES[dtype]), target.to(DEV))
    assert torch.equal(pred.cpu().long(), logits.argmax(1))
    assert torch.equal(cm.cpu(), M.confusion(pred.cpu(), target, C))
    _, cm2 = tssa.argmax_confusion(logits.to(DEV, MS_DTYPES[dtype]), target.to(DEV), confusion=cm.clone(), want_pred=False)
    assert torch.equal(cm2.cpu(), 2 * M.confusion(pred.cpu(), target, C))


# ----------------------------------------------------------------------------- 5. multi-scale

@pytest.mark.parametrize('average', ['softmax', 'logits'])
@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('C', [25, 66, 130, 256])
@pytest.mark.parametrize('geometry', ['twelve', 'odd', 'single'])
def test_wide_multiscale_prediction_matches_the_restatement(geometry, C, dtype, average):
    (lows, flips), out = ms_inputs(geometry, C)
    pred, cm = ms_fused(lows, flips, out, MS_DTYPES[dtype], average)
    assert cm is None and pred.dtype == torch.uint8 and tuple(pred.shape) == (2,) + tuple(out)
    ms_check(pred, geometry, C, average, None, 'wide %s C=%d %s %s' % (geometry, C, dtype, average))
    if geometry == 'twelve':
        packed = [torch.cat([lows[i], lows[i + 1]]) for i in range(0, len(lows), 2)]
        pred2, _ = ms_fused(packed, [(False, True)] * len(packed), out, MS_DTYPES[dtype], average)
        assert torch.equal(pred2, pred)


@pytest.mark.parametrize('C', [66, 97])
def test_wide_multiscale_confusion_matrix_is_exact(C):
    (lows, flips), out = ms_inputs('odd', C)
    target = labels((2,) + tuple(out), C, 3)
    td = target.to(DEV)
    pred, cm = ms_fused(lows, flips, out, torch.bfloat16, 'softmax', target=td)
    want = M.confusion(pred.cpu(), target, C)
    assert torch.equal(cm.cpu(), want) and int(cm.sum()) == int(((target >= 0) & (target < C) & (target != 255)).sum())
    pred2, cm2 = ms_fused(lows, flips, out, torch.bfloat16, 'softmax', target=td, confusion=cm.clone(), want_pred=False)
    assert pred2 is None and torch.equal(cm2.cpu(), 2 * want)


# ----------------------------------------------------------------------------- 6. what the parent commit cannot do

def model66(name='fastscnn'):
    from oracle.recipe import formula_state
    m = cases.product_model(name, 3, 66)
    m.load_state_dict(formula_state(m), strict=True)
    cases.zero_dropout(m)
    return m.to(DEV)


def batches66():
    from oracle.recipe import lattice_input, lattice_target
    out = []
    for i in range(2):
        y = lattice_target(2, 64, 128).roll(i, -1)
        y = torch.where(y == 255, y, (y * 7 + i) % 66)          # 66 classes out of the lattice's 19, the 255s kept
        out.append((lattice_input(2, 3, 64, 128).mul(1.0 + 0.25 * i), y))
    return out


def test_evaluators_run_with_66_classes():
    from torch_semantic_segmentation_amd import engine as E, ops
    m = model66()
    data = batches66()
    got = E.Evaluator(m, DEV, num_classes=66).run(data)
    ms = E.MultiScaleEvaluator(m, DEV, num_classes=66, scales=(0.5, 1.0), flip=True)
    got_ms = ms.run(data)
    n_valid = sum(int((y != 255).sum()) for _, y in data)
    assert got['iou'].shape == (66,) and got_ms['iou'].shape == (66,) and int(ms.confusion.sum()) == n_valid
    # the evaluators' metrics are exactly those of the hand-made calls; the planar arg-max of the model's own full-resolution
    # logits (also a wide entry: C > 64) counts the same pixels
    cm, cm_ms, cm_planar = None, None, None
    with torch.no_grad(), E.EvalPrep(m):
        for x, y in data:
            x, y = x.to(DEV), y.to(DEV)
            _, cm = ops.upsample_argmax_confusion(m.forward_lowres(x), y, scale_factor=m.logit_scale, confusion=cm, want_pred=False)
            lows = [m.forward_lowres(ops.resize_flip_image(x, s)) for s in ((32, 64), (64, 128))]
            _, cm_ms = ops.multiscale_argmax_confusion(lows, [(False, True)] * 2, y, size=(64, 128), confusion=cm_ms, want_pred=False)
            logits = m(x)
            assert logits.shape[1] == 66
            _, cm_planar = ops.argmax_confusion(logits, y, confusion=cm_planar, want_pred=False)
    assert int(cm.sum()) == n_valid and int(cm_planar.sum()) == n_valid and torch.equal(ms.confusion, cm_ms)
    want = E.confusion_metrics(cm.cpu().double())
    print('mIoU fused %.6f multi-scale %.6f' % (got['miou'], got_ms['miou']))
    assert torch.equal(got['iou'], want['iou']) and got['accuracy'] == want['accuracy']


@pytest.mark.parametrize('name', ['fastscnn', 'contextnet14'])
def test_models_with_66_classes_run_forward_lowres(name):
    from torch_semantic_segmentation_amd import ops
    from oracle.recipe import lattice_input
    m = model66(name).eval()
    with torch.no_grad():
        low = ops.to_nhwc(ops.materialize(m.forward_lowres(lattice_input(2, 3, 64, 128).to(DEV))))
    assert low.shape[1] == 66 and low.stride(3) == 72 and bool(torch.isfinite(low.float()).all())


def test_wide_entries_exist_and_answer_at_25_classes():
    from torch_semantic_segmentation_amd import _native as N, ops
    lib, ptr, st = N.lib(), N.ptr, N.stream()
    assert lib.tss_widehead_max_classes() == 256 == ops.WIDEHEAD_MAX_CLASSES
    low = torch.zeros(1, 4, 8, 32, device=DEV)
    tt = torch.zeros(1, 8, 16, dtype=torch.int64, device=DEV)
    n = lib.tss_upsample_ce_wide_ws(1, 25, 4, 8, 8, 16)
    assert n > 0
    ws, scal = torch.empty(n, device=DEV), torch.empty(2, device=DEV)
    pix, sel = torch.empty(1, 8, 16, device=DEV), torch.tensor([0.0, 0.5, 1.0, 0.0], device=DEV)
    dl = torch.empty(1, 4, 8, 32, device=DEV)
    pred, cm = torch.empty(1, 8, 16, dtype=torch.uint8, device=DEV), torch.zeros(25, 25, dtype=torch.int64, device=DEV)
    geo = (1, 25, 4, 8, 8, 16)
    assert lib.tss_upsample_ce_wide_fwd(ptr(low), 32, ptr(tt), None, 0.0, ptr(ws), ptr(scal[0:1]), ptr(scal[1:2]), *geo, 255, 0, st) == 0
    assert lib.tss_upsample_ce_wide_bwd(ptr(ws), ptr(scal[1:2]), None, ptr(dl), 32, *geo, 0, st) == 0
    assert lib.tss_upsample_pixel_ce_wide(ptr(low), 32, ptr(tt), ptr(pix), *geo, 255, 0, st) == 0
    assert lib.tss_upsample_ohem_grad_wide(ptr(low), 32, ptr(tt), ptr(pix), ptr(sel), ptr(ws), *geo, 255, 0, st) == 0
    assert lib.tss_upsample_argmax_confusion_wide(ptr(low), 32, ptr(tt), ptr(pred), ptr(cm), *geo, 255, 0, st) == 0
    assert int(cm[0, 0]) == 128 and int(pred.max()) == 0
    maps = (ops._MsMap * 1)(ops._MsMap(low.data_ptr(), 32, 4, 8, 0, 0))
    assert lib.tss_multiscale_argmax_confusion_wide(maps, 1, ptr(tt), ptr(pred), ptr(cm), 1, 25, 8, 16, 255, 0, 0, st) == 0
    planar = torch.zeros(1, 25, 8, 16, device=DEV)
    assert lib.tss_argmax_confusion_wide(ptr(planar), ptr(tt), ptr(pred), ptr(cm), 1, 25, 128, 255, 0, st) == 0
    assert int(cm[0, 0]) == 3 * 128 and abs(float(scal[0]) - float(torch.log(torch.tensor(25.0)))) <= 2e-5 * 3.3


@pytest.mark.parametrize('loss', ['ce', 'ohem'])
def test_peak_memory_stays_below_half_the_full_resolution_logits(loss):
    """low = (1, 66, 16, 32), scale 8, f32: forward + backward may raise the peak by less than half of B C H W 4 bytes."""
    from torch_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(1)
    low = ops.to_nhwc(torch.randn(1, 66, 16, 32, generator=g).to(DEV)).clone().requires_grad_(True)
    target = torch.randint(0, 66, (1, 128, 256), generator=g).to(DEV)
    full = 1 * 66 * 128 * 256 * 4
    fn = ops.upsample_cross_entropy if loss == 'ce' else ops.upsample_ohem_loss
    fn(low, target, scale_factor=8, ignore_index=255).backward()          # warm: one-time buffers (OHEM's select workspace)
    low.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    fn(low, target, scale_factor=8, ignore_index=255).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print('%s: peak rise %.2f MB, full-resolution logits %.2f MB' % (loss, rise / 1e6, full / 1e6))
    assert rise < full / 2


# ----------------------------------------------------------------------------- 7. contract

def test_past_256_classes_the_losses_fall_back_and_the_argmax_functions_raise():
    import torch_semantic_segmentation_amd as tssa
    g = torch.Generator().manual_seed(43)
    low = 2.0 * torch.randn(1, 257, 4, 8, generator=g)
    target = torch.randint(0, 257, (1, 8, 16), generator=g)
    target[torch.rand(1, 8, 16, generator=g) < 0.1] = 255
    w = torch.rand(257, generator=g) * 49 + 1
    check('fallback C=257', hip_fused(low, target, w, EPS, 2), reference(R.upsampled_wce_loss, low, target, w, EPS), False)
    with pytest.raises(ValueError, match='256'):
        tssa.upsample_argmax_confusion(low.to(DEV), scale_factor=2)
    with pytest.raises(ValueError, match='256'):
        tssa.multiscale_argmax_confusion([low.to(DEV)], [False], size=(8, 16))
    with pytest.raises(ValueError, match='256'):
        tssa.argmax_confusion(torch.zeros(1, 257, 8, 16, device=DEV))


def test_wide_contract_errors_without_a_launch():
    from torch_semantic_segmentation_amd import _native as N, ops
    lib, ptr, st = N.lib(), N.ptr, N.stream()
    big = torch.zeros(1, 4, 8, 264, device=DEV)
    tt = torch.zeros(1, 8, 16, dtype=torch.int64, device=DEV)
    ws, scal = torch.empty(4096, device=DEV), torch.empty(2, device=DEV)
    pix, sel = torch.empty(1, 8, 16, device=DEV), torch.zeros(4, device=DEV)
    pred, cm = torch.empty(1, 8, 16, dtype=torch.uint8, device=DEV), torch.zeros(257 * 257, dtype=torch.int64, device=DEV)
    S = (ptr(scal[0:1]), ptr(scal[1:2]))

    def entries(ld, C, h, w, H, W, low=ptr(big), B=1, eps=0.0, dtype=0):
        geo = (B, C, h, w, H, W)
        return [lib.tss_upsample_ce_wide_fwd(low, ld, ptr(tt), None, eps, ptr(ws), *S, *geo, 255, dtype, st),
                lib.tss_upsample_pixel_ce_wide(low, ld, ptr(tt), ptr(pix), *geo, 255, dtype, st),
                lib.tss_upsample_ohem_grad_wide(low, ld, ptr(tt), ptr(pix), ptr(sel), ptr(ws), *geo, 255, dtype, st),
                lib.tss_upsample_ce_wide_bwd(ptr(ws), S[1], None, low, ld, *geo, dtype, st),
                lib.tss_upsample_argmax_confusion_wide(low, ld, ptr(tt), ptr(pred), ptr(cm), *geo, 255, dtype, st)]

    assert entries(264, 0, 4, 8, 8, 16) == [-2] * 5
    assert entries(264, 257, 4, 8, 8, 16) == [-2] * 5
    assert entries(260, 66, 4, 8, 8, 16) == [-2] * 5                  # ld % 8 != 0
    assert entries(64, 66, 4, 8, 8, 16) == [-2] * 5                   # ld < round_up(C, 4)
    assert entries(264, 66, 4, 8, 3, 16) == [-2] * 5                  # H < h
    assert entries(264, 66, 4, 8, 8, 16, dtype=7) == [-1] * 5
    for eps in (1.5, -0.1):
        assert lib.tss_upsample_ce_wide_fwd(ptr(big), 264, ptr(tt), None, eps, ptr(ws), *S, 1, 66, 4, 8, 8, 16, 255, 0, st) == -2
    assert entries(264, 66, 4, 8, 8, 16, low=ptr(big) + 4) == [-3] * 5
    assert entries(264, 66, 4, 8, 8, 16, B=0) == [0] * 5              # empty work
    assert lib.tss_upsample_ce_wide_ws(1, 257, 4, 8, 8, 16) == 0 and lib.tss_upsample_ce_wide_ws(1, 0, 4, 8, 8, 16) == 0
    assert lib.tss_upsample_ce_wide_ws(1, 66, 4, 8, 3, 16) == 0

    ms = lib.tss_multiscale_argmax_confusion_wide
    low = torch.zeros(2, 5, 9, 72, dtype=torch.bfloat16, device=DEV)
    maps = (ops._MsMap * 17)(*[ops._MsMap(low.data_ptr(), 72, 5, 9, 0, 0) for _ in range(17)])
    args = (None, ptr(pred), None)
    assert ms(maps, 17, *args, 1, 66, 40, 72, 255, 0, N.TSS_BF16, st) == -2
    assert ms(maps, 0, *args, 1, 66, 40, 72, 255, 0, N.TSS_BF16, st) == -2
    assert ms(maps, 1, *args, 1, 66, 40, 8, 255, 0, N.TSS_BF16, st) == -2          # w = 9 > W = 8
    assert ms(maps, 1, *args, 1, 257, 40, 72, 255, 0, N.TSS_BF16, st) == -2
    assert ms(maps, 1, *args, 1, 0, 40, 72, 255, 0, N.TSS_BF16, st) == -2
    assert ms(maps, 1, *args, 1, 66, 40, 72, 255, 2, N.TSS_BF16, st) == -2         # unknown mode
    assert ms(maps, 1, *args, 1, 66, 40, 72, 255, 0, 7, st) == -1
    bad_ld = (ops._MsMap * 1)(ops._MsMap(low.data_ptr(), 68, 5, 9, 0, 0))
    assert ms(bad_ld, 1, *args, 1, 66, 40, 72, 255, 0, N.TSS_BF16, st) == -2
    odd = (ops._MsMap * 1)(ops._MsMap(low.data_ptr() + 2, 72, 5, 9, 0, 0))
    assert ms(odd, 1, *args, 1, 66, 40, 72, 255, 0, N.TSS_BF16, st) == -3
    assert ms(maps, 1, *args, 0, 66, 40, 72, 255, 0, N.TSS_BF16, st) == 0          # empty work

    pl = lib.tss_argmax_confusion_wide
    planar = torch.zeros(1, 66, 8, 16, device=DEV)
    assert pl(ptr(planar), ptr(tt), ptr(pred), ptr(cm), 1, 257, 128, 255, 0, st) == -2
    assert pl(ptr(planar), ptr(tt), ptr(pred), ptr(cm), 1, 0, 128, 255, 0, st) == -2
    assert pl(ptr(planar), ptr(tt), ptr(pred), ptr(cm), 1, 66, 124, 255, 0, st) == -2          # HW % 8 != 0
    assert pl(ptr(planar), ptr(tt), ptr(pred), ptr(cm), 1, 66, 128, 255, 7, st) == -1
    assert pl(ptr(planar) + 4, ptr(tt), ptr(pred), ptr(cm), 1, 66, 128, 255, 0, st) == -3
    assert pl(ptr(planar), ptr(tt), ptr(pred), ptr(cm), 0, 66, 128, 255, 0, st) == 0
    torch.cuda.synchronize()
    assert int(cm.sum()) == 0                                                                  # nothing ran
