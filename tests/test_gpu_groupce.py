"""Per-sample loss groups on the fused head (csrc/groupce.hip; ops.upsample_cross_entropy's sample_group / sample_weight) on the GPU.

Shapes: every head_geom call here ends at band_rows = 16, so a sub-batch has the tile geometry, hence the loss rows and gradient tiles,
of the same samples inside the full batch -- what the comparisons against the ungrouped operator on a group's sub-batch rest on.
  ragged5 / 19 / 24   B=4, 4x7 -> 25x49: a ragged strip, both class-register variants
  bands               B=3, C=19, 5x40 -> 40x300: three bands x two strips, six rows per sample
  rows257             B=2, C=8, 2x2 -> 4112x8: 257 rows per sample, more than the finalize block's 256 threads
  wide66              B=3, C=66, 4x7 -> 25x49: the class-chunked path
Logits are multiples of 2^-2 in [-8, 8] (X.head_logits: exact in bf16, so both dtypes read the same numbers), labels carry ignored and
out-of-range pixels (X.head_labels).

Tolerances, none taken from what the kernels return:
  one group, lambda = 1, plain loss: counts are integers, scale[b] = fl32(1 / N) is the ungrouped inv_count, so the gradient equals the
    ungrouped operator's on bits; the loss differs by the order of two f64 sums: 1 f32 ulp.
  several groups against the ungrouped operator on each group's sub-batch, grad_out = 1 (what Trainer passes): group_loss[g] within 1 f32
    ulp of lambda L_g; a float32 gradient within 2 f32 ulp of lambda_b x the sub-batch gradient (the two sides round the quotient
    lambda / N and the product in a different order), a bf16 gradient within 1 bf16 ulp; both on bits for lambda a power of two (the
    scale is then the ungrouped one times a power of two, and so is every product).
  class weights / label smoothing: N_g is a sum of f32 weights, the two sides add the same rows in another order, so N differs by f64
    re-association (a few 2^-53, relative), which can move the f32 scale by one ulp: the loss gets 1 f32 ulp + that term, a float32
    gradient 2 more f32 ulp (a relative 2^-23 is up to 2 ulp of a number at the top of its binade), a bf16 gradient stays at 1 bf16 ulp.
  against tests/groupce_ref.py: the counted bounds of tests/exact.py (head_loss_bound, head_grad_bound, head_slack), which
    tests/test_gpu_head_exact.py holds the ungrouped loss and gradient to, per sample and scaled by lambda_b n_b / N_g: the grouped
    loss is the sum over the samples of lambda_b n_b / N_g times the sample's own mean, its gradient likewise, and the scale
    fl32(lambda / N) grad_out applied takes the three roundings that bound counts for fl32(1 / n) grad_out.
Every comparison prints its largest ratio as a line `GROUPCE_MARGIN ...` before it asserts."""
import math

import numpy as np
import pytest
import torch

from tests import exact as X
from tests import groupce_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IGN = 255
BF, F32 = torch.bfloat16, torch.float32
DT = {'f32': F32, 'bf16': BF}
GOUT = float(np.float32(0.7))

#          B   C  h  w   H    W
CASES = {'ragged5': (4, 5, 4, 7, 25, 49), 'ragged19': (4, 19, 4, 7, 25, 49), 'ragged24': (4, 24, 4, 7, 25, 49),
         'bands': (3, 19, 5, 40, 40, 300), 'rows257': (2, 8, 2, 2, 4112, 8), 'wide66': (3, 66, 4, 7, 25, 49)}
ROWS_PER_SAMPLE = {'ragged5': 2, 'ragged19': 2, 'ragged24': 2, 'bands': 6, 'rows257': 257, 'wide66': 2}
# (group ids, lambda): interleaved ids, ids with gaps, every sample its own group; lambda 0, powers of two, odd values
GROUPINGS = {4: [([0, 1, 0, 1], [1.0, 0.5, 1.0, 0.5]), ([3, 0, 3, 0], [0.3, 2.0, 0.3, 2.0]), ([2, 0, 3, 1], [1.0, 0.0, 3.0, 0.25])],
             3: [([0, 2, 0], [1.0, 0.3, 1.0]), ([1, 2, 0], [0.5, 3.0, 0.0])],
             2: [([1, 0], [0.3, 2.0]), ([1, 1], [4.0, 4.0])]}
VARIANTS = {'plain': (False, 0.0), 'weights': (True, 0.0), 'smooth': (False, 0.125), 'both': (True, 0.125)}

_inputs = {}


def wide(name):
    return CASES[name][1] > X.HEAD_REG_CAP


def inputs(name):
    """(x f64 [B,C,h,w], labels int64 [B,H,W], class weights f64 [C]) of a case, drawn once"""
    if name not in _inputs:
        B, C, h, w, H, W = CASES[name]
        geo = X.head_geom(B, C, h, w, H, W, wide(name))
        assert geo['band_rows'] == 16 and geo['nband'] * geo['nstrip'] == ROWS_PER_SAMPLE[name], geo
        assert all(X.head_geom(b, C, h, w, H, W, wide(name))['band_rows'] == 16 for b in range(1, B + 1))
        g = X.case_gen(*[ord(ch) for ch in name], 91)
        x = X.head_logits((B, C, h, w), g)
        labels = X.head_labels(B, H, W, C, g, IGN)
        cw = torch.randint(1, 9, (C,), generator=g).double() / 4         # f32-exact, in (0.25, 2]; one class of weight exactly 0
        cw[C // 2] = 0.0
        _inputs[name] = (x, labels, cw)
    return _inputs[name]


def nhwc(x, dtype, ldl=None):
    """the logits on the device as the NHWC map of forward_lowres at pitch ldl, NaN in the pad channels; a leaf that takes a gradient"""
    B, C, h, w = x.shape
    ldl = ldl or X.cdiv(C, 8) * 8
    base = torch.full((B, h, w, ldl), float('nan'), dtype=dtype)
    base[..., :C] = x.permute(0, 2, 3, 1).to(dtype)
    a = base.to(DEV).permute(0, 3, 1, 2)[:, :C]
    assert torch.equal(a.double().cpu(), x), 'logits not exact in the dtype'
    return a.requires_grad_(True)


def run(x, labels, dtype, group=None, lam=None, cw=None, eps=0.0, gout=1.0, ldl=None, on_device=True):
    """loss (f32 scalar), gradient [B,C,h,w] and group_loss [B] (None without groups), on the host"""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    a = nhwc(x, dtype, ldl)
    assert ops.is_nhwc(a)
    kw, gl = {}, None
    if group is not None:
        gl = torch.full((x.shape[0],), float('nan'), dtype=F32, device=DEV)
        if on_device:
            group = torch.tensor(group, dtype=torch.int32, device=DEV)
            lam = None if lam is None else torch.tensor(lam, dtype=F32, device=DEV)
        kw = dict(sample_group=group, sample_weight=lam, group_loss_out=gl)
    loss = tssa.upsample_cross_entropy(a, labels.to(DEV), size=tuple(labels.shape[-2:]), ignore_index=IGN,
                                       weight=None if cw is None else cw.float().to(DEV), label_smoothing=eps, **kw)
    loss.backward(torch.tensor(gout, dtype=F32, device=DEV))
    torch.cuda.synchronize()
    return loss.detach().cpu(), a.grad.detach().cpu(), None if gl is None else gl.cpu()


def ulps(got, want, mant):
    """largest |got - want| in units of want's last place (mant = 24: float32, 8: bfloat16); where want is 0, got must be 0"""
    got, want = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    _, e = torch.frexp(want.abs())
    d = (got - want).abs() / torch.ldexp(torch.ones_like(want), e - mant)
    d = torch.where(want == 0, torch.where(got == 0, torch.zeros_like(d), torch.full_like(d, float('inf'))), d)
    return float(d.max())


def margin(name, d, what, ratio):
    print('GROUPCE_MARGIN %-9s %-5s %-44s %.4f' % (name, d, what, ratio))


def params(names):
    return [pytest.param(n, d, id='%s-%s' % (n, d)) for n in names for d in ('f32', 'bf16')]


# ------------------------------------------------------------------------------------------------ one group: the ungrouped operator
@pytest.mark.parametrize('name,d', params(CASES))
def test_one_group_is_the_ungrouped_operator(name, d):
    x, labels, _ = inputs(name)
    B = x.shape[0]
    loss0, grad0, _ = run(x, labels, DT[d], gout=GOUT)
    for group, lam, on_device in (([B - 1] * B, None, True), ([0] * B, [1.0] * B, False)):
        loss, grad, gl = run(x, labels, DT[d], group, lam, gout=GOUT, on_device=on_device)
        margin(name, d, 'one group: loss, f32 ulp', ulps(loss, loss0, 24))
        assert ulps(loss, loss0, 24) <= 1, (float(loss), float(loss0))
        assert torch.equal(X.bits(grad), X.bits(grad0)), 'the gradient of one group of weight 1 is not the ungrouped one on bits'
        want = torch.zeros(B)
        want[group[0]] = loss
        assert torch.equal(gl, want), (gl, 'the one term is the loss, unused ids are 0')


# ------------------------------------------------------------------------------------------------ several groups
def sub_batches(x, labels, dtype, group, cw, eps):
    """{g: (members, loss, grad)} of the ungrouped operator on each group's sub-batch, grad_out = 1"""
    out = {}
    for g in sorted(set(group)):
        idx = [b for b in range(len(group)) if group[b] == g]
        loss, grad, _ = run(x[idx], labels[idx], dtype, cw=cw, eps=eps)
        out[g] = (idx, loss, grad)
    return out


def check_against_sub_batches(name, d, variant, x, labels, group, lam, cw, eps):
    dtype, B, exact_counts = DT[d], x.shape[0], variant == 'plain'
    tag = '%s %s %s' % (variant, group, lam)
    loss, grad, gl = run(x, labels, dtype, group, lam, cw, eps)
    sub = sub_batches(x, labels, dtype, group, cw, eps)
    assoc = 2.0 ** -50                      # the f64 sums of <= 2^3 rows x samples in another order, relative; far below an f32 ulp
    loss_tol = 1.0 if exact_counts else 1.0 + assoc * 2.0 ** 24
    grad_tol = (2.0 if exact_counts else 4.0) if dtype == F32 else 1.0
    total = 0.0
    for g in range(B):
        if g not in sub:
            assert float(gl[g]) == 0.0, ('an id no sample uses', g, gl)
            continue
        idx, lg, gg = sub[g]
        lams = {lam[b] for b in idx}
        if len(lams) == 1:                  # uniform in the group: the term is lambda L_g
            want = lam[idx[0]] * float(lg)
            total += want
            r = ulps(gl[g], want, 24)
            margin(name, d, tag + ' group_loss[%d], f32 ulp' % g, r)
            assert r <= loss_tol, (g, float(gl[g]), want)
        for k, b in enumerate(idx):
            want = lam[b] * gg[k].double()
            r = ulps(grad[b], want, 24 if dtype == F32 else 8)
            margin(name, d, tag + ' grad[%d], ulp' % b, r)
            assert r <= grad_tol, (b, lam[b], r)
            pow2 = lam[b] == 0.0 or math.frexp(lam[b])[0] == 0.5
            if pow2 and exact_counts:
                assert torch.equal(grad[b].double(), want), ('lambda a power of two: not on bits', b, lam[b])
            if lam[b] == 0.0:
                assert float(grad[b].abs().max()) == 0.0 and not torch.isnan(grad[b]).any(), 'lambda_b = 0: not exact zeros'
    if all(len({lam[b] for b in sub[g][0]}) == 1 for g in sub):
        # the loss is the f32 rounding of the f64 sum of the terms, each within an ulp of its own: one ulp of each term, one of the sum
        tol = sum(float(np.spacing(np.float32(abs(lam[sub[g][0][0]] * float(sub[g][1]))))) for g in sub) + float(np.spacing(np.float32(total)))
        assert abs(float(loss) - total) <= tol * (1.0 if exact_counts else 1.0 + assoc * 2.0 ** 24), (float(loss), total, tol)
    assert abs(float(loss) - float(gl.double().sum())) <= float(np.spacing(np.float32(abs(float(loss))))) * len(sub), (loss, gl)


def check_against_reference(name, d, variant, x, labels, group, lam, cw, eps):
    """loss and gradient (grad_out = 0.7) against tests/groupce_ref.py within the counted bounds of tests/exact.py, per sample"""
    dtype = DT[d]
    B, C, h, w, H, W = CASES[name]
    weighted = cw is not None or eps > 0
    loss, grad, gl = run(x, labels, dtype, group, lam, cw, eps, gout=GOUT, ldl=32 if (C == 19 and name == 'ragged19') else None)
    ref = R.grouped_ce(x, labels, group, lam, (H, W), IGN, class_weight=cw, label_smoothing=eps, grad_out=GOUT)
    n = X.head_counts(B, C, h, w, H, W, wide(name))
    lb, worst = 0.0, 0.0
    for b in range(B):
        hr = X.HeadRef(x[b:b + 1], labels[b:b + 1], weight=cw, eps=eps, ignore_index=IGN, grad_out=GOUT)
        f = float(ref['scale'][b]) * hr.den                       # lambda_b n_b / N_g: the sample's share of its group's mean
        assert abs(hr.den - float(ref['n'][b])) <= 1e-12 * max(hr.den, 1.0)
        if f == 0.0:
            assert float(grad[b].abs().max()) == 0.0, ('a sample of scale 0: not exact zeros', b)
            continue
        sl = X.head_slack(hr)
        lb += f * X.head_loss_bound(hr, n, weighted, n['nchunk'], sl[1])
        gb = f * X.head_grad_bound(hr, n, weighted, dtype == BF, n['nchunk'], sl[2])[0]
        err = (grad[b].double() - ref['grad'][b]).abs()
        ratio = torch.where(gb > 0, err / gb, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float('inf'))))
        worst = max(worst, float(ratio.max()))
    margin(name, d, '%s %s ref: gradient / bound' % (variant, group), worst)
    assert worst <= 1, (name, d, variant, group, lam, worst)
    assert not torch.isnan(grad).any()
    margin(name, d, '%s %s ref: loss / bound' % (variant, group), abs(float(loss) - ref['loss']) / lb if lb > 0 else 0.0)
    assert abs(float(loss) - ref['loss']) <= lb, (float(loss), ref['loss'], lb)
    terms = ref['group_loss']
    assert float((gl.double() - terms).abs().max()) <= lb, (gl, terms, lb)


@pytest.mark.parametrize('name,d', params(CASES))
def test_groups_plain_loss(name, d):
    x, labels, _ = inputs(name)
    for group, lam in GROUPINGS[x.shape[0]]:
        check_against_sub_batches(name, d, 'plain', x, labels, group, lam, None, 0.0)
    group, lam = GROUPINGS[x.shape[0]][0]
    check_against_reference(name, d, 'plain', x, labels, group, lam, None, 0.0)


@pytest.mark.parametrize('variant', ['weights', 'smooth', 'both'])
@pytest.mark.parametrize('name,d', params(['ragged19', 'ragged24', 'bands', 'wide66']))
def test_groups_class_weights_and_smoothing(name, d, variant):
    x, labels, cwv = inputs(name)
    weighted, eps = VARIANTS[variant]
    cw = cwv if weighted else None
    group, lam = GROUPINGS[x.shape[0]][1]
    check_against_sub_batches(name, d, variant, x, labels, group, lam, cw, eps)
    check_against_reference(name, d, variant, x, labels, group, lam, cw, eps)


# ------------------------------------------------------------------------------------------------ empty groups, zero weights
@pytest.mark.parametrize('name,d', params(['ragged19', 'wide66', 'rows257']))
def test_empty_group_gives_zero_and_leaves_the_others_alone(name, d):
    x, labels, _ = inputs(name)
    B = x.shape[0]
    labels = labels.clone()
    labels[B - 1] = IGN                                 # the last sample, a group of its own, has no valid pixel
    labels[B - 1, 0, 0] = -1
    group = list(range(B))
    loss, grad, gl = run(x, labels, DT[d], group, [1.0] * B)
    assert float(gl[B - 1]) == 0.0 and math.isfinite(float(loss))
    assert float(grad[B - 1].abs().max()) == 0.0 and not torch.isnan(grad).any()
    for b in range(B - 1):          # every other group: the ungrouped operator on that sample (gradient on bits, the f64 sums re-associate)
        l1, g1, _ = run(x[b:b + 1], labels[b:b + 1], DT[d])
        assert ulps(gl[b], l1, 24) <= 1 and torch.equal(X.bits(grad[b:b + 1]), X.bits(g1)), b
    # all of them empty: 0, not nan
    loss, grad, gl = run(x, torch.full_like(labels, IGN), DT[d], group, None)
    assert float(loss) == 0.0 and float(gl.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the C entries
def c_forward(name, dtype, ldl):
    """tss_upsample_ce_fwd on the case at pitch ldl (NaN pads): (lib module, low, labels, workspace, [loss, inv_count])"""
    from torch_semantic_segmentation_amd import _native as N
    x, labels, _ = inputs(name)
    B, C, h, w, H, W = CASES[name]
    a = nhwc(x, dtype, ldl).detach()
    t = labels.to(DEV)
    ws = torch.full((N.lib().tss_upsample_ce_ws(B, C, h, w, H, W),), float('nan'), dtype=F32, device=DEV)
    out = torch.full((2,), float('nan'), dtype=F32, device=DEV)
    N.call('tss_upsample_ce_fwd', a.data_ptr(), ldl, t.data_ptr(), ws.data_ptr(), out.data_ptr(), out.data_ptr() + 4, B, C, h, w, H, W, IGN,
           N.dtype_code(dtype), N.stream())
    return N, a, t, ws, out


@pytest.mark.parametrize('d', ['f32', 'bf16'])
def test_c_entries_scale_pad_channels_and_bad_ids(d):
    dtype, name, ldl = DT[d], 'ragged19', 32
    B, C, h, w, H, W = CASES[name]
    N, a, t, ws, out = c_forward(name, dtype, ldl)
    one = torch.ones(1, dtype=F32, device=DEV)

    def finalize(group, lam):
        g = torch.tensor(group, dtype=torch.int32, device=DEV)
        lm = None if lam is None else torch.tensor(lam, dtype=F32, device=DEV)
        res = torch.full((1 + 2 * B,), float('nan'), dtype=F32, device=DEV)             # loss, scale [B], group_loss [B]
        N.call('tss_upsample_ce_group_finalize', ws.data_ptr(), B, C, h, w, H, W, 0, g.data_ptr(), N.ptr(lm), res.data_ptr(),
               res.data_ptr() + 4, res.data_ptr() + 4 * (1 + B), N.stream())
        grad = torch.full((B, h, w, ldl), float('nan'), dtype=dtype, device=DEV)
        N.call('tss_upsample_ce_bwd_rows', ws.data_ptr(), res.data_ptr() + 4, one.data_ptr(), grad.data_ptr(), ldl, B, C, h, w, H, W,
               N.dtype_code(dtype), N.stream())
        torch.cuda.synchronize()
        r = res.cpu()
        return r[0], r[1:1 + B], r[1 + B:], grad.cpu()

    grad0 = torch.full((B, h, w, ldl), float('nan'), dtype=dtype, device=DEV)
    N.call('tss_upsample_ce_bwd', ws.data_ptr(), out.data_ptr() + 4, one.data_ptr(), grad0.data_ptr(), ldl, B, C, h, w, H, W, N.dtype_code(dtype),
           N.stream())
    loss, scale, gl, grad = finalize([1, 1, 1, 1], None)
    inv = out.cpu()[1]
    assert torch.equal(X.bits(scale), X.bits(inv.expand(B).contiguous())), ('scale is not the ungrouped inv_count', scale, inv)
    assert torch.equal(X.bits(grad), X.bits(grad0.cpu())) and (grad[..., C:] == 0).all(), 'gradient / its pad channels'
    assert gl.tolist() == [0.0, float(loss), 0.0, 0.0]
    # ids outside [0, B): weight 0, in no group, nothing indexed by them
    loss2, scale2, gl2, grad2 = finalize([0, -7, 2 ** 30, B], [1.0, 1.0, 1.0, 1.0])
    assert scale2[1:].tolist() == [0.0, 0.0, 0.0] and float(grad2[1:].abs().max()) == 0.0 and (grad2[..., C:] == 0).all()
    assert gl2[1:].tolist() == [0.0, 0.0, 0.0] and float(loss2) == float(gl2[0]) and math.isfinite(float(loss2))
    # a second evaluation on the same workspace: the same bits (the finalize leaves the rows as they are)
    again = finalize([0, -7, 2 ** 30, B], [1.0, 1.0, 1.0, 1.0])
    assert all(torch.equal(X.bits(p), X.bits(q)) for p, q in zip((loss2, scale2, gl2, grad2), again))


def test_c_entries_refuse_what_the_head_refuses():
    N, a, t, ws, out = c_forward('ragged19', F32, 24)
    B, C, h, w, H, W = CASES['ragged19']
    lib = N.lib()
    g = torch.zeros(B, dtype=torch.int32, device=DEV)
    res = torch.zeros(1 + 2 * B, dtype=F32, device=DEV)
    grad = torch.zeros((B, h, w, 24), dtype=F32, device=DEV)
    p = res.data_ptr()
    fin = lambda B_, C_, h_, H_, wide_, gp: lib.tss_upsample_ce_group_finalize(ws.data_ptr(), B_, C_, h_, w, H_, W, wide_, gp, None, p,
                                                                                p + 4, p + 4 * (1 + B), N.stream())
    SHAPE, ALIGN = -2, -3
    assert fin(B, C, h, H, 0, g.data_ptr()) == 0
    assert fin(B, 257, h, H, 1, g.data_ptr()) == SHAPE and fin(B, 25, h, H, 0, g.data_ptr()) == SHAPE          # classes
    assert fin(B, C, H + 1, H, 0, g.data_ptr()) == SHAPE                                                        # H < h
    assert fin(B, C, h, H, 0, None) == SHAPE                                                                    # no group row
    assert fin(lib.tss_upsample_ce_group_max_batch() + 1, C, h, H, 0, g.data_ptr()) == SHAPE
    assert lib.tss_upsample_ce_group_finalize(ws.data_ptr() + 4, B, C, h, w, H, W, 0, g.data_ptr(), None, p, p + 4, p + 4 * (1 + B),
                                              N.stream()) == ALIGN
    for entry, cap in ((lib.tss_upsample_ce_bwd_rows, 24), (lib.tss_upsample_ce_wide_bwd_rows, 256)):
        bwd = lambda C_, h_, ld_, sp: entry(ws.data_ptr(), sp, None, grad.data_ptr(), ld_, B, C_, h_, w, H, W, 0, N.stream())
        assert bwd(cap + 1, h, 264, p + 4) == SHAPE and bwd(C, H + 1, 24, p + 4) == SHAPE and bwd(C, h, 20, p + 4) == SHAPE
        assert bwd(C, h, 24, None) == SHAPE
    k = torch.zeros(2, dtype=torch.int64, device=DEV)
    w4 = torch.zeros(4, dtype=F32, device=DEV)
    g4 = torch.zeros(4, dtype=torch.int32, device=DEV)
    sw = lambda kp, n_, lp, mode, B_: lib.tss_selftrain_weights(kp, n_, lp, mode, g4.data_ptr(), w4.data_ptr(), B_, N.stream())
    assert sw(k.data_ptr(), 64, p, 1, 2) == 0
    assert sw(k.data_ptr(), 64, p, 2, 2) == SHAPE and sw(k.data_ptr(), 0, p, 1, 2) == SHAPE and sw(k.data_ptr(), 64, None, 0, 2) == SHAPE
    assert sw(None, 64, p, 1, 2) == SHAPE and sw(None, 64, p, 0, 2) == 0 and sw(k.data_ptr(), 64, p, 0, 0) == SHAPE
    torch.cuda.synchronize()


@pytest.mark.parametrize('mode', [0, 1])
def test_selftrain_weights_kernel_equals_its_restatement(mode):
    from torch_semantic_segmentation_amd import _native as N
    for kept, npix, lam in (([10, 30], 100, 0.5), ([8191, 0, 4000], 8192, 0.7), ([3] * 300, 7, 1.3), ([0], 5, 2.0)):
        B = len(kept)
        k = torch.tensor(kept, dtype=torch.int64, device=DEV)
        lm = torch.tensor([lam], dtype=F32, device=DEV)
        g = torch.full((2 * B,), -1, dtype=torch.int32, device=DEV)
        w = torch.full((2 * B,), float('nan'), dtype=F32, device=DEV)
        N.call('tss_selftrain_weights', k.data_ptr(), npix, lm.data_ptr(), mode, g.data_ptr(), w.data_ptr(), B, N.stream())
        torch.cuda.synchronize()
        rg, rw = R.selftrain_weights(kept, npix, lam, mode)
        assert np.array_equal(g.cpu().numpy(), rg) and np.array_equal(w.cpu().numpy().view(np.uint32), rw.view(np.uint32)), (kept, lam, mode)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_errors_on_the_device():
    import torch_semantic_segmentation_amd as tssa
    x, labels, _ = inputs('ragged19')
    a, t = nhwc(x, F32), labels.to(DEV)
    call = lambda **kw: tssa.upsample_cross_entropy(a, t, size=(25, 49), ignore_index=IGN, **kw)
    for kw in (dict(sample_group=torch.zeros(4, dtype=torch.int64, device=DEV)),                                  # dtype
               dict(sample_group=torch.zeros(3, dtype=torch.int32, device=DEV)),                                  # length
               dict(sample_group=[0, 0, 1, 1], sample_weight=torch.ones(4, dtype=torch.float64, device=DEV)),
               dict(sample_group=[0, 0, 1, 1], group_loss_out=torch.zeros(3, dtype=F32, device=DEV)),
               dict(sample_group=[0, 0, 1, 4]), dict(sample_group=[0, 0, 1, 1], sample_weight=[1.0, -1.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):           # an output smaller than the map: no unfused route for groups
        tssa.upsample_cross_entropy(a, t[:, :3, :5].contiguous(), size=(3, 5), ignore_index=IGN, sample_group=[0, 0, 1, 1])


@pytest.mark.parametrize('d', ['f32', 'bf16'])
def test_module_groups_on_full_resolution_logits_and_a_captured_update(d):
    """CrossEntropyLoss.set_sample_groups: on full-resolution logits the module is the grouped operator at the logits' own size; the
    rows are device tensors the kernels read, so a captured forward + backward follows an in-place update of the weights"""
    import torch_semantic_segmentation_amd as tssa
    dtype = DT[d]
    g = X.case_gen(92)
    B, C, H, W = 4, 19, 24, 40
    x, labels = X.head_logits((B, C, H, W), g), X.head_labels(B, H, W, C, g, IGN)
    group = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=DEV)
    lam = torch.tensor([1.0, 0.5, 1.0, 0.5], dtype=F32, device=DEV)
    gl = torch.zeros(B, dtype=F32, device=DEV)
    ce = tssa.CrossEntropyLoss(ignore_index=IGN)
    ce.set_sample_groups(group, lam, gl)
    assert ce.sample_group.data_ptr() == group.data_ptr() and ce.sample_weight.data_ptr() == lam.data_ptr(), 'device rows are not copied'
    a, t = nhwc(x, dtype), labels.to(DEV)
    one = torch.ones((), dtype=F32, device=DEV)

    def eager(weights):
        lam.copy_(torch.tensor(weights))
        a.grad = None
        loss = ce(a, t)
        loss.backward(one)
        return loss.detach().clone(), a.grad.detach().clone(), gl.clone()

    want = tssa.upsample_cross_entropy(a.detach(), t, size=(H, W), ignore_index=IGN, sample_group=[0, 1, 0, 1], sample_weight=[1.0, 0.5, 1.0, 0.5])
    first = eager([1.0, 0.5, 1.0, 0.5])
    assert torch.equal(X.bits(first[0].cpu().reshape(1)), X.bits(want.cpu().reshape(1)))
    second = eager([1.0, 0.0, 1.0, 0.0])
    assert float(second[1][1].abs().max()) == 0.0 and float(second[2][1]) == 0.0 and float(first[2][1]) > 0.0
    # captured once, replayed after an in-place update of the weights
    lam.copy_(torch.tensor([1.0, 0.5, 1.0, 0.5]))
    b = nhwc(x, dtype).detach()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            bb = b.clone().requires_grad_(True)
            ce(bb, t).backward(one)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bb = b.clone().requires_grad_(True)
        out = ce(bb, t)
        out.backward(one)
        grad = bb.grad
    for weights, ref in (([1.0, 0.5, 1.0, 0.5], first), ([1.0, 0.0, 1.0, 0.0], second)):
        lam.copy_(torch.tensor(weights))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(X.bits(out.cpu().reshape(1)), X.bits(ref[0].cpu().reshape(1))), weights
        assert torch.equal(X.bits(grad.cpu()), X.bits(ref[1].cpu())) and torch.equal(gl.cpu(), ref[2].cpu()), weights
    ce.clear_sample_groups()
    assert ce.sample_group is None
