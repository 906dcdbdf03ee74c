"""Per-pixel loss weights on the fused head (csrc/pixwce.hip; ops.upsample_pixel_weighted_cross_entropy) on the GPU.

Shapes: those of tests/test_gpu_groupce.py (every head_geom call ends at band_rows = 16, so a sub-batch has the rows and tiles of the same
samples inside the full batch) and exact.HEAD_REG's one_lane_strip (1x19x5x33 -> 33x257: a strip of one lane).  Logits are multiples of
2^-2 in [-8, 8] (exact in bf16), labels carry ignored and out-of-range pixels, pad channels hold NaN and ragged19 runs at a pitch of 32.
omega is a multiple of 1/8 in [0, 2] with planted zeros, the last sample all zeros (B > 1) and one row of 2.0; the class weights are
multiples of 1/4 with one class of weight 0.  So k = omega w_t is exact in f32 in these cases; the bounds count its rounding anyway.

Against tests/pixwce_ref.py: the counted bounds of tests/exact.py with weighted=True (head_loss_bound, head_grad_bound, head_slack; the
reference object is pixwce_ref.head_ref: s = omega w_t, hot = s onehot, den = D), extended by what csrc/pixwce.hip adds, counted from its
text, in units of u = 2^-24:
  register pass, gradient: k = omega * Cw[t], one product (+1 on a term's chain); everything else is the focal pass's chain that
    head_grad_counts counts with weighted=True: k / sum scales the softmax half (V_RCP_F32, one product, one product with e_c), l0 k and
    l1 k enter the one-hot table, D is an f32 lane sum over a band's rows (band_rows), the scale fl32(lambda / D) grad_out (3).
  register pass, loss: the pixel term is ce = (m - z_t) + log2 sum, the chain of head_pix_bound's register line, which exceeds
    head_loss_counts' r_l = head_lse_err + 5 zmax by 10 zmax + 2 ln C per unit of weight (z_t is blended vertically as well, m - z_t is
    one more subtraction and the product with ln 2 -- here in f64 -- is counted there); the product with k and the product omega w_t
    are 2 roundings relative to the term (+2 S; the lane's f32 additions are head_loss_counts' band_rows).
  wide route, loss: the stored ce carries head_pix_bound(zmax, C, nchunk) per pixel; k = omega w_t (1), the f32 product k ce (1), the
    f32 loss (1): 3 S; the sums are f64.  Gradient: the coefficient's product (+1) on head_grad_counts' wide chain; the MODE 5 pass
    recomputes the log-sum-exp, the stored ce does not enter.
Every comparison prints its largest ratio as a line `PIXWCE_MARGIN ...` before it asserts (profiles/pixwce_margins.txt)."""
import math

import numpy as np
import pytest
import torch

from tests import exact as X
from tests import pixwce_ref as R
from tests import selftrain_ref
from tests.test_gpu_groupce import CASES as GROUP_CASES, GROUPINGS, nhwc, ulps

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IGN = 255
BF, F32 = torch.bfloat16, torch.float32
DT = {'f32': F32, 'bf16': BF}
GOUT = float(np.float32(0.7))
NORMS = ('weight', 'valid', 'pixels')

_one = X.HEAD_BY_NAME['one_lane_strip']
CASES = dict(GROUP_CASES, one_lane_strip=(_one.B, _one.C, _one.h, _one.w, _one.H, _one.W))
_inputs, _refs = {}, {}


def wide(name):
    return CASES[name][1] > X.HEAD_REG_CAP


def pitch(name):
    return 32 if name == 'ragged19' else None


def inputs(name):
    """(x f64 [B,C,h,w], labels int64 [B,H,W], omega f32 [B,H,W], class weights f64 [C]) of a case, drawn once"""
    if name not in _inputs:
        B, C, h, w, H, W = CASES[name]
        assert X.head_geom(B, C, h, w, H, W, wide(name))['band_rows'] == 16
        g = X.case_gen(*[ord(ch) for ch in name], 93)
        x = X.head_logits((B, C, h, w), g)
        labels = X.head_labels(B, H, W, C, g, IGN)
        om = torch.randint(1, 17, (B, H, W), generator=g).float() / 8
        om[torch.rand((B, H, W), generator=g) < 0.1] = 0.0
        om[0, H // 2] = 2.0
        if B > 1:
            om[B - 1] = 0.0
        cw = torch.randint(1, 9, (C,), generator=g).double() / 4
        cw[C // 2] = 0.0
        _inputs[name] = (x, labels, om, cw)
    return _inputs[name]


def run(x, labels, om, dtype, norm='weight', cw=None, group=None, lam=None, gout=1.0, ldl=None):
    """loss (f32 scalar), gradient [B,C,h,w] and group_loss [B], on the host"""
    import torch_semantic_segmentation_amd as tssa
    a = nhwc(x, dtype, ldl)
    gl = torch.full((x.shape[0],), float('nan'), dtype=F32, device=DEV)
    kw = {}
    if group is not None:
        kw = dict(sample_group=torch.tensor(group, dtype=torch.int32, device=DEV),
                  sample_weight=None if lam is None else torch.tensor(lam, dtype=F32, device=DEV), group_loss_out=gl)
    loss = tssa.upsample_pixel_weighted_cross_entropy(a, labels.to(DEV), om.to(DEV), size=tuple(labels.shape[-2:]), ignore_index=IGN,
                                                      weight=None if cw is None else cw.float().to(DEV), pixel_norm=norm, **kw)
    loss.backward(torch.tensor(gout, dtype=F32, device=DEV))
    torch.cuda.synchronize()
    return loss.detach().cpu(), a.grad.detach().cpu(), gl.cpu() if group is not None else None


def margin(name, d, what, ratio):
    print('PIXWCE_MARGIN %-14s %-5s %-52s %.4f' % (name, d, what, ratio))


def params(names):
    return [pytest.param(n, d, id='%s-%s' % (n, d)) for n in names for d in ('f32', 'bf16')]


def loss_bound(ref, n, nchunk, slack):
    """header: the register pass extends head_loss_bound, the wide route sums stored per-pixel losses"""
    C, zmax = ref.C, ref.zmax
    if nchunk:
        return (ref.sabs * X.head_pix_bound(zmax, C, nchunk) + X.U32 * 3.0 * ref.S) * 1.001 / ref.den + 2.0 ** -50 * ref.S / ref.den + slack
    return X.head_loss_bound(ref, n, True, 0, slack) + X.U32 * ((10.0 * zmax + 2.0 * math.log(C)) * ref.sabs + 2.0 * ref.S) * 1.001 / ref.den


def grad_bound(ref, n, bf16, nchunk, slack):
    """head_grad_bound(weighted=True) with one more rounding on the chain: the product omega w_t"""
    n_g, r_p = X.head_grad_counts(n, ref.zmax, ref.C, True, nchunk)
    k = X.U32 * (n_g + r_p + 1)
    bound = k / (1 - k) * ref.A + slack
    return bound + (2.0 ** -8 * (ref.g.abs() + bound) if bf16 else 0.0)


def reference(name, norm, weighted, group=None, lam=None):
    """(pixwce_ref result, per-sample HeadRefs scaled by lambda_b / N_g) of a case, computed once and shared by both dtypes"""
    key = (name, norm, weighted, None if group is None else (tuple(group), tuple(lam)))
    if key not in _refs:
        x, labels, om, cwv = inputs(name)
        cw = cwv if weighted else None
        ref = R.pixel_weighted_ce(x, labels, om.double(), labels.shape[-2:], IGN, cw, norm, group, lam, grad_out=GOUT)
        heads = []
        for b in range(x.shape[0]):
            sc = float(ref['scale'][b])
            heads.append(None if sc == 0.0 else R.head_ref(x[b:b + 1], labels[b:b + 1], om[b:b + 1].double(), cw, norm, IGN, grad_out=GOUT,
                                                            den=1.0 / sc))
        _refs[key] = (ref, heads)
    return _refs[key]


def check_against_reference(name, d, norm, weighted, group=None, lam=None):
    dtype = DT[d]
    B, C, h, w, H, W = CASES[name]
    x, labels, om, cwv = inputs(name)
    loss, grad, gl = run(x, labels, om, dtype, norm, cwv if weighted else None, group, lam, gout=GOUT, ldl=pitch(name))
    ref, heads = reference(name, norm, weighted, group, lam)
    n = X.head_counts(B, C, h, w, H, W, wide(name))
    tag = '%s %s%s' % (norm, 'cw' if weighted else 'plain', '' if group is None else ' %s' % (group,))
    lb, worst = 0.0, 0.0
    for b in range(B):
        hr = heads[b]
        if hr is None:                # lambda_b / N_g = 0: lambda 0 or an empty denominator
            assert float(grad[b].abs().max()) == 0.0, ('a sample of scale 0: not exact zeros', b)
            continue
        sl = X.head_slack(hr)
        lb += loss_bound(hr, n, n['nchunk'], sl[1])           # the sample's share: its sums over the group's denominator
        gb = grad_bound(hr, n, dtype == BF, n['nchunk'], sl[2])[0]
        err = (grad[b].double() - ref['grad'][b]).abs()
        ratio = torch.where(gb > 0, err / gb, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float('inf'))))
        worst = max(worst, float(ratio.max()))
    margin(name, d, tag + ': gradient / bound', worst)
    margin(name, d, tag + ': loss / bound', abs(float(loss) - ref['loss']) / lb if lb > 0 else 0.0)
    assert worst <= 1, (name, d, tag, worst)
    assert not torch.isnan(grad).any()
    assert abs(float(loss) - ref['loss']) <= lb, (float(loss), ref['loss'], lb)
    if gl is not None:
        assert float((gl.double() - ref['group_loss']).abs().max()) <= lb, (gl, ref['group_loss'], lb)


# ------------------------------------------------------------------------------------------------ against the f64 reference
@pytest.mark.parametrize('name,d', params(CASES))
def test_loss_and_gradient_against_the_reference(name, d):
    for norm in NORMS:
        for weighted in (False, True):
            check_against_reference(name, d, norm, weighted)


@pytest.mark.parametrize('name,d', params(['ragged19', 'wide66']))
def test_group_loss_out_without_groups_is_one_group(name, d):
    """no sample_group: ids all 0, weights all 1 -- the loss arrives in group_loss_out[0], the other ids get 0"""
    import torch_semantic_segmentation_amd as tssa
    x, labels, om, _ = inputs(name)
    B = x.shape[0]
    loss0, grad0, _ = run(x, labels, om, DT[d])
    loss, grad, gl = run(x, labels, om, DT[d], group=[0] * B)
    assert torch.equal(X.bits(loss.reshape(1)), X.bits(loss0.reshape(1))) and torch.equal(X.bits(grad), X.bits(grad0))
    assert gl.tolist() == [float(loss)] + [0.0] * (B - 1)
    with pytest.raises(ValueError):
        tssa.upsample_pixel_weighted_cross_entropy(nhwc(x, DT[d]), labels.to(DEV), om.to(DEV), size=tuple(labels.shape[-2:]), ignore_index=IGN,
                                                   group_loss_out=torch.zeros(B, device=DEV))


# ------------------------------------------------------------------------------------------------ exact properties, on bits
def same(a, b):
    return torch.equal(X.bits(a.reshape(-1)), X.bits(b.reshape(-1)))


@pytest.mark.parametrize('name,d', params(CASES))
def test_exact_properties(name, d):
    dtype = DT[d]
    x, labels, om, cwv = inputs(name)
    B = x.shape[0]
    for cw in (None, cwv):
        base = {norm: run(x, labels, om, dtype, norm, cw, gout=GOUT, ldl=pitch(name)) for norm in NORMS}
        # a second call: the same bits
        again = run(x, labels, om, dtype, 'weight', cw, gout=GOUT, ldl=pitch(name))
        assert same(again[0], base['weight'][0]) and same(again[1], base['weight'][1])
        # 2 omega: every product and sum doubles exactly; 'weight' divides it out again, the other two denominators stay
        for norm in NORMS:
            l2, g2, _ = run(x, labels, 2 * om, dtype, norm, cw, gout=GOUT, ldl=pitch(name))
            f = 1.0 if norm == 'weight' else 2.0
            assert same(l2, f * base[norm][0]), (norm, float(l2), float(base[norm][0]))
            assert same(g2, f * base[norm][1]), norm       # bf16 too: the rounded 2 x gradient is 2 x the rounded gradient
        # 'weight': omega = 0 on a set of pixels is ignore_index on those pixels
        gsel = X.case_gen(*[ord(ch) for ch in name], 94)
        drop = torch.rand(labels.shape, generator=gsel) < 0.3
        la, ga, _ = run(x, labels, torch.where(drop, torch.zeros_like(om), om), dtype, 'weight', cw, gout=GOUT, ldl=pitch(name))
        lb, gb, _ = run(x, torch.where(drop, torch.full_like(labels, IGN), labels), om, dtype, 'weight', cw, gout=GOUT, ldl=pitch(name))
        assert same(la, lb) and same(ga, gb)
        # a sample whose map is all zero (every sample its own group): an exactly zero gradient, no NaN, and a term of 0
        if B > 1:
            l, g, gl = run(x, labels, om, dtype, 'weight', cw, group=list(range(B)), lam=[1.0] * B)
            assert float(g[B - 1].abs().max()) == 0.0 and not torch.isnan(g).any() and float(gl[B - 1]) == 0.0 and math.isfinite(float(l))
            assert float(base['weight'][1][B - 1].abs().max()) == 0.0
        # every map zero: 0.0, a zero gradient, every term 0
        l, g, gl = run(x, labels, torch.zeros_like(om), dtype, 'weight', cw, group=list(range(B)), lam=[1.0] * B)
        assert float(l) == 0.0 and float(g.abs().max()) == 0.0 and float(gl.abs().max()) == 0.0 and not torch.isnan(g).any()
        l, g, _ = run(x, labels, torch.zeros_like(om), dtype, 'weight', cw)
        assert float(l) == 0.0 and float(g.abs().max()) == 0.0


@pytest.mark.parametrize('name,d', params(['ragged19', 'wide66']))
def test_ones_under_valid_restate_the_plain_loss(name, d):
    """omega = 1, 'valid': the numerator and the denominator of upsample_cross_entropy; the pass sums in another order (the target's
    logit leaves per pixel, not per flush), so the two agree within their bounds against the f64 reference, not on bits"""
    import torch_semantic_segmentation_amd as tssa
    x, labels, om, _ = inputs(name)
    a = nhwc(x, DT[d])
    want = tssa.upsample_cross_entropy(a.detach(), labels.to(DEV), size=tuple(labels.shape[-2:]), ignore_index=IGN)
    got, _, _ = run(x, labels, torch.ones_like(om), DT[d], 'valid')
    B, C, h, w, H, W = CASES[name]
    hr = R.head_ref(x, labels, torch.ones_like(om).double(), None, 'valid', IGN)
    n = X.head_counts(B, C, h, w, H, W, wide(name))
    sl = X.head_slack(hr)
    lb = loss_bound(hr, n, n['nchunk'], sl[1]) + X.head_loss_bound(hr, n, False, n['nchunk'], sl[1])
    margin(name, d, 'ones, valid: |pixw - plain| / (sum of the two bounds)', abs(float(got) - float(want)) / lb)
    assert abs(float(got) - float(want)) <= lb


# ------------------------------------------------------------------------------------------------ groups
def check_against_sub_batches(name, d, norm, cw, group, lam):
    """test_gpu_groupce's rule for a denominator that is a sum of f32 weights: N_g of the two sides differs by f64 re-association"""
    dtype = DT[d]
    x, labels, om, _ = inputs(name)
    B = x.shape[0]
    loss, grad, gl = run(x, labels, om, dtype, norm, cw, group, lam, ldl=pitch(name))
    assoc = 2.0 ** -50
    loss_tol = 1.0 + assoc * 2.0 ** 24
    grad_tol = 4.0 if dtype == F32 else 1.0
    for g in range(B):
        idx = [b for b in range(B) if group[b] == g]
        if not idx:
            assert float(gl[g]) == 0.0, ('an id no sample uses', g, gl)
            continue
        lg, gg, _ = run(x[idx], labels[idx], om[idx], dtype, norm, cw, ldl=pitch(name))
        if len({lam[b] for b in idx}) == 1:
            want = lam[idx[0]] * float(lg)
            r = ulps(gl[g], want, 24)
            margin(name, d, '%s %s %s group_loss[%d], f32 ulp' % (norm, 'plain' if cw is None else 'cw', group, g), r)
            assert r <= loss_tol, (g, float(gl[g]), want)
        for k, b in enumerate(idx):
            want = lam[b] * gg[k].double()
            r = ulps(grad[b], want, 24 if dtype == F32 else 8)
            margin(name, d, '%s %s %s grad[%d], ulp' % (norm, 'plain' if cw is None else 'cw', group, b), r)
            assert r <= grad_tol, (b, lam[b], r)
            if lam[b] == 0.0:
                assert float(grad[b].abs().max()) == 0.0 and not torch.isnan(grad[b]).any()
    assert abs(float(loss) - float(gl.double().sum())) <= float(np.spacing(np.float32(abs(float(loss))))) * B, (loss, gl)


@pytest.mark.parametrize('name,d', params([n for n in GROUP_CASES]))
def test_sample_groups_compose(name, d):
    x, labels, om, cwv = inputs(name)
    group, lam = GROUPINGS[x.shape[0]][0]
    for norm in NORMS:
        check_against_sub_batches(name, d, norm, None, group, lam)
    check_against_sub_batches(name, d, 'weight', cwv, group, lam)
    check_against_reference(name, d, 'weight', True, group, lam)
    check_against_reference(name, d, 'pixels', False, group, lam)


# ------------------------------------------------------------------------------------------------ the C entries
def c_pass(name, dtype, ldl, om, norm=0, cw=None):
    """tss_upsample_ce_pixw_fwd + the one-group finalize + the gather on NaN-filled buffers: (loss, grad [B,h,w,ldl]) on the host"""
    from torch_semantic_segmentation_amd import _native as N
    x, labels, _, _ = inputs(name)
    B, C, h, w, H, W = CASES[name]
    a = nhwc(x, dtype, ldl).detach()
    t = labels.to(DEV)
    ws = torch.full((N.lib().tss_upsample_ce_ws(B, C, h, w, H, W),), float('nan'), dtype=F32, device=DEV)
    N.call('tss_upsample_ce_pixw_fwd', a.data_ptr(), ldl, t.data_ptr(), om.data_ptr(), N.ptr(cw), norm, ws.data_ptr(), B, C, h, w, H, W, IGN,
           N.dtype_code(dtype), N.stream())
    g = torch.zeros(B, dtype=torch.int32, device=DEV)
    res = torch.full((1 + 2 * B,), float('nan'), dtype=F32, device=DEV)
    N.call('tss_upsample_ce_group_finalize', ws.data_ptr(), B, C, h, w, H, W, 0, g.data_ptr(), None, res.data_ptr(), res.data_ptr() + 4,
           res.data_ptr() + 4 * (1 + B), N.stream())
    grad = torch.full((B, h, w, ldl), float('nan'), dtype=dtype, device=DEV)
    one = torch.ones(1, dtype=F32, device=DEV)
    N.call('tss_upsample_ce_bwd_rows', ws.data_ptr(), res.data_ptr() + 4, one.data_ptr(), grad.data_ptr(), ldl, B, C, h, w, H, W,
           N.dtype_code(dtype), N.stream())
    torch.cuda.synchronize()
    return res.cpu()[0], grad.cpu()


@pytest.mark.parametrize('d', ['f32', 'bf16'])
def test_c_entry_pad_channels_and_the_end_of_the_map(d):
    """pad channels of the gradient are zeros; with the map at the end of an allocation whose next bytes hold NaN (W = 49: 207 lanes of
    the strip lie past the edge) the result is the one of a map that stands alone.  This shows that nothing read past the map is USED; a
    lane past the edge is never valid, so the check cannot tell whether it loaded anything -- that it does not is in the kernel's text
    (`xin ? *wrow : 0.f`, `if (xin) onext = ...`), not in this test"""
    dtype, name, ldl = DT[d], 'ragged19', 32
    B, C, h, w, H, W = CASES[name]
    _, _, om, _ = inputs(name)
    n = B * H * W
    alone = om.to(DEV).contiguous()
    big = torch.full((n + 4096,), float('nan'), dtype=F32, device=DEV)
    big[:n] = alone.reshape(-1)
    loss0, grad0 = c_pass(name, dtype, ldl, alone)
    loss1, grad1 = c_pass(name, dtype, ldl, big[:n])
    assert math.isfinite(float(loss0)) and same(loss0, loss1) and same(grad0, grad1)
    assert (grad0[..., C:] == 0).all() and not torch.isnan(grad0).any()
    # the Python operator on the same inputs gives the same bits
    x, labels, _, _ = inputs(name)
    loss2, grad2, _ = run(x, labels, om, dtype, ldl=ldl)
    assert same(loss0, loss2) and same(grad0[..., :C].permute(0, 3, 1, 2).contiguous(), grad2)


def test_c_entries_refuse_what_the_head_refuses():
    from torch_semantic_segmentation_amd import _native as N
    lib = N.lib()
    name = 'ragged19'
    B, C, h, w, H, W = CASES[name]
    x, labels, om, _ = inputs(name)
    a, t, o = nhwc(x, F32, 32).detach(), labels.to(DEV), om.to(DEV)
    ws = torch.zeros(lib.tss_upsample_ce_wide_ws(B, 66, h, w, H, W) + 8, dtype=F32, device=DEV)
    pix = torch.zeros((B, H, W), dtype=F32, device=DEV)
    SHAPE, ALIGN = -2, -3
    fwd = lambda C_=C, norm=0, w_=w, W_=W, wsp=ws.data_ptr(), op=o.data_ptr(), ld_=32: lib.tss_upsample_ce_pixw_fwd(
        a.data_ptr(), ld_, t.data_ptr(), op, None, norm, wsp, B, C_, h, w_, H, W_, IGN, 0, N.stream())
    assert fwd() == 0
    assert fwd(C_=25) == SHAPE                                    # the register entry takes at most 24 classes
    assert fwd(norm=3) == SHAPE and fwd(norm=-1) == SHAPE
    assert fwd(w_=W + 1) == SHAPE                                 # W < w
    assert fwd(ld_=20) == SHAPE                                   # a pitch that is no multiple of 8
    assert fwd(op=None) == SHAPE and fwd(wsp=None) == SHAPE
    assert fwd(wsp=ws.data_ptr() + 4) == ALIGN and fwd(op=o.data_ptr() + 2) == ALIGN
    assert lib.tss_upsample_ce_pixw_fwd(a.data_ptr(), 32, t.data_ptr(), o.data_ptr(), None, 0, ws.data_ptr(), 0, C, h, w, H, W, IGN, 0,
                                        N.stream()) == 0          # an empty batch: nothing launched
    coef = lambda C_=66, norm=0, wsp=ws.data_ptr(), op=o.data_ptr(), pp=pix.data_ptr(), W_=W: lib.tss_upsample_ce_pixw_coef_wide(
        pp, t.data_ptr(), op, None, norm, wsp, B, C_, H, W_, IGN, N.stream())
    assert coef() == 0
    assert coef(C_=257) == SHAPE and coef(norm=3) == SHAPE and coef(W_=0) == SHAPE and coef(op=None) == SHAPE and coef(pp=None) == SHAPE
    assert coef(wsp=ws.data_ptr() + 4) == ALIGN and coef(op=o.data_ptr() + 2) == ALIGN
    lab8 = torch.zeros((2, 9, 16), dtype=torch.uint8, device=DEV)
    pl = torch.zeros((2, 9, 16), dtype=F32, device=DEV)
    out = torch.zeros_like(pl)
    part = torch.zeros(2, dtype=torch.int32, device=DEV)
    sel = torch.zeros((2, 256), dtype=torch.uint8, device=DEV)
    box = torch.zeros((2, 4), dtype=torch.int32, device=DEV)
    mp = lambda W_=16, sp=sel.data_ptr(), bp=None, pp=pl.data_ptr(): lib.tss_mix_plane(pp, lab8.data_ptr(), part.data_ptr(), sp, bp,
                                                                                      out.data_ptr(), 2, 9, W_, N.stream())
    assert mp() == 0 and mp(sp=None, bp=box.data_ptr()) == 0
    assert mp(W_=12) == SHAPE and mp(sp=None) == SHAPE and mp(bp=box.data_ptr()) == SHAPE and mp(pp=pl.data_ptr() + 4) == ALIGN
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ mix_plane
@pytest.mark.parametrize('H,W', [(9, 16), (23, 40)])
def test_mix_plane_equals_its_restatement(H, W):
    import torch_semantic_segmentation_amd as tssa
    g = X.case_gen(H, W, 95)
    B = 3
    labels = torch.randint(0, 6, (B, H, W), generator=g).to(torch.uint8)
    labels[:, :, :8] = 2                              # whole groups of one side
    labels[torch.rand((B, H, W), generator=g) < 0.05] = IGN
    plane = torch.randn((B, H, W), generator=g)
    plane[0, 0, 0] = -0.0
    partner = [1, 2, 0]
    sel = torch.zeros((B, 256), dtype=torch.uint8)
    sel[0, [1, 3]] = 1
    sel[1, [0, 2, 4]] = 1
    sel[2, 255] = 1
    boxes = np.array([[2, 3, 7, 13], [0, 0, H, W], [4, 8, 4, 16]], dtype=np.int32)      # ragged edges; everything; nothing
    for kw in (dict(sel=sel), dict(boxes=boxes)):
        rkw = {k: v.numpy() if torch.is_tensor(v) else v for k, v in kw.items()}
        want = R.mix_plane(selftrain_ref.bits_of(plane), labels.numpy(), partner, **rkw)
        got = tssa.mix_plane(plane.to(DEV), labels.to(DEV), partner, **kw)
        assert np.array_equal(selftrain_ref.bits_of(got), want), list(kw)
        # a NaN on the side not chosen never arrives: sample 0 keeps its own pixel where the mask holds, its partner's elsewhere
        m = torch.from_numpy(selftrain_ref.mix_mask(labels.numpy(), **rkw))
        poisoned = plane.clone()
        poisoned[0][~m[0]] = float('nan')
        poisoned[1][m[0]] = float('nan')
        out = torch.full((B, H, W), float('nan'), dtype=F32, device=DEV)
        tssa.mix_plane(poisoned.to(DEV), labels.to(DEV), torch.tensor(partner, dtype=torch.int32, device=DEV), out=out,
                       **{k: (torch.as_tensor(v).to(DEV) if k == 'sel' else torch.from_numpy(v).to(DEV)) for k, v in kw.items()})
        assert not torch.isnan(out[0]).any()
        assert np.array_equal(selftrain_ref.bits_of(out)[0], want[0])
    with pytest.raises(ValueError):
        tssa.mix_plane(plane.to(DEV), labels.to(DEV), partner)
    with pytest.raises(ValueError):
        tssa.mix_plane(plane[:, :, :12].contiguous().to(DEV), labels[:, :, :12].contiguous().to(DEV), partner, sel=sel)
    with pytest.raises(ValueError):
        tssa.mix_plane(plane.double().to(DEV), labels.to(DEV), partner, sel=sel)
    p = plane.to(DEV)
    with pytest.raises(ValueError):
        tssa.mix_plane(p, labels.to(DEV), partner, sel=sel, out=p)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_errors_on_the_device():
    import torch_semantic_segmentation_amd as tssa
    x, labels, om, _ = inputs('ragged19')
    a, t, o = nhwc(x, F32), labels.to(DEV), om.to(DEV)
    call = lambda pixel_weight, **kw: tssa.upsample_pixel_weighted_cross_entropy(a, t, pixel_weight, size=(25, 49), ignore_index=IGN, **kw)
    for kw in (dict(pixel_weight=om),                                            # a host map
               dict(pixel_weight=o[:3]), dict(pixel_weight=o[:, :, :48]),        # shape
               dict(pixel_weight=o.double()), dict(pixel_weight=o.transpose(1, 2).contiguous().transpose(1, 2)),     # dtype, strides
               dict(pixel_weight=o, label_smoothing=0.1), dict(pixel_weight=o, pixel_norm='mean')):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):           # 257 classes: no unfused route
        tssa.upsample_pixel_weighted_cross_entropy(torch.zeros((4, 257, 4, 7), device=DEV), t, o, size=(25, 49), ignore_index=IGN)
    with pytest.raises(ValueError):           # an output smaller than the map
        tssa.upsample_pixel_weighted_cross_entropy(a, t[:, :3, :5].contiguous(), o[:, :3, :5].contiguous(), size=(3, 5), ignore_index=IGN)
    # a map that requires grad is detached: no gradient flows to it
    og = o.clone().requires_grad_(True)
    b = nhwc(x, F32)
    call2 = tssa.upsample_pixel_weighted_cross_entropy(b, t, og, size=(25, 49), ignore_index=IGN)
    call2.backward()
    assert og.grad is None and b.grad is not None


@pytest.mark.parametrize('d', ['f32', 'bf16'])
def test_module_on_full_resolution_logits_and_a_captured_update(d):
    """CrossEntropyLoss.set_pixel_weight: on full-resolution logits the module is the operator at the logits' own size; the map is a
    device tensor the kernels read, so a captured forward + backward follows an in-place update"""
    import torch_semantic_segmentation_amd as tssa
    dtype = DT[d]
    g = X.case_gen(96)
    B, C, H, W = 4, 19, 24, 40
    x, labels = X.head_logits((B, C, H, W), g), X.head_labels(B, H, W, C, g, IGN)
    om = (torch.randint(0, 17, (B, H, W), generator=g).float() / 8).to(DEV)
    om2 = (torch.randint(0, 17, (B, H, W), generator=g).float() / 8).to(DEV)
    wmap = om.clone()
    ce = tssa.CrossEntropyLoss(ignore_index=IGN)
    ce.set_pixel_weight(wmap, 'pixels')
    assert ce.pixel_weight.data_ptr() == wmap.data_ptr() and ce.pixel_norm == 'pixels', 'the map is not copied'
    a, t = nhwc(x, dtype), labels.to(DEV)
    one = torch.ones((), dtype=F32, device=DEV)

    def eager(values):
        wmap.copy_(values)
        a.grad = None
        loss = ce(a, t)
        loss.backward(one)
        return loss.detach().clone(), a.grad.detach().clone()

    want = tssa.upsample_pixel_weighted_cross_entropy(a.detach(), t, om, size=(H, W), ignore_index=IGN, pixel_norm='pixels')
    first, second = eager(om), eager(om2)
    assert same(first[0].cpu(), want.cpu()) and not same(first[0].cpu(), second[0].cpu())
    hr = R.head_ref(x, labels, om.cpu().double(), None, 'pixels', IGN)
    n = X.head_counts(B, C, H, W, H, W)
    lb = loss_bound(hr, n, 0, X.head_slack(hr)[1])
    margin('module', d, 'pixels, full-resolution logits: loss / bound', abs(float(first[0]) - hr.loss) / lb)
    assert abs(float(first[0]) - hr.loss) <= lb and abs(hr.loss - R.pixel_weighted_ce(x, labels, om.cpu().double(), norm='pixels')['loss']) < 1e-12
    wmap.copy_(om)
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
    for values, want2 in ((om, first), (om2, second)):
        wmap.copy_(values)
        graph.replay()
        torch.cuda.synchronize()
        assert same(out.cpu(), want2[0].cpu()) and same(grad.cpu(), want2[1].cpu())
    ce.clear_pixel_weight()
    assert ce.pixel_weight is None and ce.pixel_norm == 'weight'


def test_trainer_passes_the_map_and_a_captured_step_follows_an_update():
    """engine.Trainer hands loss_fn.pixel_weight to the fused head: FastSCNN in bf16 at 2x3x64x128; two steps, the map updated in place
    between them -- captured equals eager on bits, and the second step is another one than without the update"""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    from tests.test_gpu_selftrain_trainer import batches, same_bits, snapshot, student
    x, y, _ = batches()
    g = X.case_gen(97)
    om = (torch.randint(0, 17, (2, 64, 128), generator=g).float() / 8).to(DEV)

    def go(use_graph, update):
        m = student()
        ce = tssa.CrossEntropyLoss(ignore_index=IGN)
        wmap = om.clone()
        ce.set_pixel_weight(wmap)
        tr = E.Trainer(m, E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5), ce, use_graph=use_graph)
        l1 = tr.step_async(x, y).clone()
        if update:
            wmap[:, :32] = 0.0
        l2 = tr.step_async(x, y).clone()
        assert bool(tr._graphs) == use_graph
        return torch.stack([l1, l2]).cpu(), snapshot(m)

    eg, gr, keep = go(False, True), go(True, True), go(True, False)
    assert bool(torch.isfinite(eg[0]).all())
    assert torch.equal(eg[0], gr[0])
    same_bits(eg[1], gr[1])
    assert float(keep[0][0]) == float(gr[0][0]) and float(keep[0][1]) != float(gr[0][1])
    # and the map really weighs in: the plain trainer's first loss is another number
    m = student()
    tr = E.Trainer(m, E.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-5), tssa.CrossEntropyLoss(ignore_index=IGN))
    assert float(tr.step_async(x, y)) != float(eg[0][0])
