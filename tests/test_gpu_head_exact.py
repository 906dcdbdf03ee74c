"""The fused decoder head -- csrc/loss.hip (upsample_ce_onepass_kernel MODE 0..4, upsample_argmax_kernel, the gather), csrc/widehead.hip
(the class-chunked twins), csrc/ohem.hip (the radix select), csrc/headgeom.h -- through the C ABI, elementwise against the f64 reference
X.HeadRef of tests/exact.py (section "fused decoder head"; its bounds run on the CPU in tests/test_exact_bounds.py, none comes from
what a GPU returned).  Harness: `low` at its pitch with NaN pad channels and NaN spare rows behind the last pixel; NaN-filled workspace,
per-pixel array and gradient; the gradient's pad channels must come back as exact zeros and its sentinel spare rows untouched; the
workspace size is asserted against the restated planner (X.head_geom) and the floats behind it must stay untouched.

Tiers:
  1  bit for bit, the arg-max kernels on every case of X.HEAD_REG / X.HEAD_WIDE (exact_resize pairs, logits multiples of 2^-2 in
     [-8, 8], X.exact_budget asserted per case, ties natural and planted by X.head_plants): tss_upsample_argmax_confusion(_wide) with a
     prediction and without, into a non-zero matrix; tss_multiscale_argmax_confusion(_wide) with average='logits' over four exact maps,
     two of them flipped; the planar tss_argmax_confusion(_wide) on the f64 logits themselves
  2  derived bounds, everything with an exponential on every case, and everything on X.HEAD_REG_T2 / X.HEAD_WIDE_T2 (pairs that are
     not exact: + X.head_slack; their arg-max by tests/msflip_ref.margin with K = 1, the share of undecided pixels <= 0.01):
       tss_upsample_pixel_ce(_wide)                  X.head_pix_bound; ignored and out-of-range pixels an exact 0; nothing below 0
       tss_upsample_ce_fwd, _fwd_ex, _wide_fwd       plain, class weights (one class of weight exactly 0), smoothing, both:
         then tss_upsample_ce_bwd / _wide_bwd        X.head_loss_bound, inv_count, X.head_grad_bound with grad_out = 0.7; the loss rows
                                                     in use against the restated block count; a second evaluation: the same bits
       tss_upsample_ohem_grad(_wide)                 hand-made sel rows on the kernel's own per-pixel losses: threshold mode, top-n mode
                                                     with a cut that a planted share of the pixels equals exactly, a sel that selects
                                                     nothing (exact zeros); gathered with inv_count = 1
  tss_ohem_select alone: loss within one f32 ulp of X.ohem_ref (oracle.recipe.ohem's rule, pinned in tests/test_exact_bounds.py), the
     mode and the cut's bits exactly, the weights within one ulp, the workspace zeroed again.
band32 / band64 (a band of 32 and of 64 rows, 2064 / 2080 blocks) run the arg-max, the per-pixel loss and the plain loss + gradient.
Every check prints its largest |out - ref| / bound as a line `HEAD_MARGIN ...` before it asserts (profiles/head_exact_margins.txt)."""
import copy
import math

import numpy as np
import pytest
import torch

from tests import exact as X
from tests import msflip_ref
from tests.exact_gpu import DEV, SPARE, Buf, N_, to_rows

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DT = {'f32': F32, 'bf16': BF}
IGN = 255
BIG = ('band32', 'band64')
U = X.U32


def sync():
    torch.cuda.synchronize()


def params(cases):
    return [pytest.param(c, d, id='%s-%s' % (c.name, d)) for c in cases for d in c.dtypes]


ALL_REG, ALL_WIDE = X.HEAD_REG + X.HEAD_REG_T2, X.HEAD_WIDE + X.HEAD_WIDE_T2
SMALL = [c for c in ALL_REG + ALL_WIDE if c.name not in BIG]

_refs = {}


def reference(case):
    """(x, labels, X.HeadRef) of a case, computed once; of the two large cases only the latest is kept"""
    if case.name not in _refs:
        for k in [k for k in _refs if k in BIG]:
            del _refs[k]
        x, labels, _ = X.head_inputs(case)
        _refs[case.name] = (x, labels, X.HeadRef(x, labels, ignore_index=IGN, weighted=False))
    return _refs[case.name]


def margin_line(case, dtype, entry, ratio):
    print('HEAD_MARGIN %-14s %-5s %-34s %.4f' % (case.name, 'bf16' if dtype == BF else 'f32', entry, ratio))


def suffix(case):
    return '_wide' if case.wide else ''


class Low:
    """the low-resolution logits of a case on the device: [B h w + SPARE][ldl], NaN pad channels, NaN spare rows"""
    def __init__(self, case, x, dtype):
        self.buf = Buf(case.B * case.h * case.w, case.C, case.ldl, 0, to_rows(x), dtype, nan_spare=True, nan_pad=True)
        assert torch.equal(self.buf.rows(), to_rows(x)), 'logits not exact in the dtype'
        self.ptr, self.ld = self.buf.ptr, case.ldl


class Grad:
    """the gradient buffer: NaN rows (pads included), sentinel spare rows"""
    def __init__(self, case, dtype):
        self.P, self.C, self.case, self.dtype = case.B * case.h * case.w, case.C, case, dtype
        t = X.sentinel((self.P + SPARE, case.ldl), dtype=dtype)
        t[:self.P] = float('nan')
        self.t = t.to(DEV)
        self.ptr = self.t.data_ptr()

    def check(self, what):
        t = self.t.cpu()
        c = self.case
        assert (t[:self.P, self.C:] == 0).all(), (what, 'pad channels of the gradient are not exact zeros')
        sb = X.SENTINEL_BITS32 if self.dtype == F32 else X.SENTINEL_BITS
        assert (X.bits(t[self.P:]) == sb).all(), (what, 'spare rows written')
        return X.nhwc_to_nchw(t.double(), c.B, c.h, c.w, c.C)


class Workspace:
    """NaN-filled floats of the size the library asks for (asserted against the restated planner) + 64 floats that must stay untouched"""
    def __init__(self, case):
        n = N_()
        self.geo = case.geom()
        q = n.lib().tss_upsample_ce_wide_ws if case.wide else n.lib().tss_upsample_ce_ws
        self.n = q(case.B, case.C, case.h, case.w, case.H, case.W)
        assert self.n == self.geo['ws_floats'], ('workspace floats', self.n, 'restated', self.geo['ws_floats'])
        self.t = torch.full((self.n + 64,), float('nan'), dtype=F32)
        self.t[self.n:] = 7.25
        self.t = self.t.to(DEV)
        self.ptr = self.t.data_ptr()

    def check(self, what, rows=True):
        t = self.t.cpu()
        assert (t[self.n:] == 7.25).all(), (what, 'floats behind the workspace written')
        if rows:       # the loss rows in use: two doubles per restated block, every one written
            r = t[:4 * self.geo['nblocks']].view(torch.float64).reshape(-1, 2)
            assert r.shape[0] == self.geo['nblocks'] and not torch.isnan(r).any(), (what, 'loss rows')
            assert (r[:, 1] >= 0).all(), (what, 'a block counted a negative weight')
        return t


def labels_dev(labels):
    return labels.to(DEV).contiguous()


def shape_args(c):
    return (c.B, c.C, c.h, c.w, c.H, c.W)


def tier1_premise(case, ref):
    """the size pair is exact on both axes and every partial sum of a blend is an f32 number"""
    ky, kx = X.exact_resize(case.h, case.H), X.exact_resize(case.w, case.W)
    assert ky is not None and kx is not None, 'not an exact_resize pair'
    assert X.lsb_exp(ref.x) >= -2 and ref.zmax <= 8
    assert X.exact_budget(ref.zabs, -2, ky, kx), 'the interpolated logits do not fit 24 bits'


def check_argmax(case, dtype, pred, ref, labels, entry, cm=None, cm0=None):
    """tier 1: every pixel; tier 2: every pixel whose top-2 gap exceeds the margin; the counts of those pixels exactly"""
    pred = pred.cpu().long()
    if case.exact:
        tier1_premise(case, ref)
        bad = (pred != ref.arg).nonzero()
        assert bad.numel() == 0, (entry, case, dtype, 'tier 1: differs at', bad[:3].tolist(), len(bad), 'pixels')
        decided = torch.ones_like(ref.arg, dtype=torch.bool)
    else:
        m = msflip_ref.margin(1, case.C, ref.zmax, [(case.h, case.w)], (case.H, case.W), 'logits')
        decided = ref.gap > m
        share = 1.0 - float(decided.double().mean())
        print('HEAD_MARGIN %-14s %-5s %-34s undecided share %.6f margin %.3e' % (case.name, 'bf16' if dtype == BF else 'f32', entry, share, m))
        assert share <= 0.01, (entry, case, 'undecided share', share)
        bad = ((pred != ref.arg) & decided).nonzero()
        assert bad.numel() == 0, (entry, case, dtype, 'tier 2: differs at', bad[:3].tolist(), len(bad), 'decided pixels')
    if cm is not None:
        lab = torch.where(decided, labels, torch.full_like(labels, IGN))
        got = cm.cpu().long() - cm0
        und = msflip_ref.confusion(pred, torch.where(decided, torch.full_like(labels, IGN), labels), case.C, IGN)
        assert torch.equal(got - und, msflip_ref.confusion(ref.arg, lab, case.C, IGN)), (entry, case, dtype, 'confusion matrix')


# ----------------------------------------------------------------------------------------------------- arg-max (tier 1 / margin)
@pytest.mark.parametrize('case,d', params(ALL_REG + ALL_WIDE))
def test_upsample_argmax(case, d):
    n, dtype = N_(), DT[d]
    x, labels, ref = reference(case)
    low, tgt = Low(case, x, dtype), labels_dev(labels)
    entry = 'tss_upsample_argmax_confusion' + suffix(case)
    cm0 = (torch.arange(case.C * case.C).reshape(case.C, case.C) % 7 + 1).long()
    cm, cm2 = cm0.clone().to(DEV), cm0.clone().to(DEV)
    pred = torch.full((case.B, case.H, case.W), 255, dtype=torch.uint8, device=DEV)
    tail = (*shape_args(case), IGN, n.dtype_code(dtype), n.stream())
    n.call(entry, low.ptr, low.ld, tgt.data_ptr(), pred.data_ptr(), cm.data_ptr(), *tail)
    n.call(entry, low.ptr, low.ld, tgt.data_ptr(), None, cm2.data_ptr(), *tail)          # want_pred off
    sync()
    check_argmax(case, dtype, pred, ref, labels, entry, cm, cm0)
    assert torch.equal(cm, cm2), (entry, case, 'the matrix without a prediction differs')


MS_OUT = (33, 65)
MS_MAPS = ((5, 9, 0), (3, 5, 1), (33, 65, 0), (9, 17, 1))       # (h, w, flip): every pair exact_resize, the third the identity


@pytest.mark.parametrize('d', ['f32', 'bf16'])
@pytest.mark.parametrize('C', [19, 24, 33])
def test_multiscale_logits_tier1(C, d):
    """K exact maps summed in list order, flipped maps included: every z_k is a multiple of 2^-(2 + ky + kx) below 8, the sum of four
    stays an f32 number in any order, and the arg-max must be the f64 one at every pixel"""
    n, dtype = N_(), DT[d]
    from torch_semantic_segmentation_amd import ops
    B, (H, W) = 2, MS_OUT
    g = X.case_gen(77, C)
    labels = X.head_labels(B, H, W, C, g, IGN)
    total, keep, descs, worst = None, [], [], 0
    for (h, w, flip) in MS_MAPS:
        x = X.head_logits((B, C, h, w), g)
        X.head_plants(x, g)
        z = torch.einsum('oh,bchw,pw->bcop', X.bilinear_matrix(h, H), x, X.bilinear_matrix(w, W))
        total = (z.flip(-1) if flip else z) if total is None else total + (z.flip(-1) if flip else z)
        worst = max(worst, X.exact_resize(h, H) + X.exact_resize(w, W))
        case = X.HeadCase('ms', B, C, h, w, H, W)
        low = Low(case, x, dtype)
        keep.append(low)
        descs.append(ops._MsMap(low.ptr, low.ld, h, w, flip, 0))
    assert 8.0 * len(MS_MAPS) < 2.0 ** (24 - 2 - worst), 'the sum of the maps does not fit 24 bits'
    want = X.argmax_lowest(total)
    assert float((total.topk(2, dim=1).values.diff(dim=1) == 0).double().mean()) > 0, 'no tie among the pixels'
    entry = 'tss_multiscale_argmax_confusion' + ('_wide' if C > X.HEAD_REG_CAP else '')
    cm = torch.ones((C, C), dtype=torch.int64, device=DEV)
    pred = torch.full((B, H, W), 255, dtype=torch.uint8, device=DEV)
    n.call(entry, (ops._MsMap * len(descs))(*descs), len(descs), labels_dev(labels).data_ptr(), pred.data_ptr(), cm.data_ptr(), B, C, H, W, IGN,
           1, n.dtype_code(dtype), n.stream())
    sync()
    bad = (pred.cpu().long() != want).nonzero()
    assert bad.numel() == 0, (entry, C, dtype, 'differs at', bad[:3].tolist(), len(bad), 'pixels')
    assert torch.equal(cm.cpu() - 1, msflip_ref.confusion(want, labels, C, IGN)), (entry, 'confusion matrix')


@pytest.mark.parametrize('d', ['f32', 'bf16'])
@pytest.mark.parametrize('name', ['one_lane_strip', 'cp24', 'c66', 'c97', 'c256'])
def test_planar_argmax_tier1(name, d):
    """the planar kernels on the case's low-resolution logits themselves (no arithmetic: the f64 arg-max, lowest index on ties)"""
    n, dtype = N_(), DT[d]
    case = X.HEAD_BY_NAME[name]
    x, _, _ = X.head_inputs(case)
    HW = case.h * case.w // 8 * 8
    x = x.reshape(case.B, case.C, -1)[:, :, :HW].contiguous()
    C = case.C
    for p, pair in enumerate(((0, C - 1), (3, 4), (15, 16))):          # ties of the maximum: first | last class, across the groups of 4 / 16
        x[:, :, p] = x[:, :, p].clamp(max=7.75)
        x[:, pair, p] = 8.0
    x[:, :, 3] = 1.0                                                    # every class equal
    g = X.case_gen(78, case.C)
    labels = X.head_labels(case.B, 1, HW, case.C, g, IGN)
    want = X.argmax_lowest(x)
    assert (want[:, :4] == torch.tensor([0, 3, 15, 0])).all()
    xd = x.to(dtype).to(DEV)
    cm = torch.ones((case.C, case.C), dtype=torch.int64, device=DEV)
    pred = torch.full((case.B, HW), 255, dtype=torch.uint8, device=DEV)
    entry = 'tss_argmax_confusion' + ('_wide' if case.C > 64 or case.wide else '')
    n.call(entry, xd.data_ptr(), labels_dev(labels).data_ptr(), pred.data_ptr(), cm.data_ptr(), case.B, case.C, HW, IGN, n.dtype_code(dtype),
           n.stream())
    sync()
    assert torch.equal(pred.cpu().long(), want), (entry, name, dtype)
    assert torch.equal(cm.cpu() - 1, msflip_ref.confusion(want, labels, case.C, IGN)), (entry, 'confusion matrix')


# ----------------------------------------------------------------------------------------------------- per-pixel cross-entropy
def pixel_ce(case, dtype, low, tgt):
    n = N_()
    pix = torch.full((case.B, case.H, case.W), float('nan'), dtype=F32, device=DEV)
    n.call('tss_upsample_pixel_ce' + suffix(case), low.ptr, low.ld, tgt.data_ptr(), pix.data_ptr(), *shape_args(case), IGN,
           n.dtype_code(dtype), n.stream())
    sync()
    return pix


@pytest.mark.parametrize('case,d', params(ALL_REG + ALL_WIDE))
def test_pixel_ce(case, d):
    dtype = DT[d]
    x, labels, ref = reference(case)
    low, tgt = Low(case, x, dtype), labels_dev(labels)
    pix = pixel_ce(case, dtype, low, tgt).cpu().double()
    assert not torch.isnan(pix).any(), 'a pixel was not written'
    assert (pix[~ref.valid] == 0).all(), 'an ignored or out-of-range pixel is not an exact 0'
    assert (pix >= 0).all(), 'a per-pixel loss below 0'
    n = case.counts()
    bound = X.head_pix_bound(ref.zmax, case.C, n['nchunk']) + 2.0 * X.head_slack_z(ref)
    err = (pix - ref.pix).abs()
    margin_line(case, dtype, 'pixel_ce', float(err.max()) / bound)
    at = np.unravel_index(int(err.argmax()), err.shape)
    assert float(err.max()) <= bound, ('tss_upsample_pixel_ce' + suffix(case), case, dtype, 'at (b, y, x)', at, float(err.max()), bound)


# ----------------------------------------------------------------------------------------------------- loss and gradient
def class_weights(C, g):
    """f32-exact class weights in (0.25, 2], one class of weight exactly 0"""
    cw = (torch.randint(1, 9, (C,), generator=g).double() / 4)
    cw[C // 2] = 0.0
    return cw


CE_VARIANTS = (('plain', False, 0.0), ('weights', True, 0.0), ('smooth', False, 0.125), ('both', True, 0.125))


def ce_forward(case, dtype, low, tgt, cw, eps, ws):
    """the entry a variant goes through: the plain tss_upsample_ce_fwd, its _ex twin, or the wide entry (which takes both)"""
    n = N_()
    loss = torch.full((2,), float('nan'), dtype=F32, device=DEV)
    cwd = cw.float().to(DEV) if cw is not None else None
    tail = (*shape_args(case), IGN, n.dtype_code(dtype), n.stream())
    if case.wide:
        n.call('tss_upsample_ce_wide_fwd', low.ptr, low.ld, tgt.data_ptr(), n.ptr(cwd), eps, ws.ptr, loss.data_ptr(), loss.data_ptr() + 4, *tail)
    elif cw is None and eps == 0.0:
        n.call('tss_upsample_ce_fwd', low.ptr, low.ld, tgt.data_ptr(), ws.ptr, loss.data_ptr(), loss.data_ptr() + 4, *tail)
    else:
        n.call('tss_upsample_ce_fwd_ex', low.ptr, low.ld, tgt.data_ptr(), n.ptr(cwd), eps, ws.ptr, loss.data_ptr(), loss.data_ptr() + 4, *tail)
    return loss


def ce_backward(case, dtype, ws, inv_ptr, gout):
    n = N_()
    grad = Grad(case, dtype)
    n.call('tss_upsample_ce_bwd' if not case.wide else 'tss_upsample_ce_wide_bwd', ws.ptr, inv_ptr, n.ptr(gout), grad.ptr, case.ldl,
           *shape_args(case), n.dtype_code(dtype), n.stream())
    sync()
    return grad


def check_grad(case, dtype, grad, r, weighted, entry):
    out = grad.check(entry)
    n = case.counts()
    assert not torch.isnan(out).any(), (entry, case, 'a gradient element was not written')
    bound = X.head_grad_bound(r, n, weighted, dtype == BF, n['nchunk'], X.head_slack(r)[2])
    err = (out - r.g).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float('inf'))))
    margin_line(case, dtype, entry, float(ratio.max()))
    at = np.unravel_index(int(ratio.argmax()), ratio.shape)
    assert float(ratio.max()) <= 1, (entry, case, dtype, 'at (b, class, row, cell)', at, float(err[at]), float(bound[at]), float(r.g[at]))
    return out


@pytest.mark.parametrize('case,d', params(ALL_REG + ALL_WIDE))
def test_ce_loss_and_gradient(case, d):
    dtype = DT[d]
    x, labels, ref = reference(case)
    low, tgt = Low(case, x, dtype), labels_dev(labels)
    cwv = class_weights(case.C, X.case_gen(79, case.C))
    gout = torch.tensor([0.7], dtype=F32, device=DEV)
    n = case.counts()
    for (name, weighted, eps) in (CE_VARIANTS[:1] if case.name in BIG else CE_VARIANTS):
        cw = cwv if weighted else None
        r = copy.copy(ref).weights(cw, eps, grad_out=float(np.float32(0.7)))
        entry = 'ce_%s%s' % (name, suffix(case))
        ws = Workspace(case)
        loss = ce_forward(case, dtype, low, tgt, cw, eps, ws)
        grad = ce_backward(case, dtype, ws, loss.data_ptr() + 4, gout)
        ws.check(entry)
        lv, inv = [float(v) for v in loss.cpu().double()]
        lb = X.head_loss_bound(r, n, weighted or eps > 0, n['nchunk'], X.head_slack(r)[1])
        margin_line(case, dtype, entry + ' loss', abs(lv - r.loss) / lb)
        assert abs(lv - r.loss) <= lb, (entry, case, dtype, 'loss', lv, r.loss, lb)
        assert abs(inv - 1.0 / r.den) <= U * (n['band_rows'] + 2) / r.den, (entry, case, 'inv_count', inv, 1.0 / r.den)
        out = check_grad(case, dtype, grad, r, weighted or eps > 0, entry + ' grad')
        # a second evaluation: the same bits, loss and gradient
        ws2 = Workspace(case)
        loss2 = ce_forward(case, dtype, low, tgt, cw, eps, ws2)
        grad2 = ce_backward(case, dtype, ws2, loss2.data_ptr() + 4, gout)
        assert torch.equal(X.bits(loss.cpu()), X.bits(loss2.cpu())) and torch.equal(out, grad2.check(entry)), (entry, case, 'not deterministic')


@pytest.mark.parametrize('case,d', params(SMALL))
def test_ohem_grad(case, d):
    n, dtype = N_(), DT[d]
    x, labels, ref = reference(case)
    low, tgt = Low(case, x, dtype), labels_dev(labels)
    pix = pixel_ce(case, dtype, low, tgt)
    g = X.case_gen(80, case.C, case.H)
    one = torch.ones(1, dtype=F32, device=DEV)
    cnt = case.counts()
    # top-n mode: a share of the pixels is planted AT the cut
    cut = float(np.float32(pix.cpu().median()))
    planted = pix.cpu().clone()
    planted[torch.rand(planted.shape, generator=g) < 0.1] = cut
    k = max(int((planted > 1.0).sum()), 1)
    sels = (('threshold', pix, [1.0, 1.0, float(np.float32(1.0 / k)), 0.5]),          # weq is ignored in threshold mode
            ('top_n', planted.to(DEV), [0.0, cut, 0.0078125, 0.00390625]),
            ('nothing', pix, [1.0, 1e30, 1.0, 1.0]))
    for (name, p, sel) in sels:
        entry = 'ohem_grad_%s%s' % (name, suffix(case))
        seld = torch.tensor(sel, dtype=F32, device=DEV)
        ws = Workspace(case)
        n.call('tss_upsample_ohem_grad' + suffix(case), low.ptr, low.ld, tgt.data_ptr(), p.data_ptr(), seld.data_ptr(), ws.ptr, *shape_args(case),
               IGN, n.dtype_code(dtype), n.stream())
        grad = ce_backward(case, dtype, ws, one.data_ptr(), None)
        ws.check(entry, rows=False)
        pw = X.ohem_pixel_weights(p.cpu(), seld.cpu())
        if name == 'top_n':
            assert float(((p.cpu() == cut) & ref.valid).double().mean()) > 0.05, 'no pixel at the cut'
        r = copy.copy(ref).weights(pixw=pw, grad_out=1.0)
        if name == 'nothing':
            out = grad.check(entry)
            assert (out == 0).all() and float(r.A.abs().max()) == 0, (entry, case, 'a sel that selects nothing: not exact zeros')
        else:
            assert r.ssum > 0
            check_grad(case, dtype, grad, r, False, entry)


# ----------------------------------------------------------------------------------------------------- tss_ohem_select
def ulp32(v):
    return float(np.spacing(np.float32(abs(v)))) if math.isfinite(v) else 0.0


def f32_bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def from_bits(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def select_arrays():
    """(name, f32 losses >= 0, thresh, n_top): every array at a length that fills the grid's uint4 groups evenly and one that does not"""
    rng = np.random.default_rng(5)
    out = []
    for n in (4096, 4100):
        base = rng.random(n).astype(np.float32) * 3
        srt = np.sort(base)[::-1]
        k = n // 16
        v = srt[k]                                     # the (k + 1)-th largest
        out += [('all_equal', np.full(n, 0.75, np.float32), 0.5, k), ('all_equal_low', np.full(n, 0.25, np.float32), 0.5, k),
                ('all_zero', np.zeros(n, np.float32), 0.3, k),
                ('v_eq_thresh', base, float(v), k),
                ('v_above_thresh', base, float(from_bits(f32_bits(v) - 1)), k),
                ('v_below_thresh', base, float(from_bits(f32_bits(v) + 1)), k),
                ('n_top_0_above', base, 0.3, 0), ('n_top_0_below', base, 5.0, 0),
                ('bits_0_9', from_bits(np.uint32(0x3F800000) + rng.integers(0, 1 << 10, n).astype(np.uint32)), 2.0, k),
                ('bits_10_20', from_bits(np.uint32(0x3F800000) + (rng.integers(0, 1 << 11, n).astype(np.uint32) << 10)), 4.0, k),
                ('bits_21_31', from_bits(rng.integers(0, 1016, n).astype(np.uint32) << 21), 1e38, k),       # below 2^127: finite
                ('denormals', np.where(rng.random(n) < 0.5, 0, from_bits(rng.integers(1, 64, n).astype(np.uint32))).astype(np.float32), 0.5, k)]
        ties = base.copy()
        ties[rng.permutation(n)[:4 * k]] = np.float32(1.75)          # a tie group at the cut, larger than n_top, with values above it
        out.append(('tie_group', ties, 2.5, int((ties > 1.75).sum()) + k))
    return out


SELECT = select_arrays()


@pytest.mark.parametrize('i', range(len(SELECT)), ids=['%s-%d' % (s[0], len(s[1])) for s in SELECT])
def test_ohem_select(i):
    n = N_()
    name, arr, thresh, n_top = SELECT[i]
    thresh = float(np.float32(thresh))
    pix = torch.from_numpy(np.ascontiguousarray(arr)).to(DEV)
    nbytes = n.lib().tss_ohem_workspace_bytes()
    wsb = torch.zeros(nbytes + 64, dtype=torch.uint8, device=DEV)
    out = torch.full((5,), float('nan'), dtype=F32, device=DEV)
    n.call('tss_ohem_select', pix.data_ptr(), wsb.data_ptr(), out.data_ptr(), out.data_ptr() + 4, len(arr), thresh, n_top, n.stream())
    sync()
    assert (wsb.cpu() == 0).all(), (name, 'the workspace did not come back zeroed')
    loss, mode, cut, wgt, weq = [float(v) for v in out.cpu().double()]
    rl, (rmode, rcut, rwgt, rweq) = X.ohem_ref(torch.from_numpy(arr), thresh, n_top)
    assert mode == rmode, (name, 'mode', mode, rmode)
    assert f32_bits(cut) == f32_bits(rcut), (name, 'cut bits', cut, rcut)
    if math.isnan(rl):
        assert math.isnan(loss), (name, 'an empty mean is nan', loss)
        return
    assert abs(loss - rl) <= ulp32(rl), (name, 'loss', loss, rl)
    assert abs(wgt - rwgt) <= ulp32(rwgt) and abs(weq - rweq) <= ulp32(rweq), (name, 'weights', wgt, rwgt, weq, rweq)
