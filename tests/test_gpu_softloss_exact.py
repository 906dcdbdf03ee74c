"""The distillation kernels -- csrc/distill.hip, pixel- and channel-wise KL -- through the C ABI, ELEMENT BY ELEMENT against the f64
reference X.DistillRef of tests/exact.py (section "soft losses and distillation"; every bound there is counted from the kernel source and
proved on the CPU in tests/test_exact_bounds.py with the f32 emulation of tests/softloss_emu.py, none comes from what a GPU returned).
tests/test_gpu_distill.py compares the gradient by its largest element over the whole tensor; here every element, every saved statistic
and the loss have a bound of their own.

Harness: student, teacher and gradient at three different pitches (lds != ldt != ldd), the inputs' pad channels and spare rows NaN; the
statistics, the loss and the gradient NaN-filled before the call; the workspace NaN-filled, of exactly tss_distill_workspace_bytes
(asserted against the restated planner) with guard floats behind it, behind the statistics and behind the loss that must stay
untouched; the gradient's pad channels exact zeros, its sentinel spare rows untouched; a second evaluation into fresh buffers: the same
bits.  Operands: X.distill_operands (multiples of 2^-2 in [-8, 8], exact in bf16; the `hot` cases with logits of magnitude 200, held
to the same bounds without an exclusion); tau in {1, 4, 0.5, 3}; grad_out = 0.7.
  stats[.].x / .z   fl(max * inv_tau) of the f64 maximum, bit for bit
  stats[.].y / .w   X.distill_logz_bound per unit
  loss              X.distill_loss_bound
  gradient          X.distill_grad_bound per element (+ 2^-8 (|g| + bound) for a bf16 gradient)
Cases: X.distill_pixel_cases (C in {1, 7, 8, 9, 19, 25, 256} x B HW in {1, 257, 600}, the last under max_blocks = 1) and
X.distill_channel_cases (C in {8, 9, 19, 256} x HW in {1, ppb - 1, ppb + 1, 3 ppb + 2} x B in {1, 3} x max_blocks in {0, 1, 2, B}, and the
smallest shape whose split leaves an EMPTY item).

The planar focal and soft Dice kernels -- csrc/softloss.hip on the class-plane sweep of csrc/losssweep.h -- the same way, against
X.PlanarRef / X.FocalPlanarRef / X.DicePlanarRef: the logits between NaN guards, the gradient NaN-filled between sentinel guards, lse,
pixel_coef, loss, scale and the workspace (its size asserted against the restated grid) NaN-filled with guard floats behind them.
Shapes X.SOFT_PLANAR (one lane in the second block, groups that do not fill the last block, one to three Dice sweeps, 256 classes
with 255 a class or ignored) and X.SOFT_BEHIND, max_blocks in {0, 1, 2}; planted pixels whose target holds the maximum by 0, 2^-2 and
16 and lies 16 below it, an absent class and a class of one pixel.
  focal   gamma in {0, 0.5, 2} x both variants: lse, pixel_coef (an exact 0 where the pixel does not count), loss, every element of
          dlogits; scale = (float)((double)alpha / n) and the rows' valid count exactly; max_blocks changes no per-pixel bit
  Dice    smooth in {0, 1}, with and without the ignore index: lse, a_c, b_c, loss, every element of dlogits; the rows' N_c exactly
  an all-ignored target: exact zeros
tss_focal_coef_from_ce alone on hand-made cross-entropies, the focal and Dice passes of the fused head and the wide focal chain: see
the comments at their sections below.
Every check prints its largest |out - ref| / bound as a line `SOFT_MARGIN <case> <dtype> <entry> <ratio>` before it asserts
(profiles/softloss_exact_margins.txt)."""
import numpy as np
import pytest
import torch

from tests import exact as X
from tests.exact_gpu import DEV, SPARE, Buf, N_

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DT = {'f32': F32, 'bf16': BF}
GUARD = 64
GUARD_VALUE = 7.25
GRAD_OUT = 0.7
KIND_CODE = {'pixel': 0, 'channel': 1}


def margin_line(case, d, entry, ratio):
    print('SOFT_MARGIN %-36s %-5s %-28s %.4f' % (case, d, entry, ratio))


def guarded(n):
    """n NaN floats and GUARD floats of GUARD_VALUE behind them"""
    t = torch.full((n + GUARD,), float('nan'), dtype=F32)
    t[n:] = GUARD_VALUE
    return t.to(DEV)


def guards_intact(t, n):
    return bool((t[n:] == GUARD_VALUE).all())


class GradBuf:
    """[P + SPARE][ld]: NaN rows (pads included), sentinel spare rows"""
    def __init__(self, P, C, ld, dtype):
        self.P, self.C, self.dtype = P, C, dtype
        t = X.sentinel((P + SPARE, ld), dtype=dtype)
        t[:P] = float('nan')
        self.t = t.to(DEV)
        self.ptr = self.t.data_ptr()

    def check(self, what):
        t = self.t.cpu()
        assert (t[:self.P, self.C:] == 0).all(), (what, 'pad channels of the gradient are not exact zeros')
        assert (X.bits(t[self.P:]) == (X.SENTINEL_BITS32 if self.dtype == F32 else X.SENTINEL_BITS)).all(), (what, 'spare rows written')
        return t[:self.P, :self.C].double().numpy()


# ----------------------------------------------------------------------------------------------------- distillation
def distill_once(kind, s, t, B, C, HW, tau, cap, dtype):
    """one forward + backward into fresh buffers: (loss [1 + GUARD], stats, workspace, GradBuf, workspace floats)"""
    n = N_()
    P, ldc = B * HW, X.cdiv(C, 8) * 8
    lds, ldt, ldd = ldc, ldc + 8, ldc + 16
    rows = lambda v: torch.from_numpy(v.reshape(P, C))
    sb = Buf(P, C, lds, 0, rows(s), dtype, nan_spare=True, nan_pad=True)
    tb = Buf(P, C, ldt, 0, rows(t), dtype, nan_spare=True, nan_pad=True)
    assert torch.equal(sb.rows(), rows(s)) and torch.equal(tb.rows(), rows(t)), 'operands not exact in the dtype'
    units = P if kind == 'pixel' else B * C
    nbytes = n.lib().tss_distill_workspace_bytes(KIND_CODE[kind], B, C, HW, cap)
    want = 16 * X.distill_pixel_grid(P, cap) if kind == 'pixel' else 4 * X.distill_channel_split(B, C, HW, cap)['ws_floats']
    assert nbytes == want, ('workspace bytes', nbytes, 'restated', want)
    stats, ws, loss, grad = guarded(4 * units), guarded(nbytes // 4), guarded(1), GradBuf(P, C, ldd, dtype)
    go = torch.tensor([GRAD_OUT], dtype=F32, device=DEV)
    code, st = n.dtype_code(dtype), n.stream()
    n.call('tss_distill_%s_fwd' % kind, sb.ptr, lds, tb.ptr, ldt, stats.data_ptr(), ws.data_ptr(), loss.data_ptr(), B, C, HW, tau, cap, code, st)
    n.call('tss_distill_%s_bwd' % kind, sb.ptr, lds, tb.ptr, ldt, stats.data_ptr(), go.data_ptr(), grad.ptr, ldd, B, C, HW, tau, cap, code, st)
    torch.cuda.synchronize()
    return loss.cpu(), stats.cpu(), ws.cpu(), grad, nbytes // 4


def check_distill(kind, C, case, d):
    name, B, HW, cap, tau, hot = case
    dtype = DT[d]
    s, t = X.distill_operands(B, C, HW, 0, hot)
    ref = X.DistillRef(s, t, tau, kind, GRAD_OUT, cap)
    units = ref.units
    loss, stats, ws, grad, nws = distill_once(kind, s, t, B, C, HW, tau, cap, dtype)
    assert guards_intact(loss, 1) and guards_intact(stats, 4 * units) and guards_intact(ws, nws), (name, d, 'guard floats written')
    g = grad.check((name, d))
    st = stats[:4 * units].reshape(units, 4).numpy()
    assert not np.isnan(st).any() and not np.isnan(g).any() and np.isfinite(float(loss[0])), (name, d, 'an output left unwritten')
    if kind == 'pixel':                 # two doubles per block of the restated grid, every one written, the second a zero
        r = ws[:nws].view(torch.float64).reshape(-1, 2)
        assert not torch.isnan(r).any() and (r[:, 1] == 0).all(), (name, d, 'loss rows')
    else:                               # five rows per item; the columns of pad channels may hold anything, nobody reads them
        r = ws[:nws].reshape(-1, X.cdiv(C, 8) * 8)[:, :C]
        assert not torch.isnan(r).any(), (name, d, 'a partial row left unwritten')
    r = X.distill_ratios(ref, float(loss[0]), st, g.reshape(B, HW, C), dtype == BF)
    margin_line(name, d, 'tss_distill_%s_fwd:logz' % kind, r['logz'])
    margin_line(name, d, 'tss_distill_%s_fwd:loss' % kind, r['loss'])
    margin_line(name, d, 'tss_distill_%s_bwd' % kind, r['grad'])
    assert r['max'], (name, d, 'stats maxima are not fl(max * inv_tau) bit for bit')
    assert r['logz'] <= 1 and r['loss'] <= 1 and r['grad'] <= 1, (name, d, r)
    loss2, stats2, _, grad2, _ = distill_once(kind, s, t, B, C, HW, tau, cap, dtype)
    assert torch.equal(X.bits(loss2[:1]), X.bits(loss[:1])) and torch.equal(X.bits(stats2), X.bits(stats)), (name, d, 'second evaluation')
    assert torch.equal(X.bits(grad2.t.cpu()), X.bits(grad.t.cpu())), (name, d, 'second evaluation: gradient')


@pytest.mark.parametrize('d', ['f32', 'bf16'])
@pytest.mark.parametrize('C', X.DISTILL_PIXEL_C)
def test_distill_pixel(C, d):
    for case in X.distill_pixel_cases(C):
        check_distill('pixel', C, case, d)


@pytest.mark.parametrize('d', ['f32', 'bf16'])
@pytest.mark.parametrize('C', X.DISTILL_CHANNEL_C)
def test_distill_channel(C, d):
    for case in X.distill_channel_cases(C):
        check_distill('channel', C, case, d)


# ----------------------------------------------------------------------------------------------------- planar focal and Dice
ALPHA = 0.25
IGN = 255
PLANAR = X.SOFT_PLANAR + [X.SOFT_BEHIND]
PLANAR_IDS = ['x'.join(str(v) for v in s) for s in PLANAR]
_planar = {}


def planar(shape):
    """(x, labels, {has_ignore: X.PlanarRef}) of a shape, computed once"""
    if shape not in _planar:
        x, lab, _ = X.soft_planar_operands(*shape, behind=shape == X.SOFT_BEHIND)
        _planar[shape] = (x, lab, {h: X.PlanarRef(x, lab, IGN, h) for h in (True, False)})
    return _planar[shape]


class Planes:
    """[B][C][HW] planes inside an allocation with FRONT elements before and behind them: NaN for an input (a read outside the
    tensor poisons the result), the sentinel for an output that is NaN-filled itself"""
    FRONT = 64

    def __init__(self, shape, dtype, values=None):
        n = int(np.prod(shape))
        self.shape, self.n, self.dtype = shape, n, dtype
        if values is None:
            flat = X.sentinel((n + 2 * self.FRONT,), dtype=dtype)
            flat[self.FRONT:self.FRONT + n] = float('nan')
        else:
            flat = torch.full((n + 2 * self.FRONT,), float('nan'), dtype=dtype)
            flat[self.FRONT:self.FRONT + n] = torch.from_numpy(values).reshape(-1).to(dtype)
            assert torch.equal(flat[self.FRONT:self.FRONT + n].double(), torch.from_numpy(values).reshape(-1)), 'logits not exact in the dtype'
        self.t = flat.to(DEV)
        self.ptr = self.t.data_ptr() + flat.element_size() * self.FRONT

    def check(self, what):
        t = self.t.cpu()
        sb = X.SENTINEL_BITS32 if self.dtype == F32 else X.SENTINEL_BITS
        assert (X.bits(t[:self.FRONT]) == sb).all() and (X.bits(t[self.FRONT + self.n:]) == sb).all(), (what, 'written outside the gradient')
        out = t[self.FRONT:self.FRONT + self.n].double().numpy().reshape(self.shape)
        assert not np.isnan(out).any(), (what, 'a gradient element left unwritten')
        return out


def focal_once(shape, x, lab, gamma, variant, cap, dtype):
    n = N_()
    B, C, HW = shape
    P = B * HW
    nbytes = n.lib().tss_focal_workspace_bytes(B, HW, cap)
    assert nbytes == 16 * X.soft_grid(B, HW, cap, X.SOFT_FOCAL_BLOCKS)[0], ('workspace bytes', nbytes)
    xb, tgt = Planes(shape, dtype, x), torch.from_numpy(lab).to(DEV).contiguous()
    lse, coef, ws, loss, scale, dx = guarded(P), guarded(P), guarded(nbytes // 4), guarded(1), guarded(1), Planes(shape, dtype)
    go = torch.tensor([GRAD_OUT], dtype=F32, device=DEV)
    code, st = n.dtype_code(dtype), n.stream()
    n.call('tss_focal_fwd', xb.ptr, tgt.data_ptr(), lse.data_ptr(), coef.data_ptr(), ws.data_ptr(), loss.data_ptr(), scale.data_ptr(),
           B, C, HW, IGN, 1, ALPHA, gamma, variant, cap, code, st)
    n.call('tss_focal_bwd', xb.ptr, tgt.data_ptr(), lse.data_ptr(), coef.data_ptr(), scale.data_ptr(), go.data_ptr(), dx.ptr,
           B, C, HW, cap, code, st)
    torch.cuda.synchronize()
    out = dict(lse=lse.cpu(), coef=coef.cpu(), ws=ws.cpu(), loss=loss.cpu(), scale=scale.cpu())
    for k, m in (('lse', P), ('coef', P), ('ws', nbytes // 4), ('loss', 1), ('scale', 1)):
        assert guards_intact(out[k], m), (shape, k, 'guard floats written')
        filled = out[k][:m].view(torch.float64) if k == 'ws' else out[k][:m]          # the loss rows are doubles
        assert not torch.isnan(filled).any(), (shape, k, 'left unwritten')
    return out, dx


@pytest.mark.parametrize('d', ['f32', 'bf16'])
@pytest.mark.parametrize('shape', PLANAR, ids=PLANAR_IDS)
def test_planar_focal(shape, d):
    """tss_focal_fwd + tss_focal_bwd for gamma in {0, 0.5, 2} x both variants x max_blocks in {0, 1, 2}: lse, pixel_coef, loss and
    every gradient element within their bounds, scale the exact (float)((double)alpha / n), the valid count of the loss rows exact"""
    dtype, (B, C, HW) = DT[d], shape
    x, lab, refs = planar(shape)
    ref, name = refs[True], 'planar_' + 'x'.join(str(v) for v in shape)
    for gamma in X.SOFT_GAMMAS:
        for variant in (0, 1):
            fr = X.FocalPlanarRef(ref, gamma, variant, ALPHA, GRAD_OUT)
            worst, first = {}, None
            for cap in (0, 1, 2):
                out, dx = focal_once(shape, x, lab, gamma, variant, cap, dtype)
                what = (name, d, gamma, variant, cap)
                g = dx.check(what)
                rows = out['ws'][:-GUARD].view(torch.float64).reshape(-1, 2)
                assert float(rows[:, 1].sum()) == ref.nvalid, (what, 'valid count')
                assert (out['coef'][:B * HW].reshape(B, HW).numpy()[~ref.valid] == 0).all(), (what, 'coef of a pixel that does not count')
                r = X.focal_planar_ratios(fr, out['lse'][:B * HW].reshape(B, HW).numpy(), out['coef'][:B * HW].reshape(B, HW).numpy(),
                                          float(out['loss'][0]), float(out['scale'][0]), g, dtype == BF)
                assert r['scale'], (what, 'scale is not (float)((double)alpha / n)')
                for k in ('lse', 'coef', 'loss', 'grad'):
                    worst[k] = max(worst.get(k, 0.0), r[k])
                bits_now = [X.bits(out[k]) for k in ('lse', 'coef', 'scale')] + [X.bits(dx.t.cpu())]
                if first is None:
                    first = bits_now
                    out2, dx2 = focal_once(shape, x, lab, gamma, variant, cap, dtype)
                    again = [X.bits(out2[k]) for k in ('lse', 'coef', 'scale')] + [X.bits(dx2.t.cpu())]
                    assert all(torch.equal(a, b) for a, b in zip(first, again)) and torch.equal(X.bits(out['loss']), X.bits(out2['loss'])), (what, 'second evaluation')
                else:           # the grid changes the order of the f64 loss rows only: everything per pixel keeps its bits
                    assert all(torch.equal(a, b) for a, b in zip(first, bits_now)), (what, 'max_blocks changes a per-pixel result')
            for k in ('lse', 'coef', 'loss', 'grad'):
                margin_line(name, d, 'tss_focal g%.1f v%d:%s' % (gamma, variant, k), worst[k])
            assert max(worst.values()) <= 1, (name, d, gamma, variant, worst)


def dice_once(shape, x, lab, smooth, has_ignore, cap, dtype):
    n = N_()
    B, C, HW = shape
    P = B * HW
    nbytes = n.lib().tss_dice_workspace_bytes(B, C, HW, cap)
    grid = X.soft_grid(B, HW, cap, X.SOFT_DICE_BLOCKS)[0]
    coef_bytes = X.cdiv(8 * C, 256) * 256
    assert nbytes == coef_bytes + 24 * C * grid, ('workspace bytes', nbytes)
    xb, tgt = Planes(shape, dtype, x), torch.from_numpy(lab).to(DEV).contiguous()
    lse, ws, loss, dx = guarded(P), guarded(nbytes // 4), guarded(1), Planes(shape, dtype)
    go = torch.tensor([GRAD_OUT], dtype=F32, device=DEV)
    code, st = n.dtype_code(dtype), n.stream()
    n.call('tss_dice_fwd', xb.ptr, tgt.data_ptr(), lse.data_ptr(), ws.data_ptr(), loss.data_ptr(), B, C, HW, IGN, int(has_ignore), smooth,
           cap, code, st)
    n.call('tss_dice_bwd', xb.ptr, tgt.data_ptr(), lse.data_ptr(), ws.data_ptr(), go.data_ptr(), dx.ptr, B, C, HW, IGN, int(has_ignore),
           cap, code, st)
    torch.cuda.synchronize()
    out = dict(lse=lse.cpu(), ws=ws.cpu(), loss=loss.cpu())
    for k, m in (('lse', P), ('ws', nbytes // 4), ('loss', 1)):
        assert guards_intact(out[k], m), (shape, k, 'guard floats written')
    assert not torch.isnan(out['lse'][:P]).any() and not torch.isnan(out['loss'][:1]).any()
    out['coef'] = out['ws'][:2 * C]
    assert torch.isnan(out['ws'][2 * C:coef_bytes // 4]).all(), (shape, 'floats between the coefficients and the rows written')
    out['rows'] = out['ws'][coef_bytes // 4:nbytes // 4].view(torch.float64).reshape(grid, 3, C)
    assert not torch.isnan(out['coef']).any() and not torch.isnan(out['rows']).any(), (shape, 'coefficients or rows left unwritten')
    return out, dx


@pytest.mark.parametrize('d', ['f32', 'bf16'])
@pytest.mark.parametrize('shape', PLANAR, ids=PLANAR_IDS)
def test_planar_dice(shape, d):
    """tss_dice_fwd + tss_dice_bwd for smooth in {0, 1}, with and without the ignore index, max_blocks in {0, 1, 2}: lse, a_c, b_c,
    loss and every gradient element within their bounds; the counts N_c of the rows exact"""
    dtype, (B, C, HW) = DT[d], shape
    x, lab, refs = planar(shape)
    name = 'planar_' + 'x'.join(str(v) for v in shape)
    for has_ignore in (True, False):
        for smooth in (0.0, 1.0):
            for cap in (0, 1, 2):
                dr = X.DicePlanarRef(refs[has_ignore], smooth, GRAD_OUT, cap)
                out, dx = dice_once(shape, x, lab, smooth, has_ignore, cap, dtype)
                what = (name, d, has_ignore, smooth, cap)
                g = dx.check(what)
                assert np.array_equal(out['rows'][:, 2].sum(0).numpy(), dr.N), (what, 'class counts')
                r = X.dice_planar_ratios(dr, out['lse'][:B * HW].reshape(B, HW).numpy(), out['coef'].numpy(), float(out['loss'][0]), g, dtype == BF)
                for k in ('lse', 'a', 'b', 'loss', 'grad'):
                    margin_line(name, d, 'tss_dice ign%d s%.0f cap%d:%s' % (has_ignore, smooth, cap, k), r[k])
                assert max(r.values()) <= 1, (what, r)
                if cap == 0:
                    out2, dx2 = dice_once(shape, x, lab, smooth, has_ignore, cap, dtype)
                    assert torch.equal(X.bits(out2['lse']), X.bits(out['lse'])) and torch.equal(X.bits(out2['coef']), X.bits(out['coef'])), what
                    assert torch.equal(X.bits(out2['loss']), X.bits(out['loss'])) and torch.equal(X.bits(dx2.t.cpu()), X.bits(dx.t.cpu())), what


@pytest.mark.parametrize('d', ['f32', 'bf16'])
def test_planar_all_ignored_gives_exact_zeros(d):
    dtype, shape = DT[d], (3, 19, 1000)
    x, lab, _ = planar(shape)
    none = np.full_like(lab, IGN)
    out, dx = focal_once(shape, x, none, 2.0, 0, 0, dtype)
    assert float(out['loss'][0]) == 0 and float(out['scale'][0]) == 0 and (out['coef'][:-GUARD] == 0).all() and (dx.check('focal') == 0).all()
    out, dx = dice_once(shape, x, none, 1.0, True, 0, dtype)
    assert float(out['loss'][0]) == 0 and (out['coef'] == 0).all() and (dx.check('dice') == 0).all()


# ----------------------------------------------------------------------------------------------------- the wide route's planar step
@pytest.mark.parametrize('n', X.SOFT_CE_N)
def test_focal_coef_from_ce_alone(n):
    """tss_focal_coef_from_ce on hand-made cross-entropies (X.soft_ce_operands: 0, a denormal, 2^-24, 1, 40, 200 in a tail group and in
    whole ones), every gamma and both variants, against the f64 focal terms of p = exp(-ce), q = -expm1(-ce) on the stored f32 ce:
    coef per pixel, an EXACT 0 at ignored and out-of-range labels, loss, scale and the valid count; rows of exactly
    tss_focal_coef_rows doubles pairs, guards behind everything"""
    lib, C = N_(), 19
    ce, lab = X.soft_ce_operands(n, C)
    nrows = lib.lib().tss_focal_coef_rows(n)
    assert nrows == X.cdiv(X.cdiv(n, 4), X.SOFT_NT) and lib.lib().tss_focal_coef_rows(0) == 0
    tgt = torch.from_numpy(lab).to(DEV).contiguous()
    for gamma in X.SOFT_GAMMAS:
        for variant in (0, 1):
            r = X.focal_coef_ref(ce, lab, C, gamma, variant, ALPHA, IGN, True)
            got = []
            for _ in range(2):
                pix, rows, loss, scale = guarded(n), guarded(4 * nrows), guarded(1), guarded(1)
                pix[:n] = torch.from_numpy(ce).to(DEV)
                lib.call('tss_focal_coef_from_ce', pix.data_ptr(), tgt.data_ptr(), rows.data_ptr(), loss.data_ptr(), scale.data_ptr(), n, C, IGN, 1,
                         ALPHA, gamma, variant, lib.stream())
                torch.cuda.synchronize()
                got.append([v.cpu() for v in (pix, rows, loss, scale)])
            pix, rows, loss, scale = got[0]
            what = (n, gamma, variant)
            assert guards_intact(pix, n) and guards_intact(rows, 4 * nrows) and guards_intact(loss, 1) and guards_intact(scale, 1), what
            rr = rows[:4 * nrows].view(torch.float64).reshape(nrows, 2)
            assert not torch.isnan(rr).any() and float(rr[:, 1].sum()) == r['nvalid'], (what, 'rows')
            cf = pix[:n].numpy()
            assert (cf[~r['valid']] == 0).all(), (what, 'coef of a pixel that does not count')
            assert float(scale[0]) == r['scale'], (what, 'scale')
            rc = X.worst_ratio(np.abs(cf.astype(np.float64) - r['coef']), r['coef_bound'])
            rl = X.worst_ratio(abs(float(loss[0]) - r['loss']), r['loss_bound'])
            margin_line('coef_from_ce_n%d' % n, 'f32', 'g%.1f v%d:coef' % (gamma, variant), rc)
            margin_line('coef_from_ce_n%d' % n, 'f32', 'g%.1f v%d:loss' % (gamma, variant), rl)
            assert rc <= 1 and rl <= 1, (what, rc, rl)
            assert all(torch.equal(X.bits(a), X.bits(b)) for a, b in zip(got[0], got[1])), (what, 'second evaluation')


# ----------------------------------------------------------------------------------------------------- the fused head: focal and Dice
# tss_upsample_focal_fwd + tss_upsample_ce_bwd and tss_upsample_dice_fwd + tss_upsample_dice_grad + tss_upsample_ce_bwd (csrc/softhead.hip)
# with the harness of tests/test_gpu_head_exact.py -- `low` at its pitch with NaN pad channels and NaN spare rows, a NaN-filled
# workspace of the restated size with untouched floats behind it, a NaN-filled gradient whose pad channels come back as exact zeros
# and whose sentinel rows stay -- against X.HeadFocalRef / X.HeadDiceRef: loss, scale, the valid count of the loss rows, the Dice a_c /
# b_c at coef[c] / coef[24 + c] with exact zeros past C and N_c exact, every element of the gathered gradient with grad_out = 0.7.
# Cases: X.HEAD_REG without band64 (band32 once per loss, f32) and X.HEAD_REG_T2 with head_slack; focal gamma in {0, 0.5, 2} x both
# variants with X.head_focal_plants; Dice smooth in {0, 1}, an absent class, a class of one pixel, has_ignore = 0 (passed with an
# ignore_index that IS a class with pixels, which must then count), and the rare-class
# operands where C > 20.  An all-ignored target: exact zeros.
from tests.test_gpu_head_exact import Low, Workspace, ce_backward, labels_dev, shape_args      # noqa: E402

HEAD_CASES = [c for c in X.HEAD_REG + X.HEAD_REG_T2 if c.name != 'band64']
NOIGN_CLASS = 3       # the ignore_index passed along with has_ignore = 0: the class the soft operands move class 1's pixels to
_head = {}


def head_params():
    return [pytest.param(c, d, id='%s-%s' % (c.name, d)) for c in HEAD_CASES for d in (c.dtypes if c.name != 'band32' else ('f32',))]


def head_reference(case, kind, rare=False, ignore_index=IGN):
    """(x, labels, X.HeadRef) of a case's focal or Dice operands, computed once; band32's is dropped when another one comes"""
    key = (case.name, kind, rare, ignore_index)
    if key not in _head:
        for k in [k for k in _head if k[0] == 'band32']:
            del _head[k]
        x, labels, _ = X.head_soft_inputs(case, rare=rare, focal=kind == 'focal')
        _head[key] = (x, labels, X.HeadRef(x, labels, ignore_index=ignore_index, weighted=False))
    return _head[key]


def check_head_grad(case, d, entry, grad, g, bound):
    out = grad.check(entry)
    assert not torch.isnan(out).any(), (entry, case, 'a gradient element was not written')
    ratio = X.worst_ratio((out - g).abs().numpy(), bound.numpy())
    margin_line(case.name, d, entry, ratio)
    assert ratio <= 1, (entry, case, d, ratio)
    return out


def focal_head_once(case, dtype, low, tgt, gamma, variant, gout):
    n = N_()
    ws, out = Workspace(case), guarded(2)
    n.call('tss_upsample_focal_fwd', low.ptr, low.ld, tgt.data_ptr(), ws.ptr, out.data_ptr(), out.data_ptr() + 4, *shape_args(case), IGN, 1,
           ALPHA, gamma, variant, n.dtype_code(dtype), n.stream())
    grad = ce_backward(case, dtype, ws, out.data_ptr() + 4, gout)
    return ws, out.cpu(), grad


@pytest.mark.parametrize('case,d', head_params())
def test_head_focal(case, d):
    dtype = DT[d]
    x, labels, ref = head_reference(case, 'focal')
    low, tgt = Low(case, x, dtype), labels_dev(labels)
    gout = torch.tensor([GRAD_OUT], dtype=F32, device=DEV)
    n = case.counts()
    for gamma in (X.SOFT_GAMMAS if case.name != 'band32' else (2.0,)):
        for variant in ((0, 1) if case.name != 'band32' else (0,)):
            f = X.HeadFocalRef(ref, gamma, variant, ALPHA, GRAD_OUT, n)
            entry = 'head_focal g%.1f v%d' % (gamma, variant)
            ws, out, grad = focal_head_once(case, dtype, low, tgt, gamma, variant, gout)
            rows = ws.check(entry)[:4 * ws.geo['nblocks']].view(torch.float64).reshape(-1, 2)
            assert guards_intact(out, 2) and float(rows[:, 1].sum()) == f.nvalid, (entry, case, 'guards or the valid count')
            assert float(out[1]) == f.scale, (entry, case, 'scale is not (float)((double)alpha / n)')
            rl = X.worst_ratio(abs(float(out[0]) - f.loss), f.loss_bound)
            margin_line(case.name, d, entry + ':loss', rl)
            assert rl <= 1, (entry, case, d, float(out[0]), f.loss, f.loss_bound)
            got = check_head_grad(case, d, entry + ':grad', grad, f.g, f.grad_bound(dtype == BF))
            if gamma == 2.0 and variant == 0:
                ws2, out2, grad2 = focal_head_once(case, dtype, low, tgt, gamma, variant, gout)
                assert torch.equal(X.bits(out2), X.bits(out)) and torch.equal(got, grad2.check(entry)), (entry, case, 'second evaluation')


def dice_head_once(case, dtype, low, tgt, smooth, has_ignore, gout, one):
    """has_ignore = 0 is passed with ignore_index = NOIGN_CLASS, a class that occurs: a kernel that ignored the flag would drop it"""
    n = N_()
    geo = case.geom()
    nfl = n.lib().tss_upsample_dice_ws(*shape_args(case))
    assert nfl == 64 + geo['nblocks'] * 3 * case.C * 2, ('Dice workspace floats', nfl)
    dws, loss, ws = guarded(nfl), guarded(1), Workspace(case)
    tail = (*shape_args(case), IGN if has_ignore else NOIGN_CLASS, int(has_ignore))
    n.call('tss_upsample_dice_fwd', low.ptr, low.ld, tgt.data_ptr(), dws.data_ptr(), loss.data_ptr(), *tail, smooth, n.dtype_code(dtype), n.stream())
    n.call('tss_upsample_dice_grad', low.ptr, low.ld, tgt.data_ptr(), dws.data_ptr(), ws.ptr, *tail, n.dtype_code(dtype), n.stream())
    grad = ce_backward(case, dtype, ws, one.data_ptr(), gout)
    dws, loss = dws.cpu(), loss.cpu()
    assert guards_intact(dws, nfl) and guards_intact(loss, 1), (case, 'guard floats written')
    ws.check('dice', rows=False)
    rows = dws[64:nfl].view(torch.float64).reshape(geo['nblocks'], 3, case.C)
    assert not torch.isnan(rows).any() and not torch.isnan(dws[:48]).any(), (case, 'rows or coefficients left unwritten')
    return dws[:48].numpy(), float(loss[0]), rows, grad


@pytest.mark.parametrize('case,d', head_params())
def test_head_dice(case, d):
    dtype, C = DT[d], case.C
    gout = torch.tensor([GRAD_OUT], dtype=F32, device=DEV)
    one = torch.ones(1, dtype=F32, device=DEV)
    big = case.name == 'band32'
    variants = ((1.0, False, IGN),) if big else ((0.0, False, IGN), (1.0, False, IGN), (1.0, False, None)) + (((1.0, True, IGN),) if C > 20 else ())
    for smooth, rare, ign in variants:
        x, labels, ref = head_reference(case, 'dice', rare, ign)
        low, tgt = Low(case, x, dtype), labels_dev(labels)
        dr = X.dice_ref(ref, smooth, GRAD_OUT, case.counts())
        assert ign is not None or dr.N[NOIGN_CLASS] > 0, (case, 'the class passed as ignore_index with has_ignore = 0 does not occur')
        entry = 'head_dice s%.0f%s%s' % (smooth, ' rare' if rare else '', ' noign' if ign is None else '')
        coef, loss, rows, grad = dice_head_once(case, dtype, low, tgt, smooth, ign is not None, gout, one)
        assert np.array_equal(rows[:, 2].sum(0).numpy(), dr.N), (entry, case, 'class counts')
        assert (coef[C:24] == 0).all() and (coef[24 + C:48] == 0).all(), (entry, case, 'coefficients past C are not zeros')
        r = dict(a=X.worst_ratio(np.abs(coef[:C] - dr.a), dr.da), b=X.worst_ratio(np.abs(coef[24:24 + C] - dr.b), dr.db),
                 loss=X.worst_ratio(abs(loss - dr.loss), dr.loss_bound))
        for k, v in r.items():
            margin_line(case.name, d, entry + ':' + k, v)
        assert max(r.values()) <= 1, (entry, case, d, r)
        got = check_head_grad(case, d, entry + ':grad', grad, dr.g, dr.grad_bound(dtype == BF))
        if smooth == 1.0 and not rare and ign is not None:
            coef2, loss2, _, grad2 = dice_head_once(case, dtype, low, tgt, smooth, True, gout, one)
            assert np.array_equal(coef, coef2) and loss == loss2 and torch.equal(got, grad2.check(entry)), (entry, case, 'second evaluation')


@pytest.mark.parametrize('d', ['f32', 'bf16'])
def test_head_all_ignored_gives_exact_zeros(d):
    dtype, case = DT[d], X.HEAD_BY_NAME['cp24']
    x, labels, _ = head_reference(case, 'dice')
    low, tgt = Low(case, x, dtype), labels_dev(torch.full_like(labels, IGN))
    gout, one = torch.tensor([GRAD_OUT], dtype=F32, device=DEV), torch.ones(1, dtype=F32, device=DEV)
    ws, out, grad = focal_head_once(case, dtype, low, tgt, 2.0, 0, gout)
    assert float(out[0]) == 0 and float(out[1]) == 0 and (grad.check('focal') == 0).all()
    coef, loss, rows, grad = dice_head_once(case, dtype, low, tgt, 1.0, True, gout, one)
    assert loss == 0 and (coef == 0).all() and (rows == 0).all() and (grad.check('dice') == 0).all()


# ----------------------------------------------------------------------------------------------------- the wide route of the focal loss
WIDE_CASES = [c for c in X.HEAD_WIDE + X.HEAD_WIDE_T2 if c.name != 'c130']


@pytest.mark.parametrize('case,d', [pytest.param(c, d, id='%s-%s' % (c.name, d)) for c in WIDE_CASES for d in c.dtypes])
def test_wide_focal_chain(case, d):
    """tss_upsample_pixel_ce_wide -> tss_focal_coef_from_ce -> tss_upsample_coef_grad_wide -> tss_upsample_ce_wide_bwd past 24 classes.
    The stored cross-entropy is tests/test_gpu_head_exact.py's (X.head_pix_bound); the coefficient array is held per pixel against
    X.focal_coef_ref ON THAT stored ce, an exact 0 at every pixel that does not count; the gathered gradient against
    HeadRef.weights(pixw = the array the kernel itself was given) times scale, as the OHEM selections are, with X.head_grad_bound"""
    import copy
    from tests.test_gpu_head_exact import pixel_ce, reference
    lib, dtype = N_(), DT[d]
    x, labels, ref = reference(case)
    low, tgt = Low(case, x, dtype), labels_dev(labels)
    gout = torch.tensor([GRAD_OUT], dtype=F32, device=DEV)
    n, cnt = case.B * case.H * case.W, case.counts()
    nrows = lib.lib().tss_focal_coef_rows(n)
    lab = labels.reshape(-1).numpy()
    for gamma, variant in ((2.0, 0), (0.5, 1), (0.0, 0)):
        entry = 'wide_focal g%.1f v%d' % (gamma, variant)
        pix = pixel_ce(case, dtype, low, tgt)
        ce = pix.cpu().reshape(-1).numpy().copy()
        rows, out = guarded(4 * nrows), guarded(2)
        lib.call('tss_focal_coef_from_ce', pix.data_ptr(), tgt.data_ptr(), rows.data_ptr(), out.data_ptr(), out.data_ptr() + 4, n, case.C, IGN, 1,
                 ALPHA, gamma, variant, lib.stream())
        ws = Workspace(case)
        lib.call('tss_upsample_coef_grad_wide', low.ptr, low.ld, tgt.data_ptr(), pix.data_ptr(), ws.ptr, *shape_args(case), IGN,
                 lib.dtype_code(dtype), lib.stream())
        grad = ce_backward(case, dtype, ws, out.data_ptr() + 4, gout)
        ws.check(entry, rows=False)
        out, coef = out.cpu(), pix.cpu().reshape(-1).numpy()
        assert guards_intact(out, 2) and guards_intact(rows.cpu(), 4 * nrows), (entry, case, 'guard floats written')
        r = X.focal_coef_ref(ce, lab, case.C, gamma, variant, ALPHA, IGN, True)
        assert np.array_equal(r['valid'], ref.valid.reshape(-1).numpy()) and (coef[~r['valid']] == 0).all(), (entry, case, 'coef of a pixel that does not count')
        assert float(out[1]) == r['scale'], (entry, case, 'scale')
        rc = X.worst_ratio(np.abs(coef.astype(np.float64) - r['coef']), r['coef_bound'])
        rl = X.worst_ratio(abs(float(out[0]) - r['loss']), r['loss_bound'])
        margin_line(case.name, d, entry + ':coef', rc)
        margin_line(case.name, d, entry + ':loss', rl)
        assert rc <= 1 and rl <= 1, (entry, case, d, rc, rl)
        hr = copy.copy(ref).weights(pixw=torch.from_numpy(coef.astype(np.float64)).reshape(labels.shape), grad_out=float(np.float32(GRAD_OUT)) * r['scale'])
        bound = X.head_grad_bound(hr, cnt, False, dtype == BF, cnt['nchunk'], X.head_slack(hr)[2])
        check_head_grad(case, d, entry + ':grad', grad, hr.g, bound)
