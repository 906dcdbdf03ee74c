"""The planar cross-entropy and OHEM kernels -- tss_cross_entropy_fwd / _bwd (csrc/loss.hip) and tss_ohem_fwd / _bwd (csrc/ohem.hip), both on
the class-plane sweep of csrc/losssweep.h -- through the C ABI, ELEMENT BY ELEMENT against X.PlanarRef / X.PlanarCeRef of tests/exact.py
(section "planar cross-entropy and OHEM": the bounds are X.soft_lse_count and X.soft_p_count, counted from lsw::lse8 and lsw::grad8; none comes
from what a GPU returned).  tests/test_gpu_ops.py and tests/test_gpu_wce.py judge the gradient by a norm over the whole tensor.

Harness (tests/test_gpu_softloss_exact.py's): the logits between NaN guards, the gradient NaN-filled between sentinel guards; lse,
pixel_loss, loss, inv_count, params NaN-filled and the f64 sums zeroed, each with guard floats behind it; a second evaluation into fresh
buffers: the same bits.  Shapes X.PLANAR_CE_SHAPES: X.SOFT_PLANAR, X.SOFT_BEHIND and 4097 * 256 groups at C = 1, one block more than
tss::grid_for's cap, so that lanes take a second trip; X.planar_ce_operands with its planted pixels.
  tss_cross_entropy_fwd   lse per pixel within U32 soft_lse_count; acc[1] the exact valid count; acc[0] within the sum of the per-pixel bounds
                          of l - x_t; loss and inv_count one f32 rounding of the kernel's own acc
  tss_cross_entropy_bwd   every element within PlanarCeRef.grad (relative to (p_c + [c == t]) w, + 2^-8 for bf16); an exact zero of either
                          sign at pixels that do not count; grad_out = 0.7
  tss_ohem_fwd            lse bit-identical to the cross-entropy's; pixel_loss elementwise against max(lse - x_t, 0), an exact +0 where the
                          pixel does not count and at the planted pixel whose lse IS x_t; EVERY stored value has its sign bit clear (the
                          radix select ranks raw bit patterns); loss / params against X.ohem_ref on the kernel's own pixel_loss as
                          tests/test_gpu_head_exact.py::test_ohem_select does: both branches, ties at the cut, n_top = 0
  tss_ohem_bwd            every element with X.ohem_pixel_weights of the kernel's own pixel_loss and params
Every check prints its largest |out - ref| / bound as `PLANAR_MARGIN <case> <dtype> <entry> <ratio>` before it asserts
(profiles/lovasz_exact_margins.txt)."""
import math

import numpy as np
import pytest
import torch

from tests import exact as X
from tests.exact_gpu import DEV, N_
from tests.test_gpu_head_exact import f32_bits, ulp32
from tests.test_gpu_softloss_exact import GRAD_OUT, GUARD, GUARD_VALUE, Planes, guarded, guards_intact

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DT = {'f32': F32, 'bf16': BF}
IGN = 255
IDS = ['x'.join(str(v) for v in s) for s in X.PLANAR_CE_SHAPES]
_refs = {}


def margin_line(case, d, entry, ratio):
    print('PLANAR_MARGIN %-22s %-5s %-34s %.4f' % (case, d, entry, ratio))


def reference(shape):
    """(x, labels, plants, X.PlanarRef, X.PlanarCeRef), computed once; the large one is dropped when another shape comes"""
    if shape not in _refs:
        _refs.pop(X.PLANAR_CE_BIG, None)
        x, lab, plants = X.planar_ce_operands(shape)
        ref = X.PlanarRef(x, lab, IGN, True)
        _refs[shape] = (x, lab, plants, ref, X.PlanarCeRef(ref))
    return _refs[shape]


def name_of(shape):
    return 'planar_' + 'x'.join(str(v) for v in shape)


def ce_once(shape, x, lab, dtype):
    n = N_()
    B, C, HW = shape
    P = B * HW
    xb, tgt = Planes(shape, dtype, x), torch.from_numpy(lab).to(DEV).contiguous()
    lse, loss, inv, dx = guarded(P), guarded(1), guarded(1), Planes(shape, dtype)
    acc = torch.zeros(2 + GUARD, dtype=torch.float64)
    acc[2:] = GUARD_VALUE
    acc = acc.to(DEV)
    go = torch.tensor([GRAD_OUT], dtype=F32, device=DEV)
    code, st = n.dtype_code(dtype), n.stream()
    n.call('tss_cross_entropy_fwd', xb.ptr, tgt.data_ptr(), lse.data_ptr(), acc.data_ptr(), loss.data_ptr(), inv.data_ptr(), B, C, HW, IGN, code, st)
    n.call('tss_cross_entropy_bwd', xb.ptr, tgt.data_ptr(), lse.data_ptr(), inv.data_ptr(), go.data_ptr(), dx.ptr, B, C, HW, IGN, code, st)
    torch.cuda.synchronize()
    out = dict(lse=lse.cpu(), loss=loss.cpu(), inv=inv.cpu(), acc=acc.cpu())
    for k, m in (('lse', P), ('loss', 1), ('inv', 1)):
        assert guards_intact(out[k], m), (shape, k, 'guard floats written')
    assert (out['acc'][2:] == GUARD_VALUE).all(), (shape, 'guard doubles behind acc written')
    assert not torch.isnan(out['lse'][:P]).any(), (shape, 'an lse left unwritten')
    return out, dx


@pytest.mark.parametrize('d', ['f32', 'bf16'])
@pytest.mark.parametrize('shape', X.PLANAR_CE_SHAPES, ids=IDS)
def test_planar_cross_entropy(shape, d):
    dtype, (B, C, HW) = DT[d], shape
    x, lab, plants, ref, cr = reference(shape)
    name = name_of(shape)
    out, dx = ce_once(shape, x, lab, dtype)
    g = dx.check((name, d))
    lse = out['lse'][:B * HW].reshape(B, HW).double().numpy()
    acc0, acc1 = float(out['acc'][0]), float(out['acc'][1])
    r = dict(lse=X.worst_ratio(np.abs(lse - cr.lse), cr.lse_bound), acc0=X.worst_ratio(abs(acc0 - cr.total), cr.total_bound))
    assert acc1 == ref.nvalid, (name, d, 'valid count', acc1, ref.nvalid)
    assert ref.nvalid > 0
    want_loss, want_inv = np.float32(acc0 / acc1), np.float32(1.0 / acc1)
    assert f32_bits(out['loss'][0].item()) == f32_bits(want_loss) and f32_bits(out['inv'][0].item()) == f32_bits(want_inv), (name, d, 'loss / inv_count')
    gs = float(want_inv * np.float32(GRAD_OUT))                       # the f32 product the kernel forms
    want, bound = cr.grad(np.where(ref.valid, gs, 0.0), dtype == BF)
    r['grad'] = X.worst_ratio(np.abs(g - want), bound)
    for k, v in r.items():
        margin_line(name, d, 'tss_cross_entropy:' + k, v)
    assert (g.transpose(0, 2, 1)[~ref.valid] == 0).all(), (name, d, 'the gradient of a pixel that does not count is not an exact zero')
    assert max(r.values()) <= 1, (name, d, r)
    if shape != X.PLANAR_CE_BIG:
        out2, dx2 = ce_once(shape, x, lab, dtype)
        assert all(torch.equal(X.bits(out[k]), X.bits(out2[k])) for k in ('lse', 'inv')) and torch.equal(X.bits(dx.t.cpu()), X.bits(dx2.t.cpu())), (name, d, 'second evaluation')
        assert abs(float(out2['acc'][0]) - acc0) <= 2 * X.PLANAR_CE_SUM_REL * cr.total, (name, d, 'second evaluation: the atomic sum')


def ohem_once(shape, x, lab, dtype, thresh, n_top, backward=True):
    n = N_()
    B, C, HW = shape
    P = B * HW
    xb, tgt = Planes(shape, dtype, x), torch.from_numpy(lab).to(DEV).contiguous()
    lse, pix, loss, params = guarded(P), guarded(P), guarded(1), guarded(4)
    nbytes = n.lib().tss_ohem_workspace_bytes()
    wsb = torch.zeros(nbytes + 64, dtype=torch.uint8, device=DEV)
    go = torch.tensor([GRAD_OUT], dtype=F32, device=DEV)
    code, st = n.dtype_code(dtype), n.stream()
    n.call('tss_ohem_fwd', xb.ptr, tgt.data_ptr(), lse.data_ptr(), pix.data_ptr(), wsb.data_ptr(), loss.data_ptr(), params.data_ptr(), B, C, HW,
           IGN, thresh, n_top, code, st)
    dx = None
    if backward:
        dx = Planes(shape, dtype)
        n.call('tss_ohem_bwd', xb.ptr, tgt.data_ptr(), lse.data_ptr(), pix.data_ptr(), params.data_ptr(), go.data_ptr(), dx.ptr, B, C, HW, IGN, code, st)
    torch.cuda.synchronize()
    out = dict(lse=lse.cpu(), pix=pix.cpu(), loss=loss.cpu(), params=params.cpu())
    for k, m in (('lse', P), ('pix', P), ('loss', 1), ('params', 4)):
        assert guards_intact(out[k], m), (shape, k, 'guard floats written')
    assert (wsb.cpu() == 0).all(), (shape, 'the workspace did not come back zeroed')
    assert not torch.isnan(out['lse'][:P]).any() and not torch.isnan(out['pix'][:P]).any(), (shape, 'an lse or a pixel loss left unwritten')
    return out, dx


def ohem_selections(pix, nvalid):
    """(entry, thresh, n_top) on the kernel's own losses: the threshold branch, the top-n branch, n_top = 0 in both, a cut on a tie group
    (the zeros of the pixels that do not count and of the exact pixel: n_top reaches into them)"""
    P = pix.numel()
    k = max(1, P // 16)
    big = 1e30
    sel = [('thresh', 0.7, min(k, P - 1)), ('top_n', big, min(k, P - 1)), ('n_top_0_above', 0.0, 0), ('n_top_0_below', big, 0)]
    if nvalid < P:
        sel.append(('cut_in_the_zeros', big, P - 1))
    return sel


@pytest.mark.parametrize('d', ['f32', 'bf16'])
@pytest.mark.parametrize('shape', X.PLANAR_CE_SHAPES, ids=IDS)
def test_planar_ohem(shape, d):
    dtype, (B, C, HW) = DT[d], shape
    x, lab, plants, ref, cr = reference(shape)
    name, P = name_of(shape), B * HW
    ce_out, _ = ce_once(shape, x, lab, dtype)
    first = None
    for entry, thresh, n_top in ohem_selections(torch.empty(P), ref.nvalid):
        if shape == X.PLANAR_CE_BIG and entry not in ('thresh', 'top_n'):
            continue
        thresh = float(np.float32(thresh))
        out, dx = ohem_once(shape, x, lab, dtype, thresh, n_top)
        what = (name, d, entry)
        pix = out['pix'][:P]
        assert torch.equal(X.bits(out['lse'][:P]), X.bits(ce_out['lse'][:P])), (what, 'lse is not the cross-entropy\'s, bit for bit')
        pb = X.bits(pix).numpy().reshape(B, HW)
        assert (pb >= 0).all(), (what, 'a pixel loss with its sign bit set')
        assert (pb[~ref.valid] == 0).all(), (what, 'the loss of a pixel that does not count is not +0')
        if 'exact' in plants:
            assert pb[0, plants['exact']] == 0 and ref.valid[0, plants['exact']], (what, 'the pixel whose lse is x_t does not store +0')
        pl = pix.reshape(B, HW).double().numpy()
        r = dict(pixel_loss=X.worst_ratio(np.abs(pl - cr.ce), cr.ce_bound))
        if first is None:
            first = out
        else:
            assert torch.equal(X.bits(out['pix']), X.bits(first['pix'])), (what, 'the per-pixel losses depend on the selection')
        loss, (mode, cut, wgt, weq) = float(out['loss'][0]), [float(v) for v in out['params'][:4].double()]
        rl, (rmode, rcut, rwgt, rweq) = X.ohem_ref(pix, thresh, n_top)
        assert mode == rmode and f32_bits(cut) == f32_bits(rcut), (what, 'mode / cut', mode, rmode, cut, rcut)
        if math.isnan(rl):
            assert math.isnan(loss), (what, 'an empty mean is nan', loss)
            continue
        assert abs(loss - rl) <= ulp32(rl), (what, 'loss', loss, rl)
        assert abs(wgt - rwgt) <= ulp32(rwgt) and abs(weq - rweq) <= ulp32(rweq), (what, 'weights', wgt, rwgt, weq, rweq)
        sel = X.ohem_pixel_weights(pix, [mode, cut, wgt, weq]).float()         # the kernel's own selection, an f32 each
        w = (sel * torch.tensor(GRAD_OUT, dtype=F32)).double().numpy().reshape(B, HW)      # the f32 product the kernel forms
        want, bound = cr.grad(np.where(ref.valid, w, 0.0), dtype == BF)
        g = dx.check(what)
        r['grad'] = X.worst_ratio(np.abs(g - want), bound)
        for k, v in r.items():
            margin_line(name, d, 'tss_ohem %s:%s' % (entry, k), v)
        assert (g.transpose(0, 2, 1)[~ref.valid] == 0).all(), (what, 'the gradient of a pixel that does not count is not an exact zero')
        assert max(r.values()) <= 1, (what, r)
        if entry == 'thresh' and shape != X.PLANAR_CE_BIG:
            out2, dx2 = ohem_once(shape, x, lab, dtype, thresh, n_top)
            assert all(torch.equal(X.bits(out[k]), X.bits(out2[k])) for k in ('lse', 'pix', 'params')), (what, 'second evaluation')
            assert torch.equal(X.bits(dx.t.cpu()), X.bits(dx2.t.cpu())), (what, 'second evaluation: gradient')
