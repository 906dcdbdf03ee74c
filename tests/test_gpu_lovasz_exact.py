"""The Lovasz-Softmax kernels -- csrc/lovasz.hip: key build, the 4-pass stable radix sort, tile counts and their scan, closed-form weights,
the final sum and the backward -- through the C ABI, against the numpy restatement of tests/exact.py (section "Lovasz-Softmax"; pinned to
tests/lovasz_ref.py and its conditions proved on the CPU in tests/test_exact_bounds.py; no bound comes from what a GPU returned).
tests/test_gpu_lovasz.py judges the loss to 1e-5 and the gradient by a norm over the whole tensor, on at most 4 sort tiles; here every plane
the forward leaves in its workspace is read back and held element by element, up to 258 tiles (the carry loops' second trip).

Harness: the logits between NaN guards; the workspace allocated here, 256-byte aligned, of exactly tss_lovasz_workspace_bytes (asserted
against X.lovasz_plan), every byte 0xFF (NaN as a float or double, DROPPED as a key) with guard bytes behind it that must survive; loss and
n_present NaN with guard floats behind them; the gradient NaN-filled between sentinel guards; a second evaluation into fresh buffers:
the same bits everywhere.
  tier 1  key of every kept (class, pixel) of the last chunk, recovered from the sorted pairs: inside [key(e + A), key(e - A)] of
          X.LovaszRef -- one key wide at >= 99 % of them (CPU-asserted), so bit for bit there; DROPPED exactly at dropped pixels
  tier 2  bit for bit given the kernel's own keys: pay0 a permutation with bit 31 = (label == c) & kept; sorted keys non-decreasing, equal
          keys in ascending pixel order, the plane = numpy's stable argsort; G, n_present; W = (float) of the f64 closed form at the
          payload's pixel, 0.f at dropped pixels and for absent classes; loss = lovasz_final_kernel's tree on the kernel's own partial
          rows.  partial within X.LV_PARTIAL_REL sum |terms| (0.0 for an absent class); the loss within 2^-24 |loss| + the propagated
          partial bound of the f64 loss of those keys, and of X.lovasz_pipeline's where every key is the point key (small cases)
  tier 3  tss_lovasz_bwd, every element against X.lovasz_bwd_ref on the kernel's own W: X.lovasz_bwd_bound; either sign or 0 where the sign
          branch is open (the 'zero' plant alone, CPU-asserted); exact zeros at dropped pixels; grad_out = 0.7, and NULL once
Cases X.LV_CASES; both variants; f32 and bf16 logits (exact in bf16).  The chunked case: W, G, partial and loss bit-identical across
chunk_classes in (0, 4, 1).  Every check prints its worst |out - ref| / bound as `LOVASZ_MARGIN <case> <dtype> <entry> <ratio>` before it
asserts (profiles/lovasz_exact_margins.txt); a bit-for-bit entry prints 0 or inf."""
import numpy as np
import pytest
import torch

from tests import exact as X
from tests.exact_gpu import DEV, N_
from tests.test_gpu_softloss_exact import Planes, guarded, guards_intact

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DT = {'f32': F32, 'bf16': BF}
GUARD_BYTES = 1024
GUARD_BYTE = 0xA5
DROPPED = np.uint32(X.LV_DROPPED)
_refs = {}


def margin_line(case, d, entry, ratio):
    print('LOVASZ_MARGIN %-16s %-5s %-34s %.4f' % (case, d, entry, ratio))


def bitwise(ok):
    return 0.0 if ok else float('inf')


def reference(case, has_ignore):
    """(x, labels, plants, X.LovaszRef), computed once; a large one is dropped when another case comes"""
    key = (case.name, has_ignore)
    if key not in _refs:
        for k in [k for k in _refs if X.LV_BY_NAME[k[0]].N > 100000]:
            del _refs[k]
        x, lab, plants = X.lovasz_operands(case)
        _refs[key] = (x, lab, plants, X.LovaszRef(x, lab, X.LV_IGNORE, has_ignore))
    return _refs[key]


class Workspace:
    """total bytes of 0xFF at a 256-byte aligned address inside a larger allocation, GUARD_BYTES of GUARD_BYTE behind them"""
    def __init__(self, total):
        self.total = total
        self.t = torch.full((total + 256 + GUARD_BYTES,), 0xFF, dtype=torch.uint8, device=DEV)
        self.skip = (-self.t.data_ptr()) % 256
        self.t[self.skip + total:] = GUARD_BYTE
        self.ptr = self.t.data_ptr() + self.skip
        assert self.ptr % 256 == 0

    def read(self):
        h = self.t.cpu().numpy()
        assert (h[self.skip + self.total:] == GUARD_BYTE).all() and (h[:self.skip] == 0xFF).all(), 'written outside the workspace'
        self.h = h[self.skip:self.skip + self.total]
        return self

    def plane(self, off, count, dtype):
        return self.h[off:off + count * np.dtype(dtype).itemsize].copy().view(dtype)


class Forward:
    """one tss_lovasz_fwd into fresh buffers, its planes read back"""
    def __init__(self, case, x, lab, dtype, variant, chunk, has_ignore):
        n = N_()
        B, C, HW, N = case.B, case.C, case.HW, case.N
        self.plan = pl = X.lovasz_plan(N, C, chunk)
        nbytes = n.lib().tss_lovasz_workspace_bytes(N, C, chunk)
        assert nbytes == pl['total'], (case, chunk, 'workspace bytes', nbytes, 'restated', pl['total'])
        self.xb, self.tgt = Planes((B, C, HW), dtype, x), torch.from_numpy(lab).to(DEV).contiguous()
        self.ws, self.loss, self.npres = Workspace(nbytes), guarded(1), guarded(1)
        self.args = (B, C, HW)
        self.code = n.dtype_code(dtype)
        n.call('tss_lovasz_fwd', self.xb.ptr, self.tgt.data_ptr(), self.ws.ptr, self.loss.data_ptr(), self.npres.data_ptr(), B, C, HW,
               X.LV_IGNORE, int(has_ignore), variant, chunk, self.code, n.stream())
        torch.cuda.synchronize()
        ws = self.ws.read()
        loss, npres = self.loss.cpu(), self.npres.cpu()
        assert guards_intact(loss, 1) and guards_intact(npres, 1), (case, 'guard floats written')
        self.loss_bits, self.present = loss[:1].numpy().view(np.uint32)[0], float(npres[0])
        self.loss_value = float(loss[0])
        nlast = C - pl['last_c0']
        self.G = ws.plane(pl['G'], C, np.uint32)
        self.partial = ws.plane(pl['partial'], C * pl['ntiles'], np.float64).reshape(C, pl['ntiles'])
        self.W = ws.plane(pl['W'], C * N, np.float32).reshape(C, N)
        self.key0 = ws.plane(pl['key0'], nlast * N, np.uint32).reshape(nlast, N)
        self.pay0 = ws.plane(pl['pay0'], nlast * N, np.uint32).reshape(nlast, N)
        del ws.h

    def backward(self, dtype, grad_out, chunk):
        n = N_()
        B, C, HW = self.args
        dx = Planes((B, C, HW), dtype)
        go = None if grad_out is None else torch.tensor([grad_out], dtype=F32, device=DEV)
        n.call('tss_lovasz_bwd', self.xb.ptr, self.tgt.data_ptr(), self.ws.ptr, self.npres.data_ptr(), None if go is None else go.data_ptr(),
               dx.ptr, B, C, HW, chunk, self.code, n.stream())
        torch.cuda.synchronize()
        return dx

    def same_bits(self, other):
        pairs = [(self.G, other.G), (self.W.view(np.uint32), other.W.view(np.uint32)), (self.partial.view(np.uint64), other.partial.view(np.uint64))]
        return all(np.array_equal(a, b) for a, b in pairs) and self.loss_bits == other.loss_bits and self.present == other.present


def check_forward(case, d, variant, chunk, has_ignore, ref, fw):
    """tiers 1 and 2 on one forward; returns the worst ratios by entry"""
    C, N = case.C, case.N
    pl, tag = fw.plan, 'v%d c%d i%d ' % (variant, chunk, has_ignore)
    what = (case, d, variant, chunk, has_ignore)
    r = {}
    assert not np.isnan(fw.partial).any() and not np.isnan(fw.W).any() and np.isfinite(fw.loss_value), (what, 'an output left unwritten')
    all_point, ref_total, ref_slack = True, 0.0, 0.0
    for j in range(C - pl['last_c0']):
        c = pl['last_c0'] + j
        ks, pay = fw.key0[j], fw.pay0[j]
        pix, fgbit = (pay & np.uint32(0x7FFFFFFF)).astype(np.int64), (pay >> np.uint32(31)).astype(bool)
        assert pix.max() < N and np.array_equal(np.bincount(pix, minlength=N), np.ones(N, np.int64)), (what, c, 'pay0 is not a permutation')
        assert np.array_equal(fgbit, ref.fg[c][pix]), (what, c, 'bit 31 of pay0 is not (label == c) & kept')
        kbp = np.empty(N, np.uint32)
        kbp[pix] = ks
        # tier 1
        assert (kbp[~ref.kept] == DROPPED).all(), (what, c, 'a dropped pixel without the DROPPED key')
        lo, hi, k = (v[ref.kept].astype(np.float64) for v in (ref.key_lo[c], ref.key_hi[c], kbp))
        r['key'] = max(r.get('key', 0.0), X.worst_ratio(np.abs(k - (lo + hi) / 2), (hi - lo) / 2) if k.size else 0.0)
        all_point = all_point and np.array_equal(kbp, ref.key[c])
        # tier 2: the order
        dk = np.diff(ks.astype(np.int64))
        assert (dk >= 0).all(), (what, c, 'sorted keys decrease at rank', int(np.argmax(dk < 0)))
        tie = (dk == 0) & (np.diff(pix) <= 0)
        assert not tie.any(), (what, c, 'equal keys out of pixel order at rank', int(np.argmax(tie)))
        nkept = int(ref.kept.sum())
        assert (ks[:nkept] != DROPPED).all() and (ks[nkept:] == DROPPED).all(), (what, c, 'dropped pixels are not last')
        assert np.array_equal(pix, np.argsort(kbp, kind='stable')), (what, c, 'pay0 is not the stable argsort of the keys')
        # tier 2: counts, weights, tile sums
        g, G = X.lovasz_weights(fgbit, ks != DROPPED, variant)
        assert int(fw.G[c]) == G == int(ref.G[c]), (what, c, 'G', int(fw.G[c]), G)
        want = np.zeros(N, np.float32)
        want[pix] = g.astype(np.float32)
        bad = np.flatnonzero(fw.W[c].view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (what, c, 'W differs at', bad.size, 'pixels, first', int(bad[0]), float(fw.W[c][bad[0]]), float(want[bad[0]]))
        sums, sabs = X.lovasz_tile_sums(ks, g)
        if G == 0:
            assert (fw.partial[c] == 0).all() and (fw.W[c].view(np.uint32) == 0).all(), (what, c, 'an absent class is not exact zeros')
        r['partial'] = max(r.get('partial', 0.0), X.worst_ratio(np.abs(fw.partial[c] - sums), X.LV_PARTIAL_REL * sabs))
        ref_total, ref_slack = ref_total + float(sums.sum()), ref_slack + float(sabs.sum())
    present = int((fw.G > 0).sum())
    assert fw.present == float(present) == float((ref.G > 0).sum()), (what, 'n_present', fw.present, present)
    loss, pres = X.lovasz_final(fw.partial, fw.G)
    r['loss_tree'] = bitwise(pres == present and loss.view(np.uint32) == fw.loss_bits)
    if present == 0:
        assert fw.loss_bits == 0, (what, 'the loss with no class present is not 0.f')
    if pl['last_c0'] == 0:                   # every class was read back: the f64 loss of the kernel's keys, with its propagated bound
        want = ref_total / present if present else 0.0
        tree = (X.cdiv(pl['ntiles'], X.LV_NT) + 6 + 4 + C + 2) * 2.0 ** -53
        bound = 2.0 ** -24 * abs(want) + (X.LV_PARTIAL_REL + tree) * ref_slack / max(present, 1)
        r['loss_ref'] = X.worst_ratio(abs(fw.loss_value - want), bound)
        if all_point and N <= 8208:
            pipe = X.lovasz_pipeline(None, None, variant, ref=ref)['loss']
            r['loss_pipeline'] = X.worst_ratio(abs(fw.loss_value - pipe), bound)
    for k, v in r.items():
        margin_line(case.name, d, tag + k, v)
    assert all(v <= 1 for v in r.values()), (what, r)
    return r


def check_backward(case, d, variant, chunk, has_ignore, ref, fw, grad_out):
    C, N, B, HW = case.C, case.N, case.B, case.HW
    dtype, what = DT[d], (case, d, variant, chunk, has_ignore, grad_out)
    dx = fw.backward(dtype, grad_out, chunk)
    g = dx.check(what).transpose(1, 0, 2).reshape(C, N)
    assert (g[:, ~ref.kept] == 0).all(), (what, 'the gradient of a dropped pixel is not an exact zero')
    opened = ref.open_sign().any()
    worst = None
    for option in ((-1, 0, 1) if opened else (None,)):
        want, T = X.lovasz_bwd_ref(ref, fw.W, fw.present, grad_out, option)
        bound = X.lovasz_bwd_bound(want, T, C, dtype == BF)
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = (np.abs(g - want) / bound).max(0)              # per pixel: all its classes under ONE choice of the open sign
        worst = ratio if worst is None else np.minimum(worst, ratio)
    r = float(worst.max())
    margin_line(case.name, d, 'v%d c%d i%d bwd%s' % (variant, chunk, has_ignore, '' if grad_out is not None else ' null'), r)
    assert r <= 1, (what, r, 'at pixel', int(np.argmax(worst)))
    return dx


def params():
    return [pytest.param(c, d, v, id='%s-%s-v%d' % (c.name, d, v)) for c in X.LV_CASES for d in ('f32', 'bf16') for v in (0, 1)]


@pytest.mark.parametrize('case,d,variant', params())
def test_lovasz_planes(case, d, variant):
    dtype = DT[d]
    for has_ignore in case.has_ignore:
        x, lab, plants, ref = reference(case, has_ignore)
        first = None
        for chunk in case.chunks:
            fw = Forward(case, x, lab, dtype, variant, chunk, has_ignore)
            check_forward(case, d, variant, chunk, has_ignore, ref, fw)
            dx = check_backward(case, d, variant, chunk, has_ignore, ref, fw, X.LV_GRAD_OUT)
            if first is None:
                first = fw
                if variant == 0:             # a second evaluation into fresh buffers: the same bits
                    fw2 = Forward(case, x, lab, dtype, variant, chunk, has_ignore)
                    dx2 = fw2.backward(dtype, X.LV_GRAD_OUT, chunk)
                    same = fw.same_bits(fw2) and np.array_equal(fw.key0, fw2.key0) and np.array_equal(fw.pay0, fw2.pay0)
                    same = same and torch.equal(X.bits(dx.t.cpu()), X.bits(dx2.t.cpu()))
                    margin_line(case.name, d, 'v%d c%d i%d second evaluation' % (variant, chunk, has_ignore), bitwise(same))
                    assert same, (case, d, 'a second evaluation gives other bits')
                    if case.name == 'one_tile':
                        check_backward(case, d, variant, chunk, has_ignore, ref, fw, None)
            else:                            # W, G, partial and the loss do not depend on how the classes are chunked
                same = first.same_bits(fw)
                margin_line(case.name, d, 'v%d c%d i%d same bits as c%d' % (variant, chunk, has_ignore, case.chunks[0]), bitwise(same))
                assert same, (case, d, chunk, 'chunking changes a bit of W, G, partial or the loss')


@pytest.mark.parametrize('d', ['f32', 'bf16'])
def test_lovasz_nothing_present_gives_exact_zeros(d):
    """every label ignored or out of range: G = 0, n_present = 0, the loss an exact 0.f, W and the gradient exact zeros"""
    case = X.LV_BY_NAME['tile_and_group']
    x, lab, _, _ = reference(case, 1)
    lab = np.where(lab == X.LV_IGNORE, X.LV_IGNORE, -1)
    ref = X.LovaszRef(x, lab, X.LV_IGNORE, 1)
    for variant in (0, 1):
        fw = Forward(case, x, lab, DT[d], variant, 0, 1)
        check_forward(case, d, variant, 0, 1, ref, fw)
        assert fw.present == 0 and fw.loss_bits == 0 and (fw.G == 0).all() and (fw.W.view(np.uint32) == 0).all()
        g = fw.backward(DT[d], X.LV_GRAD_OUT, 0).check((case, d, variant))
        assert (g == 0).all()
