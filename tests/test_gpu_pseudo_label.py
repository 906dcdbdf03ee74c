"""tss_upsample_pseudo_label / tss_upsample_pseudo_label_wide (csrc/pseudo.hip) through the C ABI, on the cases of the fused head
(X.HEAD_REG + X.HEAD_REG_T2 + X.HEAD_WIDE + X.HEAD_WIDE_T2, both dtypes of each) against the f64 restatement tests/selftrain_ref.py.
Harness of tests/exact_gpu.py: `low` at its pitch with NaN pad channels and NaN spare rows; the label map filled with a byte that is
neither a class nor the ignore byte, the confidence map with NaN, both with sentinel spare rows that must stay untouched.

Per case, at the threshold thr = the f64 median confidence rounded to a multiple of 2^-10 (kept share asserted in [0.25, 0.75]):
  conf    every pixel within tests/msflip_ref.margin(1, C, zmax, [(h, w)], (H, W), 'softmax') of the f64 value (derived, 3e-6 .. 2e-5)
  label   arg-max at every pixel (exact cases) or at every pixel whose top-2 gap exceeds the 'logits' margin (tier 2); the keep / drop
          decision at every pixel with |conf - thr| above the bound; the pixels left out for either reason: a share of at most 0.01
  kept    accumulated into a non-zero start value: exactly the kept labels of the returned map, per sample
  thr = 0   the label map is the pred of tss_upsample_argmax_confusion[_wide] bit for bit and kept = H W
  thr = 1.5 every byte is ignore_index and kept = 0
  a second call gives the same bits; conf = NULL and kept = NULL give the same labels.
band32 / band64 run the label checks only (no confidence map).  c256 has no byte left for ignore_index: the entry refuses it, as it
refuses C = 25 at the register entry and ignore_index < C.  Every check prints its largest ratio as a PSEUDO_MARGIN line before it
asserts (profiles/selftrain_margins.txt)."""
import pytest
import torch

from tests import exact as X
from tests import selftrain_ref as R
from tests.exact_gpu import DEV, SPARE, Buf, N_, to_rows

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DT = {'f32': F32, 'bf16': BF}
IGN = 255
FILL = 0xA5                                                 # 165: no class of any case (C <= 130), not the ignore byte
BIG = ('band32', 'band64')
ERR_SHAPE = -2
CASES = X.HEAD_REG + X.HEAD_REG_T2 + X.HEAD_WIDE + X.HEAD_WIDE_T2
RUN = [c for c in CASES if c.C <= 255]
REFUSED_C = [c for c in CASES if c.C > 255]

_refs = {}


def reference(case):
    """(x, HeadRef, conf f64, thr) of a case, computed once; of the two large cases only the latest is kept"""
    if case.name not in _refs:
        for k in [k for k in _refs if k in BIG]:
            del _refs[k]
        x, labels, _ = X.head_inputs(case)
        ref = X.HeadRef(x, labels, ignore_index=IGN, weighted=False)
        conf = R.confidence(ref)
        _refs[case.name] = (x, ref, conf, R.case_threshold(conf))
    return _refs[case.name]


def params(cases):
    return [pytest.param(c, d, id='%s-%s' % (c.name, d)) for c in cases for d in c.dtypes]


def margin_line(case, d, what, value, extra=''):
    print('PSEUDO_MARGIN %-14s %-5s %-28s %.6f %s' % (case.name, d, what, value, extra))


class Low:
    """the low-resolution logits of a case on the device: [B h w + SPARE][ldl], NaN pad channels, NaN spare rows"""
    def __init__(self, case, x, dtype):
        self.buf = Buf(case.B * case.h * case.w, case.C, case.ldl, 0, to_rows(x), dtype, nan_spare=True, nan_pad=True)
        assert torch.equal(self.buf.rows(), to_rows(x)), 'logits not exact in the dtype'
        self.ptr, self.ld = self.buf.ptr, case.ldl


class Out:
    """label map (FILL bytes), confidence map (NaN) and kept counters (start values 1000 + 7 b), each with guard elements behind"""
    def __init__(self, case, want_conf=True, want_kept=True):
        self.n = case.B * case.H * case.W
        self.case = case
        self.label = torch.full((self.n + 64,), FILL, dtype=torch.uint8, device=DEV)
        self.conf = None
        if want_conf:
            c = torch.full((self.n + 64,), float('nan'), dtype=F32)
            c[self.n:] = 7.25
            self.conf = c.to(DEV)
        self.kept0 = 1000 + 7 * torch.arange(case.B + 2, dtype=torch.int64)
        self.kept = self.kept0.clone().to(DEV) if want_kept else None

    def read(self, what):
        c = self.case
        lab = self.label.cpu()
        assert (lab[self.n:] == FILL).all(), (what, 'bytes behind the label map written')
        lab = lab[:self.n].reshape(c.B, c.H, c.W)
        conf = kept = None
        if self.conf is not None:
            cf = self.conf.cpu()
            assert (cf[self.n:] == 7.25).all(), (what, 'floats behind the confidence map written')
            conf = cf[:self.n].reshape(c.B, c.H, c.W)
        if self.kept is not None:
            k = self.kept.cpu()
            assert torch.equal(k[c.B:], self.kept0[c.B:]), (what, 'counters behind kept written')
            kept = (k - self.kept0)[:c.B]
        return lab, conf, kept


def entry_of(case):
    return 'tss_upsample_pseudo_label' + ('_wide' if case.wide else '')


def run(case, dtype, low, thr, out):
    n = N_()
    t = torch.tensor([thr], dtype=F32, device=DEV)
    n.call(entry_of(case), low.ptr, low.ld, t.data_ptr(), out.label.data_ptr(), n.ptr(out.conf), n.ptr(out.kept), case.B, case.C, case.h,
           case.w, case.H, case.W, IGN, n.dtype_code(dtype), n.stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize('case,d', params(RUN))
def test_pseudo_label(case, d):
    n, dtype = N_(), DT[d]
    x, ref, conf_ref, thr = reference(case)
    big = case.name in BIG
    low = Low(case, x, dtype)
    HW = case.H * case.W
    share = float((conf_ref >= thr).double().mean())
    margin_line(case, d, 'kept share', share, 'thr %.10f' % thr)
    assert 0.25 <= share <= 0.75, (case, 'kept share of the reference', share)

    out = Out(case, want_conf=not big)
    run(case, dtype, low, thr, out)
    lab, conf, kept = out.read('median threshold')
    lab = lab.long()
    assert not (lab == FILL).any(), 'a label was not written'

    # confidence: every pixel, the derived bound
    bound = R.conf_bound(case, ref.zmax)
    if conf is not None:
        assert not torch.isnan(conf).any(), 'a confidence was not written'
        err = (conf.double() - conf_ref).abs()
        margin_line(case, d, 'conf err / bound', float(err.max()) / bound, 'bound %.3e' % bound)
        assert float(err.max()) <= bound, (entry_of(case), case, d, 'conf', float(err.max()), bound)
        # the label is the thresholded confidence the kernel itself returned
        kept_px = lab != IGN
        assert torch.equal(kept_px, conf >= float(torch.tensor(thr, dtype=F32))), 'label and confidence disagree about the threshold'

    # labels: arg-max and keep / drop wherever the reference decides them
    arg_ok, thr_ok = R.decided(case, ref, thr)
    und_arg, und_thr = 1.0 - float(arg_ok.double().mean()), 1.0 - float(thr_ok.double().mean())
    und = 1.0 - float((arg_ok & thr_ok).double().mean())
    margin_line(case, d, 'undecided share / 0.01', und / 0.01, 'arg %.6f thr %.6f' % (und_arg, und_thr))
    assert und <= 0.01, (case, 'undecided share', und)
    keep_ref = conf_ref >= thr
    bad = ((lab != IGN) != keep_ref) & thr_ok
    assert not bad.any(), (entry_of(case), case, d, 'keep / drop differs at', bad.nonzero()[:3].tolist(), int(bad.sum()), 'decided pixels')
    bad = (lab != ref.arg) & (lab != IGN) & arg_ok
    assert not bad.any(), (entry_of(case), case, d, 'arg-max differs at', bad.nonzero()[:3].tolist(), int(bad.sum()), 'decided pixels')

    # kept: exactly the kept labels of the returned map, on top of the start values
    assert torch.equal(kept, (lab != IGN).flatten(1).sum(1)), (case, 'kept', kept.tolist())

    # a second call: the same bits; without conf and kept: the same labels
    out2 = Out(case, want_conf=not big)
    run(case, dtype, low, thr, out2)
    lab2, conf2, kept2 = out2.read('second call')
    assert torch.equal(lab2.long(), lab) and torch.equal(kept2, kept), (case, 'not deterministic')
    if conf is not None:
        assert torch.equal(X.bits(conf2), X.bits(conf)), (case, 'confidence not deterministic')
    out3 = Out(case, want_conf=False, want_kept=False)
    run(case, dtype, low, thr, out3)
    assert torch.equal(out3.read('labels only')[0].long(), lab), (case, 'labels differ without conf / kept')


@pytest.mark.parametrize('case,d', params(RUN))
def test_threshold_zero_is_the_argmax_entry_and_above_one_keeps_nothing(case, d):
    n, dtype = N_(), DT[d]
    x, ref, _, _ = reference(case)
    low = Low(case, x, dtype)
    HW = case.H * case.W
    pred = torch.full((case.B, case.H, case.W), FILL, dtype=torch.uint8, device=DEV)
    n.call('tss_upsample_argmax_confusion' + ('_wide' if case.wide else ''), low.ptr, low.ld, None, pred.data_ptr(), None, case.B, case.C,
           case.h, case.w, case.H, case.W, IGN, n.dtype_code(dtype), n.stream())
    out = Out(case, want_conf=False)
    run(case, dtype, low, 0.0, out)
    lab, _, kept = out.read('threshold 0')
    diff = int((lab != pred.cpu()).sum())
    margin_line(case, d, 'thr 0: bytes off pred', float(diff))
    assert diff == 0, (entry_of(case), case, d, 'threshold 0: differs from the arg-max entry at', diff, 'pixels')
    assert kept.tolist() == [HW] * case.B, (case, 'threshold 0: kept', kept.tolist())
    out = Out(case, want_conf=False)
    run(case, dtype, low, 1.5, out)
    lab, _, kept = out.read('threshold 1.5')
    assert (lab == IGN).all() and kept.tolist() == [0] * case.B, (case, 'a threshold above 1 kept something')


def test_refused_shapes():
    n = N_()
    lib = n.lib()
    low = torch.zeros(4 * 4 * 256, dtype=F32, device=DEV)
    lab = torch.full((64,), FILL, dtype=torch.uint8, device=DEV)
    thr = torch.zeros(1, dtype=F32, device=DEV)
    st = n.stream()

    def rc(entry, C, ldl, ign, h=2, w=2, H=4, W=8):
        return getattr(lib, entry)(low.data_ptr(), ldl, thr.data_ptr(), lab.data_ptr(), None, None, 1, C, h, w, H, W, ign, 0, st)

    assert rc('tss_upsample_pseudo_label', 25, 32, 255) == ERR_SHAPE              # past the register cap
    assert rc('tss_upsample_pseudo_label', 19, 24, 18) == ERR_SHAPE               # ignore_index collides with a class
    assert rc('tss_upsample_pseudo_label_wide', 66, 72, 65) == ERR_SHAPE
    assert rc('tss_upsample_pseudo_label', 19, 24, 256) == ERR_SHAPE              # not a byte
    assert rc('tss_upsample_pseudo_label_wide', 256, 256, 255) == ERR_SHAPE       # no byte left for ignore_index
    assert rc('tss_upsample_pseudo_label_wide', 256, 256, 256) == ERR_SHAPE
    assert rc('tss_upsample_pseudo_label', 19, 24, 255, h=5) == ERR_SHAPE         # an output smaller than the map
    for case in REFUSED_C:                                                        # c256 of the head's case list
        assert rc('tss_upsample_pseudo_label_wide', case.C, case.ldl, IGN, case.h, case.w, case.H, case.W) == ERR_SHAPE
    torch.cuda.synchronize()
    assert (lab.cpu() == FILL).all(), 'a refused call wrote labels'
    assert rc('tss_upsample_pseudo_label', 19, 24, 19) == 0 and rc('tss_upsample_pseudo_label_wide', 255, 256, 255) == 0     # the edges that are inside
    torch.cuda.synchronize()


def test_public_op():
    """tssa.upsample_pseudo_labels: dispatch by class count, the cached threshold scalar and a device one, kept zero-filled or accumulated,
    the ValueErrors"""
    import torch_semantic_segmentation_amd as tssa
    for name in ('cp24', 'c33'):
        case = X.HEAD_BY_NAME[name]
        x, ref, conf_ref, thr = reference(case)
        low = x.float().to(DEV)
        lab, conf, kept = tssa.upsample_pseudo_labels(low, thr, size=(case.H, case.W), want_confidence=True)
        assert lab.dtype == torch.uint8 and conf.dtype == F32 and kept.dtype == torch.int64 and tuple(kept.shape) == (case.B,)
        assert float((conf.cpu().double() - conf_ref).abs().max()) <= R.conf_bound(case, ref.zmax)
        assert torch.equal(kept.cpu(), (lab.cpu() != IGN).flatten(1).sum(1))
        lab2, none, kept2 = tssa.upsample_pseudo_labels(low, torch.tensor([thr], dtype=F32, device=DEV), size=(case.H, case.W), kept=kept)
        assert none is None and kept2 is kept and torch.equal(lab2, lab) and torch.equal(kept.cpu(), 2 * (lab.cpu() != IGN).flatten(1).sum(1))
        with pytest.raises(ValueError):
            tssa.upsample_pseudo_labels(low, thr, size=(case.H, case.W), ignore_index=case.C - 1)
        with pytest.raises(ValueError):
            tssa.upsample_pseudo_labels(low, thr, size=(case.h - 1, case.W))
    with pytest.raises(ValueError):
        tssa.upsample_pseudo_labels(torch.zeros(1, 256, 2, 2, device=DEV), 0.5, scale_factor=2)
