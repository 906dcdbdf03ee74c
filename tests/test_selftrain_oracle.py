"""tests/selftrain_ref.py on hand-made inputs, and the premises of the GPU cases (tests/test_gpu_pseudo_label.py, tests/test_gpu_mix.py)
asserted on the CPU: no GPU result enters a threshold, a bound or a share here."""
import functools

import numpy as np
import pytest
import torch

from tests import exact as X
from tests import selftrain_ref as R

IGN = 255


# ----------------------------------------------------------------------------------------------------- classmix_select
def keys_of(B, **rows):
    k = np.full((B, 256), 1000, dtype=np.uint32)
    for b, d in rows.items():
        for c, v in d.items():
            k[int(b[1:]), c] = v
    return k


def test_classmix_picks_half_rounded_up_by_key():
    lab = np.array([[3, 3, 7, 9, 11, 200, 255, 1]], dtype=np.uint8)       # classes 1 3 7 9 11 present; 200, 255 are no classes
    keys = keys_of(1, b0={1: 50, 3: 10, 7: 40, 9: 20, 11: 30})
    sel = R.classmix_select(lab, keys, 19)
    assert sel.shape == (1, 256) and sel.dtype == np.uint8
    assert sorted(np.nonzero(sel[0])[0].tolist()) == [3, 9, 11]           # the three smallest keys of five
    assert R.classmix_select(lab[:, :3], keys, 19)[0].nonzero()[0].tolist() == [3]        # two present: one picked
    assert R.classmix_select(lab[:, 2:3], keys, 19)[0].nonzero()[0].tolist() == [7]       # one present: it is picked


def test_classmix_ties_and_unsigned_compare_and_empty():
    lab = np.array([[4, 2, 9, 6]], dtype=np.uint8)
    assert np.nonzero(R.classmix_select(lab, keys_of(1), 19)[0])[0].tolist() == [2, 4]     # equal keys: the lower class index
    top = keys_of(1, b0={2: 0x80000000, 4: 1, 6: 0x7FFFFFFF, 9: 0xFFFFFFFF})
    assert np.nonzero(R.classmix_select(lab, top, 19)[0])[0].tolist() == [4, 6]            # 0x80000000 ranks ABOVE 1 and 0x7fffffff
    onebit = keys_of(1, b0={2: 0x80000005, 4: 0x00000005, 6: 0x80000004, 9: 0x00000004})
    assert np.nonzero(R.classmix_select(lab, onebit, 19)[0])[0].tolist() == [4, 9]
    ign = np.array([[255, 255, 19, 200]], dtype=np.uint8)
    assert not R.classmix_select(ign, keys_of(1), 19).any()                                 # no valid class: an all-zero row
    assert np.nonzero(R.classmix_select(ign, keys_of(1), 66)[0])[0].tolist() == [19]        # 19 is a class of 66
    two = np.array([[1, 2, 3, 4], [255, 255, 255, 255]], dtype=np.uint8)
    s = R.classmix_select(two, keys_of(2), 19)
    assert s[0].sum() == 2 and s[1].sum() == 0


# ----------------------------------------------------------------------------------------------------- mix_batch
def small_batch():
    rng = np.random.default_rng(3)
    img = rng.integers(-2 ** 31, 2 ** 31, (3, 2, 4, 8), dtype=np.int64).astype(np.int32)
    lab = rng.integers(0, 5, (3, 4, 8)).astype(np.uint8)
    lab[0, 0, 0] = 255
    return img, lab, np.array([1, 0, 2])


def test_mix_boxes_edges():
    img, lab, partner = small_batch()
    boxes = np.array([[0, 0, 0, 0], [0, 0, 4, 8], [1, 3, 3, 5]])            # empty, whole image, interior
    out, tgt = R.mix_batch(img, lab, partner, boxes=boxes)
    assert np.array_equal(out[0], img[1]) and np.array_equal(tgt[0], lab[1])                # empty box: all from the partner
    assert np.array_equal(out[1], img[1]) and np.array_equal(tgt[1], lab[1])                # whole image: all its own
    assert np.array_equal(out[2], img[2])                                                   # its own partner: unchanged either way
    m = R.mix_mask(lab, boxes=np.array([[1, 3, 3, 5]] * 3))
    assert m[0].sum() == 4 and m[0, 1, 3] and m[0, 2, 4] and not m[0, 3, 3] and not m[0, 1, 5] and not m[0, 0, 3]   # y1, x1 exclusive
    assert tgt.dtype == np.int64
    m = R.mix_mask(lab, boxes=np.array([[2, 0, 2, 8], [0, 5, 4, 5], [3, 7, 4, 8]]))
    assert m[0].sum() == 0 and m[1].sum() == 0 and m[2].sum() == 1 and m[2, 3, 7]          # y0 == y1, x0 == x1, the last pixel


def test_mix_select_is_on_bits_and_255_stays():
    img, lab, partner = small_batch()
    sel = np.zeros((3, 256), dtype=np.uint8)
    sel[:, [0, 2]] = 1
    out, tgt = R.mix_batch(img, lab, partner, sel=sel)
    own = np.isin(lab, [0, 2])
    assert np.array_equal(out[0][:, own[0]], img[0][:, own[0]]) and np.array_equal(out[0][:, ~own[0]], img[1][:, ~own[0]])
    assert not own[0, 0, 0] and tgt[0, 0, 0] == lab[1, 0, 0]               # an ignore pixel of sample 0 takes the partner's
    lab[1, 0, 0] = 255
    assert R.mix_batch(img, lab, partner, sel=sel)[1][0, 0, 0] == 255      # 255 stays 255 as an int64
    with pytest.raises(AssertionError):
        R.mix_batch(img, lab, partner)
    with pytest.raises(AssertionError):
        R.mix_batch(img, lab, partner, sel=sel, boxes=np.zeros((3, 4), dtype=np.int64))


# ----------------------------------------------------------------------------------------------------- pseudo-labels
def test_pseudo_labels_by_hand():
    x = torch.tensor([[2.0, 0.0, 0.0], [0.0, 0.0, 0.0]]).T.reshape(1, 3, 1, 2).double()     # pixel 0: (2, 0, 0); pixel 1: all equal
    ref = X.HeadRef(x, torch.zeros(1, 1, 2, dtype=torch.int64), weighted=False)
    conf = R.confidence(ref)
    e2 = float(np.exp(2.0))
    assert abs(float(conf[0, 0, 0]) - e2 / (e2 + 2)) < 1e-15 and abs(float(conf[0, 0, 1]) - 1 / 3) < 1e-15
    lab, _, kept = R.pseudo_labels(ref, 0.5)
    assert lab.tolist() == [[[0, IGN]]] and kept.tolist() == [1]
    assert R.pseudo_labels(ref, 0.0)[0].tolist() == [[[0, 0]]]             # a tie: the lowest index
    assert R.pseudo_labels(ref, 1.5)[2].tolist() == [0]


@functools.lru_cache(maxsize=None)
def case_ref(name):
    case = X.HEAD_BY_NAME[name]
    x, labels, _ = X.head_inputs(case)
    return X.HeadRef(x, labels, ignore_index=IGN, weighted=False)


CPU_CASES = [c for c in X.HEAD_REG + X.HEAD_REG_T2 + X.HEAD_WIDE + X.HEAD_WIDE_T2 if c.name not in ('band64', 'c256')]


@pytest.mark.parametrize('case', CPU_CASES, ids=[c.name for c in CPU_CASES])
def test_gpu_case_premises(case):
    """what tests/test_gpu_pseudo_label.py relies on: the threshold is an f32 multiple of 2^-10 inside (0, 1), it keeps between a
    quarter and three quarters of the pixels, the bound is the derived one and small against the spread of the confidences, and the
    pixels the reference alone cannot decide stay under the caps"""
    ref = case_ref(case.name)
    conf = R.confidence(ref)
    thr = R.case_threshold(conf)
    assert 0 < thr < 1 and thr * 1024 == round(thr * 1024) and float(np.float32(thr)) == thr
    share = float((conf >= thr).double().mean())
    assert 0.25 <= share <= 0.75, (case, 'kept share', share)
    bound = R.conf_bound(case, ref.zmax)
    assert 0 < bound <= 2e-5, (case, bound)
    arg_ok, thr_ok = R.decided(case, ref, thr)
    assert 1.0 - float(thr_ok.double().mean()) <= 9.2e-5 + 1e-12, (case, 'threshold-undecided share')
    assert 1.0 - float(arg_ok.double().mean()) <= 0.004, (case, 'arg-max-undecided share')
    assert 1.0 - float((arg_ok & thr_ok).double().mean()) <= 0.01
    assert case.C <= IGN


def test_c256_has_no_label_byte_left():
    """the one case of the head lists the pseudo-label entries refuse: with 256 classes no byte is free for `ignore_index`"""
    assert X.HEAD_BY_NAME['c256'].C == 256 and not any(c.C > 255 for c in CPU_CASES)
