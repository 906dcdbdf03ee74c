"""float64 / integer restatements of the self-training operators (csrc/pseudo.hip, csrc/mix.hip; torch_semantic_segmentation_amd/selftrain.py).

Pseudo-labels, from tests/exact.py's HeadRef (z = the f64 bilinear upsample of the low-resolution logits):
    conf  = exp(max_c z_c - logsumexp_c z_c)          the softmax probability of the arg-max class
    label = arg (lowest index on ties) where conf >= threshold, ignore_index elsewhere
ClassMix's class pick and the mixing select in numpy integers; the select moves BITS (the image is handled as an integer view)."""
import numpy as np
import torch

from tests import msflip_ref


def confidence(ref):
    """[B][H][W] f64 from a HeadRef"""
    return torch.exp(ref.z.max(1).values - ref.lse)


def case_threshold(conf):
    """the threshold of a test case: the f64 median confidence rounded to a multiple of 2^-10 (an f32 number)"""
    return float(torch.round(conf.median() * 1024.0) / 1024.0)


def pseudo_labels(ref, threshold, ignore_index=255):
    """(label int64 [B][H][W], conf f64, kept int64 [B])"""
    conf = confidence(ref)
    keep = conf >= threshold
    label = torch.where(keep, ref.arg, torch.full_like(ref.arg, ignore_index))
    return label, conf, keep.flatten(1).sum(1)


def conf_bound(case, zmax):
    """|conf_f32 - conf_f64| of one pixel: tests/msflip_ref.margin with one map, 'softmax' (conf IS the softmax output of the arg-max class:
    e_arg = exp(0) = 1, so the product e_c * (1 / s) the margin counts is exact here)"""
    return msflip_ref.margin(1, case.C, zmax, [(case.h, case.w)], (case.H, case.W), 'softmax')


def logit_margin(case, zmax):
    return msflip_ref.margin(1, case.C, zmax, [(case.h, case.w)], (case.H, case.W), 'logits')


def decided(case, ref, threshold):
    """(arg_decided, thr_decided) bool [B][H][W]: pixels whose arg-max / keep-drop decision the f32 kernel must reproduce"""
    conf = confidence(ref)
    thr_ok = (conf - threshold).abs() > conf_bound(case, ref.zmax)
    arg_ok = torch.ones_like(thr_ok) if case.exact else ref.gap > logit_margin(case, ref.zmax)
    return arg_ok, thr_ok


def classmix_select(labels, keys, C):
    """labels uint8 [B][...], keys uint32 [B][256] -> sel uint8 [B][256]: the ceil(n / 2) present classes < C of smallest (key, index)"""
    labels = np.asarray(labels, dtype=np.uint8).reshape(len(labels), -1)
    keys = np.asarray(keys, dtype=np.uint32)
    B = labels.shape[0]
    sel = np.zeros((B, 256), dtype=np.uint8)
    for b in range(B):
        present = [int(c) for c in np.unique(labels[b]) if c < C]
        ranked = sorted(present, key=lambda c: (int(keys[b, c]), c))
        for c in ranked[:(len(ranked) + 1) // 2]:
            sel[b, c] = 1
    return sel


def mix_mask(labels, sel=None, boxes=None):
    """bool [B][H][W]: True where sample b keeps its own pixel"""
    labels = np.asarray(labels, dtype=np.uint8)
    B, H, W = labels.shape
    assert (sel is None) != (boxes is None)
    if sel is not None:
        sel = np.asarray(sel, dtype=np.uint8)
        return np.stack([sel[b][labels[b]] != 0 for b in range(B)])
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    return np.stack([(ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1) for (y0, x0, y1, x1) in np.asarray(boxes).tolist()])


def mix_batch(image_bits, labels, partner, sel=None, boxes=None):
    """image_bits: an INTEGER view [B][Ci][H][W] of the image; -> (image_out bits, target int64 [B][H][W])"""
    image_bits, labels = np.asarray(image_bits), np.asarray(labels, dtype=np.uint8)
    assert image_bits.dtype.kind in 'iu'
    partner = np.asarray(partner).astype(np.int64)
    m = mix_mask(labels, sel, boxes)
    img = np.where(m[:, None], image_bits, image_bits[partner])
    tgt = np.where(m, labels, labels[partner]).astype(np.int64)
    return img, tgt


def bits_of(t):
    """integer numpy view of a float32 / bfloat16 tensor"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()
