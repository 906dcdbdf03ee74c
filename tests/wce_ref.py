"""Restatement of the class-weighted, label-smoothed cross-entropy (torch's semantics, the project's validity rule), dtype-generic:
the tests run it in f32 and f64.  tests/test_wce_oracle.py pins it to F.cross_entropy and to a hand-worked case.

C classes, weights w[C] (None: all ones), W = sum_c w_c, eps = label_smoothing, p = softmax(x) over the classes of a pixel.
A pixel is valid iff target != ignore_index (None: no ignore index) and 0 <= target < C; every other pixel does not count
(torch raises on out-of-range labels; here they behave as ignored).

    den  = sum_valid w_t
    loss = [ (1 - eps) sum_valid w_t (lse - x_t) + eps / C sum_valid sum_c w_c (lse - x_c) ] / den          den == 0: nan (also where
                                                                  the valid pixels all have weight 0 and the second sum is positive)
    dloss/dx_c = (s p_c - hot_c) / den on a valid pixel, 0 elsewhere                                       den == 0: 0 everywhere
    s = (1 - eps) w_t + eps W / C,   hot_c = (1 - eps) w_t [c == t] + eps w_c / C
"""
import torch
from torch.nn import functional as F


def valid_mask(target, num_classes, ignore_index):
    m = (target >= 0) & (target < num_classes)
    if ignore_index is not None:
        m = m & (target != ignore_index)
    return m


def _weights(weight, C, like):
    return torch.ones(C, dtype=like.dtype) if weight is None else weight.detach().to(like.dtype)


def wce_loss(input, target, weight=None, ignore_index=-100, label_smoothing=0.0):
    """(B,C,H,W) logits, (B,H,W) int64 labels -> the scalar loss in input's dtype."""
    C = input.shape[1]
    w = _weights(weight, C, input)
    valid = valid_mask(target, C, ignore_index).to(input.dtype)
    t = target.clamp(0, C - 1)
    nlp = -F.log_softmax(input, dim=1)                            # lse - x_c
    wt = w[t] * valid
    hard = (wt * nlp.gather(1, t[:, None])[:, 0]).sum()
    soft = ((nlp * w[None, :, None, None]).sum(1) * valid).sum()
    den = wt.sum()                                                # two quotients, as torch forms them: den == 0 gives nan, never inf
    return (1 - label_smoothing) * (hard / den) + label_smoothing / C * (soft / den)


def wce_grad_closed_form(input, target, weight=None, ignore_index=-100, label_smoothing=0.0):
    C = input.shape[1]
    w = _weights(weight, C, input)
    valid = valid_mask(target, C, ignore_index).to(input.dtype)
    t = target.clamp(0, C - 1)
    wt = w[t] * valid
    den = wt.sum()
    if float(den) == 0:
        return torch.zeros_like(input)
    onehot = F.one_hot(t, C).permute(0, 3, 1, 2).to(input.dtype)
    s = ((1 - label_smoothing) * w[t] + label_smoothing * w.sum() / C) * valid
    hot = ((1 - label_smoothing) * w[t][:, None] * onehot + label_smoothing / C * w[None, :, None, None]) * valid[:, None]
    return (s[:, None] * F.softmax(input, dim=1) - hot) / den


def upsample(low, size):
    return F.interpolate(low, size=size, mode='bilinear', align_corners=True)


def upsampled_wce_loss(low, target, weight=None, ignore_index=-100, label_smoothing=0.0):
    """wce_loss of the low-resolution logits upsampled to the labels' size."""
    return wce_loss(upsample(low, tuple(target.shape[-2:])), target, weight, ignore_index, label_smoothing)


def upsampled_wce_grad_closed_form(low, target, weight=None, ignore_index=-100, label_smoothing=0.0):
    """The closed-form gradient at full resolution, carried to the low-resolution logits by the transpose of the interpolation."""
    x = low.detach().clone().requires_grad_(True)
    up = upsample(x, tuple(target.shape[-2:]))
    up.backward(wce_grad_closed_form(up.detach(), target, weight, ignore_index, label_smoothing))
    return x.grad.detach()


def loss_and_grad(fn, logits, target, dtype, *args, **kwargs):
    """fn = wce_loss or upsampled_wce_loss, run in `dtype`; (loss, gradient by autograd)."""
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    loss = fn(x, target, *args, **kwargs)
    loss.backward()
    return loss.detach(), x.grad.detach()
