"""Restatements of the reference's focal loss (TSS/losses/focal_loss.py:8-15) and of the soft Dice loss its dice_loss.py:8-26
intends, dtype-generic (the tests run them in f32 and f64), plus the closed-form gradients the HIP kernels evaluate.

A pixel is valid iff target != ignore_index (None: no ignore index) and 0 <= target < C.  No valid pixel: 0 * input.sum()
(the HIP path's rule; the reference's focal loss gives nan, its Dice loss cannot run at all).

focal, variant='reference': weight exp(q^gamma), what the reference computes (tests/golden/focal.npz pins the f32 numbers);
       variant='lin': the published weight q^gamma.  q = sum_{c != t} s_c, the reference's 1 - s_t without the cancellation.
dice : the sums I_c, U_c of csrc/softloss.hip's header over the valid pixels, with one_hot and a boolean mask; upstream's
       `target > 0` is read as the range check `target >= 0`.
"""
import torch
from torch.nn import functional as F

FOCAL_VARIANTS = ('reference', 'lin')


def valid_mask(target, num_classes, ignore_index):
    m = (target >= 0) & (target < num_classes)
    if ignore_index is not None:
        m = m & (target != ignore_index)
    return m


def _focal_parts(input, target, ignore_index):
    """valid mask, one-hot of the clamped target [B,C,H,W] (bool), softmax, log p_t, q"""
    C = input.shape[1]
    valid = valid_mask(target, C, ignore_index)
    t = target.clamp(0, C - 1)
    onehot = F.one_hot(t, C).permute(0, 3, 1, 2).bool()
    s = F.softmax(input, dim=1)
    lp = F.log_softmax(input, dim=1).gather(1, t[:, None])[:, 0]
    # value: the sum of the other classes' probabilities (no cancellation as p_t -> 1).  derivative: dq = -dp_t, the same
    # function's, taken through p_t = exp(lp): autograd through the masked sum forms s_c (1 - q) from a rounded q, which
    # cancels as q -> 1 (p_t -> 0) and costs the f32 mode a factor 10 in the gradient (1.7e-6 against the reference's
    # f32 gradient on tests/golden/focal.npz at gamma = 2, 5e-7 this way).  In exact arithmetic nothing changes.
    q = (s * (~onehot).to(s.dtype)).sum(1)
    p = torch.exp(lp)
    q = q.detach() + (p.detach() - p)
    return valid, onehot, s, lp, q


def focal_weight(q, gamma, variant):
    qg = torch.pow(q, gamma)
    if variant == 'reference':
        return torch.exp(qg)
    if variant == 'lin':
        return qg
    raise ValueError(variant)


def focal_loss(input, target, alpha=0.25, gamma=2.0, ignore_index=-100, variant='reference'):
    valid, _onehot, _s, lp, q = _focal_parts(input, target, ignore_index)
    n = int(valid.sum())
    if n == 0:
        return input.sum() * 0
    w = focal_weight(q, gamma, variant)
    return -alpha * (w * lp)[valid].sum() / n


def focal_grad_closed_form(input, target, alpha, gamma, ignore_index, variant):
    """dx_c = A ([c == t] - s_c) alpha / n_valid, A = -(p w' lp + w), w' = -gamma q^(gamma-1) w (lin: -gamma q^(gamma-1)),
    w' = 0 for gamma == 0, the term p w' lp taken as 0 where q == 0."""
    valid, onehot, s, lp, q = _focal_parts(input, target, ignore_index)
    n = int(valid.sum())
    if n == 0:
        return torch.zeros_like(input)
    p = torch.exp(lp)
    w = focal_weight(q, gamma, variant)
    if gamma == 0:
        term = torch.zeros_like(q)
    else:
        safe = torch.where(q > 0, q, torch.ones_like(q))
        wp = -gamma * torch.pow(safe, gamma - 1) * (w if variant == 'reference' else 1.0)
        term = torch.where(q > 0, p * wp * lp, torch.zeros_like(q))
    A = -(term + w) * valid.to(input.dtype)
    return A[:, None] * (onehot.to(input.dtype) - s) * (alpha / n)


def _dice_sums(input, target, num_classes, ignore_index):
    """(number of valid pixels, I_c, U_c): the valid pixels picked with a boolean mask, [t == c] as a one-hot matrix."""
    valid = valid_mask(target, num_classes, ignore_index)
    prob = F.softmax(input, dim=1).movedim(1, -1)[valid]                 # [valid pixels, C]
    hot = F.one_hot(target[valid], num_classes).to(prob.dtype)
    I = (prob * hot).sum(0)
    U = prob.sum(0) + hot.sum(0)
    return int(valid.sum()), I, U


def dice_loss(input, target, num_classes, smooth=1.0, ignore_index=-100):
    n, I, U = _dice_sums(input, target, num_classes, ignore_index)
    if n == 0:
        return input.sum() * 0
    return 1 - ((2 * I + smooth) / (U + smooth)).sum() / num_classes


def dice_grad_closed_form(input, target, num_classes, smooth, ignore_index):
    """a_c = -2 / (C (U_c + smooth)), b_c = (2 I_c + smooth) / (C (U_c + smooth)^2), G_c = a_c [t == c] + b_c,
    dx_k = p_k (G_k - sum_c p_c G_c) on the valid pixels, 0 elsewhere."""
    C = num_classes
    n, I, U = _dice_sums(input, target, C, ignore_index)
    if n == 0:
        return torch.zeros_like(input)
    a = -2.0 / (C * (U + smooth))
    b = (2.0 * I + smooth) / (C * (U + smooth) ** 2)
    valid = valid_mask(target, C, ignore_index)
    onehot = F.one_hot(target.clamp(0, C - 1), C).permute(0, 3, 1, 2).to(input.dtype)
    p = F.softmax(input, dim=1)
    G = a[None, :, None, None] * onehot + b[None, :, None, None]
    dot = (p * G).sum(1, keepdim=True)
    return p * (G - dot) * valid[:, None].to(input.dtype)


def loss_and_grad(fn, logits, target, dtype, *args, **kwargs):
    """fn = focal_loss or dice_loss, run in `dtype`; (loss, gradient by autograd)."""
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    loss = fn(x, target, *args, **kwargs)
    loss.backward()
    return loss.detach(), x.grad.detach()
