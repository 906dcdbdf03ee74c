"""Restatement of the reference's Lovasz-Softmax loss (TSS/losses/lovasz_softmax_loss.py:7-45), dtype-generic.

The reference cannot run in f64 (hard `.float()` calls); this can, and in f32 with variant='reference' it performs
the reference's operations in the reference's order (tests/golden/lovasz.npz pins that: the f32 loss bit for bit).

variant='reference': lovasz_grad as the reference runs it, jaccard[1:] -= jaccard[0:1]   (g_r = J_r - J_0)
variant='berman'   : the published successive difference,   jaccard[1:] -= jaccard[:-1] (g_r = J_r - J_{r-1})
stable=True orders equal errors by ascending pixel index (the HIP path's tie rule); False leaves ties to torch.argsort,
as the reference does.
"""
import torch
from torch.nn import functional as F

VARIANTS = ('reference', 'berman')


def lovasz_weights(gt_sorted, variant='reference'):
    """lovasz_grad (:7-17) in gt_sorted's dtype: cumsum form."""
    p = len(gt_sorted)
    gts = torch.sum(gt_sorted)
    intersection = gts - gt_sorted.cumsum(0)
    union = gts + (1. - gt_sorted).cumsum(0)
    jaccard = 1. - (intersection / union)
    if p > 1:
        if variant == 'reference':
            jaccard[1:p] = jaccard[1:p] - jaccard[0:1]
        elif variant == 'berman':
            jaccard[1:p] = jaccard[1:p] - jaccard[0:p - 1].clone()
        else:
            raise ValueError(variant)
    return jaccard


def closed_form_weights(gt_sorted, variant='reference'):
    """g_r from integers, in f64: I = G - F_r, U = G + (r+1) - F_r, J_r = (r+1)/U.
    berman: 1/U at a foreground rank, I/(U(U-1)) at a background rank; reference: J_0, then ((r+1) U_0 - U)/(U U_0)."""
    fg = gt_sorted.to(torch.int64)
    n = fg.numel()
    G = int(fg.sum())
    Fr = fg.cumsum(0)
    r1 = torch.arange(1, n + 1, dtype=torch.int64)
    I, U = G - Fr, G + r1 - Fr
    if variant == 'berman':
        g = torch.where(fg.bool(), 1.0 / U.double(), I.double() / (U.double() * (U - 1).double().clamp_min(1.0)))
    elif variant == 'reference':
        U0 = int(U[0])
        g = (r1 * U0 - U).double() / (U.double() * float(U0))
        g[0] = 1.0 / U0
    else:
        raise ValueError(variant)
    return g


def class_errors(input, target, num_classes, ignore_index=None):
    """[(class, errors, fg)] for every present class, in flat pixel order of the kept pixels (:21-39)."""
    p = F.softmax(input, dim=1)
    p = p.permute(0, 2, 3, 1).flatten(0, 2)
    target = target.flatten()
    if ignore_index is not None:
        mask = target != ignore_index
        p = p[mask]
        target = target[mask]
    out = []
    for c in range(num_classes):
        fg = (target == c).to(p.dtype)
        if fg.sum() == 0:
            continue
        out.append((c, (fg - p[:, c]).abs(), fg))
    return out


def lovasz_softmax_loss(input, target, num_classes, ignore_index=None, variant='reference', stable=False):
    """The loss in input's dtype (f32 or f64); differentiable.  No class present -> 0 * input.sum() (the HIP path's rule;
    the reference raises)."""
    losses = []
    for _c, errors, fg in class_errors(input, target, num_classes, ignore_index):
        if stable:
            indices = torch.sort(errors.detach(), dim=0, descending=True, stable=True)[1]
        else:
            indices = torch.argsort(errors, dim=0, descending=True)
        errors = errors[indices]
        fg = fg[indices]
        losses.append(torch.dot(errors, lovasz_weights(fg, variant)))
    if not losses:
        return input.sum() * 0
    return torch.stack(losses).mean()


def loss_and_grad(logits, target, num_classes, ignore_index, variant, dtype, stable=False):
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    loss = lovasz_softmax_loss(x, target, num_classes, ignore_index, variant, stable)
    loss.backward()
    return loss.detach(), x.grad.detach()


def tie_free(logits, target, num_classes, ignore_index):
    """True when, in f64, no class has two kept pixels with the same error."""
    for _c, errors, _fg in class_errors(logits.detach().double(), target, num_classes, ignore_index):
        if torch.unique(errors).numel() != errors.numel():
            return False
    return True
