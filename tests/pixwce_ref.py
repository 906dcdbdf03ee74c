"""Host reference (torch float64 / numpy) of per-pixel loss weights on the fused head (csrc/pixwce.hip, ops.upsample_pixel_weighted_cross_entropy's
pixel_weight / pixel_norm):

    loss = sum_valid k_i ce_i / D,    k_i = omega_i w_{t_i},    numerator = sum of F.cross_entropy(F.interpolate(low.double(), size,
    bilinear, align_corners=True), t, weight, reduction='none') * omega     (torch's 'none' already carries w_t)

    D = sum_valid k_i ('weight'),  sum_valid w_{t_i} ('valid'),  B H W with the ignored pixels ('pixels').

A label outside [0, C) counts as ignored, as in the kernels.  With sample groups the rules of tests/groupce_ref.py hold with n_b := D_b
(for 'pixels': H W per sample): L = sum_g (sum_{b in g} lambda_b S_b) / N_g, N_g = sum_{b in g} D_b, N_g = 0 -> L_g = 0 and a zero
gradient; without groups all samples form one group of weight 1.  Pinned against hand-worked cases in tests/test_pixwce_ref.py."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import groupce_ref

NORMS = ('weight', 'valid', 'pixels')


def sample_sums(low, target, omega, size, ignore_index=255, weight=None, norm='weight'):
    """(S [B], D [B]) in float64: S_b = sum_valid k ce (differentiable in `low`), D_b the sample's part of the denominator"""
    assert norm in NORMS
    B, C = low.shape[:2]
    z = F.interpolate(low.double(), size=tuple(size), mode='bilinear', align_corners=True)
    t = groupce_ref._clean(target, C, ignore_index)
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.double()
    ce = F.cross_entropy(z, t, weight=w, ignore_index=ignore_index, reduction='none')       # w_t ce, 0 where ignored
    valid = (t != ignore_index).double()
    om = omega.double()
    # an ignored pixel's omega is never looked at (a nan there stays there)
    S = torch.where(valid > 0, ce * om, torch.zeros_like(ce)).reshape(B, -1).sum(1)
    wt = w[t.clamp(0, C - 1)] * valid
    if norm == 'weight':
        D = torch.where(valid > 0, om * wt, torch.zeros_like(wt)).reshape(B, -1).sum(1)
    elif norm == 'valid':
        D = wt.reshape(B, -1).sum(1)
    else:
        D = torch.full((B,), float(size[0] * size[1]), dtype=torch.float64)
    return S, D


def pixel_weighted_ce(low, target, omega, size=None, ignore_index=255, class_weight=None, norm='weight', group=None, weight=None,
                      grad_out=1.0):
    """dict(loss, group_loss [B], scale [B], grad [B,C,h,w], S, n): as groupce_ref.grouped_ce, with n = D per sample; group=None is one
    group (id 0) of weight 1"""
    low = low.double().detach().requires_grad_(True)
    B = low.shape[0]
    group = [0] * B if group is None else [int(g) for g in group]
    lam = torch.ones(B, dtype=torch.float64) if weight is None else torch.as_tensor(np.asarray(weight, dtype=np.float64))
    assert len(group) == B and lam.shape == (B,) and all(0 <= g < B for g in group)
    S, n = sample_sums(low, target, omega, size if size is not None else target.shape[-2:], ignore_index, class_weight, norm)
    group_loss, scale = [torch.zeros((), dtype=torch.float64) for _ in range(B)], torch.zeros(B, dtype=torch.float64)
    for g in sorted(set(group)):
        members = [b for b in range(B) if group[b] == g]
        N = sum(float(n[b]) for b in members)
        if N > 0:
            group_loss[g] = sum(lam[b] * S[b] for b in members) / N
            for b in members:
                scale[b] = lam[b] / N
    loss = sum(group_loss)
    grad = torch.zeros_like(low)
    if torch.is_tensor(loss) and loss.requires_grad:
        grad, = torch.autograd.grad(loss * grad_out, low)
    return dict(loss=float(loss.detach()) if torch.is_tensor(loss) else float(loss), group_loss=torch.stack([g.detach() for g in group_loss]),
                scale=scale, grad=grad.detach(), S=S.detach(), n=n)


def head_ref(x, labels, omega, class_weight=None, norm='weight', ignore_index=255, grad_out=1.0, den=None):
    """exact.HeadRef of the pixel-weighted loss: s = omega w_t, hot = s onehot, den = D (the batch's, or `den` when the samples of `x`
    share a group with others), so that exact.head_slack, head_loss_bound and head_grad_bound apply as they stand"""
    from tests import exact as X
    ref = X.HeadRef(x, labels, ignore_index=ignore_index, weighted=False)
    C = ref.C
    wv = torch.ones(C, dtype=torch.float64) if class_weight is None else class_weight.double()
    v = ref.valid.double()
    wt = wv[ref.t] * v
    s = torch.where(ref.valid, omega.double() * wt, torch.zeros_like(wt))
    if den is None:
        den = {'weight': float(s.sum()), 'valid': float(wt.sum()), 'pixels': float(v.numel())}[norm]
    onehot = torch.zeros_like(ref.z).scatter_(1, ref.t[:, None], 1.0)
    hot = s[:, None] * onehot
    ref.den = den
    ref.ssum = float(s.sum())
    ref.sabs = float(s.abs().sum())
    ref.S = float((s.abs() * ref.lse.abs() + (hot.abs() * ref.zabs).sum(1)).sum())
    ref.spix = float((s.abs() * ref.pix).sum())
    ref.loss = float((s * ref.lse - (hot * ref.z).sum(1)).sum()) / den if den > 0 else 0.0
    ref.gs = grad_out / den if den > 0 else 0.0
    p = torch.softmax(ref.z, 1) * s[:, None]
    ref.T = p.abs() + hot.abs()
    ref.g = ref.gs * torch.einsum('oh,bcop,pw->bchw', ref.My, p - hot, ref.Mx)
    ref.A = abs(ref.gs) * torch.einsum('oh,bcop,pw->bchw', ref.My, ref.T, ref.Mx)
    return ref


def mix_plane(plane_bits, labels, partner, sel=None, boxes=None):
    """tss_mix_plane restated on an INTEGER view [B][H][W] of the plane: out[b] = mask ? plane[b] : plane[partner[b]], the mask of
    tests/selftrain_ref.mix_mask (sel[b][labels[b]] or the box)"""
    from tests import selftrain_ref
    plane_bits = np.asarray(plane_bits)
    assert plane_bits.dtype.kind in 'iu'
    partner = np.asarray(partner).astype(np.int64)
    m = selftrain_ref.mix_mask(labels, sel, boxes)
    return np.where(m, plane_bits, plane_bits[partner])
