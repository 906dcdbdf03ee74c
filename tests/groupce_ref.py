"""Host reference (torch float64 / numpy) of per-sample loss groups on the fused head (csrc/groupce.hip, ops.upsample_cross_entropy's
sample_group / sample_weight):

    loss = sum_g L_g,   L_g = (sum_{b in g} lambda_b CE_sum(b)) / N_g,   N_g = sum_{b in g} n_b

with CE_sum(b) = F.cross_entropy(F.interpolate(low[b].double(), size, bilinear, align_corners=True), target[b], weight, reduction='sum',
label_smoothing) and n_b = the sum of the class weights of sample b's valid pixels (their number without class weights): what
reduction='mean' divides by.  A label outside [0, C) counts as ignored, as in the kernels.  An empty group (N_g = 0) gives L_g = 0 and
a zero gradient.  Everything here is pinned against hand-worked cases in tests/test_groupce_ref.py."""
import numpy as np
import torch
import torch.nn.functional as F


def _clean(target, C, ignore_index):
    return torch.where((target >= 0) & (target < C) & (target != ignore_index), target, torch.full_like(target, ignore_index))


def sample_sums(low, target, size, ignore_index=255, weight=None, label_smoothing=0.0):
    """(S [B], n [B]) in float64; S differentiable in `low`"""
    B, C = low.shape[:2]
    z = F.interpolate(low.double(), size=tuple(size), mode='bilinear', align_corners=True)
    t = _clean(target, C, ignore_index)
    w = None if weight is None else weight.double()
    S = torch.stack([F.cross_entropy(z[b:b + 1], t[b:b + 1], weight=w, ignore_index=ignore_index, reduction='sum',
                                     label_smoothing=label_smoothing) for b in range(B)])
    valid = t != ignore_index
    per_pixel = (torch.ones(C, dtype=torch.float64) if w is None else w)[t.clamp(0, C - 1)] * valid
    return S, per_pixel.reshape(B, -1).sum(1)


def grouped_ce(low, target, group, weight=None, size=None, ignore_index=255, class_weight=None, label_smoothing=0.0, grad_out=1.0):
    """dict(loss, group_loss [B], scale [B], grad [B,C,h,w], S, n): the grouped loss, the term of every group id in [0, B) (0 for an id
    no sample uses), lambda_b / N_g(b) per sample (0 for an empty group) and grad_out * d loss / d low, all float64"""
    low = low.double().detach().requires_grad_(True)
    B = low.shape[0]
    group = [int(g) for g in group]
    lam = torch.ones(B, dtype=torch.float64) if weight is None else torch.as_tensor(np.asarray(weight, dtype=np.float64))
    assert len(group) == B and lam.shape == (B,) and all(0 <= g < B for g in group)
    S, n = sample_sums(low, target, size if size is not None else target.shape[-2:], ignore_index, class_weight, label_smoothing)
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
    if loss.requires_grad:
        grad, = torch.autograd.grad(loss * grad_out, low)
    return dict(loss=float(loss.detach()) if torch.is_tensor(loss) else float(loss), group_loss=torch.stack([g.detach() for g in group_loss]), scale=scale, grad=grad.detach(),
                S=S.detach(), n=n)


def selftrain_weights(kept, n_pixels, lam, mode):
    """tss_selftrain_weights restated: (group int32 [2B], weight float32 [2B]).  Labelled half: group 0, weight 1; unlabelled half:
    group 1, weight lam (mode 0) or lam * sum(kept) / (B * n_pixels) (mode 1: an integer sum, the expression in float64 from the
    float32 lam, rounded once to float32)"""
    B = len(kept)
    lam32 = np.float32(lam)
    u = lam32
    if mode == 1:
        total = int(sum(int(k) for k in kept))
        u = np.float32(np.float64(lam32) * np.float64(total) / (np.float64(B) * np.float64(n_pixels)))
    group = np.array([0] * B + [1] * B, dtype=np.int32)
    weight = np.array([1.0] * B + [u] * B, dtype=np.float32)
    return group, weight
