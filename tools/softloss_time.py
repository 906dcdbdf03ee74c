"""Forward + backward time of tssa.FocalLoss and tssa.DiceLoss (csrc/softloss.hip) at the training shape, bf16 and f32 logits,
next to two baselines on the same GPU: (a) the same formula on stock PyTorch (focal: log_softmax gather + pixel weight; Dice:
F.one_hot and boolean-mask indexing), and (b) this package's own cross_entropy forward + backward,
which moves the same bytes as the focal loss.  Prints one JSON line (profiles/softloss_time.json).

    python tools/softloss_time.py [--shape 8 19 1024 2048] [--iters 10] [--rounds 3]

Every candidate is warmed up, then timed with device events over `iters` forward + backward pairs; the candidates are
visited `rounds` times in turn (alternating, so drift hits all of them alike) and the per-round times are all reported.
"""
import argparse
import json
import os
import sys

import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_semantic_segmentation_amd as tssa  # noqa: E402


def _keep(target, num_classes, ignore_index):
    return (target != ignore_index) & (target >= 0) & (target < num_classes)


def stock_focal(x, target, alpha=0.25, gamma=2.0, ignore_index=255):
    """-alpha * mean over the kept pixels of exp((1 - p_t)^gamma) * log p_t: the log-probability of the labelled class
    gathered per pixel, then the pixel weight; elementwise torch ops only, no host read-back."""
    keep = _keep(target, x.shape[1], ignore_index)
    label = torch.where(keep, target, torch.zeros_like(target))
    log_pt = torch.log_softmax(x, dim=1).gather(1, label.unsqueeze(1)).squeeze(1)
    weight = ((1.0 - log_pt.exp()) ** gamma).exp()
    return -alpha * (weight * log_pt * keep).sum() / keep.sum()


def stock_dice(x, target, num_classes, smooth=1.0, ignore_index=255):
    """mean over the classes of 1 - (2 I_c + smooth) / (U_c + smooth) over the kept pixels, with F.one_hot and
    boolean-mask indexing (a host sync), as a user of stock PyTorch would write it."""
    keep = _keep(target, num_classes, ignore_index)
    prob = torch.softmax(x, dim=1).movedim(1, -1)[keep]                  # [kept pixels, C]
    hot = F.one_hot(target[keep], num_classes).to(prob.dtype)
    overlap = (prob * hot).sum(0)
    mass = prob.sum(0) + hot.sum(0)
    return 1.0 - ((2.0 * overlap + smooth) / (mass + smooth)).mean()


def one_round(fn, x, target, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        loss = fn(x, target)
        loss.backward()
        x.grad = None
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters, float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=4, default=[8, 19, 1024, 2048])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--skip-stock', action='store_true')
    a = ap.parse_args()
    B, C, H, W = a.shape
    dev = 'cuda:0'
    torch.manual_seed(0)
    logits = torch.randn(B, C, H, W, device=dev)
    target = torch.randint(0, C, (B, H, W), device=dev)
    target[torch.rand(B, H, W, device=dev) < 0.1] = 255
    focal, dice = tssa.FocalLoss(ignore_index=255), tssa.DiceLoss(C, ignore_index=255)
    inputs = {'bf16': logits.bfloat16().requires_grad_(True), 'f32': logits.clone().requires_grad_(True)}
    cands = []
    for name, x in inputs.items():
        cands.append(('hip_focal_' + name, focal, x))
        cands.append(('hip_dice_' + name, dice, x))
        cands.append(('hip_cross_entropy_' + name, lambda x, t: tssa.cross_entropy(x, t, ignore_index=255), x))
        if not a.skip_stock:
            cands.append(('stock_focal_' + name, stock_focal, x))
            cands.append(('stock_dice_' + name, lambda x, t: stock_dice(x, t, C), x))
    for _name, fn, x in cands:                         # warm-up: code objects, allocator blocks
        one_round(fn, x, target, 2)
    ms = {name: [] for name, _, _ in cands}
    loss = {}
    for _ in range(a.rounds):
        for name, fn, x in cands:
            t, loss[name] = one_round(fn, x, target, a.iters)
            ms[name].append(round(t, 4))
    esz = {'bf16': 2, 'f32': 4}
    out = {'tool': 'tools/softloss_time.py', 'device': torch.cuda.get_device_name(0), 'shape': [B, C, H, W], 'ignore_index': 255,
           'ignored_fraction': 0.1, 'iters': a.iters, 'rounds': a.rounds,
           'what': 'forward + backward of the loss alone, device events around iters pairs, ms per pair for every round'}
    for name, _, _ in cands:
        out[name] = {'ms_rounds': ms[name], 'ms_median': sorted(ms[name])[len(ms[name]) // 2], 'loss': loss[name]}
    for name in inputs:
        ce = out['hip_cross_entropy_' + name]['ms_median']
        out['focal_over_ce_' + name] = round(out['hip_focal_' + name]['ms_median'] / ce, 3)
        out['dice_over_ce_' + name] = round(out['hip_dice_' + name]['ms_median'] / ce, 3)
        # lower-bound traffic model of the focal pair: logits read twice, gradient written once, target read twice (8 B),
        # lse and coefficient written and read once each (4 x 4 B); the rate below is that model over the measured time
        need = B * H * W * (3 * C * esz[name] + 2 * 8 + 4 * 4)
        out['focal_model_GBps_' + name] = round(need / out['hip_focal_' + name]['ms_median'] / 1e6, 1)
        if not a.skip_stock:
            out['stock_over_hip_focal_' + name] = round(out['stock_focal_' + name]['ms_median'] / out['hip_focal_' + name]['ms_median'], 2)
            out['stock_over_hip_dice_' + name] = round(out['stock_dice_' + name]['ms_median'] / out['hip_dice_' + name]['ms_median'], 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
