"""Forward + backward time of tssa.LovaszSoftmaxLoss (csrc/lovasz.hip) at the training shape, bf16 and f32 logits, next to
the reference's formula (TSS/losses/lovasz_softmax_loss.py:7-45, restated below: C argsorts, cumsums, a host sync per
class) on stock PyTorch on the same GPU.  Prints one JSON line (profiles/lovasz_time.json).

    python tools/lovasz_time.py [--shape 8 19 1024 2048] [--iters 5]
"""
import argparse
import json
import os
import sys
import time

import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_semantic_segmentation_amd as tssa  # noqa: E402


def stock_lovasz(input, target, num_classes, ignore_index, variant):
    p = F.softmax(input, dim=1).permute(0, 2, 3, 1).flatten(0, 2)
    target = target.flatten()
    if ignore_index is not None:
        mask = target != ignore_index
        p, target = p[mask], target[mask]
    losses = []
    for c in range(num_classes):
        fg = (target == c).float()
        if fg.sum() == 0:
            continue
        errors = (fg - p[:, c]).abs()
        order = torch.argsort(errors, dim=0, descending=True)
        errors, fg = errors[order], fg[order]
        gts = fg.sum()
        jaccard = 1. - (gts - fg.cumsum(0)) / (gts + (1. - fg).cumsum(0))
        if len(fg) > 1:
            jaccard[1:] = jaccard[1:] - (jaccard[0:1] if variant == 'reference' else jaccard[:-1].clone())
        losses.append(torch.dot(errors, jaccard))
    return torch.stack(losses).mean()


def timed(fn, x, target, iters):
    x = x.clone().requires_grad_(True)
    for _ in range(2):
        fn(x, target).backward()
        x.grad = None
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t = time.perf_counter()
        loss = fn(x, target)
        loss.backward()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
        x.grad = None
    return {'ms_median': sorted(times)[len(times) // 2], 'ms_min': min(times), 'loss': float(loss)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=4, default=[8, 19, 1024, 2048])
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--skip-stock', action='store_true')
    a = ap.parse_args()
    B, C, H, W = a.shape
    dev = 'cuda:0'
    torch.manual_seed(0)
    logits = torch.randn(B, C, H, W, device=dev)
    target = torch.randint(0, C, (B, H, W), device=dev)
    target[torch.rand(B, H, W, device=dev) < 0.1] = 255
    out = {'tool': 'tools/lovasz_time.py', 'device': torch.cuda.get_device_name(0), 'shape': [B, C, H, W], 'ignore_index': 255,
           'ignored_fraction': 0.1, 'iters': a.iters, 'what': 'forward + backward of the loss alone, host wall clock around a sync',
           'workspace_GiB': round(tssa.ops.N.lib().tss_lovasz_workspace_bytes(B * H * W, C, 0) / 2 ** 30, 3)}
    for variant in ('reference', 'berman'):
        hip = tssa.LovaszSoftmaxLoss(C, 255, variant)
        for name, x in (('bf16', logits.bfloat16()), ('f32', logits)):
            out['hip_%s_%s' % (variant, name)] = timed(hip, x, target, a.iters)
    if not a.skip_stock:
        out['stock_pytorch_reference_f32'] = timed(lambda x, t: stock_lovasz(x, t, C, 255, 'reference'), logits, target, a.iters)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
