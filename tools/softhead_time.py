"""Time and peak memory of the focal and the soft Dice loss on the fused decoder head (csrc/softhead.hip) next to the unfused
composition they replace, at FastSCNN's low-resolution map for 8 x 3 x 1024 x 2048 images (8 x C x 128 x 256 -> 1024 x 2048, NHWC as
forward_lowres returns it), bf16 and f32 logits:

    focal_c19   forward + backward of tssa.upsample_focal_loss (the one-pass register kernel) against
                tssa.focal_loss(ops.upsample_logits(low)): what Trainer(model, opt, FocalLoss()) costs for head + loss
    dice_c19    forward + backward of tssa.upsample_dice_loss (statistics pass, gradient pass) against tssa.dice_loss(ops.upsample_logits(low))
    focal_c66   the focal loss at Mapillary's 66 classes: the wide route (per-pixel cross-entropy, coefficient array, weighted tile pass)
    ce_c19      tssa.upsample_cross_entropy at 19 classes, fused side only, for scale

Both sides of a pair are timed over windows of `--calls` calls between two device synchronisations, alternating, after a warm-up of
every configuration; median / min / max over the windows.  Peak memory: torch.cuda.max_memory_allocated() over one call after
reset_peak_memory_stats(), minus what was allocated before it (inputs excluded).

Prints one JSON line and, with --out, writes it (profiles/softhead_time.json).

    python tools/softhead_time.py [--hw 128 256] [--batch 8] [--scale 8] [--calls 10] [--windows 7] [--out profiles/softhead_time.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_semantic_segmentation_amd as tssa  # noqa: E402
from torch_semantic_segmentation_amd import ops  # noqa: E402

DEV = 'cuda:0'


def inputs(shape, scale, dtype):
    B, C, h, w = shape
    g = torch.Generator().manual_seed(0)
    low = ops.to_nhwc((2.0 * torch.randn(B, C, h, w, generator=g)).to(DEV).to(dtype)).detach().requires_grad_(True)
    y = torch.randint(0, C, (B, h * scale, w * scale), generator=g)
    y[torch.rand(y.shape, generator=g) < 0.05] = 255
    return low, y.to(DEV)


def sides(kind, C, scale):
    """{'fused': fn, 'unfused': fn}; fn(low, y) runs forward + backward and returns the loss."""
    def loss(fn):
        def run(low, y):
            out = fn(low, y)
            out.backward()
            low.grad = None
            return out
        return run
    if kind == 'focal':
        return {'fused': loss(lambda a, y: tssa.upsample_focal_loss(a, y, scale_factor=scale, ignore_index=255)),
                'unfused': loss(lambda a, y: tssa.focal_loss(ops.upsample_logits(a, scale_factor=scale), y, ignore_index=255))}
    if kind == 'dice':
        return {'fused': loss(lambda a, y: tssa.upsample_dice_loss(a, y, C, scale_factor=scale, ignore_index=255)),
                'unfused': loss(lambda a, y: tssa.dice_loss(ops.upsample_logits(a, scale_factor=scale), y, C, ignore_index=255))}
    assert kind == 'ce'
    return {'fused': loss(lambda a, y: tssa.upsample_cross_entropy(a, y, scale_factor=scale, ignore_index=255))}


def window(fn, low, y, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        out = fn(low, y)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls, out


def peak_mb(fn, low, y):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn(low, y)
    torch.cuda.synchronize()
    del out
    return round((torch.cuda.max_memory_allocated() - before) / 1e6, 2)


def compare(kind, shape, scale, dtype, calls, windows):
    low, y = inputs(shape, scale, dtype)
    fns = sides(kind, shape[1], scale)
    losses = {}
    for k, fn in fns.items():
        losses[k] = float(window(fn, low, y, max(2, calls // 2))[1])            # warm-up: code objects, allocator, clocks
    times = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():                           # alternating
            times[k].append(window(fn, low, y, calls)[0])
    out = {}
    for k, fn in fns.items():
        v = sorted(times[k])
        out[k] = {'ms_median': round(v[len(v) // 2], 4), 'ms_min': round(v[0], 4), 'ms_max': round(v[-1], 4),
                  'ms_windows_in_order': [round(t, 4) for t in times[k]], 'peak_mb': peak_mb(fn, low, y), 'loss': losses[k]}
    if len(fns) == 2:
        out['unfused_over_fused'] = round(out['unfused']['ms_median'] / out['fused']['ms_median'], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--hw', type=int, nargs=2, default=[128, 256])
    ap.add_argument('--scale', type=int, default=8)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    B, (h, w) = a.batch, a.hw
    px = B * h * w * a.scale ** 2
    out = {'tool': 'tools/softhead_time.py', 'device': torch.cuda.get_device_name(0), 'batch': B, 'lowres_hw': a.hw, 'scale': a.scale,
           'layout': 'NHWC, pitch 8-aligned', 'calls_per_window': a.calls, 'windows': a.windows,
           'full_resolution_logits_mb': {'c19_bf16': round(px * 19 * 2 / 1e6, 1), 'c19_f32': round(px * 19 * 4 / 1e6, 1),
                                         'c66_bf16': round(px * 66 * 2 / 1e6, 1), 'c66_f32': round(px * 66 * 4 / 1e6, 1)},
           'what': 'ms per call, forward + backward of head + loss: host wall clock over a window of calls that ends in a sync, median / '
                   'min / max over the windows, fused and unfused alternating, after a warm-up of each; peak_mb: rise of '
                   'torch.cuda.max_memory_allocated over one call; loss: the value of the warm-up call'}
    for name, dtype in (('bf16', torch.bfloat16), ('f32', torch.float32)):
        for kind, C in (('focal', 19), ('dice', 19), ('focal', 66), ('ce', 19)):
            out['%s_c%d_%s' % (kind, C, name)] = compare(kind, [B, C, h, w], a.scale, dtype, a.calls, a.windows)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
