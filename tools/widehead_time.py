"""Time and peak memory of the fused head at Mapillary's 66 classes (csrc/widehead.hip) next to the unfused composition it replaces,
at FastSCNN's low-resolution map for 8 x 3 x 1024 x 2048 images (8 x 66 x 128 x 256 -> 1024 x 2048, NHWC as forward_lowres returns it),
bf16 and f32 logits:

    ce_plain, ce_w_eps   forward + backward of tssa.upsample_cross_entropy (plain; class weights + label smoothing 0.1)
                         against tssa.cross_entropy(ops.upsample_logits(low)): what the same call did before the wide kernels
    ohem                 forward + backward of ops.upsample_ohem_loss against tssa.OHEMLoss()(ops.upsample_logits(low))
    argmax               tssa.upsample_argmax_confusion.  At 66 classes the unfused pair cannot run at all (its planar kernel stops
                         at 64 classes), so there is no earlier number: both paths are timed at 64 classes instead, and the fused one
                         alone at 66
    narrow19             the register kernel at 19 classes, for scale (plain cross-entropy and arg-max)

Both sides of a pair are timed over windows of `--calls` calls between two device synchronisations, alternating, after a warm-up of
every configuration; median / min / max over the windows.  Peak memory: torch.cuda.max_memory_allocated() over one call after
reset_peak_memory_stats(), minus what was allocated before it (inputs excluded).

Prints one JSON line (profiles/widehead_time.json).

    python tools/widehead_time.py [--shape 8 66 128 256] [--scale 8] [--calls 10] [--windows 7]
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
EPS = 0.1


def inputs(shape, scale, dtype):
    B, C, h, w = shape
    g = torch.Generator().manual_seed(0)
    low = ops.to_nhwc((2.0 * torch.randn(B, C, h, w, generator=g)).to(DEV).to(dtype)).detach().requires_grad_(True)
    y = torch.randint(0, C, (B, h * scale, w * scale), generator=g)
    y[torch.rand(y.shape, generator=g) < 0.05] = 255
    wgt = (torch.rand(C, generator=g) * 9 + 1).to(DEV)
    return low, y.to(DEV), wgt


def sides(kind, scale, wgt):
    """{'fused': fn, 'unfused': fn}; fn(low, y) runs forward (+ backward for the losses) and returns a tensor to read back."""
    def loss(fn):
        def run(low, y):
            out = fn(low, y)
            out.backward()
            low.grad = None
            return out
        return run
    if kind == 'ce_plain':
        return {'fused': loss(lambda a, y: tssa.upsample_cross_entropy(a, y, scale_factor=scale, ignore_index=255)),
                'unfused': loss(lambda a, y: tssa.cross_entropy(ops.upsample_logits(a, scale_factor=scale), y, 255))}
    if kind == 'ce_w_eps':
        return {'fused': loss(lambda a, y: tssa.upsample_cross_entropy(a, y, scale_factor=scale, ignore_index=255, weight=wgt, label_smoothing=EPS)),
                'unfused': loss(lambda a, y: tssa.cross_entropy(ops.upsample_logits(a, scale_factor=scale), y, 255, weight=wgt, label_smoothing=EPS))}
    if kind == 'ohem':
        ohem = tssa.OHEMLoss(ignore_index=255)
        return {'fused': loss(lambda a, y: ops.upsample_ohem_loss(a, y, scale_factor=scale, ignore_index=255)),
                'unfused': loss(lambda a, y: ohem(ops.upsample_logits(a, scale_factor=scale), y))}
    assert kind == 'argmax'

    def fused(a, y):
        with torch.no_grad():
            return tssa.upsample_argmax_confusion(a, y, scale_factor=scale, want_pred=False)[1]

    def unfused(a, y):
        with torch.no_grad():
            return tssa.argmax_confusion(ops.upsample_logits(a, scale_factor=scale), y, want_pred=False)[1]
    return {'fused': fused, 'unfused': unfused}


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


def compare(kind, shape, scale, dtype, calls, windows, which=('fused', 'unfused')):
    low, y, wgt = inputs(shape, scale, dtype)
    fns = {k: f for k, f in sides(kind, scale, wgt).items() if k in which}
    for fn in fns.values():
        window(fn, low, y, max(2, calls // 2))            # warm-up: code objects, allocator, clocks
    times = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():                           # alternating
            times[k].append(window(fn, low, y, calls)[0])
    out = {}
    for k, fn in fns.items():
        v = sorted(times[k])
        out[k] = {'ms_median': round(v[len(v) // 2], 4), 'ms_min': round(v[0], 4), 'ms_max': round(v[-1], 4),
                  'ms_windows_in_order': [round(t, 4) for t in times[k]], 'peak_mb': peak_mb(fn, low, y)}
    if len(fns) == 2:
        out['unfused_over_fused'] = round(out['unfused']['ms_median'] / out['fused']['ms_median'], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=4, default=[8, 66, 128, 256])
    ap.add_argument('--scale', type=int, default=8)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--windows', type=int, default=7)
    a = ap.parse_args()
    B, C, h, w = a.shape
    out = {'tool': 'tools/widehead_time.py', 'device': torch.cuda.get_device_name(0), 'shape': a.shape, 'scale': a.scale,
           'layout': 'NHWC, pitch 8-aligned', 'calls_per_window': a.calls, 'windows': a.windows,
           'full_resolution_logits_mb': {'bf16': round(B * C * h * w * a.scale ** 2 * 2 / 1e6, 1), 'f32': round(B * C * h * w * a.scale ** 2 * 4 / 1e6, 1)},
           'what': 'ms per call (losses: forward + backward; argmax: forward): host wall clock over a window of calls that ends in a sync, '
                   'median / min / max over the windows, fused and unfused alternating, after a warm-up of each; peak_mb: rise of '
                   'torch.cuda.max_memory_allocated over one call'}
    for name, dtype in (('bf16', torch.bfloat16), ('f32', torch.float32)):
        for kind in ('ce_plain', 'ce_w_eps', 'ohem'):
            out['%s_%s' % (kind, name)] = compare(kind, a.shape, a.scale, dtype, a.calls, a.windows)
        out['argmax_c%d_%s' % (C, name)] = compare('argmax', a.shape, a.scale, dtype, a.calls, a.windows, which=('fused',) if C > 64 else ('fused', 'unfused'))
        out['argmax_c64_%s' % name] = compare('argmax', [B, 64, h, w], a.scale, dtype, a.calls, a.windows)
        out['narrow19_ce_plain_%s' % name] = compare('ce_plain', [B, 19, h, w], a.scale, dtype, a.calls, a.windows, which=('fused',))
        out['narrow19_argmax_%s' % name] = compare('argmax', [B, 19, h, w], a.scale, dtype, a.calls, a.windows, which=('fused',))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
