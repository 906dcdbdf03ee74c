"""Forward + backward time of the class-weighted, label-smoothed cross-entropy on the decoder head of FastSCNN: low-resolution logits
8 x 19 x 128 x 256 (NHWC as forward_lowres returns them) against 8 x 1024 x 2048 labels, bf16 and f32, for

    fused_plain     tssa.upsample_cross_entropy(low, y)                              the existing one-pass instance
    fused_w         ... weight=w                                                     the weighted instance
    fused_w_eps     ... weight=w, label_smoothing=0.1                                the smoothed instance
    unfused_w       tssa.cross_entropy(ops.upsample_logits(low), y, weight=w)        the same build without the fusion
    unfused_w_eps   ... label_smoothing=0.1
    stock_w_eps     F.cross_entropy(F.interpolate(low, bilinear, align_corners=True), y, weight=w, label_smoothing=0.1) on stock PyTorch

Every side is timed over windows of forward + backward calls between two device synchronisations, the sides alternating, after a
warm-up of every side.  w = tssa.enet_class_weights(tssa.label_histogram(y)).  `faster_than_unfused_beyond_spread` compares the
slowest window of a fused side with the fastest window of its unfused counterpart.

Prints one JSON line (profiles/wce_time.json).

    python tools/wce_time.py [--shape 8 19 128 256] [--scale 8] [--calls 500] [--windows 7]
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
from torch_semantic_segmentation_amd import ops  # noqa: E402

EPS = 0.1
SLOW = ('stock_w_eps',)          # sides that get a quarter of the calls per window


def sides(size, w):
    return {
        'fused_plain': lambda low, y: tssa.upsample_cross_entropy(low, y, size=size, ignore_index=255),
        'fused_w': lambda low, y: tssa.upsample_cross_entropy(low, y, size=size, ignore_index=255, weight=w),
        'fused_w_eps': lambda low, y: tssa.upsample_cross_entropy(low, y, size=size, ignore_index=255, weight=w, label_smoothing=EPS),
        'unfused_w': lambda low, y: tssa.cross_entropy(ops.upsample_logits(low, size=size), y, 255, weight=w),
        'unfused_w_eps': lambda low, y: tssa.cross_entropy(ops.upsample_logits(low, size=size), y, 255, weight=w, label_smoothing=EPS),
        'stock_w_eps': lambda low, y: F.cross_entropy(F.interpolate(low, size=size, mode='bilinear', align_corners=True), y,
                                                      weight=w.to(low.dtype), ignore_index=255, label_smoothing=EPS),
    }


def window(fn, low, y, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        loss = fn(low, y)
        loss.backward()
        low.grad = None
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls, float(loss.detach())


def compare(dtype, shape, scale, calls, windows):
    B, C, h, w = shape
    size = (h * scale, w * scale)
    g = torch.Generator().manual_seed(0)
    low = ops.to_nhwc((2.0 * torch.randn(B, C, h, w, generator=g)).to('cuda:0').to(dtype)).detach().requires_grad_(True)
    y = torch.randint(0, C, (B,) + size, generator=g)
    y[torch.rand((B,) + size, generator=g) < 0.05] = 255
    y = y.to('cuda:0')
    cw = tssa.enet_class_weights(tssa.label_histogram(y, C, ignore_index=255))
    fns = sides(size, cw)
    n = {k: max(calls // 4, 2) if k in SLOW else calls for k in fns}
    times, losses = {k: [] for k in fns}, {}
    for k, fn in fns.items():
        window(fn, low, y, max(n[k] // 2, 2))
    for _ in range(windows):
        for k, fn in fns.items():                                         # alternating
            ms, losses[k] = window(fn, low, y, n[k])
            times[k].append(ms)
    out = {}
    for k in fns:
        v = sorted(times[k])
        out[k] = {'ms_median': round(v[len(v) // 2], 5), 'ms_min': round(v[0], 5), 'ms_max': round(v[-1], 5), 'loss': losses[k],
                  'calls_per_window': n[k], 'ms_windows_in_order': [round(x, 5) for x in times[k]]}
    for k in ('fused_w', 'fused_w_eps'):
        u = 'un' + k
        out[k]['over_fused_plain'] = round(out[k]['ms_median'] / out['fused_plain']['ms_median'], 3)
        out[k]['unfused_over_fused'] = round(out[u]['ms_median'] / out[k]['ms_median'], 3)
        out[k]['faster_than_unfused_beyond_spread'] = out[k]['ms_max'] < out[u]['ms_min']
    out['stock_over_fused_w_eps'] = round(out['stock_w_eps']['ms_median'] / out['fused_w_eps']['ms_median'], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=4, default=[8, 19, 128, 256])
    ap.add_argument('--scale', type=int, default=8)
    ap.add_argument('--calls', type=int, default=500)
    ap.add_argument('--windows', type=int, default=7)
    a = ap.parse_args()
    out = {'tool': 'tools/wce_time.py', 'device': torch.cuda.get_device_name(0), 'low_shape': a.shape, 'scale': a.scale,
           'layout': 'low: NHWC, pitch 8-aligned', 'label_smoothing': EPS, 'windows': a.windows,
           'what': 'forward + backward of head + loss, ms per call: host wall clock over a window of calls that ends in a sync, '
                   'median / min / max over the windows, the sides alternating, after a warm-up of every side'}
    for name, dtype in (('bf16', torch.bfloat16), ('f32', torch.float32)):
        out[name] = compare(dtype, a.shape, a.scale, a.calls, a.windows)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
