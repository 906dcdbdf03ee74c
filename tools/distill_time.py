"""Forward + backward time of tssa.distillation_loss (csrc/distill.hip), pixel and channel kind, at FastSCNN's low-resolution
map for 8 x 3 x 1024 x 2048 images (8 x 19 x 128 x 256, NHWC as forward_lowres returns it), bf16 and f32 logits, next to the
composition it replaces on stock PyTorch on the same GPU: F.kl_div(F.log_softmax(s / T), F.softmax(t / T)) -- for the channel
kind on (B C, h w) rows, which on the NHWC map costs the transposing copy that is part of what is timed.  Both sides are timed
over windows of `--calls` forward + backward calls between two device synchronisations, the two sides alternating, after a
warm-up; the numbers are launch-bound at this size (see README.md).

With --trainer it also times one captured engine.Trainer step (FastSCNN, bf16, FlatAdamW, fused head + cross-entropy) at the
benchmark's 8 x 3 x 1024 x 2048 without and with a teacher of the student's architecture (channel kind, T = 4).

Prints one JSON line (profiles/distill_time.json).

    python tools/distill_time.py [--shape 8 19 128 256] [--calls 200] [--windows 7] [--trainer]
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
from torch_semantic_segmentation_amd import engine as E, ops  # noqa: E402

TAU = 4.0


def stock(kind):
    def fn(s, t):
        B, C, h, w = s.shape
        if kind == 'pixel':
            return F.kl_div(F.log_softmax(s / TAU, 1), F.softmax(t / TAU, 1), reduction='sum') * (TAU ** 2 / (B * h * w))
        rs, rt = s.reshape(B * C, h * w), t.reshape(B * C, h * w)       # NHWC storage: this is the transposing copy
        return F.kl_div(F.log_softmax(rs / TAU, 1), F.softmax(rt / TAU, 1), reduction='sum') * (TAU ** 2 / (B * C))
    return fn


def window(fn, x, t, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        loss = fn(x, t)
        loss.backward()
        x.grad = None
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls, float(loss)


def compare(kind, dtype, shape, calls, windows, warm=50):
    B, C, h, w = shape
    g = torch.Generator().manual_seed(0)
    s = ops.to_nhwc((2.0 * torch.randn(B, C, h, w, generator=g)).to('cuda:0').to(dtype)).detach().requires_grad_(True)
    t = ops.to_nhwc((2.0 * torch.randn(B, C, h, w, generator=g)).to('cuda:0').to(dtype))
    sides = {'hip': lambda a, b: tssa.distillation_loss(a, b, TAU, kind), 'stock': stock(kind)}
    times = {k: [] for k in sides}
    losses = {}
    for k, fn in sides.items():
        window(fn, s, t, warm)                                            # warm-up of this shape and dtype, both sides
    if windows == 0:
        return None
    for _ in range(windows):
        for k, fn in sides.items():                                       # alternating
            ms, losses[k] = window(fn, s, t, calls)
            times[k].append(ms)
    out = {}
    for k in sides:
        v = sorted(times[k])
        out[k] = {'ms_median': round(v[len(v) // 2], 5), 'ms_min': round(v[0], 5), 'ms_max': round(v[-1], 5), 'loss': losses[k],
                  'ms_windows_in_order': [round(x, 5) for x in times[k]]}
    out['stock_over_hip'] = round(out['stock']['ms_median'] / out['hip']['ms_median'], 3)
    return out


def trainer_step(with_teacher, steps, warmup):
    import importlib
    M = importlib.import_module('torch_semantic_segmentation_amd.models.fastscnn')     # the package exports the constructor under this name too
    torch.manual_seed(0)
    model = M.fastscnn(3, 19).to('cuda:0')
    tssa.set_compute_dtype(model, torch.bfloat16)
    kw = {}
    if with_teacher:
        torch.manual_seed(1)
        teacher = M.fastscnn(3, 19).to('cuda:0')
        tssa.set_compute_dtype(teacher, torch.bfloat16)
        kw = dict(teacher=teacher, distill_loss=tssa.DistillationLoss(TAU, 'channel'), distill_weight=1.0)
    tr = E.Trainer(model, E.FlatAdamW(model.parameters(), lr=1e-3, weight_decay=1e-5), tssa.CrossEntropyLoss(ignore_index=255),
                   use_graph=True, **kw)
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(8, 3, 1024, 2048, generator=g).to('cuda:0')
    y = torch.randint(0, 19, (8, 1024, 2048), generator=g)
    y[torch.rand(8, 1024, 2048, generator=g) < 0.05] = 255
    y = y.to('cuda:0')
    tr.step_async(x, y)
    x, y = tr.static_batch(x, y)
    for _ in range(warmup):
        tr.step_async(x, y)
    per = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = tr.step_async(x, y)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e3 / steps)
    per.sort()
    res = {'ms_per_step_median': round(per[2], 4), 'ms_per_step_min': round(per[0], 4), 'ms_per_step_max': round(per[-1], 4),
           'steps_per_window': steps, 'windows': 5, 'final_loss': round(float(loss), 4)}
    del tr, model
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=4, default=[8, 19, 128, 256])
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--trainer', action='store_true')
    ap.add_argument('--trainer-steps', type=int, default=40)
    a = ap.parse_args()
    out = {'tool': 'tools/distill_time.py', 'device': torch.cuda.get_device_name(0), 'shape': a.shape, 'layout': 'NHWC, pitch 8-aligned',
           'temperature': TAU, 'calls_per_window': a.calls, 'windows': a.windows,
           'what': 'forward + backward of the loss alone, ms per call: host wall clock over a window of calls that ends in a sync, '
                   'median / min / max over the windows, hip and stock alternating, after one untimed pass over every configuration'}
    for kind in ('pixel', 'channel'):          # every configuration once before anything is timed: code objects, allocator, clocks
        for dtype in (torch.bfloat16, torch.float32):
            compare(kind, dtype, a.shape, a.calls, 0, warm=a.calls)
    for kind in ('pixel', 'channel'):
        for name, dtype in (('bf16', torch.bfloat16), ('f32', torch.float32)):
            out['%s_%s' % (kind, name)] = compare(kind, dtype, a.shape, a.calls, a.windows)
    if a.trainer:
        out['trainer_step_8x3x1024x2048_bf16_graph'] = {'without_teacher': trainer_step(False, a.trainer_steps, 10),
                                                         'with_teacher_channel_kd': trainer_step(True, a.trainer_steps, 10)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
