"""Times of tssa.strong_augment (csrc/strongaug.hip) next to its two yardsticks on the same GPU.  Prints one JSON line
(profiles/strongaug_time.json).

    python tools/strongaug_time.py [--window-ms 200] [--rounds 5] [--skip-step]

  op        strong_augment on 8 x 3 x 512 x 768 and 8 x 3 x 1024 x 2048, f32 and bf16, every sample jittered, at R = 0, 4, 8, against
              mix_batch          tssa.mix_batch alone on the same shape: it moves the same image bytes once (plus labels), so it is
                                 the floor for a pass that also reads the image a second time for the statistics
              torch_R            the plain-torch composition of the same formulas: elementwise ops for the jitter (the HSV turn
                                 spelled out) plus two depthwise F.conv2d on a reflect-padded tensor -- what a user would write today
            with the peak device memory each call adds
  step      one captured self-training step (8 labelled + 8 unlabelled at 3 x 512 x 768, FastSCNN bf16, ClassMix) with and without
            strong=StrongAugment()

Method: every group (one shape and dtype, or the step) runs in a fresh process of its own; in it every candidate is warmed up, a probe
sizes its window to about --window-ms of back-to-back calls between two device events, then the candidates take turns for --rounds
rounds; the figure is the median of a candidate's rounds, and all rounds are kept (their range is the spread)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_semantic_segmentation_amd as tssa  # noqa: E402
from torch_semantic_segmentation_amd import engine as E, ops  # noqa: E402

DEV = 'cuda:0'
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SHAPES = {'8x3x512x768': (8, 512, 768), '8x3x1024x2048': (8, 1024, 2048)}


def window(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(steps, window_ms, rounds):
    iters = {}
    for name, step in steps.items():
        window(step, 3)                                         # warm-up
        iters[name] = max(3, int(window_ms / max(window(step, 5), 1e-4)))
    got = {name: [] for name in steps}
    for _ in range(rounds):
        for name, step in steps.items():
            got[name].append(window(step, iters[name]))
    return {name: {'ms': round(statistics.median(v), 4), 'range_ms': [round(min(v), 4), round(max(v), 4)],
                   'rounds_ms': [round(t, 4) for t in v], 'calls_per_window': iters[name]} for name, v in got.items()}


def peak_added(step):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def torch_hue(u, dh):
    """the HSV turn of include/tss_hip.h (ds = dv = 0) on u [B,3,H,W] in [0, 1], dh [B,1,1] of a turn, in stock elementwise ops"""
    p = u * 255.0
    r, g, b = p[:, 0], p[:, 1], p[:, 2]
    V = p.amax(1)
    D = V - p.amin(1)
    s = D / V.clamp_min(1e-30)
    Dn = D.clamp_min(1e-30)
    H = torch.where(V == r, 30.0 * (g - b) / Dn, torch.where(V == g, 60.0 + 30.0 * (b - r) / Dn, 120.0 + 30.0 * (r - g) / Dn))
    H = torch.where(H < 0, H + 180.0, H) + 180.0 * dh
    H = torch.where(H < 0, H + 180.0, torch.where(H >= 180.0, H - 180.0, H))
    h = H / 30.0
    i = h.floor()
    f = h - i
    pp, q, t = V * (1.0 - s), V * (1.0 - f * s), V * (1.0 - (1.0 - f) * s)
    i = i.long() % 6
    rr = torch.stack([V, q, pp, pp, t, V], 1).gather(1, i[:, None])
    gg = torch.stack([t, V, V, q, pp, pp], 1).gather(1, i[:, None])
    bb = torch.stack([pp, pp, t, V, V, q], 1).gather(1, i[:, None])
    return torch.cat([rr, gg, bb], 1) / 255.0


def torch_compose(x, color, R, taps, mean, std):
    """strong_augment's formulas in stock torch ops, every sample jittered, one radius for the batch"""
    B = x.shape[0]
    u = x.float() * std + mean
    fb, fc, fs, dh = (color[:, k].view(B, 1, 1, 1) for k in (1, 2, 3, 4))
    grey = lambda v: 0.299 * v[:, 0:1] + 0.587 * v[:, 1:2] + 0.114 * v[:, 2:3]  # noqa: E731
    u = (u * fb).clamp(0, 1)
    m = grey(u).double().mean((1, 2, 3), keepdim=True).float()
    u = (m + fc * (u - m)).clamp(0, 1)
    g = grey(u)
    u = (g + fs * (u - g)).clamp(0, 1)
    u = torch_hue(u, dh.view(B, 1, 1))
    if R > 0:
        w = torch.cat([taps[0, 1:R + 1].flip(0), taps[0, :R + 1]])
        u = F.conv2d(F.pad(u, (R, R, 0, 0), mode='reflect'), w.view(1, 1, 1, -1).expand(3, 1, 1, -1).contiguous(), groups=3)
        u = F.conv2d(F.pad(u, (0, 0, R, R), mode='reflect'), w.view(1, 1, -1, 1).expand(3, 1, -1, 1).contiguous(), groups=3)
    return (u / std - mean / std).to(x.dtype)


def rows(B, R):
    rng = np.random.default_rng(R)
    color = np.zeros((B, 8), np.float32)
    color[:, 0] = 1
    color[:, 1:4] = rng.uniform(0.75, 1.25, (B, 3))
    color[:, 4] = rng.uniform(-0.25, 0.25, B)
    taps = np.zeros((B, 12), np.float32)
    taps[:] = tssa.gaussian_taps(R / 3.0)[1]
    dev = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return dev(color), dev(np.full(B, R, np.int32)), dev(taps)


def op_group(shape, dtype, a):
    B, H, W = SHAPES[shape]
    dt = torch.bfloat16 if dtype == 'bf16' else torch.float32
    g = torch.Generator(device=DEV).manual_seed(0)
    mean, std = (torch.tensor(v, device=DEV).view(1, 3, 1, 1) for v in (MEAN, STD))
    x = ((torch.rand(B, 3, H, W, device=DEV, generator=g) - mean) / std).to(dt)
    out = torch.empty_like(x)
    ws = torch.empty(B * 64, dtype=torch.float64, device=DEV)
    labels = torch.randint(0, 19, (B, H, W), device=DEV, generator=g).to(torch.uint8)
    partner = torch.roll(torch.arange(B, dtype=torch.int32, device=DEV), 1)
    boxes = torch.tensor([[H // 4, W // 4, 3 * H // 4, 3 * W // 4]] * B, dtype=torch.int32, device=DEV)
    out_t = torch.empty((B, H, W), dtype=torch.int64, device=DEV)
    steps = {'mix_batch': lambda: tssa.mix_batch(x, labels, partner, boxes=boxes, out_image=out, out_target=out_t)}
    for R in (0, 4, 8):
        c, r, t = rows(B, R)
        steps['fused_R%d' % R] = (lambda c=c, r=r, t=t: tssa.strong_augment(x, c, r, t, MEAN, STD, out=out, workspace=ws))
        steps['torch_R%d' % R] = (lambda c=c, R=R, t=t: torch_compose(x, c, R, t, mean, std))
    res = alternate(steps, a.window_ms, a.rounds)
    esz = 2 if dtype == 'bf16' else 4
    res['image_bytes'] = B * 3 * H * W * esz
    for R in (0, 4, 8):
        f, s = res['fused_R%d' % R], res['torch_R%d' % R]
        c, r, t = rows(B, R)
        f['peak_bytes_added'] = peak_added(lambda: tssa.strong_augment(x, c, r, t, MEAN, STD))
        s['peak_bytes_added'] = peak_added(lambda: torch_compose(x, c, R, t, mean, std))
        f['achieved_GBps_of_3_image_passes'] = round(3 * res['image_bytes'] / (f['ms'] * 1e-3) / 1e9, 1)
        res['torch_over_fused_R%d' % R] = round(s['ms'] / f['ms'], 2)
        res['fused_over_mix_batch_R%d' % R] = round(f['ms'] / res['mix_batch']['ms'], 2)
    res['fused_not_slower_than_torch'] = all(res['fused_R%d' % R]['ms'] <= res['torch_R%d' % R]['ms'] for R in (0, 4, 8))
    return res


def step_group(a):
    import importlib
    FS = importlib.import_module('torch_semantic_segmentation_amd.models.fastscnn')
    B, H, W = 8, 512, 768
    g = torch.Generator().manual_seed(3)
    x16 = torch.randn(2 * B, 3, H, W, generator=g).to(DEV)
    y16 = torch.randint(0, 19, (2 * B, H, W), generator=g).to(DEV)
    xu = x16[B:].contiguous()

    def selftraining(strong):
        torch.manual_seed(0)
        m = tssa.set_compute_dtype(FS.fastscnn(3, 19).to(DEV), torch.bfloat16)
        opt = E.FlatAdamW(m.parameters(), lr=1e-4)
        ema = E.ModelEMA(m, opt, 0.99)
        tr = E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=255), use_graph=True, ema=ema)
        st = tssa.SelfTraining(tr, ema.module, 19, threshold=0.5, mix='classmix', strong=strong)
        with torch.no_grad(), E.EvalPrep(ema.module):
            low0 = ops.materialize(ema.module.forward_lowres(xu))
        st.set_threshold(float(tssa.upsample_pseudo_labels(low0, 0.0, size=(H, W), want_confidence=True)[1].median()))
        return st

    plain = selftraining(None)
    strong = selftraining(tssa.StrongAugment(mean=MEAN, std=STD, color_p=1.0, blur_p=1.0, sigma=(1.0, 8.0 / 3.0)))
    steps = {'selftrain_step_8_plus_8': lambda: plain.step(x16[:B], y16[:B], xu),
             'selftrain_step_8_plus_8_strong': lambda: strong.step(x16[:B], y16[:B], xu)}
    res = alternate(steps, a.window_ms, a.rounds)
    res['strong_minus_plain_ms'] = round(res['selftrain_step_8_plus_8_strong']['ms'] - res['selftrain_step_8_plus_8']['ms'], 4)
    res['strong_over_plain'] = round(res['selftrain_step_8_plus_8_strong']['ms'] / res['selftrain_step_8_plus_8']['ms'], 4)
    res['note'] = 'every unlabelled sample jittered and blurred with R in 3..8 (color_p = blur_p = 1): the dearest draw'
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window-ms', type=float, default=200.0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--group', default=None, help='internal: run one group in this process and print its JSON')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/strongaug_time.py needs a GPU: nothing is timed without one')
    if a.group is not None:
        res = step_group(a) if a.group == 'step' else op_group(*a.group.split(':'), a)
        print('GROUP_JSON ' + json.dumps(res))
        return
    out = {'tool': 'tools/strongaug_time.py', 'device': torch.cuda.get_device_name(0), 'window_ms': a.window_ms, 'rounds': a.rounds,
           'what': 'ms per call: device events around a window of back-to-back calls, a fresh process per group, the candidates of a '
                   'group alternating, median of the rounds with their range; peak_bytes_added = max_memory_allocated over one call '
                   'minus what was allocated before it'}
    groups = ['%s:%s' % (s, d) for s in SHAPES for d in ('f32', 'bf16')] + ([] if a.skip_step else ['step'])
    for grp in groups:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--group', grp, '--window-ms', str(a.window_ms), '--rounds',
                            str(a.rounds)], capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise SystemExit('group %s failed (%d):\n%s' % (grp, p.returncode, p.stderr[-2000:]))
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('GROUP_JSON ')][-1]
        out['step_fastscnn_bf16_3x512x768' if grp == 'step' else 'op_' + grp.replace(':', '_')] = json.loads(line[len('GROUP_JSON '):])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
