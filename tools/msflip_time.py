"""Time of multi-scale + flip evaluation (csrc/msflip.hip) for one 1x3x1024x2048 image through FastSCNN (bf16 activations) at the
default six scales with flip: twelve low-resolution logit maps fused into one prediction and one confusion-matrix update.

  fused            tssa.multiscale_argmax_confusion on the six 2B maps: one launch, no full-resolution float tensor
  composed         the same maps through operators that existed before it: per map upsample_logits -> torch softmax -> flip ->
                   add_ into an f32 [1,19,H,W] accumulator, then argmax_confusion
  single_scale_xK  K = 12 calls of upsample_argmax_confusion, one per map (a different result: the floor of K launches that
                   each write a prediction; what the fused kernel's K-map loop is compared with)
  protocol         MultiScaleEvaluator.predict: six resize_flip_image + forward_lowres passes and the fused call

    python tools/msflip_time.py [--size 1024 2048] [--window-ms 300] [--rounds 5] [--out FILE]

Every candidate is warmed up, then timed with device events over a window of calls; the window is sized per candidate from a first
timing so that it lasts about `window-ms` (a sub-millisecond call is repeated hundreds of times, a slow composition a few), and
never fewer than 3 calls.  The candidates are visited `rounds` times in turn (alternating, so drift hits all of them alike); the
per-round times are all reported, the median is the headline.
"""
import argparse
import importlib
import json
import math
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_semantic_segmentation_amd as tssa  # noqa: E402
from torch_semantic_segmentation_amd import engine as E, ops  # noqa: E402


def one_round(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters * 1e3          # microseconds per call


def commit():
    try:
        return subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, nargs=2, default=[1024, 2048])
    ap.add_argument('--window-ms', type=float, default=300.0, help='length of one timed window, per candidate and round')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--commit', default=None, help='recorded in the file (default: git rev-parse of the checkout, if it is one)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'msflip_time.json'))
    a = ap.parse_args()
    H, W = a.size
    dev = 'cuda:0'
    torch.manual_seed(0)
    model = importlib.import_module('torch_semantic_segmentation_amd.models.fastscnn').fastscnn(3, 19).to(dev).eval()
    tssa.set_compute_dtype(model, torch.bfloat16)
    x = torch.randn(1, 3, H, W, device=dev)
    target = torch.randint(0, 19, (1, H, W), device=dev)
    target[:, :8] = 255
    ev = E.MultiScaleEvaluator(model, dev)
    with torch.no_grad():
        lows, flips = ev.lowres_maps(x)
        lows = [ops.to_nhwc(ops.materialize(low)) for low in lows]
        halves = [(low[i:i + 1], f) for low in lows for i, f in enumerate((False, True))]
        K = len(halves)
        cm = torch.zeros((19, 19), dtype=torch.int64, device=dev)
        acc = torch.empty((1, 19, H, W), dtype=torch.float32, device=dev)

        def fused():
            return tssa.multiscale_argmax_confusion(lows, flips, target, size=(H, W), confusion=cm)

        def composed():
            for i, (low, f) in enumerate(halves):
                p = torch.softmax(ops.upsample_logits(low, size=(H, W)).float(), dim=1)
                if f:
                    p = p.flip(-1)
                if i == 0:
                    acc.copy_(p)
                else:
                    acc.add_(p)
            return tssa.argmax_confusion(acc, target, confusion=cm)

        def single_scale_xk():
            for low, _f in halves:
                tssa.upsample_argmax_confusion(low, target, size=(H, W), confusion=cm)

        def protocol():
            return ev.predict(x)

        cands = [('fused', fused), ('composed', composed), ('single_scale_xK', single_scale_xk), ('protocol', protocol)]
        agree = float((fused()[0] == composed()[0]).double().mean())      # also the warm-up of both
        iters = {}
        for name, fn in cands:
            one_round(fn, 2)
            iters[name] = max(3, int(math.ceil(a.window_ms * 1e3 / max(one_round(fn, 3), 1e-3))))
        us = {name: [] for name, _ in cands}
        for _ in range(a.rounds):
            for name, fn in cands:
                us[name].append(round(one_round(fn, iters[name]), 1))
    esz = lows[0].element_size()
    low_bytes = sum(low.shape[0] * low.shape[2] * low.shape[3] * 19 * esz for low in lows)
    need = low_bytes + H * W * (1 + 8)                       # the maps once, the int64 target, the uint8 prediction
    res = {'tool': 'tools/msflip_time.py', 'device': torch.cuda.get_device_name(0), 'commit': a.commit or commit(),
           'image': [1, 3, H, W], 'scales': list(ev.scales), 'flip': True, 'maps': [list(low.shape) for low in lows], 'K': K,
           'map_dtype': str(lows[0].dtype), 'window_ms': a.window_ms, 'iters': iters, 'rounds': a.rounds,
           'what': 'device events around a window of iters[candidate] calls, microseconds per call for every round; GB/s = algorithmic bytes (the maps '
                   'once + int64 target + uint8 prediction) over the median; pred_agreement = share of pixels where the fused and '
                   'the composed prediction are equal (they round differently: bf16 full-resolution logits in the composition)',
           'algorithmic_bytes': int(need), 'composed_full_resolution_bytes_per_map': 19 * H * W * esz,
           'pred_agreement_fused_vs_composed': round(agree, 6)}
    for name, _ in cands:
        res[name] = {'us_rounds': us[name], 'us_median': sorted(us[name])[len(us[name]) // 2]}
    res['fused']['GBps'] = round(need / res['fused']['us_median'] / 1e3, 1)
    res['composed_over_fused'] = round(res['composed']['us_median'] / res['fused']['us_median'], 2)
    res['single_scale_xK_over_fused'] = round(res['single_scale_xK']['us_median'] / res['fused']['us_median'], 2)
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
