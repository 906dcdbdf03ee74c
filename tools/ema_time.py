"""Time of one optimizer step that also keeps a moving average of the weights (engine.FlatOptimizer.attach_ema, csrc/optim.hip), next
to the ways of getting the same average without it, on the same GPU.  Prints one JSON line (profiles/ema_time.json).

    python tools/ema_time.py [--sizes 1137795 50000000] [--window-ms 200] [--rounds 5] [--tensors 200]

Candidates, all AdamW over the same number of elements:
    step            FlatAdamW.step() alone, no average                                       28 B per element
    fused           FlatAdamW.step() with attach_ema: the step kernel averages               36 B
    separate_lerp   FlatAdamW.step(), then ema_flat.lerp_(flat_param, 1 - decay)             28 + 12 B, one more launch
    stock_foreach   torch.optim.AdamW over ~`tensors` parameter tensors, then torch._foreach_lerp_ over them      40 B

Method: every candidate is warmed up, a probe sizes its window to about --window-ms of back-to-back steps between two device events,
then the candidates take turns for --rounds rounds; the figure is the median of a candidate's rounds, and all rounds are kept.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_semantic_segmentation_amd import engine as E  # noqa: E402

FASTSCNN_PARAMS = 1137795        # cases.product_model('fastscnn'): tests/test_boundary.py
BYTES = {'step': 28, 'fused': 36, 'separate_lerp': 40, 'stock_foreach': 40}
DECAY = 0.999


def tensors(n, count, dev, seed):
    """`count` parameter tensors of n elements in all (the last takes the remainder), N(0, 1) gradients next to them."""
    g = torch.Generator(device=dev).manual_seed(seed)
    per = max(1, n // count)
    sizes = [per] * (count - 1) + [n - per * (count - 1)] if n > per * (count - 1) else [n]
    ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g)) for s in sizes]
    return ps, [torch.randn(s, device=dev, generator=g) for s in sizes]


def window(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def candidates(n, count, dev):
    out = {}

    def flat(attach):
        ps, gs = tensors(n, count, dev, 1)
        opt = E.FlatAdamW(ps, lr=1e-3)
        for p, g in zip(ps, gs):
            p.grad.copy_(g)
        ema = opt.flat_param.clone()
        if attach:
            opt.attach_ema(ema, DECAY)
        return opt, ema

    opt, _ = flat(False)
    out['step'] = opt.step
    opt_f, _ = flat(True)
    out['fused'] = opt_f.step
    opt_s, ema_s = flat(False)

    def separate():
        opt_s.step()
        ema_s.lerp_(opt_s.flat_param, 1.0 - DECAY)
    out['separate_lerp'] = separate

    ps, gs = tensors(n, count, dev, 1)
    stock = torch.optim.AdamW(ps, lr=1e-3)
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    emas = [p.detach().clone() for p in ps]
    live = [p.detach() for p in ps]

    def foreach():
        stock.step()
        torch._foreach_lerp_(emas, live, 1.0 - DECAY)
    out['stock_foreach'] = foreach
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[FASTSCNN_PARAMS, 50_000_000])
    ap.add_argument('--window-ms', type=float, default=200.0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--tensors', type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/ema_time.py needs a GPU: nothing is timed without one')
    dev = 'cuda:0'
    out = {'tool': 'tools/ema_time.py', 'device': torch.cuda.get_device_name(0), 'decay': DECAY, 'tensors': a.tensors,
           'window_ms': a.window_ms, 'rounds': a.rounds,
           'what': 'ms per optimizer step (average included where named): device events around a window of back-to-back steps, '
                   'candidates alternating, median of the rounds', 'sizes': {}}
    for n in a.sizes:
        steps = candidates(n, a.tensors, dev)
        iters = {}
        for name, step in steps.items():
            window(step, 10)                                        # warm-up
            iters[name] = max(10, int(a.window_ms / max(window(step, 20), 1e-4)))
        rounds = {name: [] for name in steps}
        for _ in range(a.rounds):
            for name, step in steps.items():
                rounds[name].append(window(step, iters[name]))
        res = {}
        for name in steps:
            ms = statistics.median(rounds[name])
            res[name] = {'ms_per_step': round(ms, 4), 'rounds_ms': [round(v, 4) for v in rounds[name]], 'steps_per_window': iters[name],
                         'bytes_per_element': BYTES[name], 'algorithmic_GBps': round(BYTES[name] * n / (ms * 1e-3) / 1e9, 1)}
        base = res['step']['ms_per_step']
        res['ratios'] = {'fused_over_step': round(res['fused']['ms_per_step'] / base, 3), 'expected_from_traffic_fused': round(36 / 28, 3),
                         'separate_lerp_over_step': round(res['separate_lerp']['ms_per_step'] / base, 3),
                         'expected_from_traffic_separate': round(40 / 28, 3),
                         'fused_over_separate_lerp': round(res['fused']['ms_per_step'] / res['separate_lerp']['ms_per_step'], 3)}
        res['fused_not_slower_than_separate_lerp'] = res['fused']['ms_per_step'] <= res['separate_lerp']['ms_per_step']
        out['sizes'][str(n)] = res
        del steps
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
