"""Time of one optimizer step of engine.FlatAdamW / engine.FlatSGD (csrc/optim.hip) on the flat buffers -- one group, three groups,
three groups + global-norm clip, Nesterov SGD + clip -- next to torch.optim.AdamW / SGD (+ torch.nn.utils.clip_grad_norm_) over the
same number of elements split into ~200 parameter tensors, on the same GPU.  Prints one JSON line (profiles/flat_optim_time.json).

    python tools/flat_optim_time.py [--sizes 1137795 50000000] [--iters 50] [--tensors 200]

Times come from device events around `iters` back-to-back steps after a warm-up; bytes/s from the algorithmic bytes: AdamW step 28 B
per element (p, g, m, v read; p, m, v written), SGD with momentum 20 B, the norm 4 B.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_semantic_segmentation_amd import engine as E  # noqa: E402

FASTSCNN_PARAMS = 1137795        # cases.product_model('fastscnn'): tests/test_boundary.py
BYTES = {'adamw': 28, 'sgd_momentum': 20, 'norm': 4}


def tensors(n, count, dev, seed):
    """`count` parameter tensors of n elements in all (the last takes the remainder), N(0, 1) gradients attached."""
    g = torch.Generator(device=dev).manual_seed(seed)
    per = max(1, n // count)
    sizes = [per] * (count - 1) + [n - per * (count - 1)] if n > per * (count - 1) else [n]
    ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g)) for s in sizes]
    return ps, [torch.randn(s, device=dev, generator=g) for s in sizes]


def three(ps):
    k = len(ps) // 3
    return [dict(params=ps[:k]), dict(params=ps[k:2 * k], weight_decay=0.0), dict(params=ps[2 * k:], lr=1e-2)]


def timed(step, iters, warmup=5):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def row(ms, n, bytes_per_element):
    return {'ms_per_step': round(ms, 4), 'algorithmic_GBps': round(bytes_per_element * n / (ms * 1e-3) / 1e9, 1),
            'bytes_per_element': bytes_per_element}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[FASTSCNN_PARAMS, 50_000_000])
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--tensors', type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/flat_optim_time.py needs a GPU: nothing is timed without one')
    dev = 'cuda:0'
    out = {'tool': 'tools/flat_optim_time.py', 'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'tensors': a.tensors,
           'what': 'one optimizer step (clip included where named), device events around `iters` back-to-back steps', 'sizes': {}}
    for n in a.sizes:
        res = {}

        def flat(make, bytes_per_element):
            ps, gs = tensors(n, a.tensors, dev, 1)
            opt = make(ps)
            for p, g in zip(ps, gs):
                p.grad.copy_(g)
            return row(timed(opt.step, a.iters), n, bytes_per_element)

        def stock(make, clip, bytes_per_element):
            ps, gs = tensors(n, a.tensors, dev, 1)
            opt = make(ps)
            for p, g in zip(ps, gs):
                p.grad = g.clone()

            def step():
                if clip is not None:
                    torch.nn.utils.clip_grad_norm_(ps, clip)
                opt.step()
            return row(timed(step, a.iters), n, bytes_per_element)

        clip = 1e30          # never engages: the gradients (and so the work) stay the same from step to step
        res['flat_adamw_1group'] = flat(lambda ps: E.FlatAdamW(ps, lr=1e-3), BYTES['adamw'])
        res['flat_adamw_3groups'] = flat(lambda ps: E.FlatAdamW(three(ps), lr=1e-3), BYTES['adamw'])
        res['flat_adamw_3groups_clip'] = flat(lambda ps: E.FlatAdamW(three(ps), lr=1e-3, max_grad_norm=clip), BYTES['adamw'] + BYTES['norm'])
        res['flat_sgd_nesterov_clip'] = flat(lambda ps: E.FlatSGD(three(ps), lr=1e-3, momentum=0.9, nesterov=True, max_grad_norm=clip),
                                             BYTES['sgd_momentum'] + BYTES['norm'])
        res['stock_adamw_3groups'] = stock(lambda ps: torch.optim.AdamW(three(ps), lr=1e-3), None, BYTES['adamw'])
        res['stock_adamw_3groups_clip'] = stock(lambda ps: torch.optim.AdamW(three(ps), lr=1e-3), clip, BYTES['adamw'] + BYTES['norm'])
        res['stock_sgd_nesterov_clip'] = stock(lambda ps: torch.optim.SGD(three(ps), lr=1e-3, momentum=0.9, nesterov=True), clip,
                                               BYTES['sgd_momentum'] + BYTES['norm'])
        out['sizes'][str(n)] = res
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
