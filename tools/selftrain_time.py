"""Times of the self-training operators (torch_semantic_segmentation_amd/selftrain.py; csrc/pseudo.hip, csrc/mix.hip) next to their
stock compositions on the same GPU.  Prints one JSON line (profiles/selftrain_time.json).

    python tools/selftrain_time.py [--window-ms 200] [--rounds 5] [--skip-step]

  pseudo    at 8 x 19 x 128 x 256 -> 1024 x 2048, bf16 and f32:
              fused, fused_conf   tssa.upsample_pseudo_labels without / with the confidence map
              stock               F.interpolate(bilinear, align_corners=True) -> softmax -> max -> where
              argmax              tssa.upsample_argmax_confusion (no exponentials: for scale)
            and the peak device memory each call adds
  mix       classmix_select + mix_batch on 8 x 3 x 1024 x 2048 f32 against a torch.where composition that is handed the class pick
            (stock_where) and one that also makes the pick with torch.unique per sample (stock_unique); achieved bytes / s from the
            bytes the shapes require (image read once and written once, two label reads, the int64 target)
  step      one captured self-training step (8 labelled + 8 unlabelled at 3 x 512 x 768, FastSCNN bf16, ClassMix) against a plain
            captured step on 16 labelled samples and the teacher's captured forward alone

Method: every candidate is warmed up, a probe sizes its window to about --window-ms of back-to-back calls between two device events,
then the candidates of a group take turns for --rounds rounds; the figure is the median of a candidate's rounds, and all rounds are kept."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_semantic_segmentation_amd as tssa  # noqa: E402
from torch_semantic_segmentation_amd import engine as E, ops  # noqa: E402

DEV = 'cuda:0'


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
    return {name: {'ms': round(statistics.median(v), 4), 'rounds_ms': [round(t, 4) for t in v], 'calls_per_window': iters[name]}
            for name, v in got.items()}


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


def pseudo_group(dtype, a):
    B, C, h, w, H, W = 8, 19, 128, 256, 1024, 2048
    g = torch.Generator(device=DEV).manual_seed(0)
    nchw = (torch.randn(B, C, h, w, device=DEV, generator=g) * 3).to(dtype)
    low = ops.to_nhwc(nchw)
    thr = torch.tensor([0.9], dtype=torch.float32, device=DEV)
    lab = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)
    kept = torch.zeros(B, dtype=torch.int64, device=DEV)
    ign = torch.full((), 255, dtype=torch.int64, device=DEV)

    def stock():
        z = F.interpolate(nchw, size=(H, W), mode='bilinear', align_corners=True)
        conf, arg = torch.softmax(z, 1).max(1)
        return torch.where(conf >= thr.to(conf.dtype), arg, ign)

    steps = {'fused': lambda: tssa.upsample_pseudo_labels(low, thr, size=(H, W), kept=kept, out=lab),
             'fused_conf': lambda: tssa.upsample_pseudo_labels(low, thr, size=(H, W), want_confidence=True, kept=kept, out=lab),
             'stock': stock,
             'argmax': lambda: tssa.upsample_argmax_confusion(low, size=(H, W))}
    res = alternate(steps, a.window_ms, a.rounds)
    for name, step in steps.items():
        res[name]['peak_bytes_added'] = peak_added(step)
    res['fused_not_slower_than_stock'] = res['fused']['ms'] <= res['stock']['ms'] and res['fused_conf']['ms'] <= res['stock']['ms']
    res['stock_over_fused'] = round(res['stock']['ms'] / res['fused']['ms'], 2)
    res['stock_over_fused_conf'] = round(res['stock']['ms'] / res['fused_conf']['ms'], 2)
    res['fused_over_argmax'] = round(res['fused']['ms'] / res['argmax']['ms'], 2)
    return res


def mix_group(a):
    B, Ci, H, W, C = 8, 3, 1024, 2048, 19
    g = torch.Generator(device=DEV).manual_seed(1)
    image = torch.randn(B, Ci, H, W, device=DEV, generator=g)
    # label maps made of 64 x 64 patches, as coherent as a segmentation map; 3 % ignore bytes
    coarse = torch.randint(0, C, (B, 1, H // 64, W // 64), device=DEV, generator=g).float()
    labels = F.interpolate(coarse, size=(H, W), mode='nearest')[:, 0].to(torch.uint8)
    labels[torch.rand(B, H, W, device=DEV, generator=g) < 0.03] = 255
    rng = np.random.default_rng(2)
    keys = torch.from_numpy(rng.integers(0, 2 ** 32, (B, 256), dtype=np.uint64).astype(np.uint32).view(np.int32)).to(DEV)
    partner = torch.roll(torch.arange(B, dtype=torch.int32, device=DEV), 1)
    pl = partner.long()
    out_i, out_t = torch.empty_like(image), torch.empty((B, H, W), dtype=torch.int64, device=DEV)
    sel0 = tssa.classmix_select(labels, keys, C)

    def fused():
        sel = tssa.classmix_select(labels, keys, C)
        return tssa.mix_batch(image, labels, partner, sel=sel, out_image=out_i, out_target=out_t)

    def where(sel):
        mask = sel.gather(1, labels.flatten(1).long()).view(B, H, W).bool()
        return torch.where(mask[:, None], image, image[pl]), torch.where(mask, labels, labels[pl]).long()

    def stock_unique():
        sel = torch.zeros((B, 256), dtype=torch.uint8, device=DEV)
        for b in range(B):
            present = torch.unique(labels[b])
            present = present[present < C]
            order = torch.argsort(keys[b][present.long()].long() & 0xffffffff, stable=True)
            sel[b, present[order[:(len(order) + 1) // 2]].long()] = 1
        return where(sel)

    steps = {'fused': fused, 'mix_batch_alone': lambda: tssa.mix_batch(image, labels, partner, sel=sel0, out_image=out_i, out_target=out_t),
             'classmix_select_alone': lambda: tssa.classmix_select(labels, keys, C),
             'stock_where': lambda: where(sel0), 'stock_unique': stock_unique}
    res = alternate(steps, a.window_ms, a.rounds)
    need = B * H * W * (2 * Ci * 4 + 2 + 8)
    res['bytes_required'] = need
    for name in ('fused', 'mix_batch_alone'):
        res[name]['achieved_GBps'] = round(need / (res[name]['ms'] * 1e-3) / 1e9, 1)
    res['classmix_select_alone']['achieved_GBps'] = round(B * H * W / (res['classmix_select_alone']['ms'] * 1e-3) / 1e9, 1)
    res['fused_not_slower_than_stock'] = res['fused']['ms'] <= res['stock_where']['ms']
    res['stock_where_over_fused'] = round(res['stock_where']['ms'] / res['fused']['ms'], 2)
    res['stock_unique_over_fused'] = round(res['stock_unique']['ms'] / res['fused']['ms'], 2)
    return res


def step_group(a):
    import importlib
    FS = importlib.import_module('torch_semantic_segmentation_amd.models.fastscnn')
    B, H, W = 8, 512, 768
    g = torch.Generator().manual_seed(3)
    x16 = torch.randn(2 * B, 3, H, W, generator=g).to(DEV)
    y16 = torch.randint(0, 19, (2 * B, H, W), generator=g).to(DEV)

    def model():
        torch.manual_seed(0)
        return tssa.set_compute_dtype(FS.fastscnn(3, 19).to(DEV), torch.bfloat16)

    m = model()
    opt = E.FlatAdamW(m.parameters(), lr=1e-4)
    ema = E.ModelEMA(m, opt, 0.99)
    tr = E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=255), use_graph=True, ema=ema)
    st = tssa.SelfTraining(tr, ema.module, 19, threshold=0.5, mix='classmix')
    with torch.no_grad(), E.EvalPrep(ema.module):           # the median confidence of the initial teacher: about half is kept
        low0 = ops.materialize(ema.module.forward_lowres(x16[B:].contiguous()))
    st.set_threshold(float(tssa.upsample_pseudo_labels(low0, 0.0, size=(H, W), want_confidence=True)[1].median()))
    mp = model()
    optp = E.FlatAdamW(mp.parameters(), lr=1e-4)
    trp = E.Trainer(mp, optp, tssa.CrossEntropyLoss(ignore_index=255), use_graph=True, ema=E.ModelEMA(mp, optp, 0.99))
    teacher = E.GraphedInference(model().eval(), lowres=True, frozen_weights=False)
    xu = x16[B:].contiguous()
    steps = {'selftrain_step_8_plus_8': lambda: st.step(x16[:B], y16[:B], xu),
             'plain_step_16': lambda: trp.step_async(x16, y16),
             'teacher_forward_8': lambda: teacher(xu)}
    res = alternate(steps, a.window_ms, a.rounds)
    res['kept_share_last_step'] = round(float(st.last_kept.sum()) / (B * H * W), 4)
    res['selftrain_minus_plain_ms'] = round(res['selftrain_step_8_plus_8']['ms'] - res['plain_step_16']['ms'], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window-ms', type=float, default=200.0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--skip-step', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/selftrain_time.py needs a GPU: nothing is timed without one')
    out = {'tool': 'tools/selftrain_time.py', 'device': torch.cuda.get_device_name(0), 'window_ms': a.window_ms, 'rounds': a.rounds,
           'what': 'ms per call: device events around a window of back-to-back calls, the candidates of a group alternating, median of the '
                   'rounds; peak_bytes_added = max_memory_allocated over one call minus what was allocated before it',
           'pseudo_8x19x128x256_to_1024x2048': {'bf16': pseudo_group(torch.bfloat16, a), 'f32': pseudo_group(torch.float32, a)},
           'mix_8x3x1024x2048_f32': mix_group(a)}
    if not a.skip_step:
        out['step_fastscnn_bf16_3x512x768'] = step_group(a)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
