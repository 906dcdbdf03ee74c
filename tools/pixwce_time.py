"""Times of per-pixel loss weights on the fused head (csrc/pixwce.hip) next to the plain fused loss and to stock PyTorch, on the same GPU.
Prints one JSON line and writes it to --out (profiles/pixwce_time.json); a part that is skipped keeps what the file already holds.

    python tools/pixwce_time.py [--window-ms 200] [--rounds 5] [--skip-head] [--skip-step] [--out profiles/pixwce_time.json]

  head      forward + backward of head + loss at 16 x 19 x 64 x 96 -> 512 x 768, 8 x 19 x 128 x 256 -> 1024 x 2048 and
            8 x 66 x 64 x 96 -> 512 x 768 (the class-chunked route), bf16 and f32:
              plain       tssa.upsample_cross_entropy without a map: the floor (8 instead of 12 bytes per output pixel)
              pixw        tssa.upsample_pixel_weighted_cross_entropy (a float32 map, multiples of 1/8 in [0, 2]), pixel_norm='weight'
              stock       (F.cross_entropy(F.interpolate(low, size, bilinear, align_corners=True), t, reduction='none') * w).sum() / w.sum()
                          on stock PyTorch (w zeroed on the ignored pixels), with its peak memory over the resident tensors
  step      one captured self-training step (8 labelled + 8 unlabelled at 3 x 512 x 768, FastSCNN bf16, ClassMix) with
            pixel_weighting=None and with pixel_weighting='confidence'

Method: every window runs in a FRESH process (this file with --child): the side is warmed up, a probe sizes the window to about
--window-ms of back-to-back calls between two device events, and the window's ms per call is the child's answer.  The sides of a
group take turns for --rounds rounds; the figure is the median of a side's rounds, and all rounds are kept.  A child that fails ends
the run: nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_SIDES = ('plain', 'pixw', 'stock')
STEP_SIDES = ('selftrain_step', 'selftrain_step_confidence')
SHAPES = {'16x19x64x96_to_512x768': (16, 19, 64, 96, 512, 768), '8x19x128x256_to_1024x2048': (8, 19, 128, 256, 1024, 2048),
          '8x66x64x96_to_512x768': (8, 66, 64, 96, 512, 768)}
DEV = 'cuda:0'


def window(step, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def one_window(step, window_ms):
    window(step, 3)                                         # warm-up
    iters = max(3, int(window_ms / max(window(step, 5), 1e-4)))
    return {'ms': window(step, iters), 'calls': iters}


def head_step(side, dtype, shape):
    import torch
    import torch.nn.functional as F
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    B, C, h, w, H, W = SHAPES[shape]
    g = torch.Generator(device=DEV).manual_seed(0)
    low = (torch.randn(B, C, h, w, device=DEV, generator=g) * 3).to(dtype)
    t = torch.randint(0, C, (B, H, W), device=DEV, generator=g)
    t[torch.rand(B, H, W, device=DEV, generator=g) < 0.05] = 255
    om = torch.randint(0, 17, (B, H, W), device=DEV, generator=g).float() / 8
    one = torch.ones((), dtype=torch.float32, device=DEV)
    if side == 'stock':
        a = low.clone().requires_grad_(True)
        wv = om * (t != 255)

        def stock():
            a.grad = None
            z = F.interpolate(a, size=(H, W), mode='bilinear', align_corners=True)
            ((F.cross_entropy(z, t, ignore_index=255, reduction='none') * wv).sum() / wv.sum()).backward(one)
        return stock
    a = ops.to_nhwc(low).requires_grad_(True)

    def plain():
        a.grad = None
        tssa.upsample_cross_entropy(a, t, size=(H, W), ignore_index=255).backward(one)

    def pixw():
        a.grad = None
        tssa.upsample_pixel_weighted_cross_entropy(a, t, om, size=(H, W), ignore_index=255).backward(one)

    return {'plain': plain, 'pixw': pixw}[side]


def selftrain_step(side):
    import importlib
    import torch
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E, ops
    FS = importlib.import_module('torch_semantic_segmentation_amd.models.fastscnn')
    B, H, W = 8, 512, 768
    g = torch.Generator().manual_seed(3)
    x16 = torch.randn(2 * B, 3, H, W, generator=g).to(DEV)
    y16 = torch.randint(0, 19, (2 * B, H, W), generator=g).to(DEV)
    torch.manual_seed(0)
    m = tssa.set_compute_dtype(FS.fastscnn(3, 19).to(DEV), torch.bfloat16)
    opt = E.FlatAdamW(m.parameters(), lr=1e-4)
    ema = E.ModelEMA(m, opt, 0.99)
    tr = E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=255), use_graph=True, ema=ema)
    st = tssa.SelfTraining(tr, ema.module, 19, threshold=0.5, mix='classmix',
                           pixel_weighting='confidence' if side == 'selftrain_step_confidence' else None)
    xu = x16[B:].contiguous()
    with torch.no_grad(), E.EvalPrep(ema.module):           # the median confidence of the initial teacher: about half is kept
        low0 = ops.materialize(ema.module.forward_lowres(xu))
    st.set_threshold(float(tssa.upsample_pseudo_labels(low0, 0.0, size=(H, W), want_confidence=True)[1].median()))
    return lambda: st.step(x16[:B], y16[:B], xu)


def child(a):
    import torch
    sys.path.insert(0, ROOT)
    if not torch.cuda.is_available():
        raise SystemExit('tools/pixwce_time.py needs a GPU: nothing is timed without one')
    if a.child in HEAD_SIDES:
        step = head_step(a.child, torch.bfloat16 if a.dtype == 'bf16' else torch.float32, a.shape)
    else:
        step = selftrain_step(a.child)
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = one_window(step, a.window_ms)
    res['peak_mb_over_resident'] = round((torch.cuda.max_memory_allocated() - resident) / 2.0 ** 20, 1)
    res['device'] = torch.cuda.get_device_name(0)
    print('PIXWCE_TIME ' + json.dumps(res))


def run_child(side, dtype, shape, a):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', side, '--dtype', dtype, '--shape', shape, '--window-ms', str(a.window_ms)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise SystemExit('child %s %s %s failed (%s); nothing more is started\n%s\n%s' % (side, dtype, shape, p.returncode, p.stdout[-2000:],
                                                                                        p.stderr[-4000:]))
    line = [l for l in p.stdout.splitlines() if l.startswith('PIXWCE_TIME ')][-1]
    return json.loads(line[len('PIXWCE_TIME '):])


def alternate(sides, dtype, shape, a, device):
    got = {s: [] for s in sides}
    last = {}
    for _ in range(a.rounds):
        for s in sides:
            r = run_child(s, dtype, shape, a)
            got[s].append(r['ms'])
            last[s] = r
            device[0] = r['device']
    return {s: {'ms': round(statistics.median(v), 4), 'rounds_ms': [round(t, 4) for t in v], 'calls_per_window': last[s]['calls'],
                'peak_mb_over_resident': last[s]['peak_mb_over_resident']} for s, v in got.items()}


def ratio_range(num, den):
    """the ratio of the medians and the range the rounds span: [min(num) / max(den), max(num) / min(den)]"""
    return {'median': round(num['ms'] / den['ms'], 3),
            'range': [round(min(num['rounds_ms']) / max(den['rounds_ms']), 3), round(max(num['rounds_ms']) / min(den['rounds_ms']), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window-ms', type=float, default=200.0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--skip-head', action='store_true')
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pixwce_time.json'))
    ap.add_argument('--child', default=None, choices=HEAD_SIDES + STEP_SIDES)
    ap.add_argument('--dtype', default='bf16', choices=('bf16', 'f32'))
    ap.add_argument('--shape', default='16x19x64x96_to_512x768', choices=tuple(SHAPES))
    ap.add_argument('--child-timeout', type=float, default=180.0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    device = [None]
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.loads(f.read())
    out.update({'tool': 'tools/pixwce_time.py', 'window_ms': a.window_ms, 'rounds': a.rounds,
                'what': 'ms per call (forward + backward, or one captured step): device events around a window of back-to-back calls, '
                        'every window in a fresh process, the sides of a group alternating, median of the rounds; peak_mb_over_resident: '
                        'torch.cuda.max_memory_allocated over the window minus what the inputs hold'})

    def save():                       # after every group: a run that is cut short keeps what it measured
        out['device'] = device[0] or out.get('device')
        with open(a.out, 'w') as f:
            f.write(json.dumps(out) + '\n')

    if not a.skip_head:
        for shape in SHAPES:
            head = {}
            for dtype in ('bf16', 'f32'):
                res = alternate(HEAD_SIDES, dtype, shape, a, device)
                res['pixw_over_plain'] = ratio_range(res['pixw'], res['plain'])
                res['stock_over_pixw'] = ratio_range(res['stock'], res['pixw'])
                head[dtype] = res
                out['head_' + shape] = head
                save()
    if not a.skip_step:
        res = alternate(STEP_SIDES, 'bf16', '16x19x64x96_to_512x768', a, device)
        res['confidence_minus_none_ms'] = round(res['selftrain_step_confidence']['ms'] - res['selftrain_step']['ms'], 4)
        res['confidence_over_none'] = ratio_range(res['selftrain_step_confidence'], res['selftrain_step'])
        out['step_fastscnn_bf16_8_plus_8_3x512x768'] = res
    save()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
