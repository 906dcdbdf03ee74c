"""Times of per-sample loss groups on the fused head (csrc/groupce.hip) next to what they replace, on the same GPU.  Prints one JSON
line and writes it to --out (profiles/groupce_time.json).

    python tools/groupce_time.py [--window-ms 200] [--rounds 5] [--skip-step] [--out profiles/groupce_time.json]

  head      forward + backward of head + loss at 16 x 19 x 64 x 96 -> 512 x 768, bf16 and f32:
              ungrouped   tssa.upsample_cross_entropy, one mean over the 16 samples
              grouped     the same call with two groups of 8 (weights 1 and 0.5): one head pass, the grouped finalize, the gather
                          that reads its scale per sample
              two_calls   the only way to L_sup + 0.5 L_unsup without groups: the ungrouped operator on each half, their weighted
                          sum, and autograd's add of the two gradients into the one map
  step      one captured self-training step (8 labelled + 8 unlabelled at 3 x 512 x 768, FastSCNN bf16, ClassMix) with
            unsup_weight=None and with unsup_weight=0.5

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
HEAD_SIDES = ('ungrouped', 'grouped', 'two_calls')
STEP_SIDES = ('selftrain_step', 'selftrain_step_unsup_weight')
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


def head_step(side, dtype):
    import torch
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    B, C, h, w, H, W = 16, 19, 64, 96, 512, 768
    g = torch.Generator(device=DEV).manual_seed(0)
    a = ops.to_nhwc((torch.randn(B, C, h, w, device=DEV, generator=g) * 3).to(dtype)).requires_grad_(True)
    t = torch.randint(0, C, (B, H, W), device=DEV, generator=g)
    t[torch.rand(B, H, W, device=DEV, generator=g) < 0.05] = 255
    t1, t2 = t[:B // 2].contiguous(), t[B // 2:].contiguous()
    one = torch.ones((), dtype=torch.float32, device=DEV)
    group = torch.tensor([0] * (B // 2) + [1] * (B // 2), dtype=torch.int32, device=DEV)
    weight = torch.tensor([1.0] * (B // 2) + [0.5] * (B // 2), dtype=torch.float32, device=DEV)
    terms = torch.zeros(B, dtype=torch.float32, device=DEV)

    def ungrouped():
        a.grad = None
        tssa.upsample_cross_entropy(a, t, size=(H, W), ignore_index=255).backward(one)

    def grouped():
        a.grad = None
        tssa.upsample_cross_entropy(a, t, size=(H, W), ignore_index=255, sample_group=group, sample_weight=weight,
                                    group_loss_out=terms).backward(one)

    def two_calls():
        a.grad = None
        l1 = tssa.upsample_cross_entropy(a[:B // 2], t1, size=(H, W), ignore_index=255)
        l2 = tssa.upsample_cross_entropy(a[B // 2:], t2, size=(H, W), ignore_index=255)
        (l1 + 0.5 * l2).backward(one)

    return {'ungrouped': ungrouped, 'grouped': grouped, 'two_calls': two_calls}[side]


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
    st = tssa.SelfTraining(tr, ema.module, 19, threshold=0.5, mix='classmix', unsup_weight=0.5 if side == 'selftrain_step_unsup_weight' else None)
    xu = x16[B:].contiguous()
    with torch.no_grad(), E.EvalPrep(ema.module):           # the median confidence of the initial teacher: about half is kept
        low0 = ops.materialize(ema.module.forward_lowres(xu))
    st.set_threshold(float(tssa.upsample_pseudo_labels(low0, 0.0, size=(H, W), want_confidence=True)[1].median()))
    return lambda: st.step(x16[:B], y16[:B], xu)


def child(a):
    import torch
    sys.path.insert(0, ROOT)
    if not torch.cuda.is_available():
        raise SystemExit('tools/groupce_time.py needs a GPU: nothing is timed without one')
    if a.child in HEAD_SIDES:
        step = head_step(a.child, torch.bfloat16 if a.dtype == 'bf16' else torch.float32)
    else:
        step = selftrain_step(a.child)
    res = one_window(step, a.window_ms)
    res['device'] = torch.cuda.get_device_name(0)
    print('GROUPCE_TIME ' + json.dumps(res))


def run_child(side, dtype, a):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', side, '--dtype', dtype, '--window-ms', str(a.window_ms)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise SystemExit('child %s %s failed (%s); nothing more is started\n%s\n%s' % (side, dtype, p.returncode, p.stdout[-2000:], p.stderr[-4000:]))
    line = [l for l in p.stdout.splitlines() if l.startswith('GROUPCE_TIME ')][-1]
    return json.loads(line[len('GROUPCE_TIME '):])


def alternate(sides, dtype, a, device):
    got = {s: [] for s in sides}
    calls = {}
    for _ in range(a.rounds):
        for s in sides:
            r = run_child(s, dtype, a)
            got[s].append(r['ms'])
            calls[s] = r['calls']
            device[0] = r['device']
    return {s: {'ms': round(statistics.median(v), 4), 'rounds_ms': [round(t, 4) for t in v], 'calls_per_window': calls[s]} for s, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window-ms', type=float, default=200.0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'groupce_time.json'))
    ap.add_argument('--child', default=None, choices=HEAD_SIDES + STEP_SIDES)
    ap.add_argument('--dtype', default='bf16', choices=('bf16', 'f32'))
    ap.add_argument('--child-timeout', type=float, default=180.0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    device = [None]
    out = {'tool': 'tools/groupce_time.py', 'window_ms': a.window_ms, 'rounds': a.rounds,
           'what': 'ms per call (forward + backward, or one captured step): device events around a window of back-to-back calls, every '
                   'window in a fresh process, the sides of a group alternating, median of the rounds'}
    head = {}
    for dtype in ('bf16', 'f32'):
        res = alternate(HEAD_SIDES, dtype, a, device)
        res['grouped_over_ungrouped'] = round(res['grouped']['ms'] / res['ungrouped']['ms'], 3)
        res['two_calls_over_grouped'] = round(res['two_calls']['ms'] / res['grouped']['ms'], 3)
        head[dtype] = res
    out['head_16x19x64x96_to_512x768'] = head
    if not a.skip_step:
        res = alternate(STEP_SIDES, 'bf16', a, device)
        res['unsup_weight_minus_none_ms'] = round(res['selftrain_step_unsup_weight']['ms'] - res['selftrain_step']['ms'], 4)
        out['step_fastscnn_bf16_8_plus_8_3x512x768'] = res
    out['device'] = device[0]
    text = json.dumps(out)
    print(text)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
