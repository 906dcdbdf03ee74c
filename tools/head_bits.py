"""SHA-256 of everything the fused decoder head returns, on seeded inputs: the check that a change of csrc/loss.hip, softhead.hip,
widehead.hip, msflip.hip or headgeom.h computes the same BITS as the build before it.

Every head entry point of ops.py runs in float32 and bfloat16 on the small cases below (register path, both class-register variants,
an output that is no multiple of the map, the wide path with more than one strip), and once at the benchmark's size in bfloat16; the
loss, the low-resolution gradient, the per-pixel cross-entropy, the prediction and the confusion matrix are hashed one by one.

    python tools/head_bits.py --out profiles/head_bits_change.json
    TSS_HIP_LIB=/path/to/the/other/libtss_hip.so python tools/head_bits.py --out profiles/head_bits_parent.json

Run the two in fresh processes (TSS_HIP_LIB is read when the package is imported) and compare the files: they must be equal key for key.
"""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_semantic_segmentation_amd import ops  # noqa: E402
from torch_semantic_segmentation_amd import _native as N  # noqa: E402

DEV = 'cuda:0'
# (B, C, h, w) -> (H, W)
SMALL = [((2, 19, 8, 16), (64, 128)), ((1, 21, 6, 9), (24, 36)), ((1, 19, 15, 29), (16, 32)), ((2, 33, 8, 16), (32, 64)),
         ((1, 150, 5, 40), (40, 320))]
BENCH = ((8, 19, 128, 256), (1024, 2048))
VALUES = {}                   # the losses as numbers, printed with --values


def sha(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def inputs(shape, size, dtype):
    B, C, h, w = shape
    g = torch.Generator().manual_seed(1234 + C * 7 + h)
    low = (2.0 * torch.randn(B, C, h, w, generator=g)).to(DEV).to(dtype)
    y = torch.randint(0, C, (B,) + tuple(size), generator=g)
    y[torch.rand(y.shape, generator=g) < 0.05] = 255
    cw = (0.5 + torch.rand(C, generator=g)).to(DEV)
    return low, y.to(DEV), cw


def loss_and_grad(out, key, fn, low):
    a = ops.to_nhwc(low).detach().requires_grad_(True)
    loss = fn(a)
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(a.grad).all()), key      # two NaNs would hash alike
    out[key + '/loss'] = sha(loss)
    VALUES[key + '/loss'] = float(loss)
    out[key + '/grad'] = sha(a.grad)


def pixel_ce(low, y, size):
    a = ops.to_nhwc(low)
    B, C, h, w = a.shape
    pix = torch.empty((B,) + tuple(size), dtype=torch.float32, device=a.device)
    N.call('tss_upsample_pixel_ce' + ops._wide(C), N.ptr(a), ops.ld(a), N.ptr(y), N.ptr(pix), B, C, h, w, size[0], size[1], 255,
           N.dtype_code(a.dtype), N.stream())
    return pix


def run_case(out, shape, size, dtype, name):
    low, y, cw = inputs(shape, size, dtype)
    C = shape[1]
    k = '%s/%s' % (name, 'bf16' if dtype == torch.bfloat16 else 'f32')
    ce = ops.upsample_cross_entropy
    loss_and_grad(out, k + '/ce', lambda a: ce(a, y, size=size, ignore_index=255), low)
    loss_and_grad(out, k + '/ce_weighted', lambda a: ce(a, y, size=size, ignore_index=255, weight=cw), low)
    loss_and_grad(out, k + '/ce_smoothed', lambda a: ce(a, y, size=size, ignore_index=255, weight=cw, label_smoothing=0.1), low)
    loss_and_grad(out, k + '/ohem', lambda a: ops.upsample_ohem_loss(a, y, size=size, ignore_index=255), low)
    out[k + '/pixel_ce'] = sha(pixel_ce(low, y, size))
    for variant in ('reference', 'lin'):
        loss_and_grad(out, k + '/focal_' + variant,
                      lambda a: ops.upsample_focal_loss(a, y, size=size, ignore_index=255, variant=variant), low)
    loss_and_grad(out, k + '/dice', lambda a: ops.upsample_dice_loss(a, y, C, size=size, ignore_index=255), low)
    pred, cm = ops.upsample_argmax_confusion(low, y, size=size, ignore_index=255)
    out[k + '/argmax/pred'] = sha(pred)
    out[k + '/argmax/confusion'] = sha(cm)
    low2 = torch.cat([low, low.flip(-1) * 0.5 + 0.25], 0)          # the plain and the "mirrored" half of one forward
    B, _, h, w = shape
    g = torch.Generator().manual_seed(99)
    small = (2.0 * torch.randn(B, C, max(1, h // 2), max(1, w // 2), generator=g)).to(DEV).to(dtype)
    for average in ('softmax', 'logits'):
        pred, cm = ops.multiscale_argmax_confusion([low2, small], [(False, True), False], y, size=size, ignore_index=255, average=average)
        out[k + '/multiscale_' + average + '/pred'] = sha(pred)
        out[k + '/multiscale_' + average + '/confusion'] = sha(cm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--no-bench-size', action='store_true')
    ap.add_argument('--values', action='store_true', help='print every loss value')
    a = ap.parse_args()
    out = {}
    for shape, size in SMALL:
        for dtype in (torch.float32, torch.bfloat16):
            run_case(out, shape, size, dtype, '%dx%dx%dx%d_to_%dx%d' % (shape + size))
    if not a.no_bench_size:
        run_case(out, BENCH[0], BENCH[1], torch.bfloat16, '%dx%dx%dx%d_to_%dx%d' % (BENCH[0] + BENCH[1]))
    torch.cuda.synchronize()
    if a.values:
        for k in sorted(VALUES):
            print('%-60s %r' % (k, VALUES[k]))
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d hashes -> %s (library: %s)' % (len(out), a.out, N.LIB_PATH))


if __name__ == '__main__':
    main()
