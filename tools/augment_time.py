"""Time of tssa.augment_batch (csrc/augment.hip: random scale + crop + flip + Normalize + ToTensor of a uint8 batch in one gather
kernel) at the recipe's shape, next to two baselines on the same GPU: (a) tss_decode_batch_u8 at the same OUTPUT size (Normalize +
ToTensor only: the floor for writing that output), and (b) the same transform restated on stock PyTorch on the device, per sample:
F.interpolate (bilinear for the image, nearest for the labels) of the whole frame, slice, flip, normalize.
Writes one JSON file (default profiles/augment_time.json) and prints it.

    python tools/augment_time.py [--source 1024 2048] [--crop 512 768] [--batch 8] [--iters 20] [--rounds 5] [--out FILE]
    python tools/augment_time.py --hsv       # the plain entry next to tss_augment_batch_u8_ex -> profiles/augment_hsv_time.json

--hsv times, on the same batch and rows: the plain entry; the _ex entry with both pointers NULL (the same work through the other
instantiation), with the label table alone, with HueSaturationValue on EVERY sample alone, and with both (the headline:
hsv_lut_over_plain).

Every candidate is warmed up, then timed with device events over `iters` calls; the candidates are visited `rounds` times in turn
(alternating, so drift hits all of them alike); the per-round times are all reported, the median is the headline.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_semantic_segmentation_amd as tssa  # noqa: E402
from torch_semantic_segmentation_amd import _native as N  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def stock_augment(image_hwc, target, rows, crop, mean, std):
    """The same transform on stock PyTorch device ops, one sample at a time (each has its own scaled size)."""
    ch, cw = crop
    xs, ys = [], []
    for b, (Hs, Ws, oy, ox, flip, _) in enumerate(rows):
        x = image_hwc[b].permute(2, 0, 1).unsqueeze(0).float()
        x = F.interpolate(x, size=(Hs, Ws), mode='bilinear', align_corners=False)[0, :, oy:oy + ch, ox:ox + cw]
        y = F.interpolate(target[b][None, None].float(), size=(Hs, Ws), mode='nearest')[0, 0, oy:oy + ch, ox:ox + cw].long()
        if flip:
            x, y = x.flip(-1), y.flip(-1)
        xs.append((x / 255.0 - mean) / std)
        ys.append(y)
    return torch.stack(xs), torch.stack(ys)


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
    ap.add_argument('--source', type=int, nargs=2, default=[1024, 2048])
    ap.add_argument('--crop', type=int, nargs=2, default=[512, 768])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--skip-stock', action='store_true')
    ap.add_argument('--hsv', action='store_true', help='time tss_augment_batch_u8_ex (HSV on every sample + label table) next to the plain entry')
    ap.add_argument('--commit', default=None, help='recorded in the file (default: git rev-parse of the checkout, if it is one)')
    ap.add_argument('--out', default=None, help='default profiles/augment_time.json, with --hsv profiles/augment_hsv_time.json')
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, 'profiles', 'augment_hsv_time.json' if a.hsv else 'augment_time.json')
    B, (H, W), (ch, cw) = a.batch, a.source, a.crop
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(0)
    image = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    target = torch.randint(0, 19, (B, H, W), generator=g, dtype=torch.uint8).to(dev)
    aug = tssa.TrainAugment((ch, cw), scale_range=(0.5, 2.0), mean=MEAN, std=STD)
    rows = aug.draw(B, (H, W), generator=g)
    params = rows.to(dev)
    out = (torch.empty((B, 3, ch, cw), dtype=torch.float32, device=dev), torch.empty((B, ch, cw), dtype=torch.int64, device=dev))
    crop_u8 = (image[:, :ch, :cw].contiguous(), target[:, :ch, :cw].contiguous())
    mean3, std3 = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    mean_t, std_t = torch.tensor(MEAN, device=dev).view(3, 1, 1), torch.tensor(STD, device=dev).view(3, 1, 1)
    row_list = rows.tolist()

    def hip_augment():
        N.call('tss_augment_batch_u8', N.ptr(image), 1, mean3, std3, N.ptr(out[0]), N.ptr(target), N.ptr(out[1]), N.ptr(params),
               B, 3, H, W, ch, cw, N.stream())

    def hip_decode():
        N.call('tss_decode_batch_u8', N.ptr(crop_u8[0]), 1, mean3, std3, N.ptr(out[0]), N.ptr(crop_u8[1]), N.ptr(out[1]),
               B, 3, ch * cw, N.stream())

    color = tssa.TrainAugment((ch, cw), hsv_p=1.0).draw_color(B, generator=g)
    lut = torch.randint(0, 20, (256,), generator=g).to(torch.uint8)
    color_dev, lut_dev = color.to(dev), lut.to(dev)

    def hip_augment_ex(color_rows, table):
        def run():
            N.call('tss_augment_batch_u8_ex', N.ptr(image), 1, mean3, std3, N.ptr(out[0]), N.ptr(target), N.ptr(out[1]), N.ptr(params),
                   N.ptr(color_rows), N.ptr(table), B, 3, H, W, ch, cw, N.stream())
        return run

    cands = [('hip_augment', hip_augment), ('hip_decode_same_output', hip_decode)]
    if a.hsv:
        cands = [('hip_augment', hip_augment), ('hip_augment_ex_null', hip_augment_ex(None, None)),
                 ('hip_augment_ex_lut', hip_augment_ex(None, lut_dev)), ('hip_augment_ex_hsv', hip_augment_ex(color_dev, None)),
                 ('hip_augment_ex_hsv_lut', hip_augment_ex(color_dev, lut_dev))]
    elif not a.skip_stock:
        cands.append(('stock_interpolate_slice_flip_normalize', lambda: stock_augment(image, target, row_list, (ch, cw), mean_t, std_t)))
    for _name, fn in cands:                                # warm-up: code objects, allocator blocks
        one_round(fn, 2)
    us = {name: [] for name, _ in cands}
    for _ in range(a.rounds):
        for name, fn in cands:
            us[name].append(round(one_round(fn, a.iters), 2))
    # bytes the algorithm needs: the outputs in full (f32 image planes + int64 labels); of the source, the texels under the crop
    # windows (each window covers crop / scale source pixels per axis), once
    out_bytes = B * ch * cw * (3 * 4 + 8)
    src_px = sum((ch * H / Hs) * (cw * W / Ws) for Hs, Ws, *_ in row_list)
    need = out_bytes + src_px * (3 + 1)
    res = {'tool': 'tools/augment_time.py', 'device': torch.cuda.get_device_name(0), 'commit': a.commit or commit(),
           'source': [B, H, W, 3], 'crop': [ch, cw], 'rows': row_list, 'iters': a.iters, 'rounds': a.rounds,
           'what': 'device events around iters calls, microseconds per call for every round; GB/s = algorithmic bytes '
                   '(outputs in full + source texels under the crop windows once) over the median',
           'output_bytes': out_bytes, 'algorithmic_bytes': int(need)}
    for name, _ in cands:
        med = sorted(us[name])[len(us[name]) // 2]
        res[name] = {'us_rounds': us[name], 'us_median': med}
    res['hip_augment']['GBps'] = round(need / res['hip_augment']['us_median'] / 1e3, 1)
    if a.hsv:
        res['color_rows'] = color.tolist()
        for name, _ in cands[1:]:
            res[name.replace('hip_augment_ex_', '') + '_over_plain'] = round(res[name]['us_median'] / res['hip_augment']['us_median'], 3)
    else:
        res['hip_decode_same_output']['GBps'] = round((out_bytes + B * ch * cw * 4) / res['hip_decode_same_output']['us_median'] / 1e3, 1)
        res['augment_over_decode'] = round(res['hip_augment']['us_median'] / res['hip_decode_same_output']['us_median'], 2)
    if not a.skip_stock and not a.hsv:
        res['stock_over_augment'] = round(res['stock_interpolate_slice_flip_normalize']['us_median'] / res['hip_augment']['us_median'], 2)
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
