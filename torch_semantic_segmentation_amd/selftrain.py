"""Mean-teacher self-training on unlabelled frames (Mean Teacher / CutMix-Seg / ClassMix / DACS): pseudo-labels straight from the
teacher's low-resolution logits (csrc/pseudo.hip), the ClassMix / CutMix perturbation on the device (csrc/mix.hip), and SelfTraining,
which runs both as the captured prologue of an ordinary engine.Trainer step.

None of the functions here has an ATen fall-back: a shape outside a kernel's contract is a ValueError."""
import numpy as np
import torch

from . import _native as N
from . import ops

call, ptr, stream = N.call, N.ptr, N.stream

_THRESHOLDS = {}        # (device, value) -> 1-float device tensor: the threshold is read by the kernel, like CrossEntropyLoss's weights


def _threshold_tensor(threshold, dev):
    if isinstance(threshold, torch.Tensor):
        if threshold.dtype != torch.float32 or threshold.numel() != 1:
            raise ValueError('threshold tensor must hold one float32, got %s %s' % (threshold.dtype, tuple(threshold.shape)))
        ops._check_device(threshold)
        return threshold
    key = (str(dev), float(threshold))
    if key not in _THRESHOLDS:
        _THRESHOLDS[key] = torch.tensor([float(threshold)], dtype=torch.float32, device=dev)
    return _THRESHOLDS[key]


def upsample_pseudo_labels(low, threshold, scale_factor=None, size=None, ignore_index=255, want_confidence=False, kept=None, out=None,
                           out_confidence=None):
    """Pseudo-labels of F.interpolate(low, bilinear, align_corners=True) without the full-resolution logits
    (tss_upsample_pseudo_label[_wide]): per pixel the arg-max class (lowest index wins ties) where its softmax probability reaches
    `threshold`, `ignore_index` elsewhere.  low: the NHWC map of forward_lowres, read in place, or an NCHW tensor; threshold: a float
    (kept in a cached device scalar) or a one-element float32 device tensor, read by the kernel -- a captured step follows its value.
    Returns (labels uint8 [B,H,W], confidence float32 [B,H,W] or None, kept int64 [B]): confidence is written for every pixel; kept
    counts the labels kept per sample and is zero-filled here unless the caller passes a tensor of their own to accumulate into.
    `out`: a uint8 [B,H,W] tensor to write the labels into; `out_confidence`: a float32 [B,H,W] tensor to write the confidence into
    (it implies want_confidence).  Up to 24 classes the scores of a pixel live in registers, up to 255
    the class-chunked kernel runs.  ValueError: more than 255 classes, ignore_index outside [C, 255] (the label is a byte and must
    not collide with a class), an output smaller than the map."""
    low = ops.to_nhwc(ops.materialize(low))
    ops._check_device(low)
    ho, wo = ops._out_size(low, size, scale_factor)
    B, C, h, w = low.shape
    if C > 255:
        raise ValueError('upsample_pseudo_labels supports at most 255 classes (the label is a byte), got %d' % C)
    if not C <= int(ignore_index) <= 255:
        raise ValueError('ignore_index must lie in [%d, 255] (a byte that is no class), got %r' % (C, ignore_index))
    if ho < h or wo < w:
        raise ValueError('the output %dx%d is smaller than the map %dx%d (logits are upsampled, never reduced)' % (ho, wo, h, w))
    dev = low.device
    thr = _threshold_tensor(threshold, dev)
    if out is None:
        out = torch.empty((B, ho, wo), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, ho, wo) or not out.is_contiguous() or out.device != dev:
        raise ValueError('out must be a contiguous uint8 tensor of shape %s on %s' % ((B, ho, wo), dev))
    if out_confidence is not None:
        conf = out_confidence
        if conf.dtype != torch.float32 or tuple(conf.shape) != (B, ho, wo) or not conf.is_contiguous() or conf.device != dev:
            raise ValueError('out_confidence must be a contiguous float32 tensor of shape %s on %s' % ((B, ho, wo), dev))
    else:
        conf = torch.empty((B, ho, wo), dtype=torch.float32, device=dev) if want_confidence else None
    if kept is None:
        kept = torch.zeros(B, dtype=torch.int64, device=dev)
    elif kept.dtype != torch.int64 or tuple(kept.shape) != (B,) or not kept.is_contiguous() or kept.device != dev:
        raise ValueError('kept must be a contiguous int64 tensor of shape (%d,) on %s' % (B, dev))
    call('tss_upsample_pseudo_label' + ops._wide(C), ptr(low), ops.ld(low), ptr(thr), ptr(out), ptr(conf), ptr(kept), B, C, h, w, ho, wo,
         int(ignore_index), N.dtype_code(low.dtype), stream())
    return out, conf, kept


def _rows(t, name, shape, lo, hi, dev):
    """A row tensor for the device: a device int32 tensor is taken as it is; a host tensor / array is validated (integer dtype,
    shape, lo <= value < hi) and copied."""
    if isinstance(t, torch.Tensor) and t.is_cuda:
        if t.dtype != torch.int32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError('%s on the device must be a contiguous int32 tensor of shape %s' % (name, tuple(shape)))
        return t
    a = t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if a.dtype.kind not in 'iu':
        raise ValueError('%s must hold integers, got %s' % (name, a.dtype))
    if tuple(a.shape) != tuple(shape):
        raise ValueError('%s must have shape %s, got %s' % (name, tuple(shape), tuple(a.shape)))
    if a.size and (int(a.min()) < lo or int(a.max()) >= hi):
        raise ValueError('%s must lie in [%d, %d), got [%d, %d]' % (name, lo, hi, int(a.min()), int(a.max())))
    a = a.astype(np.int64).astype(np.uint32).view(np.int32) if hi > 2 ** 31 else a.astype(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def classmix_select(labels, keys, num_classes):
    """ClassMix's class pick on the device (tss_classmix_select): labels uint8 [B,H,W] (or [B,HW]); keys [B,256] random 32-bit
    values drawn by the caller (a host array / tensor of integers in [0, 2^32), validated and copied, or a device int32 tensor
    holding those bits, taken as it is).  Per sample the classes < num_classes that occur (larger bytes, the ignore byte included,
    never count) are ranked by (key, class index), unsigned, and the ceil(n/2) of smallest rank are picked.  Returns sel uint8
    [B,256], 1 for a picked class.  No `unique`, no host synchronisation."""
    ops._check_device(labels)
    if labels.dtype != torch.uint8 or labels.dim() < 2:
        raise ValueError('labels must be a uint8 tensor [B, ...], got %s %s' % (labels.dtype, tuple(labels.shape)))
    if not 1 <= int(num_classes) <= 256:
        raise ValueError('num_classes must lie in [1, 256], got %r' % (num_classes,))
    labels = labels.contiguous()
    B = labels.shape[0]
    keys = _rows(keys, 'keys', (B, 256), 0, 2 ** 32, labels.device)
    sel = torch.empty((B, 256), dtype=torch.uint8, device=labels.device)
    call('tss_classmix_select', ptr(labels), ptr(keys), ptr(sel), B, labels.numel() // max(B, 1), int(num_classes), stream())
    return sel


def mix_batch(image, labels, partner, sel=None, boxes=None, out_image=None, out_target=None):
    """The mixing select of ClassMix (`sel`, from classmix_select) or CutMix (`boxes` [B,4] = y0, x0, y1, x1), one launch
    (tss_mix_batch): with mask = sel[b][labels[b]] or the box,
        out_image[b] = mask ? image[b] : image[partner[b]],    out_target[b] = int64(mask ? labels[b] : labels[partner[b]]).
    A select on bits: the value that is not chosen never reaches the output, the chosen one arrives bit for bit (255 stays 255).
    image [B,Ci,H,W] float32 | bfloat16 with W % 8 == 0, labels uint8 [B,H,W]; partner [B] and boxes as host arrays / tensors
    are validated (0 <= partner < B, 0 <= y <= H, 0 <= x <= W) and copied, as device int32 tensors they are taken as they are (the
    kernel clamps them into range).  Exactly one of sel / boxes.  DACS is the same call on a concatenated batch.
    Returns (out_image, out_target); given outputs must not alias the inputs."""
    ops._check_device(image)
    if (sel is None) == (boxes is None):
        raise ValueError('mix_batch takes exactly one of sel (ClassMix) and boxes (CutMix)')
    if image.dim() != 4 or not image.is_contiguous():
        raise ValueError('image must be a contiguous [B,Ci,H,W] tensor')
    B, Ci, H, W = image.shape
    dev = image.device
    if W % 8:
        raise ValueError('mix_batch needs a width that is a multiple of 8, got %d' % W)
    if labels.dtype != torch.uint8 or tuple(labels.shape) != (B, H, W) or not labels.is_contiguous() or labels.device != dev:
        raise ValueError('labels must be a contiguous uint8 tensor of shape %s on %s' % ((B, H, W), dev))
    partner = _rows(partner, 'partner', (B,), 0, max(B, 1), dev)
    if boxes is not None:
        if not (isinstance(boxes, torch.Tensor) and boxes.is_cuda):
            b = boxes.numpy() if isinstance(boxes, torch.Tensor) else np.asarray(boxes)
            if b.ndim == 2 and b.shape[1] == 4 and b.size and b.dtype.kind in 'iu' and (int(b[:, 0::2].max()) > H or int(b[:, 1::2].max()) > W):
                raise ValueError('boxes must lie inside the %dx%d image' % (H, W))
        boxes = _rows(boxes, 'boxes', (B, 4), 0, max(H, W) + 1, dev)
    else:
        if not (isinstance(sel, torch.Tensor) and sel.dtype == torch.uint8 and tuple(sel.shape) == (B, 256)):
            raise ValueError('sel must be a uint8 tensor of shape (%d, 256)' % B)
        if not sel.is_cuda:
            if int(sel.max()) > 1:
                raise ValueError('sel must hold 0 / 1')
            sel = sel.to(dev)
        sel = sel.contiguous()
    if out_image is None:
        out_image = torch.empty_like(image)
    elif out_image.dtype != image.dtype or tuple(out_image.shape) != (B, Ci, H, W) or not out_image.is_contiguous() or out_image.device != dev:
        raise ValueError('out_image must be a contiguous %s tensor of shape %s on %s' % (image.dtype, (B, Ci, H, W), dev))
    if out_target is None:
        out_target = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    elif out_target.dtype != torch.int64 or tuple(out_target.shape) != (B, H, W) or not out_target.is_contiguous() or out_target.device != dev:
        raise ValueError('out_target must be a contiguous int64 tensor of shape %s on %s' % ((B, H, W), dev))
    if out_image.data_ptr() == image.data_ptr():
        raise ValueError('out_image must not alias image')
    call('tss_mix_batch', ptr(image), ptr(labels), ptr(partner), ptr(sel), ptr(boxes), ptr(out_image), ptr(out_target), B, Ci, H, W,
         N.dtype_code(image.dtype), stream())
    return out_image, out_target


def mix_plane(plane, labels, partner, sel=None, boxes=None, out=None):
    """mix_batch's select on ONE float32 [B,H,W] plane, one launch (tss_mix_plane): with mask = sel[b][labels[b]] or the box,
        out[b] = mask ? plane[b] : plane[partner[b]]
    on bits (the value that is not chosen never reaches the output) -- a confidence map that follows the mixed pseudo-labels, or
    DACS's two-valued source / target map from constant planes.  W % 8 == 0; labels uint8 [B,H,W] (read for `sel` only); partner,
    sel and boxes as for mix_batch (host rows validated and copied, device rows taken as they are and clamped).  Exactly one of
    sel / boxes.  Returns out, which must not alias plane."""
    ops._check_device(plane)
    if (sel is None) == (boxes is None):
        raise ValueError('mix_plane takes exactly one of sel (ClassMix) and boxes (CutMix)')
    if plane.dim() != 3 or plane.dtype != torch.float32 or not plane.is_contiguous():
        raise ValueError('plane must be a contiguous float32 [B,H,W] tensor, got %s %s' % (plane.dtype, tuple(plane.shape)))
    B, H, W = plane.shape
    dev = plane.device
    if W % 8:
        raise ValueError('mix_plane needs a width that is a multiple of 8, got %d' % W)
    if labels.dtype != torch.uint8 or tuple(labels.shape) != (B, H, W) or not labels.is_contiguous() or labels.device != dev:
        raise ValueError('labels must be a contiguous uint8 tensor of shape %s on %s' % ((B, H, W), dev))
    partner = _rows(partner, 'partner', (B,), 0, max(B, 1), dev)
    if boxes is not None:
        if not (isinstance(boxes, torch.Tensor) and boxes.is_cuda):
            b = boxes.numpy() if isinstance(boxes, torch.Tensor) else np.asarray(boxes)
            if b.ndim == 2 and b.shape[1] == 4 and b.size and b.dtype.kind in 'iu' and (int(b[:, 0::2].max()) > H or int(b[:, 1::2].max()) > W):
                raise ValueError('boxes must lie inside the %dx%d image' % (H, W))
        boxes = _rows(boxes, 'boxes', (B, 4), 0, max(H, W) + 1, dev)
    else:
        if not (isinstance(sel, torch.Tensor) and sel.dtype == torch.uint8 and tuple(sel.shape) == (B, 256)):
            raise ValueError('sel must be a uint8 tensor of shape (%d, 256)' % B)
        if not sel.is_cuda:
            if int(sel.max()) > 1:
                raise ValueError('sel must hold 0 / 1')
            sel = sel.to(dev)
        sel = sel.contiguous()
    if out is None:
        out = torch.empty_like(plane)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, H, W) or not out.is_contiguous() or out.device != dev:
        raise ValueError('out must be a contiguous float32 tensor of shape %s on %s' % ((B, H, W), dev))
    if out.data_ptr() == plane.data_ptr() and B:
        raise ValueError('out must not alias plane')
    call('tss_mix_plane', ptr(plane), ptr(labels), ptr(partner), ptr(sel), ptr(boxes), ptr(out), B, H, W, stream())
    return out


STRONG_MAX_RADIUS = 8
STRONG_MAX_SIGMA = 8.0 / 3.0


def gaussian_taps(sigma):
    """(R, taps): the one-sided taps of a normalised Gaussian of standard deviation `sigma`, R = min(ceil(3 sigma), 8),
    w_k = exp(-k^2 / 2 sigma^2) / sum_{j=-R..R} exp(-j^2 / 2 sigma^2) for k = 0..R, computed in float64 and rounded to float32;
    taps is a float32 array of 12 with zeros past R.  sigma = 0 gives R = 0 (no blur, taps (1, 0, ...)).  ValueError for sigma < 0
    or sigma > 8/3 (the kernel's halo is 8 pixels)."""
    s = float(sigma)
    if not 0.0 <= s <= STRONG_MAX_SIGMA:
        raise ValueError('sigma must lie in [0, 8/3], got %r' % (sigma,))
    taps = np.zeros(12, dtype=np.float32)
    if s == 0.0:
        taps[0] = 1.0
        return 0, taps
    R = min(int(np.ceil(3.0 * s)), STRONG_MAX_RADIUS)
    k = np.arange(R + 1, dtype=np.float64)
    e = np.exp(-k * k / (2.0 * s * s))
    taps[:R + 1] = (e / (e[0] + 2.0 * e[1:].sum())).astype(np.float32)
    return R, taps


class StrongAugment:
    """The photometric strong augmentation of the student's unlabelled input (ClassMix, DACS, CutMix-Seg, FixMatch): colour jitter
    with probability `color_p`, then a Gaussian blur with probability `blur_p`, drawn on the host and applied on the device by
    strong_augment (csrc/strongaug.hip; include/tss_hip.h has the formulas).  mean / std: the Normalize constants of the batch
    (None: 0 / 1).  brightness, contrast, saturation = a: the factor is uniform in [max(0, 1 - a), 1 + a]; hue: the shift is uniform
    in [-hue, hue] of a turn (hue <= 0.5); sigma = (lo, hi): the blur's standard deviation, uniform, at most 8/3.

    draw(B, generator) returns the host rows (color float32 [B,8] = (apply, fb, fc, fs, dh, 0, 0, 0), radius int32 [B],
    taps float32 [B,12]); `generator` is a numpy Generator (None: a fresh default_rng()), seven uniform numbers per sample, every
    parameter drawn whether or not its step applies, so the stream does not depend on the outcome.  Labels are not touched."""

    def __init__(self, mean=None, std=None, color_p=0.8, brightness=0.25, contrast=0.25, saturation=0.25, hue=0.25, blur_p=0.5,
                 sigma=(0.15, 1.15)):
        self.mean = None if mean is None else tuple(float(v) for v in mean)
        self.std = None if std is None else tuple(float(v) for v in std)
        for name, v in (('mean', self.mean), ('std', self.std)):
            if v is not None and (len(v) != 3 or not all(np.isfinite(v)) or (name == 'std' and min(v) <= 0.0)):
                raise ValueError('%s must be three finite numbers%s, got %r' % (name, ' > 0' if name == 'std' else '', v))
        self.color_p, self.blur_p = float(color_p), float(blur_p)
        self.brightness, self.contrast, self.saturation, self.hue = float(brightness), float(contrast), float(saturation), float(hue)
        self.sigma = (float(sigma[0]), float(sigma[1]))
        for name in ('color_p', 'blur_p'):
            if not 0.0 <= getattr(self, name) <= 1.0:
                raise ValueError('%s must be a probability, got %r' % (name, getattr(self, name)))
        for name in ('brightness', 'contrast', 'saturation'):
            v = getattr(self, name)
            if not (v >= 0.0 and v != float('inf')):
                raise ValueError('%s must be a finite number >= 0, got %r' % (name, v))
        if not 0.0 <= self.hue <= 0.5:
            raise ValueError('hue must lie in [0, 0.5] of a turn, got %r' % (hue,))
        if not 0.0 <= self.sigma[0] <= self.sigma[1] <= STRONG_MAX_SIGMA:
            raise ValueError('sigma must be 0 <= lo <= hi <= 8/3, got %r' % (sigma,))

    def draw(self, B, generator=None):
        rng = np.random.default_rng() if generator is None else generator
        u = rng.random((int(B), 7))
        color = np.zeros((int(B), 8), dtype=np.float32)
        color[:, 0] = u[:, 0] < self.color_p
        for j, a in enumerate((self.brightness, self.contrast, self.saturation)):
            lo = max(0.0, 1.0 - a)
            color[:, 1 + j] = lo + (1.0 + a - lo) * u[:, 1 + j]
        color[:, 4] = np.clip(self.hue * (2.0 * u[:, 4] - 1.0), -self.hue, self.hue)
        sig = np.where(u[:, 5] < self.blur_p, np.clip(self.sigma[0] + (self.sigma[1] - self.sigma[0]) * u[:, 6], *self.sigma), 0.0)
        radius = np.zeros(int(B), dtype=np.int32)
        taps = np.zeros((int(B), 12), dtype=np.float32)
        for b in range(int(B)):
            radius[b], taps[b] = gaussian_taps(sig[b])
        return color, radius, taps


def _strong_rows(color, radius, taps, B, dev):
    """The three row tensors on the device: device tensors are taken as they are (dtype, shape), host rows are validated, copied."""
    out = []
    for t, name, shape, dtype in ((color, 'color', (B, 8), torch.float32), (radius, 'radius', (B,), torch.int32),
                                  (taps, 'taps', (B, 12), torch.float32)):
        if isinstance(t, torch.Tensor) and t.is_cuda:
            if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                raise ValueError('%s on the device must be a contiguous %s tensor of shape %s on %s' % (name, dtype, shape, dev))
            out.append(t)
            continue
        a = t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        if tuple(a.shape) != shape:
            raise ValueError('%s must have shape %s, got %s' % (name, shape, tuple(a.shape)))
        if name == 'radius':
            if a.dtype.kind not in 'iu' or (a.size and (int(a.min()) < 0 or int(a.max()) > STRONG_MAX_RADIUS)):
                raise ValueError('radius must hold integers in [0, %d], got %s' % (STRONG_MAX_RADIUS, a))
            a = a.astype(np.int32)
        else:
            if a.dtype.kind not in 'fiu':
                raise ValueError('%s must hold numbers, got %s' % (name, a.dtype))
            a = a.astype(np.float32)
            if not np.isfinite(a).all():
                raise ValueError('%s must be finite' % name)
            if name == 'color' and a.size and (float(a[:, 1:4].min()) < 0.0 or float(np.abs(a[:, 4]).max()) > 0.5):
                raise ValueError('color rows need factors >= 0 and |dh| <= 0.5, got %s' % (a,))
        out.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    return out


def strong_augment(image, color, radius, taps, mean=None, std=None, out=None, workspace=None):
    """Colour jitter and Gaussian blur of a normalised batch, two launches (tss_strong_augment; include/tss_hip.h has the formulas,
    StrongAugment.draw / gaussian_taps make the rows).  image [B,3,H,W] float32 | bfloat16, contiguous, W % 8 == 0, W >= 16, H >= 9;
    mean / std: the constants the batch was normalised with (None: 0 / 1).  color [B,8], radius [B], taps [B,12] as host arrays /
    tensors are validated (shapes, 0 <= R <= 8, finite factors >= 0, |dh| <= 0.5) and copied; as device tensors (float32, int32,
    float32) they are taken as they are and the kernel clamps R and dh into range.  A sample with apply = 0 and R = 0 is copied on
    bits.  `out` must not alias `image`; `workspace`: a float64 device tensor of tss_strong_augment_ws bytes to reuse between calls
    (SelfTraining keeps one).  No ATen fall-back: anything outside the contract is a ValueError."""
    ops._check_device(image)
    if image.dim() != 4 or not image.is_contiguous() or image.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError('image must be a contiguous float32 / bfloat16 [B,3,H,W] tensor, got %s %s' % (image.dtype, tuple(image.shape)))
    B, Ci, H, W = image.shape
    if Ci != 3 or W % 8 or W < 16 or H < 9:
        raise ValueError('strong_augment needs 3 channels, a width that is a multiple of 8 and >= 16 and a height >= 9, got %s'
                         % (tuple(image.shape),))
    dev = image.device
    for name, v in (('mean', mean), ('std', std)):
        if v is not None and (len(v) != 3 or not all(np.isfinite([float(x) for x in v])) or (name == 'std' and min(float(x) for x in v) <= 0)):
            raise ValueError('%s must be three finite numbers%s, got %r' % (name, ' > 0' if name == 'std' else '', v))
    color, radius, taps = _strong_rows(color, radius, taps, B, dev)
    if out is None:
        out = torch.empty_like(image)
    elif out.dtype != image.dtype or tuple(out.shape) != (B, Ci, H, W) or not out.is_contiguous() or out.device != dev:
        raise ValueError('out must be a contiguous %s tensor of shape %s on %s' % (image.dtype, (B, Ci, H, W), dev))
    if out.data_ptr() == image.data_ptr() and B:
        raise ValueError('out must not alias image')
    need = N.lib().tss_strong_augment_ws(B, H, W)
    if need < 0:
        raise ValueError('strong_augment: shape %s is outside the kernel\'s contract' % (tuple(image.shape),))
    if workspace is None:
        workspace = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
    elif workspace.dtype != torch.float64 or workspace.numel() * 8 < need or not workspace.is_contiguous() or workspace.device != dev:
        raise ValueError('workspace must be a contiguous float64 tensor of at least %d bytes on %s' % (need, dev))
    call('tss_strong_augment', ptr(image), ptr(out), ptr(color), ptr(radius), ptr(taps), ops._float3(mean, 0.0), ops._float3(std, 1.0),
         ptr(workspace), B, Ci, H, W, N.dtype_code(image.dtype), stream())
    return out


class SelfTraining:
    """Mean-teacher self-training through an existing (captured or eager) engine.Trainer.

        ema = E.ModelEMA(model, optimizer, 0.99)
        trainer = E.Trainer(model, optimizer, tssa.CrossEntropyLoss(ignore_index=255), use_graph=True, ema=ema)
        st = tssa.SelfTraining(trainer, ema.module, num_classes=19, threshold=0.95, mix='classmix')
        loss = st.step(x, y, xu)          # B labelled samples + B unlabelled frames

    Every step the teacher labels the unlabelled frames (upsample_pseudo_labels of its forward_lowres, under no_grad, in an EvalPrep
    that is refreshed every step when the teacher is trainer.ema.module because its weights move, else once), the frames and their
    pseudo-labels are mixed with their neighbour in the batch (partner = roll by one) by ClassMix (half of the classes of each frame,
    classmix_select + mix_batch), by CutMix (one box per frame whose area share is drawn from `cut_area`) or not at all (mix=None),
    and the student takes ONE batch of 2B samples -- the labelled half as given, the mixed half behind it -- through the trainer's
    own step and fused head loss.  All of that is device work at fixed addresses, handed to Trainer.step_async as its `prologue`, so
    a trainer with use_graph=True captures it with the step; the rows of a step (partner, keys or boxes, drawn from a numpy generator
    seeded by `seed`) and the threshold (`set_threshold`) live in device memory and are read by the kernels, so one graph serves every
    draw and a threshold schedule.  `last_kept` is the per-sample count of kept pseudo-labels of the last step (a device tensor).

    Weighting: with unsup_weight=None the loss is the trainer's mean over the valid pixels of all 2B samples, so the unlabelled half
    weighs in by its share of kept pixels.  unsup_weight=lambda (a float >= 0) makes it L = L_sup + lambda * L_unsup, each term a mean
    over its OWN valid pixels, from the same single head pass (per-sample loss groups, ops.upsample_cross_entropy's sample_group):
    the prologue writes the rows of the batch (tss_selftrain_weights: labelled half group 0 / weight 1, unlabelled half group 1 /
    weight lambda) and the trainer's CrossEntropyLoss reads them.  lambda lives in device memory: `set_unsup_weight` moves it from the
    next step on, captured or eager, so a ramp-up needs no re-capture.  unsup_weighting='kept_share' multiplies lambda by the batch's
    share of confident pixels, sum_b last_kept[b] / (B * H * W), the weight of ClassMix and DACS -- from the counts BEFORE mixing
    (last_kept), where ClassMix's own code counts the mixed pseudo-label map; the two differ by what the pasted classes cover.  An
    unlabelled half with no kept pixel contributes 0 and a zero gradient.  `last_group_loss` (device, float32 [2]) holds the two terms
    of the last step: L_sup and the weighted lambda * L_unsup; their sum is the returned loss.  Needs a trainer whose loss is
    tssa.CrossEntropyLoss on the fused-head route (ValueError otherwise) and B <= 512.
    Data parallel needs nothing extra: every rank draws its own rows (give the ranks different seeds).

    strong=tssa.StrongAugment(...) adds the photometric strong augmentation of the student's unlabelled input (colour jitter and
    Gaussian blur, strong_augment): the mix then writes into a scratch batch and the augmentation writes x_all[B:], both in the
    captured prologue; y_all[B:] is the mix's target as before.  Its rows are drawn in step() after the mix rows, from the same
    generator, into fixed device buffers; last_rows grows by (color, radius, taps).  With mix=None this is FixMatch's pair: the
    teacher on xu, the student on strong(xu).  Needs 3 channels, H >= 9, W >= 16.  strong=None: the launches and bits as before.

    pixel_weighting='confidence' weights every pseudo-labelled pixel's loss by the teacher's confidence (the softmax probability of
    its arg-max class): the prologue asks upsample_pseudo_labels for the confidence map, mixes it with the mask of the labels
    (mix_plane) into w_all[B:] -- w_all is float32 [2B,H,W], its labelled half ones -- and hands w_all to the trainer's
    CrossEntropyLoss (upsample_pixel_weighted_cross_entropy, normalised by `pixel_norm`).  The threshold keeps working (rejected
    pixels are ignore_index; threshold=0 is pure soft weighting) and it composes with unsup_weight.  Needs the trainer of
    unsup_weight, label smoothing 0 and B <= 512.  pixel_weighting=None: the launches and bits as before.

    What stays set: the prologue assigns the trainer's CrossEntropyLoss its map (pixel_weighting) and its sample rows (unsup_weight),
    both sized for the 2B samples of a step, and leaves them there for the next step.  Before the SAME module scores a batch of
    another size (validation, a plain supervised step) call loss_fn.clear_pixel_weight() / loss_fn.clear_sample_groups(), or it raises
    ValueError for the shape; the next step() sets them again."""

    def __init__(self, trainer, teacher, num_classes, threshold=0.95, mix='classmix', cut_area=(0.25, 0.5), ignore_index=255, seed=0,
                 unsup_weight=None, unsup_weighting='mean', strong=None, pixel_weighting=None, pixel_norm='weight'):
        if pixel_weighting not in (None, 'confidence'):
            raise ValueError("pixel_weighting must be None or 'confidence', got %r" % (pixel_weighting,))
        if pixel_norm not in ops.PIXEL_NORMS:
            raise ValueError("pixel_norm must be 'weight', 'valid' or 'pixels', got %r" % (pixel_norm,))
        self.pixel_weighting, self.pixel_norm = pixel_weighting, pixel_norm
        if pixel_weighting is not None and not (type(trainer.loss_fn) is ops.CrossEntropyLoss and trainer.fuse_head_loss
                                                and not (trainer.model._forward_hooks or trainer.model._forward_pre_hooks)
                                                and trainer.loss_fn.label_smoothing == 0.0):
            raise ValueError('SelfTraining(pixel_weighting=...): the trainer must run tssa.CrossEntropyLoss without label smoothing on '
                             'the fused-head route (a model with forward_lowres and no forward hooks), got %s'
                             % type(trainer.loss_fn).__name__)
        if strong is not None and not isinstance(strong, StrongAugment):
            raise ValueError('strong must be a tssa.StrongAugment or None, got %s' % type(strong).__name__)
        self.strong = strong
        if mix not in ('classmix', 'cutmix', None):
            raise ValueError("mix must be 'classmix', 'cutmix' or None, got %r" % (mix,))
        if unsup_weighting not in ('mean', 'kept_share'):
            raise ValueError("unsup_weighting must be 'mean' or 'kept_share', got %r" % (unsup_weighting,))
        self.unsup_weighting = unsup_weighting
        self._lam0 = None if unsup_weight is None else self._check_lambda(unsup_weight)
        if self._lam0 is not None and not (type(trainer.loss_fn) is ops.CrossEntropyLoss and trainer.fuse_head_loss
                                           and not (trainer.model._forward_hooks or trainer.model._forward_pre_hooks)):
            raise ValueError('SelfTraining(unsup_weight=...): the trainer must run tssa.CrossEntropyLoss on the fused-head route '
                             '(a model with forward_lowres and no forward hooks), got %s' % type(trainer.loss_fn).__name__)
        if not hasattr(teacher, 'forward_lowres'):
            raise NotImplementedError('SelfTraining: the teacher (%s) has no forward_lowres()' % type(teacher).__name__)
        if not 1 <= int(num_classes) <= 255 or not int(num_classes) <= int(ignore_index) <= 255:
            raise ValueError('SelfTraining: need num_classes <= ignore_index <= 255, got %r and %r' % (num_classes, ignore_index))
        lo, hi = float(cut_area[0]), float(cut_area[1])
        if not 0.0 <= lo <= hi <= 1.0:
            raise ValueError('cut_area must be 0 <= lo <= hi <= 1, got %r' % (cut_area,))
        from .engine import EvalPrep
        self.trainer, self.teacher, self.num_classes, self.mix = trainer, teacher, int(num_classes), mix
        self.cut_area, self.ignore_index = (lo, hi), int(ignore_index)
        self.rng = np.random.default_rng(seed)
        teacher.eval()
        self._teacher_prep = EvalPrep(teacher, frozen=not (trainer.ema is not None and teacher is trainer.ema.module))
        self._threshold0 = float(threshold)
        self.slot = trainer.new_slots(1)[0]
        self.x_all = None             # buffers are allocated from the first batch: a captured step reads fixed addresses

    def _allocate(self, x, y, xu):
        dev = self.trainer.device if self.trainer.device is not None else torch.device('cuda', torch.cuda.current_device())
        dev = torch.device(dev)
        B, Ci, H, W = x.shape
        if tuple(xu.shape) != (B, Ci, H, W) or xu.dtype != x.dtype:
            raise ValueError('SelfTraining: the unlabelled batch must match the labelled one (%s %s), got %s %s'
                             % (tuple(x.shape), x.dtype, tuple(xu.shape), xu.dtype))
        if tuple(y.shape) != (B, H, W) or y.dtype != torch.int64:
            raise ValueError('SelfTraining: the target must be int64 of shape %s' % ((B, H, W),))
        if W % 8:
            raise ValueError('SelfTraining needs a width that is a multiple of 8, got %d' % W)
        if self.strong is not None and (Ci != 3 or H < 9 or W < 16):
            raise ValueError('SelfTraining(strong=...) needs 3 channels, a height >= 9 and a width >= 16, got %s' % ((Ci, H, W),))
        self.geom = (B, Ci, H, W)
        self.x_all = torch.empty((2 * B, Ci, H, W), dtype=x.dtype, device=dev)
        self.y_all = torch.empty((2 * B, H, W), dtype=torch.int64, device=dev)
        self.xu = torch.empty((B, Ci, H, W), dtype=x.dtype, device=dev)
        self.pseudo = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        self.partner = torch.zeros(B, dtype=torch.int32, device=dev)
        self.keys = torch.zeros((B, 256), dtype=torch.int32, device=dev)
        self.boxes = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        self.sel = torch.zeros((B, 256), dtype=torch.uint8, device=dev)
        self.threshold = torch.full((1,), self._threshold0, dtype=torch.float32, device=dev)
        self.last_kept = torch.zeros(B, dtype=torch.int64, device=dev)
        if self.strong is not None:
            self.mixed = torch.empty((B, Ci, H, W), dtype=x.dtype, device=dev)
            self.sa_color = torch.zeros((B, 8), dtype=torch.float32, device=dev)
            self.sa_radius = torch.zeros(B, dtype=torch.int32, device=dev)
            self.sa_taps = torch.zeros((B, 12), dtype=torch.float32, device=dev)
            self.sa_ws = torch.zeros(N.lib().tss_strong_augment_ws(B, H, W) // 8, dtype=torch.float64, device=dev)
        if self.pixel_weighting is not None:
            if 2 * B > ops.GROUP_MAX_BATCH:
                raise ValueError('SelfTraining(pixel_weighting=...) takes at most %d labelled samples, got %d' % (ops.GROUP_MAX_BATCH // 2, B))
            self.w_all = torch.ones((2 * B, H, W), dtype=torch.float32, device=dev)     # the labelled half stays ones
            self.conf = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        if self._lam0 is not None:
            if 2 * B > ops.GROUP_MAX_BATCH:
                raise ValueError('SelfTraining(unsup_weight=...) takes at most %d labelled samples, got %d' % (ops.GROUP_MAX_BATCH // 2, B))
            self.group = torch.zeros(2 * B, dtype=torch.int32, device=dev)
            self.weight = torch.ones(2 * B, dtype=torch.float32, device=dev)
            self.lam = torch.full((1,), self._lam0, dtype=torch.float32, device=dev)
            self._group_loss = torch.zeros(2 * B, dtype=torch.float32, device=dev)
            self.last_group_loss = self._group_loss[:2]         # L_sup, lambda * L_unsup
        if self.trainer.use_graph:
            self.trainer.static_batch(self.x_all, self.y_all, self.slot, adopt=True)

    def set_threshold(self, value):
        """The confidence threshold from the next step on (the captured step reads it from device memory)."""
        self._threshold0 = float(value)
        if self.x_all is not None:
            self.threshold.fill_(float(value))

    @staticmethod
    def _check_lambda(value):
        v = float(value)
        if not (v >= 0.0 and v != float('inf')):
            raise ValueError('unsup_weight must be a finite number >= 0, got %r' % (value,))
        return v

    def set_unsup_weight(self, value):
        """lambda of L_sup + lambda * L_unsup from the next step on (the prologue's kernel reads it from device memory)."""
        if self._lam0 is None:
            raise ValueError('set_unsup_weight needs a SelfTraining built with unsup_weight')
        self._lam0 = self._check_lambda(value)
        if self.x_all is not None:
            self.lam.fill_(self._lam0)

    def draw(self):
        """The rows of one step as host arrays: (partner int32 [B], keys uint32 [B,256], boxes int32 [B,4])."""
        B, _, H, W = self.geom
        partner = np.roll(np.arange(B, dtype=np.int32), 1) if self.mix is not None else np.arange(B, dtype=np.int32)
        keys = np.zeros((B, 256), dtype=np.uint32)
        boxes = np.tile(np.array([0, 0, H, W], dtype=np.int32), (B, 1))       # mix=None: the whole frame stays
        if self.mix == 'classmix':
            keys = self.rng.integers(0, 2 ** 32, size=(B, 256), dtype=np.uint64).astype(np.uint32)
        elif self.mix == 'cutmix':
            area = self.rng.uniform(self.cut_area[0], self.cut_area[1], size=B)
            aspect = np.exp(self.rng.uniform(np.log(0.5), np.log(2.0), size=B))
            bh = np.clip(np.rint(np.sqrt(area * aspect) * H), 1, H).astype(np.int64)
            bw = np.clip(np.rint(area * H * W / bh), 1, W).astype(np.int64)
            y0 = (self.rng.random(B) * (H - bh + 1)).astype(np.int64)
            x0 = (self.rng.random(B) * (W - bw + 1)).astype(np.int64)
            boxes = np.stack([y0, x0, y0 + bh, x0 + bw], 1).astype(np.int32)
        return partner, keys, boxes

    def _prepare(self):
        """The captured prologue: device work only, and idempotent (the capture warm-up runs it twice)."""
        B, Ci, H, W = self.geom
        with torch.no_grad(), self._teacher_prep:
            low = ops.materialize(self.teacher.forward_lowres(self.xu))
            self.last_kept.zero_()
            conf = self.conf if self.pixel_weighting is not None else None
            upsample_pseudo_labels(low, self.threshold, size=(H, W), ignore_index=self.ignore_index, kept=self.last_kept, out=self.pseudo,
                                   out_confidence=conf)
            if self.mix == 'classmix':
                call('tss_classmix_select', ptr(self.pseudo), ptr(self.keys), ptr(self.sel), B, H * W, self.num_classes, stream())
            mix_batch(self.xu, self.pseudo, self.partner, sel=self.sel if self.mix == 'classmix' else None,
                      boxes=None if self.mix == 'classmix' else self.boxes,
                      out_image=self.x_all[B:] if self.strong is None else self.mixed, out_target=self.y_all[B:])
            if self.pixel_weighting is not None:        # the confidence follows the mask of the labels (mix=None: the whole-frame box copies)
                mix_plane(self.conf, self.pseudo, self.partner, sel=self.sel if self.mix == 'classmix' else None,
                          boxes=None if self.mix == 'classmix' else self.boxes, out=self.w_all[B:])
                self.trainer.loss_fn.pixel_weight, self.trainer.loss_fn.pixel_norm = self.w_all, self.pixel_norm
            if self.strong is not None:
                strong_augment(self.mixed, self.sa_color, self.sa_radius, self.sa_taps, self.strong.mean, self.strong.std,
                               out=self.x_all[B:], workspace=self.sa_ws)
            if self._lam0 is not None:
                call('tss_selftrain_weights', ptr(self.last_kept), H * W, ptr(self.lam), 1 if self.unsup_weighting == 'kept_share' else 0,
                     ptr(self.group), ptr(self.weight), B, stream())
                loss_fn = self.trainer.loss_fn
                loss_fn.sample_group, loss_fn.sample_weight, loss_fn.group_loss_out = self.group, self.weight, self._group_loss

    def step(self, x, y, xu):
        """One self-training step on the labelled batch (x, y) and the unlabelled frames xu; returns the loss as a device tensor."""
        if self.x_all is None:
            self._allocate(x, y, xu)
        B = self.geom[0]
        self.x_all[:B].copy_(x, non_blocking=True)
        self.y_all[:B].copy_(y, non_blocking=True)
        self.xu.copy_(xu, non_blocking=True)
        partner, keys, boxes = self.draw()
        self.partner.copy_(torch.from_numpy(partner))
        if self.mix == 'classmix':
            self.keys.copy_(torch.from_numpy(keys.view(np.int32)))
        else:
            self.boxes.copy_(torch.from_numpy(boxes))
        self.last_rows = (partner, keys, boxes)
        if self.strong is not None:
            color, radius, taps = self.strong.draw(B, self.rng)
            self.sa_color.copy_(torch.from_numpy(color))
            self.sa_radius.copy_(torch.from_numpy(radius))
            self.sa_taps.copy_(torch.from_numpy(taps))
            self.last_rows += (color, radius, taps)
        return self.trainer.step_async(self.x_all, self.y_all, self.slot, prologue=self._prepare)
