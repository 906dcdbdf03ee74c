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


def upsample_pseudo_labels(low, threshold, scale_factor=None, size=None, ignore_index=255, want_confidence=False, kept=None, out=None):
    """Pseudo-labels of F.interpolate(low, bilinear, align_corners=True) without the full-resolution logits
    (tss_upsample_pseudo_label[_wide]): per pixel the arg-max class (lowest index wins ties) where its softmax probability reaches
    `threshold`, `ignore_index` elsewhere.  low: the NHWC map of forward_lowres, read in place, or an NCHW tensor; threshold: a float
    (kept in a cached device scalar) or a one-element float32 device tensor, read by the kernel -- a captured step follows its value.
    Returns (labels uint8 [B,H,W], confidence float32 [B,H,W] or None, kept int64 [B]): confidence is written for every pixel; kept
    counts the labels kept per sample and is zero-filled here unless the caller passes a tensor of their own to accumulate into.
    `out`: a uint8 [B,H,W] tensor to write the labels into.  Up to 24 classes the scores of a pixel live in registers, up to 255
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
    Data parallel needs nothing extra: every rank draws its own rows (give the ranks different seeds)."""

    def __init__(self, trainer, teacher, num_classes, threshold=0.95, mix='classmix', cut_area=(0.25, 0.5), ignore_index=255, seed=0,
                 unsup_weight=None, unsup_weighting='mean'):
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
            upsample_pseudo_labels(low, self.threshold, size=(H, W), ignore_index=self.ignore_index, kept=self.last_kept, out=self.pseudo)
            if self.mix == 'classmix':
                call('tss_classmix_select', ptr(self.pseudo), ptr(self.keys), ptr(self.sel), B, H * W, self.num_classes, stream())
            mix_batch(self.xu, self.pseudo, self.partner, sel=self.sel if self.mix == 'classmix' else None,
                      boxes=None if self.mix == 'classmix' else self.boxes, out_image=self.x_all[B:], out_target=self.y_all[B:])
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
        return self.trainer.step_async(self.x_all, self.y_all, self.slot, prologue=self._prepare)
