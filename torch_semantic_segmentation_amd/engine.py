"""Train / eval step of the hot path: the counterpart of TSS/engine.py (rows R, S of SURVEY.md §8a).

`create_segmentation_trainer` reproduces the body of the reference's `update_fn` (TSS/engine.py:24-39):
train mode, zero_grad, forward, loss, backward, optimizer step, loss value.  ignite and apex are not
dependencies: the returned :class:`Trainer` is a plain object with `update(batch)` and `run(loader, epochs)`.

MI355X specifics
  * parameters and gradients of the model live in two flat f32 buffers (`FlatAdamW`, `FlatSGD`), so the optimizer is one
    fused kernel (tss_adamw_step_groups / tss_sgd_step_groups) and data-parallel training needs ONE RCCL all-reduce per step;
  * weight-gradient kernels accumulate straight into the flat gradient buffer (ops.direct_grads), so there is
    no per-parameter `.grad +=` launch;
  * zero_grad + forward + loss + backward can be captured once into a HIP graph (`use_graph=True`) and
    replayed, removing ~10^3 Python-side launches per step;
  * one process per GPU; gradients are averaged with `torch.distributed.all_reduce` (backend "nccl" = RCCL over
    xGMI on GPUs, "gloo" on CPU for tests).  BatchNorm statistics stay per replica unless the model
    went through `convert_syncbn_model` (ops.SyncBatchNorm: one small all-reduce per BatchNorm layer and direction).
"""
import copy
import ctypes
import os
from functools import partial

import numpy as np
import torch
import torch.distributed as dist
from torch import nn

from . import _native as N
from . import ops


# ----------------------------------------------------------------------------- flat parameters + fused optimizers

MAX_PARAM_GROUPS = 8            # TSS_OPT_MAX_GROUPS of include/tss_hip.h: the group table travels in the kernel arguments
_UNSUPPORTED_FLAGS = ('amsgrad', 'maximize', 'foreach', 'fused')


class _OptGroup(ctypes.Structure):
    """tss_optgroup of include/tss_hip.h."""
    _fields_ = [('begin', ctypes.c_long), ('end', ctypes.c_long), ('lr', ctypes.c_float), ('weight_decay', ctypes.c_float),
                ('beta1', ctypes.c_float), ('beta2', ctypes.c_float), ('eps', ctypes.c_float), ('flags', ctypes.c_int)]


def ema_omd(k, decay, warmup=False):
    """The factor 1 - d_k of update number k (0-based) of the weight average, as a numpy float32: d_k = decay, or warming up
    min(decay, (1 + k) / (10 + k)).  Every operation is a float32 one, as in the tick kernel of csrc/optim.hip: the same bits."""
    d = np.float32(decay)
    if warmup:
        d = np.minimum(d, (np.float32(1.0) + np.float32(k)) / (np.float32(10.0) + np.float32(k)))
    return np.float32(1.0) - d


def _check_decay(decay, who):
    if not (0.0 <= float(decay) < 1.0) or not (0.0 <= float(np.float32(decay)) < 1.0):
        raise ValueError('%s: decay must lie in [0, 1) (in float32 too), got %r' % (who, decay))
    return float(decay)


class FlatOptimizer(torch.optim.Optimizer):
    """What FlatAdamW and FlatSGD share: the parameters of all groups packed into ONE flat f32 buffer (groups in order, parameters in
    order within a group), their gradients aliased into a second one, and the step as one fused kernel over both.

    `params` is an iterable of tensors or of group dicts, with torch.optim's defaulting rules; at most MAX_PARAM_GROUPS groups.
    Each `param_groups[i]['lr']` stays a Python float so LR schedulers work; the rates are kernel arguments of the step, or (with
    `device_state = True`) mirrored into device memory before every step() that is not being captured -- call sync_lr() between the
    replays of a captured step().

    `max_grad_norm`: torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) over ALL groups as part of step(): one
    deterministic reduction over the flat gradient buffer (after the all-reduce, `grad_scale` applied), whose clip factor the
    step kernel reads from the device.  The gradients themselves (`p.grad`) are NOT rescaled in place.  `last_grad_norm` is the
    pre-clip norm of the latest step as a 0-dim device tensor (a view: no synchronisation, overwritten by the next step); a
    non-finite norm propagates into the parameters as it does in torch.
    """

    def __init__(self, params, defaults, max_grad_norm=None, **flags):
        name = type(self).__name__
        self._reject_flags(flags)
        params = list(params)
        if params and isinstance(params[0], dict):
            if len(params) > MAX_PARAM_GROUPS:
                raise ValueError('%s: at most %d parameter groups, got %d' % (name, MAX_PARAM_GROUPS, len(params)))
            groups = []
            for g in params:
                g = dict(g)
                ps = g['params']
                g['params'] = [ps] if isinstance(ps, torch.Tensor) else list(ps)
                if not g['params']:
                    raise ValueError('%s: an empty parameter group' % name)
                self._reject_flags(g)
                groups.append(g)
            params = groups
        self._laid_out = False
        super().__init__(params, defaults)
        for g in self.param_groups:
            self._check_group(g)
        ps = [p for g in self.param_groups for p in g['params']]
        dev = ps[0].device
        if any(p.dtype != torch.float32 or p.device != dev for p in ps):
            raise TypeError('%s: float32 parameters on one device' % name)
        n = sum(p.numel() for p in ps)
        self.flat_param = torch.empty(n, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(n, dtype=torch.float32, device=dev)
        off = 0
        self.group_ranges = []           # [begin, end) of every group in the flat buffers
        with torch.no_grad():
            for g in self.param_groups:
                begin = off
                for p in g['params']:
                    k = p.numel()
                    self.flat_param[off:off + k].copy_(p.reshape(-1))
                    p.data = self.flat_param[off:off + k].view_as(p)
                    p.grad = self.flat_grad[off:off + k].view_as(p)
                    off += k
                self.group_ranges.append((begin, off))
        self._laid_out = True
        G = len(self.param_groups)
        # step counter and learning rates: on the host (kernel arguments of ONE launch per step) unless device_state=True, which
        # keeps them in device memory behind a tick kernel so that step() itself can be captured in a HIP graph
        self.device_state = False
        self.step_count = 0
        self.state_vec = torch.zeros(3 * G, dtype=torch.float32, device=dev)  # device_state: per group step, bias corrections
        self.lr_dev = torch.tensor([float(g['lr']) for g in self.param_groups], dtype=torch.float32).to(dev)
        self.grad_scale = 1.0
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        if self.max_grad_norm is not None:
            self._clip_out = torch.zeros(2, dtype=torch.float32, device=dev)     # tss_grad_sqnorm: norm, gradient factor
            self._clip_ws = None                               # its partial rows (on the device: the library is there to ask)
            if dev.type == 'cuda':
                self._clip_ws = torch.empty(N.lib().tss_grad_sqnorm_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
            self.last_grad_norm = self._clip_out[0]
        self.ema_flat = None             # attach_ema(): a third flat buffer the step kernel averages the new parameters into

    def attach_ema(self, ema_flat, decay, warmup=False):
        """From now on every step() also updates `ema_flat` (float32, laid out as flat_param) in the step kernel itself:
        e += (p_new - e) * (1 - d_k), d_k = decay, or with warmup min(decay, (1 + k) / (10 + k)) for update number k.  No extra launch,
        8 more bytes per element.  The counter k and the factor live on the host (kernel arguments) or, with device_state, in
        `ema_state` behind the tick kernel, so a captured step() replays them.  engine.ModelEMA is the owner of such a buffer."""
        name = type(self).__name__
        decay = _check_decay(decay, name + '.attach_ema')
        if (ema_flat.dtype != torch.float32 or ema_flat.shape != self.flat_param.shape or ema_flat.device != self.flat_param.device
                or not ema_flat.is_contiguous()):
            raise ValueError('%s.attach_ema: the average is a contiguous float32 buffer of %d elements on %s'
                             % (name, self.flat_param.numel(), self.flat_param.device))
        if ema_flat.data_ptr() == self.flat_param.data_ptr():
            raise ValueError('%s.attach_ema: the average must not alias the parameters' % name)
        self.ema_flat, self.ema_decay, self.ema_warmup = ema_flat, decay, bool(warmup)
        self.ema_updates = 0             # k: the updates done so far (host mirror of ema_state[0])
        self.ema_state = torch.zeros(2, dtype=torch.float32, device=ema_flat.device)      # device_state: {k, 1 - d_(k-1)}

    def _ema_row(self, k):
        """{k, factor of the latest update}: what the tick kernel leaves in ema_state after k updates."""
        return [float(k), float(ema_omd(k - 1, self.ema_decay, self.ema_warmup)) if k > 0 else 0.0]

    def _ema_args(self):
        """The trailing arguments of the _ema entries: decay, warmup, the host's factor for this update, the device row."""
        return (self.ema_decay, int(self.ema_warmup), float(ema_omd(self.ema_updates, self.ema_decay, self.ema_warmup)),
                N.ptr(self.ema_state) if self.device_state else None)

    @staticmethod
    def _reject_flags(mapping):
        for flag in _UNSUPPORTED_FLAGS:
            if mapping.get(flag):
                raise ValueError('the flat optimizers have one fused kernel per step: %s=%r is not supported' % (flag, mapping[flag]))

    def _check_group(self, group):
        """Subclass hook: validate one parameter group (after torch filled in its defaults)."""

    def add_param_group(self, param_group):
        if getattr(self, '_laid_out', False):
            raise NotImplementedError('%s.add_param_group: the flat parameter, gradient and state buffers are laid out once, at '
                                      'construction, and every parameter is a view into them; build a new optimizer with all '
                                      'groups instead' % type(self).__name__)
        super().add_param_group(param_group)

    def _params(self):
        return (p for g in self.param_groups for p in g['params'])

    def zero_grad(self, set_to_none=False):
        self.flat_grad.zero_()

    def _check_aliases(self):
        """Every p.grad must still be its slice of flat_grad (model.zero_grad(set_to_none=True) or an optimizer-external
        `p.grad = ...` detaches it; stepping would then silently apply zero gradients)."""
        off = 0
        base = self.flat_grad.data_ptr()
        esz = self.flat_grad.element_size()
        for p in self._params():
            g = p.grad
            if g is None or g.data_ptr() != base + esz * off:
                raise RuntimeError('%s: a parameter gradient no longer aliases the flat gradient buffer (was '
                                   'model.zero_grad(set_to_none=True) called?); use optimizer.zero_grad() or reattach()'
                                   % type(self).__name__)
            off += p.numel()

    def reattach(self):
        """Point every p.grad back at its slice of the flat gradient buffer."""
        off = 0
        for p in self._params():
            k = p.numel()
            p.grad = self.flat_grad[off:off + k].view_as(p)
            off += k

    def sync_lr(self):
        """device_state: mirror every group's learning rate into device memory (one small fill per group, outside any capture)."""
        for i, g in enumerate(self.param_groups):
            self.lr_dev[i:i + 1].fill_(float(g['lr']))

    # -- what a subclass supplies
    _state_names = ()                    # its flat state buffers, as named in state_dict()['flat']

    def _state_rows(self, k):
        """[3 * groups] floats of the device-side state after k steps (what the tick kernel would have written)."""
        raise NotImplementedError

    def _group_row(self, group, begin, end):
        raise NotImplementedError

    def _launch(self, rows, scale):
        raise NotImplementedError

    def state_dict(self):
        """torch.optim state_dict plus the flat state buffers, the group ranges and the step counter (checkpoint / resume)."""
        sd = super().state_dict()
        sv = self.state_vec.clone()
        if not self.device_state:
            sv = torch.tensor(self._state_rows(float(self.step_count)), dtype=torch.float32, device=sv.device)
        flat = {name: (None if getattr(self, name) is None else getattr(self, name).clone()) for name in self._state_names}
        flat['state_vec'] = sv
        flat['group_ranges'] = [list(r) for r in self.group_ranges]
        if self.ema_flat is not None:    # the counter and latest factor of the average (its values: ModelEMA.state_dict())
            flat['ema_state'] = self.ema_state.clone() if self.device_state else \
                torch.tensor(self._ema_row(self.ema_updates), dtype=torch.float32, device=sv.device)
        sd['flat'] = flat
        return sd

    def load_state_dict(self, state_dict):
        name = type(self).__name__
        state_dict = dict(state_dict)
        flat = state_dict.pop('flat', None)
        if flat is None and state_dict.get('state'):
            # a torch.optim checkpoint (per-parameter exp_avg / exp_avg_sq / step / momentum_buffer): its state would land in
            # self.state and never be read -- a resume would silently restart the bias correction
            raise ValueError('%s.load_state_dict: this state_dict has per-parameter state but no flat moments (it was not '
                             'written by %s.state_dict()); pack it into the flat buffers before loading' % (name, name))
        if flat is not None:
            ranges = flat.get('group_ranges')
            mine = [list(r) for r in self.group_ranges]
            if ranges is None:           # written before parameter groups existed: one group over the whole buffer
                whole = flat.get(self._state_names[0])
                ranges = [[0, int(whole.numel())]] if whole is not None else None
            if ranges is None or [list(map(int, r)) for r in ranges] != mine:
                raise ValueError('%s.load_state_dict: the checkpoint lays its parameter groups out as %s, this optimizer as %s'
                                 % (name, ranges, mine))
            missing = [k for k in self._state_names if k not in flat]
            if missing:
                raise ValueError('%s.load_state_dict: the checkpoint has no flat %s' % (name, ', '.join(missing)))
        super().load_state_dict(state_dict)
        if flat is not None:
            with torch.no_grad():
                for k in self._state_names:
                    if flat[k] is not None and getattr(self, k) is not None:
                        getattr(self, k).copy_(flat[k])
                self.state_vec.copy_(flat['state_vec'])
            self.step_count = int(round(float(flat['state_vec'][0])))
            if self.ema_flat is not None and flat.get('ema_state') is not None:
                with torch.no_grad():
                    self.ema_state.copy_(flat['ema_state'])
                self.ema_updates = int(round(float(flat['ema_state'][0])))

    @torch.no_grad()
    def step(self, closure=None):
        if not self.flat_param.is_cuda:
            raise RuntimeError('%s runs on the HIP path only (no CPU fallback)' % type(self).__name__)
        self._check_aliases()
        self.step_count += 1
        if self.device_state and not torch.cuda.is_current_stream_capturing():
            self.sync_lr()
        rows = (_OptGroup * len(self.param_groups))(*[self._group_row(g, b, e)
                                                      for g, (b, e) in zip(self.param_groups, self.group_ranges)])
        scale = None
        if self.max_grad_norm is not None:
            N.call('tss_grad_sqnorm', N.ptr(self.flat_grad), self.flat_grad.numel(), N.ptr(self._clip_ws), float(self.grad_scale),
                   self.max_grad_norm, N.ptr(self._clip_out), N.stream())
            scale = self._clip_out.data_ptr() + self._clip_out.element_size()
        self._launch(rows, scale)
        if self.ema_flat is not None:
            self.ema_updates += 1


class FlatAdamW(FlatOptimizer):
    """torch.optim.AdamW semantics (decoupled weight decay, bias correction) on ONE flat f32 buffer, with parameter groups (a group
    may override lr, betas, eps, weight_decay) and optional global-norm clipping: see FlatOptimizer."""
    _state_names = ('exp_avg', 'exp_avg_sq')

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, amsgrad=False,
                 maximize=False, foreach=None, fused=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), max_grad_norm=max_grad_norm,
                         amsgrad=amsgrad, maximize=maximize, foreach=foreach, fused=fused)
        self.exp_avg = torch.zeros_like(self.flat_param)
        self.exp_avg_sq = torch.zeros_like(self.flat_param)

    def _state_rows(self, k):
        rows = []
        for g in self.param_groups:
            b1, b2 = g['betas']
            rows += [k, 1.0 - b1 ** k, (1.0 - b2 ** k) ** 0.5]
        return rows

    def _group_row(self, g, begin, end):
        b1, b2 = g['betas']
        return _OptGroup(begin, end, float(g['lr']), float(g['weight_decay']), float(b1), float(b2), float(g['eps']), 0)

    def _launch(self, rows, scale):
        dev = self.device_state
        tail = (self.flat_param.numel(), rows, len(rows), N.ptr(self.lr_dev) if dev else None, N.ptr(self.state_vec) if dev else None,
                scale, float(self.grad_scale), int(self.step_count))
        head = (N.ptr(self.flat_param), N.ptr(self.flat_grad), N.ptr(self.exp_avg), N.ptr(self.exp_avg_sq))
        if self.ema_flat is not None:
            N.call('tss_adamw_step_groups_ema', *head, N.ptr(self.ema_flat), *tail, *self._ema_args(), N.stream())
        else:
            N.call('tss_adamw_step_groups', *head, *tail, N.stream())


class FlatSGD(FlatOptimizer):
    """torch.optim.SGD semantics (weight decay added to the gradient, momentum with dampening, Nesterov) on ONE flat f32 buffer, with
    parameter groups (a group may override lr, momentum, dampening, weight_decay, nesterov) and optional global-norm clipping: see
    FlatOptimizer.  The momentum buffer exists only when some group has momentum; a group without never touches it."""
    _state_names = ('momentum_buffer',)

    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, max_grad_norm=None, maximize=False,
                 foreach=None, fused=None):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov),
                         max_grad_norm=max_grad_norm, maximize=maximize, foreach=foreach, fused=fused)
        self.momentum_buffer = None
        if any(g['momentum'] != 0 for g in self.param_groups):
            self.momentum_buffer = torch.zeros_like(self.flat_param)

    def _check_group(self, g):
        if g['nesterov'] and (g['momentum'] <= 0 or g['dampening'] != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')

    def _state_rows(self, k):
        return [k, 0.0, 0.0] * len(self.param_groups)

    def _group_row(self, g, begin, end):
        return _OptGroup(begin, end, float(g['lr']), float(g['weight_decay']), float(g['momentum']), float(g['dampening']), 0.0,
                         1 if g['nesterov'] else 0)

    def _launch(self, rows, scale):
        dev = self.device_state
        tail = (self.flat_param.numel(), rows, len(rows), N.ptr(self.lr_dev) if dev else None, N.ptr(self.state_vec) if dev else None,
                scale, float(self.grad_scale), int(self.step_count))
        head = (N.ptr(self.flat_param), N.ptr(self.flat_grad), N.ptr(self.momentum_buffer))
        if self.ema_flat is not None:
            N.call('tss_sgd_step_groups_ema', *head, N.ptr(self.ema_flat), *tail, *self._ema_args(), N.stream())
        else:
            N.call('tss_sgd_step_groups', *head, *tail, N.stream())


# ----------------------------------------------------------------------------- weight average

EMA_LERP_F32, EMA_COPY_F32, EMA_COPY_I64 = 0, 1, 2       # TSS_EMA_* of include/tss_hip.h


class ModelEMA:
    """Exponential moving average of a model's weights, the model that segmentation recipes evaluate, checkpoint and (as a mean
    teacher) distill from:  e += (p - e) * (1 - d_k) after every optimizer step, d_k = decay, or with warmup=True
    min(decay, (1 + k) / (10 + k)) for update number k = 0, 1, ...  (torch.optim.swa_utils.AveragedModel with
    get_ema_multi_avg_fn(decay) and use_buffers=True, in float32 and without its host loop).

    `.module` is the averaged model: copy.deepcopy(model), or `module`, a second instance with the same state_dict keys and shapes
    (it is overwritten with the model's values).  It is in eval(), none of its parameters requires grad, and it keeps the compute
    dtype of `model`.  It shares no storage with `model`.

    With a FlatOptimizer the parameters of `.module` that the optimizer holds become views into ONE flat buffer laid out as the
    optimizer's flat_param, and the optimizer's own step kernel averages them (FlatOptimizer.attach_ema): update() then launches
    one kernel (tss_ema_rows) for the rest -- floating-point buffers (BatchNorm running statistics) are averaged, integer ones
    (num_batches_tracked) and parameters outside the optimizer are copied.  Call update() once after every optimizer.step(), on its
    stream (Trainer(ema=...) does).  With any other optimizer, or none, update() is that one launch over every parameter and buffer.

    Data parallel: after the all-reduced step every rank holds identical parameters, so every rank computes the same average of them
    and no communication is needed; the running statistics are per replica (or identical under SyncBatchNorm), and so are their
    averages.

    The table of the rows kernel holds device addresses: build a new ModelEMA after anything that reallocates the model's tensors
    (model.to(...)); load_state_dict() and optimizer steps write in place and are fine."""

    def __init__(self, model, optimizer=None, decay=0.999, warmup=False, module=None):
        self.decay, self.warmup = _check_decay(decay, 'ModelEMA'), bool(warmup)
        src = dict(model.state_dict(keep_vars=True))
        if module is None:
            module = copy.deepcopy(model)
        elif module is model:
            raise ValueError('ModelEMA: `module` must be a second instance, not the model itself')
        dst = dict(module.state_dict(keep_vars=True))
        if list(src) != list(dst):
            raise ValueError('ModelEMA: the state_dict keys of `module` differ from the model\'s: %s'
                             % sorted(set(src) ^ set(dst))[:8])
        for k in src:
            if src[k].shape != dst[k].shape or src[k].dtype != dst[k].dtype:
                raise ValueError('ModelEMA: %s is %s %s in the model, %s %s in `module`'
                                 % (k, tuple(src[k].shape), src[k].dtype, tuple(dst[k].shape), dst[k].dtype))
        if any(not t.is_cuda for t in src.values()) or any(not t.is_cuda for t in dst.values()):
            raise RuntimeError('ModelEMA runs on the HIP path only (no CPU fallback): move the model to the GPU first')
        for k, t in src.items():
            if t.dtype not in (torch.float32, torch.int64) or not t.is_contiguous() or not dst[k].is_contiguous():
                raise ValueError('ModelEMA: %s is %s%s; the average takes contiguous float32 tensors and int64 counters'
                                 % (k, t.dtype, '' if t.is_contiguous() else ', not contiguous'))
        self.module, self.optimizer, self.num_updates = module, optimizer, 0
        self.flat = isinstance(optimizer, FlatOptimizer)
        self.ema_flat = None             # with a FlatOptimizer: the buffer its step kernel averages into
        if hasattr(model, 'compute_dtype'):
            from .models import set_compute_dtype
            set_compute_dtype(module, model.compute_dtype)
        module.eval()
        params = dict(model.named_parameters())
        held = set()                     # the names of the parameters the optimizer's step kernel averages
        with torch.no_grad():
            for k in src:
                dst[k].copy_(src[k])
            if self.flat:
                names = {id(p): k for k, p in params.items()}
                self.ema_flat = optimizer.flat_param.clone()
                off = 0
                for p in optimizer._params():
                    n = p.numel()
                    k = names.get(id(p))
                    if k is not None:    # (a parameter of another model in the same optimizer is averaged too, into the flat buffer only)
                        dst[k].data = self.ema_flat[off:off + n].view_as(p)
                        held.add(k)
                    off += n
                optimizer.attach_ema(self.ema_flat, self.decay, self.warmup)
        for p in module.parameters():
            p.requires_grad_(False)
            p.grad = None
        rows = []
        for k, t in src.items():
            if k in held or t.numel() == 0:
                continue
            mode = EMA_COPY_I64 if t.dtype == torch.int64 else (EMA_COPY_F32 if (self.flat and k in params) else EMA_LERP_F32)
            rows.append([t.data_ptr(), dst[k].data_ptr(), t.numel(), mode])
        self._keep = [(src[k], dst[k]) for k in src]        # the table's addresses stay allocated as long as it is used
        dev = next(iter(src.values())).device if src else None
        self.table = torch.tensor(rows, dtype=torch.int64, device=dev).reshape(-1, 4) if rows else None

    def update(self):
        """One update of everything the optimizer's step kernel does not average: one launch, on the current stream."""
        k = self.num_updates
        state = None
        if self.flat:
            opt = self.optimizer
            if opt.device_state:
                state = N.ptr(opt.ema_state)          # the factor the step's tick wrote
            elif opt.ema_updates != k + 1:
                raise RuntimeError('ModelEMA.update() follows optimizer.step(), once: the optimizer has averaged %d steps, this is '
                                   'update %d' % (opt.ema_updates, k + 1))
        if self.table is not None:
            N.call('tss_ema_rows', N.ptr(self.table), self.table.shape[0], float(ema_omd(k, self.decay, self.warmup)), state, N.stream())
        self.num_updates = k + 1

    @torch.no_grad()
    def copy_to(self, model):
        """Write the averaged parameters and buffers into `model`, in place."""
        model.load_state_dict(self.module.state_dict(), strict=True)

    def state_dict(self):
        return {'module': {k: v.detach().clone() for k, v in self.module.state_dict().items()}, 'num_updates': self.num_updates,
                'decay': self.decay, 'warmup': self.warmup}

    def load_state_dict(self, state_dict):
        """The averaged values and the update counter (in place: the flat views stay).  With a FlatOptimizer load the optimizer's
        own state_dict too: it carries the counter of the step kernel's part."""
        self.module.load_state_dict(state_dict['module'], strict=True)
        self.num_updates = int(state_dict['num_updates'])

# ----------------------------------------------------------------------------- distributed helpers

def setup_distributed(enable=True, local_rank=None, backend=None):
    """TSS/utils/training.py:5-19 without the GPU-only assumption: returns (world_size, rank, local_rank).
    Reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment (torch.distributed.run)."""
    if not enable:
        return 1, 0, 0
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0')) if local_rank is None else local_rank
    # (gloo ranks hold CPU tensors: more of them than visible devices is fine; any other backend needs its own device and raises here)
    if torch.cuda.is_available() and (backend != 'gloo' or local_rank < torch.cuda.device_count()):
        torch.cuda.set_device(local_rank)
    launched = 'RANK' in os.environ and 'MASTER_ADDR' in os.environ     # under torch.distributed.run, even with 1 rank
    if (world > 1 or launched) and not dist.is_initialized():
        dist.init_process_group(backend or ('nccl' if torch.cuda.is_available() else 'gloo'), init_method='env://')
    if dist.is_initialized():
        return dist.get_world_size(), dist.get_rank(), local_rank
    return 1, 0, local_rank


def shard_batch(n_items, world_size, rank):
    """DistributedSampler's partition without shuffling (TSS/utils/training.py:54-61): rank r owns r, r+W, ..."""
    return list(range(rank, n_items, world_size))


def allreduce_mean_(flat, world_size, group=None):
    """ONE collective per step over the flat gradient buffer: sum here, the 1/world factor is folded into the optimizer
    step (FlatOptimizer.grad_scale)."""
    if world_size > 1 or (dist.is_available() and dist.is_initialized()):
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    return flat


# ----------------------------------------------------------------------------- trainer

class Trainer:
    def __init__(self, model, optimizer, loss_fn, device=None, use_graph=False, world_size=None,
                 non_blocking=True, fuse_head_loss=True, graph_allreduce=None, teacher=None, distill_loss=None, distill_weight=1.0,
                 ema=None):
        self.model, self.optimizer, self.loss_fn = model, optimizer, loss_fn
        # `ema`: a ModelEMA of `model` (built over `optimizer`), updated right after every optimizer step on the step's stream.
        # teacher=ema.module makes it a mean teacher: its preparation (bf16 shadows, eval affines, 3x3 copies) is then refreshed
        # inside every step, captured or not, because its weights move.
        if ema is not None and ema.optimizer is not None and ema.optimizer is not optimizer:
            raise ValueError('Trainer: `ema` was built over another optimizer than the one that steps')
        self.ema = ema
        # Logit distillation: `distill_weight * distill_loss(low, teacher_low)` on the low-resolution logits is added to the loss.  The
        # teacher is frozen: eval() once and for all, forward under no_grad inside an EvalPrep(frozen=True) whose preparation launches
        # run once (its weights never change), on the step's stream and, with use_graph, inside the captured step.
        if (teacher is None) != (distill_loss is None):
            raise ValueError('Trainer: teacher and distill_loss come together (got teacher=%s, distill_loss=%s)'
                             % (type(teacher).__name__, type(distill_loss).__name__))
        if teacher is not None:
            for m, who in ((teacher, 'teacher'), (model, 'model')):
                if not hasattr(m, 'forward_lowres'):
                    raise NotImplementedError('Trainer: distillation compares low-resolution logits, but the %s (%s) has no '
                                              'forward_lowres()' % (who, type(m).__name__))
            teacher.eval()
        self.teacher, self.distill_loss, self.distill_weight = teacher, distill_loss, distill_weight
        self._teacher_prep = None
        self.device = device
        self.non_blocking = non_blocking
        # gradients are SUMMED over the ranks and scaled by 1/world_size: the factor must be the size of the group the
        # all-reduce runs over, so it is derived from torch.distributed unless given (and checked when given)
        live = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        if world_size is None:
            world_size = live
        elif world_size != live:
            raise ValueError('Trainer(world_size=%d) but torch.distributed has %d rank(s): gradients would be scaled wrongly'
                             % (world_size, live))
        self.world_size = world_size
        self.use_graph = use_graph
        self.flat = isinstance(optimizer, FlatOptimizer)
        # model(x) followed by CrossEntropyLoss == the fused head+loss operator on model.forward_lowres(x): same
        # value and gradients, but the full-resolution logits never exist (-1.3 GB and ~0.8 ms at 8x1024x2048:
        # one 0.26 ms kernel instead of five that move 3.8 GB).  Only taken when nothing can observe the difference
        # (our loss class, a model that offers forward_lowres, no hooks on the model itself).  FocalLoss and DiceLoss have a fused
        # operator too (ops.upsample_focal_loss / upsample_dice_loss), but its result differs from the unfused one in the last bits,
        # so they take it only when the module was built with fused_head=True.
        fusable = type(loss_fn) in (ops.CrossEntropyLoss, ops.OHEMLoss) \
            or (type(loss_fn) in (ops.FocalLoss, ops.DiceLoss) and loss_fn.fused_head)
        self.fuse_head_loss = bool(fuse_head_loss) and fusable and hasattr(model, 'forward_lowres') and hasattr(model, 'logit_scale')
        if self.flat:
            optimizer.grad_scale = 1.0 / world_size
        self.shadows = None
        # The gradient all-reduce INSIDE the captured step (RCCL collectives on the capturing stream are recorded into the HIP
        # graph): the step is then replay + optimizer, nothing else on the host.  Opt-in (argument or TSS_GRAPH_ALLREDUCE=1):
        # validated on hardware with a one-rank RCCL group only -- a multi-GPU node was never available to this repo -- so the
        # default keeps the collective an ordinary eager launch behind the replay, which is the form the 8-GPU run depends on.
        if graph_allreduce is None:
            graph_allreduce = os.environ.get('TSS_GRAPH_ALLREDUCE') == '1'
        self.graph_allreduce = bool(graph_allreduce) and self.flat and dist.is_available() and dist.is_initialized() \
            and dist.get_backend() == 'nccl'
        self._reduce_captured = False
        self._collectives_in_graph = False
        # captured steps, one per input slot: slot -> (graph, loss tensor).  Slot 0 is the ordinary one; a loader that
        # double-buffers its batches (HostBatchPipeline) captures one step per staging slot so that the step reads the
        # staged batch in place -- no device-to-device copy between the H2D copy and the step
        self._graphs = {}
        self._statics = {}
        self._one = None
        self._next_slot = 1           # slot 0 is the trainer's own; new_slots() hands out the rest, never twice
        self._pool = None             # one private memory pool shared by the captured steps of all slots (they never run concurrently)
        self.iteration = 0
        self.last_loss = None

    @property
    def _graph(self):
        g = self._graphs.get(0)
        return g[0] if g else None

    # -- one un-captured iteration: exactly the statements of the reference's update_fn
    def _forward_backward(self, x, y, prologue=None):
        if prologue is not None:      # device-side preparation of (x, y), e.g. the uint8 decode: part of the captured step
            prologue()
        self.model.train()
        if self.shadows is None:
            self.shadows = ops.WeightShadows(self.model)
        # the optimizer step of the previous iteration changed the weights: one launch rewrites their bf16 shadows AND clears the
        # flat gradient buffer (optimizer.zero_grad() of TSS/engine.py:28)
        if self.flat and os.environ.get('TSS_MEMSET_NODES') == '1':
            # diagnostic only (tools/graph_memset_probe.py): the gradient buffer cleared by a memset NODE
            g = self.optimizer.flat_grad
            N.call('tss_memset_zero', N.ptr(g), g.numel() * g.element_size(), N.stream())
            self.shadows.refresh()
        elif not self.shadows.refresh(zero=self.optimizer.flat_grad if self.flat else None):
            self.optimizer.zero_grad()
        if self._one is None or self._one.device != x.device:
            self._one = torch.ones((), dtype=torch.float32, device=x.device)     # d(loss)/d(loss): no fill launch per step
        with ops.direct_grads(self.flat), self.shadows:
            if self.fuse_head_loss and not (self.model._forward_hooks or self.model._forward_pre_hooks):
                low = self.model.forward_lowres(x)
                if self.teacher is not None:     # two consumers: the head loss and the distillation term
                    low, low_kd = ops.two_consumers(ops.to_nhwc(ops.materialize(low)))
                if type(self.loss_fn) is ops.OHEMLoss:
                    loss = ops.upsample_ohem_loss(low, y, scale_factor=self.model.logit_scale, ignore_index=self.loss_fn.ignore_index,
                                                  thresh_loss=self.loss_fn.thresh_loss, numel_frac=self.loss_fn.numel_frac)
                elif type(self.loss_fn) is ops.FocalLoss:
                    loss = ops.upsample_focal_loss(low, y, scale_factor=self.model.logit_scale, alpha=self.loss_fn.alpha,
                                                   gamma=self.loss_fn.gamma, ignore_index=self.loss_fn.ignore_index,
                                                   variant=self.loss_fn.variant)
                elif type(self.loss_fn) is ops.DiceLoss:
                    loss = ops.upsample_dice_loss(low, y, self.loss_fn.num_classes, scale_factor=self.model.logit_scale,
                                                  smooth=self.loss_fn.smooth, ignore_index=self.loss_fn.ignore_index)
                else:
                    groups = {}
                    if getattr(self.loss_fn, 'sample_group', None) is not None:      # CrossEntropyLoss.set_sample_groups
                        groups = dict(sample_group=self.loss_fn.sample_group, sample_weight=self.loss_fn.sample_weight,
                                      group_loss_out=self.loss_fn.group_loss_out)
                    head_loss = ops.upsample_cross_entropy
                    if getattr(self.loss_fn, 'pixel_weight', None) is not None:      # CrossEntropyLoss.set_pixel_weight
                        head_loss = ops.upsample_pixel_weighted_cross_entropy
                        groups.update(pixel_weight=self.loss_fn.pixel_weight, pixel_norm=self.loss_fn.pixel_norm)
                    loss = head_loss(low, y, scale_factor=self.model.logit_scale,
                                     ignore_index=self.loss_fn.ignore_index, weight=self.loss_fn.weight,
                                     label_smoothing=self.loss_fn.label_smoothing, **groups)
            elif self.teacher is not None:
                low_kd, y_pred = self._forward_with_lowres(x)
                loss = self.loss_fn(y_pred, y)
            else:
                y_pred = self.model(x)
                loss = self.loss_fn(y_pred, y)
            if self.teacher is not None:
                loss = loss + self.distill_weight * self._distill_term(x, low_kd)
            loss.backward(self._one if (loss.dtype == torch.float32 and loss.dim() == 0 and loss.device == self._one.device) else None)
        return loss

    def _forward_with_lowres(self, x):
        """(low-resolution logits, model(x)) of ONE student forward: the map that model.forward hands to its head is picked up on
        its way out of forward_lowres (a second forward would advance the BatchNorm statistics twice and draw other dropout masks)."""
        seen = []
        inner = self.model.forward_lowres

        def tap(*args, **kwargs):
            low, low_kd = ops.two_consumers(ops.to_nhwc(ops.materialize(inner(*args, **kwargs))))
            seen.append(low_kd)
            return low

        self.model.forward_lowres = tap         # an instance attribute in front of the method, for this call only
        try:
            y_pred = self.model(x)
        finally:
            del self.model.forward_lowres
        if len(seen) != 1:
            raise NotImplementedError('Trainer: distillation needs a model whose forward() goes through forward_lowres() once; %s '
                                      'called it %d times' % (type(self.model).__name__, len(seen)))
        return seen[0], y_pred

    def _distill_term(self, x, low):
        if self._teacher_prep is None:
            self._teacher_prep = EvalPrep(self.teacher, frozen=not (self.ema is not None and self.teacher is self.ema.module))
        with torch.no_grad(), self._teacher_prep:
            t_low = ops.materialize(self.teacher.forward_lowres(x))
        if tuple(t_low.shape) != tuple(low.shape):
            raise NotImplementedError('Trainer: the teacher\'s low-resolution logits are %s, the student\'s %s; distillation of maps of '
                                      'different shapes is not supported (resize the teacher\'s, e.g. with ops.bilinear, in a wrapper)'
                                      % (tuple(t_low.shape), tuple(low.shape)))
        return self.distill_loss(low, t_low)

    def _reduce_and_step(self, captured_reduce=False):
        if captured_reduce:
            pass                # the all-reduce of the flat gradient buffer was replayed with the step
        elif self.world_size > 1 or (dist.is_available() and dist.is_initialized()):
            if self.flat:
                allreduce_mean_(self.optimizer.flat_grad, self.world_size)
            else:
                for p in self.model.parameters():
                    if p.grad is not None:
                        dist.all_reduce(p.grad)
                        p.grad.div_(self.world_size)
        self.optimizer.step()
        if self.ema is not None:
            self.ema.update()

    def new_slots(self, n):
        """`n` fresh input-slot numbers (for a loader that captures one step per staging buffer).  Slot numbers are never
        reused, so a pipeline created after another one was dropped can not inherit its captured steps."""
        first = self._next_slot
        self._next_slot += int(n)
        return list(range(first, first + int(n)))

    def release_slot(self, slot):
        """Drop the captured step and the static input buffers of `slot` (its activations go back to the shared pool)."""
        self._graphs.pop(slot, None)
        self._statics.pop(slot, None)

    def static_batch(self, x, y, slot=0, adopt=False):
        """The (image, target) device buffers the captured step of `slot` reads.  A loader can fill them in place (H2D copy
        straight into them) and pass them to step_async, which then skips its own device-to-device copy.  adopt=True:
        x and y (device tensors) BECOME the static buffers of a slot that has none yet; for a slot that already has
        buffers they must BE those buffers (a captured step reads fixed addresses)."""
        if adopt and slot in self._statics and x.is_cuda and y.is_cuda:
            sx, sy = self._statics[slot]
            if sx.data_ptr() != x.data_ptr() or sy.data_ptr() != y.data_ptr():
                raise RuntimeError('Trainer.static_batch(adopt=True): slot %d already has other input buffers; take fresh '
                                   'slot numbers from Trainer.new_slots() or release_slot() it first' % slot)
        if slot not in self._statics:
            dev = self.device if self.device is not None else x.device
            if adopt and x.is_cuda and y.is_cuda:
                self._statics[slot] = (x, y)
            else:
                self._statics[slot] = (torch.empty(x.shape, dtype=x.dtype, device=dev), torch.empty(y.shape, dtype=y.dtype, device=dev))
        sx, sy = self._statics[slot]
        if tuple(sx.shape) != tuple(x.shape) or tuple(sy.shape) != tuple(y.shape) or sx.dtype != x.dtype or sy.dtype != y.dtype:
            raise ValueError('HIP-graph trainer: the batch shape/dtype is fixed at the first step '
                             f'({tuple(sx.shape)} {sx.dtype}); got {tuple(x.shape)} {x.dtype}')
        if x.data_ptr() != sx.data_ptr():
            sx.copy_(x, non_blocking=True)
        if y.data_ptr() != sy.data_ptr():
            sy.copy_(y, non_blocking=True)
        return sx, sy

    def _capture(self, x, y, slot=0, prologue=None):
        sx, sy = self.static_batch(x, y, slot)
        # warm-up on a side stream (lazily initialised state must exist before capture); buffers that a
        # forward pass mutates (BatchNorm running statistics) are restored so the warm-up leaves no trace
        saved = [(b, b.clone()) for b in self.model.buffers()]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._forward_backward(sx, sy, prologue)
        torch.cuda.current_stream().wait_stream(side)
        with torch.no_grad():
            for b, v in saved:
                b.copy_(v)
        dot = getattr(self, 'debug_dot', None)       # tools/graph_memset_probe.py: hipGraphDebugDotPrint of the captured step
        graph = torch.cuda.CUDAGraph(keep_graph=True) if dot else torch.cuda.CUDAGraph()
        if self._pool is None:
            self._pool = torch.cuda.graph_pool_handle()
        # with a live RCCL process group its watchdog thread polls events while we capture: in the default 'global' capture
        # mode that aborts the capture (seen as a flaky crash); only this thread's calls are checked in 'thread_local' mode
        mode = 'thread_local' if (dist.is_available() and dist.is_initialized() and dist.get_backend() == 'nccl') else 'global'
        with torch.cuda.graph(graph, pool=self._pool, capture_error_mode=mode):
            loss = self._forward_backward(sx, sy, prologue).detach()
            if self.graph_allreduce:
                allreduce_mean_(self.optimizer.flat_grad, self.world_size)
        self._graphs[slot] = (graph, loss)
        self._reduce_captured = self.graph_allreduce
        if dot:
            try:        # the captured hipGraph_t straight to the runtime's own printer
                import ctypes
                hip = ctypes.CDLL('libamdhip64.so')
                hip.hipGraphDebugDotPrint.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint]
                rc = hip.hipGraphDebugDotPrint(ctypes.c_void_p(graph.raw_cuda_graph()), dot.encode(), 1)   # 1 = verbose
                if rc != 0:
                    raise RuntimeError('hipGraphDebugDotPrint returned %d' % rc)
            except Exception as exc:      # noqa: BLE001
                import warnings
                warnings.warn('graph dot dump failed: %s' % exc)

    def step_async(self, x, y, slot=0, prologue=None):
        """One training iteration; returns the loss as a device tensor (no host sync).  `slot` selects one of several
        captured steps (each with its own input buffers, see static_batch); `prologue` is a callable that prepares (x, y)
        on the device and is captured with the step."""
        if self.use_graph and not self._graphs and any(ops._sync_group(m, any_mode=True) is not None for m in self.model.modules()
                                                          if isinstance(m, nn.modules.batchnorm._BatchNorm)):
            # cross-replica BatchNorm puts 2 small collectives per BatchNorm layer inside the step.  RCCL collectives on the
            # capturing stream are recorded into the HIP graph like kernels (validated with a one-rank RCCL group on one
            # MI355X, tests/test_gpu_models.py; a multi-GPU node was not available); collectives of a host-side backend
            # (gloo) cannot be captured, and if the capture fails for any reason the step runs un-captured (correct,
            # ~10^3 host launches per step).
            import warnings
            backend = dist.get_backend() if dist.is_initialized() else None
            dev = next(self.model.parameters()).device
            groups = {id(g): g for g in (ops._sync_group(m, any_mode=True) for m in self.model.modules()
                                         if isinstance(m, nn.modules.batchnorm._BatchNorm)) if g is not None}
            if groups and all(ops._exchange(g, dev) is not None for g in groups.values()):
                # round 4: the statistics cross the ranks INSIDE the finalize kernels (mailboxes over HIP IPC, csrc/xchg.hip): the step
                # contains no collective at all and is captured like any other, whatever the backend of the process group
                pass
            elif backend != 'nccl':
                warnings.warn('SyncBatchNorm over the %s backend: the training step is not captured in a HIP graph' % backend)
                self.use_graph = False
            else:
                self._collectives_in_graph = True
        if self.use_graph and slot not in self._graphs:
            if self._collectives_in_graph or self.graph_allreduce:
                # a step with RCCL collectives inside: if ANY slot's capture fails, every slot runs un-captured from then on
                # (correct, ~10^3 host launches per step) -- one decision per trainer, taken by whichever slot captures first
                try:
                    self._capture(x, y, slot, prologue)
                except Exception as exc:      # noqa: BLE001 -- any capture failure: fall back, loudly
                    import warnings
                    warnings.warn('HIP-graph capture of a step with RCCL collectives failed (%s: %s); running un-captured'
                                  % (type(exc).__name__, exc))
                    self._graphs.clear()
                    self.use_graph = False
                    self._reduce_captured = False
                    torch.cuda.synchronize()
            else:
                self._capture(x, y, slot, prologue)
        elif self.use_graph:
            self.static_batch(x, y, slot)
        if self.use_graph:
            graph, loss = self._graphs[slot]
            graph.replay()
        else:
            loss = self._forward_backward(x, y, prologue).detach()
        self._reduce_and_step(captured_reduce=self.use_graph and self._reduce_captured)
        self.iteration += 1
        return loss

    def update(self, batch):
        """TSS/engine.py:24-39: returns loss.item() (a device->host sync per iteration, as in the reference)."""
        x, y = batch
        if self.device is not None and not self.use_graph:   # graph mode copies straight into the static buffers
            x = x.to(self.device, non_blocking=self.non_blocking)
            y = y.to(self.device, non_blocking=self.non_blocking)
        self.last_loss = self.step_async(x, y).item()
        return self.last_loss

    def run(self, data, max_epochs=1):
        history = []
        for _ in range(max_epochs):
            for batch in data:
                history.append(self.update(batch))
        return history


class HostBatchPipeline:
    """The host side of `update_fn` under load (TSS/engine.py:27: `x.to(device, non_blocking=True)` every iteration): the
    batch of step i+1 crosses PCIe on a copy stream while step i computes, through `depth` device staging slots.  With a
    captured trainer there is one captured step per slot, reading its slot in place: nothing but the graph replay (and the
    optimizer) is launched per step.

    wire = 'f32': float32 NCHW image + int64 target, as the reference's DataLoader delivers them (335 MB per 8 x 3 x 1024 x
           2048 batch -- 6.1 ms over PCIe Gen5, as long as the step itself; hidden, but only just);
    wire = 'u8' : uint8 image (CHW, or HWC as decoded: image_hwc=True) + uint8 target (67 MB); `mean` / `std` are the
           albumentations.Normalize constants (scripts/train_fastscnn.py:62-68), applied on the device by tss_decode_batch_u8
           at the top of the (captured) step.
    augment = ops.TrainAugment(...) (wire 'u8' only), with source_size = (H, W): the loader ships the FULL uint8 frame and label
           map, undecorated; put() draws one (scale, crop origin, flip) row per sample on the host (`generator`: a
           torch.Generator for reproducible draws) and copies the rows with the batch, and tss_augment_batch_u8 writes the
           normalized float32 crop and the int64 target crop at the top of the (captured) step.  example_x / example_y keep the
           CROP shape (what the step reads); mean / std default to the augmentation's.  The rows live in device memory, so one
           captured graph serves every draw.  An augmentation with hsv_p > 0 or a label_map goes through
           tss_augment_batch_u8_ex instead: with hsv_p > 0 put() also draws the batch's colour rows (TrainAugment.draw_color,
           after its geometry rows, from the same generator) into a [B, 4] device buffer per slot; the label table is copied
           to the device once, here.

        pipe = HostBatchPipeline(trainer, example_x_f32, example_y_i64, wire='u8', mean=..., std=...)
        pipe.put(x0, y0)
        for next_batch in loader:          # pinned host tensors (DataLoader(pin_memory=True)); others are pinned by a copy
            pipe.put(*next_batch)          # H2D of the next batch starts now, on the copy stream
            loss = pipe.step()             # waits for the oldest staged batch only, runs the step on it
    """

    def __init__(self, trainer, example_x, example_y, wire='f32', mean=None, std=None, image_hwc=False, depth=2, device=None,
                 augment=None, source_size=None, generator=None):
        if wire not in ('f32', 'u8'):
            raise ValueError("wire must be 'f32' or 'u8'")
        if augment is not None and wire != 'u8':
            raise ValueError("augment needs wire='u8': the device augmentation reads the uint8 frame")
        if augment is not None and source_size is None:
            raise ValueError('augment needs source_size=(H, W), the size of the frames the loader ships')
        self.augment, self.generator, self.params = augment, generator, []
        self.color, self._lut = [], None     # colour rows per slot / the label table: the _ex entry when either is there
        self.trainer, self.wire, self.image_hwc, self.depth = trainer, wire, bool(image_hwc), int(depth)
        dev = device if device is not None else (trainer.device if trainer.device is not None else torch.device('cuda', torch.cuda.current_device()))
        self.device = torch.device(dev)
        B, C, H, W = example_x.shape
        self.geom = (B, C, H, W)
        f32 = lambda: (torch.empty((B, C, H, W), dtype=torch.float32, device=self.device),      # noqa: E731
                       torch.empty((B, H, W), dtype=torch.int64, device=self.device))
        if wire == 'u8':
            import ctypes
            SH, SW = H, W                    # size of the staged frame: the step's own, or the source of the augmentation
            if augment is not None:
                SH, SW = int(source_size[0]), int(source_size[1])
                if tuple(augment.crop_size) != (H, W):
                    raise ValueError('augment.crop_size %s differs from the example batch %s' % (tuple(augment.crop_size), (H, W)))
                augment.check_source((SH, SW))
                mean = augment.mean if mean is None else mean
                std = augment.std if std is None else std
                self.source_size = (SH, SW)
                self.params = [torch.zeros((B, 6), dtype=torch.int32, device=self.device) for _ in range(depth)]
                if augment.hsv_p > 0:
                    if C != 3:
                        raise ValueError('augment.hsv_p > 0 needs a 3-channel image, the example batch has %d' % C)
                    self.color = [torch.zeros((B, 4), dtype=torch.int32, device=self.device) for _ in range(depth)]
                if augment.label_map is not None:
                    self._lut = augment.label_map.to(self.device)
            xs = (B, SH, SW, C) if image_hwc else (B, C, SH, SW)
            self.stage = [(torch.empty(xs, dtype=torch.uint8, device=self.device), torch.empty((B, SH, SW), dtype=torch.uint8, device=self.device))
                          for _ in range(depth)]
            self._mean = (ctypes.c_float * 3)(*([float(v) for v in mean] + [0.0] * 3)[:3]) if mean is not None else None
            self._std = (ctypes.c_float * 3)(*([float(v) for v in std] + [1.0] * 3)[:3]) if std is not None else None
            self.decoded = f32()             # one decoded batch, shared by the slots: written and read inside one step
        else:
            self.stage = [f32() for _ in range(depth)]
            self.decoded = None
        self.slots = trainer.new_slots(depth)         # private slot numbers of this pipeline inside the trainer, never reused
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.ready = [torch.cuda.Event() for _ in range(depth)]
        self.consumed = [torch.cuda.Event() for _ in range(depth)]
        self._keep = [None] * depth          # host tensors stay referenced until their copy has been consumed
        self._head = self._count = 0

    def put(self, x, y):
        """Start the H2D copy of one batch.  Raises when all `depth` slots are still in use."""
        if self._count == self.depth:
            raise RuntimeError('HostBatchPipeline: %d batches already staged; call step() first' % self.depth)
        slot = (self._head + self._count) % self.depth
        sx, sy = self.stage[slot]
        if tuple(x.shape) != tuple(sx.shape) or x.dtype != sx.dtype or tuple(y.shape) != tuple(sy.shape) or y.dtype != sy.dtype:
            raise ValueError('HostBatchPipeline(wire=%r): expected image %s %s and target %s %s, got %s %s / %s %s'
                             % (self.wire, tuple(sx.shape), sx.dtype, tuple(sy.shape), sy.dtype, tuple(x.shape), x.dtype,
                                tuple(y.shape), y.dtype))
        if not x.is_cuda and not x.is_pinned():
            x = x.pin_memory()
        if not y.is_cuda and not y.is_pinned():
            y = y.pin_memory()
        rows = crows = None
        if self.augment is not None:         # this batch's (scale, crop origin, flip) rows travel with it
            rows = self.augment.draw(self.geom[0], self.source_size, generator=self.generator).pin_memory()
            if self.color:                   # ... and its (apply, dh, ds, dv) rows
                crows = self.augment.draw_color(self.geom[0], generator=self.generator).pin_memory()
        self._keep[slot] = (x, y, rows, crows)
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(self.consumed[slot])      # the step that read this slot last has finished with it
            sx.copy_(x, non_blocking=True)
            sy.copy_(y, non_blocking=True)
            if rows is not None:
                self.params[slot].copy_(rows, non_blocking=True)
            if crows is not None:
                self.color[slot].copy_(crows, non_blocking=True)
            self.ready[slot].record(self.copy_stream)
        self._count += 1

    def close(self):
        """Release this pipeline's captured steps and input slots in the trainer (call when the loader is re-created, e.g. per
        epoch); the pipeline can not be used afterwards."""
        torch.cuda.current_stream(self.device).synchronize()
        self.copy_stream.synchronize()
        for s in self.slots:
            self.trainer.release_slot(s)
        self.slots, self.stage, self.decoded, self._keep, self._count = [], [], None, [], 0
        self.params, self.color, self._lut = [], [], None

    def _decode(self, slot):
        sx, sy = self.stage[slot]
        dx, dy = self.decoded
        B, C, H, W = self.geom
        if self.augment is not None:
            SH, SW = self.source_size
            head = (N.ptr(sx), int(self.image_hwc), self._mean, self._std, N.ptr(dx), N.ptr(sy), N.ptr(dy), N.ptr(self.params[slot]))
            if self.color or self._lut is not None:
                N.call('tss_augment_batch_u8_ex', *head, N.ptr(self.color[slot]) if self.color else None, N.ptr(self._lut),
                       B, C, SH, SW, H, W, N.stream())
            else:
                N.call('tss_augment_batch_u8', *head, B, C, SH, SW, H, W, N.stream())
            return
        N.call('tss_decode_batch_u8', N.ptr(sx), int(self.image_hwc), self._mean, self._std, N.ptr(dx), N.ptr(sy), N.ptr(dy),
               B, C, H * W, N.stream())

    def step(self):
        """Run one training step on the oldest staged batch; returns the loss as a device tensor."""
        if self._count == 0:
            raise RuntimeError('HostBatchPipeline.step(): nothing staged; call put() first')
        slot = self._head
        main = torch.cuda.current_stream(self.device)
        main.wait_event(self.ready[slot])
        tslot = self.slots[slot]
        if self.wire == 'u8':
            dx, dy = self.decoded
            self.trainer.static_batch(dx, dy, tslot, adopt=True)
            loss = self.trainer.step_async(dx, dy, slot=tslot, prologue=lambda: self._decode(slot))
        else:
            sx, sy = self.stage[slot]
            self.trainer.static_batch(sx, sy, tslot, adopt=True)
            loss = self.trainer.step_async(sx, sy, slot=tslot)
        self.consumed[slot].record(main)
        self._head = (self._head + 1) % self.depth
        self._count -= 1
        return loss


def create_segmentation_trainer(model, optimizer, loss_fn, device, use_f16=False, logging=True,
                                non_blocking=True, use_graph=False, world_size=None, fuse_head_loss=True,
                                teacher=None, distill_loss=None, distill_weight=1.0, ema=None):
    """Same arguments as TSS/engine.py:22; `teacher`, `distill_loss` and `distill_weight` add a logit-distillation term (Trainer), `ema` a
    ModelEMA updated after every step (teacher=ema.module: a mean teacher).  `use_f16` selects bf16 activations (f32 master parameters), the
    MI355X counterpart of the reference's apex amp O2 branch (TSS/engine.py:32-34); no loss scaling is needed."""
    from .models import set_compute_dtype
    set_compute_dtype(model, torch.bfloat16 if use_f16 else torch.float32)
    if teacher is not None:         # the distillation kernels read student and teacher logits of one dtype
        set_compute_dtype(teacher, torch.bfloat16 if use_f16 else torch.float32)
    if ema is not None:             # the averaged model computes as the model it averages
        set_compute_dtype(ema.module, torch.bfloat16 if use_f16 else torch.float32)
    if world_size is None:
        world_size = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    return Trainer(model, optimizer, loss_fn, device=device, use_graph=use_graph, world_size=world_size,
                   non_blocking=non_blocking, fuse_head_loss=fuse_head_loss, teacher=teacher, distill_loss=distill_loss,
                   distill_weight=distill_weight, ema=ema)


# ----------------------------------------------------------------------------- evaluator

class EvalPrep:
    """Model-wide preparation of an eval-mode forward: bf16 shadows of the 1x1 weights (ops.WeightShadows, one launch), the affines
    of every BatchNorm that runs on its running statistics (ops.EvalAffines, one launch) and the bf16 tap-major copies of the dense
    3x3 weights (ops.Dense3x3Shadows, one small launch per layer).  `with prep:` refreshes them from the live parameters / buffers
    and makes them visible to the layers inside; with `frozen=True` they are refreshed by refresh() only (weights that do not change
    between forwards: the preparation leaves the forward, as `model.half()` leaves the timed loop of TSS/utils/benchmark.py)."""

    def __init__(self, model, frozen=False):
        self.shadows, self.affines, self.w3 = ops.WeightShadows(model), ops.EvalAffines(model), ops.Dense3x3Shadows(model)
        self.frozen, self.fresh = frozen, False

    def refresh(self):
        self.shadows.refresh()
        self.affines.refresh()
        self.w3.refresh()
        self.fresh = True

    def __enter__(self):
        if not (self.frozen and self.fresh):
            self.refresh()
        self.shadows.__enter__()
        self.affines.__enter__()
        self.w3.__enter__()
        return self

    def __exit__(self, *exc):
        self.w3.__exit__(*exc)
        self.affines.__exit__(*exc)
        self.shadows.__exit__(*exc)
        return False


class Evaluator:
    """model.eval() + no_grad forward, argmax, confusion matrix -> IoU / mIoU / accuracy / Dice
    (the metrics of create_segmentation_evaluator, TSS/engine.py:59-82; confusion rows = truth)."""

    def __init__(self, model, device=None, num_classes=19, loss_fn=None, ignore_index=255, non_blocking=True):
        self.model, self.device, self.num_classes = model, device, num_classes
        self.loss_fn, self.ignore_index, self.non_blocking = loss_fn, ignore_index, non_blocking

    @torch.no_grad()
    def run(self, data):
        self.model.eval()
        cm = None
        loss_sum, n = 0.0, 0
        prep = None
        for x, y in data:
            if self.device is not None:
                x = x.to(self.device, non_blocking=self.non_blocking)
                y = y.to(self.device, non_blocking=self.non_blocking)
            if prep is None:
                prep = EvalPrep(self.model)
            with prep:
                cm, loss_sum, n = self._batch(x, y, cm, loss_sum, n)
        metrics = confusion_metrics(cm.cpu().double())
        if self.loss_fn is not None and n:
            metrics['loss'] = loss_sum / n
        return metrics

    def _batch(self, x, y, cm, loss_sum, n):
        fused = (self.loss_fn is None and hasattr(self.model, 'forward_lowres') and hasattr(self.model, 'logit_scale')
                 and not (self.model._forward_hooks or self.model._forward_pre_hooks))
        if fused:   # decoder upsample + argmax + confusion matrix as one operator: no full-resolution logits
            low = self.model.forward_lowres(x)
            _, cm = ops.upsample_argmax_confusion(low, y, scale_factor=self.model.logit_scale,
                                                  ignore_index=self.ignore_index, confusion=cm, want_pred=False)
            return cm, loss_sum, n
        logits = self.model(x)
        _, cm = ops.argmax_confusion(logits, y, ignore_index=self.ignore_index, confusion=cm, want_pred=False)
        if self.loss_fn is not None:
            loss_sum += float(self.loss_fn(logits, y)) * x.shape[0]
            n += x.shape[0]
        return cm, loss_sum, n


def confusion_metrics(cm):
    tp = cm.diag()
    iou = tp / (cm.sum(0) + cm.sum(1) - tp + 1e-15)
    return {'iou': iou, 'miou': iou.mean().item(), 'accuracy': (tp.sum() / (cm.sum() + 1e-15)).item(),
            'dice': 2 * tp / (cm.sum(0) + cm.sum(1) + 1e-15)}


class MultiScaleEvaluator:
    """Multi-scale + horizontal-flip evaluation, the protocol of the published Cityscapes numbers: per batch, the image is resized to
    every scale (sides rounded to a multiple of `size_multiple`), each scale runs once through `model.forward_lowres` as a 2B batch of
    the plain and the mirrored image (ops.resize_flip_image), and ONE ops.multiscale_argmax_confusion call upsamples the maps to
    the target's size, mirrors the flipped ones back, sums the per-map softmax (average='softmax') or logits ('logits') and updates
    the confusion matrix.  No full-resolution logits, no ATen arithmetic, no host synchronisation inside a batch.
    Same run(data) and metric dict as Evaluator; predict(x) returns the uint8 label map."""

    def __init__(self, model, device=None, num_classes=19, scales=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75), flip=True, size_multiple=32,
                 average='softmax', ignore_index=255, non_blocking=True):
        if not (hasattr(model, 'forward_lowres') and hasattr(model, 'logit_scale')):
            raise NotImplementedError('MultiScaleEvaluator needs a model with forward_lowres() and logit_scale (the low-resolution '
                                      'logits of the decoder head); %s has none' % type(model).__name__)
        scales = tuple(float(s) for s in scales)
        if not scales or min(scales) <= 0:
            raise ValueError('scales must be a non-empty sequence of positive factors, got %r' % (scales,))
        if len(scales) * (2 if flip else 1) > ops.MULTISCALE_MAX_MAPS:
            raise ValueError('%d scales%s are more than the %d maps one fused call takes'
                             % (len(scales), ' with flip' if flip else '', ops.MULTISCALE_MAX_MAPS))
        if average not in ('softmax', 'logits'):
            raise ValueError("average must be 'softmax' or 'logits', got %r" % (average,))
        self.model, self.device, self.num_classes = model, device, num_classes
        self.scales, self.flip, self.size_multiple = scales, bool(flip), int(size_multiple)
        self.average, self.ignore_index, self.non_blocking = average, ignore_index, non_blocking
        self._prep = None
        self.confusion = None      # the int64 [C, C] matrix of the last run(), on the device

    def scaled_size(self, H, W, s):
        m = self.size_multiple
        return max(m, int(round(H * s / m)) * m), max(m, int(round(W * s / m)) * m)

    @torch.no_grad()
    def lowres_maps(self, x):
        """(lows, flips) as ops.multiscale_argmax_confusion takes them: the low-resolution logits of the device batch x at every
        scale (a 2B batch each with flip), under the shared EvalPrep."""
        H, W = x.shape[-2:]
        if self._prep is None:
            self._prep = EvalPrep(self.model)
        lows = []
        with self._prep:
            for s in self.scales:
                xs = ops.resize_flip_image(x, self.scaled_size(H, W, s), flip=self.flip)   # float32, as Evaluator feeds the image
                low = self.model.forward_lowres(xs)
                if low.shape[1] != self.num_classes:
                    raise ValueError('the model scores %d classes, the evaluator was built for num_classes=%d'
                                     % (low.shape[1], self.num_classes))
                lows.append(low)
        return lows, [(False, True) if self.flip else False] * len(lows)

    @torch.no_grad()
    def predict(self, x):
        self.model.eval()
        if self.device is not None:
            x = x.to(self.device, non_blocking=self.non_blocking)
        lows, flips = self.lowres_maps(x)
        pred, _ = ops.multiscale_argmax_confusion(lows, flips, size=tuple(x.shape[-2:]), ignore_index=self.ignore_index,
                                                  average=self.average)
        return pred

    @torch.no_grad()
    def run(self, data):
        self.model.eval()
        cm = None
        for x, y in data:
            if self.device is not None:
                x = x.to(self.device, non_blocking=self.non_blocking)
                y = y.to(self.device, non_blocking=self.non_blocking)
            lows, flips = self.lowres_maps(x)
            _, cm = ops.multiscale_argmax_confusion(lows, flips, y, size=tuple(y.shape[-2:]), ignore_index=self.ignore_index,
                                                    confusion=cm, want_pred=False, average=self.average)
        if cm is None:
            raise ValueError('MultiScaleEvaluator.run got no batches: there is nothing to score')
        self.confusion = cm
        return confusion_metrics(cm.cpu().double())


def create_segmentation_evaluator(model, device, num_classes=19, loss_fn=None, non_blocking=True, scales=None, flip=False,
                                  size_multiple=32, average='softmax', ignore_index=255):
    """`scales` given: the multi-scale (+ `flip`) protocol (MultiScaleEvaluator, which also takes `size_multiple` and `average`; it
    reports no loss); otherwise the single forward."""
    if scales is not None:
        if loss_fn is not None:
            raise ValueError('the multi-scale evaluator has no full-resolution logits to feed a loss_fn')
        return MultiScaleEvaluator(model, device, num_classes=num_classes, scales=scales, flip=flip, size_multiple=size_multiple,
                                   average=average, ignore_index=ignore_index, non_blocking=non_blocking)
    return Evaluator(model, device, num_classes=num_classes, loss_fn=loss_fn, ignore_index=ignore_index, non_blocking=non_blocking)


# ----------------------------------------------------------------------------- deep supervision (row S)

class DeepSupervisionWrapper(nn.Module):
    """Forward hooks on inner blocks feed auxiliary heads in training mode
    (TSS/wrappers/deep_supervision_wrapper.py:10-43): train -> (output, [aux...]); eval -> output."""

    def __init__(self, module, auxiliary_modules):
        super().__init__()
        self.module = module
        self.layers = [layer for layer, _ in auxiliary_modules]
        self.auxiliary = nn.ModuleList([head for _, head in auxiliary_modules])

    def forward(self, input):
        if not self.training:
            return self.module(input)
        aux_outputs = [None] * len(self.layers)

        def capture(_module, _inputs, output, slot, head):
            aux_outputs[slot] = head(output)

        handles = [layer.register_forward_hook(partial(capture, slot=i, head=head))
                   for i, (layer, head) in enumerate(zip(self.layers, self.auxiliary))]
        try:
            output = self.module(input)
        finally:
            for h in handles:
                h.remove()
        return output, aux_outputs


# ----------------------------------------------------------------------------- inference (TSS/utils/benchmark.py)

class GraphedInference:
    """eval-mode, no-grad forward of `model` captured once in a HIP graph and replayed: the input is copied into a fixed
    device buffer, the returned logits live in a fixed output buffer (overwritten by the next call).  Shapes are fixed
    at the first call.  `lowres=True` returns the 1/8-resolution logits of `model.forward_lowres` (what the fused
    evaluation head consumes) instead of the x8-upsampled ones.
    `frozen_weights=False` (default): the model-wide weight / statistics preparation (EvalPrep) is captured with the layers, so every
    replay follows the live parameters and buffers.  `frozen_weights=True`: it runs once, before the capture, and again only when
    refresh_weights() is called -- for deployed models whose weights do not change between forwards."""

    def __init__(self, model, lowres=False, frozen_weights=False):
        self.model, self.lowres, self.frozen = model, lowres, bool(frozen_weights)
        self._graph = self._x = self._out = self._prep = None

    def refresh_weights(self):
        """Re-run the weight / statistics preparation after the parameters or buffers changed (frozen_weights=True only)."""
        if self._prep is not None:
            self._prep.refresh()

    def _forward(self, x):
        if self._prep is None:
            self._prep = EvalPrep(self.model, frozen=self.frozen)
        with self._prep:      # model-wide preparation launches: captured with the rest (live weights) unless frozen_weights
            return self.model.forward_lowres(x) if self.lowres else self.model(x)

    def static_input(self, x):
        """The device buffer the captured forward reads: fill it in place (H2D copy straight into it) and pass it to
        __call__, which then skips its own device-to-device copy."""
        if self._x is None:
            self._x = torch.empty_like(x)
        if x.data_ptr() != self._x.data_ptr():
            self._x.copy_(x, non_blocking=True)
        return self._x

    @torch.no_grad()
    def __call__(self, x):
        if self._graph is None:
            self.model.eval()
            self.static_input(x)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    self._forward(self._x)
            torch.cuda.current_stream().wait_stream(side)
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self._out = self._forward(self._x)
        elif tuple(x.shape) != tuple(self._x.shape) or x.dtype != self._x.dtype:
            raise ValueError(f'GraphedInference: input fixed at {tuple(self._x.shape)} {self._x.dtype}, got {tuple(x.shape)} {x.dtype}')
        if x.data_ptr() != self._x.data_ptr():
            self._x.copy_(x, non_blocking=True)
        self._graph.replay()
        return self._out


def benchmark_model(model, batch, iterations, warmup, use_graph=False):
    """Same arguments and result keys as TSS/utils/benchmark.py:6-33 (fps / min / max / mean / std of the forward time
    in seconds, gradients disabled).  Each iteration is bracketed by a device synchronisation -- kernels are
    asynchronous, the reference's host-side `time()` pair only measures a GPU model if something blocks.  The caller
    chooses train/eval mode as in the reference; `use_graph` replays a captured eval forward (GraphedInference)."""
    import time
    import numpy as np
    fwd = GraphedInference(model) if use_graph else model
    cuda = batch.is_cuda
    record = np.zeros(iterations)
    with torch.set_grad_enabled(False):
        for _ in range(warmup):
            fwd(batch)
        for it in range(iterations):
            if cuda:
                torch.cuda.synchronize()
            start = time.perf_counter()
            fwd(batch)
            if cuda:
                torch.cuda.synchronize()
            record[it] = time.perf_counter() - start
    return {'fps': 1 / np.mean(record), 'min': np.min(record), 'max': np.max(record), 'mean': np.mean(record),
            'std': np.std(record)}
