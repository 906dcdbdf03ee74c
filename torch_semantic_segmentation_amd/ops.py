"""Autograd operators of the HIP path: thin Python glue over include/tss_hip.h.

Design: a convolution stores its output RAW.  The BatchNorm(+ReLU) that follows it in the
reference's blocks (TSS/models/fastscnn.py:164-199, TSS/models/contextnet.py:150-177) is carried as a
`Deferred` (raw tensor + per-channel affine + relu flag) and applied by the consumer while it loads its
input; a normalised activation is only written where the reference needs a real tensor (block outputs,
residual sums) by `join`.  Backward mirrors it: between two of these operators the tensor handed back
through autograd for a raw conv output is e = d(loss)/d(BN output), already ReLU-masked, and the
BatchNorm backward (which needs two per-channel sums over e) is applied on load by the producer's
backward kernels from coefficients finalised out of `BNLink.bstats`.  Tensors that leave a block are
ordinary tensors with ordinary gradients.

There is no torch/ATen fallback here: every operator calls the C ABI and raises if it is unavailable.
"""
import collections
import ctypes
import math
import os
import threading

import torch
from torch.autograd import Function
from torch.nn.modules.batchnorm import _BatchNorm

from . import _native as N

call, ptr, stream = N.call, N.ptr, N.stream


# ----------------------------------------------------------------------------- direct gradient accumulation

_DIRECT = [False]


class direct_grads:
    """While active, parameter gradients are accumulated by the kernels straight into an existing float32
    `.grad` (e.g. FlatAdamW's flat buffer) and autograd is handed None for them: no per-parameter zero-fill
    and no `.grad +=` launch.  Off by default: then every backward returns ordinary gradient tensors."""

    def __init__(self, enabled=True):
        self.enabled = bool(enabled)

    def __enter__(self):
        self.prev = _DIRECT[0]
        _DIRECT[0] = self.enabled
        return self

    def __exit__(self, *exc):
        _DIRECT[0] = self.prev
        return False


# Launch a layer's weight gradient on a side stream, concurrently with its input gradient (ConvUnitFn.backward).
overlap_wgrad = os.environ.get('TSS_OVERLAP_WGRAD', '0') == '1'   # measured: no gain on MI355X once the kernels are pipelined (9.88 ms off vs 9.84-9.95 ms on)
# depthwise layers: input gradient and weight gradient from one kernel (tss_dwconv3x3_bwd_fused) instead of two launches.
# Opt-in: correct, reads e / y / x once, but measured slower on MI355X (1 wave/SIMD, see dwconv.hip): 7.28 vs 7.05 ms/step.
fuse_dw_backward = os.environ.get('TSS_FUSE_DW_BWD', '0') == '1'
overlap_max_elems = int(os.environ.get('TSS_OVERLAP_MAX', str(48 << 20)))   # only layers too small to fill the chip on their own (large ones just contend)
overlap_min_elems = int(os.environ.get('TSS_OVERLAP_MIN', '0'))
# the row reductions of the one-sweep depthwise backward, collected over a backward pass and summed in one launch at its end
# (only for gradients written straight into their final buffer: a gradient RETURNED to autograd must be complete on return)
batch_dw_reductions = os.environ.get('TSS_BATCH_DW_REDUCE', '1') == '1'
fuse_pw_backward = os.environ.get('TSS_PW_BWD_FUSED', '1') != '0'     # csrc/pwbwd.hip, for the layers it prefers
sweep_pw_backward = os.environ.get('TSS_PW_SWEEP', '1') != '0'        # csrc/pwsweep.hip: the large 1x1 layers, one sweep (round 4)
# Backward-pass scheduling ("launch count"): every dependent launch costs >= 4.7 us in the replayed step, so
#   * the weight gradient of a 1x1 layer -- which nothing downstream in the backward pass depends on -- is POSTPONED until the
#     next BatchNorm-backward finalize is due, and that finalize rides in front of its grid (tss_pwconv_bwd_weight's `fin`);
#   * the slot reduction of a launched weight gradient rides in front of the next backward-data grid of ANY 1x1 layer.
# Everything left over is flushed by the end-of-pass callback, so gradients are complete when backward() returns (and not before:
# see direct_grads).
postpone_wgrad = os.environ.get('TSS_POSTPONE_WGRAD', '1') != '0'
# weight gradient of the three-tap (1x3 / 3x1) layers: unfold + the pipelined pointwise kernel (0: the generic tap-loop kernel)
unfold_1d_wgrad = os.environ.get('TSS_FC1D_WGRAD', '1') != '0'
# stem weight gradient: y recomputed from the taps and the weights inside the kernel instead of read back (csrc/stem.hip,
# tss_stem3x3_bwd_weight_rc; the same bits, a third less memory traffic).  0: the kernel that reads y.
stem_wgrad_recompute = os.environ.get('TSS_STEM_WGRAD_RC', '1') != '0'
_CONST_ROWS = {}


def _per_device(cache, dev, make, stale=lambda got: False):
    """cache[dev], filled by make() on first use (and again when stale(entry)): one entry per (device type, index)."""
    key = (dev.type, dev.index)
    if key not in cache or stale(cache[key]):
        cache[key] = make()
    return cache[key]


def _const_rows(dev, n):
    """(ones, zeros) f32 rows of at least n channels on `dev`: BatchNorm-backward coefficients of a layer that has none."""
    m = max(768, n)
    return _per_device(_CONST_ROWS, dev, lambda: (torch.ones(m, dtype=torch.float32, device=dev), torch.zeros(m, dtype=torch.float32, device=dev)),
                       stale=lambda got: got[0].numel() < n)
# Layers that run inside a two-stream region of the forward pass (ContextNet's branches, `overlap_region`) are not postponed: there
# the other stream's kernels already fill the launch gaps, and what postponing leaves for the end of the pass (a weight gradient and
# its slot reduction per stream, un-overlapped) costs more than the finalize launches it saves (measured: 6.32 vs 6.21 ms per step).
_overlap_depth = [0]
postpone_in_overlap = os.environ.get('TSS_POSTPONE_OVERLAPPED', '0') == '1'     # A/B: postpone inside two-stream regions too


class _Pass:
    """Scheduling state of ONE running backward pass (one autograd graph task).  Round 4: the state used to be module-global and
    was cleared whenever the graph-task id changed, so a nested pass (torch.utils.checkpoint(use_reentrant=True), a hook calling
    torch.autograd.grad) silently deleted the OUTER pass's postponed weight gradients and row reductions.  Now every graph task has
    its own: a nested pass postpones, flushes and completes its own work, the outer one keeps its own.
    `wg` / `red` are keyed by the stream the postponed work belongs to: a model whose branches run on two streams (ContextNet) has
    two independent backward chains, and a launch postponed on one stream must neither ride on nor carry work of the other."""
    __slots__ = ('dw', 'wg', 'red')

    def __init__(self):
        self.dw = []        # (ws, dw, ncols, nrows): row reductions for the one launch at the end of the pass
        self.wg = {}        # stream id -> (launch(fin_job or None), device, stream)
        self.red = {}       # stream id -> (ws, dw, P, K, N, device, stream)


_passes = {}                # graph-task id -> _Pass
_lock = threading.RLock()   # two trainers in two threads (each with its own autograd device thread) share this module


class BnBwdJob(ctypes.Structure):
    """tss_bn_bwd_job of include/tss_hip.h."""
    _fields_ = [('bstats', ctypes.c_void_p), ('count', ctypes.c_double), ('invstd', ctypes.c_void_p), ('gamma', ctypes.c_void_p),
                ('training', ctypes.c_int), ('accumulate', ctypes.c_int), ('dgamma', ctypes.c_void_p), ('dbeta', ctypes.c_void_p),
                ('ga', ctypes.c_void_p), ('gb', ctypes.c_void_p), ('gce', ctypes.c_void_p), ('C', ctypes.c_int),
                ('xchg_world', ctypes.c_int), ('xchg_rank', ctypes.c_int), ('xchg_peers', ctypes.c_void_p * 8), ('xchg_counters', ctypes.c_void_p)]


def _backward_task():
    """Id of the running autograd graph task (-1: none, or nothing can be deferred).  The first call of a pass creates its state and
    queues its end-of-pass flush on THAT graph task."""
    try:
        task = torch._C._current_graph_task_id()
    except AttributeError:          # private API gone: nothing is deferred
        return -1
    if task == -1:
        return -1
    with _lock:
        if task not in _passes:
            try:
                torch.autograd.variable.Variable._execution_engine.queue_callback(lambda _t=task: _end_of_backward(_t))
            except Exception:           # noqa: BLE001 -- no callback, no deferral
                return -1
            # state of passes that raised before their callback ran is void; graph-task ids only grow, and a running outer pass of a
            # nested one is never more than a few ids behind: keep the newest 16
            for old in sorted(_passes)[:-15]:
                del _passes[old]
            _passes[task] = _Pass()
    return task


def _cur_pass():
    task = _backward_task()
    return _passes.get(task) if task != -1 else None


def _flush_wg(sid=None, ps=None):
    """Launch postponed weight gradients now, without a rider, each on the stream it belongs to (sid: only that stream's)."""
    ps = ps if ps is not None else _cur_pass()
    if ps is None:
        return
    for k in ([sid] if sid is not None else list(ps.wg)):
        with _lock:
            ent = ps.wg.pop(k, None)
        if ent is not None:
            launch, dev, st_ = ent
            with torch.cuda.device(dev), torch.cuda.stream(st_):
                launch(None)


def _flush_red(sid=None, ps=None):
    ps = ps if ps is not None else _cur_pass()
    if ps is None:
        return
    for k in ([sid] if sid is not None else list(ps.red)):
        with _lock:
            ent = ps.red.pop(k, None)
        if ent is not None:
            ws, dw, P, K, Nn, dev, st_ = ent
            with torch.cuda.device(dev), torch.cuda.stream(st_):
                call('tss_pwconv_wg_reduce', ptr(ws), ptr(dw), P, K, Nn, stream())


def _take_red(dev):
    """(ws ptr, dw ptr, P, K, N) of a slot reduction waiting for a carrier on THIS stream (else NULLs) + its tensors (kept alive by the caller)."""
    ps = _cur_pass()
    ent = None
    if ps is not None:
        with _lock:
            ent = ps.red.pop(stream(), None)
    if ent is not None:
        ws, dw, P, K, Nn = ent[:5]
        return (ptr(ws), ptr(dw), P, K, Nn), (ws, dw)
    return (None, None, 0, 0, 0), None


def _end_of_backward(task):
    with _lock:
        ps = _passes.pop(task, None)
    if ps is None:
        return
    _flush_wg(ps=ps)
    _flush_red(ps=ps)
    # the row reductions below run on the current stream: order it behind the side streams whose kernels wrote some of the rows
    # (the autograd engine joins its leaf streams only AFTER the final callbacks)
    if ps.dw and _side_streams:
        cur = torch.cuda.current_stream()
        for s_ in _side_streams.values():
            if s_.device == cur.device:
                cur.wait_stream(s_)
    _flush_dw_reductions(ps)


def _bn_bwd_finalize(link, C, acc, dgamma, dbeta, st, training=None):
    """BatchNorm-backward coefficients + d(gamma), d(beta) of `link`: in front of a postponed weight-gradient grid of the same
    stream (and the same pass) when there is one (no launch of its own), else tss_bn_bwd_finalize.  A cross-replica BatchNorm
    (link.sync): the sums cross the ranks inside the same finalize blocks, riding or not (IPC exchange, csrc/xchg.hip) -- or, without
    the exchange, through the process group's all-reduce."""
    training = int(link.training if training is None else training)
    ex = None
    if link.sync is not None:
        ex = _exchange(link.sync, link.bstats.device) if C <= 768 else None
        if ex is None:
            _flush_wg(st)
            gs = _allreduce_stats(link.bstats, link.count, C, link.sync, st)
            call('tss_bn_bwd_finalize_sync', ptr(link.bstats), ptr(gs), ptr(link.invstd), ptr(link.gamma), int(acc),
                 ptr(dgamma), ptr(dbeta), ptr(link.ga), ptr(link.gb), ptr(link.gce), C, st)
            return
    ps = _cur_pass()
    ent = None
    if ps is not None:
        with _lock:
            ent = ps.wg.get(st)
            if ent is not None and ent[1] == link.bstats.device:
                ps.wg.pop(st, None)
            else:
                ent = None
    if ent is not None:
        job = BnBwdJob(ptr(link.bstats), float(link.count), ptr(link.invstd), ptr(link.gamma), training, int(acc),
                       ptr(dgamma), ptr(dbeta), ptr(link.ga), ptr(link.gb), ptr(link.gce), int(C))
        if ex is not None:
            job.xchg_world, job.xchg_rank, job.xchg_counters = ex.world, ex.rank, ptr(ex.counters)
            for r_ in range(ex.world):
                job.xchg_peers[r_] = ex.peers[r_]
        ent[0](job)
        return
    if ex is not None:
        call('tss_bn_bwd_finalize_xchg', ptr(link.bstats), float(link.count), ex.peers, ex.rank, ex.world, ptr(ex.counters),
             ptr(link.invstd), ptr(link.gamma), int(acc), ptr(dgamma), ptr(dbeta), ptr(link.ga), ptr(link.gb), ptr(link.gce), C, st)
        return
    call('tss_bn_bwd_finalize', ptr(link.bstats), float(link.count), ptr(link.invstd), ptr(link.gamma), training, int(acc),
         ptr(dgamma), ptr(dbeta), ptr(link.ga), ptr(link.gb), ptr(link.gce), C, st)


def _bn_backward_prologue(link, has_affine, p_gamma, p_beta, C, y, dev, st):
    """What the backward of a unit with a BatchNorm behind it does first: d(gamma) / d(beta) targets (the parameters' own .grad under
    direct_grads, else one fresh pair), the finalize, and the coefficients its kernels apply on load.
    Returns (d(gamma), d(beta) for autograd -- None when accumulated directly --, y, ga, gb, gce, mean); a frozen BatchNorm needs
    neither y nor gb / gce / mean (None), a unit without BatchNorm (link None) none of them."""
    if link is None:
        return None, None, None, None, None, None, None
    dgamma = dbeta = None
    acc = 0
    if has_affine:
        dgamma, dbeta = _direct_target(p_gamma), _direct_target(p_beta)
        if dgamma is not None and dbeta is not None:
            acc = 1
        else:
            dgb = torch.empty((2, C), dtype=torch.float32, device=dev)
            dgamma, dbeta = dgb[0], dgb[1]
    _bn_bwd_finalize(link, C, acc, dgamma, dbeta, st)       # (local or cross-replica statistics: link.sync)
    if acc:
        dgamma = dbeta = None
    if not link.training:
        return dgamma, dbeta, None, link.ga, None, None, None
    return dgamma, dbeta, y, link.ga, link.gb, link.gce, link.mean


def _flush_dw_reductions(ps):
    with _lock:
        jobs = list(ps.dw)
        del ps.dw[:]
    if not jobs:
        return
    n = len(jobs)
    ws = (ctypes.c_void_p * n)(*[j[0].data_ptr() for j in jobs])
    dw = (ctypes.c_void_p * n)(*[j[1].data_ptr() for j in jobs])
    cols = (ctypes.c_int * n)(*[j[2] for j in jobs])
    rows = (ctypes.c_int * n)(*[j[3] for j in jobs])
    with torch.cuda.device(jobs[0][0].device):
        call('tss_dw_reduce_many', n, ws, dw, cols, rows, stream())


def _reduce_rows_now(ws, dw, ncols, nrows):
    a, b = (ctypes.c_void_p * 1)(ws.data_ptr()), (ctypes.c_void_p * 1)(dw.data_ptr())
    call('tss_dw_reduce_many', 1, a, b, (ctypes.c_int * 1)(ncols), (ctypes.c_int * 1)(nrows), stream())


def _param_observed(p):
    """A parameter whose gradient somebody may read BEFORE backward() returns (tensor hooks, post-accumulate-grad hooks, e.g. a
    bucketed all-reduce that overlaps the backward pass): its weight gradient is completed in place, never deferred."""
    return p is not None and bool(getattr(p, '_backward_hooks', None) or getattr(p, '_post_accumulate_grad_hooks', None))


def _defer_dw_reduction(ws, dw, ncols, nrows, param=None):
    """Queue the row reduction of a one-sweep backward for the single launch at the end of the pass (now, if nothing can be deferred).
    Contract of the deferral (and of the postponed 1x1 weight gradients): directly accumulated gradients are complete when backward()
    returns, not earlier -- except for parameters with hooks, which are finished at once."""
    ps = _cur_pass()
    if ps is None or _param_observed(param):
        _reduce_rows_now(ws, dw, ncols, nrows)
        return
    if ps.dw and ps.dw[0][0].device != ws.device:
        _flush_dw_reductions(ps)
    with _lock:
        ps.dw.append((ws, dw, ncols, nrows))


def _add_rows(ws, target, ncols, nrows, param, returned):
    """target += the nrows rows of per-block partial sums in ws: queued for the one launch at the end of the pass when `target` is
    the parameter's own gradient buffer (returned None), at once when it goes back to autograd (complete on return)."""
    if returned is None and batch_dw_reductions:
        _defer_dw_reduction(ws, target, ncols, nrows, param)
    else:
        _reduce_rows_now(ws, target, ncols, nrows)


# Residual blocks: the block input has two consumers (the first 1x1 layer and the skip), so its gradient is a sum of two tensors.
# Autograd would add them with an elementwise launch of its own; instead the skip's gradient (produced first, by the join's
# backward) is handed to the first layer's backward-data kernel, which adds it in its epilogue (tss_pwconv_bwd_data_radd).
fold_residual_adds = os.environ.get('TSS_FOLD_RESIDUAL', '1') != '0'


class _Fork:
    __slots__ = ('g2', 'consumed', 'prev_join', '__weakref__')      # (__weakref__: only the tests use it, to watch a fork die)

    def __init__(self):
        self.g2, self.consumed, self.prev_join = None, False, None


# A producer's note for the operator that consumes its output travels ON the tensor, as a private attribute: it dies with the
# tensor, and no other tensor, operator or thread can see it.  (Views, detach() and copies do not inherit it.)
_FORK, _STASH, _JOIN = '_tss_fork', '_tss_stash', '_tss_join'


def _hand(t, key, value):
    """Leave `value` on tensor `t` for its consumer.  `value` may hold other tensors (a join's j_a, a fork's g2) but must never
    reference `t` itself: the pair would then only die when the garbage collector runs."""
    setattr(t, key, value)


def _take(t, key):
    """The note left on `t` under `key`, removed from it (a second consumer of `t` finds nothing), or None."""
    return t.__dict__.pop(key, None)


class ForkFn(Function):
    """x -> (x, x): two handles of one tensor whose gradients meet here.  If the consumer of the first handle has already added the
    second handle's gradient into its own (fork.consumed), that sum is passed on as it is."""

    @staticmethod
    def forward(ctx, x, fork):
        ctx.fork = fork
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, ga, gb):
        fork = ctx.fork
        consumed = fork.consumed
        fork.g2, fork.consumed = None, False
        if ga is None:
            return gb, None
        if gb is None or consumed:
            return ga, None
        return ga + gb, None


def residual_fork(x):
    """(handle for the convolution path, handle for the skip, fork) of a residual block's input; (x, x, None) when nothing is folded.
    The fork rides on the first handle as a note for the operator that consumes it; a handle nobody consumes takes its note with it."""
    if not (fold_residual_adds and torch.is_grad_enabled() and torch.is_tensor(x) and x.requires_grad and x.is_cuda
            and x.dtype == torch.bfloat16 and not N.fast_paths_disabled()):
        return x, x, None
    fork = _Fork()
    fork.prev_join = _take_join(x)         # x is a block output: its join's backward can ride in the first layer's backward-data launch
    xa, xb = ForkFn.apply(x, fork)
    _hand(xa, _FORK, fork)                 # taken by the first operator that consumes xa (conv_unit, adaptive_avg_pool_multi)
    return xa, xb, fork


# A relu join whose output feeds a 1x1 layer (block output -> the next block's expand conv): the join's backward (ReLU mask of its
# output + the BatchNorm-backward sums) can run in the epilogue of that layer's backward-data launch (tss_pwconv_bwd_data_joined).
# join() leaves its configuration on the output tensor; the consuming conv unit takes it.
fuse_join_backward = os.environ.get('TSS_FUSE_JOIN_BWD', '1') != '0'
# ... for block outputs up to this many elements: the two extra loads of the epilogue drain the next tile's prefetch, which costs a long
# layer more than the join launch it saves (262 k pixels x 64 channels: +48 us against a 28 us join; 65 k x 64: +10 against 14;
# 16 k x 96-128: +2 against 9)
fuse_join_backward_max = int(os.environ.get('TSS_FUSE_JOIN_BWD_MAX', '4000000'))


def _take_join(x):
    return _take(x, _JOIN) if torch.is_tensor(x) else None


def fork_two(x):
    """(xa, xb, fork) for a materialised activation with TWO consumers whose gradients would otherwise meet in an elementwise launch of
    autograd's: the consumer of xb (created later, so its backward runs first) leaves its input gradient in fork.g2, the 1x1 layer
    that consumes xa adds it in the epilogue of its backward-data kernel (tss_pwconv_bwd_data_radd) -- or, for pooled maps,
    tss_ppm_pool_bwd does.  Falls back to autograd's add whenever a side cannot take part.  (x, x, None) when nothing is folded.
    Both requests ride on the handles themselves (the fork on xa, the stash on xb): a consumer outside the envelope leaves its note
    where it is, and the note goes with the handle."""
    xa, xb, fork = residual_fork(x)
    if fork is not None:
        _hand(xb, _STASH, fork)                # taken by the operator that consumes xb (conv_unit, concat_upsampled_arms)
    return xa, xb, fork


# independent branches of a model (ContextNet's spatial / context branches) on two streams: parallel branches of the captured graph
overlap_branches = os.environ.get('TSS_OVERLAP_BRANCHES', '1') != '0'     # measured: ContextNet14 step 6.34 -> 6.27 ms


class overlap_region:
    """Marks the part of a forward pass whose layers run on two streams at once (see _overlap_depth)."""

    def __enter__(self):
        _overlap_depth[0] += 1
        return self

    def __exit__(self, *exc):
        _overlap_depth[0] -= 1
        return False


def tensors_of(x):
    """The device tensors behind an activation (a tensor, or a Deferred with its BatchNorm link)."""
    if isinstance(x, Deferred):
        out = [x.raw]
        if x.link is not None:
            out += [x.link.vec, x.link.stats]
        return out
    return [x] if torch.is_tensor(x) else []


_side_streams = {}


def _side_stream(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=device)
    return _side_streams[key]


class _Scoped:
    """`with obj:` installs obj.entries in the module-level table obj._table; leaving the block restores what the table held before."""
    _table = None

    def __enter__(self):
        self.prev = dict(self._table)
        self._table.update(self.entries)
        return self

    def __exit__(self, *exc):
        self._table.clear()
        self._table.update(self.prev)
        return False


# bf16 shadows of the 1x1 convolution weights (WeightShadows below): {weight.data_ptr(): (copy [N][K], transpose [K][N])},
# only populated while a `with shadows:` block is active, i.e. while somebody guarantees they are current.
_SHADOWS = {}


class WeightShadows(_Scoped):
    """bf16 copies (and transposes) of every 1x1 convolution weight of a model, refreshed by ONE kernel launch
    (`tss_cast_weights`).  The pointwise kernels then stage their weight tiles with plain 16-byte copies instead of
    converting f32 in every block.  Opt-in and explicit: the owner calls refresh() whenever the weights changed
    (Trainer: at the top of every step, inside the captured graph) and wraps the pass in `with shadows:`; outside such
    a block the kernels read the f32 weights as before, so a stale shadow can never be used."""
    _table = _SHADOWS

    def __init__(self, module):
        ws = [p for p in module.parameters() if p.dim() == 4 and p.shape[2] == 1 and p.shape[3] == 1
              and p.dtype == torch.float32 and p.is_cuda and p.shape[1] % 8 == 0]
        self.weights = ws
        self.table = None
        self.entries = {}
        if not ws:
            return
        dev = ws[0].device
        rows, off = [], 0
        for p in ws:
            n, k = p.shape[0], p.shape[1]
            rows.append((p, off, n, k))
            off += (n * k + 7) // 8 * 8                                # 16-byte aligned segments
        self.flat = torch.empty(off, dtype=torch.bfloat16, device=dev)
        self.flat_t = torch.empty(off, dtype=torch.bfloat16, device=dev)
        table = []
        for p, o, n, k in rows:
            c, t = self.flat[o:o + n * k], self.flat_t[o:o + n * k]
            self.entries[p.data_ptr()] = (c, t)
            table.append([p.data_ptr(), c.data_ptr(), t.data_ptr(), n, k])
        self.table = torch.tensor(table, dtype=torch.int64, device=dev)
        self.blocks = max(1, min(64, (max(n * k for _, _, n, k in rows) + 255) // 256))

    def refresh(self, zero=None):
        """Rewrite the shadows from the live weights.  `zero` (a contiguous float32 tensor, e.g. the flat gradient buffer) is
        cleared by the same launch.  Returns True when `zero` was cleared here."""
        if self.table is not None:
            for p in self.weights:                                        # parameters re-pointed since construction?
                if p.data_ptr() not in self.entries:
                    raise RuntimeError('WeightShadows: a parameter was reallocated; rebuild the shadows')
            fold = zero is not None and zero.dtype == torch.float32 and zero.is_contiguous() and zero.device == self.table.device
            call('tss_cast_weights', ptr(self.table), self.table.shape[0], self.blocks, ptr(zero) if fold else None,
                 zero.numel() if fold else 0, stream())
            return fold
        return False


# bf16 tap-major copies of dense 3x3 weights prepared ahead of a forward (Dense3x3Shadows below): {weight.data_ptr(): [9][N][K] bf16}
_W3X3 = {}


class Dense3x3Shadows(_Scoped):
    """The bf16 [tap][output][input] copies of every dense 3x3 weight of a model that the matrix-core 3x3 kernels read (wstat.hip,
    atrous.hip, conv3x3.hip), written ahead of the forward instead of by one tss_permute_w3x3_bf16 launch per layer inside it.  Same
    contract as WeightShadows: refresh() rewrites them from the live weights; only visible inside `with shadows:`."""
    _table = _W3X3

    def __init__(self, module):
        self.items = []
        for m in module.modules():
            if (isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m.groups == 1 and m.weight.is_cuda
                    and m.weight.dtype == torch.float32 and m.in_channels % 8 == 0 and m.out_channels % 8 == 0):
                w = m.weight
                self.items.append((w, w.data_ptr(), torch.empty((9, m.out_channels, m.in_channels), dtype=torch.bfloat16, device=w.device)))
        self.entries = {p: t for _, p, t in self.items}

    def refresh(self):
        for w, p, t in self.items:
            if w.data_ptr() != p:
                raise RuntimeError('Dense3x3Shadows: a parameter was reallocated; rebuild the shadows')
            call('tss_permute_w3x3_bf16', ptr(w), ptr(t), None, w.shape[0], w.shape[1], stream())


# eval-mode BatchNorm affines computed for a whole model by one launch (EvalAffines below): {id(bn): [3][C] f32 view},
# only populated inside a `with affines:` block, for the forward that follows its refresh().
_EVAL_AFFINES = {}


class EvalAffines(_Scoped):
    """(mean, invstd, gamma*invstd) of every BatchNorm of a model that normalises with its running statistics, written
    by ONE kernel (`tss_bn_eval_affine_batched`) instead of one tiny launch per layer (44 in FastSCNN: 15 % of an
    eval-mode forward at 2048 x 4096).  Same contract as WeightShadows: the owner calls refresh() at the top of each
    forward (inside a captured graph it is replayed with it, so the values always follow the live parameters and
    buffers) and wraps the forward in `with affines:`; outside such a block every layer computes its own."""
    _table = _EVAL_AFFINES

    def __init__(self, module):
        import struct
        bns = [m for m in module.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)
               and m.running_mean is not None and m.running_var is not None and m.running_mean.is_cuda
               and m.running_mean.dtype == torch.float32 and (m.weight is None or m.weight.dtype == torch.float32)]
        self.bns, self.table, self.entries = bns, None, {}
        if not bns:
            return
        dev = bns[0].running_mean.device
        total = sum(3 * m.num_features for m in bns)
        self.flat = torch.empty(total, dtype=torch.float32, device=dev)
        rows, off = [], 0
        for m in bns:
            C = m.num_features
            out = self.flat[off:off + 3 * C].view(3, C)
            off += 3 * C
            self.entries[id(m)] = out
            eps_bits = struct.unpack('<i', struct.pack('<f', float(m.eps)))[0]
            rows.append([m.weight.data_ptr() if m.weight is not None else 0, m.running_mean.data_ptr(),
                         m.running_var.data_ptr(), out.data_ptr(), C, eps_bits])
        self.ptrs = [(r[0], r[1], r[2]) for r in rows]
        self.table = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.max_c = max(m.num_features for m in bns)

    def refresh(self):
        if self.table is None:
            return
        for m, (g, rm, rv) in zip(self.bns, self.ptrs):                  # re-pointed parameters / buffers since construction?
            if (m.weight.data_ptr() if m.weight is not None else 0) != g or m.running_mean.data_ptr() != rm \
                    or m.running_var.data_ptr() != rv:
                raise RuntimeError('EvalAffines: a BatchNorm tensor was reallocated; rebuild the affines')
        call('tss_bn_eval_affine_batched', ptr(self.table), self.table.shape[0], self.max_c, stream())


# The LDS-halo dense 3x3 kernel handles dilation <= 18, but it restages its nine 32 KB weight taps for every 64-pixel tile: on
# the 131 k-pixel map of BASELINE config 5 the three atrous branches of the ASPP head were 0.25 ms SLOWER through it than through
# the implicit-GEMM tap loop (3.41 vs 3.15 ms per image, profiles/README.md), so dilated convolutions stay on the general kernel
# unless this is raised (A/B: TSS_CONV3X3_LEAN_MAXDIL=18).
conv3x3_lean_max_dilation = int(os.environ.get('TSS_CONV3X3_LEAN_MAXDIL', '1'))


def _conv3x3_lean(dtype, k, n, stride, dil):
    """Domain of the LDS-halo dense 3x3 kernel (conv3x3.hip): contraction k, outputs n."""
    return (dtype == torch.bfloat16 and stride == 1 and 1 <= dil <= conv3x3_lean_max_dilation and k in (32, 64, 128) and n % 16 == 0 and 16 <= n <= 128
            and not N.fast_paths_disabled())


conv3x3_stream = os.environ.get('TSS_CONV3X3_STREAM', '1') != '0'


def _conv3x3_stream(dtype, k, n, stride, in_link, in_relu):
    """Domain of the register-streamed dense 3x3 kernel (atrous.hip): materialised bf16 input, stride 1, any dilation."""
    return (conv3x3_stream and dtype == torch.bfloat16 and stride == 1 and in_link is None and not in_relu and k % 32 == 0
            and 32 <= k <= 128 and n % 16 == 0 and 16 <= n <= 128 and not N.fast_paths_disabled())


def _shadow(weight, which):
    ent = _SHADOWS.get(weight.data_ptr()) if _SHADOWS else None
    return ptr(ent[which]) if ent is not None else None


def _aff(link):
    """(mean, scale, bias) device pointers of a pending BatchNorm: a = (x - mean) * scale + bias."""
    if link is None:
        return None, None, None
    return ptr(link.mean), ptr(link.scale), ptr(link.beta)


def _direct_target(param):
    g = param.grad if (param is not None and param.is_leaf) else None
    if _DIRECT[0] and g is not None and g.dtype == torch.float32 and g.is_contiguous() and g.is_cuda:
        return g
    return None


def _grad_target(param, like, shape=None):
    """(buffer the kernels add a parameter's gradient into, the tensor to hand back to autograd): the parameter's own .grad and None
    under direct_grads, else one fresh zero-filled tensor for both (zeros_like(like), or float32 `shape` on like's device)."""
    g = _direct_target(param)
    if g is not None:
        return g, None
    g = torch.zeros_like(like) if shape is None else torch.zeros(shape, dtype=torch.float32, device=like.device)
    return g, g


# ----------------------------------------------------------------------------- layout helpers

def round_up(v, m):
    return (v + m - 1) // m * m


def new_nhwc(b, c, h, w, dtype, device, ld=None):
    """Logical (B,C,H,W) tensor stored NHWC with row pitch `ld` (>= C, multiple of 8)."""
    ld = round_up(c, 8) if ld is None else ld
    base = torch.empty((b, h, w, ld), dtype=dtype, device=device)
    t = base.permute(0, 3, 1, 2)
    return t if ld == c else t[:, :c]


def is_nhwc(t):
    if t.dim() != 4 or not t.is_cuda:
        return False
    b, c, h, w = t.shape
    ld = t.stride(3)
    return (t.stride() == (h * w * ld, 1, w * ld, ld) and ld % 8 == 0 and ld >= c
            and t.data_ptr() % 16 == 0)


def to_nhwc(t):
    """Canonical NHWC-strided view/copy of a logical NCHW tensor (the copy is boundary plumbing)."""
    if is_nhwc(t):
        return t
    _check_device(t)
    out = new_nhwc(*t.shape, t.dtype, t.device)
    out.copy_(t)
    return out


def _check_device(t):
    if not t.is_cuda:
        raise RuntimeError('torch_semantic_segmentation_amd runs on the MI355X HIP path only: got a %s tensor. '
                           'There is no CPU fallback (the CPU oracle lives in oracle/, for tests).' % t.device)
    if t.device.index is not None and t.device.index != torch.cuda.current_device():
        # the C ABI launches on the current device's current stream: a tensor of another device would be dereferenced there
        raise RuntimeError('tensor lives on cuda:%d but the current device is cuda:%d; wrap the call in '
                           'torch.cuda.device(%d) (one process per GPU is the supported layout)'
                           % (t.device.index, torch.cuda.current_device(), t.device.index))
    N.lib()


def ld(t):
    return t.stride(3)


def npix(t):
    return t.shape[0] * t.shape[2] * t.shape[3]


# ----------------------------------------------------------------------------- deferred BatchNorm

class BNLink:
    """State shared by the producer and the consumer of one deferred BatchNorm."""
    __slots__ = ('C', 'count', 'training', 'gamma', 'beta', 'vec', 'scale', 'mean', 'invstd',
                 'ga', 'gb', 'gce', 'stats', 'bstats', 'consumed', 'sync')

    def __init__(self, C, count, training, gamma, beta, device, slabs=True):
        self.C, self.count, self.training, self.gamma, self.beta = C, count, training, gamma, beta
        self.vec = torch.empty((6, C), dtype=torch.float32, device=device)
        self.mean, self.invstd, self.scale, self.ga, self.gb, self.gce = self.vec.unbind(0)
        if slabs:
            # [forward | backward][slab rows][sum, second moment]: written in full by the kernels, never cleared here
            both = torch.empty((2, N.stat_slabs(), 2 * C), dtype=torch.float64, device=device)
            self.stats, self.bstats = both[0], both[1]
        else:       # a unit that keeps its statistics on chip (ppm_arms): nobody writes slab rows for it
            self.stats = self.bstats = None
        self.consumed = False
        self.sync = None          # process group of a cross-replica (Sync) BatchNorm, see SyncBatchNorm below


class Deferred:
    """A raw conv output plus the BatchNorm(+ReLU) that its consumer still has to apply."""
    __slots__ = ('raw', 'link', 'relu')

    def __init__(self, raw, link=None, relu=False):
        self.raw, self.link, self.relu = raw, link, relu

    @property
    def shape(self):
        return self.raw.shape


    def take(self):
        """Mark the single allowed consumption of a BN-pending tensor (its backward sums are single-use)."""
        if self.link is not None:
            if self.link.consumed:
                raise RuntimeError('a deferred BatchNorm output may feed exactly one consumer; materialize it first')
            self.link.consumed = True
        return self


class SyncBatchNorm(torch.nn.BatchNorm2d):
    """Cross-replica BatchNorm for the data-parallel path (apex.parallel.SyncBatchNorm as the reference's scripts use it,
    scripts/train_fastscnn.py:144-145): in training mode the batch statistics are those of the GLOBAL batch.  Same
    parameters, buffers and state_dict keys as nn.BatchNorm2d.  The HIP path implements it as one all-reduce of a
    [2C+1] f64 vector per layer and direction between the producing kernel and the finalize kernel."""
    process_group = None


def convert_syncbn_model(module, process_group=None):
    """apex.parallel.convert_syncbn_model: every BatchNorm2d of `module` becomes a SyncBatchNorm, in place (the
    module objects, parameters and buffers stay the same, so optimizers and state_dicts are unaffected)."""
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm2d) and not isinstance(m, SyncBatchNorm):
            m.__class__ = SyncBatchNorm
            m.process_group = process_group
    return module


def _sync_group(bn, any_mode=False):
    """The process group over which this BatchNorm's statistics are reduced, or None (local statistics: not a Sync
    layer, eval mode unless `any_mode`, no process group, or a single rank)."""
    import torch.distributed as dist
    if not isinstance(bn, (SyncBatchNorm, torch.nn.SyncBatchNorm)) or not (bn.training or any_mode):
        return None
    if not (dist.is_available() and dist.is_initialized()):
        return None
    group = getattr(bn, 'process_group', None) or dist.group.WORLD
    # TSS_SYNCBN_FORCE=1: take the cross-replica path even in a one-rank group (exercises the collectives, their HIP-graph
    # capture and their cost on a single GPU; the result equals local BatchNorm)
    return group if (dist.get_world_size(group) > 1 or os.environ.get('TSS_SYNCBN_FORCE') == '1') else None


# ---- the exchange inside the finalize kernels (csrc/xchg.hip): mailboxes of the ranks of one node, mapped through HIP IPC
syncbn_ipc = os.environ.get('TSS_SYNCBN_IPC', '1') != '0'       # 0: every BatchNorm statistic through dist.all_reduce (RCCL), as in round 3
_XCHG = {}


class _Exchange:
    """This rank's mailbox + the peers' mailboxes as mapped into this process, for one (process group, device)."""

    def __init__(self, group, device):
        import socket
        import torch.distributed as dist
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        self.device = device
        if self.world > 8:
            raise RuntimeError('more than 8 ranks')
        nbytes = N.lib().tss_bn_xchg_bytes()
        own, handle = ctypes.c_void_p(), (ctypes.c_char * 64)()
        with torch.cuda.device(device):
            call('tss_ipc_alloc', nbytes, ctypes.byref(own), handle)
            self.own = own.value
            me = (socket.gethostname(), os.getpid(), bytes(handle.raw))
            everyone = [None] * self.world
            if self.world > 1:
                dist.all_gather_object(everyone, me, group=group)       # (also the barrier behind which every mailbox is zero-filled)
            else:
                everyone[0] = me
            if len({h for h, _, _ in everyone}) != 1:
                call('tss_ipc_free', self.own)
                raise RuntimeError('the ranks of the group are not on one node')
            self.mapped = []
            ptrs = []
            for r, (_, pid, hb) in enumerate(everyone):
                if r == self.rank:
                    ptrs.append(self.own)
                    continue
                if pid == os.getpid():
                    raise RuntimeError('two ranks in one process')
                p_ = ctypes.c_void_p()
                call('tss_ipc_open', ctypes.create_string_buffer(hb, 64), ctypes.byref(p_))
                self.mapped.append(p_.value)
                ptrs.append(p_.value)
        self.peers = (ctypes.c_void_p * self.world)(*ptrs)
        self.counters = torch.zeros(N.lib().tss_bn_xchg_counters(), dtype=torch.int64, device=device)
        if self.world > 1:
            dist.barrier(group=group)          # every rank has mapped every mailbox before anybody writes

    def error(self):
        out = ctypes.c_long(0)
        with torch.cuda.device(self.device):
            call('tss_bn_xchg_error', self.own, ctypes.byref(out))
        return out.value


def _exchange(group, device):
    """The IPC exchange of `group` on `device`, or None (switched off, set-up failed: the caller uses dist.all_reduce)."""
    if not syncbn_ipc:
        return None
    key = (group, device.index)        # the group object itself: the entry keeps it alive, so no later group can alias it
    if key not in _XCHG:
        try:
            _XCHG[key] = _Exchange(group, device)
        except Exception as exc:       # noqa: BLE001 -- any failure of the IPC set-up: the collective library still works
            import warnings
            warnings.warn('SyncBatchNorm: HIP IPC exchange unavailable (%s); using dist.all_reduce' % (exc,))
            _XCHG[key] = None
    return _XCHG[key]


def _allreduce_stats(slabs, count, C, group, st):
    """slab rows of this replica -> [2C+1] f64 (sums, second moments, count), summed over the ranks."""
    import torch.distributed as dist
    vec = torch.empty(2 * C + 1, dtype=torch.float64, device=slabs.device)
    call('tss_slab_reduce', ptr(slabs), float(count), ptr(vec), C, st)
    dist.all_reduce(vec, op=dist.ReduceOp.SUM, group=group)
    return vec


def as_deferred(x):
    if isinstance(x, Deferred):
        return x
    _check_device(x)
    N.dtype_code(x.dtype)
    return Deferred(to_nhwc(x))


def materialize(d, relu_override=None):
    """Deferred -> ordinary tensor (applies the pending BatchNorm/ReLU with one `join` pass)."""
    if not isinstance(d, Deferred):
        return d
    if d.link is None and not d.relu:
        return d.raw
    return join(d, None, d.relu)


# ----------------------------------------------------------------------------- convolution unit

class UnitCfg:
    __slots__ = ('kind', 'stride', 'dil', 'in_link', 'in_relu', 'bn', 'training', 'out_dtype', 'out_link',
                 'image_f32', 'cin', 'cout', 'params', 'res_fork', 'stash_fork', 'overlapped', 'kh', 'kw', 'drop_p', 'prev_join',
                 'stem_rc')


def _classify(conv, x_is_image):
    k = conv.kernel_size
    if tuple(k) in ((1, 3), (3, 1)):
        # factorized convolution (TSS/models/lednet.py:157-180): 3 taps along one axis, padding = dilation on that axis
        ax = 0 if tuple(k) == (1, 3) else 1                 # 0: along W, 1: along H
        d = conv.dilation[1 - ax]
        want_pad, want_dil = ((0, d), (1, d)) if ax == 0 else ((d, 0), (d, 1))
        if (conv.padding_mode != 'zeros' or conv.groups != 1 or tuple(conv.stride) != (1, 1) or tuple(conv.padding) != want_pad
                or tuple(conv.dilation) != want_dil or x_is_image):
            raise NotImplementedError('HIP path: 1x3 / 3x1 convolutions must be dense, stride 1, padding = dilation on the '
                                      'kernel axis: %r' % conv)
        return 'dense1d_w' if ax == 0 else 'dense1d_h', 1, d
    kh, kw = k
    if conv.groups == 1 and not x_is_image and kh % 2 == 1 and kw % 2 == 1 and (kh != kw or kh > 3):
        # general dense convolution (csrc/convgemm.hip, kh x kw tap grid): the 5x5 / 7x7 stride-2 layers of LEDNet's APN decoder
        # (TSS/models/lednet.py:63-64), the 1x5 / 5x1 layers of ESNet's FCUBlock (TSS/models/esnet.py:83-113)
        dd = [conv.dilation[i] for i in (0, 1) if k[i] > 1]
        d = dd[0]
        if (conv.padding_mode != 'zeros' or conv.stride[0] != conv.stride[1] or any(v != d for v in dd)
                or tuple(conv.padding) != (d * (kh - 1) // 2 if kh > 1 else 0, d * (kw - 1) // 2 if kw > 1 else 0)):
            raise NotImplementedError('HIP path: dense k x k convolutions need padding = dilation * (k - 1) / 2 and one stride: %r' % conv)
        return 'ckk', conv.stride[0], d
    if conv.padding_mode != 'zeros' or k[0] != k[1] or conv.stride[0] != conv.stride[1] \
            or conv.dilation[0] != conv.dilation[1] or conv.padding[0] != conv.padding[1]:
        raise NotImplementedError('HIP path: square kernels/strides/dilations with zero padding only: %r' % conv)
    k, s, d, p = k[0], conv.stride[0], conv.dilation[0], conv.padding[0]
    if k == 1:
        if conv.groups != 1 or s != 1 or p != 0:
            raise NotImplementedError('HIP path: 1x1 convolutions must be dense, stride 1, padding 0: %r' % conv)
        return 'pw', 1, 1
    if k != 3 or p != d:
        raise NotImplementedError('HIP path: 3x3 convolutions need padding == dilation: %r' % conv)
    if conv.groups == conv.in_channels == conv.out_channels and conv.groups > 1:
        return 'dw', s, d
    if conv.groups != 1:
        raise NotImplementedError('HIP path: grouped convolutions other than depthwise are not on the hot path: %r' % conv)
    if x_is_image:
        if d != 1 or conv.in_channels * 9 > 64:
            raise NotImplementedError('HIP path: image stem needs dilation 1 and in_channels*9 <= 64: %r' % conv)
        return 'stem', s, 1
    return 'dense', s, d


_KEEP = object()
_drop_mask_probe = None       # a list while a test collects the masks drawn by dropout-on-load convolutions


def drop_conv_supported(x, conv, p):
    """nn.Dropout(p) -> 1x1 `conv` (no BatchNorm behind it) can run as ONE unit that applies the dropout on load (conv_unit's drop_p)
    instead of a pass of its own over the activation: the Classifier tails (TSS/models/fastscnn.py:96-97, contextnet.py:85-86)."""
    if not (fuse_dropout and fuse_dropout_conv) or N.fast_paths_disabled() or not (0.0 < p < 1.0):
        return False
    try:
        kind = _classify(conv, False)[0]
    except NotImplementedError:
        return False
    raw = x.raw if isinstance(x, Deferred) else x
    if kind != 'pw' or raw.dim() != 4 or raw.dtype != torch.bfloat16 or raw.shape[1] != conv.in_channels:
        return False
    P, dt = npix(raw), N.dtype_code(raw.dtype)
    return bool(N.lib().tss_pwconv_drop_supported(P, conv.in_channels, conv.out_channels, dt)
                and N.lib().tss_pwconv_bwd_fused_drop_supported(P, conv.in_channels, conv.out_channels, dt))


def conv_unit(x, conv, bn=None, relu=False, out_dtype=None, weight=None, bias=_KEEP, gamma=None, beta=None, cout=None, drop_p=0.0):
    """conv -> [BatchNorm] -> [ReLU] as ONE deferred unit.  `x` is a Deferred, an NHWC/NCHW activation tensor
    or (for the stem) the contiguous NCHW image.  Returns a Deferred.
    drop_p > 0 (after drop_conv_supported): nn.Dropout(drop_p) sits between x's pending activation and the convolution.
    weight / bias / gamma / beta / cout: run the unit with these tensors instead of the modules' own parameters (a weight padded
    with zero output rows so that a ragged channel count fills whole 8-channel vectors, a bias that a later kernel adds)."""
    is_image = (not isinstance(x, Deferred)) and x.dim() == 4 and x.shape[1] % 8 != 0
    kind, stride, dil = _classify(conv, is_image)
    cfg = UnitCfg()
    cfg.kind, cfg.stride, cfg.dil = kind, stride, dil
    cfg.drop_p = float(drop_p)
    cfg.stem_rc = None      # (weight, its _version) once the direct stem kernel has run this unit's forward (_fwd_stem)
    if cfg.drop_p and (kind != 'pw' or bn is not None):
        raise RuntimeError('conv_unit: dropout on load needs a 1x1 convolution without BatchNorm (drop_conv_supported)')
    cfg.overlapped = _overlap_depth[0] > 0 and not postpone_in_overlap
    cfg.cin, cfg.cout = conv.in_channels, (cout or conv.out_channels)
    cfg.kh, cfg.kw = conv.kernel_size
    if kind == 'stem':
        _check_device(x)
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError('image must be float32 or bfloat16')
        x_raw = x.contiguous()
        cfg.in_link, cfg.in_relu = None, False
        cfg.image_f32 = x_raw.dtype == torch.float32
        cfg.out_dtype = out_dtype or x_raw.dtype
        cfg.res_fork = cfg.stash_fork = cfg.prev_join = None
    else:
        d = as_deferred(x).take()
        x_raw = d.raw
        cfg.in_link, cfg.in_relu = d.link, d.relu
        cfg.image_f32 = False
        cfg.out_dtype = x_raw.dtype
        cfg.res_fork = _take(x_raw, _FORK)
        cfg.stash_fork = _take(x_raw, _STASH)
        cfg.prev_join = cfg.res_fork.prev_join if cfg.res_fork is not None else (_take_join(x_raw) if d.link is None and not d.relu else None)
    if x_raw.shape[1] != conv.in_channels:
        raise RuntimeError('expected %d input channels, got %d' % (conv.in_channels, x_raw.shape[1]))
    cfg.bn = bn
    cfg.training = False
    if bn is None:
        gamma = beta = None
    if bn is not None:
        if not isinstance(bn, _BatchNorm):
            raise TypeError('expected a BatchNorm module, got %r' % bn)
        cfg.training = bn.training or (bn.running_mean is None and bn.running_var is None)
        if cfg.training and bn.momentum is None:
            raise NotImplementedError('HIP path: BatchNorm with momentum=None (cumulative average) is not supported')
        if gamma is None:
            gamma, beta = bn.weight, bn.bias
    p_weight = conv.weight if weight is None else weight
    p_bias = conv.bias if bias is _KEEP else bias
    cfg.params = (p_weight, gamma, beta, p_bias)
    # the kernels read float32 parameters; a model cast with .half() / .to(torch.bfloat16) (TSS
    # scripts/contextnet/benchmark_contextnet.py:62) hands them differentiable f32 views of its 16-bit parameters (boundary
    # plumbing: the gradient flows back through the cast, and the direct-accumulation path below stays off for them)
    weight, bias = _f32(p_weight), _f32(p_bias)
    y = ConvUnitFn.apply(x_raw, weight, _f32(gamma), _f32(beta), bias, cfg)
    return Deferred(y, cfg.out_link, relu)


def conv_unit_multi(branches, conv, bn=None, relu=False):
    """conv(torch.cat(branches, dim=1)) -> [BatchNorm] -> [ReLU] for a 1x1 `conv`, with NO concatenated tensor: the kernel walks the
    contraction source by source and applies every branch's pending BatchNorm (+ the branches' common ReLU) on load
    (tss_pwconv_fwd_multi).  A branch of shape [1, C, 1, 1] is broadcast over the map (an image-pooling branch needs no upsampled
    copy).  Eval-mode / no-grad forward only; returns None when the call is outside that envelope (the caller concatenates)."""
    if torch.is_grad_enabled() or N.fast_paths_disabled() or not (2 <= len(branches) <= 6):
        return None
    if conv.kernel_size != (1, 1) or conv.groups != 1 or conv.stride != (1, 1) or conv.padding != (0, 0) or conv.in_channels != 128 * len(branches):
        return None
    if bn is not None and (not isinstance(bn, _BatchNorm) or bn.training or bn.running_mean is None):
        return None
    ds = [as_deferred(b) for b in branches]
    full = next((d.raw for d in ds if d.raw.shape[2] * d.raw.shape[3] > 1), None)
    if full is None or full.dtype != torch.bfloat16 or conv.weight.dtype != torch.float32 or conv.out_channels % 4:
        return None
    B, _, H, W = full.shape
    in_relu = ds[0].relu
    for d in ds:
        r = d.raw
        bcast = tuple(r.shape) == (1, 128, 1, 1) and B == 1
        if r.dtype != torch.bfloat16 or r.shape[1] != 128 or d.relu != in_relu or not (bcast or tuple(r.shape) == (B, 128, H, W)) or not is_nhwc(r):
            return None
    for d in ds:
        d.take()
    dev, st = full.device, stream()
    n = len(ds)
    srcs = (ctypes.c_void_p * n)(*[d.raw.data_ptr() for d in ds])
    lds = (ctypes.c_long * n)(*[0 if d.raw.shape[2] * d.raw.shape[3] == 1 else ld(d.raw) for d in ds])

    def vec(getter):
        return (ctypes.c_void_p * n)(*[(getter(d.link).data_ptr() if d.link is not None and getter(d.link) is not None else None) for d in ds])
    means, scales, biases = vec(lambda l: l.mean), vec(lambda l: l.scale), vec(lambda l: l.beta)
    Cout, P = conv.out_channels, B * H * W
    y = new_nhwc(B, Cout, H, W, torch.bfloat16, dev)
    weight = conv.weight
    call('tss_pwconv_fwd_multi', srcs, lds, means, scales, biases, n, int(in_relu), ptr(weight), _shadow(weight, 0), ptr(_f32(conv.bias)),
         ptr(y), ld(y), P, Cout, N.dtype_code(torch.bfloat16), st)
    link = _frozen_link(bn, Cout, P, dev, st)[0] if bn is not None else None
    return Deferred(y, link, relu)


eval_epilogue = os.environ.get('TSS_EVAL_EPILOGUE', '1') != '0'   # A/B: 0 = eval-mode block outputs through the join pass, as in training


def conv_unit_joined(x, block, residual=None, relu=True):
    """Eval-mode, no-grad form of `join(block(x), residual, relu)` for block = FusedSequential(1x1 Conv2d, BatchNorm2d): the frozen
    BatchNorm, the skip and the ReLU run in the epilogue of the convolution (tss_pwconv_fwd_joined), so the block output is written
    once and no join pass exists (BottleneckBlock.forward of both models under model.eval()).  Returns the materialised tensor, or None
    when the call is outside that envelope (training statistics, gradients, f32, hooks: the caller takes the ordinary path)."""
    if not eval_epilogue or torch.is_grad_enabled() or N.fast_paths_disabled():
        return None
    mods = list(block) if isinstance(block, torch.nn.Sequential) else None
    if mods is None or len(mods) != 2 or not isinstance(mods[0], torch.nn.Conv2d) or not isinstance(mods[1], _BatchNorm):
        return None
    conv, bn = mods
    if bn.training or bn.running_mean is None or bn.running_var is None:
        return None
    try:
        kind = _classify(conv, False)[0]
    except NotImplementedError:
        return None
    raw = x.raw if isinstance(x, Deferred) else x
    if (kind != 'pw' or raw.dim() != 4 or raw.dtype != torch.bfloat16 or raw.shape[1] != conv.in_channels
            or conv.in_channels % 8 or conv.in_channels > 768 or conv.out_channels % 8 or conv.weight.dtype != torch.float32):
        return None
    B, _, H, W = raw.shape
    Cout, P = conv.out_channels, B * H * W
    if residual is not None:
        residual = to_nhwc(materialize(residual))
        if tuple(residual.shape) != (B, Cout, H, W) or residual.dtype != raw.dtype:
            return None
    d = as_deferred(x).take()
    dev, st = raw.device, stream()
    link, beta = _frozen_link(bn, Cout, P, dev, st)
    y = new_nhwc(B, Cout, H, W, raw.dtype, dev)
    call('tss_pwconv_fwd_joined', ptr(d.raw), ld(d.raw), *_aff(d.link), int(d.relu), ptr(conv.weight), _shadow(conv.weight, 0),
         ptr(_f32(conv.bias)), ptr(link.mean), ptr(link.scale), ptr(beta), ptr(residual), ld(residual) if residual is not None else 0,
         int(bool(relu)), ptr(y), ld(y), P, conv.in_channels, Cout, N.dtype_code(raw.dtype), st)
    return y


eval_bottleneck = os.environ.get('TSS_BNECK_EVAL', '1') != '0'     # A/B: 0 = eval-mode inverted residuals layer by layer


def bottleneck_eval(x, conv1, conv2, conv3):
    """Eval-mode, no-grad form of a whole inverted residual -- conv1 (1x1, BatchNorm, ReLU) -> conv2 (depthwise 3x3, BatchNorm, ReLU) ->
    conv3 (1x1, BatchNorm) -> (+ x) -> ReLU, each convN a FusedSequential as the block builders make them -- as ONE kernel
    (csrc/bneck.hip: the expanded tensors live in LDS only; BottleneckBlock.forward of both models under model.eval(),
    TSS/models/fastscnn.py:152-161, TSS/models/contextnet.py:139-147).  Returns the materialised block output, or None when the call
    is outside that envelope (gradients, batch statistics, f32, hooks, channel counts: the caller goes layer by layer)."""
    if not eval_bottleneck or torch.is_grad_enabled() or N.fast_paths_disabled():
        return None
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16):
        return None
    parts = []
    for blk, want_relu in ((conv1, True), (conv2, True), (conv3, False)):
        mods = list(blk) if isinstance(blk, torch.nn.Sequential) else None
        if mods is None or len(mods) != (3 if want_relu else 2) or not isinstance(mods[0], torch.nn.Conv2d) \
                or not isinstance(mods[1], _BatchNorm) or (want_relu and not isinstance(mods[2], torch.nn.ReLU)):
            return None
        conv, bn = mods[0], mods[1]
        if bn.training or bn.running_mean is None or bn.running_var is None or conv.bias is not None \
                or conv.weight.dtype != torch.float32 or (bn.weight is not None and bn.weight.dtype != torch.float32):
            return None
        parts.append((conv, bn))
    (c1, bn1), (c2, bn2), (c3, bn3) = parts
    try:
        k1, k2, k3 = _classify(c1, False), _classify(c2, False), _classify(c3, False)
    except NotImplementedError:
        return None
    if k1[0] != 'pw' or k3[0] != 'pw' or k2[0] != 'dw' or k2[2] != 1 or k2[1] not in (1, 2):
        return None
    B, Cin, H, W = x.shape
    Cmid, Cout, stride = c1.out_channels, c3.out_channels, k2[1]
    if c1.in_channels != Cin or c2.in_channels != Cmid or c3.in_channels != Cmid:
        return None
    residual = int(stride == 1 and Cin == Cout)
    dt = N.dtype_code(x.dtype)
    if not N.lib().tss_bneck_eval_supported(Cin, Cmid, Cout, stride, residual, dt):
        return None
    x = to_nhwc(x)
    dev, st = x.device, stream()
    links = [_frozen_link(bn, C, 1, dev, st) for bn, C in ((bn1, Cmid), (bn2, Cmid), (bn3, Cout))]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = new_nhwc(B, Cout, Ho, Wo, x.dtype, dev)
    aff = []
    for link, beta in links:
        aff += [ptr(link.mean), ptr(link.scale), ptr(beta if beta is not None else torch.zeros_like(link.mean))]
    call('tss_bneck_eval_fwd', ptr(x), ld(x), ptr(c1.weight), _shadow(c1.weight, 0), aff[0], aff[1], aff[2],
         ptr(c2.weight), aff[3], aff[4], aff[5], ptr(c3.weight), _shadow(c3.weight, 0), aff[6], aff[7], aff[8],
         residual, ptr(y), ld(y), B, H, W, Cin, Cmid, Cout, stride, dt, st)
    return y


def _f32(p):
    if p is None or p.dtype == torch.float32:
        return p
    if p.dtype not in (torch.float16, torch.bfloat16):
        raise TypeError('HIP path: parameters must be float32, float16 or bfloat16, got %s' % p.dtype)
    return p.float()


class _F32Buffers:
    """float32 stand-ins for the running statistics of a BatchNorm whose buffers were cast to 16 bits by model.half():
    the finalize kernels update the stand-ins, close() writes them back."""

    def __init__(self, bn, track):
        self.pairs = []
        self.mean = self.var = None
        if track:
            self.mean, self.var = self._get(bn.running_mean), self._get(bn.running_var)

    def _get(self, buf):
        if buf.dtype == torch.float32:
            return buf
        tmp = buf.float()
        self.pairs.append((buf, tmp))
        return tmp

    def close(self):
        for buf, tmp in self.pairs:
            buf.copy_(tmp)


def _colsum(e, C, st):
    """Per-channel sums of an NHWC tensor over its pixels (f32 [C]) through the statistics slab rows: fixed order, any C."""
    P = npix(e)
    Cw = C
    if C % 8 and ld(e) >= round_up(C, 8) and e.data_ptr() % 16 == 0:
        Cw = round_up(C, 8)       # whole 8-channel vectors (the vectorised kernel): the neighbouring columns of the buffer are summed too, and dropped
    slab = torch.empty((N.stat_slabs(), 2 * Cw), dtype=torch.float64, device=e.device)
    vec = torch.empty(2 * Cw + 1, dtype=torch.float64, device=e.device)
    call('tss_tensor_stats', ptr(e), ld(e), P, Cw, ptr(slab), N.dtype_code(e.dtype), st)
    call('tss_slab_reduce', ptr(slab), float(P), ptr(vec), Cw, st)
    return vec[:C].float()


def _bias_grad_into(e, P, Cout, out, dt, st):
    """out (f32 [Cout], pre-filled) += column sums of e"""
    if Cout <= 64:
        call('tss_bias_grad', ptr(e), ld(e), P, Cout, ptr(out), dt, st)
    else:
        out.add_(_colsum(e, Cout, st))


def _finalize_forward(link, bn, training, P, Cout, gamma, st):
    """Statistics slab rows (training) or running statistics (eval) -> mean / invstd / scale of `link`; running statistics updated."""
    if training:
        track = bn.track_running_stats and bn.running_mean is not None
        rbuf = _F32Buffers(bn, track)
        run_args = (ptr(rbuf.mean), ptr(rbuf.var),
                    ptr(bn.num_batches_tracked) if (track and bn.num_batches_tracked is not None) else None)
        link.sync = _sync_group(bn)
        ex = _exchange(link.sync, link.stats.device) if (link.sync is not None and Cout <= 768) else None
        if ex is not None:
            # slab rows -> statistics of ALL ranks inside ONE kernel (mailboxes over HIP IPC): no collective, no extra launch
            call('tss_bn_finalize_xchg', ptr(link.stats), float(P), ex.peers, ex.rank, ex.world, ptr(ex.counters), ptr(gamma),
                 float(bn.eps), float(bn.momentum), *run_args, ptr(link.mean), ptr(link.invstd), ptr(link.scale), Cout, st)
        elif link.sync is not None:
            gs = _allreduce_stats(link.stats, P, Cout, link.sync, st)
            call('tss_bn_finalize_sync', ptr(gs), ptr(gamma), float(bn.eps), float(bn.momentum), *run_args,
                 ptr(link.mean), ptr(link.invstd), ptr(link.scale), Cout, st)
        else:
            call('tss_bn_finalize', ptr(link.stats), float(P), ptr(gamma), float(bn.eps),
                 float(bn.momentum), *run_args, ptr(link.mean), ptr(link.invstd), ptr(link.scale), Cout, st)
        rbuf.close()
    else:
        pre = _EVAL_AFFINES.get(id(bn)) if _EVAL_AFFINES else None
        if pre is not None:     # written by the model-wide launch at the top of this forward
            link.mean, link.invstd, link.scale = pre.unbind(0)
        else:
            rbuf = _F32Buffers(bn, True)
            call('tss_bn_eval_affine', ptr(gamma), ptr(rbuf.mean), ptr(rbuf.var),
                 float(bn.eps), ptr(link.mean), ptr(link.invstd), ptr(link.scale), Cout, st)


def _frozen_link(bn, C, P, dev, st):
    """(link, beta) of a BatchNorm with frozen statistics behind an eval-only fast path: mean / scale from the running statistics,
    no slab rows (nothing is summed)."""
    gamma, beta = _f32(bn.weight), _f32(bn.bias)
    link = BNLink(C, P, False, gamma, beta, dev, slabs=False)
    _finalize_forward(link, bn, False, P, C, gamma, st)
    return link, beta


# What one ConvUnitFn.forward hands the handler of its kind: aff = the pending BatchNorm of the input (applied on load),
# stats = the slab rows of this layer's own BatchNorm (NULL when it keeps none).
_FwdArgs = collections.namedtuple('_FwdArgs', 'cfg x weight bias y aff stats B Hin Win Cout P s d dt dev st')


def _fwd_stem(f):
    cfg, y = f.cfg, f.y
    if f.bias is not None:
        raise NotImplementedError('HIP path: stem convolution with bias')
    call('tss_stem3x3_fwd', ptr(f.x), int(cfg.image_f32), ptr(f.weight), ptr(y), ld(y), f.stats,
         f.B, cfg.cin, f.Hin, f.Win, f.Cout, f.s, f.dt, f.st)
    if y.dtype == torch.bfloat16 and cfg.cin <= 3 and f.Cout == 32 and not N.fast_paths_disabled():
        # the direct kernel (csrc/stem.hip) wrote y: the backward may form it again from (x, this weight as it is now)
        cfg.stem_rc = (f.weight, f.weight._version)


def _fwd_pw(f):
    """Returns the dropout mask of a dropout-on-load layer (saved for the backward sweep), else None."""
    cfg, x, weight, y, st = f.cfg, f.x, f.weight, f.y, f.st
    if not cfg.drop_p:
        call('tss_pwconv_fwd', ptr(x), ld(x), *f.aff, int(cfg.in_relu), ptr(weight), _shadow(weight, 0), ptr(f.bias),
             ptr(y), ld(y), f.stats, f.P, cfg.cin, f.Cout, f.dt, st)
        return None
    # the mask is drawn by its own small launch (one byte per 8 channels), applied on load here and in the backward sweep
    mask = torch.empty((f.P, 16), dtype=torch.uint8, device=f.dev)
    counter = _dropout_counter(f.dev)
    call('tss_dropout_mask', ptr(counter), ptr(mask), f.P, cfg.cin, cfg.drop_p, st)
    if _drop_mask_probe is not None:         # tests read the mask back to hand the oracle the same one
        _drop_mask_probe.append(mask)
    call('tss_pwconv_fwd_drop', ptr(x), ld(x), *f.aff, int(cfg.in_relu), ptr(weight), _shadow(weight, 0), ptr(f.bias),
         ptr(y), ld(y), ptr(mask), cfg.drop_p, ptr(counter), f.P, cfg.cin, f.Cout, f.dt, st)
    return mask


def _fwd_dw(f):
    cfg, x, y = f.cfg, f.x, f.y
    if f.bias is not None:
        raise NotImplementedError('HIP path: depthwise convolution with bias')
    call('tss_dwconv3x3_fwd', ptr(x), ld(x), *f.aff, int(cfg.in_relu), ptr(f.weight),
         ptr(y), ld(y), f.stats, f.B, f.Hin, f.Win, f.Cout, f.s, f.d, f.dt, f.st)


def _fwd_ckk(f):
    cfg, x, y, Cout, st = f.cfg, f.x, f.y, f.Cout, f.st
    nt = cfg.kh * cfg.kw
    w_tnc = torch.empty((nt, Cout, cfg.cin), dtype=torch.float32, device=f.dev)
    call('tss_permute_wtaps', ptr(f.weight), ptr(w_tnc), None, Cout, cfg.cin, nt, st)
    call('tss_convkxk_fwd', ptr(x), ld(x), *f.aff, int(cfg.in_relu), ptr(w_tnc), ptr(f.bias), ptr(y), ld(y), f.stats,
         f.B, f.Hin, f.Win, cfg.cin, Cout, cfg.kh, cfg.kw, f.s, f.d, f.dt, st)


def _fwd_dense(f):
    if f.bias is not None:          # the 3x3 kernels add no bias: the general tap-grid kernel
        return _fwd_ckk(f)
    cfg, x, weight, y, Cout, st = f.cfg, f.x, f.weight, f.y, f.Cout, f.st
    w_tnc = w_tnc16 = None
    if _conv3x3_stream(x.dtype, cfg.cin, Cout, f.s, cfg.in_link, cfg.in_relu) or _conv3x3_lean(x.dtype, cfg.cin, Cout, f.s, f.d):
        # bf16 tap-major copy: the weight-stationary / register-streamed kernels (wstat.hip, atrous.hip), the LDS-halo kernel (conv3x3.hip)
        w_tnc16 = _W3X3.get(weight.data_ptr()) if _W3X3 else None          # prepared ahead of the forward (Dense3x3Shadows)
        if w_tnc16 is None:
            w_tnc16 = torch.empty((9, Cout, cfg.cin), dtype=torch.bfloat16, device=f.dev)
            call('tss_permute_w3x3_bf16', ptr(weight), ptr(w_tnc16), None, Cout, cfg.cin, st)
    else:
        w_tnc = torch.empty((9, Cout, cfg.cin), dtype=torch.float32, device=f.dev)
        call('tss_permute_w3x3', ptr(weight), ptr(w_tnc), None, Cout, cfg.cin, st)
    call('tss_conv3x3_fwd', ptr(x), ld(x), *f.aff, int(cfg.in_relu), ptr(w_tnc), ptr(w_tnc16),
         ptr(y), ld(y), f.stats, f.B, f.Hin, f.Win, cfg.cin, Cout, f.s, f.d, f.dt, st)


def _fwd_dense1d(f):
    cfg, x, weight, y, Cout, st = f.cfg, f.x, f.weight, f.y, f.Cout, f.st
    axis = 0 if cfg.kind == 'dense1d_w' else 1
    if N.lib().tss_conv1d3_lean_supported(cfg.cin, Cout, f.dt):      # reads the layer's own weight tensor
        call('tss_conv1d3_fwd_w', ptr(x), ld(x), *f.aff, int(cfg.in_relu), ptr(weight), ptr(f.bias), ptr(y), ld(y), f.stats,
             f.B, f.Hin, f.Win, cfg.cin, Cout, axis, f.d, f.dt, st)
    else:
        w_tnc = torch.empty((3, Cout, cfg.cin), dtype=torch.float32, device=f.dev)
        call('tss_permute_wtaps', ptr(weight), ptr(w_tnc), None, Cout, cfg.cin, 3, st)
        call('tss_conv1d3_fwd', ptr(x), ld(x), *f.aff, int(cfg.in_relu), ptr(w_tnc), ptr(f.bias), ptr(y), ld(y), f.stats,
             f.B, f.Hin, f.Win, cfg.cin, Cout, axis, f.d, f.dt, st)


# keyed by what _classify returns
_FWD = {'stem': _fwd_stem, 'pw': _fwd_pw, 'dw': _fwd_dw, 'ckk': _fwd_ckk, 'dense': _fwd_dense,
        'dense1d_w': _fwd_dense1d, 'dense1d_h': _fwd_dense1d}


class _Bwd:
    """What one ConvUnitFn.backward hands the handler of its kind (built once per layer and pass; every field is bound for every kind).
    y, ga are what _bn_backward_prologue left (y None: no BatchNorm behind the layer, or a frozen one).
    gargs: the gradient operand -- e, y and the BatchNorm-backward coefficients applied on load.  xargs: the layer's input with its
    pending BatchNorm / ReLU.  margs: the same where a backward-data kernel masks / sums for that pending BatchNorm (deferred_in),
    else NULLs; bst: the slab rows those sums go to.  dw / dw_ret: _grad_target of the weight.  st: this stream, wst: the stream of
    the weight-gradient launch (the side stream when there is one)."""
    __slots__ = ('cfg', 'x', 'weight', 'y', 'e', 'drop_mask', 'ga', 'gargs', 'xargs', 'margs', 'bst', 'B', 'Hin', 'Win', 'Cin', 'Cout',
                 'P', 's', 'd', 'dt', 'dev', 'st', 'wst', 'side', 'need_dx', 'has_bias', 'dw', 'dw_ret', 'p_weight', 'p_bias',
                 'link', 'il', 'deferred_in', 'temps')

    def tmp(self, shape, dtype=torch.float32):
        """A workspace / weight permute for this layer's launches.  It stays alive until backward() returns: the launch that uses it
        may be on the side stream, which joins only there."""
        t = torch.empty(shape, dtype=dtype, device=self.dev)
        self.temps.append(t)
        return t


# what a handler returns next to e_in: (rows of weight-gradient partial sums to add after the side stream has joined: (ws, nrows,
# ncols) or None; the handler has produced the bias gradient; that gradient where it goes back to autograd)
_NO_EXTRAS = (None, False, None)


def _wgrad_side_stream(cfg, need_dx, drop_mask, P, dev):
    """Backward-weight and backward-data of one layer are independent: the side stream the weight gradient goes to, or None."""
    if (overlap_wgrad and need_dx and cfg.kind != 'stem' and drop_mask is None
            and overlap_min_elems <= P * (cfg.cin + cfg.cout) <= overlap_max_elems):
        return _side_stream(dev)
    return None


def _new_e_in(c):
    """The input-gradient tensor, when this backward writes one (dropout on load: always -- the one sweep is the only backward)."""
    if c.need_dx or c.drop_mask is not None:
        return new_nhwc(c.B, c.Cin, c.Hin, c.Win, c.e.dtype, c.dev)
    return None


def _res_grad(cfg):
    """(fork, the gradient the other consumer of this layer's input left for the epilogue of its backward-data kernel, or None)"""
    fork = cfg.res_fork
    return fork, (fork.g2 if fork is not None else None)


def _stem_recompute(c):
    """The stem's y need not be read back: the direct kernel wrote it in this unit's forward from the weight tensor that is still
    the same object at the same version, a train-mode BatchNorm is pending behind it, and nothing has switched the fast paths off."""
    rc = c.cfg.stem_rc
    return bool(stem_wgrad_recompute and rc is not None and c.y is not None and c.link is not None and c.link.training
                and c.weight is rc[0] and c.weight._version == rc[1] and c.e.dtype == torch.bfloat16 and c.Cin <= 3 and c.Cout == 32
                and not N.fast_paths_disabled())


def _bwd_stem(c):
    ws = c.tmp((N.stat_slabs(), c.Cout * 28))
    if _stem_recompute(c):
        e, lde, _, _, ga, gb, gce, gmu = c.gargs
        call('tss_stem3x3_bwd_weight_rc', e, lde, ptr(c.weight), ga, gb, gce, gmu, ptr(c.x), int(c.cfg.image_f32), ptr(c.dw), ptr(ws),
             c.B, c.Cin, c.Hin, c.Win, c.Cout, c.s, c.dt, c.st)
    else:
        call('tss_stem3x3_bwd_weight', *c.gargs, ptr(c.x), int(c.cfg.image_f32), ptr(c.dw), ptr(ws),
             c.B, c.Cin, c.Hin, c.Win, c.Cout, c.s, c.dt, c.st)
    if c.need_dx:
        raise NotImplementedError('HIP path: gradient with respect to the input image is not implemented')
    return None, _NO_EXTRAS


# ---- 1x1: one of three strategies, chosen once

def _bwd_pw(c):
    P, Cin, Cout, dt = c.P, c.Cin, c.Cout, c.dt
    # few channels, many pixels: input gradient and weight gradient in ONE sweep (csrc/pwbwd.hip): e, y, x read once
    fused = bool(fuse_pw_backward and c.need_dx and c.side is None and c.e.dtype == torch.bfloat16
                 and not N.fast_paths_disabled() and N.lib().tss_pwconv_bwd_fused_preferred(P, Cin, Cout, dt))
    if c.drop_mask is not None:        # dropout on load: the one sweep is the only backward that knows the mask
        fused = True
    if fused:
        return _bwd_pw_fused(c)
    # the large layers (128 -> 128, 64 -> 384, 384 -> 64 with enough pixels): one sweep with the whole weight-gradient tile in
    # the registers of one 512-thread block per CU (csrc/pwsweep.hip)
    radd_s = _res_grad(c.cfg)[1]
    sweep = bool(sweep_pw_backward and c.need_dx and c.side is None and c.e.dtype == torch.bfloat16 and c.x.dtype == torch.bfloat16
                 and not N.fast_paths_disabled()
                 and N.lib().tss_pwconv_bwd_sweep_preferred(P, Cin, Cout, int(bool(c.deferred_in)), dt)
                 and (radd_s is None or (not c.deferred_in and radd_s.dtype == c.e.dtype and tuple(radd_s.shape) == tuple(c.x.shape)
                                         and is_nhwc(radd_s))))
    if sweep:
        return _bwd_pw_sweep(c)
    return _bwd_pw_split(c)


def _bwd_pw_fused(c):
    """tss_pwconv_bwd_fused[_drop]: input, weight and bias gradient of the layer from one sweep."""
    e_in = _new_e_in(c)
    if e_in is None:
        return None, _NO_EXTRAS
    P, Cin, Cout, weight, drop_mask = c.P, c.Cin, c.Cout, c.weight, c.drop_mask
    rows = (N.lib().tss_pwconv_bwd_fused_drop_rows(P) if drop_mask is not None
            else N.lib().tss_pwconv_bwd_fused_rows(P, Cin, Cout))
    ws = c.tmp((rows, Cout * Cin))
    bws = dbias = dbias_ret = None
    if c.has_bias:          # the bias gradient leaves the same sweep as per-block rows (no colsum launch, no atomics)
        bws = c.tmp((rows, Cout))
        dbias, dbias_ret = _grad_target(c.p_bias, weight, Cout)
    if drop_mask is not None:
        call('tss_pwconv_bwd_fused_drop', *c.gargs, ptr(weight), *c.xargs, int(bool(c.deferred_in)), ptr(drop_mask),
             c.cfg.drop_p, ptr(e_in), ld(e_in), c.bst, ptr(ws), ptr(bws), P, Cin, Cout, c.dt, c.st)
    else:
        call('tss_pwconv_bwd_fused', *c.gargs, ptr(weight), _shadow(weight, 1), *c.xargs, int(bool(c.deferred_in)),
             ptr(e_in), ld(e_in), c.bst, ptr(ws), ptr(bws), P, Cin, Cout, c.dt, c.st)
    # weight and bias rows together: both queued for the end of the pass (summed with the depthwise rows), or both added now because
    # one of the two gradients goes back to autograd
    returned = c.dw_ret if c.dw_ret is not None else dbias_ret
    _add_rows(ws, c.dw, Cout * Cin, rows, c.p_weight, returned)
    if bws is not None:
        _add_rows(bws, dbias, Cout, rows, c.p_bias, returned)
    return e_in, (None, True, dbias_ret)


def _bwd_pw_sweep(c):
    """tss_pwconv_bwd_sweep: input and weight gradient from one sweep; adds the skip's gradient in its epilogue."""
    e_in = _new_e_in(c)
    if e_in is None:
        return None, _NO_EXTRAS
    P, Cin, Cout, weight = c.P, c.Cin, c.Cout, c.weight
    fork, radd_s = _res_grad(c.cfg)
    rows = N.lib().tss_pwconv_bwd_sweep_rows(P, Cin, Cout)
    ws = c.tmp((rows, Cout * Cin))
    wT = _shadow(weight, 1)
    hold_wT = None
    if wT is None:          # no current shadow (plain autograd outside a Trainer): a transpose of this call's own
        hold_wT = weight.detach().reshape(Cout, Cin).t().contiguous().to(torch.bfloat16)
        wT = ptr(hold_wT)
    call('tss_pwconv_bwd_sweep', *c.gargs, wT, *c.xargs, int(bool(c.deferred_in)), ptr(radd_s),
         ld(radd_s) if radd_s is not None else 0, ptr(e_in), ld(e_in), c.bst, ptr(ws), P, Cin, Cout, c.dt, c.st)
    del hold_wT
    if radd_s is not None:
        fork.consumed = True
    _add_rows(ws, c.dw, Cout * Cin, rows, c.p_weight, c.dw_ret)       # summed with the depthwise rows, at the end of the pass
    return e_in, _NO_EXTRAS


def _bwd_pw_split(c):
    """Weight gradient and input gradient as two launches: the weight gradient at once, or postponed behind the input gradient until
    the next BatchNorm-backward finalize of this pass is due, which it then carries (see _Pass.wg)."""
    P, Cin, Cout, dt = c.P, c.Cin, c.Cout, c.dt
    nws = N.lib().tss_pwconv_bwd_weight_ws(P, Cin, Cout, dt) if c.y is not None else 0
    ws = c.tmp(nws) if nws else None
    defer = 1 if (ws is not None and c.need_dx and c.side is None) else 0   # a backward-data launch carries the reduce
    postponed = bool(defer and postpone_wgrad and c.dw_ret is None and not c.cfg.overlapped
                     and _backward_task() != -1 and not _param_observed(c.p_weight))
    if not postponed:
        _flush_wg(c.st)
        _flush_red(c.st)
        call('tss_pwconv_bwd_weight', *c.gargs, *c.xargs, ptr(c.dw), ptr(ws), defer, P, Cin, Cout, dt, None, c.wst)
    e_in = _new_e_in(c)
    if e_in is None:
        return None, _NO_EXTRAS
    if postponed:      # this launch carries the slot reduction of an EARLIER layer's weight gradient, if one waits
        red, hold = _take_red(c.dev)
    else:
        red, hold = ((ptr(ws), ptr(c.dw), 0, 0, 0) if defer else (None, None, 0, 0, 0)), None
    _pw_data_grad(c, e_in, red)
    del hold
    if postponed:
        _postpone_pw_wgrad(c, ws)
    return e_in, _NO_EXTRAS


def _pw_data_grad(c, e_in, red):
    """The backward-data launch of a 1x1 layer; `red`: the weight-gradient slot reduction that rides in front of its grid."""
    e, x, y, weight, P, Cin, Cout, dt, st = c.e, c.x, c.y, c.weight, c.P, c.Cin, c.Cout, c.dt, c.st
    deferred_in = c.deferred_in
    fork, radd = _res_grad(c.cfg)
    radd_ok = (radd is not None and not deferred_in and y is not None and e.dtype == torch.bfloat16 and radd.dtype == e.dtype
               and tuple(radd.shape) == tuple(e_in.shape) and N.lib().tss_pwconv_bwd_data_radd_supported(P, Cin, Cout, dt))
    pj = c.cfg.prev_join
    if (pj is not None and (radd is None or radd_ok) and not deferred_in and y is not None and e.dtype == torch.bfloat16
            and P * Cin <= fuse_join_backward_max
            and pj.j_a is not None and tuple(pj.j_a.shape) == tuple(x.shape)
            and is_nhwc(pj.j_a) and N.lib().tss_pwconv_bwd_data_radd_supported(P, Cin, Cout, dt)):
        # this layer's input is a block output: that join's backward (ReLU mask + BatchNorm-backward sums) in the epilogue
        jl = pj.a_link
        call('tss_pwconv_bwd_data_joined', *c.gargs, ptr(weight), _shadow(weight, 1), ptr(e_in), ld(e_in), *red,
             ptr(radd), ld(radd) if radd is not None else 0, ptr(x), ld(x), ptr(pj.j_a), ld(pj.j_a), ptr(jl.mean),
             ptr(jl.bstats), P, Cin, Cout, dt, st)
        pj.fused_e = e_in
        if radd is not None:
            fork.consumed = True
    elif radd_ok:
        call('tss_pwconv_bwd_data_radd', *c.gargs, ptr(weight), _shadow(weight, 1), ptr(e_in), ld(e_in),
             *red, ptr(radd), ld(radd), P, Cin, Cout, dt, st)
        fork.consumed = True
    else:
        call('tss_pwconv_bwd_data', *c.gargs, ptr(weight), _shadow(weight, 1), *c.margs, ptr(e_in), ld(e_in), c.bst,
             *red, P, Cin, Cout, dt, st)


def _postpone_pw_wgrad(c, ws):
    """Register this layer's weight-gradient launch with the running pass: the next BatchNorm-backward finalize on this stream rides
    in front of its grid (_bn_bwd_finalize), or the end of the pass flushes it.  The closure's defaults keep every tensor the launch
    reads alive until then; its slot reduction waits in _Pass.red for the next backward-data launch."""
    st = c.st
    _flush_wg(st)          # at most one weight gradient waits per stream
    own = torch.cuda.current_stream(c.dev)
    ps = _cur_pass()

    def launch_wg(fin, _keep=(c.e, c.y, c.x, c.link, c.il, ws, c.dw), _args=(c.gargs, c.xargs, ptr(c.dw), ptr(ws), c.P, c.Cin, c.Cout, c.dt),
                  _sid=st, _own=own, _ps=ps):
        ga_, xa_, dwp, wsp, P_, K_, N_, dt_ = _args
        call('tss_pwconv_bwd_weight', *ga_, *xa_, dwp, wsp, 1, P_, K_, N_, dt_,
             ctypes.byref(fin) if fin is not None else None, _sid)
        _flush_red(_sid, _ps)
        with _lock:
            _ps.red[_sid] = (_keep[5], _keep[6], P_, K_, N_, _keep[0].device, _own)
    with _lock:
        ps.wg[st] = (launch_wg, c.dev, own)


# ---- the other kinds

def _bwd_dw(c):
    weight, B, Hin, Win, Cout, s, d, dt, st = c.weight, c.B, c.Hin, c.Win, c.Cout, c.s, c.d, c.dt, c.st
    ws = c.tmp((N.stat_slabs(), Cout * 9))
    defer = 1 if (c.need_dx and c.side is None) else 0      # backward-data carries the row reduction
    # input gradient and weight gradient in ONE sweep when the shape allows (e, y, x read once)
    fused = bool(defer and ((fuse_dw_backward and N.lib().tss_dwconv3x3_bwd_fused_supported(Cout, s, d, dt))
                            or N.lib().tss_dwconv3x3_bwd_fused_preferred(Cout, s, d, dt)))
    if not fused:
        call('tss_dwconv3x3_bwd_weight', *c.gargs, *c.xargs, ptr(c.dw), ptr(ws), defer, B, Hin, Win, Cout, s, d, dt, c.wst)
    e_in = _new_e_in(c)
    if e_in is None:
        return None, _NO_EXTRAS
    if fused and c.dw_ret is None and batch_dw_reductions:
        # the rows of per-block partial sums stay in ws; they are added to the (direct) gradient together with
        # those of every other depthwise layer, in one launch at the end of this backward pass
        rows = ctypes.c_int(0)
        call('tss_dwconv3x3_bwd_fused_sweep', *c.gargs, ptr(weight), *c.xargs, int(bool(c.deferred_in)), ptr(e_in), ld(e_in),
             c.bst, ptr(ws), B, Hin, Win, Cout, s, d, dt, st, ctypes.byref(rows))
        _add_rows(ws, c.dw, Cout * 9, rows.value, c.p_weight, c.dw_ret)      # (queued: the test above is _add_rows' own)
    elif fused:
        call('tss_dwconv3x3_bwd_fused', *c.gargs, ptr(weight), *c.xargs, int(bool(c.deferred_in)), ptr(e_in), ld(e_in),
             c.bst, ptr(ws), ptr(c.dw), B, Hin, Win, Cout, s, d, dt, st)
    else:
        call('tss_dwconv3x3_bwd_data', *c.gargs, ptr(weight), *c.margs, ptr(e_in), ld(e_in), c.bst,
             ptr(ws) if defer else None, ptr(c.dw) if defer else None, B, Hin, Win, Cout, s, d, dt, st)
    return e_in, _NO_EXTRAS


def _tap_sweep_wgrad(c, entry, rows, taps, *geom):
    """Weight gradient of a tap-row layer from one sweep over e, y and x (csrc/fc1d.hip, fcg.hip, sconv.hip).  The sweep may be on the
    side stream: its rows of per-block partial sums are queued / added after the join, together with those of every other such layer
    in one launch at the end of the backward pass.  Returns the handler's rows_after_join."""
    ncols = c.Cout * c.Cin * taps
    ws = c.tmp((rows, ncols))
    call(entry, *c.gargs, *c.xargs, ptr(ws), c.B, c.Hin, c.Win, c.Cin, c.Cout, *geom, c.dt, c.wst)
    return ws, rows, ncols


def _pw_wgrad_of_columns(c, gargs, col, K):
    """The pointwise weight-gradient kernel on an unfolded input (col: bf16 [P][K], no pending BatchNorm), complete on return."""
    nws = N.lib().tss_pwconv_bwd_weight_ws(c.P, K, c.Cout, c.dt)
    ws = c.tmp(nws) if nws else None
    call('tss_pwconv_bwd_weight', *gargs, ptr(col), K, None, None, None, 0, ptr(c.dw), ptr(ws), 0,
         c.P, K, c.Cout, c.dt, None, c.wst)


def _dense1d_wgrad(c, axis):
    """Weight gradient of a 1x3 / 3x1 layer; returns rows_after_join."""
    e, y, P, Cin, Cout, d, dt = c.e, c.y, c.P, c.Cin, c.Cout, c.d, c.dt
    rows = N.lib().tss_conv1d3_bwd_weight_rows(P, Cin, Cout, dt)
    rows_w = 0 if rows else N.lib().tss_convtap_bwd_weight_rows(P, Cin, Cout, 3, dt)      # 128-channel layers (csrc/fcg.hip)
    if rows_w:
        return _tap_sweep_wgrad(c, 'tss_convtap_bwd_weight_sweep', rows_w, 3, 3, axis, d)
    if rows:
        return _tap_sweep_wgrad(c, 'tss_conv1d3_bwd_weight_sweep', rows, 3, axis, d)
    if (e.dtype == torch.bfloat16 and Cin % 8 == 0 and Cout % 8 == 0 and unfold_1d_wgrad and not N.fast_paths_disabled()):
        # unfold once (bf16 [P][Cin*3], column c*3 + tap), then the pipelined pointwise MFMA weight-gradient kernel with
        # K = 3*Cin writes torch's [N][Cin][1][3] / [N][Cin][3][1] layout directly (as the dense 3x3)
        col = c.tmp((P, Cin * 3), torch.bfloat16)
        call('tss_im2col1d3', *c.xargs, ptr(col), c.B, c.Hin, c.Win, Cin, axis, d, dt, c.wst)
        g_ = c.gargs
        if y is None:        # no BatchNorm behind this layer (or a frozen one): g = ga * e, written as ga * e + 0 * e + 0
            one, zero = _const_rows(c.dev, Cout)
            g_ = (ptr(e), ld(e), ptr(e), ld(e), ptr(c.ga) if c.ga is not None else ptr(one), ptr(zero), ptr(zero), ptr(zero))
        _pw_wgrad_of_columns(c, g_, col, Cin * 3)
    else:
        call('tss_conv1d3_bwd_weight', *c.gargs, *c.xargs, ptr(c.dw), c.B, c.Hin, c.Win, Cin, Cout, axis, d, dt, c.wst)
    return None


def _bwd_dense1d(c):
    weight, B, Hin, Win, Cin, Cout, d, dt, st = c.weight, c.B, c.Hin, c.Win, c.Cin, c.Cout, c.d, c.dt, c.st
    axis = 0 if c.cfg.kind == 'dense1d_w' else 1
    extras = (_dense1d_wgrad(c, axis), False, None)
    e_in = _new_e_in(c)
    if e_in is None:
        return None, extras
    if N.lib().tss_conv1d3_lean_supported(Cin, Cout, dt):
        call('tss_conv1d3_bwd_data_w', *c.gargs, ptr(weight), *c.margs, ptr(e_in), ld(e_in), c.bst,
             B, Hin, Win, Cin, Cout, axis, d, dt, st)
    else:
        w_tcn = c.tmp((3, Cin, Cout))
        call('tss_permute_wtaps', ptr(weight), None, ptr(w_tcn), Cout, Cin, 3, st)
        call('tss_conv1d3_bwd_data', *c.gargs, ptr(w_tcn), *c.margs, ptr(e_in), ld(e_in), c.bst,
             B, Hin, Win, Cin, Cout, axis, d, dt, st)
    return e_in, extras


def _kxk_data_grad(c, e_in):
    """General tap grid / transposed gather of a strided layer (generic implicit-GEMM kernel)."""
    cfg, Cin, Cout, st = c.cfg, c.Cin, c.Cout, c.st
    nt = cfg.kh * cfg.kw
    w_tcn = c.tmp((nt, Cin, Cout))
    call('tss_permute_wtaps', ptr(c.weight), None, ptr(w_tcn), Cout, Cin, nt, st)
    call('tss_convkxk_bwd_data', *c.gargs, ptr(w_tcn), *c.margs, ptr(e_in), ld(e_in), c.bst,
         c.B, c.Hin, c.Win, Cin, Cout, cfg.kh, cfg.kw, c.s, c.d, c.dt, st)


def _bwd_ckk(c):
    cfg, P, Cin, Cout, s, d, dt = c.cfg, c.P, c.Cin, c.Cout, c.s, c.d, c.dt
    rows_after_join = None
    if (s == 1 and (cfg.kh, cfg.kw) in ((1, 5), (5, 1)) and N.lib().tss_convtap_bwd_weight_rows(P, Cin, Cout, 5, dt)):
        # ESNet's 64-channel 1x5 / 5x1 layers: one sweep over e, y and x (csrc/fcg.hip), rows added at the end of the pass
        rows = N.lib().tss_convtap_bwd_weight_rows(P, Cin, Cout, 5, dt)
        rows_after_join = _tap_sweep_wgrad(c, 'tss_convtap_bwd_weight_sweep', rows, 5, 5, 0 if cfg.kh == 1 else 1, d)
    else:
        call('tss_convkxk_bwd_weight', *c.gargs, *c.xargs, ptr(c.dw), c.B, c.Hin, c.Win, Cin, Cout, cfg.kh, cfg.kw, s, d, dt, c.wst)
    e_in = _new_e_in(c)
    if e_in is not None:
        _kxk_data_grad(c, e_in)
    return e_in, (rows_after_join, False, None)


def _dense_wgrad(c):
    """Weight gradient of a dense 3x3 layer; returns rows_after_join."""
    e, B, Hin, Win, P, Cin, Cout, s, d, dt = c.e, c.B, c.Hin, c.Win, c.P, c.Cin, c.Cout, c.s, c.d, c.dt
    if (s == 2 and d == 1 and N.lib().tss_sconv_bwd_weight_rows(B, Hin, Win, Cin, Cout, dt)):
        # stride-2 3x3 of the downsampling blocks: one sweep over e and x (csrc/sconv.hip), rows added at the end of the pass
        rows = N.lib().tss_sconv_bwd_weight_rows(B, Hin, Win, Cin, Cout, dt)
        return _tap_sweep_wgrad(c, 'tss_sconv_bwd_weight_sweep', rows, 9)
    if (e.dtype == torch.bfloat16 and s == 1 and c.y is not None and (Cin * 9) % 8 == 0 and Cout % 8 == 0
            and not N.fast_paths_disabled()):
        # unfold once (bf16 [P][Cin*9], column c*9 + tap), then the pointwise MFMA weight-gradient kernel with
        # K = 9*Cin writes torch's [N][Cin][3][3] layout directly
        col = c.tmp((P, Cin * 9), torch.bfloat16)
        call('tss_im2col3x3', *c.xargs, ptr(col), B, Hin, Win, Cin, d, dt, c.wst)
        _pw_wgrad_of_columns(c, c.gargs, col, Cin * 9)
    else:
        call('tss_conv3x3_bwd_weight', *c.gargs, *c.xargs, ptr(c.dw), B, Hin, Win, Cin, Cout, s, d, dt, c.wst)
    return None


def _bwd_dense(c):
    weight, Cin, Cout, d, st = c.weight, c.Cin, c.Cout, c.d, c.st
    extras = (_dense_wgrad(c), False, None)
    e_in = _new_e_in(c)
    if e_in is None:
        return None, extras
    if c.s != 1:
        _kxk_data_grad(c, e_in)
        return e_in, extras
    w_tcn = w_tcn16 = None
    if _conv3x3_lean(c.e.dtype, Cout, Cin, 1, d):       # contraction over Cout, outputs = Cin
        w_tcn16 = c.tmp((9, Cin, Cout), torch.bfloat16)
        call('tss_permute_w3x3_bf16', ptr(weight), None, ptr(w_tcn16), Cout, Cin, st)
    else:
        w_tcn = c.tmp((9, Cin, Cout))
        call('tss_permute_w3x3', ptr(weight), None, ptr(w_tcn), Cout, Cin, st)
    call('tss_conv3x3_bwd_data', *c.gargs, ptr(w_tcn), ptr(w_tcn16), *c.margs, ptr(e_in), ld(e_in), c.bst,
         c.B, c.Hin, c.Win, Cin, Cout, d, c.dt, st)
    return e_in, extras


# keyed by what _classify returns
_BWD = {'stem': _bwd_stem, 'pw': _bwd_pw, 'dw': _bwd_dw, 'ckk': _bwd_ckk, 'dense': _bwd_dense,
        'dense1d_w': _bwd_dense1d, 'dense1d_h': _bwd_dense1d}


def _bias_backward(c):
    """d(bias) of a layer whose backward sweep has not produced it.  Returns the tensor for autograd (None: accumulated directly)."""
    e, P, Cout, link = c.e, c.P, c.Cout, c.link
    if link is not None and link.training:
        # BatchNorm with batch statistics removes any per-channel shift: d(loss)/d(bias) is exactly zero
        return _grad_target(c.p_bias, c.weight, Cout)[1]
    if link is not None:          # frozen statistics: d(bias) = scale * sum(e)
        dbias = _direct_target(c.p_bias)
        tmp = torch.zeros(Cout, dtype=torch.float32, device=c.dev)
        _bias_grad_into(e, P, Cout, tmp, c.dt, c.st)
        if dbias is None:
            return tmp * link.ga
        dbias.addcmul_(tmp, link.ga)
        return None
    dbias, dbias_ret = _grad_target(c.p_bias, c.weight, Cout)
    _bias_grad_into(e, P, Cout, dbias, c.dt, c.st)
    return dbias_ret


class ConvUnitFn(Function):
    @staticmethod
    def forward(ctx, x, weight, gamma, beta, bias, cfg):
        dev = x.device
        B = x.shape[0]
        dt = N.dtype_code(cfg.out_dtype)
        s, d = cfg.stride, cfg.dil
        Hin, Win = x.shape[2], x.shape[3]
        Ho, Wo = (Hin - 1) // s + 1, (Win - 1) // s + 1
        Cout = cfg.cout
        y = new_nhwc(B, Cout, Ho, Wo, cfg.out_dtype, dev)
        P = B * Ho * Wo
        link = None
        if cfg.bn is not None:
            if cfg.training and P <= 1:
                raise ValueError('Expected more than 1 value per channel when training, got input size %s'
                                 % (tuple(y.shape),))
            link = BNLink(Cout, P, cfg.training, gamma, beta, dev)
        stats = ptr(link.stats) if (link is not None and cfg.training) else None
        st = stream()
        mask = _FWD[cfg.kind](_FwdArgs(cfg, x, weight, bias, y, _aff(cfg.in_link), stats, B, Hin, Win, Cout, P, s, d, dt, dev, st))
        if link is not None:
            _finalize_forward(link, cfg.bn, cfg.training, P, Cout, gamma, st)
        cfg.out_link = link
        ctx.cfg = cfg
        ctx.save_for_backward(x, weight, y if link is not None else None, mask)
        ctx.has_bias = bias is not None
        ctx.has_affine = gamma is not None
        return y

    @staticmethod
    def backward(ctx, e):
        cfg = ctx.cfg
        c = _Bwd()
        c.cfg, c.temps = cfg, []
        x, weight, y, drop_mask = ctx.saved_tensors
        c.x, c.weight, c.drop_mask = x, weight, drop_mask
        c.dev = dev = x.device
        c.e = e = to_nhwc(e)
        c.dt = N.dtype_code(e.dtype)
        c.st = st = stream()
        c.link = link = cfg.out_link
        c.B, c.Hin, c.Win = x.shape[0], x.shape[2], x.shape[3]
        c.s, c.d = cfg.stride, cfg.dil
        c.Cout, c.Cin = cfg.cout, cfg.cin
        Cout = c.Cout
        c.P = P = npix(e)
        c.p_weight, p_gamma, p_beta, c.p_bias = cfg.params
        dgamma, dbeta, c.y, c.ga, gb, gce, gmu = _bn_backward_prologue(link, ctx.has_affine, p_gamma, p_beta, Cout, y, dev, st)
        y = c.y
        c.gargs = (ptr(e), ld(e), ptr(y), ld(y) if y is not None else 0, ptr(c.ga), ptr(gb), ptr(gce), ptr(gmu))
        c.il = il = cfg.in_link
        c.xargs = (ptr(x), ld(x), *_aff(il), int(cfg.in_relu))
        c.deferred_in = il is not None or cfg.in_relu
        c.margs = c.xargs if c.deferred_in else (None, 0, None, None, None, 0)
        c.bst = ptr(il.bstats) if il is not None else None
        c.dw, c.dw_ret = _grad_target(c.p_weight, weight)
        c.need_dx = need_dx = ctx.needs_input_grad[0]
        c.has_bias = ctx.has_bias
        # backward-weight and backward-data of one layer are independent: the weight gradient goes to a side stream
        # (fork after the finalize above, join before this function returns, so every tensor it reads is still alive
        # and a HIP-graph capture sees two parallel branches)
        main = torch.cuda.current_stream(dev)
        c.side = side = _wgrad_side_stream(cfg, need_dx, drop_mask, P, dev)
        c.wst = st
        if side is not None:
            side.wait_stream(main)
            c.wst = side.cuda_stream
        e_in, (rows_after_join, bias_done, dbias_ret) = _BWD[cfg.kind](c)
        stash = cfg.stash_fork
        if stash is not None and e_in is not None and not c.deferred_in:
            stash.g2 = e_in                # the other consumer of this layer's input adds it in its own backward (fork_two)
        if ctx.has_bias and not bias_done:
            dbias_ret = _bias_backward(c)
        if side is not None:
            main.wait_stream(side)
        if rows_after_join is not None:
            ws, rows, ncols = rows_after_join
            _add_rows(ws, c.dw, ncols, rows, c.p_weight, c.dw_ret)
        return e_in, c.dw_ret, dgamma, dbeta, dbias_ret, None


# ----------------------------------------------------------------------------- join (materialise / add / relu)

class JoinCfg:
    __slots__ = ('a_link', 'b_link', 'relu', 'drop_p', 'res_fork', 'j_a', 'fused_e')


class BranchCfg:
    """Pending BatchNorm links and ReLU flags of the branches that ssnbt_tail, concat_joined and concat_upsampled_arms write into
    one buffer; res_fork: the stash of concat_upsampled_arms' first operand (fork_two)."""
    __slots__ = ('links', 'relus', 'res_fork')


class PpmArmsCfg:
    """The modules of the arms that ppm_arms runs in one launch, and the links their BatchNorms leave pending."""
    __slots__ = ('convs', 'bns', 'links')


def join(a, b=None, relu=False, dropout_p=0.0, fork=None):
    """relu?(bn_a(a) + bn_b(b)) -> ordinary NHWC tensor.  a, b: Deferred (without pending ReLU) or tensors.
    dropout_p > 0 (ReLU joins only): nn.Dropout applied in the same pass, forward and backward."""
    a = as_deferred(a).take()
    cfg = JoinCfg()
    cfg.relu = bool(relu)
    cfg.drop_p = float(dropout_p)
    if cfg.drop_p and not (relu and 0.0 < cfg.drop_p < 1.0):
        raise RuntimeError('join: dropout can only be folded into a ReLU join, 0 < p < 1')
    if a.relu and (b is not None or not relu):
        raise RuntimeError('join: a pending ReLU can only be folded into a single-input relu join')
    cfg.a_link = a.link
    braw = None
    cfg.b_link = None
    if b is not None:
        b = as_deferred(b).take()
        if b.relu:
            raise RuntimeError('join: operand b carries a pending ReLU; materialize it first')
        if b.raw.shape != a.raw.shape or b.raw.dtype != a.raw.dtype:
            raise RuntimeError('join: operands differ in shape/dtype: %s vs %s' % (a.raw.shape, b.raw.shape))
        braw, cfg.b_link = b.raw, b.link
    cfg.res_fork = fork if b is not None else None
    cfg.j_a = cfg.fused_e = None
    out = JoinFn.apply(a.raw, braw, cfg)
    if (fuse_join_backward and cfg.relu and not cfg.drop_p and cfg.a_link is not None and cfg.b_link is None and out.requires_grad
            and out.dtype == torch.bfloat16 and not N.fast_paths_disabled()):
        cfg.j_a = a.raw
        _hand(out, _JOIN, cfg)            # taken by the conv unit (or residual_fork) that consumes `out`, if one does
    return out


class JoinFn(Function):
    @staticmethod
    def forward(ctx, a, b, cfg):
        out = new_nhwc(*a.shape, a.dtype, a.device)
        al, bl = cfg.a_link, cfg.b_link
        slot = None
        if cfg.drop_p:
            slot = torch.empty(1, dtype=torch.int64, device=a.device)
            call('tss_dropout_tick', ptr(_dropout_counter(a.device)), ptr(slot), stream())
        call('tss_join_fwd', ptr(a), ld(a), *_aff(al), ptr(b), ld(b) if b is not None else 0, *_aff(bl),
             ptr(out), ld(out), int(cfg.relu), cfg.drop_p, ptr(slot), npix(a), a.shape[1], N.dtype_code(a.dtype), stream())
        ctx.cfg = cfg
        ctx.has_b = b is not None
        ctx.save_for_backward(a if al is not None else None, b if bl is not None else None,
                              out if cfg.relu else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        cfg = ctx.cfg
        a, b, out = ctx.saved_tensors
        fe = cfg.fused_e
        cfg.fused_e = None
        if (fe is not None and dout.data_ptr() == fe.data_ptr() and dout.shape == fe.shape and dout.dtype == fe.dtype
                and dout.stride() == fe.stride()):
            # the consumer's backward-data launch already did this join's backward on the complete gradient (mask + slab rows written):
            # dout IS e.  (Any other gradient of `out` would have made autograd hand us a different, summed tensor.)
            fork = cfg.res_fork
            if fork is not None and ctx.has_b:
                fork.g2 = dout
            return dout, (dout if ctx.has_b else None), None
        del fe
        dout = to_nhwc(dout)
        al, bl = cfg.a_link, cfg.b_link
        e = new_nhwc(*dout.shape, dout.dtype, dout.device) if cfg.relu else None
        if cfg.relu or al is not None or bl is not None:
            call('tss_join_bwd', ptr(dout), ld(dout), ptr(out), ld(out) if out is not None else 0, int(cfg.relu),
                 ptr(a), ld(a) if a is not None else 0, ptr(al.mean) if al else None, ptr(al.bstats) if al else None,
                 ptr(b), ld(b) if b is not None else 0, ptr(bl.mean) if bl else None, ptr(bl.bstats) if bl else None,
                 ptr(e), ld(e) if e is not None else 0, 1.0 / (1.0 - cfg.drop_p) if cfg.drop_p else 1.0,
                 npix(dout), dout.shape[1], N.dtype_code(dout.dtype), stream())
        g = e if e is not None else dout
        fork = cfg.res_fork
        if fork is not None and ctx.has_b:
            fork.g2 = g                    # the skip's gradient, for the epilogue of the block's first layer
        return g, (g if ctx.has_b else None), None


# ----------------------------------------------------------------------------- dropout

_dropout_counters = {}


def _dropout_counter(device):
    return _per_device(_dropout_counters, device,
                       lambda: torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF], dtype=torch.int64, device=device))


def dropout(x, p, training):
    """nn.Dropout on a materialised NHWC tensor (Philox mask, regenerated in backward)."""
    if not training or p == 0.0:
        return x
    if p >= 1.0:
        raise NotImplementedError('HIP path: dropout with p >= 1')
    return DropoutFn.apply(to_nhwc(x), float(p))


class DropoutFn(Function):
    @staticmethod
    def forward(ctx, x, p):
        slot = torch.empty(1, dtype=torch.int64, device=x.device)
        call('tss_dropout_tick', ptr(_dropout_counter(x.device)), ptr(slot), stream())
        y = new_nhwc(*x.shape, x.dtype, x.device)
        call('tss_dropout', ptr(x), ld(x), ptr(y), ld(y), npix(x), x.shape[1], p, ptr(slot),
             N.dtype_code(x.dtype), stream())
        ctx.p = p
        ctx.save_for_backward(slot)
        return y

    @staticmethod
    def backward(ctx, dy):
        (slot,) = ctx.saved_tensors
        dy = to_nhwc(dy)
        dx = new_nhwc(*dy.shape, dy.dtype, dy.device)
        call('tss_dropout', ptr(dy), ld(dy), ptr(dx), ld(dx), npix(dy), dy.shape[1], ctx.p, ptr(slot),
             N.dtype_code(dy.dtype), stream())
        return dx, None


# ----------------------------------------------------------------------------- resampling

def _out_size(x, size, scale_factor):
    if size is not None:
        return (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    sf = (scale_factor, scale_factor) if not isinstance(scale_factor, (tuple, list)) else scale_factor
    # torch: output = floor(input * scale_factor)
    import math
    return int(math.floor(x.shape[2] * sf[0])), int(math.floor(x.shape[3] * sf[1]))


def bilinear(x, size=None, scale_factor=None, out=None):
    """F.interpolate(mode='bilinear', align_corners=True) on an NHWC activation tensor."""
    x = to_nhwc(materialize(x))
    ho, wo = _out_size(x, size, scale_factor)
    return BilinearFn.apply(x, ho, wo)


class BilinearFn(Function):
    @staticmethod
    def forward(ctx, x, ho, wo):
        B, C, H, W = x.shape
        y = new_nhwc(B, C, ho, wo, x.dtype, x.device)
        call('tss_bilinear_nhwc_fwd', ptr(x), ld(x), ptr(y), ld(y), B, H, W, ho, wo, C,
             N.dtype_code(x.dtype), stream())
        ctx.geom = (B, C, H, W, ho, wo)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, H, W, ho, wo = ctx.geom
        dy = to_nhwc(dy)
        dx = new_nhwc(B, C, H, W, dy.dtype, dy.device)
        tmp = torch.empty((B * H * wo * C,), dtype=torch.float32, device=dy.device)
        call('tss_bilinear_nhwc_bwd', ptr(dy), ld(dy), ptr(dx), ld(dx), ptr(tmp), B, H, W, ho, wo, C,
             N.dtype_code(dy.dtype), stream())
        return dx, None, None


class _UpDwCfg:
    __slots__ = ('size', 'dil', 'bn', 'training', 'out_link', 'params')


def upsample_dw_unit(x, size, block):
    """Bilinear upsample (align_corners=True) to `size` followed by `block` = depthwise 3x3 conv (padding = dilation) -> [BatchNorm]
    -> [ReLU] as ONE deferred unit (csrc/updw.hip): the upsampled tensor is never written -- the low-resolution branch of the
    feature-fusion modules (TSS/models/fastscnn.py:74-76, TSS/models/contextnet.py:110-122).  Returns a Deferred, or None when
    the call is outside the kernel's envelope (the caller then runs the two operators one after the other).  TSS_UPDW=0: never."""
    mods = list(block) if isinstance(block, torch.nn.Sequential) else None
    if mods is None or not mods or N.fast_paths_disabled():
        return None
    conv = mods[0]
    bn = mods[1] if len(mods) > 1 and isinstance(mods[1], _BatchNorm) else None
    relu = isinstance(mods[-1], torch.nn.ReLU) and len(mods) > 1
    if len(mods) != 1 + int(bn is not None) + int(relu) or not isinstance(conv, torch.nn.Conv2d) or conv.bias is not None:
        return None
    try:
        kind, s, d = _classify(conv, False)
    except NotImplementedError:
        return None
    if kind != 'dw' or s != 1:
        return None
    x = to_nhwc(materialize(x))
    ho, wo = int(size[0]), int(size[1])
    B, C, Hs, Ws = x.shape
    if (x.dtype != torch.bfloat16 or C != conv.in_channels
            or not N.lib().tss_updw_supported(B, Hs, Ws, ho, wo, C, d, N.dtype_code(x.dtype))):
        return None
    cfg = _UpDwCfg()
    cfg.size, cfg.dil, cfg.bn, cfg.training = (ho, wo), d, bn, False
    gamma = beta = None
    if bn is not None:
        cfg.training = bn.training or (bn.running_mean is None and bn.running_var is None)
        if cfg.training and bn.momentum is None:
            return None
        gamma, beta = bn.weight, bn.bias
    cfg.params = (conv.weight, gamma, beta)
    y = UpDwFn.apply(x, _f32(conv.weight), _f32(gamma), _f32(beta), cfg)
    return Deferred(y, cfg.out_link, relu)


class UpDwFn(Function):
    @staticmethod
    def forward(ctx, x, weight, gamma, beta, cfg):
        dev, st = x.device, stream()
        B, C, Hs, Ws = x.shape
        ho, wo = cfg.size
        y = new_nhwc(B, C, ho, wo, x.dtype, dev)
        P = B * ho * wo
        link = None
        if cfg.bn is not None:
            if cfg.training and P <= 1:
                raise ValueError('Expected more than 1 value per channel when training, got input size %s' % (tuple(y.shape),))
            link = BNLink(C, P, cfg.training, gamma, beta, dev)
        stats = ptr(link.stats) if (link is not None and cfg.training) else None
        call('tss_updw_fwd', ptr(x), ld(x), Hs, Ws, ptr(weight), ptr(y), ld(y), stats, B, ho, wo, C, cfg.dil,
             N.dtype_code(x.dtype), st)
        if link is not None:
            _finalize_forward(link, cfg.bn, cfg.training, P, C, gamma, st)
        cfg.out_link = link
        ctx.cfg = cfg
        ctx.save_for_backward(x, weight, y if link is not None else None)
        ctx.has_affine = gamma is not None
        return y

    @staticmethod
    def backward(ctx, e):
        cfg = ctx.cfg
        x, weight, y = ctx.saved_tensors
        dev, st = x.device, stream()
        e = to_nhwc(e)
        dt = N.dtype_code(e.dtype)
        B, C, Hs, Ws = x.shape
        ho, wo = cfg.size
        link = cfg.out_link
        p_weight, p_gamma, p_beta = cfg.params
        dgamma, dbeta, y, ga, gb, gce, gmu = _bn_backward_prologue(link, ctx.has_affine, p_gamma, p_beta, C, y, dev, st)
        dw, dw_ret = _grad_target(p_weight, weight)
        ws = torch.empty((N.lib().tss_updw_ws_rows(B, Hs, Ws, ho, wo, C, cfg.dil, dt), C * 9), dtype=torch.float32, device=dev)
        e_up = new_nhwc(B, C, ho, wo, e.dtype, dev)
        rows = ctypes.c_int(0)
        call('tss_updw_bwd', ptr(e), ld(e), ptr(y), ld(y) if y is not None else 0, ptr(ga), ptr(gb), ptr(gce), ptr(gmu),
             ptr(weight), ptr(x), ld(x), Hs, Ws, ptr(e_up), ld(e_up), ptr(ws), B, ho, wo, C, cfg.dil, dt, st, ctypes.byref(rows))
        _add_rows(ws, dw, C * 9, rows.value, p_weight, dw_ret)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = new_nhwc(B, C, Hs, Ws, e.dtype, dev)
            tmp = torch.empty((B * Hs * wo * C,), dtype=torch.float32, device=dev)
            call('tss_bilinear_nhwc_bwd', ptr(e_up), ld(e_up), ptr(dx), ld(dx), ptr(tmp), B, Hs, Ws, ho, wo, C, dt, st)
        return dx, dw_ret, dgamma, dbeta, None


def resize_image(x, size=None, scale_factor=None, out_dtype=None):
    """Bilinear (align_corners=True) resize of the NCHW image itself (ContextNet's context branch input,
    TSS/models/contextnet.py:65-67).  No gradient flows to the image."""
    _check_device(x)
    x = x.contiguous()
    ho, wo = _out_size(x, size, scale_factor)
    B, C, H, W = x.shape
    out_dtype = out_dtype or x.dtype
    y = torch.empty((B, C, ho, wo), dtype=out_dtype, device=x.device)
    call('tss_bilinear_planar_fwd', ptr(x), N.dtype_code(x.dtype), ptr(y), N.dtype_code(out_dtype),
         B * C, H, W, ho, wo, stream())
    return y


def upsample_logits(low, scale_factor=None, size=None):
    """The decoder head's final F.interpolate: NHWC low-res logits -> NCHW-contiguous full-res logits."""
    low = to_nhwc(materialize(low))
    ho, wo = _out_size(low, size, scale_factor)
    if wo % 8:
        raise NotImplementedError('HIP path: logits width must be a multiple of 8, got %d' % wo)
    return UpsampleHeadFn.apply(low, ho, wo)


class Upsample(torch.nn.Module):
    """nn.Upsample(scale_factor=k, mode='bilinear', align_corners=True) on the HIP path: the auxiliary heads of the
    reference's deep-supervision recipe (scripts/train_fastscnn.py:108-117) end in one.  NHWC logits in, NCHW-contiguous
    full-resolution logits out (what the losses consume), through tss_upsample_head_{fwd,bwd}."""

    def __init__(self, size=None, scale_factor=None, mode='bilinear', align_corners=True):
        super().__init__()
        if mode != 'bilinear' or not align_corners:
            raise NotImplementedError("HIP path: Upsample(mode='bilinear', align_corners=True) only")
        self.size, self.scale_factor = size, scale_factor

    def forward(self, input):
        return upsample_logits(input, scale_factor=self.scale_factor, size=self.size)

    def extra_repr(self):
        return 'size=%r, scale_factor=%r, mode=bilinear, align_corners=True' % (self.size, self.scale_factor)


class UpsampleHeadFn(Function):
    @staticmethod
    def forward(ctx, low, ho, wo):
        B, C, h, w = low.shape
        y = torch.empty((B, C, ho, wo), dtype=low.dtype, device=low.device)
        call('tss_upsample_head_fwd', ptr(low), ld(low), ptr(y), B, C, h, w, ho, wo,
             N.dtype_code(low.dtype), stream())
        ctx.geom = (B, C, h, w, ho, wo, ld(low))
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, h, w, ho, wo, ldl = ctx.geom
        dy = dy.contiguous()
        tmp = torch.empty((B * C * h * wo,), dtype=torch.float32, device=dy.device)
        # padded channels of dlow must be finite zeros: they are read (and discarded) by 8-wide loaders
        base = torch.zeros((B, h, w, ldl), dtype=dy.dtype, device=dy.device)
        dlow = base.permute(0, 3, 1, 2)[:, :C]
        call('tss_upsample_head_bwd', ptr(dy), None, ptr(tmp), ptr(dlow), ldl, B, C, h, w, ho, wo,
             N.dtype_code(dy.dtype), stream())
        return dlow, None, None


def adaptive_avg_pool(x, bins):
    """nn.AdaptiveAvgPool2d(bins).  Few, large windows (global average pooling: the image-pooling branch of an ASPP head pools ONE
    256 x 512 window per image at 2048 x 4096 -- 1.05 ms through the one-block-per-window kernel) go through the row-sliced
    pyramid-pooling kernel; many small windows through the one-block-per-window kernel."""
    x = to_nhwc(materialize(x))
    bins = int(bins)
    if x.shape[0] * bins * bins <= 128 and x.shape[2] * x.shape[3] >= 4096:
        return PoolMultiFn.apply(x, (bins,), None)[0]
    return AdaptivePoolFn.apply(x, bins)


class AdaptivePoolFn(Function):
    @staticmethod
    def forward(ctx, x, bins):
        B, C, H, W = x.shape
        y = new_nhwc(B, C, bins, bins, x.dtype, x.device)
        call('tss_adaptive_pool_fwd', ptr(x), ld(x), ptr(y), ld(y), B, H, W, C, bins,
             N.dtype_code(x.dtype), stream())
        ctx.geom = (B, C, H, W, bins)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, H, W, bins = ctx.geom
        dy = to_nhwc(dy)
        dx = new_nhwc(B, C, H, W, dy.dtype, dy.device)
        call('tss_adaptive_pool_bwd', ptr(dy), ld(dy), ptr(dx), ld(dx), B, H, W, C, bins,
             N.dtype_code(dy.dtype), stream())
        return dx, None


def concat_upsampled(x, branches):
    """torch.cat([x, *[bilinear(b, size=x.shape[2:]) for b in branches]], dim=1) written in place into one
    NHWC buffer (TSS/models/fastscnn.py:118-122)."""
    x = to_nhwc(materialize(x))
    branches = [to_nhwc(materialize(b)) for b in branches]
    return ConcatUpFn.apply(x, *branches)


class ConcatUpFn(Function):
    @staticmethod
    def forward(ctx, x, *branches):
        B, C, H, W = x.shape
        ctot = C + sum(b.shape[1] for b in branches)
        out = new_nhwc(B, ctot, H, W, x.dtype, x.device)
        dt, st = N.dtype_code(x.dtype), stream()
        call('tss_copy_nhwc', ptr(x), ld(x), ptr(out), ld(out), npix(x), C, dt, st)
        off = C
        geoms = []
        for b in branches:
            cb, hb, wb = b.shape[1], b.shape[2], b.shape[3]
            sl = out[:, off:off + cb]
            call('tss_bilinear_nhwc_fwd', ptr(b), ld(b), ptr(sl), ld(out), B, hb, wb, H, W, cb, dt, st)
            geoms.append((off, cb, hb, wb))
            off += cb
        ctx.geom = (B, C, H, W, geoms)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, C, H, W, geoms = ctx.geom
        dout = to_nhwc(dout)
        dt, st = N.dtype_code(dout.dtype), stream()
        grads = [dout[:, :C]]
        for off, cb, hb, wb in geoms:
            db = new_nhwc(B, cb, hb, wb, dout.dtype, dout.device)
            sl = dout[:, off:off + cb]
            tmp = torch.empty((B * hb * W * cb,), dtype=torch.float32, device=dout.device)
            call('tss_bilinear_nhwc_bwd', ptr(sl), ld(dout), ptr(db), ld(db), ptr(tmp), B, hb, wb, H, W, cb, dt, st)
            grads.append(db)
        return tuple(grads)


def channel_shuffle(x, groups):
    """channel_shuffle of TSS/models/lednet.py:183-188 on an NHWC activation (the channel index is the fastest axis, so this
    is a permutation inside every pixel row)."""
    x = to_nhwc(materialize(x))
    if x.shape[1] % groups or x.shape[1] % 8:
        raise RuntimeError('channel_shuffle: channels must be a multiple of groups and of 8')
    return ChannelShuffleFn.apply(x, int(groups))


class ChannelShuffleFn(Function):
    @staticmethod
    def forward(ctx, x, groups):
        y = new_nhwc(*x.shape, x.dtype, x.device)
        call('tss_channel_shuffle', ptr(x), ld(x), ptr(y), ld(y), npix(x), x.shape[1], groups, N.dtype_code(x.dtype), stream())
        ctx.groups = groups
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = to_nhwc(dy)
        dx = new_nhwc(*dy.shape, dy.dtype, dy.device)
        call('tss_channel_shuffle', ptr(dy), ld(dy), ptr(dx), ld(dx), npix(dy), dy.shape[1], dy.shape[1] // ctx.groups,
             N.dtype_code(dy.dtype), stream())
        return dx, None


def channel_slice(x, C):
    """x[:, :C] of an NHWC tensor computed with padded channels: a view; its gradient is padded back in one pass (tss_pad_channels)."""
    if C == x.shape[1]:
        return x
    return ChannelSliceFn.apply(x, int(C))


class ChannelSliceFn(Function):
    @staticmethod
    def forward(ctx, x, C):
        ctx.cp = x.shape[1]
        return x[:, :C]

    @staticmethod
    def backward(ctx, g):
        B, C, H, W = g.shape
        pitch = g.stride(3)
        if not (g.is_cuda and g.stride(1) == 1 and pitch >= C and g.stride(2) == W * pitch and g.stride(0) == H * W * pitch):
            g = to_nhwc(g)          # (any pitch is fine for the kernel; only a non-channels-last gradient is re-laid out)
        out = new_nhwc(B, ctx.cp, H, W, g.dtype, g.device)
        call('tss_pad_channels', ptr(g), g.stride(3), C, ptr(out), ld(out), ctx.cp, B * H * W, N.dtype_code(g.dtype), stream())
        return out, None


def split_fork(x):
    """(x[:, :C/2], x[:, C/2:], x) for a unit that runs two branches on torch.chunk(input, 2, 1) and adds the whole input back
    (SSnbtBlock, TSS/models/lednet.py:112-124): three views, no copy; the gradient is cat(g_left, g_right) + g_skip in ONE pass
    (tss_cat2_add) instead of autograd's two zero-filled tensors, two slice copies and two additions."""
    x = to_nhwc(materialize(x))
    if x.shape[1] % 16:
        raise NotImplementedError('HIP path: a split unit needs a multiple of 16 channels')
    return SplitForkFn.apply(x)


class SplitForkFn(Function):
    @staticmethod
    def forward(ctx, x):
        half = x.shape[1] // 2
        return x[:, :half], x[:, half:], x.view_as(x)

    @staticmethod
    def backward(ctx, gl, gr, gs):
        ref = gl if gl is not None else (gr if gr is not None else gs)
        if ref is None:
            return None
        B, _, H, W = ref.shape
        half = (ref.shape[1] // 2) if (gl is None and gr is None) else ref.shape[1]
        if gl is None and gr is None:
            return gs
        gl = to_nhwc(gl) if gl is not None else new_nhwc(B, half, H, W, ref.dtype, ref.device).zero_()
        gr = to_nhwc(gr) if gr is not None else new_nhwc(B, half, H, W, ref.dtype, ref.device).zero_()
        gs = to_nhwc(gs) if gs is not None else None
        out = new_nhwc(B, 2 * half, H, W, ref.dtype, ref.device)
        call('tss_cat2_add', ptr(gl), ld(gl), ptr(gr), ld(gr), ptr(gs), ld(gs) if gs is not None else 0, ptr(out), ld(out),
             B * H * W, half, N.dtype_code(ref.dtype), stream())
        return out


fuse_ssnbt_tail = os.environ.get('TSS_SSNBT_TAIL', '1') != '0'     # A/B: 0 = concat_joined, channel_dropout, join, channel_shuffle as four operators


def ssnbt_tail(left, right, x, drop_p, training):
    """channel_shuffle(relu(x + dropout2d(cat([bn(left), bn(right)], 1))), 2): the tail of SSnbtBlock.forward (TSS/models/lednet.py:112-124)
    in one pass each way (csrc/ssnbt.hip).  left / right: Deferreds whose BatchNorm (no ReLU) is still pending; x: the unit's input."""
    dl, dr = as_deferred(left), as_deferred(right)
    x = to_nhwc(materialize(x))
    ok = (fuse_ssnbt_tail and dl.link is not None and dr.link is not None and not dl.relu and not dr.relu
          and dl.raw.shape == dr.raw.shape and dl.raw.dtype == dr.raw.dtype == x.dtype and dl.raw.shape[1] % 8 == 0
          and x.shape[1] == 2 * dl.raw.shape[1] and tuple(x.shape[2:]) == tuple(dl.raw.shape[2:]) and x.shape[0] == dl.raw.shape[0])
    # the envelope of tss_ssnbt_tail_fwd / _bwd (csrc/ssnbt.hip): C <= 512, pitches % 8, 16-byte aligned tensors
    ok = ok and x.shape[1] <= 512 and all(ld(t) % 8 == 0 and t.data_ptr() % 16 == 0 for t in (dl.raw, dr.raw, x))
    if not ok:
        y = concat_joined([dl, dr], relu=False)
        y = channel_dropout(y, drop_p, training)
        return channel_shuffle(join(y, x, relu=True), 2)
    dl.take(); dr.take()
    m = None
    if training and drop_p > 0.0:
        keep = 1.0 - float(drop_p)
        m = (torch.rand((x.shape[0], x.shape[1]), device=x.device) < keep).to(torch.float32)
        if keep > 0.0:
            m = m / keep
    cfg = BranchCfg()
    cfg.links = [dl.link, dr.link]
    return SSnbtTailFn.apply(cfg, dl.raw, dr.raw, x, m)


class SSnbtTailFn(Function):
    @staticmethod
    def forward(ctx, cfg, l, r, x, m):
        B, C, H, W = x.shape
        out = new_nhwc(B, C, H, W, x.dtype, x.device)
        call('tss_ssnbt_tail_fwd', ptr(l), ld(l), *_aff(cfg.links[0]), ptr(r), ld(r), *_aff(cfg.links[1]), ptr(x), ld(x), ptr(m),
             ptr(out), ld(out), B, H * W, C, N.dtype_code(x.dtype), stream())
        ctx.cfg = cfg
        ctx.save_for_backward(out, l, r, m)
        return out

    @staticmethod
    def backward(ctx, dout):
        out, l, r, m = ctx.saved_tensors
        ll, lr = ctx.cfg.links
        dout = to_nhwc(dout)       # is_nhwc: a view with a pitch % 8 or a pointer not 16-byte aligned is copied (the kernel's envelope)
        B, C, H, W = out.shape
        half = C // 2
        gs = new_nhwc(B, C, H, W, dout.dtype, dout.device)
        e = new_nhwc(B, C, H, W, dout.dtype, dout.device) if m is not None else None
        call('tss_ssnbt_tail_bwd', ptr(dout), ld(dout), ptr(out), ld(out), ptr(l), ld(l), ptr(ll.mean), ptr(r), ld(r), ptr(lr.mean),
             ptr(m), ptr(e), ld(e) if e is not None else 0, ptr(gs), ld(gs), ptr(ll.bstats), ptr(lr.bstats), B, H * W, C,
             N.dtype_code(dout.dtype), stream())
        ee = e if e is not None else gs
        return None, ee[:, :half], ee[:, half:], gs, None


def concat(tensors):
    """torch.cat(tensors, dim=1) of equally sized activation tensors into one NHWC buffer (tss_copy_nhwc per operand; the
    gradient is a channel slice of the incoming one, no copy).  Channel counts must be multiples of 8."""
    ts = [to_nhwc(materialize(t)) for t in tensors]
    if any(t.shape[1] % 8 or t.shape[0] != ts[0].shape[0] or t.shape[2:] != ts[0].shape[2:] or t.dtype != ts[0].dtype for t in ts):
        raise RuntimeError('concat: operands must share batch / spatial size / dtype and have channel counts that are multiples of 8')
    return ConcatFn.apply(*ts)


class ConcatFn(Function):
    @staticmethod
    def forward(ctx, *ts):
        B, _, H, W = ts[0].shape
        out = new_nhwc(B, sum(t.shape[1] for t in ts), H, W, ts[0].dtype, ts[0].device)
        dt, st, off = N.dtype_code(out.dtype), stream(), 0
        for t in ts:
            c = t.shape[1]
            call('tss_copy_nhwc', ptr(t), ld(t), ptr(out[:, off:off + c]), ld(out), npix(t), c, dt, st)
            off += c
        ctx.widths = [t.shape[1] for t in ts]
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = to_nhwc(dout)
        grads, off = [], 0
        for c in ctx.widths:
            grads.append(dout[:, off:off + c])
            off += c
        return tuple(grads)


def concat_joined(branches, relu=True):
    """torch.cat([relu?(bn_i(branch_i)) for i], dim=1): every branch is a Deferred whose pending BatchNorm(+ReLU) is applied
    while it is written into its channel slice of the result -- one pass per branch, no normalised copy, no concat copy (the
    parallel branches of an ASPP module).  Backward hands each branch its masked gradient and BatchNorm-backward sums."""
    ds = [as_deferred(b).take() for b in branches]
    if any(d.raw.shape[1] % 8 or d.raw.shape[0] != ds[0].raw.shape[0] or d.raw.shape[2:] != ds[0].raw.shape[2:]
           or d.raw.dtype != ds[0].raw.dtype for d in ds):
        raise RuntimeError('concat_joined: branches must share batch / spatial size / dtype, channels multiples of 8')
    cfg = BranchCfg()
    cfg.links = [d.link for d in ds]
    cfg.relus = [bool(relu) or bool(d.relu) for d in ds]
    return ConcatJoinFn.apply(cfg, *[d.raw for d in ds])


class ConcatJoinFn(Function):
    @staticmethod
    def forward(ctx, cfg, *raws):
        B, _, H, W = raws[0].shape
        out = new_nhwc(B, sum(r.shape[1] for r in raws), H, W, raws[0].dtype, raws[0].device)
        dt, st, off = N.dtype_code(out.dtype), stream(), 0
        for r, link, relu in zip(raws, cfg.links, cfg.relus):
            c = r.shape[1]
            call('tss_join_fwd', ptr(r), ld(r), *_aff(link), None, 0, None, None, None, ptr(out[:, off:off + c]), ld(out),
                 int(relu), 0.0, None, npix(r), c, dt, st)
            off += c
        ctx.cfg = cfg
        ctx.save_for_backward(out, *raws)
        return out

    @staticmethod
    def backward(ctx, dout):
        out, *raws = ctx.saved_tensors
        cfg = ctx.cfg
        dout = to_nhwc(dout)
        dt, st, off, grads = N.dtype_code(dout.dtype), stream(), 0, []
        for r, link, relu in zip(raws, cfg.links, cfg.relus):
            c = r.shape[1]
            dsl, osl = dout[:, off:off + c], out[:, off:off + c]
            if relu or link is not None:
                e = new_nhwc(*r.shape, dout.dtype, dout.device) if relu else None
                call('tss_join_bwd', ptr(dsl), ld(dout), ptr(osl), ld(out), int(relu), ptr(r) if link is not None else None, ld(r),
                     ptr(link.mean) if link is not None else None, ptr(link.bstats) if link is not None else None,
                     None, 0, None, None, ptr(e), ld(e) if e is not None else 0, 1.0, npix(r), c, dt, st)
                grads.append(e if e is not None else dsl)
            else:
                grads.append(dsl)
            off += c
        return (None, *grads)


# ----------------------------------------------------------------------------- channel-attention gate (BiSeNet)

def gate(x, a, add_one=False):
    """x * (sigmoid(a) + add_one) with a = one value per image and channel ([B, C, 1, 1], the 1x1 convolution's output on the
    pooled map before the sigmoid): TSS/models/bisenet.py:128-131 (add_one) and :144-148."""
    x = to_nhwc(materialize(x))
    a = to_nhwc(materialize(a))
    if a.shape != (x.shape[0], x.shape[1], 1, 1) or a.dtype != x.dtype:
        raise RuntimeError('gate: attention must be (B, C, 1, 1) of the map\'s dtype, got %s %s for %s %s'
                           % (tuple(a.shape), a.dtype, tuple(x.shape), x.dtype))
    if x.shape[1] % 8:
        raise NotImplementedError('HIP path: gate needs a channel count that is a multiple of 8')
    return GateFn.apply(x, a, 1.0 if add_one else 0.0)


class GateFn(Function):
    @staticmethod
    def forward(ctx, x, a, add_one):
        B, C, H, W = x.shape
        out = new_nhwc(B, C, H, W, x.dtype, x.device)
        call('tss_gate_fwd', ptr(x), ld(x), ptr(a), ld(a), ptr(out), ld(out), B, H * W, C, add_one, N.dtype_code(x.dtype), stream())
        ctx.add_one = add_one
        ctx.save_for_backward(x, a)
        return out

    @staticmethod
    def backward(ctx, g):
        x, a = ctx.saved_tensors
        B, C, H, W = x.shape
        g = to_nhwc(g)
        dx = new_nhwc(B, C, H, W, x.dtype, x.device)
        da = new_nhwc(B, C, 1, 1, x.dtype, x.device)
        ws = torch.empty(B * N.lib().tss_gate_slices(B, H * W) * C, dtype=torch.float32, device=x.device)
        call('tss_gate_bwd', ptr(g), ld(g), ptr(x), ld(x), ptr(a), ld(a), ptr(dx), ld(dx), ptr(da), ld(da), ptr(ws), B, H * W, C,
             ctx.add_one, N.dtype_code(x.dtype), stream())
        return dx, da, None


# ----------------------------------------------------------------------------- pyramid pooling, all arms per launch

fuse_dropout = True    # nn.Dropout after a pending BatchNorm + ReLU rides in the join that materialises it (False: own pass)
# nn.Dropout in front of a 1x1 convolution is applied on load by that convolution (no join at all; TSS_DROP_CONV=0: the join form)
fuse_dropout_conv = os.environ.get('TSS_DROP_CONV', '1') != '0'
ppm_fused = os.environ.get('TSS_PPM_FUSED', '1') != '0'   # False: every arm through the generic operators (A/B checks)


# ----------------------------------------------------------------------------- LEDNet / ESNet glue (csrc/zoo.hip)

class _BNCfg:
    __slots__ = ('bn', 'training', 'link', 'params')


def batch_norm(z, bn, relu=False, gamma=None, beta=None):
    """BatchNorm2d (+ReLU) on a MATERIALISED tensor as a deferred unit: the statistics are computed now (one pass over z), the
    normalisation is applied by the consumer's load like after a convolution.  The nn.BatchNorm2d that follows
    torch.cat([conv(x), pool(x)]) in DownsamplingBlock (TSS/models/lednet.py:126-144, TSS/models/esnet.py:47-68)."""
    z = to_nhwc(materialize(z))
    if not isinstance(bn, _BatchNorm):
        raise TypeError('expected a BatchNorm module, got %r' % bn)
    if z.shape[1] % 8 or z.shape[1] != bn.num_features:
        raise NotImplementedError('HIP path: batch_norm needs %d channels, a multiple of 8; got %d' % (bn.num_features, z.shape[1]))
    cfg = _BNCfg()
    cfg.bn = bn
    cfg.training = bn.training or (bn.running_mean is None and bn.running_var is None)
    if cfg.training and bn.momentum is None:
        raise NotImplementedError('HIP path: BatchNorm with momentum=None (cumulative average) is not supported')
    if gamma is None:
        gamma, beta = bn.weight, bn.bias
    cfg.params = (gamma, beta)
    y = StandaloneBNFn.apply(z, _f32(gamma), _f32(beta), cfg)
    return Deferred(y, cfg.link, relu)


class StandaloneBNFn(Function):
    @staticmethod
    def forward(ctx, z, gamma, beta, cfg):
        C, P = z.shape[1], npix(z)
        if cfg.training and P <= 1:
            raise ValueError('Expected more than 1 value per channel when training, got input size %s' % (tuple(z.shape),))
        st = stream()
        link = BNLink(C, P, cfg.training, gamma, beta, z.device)
        if cfg.training:
            call('tss_tensor_stats', ptr(z), ld(z), P, C, ptr(link.stats), N.dtype_code(z.dtype), st)
        _finalize_forward(link, cfg.bn, cfg.training, P, C, gamma, st)
        cfg.link = link
        ctx.cfg = cfg
        ctx.has_affine = gamma is not None
        ctx.save_for_backward(z)
        return z.view_as(z)

    @staticmethod
    def backward(ctx, e):
        cfg = ctx.cfg
        z, = ctx.saved_tensors
        link = cfg.link
        e = to_nhwc(e)
        C, P = z.shape[1], npix(z)
        st = stream()
        dgamma, dbeta, zt, ga, gb, gce, gmu = _bn_backward_prologue(link, ctx.has_affine, cfg.params[0], cfg.params[1], C, z, z.device, st)
        dz = new_nhwc(*z.shape, e.dtype, z.device)
        call('tss_bn_bwd_apply', ptr(e), ld(e), ptr(zt), ld(z), ptr(ga), ptr(gb), ptr(gce), ptr(gmu), ptr(dz), ld(dz), P, C,
             N.dtype_code(e.dtype), st)
        return dz, dgamma, dbeta, None


def pool_concat(y1, bias, x, n1=None):
    """torch.cat([y1 + bias, F.max_pool2d(x, 2)], dim=1) in one pass (DownsamplingBlock, TSS/models/lednet.py:138-141 /
    TSS/models/esnet.py:62-65).  y1: the strided convolution's raw output (first n1 channels used; n1 < y1.shape[1] when the layer
    ran with zero-padded output rows), x: the block input -- an NHWC activation, or the NCHW image."""
    y1 = to_nhwc(materialize(y1))
    n1 = y1.shape[1] if n1 is None else n1
    is_image = x.dim() == 4 and x.shape[1] % 8 != 0
    if not is_image:
        x = to_nhwc(materialize(x))
    else:
        _check_device(x)
    B, Cin, Hin, Win = x.shape
    if Hin % 2 or Win % 2:
        raise NotImplementedError('HIP path: DownsamplingBlock needs even height and width (torch.cat of the reference fails otherwise)')
    if tuple(y1.shape) != (B, y1.shape[1], Hin // 2, Win // 2) or n1 > y1.shape[1]:
        raise RuntimeError('pool_concat: convolution output %s does not match the pooled input %s' % (tuple(y1.shape), tuple(x.shape)))
    if x.dtype != y1.dtype and x.dtype != torch.float32:
        raise TypeError('pool_concat: input dtype %s with activations of %s' % (x.dtype, y1.dtype))
    return PoolConcatFn.apply(y1, _f32(bias), x, n1)


class PoolConcatFn(Function):
    @staticmethod
    def forward(ctx, y1, bias, x, n1):
        B, Cin, Hin, Win = x.shape
        z = new_nhwc(B, n1 + Cin, Hin // 2, Win // 2, y1.dtype, y1.device)
        x_f32 = int(x.dtype == torch.float32)
        call('tss_pool_concat_fwd', ptr(y1), ld(y1), ptr(bias), n1, ptr(x), x_f32, *x.stride(), Cin, ptr(z), ld(z), B, Hin, Win,
             N.dtype_code(z.dtype), stream())
        ctx.n1, ctx.full1, ctx.has_bias = n1, y1.shape[1], bias is not None
        ctx.save_for_backward(x)
        return z

    @staticmethod
    def backward(ctx, dz):
        x, = ctx.saved_tensors
        dz = to_nhwc(dz)
        B, Cin, Hin, Win = x.shape
        n1, st, dt = ctx.n1, stream(), N.dtype_code(dz.dtype)
        dev = dz.device
        if ctx.full1 == n1:
            dy1 = dz[:, :n1]
        elif ctx.full1 == dz.shape[1]:
            dy1 = dz       # the layer ran with zero-padded output rows: their gradient is discarded by the padding's own backward
        else:
            dy1 = new_nhwc(B, ctx.full1, Hin // 2, Win // 2, dz.dtype, dev)
            dy1.zero_()
            dy1[:, :n1].copy_(dz[:, :n1])
        dbias = None
        if ctx.has_bias and ctx.needs_input_grad[1]:     # column sums through the slab rows: fixed order, no atomics
            dbias = _colsum(dz, n1, st)
        dx = None
        if ctx.needs_input_grad[2]:
            dx = new_nhwc(B, Cin, Hin, Win, dz.dtype, dev)
            call('tss_pool_concat_bwd', ptr(dz), ld(dz), n1, ptr(x), int(x.dtype == torch.float32), *x.stride(), Cin,
                 ptr(dx), ld(dx), B, Hin, Win, dt, st)
        return dy1, dbias, dx, None


def conv_transpose(x, weight, bias, stride, cout=None):
    """nn.ConvTranspose2d(k odd, stride, padding = (k - 1) / 2, output_padding = stride - 1, bias) on a materialised NHWC tensor
    (UpsamplingBlock, TSS/models/esnet.py:71-80): the transposed gather of the generic implicit-GEMM kernel.  `weight` is the layer's
    [Cin][Cout][kh][kw] tensor (Cout may be zero-padded by the caller to a multiple of 8)."""
    x = to_nhwc(materialize(x))
    if weight.shape[0] != x.shape[1] or x.shape[1] % 8 or weight.shape[1] % 8 or weight.shape[2] % 2 == 0 or weight.shape[3] % 2 == 0:
        raise NotImplementedError('HIP path: transposed convolution needs channel counts that are multiples of 8 and odd kernel sides; '
                                  'got weight %s for input %s' % (tuple(weight.shape), tuple(x.shape)))
    return ConvTransposeFn.apply(x, _f32(weight), _f32(bias), int(stride))


class ConvTransposeFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        B, Ci, H, W = x.shape
        Co, kh, kw = weight.shape[1], weight.shape[2], weight.shape[3]
        dev, st, dt = x.device, stream(), N.dtype_code(x.dtype)
        y = new_nhwc(B, Co, H * stride, W * stride, x.dtype, dev)
        w_tcn = torch.empty((kh * kw, Co, Ci), dtype=torch.float32, device=dev)
        call('tss_permute_wtaps', ptr(weight), None, ptr(w_tcn), Ci, Co, kh * kw, st)
        call('tss_convkxk_transposed_fwd', ptr(x), ld(x), ptr(w_tcn), ptr(bias), ptr(y), ld(y), B, H * stride, W * stride, Co, Ci,
             kh, kw, stride, dt, st)
        ctx.stride = stride
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = to_nhwc(g)
        B, Ci, H, W = x.shape
        Co, kh, kw = weight.shape[1], weight.shape[2], weight.shape[3]
        s = ctx.stride
        dev, st, dt = x.device, stream(), N.dtype_code(g.dtype)
        dx = dw = dbias = None
        if ctx.needs_input_grad[0]:        # the strided convolution of the gradient with the same weights
            w_tnc = torch.empty((kh * kw, Ci, Co), dtype=torch.float32, device=dev)
            call('tss_permute_wtaps', ptr(weight), ptr(w_tnc), None, Ci, Co, kh * kw, st)
            dx = new_nhwc(B, Ci, H, W, g.dtype, dev)
            call('tss_convkxk_fwd', ptr(g), ld(g), None, None, None, 0, ptr(w_tnc), None, ptr(dx), ld(dx), None,
                 B, H * s, W * s, Co, Ci, kh, kw, s, 1, dt, st)
        if ctx.needs_input_grad[1]:        # that convolution's weight gradient with the roles of activation and gradient swapped
            dw = torch.zeros_like(weight)
            rows = N.lib().tss_sconv_bwd_weight_rows(B, H * s, W * s, Co, Ci, dt) if (kh == 3 and kw == 3 and s == 2) else 0
            if rows:      # one sweep over x and g (csrc/sconv.hip, rectangular form), then the row reduction
                ws = torch.empty((rows, Ci * Co * 9), dtype=torch.float32, device=dev)
                call('tss_sconv_bwd_weight_sweep', ptr(x), ld(x), None, 0, None, None, None, None, ptr(g), ld(g), None, None, None, 0,
                     ptr(ws), B, H * s, W * s, Co, Ci, dt, st)
                _reduce_rows_now(ws, dw, Ci * Co * 9, rows)
            else:
                call('tss_convkxk_bwd_weight', ptr(x), ld(x), None, 0, None, None, None, None, ptr(g), ld(g), None, None, None, 0,
                     ptr(dw), B, H * s, W * s, Co, Ci, kh, kw, s, 1, dt, st)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            dbias = _colsum(g, Co, st)
        return dx, dw, dbias, None


def mul_addrows(u, a, r):
    """u * a + r with r one row per image ([B, C, 1, 1]): `x * level4(input) + level5(pooled)` of APNModule, TSS/models/lednet.py:86-90."""
    u, a, r = to_nhwc(materialize(u)), to_nhwc(materialize(a)), to_nhwc(materialize(r))
    if u.shape != a.shape or u.dtype != a.dtype or r.dtype != u.dtype or tuple(r.shape) != (u.shape[0], u.shape[1], 1, 1) or u.shape[1] % 8:
        raise RuntimeError('mul_addrows: operands %s, %s, %s' % (tuple(u.shape), tuple(a.shape), tuple(r.shape)))
    return MulAddRowsFn.apply(u, a, r)


class MulAddRowsFn(Function):
    @staticmethod
    def forward(ctx, u, a, r):
        B, C, H, W = u.shape
        out = new_nhwc(B, C, H, W, u.dtype, u.device)
        call('tss_mul_addrows_fwd', ptr(u), ld(u), ptr(a), ld(a), ptr(r), ld(r), ptr(out), ld(out), B, H * W, C,
             N.dtype_code(u.dtype), stream())
        ctx.save_for_backward(u, a)
        return out

    @staticmethod
    def backward(ctx, g):
        u, a = ctx.saved_tensors
        g = to_nhwc(g)
        B, C, H, W = u.shape
        dev = u.device
        du, da = new_nhwc(B, C, H, W, g.dtype, dev), new_nhwc(B, C, H, W, g.dtype, dev)
        dr = new_nhwc(B, C, 1, 1, g.dtype, dev)
        ws = torch.empty(B * N.lib().tss_rows_slices(B, H * W) * C, dtype=torch.float32, device=dev)
        call('tss_mul_addrows_bwd', ptr(g), ld(g), ptr(u), ld(u), ptr(a), ld(a), ptr(du), ld(du), ptr(da), ld(da), ptr(dr), ld(dr),
             ptr(ws), B, H * W, C, N.dtype_code(g.dtype), stream())
        return du, da, dr


def channel_dropout(x, p, training):
    """nn.Dropout2d (TSS/models/lednet.py:113, TSS/models/esnet.py:117,163): whole channels of an image are zeroed with probability
    p, the others scaled by 1 / (1 - p).  The mask is drawn with torch's generator (one [B, C] draw), applied by tss_scale_rows."""
    if not training or p <= 0.0:
        return x
    x = to_nhwc(materialize(x))
    if x.shape[1] % 8:
        raise NotImplementedError('HIP path: channel dropout needs a multiple of 8 channels')
    keep = 1.0 - float(p)
    m = (torch.rand((x.shape[0], x.shape[1]), device=x.device) < keep).to(torch.float32)
    if keep > 0.0:
        m = m / keep
    return ScaleRowsFn.apply(x, m)


class ScaleRowsFn(Function):
    @staticmethod
    def _run(x, m):
        B, C, H, W = x.shape
        out = new_nhwc(B, C, H, W, x.dtype, x.device)
        call('tss_scale_rows', ptr(x), ld(x), ptr(m), ptr(out), ld(out), B, H * W, C, N.dtype_code(x.dtype), stream())
        return out

    @staticmethod
    def forward(ctx, x, m):
        ctx.save_for_backward(m)
        return ScaleRowsFn._run(x, m)

    @staticmethod
    def backward(ctx, g):
        m, = ctx.saved_tensors
        return ScaleRowsFn._run(to_nhwc(g), m), None


def _hp(tensors):
    """Host array of device pointers (None -> NULL) for the tss_ppm_* entry points."""
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _hl(vals):
    import ctypes
    return (ctypes.c_long * len(vals))(*[int(v) for v in vals])


def _hi(vals):
    import ctypes
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def adaptive_avg_pool_multi(x, bins):
    """[AdaptiveAvgPool2d(b)(x) for b in bins] from one launch (and one launch for the summed gradient)."""
    x = to_nhwc(materialize(x))
    fork = _take(x, _FORK)      # x has another consumer (fork_two): its gradient is added in our backward
    return PoolMultiFn.apply(x, tuple(int(b) for b in bins), fork)


class PoolMultiFn(Function):
    @staticmethod
    def forward(ctx, x, bins, fork=None):
        ctx.fork = fork
        B, C, H, W = x.shape
        ys = [new_nhwc(B, C, b, b, x.dtype, x.device) for b in bins]
        ncells = sum(b * b for b in bins)
        S = N.lib().tss_ppm_pool_slices(B, ncells)
        ws = torch.empty(B * ncells * S * C, dtype=torch.float32, device=x.device) if S > 1 else None
        call('tss_ppm_pool_fwd', ptr(x), ld(x), _hp(ys), _hl([ld(y) for y in ys]), _hi(bins), len(bins), ptr(ws), B, H, W, C,
             N.dtype_code(x.dtype), stream())
        ctx.geom = (B, C, H, W, bins, x.dtype, x.device)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        B, C, H, W, bins, dtype, dev = ctx.geom
        dys = [to_nhwc(d) if d is not None else new_nhwc(B, C, b, b, dtype, dev).zero_() for d, b in zip(dys, bins)]
        dx = new_nhwc(B, C, H, W, dtype, dev)
        fork = ctx.fork
        radd = fork.g2 if fork is not None else None
        if radd is not None and not (radd.dtype == dtype and tuple(radd.shape) == (B, C, H, W) and is_nhwc(radd)):
            radd = None
        call('tss_ppm_pool_bwd', _hp(dys), _hl([ld(d) for d in dys]), _hi(bins), len(bins), ptr(dx), ld(dx),
             ptr(radd), ld(radd) if radd is not None else 0, B, H, W, C, N.dtype_code(dtype), stream())
        if radd is not None:
            fork.consumed = True
        return dx, None, None


def ppm_arms_fusable(x, arms):
    """concat_upsampled_arms covers these arms: <= 4 Deferred square maps of equal channel count, one slab row per cell."""
    if not ppm_fused or not 1 <= len(arms) <= 4 or not all(isinstance(a, Deferred) for a in arms):
        return False
    ca = arms[0].raw.shape[1]
    return all(a.raw.shape[1] == ca and a.raw.shape[2] == a.raw.shape[3] and a.raw.dtype == x.dtype
               and x.shape[0] * a.raw.shape[2] ** 2 <= N.stat_slabs() for a in arms) and ca % 8 == 0 and 256 % (ca // 8) == 0


def concat_upsampled_arms(x, arms):
    """torch.cat([x, *[upsample(relu(bn(arm))) for arm in arms]], 1): the pending BatchNorm + ReLU of every arm is applied
    per bilinear tap, all arms in one launch; backward hands every arm its masked gradient and BatchNorm-backward sums."""
    x = to_nhwc(materialize(x))
    ds = [a.take() for a in arms]
    cfg = BranchCfg()
    cfg.res_fork = _take(x, _STASH)
    cfg.links = [d.link for d in ds]
    cfg.relus = [bool(d.relu) for d in ds]
    return PpmConcatFn.apply(x, cfg, *[d.raw for d in ds])


class PpmConcatFn(Function):
    @staticmethod
    def _tables(cfg):
        links = cfg.links
        return (_hp([l.mean if l is not None else None for l in links]), _hp([l.scale if l is not None else None for l in links]),
                _hp([l.beta if l is not None else None for l in links]), _hi(cfg.relus))

    @staticmethod
    def forward(ctx, x, cfg, *raws):
        B, C, H, W = x.shape
        n, ca = len(raws), raws[0].shape[1]
        bins = [r.shape[2] for r in raws]
        out = new_nhwc(B, C + n * ca, H, W, x.dtype, x.device)
        call('tss_ppm_concat_fwd', ptr(x), ld(x), _hp(raws), _hl([ld(r) for r in raws]), _hi(bins), *PpmConcatFn._tables(cfg),
             n, ptr(out), ld(out), B, H, W, C, ca, N.dtype_code(x.dtype), stream())
        ctx.cfg, ctx.geom = cfg, (B, C, H, W, ca, bins)
        ctx.save_for_backward(*raws)
        return out

    @staticmethod
    def backward(ctx, dout):
        raws = ctx.saved_tensors
        B, C, H, W, ca, bins = ctx.geom
        dout = to_nhwc(dout)
        es = [new_nhwc(B, ca, b, b, dout.dtype, dout.device) for b in bins]
        call('tss_ppm_concat_bwd', ptr(dout), ld(dout), _hp(raws), _hl([ld(r) for r in raws]), _hi(bins),
             *PpmConcatFn._tables(ctx.cfg), _hp([l.bstats if l is not None else None for l in ctx.cfg.links]),   # (None: sums taken on chip by ppm_arms)
             _hp(es), _hl([ld(e) for e in es]), len(raws), B, H, W, C, ca, N.dtype_code(dout.dtype), stream())
        stash = ctx.cfg.res_fork
        if stash is not None:
            stash.g2 = dout[:, :C]         # x's other consumer (the pools) adds it in tss_ppm_pool_bwd (fork_two)
        return (dout[:, :C], None, *es)


# the arms themselves (1x1 convolution + BatchNorm statistics + finalize per arm): one launch for all of them, forward and backward
ppm_arms_fused = os.environ.get('TSS_PPM_ARMS', '1') != '0'    # '0': every arm through conv_unit (A/B checks)


def ppm_arms(blocks, pooled):
    """[block_i(pooled_i)] for the arms of a pyramid pooling module, each block = (Conv2d 1x1, BatchNorm2d[, ReLU]) -> list of
    Deferred (raw conv output + pending BatchNorm + ReLU), from ONE launch (csrc/ppm.hip); None when the arms are outside that
    kernel's envelope (the caller then runs them one by one)."""
    if not ppm_arms_fused or N.fast_paths_disabled() or not 1 <= len(blocks) <= 4:
        return None
    convs, bns, relus = [], [], []
    for blk in blocks:
        mods = list(blk)
        if len(mods) not in (2, 3) or not isinstance(mods[0], torch.nn.Conv2d) or not isinstance(mods[1], _BatchNorm):
            return None
        if len(mods) == 3 and not isinstance(mods[2], torch.nn.ReLU):
            return None
        c, bn = mods[0], mods[1]
        if (c.kernel_size != (1, 1) or c.groups != 1 or c.bias is not None or c.stride != (1, 1) or c.padding != (0, 0)
                or c.weight.dtype != torch.float32 or bn.weight is None or bn.weight.dtype != torch.float32
                or (bn.training and (bn.momentum is None or not bn.track_running_stats)) or _sync_group(bn) is not None
                or bn.running_mean is None or bn.running_mean.dtype != torch.float32
                or getattr(blk, 'act_dtype', None) not in (None, torch.bfloat16)):
            return None
        convs.append(c); bns.append(bn); relus.append(len(mods) == 3)
    ps = [p.raw if isinstance(p, Deferred) and p.link is None and not p.relu else p for p in pooled]
    if any(not torch.is_tensor(p) or p.dtype != torch.bfloat16 or not is_nhwc(p) for p in ps):
        return None
    C, Ca = convs[0].in_channels, convs[0].out_channels
    training = bns[0].training
    if any(c.in_channels != C or c.out_channels != Ca for c in convs) or any(p.shape[1] != C for p in ps) \
            or any(bn.training != training or bn.eps != bns[0].eps or bn.momentum != bns[0].momentum for bn in bns):
        return None
    counts = [npix(p) for p in ps]
    if training and min(counts) <= 1:
        return None                     # conv_unit raises torch's "Expected more than 1 value per channel"
    if not N.lib().tss_ppm_arms_supported(len(ps), C, Ca, _hi(counts), N.TSS_BF16):
        return None
    cfg = PpmArmsCfg()
    cfg.links = [None] * len(ps)
    cfg.convs, cfg.bns = convs, bns
    ys = PpmArmsFn.apply(cfg, *ps, *[c.weight for c in convs], *[bn.weight for bn in bns], *[bn.bias for bn in bns])
    return [Deferred(y, link, relu) for y, link, relu in zip(ys, cfg.links, relus)]


class PpmArmsFn(Function):
    @staticmethod
    def forward(ctx, cfg, *ts):
        convs, bns = cfg.convs, cfg.bns
        n = len(convs)
        ps, ws, gammas, betas = ts[:n], ts[n:2 * n], ts[2 * n:3 * n], ts[3 * n:4 * n]
        dev = ps[0].device
        C, Ca = convs[0].in_channels, convs[0].out_channels
        training = bns[0].training
        ys = [new_nhwc(p.shape[0], Ca, p.shape[2], p.shape[3], p.dtype, dev) for p in ps]
        counts = [npix(p) for p in ps]
        links = [BNLink(Ca, cnt, training, g_, b_, dev, slabs=False) for cnt, g_, b_ in zip(counts, gammas, betas)]
        run = [(bn.running_mean, bn.running_var, bn.num_batches_tracked) if training else (None, None, None) for bn in bns]
        call('tss_ppm_arms_fwd', _hp(ps), _hl([ld(p) for p in ps]), _hp(ws), _hp(gammas), _hp([r[0] for r in run]),
             _hp([r[1] for r in run]), _hp([r[2] for r in run]), _hp(ys), _hl([ld(y) for y in ys]), _hp([l.vec for l in links]),
             _hi(counts), n, C, Ca, int(training), float(bns[0].eps), float(bns[0].momentum if bns[0].momentum is not None else 0.0),
             N.TSS_BF16, stream())
        if not training:
            for bn, link, cnt, g_ in zip(bns, links, counts, gammas):
                _finalize_forward(link, bn, False, cnt, Ca, g_, stream())
        cfg.links = links
        ctx.cfg, ctx.n, ctx.geom = cfg, n, (C, Ca, counts, training)
        ctx.save_for_backward(*ps, *ws, *ys)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *es):
        n = ctx.n
        saved = ctx.saved_tensors
        ps, ws, ys = saved[:n], saved[n:2 * n], saved[2 * n:3 * n]
        convs, bns, links = ctx.cfg.convs, ctx.cfg.bns, ctx.cfg.links
        C, Ca, counts, training = ctx.geom
        dev = ps[0].device
        es = [to_nhwc(e) if e is not None else new_nhwc(*y.shape, y.dtype, dev).zero_() for e, y in zip(es, ys)]
        targets = [(_direct_target(c.weight), _direct_target(bn.weight), _direct_target(bn.bias)) for c, bn in zip(convs, bns)]
        direct = all(t is not None for tr in targets for t in tr)
        if not direct:
            targets = [(torch.empty_like(c.weight), torch.empty_like(bn.weight), torch.empty_like(bn.bias)) for c, bn in zip(convs, bns)]
        eins = [new_nhwc(p.shape[0], C, p.shape[2], p.shape[3], p.dtype, dev) for p in ps]
        call('tss_ppm_arms_bwd', _hp(es), _hl([ld(e) for e in es]), _hp(ys), _hl([ld(y) for y in ys]), _hp(ps), _hl([ld(p) for p in ps]),
             _hp(ws), _hp([l.gamma for l in links]), _hp([l.vec for l in links]), _hp([t[0] for t in targets]),
             _hp([t[1] for t in targets]), _hp([t[2] for t in targets]), int(direct), _hp(eins), _hl([ld(t) for t in eins]),
             _hi(counts), n, C, Ca, int(training), N.TSS_BF16, stream())
        if direct:
            return (None, *eins, *([None] * (3 * n)))
        return (None, *eins, *[t[0] for t in targets], *[t[1] for t in targets], *[t[2] for t in targets])


# ----------------------------------------------------------------------------- loss / metrics (caller side)

def _check_logits_target(logits, target):
    """The common opening of the losses on full-resolution logits: (B,C,H,W) logits and (B,H,W) int64 target, both contiguous."""
    _check_device(logits)
    logits = logits.contiguous()
    B, C, H, W = logits.shape
    if (H * W) % 8:
        raise NotImplementedError('HIP path: H*W must be a multiple of 8')
    if target.dtype != torch.int64 or target.shape != (B, H, W):
        raise RuntimeError('target must be int64 of shape (B,H,W)')
    return logits, target.contiguous()


def _ignore_pair(ignore_index):
    """(ignore value, has_ignore) as the entry points take them; ignore_index=None: no label is ignored."""
    return (int(ignore_index), 1) if ignore_index is not None else (0, 0)


def _open_backward(logits, gout):
    """The common opening of the loss backwards: grad_out as contiguous float32, the uninitialised dlogits, (B, C, H*W)."""
    B, C, H, W = logits.shape
    return gout.to(torch.float32).contiguous(), torch.empty_like(logits), (B, C, H * W)


def _check_variant(variant, variants):
    if variant not in variants:
        raise ValueError('variant must be %s, got %r' % (' or '.join(repr(v) for v in variants), variant))


def _check_num_classes(input, num_classes):
    if input.dim() != 4 or int(num_classes) != input.shape[1]:
        raise ValueError('num_classes (%s) must equal the channel count of the (B,C,H,W) logits %s'
                         % (num_classes, tuple(input.shape)))


class CrossEntropyFn(Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        logits, target = _check_logits_target(logits, target)
        B, C, H, W = logits.shape
        dev = logits.device
        lse = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        acc = torch.zeros(2, dtype=torch.float64, device=dev)
        scal = torch.empty(2, dtype=torch.float32, device=dev)
        call('tss_cross_entropy_fwd', ptr(logits), ptr(target), ptr(lse), ptr(acc), ptr(scal[0:1]), ptr(scal[1:2]),
             B, C, H * W, int(ignore_index), N.dtype_code(logits.dtype), stream())
        ctx.ignore_index = int(ignore_index)
        ctx.save_for_backward(logits, target, lse, scal)
        return scal[0].clone()

    @staticmethod
    def backward(ctx, gout):
        logits, target, lse, scal = ctx.saved_tensors
        gout, d, dims = _open_backward(logits, gout)
        call('tss_cross_entropy_bwd', ptr(logits), ptr(target), ptr(lse), ptr(scal[1:2]), ptr(gout), ptr(d),
             *dims, ctx.ignore_index, N.dtype_code(logits.dtype), stream())
        return d, None, None


def _check_smoothing(label_smoothing):
    eps = float(label_smoothing)
    if not 0.0 <= eps <= 1.0:
        raise ValueError('label_smoothing must be in [0, 1], got %r' % (label_smoothing,))
    return eps


def _class_weight(weight, num_classes, dev=None):
    """The class weights as the kernels read them: contiguous float32 of shape (C,); None stays None (all ones).  Weights that
    already have that form are returned as they are, so an in-place update of the caller's tensor reaches a captured step."""
    if weight is None:
        return None
    if not torch.is_tensor(weight) or not weight.is_floating_point():
        raise ValueError('weight must be a floating-point tensor')
    if weight.dim() != 1 or (num_classes is not None and weight.shape[0] != num_classes):
        raise ValueError('weight must have shape (C,) = (%s,), got %s' % (num_classes, tuple(weight.shape)))
    if dev is not None and weight.device != dev:
        raise ValueError('weight lives on %s but the logits on %s' % (weight.device, dev))
    if weight.dtype != torch.float32 or not weight.is_contiguous():
        weight = weight.detach().to(torch.float32).contiguous()
    return weight.detach()


class WeightedCrossEntropyFn(Function):
    """cross_entropy with class weights and / or label smoothing (tss_cross_entropy_{fwd,bwd}_ex): per-block partial rows summed in
    a fixed order, no atomics, so two evaluations give the same bits.  The weights are constants: no gradient flows to them."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, weight, eps):
        logits, target = _check_logits_target(logits, target)
        B, C, H, W = logits.shape
        dev = logits.device
        lse = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        rows = torch.empty((max(N.lib().tss_cross_entropy_ex_rows(B, H * W), 1), 2), dtype=torch.float64, device=dev)
        scal = torch.empty(2, dtype=torch.float32, device=dev)
        call('tss_cross_entropy_fwd_ex', ptr(logits), ptr(target), ptr(weight), eps, ptr(lse), ptr(rows), ptr(scal[0:1]), ptr(scal[1:2]),
             B, C, H * W, int(ignore_index), N.dtype_code(logits.dtype), stream())
        ctx.ignore_index, ctx.eps = int(ignore_index), eps
        ctx.has_weight = weight is not None
        ctx.save_for_backward(logits, target, lse, scal, *([weight] if weight is not None else []))
        return scal[0].clone()

    @staticmethod
    def backward(ctx, gout):
        logits, target, lse, scal = ctx.saved_tensors[:4]
        weight = ctx.saved_tensors[4] if ctx.has_weight else None
        gout, d, dims = _open_backward(logits, gout)
        call('tss_cross_entropy_bwd_ex', ptr(logits), ptr(target), ptr(weight), ctx.eps, ptr(lse), ptr(scal[1:2]), ptr(gout), ptr(d),
             *dims, ctx.ignore_index, N.dtype_code(logits.dtype), stream())
        return d, None, None, None, None


def cross_entropy(logits, target, ignore_index=-100, weight=None, label_smoothing=0.0):
    """F.cross_entropy(logits, target, weight=..., ignore_index=..., reduction='mean', label_smoothing=...) for (B,C,H,W) logits.
    weight: floating (C,) tensor on the logits' device or None; the mean is over the sum of the valid pixels' weights, as in torch."""
    eps = _check_smoothing(label_smoothing)
    if weight is None and eps == 0.0:
        return CrossEntropyFn.apply(logits, target, ignore_index)
    weight = _class_weight(weight, logits.shape[1] if logits.dim() == 4 else None, logits.device)
    return WeightedCrossEntropyFn.apply(logits, target, ignore_index, weight, eps)


class CrossEntropyLoss(torch.nn.Module):
    """Drop-in for nn.CrossEntropyLoss(ignore_index=...) as scripts/train_fastscnn.py:132 builds it, and for
    nn.CrossEntropyLoss(ignore_index=255, weight=...) of scripts/contextnet/train_contextnet.py:123-125.  `weight` is a registered
    buffer (contiguous float32 (C,), or None): .cuda() / .to() move it, and the kernels read it from device memory, so an in-place
    update between replays of a captured step takes effect without a re-capture."""

    def __init__(self, ignore_index=-100, weight=None, label_smoothing=0.0):
        super().__init__()
        self.ignore_index = ignore_index
        self.label_smoothing = _check_smoothing(label_smoothing)
        weight = _class_weight(weight, None)
        self.register_buffer('weight', None if weight is None else weight.clone())
        self.sample_group = self.sample_weight = self.group_loss_out = None
        self.pixel_weight, self.pixel_norm = None, 'weight'

    def set_sample_groups(self, group, weight=None, group_loss_out=None):
        """Per-sample loss groups for every following call (upsample_cross_entropy's sample_group / sample_weight / group_loss_out):
        each group is normalised over its own valid pixels and the loss is the sum of the groups' terms.  The module holds DEVICE
        tensors (int32 [B], float32 [B]) that the kernels read, so an in-place update between replays of a captured step takes
        effect without a re-capture; host sequences are validated and copied to the current device here.  The rows are plain
        attributes, not buffers: they belong to a batch layout, not to the state dict."""
        on_dev = torch.is_tensor(group) and group.is_cuda
        batch = int(group.shape[0]) if on_dev else len(group)
        host = [t is not None and not (torch.is_tensor(t) and t.is_cuda) for t in (group, weight)]
        if host[0] or host[1]:
            check_sample_groups(group if host[0] else list(range(batch)), weight if host[1] else None, batch)
        dev = group.device if on_dev else (weight.device if torch.is_tensor(weight) and weight.is_cuda
                                           else torch.device('cuda', torch.cuda.current_device()))
        self.sample_group, self.sample_weight = _sample_rows(group, weight, batch, dev)
        self.group_loss_out = group_loss_out

    def clear_sample_groups(self):
        self.sample_group = self.sample_weight = self.group_loss_out = None

    def set_pixel_weight(self, pixel_weight, norm='weight'):
        """A per-pixel weight map for every following call (upsample_pixel_weighted_cross_entropy's pixel_weight / pixel_norm): a contiguous
        float32
        [B,H,W] DEVICE tensor that the kernels read, so an in-place update between replays of a captured step takes effect without
        a re-capture.  A plain attribute like the sample rows, not a buffer; label smoothing must be 0."""
        if norm not in PIXEL_NORMS:
            raise ValueError("norm must be 'weight', 'valid' or 'pixels', got %r" % (norm,))
        if self.label_smoothing > 0.0:
            raise ValueError('label smoothing together with a per-pixel weight map is not supported')
        if not (torch.is_tensor(pixel_weight) and pixel_weight.is_cuda and pixel_weight.dtype == torch.float32 and pixel_weight.dim() == 3
                and pixel_weight.is_contiguous()):
            raise ValueError('pixel_weight must be a contiguous float32 [B,H,W] tensor on the device')
        self.pixel_weight, self.pixel_norm = pixel_weight.detach(), norm

    def clear_pixel_weight(self):
        self.pixel_weight, self.pixel_norm = None, 'weight'

    def forward(self, input, target):
        if self.pixel_weight is not None:      # the map exists on the fused head: the same operator at the logits' own size
            return upsample_pixel_weighted_cross_entropy(input, target, self.pixel_weight, size=tuple(input.shape[2:]),
                                                         ignore_index=self.ignore_index, weight=self.weight,
                                                         label_smoothing=self.label_smoothing, pixel_norm=self.pixel_norm,
                                                         sample_group=self.sample_group, sample_weight=self.sample_weight,
                                                         group_loss_out=self.group_loss_out)
        if self.sample_group is not None:      # groups exist on the fused head: the same operator at the logits' own size
            return upsample_cross_entropy(input, target, size=tuple(input.shape[2:]), ignore_index=self.ignore_index, weight=self.weight,
                                          label_smoothing=self.label_smoothing, sample_group=self.sample_group,
                                          sample_weight=self.sample_weight, group_loss_out=self.group_loss_out)
        return cross_entropy(input, target, self.ignore_index, self.weight, self.label_smoothing)


def label_histogram(target, num_classes, ignore_index=255, out=None):
    """Number of labels per class in an int64 label tensor of any shape, on the device: int64 [num_classes].  Labels equal to
    ignore_index (None: no ignore index) or outside [0, num_classes) are not counted.  With `out` (int64 [num_classes] on the
    target's device) the counts are ADDED to it, so a loop over a dataset accumulates; integer arithmetic only, exact.
    No bincount over a masked copy, no host sync."""
    _check_device(target)
    C = int(num_classes)
    if target.dtype != torch.int64:
        raise RuntimeError('target must be int64')
    if not 0 < C <= N.lib().tss_label_histogram_max_classes():
        raise NotImplementedError('HIP path: label_histogram supports 1..%d classes, got %d' % (N.lib().tss_label_histogram_max_classes(), C))
    if out is None:
        out = torch.zeros(C, dtype=torch.int64, device=target.device)
    elif out.dtype != torch.int64 or out.shape != (C,) or out.device != target.device or not out.is_contiguous():
        raise RuntimeError('out must be a contiguous int64 tensor of shape (%d,) on %s' % (C, target.device))
    target = target.contiguous()
    has_ignore = ignore_index is not None
    call('tss_label_histogram', ptr(target), ptr(out), target.numel(), C, int(ignore_index) if has_ignore else 0, int(has_ignore), 0, stream())
    return out


def enet_class_weights(counts_or_freq, c=1.02):
    """The ENet / ERFNet class balancing 1 / log(c + frequency) (Paszke et al. 2016), the recipe of
    scripts/contextnet/train_contextnet.py:123-124: float32 weights on the input's device.  An integer tensor is taken as
    counts (label_histogram's output) and normalized to frequencies first; a floating one is taken as frequencies."""
    freq = counts_or_freq
    if not freq.is_floating_point():
        freq = freq.to(torch.float64)
        freq = freq / freq.sum()
    return (1.0 / torch.log(c + freq)).to(torch.float32)


AUGMENT_MAX_SIZE = 8192      # source and scaled sizes for which every index of tss_augment_batch_u8 fits in int32


def _float3(values, fill):
    """HOST array of 3 floats for the mean3 / std3 arguments of the wire-format entries (None -> NULL)."""
    if values is None:
        return None
    return (ctypes.c_float * 3)(*([float(v) for v in values] + [fill] * 3)[:3])


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def check_augment_params(params, source_size, crop_size):
    """Raise ValueError unless every (Hs, Ws, oy, ox, flip, 0) row of the CPU tensor `params` keeps its crop inside its scaled
    image: crop <= scaled size <= 8192 and 0 <= origin <= scaled size - crop.  The kernel does not validate the rows."""
    (H, W), (ch, cw) = _pair(source_size), _pair(crop_size)
    if params.dtype != torch.int32 or params.dim() != 2 or params.shape[1] != 6:
        raise ValueError('augmentation parameters must be int32 [B, 6], got %s %s' % (params.dtype, tuple(params.shape)))
    Hs, Ws, oy, ox, flip, _ = params.long().unbind(1)
    ok = ((Hs >= ch) & (Hs <= AUGMENT_MAX_SIZE) & (Ws >= cw) & (Ws <= AUGMENT_MAX_SIZE) & (oy >= 0) & (oy <= Hs - ch)
          & (ox >= 0) & (ox <= Ws - cw) & ((flip == 0) | (flip == 1)))
    if not bool(ok.all()):
        raise ValueError('augmentation parameter row %d = %s does not keep a %dx%d crop inside its scaled image'
                         % (int((~ok).nonzero()[0]), params[int((~ok).nonzero()[0])].tolist(), ch, cw))


def check_color_params(color):
    """Raise ValueError unless the CPU tensor `color` holds int32 [B, 4] rows (apply, dh, ds, dv) with apply in {0, 1}, |dh| <= 180
    (the kernel wraps the hue once) and |ds|, |dv| <= 255.  The kernel does not validate the rows."""
    if color.dtype != torch.int32 or color.dim() != 2 or color.shape[1] != 4:
        raise ValueError('colour rows must be int32 [B, 4], got %s %s' % (color.dtype, tuple(color.shape)))
    apply, dh, ds, dv = color.long().unbind(1)
    ok = ((apply == 0) | (apply == 1)) & (dh.abs() <= 180) & (ds.abs() <= 255) & (dv.abs() <= 255)
    if not bool(ok.all()):
        raise ValueError('colour row %d = %s: need apply in {0, 1}, |dh| <= 180, |ds| <= 255, |dv| <= 255'
                         % (int((~ok).nonzero()[0]), color[int((~ok).nonzero()[0])].tolist()))


def label_lut(label_map, device=None):
    """The 256-byte table of augment_batch / remap_labels as a uint8 tensor (on `device` if given): `label_map` is a sequence or
    tensor of 256 integers in 0..255, entry i = the train id of raw label i.  A uint8 tensor already on the device is returned
    as it is, so build the table once and pass it on."""
    t = label_map if torch.is_tensor(label_map) else torch.as_tensor(list(label_map))
    if t.dim() != 1 or t.numel() != 256 or t.is_floating_point() or t.is_complex():
        raise ValueError('label_map must hold 256 integers, got %s %s' % (t.dtype, tuple(t.shape)))
    if t.dtype != torch.uint8:
        if bool(((t < 0) | (t > 255)).any()):
            raise ValueError('label_map entries must lie in 0..255')
        t = t.to(torch.uint8)
    return t.contiguous() if device is None else t.to(device).contiguous()


class TrainAugment:
    """The reference's train-time augmentation (scripts/train_fastscnn.py:62-68), drawn on the host and applied on the device:

        albu.RandomScale -> albu.RandomCrop(crop_size) -> albu.HorizontalFlip(p=flip_p) -> albu.Normalize(mean, std) -> ToTensor()

    crop_size = (height, width), width a multiple of 8.  `scale_range` is the range of the MULTIPLICATIVE factor itself
    (albumentations versions differ on whether a `scale_limit` tuple gets 1 added: pass the factors you mean, (0.5, 2.0) for
    the recipe).  `mean` / `std` are the Normalize constants (None: 0 / 1, i.e. x / 255).

    draw() produces one int32 row (Hs, Ws, oy, ox, flip, 0) per sample on the CPU: s uniform in scale_range,
    Hs = max(crop height, floor(H s + 0.5)), Ws likewise, the crop origin uniform over the positions that keep the crop inside
    the scaled image, flip Bernoulli(flip_p).  augment_batch / tss_augment_batch_u8 apply the rows: bilinear (half-pixel centres,
    clamped edges, as cv2.INTER_LINEAR) for the image, nearest (as cv2.INTER_NEAREST) for the labels.  The image is blended in
    float32 from the four uint8 texels and NOT rounded back to uint8 before Normalize as cv2 does: at most half a grey level
    away from the reference's pixel, on purpose (one rounding fewer, and no quantisation noise added to the input).

    The reference's RandomCrop raises when the scaled image is smaller than the crop; check_source() / draw() (and
    engine.HostBatchPipeline at construction) raise ValueError when scale_range[0] makes that possible for the source size.

    hsv_p > 0 adds the other recipe's colour step (scripts/contextnet/train_contextnet.py: ... HorizontalFlip ->
    albu.HueSaturationValue(p=hsv_p) -> Normalize ...; the limits default to albumentations'): draw_color() produces one int32 row
    (apply, dh, ds, dv) per sample, and the kernel shifts the blended float32 (r, g, b) of a sample with apply = 1 in HSV, on
    cv2's 8-bit scale (H in [0, 180), S and V in [0, 255]) kept CONTINUOUS: neither H, S, V nor the RGB result is rounded to
    uint8 as cv2 does (include/tss_hip.h, tss_augment_batch_u8_ex, has the formulas).  A grey pixel has hue 0, so ds > 0 tints it
    red, as in the reference.  `label_map` (256 integers in 0..255, e.g. the dataset's TRAIN_MAPPING; none ships with the
    package) sends the raw label byte through a table on the device, so the loader ships the label PNG as decoded."""

    def __init__(self, crop_size, scale_range=(0.5, 2.0), flip_p=0.5, mean=None, std=None, hsv_p=0.0, hue_shift_limit=20,
                 sat_shift_limit=30, val_shift_limit=20, label_map=None):
        self.crop_size = _pair(crop_size)
        self.scale_range = (float(scale_range[0]), float(scale_range[1]))
        self.flip_p = float(flip_p)
        self.mean = None if mean is None else tuple(float(v) for v in mean)
        self.std = None if std is None else tuple(float(v) for v in std)
        ch, cw = self.crop_size
        if ch < 1 or cw < 8 or cw % 8 or max(ch, cw) > AUGMENT_MAX_SIZE:
            raise ValueError('crop_size must be (height >= 1, width a multiple of 8), at most %d: got %s' % (AUGMENT_MAX_SIZE, (ch, cw)))
        if not 0.0 < self.scale_range[0] <= self.scale_range[1]:
            raise ValueError('scale_range must be 0 < low <= high, got %s' % (self.scale_range,))
        if not 0.0 <= self.flip_p <= 1.0:
            raise ValueError('flip_p must be a probability, got %r' % flip_p)
        self.hsv_p = float(hsv_p)
        self.shift_limits = (int(hue_shift_limit), int(sat_shift_limit), int(val_shift_limit))
        self.label_map = None if label_map is None else label_lut(label_map).cpu()
        if not 0.0 <= self.hsv_p <= 1.0:
            raise ValueError('hsv_p must be a probability, got %r' % hsv_p)
        if not (0 <= self.shift_limits[0] <= 180 and 0 <= self.shift_limits[1] <= 255 and 0 <= self.shift_limits[2] <= 255):
            raise ValueError('shift limits must be 0 <= hue <= 180, 0 <= sat <= 255, 0 <= val <= 255, got %s' % (self.shift_limits,))

    @staticmethod
    def _scaled(n, s):
        return int(math.floor(n * s + 0.5))

    def check_source(self, source_size):
        """ValueError when some scale of the range gives a scaled image smaller than the crop or larger than 8192."""
        H, W = _pair(source_size)
        ch, cw = self.crop_size
        lo, hi = self.scale_range
        if not (1 <= H <= AUGMENT_MAX_SIZE and 1 <= W <= AUGMENT_MAX_SIZE):
            raise ValueError('source size %s outside 1..%d' % ((H, W), AUGMENT_MAX_SIZE))
        if self._scaled(H, lo) < ch or self._scaled(W, lo) < cw:
            raise ValueError('scale_range[0] = %g shrinks a %dx%d source to %dx%d, smaller than the %dx%d crop (RandomCrop would raise)'
                             % (lo, H, W, self._scaled(H, lo), self._scaled(W, lo), ch, cw))
        if self._scaled(H, hi) > AUGMENT_MAX_SIZE or self._scaled(W, hi) > AUGMENT_MAX_SIZE:
            raise ValueError('scale_range[1] = %g grows a %dx%d source past %d' % (hi, H, W, AUGMENT_MAX_SIZE))

    def draw(self, B, source_size, generator=None):
        """int32 [B, 6] rows (Hs, Ws, oy, ox, flip, 0) on the CPU; deterministic for a given torch.Generator state."""
        self.check_source(source_size)
        H, W = _pair(source_size)
        ch, cw = self.crop_size
        lo, hi = self.scale_range
        u = torch.rand((int(B), 4), generator=generator, dtype=torch.float64)
        s = lo + (hi - lo) * u[:, 0]
        Hs = torch.floor(H * s + 0.5).long().clamp_(min=ch)
        Ws = torch.floor(W * s + 0.5).long().clamp_(min=cw)
        oy = torch.minimum(torch.floor(u[:, 1] * (Hs - ch + 1)).long(), Hs - ch)      # uniform integers in [0, Hs - ch]
        ox = torch.minimum(torch.floor(u[:, 2] * (Ws - cw + 1)).long(), Ws - cw)
        flip = (u[:, 3] < self.flip_p).long()
        rows = torch.stack([Hs, Ws, oy, ox, flip, torch.zeros_like(flip)], 1).to(torch.int32)
        check_augment_params(rows, (H, W), (ch, cw))
        return rows

    def draw_color(self, B, generator=None):
        """int32 [B, 4] rows (apply, dh, ds, dv) on the CPU: apply Bernoulli(hsv_p), every shift a uniform integer in
        [-limit, limit], drawn whether or not the row applies; deterministic for a given torch.Generator state.  Call it after
        draw(): the pipeline draws the geometry rows of a batch first, then its colour rows, from one generator."""
        u = torch.rand((int(B), 4), generator=generator, dtype=torch.float64)
        cols = [(u[:, 0] < self.hsv_p).long()]
        for k, lim in enumerate(self.shift_limits):
            cols.append(torch.floor(u[:, k + 1] * (2 * lim + 1)).long().clamp_(max=2 * lim) - lim)
        rows = torch.stack(cols, 1).to(torch.int32)
        check_color_params(rows)
        return rows


def augment_batch(image_u8, target_u8, params, crop_size, mean=None, std=None, image_hwc=False, out=None, color=None, label_map=None):
    """Scale + crop + flip + Normalize + ToTensor of a uint8 batch on the device (tss_augment_batch_u8; semantics: TrainAugment).

    image_u8 [B, H, W, C] (image_hwc=True) or [B, C, H, W], C <= 3; target_u8 [B, H, W]; either may be None.  params: int32
    [B, 6] rows (Hs, Ws, oy, ox, flip, 0) as TrainAugment.draw returns them -- a CPU tensor is validated and copied to the
    device, a device tensor is used as it is (not validated: no host sync).  Returns (float32 [B, C, ch, cw], int64 [B, ch, cw]);
    with out=(image_out, target_out) the results are written there.

    color: int32 [B, 4] rows (apply, dh, ds, dv) as TrainAugment.draw_color returns them (CPU: validated and copied; device:
    used as it is): HueSaturationValue between the blend and Normalize, C == 3 only.  label_map: 256 integers in 0..255 (see
    label_lut; a uint8 device tensor is used as it is), applied to the label bytes.  With either, the call goes to
    tss_augment_batch_u8_ex; with both None it is the plain entry, as before."""
    first = image_u8 if image_u8 is not None else target_u8
    if first is None:
        raise ValueError('augment_batch needs an image or a target')
    _check_device(first)
    ch, cw = _pair(crop_size)
    dev = first.device
    B = first.shape[0]
    C, size = 1, None
    if image_u8 is not None:
        if image_u8.dtype != torch.uint8 or image_u8.dim() != 4 or not image_u8.is_contiguous():
            raise ValueError('image must be a contiguous uint8 [B, H, W, C] or [B, C, H, W] tensor')
        (H, W, C) = image_u8.shape[1:] if image_hwc else (image_u8.shape[2], image_u8.shape[3], image_u8.shape[1])
        size = (H, W)
    if target_u8 is not None:
        _check_device(target_u8)
        if target_u8.dtype != torch.uint8 or target_u8.dim() != 3 or not target_u8.is_contiguous() or target_u8.shape[0] != B:
            raise ValueError('target must be a contiguous uint8 [B, H, W] tensor')
        if size is not None and tuple(target_u8.shape[1:]) != size:
            raise ValueError('image is %dx%d but target is %s' % (size[0], size[1], tuple(target_u8.shape[1:])))
        size = tuple(target_u8.shape[1:])
    H, W = size
    if not 1 <= C <= 3:
        raise ValueError('HIP path: augment_batch supports 1..3 channels, got %d' % C)
    if cw % 8 or cw < 8 or ch < 1 or max(H, W, ch, cw) > AUGMENT_MAX_SIZE:
        raise ValueError('crop width must be a multiple of 8 and every size at most %d: source %dx%d, crop %dx%d'
                         % (AUGMENT_MAX_SIZE, H, W, ch, cw))
    if tuple(params.shape) != (B, 6) or params.dtype != torch.int32:
        raise ValueError('params must be int32 [%d, 6], got %s %s' % (B, params.dtype, tuple(params.shape)))
    if not params.is_cuda:
        check_augment_params(params, (H, W), (ch, cw))
        params = params.to(dev)
    params = params.contiguous()
    if color is not None:
        if C != 3 or image_u8 is None:
            raise ValueError('color needs a 3-channel image (hue is defined on r, g, b), got %s' % ('no image' if image_u8 is None else 'C = %d' % C))
        if tuple(color.shape) != (B, 4) or color.dtype != torch.int32:
            raise ValueError('color must be int32 [%d, 4], got %s %s' % (B, color.dtype, tuple(color.shape)))
        if not color.is_cuda:
            check_color_params(color)
            color = color.to(dev)
        color = color.contiguous()
    lut = None if label_map is None else label_lut(label_map, dev)
    ox, oy = out if out is not None else (None, None)
    if image_u8 is not None:
        if ox is None:
            ox = torch.empty((B, C, ch, cw), dtype=torch.float32, device=dev)
        elif ox.dtype != torch.float32 or tuple(ox.shape) != (B, C, ch, cw) or not ox.is_contiguous() or ox.device != dev or ox.data_ptr() % 16:
            raise ValueError('out[0] must be a contiguous, 16-byte aligned float32 %s tensor on %s' % ((B, C, ch, cw), dev))
    if target_u8 is not None:
        if oy is None:
            oy = torch.empty((B, ch, cw), dtype=torch.int64, device=dev)
        elif oy.dtype != torch.int64 or tuple(oy.shape) != (B, ch, cw) or not oy.is_contiguous() or oy.device != dev or oy.data_ptr() % 16:
            raise ValueError('out[1] must be a contiguous, 16-byte aligned int64 %s tensor on %s' % ((B, ch, cw), dev))
    head = (ptr(image_u8), int(bool(image_hwc)), _float3(mean, 0.0), _float3(std, 1.0), ptr(ox) if image_u8 is not None else None,
            ptr(target_u8), ptr(oy) if target_u8 is not None else None, ptr(params))
    if color is None and lut is None:
        call('tss_augment_batch_u8', *head, B, C, H, W, ch, cw, stream())
    else:
        call('tss_augment_batch_u8_ex', *head, ptr(color), ptr(lut), B, C, H, W, ch, cw, stream())
    return (ox if image_u8 is not None else None), (oy if target_u8 is not None else None)


def remap_labels(target_u8, label_map, out=None):
    """int64 [B, H, W] = label_map[target_u8] on the device (tss_remap_labels_u8): the dataset's raw-id -> train-id table for the
    evaluation path, where no augmentation launch carries it.  target_u8: contiguous uint8 tensor (any shape; the result has its
    shape); label_map as in augment_batch; out: a contiguous int64 tensor of that shape to write into."""
    _check_device(target_u8)
    if target_u8.dtype != torch.uint8 or not target_u8.is_contiguous() or target_u8.data_ptr() % 8:
        raise ValueError('target must be a contiguous, 8-byte aligned uint8 tensor')
    lut = label_lut(label_map, target_u8.device)
    if out is None:
        out = torch.empty(target_u8.shape, dtype=torch.int64, device=target_u8.device)
    elif (out.dtype != torch.int64 or out.shape != target_u8.shape or not out.is_contiguous() or out.device != target_u8.device
          or out.data_ptr() % 16):
        raise ValueError('out must be a contiguous, 16-byte aligned int64 %s tensor on %s' % (tuple(target_u8.shape), target_u8.device))
    call('tss_remap_labels_u8', ptr(target_u8), ptr(lut), ptr(out), target_u8.numel(), stream())
    return out


class OHEMFn(Function):
    """ohem_loss (TSS/losses/ohem_loss.py:10-21): per-pixel CE, the (n+1)-th largest found by a device-side radix select."""
    _ws = {}

    @staticmethod
    def workspace(dev):          # zeroed once; every call leaves it zeroed
        return _per_device(OHEMFn._ws, dev, lambda: torch.zeros(N.lib().tss_ohem_workspace_bytes(), dtype=torch.uint8, device=dev))

    @staticmethod
    def forward(ctx, logits, target, ignore_index, thresh_loss, numel_frac):
        logits, target = _check_logits_target(logits, target)
        B, C, H, W = logits.shape
        dev = logits.device
        lse = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        pix = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        out = torch.empty(5, dtype=torch.float32, device=dev)              # loss, then the 4 selection parameters
        n_top = int(B * H * W * float(numel_frac))
        call('tss_ohem_fwd', ptr(logits), ptr(target), ptr(lse), ptr(pix), ptr(OHEMFn.workspace(dev)), ptr(out[0:1]),
             ptr(out[1:5]), B, C, H * W, int(ignore_index), float(thresh_loss), n_top, N.dtype_code(logits.dtype),
             stream())
        ctx.ignore_index = int(ignore_index)
        ctx.save_for_backward(logits, target, lse, pix, out)
        return out[0].clone()

    @staticmethod
    def backward(ctx, gout):
        logits, target, lse, pix, out = ctx.saved_tensors
        gout, d, dims = _open_backward(logits, gout)
        call('tss_ohem_bwd', ptr(logits), ptr(target), ptr(lse), ptr(pix), ptr(out[1:5]), ptr(gout), ptr(d),
             *dims, ctx.ignore_index, N.dtype_code(logits.dtype), stream())
        return d, None, None, None, None


def ohem_loss(input, target, ignore_index=-100, thresh_loss=0.35667494393873245, numel_frac=0.01):
    """TSS/losses/ohem_loss.py:10-21 (thresh_loss default = -log(0.7))."""
    return OHEMFn.apply(input, target, ignore_index, thresh_loss, numel_frac)


class OHEMLoss(torch.nn.Module):
    """Drop-in for TSS.losses.OHEMLoss (TSS/losses/ohem_loss.py:24-37), the loss of scripts/train_fastscnn.py."""

    def __init__(self, ignore_index=-100, thresh_loss=0.35667494393873245, numel_frac=0.01):
        super().__init__()
        self.ignore_index, self.thresh_loss, self.numel_frac = ignore_index, thresh_loss, numel_frac

    def forward(self, input, target):
        return ohem_loss(input, target, self.ignore_index, self.thresh_loss, self.numel_frac)


LOVASZ_VARIANTS = {'reference': 0, 'berman': 1}
lovasz_chunk_classes = 0     # classes sorted at a time; 0: as many as fit in 2 GiB of sort buffers (csrc/lovasz.hip)


class LovaszSoftmaxFn(Function):
    """lovasz_softmax_loss (TSS/losses/lovasz_softmax_loss.py:20-45): a segmented stable radix sort of the per-class errors,
    a scan of the foreground flags and closed-form Lovasz weights, all on the device (csrc/lovasz.hip); no argsort, no
    host read-back, graph-capturable and bit-reproducible."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, variant):
        logits, target = _check_logits_target(logits, target)
        B, C, H, W = logits.shape
        if B * H * W >= 2 ** 31:
            raise NotImplementedError('HIP path: lovasz_softmax_loss needs B*H*W < 2**31')
        dev = logits.device
        code = N.dtype_code(logits.dtype)
        # g_rank per class and pixel (read by backward) + the bounded sort buffers; the caching allocator returns
        # 512-byte aligned blocks, and inside a graph capture the block comes from the graph's own pool
        chunk = int(lovasz_chunk_classes)
        ws = torch.empty(N.lib().tss_lovasz_workspace_bytes(B * H * W, C, chunk), dtype=torch.uint8, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)              # loss, number of present classes
        call('tss_lovasz_fwd', ptr(logits), ptr(target), ptr(ws), ptr(out[0:1]), ptr(out[1:2]), B, C, H * W,
             *_ignore_pair(ignore_index), LOVASZ_VARIANTS[variant], chunk, code, stream())
        ctx.chunk = chunk
        ctx.save_for_backward(logits, target, ws, out)
        return out[0].clone()

    @staticmethod
    def backward(ctx, gout):
        logits, target, ws, out = ctx.saved_tensors
        gout, d, dims = _open_backward(logits, gout)
        call('tss_lovasz_bwd', ptr(logits), ptr(target), ptr(ws), ptr(out[1:2]), ptr(gout), ptr(d), *dims,
             ctx.chunk, N.dtype_code(logits.dtype), stream())
        return d, None, None, None


def lovasz_softmax_loss(input, target, num_classes, ignore_index=None, variant='reference'):
    """TSS/losses/lovasz_softmax_loss.py:20-45 for (B,C,H,W) logits and an int64 (B,H,W) target.

    variant='reference' weights rank r >= 1 with J_r - J_0, which is what the reference's lovasz_grad (:15-16) computes
    (value and gradient are a drop-in for it; the value grows with the number of pixels); variant='berman' uses the
    published successive difference J_r - J_{r-1} (Berman et al. 2018), a loss in [0, 1].  Pixels with target ==
    ignore_index are dropped (None keeps all); other labels outside [0, C) are background for every class, as upstream.

    Two documented differences from the reference: equal errors are ordered by ascending flat pixel index (torch.argsort
    leaves ties unspecified), which keeps the step bit-reproducible; and when no class is present (e.g. every pixel
    ignored) the loss is 0.0 with a zero gradient, without a host read-back, where the reference raises from
    torch.stack([])."""
    _check_variant(variant, LOVASZ_VARIANTS)
    _check_num_classes(input, num_classes)
    return LovaszSoftmaxFn.apply(input, target, ignore_index, variant)


class LovaszSoftmaxLoss(torch.nn.Module):
    """Drop-in for TSS.losses.LovaszSoftmaxLoss (TSS/losses/lovasz_softmax_loss.py:48-59); see lovasz_softmax_loss."""

    def __init__(self, num_classes, ignore_index=-100, variant='reference'):
        super().__init__()
        _check_variant(variant, LOVASZ_VARIANTS)
        self.num_classes, self.ignore_index, self.variant = num_classes, ignore_index, variant

    def forward(self, input, target):
        return lovasz_softmax_loss(input, target, self.num_classes, self.ignore_index, self.variant)


FOCAL_VARIANTS = {'reference': 0, 'lin': 1}
softloss_max_blocks = 0      # block cap of the focal / Dice kernels; 0: their default (csrc/softloss.hip)


class FocalFn(Function):
    """focal_loss (TSS/losses/focal_loss.py:8-15) on csrc/softloss.hip: one sweep over the class planes per direction, per-block
    partial rows and a fixed-order finalize (no atomics, no host read-back): graph-capturable and bit-reproducible."""

    @staticmethod
    def forward(ctx, logits, target, alpha, gamma, ignore_index, variant):
        logits, target = _check_logits_target(logits, target)
        B, C, H, W = logits.shape
        dev = logits.device
        cap = int(softloss_max_blocks)
        lse = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        coef = torch.empty((B, H, W), dtype=torch.float32, device=dev)     # per-pixel gradient coefficient, 0 outside the valid set
        ws = torch.empty(N.lib().tss_focal_workspace_bytes(B, H * W, cap), dtype=torch.uint8, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)              # loss, alpha / number of valid pixels
        call('tss_focal_fwd', ptr(logits), ptr(target), ptr(lse), ptr(coef), ptr(ws), ptr(out[0:1]), ptr(out[1:2]), B, C, H * W,
             *_ignore_pair(ignore_index), float(alpha), float(gamma), FOCAL_VARIANTS[variant], cap, N.dtype_code(logits.dtype), stream())
        ctx.cap = cap
        ctx.save_for_backward(logits, target, lse, coef, out)
        return out[0].clone()

    @staticmethod
    def backward(ctx, gout):
        logits, target, lse, coef, out = ctx.saved_tensors
        gout, d, dims = _open_backward(logits, gout)
        call('tss_focal_bwd', ptr(logits), ptr(target), ptr(lse), ptr(coef), ptr(out[1:2]), ptr(gout), ptr(d), *dims,
             ctx.cap, N.dtype_code(logits.dtype), stream())
        return d, None, None, None, None, None


def focal_loss(input, target, alpha=0.25, gamma=2.0, ignore_index=-100, variant='reference'):
    """TSS/losses/focal_loss.py:8-15 for (B,C,H,W) logits and an int64 (B,H,W) target: -alpha * mean over the valid pixels of
    w * log p_t, with q = 1 - p_t evaluated as the sum of the other classes' probabilities.

    variant='reference' weights a pixel with w = exp(q^gamma), which is what the reference computes (torch.exp(factor) *
    log_softmax; value and gradient are a drop-in for it); variant='lin' uses the published w = q^gamma (Lin et al. 2017).
    A pixel is valid iff target != ignore_index and 0 <= target < C (the rule of cross_entropy here).

    Two documented differences from the reference: ignore_index=None keeps every in-range pixel, where the reference
    raises a TypeError from nll_loss; and with no valid pixel the loss is 0.0 with a zero gradient, without a host
    read-back, where the reference returns nan."""
    _check_variant(variant, FOCAL_VARIANTS)
    if not float(gamma) >= 0.0:
        raise ValueError('gamma must be >= 0, got %r' % (gamma,))
    return FocalFn.apply(input, target, alpha, gamma, ignore_index, variant)


class FocalLoss(torch.nn.Module):
    """Drop-in for TSS.losses.FocalLoss (TSS/losses/focal_loss.py:18-32), constructor defaults included; the default
    ignore_index=None keeps every in-range pixel (the reference raises there).  See focal_loss.
    fused_head=True lets engine.Trainer take upsample_focal_loss on the model's low-resolution logits; the module itself, called on
    full-resolution logits, computes the same either way."""

    def __init__(self, alpha=0.25, gamma=2.0, ignore_index=None, variant='reference', fused_head=False):
        super().__init__()
        _check_variant(variant, FOCAL_VARIANTS)
        self.alpha, self.gamma, self.ignore_index, self.variant = alpha, gamma, ignore_index, variant
        self.fused_head = bool(fused_head)

    def forward(self, input, target):
        return focal_loss(input, target, self.alpha, self.gamma, self.ignore_index, self.variant)


DICE_MAX_CLASSES = 256


class DiceFn(Function):
    """dice_loss (TSS/losses/dice_loss.py:8-26) on csrc/softloss.hip: per-class sums in registers, per-block partial rows and a
    fixed-order finalize that also leaves the 2C backward coefficients (no atomics, no one_hot, no boolean-mask indexing, no
    host read-back): graph-capturable and bit-reproducible."""

    @staticmethod
    def forward(ctx, logits, target, smooth, ignore_index):
        logits, target = _check_logits_target(logits, target)
        B, C, H, W = logits.shape
        if C > DICE_MAX_CLASSES:
            raise NotImplementedError('HIP path: dice_loss supports at most %d classes, got %d' % (DICE_MAX_CLASSES, C))
        dev = logits.device
        cap = int(softloss_max_blocks)
        lse = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        ws = torch.empty(N.lib().tss_dice_workspace_bytes(B, C, H * W, cap), dtype=torch.uint8, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ign = _ignore_pair(ignore_index)
        call('tss_dice_fwd', ptr(logits), ptr(target), ptr(lse), ptr(ws), ptr(loss), B, C, H * W, *ign, float(smooth), cap,
             N.dtype_code(logits.dtype), stream())
        ctx.cap, ctx.ign = cap, ign
        ctx.save_for_backward(logits, target, lse, ws)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, gout):
        logits, target, lse, ws = ctx.saved_tensors
        gout, d, dims = _open_backward(logits, gout)
        call('tss_dice_bwd', ptr(logits), ptr(target), ptr(lse), ptr(ws), ptr(gout), ptr(d), *dims, *ctx.ign,
             ctx.cap, N.dtype_code(logits.dtype), stream())
        return d, None, None, None


def dice_loss(input, target, num_classes, smooth=1.0, ignore_index=-100):
    """The soft Dice loss TSS/losses/dice_loss.py:8-26 intends, for (B,C,H,W) logits and an int64 (B,H,W) target: over the
    valid pixels, I_c = sum p_c [t == c], U_c = sum p_c + sum [t == c], loss = mean over all num_classes classes (an absent
    class counts) of 1 - (2 I_c + smooth) / (U_c + smooth).

    The reference itself raises on every call (the chained `&` of its mask line, :15), so there is no reference number;
    its evident intent is built.  Reading taken of that line: `target > 0` is read as the range check `target >= 0`, so
    a pixel is valid iff target != ignore_index and 0 <= target < num_classes, the rule of every loss here
    (ignore_index=None: every in-range pixel).  With no valid pixel the loss is 0.0 with a zero gradient (also for
    smooth=0), without a host read-back.  num_classes must equal the channel count, at most 256."""
    _check_num_classes(input, num_classes)
    if not float(smooth) >= 0.0:
        raise ValueError('smooth must be >= 0, got %r' % (smooth,))
    return DiceFn.apply(input, target, smooth, ignore_index)


class DiceLoss(torch.nn.Module):
    """Drop-in for TSS.losses.DiceLoss (TSS/losses/dice_loss.py:29-42), which cannot run upstream; see dice_loss.
    fused_head=True lets engine.Trainer take upsample_dice_loss on the model's low-resolution logits; the module itself, called on
    full-resolution logits, computes the same either way."""

    def __init__(self, num_classes, smooth=1.0, ignore_index=-100, fused_head=False):
        super().__init__()
        self.num_classes, self.smooth, self.ignore_index = num_classes, smooth, ignore_index
        self.fused_head = bool(fused_head)

    def forward(self, input, target):
        return dice_loss(input, target, self.num_classes, self.smooth, self.ignore_index)


DISTILL_KINDS = {'pixel': 0, 'channel': 1}
DISTILL_MAX_CLASSES = 256
distill_max_blocks = 0       # block cap of the distillation kernels; 0: their default (csrc/distill.hip)


def _check_distill(temperature, kind):
    if kind not in DISTILL_KINDS:
        raise ValueError("kind must be 'pixel' or 'channel', got %r" % (kind,))
    if not float(temperature) > 0.0:
        raise ValueError('temperature must be > 0, got %r' % (temperature,))


class DistillFn(Function):
    """distillation_loss on csrc/distill.hip, student and teacher as NHWC low-resolution logits of one dtype: the forward (two
    launches for the pixel kind, three for the channel kind) leaves the loss and four floats per pixel / per plane, the backward is
    one elementwise sweep from them.  Per-block partial rows and a fixed-order finalize (no atomics, no host read-back):
    graph-capturable and bit-reproducible.  The teacher gets no gradient."""

    @staticmethod
    def forward(ctx, student, teacher, temperature, kind):
        B, C, h, w = student.shape
        dev = student.device
        cap, code, tau = int(distill_max_blocks), N.dtype_code(student.dtype), float(temperature)
        units = B * h * w if kind == 'pixel' else B * C
        stats = torch.empty((units, 4), dtype=torch.float32, device=dev)
        ws = torch.empty(N.lib().tss_distill_workspace_bytes(DISTILL_KINDS[kind], B, C, h * w, cap), dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        call('tss_distill_%s_fwd' % kind, ptr(student), ld(student), ptr(teacher), ld(teacher), ptr(stats), ptr(ws), ptr(loss),
             B, C, h * w, tau, cap, code, stream())
        ctx.args = (kind, B, C, h, w, tau, cap, code)
        ctx.save_for_backward(student, teacher, stats)
        return loss

    @staticmethod
    def backward(ctx, gout):
        student, teacher, stats = ctx.saved_tensors
        kind, B, C, h, w, tau, cap, code = ctx.args
        gout = gout.to(torch.float32).contiguous()
        ldd = ld(student)
        base = torch.empty((B, h, w, ldd), dtype=student.dtype, device=student.device)   # pad channels are written as zeros
        call('tss_distill_%s_bwd' % kind, ptr(student), ldd, ptr(teacher), ld(teacher), ptr(stats), ptr(gout), ptr(base), ldd,
             B, C, h * w, tau, cap, code, stream())
        return base.permute(0, 3, 1, 2)[:, :C], None, None, None


def distillation_loss(student, teacher, temperature=1.0, kind='pixel'):
    """Logit distillation of (B,C,h,w) student logits against teacher logits of the same shape and dtype (float32 or bfloat16),
    at the resolution of the logits (for the models here: the 1/8-resolution map of forward_lowres).  With x = logits /
    temperature, p = softmax(x_teacher) and q = softmax(x_student):

    kind='pixel'   (Hinton et al.): softmax over the classes of a pixel, loss = T^2 / (B h w) * sum over pixels of KL(p || q),
                   which is F.kl_div(F.log_softmax(s / T, 1), F.softmax(t / T, 1), reduction='sum') * T^2 / (B h w);
    kind='channel' (Shu et al., ICCV 2021): softmax over the h w positions of a (sample, class) plane,
                   loss = T^2 / (B C) * sum over planes of KL(p || q).

    Every pixel counts (no target, no ignore mask).  The teacher is a constant: it receives no gradient, whatever its
    requires_grad.  NHWC tensors (what forward_lowres returns) are read in place; a contiguous NCHW tensor is copied to NHWC first
    (boundary plumbing).  Returns a 0-dim float32 device tensor.  At most 256 classes."""
    _check_distill(temperature, kind)
    student, teacher = materialize(student), materialize(teacher)
    if student.dim() != 4 or tuple(student.shape) != tuple(teacher.shape):
        raise ValueError('student and teacher logits must have one (B,C,h,w) shape, got %s and %s'
                         % (tuple(student.shape), tuple(teacher.shape)))
    if student.shape[1] > DISTILL_MAX_CLASSES:
        raise ValueError('HIP path: distillation_loss supports at most %d classes, got %d' % (DISTILL_MAX_CLASSES, student.shape[1]))
    if min(student.shape) < 1:
        raise ValueError('student and teacher logits must not be empty, got %s' % (tuple(student.shape),))
    if student.dtype != teacher.dtype:
        raise TypeError('student and teacher logits must share one dtype, got %s and %s' % (student.dtype, teacher.dtype))
    N.dtype_code(student.dtype)               # TypeError for anything but float32 / bfloat16
    _check_device(student)
    _check_device(teacher)
    return DistillFn.apply(to_nhwc(student), to_nhwc(teacher.detach()), temperature, kind)


class TwoConsumersFn(Function):
    """x -> (x, x) for low-resolution logits that two losses read (the head loss and the distillation term).  Both hand back an NHWC
    gradient whose pad channels are zeros; the backward adds them over the whole padded rows (one ATen add), so the sum is again
    an NHWC tensor with zero pads, the layout the classifier's backward gets from the head loss alone.  Autograd's own add would
    return a dense C-channel tensor, and its NHWC copy has uninitialised pad channels."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None or gb is None:
            return gb if ga is None else ga
        B, C, h, w = ga.shape
        pitch = ld(ga)

        def whole_rows(g):      # an NHWC view whose storage holds every row up to the pitch
            return is_nhwc(g) and ld(g) == pitch and (g.storage_offset() + B * h * w * pitch) * g.element_size() <= g.untyped_storage().nbytes()

        if ga.dtype == gb.dtype and whole_rows(ga) and whole_rows(gb):
            size, stride = (B, h, w, pitch), (h * w * pitch, w * pitch, pitch, 1)
            return (torch.as_strided(ga, size, stride) + torch.as_strided(gb, size, stride)).permute(0, 3, 1, 2)[:, :C]
        return ga + gb


def two_consumers(x):
    return TwoConsumersFn.apply(x)


class DistillationLoss(torch.nn.Module):
    """forward(student, teacher) = distillation_loss(student, teacher, temperature, kind); engine.Trainer(teacher=...,
    distill_loss=DistillationLoss(...)) adds it to the head loss on the low-resolution logits."""

    def __init__(self, temperature=1.0, kind='pixel'):
        super().__init__()
        _check_distill(temperature, kind)
        self.temperature, self.kind = temperature, kind

    def forward(self, student, teacher):
        return distillation_loss(student, teacher, self.temperature, self.kind)


HEAD_REGISTER_CLASSES = 24        # the fused head's kernels that keep every class of a pixel in registers (csrc/loss.hip, msflip.hip)
WIDEHEAD_MAX_CLASSES = 256        # their class-chunked counterparts (csrc/widehead.hip, tss_widehead_max_classes())


def _wide(C):
    """The suffix of the fused head's entry points for C classes: '' up to 24 (the register kernels), '_wide' up to 256."""
    return '_wide' if C > HEAD_REGISTER_CLASSES else ''


class UpsampleCrossEntropyFn(Function):
    """cross_entropy(F.interpolate(low, scale, bilinear, align_corners=True), target) without the full-res logits:
    one pass yields the loss and the unscaled low-res gradient (per-block tiles in a workspace, no atomics, nothing to
    zero-fill), backward gathers the tiles in a fixed order and scales by grad_out / #valid: bit-identical from run to run.
    More than 24 classes: the class-chunked entries (tss_upsample_ce_wide_*), same workspace convention, same returns."""

    @staticmethod
    def forward(ctx, low, target, ho, wo, ignore_index, weight=None, eps=0.0):
        B, C, h, w = low.shape
        dev = low.device
        target = target.contiguous()
        nws = getattr(N.lib(), 'tss_upsample_ce%s_ws' % _wide(C))(B, C, h, w, ho, wo)
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)        # written by the kernel: no copy launch for the return value
        inv = torch.empty(1, dtype=torch.float32, device=dev)
        if _wide(C):    # one entry for the plain, the weighted and the smoothed loss
            call('tss_upsample_ce_wide_fwd', ptr(low), ld(low), ptr(target), ptr(weight), eps, ptr(ws), ptr(loss),
                 ptr(inv), B, C, h, w, ho, wo, int(ignore_index), N.dtype_code(low.dtype), stream())
        elif weight is None and eps == 0.0:
            call('tss_upsample_ce_fwd', ptr(low), ld(low), ptr(target), ptr(ws), ptr(loss),
                 ptr(inv), B, C, h, w, ho, wo, int(ignore_index), N.dtype_code(low.dtype), stream())
        else:       # class weights / label smoothing: other instances of the same pass, same workspace, same gather
            call('tss_upsample_ce_fwd_ex', ptr(low), ld(low), ptr(target), ptr(weight), eps, ptr(ws), ptr(loss),
                 ptr(inv), B, C, h, w, ho, wo, int(ignore_index), N.dtype_code(low.dtype), stream())
        ctx.geom = (B, C, h, w, ho, wo, ld(low), low.dtype)
        ctx.save_for_backward(ws, inv)
        return loss

    @staticmethod
    def backward(ctx, gout):
        ws, inv = ctx.saved_tensors
        B, C, h, w, ho, wo, ldl, dtype = ctx.geom
        gout = gout.to(torch.float32).contiguous()
        base = torch.empty((B, h, w, ldl), dtype=dtype, device=ws.device)   # pad channels are written as zeros
        call('tss_upsample_ce%s_bwd' % _wide(C), ptr(ws), ptr(inv), ptr(gout), ptr(base), ldl, B, C, h, w, ho, wo,
             N.dtype_code(dtype), stream())
        return base.permute(0, 3, 1, 2)[:, :C], None, None, None, None, None, None


GROUP_MAX_BATCH = 1024       # tss_upsample_ce_group_max_batch(): the samples whose sums the grouped finalize keeps on chip
STRONGAUG_TILE = (32, 32)    # tss_strong_augment_tile(): (TH, TW), the output tile of one block of csrc/strongaug.hip


def check_sample_groups(group, weight, batch):
    """Host-side validation of per-sample loss groups, before anything touches the device: `group` a sequence of `batch` integers
    in [0, batch), `weight` None or a sequence of `batch` finite, non-negative numbers.  Returns them as (int32 array, float32 array
    or None); ValueError otherwise."""
    import numpy as np
    g = group.numpy() if torch.is_tensor(group) else np.asarray(group)
    if g.ndim != 1 or g.shape[0] != batch:
        raise ValueError('sample_group must have length B = %d, got shape %s' % (batch, tuple(g.shape)))
    if g.dtype.kind not in 'iu':
        raise ValueError('sample_group must hold integers, got %s' % g.dtype)
    if g.size and (int(g.min()) < 0 or int(g.max()) >= batch):
        raise ValueError('sample_group ids must lie in [0, %d), got [%d, %d]' % (batch, int(g.min()), int(g.max())))
    if weight is None:
        return g.astype(np.int32), None
    w = weight.numpy() if torch.is_tensor(weight) else np.asarray(weight)
    if w.dtype.kind not in 'fiu':
        raise ValueError('sample_weight must hold numbers, got %s' % w.dtype)
    w = w.astype(np.float64)
    if w.ndim != 1 or w.shape[0] != batch:
        raise ValueError('sample_weight must have length B = %d, got shape %s' % (batch, tuple(w.shape)))
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError('sample_weight must be finite and non-negative, got %s' % (w.tolist(),))
    return g.astype(np.int32), w.astype(np.float32)


def _sample_rows(group, weight, batch, dev):
    """The rows of a grouped loss as the kernels read them (int32 [B], float32 [B] or None).  Device tensors are taken as they are
    (dtype, shape and contiguity checked, values not: the kernel gives an id outside [0, B) the weight 0), so an in-place update
    reaches a captured step; host sequences are validated (check_sample_groups) and copied."""
    on_dev = [torch.is_tensor(t) and t.is_cuda for t in (group, weight)]
    host = check_sample_groups(list(range(batch)) if on_dev[0] else group, None if on_dev[1] else weight, batch)
    rows = []
    for t, is_dev, h, dtype, name in ((group, on_dev[0], host[0], torch.int32, 'sample_group'),
                                      (weight, on_dev[1], host[1], torch.float32, 'sample_weight')):
        if t is None:
            rows.append(None)
        elif is_dev:
            if t.dtype != dtype or tuple(t.shape) != (batch,) or not t.is_contiguous() or t.device != dev:
                raise ValueError('%s on the device must be a contiguous %s tensor of shape (%d,) on %s' % (name, dtype, batch, dev))
            rows.append(t.detach())
        else:
            rows.append(torch.from_numpy(h).to(dev))
    return rows


class UpsampleGroupedCrossEntropyFn(Function):
    """upsample_cross_entropy with per-sample loss groups: sum over the groups g of (sum_{b in g} lambda_b CE_sum(b)) / N_g, every
    group normalised over its own valid pixels (their class weights).  The forward entry of UpsampleCrossEntropyFn runs as it is
    (its own loss and 1 / count go to two scratch words); tss_upsample_ce_group_finalize turns its loss rows into the loss, the
    per-group terms and one gradient scale per sample, and backward is the gather that reads its scale per sample.  f64 sums in a
    fixed order, no atomics, no host read-back: the same bits on every run, capturable.  An empty group contributes 0 and a zero
    gradient (the rule of focal_loss / dice_loss, not the nan of the ungrouped mean)."""

    @staticmethod
    def forward(ctx, low, target, ho, wo, ignore_index, weight, eps, rows):
        group, sweight, group_loss = rows
        B, C, h, w = low.shape
        dev = low.device
        target = target.contiguous()
        nws = getattr(N.lib(), 'tss_upsample_ce%s_ws' % _wide(C))(B, C, h, w, ho, wo)
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        scratch = torch.empty(2, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        scale = torch.empty(B, dtype=torch.float32, device=dev)
        head = (B, C, h, w, ho, wo, int(ignore_index), N.dtype_code(low.dtype), stream())
        if _wide(C):
            call('tss_upsample_ce_wide_fwd', ptr(low), ld(low), ptr(target), ptr(weight), eps, ptr(ws), ptr(scratch[0:1]),
                 ptr(scratch[1:2]), *head)
        elif weight is None and eps == 0.0:
            call('tss_upsample_ce_fwd', ptr(low), ld(low), ptr(target), ptr(ws), ptr(scratch[0:1]), ptr(scratch[1:2]), *head)
        else:
            call('tss_upsample_ce_fwd_ex', ptr(low), ld(low), ptr(target), ptr(weight), eps, ptr(ws), ptr(scratch[0:1]),
                 ptr(scratch[1:2]), *head)
        call('tss_upsample_ce_group_finalize', ptr(ws), B, C, h, w, ho, wo, 1 if _wide(C) else 0, ptr(group), ptr(sweight), ptr(loss),
             ptr(scale), ptr(group_loss), stream())
        ctx.geom = (B, C, h, w, ho, wo, ld(low), low.dtype)
        ctx.save_for_backward(ws, scale)
        return loss

    @staticmethod
    def backward(ctx, gout):
        ws, scale = ctx.saved_tensors
        B, C, h, w, ho, wo, ldl, dtype = ctx.geom
        gout = gout.to(torch.float32).contiguous()
        base = torch.empty((B, h, w, ldl), dtype=dtype, device=ws.device)   # pad channels are written as zeros
        call('tss_upsample_ce%s_bwd_rows' % _wide(C), ptr(ws), ptr(scale), ptr(gout), ptr(base), ldl, B, C, h, w, ho, wo,
             N.dtype_code(dtype), stream())
        return base.permute(0, 3, 1, 2)[:, :C], None, None, None, None, None, None, None


def _upsample_grouped_cross_entropy(low, target, scale_factor, size, ignore_index, weight, eps, sample_group, sample_weight,
                                    group_loss_out):
    B = low.shape[0]
    if not 1 <= B <= GROUP_MAX_BATCH:
        raise ValueError('sample groups take a batch of 1 to %d samples, got %d' % (GROUP_MAX_BATCH, B))
    host = [t is not None and not (torch.is_tensor(t) and t.is_cuda) for t in (sample_group, sample_weight)]
    if host[0] or host[1]:      # host sequences: refused here, before the first device access
        check_sample_groups(sample_group if host[0] else list(range(B)), sample_weight if host[1] else None, B)
    ho, wo = _out_size(low, size, scale_factor)
    if low.shape[1] > WIDEHEAD_MAX_CLASSES or ho < low.shape[2] or wo < low.shape[3]:
        raise ValueError('sample groups exist on the fused head only (at most %d classes, an output no smaller than the map): got %d '
                         'classes, %dx%d -> %dx%d' % (WIDEHEAD_MAX_CLASSES, low.shape[1], low.shape[2], low.shape[3], ho, wo))
    low = to_nhwc(materialize(low))
    _check_head_target(low, target, ho, wo)
    dev = low.device
    group, sweight = _sample_rows(sample_group, sample_weight, B, dev)
    if group_loss_out is None:
        group_loss_out = torch.empty(B, dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(group_loss_out) and group_loss_out.dtype == torch.float32 and tuple(group_loss_out.shape) == (B,)
              and group_loss_out.is_contiguous() and group_loss_out.device == dev):
        raise ValueError('group_loss_out must be a contiguous float32 tensor of shape (%d,) on %s' % (B, dev))
    return UpsampleGroupedCrossEntropyFn.apply(low, target, ho, wo, ignore_index, _class_weight(weight, low.shape[1], dev), eps,
                                               (group, sweight, group_loss_out))


PIXEL_NORMS = {'weight': 0, 'valid': 1, 'pixels': 2}      # the `norm` argument of csrc/pixwce.hip's entries


def check_pixel_weight(pixel_weight, shape, dev, pixel_norm='weight'):
    """Host-side validation of a per-pixel weight map: a contiguous float32 tensor of `shape` = (B, H, W) on the logits' device `dev`
    (a host tensor is refused: the map is too large to copy silently), and a known pixel_norm.  ValueError otherwise."""
    if pixel_norm not in PIXEL_NORMS:
        raise ValueError("pixel_norm must be 'weight', 'valid' or 'pixels', got %r" % (pixel_norm,))
    if not torch.is_tensor(pixel_weight):
        raise ValueError('pixel_weight must be a tensor, got %s' % type(pixel_weight).__name__)
    if (pixel_weight.dtype != torch.float32 or tuple(pixel_weight.shape) != tuple(shape) or not pixel_weight.is_contiguous()
            or pixel_weight.device != torch.device(dev)):
        raise ValueError('pixel_weight must be a contiguous float32 tensor of shape %s on %s, got %s %s on %s'
                         % (tuple(shape), dev, pixel_weight.dtype, tuple(pixel_weight.shape), pixel_weight.device))


class UpsamplePixelWeightedCrossEntropyFn(Function):
    """upsample_pixel_weighted_cross_entropy: a per-pixel weight map omega (csrc/pixwce.hip): loss = sum_valid k ce / D, k = omega w_t, D by
    `norm`.  Up to 24 classes one pass leaves the rows (sum k ce, D-part) and the unscaled gradient tiles; up to 256 the wide head's
    per-pixel cross-entropy is turned in place into k by tss_upsample_ce_pixw_coef_wide, which also writes the rows, and
    tss_upsample_coef_grad_wide fills the tiles.  Both always finish through tss_upsample_ce_group_finalize (without sample groups:
    one group of weight 1) and the per-sample gather, so D = 0 gives 0.0 and an exactly zero gradient.  No atomics, no host
    read-back: the same bits on every run, capturable; omega is read from device memory by every replay."""

    @staticmethod
    def forward(ctx, low, target, ho, wo, ignore_index, weight, pixw, norm, rows):
        group, sweight, group_loss = rows
        B, C, h, w = low.shape
        dev = low.device
        target = target.contiguous()
        code = N.dtype_code(low.dtype)
        ws = torch.empty(getattr(N.lib(), 'tss_upsample_ce%s_ws' % _wide(C))(B, C, h, w, ho, wo), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        scale = torch.empty(B, dtype=torch.float32, device=dev)
        if _wide(C):
            pix = torch.empty((B, ho, wo), dtype=torch.float32, device=dev)
            call('tss_upsample_pixel_ce_wide', ptr(low), ld(low), ptr(target), ptr(pix), B, C, h, w, ho, wo, int(ignore_index), code, stream())
            call('tss_upsample_ce_pixw_coef_wide', ptr(pix), ptr(target), ptr(pixw), ptr(weight), norm, ptr(ws), B, C, ho, wo,
                 int(ignore_index), stream())
            call('tss_upsample_coef_grad_wide', ptr(low), ld(low), ptr(target), ptr(pix), ptr(ws), B, C, h, w, ho, wo, int(ignore_index),
                 code, stream())
        else:
            call('tss_upsample_ce_pixw_fwd', ptr(low), ld(low), ptr(target), ptr(pixw), ptr(weight), norm, ptr(ws), B, C, h, w, ho, wo,
                 int(ignore_index), code, stream())
        call('tss_upsample_ce_group_finalize', ptr(ws), B, C, h, w, ho, wo, 1 if _wide(C) else 0, ptr(group), ptr(sweight), ptr(loss),
             ptr(scale), ptr(group_loss), stream())
        ctx.geom = (B, C, h, w, ho, wo, ld(low), low.dtype)
        ctx.save_for_backward(ws, scale)
        return loss

    @staticmethod
    def backward(ctx, gout):
        ws, scale = ctx.saved_tensors
        B, C, h, w, ho, wo, ldl, dtype = ctx.geom
        gout = gout.to(torch.float32).contiguous()
        base = torch.empty((B, h, w, ldl), dtype=dtype, device=ws.device)   # pad channels are written as zeros
        call('tss_upsample_ce%s_bwd_rows' % _wide(C), ptr(ws), ptr(scale), ptr(gout), ptr(base), ldl, B, C, h, w, ho, wo,
             N.dtype_code(dtype), stream())
        return base.permute(0, 3, 1, 2)[:, :C], None, None, None, None, None, None, None, None


_ONE_GROUP = {}


def upsample_pixel_weighted_cross_entropy(low, target, pixel_weight, scale_factor=None, size=None, ignore_index=-100, weight=None,
                                          label_smoothing=0.0, pixel_norm='weight', sample_group=None, sample_weight=None,
                                          group_loss_out=None):
    """upsample_cross_entropy with every pixel's cross-entropy weighted by a map, from the low-resolution logits (csrc/pixwce.hip); a
    function of its own, so that upsample_cross_entropy keeps its parameter list.  pixel_weight: a contiguous float32 [B,H,W] tensor on
    the logits' device, a constant (no gradient flows to it; a tensor that requires grad is detached).  With k_i = pixel_weight_i *
    weight[t_i] over the valid pixels (target != ignore_index and 0 <= target < C),
        loss = sum_valid k_i ce_i / D,    D = sum_valid k_i ('weight', the weighted mean), sum_valid weight[t_i] ('valid', what the
        plain loss divides by) or B*H*W, ignored pixels included ('pixels': torch.mean(ce * pixel_weight) of DACS / DAFormer).
    The kernels read the map from device memory as it is (negative values and nan included), so an in-place update reaches a
    captured step; a pixel of weight 0 still counts as valid for 'valid' and 'pixels'.  sample_group / sample_weight / group_loss_out
    are upsample_cross_entropy's (N_g is the sum of D over the group's samples); D = 0 gives 0.0 and a zero gradient, with or without
    groups.  ValueError: a host map, a wrong shape, dtype or strides, an unknown pixel_norm, label_smoothing > 0 (not supported with a
    map), more than 256 classes, an output smaller than the map, a batch of more than GROUP_MAX_BATCH samples -- there is no unfused
    route."""
    eps = _check_smoothing(label_smoothing)
    if pixel_norm not in PIXEL_NORMS:
        raise ValueError("pixel_norm must be 'weight', 'valid' or 'pixels', got %r" % (pixel_norm,))
    if eps > 0.0:
        raise ValueError('label smoothing together with a per-pixel weight map is not supported')
    B = low.shape[0]
    if not 1 <= B <= GROUP_MAX_BATCH:
        raise ValueError('a per-pixel weight map takes a batch of 1 to %d samples, got %d' % (GROUP_MAX_BATCH, B))
    if sample_group is None and (sample_weight is not None or group_loss_out is not None):
        raise ValueError('sample_weight and group_loss_out need sample_group')
    host = [t is not None and not (torch.is_tensor(t) and t.is_cuda) for t in (sample_group, sample_weight)]
    if host[0] or host[1]:
        check_sample_groups(sample_group if host[0] else list(range(B)), sample_weight if host[1] else None, B)
    ho, wo = _out_size(low, size, scale_factor)
    if low.shape[1] > WIDEHEAD_MAX_CLASSES or ho < low.shape[2] or wo < low.shape[3]:
        raise ValueError('a per-pixel weight map exists on the fused head only (at most %d classes, an output no smaller than the map): '
                         'got %d classes, %dx%d -> %dx%d' % (WIDEHEAD_MAX_CLASSES, low.shape[1], low.shape[2], low.shape[3], ho, wo))
    low = to_nhwc(materialize(low))
    check_pixel_weight(pixel_weight, (B, ho, wo), low.device, pixel_norm)
    _check_head_target(low, target, ho, wo)
    dev = low.device
    if sample_group is None:        # one group of weight 1: ids all 0, a NULL weight row
        group = _per_device(_ONE_GROUP, dev, lambda: torch.zeros(GROUP_MAX_BATCH, dtype=torch.int32, device=dev))[:B]
        sweight = None
    else:
        group, sweight = _sample_rows(sample_group, sample_weight, B, dev)
    if group_loss_out is None:
        group_loss_out = torch.empty(B, dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(group_loss_out) and group_loss_out.dtype == torch.float32 and tuple(group_loss_out.shape) == (B,)
              and group_loss_out.is_contiguous() and group_loss_out.device == dev):
        raise ValueError('group_loss_out must be a contiguous float32 tensor of shape (%d,) on %s' % (B, dev))
    return UpsamplePixelWeightedCrossEntropyFn.apply(low, target, ho, wo, ignore_index, _class_weight(weight, low.shape[1], dev),
                                                     pixel_weight.detach(), PIXEL_NORMS[pixel_norm], (group, sweight, group_loss_out))


def upsample_cross_entropy(low, target, scale_factor=None, size=None, ignore_index=-100, weight=None, label_smoothing=0.0,
                           sample_group=None, sample_weight=None, group_loss_out=None):
    """Fused decoder head + loss:
    F.cross_entropy(F.interpolate(low, scale_factor, mode='bilinear', align_corners=True), target, weight=weight,
    ignore_index=ignore_index, label_smoothing=label_smoothing)
    computed from the low-resolution logits; the full-resolution logits are never materialised.

    sample_group (B ids in [0, B)) splits the batch into loss groups, each normalised over its OWN valid pixels:
        loss = sum_g (sum_{b in g} sample_weight[b] * CE_sum(b)) / N_g,    N_g = sum_{b in g} (valid pixels' class weights of b)
    e.g. L_sup + lambda * L_unsup of a self-training batch from one head pass.  sample_weight: B non-negative numbers, None = ones.
    group_loss_out: a float32 [B] device tensor that receives the term of every group id (0 for an id no sample uses).  An empty
    group (no valid pixel) contributes 0.0 and a zero gradient -- the rule of focal_loss and dice_loss, NOT the nan of the
    ungrouped mean.  Host sequences are validated before they are copied (ValueError: a wrong length, an id outside [0, B), a
    negative or non-finite weight); device tensors (int32 / float32 [B]) are taken as they are and read by the kernels, so an
    in-place update reaches a captured step (an id outside [0, B) then gives its sample the weight 0).  Grouping exists on the
    fused head only: more than 256 classes or an output smaller than the map is a ValueError, there is no unfused route.
    A per-pixel weight map: upsample_pixel_weighted_cross_entropy."""
    eps = _check_smoothing(label_smoothing)
    if sample_group is not None:
        return _upsample_grouped_cross_entropy(low, target, scale_factor, size, ignore_index, weight, eps, sample_group,
                                               sample_weight, group_loss_out)
    if sample_weight is not None or group_loss_out is not None:
        raise ValueError('sample_weight and group_loss_out need sample_group')
    low = to_nhwc(materialize(low))
    ho, wo = _out_size(low, size, scale_factor)
    if low.shape[1] > WIDEHEAD_MAX_CLASSES or ho < low.shape[2] or wo < low.shape[3]:
        # outside the fused kernels' envelope (at most 256 classes, upsampling only): same result, unfused
        return cross_entropy(upsample_logits(low, size=(ho, wo)), target, ignore_index=ignore_index, weight=weight, label_smoothing=eps)
    if target.dtype != torch.int64 or tuple(target.shape) != (low.shape[0], ho, wo):
        raise RuntimeError('target must be int64 of shape (B,H,W) = %s' % ((low.shape[0], ho, wo),))
    _check_device(target)
    return UpsampleCrossEntropyFn.apply(low, target, ho, wo, ignore_index, _class_weight(weight, low.shape[1], low.device), eps)


class UpsampleOHEMFn(Function):
    """ohem_loss(F.interpolate(low, scale, bilinear, align_corners=True), target) (TSS/losses/ohem_loss.py:10-21 on the
    decoder head of TSS/models/fastscnn.py:40-43) without the full-resolution logits: the per-pixel cross-entropy is computed
    straight from the low-res logits, the radix select runs on that [B,H,W] f32 array, and backward recomputes the softmax of
    the selected pixels from the low-res logits again (gradient tiles, fixed-order gather: no atomics)."""

    @staticmethod
    def forward(ctx, low, target, ho, wo, ignore_index, thresh_loss, numel_frac):
        B, C, h, w = low.shape
        dev = low.device
        target = target.contiguous()
        pix = torch.empty((B, ho, wo), dtype=torch.float32, device=dev)
        out = torch.empty(8, dtype=torch.float32, device=dev)              # loss, 3 pad, the 4 selection parameters (16 B aligned)
        code = N.dtype_code(low.dtype)
        call('tss_upsample_pixel_ce' + _wide(C), ptr(low), ld(low), ptr(target), ptr(pix), B, C, h, w, ho, wo, int(ignore_index), code,
             stream())
        call('tss_ohem_select', ptr(pix), ptr(OHEMFn.workspace(dev)), ptr(out[0:1]), ptr(out[4:8]), B * ho * wo, float(thresh_loss),
             int(B * ho * wo * float(numel_frac)), stream())
        ctx.geom = (B, C, h, w, ho, wo, ld(low), low.dtype, int(ignore_index))
        ctx.save_for_backward(low, target, pix, out)
        return out[0]

    @staticmethod
    def backward(ctx, gout):
        low, target, pix, out = ctx.saved_tensors
        B, C, h, w, ho, wo, ldl, dtype, ignore_index = ctx.geom
        dev = low.device
        gout = gout.to(torch.float32).contiguous()
        ws = torch.empty(getattr(N.lib(), 'tss_upsample_ce%s_ws' % _wide(C))(B, C, h, w, ho, wo), dtype=torch.float32, device=dev)
        code = N.dtype_code(dtype)
        call('tss_upsample_ohem_grad' + _wide(C), ptr(low), ldl, ptr(target), ptr(pix), ptr(out[4:8]), ptr(ws), B, C, h, w, ho, wo,
             ignore_index, code, stream())
        base = torch.empty((B, h, w, ldl), dtype=dtype, device=dev)
        call('tss_upsample_ce%s_bwd' % _wide(C), ptr(ws), ptr(_unit(dev)), ptr(gout), ptr(base), ldl, B, C, h, w, ho, wo, code, stream())
        return base.permute(0, 3, 1, 2)[:, :C], None, None, None, None, None, None


_UNIT = {}


def _unit(dev):
    return _per_device(_UNIT, dev, lambda: torch.ones(1, dtype=torch.float32, device=dev))


def upsample_ohem_loss(low, target, scale_factor=None, size=None, ignore_index=-100, thresh_loss=0.35667494393873245,
                       numel_frac=0.01):
    """Fused decoder head + the reference recipe's loss (scripts/train_fastscnn.py with TSS/losses/ohem_loss.py):
    ohem_loss(F.interpolate(low, scale_factor, mode='bilinear', align_corners=True), target, ...) from the low-res logits."""
    low = to_nhwc(materialize(low))
    ho, wo = _out_size(low, size, scale_factor)
    B = low.shape[0]
    if low.shape[1] > WIDEHEAD_MAX_CLASSES or ho < low.shape[2] or wo < low.shape[3] or (B * ho * wo) % 4:
        return ohem_loss(upsample_logits(low, size=(ho, wo)), target, ignore_index, thresh_loss, numel_frac)
    if target.dtype != torch.int64 or tuple(target.shape) != (B, ho, wo):
        raise RuntimeError('target must be int64 of shape (B,H,W) = %s' % ((B, ho, wo),))
    _check_device(target)
    return UpsampleOHEMFn.apply(low, target, ho, wo, ignore_index, thresh_loss, numel_frac)


def _head_gather(ws, scale, gout, geom):
    """The backward every fused head loss ends in: the gradient tiles of `ws` gathered in a fixed order and scaled by scale * gout;
    returns the NCHW view of the NHWC gradient (pad channels written as zeros)."""
    B, C, h, w, ho, wo, ldl, dtype = geom
    gout = gout.to(torch.float32).contiguous()
    base = torch.empty((B, h, w, ldl), dtype=dtype, device=ws.device)
    call('tss_upsample_ce%s_bwd' % _wide(C), ptr(ws), ptr(scale), ptr(gout), ptr(base), ldl, B, C, h, w, ho, wo, N.dtype_code(dtype), stream())
    return base.permute(0, 3, 1, 2)[:, :C]


class UpsampleFocalFn(Function):
    """focal_loss(F.interpolate(low, bilinear, align_corners=True), target) without the full-resolution logits (csrc/softhead.hip).
    Up to 24 classes: one pass leaves the loss rows and the unscaled gradient tiles, as UpsampleCrossEntropyFn does.  Up to 256: the
    OHEM route -- the per-pixel cross-entropy of the wide head, turned in place into the per-pixel gradient coefficient (and the loss),
    and in backward the wide gradient-tile pass weighted by that array.  No atomics, no host read-back, the same bits on every run."""

    @staticmethod
    def forward(ctx, low, target, ho, wo, alpha, gamma, ignore_index, variant):
        B, C, h, w = low.shape
        dev = low.device
        target = target.contiguous()
        ign, code = _ignore_pair(ignore_index), N.dtype_code(low.dtype)
        out = torch.empty(2, dtype=torch.float32, device=dev)              # loss, alpha / number of valid pixels
        ctx.geom = (B, C, h, w, ho, wo, ld(low), low.dtype)
        if not _wide(C):
            ws = torch.empty(N.lib().tss_upsample_ce_ws(B, C, h, w, ho, wo), dtype=torch.float32, device=dev)
            call('tss_upsample_focal_fwd', ptr(low), ld(low), ptr(target), ptr(ws), ptr(out[0:1]), ptr(out[1:2]), B, C, h, w, ho, wo,
                 *ign, float(alpha), float(gamma), FOCAL_VARIANTS[variant], code, stream())
            ctx.save_for_backward(ws, out)
        else:
            # the wide pixel pass has no has_ignore flag: -1 is out of range, hence ignored anyway
            ctx.wide_ignore = ign[0] if ign[1] else -1
            pix = torch.empty((B, ho, wo), dtype=torch.float32, device=dev)
            rows = torch.empty((N.lib().tss_focal_coef_rows(B * ho * wo), 2), dtype=torch.float64, device=dev)
            call('tss_upsample_pixel_ce_wide', ptr(low), ld(low), ptr(target), ptr(pix), B, C, h, w, ho, wo, ctx.wide_ignore, code, stream())
            call('tss_focal_coef_from_ce', ptr(pix), ptr(target), ptr(rows), ptr(out[0:1]), ptr(out[1:2]), B * ho * wo, C, *ign,
                 float(alpha), float(gamma), FOCAL_VARIANTS[variant], stream())
            ctx.save_for_backward(low, target, pix, out)
        return out[0]

    @staticmethod
    def backward(ctx, gout):
        B, C, h, w, ho, wo, ldl, dtype = ctx.geom
        if not _wide(C):
            ws, out = ctx.saved_tensors
        else:
            low, target, pix, out = ctx.saved_tensors
            ws = torch.empty(N.lib().tss_upsample_ce_wide_ws(B, C, h, w, ho, wo), dtype=torch.float32, device=low.device)
            call('tss_upsample_coef_grad_wide', ptr(low), ldl, ptr(target), ptr(pix), ptr(ws), B, C, h, w, ho, wo, ctx.wide_ignore,
                 N.dtype_code(dtype), stream())
        return _head_gather(ws, out[1:2], gout, ctx.geom), None, None, None, None, None, None, None


def _check_head_target(low, target, ho, wo):
    if target.dtype != torch.int64 or tuple(target.shape) != (low.shape[0], ho, wo):
        raise RuntimeError('target must be int64 of shape (B,H,W) = %s' % ((low.shape[0], ho, wo),))
    _check_device(target)


def upsample_focal_loss(low, target, scale_factor=None, size=None, alpha=0.25, gamma=2.0, ignore_index=-100, variant='reference'):
    """Fused decoder head + focal loss: focal_loss(F.interpolate(low, scale_factor, mode='bilinear', align_corners=True), target, alpha,
    gamma, ignore_index, variant) from the low-resolution logits (the NHWC map of forward_lowres, read in place, or an NCHW tensor);
    the full-resolution logits and their gradient are never materialised.  Every rule of focal_loss holds (validity, both variants,
    ignore_index=None, 0.0 and a zero gradient for an empty valid set).  More than 256 classes, or an output smaller than the map:
    the unfused composition."""
    _check_variant(variant, FOCAL_VARIANTS)
    if not float(gamma) >= 0.0:
        raise ValueError('gamma must be >= 0, got %r' % (gamma,))
    low = to_nhwc(materialize(low))
    ho, wo = _out_size(low, size, scale_factor)
    if low.shape[1] > WIDEHEAD_MAX_CLASSES or ho < low.shape[2] or wo < low.shape[3]:
        return focal_loss(upsample_logits(low, size=(ho, wo)), target, alpha, gamma, ignore_index, variant)
    _check_head_target(low, target, ho, wo)
    return UpsampleFocalFn.apply(low, target, ho, wo, alpha, gamma, ignore_index, variant)


class UpsampleDiceFn(Function):
    """dice_loss(F.interpolate(low, bilinear, align_corners=True), target) without the full-resolution logits (csrc/softhead.hip), up to
    24 classes: a statistics pass and a one-block finalize (loss and the 2C backward coefficients) forward; backward recomputes the
    softmax from the low-resolution rows into gradient tiles, gathered in a fixed order.  No atomics, no host read-back."""

    @staticmethod
    def forward(ctx, low, target, ho, wo, smooth, ignore_index):
        B, C, h, w = low.shape
        dev = low.device
        target = target.contiguous()
        ign = _ignore_pair(ignore_index)
        dws = torch.empty(N.lib().tss_upsample_dice_ws(B, C, h, w, ho, wo), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        call('tss_upsample_dice_fwd', ptr(low), ld(low), ptr(target), ptr(dws), ptr(loss), B, C, h, w, ho, wo, *ign, float(smooth),
             N.dtype_code(low.dtype), stream())
        ctx.geom, ctx.ign = (B, C, h, w, ho, wo, ld(low), low.dtype), ign
        ctx.save_for_backward(low, target, dws)
        return loss

    @staticmethod
    def backward(ctx, gout):
        low, target, dws = ctx.saved_tensors
        B, C, h, w, ho, wo, ldl, dtype = ctx.geom
        ws = torch.empty(N.lib().tss_upsample_ce_ws(B, C, h, w, ho, wo), dtype=torch.float32, device=low.device)
        call('tss_upsample_dice_grad', ptr(low), ldl, ptr(target), ptr(dws), ptr(ws), B, C, h, w, ho, wo, *ctx.ign, N.dtype_code(dtype),
             stream())
        return _head_gather(ws, _unit(low.device), gout, ctx.geom), None, None, None, None, None


def upsample_dice_loss(low, target, num_classes, scale_factor=None, size=None, smooth=1.0, ignore_index=-100):
    """Fused decoder head + soft Dice loss: dice_loss(F.interpolate(low, scale_factor, mode='bilinear', align_corners=True), target,
    num_classes, smooth, ignore_index) from the low-resolution logits; the full-resolution logits and their gradient are never
    materialised.  Every rule of dice_loss holds.  More than 24 classes (HEAD_REGISTER_CLASSES), or an output smaller than the map:
    the unfused composition."""
    low = materialize(low)
    _check_num_classes(low, num_classes)
    if not float(smooth) >= 0.0:
        raise ValueError('smooth must be >= 0, got %r' % (smooth,))
    low = to_nhwc(low)
    ho, wo = _out_size(low, size, scale_factor)
    if low.shape[1] > HEAD_REGISTER_CLASSES or ho < low.shape[2] or wo < low.shape[3]:
        return dice_loss(upsample_logits(low, size=(ho, wo)), target, num_classes, smooth, ignore_index)
    _check_head_target(low, target, ho, wo)
    return UpsampleDiceFn.apply(low, target, ho, wo, smooth, ignore_index)


def upsample_argmax_confusion(low, target=None, scale_factor=None, size=None, ignore_index=255, confusion=None,
                              want_pred=True):
    """argmax_confusion(F.interpolate(low, scale, bilinear, align_corners=True), ...) without the full-resolution logits
    (the evaluator's decoder head + metric update as one operator).  Returns (pred uint8 or None, confusion)."""
    low = to_nhwc(materialize(low))
    _check_device(low)
    ho, wo = _out_size(low, size, scale_factor)
    B, C, h, w = low.shape
    if C > WIDEHEAD_MAX_CLASSES:
        raise ValueError('upsample_argmax_confusion supports at most %d classes, got %d' % (WIDEHEAD_MAX_CLASSES, C))
    if ho < h or wo < w:
        return argmax_confusion(upsample_logits(low, size=(ho, wo)), target, ignore_index=ignore_index,
                                confusion=confusion, want_pred=want_pred)
    pred = torch.empty((B, ho, wo), dtype=torch.uint8, device=low.device) if want_pred else None
    if target is not None:
        if target.dtype != torch.int64 or tuple(target.shape) != (B, ho, wo):
            raise RuntimeError('target must be int64 of shape (B,H,W) = %s' % ((B, ho, wo),))
        _check_device(target)
        if confusion is None:
            confusion = torch.zeros((C, C), dtype=torch.int64, device=low.device)
    call('tss_upsample_argmax_confusion' + _wide(C), ptr(low), ld(low), ptr(target.contiguous()) if target is not None else None,
         ptr(pred), ptr(confusion), B, C, h, w, ho, wo, int(ignore_index), N.dtype_code(low.dtype), stream())
    return pred, confusion


class _MsMap(ctypes.Structure):
    """tss_msmap of include/tss_hip.h."""
    _fields_ = [('low', ctypes.c_void_p), ('ldl', ctypes.c_long), ('h', ctypes.c_int), ('w', ctypes.c_int),
                ('flip', ctypes.c_int), ('first', ctypes.c_int)]


MULTISCALE_MAX_MAPS = 16
_MS_AVERAGE = {'softmax': 0, 'logits': 1}


def resize_flip_image(x, size, flip=True, out_dtype=None):
    """The input of one scale of multi-scale + flip inference, one launch: the float32 NCHW batch x resized (bilinear,
    align_corners=True, up or down) to `size`, followed -- with `flip` -- by its horizontal mirror as samples B..2B-1.  The first
    half is bit-identical to resize_image(x, size, out_dtype=...), the second to its .flip(-1)."""
    _check_device(x)
    if x.dtype != torch.float32:
        raise TypeError('resize_flip_image takes the float32 image, got %s' % x.dtype)
    x = x.contiguous()
    ho, wo = _out_size(x, size, None)
    B, C, H, W = x.shape
    out_dtype = out_dtype or x.dtype
    y = torch.empty((2 * B if flip else B, C, ho, wo), dtype=out_dtype, device=x.device)
    call('tss_resize_flip_planar', ptr(x), ptr(y), N.dtype_code(out_dtype), B, C, H, W, ho, wo, 1 if flip else 0, stream())
    return y


def multiscale_argmax_confusion(lows, flips, target=None, size=None, ignore_index=255, confusion=None, want_pred=True,
                                average='softmax'):
    """Multi-scale + flip fusion of low-resolution logit maps (tss_multiscale_argmax_confusion): every map is upsampled to `size`
    (bilinear, align_corners=True), mirrored back where its `flips` entry says it came from the mirrored image (the flip is taken
    AFTER the upsample: F.interpolate(...).flip(-1)), the per-map softmax (average='softmax') or the raw logits ('logits') are summed
    in list order, and the arg-max of the sum is scored against `target`.  No full-resolution float tensor exists.
    lows[i]: logits [B,C,h,w] with flips[i] a bool, or [2B,C,h,w] with flips[i] == (False, True): the plain and the mirrored half of
    one forward (two maps).  At most 16 maps, at most 256 classes (up to 24 the scores of a pixel live in registers, past that the
    class-chunked kernel of csrc/widehead.hip runs: same arithmetic per score, same results), no map larger than `size`.
    Returns (pred uint8 or None, confusion)."""
    if average not in _MS_AVERAGE:
        raise ValueError("average must be 'softmax' or 'logits', got %r" % (average,))
    lows, flips = list(lows), list(flips)
    if not lows:
        raise ValueError('multiscale_argmax_confusion needs at least one map')
    if len(lows) != len(flips):
        raise ValueError('%d maps but %d flips entries' % (len(lows), len(flips)))
    lows = [materialize(low) for low in lows]
    first = lows[0]
    C = first.shape[1]
    for low in lows:
        if low.dtype != first.dtype or low.device != first.device or low.shape[1] != C:
            raise ValueError('the maps must share dtype, device and class count: got %s %s C=%d after %s %s C=%d'
                             % (low.dtype, low.device, low.shape[1], first.dtype, first.device, C))
    _check_device(first)        # one device for all (above); to_nhwc passes a channels-last tensor on unchecked, wherever it lives
    lows = [to_nhwc(low) for low in lows]
    first = lows[0]
    if target is not None:
        B = target.shape[0]
    else:
        B = first.shape[0] // 2 if isinstance(flips[0], (tuple, list)) else first.shape[0]
    if size is None:
        if target is None:
            raise ValueError('multiscale_argmax_confusion needs `size` or a target')
        size = tuple(target.shape[-2:])
    ho, wo = _out_size(first, size, None)
    descs = []
    for low, f in zip(lows, flips):
        halves = tuple(bool(v) for v in f) if isinstance(f, (tuple, list)) else (bool(f),)
        if low.shape[0] != len(halves) * B:
            raise ValueError('a map of batch %d does not match flips entry %r at batch size %d' % (low.shape[0], f, B))
        h, w = low.shape[2], low.shape[3]
        if h > ho or w > wo:
            raise ValueError('map %dx%d is larger than the output %dx%d (maps are upsampled, never reduced)' % (h, w, ho, wo))
        descs += [_MsMap(low.data_ptr(), ld(low), h, w, int(fl), i * B) for i, fl in enumerate(halves)]
    if len(descs) > MULTISCALE_MAX_MAPS:
        raise ValueError('at most %d maps per call, got %d' % (MULTISCALE_MAX_MAPS, len(descs)))
    if C > WIDEHEAD_MAX_CLASSES:
        raise ValueError('multiscale_argmax_confusion supports at most %d classes, got %d' % (WIDEHEAD_MAX_CLASSES, C))
    pred = torch.empty((B, ho, wo), dtype=torch.uint8, device=first.device) if want_pred else None
    if target is not None:
        if target.dtype != torch.int64 or tuple(target.shape) != (B, ho, wo):
            raise RuntimeError('target must be int64 of shape (B,H,W) = %s' % ((B, ho, wo),))
        _check_device(target)
        target = target.contiguous()
        if confusion is None:
            confusion = torch.zeros((C, C), dtype=torch.int64, device=first.device)
    call('tss_multiscale_argmax_confusion' + _wide(C), (_MsMap * len(descs))(*descs), len(descs), ptr(target), ptr(pred), ptr(confusion),
         B, C, ho, wo, int(ignore_index), _MS_AVERAGE[average], N.dtype_code(first.dtype), stream())
    return pred, confusion


def argmax_confusion(logits, target=None, num_classes=None, ignore_index=255, confusion=None, want_pred=True):
    """argmax over dim 1 (lowest index wins ties) and, with a target, the confusion-matrix update
    (rows = truth, cols = prediction) that create_segmentation_evaluator's metrics need (TSS/engine.py:65-72).  At most 256 classes
    (past 64 the counters of the first kernel no longer fit LDS: tss_argmax_confusion_wide)."""
    _check_device(logits)
    logits = logits.contiguous()
    B, C, H, W = logits.shape
    if C > WIDEHEAD_MAX_CLASSES:
        raise ValueError('argmax_confusion supports at most %d classes, got %d' % (WIDEHEAD_MAX_CLASSES, C))
    pred = torch.empty((B, H, W), dtype=torch.uint8, device=logits.device) if want_pred else None
    if target is not None and confusion is None:
        confusion = torch.zeros((C, C), dtype=torch.int64, device=logits.device)
    call('tss_argmax_confusion' + ('_wide' if C > 64 else ''), ptr(logits), ptr(target.contiguous()) if target is not None else None, ptr(pred),
         ptr(confusion), B, C, H * W, int(ignore_index), N.dtype_code(logits.dtype), stream())
    return pred, confusion
