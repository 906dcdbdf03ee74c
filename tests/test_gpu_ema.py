"""The weight average of csrc/optim.hip -- the step kernels' EMA instances (FlatOptimizer.attach_ema: tss_adamw_step_groups_ema,
tss_sgd_step_groups_ema) and the rows kernel (tss_ema_rows) -- against tests/ema_ref.py.

Bounds.  Trajectories: cases.rel_err < 1e-5 against the float64 restatement, the criterion of tests/test_gpu_flat_optim.py for the
parameters of the same cases.  The average itself, given the parameters the kernel produced: bit for bit against the float32
restatement of its three roundings (ema_ref.lerp32); the factor: bit for bit (plain) or within one unit in the last place (warm-up:
the device's division is the only freedom) of ema_ref.omd32."""
import functools

import numpy as np
import pytest
import torch

from tests import cases, ema_ref as M, flatopt_ref as R
from tests.test_gpu_flat_optim import make_opt, ref_groups

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BIG = 2048 * 256 + 77             # the step kernels' grid is capped at 2048 blocks of 256: a second trip for 77 elements
CUT = 300001
STEP_KINDS = ['adamw', 'sgd_plain', 'sgd_momentum', 'sgd_nesterov']


@functools.lru_cache(maxsize=None)
def small_case():
    return R.make_case()


def f32(case):
    return R.flatten(case['params']).astype(np.float32)


def load_grads(opt, gs):
    opt.flat_grad.copy_(torch.from_numpy(R.flatten(gs).astype(np.float32)))


def with_ema(case, kind, decay, warmup=False, max_norm=None, device_state=False, ema=None):
    opt, _ = make_opt(case, kind, ref_groups(case, kind), max_norm)
    opt.device_state = device_state
    if ema is None:
        ema = torch.empty_like(opt.flat_param)
    ema.copy_(opt.flat_param)
    opt.attach_ema(ema, decay, warmup)
    return opt, ema


def bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).tobytes()


# ----------------------------------------------------------------------------- 1. trajectories

@pytest.mark.parametrize('max_norm', [None, 5.0])
@pytest.mark.parametrize('kind', STEP_KINDS)
def test_trajectories_match_the_restatement(kind, max_norm):
    """The 3-group case of flatopt_ref (its six tensors: 1354 elements, 8 steps) through the fused entry, decay 0.9: parameters and
    average against the float64 restatement, and the average inside the hull of the parameters it averaged."""
    case = small_case()
    assert len(case['ranges']) == 3 and len(case['grads']) == 8
    opt, ema = with_ema(case, kind, 0.9, max_norm=max_norm)
    for gs in case['grads']:
        load_grads(opt, gs)
        opt.step()
    want_p, want_e, history = M.run(case, kind.split('_')[0], ref_groups(case, kind), 0.9, max_norm=max_norm)
    got_p, got_e = opt.flat_param.cpu().numpy(), ema.cpu().numpy()
    err_p, err_e = cases.rel_err(got_p, want_p), cases.rel_err(got_e, want_e)
    print(kind, 'max_norm', max_norm, 'rel_err p', err_p, 'e', err_e)
    assert err_p < 1e-5 and err_e < 1e-5, (kind, max_norm, err_p, err_e)
    assert opt.ema_updates == R.STEPS and cases.rel_err(got_e, got_p) > 1e-3         # an average, not a copy
    # a convex combination of the initial and the 8 stepped parameters: the restatement's hull, widened by the trajectory bound and
    # by 3 float32 roundings per step, both relative to the largest parameter
    slack = (1e-5 + R.STEPS * 3 * 2.0 ** -24) * np.abs(history).max()
    assert (got_e >= np.min(history, axis=0) - slack).all() and (got_e <= np.max(history, axis=0) + slack).all()


# ----------------------------------------------------------------------------- 2. the average, bit for bit

@pytest.mark.parametrize('device_state', [False, True])
@pytest.mark.parametrize('warmup', [False, True])
@pytest.mark.parametrize('decay', [0.0, 0.5, 0.999, 0.9999])
@pytest.mark.parametrize('kind', ['adamw', 'sgd_nesterov'])
def test_average_is_the_three_rounding_restatement_bit_for_bit(kind, decay, warmup, device_state):
    from torch_semantic_segmentation_amd import engine as E
    case = small_case()
    opt, ema = with_ema(case, kind, decay, warmup, device_state=device_state)
    for k, gs in enumerate(case['grads']):
        prev = ema.cpu().numpy()
        load_grads(opt, gs)
        opt.step()
        if device_state:
            row = opt.ema_state.cpu().numpy()
            assert row[0] == k + 1
            omd = row[1]
        else:
            omd = E.ema_omd(k, decay, warmup)
        assert omd.dtype == np.float32
        want = M.omd32(k, decay, warmup)
        if warmup:
            assert M.ulps32(omd, want) <= 1, (k, omd, want)
        else:
            assert omd.tobytes() == want.tobytes() == (np.float32(1.0) - np.float32(decay)).tobytes()
        assert bits(ema) == bits(M.lerp32(prev, opt.flat_param.cpu().numpy(), omd)), (kind, decay, warmup, device_state, k)
    sd = opt.state_dict()['flat']['ema_state'].cpu().numpy()
    assert sd[0] == R.STEPS and M.ulps32(sd[1], M.omd32(R.STEPS - 1, decay, warmup)) <= (1 if warmup else 0)
    if decay == 0.0 and not warmup:          # omd = 1: e + (p - e), one rounding away from p wherever p - e is inexact
        assert cases.rel_err(ema.cpu().numpy(), opt.flat_param.cpu().numpy()) < 2.0 ** -22


# ----------------------------------------------------------------------------- 3. the step is not disturbed

@pytest.mark.parametrize('device_state', [False, True])
@pytest.mark.parametrize('max_norm', [None, 5.0])
@pytest.mark.parametrize('kind', STEP_KINDS)
def test_step_is_bit_identical_with_and_without_the_average(kind, max_norm, device_state):
    case = small_case()
    plain, _ = make_opt(case, kind, ref_groups(case, kind), max_norm)
    plain.device_state = device_state
    fused, ema = with_ema(case, kind, 0.999, max_norm=max_norm, device_state=device_state)
    for gs in case['grads'][:3]:
        for opt in (plain, fused):
            load_grads(opt, gs)
            opt.step()
    for name in ('flat_param',) + type(plain)._state_names:
        a, b = getattr(plain, name), getattr(fused, name)
        assert (a is None) == (b is None), name
        if a is not None:
            assert bits(a) == bits(b), (kind, name)
    assert cases.rel_err(plain.flat_param.cpu().numpy(), f32(case)) > 1e-3 and bits(ema) != bits(fused.flat_param)


# ----------------------------------------------------------------------------- 4. grid stride, group boundary, sentinels

@functools.lru_cache(maxsize=None)
def big_case():
    return R.make_case(shapes=((CUT,), (BIG - CUT,)), group_sizes=(1, 1), steps=2, big_step=1, seed=12)


@pytest.mark.parametrize('kind', ['adamw', 'sgd_nesterov'])
def test_grid_stride_second_trip_group_boundary_and_sentinels(kind):
    from torch_semantic_segmentation_amd import engine as E
    case = big_case()
    assert case['ranges'] == [(0, CUT), (CUT, BIG)]
    guard = 64                               # floats on either side: the average stays 16-byte aligned, as an allocation is
    arena = torch.full((BIG + 2 * guard,), float('nan'), device=DEV)
    opt, ema = with_ema(case, kind, 0.9, max_norm=5.0, ema=arena[guard:guard + BIG])
    sentinels = bits(torch.cat([arena[:guard], arena[guard + BIG:]]).view(torch.int32))
    want = ema.cpu().numpy()
    for k, gs in enumerate(case['grads']):
        load_grads(opt, gs)
        opt.step()
        want = M.lerp32(want, opt.flat_param.cpu().numpy(), E.ema_omd(k, 0.9))
    got = ema.cpu().numpy()
    assert bits(got[-5:]) == bits(want[-5:]) and bits(got[CUT - 1:CUT + 1]) == bits(want[CUT - 1:CUT + 1])
    assert bits(got) == bits(want)
    assert not np.isnan(got).any() and cases.rel_err(got, f32(case)) > 1e-6          # it moved, everywhere it should
    assert bits(torch.cat([arena[:guard], arena[guard + BIG:]]).view(torch.int32)) == sentinels
    want_p, want_e, _ = M.run(case, kind.split('_')[0], ref_groups(case, kind), 0.9, max_norm=5.0)
    assert cases.rel_err(opt.flat_param.cpu().numpy(), want_p) < 1e-5 and cases.rel_err(got, want_e) < 1e-5


# ----------------------------------------------------------------------------- 5. capture

CAPTURE_CASE = dict(shapes=((300,), (41,), (700,)), group_sizes=(2, 1), steps=3, big_step=1, seed=14)


def captured_run(case, kind, attach=True):
    """device_state=True, step() captured once (tick + step kernel), replayed once per gradient set; the parameters after each."""
    if attach:
        opt, ema = with_ema(case, kind, 0.999, warmup=True, device_state=True)
    else:
        (opt, _), ema = make_opt(case, kind, ref_groups(case, kind)), None
        opt.device_state = True
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    after = []
    for gs in case['grads']:
        load_grads(opt, gs)
        graph.replay()
        after.append(opt.flat_param.cpu().numpy())
    torch.cuda.synchronize()
    return opt, ema, after


@pytest.mark.parametrize('kind', ['sgd_plain', 'sgd_momentum', 'sgd_nesterov'])
def test_captured_device_state_step_equals_eager_host_steps(kind):
    """3 replays of a captured device_state step against 3 eager steps whose counter and factor are kernel arguments computed on the
    host: parameters and average bit for bit, warm-up on.  SGD, whose two modes share every operand (the learning rates are the same
    float32 values on either side); AdamW has its own test below."""
    case = R.make_case(**CAPTURE_CASE)
    eager, ema_e = with_ema(case, kind, 0.999, warmup=True)
    for gs in case['grads']:
        load_grads(eager, gs)
        eager.step()
    dev, ema_d, _ = captured_run(case, kind)
    assert dev.ema_state.cpu().numpy()[0] == 3
    assert bits(dev.ema_state) == bits(eager.state_dict()['flat']['ema_state'])      # the host mirror has the tick's bits
    assert bits(dev.flat_param) == bits(eager.flat_param)
    assert bits(ema_d) == bits(ema_e)
    assert cases.rel_err(ema_e.cpu().numpy(), eager.flat_param.cpu().numpy()) > 1e-4


def test_captured_device_state_adamw_step():
    """AdamW's bias corrections 1 - beta^step come from the host's powf as kernel arguments and from the device's powf in the tick
    kernel, with or without an average: its parameters are not bit-identical across the two modes to begin with (tests/
    test_gpu_flat_optim.py holds the captured step to 1e-5).  What the average adds IS exact across the modes: the row {k, omd} has
    the host mirror's bits, the captured parameters are bit for bit those of the captured step without an average, and the average
    is bit for bit the host-mode arithmetic (host factor, three roundings) applied to those parameters."""
    from torch_semantic_segmentation_amd import engine as E
    case = R.make_case(**CAPTURE_CASE)
    eager, ema_e = with_ema(case, 'adamw', 0.999, warmup=True)
    for gs in case['grads']:
        load_grads(eager, gs)
        eager.step()
    dev, ema_d, after = captured_run(case, 'adamw')
    bare, _, after_bare = captured_run(case, 'adamw', attach=False)
    assert dev.ema_state.cpu().numpy()[0] == 3
    assert bits(dev.ema_state) == bits(eager.state_dict()['flat']['ema_state'])
    assert [a.tobytes() for a in after] == [a.tobytes() for a in after_bare]
    assert bits(dev.exp_avg) == bits(bare.exp_avg) and bits(dev.exp_avg_sq) == bits(bare.exp_avg_sq)
    want = f32(case)
    for k, p in enumerate(after):
        want = M.lerp32(want, p, E.ema_omd(k, 0.999, True))
    assert bits(ema_d) == bits(want)
    err_p = cases.rel_err(after[-1], eager.flat_param.cpu().numpy())
    err_e = cases.rel_err(ema_d.cpu().numpy(), ema_e.cpu().numpy())
    print('adamw captured vs eager host mode: rel_err p', err_p, 'e', err_e)
    assert err_p < 1e-5 and err_e < 1e-5


# ----------------------------------------------------------------------------- 6. the rows kernel

LERP, COPY_F32, COPY_I64 = 0, 1, 2
SENTINEL = 0x7FC0DEAD                    # a NaN with a payload: guards are compared on bits


def float_rows():
    """(mode, length, source offset, destination offset) in floats from a 16-byte boundary."""
    rows = [(LERP, n, so, do) for n in (0, 1, 3, 4, 5, 257, 1025) for so in range(4) for do in range(4)]
    rows += [(LERP, 70001, o, o) for o in range(4)] + [(LERP, 70001, 1, 3), (LERP, 70001, 0, 2)]
    rows += [(COPY_F32, n, so, do) for n in (0, 1, 5, 257, 1025) for so, do in ((0, 0), (1, 1), (3, 3), (0, 2), (3, 1))]
    return rows


def lay_out(rows, gap=8):
    """Element offsets of the rows in an arena: each starts `offset` elements past a multiple of 4 with at least `gap` guard
    elements before it; returns (offsets, arena size)."""
    at, out = gap, []
    for n, off in rows:
        at = (at + 3) // 4 * 4 + off
        out.append(at)
        at += n + gap
    return out, at + gap


def run_rows(table, omd, state=None):
    from torch_semantic_segmentation_amd import _native as N
    t = torch.tensor(table, dtype=torch.int64, device=DEV).reshape(-1, 4)
    N.call('tss_ema_rows', N.ptr(t), t.shape[0], float(omd), N.ptr(state), N.stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize('omd_on_device', [False, True])
def test_rows_kernel_values_and_guards(omd_on_device):
    rng = np.random.RandomState(21)
    rows = float_rows()
    s_at, s_size = lay_out([(n, so) for _, n, so, _ in rows])
    d_at, d_size = lay_out([(n, do) for _, n, _, do in rows])
    src = rng.standard_normal(s_size).astype(np.float32)
    dst = np.full(d_size, SENTINEL, dtype=np.uint32).view(np.float32)
    for (mode, n, _, _), d in zip(rows, d_at):
        dst[d:d + n] = rng.standard_normal(n).astype(np.float32)
    irows = [(1, 0), (5, 1), (1, 1), (5, 0)]                                        # (length, offset in int64 from a 16-byte boundary)
    is_at, is_size = lay_out([(n, o % 2) for n, o in irows])
    id_at, id_size = lay_out([(n, (o + 1) % 2) for n, o in irows])
    isrc = rng.randint(-2 ** 62, 2 ** 62, size=is_size, dtype=np.int64)
    idst = np.full(id_size, -0x0DEAD0000DEAD, dtype=np.int64)

    omd = M.omd32(0, 0.999)
    want, iwant = dst.copy(), idst.copy()
    for (mode, n, _, _), s, d in zip(rows, s_at, d_at):
        want[d:d + n] = M.lerp32(dst[d:d + n], src[s:s + n], omd) if mode == LERP else src[s:s + n]
    for (n, _), s, d in zip(irows, is_at, id_at):
        iwant[d:d + n] = isrc[s:s + n]

    tsrc, tdst = torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV)
    tisrc, tidst = torch.from_numpy(isrc).to(DEV), torch.from_numpy(idst).to(DEV)
    assert tsrc.data_ptr() % 16 == 0 and tdst.data_ptr() % 16 == 0 and tisrc.data_ptr() % 16 == 0 and tidst.data_ptr() % 16 == 0
    table = [[tsrc.data_ptr() + 4 * s, tdst.data_ptr() + 4 * d, n, mode] for (mode, n, _, _), s, d in zip(rows, s_at, d_at)]
    table += [[tisrc.data_ptr() + 8 * s, tidst.data_ptr() + 8 * d, n, COPY_I64] for (n, _), s, d in zip(irows, is_at, id_at)]
    assert {(r[0] % 16, r[1] % 16) for r in table[:112]} == {(4 * a, 4 * b) for a in range(4) for b in range(4)}
    if omd_on_device:                        # {k, omd} as the step's tick leaves it; the host argument is then not read
        run_rows(table, 0.5, torch.tensor([7.0, float(omd)], dtype=torch.float32, device=DEV))
    else:
        run_rows(table, omd)
    assert bits(tdst.view(torch.int32)) == want.view(np.int32).tobytes()            # rows AND the guards between and around them
    assert bits(tidst) == iwant.tobytes()
    assert bits(tsrc) == src.tobytes() and bits(tisrc) == isrc.tobytes()            # sources are read only
    assert sum(n for m, n, _, _ in rows if m == LERP) > 0 and not np.array_equal(want.view(np.int32), dst.view(np.int32))


def test_rows_kernel_more_rows_than_its_grid_and_none_at_all():
    """4100 rows of 0..3 elements (the grid has at most 4096 rows of blocks: the last ones take a second trip), then the empty table."""
    from torch_semantic_segmentation_amd import _native as N
    rng = np.random.RandomState(22)
    lens = [r % 4 for r in range(4100)]
    at, size = lay_out([(n, r % 3) for r, n in enumerate(lens)], gap=2)
    src = rng.standard_normal(size).astype(np.float32)
    dst = np.full(size, SENTINEL, dtype=np.uint32).view(np.float32)
    for a, n in zip(at, lens):
        dst[a:a + n] = rng.standard_normal(n).astype(np.float32)
    omd = M.omd32(3, 0.9999, True)
    want = dst.copy()
    for a, n in zip(at, lens):
        want[a:a + n] = M.lerp32(dst[a:a + n], src[a:a + n], omd)
    tsrc, tdst = torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV)
    table = [[tsrc.data_ptr() + 4 * a, tdst.data_ptr() + 4 * a, n, LERP] for a, n in zip(at, lens)]
    run_rows(table, omd)
    assert bits(tdst.view(torch.int32)) == want.view(np.int32).tobytes()
    t = torch.tensor(table, dtype=torch.int64, device=DEV)
    assert N.lib().tss_ema_rows(N.ptr(t), 0, float(omd), None, N.stream()) == 0     # no rows: success, nothing launched
    assert N.lib().tss_ema_rows(None, 0, float(omd), None, N.stream()) == 0
    torch.cuda.synchronize()
    assert bits(tdst.view(torch.int32)) == want.view(np.int32).tobytes()
    for bad in ((N.ptr(t), -1, float(omd), None), (None, 3, float(omd), None), (N.ptr(t), 3, 0.0, None), (N.ptr(t), 3, 1.5, None),
                (N.ptr(t), 3, float('nan'), None)):
        assert N.lib().tss_ema_rows(*bad, N.stream()) == -2
    torch.cuda.synchronize()
    assert bits(tdst.view(torch.int32)) == want.view(np.int32).tobytes()


# ----------------------------------------------------------------------------- 7. rejections of the C entries

@pytest.mark.parametrize('kind', ['adamw', 'sgd'])
def test_c_abi_rejections_launch_nothing(kind):
    from torch_semantic_segmentation_amd import _native as N
    from torch_semantic_segmentation_amd.engine import _OptGroup
    n = 1000
    g = torch.Generator(device=DEV).manual_seed(3)
    p, grad, m, v, e = (torch.randn(n, device=DEV, generator=g) for _ in range(5))
    v.abs_()
    state, lr, ema_state = torch.zeros(6, device=DEV), torch.full((2,), 1e-2, device=DEV), torch.zeros(2, device=DEV)
    everything = (p, grad, m, v, e, state, ema_state)
    before = [bits(t) for t in everything]
    good = (_OptGroup * 2)(_OptGroup(0, 400, 1e-2, 0.0, 0.9, 0.999 if kind == 'adamw' else 0.0, 1e-8, 0),
                           _OptGroup(400, n, 1e-2, 0.0, 0.9, 0.999 if kind == 'adamw' else 0.0, 1e-8, 0))
    gap = (_OptGroup * 2)(good[0], _OptGroup(401, n, 1e-2, 0.0, 0.9, 0.0, 1e-8, 0))
    short = (_OptGroup * 2)(good[0], _OptGroup(400, n - 1, 1e-2, 0.0, 0.9, 0.0, 1e-8, 0))

    def call(ema=e, groups=good, ngroups=2, decay=0.999, omd=1e-3, device=False, row=ema_state):
        moments = (N.ptr(m), N.ptr(v)) if kind == 'adamw' else (N.ptr(m),)
        fn = N.lib().tss_adamw_step_groups_ema if kind == 'adamw' else N.lib().tss_sgd_step_groups_ema
        return fn(N.ptr(p), N.ptr(grad), *moments, N.ptr(ema), n, groups, ngroups, N.ptr(lr) if device else None,
                  N.ptr(state) if device else None, None, 1.0, 1, decay, 0, omd, N.ptr(row) if device else None, N.stream())

    for device in (False, True):
        assert call(ema=None, device=device) == -2
        for decay in (1.0, -0.25, 1.5, float('nan')):
            assert call(decay=decay, device=device) == -2
        for groups in (gap, short):
            assert call(groups=groups, device=device) == -2
        assert call(ngroups=0, device=device) == -2 and call(ngroups=9, device=device) == -2
    for omd in (0.0, -0.5, 1.5, float('nan')):           # the host's factor, read without a device state only
        assert call(omd=omd) == -2
    assert call(device=True, row=None) == -2               # a device state needs the average's row next to it
    torch.cuda.synchronize()
    assert [bits(t) for t in everything] == before
    assert call() == 0                                     # and the well-formed call steps
    torch.cuda.synchronize()
    assert bits(p) != before[0] and bits(e) != before[4] and bits(grad) == before[1]
