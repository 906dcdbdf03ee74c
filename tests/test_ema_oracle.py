"""The checker of the weight-average tests (tests/ema_ref.py) against torch.optim.swa_utils.AveragedModel in float64, its float32
restatement of the kernel's three roundings, the warm-up sequence, and the host-side contract of engine.ModelEMA /
FlatOptimizer.attach_ema on CPU tensors (rejections, state_dict).  CPU only: nothing here launches a kernel."""
import copy

import numpy as np
import pytest
import torch
from torch import nn
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from tests import cases, ema_ref as M, flatopt_ref as R


def small_module():
    torch.manual_seed(3)
    return nn.Sequential(nn.Conv2d(3, 4, 3, bias=True), nn.BatchNorm2d(4)).double()


@pytest.mark.parametrize('decay', [0.5, 0.999])
def test_restatement_is_torch_averaged_model_in_float64(decay):
    """8 updates of a module with one BatchNorm whose parameters and running statistics move between them.  AveragedModel COPIES on
    its first update_parameters(); called once right after construction, every later call is the lerp, as ModelEMA.update() is from
    the first.  Both sides float64, only the operation order differs: 1e-12.  num_batches_tracked is an integer: torch runs it
    through the same average and truncates, ModelEMA copies the model's counter -- it is not compared."""
    m = small_module()
    avg = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=True)
    avg.update_parameters(m)
    mine = {k: v.detach().numpy().copy() for k, v in m.state_dict().items() if v.is_floating_point()}
    g = torch.Generator().manual_seed(5)
    for k in range(8):
        m.train()
        with torch.no_grad():
            for p in m.parameters():         # a stand-in for the optimizer step; the forward moves the running statistics
                p.add_(0.1 * torch.randn(p.shape, dtype=torch.float64, generator=g))
            m(torch.randn(2, 3, 6, 6, dtype=torch.float64, generator=g))
        avg.update_parameters(m)
        for name, v in m.state_dict().items():
            if v.is_floating_point():
                mine[name] = M.step64(mine[name], v.detach().numpy(), k, decay)
    theirs = avg.module.state_dict()
    assert set(mine) == {'0.weight', '0.bias', '1.weight', '1.bias', '1.running_mean', '1.running_var'}
    for name, v in mine.items():
        assert cases.rel_err(v, theirs[name].numpy()) < 1e-12, name
        assert cases.rel_err(v, m.state_dict()[name].numpy()) > 1e-3, name        # the average lags the model: it is not a copy


def test_trajectory_restatement_averages_the_flat_optimizer_restatement():
    case = R.make_case()
    p, e, history = M.run(case, 'adamw', R.adamw_groups(case), 0.9)
    want, _ = R.run(case, 'adamw', R.adamw_groups(case))
    assert np.array_equal(p, want) and len(history) == R.STEPS + 1
    assert (e >= np.min(history, axis=0) - 1e-12).all() and (e <= np.max(history, axis=0) + 1e-12).all()
    direct = history[0]
    for k in range(R.STEPS):
        direct = 0.9 * direct + 0.1 * history[k + 1]
    assert cases.rel_err(e, direct) < 1e-12


@pytest.mark.parametrize('decay', [0.0, 0.5, 0.999, 0.9999])
def test_float32_restatement_rounds_three_times(decay):
    """lerp32 against float64: p - e, the product and the sum each err by at most 2^-24 relative to their own result; every
    intermediate is at most 2 * max(|e|, |p|) in magnitude, so the result is within 3 * 2^-23 * max(|e|, |p|) of the exact one."""
    rng = np.random.RandomState(1)
    e, p = rng.standard_normal(4096).astype(np.float32), rng.standard_normal(4096).astype(np.float32)
    omd = M.omd32(0, decay)
    got = M.lerp32(e, p, omd)
    want = e.astype(np.float64) + (p.astype(np.float64) - e) * float(omd)
    assert got.dtype == np.float32
    assert (np.abs(got - want) <= 3 * 2.0 ** -23 * np.maximum(np.abs(e), np.abs(p))).all()
    assert np.array_equal(M.lerp32(e, e, omd), e)                                  # a fixed point, exactly


def test_lerp_form_against_the_weighted_sum_at_decay_09999():
    """Why the kernel computes e + (p - e) * omd and not d*e + (1 - d)*p: at decay = 0.9999 a step moves the average by about 1e-4 of
    the distance to the parameter, around one unit in the last place of e when p is within a per cent of it.  In the lerp form p - e
    is exact there (Sterbenz), the product errs by 2^-24 of that tiny move, and only the final sum rounds at the scale of e: at most
    half a unit in the last place off the exact result, and exactly e when p == e.  The weighted sum rounds d*e and the sum at the
    scale of e -- up to a whole unit, as large as the move itself."""
    rng = np.random.RandomState(2)
    e = rng.standard_normal(4096).astype(np.float32)
    p = (e * np.float32(1.0 + 2.0 ** -7)).astype(np.float32)
    d, omd = np.float32(0.9999), M.omd32(0, 0.9999)
    exact = e.astype(np.float64) + (p.astype(np.float64) - e) * float(omd)
    lerp = M.lerp32(e, p, omd)
    weighted = ((d * e).astype(np.float32) + (omd * p).astype(np.float32)).astype(np.float32)
    half_ulp = 2.0 ** -24 * np.abs(p).astype(np.float64)                              # |e'| <= |p|
    err_lerp, err_weighted = np.abs(lerp - exact), np.abs(weighted - exact)
    assert (err_lerp <= half_ulp * (1 + 2.0 ** -10)).all()
    assert err_weighted.max() > 1.5 * err_lerp.max() and (err_weighted > half_ulp * (1 + 2.0 ** -10)).any()
    assert np.array_equal(M.lerp32(e, e, omd), e)


def test_warmup_sequence():
    for k in range(21):
        assert M.d_k(k, 0.999, True) == (1.0 + k) / (10.0 + k)                     # below the decay all the way
        assert M.d_k(k, 0.999, False) == 0.999
        assert M.d_k(k, 0.5, True) == ((1.0 + k) / (10.0 + k) if k < 8 else 0.5)     # (1 + 8) / (10 + 8) = 0.5: the decay takes over
        for decay in (0.5, 0.999):
            w32, w64 = M.omd32(k, decay, True), 1.0 - M.d_k(k, decay, True)
            assert w32.dtype == np.float32 and abs(float(w32) - w64) <= 2.0 ** -23   # two roundings of values below 1
    assert M.d_k(0, 0.999, True) == 0.1 and float(M.omd32(0, 0.999, True)) == float(np.float32(1) - np.float32(0.1))
    assert M.omd32(3, 0.25, True) == np.float32(0.75)                              # 4 / 13 > 0.25
    assert M.omd32(0, 0.0) == np.float32(1.0)


@pytest.mark.parametrize('warmup', [False, True])
def test_host_mirror_has_the_restatements_bits(warmup):
    from torch_semantic_segmentation_amd import engine as E
    for decay in (0.0, 0.5, 0.999, 0.9999):
        for k in range(21):
            got = E.ema_omd(k, decay, warmup)
            assert got.dtype == np.float32 and got.tobytes() == M.omd32(k, decay, warmup).tobytes()


# ----------------------------------------------------------------------------- host contract (CPU tensors)

def test_model_ema_is_exported_and_rejects():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    assert tssa.ModelEMA is E.ModelEMA
    m = small_module().float()
    for decay in (1.0, -0.1, 1.5, float('nan'), 1.0 - 1e-9):                       # the last one is 1 in float32
        with pytest.raises(ValueError):
            E.ModelEMA(m, decay=decay)
    other = nn.Sequential(nn.Conv2d(3, 4, 3, bias=False), nn.BatchNorm2d(4))        # a key less
    with pytest.raises(ValueError):
        E.ModelEMA(m, module=other)
    wide = nn.Sequential(nn.Conv2d(3, 4, 5, bias=True), nn.BatchNorm2d(4))         # same keys, another shape
    with pytest.raises(ValueError):
        E.ModelEMA(m, module=wide)
    with pytest.raises(ValueError):
        E.ModelEMA(m, module=m)
    with pytest.raises(RuntimeError):                                              # a CPU model: no fallback, as the flat optimizers
        E.ModelEMA(m)
    with pytest.raises(RuntimeError):
        E.ModelEMA(m, optimizer=E.FlatAdamW(m.parameters(), lr=1e-3), module=copy.deepcopy(m))


def test_attach_ema_contract_and_state_dict():
    from torch_semantic_segmentation_amd import engine as E
    ps = [nn.Parameter(torch.randn(7, 5)), nn.Parameter(torch.randn(33))]
    opt = E.FlatAdamW(ps, lr=1e-3)
    plain = opt.state_dict()
    assert 'ema_state' not in plain['flat'] and opt.ema_flat is None
    for bad in (torch.zeros(67), torch.zeros(68, dtype=torch.float64), torch.zeros(136)[::2], opt.flat_param):
        with pytest.raises(ValueError):
            opt.attach_ema(bad, 0.9)
    for decay in (1.0, -1e-3):
        with pytest.raises(ValueError):
            opt.attach_ema(torch.zeros(68), decay)
    assert opt.ema_flat is None
    opt.load_state_dict(plain)                                                      # no average on either side: as before
    assert opt.ema_flat is None and opt.step_count == 0

    ema = opt.flat_param.clone()
    opt.attach_ema(ema, 0.999, warmup=True)
    assert opt.ema_flat is ema and opt.ema_updates == 0
    assert opt.state_dict()['flat']['ema_state'].tolist() == [0.0, 0.0]
    opt.ema_updates = 5                                                             # as after 5 steps
    row = opt.state_dict()['flat']['ema_state']
    assert row.dtype == torch.float32 and row.numpy().tobytes() == np.float32([5.0, M.omd32(4, 0.999, True)]).tobytes()
    sd = opt.state_dict()
    opt.ema_updates = 0
    opt.load_state_dict(sd)
    assert opt.ema_updates == 5
    opt.load_state_dict(plain)                                                      # a checkpoint without the row: the counter stays
    assert opt.ema_updates == 5
    bare = E.FlatAdamW([nn.Parameter(torch.randn(7, 5)), nn.Parameter(torch.randn(33))], lr=1e-3)
    bare.load_state_dict(sd)                                                        # ... and a row without an average is not read
    assert bare.ema_flat is None
    with pytest.raises(RuntimeError):                                               # no CPU fallback, with or without the average
        opt.step()


def test_trainer_takes_an_ema_argument():
    from torch_semantic_segmentation_amd import engine as E
    conv = nn.Conv2d(3, 4, 1)
    tr = E.Trainer(conv, E.FlatSGD(conv.parameters(), lr=0.1), nn.CrossEntropyLoss())
    assert tr.ema is None
