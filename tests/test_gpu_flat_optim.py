"""engine.FlatAdamW / engine.FlatSGD with parameter groups and global-norm clipping (csrc/optim.hip) against the float64 restatement
of torch.optim.AdamW / SGD and clip_grad_norm_ (tests/flatopt_ref.py, held to torch itself by tests/test_flat_optim_oracle.py).

Bounds.  Trajectories: cases.rel_err < 1e-5, the criterion of test_gpu_ops.py::test_flat_adamw_matches_torch_adamw for this kernel
(torch's own float32 run of these cases is ~1e-7 from its float64 run).  Where two runs must agree exactly (a clip that never
engages, identical groups against one group, a repeated run) the comparison is on bits.  The norm: see test_norm_accuracy."""
import functools

import numpy as np
import pytest
import torch
from torch import nn

from oracle.recipe import formula_state, synthetic_batch
from tests import cases, flatopt_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BIG = 2048 * 256 + 5              # the step kernels' grid is capped at 2048 blocks of 256: a second trip for 5 elements

KINDS = {'adamw': None, 'sgd_plain': dict(momentum=0.0, dampening=0.0, nesterov=False),
         'sgd_momentum': dict(momentum=0.9, dampening=0.0, nesterov=False), 'sgd_nesterov': dict(momentum=0.9, dampening=0.0, nesterov=True),
         'sgd_dampening': dict(momentum=0.9, dampening=0.5, nesterov=False)}


@functools.lru_cache(maxsize=None)
def small_case():
    return R.make_case()


@functools.lru_cache(maxsize=None)
def big_case():
    return R.make_case(shapes=((300001,), (BIG - 300001,)), group_sizes=(1, 1), steps=2, big_step=1, seed=12)


def ref_groups(case, kind):
    return R.adamw_groups(case) if kind == 'adamw' else R.sgd_groups(case, **KINDS[kind])


def make_opt(case, kind, ref, max_norm=None, single_group=False):
    """The optimizer over the case's tensors on the device, one group per restatement group (or all tensors in one group with the
    first group's hyper-parameters)."""
    from torch_semantic_segmentation_amd import engine as E
    ps = [nn.Parameter(torch.from_numpy(p).to(DEV)) for p in case['params']]
    keys = ('lr', 'weight_decay', 'betas', 'eps') if kind == 'adamw' else ('lr', 'weight_decay', 'momentum', 'dampening', 'nesterov')
    groups = [dict(params=[ps[i] for i in idx], **{k: g[k] for k in keys}) for idx, g in zip(case['tensor_groups'], ref)]
    if single_group:
        groups = [dict(groups[0], params=ps)]
    opt = E.FlatAdamW(groups, max_grad_norm=max_norm) if kind == 'adamw' else E.FlatSGD(groups, lr=1.0, max_grad_norm=max_norm)
    return opt, ps


def run_hip(case, kind, ref, max_norm=None, grad_scale=1.0, single_group=False):
    opt, ps = make_opt(case, kind, ref, max_norm, single_group)
    opt.grad_scale = grad_scale
    norms = []
    for gs in case['grads']:
        opt.flat_grad.copy_(torch.from_numpy(R.flatten(gs).astype(np.float32)))
        opt.step()
        if max_norm is not None:
            norms.append(opt.last_grad_norm.clone())
    torch.cuda.synchronize()
    return opt, [float(v) for v in norms]


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_grouped_trajectories_match_the_restatement(kind):
    """8 steps, three groups with their own lr / weight_decay; clipping off, max_norm=1e3 (never engages: bit-identical to off) and
    max_norm=5.0 (engages every step: the norms are ~36, ~368 on the x10 step); grad_scale 1 and 1/4."""
    case = small_case()
    got = {}
    for max_norm in (None, 1e3, 5.0):
        want, norms = R.run(case, kind.split('_')[0], ref_groups(case, kind), max_norm=max_norm)
        opt, norms_hip = run_hip(case, kind, ref_groups(case, kind), max_norm)
        got[max_norm] = opt.flat_param.cpu().numpy()
        err = cases.rel_err(got[max_norm], want)
        print(kind, 'max_norm', max_norm, 'rel_err', err)
        assert err < 1e-5, (kind, max_norm, err)
        if max_norm is not None:
            assert cases.rel_err(norms_hip, norms) < 1e-6
    assert got[1e3].tobytes() == got[None].tobytes()
    assert cases.rel_err(got[5.0], got[None]) > 1e-3                      # the clip did engage
    want, _ = R.run(case, kind.split('_')[0], ref_groups(case, kind), max_norm=5.0, grad_scale=0.25)
    opt, _ = run_hip(case, kind, ref_groups(case, kind), 5.0, grad_scale=0.25)
    assert cases.rel_err(opt.flat_param.cpu().numpy(), want) < 1e-5


@pytest.mark.parametrize('kind', ['adamw', 'sgd_dampening'])
@pytest.mark.parametrize('cuts', [(1, 256), (37, 293)])
def test_identical_groups_are_bit_identical_to_one_group(kind, cuts):
    """Group boundaries at element 1, on a block edge (256) and inside a wave (37, 293): three groups with the SAME hyper-parameters
    against the single-group optimizer over the same tensors -- parameters and moments, bit for bit."""
    sizes = (cuts[0], cuts[1] - cuts[0], 1037 - cuts[1])
    case = R.make_case(shapes=tuple((s,) for s in sizes), group_sizes=(1, 1, 1), steps=3, big_step=1, seed=13)
    same = (1e-2,) * 3
    ref = R.adamw_groups(case, lrs=same, wds=same) if kind == 'adamw' else R.sgd_groups(case, lrs=same, wds=same, **KINDS[kind])
    three, _ = run_hip(case, kind, ref)
    one, _ = run_hip(case, kind, ref, single_group=True)
    assert three.group_ranges == [(0, cuts[0]), cuts, (cuts[1], 1037)] and one.group_ranges == [(0, 1037)]
    for name in ('flat_param',) + type(three)._state_names:
        assert getattr(three, name).cpu().numpy().tobytes() == getattr(one, name).cpu().numpy().tobytes(), name
    assert cases.rel_err(three.flat_param.cpu().numpy(), R.flatten(case['params'])) > 1e-3     # it did step


@pytest.mark.parametrize('kind', ['adamw', 'sgd_nesterov'])
def test_grid_stride_second_trip_with_a_group_boundary_at_an_odd_offset(kind):
    case = big_case()
    assert case['ranges'] == [(0, 300001), (300001, BIG)]
    want, _ = R.run(case, kind.split('_')[0], ref_groups(case, kind), max_norm=5.0)
    opt, _ = run_hip(case, kind, ref_groups(case, kind), 5.0)
    got = opt.flat_param.cpu().numpy()
    assert cases.rel_err(got, want) < 1e-5
    assert cases.rel_err(got[-5:], want[-5:]) < 1e-5 and cases.rel_err(got[300000:300002], want[300000:300002]) < 1e-5


def one_norm(grad, grad_scale, max_norm=1.0):
    """(norm, factor, parameters after the step) of a FlatSGD(lr=1) step over `grad` (a float32 numpy vector), parameters zero."""
    from torch_semantic_segmentation_amd import engine as E
    opt = E.FlatSGD([nn.Parameter(torch.zeros(grad.size, device=DEV))], lr=1.0, max_grad_norm=max_norm)
    opt.grad_scale = grad_scale
    opt.flat_grad.copy_(torch.from_numpy(grad))
    before = opt.flat_grad.clone()
    opt.step()
    assert torch.equal(opt.flat_grad.view(torch.int32), before.view(torch.int32))      # the gradient buffer is not rewritten (bits: NaN)
    return opt.last_grad_norm.cpu().numpy(), opt._clip_out[1].cpu().numpy(), opt.flat_param.cpu().numpy()


@pytest.mark.parametrize('grad_scale', [1.0, 0.125])
@pytest.mark.parametrize('n', [1, 255, 257, BIG, 1024 * 4096 + 4099])
def test_norm_accuracy(n, grad_scale):
    """last_grad_norm against the float64 norm: relative error <= 2^-23.  The f64 squares of f32 values are exact (24-bit
    significands, 48-bit products); the f64 sum of n non-negative terms, in any order, errs by at most (n - 1) * 2^-53 relative, so
    the square root and the product with grad_scale stay within a few 2^-53 of the true norm for every n here (n < 2^23); the one
    rounding to f32 adds at most 2^-24.  The sum is 2^-24 and a little, under 2^-23.  The same holds for the clip factor.
    n = 1024 * 4096 + 4099 is past the reduction's block cap (1024 blocks of 4096 elements): its blocks take a second trip."""
    grad = np.random.RandomState(n % 1000).standard_normal(n).astype(np.float32)
    norm, s, _ = one_norm(grad, grad_scale, max_norm=0.5)
    want_norm, want_s = R.clip(grad, grad_scale, 0.5)
    assert norm.dtype == np.float32 and norm.shape == ()
    e_norm, e_s = abs(float(norm) - want_norm) / want_norm, abs(float(s) - want_s) / want_s
    print('n', n, 'grad_scale', grad_scale, 'norm err', e_norm, 'factor err', e_s)
    assert e_norm <= 2.0 ** -23 and e_s <= 2.0 ** -23


def test_norm_edge_cases():
    norm, s, p = one_norm(np.zeros(300, dtype=np.float32), 0.125)
    assert float(norm) == 0.0 and float(s) == 0.125 and not np.isnan(p).any() and (p == 0).all()
    grad = np.ones(300, dtype=np.float32)
    grad[17] = np.inf
    norm, s, p = one_norm(grad, 1.0)
    assert np.isinf(float(norm)) and float(s) == 0.0
    assert np.isnan(p[17]) and (np.delete(p, 17) == 0).all()      # inf * 0, as torch's clip leaves it; the others are scaled by 0
    grad[17] = np.nan
    norm, s, p = one_norm(grad, 1.0)
    assert np.isnan(float(norm)) and np.isnan(float(s)) and np.isnan(p).all()      # a non-finite norm propagates: no skip logic
    norm, s, _ = one_norm(np.full(4, 0.25, dtype=np.float32), 0.125, max_norm=1e3)     # not engaged: the factor IS grad_scale
    assert float(s) == 0.125 and float(norm) == 0.0625


@pytest.mark.parametrize('kind', ['adamw', 'sgd_momentum'])
def test_clipped_step_is_deterministic(kind):
    case = big_case()
    runs = []
    for _ in range(2):
        opt, _ = run_hip(case, kind, ref_groups(case, kind), 5.0)
        runs.append((opt.flat_param.cpu().numpy().tobytes(), opt.last_grad_norm.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]


@pytest.mark.parametrize('kind', ['adamw', 'sgd_momentum'])
def test_device_state_step_replays_from_a_captured_graph(kind):
    """Two groups, device_state=True: step() captured once (tick kernel + step kernel, clip included), replayed 3 times with both
    learning rates changed between the replays through param_groups + sync_lr()."""
    case = R.make_case(shapes=((300,), (41,), (700,)), group_sizes=(2, 1), steps=3, big_step=1, seed=14)
    ref = ref_groups(case, kind)[:2]
    opt, _ = make_opt(case, kind, ref, max_norm=5.0)
    opt.device_state = True
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for k, gs in enumerate(case['grads']):
        for g in opt.param_groups:
            g['lr'] = g['lr'] * 0.5 if k else g['lr']
        opt.sync_lr()
        opt.flat_grad.copy_(torch.from_numpy(R.flatten(gs).astype(np.float32)))
        graph.replay()
    torch.cuda.synchronize()

    def halve(k, groups):
        for g in groups:
            g['lr'] = g['lr'] * 0.5 if k else g['lr']
    want, norms = R.run(case, kind.split('_')[0], ref, max_norm=5.0, lr_schedule=halve)
    assert cases.rel_err(opt.flat_param.cpu().numpy(), want) < 1e-5
    assert opt.state_vec.cpu().numpy().reshape(2, 3)[:, 0].tolist() == [3.0, 3.0]
    assert abs(float(opt.last_grad_norm) - norms[-1]) <= 1e-6 * norms[-1]


# ----------------------------------------------------------------------------- under the trainer

def fastscnn_groups(m):
    """BatchNorm and bias parameters in a weight_decay=0 group, as segmentation recipes do."""
    no_decay = [p for p in m.parameters() if p.dim() == 1]
    decay = [p for p in m.parameters() if p.dim() != 1]
    assert no_decay and decay
    return [dict(params=decay), dict(params=no_decay, weight_decay=0.0)]


def trainer_run(make_optimizer, use_graph=False, stock_clip=None, steps=3):
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    x, y = synthetic_batch(2, 64, 128)
    x, y = x.to(DEV), y.to(DEV)
    m = cases.product_model('fastscnn')
    m.load_state_dict(formula_state(m), strict=True)
    cases.zero_dropout(m)
    m.to(DEV)
    opt = make_optimizer(fastscnn_groups(m))
    tr = E.Trainer(m, opt, tssa.CrossEntropyLoss(ignore_index=255), use_graph=use_graph, fuse_head_loss=False)
    losses, norms = [], []
    for _ in range(steps):
        if stock_clip is None:
            losses.append(tr.step_async(x, y).item())
            norms.append(float(opt.last_grad_norm))
        else:       # the stock recipe: backward, clip_grad_norm_ over the parameter views, torch's own step
            losses.append(tr._forward_backward(x, y).item())
            norms.append(float(torch.nn.utils.clip_grad_norm_(m.parameters(), stock_clip)))
            opt.step()
    assert bool(tr._graphs) == use_graph
    return losses, torch.cat([p.detach().flatten() for p in m.parameters()]).double().cpu(), norms


@functools.lru_cache(maxsize=None)
def first_step_norm():
    from torch_semantic_segmentation_amd import engine as E
    norm = trainer_run(lambda gs: E.FlatAdamW(gs, lr=1e-3, weight_decay=1e-5, max_grad_norm=1e30), steps=1)[2][0]
    assert np.isfinite(norm) and norm > 0
    return norm


def close(a, b):
    assert np.allclose(a[0], b[0], rtol=1e-3), (a[0], b[0])
    err = ((a[1] - b[1]).norm() / b[1].norm()).item()
    assert err < 2e-3, err                # the bounds of test_flat_adamw_and_graph_replay_match_eager for the same comparison


def test_trainer_grouped_clipped_adamw_eager_graph_and_stock():
    """fastscnn at 2 x 3 x 64 x 128, two groups, max_grad_norm = half the first step's norm (so the clip engages): 3 steps eagerly,
    from a captured graph, and with torch.optim.AdamW(groups) + clip_grad_norm_ on the same model."""
    from torch_semantic_segmentation_amd import engine as E
    clip = 0.5 * first_step_norm()
    eager = trainer_run(lambda gs: E.FlatAdamW(gs, lr=1e-3, weight_decay=1e-5, max_grad_norm=clip))
    graph = trainer_run(lambda gs: E.FlatAdamW(gs, lr=1e-3, weight_decay=1e-5, max_grad_norm=clip), use_graph=True)
    stock = trainer_run(lambda gs: torch.optim.AdamW(gs, lr=1e-3, weight_decay=1e-5), stock_clip=clip)
    for run in (eager, graph, stock):         # the first step's norm is the measured one, twice the bound: the clip engages
        assert run[2][0] == pytest.approx(first_step_norm(), rel=1e-3) and all(np.isfinite(run[2]))
    close(graph, eager)
    close(eager, stock)


def test_trainer_grouped_clipped_nesterov_sgd_eager_and_graph():
    from torch_semantic_segmentation_amd import engine as E
    clip = 0.5 * first_step_norm()
    make = lambda gs: E.FlatSGD(gs, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-5, max_grad_norm=clip)   # noqa: E731
    eager = trainer_run(make)
    graph = trainer_run(make, use_graph=True)
    assert eager[2][0] == pytest.approx(first_step_norm(), rel=1e-3) and all(np.isfinite(eager[0]))
    close(graph, eager)
