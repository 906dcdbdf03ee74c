"""The checker of the flat-optimizer tests (tests/flatopt_ref.py) against torch.optim.AdamW / torch.optim.SGD and
torch.nn.utils.clip_grad_norm_ in float64, and the host-side contract of engine.FlatAdamW / engine.FlatSGD on CPU tensors (layout,
aliasing, parameter groups, schedulers, state_dict, errors).  CPU only: nothing here launches a kernel."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import cases, flatopt_ref as R

SGD_VARIANTS = {'plain': dict(momentum=0.0, dampening=0.0, nesterov=False), 'momentum': dict(momentum=0.9, dampening=0.0, nesterov=False),
                'nesterov': dict(momentum=0.9, dampening=0.0, nesterov=True), 'dampening': dict(momentum=0.9, dampening=0.5, nesterov=False)}


def torch_run(case, make_opt, max_norm):
    ps = [nn.Parameter(torch.from_numpy(p).double()) for p in case['params']]
    groups = [[ps[i] for i in idx] for idx in case['tensor_groups']]
    opt = make_opt(groups)
    norms = []
    for gs in case['grads']:
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g).double()
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
        opt.step()
    return R.flatten([p.detach().numpy() for p in ps]), norms


@pytest.mark.parametrize('max_norm', [None, 5.0])
def test_adamw_restatement_is_torch_adamw_in_float64(max_norm):
    """Both sides float64, only the operation order differs: 1e-12."""
    case = R.make_case()
    want, norms_t = torch_run(case, lambda gs: torch.optim.AdamW(
        [dict(params=g, lr=lr, weight_decay=wd) for g, lr, wd in zip(gs, R.GROUP_LR, R.GROUP_WD)], lr=1.0), max_norm)
    got, norms = R.run(case, 'adamw', R.adamw_groups(case), max_norm=max_norm)
    assert cases.rel_err(got, want) < 1e-12
    if max_norm is not None:
        assert cases.rel_err(norms, norms_t) < 1e-12
        assert all(35.0 < v < 38.5 for i, v in enumerate(norms) if i != R.BIG_STEP) and 350.0 < norms[R.BIG_STEP] < 385.0


@pytest.mark.parametrize('variant', sorted(SGD_VARIANTS))
@pytest.mark.parametrize('max_norm', [None, 5.0])
def test_sgd_restatement_is_torch_sgd_in_float64(variant, max_norm):
    case = R.make_case()
    kw = SGD_VARIANTS[variant]
    want, _ = torch_run(case, lambda gs: torch.optim.SGD(
        [dict(params=g, lr=lr, weight_decay=wd) for g, lr, wd in zip(gs, R.GROUP_LR, R.GROUP_WD)], lr=1.0, **kw), max_norm)
    got, _ = R.run(case, 'sgd', R.sgd_groups(case, **kw), max_norm=max_norm)
    assert cases.rel_err(got, want) < 1e-12


def test_clip_formula_edge_cases():
    assert R.clip(np.zeros(5), 0.125, 5.0) == (0.0, 0.125)               # nothing to clip: the factor is grad_scale itself
    assert R.clip(np.ones(4), 0.5, 1e3) == (1.0, 0.5)
    norm, s = R.clip(np.array([3.0, 4.0]), 1.0, 1.0)
    assert norm == 5.0 and abs(s - 1.0 / (5.0 + 1e-6)) < 1e-15
    norm, s = R.clip(np.array([1.0, np.inf]), 1.0, 1.0)
    assert norm == np.inf and s == 0.0


# ----------------------------------------------------------------------------- host contract (CPU tensors)

def three_groups():
    torch.manual_seed(0)
    ps = [nn.Parameter(torch.randn(*s)) for s in R.SHAPES]
    return ps, [dict(params=ps[0:2]), dict(params=ps[2:4], lr=3e-3, weight_decay=0.0), dict(params=ps[4:6], betas=(0.8, 0.99), eps=1e-6)]


def test_flat_sgd_exists_and_is_exported():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E
    assert issubclass(E.FlatSGD, E.FlatOptimizer) and issubclass(E.FlatAdamW, E.FlatOptimizer)
    assert issubclass(E.FlatOptimizer, torch.optim.Optimizer)
    assert tssa.FlatSGD is E.FlatSGD and tssa.FlatAdamW is E.FlatAdamW
    assert E.Trainer(nn.Conv2d(3, 4, 1), E.FlatSGD(nn.Conv2d(3, 4, 1).parameters(), lr=0.1), nn.CrossEntropyLoss()).flat


def test_three_groups_layout_aliasing_and_reattach():
    from torch_semantic_segmentation_amd import engine as E
    ps, groups = three_groups()
    before = [p.detach().clone() for p in ps]
    opt = E.FlatAdamW(groups, lr=1e-2, weight_decay=1e-2)
    sizes = [p.numel() for p in ps]
    assert opt.flat_param.numel() == sum(sizes) == opt.flat_grad.numel() == 1354
    assert opt.group_ranges == [(0, 68), (68, 326), (326, 1354)]
    off = 0
    for p, b in zip(ps, before):
        assert torch.equal(p.detach(), b)
        assert p.data_ptr() == opt.flat_param.data_ptr() + 4 * off and p.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * off
        off += p.numel()
    # torch's defaulting rules: what a group leaves out comes from the constructor
    g0, g1, g2 = opt.param_groups
    assert (g0['lr'], g0['weight_decay'], g0['betas'], g0['eps']) == (1e-2, 1e-2, (0.9, 0.999), 1e-8)
    assert (g1['lr'], g1['weight_decay']) == (3e-3, 0.0) and g2['betas'] == (0.8, 0.99) and g2['eps'] == 1e-6
    opt.flat_grad.fill_(2.0)
    assert all(torch.equal(p.grad, torch.full_like(p, 2.0)) for p in ps)
    opt._check_aliases()
    ps[3].grad = None
    with pytest.raises(RuntimeError, match='no longer aliases'):
        opt._check_aliases()
    opt.reattach()
    opt._check_aliases()
    assert ps[3].grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * sum(sizes[:3])
    with pytest.raises(RuntimeError, match='HIP path only'):
        opt.step()
    assert opt.last_grad_norm is None and E.FlatAdamW([nn.Parameter(torch.zeros(3))], max_grad_norm=1.0).last_grad_norm.dim() == 0


def test_single_tensor_iterable_is_one_group_in_the_old_layout():
    from torch_semantic_segmentation_amd import engine as E
    m = nn.Sequential(nn.Conv2d(3, 4, 1), nn.BatchNorm2d(4))
    opt = E.FlatSGD(m.parameters(), lr=0.1, momentum=0.9)
    assert len(opt.param_groups) == 1 and opt.group_ranges == [(0, 24)] and opt.momentum_buffer.numel() == 24
    assert E.FlatSGD(nn.Conv2d(3, 4, 1).parameters(), lr=0.1).momentum_buffer is None        # momentum 0 needs no buffer
    assert torch.equal(opt.flat_param[:12], m[0].weight.detach().flatten())


@pytest.mark.filterwarnings('ignore:Detected call of `lr_scheduler.step')      # no step() without a GPU: only the rates are checked
def test_a_scheduler_changes_one_groups_learning_rate():
    from torch_semantic_segmentation_amd import engine as E
    _, groups = three_groups()
    opt = E.FlatSGD([dict(params=g['params']) for g in groups[:2]] + [dict(params=groups[2]['params'], lr=1.0)], lr=0.1, momentum=0.9)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, [lambda e: 1.0, lambda e: 0.5 ** e, lambda e: 1.0])
    for _ in range(2):
        sched.step()
    assert [g['lr'] for g in opt.param_groups] == [0.1, 0.025, 1.0] and all(type(g['lr']) is float for g in opt.param_groups)
    poly = torch.optim.lr_scheduler.PolynomialLR(E.FlatAdamW(three_groups()[1], lr=1e-2), total_iters=4, power=0.9)
    poly.step()
    assert abs(poly.optimizer.param_groups[1]['lr'] - 3e-3 * 0.75 ** 0.9) < 1e-12


@pytest.mark.parametrize('kind', ['adamw', 'sgd'])
def test_state_dict_round_trip_and_mismatched_ranges(kind):
    from torch_semantic_segmentation_amd import engine as E

    def make(split=2):
        ps, _ = three_groups()
        groups = [dict(params=ps[:split]), dict(params=ps[split:], lr=0.5)]
        return E.FlatAdamW(groups, lr=1e-3) if kind == 'adamw' else E.FlatSGD(groups, lr=1e-3, momentum=0.9)
    opt = make()
    names = ('exp_avg', 'exp_avg_sq') if kind == 'adamw' else ('momentum_buffer',)
    for i, n in enumerate(names):
        getattr(opt, n).copy_(torch.arange(1354.0) + i)
    opt.step_count = 3
    opt.param_groups[1]['lr'] = 0.25
    sd = opt.state_dict()
    assert sd['flat']['group_ranges'] == [[0, 68], [68, 1354]] and set(names) < set(sd['flat'])
    assert sd['flat']['state_vec'].shape == (6,) and float(sd['flat']['state_vec'][3]) == 3.0
    opt2 = make()
    opt2.load_state_dict(sd)
    assert all(torch.equal(getattr(opt2, n), getattr(opt, n)) for n in names)
    assert opt2.step_count == 3 and opt2.param_groups[1]['lr'] == 0.25 and torch.equal(opt2.state_vec, sd['flat']['state_vec'])
    with pytest.raises(ValueError, match='lays its parameter groups out'):
        make(split=3).load_state_dict(sd)


def test_a_checkpoint_of_the_single_group_optimizer_still_loads():
    """The dict FlatAdamW.state_dict() wrote before parameter groups existed: no ranges, a [3] state row."""
    from torch_semantic_segmentation_amd import engine as E
    new = lambda: E.FlatAdamW(nn.Sequential(nn.Conv2d(3, 4, 1), nn.BatchNorm2d(4)).parameters(), lr=1e-3)   # noqa: E731
    opt = new()
    old = {'state': {}, 'param_groups': [{'lr': 5e-4, 'betas': (0.9, 0.999), 'eps': 1e-8, 'weight_decay': 1e-2, 'params': list(range(4))}],
           'flat': {'exp_avg': torch.full((24,), 0.5), 'exp_avg_sq': torch.full((24,), 0.25),
                    'state_vec': torch.tensor([3.0, 1 - 0.9 ** 3, (1 - 0.999 ** 3) ** 0.5])}}
    opt.load_state_dict(old)
    assert opt.step_count == 3 and opt.param_groups[0]['lr'] == 5e-4
    assert float(opt.exp_avg.mean()) == 0.5 and float(opt.exp_avg_sq.mean()) == 0.25
    old['flat']['exp_avg'] = torch.zeros(23)
    with pytest.raises(ValueError, match='lays its parameter groups out'):
        new().load_state_dict(old)


def test_errors():
    from torch_semantic_segmentation_amd import engine as E
    P = lambda: nn.Parameter(torch.zeros(3))   # noqa: E731
    for cls, kw in ((E.FlatAdamW, {}), (E.FlatSGD, {'lr': 0.1})):
        with pytest.raises(ValueError, match='at most 8 parameter groups'):
            cls([dict(params=[P()]) for _ in range(9)], **kw)
        assert len(cls([dict(params=[P()]) for _ in range(8)], **kw).param_groups) == 8
        with pytest.raises(ValueError, match='empty parameter group'):
            cls([dict(params=[P()]), dict(params=[])], **kw)
        for flag in ('maximize', 'foreach', 'fused') + (('amsgrad',) if cls is E.FlatAdamW else ()):
            with pytest.raises(ValueError, match=flag):
                cls([P()], **{flag: True}, **kw)
            with pytest.raises(ValueError, match=flag):
                cls([{'params': [P()], flag: True}], **kw)
            cls([P()], **{flag: False}, **kw)
        opt = cls([P()], **kw)
        with pytest.raises(NotImplementedError, match='laid out once'):
            opt.add_param_group({'params': [P()]})
    with pytest.raises(ValueError, match='Nesterov momentum requires a momentum and zero dampening'):
        E.FlatSGD([P()], lr=0.1, nesterov=True)
    with pytest.raises(ValueError, match='Nesterov momentum requires a momentum and zero dampening'):
        E.FlatSGD([P()], lr=0.1, momentum=0.9, dampening=0.5, nesterov=True)
    with pytest.raises(ValueError, match='Nesterov momentum requires a momentum and zero dampening'):
        E.FlatSGD([dict(params=[P()]), dict(params=[P()], dampening=0.1)], lr=0.1, momentum=0.9, nesterov=True)
    assert E.FlatSGD([P()], lr=0.1, momentum=0.9, nesterov=True).param_groups[0]['nesterov'] is True


def test_header_still_parses_and_declares_the_new_entries():
    from torch_semantic_segmentation_amd import _native as N
    decls = N.parse_header()
    import ctypes
    P, L, I, F = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_float
    assert decls['tss_adamw_step_groups'] == (I, [P, P, P, P, L, P, I, P, P, P, F, L, P])
    assert decls['tss_sgd_step_groups'] == (I, [P, P, P, L, P, I, P, P, P, F, L, P])
    assert decls['tss_grad_sqnorm'] == (I, [P, L, P, F, F, P, P]) and decls['tss_grad_sqnorm_workspace_bytes'] == (L, [L])
    assert decls['tss_adamw_step'] == (I, [P, P, P, P, L, P, F, F, F, F, P, F, F, L, P])          # unchanged
    from torch_semantic_segmentation_amd.engine import _OptGroup
    assert ctypes.sizeof(_OptGroup) == 40
