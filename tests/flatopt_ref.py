"""float64 numpy restatement of what engine.FlatAdamW / engine.FlatSGD compute on their flat buffers: torch.optim.AdamW and
torch.optim.SGD per element with per-group hyper-parameters, and the factor of torch.nn.utils.clip_grad_norm_ folded into the
gradient.  tests/test_flat_optim_oracle.py holds it to torch itself (float64, 1e-12); the GPU tests compare the kernels with it.

A group is a dict: begin, end (its range of the flat vectors) plus lr, weight_decay and, for AdamW, betas, eps; for SGD, momentum,
dampening, nesterov.
"""
import numpy as np

SHAPES = ((7, 5), (33,), (1,), (257,), (1025,), (3,))        # the parameter tensors of the trajectory cases, in flat order
GROUP_SIZES = (2, 2, 2)                                      # tensors per group
GROUP_LR = (1e-2, 3e-3, 1e-1)
GROUP_WD = (1e-2, 0.0, 1e-3)
STEPS = 8
BIG_STEP = 5                                                 # 0-based: this step's gradients are x10


def clip(grad, grad_scale, max_norm):
    """(norm, s): norm = grad_scale * ||grad||_2, s = grad_scale * min(1, max_norm / (norm + 1e-6)); max_norm None: s = grad_scale."""
    g = np.asarray(grad, dtype=np.float64)
    norm = float(grad_scale) * float(np.sqrt(np.sum(g * g)))
    if max_norm is None:
        return norm, float(grad_scale)
    coef = float(max_norm) / (norm + 1e-6)
    if coef > 1.0:
        coef = 1.0
    return norm, float(grad_scale) * coef


def adamw_step(p, g, m, v, groups, step, s=1.0):
    """One torch.optim.AdamW step (step is 1-based) on the flat float64 vectors p, m, v, in place; g is scaled by s."""
    for gr in groups:
        sl = slice(gr['begin'], gr['end'])
        b1, b2 = gr['betas']
        gi = g[sl] * s
        p[sl] *= 1.0 - gr['lr'] * gr['weight_decay']
        m[sl] += (gi - m[sl]) * (1.0 - b1)
        v[sl] = v[sl] * b2 + (1.0 - b2) * gi * gi
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        p[sl] -= (gr['lr'] / bc1) * (m[sl] / (np.sqrt(v[sl]) / np.sqrt(bc2) + gr['eps']))


def sgd_step(p, g, buf, groups, step, s=1.0):
    """One torch.optim.SGD step (step is 1-based) on the flat float64 vectors p, buf, in place; g is scaled by s."""
    for gr in groups:
        sl = slice(gr['begin'], gr['end'])
        gi = g[sl] * s
        if gr['weight_decay'] != 0:
            gi = gi + gr['weight_decay'] * p[sl]
        mu = gr['momentum']
        if mu != 0:
            buf[sl] = gi if step == 1 else mu * buf[sl] + (1.0 - gr['dampening']) * gi
            gi = gi + mu * buf[sl] if gr['nesterov'] else buf[sl]
        p[sl] -= gr['lr'] * gi


def make_case(shapes=SHAPES, group_sizes=GROUP_SIZES, steps=STEPS, big_step=BIG_STEP, seed=11):
    """Initial parameters and per-step gradients (float32 values), and the group ranges.  Returns a dict:
    params: [array per tensor], grads: [steps][array per tensor], tensor_groups: [[tensor index ...] per group], ranges: [(b, e)]."""
    rng = np.random.RandomState(seed)
    params = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    grads = []
    for k in range(steps):
        f = 10.0 if k == big_step else 1.0
        grads.append([(f * rng.standard_normal(s)).astype(np.float32) for s in shapes])
    tensor_groups, ranges, t, off = [], [], 0, 0
    for n in group_sizes:
        idx = list(range(t, t + n))
        size = sum(int(np.prod(shapes[i])) for i in idx)
        tensor_groups.append(idx)
        ranges.append((off, off + size))
        t, off = t + n, off + size
    assert t == len(shapes)
    return {'params': params, 'grads': grads, 'tensor_groups': tensor_groups, 'ranges': ranges}


def adamw_groups(case, lrs=GROUP_LR, wds=GROUP_WD, betas=(0.9, 0.999), eps=1e-8):
    return [dict(begin=b, end=e, lr=lr, weight_decay=wd, betas=betas, eps=eps) for (b, e), lr, wd in zip(case['ranges'], lrs, wds)]


def sgd_groups(case, momentum=0.0, dampening=0.0, nesterov=False, lrs=GROUP_LR, wds=GROUP_WD):
    return [dict(begin=b, end=e, lr=lr, weight_decay=wd, momentum=momentum, dampening=dampening, nesterov=nesterov)
            for (b, e), lr, wd in zip(case['ranges'], lrs, wds)]


def flatten(tensors):
    return np.concatenate([np.asarray(t, dtype=np.float64).reshape(-1) for t in tensors])


def run(case, kind, groups, max_norm=None, grad_scale=1.0, lr_schedule=None):
    """The whole trajectory: (final flat float64 parameters, [pre-clip norm per step]).  kind: 'adamw' | 'sgd'.
    lr_schedule(step0, groups): optional, changes the groups' lr in place before step step0 (0-based)."""
    p = flatten(case['params'])
    a, b = np.zeros_like(p), np.zeros_like(p)
    norms = []
    for k, gs in enumerate(case['grads']):
        if lr_schedule is not None:
            lr_schedule(k, groups)
        g = flatten(gs)
        norm, s = clip(g, grad_scale, max_norm)
        norms.append(norm)
        if kind == 'adamw':
            adamw_step(p, g, a, b, groups, k + 1, s)
        else:
            sgd_step(p, g, a, groups, k + 1, s)
    return p, norms
