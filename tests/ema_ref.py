"""Restatements of the weight average of engine.ModelEMA / FlatOptimizer.attach_ema (csrc/optim.hip):

    e' = e + (p - e) * (1 - d_k),    d_k = decay, or warming up  min(decay, (1 + k) / (10 + k)),    k = 0, 1, ... updates done before

* float64 (d_k, step64, run): what the GPU trajectories are compared with; tests/test_ema_oracle.py holds it to
  torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=True) in float64.
* float32 (omd32, lerp32): the kernel's own arithmetic, every operation rounded on its own -- the factor 1 - d_k, then t = p - e,
  u = t * omd, e' = e + u.  The GPU results are compared with it bit for bit.
"""
import numpy as np

from tests import flatopt_ref as R


def d_k(k, decay, warmup=False):
    """The decay of update number k (0-based), float64."""
    return min(float(decay), (1.0 + k) / (10.0 + k)) if warmup else float(decay)


def step64(e, p, k, decay, warmup=False):
    e = np.asarray(e, dtype=np.float64)
    return e + (np.asarray(p, dtype=np.float64) - e) * (1.0 - d_k(k, decay, warmup))


def omd32(k, decay, warmup=False):
    """1 - d_k with every operation in float32 (the division included)."""
    one, d = np.float32(1.0), np.float32(decay)
    if warmup:
        d = min(d, (one + np.float32(k)) / (np.float32(10.0) + np.float32(k)))
    return np.float32(one - d)


def lerp32(e, p, omd):
    """The three roundings: numpy float32 arrays in, float32 array out."""
    e, p, omd = np.asarray(e), np.asarray(p), np.float32(omd)
    assert e.dtype == np.float32 and p.dtype == np.float32
    t = (p - e).astype(np.float32)
    u = (t * omd).astype(np.float32)
    return (e + u).astype(np.float32)


def ulps32(a, b):
    """Distance of two positive float32 values in units of the last place."""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def run(case, kind, groups, decay, warmup=False, max_norm=None, grad_scale=1.0):
    """flatopt_ref.run with the average updated after every step: (final parameters, final average, [parameters after each step,
    the initial ones first]), float64.  The average starts as a copy of the initial parameters."""
    p = R.flatten(case['params'])
    e = p.copy()
    a, b = np.zeros_like(p), np.zeros_like(p)
    history = [p.copy()]
    for k, gs in enumerate(case['grads']):
        g = R.flatten(gs)
        _, s = R.clip(g, grad_scale, max_norm)
        if kind == 'adamw':
            R.adamw_step(p, g, a, b, groups, k + 1, s)
        else:
            R.sgd_step(p, g, a, groups, k + 1, s)
        e = step64(e, p, k, decay, warmup)
        history.append(p.copy())
    return p, e, history
