"""numpy float32 emulations of the soft-loss and distillation kernels, one f32 operation per numpy operation in the kernel's order
(tests/test_exact_bounds.py holds them to the bounds of tests/exact.py, section "soft losses and distillation", and shows that each
with ONE injected defect fails them).  What is not IEEE is restated as the bounds take it:
  expf     __expf as the compiler emits it: V_EXP_F32(fl(a LOG2E)); the exponential itself is the correctly rounded one here (within the
           1 ulp the bounds grant the hardware), results below the smallest normal f32 are flushed to 0
  logf     the correctly rounded logarithm
  fma      a b + c with the product exact in f64 and the sum rounded to f64, then to f32 (a double rounding: half an f64 ulp from the
           single one)
The emulations are not claimed to give the kernels' bits; they give A legitimate f32 evaluation in the kernels' order."""
import numpy as np

from tests import exact as X

F32 = np.float32
F64 = np.float64
LOG2E = F32(1.4426950408889634)          # 0x3fb8aa3b


def expf(a):
    with np.errstate(under='ignore', over='ignore'):
        r = np.exp2((F32(a) * LOG2E).astype(F64)).astype(F32)
    return np.where(r < F32(2.0 ** -126), F32(0), r)


def logf(x):
    with np.errstate(divide='ignore'):
        return np.log(x.astype(F64)).astype(F32)


def fma(a, b, c):
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


def to_bf16(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=F32)).to(torch.bfloat16).float().numpy()


# ----------------------------------------------------------------------------------------------------------- csrc/distill.hip
DISTILL_DEFECTS = ('own_max', 'drop_tail', 'fused_stats')


def _unit_kl(a, zs, zt, ms, mt):
    """a / zt + (ms - mt) + logf(zs / zt), and the row (ms, logf(zs), mt, logf(zt))"""
    return a / zt + (ms - mt) + logf(zs / zt), np.stack([ms, logf(zs), mt, logf(zt)], -1)


def distill_pixel_fwd(s, t, tau):
    """distill_pixel_fwd_kernel + finalize on s, t [B][HW][C]: (loss f32, stats [P][4] f32).  The f64 block sums are one f64 sum"""
    B, HW, C = s.shape
    s, t = s.reshape(-1, C).astype(F32), t.reshape(-1, C).astype(F32)
    inv = F32(1.0) / F32(tau)
    ms, mt = s.max(1) * inv, t.max(1) * inv
    zs, zt, a = (np.zeros(len(s), F32) for _ in range(3))
    for c in range(C):
        es, et = expf(fma(s[:, c], inv, -ms)), expf(fma(t[:, c], inv, -mt))
        d = (t[:, c] - s[:, c]) * inv
        zs, zt, a = zs + es, zt + et, fma(et, d, a)
    kl, stats = _unit_kl(a, zs, zt, ms, mt)
    norm = F64(F32(tau)) * F64(F32(tau)) / F64(len(s))
    return F32(norm * kl.astype(F64).sum()), stats


def _slot_tree(red, ppb):
    """slot_reduce<., false>: red [ppb][...] summed over the position slots in the kernel's fixed tree"""
    half = 1
    while half < ppb:
        half <<= 1
    half >>= 1
    while half > 0:
        n = min(half, ppb - half)
        red[:n] = red[:n] + red[half:half + n]
        half >>= 1
    return red[0]


def distill_channel_fwd(s, t, tau, max_blocks=0, defect=None):
    """distill_channel_{max,sum,finalize}_kernel on s, t [B][HW][C]: (loss f32, stats [B C][4] f32).  Defects:
      own_max     the last segment of a plane sums against its own partial maxima instead of the plane's
      drop_tail   the last position of every plane (i1 - 1 of the last segment) is left out of the sums"""
    B, HW, C = s.shape
    s, t = s.astype(F32), t.astype(F32)
    sp = X.distill_channel_split(B, C, HW, max_blocks)
    ppb, S = sp['ppb'], sp['S']
    segs = X.distill_segments(HW, S)
    inv = F32(1.0) / F32(tau)
    stats = np.zeros((B, C, 4), F32)
    kls = np.zeros((B, C), F32)
    for b in range(B):
        ms, mt = s[b].max(0) * inv, t[b].max(0) * inv                    # plane_max: exact maxima in any order, times 1 / tau
        zs, zt, a = (np.zeros(C, F32) for _ in range(3))
        for q, (i0, i1) in enumerate(segs):
            last = q == S - 1
            if defect == 'drop_tail' and last:
                i1 -= 1
            us, ut = ms, mt
            if defect == 'own_max' and last and i1 > i0:
                us, ut = s[b, i0:i1].max(0) * inv, t[b, i0:i1].max(0) * inv
            n = max(i1 - i0, 0)
            trips = X.cdiv(n, ppb)
            acc = np.zeros((3, ppb, C), F32)
            for k in range(trips):
                lo, hi = i0 + k * ppb, min(i0 + (k + 1) * ppb, i1)
                vs, vt = s[b, lo:hi], t[b, lo:hi]
                et = expf(fma(vt, inv, -ut))
                m = hi - lo
                acc[0, :m] = acc[0, :m] + expf(fma(vs, inv, -us))
                acc[1, :m] = acc[1, :m] + et
                acc[2, :m] = fma(et, (vt - vs) * inv, acc[2, :m])
            zs, zt, a = zs + _slot_tree(acc[0], ppb), zt + _slot_tree(acc[1], ppb), a + _slot_tree(acc[2], ppb)
        kls[b], stats[b] = _unit_kl(a, zs, zt, ms, mt)
    norm = F64(F32(tau)) * F64(F32(tau)) / F64(B * C)
    return F32(norm * kls.astype(F64).sum()), stats.reshape(B * C, 4)


def distill_bwd(s, t, stats, tau, kind, grad_out=1.0, bf16=False, defect=None):
    """distill_bwd_kernel: d [B][HW][C].  Defect fused_stats: the backward reads m + log Z saved as ONE float per softmax"""
    B, HW, C = s.shape
    s, t = s.astype(F32), t.astype(F32)
    st = stats.reshape(B, HW, 1, 4) if kind == 'pixel' else stats.reshape(B, 1, C, 4)
    inv = F32(1.0) / F32(tau)
    norm = F32(F64(F32(tau)) / F64(B * HW if kind == 'pixel' else B * C))
    if defect == 'fused_stats':
        q = expf(fma(s, inv, -(st[..., 0] + st[..., 1])))
        p = expf(fma(t, inv, -(st[..., 2] + st[..., 3])))
    else:
        q = expf(fma(s, inv, -st[..., 0]) - st[..., 1])
        p = expf(fma(t, inv, -st[..., 2]) - st[..., 3])
    d = F32(grad_out) * (norm * (q - p))
    return to_bf16(d) if bf16 else d


def distill(s, t, tau, kind, max_blocks=0, grad_out=1.0, bf16=False, defect=None):
    """forward + backward: (loss, stats, d)"""
    if kind == 'pixel':
        loss, stats = distill_pixel_fwd(s, t, tau)
    else:
        loss, stats = distill_channel_fwd(s, t, tau, max_blocks, defect)
    return loss, stats, distill_bwd(s, t, stats, tau, kind, grad_out, bf16, defect)


# ----------------------------------------------------------------------------------------------------------- csrc/softloss.hip
LN2 = F32(0.6931471805599453)            # 0x3f317218
FOCAL_DEFECTS = ('q_one_minus_p', 'no_log1p', 'no_second_term')
DICE_DEFECTS = ('skip_last_group',)


def hw_log2f(x):
    with np.errstate(divide='ignore'):
        return np.log2(np.asarray(x, F32).astype(F64)).astype(F32)


def hw_logf(x):
    """__logf: V_LOG_F32(x) LN2"""
    return hw_log2f(x) * LN2


def exp2f(x):
    return np.exp2(np.asarray(x, F32).astype(F64)).astype(F32)


def log1pf(x):
    return np.log1p(np.asarray(x, F32).astype(F64)).astype(F32)


def _labels(labels, C, ignore_index, has_ignore):
    """lsw::load_labels: the class of a pixel that counts, a negative number for every other one"""
    ok = (labels >= 0) & (labels < C)
    if has_ignore:
        ok &= labels != ignore_index
    return np.where(ok, labels, -1)


def lse8(x):
    """lsw::lse8 on x [B][C][HW] f32: the online log-sum-exp, class by class"""
    B, C, HW = x.shape
    m, s = np.full((B, HW), -np.inf, F32), np.zeros((B, HW), F32)
    for c in range(C):
        v = x[:, c]
        mn = np.maximum(m, v)
        with np.errstate(invalid='ignore'):
            s = s * expf(m - mn) + expf(v - mn)
        m = mn
    return m + hw_logf(s)


def focal_fwd(x, labels, gamma, variant, alpha, ignore_index=255, has_ignore=True, defect=None):
    """focal_fwd_kernel + focal_finalize_kernel: (lse [B][HW], pixel_coef [B][HW], loss, scale).  Defects:
      q_one_minus_p    q = 1 - p instead of so / s
      no_log1p         the et == 1.f branch dropped: __logf(s) always
      no_second_term   coef = -w"""
    x = x.astype(F32)
    B, C, HW = x.shape
    tv = _labels(labels, C, ignore_index, has_ignore)
    gamma = F32(gamma)
    m, so, xt = np.full((B, HW), -np.inf, F32), np.zeros((B, HW), F32), np.zeros((B, HW), F32)
    for c in range(C):
        v = x[:, c]
        mn = np.maximum(m, v)
        is_ = tv == c
        with np.errstate(invalid='ignore'):
            so = so * expf(m - mn) + np.where(is_, F32(0), expf(v - mn))
        m = mn
        xt = np.where(is_, v, xt)
    valid = tv >= 0
    et = np.where(valid, expf(xt - m), F32(0))
    s = so + et
    lg = hw_logf(s) if defect == 'no_log1p' else np.where(et == 1, log1pf(so), hw_logf(s))
    l = m + lg
    lp = (xt - m) - lg
    inv = F32(1) / s
    p, q = et * inv, so * inv
    if defect == 'q_one_minus_p':
        q = F32(1) - p
    qg, dqg = np.ones_like(q), np.zeros_like(q)
    if gamma != 0:
        pos = q > 0
        qs = np.where(pos, q, F32(1))
        qg = np.where(pos, exp2f(gamma * hw_log2f(qs)), F32(0))
        dqg = np.where(pos, gamma * qg / qs, F32(0))
    w = expf(qg) if variant == 0 else qg
    wp = -dqg * w if variant == 0 else -dqg
    a = -w if defect == 'no_second_term' else -(p * wp * lp + w)
    a = np.where(valid, a, F32(0)).astype(F32)
    lsum = (w * lp).astype(F64)[valid].sum()
    cnt = float(valid.sum())
    loss = F32(-F64(F32(alpha)) * lsum / cnt) if cnt else F32(0)
    scale = F32(F64(F32(alpha)) / cnt) if cnt else F32(0)
    return l.astype(F32), a, loss, scale


def focal_bwd(x, labels, lse, coef, scale, grad_out=1.0, bf16=False):
    """focal_bwd_kernel: grad8<NEGATED> with w = coef gs, the labels loaded without the ignore index"""
    x = x.astype(F32)
    B, C, HW = x.shape
    tv = _labels(labels, C, 0, False)
    gs = F32(scale) * F32(grad_out)
    w = coef * gs
    e = expf(x - lse[:, None])
    h = (np.arange(C)[None, :, None] == tv[:, None]).astype(F32)
    d = ((h - e) * w[:, None]).astype(F32)
    return to_bf16(d) if bf16 else d


def dice_fwd(x, labels, smooth, ignore_index=255, has_ignore=True, max_blocks=0, defect=None):
    """dice_fwd_kernel + dice_finalize_kernel: (lse, coef [2 C] f32, loss, (P, I, N) f64).  The lane sums are f32: the 8 pixels of
    a group in order, one addition per trip; then f64.  Defect skip_last_group: the statistics' group loop stops one group short
    when the groups do not fill the last block"""
    x = x.astype(F32)
    B, C, HW = x.shape
    tv = _labels(labels, C, ignore_index, has_ignore)
    l = lse8(x)
    grid, trips = X.soft_grid(B, HW, max_blocks, X.SOFT_DICE_BLOCKS)
    G, nl = B * HW // 8, grid * X.SOFT_NT
    live = np.ones(G, bool)
    if defect == 'skip_last_group' and G % X.SOFT_NT:
        live[-1] = False
    valid = (tv >= 0).reshape(G, 8) & live[:, None]
    P, I, N = np.zeros(C), np.zeros(C), np.zeros(C)
    lg = l.reshape(G, 8)
    for c in range(C):
        v = np.transpose(x[:, c].reshape(B, HW // 8, 8), (0, 1, 2)).reshape(G, 8)
        p = np.where(valid, expf(v - lg), F32(0))
        is_ = (tv.reshape(G, 8) == c) & valid
        out = []
        for term in (p, np.where(is_, p, F32(0)), is_.astype(F32)):
            sp = np.zeros(G, F32)
            for j in range(8):
                sp = sp + term[:, j]
            pad = np.zeros(trips * nl, F32)
            pad[:G] = sp
            acc = np.zeros(nl, F32)
            for k in range(trips):
                acc = acc + pad[k * nl:(k + 1) * nl]
            out.append(acc.astype(F64).sum())
        P[c], I[c], N[c] = out
    sm = F64(F32(smooth))
    coef = np.zeros(2 * C, F32)
    term = np.zeros(C)
    if N.sum() > 0:
        den, num = P + N + sm, 2.0 * I + sm
        ok = den > 0
        dd = np.where(ok, den, 1.0)
        term = np.where(ok, 1.0 - num / dd, 1.0)
        coef[:C] = np.where(ok, -2.0 / (C * dd), 0.0).astype(F32)
        coef[C:] = np.where(ok, num / (C * dd * dd), 0.0).astype(F32)
    return l, coef, F32(term.sum() / C), (P, I, N)


def dice_bwd(x, labels, lse, coef, grad_out=1.0, ignore_index=255, has_ignore=True, bf16=False):
    """dice_bwd_kernel: dot = sum_c p_c G_c class by class, then d = p_k ((G_k) - dot) gv"""
    x = x.astype(F32)
    B, C, HW = x.shape
    tv = _labels(labels, C, ignore_index, has_ignore)
    gv = np.where(tv >= 0, F32(grad_out), F32(0))
    dot = np.zeros((B, HW), F32)
    G = []
    for c in range(C):
        Gc = coef[C + c] + np.where(tv == c, coef[c], F32(0))
        G.append(Gc)
        dot = dot + expf(x[:, c] - lse) * Gc
    d = np.stack([expf(x[:, c] - lse) * (G[c] - dot) * gv for c in range(C)], 1).astype(F32)
    return to_bf16(d) if bf16 else d


# ----------------------------------------------------------------------------------------------------------- csrc/softhead.hip
def head_focal_terms(p, q, lp, gamma, variant):
    """focal_terms of csrc/softhead.hip: (w, coef = w - w' p lp)"""
    gamma = F32(gamma)
    qg, dqg = np.ones_like(q), np.zeros_like(q)
    if gamma != 0:
        pos = q > 0
        qs = np.where(pos, q, F32(1))
        qg = np.where(pos, exp2f(gamma * hw_log2f(qs)), F32(0))
        dqg = np.where(pos, gamma * qg / qs, F32(0))
    wq = expf(qg) if variant == 0 else qg
    dw = dqg * wq if variant == 0 else dqg
    return wq, (wq - dw * p * lp).astype(F32)


def focal_coef_from_ce(ce, labels, C, gamma, variant, alpha, ignore_index=255, has_ignore=True, defect=None):
    """focal_coef_kernel + softhead_focal_finalize_kernel: (coef [n], loss, scale).  q = -expm1f(-ce), correctly rounded here;
    denormal q are flushed on the way into the logarithm.  Defect leak: the coef of a pixel that does not count is left as computed"""
    ce = np.asarray(ce, F32)
    valid = _labels(labels, C, ignore_index, has_ignore) >= 0
    lp = -ce
    q = (-np.expm1(lp.astype(F64))).astype(F32)
    q = np.where(q < F32(2.0 ** -126), F32(0), q)
    with np.errstate(under='ignore'):
        wq, cf = head_focal_terms(expf(lp), q, lp, gamma, variant)
        lsum = (wq * lp).astype(F64)[valid].sum()
    cnt = float(valid.sum())
    if defect != 'leak':
        cf = np.where(valid, cf, F32(0))
    a = F64(F32(alpha))
    return cf, (F32(-a * lsum / cnt) if cnt else F32(0)), (F32(a / cnt) if cnt else F32(0))
