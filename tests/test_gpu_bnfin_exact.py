"""The BatchNorm finalize chain (tss_bn_finalize, tss_bn_bwd_finalize, tss_slab_reduce, tss_bn_finalize_sync, tss_bn_bwd_finalize_sync:
csrc/pointwise.hip, csrc/bnfin.h), the dropout kernels (tss_dropout, tss_dropout_tick, tss_dropout_mask), tss_tensor_stats (csrc/zoo.hip),
tss_bias_grad and tss_cast_weights, each called through _native.call against an independent reference: tests/exact.py (last section:
numpy float64 restatements whose last steps are IEEE float32) and tests/philox_ref.py (Philox4x32-10 in numpy, pinned to the Random123
known answers on the CPU).  Every output sits in a buffer longer than needed whose tail of sentinels must survive; statistics slabs
start as NaN.  No bound comes from what a GPU returned; the references, premises and bounds are run on the CPU in
tests/test_exact_bounds.py, with one realistic defect each.

Equalities (bit for bit): every dropout mask and every kept value at p = 1/2, 3/4 and 0; tss_dropout_tick; the tier-1 finalize (mean, scale
from the stored invstd, running_mean, running_var, num_batches_tracked, every output of the backward finalize, tss_slab_reduce, the
_sync pair against the union and against the plain kernels); the f32 sums of tss_tensor_stats on 12-bit values; tss_bias_grad on its
exact operands; tss_cast_weights.
Bounded (the largest |out - ref| / bound is printed on a BNFIN_MARGIN line before the assertion: profiles/bnfin_exact_margins.txt): the
kept values at p = 0.1, 0.3; invstd; the tier-2 finalize; the bf16 sums of tss_tensor_stats; the tier-2 tss_bias_grad.
A channel whose variance is negative before the clamp is built in tier 1 (between -1/4 and -1/8 on exact slabs: without the clamp invstd is a NaN);
through tss_tensor_stats it could not be built without restating that kernel's summation order, and at that size (2^-51 of mean^2) the
clamp cannot be told from its absence behind eps."""
import ctypes

import numpy as np
import pytest
import torch

from tests import exact as X
from tests import philox_ref as R
from tests.exact_gpu import DEV, Buf, N_, check_slab_rows, nan_slabs

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [BF, F32]
PAD = 16
NPF = np.float32


def sync():
    torch.cuda.synchronize()


def code(dtype):
    return N_().dtype_code(dtype)


def margin(check, dtype, ratio):
    print('BNFIN_MARGIN %-34s %-5s %.4f' % (check, {BF: 'bf16', F32: 'f32', None: '-'}[dtype], ratio))
    return ratio


class FVec:
    """an f32 device vector of n values (sentinel when none are given) and PAD sentinels behind them"""
    def __init__(self, n, values=None):
        t = X.sentinel((n + PAD,), dtype=F32)
        if values is not None:
            t[:n] = torch.from_numpy(np.ascontiguousarray(values, dtype=NPF))
        self.n, self.t = n, t.to(DEV)
        self.ptr = self.t.data_ptr()

    def get(self):
        return self.t[:self.n].cpu().numpy()

    def tail_ok(self):
        return bool((X.bits(self.t.cpu())[self.n:] == X.SENTINEL_BITS32).all())

    def untouched(self):
        return bool((X.bits(self.t.cpu()) == X.SENTINEL_BITS32).all())


def opt(v):
    return None if v is None else v.ptr


def same32(out, want, what):
    out, want = np.ascontiguousarray(out, NPF), np.ascontiguousarray(want, NPF)
    bad = np.nonzero(out.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (what, 'not bit for bit at', bad[:3].tolist(), out[bad[:3]].tolist(), want[bad[:3]].tolist(), bad.size)


def slot_of(seed):
    return torch.tensor([ctypes.c_int64(seed).value], dtype=torch.int64, device=DEV)


# ----------------------------------------------------------------------------------------------------- tss_dropout
DROP_CASES = [(1, 8, 8), (37, 24, 40), (1000, 128, 136), (33001, 128, 128)]      # the last: 528016 vectors > 2048 x 256, a second trip
SEEDS = [0, 12345, (7 << 32) | 3, 2 ** 64 - 1]
DROP_REL = {F32: 2.0 ** -23, BF: 2.0 ** -8 + 2.0 ** -22}


def drop_scale_premise(p):
    """the kernel's inv = fl(1 / fl(1 - p)) against the reference's 1 / (1 - f32(p)): with its relative error d (numpy float32, IEEE), a
    kept value fl(x inv) is within d + 2^-24 (1 + d) of the f64 product, which must fit the 2^-23 the check allows"""
    p32 = NPF(p)
    exact = 1.0 / (1.0 - np.float64(p32))
    d = abs(float(NPF(1) / (NPF(1) - p32)) - exact) / exact
    return d + 2.0 ** -24 * (1 + d) <= 2.0 ** -23


def run_dropout(x, P, C, ld, p, slot, dtype):
    n = N_()
    off = min(ld - C, 8)
    xb = Buf(P, C, ld, off, x, dtype, nan_spare=True, nan_pad=True)
    yb = Buf(P, C, ld, off, dtype=dtype)
    n.call('tss_dropout', xb.ptr, xb.ld, yb.ptr, yb.ld, P, C, p, slot.data_ptr(), code(dtype), n.stream())
    sync()
    assert yb.untouched(), ('dropout', P, C, ld, p, 'padding or spare rows overwritten')
    return xb, yb


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('P,C,ld', DROP_CASES)
def test_dropout_mask_and_values(P, C, ld, seed, dtype):
    x = X.dyadic((P, C), X.case_gen(101, P, C))                   # never 0: the kept set can be read off the output
    slot = slot_of(seed)
    for p in (0.5, 0.75, 0.1, 0.3):
        what = ('dropout', P, C, ld, hex(seed), dtype, p)
        keep = torch.from_numpy(R.dropout_keep(P, C, p, seed))
        xb, yb = run_dropout(x, P, C, ld, p, slot, dtype)
        out = yb.rows()
        assert torch.equal(out != 0, keep), (what, 'kept set', int(((out != 0) != keep).sum()), 'elements differ')
        if p in (0.5, 0.75):
            assert torch.equal(out, torch.where(keep, x / (1 - p), torch.zeros_like(x))), (what, 'kept values are exact')
        else:
            assert drop_scale_premise(p)
            ref = x / (1.0 - float(NPF(p)))
            ratio = float(((out - ref).abs()[keep] / (DROP_REL[dtype] * ref.abs()[keep])).max()) if bool(keep.any()) else 0.0
            margin('dropout value p=%.1f' % p, dtype, ratio)
            assert ratio <= 1, (what, ratio)
    # the pitch plays no part: the other pitch gives the same output
    _, y1 = run_dropout(x, P, C, ld, 0.5, slot, dtype)
    _, y2 = run_dropout(x, P, C, C if ld > C else C + 8, 0.5, slot, dtype)
    assert torch.equal(y1.rows(), y2.rows()), ('dropout', P, C, ld, 'mask depends on the pitch')
    # backward: the same slot applies the same mask to another tensor
    g = X.dyadic((P, C), X.case_gen(102, P, C))
    _, gb = run_dropout(g, P, C, ld, 0.5, slot, dtype)
    assert torch.equal(gb.rows(), torch.where(torch.from_numpy(R.dropout_keep(P, C, 0.5, seed)), g * 2, torch.zeros_like(g)))
    # p = 0: the input's bits
    xb, yb = run_dropout(x, P, C, ld, 0.0, slot, dtype)
    win = lambda b: X.bits(b.t[:P, b.off:b.off + C].cpu())
    assert torch.equal(win(xb), win(yb)), ('dropout', P, C, ld, 'p = 0 changes bits')


def test_dropout_tick_hands_out_the_counter_and_advances_it_by_one():
    n = N_()
    start = (1 << 32) - 1                                         # the first tick carries into the high word
    counter, slot = slot_of(start), slot_of(77)
    n.call('tss_dropout_tick', counter.data_ptr(), slot.data_ptr(), n.stream())
    sync()
    assert slot.item() == start and counter.item() == start + 1
    n.call('tss_dropout_tick', counter.data_ptr(), slot.data_ptr(), n.stream())
    sync()
    assert slot.item() == start + 1 and counter.item() == start + 2


# ----------------------------------------------------------------------------------------------------- tss_dropout_mask
MASK_FILL = 0xA5


def mask_buffer(P):
    return torch.full((P * 16 + 64,), MASK_FILL, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('C', [8, 128])
@pytest.mark.parametrize('P', [1, 77, 131075])                   # the last: 524300 words > 2048 x 256, a second trip
def test_dropout_mask_bytes(P, C, p):
    n = N_()
    for seed in SEEDS:
        counter, m = slot_of(seed), mask_buffer(P)
        n.call('tss_dropout_mask', counter.data_ptr(), m.data_ptr(), P, C, p, n.stream())
        sync()
        got = m.cpu().numpy()
        want = R.dropout_mask_bytes(P, p, seed).reshape(-1)
        bad = np.nonzero(got[:P * 16] != want)[0]
        assert bad.size == 0, ('mask bytes', P, C, p, hex(seed), bad[:3].tolist(), bad.size)
        assert (got[P * 16:] == MASK_FILL).all(), 'bytes behind the mask overwritten'
        assert counter.item() == ctypes.c_int64(seed).value, 'tss_dropout_mask advanced the counter'


@pytest.mark.parametrize('C,p', [(136, 0.1), (8, 0.0)])
def test_dropout_mask_refuses(C, p):
    n = N_()
    counter, m = slot_of(5), mask_buffer(4)
    with pytest.raises(RuntimeError):
        n.call('tss_dropout_mask', counter.data_ptr(), m.data_ptr(), 4, C, p, n.stream())
    sync()
    assert bool((m == MASK_FILL).all()) and counter.item() == 5


# ----------------------------------------------------------------------------------------------------- finalize, tier 1
FIN_MODES = [(1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (0, 0, 0, 0)]     # gamma, running_mean, running_var, nbt
FIN_CASES = [(C, 10, m) for C in X.FIN_CHANNELS for m in range(len(FIN_MODES))] + \
            [(19, 0, 0), (132, 0, 1), (8, 3, 0), (264, 16, 0), (768, 16, 4), (4, 0, 5)]
NBT0 = 41


class FinOperands:
    """device operands of one forward finalize: gamma (ordinary f32 values), 8-bit dyadic running statistics, the batch counter"""
    def __init__(self, C, rng, mode=(1, 1, 1, 1), dyadic=True):
        has_g, has_rm, has_rv, has_nbt = mode
        self.C = C
        self.gamma = rng.uniform(-2, 2, size=C).astype(NPF) if has_g else None
        self.rm0 = (X.dyadic8_np(C, rng) if dyadic else rng.uniform(-3, 3, size=C).astype(NPF)) if has_rm else None
        self.rv0 = (X.dyadic8_np(C, rng, True) if dyadic else rng.uniform(0.01, 0.03, size=C).astype(NPF)) if has_rv else None
        self.fresh(has_nbt)

    def fresh(self, has_nbt=True):
        self.g = FVec(self.C, self.gamma) if self.gamma is not None else None
        self.rm = FVec(self.C, self.rm0) if self.rm0 is not None else None
        self.rv = FVec(self.C, self.rv0) if self.rv0 is not None else None
        self.nbt = torch.tensor([NBT0, -3], dtype=torch.int64, device=DEV) if has_nbt else None
        self.mean, self.invstd, self.scale = FVec(self.C), FVec(self.C), FVec(self.C)
        return self

    def call(self, entry, src, count, eps, momentum):
        n = N_()
        args = ([src.data_ptr(), float(count)] if entry == 'tss_bn_finalize' else [src.data_ptr()]) + \
            [opt(self.g), eps, momentum, opt(self.rm), opt(self.rv), None if self.nbt is None else self.nbt.data_ptr(),
             self.mean.ptr, self.invstd.ptr, self.scale.ptr, self.C, n.stream()]
        n.call(entry, *args)
        sync()

    def outputs(self):
        return {k: v.get() for k, v in (('mean', self.mean), ('invstd', self.invstd), ('scale', self.scale), ('running_mean', self.rm),
                                        ('running_var', self.rv)) if v is not None}

    def check_frame(self, what, launches=1):
        """sentinels behind every vector, the inputs that are read only unchanged, the batch counter + 1 per launch"""
        for v in (self.mean, self.invstd, self.scale, self.rm, self.rv, self.g):
            assert v is None or v.tail_ok(), (what, 'sentinel overwritten')
        if self.g is not None:
            same32(self.g.get(), self.gamma, (what, 'gamma changed'))
        if self.nbt is not None:
            assert self.nbt.tolist() == [NBT0 + launches, -3], (what, 'num_batches_tracked', self.nbt.tolist())


def check_tier1(o, ref, what):
    out = o.outputs()
    same32(out['mean'], ref['mean'], (what, 'mean'))
    assert np.isfinite(out['invstd']).all(), (what, 'invstd not finite: the clamp')
    r64 = ref['invstd64']
    ratio = float((np.abs(out['invstd'].astype(np.float64) - r64) / (X.FIN_INVSTD_REL * r64)).max())
    margin('finalize tier 1 invstd', None, ratio)
    assert ratio <= 1, (what, 'invstd', ratio)
    same32(out['scale'], X.bn_scale_ref(o.gamma, out['invstd']), (what, 'scale from the stored invstd'))
    for k in ('running_mean', 'running_var'):
        if k in out:
            same32(out[k], ref[k], (what, k))
    return out


@pytest.mark.parametrize('C,k,mode', FIN_CASES)
def test_bn_finalize_tier1(C, k, mode):
    rng = X.np_rng(201, C, k, mode)
    slabs, s, q = X.fin_tier1_slabs(C, k, rng)
    o = FinOperands(C, rng, FIN_MODES[mode])
    eps, momentum = (1e-5, 0.125) if mode % 2 == 0 else (1e-3, 0.5)
    o.call('tss_bn_finalize', torch.from_numpy(slabs).to(DEV), 2.0 ** k, eps, momentum)
    ref = X.bn_finalize_ref(s, q, 2.0 ** k, o.gamma, eps, momentum, o.rm0, o.rv0)
    what = ('bn_finalize', C, k, FIN_MODES[mode])
    out = check_tier1(o, ref, what)
    o.check_frame(what)
    assert ref['var64'][0] == 0 and ref['invstd64'][0] == 1.0 / np.sqrt(np.float64(NPF(eps))), (what, 'the constant channel')
    if C > 1:
        assert out['invstd'][1] == out['invstd'][0], (what, 'the channel whose variance is negative before the clamp')


@pytest.mark.parametrize('C,count', [(8, 0.0), (0, 16.0)])
def test_bn_finalize_refuses(C, count):
    n = N_()
    slabs, o = nan_slabs(8), FinOperands(8, X.np_rng(1))
    for entry, args in (('tss_bn_finalize', [slabs.data_ptr(), count, o.g.ptr, 1e-5, 0.1, o.rm.ptr, o.rv.ptr, o.nbt.data_ptr(), o.mean.ptr,
                                             o.invstd.ptr, o.scale.ptr, C, n.stream()]),
                        ('tss_bn_bwd_finalize', [slabs.data_ptr(), count, o.g.ptr, o.g.ptr, 1, 0, o.rm.ptr, o.rv.ptr, o.mean.ptr, o.invstd.ptr,
                                                 o.scale.ptr, C, n.stream()])):
        with pytest.raises(RuntimeError):
            n.call(entry, *args)
    sync()
    assert o.mean.untouched() and o.invstd.untouched() and o.scale.untouched() and o.nbt.tolist() == [NBT0, -3]
    same32(o.rm.get(), o.rm0, 'running_mean')
    same32(o.rv.get(), o.rv0, 'running_var')


# ----------------------------------------------------------------------------------------------------- backward finalize, tier 1
class BwdOperands:
    """device operands of one backward finalize: invstd and gamma ordinary f32 values, old dgamma / dbeta, the three outputs"""
    def __init__(self, C, rng, has_gamma=True, has_dg=True, has_db=True):
        self.C = C
        self.invstd = rng.uniform(0.05, 40, size=C).astype(NPF)
        self.gamma = rng.uniform(-2, 2, size=C).astype(NPF) if has_gamma else None
        self.dg0 = rng.standard_normal(C).astype(NPF) if has_dg else None
        self.db0 = rng.standard_normal(C).astype(NPF) if has_db else None
        self.fresh()

    def fresh(self):
        self.r, self.g = FVec(self.C, self.invstd), (FVec(self.C, self.gamma) if self.gamma is not None else None)
        self.dg = FVec(self.C, self.dg0) if self.dg0 is not None else None
        self.db = FVec(self.C, self.db0) if self.db0 is not None else None
        self.ga, self.gb, self.gce = FVec(self.C), FVec(self.C), FVec(self.C)
        return self

    def call(self, slabs, count=None, training=1, accumulate=0, gsums=None):
        n = N_()
        tail = [accumulate, opt(self.dg), opt(self.db), self.ga.ptr, self.gb.ptr, self.gce.ptr, self.C, n.stream()]
        if gsums is None:
            n.call('tss_bn_bwd_finalize', slabs.data_ptr(), float(count), self.r.ptr, opt(self.g), training, *tail)
        else:
            n.call('tss_bn_bwd_finalize_sync', slabs.data_ptr(), gsums.data_ptr(), self.r.ptr, opt(self.g), *tail)
        sync()

    def check(self, ref, what):
        for k, v in (('ga', self.ga), ('gb', self.gb), ('gce', self.gce), ('dgamma', self.dg), ('dbeta', self.db)):
            if v is not None:
                same32(v.get(), ref[k], (what, k))
                assert v.tail_ok(), (what, k, 'sentinel overwritten')
        same32(self.r.get(), self.invstd, (what, 'invstd changed'))
        assert self.r.tail_ok() and (self.g is None or self.g.tail_ok())


# (has gamma, dgamma, dbeta), training, accumulate
BWD_MODES = [((1, 1, 1), 1, 0), ((1, 1, 1), 1, 1), ((1, 1, 1), 0, 0), ((1, 1, 1), 0, 1), ((0, 1, 1), 1, 1), ((1, 0, 1), 1, 1),
             ((1, 1, 0), 1, 0), ((0, 0, 0), 1, 0)]


@pytest.mark.parametrize('mode', range(len(BWD_MODES)))
@pytest.mark.parametrize('C', X.FIN_CHANNELS)
def test_bn_bwd_finalize_tier1(C, mode):
    has, training, accumulate = BWD_MODES[mode]
    rng = X.np_rng(203, C, mode)
    slabs, se, sey = X.fin_bwd_slabs(C, rng)
    count = (1000.0, 1024.0, 1.0, 98304.0)[mode % 4]
    o = BwdOperands(C, rng, *has)
    o.call(torch.from_numpy(slabs).to(DEV), count, training, accumulate)
    o.check(X.bn_bwd_finalize_ref(se, sey, count, o.invstd, o.gamma, training, accumulate, o.dg0, o.db0),
            ('bn_bwd_finalize', C, has, training, accumulate, count))


# ----------------------------------------------------------------------------------------------------- the _sync pair, one process
GS_FILL = -7.25e77


def slab_reduce(slabs, count, C):
    """tss_slab_reduce into a [2 C + 1] window of a longer f64 buffer; returns the window as numpy, the tail checked"""
    n = N_()
    out = torch.full((2 * C + 1 + PAD,), GS_FILL, dtype=torch.float64, device=DEV)
    n.call('tss_slab_reduce', slabs.data_ptr(), float(count), out.data_ptr(), C, n.stream())
    sync()
    v = out.cpu().numpy()
    assert (v[2 * C + 1:] == GS_FILL).all(), 'tss_slab_reduce wrote behind 2 C + 1'
    return v[:2 * C + 1]


@pytest.mark.parametrize('C', X.FIN_CHANNELS)
def test_sync_pair_over_two_slab_buffers(C):
    """two replicas' slab buffers with counts 768 and 256 (the union: 1024, a tier-1 case split over 1024 rows), reduced one by one,
    added on the host in f64 (exact: integers): the forward _sync kernel equals the reference over the union, the backward one takes ga,
    gb, gce from the global sums and dgamma, dbeta from the first replica's slabs"""
    rng = X.np_rng(205, C)
    slabs, s, q = X.fin_tier1_slabs(C, 10, rng, rows=2 * X.STAT_SLABS)
    halves = [torch.from_numpy(np.ascontiguousarray(slabs[i * X.STAT_SLABS:(i + 1) * X.STAT_SLABS])).to(DEV) for i in range(2)]
    vecs = [slab_reduce(h, cnt, C) for h, cnt in zip(halves, (768.0, 256.0))]
    for i, (v, cnt) in enumerate(zip(vecs, (768.0, 256.0))):
        want = np.concatenate([slabs[i * X.STAT_SLABS:(i + 1) * X.STAT_SLABS].sum(0), [cnt]])
        assert (v == want).all(), ('tss_slab_reduce', C, i, np.nonzero(v != want)[0][:3].tolist())
    g = vecs[0] + vecs[1]
    assert (g[:C] == s).all() and (g[C:2 * C] == q).all() and g[2 * C] == 1024.0
    gs = torch.from_numpy(g).to(DEV)
    o = FinOperands(C, rng)
    o.call('tss_bn_finalize_sync', gs, None, 1e-5, 0.125)
    what = ('bn_finalize_sync', C)
    check_tier1(o, X.bn_finalize_ref(s, q, 1024.0, o.gamma, 1e-5, 0.125, o.rm0, o.rv0), what)
    o.check_frame(what)
    # backward: integer slabs of two replicas
    (b0, se0, sey0), (b1, se1, sey1) = X.fin_bwd_slabs(C, rng), X.fin_bwd_slabs(C, rng)
    d0, d1 = torch.from_numpy(b0).to(DEV), torch.from_numpy(b1).to(DEV)
    gb = torch.from_numpy(slab_reduce(d0, 768.0, C) + slab_reduce(d1, 256.0, C)).to(DEV)
    for acc in (0, 1):
        w = BwdOperands(C, rng)
        w.call(d0, accumulate=acc, gsums=gb)
        w.check(X.bn_bwd_finalize_ref(se0 + se1, sey0 + sey1, 1024.0, w.invstd, w.gamma, 1, acc, w.dg0, w.db0, local=(se0, sey0)),
                ('bn_bwd_finalize_sync', C, acc))


@pytest.mark.parametrize('C', X.FIN_CHANNELS)
def test_sync_pair_with_one_rank_equals_the_plain_kernels(C):
    rng = X.np_rng(207, C)
    slabs, s, q = X.fin_tier1_slabs(C, 10, rng)
    d = torch.from_numpy(slabs).to(DEV)
    own = torch.from_numpy(slab_reduce(d, 1024.0, C)).to(DEV)
    o = FinOperands(C, rng)
    o.call('tss_bn_finalize', d, 1024.0, 1e-3, 0.5)
    plain = o.outputs()
    o.fresh().call('tss_bn_finalize_sync', own, None, 1e-3, 0.5)
    for k, v in o.outputs().items():
        same32(v, plain[k], ('sync == plain', C, k))
    o.check_frame(('bn_finalize_sync', C))
    b, se, sey = X.fin_bwd_slabs(C, rng)
    db = torch.from_numpy(b).to(DEV)
    ownb = torch.from_numpy(slab_reduce(db, 1000.0, C)).to(DEV)
    w = BwdOperands(C, rng)
    w.call(db, 1000.0, 1, 1)
    plain = {k: v.get() for k, v in (('ga', w.ga), ('gb', w.gb), ('gce', w.gce), ('dgamma', w.dg), ('dbeta', w.db))}
    w.fresh().call(db, accumulate=1, gsums=ownb)
    for k, v in (('ga', w.ga), ('gb', w.gb), ('gce', w.gce), ('dgamma', w.dg), ('dbeta', w.db)):
        same32(v.get(), plain[k], ('bwd sync == plain', C, k))


# ----------------------------------------------------------------------------------------------------- finalize, tier 2
@pytest.mark.parametrize('P,C,ld,off,kind', [(3000, 24, 32, 8, 'vec'), (3000, 19, 24, 3, 'scalar'), (2999, 136, 144, 8, 'vec')])
def test_bn_finalize_tier2_from_tensor_stats(P, C, ld, off, kind):
    """stored f32 values near 30 with a deviation of 2^-3 -> tss_tensor_stats -> tss_bn_finalize, against the f64 BatchNorm of the stored
    values (through integers) within X.fin_tier2_bounds; the slab sums themselves are exact (asserted)"""
    n = N_()
    rng = X.np_rng(209, P, C)
    x = X.offset_values(P, C, rng)
    assert X.tensor_stats_plan(P, C, ld)[0] == kind
    zb = Buf(P, C, ld, off, torch.from_numpy(x), F32, nan_spare=True, nan_pad=True)
    slabs = nan_slabs(C)
    n.call('tss_tensor_stats', zb.ptr, zb.ld, P, C, slabs.data_ptr(), n.TSS_F32, n.stream())
    o = FinOperands(C, rng, dyadic=False)
    eps, momentum = 1e-5, 0.1
    o.call('tss_bn_finalize', slabs, float(P), eps, momentum)
    sums = slabs.cpu().numpy().sum(0)
    assert (sums[:C] == x.sum(0)).all() and (sums[C:] == (x * x).sum(0)).all(), 'the 12-bit premise: slab sums are exact'
    mean, var, qc = X.exact_moments(x)
    assert var[0] == 0 and (var[1:] > 2.0 ** -8).all()
    b = X.fin_tier2_bounds(var, qc, mean, eps, float(P), momentum, o.rm0.astype(np.float64), o.rv0.astype(np.float64))
    out = o.outputs()
    m64, t = np.float64(NPF(momentum)), var + np.float64(NPF(eps))
    rm0, rv0 = o.rm0.astype(np.float64), o.rv0.astype(np.float64)
    refs = dict(mean=mean, invstd=t ** -0.5, running_mean=(1 - m64) * rm0 + m64 * mean, running_var=(1 - m64) * rv0 + m64 * var * P / (P - 1.0))
    b['mean'] = (2.0 ** -24 + 2.0 ** -52) * np.abs(mean)
    what = ('finalize tier 2', P, C)
    for k in ('mean', 'invstd', 'running_mean', 'running_var'):
        ratio = float((np.abs(out[k].astype(np.float64) - refs[k]) / b[k]).max())
        margin('finalize tier 2 %s' % k, F32, ratio)
        assert ratio <= 1, (what, k, ratio)
    r0 = 1.0 / np.sqrt(np.float64(NPF(eps)))
    assert abs(float(out['invstd'][0]) - r0) <= X.FIN_INVSTD_REL * r0, (what, 'constant channel: var exactly 0, invstd = 1 / sqrt(eps)')
    same32(out['scale'], X.bn_scale_ref(o.gamma, out['invstd']), (what, 'scale'))
    o.check_frame(what)


# ----------------------------------------------------------------------------------------------------- tss_tensor_stats
# (P, C, ld, column offset, kernel)
TS_CASES = [(68123, 128, 136, 8, 'vec'),       # per = 134, npl = 16: a lane takes 9 pixels, two trips of four and a ragged third
            (70001, 16, 24, 8, 'vec'),         # npl = 128: two pixels per lane, idle lanes in the last block
            (2100, 1024, 1032, 8, 'vec'),      # the widest vector instance, npl = 2
            (1500, 264, 269, 3, 'scalar'),     # P below the vector threshold; two channel passes (256 + 8), an odd pitch
            (600, 1032, 1040, 8, 'scalar'),    # C above the vector limit: five passes
            (300, 24, 32, 8, 'scalar'),        # blocks 300 .. 511 own nothing
            (0, 24, 32, 8, 'scalar')]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('P,C,ld,off,kind', TS_CASES)
def test_tensor_stats_rows(P, C, ld, off, kind, dtype):
    n = N_()
    g = X.case_gen(211, P, C)
    v = X.dyadic((P, C), g) if dtype == BF else X.dyadic_q((P, C), g, 12, -4, 2)
    plan, per, npl = X.tensor_stats_plan(P, C, ld)
    assert plan == kind
    zb = Buf(P, C, ld, off, v, dtype, nan_spare=True, nan_pad=True)
    assert P == 0 or torch.equal(zb.rows(), v)
    slabs = nan_slabs(C)
    n.call('tss_tensor_stats', zb.ptr, zb.ld, P, C, slabs.data_ptr(), code(dtype), n.stream())
    sync()
    what = ('tensor_stats', P, C, ld, kind, dtype)
    check_slab_rows(slabs, range(X.cdiv(P, per)) if P else [], what)
    rows = slabs.cpu()
    f32_chain = kind == 'vec' and dtype == BF
    rel = (2.0 ** -23 * X.tensor_stats_chain(P, C) + 2.0 ** -50) if f32_chain else 2.0 ** -50
    worst = 0.0
    for half, terms in ((0, v), (1, v * v)):
        ref, mag = X.block_sums(terms, per), X.block_sums(terms.abs(), per)
        diff = (rows[:, half * C:(half + 1) * C] - ref).abs()
        assert bool((diff[mag == 0] == 0).all()), (what, 'a row of a block that owns no pixel')
        if bool((mag > 0).any()):
            worst = max(worst, float((diff[mag > 0] / (rel * mag[mag > 0])).max()))
    margin('tensor_stats %s rows' % kind, dtype, worst)
    assert worst <= 1, (what, 'block i owns pixels [i per, (i + 1) per)', worst)
    if dtype == BF and P:
        assert X.stats_excess(rows.sum(0), torch.cat([v, v * v], 1), X.tensor_stats_chain(P, C) if f32_chain else 1) <= 0, what


# ----------------------------------------------------------------------------------------------------- tss_bias_grad
def run_bias_grad(e, P, N, lde, init, dtype):
    n = N_()
    eb = Buf(P, N, lde, 3 if lde > N else 0, e, dtype, nan_spare=True, nan_pad=True)
    assert torch.equal(eb.rows(), e)
    db = FVec(N, init)
    n.call('tss_bias_grad', eb.ptr, eb.ld, P, N, db.ptr, code(dtype), n.stream())
    sync()
    assert db.tail_ok(), ('bias_grad', P, N, lde, 'wrote behind N')
    return db.get()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('P', [1, 3, 4101, 40000])               # the last: 10000 pixel groups over the 1024-block cap
@pytest.mark.parametrize('N', [1, 19, 64])
def test_bias_grad_adds_the_exact_column_sums(N, P, dtype):
    for lde in (N, N + 5):
        e, init = X.colsum_exact_values(P, N, X.np_rng(213, N, P, lde))
        out = run_bias_grad(torch.from_numpy(e), P, N, lde, init, dtype)
        same32(out, (init + e.sum(0)).astype(NPF), ('bias_grad', N, P, lde, dtype))


@pytest.mark.parametrize('dtype', DTYPES)
def test_bias_grad_tier2(dtype):
    P, N, lde = 40000, 19, 24
    rng = X.np_rng(215)
    e = torch.from_numpy(rng.standard_normal((P, N))).to(dtype).double()
    init = rng.standard_normal(N).astype(NPF)
    out = run_bias_grad(e, P, N, lde, init, dtype).astype(np.float64)
    ref = init.astype(np.float64) + e.sum(0).numpy()
    chain = X.colsum_chain(P)
    assert chain == 10 + 3 + 1024
    bound = 2.0 ** -23 * chain * (np.abs(init) + e.abs().sum(0).numpy())
    ratio = margin('bias_grad tier 2', dtype, float((np.abs(out - ref) / bound).max()))
    assert ratio <= 1, ratio


def test_bias_grad_refuses_65_channels():
    n = N_()
    eb, db = Buf(4, 65, 72, 0, torch.ones(4, 65), BF), FVec(65, np.zeros(65))
    with pytest.raises(RuntimeError):
        n.call('tss_bias_grad', eb.ptr, eb.ld, 4, 65, db.ptr, n.TSS_BF16, n.stream())
    sync()
    assert (db.get() == 0).all() and db.tail_ok()


# ----------------------------------------------------------------------------------------------------- tss_cast_weights
@pytest.mark.parametrize('blocks', [1, 3])
@pytest.mark.parametrize('zero_n', [0, 7, 4096 + 3])
def test_cast_weights_copy_transpose_and_zero_fill(zero_n, blocks):
    n = N_()
    jobs, keep, rows = [(19, 128), (64, 24)], [], []
    for i, (N, K) in enumerate(jobs):
        src = X.cast_sources(N, K, X.np_rng(217, i))
        s = X.sentinel((N * K + PAD,), dtype=F32)
        s[:N * K] = src.reshape(-1)
        d = [s.to(DEV), X.sentinel((N * K + PAD,), DEV, BF), X.sentinel((N * K + PAD,), DEV, BF)]
        keep.append((src, d))
        rows.append([d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), N, K])
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    zero = X.sentinel((zero_n + PAD,), DEV, F32)
    n.call('tss_cast_weights', table.data_ptr(), len(jobs), blocks, zero.data_ptr(), zero_n, n.stream())
    sync()
    for (N, K), (src, d) in zip(jobs, keep):
        what = ('cast_weights', N, K, zero_n, blocks)
        want = src.to(BF)
        copy, tr = d[1].cpu(), d[2].cpu()
        assert torch.equal(X.bits(copy[:N * K]), X.bits(want.reshape(-1))), (what, 'copy')
        assert torch.equal(X.bits(tr[:N * K]), X.bits(want.t().contiguous().reshape(-1))), (what, 'transpose')
        assert bool((X.bits(copy[N * K:]) == X.SENTINEL_BITS).all()) and bool((X.bits(tr[N * K:]) == X.SENTINEL_BITS).all()), what
        s = d[0].cpu()
        assert torch.equal(X.bits(s[:N * K]), X.bits(src.reshape(-1))) and bool((X.bits(s[N * K:]) == X.SENTINEL_BITS32).all()), what
    z = zero.cpu()
    assert bool((X.bits(z[:zero_n]) == 0).all()) and bool((X.bits(z[zero_n:]) == X.SENTINEL_BITS32).all()), ('zero fill', zero_n, blocks)
