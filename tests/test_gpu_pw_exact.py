"""Each C entry point of the pointwise (1x1) kernel family (csrc/pwfast.hip, wgrad.hip + wgreduce.h, pwbwd.hip, pwsweep.hip and the A_PW
path of convgemm.hip), called once per case through _native.call, against f64 conv2d / conv2d_input / conv2d_weight with a 1x1 kernel on
dyadic operands (tests/exact.py), with the harness of tests/test_gpu_zoo_exact.py and tests/test_gpu_dw_exact.py (tests/exact_gpu.py):
sentinel-filled output buffers with a pitch wider than the channel count, a column offset where the entry's alignment rule allows one and
spare rows behind, sentinel pad channels in the input pitches, NaN statistics slabs, NaN weight-gradient workspaces.

Every check is elementwise: conv_excess with K the contraction length (+1 with a bias or a folded residual, +2 behind
tss_pwconv_fwd_joined's epilogue: X.joined_fwd_ref), wgrad_excess with the chain of the kernel that ran (X.pw_wgrad_chain,
X.pwbwd_wgrad_chain, X.generic_wgrad_chain), stats_excess on the stored output bits (X.pwfast_stats_chain, X.pwbwd_stats_chain,
X.generic_stats_chain), Buf.untouched() for everything around the output window.  No tolerance is measured on the kernels, no element is
left out and no case is skipped.  The chain helpers restate the launch planners; their rows / workspace counts are asserted against
tss_pwconv_bwd_weight_ws, tss_pwconv_bwd_fused_rows, tss_pwconv_bwd_fused_drop_rows and tss_pwconv_bwd_sweep_rows, and the slab rows a
launch leaves in use against the restated grid.  Large pixel counts are evaluated and checked in row blocks (check_blocked).

Every instance is reached by its natural dispatch (the thresholds of pwfast.hip are function-local statics): the smallest pixel count
that selects it is the case's P, and X.pwfast_plan -- asserted per case -- says which instance that is.  Every lean case runs with and
without the bf16 weight shadows (w_bf16 / wT_bf16): the weights are bf16-exact, so the two runs must agree bit for bit.

Template instances the C entry points cannot reach: none of pwfast.hip, wgrad.hip, pwbwd.hip or pwsweep.hip; pwbwd_kernel<512, 128, 8, 1,
2> (128 -> 128) runs only through tss_pwconv_bwd_fused itself -- tss_pwconv_bwd_fused_preferred never selects it -- and the
transposed-read instance only under TSS_PW_BWD_BIG=2."""
import ctypes

import pytest
import torch

from tests import exact as X
from tests.exact_gpu import (DEV, Buf, Layer, N_, check_blocked, check_stats_sums, dev, env, nan_slabs, reduce_many, to_rows, vecs)

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
VARIANTS = {'bnrelu': (True, True), 'bn': (True, False), 'mat': (False, False)}       # (pending BatchNorm, ReLU)
NO_X = (None, 0, None, None, None, 0)
NO_RED = (None, None, 0, 0, 0)


def pad8(n):
    return (n + 7) // 8 * 8


def raw(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def both_shadows(run):
    """run(shadow) -> device tensors / Bufs / None, with and without the bf16 weight shadows: bit-identical; the first run's results"""
    a, b = run(True), run(False)
    for i, (u, v) in enumerate(zip(a, b)):
        if u is not None:
            assert torch.equal(raw(u.t if isinstance(u, Buf) else u), raw(v.t if isinstance(v, Buf) else v)), ('weight shadows change result', i)
    return a


class Pw:
    """dyadic operands of a 1x1 layer K -> N over P pixels (Layer with B = 1, H = P, W = 1) and their device buffers in one dtype"""
    def __init__(self, seed, P, K, N, variant='bnrelu', cbias=False, dtype=BF):
        affine, relu = VARIANTS[variant]
        self.L = L = Layer(seed, 1, K, P, 1, N, (1, 1), P, 1, affine=affine, relu=relu, cbias=cbias)
        n = N_()
        self.P, self.K, self.N, self.dtype, self.pending = P, K, N, dtype, affine
        self.code, self.st = n.dtype_code(dtype), n.stream()
        self.v = v = vecs(L)
        self.w = dev(L.w.reshape(N, K))
        self.wb, self.wT = self.w.to(BF), self.w.t().contiguous().to(BF)
        self.xb = Buf(P, K, K + 8, 0, to_rows(L.x), dtype)
        self.xargs = (self.xb.ptr, self.xb.ld, n.ptr(v['mean']), n.ptr(v['scale']), n.ptr(v['bias']), int(relu))
        self.eb = self.yrb = None

    def a(self):
        L = self.L
        return L.a() if self.dtype == BF else X.act_f32(L.x, L.mean, L.scale, L.bias, L.relu)

    def gop(self, mode):
        L = self.L
        if self.dtype == BF:
            return L.gop(mode)
        return X.gcomb_f32(L.e, L.y, L.ga, L.gb, L.gce, L.gmu) if mode == 2 else X.gcomb_f32(L.e, ga=L.ga)

    def gargs(self, mode):
        """mode 2: g = ga (e - gce) + gb (y - gmu); 1: g = ga e (yraw = NULL)"""
        n, v, L = N_(), self.v, self.L
        if self.eb is None:
            self.eb = Buf(self.P, self.N, pad8(self.N) + 16, 0, to_rows(L.e), self.dtype)
            self.yrb = Buf(self.P, self.N, pad8(self.N) + 8, 0, to_rows(L.y), self.dtype)
        if mode == 2:
            return (self.eb.ptr, self.eb.ld, self.yrb.ptr, self.yrb.ld, n.ptr(v['ga']), n.ptr(v['gb']), n.ptr(v['gce']), n.ptr(v['gmu']))
        return (self.eb.ptr, self.eb.ld, None, 0, n.ptr(v['ga']), None, None, None)

    def xc(self):
        return to_rows(self.L.x - (self.L.mean if self.pending else 0))


def fwd_ref(a, w, cb=None, scale=1.0):
    """row-block reference of y = scale (a W^T) + bias for check_blocked"""
    def f(r0, r1):
        ref, S = X.conv_ref(a[:, :, r0:r1], w)
        ref, S = to_rows(ref) * scale, to_rows(S) * scale
        return (ref + cb, S + cb.abs()) if cb is not None else (ref, S)
    return f


def bwd_ref(gop, w, mask=None):
    """row-block reference of e_in = mask (g W)"""
    def f(r0, r1):
        g = gop[:, :, r0:r1]
        ref, S = X.conv_input_ref((1, w.shape[1], g.shape[2], 1), w, g)
        ref, S = to_rows(ref), to_rows(S)
        return (ref * mask[r0:r1], S * mask[r0:r1]) if mask is not None else (ref, S)
    return f


def out_excess(dtype):
    return X.conv_excess if dtype == BF else X.f32_excess


def generic(fn):
    """fn() on the generic kernels (tss_set_option(TSS_OPT_DISABLE_FAST_PATHS, 1)), the option restored whatever happens"""
    n = N_()
    n.call('tss_set_option', 1, 1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        n.call('tss_set_option', 1, 0)


# ----------------------------------------------------------------------------------------------------- forward: pwfast_kernel / _mc
def run_fwd(P, K, N, variant, cbias, stats, plan, seed=0):
    n = N_()
    D = Pw(seed + P + 3 * K + 7 * N, P, K, N, variant, cbias)
    assert X.pwfast_plan(P, K, N) == plan
    # a ragged N (the classifier): the last 4-channel group is stored whole, so the contract puts a 0 into each pad channel up to N % 4 == 0
    Nw = (N + 3) // 4 * 4
    cb = D.L.cb

    def run(shadow):
        yb, sl = Buf(P, Nw, Nw + (4 if Nw != N else 16), 0 if Nw != N else 8), (nan_slabs(N) if stats else None)
        n.call('tss_pwconv_fwd', *D.xargs, n.ptr(D.w), n.ptr(D.wb) if shadow else None, n.ptr(D.v['cb']), yb.ptr, yb.ld, n.ptr(sl),
               P, K, N, D.code, D.st)
        torch.cuda.synchronize()
        return yb, sl
    yb, sl = both_shadows(run)
    f = fwd_ref(D.a(), D.L.w, cb)

    def ref_fn(r0, r1):
        ref, S = f(r0, r1)
        z = torch.zeros(r1 - r0, Nw - N, dtype=torch.float64)
        return torch.cat([ref, z], 1), torch.cat([S, z], 1)
    sums = check_blocked(yb, ref_fn, K + (1 if cbias else 0), ('fwd', plan), second=(lambda out, r0, r1: out) if stats else None)
    if stats:
        chain, rows = X.pwfast_stats_chain(P, K, N)
        check_stats_sums(sl, sums, chain, ('fwd stats', plan), rows_used=rows)


# (P, K, N, variant, conv bias, statistics): pwfast_kernel<false, 64> at P = 200 = 3 tiles of 64 + 8 pixels: K 8 / 48 / 128 (one k-step
# of which 3/4 is padding, two with half of the second padding, four), N 4 / 96 / 132 (one fragment of which 3/4 is outside, six
# fragments over both wave columns, a second column chunk of 4 channels)
FWD_64 = [(200, K, N, ('bnrelu', 'bn', 'mat')[(i + j) % 3], (i + j) % 2 == 0, True)
          for i, K in enumerate((8, 48, 128)) for j, N in enumerate((4, 96, 132))]


@pytest.mark.parametrize('P,K,N,variant,cbias,stats', FWD_64 + [(200, 128, 19, 'bnrelu', True, False), (1, 8, 4, 'mat', False, True)])
def test_forward_single_chunk_small_tile_within_the_exact_bound(P, K, N, variant, cbias, stats):
    run_fwd(P, K, N, variant, cbias, stats, (False, 64))


def test_forward_single_chunk_small_tile_with_three_tiles_per_block():
    """66 037 pixels = 1 031 tiles of 64 + 53: 129 per XCD range over 64 blocks, so a block owns 3 (two prefetches in its loop) and the last
    tile is ragged"""
    assert X.pwfast_stats_chain(66037, 32, 32) == (2 * 3 + 4, 512)
    run_fwd(66037, 32, 32, 'bnrelu', False, True, (False, 64))


def test_forward_single_chunk_large_tile_within_the_exact_bound():
    """pwfast_kernel<false, 128>: 700 tiles x 6 column chunks = 4 200 block-tiles, the smallest count that selects it; narrow contraction
    (one k-step, 3/4 padding), 9 tiles per block, the last one ragged"""
    P = 128 * 700 - 59
    assert X.pwfast_plan(P - 128, 8, 768) == (False, 64) and X.pwfast_stats_chain(P, 8, 768) == (4 * 9 + 4, 80)
    run_fwd(P, 8, 768, 'bnrelu', True, True, (False, 128))


# pwfast_mc_kernel<false, 32 | 64 | 128>: t = ceil(P / 128) x 2 chunks of N = 256: 16, 194 (97 tiles), 256 (128 tiles); K = 136: a second
# contraction chunk of 8 channels; K = 768: six chunks; (1 000, 264, 132): a third chunk of 8 and a second column chunk of 4 channels
@pytest.mark.parametrize('P,K,N,variant,cbias,plan', [(1000, 768, 256, 'bnrelu', True, (True, 32)), (1000, 264, 132, 'bn', False, (True, 32)),
                                                     (12300, 136, 256, 'mat', False, (True, 64)), (16300, 136, 256, 'bnrelu', True, (True, 128))])
def test_forward_multi_chunk_every_tile_size_within_the_exact_bound(P, K, N, variant, cbias, plan):
    run_fwd(P, K, N, variant, cbias, True, plan)


# ----------------------------------------------------------------------------------------------------- forward: concat sources
@pytest.mark.parametrize('nsrc,bcast,P,N,plan', [(2, 1, 300, 64, (True, 32)), (5, 0, 300, 132, (True, 32)), (2, None, 16300, 256, (True, 128))])
def test_forward_over_concatenated_sources_within_the_exact_bound(nsrc, bcast, P, N, plan):
    """tss_pwconv_fwd_multi: chunk kc of the contraction reads source kc with its own pending BatchNorm (one source materialised: NULL
    vectors); source `bcast` is ONE row with pitch 0, broadcast to every pixel"""
    n = N_()
    st = n.stream()
    assert X.pwfast_plan(P, 128 * nsrc, N) == plan
    Ls = [Layer(100 + 7 * nsrc + i, 1, 128, 1 if i == bcast else P, 1, 8, (1, 1), 1, 1, affine=i != nsrc - 1, relu=True, cbias=False)
          for i in range(nsrc)]
    g = torch.Generator().manual_seed(nsrc)
    w = X.dyadic((N, 128 * nsrc, 1, 1), g, emin=-6, emax=-2)
    cb = X.dyadic((N,), g)
    w_d, cb_d = dev(w.reshape(N, -1)), dev(cb)
    wb = w_d.to(BF)
    bufs = [Buf(L.H, 128, 136, 0, to_rows(L.x)) for L in Ls]
    vs = [vecs(L) for L in Ls]
    arr = lambda key: (ctypes.c_void_p * nsrc)(*[n.ptr(v[key]) for v in vs])
    srcs = (ctypes.c_void_p * nsrc)(*[b.ptr for b in bufs])
    lds = (ctypes.c_long * nsrc)(*[0 if i == bcast else b.ld for i, b in enumerate(bufs)])
    a = torch.cat([L.a().expand(1, 128, P, 1) for L in Ls], 1)

    def run(shadow):
        yb = Buf(P, N, N + 8, 4)
        n.call('tss_pwconv_fwd_multi', srcs, lds, arr('mean'), arr('scale'), arr('bias'), nsrc, 1, n.ptr(w_d), n.ptr(wb) if shadow else None,
               n.ptr(cb_d), yb.ptr, yb.ld, P, N, n.TSS_BF16, st)
        torch.cuda.synchronize()
        return (yb,)
    yb, = both_shadows(run)
    check_blocked(yb, fwd_ref(a, w, cb), 128 * nsrc + 1, ('multi', nsrc))


# ----------------------------------------------------------------------------------------------------- forward: dropout on load
def drop_mask(P, K, p, counter):
    """tss_dropout_mask's bytes ([P][16], bit j of byte v: channel 8 v + j kept) and the keep factor [P][K] read back from them"""
    n = N_()
    mask = torch.zeros(P, 16, dtype=torch.uint8, device=DEV)
    n.call('tss_dropout_mask', n.ptr(counter), n.ptr(mask), P, K, p, n.stream())
    torch.cuda.synchronize()
    m = mask.cpu().to(torch.int32)
    keep = torch.stack([(m[:, k // 8] >> (k % 8)) & 1 for k in range(K)], 1).double()
    assert 0.5 * (1 - p) < keep.mean().item() < min(1.0, 1.5 * (1 - p))
    return mask, keep


# TM 64 at P = 200 (the classifier's ragged N; p = 0.75: 1 / (1 - p) = 4); TM 128 at 4 200 tiles of 128
@pytest.mark.parametrize('P,K,N,p,variant,plan', [(200, 128, 19, 0.5, 'bnrelu', 64), (200, 48, 64, 0.75, 'bn', 64),
                                                  (128 * 4200 - 77, 8, 4, 0.5, 'bnrelu', 128)])
def test_forward_with_dropout_on_load_within_the_exact_bound(P, K, N, p, variant, plan):
    n = N_()
    D = Pw(31 + K + N, P, K, N, variant, cbias=True)
    assert X.pwfast_plan(P, K, N)[1] == plan and n.lib().tss_pwconv_drop_supported(P, K, N, n.TSS_BF16) == 1
    counter = torch.full((1,), 12345, dtype=torch.int64, device=DEV)
    mask, keep = drop_mask(P, K, p, counter)
    Nw = (N + 3) // 4 * 4

    def run(shadow):
        yb = Buf(P, Nw, Nw + 4, 4)
        n.call('tss_pwconv_fwd_drop', *D.xargs, n.ptr(D.w), n.ptr(D.wb) if shadow else None, n.ptr(D.v['cb']), yb.ptr, yb.ld, n.ptr(mask), p,
               n.ptr(counter), P, K, N, D.code, D.st)
        torch.cuda.synchronize()
        return (yb,)
    yb, = both_shadows(run)
    assert counter.item() == 12345 + 2                      # the consumer advances the Philox counter, once per launch
    a = D.a() * keep.t().reshape(1, K, P, 1)                # kept or zero, 1 / (1 - p) (a power of two) on the accumulator
    f = fwd_ref(a, D.L.w, D.L.cb, scale=1.0 / (1.0 - p))

    def ref_fn(r0, r1):
        ref, S = f(r0, r1)
        z = torch.zeros(r1 - r0, Nw - N, dtype=torch.float64)
        return torch.cat([ref, z], 1), torch.cat([S, z], 1)
    check_blocked(yb, ref_fn, K + 1, ('drop', plan))


# ----------------------------------------------------------------------------------------------------- forward: eval epilogue
@pytest.mark.parametrize('K,plan', [(64, (False, 64)), (264, (True, 32))])
@pytest.mark.parametrize('res,relu', [(False, False), (False, True), (True, False), (True, True)])
def test_forward_with_the_joined_epilogue_within_its_derived_bound(K, plan, res, relu):
    """tss_pwconv_fwd_joined at P = 300 (ragged last tile), N = 96: X.joined_fwd_ref's bound"""
    n = N_()
    P, N = 300, 96
    D = Pw(57 + K + 2 * res + relu, P, K, N, 'bnrelu', cbias=True)
    assert X.pwfast_plan(P, K, N) == plan
    g = torch.Generator().manual_seed(K + res)
    omean, obeta, oscale = X.dyadic((N,), g), X.dyadic((N,), g), X.pow2((N,), g, 0.5, 4)
    resid = X.dyadic((P, N), g, zero_frac=0.05)
    ov = [dev(t) for t in (omean, oscale, obeta)]
    rb = Buf(P, N, N + 4, 0, resid) if res else None

    def run(shadow):
        yb = Buf(P, N, N + 8, 4)
        n.call('tss_pwconv_fwd_joined', *D.xargs, n.ptr(D.w), n.ptr(D.wb) if shadow else None, n.ptr(D.v['cb']), *[n.ptr(t) for t in ov],
               rb.ptr if res else None, rb.ld if res else 0, int(relu), yb.ptr, yb.ld, P, K, N, D.code, D.st)
        torch.cuda.synchronize()
        return (yb,)
    yb, = both_shadows(run)
    f = fwd_ref(D.a(), D.L.w)

    def ref_fn(r0, r1):
        conv, S = f(r0, r1)
        return X.joined_fwd_ref(conv, S, D.L.cb, omean, oscale, obeta, resid[r0:r1] if res else None, relu)
    check_blocked(yb, ref_fn, K + 2, ('joined', plan, res, relu))


# ----------------------------------------------------------------------------------------------------- weight gradient: wgfast_kernel
class Wg:
    """tss_pwconv_bwd_weight of a layer on the lean kernel: workspace (NaN, with a NaN tail that must survive) + dW, and the check"""
    def __init__(self, P, K, N, variant='bnrelu', D=None):
        self.D = D = D or Pw(211 + P + 3 * K + 5 * N, P, K, N, variant)
        n = N_()
        self.P, self.K, self.N = P, K, N
        self.chain, self.nws = X.pw_wgrad_chain(P, K, N)
        assert n.lib().tss_pwconv_bwd_weight_ws(P, K, N, n.TSS_BF16) == self.nws, ('workspace floats', self.nws)
        a = D.a()
        self.ref, self.S = X.conv_weight_ref(a, (N, K, 1, 1), D.gop(2))

    def launch(self, defer, fin=None):
        n, D = N_(), self.D
        ws = torch.full((self.nws + 64,), float('nan'), device=DEV)
        dw = torch.zeros(self.N, self.K, device=DEV)
        n.call('tss_pwconv_bwd_weight', *D.gargs(2), *D.xargs, n.ptr(dw), n.ptr(ws), int(defer), self.P, self.K, self.N, D.code, fin, D.st)
        return ws, dw

    def red_args(self, ws, dw):
        return (N_().ptr(ws), N_().ptr(dw), self.P, self.K, self.N)

    def check(self, ws, dw, what):
        torch.cuda.synchronize()
        assert torch.isnan(ws[self.nws:]).all(), (what, 'wrote behind the workspace')
        ex = X.wgrad_excess(dw.double().cpu().reshape(self.ref.shape), self.ref, self.S, self.chain)
        # (a NaN -- a slot element read but never written -- fails too)
        assert ex <= 0, (what, 'weight gradient excess', ex, 'chain', self.chain)


# (P, K, N, variant, (stage, nsplit, tiles)).  wgfast_kernel<128> (both chunk widths <= 64): 300 pixels = 2 stages + 44, the small-layer rule
# (256 pixels per block); 130 600 pixels: ceil(P / 512) = 256, the other side of the rule, 4 stages per block, ragged; <64>: 1 000 pixels at
# 128 x 128 (all four waves own a quadrant), K or N over 128 (several tiles, the last 8 / 64 wide: waves that split the pixels instead),
# 22 000 pixels x 6 tiles: tiles ceil(P / 512) = 258, the other side of the rule with several tiles
WG = [(300, 64, 64, 'bnrelu', (128, 2, 1)), (130600, 8, 16, 'bn', (128, 256, 1)), (517, 48, 8, 'mat', (128, 3, 1)),
      (1000, 128, 128, 'bnrelu', (64, 4, 1)), (777, 96, 576, 'bn', (64, 4, 5)), (600, 264, 8, 'bnrelu', (64, 3, 3)),
      (22000, 136, 264, 'mat', (64, 43, 6))]


@pytest.mark.parametrize('P,K,N,variant,split', WG)
@pytest.mark.parametrize('defer', [0, 1])
def test_weight_gradient_lean_kernel_within_the_exact_bound(P, K, N, variant, split, defer):
    """defer_reduce = 0: the slot reduction follows in the same call; 1: tss_pwconv_wg_reduce"""
    n = N_()
    assert X.pw_wgrad_split(P, K, N) == split
    W = Wg(P, K, N, variant)
    ws, dw = W.launch(defer)
    if defer:
        torch.cuda.synchronize()
        assert not dw.any(), 'defer_reduce = 1 touched dW'
        n.call('tss_pwconv_wg_reduce', n.ptr(ws), n.ptr(dw), P, K, N, n.stream())
    W.check(ws, dw, ('wgfast', split, defer))


def test_weight_gradient_carries_the_finalize_of_another_layer():
    """the `fin` job: the first blocks of the wgfast grid run tss_bn_bwd_finalize's block of ANOTHER layer (132 channels); its five
    outputs equal the stand-alone call bit for bit, and the weight gradient behind those blocks holds its bound"""
    from torch_semantic_segmentation_amd import ops
    n = N_()
    C2, st = 132, n.stream()
    g = torch.Generator().manual_seed(9)
    bst = torch.randn(n.stat_slabs(), 2 * C2, generator=g, dtype=torch.float64).to(DEV)
    invstd, gamma = (torch.rand(C2, generator=g) + 0.5).to(DEV), torch.randn(C2, generator=g).to(DEV)

    def outs():
        o = torch.full((5, C2), float('nan'), device=DEV)
        o[0:2] = 1.0                                                    # accumulate = 1: onto existing gradients
        return o
    a, b = outs(), outs()
    job = ops.BnBwdJob(n.ptr(bst), 4321.0, n.ptr(invstd), n.ptr(gamma), 1, 1, *[n.ptr(a[i]) for i in range(5)], C2)
    W = Wg(1000, 128, 128)
    ws, dw = W.launch(0, ctypes.byref(job))
    n.call('tss_bn_bwd_finalize', n.ptr(bst), 4321.0, n.ptr(invstd), n.ptr(gamma), 1, 1, *[n.ptr(b[i]) for i in range(5)], C2, st)
    W.check(ws, dw, 'wgfast + fin')
    assert torch.isfinite(a).all() and torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------- backward-data: pwfast_kernel / _mc
def run_bwd(P, K, N, kind, carry, plan, seed=0):
    """kind: 'bnrelu' / 'bn' (pending input: mask + bstats), 'mat' (materialised), 'radd' (tss_pwconv_bwd_data_radd), 'joined' /
    'joined_radd' (tss_pwconv_bwd_data_joined).  carry: None, 'own' (this layer's weight-gradient slots, wg_P = 0) or 'other' (another
    layer's, wg_P / wg_K / wg_N given): the first blocks of the launch reduce them"""
    n = N_()
    variant = kind if kind in VARIANTS else 'mat'
    D = Pw(seed + 401 + P + 3 * K + 5 * N + len(kind), P, K, N, variant)
    assert X.pwfast_plan(P, N, K, bwd=True) == plan
    L = D.L
    g = torch.Generator().manual_seed(P + K)
    radd = X.dyadic((P, K), g, zero_frac=0.05) if kind.endswith('radd') else None
    joined = kind.startswith('joined')
    jout, jy, jmean = (X.dyadic((P, K), g, zero_frac=0.1), X.dyadic((P, K), g), X.dyadic((K,), g)) if joined else (None, None, None)
    rb = Buf(P, K, K + 4, 0, radd) if radd is not None else None
    job, jyb, jm = (Buf(P, K, K + 4, 0, jout), Buf(P, K, K + 12, 4, jy), dev(jmean)) if joined else (None, None, None)
    W = None
    if carry == 'own':
        W = Wg(P, K, N, D=D)                                      # the same operands: the slots of THIS layer's weight gradient
    elif carry == 'other':
        W = Wg(700, 48, 136, 'bn')

    def run(shadow):
        ob = Buf(P, K, K + 16, 8)
        sl = nan_slabs(K) if (D.pending or joined) else None
        red, wsdw = NO_RED, (None, None)
        if W is not None:
            wsdw = W.launch(1)
            red = (n.ptr(wsdw[0]), n.ptr(wsdw[1])) + ((0, 0, 0) if carry == 'own' else (W.P, W.K, W.N))
        wT = n.ptr(D.wT) if shadow else None
        if joined:
            n.call('tss_pwconv_bwd_data_joined', *D.gargs(2), n.ptr(D.w), wT, ob.ptr, ob.ld, *red, rb.ptr if rb else None, rb.ld if rb else 0,
                   job.ptr, job.ld, jyb.ptr, jyb.ld, n.ptr(jm), n.ptr(sl), P, K, N, D.code, D.st)
        elif kind == 'radd':
            assert n.lib().tss_pwconv_bwd_data_radd_supported(P, K, N, D.code) == 1
            n.call('tss_pwconv_bwd_data_radd', *D.gargs(2), n.ptr(D.w), wT, ob.ptr, ob.ld, *red, rb.ptr, rb.ld, P, K, N, D.code, D.st)
        else:
            n.call('tss_pwconv_bwd_data', *D.gargs(2), n.ptr(D.w), wT, *(D.xargs if D.pending else NO_X), ob.ptr, ob.ld, n.ptr(sl), *red,
                   P, K, N, D.code, D.st)
        torch.cuda.synchronize()
        if W is not None:
            W.check(*wsdw, ('carried reduction', carry, kind))
        return ob, sl
    ob, sl = both_shadows(run)
    what = ('bwd data', kind, plan)
    mask = to_rows(L.mask()) if D.pending else None
    f = bwd_ref(D.gop(2), L.w, mask)
    if joined or radd is not None:
        def ref_fn(r0, r1):
            rin, Sin = f(r0, r1)
            rd = radd[r0:r1] if radd is not None else None
            return X.joined_bwd_ref(rin, Sin, rd, jout[r0:r1]) if joined else (rin + rd, Sin + rd.abs())
    else:
        ref_fn = f
    second = None
    if sl is not None:
        fac = (jy - jmean) if joined else D.xc()
        second = lambda out, r0, r1: fac[r0:r1]
    sums = check_blocked(ob, ref_fn, N + (1 if radd is not None else 0), what, second=second)
    if sl is not None:
        chain, rows = X.pwfast_stats_chain(P, N, K, bwd=True)
        check_stats_sums(sl, sums, chain, ('bstats',) + what, rows_used=rows)


# (P, conv K, conv N, kind, carry).  pwfast_kernel<true, 32> (+ JB) at P = 200 = 6 tiles of 32 + 8: output widths 8 / 96 / 136 (a second
# column chunk of 8 channels), contractions 8 / 48 / 128
BWD_32 = [(200, 8, 8, 'bnrelu', None), (200, 96, 48, 'bn', 'own'), (200, 136, 128, 'mat', 'other'), (200, 96, 128, 'radd', 'own'),
          (200, 8, 48, 'joined', None), (200, 136, 8, 'joined_radd', 'other'), (200, 96, 8, 'bnrelu', 'other'), (200, 8, 128, 'radd', None),
          (200, 136, 48, 'joined', 'own'), (1, 8, 8, 'bnrelu', None)]


@pytest.mark.parametrize('P,K,N,kind,carry', BWD_32)
def test_backward_data_single_chunk_small_tile_within_the_exact_bound(P, K, N, kind, carry):
    run_bwd(P, K, N, kind, carry, (False, 32))


@pytest.mark.parametrize('kind', ['bnrelu', 'joined_radd'])
def test_backward_data_single_chunk_small_tile_with_three_tiles_per_block(kind):
    """33 013 pixels = 1 031 tiles of 32 + 21: 129 per XCD range over 64 blocks: 3 per block, the last tile ragged"""
    assert X.pwfast_stats_chain(33013, 32, 32, bwd=True) == (1 * 3 + 4, 512)
    run_bwd(33013, 32, 32, kind, None, (False, 32))


@pytest.mark.parametrize('kind,carry', [('bnrelu', 'other'), ('joined_radd', None)])
def test_backward_data_single_chunk_large_tile_within_the_exact_bound(kind, carry):
    """pwfast_kernel<true, 64> (+ JB): 700 tiles of 64 x 6 column chunks = 4 200, the smallest count that selects it; contraction 8"""
    P = 64 * 700 - 14
    assert X.pwfast_plan(P - 64, 8, 768, bwd=True) == (False, 32)
    run_bwd(P, 768, 8, kind, carry, (False, 64))


# pwfast_mc_kernel<true, 32 | 64 | 128> (+ JB): contraction (conv N) 768 / 136, output width 256: the forward's three pixel counts
BWD_MC = [(1000, 256, 768, 'bnrelu', 'own', (True, 32)), (1000, 136, 136, 'joined', None, (True, 32)),
          (12300, 256, 136, 'radd', None, (True, 64)), (12300, 256, 136, 'bn', 'other', (True, 64)), (12300, 256, 136, 'joined', 'own', (True, 64)),
          (16300, 256, 136, 'joined_radd', 'other', (True, 128)), (16300, 256, 136, 'bnrelu', None, (True, 128))]


@pytest.mark.parametrize('P,K,N,kind,carry,plan', BWD_MC)
def test_backward_data_multi_chunk_every_tile_size_within_the_exact_bound(P, K, N, kind, carry, plan):
    run_bwd(P, K, N, kind, carry, plan)


# ----------------------------------------------------------------------------------------------------- generic kernels (A_PW)
def check_generic_stats(sl, sums, P, ND, dtype, what):
    check_stats_sums(sl, sums, X.generic_stats_chain(P, ND), what, f64=dtype == F32)


def run_generic(P, K, N, variant, dtype, forced):
    """convgemm_kernel A_PW (forward, backward-data) and wgrad_kernel on one layer.  forced: under tss_set_option(1, 1) with both
    backward operand modes; not forced (bf16): yraw = NULL alone, which takes the generic kernels by itself -- the weight-gradient slots
    of another layer then reduce in a launch of their own (tss_wg_reduce_standalone)"""
    n = N_()
    D = Pw(601 + P + K + N, P, K, N, variant, cbias=True, dtype=dtype)
    L = D.L
    ex = out_excess(dtype)

    def body():
        if forced:
            yb, sl = Buf(P, N, pad8(N) + 8, 8, dtype=dtype), nan_slabs(N)
            n.call('tss_pwconv_fwd', *D.xargs, n.ptr(D.w), None, n.ptr(D.v['cb']), yb.ptr, yb.ld, n.ptr(sl), P, K, N, D.code, D.st)
            torch.cuda.synchronize()
            sums = check_blocked(yb, fwd_ref(D.a(), L.w, L.cb), K + 1, ('generic fwd', dtype), second=lambda out, r0, r1: out, excess=ex)
            check_generic_stats(sl, sums, P, N, dtype, ('generic fwd stats', dtype))
        for mode in ((2, 1) if forced else (1,)):
            W = Wg(700, 48, 136, 'bn') if not forced else None
            ob, sl = Buf(P, K, K + 16, 8, dtype=dtype), (nan_slabs(K) if D.pending else None)
            red = NO_RED
            if W is not None:
                ws, wdw = W.launch(1)
                red = W.red_args(ws, wdw)
            n.call('tss_pwconv_bwd_data', *D.gargs(mode), n.ptr(D.w), None, *(D.xargs if D.pending else NO_X), ob.ptr, ob.ld, n.ptr(sl), *red,
                   P, K, N, D.code, D.st)
            torch.cuda.synchronize()
            if W is not None:
                W.check(ws, wdw, 'reduction behind a generic backward-data')
            gop = D.gop(mode)
            mask = to_rows(L.mask()) if D.pending else None
            xc = D.xc()
            sums = check_blocked(ob, bwd_ref(gop, L.w, mask), N, ('generic bwd', dtype, mode),
                                 second=(lambda out, r0, r1: xc[r0:r1]) if D.pending else None, excess=ex)
            if D.pending:
                check_generic_stats(sl, sums, P, K, dtype, ('generic bstats', dtype, mode))
            dw = torch.zeros(N, K, device=DEV)
            n.call('tss_pwconv_bwd_weight', *D.gargs(mode), *D.xargs, n.ptr(dw), None, 0, P, K, N, D.code, None, D.st)
            torch.cuda.synchronize()
            ref, S = X.conv_weight_ref(D.a(), (N, K, 1, 1), gop)
            chain = X.generic_wgrad_chain(P, K, N, 1) if dtype == BF else 2 * X.generic_wgrad_chain(P, K, N, 1, pt=32)
            e = X.wgrad_excess(dw.double().cpu().reshape(ref.shape), ref, S, chain)
            assert e <= 0, ('generic wgrad', dtype, mode, e)
    if forced:
        generic(body)
        assert not n.fast_paths_disabled()
    else:
        body()


# P = 300: 3 tiles, ragged; 136 -> 132: two contraction chunks and two column chunks each way; 72 -> 36: a ragged Cout (e / y through their
# pitch); P = 5 000: 40 tiles over 8 ranges of 5, 10 weight-gradient stages per block
@pytest.mark.parametrize('P,K,N,variant,dtype', [(300, 136, 132, 'bnrelu', BF), (300, 72, 36, 'bn', BF), (5000, 64, 128, 'mat', BF),
                                                 (300, 136, 132, 'bnrelu', F32), (300, 72, 36, 'mat', F32), (5000, 64, 128, 'bn', F32)])
def test_generic_pointwise_kernels_within_the_exact_bound(P, K, N, variant, dtype):
    run_generic(P, K, N, variant, dtype, True)


@pytest.mark.parametrize('P,K,N,variant', [(300, 96, 128, 'bnrelu'), (5000, 64, 64, 'mat')])
def test_backward_without_batchnorm_statistics_takes_the_generic_kernels(P, K, N, variant):
    run_generic(P, K, N, variant, BF, False)


# ----------------------------------------------------------------------------------------------------- one-sweep backward: pwbwd.hip
def run_fused(P, Cin, Cout, variant, with_y, bias, big_tr=False, drop_p=None, seed=0):
    """tss_pwconv_bwd_fused (+ tss_dw_reduce_many over its workspace rows) / tss_pwconv_bwd_fused_drop"""
    n = N_()
    drop = drop_p is not None
    D = Pw(seed + 701 + P + 3 * Cin + 5 * Cout, P, Cin, Cout, variant)
    L = D.L
    plan = X.pwbwd_rows(P, Cin, Cout, big_tr=big_tr, drop=drop)
    rows = plan[3]
    mode = 2 if with_y else 1
    if drop:
        counter = torch.full((1,), 777, dtype=torch.int64, device=DEV)
        mask, keep = drop_mask(P, Cin, drop_p, counter)
        dinv = 1.0 / (1.0 - drop_p)
    with env(TSS_PW_BWD_BIG=2 if big_tr else 0):
        lib_rows = n.lib().tss_pwconv_bwd_fused_drop_rows(P) if drop else n.lib().tss_pwconv_bwd_fused_rows(P, Cin, Cout)
        assert lib_rows == rows, (lib_rows, plan)

        def run(shadow):
            ob = Buf(P, Cin, Cin + 8, 4)
            sl = nan_slabs(Cin) if D.pending else None
            ws = torch.full((rows + 2, Cout * Cin), float('nan'), device=DEV)
            bws = torch.full((rows + 2, Cout), float('nan'), device=DEV) if bias else None
            tail = (ob.ptr, ob.ld, n.ptr(sl), n.ptr(ws), n.ptr(bws), P, Cin, Cout, D.code, D.st)
            if drop:
                n.call('tss_pwconv_bwd_fused_drop', *D.gargs(1), n.ptr(D.w), *D.xargs, int(D.pending), n.ptr(mask), drop_p, *tail)
            else:
                n.call('tss_pwconv_bwd_fused', *D.gargs(mode), n.ptr(D.w), n.ptr(D.wT) if shadow else None, *D.xargs, int(D.pending), *tail)
            dw = torch.zeros(Cout, Cin, device=DEV)
            reduce_many([(ws, dw, Cout * Cin, rows)])
            torch.cuda.synchronize()
            return ob, sl, ws, bws, dw
        ob, sl, ws, bws, dw = both_shadows(run) if not drop else run(False)
    what = ('fused', plan[0], variant, with_y)
    w = ws.cpu()
    assert not torch.isnan(w[:rows]).any() and torch.isnan(w[rows:]).all(), (what, 'workspace rows')
    gop, a = D.gop(mode), D.a()
    mask_in = to_rows(L.mask()) if D.pending else torch.ones(P, Cin, dtype=torch.float64)
    scale = 1.0
    if drop:
        a, mask_in, scale = a * keep.t().reshape(1, Cin, P, 1), mask_in * keep, dinv
    ref, S = X.conv_weight_ref(a, (Cout, Cin, 1, 1), gop)
    ex = X.wgrad_excess(dw.double().cpu().reshape(ref.shape), ref * scale, S * scale, X.pwbwd_wgrad_chain(plan))
    assert ex <= 0, (what, 'weight gradient excess', ex)
    f = bwd_ref(gop, L.w, mask_in)
    xc = D.xc()
    sums = check_blocked(ob, lambda r0, r1: tuple(t * scale for t in f(r0, r1)), Cout, what,
                         second=(lambda out, r0, r1: xc[r0:r1]) if D.pending else None)
    if D.pending:
        check_stats_sums(sl, sums, X.pwbwd_stats_chain(plan), ('fused bstats',) + what, rows_used=rows)
    if bias:
        b = bws.cpu()
        assert not torch.isnan(b[:rows]).any() and torch.isnan(b[rows:]).all(), (what, 'bias rows')
        gf = to_rows(X.gcomb_f32(L.e, L.y, L.ga, L.gb, L.gce, L.gmu) if with_y else X.gcomb_f32(L.e, ga=L.ga))      # the UNROUNDED g
        exb = X.wgrad_excess(b[:rows].double().sum(0), gf.sum(0), gf.abs().sum(0), X.pwbwd_bias_chain(plan))
        assert exb <= 0, (what, 'bias gradient excess', exb)


# (P, Cin, Cout, variant, yraw, bias_ws): the four default instances -- small 64 -> 64 and 8 -> 8 (TM 128), mid 64 -> 128, tall 128 -> 64 and
# 128 -> 19 (a ragged Cout through the pitch), big 128 -> 128 (one 8-wave block) -- at a ragged P of 2 - 5 tiles, and with several tiles per
# block (P > 512 TM: 2 per block, the last ragged)
FUSED = [(300, 64, 64, 'bnrelu', True, True), (300, 8, 8, 'mat', False, False), (517, 48, 24, 'bn', True, False),
         (300, 64, 128, 'bnrelu', True, False), (300, 24, 72, 'mat', True, True),
         (300, 128, 64, 'bn', False, True), (300, 128, 19, 'bnrelu', False, True), (300, 72, 40, 'mat', True, False),
         (300, 128, 128, 'bnrelu', True, True), (300, 72, 128, 'mat', False, False),
         (512 * 128 + 300, 8, 8, 'bnrelu', True, True), (512 * 64 + 77, 64, 128, 'bnrelu', True, False), (512 * 64 + 77, 128, 19, 'mat', False, True)]


@pytest.mark.parametrize('P,Cin,Cout,variant,with_y,bias', FUSED)
def test_one_sweep_backward_default_instances_within_the_exact_bound(P, Cin, Cout, variant, with_y, bias):
    run_fused(P, Cin, Cout, variant, with_y, bias)


@pytest.mark.parametrize('P,Cin,Cout,variant,with_y', [(300, 128, 128, 'bnrelu', True), (300, 72, 128, 'mat', False),
                                                     (512 * 64 + 77, 128, 72, 'bn', True)])
def test_one_sweep_backward_transposed_read_instance_within_the_exact_bound(P, Cin, Cout, variant, with_y):
    run_fused(P, Cin, Cout, variant, with_y, True, big_tr=True)


@pytest.mark.parametrize('P,Cin,Cout,variant,p', [(300, 128, 19, 'bnrelu', 0.5), (300, 48, 64, 'mat', 0.75), (512 * 64 + 9, 16, 8, 'bn', 0.5)])
def test_one_sweep_backward_with_dropout_within_the_exact_bound(P, Cin, Cout, variant, p):
    run_fused(P, Cin, Cout, variant, False, True, drop_p=p)


# ----------------------------------------------------------------------------------------------------- one-sweep backward: pwsweep.hip
def sweep_call(D, pending, with_y, rb, ob, sl, ws, P):
    n = N_()
    return ('tss_pwconv_bwd_sweep', *D.gargs(2 if with_y else 1), n.ptr(D.wT), *D.xargs, int(pending), rb.ptr if rb else None, rb.ld if rb else 0,
            ob.ptr, ob.ld, n.ptr(sl), n.ptr(ws), P, D.K, D.N, D.code, D.st)


@pytest.mark.parametrize('Cin,Cout,variant,with_y,radd', [
    (128, 128, 'bnrelu', True, False), (128, 128, 'bn', False, False), (128, 128, 'mat', True, True), (128, 128, 'mat', False, False),
    (64, 384, 'mat', True, True), (64, 384, 'mat', False, False), (384, 64, 'bnrelu', True, False), (384, 64, 'bn', False, False),
    (32, 192, 'mat', False, True), (32, 192, 'mat', True, False), (192, 32, 'bnrelu', False, False), (192, 32, 'bn', True, False)])
@pytest.mark.parametrize('tiles', [8, 256 * 3 + 8])
def test_large_one_sweep_backward_within_the_exact_bound(Cin, Cout, variant, with_y, radd, tiles):
    """tss_pwconv_bwd_sweep, all five shapes (128 -> 128 pending and materialised).  8 tiles: one per block of the 8-block grid; 776 tiles:
    97 per XCD range over 32 blocks, so a block owns 4 or 3 (the last range 97 too: none is short)"""
    n = N_()
    TM = X.PWSWEEP_KINDS[(Cin, Cout)][0]
    P = TM * tiles
    D = Pw(801 + Cin + 3 * Cout + tiles, P, Cin, Cout, variant)
    L = D.L
    plan = X.pwsweep_rows(P, Cin, Cout)
    rows = plan[3]
    assert n.lib().tss_pwconv_bwd_sweep_rows(P, Cin, Cout) == rows and plan[4] == (1 if tiles == 8 else 4)
    g = torch.Generator().manual_seed(Cin + tiles)
    rd = X.dyadic((P, Cin), g, zero_frac=0.05) if radd else None
    rb = Buf(P, Cin, Cin + 4, 0, rd) if radd else None
    ob = Buf(P, Cin, Cin + 8, 4)
    sl = nan_slabs(Cin) if D.pending else None
    ws = torch.full((rows + 2, Cout * Cin), float('nan'), device=DEV)
    # a pixel count that is no multiple of the tile is refused, not rounded
    bad = sweep_call(D, D.pending, with_y, rb, ob, sl, ws, P - 8)
    assert getattr(n.lib(), bad[0])(*bad[1:]) == -2                 # TSS_ERR_SHAPE
    n.call(*sweep_call(D, D.pending, with_y, rb, ob, sl, ws, P))
    dw = torch.zeros(Cout, Cin, device=DEV)
    reduce_many([(ws, dw, Cout * Cin, rows)])
    torch.cuda.synchronize()
    what = ('sweep', Cin, Cout, variant, with_y, radd, tiles)
    w = ws.cpu()
    assert not torch.isnan(w[:rows]).any() and torch.isnan(w[rows:]).all(), (what, 'workspace rows')
    gop = D.gop(2 if with_y else 1)
    ref, S = X.conv_weight_ref(D.a(), (Cout, Cin, 1, 1), gop)
    ex = X.wgrad_excess(dw.double().cpu().reshape(ref.shape), ref, S, X.pwbwd_wgrad_chain(plan))
    assert ex <= 0, (what, 'weight gradient excess', ex)
    f = bwd_ref(gop, L.w, to_rows(L.mask()) if D.pending else None)

    def ref_fn(r0, r1):
        rin, Sin = f(r0, r1)
        return (rin + rd[r0:r1], Sin + rd[r0:r1].abs()) if radd else (rin, Sin)
    xc = D.xc()
    sums = check_blocked(ob, ref_fn, Cout + (1 if radd else 0), what, second=(lambda out, r0, r1: xc[r0:r1]) if D.pending else None)
    if D.pending:
        check_stats_sums(sl, sums, X.pwbwd_stats_chain(plan), ('sweep bstats',) + what, rows_used=rows)
