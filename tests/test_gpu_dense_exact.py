"""Each C entry point of the dense 3x3 family and the stem (csrc/wstat.hip, atrous.hip, conv3x3.hip, stem.hip and the 9-tap A_TAPS / A_STEM
paths of convgemm.hip and wgrad.hip), called once per case through _native.call, against f64 conv2d / conv2d_input / conv2d_weight on
dyadic operands (tests/exact.py), with the harness of tests/test_gpu_pw_exact.py (tests/exact_gpu.py): sentinel-filled output buffers
with a pitch wider than the channel count, a 16-byte column offset (tss_conv3x3_fwd / _bwd_data ask for 16-byte aligned outputs) and spare
rows behind, sentinel pad channels in the input pitches, NaN statistics slabs, NaN workspaces, and a dW that starts from a nonzero
dyadic value (the entries accumulate: one more rounding in the chain).

Bounds, all elementwise, none measured on the kernels, no element left out, no case skipped:
  forward / backward-data, bf16     X.conv_excess with K = 9 x contraction (exact products of bf16 operands, f32 sums in any order)
  forward / backward-data, f32      X.f32_excess with the same K on the UNROUNDED operands (X.act_f32 / X.gcomb_f32: products round too)
  statistics / bstats               X.stats_excess on the stored bits with the chain of the kernel that ran -- X.wstat_plan,
                                    X.stream_plan, X.lean3x3_plan, X.generic_stats_chain, X.stem_fwd_plan -- and the slab rows left in
                                    use against the restated grid (check_slab_rows); the f32 instances sum in f64
  weight gradients                  X.wgrad_excess with X.generic_wgrad_chain(P, Cin, N, 9) (f32: pt = 32, doubled), X.pw_wgrad_chain(P,
                                    9 Cin, N) behind tss_im2col3x3 (workspace count asserted against tss_pwconv_bwd_weight_ws),
                                    X.stem_wgrad_plan; + 1 for the dW they add onto
  tss_permute_w3x3 / _bf16, tss_im2col3x3     bit for bit (dyadic weights are bf16-exact; the unfold of X.act has zeros outside the image)
  everything around an output window           Buf.untouched()
The derivations are in the docstrings of tests/exact.py; tests/test_exact_bounds.py runs them on the CPU.

Dispatch.  Every instance is reached by its natural dispatch (TSS_CONV3X3_WSTAT / TSS_CONV3X3_STREAM are read once per process and are not
used); X.conv3x3_fwd_route / X.conv3x3_bwd_route restate tss_conv3x3_fwd's and tss_conv3x3_bwd_data's order of questions and every case
asserts the route it names:
  conv3x3_wstat_kernel<false | true>              materialised 128 -> 128, stride 1, dilation <= 18, H >= dilation, pitches % 8 == 0
  conv3x3_stream_kernel<4, true, false | true, 1>    the same layer where wstat declines: dilation 19 / 24, H < dilation, ldy = 140
  conv3x3_stream_kernel<0, false, false | true, 1>   materialised, Cin % 32 == 0 <= 128, N % 16 == 0 <= 128, not 128 -> 128
  conv3x3_lean_kernel<false, 2 | 3>               a pending BatchNorm and / or ReLU on the input, K in {32, 64, 128}, dilation 1 | 2, 18
  conv3x3_lean_kernel<true, 2 | 3>                tss_conv3x3_bwd_data with yraw, contraction in {32, 64, 128}, outputs % 16 == 0
  convgemm_kernel<bf16 | f32, false | true, A_TAPS>   whatever the lean kernels decline (the cases say why), and the f32 dtype
  wgrad_kernel<bf16 | f32>                        tss_conv3x3_bwd_weight (always), tss_stem3x3_bwd_weight with N = 16, ws == NULL or f32
  im2col3x3_kernel + wgfast_kernel                the composed weight gradient ops._dense_wgrad takes
  stem_fwd_mfma_kernel<float | bf16_t>, stem_wgrad_mfma_kernel<float | bf16_t>, stem_wgrad_kernel<bf16_t, float | bf16_t>,
  stem_wgrad_reduce_kernel, convgemm_kernel<., false, A_STEM>
Template instances the C entries cannot reach: none of wstat.hip, atrous.hip, conv3x3.hip or stem.hip.

Stem: where the image is rounded.  stem_fwd_mfma_kernel and stem_wgrad_mfma_kernel pack the taps as bf16 (V8<T>::store / (T)v), and so do
convgemm_kernel<bf16_t> (Xs = (T)v) and wgrad_kernel<bf16_t> (Pack4<bf16_t>): their references round the image with X.rne_bf16 first.
stem_wgrad_kernel (the VALU form, yraw == NULL) and the f32 instances of convgemm_kernel / wgrad_kernel keep the f32 image and the f32
g: their references use the unrounded image and X.gcomb_f32, and every product counts as a rounding (doubled chain).  The image lies in
a larger allocation with NaN around it (GuardedImage): the kernels select a tap or 0.f, so a tap from outside poisons the result."""
import pytest
import torch

from tests import exact as X
from tests.exact_gpu import (DEV, Buf, GuardedImage, Layer, N_, check_blocked, check_slab_rows, check_stats_sums, dev, nan_slabs, to_rows,
                             vecs)

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
VARIANTS = {'bnrelu': (True, True), 'bn': (True, False), 'relu': (False, True), 'mat': (False, False)}       # (pending BatchNorm, ReLU)
NO_X = (None, 0, None, None, None, 0)


class Ops(Layer):
    """Layer with a [N][Cin][3][3] weight and no conv bias; the backward operands only where a case needs them"""
    def __init__(self, seed, B, Cin, H, W, N, Ho, Wo, affine, relu, backward):
        g = torch.Generator().manual_seed(seed)
        self.draw_input(g, B, Cin, H, W, affine, relu)
        self.w = X.dyadic((N, Cin, 3, 3), g, emin=-6, emax=-2)
        self.cb = None
        if backward:
            self.draw_backward(g, N, Ho, Wo)


class Dense:
    """dyadic operands of a dense 3x3 layer Cin -> N (padding = dilation) and their device buffers in one dtype; the four weight layouts
    come from tss_permute_w3x3 / tss_permute_w3x3_bf16 and are compared bit for bit with the permuted reference"""
    def __init__(self, seed, B, H, W, Cin, N, dil=1, stride=1, variant='mat', dtype=BF, backward=False):
        n = N_()
        affine, relu = VARIANTS[variant]
        self.B, self.H, self.W, self.Cin, self.N, self.dil, self.stride, self.dtype = B, H, W, Cin, N, dil, stride, dtype
        self.Ho, self.Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        self.P, self.Pin = B * self.Ho * self.Wo, B * H * W
        self.pending, self.relu = affine, relu
        self.L = L = Ops(seed + 7 * H + 3 * W + Cin + 5 * N + dil, B, Cin, H, W, N, self.Ho, self.Wo, affine, relu, backward)
        self.code, self.st = n.dtype_code(dtype), n.stream()
        self.v = v = vecs(L)
        self.xb = Buf(self.Pin, Cin, Cin + 8, 0, to_rows(L.x), dtype)
        self.xargs = (self.xb.ptr, self.xb.ld, n.ptr(v['mean']), n.ptr(v['scale']), n.ptr(v['bias']), int(relu))
        self.wt = dev(L.w)
        nan = lambda *s: torch.full(s, float('nan'), device=DEV)
        self.w_tnc, self.w_tcn = nan(9, N, Cin), nan(9, Cin, N)
        self.b_tnc, self.b_tcn = nan(9, N, Cin).to(BF), nan(9, Cin, N).to(BF)
        n.call('tss_permute_w3x3', n.ptr(self.wt), n.ptr(self.w_tnc), n.ptr(self.w_tcn), N, Cin, self.st)
        n.call('tss_permute_w3x3_bf16', n.ptr(self.wt), n.ptr(self.b_tnc), n.ptr(self.b_tcn), N, Cin, self.st)
        torch.cuda.synchronize()
        tnc, tcn = L.w.permute(2, 3, 0, 1).reshape(9, N, Cin).float(), L.w.permute(2, 3, 1, 0).reshape(9, Cin, N).float()
        for got, want in ((self.w_tnc, tnc), (self.w_tcn, tcn), (self.b_tnc, tnc.to(BF)), (self.b_tcn, tcn.to(BF))):
            assert torch.equal(X.bits(got.cpu()), X.bits(want)), 'permuted weights differ'
        self.eb = None

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
            self.eb = Buf(self.P, self.N, self.N + 16, 0, to_rows(L.e), self.dtype)
            self.yrb = Buf(self.P, self.N, self.N + 8, 0, to_rows(L.y), self.dtype)
        if mode == 2:
            return (self.eb.ptr, self.eb.ld, self.yrb.ptr, self.yrb.ld, n.ptr(v['ga']), n.ptr(v['gb']), n.ptr(v['gce']), n.ptr(v['gmu']))
        return (self.eb.ptr, self.eb.ld, None, 0, n.ptr(v['ga']), None, None, None)

    def xc(self):
        return to_rows(self.L.x - (self.L.mean if self.pending else 0))

    def kw(self):
        return dict(stride=self.stride, padding=self.dil, dilation=self.dil)


def out_excess(dtype):
    return X.conv_excess if dtype == BF else X.f32_excess


def sliced(ref, S, mask=None):
    ref, S = to_rows(ref), to_rows(S)
    if mask is not None:
        ref, S = ref * mask, S * mask
    return lambda r0, r1: (ref[r0:r1], S[r0:r1])


# ----------------------------------------------------------------------------------------------------- tss_conv3x3_fwd
def run_fwd(B, H, W, Cin, N, dil, variant, stats, route, stride=1, ldy=None, dtype=BF, shadow=True, seed=0):
    n = N_()
    D = Dense(seed, B, H, W, Cin, N, dil, stride, variant, dtype)
    ldy = ldy or N + 16
    assert X.conv3x3_fwd_route(H, Cin, N, stride, dil, D.pending, D.relu, D.xb.ld, ldy, shadow, dtype == BF) == route
    yb, sl = Buf(D.P, N, ldy, 8, dtype=dtype), (nan_slabs(N) if stats else None)
    n.call('tss_conv3x3_fwd', *D.xargs, n.ptr(D.w_tnc), n.ptr(D.b_tnc) if shadow else None, yb.ptr, yb.ld, n.ptr(sl),
           B, H, W, Cin, N, stride, dil, D.code, D.st)
    torch.cuda.synchronize()
    what = ('fwd', route, B, H, W, Cin, N, dil, variant)
    ref, S = X.conv_ref(D.a(), D.L.w, **D.kw())
    sums = check_blocked(yb, sliced(ref, S), 9 * Cin, what, second=(lambda out, r0, r1: out) if stats else None, excess=out_excess(dtype))
    if not stats:
        return
    owners = None
    if route == 'wstat':
        plan = X.wstat_plan(B, H, W, dil)
        chain, owners = plan['chain'], range(plan['grid'])
    elif route.startswith('stream'):
        chain, owners, _ = X.stream_plan(D.P)
    elif route.startswith('lean'):
        chain, owners, _ = X.lean3x3_plan(B, H, W)
    else:
        chain = X.generic_stats_chain(D.P, N)
    check_stats_sums(sl, sums, chain, ('fwd stats',) + what, f64=dtype == F32)
    if owners is not None:
        check_slab_rows(sl, owners, what)


@pytest.mark.parametrize('stats', [False, True])
def test_weight_stationary_forward_with_one_row_per_block(stats):
    """conv3x3_wstat_kernel<false | true>: 2 x 2 strips x 9 rows = 36 units on 36 blocks, the second strip 6 pixels wide"""
    assert X.wstat_plan(2, 9, 70, 1)['rows'] == 1
    run_fwd(2, 9, 70, 128, 128, 1, 'mat', stats, 'wstat')


RING = (3, 100, 321)      # 3 x 6 strips x 100 rows = 1 800 units >= 6 x 256 on 96 300 pixels; the last strip is one pixel wide


def test_weight_stationary_ranges_reach_the_ring_steady_state_and_every_boundary():
    """the restated walk (X.wstat_plan): a block owns 7 or 8 units; at every dilation used below some range runs more than 4 consecutive
    rows of one walk (the four ring slots wrap), and the ranges cross a strip and an image boundary, at D = 7 and 18 a class boundary
    too; at D = 18 a class has 5 or 6 rows, so every range spans two walks"""
    for D, cross in ((1, {'strip', 'image'}), (7, {'class', 'strip', 'image'}), (18, {'class', 'strip', 'image'})):
        plan = X.wstat_plan(*RING, D)
        assert plan['grid'] == 256 and plan['rows'] == 8 and plan['run'] > 4 and plan['cross'] == cross, plan
    assert all(len(X.wstat_segments(lo, hi, RING[1], RING[2], 18)) >= 2 for lo, hi in X.wstat_ranges(*RING))


@pytest.mark.parametrize('D,stats', [(1, True), (7, False), (18, True), (18, False)])
def test_weight_stationary_forward_in_the_ring_steady_state(D, stats):
    run_fwd(*RING, 128, 128, D, 'mat', stats, 'wstat')


# H == D (every class one row), H == D + 1 (class 0 has two), W < D (every horizontal tap outside), W = 64 and 65 (a second strip of 1)
@pytest.mark.parametrize('B,H,W,D,stats', [(2, 6, 70, 6, True), (2, 7, 65, 6, False), (2, 20, 5, 18, True), (2, 9, 64, 2, False),
                                           (2, 9, 65, 2, True)])
def test_weight_stationary_forward_at_the_dilation_edges(B, H, W, D, stats):
    run_fwd(B, H, W, 128, 128, D, 'mat', stats, 'wstat')


# the three routes past wstat for 128 -> 128: dilation > 18, H < dilation, ldy = 140 = 4 (mod 8).  P is no multiple of 256 and a
# 256-pixel tile straddles two images: 3 x 25 x 37 = 2 775 (an image is 925 pixels), 3 x 5 x 37 = 555 (185), 3 x 11 x 37 = 1 221 (407)
@pytest.mark.parametrize('H,D,ldy', [(25, 19, None), (25, 24, None), (5, 6, None), (11, 3, 140)])
@pytest.mark.parametrize('stats', [False, True])
def test_streamed_forward_straight_line_instance_on_each_route_past_wstat(H, D, ldy, stats):
    run_fwd(3, H, 37, 128, 128, D, 'mat', stats, 'stream<4, true>', ldy=ldy)


@pytest.mark.parametrize('Cin,N,D,stats', [(32, 16, 1, True), (96, 48, 3, False), (64, 128, 19, True), (128, 112, 2, False), (128, 112, 5, True),
                                           (32, 16, 2, False)])
def test_streamed_forward_general_instance(Cin, N, D, stats):
    run_fwd(3, 11, 37, Cin, N, D, 'mat', stats, 'stream<0, false>')


def test_streamed_forward_with_two_tiles_per_block():
    """32 -> 16 at 2 x 257 x 257 = 132 098 pixels = 516 tiles of 256 + 2 pixels: 65 per XCD range over 64 blocks, so a block owns 2 or 1; the
    last range has 62 tiles, so its last two blocks own none and their slab rows stay zero"""
    chain, owners, grid = X.stream_plan(2 * 257 * 257)
    assert (chain, grid, len(owners)) == (4 * 2 + 4, 512, 510) and len(X.stream_tiles(0, 2 * 257 * 257)) == 2
    run_fwd(2, 257, 257, 32, 16, 2, 'mat', True, 'stream<0, false>')


# conv3x3_lean_kernel<false, 2> (D = 1) and <false, 3> (D = 2, 18): K x N x W in a Latin square over the three pending variants, H = 3
# (every fourth case without statistics)
LEAN_FWD = [(K, N, (5, 64, 65)[(i + j + d) % 3], D, ('bnrelu', 'bn', 'relu')[(i + 2 * j + d) % 3], (i + j + 2 * d) % 4 != 0)
            for i, K in enumerate((32, 64, 128)) for j, N in enumerate((16, 48, 128)) for d, D in enumerate((1, 2, 18))]


@pytest.mark.parametrize('K,N,W,D,variant,stats', LEAN_FWD)
def test_lean_forward_with_a_pending_input_transform(K, N, W, D, variant, stats):
    run_fwd(2, 3, W, K, N, D, variant, stats, 'lean<false, 2>' if D == 1 else 'lean<false, 3>')


def test_lean_forward_with_blocks_that_loop_over_tiles():
    """2 x 130 rows x 2 tiles = 520 tiles on 512 blocks: the first 8 blocks own two"""
    assert X.lean3x3_plan(2, 130, 65) == (2 * 2 + 4, list(range(512)), 512)
    run_fwd(2, 130, 65, 32, 16, 1, 'bnrelu', True, 'lean<false, 2>')


# convgemm_kernel, 9 taps: a pending BatchNorm at dilation 19 (past the lean kernel's 18), Cin = 40 and N = 20 (outside its channel sets; N = 20
# with ldy = 28 = 4 (mod 8)), stride 2 with Cin = 128 and with dilation 2 (sconv.hip takes only Cin <= 64 at dilation 1), no bf16 copy, f32
GENERIC_FWD = [(2, 21, 23, 32, 16, 19, 1, 'bnrelu', None, BF, True), (2, 7, 19, 40, 16, 1, 1, 'bnrelu', None, BF, True),
               (2, 7, 19, 32, 20, 2, 1, 'mat', 28, BF, True), (2, 9, 14, 128, 32, 1, 2, 'bn', None, BF, True),
               (2, 10, 13, 32, 16, 2, 2, 'relu', None, BF, True), (2, 7, 19, 32, 16, 1, 1, 'mat', None, BF, False),
               (2, 7, 19, 40, 20, 2, 1, 'bnrelu', None, F32, True), (2, 9, 14, 16, 136, 1, 2, 'mat', None, F32, True)]


@pytest.mark.parametrize('B,H,W,Cin,N,D,stride,variant,ldy,dtype,shadow', GENERIC_FWD)
def test_generic_nine_tap_forward(B, H, W, Cin, N, D, stride, variant, ldy, dtype, shadow):
    run_fwd(B, H, W, Cin, N, D, variant, True, 'generic', stride=stride, ldy=ldy, dtype=dtype, shadow=shadow)


# ----------------------------------------------------------------------------------------------------- tss_conv3x3_bwd_data
def run_bwd(B, H, W, Cin, N, dil, variant, mode, route, dtype=BF, shadow=True, seed=100):
    """contraction over the N channels of e (and y), outputs the Cin channels of e_in; a pending variant passes xraw (ReLU mask + bstats)"""
    n = N_()
    D = Dense(seed, B, H, W, Cin, N, dil, 1, variant, dtype, backward=True)
    L = D.L
    assert X.conv3x3_bwd_route(Cin, N, dil, mode == 2, shadow, dtype == BF) == route
    with_x = variant != 'mat'
    ob, sl = Buf(D.Pin, Cin, Cin + 16, 8, dtype=dtype), (nan_slabs(Cin) if with_x else None)
    n.call('tss_conv3x3_bwd_data', *D.gargs(mode), n.ptr(D.w_tcn), n.ptr(D.b_tcn) if shadow else None, *(D.xargs if with_x else NO_X),
           ob.ptr, ob.ld, n.ptr(sl), B, H, W, Cin, N, dil, D.code, D.st)
    torch.cuda.synchronize()
    what = ('bwd data', route, B, H, W, Cin, N, dil, variant, mode)
    ref, S = X.conv_input_ref(L.x.shape, L.w, D.gop(mode), padding=dil, dilation=dil)
    xc = D.xc()
    sums = check_blocked(ob, sliced(ref, S, to_rows(L.mask()) if with_x else None), 9 * N, what,
                         second=(lambda out, r0, r1: xc[r0:r1]) if with_x else None, excess=out_excess(dtype))
    if with_x:
        if route.startswith('lean'):
            chain, owners, _ = X.lean3x3_plan(B, H, W)
            check_slab_rows(sl, owners, what)
        else:
            chain = X.generic_stats_chain(D.Pin, Cin)
        check_stats_sums(sl, sums, chain, ('bstats',) + what, f64=dtype == F32)


# conv3x3_lean_kernel<true, 2 | 3>: contraction (N) x outputs (Cin) x W, with the producer's raw output (mask + bstats) and without
LEAN_BWD = [(Cin, N, (5, 64, 65)[(i + j + d) % 3], D, ('bnrelu', 'mat', 'relu', 'bn')[(i + j + 2 * d) % 4])
            for i, N in enumerate((32, 64, 128)) for j, Cin in enumerate((16, 48, 128)) for d, D in enumerate((1, 2, 18)) if (i + j + d) % 2 == 0 or D == 1]


@pytest.mark.parametrize('Cin,N,W,D,variant', LEAN_BWD)
def test_lean_backward_data(Cin, N, W, D, variant):
    run_bwd(2, 4, W, Cin, N, D, variant, 2, 'lean<true, 2>' if D == 1 else 'lean<true, 3>')


def test_lean_backward_data_with_blocks_that_loop_over_tiles():
    run_bwd(2, 130, 65, 16, 32, 1, 'bnrelu', 2, 'lean<true, 2>')


# convgemm_kernel<., false | true, A_TAPS>, tap_sign = -1: yraw == NULL (g = ga e), contraction 40, outputs 20, dilation 19, f32
@pytest.mark.parametrize('B,H,W,Cin,N,D,variant,mode,dtype', [
    (2, 5, 19, 32, 32, 1, 'bnrelu', 1, BF), (2, 5, 19, 16, 40, 2, 'mat', 2, BF), (2, 5, 19, 20, 32, 1, 'bnrelu', 2, BF),
    (2, 21, 23, 32, 32, 19, 'relu', 2, BF), (2, 5, 19, 20, 40, 2, 'bnrelu', 2, F32), (2, 5, 19, 32, 32, 1, 'mat', 1, F32)])
def test_generic_nine_tap_backward_data(B, H, W, Cin, N, D, variant, mode, dtype):
    run_bwd(B, H, W, Cin, N, D, variant, mode, 'generic', dtype=dtype)


# ----------------------------------------------------------------------------------------------------- weight gradients
def dw_start(shape, seed):
    """the nonzero dyadic value the accumulating entries add onto"""
    return X.dyadic(shape, torch.Generator().manual_seed(seed), emin=-2, emax=1)


@pytest.mark.parametrize('stride,D', [(1, 1), (1, 3), (2, 1), (2, 3)])
@pytest.mark.parametrize('mode', [2, 1])
@pytest.mark.parametrize('dtype', [BF, F32])
def test_nine_tap_weight_gradient_lands_in_the_torch_layout(stride, D, mode, dtype):
    """tss_conv3x3_bwd_weight: wgrad_kernel over 9 taps x 2 contraction chunks (Cin = 136), f32 atomics onto dW [N][Cin][3][3]"""
    n = N_()
    B, H, W, Cin, N = 2, 9, 21, 136, 24
    V = Dense(200 + mode, B, H, W, Cin, N, D, stride, ('bnrelu', 'relu')[mode - 1], dtype, backward=True)
    dw0 = dw_start((N, Cin, 3, 3), stride + D)
    dw = dev(dw0)
    n.call('tss_conv3x3_bwd_weight', *V.gargs(mode), *V.xargs, n.ptr(dw), B, H, W, Cin, N, stride, D, V.code, V.st)
    torch.cuda.synchronize()
    ref, S = X.conv_weight_ref(V.a(), (N, Cin, 3, 3), V.gop(mode), **V.kw())
    chain = X.generic_wgrad_chain(V.P, Cin, N, 9) if dtype == BF else 2 * X.generic_wgrad_chain(V.P, Cin, N, 9, pt=32)
    ex = X.wgrad_excess(dw.double().cpu(), ref + dw0, S + dw0.abs(), chain + 1)
    assert ex <= 0, ('conv3x3 wgrad', stride, D, mode, dtype, ex)


@pytest.mark.parametrize('C,D,W', [(8, 1, 19), (24, 2, 19), (128, 1, 7), (8, 9, 7), (24, 1, 1), (128, 2, 19)])
@pytest.mark.parametrize('variant', ['bnrelu', 'bn', 'relu', 'mat'])
def test_unfold_is_the_activated_input_bit_for_bit(C, D, W, variant):
    """tss_im2col3x3: col[p][c 9 + tap] = act(x)[p + off(tap)][c], 0 where the tap leaves the image (D = 9 > W = 7: every horizontal tap)"""
    n = N_()
    B, H = 2, 5
    V = Dense(300, B, H, W, C, 8, D, 1, variant)
    col = Buf(V.P, 9 * C, 9 * C)
    n.call('tss_im2col3x3', *V.xargs, col.ptr, B, H, W, C, D, V.code, V.st)
    torch.cuda.synchronize()
    want = torch.nn.functional.unfold(V.a(), 3, dilation=D, padding=D).permute(0, 2, 1).reshape(V.P, 9 * C)
    assert torch.equal(X.bits(col.t[:V.P].cpu()), X.bits(want.to(BF))) and col.untouched()


@pytest.mark.parametrize('B,H,W,Cin,N,D,variant', [(2, 9, 21, 24, 16, 1, 'bnrelu'), (2, 9, 21, 32, 136, 2, 'relu'), (2, 30, 33, 128, 128, 1, 'bn')])
def test_composed_weight_gradient_through_the_unfold(B, H, W, Cin, N, D, variant):
    """tss_im2col3x3 then tss_pwconv_bwd_weight with K = 9 Cin (wgfast_kernel + its slot reduction), as ops._dense_wgrad composes them"""
    n = N_()
    V = Dense(400, B, H, W, Cin, N, D, 1, variant, backward=True)
    K = 9 * Cin
    col = Buf(V.P, K, K)
    n.call('tss_im2col3x3', *V.xargs, col.ptr, B, H, W, Cin, D, V.code, V.st)
    chain, nws = X.pw_wgrad_chain(V.P, K, N)
    assert n.lib().tss_pwconv_bwd_weight_ws(V.P, K, N, n.TSS_BF16) == nws
    ws = torch.full((nws + 64,), float('nan'), device=DEV)
    dw0 = dw_start((N, Cin, 3, 3), Cin)
    dw = dev(dw0)
    n.call('tss_pwconv_bwd_weight', *V.gargs(2), col.ptr, col.ld, None, None, None, 0, n.ptr(dw), n.ptr(ws), 0, V.P, K, N, V.code, None, V.st)
    torch.cuda.synchronize()
    assert torch.isnan(ws[nws:]).all() and col.untouched()
    ref, S = X.conv_weight_ref(V.a(), (N, Cin, 3, 3), V.gop(2), padding=D, dilation=D)
    ex = X.wgrad_excess(dw.double().cpu(), ref + dw0, S + dw0.abs(), chain + 1)
    assert ex <= 0, ('composed wgrad', Cin, N, D, ex, 'chain', chain)


# ----------------------------------------------------------------------------------------------------- stem
STEM_W, STEM_H = (1, 2, 3, 4, 5, 7, 8, 70), (1, 2, 9)


class Stem:
    """operands of the stem Cin -> N over a B x Cin x Hin x Win image of one kind: 'f32' (24-bit significands), 'dyadic' (f32 storage,
    bf16-exact values) or 'bf16' (x_is_f32 = 0: the image in the activations' dtype)"""
    def __init__(self, seed, B, Cin, Hin, Win, N, stride, kind, dtype=BF):
        n = N_()
        g = torch.Generator().manual_seed(seed)
        self.B, self.Cin, self.Hin, self.Win, self.N, self.stride, self.dtype = B, Cin, Hin, Win, N, stride, dtype
        self.Ho, self.Wo = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
        self.P = B * self.Ho * self.Wo
        self.x = X.full_f32((B, Cin, Hin, Win), g) if kind == 'f32' else X.dyadic((B, Cin, Hin, Win), g, zero_frac=0.04)
        self.is_f32 = int(kind != 'bf16')
        self.img = GuardedImage(self.x, F32 if (self.is_f32 or dtype == F32) else BF)
        self.w = X.dyadic((N, Cin, 3, 3), g, emin=-6, emax=-2)
        self.wd = dev(self.w)
        self.draw_backward = Layer.draw_backward.__get__(self)
        self.draw_backward(g, N, self.Ho, self.Wo)
        self.v = vecs(self)
        self.code, self.st = n.dtype_code(dtype), n.stream()
        self.eb = Buf(self.P, N, N + 16, 0, to_rows(self.e), dtype)
        self.yrb = Buf(self.P, N, N + 8, 0, to_rows(self.y), dtype)

    def image(self, rounded):
        return X.rne_bf16(self.x) if rounded else self.x

    def gargs(self, mode):
        n, v = N_(), self.v
        if mode == 2:
            return (self.eb.ptr, self.eb.ld, self.yrb.ptr, self.yrb.ld, n.ptr(v['ga']), n.ptr(v['gb']), n.ptr(v['gce']), n.ptr(v['gmu']))
        return (self.eb.ptr, self.eb.ld, None, 0, n.ptr(v['ga']), None, None, None)

    def gop(self, mode, rounded):
        f = X.gcomb if rounded else X.gcomb_f32
        return f(self.e, self.y, self.ga, self.gb, self.gce, self.gmu) if mode == 2 else f(self.e, ga=self.ga)

    def forward(self, stats, direct):
        """tss_stem3x3_fwd; direct: stem_fwd_mfma_kernel (bf16, N = 32), else convgemm_kernel<., false, A_STEM>"""
        n = N_()
        bf = self.dtype == BF
        assert direct == (bf and self.Cin <= 3 and self.N == 32)
        yb, sl = Buf(self.P, self.N, self.N + 16, 8, dtype=self.dtype), (nan_slabs(self.N) if stats else None)
        n.call('tss_stem3x3_fwd', self.img.ptr, self.is_f32, n.ptr(self.wd), yb.ptr, yb.ld, n.ptr(sl), self.B, self.Cin, self.Hin, self.Win,
               self.N, self.stride, self.code, self.st)
        torch.cuda.synchronize()
        what = ('stem fwd', self.Cin, self.Hin, self.Win, self.N, self.stride, self.is_f32, self.dtype)
        ref, S = X.conv_ref(self.image(bf), self.w, stride=self.stride, padding=1)
        sums = check_blocked(yb, sliced(ref, S), 9 * self.Cin, what, second=(lambda out, r0, r1: out) if stats else None,
                             excess=out_excess(self.dtype))
        if stats:
            chain, owners, _ = X.stem_fwd_plan(self.P) if direct else (X.generic_stats_chain(self.P, self.N), None, None)
            check_stats_sums(sl, sums, chain, ('stem stats',) + what, f64=not bf)
            if direct:
                check_slab_rows(sl, owners, what)

    def wgrad(self, mode, with_ws, kernel):
        """tss_stem3x3_bwd_weight; kernel: 'mfma' (mode 2, ws), 'valu' (yraw == NULL, ws), 'generic' (wgrad_kernel, A_STEM)"""
        n = N_()
        bf = self.dtype == BF
        direct = bf and self.Cin <= 3 and self.N == 32 and with_ws
        assert kernel == (('mfma' if mode == 2 else 'valu') if direct else 'generic')
        slabs = n.stat_slabs()
        ws = torch.full((slabs + 2, 32 * 28), float('nan'), device=DEV) if with_ws else None
        dw0 = dw_start((self.N, self.Cin, 3, 3), self.Win)
        dw = dev(dw0)
        n.call('tss_stem3x3_bwd_weight', *self.gargs(mode), self.img.ptr, self.is_f32, n.ptr(dw), n.ptr(ws), self.B, self.Cin, self.Hin,
               self.Win, self.N, self.stride, self.code, self.st)
        torch.cuda.synchronize()
        what = ('stem wgrad', kernel, self.Cin, self.Hin, self.Win, self.N, self.stride, self.is_f32, self.dtype, mode)
        rounded = bf and kernel != 'valu'
        if direct:
            chain, rows = X.stem_wgrad_plan(self.P, kernel == 'mfma')
            w = ws.cpu()
            assert not torch.isnan(w[:rows]).any() and torch.isnan(w[rows:]).all(), (what, 'workspace rows')
        else:
            chain = X.generic_wgrad_chain(self.P, 9 * self.Cin, self.N, 1) if bf else 2 * X.generic_wgrad_chain(self.P, 9 * self.Cin, self.N, 1, pt=32)
            assert ws is None or torch.isnan(ws).all(), (what, 'the generic kernel wrote the workspace')
        ref, S = X.conv_weight_ref(self.image(rounded), (self.N, self.Cin, 3, 3), self.gop(mode, rounded), stride=self.stride, padding=1)
        ex = X.wgrad_excess(dw.double().cpu(), ref + dw0, S + dw0.abs(), chain + 1)
        assert ex <= 0, (what, 'weight gradient excess', ex, 'chain', chain)


@pytest.mark.parametrize('stride', [2, 1])
@pytest.mark.parametrize('Cin', [1, 2, 3])
@pytest.mark.parametrize('kind', ['f32', 'dyadic', 'bf16'])
def test_stem_direct_kernels_at_every_window_edge(stride, Cin, kind):
    """stem_fwd_mfma_kernel / stem_wgrad_mfma_kernel / stem_wgrad_kernel<bf16_t, .> + stem_wgrad_reduce_kernel over Win x Hin: stem_taps'
    16-byte window (f32, stride 2, Win >= 4) clamped at both row ends, its per-tap form everywhere else; B = 2 so that a tap past the last
    row or column of image 0 would land in image 1"""
    for i, Win in enumerate(STEM_W):
        for j, Hin in enumerate(STEM_H):
            s = Stem(500 + 31 * Win + Hin + Cin, 2, Cin, Hin, Win, 32, stride, kind)
            s.forward((i + j) % 2 == 0, True)
            s.wgrad(2, True, 'mfma')
            s.wgrad(1, True, 'valu')
            if (i + j) % 3 == 0:
                s.wgrad(2, False, 'generic')


@pytest.mark.parametrize('N,dtype,kind,stride,Cin,Hin,Win', [(16, BF, 'f32', 2, 3, 9, 7), (16, BF, 'bf16', 1, 2, 2, 5), (32, F32, 'f32', 2, 3, 9, 70),
                                                             (16, F32, 'bf16', 1, 1, 9, 4), (32, F32, 'dyadic', 2, 2, 1, 8)])
def test_stem_generic_kernels(N, dtype, kind, stride, Cin, Hin, Win):
    """N = 16 and the f32 dtype take convgemm_kernel<., false, A_STEM> and wgrad_kernel; with dtype f32 and x_is_f32 = 0 the image is f32 too"""
    s = Stem(600 + N + Win, 2, Cin, Hin, Win, N, stride, kind, dtype)
    s.forward(True, False)
    for mode in (2, 1):
        s.wgrad(mode, True, 'generic')
    s.wgrad(2, False, 'generic')


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_stem_direct_kernels_with_blocks_that_own_two_tiles(kind):
    """1 x 3 x 520 x 1024 at stride 2: 260 x 512 = 133 120 output pixels = 520 tiles of 256 on 512 blocks"""
    s = Stem(700, 1, 3, 520, 1024, 32, 2, kind)
    assert X.stem_fwd_plan(s.P) == (4 * 2 + 4, list(range(512)), 512) and X.stem_wgrad_plan(s.P, True) == (64 * 2 + 3 + 32 + 16 + 1, 512)
    s.forward(True, True)
    s.wgrad(2, True, 'mfma')
    s.wgrad(1, True, 'valu')
