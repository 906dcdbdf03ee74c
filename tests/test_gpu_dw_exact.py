"""Each C entry point of the depthwise 3x3 family (csrc/dwconv.hip, dwroll.hip, updw.hip), called once per case through _native.call,
against f64 on dyadic operands (tests/exact.py), with the harness tests/test_gpu_zoo_exact.py uses (tests/exact_gpu.py): sentinel-padded buffers with spare
rows, NaN statistics slabs and NaN workspace rows, planted exact zeros of the pre-activation.

These kernels keep the activated operand a and the backward operand g in f32 and their weights are f32 (24 significant bits, drawn from
a normal distribution here), so the references use the UNROUNDED a and g (X.act_f32 / X.gcomb_f32) and every term carries the rounding
of its product besides those of the additions: conv_excess(.., 9) for bf16 outputs, f32_excess(.., 9) for the f32 instances,
wgrad_excess with the chain of the kernel that ran (X.dw_wgrad_chain, X.roll_wgrad_chain, X.updw_wgrad_chain), stats_excess on the stored
output bits (X.dw_stats_chain, X.roll_stats_chain, X.updw_stats_chain).  No tolerance is measured on the kernels, no element is left
out, no case is skipped: where a case is meant for one kernel, the matching *_supported / *_preferred / *_rows entry is asserted.

tss_updw_*: the interpolated pixel is rounded to bf16 on load.  At dyadic size pairs (Ho - 1 = 2^k (Hs - 1), likewise W) ac_tap's
weights are exact multiples of 2^-k, the blend is exact in f32 (tests/test_exact_bounds.py) and the reference operand is
X.upsampled_operand's rounded map: the hard bound.  At the other size pairs the kernel's f32 blend is off by at most
X.bilinear_f32_slack before its rounding, so its operand is within 2^-8 (|v| + slack) + slack of the unrounded v: the
reference is the convolution of v and the bound grows by that amount times the absolute weights (or gradients).

Template instances the C entry points cannot reach: dw_bwd_data_strip_kernel<float, S, D, true> is never instantiated
(launch_strip_fused is bf16 only: the f32 path keeps the two separate kernels)."""
import ctypes

import pytest
import torch

from tests import exact as X
from tests.exact_gpu import DEV, Buf, Layer, N_, check_out, check_stats, dev, env, nan_slabs, reduce_many, to_rows, vecs

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
VARIANTS = {'bnrelu': (True, True), 'bn': (True, False), 'mat': (False, False)}       # (pending BatchNorm, ReLU)


class DwLayer(Layer):
    """dyadic operands of a depthwise 3x3 layer (padding = dilation): Layer's x, BatchNorm vectors, e, y and (ga, gb, gce, gmu); f32
    weights [C][1][3][3] with full significands; a and g unrounded"""
    def __init__(self, seed, B, C, H, W, stride, variant='bnrelu'):
        affine, relu = VARIANTS[variant]
        g = torch.Generator().manual_seed(seed)
        self.C, self.stride, self.cb = C, stride, None
        self.draw_input(g, B, C, H, W, affine, relu)
        self.w = (torch.randn((C, 1, 3, 3), generator=g) * 0.25).float().double()
        self.draw_backward(g, C, (H - 1) // stride + 1, (W - 1) // stride + 1)

    def a(self):
        return X.act_f32(self.x, self.mean, self.scale, self.bias, self.relu)

    def gop(self, mode):
        """mode 0: g = e; 1: g = ga e; 2: the BatchNorm-backward combination"""
        if mode == 2:
            return X.gcomb_f32(self.e, self.y, self.ga, self.gb, self.gce, self.gmu)
        return X.gcomb_f32(self.e, ga=self.ga) if mode == 1 else self.e

    def xc(self):
        return to_rows(self.x - (self.mean if self.mean is not None else 0))


class Dev:
    """device operands of a DwLayer in one dtype"""
    def __init__(self, L, dtype):
        N = N_()
        self.L, self.dtype, self.code, self.st = L, dtype, N.dtype_code(dtype), N.stream()
        self.v = vecs(L)
        self.w = dev(L.w.reshape(L.C, 9))
        P, Po, C = L.B * L.H * L.W, L.B * L.Ho * L.Wo, L.C
        self.P, self.Po = P, Po
        self.xb = Buf(P, C, C + 8, 0, to_rows(L.x), dtype)
        self.eb = Buf(Po, C, C + 16, 0, to_rows(L.e), dtype)
        self.yb = Buf(Po, C, C + 8, 0, to_rows(L.y), dtype)
        v = self.v
        self.xargs = (self.xb.ptr, self.xb.ld, N.ptr(v['mean']), N.ptr(v['scale']), N.ptr(v['bias']), int(L.relu))

    def gargs(self, mode):
        N, v = N_(), self.v
        if mode == 2:
            return (self.eb.ptr, self.eb.ld, self.yb.ptr, self.yb.ld, N.ptr(v['ga']), N.ptr(v['gb']), N.ptr(v['gce']), N.ptr(v['gmu']))
        return (self.eb.ptr, self.eb.ld, None, 0, N.ptr(v['ga']) if mode == 1 else None, None, None, None)

    def out(self, P, off=8):
        return Buf(P, self.L.C, self.L.C + 16, off, dtype=self.dtype)


def check_any(buf, ref, S, what):
    """an output buffer of either dtype under its bound (K = 9 taps), sentinels intact"""
    if buf.t.dtype == BF:
        return check_out(buf, ref, S, 9, what)
    out = buf.rows()
    ex = X.f32_excess(out, ref, S, 9)
    assert ex <= 0, (what, 'excess over the bound', ex)
    assert buf.untouched(), (what, 'sentinel overwritten')
    return out


def check_stats_any(slabs, terms, chain, dtype, what):
    """bf16 instances add a lane's terms in f32 (chain); f32 instances in f64 throughout (StatAcc<float>): terms exact in f64 (24 x 24
    bits), fewer than 2^13 per sum: within 2^-40 sum|terms|"""
    if dtype == BF:
        return check_stats(slabs, terms, chain, what)
    s = slabs.double().cpu()
    assert not torch.isnan(s).any(), (what, 'a slab row neither written nor zeroed')
    assert ((s.sum(0) - terms.sum(0)).abs() <= 2.0 ** -40 * terms.abs().sum(0)).all(), what


def new_ws(C, rows=None):
    return torch.full((rows or N_().stat_slabs(), C * 9), float('nan'), device=DEV)


def check_dw(dw, ref, S, chain, what):
    ex = X.wgrad_excess(dw.double().cpu().reshape(ref.shape), ref, S, chain)
    assert ex <= 0, (what, 'weight gradient excess', ex, 'chain', chain)


def check_rows(ws, rows, what):
    w = ws.cpu()
    assert not torch.isnan(w[:rows]).any(), (what, 'a workspace row not written')
    assert torch.isnan(w[rows:]).all(), (what, 'a workspace row beyond the grid written')


def path_of(C, stride, dil, dtype, roll_on=True):
    if roll_on and dtype == BF and dil == 1 and stride in (1, 2):
        return 'roll'
    return 'strip' if X.dw_strip_pair(stride, dil) else 'generic'


# ----------------------------------------------------------------------------------------------------- forward
def run_fwd(C, B, H, W, stride, dil, variant, dtype, roll=True, seed=0, multi_unit=False, seg_carry=False):
    N = N_()
    L = DwLayer(seed + C + 3 * W + H + dil, B, C, H, W, stride, variant)
    D = Dev(L, dtype)
    path = path_of(C, stride, dil, dtype, roll)
    ref, S = X.conv_ref(L.a(), L.w, stride=stride, padding=dil, dilation=dil, groups=C)
    ref, S = to_rows(ref), to_rows(S)
    yb, sl = D.out(D.Po), nan_slabs(C)
    with env(TSS_DW_ROLL=1 if roll else 0):
        N.call('tss_dwconv3x3_fwd', *D.xargs, N.ptr(D.w), yb.ptr, yb.ld, N.ptr(sl), B, H, W, C, stride, dil, D.code, D.st)
        torch.cuda.synchronize()
    out = check_any(yb, ref, S, ('fwd', path))
    if path == 'roll':
        plan = X.roll_plan(B, L.Ho, L.Wo, C, stride)
        assert (plan['k'] > 1) == multi_unit, plan
        assert (plan['nseg'] > 1 and plan['rows_used'] % plan['nseg'] != 0) == seg_carry, plan
        chain = X.roll_stats_chain(plan, 8)
    else:
        chain = X.dw_stats_chain(B, L.Ho, L.Wo, C, path == 'strip', dil)
    check_stats_any(sl, torch.cat([out, out * out], 1), chain, dtype, ('fwd stats', path))


# (C, B, H, W, stride, variant): dw_fwd_roll_kernel.  Wout at PXL - 1, PXL, PXL + 1 (PXL = 32 at >= 64 channels, 256 at 8); stride 2
# with Win 61 .. 66 (both parities either side of the strip edge); Hout 9 = 5 + 4, 13 = 4 + 4 + 4 + 1, < 4: one short segment (fewer
# rows than the prefetch depth); 48 / 200 channels: a partial last wave / a last slice of one vector, 72: a second slice of one vector
ROLL_FWD = [
    (64, 1, 9, 31, 1, 'bnrelu'), (64, 2, 9, 32, 1, 'bn'), (64, 1, 13, 33, 1, 'mat'),
    (64, 1, 17, 61, 2, 'bnrelu'), (64, 1, 18, 62, 2, 'bn'), (64, 1, 17, 63, 2, 'mat'), (64, 2, 18, 64, 2, 'bnrelu'),
    (64, 1, 5, 65, 2, 'bnrelu'), (64, 1, 6, 66, 2, 'bn'),
    (64, 2, 3, 40, 1, 'bnrelu'), (48, 1, 1, 5, 1, 'bn'), (48, 2, 2, 35, 2, 'bnrelu'), (48, 2, 7, 35, 1, 'mat'),
    (8, 1, 5, 255, 1, 'bnrelu'), (8, 2, 3, 256, 1, 'mat'), (8, 1, 6, 257, 1, 'bn'), (8, 1, 4, 513, 2, 'bnrelu'),
    (72, 1, 9, 33, 1, 'bnrelu'), (72, 1, 9, 65, 2, 'bn'), (200, 1, 9, 33, 2, 'bnrelu'), (200, 2, 5, 31, 1, 'mat'),
    (768, 1, 6, 33, 1, 'bnrelu'),
]


@pytest.mark.parametrize('C,B,H,W,stride,variant', ROLL_FWD)
def test_row_pipelined_forward_within_the_exact_bound(C, B, H, W, stride, variant):
    run_fwd(C, B, H, W, stride, 1, variant, BF)


@pytest.mark.parametrize('B,H,W,stride,seg_carry', [(4, 5, 352, 1, False), (23, 18, 66, 2, True), (23, 9, 33, 1, True)])
def test_row_pipelined_forward_with_several_units_per_block(B, H, W, stride, seg_carry):
    """768 channels = 12 slices: 512 / 12 = 42 blocks per slice.  4 images x 11 strips = 44 units: 22 blocks of two units, the cursor
    steps by whole images only (dseg 0, dstrip 0, db 2) and the requests past the end of the stream run.  23 images x 2 strips x 2
    segments = 92 units: 31 blocks of three units, dseg = 31 % 2 = 1, dstrip = 1, db = 7, so advance() takes the segment -> strip and the
    strip -> image carry and o0 / x0 change from unit to unit"""
    run_fwd(768, B, H, W, stride, 1, 'bnrelu', BF, multi_unit=True, seg_carry=seg_carry)


# (C, B, H, W, stride, dil, variant, dtype): the strip kernels (TSS_DW_ROLL=0 for bf16 at dilation 1; (1, 4) always takes them) and the
# generic per-pixel kernel.  Strips of 4: W (stride 2: Wout) at 3, 4, 5, 7; H = 1, 2; dilation 4 on a 3 x 3 map: every off-centre tap
# out of range; generic: P no multiple of NPL, stride 2 with dilation 2 (oy * stride == ny rejects taps backward)
STRIP_GENERIC = [
    (64, 1, 1, 3, 1, 1, 'bnrelu', BF), (64, 2, 2, 4, 1, 1, 'bn', BF), (48, 1, 5, 5, 1, 1, 'mat', BF), (200, 2, 3, 7, 1, 1, 'bnrelu', BF),
    (64, 1, 1, 5, 2, 1, 'bnrelu', BF), (72, 2, 2, 7, 2, 1, 'mat', BF), (64, 1, 5, 9, 2, 1, 'bn', BF), (8, 2, 6, 13, 2, 1, 'bnrelu', BF),
    (48, 1, 4, 8, 2, 1, 'bnrelu', BF),
    (64, 2, 3, 3, 1, 4, 'bnrelu', BF), (72, 1, 9, 17, 1, 4, 'bn', BF), (8, 1, 6, 21, 1, 4, 'mat', BF), (200, 1, 5, 12, 1, 4, 'bnrelu', BF),
    (768, 1, 7, 9, 1, 1, 'bnrelu', BF), (768, 2, 3, 5, 1, 4, 'bn', BF),
    (64, 1, 2, 5, 1, 1, 'bnrelu', F32), (48, 2, 5, 7, 2, 1, 'bn', F32), (72, 1, 6, 9, 1, 4, 'mat', F32), (8, 1, 9, 40, 1, 1, 'bnrelu', F32),
    (64, 1, 5, 7, 1, 2, 'bnrelu', BF), (48, 2, 6, 9, 2, 2, 'bn', BF), (200, 1, 7, 5, 1, 3, 'mat', BF), (8, 1, 9, 31, 2, 2, 'bnrelu', BF),
    (768, 1, 3, 5, 1, 2, 'bnrelu', BF),
    (64, 1, 5, 7, 1, 2, 'bn', F32), (72, 2, 6, 9, 2, 2, 'bnrelu', F32), (8, 1, 9, 31, 1, 3, 'mat', F32),
]


@pytest.mark.parametrize('C,B,H,W,stride,dil,variant,dtype', STRIP_GENERIC)
def test_strip_and_generic_forward_within_the_exact_bound(C, B, H, W, stride, dil, variant, dtype):
    run_fwd(C, B, H, W, stride, dil, variant, dtype, roll=False)


# ----------------------------------------------------------------------------------------------------- backward: separate kernels
def run_bwd(C, B, H, W, stride, dil, variant, dtype, mode, masked, carry, seed=0):
    """tss_dwconv3x3_bwd_weight (defer_reduce = carry) then tss_dwconv3x3_bwd_data (with wg_ws / wg_dw when carry): dW, e_in and the
    slab rows of the same calls"""
    N = N_()
    L = DwLayer(seed + 11 + C + 3 * W + H + dil + mode, B, C, H, W, stride, variant)
    D = Dev(L, dtype)
    strip = X.dw_strip_pair(stride, dil)
    gop = L.gop(mode)
    _, (rin, Sin), (rw, Sw) = X.dw_refs(L.a(), L.w, gop, L.x.shape, stride, dil)
    mk = L.mask() if masked else torch.ones_like(L.x)
    rin, Sin = to_rows(rin * mk), to_rows(Sin * mk)
    NPL, rows, _, waves = X.dw_sweep(B, L.Ho, L.Wo, C, strip, dil)
    ws, dw = new_ws(C), torch.zeros(C, 9, device=DEV)
    N.call('tss_dwconv3x3_bwd_weight', *D.gargs(mode), *D.xargs, N.ptr(dw), N.ptr(ws), int(carry), B, H, W, C, stride, dil, D.code, D.st)
    ob = D.out(D.P)
    sl = nan_slabs(C) if masked else None
    margs = D.xargs if masked else (None, 0, None, None, None, 0)
    N.call('tss_dwconv3x3_bwd_data', *D.gargs(mode), N.ptr(D.w), *margs, ob.ptr, ob.ld, N.ptr(sl), N.ptr(ws) if carry else None,
           N.ptr(dw) if carry else None, B, H, W, C, stride, dil, D.code, D.st)
    torch.cuda.synchronize()
    what = (strip, mode, masked, carry)
    check_rows(ws, rows, what)
    # carry on a strip pair: the lead blocks of the backward-data grid add the rows (the sweeping kernel's waves per block); otherwise
    # dw_reduce_kernel's 16 waves
    check_dw(dw, rw, Sw, X.dw_wgrad_chain(B, L.Ho, L.Wo, C, strip, dil, lead_waves=waves if (carry and strip) else None), what)
    out = check_any(ob, rin, Sin, ('bwd data',) + what)
    if masked:
        check_stats_any(sl, torch.cat([out, out * L.xc()], 1), X.dw_stats_chain(B, H, W, C, strip, dil), dtype, ('bstats',) + what)


# (C, B, H, W, stride, dil, variant, dtype, mode, masked, carry)
BWD = [
    (64, 1, 1, 3, 1, 1, 'bnrelu', BF, 2, True, False), (64, 2, 2, 4, 1, 1, 'bn', BF, 1, True, True), (48, 1, 5, 5, 1, 1, 'mat', BF, 0, False, False),
    (200, 2, 3, 7, 1, 1, 'bnrelu', BF, 2, True, True), (64, 1, 1, 5, 2, 1, 'bnrelu', BF, 0, True, True), (72, 2, 2, 7, 2, 1, 'mat', BF, 2, True, False),
    (64, 1, 5, 9, 2, 1, 'bn', BF, 1, False, True), (8, 2, 6, 13, 2, 1, 'bnrelu', BF, 2, True, False), (48, 1, 4, 8, 2, 1, 'bnrelu', BF, 2, True, True),
    (64, 2, 3, 3, 1, 4, 'bnrelu', BF, 2, True, True), (72, 1, 9, 17, 1, 4, 'bn', BF, 0, True, False), (8, 1, 6, 21, 1, 4, 'mat', BF, 1, False, True),
    (200, 1, 5, 12, 1, 4, 'bnrelu', BF, 2, True, False), (768, 1, 7, 9, 1, 1, 'bnrelu', BF, 2, True, True), (768, 2, 3, 5, 1, 4, 'bn', BF, 1, True, False),
    (8, 2, 40, 70, 1, 1, 'bnrelu', BF, 2, True, True),
    (64, 1, 2, 5, 1, 1, 'bnrelu', F32, 2, True, True), (48, 2, 5, 7, 2, 1, 'bn', F32, 1, True, False), (72, 1, 6, 9, 1, 4, 'mat', F32, 0, False, True),
    (8, 1, 9, 40, 1, 1, 'bnrelu', F32, 2, True, False),
    (64, 1, 5, 7, 1, 2, 'bnrelu', BF, 2, True, True), (48, 2, 6, 9, 2, 2, 'bn', BF, 1, True, False), (200, 1, 7, 5, 1, 3, 'mat', BF, 0, False, True),
    (8, 1, 9, 31, 2, 2, 'bnrelu', BF, 2, True, False), (768, 1, 3, 5, 1, 2, 'bnrelu', BF, 1, True, True),
    (64, 1, 5, 7, 1, 2, 'bn', F32, 2, True, False), (72, 2, 6, 9, 2, 2, 'bnrelu', F32, 2, True, True), (8, 1, 9, 31, 1, 3, 'mat', F32, 1, False, False),
]


@pytest.mark.parametrize('C,B,H,W,stride,dil,variant,dtype,mode,masked,carry', BWD)
def test_backward_data_and_weight_kernels_within_the_exact_bound(C, B, H, W, stride, dil, variant, dtype, mode, masked, carry):
    run_bwd(C, B, H, W, stride, dil, variant, dtype, mode, masked, carry)


# ----------------------------------------------------------------------------------------------------- backward: one sweep
def run_fused(C, B, H, W, stride, dil, variant, mode, kernel, sweep, seed=0, multi_unit=False, seg_carry=False):
    """kernel: 'roll2' (default), 'roll1' (TSS_ROLL_RPJ=1), 'strip' (TSS_DW_ROLL_BWD=0: the 8-channel fused strip variant).
    sweep: tss_dwconv3x3_bwd_fused_sweep + tss_dw_reduce_many instead of tss_dwconv3x3_bwd_fused"""
    N = N_()
    L = DwLayer(seed + 23 + C + 3 * W + H + mode, B, C, H, W, stride, variant)
    D = Dev(L, BF)
    pending = variant != 'mat'
    gop = L.gop(mode)
    _, (rin, Sin), (rw, Sw) = X.dw_refs(L.a(), L.w, gop, L.x.shape, stride, dil)
    mk = L.mask() if pending else torch.ones_like(L.x)
    rin, Sin = to_rows(rin * mk), to_rows(Sin * mk)
    ws, dw = new_ws(C), torch.zeros(C, 9, device=DEV)
    ob = D.out(D.P)
    sl = nan_slabs(C) if pending else None
    rows_out = ctypes.c_int(-1)
    with env(TSS_DW_ROLL_BWD=0 if kernel == 'strip' else 1, TSS_ROLL_RPJ=1 if kernel == 'roll1' else 2):
        assert N.lib().tss_dwconv3x3_bwd_fused_supported(C, stride, dil, N.TSS_BF16) == 1
        assert N.lib().tss_dwconv3x3_bwd_fused_preferred(C, stride, dil, N.TSS_BF16) == (0 if kernel == 'strip' else 1)
        args = (*D.gargs(mode), N.ptr(D.w), *D.xargs, int(pending), ob.ptr, ob.ld, N.ptr(sl), N.ptr(ws))
        if sweep:
            N.call('tss_dwconv3x3_bwd_fused_sweep', *args, B, H, W, C, stride, dil, D.code, D.st, ctypes.byref(rows_out))
        else:
            N.call('tss_dwconv3x3_bwd_fused', *args, N.ptr(dw), B, H, W, C, stride, dil, D.code, D.st)
        torch.cuda.synchronize()
    if kernel == 'strip':
        rows = X.dw_sweep(B, H, W, C, True, dil)[1]
        wchain = X.dw_wgrad_chain(B, H, W, C, True, dil)
        schain = X.dw_stats_chain(B, H, W, C, True, dil)
    else:
        plan = X.roll_plan(B, L.Ho, L.Wo, C, stride, lanes_per_slice=16, rpj=2 if (kernel == 'roll2' and stride == 1) else 1)
        assert (plan['k'] > 1) == multi_unit, plan
        assert (plan['nseg'] > 1 and plan['rows_used'] % plan['nseg'] != 0) == seg_carry, plan
        rows = plan['rows_used']
        wchain = X.roll_wgrad_chain(plan)
        schain = X.roll_stats_chain(plan, 4, per_row=4 if stride == 2 else 1)
    what = (kernel, sweep, mode, variant)
    if sweep:
        assert rows_out.value == rows, (rows_out.value, rows)
        reduce_many([(ws, dw, C * 9, rows)])
        torch.cuda.synchronize()
    check_rows(ws, rows, what)
    check_dw(dw, rw, Sw, wchain, what)
    out = check_out(ob, rin, Sin, 9, ('fused e_in',) + what)
    if pending:
        check_stats(sl, torch.cat([out, out * L.xc()], 1), schain, ('fused bstats',) + what)


# (C, B, H, W, stride, variant, mode, sweep): PXL = 16 at >= 64 channels: Wo at 15 / 16 / 17; stride 2: the four parities of (Hin, Win);
# Ho = 5, 9: segments of 5 and 5 + 4 rows -- odd under two rows per step; 8 channels: PXL = 128; 48: PXL = 21 (252 lanes); 200: a last
# slice of two lanes; 72: a second slice of two lanes
FUSED_S1 = [
    (64, 1, 9, 15, 1, 'bnrelu', 2, False), (64, 2, 5, 16, 1, 'bn', 1, True), (64, 1, 13, 17, 1, 'mat', 0, False), (64, 2, 3, 33, 1, 'bnrelu', 2, True),
    (8, 1, 5, 129, 1, 'bnrelu', 2, False), (48, 2, 7, 22, 1, 'bn', 2, True), (200, 1, 9, 17, 1, 'bnrelu', 1, False), (72, 1, 1, 5, 1, 'mat', 2, True),
    (768, 1, 6, 17, 1, 'bnrelu', 2, False),
]
FUSED_S2 = [
    (64, 1, 9, 31, 2, 'bnrelu', 2, False), (64, 2, 10, 32, 2, 'bn', 1, True), (64, 1, 9, 32, 2, 'mat', 0, False), (64, 1, 10, 33, 2, 'bnrelu', 2, True),
    (8, 1, 18, 257, 2, 'bnrelu', 2, False), (48, 2, 7, 43, 2, 'bn', 2, True), (200, 1, 17, 33, 2, 'bnrelu', 1, False), (72, 1, 1, 5, 2, 'mat', 2, True),
    (64, 2, 2, 2, 2, 'bnrelu', 2, False), (768, 1, 6, 34, 2, 'bnrelu', 2, True),
]


@pytest.mark.parametrize('C,B,H,W,stride,variant,mode,sweep', FUSED_S1 + FUSED_S2)
def test_row_pipelined_backward_within_the_exact_bound(C, B, H, W, stride, variant, mode, sweep):
    run_fused(C, B, H, W, stride, 1, variant, mode, 'roll2', sweep)


@pytest.mark.parametrize('C,B,H,W,stride,variant,mode,sweep', FUSED_S1)
def test_row_pipelined_backward_one_row_per_step_within_the_exact_bound(C, B, H, W, stride, variant, mode, sweep):
    run_fused(C, B, H, W, stride, 1, variant, mode, 'roll1', sweep)


@pytest.mark.parametrize('B,H,W,stride,kernel,seg_carry', [(4, 5, 352, 1, 'roll2', False), (9, 11, 33, 1, 'roll2', True),
                                                         (23, 18, 34, 2, 'roll2', True), (23, 9, 17, 1, 'roll1', True)])
def test_row_pipelined_backward_with_several_units_per_block(B, H, W, stride, kernel, seg_carry):
    """768 channels: 42 blocks per slice.  4 images x 22 strips of 16 = 88 units in one segment: 30 blocks of three, dseg 0.  9 images x 3
    strips x 3 segments = 81 units: 41 blocks of two, dseg = 41 % 3 = 2, dstrip 1, db 4.  23 images x 2 strips x 2 segments = 92 units:
    31 blocks of three, dseg 1, dstrip 1, db 7.  The last three take both carries of advance() in each backward kernel"""
    run_fused(768, B, H, W, stride, 1, 'bnrelu', 2, kernel, True, multi_unit=True, seg_carry=seg_carry)


# the 8-channel fused strip variant at its three (stride, dilation) pairs: (C, B, H, W, stride, dil, variant, mode, sweep)
FUSED_STRIP = [
    (64, 1, 1, 3, 1, 1, 'bnrelu', 2, False), (48, 2, 2, 4, 1, 1, 'mat', 1, True), (200, 1, 5, 7, 1, 1, 'bn', 2, False),
    (64, 1, 1, 5, 2, 1, 'bnrelu', 2, True), (72, 2, 5, 9, 2, 1, 'mat', 0, False), (8, 2, 6, 13, 2, 1, 'bnrelu', 2, True), (48, 1, 4, 8, 2, 1, 'bn', 1, False),
    (64, 2, 3, 3, 1, 4, 'bnrelu', 2, False), (72, 1, 9, 17, 1, 4, 'bn', 1, True), (8, 1, 6, 21, 1, 4, 'mat', 2, False), (768, 1, 5, 9, 1, 4, 'bnrelu', 2, True),
    (8, 2, 40, 70, 1, 1, 'bnrelu', 2, True),
]


@pytest.mark.parametrize('C,B,H,W,stride,dil,variant,mode,sweep', FUSED_STRIP)
def test_fused_strip_backward_within_the_exact_bound(C, B, H, W, stride, dil, variant, mode, sweep):
    run_fused(C, B, H, W, stride, dil, variant, mode, 'strip', sweep)


# ----------------------------------------------------------------------------------------------------- row reduction
def test_row_reduction_of_many_jobs_is_bit_exact_on_integer_rows():
    """tss_dw_reduce_many alone: workspace rows of small integers (every f32 sum exact, so the result is compared bit for bit), added
    onto a non-zero dw; the 16-byte path (n % 4 == 0, aligned pointers) and the scalar path (n % 4 != 0; a misaligned ws; a misaligned
    dw); rows = 1; 16 x 32 + 1 rows (a second trip of the row loop); 85 jobs > 2 x RED_MANY = 80, so the host loop chunks three times"""
    g = torch.Generator().manual_seed(3)
    shapes = [(72, 5), (70, 7), (576, 1), (1, 1), (257, 33), (6912, 24), (64, 513), (260, 17)]
    jobs, keep, expect = [], [], []
    for j in range(85):
        n, rows = shapes[j % len(shapes)]
        mis_ws, mis_dw = j % 5 == 1, j % 7 == 2            # a pointer 4 bytes off a 16-byte boundary
        wsf = torch.full((rows * n + 8,), float('nan'), device=DEV)
        dwf = torch.full((n + 8,), float('nan'), device=DEV)
        o_ws, o_dw = (1 if mis_ws else 4), (1 if mis_dw else 4)
        rws = torch.randint(-64, 65, (rows, n), generator=g).float()
        d0 = torch.randint(-1000, 1001, (n,), generator=g).float()
        wsf[o_ws:o_ws + rows * n] = rws.flatten().to(DEV)
        dwf[o_dw:o_dw + n] = d0.to(DEV)
        keep.append((wsf, dwf))
        jobs.append((wsf.data_ptr() + 4 * o_ws, dwf.data_ptr() + 4 * o_dw, n, rows))
        expect.append((o_dw, n, (d0.double() + rws.double().sum(0)).float()))
    reduce_many(jobs)
    torch.cuda.synchronize()
    for j, ((wsf, dwf), (o_dw, n, exp)) in enumerate(zip(keep, expect)):
        got = dwf.cpu()
        assert torch.equal(X.bits(got[o_dw:o_dw + n]), X.bits(exp)), ('job', j, jobs[j][2:])
        assert torch.isnan(got[:o_dw]).all() and torch.isnan(got[o_dw + n:]).all(), ('job', j, 'wrote outside dw')


# ----------------------------------------------------------------------------------------------------- upsample + depthwise
def run_updw(C, B, Hs, Ws, Ho, Wo, D, mode, seed=0, segments=False):
    N = N_()
    BFc, st = N.TSS_BF16, N.stream()
    g = torch.Generator().manual_seed(seed + C + Hs * 7 + Wo)
    x = X.dyadic((B, C, Hs, Ws), g, zero_frac=0.04)
    L = DwLayer(seed + 5 + C + Wo, B, C, Ho, Wo, 1, 'mat')             # e, y, the backward coefficients and the weights at (Ho, Wo)
    dyadic = X.dyadic_resize(Hs, Ho) and X.dyadic_resize(Ws, Wo)
    xup, v = X.upsampled_operand(x, Ho, Wo)
    if dyadic:
        X.exact_f32(v)
        op, dop = xup, torch.zeros_like(v)
    else:
        # the kernel's operand is rne_bf16 of an f32 blend within `slack` of v (half an ulp of 8 significant bits is <= 2^-8 of the
        # value): |operand - v| <= 2^-8 (|v| + slack) + slack
        slack = X.bilinear_f32_slack(x, Ho, Wo)
        op, dop = v, 2.0 ** -8 * (v.abs() + slack) + slack
    assert N.lib().tss_updw_supported(B, Hs, Ws, Ho, Wo, C, D, BFc) == 1
    fgeo, bgeo = X.updw_fwd_geometry(B, Hs, Ws, Ho, Wo, C, D), X.updw_bwd_geometry(B, Hs, Ws, Ho, Wo, C, D)
    assert N.lib().tss_updw_ws_rows(B, Hs, Ws, Ho, Wo, C, D, BFc) == bgeo['nunits']
    assert not segments or (fgeo['nseg'] > 1 and bgeo['nseg'] > 1), (fgeo, bgeo)      # several row segments per residue class
    kw = dict(padding=D, dilation=D, groups=C)
    F, G = torch.nn.functional, torch.nn.grad
    P, Ps = B * Ho * Wo, B * Hs * Ws
    w_d = dev(L.w.reshape(C, 9))
    xb = Buf(Ps, C, C + 8, 0, to_rows(x))
    # ---- forward
    ref = F.conv2d(op, L.w, **kw)
    S = F.conv2d(op.abs() + dop, L.w.abs(), **kw)
    slackS = F.conv2d(dop, L.w.abs(), **kw)
    yb, sl = Buf(P, C, C + 16, 8), nan_slabs(C)
    N.call('tss_updw_fwd', xb.ptr, xb.ld, Hs, Ws, N.ptr(w_d), yb.ptr, yb.ld, N.ptr(sl), B, Ho, Wo, C, D, BFc, st)
    torch.cuda.synchronize()
    out = yb.rows()
    bound = 2.0 ** -8 * to_rows(ref).abs() + 2.0 ** -22 * 9 * to_rows(S) + (1 + 2.0 ** -8) * to_rows(slackS)
    ex = ((out - to_rows(ref)).abs() - bound).max().item()
    assert ex <= 0, ('updw fwd excess', ex)
    assert yb.untouched()
    check_stats(sl, torch.cat([out, out * out], 1), X.updw_stats_chain(fgeo), 'updw stats')
    # ---- backward: e_up = gradient with respect to the upsampled map (no operand of it is interpolated), dW from the interpolated map
    gop = L.gop(mode)
    rin, Sin = X.conv_input_ref((B, C, Ho, Wo), L.w, gop, **kw)
    rw = G.conv2d_weight(op, L.w.shape, gop, **kw)
    Sw = G.conv2d_weight(op.abs() + dop, L.w.shape, gop.abs(), **kw)
    slackW = G.conv2d_weight(dop, L.w.shape, gop.abs(), **kw)
    Dv = Dev(L, BF)
    ga = Dv.gargs(mode)
    ws = new_ws(C, bgeo['nunits'] + 3)
    dw = torch.zeros(C, 9, device=DEV)
    ub = Buf(P, C, C + 16, 8)
    rows_out = ctypes.c_int(-1)
    N.call('tss_updw_bwd', *ga, N.ptr(w_d), xb.ptr, xb.ld, Hs, Ws, ub.ptr, ub.ld, N.ptr(ws), B, Ho, Wo, C, D, BFc, st, ctypes.byref(rows_out))
    torch.cuda.synchronize()
    assert rows_out.value == bgeo['nunits']
    check_rows(ws, bgeo['nunits'], 'updw ws')
    reduce_many([(ws, dw, C * 9, bgeo['nunits'])])
    torch.cuda.synchronize()
    check_out(ub, to_rows(rin), to_rows(Sin), 9, 'updw e_up')
    exw = ((dw.double().cpu().reshape(rw.shape) - rw).abs() - 2.0 ** -23 * X.updw_wgrad_chain(bgeo) * Sw - slackW).max().item()
    assert exw <= 0, ('updw dW excess', exw)


# (C, B, Hs, Ws, Ho, Wo, D, mode).  Dyadic pairs (the hard bound): x4 at D = 4 with three forward / five backward column strips, and
# 42 -> 165 rows: three row segments per residue class forward, two backward; sources of 1 x 1 and 1 x n; D = 2 and D = 8; 48 / 72 / 200 channels.  Non-dyadic pairs, one
# per direction and both: the bound carries X.bilinear_f32_slack
UPDW = [
    (64, 2, 5, 19, 17, 73, 4, 2), (72, 1, 42, 19, 165, 73, 4, 1), (48, 2, 1, 1, 9, 21, 4, 2), (64, 1, 1, 6, 7, 41, 4, 0),
    (200, 1, 3, 9, 9, 33, 2, 2), (64, 1, 4, 3, 25, 17, 8, 1), (8, 2, 5, 5, 17, 17, 1, 2),
    (64, 1, 5, 9, 18, 33, 4, 2), (48, 1, 5, 9, 17, 30, 4, 1), (72, 2, 6, 7, 22, 50, 4, 2),
]


@pytest.mark.parametrize('C,B,Hs,Ws,Ho,Wo,D,mode', UPDW)
def test_upsample_depthwise_operator_within_the_exact_bound(C, B, Hs, Ws, Ho, Wo, D, mode):
    run_updw(C, B, Hs, Ws, Ho, Wo, D, mode, segments=Hs == 42)
