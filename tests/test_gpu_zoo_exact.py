"""Each C entry point of the LEDNet / ESNet kernels (csrc/fc1d.hip, fcg.hip, sconv.hip, ssnbt.hip, zoo.hip), called once, against f64 on
dyadic operands (tests/exact.py): the kernel's only freedom is its f32 accumulation order and the final bf16 rounding, so every output
element is held to a worst-case bound -- one wrong contraction term in one element fails.  Every case runs twice: on the lean kernels
and with tss_set_option(TSS_OPT_DISABLE_FAST_PATHS, 1) on the generic ones, under the same bound.  Output buffers are filled with a
sentinel (pitch padding, a concat offset, spare rows) that must survive bit for bit; statistics slabs start as NaN."""
import pytest
import torch

from tests import exact as X
from tests.exact_gpu import DEV, Buf, Layer, N_, check_out, check_stats, dev, nan_slabs, to_rows, vecs as _vecs

pytestmark = pytest.mark.gpu


def in_modes(fn):
    """fn(generic) on the lean kernels (generic False) and on the generic ones (tss_set_option(1, 1))"""
    N = N_()
    fn(False)
    N.call('tss_set_option', 1, 1)
    try:
        fn(True)
    finally:
        N.call('tss_set_option', 1, 0)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------- fc1d / fcg tap layers
def run_tap_layer(C, T, B, H, W, axis, dil, relu, affine, cbias, seed=0, wgrad=False, cap=None):
    N = N_()
    BF, st = N.TSS_BF16, N.stream()
    ks, pad, dl = X.tap_geom(T, axis, dil)
    L = Layer(seed, B, C, H, W, C, ks, H, W, affine=affine, relu=relu, cbias=cbias)
    P, K = B * H * W, T * C
    v = _vecs(L)
    w_t = dev(L.w.reshape(C, C, T))
    w_tnc, w_tcn = torch.empty(T, C, C, device=DEV), torch.empty(T, C, C, device=DEV)
    N.call('tss_permute_wtaps', N.ptr(w_t), N.ptr(w_tnc), N.ptr(w_tcn), C, C, T, st)
    xb = Buf(P, C, C + 8, 0, to_rows(L.x))
    xargs = (xb.ptr, xb.ld, N.ptr(v['mean']), N.ptr(v['scale']), N.ptr(v['bias']), int(relu))
    a = L.a()
    ref, S = X.conv_ref(a, L.w, padding=pad, dilation=dl)
    if cbias:
        ref, S = ref + L.cb.view(1, -1, 1, 1), S + L.cb.abs().view(1, -1, 1, 1)
    ref, S = to_rows(ref), to_rows(S)

    def chain(generic, mode):
        """f32 statistics chain of the launch: the generic kernel's, or the lean instance's (MT, rows per block) of this MODE"""
        if generic:
            return X.generic_stats_chain(P, C)
        if T == 3 and C <= 64:               # fc1d: four rows per block; MT 4 / 4 / 1 at 16 / 32 / 64 channels, 2 for MODE 2 at 32
            return X.lean_stats_chain(B * H, W, {16: 4, 32: 2 if mode == 2 else 4, 64: 1}[C], 4)
        if C == 64:                          # fcg 64 x 5: four waves, MT 4 (2 in MODE 2)
            return X.lean_stats_chain(B * H, W, 2 if mode == 2 else 4, 4)
        # fcg 128 x 3: eight waves, MT 2 forward / 1 backward; MODE 2 splits the channels over wave pairs (four rows per block)
        return X.lean_stats_chain(B * H, W, 2 if mode == 0 else 1, 4 if mode == 2 else 8)
    xc = to_rows(L.x - (L.mean if affine else 0))
    lean_w = T == 3 and C in (16, 32, 64)

    if T == 3 and C in (16, 32, 64):
        assert N.lib().tss_conv1d3_lean_supported(C, C, BF) == 1
    # ---- forward, through the permuted-weight entry (both modes) and the layer's own weights (lean only, 8-byte aligned concat store)
    def fwd(generic):
        yb, sl = Buf(P, C, C + 8, 8), nan_slabs(C)
        if T == 3:
            N.call('tss_conv1d3_fwd', *xargs, N.ptr(w_tnc), N.ptr(v['cb']), yb.ptr, yb.ld, N.ptr(sl), B, H, W, C, C, axis, dil, BF, st)
        else:
            N.call('tss_convkxk_fwd', *xargs, N.ptr(w_tnc), N.ptr(v['cb']), yb.ptr, yb.ld, N.ptr(sl), B, H, W, C, C, ks[0], ks[1], 1, dil,
                   BF, st)
        torch.cuda.synchronize()
        out = check_out(yb, ref, S, K, ('fwd', generic))
        check_stats(sl, torch.cat([out, out * out], 1), chain(generic, 0), ('fwd stats', generic))
        if lean_w and not generic:
            yb, sl = Buf(P, C, C + 4, 4), nan_slabs(C)
            N.call('tss_conv1d3_fwd_w', *xargs, N.ptr(w_t), N.ptr(v['cb']), yb.ptr, yb.ld, N.ptr(sl), B, H, W, C, C, axis, dil, BF, st)
            torch.cuda.synchronize()
            out = check_out(yb, ref, S, K, ('fwd_w', generic))
            check_stats(sl, torch.cat([out, out * out], 1), chain(generic, 0), ('fwd_w stats', generic))
    in_modes(fwd)

    # ---- backward-data: MODE 1 (g = ga e) and MODE 2 (BatchNorm-backward combination), with and without the input's mask + bstats
    eb = Buf(P, C, C + 16, 0, to_rows(L.e))
    yrb = Buf(P, C, C + 16, 0, to_rows(L.y))
    for mode in (1, 2):
        for masked in (False, True):
            gop = L.gop(mode)
            rin, Sin = X.conv_input_ref((B, C, H, W), L.w, gop, padding=pad, dilation=dl)
            mk = L.mask() if masked else torch.ones_like(L.x)
            rin, Sin = to_rows(rin * mk), to_rows(Sin * mk)
            gargs = ((eb.ptr, eb.ld, yrb.ptr, yrb.ld, N.ptr(v['ga']), N.ptr(v['gb']), N.ptr(v['gce']), N.ptr(v['gmu'])) if mode == 2
                     else (eb.ptr, eb.ld, None, 0, N.ptr(v['ga']), None, None, None))
            margs = xargs if masked else (None, 0, None, None, None, 0)

            def bwd(generic):
                ob = Buf(P, C, C + 8, 8)
                sl = nan_slabs(C) if masked else None
                if T == 3:
                    N.call('tss_conv1d3_bwd_data', *gargs, N.ptr(w_tcn), *margs, ob.ptr, ob.ld, N.ptr(sl), B, H, W, C, C, axis, dil, BF, st)
                else:
                    N.call('tss_convkxk_bwd_data', *gargs, N.ptr(w_tcn), *margs, ob.ptr, ob.ld, N.ptr(sl), B, H, W, C, C, ks[0], ks[1], 1,
                           dil, BF, st)
                torch.cuda.synchronize()
                out = check_out(ob, rin, Sin, K, ('bwd', mode, masked, generic))
                if masked:
                    check_stats(sl, torch.cat([out, out * xc], 1), chain(generic, mode), ('bstats', mode, generic))
                if lean_w and not generic:
                    ob = Buf(P, C, C + 4, 4)
                    sl = nan_slabs(C) if masked else None
                    N.call('tss_conv1d3_bwd_data_w', *gargs, N.ptr(w_t), *margs, ob.ptr, ob.ld, N.ptr(sl), B, H, W, C, C, axis, dil, BF, st)
                    torch.cuda.synchronize()
                    out = check_out(ob, rin, Sin, K, ('bwd_w', mode, masked))
                    if masked:
                        check_stats(sl, torch.cat([out, out * xc], 1), chain(generic, mode), ('bstats_w', mode))
            in_modes(bwd)

    if wgrad:
        run_tap_wgrad(L, v, xb, eb, yrb, T, axis, dil, pad, dl, cap)
    return L


def run_tap_wgrad(L, v, xb, eb, yrb, T, axis, dil, pad, dl, cap):
    N = N_()
    BF, st = N.TSS_BF16, N.stream()
    B, C, H, W = L.B, L.Cin, L.H, L.W
    P = B * H * W
    a = L.a()
    xargs = (xb.ptr, xb.ld, N.ptr(v['mean']), N.ptr(v['scale']), N.ptr(v['bias']), int(L.relu))
    fc1d = T == 3 and C <= 64
    for with_y in (False, True):
        gop = L.gop(2 if with_y else 1)
        ref, S = X.conv_weight_ref(a, L.w.shape, gop, padding=pad, dilation=dl)
        ref, S = ref.reshape(C, C, T), S.reshape(C, C, T)
        gargs = ((eb.ptr, eb.ld, yrb.ptr, yrb.ld, N.ptr(v['ga']), N.ptr(v['gb']), N.ptr(v['gce']), N.ptr(v['gmu'])) if with_y
                 else (eb.ptr, eb.ld, None, 0, N.ptr(v['ga']), None, None, None))

        def wg(generic):
            dw = torch.zeros(C, C, T, device=DEV)
            if generic:
                assert (N.lib().tss_conv1d3_bwd_weight_rows(P, C, C, BF) if fc1d else N.lib().tss_convtap_bwd_weight_rows(P, C, C, T, BF)) == 0
                ks = (1, T) if axis == 0 else (T, 1)
                if T == 3:
                    N.call('tss_conv1d3_bwd_weight', *gargs, *xargs, N.ptr(dw), B, H, W, C, C, axis, dil, BF, st)
                else:
                    N.call('tss_convkxk_bwd_weight', *gargs, *xargs, N.ptr(dw), B, H, W, C, C, ks[0], ks[1], 1, dil, BF, st)
                chain = X.generic_wgrad_chain(P, C, C, T)
            else:
                rows = N.lib().tss_conv1d3_bwd_weight_rows(P, C, C, BF) if fc1d else N.lib().tss_convtap_bwd_weight_rows(P, C, C, T, BF)
                assert rows > 1
                if cap:
                    assert rows == cap, rows          # the persistent-grid path: rows at the sweep's grid cap
                ws = torch.full((rows, C * C * T), float('nan'), device=DEV)
                name = 'tss_conv1d3_bwd_weight_sweep' if fc1d else 'tss_convtap_bwd_weight_sweep'
                extra = (B, H, W, C, C, axis, dil) if fc1d else (B, H, W, C, C, T, axis, dil)
                N.call(name, *gargs, *xargs, N.ptr(ws), *extra, BF, st)
                from torch_semantic_segmentation_amd import ops
                ops._reduce_rows_now(ws, dw, C * C * T, rows)
                # fc1d: 64-pixel stages at 64 channels, 128 otherwise (C = 16: the four waves split a stage and meet in 4 LDS atomics);
                # fcg: 32-pixel stages
                PT = (64 if C == 64 else 128) if fc1d else 32
                chain = X.sweep_chain(P, PT, rows) + (4 if fc1d and C == 16 else 0)
            torch.cuda.synchronize()
            ex = X.wgrad_excess(dw.double().cpu(), ref, S, chain)
            assert ex <= 0, ('wgrad', with_y, generic, ex)
        in_modes(wg)


# (C, B, H, W, axis, dil, relu, affine, cbias): W at tile - 1, tile, tile + 1 of each instance's 16 MT-pixel row tile (fc1d: C16 64, C32
# 64 / 32 in MODE 2, C64 16), dilations 1 .. 17 with one >= W (axis 0) and one >= H (axis 1), B = 3 for axis 1
FC1D_CASES = [
    (16, 1, 1, 63, 0, 1, True, True, True), (16, 1, 1, 64, 0, 2, False, True, False), (16, 1, 1, 65, 0, 5, True, False, True),
    (16, 3, 7, 20, 1, 9, True, True, True),
    (32, 1, 1, 31, 0, 1, True, True, False), (32, 1, 1, 32, 0, 17, False, False, True), (32, 1, 1, 33, 0, 2, True, True, True),
    (32, 1, 1, 63, 0, 5, True, True, True), (32, 1, 1, 64, 0, 1, True, True, True), (32, 1, 1, 65, 0, 9, False, True, True), (32, 3, 5, 18, 1, 2, True, True, False),
    (64, 1, 1, 15, 0, 1, True, True, True), (64, 1, 1, 16, 0, 5, True, False, False), (64, 1, 1, 17, 0, 9, False, True, True),
    (64, 2, 3, 12, 0, 17, True, True, True), (64, 3, 9, 10, 1, 17, True, True, True), (64, 3, 6, 20, 1, 5, False, False, True),
]


@pytest.mark.parametrize('C,B,H,W,axis,dil,relu,affine,cbias', FC1D_CASES)
def test_fc1d_three_tap_layers_within_the_exact_bound(C, B, H, W, axis, dil, relu, affine, cbias):
    run_tap_layer(C, 3, B, H, W, axis, dil, relu, affine, cbias, seed=C * 100 + W + dil)


# fcg: 64 channels x 5 taps (tile 64, 32 in MODE 2) and 128 x 3 (tile 32 forward, 16 backward; MODE 2 is the split-wave NSPL = 2 form)
FCG_CASES = [
    (64, 5, 1, 1, 63, 0, 2, True, True, True), (64, 5, 1, 1, 33, 0, 5, True, False, True), (64, 5, 3, 11, 9, 1, 9, True, True, False),
    (64, 5, 2, 3, 20, 0, 17, False, True, True), (64, 5, 1, 1, 64, 0, 1, True, True, True), (64, 5, 1, 1, 65, 0, 9, True, True, True),
    (64, 5, 1, 1, 31, 0, 2, False, True, True), (64, 5, 1, 1, 32, 0, 5, True, True, False),
    (128, 3, 1, 1, 31, 0, 2, True, True, True), (128, 3, 1, 1, 17, 0, 9, True, True, False), (128, 3, 3, 7, 16, 1, 5, False, True, True),
    (128, 3, 2, 18, 5, 1, 17, True, False, True), (128, 3, 1, 1, 32, 0, 1, True, True, True), (128, 3, 1, 1, 33, 0, 5, True, True, True),
    (128, 3, 1, 1, 15, 0, 2, False, True, True),
]


@pytest.mark.parametrize('C,T,B,H,W,axis,dil,relu,affine,cbias', FCG_CASES)
def test_fcg_tap_layers_within_the_exact_bound(C, T, B, H, W, axis, dil, relu, affine, cbias):
    run_tap_layer(C, T, B, H, W, axis, dil, relu, affine, cbias, seed=C * 100 + W + dil)


# weight gradients: P of 2 - 5 k pixels with several partial rows, and one case with the rows at the grid cap (persistent sweep)
# cap: fc1d's sweep reaches its 512 rows at ceil(P / 64) >= 2048 stages (64 channels), fcg's its 256 rows at ceil(P / 32) >= 2048
WG_CASES = [(16, 3, 2, 30, 50, 0, 2, None), (32, 3, 3, 20, 50, 1, 5, None), (64, 3, 2, 25, 60, 0, 9, None), (64, 5, 2, 30, 40, 1, 2, None),
            (128, 3, 2, 24, 50, 0, 17, None), (64, 3, 4, 128, 256, 1, 1, 512), (64, 5, 2, 128, 256, 0, 2, 256), (128, 3, 2, 128, 256, 1, 5, 256)]


@pytest.mark.parametrize('C,T,B,H,W,axis,dil,cap', WG_CASES)
def test_tap_weight_gradient_sweeps_within_the_exact_bound(C, T, B, H, W, axis, dil, cap):
    run_tap_layer(C, T, B, H, W, axis, dil, True, True, True, seed=C + W, wgrad=True, cap=cap)


# ----------------------------------------------------------------------------------------------------- sconv: stride-2 3x3
def _sc_layer(seed, B, Cin, H, W, N, affine=True, relu=True, cbias=True):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return Layer(seed, B, Cin, H, W, N, (3, 3), Ho, Wo, affine=affine, relu=relu, cbias=cbias)


SC_FWD = [(64, 64), (32, 32), (16, 64), (24, 16), (16, 16), (16, 48), (64, 128)]
SC_FWD_MT = {(64, 64): 1, (32, 32): 2, (16, 64): 2, (24, 16): 4, (16, 16): 4, (16, 48): 2, (64, 128): 1}     # tss_sconv_fwd's instances
HW_PAR = [(2, 3), (3, 2), (7, 10), (6, 9)]          # Hin and Win in {2, 3, odd, even}: every parity class, the 1-tap last row / column


@pytest.mark.parametrize('Cin,Nout', SC_FWD)
@pytest.mark.parametrize('H,W', HW_PAR)
def test_sconv_forward_instances_within_the_exact_bound(Cin, Nout, H, W):
    N = N_()
    BF, st = N.TSS_BF16, N.stream()
    B = 2
    L = _sc_layer(Cin + Nout + H * W, B, Cin, H, W, Nout)
    v = _vecs(L)
    P, Po = B * H * W, B * L.Ho * L.Wo
    w9 = dev(L.w.reshape(Nout, Cin, 9))
    w_tnc, w_tcn = torch.empty(9, Nout, Cin, device=DEV), torch.empty(9, Cin, Nout, device=DEV)
    N.call('tss_permute_wtaps', N.ptr(w9), N.ptr(w_tnc), N.ptr(w_tcn), Nout, Cin, 9, st)
    xb = Buf(P, Cin, Cin + 8, 0, to_rows(L.x))
    ref, S = X.conv_ref(L.a(), L.w, stride=2, padding=1)
    ref, S = to_rows(ref + L.cb.view(1, -1, 1, 1)), to_rows(S + L.cb.abs().view(1, -1, 1, 1))

    def fwd(generic):
        yb, sl = Buf(Po, Nout, 2 * Nout + 8, 8), nan_slabs(Nout)      # the convolution's part of a concat buffer
        N.call('tss_convkxk_fwd', xb.ptr, xb.ld, N.ptr(v['mean']), N.ptr(v['scale']), N.ptr(v['bias']), 1, N.ptr(w_tnc), N.ptr(v['cb']),
               yb.ptr, yb.ld, N.ptr(sl), B, H, W, Cin, Nout, 3, 3, 2, 1, BF, st)
        torch.cuda.synchronize()
        out = check_out(yb, ref, S, 9 * Cin, ('sconv fwd', generic))
        chain = (X.generic_stats_chain(Po, Nout) if generic
                 else X.lean_stats_chain(B * L.Ho, L.Wo, SC_FWD_MT[(Cin, Nout)], 4))
        check_stats(sl, torch.cat([out, out * out], 1), chain, ('sconv stats', generic))
    in_modes(fwd)


SC_BWD = [(48, 16), (64, 64), (32, 32)]      # (N gradient channels, Cin)


@pytest.mark.parametrize('Nout,Cin', SC_BWD)
@pytest.mark.parametrize('H,W', HW_PAR)
@pytest.mark.parametrize('masked', [False, True])
def test_sconv_backward_data_instances_within_the_exact_bound(Nout, Cin, H, W, masked):
    N = N_()
    BF, st = N.TSS_BF16, N.stream()
    B = 2
    L = _sc_layer(Cin + Nout + H * W + masked, B, Cin, H, W, Nout)
    v = _vecs(L)
    P, Po = B * H * W, B * L.Ho * L.Wo
    w9 = dev(L.w.reshape(Nout, Cin, 9))
    w_tnc, w_tcn = torch.empty(9, Nout, Cin, device=DEV), torch.empty(9, Cin, Nout, device=DEV)
    N.call('tss_permute_wtaps', N.ptr(w9), N.ptr(w_tnc), N.ptr(w_tcn), Nout, Cin, 9, st)
    xb = Buf(P, Cin, Cin + 8, 0, to_rows(L.x))
    eb = Buf(Po, Nout, 2 * Nout, 0, to_rows(L.e))
    gop = L.gop(1)
    rin, Sin = X.conv_input_ref((B, Cin, H, W), L.w, gop, stride=2, padding=1)
    mk = L.mask() if masked else torch.ones_like(L.x)
    rin, Sin = to_rows(rin * mk), to_rows(Sin * mk)
    xc = to_rows(L.x - L.mean)
    margs = (xb.ptr, xb.ld, N.ptr(v['mean']), N.ptr(v['scale']), N.ptr(v['bias']), 1) if masked else (None, 0, None, None, None, 0)

    def bwd(generic):
        ob = Buf(P, Cin, Cin + 8, 8)
        sl = nan_slabs(Cin) if masked else None
        N.call('tss_convkxk_bwd_data', eb.ptr, eb.ld, None, 0, N.ptr(v['ga']), None, None, None, N.ptr(w_tcn), *margs, ob.ptr, ob.ld,
               N.ptr(sl), B, H, W, Cin, Nout, 3, 3, 2, 1, BF, st)
        torch.cuda.synchronize()
        out = check_out(ob, rin, Sin, 4 * Nout, ('sconv bwd', generic))      # <= 4 taps reach an input pixel
        if masked:
            # the parity-class kernel: tiles of 16 MT pixels of one column parity of an input row (MT 2 / 2 / 4 at 48 / 64 / 32)
            chain = (X.generic_stats_chain(P, Cin) if generic
                     else X.lean_stats_chain(B * H, (W + 1) // 2, {48: 2, 64: 2, 32: 4}[Nout], 4, parities=2))
            check_stats(sl, torch.cat([out, out * xc], 1), chain, ('sconv bstats', generic))
    in_modes(bwd)


SC_T = [(64, 16), (16, 24), (16, 16), (128, 64)]        # ConvTranspose2d(Cin_t, Cout)


@pytest.mark.parametrize('Cin_t,Cout', SC_T)
@pytest.mark.parametrize('h,w', [(1, 1), (1, 2), (4, 5), (3, 6)])
def test_sconv_transposed_instances_within_the_exact_bound(Cin_t, Cout, h, w):
    N = N_()
    BF, st = N.TSS_BF16, N.stream()
    B = 2
    g = torch.Generator().manual_seed(Cin_t + Cout + h * w)
    x = X.dyadic((B, Cin_t, h, w), g, zero_frac=0.04)
    wt = X.dyadic((Cin_t, Cout, 3, 3), g, emin=-6, emax=-2)
    bias = X.dyadic((Cout,), g)
    Ho, Wo = 2 * h, 2 * w
    w_d = dev(wt.reshape(Cin_t, Cout, 9))
    w_tnc, w_tcn = torch.empty(9, Cin_t, Cout, device=DEV), torch.empty(9, Cout, Cin_t, device=DEV)
    N.call('tss_permute_wtaps', N.ptr(w_d), N.ptr(w_tnc), N.ptr(w_tcn), Cin_t, Cout, 9, st)
    xb = Buf(B * h * w, Cin_t, Cin_t + 8, 0, to_rows(x))
    bd = dev(bias)
    ref, S = X.convT_ref(x, wt)
    ref, S = to_rows(ref + bias.view(1, -1, 1, 1)), to_rows(S + bias.abs().view(1, -1, 1, 1))

    def tf(generic):
        yb = Buf(B * Ho * Wo, Cout, Cout + 8, 8)
        N.call('tss_convkxk_transposed_fwd', xb.ptr, xb.ld, N.ptr(w_tcn), N.ptr(bd), yb.ptr, yb.ld, B, Ho, Wo, Cout, Cin_t, 3, 3, 2, BF, st)
        torch.cuda.synchronize()
        check_out(yb, ref, S, 4 * Cin_t, ('sconv transposed', generic))      # <= 4 taps reach an output pixel
    in_modes(tf)


# sweeps: (N channels on the output grid, Cin on the input grid): sw<32>, sw<64>, swr<64,16>, swr<16,24>, swr<16,16>
# cap: sw<32> and swr reach 512 rows at ceil(Po / 64) >= 4096 stages, sw<64> its 256 rows at ceil(Po / 32) >= 2048
SC_WG = [(32, 32, 2, 90, 70, None), (64, 64, 2, 60, 90, None), (64, 16, 2, 80, 90, None), (16, 24, 2, 80, 90, None), (16, 16, 2, 81, 91, None),
         (32, 32, 4, 512, 512, 512), (64, 64, 1, 512, 512, 256), (64, 16, 4, 512, 512, 512)]


@pytest.mark.parametrize('Nout,Cin,B,H,W,cap', SC_WG)
def test_sconv_weight_gradient_sweeps_within_the_exact_bound(Nout, Cin, B, H, W, cap):
    N = N_()
    BF, st = N.TSS_BF16, N.stream()
    L = _sc_layer(Nout * Cin + H, B, Cin, H, W, Nout)
    v = _vecs(L)
    P, Po = B * H * W, B * L.Ho * L.Wo
    xb = Buf(P, Cin, Cin + 8, 0, to_rows(L.x))
    eb, yrb = Buf(Po, Nout, Nout + 8, 0, to_rows(L.e)), Buf(Po, Nout, Nout + 8, 0, to_rows(L.y))
    xargs = (xb.ptr, xb.ld, N.ptr(v['mean']), N.ptr(v['scale']), N.ptr(v['bias']), 1)
    a = L.a()
    for with_y in (False, True):
        gop = L.gop(2 if with_y else 1)
        ref, S = X.conv_weight_ref(a, L.w.shape, gop, stride=2, padding=1)
        gargs = ((eb.ptr, eb.ld, yrb.ptr, yrb.ld, N.ptr(v['ga']), N.ptr(v['gb']), N.ptr(v['gce']), N.ptr(v['gmu'])) if with_y
                 else (eb.ptr, eb.ld, None, 0, N.ptr(v['ga']), None, None, None))

        def wg(generic):
            dw = torch.zeros(Nout, Cin, 3, 3, device=DEV)
            if generic:
                assert N.lib().tss_sconv_bwd_weight_rows(B, H, W, Cin, Nout, BF) == 0
                N.call('tss_convkxk_bwd_weight', *gargs, *xargs, N.ptr(dw), B, H, W, Cin, Nout, 3, 3, 2, 1, BF, st)
                chain = X.generic_wgrad_chain(Po, Cin, Nout, 9)
            else:
                rows = N.lib().tss_sconv_bwd_weight_rows(B, H, W, Cin, Nout, BF)
                assert rows > 1
                if cap:
                    assert rows == cap, rows                 # the persistent-grid path: rows at the sweep's grid cap
                ws = torch.full((rows, 9 * Nout * Cin), float('nan'), device=DEV)
                N.call('tss_sconv_bwd_weight_sweep', *gargs, *xargs, N.ptr(ws), B, H, W, Cin, Nout, BF, st)
                from torch_semantic_segmentation_amd import ops
                ops._reduce_rows_now(ws, dw, 9 * Nout * Cin, rows)
                # stages: 32 output pixels for sw<64>, 64 for sw<32> and every swr
                chain = X.sweep_chain(Po, 32 if (Nout == 64 and Cin == 64) else 64, rows)
            torch.cuda.synchronize()
            ex = X.wgrad_excess(dw.double().cpu(), ref, S, chain)
            assert ex <= 0, ('sconv wgrad', with_y, generic, ex)
        in_modes(wg)


# ----------------------------------------------------------------------------------------------------- benchmark-size maps
@pytest.mark.parametrize('kind', ['fc1d', 'fcg', 'sconv', 'transposed'])
def test_benchmark_size_maps_within_the_exact_bound(kind):
    """the maps of the benchmark's 8 x 3 x 1024 x 2048 at 1/8 resolution, 128 x 256 (LEDNet's 64 channels at batch 8; ESNet's 128-channel
    three-tap layers and its ConvTranspose2d(128, 64) at batch 2): forward and backward-data"""
    if kind == 'fc1d':
        run_tap_layer(64, 3, 8, 128, 256, 1, 1, True, True, True, seed=9)
    elif kind == 'fcg':
        run_tap_layer(128, 3, 2, 128, 256, 0, 2, True, True, True, seed=10)
    elif kind == 'transposed':
        test_sconv_transposed_instances_within_the_exact_bound(128, 64, 64, 128)
    else:
        test_sconv_forward_instances_within_the_exact_bound(64, 64, 128, 256)
        test_sconv_backward_data_instances_within_the_exact_bound(64, 64, 128, 256, True)


# ----------------------------------------------------------------------------------------------------- ssnbt tail
def _ulp(v, dtype):
    mant = 7 if dtype == torch.bfloat16 else 23
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -100)))
    return torch.pow(2.0, e - mant)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('mkind', [None, True, False])
@pytest.mark.parametrize('C', [32, 128])
def test_ssnbt_tail_against_its_emulation(C, mkind, dtype):
    N = N_()
    st = N.stream()
    B, HW = 3, 37
    P, H = B * HW, C // 2
    g = torch.Generator().manual_seed(C + (mkind is None) * 7 + (mkind is True) * 3)
    l, r, x = X.dyadic((P, H), g), X.dyadic((P, H), g), X.dyadic((P, C), g)
    ml, mr, bl, br = (X.dyadic((H,), g) for _ in range(4))
    sl, sr = X.pow2((H,), g, 0.5, 4), X.pow2((H,), g, 0.5, 4)
    if mkind is None:
        m = None
    elif mkind:
        m = (torch.rand((B, C), generator=g) < 0.5).double() * 2.0          # p = 0.5: 0 or 2, zeroed channels
    else:
        m = ((torch.rand((B, C), generator=g) < 0.7).double() / 0.7).float().double()     # p = 0.3: 1 / 0.7 is not dyadic
    bimg = torch.arange(P) // HW
    y = torch.cat([(l - ml) * sl + bl, (r - mr) * sr + br], 1)
    if m is not None:
        y = y * m[bimg]
    if mkind is not False:
        # exact zeros of x + y, planted where -y is a bf16 value: relu's > 0 convention forward and backward
        cand = (-y).float().to(torch.bfloat16).double()
        pick = (torch.rand((P, C), generator=g, dtype=torch.float64) < 0.05) & cand.eq(-y) & y.ne(0)
        assert pick.any()
        x = torch.where(pick, -y, x)
    pre = x + y
    code = N.dtype_code(dtype)
    sh = pre.reshape(P, 2, H).transpose(1, 2).reshape(P, C).clamp_min(0.0)      # out[p][2j + g] = relu(pre[p][g H + j])
    exp_out = sh.float().to(dtype).double()
    Lb, Rb = Buf(P, H, H + 8, 0, l, dtype), Buf(P, H, H + 8, 0, r, dtype)
    Xb = Buf(P, C, C + 8, 0, x, dtype)
    cv = [dev(t) for t in (ml, sl, bl, mr, sr, br)]
    md = dev(m)
    dout = X.dyadic((P, C), torch.Generator().manual_seed(C))
    Db = Buf(P, C, C + 8, 0, dout, dtype)

    def run(generic):
        ob = Buf(P, C, C + 16, 8, dtype=dtype)
        N.call('tss_ssnbt_tail_fwd', Lb.ptr, Lb.ld, *(N.ptr(t) for t in cv[:3]), Rb.ptr, Rb.ld, *(N.ptr(t) for t in cv[3:]), Xb.ptr, Xb.ld,
               N.ptr(md), ob.ptr, ob.ld, B, HW, C, code, st)
        torch.cuda.synchronize()
        got = ob.rows()
        assert ob.untouched()
        if mkind is False:
            # 1 / 0.7 is not dyadic: m * bn(raw) rounds once in f32 before the sum with x (an FMA may fuse the two); the emulation rounds
            # once at the end.  Two f32 roundings of a value that is then stored: at most 1 ulp of the result
            assert ((got - exp_out).abs() <= _ulp(torch.maximum(exp_out.abs(), got.abs()), dtype)).all()
        else:
            assert torch.equal(got, exp_out)
        # ---- backward, from the kernel's own output
        gsb = Buf(P, C, C + 16, 8, dtype=dtype)
        eb = Buf(P, C, C + 16, 8, dtype=dtype) if m is not None else None
        s_l, s_r = nan_slabs(H), nan_slabs(H)
        N.call('tss_ssnbt_tail_bwd', Db.ptr, Db.ld, ob.ptr, ob.ld, Lb.ptr, Lb.ld, N.ptr(cv[0]), Rb.ptr, Rb.ld, N.ptr(cv[3]), N.ptr(md),
               eb.ptr if eb else None, eb.ld if eb else 0, gsb.ptr, gsb.ld, N.ptr(s_l), N.ptr(s_r), B, HW, C, code, st)
        torch.cuda.synchronize()
        gsh = torch.where(got > 0, dout, torch.zeros_like(dout))                  # relu backward in the shuffled order
        exp_gs = gsh.reshape(P, H, 2).transpose(1, 2).reshape(P, C)               # unshuffle
        assert torch.equal(gsb.rows(), exp_gs) and gsb.untouched()
        if m is not None:
            exp_e = (exp_gs * m[bimg]).float().to(dtype).double()   # an exact product rounded to f32, then stored: the kernel's two steps
            ge = eb.rows()
            assert torch.equal(ge, exp_e) and eb.untouched()
        else:
            ge = exp_gs
        # BatchNorm-backward sums of the branches from the stored e: a thread adds its pixels (B ceil(HW / (grid npl)) of them) in f32
        # for bf16, in f64 for f32; the block's lanes meet in f64
        npl = 256 // (H // 8)
        grid = min(X.cdiv(HW, npl), N.stat_slabs())
        chain = B * X.cdiv(HW, grid * npl)
        for half, raw, mean, slab in ((0, l, ml, s_l), (1, r, mr, s_r)):
            ee = ge[:, half * H:(half + 1) * H]
            terms = torch.cat([ee, ee * (raw - mean)], 1)
            sc = slab.cpu()
            assert not torch.isnan(sc).any()
            if dtype == torch.float32:
                # f64 sums of terms exact in f64, fewer than 2^13 of them: within 2^-40 sum|terms|
                assert ((sc.sum(0) - terms.sum(0)).abs() <= 2.0 ** -40 * terms.abs().sum(0)).all()
            else:
                assert X.stats_excess(sc.sum(0), terms, chain) <= 0
    in_modes(run)


# ----------------------------------------------------------------------------------------------------- zoo glue
def test_channel_shuffle_cat2_add_pad_channels_are_bit_exact():
    N = N_()
    st = N.stream()
    g = torch.Generator().manual_seed(1)
    P, C = 301, 48
    x = X.dyadic((P, C), g)
    xb = Buf(P, C, C + 8, 0, x)
    half = 24
    gl, gr, gs = X.dyadic((P, half), g), X.dyadic((P, half), g), X.dyadic((P, 2 * half), g)
    Lb, Rb, Sb = Buf(P, half, half + 8, 0, gl), Buf(P, half, half + 8, 0, gr), Buf(P, 2 * half, 2 * half + 8, 0, gs)
    Cp, Cr = 24, 19
    gg = X.dyadic((P, Cr), g)
    Gb = Buf(P, Cr, 40, 0, gg)

    def run(generic):
        for groups in (2, 3):
            yb = Buf(P, C, C + 16, 8)
            N.call('tss_channel_shuffle', xb.ptr, xb.ld, yb.ptr, yb.ld, P, C, groups, N.TSS_BF16, st)
            torch.cuda.synchronize()
            exp = x.reshape(P, groups, C // groups).transpose(1, 2).reshape(P, C)
            assert torch.equal(yb.rows(), exp) and yb.untouched()
        for with_s in (False, True):
            ob = Buf(P, 2 * half, 2 * half + 16, 8)
            N.call('tss_cat2_add', Lb.ptr, Lb.ld, Rb.ptr, Rb.ld, Sb.ptr if with_s else None, Sb.ld if with_s else 0, ob.ptr, ob.ld, P, half,
                   N.TSS_BF16, st)
            torch.cuda.synchronize()
            exp = torch.cat([gl, gr], 1) + (gs if with_s else 0)      # one exact f32 sum of two dyadic values, one rounding
            assert torch.equal(ob.rows(), exp.float().to(torch.bfloat16).double()) and ob.untouched()
        ob = Buf(P, Cp, Cp + 16, 8)
        N.call('tss_pad_channels', Gb.ptr, Gb.ld, Cr, ob.ptr, ob.ld, Cp, P, N.TSS_BF16, st)
        torch.cuda.synchronize()
        o = ob.rows()
        assert torch.equal(o[:, :Cr], gg) and not o[:, Cr:].any() and ob.untouched()
    in_modes(run)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_bn_bwd_apply_scale_rows_mul_addrows_against_their_emulation(dtype):
    """bit-identity where one rounding follows exact f32 arithmetic; dr of mul_addrows_bwd (a reduction) under an f32 chain bound"""
    N = N_()
    st = N.stream()
    code = N.dtype_code(dtype)
    g = torch.Generator().manual_seed(2)
    B, HW, C = 3, 257, 48
    P = B * HW
    bimg = torch.arange(P) // HW
    rnd = lambda t: t.float().to(dtype).double()
    e, z = X.dyadic((P, C), g), X.dyadic((P, C), g)
    ga, gb = X.pow2((C,), g, 0.25, 2), X.pow2((C,), g, 2.0 ** -6, 2.0 ** -3)
    gce, gmu = X.dyadic((C,), g), X.dyadic((C,), g)
    m = (torch.rand((B, C), generator=g) < 0.5).double() * 2.0
    # mul_addrows operands with exponents in [-1, 2): u a (16 significant bits, 2^-16 .. 2^4) + r (2^-8 .. 2^2) spans 21 bits, exact in f32
    u, a, rr = X.dyadic((P, C), g, -1, 2), X.dyadic((P, C), g, -1, 2), X.dyadic((B, C), g, -1, 2)
    gr = X.dyadic((P, C), g)
    Eb, Zb = Buf(P, C, C + 8, 0, e, dtype), Buf(P, C, C + 8, 0, z, dtype)
    Ub, Ab, Rb, Gb = Buf(P, C, C + 8, 0, u, dtype), Buf(P, C, C + 8, 0, a, dtype), Buf(B, C, C + 8, 0, rr, dtype), Buf(P, C, C + 8, 0, gr, dtype)
    dga, dgb, dgce, dgmu, dm = dev(ga), dev(gb), dev(gce), dev(gmu), dev(m)

    def run(generic):
        for with_y in (False, True):
            ob = Buf(P, C, C + 16, 8, dtype=dtype)
            if with_y:
                N.call('tss_bn_bwd_apply', Eb.ptr, Eb.ld, Zb.ptr, Zb.ld, N.ptr(dga), N.ptr(dgb), N.ptr(dgce), N.ptr(dgmu), ob.ptr, ob.ld, P, C,
                       code, st)
                exp = rnd(ga * (e - gce) + gb * (z - gmu))
            else:
                N.call('tss_bn_bwd_apply', Eb.ptr, Eb.ld, None, 0, N.ptr(dga), None, None, None, ob.ptr, ob.ld, P, C, code, st)
                exp = rnd(ga * e)
            torch.cuda.synchronize()
            assert torch.equal(ob.rows(), exp) and ob.untouched(), ('bn_bwd_apply', with_y)
        ob = Buf(P, C, C + 16, 8, dtype=dtype)
        N.call('tss_scale_rows', Eb.ptr, Eb.ld, N.ptr(dm), ob.ptr, ob.ld, B, HW, C, code, st)
        torch.cuda.synchronize()
        assert torch.equal(ob.rows(), rnd(e * m[bimg])) and ob.untouched()
        ob = Buf(P, C, C + 16, 8, dtype=dtype)
        N.call('tss_mul_addrows_fwd', Ub.ptr, Ub.ld, Ab.ptr, Ab.ld, Rb.ptr, Rb.ld, ob.ptr, ob.ld, B, HW, C, code, st)
        torch.cuda.synchronize()
        assert torch.equal(ob.rows(), rnd(u * a + rr[bimg])) and ob.untouched()
        S = N.lib().tss_rows_slices(B, HW)
        ws = torch.full((B * S * C,), float('nan'), device=DEV)
        dub, dab, drb = Buf(P, C, C + 16, 8, dtype=dtype), Buf(P, C, C + 16, 8, dtype=dtype), Buf(B, C, C + 16, 8, dtype=dtype)
        N.call('tss_mul_addrows_bwd', Gb.ptr, Gb.ld, Ub.ptr, Ub.ld, Ab.ptr, Ab.ld, dub.ptr, dub.ld, dab.ptr, dab.ld, drb.ptr, drb.ld, N.ptr(ws),
               B, HW, C, code, st)
        torch.cuda.synchronize()
        assert torch.equal(dub.rows(), rnd(gr * a)) and dub.untouched()
        assert torch.equal(dab.rows(), rnd(gr * u)) and dab.untouched()
        # dr[b] = sum over the image of g: per (image, slice) block, a lane adds ceil(ceil(HW / S) / npl) pixels in f32, the block's npl
        # lanes are added in f32, then the S slices in f32 (rows_reduce_kernel) -- the chain; then one rounding to the dtype
        npl = 256 // (C // 8)
        chain = X.cdiv(X.cdiv(HW, S), npl) + npl + S
        ref = torch.zeros(B, C, dtype=torch.float64).index_add_(0, bimg, gr)
        Sabs = torch.zeros(B, C, dtype=torch.float64).index_add_(0, bimg, gr.abs())
        assert X.conv_excess(drb.rows(), ref, Sabs, chain) <= 0 and drb.untouched()
    in_modes(run)


@pytest.mark.parametrize('P,C', [(1000, 19), (3000, 48)])
def test_tensor_stats_within_the_statistics_bound(P, C):
    """the scalar kernel (C % 8 != 0) and the vector kernel (P >= 4 x 512 slabs): per-lane f64 sums of bf16 values and their exact
    squares, fewer than 2^13 terms per sum: within 2^-40 sum|terms|"""
    N = N_()
    z = X.dyadic((P, C), torch.Generator().manual_seed(P))
    Zb = Buf(P, C, C + 13 if C % 8 else C + 8, 0, z)
    terms = torch.cat([z, z * z], 1)

    def run(generic):
        sl = nan_slabs(C)
        N.call('tss_tensor_stats', Zb.ptr, Zb.ld, P, C, N.ptr(sl), N.TSS_BF16, N.stream())
        torch.cuda.synchronize()
        s = sl.cpu()
        assert not torch.isnan(s).any()
        assert ((s.sum(0) - terms.sum(0)).abs() <= 2.0 ** -40 * terms.abs().sum(0)).all()
    in_modes(run)


def _pool_ref(x):
    """max_pool2d(x, 2) of [B][C][H][W] f64 and torch's arg-max indices (first maximum in row-major window order)"""
    return torch.nn.functional.max_pool2d(x, 2, return_indices=True)


@pytest.mark.parametrize('path', ['vec', 'img', 'scalar'])
def test_pool_concat_forward_and_backward_are_bit_exact_with_ties(path):
    """z = cat([y1 + bias, max_pool2d(x, 2)]); the gradient of the pooled channels goes to torch's first-max index of each window.
    x takes four values only, so most windows hold ties.  Paths: NHWC bf16 vectors, the NCHW f32 image, the element-wise kernel"""
    N = N_()
    st = N.stream()
    g = torch.Generator().manual_seed(4)
    B, Hin, Win = 2, 10, 14
    Ho, Wo = Hin // 2, Win // 2
    N1, Cin = {'vec': (16, 16), 'img': (13, 3), 'scalar': (12, 4)}[path]
    vals = torch.tensor([-1.0, 0.0, 0.5, 1.0], dtype=torch.float64)
    x = vals[torch.randint(0, 4, (B, Cin, Hin, Win), generator=g)]
    pooled, idx = _pool_ref(x)
    assert (x.unfold(2, 2, 2).unfold(3, 2, 2).reshape(B, Cin, Ho, Wo, 4) == pooled.unsqueeze(-1)).sum(-1).gt(1).any()    # ties exist
    Po = B * Ho * Wo
    y1 = X.dyadic((Po, N1), g)
    bias = X.dyadic((N1,), g)
    Y1 = Buf(Po, N1, N1 + 8 - N1 % 8 if N1 % 8 else N1 + 8, 0, y1)
    if path == 'img':
        xd = x.float().to(DEV).contiguous()
        strides, x_f32 = (Cin * Hin * Win, Hin * Win, Win, 1), 1
    else:
        ldx = Cin + (8 if path == 'vec' else 4)
        Xb = Buf(B * Hin * Win, Cin, ldx, 0, to_rows(x))
        xd = Xb.t
        strides, x_f32 = (Hin * Win * ldx, 1, Win * ldx, ldx), 0
    bd = dev(bias)
    exp_z = torch.cat([(y1 + bias).float().to(torch.bfloat16).double(), to_rows(pooled)], 1)
    dzv = X.dyadic((Po, N1 + Cin), g)
    dz = Buf(Po, N1 + Cin, N1 + Cin + 8, 0, dzv)
    gpool = dzv[:, N1:].reshape(B, Ho, Wo, Cin).permute(0, 3, 1, 2)
    exp_dx = torch.zeros(B, Cin, Hin * Win, dtype=torch.float64).scatter_(2, idx.reshape(B, Cin, -1), gpool.reshape(B, Cin, -1))
    exp_dx = to_rows(exp_dx.reshape(B, Cin, Hin, Win))

    def run(generic):
        zb = Buf(Po, N1 + Cin, N1 + Cin + 16 if path != 'scalar' else N1 + Cin + 4, 8 if path != 'scalar' else 2)
        N.call('tss_pool_concat_fwd', Y1.ptr, Y1.ld, N.ptr(bd), N1, xd.data_ptr(), x_f32, *strides, Cin, zb.ptr, zb.ld, B, Hin, Win,
               N.TSS_BF16, st)
        torch.cuda.synchronize()
        assert torch.equal(zb.rows(), exp_z) and zb.untouched()
        dxb = Buf(B * Hin * Win, Cin, Cin + 8, 0)
        N.call('tss_pool_concat_bwd', dz.ptr, dz.ld, N1, xd.data_ptr(), x_f32, *strides, Cin, dxb.ptr, dxb.ld, B, Hin, Win, N.TSS_BF16, st)
        torch.cuda.synchronize()
        assert torch.equal(dxb.rows(), exp_dx) and dxb.untouched()
    in_modes(run)


# ----------------------------------------------------------------------------------------------------- ops.ssnbt_tail envelope
def test_ssnbt_tail_outside_the_kernel_envelope_takes_the_four_operators():
    """C = 544 > 512: ops.ssnbt_tail must fall back to concat_joined -> channel_dropout -> join -> channel_shuffle (it raised TSS_ERR_SHAPE)"""
    from torch_semantic_segmentation_amd import ops
    B, C, H, W = 2, 544, 3, 5
    half = C // 2
    results = []
    for fused in (True, False):
        torch.manual_seed(3)
        bnl, bnr = torch.nn.BatchNorm2d(half).to(DEV), torch.nn.BatchNorm2d(half).to(DEV)
        convl = torch.nn.Conv2d(half, half, 1, bias=False).to(DEV)
        convr = torch.nn.Conv2d(half, half, 1, bias=False).to(DEV)
        x = ops.to_nhwc(torch.randn(B, C, H, W, device=DEV)).requires_grad_(True)
        xl, xr, xs = ops.split_fork(x)
        left = ops.conv_unit(xl, convl, bnl, False)
        right = ops.conv_unit(xr, convr, bnr, False)
        old = ops.fuse_ssnbt_tail
        ops.fuse_ssnbt_tail = fused
        try:
            out = ops.ssnbt_tail(left, right, xs, 0.0, True)
        finally:
            ops.fuse_ssnbt_tail = old
        out.backward(ops.to_nhwc(torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(5)).to(DEV)))
        torch.cuda.synchronize()
        results.append((out.detach().float(), x.grad.float(), convl.weight.grad.clone(), bnr.bias.grad.clone()))
    for a, b in zip(*results):
        assert torch.equal(a, b)
