"""The exact-operand method of tests/exact.py checked on the CPU (no GPU): its premise (the on-load transforms are exact in f32), the
soundness of its bounds (an f32 emulation of each convolution from the same bf16 operands passes) and their sharpness (the same emulation
with one realistic kernel defect fails)."""
import numpy as np
import pytest
import torch

from tests import exact as X
from tests import philox_ref as PR


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_dyadic_transforms_are_exact_in_f32_in_every_order():
    g = _gen(0)
    n = 1 << 20
    x, mean, bias = X.dyadic((n,), g), X.dyadic((n,), g), X.dyadic((n,), g)
    scale = X.pow2((n,), g, 0.5, 4)
    ref = (x - mean) * scale + bias
    f = lambda t: t.float()
    plain = (f(x) - f(mean)) * f(scale) + f(bias)
    folded = f(x) * f(scale) + (f(bias) - f(mean) * f(scale))
    assert torch.equal(plain.double(), ref) and torch.equal(folded.double(), ref)
    e, y, gce, gmu = X.dyadic((n,), g), X.dyadic((n,), g), X.dyadic((n,), g), X.dyadic((n,), g)
    ga, gb = X.pow2((n,), g, 0.25, 2), X.pow2((n,), g, 2.0 ** -6, 2.0 ** -3)
    ref = ga * (e - gce) + gb * (y - gmu)
    plain = f(ga) * (f(e) - f(gce)) + f(gb) * (f(y) - f(gmu))
    folded = (f(e) * f(ga) + (-(f(ga) * f(gce)) - f(gb) * f(gmu))) + f(y) * f(gb)     # fc1d / fcg / sconv order
    sweep = f(ga) * f(e) + f(gb) * f(y) + (-(f(ga) * f(gce)) - f(gb) * f(gmu))        # the weight-gradient sweeps' order
    assert torch.equal(plain.double(), ref) and torch.equal(folded.double(), ref) and torch.equal(sweep.double(), ref)
    # the backward-statistics factor (x - mean) and its product with a bf16 value are exact as well
    r = X.rne_bf16(X.dyadic((n,), g) * 3)
    assert torch.equal((f(r) * (f(x) - f(mean))).double(), r * (x - mean))


# ---------------------------------------------------------------------------------------------------------- f32 emulation
def _shift(a, off, axis, flat_images=False):
    """a [B][C][H][W] read at (h, w + off) (axis 0) or (h + off, w) (axis 1), zero outside the image (flat_images: outside the B*H stack)"""
    B, C, H, W = a.shape
    if axis == 1 and flat_images:
        s = a.permute(1, 0, 2, 3).reshape(1, C, B * H, W)
        return _shift(s, off, 1).reshape(C, B, H, W).permute(1, 0, 2, 3)
    out = torch.zeros_like(a)
    n = W if axis == 0 else H
    lo, hi = max(0, -off), min(n, n - off)
    if lo < hi:
        if axis == 0:
            out[..., lo:hi] = a[..., lo + off:hi + off]
        else:
            out[:, :, lo:hi] = a[:, :, lo + off:hi + off]
    return out


def _emulate_taps(a, w, axis, dil, flat_images=False, ragged_tile=0):
    """f32 sum over taps and channels of a T-tap layer, as a kernel computes it; ragged_tile > 0: the last tap of the last (partial)
    ragged_tile-pixel column tile of every row reads one pixel too far (a halo off by one)"""
    T = w.shape[-1]
    a32, w32 = a.float(), w.float()
    out = torch.zeros(a.shape[0], w.shape[0], a.shape[2], a.shape[3])
    for t in range(T):
        off = (t - T // 2) * dil
        src = _shift(a32, off, axis, flat_images)
        if ragged_tile and t == T - 1:
            W = a.shape[3]
            x0 = (W // ragged_tile) * ragged_tile
            bad = _shift(a32, off + 1, axis)
            src[..., x0:] = bad[..., x0:]
        out += torch.einsum('bchw,nc->bnhw', src, w32[:, :, t])
    return out


def _tap_case(seed, C=32, T=3, B=2, H=5, W=37, axis=0, dil=2):
    g = _gen(seed)
    a = X.rne_bf16(X.dyadic((B, C, H, W), g, zero_frac=0.05))
    w = X.dyadic((C, C, T), g, emin=-6, emax=-2)
    return a, w


def _tap_ref(a, w, axis, dil):
    T = w.shape[-1]
    ks, pad, dl = X.tap_geom(T, axis, dil)
    return X.conv_ref(a, w.reshape(w.shape[0], w.shape[1], *ks), padding=pad, dilation=dl)


@pytest.mark.parametrize('axis,dil,T', [(0, 1, 3), (0, 9, 3), (1, 2, 3), (1, 5, 5), (0, 17, 5)])
def test_f32_emulation_of_a_tap_layer_meets_the_bound(axis, dil, T):
    a, w = _tap_case(axis * 10 + dil, T=T, axis=axis, dil=dil)
    ref, S = _tap_ref(a, w, axis, dil)
    out = X.rne_bf16(_emulate_taps(a, w, axis, dil).double())
    assert X.conv_excess(out, ref, S, T * w.shape[1]) <= 0


def test_f32_emulation_of_the_strided_and_transposed_3x3_meets_the_bound():
    g = _gen(7)
    a = X.rne_bf16(X.dyadic((2, 16, 9, 12), g))
    w = X.dyadic((24, 16, 3, 3), g, emin=-6, emax=-2)
    ref, S = X.conv_ref(a, w, stride=2, padding=1)
    out = torch.nn.functional.conv2d(a.float(), w.float(), stride=2, padding=1)
    assert X.conv_excess(X.rne_bf16(out.double()), ref, S, 9 * 16) <= 0
    wt = X.dyadic((16, 24, 3, 3), g, emin=-6, emax=-2)
    ref, S = X.convT_ref(a, wt)
    out = torch.nn.functional.conv_transpose2d(a.float(), wt.float(), stride=2, padding=1, output_padding=1)
    assert X.conv_excess(X.rne_bf16(out.double()), ref, S, 9 * 16) <= 0


def test_one_dropped_tap_of_one_channel_at_one_pixel_fails():
    a, w = _tap_case(1, axis=0, dil=2)
    ref, S = _tap_ref(a, w, 0, 2)
    out = _emulate_taps(a, w, 0, 2)
    b, h, x = 1, 3, 20
    src = torch.stack([_shift(a.float(), (t - 1) * 2, 0)[b, :, h, x] for t in range(3)], 1)        # [C][T]
    n = 5
    terms = w[n].float() * src                                                                     # [C][T] of output channel n
    c, t = divmod(int(terms.abs().argmax()), 3)                                                    # the largest term: a defect that matters
    out[b, n, h, x] -= terms[c, t]
    out = X.rne_bf16(out.double())
    assert X.conv_excess(out, ref, S, 3 * w.shape[1]) > 0


def test_a_halo_shifted_by_one_pixel_at_a_ragged_tile_end_fails():
    a, w = _tap_case(2, W=37, axis=0, dil=1)
    ref, S = _tap_ref(a, w, 0, 1)
    out = X.rne_bf16(_emulate_taps(a, w, 0, 1, ragged_tile=16).double())
    assert X.conv_excess(out, ref, S, 3 * w.shape[1]) > 0


def test_a_three_by_one_tap_across_an_image_boundary_fails():
    a, w = _tap_case(3, B=3, H=4, W=9, axis=1, dil=1)
    ref, S = _tap_ref(a, w, 1, 1)
    out = X.rne_bf16(_emulate_taps(a, w, 1, 1, flat_images=True).double())
    assert X.conv_excess(out, ref, S, 3 * w.shape[1]) > 0


def _wgrad_rows(a, gr, axis, dil, PT, rows):
    """per-block f32 partial rows of dW of a 3-tap layer (blocks own consecutive PT-pixel stages), as the sweep kernels leave them"""
    B, C, H, W = a.shape
    T = 3
    src = torch.stack([_shift(a.float(), (t - 1) * dil, axis) for t in range(T)], -1)             # [B][C][H][W][T]
    srcp = src.permute(0, 2, 3, 1, 4).reshape(B * H * W, C, T)
    gp = gr.float().permute(0, 2, 3, 1).reshape(B * H * W, -1)
    P = B * H * W
    nstage = -(-P // PT)
    per = -(-nstage // rows)
    out = []
    for r in range(rows):
        p0, p1 = min(P, r * per * PT), min(P, (r + 1) * per * PT)
        out.append(torch.einsum('pn,pct->nct', gp[p0:p1], srcp[p0:p1]))
    return out


def test_weight_gradient_rows_meet_the_bound_and_a_left_out_row_fails():
    g = _gen(4)
    B, C, H, W, axis, dil = 2, 16, 30, 50, 1, 2
    a = X.rne_bf16(X.dyadic((B, C, H, W), g, zero_frac=0.05))
    gr = X.rne_bf16(X.dyadic((B, C, H, W), g))
    ks, pad, dl = X.tap_geom(3, axis, dil)
    ref, S = X.conv_weight_ref(a, (C, C) + ks, gr, padding=pad, dilation=dl)
    ref, S = ref.reshape(C, C, 3), S.reshape(C, C, 3)
    PT, rows = 128, 6                                   # P = 3000: 24 stages, 4 per block
    parts = _wgrad_rows(a, gr, axis, dil, PT, rows)
    chain = X.sweep_chain(B * H * W, PT, rows)
    dw = torch.zeros(C, C, 3)
    for p in parts:
        dw += p
    assert X.wgrad_excess(dw.double(), ref, S, chain) <= 0
    dw = torch.zeros(C, C, 3)
    for p in parts[:2] + parts[3:]:
        dw += p
    assert X.wgrad_excess(dw.double(), ref, S, chain) > 0


def test_statistics_slabs_meet_the_bound_and_a_row_not_zeroed_fails():
    g = _gen(5)
    P, C, rows = 2000, 16, 8
    out = X.rne_bf16(X.dyadic((P, C), g))
    terms = torch.cat([out, out * out], 1)
    slabs = torch.full((512, 2 * C), float('nan'), dtype=torch.float64)        # the kernels' contract: every row written or zeroed
    per = P // rows
    for r in range(rows):                                                        # each block: f32 lane sums of its pixels
        slabs[r] = terms[r * per:(r + 1) * per].float().sum(0).double()
    slabs[rows:] = 0.0
    chain = per + 4
    assert X.stats_excess(slabs.sum(0), terms, chain) <= 0
    slabs[rows + 3] = float('nan')
    assert not (X.stats_excess(slabs.sum(0), terms, chain) <= 0)
    slabs[rows + 3] = slabs[0]                                                  # a stale row from an earlier call
    assert X.stats_excess(slabs.sum(0), terms, chain) > 0


# ---------------------------------------------------------------------------------------------------------- depthwise 3x3 family
# f32 emulation of csrc/dwconv.hip / dwroll.hip: unrounded f32 operands a and g, f32 weights, every product rounded on its own (no FMA)
# and added to a running f32 sum tap by tap; the weight gradient per (image, row segment) block -- a lane per column adds its rows, the
# block adds its lanes one after the other, the rows are added one after the other onto dW
def _dw_tap(a, ky, kx, stride, dil, Ho, Wo):
    """a [B][C][H][W] read at (oy stride + (ky - 1) dil, ox stride + (kx - 1) dil) for every output pixel, zero outside"""
    B, C, H, W = a.shape
    pad = torch.zeros(B, C, H + 2 * dil, W + 2 * dil, dtype=a.dtype)
    pad[:, :, dil:dil + H, dil:dil + W] = a
    y0, x0 = ky * dil, kx * dil
    return pad[:, :, y0:y0 + (Ho - 1) * stride + 1:stride, x0:x0 + (Wo - 1) * stride + 1:stride]


def _dw_case(seed, B=2, C=16, H=11, W=19, stride=1, relu=True):
    g = _gen(seed)
    mean, bias, scale = X.dyadic((1, C, 1, 1), g), X.dyadic((1, C, 1, 1), g), X.pow2((1, C, 1, 1), g, 0.5, 4)
    x = X.plant_zeros(X.dyadic((B, C, H, W), g), mean, scale, bias, g, 0.05)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    w = (torch.randn((C, 1, 3, 3), generator=g) * 0.25).double()                       # f32 weights with all 24 bits in use
    e, y = X.dyadic((B, C, Ho, Wo), g), X.dyadic((B, C, Ho, Wo), g)
    ga, gb = X.pow2((1, C, 1, 1), g, 0.25, 2), X.pow2((1, C, 1, 1), g, 2.0 ** -6, 2.0 ** -3)
    gce, gmu = X.dyadic((1, C, 1, 1), g), X.dyadic((1, C, 1, 1), g)
    a = X.act_f32(x, mean, scale, bias, relu)
    gop = X.gcomb_f32(e, y, ga, gb, gce, gmu)
    mask = (X.pre_act(x, mean, scale, bias) > 0).double() if relu else torch.ones_like(x)
    mask_ge = (X.pre_act(x, mean, scale, bias) >= 0).double()
    return dict(x=x, a=a, w=w, gop=gop, mask=mask, mask_ge=mask_ge, Ho=Ho, Wo=Wo, C=C, stride=stride)


def _dw_fwd_emulated(a, w, stride, dil, Ho, Wo, defect=None, strip=8):
    a32, w32 = a.float(), w.float()
    acc = torch.zeros(a.shape[0], a.shape[1], Ho, Wo)
    for ky in range(3):
        for kx in range(3):
            src = _dw_tap(a32, ky, kx, stride, dil, Ho, Wo).clone()
            if defect == 'halo' and kx == 2:
                # the right halo column of the last, ragged strip: clamped to the row's last pixel and not masked
                assert Wo % strip != 0 and stride == 1 and dil == 1
                src[..., Wo - 1] = _dw_tap(a32, ky, 1, stride, dil, Ho, Wo)[..., Wo - 1]
            acc = acc + src * w32[:, 0, ky, kx].view(1, -1, 1, 1)
    return acc


def _dw_bwd_data_emulated(gop, w, shape, stride, dil, mask, defect=None):
    """input gradient as the kernels gather it: per input pixel, the flipped taps over the output pixels that reach it"""
    B, C, H, W = shape
    Ho, Wo = gop.shape[2:]
    g32, w32 = gop.float(), w.float().clone()
    if defect == 'mirror_tap':
        w32[:, 0, 1, 0], w32[:, 0, 1, 2] = w32[:, 0, 1, 2].clone(), w32[:, 0, 1, 0].clone()
    up = torch.zeros(B, C, (Ho - 1) * stride + 1 + 2 * dil, (Wo - 1) * stride + 1 + 2 * dil)      # g on the input grid, zero between
    up[:, :, dil:dil + (Ho - 1) * stride + 1:stride, dil:dil + (Wo - 1) * stride + 1:stride] = g32
    full = torch.zeros(B, C, max(H, (Ho - 1) * stride + 1) + 2 * dil, max(W, (Wo - 1) * stride + 1) + 2 * dil)
    full[:, :, :up.shape[2], :up.shape[3]] = up
    acc = torch.zeros(B, C, H, W)
    for ky in range(3):
        for kx in range(3):
            y0, x0 = (2 - ky) * dil, (2 - kx) * dil                     # input pixel (iy, ix) sees output position iy - (ky - 1) dil
            acc = acc + full[:, :, y0:y0 + H, x0:x0 + W] * w32[:, 0, ky, kx].view(1, -1, 1, 1)
    return acc * mask.float()


def _dw_wgrad_emulated(a, gop, stride, dil, RS, defect=None):
    """(dW [C][1][3][3] in f32, its chain): blocks = (image, segment of RS output rows); a lane per output column"""
    B, C, Ho, Wo = gop.shape
    a32, g32 = a.float(), gop.float()
    nseg = -(-Ho // RS)
    rows = []
    for b in range(B):
        for s in range(nseg):
            o0, o1 = s * RS, min(Ho, (s + 1) * RS)
            if defect == 'row_twice' and s > 0:
                o0 -= 1                                                  # the boundary row of the segment above is counted again
            part = torch.zeros(C, 3, 3)
            for ky in range(3):
                for kx in range(3):
                    src = _dw_tap(a32, ky, kx, stride, dil, Ho, Wo)[b]
                    lane = torch.zeros(C, Wo)
                    for o in range(o0, o1):
                        lane = lane + g32[b, :, o] * src[:, o]
                    tot = torch.zeros(C)
                    for p in range(Wo):
                        tot = tot + lane[:, p]
                    part[:, ky, kx] = tot
            rows.append(part)
    dw = torch.zeros(C, 3, 3)
    for r in rows:
        dw = dw + r
    return dw.reshape(C, 1, 3, 3), 2 * RS + Wo + len(rows)


def _dw_refs(c, dil):
    return X.dw_refs(c['a'], c['w'], c['gop'], c['x'].shape, c['stride'], dil)


DW_GEOMS = [(1, 1), (2, 1), (1, 4), (2, 2), (1, 3)]


@pytest.mark.parametrize('stride,dil', DW_GEOMS)
def test_f32_emulation_of_the_depthwise_layer_meets_the_unrounded_operand_bounds(stride, dil):
    c = _dw_case(stride * 10 + dil, stride=stride)
    (ref, S), (rin, Sin), (rw, Sw) = _dw_refs(c, dil)
    out = _dw_fwd_emulated(c['a'], c['w'], stride, dil, c['Ho'], c['Wo'])
    assert X.f32_excess(out.double(), ref, S, 9) <= 0
    assert X.conv_excess(X.rne_bf16(out.double()), ref, S, 9) <= 0
    ein = _dw_bwd_data_emulated(c['gop'], c['w'], c['x'].shape, stride, dil, c['mask'])
    assert X.f32_excess(ein.double(), rin * c['mask'], Sin * c['mask'], 9) <= 0
    assert X.conv_excess(X.rne_bf16(ein.double()), rin * c['mask'], Sin * c['mask'], 9) <= 0
    dw, chain = _dw_wgrad_emulated(c['a'], c['gop'], stride, dil, 4)
    assert X.wgrad_excess(dw.double(), rw, Sw, chain) <= 0
    # statistics of the stored bf16 outputs, a lane per column adding its rows in f32, lanes and blocks meeting in f64
    o = X.rne_bf16(out.double())
    terms = torch.cat([X.nchw_to_rows(o), X.nchw_to_rows(o * o)], 1)
    lanes = torch.cat([o.float().sum(2), (o.float() * o.float()).sum(2)], 1)               # [B][2C][Wo]: f32 over the rows
    assert X.stats_excess(lanes.double().sum((0, 2)), terms, c['Ho']) <= 0


@pytest.mark.parametrize('defect', ['halo', 'row_twice', 'mask_ge', 'mirror_tap', 'stats_row'])
def test_one_realistic_depthwise_defect_fails_the_bound(defect):
    stride = 2 if defect == 'mirror_tap' else 1
    c = _dw_case(40 + len(defect), stride=stride)
    (ref, S), (rin, Sin), (rw, Sw) = _dw_refs(c, 1)
    if defect == 'halo':
        out = _dw_fwd_emulated(c['a'], c['w'], 1, 1, c['Ho'], c['Wo'], defect=defect)
        ex = X.conv_excess(X.rne_bf16(out.double()), ref, S, 9)
    elif defect == 'row_twice':
        dw, chain = _dw_wgrad_emulated(c['a'], c['gop'], 1, 1, 4, defect=defect)
        ex = X.wgrad_excess(dw.double(), rw, Sw, chain)
    elif defect == 'mask_ge':
        assert (c['mask_ge'] - c['mask']).sum() > 0                      # exact zeros of the pre-activation are planted
        ein = _dw_bwd_data_emulated(c['gop'], c['w'], c['x'].shape, 1, 1, c['mask_ge'])
        ex = X.conv_excess(X.rne_bf16(ein.double()), rin * c['mask'], Sin * c['mask'], 9)
    elif defect == 'mirror_tap':
        ein = _dw_bwd_data_emulated(c['gop'], c['w'], c['x'].shape, 2, 1, c['mask'], defect=defect)
        ex = X.conv_excess(X.rne_bf16(ein.double()), rin * c['mask'], Sin * c['mask'], 9)
    else:
        o = X.rne_bf16(_dw_fwd_emulated(c['a'], c['w'], 1, 1, c['Ho'], c['Wo']).double())
        terms = torch.cat([X.nchw_to_rows(o), X.nchw_to_rows(o * o)], 1)
        lanes = torch.cat([o.float().sum(2), (o.float() * o.float()).sum(2)], 1)
        slabs = lanes.double().sum(2)                                     # one slab row per image
        ex = X.stats_excess(slabs[1:].sum(0), terms, c['Ho'])             # the first block's row never arrives
    print(defect, 'excess over the bound', ex)
    assert ex > 0


def test_dyadic_transforms_are_exact_in_f32_in_the_depthwise_kernels_orders():
    """the orders of csrc/dwconv.hip / dwroll.hip / updw.hip that test_dyadic_transforms_are_exact_in_f32_in_every_order does not list:
    sh' = fma(-mean, scale, bias) then x scale + sh' (strip and roll kernels), g = ga e + (gb y + kd) with kd = -(ga gce) - gb gmu,
    the mask's (x - mean) scale + bias > 0 and x scale + sh' > 0, and the dyadic bilinear blend of tss_updw_*"""
    g = _gen(11)
    n = 1 << 18
    f = lambda t: t.float()
    x, mean, bias = X.dyadic((n,), g), X.dyadic((n,), g), X.dyadic((n,), g)
    scale = X.pow2((n,), g, 0.5, 4)
    ref = (x - mean) * scale + bias
    shp = torch.addcmul(f(bias), -f(mean), f(scale))                       # one rounding at most: exact here
    assert torch.equal((f(x) * f(scale) + shp).double(), ref)
    e, y, gce, gmu = X.dyadic((n,), g), X.dyadic((n,), g), X.dyadic((n,), g), X.dyadic((n,), g)
    ga, gb = X.pow2((n,), g, 0.25, 2), X.pow2((n,), g, 2.0 ** -6, 2.0 ** -3)
    kd = -(f(ga) * f(gce)) - f(gb) * f(gmu)
    assert torch.equal((f(ga) * f(e) + (f(gb) * f(y) + kd)).double(), ga * (e - gce) + gb * (y - gmu))
    # tss_updw_*'s own coordinate formula (ac_scale / ac_tap in f32) gives exactly the f64 weights at every dyadic size pair the GPU cases
    # use (x4, x8, x2, x1, a source of one pixel), and does not at a non-dyadic one
    for n_in, n_out in [(5, 17), (19, 73), (42, 165), (6, 41), (3, 9), (9, 33), (4, 25), (3, 17), (5, 33), (1, 9), (1, 21), (1, 7)]:
        assert X.dyadic_resize(n_in, n_out)
        M = torch.zeros(n_out, n_in, dtype=torch.float64)
        for d, (i0, i1, l0, l1) in enumerate(X.ac_taps_f32(n_in, n_out)):
            M[d, i0] += l0.double()
            M[d, i1] += l1.double()
        assert torch.equal(M, X.bilinear_matrix(n_in, n_out)), (n_in, n_out)
    assert not X.dyadic_resize(5, 18) and not X.dyadic_resize(9, 30) and not X.dyadic_resize(6, 22) and not X.dyadic_resize(7, 50)
    M = torch.zeros(18, 5, dtype=torch.float64)
    for d, (i0, i1, l0, l1) in enumerate(X.ac_taps_f32(5, 18)):
        M[d, i0] += l0.double()
        M[d, i1] += l1.double()
    assert not torch.equal(M, X.bilinear_matrix(5, 18)) and (M - X.bilinear_matrix(5, 18)).abs().max() < 2.0 ** -20
    # the blend at a dyadic size pair (3 -> 9 rows, 5 -> 33 columns) with the kernel's own f32 weights, in lerp_store's order
    xs = X.dyadic((2, 3, 3, 5), g)
    _, v = X.upsampled_operand(xs, 9, 33)
    X.exact_f32(v)
    for oy, (i0, i1, l0y, l1y) in enumerate(X.ac_taps_f32(3, 9)):
        for ox, (j0, j1, l0x, l1x) in enumerate(X.ac_taps_f32(5, 33)):
            a, b_, c_, d = (f(xs[:, :, r, q]) for r, q in ((i0, j0), (i0, j1), (i1, j0), (i1, j1)))
            o = l0y * (l0x * a + l1x * b_) + l1y * (l0x * c_ + l1x * d)
            assert torch.equal(o.double(), v[:, :, oy, ox])


# ---------------------------------------------------------------------------------------------------------- pointwise (1x1) family
# f32 emulation of csrc/pwfast.hip, wgrad.hip (wgfast_kernel + wgreduce.h), pwbwd.hip and pwsweep.hip in their planners' order: rows are
# pixels, operands a / g already rounded to bf16, every product exact, the f32 sum walked in 8-channel steps of 128-channel chunks
# (forward, backward-data) or stage by stage (weight gradient); statistics per block and lane as the epilogues add them
def _pw_case(seed, P, K, N, zero_frac=0.05):
    g = _gen(seed)
    a = X.rne_bf16(X.dyadic((P, K), g, zero_frac=zero_frac))
    w = X.dyadic((N, K), g, emin=-6, emax=-2)
    gr = X.rne_bf16(X.dyadic((P, N), g))
    return a, w, gr


def _as_map(rows):
    """[P][C] rows as the [1][C][P][1] map the f64 references take"""
    return rows.t().reshape(1, rows.shape[1], rows.shape[0], 1)


def _pw_ref(a, w):
    ref, S = X.conv_ref(_as_map(a), w.reshape(*w.shape, 1, 1))
    return X.nchw_to_rows(ref), X.nchw_to_rows(S)


def _pw_wref(a, gr):
    ref, S = X.conv_weight_ref(_as_map(a), (gr.shape[1], a.shape[1], 1, 1), _as_map(gr))
    return ref.reshape(gr.shape[1], a.shape[1]), S.reshape(gr.shape[1], a.shape[1])


def _pw_gemm32(a, w, drop=None):
    """f32 a W^T, 8 channels at a time; drop = (pixel, first channel): that 8-channel step never reaches the accumulator of that pixel"""
    a32, w32 = a.float(), w.float()
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k0 in range(0, a.shape[1], 8):
        step = a32[:, k0:k0 + 8] @ w32[:, k0:k0 + 8].t()
        if drop is not None and drop[1] == k0:
            step[drop[0]] = 0.0
        acc = acc + step
    return acc


def _pw_slabs(out, fac, TM, rows):
    """slab rows of pwfast_kernel / pwfast_mc_kernel from the stored outputs: the tiles dealt to 8 XCD ranges shared by rows / 8 blocks; a
    lane (pixel half, fragment row) adds its TM / 32 pixels per tile in f32, 16 lanes meet in a 4-level tree, the rest is f64"""
    P, C = out.shape
    gs, ntiles = rows // 8, X.cdiv(P, TM)
    per = X.cdiv(ntiles, 8)
    terms = torch.zeros(ntiles * TM, 2 * C)
    terms[:P] = torch.cat([out.float(), out.float() * fac.float()], 1)
    terms = terms.reshape(ntiles, 2, TM // 32, 16, 2 * C)
    slabs = torch.zeros(512, 2 * C, dtype=torch.float64)
    for xcd in range(8):
        for gslot in range(gs):
            lanes = torch.zeros(2, 16, 2 * C)
            for t in range(xcd * per + gslot, min(xcd * per + per, ntiles), gs):
                for m in range(TM // 32):
                    lanes = lanes + terms[t, :, m]
            for half in (8, 4, 2, 1):
                lanes = lanes[:, :half] + lanes[:, half:2 * half]
            slabs[xcd + 8 * gslot] = lanes.double().sum((0, 1))
    return slabs


# (P, K, N, backward-data, statistics chain): one tile per block (multi-chunk TM 32, two column chunks); 625 tiles of 64: 79 per range
# over 64 blocks, 2 per block; 1 032 tiles of 32: 3 per block, the last ragged
@pytest.mark.parametrize('P,K,N,bwd,chain', [(1000, 264, 40, False, 5), (3075, 136, 256, False, 5), (40000, 8, 8, False, 2 * 2 + 4),
                                             (33013, 8, 8, True, 1 * 3 + 4)])
def test_f32_emulation_of_the_pointwise_layer_meets_the_bounds_in_the_planners_order(P, K, N, bwd, chain):
    a, w, _ = _pw_case(P + K, P, K, N)
    ref, S = _pw_ref(a, w)
    out = X.rne_bf16(_pw_gemm32(a, w).double())
    assert X.conv_excess(out, ref, S, K) <= 0
    _, TM = X.pwfast_plan(P, K, N, bwd)
    assert X.pwfast_stats_chain(P, K, N, bwd)[0] == chain
    rows = X.pwfast_stats_chain(P, K, N, bwd)[1]
    fac = out if not bwd else X.dyadic((P, N), _gen(1)) - X.dyadic((1, N), _gen(2))
    slabs = _pw_slabs(out, fac, TM, rows)
    assert (slabs[rows:] == 0).all() and (slabs[rows - 8] != 0).any()
    assert X.stats_excess(slabs.sum(0), torch.cat([out, out * fac], 1), chain) <= 0


def test_a_dropped_k_step_of_the_second_contraction_chunk_at_one_pixel_fails():
    P, K, N = 300, 264, 40
    a, w, _ = _pw_case(3, P, K, N, zero_frac=0.0)
    ref, S = _pw_ref(a, w)
    out = X.rne_bf16(_pw_gemm32(a, w, drop=(217, 128 + 40)).double())
    assert X.conv_excess(out, ref, S, K) > 0
    assert X.conv_excess(torch.cat([out[:217], out[218:]]), torch.cat([ref[:217], ref[218:]]), torch.cat([S[:217], S[218:]]), K) <= 0


def test_a_ragged_last_tile_that_repeats_the_previous_tile_fails():
    P, K, N, TM = 200, 48, 96, 64
    a, w, _ = _pw_case(4, P, K, N)
    ref, S = _pw_ref(a, w)
    out = X.rne_bf16(_pw_gemm32(a, w).double())
    p0 = P // TM * TM
    out[p0:] = out[p0 - TM:p0 - TM + (P - p0)]                      # the prefetched tile consumed one iteration late
    assert X.conv_excess(out, ref, S, K) > 0


def _wgfast_slots(a, gr, P, K, N):
    """per-block f32 partial tiles of wgfast_kernel (one output tile: K, N <= 128): split s owns ceil(nstage / nsplit) stages of pt
    pixels, added 32 pixels (one MFMA k-step) at a time"""
    pt, ns, tiles = X.pw_wgrad_split(P, K, N)
    assert tiles == 1
    per = X.cdiv(X.cdiv(P, pt), ns)
    slots = []
    for s in range(ns):
        acc = torch.zeros(N, K)
        for p0 in range(s * per * pt, min((s + 1) * per * pt, P), 32):
            p1 = min(p0 + 32, P, (s + 1) * per * pt)
            acc = acc + gr[p0:p1].float().t() @ a[p0:p1].float()
        slots.append(acc)
    return slots


def _wg_reduce(slots, leave_out=None):
    """tss_wg::reduce_block: wave w adds slots w, w + 4, ..., one thread adds the four waves, the total goes onto dW"""
    waves = []
    for wv in range(4):
        acc = torch.zeros_like(slots[0])
        for q in range(wv, len(slots), 4):
            if q != leave_out:
                acc = acc + slots[q]
        waves.append(acc)
    t = torch.zeros_like(slots[0])
    for acc in waves:
        t = t + acc
    return torch.zeros_like(t) + t


@pytest.mark.parametrize('P,K,N', [(3000, 64, 64), (5000, 128, 128), (517, 48, 8)])
def test_weight_gradient_slots_meet_the_bound_and_a_slot_left_out_fails(P, K, N):
    a, _, gr = _pw_case(5 + P, P, K, N)
    ref, S = _pw_wref(a, gr)
    chain, nws = X.pw_wgrad_chain(P, K, N)
    slots = _wgfast_slots(a, gr, P, K, N)
    assert nws == len(slots) * X.pw_ws_dim(N) * X.pw_ws_dim(K) and len(slots) >= 2
    assert X.wgrad_excess(_wg_reduce(slots).double(), ref, S, chain) <= 0
    assert X.wgrad_excess(_wg_reduce(slots, leave_out=len(slots) - 1).double(), ref, S, chain) > 0


@pytest.mark.parametrize('Cin,Cout,P,sweep', [(8, 8, 512 * 128 + 300, False), (64, 128, 700, False), (32, 192, 64 * 40, True), (192, 32, 32 * 776, True)])
def test_one_sweep_backward_rows_meet_the_bounds_in_the_planners_order(Cin, Cout, P, sweep):
    """pwbwd_kernel / pwsweep_kernel: a block keeps its [Cout][Cin] tile over every tile it owns and writes one row; dw_reduce_block adds
    rows w, w + 16, ... per wave, then the 16 waves, then onto dW"""
    a, _, gr = _pw_case(Cin + P, P, Cin, Cout)
    ref, S = _pw_wref(a, gr)
    plan = X.pwsweep_rows(P, Cin, Cout) if sweep else X.pwbwd_rows(P, Cin, Cout)
    _, TM, _, rows, tpb = plan
    gs, ntiles = rows // 8, X.cdiv(P, TM)
    per = X.cdiv(ntiles, 8)
    ws = torch.zeros(rows, Cout, Cin)
    most = 0
    for xcd in range(8):
        for gslot in range(gs):
            mine = range(xcd * per + gslot, min(xcd * per + per, ntiles), gs)
            most = max(most, len(mine))
            for t in mine:
                for p0 in range(t * TM, min((t + 1) * TM, P), 32):
                    p1 = min(p0 + 32, P)
                    ws[xcd + 8 * gslot] = ws[xcd + 8 * gslot] + gr[p0:p1].float().t() @ a[p0:p1].float()
    assert most == tpb
    waves = []
    for wv in range(X.RED_WAVES):
        acc = torch.zeros(Cout, Cin)
        for r in range(wv, rows, X.RED_WAVES):
            acc = acc + ws[r]
        waves.append(acc)
    dw = torch.zeros(Cout, Cin)
    for acc in waves:
        dw = dw + acc
    assert X.wgrad_excess(dw.double(), ref, S, X.pwbwd_wgrad_chain(plan)) <= 0


def _joined_fwd_case(K, res, relu, seed=0):
    P, N = 300, 24
    a, w, _ = _pw_case(seed + K, P, K, N)
    g = _gen(seed + 9)
    cb, omean, obeta, oscale = X.dyadic((N,), g), X.dyadic((N,), g), X.dyadic((N,), g), X.pow2((N,), g, 0.5, 4)
    resid = X.dyadic((P, N), g, zero_frac=0.05) if res else None
    conv, S = _pw_ref(a, w)
    ref, M = X.joined_fwd_ref(conv, S, cb, omean, oscale, obeta, resid, relu)
    f = lambda t: t.float()
    shift = f(obeta) + (f(cb) - f(omean)) * f(oscale)
    v = _pw_gemm32(a, w) * f(oscale) + shift                       # the epilogue's order: one rounding here ...
    return v, f(resid) if res else None, ref, M


@pytest.mark.parametrize('K', [64, 264])
@pytest.mark.parametrize('res,relu', [(False, False), (False, True), (True, False), (True, True)])
def test_f32_emulation_of_the_joined_forward_epilogue_meets_its_bound(K, res, relu):
    v, resid, ref, M = _joined_fwd_case(K, res, relu)
    if res:
        v = v + resid                                               # ... one here
    if relu:
        v = v.clamp_min(0.0)
    assert X.conv_excess(X.rne_bf16(v.double()), ref, M, K + 2) <= 0


def test_a_joined_forward_epilogue_that_applies_the_relu_before_the_residual_fails():
    v, resid, ref, M = _joined_fwd_case(64, True, True, seed=1)
    assert X.conv_excess(X.rne_bf16((v.clamp_min(0.0) + resid).double()), ref, M, 64 + 2) > 0


def _joined_bwd_case(seed=0):
    P, K, N = 300, 48, 24                                           # contraction K = the convolution's Cout, N = its Cin
    gr, w, _ = _pw_case(seed + 21, P, K, N)
    g = _gen(seed + 22)
    radd, jout = X.dyadic((P, N), g, zero_frac=0.05), X.dyadic((P, N), g, zero_frac=0.1)
    jy, jmean = X.dyadic((P, N), g), X.dyadic((1, N), g)
    rin, Sin = _pw_ref(gr, w)
    return gr, w, radd, jout, jy - jmean, X.joined_bwd_ref(rin, Sin, radd, jout), K


def test_f32_emulation_of_the_joined_backward_epilogue_meets_its_bounds():
    gr, w, radd, jout, fac, (ref, M), K = _joined_bwd_case()
    v = _pw_gemm32(gr, w) + radd.float()
    out = X.rne_bf16(torch.where(jout > 0, v, torch.zeros_like(v)).double())
    assert X.conv_excess(out, ref, M, K + 1) <= 0
    assert (jout <= 0).any() and (out[jout <= 0] == 0).all()
    chain, rows = X.pwfast_stats_chain(300, K, 24, bwd=True)
    slabs = _pw_slabs(out, fac, 32, rows)
    assert X.stats_excess(slabs.sum(0), torch.cat([out, out * fac], 1), chain) <= 0


def test_a_residual_added_behind_the_join_mask_fails():
    gr, w, radd, jout, fac, (ref, M), K = _joined_bwd_case(seed=1)
    v = _pw_gemm32(gr, w)
    out = X.rne_bf16((torch.where(jout > 0, v, torch.zeros_like(v)) + radd.float()).double())
    assert X.conv_excess(out, ref, M, K + 1) > 0


def test_a_dropout_keep_byte_of_the_neighbouring_channel_group_fails():
    """tss_pwconv_fwd_drop with p = 0.75: the reference applies the mask bytes as read back; a kernel that takes byte v + 1 for the 8-channel
    vector v keeps other channels"""
    P, K, N, dinv = 200, 48, 24, 4.0
    a, w, _ = _pw_case(31, P, K, N, zero_frac=0.0)
    mbytes = torch.randint(0, 256, (P, 16), generator=_gen(32)) & torch.randint(0, 256, (P, 16), generator=_gen(33))       # ~1/4 kept
    keep = lambda shift: torch.stack([(mbytes[:, (k // 8 + shift) % (K // 8)] >> (k % 8)) & 1 for k in range(K)], 1).double()
    ref, S = _pw_ref(a * keep(0), w)
    ok = X.rne_bf16((_pw_gemm32(a * keep(0), w) * dinv).double())
    assert X.conv_excess(ok, ref * dinv, S * dinv, K) <= 0
    bad = X.rne_bf16((_pw_gemm32(a * keep(1), w) * dinv).double())
    assert X.conv_excess(bad, ref * dinv, S * dinv, K) > 0


# ---------------------------------------------------------------------------------------------------------- dense 3x3 family and stem
# f32 emulation of csrc/wstat.hip, atrous.hip, conv3x3.hip, the 9-tap paths of convgemm.hip / wgrad.hip and csrc/stem.hip in their planners'
# order: operands a / g already rounded to bf16, every product exact, one f32 addition per 32-channel MFMA k-step and tap; statistics per
# block, wave and lane as the epilogues add them; the weight gradient stage by stage and split by split.  Defects go into the emulation.
@pytest.mark.parametrize('B,H,W,D', [(1, 7, 5, 1), (2, 11, 70, 3), (3, 20, 129, 18), (2, 19, 64, 18), (1, 6, 65, 6), (2, 7, 200, 6), (3, 100, 321, 7)])
def test_weight_stationary_walk_visits_every_row_once_and_its_ranges_partition_it(B, H, W, D):
    nstrip = X.cdiv(W, 64)
    nrows = B * nstrip * H
    seen = []
    for u in range(nrows):
        b, sx, r, j, nj = X.wstat_decode(u, H, W, D)
        assert 0 <= r < D and 0 <= j < nj and nj == len(range(r, H, D))
        seen.append((b, sx, r + j * D))
    assert sorted(seen) == [(b, sx, y) for b in range(B) for sx in range(nstrip) for y in range(H)]
    ranges = X.wstat_ranges(B, H, W)
    assert ranges[0][0] == 0 and ranges[-1][1] == nrows and all(p[1] == q[0] for p, q in zip(ranges, ranges[1:]))
    assert len(ranges) == min(nrows, 256) and max(hi - lo for lo, hi in ranges) == X.cdiv(nrows, len(ranges)) == X.wstat_plan(B, H, W, D)['rows']
    walked = []
    for lo, hi in ranges:                                          # the kernel's while loop walks exactly its range, row by row
        for b, sx, r, j0, j1 in X.wstat_segments(lo, hi, H, W, D):
            assert 0 <= j0 < j1
            walked += [(b, sx, r + j * D) for j in range(j0, j1)]
    assert walked == seen


def _dense_case(seed, B=2, C=64, N=16, H=9, W=70, Ho=None, Wo=None):
    g = _gen(seed)
    a = X.rne_bf16(X.dyadic((B, C, H, W), g, zero_frac=0.05))
    w = X.dyadic((N, C, 3, 3), g, emin=-6, emax=-2)
    gr = X.rne_bf16(X.dyadic((B, N, Ho or H, Wo or W), g))
    return a, w, gr


def _dense_fwd32(a, w, D, defect=None):
    """f32 sum over the nine taps and the 32-channel k-steps of each.  Defects, each at ONE pixel: 'ring' -- the ring slot of row y + D
    still holds row y - 2 D (refilled one row late); 'wrap' -- the left tap at x = 0 reads D pixels back in the flat row-major image, i.e.
    the end of the previous image row"""
    B, C, H, W = a.shape
    a32, w32 = a.float(), w.float()
    out = torch.zeros(B, w.shape[0], H, W)
    b, y = B - 1, 2 * D
    for ky in range(3):
        for kx in range(3):
            src = _dw_tap(a32, ky, kx, 1, D, H, W).clone()
            if defect == 'ring' and ky == 2:
                x = W // 2
                xs = x + (kx - 1) * D
                src[b, :, y, x] = a32[b, :, y - 2 * D, xs] if 0 <= xs < W else 0.0
            if defect == 'wrap' and kx == 0:
                yy = y + (ky - 1) * D
                if 0 < yy < H:
                    src[b, :, y, 0] = a32[b, :, yy - 1, W - D]
            for k0 in range(0, C, 32):
                out = out + torch.einsum('bchw,nc->bnhw', src[:, k0:k0 + 32], w32[:, k0:k0 + 32, ky, kx])
    return out


def _frag(p0, n, limit):
    """pixel indices of a 16-lane fragment starting at p0 (lanes past `limit` or past n lanes: -1)"""
    i = torch.arange(16) + p0
    return torch.where((torch.arange(16) < n) & (i < limit), i, torch.full_like(i, -1))


def _dense_blocks(kind, B, H, W, D=1):
    """[(slab row, [per f64-meeting wave group: [16-lane fragments in the order a lane adds them]])] of a launch over the [B][H][W] outputs"""
    P = B * H * W
    blocks = []
    if kind == 'wstat':
        for i, (lo, hi) in enumerate(X.wstat_ranges(B, H, W)):
            frags = []
            for b, sx, r, j0, j1 in X.wstat_segments(lo, hi, H, W, D):
                for j in range(j0, j1):
                    row0 = (b * H + r + j * D) * W
                    frags += [_frag(row0 + sx * 64 + m * 16, W - sx * 64 - m * 16, P) for m in range(4)]
            blocks.append((i, [frags]))
    elif kind in ('stream', 'stem'):
        ntiles = X.cdiv(P, 256)
        plan = X.stream_plan(P) if kind == 'stream' else X.stem_fwd_plan(P)
        for i in range(plan[2]):
            tiles = X.stream_tiles(i, P) if kind == 'stream' else list(range(i, ntiles, plan[2]))
            blocks.append((i, [[_frag(t * 256 + wv * 64 + m * 16, 16, P) for t in tiles for m in range(4)] for wv in range(4)]))
    else:
        tpr = X.cdiv(W, 64)
        ntiles, grid = B * H * tpr, X.lean3x3_plan(B, H, W)[2]
        for i in range(grid):
            groups = []
            for wm in range(2):
                frags = []
                for t in range(i, ntiles, grid):
                    by, tx = divmod(t, tpr)
                    x0 = tx * 64 + wm * 32
                    frags += [_frag(by * W + x0 + m * 16, W - x0 - m * 16, P) for m in range(2)]
                groups.append(frags)
            blocks.append((i, groups))
    return blocks


def _slabs_from_blocks(out_rows, fac_rows, blocks, stale=None):
    """slab rows of the launch: a lane adds its fragments' values in f32, 16 lanes meet in row16_sum's 4-level tree, the groups of a block
    and the rows meet in f64; rows no block owns are zeroed -- but `stale`, a row beyond the grid a defective kernel leaves as it was"""
    P, C = out_rows.shape
    terms = torch.zeros(P + 1, 2 * C)
    terms[:P] = torch.cat([out_rows.float(), out_rows.float() * fac_rows.float()], 1)
    slabs = torch.zeros(512, 2 * C, dtype=torch.float64)
    longest = 0
    for row, groups in blocks:
        for frags in groups:
            lanes = torch.zeros(16, 2 * C)
            longest = max(longest, len(frags))
            for f in frags:
                lanes = lanes + terms[f]                        # (index -1 is the zero row P)
            for half in (8, 4, 2, 1):
                lanes = lanes[:half] + lanes[half:2 * half]
            slabs[row] += lanes[0].double()
    if stale is not None:
        slabs[stale] = slabs[0] + 1.0
    return slabs, longest + 4


@pytest.mark.parametrize('kind,B,H,W,D,C', [('wstat', 2, 40, 130, 3, 32), ('wstat', 2, 9, 70, 1, 32), ('stream', 3, 11, 37, 2, 32), ('stream', 2, 257, 257, 1, 32),
                                            ('lean', 2, 3, 65, 1, 64), ('lean', 2, 130, 65, 2, 32)])
def test_f32_emulation_of_the_dense_3x3_layer_meets_the_bounds_in_each_planners_order(kind, B, H, W, D, C):
    N = 16 if H * W > 9000 else 48
    a, w, _ = _dense_case(B + H + W, B=B, C=C, N=N, H=H, W=W)
    ref, S = X.conv_ref(a, w, padding=D, dilation=D)
    out = X.rne_bf16(_dense_fwd32(a, w, D).double())
    assert X.conv_excess(out, ref, S, 9 * C) <= 0
    rows = X.nchw_to_rows(out)
    blocks = _dense_blocks(kind, B, H, W, D)
    slabs, chain = _slabs_from_blocks(rows, rows, blocks)
    want, owners = {'wstat': lambda: (X.wstat_plan(B, H, W, D)['chain'], range(X.wstat_plan(B, H, W, D)['grid'])),
                    'stream': lambda: X.stream_plan(B * H * W)[:2], 'lean': lambda: X.lean3x3_plan(B, H, W)[:2]}[kind]()
    assert chain == want and [r for r, _ in blocks if (slabs[r] != 0).any()] == list(owners)
    assert X.stats_excess(slabs.sum(0), torch.cat([rows, rows * rows], 1), chain) <= 0


@pytest.mark.parametrize('defect', ['ring', 'wrap'])
def test_one_wrong_input_row_or_column_at_one_pixel_of_the_dense_layer_fails(defect):
    D = 2
    a, w, _ = _dense_case(50, H=9, W=70)
    ref, S = X.conv_ref(a, w, padding=D, dilation=D)
    out = X.rne_bf16(_dense_fwd32(a, w, D, defect=defect).double())
    ex = X.conv_excess(out, ref, S, 9 * a.shape[1])
    print(defect, 'excess over the bound', ex)
    assert ex > 0
    good = X.rne_bf16(_dense_fwd32(a, w, D).double())
    assert (out != good).any((1,)).sum() == 1                       # one pixel


def test_a_statistics_row_of_a_block_beyond_the_grid_not_zeroed_fails():
    B, H, W, D = 2, 9, 70, 1
    a, w, _ = _dense_case(51, H=H, W=W)
    rows = X.nchw_to_rows(X.rne_bf16(_dense_fwd32(a, w, D).double()))
    blocks = _dense_blocks('wstat', B, H, W, D)
    assert len(blocks) == 36
    slabs, chain = _slabs_from_blocks(rows, rows, blocks, stale=36 + 3 * 36)      # a row the block-0 loop `rr += gridDim.x` must clear
    assert X.stats_excess(slabs.sum(0), torch.cat([rows, rows * rows], 1), chain) > 0


def _dense_wgrad32(a, gr, stride, D, mirror=False):
    """wgrad_kernel + its atomics (csrc/wgrad.hip): per tap and split, stages of 64 pixels in two 32-pixel k-steps, then one f32 addition
    per split onto dW [N][C][3][3]; mirror: the tap's result lands at the mirrored kx"""
    B, C, H, W = a.shape
    N, Ho, Wo = gr.shape[1:]
    P = B * Ho * Wo
    tiles = X.cdiv(N, 128) * X.cdiv(C, 128) * 9
    nstage = X.cdiv(P, 64)
    ns = max(1, min(max(1, 1024 // tiles), X.cdiv(nstage, 8)))
    per = X.cdiv(nstage, ns)
    gp = X.nchw_to_rows(gr).float()
    dw = torch.zeros(N, C, 3, 3)
    for ky in range(3):
        for kx in range(3):
            src = X.nchw_to_rows(_dw_tap(a.float(), ky, kx, stride, D, Ho, Wo)).float()
            for s in range(ns):
                acc = torch.zeros(N, C)
                for p0 in range(s * per * 64, min((s + 1) * per * 64, P), 32):
                    p1 = min(p0 + 32, P)
                    acc = acc + gp[p0:p1].t() @ src[p0:p1]
                dw[:, :, ky, 2 - kx if mirror else kx] += acc
    return dw


@pytest.mark.parametrize('stride,D', [(1, 1), (2, 3)])
def test_nine_tap_weight_gradient_meets_the_bound_and_a_mirrored_tap_fails(stride, D):
    B, C, N, H, W = 2, 40, 24, 33, 41
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    a, _, gr = _dense_case(60 + D, B=B, C=C, N=N, H=H, W=W, Ho=Ho, Wo=Wo)
    ref, S = X.conv_weight_ref(a, (N, C, 3, 3), gr, stride=stride, padding=D, dilation=D)
    chain = X.generic_wgrad_chain(B * Ho * Wo, C, N, 9)
    assert X.wgrad_excess(_dense_wgrad32(a, gr, stride, D).double(), ref, S, chain) <= 0
    assert X.wgrad_excess(_dense_wgrad32(a, gr, stride, D, mirror=True).double(), ref, S, chain) > 0


def test_dyadic_transforms_are_exact_in_f32_in_the_dense_kernels_orders():
    """the kadd folds of conv3x3_lean_kernel (forward: x k0 + (c2 - c1 c0); backward: (e k0 + kadd) + y k1, kadd = -(c0 c2) - c1 c3),
    wgrad_kernel (x cs + (cb - cm cs); ca e + (cb y + cc)), stem_wgrad_mfma_kernel (the same), im2col3x3_kernel ((x - mu) sc + be) and
    the masks' (x - mean) scale + bias > 0, with ReLU alone (no scale) as the identity transform"""
    g = _gen(12)
    n = 1 << 18
    f = lambda t: t.float()
    x, mean, bias, scale = X.dyadic((n,), g), X.dyadic((n,), g), X.dyadic((n,), g), X.pow2((n,), g, 0.5, 4)
    ref = (x - mean) * scale + bias
    for got in (f(x) * f(scale) + (f(bias) - f(mean) * f(scale)), (f(x) - f(mean)) * f(scale) + f(bias)):
        assert torch.equal(got.double(), ref)
    assert torch.equal((f(x) * 1.0 + (0.0 - 0.0 * 1.0)).double(), x)
    e, y, gce, gmu = X.dyadic((n,), g), X.dyadic((n,), g), X.dyadic((n,), g), X.dyadic((n,), g)
    ga, gb = X.pow2((n,), g, 0.25, 2), X.pow2((n,), g, 2.0 ** -6, 2.0 ** -3)
    ref = ga * (e - gce) + gb * (y - gmu)
    kadd = -(f(ga) * f(gce)) - f(gb) * f(gmu)
    for got in ((f(e) * f(ga) + kadd) + f(y) * f(gb), f(ga) * f(e) + (f(gb) * f(y) + kadd), f(ga) * (f(e) - f(gce)) + f(gb) * (f(y) - f(gmu))):
        assert torch.equal(got.double(), ref)
    # the 24-bit stem image is exact in f32 and its bf16 rounding moves it
    v = X.full_f32((4096,), g)
    assert (X.rne_bf16(v) != v).float().mean() > 0.9


def _stem_patches(x, stride, window, defect=False):
    """[P][Cin 9] taps of every output pixel as stem_taps picks them (X.stem_tap_columns); defect: the right-edge tap at ix == Win is not
    masked and reads the clamped element"""
    B, Cin, Hin, Win = x.shape
    Ho, Wo = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    out = torch.zeros(B, Ho, Wo, Cin, 3, 3, dtype=x.dtype)
    for ox in range(Wo):
        cols = X.stem_tap_columns(ox, Win, stride, window)
        for kx, col in enumerate(cols):
            if col is None and defect and ox * stride + kx - 1 == Win:
                col = Win - 1
            if col is None:
                continue
            for oy in range(Ho):
                for ky in range(3):
                    iy = oy * stride + ky - 1
                    if 0 <= iy < Hin:
                        out[:, oy, ox, :, ky, kx] = x[:, :, iy, col]
    return out.reshape(B * Ho * Wo, Cin * 9)


@pytest.mark.parametrize('stride', [2, 1])
def test_stem_window_arithmetic_picks_the_padded_taps_at_every_width(stride):
    for Win in range(1, 10):
        x = X.dyadic((2, 3, 4, Win), _gen(Win))
        want = torch.nn.functional.unfold(x, 3, padding=1, stride=stride).permute(0, 2, 1).reshape(-1, 27)
        for window in ([False, True] if (stride == 2 and Win >= 4) else [False]):
            assert torch.equal(_stem_patches(x, stride, window), want), (Win, stride, window)


def test_f32_emulation_of_the_stem_meets_the_bounds_and_an_unmasked_right_edge_tap_fails():
    B, Hin, Win, N = 2, 9, 35, 32                                   # odd width: the last output column's right tap is at ix == Win
    g = _gen(70)
    x = X.full_f32((B, 3, Hin, Win), g)
    xb = X.rne_bf16(x)                                              # the MFMA forms pack the taps as bf16
    w = X.dyadic((N, 3, 3, 3), g, emin=-6, emax=-2)
    ref, S = X.conv_ref(xb, w, stride=2, padding=1)
    P = ref.numel() // N
    for defect in (False, True):
        pt = _stem_patches(xb, 2, True, defect=defect).float()
        out = X.rne_bf16((pt @ w.reshape(N, 27).float().t()).double())
        ex = X.conv_excess(out, X.nchw_to_rows(ref), X.nchw_to_rows(S), 27)
        assert (ex > 0) == defect, (defect, ex)
    # statistics and weight gradient in the planners' order (stem_fwd_plan / stem_wgrad_plan: one tile per block here, 360 pixels = 2 tiles)
    Ho, Wo = ref.shape[2:]
    slabs, chain = _slabs_from_blocks(out, out, _dense_blocks('stem', 1, 1, P))
    assert chain == X.stem_fwd_plan(P)[0] and X.stats_excess(slabs.sum(0), torch.cat([out, out * out], 1), chain) <= 0
    gr = X.rne_bf16(X.dyadic((B, N, Ho, Wo), g))
    rw, Sw = X.conv_weight_ref(xb, (N, 3, 3, 3), gr, stride=2, padding=1)
    pt, gp = _stem_patches(xb, 2, True).float(), X.nchw_to_rows(gr).float()
    chain_w, rows = X.stem_wgrad_plan(P, True)
    ws = []
    for i in range(rows):
        waves = [torch.zeros(N, 27) for _ in range(4)]
        for t in range(i, X.cdiv(P, 256), rows):
            for wv in range(4):
                for p0 in range(t * 256 + wv * 64, min(t * 256 + wv * 64 + 64, P), 32):
                    p1 = min(p0 + 32, P)
                    waves[wv] = waves[wv] + gp[p0:p1].t() @ pt[p0:p1]
        ws.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    groups = [torch.zeros(N, 27) for _ in range(16)]
    for r, part in enumerate(ws):
        groups[r % 16] = groups[r % 16] + part
    tot = torch.zeros(N, 27)
    for gsum in groups:
        tot = tot + gsum
    dw = torch.zeros(N, 27) + tot
    assert X.wgrad_excess(dw.double().reshape(rw.shape), rw, Sw, chain_w) <= 0
    # the VALU form keeps the f32 image: unrounded reference, every product a rounding, 256 pixels per lane and tile
    rwf, Swf = X.conv_weight_ref(x, (N, 3, 3, 3), gr, stride=2, padding=1)
    ptf = _stem_patches(x, 2, True).float()
    acc = torch.zeros(N, 27)
    for p in range(P):
        acc = acc + gp[p].unsqueeze(1) * ptf[p].unsqueeze(0)
    chain_v, _ = X.stem_wgrad_plan(512, False)                      # one lane's chain over two tiles, as this single accumulator adds them
    assert X.wgrad_excess(acc.double().reshape(rwf.shape), rwf, Swf, chain_v) <= 0


# ---------------------------------------------------------------------------------------------------------- resample, pyramid, gate
# the restated planners and f32 emulations behind tests/test_gpu_resample_exact.py (csrc/resample.hip, gate.hip)
NAN = float('nan')


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _blend32(x, Ho, Wo, order=0, clamp=True, fused=True):
    """bilinear_nhwc_fwd_kernel / planar_bilinear in f32: rows of columns (order 0, the kernels') or columns of rows (order 1: the head's
    fast kernel blends vertically first).  clamp=False: i1 = i0 + 1 behind the last source row, where the harness keeps NaN"""
    B, C, H, W = x.shape
    y0, y1, ly0, ly1 = X.ac_taps_np(H, Ho, fused)
    x0, x1, lx0, lx1 = X.ac_taps_np(W, Wo, fused)
    xf = x.float()
    if not clamp:
        xf, y1 = torch.cat([xf, torch.full((B, C, 1, W), NAN)], 2), y0 + 1
    ly0, ly1, lx0, lx1 = _T(ly0)[:, None], _T(ly1)[:, None], _T(lx0)[None, :], _T(lx1)[None, :]
    v = lambda iy, ix: xf[:, :, _T(iy)][:, :, :, _T(ix)]
    if order == 0:
        return ly0 * (lx0 * v(y0, x0) + lx1 * v(y0, x1)) + ly1 * (lx0 * v(y1, x0) + lx1 * v(y1, x1))
    return lx0 * (ly0 * v(y0, x0) + ly1 * v(y1, x0)) + lx1 * (ly0 * v(y0, x1) + ly1 * v(y1, x1))


def _gather32(g, n_in, axis, reverse=False, short=0, fused=True):
    """one pass of a two-pass backward in f32: out[.., i, ..] = the window's weighted sum along `axis` (2 or 3) in window order (or
    reversed), weight 0 skipped as the kernels do.  short: ac_window's hi one short"""
    n_out = g.shape[axis]
    M = X.tap_matrix_f32(n_in, n_out, fused=fused).float()
    lo, hi = X.ac_windows_np(n_in, n_out)
    gf = g.float().movedim(axis, 0)
    out = torch.zeros((n_in,) + tuple(gf.shape[1:]))
    for i in range(n_in):
        idx = list(range(int(lo[i]), int(hi[i]) + 1 - short))
        for o in (reversed(idx) if reverse else idx):
            if M[o, i] != 0:
                out[i] = out[i] + M[o, i] * gf[o]
    return out.movedim(0, axis)


def _as_dtype(v, bf16):
    return v.bfloat16().double() if bf16 else v.double()


def test_exact_resize_pairs_have_exact_taps_and_contain_the_dyadic_ones():
    exact = 0
    for n_in in range(1, 41):
        for n_out in range(1, 200):
            k = X.exact_resize(n_in, n_out)
            assert k is not None or not X.dyadic_resize(n_in, n_out)
            if k is not None:
                exact += 1
                M = X.tap_matrix_f32(n_in, n_out)
                assert torch.equal(M, X.bilinear_matrix(n_in, n_out)), (n_in, n_out)
                assert torch.equal(torch.round(M * 2 ** k), M * 2 ** k)
    assert exact > 300 and X.exact_resize(6, 17) == 4 and not X.dyadic_resize(6, 17) and X.exact_resize(13, 32) is None
    for n_in, n_out in ((13, 50), (17, 6), (1, 12), (5, 1), (6, 17)):      # the vectorised taps are ac_taps_f32's
        i0, i1, l0, l1 = X.ac_taps_np(n_in, n_out, fused=False)
        fz = X.ac_taps_np(n_in, n_out)
        assert (i0 == fz[0]).all() and np.abs(l1 - fz[3]).max() <= X.U32 * (n_in - 1)
        for d, t in enumerate(X.ac_taps_f32(n_in, n_out)):
            assert (int(i0[d]), int(i1[d]), float(l0[d]), float(l1[d])) == (t[0], t[1], float(t[2]), float(t[3]))


def test_restated_windows_hold_every_tap_and_one_short_does_not():
    taps = 0
    for n_in in range(1, 41):
        for n_out in range(1, 200):
            assert X.window_misses(n_in, n_out) == 0, (n_in, n_out)
            taps += n_out
    assert taps == 40 * 199 * 100
    for Hi, Wi, Ho, Wo, _, _ in X.RS_BILINEAR:
        assert X.window_misses(Hi, Ho, 1) > 0 and X.window_misses(Wi, Wo, 1) > 0


def test_head_dispatch_keeps_every_lane_within_the_columns_of_its_instance():
    count = {'three': 0, 'four': 0, 'generic': 0}
    for w in range(1, 70):
        for W in range(8, 1097, 8):
            inst = X.head_instance(w, W, 24, 19)
            count[inst] += 1
            assert inst == 'generic' or X.head_columns_hold(w, W, 3 if inst == 'three' else 4), (w, W, inst)
    assert min(count.values()) > 900
    for w, W, inst in X.RS_HEAD:
        assert X.head_instance(w, W, 24, 19) == X.head_instance(w, W, 8, 8) == inst
        assert X.head_instance(w, W, 5, 5) == X.head_instance(w, W, 24, 19, aligned=False) == 'generic'
    # which of the chosen pairs READ the fourth column: only 6 -> 24; at 5 -> 16 the last-column clamp keeps the lanes within three
    assert [p[:2] for p in X.RS_HEAD if not X.head_columns_hold(p[0], p[1], 3) and p[2] != 'generic'] == [(6, 24)]


def test_pool_windows_slices_and_gate_walks_partition_what_they_cover():
    F = torch.nn.functional
    g = _gen(5)
    for H, W, bins in ((13, 21, 1), (13, 21, 2), (13, 21, 3), (13, 21, 6), (4, 5, 6), (3, 4, 2), (17, 33, 6), (9, 9, 8)):
        x = X.dyadic((2, 3, H, W), g)
        sums, _, n = X.pool_ref(x, bins)
        assert torch.allclose(sums / n, F.adaptive_avg_pool2d(x, bins), rtol=1e-14, atol=0)
        for y0, y1 in X.pool_windows(H, bins):
            assert y1 > y0
            for S in (1, 2, 21, 27, 256):
                sl = X.ppm_slice_rows(y0, y1, S)
                assert sl[0][0] == y0 and sl[-1][1] == y1 and all(a[1] == b[0] for a, b in zip(sl, sl[1:])) and all(b >= a for a, b in sl)
    assert [X.ppm_pool_slices(*a) for a in ((1, 50), (1, 1), (3, 13), (2, 50), (3, 50), (0, 5))] == [21, 256, 27, 11, 1, 1]
    for B in (1, 2, 3, 64, 2000):
        for HW in (1, 35, 64, 65, 130, 200, 4096, 70000):
            S = X.gate_slices(B, HW)
            walk = X.gate_slice_walk(HW, S)
            assert 1 <= S <= max(1, X.cdiv(HW, 64)) and walk[0][0] == 0 and walk[-1][1] == HW
            assert all(a[1] == b[0] for a, b in zip(walk, walk[1:])) and all(b >= a for a, b in walk)
    assert [X.gate_slices(B, HW) for B, HW, _, _ in X.RS_GATE] == [s for _, _, _, s in X.RS_GATE]


@pytest.mark.parametrize('bf16', [True, False])
@pytest.mark.parametrize('Hi,Wi,Ho,Wo,C,tier', X.RS_BILINEAR)
def test_f32_emulation_of_the_bilinear_forward_meets_its_tier(Hi, Wi, Ho, Wo, C, tier, bf16):
    x = X.bilinear_fwd_operand(Hi, Wi, Ho, Wo, C)
    ref, S = X.resize_ref(x, Ho, Wo)
    assert X.resize_tier1(x, S, [(Hi, Ho), (Wi, Wo)]) == (tier == 1)
    a, b, c = _blend32(x, Ho, Wo, 0), _blend32(x, Ho, Wo, 1), _blend32(x, Ho, Wo, 0, fused=False)
    if tier == 1:       # the budget: two orders, contracted or not, the same bits, the exact value's
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(_as_dtype(a, bf16), X.out_bits_ref(ref, bf16))
    else:
        for out in (a, b, c):
            assert X.resample_excess(_as_dtype(out, bf16), ref, S, X.BLEND_N, bf16, X.tap_slack(x, Ho, Wo)) <= 0
            assert X.resize_matrix_excess(_as_dtype(out, bf16), x, Ho, Wo, bf16) <= 0
    if Ho > 1 or Hi == 1:       # (a single output row reads source rows 0 and 1 only)
        bad = _as_dtype(_blend32(x, Ho, Wo, 0, clamp=False), bf16)         # defect: i1 not clamped at the last source index
        assert not X.resample_excess(bad, ref, S, X.BLEND_N, bf16, X.tap_slack(x, Ho, Wo)) <= 0


@pytest.mark.parametrize('bf16', [True, False])
@pytest.mark.parametrize('Hi,Wi,Ho,Wo,C,tier', X.RS_BILINEAR)
def test_f32_emulation_of_the_two_pass_backward_meets_its_tier(Hi, Wi, Ho, Wo, C, tier, bf16):
    dy = X.bilinear_bwd_operand(Hi, Wi, Ho, Wo, C, tier)
    t, ta, ref, S = X.resize_bwd_ref(dy, Hi, Wi)
    assert (X.resize_tier1(dy, S, [(Hi, Ho), (Wi, Wo)]) and X.resize_tier1(dy, ta, [(Hi, Ho)])) == (tier == 1)
    ny = X.window_len(Hi, Ho) + 1
    nx = ny + X.window_len(Wi, Wo) + 1
    tmp = _gather32(dy, Hi, 2)
    dx = _gather32(tmp.double(), Wi, 3)
    rev = _gather32(_gather32(dy, Hi, 2, reverse=True, fused=False).double(), Wi, 3, reverse=True, fused=False)
    if tier == 1:
        assert torch.equal(tmp.double(), t) and torch.equal(dx, rev) and torch.equal(_as_dtype(dx, bf16), X.out_bits_ref(ref, bf16))
    else:
        assert X.resample_excess(tmp.double(), t, ta, ny, False, X.tap_slack_bwd(dy, Hi)) <= 0
        for out in (dx, rev):
            assert X.resample_excess(_as_dtype(out, bf16), ref, S, nx, bf16, X.tap_slack_bwd(dy, Hi, Wi)) <= 0
            assert X.resize_bwd_matrix_excess(_as_dtype(out, bf16), dy, Hi, Wi, nx, bf16) <= 0
    bad = _gather32(_gather32(dy, Hi, 2, short=1).double(), Wi, 3, short=1)       # defect: ac_window's hi one short
    assert X.resample_excess(_as_dtype(bad, bf16), ref, S, nx, bf16, X.tap_slack_bwd(dy, Hi, Wi)) > 0


def _head32(low, H, W, ncols):
    """upsample_head_fwd_kernel<T, ncols> in f32: the vertical blend of source columns c0 .. c0 + ncols - 1 first, then per output the
    two columns picked by d = i - c0 (d >= ncols - 1 picks the last one)"""
    B, N, h, w = low.shape
    y0, y1, ly0, ly1 = X.ac_taps_np(h, H)
    x0, x1, lx0, lx1 = X.ac_taps_np(w, W)
    lf = low.float()
    rows = _T(ly0)[:, None] * lf[:, :, _T(y0)] + _T(ly1)[:, None] * lf[:, :, _T(y1)]          # [B][N][H][w]
    c0 = np.repeat(x0.reshape(-1, 8)[:, :1], 8, 1).reshape(-1)
    pick = lambda i: _T(np.minimum(c0 + np.minimum(i - c0, ncols - 1), w - 1))
    return _T(lx0) * rows[..., pick(x0)] + _T(lx1) * rows[..., pick(x1)]


@pytest.mark.parametrize('bf16', [True, False])
@pytest.mark.parametrize('w,W,inst', X.RS_HEAD)
def test_f32_emulation_of_the_head_meets_the_bound_and_three_columns_where_four_are_read_fail(w, W, inst, bf16):
    low = X.dyadic((2, 19, 6, w), X.case_gen(4, w, W, 19), zero_frac=0.03)
    ref, S = X.resize_ref(low, 14, W)
    ncols = {'three': 3, 'four': 4, 'generic': 8}[inst]
    out = _as_dtype(_head32(low, 14, W, ncols), bf16)
    slack = X.tap_slack(low, 14, W)
    assert X.resample_excess(out, ref, S, X.BLEND_N, bf16, slack) <= 0 and X.resize_matrix_excess(out, low, 14, W, bf16) <= 0
    if (w, W) == (6, 24):       # defect: the 3-column selection on a pair that reads the fourth
        assert X.resample_excess(_as_dtype(_head32(low, 14, W, 3), bf16), ref, S, X.BLEND_N, bf16, slack) > 0
    if (w, W) == (5, 16):       # ... which 5 -> 16 does not: three columns are enough there
        assert torch.equal(_head32(low, 14, W, 3), _head32(low, 14, W, 4))


def _pool32(x, bins, chunk=None, drop_last=False):
    """f32 window sums in pixel order, or as partial sums of `chunk` pixels added afterwards (the lanes of a block)"""
    out = torch.zeros(x.shape[0], x.shape[1], bins, bins)
    for i, (y0, y1) in enumerate(X.pool_windows(x.shape[2], bins)):
        y1 = y1 - 1 if drop_last and y1 - y0 > 1 else y1
        for j, (x0, x1) in enumerate(X.pool_windows(x.shape[3], bins)):
            px = x[:, :, y0:y1, x0:x1].float().reshape(x.shape[0], x.shape[1], -1)
            parts = [px] if chunk is None else list(px.split(chunk, 2))
            tot = torch.zeros(px.shape[:2])
            for p in parts:
                s = torch.zeros(px.shape[:2])
                for k in range(p.shape[2]):
                    s = s + p[:, :, k]
                tot = tot + s
            out[:, :, i, j] = tot
    return out


@pytest.mark.parametrize('bf16', [True, False])
@pytest.mark.parametrize('H,W,C,bins', X.RS_POOL)
def test_f32_emulation_of_the_pools_meets_the_bounds_and_a_dropped_row_or_a_slice_count_fails(H, W, C, bins, bf16):
    x = X.dyadic((2, C, H, W), X.case_gen(6, H, W, C, bins), zero_frac=0.03)
    sums, sabs, n = X.pool_ref(x, bins)
    assert X.exact_budget(sabs, X.lsb_exp(x))
    a, b = _pool32(x, bins), _pool32(x, bins, chunk=7)
    assert torch.equal(a, b) and torch.equal(a.double(), sums)            # the budget: exact whatever the order
    out = _as_dtype(a / n.float(), bf16)
    assert X.pool_fwd_excess(out, sums, n, bf16) <= 0
    if H > bins:
        assert X.pool_fwd_excess(_as_dtype(_pool32(x, bins, drop_last=True) / n.float(), bf16), sums, n, bf16) > 0      # defect: a dropped row
        rows = torch.tensor([float(y1 - y0) for y0, y1 in X.pool_windows(H, bins)])[:, None]
        sliced = a / (n.float() / rows * (rows - 1).clamp_min(1))          # defect: divided by the pixels of a slice one row short
        assert X.pool_fwd_excess(_as_dtype(sliced, bf16), sums, n, bf16) > 0
    # backward: every pixel adds v * fl(1 / n) per window that holds it
    dy = X.dyadic((2, C, bins, bins), X.case_gen(7, H, W, C, bins), zero_frac=0.03)
    ref, S, chain = X.pool_bwd_ref([dy], H, W, [bins])
    dx = torch.zeros(2, C, H, W)
    for i, (y0, y1) in enumerate(X.pool_windows(H, bins)):
        for j, (x0, x1) in enumerate(X.pool_windows(W, bins)):
            inv = torch.tensor(1.0) / torch.tensor(float((y1 - y0) * (x1 - x0)))
            dx[:, :, y0:y1, x0:x1] = dx[:, :, y0:y1, x0:x1] + (dy[:, :, i, j].float() * inv)[:, :, None, None]
    assert X.resample_excess(_as_dtype(dx, bf16), ref, S, chain, bf16) <= 0


@pytest.mark.parametrize('bf16', [True, False])
@pytest.mark.parametrize('H,W,tier', [(17, 33, 1), (12, 20, 2)])
def test_f32_emulation_of_the_concat_meets_its_tier_and_its_defects_fail(H, W, tier, bf16):
    B, C, ca = 2, 8, 8
    g = X.case_gen(10, H, W, C, ca)
    A = X.ArmOperands(g, B, ca, tier, bf16)
    taken = {'late': 0, 'mask': 0}
    for k, bins in enumerate(A.binss):
        ref, S = X.resize_ref(A.act[k], H, W)
        t1 = X.resize_tier1(A.act[k], S, [(bins, H), (bins, W)])
        assert t1 == (tier == 1 or bins == 1)
        a, b = _blend32(A.act[k], H, W, 0), _blend32(A.act[k], H, W, 1)
        if t1:
            assert torch.equal(a, b) and torch.equal(_as_dtype(a, bf16), X.out_bits_ref(ref, bf16))
        else:
            assert X.resample_excess(_as_dtype(a, bf16), ref, S, X.BLEND_N, bf16, X.tap_slack(A.act[k], H, W)) <= 0
    # defect: BatchNorm + ReLU applied after the blend instead of per tap (linked ReLU arms with more than one bin)
    D = X.ArmOperands(X.case_gen(10, H, W, C, ca, 1), B, ca, tier, bf16, binss=(3, 6), link=(True, True), relu=(1, 1))
    for k in range(2):
        ref, S = X.resize_ref(D.act[k], H, W)
        mean, scale, beta = D.links[k]
        late = (_blend32(D.raw[k], H, W, 0).double() - mean) * scale + beta
        assert X.resample_excess(_as_dtype(late.clamp_min(0).float(), bf16), ref, S, X.BLEND_N, bf16, X.tap_slack(D.act[k], H, W)) > 0
        taken['late'] += 1
    # backward on the GPU file's operands: the gather, the mask act > 0, the slab rows
    g = X.case_gen(11, B, H, W, C, ca)
    A = X.ArmOperands(g, B, ca, tier, bf16)
    Ct = C + 4 * ca
    dout = X.narrow((B, Ct, H, W), g, 0.03) if tier == 1 else X.dyadic((B, Ct, H, W), g, zero_frac=0.03)
    for k, bins in enumerate(A.binss):
        gk = dout[:, C + k * ca:C + (k + 1) * ca]
        _, _, ref, S = X.resize_bwd_ref(gk, bins, bins)
        keep = (A.pre[k] > 0).double() if A.relu[k] else torch.ones_like(ref)
        n = X.concat_gather_chain(bins, H, W, ca)
        raw = _gather32(_gather32(gk, bins, 2).double(), bins, 3)
        rev = _gather32(_gather32(gk, bins, 3, reverse=True).double(), bins, 2, reverse=True)
        t1 = X.resize_tier1(gk, S, [(bins, H), (bins, W)])
        assert t1 == (tier == 1 or bins == 1)
        for out in (raw, rev):
            e = _as_dtype(out * keep.float(), bf16)
            if t1:
                assert torch.equal(e, X.out_bits_ref(ref * keep, bf16))
            else:
                assert X.resample_excess(e, ref * keep, S * keep, n, bf16, X.tap_slack_bwd(gk, bins, bins) * keep) <= 0
        if A.relu[k] and bool(((A.pre[k] == 0) & (ref != 0)).any()):          # defect: the ReLU mask taken on >= 0
            loose = _as_dtype(raw * (A.pre[k] >= 0).float(), bf16)
            assert X.resample_excess(loose, ref * keep, S * keep, n, bf16, X.tap_slack_bwd(gk, bins, bins) * keep) > 0
            taken['mask'] += 1
        rows, er, xc = B * bins * bins, X.nchw_to_rows(e), X.nchw_to_rows(A.xc[k])
        slab = torch.zeros(X.STAT_SLABS, 2 * ca, dtype=torch.float64)
        slab[:rows] = torch.cat([er, er * xc], 1)
        assert X.concat_slab_faults(slab, er, xc, rows) == []
        slab[rows + 3, 1] = NAN                                                # defect: a slab row beyond rows_used left stale
        assert X.concat_slab_faults(slab, er, xc, rows) == ['a slab row neither written nor zeroed', 'a slab row beyond B bins^2 holds a value']
    assert taken['late'] > 0 and taken['mask'] > 0, ('a defect branch was never taken', taken)


@pytest.mark.parametrize('bf16', [True, False])
@pytest.mark.parametrize('add_one', [0.0, 1.0])
@pytest.mark.parametrize('B,HW,C,S', X.RS_GATE)
def test_f32_emulation_of_the_gates_meets_the_bounds(B, HW, C, S, add_one, bf16):
    g = X.case_gen(14, B, HW, C)
    x = X.dyadic((B, HW, C), g, zero_frac=0.03)
    a = X.dyadic((B, 1, C), g, zero_frac=0.25)
    gr = X.dyadic((B, HW, C), g, zero_frac=0.03)
    # sigm() with exp2 of the f32 product as __expf forms it (the host's exp2f stands in for V_EXP_F32: both within 1 ulp)
    sg = 1.0 / (1.0 + torch.exp2(torch.tensor(1.4426950408889634).float() * -a.float()))
    assert bool((sg[a == 0] == 0.5).all())
    out = _as_dtype(gr.float() * (sg + add_one), bf16)
    ref, bound = X.gate_fwd_bound(gr, a.expand_as(gr), add_one, bf16)
    assert ((out - ref).abs() - bound).max() <= 0
    z = (a == 0).expand_as(gr)
    assert torch.equal(out[z], X.out_bits_ref(ref[z], bf16))
    wrong = _as_dtype(gr.float() * (sg * (1 + 2.0 ** -18) + add_one), bf16)          # a sigmoid 64 ulp off fails in f32, and at a == 0
    assert bf16 or ((wrong - ref).abs() - bound).max() > 0
    # da: the slice walk in f32 (lanes, then slices), times s (1 - s)
    prod = (gr * x).float()
    NPL = 256 // (C // 8)
    t = torch.zeros(B, C)
    for q0, q1 in X.gate_slice_walk(HW, S):
        lanes = torch.zeros(B, NPL, C)
        for q in range(q0, q1):
            lanes[:, (q - q0) % NPL] = lanes[:, (q - q0) % NPL] + prod[:, q]
        sl = torch.zeros(B, C)
        for r in range(NPL):
            sl = sl + lanes[:, r]
        t = t + sl
    s1 = sg.reshape(B, C)
    da = _as_dtype(t * s1 * (1 - s1), bf16)
    p64 = gr * x
    ref, bound = X.gate_da_bound(p64.sum(1), p64.abs().sum(1), a.reshape(B, C), X.gate_chain(HW, S, C), bf16)
    assert ((da - ref).abs() - bound).max() <= 0
    short = _as_dtype((t - prod[:, HW - 1]) * s1 * (1 - s1), bf16)          # defect: the ragged last slice one pixel short
    assert ((short - ref).abs() - bound).max() > 0


def _arms_finalize32(yq, gamma, rmean, rvar, biased=False):
    """the statistics of ppm_arms_fwd_kernel in its order: f32 lane sums over the 64-pixel tiles, row16_sum's four rotations, the four
    waves in f64, the finalize in f64 and its f32 stores; the running statistics in f32"""
    P, Ca = yq.shape
    y = torch.zeros(X.cdiv(P, 64) * 64, Ca)
    y[:P] = yq.float()
    s1, s2 = torch.zeros(64, Ca), torch.zeros(64, Ca)
    for t in y.split(64):
        s1, s2 = s1 + t, s2 + t * t
    tot = []
    for v in (s1, s2):
        v = v.reshape(4, 16, Ca)
        for r in (8, 4, 2, 1):
            v = v + torch.roll(v, -r, 1)
        tot.append(v[:, 0].double().sum(0))
    mean = tot[0] / P
    var = (tot[1] / P - mean * mean).clamp_min(0.0)
    inv = ((var + X.ARMS_EPS) ** -0.5).float()
    m, mom = mean.float(), torch.tensor(X.ARMS_MOMENTUM).float()
    unb = (var if biased or P == 1 else var * P / (P - 1.0)).float()
    return dict(mean=m, invstd=inv, scale=gamma.float() * inv, rmean=(1 - mom) * rmean.float() + mom * m,
                rvar=(1 - mom) * rvar.float() + mom * unb)


@pytest.mark.parametrize('C,Ca,Ps,training', X.RS_ARMS)
def test_f32_emulation_of_the_arms_finalize_meets_its_bounds_and_a_biased_running_variance_fails(C, Ca, Ps, training):
    for o in X.arms_operands(C, Ca, Ps):
        ref, S = o['x'] @ o['w'].T, o['x'].abs() @ o['w'].abs().T
        yq = (o['x'].float() @ o['w'].float().T).bfloat16().double()          # an f32 GEMM in the host's order, rounded once
        assert X.conv_excess(yq, ref, S, C) <= 0
        want = X.arms_vec_ref(yq, o['gamma'], o['rmean'], o['rvar'])
        got = _arms_finalize32(yq, o['gamma'], o['rmean'], o['rvar'])
        for name, (r, b) in want.items():
            assert ((got[name].double() - r).abs() - b).max() <= 0, (name, o['P'])
        if o['P'] == 1:
            assert bool((got['invstd'] == torch.tensor(X.ARMS_EPS ** -0.5).float()).all())       # count = 1: the variance is an exact 0
        elif o['P'] <= 130:
            bad = _arms_finalize32(yq, o['gamma'], o['rmean'], o['rvar'], biased=True)
            r, b = want['rvar']
            assert ((bad['rvar'].double() - r).abs() - b).max() > 0


def _arms_bwd32(o, R, training, accumulate, mirror=False):
    """ppm_arms_bwd_kernel from its staging on, in f32: g by line 293 with the f32 coefficients, rounded to bf16; e_in as one k-step
    per output (the f64 sum of the exact products rounded once); dw as ceil(P / 32) k-steps of 32 pixels, each an f64 sum rounded once
    and added in f32, then onto the prior.  mirror: the channel vector cv of the transposed store written to rows of nvg - 1 - cv"""
    P, Ca = o['e'].shape
    ga, gb, gce = (R[k][0].float() for k in ('ga', 'gb', 'gce'))
    g = (ga * (o['e'].float() - gce) + gb * (o['y'].float() - o['mean'].float())).bfloat16().double()
    e_in = (g @ o['w']).float().bfloat16().double()
    gt = g.reshape(P, Ca // 8, 8).flip(1).reshape(P, Ca) if mirror else g
    dw = torch.zeros(Ca, o['x'].shape[1])
    for p0 in range(0, P, 32):
        dw = dw + (gt[p0:p0 + 32].T @ o['x'][p0:p0 + 32]).float()
    dw = (o['dw0'].float() if accumulate else 0.0) + dw
    return g, e_in, dw.double()


@pytest.mark.parametrize('C,Ca,Ps,training,accumulate', X.RS_ARMS_BWD)
def test_f32_emulation_of_the_arms_backward_meets_tier_3_and_a_mirrored_channel_vector_fails(C, Ca, Ps, training, accumulate):
    for o in X.arms_bwd_operands(C, Ca, Ps, training, accumulate):
        R = X.arms_bwd_ref(o, training, accumulate)
        near = R['near']
        assert float(near.double().mean()) <= X.NEAR_TIE_CAP                    # the cap, from the reference alone
        g, e_in, dw = _arms_bwd32(o, R, training, accumulate)
        # the premise of tier 3: away from a tie the f32 chain rounds as the reference does; near one it is at most one ulp off
        _, ulp, _ = X.bf16_of_f64(R['gq'])
        assert torch.equal(g[~near], R['gq'][~near]) and bool(((g - R['gq']).abs() <= ulp)[near].all())
        assert training or not bool(near.any())
        for name, out in (('e_in', e_in), ('dw', dw)):
            ref, bound = R[name]
            assert ((out - ref).abs() - bound).max() <= 0, (name, o['P'])
        # dgamma / dbeta: f64 sums in another order (per-thread partials of 8 pixels, then the partials), stored as the kernel stores
        xc = o['y'] - o['mean']
        for name, terms, scale, prior in (('dgamma', o['e'] * xc, o['invstd'], o['dgamma0']), ('dbeta', o['e'], 1.0, o['dbeta0'])):
            part = torch.stack([t.flip(0).sum(0) for t in terms.split(8)]).sum(0)
            out = (scale * part).float()
            out = (prior.float() + out) if accumulate else out
            ref, bound = R[name]
            assert ((out.double() - ref).abs() - bound).max() <= 0, name
        _, _, bad = _arms_bwd32(o, R, training, accumulate, mirror=True)          # defect: a mirrored cv in the transposed store
        ref, bound = R['dw']
        assert ((bad - ref).abs() - bound).max() > 0


# ---------------------------------------------------------------------------------------------------------- eval bottleneck, affines, joins
def test_bneck_route_and_lds_reach_every_tile_form_of_the_case_tables():
    lds = X.bneck_lds
    assert 140 * 1024 < lds(1, 8, 16, 64, 64) <= X.BK_LDS                     # about 144 KB
    assert lds(1, 8, 16, 96, 96) > X.BK_LDS and lds(1, 8, 16, 128, 128) > X.BK_LDS
    assert lds(1, 8, 8, 128, 128) <= X.BK_LDS and lds(1, 4, 8, 128, 128) <= X.BK_LDS      # stride 1 always has a form that fits
    assert lds(2, 4, 16, 64, 128) <= X.BK_LDS < min(lds(2, 4, 16, 128, 16), lds(2, 4, 16, 96, 128))     # stride 2: any Cout at Cin <= 64
    assert X.bneck_route(2, 57, 250, 64, 64, 1) == 816 and X.bneck_route(2, 57, 250, 128, 128, 1) == 808      # enough blocks, no fit
    assert X.bneck_route(2, 57, 240, 64, 64, 1) == 808                         # 240 blocks of 8 x 16 only
    assert X.bneck_route(1, 80, 160, 32, 32, 1) == 808 and X.bneck_route(1, 80, 152, 32, 32, 1) == 408       # 200 / 190 tiles of 8 x 8
    for c in X.BK_TIER1 + X.BK_TIER2:
        S, TH, TW = X.BK_FORMS[c.form]
        assert X.bneck_route(c.B, c.H, c.W, c.Cin, c.Cout, c.stride) == c.form and S == c.stride, c
        assert lds(S, TH, TW, c.Cin, c.Cout) <= X.BK_LDS and X.bneck_supported(c.Cin, c.Cmid, c.Cout, c.stride, c.res), c
    c = X.BK_TIER1[0]
    assert c.B * X.cdiv(c.Ho, 8) * X.cdiv(c.Wo, 16) == 256 and c.Ho % 8 and c.Wo % 16 and c.Cmid // X.BK_CM == 3
    for table in (X.BK_TIER1, X.BK_TIER2):       # the four tile forms and both numeric forms at least twice (tier 1), once (tier 2)
        forms = [c.form for c in table]
        assert all(forms.count(f) >= (2 if table is X.BK_TIER1 else 1) for f in X.BK_FORMS)
    assert {c.wmode for c in X.BK_TIER1 if c.stride == 1} == {c.wmode for c in X.BK_TIER1 if c.stride == 2} == {'shadow', 'f32', 'skew'}
    assert not any(X.bneck_supported(*r) for r in X.BK_REFUSED)


@pytest.mark.parametrize('c', X.BK_TIER1, ids=repr)
def test_bneck_budget_accepts_every_tier1_case_and_rejects_8_bit_operands(c):
    o = X.BkOperands(c, 1)
    r = X.bneck_ref(o, o.bn)
    assert X.bneck_exact(o, r) and max(X.bneck_bits(r)) < 24
    ok, census = X.bneck_conditions(o, r)
    assert ok, census
    o8 = X.BkOperands(c, 1, eight_bit=True)
    assert not X.bneck_exact(o8, X.bneck_ref(o8, o8.bn, bound=True))
    with pytest.raises(AssertionError):          # and the reference itself refuses to round what is not an f32 number
        X.bneck_ref(o8, o8.bn)


def _fma32(a, b, c):
    """one FMA in f32: the product of two f32 numbers is exact in f64"""
    return (a.double() * b.double() + c.double()).float()


def _bk_tile(c):
    """the last tile of the last image, the ragged end of the map: (b, oy0, oy1, ox0, ox1) in output pixels"""
    _, TH, TW = X.BK_FORMS[c.form]
    oy0, ox0 = (c.Ho - 1) // TH * TH, (c.Wo - 1) // TW * TW
    return c.B - 1, oy0, c.Ho, ox0, c.Wo


def _bk_emulate(o, bn, defect=None):
    """f32 emulation of the three stages of csrc/bneck.hip from the same operands in a deliberately bad accumulation order -- channels
    last to first, one rounded addition per product; taps last to first with the product and the addition rounded apart -- rounding to
    bf16 where the kernel does.  defect: one realistic kernel defect in ONE tile (_bk_tile) of the case's tile form"""
    c = o.c
    f, v4 = (lambda t: t.float()), (lambda t: t.float().view(1, -1, 1, 1))
    bf = lambda t: t.bfloat16().float()
    x, w1, wd, w3 = f(o.x), f(o.w1), f(o.wdw), f(o.w3)
    sc = [v4(s) for _, s, _ in bn]
    sh = [v4(X.fma_f32(-m, s, b)) for m, s, b in bn]
    b_, oy0, oy1, ox0, ox1 = _bk_tile(c)
    S = c.stride

    def splice(good, bad, x0=ox0, x1=ox1, ch=slice(None)):
        out = good.clone()
        out[b_, ch, oy0:oy1, x0:x1] = bad[b_, ch, oy0:oy1, x0:x1]
        return out

    acc = torch.zeros(c.B, c.Cmid, c.H, c.W)
    for ci in reversed(range(c.Cin)):
        acc = acc + x[:, ci:ci + 1] * w1[:, ci].view(1, -1, 1, 1)
    E = _fma32(acc, sc[0], sh[0]).clamp_min(0.0)
    if S == 2:
        E = bf(E)

    def depthwise(E, pad_value=None, s2=sc[1], t2=sh[1], shift_col=None):
        Ep = torch.nn.functional.pad(E, (1, 1, 1, 1))
        if pad_value is not None:                   # defect: relu(bn1(0)) instead of 0 outside the image
            border = torch.ones(1, 1, c.H + 2, c.W + 2)
            border[:, :, 1:-1, 1:-1] = 0
            Ep = Ep + border * pad_value
        if shift_col is not None:                   # defect: the tile's left halo column read one pixel too far left
            Ep = Ep.clone()
            Ep[:, :, :, shift_col + 1] = Ep[:, :, :, shift_col]
        acc = torch.zeros(c.B, c.Cmid, c.Ho, c.Wo)
        for t in reversed(range(9)):
            ky, kx = divmod(t, 3)
            win = Ep[:, :, ky:ky + S * (c.Ho - 1) + 1:S, kx:kx + S * (c.Wo - 1) + 1:S]
            acc = acc + win * wd[:, ky, kx].view(1, -1, 1, 1)
        return bf(_fma32(acc, s2, t2).clamp_min(0.0))

    D = depthwise(E)
    if defect == 'E not zeroed':
        D = splice(D, depthwise(E, pad_value=sh[0].clamp_min(0.0)))
    elif defect == 'halo shifted':
        assert ox0 > 0
        D = splice(D, depthwise(E, shift_col=ox0 * S - 1))
    elif defect == 'stale bn2':
        st = lambda t: torch.cat([t[:, :X.BK_CM], t[:, :X.BK_CM], t[:, 2 * X.BK_CM:]], 1)
        D = splice(D, depthwise(E, s2=st(sc[1]), t2=st(sh[1])))
    elif defect == 'E in bf16':
        assert S == 1
        D = splice(D, depthwise(bf(E)))

    acc = torch.zeros(c.B, c.Cout, c.Ho, c.Wo)
    for cm in reversed(range(c.Cmid)):
        acc = acc + D[:, cm:cm + 1] * w3[:, cm].view(1, -1, 1, 1)
    if defect == 'Cout tail':
        assert c.Cout % 16 == 4                       # the quarter fragment takes the next quarter's accumulators: padded channels, zeros
        acc = splice(acc, torch.zeros_like(acc), ch=slice(c.Cout - 4, c.Cout))
    v = _fma32(acc, sc[2], sh[2])
    if c.res:
        skip = x
        if defect == 'skip from the neighbour':       # the tile's first column adds the pixel to its right
            skip = splice(x, torch.roll(x, -1, 3), x1=ox0 + 1)
        v = v + skip
    return bf(v.clamp_min(0.0)).double()


def _affine32(gamma, rm, rv, eps, eps_outside=False):
    """bn_eval_affine_kernel step by step in f32: (mean, invstd, scale) as f64.  eps_outside: a defect, 1 / (sqrt(var) + eps)"""
    f = lambda t: t.numpy().astype(X.F32)
    e = X.F32(eps)
    invstd = X.F32(1) / (np.sqrt(f(rv)) + e if eps_outside else np.sqrt(f(rv) + e))
    scale = invstd if gamma is None else f(gamma) * invstd
    t = lambda a: torch.from_numpy(a.astype(np.float64))
    return rm, t(invstd), t(scale)


T1_EMU = [X.BK_TIER1[4], X.BK_TIER1[10], X.BK_TIER1[13], X.BK_TIER1[8]]      # (128, 768, 128) + skip; (40, 128, 20) 13 x 21; stride 2; 1 x 9
T1_DEFECTS = [(4, 'E not zeroed'), (4, 'halo shifted'), (4, 'skip from the neighbour'), (4, 'stale bn2'), (4, 'E in bf16'), (10, 'Cout tail'),
              (13, 'E not zeroed'), (13, 'halo shifted')]


@pytest.mark.parametrize('c', T1_EMU, ids=repr)
def test_bneck_f32_emulation_in_a_bad_order_is_bit_for_bit_on_tier1_operands(c):
    o = X.BkOperands(c, 1)
    r = X.bneck_ref(o, o.bn)
    assert X.bneck_exact(o, r)
    assert torch.equal(_bk_emulate(o, o.bn), r['y'])


@pytest.mark.parametrize('i,defect', T1_DEFECTS)
def test_bneck_tier1_fails_with_one_defect_in_one_tile(i, defect):
    o = X.BkOperands(X.BK_TIER1[i], 1)
    r = X.bneck_ref(o, o.bn)
    bad = _bk_emulate(o, o.bn, defect)
    wrong = (bad != r['y']).nonzero()
    assert len(wrong) > 0, defect
    b_, oy0, oy1, ox0, ox1 = _bk_tile(o.c)           # and only that tile is wrong
    assert bool(((wrong[:, 0] == b_) & (wrong[:, 2] >= oy0) & (wrong[:, 3] >= ox0)).all())


def _t2_affines(o):
    return [_affine32(g, rm, rv, X.BK_EPS)[::2] + (beta,) for g, rm, rv, beta in o.frozen]


T2_EMU = [X.BK_TIER2[2], X.BK_TIER2[3], X.BK_TIER2[4]]                        # (128, 768, 128) + skip; (40, 128, 20); stride 2
T2_DEFECTS = [(2, 'E not zeroed'), (2, 'halo shifted'), (2, 'skip from the neighbour'), (2, 'stale bn2'), (3, 'Cout tail'), (4, 'E not zeroed')]


@pytest.mark.parametrize('c', T2_EMU, ids=repr)
def test_bneck_f32_emulation_in_a_bad_order_meets_the_tier2_bound(c):
    o = X.BkOperands(c, 2)
    bn = _t2_affines(o)
    r = X.bneck_ref(o, bn, bound=True)
    out = _bk_emulate(o, bn)
    assert bool(((out - r['y']).abs() <= r['bound']).all())
    assert bool((torch.isfinite(r['bound']) & (r['bound'] >= 0)).all())
    assert float((r['y'] == 0).double().mean()) <= X.BK_ZERO_CAP


@pytest.mark.parametrize('i,defect', T2_DEFECTS)
def test_bneck_tier2_fails_with_one_defect_in_one_tile(i, defect):
    o = X.BkOperands(X.BK_TIER2[i], 2)
    bn = _t2_affines(o)
    r = X.bneck_ref(o, bn, bound=True)
    assert not bool(((_bk_emulate(o, bn, defect) - r['y']).abs() <= r['bound']).all()), defect


def test_fma_f32_rounds_once():
    g = _gen(5)
    a, b, c = (X.full_f32((512,), g) for _ in range(3))
    got = X.fma_f32(a, b, c)
    assert torch.equal(got.float().double(), got)
    exact = a * b + c                                 # f64: off by at most 2^-53 relative, so the f32 neighbours bracket it
    assert bool(((got - exact).abs() <= 2.0 ** -24 * exact.abs() * (1 + 2.0 ** -20)).all())
    assert torch.equal(X.fma_f32(torch.tensor([3.0]), torch.tensor([0.5]), torch.tensor([0.25])), torch.tensor([1.75], dtype=torch.float64))


def test_affine_u_counts_hold_for_an_f32_emulation_over_a_sweep_of_variances():
    g = _gen(6)
    n = 200000
    rv = torch.exp(torch.rand((n,), generator=g, dtype=torch.float64) * 30 - 18).float().double()      # 1.5e-8 .. 1.6e5
    gamma, rm = X.dyadic((n,), g) * 1.37, X.dyadic((n,), g)
    gamma = gamma.float().double()
    for eps in (1e-5, 1e-3):
        for gm in (gamma, None):
            mean, invstd, scale = X.affine_ref(gm, rm, rv, eps)
            m32, i32, s32 = _affine32(gm, rm, rv, eps)
            assert torch.equal(m32, mean)
            assert X.affine_excess(i32, invstd, X.AFFINE_U[0]) <= 0 and X.affine_excess(s32, scale, X.AFFINE_U[1]) <= 0
            assert X.affine_excess(i32, invstd, 1) > 0            # three roundings do show: one u would not hold
            _, ibad, _ = _affine32(gm, rm, rv, eps, eps_outside=True)
            assert X.affine_excess(ibad, invstd, X.AFFINE_U[0]) > 0


def test_join_geometry_edges_and_the_lane_chain():
    assert X.join_geometry(1, 8) == (256, 1) and X.join_geometry(38407, 136) == (15, 512) and X.join_geometry(512, 2048) == (1, 512)
    for C in (8, 24, 136, 2048):
        NPL = X.JOIN_NT // (C // 8)
        assert X.join_P('grid', C) == 512 * NPL and X.join_geometry(X.join_P('grid', C), C, X.JOIN_FWD_BLOCKS)[1] == 512
        assert X.join_stats_chain(X.join_P('grid', C), C) == 1 and X.join_stats_chain(X.join_P('grid', C) + 1, C) == 2
    assert X.JOIN_NT // (136 // 8) * (136 // 8) == 255            # C = 136: the block's last thread owns no pixel
    P = X.join_P('second', 136)
    assert P == 38407 and X.join_stats_chain(P, 136) == 6
    # a lane's second trip (pixels p0 + 4 k stride, k = 0 .. 3) is partly inside for the first 7 lanes of block 0 and wholly outside for none
    stride = 512 * 15
    inside = [sum(p0 + 4 * stride + u * stride < P for u in range(4)) for p0 in range(stride)]
    assert set(inside) == {1, 2} and inside.count(2) == 7


def _join32(a, A, b, Bf, relu, dtype, relu_first=False):
    """join_fwd_kernel in f32, in the kernel's order; relu_first: a defect, the ReLU applied before the second branch is added"""
    br = lambda v, aff: (v.float() - aff[0].float()) * aff[1].float() + aff[2].float() if aff is not None else v.float()
    s = br(a, A)
    if relu_first and relu:
        s = s.clamp_min(0.0)
    if b is not None:
        s = s + br(b, Bf)
    if relu:
        s = s.clamp_min(0.0)
    return (s.bfloat16() if dtype == torch.bfloat16 else s).double()


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_join_emulation_is_bit_for_bit_and_a_relu_before_the_second_branch_fails(dtype):
    g = _gen(7)
    P, C = 300, 24
    mk = lambda: (X.dyadic((C,), g), X.pow2((C,), g, 0.5, 4), X.dyadic((C,), g))
    A, Bf = mk(), mk()
    a, b = X.plant_zeros(X.dyadic((P, C), g), *A, g, 0.25), X.plant_zeros(X.dyadic((P, C), g), *Bf, g, 0.25)
    for relu in (0, 1):
        for aa, bb, AA, BB in ((a, b, A, Bf), (a, b, None, Bf), (a, b, A, None), (a, None, A, None), (a, None, None, None)):
            want = X.out_bits_ref(X.join_fwd_ref(aa, AA, bb, BB, relu), dtype == torch.bfloat16)
            assert torch.equal(_join32(aa, AA, bb, BB, relu, dtype), want)
    want = X.out_bits_ref(X.join_fwd_ref(a, A, b, Bf, 1), dtype == torch.bfloat16)
    assert bool((X.join_fwd_ref(a, A, b, Bf, 0) == 0).any())
    assert not torch.equal(_join32(a, A, b, Bf, 1, dtype, relu_first=True), want)


def _join_bwd_slabs(e, raw, mean, C, P, skip_zeroing=None):
    """join_bwd_kernel<bf16>'s statistics rows on the CPU from NaN slabs: a lane adds the pixels it owns in f32, the block's lanes meet
    in f64, and the blocks zero the rows nobody owns.  skip_zeroing: a defect, that row is left as it was"""
    NPL, grid = X.join_geometry(P, C)
    slabs = torch.full((X.STAT_SLABS, 2 * C), float('nan'), dtype=torch.float64)
    terms = torch.cat([e, e * (raw - mean)], 1).float()
    span = grid * NPL
    trips = X.cdiv(P, span)
    padded = torch.zeros(trips * span, 2 * C)
    padded[:P] = terms
    lanes = torch.zeros(span, 2 * C)
    for k in range(trips):
        lanes = lanes + padded[k * span:(k + 1) * span]
    slabs[:grid] = lanes.double().reshape(grid, NPL, 2 * C).sum(1)
    for r in range(grid, X.STAT_SLABS):
        if r != skip_zeroing:
            slabs[r] = 0.0
    return slabs, grid


def test_join_backward_statistics_emulation_and_an_unowned_row_left_unzeroed_fails():
    from tests.exact_gpu import check_slab_rows
    g = _gen(8)
    for C, kind in ((136, 'second'), (24, 'short')):
        P = X.join_P(kind, C)
        dout, out = X.dyadic((P, C), g, zero_frac=0.03), X.dyadic((P, C), g).clamp_min(0.0)
        raw, mean = X.dyadic((P, C), g), X.dyadic((C,), g)
        e = X.join_bwd_ref(dout, out, 1, 2.0)
        assert torch.equal(e, X.rne_bf16(e)) and bool(((e == 0) == ((out <= 0) | (dout == 0))).all())
        slabs, grid = _join_bwd_slabs(e, raw, mean, C, P)
        check_slab_rows(slabs, range(grid), kind)
        terms = X.exact_f32(torch.cat([e, e * X.exact_f32(raw - mean)], 1))
        assert X.stats_excess(slabs.sum(0), terms, X.join_stats_chain(P, C)) <= 0
        bad, _ = _join_bwd_slabs(e, raw, mean, C, P, skip_zeroing=X.STAT_SLABS - 1 if grid < X.STAT_SLABS else None)
        if grid < X.STAT_SLABS:
            with pytest.raises(AssertionError):
                check_slab_rows(bad, range(grid), kind)
        else:                                     # every row owned: a block that wrote nothing leaves its NaN
            slabs[grid - 1] = float('nan')
            with pytest.raises(AssertionError):
                check_slab_rows(slabs, range(grid), kind)


# ---------------------------------------------------------------------------------------------------------- fused decoder head
from tests import head_emu as HE          # noqa: E402
from tests import msflip_ref, wce_ref     # noqa: E402

HEAD_ALL = X.HEAD_REG + X.HEAD_REG_T2 + X.HEAD_WIDE + X.HEAD_WIDE_T2
HEAD_EMU = [c for c in X.HEAD_REG + X.HEAD_REG_T2 if c.name not in ('band32', 'band64')]        # what the emulation walks in seconds
_head_refs = {}


def _head(case):
    if case.name not in _head_refs:
        x, labels, plants = X.head_inputs(case)
        _head_refs[case.name] = (x, labels, plants, X.HeadRef(x, labels, weighted=False))
    return _head_refs[case.name]


@pytest.mark.parametrize('c', HEAD_ALL, ids=repr)
def test_head_restated_geometry_holds_every_tap(c):
    """every tap of every output pixel lies inside the band rows and strip cells the restatement gives, the tile extents cover that
    footprint, the gather windows hold every lane that touches a cell (one lane short does not) and the table clamp never cuts"""
    geo = c.geom()
    yi0, yi1, _, _ = X.ac_taps_np(c.h, c.H)
    xi0, xi1, xl0, xl1 = X.ac_taps_np(c.w, c.W)
    assert geo['nband'] * geo['band_rows'] >= c.H > (geo['nband'] - 1) * geo['band_rows']
    for band in range(geo['nband']):
        ya, yb = X.head_band(geo, band, c.H)
        r0, r1 = X.head_band_rows(c.h, c.H, ya, yb)
        assert r0 <= yi0[ya:yb].min() and yi1[ya:yb].max() <= r1 and r1 - r0 + 1 <= geo['tile_rows'] <= c.h
        assert (np.diff(yi0[ya:yb]) <= 1).all()                 # loss.hip's `if (ty.i0 != rA)` advances by one row at most
    for strip in range(geo['nstrip']):
        s = X.head_strip_cells(c.w, c.W, strip)
        x0 = strip * X.HEAD_NT
        assert s['c0'] <= xi0[x0:x0 + s['lanes']].min() and xi1[x0:x0 + s['lanes']].max() < s['c0'] + s['ncell']
        assert s['ncell'] <= geo['tile_cells'] and s['ncell'] <= X.HEAD_NT + 2
        for cell in range(s['ncell']):
            lo, hi = X.head_lane_window(c.w, c.W, strip, cell)
            lanes = np.arange(s['lanes'])
            col = s['c0'] + cell
            touch = lanes[((xi0[x0 + lanes] == col) & (xl0[x0 + lanes] != 0)) | ((xi1[x0 + lanes] == col) & (xl1[x0 + lanes] != 0))]
            assert touch.size == 0 or (lo <= touch.min() and touch.max() <= hi), (strip, cell)
            full = X.ac_window(c.w, c.W, col)
            assert (not s['wtab']) or min(full[1] - x0, X.HEAD_NT - 1) - max(full[0] - x0, 0) + 1 <= s['maxwin']      # "cannot happen"
    assert X.window_misses(c.w, c.W) == 0 and X.window_misses(c.w, c.W, short=1) > 0
    assert X.window_misses(c.h, c.H) == 0
    assert geo['ws_floats'] == geo['nblocks'] * (4 + geo['tile_rows'] * geo['tile_cells'] * geo['cp'])


def test_head_cases_reach_what_they_are_listed_for():
    by = X.HEAD_BY_NAME
    last_band = lambda c: c.H - (c.geom()['nband'] - 1) * c.geom()['band_rows']
    c = by['one_lane_strip']
    assert (c.geom()['nstrip'], c.geom()['nband'], last_band(c)) == (2, 3, 1) and [s['lanes'] for s in c.strips()] == [256, 1]
    assert all(s['wtab'] for s in c.strips())
    c = by['no_table']
    assert X.ac_scale_f32(c.w, c.W) == 0.5 and [s['wtab'] for s in c.strips()] == [False, True] and c.strips()[0]['ncell'] * 10 > X.HEAD_WTAB
    c = by['identity']
    yi0 = X.ac_taps_np(c.h, c.H)[0]
    assert (np.diff(yi0) == 1).all() and yi0[-1] == c.h - 1                     # a flush on every row; rB == rA at the end
    assert (c.geom()['nband'], last_band(c)) == (2, 2) and [s['lanes'] for s in c.strips()] == [256, 44]
    assert [s['wtab'] for s in c.strips()] == [False, True]       # 257 x 8 > 1024: the full strip gathers without the table, the 44-lane one with it
    assert by['few_class'].ldl == 8 < X.head_cp(5)
    assert X.head_cp(20) == 20 == by['c20'].C and X.head_cp(21) == 24 > by['cp24'].C and X.head_cp(24) == 24 == by['c24'].ldl == by['c24'].C
    assert by['h1'].h == 1 and by['w1'].w == 1 and X.head_lane_window(1, by['w1'].W, 0, 0) == (0, by['w1'].W - 1)
    assert by['pitch32'].ldl == 32
    assert (by['band32'].geom()['band_rows'], by['band32'].geom()['nband'], last_band(by['band32'])) == (32, 129, 1)
    assert by['band64'].geom()['band_rows'] == 64 and by['band64'].geom()['nblocks'] >= X.HEAD_FULL_GRID
    assert all(c.geom()['band_rows'] == 16 for c in HEAD_ALL if c.name not in ('band32', 'band64'))
    assert all(c.exact for c in X.HEAD_REG + X.HEAD_WIDE) and not any(c.exact for c in X.HEAD_REG_T2 + X.HEAD_WIDE_T2)
    assert all(c.C <= X.HEAD_REG_CAP for c in X.HEAD_REG + X.HEAD_REG_T2) and all(X.HEAD_REG_CAP < c.C <= X.HEAD_WIDE_CAP for c in X.HEAD_WIDE)
    assert by['c33'].C % X.HEAD_WK == 1 and by['c97'].C == X.HEAD_WCM_LDS + 1 and by['c256'].counts()['nchunk'] == 16
    assert [c.counts()['nchunk'] for c in X.HEAD_WIDE] == [2, 3, 5, 9, 16, 7]


@pytest.mark.parametrize('c', [c for c in X.HEAD_REG + X.HEAD_WIDE if c.name not in ('band32', 'band64')], ids=repr)
def test_head_tier1_premise_and_planted_ties(c):
    """the budget of every tier-1 case, and the planted ties where the case has room for them: the pair's classes tie for the maximum
    somewhere and the reference gives the lower index"""
    x, labels, plants, ref = _head(c)
    ky, kx = X.exact_resize(c.h, c.H), X.exact_resize(c.w, c.W)
    assert X.lsb_exp(x) >= -2 and ref.zmax <= 8 and X.exact_budget(ref.zabs, -2, ky, kx)
    assert torch.equal(ref.z.float().double(), ref.z)                        # every interpolated logit is an f32 number
    assert float((ref.gap == 0).double().mean()) > 0
    ry, rx = (c.H - 1) // max(c.h - 1, 1), (c.W - 1) // max(c.w - 1, 1)         # whole ratios on every case of the tables
    for (kind, a, b, r, col) in plants:
        oy, ox = r * ry, col * rx
        if kind == 'cross':
            if rx % 2:
                continue                                                     # no output pixel at the midpoint
            ox += rx // 2
            assert (ref.z[:, a, oy, ox] == 2).all()
        zp = ref.z[:, :, oy, ox]
        if kind == 'all':
            assert (zp == 1).all() and (ref.arg[:, oy, ox] == 0).all(), (c, kind)
        else:
            assert (zp[:, a] == zp[:, b]).all() and (zp[:, a] == zp.max(1).values).all() and (ref.arg[:, oy, ox] == a).all(), (c, kind, a, b)
    pairs = {(p[1], p[2]) for p in plants if p[0] == 'planes'}
    if c.name in ('one_lane_strip', 'cp24', 'pitch32'):
        assert {(3, 4), (0, 1)} <= pairs
    if c.name in ('cp24', 'c24'):
        assert (19, 20) in pairs
    if c.wide:
        assert (15, 16) in pairs and (c.C < 256 or (0, 255) in pairs)


def test_head_read_extent_stays_inside_the_pitch():
    """every kernel of the family, every case: the channels read of a pixel end inside its pitch; the extents of loss.hip before its
    GUARD instances did not ('few_class', C = 5 at ldl = 8: 20 channels)"""
    import os
    for c in HEAD_ALL:
        for k in X.HEAD_KERNELS:
            if k.startswith('wide') == c.wide:
                assert X.head_read_extent(c.C, c.ldl, k) <= c.ldl, (c, k)
    old = [c.name for c in X.HEAD_REG + X.HEAD_REG_T2 if X.head_read_extent(c.C, c.ldl, 'ce_onepass', guarded=False) > c.ldl]
    assert old == ['few_class'] and X.head_read_extent(5, 8, 'argmax', guarded=False) == 20
    for C in range(1, 25):                          # ops.new_nhwc's pitch, and the narrowest pitch head_shape_ok lets through
        for ldl in (X.cdiv(C, 8) * 8, X.cdiv(X.cdiv(C, 4) * 4, 8) * 8):
            assert X.head_read_extent(C, ldl, 'ce_onepass') <= ldl and X.head_read_extent(C, ldl, 'argmax') <= ldl
            assert (X.head_read_extent(C, ldl, 'ce_onepass', guarded=False) > ldl) == (C <= 16)
    src = open(os.path.join(os.path.dirname(__file__), '..', 'torch_semantic_segmentation_amd', 'csrc', 'loss.hip')).read()
    assert src.count('TSS_WITH_ROW_GUARD(ldl < CPV,') == 6 and src.count('if (!GUARD || c4 < C)') == 2      # the host rule restated above


def test_head_reference_is_wce_ref_and_the_recipe_ohem():
    """X.HeadRef against tests/wce_ref.py (loss and autograd gradient, f64) on an exact pair, where bilinear_matrix is torch's
    align_corners=True; X.ohem_ref against oracle.recipe.ohem"""
    from oracle import recipe
    c = X.HEAD_BY_NAME['cp24']
    x, labels, _, ref = _head(c)
    g = _gen(3)
    cw = torch.randint(1, 9, (c.C,), generator=g).double() / 4
    cw[c.C // 2] = 0
    for (w_, eps) in ((None, 0.0), (cw, 0.0), (None, 0.125), (cw, 0.125)):
        import copy
        r = copy.copy(ref).weights(w_, eps, grad_out=0.7)
        loss, grad = wce_ref.loss_and_grad(wce_ref.upsampled_wce_loss, x, labels, torch.float64, w_, 255, eps)
        assert abs(r.loss - float(loss)) <= 1e-12 * abs(r.loss)
        assert float((r.g - 0.7 * grad).abs().max()) <= 1e-12 * float(r.A.max())
        assert (r.A >= r.g.abs() - 1e-18).all() and r.S >= abs(r.loss) * r.den
    logits = torch.randn(2, 5, 8, 16, generator=g, dtype=torch.float64) * 3
    tgt = torch.randint(0, 5, (2, 8, 16), generator=g)
    tgt[0, :2] = 255
    per = torch.nn.functional.cross_entropy(logits, tgt, ignore_index=255, reduction='none')
    for (thresh, frac) in ((0.35, 0.1), (0.35, 0.9), (50.0, 0.25)):
        want = recipe.ohem(logits, tgt, 255, thresh, frac)
        got, sel = X.ohem_ref(per, thresh, int(per.numel() * frac))
        assert abs(got - float(want)) <= 1e-12 * abs(float(want))
        pw = X.ohem_pixel_weights(per, sel)                                  # the params reproduce the loss as a weighted sum
        assert abs(float((pw * per).sum()) - got) <= 1e-12 * abs(got)


def _ratio(out, ref, bound):
    err = (torch.as_tensor(np.asarray(out, dtype=np.float64)) - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float('inf'))))
    r = torch.where(torch.isnan(err), torch.full_like(r, float('inf')), r)
    return float(r.max())


def _head_variants(c):
    cw = torch.randint(1, 9, (c.C,), generator=_gen(11)).double() / 4
    cw[c.C // 2] = 0
    return ((0, None, 0.0), (3, cw, 0.0), (4, None, 0.125), (4, cw, 0.125))


def _emu_ratios(c, mode, cw, eps, defect=None, order=1):
    """(loss ratio, gradient ratio) of the emulated pass against the case's bounds"""
    import copy
    x, labels, _, ref = _head(c)
    r = copy.copy(ref).weights(cw, eps, grad_out=float(np.float32(0.7)))
    n = c.counts()
    o = HE.ce_pass(x.numpy(), labels.numpy(), c.H, c.W, mode=mode, weight=None if cw is None else cw.numpy(), eps=eps, grad_out=0.7,
                   defect=defect, class_order=order)
    weighted = mode >= 3
    spix, sloss, sg = X.head_slack(r)
    rl = abs(float(o['loss']) - r.loss) / X.head_loss_bound(r, n, weighted, 0, sloss)
    assert defect is not None or abs(float(o['inv_count']) - 1 / r.den) <= X.U32 * (n['band_rows'] + 2) / r.den
    return rl, _ratio(o['dlow'], r.g, X.head_grad_bound(r, n, weighted, False, 0, sg))


@pytest.mark.parametrize('c', HEAD_EMU, ids=repr)
def test_head_f32_emulation_meets_the_tier2_bounds(c):
    """loss, gradient (plain, class weights, smoothing, both; the class loop also backwards), per-pixel cross-entropy and the OHEM
    gradient of the emulated pass within head_loss_bound / head_grad_bound / head_pix_bound"""
    import copy
    x, labels, _, ref = _head(c)
    n = c.counts()
    for i, (mode, cw, eps) in enumerate(_head_variants(c)):
        rl, rg = _emu_ratios(c, mode, cw, eps, order=-1 if i == 1 else 1)
        assert rl <= 1 and rg <= 1, (c, mode, rl, rg)
    pix = HE.ce_pass(x.numpy(), labels.numpy(), c.H, c.W, mode=1)['pix']
    assert (pix >= 0).all() and (pix[~ref.valid.numpy()] == 0).all()
    assert _ratio(pix, ref.pix, X.head_pix_bound(ref.zmax, c.C) + 2 * X.head_slack_z(ref)) <= 1
    cut = np.float32(np.median(pix))
    planted = pix.copy()
    planted[torch.rand(pix.shape, generator=_gen(12)).numpy() < 0.1] = cut
    sel = [0.0, float(cut), 0.0078125, 0.00390625]
    o = HE.ce_pass(x.numpy(), labels.numpy(), c.H, c.W, mode=2, pix=planted, sel=sel, grad_out=1.0)
    r = copy.copy(ref).weights(pixw=X.ohem_pixel_weights(torch.from_numpy(planted), sel), grad_out=1.0)
    assert _ratio(o['dlow'], r.g, X.head_grad_bound(r, n, False, False, 0, X.head_slack(r)[2])) <= 1


@pytest.mark.parametrize('c', [c for c in HEAD_ALL if c.name not in ('band32', 'band64')], ids=repr)
def test_head_argmax_emulation_is_bit_for_bit_on_tier1_and_inside_the_margin_elsewhere(c):
    """tier 1: the f32 walk gives the f64 arg-max at every pixel, forwards, with the class loop run backwards, and chunk by chunk;
    elsewhere every pixel whose top-2 gap exceeds msflip_ref.margin (K = 1) agrees and at most 1 % of the pixels are left out"""
    x, labels, _, ref = _head(c)
    chunk = X.HEAD_WK if c.wide else None
    for order in (1, -1):
        arg = torch.from_numpy(HE.argmax_walk(x.numpy(), c.H, c.W, class_order=order, chunk=chunk))
        if c.exact:
            assert torch.equal(arg, ref.arg), (c, order)
        else:
            m = msflip_ref.margin(1, c.C, ref.zmax, [(c.h, c.w)], (c.H, c.W), 'logits')
            decided = ref.gap > m
            assert 1 - float(decided.double().mean()) <= X.NEAR_TIE_CAP and torch.equal(arg[decided], ref.arg[decided])


HEAD_DEFECTS = (('edge_lane', 0), ('no_last_flush', 0), ('one_tile', 0), ('swap_last_row', 0), ('drop_onehot', 0), ('smooth_once', 4))


@pytest.mark.parametrize('defect,mode', HEAD_DEFECTS)
def test_head_emulation_with_one_defect_fails_the_gradient_bound(defect, mode):
    c = X.HEAD_BY_NAME['one_lane_strip']
    rl, rg = _emu_ratios(c, mode, None, 0.125 if mode == 4 else 0.0, defect=defect)
    assert rg > 1, (defect, rg)
    if defect in ('drop_onehot', 'smooth_once'):                  # the one-hot half also carries the target logits of the loss
        assert rl > 1, (defect, rl)


def test_head_emulation_arg_max_and_pixel_defects_fail():
    c = X.HEAD_BY_NAME['one_lane_strip']
    x, labels, _, ref = _head(c)
    ge = torch.from_numpy(HE.argmax_walk(x.numpy(), c.H, c.W, ge=True))
    assert not torch.equal(ge, ref.arg) and ((ge != ref.arg) <= (ref.gap == 0)).all()        # `>=`: wrong exactly on ties
    c = X.HEAD_BY_NAME['c33']
    x, labels, _, ref = _head(c)
    late = torch.from_numpy(HE.argmax_walk(x.numpy(), c.H, c.W, chunk=X.HEAD_WK, chunk_ge=True))
    assert not torch.equal(late, ref.arg) and set(late[late != ref.arg].tolist()) <= {16, 32}     # the later chunk's first class
    for name in ('one_lane_strip', 'few_class'):
        c = X.HEAD_BY_NAME[name]
        x, labels, _, ref = _head(c)
        pix = HE.ce_pass(x.numpy(), labels.numpy(), c.H, c.W, mode=1, defect='unclamped_i1')['pix']
        assert _ratio(pix, ref.pix, X.head_pix_bound(ref.zmax, c.C)) > 1


# ---------------------------------------------------------------------------------------------------------- Philox and the dropout masks
PHILOX_KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
              ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
              ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
SEED_HI = (7 << 32) | 3


def test_philox4x32_10_known_answers():
    """the Random123 known-answer vectors, one by one and as one batch"""
    for ctr, key, want in PHILOX_KAT:
        assert tuple(int(v) for v in PR.philox4x32_10([ctr], *key)[0]) == want
    same_key = PR.philox4x32_10([PHILOX_KAT[0][0], (1, 0, 0, 0), PHILOX_KAT[0][0]], 0, 0)
    assert tuple(int(v) for v in same_key[0]) == PHILOX_KAT[0][2] and (same_key[0] == same_key[2]).all() and (same_key[0] != same_key[1]).all()


@pytest.mark.parametrize('p', [0.1, 0.3, 0.5, 0.75])
def test_dropout_rules_keep_a_share_of_one_minus_p(p):
    """2^20 elements: the kept share within 6 standard deviations of the rule's exact probability (threshold / 2^32, / 2^16)"""
    n = 1 << 20
    keep = PR.dropout_keep(n // 128, 128, p, SEED_HI)
    q = 1 - PR.keep_threshold(p) / 2.0 ** 32
    assert abs(q - (1 - p)) < 2.0 ** -24 and abs(keep.mean() - q) <= 6 * np.sqrt(q * (1 - q) / n)
    bits_ = np.unpackbits(PR.dropout_mask_bytes(n // 128, p, SEED_HI))
    q = 1 - PR.mask_threshold(p) / 65536.0
    assert abs(q - (1 - p)) <= 2.0 ** -16 and bits_.size == n and abs(bits_.mean() - q) <= 6 * np.sqrt(q * (1 - q) / n)
    assert not np.array_equal(keep, PR.dropout_keep(n // 128, 128, p, 12345))


def _keep_mutant(P, C, p, seed, ld=None, high_word=True):
    """dropout_keep with the counter built from pix ld + c, or the key without the seed's high word"""
    idx = (np.arange(P, dtype=np.uint64)[:, None] * np.uint64(ld or C) + np.arange(C, dtype=np.uint64)[None, :]).reshape(-1)
    k0, k1 = PR.seed_key(seed)
    cw = np.zeros((idx.size, 4), np.uint64)
    cw[:, 0], cw[:, 1] = (idx >> np.uint64(2)) & np.uint64(0xFFFFFFFF), idx >> np.uint64(34)
    w = PR.philox4x32_10(cw, k0, k1 if high_word else PR.KEY_XOR)
    return (w[np.arange(idx.size), (idx & np.uint64(3)).astype(np.int64)] >= np.uint32(PR.keep_threshold(p))).reshape(P, C)


def test_dropout_rule_defects_change_the_mask():
    P, C, p = 37, 24, 0.5
    ref = PR.dropout_keep(P, C, p, SEED_HI)
    assert np.array_equal(_keep_mutant(P, C, p, SEED_HI), ref)                       # the mutant's own plumbing is sound
    assert not np.array_equal(_keep_mutant(P, C, p, SEED_HI, ld=40), ref)            # the counter from the pitch
    assert np.array_equal(_keep_mutant(P, C, p, SEED_HI, ld=40)[0], ref[0])          # ... which the first pixel alone cannot show
    assert not np.array_equal(_keep_mutant(P, C, p, SEED_HI, high_word=False), ref)  # the key without the seed's high word
    assert np.array_equal(_keep_mutant(P, C, p, 12345, high_word=False), PR.dropout_keep(P, C, p, 12345))   # ... invisible below 2^32
    # two elements sharing one word: every element of a counter's four has its own
    w = PR.dropout_words(1 << 12, SEED_HI)
    assert len(set(w.tolist())) > (1 << 12) - 4
    # the mask byte indexed by pix (C / 8) + v instead of pix 16 + v
    C8 = 1
    want = PR.dropout_mask_bytes(P, p, SEED_HI)
    dense = PR.dropout_mask_bytes(P, p, SEED_HI).reshape(-1)[:P * C8].reshape(P, C8)        # byte b of the dense numbering
    assert np.array_equal(dense[0], want[0, :C8]) and not np.array_equal(dense[1:, 0], want[1:, 0])
    assert len(set(want[:, 0].tolist())) > 8, 'a byte that repeats across pixels'


# ---------------------------------------------------------------------------------------------------------- BatchNorm finalize chain
def _slabs_of(x, rows=X.STAT_SLABS):
    """[rows][2 C] f64 slab rows of x [P][C] (numpy f64) as tss_tensor_stats lays them out: block i owns [i per, (i + 1) per)"""
    t = torch.from_numpy(x)
    per = X.cdiv(x.shape[0], rows)
    return torch.cat([X.block_sums(t, per, rows), X.block_sums(t * t, per, rows)], 1).numpy()


def test_bn_finalize_ref_is_torch_batchnorm_in_training_mode():
    """two training steps of torch.nn.BatchNorm2d in float64: batch statistics (through the normalised output), running statistics
    with the unbiased variance, to the f32 roundings the reference makes on purpose"""
    rng = X.np_rng(301)
    C, eps, mom = 5, 1e-5, 0.1
    bn = torch.nn.BatchNorm2d(C, eps=float(np.float32(eps)), momentum=float(np.float32(mom))).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 2, C).astype(np.float32).astype(np.float64)))
        bn.bias.zero_()
    rm, rv = np.zeros(C, np.float32), np.ones(C, np.float32)
    for step in range(2):
        x = rng.standard_normal((3, C, 7, 5)) * rng.uniform(0.5, 3, (1, C, 1, 1)) + rng.uniform(-2, 2, (1, C, 1, 1))
        y = bn(torch.from_numpy(x)).detach().numpy()
        rows = x.transpose(0, 2, 3, 1).reshape(-1, C)
        r = X.bn_finalize_ref(rows.sum(0), (rows * rows).sum(0), rows.shape[0], bn.weight.detach().numpy(), eps, mom, rm, rv)
        mine = (x - r['mean'].reshape(1, C, 1, 1).astype(np.float64)) * r['scale'].reshape(1, C, 1, 1).astype(np.float64)
        assert np.abs(mine - y).max() <= 2.0 ** -21 * np.abs(y).max()
        rm, rv = r['running_mean'], r['running_var']
        assert np.allclose(r['unbiased64'], rows.var(0, ddof=1), rtol=1e-12)
        assert np.allclose(rm, bn.running_mean.numpy(), rtol=2.0 ** -21, atol=2.0 ** -24)
        assert np.allclose(rv, bn.running_var.numpy(), rtol=2.0 ** -21)
    assert bn.num_batches_tracked.item() == 2
    one = X.bn_finalize_ref(np.array([3.0]), np.array([9.0]), 1.0, None, eps, mom, np.zeros(1), np.ones(1))
    assert one['var64'][0] == 0 and one['running_var'][0] == np.float32(1) - np.float32(mom)       # count 1: var itself, no division by 0


@pytest.mark.parametrize('training', [1, 0])
def test_bn_bwd_finalize_ref_is_torch_autograd(training):
    """ga (e - gce) + gb (y - mean) against torch's float64 input gradient of BatchNorm2d, dgamma / dbeta its parameter gradients"""
    rng = X.np_rng(303, training)
    C, eps = 6, 1e-5
    bn = torch.nn.BatchNorm2d(C, eps=float(np.float32(eps))).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 2, C).astype(np.float32).astype(np.float64)))
        bn.running_mean.copy_(torch.from_numpy(rng.uniform(-1, 1, C)))
        bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 2, C)))
    bn.train(bool(training))
    y = torch.from_numpy(rng.standard_normal((2, C, 5, 3)) * 2 + 1).requires_grad_(True)
    e = torch.from_numpy(rng.standard_normal((2, C, 5, 3)))
    rows = lambda t: t.detach().numpy().transpose(0, 2, 3, 1).reshape(-1, C)
    yr, er = rows(y), rows(e)
    if training:
        f = X.bn_finalize_ref(yr.sum(0), (yr * yr).sum(0), yr.shape[0], None, eps, 0.1)
        mean, invstd = f['mean'].astype(np.float64), f['invstd']
    else:
        mean, invstd = bn.running_mean.numpy(), (1.0 / np.sqrt(bn.running_var.numpy() + np.float64(np.float32(eps)))).astype(np.float32)
    bn(y).backward(e)
    b = X.bn_bwd_finalize_ref(er.sum(0), (er * (yr - mean)).sum(0), yr.shape[0], invstd, bn.weight.detach().numpy(), training, 1,
                              np.ones(C, np.float32), np.full(C, 2, np.float32))
    g = b['ga'].astype(np.float64) * (er - b['gce']) + b['gb'].astype(np.float64) * (yr - mean)
    assert np.abs(g - rows(y.grad)).max() <= 2.0 ** -19 * np.abs(rows(y.grad)).max()
    assert np.allclose(b['dgamma'] - 1, bn.weight.grad.numpy(), rtol=2.0 ** -18, atol=2.0 ** -20)
    assert np.allclose(b['dbeta'] - 2, bn.bias.grad.numpy(), rtol=2.0 ** -18, atol=2.0 ** -20)
    if not training:
        assert (b['gb'] == 0).all() and (b['gce'] == 0).all()


@pytest.mark.parametrize('k', [0, 3, 10, 16])
def test_finalize_tier1_premise(k):
    """integer slab rows sum exactly in any order; mean, mean^2, q / count and the variance are f64 numbers, with or without an FMA; the
    constant channel has var 0 and channel 1 is negative before the clamp; the running-statistics products are exact in f32"""
    rng = X.np_rng(305, k)
    C = 19
    slabs, s, q = X.fin_tier1_slabs(C, k, rng)
    assert slabs.shape == (X.STAT_SLABS, 2 * C) and ((slabs != 0).any(1).sum() <= X.STAT_SLABS // 2 + 1)
    for order in (np.arange(X.STAT_SLABS), rng.permutation(X.STAT_SLABS), np.arange(X.STAT_SLABS)[::-1]):
        acc = np.zeros(2 * C)
        for r in order:
            acc = acc + slabs[r]
        assert (acc[:C] == s).all() and (acc[C:] == q).all()
    si, qi = s.astype(np.int64), q.astype(np.int64)
    assert X.fin_tier1_premise(si, qi, k)
    bad = si.copy()
    bad[2] = 2 ** 27 + 1                                          # 28 bits: mean^2 is no f64 number any more
    assert not X.fin_tier1_premise(bad, qi, k)
    cnt = 2.0 ** k
    raw = q / cnt - (s / cnt) ** 2
    assert raw[0] == 0 and raw[1] <= -0.125 and raw[1] >= -2 and (raw[2:] > 0).all()
    assert int(np.abs(s).max()) >= 2 ** 21 and (k < 10 or (s / cnt).astype(np.float32).astype(np.float64).tolist() != (s / cnt).tolist())
    for m in (0.125, 0.5):
        rm = X.dyadic8_np(4096, rng).astype(np.float64)
        x = rng.standard_normal(4096).astype(np.float32).astype(np.float64)
        assert (((1 - m) * rm).astype(np.float32) == (1 - m) * rm).all() and ((m * x).astype(np.float32) == m * x).all()


def _emu_slab_sum(slabs, C, defect=None):
    """slab_sum of csrc/bnfin.h in its own order: lane (row group, column half, channel) adds rows wave 4 + rg + 16 u, u = 0 .. 31, the 16
    lane sums of a column meet in wave-major order.  Returns [2][8 blocks]; lanes past C hold 0 (no_guard: what they read and summed)"""
    rows, nblk = slabs.shape[0], X.cdiv(C, X.FIN_CH)
    flat = np.concatenate([slabs.reshape(-1), np.zeros(2 * C + 8)])
    out = np.zeros((2, nblk * X.FIN_CH))
    trips = rows // X.FIN_ROWS_PER_LOAD - (1 if defect == 'skip_row' else 0)
    for c in range(nblk * X.FIN_CH):
        inside = c < C
        for hs in range(2):
            col = flat[np.arange(rows) * 2 * C + hs * C + (c if inside or defect == 'no_guard' else 0)].reshape(-1, X.FIN_ROWS_PER_LOAD)
            lane = np.zeros(X.FIN_ROWS_PER_LOAD)
            for u in range(trips):
                lane = lane + col[u]
            a = 0.0
            for v in lane:
                a = a + v
            out[hs, c] = a if inside or defect == 'no_guard' else 0.0
    return out


PADV = 8
SENT = np.float32(0.8529)


def _emu_finalize(slabs, count, gamma, eps, momentum, rm, rv, C, defect=None):
    """bn_finalize_kernel in numpy: f64 up to invstd, f32 behind it; outputs in vectors with PADV sentinels behind C"""
    f32 = np.float32
    ss = _emu_slab_sum(slabs, C, defect)
    n = ss.shape[1] if defect == 'no_guard' else C
    s, q = ss[0, :n], ss[1, :n]
    if defect == 'f32_var':
        mean = (s.astype(f32) / f32(count))
        var = ((q.astype(f32) / f32(count)) - mean * mean).astype(np.float64)
        mean = mean.astype(np.float64)
    else:
        mean = s / count
        var = q / count - mean * mean
    if defect != 'no_clamp':
        var = np.maximum(var, 0.0)
    with np.errstate(invalid='ignore'):
        invstd = (1.0 / np.sqrt(var + np.float64(f32(eps)))).astype(f32)
    pad = lambda v: np.concatenate([np.asarray(v, f32), np.full(max(0, C + PADV - len(v)), SENT, f32)])[:C + PADV]
    g = np.ones(n, f32) if gamma is None else pad(gamma)[:n]
    m = f32(momentum)
    a, b = (m, f32(1) - m) if defect == 'swap_momentum' else (f32(1) - m, m)
    unbiased = var * count / (count - 1.0) if count > 1 and defect != 'biased' else var
    return dict(mean=pad(mean.astype(f32)), invstd=pad(invstd), scale=pad(g * invstd), running_mean=pad(a * pad(rm)[:n] + b * mean.astype(f32)),
                running_var=pad(a * pad(rv)[:n] + b * unbiased.astype(f32)))


def _tier1_faults(out, ref, gamma, C):
    """the checks of tests/test_gpu_bnfin_exact.py::check_tier1 and check_frame as a list of what fails"""
    bitsof = lambda v: np.ascontiguousarray(v, np.float32).view(np.uint32)
    bad = [k for k in ('mean', 'running_mean', 'running_var') if not np.array_equal(bitsof(out[k][:C]), bitsof(ref[k]))]
    inv = out['invstd'][:C].astype(np.float64)
    if not np.isfinite(inv).all() or (np.abs(inv - ref['invstd64']) > X.FIN_INVSTD_REL * ref['invstd64']).any():
        bad.append('invstd')
    if not np.array_equal(bitsof(out['scale'][:C]), bitsof(X.bn_scale_ref(gamma, out['invstd'][:C]))):
        bad.append('scale')
    if any((v[C:] != SENT).any() for v in out.values()):
        bad.append('tail')
    return bad


FIN_DEFECTS = {'f32_var': 'invstd', 'biased': 'running_var', 'swap_momentum': 'running_mean', 'skip_row': 'mean', 'no_guard': 'tail',
               'no_clamp': 'invstd'}


@pytest.mark.parametrize('C', [4, 19, 132])
def test_finalize_emulation_is_bit_for_bit_on_tier1_and_each_defect_is_not(C):
    rng = X.np_rng(307, C)
    slabs, s, q = X.fin_tier1_slabs(C, 10, rng)
    gamma, rm, rv = rng.uniform(-2, 2, C).astype(np.float32), X.dyadic8_np(C, rng), X.dyadic8_np(C, rng, True)
    ref = X.bn_finalize_ref(s, q, 1024.0, gamma, 1e-5, 0.125, rm, rv)
    assert _tier1_faults(_emu_finalize(slabs, 1024.0, gamma, 1e-5, 0.125, rm, rv, C), ref, gamma, C) == []
    for defect, shows in FIN_DEFECTS.items():
        faults = _tier1_faults(_emu_finalize(slabs, 1024.0, gamma, 1e-5, 0.125, rm, rv, C, defect), ref, gamma, C)
        if defect == 'no_guard' and C % X.FIN_CH == 0:
            assert faults == []                                   # only a ragged channel count has lanes past C
        else:
            assert shows in faults, (defect, faults)


def test_finalize_tier2_bound_holds_for_the_emulation_and_rejects_an_f32_variance():
    """stored values near 30, deviation 2^-3: the f64 finalize sits orders of magnitude inside fin_tier2_bounds, an f32 variance orders of
    magnitude outside; a biased running_var and a swapped momentum fail their bounds too"""
    rng = X.np_rng(309)
    P, C, eps, mom = 3000, 24, 1e-5, 0.1
    x = X.offset_values(P, C, rng)
    slabs = _slabs_of(x)
    assert (slabs.sum(0)[:C] == x.sum(0)).all() and (slabs.sum(0)[C:] == (x * x).sum(0)).all()
    mean, var, qc = X.exact_moments(x)
    assert var[0] == 0 and np.allclose(var[1:], x.var(0)[1:], rtol=1e-9) and np.allclose(mean, x.mean(0), rtol=1e-14)
    rm, rv = rng.uniform(-3, 3, C).astype(np.float32), rng.uniform(0.01, 0.03, C).astype(np.float32)
    b = X.fin_tier2_bounds(var, qc, mean, eps, float(P), mom, rm.astype(np.float64), rv.astype(np.float64))
    m64, t = np.float64(np.float32(mom)), var + np.float64(np.float32(eps))
    refs = dict(invstd=t ** -0.5, running_mean=(1 - m64) * rm.astype(np.float64) + m64 * mean,
                running_var=(1 - m64) * rv.astype(np.float64) + m64 * var * P / (P - 1.0))

    def ratios(defect=None):
        o = _emu_finalize(slabs, float(P), None, eps, mom, rm, rv, C, defect)
        return {k: float((np.abs(o[k][:C].astype(np.float64) - refs[k]) / b[k]).max()) for k in refs}
    ok = ratios()
    assert max(ok.values()) <= 1, ok
    assert (b['invstd'][1:] <= 1.01 * X.FIN_INVSTD_REL * refs['invstd'][1:]).all()        # the bound is one f32 rounding, not slack
    assert ratios('f32_var')['invstd'] > 1000 and ratios('biased')['running_var'] > 100 and ratios('swap_momentum')['running_mean'] > 1000


def _emu_bwd(slabs, count, invstd, gamma, C, defect=None):
    ss = _emu_slab_sum(slabs, C, 'skip_row' if defect == 'skip_row' else None)
    se, sey, r = ss[0, :C], ss[1, :C], invstd.astype(np.float64)
    k = gamma.astype(np.float64) * r
    c2 = r * sey / count
    gb = -k * c2 if defect == 'gb_one_invstd' else -k * c2 * r
    return dict(dgamma=np.float32(0) + (r * sey).astype(np.float32), dbeta=np.float32(0) + se.astype(np.float32), ga=k.astype(np.float32),
                gb=gb.astype(np.float32), gce=(se / count).astype(np.float32))


def test_bwd_finalize_emulation_is_bit_for_bit_and_each_defect_is_not():
    C = 19
    rng = X.np_rng(311)
    slabs, se, sey = X.fin_bwd_slabs(C, rng)
    invstd, gamma = rng.uniform(0.05, 40, C).astype(np.float32), rng.uniform(-2, 2, C).astype(np.float32)
    ref = X.bn_bwd_finalize_ref(se, sey, 1000.0, invstd, gamma)
    same = lambda o: [k for k in ref if not np.array_equal(o[k].view(np.uint32), ref[k].view(np.uint32))]
    assert same(_emu_bwd(slabs, 1000.0, invstd, gamma, C)) == []
    assert same(_emu_bwd(slabs, 1000.0, invstd, gamma, C, 'gb_one_invstd')) == ['gb']
    assert set(same(_emu_bwd(slabs, 1000.0, invstd, gamma, C, 'skip_row'))) >= {'dgamma', 'dbeta', 'gb', 'gce'}
    # the sign convention of gb: g = ga (e - gce) + gb (y - mean) must REMOVE the component along y - mean
    assert (np.sign(ref['gb']) == -np.sign(gamma.astype(np.float64) * sey)).all()
    frozen = X.bn_bwd_finalize_ref(se, sey, 1000.0, invstd, gamma, training=0, accumulate=1, dgamma=np.ones(C), dbeta=np.ones(C))
    assert (frozen['gb'] == 0).all() and (frozen['gce'] == 0).all() and np.array_equal(frozen['dbeta'], np.float32(1) + se.astype(np.float32))
    two = X.bn_bwd_finalize_ref(se * 2, sey * 2, 2000.0, invstd, gamma, local=(se, sey))       # two equal replicas: the same coefficients
    assert same(two) == []


def _emu_tensor_stats_vec(v, P, C):
    """tensor_stats_vec_kernel<bf16>: a lane's f32 partial sums over its pixels p0 + pl + j npl in order, lanes and rows in f64"""
    _, per, npl = X.tensor_stats_plan(P, C, 8)
    rows = np.zeros((X.STAT_SLABS, 2 * C))
    x = v.astype(np.float32)
    for i in range(X.STAT_SLABS):
        blk = x[i * per:min(P, (i + 1) * per)]
        trips = X.cdiv(len(blk), npl)
        if trips == 0:
            continue
        padded = np.zeros((trips * npl, C), np.float32)
        padded[:len(blk)] = blk
        padded = padded.reshape(trips, npl, C)
        s, q = np.zeros((npl, C), np.float32), np.zeros((npl, C), np.float32)
        for j in range(trips):
            s, q = s + padded[j], q + padded[j] * padded[j]
        rows[i, :C], rows[i, C:] = s.astype(np.float64).sum(0), q.astype(np.float64).sum(0)
    return rows


@pytest.mark.parametrize('P,C', [(70001, 16), (2100, 1024), (20000, 128)])
def test_tensor_stats_emulation_meets_the_row_bound(P, C):
    v = X.dyadic((P, C), _gen(313))
    rows = torch.from_numpy(_emu_tensor_stats_vec(v.numpy(), P, C))
    _, per, npl = X.tensor_stats_plan(P, C, 8)
    chain = X.tensor_stats_chain(P, C)
    assert chain == X.cdiv(X.cdiv(P, 512), npl) + 1
    worst = 0.0
    for half, terms in ((0, v), (1, v * v)):
        ref, mag = X.block_sums(terms, per), X.block_sums(terms.abs(), per)
        worst = max(worst, float(((rows[:, half * C:(half + 1) * C] - ref).abs() / ((2.0 ** -23 * chain + 2.0 ** -50) * mag.clamp_min(1e-300))).max()))
    assert worst <= 1
    assert X.stats_excess(rows.sum(0), torch.cat([v, v * v], 1), chain) <= 0
    shifted = torch.from_numpy(_emu_tensor_stats_vec(np.roll(v.numpy(), 1, 0), P, C))           # every block owns the pixel before its range
    assert float(((shifted[:, :C] - X.block_sums(v, per)).abs() - (2.0 ** -23 * chain + 2.0 ** -50) * X.block_sums(v.abs(), per)).max()) > 0
    assert X.tensor_stats_plan(2047, 128, 128)[0] == 'scalar' and X.tensor_stats_plan(2048, 1032, 1032)[0] == 'scalar' and \
        X.tensor_stats_plan(2048, 128, 133)[0] == 'scalar' and X.tensor_stats_plan(2048, 1024, 1024) == ('vec', 4, 2)


def _emu_colsum(e, init, defect=None):
    """colsum_kernel in f32: lane sums in pixel order, the four lane rows of a block, one atomic per block in block order"""
    P, N = e.shape
    grid, lane = X.colsum_plan(P)
    x = np.zeros((lane * grid * 4, N), np.float32)
    x[:P] = e.astype(np.float32)
    x = x.reshape(lane, grid, 4, N)
    s = np.zeros((grid, 4, N), np.float32)
    for j in range(lane):
        s = s + x[j]
    blk = ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]
    out = init.astype(np.float32)
    for b in range(grid):
        out = blk[b] if defect == 'overwrite' else out + blk[b]
    return out


def test_colsum_emulation_is_exact_on_tier1_within_the_chain_bound_on_tier2_and_overwriting_is_not():
    for P in (3, 4101, 40000):
        e, init = X.colsum_exact_values(P, 19, X.np_rng(315, P))
        want = (init + e.sum(0)).astype(np.float32)
        assert (want.astype(np.float64) == init + e.sum(0)).all() and (init != 0).all()
        assert np.array_equal(_emu_colsum(e, init), want) and not np.array_equal(_emu_colsum(e, init, 'overwrite'), want)
        assert X.colsum_plan(P) == (min(X.cdiv(P, 4), 1024), X.cdiv(P, 4 * min(X.cdiv(P, 4), 1024)))
    rng = X.np_rng(317)
    P, N = 40000, 19
    e = rng.standard_normal((P, N)).astype(np.float32).astype(np.float64)
    init = rng.standard_normal(N).astype(np.float32)
    assert X.colsum_chain(P) == 10 + 3 + 1024
    bound = 2.0 ** -23 * X.colsum_chain(P) * (np.abs(init) + np.abs(e).sum(0))
    assert (np.abs(_emu_colsum(e, init).astype(np.float64) - (init + e.sum(0))) <= bound).all()
    assert not (np.abs(_emu_colsum(e, init, 'overwrite').astype(np.float64) - (init + e.sum(0))) <= bound).all()


def test_cast_sources_hold_the_planted_roundings():
    src = X.cast_sources(19, 128, X.np_rng(319))
    b = src.numpy().view(np.uint32)
    low = b & 0xFFFF
    assert ((low == 0x8000) & (((b >> 16) & 1) == 0)).any() and ((low == 0x8000) & (((b >> 16) & 1) == 1)).any()     # ties to even: down, up
    assert (low == 0x8001).any() and (low == 0x7FFF).any()
    expo = (b >> 23) & 0xFF
    assert ((expo == 0) & ((b & 0x7FFFFF) != 0)).any() and (b == 0).any() and (b == 0x80000000).any() and torch.isfinite(src).all()
    r = src.to(torch.bfloat16)
    rb = r.view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    tie = low == 0x8000
    assert ((rb[tie] & 1) == 0).all()                             # torch rounds ties to even: the reference of the GPU test
    assert (rb[low == 0x8001] == ((b[low == 0x8001] >> 16) + 1) & 0xFFFF).all() and (rb[low == 0x7FFF] == (b[low == 0x7FFF] >> 16)).all()


# ---------------------------------------------------------------------------------------------------------- soft losses and distillation
from tests import cases, distill_ref, softloss_emu as SE          # noqa: E402

DISTILL_KINDS = (('pixel', X.DISTILL_PIXEL_C, X.distill_pixel_cases), ('channel', X.DISTILL_CHANNEL_C, X.distill_channel_cases))
DISTILL_ALL = [(kind, C) + case for kind, Cs, casef in DISTILL_KINDS for C in Cs for case in casef(C)]
DISTILL_BY_NAME = {c[2]: c for c in DISTILL_ALL}


def _distill_emu(case, bf16, defect=None):
    kind, C, name, B, HW, cap, tau, hot = case
    s, t = X.distill_operands(B, C, HW, 0, hot)
    ref = X.DistillRef(s, t, tau, kind, 0.7, cap)
    loss, stats, d = SE.distill(s, t, tau, kind, cap, 0.7, bf16, defect)
    return s, t, ref, d, X.distill_ratios(ref, loss, stats, d, bf16)


def _old_gradient_criterion(case, s, t, d, bf16):
    """tests/test_gpu_distill.py's check on the gradient: cases.rel_err (max |a - b| / max |b| over the WHOLE tensor) against
    max(2e-5, 3 d_ref), d_ref the restatement's own f32-vs-f64 distance; 2e-2 for a bf16 gradient.  (error, bound)"""
    kind, C, name, B, HW, cap, tau, hot = case
    nchw = lambda v: torch.from_numpy(np.ascontiguousarray(np.transpose(v, (0, 2, 1)))).reshape(B, C, HW, 1)
    go = float(np.float32(0.7))
    g64 = distill_ref.loss_and_grad(nchw(s), nchw(t), torch.float64, tau, kind)[1].numpy() * go
    g32 = distill_ref.loss_and_grad(nchw(s), nchw(t), torch.float32, tau, kind)[1].double().numpy() * go
    return cases.rel_err(nchw(d.astype(np.float64)).numpy(), g64), (2e-2 if bf16 else max(2e-5, 3 * cases.rel_err(g32, g64)))


def test_distill_reference_is_the_restatement_and_its_operands_are_exact():
    """DistillRef against tests/distill_ref.py in f64 (tau = 3 apart from fl(1 / 3)'s one rounding), and the premises: bf16-exact
    operands, 1 / tau exact for the powers of two, the hot plants in place"""
    for name in ('pixel_c19_p257', 'pixel_c19_p257_hot', 'channel_c9_hw129_b3_cap2', 'channel_c19_hw257_b3_cap0_hot', 'pixel_c8_p600'):
        kind, C, _, B, HW, cap, tau, hot = DISTILL_BY_NAME[name]
        s, t = X.distill_operands(B, C, HW, 0, hot)
        for v in (s, t):
            assert np.array_equal(torch.from_numpy(v).to(torch.bfloat16).double().numpy(), v)
            assert (np.abs(v).max() == 200.0) == hot
        ref = X.DistillRef(s, t, tau, kind, 1.0, cap)
        assert (ref.inv * tau == 1.0) == (tau != 3.0)
        nchw = lambda v: torch.from_numpy(np.ascontiguousarray(np.transpose(v, (0, 2, 1)))).reshape(B, C, HW, 1)
        loss, g = distill_ref.loss_and_grad(nchw(s), nchw(t), torch.float64, 1.0 / ref.inv, kind)
        assert abs(ref.loss * (1.0 / ref.inv / tau) ** 2 - float(loss)) <= 1e-12 * abs(float(loss))
        want = g.numpy().reshape(B, C, HW).transpose(0, 2, 1) * (ref.norm / (1.0 / ref.inv / ref.units))
        assert np.abs(ref.g - want).max() <= 1e-12 * np.abs(want).max()
        assert (ref.q > 0).any() and abs(float(ref.q.sum(ref.ax).max()) - 1) < 1e-12


def test_distill_cases_reach_what_they_are_listed_for():
    """the restated planners on the listed shapes: the pixel kind's one block walking 600 pixels and the two-block grid of 257; the
    channel kind's 1, 2, 3 and 32 vectors per row with an idle thread at 19 classes, S = 1, capped and uncapped, a block that walks
    items of two images, a ragged last segment, several trips -- and the empty item, which only the added shape has"""
    assert X.distill_pixel_grid(1) == 1 and X.distill_pixel_grid(257) == 2 and X.distill_pixel_grid(600, 1) == 1
    assert X.distill_pixel_grid(600) == 3 and X.distill_pixel_grid(10 ** 7) == X.DISTILL_PIXEL_BLOCKS
    assert [X.distill_channel_split(1, C, 1)['nch'] for C in X.DISTILL_CHANNEL_C] == [1, 2, 3, 32]
    assert X.DISTILL_NT - 3 * X.distill_channel_split(1, 19, 1)['ppb'] == 1
    seen = set()
    for C in X.DISTILL_CHANNEL_C:
        for (name, B, HW, cap, tau, hot) in X.distill_channel_cases(C):
            sp = X.distill_channel_split(B, C, HW, cap)
            segs = X.distill_segments(HW, sp['S'])
            assert sp['S'] >= 1 and sp['grid'] >= 1 and sp['grid'] <= (cap or X.DISTILL_CHANNEL_BLOCKS) and segs[-1][1] == HW
            assert sorted(i for a, b in segs for i in range(a, b)) == list(range(HW))          # every position in one segment
            empty = any(a >= b for a, b in segs)
            assert empty == name.endswith('_empty')
            full = X.cdiv(HW, sp['ppb'])
            seen.add('S1' if sp['S'] == 1 else 'capped' if sp['S'] < full else 'uncapped')
            if sp['grid'] < sp['items'] and B > 1:
                seen.add('two_images')
            if segs[-1][1] - segs[-1][0] not in (0, sp['len']):
                seen.add('ragged')
            if sp['len'] > sp['ppb']:
                seen.add('trips')
            assert X.distill_depth('channel', B, C, HW, cap) == X.cdiv(sp['len'], sp['ppb']) + (sp['ppb'] - 1).bit_length() + sp['S']
    assert seen == {'S1', 'capped', 'uncapped', 'two_images', 'ragged', 'trips'}


def test_distill_channel_split_leaves_an_empty_item_only_where_the_cap_cuts_short_segments():
    """over HW <= 4096, every vector count (C <= 256) and every S the caps 1 .. 512 can select: an item is empty exactly when
    (S - 1) ceil(HW / S) >= HW.  That needs short segments (S > 1 <= ceil(HW / ppb)): it is reachable -- first at 32 vectors per row,
    HW = 81, S = 10 -- and never with S at its uncapped value at the listed class counts' ppb >= 85"""
    HW = np.arange(1, 4097)
    first = {}
    for nch in range(1, 33):
        ppb = X.DISTILL_NT // nch
        smax = -(-HW // ppb)
        for S in range(2, 513):
            e = (S <= smax) & ((S - 1) * -(-HW // S) >= HW)
            if e.any():
                first.setdefault(nch, (int(HW[e][0]), S))
                first[nch] = min(first[nch], (int(HW[e][0]), S))
    assert first[32] == (81, 10) and all(n not in first for n in (1, 2, 3))
    segs = X.distill_segments(81, X.distill_channel_split(1, 256, 81, 10)['S'])
    assert len(segs) == 10 and segs[-1] == (81, 81) and segs[-2] == (72, 81)


@pytest.mark.parametrize('kind,C', [(k, C) for k, Cs, _ in DISTILL_KINDS for C in Cs])
def test_distill_f32_emulation_meets_every_bound(kind, C):
    """stats maxima bit for bit, log Z, loss and every gradient element of the emulated kernels within the bounds on every listed
    case, f32 and bf16 gradient.  The f32 channel-kind ratios must stay <= 1 / 2 (a bf16 gradient's bound IS its rounding, 2^-8 |g|:
    its ratio approaches 1 by construction)"""
    for case in [c for c in DISTILL_ALL if c[0] == kind and c[1] == C]:
        for bf16 in (False, True):
            r = _distill_emu(case, bf16)[4]
            print('SOFT_MARGIN_EMU %-36s %-4s max %d logz %.4f loss %.4f grad %.4f' % (case[2], 'bf16' if bf16 else 'f32', r['max'], r['logz'],
                                                                                     r['loss'], r['grad']))
            assert r['max'] and r['logz'] <= 1 and r['loss'] <= 1 and r['grad'] <= 1, (case[2], bf16, r)
            if kind == 'channel' and not bf16:
                assert max(r['logz'], r['loss'], r['grad']) <= 0.5, (case[2], r)


# (defect, case on which the elementwise bound fails while the old whole-tensor criterion passes, bf16 gradient)
DISTILL_DEFECT_CASES = (('own_max', 'channel_c8_hw770_b1_cap0', True),
                        ('drop_tail', 'channel_c19_hw257_b3_cap3', True),
                        ('drop_tail', 'channel_c9_hw386_b1_cap2', True),
                        ('fused_stats', 'pixel_c19_p257_hot', False),
                        ('fused_stats', 'channel_c19_hw257_b3_cap0_hot', False))


@pytest.mark.parametrize('defect,name,bf16', DISTILL_DEFECT_CASES)
def test_distill_emulation_with_one_defect_fails_the_elementwise_bound_where_the_old_criterion_passes(defect, name, bf16):
    case = DISTILL_BY_NAME[name]
    s, t, ref, d, r = _distill_emu(case, bf16, defect)
    err, bound = _old_gradient_criterion(case, s, t, d, bf16)
    print('defect %-12s %-34s new grad ratio %.3f logz ratio %.3f | old %.3e <= %.3e' % (defect, name, r['grad'], r['logz'], err, bound))
    assert r['grad'] > 1, (defect, name, r)
    assert err <= bound, (defect, name, err, bound)
    if defect != 'fused_stats':           # the forward's sums are wrong: the saved log Z fails its own bound too
        assert r['logz'] > 1
    s, t, ref, d, r = _distill_emu(case, bf16)
    assert r['grad'] <= 1 and _old_gradient_criterion(case, s, t, d, bf16)[0] <= bound


# --- planar focal and soft Dice
import functools                     # noqa: E402

from tests import softloss_ref       # noqa: E402

SOFT_ALPHA, SOFT_GO = 0.25, 0.7
SOFT_VARIANTS = {0: 'reference', 1: 'lin'}
SOFT_IDS = lambda s: 'x'.join(str(v) for v in s)


@functools.lru_cache(maxsize=None)
def _planar(shape, has_ignore=True):
    x, lab, plants = X.soft_planar_operands(*shape, behind=shape == X.SOFT_BEHIND)
    return x, lab, plants, X.PlanarRef(x, lab, 255, has_ignore)


def _restated(fn, x, lab, *args):
    """(f64 loss, f64 gradient times grad_out, the old criterion's f32 bound) of tests/softloss_ref.py"""
    B, C, HW = x.shape
    xt, lt = torch.from_numpy(x).reshape(B, C, HW, 1), torch.from_numpy(lab).reshape(B, HW, 1)
    l64, g64 = softloss_ref.loss_and_grad(fn, xt, lt, torch.float64, *args)
    _, g32 = softloss_ref.loss_and_grad(fn, xt, lt, torch.float32, *args)
    go = float(np.float32(SOFT_GO))
    g64 = g64.numpy().reshape(B, C, HW) * go
    d_ref = cases.rel_err(g32.numpy().reshape(B, C, HW) * go, g64) if bool(torch.isfinite(g32).all()) else None
    return float(l64), g64, (2e-5 if d_ref is None else max(2e-5, 3 * d_ref))


def _old_planar_criterion(d, g64, f32_bound, bf16):
    """tests/test_gpu_softloss.py's check on the gradient: cases.rel_err over the WHOLE tensor; (error, bound)"""
    return cases.rel_err(np.asarray(d, np.float64), g64), (2e-2 if bf16 else f32_bound)


def _half_but_last(out, ref, bound, last):
    """the f32 emulation stays at 1 / 2 of a bound whose last `last` roundings are taken out at their exact size: |out - ref| <=
    last hu(ref) + (bound - last hu(ref)) / 2, hu = half an ulp of the f32 number nearest ref.  Where ONE rounding of the stored value
    dominates (lse = m + lg at a leading target: u |lse| of a bound of u (|lse| + 1 + ...); coef = -(T1 + w) near -1 or -e: the
    exponential's and the sum's) a value just above a power of two uses u |v| in full -- half an ulp IS u |v| there -- so the plain
    ratio reaches 0.8 with nothing missing, exactly as a bf16 gradient's reaches 0.99.  What is left after those roundings must still
    fit half of what is left of the bound: a missing term would show here"""
    ref = np.asarray(ref, np.float64)
    hu = np.where(ref != 0, 2.0 ** (np.floor(np.log2(np.where(ref != 0, np.abs(ref), 1.0))) - 24), 0.0)
    err = np.abs(np.asarray(out, np.float64) - ref)
    return bool((err <= last * hu + np.maximum(bound - last * hu, 0.0) / 2 + 1e-300).all())


def test_soft_planar_cases_reach_what_they_are_listed_for():
    assert X.soft_grid(1, 2056, 0, X.SOFT_FOCAL_BLOCKS) == (2, 1) and 2056 // 8 - X.SOFT_NT == 1          # the second block: one lane
    assert 3 * (1000 // 8) == 375 and 375 % X.SOFT_NT != 0
    assert [X.cdiv(C, X.SOFT_DICE_CP) for C in (24, 25, 48, 49)] == [1, 2, 2, 3]
    assert X.soft_grid(3, 1000, 1, X.SOFT_DICE_BLOCKS) == (1, 2) and X.soft_grid(3, 1000, 2, X.SOFT_DICE_BLOCKS) == (2, 1)
    for shape in X.SOFT_PLANAR:
        B, C, HW = shape
        x, lab, plants, ref = _planar(shape)
        assert HW % 8 == 0 and np.array_equal(torch.from_numpy(x).to(torch.bfloat16).double().numpy(), x)
        assert (lab == 255).any() or HW * B <= 16
        if C >= 19:
            i0, i1, i2, i3 = (plants['gap%g' % g] for g in (0, 0.25, 16, -16))
            assert ref.valid[0, [i0, i1, i2, i3]].all()
            assert ref.lead[0, i0] and (ref.D[0, :, i0] == 0).sum() == 2                 # et == 1 with a tie: s = 2 + ...
            assert ref.lead[0, i1] and np.sort(ref.D[0, :, i1])[-2] == -0.25
            assert ref.lead[0, i2] and ref.q[0, i2] < 1e-4 and ref.pt[0, i3] < 1e-6 and not ref.lead[0, i3]
            n = ref.onehot.sum((0, 2))
            assert n[plants['absent']] == 0 and n[plants['single']] == 1
        if C == 1:
            assert (ref.q == 0).all() and ref.lead[ref.valid].all()
    _, lab, _, ref = _planar((1, 256, 16), False)
    assert ((lab == 255) <= ref.valid).all() and (lab == 255).any()                     # without an ignore index 255 is a class
    x, lab, _, ref = _planar(X.SOFT_BEHIND)
    assert ref.valid.all() and (ref.Dt == -6).all()


@pytest.mark.parametrize('shape', [(2, 2, 8), (3, 19, 1000), (1, 25, 64), X.SOFT_BEHIND], ids=SOFT_IDS)
def test_soft_planar_reference_is_the_restatement(shape):
    x, lab, _, ref = _planar(shape)
    for gamma in X.SOFT_GAMMAS:
        for variant in (0, 1):
            fr = X.FocalPlanarRef(ref, gamma, variant, SOFT_ALPHA, SOFT_GO)
            loss, g, _ = _restated(softloss_ref.focal_loss, x, lab, float(np.float32(SOFT_ALPHA)), gamma, 255, SOFT_VARIANTS[variant])
            assert abs(fr.loss - loss) <= 1e-12 * abs(loss)
            assert np.abs(fr.g * (float(np.float32(SOFT_ALPHA)) / fr.nvalid / fr.scale) - g).max() <= 1e-11 * np.abs(g).max()
    for smooth in (0.0, 1.0):
        dr = X.DicePlanarRef(ref, smooth, SOFT_GO)
        loss, g, _ = _restated(softloss_ref.dice_loss, x, lab, shape[1], smooth, 255)
        assert abs(dr.loss - loss) <= 1e-12 and np.abs(dr.g - g).max() <= 1e-12 * np.abs(g).max()


@pytest.mark.parametrize('shape', X.SOFT_PLANAR + [X.SOFT_BEHIND], ids=SOFT_IDS)
def test_soft_planar_f32_emulation_meets_every_bound(shape):
    """lse, pixel_coef, loss, scale and every gradient element of the emulated focal kernels for every gamma and both variants; lse,
    a_c, b_c, loss and every gradient element of the emulated Dice kernels for both smooth values, with and without the ignore
    index, at max_blocks 0, 1, 2; f32 and bf16 gradients"""
    x, lab, _, ref = _planar(shape)
    C = shape[1]
    for gamma in X.SOFT_GAMMAS:
        for variant in (0, 1):
            fr = X.FocalPlanarRef(ref, gamma, variant, SOFT_ALPHA, SOFT_GO)
            l, a, loss, scale = SE.focal_fwd(x, lab, gamma, variant, SOFT_ALPHA)
            assert (a[~ref.valid] == 0).all()
            for bf16 in (False, True):
                d = SE.focal_bwd(x, lab, l, a, scale, SOFT_GO, bf16)
                r = X.focal_planar_ratios(fr, l, a, loss, scale, d, bf16)
                print('SOFT_MARGIN_EMU focal %-12s g%.1f v%d %-4s' % (SOFT_IDS(shape), gamma, variant, 'bf16' if bf16 else 'f32'), r)
                assert r['scale'] and max(r['lse'], r['coef'], r['loss'], r['grad']) <= 1, (shape, gamma, variant, bf16, r)
                if not bf16:
                    assert r['loss'] <= 0.5 and r['grad'] <= 0.5, (shape, gamma, variant, r)
                    assert _half_but_last(l, fr.lse, fr.lse_bound, 1) and _half_but_last(a, fr.coef, fr.coef_bound, 2), (shape, gamma, variant, r)
    for has_ignore in (True, False):
        refd = _planar(shape, has_ignore)[3]
        for smooth in (0.0, 1.0):
            for cap in (0, 1, 2):
                dr = X.DicePlanarRef(refd, smooth, SOFT_GO, cap)
                l, coef, loss, (P, I, N) = SE.dice_fwd(x, lab, smooth, 255, has_ignore, cap)
                assert np.array_equal(N, dr.N)
                for bf16 in (False, True):
                    d = SE.dice_bwd(x, lab, l, coef, SOFT_GO, 255, has_ignore, bf16)
                    r = X.dice_planar_ratios(dr, l, coef, loss, d, bf16)
                    print('SOFT_MARGIN_EMU dice %-12s ign%d s%.0f cap%d %-4s' % (SOFT_IDS(shape), has_ignore, smooth, cap, 'bf16' if bf16 else 'f32'), r)
                    assert max(r.values()) <= 1, (shape, has_ignore, smooth, cap, bf16, r)
                    if not bf16:
                        assert max(r[k] for k in ('a', 'b', 'loss', 'grad')) <= 0.5, (shape, has_ignore, smooth, cap, r)
                        assert _half_but_last(l, dr.lse, dr.lse_bound, 1), (shape, r)


# (defect, shape, gamma, variant, bf16 gradient): the elementwise bound fails there while the old whole-tensor criterion passes
SOFT_FOCAL_DEFECT_CASES = (('q_one_minus_p', (2, 2, 8), 0.5, 1, False),           # the lead-by-16 pixel: q ~ 1e-7, 1 - p is 0 or 2^-24 steps
                           ('no_log1p', (2, 2, 8), 0.5, 1, False),                # the same pixel: log(fl(1 + so)) loses so's bits
                           ('no_second_term', X.SOFT_BEHIND, 0.5, 0, True))


@pytest.mark.parametrize('defect,shape,gamma,variant,bf16', SOFT_FOCAL_DEFECT_CASES)
def test_focal_emulation_with_one_defect_fails_the_elementwise_bound_where_the_old_criterion_passes(defect, shape, gamma, variant, bf16):
    x, lab, _, ref = _planar(shape)
    fr = X.FocalPlanarRef(ref, gamma, variant, SOFT_ALPHA, SOFT_GO)
    _, g64, f32_bound = _restated(softloss_ref.focal_loss, x, lab, float(np.float32(SOFT_ALPHA)), gamma, 255, SOFT_VARIANTS[variant])
    out = {}
    for dfc in (None, defect):
        l, a, loss, scale = SE.focal_fwd(x, lab, gamma, variant, SOFT_ALPHA, defect=dfc)
        d = SE.focal_bwd(x, lab, l, a, scale, SOFT_GO, bf16)
        out[dfc] = (X.focal_planar_ratios(fr, l, a, loss, scale, d, bf16), _old_planar_criterion(d, g64 * (fr.scale * fr.nvalid / float(np.float32(SOFT_ALPHA))), f32_bound, bf16))
        print('defect %-15s' % dfc, out[dfc])
    (r0, (e0, b0)), (r1, (e1, b1)) = out[None], out[defect]
    assert max(r0['lse'], r0['coef'], r0['loss'], r0['grad']) <= 1 and e0 <= b0
    assert r1['coef'] > 1, (defect, r1)
    assert e1 <= b1, (defect, e1, b1)


def test_dice_emulation_that_skips_the_last_group_fails_the_coefficient_bounds_where_the_old_criterion_passes():
    """375 groups, one full block and a ragged one: the statistics lose 8 of 3000 pixels, every coefficient moves by a few parts in a
    thousand and with it every gradient element -- inside 2e-2 of the largest for a bf16 gradient, far outside da, db and the
    elementwise bound"""
    shape, smooth, bf16 = (3, 19, 1000), 0.0, True
    x, lab, _, ref = _planar(shape)
    dr = X.DicePlanarRef(ref, smooth, SOFT_GO)
    _, g64, f32_bound = _restated(softloss_ref.dice_loss, x, lab, shape[1], smooth, 255)
    out = {}
    for dfc in (None, 'skip_last_group'):
        l, coef, loss, _ = SE.dice_fwd(x, lab, smooth, defect=dfc)
        d = SE.dice_bwd(x, lab, l, coef, SOFT_GO, bf16=bf16)
        out[dfc] = (X.dice_planar_ratios(dr, l, coef, loss, d, bf16), _old_planar_criterion(d, g64, f32_bound, bf16))
        print('defect %-15s' % dfc, out[dfc])
    (r0, (e0, b0)), (r1, (e1, b1)) = out[None], out['skip_last_group']
    assert max(r0.values()) <= 1 and e0 <= b0
    assert r1['a'] > 1 and r1['b'] > 1 and r1['grad'] > 1 and r1['loss'] > 1 and e1 <= b1


def test_focal_coef_emulation_meets_the_bound_and_a_leaked_coef_is_seen():
    """focal_coef_kernel's emulation on the hand-made cross-entropies (0, a denormal, 2^-24, 1, 40, 200 among multiples of 2^-4) for
    every gamma and both variants, every n with its tail group; a coef left at a pixel that does not count is not an exact 0"""
    for n in X.SOFT_CE_N:
        ce, lab = X.soft_ce_operands(n)
        assert tuple(ce[:min(n, 6)].astype(np.float64)) == tuple(np.float32(X.SOFT_CE_VALUES[:min(n, 6)]).astype(np.float64))
        for gamma in X.SOFT_GAMMAS:
            for variant in (0, 1):
                r = X.focal_coef_ref(ce, lab, 19, gamma, variant, SOFT_ALPHA)
                cf, loss, scale = SE.focal_coef_from_ce(ce, lab, 19, gamma, variant, SOFT_ALPHA)
                assert (cf[~r['valid']] == 0).all() and float(scale) == r['scale']
                assert X.worst_ratio(np.abs(cf - r['coef']), r['coef_bound']) <= 1, (n, gamma, variant)
                assert X.worst_ratio(abs(float(loss) - r['loss']), r['loss_bound']) <= 1, (n, gamma, variant)
    ce, lab = X.soft_ce_operands(1027)
    r = X.focal_coef_ref(ce, lab, 19, 2.0, 0, SOFT_ALPHA)
    assert 0 < (~r['valid']).sum() < 200 and r['nvalid'] + (~r['valid']).sum() == 1027
    cf = SE.focal_coef_from_ce(ce, lab, 19, 2.0, 0, SOFT_ALPHA, defect='leak')[0]
    assert (cf[~r['valid']] != 0).any() and X.worst_ratio(np.abs(cf - r['coef']), r['coef_bound']) == float('inf')


def test_a_coef_leaked_at_an_ignored_pixel_fails_the_exact_zero_check_where_the_old_criterion_passes():
    """the wide route on c33: tss_focal_coef_from_ce's emulation on the case's own cross-entropies (an exact 0 where the pixel does
    not count, as tss_upsample_pixel_ce_wide stores it) with the coef of those pixels left as computed -- w(q = 0) = 1 at gamma = 2,
    variant 0.  The MODE 5 instance of wide_ce_kernel gates both halves of its gradient on the label (`valid`, `inv = valid ? wsm :
    0`), which HeadRef.weights(pixw=...) restates: the leaked values never reach the gathered gradient, so the old whole-tensor
    criterion passes with error 0 and only the new per-pixel exact-0 check sees the defect.  Both halves asserted"""
    import copy
    c = X.HEAD_BY_NAME['c33']
    x, labels, _, ref = _head(c)
    ce = ref.pix.float().reshape(-1).numpy()
    lab = labels.reshape(-1).numpy()
    r = X.focal_coef_ref(ce, lab, c.C, 2.0, 0, SOFT_ALPHA)
    assert np.array_equal(r['valid'], ref.valid.reshape(-1).numpy()) and (ce[~r['valid']] == 0).all() and (~r['valid']).sum() > 5
    g = {}
    for dfc in (None, 'leak'):
        cf, _, scale = SE.focal_coef_from_ce(ce, lab, c.C, 2.0, 0, SOFT_ALPHA, defect=dfc)
        zero_ok = bool((cf[~r['valid']] == 0).all())
        within = X.worst_ratio(np.abs(cf - r['coef']), r['coef_bound']) <= 1
        g[dfc] = copy.copy(ref).weights(pixw=torch.from_numpy(cf.astype(np.float64)).reshape(labels.shape), grad_out=SOFT_GO * float(scale)).g.numpy()
        assert (zero_ok and within) == (dfc is None), (dfc, zero_ok, within)
        if dfc == 'leak':
            assert (cf[~r['valid']] == 1).all()
    old = cases.rel_err(g['leak'], g[None])
    assert old == 0.0 and old <= 2e-5 and np.abs(g[None]).max() > 0
    assert X.soft_grid(1, 8 * X.cdiv(1027, 4), 0, 4096)[0] == 2                   # 257 groups of 4: two blocks, the second of one lane


# --- soft Dice and focal on the fused head (csrc/softhead.hip)
HEAD_SOFT_EMU = HEAD_EMU + [X.HEAD_SOFT_EXTRA]
HEAD_FULL_BLOCK = ('one_lane_strip', 'no_table', 'identity', 'prod')       # W >= 256: a block with every lane live
_head_soft_refs = {}


def _head_soft(c, rare=False, ignore_index=255):
    key = (c.name, rare, ignore_index)
    if key not in _head_soft_refs:
        x, labels, _ = X.head_soft_inputs(c, rare)
        _head_soft_refs[key] = (x, labels, X.HeadRef(x, labels, ignore_index=ignore_index, weighted=False))
    return _head_soft_refs[key]


def _head_dice_emu(c, smooth, rare=False, ignore_index=255, defect=None, bf16=False):
    """(HeadDiceRef, ratios of a, b, loss, gradient; N exact; the old whole-tensor error of the gradient)"""
    x, labels, ref = _head_soft(c, rare, ignore_index)
    d = X.dice_ref(ref, smooth, SOFT_GO, c.counts())
    kw = dict(ignore_index=ignore_index, defect=defect)
    st = HE.ce_pass(x.numpy(), labels.numpy(), c.H, c.W, mode='dice_stats', **kw)['stats']
    coef, loss = HE.dice_finalize(st, c.C, smooth)
    dl = HE.ce_pass(x.numpy(), labels.numpy(), c.H, c.W, mode='dice_grad', coef=coef, grad_out=SOFT_GO, **kw)['dlow']
    dl = SE.to_bf16(dl) if bf16 else dl
    C, g = c.C, d.g.numpy()
    r = dict(a=X.worst_ratio(np.abs(coef[:C] - d.a), d.da), b=X.worst_ratio(np.abs(coef[24:24 + C] - d.b), d.db),
             loss=X.worst_ratio(abs(float(loss) - d.loss), d.loss_bound), grad=X.worst_ratio(np.abs(dl - g), d.grad_bound(bf16).numpy()))
    assert (coef[C:24] == 0).all() and (coef[24 + C:] == 0).all()
    return d, r, np.array_equal(st[2], d.N), cases.rel_err(dl.astype(np.float64), g)


def test_head_soft_cases_reach_what_they_are_listed_for():
    for c in HEAD_SOFT_EMU:
        x, labels, ref = _head_soft(c)
        if c.C >= 5:
            n = torch.zeros(c.C).scatter_add_(0, ref.t[ref.valid], torch.ones(int(ref.valid.sum())))
            assert n[1] == 0 and n[2] == 1, c                                            # an absent class, a class of one pixel
        assert X.head_cp(c.C) - c.C == {5: 15, 19: 1, 20: 0, 21: 3, 24: 0}[c.C]          # pad classes or none
    c = X.HEAD_BY_NAME['cp24']
    x, labels, ref = _head_soft(c, rare=True)
    p = torch.softmax(ref.z, 1)
    assert float(p[:, 20:].max()) < 1e-7 and not ((ref.t >= 20) & ref.valid).any() and (labels == 255).any()
    assert X.HEAD_SOFT_EXTRA.W % X.HEAD_NT == X.HEAD_NT - 1                              # one lane past the image edge
    _, labels, ref = _head_soft(c, ignore_index=None)
    assert ref.valid[labels == 255].sum() == 0 and ref.valid.sum() == ((labels >= 0) & (labels < c.C)).sum()


@pytest.mark.parametrize('c', HEAD_SOFT_EMU, ids=repr)
def test_head_dice_f32_emulation_meets_the_bounds(c):
    """the emulated statistics pass, finalize and gradient pass + gather within da, db, the loss bound and the elementwise gradient
    bound for smooth 0 and 1, with and without the ignore index, and on the rare-class operands; N_c exact; the full-block cases at
    no more than half of every bound"""
    for smooth, rare, ign in ((0.0, False, 255), (1.0, False, 255), (1.0, False, None)) + (((1.0, True, 255),) if c.C > 20 else ()):
        for bf16 in (False, True):
            d, r, n_exact, _ = _head_dice_emu(c, smooth, rare, ign, bf16=bf16)
            print('SOFT_MARGIN_EMU head_dice %-14s s%.0f rare%d ign%s %-4s' % (c.name, smooth, rare, ign, 'bf16' if bf16 else 'f32'), r)
            assert n_exact and max(r.values()) <= 1, (c, smooth, rare, ign, bf16, r)
            if c.name in HEAD_FULL_BLOCK and not bf16:
                assert max(r.values()) <= 0.5, (c, r)


# (defect, case, rare operands): the elementwise bound fails while the old whole-tensor criterion of a bf16 gradient (2e-2) passes
HEAD_DICE_DEFECTS = (('b_from_a', 'cp24', True),          # classes 20 .. 23 carry p < 1e-7: their planes are invisible next to the largest element
                     ('pad_in_S', 'near', False),
                     ('edge_N', 'edge_few', False))         # one lane past the edge: N_c moves by at most 9 of ~120


@pytest.mark.parametrize('defect,name,rare', HEAD_DICE_DEFECTS)
def test_head_dice_emulation_with_one_defect_fails_the_elementwise_bound_where_the_old_criterion_passes(defect, name, rare):
    c = X.HEAD_SOFT_EXTRA if name == 'edge_few' else X.HEAD_BY_NAME[name]
    _, r0, n0, old0 = _head_dice_emu(c, 1.0, rare, bf16=True)
    _, r1, n1, old1 = _head_dice_emu(c, 1.0, rare, defect=defect, bf16=True)
    print('defect %-9s %-9s new grad ratio %.2f (correct %.3f) | old %.3e (correct %.3e) <= 2e-2' % (defect, name, r1['grad'], r0['grad'], old1, old0))
    assert max(r0.values()) <= 1 and n0 and old0 <= 2e-2
    assert r1['grad'] > 1 and old1 <= 2e-2, (defect, r1, old1)
    if defect == 'edge_N':
        assert not n1 and r1['a'] > 1 and r1['b'] > 1


def _head_focal_emu(c, gamma, variant, defect=None, bf16=False):
    """(loss ratio, gradient ratio, scale exact, the old whole-tensor error of the gradient) of the emulated focal one-pass"""
    key = (c.name, 'focal')
    if key not in _head_soft_refs:
        x, labels, plants = X.head_soft_inputs(c, focal=True)
        _head_soft_refs[key] = (x, labels, X.HeadRef(x, labels, weighted=False), plants)
    x, labels, ref, _ = _head_soft_refs[key]
    f = X.HeadFocalRef(ref, gamma, variant, SOFT_ALPHA, SOFT_GO, c.counts())
    o = HE.ce_pass(x.numpy(), labels.numpy(), c.H, c.W, mode='focal', gamma=gamma, variant=variant, alpha=SOFT_ALPHA, grad_out=SOFT_GO, defect=defect)
    dl = SE.to_bf16(o['dlow']) if bf16 else o['dlow']
    g = f.g.numpy()
    return (X.worst_ratio(abs(float(o['loss']) - f.loss), f.loss_bound), X.worst_ratio(np.abs(dl - g), f.grad_bound(bf16).numpy()),
            float(o['inv_count']) == f.scale, cases.rel_err(dl.astype(np.float64), g))


def test_head_focal_plants_reach_every_branch():
    c = X.HEAD_BY_NAME['identity']
    x, labels, plants = X.head_soft_inputs(c, focal=True)
    ref = X.HeadRef(x, labels, weighted=False)
    assert [g for g, _, _ in plants] == [0.0, 0.25, 16.0, -16.0]
    for gap, y, xo in plants:
        z = ref.z[0, :, y, xo]
        t = int(labels[0, y, xo])
        assert bool(ref.valid[0, y, xo]) and float(z[t] - z[torch.arange(c.C) != t].max()) == gap
    assert all(len(X.head_soft_inputs(k, focal=True)[2]) == (4 if k.exact and k.h * k.w >= 4 else 0) for k in HEAD_EMU)


@pytest.mark.parametrize('c', HEAD_EMU, ids=repr)
def test_head_focal_f32_emulation_meets_the_bounds(c):
    """loss, scale and every element of the gathered gradient of the emulated focal one-pass for gamma in {0, 0.5, 2} x both variants,
    f32 and bf16 gradient; the full-block cases at no more than half of the bounds"""
    for gamma in X.SOFT_GAMMAS:
        for variant in (0, 1):
            for bf16 in (False, True):
                rl, rg, exact_scale, _ = _head_focal_emu(c, gamma, variant, bf16=bf16)
                print('SOFT_MARGIN_EMU head_focal %-14s g%.1f v%d %-4s loss %.4f grad %.4f' % (c.name, gamma, variant, 'bf16' if bf16 else 'f32', rl, rg))
                assert exact_scale and rl <= 1 and rg <= 1, (c, gamma, variant, bf16, rl, rg)
                if c.name in HEAD_FULL_BLOCK and not bf16:
                    assert rl <= 0.5 and rg <= 0.5, (c, gamma, variant, rl, rg)


# (defect, case, gamma, variant, bf16 gradient)
HEAD_FOCAL_DEFECTS = (('q_one_minus_p', 'identity', 2.0, 1, False), ('no_log1p', 'identity', 0.5, 1, False), ('no_second_term', 'h1', 0.5, 0, True))


@pytest.mark.parametrize('defect,name,gamma,variant,bf16', HEAD_FOCAL_DEFECTS)
def test_head_focal_emulation_with_one_defect_fails_the_gradient_bound_where_the_old_criterion_passes(defect, name, gamma, variant, bf16):
    """the old criterion: cases.rel_err over the whole gathered gradient <= 2e-5 (the floor of max(2e-5, 3 d_ref): the strictest it can
    be) in f32, 2e-2 in bf16"""
    c = X.HEAD_BY_NAME[name]
    old_bound = 2e-2 if bf16 else 2e-5
    rl0, rg0, _, old0 = _head_focal_emu(c, gamma, variant, bf16=bf16)
    rl1, rg1, _, old1 = _head_focal_emu(c, gamma, variant, defect=defect, bf16=bf16)
    print('defect %-15s %-9s new grad ratio %.2f (correct %.3f) | old %.3e (correct %.3e) <= %.0e' % (defect, name, rg1, rg0, old1, old0, old_bound))
    assert rg0 <= 1 and rl0 <= 1 and old0 <= old_bound
    assert rg1 > 1 and old1 <= old_bound, (defect, rg1, old1)


# --- Lovasz-Softmax: the restated pipeline of tests/exact.py (section "Lovasz-Softmax") that tests/test_gpu_lovasz_exact.py holds the kernels to
from tests import lovasz_ref         # noqa: E402

LV_IDS = lambda c: c.name


@functools.lru_cache(maxsize=None)
def _lovasz(name, has_ignore=1):
    case = X.LV_BY_NAME[name]
    x, lab, plants = X.lovasz_operands(case)
    return x, lab, plants, X.LovaszRef(x, lab, X.LV_IGNORE, has_ignore)


def test_lovasz_plan_restates_make_plan():
    """the offsets by hand at one shape, the chunk rule, and the tile counts the cases are listed for"""
    p = X.lovasz_plan(4104, 19, 4)
    assert (p['ntiles'], p['Cc'], p['last_c0']) == (2, 4, 16)
    assert p['G'] == 0 and p['partial'] == 256 and p['W'] == 256 + 512 and p['key0'] == 768 + X.up256(4 * 19 * 4104)
    plane = X.up256(4 * 4 * 4104)
    assert p['key1'] - p['key0'] == plane and p['pay0'] - p['key0'] == 2 * plane and p['hist'] - p['pay1'] == plane
    assert p['dtot'] - p['hist'] == 4 * 4 * 256 * 2 and p['tcnt'] - p['dtot'] == 4 * 4 * 256 and p['total'] - p['tcnt'] == 256
    assert X.lovasz_plan(4104, 19, 0)['Cc'] == 19 and X.lovasz_plan(4104, 19, 1)['last_c0'] == 18 and X.lovasz_plan(4104, 19, 40)['Cc'] == 19
    assert X.lovasz_plan(8 * 1024 * 2048, 19, 0)['Cc'] == 8            # the production shape sorts 8 classes at a time
    tiles = {c.name: X.lovasz_plan(c.N, c.C)['ntiles'] for c in X.LV_CASES}
    assert tiles == dict(smallest=1, one_tile=1, tile_and_group=2, three_ragged=3, carry=258, carry_batched=258, chunked=2, c256=1, all_equal=2)
    assert 4104 - 4096 == 8 and 8208 % 4096 == 16 and 2736 % 4096 != 0
    assert 1052680 == 257 * 4096 + 8 and 258 > X.LV_NT       # 257 whole tiles and one group: the second trip of the carry loops holds 2 tiles


def test_lovasz_key_is_monotonic_and_round_trips():
    rng = X.np_rng(4714)
    sample = np.concatenate([rng.uniform(0, 1, 20000), 2.0 ** rng.uniform(-149, 0, 20000), 1 - 2.0 ** rng.uniform(-24, -1, 20000)])
    f = np.unique(np.clip(sample, 0, 1).astype(np.float32)).astype(np.float64)
    lo, hi = f[f <= 0.5], 1.0 - f[f <= 0.5]                            # every f32 below the seam, and its mirror above it
    for v in (lo, hi[hi > 0.5]):
        k = X.lovasz_key(v)
        assert np.array_equal(X.lovasz_key_error(k), v)                 # round trip on values the key holds exactly
    e = np.sort(np.concatenate([sample, lo, hi]))
    k = X.lovasz_key(e).astype(np.int64)
    assert (np.diff(k) <= 0).all() and k.max() <= X.LV_KEY_MAX and k.min() >= 0      # the key falls as the error grows
    back = X.lovasz_key_error(k)
    assert (np.diff(back) >= 0).all() and (np.abs(back - e) <= 2.0 ** -24 * np.minimum(e, 1 - e) + 2.0 ** -150).all()
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    special = np.array([0.0, 2.0 ** -149, 0.5, above, 1 - 2.0 ** -24, 1.0])
    ks = X.lovasz_key(special).astype(np.int64)
    assert ks.tolist() == [X.LV_KEY_MAX, X.LV_KEY_MAX - 1, X.LV_HALF_BITS, X.LV_HALF_BITS - 2, 0x33800000, 0]       # above the seam 1 - e has twice f32's resolution of e
    assert np.array_equal(X.lovasz_key_error(ks), special)
    assert X.lovasz_key(-1e-3) == X.LV_KEY_MAX and X.lovasz_key(1 + 1e-9) == 0 and X.LV_KEY_MAX == 0x7E000000 < X.LV_DROPPED


@pytest.mark.parametrize('case', X.LV_CASES, ids=LV_IDS)
def test_lovasz_case_inputs_hold_their_conditions(case):
    """per case input: bf16-exact logits; the labels the issue lists; at least 99 % of the kept (class, pixel) keys outside the planted
    pixels have a one-key interval (so the GPU test checks them bit for bit); the planted keys; the sign branch of the backward is open
    at the 'zero' plant alone; rank 0 is foreground for class t and background for class o"""
    for h in case.has_ignore:
        x, lab, plants, ref = _lovasz(case.name, h)
        B, C, HW, N = case.B, case.C, case.HW, case.N
        flat = lab.reshape(N)
        assert HW % 8 == 0 and np.array_equal(torch.from_numpy(x).to(torch.bfloat16).double().numpy(), x)
        assert (flat[-2:] == 255).all() and (flat == 255).sum() >= 2
        if N >= 16:
            assert (flat == -1).sum() >= 3 and (flat == 300).sum() >= 2 and 0.05 < (flat == 255).mean() < 0.4
        if not case.populated:
            assert ref.G[1] == 0 and (ref.G == 1).sum() >= 1              # an absent class, a class of one pixel
        spots = sorted(plants.values())
        free = np.ones(N, bool)
        free[spots] = False
        ok = ref.one_key()[:, free & ref.kept]
        print('lovasz %-14s ign%d one-key fraction %.6f of %d' % (case.name, h, ok.mean() if ok.size else 1.0, ok.size))
        assert ok.size == 0 or ok.mean() >= 0.99
        opened = np.argwhere(ref.open_sign())
        assert opened.tolist() == ([[0, plants['zero']]] if 'zero' in plants else []), opened[:4]
        if 'zero' in plants:
            assert ref.e[0, plants['zero']] == 0 and ref.key[0, plants['zero']] == X.LV_KEY_MAX
        if 'one' in plants:
            i, o = plants['one'], int(np.argmax(x[0, :, plants['one']]))
            assert ref.e[0, i] == 1 and ref.key[0, i] == 0 and ref.fg[0, i] and (ref.key[0] == 0).sum() == 1          # U0 = G
            assert ref.e[o, i] == 1 and ref.key[o, i] == 0 and not ref.fg[o, i] and (ref.key[o] == 0).sum() == 1      # U0 = G + 1
            assert ref.G[0] > 0 and (ref.G[o] > 0 or (C == 2 and not case.populated) or (C == 256 and h == 1 and o == 255))
        if case.equal:
            assert (ref.e == 0.5).all() and (ref.key[:, ref.kept] == X.LV_HALF_BITS).all() and ref.G.min() > 1000
    if case.name == 'c256':
        assert _lovasz('c256', 1)[3].G[255] == 0 and _lovasz('c256', 0)[3].G[255] >= 2 and _lovasz('c256', 0)[3].kept.all()


def _oracle_loss_and_grad(x, lab, C, ignore, variant, key_order):
    """tests/lovasz_ref.py in f64: lovasz_softmax_loss(..., stable=True) and its autograd gradient.  key_order: the same lines of that
    function (class_errors, a stable descending sort, lovasz_weights, the mean) with the sort taken on the errors AT THE KEY'S RESOLUTION
    -- key_error(key(e)) -- which is the kernel's documented tie rule: errors that differ below 2^-24 keep ascending pixel index"""
    B, _, HW = x.shape
    xt = torch.from_numpy(x).reshape(B, C, HW, 1).clone().requires_grad_(True)
    lt = torch.from_numpy(lab).reshape(B, HW, 1)
    if not key_order:
        loss = lovasz_ref.lovasz_softmax_loss(xt, lt, C, ignore, variant, stable=True)
    else:
        losses = []
        for _c, errors, fg in lovasz_ref.class_errors(xt, lt, C, ignore):
            q = torch.from_numpy(X.lovasz_key_error(X.lovasz_key(errors.detach().numpy())))
            idx = torch.sort(q, dim=0, descending=True, stable=True)[1]
            losses.append(torch.dot(errors[idx], lovasz_ref.lovasz_weights(fg[idx], variant)))
        loss = torch.stack(losses).mean() if losses else xt.sum() * 0
    loss.backward()
    return float(loss.detach()), xt.grad.numpy().reshape(B, C, HW)


@pytest.mark.parametrize('variant', (0, 1))
@pytest.mark.parametrize('case', X.LV_SMALL, ids=LV_IDS)
def test_lovasz_restated_pipeline_is_the_oracle_pinned_restatement(case, variant):
    """X.lovasz_pipeline (keys, stable order, closed-form weights, tile sums, backward formula) against tests/lovasz_ref.py's loss and
    autograd gradient in f64, stable order.  The pipeline reads every error back from its f32 key (2^-24 relative to min(e, 1 - e)) and
    stores the weights in f32 (2^-24), the oracle keeps both in f64: the loss within 2^-22, every gradient element within 2^-22 of
    p (w + sum_c p_c w_c) / present.  Where the f32 keys order the kept pixels exactly as the f64 errors do, the oracle is
    lovasz_softmax_loss(..., stable=True) itself; on the larger cases two pixels whose logits are permutations of each other have
    errors one f64 ulp apart and ONE key, and the oracle sorts at the key's resolution (_oracle_loss_and_grad)"""
    for h in case.has_ignore:
        x, lab, plants, ref = _lovasz(case.name, h)
        B, C, HW = x.shape
        same = all(np.array_equal(np.argsort(ref.key[c][ref.kept], kind='stable'), np.argsort(-ref.e[c][ref.kept], kind='stable')) for c in range(C))
        assert same or case.N > 16
        out = X.lovasz_pipeline(x, lab, variant, X.LV_IGNORE, h, grad_out=None, ref=ref)
        l64, g64 = _oracle_loss_and_grad(x, lab, C, X.LV_IGNORE if h else None, lovasz_ref.VARIANTS[variant], not same)
        assert out['present'] == int((ref.G > 0).sum())
        assert abs(out['loss'] - l64) <= 2.0 ** -22 * abs(l64)
        _, T = X.lovasz_bwd_ref(ref, out['W'], out['present'], None)
        T = T.reshape(C, B, HW).transpose(1, 0, 2)
        r = X.worst_ratio(np.abs(out['grad'] - g64), 2.0 ** -22 * T + 1e-300)
        print('lovasz %-14s v%d ign%d loss %.9f | gradient vs the oracle restatement, ratio %.3f%s' % (case.name, variant, h, l64, r, '' if same else ' (key order)'))
        assert r <= 1


def test_lovasz_closed_form_weights_are_lovasz_refs_formula():
    rng = X.np_rng(4715)
    for n, pfg in ((1, 1.0), (7, 0.5), (5000, 0.1), (5000, 0.9)):
        fg = rng.uniform(size=n) < pfg
        fg[0] = True
        for first in (True, False):
            if n > 1:
                fg[0], fg[1] = first, True
            for variant in (0, 1):
                g, G = X.lovasz_weights(fg, np.ones(n, bool), variant)
                want = lovasz_ref.closed_form_weights(torch.from_numpy(fg), lovasz_ref.VARIANTS[variant]).numpy()
                assert G == fg.sum() and np.array_equal(g, want), (n, first, variant)       # the same IEEE operations: the same bits
    g, G = X.lovasz_weights(np.zeros(9, bool), np.ones(9, bool), 0)
    assert G == 0 and (g == 0).all()


def test_lovasz_final_tree_and_a_broken_carry_are_seen():
    """lovasz_final on rows it can sum exactly; and what a dropped `carry += tot` of the offset scan does to a 257-tile plane: tile 256's
    elements land on tile 0's, which a permutation check sees"""
    part = np.arange(2 * 300, dtype=np.float64).reshape(2, 300)
    loss, present = X.lovasz_final(part, np.array([3, 0]))
    assert present == 1 and loss == np.float32(part[0].sum())
    loss, present = X.lovasz_final(part, np.array([0, 0]))
    assert present == 0 and loss == 0
    v = np.arange(64, dtype=np.float64)[None, :] * np.ones((4, 1))
    assert (X.wave_sum_lane0(v) == 2016).all()


# --- planar cross-entropy and OHEM (tests/test_gpu_planar_ce_exact.py)
from tests import softloss_emu       # noqa: E402


def _planar_ce_emu(shape, bf16=False, defect=None):
    """ce_fwd_kernel / ohem_pixel_kernel and ce_bwd_kernel in f32 (tests/softloss_emu.py: lse8, expf): (lse, per-pixel loss, gradient with
    w = fl(fl(1 / n) 0.7)).  defect 'last_plane': grad8 leaves the last class plane as the plane before it"""
    x, lab, plants = X.planar_ce_operands(shape)
    ref = X.PlanarRef(x, lab, 255, True)
    x32 = x.astype(np.float32)
    lse = softloss_emu.lse8(x32)
    xt = np.take_along_axis(x32, ref.t[:, None, :], 1)[:, 0]
    pix = np.where(ref.valid, np.maximum(lse - xt, np.float32(0)), np.float32(0))
    gs = np.float32(1.0 / ref.nvalid) * np.float32(0.7)
    w = np.where(ref.valid, gs, np.float32(0))
    g = (softloss_emu.expf(x32 - lse[:, None]) - ref.onehot.astype(np.float32)) * w[:, None]
    if defect == 'last_plane':
        g[:, -1] = g[:, -2]
    if bf16:
        g = softloss_emu.to_bf16(g)
    return x, lab, plants, ref, X.PlanarCeRef(ref), lse, pix, g.astype(np.float64), float(gs)


@pytest.mark.parametrize('shape', X.PLANAR_CE_SHAPES[:-1], ids=SOFT_IDS)
def test_planar_ce_f32_emulation_meets_every_bound(shape):
    """lse, the per-pixel loss and every gradient element of an f32 evaluation in the kernels' order stay inside the bounds the GPU test
    uses; the planted 'exact' pixel stores lse == x_t and a loss of +0; the 2^-8 of a bf16 gradient is enough"""
    for bf16 in (False, True):
        x, lab, plants, ref, cr, lse, pix, g, gs = _planar_ce_emu(shape, bf16)
        want, bound = cr.grad(np.where(ref.valid, gs, 0.0), bf16)
        r = (X.worst_ratio(np.abs(lse - cr.lse), cr.lse_bound), X.worst_ratio(np.abs(pix - cr.ce), cr.ce_bound), X.worst_ratio(np.abs(g - want), bound))
        print('planar CE emulation %-12s bf16 %d: lse %.3f pixel loss %.3f gradient %.3f' % ((SOFT_IDS(shape), bf16) + r))
        assert max(r) <= 1
        assert not np.signbit(pix).any() and (pix[~ref.valid] == 0).all()
        if 'exact' in plants:
            i = plants['exact']
            assert ref.valid[0, i] and lse[0, i] == x[0, 0, i] == 16 and pix[0, i] == 0 and 0 < cr.ce[0, i] < 1e-11
    assert abs(float(pix.astype(np.float64).sum()) - cr.total) <= cr.total_bound


def test_planar_ce_big_shape_takes_a_second_trip():
    B, C, HW = X.PLANAR_CE_BIG
    groups = B * (HW // 8)
    assert X.soft_grid(B, HW, 0, 4096) == (4096, 2) and groups == 4097 * X.SOFT_NT      # block 0 alone goes round twice


def test_planar_ce_emulation_that_repeats_a_class_plane_fails_the_elementwise_bound():
    """grad8 writing plane C - 2 once more in place of the last one of 19: the elementwise bound sees it in f32 and bf16 alike (on the GPU
    a plane that is skipped outright stays NaN, which the harness sees before any bound)"""
    shape = (3, 19, 1000)
    for bf16 in (False, True):
        x, lab, plants, ref, cr, lse, pix, g, gs = _planar_ce_emu(shape, bf16, defect='last_plane')
        want, bound = cr.grad(np.where(ref.valid, gs, 0.0), bf16)
        assert X.worst_ratio(np.abs(g - want), bound) > 1


# --- the two sort mutations that are not run on a device (their unwritten slots end as payloads that index past W): in numpy
def _lovasz_sort_emu(keys, pay, defect=None):
    """the 4 LSD passes of csrc/lovasz.hip (hist, digit totals, the offset scan with its carry loop over NT tiles at a time, the scatter
    with a rank among equal digits of the tile) on one class plane.  The destination starts as 0xFFFFFFFF, as the GPU test's workspace
    does, with spare slots behind it for a position past the end.  Defects: 'carry' drops the `carry += tot` of lovasz_offset_kernel;
    'below' forms the scatter's `below` with the lane's own bit set, so that no lane ever updates the wave's running count"""
    N = keys.size
    ntiles = X.cdiv(N, X.LV_TILE)
    idx = np.arange(N)
    tile = idx // X.LV_TILE
    k, q = keys.copy(), pay.copy()
    for shift in (0, 8, 16, 24):
        d = ((k >> np.uint32(shift)) & np.uint32(255)).astype(np.int64)
        hist = np.zeros((256, ntiles), np.int64)
        np.add.at(hist, (d, tile), 1)
        dtot = hist.sum(1)
        carry, offs = np.cumsum(dtot) - dtot, np.empty_like(hist)
        for i0 in range(0, ntiles, X.LV_NT):
            seg = hist[:, i0:i0 + X.LV_NT]
            offs[:, i0:i0 + X.LV_NT] = carry[:, None] + np.cumsum(seg, 1) - seg
            if defect != 'carry':
                carry = carry + seg.sum(1)
        group = (tile if defect != 'below' else idx // 64) * 256 + d        # equal digits of a tile; of one wave round under 'below'
        order = np.argsort(group, kind='stable')
        gs = group[order]
        start = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]])
        rank = np.empty(N, np.int64)
        rank[order] = idx - np.repeat(start, np.diff(np.r_[start, N]))
        pos = offs[d, tile] + rank + (1 if defect == 'below' else 0)
        assert pos.max() < N + 64
        k2, q2 = np.full(N + 64, X.LV_DROPPED, np.uint32), np.full(N + 64, X.LV_DROPPED, np.uint32)
        k2[pos], q2[pos] = k, q
        if defect is None:
            k, q = k2[:N], q2[:N]
        else:
            return k2[:N], q2[:N], int(pos.max())                # one broken pass is enough
    return k, q, N - 1


def _is_permutation(pay, N):
    pix = (pay & np.uint32(0x7FFFFFFF)).astype(np.int64)
    return pix.max() < N and np.array_equal(np.bincount(pix, minlength=N), np.ones(N, np.int64))


def test_lovasz_sort_emulation_and_the_two_mutations_that_are_not_run_on_a_device():
    """the emulated passes give the stable argsort; without the offset scan's `carry += tot` nothing changes up to 256 tiles (every case of
    tests/test_gpu_lovasz.py) and pay0 stops being a permutation at 258 (the `carry` case); with the lane's own bit in `below` it stops
    being one on a single tile, and the last position lies one past the plane.  In both, slots stay unwritten, which on a device hold
    whatever was there before: a payload that the weight kernel would use as an index.  So these two are shown here and not run there"""
    x, lab, plants, ref = _lovasz('three_ragged')
    keys = ref.key[0]
    pay = np.arange(keys.size, dtype=np.uint32) | (ref.fg[0].astype(np.uint32) << np.uint32(31))
    k, q, _ = _lovasz_sort_emu(keys, pay)
    order, want = X.lovasz_order(keys, ref.fg[0])
    assert np.array_equal(q, want) and np.array_equal(k, keys[order])
    k1, q1, _ = _lovasz_sort_emu(keys, pay, 'carry')
    k0, q0, last = _lovasz_sort_emu(keys, pay, 'below')
    assert _is_permutation(q1, keys.size) and not _is_permutation(q0, keys.size)
    assert last == keys.size                                                          # the run of ignored pixels ends the plane: one past it
    x, lab, plants, ref = _lovasz('carry')
    keys = ref.key[0]
    pay = np.arange(keys.size, dtype=np.uint32) | (ref.fg[0].astype(np.uint32) << np.uint32(31))
    head = 256 * X.LV_TILE
    assert _is_permutation(_lovasz_sort_emu(keys[:head], pay[:head], 'carry')[1], head)         # 256 tiles: one trip, the carry is never used
    k1, q1, _ = _lovasz_sort_emu(keys, pay, 'carry')
    assert not _is_permutation(q1, keys.size) and (q1 == np.uint32(X.LV_DROPPED)).any()         # 258 tiles: tiles 256, 257 land on tiles 0, 1
