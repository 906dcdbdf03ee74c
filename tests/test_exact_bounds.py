"""The exact-operand method of tests/exact.py checked on the CPU (no GPU): its premise (the on-load transforms are exact in f32), the
soundness of its bounds (an f32 emulation of each convolution from the same bf16 operands passes) and their sharpness (the same emulation
with one realistic kernel defect fails)."""
import pytest
import torch

from tests import exact as X


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
