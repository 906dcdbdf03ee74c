"""Exact-operand f64 references for the bf16 convolution kernels (tests/test_exact_bounds.py, tests/test_gpu_zoo_exact.py).

Every operand is a DYADIC bf16 value, +-(1 + k/128) * 2^e with e in [-4, 2): 8 significant bits.  BatchNorm scales are powers of two in
[1/2, 4], the backward pair (ga, gb) powers of two in [1/4, 2] and [2^-6, 2^-3].  Then the on-load transforms of the kernels

    a = relu?((x - mean) * scale + bias)       computed folded as  x * scale + (bias - mean * scale)
    g = ga (e - gce) + gb (y - gmu)            computed folded as  ga * e + gb * y + (-(ga gce) - gb gmu)

are EXACT in f32 whatever the operation order: every product is a power-of-two shift, and the widest sum spans 2^5 .. 2^-17, i.e. fewer
than 24 bits.  The only rounding before the MFMA is then the f32 -> bf16 conversion (round to nearest even), which the helpers below
reproduce bit for bit.  What is left between a kernel and the f64 reference is its f32 accumulation order and the final bf16 rounding,
which the bounds below cover as worst cases, elementwise.

Unit roundoff: u = 2^-24 for f32, 2^-9 for bf16 (half an ulp of an 8-bit significand).  For n terms summed in f32 in ANY order (a chain,
a tree, MFMA partial sums, atomics) |fl(sum) - sum| <= gamma_n * sum|terms| with gamma_n = n u / (1 - n u) <= 2 n u = 2^-23 n for
n u <= 1/2, n the longest chain of roundings a term goes through."""
import math

import torch

U32 = 2.0 ** -24
SENTINEL_BITS = 0x3F5A          # a finite bf16 (0.85156) no kernel writes by accident: untouched pitch padding / spare rows keep it


# ---------------------------------------------------------------------------------------------------------- operands
def dyadic(shape, gen, emin=-4, emax=2, zero_frac=0.0):
    """+-(1 + k/128) 2^e, k in [0, 128), e in [emin, emax) as f64 (exactly representable in bf16); a fraction of exact zeros"""
    k = torch.randint(0, 128, shape, generator=gen).double()
    e = torch.randint(emin, emax, shape, generator=gen).double()
    s = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    v = s * (1 + k / 128) * torch.pow(2.0, e)
    if zero_frac > 0:
        v = torch.where(torch.rand(shape, generator=gen, dtype=torch.float64) < zero_frac, torch.zeros_like(v), v)
    return v


def pow2(shape, gen, lo, hi):
    """powers of two 2^e, e uniform in [log2 lo, log2 hi]"""
    e = torch.randint(int(math.log2(lo)), int(math.log2(hi)) + 1, shape, generator=gen).double()
    return torch.pow(2.0, e)


def rne_bf16(v):
    """round f64 values that are exact in f32 to bf16 (nearest even), as the kernels' (bf16_t)f does, back as f64"""
    f = v.float()
    assert torch.equal(f.double(), v), 'operand not exact in f32: the dyadic premise is broken'
    return f.to(torch.bfloat16).double()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


SENTINEL_BITS32 = 0x3F5A5A5A    # the same for f32 buffers


def sentinel(shape, device='cpu', dtype=torch.bfloat16):
    if dtype == torch.float32:
        return torch.full(shape, SENTINEL_BITS32, dtype=torch.int32, device=device).view(torch.float32)
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int16, device=device).view(torch.bfloat16)


def act(x, mean=None, scale=None, bias=None, relu=False):
    """the activated operand: f64 transform (exact), ReLU, bf16 rounding"""
    a = x
    if scale is not None:
        a = (x - mean) * scale + bias
    if relu:
        a = a.clamp_min(0.0)
    return rne_bf16(a)


def pre_act(x, mean, scale, bias):
    return (x - mean) * scale + bias if scale is not None else x


def gcomb(e, y=None, ga=None, gb=None, gce=None, gmu=None):
    """the backward operand: ga (e - gce) + gb (y - gmu) (or ga e, or e) in f64 (exact), bf16 rounding"""
    if y is not None:
        return rne_bf16(ga * (e - gce) + gb * (y - gmu))
    if ga is not None:
        return rne_bf16(ga * e)
    return e


def plant_zeros(x, mean, scale, bias, gen, frac=0.03):
    """set a fraction of x to mean - bias / scale where that is a dyadic bf16 value: the pre-activation is an exact 0 there"""
    z = mean - bias / scale
    ok = rne_bf16(z.expand_as(x).float().double()).eq(z.expand_as(x))
    pick = (torch.rand(x.shape, generator=gen, dtype=torch.float64) < frac) & ok
    assert x.numel() < 2000 or bool(pick.any()), 'no exact zero planted'
    return torch.where(pick, z.expand_as(x), x)


# ---------------------------------------------------------------------------------------------------------- layouts
def nhwc_to_nchw(t, B, H, W, C):
    return t[:B * H * W, :C].reshape(B, H, W, C).permute(0, 3, 1, 2)


def nchw_to_rows(t):
    B, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * H * W, C)


# ---------------------------------------------------------------------------------------------------------- bounds
def conv_excess(out, ref, S, K):
    """forward / backward-data / transposed: |out - ref| <= 2^-8 |ref| + 2^-22 K S elementwise (S includes |bias|).
    The kernel's f32 sum v of K products (exact: 8 x 8-bit significands) and the bias obeys |v - ref| <= gamma_(K+1) S <= 2^-23 (K+1) S; the
    bf16 rounding adds at most 2^-9 |v| <= 2^-9 (|ref| + 2^-23 (K+1) S).  Together <= 2^-9 |ref| + 2^-22 K S for K >= 2 -- the bound
    keeps a factor 2 on the |ref| term, which no rounding consumes.  Returns max(|out - ref| - bound) (<= 0: within the bound)."""
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -22 * K * S
    return ((out - ref).abs() - bound).max().item()


def wgrad_excess(dw, ref, S, chain):
    """weight gradient (per-block f32 partial rows + their f32 reduction): |dW - ref| <= gamma_chain S <= 2^-23 chain S"""
    return ((dw - ref).abs() - 2.0 ** -23 * chain * S).max().item()


def sweep_chain(P, PT, rows):
    """longest rounding chain of one sweep kernel + tss_dw_reduce_many: a block owns ceil(ceil(P / PT) / rows) stages of PT pixels,
    each pixel one product per accumulator (MFMA partial sums round at most once per product), then rows - 1 additions of the other
    blocks' rows and one into the zeroed gradient"""
    per = -(-(-(-P // PT)) // rows)
    return per * PT + rows


def stats_excess(slab_sum, terms, chain):
    """statistics slabs from the STORED output bits: each term (a bf16 value, or a product of one with an exact f32 difference: at most
    16 + 8 significant bits) is exact in f32; a lane adds its terms in f32 (chain: the longest such chain plus the in-wave tree), the
    block and slab sums are f64 (2^-50 covers them).  |sum - f64 sum of the terms| <= (2^-23 chain + 2^-50) sum|terms|"""
    ref = terms.sum(0)
    bound = (2.0 ** -23 * chain + 2.0 ** -50) * terms.abs().sum(0)
    return ((slab_sum - ref).abs() - bound).max().item()


def cdiv(a, b):
    return -(-a // b)


def lean_stats_chain(rows, W, MT, RPB, parities=1):
    """f32 chain of one lane's statistics in a row-tiled lean kernel (fc1d, fcg, sconv): block-tiles are (RPB image rows, 16 MT
    columns), nblk of them; the grid is min(256 x blocks per CU (>= 1), 512, nblk) >= min(256, nblk) blocks, each looping over
    ceil(nblk / grid) tiles in which a lane adds MT pixels (m * 16 + fr), then row16_sum's 4 levels (the block's waves meet in f64).
    parities = 2: sconv's backward, whose tiles are one column parity of a row (W = its ceil(Win / 2) pixels)"""
    nblk = cdiv(rows, RPB) * parities * cdiv(W, 16 * MT)
    return cdiv(nblk, min(256, nblk)) * MT + 4


def generic_stats_chain(P, ND):
    """the same for convgemm_kernel: 128-pixel tiles, 8 XCD ranges of ceil(ntiles / 8) tiles each shared by gs = min(ceil(ntiles / 8),
    max(1, 64 / nchunks)) blocks; a lane adds 4 pixels per tile, then 4 shuffle levels (the two pixel halves meet in f64)"""
    ntiles = cdiv(P, 128)
    per = cdiv(ntiles, 8)
    gs = max(1, min(per, max(1, 64 // cdiv(ND, 128))))
    return 4 * cdiv(per, gs) + 4


def generic_wgrad_chain(P, K, N, ntaps):
    """wgrad_kernel (the generic bf16 weight gradient): 64-pixel stages, ns = clamp(1024 / tiles, <= ceil(nstage / 8), >= 1) blocks per
    output tile, each owning ceil(nstage / ns) stages; a product per pixel, the block's 4 waves combined, ns f32 atomics onto dw"""
    tiles = cdiv(N, 128) * cdiv(K, 128) * ntaps
    nstage = cdiv(P, 64)
    ns = max(1, min(max(1, 1024 // tiles), cdiv(nstage, 8)))
    return cdiv(nstage, ns) * 64 + 4 + ns


# ---------------------------------------------------------------------------------------------------------- references
def conv_ref(a, w, stride=1, padding=0, dilation=1):
    """(reference, its absolute twin) of conv2d in f64"""
    F = torch.nn.functional
    return (F.conv2d(a, w, stride=stride, padding=padding, dilation=dilation),
            F.conv2d(a.abs(), w.abs(), stride=stride, padding=padding, dilation=dilation))


def conv_input_ref(shape, w, g, stride=1, padding=0, dilation=1):
    G = torch.nn.grad
    return (G.conv2d_input(shape, w, g, stride=stride, padding=padding, dilation=dilation),
            G.conv2d_input(shape, w.abs(), g.abs(), stride=stride, padding=padding, dilation=dilation))


def conv_weight_ref(a, wshape, g, stride=1, padding=0, dilation=1):
    G = torch.nn.grad
    return (G.conv2d_weight(a, wshape, g, stride=stride, padding=padding, dilation=dilation),
            G.conv2d_weight(a.abs(), wshape, g.abs(), stride=stride, padding=padding, dilation=dilation))


def convT_ref(x, w, stride=2, padding=1, output_padding=1):
    F = torch.nn.functional
    return (F.conv_transpose2d(x, w, stride=stride, padding=padding, output_padding=output_padding),
            F.conv_transpose2d(x.abs(), w.abs(), stride=stride, padding=padding, output_padding=output_padding))


def tap_geom(T, axis, dil):
    """(kernel shape, padding, dilation) of a T-tap layer along W (axis 0) or H (axis 1), padding = dilation (T - 1) / 2"""
    p = dil * (T - 1) // 2
    return ((1, T), (0, p), (1, dil)) if axis == 0 else ((T, 1), (p, 0), (dil, 1))
