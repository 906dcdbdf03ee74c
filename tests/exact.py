"""Exact-operand f64 references for the bf16 convolution kernels (tests/test_exact_bounds.py, tests/test_gpu_zoo_exact.py,
tests/test_gpu_dw_exact.py, tests/test_gpu_pw_exact.py, tests/test_gpu_dense_exact.py), for the resample, pyramid and gate kernels
(tests/test_gpu_resample_exact.py: a section of its own, with its own tiers) and for the eval bottleneck kernel, the frozen-BatchNorm
affines and the joins (tests/test_gpu_bneck_exact.py), and for the fused decoder head (tests/test_gpu_head_exact.py: the last section of
this file, with its own tiers, f64 reference and counted bounds).  The bottleneck section's tiers and cases:
  bottleneck tier 1   bit for bit on fixed-point operands (multiples of 2^-2, power-of-two scales, stage grids 2^-4 / 2^-6 / 2^-8), the
                      budget asserted per case (bneck_exact); BK_TIER1: 8 x 16 (2 cases), 8 x 8 (3), 4 x 8 (9) at stride 1 with an f32 E,
                      4 x 16 at stride 2 with a bf16 E (6); bf16 weight copies given, absent, and misaligned with other values
  bottleneck tier 2   8-bit dyadic operands, ordinary BatchNorm values through tss_bn_eval_affine_batched; BK_TIER2 (6 cases, every
                      form) within the running error bound bneck_ref carries
  BK_REFUSED          shapes the entry refuses, among them the stride-2 (128, 768, 128) whose only tile form does not fit the LDS
  affines             mean bit for bit, invstd within 3 u, scale within 4 u (affine_ref); batched == single
  joins               forward bit for bit (every branch and the sum exact in f32); backward e bit for bit and the statistics rows
                      within stats_excess with join_stats_chain, rows in use against join_geometry
The BatchNorm finalize chain (tss_bn_finalize, tss_bn_bwd_finalize, tss_slab_reduce and the _sync pair), tss_tensor_stats, tss_bias_grad
and tss_cast_weights (tests/test_gpu_bnfin_exact.py) have the last section of this file: numpy restatements of the kernels' f64 formulas
whose last steps are IEEE float32 operations, integer slab rows on which every output but invstd is held bit for bit (invstd: one f32
rounding of an f64 value), a bounded tier whose slabs tss_tensor_stats writes from stored values near 30, and the restated grids and
chains of the statistics and column-sum kernels.  The dropout masks are predicted by tests/philox_ref.py (Philox4x32-10 in numpy).
The last two sections restate the Lovasz-Softmax path (csrc/lovasz.hip: planner, key, stable order, integer weights, tile sums, final
tree, backward; tests/test_gpu_lovasz_exact.py) and carry the bounds of the planar cross-entropy and OHEM kernels
(tests/test_gpu_planar_ce_exact.py).

Every operand is a DYADIC bf16 value, +-(1 + k/128) * 2^e with e in [-4, 2): 8 significant bits.  BatchNorm scales are powers of two in
[1/2, 4], the backward pair (ga, gb) powers of two in [1/4, 2] and [2^-6, 2^-3].  Then the on-load transforms of the kernels

    a = relu?((x - mean) * scale + bias)       computed folded as  x * scale + (bias - mean * scale)
    g = ga (e - gce) + gb (y - gmu)            computed folded as  ga * e + gb * y + (-(ga gce) - gb gmu)

are EXACT in f32 whatever the operation order: every product is a power-of-two shift, and the widest sum spans 2^5 .. 2^-17, i.e. fewer
than 24 bits.  The only rounding before the MFMA is then the f32 -> bf16 conversion (round to nearest even), which the helpers below
reproduce bit for bit.  What is left between a kernel and the f64 reference is its f32 accumulation order and the final bf16 rounding,
which the bounds below cover as worst cases, elementwise.

Unit roundoff: u = 2^-24 for f32, 2^-8 for bf16 (half an ulp of an 8-bit significand, relative to the value).  For n terms summed in f32 in ANY order (a chain,
a tree, MFMA partial sums, atomics) |fl(sum) - sum| <= gamma_n * sum|terms| with gamma_n = n u / (1 - n u) <= 2 n u = 2^-23 n for
n u <= 1/2, n the longest chain of roundings a term goes through.

The depthwise 3x3 family (csrc/dwconv.hip, dwroll.hip, updw.hip; tests/test_gpu_dw_exact.py) does not feed the matrix unit: its
activated operand a and backward operand g stay f32 and its weights are f32.  Its references therefore use the UNROUNDED f64 a and g
(act_f32 / gcomb_f32, still exact in f32 under the dyadic premise), its products are no longer exact (24 x 8 bits forward, up to
24 x 24 in the weight gradient: one more rounding per term unless the compiler contracts it into an FMA, which no bound relies on), and
the chain helpers at the end of this file restate each kernel's planner.  tss_updw_* rounds the interpolated pixel to bf16 as the
materialised upsampled tensor would have been: bilinear_ref / upsampled_operand."""
import math

import numpy as np
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


def exact_f32(v):
    """v (f64) as it is, after checking that f32 holds it exactly (the dyadic premise of the unrounded operands)"""
    assert torch.equal(v.float().double(), v), 'operand not exact in f32: the dyadic premise is broken'
    return v


def act_f32(x, mean=None, scale=None, bias=None, relu=False):
    """the activated operand of the depthwise kernels: the f64 transform (exact in f32) and ReLU, NOT rounded to bf16"""
    a = pre_act(x, mean, scale, bias)
    if relu:
        a = a.clamp_min(0.0)
    return exact_f32(a)


def gcomb_f32(e, y=None, ga=None, gb=None, gce=None, gmu=None):
    """the backward operand of the depthwise kernels: ga (e - gce) + gb (y - gmu) (or ga e, or e), exact in f32, NOT rounded"""
    if y is not None:
        return exact_f32(ga * (e - gce) + gb * (y - gmu))
    if ga is not None:
        return exact_f32(ga * e)
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
    bf16 rounding adds at most 2^-8 |v| <= 2^-8 (|ref| + 2^-23 (K+1) S).  Together <= 2^-8 |ref| + 2^-22 K S for K >= 2.
    Returns max(|out - ref| - bound) (<= 0: within the bound).
    Depthwise kernels (K = 9 taps, f32 weights, f32 a / g): a product is rounded too, so a term goes through at most 1 + 9 roundings
    (2 K = 18 if every partial sum of a split accumulation is counted): |v - ref| <= gamma_18 S, and rounding v to bf16 (8 significant
    bits: half an ulp is at most 2^-8 |v|) adds <= 2^-8 |ref| + 2^-8 gamma_18 S.  Together <= 2^-8 |ref| + gamma_18 (1 + 2^-8) S, and
    gamma_18 (1 + 2^-8) = 18 u (1 + 2^-8) / (1 - 18 u) < 2^-24 18.1 < 2^-22 9: conv_excess(out, ref, S, 9) still holds, with nothing
    to spare on the |ref| term (a result off by one bf16 ulp where the exact value is not near a tie fails)."""
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -22 * K * S
    return ((out - ref).abs() - bound).max().item()


def f32_excess(out, ref, S, K):
    """an f32 instance of a depthwise kernel (f32 activations, nothing rounded to bf16): |out - ref| <= gamma_2K S <= 2^-22 K S"""
    return ((out - ref).abs() - 2.0 ** -22 * K * S).max().item()


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
    return stats_excess_sums(slab_sum, terms.sum(0), terms.abs().sum(0), chain)


def stats_excess_sums(slab_sum, tsum, tabs, chain):
    """stats_excess from the column sums of the terms and of their magnitudes (accumulated over row blocks of a large tensor)"""
    return ((slab_sum - tsum).abs() - (2.0 ** -23 * chain + 2.0 ** -50) * tabs).max().item()


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


def generic_wgrad_chain(P, K, N, ntaps, pt=64):
    """wgrad_kernel (the generic bf16 weight gradient): 64-pixel stages, ns = clamp(1024 / tiles, <= ceil(nstage / 8), >= 1) blocks per
    output tile, each owning ceil(nstage / ns) stages; a product per pixel, the block's 4 waves combined, ns f32 atomics onto dw.
    pt = 32: the f32 instance's stages (its products of two f32 operands round too: the caller doubles the chain)"""
    tiles = cdiv(N, 128) * cdiv(K, 128) * ntaps
    nstage = cdiv(P, pt)
    ns = max(1, min(max(1, 1024 // tiles), cdiv(nstage, 8)))
    return cdiv(nstage, ns) * pt + 4 + ns


# ---------------------------------------------------------------------------------------------------------- references
def conv_ref(a, w, stride=1, padding=0, dilation=1, groups=1):
    """(reference, its absolute twin) of conv2d in f64"""
    F = torch.nn.functional
    return (F.conv2d(a, w, stride=stride, padding=padding, dilation=dilation, groups=groups),
            F.conv2d(a.abs(), w.abs(), stride=stride, padding=padding, dilation=dilation, groups=groups))


def conv_input_ref(shape, w, g, stride=1, padding=0, dilation=1, groups=1):
    G = torch.nn.grad
    return (G.conv2d_input(shape, w, g, stride=stride, padding=padding, dilation=dilation, groups=groups),
            G.conv2d_input(shape, w.abs(), g.abs(), stride=stride, padding=padding, dilation=dilation, groups=groups))


def conv_weight_ref(a, wshape, g, stride=1, padding=0, dilation=1, groups=1):
    G = torch.nn.grad
    return (G.conv2d_weight(a, wshape, g, stride=stride, padding=padding, dilation=dilation, groups=groups),
            G.conv2d_weight(a.abs(), wshape, g.abs(), stride=stride, padding=padding, dilation=dilation, groups=groups))


def dw_refs(a, w, gop, xshape, stride, dil):
    """((forward, S), (input gradient, S), (weight gradient, S)) of a depthwise 3x3 layer, padding = dilation, in f64"""
    kw = dict(stride=stride, padding=dil, dilation=dil, groups=w.shape[0])
    return conv_ref(a, w, **kw), conv_input_ref(xshape, w, gop, **kw), conv_weight_ref(a, w.shape, gop, **kw)


def convT_ref(x, w, stride=2, padding=1, output_padding=1):
    F = torch.nn.functional
    return (F.conv_transpose2d(x, w, stride=stride, padding=padding, output_padding=output_padding),
            F.conv_transpose2d(x.abs(), w.abs(), stride=stride, padding=padding, output_padding=output_padding))


def tap_geom(T, axis, dil):
    """(kernel shape, padding, dilation) of a T-tap layer along W (axis 0) or H (axis 1), padding = dilation (T - 1) / 2"""
    p = dil * (T - 1) // 2
    return ((1, T), (0, p), (1, dil)) if axis == 0 else ((T, 1), (p, 0), (dil, 1))


# ---------------------------------------------------------------------------------------------------------- depthwise 3x3 family
STAT_SLABS = 512          # TSS_STAT_SLABS (csrc/common.h): statistics slab rows, and the grid cap of the depthwise kernels
DW_NT = 256               # NT_MAX of csrc/dwconv.hip, NT of dwroll.hip / updw.hip
DW_SW = 4                 # SW: pixels of a strip (csrc/dwconv.hip)
RED_WAVES = 16            # waves of dw_reduce_kernel / dw_reduce_many_kernel


def reduce_chain(rows, waves=RED_WAVES):
    """dw_reduce_block / dw_reduce_block4 (csrc/dwconv.hip): a lane of wave w adds rows w, w + waves, ... (ceil(rows / waves)
    additions), one thread adds the waves' partial sums, and the total is added to dw"""
    return cdiv(rows, waves) + waves + 1


def dw_sweep(B, H, W, C, strip, dil=1):
    """geometry() + tss::persistent_blocks + xcd_tiles (csrc/dwconv.hip, common.h) of a launch over a [B][H][W] grid: (NPL lane items
    per tile, grid = workspace / slab rows written, tiles per block, waves per block).  Lane items are pixels (generic kernels) or
    4-pixel strips; the host sizes the grid by B H ceil(W / 4) strips, the stride-1 strip kernels walk ceil(W / 4 dil) dil interleaved
    strips per row (more at dilation 4 when W is ragged).  The tiles are dealt to 8 XCD ranges of ceil(ntiles / 8), each shared by
    grid / 8 blocks"""
    CV = C // 8
    NPL = DW_NT // CV
    host_units = B * H * (cdiv(W, DW_SW) if strip else W)
    units = B * H * cdiv(W, DW_SW * dil) * dil if strip else host_units
    grid = cdiv(min(max(cdiv(host_units, NPL), 1), STAT_SLABS), 8) * 8
    return NPL, grid, cdiv(cdiv(cdiv(units, NPL), 8), grid // 8), cdiv(CV * NPL, 64)


def dw_strip_pair(stride, dil):
    """strip_supported (csrc/dwconv.hip)"""
    return (stride, dil) in ((1, 1), (2, 1), (1, 4))


def dw_stats_chain(B, H, W, C, strip, dil=1):
    """f32 chain of one lane's statistics in dw_fwd_kernel / dw_bwd_data_kernel / their strip forms (bf16 instances; the f32
    instances add in f64): one value per pixel of every tile the block owns, 4 per strip; flush_stats then adds in f64"""
    _, _, tpb, _ = dw_sweep(B, H, W, C, strip, dil)
    return tpb * (DW_SW if strip else 1)


def dw_wgrad_chain(B, Ho, Wo, C, strip, dil=1, lead_waves=None, rows=None):
    """dw_bwd_weight_kernel / dw_bwd_weight_strip_kernel / dw_bwd_data_strip_kernel<WG> (the latter over the INPUT grid) + the row
    reduction: a lane adds one product per pixel it owns to each tap's accumulator (2 roundings each: the product, the addition), the
    block adds its NPL lanes through LDS, and the rows are added by dw_reduce_kernel (16 waves), tss_dw_reduce_many (16) or the lead
    blocks of tss_dwconv3x3_bwd_data (lead_waves = the sweeping kernel's waves per block)"""
    NPL, grid, tpb, _ = dw_sweep(B, Ho, Wo, C, strip, dil)
    return 2 * tpb * (DW_SW if strip else 1) + NPL + reduce_chain(grid if rows is None else rows, lead_waves or RED_WAVES)


def roll_plan(B, Ho, Wo, C, stride, lanes_per_slice=8, rpj=1):
    """plan (lanes_per_slice 8: dw_fwd_roll_kernel, 8 channels per lane) and plan_bwd (16: the backward kernels, 4 channels per lane;
    rpj = input rows per step) of csrc/dwroll.hip: column strips of PXL pixels x row segments of RS output rows x 64-channel slices;
    rows_used blocks per slice, each owning k = ceil(units / rows_used) units"""
    cv = C // (64 // lanes_per_slice)
    nsl = cdiv(C, 64)
    CVS = min(cv, lanes_per_slice)
    PXL = DW_NT // CVS
    nstrips = cdiv(Wo, PXL)
    cap = max(STAT_SLABS // nsl, 1)
    halo = 2 if stride == 1 else 1
    best = None
    for nseg in range(1, Ho + 1):
        RS = cdiv(Ho, nseg)
        if RS < 4 and nseg > 1:
            break
        segs = cdiv(Ho, RS)
        units = B * nstrips * segs
        k = cdiv(units, cap)
        cost = k * (cdiv(RS + halo, rpj) * rpj) + 6
        if best is None or cost < best['cost']:
            best = dict(cost=cost, RS=RS, nseg=segs, units=units, k=k, rows_used=cdiv(units, k))
    best.update(nsl=nsl, CVS=CVS, PXL=PXL, nstrips=nstrips)
    best['k'] = cdiv(best['units'], best['rows_used'])
    return best


def roll_stats_chain(plan, channels_per_lane, per_row=1):
    """a lane of a row-pipelined kernel adds one value per output row of every unit it owns (per_row = 4 in dw_bwd_roll_s2_kernel: the
    2 x 2 input pixels under an output pixel), then flush_slab adds ceil(PXL / share) lanes in f32, share = 256 / (2 CVS channels
    per lane) threads per column, before the f64 sum"""
    share = DW_NT // (2 * plan['CVS'] * channels_per_lane)
    return plan['k'] * plan['RS'] * per_row + cdiv(plan['PXL'], share)


def roll_wgrad_chain(plan, rows=None):
    """dw_bwd_roll_s1_kernel / dw_bwd_roll_s2_kernel: per tap one product per owned output row of every unit (2 roundings each), PXL
    lanes through LDS, then the rows_used rows by dw_reduce_kernel / tss_dw_reduce_many"""
    return 2 * plan['k'] * plan['RS'] + plan['PXL'] + reduce_chain(plan['rows_used'] if rows is None else rows)


def updw_geometry(B, Hs, Ws, Ho, Wo, C, D, px, halo, budgets, max_units):
    """geometry() of csrc/updw.hip (px = 32, halo = D, budgets 40 K then 56 K, 512 units forward; px = 16, halo 0, 36 K, 8192 units
    backward): segments per residue class such that a unit's source tile fits the LDS budget.  Its two scales are f32 quotients"""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    sy = (f32(Hs - 1) / f32(Ho - 1)) if Ho > 1 else f32(0.0)
    sx = (f32(Ws - 1) / f32(Wo - 1)) if Wo > 1 else f32(0.0)
    nstrips = cdiv(Wo, px)
    ncols = min(int(f32(px + 2 * halo - 1) * sx) + 4, Ws)
    njmax = cdiv(Ho, D)
    for budget in budgets:
        for nseg in range(1, njmax + 1):
            steps = cdiv(njmax, nseg)
            nrows = min(int(f32((steps + 3) * D) * sy) + 4, Hs)
            units = B * nstrips * D * nseg
            if units > max_units:
                break
            if nrows * ncols * 128 <= budget:
                return dict(nseg=nseg, seg_steps=steps, nunits=units, nstrips=nstrips)
    return None


def updw_fwd_geometry(B, Hs, Ws, Ho, Wo, C, D):
    return updw_geometry(B, Hs, Ws, Ho, Wo, C, D, 32, D, (40 * 1024, 56 * 1024), STAT_SLABS)


def updw_bwd_geometry(B, Hs, Ws, Ho, Wo, C, D):
    return updw_geometry(B, Hs, Ws, Ho, Wo, C, D, 16, 0, (36 * 1024,), 8192)


def updw_stats_chain(geo):
    """updw_fwd_kernel: a lane adds the seg_steps rows its unit owns in f32; the unit's 32 pixel lanes meet in f64"""
    return geo['seg_steps']


def updw_wgrad_chain(geo):
    """updw_bwd_kernel + tss_dw_reduce_many: per tap one product per owned class row (2 roundings each), BPX = 16 pixel lanes through
    LDS, then the nunits workspace rows"""
    return 2 * geo['seg_steps'] + 16 + reduce_chain(geo['nunits'])


def bilinear_matrix(n_in, n_out):
    """[n_out][n_in] f64 weights of bilinear interpolation with align_corners=True: source coordinate dst (n_in - 1) / (n_out - 1)"""
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    for d in range(n_out):
        src = d * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        i0 = min(int(math.floor(src)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        M[d, i0] += 1.0 - (src - i0)
        M[d, i1] += src - i0
    return M


def ac_taps_f32(n_in, n_out):
    """ac_scale / ac_tap of csrc/common.h, as updw.hip's lerp_store and lerp use them, step by step in f32: [(i0, i1, l0, l1)] per
    destination index"""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0.0)
    taps = []
    for dst in range(n_out):
        src = scale * f32(dst)
        i0 = min(int(src), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = src - f32(i0)
        taps.append((i0, i1, f32(1.0) - l1, l1))
    return taps


def dyadic_resize(n_in, n_out):
    """n_out - 1 = 2^k (n_in - 1): then ac_scale / ac_tap (csrc/common.h) -- scale = fl((n_in - 1) / (n_out - 1)) = 2^-k, src = scale *
    dst, i0 = (int)src, l1 = src - i0, l0 = 1 - l1 -- are all exact in f32 and equal bilinear_matrix's weights (multiples of 2^-k):
    ac_taps_f32 against bilinear_matrix in tests/test_exact_bounds.py"""
    if n_in == 1:
        return True
    q, r = divmod(n_out - 1, n_in - 1)
    return r == 0 and q >= 1 and (q & (q - 1)) == 0


def upsampled_operand(x, Ho, Wo):
    """(bf16-rounded upsampled map, its unrounded f64 value) of x [B][C][Hs][Ws]: the operand bits tss_updw_* forms on load"""
    My, Mx = bilinear_matrix(x.shape[2], Ho), bilinear_matrix(x.shape[3], Wo)
    v = torch.einsum('oh,bchw,pw->bcop', My, x, Mx)
    return v.float().to(torch.bfloat16).double(), v


def bilinear_f32_slack(x, Ho, Wo):
    """bound on |v_kernel - v| of one interpolated pixel BEFORE its bf16 rounding when the size pair is not dyadic, from ac_tap /
    lerp_store (csrc/common.h, updw.hip), u = 2^-24, M = max|x|:
      coordinates  scale = fl((n_in - 1) / (n_out - 1)) and src = fl(scale dst) are off by <= 2 u src (1 + u) = 2^-23 (1 + u) src, taken
                   as <= 2^-22 (n_in - 1) (a deliberate factor 2: it is dwarfed by the 2^-8 rounding of the operand that follows); the
                   blend is continuous and piecewise linear in src with slope <= 2 M per axis (|x[i + 1] - x[i]| <= 2 M), also across
                   an integer, where (int)src changes and l1 jumps between ~1 and ~0: <= 2^-21 M (n_in - 1) per axis;
      weights      l1 = src - i0 is exact (Sterbenz), l0 = fl(1 - l1) is off by <= u;
      blend        l0y (l0x a + l1x b) + l1y (l0x c + l1x d): every value goes through <= 5 roundings (two products, two sums, or an
                   FMA fewer) plus the weight's: <= gamma_6 sum of |weight products| M <= 2^-21 M (the weights sum to <= 1 + 2 u).
    Together <= 2^-21 M (Hs + Ws)"""
    return 2.0 ** -21 * float(x.abs().max()) * (x.shape[2] + x.shape[3])


# ---------------------------------------------------------------------------------------------------------- pointwise (1x1) family
# csrc/pwfast.hip, wgrad.hip (wgfast_kernel) + wgreduce.h, pwbwd.hip, pwsweep.hip; tests/test_gpu_pw_exact.py.  These kernels feed the
# matrix unit: a and g are rounded to bf16 (act / gcomb) and the weights are bf16-exact, so every product is exact and conv_excess holds
# with K the contraction length.  Each helper below restates a launch planner of the C source; the GPU test asserts its rows / workspace
# count against the library's own entry, so a planner that moves makes the test fail instead of the bound drift.
PW_SINGLE_THR = 4200      # block-tiles below which the single-chunk kernels take the small tile (TSS_PW_FWD_SMALL / TSS_PW_BWD_SMALL)


def pwfast_plan(P, K, N, bwd=False):
    """tss_pwfast_fwd / tss_pwconv_fwd_joined / tss_pwfast_bwd_data (csrc/pwfast.hip): (multi-chunk kernel, pixels per tile TM) of a
    GEMM with contraction K and N output columns (backward-data: K = the convolution's Cout, N = its Cin).  K <= 128:
    pwfast_kernel, forward TM 64 below 4200 block-tiles of 128 pixels else 128, backward 32 below 4200 block-tiles of 64 else 64;
    K > 128: pwfast_mc_kernel, TM 32 / 64 / 128 at t < 192 / t < 256 / otherwise, t = ceil(P / 128) ceil(N / 128)"""
    nch = cdiv(N, 128)
    if K <= 128:
        if bwd:
            return False, (32 if cdiv(P, 64) * nch < PW_SINGLE_THR else 64)
        return False, (64 if cdiv(P, 128) * nch < PW_SINGLE_THR else 128)
    t = cdiv(P, 128) * nch
    return True, (32 if t < 192 else 64 if t < 256 else 128)


def pwfast_stats_chain(P, K, N, bwd=False):
    """(f32 chain of one lane's statistics, slab rows in use) of launch_fast / launch_fast_mc_tm: the tiles are dealt to 8 XCD ranges of
    per = ceil(ntiles / 8), each shared by gs = min(per, cap) blocks, cap = (96 for the small single-chunk tile, else 64) / column
    chunks, at most 64, at least 1; a block owns ceil(per / gs) tiles, a lane adds TM / 32 pixels per tile (two waves split the tile's
    pixels, 16 per MFMA fragment), then row16_sum's 4 levels; the two pixel halves and the slab rows meet in f64"""
    mc, TM = pwfast_plan(P, K, N, bwd)
    nch = cdiv(N, 128)
    small = not mc and TM == (32 if bwd else 64)
    cap = max(1, min(64, (96 if small else 64) // nch))
    per = cdiv(cdiv(P, TM), 8)
    gs = min(per, cap)
    return TM // 32 * cdiv(per, gs) + 4, 8 * gs


def pw_ws_dim(d):
    """tss_wg::ws_dim: a workspace slot's extent along one axis"""
    return (min(d, 128) + 15) & ~15


def pw_wgrad_split(P, K, N):
    """tss_wg::split_for (csrc/wgreduce.h): (stage length, blocks per output tile, output tiles).  128-pixel stages when both chunk
    widths are <= 64 channels; a block owns >= 512 pixels, or >= 256 when tiles ceil(P / 512) < 256 (the small-layer rule)"""
    pt = 128 if max(min(N, 128), min(K, 128)) <= 64 else 64
    tiles = cdiv(N, 128) * cdiv(K, 128)
    nstage = cdiv(P, pt)
    min_px = 256 if tiles * cdiv(P, 512) < 256 else 512
    ns = max(1, min(max(1, 1024 // tiles), cdiv(nstage, cdiv(min_px, pt))))
    return pt, ns, tiles


def pw_wgrad_chain(P, K, N):
    """(f32 chain, workspace floats) of wgfast_kernel + tss_wg::reduce_block: a block owns ceil(nstage / nsplit) stages of pt pixels,
    one exact product per pixel into an accumulator (waves that split a stage's k-steps meet in one LDS addition); reduce_block: a wave
    adds slots w, w + 4, ... (ceil(nsplit / 4)), one thread adds the 4 waves' sums, and the total is added to dW"""
    pt, ns, tiles = pw_wgrad_split(P, K, N)
    return cdiv(cdiv(P, pt), ns) * pt + 1 + cdiv(ns, 4) + 4 + 1, tiles * ns * pw_ws_dim(N) * pw_ws_dim(K)


def pwbwd_rows(P, Cin, Cout, big_tr=False, drop=False):
    """tss_pwconv_bwd_fused_rows / _drop_rows + launch() of csrc/pwbwd.hip: (instance, TM, pixels a lane adds per tile MFX, workspace =
    slab rows 8 gs, tiles per block).  MFX = TM / (waves / NSPLIT) / 16"""
    if drop:
        name, TM, MFX, cap = 'drop', 64, 2, 64
    elif Cin <= 64 and Cout <= 64:
        name, TM, MFX, cap = 'small', 128, 2, 64
    elif Cin <= 64:
        name, TM, MFX, cap = 'mid', 64, 1, 64
    elif Cout <= 64:
        name, TM, MFX, cap = 'tall', 64, 1, 64
    elif big_tr:
        name, TM, MFX, cap = 'big_tr', 64, 2, 64
    else:
        name, TM, MFX, cap = 'big', 128, 2, 32
    per = cdiv(cdiv(P, TM), 8)
    gs = max(1, min(per, cap))
    return name, TM, MFX, 8 * gs, cdiv(per, gs)


def pwbwd_stats_chain(plan):
    """pwbwd_kernel / pwsweep_kernel: a lane adds MFX pixels per tile it owns, then row16_sum's 4 levels (the waves meet in f64)"""
    return plan[2] * plan[4] + 4


def pwbwd_wgrad_chain(plan):
    """pwbwd_kernel / pwsweep_kernel + tss_dw_reduce_many: the block keeps its [Cout][Cin] tile in accumulators over every tile it owns
    (TM exact products each), writes one workspace row, and the rows are added by dw_reduce_block (reduce_chain)"""
    return plan[4] * plan[1] + reduce_chain(plan[3])


def pwbwd_bias_chain(plan):
    """the bias-gradient row of pwbwd_kernel: a thread adds (v0 + v1) + (v2 + v3) of its 4 pixels to its sum per tile (3 roundings a
    term goes through), then one thread adds the TM / 4 pixel groups"""
    return 3 * plan[4] + plan[1] // 4


PWSWEEP_KINDS = {(128, 128): (64, 2), (64, 384): (32, 1), (384, 64): (32, 2), (32, 192): (64, 1), (192, 32): (32, 1)}     # (TM, DXM)


def pwsweep_rows(P, Cin, Cout):
    """slots_for + Cfg of csrc/pwsweep.hip in pwbwd_rows' form: one 512-thread block per CU (gs <= 32), P / TM whole tiles"""
    TM, DXM = PWSWEEP_KINDS[(Cin, Cout)]
    assert P % TM == 0
    per = cdiv(P // TM, 8)
    gs = max(1, min(per, 32))
    return 'sweep', TM, DXM, 8 * gs, cdiv(per, gs)


def joined_fwd_ref(conv, S, cbias, omean, oscale, obeta, res=None, relu=False):
    """tss_pwconv_fwd_joined: y = relu?((v - out_mean) out_scale + out_beta + residual), v = conv + bias.  Returns (ref, M) for
    conv_excess(out, ref, M, K + 2).  The kernel computes shift = out_beta + (bias - out_mean) out_scale once per channel: exact in
    f32 for dyadic vectors and a power-of-two out_scale (checked here), whatever the contraction of the compiler.  Then per element
        acc  = f32 sum of the K exact products             |acc - conv| <= gamma_K S
        t1   = fl(acc out_scale + shift)                   the product is a shift: ONE rounding, of a value <= out_scale S' + |shift|
        t2   = fl(t1 + residual)                           one more, of a value <= |t1| + |residual|
    so |t2 - r| <= out_scale gamma_K S + u (1 + u) (|t1| + |t2|) <= gamma_(K + 2) M with M = out_scale S + |shift| + |residual| (the
    accumulation term is multiplied by out_scale, as are S and hence M).  ReLU is 1-Lipschitz, and the bf16 rounding adds
    2^-8 (|ref| + gamma_(K + 2) M): |y - ref| <= 2^-8 |ref| + 2^-23 (K + 2) (1 + 2^-8) M <= 2^-8 |ref| + 2^-22 (K + 2) M"""
    shift = exact_f32(obeta + ((cbias if cbias is not None else 0.0) - omean) * oscale)
    r, M = conv * oscale + shift, S * oscale + shift.abs()
    if res is not None:
        r, M = r + res, M + res.abs()
    return (r.clamp_min(0.0) if relu else r), M


def joined_bwd_ref(rin, Sin, radd, jout):
    """tss_pwconv_bwd_data_joined: e_in = (g W + radd) where join_out > 0, else 0.  Returns (ref, M) for conv_excess(out, ref, M, K + 1):
    the f32 sum of the K exact products takes radd (a bf16 value, exact) in one more addition -- K + 1 terms, gamma_(K + 1) M with
    M = S + |radd| -- the mask selects the value or an exact 0 (join_out is given, so the mask is the reference's own), and the result is
    rounded to bf16 once.  join_bstats then holds sum e_in and sum e_in (join_y - join_mean) of the STORED bits: stats_excess with the
    launch's pwfast_stats_chain (the difference is exact in f32 for dyadic operands, the product has <= 8 + 16 bits)"""
    keep = (jout > 0).double()
    if radd is not None:
        rin, Sin = rin + radd, Sin + radd.abs()
    return rin * keep, Sin * keep


# ---------------------------------------------------------------------------------------------------------- dense 3x3 family and stem
# csrc/wstat.hip, atrous.hip, conv3x3.hip, the 9-tap A_TAPS path of convgemm.hip / wgrad.hip and csrc/stem.hip; tests/test_gpu_dense_exact.py.
# These kernels feed the matrix unit from bf16 operands (act / gcomb; the weights are bf16-exact), so conv_excess holds with K = 9 x the
# contraction.  Each helper restates a dispatch rule or a launch planner of the C source; the GPU test checks the slab / workspace rows a
# launch leaves in use against the restated grid.
WSTAT_TP, WSTAT_GRID, WSTAT_MAXD = 64, 256, 18      # TP, the launch's block count, MAXD of csrc/wstat.hip
LEAN_MAXDIL = 18                                      # MAXDIL of csrc/conv3x3.hip


def conv3x3_fwd_route(H, Cin, N, stride, dil, pending, relu, ldx, ldy, shadow=True, bf16=True):
    """which kernel tss_conv3x3_fwd (csrc/convgemm.hip) launches, in the order it asks: tss_conv3x3_wstat_fwd, tss_conv3x3_stream_fwd,
    tss_conv3x3_lean_fwd (all three need the bf16 weight copy), tss_sconv_fwd, convgemm_kernel.  pending: in_scale given"""
    if bf16 and shadow:
        mat = not pending and not relu and stride == 1
        if mat and dil <= WSTAT_MAXD and Cin == 128 and N == 128 and ldx % 8 == 0 and ldy % 8 == 0 and H >= dil:
            return 'wstat'
        if mat and 32 <= Cin <= 128 and Cin % 32 == 0 and 16 <= N <= 128 and N % 16 == 0 and ldx % 8 == 0 and ldy % 4 == 0:
            return 'stream<4, true>' if (Cin, N) == (128, 128) else 'stream<0, false>'
        if stride == 1 and dil <= LEAN_MAXDIL and Cin in (32, 64, 128) and 16 <= N <= 128 and N % 16 == 0 and ldx % 8 == 0 and ldy % 4 == 0:
            return 'lean<false, 2>' if dil == 1 else 'lean<false, 3>'
    if bf16 and stride == 2 and dil == 1 and Cin <= 64 and N <= 128:
        return 'sconv or generic'
    return 'generic'


def conv3x3_bwd_route(Cin, N, dil, with_y, shadow=True, bf16=True):
    """tss_conv3x3_bwd_data: conv3x3_lean_kernel<true, 2 | 3> (contraction N in {32, 64, 128}, outputs Cin % 16 == 0 <= 128, yraw and
    the bf16 weight copy given, dilation <= 18), else convgemm_kernel with two sources (yraw) or one"""
    if bf16 and shadow and with_y and dil <= LEAN_MAXDIL and N in (32, 64, 128) and 16 <= Cin <= 128 and Cin % 16 == 0:
        return 'lean<true, 2>' if dil == 1 else 'lean<true, 3>'
    return 'generic'


def wstat_decode(u, H, W, D):
    """decode() of conv3x3_wstat_kernel: unit u of the walk order -- (image, strip) major, then residue class r = y mod D, then j
    (y = r + j D) -- as (b, strip, r, j, rows of the class)"""
    nstrip = cdiv(W, WSTAT_TP)
    qd = H // D
    rem = H - qd * D                          # classes r < rem have qd + 1 rows, the others qd
    bs, pp = divmod(u, H)
    b, sx = divmod(bs, nstrip)
    if pp < rem * (qd + 1):
        r, j = divmod(pp, qd + 1)
        return b, sx, r, j, qd + 1
    pp -= rem * (qd + 1)
    r = rem + pp // qd
    return b, sx, r, pp - (r - rem) * qd, qd


def wstat_ranges(B, H, W):
    """the launch of tss_conv3x3_wstat_fwd: nrows = B ceil(W / 64) H units, grid = min(nrows, 256), block i owns
    [i nrows / grid, (i + 1) nrows / grid)"""
    nrows = B * cdiv(W, WSTAT_TP) * H
    grid = min(nrows, WSTAT_GRID)
    return [(i * nrows // grid, (i + 1) * nrows // grid) for i in range(grid)]


def wstat_segments(lo, hi, H, W, D):
    """the while loop of conv3x3_wstat_kernel over one block's range: [(b, strip, r, j0, j1)], rows j0 .. j1 - 1 of one walk each"""
    segs, u = [], lo
    while u < hi:
        b, sx, r, j0, nj = wstat_decode(u, H, W, D)
        j1 = nj if nj - j0 < hi - u else j0 + (hi - u)
        segs.append((b, sx, r, j0, j1))
        u += j1 - j0
    return segs


def wstat_plan(B, H, W, D):
    """rows per block, the statistics chain (a lane adds 4 pixel fragments per owned row, then row16_sum's 4 levels; waves own their
    channels alone and blocks meet in f64), the slab rows in use, and what the ranges exercise: the longest run of consecutive rows of
    one walk (> 4: the four ring slots wrap) and whether some range crosses a class, a strip and an image boundary"""
    ranges = wstat_ranges(B, H, W)
    run, cross = 0, set()
    for lo, hi in ranges:
        segs = wstat_segments(lo, hi, H, W, D)
        run = max([run] + [s[4] - s[3] for s in segs])
        for p, q in zip(segs, segs[1:]):
            cross.add('image' if p[0] != q[0] else 'strip' if p[1] != q[1] else 'class')
    rows = max(hi - lo for lo, hi in ranges)
    return dict(grid=len(ranges), rows=rows, chain=4 * rows + 4, run=run, cross=cross)


def stream_plan(P):
    """tss_conv3x3_stream_fwd + xcd_tiles (csrc/atrous.hip, common.h): 256-pixel tiles dealt to 8 XCD ranges of per = ceil(ntiles / 8),
    each shared by grid / 8 blocks, grid = persistent_blocks(ntiles, 512).  (statistics chain: a lane adds 4 pixels per tile it owns, then
    row16_sum's 4 levels, the waves meet in f64; slab rows that own a tile; grid)"""
    ntiles = cdiv(P, 256)
    grid = cdiv(min(max(ntiles, 1), STAT_SLABS), 8) * 8
    slots, per = grid // 8, cdiv(ntiles, 8)
    owners = [r for r in range(grid) if (r & 7) * per + (r >> 3) < min((r & 7) * per + per, ntiles)]
    return 4 * cdiv(per, slots) + 4, owners, grid


def stream_tiles(row, P):
    """the tiles block `row` of the stream kernel's grid owns, in its order"""
    ntiles = cdiv(P, 256)
    grid = cdiv(min(max(ntiles, 1), STAT_SLABS), 8) * 8
    per = cdiv(ntiles, 8)
    return list(range((row & 7) * per + (row >> 3), min((row & 7) * per + per, ntiles), grid // 8))


def lean3x3_plan(B, H, W):
    """launch_lean_nb + the grid-stride tile loop of conv3x3_lean_kernel (csrc/conv3x3.hip): tiles of 64 pixels of one image row,
    grid = min(ntiles, 512), block i owns tiles i, i + grid, ...; a lane adds 2 pixels per tile, then row16_sum's 4 levels, and the two
    wm halves meet in f64.  (statistics chain, slab rows that own a tile, grid)"""
    ntiles = B * H * cdiv(W, 64)
    grid = min(ntiles, STAT_SLABS)
    return 2 * cdiv(ntiles, grid) + 4, list(range(grid)), grid


def stem_fwd_plan(P):
    """tss_stem_direct_fwd + stem_fwd_mfma_kernel (csrc/stem.hip): 256-pixel tiles, grid = persistent_blocks(ceil(P / 256), 512), block
    i owns tiles i, i + grid, ...; a lane adds 4 pixels per tile, then row16_sum's 4 levels, the waves meet in f64"""
    ntiles = cdiv(P, 256)
    grid = cdiv(min(max(ntiles, 1), STAT_SLABS), 8) * 8
    return 4 * cdiv(ntiles, grid) + 4, list(range(min(ntiles, grid))), grid


def stem_wgrad_plan(P, mfma):
    """tss_stem_direct_wgrad: grid = min(ceil(P / 256), 512) blocks = workspace rows, block i owns tiles i, i + grid, ...
    MFMA form: a wave adds its 64 pixels of every tile to its accumulators (exact products), the 4 waves meet in 3 additions.
    VALU form (yraw == NULL): a lane adds the 256 pixels of every tile, each product of an f32 g and an f32 tap rounded first (2
    roundings per pixel).  stem_wgrad_reduce_kernel: a lane adds rows rg, rg + 16, ..., one thread the 16 groups, the total onto dW.
    (chain, workspace rows)"""
    ntiles = cdiv(P, 256)
    grid = min(ntiles, STAT_SLABS)
    tpb = cdiv(ntiles, grid)
    return (64 * tpb + 3 if mfma else 2 * 256 * tpb) + cdiv(grid, 16) + 16 + 1, grid


def stem_tap_columns(ox, Win, stride, window):
    """the image column each of the three kx taps of output column ox reads (None: the tap is a 0), as stem_taps (csrc/stem.hip) picks
    it.  window: the f32 stride-2 path at Win >= 4 -- ONE 4-float load at base = clamp(2 ox - 1, 0, Win - 4), tap kx at position
    kx + (2 ox - 1 - base) of it (positions <= 0 read element 0, >= 3 element 3), masked where that position is left of the window or the
    tap's column is >= Win; else one load per tap at the column clamped into [0, Win - 1], masked outside the image"""
    cols = []
    if window:
        assert stride == 2 and Win >= 4
        ix0 = 2 * ox - 1
        base = 0 if ix0 < 0 else (Win - 4 if ix0 > Win - 4 else ix0)
        sh = ix0 - base
        for kx in range(3):
            idx = kx + sh
            pos = 0 if idx <= 0 else min(idx, 3)
            cols.append(base + pos if (idx >= 0 and ix0 + kx < Win) else None)
        return cols
    for kx in range(3):
        ix = ox * stride + kx - 1
        cols.append(min(max(ix, 0), Win - 1) if 0 <= ix < Win else None)
    return cols


def full_f32(shape, gen):
    """f32 values with all 24 bits of the significand in use: the sum of two dyadic values whose exponents differ by 16 (bits e .. e - 7
    and e - 16 .. e - 23: exact in f32, checked), so rounding one to bf16 moves it"""
    e = torch.randint(-4, 2, shape, generator=gen).double()
    parts = []
    for shift in (0.0, 16.0):
        k = torch.randint(0, 128, shape, generator=gen).double()
        s = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
        parts.append(s * (1 + k / 128) * torch.pow(2.0, e - shift))
    return exact_f32(parts[0] + parts[1])


# ---------------------------------------------------------------------------------------------------------- resample, pyramid, gate
# csrc/resample.hip and gate.hip; tests/test_gpu_resample_exact.py.  None of these kernels feeds the matrix unit: operands are loaded
# into f32, blended / gathered / averaged in f32 and rounded once to the output dtype.  Three tiers (the GPU file names the tier of a case):
#   1  bit for bit.  The size pair is exact_resize on both axes: every tap weight is a multiple of 2^-k.  With operands that are
#      multiples of 2^lsb, every product and every partial sum of a blend or a gather is a multiple of 2^(lsb - ky - kx) and, in ANY
#      order and with or without FMA contraction, at most sum|terms| in magnitude: if max sum|terms| < 2^(24 + lsb - ky - kx) all of
#      them are f32 numbers and nothing rounds (exact_budget).  The f32 output equals the f64 reference, the bf16 output its rne_bf16.
#   2  derived bound on the restated taps.  Indices and f32 weights from ac_taps_f32 (tap_matrix_f32), blended / gathered in f64;
#      the kernel's roundings are counted in u = 2^-24 against sum|terms|, + 2^-8 |ref| for a bf16 output (resample_excess).  The same
#      outputs are also held to bilinear_matrix within bilinear_f32_slack (+ the same bound): the only check that would catch the
#      restated taps and the kernel being wrong together.
#   3  near-tie allowance, tss_ppm_arms_bwd in training mode only: arms_bwd_ref at the end of this file.
F32 = np.float32


def dyadic_q(shape, gen, bits, emin, emax, zero_frac=0.0):
    """dyadic with `bits` significant bits: +-(1 + k / 2^(bits-1)) 2^e, k in [0, 2^(bits-1)), e in [emin, emax): multiples of
    2^(emin - bits + 1), below 2^emax in magnitude.  The narrow operands of the tier-1 gathers, whose window sums have to fit 24 bits"""
    m = 1 << (bits - 1)
    k = torch.randint(0, m, shape, generator=gen).double()
    e = torch.randint(emin, emax, shape, generator=gen).double()
    s = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    v = s * (1 + k / m) * torch.pow(2.0, e)
    if zero_frac > 0:
        v = torch.where(torch.rand(shape, generator=gen, dtype=torch.float64) < zero_frac, torch.zeros_like(v), v)
    return v


def lsb_exp(v):
    """largest e such that every element of v (f64) is a multiple of 2^e"""
    nz = v[v != 0]
    e = 0
    while not torch.equal(torch.round(nz * 2.0 ** -e), nz * 2.0 ** -e):
        e -= 1
    return e


def ac_scale_f32(n_in, n_out):
    return F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0.0)


def exact_resize(n_in, n_out):
    """tier-1 premise of one axis: n_out - 1 = 2^k >= n_in - 1 (or one of the extents is 1).  Then ac_scale = (n_in - 1) 2^-k is exact
    in f32, src = scale dst = (n_in - 1) dst 2^-k has < 24 bits, i0 = (int)src = floor of the exact coordinate, l1 = src - i0 is a
    multiple of 2^-k in [0, 1) and l0 = 1 - l1 is exact.  Wider than dyadic_resize (which asks for a power-of-two RATIO): 6 -> 17,
    4 -> 33 and 7 -> 33 are exact although 16 / 5, 32 / 3 and 32 / 6 are not integers.  Returns k or None;
    ac_taps_f32 is compared with bilinear_matrix on every such pair in tests/test_exact_bounds.py"""
    if n_in == 1 or n_out == 1 or n_in == n_out:      # scale 0 (every weight 1 at index 0) or exactly 1 (l1 = 0)
        return 0
    m = n_out - 1
    if m & (m - 1) == 0 and n_in - 1 <= m:
        return m.bit_length() - 1
    if dyadic_resize(n_in, n_out):                      # the ratio itself is 2^k: scale = 2^-k whatever n_out - 1 is
        return (m // (n_in - 1)).bit_length() - 1
    return None


def tap_matrix_f32(n_in, n_out, clamp=True, fused=True):
    """[n_out][n_in] f64 matrix of the restated f32 taps (ac_taps_f32): row d holds l0 at i0 and l1 at i1, as f32 values.
    clamp=False is the injected defect of tests/test_exact_bounds.py: i1 = i0 + 1 unclamped (reads the next row / image)"""
    i0, i1, l0, l1 = ac_taps_np(n_in, n_out, fused)
    M = np.zeros((n_out, n_in + (0 if clamp else 1)))
    d = np.arange(n_out)
    np.add.at(M, (d, i0), l0.astype(np.float64))
    np.add.at(M, (d, i1 if clamp else i0 + 1), l1.astype(np.float64))
    return torch.from_numpy(M)


def ac_taps_np(n_in, n_out, fused=True):
    """ac_tap of csrc/common.h for all destinations at once (numpy f32 arrays i0, i1, l0, l1).  fused: l1 = fl(scale dst - i0) in ONE
    rounding, which is what hipcc's default -ffp-contract=fast makes of `src - (float)i0` with src = scale * dst (a v_fma_f32 in the
    disassembly of every kernel of resample.hip; i0 = (int)src still comes from the ROUNDED product).  The f64 product of a 24-bit
    scale and an integer below 2^29 is exact, so rounding it once to f32 restates the FMA bit for bit.  fused=False is ac_taps_f32,
    l1 = fl(fl(scale dst) - i0); the two differ by the rounding of src, <= u src <= u (n_in - 1) (tap_slack), and not at all on an
    exact_resize pair, where src is exact.  Both are compared with ac_taps_f32 / bilinear_matrix in tests/test_exact_bounds.py"""
    scale = ac_scale_f32(n_in, n_out)
    dst = np.arange(n_out)
    src = scale * dst.astype(F32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (np.float64(scale) * dst - i0).astype(F32) if fused else src - i0.astype(F32)
    return i0, i1, F32(1.0) - l1, l1


def tap_support(n_in, n_out):
    """[n_out][n_in] 0/1: the source indices an output reads (i0 and i1, whatever their weights)"""
    i0, i1, _, _ = ac_taps_np(n_in, n_out)
    M = np.zeros((n_out, n_in))
    M[np.arange(n_out), i0] = 1.0
    M[np.arange(n_out), i1] = 1.0
    return torch.from_numpy(M)


def tap_slack(x, Ho, Wo):
    """what a forward blend of x [B][C][H][W] may differ by when the compiler does NOT contract l1 (or contracts where the restated taps do
    not): each weight of an axis moves by <= u (n_in - 1), and the blend by that times the sum of the |values| it reads (the other
    axis' weights sum to <= 1 + 2 u, covered by the factor 1.001)"""
    T = torch.einsum('oh,bchw,pw->bcop', tap_support(x.shape[2], Ho), x.abs(), tap_support(x.shape[3], Wo))
    return 1.001 * U32 * (x.shape[2] - 1 + x.shape[3] - 1) * T


def tap_slack_bwd(g, Hin, Win=None):
    """the same for the transposed gather of g [B][C][Ho][Wo] onto [Hin][Win]; Win=None: the row pass alone, onto [Hin][Wo]"""
    sy = tap_support(Hin, g.shape[2])
    if Win is None:
        return 1.001 * U32 * (Hin - 1) * torch.einsum('oh,bcop->bchp', sy, g.abs())
    T = torch.einsum('oh,bcop,pw->bchw', sy, g.abs(), tap_support(Win, g.shape[3]))
    return 1.001 * U32 * (Hin - 1 + Win - 1) * T


def ac_windows_np(n_in, n_out):
    """ac_window of csrc/common.h in f32 for every source index at once: the conservative ranges [lo, hi] of outputs whose taps can
    include source index i"""
    scale = ac_scale_f32(n_in, n_out)
    if scale <= 0:
        return np.zeros(n_in, dtype=np.int64), np.full(n_in, n_out - 1, dtype=np.int64)
    i = np.arange(n_in)
    lo = np.floor((i - 1).astype(F32) / scale).astype(np.int64) - 1
    hi = np.ceil((i + 1).astype(F32) / scale).astype(np.int64) + 1
    return np.maximum(lo, 0), np.minimum(hi, n_out - 1)


def ac_window_f32(n_in, n_out, i):
    lo, hi = ac_windows_np(n_in, n_out)
    return int(lo[i]), int(hi[i])


def window_len(n_in, n_out):
    """longest restated window over the source indices: the n of gamma_n of a backward gather along this axis"""
    lo, hi = ac_windows_np(n_in, n_out)
    return int((hi - lo).max()) + 1


def window_misses(n_in, n_out, short=0):
    """taps with a nonzero f32 weight whose output lies outside the restated window of their source index (hi - short: the defect)"""
    i0, i1, l0, l1 = ac_taps_np(n_in, n_out)
    lo, hi = ac_windows_np(n_in, n_out)
    hi = hi - short
    d = np.arange(n_out)
    return int(((l0 != 0) & ((d < lo[i0]) | (d > hi[i0]))).sum() + ((l1 != 0) & ((d < lo[i1]) | (d > hi[i1]))).sum())


def windowed(M, n_in, n_out, short=0):
    """the tap matrix with everything outside the restated windows zeroed: what a gather over ac_window_f32 sums"""
    Mw = torch.zeros_like(M)
    for i in range(n_in):
        lo, hi = ac_window_f32(n_in, n_out, i)
        Mw[lo:hi + 1 - short, i] = M[lo:hi + 1 - short, i]
    return Mw


def resize_ref(x, Ho, Wo, My=None, Mx=None):
    """(reference, sum|terms|) of the align_corners=True resize of x [B][C][H][W] on the restated f32 taps, in f64"""
    My = tap_matrix_f32(x.shape[2], Ho) if My is None else My
    Mx = tap_matrix_f32(x.shape[3], Wo) if Mx is None else Mx
    return torch.einsum('oh,bchw,pw->bcop', My, x, Mx), torch.einsum('oh,bchw,pw->bcop', My, x.abs(), Mx)


def resize_bwd_ref(g, Hin, Win):
    """(tmp reference, its sum|terms|, dx reference, its sum|terms|) of the two-pass backward of a resize to g's [B][C][Ho][Wo]: the
    row pass tmp [B][C][Hin][Wo] = My^T g, then dx [B][C][Hin][Win] = tmp Mx.  The restated windows hold every nonzero weight
    (window_misses == 0, asserted on the CPU), so the windowed gather equals the full transposed product"""
    My, Mx = tap_matrix_f32(Hin, g.shape[2]), tap_matrix_f32(Win, g.shape[3])
    t, ta = torch.einsum('oh,bcop->bchp', My, g), torch.einsum('oh,bcop->bchp', My, g.abs())
    return t, ta, torch.einsum('bchp,pw->bchw', t, Mx), torch.einsum('bchp,pw->bchw', ta, Mx)


def resize_matrix_excess(out, x, Ho, Wo, bf16):
    """the forward outputs against bilinear_matrix (f64 coordinates) within bilinear_f32_slack, which already holds the blend's own
    roundings; a bf16 output adds 2^-8 (|ref| + slack)"""
    My, Mx = bilinear_matrix(x.shape[2], Ho), bilinear_matrix(x.shape[3], Wo)
    ref = torch.einsum('oh,bchw,pw->bcop', My, x, Mx)
    slack = bilinear_f32_slack(x, Ho, Wo)
    bound = slack + (2.0 ** -8 * (ref.abs() + slack) if bf16 else 0.0)
    return ((out - ref).abs() - bound).max().item()


def resize_bwd_matrix_excess(out, g, Hin, Win, n, bf16, gs=1.0):
    """the backward outputs dx [B][C][Hin][Win] against the transposed bilinear_matrix.  The weight with which output o reads source i
    is the hat function max(0, 1 - |src_o - i|) of the coordinate: 1-Lipschitz, so the f32 weight is within |d src| + u of the f64
    one, |d src| <= 2^-22 (n_in - 1) as in bilinear_f32_slack, and a product of two weights (each <= 1) within the sum of the two
    (+ their product, covered by the factor 2 already in 2^-22).  Summed over the outputs where either weight is nonzero; plus the
    gather's own bound resample_excess(n) on the f64 weights' sum|terms|"""
    My, Mx = bilinear_matrix(Hin, g.shape[2]), bilinear_matrix(Win, g.shape[3])
    sy = ((My != 0) | (tap_matrix_f32(Hin, g.shape[2]) != 0)).double()
    sx = ((Mx != 0) | (tap_matrix_f32(Win, g.shape[3]) != 0)).double()
    ref = gs * torch.einsum('oh,bcop,pw->bchw', My, g, Mx)
    S = gs * torch.einsum('oh,bcop,pw->bchw', My, g.abs(), Mx)
    slack = gs * (2.0 ** -22 * (Hin - 1 + Win - 1) + 4 * U32) * torch.einsum('oh,bcop,pw->bchw', sy, g.abs(), sx)
    bound = slack + 2.0 ** -23 * (n + (1 if bf16 else 0)) * (S + slack) + (2.0 ** -8 * (ref.abs() + slack) if bf16 else 0.0)
    return ((out - ref).abs() - bound).max().item()


BLEND_N = 6     # roundings a value goes through in a 2 x 2 blend: two products and two sums (an FMA fewer) + the weight's l0 = fl(1 - l1)


def resample_excess(out, ref, S, n, bf16, slack=0.0):
    """|out - ref| <= gamma_n S (<= 2^-23 n S) + slack + 2^-8 (|ref| + gamma_n S + slack) for a bf16 output.  n = BLEND_N for a forward
    blend; a gather over a window of L outputs rounds each product once and each partial sum once: n = L + 1 per pass, and the column
    pass of a two-pass backward inherits the row pass's: n = Ly + Lx + 2.  2^-8 gamma_n S is covered by counting one more rounding
    (n + 1).  slack: tap_slack / tap_slack_bwd, the contraction of l1 the compiler is free to make or not.
    Returns max(|out - ref| - bound)"""
    bound = 2.0 ** -23 * (n + (1 if bf16 else 0)) * S + slack * (1 + 2.0 ** -8) + (2.0 ** -8 * ref.abs() if bf16 else 0.0)
    return ((out - ref).abs() - bound).max().item()


def exact_budget(S, lsb, ky=0, kx=0):
    """tier-1 premise: every partial sum (<= max S = sum|terms|) of multiples of 2^(lsb - ky - kx) stays below 2^24 of them"""
    return float(S.max()) < 2.0 ** (24 + lsb - ky - kx)


def out_bits_ref(ref, bf16):
    """the bits a tier-1 kernel must store: the exact value (checked to be an f32 number), rounded to bf16 once for a bf16 output"""
    return rne_bf16(ref) if bf16 else exact_f32(ref)


# --- logits head (upsample_head_fwd_kernel<T, 3 | 4>, upsample_head_fwd_generic_kernel)
def head_instance(w, W, ldl, N, aligned=True):
    """the dispatch of tss_upsample_head_fwd: 'three' / 'four' source columns per lane of 8 outputs, or 'generic'"""
    sx = F32(w - 1) / F32(W - 1) if W > 1 else F32(0.0)
    fast = F32(7.0) * sx < F32(1.99) and ldl % 8 == 0 and ldl >= cdiv(N, 8) * 8 and aligned
    if not fast:
        return 'generic'
    return 'three' if F32(7.0) * sx < F32(0.99) else 'four'


def head_columns_hold(w, W, ncols):
    """every lane's 8 outputs read source columns c0 .. c0 + ncols - 1 only, c0 = i0 of the lane's first output (an i1 beyond them
    with the weight l1 == 0 multiplies a finite column by 0: harmless)"""
    i0, i1, _, l1 = (v.reshape(W // 8, 8) for v in ac_taps_np(w, W))
    c0 = i0[:, :1]
    return bool(((i0 - c0 >= 0) & (i0 - c0 < ncols) & ((i1 - c0 < ncols) | (l1 == 0))).all())


# --- adaptive average pooling (adaptive_pool_*_kernel, ppm_pool_*_kernel)
def pool_windows(n, bins):
    """pool_start / pool_end: [(start, end)] of the bins windows along an extent of n (overlapping when bins does not divide n,
    one-pixel windows that repeat when bins > n)"""
    return [(i * n // bins, ((i + 1) * n + bins - 1) // bins) for i in range(bins)]


def pool_matrix(n, bins, inverse=False, drop_last=False):
    """[bins][n] 0/1 membership; inverse: 1 / window length instead (the f64 reciprocal).  drop_last: the defect of a window one short"""
    M = torch.zeros(bins, n, dtype=torch.float64)
    for i, (a, b) in enumerate(pool_windows(n, bins)):
        b2 = b - 1 if drop_last and b - a > 1 else b
        M[i, a:b2] = 1.0 / (b - a) if inverse else 1.0
    return M


def pool_ref(x, bins):
    """(window sums, sum|terms|, window sizes [bins][bins]) of x [B][C][H][W] in f64"""
    Py, Px = pool_matrix(x.shape[2], bins), pool_matrix(x.shape[3], bins)
    n = Py.sum(1)[:, None] * Px.sum(1)[None, :]
    return torch.einsum('ih,bchw,jw->bcij', Py, x, Px), torch.einsum('ih,bchw,jw->bcij', Py, x.abs(), Px), n


def pool_fwd_excess(out, sums, n, bf16):
    """forward: the window sum is EXACT in f32 (operands multiples of 2^-11 below 4, at most 2^11 of them: exact_budget, asserted by the
    caller), then ONE f32 division s / (float)n.  hipcc's default (-O3, no fast-math; -fhip-fp32-correctly-rounded-divide-sqrt is on
    by default, clang's HIP options reference) lowers `/` to the v_div_scale / v_div_fmas / v_div_fixup sequence: correctly rounded,
    |fl(q) - q| <= u |q|.  A bf16 output rounds fl(q) once more: <= 2^-8 |fl(q)| <= 2^-8 (1 + u) |q|"""
    ref = sums / n
    bound = ref.abs() * (U32 + (2.0 ** -8 * (1 + U32) if bf16 else 0.0))
    return ((out - ref).abs() - bound).max().item()


def pool_bwd_ref(gs, H, W, binss, radd=None):
    """(reference, sum|terms|, longest chain) of dx = sum over arms of P_y^T (dy / n) P_x (+ radd): every pixel adds v * fl(1 / n) per
    window that holds it.  A term is rounded in fl(1 / n) (correctly rounded), in the product and in each addition that follows it:
    chain = 2 + the number of terms a pixel can add (overlaps per arm, + 1 for radd)"""
    ref = torch.zeros(gs[0].shape[0], gs[0].shape[1], H, W, dtype=torch.float64)
    S, terms = torch.zeros_like(ref), 0
    for g, bins in zip(gs, binss):
        Py, Px = pool_matrix(H, bins), pool_matrix(W, bins)
        n = Py.sum(1)[:, None] * Px.sum(1)[None, :]
        ref += torch.einsum('ih,bcij,jw->bchw', Py, g / n, Px)
        S += torch.einsum('ih,bcij,jw->bchw', Py, g.abs() / n, Px)
        terms += int(Py.sum(0).max()) * int(Px.sum(0).max())
    if radd is not None:
        ref, S, terms = ref + radd, S + radd.abs(), terms + 1
    return ref, S, 2 + terms


def ppm_pool_slices(B, ncells):
    """tss_ppm_pool_slices: row slices per window"""
    w = B * ncells
    if w <= 0 or w > 128:
        return 1
    return min(cdiv(1024, w), 256)


def ppm_slice_rows(y0, y1, S):
    """the rows [a, b) of slice sl = 0 .. S - 1 of a window [y0, y1) in ppm_pool_fwd_kernel (empty where S exceeds the rows)"""
    return [(y0 + (y1 - y0) * sl // S, y0 + (y1 - y0) * (sl + 1) // S) for sl in range(S)]


# --- attention gates (csrc/gate.hip)
def gate_slices(B, HW):
    """tss_gate_slices: min(ceil(1024 / B), ceil(HW / 64)), at least 1"""
    if B <= 0 or HW <= 0:
        return 1
    return max(1, min(cdiv(1024, B), cdiv(HW, 64)))


def gate_slice_walk(HW, S):
    """[q0, q1) of every slice of gate_bwd_kernel: per = ceil(HW / S) pixels, the last ones ragged or empty"""
    per = cdiv(HW, S)
    return [(min(sl * per, HW), min(sl * per + per, HW)) for sl in range(S)]


def gate_chain(HW, S, C):
    """f32 chain of da's sum: a lane adds the products (EXACT: two 8-bit significands) of ceil(per / NPL) pixels, one thread adds the
    NPL lanes, gate_bwd_reduce_kernel the S slices"""
    NPL = 256 // (C // 8)
    return cdiv(cdiv(HW, S), NPL) + NPL + S


def sigmoid_rel_err(a):
    """relative error bound of sigm(a) = 1.f / (1.f + __expf(-a)) in units of u = 2^-24, elementwise.
    __expf(x) is __builtin_amdgcn_exp2f(0x1.715476p+0f * x) (clang's __clang_hip_math.h, which the HIP math API reference lists under
    the fast intrinsics): the constant is log2(e) within u, the product rounds once, so the argument of exp2 is off by <= 2 u (1 + u)
    |x| log2(e) and the value by the factor exp2 of that: <= 2 u (1 + u) |x| log2(e) ln(2) (1 + ..) <= 2.01 u |x|; V_EXP_F32 itself is
    accurate to 1 ulp <= 2 u (CDNA4 ISA guide).  Together E = __expf(-a) has relative error <= (2 + 2.01 |a|) u (1 + 2^-20).
    1 + E rounds once (u), the division is correctly rounded (u); d s / s = -E / (1 + E) dE / E, and E / (1 + E) < 1:
        rel(s) <= (2 + 2.01 |a| + 2) u (1 + 2^-20) <= (4.01 + 2.02 |a|) u.
    a == 0: exp2(0) = 1, s = 0.5: no error at all"""
    r = 4.01 + 2.02 * a.abs()
    return torch.where(a == 0, torch.zeros_like(r), r)


def gate_fwd_bound(x, a, add_one, bf16):
    """out = x * (s + add_one): |out - ref| <= |x| s rel(s) u  [the sigmoid]  + (add_one: u (s + 1) |x|: the sum rounds)
    + u |out| (the product) + 2^-8 (1 + 2^-20) |out| for bf16.  Where a == 0 the factor is 0.5 or 1.5 and the product of an 8-bit x with
    it is exact: the bound is the bf16 rounding alone (f32: 0, bit for bit)"""
    s = torch.sigmoid(a)
    ref = x * (s + add_one)
    b = x.abs() * s * sigmoid_rel_err(a) * U32 + torch.where(a == 0, torch.zeros_like(ref), ((s + 1) * x.abs() * add_one + ref.abs()) * U32 * 1.001)
    if bf16:
        b = b + 2.0 ** -8 * (ref.abs() + b)
    return ref, b


def gate_da_bound(t, tabs, a, chain, bf16):
    """da = fl(fl(t sg) fl(1 - sg)), t the f32 slice sum (gamma_chain on sum|g x|): sg has rel(s) u, 1 - sg the absolute error
    sg rel(s) u + u (1 - sg), i.e. relative (e^a rel(s) + 1) u, and the two products round once each.  a == 0: sg = 1 - sg = 0.5, the
    products are shifts: only the sum's error"""
    s = torch.sigmoid(a)
    ref = t * s * (1 - s)
    rel = sigmoid_rel_err(a)
    relp = torch.where(a == 0, torch.zeros_like(rel), rel + rel * torch.exp(a) + 1 + 2)
    b = (2.0 ** -23 * chain * tabs * s * (1 - s) + ref.abs() * relp * U32) * 1.001
    if bf16:
        b = b + 2.0 ** -8 * (ref.abs() + b)
    return ref, b


# --- the cases of tests/test_gpu_resample_exact.py and their operands, shared with the f32 emulations of tests/test_exact_bounds.py
#               Hin Win Hout Wout C  tier
RS_BILINEAR = [(5, 9, 17, 33, 8, 1), (2, 3, 17, 33, 24, 1), (13, 21, 32, 50, 8, 2), (17, 33, 6, 11, 24, 2), (7, 9, 7, 9, 8, 1),
               (1, 9, 17, 33, 8, 1), (5, 1, 17, 33, 24, 1), (5, 9, 1, 33, 8, 1), (5, 9, 17, 1, 8, 1), (1, 1, 12, 20, 24, 1), (3, 4, 12, 20, 8, 2)]
#           w   W  instance       7 sx
RS_HEAD = [(11, 72, 'three'),     # 0.986
           (3, 16, 'three'),      # 0.933
           (2, 8, 'four'),        # exactly 1.0
           (10, 64, 'four'),      # 1.0
           (5, 16, 'four'),       # 1.867
           (3, 8, 'generic'),     # 2.0
           (10, 32, 'generic'),   # 2.03
           (6, 24, 'four')]       # 1.52: the smallest pair whose lanes READ the fourth column (none of the seven above does:
#                                   at 5 -> 16 the clamp at the last source column keeps the second lane within three)
#           H   W   C   bins
RS_POOL = [(13, 21, 24, 1), (13, 21, 24, 2), (13, 21, 24, 3), (13, 21, 24, 6),     # NPL = 85 with idle lanes; overlapping windows
           (4, 5, 8, 6),                                                           # bins > H: one-pixel windows repeat
           (13, 21, 8, 2),                                                         # NPL = 256 > the 77 pixels of a window
           (3, 4, 2048, 2)]                                                        # NPL = 1
#               B  bins          H   W   C   workspace  S
RS_PPM_POOL = [(2, (1, 2, 3, 6), 13, 21, 24, False, 1),
               (1, (1, 2, 3, 6), 13, 21, 24, True, 21),       # the 6-bin windows are 3 rows high: most of their slices are empty
               (1, (1,), 13, 21, 8, True, 256),               # S > H
               (3, (2, 3), 13, 21, 16, True, 27)]
#           B  HW   C   slices
RS_GATE = [(2, 35, 8, 1), (3, 200, 24, 4), (2, 130, 8, 3), (1, 130, 24, 3)]      # 130 / 3: slices of 44, 44 and a ragged 42


def case_gen(*key):
    """the generator of a case, seeded by its parameters"""
    s = 17
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def narrow(shape, g, zero_frac=0.0):
    """4 significant bits, multiples of 2^-4 below 2: the operands of the tier-1 gathers"""
    return dyadic_q(shape, g, 4, -1, 1, zero_frac)


def resize_tier1(x, S, pairs):
    """the tier of a case from its own operands: every (n_in, n_out) pair exact_resize and the budget of sum|terms| S"""
    ks = [exact_resize(a, b) for a, b in pairs]
    return all(k is not None for k in ks) and exact_budget(S, lsb_exp(x), sum(ks))


def bilinear_fwd_operand(Hi, Wi, Ho, Wo, C, B=2):
    return dyadic((B, C, Hi, Wi), case_gen(1, Hi, Wi, Ho, Wo), zero_frac=0.03)


def bilinear_bwd_operand(Hi, Wi, Ho, Wo, C, tier, B=2):
    g = case_gen(2, Hi, Wi, Ho, Wo)
    return narrow((B, C, Ho, Wo), g, 0.03) if tier == 1 else dyadic((B, C, Ho, Wo), g, zero_frac=0.03)


def concat_slab_faults(s, e, xc, rows):
    """what is wrong with the statistics slab an arm of tss_ppm_concat_bwd leaves, [] if nothing: s [512][2 ca] f64, e the STORED
    gradient rows [rows][ca], xc = raw - mean"""
    faults = []
    if torch.isnan(s).any():
        faults.append('a slab row neither written nor zeroed')
    if not bool((s[rows:] == 0).all()):
        faults.append('a slab row beyond B bins^2 holds a value')
    if not torch.equal(s[:rows], torch.cat([e, e * xc], 1)):
        faults.append('slab rows differ from (t, t (raw - mean))')
    return faults


RS_BINS = (1, 2, 3, 6)
RS_LINK = (False, True, False, True)       # the arm has a BatchNorm link (mean, scale, beta) or none (the null-pointer path, also on
RS_RELU = (1, 1, 0, 0)                     # the one-bin arm): unlinked + ReLU, linked + ReLU on 2 bins, unlinked, linked without ReLU


class ArmOperands:
    """the arms' raw tensors [B][ca][bins][bins] of tss_ppm_concat_* with their links (mean, scale, beta or None), the pre-activation
    (exact zeros planted), the activation as the kernel rounds it (bf16: rne_bf16; f32: not at all) and xc = raw - mean.  Tier 1: narrow
    operands and scales 1 or 2: the pre-activations are multiples of 2^-4 below 10, which bf16 holds, so nothing is rounded in either
    dtype and exact_budget holds with lsb = -4"""
    def __init__(self, g, B, ca, tier, bf16, binss=RS_BINS, link=RS_LINK, relu=RS_RELU):
        draw = (lambda s: narrow(s, g)) if tier == 1 else (lambda s: dyadic(s, g))
        self.binss, self.link, self.relu, self.ca, self.B = binss, link, relu, ca, B
        self.raw, self.links, self.pre, self.act, self.xc = [], [], [], [], []
        for bins, lk, rl in zip(binss, link, relu):
            raw = draw((B, ca, bins, bins))
            if lk:
                mean, beta = draw((1, ca, 1, 1)), draw((1, ca, 1, 1))
                scale = pow2((1, ca, 1, 1), g, 1, 2) if tier == 1 else pow2((1, ca, 1, 1), g, 0.5, 4)
                raw = plant_zeros(raw, mean, scale, beta, g, 0.1)
                pre = pre_act(raw, mean, scale, beta)
                self.links.append([mean, scale, beta])
                self.xc.append(raw - mean)
            else:
                raw = torch.where(torch.rand(raw.shape, generator=g, dtype=torch.float64) < 0.1, torch.zeros_like(raw), raw)
                pre = raw
                self.links.append([None, None, None])
                self.xc.append(raw)
            a = exact_f32(pre.clamp_min(0.0) if rl else pre)
            self.raw.append(raw)
            self.pre.append(pre)
            self.act.append(rne_bf16(a) if bf16 else a)
        assert sum(int((p == 0).sum()) for p in self.pre) > 0, 'no exact zero of a pre-activation planted'


def concat_gather_chain(bins, H, W, ca):
    """ppm_concat_bwd_kernel: the weight product and the term round once each, a lane adds ceil(n / NPL) terms of the window's n, one
    thread the min(n, NPL) lanes that hold one (the others add an exact 0)"""
    n = window_len(bins, H) * window_len(bins, W)
    NPL = 256 // (ca // 8)
    return 2 + cdiv(n, NPL) + min(n, NPL)


# --- the arms of the pyramid (csrc/ppm.hip, forward): one block per arm, 1x1 convolution on the matrix unit + batch statistics
#           C    Ca  P per arm          training
RS_ARMS = [(32, 16, (3, 12, 27, 108), 1), (128, 32, (3, 12, 27, 108), 1), (128, 16, (512, 1), 1), (32, 32, (512, 1, 130), 1),
           (32, 16, (3, 12, 27, 108), 0), (128, 32, (512, 1), 0)]
ARMS_EPS, ARMS_MOMENTUM = float(np.float32(1e-5)), 0.1          # eps as the f32 the entry receives


def arms_operands(C, Ca, Ps, seed=0):
    """per arm: x [P][C] and w [Ca][C] (bf16-exact, so every product is exact), gamma, running mean / variance (f32-exact)"""
    g = case_gen(15, C, Ca, len(Ps), seed)
    return [dict(x=dyadic((P, C), g, zero_frac=0.03), w=dyadic((Ca, C), g, emin=-6, emax=-2), gamma=dyadic((Ca,), g),
                 rmean=dyadic((Ca,), g), rvar=dyadic((Ca,), g).abs(), P=P) for P in Ps]


def arms_stats_chain(P):
    """ppm_arms_fwd_kernel: lane (wave, fr) adds its pixel of every 64-pixel tile in f32 (ceil(P / 64) additions), row16_sum adds the
    16 lanes of a row in 4 levels; the 4 waves meet in f64"""
    return cdiv(P, 64) + 4


def arms_vec_ref(yq, gamma, rmean, rvar, eps=ARMS_EPS, momentum=ARMS_MOMENTUM):
    """(reference, bound) per output of the training-mode finalize, from the STORED y (yq [P][Ca], f64 of the bf16 bits): mean, invstd,
    gamma invstd, running mean, running variance.  With g = gamma_chain (<= 2^-23 chain), the f32 sums obey |s - sum y| <= g sum|y| and
    |ss - sum y^2| <= g sum y^2 (y y is exact: 16 bits).  Everything after is f64 (2^-48 relative covers it) until the f32 stores:
      mean    Em = g sum|y| / P                                        stored: + u |mean|
      var     Ev = g sum y^2 / P + 2 |mean| Em + Em^2                  (clamped at 0: 1-Lipschitz)
      invstd  f(v) = (v + eps)^-1/2, |f'| <= (vmin + eps)^-3/2 / 2 on [vmin, ..], vmin = max(var - Ev, 0):  Ei = that times Ev; + u f
      scale   gamma * invstd_f32 rounds once:  |gamma| (Ei + u f) + u |gamma f|
      running (1.f - m) r + m v in f32: 1.f - m rounds, two products, one sum (or an FMA): <= 3 u (|(1 - m) r| + |m v|), + m times v's
              own error; the variance enters unbiased, var P / (P - 1) (P = 1: var), rounded to f32 first"""
    P = yq.shape[0]
    g = 2.0 ** -23 * arms_stats_chain(P)
    tiny = 1 + 2.0 ** -40
    mean, sa, sq = yq.sum(0) / P, yq.abs().sum(0) / P, (yq * yq).sum(0) / P
    Em = g * sa * tiny
    var = (sq - mean * mean).clamp_min(0.0)
    Ev = (g * sq + 2 * mean.abs() * Em + Em * Em) * tiny + 2.0 ** -48 * (sq + mean * mean)
    inv = (var + eps) ** -0.5
    Ei = 0.5 * ((var - Ev).clamp_min(0.0) + eps) ** -1.5 * Ev * tiny
    bm, bi = Em + U32 * mean.abs() * tiny, Ei + U32 * inv * tiny
    m32 = float(np.float32(momentum))
    keep = float(np.float32(1.0) - np.float32(momentum))           # fl(1.f - momentum), as the kernel forms it
    unb = var * (P / (P - 1.0) if P > 1 else 1.0)
    bu = Ev * (P / (P - 1.0) if P > 1 else 1.0) + U32 * unb * tiny
    run = lambda r, v, bv: (keep * r + m32 * v, 3.01 * U32 * ((keep * r).abs() + (m32 * v).abs() + m32 * bv) + m32 * bv)
    return dict(mean=(mean, bm), invstd=(inv, bi), scale=(gamma * inv, gamma.abs() * bi + U32 * (gamma * inv).abs() * tiny),
                rmean=run(rmean, mean, bm), rvar=run(rvar, unb, bu))


# --- the arms of the pyramid, backward (ppm_arms_bwd_kernel): tier 3
#               C    Ca  P per arm          training  accumulate
RS_ARMS_BWD = [(32, 32, (130, 3), 1, 0),                 # a second pixel chunk with 2 live pixels
               (128, 16, (512, 1), 1, 1),                # the MAXU edge; Ca = 16: the zeroed upper half of the k-step; count = 1
               (32, 16, (3, 12, 27, 108), 1, 1),
               (128, 32, (130,), 1, 0),
               (32, 32, (130, 512), 0, 1),               # eval: gamma invstd a power of two, g = ga e exact
               (128, 16, (3, 12, 27, 108), 0, 0)]
NEAR_TIE_CAP = 0.01


def arms_bwd_operands(C, Ca, Ps, training, accumulate):
    """per arm: e, y [P][Ca], x [P][C], w [Ca][C] (bf16-exact), mean (dyadic: y - mean is exact in f32), gamma and invstd -- dyadic in
    training mode, powers of two in eval mode (g = gamma invstd e is then a shift of e: exact) -- and the dyadic prior contents of dw,
    dgamma, dbeta the launch adds onto when `accumulate`"""
    g = case_gen(16, C, Ca, len(Ps), training, accumulate)
    ops = []
    for P in Ps:
        o = dict(P=P, e=dyadic((P, Ca), g, zero_frac=0.03), y=dyadic((P, Ca), g), x=dyadic((P, C), g, zero_frac=0.03),
                 w=dyadic((Ca, C), g, emin=-6, emax=-2), mean=dyadic((Ca,), g))
        if training:
            o.update(gamma=dyadic((Ca,), g), invstd=dyadic((Ca,), g).abs())
        else:
            o.update(gamma=pow2((Ca,), g, 0.5, 2), invstd=pow2((Ca,), g, 0.25, 4))
        o.update(dw0=dyadic((Ca, C), g), dgamma0=dyadic((Ca,), g), dbeta0=dyadic((Ca,), g))
        ops.append(o)
    return ops


def bf16_of_f64(v):
    """(v rounded ONCE to bf16, nearest even; the bf16 ulp at v; the distance of v to the nearest rounding tie), all f64.  frexp gives
    |v| = m 2^e with m in [1/2, 1): 8 significant bits are multiples of 2^(e - 8), ties sit half way between them"""
    m, e = torch.frexp(v.abs())
    ulp = torch.ldexp(torch.full_like(v, 2.0 ** -8), e)
    t = m * 256
    q = torch.sign(v) * torch.round(t) * ulp
    return q, ulp, ((t - torch.floor(t)) - 0.5).abs() * ulp


def arms_bwd_ref(o, training, accumulate):
    """references and bounds of one arm of tss_ppm_arms_bwd, {name: (reference, bound)} + 'near' (the near-tie mask of g).
    se = sum e and sey = sum e (y - mean) are f64 sums of exact terms (y - mean is exact in f32, the product of two f32 numbers exact in
    f64): 2^-40 sum|terms| covers any order.  dg = invstd sey, db = se, k = gamma invstd (exact in f64).
      dgamma, dbeta   (float) of the f64 value (u), added onto the prior in f32 when accumulate (u of the sum)
      vec[3..5]       ga = fl(k); training: gb = fl(-k (dg / P) invstd), gce = fl(db / P); eval: 0, 0.  u each + the sums' 2^-40
      g               line 293 of ppm.hip: ga (e - gce) + gb (y - mean) in f32, then ONE bf16 rounding.  Against the f64 g of the f64
                      coefficients the f32 value is off by at most Eg: with A = |ga (e - gce)|, B = |gb (y - mean)|
                        e - gce rounds (u A), gce is off by u |gce| (u |ga gce|), ga by u |ga| (u A), the product rounds (u A),
                        gb is off by u |gb| (u B), its product rounds (u B), the sum (or FMA) rounds (u (A + B))
                      Eg = 1.01 u (4 A + 3 B + |ga gce|).  Eval mode: ga is a power of two and gb = gce = 0: g = ga e, Eg = 0.
      tier 3          an element whose f64 g lies closer than Eg to a bf16 rounding tie may round either way: it contributes ONE bf16 ulp
                      of itself times |w| (e_in) or |x| (dw) to the bound of every sum it enters; every other element rounds as the
                      reference does and contributes nothing.  At most NEAR_TIE_CAP of the elements may be near a tie (asserted from
                      the reference alone in tests/test_exact_bounds.py): a cap on the allowance, not a tolerance
      e_in            conv_excess with K = Ca on the rounded g (exact products), + the allowance (1 + 2^-8)
      dw              wgrad_excess with chain = ceil(P / 32) MFMA steps + 1 (the addition onto the prior / the zero), + the allowance"""
    P, Ca = o['e'].shape
    e, x, w, r = o['e'], o['x'], o['w'], o['invstd']
    xc = exact_f32(o['y'] - o['mean'])
    noise = 2.0 ** -40
    se, sea, sey, seya = e.sum(0), e.abs().sum(0), (e * xc).sum(0), (e * xc).abs().sum(0)
    dg, db, k = r * sey, se, o['gamma'] * r
    if training:
        ga, gb, gce = k, -k * (dg / P) * r, db / P
    else:
        ga, gb, gce = k, torch.zeros_like(k), torch.zeros_like(k)
    u = 1.001 * U32
    out = dict(ga=(ga, u * ga.abs()), gb=(gb, u * gb.abs() + noise * (k * r * r).abs() * seya / P), gce=(gce, u * gce.abs() + noise * sea / P))
    for name, v, va, prior in (('dgamma', dg, r * seya, o['dgamma0']), ('dbeta', db, sea, o['dbeta0'])):
        ref = v + prior if accumulate else v
        out[name] = (ref, noise * va + u * v.abs() + (u * ref.abs() if accumulate else 0.0))
    g64 = ga * (e - gce) + gb * xc
    A, B = (ga * (e - gce)).abs(), (gb * xc).abs()
    Eg = 1.01 * U32 * (4 * A + 3 * B + (ga * gce).abs()) if training else torch.zeros_like(g64)
    gq, ulp, dist = bf16_of_f64(g64)
    if not training:
        assert torch.equal(gq, g64), 'eval mode: g = ga e is not a bf16 number'
    near = dist < Eg
    allow = near.double() * ulp
    ref, S = gq @ w, gq.abs() @ w.abs()
    out['e_in'] = (ref, 2.0 ** -8 * ref.abs() + 2.0 ** -22 * Ca * S + (1 + 2.0 ** -8) * (allow @ w.abs()))
    ref, S = gq.T @ x, gq.abs().T @ x.abs()
    if accumulate:
        ref, S = ref + o['dw0'], S + o['dw0'].abs()
    out['dw'] = (ref, 2.0 ** -23 * (cdiv(P, 32) + 1) * S + allow.T @ x.abs())
    out['near'] = near
    out['gq'] = gq
    return out


# ---------------------------------------------------------------------------------------------------------- eval bottleneck, affines, joins
# csrc/bneck.hip (tss_bneck_eval_fwd), tss_bn_eval_affine / _batched and tss_join_fwd / tss_join_bwd of csrc/pointwise.hip;
# tests/test_gpu_bneck_exact.py.  The bottleneck has two tiers:
#   1  bit for bit on FIXED-POINT operands.  x, w1, wdw, w3 are multiples of 2^-2 (|x| < 2, |w| < 1), the BatchNorm scales powers of two
#      in [1, 4] and the means and betas multiples of the stage's grid: 2^-4 behind the expand, 2^-6 behind the depthwise layer, 2^-8
#      behind the projection.  Every product and every partial sum of a stage, in ANY order and with or without FMA contraction, is a
#      multiple of the stage's grid and at most S = |scale| sum|terms| + |shift| (+ |x| with the skip) in magnitude: with
#      S < 2^(24 + lsb) (bneck_bits: the bits a stage uses, < 24) nothing rounds in f32.  What rounds is what the kernel rounds on
#      purpose -- D, E at stride 2, y, each to bf16, nearest even -- and bneck_ref rounds at the same points.
#   2  8-bit X.dyadic operands and ordinary BatchNorm values; a forward running error is carried next to the reference (bneck_ref).
BK_CM, BK_LDS = 64, 160 * 1024              # CM and the LDS cap of csrc/bneck.hip
BK_FORMS = {816: (1, 8, 16), 808: (1, 8, 8), 408: (1, 4, 8), 416: (2, 4, 16)}      # TH * 100 + TW -> (stride, TH, TW)


def bneck_lds(S, TH, TW, Cin, Cout):
    """Geo<S, TH, TW>::lds: Xh | E (f32 at stride 1, bf16 at stride 2) | D | 2 x (W1c, W3c, chunk constants) | bn3 | validity"""
    TP, HP = TH * TW, (S * (TH - 1) + 3) * (S * (TW - 1) + 3)
    HPp = (HP + 15) & ~15
    PE = BK_CM * 2 + 16
    PEE = BK_CM * 4 + 16 if S == 1 else PE
    px, cop = ((Cin + 31) & ~31) * 2 + 16, (Cout + 15) & ~15
    kset = (4 * BK_CM + 9 * BK_CM) * 4
    return HPp * px + HPp * PEE + TP * PE + 2 * (BK_CM * px + cop * PE + kset) + 2 * 128 * 4 + HPp * 4


def bneck_route(B, H, W, Cin, Cout, stride):
    """the tile form tss_bneck_eval_fwd launches, TH * 100 + TW (tss_bneck_eval_tile): 4 x 16 at stride 2; 8 x 16 when that makes >= 256
    blocks and fits the LDS; 8 x 8 when that makes >= 200 blocks; else 4 x 8"""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if stride == 2:
        return 416
    if B * cdiv(Ho, 8) * cdiv(Wo, 16) >= 256 and bneck_lds(1, 8, 16, Cin, Cout) <= BK_LDS:
        return 816
    if B * cdiv(Ho, 8) * cdiv(Wo, 8) >= 200:
        return 808
    return 408


def bneck_supported(Cin, Cmid, Cout, stride, residual):
    """tss_bneck_eval_supported for bf16: the channel rules, the residual rule, and the one stride-2 tile form fitting the LDS"""
    if stride not in (1, 2) or Cin < 8 or Cin > 128 or Cin % 8 or Cmid < BK_CM or Cmid % BK_CM or Cout < 16 or Cout > 128 or Cout % 4:
        return False
    if residual and (stride != 1 or Cin != Cout):
        return False
    return stride == 1 or bneck_lds(2, 4, 16, Cin, Cout) <= BK_LDS


class BkCase:
    """one bottleneck case: shape, the tile form it must reach, where the 1x1 weights come from ('shadow': both bf16 copies given;
    'f32': neither, the f32 parameters carry low bits; 'skew': a copy pointer off 16-byte alignment that holds OTHER values -- the entry
    must fall back to the f32 parameter) and the seed of its operands"""
    def __init__(self, form, Cin, Cmid, Cout, B, H, W, res=0, wmode='shadow', seed=0):
        self.form, self.Cin, self.Cmid, self.Cout, self.B, self.H, self.W = form, Cin, Cmid, Cout, B, H, W
        self.stride, self.res, self.wmode, self.seed = BK_FORMS[form][0], res, wmode, seed
        self.Ho, self.Wo = (H - 1) // self.stride + 1, (W - 1) // self.stride + 1

    def __repr__(self):
        return '%d-c%d.%d.%d-b%dx%dx%d-s%d%s-%s' % (self.form, self.Cin, self.Cmid, self.Cout, self.B, self.H, self.W, self.stride,
                                                   'r' if self.res else '', self.wmode)


BK_TIER1 = [
    BkCase(816, 64, 192, 64, 2, 57, 250, res=1),               # 256 blocks exactly, ragged on both axes, three chunks: both sets reused
    BkCase(816, 64, 128, 48, 2, 57, 250, wmode='f32'),
    BkCase(808, 128, 128, 128, 1, 113, 105, res=1),            # 8 x 16 would not fit the LDS
    BkCase(808, 32, 64, 32, 1, 80, 160, wmode='f32'),          # 200 tiles of 8 x 8 exactly, too few blocks for 8 x 16
    BkCase(408, 128, 768, 128, 1, 13, 21, res=1),              # twelve chunks, the widest sums
    BkCase(408, 96, 128, 96, 3, 5, 9, res=1, wmode='skew'),
    BkCase(408, 8, 64, 16, 1, 4, 8),                           # Cin padded 8 -> 32, one chunk: no second set is ever staged; one whole tile
    BkCase(408, 8, 64, 16, 1, 5, 9, wmode='f32'),              # four tiles, three of them one row or one column
    BkCase(408, 40, 128, 20, 1, 1, 9, wmode='f32'),            # Cin padded to 64; Cout 20: a quarter fragment, ldy = 28
    BkCase(408, 40, 128, 20, 1, 9, 1),
    BkCase(408, 40, 128, 20, 1, 13, 21, wmode='skew'),
    BkCase(408, 48, 64, 48, 3, 1, 1, res=1, wmode='f32', seed=3),   # 1 x 1 maps: every halo pixel but one outside the image
    BkCase(408, 48, 64, 48, 3, 5, 9),
    BkCase(416, 64, 128, 96, 1, 9, 33),                        # -> 5 x 17: a second tile on both axes with one row / column
    BkCase(416, 8, 64, 20, 1, 8, 32, wmode='f32'),             # -> 4 x 16: one whole tile, the last halo row and column outside the image
    BkCase(416, 8, 64, 20, 1, 2, 2, seed=1),                   # -> 1 x 1
    BkCase(416, 64, 128, 96, 2, 1, 1, wmode='skew'),           # -> 1 x 1
    BkCase(416, 64, 768, 128, 1, 13, 21),                      # twelve chunks at stride 2 (Cin 128 does not fit the stride-2 tile: BK_REFUSED)
    BkCase(416, 64, 128, 96, 2, 13, 21, wmode='f32'),
    BkCase(808, 96, 64, 96, 2, 57, 250, res=1, wmode='skew'),  # 256 blocks of 8 x 16, which do not fit the LDS at 96 channels
]
BK_TIER2 = [BkCase(816, 64, 192, 64, 2, 57, 250, res=1), BkCase(808, 128, 128, 128, 1, 113, 105, res=1, wmode='f32'),
            BkCase(408, 128, 768, 128, 1, 13, 21, res=1), BkCase(408, 40, 128, 20, 3, 5, 9), BkCase(416, 64, 128, 96, 1, 9, 33),
            BkCase(416, 64, 768, 128, 1, 13, 21, wmode='f32')]
# (Cin, Cmid, Cout, stride, residual) the entry refuses with TSS_ERR_SHAPE.  The last one has legal channel counts but its stride-2 tile
# (a 9 x 33 halo of 128 input channels) needs 211 KB of LDS
BK_REFUSED = [(64, 128, 96, 1, 1), (64, 128, 64, 2, 1), (64, 96, 64, 1, 0), (64, 128, 132, 1, 0), (128, 768, 128, 2, 0)]
BK_ZERO_CAP, BK_ROUNDED_MIN, BK_EPS = 0.70, 0.10, 1e-5


def grid_q(shape, gen, lsb, lim, zero_frac=0.0, pos_frac=0.5):
    """multiples of 2^lsb with 0 < |v| < lim, positive with probability pos_frac; a fraction of exact zeros"""
    n = int(round(lim * 2.0 ** -lsb))
    k = torch.randint(1, n, shape, generator=gen).double()
    s = (torch.rand(shape, generator=gen, dtype=torch.float64) < pos_frac).double() * 2 - 1
    v = s * k * 2.0 ** lsb
    if zero_frac > 0:
        v = torch.where(torch.rand(shape, generator=gen, dtype=torch.float64) < zero_frac, torch.zeros_like(v), v)
    return v


BK_LSB = (-4, -6, -8)          # the grid behind each stage of a tier-1 case


class BkOperands:
    """x [B][Cin][H][W], w1 [Cmid][Cin], wdw [Cmid][3][3], w3 [Cout][Cmid] (f64, exact bf16 values; w1p / w3p: the f32 parameters the
    entry is given, with low bits in wmode 'f32' and 'skew') and per stage either the frozen BatchNorm itself (tier 2: gamma,
    running_mean, running_var, beta as f32 numbers) or its affine (tier 1: bn = [(mean, scale, beta)])"""
    def __init__(self, c, tier, eight_bit=False):
        g = case_gen(71, tier, c.form, c.Cin, c.Cmid, c.Cout, c.B, c.H, c.W, c.stride, c.res, c.seed)
        self.c, self.tier = c, tier
        chans = (c.Cmid, c.Cmid, c.Cout)
        if tier == 1 and not eight_bit:
            self.x = grid_q((c.B, c.Cin, c.H, c.W), g, -2, 2.0)
            self.w1, self.w3 = grid_q((c.Cmid, c.Cin), g, -2, 1.0, 0.5), grid_q((c.Cout, c.Cmid), g, -2, 1.0, 0.5)
            self.wdw = grid_q((c.Cmid, 3, 3), g, -2, 1.0, 0.2)
        else:
            self.x = dyadic((c.B, c.Cin, c.H, c.W), g, -3, 1, 0.02)
            self.w1, self.w3 = dyadic((c.Cmid, c.Cin), g, -5, -2), dyadic((c.Cout, c.Cmid), g, -5, -2)
            self.wdw = dyadic((c.Cmid, 3, 3), g, -3, 0)
        if tier == 1:
            # the shift t = beta - mean scale is drawn on the stage's grid, then beta = t + mean scale: both products are shifts.  Behind
            # the expand t > 0 on about 2/3 of the channels: relu(bn1(0)) instead of 0 outside the image then shows in the border outputs
            self.bn = []
            for i, C in enumerate(chans):
                scale, mean = pow2((C,), g, 1, 4), grid_q((C,), g, BK_LSB[i], 2.0)
                t = grid_q((C,), g, BK_LSB[i], 4.0, pos_frac=0.66 if i == 0 else 0.5)
                self.bn.append((mean, scale, exact_f32(t + mean * scale)))
        else:
            f32 = lambda v: v.float().double()
            u = lambda C, lo, hi: lo + (hi - lo) * torch.rand((C,), generator=g, dtype=torch.float64)
            self.frozen = [(f32(u(C, 0.5, 1.5)), f32(u(C, -0.5, 0.5)), f32(u(C, 0.5, 2.0)), f32(u(C, -0.25, 0.5 if i == 0 else 0.25)))
                           for i, C in enumerate(chans)]          # gamma, running_mean, running_var, beta
        low = (lambda w: w + torch.sign(w) * 2.0 ** -20) if c.wmode != 'shadow' else (lambda w: w)
        self.w1p, self.w3p = exact_f32(low(self.w1)), exact_f32(low(self.w3))
        assert torch.equal(rne_bf16(self.w1p), self.w1) and torch.equal(rne_bf16(self.w3p), self.w3)


def fma_f32(a, b, c):
    """fl32(a b + c), ONE rounding, of f64 vectors that hold f32 numbers (the per-channel shift of csrc/bneck.hip's stage):
    exact rational arithmetic, then the nearest f32 (ties to even) among the f64-rounded candidate and its two neighbours"""
    from fractions import Fraction
    out = []
    for x, y, z in zip(a.tolist(), b.tolist(), c.tolist()):
        t = Fraction(x) * Fraction(y) + Fraction(z)
        f = F32(float(t))
        cands = (f, np.nextafter(f, F32(np.inf)), np.nextafter(f, F32(-np.inf)))
        out.append(float(min(cands, key=lambda q: (abs(Fraction(float(q)) - t), int(q.view(np.uint32)) & 1))))
    return torch.tensor(out, dtype=torch.float64)


def round_interval(v, err):
    """(R(v), bound on |R(k) - R(v)| for every k with |k - v| <= err), R = one bf16 rounding: rounding is monotone, so R(k) lies
    between R(v - err) and R(v + err).  Where no rounding tie lies within err of v the bound is 0: the kernel must store the
    reference's bits; where one does it is the one-ulp flip (plus err's own ulps)"""
    q = bf16_of_f64(v)[0]
    return q, torch.maximum((bf16_of_f64(v - err)[0] - q).abs(), (bf16_of_f64(v + err)[0] - q).abs())


def _gam(n):
    return 2.0 ** -23 * n          # gamma_n <= 2 n u, the convention of this file


def bneck_ref(o, bn, bound=False):
    """The eval bottleneck in f64 with the kernel's rounding points.  bn: [(mean, scale, beta)] per stage, f64 vectors of f32 numbers
    (tier 2: the kernel's own vectors read back); shift = fma_f32(-mean, scale, beta) as `stage` forms it.

        E = relu(bn1(conv1(x))), zero outside the image;  stride 2: E := rne_bf16(E)
        D = rne_bf16(relu(bn2(dw(E))))
        y = rne_bf16(relu(bn3(conv3(D)) + x?))

    bound=False (tier 1): every rounding goes through rne_bf16, which asserts that its argument is an f32 number; 'S' holds the per
    stage S = |scale| sum|terms| + |shift| (+ |x|) for bneck_bits.
    bound=True (tier 2): a forward running error is carried next to every tensor (key 'bound': on |out - y|), u = 2^-24:
      expand     acc1 = f32 sum of Cin exact products (bf16 x bf16):            |acc1 - c1| <= gamma_Cin A1,  A1 = sum|x||w1|
                 e = fl(acc1 s1 + t1), one FMA:                                 err1 = |s1| gamma_Cin A1 (1 + u) + u |e|
                 ReLU is 1-Lipschitz and the validity factor 0 / 1 exact.  Stride 2 rounds E to bf16: round_interval(E, err1)
      depthwise  9 products of an f32 E and an f32 tap, each rounded and added (FMA: one rounding fewer; 18 counted):
                                   |acc2 - c2| <= sum|w| errE + gamma_18 sum|w| (|E| + errE)
                 d = fl(acc2 s2 + t2): err2 = |s2| (that) (1 + u) + u |d|;  D = R(relu(d)): round_interval -- 2^-8 |d| at most, and 0
                 wherever no tie lies within err2 of d
      project    acc3 = f32 sum of Cmid exact products over the chunks:         |acc3 - c3| <= sum|w3| errD + gamma_Cmid sum|w3| (|D| + errD)
                 v = fl(acc3 s3 + t3): err3 = |s3| (that) (1 + u) + u |v|;  the skip is one more f32 addition: + u (|v + x| + err3)
                 y = R(relu(v)): round_interval(relu(v), err3)
    Each stage's error reaches the next through |scale| sum|w| of that stage, as the convolutions of errE / errD with |w| above."""
    Fn, c = torch.nn.functional, o.c
    v4 = lambda t: t.view(1, -1, 1, 1)
    sc = [v4(s) for _, s, _ in bn]
    sh = [v4(fma_f32(-m, s, b)) for m, s, b in bn]
    if not bound:
        for (m, s, b), t in zip(bn, sh):
            assert torch.equal(t.flatten(), b - m * s), 'tier 1: the shift is not exact'
    R = (lambda v: bf16_of_f64(v)[0]) if bound else rne_bf16
    w1, w3, wd = o.w1[:, :, None, None], o.w3[:, :, None, None], o.wdw[:, None]
    dw = lambda t, w: Fn.conv2d(t, w, stride=c.stride, padding=1, groups=c.Cmid)
    r = {}
    # expand
    c1, A1 = Fn.conv2d(o.x, w1), Fn.conv2d(o.x.abs(), w1.abs())
    e = c1 * sc[0] + sh[0]
    S1 = sc[0].abs() * A1 + sh[0].abs()
    E = e.clamp_min(0.0)
    errE = None
    if bound:
        errE = sc[0].abs() * _gam(c.Cin) * A1 * (1 + U32) + U32 * e.abs()
    r['E_f32'] = E
    if c.stride == 2:
        E, errE = round_interval(E, errE) if bound else (R(E), None)
    # depthwise
    c2, A2 = dw(E, wd), dw(E.abs(), wd.abs())
    d = c2 * sc[1] + sh[1]
    S2 = sc[1].abs() * A2 + sh[1].abs()
    Dp = d.clamp_min(0.0)
    if bound:
        pe = dw(errE, wd.abs())
        err2 = sc[1].abs() * (pe + _gam(18) * (A2 + pe)) * (1 + U32) + U32 * d.abs()
        D, errD = round_interval(Dp, err2)
    else:
        D = R(exact_f32(Dp))
    # project
    c3, A3 = Fn.conv2d(D, w3), Fn.conv2d(D.abs(), w3.abs())
    v = c3 * sc[2] + sh[2]
    S3 = sc[2].abs() * A3 + sh[2].abs()
    if bound:
        pd = Fn.conv2d(errD, w3.abs())
        err3 = sc[2].abs() * (pd + _gam(c.Cmid) * (A3 + pd)) * (1 + U32) + U32 * v.abs()
    if c.res:
        v, S3 = v + o.x, S3 + o.x.abs()
        if bound:
            err3 = err3 + U32 * (v.abs() + err3)
    yp = v.clamp_min(0.0)
    if bound:
        y, r['bound'] = round_interval(yp, err3)
        r['err3'] = err3
    else:
        y = R(exact_f32(yp))
    r.update(E=E, Dp=Dp, D=D, yp=yp, y=y, S=(S1, S2, S3))
    return r


def bneck_bits(r):
    """bits of the f32 significand each stage of a tier-1 case uses: log2(max S) - lsb; < 24 means no f32 operation of it rounds"""
    return [math.log2(float(S.max())) - lsb for S, lsb in zip(r['S'], BK_LSB)]


def bneck_exact(o, r):
    """the tier-1 premise of a case from its own operands (X.exact_budget per stage) and that its operands sit on their grids"""
    grids = all(lsb_exp(t) >= -2 for t in (o.x, o.w1, o.wdw, o.w3)) and all(
        lsb_exp(torch.cat([m, b])) >= lsb and bool(((s == 1) | (s == 2) | (s == 4)).all()) for (m, s, b), lsb in zip(o.bn, BK_LSB))
    return grids and all(exact_budget(S, lsb) for S, lsb in zip(r['S'], BK_LSB))


def rounding_census(pre, q):
    """(fraction of the elements their bf16 rounding changes, number of exact ties among them)"""
    return float((pre != q).double().mean()), int(((bf16_of_f64(pre)[2] == 0) & (pre != q)).sum())


def bneck_conditions(o, r):
    """what a tier-1 case must exercise, from the reference alone: output zeros under the cap (ReLU must not hide a stage), both
    roundings at work including ties to even, and relu(bn1(0)) > 0 on at least half of the expanded channels"""
    zeros = float((r['y'] == 0).double().mean())
    (fd, td), (fy, ty) = rounding_census(r['Dp'], r['D']), rounding_census(r['yp'], r['y'])
    m, s, b = o.bn[0]
    pos = float((b - m * s > 0).double().mean())
    ok = zeros <= BK_ZERO_CAP and fd >= BK_ROUNDED_MIN and fy >= BK_ROUNDED_MIN and td >= 1 and ty >= 1 and pos >= 0.5
    return ok, dict(zeros=zeros, rounded_D=fd, ties_D=td, rounded_y=fy, ties_y=ty, positive_shift1=pos)


# --- frozen-BatchNorm affines (bn_eval_affine_kernel, bn_eval_affine_batched_kernel)
AFFINE_U = (3, 4)      # u-counts of invstd and scale, below


def affine_ref(gamma, rmean, rvar, eps):
    """(mean, invstd, scale) in f64 from f64 vectors of f32 numbers, eps the f32 number the entry receives.  The kernel computes
        t = fl(var + eps)  (1 + d1);   r = fl(sqrt(t))  (1 + d2);   invstd = fl(1 / r)  (1 + d3);   scale = fl(gamma invstd)  (1 + d4)
    with |d_i| <= u (correctly rounded sqrt and divide), so invstd = (var + eps)^-1/2 (1 + d1)^-1/2 (1 + d2)^-1 (1 + d3): relative error
    <= u / 2 + u + u + O(u^2) < 3 u, and scale one rounding more: < 4 u.  mean is a copy: bit for bit.  gamma None: scale = invstd"""
    invstd = 1.0 / torch.sqrt(rvar + float(F32(eps)))
    return rmean, invstd, (gamma * invstd if gamma is not None else invstd)


def affine_excess(out, ref, n):
    return ((out - ref).abs() - n * U32 * ref.abs()).max().item()


# --- joins (join_fwd_kernel, join_bwd_kernel)
JOIN_NT, JOIN_FWD_BLOCKS = 256, 512


def join_geometry(P, C, max_blocks=STAT_SLABS):
    """join_geometry of csrc/pointwise.hip: (NPL pixels per block trip, grid).  A lane owns one 8-channel group of pixels
    blk NPL + pl + k grid NPL; the forward's grid cap is 512 blocks, the backward's the slab rows"""
    NPL = JOIN_NT // (C // 8)
    return NPL, max(1, min(cdiv(P, NPL), max_blocks))


def join_P(kind, C):
    """the pixel counts of the join cases, from the restated geometry: one pixel; a block's last lane row idle; the 512-block grid filled
    exactly; five whole sweeps and 7 pixels, so that a lane's second 4-pixel trip is only partly inside"""
    NPL = JOIN_NT // (C // 8)
    return {'one': 1, 'short': max(NPL - 1, 1), 'grid': JOIN_FWD_BLOCKS * NPL, 'second': JOIN_FWD_BLOCKS * NPL * 5 + 7}[kind]


def join_stats_chain(P, C):
    """f32 chain of a lane of join_bwd_kernel<bf16>: one addition per pixel it owns, ceil(P / (grid NPL)); lanes meet in f64 (1 when the
    grid covers P)"""
    NPL, grid = join_geometry(P, C)
    return cdiv(P, grid * NPL)


def join_fwd_ref(a, affa, b=None, affb=None, relu=False):
    """relu?(a' + b'), each branch (v - mean) scale + beta or v itself: every branch and the sum exact in f32 (checked)"""
    br = lambda v, aff: exact_f32(pre_act(v, *aff)) if aff is not None else v
    s = br(a, affa)
    if b is not None:
        s = exact_f32(s + br(b, affb))
    return s.clamp_min(0.0) if relu else s


def join_bwd_ref(dout, out, relu, dscale=1.0):
    """e = dout dscale (a power of two: exact) where out > 0 (or everywhere without ReLU), else 0"""
    e = dout * dscale
    return e * (out > 0).double() if relu else e


# ---------------------------------------------------------------------------------------------------------- fused decoder head
# csrc/loss.hip (upsample_ce_onepass_kernel MODE 0..4, upsample_argmax_kernel, upsample_ce_gather_kernel), csrc/widehead.hip (the
# class-chunked twins), csrc/ohem.hip (the radix select) and csrc/headgeom.h (the band walk and the tile gather they share);
# tests/test_gpu_head_exact.py.  Two tiers (the GPU file names the tier of every case):
#   1  bit for bit: the arg-max kernels on an exact_resize pair with logits that are multiples of 2^-2 in [-8, 8].  Every interpolated
#      logit is then an f32 number whatever the contraction (exact_budget, asserted per case), neither arg-max kernel multiplies by
#      log2 e, and the prediction must be the f64 arg-max (lowest index on ties) at EVERY pixel, the confusion matrix equal.
#   2  derived bound, elementwise: everything with an exponential (per-pixel cross-entropy, loss, gradient) and every size pair that is
#      not exact.  head_pix_bound / head_loss_bound / head_grad_bound below count the roundings; the arg-max of a pair that is not
#      exact follows tests/msflip_ref.margin with K = 1.
# The f64 reference interpolates with bilinear_matrix (exact coordinates).  On an exact_resize pair the kernels' taps ARE those weights
# and the coordinate slack is zero; elsewhere head_slack bounds what the f32 coordinates (both contractions of l1) can move.
HEAD_NT = 256             # NT: output columns of a strip, lanes of a block (csrc/headgeom.h)
HEAD_WROWS = 16           # WROWS: output rows of a band of the wide head
HEAD_WK = 16              # WK: classes per chunk of the wide head (csrc/widehead.hip)
HEAD_WTAB = 1024          # WTAB: floats of the gather-weight table
HEAD_WCM_LDS = 96         # WCM_LDS: classes up to which the wide evaluators count in LDS
HEAD_REG_CAP, HEAD_WIDE_CAP = 24, 256
HEAD_FULL_GRID = 2048     # blocks below which head_geom halves the band


def head_cp(C, wide=False):
    """class pitch of a tile: TSS_WITH_CLASS_REGS (20 up to 20 classes, else 24) for the register kernels, round_up(C, 4) for the wide"""
    return cdiv(C, 4) * 4 if wide else (20 if C <= 20 else 24)


def head_geom(B, C, h, w, H, W, wide=False):
    """head_geom / head_blocks / head_ws_floats of csrc/headgeom.h: strips of NT columns; bands of 64 rows, halved while above 16 and
    B nstrip ceil(H / band_rows) < 2048 (the wide head: always WROWS); the conservative tile extents, in double as the host computes
    them; the class pitch; blocks; floats of the workspace (2 doubles per block, then the tiles)"""
    nstrip = cdiv(W, HEAD_NT)
    band_rows = HEAD_WROWS if wide else 64
    while not wide and band_rows > 16 and B * nstrip * cdiv(H, band_rows) < HEAD_FULL_GRID:
        band_rows //= 2
    nband = cdiv(H, band_rows)
    sy = (h - 1) / (H - 1) if H > 1 else 0.0
    sx = (w - 1) / (W - 1) if W > 1 else 0.0
    tile_rows = min(int((band_rows - 1) * sy) + 3, h)
    tile_cells = min(int((HEAD_NT - 1) * sx) + 3, w)
    cp = head_cp(C, wide)
    nblocks = B * nstrip * nband
    return dict(nstrip=nstrip, band_rows=band_rows, nband=nband, tile_rows=tile_rows, tile_cells=tile_cells, cp=cp, nblocks=nblocks,
                ws_floats=nblocks * 4 + nblocks * tile_rows * tile_cells * cp)


def head_band(geo, band, H):
    """head_band: output rows [ya, yb) of a band"""
    ya = band * geo['band_rows']
    return ya, min(ya + geo['band_rows'], H)


def head_band_rows(h, H, ya, yb):
    """head_band_rows: first / last low-resolution row the block of output rows [ya, yb) touches, on the restated f32 taps"""
    i0, i1, _, _ = ac_taps_np(h, H)
    return int(i0[ya]), int(i1[yb - 1])


def head_strip_cells(w, W, strip):
    """head_strip_cells and the table switch of gather_windows: first cell c0 and cell count of a strip, its live lanes, maxwin =
    (int)(2 / sx) + 6 (NT for sx == 0), wtab = ncell maxwin <= WTAB"""
    i0, i1, _, _ = ac_taps_np(w, W)
    x0 = strip * HEAD_NT
    xl = min(x0 + HEAD_NT - 1, W - 1)
    c0 = int(i0[x0])
    ncell = int(i1[xl]) - c0 + 1
    sx = ac_scale_f32(w, W)
    maxwin = int(F32(2.0) / sx) + 6 if sx > 0 else HEAD_NT
    return dict(c0=c0, ncell=ncell, lanes=xl - x0 + 1, maxwin=maxwin, wtab=ncell * maxwin <= HEAD_WTAB)


ac_window = ac_window_f32     # ac_window of csrc/common.h: the conservative range of outputs whose taps can include a source index


def head_lane_window(w, W, strip, cell):
    """the lanes [lo, hi] of a strip that gather_windows lets the flush sum for the strip's cell `cell`: ac_window of column c0 + cell,
    relative to the strip, clamped to its NT lanes and (with the table) to maxwin"""
    s = head_strip_cells(w, W, strip)
    lo, hi = ac_window(w, W, s['c0'] + cell)
    lo, hi = max(lo - strip * HEAD_NT, 0), min(hi - strip * HEAD_NT, HEAD_NT - 1)
    if s['wtab'] and hi - lo + 1 > s['maxwin']:
        hi = lo + s['maxwin'] - 1
    return lo, hi


def head_longest_window(w, W):
    """longest gather window (lanes) over every strip and cell of a case: the chain of one flush sum"""
    best = 0
    for strip in range(cdiv(W, HEAD_NT)):
        for cell in range(head_strip_cells(w, W, strip)['ncell']):
            lo, hi = head_lane_window(w, W, strip, cell)
            best = max(best, hi - lo + 1)
    return best


def head_band_chain(h, H, band_rows):
    """most output rows of one band that feed one low-resolution row: the chain of a lane's gA / gB / Hh accumulators"""
    i0, i1, _, _ = ac_taps_np(h, H)
    best = 0
    for ya in range(0, H, band_rows):
        rows = np.concatenate([i0[ya:ya + band_rows], i1[ya:ya + band_rows]])
        best = max(best, int(max(((i0[ya:ya + band_rows] == r) | (i1[ya:ya + band_rows] == r)).sum() for r in np.unique(rows))))
    return best


HEAD_KERNELS = ('ce_onepass', 'argmax', 'softhead', 'msflip', 'wide_ce', 'wide_argmax', 'wide_msflip')


def head_read_extent(C, ldl, kernel, guarded=True):
    """channels of a pixel (from its first) that an instance of the family reads.  The two register kernels of loss.hip keep their
    load_row written out over all CP channels when the pitch holds them (ldl >= CP) and take the GUARD instance otherwise, which
    skips the 4-channel groups that start at or past C like headgeom.h's load_row (softhead.hip, msflip.hip): round_up(C, 4).
    widehead.hip loads 8-channel groups that start below C: round_up(C, 8).  guarded=False: loss.hip before the GUARD instances
    existed, CP whatever the pitch -- past the pitch for C <= 16 at ldl = round_up(C, 8), past the buffer at its last pixel"""
    assert kernel in HEAD_KERNELS
    if kernel.startswith('wide'):
        return cdiv(C, 8) * 8
    if kernel in ('ce_onepass', 'argmax'):
        cp = head_cp(C)
        if not guarded or ldl >= cp:
            return cp
    return cdiv(C, 4) * 4


def head_logits(shape, gen):
    """tier-1 logits: multiples of 2^-2 in [-8, 8], bf16-exact (7 significant bits), so the f32 and the bf16 kernels read the same"""
    return torch.randint(-32, 33, shape, generator=gen).double() / 4


def head_labels(B, H, W, C, gen, ignore_index=255):
    """labels in [0, C) with pixels of ignore_index, -1 and 300 (out of range: they do not count) scattered in"""
    t = torch.randint(0, C, (B, H, W), generator=gen)
    r = torch.rand((B, H, W), generator=gen)
    t[r < 0.06] = ignore_index
    t[(r >= 0.06) & (r < 0.08)] = -1
    t[(r >= 0.08) & (r < 0.10)] = 300
    return t


def argmax_lowest(z):
    """arg-max over dim 1, the lowest index among equal maxima (torch.argmax's rule, spelled out)"""
    C = z.shape[1]
    idx = torch.arange(C).reshape(1, C, *([1] * (z.dim() - 2)))
    return torch.where(z == z.max(1, keepdim=True).values, idx, C).min(1).values


class HeadRef:
    """f64 reference of the fused head on low-resolution logits x [B][C][h][w] and int64 labels [B][H][W]:
      z, zabs   the upsampled logits My x Mx^T and their absolute twin My |x| Mx^T (>= |z|: what the blends' roundings scale with)
      arg       arg-max of z, lowest index on ties;  gap: best minus second-best
      valid     label != ignore_index and 0 <= label < C
      lse, pix  log-sum-exp and per-pixel cross-entropy lse - z_t (0 where not valid)
    and, for pixel weights (s, hot) -- tests/wce_ref.py's: s = (1 - eps) w_t + eps W / C, hot_c = (1 - eps) w_t [c == t] + eps w_c / C,
    den = sum_valid w_t; or, with pixw [B][H][W] (OHEM's selection weights), s = pixw, hot_c = pixw [c == t], den = 1 --
      loss      sum_valid (s lse - sum_c hot_c z_c) / den
      S         the loss's twin sum_valid (s |lse| + sum_c hot_c zabs_c)      (= sum omega (|lse| + |z_t|) where no blend cancels)
      ssum      sum_valid s
      g         gs sum_pixels My Mx (s p_c - hot_c) on the low-resolution grid, gs = grad_out / den
      A         its absolute twin gs sum_pixels My Mx (s p_c + hot_c)"""
    def __init__(self, x, labels, weight=None, eps=0.0, ignore_index=255, pixw=None, grad_out=1.0, weighted=True):
        from tests import wce_ref
        B, C, h, w = x.shape
        H, W = labels.shape[-2:]
        self.x, self.labels, self.C, self.size, self.low = x, labels, C, (H, W), (h, w)
        My, Mx = bilinear_matrix(h, H), bilinear_matrix(w, W)
        self.My, self.Mx = My, Mx
        self.z = torch.einsum('oh,bchw,pw->bcop', My, x, Mx)
        self.zabs = torch.einsum('oh,bchw,pw->bcop', My, x.abs(), Mx)
        self.zmax = float(x.abs().max())
        self.arg = argmax_lowest(self.z)
        self.valid = wce_ref.valid_mask(labels, C, ignore_index)
        self.t = labels.clamp(0, C - 1)
        self.lse = torch.logsumexp(self.z, 1)
        v = self.valid.double()
        self.pix = (self.lse - self.z.gather(1, self.t[:, None])[:, 0]) * v
        if weighted:
            self.weights(weight, eps, pixw, grad_out)

    @property
    def gap(self):
        top = self.z.topk(2, dim=1).values if self.C > 1 else torch.cat([self.z, self.z - float('inf')], 1)
        return top[:, 0] - top[:, 1]

    def weights(self, weight=None, eps=0.0, pixw=None, grad_out=1.0):
        """(re)compute loss, S, ssum, den, g, A for other pixel weights on the same logits and labels"""
        C, v = self.C, self.valid.double()
        onehot = torch.zeros_like(self.z).scatter_(1, self.t[:, None], 1.0)
        if pixw is None:
            wv = torch.ones(C, dtype=torch.float64) if weight is None else weight.double()
            wt = wv[self.t] * v
            s = ((1 - eps) * wv[self.t] + eps * wv.sum() / C) * v
            hot = ((1 - eps) * wv[self.t][:, None] * onehot + eps / C * wv[None, :, None, None]) * v[:, None]
            self.den = float(wt.sum())
        else:
            s = pixw.double() * v
            hot = s[:, None] * onehot
            self.den = 1.0
        self.ssum = float(s.sum())
        self.S = float((s * self.lse.abs() + (hot * self.zabs).sum(1)).sum())
        self.loss = float((s * self.lse - (hot * self.z).sum(1)).sum()) / self.den if self.den > 0 else float('nan')
        self.gs = grad_out / self.den if self.den > 0 else 0.0
        p = torch.softmax(self.z, 1) * s[:, None]
        self.T = p + hot
        self.g = self.gs * torch.einsum('oh,bcop,pw->bchw', self.My, p - hot, self.Mx)
        self.A = self.gs * torch.einsum('oh,bcop,pw->bchw', self.My, self.T, self.Mx)
        return self


def ohem_pixel_weights(pix, sel):
    """the weight upsample_ce_onepass_kernel<MODE 2> / wide_ce_kernel<2> derive from a stored per-pixel loss and sel = [mode, cut,
    weight of l > cut, weight of l == cut (top-n mode only)]"""
    mode, cut, wgt, weq = [float(v) for v in sel]
    weq = 0.0 if mode != 0 else weq
    pix = pix.double()
    return torch.where(pix > cut, torch.full_like(pix, wgt), torch.where(pix == cut, torch.full_like(pix, weq), torch.zeros_like(pix)))


def ohem_ref(pix, thresh, n_top):
    """f64 restatement of tss_ohem_select on f32 losses `pix` (>= 0): oracle.recipe.ohem's rule -- v = the (n_top + 1)-th largest; v >
    thresh: the mean of the losses above thresh, else the mean of the n_top largest -- and the params [mode, cut, weight of l > cut,
    weight of l == cut]; ties at v share what is left of n_top evenly.  n_top == 0 in top-n mode: nan, like torch's empty mean"""
    l = pix.double().reshape(-1)
    order = torch.sort(l, descending=True).values
    v = float(order[n_top])
    if v > thresh:
        k = float((l > thresh).sum())
        return float(l[l > thresh].sum()) / k, [1.0, float(thresh), 1.0 / k, 0.0]
    if n_top == 0:
        return float('nan'), [0.0, v, float('inf'), float('nan')]
    above, ties_n = l[l > v], float((l == v).sum())
    ties = n_top - float(above.numel())
    return (float(above.sum()) + ties * v) / n_top, [0.0, v, 1.0 / n_top, ties / (ties_n * n_top) if ties_n > 0 else 0.0]


def head_slack_z(ref):
    """what the f32 coordinates may move one interpolated logit by on a pair that is not exact_resize (0 on one that is).  As
    tests/msflip_ref.margin: the bilinear surface has slope <= 2 zmax per source pixel along each axis, so
        slack_z = 2 zmax (coord_error(h, H) + coord_error(w, W))           (both contractions of l1 are inside coord_error)"""
    from tests import msflip_ref
    (h, w), (H, W) = ref.low, ref.size
    if exact_resize(h, H) is not None and exact_resize(w, W) is not None:
        return 0.0
    return 2.0 * ref.zmax * (msflip_ref.coord_error(h, H) + msflip_ref.coord_error(w, W))


def head_slack(ref):
    """(slack_pix, slack_loss, slack_g [B][C][h][w]) from head_slack_z; all zero on an exact_resize pair.  lse is 1-Lipschitz in the
    logits (max norm): a per-pixel cross-entropy moves by <= 2 slack_z, the loss by <= 2 slack_z ssum / den.
    Gradient: a softmax value moves by <= 2 p_c slack_z (|dp_c| <= 2 p_c (1 - p_c) d); and the gather's own weights are the hat
    function of the coordinate, 1-Lipschitz: a weight of the row axis is off by <= ey = coord_error(h, H) wherever the f32 tap (either
    contraction) or the exact tap reads the row (the support Sy), likewise ex / Sx, so the product My Mx is off by <=
    ey Sy Mx + ex My Sx + ey ex Sy Sx, applied to the |terms| T = s p + hot of the window"""
    from tests import msflip_ref
    sz = head_slack_z(ref)
    if sz == 0.0:
        return 0.0, 0.0, 0.0
    (h, w), (H, W) = ref.low, ref.size
    ey, ex = msflip_ref.coord_error(h, H), msflip_ref.coord_error(w, W)
    Sy = ((ref.My != 0) | (tap_matrix_f32(h, H) != 0) | (tap_matrix_f32(h, H, fused=False) != 0)).double()
    Sx = ((ref.Mx != 0) | (tap_matrix_f32(w, W) != 0) | (tap_matrix_f32(w, W, fused=False) != 0)).double()
    e = lambda a, b: torch.einsum('oh,bcop,pw->bchw', a, ref.T, b)
    sg = 2.0 * sz * ref.A + ref.gs * (ey * e(Sy, ref.Mx) + ex * e(ref.My, Sx) + ey * ex * e(Sy, Sx))
    return 2.0 * sz, (2.0 * sz * ref.ssum / ref.den if ref.den > 0 else 0.0), sg


def head_counts(B, C, h, w, H, W, wide=False):
    """the chain lengths of a case from the restated geometry: Ry = rows of a band that feed one low-resolution row, Lx = the longest
    gather window of lanes, the band height, the tile rows (flushes of a band) and the wide head's chunks"""
    geo = head_geom(B, C, h, w, H, W, wide)
    return dict(Ry=head_band_chain(h, H, geo['band_rows']), Lx=head_longest_window(w, W), band_rows=geo['band_rows'],
                tile_rows=geo['tile_rows'], nchunk=cdiv(C, HEAD_WK) if wide else 0)


def head_lse_err(zmax, C, nchunk=0):
    """roundings (units of u = 2^-24, nats) of one log-sum-exp of C logits of magnitude <= zmax.  The hardware transcendentals
    V_EXP_F32 / V_LOG_F32 / V_RCP_F32 are taken at 1 ulp (<= 2 u relative), the figure sigmoid_rel_err already takes for V_EXP_F32
    from the vendor's ISA guide; it has not been measured here.
      8 zmax     one interpolated logit in log2 units: the horizontal blend (l0x = 1 - l1x, two products whose magnitudes add up to
                 <= zmax, one sum: 3), the product with LOG2E and LOG2E's own rounding (2), the vertical blend (3); lse is
                 1-Lipschitz in the logits
      2 zmax     the subtractions z_c - m, |z_c - m| <= 2 zmax, as perturbations of the logits
      2          V_EXP_F32 on every term of the sum
      C - 1      the additions of the positive terms
      2 ln C     V_LOG_F32, relative on |log2 sum| <= log2 C
      zmax + ln C    the addition m + log2 sum
    widehead.hip's running maximum and sum add, per chunk, one rescale exp2(mo - mn): the subtraction (2 zmax), V_EXP_F32 (2), the
    product (1) and the carry's addition (1)"""
    return 11.0 * zmax + 1 + C + 3.0 * math.log(C) + nchunk * (2.0 * zmax + 4)


def head_pix_bound(zmax, C, nchunk=0):
    """|pix - ref| <= u (a + b zmax) on an exact pair (+ 2 slack_z elsewhere).  loss.hip MODE 1: d = ((m - z_t) + log2 sum) ln 2 --
    head_lse_err without its last line (m enters through m - z_t), + 8 zmax for z_t, 2 zmax for m - z_t, 2 zmax + ln C for the
    addition, 2 (2 zmax + ln C) for the product with ln 2 and that constant's rounding: b = 26, a = C + 1 + 5 ln C.  widehead.hip
    MODE 1: (lse - z_t) ln 2 with the running sum: head_lse_err + 8 zmax + 3 (2 zmax + ln C).  The clamp max(d, 0) moves d towards
    the reference, which is >= 0"""
    if nchunk:
        return U32 * (head_lse_err(zmax, C, nchunk) + 14.0 * zmax + 3.0 * math.log(C))
    return U32 * (26.0 * zmax + C + 1 + 5.0 * math.log(C))


def head_grad_counts(n, zmax, C, weighted, nchunk=0):
    """(n_g, r_p) of |dlow - g| <= u (n_g + r_p) A + slack_g (+ 2^-8 (|g| + bound) for a bf16 gradient).
    n_g, the longest f32 chain a term of the gather goes through.  Both halves: l0y = 1 - l1y and its product (2), the Ry additions
    of a band's rows into gA / gB or Hh, g - Hh (1), the gather weight 1 - l1x and its product (2), the Lx additions of the window, up
    to four tiles (4), gs = fl(1 / n) grad_out applied (3): Ry + Lx + 12.  The one-hot half also carries its weight (1 - eps) w_t (2)
    and, smoothed, the row-weight sum Nn (Ry additions), eps / C, Nn eC, its product with w_c and the addition (4):
    n_g = 2 Ry + Lx + 18; with class weights the denominator is an f32 chain of band_rows additions per lane: + band_rows.
    r_p, the roundings of one softmax value times its pixel weight.  Register kernels: 2 (8 + 2) zmax (a softmax value moves by <=
    2 p_c d under a perturbation d of the logits: the interpolation and the subtraction z - m of head_lse_err), V_EXP_F32 on the
    value and on the sum (4), the C - 1 additions, V_RCP_F32 (2), its product with the pixel weight and the product e_c inv (2);
    the pixel weight s = (1 - eps) w_t + eps W / C adds C + 4 (the C - 1 additions of W; eps / C and its product with W; 1 - eps and
    its product with w_t; the sum).  widehead.hip: p_c = exp2(z_c - lse) s: head_lse_err for lse, 8 zmax for z_c, 2 zmax + ln C for
    the subtraction (|z_c - lse| <= 2 zmax + ln C), V_EXP_F32 (2), the product with s (1).
    The transcendentals' 1 ulp is the vendor's figure (head_lse_err), not measured here"""
    n_g = 2 * n['Ry'] + n['Lx'] + 18 + (n['band_rows'] if weighted else 0)
    if nchunk:
        r_p = head_lse_err(zmax, C, nchunk) + 10.0 * zmax + math.log(C) + 3
    else:
        r_p = 20.0 * zmax + 4 + (C - 1) + 4
    return n_g, r_p + (C + 4 if weighted else 0)


def head_grad_bound(ref, n, weighted, bf16, nchunk=0, slack=0.0):
    n_g, r_p = head_grad_counts(n, ref.zmax, ref.C, weighted, nchunk)
    k = U32 * (n_g + r_p)
    bound = k / (1 - k) * ref.A + slack
    return bound + (2.0 ** -8 * (ref.g.abs() + bound) if bf16 else 0.0)


def head_loss_counts(n, zmax, C, weighted, nchunk=0):
    """(n_l, r_l) of |loss - ref| <= [u n_l S + u r_l ssum + 2^-50 S] / den + slack: n_l counts the roundings relative to a term's
    magnitude (S sums them), r_l the ones that scale with zmax whatever the term (per unit of pixel weight; ssum sums the weights;
    with unit weights and no smoothing ssum = den <= S / lse and the form is the issue's u (n_l + r_l) S / den).
    loss.hip: the lane's f32 sum takes one addition per row of the band and one subtraction per flush (band_rows + tile_rows); a
    lse term m + log2 sum (1) times its weight (1); a target-logit term sum_c a[c] Hh[c]: the C products and additions (C + 1) on
    Hh's chain (l0y, its product with the weight (1 - eps) w_t: 4; Ry additions; smoothed: Nn's Ry additions and 4 more); the f32
    loss (1) and, weighted, the denominator's chain (band_rows): n_l = 2 band_rows + tile_rows + 2 Ry + C + 10.
    r_l = head_lse_err for the lse + 5 zmax for a horizontally blended row a[c] (the vertical weights are Hh's) + C + 4, weighted.
    widehead.hip sums in f64: a lse term times its weight (2), a target-logit term times its weight (3), the smoothing's sum over
    a chunk (WK + 2), the denominator's chain (WROWS), the f32 loss (1): n_l = WK + WROWS + 8; r_l = head_lse_err + 8 zmax"""
    if nchunk:
        return HEAD_WK + HEAD_WROWS + 8 + (C + 4 if weighted else 0), head_lse_err(zmax, C, nchunk) + 8.0 * zmax
    return 2 * n['band_rows'] + n['tile_rows'] + 2 * n['Ry'] + C + 10 + (C + 4 if weighted else 0), head_lse_err(zmax, C) + 5.0 * zmax


def head_loss_bound(ref, n, weighted, nchunk=0, slack=0.0):
    n_l, r_l = head_loss_counts(n, ref.zmax, ref.C, weighted, nchunk)
    return (U32 * (n_l * ref.S + r_l * ref.ssum) * 1.001 + 2.0 ** -50 * ref.S) / ref.den + slack


# --- the cases (tests/test_exact_bounds.py asserts from the restated geometry that each reaches what it is listed for)
class HeadCase:
    """(B, C, h, w) -> (H, W) at pitch ldl (default round_up(C, 8)); tier 1: an exact_resize pair with planted ties"""
    def __init__(self, name, B, C, h, w, H, W, ldl=None, wide=False, dtypes=('f32', 'bf16')):
        self.name, self.B, self.C, self.h, self.w, self.H, self.W, self.wide, self.dtypes = name, B, C, h, w, H, W, wide, dtypes
        self.ldl = ldl or cdiv(C, 8) * 8
        self.exact = exact_resize(h, H) is not None and exact_resize(w, W) is not None

    def geom(self):
        return head_geom(self.B, self.C, self.h, self.w, self.H, self.W, self.wide)

    def counts(self):
        return head_counts(self.B, self.C, self.h, self.w, self.H, self.W, self.wide)

    def strips(self):
        return [head_strip_cells(self.w, self.W, s) for s in range(cdiv(self.W, HEAD_NT))]

    def __repr__(self):
        return self.name


HEAD_REG = [HeadCase('one_lane_strip', 1, 19, 5, 33, 33, 257),      # two strips, the second of one lane; three bands, the last of one row
            HeadCase('no_table', 1, 19, 9, 129, 17, 257),            # sx = 1/2: strip 0 gathers without the table, strip 1 with it
            HeadCase('identity', 1, 19, 18, 300, 18, 300),           # a flush on every row, rB == rA at the end; 16 + 2 rows, 256 + 44 lanes
            HeadCase('few_class', 2, 5, 3, 5, 9, 17),                # ldl = 8 < CP: the GUARD instances
            HeadCase('c20', 1, 20, 3, 3, 17, 17),                    # CP 20 with no pad class
            HeadCase('cp24', 1, 21, 5, 9, 33, 65),                   # CP 24 with pad classes
            HeadCase('c24', 1, 24, 3, 3, 17, 17),                    # CP 24, pitch equal to CP
            HeadCase('h1', 1, 19, 1, 5, 17, 33),
            HeadCase('w1', 1, 19, 5, 1, 33, 17),                     # sx = 0: the window is the whole strip
            HeadCase('pitch32', 1, 19, 5, 9, 33, 65, ldl=32),
            HeadCase('band32', 16, 19, 513, 3, 4097, 5),             # band_rows = 32, the benchmark's; 129 bands, the last of one row
            HeadCase('band64', 32, 19, 513, 3, 4097, 5, dtypes=('f32',))]
HEAD_REG_T2 = [HeadCase('prod', 2, 19, 16, 32, 128, 256), HeadCase('near', 1, 19, 15, 29, 16, 32), HeadCase('edge', 1, 19, 5, 7, 40, 56)]
HEAD_WIDE = [HeadCase('c25', 1, 25, 5, 33, 33, 257, wide=True),
             HeadCase('c33', 1, 33, 3, 5, 9, 17, wide=True),         # a one-class chunk
             HeadCase('c66', 2, 66, 3, 5, 17, 33, wide=True),
             HeadCase('c130', 1, 130, 18, 300, 18, 300, wide=True),
             HeadCase('c256', 1, 256, 3, 3, 9, 9, wide=True),
             HeadCase('c97', 1, 97, 3, 5, 9, 17, wide=True)]         # the first count past the LDS counters
HEAD_WIDE_T2 = [HeadCase('wide_t2', 2, 66, 6, 9, 48, 72, wide=True)]
HEAD_BY_NAME = {c.name: c for c in HEAD_REG + HEAD_REG_T2 + HEAD_WIDE + HEAD_WIDE_T2}
HEAD_TIE_PAIRS = ((3, 4), (19, 20), (0, 1), (1, 2))           # across the 4-class register groups; with class 0
HEAD_TIE_PAIRS_WIDE = ((15, 16), (0, 255), (0, 1), (3, 4))    # across the 16-class chunks; the first and the last class


def head_plants(x, gen):
    """plant ties into tier-1 logits x [B][C][h][w] (in place), each at sites of its own: for every pair (a, b) of HEAD_TIE_PAIRS
    (HEAD_TIE_PAIRS_WIDE past 24 classes) the case has classes for, as far as its sites go round, (i) two equal planes over a horizontal cell pair -- a = b = 8 there, every other class <= 7.75 -- and (ii) a
    tie that exists only after interpolation -- a goes 0 -> 4 across the cell pair, b 4 -> 0, the others <= 1.75: equal (2) at the
    midpoint only; and one low-resolution pixel where every class holds 1.  With w == 1 the sites are single pixels and (ii) is
    left out.  Returns [(kind, a, b, r, c)]"""
    B, C, h, w = x.shape
    step = 2 if w > 1 else 1
    sites = [(r, c) for r in range(h) for c in range(0, w - step + 1, step + 1)]
    perm = torch.randperm(len(sites), generator=gen).tolist()
    sites = [sites[i] for i in perm]
    pairs = [p for p in (HEAD_TIE_PAIRS_WIDE if C > HEAD_REG_CAP else HEAD_TIE_PAIRS) if p[1] < C]
    plants = [('planes',) + p for p in pairs] + ([('cross',) + p for p in pairs] if w > 1 else []) + [('all', 0, C - 1)]
    done = []
    for k, (kind, a, b) in enumerate(plants):
        for (r, c) in sites[k::len(plants)][:3]:
            cols = slice(c, c + step)
            if kind == 'planes':
                x[:, :, r, cols] = x[:, :, r, cols].clamp(max=7.75)
                x[:, a, r, cols] = 8.0
                x[:, b, r, cols] = 8.0
            elif kind == 'cross':
                x[:, :, r, cols] = x[:, :, r, cols].clamp(max=1.75)
                x[:, a, r, c], x[:, a, r, c + 1] = 0.0, 4.0
                x[:, b, r, c], x[:, b, r, c + 1] = 4.0, 0.0
            else:
                x[:, :, r, c] = 1.0
            done.append((kind, a, b, r, c))
    return done


def head_inputs(case, seed=0):
    """(x [B][C][h][w] f64 tier-1 logits, labels [B][H][W] int64, plants); tier-2 pairs carry no plants"""
    g = case_gen(*[ord(ch) for ch in case.name], seed)
    x = head_logits((case.B, case.C, case.h, case.w), g)
    plants = head_plants(x, g) if case.exact else []
    return x, head_labels(case.B, case.H, case.W, case.C, g), plants


# ---------------------------------------------------------------------------------------------------------- BatchNorm finalize chain
# csrc/bnfin.h (slab_sum, bn_bwd_finalize_block) and csrc/pointwise.hip (bn_finalize_kernel, slab_reduce_kernel, the _sync pair,
# colsum_kernel, cast_weights_kernel), csrc/zoo.hip (tensor_stats_kernel, tensor_stats_vec_kernel); tests/test_gpu_bnfin_exact.py.
# The mask rules of the dropout kernels live in tests/philox_ref.py.  All of this section is numpy: float64 for the kernels' f64
# formulas, float32 (IEEE, one rounding per operation) for their last f32 steps.
#   tier 1  bit for bit.  Slab rows are integers (every f64 sum exact in any order), count = 2^k, the channel sum s an integer of at
#           most 26 bits: mean = s / 2^k and mean^2 are exact, q / 2^k is exact, and var = q / 2^k - mean^2 is a multiple of 2^-2k
#           below 2^4, i.e. an f64 number: the subtraction returns it exactly, and so does an FMA that rounds the exact
#           q / 2^k - mean mean once (fin_tier1_premise checks both with rationals).  Running statistics are 8-bit dyadic and the
#           momentum 2^-3 or 2^-1: (1 - m) rm and m f32(mean) are exact products, so `(1 - m) rm + m x` rounds once with or without a
#           contraction.  invstd alone is held to one f32 rounding of an f64 value, FIN_INVSTD_REL.
#   tier 2  bounded (fin_tier2_bounds): slabs written by tss_tensor_stats from stored 12-bit values with mean ~ 30 and deviation ~ 2^-3.
FIN_CH, FIN_ROWS_PER_LOAD = 8, 16      # channels of a finalize block; FIN_WAVES x FIN_RG rows per load instruction (csrc/bnfin.h)
FIN_INVSTD_REL = 2.0 ** -24 + 2.0 ** -48   # one f32 rounding of the f64 1 / sqrt(var + eps), itself within a few 2^-53
FIN_CHANNELS = (4, 8, 19, 132, 264, 768)


def np_rng(*key):
    s = 29
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return np.random.RandomState(s)


def bn_finalize_ref(s, q, count, gamma, eps, momentum, rmean=None, rvar=None):
    """bn_finalize_kernel / bn_finalize_sync_kernel from the column sums s, q (f64 [C]) in the kernel's operation order:
        mean = s / count;  var = max(q / count - mean^2, 0);  invstd = f32(1 / sqrt(var + f64(eps)));  scale = f32(gamma) *_f32 invstd
        running_mean = (1 - m) rm + m f32(mean)  in f32;  running_var likewise with f32(var count / (count - 1)) (var itself at count 1)
    gamma None: 1.  Returns a dict of numpy arrays: mean64 / var64 / invstd64 (f64, before their f32 rounding), mean / invstd / scale /
    running_mean / running_var (f32)"""
    s, q, count = np.asarray(s, np.float64), np.asarray(q, np.float64), np.float64(count)
    mean = s / count
    var = np.maximum(q / count - mean * mean, 0.0)
    inv64 = 1.0 / np.sqrt(var + np.float64(F32(eps)))
    r = dict(mean64=mean, var64=var, invstd64=inv64, mean=mean.astype(F32), invstd=inv64.astype(F32))
    r['scale'] = bn_scale_ref(gamma, r['invstd'])
    m = F32(momentum)
    if rmean is not None:
        r['running_mean'] = (F32(1) - m) * np.asarray(rmean, F32) + m * r['mean']
    unbiased = var * count / (count - 1.0) if count > 1.0 else var
    r['unbiased64'] = unbiased
    if rvar is not None:
        r['running_var'] = (F32(1) - m) * np.asarray(rvar, F32) + m * unbiased.astype(F32)
    return r


def bn_scale_ref(gamma, invstd32):
    """scale from the STORED invstd bits: one f32 product"""
    invstd32 = np.asarray(invstd32, F32)
    return invstd32.copy() if gamma is None else np.asarray(gamma, F32) * invstd32


def bn_bwd_finalize_ref(se, sey, count, invstd, gamma, training=1, accumulate=0, dgamma=None, dbeta=None, local=None):
    """bn_bwd_finalize_block / bn_bwd_finalize_sync_kernel: r = f64(invstd), k = gamma r,
        dgamma = (acc ? old : 0) +_f32 f32(r sey);  dbeta = (acc ? old : 0) +_f32 f32(se);  ga = f32(k);
        gb = f32(((-k) (r sey / cnt)) r);  gce = f32(se / cnt);  frozen: gb = gce = 0.
    local = (se, sey) of this replica for dgamma / dbeta when (se, sey, count) are the sums over all replicas (the _sync kernel).
    No addition follows the sums in f64, so no contraction can change a bit"""
    se, sey, cnt = np.asarray(se, np.float64), np.asarray(sey, np.float64), np.float64(count)
    lse, lsey = (se, sey) if local is None else (np.asarray(local[0], np.float64), np.asarray(local[1], np.float64))
    r = np.asarray(invstd, F32).astype(np.float64)
    old = lambda v: np.asarray(v, F32) if accumulate else np.zeros(se.shape, F32)
    out = dict(dgamma=old(dgamma) + (r * lsey).astype(F32), dbeta=old(dbeta) + lse.astype(F32))
    k = (np.asarray(gamma, F32).astype(np.float64) if gamma is not None else 1.0) * r
    out['ga'] = k.astype(F32)
    if training:
        c2 = r * sey / cnt
        out['gb'], out['gce'] = (-k * c2 * r).astype(F32), (se / cnt).astype(F32)
    else:
        out['gb'], out['gce'] = np.zeros(se.shape, F32), np.zeros(se.shape, F32)
    return out


def spread_rows(total, rows, rng, zero_half=True):
    """int64 [rows][n] whose columns sum to total (int64 [n]): a random half of the rows all zero (a producer with fewer blocks leaves
    them so), the others total / their number plus a random integer below 2^30 in magnitude, the last of them the remainder"""
    total = np.asarray(total, np.int64)
    nz = np.sort(rng.permutation(rows)[:rows // 2] if zero_half else np.arange(rows))
    v = total // len(nz) + rng.randint(-2 ** 30, 2 ** 30, size=(len(nz), total.size)).astype(np.int64)
    v[-1] += total - v.sum(0)
    out = np.zeros((rows, total.size), np.int64)
    out[nz] = v
    assert (out.sum(0) == total).all() and int(np.abs(out).max()) < 2 ** 40 and int(np.abs(out).sum(0).max()) < 2 ** 53
    return out


def fin_tier1_sums(C, k, rng):
    """(s, q) int64 [C] of a tier-1 case with count 2^k: s of up to min(26, (47 + k) / 2) bits, either sign; q = ceil(s^2 / 2^k) + v,
    v in [1, 2^(k+3)): var in (v - 1, v] 2^-k.  Channel 0: s a multiple of 2^k and q = s^2 / 2^k, var exactly 0.  Channel 1: v =
    -max(2, 2^(k-2)): var in (-1/4, -1/8] (-2 at count 1) BEFORE the clamp, far below -eps: without the clamp invstd is a NaN"""
    tb = min(26, (47 + k) // 2)
    s = rng.randint(2 ** (tb - 2), 2 ** tb, size=C).astype(np.int64) * rng.choice([-1, 1], size=C)
    s[0] = (s[0] >> k) << k if abs(int(s[0])) >> k else 1 << k
    sq = s * s
    up = -((-sq) >> k)                                   # ceil(s^2 / 2^k)
    q = up + rng.randint(1, 2 ** (k + 3), size=C).astype(np.int64)
    q[0] = sq[0] >> k
    if C > 1:
        q[1] = up[1] - max(2, 2 ** (k - 2))
    return s, q


def fin_tier1_premise(s, q, k):
    """mean, mean^2, q / count and q / count - mean^2 are f64 numbers (rationals against floats): the subtraction is exact, and an FMA,
    which rounds the exact q / count - mean mean once, returns the same bits"""
    from fractions import Fraction
    cnt = float(2 ** k)
    for si, qi in zip(s.tolist(), q.tolist()):
        mean = si / cnt
        if abs(si) >= 2 ** 26 or Fraction(mean) != Fraction(si, 2 ** k) or Fraction(mean * mean) != Fraction(si, 2 ** k) ** 2:
            return False
        exact = Fraction(qi, 2 ** k) - Fraction(si, 2 ** k) ** 2
        if Fraction(qi / cnt) != Fraction(qi, 2 ** k) or Fraction(qi / cnt - mean * mean) != exact or Fraction(float(exact)) != exact:
            return False
    return True


def fin_tier1_slabs(C, k, rng, rows=STAT_SLABS):
    """f64 [rows][2 C] slab rows (sums | second moments) of fin_tier1_sums, and the column sums (s, q) as f64"""
    s, q = fin_tier1_sums(C, k, rng)
    assert fin_tier1_premise(s, q, k)
    slabs = spread_rows(np.concatenate([s, q]), rows, rng).astype(np.float64)
    return slabs, s.astype(np.float64), q.astype(np.float64)


def dyadic8_np(n, rng, positive=False):
    """8-bit dyadic f32 values +-(1 + j/128) 2^e, e in [-3, 2): the running statistics of tier 1"""
    v = (1 + rng.randint(0, 128, size=n) / 128.0) * 2.0 ** rng.randint(-3, 2, size=n)
    return (v if positive else v * rng.choice([-1, 1], size=n)).astype(F32)


def fin_bwd_slabs(C, rng, rows=STAT_SLABS):
    """integer slab rows [rows][2 C] of a backward case (sums of e | of e (y - mean)), either sign, column sums below 2^44"""
    tot = rng.randint(-2 ** 43, 2 ** 43, size=2 * C).astype(np.int64)
    slabs = spread_rows(tot, rows, rng).astype(np.float64)
    return slabs, tot[:C].astype(np.float64), tot[C:].astype(np.float64)


def fin_tier2_bounds(ref_var, qc, mean, eps, count, momentum, rmean, rvar):
    """Tier 2: the slab sums are EXACT (12-bit stored values: every term and every partial sum is an f64 integer multiple of 2^-14), so
    only the finalize's own roundings separate its var from the f64 BatchNorm of the stored values: mean = fl(s / count) (relative
    2^-53), fl(q / count) (2^-53), fl(mean mean) (2^-53; none if contracted) and the subtraction (2^-53 |var|):
        |var - var_ref| <= 2^-53 q/count + 3 2^-53 mean^2 (1 + 2^-52) + 2^-53 |var|  <  Dv = 2^-51 (q / count + mean^2).
    invstd: t -> t^-1/2 is convex and decreasing, so a var within Dv of var_ref (clamped at 0, which only moves it towards
    var_ref >= 0) gives |(var + eps)^-1/2 - (var_ref + eps)^-1/2| <= (var_ref + eps - Dv)^-1/2 - (var_ref + eps)^-1/2 = Di; the f64
    sqrt and division and the f32 rounding add FIN_INVSTD_REL of the value.  The running statistics go through at most three f32
    roundings per term (fl(1 - m), a product, the sum; f32(mean) or f32(unbiased), a product, the sum): 4 u (|a| + |b|), u = 2^-24,
    plus m times the error the new statistic inherits.  An f32 variance is off by about 2^-24 mean^2 = 2^27 Dv.
    Returns dict(var, invstd, running_mean, running_var) of f64 bounds"""
    Dv = 2.0 ** -51 * (qc + mean * mean)
    t = ref_var + np.float64(F32(eps))
    Di = (t - Dv) ** -0.5 - t ** -0.5
    inv = t ** -0.5
    m = np.float64(F32(momentum))
    ub = count / (count - 1.0) if count > 1 else 1.0
    return dict(var=Dv, invstd=Di * (1 + FIN_INVSTD_REL) + FIN_INVSTD_REL * inv,
                running_mean=4 * U32 * (np.abs((1 - m) * rmean) + np.abs(m * mean)) + m * 2.0 ** -52 * np.abs(mean),
                running_var=4 * U32 * (np.abs((1 - m) * rvar) + np.abs(m * ref_var * ub)) + m * ub * Dv * 1.001)


def offset_values(P, C, rng):
    """stored values of tier 2, f64 [P][C]: multiples of 2^-7 near 30 (12 significant bits: exact in f32; the squares have 24), standard
    deviation about 2^-3 (16 steps); channel 0 constant, so that its variance is exactly 0"""
    n = np.rint(3840 + 16 * rng.standard_normal((P, C)) + rng.randint(-200, 200, size=C)).astype(np.int64).clip(2049, 4095)
    n[:, 0] = 3872
    return n / 128.0


def exact_moments(x, scale_bits=7):
    """(mean, var, q / count) of the columns of x (multiples of 2^-scale_bits) as correctly rounded f64, through integers"""
    from fractions import Fraction
    n = np.rint(x * 2 ** scale_bits).astype(np.int64)
    assert (n / 2.0 ** scale_bits == x).all()
    P = x.shape[0]
    out = []
    for c in range(x.shape[1]):
        s1, s2 = int(n[:, c].sum()), int((n[:, c] * n[:, c]).sum())
        out.append((float(Fraction(s1, P << scale_bits)), float(Fraction(P * s2 - s1 * s1, (P * P) << (2 * scale_bits))),
                    float(Fraction(s2, P << (2 * scale_bits)))))
    return tuple(np.array(v) for v in zip(*out))


# --- tss_tensor_stats (csrc/zoo.hip)
TS_NT = 256


def tensor_stats_plan(P, C, ldz, aligned=True):
    """('vec' | 'scalar', per, npl): block i of the 512 owns pixels [i per, (i + 1) per).  The vector kernel (C a multiple of 8 up to
    1024, pitch a multiple of 8, 16-byte aligned, P >= 2048): a lane owns 8 channels of every npl-th pixel of the block's range.  The
    scalar kernel sweeps the channels in passes of 256"""
    per = cdiv(P, STAT_SLABS)
    if C % 8 == 0 and C <= TS_NT * 4 and ldz % 8 == 0 and aligned and P >= 4 * STAT_SLABS:
        return 'vec', per, TS_NT // (C // 8)
    return 'scalar', per, None


def tensor_stats_chain(P, C):
    """f32 chain of a lane of tensor_stats_vec_kernel<bf16>: its ceil(per / npl) terms (a bf16 value or its square: exact in f32) and
    one for the step into f64; lanes, blocks and slab rows meet in f64 (the 2^-50 of stats_excess)"""
    _, per, npl = tensor_stats_plan(P, C, 8)
    return cdiv(per, npl) + 1


def block_sums(v, per, rows=STAT_SLABS):
    """f64 [rows][C]: the sums over each block's pixel range [i per, (i + 1) per) of v [P][C]"""
    out = torch.zeros(rows, v.shape[1], dtype=torch.float64)
    if per > 0:
        full = v.shape[0] // per
        out[:full] = v[:full * per].reshape(full, per, -1).sum(1)
        if full < rows and full * per < v.shape[0]:
            out[full] = v[full * per:].sum(0)
    return out


# --- tss_bias_grad (colsum_kernel), tss_cast_weights
def colsum_plan(P):
    """(grid, terms of a lane): blocks of 4 pixel lanes x 64 channels, at most 1024; a lane walks pixels blk 4 + pl + j 4 grid"""
    grid = min(cdiv(P, 4), 1024)
    return grid, cdiv(P, 4 * grid)


def colsum_chain(P):
    """f32 roundings a term of colsum_kernel goes through: the lane's own sum, 3 additions of the four lane rows in LDS, and one f32
    atomic per block onto the same address, in any order"""
    grid, lane = colsum_plan(P)
    return lane + 3 + grid


def colsum_exact_values(P, N, rng, bf16=True):
    """multiples of 2^-6 up to 255/64 in magnitude (8 bits: bf16 numbers): every partial sum of up to 2^16 of them plus the initial
    dbias (a non-zero multiple of 2^-6 below 2^9) is a multiple of 2^-6 below 2^18, an f32 number: f32 additions in any order are exact"""
    assert P * 255 + 2 ** 16 < 2 ** 24
    return rng.randint(-255, 256, size=(P, N)) / 64.0, rng.randint(1, 2 ** 15, size=N) * rng.choice([-1, 1], size=N) / 64.0


def cast_sources(N, K, rng):
    """f32 [N][K] sources of tss_cast_weights: ordinary values, and planted bf16 rounding ties (low half 0x8000, to an even and to an
    odd neighbour), values one f32 ulp past a tie, f32 denormals, the smallest normals, +-0, values that round up into the next binade"""
    v = rng.standard_normal(N * K).astype(F32)
    b = v.view(np.uint32).copy()
    pick = rng.permutation(N * K)
    m = max(1, N * K // 16)
    sl = [pick[i * m:(i + 1) * m] for i in range(7)]
    b[sl[0]] = (b[sl[0]] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)                       # ties, either parity of the kept half
    b[sl[1]] = (b[sl[1]] & np.uint32(0xFFFF0000)) | np.uint32(0x8001)                       # just past a tie
    b[sl[2]] = (b[sl[2]] & np.uint32(0xFFFF0000)) | np.uint32(0x7FFF)                       # just short of one
    b[sl[3]] = (b[sl[3]] & np.uint32(0x80000000)) | rng.randint(1, 2 ** 23, size=len(sl[3])).astype(np.uint32)     # f32 denormals
    b[sl[4]] = (b[sl[4]] & np.uint32(0x80000000)) | np.uint32(0x00800000) | rng.randint(0, 2 ** 17, size=len(sl[4])).astype(np.uint32)
    b[sl[5]] = b[sl[5]] & np.uint32(0x80000000)                                              # +-0
    b[sl[6]] = (b[sl[6]] & np.uint32(0xFF800000)) | np.uint32(0x007FC000)                    # carries into the exponent
    return torch.from_numpy(b.view(F32).reshape(N, K).copy())


# ---------------------------------------------------------------------------------------------------------- soft losses and distillation
# csrc/distill.hip (pixel- and channel-wise KL), then csrc/softloss.hip (planar focal and soft Dice), tss_focal_coef_from_ce and the
# focal and Dice passes of the fused head (csrc/softhead.hip); tests/test_gpu_softloss_exact.py, the f32 emulations in
# tests/softloss_emu.py and tests/head_emu.py and their CPU proofs in tests/test_exact_bounds.py.  The distillation part, first, is numpy float64
# on operands [B][HW][C] that are f32 (and bf16) numbers.
# u = 2^-24.  The hardware V_EXP_F32 is taken at 1 ulp (<= 2 u relative), the figure head_lse_err takes: the vendor's, not measured
# here; logf is the library's (also taken at 1 ulp).  A result below the smallest normal f32 may be flushed: the floors of 2^-126.
DISTILL_NT = 256                 # lsw::NT
DISTILL_PIXEL_BLOCKS = 4096      # default block caps of csrc/distill.hip
DISTILL_CHANNEL_BLOCKS = 512
DISTILL_TAUS = (1.0, 4.0, 0.5, 3.0)       # 1 / tau is exact for the powers of two; fl(1 / 3) carries one rounding, which the reference
DISTILL_FLOOR = 2.0 ** -126               # reads as the entry forms it (inv_tau below), so no case pays for it in the bound


def distill_pixel_grid(P, max_blocks=0):
    """pixel_grid: tss::grid_for(P, NT, cap); the workspace is 2 doubles per block"""
    return max(1, min(cdiv(P, DISTILL_NT), max_blocks if max_blocks > 0 else DISTILL_PIXEL_BLOCKS))


def distill_channel_split(B, C, HW, max_blocks=0):
    """channel_split and Strip of csrc/distill.hip: vectors per row, positions per block and trip, segments per image S (as many as
    the cap allows while it allows one item per image), positions per segment, items, grid, floats of the workspace (5 rows of
    round_up(C, 8) per item: two of maxima, three of sums)"""
    cap = max_blocks if max_blocks > 0 else DISTILL_CHANNEL_BLOCKS
    nch = cdiv(C, 8)
    ppb = DISTILL_NT // nch
    S = min(cdiv(HW, ppb), max(cap // B, 1))
    return dict(nch=nch, ppb=ppb, S=S, len=cdiv(HW, S), items=B * S, grid=min(B * S, cap), ws_floats=5 * 8 * nch * B * S)


def distill_segments(HW, S):
    """[(i0, i1)] of the S segments of a plane; an EMPTY one has i0 >= i1 (its partial rows are the identities -inf and 0)"""
    n = cdiv(HW, S)
    return [(q * n, min(q * n + n, HW)) for q in range(S)]


def distill_depth(kind, B, C, HW, max_blocks=0):
    """additions a term of Z_S, Z_T or A goes through.  pixel: the lane's C.  channel: the lane's trips over its segment, the levels
    of slot_reduce's tree over the ppb position slots, the S partial rows of the finalize"""
    if kind == 'pixel':
        return C
    sp = distill_channel_split(B, C, HW, max_blocks)
    return cdiv(sp['len'], sp['ppb']) + max(sp['ppb'] - 1, 0).bit_length() + sp['S']


class DistillRef:
    """f64 reference of csrc/distill.hip on s, t [B][HW][C] (f64 arrays of f32 numbers), from the f32 scalars the entry forms:
    inv_tau = fl(1 / tau), norm = fl(tau / #units), grad_out as an f32.  x = logit * inv_tau in f64 (exact: 24 x 24 bits); a unit is
    a pixel (axis C) or a plane (axis HW):
      ms, mt        fl(max * inv_tau): what stats[.].x / .z must hold bit for bit (the product is exact in f64, then ONE f32 rounding)
      Ds, Dt        x - m (m the f32 number), <= 0 up to m's rounding
      lzs, lzt      log sum exp(D): what stats[.].y / .w approximate
      q, p          softmax values, exp(D - lz)
      kl, loss      sum p (log p - log q) per unit;  (double)tau^2 / #units * sum kl
      g             norm * grad_out * (q - p)
    and the terms of the bounds: dbs, dbt = sum q |Ds|, sum p |Dt| (what the exponent's roundings weigh on the sum), r = |sum p d|,
    ra = sum p |d| (3 |Dt| + 4 + depth), d = (t - s) inv_tau"""
    def __init__(self, s, t, tau, kind, grad_out=1.0, max_blocks=0):
        B, HW, C = s.shape
        self.kind, self.shape, self.tau = kind, (B, C, HW), float(F32(tau))
        ax = 2 if kind == 'pixel' else 1
        self.ax, self.units = ax, (B * HW if kind == 'pixel' else B * C)
        self.inv = float(F32(1.0) / F32(tau))
        self.norm = float(F32(float(F32(tau)) / self.units))
        self.go = float(F32(grad_out))
        self.depth = distill_depth(kind, B, C, HW, max_blocks)
        xs, xt = s * self.inv, t * self.inv
        self.ms = (s.max(ax, keepdims=True) * self.inv).astype(F32).astype(np.float64)
        self.mt = (t.max(ax, keepdims=True) * self.inv).astype(F32).astype(np.float64)
        self.Ds, self.Dt = xs - self.ms, xt - self.mt
        es, et = np.exp(self.Ds), np.exp(self.Dt)
        zs, zt = es.sum(ax, keepdims=True), et.sum(ax, keepdims=True)
        self.lzs, self.lzt = np.log(zs), np.log(zt)
        self.lq, self.lp = self.Ds - self.lzs, self.Dt - self.lzt
        self.q, self.p = np.exp(self.lq), np.exp(self.lp)
        self.kl = (self.p * (self.lp - self.lq)).sum(ax, keepdims=True)
        self.loss = self.tau * self.tau / self.units * float(self.kl.sum())
        self.g = self.norm * self.go * (self.q - self.p)
        self.dbs, self.dbt = (self.q * np.abs(self.Ds)).sum(ax, keepdims=True), (self.p * np.abs(self.Dt)).sum(ax, keepdims=True)
        d = (t - s) * self.inv
        self.r = np.abs((self.p * d).sum(ax, keepdims=True))
        self.ra = (self.p * np.abs(d) * (3 * np.abs(self.Dt) + 4 + self.depth)).sum(ax, keepdims=True)


def _first_order(k):
    """u k / (1 - u k): a relative error of k roundings, and of exp of an exponent off by u k"""
    return U32 * k / (1 - U32 * k)


def distill_logz_counts(ref):
    """(L_S, L_T) per unit, units of u, of |stats.y - lzs| and |stats.w - lzt|, counted from the second sweep of
    distill_pixel_fwd_kernel / distill_channel_sum_kernel and the finalize.  A term e_i = __expf(fmaf(x_i, inv_tau, -m)), which the
    compiler makes V_EXP_F32(fl(fl(x_i inv_tau - m) LOG2E)): the fma's rounding (|D_i|), the constant LOG2E's own (|D_i|), the product
    (|D_i|), V_EXP_F32 (2): relative 3 |D_i| + 2.  Weighted by e_i / Z that is 3 sum q_i |D_i| + 2 on Z.  The sum adds positive
    terms: `depth` (distill_depth).  logf: 2 |log Z|.  + 1 for the terms below the smallest normal that V_EXP_F32 may flush (the
    largest term is >= 1 - u |m|, N 2^-126 is far below one u of Z) and the second order of the lot"""
    return (3 * ref.dbs + 2 + ref.depth + 2 * np.abs(ref.lzs) + 1, 3 * ref.dbt + 2 + ref.depth + 2 * np.abs(ref.lzt) + 1)


def distill_logz_bound(ref):
    Ls, Lt = distill_logz_counts(ref)
    return _first_order(Ls), _first_order(Lt)


def distill_grad_bound(ref, bf16):
    """|d - g| <= norm go [u' (kq + 3) q + u' (kp + 3) p] + floor, per ELEMENT, u' k = u k / (1 - u k); the form u k(x) norm go
    (q + p) with k taken per softmax.  Counted from distill_bwd_kernel, q = __expf(fmaf(s, inv_tau, -m_S) - log Z_S):
      |D|          the fma's rounding, of x - m
      L_S          the stored log Z_S (distill_logz_counts)
      |log q|      the subtraction's rounding
      2 |log q|    the product with LOG2E and that constant's rounding
      2            V_EXP_F32
    kq = |D| + 3 |log q| + L_S + 2, likewise kp.  Then q - p (one rounding of |q - p| <= q + p) and the products with norm and with
    grad_out (two more, each of a value <= q + p): 3 u (q + p), written below as + 3 in kq AND in kp -- u (kq + 3) q + u (kp + 3) p
    = u kq q + u kp p + 3 u (q + p), each of the three roundings counted once.  The bound is relative to q + p, not to |q - p|: the exponent's error is absolute in nats, so each softmax value
    carries an error relative to ITSELF, which does not cancel in the difference.  Floor: each exponential and the stored element may
    be flushed below the smallest normal, 2^-126 (2 norm go + 1).  A bf16 gradient adds 2^-8 (|g| + bound)"""
    Ls, Lt = distill_logz_counts(ref)
    kq = np.abs(ref.Ds) + 3 * np.abs(ref.lq) + Ls + 2 + 3
    kp = np.abs(ref.Dt) + 3 * np.abs(ref.lp) + Lt + 2 + 3
    bound = ref.norm * ref.go * (_first_order(kq) * ref.q + _first_order(kp) * ref.p) + DISTILL_FLOOR * (2 * ref.norm * ref.go + 1)
    return bound + (2.0 ** -8 * (np.abs(ref.g) + bound) if bf16 else 0.0)


def distill_kl_bound(ref):
    """per unit, |KL_f32 - kl| of KL = a / zt + (ms - mt) + logf(zs / zt), counted from the forward kernels:
      A = sum e_i d_i    d_i = fl(fl(t - s) inv_tau) (2), e_i (3 |D_i| + 2), the fma sum (depth): ra = sum p |d| (3 |Dt| + 4 + depth);
      a / zt             zt's own 3 dbt + 2 + depth and the division (1), on r = |A / Z_T|
      ms - mt            one rounding
      logf(zs / zt)      both sums (3 dbs + 3 dbt + 4 + 2 depth), the division (1), logf (2 |log(Z_S / Z_T)|)
      the two additions  on |a / zt| + |ms - mt| and on that + |log|
    The kernel header's own count k = 16 (on M = max|x| + ln N) takes every sum as ONE rounding whatever its length; that is an
    expectation, not a bound -- a worst case pays `depth` per sum, as here"""
    lr = np.abs(ref.lzs - ref.lzt)
    dm = np.abs(ref.ms - ref.mt)
    k = (ref.ra + ref.r * (3 * ref.dbt + ref.depth + 3) + dm + 3 * ref.dbs + 3 * ref.dbt + 2 * ref.depth + 5 + 2 * lr
         + (ref.r + dm) + (ref.r + dm + lr))
    return U32 * k * 1.001


def distill_loss_bound(ref):
    """the units' bounds through the f64 partial sums (2^-45 of the terms' magnitudes covers any order) and ONE f32 rounding of
    (double)tau^2 / #units * sum"""
    mag = float((ref.r + np.abs(ref.ms - ref.mt) + np.abs(ref.lzs - ref.lzt)).sum())
    return ref.tau * ref.tau / ref.units * (float(distill_kl_bound(ref).sum()) + 2.0 ** -45 * mag) + U32 * abs(ref.loss) * 1.001


def worst_ratio(err, bound):
    """max err / bound; inf where the bound is 0 and the error is not, and where the error is NaN"""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.where(np.isnan(err), np.inf, r).max())


def distill_ratios(ref, loss, stats, d, bf16):
    """a result (loss, stats [units][4], d [B][HW][C]) against the reference: dict(max: the stored maxima hold the reference's bits,
    logz, loss, grad: the largest |out - ref| / bound)"""
    B, C, HW = ref.shape
    st = np.asarray(stats, np.float64).reshape((B, HW, 1, 4) if ref.kind == 'pixel' else (B, 1, C, 4))
    bs, bt = distill_logz_bound(ref)
    return dict(max=bool((st[..., 0] == ref.ms).all() and (st[..., 2] == ref.mt).all()),
                logz=max(worst_ratio(np.abs(st[..., 1] - ref.lzs), bs), worst_ratio(np.abs(st[..., 3] - ref.lzt), bt)),
                loss=worst_ratio(abs(float(loss) - ref.loss), distill_loss_bound(ref)),
                grad=worst_ratio(np.abs(np.asarray(d, np.float64) - ref.g), distill_grad_bound(ref, bf16)))


def distill_operands(B, C, HW, seed, hot=False):
    """(s, t) [B][HW][C]: head_logits (multiples of 2^-2 in [-8, 8], exact in bf16); hot (needs HW >= 8, C >= 8): logits of
    magnitude 200 (bf16 numbers) on a 3 x 3 block of (position, class) whose rows and columns hold one, two and three of them in
    the student -- so a pixel and a plane have m = 200 / tau with log Z = 0, ln 2 and ln 3, where m + log Z in ONE float rounds at
    the size of m -- some matched in the teacher, some opposed, and a -200 in each"""
    g = case_gen(4711, B, C, HW, seed)
    s, t = head_logits((B, HW, C), g).numpy(), head_logits((B, HW, C), g).numpy()
    if hot:
        i, c = HW // 2, C // 2
        for di, dc in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)):
            s[B - 1, i + di, c + dc] = 200.0
        for di, dc in ((0, 0), (1, 1), (2, 1), (2, 2), (0, 2)):
            t[B - 1, i + di, c + dc] = 200.0
        s[B - 1, i + 3, c], t[B - 1, i, c + 1], t[B - 1, i + 2, c] = -200.0, -200.0, -200.0
    return s, t


DISTILL_PIXEL_C = (1, 7, 8, 9, 19, 25, 256)
DISTILL_PIXEL_P = ((1, 0), (257, 0), (600, 1))            # (B HW, max_blocks)
DISTILL_CHANNEL_C = (8, 9, 19, 256)                       # 1, 2, 3 and 32 vectors per row; 19: 85 slots, one thread of the block idle


def distill_pixel_cases(C):
    """[(name, B, HW, max_blocks, tau, hot)]: 257 pixels as one image, 600 as 3 x 200 under one block; tau cycles through DISTILL_TAUS"""
    out = []
    for i, (P, cap) in enumerate(DISTILL_PIXEL_P):
        B = 3 if P % 3 == 0 else 1
        out.append(('pixel_c%d_p%d' % (C, P), B, P // B, cap, DISTILL_TAUS[(i + C) % 4], False))
    if C == 19:
        out.append(('pixel_c19_p257_hot', 1, 257, 0, 0.5, True))
    return out


def distill_channel_cases(C):
    """[(name, B, HW, max_blocks, tau, hot)]: HW in {1, ppb - 1, ppb + 1, 3 ppb + 2}, B in {1, 3}, max_blocks in {0, 1, 2, B}"""
    ppb = DISTILL_NT // cdiv(C, 8)
    out, i = [], 0
    for HW in (1, ppb - 1, ppb + 1, 3 * ppb + 2):
        for B in (1, 3):
            for cap in sorted({0, 1, 2, B}):
                out.append(('channel_c%d_hw%d_b%d_cap%d' % (C, HW, B, cap), B, HW, cap, DISTILL_TAUS[i % 4], False))
                i += 1
    if C == 19:
        out.append(('channel_c19_hw%d_b3_cap0_hot' % (3 * ppb + 2), 3, 3 * ppb + 2, 0, 0.5, True))
    if C == 256:      # S = 10 segments of 9 positions: the tenth is EMPTY (the smallest such shape; none of the shapes above has one)
        out.append(('channel_c256_hw81_b1_cap10_empty', 1, 81, 10, 4.0, False))
    return out


# --- planar focal and soft Dice (csrc/softloss.hip on the class-plane sweep of csrc/losssweep.h): logits x [B][C][HW], labels [B][HW]
SOFT_NT = 256                    # lsw::NT: lanes of a block, one group of 8 pixels per lane and trip
SOFT_FOCAL_BLOCKS = 4096         # default grid caps
SOFT_DICE_BLOCKS = 768
SOFT_DICE_CP = 24                # DICE_CP: classes per sweep of dice_fwd_kernel
SOFT_GAMMAS = (0.0, 0.5, 2.0)
#               B, C, HW
SOFT_PLANAR = [(1, 1, 8),         # one class: q == 0 at every pixel
               (2, 2, 8),
               (1, 19, 2056),     # 257 groups: the second block has one lane
               (3, 19, 1000),     # 375 groups, not a multiple of the block
               (1, 24, 64), (1, 25, 64), (1, 48, 64), (1, 49, 64),      # one, two, two and three Dice sweeps of DICE_CP classes
               (1, 256, 16)]      # label 255 is a class: ignored with has_ignore, counted without
SOFT_BEHIND = (1, 2, 64)          # added: every pixel valid with its target 6 BELOW the other class (p = 2.5e-3): the second term of
                                  # coef is 0.7 % of the first at gamma = 0.5, under the whole-tensor criterion of a bf16 gradient


def soft_grid(B, HW, max_blocks, default_cap):
    """(grid, trips of a lane) of a class-plane sweep over the B HW / 8 groups"""
    groups = B * (HW // 8)
    grid = max(1, min(cdiv(groups, SOFT_NT), max_blocks if max_blocks > 0 else default_cap))
    return grid, cdiv(groups, grid * SOFT_NT)


def soft_planar_operands(B, C, HW, behind=False):
    """(x [B][C][HW] head_logits, labels [B][HW] head_labels, {name: (class or pixel)}).  With C >= 19, planted in image 0:
    pixels 0..3 whose target (classes C-2 .. C-5, never 255) holds the maximum by 0 (a tie with the next class), by 2^-2 and by 16, and lies 16
    below it; class 1 ABSENT from the labels and class 2 present at pixel 5 only.  C == 2: the lead-by-16 and the 16-below pixel.
    behind: every pixel valid, its target at -3 and every other class at 3"""
    g = case_gen(4712, B, C, HW)
    x = head_logits((B, C, HW), g).numpy()
    lab = head_labels(B, 1, HW, C, g).reshape(B, HW).numpy().copy()
    plants = {}
    if behind:
        lab = torch.randint(0, C, (B, HW), generator=g).numpy()
        x[:] = 3.0
        np.put_along_axis(x, lab[:, None, :], -3.0, 1)
        return x, lab, plants
    if C >= 19:
        lab[lab == 1] = 3
        lab[lab == 2] = 4
        lab[0, 5] = 2
        plants.update(absent=1, single=2)
    if C >= 2:
        gaps = ((0.0, 0), (0.25, 1), (16.0, 2), (-16.0, 3)) if C >= 19 else ((16.0, 2), (-16.0, 3))
        for gap, i in gaps:
            t = (C - 2 - i) % C
            o = (t + 1) % C
            lab[0, i] = t
            if gap == 16.0:
                x[0, :, i], x[0, t, i] = -8.0, 8.0
            elif gap == -16.0:
                x[0, t, i], x[0, o, i] = -8.0, 8.0
            else:
                x[0, :, i] = np.minimum(x[0, :, i], 4.0 - max(gap, 0.25))
                x[0, t, i], x[0, o, i] = 4.0, 4.0 - gap
            plants['gap%g' % gap] = i
    return x, lab, plants


def focal_terms(p, q, lp, gamma, variant):
    """f64 terms of the focal loss as the kernels define them, per pixel: p the target's probability, q the SUM of the other
    classes', lp = log p.  w = exp(q^gamma) (variant 0, the reference's) or q^gamma (variant 1, Lin et al.); w' = dw/dp =
    -gamma q^(gamma - 1) w (variant 1: -gamma q^(gamma - 1)); the second term p w' lp is 0 at q == 0 or gamma == 0.
    Returns (w, w', coef = -(p w' lp + w), the loss term w lp)"""
    q = np.asarray(q, np.float64)
    pos = q > 0
    qs = np.where(pos, q, 1.0)
    if gamma == 0:
        qg, dqg = np.ones_like(q), np.zeros_like(q)
    else:
        qg, dqg = np.where(pos, qs ** gamma, 0.0), np.where(pos, gamma * qs ** (gamma - 1), 0.0)
    w = np.exp(qg) if variant == 0 else qg
    wp = -dqg * w if variant == 0 else -dqg
    return w, wp, -(p * wp * lp + w), w * lp


class PlanarRef:
    """f64 softmax state of planar logits x [B][C][HW] with labels [B][HW]: valid (the one validity rule), t (clamped), onehot,
    m = max_c, D = x - m, s = sum exp D, lse, lp = log softmax, p = softmax, dbar = sum_c p_c |D_c|; per pixel for the focal
    kernel, which keeps the target out of its running sum: so = sum_{c != t} exp D_c (all classes where not valid), et = exp D_t, pt, q = so / s, lpt,
    dbo = sum_{c != t} exp(D_c) |D_c| / so, lead = the target holds the maximum (et == 1.f: the log1pf branch)"""
    def __init__(self, x, labels, ignore_index=255, has_ignore=True):
        B, C, HW = x.shape
        self.x, self.labels, self.shape = x, labels, (B, C, HW)
        self.valid = (labels >= 0) & (labels < C) & ((labels != ignore_index) | (not has_ignore))
        self.t = np.clip(labels, 0, C - 1)
        self.onehot = (np.arange(C)[None, :, None] == self.t[:, None, :]) & self.valid[:, None, :]
        self.m = x.max(1)
        self.D = x - self.m[:, None]
        E = np.exp(self.D)
        self.s = E.sum(1)
        self.lse = self.m + np.log(self.s)
        self.lp = self.D - np.log(self.s)[:, None]
        self.p = np.exp(self.lp)
        self.dbar = (self.p * np.abs(self.D)).sum(1)
        self.et = (E * self.onehot).sum(1)
        self.so = (E * ~self.onehot).sum(1)
        self.Dt = (self.D * self.onehot).sum(1)
        self.dbo = (E * ~self.onehot * np.abs(self.D)).sum(1) / np.where(self.so > 0, self.so, 1.0)
        self.pt, self.q = self.et / self.s, self.so / self.s
        self.lead = self.valid & (self.Dt == 0)
        self.lg = np.where(self.lead, np.log1p(self.so), np.log(self.s))
        self.lpt = np.where(self.valid, self.Dt - self.lg, 0.0)
        self.nvalid = int(self.valid.sum())
        # premises of the counts: the logits are spaced wider than 2^-24 (et == 1.f iff the target holds the maximum) and no q
        # is so small that f32 loses it (q == 0 only with a single class)
        assert (self.q[self.valid] > 2.0 ** -100).all() or C == 1


def soft_lse_count(ref):
    """roundings (units of u, nats) of lsw::lse8's stored l = m + __logf(s), the online log-sum-exp.  Per class one rescale and one
    new term, s = s __expf(m - mn) + __expf(v - mn): the rescale's V_EXP_F32 (2), the product (1), the addition (1) -- 4 for every
    later class a term lives through, <= 4 (C - 1) -- and V_EXP_F32 on the term itself (2).  The exponents: every subtraction
    (v - mn, m - mn), the product with LOG2E and that constant's own rounding are relative to a step of the running maximum, and the
    steps a term sees add up to |D_c| = m - x_c: 3 |D_c|, weighted by p_c on the sum: 3 dbar.  __logf(s) = fl(V_LOG_F32(s) LN2):
    V_LOG_F32 (2), the constant and the product: 4 |log s|.  m + log s and the store: |lse|.  + 1 for the second order"""
    C = ref.shape[1]
    return 3 * ref.dbar + 4 * C + 4 * np.abs(np.log(ref.s)) + np.abs(ref.lse) + 1


def soft_p_count(ref, lse_count):
    """relative error (units of u) of a softmax value recomputed as __expf(x - l) from the stored l (grad8, the Dice sweeps): l's own
    error, the subtraction's rounding (|log p|), the product with LOG2E and that constant (2 |log p|), V_EXP_F32 (2).  The
    exponent's error is ABSOLUTE in nats -- u (|x| + 2 |lse|) at the least -- so p_c carries an error relative to ITSELF and the
    gradient's bound is relative to p_c + [c == t], not to |p_c - [c == t]|: near p_t = 1 the difference is far smaller than
    either term's error"""
    return lse_count[:, None] + 3 * np.abs(ref.lp) + 2


def focal_planar_counts(ref, gamma, variant):
    """per valid pixel, from focal_fwd_kernel (units of u): dict of
      lse     absolute, of the stored l = m + lg
      coef    absolute, of pixel_coef = -(p w' lp + w)
      term    absolute, of the loss term w lp
    and the f64 terms (w, wp, coef, wlp).  The chain, rounding by rounding:
      so      the running sum WITHOUT the target: Kso = 3 dbo + 4 C (soft_lse_count's sum)
      et      __expf(xt - m): Ket = 3 |Dt| + 2
      s       so + et: Ks = q Kso + p Ket + 1
      lg      the target holds the maximum (et == 1.f): log1pf(so), q Kso + 2 lg -- RELATIVE to lg ~ q when q is small, which
              __logf(1 + so) is not; otherwise __logf(s): Ks + 4 |lg|
      lp      (xt - m) - lg: at a leading target 0 - lg, exact; otherwise |Dt| + |lp| for the two subtractions
      p, q    et inv, so inv with inv = 1 / s (correctly rounded): Kp = Ket + Ks + 2, Kq = Kso + Ks + 2
      q^gamma exp2f(gamma __log2f(q)): V_LOG_F32 (2 |log2 q|) and q's own error through the logarithm (Kq / ln 2), both times gamma;
              the product (|gamma log2 q|); exp2f (2): in nats Kqg = gamma Kq + 3 |gamma ln q| + 2 -- the first term is the
              conditioning of q^gamma in the relative error of q
      gamma q^(gamma-1)   gamma qg / q: Kdqg = Kqg + Kq + 2 (>= the conditioning |gamma - 1| Kq)
      w       variant 0: __expf(qg), qg (Kqg + 2) + 2;  variant 1: Kqg
      w'      variant 0: dqg w, Kdqg + Kw + 1;  variant 1: Kdqg
      coef    T1 = p w' lp >= 0 and w >= 0 add without cancellation: T1 (Kp + Kwp + 2) + p |w'| E(lp) + w Kw + (T1 + w)
      w lp    |w lp| (Kw + 1) + w E(lp)
    V_EXP_F32 / V_LOG_F32 at 1 ulp: the vendor's figure, not measured here; exp2f, log1pf and the division at 1 ulp or better"""
    C = ref.shape[1]
    v = ref.valid
    Kso = np.where(ref.so > 0, 3 * ref.dbo + 4 * C, 0.0)
    Ket = 3 * np.abs(ref.Dt) + 2
    Ks = np.where(v, ref.q * Kso + ref.pt * Ket + 1, Kso)
    lg = np.abs(ref.lg)
    Elg = np.where(ref.lead, ref.q * Kso + 2 * lg, Ks + 4 * lg)
    Elp = np.where(ref.lead, Elg, np.abs(ref.Dt) + Elg + np.abs(ref.lpt))
    Kp, Kq = Ket + Ks + 2, Kso + Ks + 2
    w, wp, coef, wlp = focal_terms(ref.pt, ref.q, ref.lpt, gamma, variant)
    live = (ref.q > 0) & (gamma != 0)
    lnq = np.abs(np.log(np.where(ref.q > 0, ref.q, 1.0)))
    Kqg = np.where(live, gamma * Kq + 3 * gamma * lnq + 2, 0.0)
    Kdqg = np.where(live, Kqg + Kq + 2, 0.0)
    qg = np.ones_like(ref.q) if gamma == 0 else np.where(ref.q > 0, np.where(ref.q > 0, ref.q, 1.0) ** gamma, 0.0)
    Kw = qg * (Kqg + 2) + 2 if variant == 0 else Kqg
    Kwp = np.where(live, Kdqg + Kw + 1, 0.0) if variant == 0 else Kdqg
    T1 = np.abs(ref.pt * wp * ref.lpt)
    Ecoef = T1 * (Kp + Kwp + 2) + ref.pt * np.abs(wp) * Elp + w * Kw + (T1 + w)
    Eterm = np.abs(wlp) * (Kw + 1) + w * Elp
    z = lambda a: np.where(v, a, 0.0)
    return dict(lse=Elg + np.abs(ref.m + ref.lg) + 1, coef=z(Ecoef), term=z(Eterm), w=z(w), wp=z(wp), A=z(coef), wlp=z(wlp))


def focal_coef_err(ref, gamma, variant):
    """(relative error of one coef, of one w lp), units of u, per valid pixel (0 elsewhere) of the PLANAR kernel: focal_planar_counts, on
    a PlanarRef.  The same two figures of the fused head's softhead_pass_kernel<., ., SH_FOCAL> are head_focal_coef_err (on a
    HeadFocalRef, counted in its docstring); those of focal_coef_kernel are inside focal_coef_ref"""
    k = focal_planar_counts(ref, gamma, variant)
    rel = lambda e, v: np.where(v != 0, e / np.where(v != 0, np.abs(v), 1.0), 0.0)
    return rel(k['coef'], k['A']), rel(k['term'], k['wlp'])


class FocalPlanarRef:
    """reference and bounds of tss_focal_fwd / tss_focal_bwd: lse, coef, loss, scale = (float)((double)alpha / n) exactly, g"""
    def __init__(self, ref, gamma, variant, alpha, grad_out):
        k = focal_planar_counts(ref, gamma, variant)
        n = ref.nvalid
        a32, go = float(F32(alpha)), float(F32(grad_out))
        self.lse = ref.m + ref.lg
        self.lse_bound = U32 * k['lse'] * 1.001
        self.coef, self.coef_bound = k['A'], U32 * k['coef'] * 1.001
        self.scale = float(F32(a32 / n)) if n else 0.0
        self.nvalid = n
        self.loss = -a32 * float(k['wlp'].sum()) / n if n else 0.0
        self.loss_bound = (a32 / n * (U32 * float(k['term'].sum()) * 1.001 + 2.0 ** -45 * float(np.abs(k['wlp']).sum()))
                           + U32 * abs(self.loss) * 1.001) if n else 0.0
        gs = self.scale * go
        h = ref.onehot.astype(np.float64)
        self.g = (h - ref.p) * (self.coef * gs)[:, None]
        # gs = fl(scale go) and a gs (2); e = __expf(x - l) (soft_p_count on the focal lse); h - e (1, of |h - e| <= p + h); times w (1)
        kp = _first_order(soft_p_count(ref, k['lse']))
        A = np.abs(self.coef)[:, None]
        self.g_bound = gs * (A * ref.p * kp + (ref.p + h) * (U32 * 1.001 * (4 * A + k['coef'][:, None])))

    def grad_bound(self, bf16):
        return self.g_bound + (2.0 ** -8 * (np.abs(self.g) + self.g_bound) if bf16 else 0.0)


def dice_coef_ref(P, I, N, dP, dI, smooth, any_valid):
    """the f64 finalize of both Dice routes on class sums P, I, N with errors dP, dI (N is exact): (a, b, da, db, loss, loss bound);
    den = P + N + smooth, num = 2 I + smooth, a = -2 / (C den), b = num / (C den^2), loss = mean 1 - num / den.  da = |a| dP / den,
    db = 2 dI / (C den^2) + 2 b dP / den (both over (1 - dP / den)^2 for the second order) and the cast to f32 (1); the loss:
    sum (2 dI + (num / den) dP) / den / C and its cast.  No valid pixel: everything 0"""
    C = len(P)
    if not any_valid:
        z = np.zeros(C)
        return z, z, z, z, 0.0, 0.0
    sm = float(F32(smooth))
    den, num = P + N + sm, 2 * I + sm
    assert (den > 0).all()
    tight = 1.0 / (1.0 - dP / den) ** 2
    a, b = -2.0 / (C * den), num / (C * den * den)
    da = (np.abs(a) * dP / den * tight + U32 * np.abs(a)) * 1.001
    db = ((2 * dI / (C * den * den) + 2 * b * dP / den) * tight + U32 * b) * 1.001
    loss = float((1 - num / den).mean())
    return a, b, da, db, loss, float(((2 * dI + num / den * dP) / den * tight).sum()) / C + U32 * abs(loss) * 1.001


class DicePlanarRef:
    """reference and bounds of tss_dice_fwd / tss_dice_bwd at a grid (max_blocks): P_c = sum_V p_c, I_c, N_c, den_c = P_c + N_c +
    smooth, loss, coef a_c, b_c, the gradient p_k (G_k - sum_c p_c G_c) grad_out, and
      dP, dI    of the statistics: every p = __expf(x - l) (soft_p_count), the lane's f32 chain -- the 8 pixels of a group and one
                addition per trip, 8 + trips -- then f64.  Past DICE_CP classes the later sweeps read l back: the same float, nothing more
      da, db    through the f64 finalize (a = -2 / (C den): |a| dP / den; b = num / (C den^2): 2 dI / (C den^2) + 2 |b| dP / den)
                and the cast to f32 (1)
      loss      sum_c (2 dI_c + (num / den) dP_c) / den_c / C and the cast
      gradient  dot = sum_c p_c G_c in f32: per term p_c's error, the addition b_c + a_c at the target (1), the product (1) and the C
                accumulations, plus the coefficients' own error; then e ((G_k) - dot) gv: the subtraction and two products (3)"""
    def __init__(self, ref, smooth, grad_out, max_blocks=0):
        B, C, HW = ref.shape
        self.grid, trips = soft_grid(B, HW, max_blocks, SOFT_DICE_BLOCKS)
        v = ref.valid[:, None, :]
        h = ref.onehot.astype(np.float64)
        pv = ref.p * v
        kl = soft_lse_count(ref)
        kp = soft_p_count(ref, kl)
        cls = lambda a: a.sum((0, 2))
        self.lse, self.lse_bound = ref.lse, U32 * kl * 1.001
        self.P, self.I, self.N = cls(pv), cls(pv * h), cls(h)
        chain = 8 + trips
        dP = U32 * 1.001 * (cls(pv * kp) + chain * self.P) + 2.0 ** -45 * self.P
        dI = U32 * 1.001 * (cls(pv * h * kp) + chain * self.I) + 2.0 ** -45 * self.I
        go = float(F32(grad_out))
        self.a, self.b, self.da, self.db, self.loss, self.loss_bound = dice_coef_ref(self.P, self.I, self.N, dP, dI, smooth, ref.nvalid > 0)
        a, b, da, db = (q[None, :, None] for q in (self.a, self.b, self.da, self.db))
        G = b + h * a
        dG = db + h * (da + U32 * np.abs(G))
        dot = (ref.p * G).sum(1, keepdims=True)
        Edot = (ref.p * (np.abs(G) * (_first_order(kp) + U32 * (1 + C) * 1.001) + dG)).sum(1, keepdims=True)
        self.g = ref.p * (G - dot) * go * v
        self.g_bound = go * v * ref.p * (_first_order(kp) * np.abs(G - dot) + dG + Edot + 3 * U32 * 1.001 * np.abs(G - dot))

    def grad_bound(self, bf16):
        return self.g_bound + (2.0 ** -8 * (np.abs(self.g) + self.g_bound) if bf16 else 0.0)


def _err(out, ref):
    return np.abs(np.asarray(out, np.float64) - ref)


# --- tss_focal_coef_from_ce (focal_coef_kernel of csrc/softhead.hip): the wide route's planar step on a stored cross-entropy
SOFT_CE_VALUES = (0.0, 1e-40, 2.0 ** -24, 1.0, 40.0, 200.0)       # p = 1 and q = 0; a denormal; q = 2^-24; ordinary; p ~ 4e-18; p below f32
SOFT_CE_N = (1, 3, 4, 5, 1027)                                    # tail groups of 1 and 3 pixels, one whole group, 257 groups in two blocks


def soft_ce_operands(n, C=19):
    """(ce f32 [n], labels [n]): SOFT_CE_VALUES in turn, then multiples of 2^-4 below 16; about 10 % of the labels 255, -1 or 300"""
    g = case_gen(4713, n)
    ce = (torch.randint(0, 256, (n,), generator=g).double() / 16).numpy()
    k = min(n, len(SOFT_CE_VALUES))
    ce[:k] = SOFT_CE_VALUES[:k]
    if n > 2 * len(SOFT_CE_VALUES):
        ce[-len(SOFT_CE_VALUES):] = SOFT_CE_VALUES                # again at the far end: the tail group and the second block
    lab = head_labels(1, 1, n, C, g).reshape(n).numpy().copy()
    lab[:k] = np.arange(k) % C
    return ce.astype(F32), lab


def focal_coef_ref(ce, labels, C, gamma, variant, alpha, ignore_index=255, has_ignore=True):
    """f64 reference of tss_focal_coef_from_ce on the STORED f32 ce: p = exp(-ce), q = -expm1(-ce), lp = -ce, coef = w - w'(q) p lp
    of X.focal_terms (0 where the pixel does not count), loss = -alpha sum w lp / n, scale = (float)((double)alpha / n), and bounds
    counted from focal_coef_kernel and softhead.hip's focal_terms (units of u):
      p       __expf(lp): the product with LOG2E and that constant (2 |lp|), V_EXP_F32 (2); below the smallest normal it may be flushed
      q       -expm1f(lp), the library's, taken at 1 ulp (2)
      q^gamma, gamma q^(gamma-1), w, w'      as focal_planar_counts: Kqg = gamma Kq + 3 |gamma ln q| + 2, Kdqg = Kqg + Kq + 2,
              Kw = qg (Kqg + 2) + 2 (variant 0) or Kqg, Kdw = Kdqg + Kw + 1 or Kdqg
      coef    wq - (dw p) lp, both terms >= 0: wq Kw + T1 (Kdw + Kp + 2) + (wq + T1), T1 = |dw p lp|
      w lp    |w lp| (Kw + 1)
    A q below the smallest normal (ce = 1e-40) may be flushed by V_LOG_F32, and then q^gamma is taken as 0: (1 + gamma) q^gamma e
    covers both terms of coef there.  The hardware's and the library's 1 ulp are the vendor's figures, not measured here"""
    ce = np.asarray(ce, F32).astype(np.float64)
    valid = (labels >= 0) & (labels < C) & ((labels != ignore_index) | (not has_ignore))
    lp = -ce
    p, q = np.exp(lp), -np.expm1(lp)
    w, wp, negcoef, wlp = focal_terms(p, q, lp, gamma, variant)
    live = (q > 0) & (gamma != 0)
    qs = np.where(q > 0, q, 1.0)
    Kp, Kq = 2 * ce + 2, 2.0
    Kqg = np.where(live, gamma * Kq + 3 * gamma * np.abs(np.log(qs)) + 2, 0.0)
    Kdqg = np.where(live, Kqg + Kq + 2, 0.0)
    qg = np.ones_like(q) if gamma == 0 else np.where(q > 0, qs ** gamma, 0.0)
    Kw = qg * (Kqg + 2) + 2 if variant == 0 else Kqg
    Kdw = np.where(live, Kdqg + Kw + 1, 0.0) if variant == 0 else Kdqg
    T1 = np.abs(wp * p * lp)
    tiny = DISTILL_FLOOR
    flushed = np.where(live & (q < tiny), (1 + gamma) * qg * math.e, 0.0)
    Ecoef = U32 * 1.001 * (w * Kw + T1 * (Kdw + Kp + 2) + (w + T1)) + np.abs(wp * lp) * tiny + flushed + tiny
    Eterm = U32 * 1.001 * np.abs(wlp) * (Kw + 1) + flushed * ce + tiny
    n = int(valid.sum())
    a32 = float(F32(alpha))
    z = lambda a: np.where(valid, a, 0.0)
    loss = -a32 * float(z(wlp).sum()) / n if n else 0.0
    return dict(valid=valid, coef=z(-negcoef), coef_bound=z(Ecoef), loss=loss, scale=float(F32(a32 / n)) if n else 0.0, nvalid=n,
                loss_bound=(a32 / n * float(z(Eterm).sum()) * (1 + 2.0 ** -40) + U32 * abs(loss) * 1.001) if n else 0.0)


def focal_planar_ratios(fr, lse, coef, loss, scale, d, bf16):
    """a result of tss_focal_fwd / _bwd against a FocalPlanarRef: the largest |out - ref| / bound of lse, pixel_coef, loss and
    dlogits; scale: the stored bits are (float)((double)alpha / n)"""
    return dict(lse=worst_ratio(_err(lse, fr.lse), fr.lse_bound), coef=worst_ratio(_err(coef, fr.coef), fr.coef_bound),
                loss=worst_ratio(abs(float(loss) - fr.loss), fr.loss_bound), grad=worst_ratio(_err(d, fr.g), fr.grad_bound(bf16)),
                scale=float(scale) == fr.scale)


def dice_planar_ratios(dr, lse, coef, loss, d, bf16):
    """a result of tss_dice_fwd / _bwd (coef: a_c then b_c) against a DicePlanarRef"""
    C = len(dr.a)
    return dict(lse=worst_ratio(_err(lse, dr.lse), dr.lse_bound), a=worst_ratio(_err(coef[:C], dr.a), dr.da),
                b=worst_ratio(_err(coef[C:2 * C], dr.b), dr.db), loss=worst_ratio(abs(float(loss) - dr.loss), dr.loss_bound),
                grad=worst_ratio(_err(d, dr.g), dr.grad_bound(bf16)))


# --- focal and soft Dice on the fused head (csrc/softhead.hip: softhead_pass_kernel<T, CP, SH_FOCAL | SH_DICE_STATS | SH_DICE_GRAD>, the
# finalize kernels, then the gather of tss_upsample_ce_bwd).  The references stand on HeadRef (z, valid, softmax, My, Mx); the chains of
# the band walk and the gather are head_grad_counts', the coordinate slack of a pair that is not exact is head_slack's.
HEAD_SOFT_EXTRA = HeadCase('edge_few', 1, 19, 3, 33, 9, 255)     # added, CPU only: ONE lane past the image edge (W = 255), so that counting
                                                                 # its N_c moves the coefficients by less than the old criterion sees


def head_soft_p_count(zmax, CP):
    """relative error (units of u) of one softmax value p_c = e_c inv of softhead_pass_kernel, head_grad_counts' register r_p without a
    pixel weight: 20 zmax (the interpolation and z - m as perturbations d of the logits, which move p_c by <= 2 p_c d), V_EXP_F32 on
    the value and on the terms of the sum (4), the CP - 1 additions (the pad classes add exact zeros), V_RCP_F32 (2), the product (1)"""
    return 20.0 * zmax + CP + 6


class HeadDiceRef:
    """dice_ref: f64 soft Dice on the fused head from a HeadRef (its valid mask decides has_ignore), with the bounds.
      P, I, N       sum_V p_c, sum_V p_c [t == c], sum_V [t == c];  a, b, loss as softhead_dice_finalize_kernel forms them
      dz            p_k (b_k - S) + [k == t] a_t p_t, S = sum_c b_c p_c + a_t p_t, on V;  g = grad_out My dz Mx^T (inv_count = 1)
      T, A          the absolute twin p_k (|b_k| + sum_c |b_c| p_c + |a_t| p_t) + [k == t] |a_t| p_t and its gather
    Coefficients: every p (head_soft_p_count, + 2 slack_z relative on a pair that is not exact), the lane's f32 sum over the rows
    of its band (band_rows additions; the one-hot sums in LDS likewise; N counts to at most band_rows, exact), then f64, the
    finalize's divisions and the cast: dice_coef_ref.
    Gradient: |dlow - g| <= u (n_g + r_dz) A + grad_out My Tc Mx^T + slack, n_g head_grad_counts' chain of the band walk and the
    gather; r_dz = 2 r_p + CP + 6 -- p_k and the p_c inside S (2 r_p), S's CP products and additions and the one-hot term's product
    and addition (CP + 3), b_k - S, the product with p_k (2), one spare; Tc the twin with (da, db) in place of (|a|, |b|): the
    coefficients' own error carried through.  slack: head_slack on T (a softmax value moves by 2 p slack_z) + 2 slack_z A once more
    for S, which moves with every p_c"""
    def __init__(self, ref, smooth, grad_out, n):
        C, CP = ref.C, head_cp(ref.C)
        self.low, self.size, self.zmax, self.My, self.Mx = ref.low, ref.size, ref.zmax, ref.My, ref.Mx
        p = torch.softmax(ref.z, 1)
        v = ref.valid.double()[:, None]
        onehot = torch.zeros_like(ref.z).scatter_(1, ref.t[:, None], 1.0) * v
        sz = head_slack_z(ref)
        r_p = head_soft_p_count(ref.zmax, CP)
        cls = lambda q: q.sum((0, 2, 3)).numpy()
        self.P, self.I, self.N = cls(p * v), cls(p * onehot), cls(onehot)
        rel = U32 * 1.001 * (r_p + n['band_rows']) + 2 * sz + 2.0 ** -45
        self.a, self.b, self.da, self.db, self.loss, self.loss_bound = dice_coef_ref(self.P, self.I, self.N, rel * self.P, rel * self.I, smooth,
                                                                                     bool(ref.valid.any()))
        self.go = self.gs = float(F32(grad_out))
        self.den, self.ssum = 1.0, 0.0          # head_slack's loss part is not used
        col = lambda q: torch.from_numpy(np.ascontiguousarray(q))[None, :, None, None]

        def terms(a, b):
            pt = (p * onehot).sum(1, keepdim=True)
            at = (col(a) * onehot).sum(1, keepdim=True)
            return (col(b) * p).sum(1, keepdim=True) + at * pt, at * pt
        S, hot = terms(self.a, self.b)
        Sabs, hotabs = terms(np.abs(self.a), np.abs(self.b))
        Sd, hotd = terms(self.da, self.db)
        dz = (p * (col(self.b) - S) + onehot * hot) * v
        self.T = (p * (col(np.abs(self.b)) + Sabs) + onehot * hotabs) * v
        Tc = (p * (col(self.db) + Sd) + onehot * hotd) * v
        gather = lambda q: self.go * torch.einsum('oh,bcop,pw->bchw', ref.My, q, ref.Mx)
        self.g, self.A = gather(dz), gather(self.T)
        k = U32 * (head_grad_counts(n, ref.zmax, C, False)[0] + 2 * r_p + CP + 6)
        slack = head_slack(self)[2] + 2 * sz * self.A if sz else 0.0
        self.g_bound = k / (1 - k) * self.A + 1.001 * gather(Tc) + slack

    def grad_bound(self, bf16):
        return self.g_bound + (2.0 ** -8 * (self.g.abs() + self.g_bound) if bf16 else 0.0)


def dice_ref(ref, smooth, grad_out=1.0, n=None):
    """HeadDiceRef of a HeadRef with the chain lengths of its shape; n: the case's head_counts, restated from the shape when not given"""
    (h, w), (H, W) = ref.low, ref.size
    return HeadDiceRef(ref, smooth, grad_out, n or head_counts(ref.x.shape[0], ref.C, h, w, H, W))


def head_soft_inputs(case, rare=False, focal=False):
    """head_inputs with the labels the soft losses are listed for -- class 1 ABSENT (its pixels go to class 3), class 2 at exactly ONE
    pixel (the others go to class 4; C >= 5).  rare (C > 20): the classes from 20 on lie at -8
    everywhere and never occur as a label, and classes 0 and 7 lie at +8 everywhere: p_c < 1e-7 on those planes, so
    a wrong b_c there (coef[c] read for coef[24 + c]) moves nothing the largest gradient element could show"""
    x, labels, plants = head_inputs(case)
    labels = labels.clone()
    if focal:                     # the focal operands: head_focal_plants instead of the Dice label plants
        return x, labels, head_focal_plants(case, x, labels)
    if case.C >= 5:
        labels[labels == 1] = 3
        labels[labels == 2] = 4
        labels[0, case.H // 2, case.W // 2] = 2
    if rare:
        assert case.C > 20
        B, C, h, w = x.shape
        x[:, 20:] = -8.0
        x[:, :20] = x[:, :20].clamp(max=4.0)
        x[:, 0], x[:, 7] = 8.0, 8.0
        labels[(labels >= 20) & (labels < C)] = 5
    return x, labels, plants


def head_focal_plants(case, x, labels):
    """in place, on an exact pair with at least four low-resolution cells: at the first four cells of image 0 (row-major) the logits of
    a pixel whose target holds the maximum by 0 (a tie with the next class), by 2^-2 and by 16, and lies 16 below it, and that target
    at the output pixel that sits ON the cell (where the interpolation returns the cell itself): the et == 1.f, s == 1.f-or-nearly
    and q -> 0 branches of softhead_pass_kernel<SH_FOCAL>.  Returns [(gap, output y, output x)]"""
    B, C, h, w = x.shape
    H, W = labels.shape[-2:]
    if not case.exact or h * w < 4 or C < 2:
        return []
    out = []
    for i, gap in enumerate((0.0, 0.25, 16.0, -16.0)):
        r, c = divmod(i, w)
        y, xo = (r * (H - 1) // (h - 1) if h > 1 else 0), (c * (W - 1) // (w - 1) if w > 1 else 0)
        t = (C - 2 - i) % C
        o = (t + 1) % C
        if gap == 16.0:
            x[0, :, r, c], x[0, t, r, c] = -8.0, 8.0
        elif gap == -16.0:
            x[0, t, r, c], x[0, o, r, c] = -8.0, 8.0
        else:
            x[0, :, r, c] = x[0, :, r, c].clamp(max=4.0 - max(gap, 0.25))
            x[0, t, r, c], x[0, o, r, c] = 4.0, 4.0 - gap
        labels[0, y, xo] = t
        out.append((gap, y, xo))
    return out


class HeadFocalRef:
    """f64 focal loss on the fused head from a HeadRef, with the bounds of softhead_pass_kernel<., ., SH_FOCAL>, its finalize and the
    gather.  Per valid pixel (nats): D = z - max, so = sum_{c != t} exp D_c, et = exp D_t, s = so + et, p = et / s, q = so / s, lp,
    (w, coef = w - w' p lp) of focal_terms; loss = -alpha sum w lp / n, scale = (float)((double)alpha / n), g = scale grad_out
    My (coef (p_k - [k == t])) Mx^T -- HeadRef.weights with pixw = coef.  Counts, units of u; d = 10 zmax + slack_z / u is what the
    interpolation, the product with LOG2E, z - m (head_lse_err) and, on a pair that is not exact, the f32 coordinates move a logit by:
      so, et   e_c = V_EXP_F32(z_c - m): 2 d (z_c and m both move) + 2; the CP - 1 additions: Kso = 2 d + 2 + CP, Ket = 2 d + 2
      s        so + et: Ks = q Kso + p Ket + 1;  inv = V_RCP_F32(s) (2): Kp = Ket + Ks + 3, Kq = Kso + Ks + 3
      lg       the target holds the maximum (et == 1.f; exact pairs only -- elsewhere the f32 taps decide the branch and the absolute
               form, which is never the smaller, is taken): s == 1.f: so itself (so^2 / 2 < u so); else __logf(u) so V_RCP_F32(u - 1)
               with u = fl(1 + so): log1p without the rounding of 1 + so; __logf (4), the reciprocal (2), two products (2), the
               formula's own O(u) (1), so's Kso: (Kso + 10) lg, RELATIVE to lg ~ q.  Otherwise __logf(s): Ks + 4 |lg|
      lp       (zt - m) LN2F - lg: at a leading target -lg; otherwise 2 d for the difference, 3 |Dt| (the subtraction, LN2F and the
               product), |lp| for the last subtraction
      q^gamma, gamma q^(gamma-1), w, w', coef, w lp     as focal_coef_ref: Kqg = gamma Kq + 3 |gamma ln q| + 2 (the conditioning of
               q^gamma in q's relative error, the |gamma log2 q| of the exp2f(gamma __log2f(q)) pair), Kdqg = Kqg + Kq + 2, Kw, Kdw;
               E(coef) = w Kw + T1 (Kdw + Kp + 2) + w' p E(lp) + (w + T1);  E(w lp) = |w lp| (Kw + 1) + w E(lp)
    Loss: the lane's f32 sum over the rows of its band (band_rows), then f64, one f32 cast.
    Gradient: head_grad_bound's form: u (n_g + r_p) A with r_p = head_soft_p_count + 1 (the product coef inv), plus the coefficient's
    own error through the same gather, scale grad_out My (E(coef) (p_k + [k == t])) Mx^T, plus head_slack.
    V_EXP_F32 / V_LOG_F32 / V_RCP_F32 at 1 ulp: the vendor's figure (head_lse_err), not measured here"""
    def __init__(self, ref, gamma, variant, alpha, grad_out, n):
        import copy
        C, CP = ref.C, head_cp(ref.C)
        sz = head_slack_z(ref)
        d = 10.0 * ref.zmax + sz / U32
        z = ref.z.numpy()
        valid = ref.valid.numpy()
        hot = (np.arange(C)[None, :, None, None] == ref.t.numpy()[:, None]) & valid[:, None]
        D = z - z.max(1, keepdims=True)
        E = np.exp(D)
        so, et, Dt = (E * ~hot).sum(1), (E * hot).sum(1), (D * hot).sum(1)
        s = so + et
        p, q = et / s, so / s
        lead = valid & (Dt == 0) & (sz == 0)
        lg = np.where(lead, np.log1p(so), np.log(s))
        lp = np.where(valid, Dt - lg, 0.0)
        assert (q[valid] > 2.0 ** -100).all()
        Kso, Ket = 2 * d + 2 + CP, np.where(lead, 0.0, 2 * d + 2)
        Ks = q * Kso + p * Ket + 1
        Kp, Kq = Ket + Ks + 3, Kso + Ks + 3
        Elg = np.where(lead, (Kso + 10) * lg, Ks + 4 * np.abs(lg))
        Elp = np.where(lead, Elg, 2 * d + 3 * np.abs(Dt) + Elg + np.abs(lp))
        w, wp, negcoef, wlp = focal_terms(p, q, lp, gamma, variant)
        live = gamma != 0
        Kqg = (gamma * Kq + 3 * gamma * np.abs(np.log(q)) + 2) if live else np.zeros_like(q)
        Kdqg = Kqg + Kq + 2 if live else np.zeros_like(q)
        qg = q ** gamma if live else np.ones_like(q)
        Kw = qg * (Kqg + 2) + 2 if variant == 0 else Kqg
        Kdw = (Kdqg + Kw + 1 if variant == 0 else Kdqg) if live else np.zeros_like(q)
        T1 = np.abs(wp * p * lp)
        vz = lambda a: np.where(valid, a, 0.0)
        self.coef = vz(-negcoef)
        self.coef_err = vz(U32 * 1.002 * (w * Kw + T1 * (Kdw + Kp + 2) + np.abs(wp) * p * Elp + (w + T1)))
        Eterm = vz(U32 * 1.002 * (np.abs(wlp) * (Kw + 1 + n['band_rows']) + w * Elp))
        self.wlp, self.term_err = vz(wlp), vz(U32 * 1.002 * (np.abs(wlp) * (Kw + 1) + w * Elp))
        self.nvalid = nv = int(valid.sum())
        a32, go = float(F32(alpha)), float(F32(grad_out))
        self.scale = float(F32(a32 / nv)) if nv else 0.0
        self.loss = -a32 * float(vz(wlp).sum()) / nv if nv else 0.0
        self.loss_bound = (a32 / nv * float(Eterm.sum()) * (1 + 2.0 ** -40) + U32 * abs(self.loss) * 1.001) if nv else 0.0
        r = copy.copy(ref).weights(pixw=torch.from_numpy(self.coef), grad_out=go * self.scale)
        self.g, self.A = r.g, r.A
        k = U32 * (head_grad_counts(n, ref.zmax, C, False)[0] + head_soft_p_count(ref.zmax, CP) + 1)
        ce = torch.from_numpy(self.coef_err)[:, None] * (torch.softmax(ref.z, 1) + torch.from_numpy(hot.astype(np.float64)))
        carried = go * self.scale * torch.einsum('oh,bcop,pw->bchw', ref.My, ce, ref.Mx)
        self.g_bound = k / (1 - k) * self.A + carried + (head_slack(r)[2] if sz else 0.0)

    def grad_bound(self, bf16):
        return self.g_bound + (2.0 ** -8 * (self.g.abs() + self.g_bound) if bf16 else 0.0)


def head_focal_coef_err(f):
    """(relative error of one coef, of one w lp), units of u, per valid pixel (0 elsewhere) of the fused head's focal pass, from a
    HeadFocalRef: counted from softhead_pass_kernel<., ., SH_FOCAL> and softhead.hip's focal_terms in that class's docstring (the lane's
    band_rows additions of the loss sum are not part of one term)"""
    rel = lambda e, v: np.where(v != 0, e / np.where(v != 0, np.abs(v), 1.0), 0.0) / U32
    return rel(f.coef_err, f.coef), rel(f.term_err, f.wlp)


# ---------------------------------------------------------------------------------------------------------- Lovasz-Softmax (csrc/lovasz.hip)
# Restated in numpy: the workspace planner, the symmetric key, the two-pass f64 softmax behind it, the stable order, the closed-form
# integer weights, the tile sums, the final reduction tree and the backward formula.  After the key everything is integers or IEEE f64
# in the kernel's operation order, so tests/test_gpu_lovasz_exact.py compares it bit for bit GIVEN the kernel's own keys; the key itself
# is held to an interval (LovaszRef).  tests/test_exact_bounds.py pins this restatement to tests/lovasz_ref.py.
LV_NT, LV_ITEMS = 256, 16                      # lsw::NT, ITEMS
LV_TILE = LV_NT * LV_ITEMS                     # TILE: pairs of a sort tile
LV_HALF_BITS = 0x3F000000                      # bits(0.5f)
LV_KEY_MAX = 2 * LV_HALF_BITS                  # the largest key of a kept pixel: e == 0
LV_DROPPED = 0xFFFFFFFF
LV_SORT_BYTES_CAP = 2 << 30
LV_IGNORE = 255
LV_GRAD_OUT = 0.7
LV_PARTIAL_REL = 2.0 ** -45                    # a tile's sum: any order of 4096 f64 terms stays within 4096 * 2^-53 = 2^-41 of sum |terms|; the
#   kernel's tree is 16 fused multiply-adds per lane, 6 wave_sum levels and 4 waves added in turn: depth 26, one product rounding, so
#   27 * 2^-53 sum |terms|, and the reference's own pairwise sum stays below 13 * 2^-53: 40 * 2^-53 < 2^-47 < 2^-45


def up256(x):
    return cdiv(x, 256) * 256


def lovasz_plan(N, C, chunk_classes=0):
    """make_plan of csrc/lovasz.hip: byte offsets of G, partial, W, key0/1, pay0/1, hist, dtot and tcnt, each rounded up to 256"""
    ntiles = cdiv(N, LV_TILE)
    cc = chunk_classes if chunk_classes > 0 else LV_SORT_BYTES_CAP // (16 * N)
    Cc = max(1, min(C, cc))
    p, o = dict(N=N, C=C, Cc=Cc, ntiles=ntiles), 0
    p['G'], o = o, up256(o + 4 * C)
    p['partial'], o = o, up256(o + 8 * C * ntiles)
    p['W'], o = o, up256(o + 4 * C * N)
    plane = up256(4 * Cc * N)
    for k in ('key0', 'key1', 'pay0', 'pay1'):
        p[k], o = o, o + plane
    p['hist'], o = o, up256(o + 4 * Cc * 256 * ntiles)
    p['dtot'], o = o, up256(o + 4 * Cc * 256)
    p['tcnt'], o = o, up256(o + 4 * Cc * ntiles)
    p['total'] = o
    p['last_c0'] = (C - 1) // Cc * Cc            # first class of the last chunk: its sorted pairs are what buffer 0 holds afterwards
    return p


def _f32_bits(v):
    return np.ascontiguousarray(np.asarray(v, np.float64).astype(np.float32)).view(np.uint32).astype(np.int64)


def _bits_f32(b):
    return np.ascontiguousarray(np.asarray(b).astype(np.uint32)).view(np.float32).astype(np.float64)


def lovasz_key(e):
    """error_key: e clamped to [0, 1]; k = bits((float)e) for e <= 1/2, 2 bits(1/2) - bits((float)(1 - e)) above; the key is KEY_MAX - k"""
    e = np.clip(np.asarray(e, np.float64), 0.0, 1.0)
    k = np.where(e <= 0.5, _f32_bits(e), LV_KEY_MAX - _f32_bits(1.0 - e))
    return (LV_KEY_MAX - k).astype(np.uint32)


def lovasz_key_error(key):
    """key_error: the f64 error a key stands for (anything for DROPPED, which no caller reads)"""
    k = LV_KEY_MAX - np.asarray(key).astype(np.int64)
    return np.where(k <= LV_HALF_BITS, _bits_f32(np.clip(k, 0, None)), 1.0 - _bits_f32(np.clip(LV_KEY_MAX - k, 0, LV_HALF_BITS)))


def lovasz_p_count(C):
    """units of 2^-52, RELATIVE to p_c, by which the kernel's p = exp(v - m) * (1 / sum_c exp(v_c - m)) and numpy's differ.  One
    evaluation: v - m is exact (f32 operands a few binades apart); exp within 1 ulp <= 2^-52 relative (the figure of the device library
    and of numpy's libm, not measured) on the numerator, and on every term of the sum, which are positive, so 2^-52 on the sum;
    C - 1 additions, 2^-53 each; the reciprocal 2^-53; the product 2^-53: (C + 5) 2^-53.  Two evaluations: (C + 5) 2^-52, + 1 for the
    second order.  p <= 1, so this is also the ABSOLUTE error A of the issue; relative to p it is the tighter statement"""
    return C + 6


class LovaszRef:
    """f64 state of one case: [C][N] planes p (two-pass softmax, exp * (1 / s) as softmax_stats and the key kernel form it), fg, e = |fg - p|,
    A = the error of e (lovasz_p_count * 2^-52 * p, + 2^-52 e for the rounding of 1 - p where it is not exact), and the key interval
    [key_lo, key_hi] = [key(e + A), key(e - A)] (the key falls as e grows) with the point key(e) in `key`; DROPPED where not kept.
    fgb: the foreground term of the backward, which loads the labels without the ignore index"""
    def __init__(self, x, labels, ignore_index=LV_IGNORE, has_ignore=True):
        B, C, HW = x.shape
        N = B * HW
        lab = labels.reshape(N)
        self.shape, self.N = (B, C, HW), N
        self.kept = ~((lab == ignore_index) & bool(has_ignore))
        inrange = (lab >= 0) & (lab < C)
        cls = np.arange(C)[:, None]
        self.fg = (cls == np.where(inrange & self.kept, lab, -1)[None, :])
        self.fgb = (cls == np.where(inrange, lab, -1)[None, :])
        m = x.max(1)
        E = np.exp(x - m[:, None])
        inv = 1.0 / E.sum(1)
        self.p = (E * inv[:, None]).transpose(1, 0, 2).reshape(C, N)
        self.e = np.abs(self.fg - self.p)
        self.A = 2.0 ** -52 * (lovasz_p_count(C) * self.p + self.e)
        drop = lambda k: np.where(self.kept[None, :], k, np.uint32(LV_DROPPED))
        self.key, self.key_lo, self.key_hi = drop(lovasz_key(self.e)), drop(lovasz_key(self.e + self.A)), drop(lovasz_key(self.e - self.A))
        self.G = self.fg.sum(1)

    def one_key(self):
        """[C][N]: the interval is a single key, so the kernel's key is checked bit for bit (dropped pixels count as such)"""
        return self.key_lo == self.key_hi

    def open_sign(self):
        """[C][N]: |fgb - p| within its own error, where lovasz_bwd_kernel's sign branch may go either way"""
        d = np.abs(self.fgb - self.p)
        return d <= 2.0 ** -52 * (lovasz_p_count(self.shape[1]) * self.p + d)


def lovasz_order(keys, fg_kept):
    """the stable ascending order of one class's keys [N] and the payload plane it implies: pixel | fg << 31"""
    order = np.argsort(keys, kind='stable')
    return order, (order.astype(np.uint32) | (fg_kept[order].astype(np.uint32) << np.uint32(31)))


def lovasz_weights(fg_sorted, kept_sorted, variant):
    """lovasz_weight_kernel's g per RANK in f64, in its operation order (IEEE division: reproducible bit for bit), 0 at dropped ranks:
    I = G - F_r, U = G + (r + 1) - F_r; berman (variant 1) and rank 0: 1 / U at a foreground rank, I / (U (U - 1)) at a background one;
    reference (variant 0): ((r + 1) U0 - U) / (U U0) with U0 = G (rank 0 foreground) or G + 1.  All zeros for an absent class"""
    n = fg_sorted.size
    fg = fg_sorted.astype(np.int64)
    G = int(fg.sum())
    if G == 0:
        return np.zeros(n), G
    Fr = np.cumsum(fg)
    r1 = np.arange(1, n + 1, dtype=np.int64)
    I, U = G - Fr, G + r1 - Fr
    U0 = G if fg_sorted[0] else G + 1
    Ud = U.astype(np.float64)
    berman = np.where(fg_sorted, 1.0 / Ud, I.astype(np.float64) / (Ud * np.maximum(U - 1, 1).astype(np.float64)))
    if variant == 1:
        g = berman
    else:
        g = (r1 * U0 - U).astype(np.float64) / (Ud * float(U0))
        g[0] = berman[0]
    return np.where(kept_sorted, g, 0.0), G


def lovasz_tile_sums(keys_sorted, g):
    """(sum, sum |.|) of key_error(key) * g over the ranks of every tile, f64"""
    kept = keys_sorted != np.uint32(LV_DROPPED)
    t = np.where(kept, lovasz_key_error(np.where(kept, keys_sorted, 0)) * g, 0.0)
    at = np.arange(0, t.size, LV_TILE)
    return np.add.reduceat(t, at), np.add.reduceat(np.abs(t), at)


def wave_sum_lane0(v):
    """lane 0 of wave_sum (csrc/common.h): v += shfl_xor(v, m) for m = 32 .. 1, over [..., 64]"""
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ m]
    return v[..., 0]


def lovasz_final(partial, G):
    """lovasz_final_kernel on the rows partial [C][ntiles]: thread t adds tiles t, t + NT, ... in turn, wave_sum, the 4 waves in turn, the
    present classes in turn; (float)(total / present).  Returns (f32 loss, present)"""
    C, ntiles = partial.shape
    total, present = 0.0, 0
    for c in range(C):
        if G[c] == 0:
            continue
        s = np.zeros(LV_NT)
        for i0 in range(0, ntiles, LV_NT):
            seg = partial[c, i0:i0 + LV_NT]
            s[:seg.size] = s[:seg.size] + seg
        lc = 0.0
        for w in wave_sum_lane0(s.reshape(LV_NT // 64, 64)):
            lc = lc + float(w)
        total, present = total + lc, present + 1
    return (np.float32(total / present) if present else np.float32(0.0)), present


def lovasz_bwd_slack(C):
    """units of 2^-52, relative to T = p (|D| + sum_c p_c |D_c|) scale, of lovasz_bwd_kernel's f64 value against numpy's.  p carries
    a = lovasz_p_count(C) (both evaluations).  Per evaluation: D is exact; a term D_c p_c one rounding and the C additions of dot one each,
    (C + 1) 2^-53 of sum |terms|; D - dot, the product with p and with scale one each, 3 * 2^-53 (scale itself is the same IEEE
    quotient on both sides).  The |D| part: a + 3 * 2^-53 each side; the dot part: 2 a (p enters twice) + (C + 4) 2^-53 each side.  Two sides:
    2 a + (C + 4) = 3 C + 16, + 1 for the second order"""
    return 2 * lovasz_p_count(C) + C + 4 + 1


def lovasz_bwd_ref(ref, W, n_present, grad_out, open_option=None):
    """lovasz_bwd_kernel in f64 with the kernel's own weight plane W [C][N] (f32 values): diff = fgb - p, D = -w (diff > 0), w (diff < 0),
    0; dot = sum_c D_c p_c; d = p (D - dot) scale, scale = (double)(float)grad_out / n_present (0 when nothing is present; grad_out None:
    1).  open_option in (-1, 0, 1): the sign taken where the branch is open (ref.open_sign()).  Returns (d, T) as [C][N]"""
    scale = float(np.float32(1.0 if grad_out is None else grad_out)) / float(n_present) if n_present > 0 else 0.0
    diff = ref.fgb - ref.p
    sign = np.where(diff > 0, -1.0, np.where(diff < 0, 1.0, 0.0))
    if open_option is not None:
        sign = np.where(ref.open_sign(), float(open_option), sign)
    W = np.asarray(W, np.float64)
    D = sign * W
    dot = (D * ref.p).sum(0)
    return ref.p * (D - dot[None, :]) * scale, ref.p * (W + (ref.p * W).sum(0)[None, :]) * abs(scale)


def lovasz_bwd_bound(g, T, C, bf16):
    """one rounding of the stored type on the f64 value, the f64 slack, and the smallest normal f32 (a flushed denormal)"""
    return (2.0 ** -8 if bf16 else 2.0 ** -24) * np.abs(g) + 2.0 ** -52 * lovasz_bwd_slack(C) * T + 2.0 ** -126


class LvCase:
    def __init__(self, name, B, C, HW, chunks=(0,), has_ignore=(1,), populated=False, equal=False):
        self.name, self.B, self.C, self.HW, self.chunks, self.has_ignore = name, B, C, HW, chunks, has_ignore
        self.populated, self.equal = populated, equal
        self.N = B * HW

    def __repr__(self):
        return self.name


LV_CASES = [LvCase('smallest', 1, 2, 8),                                  # one group; a tile of 4088 idle lanes that act as the largest digit
            LvCase('one_tile', 1, 3, 4096),                               # exactly one tile
            LvCase('tile_and_group', 1, 3, 4104),                         # a second tile of 8 elements
            LvCase('three_ragged', 3, 5, 2736),                           # 3 tiles, the last ragged; images end inside a tile
            LvCase('carry', 1, 2, 1052680, populated=True),               # 257 tiles and a group: the second trip of both carry loops, the strided digit total
            LvCase('carry_batched', 2, 2, 526344),                        # the same tile count from two images, one run
            LvCase('chunked', 1, 19, 4104, chunks=(0, 4, 1)),             # chunks of 19, 4 (the last ragged: 4 * 4 + 3) and 1 classes
            LvCase('c256', 1, 256, 16, has_ignore=(1, 0)),                # label 255 ignored, then a class
            LvCase('all_equal', 1, 2, 4104, populated=True, equal=True)]  # added: every kept error 1/2 exactly, the seam of the key, tied in all 4 digits
LV_BY_NAME = {c.name: c for c in LV_CASES}
LV_SMALL = [c for c in LV_CASES if c.N <= 8208]


def lovasz_operands(case):
    """(x [B][C][HW] f64, labels [B][HW] int64, plants {name: flat pixel}).  Logits: multiples of 2^-4 in [-4, 4] (7 significant bits: exact
    in bf16), so that no error is below e^-8 / C and the key of a random pixel is decided far from an f32 rounding seam; `equal`: all 0.
    Labels: about 10 % 255; -1 at three pixels, 300 at two; the last pixels a run of 255, so that real DROPPED keys sit next to the padding
    lanes of the last tile.  C >= 3: class 1 absent, class `single` (C - 1; 254 of 256, where 255 is the ignore label) at one pixel,
    planted classes t = 0 and o = single.  C == 2 populated: both classes drawn, t = 0, o = 1.  C == 2 otherwise: class 1 absent, class
    0 at the planted pixel alone and every other kept label out of range (-1 or 300).
    Plants (image 0; exempt from the one-key condition):
      'zero'  label t, x_t = 32 and every other class -32: p_t = 1 and e = 0 exactly in f64 on both sides: key KEY_MAX, the branch diff == 0
      'one'   label t, x_t = -32, x_o = 32, the rest -32: e_t = 1 - e^-64 = 1 exactly (key 0, a FOREGROUND rank 0 of class t) and e_o =
              p_o = 1 exactly (key 0, a BACKGROUND rank 0 of class o): both values of U0
    (`smallest` and `carry_batched` have no second pixel of class 0, so no 'zero'; `all_equal` has no plants)"""
    B, C, HW, N = case.B, case.C, case.HW, case.N
    g = case_gen(4714, B, C, HW, int(case.equal))
    x = (torch.randint(-64, 65, (B, C, HW), generator=g).double() / 16).numpy()
    if case.equal:
        x[:] = 0.0
    lab = torch.randint(0, C, (B, HW), generator=g).numpy()
    r = torch.rand((B, HW), generator=g).numpy()
    sparse = C == 2 and not case.populated
    single = None
    if C >= 3:
        single = C - 1 if C != 256 else 254
        lab[(lab == 1) | (lab == single)] = 0
    if sparse:
        lab = np.where(lab == 0, -1, 300)
    lab[r < 0.10] = LV_IGNORE
    flat = lab.reshape(N)
    if N >= 16:
        flat[7:10], flat[10:12] = -1, 300
    flat[N - max(2, min(24, N // 4)):] = LV_IGNORE
    plants = {}
    if not case.equal:
        t, o = 0, (single if C >= 3 else 1)
        if single is not None:
            flat[5] = single
        if not sparse:
            plants['zero'] = 1
            flat[1] = t
            x[0, :, 1], x[0, t, 1] = -32.0, 32.0
        i = 2 if not sparse else 0
        plants['one'] = i
        flat[i] = t
        x[0, :, i], x[0, t, i], x[0, o, i] = -32.0, -32.0, 32.0
    return x, lab, plants


def lovasz_pipeline(x, labels, variant, ignore_index=LV_IGNORE, has_ignore=True, grad_out=None, ref=None):
    """the whole restated forward and backward in f64 on the point keys: dict(loss (f64, before its f32 rounding), present, G [C],
    W [C][N] (f32 values as f64), grad [B][C][HW]); with `ref` (a LovaszRef) x and labels are not read.  What tests/test_exact_bounds.py
    pins to tests/lovasz_ref.py"""
    ref = ref or LovaszRef(x, labels, ignore_index, has_ignore)
    B, C, HW = ref.shape
    W, total, present = np.zeros((C, ref.N)), 0.0, 0
    for c in range(C):
        fgk = ref.fg[c]
        order, _ = lovasz_order(ref.key[c], fgk)
        ks = ref.key[c][order]
        g, G = lovasz_weights(fgk[order], ks != np.uint32(LV_DROPPED), variant)
        W[c, order] = g.astype(np.float32)
        if G > 0:
            total, present = total + float(lovasz_tile_sums(ks, g)[0].sum()), present + 1
    d, _ = lovasz_bwd_ref(ref, W, present, grad_out)
    return dict(loss=total / present if present else 0.0, present=present, G=ref.G, W=W,
                grad=d.reshape(C, B, HW).transpose(1, 0, 2))


# ---------------------------------------------------------------------------------------------------------- planar cross-entropy and OHEM
# tss_cross_entropy_fwd / _bwd (ce_fwd_kernel, ce_bwd_kernel of csrc/loss.hip) and tss_ohem_fwd / _bwd (ohem_pixel_kernel, ohem_bwd_kernel of
# csrc/ohem.hip): lsw::lse8 and lsw::grad8 of csrc/losssweep.h, which soft_lse_count and soft_p_count above already count.
PLANAR_CE_BIG = (1, 1, 4097 * 256 * 8)       # 4097 * 256 groups: one more block than tss::grid_for's cap of 4096, so block 0's lanes take two trips
PLANAR_CE_SHAPES = SOFT_PLANAR + [SOFT_BEHIND, PLANAR_CE_BIG]
PLANAR_CE_SUM_REL = 2.0 ** -40               # the f64 loss sum: <= 2 * 8 terms per lane, 6 wave_sum levels, 4 waves, <= 4096 atomics in any order:
#                                              under 4200 * 2^-53 < 2^-40 of sum |terms|


def planar_ce_operands(shape):
    """soft_planar_operands and, with C >= 2, one more planted pixel 'exact' (image 0, pixel 6): label 0 at 16 and every other class at -16.
    The other classes add (C - 1) e^-32 < 2^-38 to a running sum of 1.f, which stays 1.f, and __logf(1.f) is 0: the stored lse IS x_t and
    the pixel's cross-entropy an exact 0 (in f64 it is 2e-13, inside the bound of lse).  With C == 1 every pixel is such a pixel"""
    x, lab, plants = soft_planar_operands(*shape, behind=shape == SOFT_BEHIND)
    if shape[1] >= 2 and shape != SOFT_BEHIND:
        x[0, :, 6], x[0, 0, 6], lab[0, 6] = -16.0, 16.0, 0
        plants['exact'] = 6
    return x, lab, plants


class PlanarCeRef:
    """reference and bounds of the planar cross-entropy on a PlanarRef (has_ignore: both entries always apply their ignore index):
      lse, lse_bound      per pixel: U32 soft_lse_count
      ce, ce_bound        per pixel: max(lse - x_t, 0) where the pixel counts, 0 elsewhere; lse's bound and the subtraction's rounding
      total, total_bound  the f64 sum of the counted lse - x_t: the per-pixel bounds added up, + PLANAR_CE_SUM_REL sum |terms|"""
    def __init__(self, ref):
        self.ref = ref
        self.k = soft_lse_count(ref)
        self.lse, self.lse_bound = ref.lse, U32 * self.k * 1.001
        xt = np.take_along_axis(ref.x, ref.t[:, None, :], 1)[:, 0]
        self.ce = np.where(ref.valid, np.maximum(ref.lse - xt, 0.0), 0.0)
        self.ce_bound = np.where(ref.valid, self.lse_bound + U32 * 1.001 * self.ce, 0.0)
        self.total = float(self.ce.sum())
        self.total_bound = float(self.ce_bound.sum()) + PLANAR_CE_SUM_REL * self.total
        self.kp = None

    def grad(self, w, bf16):
        """(g, bound) [B][C][HW] of lsw::grad8<false> with the per-pixel weight w [B][HW] (f64 of the f32 the kernel forms; 0 where the pixel
        does not count): g = (p - h) w.  e = __expf(x - l) from the stored l: soft_p_count, relative to p; the weight's own product, h - e
        and the product with w one rounding each, relative to p + h (soft_p_count's docstring); __expf may flush a result below 2^-126"""
        ref = self.ref
        if self.kp is None:
            self.kp = _first_order(soft_p_count(ref, self.k))
        h = ref.onehot.astype(np.float64)
        g = (ref.p - h) * w[:, None]
        bound = np.abs(w)[:, None] * (ref.p * self.kp + (ref.p + h) * (3 * U32 * 1.001) + 2.0 ** -126)
        return g, bound + (2.0 ** -8 * (np.abs(g) + bound) if bf16 else 0.0)
