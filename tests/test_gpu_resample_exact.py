"""Each C entry point of csrc/resample.hip and csrc/gate.hip and csrc/ppm.hip, called ONCE per case through _native.call, against an f64 reference on dyadic
operands (tests/exact.py), with the harness of the other exact-operand files (tests/exact_gpu.py): sentinel-filled outputs with a pitch
wider than the channel count, a 16-byte column offset where the entry allows one, SPARE sentinel rows behind, sentinel pad channels in
the input pitches, NaN statistics slabs, sentinel workspaces.  The pointer-table entries (tss_ppm_*) take ctypes arrays (ptr_table).

Tiers (derived in tests/exact.py, run on the CPU in tests/test_exact_bounds.py; no bound or cap comes from what a GPU returned):
  1  bit for bit: the size pair is X.exact_resize on both axes and X.exact_budget holds for the case's own operands, so nothing in the
     kernel rounds before the store.  f32 bits == the f64 reference, bf16 bits == X.rne_bf16 of it.  The backward gathers sum up to a
     whole output map, so their tier-1 operands are the 4-bit X.dyadic_q (multiples of 2^-4 below 2), not the 8-bit X.dyadic
  3  tss_ppm_arms_bwd in training mode only: see its entry below
  2  X.resample_excess on the restated f32 taps (X.tap_matrix_f32), and the same outputs against X.bilinear_matrix within
     X.bilinear_f32_slack (X.resize_matrix_excess / X.resize_bwd_matrix_excess).  The restated taps form l1 with ONE fused multiply-add,
     as the disassembly shows every l1 of the bilinear NHWC, planar, head-backward and concat-backward kernels is formed: those are
     held to the u-counted bound alone.  upsample_head_fwd_kernel fuses six of its eight l1 and upsample_head_fwd_generic_kernel and
     ppm_concat_fwd_kernel none (the compiler's choice per use): only their cases add X.tap_slack, which admits either form
Which case uses which:
  tss_bilinear_nhwc_fwd / _bwd      1 on 5x9 -> 17x33, 2x3 -> 17x33, the identity, every pair with an extent of 1 (1x1 -> 12x20: scale 0,
                                    the window is the whole extent, 12 / 20 rows in 4-per-trip steps); 2 on 13x21 -> 32x50 and the
                                    downscale 17x33 -> 6x11.  dx AND the f32 workspace tmp (the row pass alone) are checked
  tss_bilinear_planar_fwd           all four (input, output) dtype instances: 1 on 5x9 -> 17x33, 2 on 17x33 -> 6x11, 3 planes, the image
                                    between NaN guards; the f32 -> bf16 instance is rne_bf16 of the f32 -> f32 instance's bits
  tss_upsample_head_fwd / _bwd      2 throughout: W % 8 == 0 makes W - 1 odd, so the head's WIDTH is never exact_resize; the height is
                                    (5 -> 17) on half of the cases -- there the backward's row pass (tmp) is tier 1, on narrow operands -- and not (6 -> 14) on the others.  The seven width pairs next to the
                                    dispatch thresholds 7 sx < 0.99 / 1.99 (X.head_instance restates the dispatch, X.head_columns_hold
                                    the column window of the instance) and 6 -> 24, the smallest pair whose lanes READ the fourth
                                    column of the 4-column instance (none of the seven does: tests/test_exact_bounds.py), N = 19 with ldl = 24 (ragged last class group, sentinel pad
                                    classes in `low` that must reach no plane), N = 8, N = 5 with ldl = 5 (generic at a fast scale)
  tss_adaptive_pool_fwd / _bwd,     the window sum is exact in f32 (X.exact_budget), then one correctly rounded division
  tss_ppm_pool_fwd / _bwd           (X.pool_fwd_excess); backward X.resample_excess with X.pool_bwd_ref's chain.  With a workspace the
                                    slice count is asserted against tss_ppm_pool_slices and every workspace row against the restated
                                    slice walk, bit for bit (exact sums)
  tss_ppm_concat_fwd / _bwd         1 on 17x33 with bins (1, 2, 3, 6) and narrow operands, 2 on 12x20 (its one-bin arm is 1 too); per arm unlinked + ReLU
                                    (one bin), linked + ReLU (2 bins), unlinked, linked without ReLU.  Backward: e per arm after the mask act > 0 (exact zeros of the
                                    pre-activation planted: they are masked), slab row q == (t, t (raw - mean)) of the STORED t bit for
                                    bit, rows >= B bins^2 exact zeros, no NaN left; 512 rows in use, and the refusal at 513
  tss_copy_nhwc                     bit for bit
  tss_gate_fwd / _bwd               X.gate_fwd_bound / X.gate_da_bound (the __expf chain of X.sigmoid_rel_err); where a == 0 was
                                    planted s = 0.5 exactly: f32 bit for bit, bf16 rne_bf16; dx = g s like the forward
  tss_ppm_arms_fwd (csrc/ppm.hip)   y within X.conv_excess (K = C); mean, invstd, gamma invstd and the running statistics within
                                    X.arms_vec_ref, formed from the kernel's own stored y; P = 512, P = 1, eval mode
  tss_ppm_arms_bwd                  eval mode (gamma invstd a power of two: g exact) within X.conv_excess (K = Ca) / X.wgrad_excess (chain =
                                    ceil(P / 32) MFMA steps + 1); training mode in tier 3: the f64 g of the f64 coefficients, one bf16 ulp
                                    of allowance per element nearer to a rounding tie than the derived f32 error of the kernel's g
                                    (X.arms_bwd_ref), at most 1 % of the elements; dgamma, dbeta, vec[3..5]; accumulate 0 and 1;
                                    P = 130, 512, 1; Ca = 16
Not covered here: tss_gate_slices' 1024 / B arm, which needs HW > 64 x 342 pixels at B <= 3."""
import pytest
import torch

from tests import exact as X
from tests.exact_gpu import DEV, Buf, GuardedImage, N_, check_resample, dev, int_table, long_table, nan_slabs, ptr_table, to_rows

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [BF, F32]


gen, narrow, tier1 = X.case_gen, X.narrow, X.resize_tier1


def sync():
    torch.cuda.synchronize()


def code(dtype):
    return N_().dtype_code(dtype)


# ----------------------------------------------------------------------------------------------------- tss_bilinear_nhwc_*
BILINEAR = X.RS_BILINEAR


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Hi,Wi,Ho,Wo,C,tier', BILINEAR)
def test_bilinear_nhwc_fwd(Hi, Wi, Ho, Wo, C, tier, dtype):
    n, B = N_(), 2
    x = X.bilinear_fwd_operand(Hi, Wi, Ho, Wo, C)
    xb, yb = Buf(B * Hi * Wi, C, C + 8, 0, to_rows(x), dtype, nan_spare=True), Buf(B * Ho * Wo, C, C + 16, 8, dtype=dtype)
    n.call('tss_bilinear_nhwc_fwd', xb.ptr, xb.ld, yb.ptr, yb.ld, B, Hi, Wi, Ho, Wo, C, code(dtype), n.stream())
    sync()
    ref, S = X.resize_ref(x, Ho, Wo)
    t1 = tier1(x, S, [(Hi, Ho), (Wi, Wo)])
    assert t1 == (tier == 1), 'the case is not of the tier it names'
    what = ('bilinear fwd', Hi, Wi, Ho, Wo, C, dtype)
    out = check_resample(yb, to_rows(ref), to_rows(S), X.BLEND_N, what, t1)
    ex = X.resize_matrix_excess(X.nhwc_to_nchw(out, B, Ho, Wo, C), x, Ho, Wo, dtype == BF)
    assert ex <= 0, (what, 'against bilinear_matrix', ex)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Hi,Wi,Ho,Wo,C,tier', BILINEAR)
def test_bilinear_nhwc_bwd(Hi, Wi, Ho, Wo, C, tier, dtype):
    n, B = N_(), 2
    dy = X.bilinear_bwd_operand(Hi, Wi, Ho, Wo, C, tier)
    dyb, dxb = Buf(B * Ho * Wo, C, C + 8, 0, to_rows(dy), dtype), Buf(B * Hi * Wi, C, C + 16, 8, dtype=dtype)
    tmp = Buf(B * Hi * Wo, C, C, 0, dtype=F32)
    n.call('tss_bilinear_nhwc_bwd', dyb.ptr, dyb.ld, dxb.ptr, dxb.ld, tmp.ptr, B, Hi, Wi, Ho, Wo, C, code(dtype), n.stream())
    sync()
    t, ta, ref, S = X.resize_bwd_ref(dy, Hi, Wi)
    t1 = tier1(dy, S, [(Hi, Ho), (Wi, Wo)]) and tier1(dy, ta, [(Hi, Ho)])
    assert t1 == (tier == 1), 'the case is not of the tier it names'
    ny = X.window_len(Hi, Ho) + 1
    nx = ny + X.window_len(Wi, Wo) + 1
    what = ('bilinear bwd', Hi, Wi, Ho, Wo, C, dtype)
    check_resample(tmp, to_rows(t), to_rows(ta), ny, what + ('tmp',), t1)
    out = check_resample(dxb, to_rows(ref), to_rows(S), nx, what, t1)
    ex = X.resize_bwd_matrix_excess(X.nhwc_to_nchw(out, B, Hi, Wi, C), dy, Hi, Wi, nx, dtype == BF)
    assert ex <= 0, (what, 'against bilinear_matrix', ex)


# ----------------------------------------------------------------------------------------------------- tss_bilinear_planar_fwd
def run_planar(Hi, Wi, Ho, Wo, tin, tout):
    n, P = N_(), 3
    x = X.dyadic((1, P, Hi, Wi), gen(3, Hi, Wi, Ho, Wo), zero_frac=0.03)
    img, yb = GuardedImage(x, tin), Buf(P * Ho, Wo, Wo, 0, dtype=tout)
    n.call('tss_bilinear_planar_fwd', img.ptr, code(tin), yb.ptr, code(tout), P, Hi, Wi, Ho, Wo, n.stream())
    sync()
    return x, yb


@pytest.mark.parametrize('tout', DTYPES)
@pytest.mark.parametrize('tin', DTYPES)
@pytest.mark.parametrize('Hi,Wi,Ho,Wo,tier', [(5, 9, 17, 33, 1), (17, 33, 7, 11, 2)])
def test_bilinear_planar_fwd(Hi, Wi, Ho, Wo, tier, tin, tout):
    x, yb = run_planar(Hi, Wi, Ho, Wo, tin, tout)
    ref, S = X.resize_ref(x, Ho, Wo)
    t1 = tier1(x, S, [(Hi, Ho), (Wi, Wo)])
    assert t1 == (tier == 1)
    what = ('planar', Hi, Wi, Ho, Wo, tin, tout)
    out = check_resample(yb, ref.reshape(-1, Wo), S.reshape(-1, Wo), X.BLEND_N, what, t1)
    ex = X.resize_matrix_excess(out.reshape(ref.shape), x, Ho, Wo, tout == BF)
    assert ex <= 0, (what, 'against bilinear_matrix', ex)


def test_planar_f32_to_bf16_is_the_rounded_f32_instance():
    """the two instances share planar_bilinear: on a tier-2 pair (nothing is exact) the bf16 output is the f32 output's value rounded
    once, bit for bit.  Two instances, one call each"""
    _, y32 = run_planar(17, 33, 7, 11, F32, F32)
    _, y16 = run_planar(17, 33, 7, 11, F32, BF)
    assert torch.equal(y32.t[:y32.P].to(BF).view(torch.int16), y16.t[:y16.P].view(torch.int16))


# ----------------------------------------------------------------------------------------------------- tss_upsample_head_*
HEAD = X.RS_HEAD


def head_cases():
    out = []
    for i, (w, W, inst) in enumerate(HEAD):
        out.append((w, W, 19, 24, inst, i))
    out += [(11, 72, 8, 8, 'three', 8), (6, 24, 8, 16, 'four', 9), (11, 72, 5, 5, 'generic', 10), (2, 8, 5, 5, 'generic', 11)]
    return out


def head_heights(i):
    return (5, 17) if i % 2 == 0 else (6, 14)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('w,W,N,ldl,inst,i', head_cases())
def test_upsample_head_fwd(w, W, N, ldl, inst, i, dtype):
    n, B = N_(), 2
    h, H = head_heights(i)
    assert X.head_instance(w, W, ldl, N) == inst
    assert inst == 'generic' or X.head_columns_hold(w, W, 3 if inst == 'three' else 4)
    low = X.dyadic((B, N, h, w), gen(4, w, W, N), zero_frac=0.03)
    lb, yb = Buf(B * h * w, N, ldl, 0, to_rows(low), dtype, nan_spare=True), Buf(B * N * H, W, W, 0, dtype=dtype)
    n.call('tss_upsample_head_fwd', lb.ptr, lb.ld, yb.ptr, B, N, h, w, H, W, code(dtype), n.stream())
    sync()
    ref, S = X.resize_ref(low, H, W)
    what = ('head fwd', w, W, N, ldl, inst, dtype)
    out = check_resample(yb, ref.reshape(-1, W), S.reshape(-1, W), X.BLEND_N, what, slack=X.tap_slack(low, H, W).reshape(-1, W))
    ex = X.resize_matrix_excess(out.reshape(ref.shape), low, H, W, dtype == BF)
    assert ex <= 0, (what, 'against bilinear_matrix', ex)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('w,W,N,ldl,inst,i', head_cases())
def test_upsample_head_bwd(w, W, N, ldl, inst, i, dtype):
    n, B = N_(), 2
    h, H = head_heights(i)
    gs = 0.25 if i % 2 else None
    exact_h = X.exact_resize(h, H) is not None          # 5 -> 17: the row pass alone is tier 1 on narrow operands
    dy = narrow((B, N, H, W), gen(5, w, W, N), 0.03) if exact_h else X.dyadic((B, N, H, W), gen(5, w, W, N), zero_frac=0.03)
    dyb, tmp = Buf(B * N * H, W, W, 0, dy.reshape(-1, W), dtype), Buf(B * N * h, W, W, 0, dtype=F32)
    dlb = Buf(B * h * w, N, ldl, 0, dtype=dtype)
    gsd = torch.tensor([gs], dtype=F32, device=DEV) if gs else None
    n.call('tss_upsample_head_bwd', dyb.ptr, n.ptr(gsd), tmp.ptr, dlb.ptr, dlb.ld, B, N, h, w, H, W, code(dtype), n.stream())
    sync()
    t, ta, ref, S = [v * (gs or 1.0) for v in X.resize_bwd_ref(dy, h, w)]
    ny = X.window_len(h, H) + 1
    nx = ny + X.window_len(w, W) + 1
    what = ('head bwd', w, W, N, ldl, gs, dtype)
    assert tier1(dy, ta, [(h, H)]) == exact_h
    check_resample(tmp, t.reshape(-1, W), ta.reshape(-1, W), ny, what + ('tmp',), exact_h)
    out = check_resample(dlb, to_rows(ref), to_rows(S), nx, what)
    ex = X.resize_bwd_matrix_excess(X.nhwc_to_nchw(out, B, h, w, N), dy, h, w, nx, dtype == BF, gs or 1.0)
    assert ex <= 0, (what, 'against bilinear_matrix', ex)


# ----------------------------------------------------------------------------------------------------- tss_adaptive_pool_*
POOL = X.RS_POOL


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('H,W,C,bins', POOL)
def test_adaptive_pool_fwd(H, W, C, bins, dtype):
    n, B = N_(), 2
    x = X.dyadic((B, C, H, W), gen(6, H, W, C, bins), zero_frac=0.03)
    xb, yb = Buf(B * H * W, C, C + 8, 0, to_rows(x), dtype), Buf(B * bins * bins, C, C + 8, 8, dtype=dtype)
    n.call('tss_adaptive_pool_fwd', xb.ptr, xb.ld, yb.ptr, yb.ld, B, H, W, C, bins, code(dtype), n.stream())
    sync()
    sums, sabs, cnt = X.pool_ref(x, bins)
    assert X.exact_budget(sabs, X.lsb_exp(x)), 'the window sums are not exact in f32'
    ex = X.pool_fwd_excess(yb.rows(), to_rows(sums), to_rows(cnt.expand_as(sums)), dtype == BF)
    assert ex <= 0, ('pool fwd', H, W, C, bins, dtype, ex)
    assert yb.untouched()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('H,W,C,bins', POOL)
def test_adaptive_pool_bwd(H, W, C, bins, dtype):
    n, B = N_(), 2
    dy = X.dyadic((B, C, bins, bins), gen(7, H, W, C, bins), zero_frac=0.03)
    dyb, dxb = Buf(B * bins * bins, C, C + 8, 0, to_rows(dy), dtype), Buf(B * H * W, C, C + 16, 8, dtype=dtype)
    n.call('tss_adaptive_pool_bwd', dyb.ptr, dyb.ld, dxb.ptr, dxb.ld, B, H, W, C, bins, code(dtype), n.stream())
    sync()
    ref, S, chain = X.pool_bwd_ref([dy], H, W, [bins])
    check_resample(dxb, to_rows(ref), to_rows(S), chain, ('pool bwd', H, W, C, bins, dtype))


# ----------------------------------------------------------------------------------------------------- tss_ppm_pool_*
PPM_POOL = X.RS_PPM_POOL


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,binss,H,W,C,use_ws,S', PPM_POOL)
def test_ppm_pool_fwd(B, binss, H, W, C, use_ws, S, dtype):
    n = N_()
    cells = sum(b * b for b in binss)
    if use_ws:
        assert X.ppm_pool_slices(B, cells) == S == n.lib().tss_ppm_pool_slices(B, cells)
    x = X.dyadic((B, C, H, W), gen(8, B, H, W, C, len(binss)), zero_frac=0.03)
    xb = Buf(B * H * W, C, C + 8, 0, to_rows(x), dtype)
    ys = [Buf(B * b * b, C, C + 8, 8, dtype=dtype) for b in binss]
    ws = Buf(B * cells * S, C, C, 0, dtype=F32) if use_ws else None
    n.call('tss_ppm_pool_fwd', xb.ptr, xb.ld, ptr_table(ys), long_table(ys), int_table(binss), len(binss), ws.ptr if ws else None,
           B, H, W, C, code(dtype), n.stream())
    sync()
    for yb, bins in zip(ys, binss):
        sums, sabs, cnt = X.pool_ref(x, bins)
        assert X.exact_budget(sabs, X.lsb_exp(x)), 'the window sums are not exact in f32'
        ex = X.pool_fwd_excess(yb.rows(), to_rows(sums), to_rows(cnt.expand_as(sums)), dtype == BF)
        assert ex <= 0, ('ppm pool fwd', B, binss, bins, dtype, ex)
        assert yb.untouched()
    if ws:
        want, row = torch.zeros(B * cells * S, C, dtype=torch.float64), 0
        for b in range(B):
            for bins in binss:
                for y0, y1 in X.pool_windows(H, bins):
                    for x0, x1 in X.pool_windows(W, bins):
                        for r0, r1 in X.ppm_slice_rows(y0, y1, S):
                            want[row] = x[b, :, r0:r1, x0:x1].sum((1, 2))
                            row += 1
        assert torch.equal(ws.rows(), want), 'a workspace row differs from the restated slice walk'
        assert ws.untouched()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('radd', [False, True])
@pytest.mark.parametrize('binss', [(3,), (1, 2, 3, 6)])
def test_ppm_pool_bwd(binss, radd, dtype):
    n, B, H, W, C = N_(), 2, 13, 21, 16
    g = gen(9, len(binss), radd)
    dys = [X.dyadic((B, C, b, b), g, zero_frac=0.03) for b in binss]
    r = X.dyadic((B, C, H, W), g) if radd else None
    dyb = [Buf(B * b * b, C, C + 8, 0, to_rows(d), dtype) for d, b in zip(dys, binss)]
    rb = Buf(B * H * W, C, C + 8, 0, to_rows(r), dtype) if radd else None
    dxb = Buf(B * H * W, C, C + 16, 8, dtype=dtype)
    n.call('tss_ppm_pool_bwd', ptr_table(dyb), long_table(dyb), int_table(binss), len(binss), dxb.ptr, dxb.ld,
           rb.ptr if rb else None, rb.ld if rb else 0, B, H, W, C, code(dtype), n.stream())
    sync()
    ref, S, chain = X.pool_bwd_ref(dys, H, W, binss, r)
    check_resample(dxb, to_rows(ref), to_rows(S), chain, ('ppm pool bwd', binss, radd, dtype))


# ----------------------------------------------------------------------------------------------------- tss_ppm_concat_*
BINS, LINK, RELU = X.RS_BINS, X.RS_LINK, X.RS_RELU


class Arms(X.ArmOperands):
    """X.ArmOperands with their device buffers and link vectors"""
    def __init__(self, g, B, ca, tier, dtype, binss=BINS, link=LINK, relu=RELU):
        super().__init__(g, B, ca, tier, dtype == BF, binss, link, relu)
        self.vec = [[dev(v.reshape(-1)) if v is not None else None for v in lk] for lk in self.links]
        self.rawb = [Buf(B * b * b, ca, ca + 8, 8, to_rows(r), dtype, nan_spare=True) for r, b in zip(self.raw, binss)]

    def tables(self):
        return (ptr_table(self.rawb), long_table(self.rawb), int_table(self.binss), ptr_table([v[0] for v in self.vec]),
                ptr_table([v[1] for v in self.vec]), ptr_table([v[2] for v in self.vec]), int_table(self.relu))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,ca', [(8, 8), (32, 16)])
@pytest.mark.parametrize('H,W,tier', [(17, 33, 1), (12, 20, 2)])
def test_ppm_concat_fwd(H, W, tier, C, ca, dtype):
    n, B = N_(), 2
    g = gen(10, H, W, C, ca)
    A = Arms(g, B, ca, tier, dtype)
    x = X.dyadic((B, C, H, W), g, zero_frac=0.03)
    Ct = C + 4 * ca
    xb, ob = Buf(B * H * W, C, C + 8, 0, to_rows(x), dtype), Buf(B * H * W, Ct, Ct + 16, 8, dtype=dtype)
    n.call('tss_ppm_concat_fwd', xb.ptr, xb.ld, *A.tables(), 4, ob.ptr, ob.ld, B, H, W, C, ca, code(dtype), n.stream())
    sync()
    out = ob.rows()
    assert ob.untouched()
    assert torch.equal(out[:, :C], to_rows(x)), 'the copied channels differ'
    for k, bins in enumerate(BINS):
        ref, S = X.resize_ref(A.act[k], H, W)
        t1 = tier1(A.act[k], S, [(bins, H), (bins, W)])
        assert t1 == (tier == 1 or bins == 1), 'the arm is not of the tier the case names (the one-bin arm is a broadcast: always 1)'
        got = out[:, C + k * ca:C + (k + 1) * ca]
        what = ('concat fwd', H, W, C, ca, dtype, 'arm', k)
        if t1:
            assert torch.equal(got, X.out_bits_ref(to_rows(ref), dtype == BF)), what
        else:
            ex = X.resample_excess(got, to_rows(ref), to_rows(S), X.BLEND_N, dtype == BF, to_rows(X.tap_slack(A.act[k], H, W)))
            assert ex <= 0, (what, ex)
            ex = X.resize_matrix_excess(X.nhwc_to_nchw(got, B, H, W, ca), A.act[k], H, W, dtype == BF)
            assert ex <= 0, (what, 'against bilinear_matrix', ex)


def run_concat_bwd(B, H, W, C, ca, tier, dtype, binss=BINS, link=LINK, relu=RELU, stats=None):
    n = N_()
    g = gen(11, B, H, W, C, ca)
    A = Arms(g, B, ca, tier, dtype, binss, link, relu)
    na = len(binss)
    Ct = C + na * ca
    dout = narrow((B, Ct, H, W), g, 0.03) if tier == 1 else X.dyadic((B, Ct, H, W), g, zero_frac=0.03)
    db = Buf(B * H * W, Ct, Ct + 8, 0, to_rows(dout), dtype)
    eb = [Buf(B * b * b, ca, ca + 8, 8, dtype=dtype) for b in binss]
    stats = stats if stats is not None else [True] * na
    slabs = [nan_slabs(ca) for _ in binss]
    rawt, ldr, bt, mt, st, bet, rt = A.tables()
    n.call('tss_ppm_concat_bwd', db.ptr, db.ld, rawt, ldr, bt, mt, st, bet, rt, ptr_table([s if on else None for s, on in zip(slabs, stats)]),
           ptr_table(eb), long_table(eb), na, B, H, W, C, ca, code(dtype), n.stream())
    sync()
    assert db.untouched()
    for k, bins in enumerate(binss):
        gk = dout[:, C + k * ca:C + (k + 1) * ca]
        _, _, ref, S = X.resize_bwd_ref(gk, bins, bins)
        keep = (A.pre[k] > 0).double() if relu[k] else torch.ones_like(ref)
        ref, S = ref * keep, S * keep
        t1 = tier1(gk, S, [(bins, H), (bins, W)])
        assert t1 == (tier == 1 or bins == 1), 'the arm is not of the tier the case names (the one-bin arm is a plain sum: always 1)'
        what = ('concat bwd', B, H, W, C, ca, dtype, 'arm', k)
        e = check_resample(eb[k], to_rows(ref), to_rows(S), X.concat_gather_chain(bins, H, W, ca), what, t1)
        s = slabs[k].double().cpu()
        if not stats[k]:
            assert torch.isnan(s).all(), (what, 'a slab written without bstats')
            continue
        faults = X.concat_slab_faults(s, e, to_rows(A.xc[k]), B * bins * bins)
        assert not faults, (what, faults)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,ca', [(8, 8), (32, 16)])
@pytest.mark.parametrize('H,W,tier', [(17, 33, 1), (12, 20, 2)])
def test_ppm_concat_bwd(H, W, tier, C, ca, dtype):
    run_concat_bwd(2, H, W, C, ca, tier, dtype, stats=[True, True, False, True])


@pytest.mark.parametrize('dtype', DTYPES)
def test_ppm_concat_bwd_fills_all_512_slab_rows(dtype):
    assert 8 * 8 * 8 == N_().stat_slabs()
    run_concat_bwd(8, 9, 9, 8, 8, 1, dtype, binss=(8,), link=(True,), relu=(1,))


def test_ppm_concat_bwd_refuses_513_slab_rows():
    with pytest.raises(RuntimeError, match='TSS_ERR_SHAPE'):
        run_concat_bwd(57, 4, 4, 8, 8, 2, BF, binss=(3,), link=(True,), relu=(1,))


# ----------------------------------------------------------------------------------------------------- tss_copy_nhwc
@pytest.mark.parametrize('dtype', DTYPES)
def test_copy_nhwc_into_a_channel_slice(dtype):
    n, P, C = N_(), 301, 24
    x = X.dyadic((P, C), gen(12), zero_frac=0.03)
    xb, yb = Buf(P, C, C + 8, 0, x, dtype), Buf(P, C, C + 32, 16, dtype=dtype)
    n.call('tss_copy_nhwc', xb.ptr, xb.ld, yb.ptr, yb.ld, P, C, code(dtype), n.stream())
    sync()
    assert torch.equal(yb.rows(), x) and yb.untouched()


# ----------------------------------------------------------------------------------------------------- tss_gate_*
GATE = X.RS_GATE


def gate_operands(B, HW, C, seed):
    g = gen(seed, B, HW, C)
    x = X.dyadic((B, HW, C), g, zero_frac=0.03)
    a = X.dyadic((B, 1, C), g, zero_frac=0.25)
    assert bool((a == 0).any()) and bool((a != 0).any())
    return g, x, a


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('add_one', [0.0, 1.0])
@pytest.mark.parametrize('B,HW,C,S', GATE)
def test_gate_fwd(B, HW, C, S, add_one, dtype):
    n = N_()
    _, x, a = gate_operands(B, HW, C, 13)
    xb, ab = Buf(B * HW, C, C + 8, 0, x.reshape(-1, C), dtype), Buf(B, C, C + 8, 0, a.reshape(B, C), dtype)
    ob = Buf(B * HW, C, C + 16, 8, dtype=dtype)
    n.call('tss_gate_fwd', xb.ptr, xb.ld, ab.ptr, ab.ld, ob.ptr, ob.ld, B, HW, C, add_one, code(dtype), n.stream())
    sync()
    check_gated(ob, x, a, add_one, dtype, ('gate fwd', B, HW, C, add_one, dtype))


def check_gated(ob, x, a, add_one, dtype, what):
    ref, bound = X.gate_fwd_bound(x, a.expand_as(x), add_one, dtype == BF)
    out = ob.rows().reshape(x.shape)
    assert ob.untouched(), (what, 'sentinel overwritten')
    ex = ((out - ref).abs() - bound).max().item()
    assert ex <= 0, (what, 'excess over the bound', ex)
    z = (a == 0).expand_as(x)
    assert torch.equal(out[z], X.out_bits_ref(ref[z], dtype == BF)), (what, 's = 0.5 is not exact where a == 0')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('add_one', [0.0, 1.0])
@pytest.mark.parametrize('B,HW,C,S', GATE)
def test_gate_bwd(B, HW, C, S, add_one, dtype):
    n = N_()
    assert X.gate_slices(B, HW) == S == n.lib().tss_gate_slices(B, HW)
    walk = X.gate_slice_walk(HW, S)
    assert walk[-1][1] == HW and all(q1 > q0 for q0, q1 in walk)
    g, x, a = gate_operands(B, HW, C, 14)
    gr = X.dyadic((B, HW, C), g, zero_frac=0.03)
    mk = lambda t: Buf(B * HW, C, C + 8, 0, t.reshape(-1, C), dtype)
    gb, xb, ab = mk(gr), mk(x), Buf(B, C, C + 8, 0, a.reshape(B, C), dtype)
    dxb, dab, ws = Buf(B * HW, C, C + 16, 8, dtype=dtype), Buf(B, C, C + 8, 8, dtype=dtype), Buf(B * S, C, C, 0, dtype=F32)
    n.call('tss_gate_bwd', gb.ptr, gb.ld, xb.ptr, xb.ld, ab.ptr, ab.ld, dxb.ptr, dxb.ld, dab.ptr, dab.ld, ws.ptr, B, HW, C, add_one,
           code(dtype), n.stream())
    sync()
    what = ('gate bwd', B, HW, C, add_one, dtype)
    check_gated(dxb, gr, a, add_one, dtype, what + ('dx',))
    prod = gr * x
    ref, bound = X.gate_da_bound(prod.sum(1), prod.abs().sum(1), a.reshape(B, C), X.gate_chain(HW, S, C), dtype == BF)
    ex = ((dab.rows() - ref).abs() - bound).max().item()
    assert ex <= 0, (what, 'da excess over the bound', ex)
    assert dab.untouched() and ws.untouched(), (what, 'sentinel overwritten')
    # the workspace rows are the slices' own sums: gamma of the in-slice chain, from the restated walk
    want = torch.stack([prod[:, q0:q1].sum(1) for q0, q1 in walk], 1).reshape(B * S, C)
    wabs = torch.stack([prod[:, q0:q1].abs().sum(1) for q0, q1 in walk], 1).reshape(B * S, C)
    ex = X.resample_excess(ws.rows(), want, wabs, X.gate_chain(HW, S, C) - S, False)
    assert ex <= 0, (what, 'a workspace row differs from the restated slice walk', ex)


# ----------------------------------------------------------------------------------------------------- tss_ppm_arms_fwd
@pytest.mark.parametrize('C,Ca,Ps,training', X.RS_ARMS)
def test_ppm_arms_fwd(C, Ca, Ps, training):
    """y within X.conv_excess (K = C, exact products); vec[0..2] and the running statistics within X.arms_vec_ref, formed from the
    kernel's own stored y; vec[3..5] (the backward's) untouched; num_batches_tracked incremented once; eval mode writes y alone"""
    n, na = N_(), len(Ps)
    ops = X.arms_operands(C, Ca, Ps)
    assert n.lib().tss_ppm_arms_supported(na, C, Ca, int_table(Ps), code(BF)) == 1
    xb = [Buf(o['P'], C, C + 8, 0, o['x'], BF, nan_spare=True) for o in ops]
    yb = [Buf(o['P'], Ca, Ca + 12, 4, dtype=BF) for o in ops]
    f32 = lambda k: [dev(o[k]).contiguous() for o in ops]
    w, gamma, rmean, rvar = f32('w'), f32('gamma'), f32('rmean'), f32('rvar')
    nbt = [torch.full((1,), 7, dtype=torch.int64, device=DEV) for _ in ops]
    vec = [torch.full((6, Ca), float('nan'), device=DEV) for _ in ops]
    n.call('tss_ppm_arms_fwd', ptr_table(xb), long_table(xb), ptr_table(w), ptr_table(gamma), ptr_table(rmean), ptr_table(rvar),
           ptr_table(nbt), ptr_table(yb), long_table(yb), ptr_table(vec), int_table(Ps), na, C, Ca, training, X.ARMS_EPS, X.ARMS_MOMENTUM,
           code(BF), n.stream())
    sync()
    for k, o in enumerate(ops):
        what = ('arms fwd', C, Ca, o['P'], training, 'arm', k)
        ref, S = o['x'] @ o['w'].T, o['x'].abs() @ o['w'].abs().T
        yq = yb[k].rows()
        ex = X.conv_excess(yq, ref, S, C)
        assert ex <= 0 and yb[k].untouched(), (what, 'y', ex)
        v = vec[k].double().cpu()
        got = dict(mean=v[0], invstd=v[1], scale=v[2], rmean=rmean[k].double().cpu(), rvar=rvar[k].double().cpu())
        if not training:
            assert torch.isnan(v).all() and int(nbt[k]) == 7, (what, 'eval mode wrote statistics')
            assert torch.equal(got['rmean'], o['rmean']) and torch.equal(got['rvar'], o['rvar']), what
            continue
        assert torch.isnan(v[3:]).all() and int(nbt[k]) == 8, (what, 'vec[3..5] / num_batches_tracked')
        for name, (r, b) in X.arms_vec_ref(yq, o['gamma'], o['rmean'], o['rvar']).items():
            ex = ((got[name] - r).abs() - b).max().item()
            assert ex <= 0, (what, name, 'excess over the bound', ex)


def test_ppm_arms_supported_refuses_what_the_kernels_cannot_take():
    sup = lambda C, Ca, Ps, dt=BF: N_().lib().tss_ppm_arms_supported(len(Ps), C, Ca, int_table(Ps), code(dt))
    assert sup(32, 16, (512, 1)) == 1 and sup(128, 32, (3, 12, 27, 108)) == 1
    assert sup(16, 16, (3,)) == 0 and sup(32, 8, (3,)) == 0 and sup(32, 16, (513,)) == 0 and sup(32, 16, (3,), F32) == 0


# ----------------------------------------------------------------------------------------------------- tss_ppm_arms_bwd
@pytest.mark.parametrize('C,Ca,Ps,training,accumulate', X.RS_ARMS_BWD)
def test_ppm_arms_bwd(C, Ca, Ps, training, accumulate):
    """X.arms_bwd_ref: eval mode with a power-of-two gamma invstd (g exact: conv_excess / wgrad_excess alone), training mode in tier 3
    (the near-tie allowance; the share of near-tie elements is capped); dgamma, dbeta, vec[3..5]; accumulate 0 (NaN prior contents
    must not reach the result) and 1 (dyadic prior contents)"""
    n, na = N_(), len(Ps)
    ops = X.arms_bwd_operands(C, Ca, Ps, training, accumulate)
    eb = [Buf(o['P'], Ca, Ca + 8, 0, o['e'], BF, nan_spare=True) for o in ops]
    yb = [Buf(o['P'], Ca, Ca + 16, 0, o['y'], BF, nan_spare=True) for o in ops]
    xb = [Buf(o['P'], C, C + 8, 0, o['x'], BF, nan_spare=True) for o in ops]
    ib = [Buf(o['P'], C, C + 12, 4, dtype=BF) for o in ops]
    nan = float('nan')
    prior = lambda k: [dev(o[k]).contiguous() if accumulate else torch.full(o[k].shape, nan, device=DEV) for o in ops]
    w, gamma = [dev(o['w']).contiguous() for o in ops], [dev(o['gamma']) for o in ops]
    dw, dgamma, dbeta = prior('dw0'), prior('dgamma0'), prior('dbeta0')
    vec = []
    for o in ops:
        v = torch.full((6, Ca), nan)
        v[0], v[1] = o['mean'].float(), o['invstd'].float()
        vec.append(v.to(DEV))
    n.call('tss_ppm_arms_bwd', ptr_table(eb), long_table(eb), ptr_table(yb), long_table(yb), ptr_table(xb), long_table(xb), ptr_table(w),
           ptr_table(gamma), ptr_table(vec), ptr_table(dw), ptr_table(dgamma), ptr_table(dbeta), accumulate, ptr_table(ib), long_table(ib),
           int_table(Ps), na, C, Ca, training, code(BF), n.stream())
    sync()
    for k, o in enumerate(ops):
        what = ('arms bwd', C, Ca, o['P'], training, accumulate, 'arm', k)
        R = X.arms_bwd_ref(o, training, accumulate)
        assert float(R['near'].double().mean()) <= X.NEAR_TIE_CAP, (what, 'too many g elements near a rounding tie')
        v = vec[k].double().cpu()
        assert torch.equal(v[0], o['mean']) and torch.equal(v[1], o['invstd']) and torch.isnan(v[2]).all(), (what, 'vec[0..2] touched')
        got = dict(ga=v[3], gb=v[4], gce=v[5], dgamma=dgamma[k].double().cpu(), dbeta=dbeta[k].double().cpu(), dw=dw[k].double().cpu(),
                   e_in=ib[k].rows())
        for name, out in got.items():
            ref, bound = R[name]
            ex = ((out - ref).abs() - bound).max().item()
            assert ex <= 0, (what, name, 'excess over the bound', ex)
        assert ib[k].untouched(), (what, 'sentinel overwritten')
