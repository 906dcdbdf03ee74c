"""tss_bneck_eval_fwd (csrc/bneck.hip), tss_bn_eval_affine / tss_bn_eval_affine_batched and tss_join_fwd / tss_join_bwd (csrc/pointwise.hip),
each called ONCE per case through _native.call, against an f64 reference on exactly representable operands (tests/exact.py, last
section) with the harness of the other exact-operand files (tests/exact_gpu.py): outputs in sentinel-filled buffers with a pitch wider
than the channel count, a column offset, SPARE sentinel rows behind; NaN in the input's pad columns and spare rows; NaN statistics slabs.
No bound or cap comes from what a GPU returned; all of them are run on the CPU in tests/test_exact_bounds.py.

Bottleneck.  Every case asserts X.bneck_route (the restated tile choice) against the library's tss_bneck_eval_tile and against the form
the case names, so a planner that moves fails the case instead of silently uncovering a form.
  tier 1  bit for bit.  Fixed-point operands (multiples of 2^-2, power-of-two scales, means and betas on the stage's grid): X.bneck_exact
          asserts from the case's own operands that no f32 operation of any stage rounds; the stored bits equal X.bneck_ref's, which
          rounds where the kernel rounds on purpose (D, E at stride 2, y; to bf16, nearest even).  X.bneck_conditions asserts that at most
          70 % of the outputs are zero, that >= 10 % of D and of y are changed by their rounding with at least one exact tie each, and
          that relu(bn1(0)) > 0 on half of the expanded channels (an E not zeroed outside the image shows).  X.BK_TIER1:
            8 x 16   (64, 192, 64) + skip and (64, 128, 48) on 2 x 57 x 250: 256 blocks exactly, ragged on both axes, three chunks
            8 x 8    (128, 128, 128) + skip on 113 x 105 (8 x 16 would not fit the LDS); (32, 64, 32) on 80 x 160 (200 tiles exactly);
                     (96, 64, 96) + skip on 2 x 57 x 250 (256 blocks of 8 x 16 that do not fit: the LDS test alone decides)
            4 x 8    (128, 768, 128) + skip on 13 x 21; (96, 128, 96) + skip on 3 x 5 x 9; (8, 64, 16) on 4 x 8 and 5 x 9 (Cin padded to
                     32, a single chunk); (40, 128, 20) on 1 x 9, 9 x 1 and 13 x 21 (Cin padded to 64, a quarter output fragment,
                     ldy = 28); (48, 64, 48) + skip on 3 x 1 x 1 and without on 3 x 5 x 9
            4 x 16, stride 2 (E in bf16)   (64, 128, 96) on 9 x 33 -> 5 x 17, 2 x 13 x 21 and 2 x 1 x 1; (8, 64, 20) on 8 x 32 -> 4 x 16
                     and 2 x 2 -> 1 x 1; (64, 768, 128) on 13 x 21
          weights: both bf16 copies; neither (the f32 parameters carry +-2^-20, which the kernel's conversion removes); a copy pointer
          off 16-byte alignment holding the NEGATED weights (the entry must fall back to the f32 parameter)
  tier 2  X.BK_TIER2, one or two cases per form: 8-bit X.dyadic operands, ordinary gamma / running_var / eps, the affines written by
          tss_bn_eval_affine_batched and read back; |out - ref| <= the running error bound X.bneck_ref carries (zero wherever no bf16
          rounding tie of y lies within the running error, whole bf16 ulps elsewhere).  The largest |out - ref| / bound per case
          is printed before the assertion (profiles/bneck_tier2_margins.txt)
  refused X.BK_REFUSED: a skip with Cin != Cout or at stride 2, Cmid = 96, Cout = 132 and the stride-2 (128, 768, 128), whose one tile
          form needs 211 KB of LDS: TSS_ERR_SHAPE, tss_bneck_eval_supported 0, nothing written
Affines.  mean bit for bit, invstd within 3 u and scale within 4 u of f64 (X.affine_ref); batched == single bit for bit; sentinels intact.
Joins.  Forward: X.dyadic operands and power-of-two scales make each branch and the sum exact in f32 (asserted): f32 output == the value,
bf16 output == its rne_bf16.  With a seed slot the forward also applies nn.Dropout: the kept set is predicted by tests/philox_ref.py
(Philox4x32-10 in numpy), kept values times 1 / (1 - p) (p = 1/2, 3/4: exact), bit for bit, and bit for bit tss_dropout of the plain join.
Backward: e bit for bit (ReLU mask, dout_scale 2 and 4, in place), the statistics rows within X.stats_excess of
the STORED e with the restated lane chain, the rows in use against the restated grid (check_slab_rows)."""
import ctypes

import pytest
import torch

from tests import exact as X
from tests import philox_ref
from tests.exact_gpu import (DEV, Buf, N_, affine_batched, bneck_call, bneck_tile, check_slab_rows, dev, nan_slabs, to_rows)

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [BF, F32]
gen = X.case_gen


def sync():
    torch.cuda.synchronize()


def code(dtype):
    return N_().dtype_code(dtype)


def same_bits(out, want, what):
    bad = (out != want).nonzero()
    assert bad.numel() == 0, (what, 'not bit for bit at', bad[:3].tolist(), len(bad), 'of', out.numel(), 'elements')


# ----------------------------------------------------------------------------------------------------- tss_bneck_eval_fwd
def assert_route(c):
    assert X.bneck_supported(c.Cin, c.Cmid, c.Cout, c.stride, c.res)
    assert N_().lib().tss_bneck_eval_supported(c.Cin, c.Cmid, c.Cout, c.stride, c.res, N_().TSS_BF16) == 1
    assert bneck_tile(c) == X.bneck_route(c.B, c.H, c.W, c.Cin, c.Cout, c.stride) == c.form, 'the case no longer reaches its tile form'
    S, TH, TW = X.BK_FORMS[c.form]
    assert X.bneck_lds(S, TH, TW, c.Cin, c.Cout) <= X.BK_LDS


@pytest.mark.parametrize('c', X.BK_TIER1, ids=repr)
def test_bneck_tier1_bit_for_bit(c):
    o = X.BkOperands(c, 1)
    r = X.bneck_ref(o, o.bn)
    assert X.bneck_exact(o, r), ('the case breaks its exactness budget', X.bneck_bits(r))
    ok, census = X.bneck_conditions(o, r)
    assert ok, census
    assert_route(c)
    yb = bneck_call(o, [tuple(dev(v) for v in st) for st in o.bn])
    same_bits(yb.rows(), to_rows(r['y']), c)
    assert yb.untouched(), (c, 'sentinel overwritten')


@pytest.mark.parametrize('c', X.BK_TIER2, ids=repr)
def test_bneck_tier2_running_error_bound(c):
    o = X.BkOperands(c, 2)
    assert_route(c)
    outs, jobs = [], []
    for gamma, rm, rv, beta in o.frozen:
        C = gamma.numel()
        outs.append(torch.zeros(3 * C, dtype=F32, device=DEV))
        jobs.append((dev(gamma), dev(rm), dev(rv), outs[-1], C, X.BK_EPS))
    affine_batched(jobs)
    bn_dev = [(a[:st[0].numel()], a[2 * st[0].numel():], dev(st[3])) for a, st in zip(outs, o.frozen)]
    yb = bneck_call(o, bn_dev)
    r = X.bneck_ref(o, [(m.double().cpu(), s.double().cpu(), b.double().cpu()) for m, s, b in bn_dev], bound=True)
    out, ref, bound = yb.rows(), to_rows(r['y']), to_rows(r['bound'])
    diff = (out - ref).abs()
    loose = bound > 0
    ratio = float((diff[loose] / bound[loose]).max()) if bool(loose.any()) else 0.0
    print('bneck tier 2 %r: max |out - ref| / bound = %.3f over the %.2f %% of the elements with a bound > 0; the others are held bit '
          'for bit; %d elements differ from the reference at all' % (c, ratio, 100.0 * float(loose.double().mean()), int((diff > 0).sum())))
    assert not torch.isnan(out).any(), c
    assert bool((diff <= bound).all()), (c, 'excess over the running error bound', float((diff - bound).max()))
    assert yb.untouched(), (c, 'sentinel overwritten')


@pytest.mark.parametrize('Cin,Cmid,Cout,stride,res', X.BK_REFUSED)
def test_bneck_refuses(Cin, Cmid, Cout, stride, res):
    n = N_()
    assert not X.bneck_supported(Cin, Cmid, Cout, stride, res)
    assert n.lib().tss_bneck_eval_supported(Cin, Cmid, Cout, stride, res, n.TSS_BF16) == 0
    B, H, W = 1, 5, 9
    xb, yb = Buf(B * H * W, Cin, Cin, 0, torch.zeros(B * H * W, Cin)), Buf(B * H * W, Cout, Cout + 8, 4)
    v = [torch.zeros(max(Cmid, Cout), dtype=F32, device=DEV) for _ in range(3)]
    w = torch.zeros(max(Cmid * Cin, Cout * Cmid, Cmid * 9), dtype=F32, device=DEV)
    p = lambda t: t.data_ptr()
    rc = n.lib().tss_bneck_eval_fwd(xb.ptr, xb.ld, p(w), None, p(v[0]), p(v[1]), p(v[2]), p(w), p(v[0]), p(v[1]), p(v[2]), p(w), None,
                                    p(v[0]), p(v[1]), p(v[2]), res, yb.ptr, yb.ld, B, H, W, Cin, Cmid, Cout, stride, n.TSS_BF16, n.stream())
    sync()
    assert rc == -2, rc
    yb.C = 0
    assert yb.untouched()


def test_a_stride2_block_too_wide_for_the_kernel_goes_layer_by_layer():
    """tss_bneck_eval_supported now answers 0 where the one stride-2 tile form does not fit the LDS (Cin = 128): the product's eval forward
    of such a block runs layer by layer, with the bits of the layer-by-layer switch, instead of failing with TSS_ERR_SHAPE"""
    import importlib
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    mod = importlib.import_module('torch_semantic_segmentation_amd.models.fastscnn')
    torch.manual_seed(3)
    m = mod.BottleneckBlock(128, 128, stride=2, expansion=1).to(DEV).eval()
    tssa.set_compute_dtype(m, BF)
    x = torch.randn(1, 128, 9, 13, generator=torch.Generator().manual_seed(4)).to(DEV).to(BF)
    assert ops.eval_bottleneck and not X.bneck_supported(128, 128, 128, 2, 0)
    outs = []
    for fused in (True, False):
        ops.eval_bottleneck = fused
        try:
            with torch.no_grad():
                assert not fused or ops.bottleneck_eval(x, m.conv1, m.conv2, m.conv3) is None
                outs.append(ops.materialize(m(x)).float().cpu())
        finally:
            ops.eval_bottleneck = True
    sync()
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])


def test_bneck_tile_query_follows_the_restated_route():
    """the read-only query over the thresholds of the planner: block counts next to 256 and 200, the LDS fit of 8 x 16, stride 2"""
    lib = N_().lib()
    for B, H, W in [(2, 57, 250), (2, 57, 240), (1, 113, 105), (1, 80, 160), (1, 80, 152), (1, 13, 21), (4, 64, 128), (1, 128, 256),
                    (1, 1, 1), (3, 200, 200)]:
        for Cin, Cout in [(64, 64), (64, 128), (96, 96), (128, 128), (8, 16), (128, 16), (32, 128)]:
            for stride in (1, 2):
                assert lib.tss_bneck_eval_tile(B, H, W, Cin, Cout, stride) == X.bneck_route(B, H, W, Cin, Cout, stride), (B, H, W, Cin, Cout, stride)
    assert lib.tss_bneck_eval_tile(2, 57, 250, 64, 64, 1) == 816 and lib.tss_bneck_eval_tile(2, 57, 250, 128, 128, 1) == 808


# ----------------------------------------------------------------------------------------------------- tss_bn_eval_affine(_batched)
def affine_operands(C, key, gamma=True):
    g = gen(83, C, key)
    u = lambda lo, hi: (lo + (hi - lo) * torch.rand((C,), generator=g, dtype=torch.float64)).float().double()
    rv = torch.exp(torch.rand((C,), generator=g, dtype=torch.float64) * 16 - 10).float().double()     # variances over 2^-14 .. 2^9
    return (u(-2, 2) if gamma else None), u(-3, 3), rv


def affine_window(C):
    """an f32 buffer with sentinel in front of and behind the 3 C outputs: (tensor, pointer of the window)"""
    t = X.sentinel((3 * C + 32,), DEV, F32)
    return t, t.data_ptr() + 64


def check_affine(t, C, gamma, rm, rv, eps, what):
    w = t.cpu()
    b = X.bits(w).clone()
    assert bool((b[:16] == X.SENTINEL_BITS32).all()) and bool((b[16 + 3 * C:] == X.SENTINEL_BITS32).all()), (what, 'sentinel overwritten')
    out = w[16:16 + 3 * C].double().view(3, C)
    mean, invstd, scale = X.affine_ref(gamma, rm, rv, eps)
    assert torch.equal(out[0], mean), (what, 'mean is a copy')
    assert X.affine_excess(out[1], invstd, X.AFFINE_U[0]) <= 0, (what, 'invstd')
    assert X.affine_excess(out[2], scale, X.AFFINE_U[1]) <= 0, (what, 'scale')
    if gamma is None:
        assert torch.equal(out[2], out[1]), (what, 'gamma NULL: scale is invstd')
    return w[16:16 + 3 * C]


AFFINE_JOBS = [(1, True, 1e-5), (130, True, 1e-5), (768, True, 1e-3), (130, False, 1e-5), (8, True, 1e-5)]


def single_affine(C, gamma_on, eps):
    n = N_()
    gamma, rm, rv = affine_operands(C, int(gamma_on), gamma_on)
    t, ptr = affine_window(C)
    keep = [dev(gamma), dev(rm), dev(rv)]
    n.call('tss_bn_eval_affine', None if gamma is None else keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), eps,
           ptr, ptr + 4 * C, ptr + 8 * C, C, n.stream())
    sync()
    return t, (gamma, rm, rv), keep


@pytest.mark.parametrize('C,gamma_on,eps', AFFINE_JOBS)
def test_bn_eval_affine(C, gamma_on, eps):
    t, (gamma, rm, rv), _ = single_affine(C, gamma_on, eps)
    check_affine(t, C, gamma, rm, rv, eps, ('affine', C, gamma_on))


def test_bn_eval_affine_batched_equals_the_single_jobs():
    """one launch over jobs of different C (8 is far below max_channels = 768: six of its seven blocks find no channel), one of them with
    gamma 0 (NULL): every window within the bound, equal to the single-job bits, sentinels intact"""
    singles, jobs, wins = [], [], []
    for C, gamma_on, eps in AFFINE_JOBS:
        t1, (gamma, rm, rv), keep = single_affine(C, gamma_on, eps)
        t, ptr = affine_window(C)
        singles.append((t1, gamma, rm, rv))
        wins.append(t)
        jobs.append((keep[0], keep[1], keep[2], ptr, C, eps))
    affine_batched(jobs, 768)
    for (C, gamma_on, eps), t, (t1, gamma, rm, rv) in zip(AFFINE_JOBS, wins, singles):
        w = check_affine(t, C, gamma, rm, rv, eps, ('batched affine', C, gamma_on))
        assert torch.equal(X.bits(w), X.bits(t1.cpu()[16:16 + 3 * C])), ('batched != single', C)


# ----------------------------------------------------------------------------------------------------- tss_join_fwd
def join_branch(P, C, g, affine):
    """(x [P][C], (mean, scale, bias) or None): exact zeros of the branch's pre-activation planted"""
    if not affine:
        return X.dyadic((P, C), g, zero_frac=0.25), None
    mean, bias, scale = X.dyadic((C,), g), X.dyadic((C,), g), X.pow2((C,), g, 0.5, 4)
    return X.plant_zeros(X.dyadic((P, C), g), mean, scale, bias, g, 0.25), (mean, scale, bias)


def aff_ptrs(aff):
    """device (mean, scale, bias) of a branch, or three NULLs: scale NULL means identity"""
    if aff is None:
        return [None, None, None], [None, None, None]
    keep = [dev(v) for v in aff]
    return keep, [k.data_ptr() for k in keep]


# (C, P kind, two branches, affine on a, affine on b, relu)
JOIN_FWD = [(8, 'one', 1, 1, 1, 1), (8, 'short', 1, 1, 1, 1), (8, 'grid', 1, 1, 1, 1), (24, 'one', 1, 1, 1, 0), (24, 'short', 1, 1, 1, 1),
            (24, 'grid', 1, 0, 0, 1), (24, 'short', 1, 1, 0, 1), (24, 'short', 1, 0, 1, 0), (24, 'short', 0, 1, 0, 1), (24, 'short', 0, 0, 0, 1),
            (24, 'short', 0, 1, 0, 0), (136, 'one', 1, 1, 1, 1), (136, 'short', 1, 1, 1, 1), (136, 'grid', 0, 1, 0, 1),
            (136, 'second', 1, 1, 1, 1), (2048, 'one', 1, 1, 1, 1), (2048, 'grid', 1, 1, 0, 1)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,kind,two,affa,affb,relu', JOIN_FWD)
def test_join_fwd(C, kind, two, affa, affb, relu, dtype):
    n, P = N_(), X.join_P(kind, C)
    NPL, grid = X.join_geometry(P, C, X.JOIN_FWD_BLOCKS)
    if kind == 'grid':
        assert grid == X.JOIN_FWD_BLOCKS and P == grid * NPL
    if kind == 'second':
        assert 4 * grid * NPL < P < 5 * grid * NPL + grid * NPL and P % (grid * NPL) == 7
    g = gen(91, C, P, two, affa, affb, relu)
    a, A = join_branch(P, C, g, affa)
    b, Bf = join_branch(P, C, g, affb) if two else (None, None)
    ref = X.join_fwd_ref(a, A, b, Bf, relu)
    assert P * C < 2000 or bool((X.join_fwd_ref(a, A, b, Bf, False) == 0).any()), 'no exact zero of the pre-activation sum planted'
    ab = Buf(P, C, C + 8, 0, a, dtype, nan_spare=True)
    bb = Buf(P, C, C + 16, 8, b, dtype, nan_spare=True) if two else None
    ob = Buf(P, C, C + 16, 8, dtype=dtype)
    ka, pa = aff_ptrs(A)
    kb, pb = aff_ptrs(Bf)
    n.call('tss_join_fwd', ab.ptr, ab.ld, pa[0], pa[1], pa[2], bb.ptr if two else None, bb.ld if two else 0, pb[0], pb[1], pb[2],
           ob.ptr, ob.ld, relu, 0.0, None, P, C, code(dtype), n.stream())
    sync()
    what = ('join fwd', C, kind, P, two, affa, affb, relu, dtype)
    same_bits(ob.rows(), X.out_bits_ref(ref, dtype == BF), what)
    assert ob.untouched(), (what, 'sentinel overwritten')


# (C, P kind, two branches): 'second' -- ceil(P / NPL) = 2561 tiles over the 512 blocks, a block takes more than one
JOIN_DROP = [(8, 'one', 1), (24, 'short', 1), (24, 'short', 0), (24, 'grid', 1), (136, 'short', 0), (136, 'second', 1), (136, 'second', 0)]
JOIN_DROP_SEEDS = {0.5: (7 << 32) | 3, 0.75: 2 ** 64 - 1}


def seed_slot(seed):
    return torch.tensor([ctypes.c_int64(seed).value], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('p', [0.5, 0.75])
@pytest.mark.parametrize('C,kind,two', JOIN_DROP)
def test_join_fwd_with_dropout(C, kind, two, p, dtype):
    """the dropout folded into a ReLU join: relu(affA(a) + affB(b)) in f64 (exact), rounded to the dtype, kept elements (the mask of
    philox_ref.dropout_keep on the LOGICAL index pix C + c) times 1 / (1 - p), a power of two, dropped ones 0, rounded again: bit for
    bit; and bit for bit what tss_dropout makes of the plain join's output with the same slot"""
    n, P = N_(), X.join_P(kind, C)
    NPL, grid = X.join_geometry(P, C, X.JOIN_FWD_BLOCKS)
    assert kind != 'second' or X.cdiv(P, NPL) > X.JOIN_FWD_BLOCKS
    g = gen(95, C, P, two)
    a, A = join_branch(P, C, g, True)
    b, Bf = join_branch(P, C, g, True) if two else (None, None)
    seed = JOIN_DROP_SEEDS[p]
    slot = seed_slot(seed)
    bf = dtype == BF
    plain = X.out_bits_ref(X.join_fwd_ref(a, A, b, Bf, True), bf)
    keep = torch.from_numpy(philox_ref.dropout_keep(P, C, p, seed))
    want = X.out_bits_ref(torch.where(keep, plain / (1 - p), torch.zeros_like(plain)), bf)
    assert bool((plain[keep] > 0).any()) and bool((plain[~keep] > 0).any()) or P * C < 100
    ab = Buf(P, C, C + 8, 0, a, dtype, nan_spare=True)
    bb = Buf(P, C, C + 16, 8, b, dtype, nan_spare=True) if two else None
    ka, pa = aff_ptrs(A)
    kb, pb = aff_ptrs(Bf)
    outs = []
    for drop in (True, False):
        ob = Buf(P, C, C + 16, 8, dtype=dtype)
        n.call('tss_join_fwd', ab.ptr, ab.ld, pa[0], pa[1], pa[2], bb.ptr if two else None, bb.ld if two else 0, pb[0], pb[1], pb[2],
               ob.ptr, ob.ld, 1, p if drop else 0.0, slot.data_ptr() if drop else None, P, C, code(dtype), n.stream())
        sync()
        assert ob.untouched(), ('join fwd dropout', C, kind, drop, 'sentinel overwritten')
        outs.append(ob)
    what = ('join fwd dropout', C, kind, P, two, p, dtype)
    same_bits(outs[0].rows(), want, what)
    same_bits(outs[1].rows(), plain, what + ('plain',))
    db = Buf(P, C, C + 8, 0, dtype=dtype)
    n.call('tss_dropout', outs[1].ptr, outs[1].ld, db.ptr, db.ld, P, C, p, slot.data_ptr(), code(dtype), n.stream())
    sync()
    assert torch.equal(X.bits(db.t[:P, :C].cpu()), X.bits(outs[0].t[:P, 8:8 + C].cpu())), (what, 'tss_dropout of the plain join differs')
    assert db.untouched() and slot.item() == ctypes.c_int64(seed).value


def test_join_dropout_refusals():
    """seed_slot without relu; dout_scale != 1 without relu; dout_scale <= 0: TSS_ERR_SHAPE, nothing written"""
    n = N_()
    P, C = 5, 8
    ab, ob, eb = Buf(P, C, C, 0, torch.ones(P, C)), Buf(P, C, C + 8, 0), Buf(P, C, C + 8, 0)
    slot = seed_slot(3)
    with pytest.raises(RuntimeError):
        n.call('tss_join_fwd', ab.ptr, ab.ld, None, None, None, None, 0, None, None, None, ob.ptr, ob.ld, 0, 0.5, slot.data_ptr(), P, C,
               n.TSS_BF16, n.stream())
    bwd = lambda relu, scale: n.call('tss_join_bwd', ab.ptr, ab.ld, ab.ptr if relu else None, ab.ld if relu else 0, relu, None, 0, None, None,
                                     None, 0, None, None, eb.ptr, eb.ld, scale, P, C, n.TSS_BF16, n.stream())
    for relu, scale in ((0, 2.0), (1, 0.0), (1, -2.0), (0, 0.0)):
        with pytest.raises(RuntimeError):
            bwd(relu, scale)
    sync()
    ob.C = eb.C = 0
    assert ob.untouched() and eb.untouched()


def test_join_refuses_2056_channels():
    n = N_()
    ab, ob = Buf(1, 2056, 2056, 0, torch.zeros(1, 2056)), Buf(1, 2056, 2056, 0)
    lib = n.lib()
    assert lib.tss_join_fwd(ab.ptr, ab.ld, None, None, None, None, 0, None, None, None, ob.ptr, ob.ld, 1, 0.0, None, 1, 2056, n.TSS_BF16,
                            n.stream()) == -2
    assert lib.tss_join_bwd(ab.ptr, ab.ld, ab.ptr, ab.ld, 1, None, 0, None, None, None, 0, None, None, ob.ptr, ob.ld, 1.0, 1, 2056,
                            n.TSS_BF16, n.stream()) == -2
    sync()
    ob.C = 0
    assert ob.untouched()


# ----------------------------------------------------------------------------------------------------- tss_join_bwd
# (C, P kind, relu, stats_a, stats_b, e: 'out' | 'inplace' | None, dout_scale)
JOIN_BWD = [(8, 'one', 1, 1, 1, 'out', 1.0), (8, 'short', 1, 1, 1, 'out', 1.0), (8, 'grid', 1, 1, 1, 'out', 2.0),
            (24, 'short', 1, 1, 0, 'out', 1.0), (24, 'short', 1, 0, 1, 'out', 2.0), (24, 'short', 1, 0, 0, 'out', 1.0),
            (24, 'short', 0, 1, 1, 'out', 1.0), (24, 'grid', 1, 1, 1, 'inplace', 1.0), (24, 'short', 1, 1, 1, None, 1.0),
            (136, 'one', 1, 1, 1, 'out', 1.0), (136, 'short', 1, 1, 1, 'inplace', 2.0), (136, 'grid', 1, 1, 1, 'out', 1.0),
            (136, 'second', 1, 1, 1, 'out', 1.0), (2048, 'one', 1, 1, 1, 'out', 1.0), (2048, 'grid', 1, 1, 0, 'out', 1.0),
            # the backward of a join with dropout folded in: dout_scale = 1 / (1 - p) for p = 1/2 and 3/4
            (8, 'short', 1, 1, 1, 'out', 4.0), (24, 'grid', 1, 1, 1, 'out', 4.0), (24, 'short', 1, 1, 1, 'inplace', 4.0),
            (136, 'second', 1, 1, 1, 'out', 2.0), (136, 'second', 1, 1, 0, 'out', 4.0), (2048, 'one', 1, 0, 1, 'out', 4.0)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,kind,relu,sa,sb,emode,dscale', JOIN_BWD)
def test_join_bwd(C, kind, relu, sa, sb, emode, dscale, dtype):
    n, P = N_(), X.join_P(kind, C)
    NPL, grid = X.join_geometry(P, C)
    g = gen(93, C, P, relu, sa, sb, 0 if emode is None else len(emode), int(dscale))
    dout, out = X.dyadic((P, C), g, zero_frac=0.03), X.dyadic((P, C), g).clamp_min(0.0)
    a, bq, ma, mb = X.dyadic((P, C), g), X.dyadic((P, C), g), X.dyadic((C,), g), X.dyadic((C,), g)
    db = Buf(P, C, C + 16, 8, dout, dtype, nan_spare=True)
    ob = Buf(P, C, C + 8, 0, out, dtype, nan_spare=True)
    ab, bb = Buf(P, C, C + 8, 8, a, dtype, nan_spare=True), Buf(P, C, C + 24, 16, bq, dtype, nan_spare=True)
    eb = Buf(P, C, C + 24, 8, dtype=dtype) if emode == 'out' else db if emode == 'inplace' else None
    slab_a, slab_b = (nan_slabs(C) if sa else None), (nan_slabs(C) if sb else None)
    kma, kmb = dev(ma), dev(mb)
    p = lambda t: None if t is None else t.data_ptr()
    n.call('tss_join_bwd', db.ptr, db.ld, ob.ptr if relu else None, ob.ld if relu else 0, relu,
           ab.ptr if sa else None, ab.ld if sa else 0, p(kma) if sa else None, p(slab_a),
           bb.ptr if sb else None, bb.ld if sb else 0, p(kmb) if sb else None, p(slab_b),
           eb.ptr if eb is not None else None, eb.ld if eb is not None else 0, dscale, P, C, code(dtype), n.stream())
    sync()
    what = ('join bwd', C, kind, P, relu, sa, sb, emode, dscale, dtype)
    ref = X.join_bwd_ref(dout, out, relu, dscale)
    e = ref
    if eb is not None:
        e = eb.rows()
        same_bits(e, ref, what)
        if emode == 'out':
            assert eb.untouched(), (what, 'sentinel overwritten')
            same_bits(db.rows(), dout, what + ('dout changed',))
    chain = X.join_stats_chain(P, C)
    assert chain == (6 if kind == 'second' else 1)
    for slab, raw, mean in ((slab_a, a, ma), (slab_b, bq, mb)):
        if slab is None:
            continue
        check_slab_rows(slab, range(grid), what)
        terms = torch.cat([e, e * X.exact_f32(raw - mean)], 1)
        s = slab.double().cpu().sum(0)
        if dtype == F32:
            assert bool(((s - terms.sum(0)).abs() <= 2.0 ** -40 * terms.abs().sum(0)).all()), (what, 'f64 statistics')
        else:
            ex = X.stats_excess(s, X.exact_f32(terms), chain)
            assert ex <= 0, (what, 'statistics excess', ex, 'chain', chain)
