"""tssa.distillation_loss / DistillationLoss (csrc/distill.hip), pixel and channel kind, against the f64 restatement of
tests/distill_ref.py (pinned to F.kl_div and a hand-worked value by tests/test_distill_oracle.py).

Inputs are built on the CPU from fixed seeds: student 2 randn; teacher `indep` (a second 2 randn) or `near` (student + 1e-3
randn).  bf16 inputs are bf16-exact and the restatement reads the same values.

Bounds.
Loss: |loss - ref64| <= 1e-5 |ref64| + tau^2 k 2^-24 M,  M = max(|s|, |t|) / tau + ln N,  N = C (pixel) or h w (channel).
  The relative part is the project's loss bound (test_gpu_softloss.py).  The absolute part is there because a unit's KL is a
  difference of terms of size M (without it `near`, whose loss is ~1e-6, could not be met by any f32 evaluation).
  k = 16 is the number of f32 roundings between the inputs and a unit's KL in csrc/distill.hip, counted from its code (two
  sweeps: exact maxima first, so no running-maximum rescale is on the chain): 1 / tau (1); per softmax fma(x, 1 / tau, -m),
  exp, the sum Z (2 x 3); A = sum e_T (t - s) / tau: t - s, times 1 / tau, the fma sum, A / Z_T (4); m_S - m_T, Z_S / Z_T, log,
  two additions (5).  A sum counts once whatever its length.
Gradient, f32 logits: cases.rel_err <= max(2e-5, 3 d_ref), d_ref the restatement's own f32-vs-f64 distance on that input (in
  `near` the gradient is a difference of near-equal probabilities and d_ref is 1e-4 .. 1e-3).  bf16 logits: 2e-2 (stored in bf16).
"""
import functools
import math

import pytest
import torch

from tests import cases, distill_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K_ROUNDINGS = 16
TAUS = (1.0, 4.0, 0.5)
DTYPES = pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
KINDS = pytest.mark.parametrize('kind', R.KINDS)

#               B,  C,  h,  w
CASES = {
    'sub_wave':    (2, 19, 8, 8),       # 64 positions: fewer than one block's slots; empty partials are identities (ld 24, 5 pads)
    'odd_size':    (1, 19, 5, 7),       # 35 positions, nothing a multiple of anything
    'ragged':      (1, 5, 24, 40),      # 960 positions: the last block / segment ragged; ld 8 with 3 pads
    'odd_batch':   (3, 21, 16, 40),     # odd batch, C > 20
    'two_classes': (2, 2, 8, 8),        # the smallest softmax
    'wide':        (1, 65, 8, 8),       # C > 24: nine 8-channel vectors per row, 7 pads
    'plane':       (1, 3, 64, 96),      # 6144 positions per plane: several blocks per plane
}


@functools.lru_cache(maxsize=None)
def case_input(name, mode, bf16, scale_to=None):
    shape = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 900)
    s = 2.0 * torch.randn(*shape, generator=g)
    t = 2.0 * torch.randn(*shape, generator=g) if mode == 'indep' else s + 1e-3 * torch.randn(*shape, generator=g)
    if scale_to is not None:
        s, t = s * (scale_to / float(s.abs().max())), t * (scale_to / float(t.abs().max()))
    if bf16:
        s, t = s.bfloat16().float(), t.bfloat16().float()
    return s, t


@functools.lru_cache(maxsize=None)
def reference(name, mode, bf16, tau, kind, scale_to=None):
    """(f64 loss, f64 gradient, d_ref, M) of the restatement"""
    s, t = case_input(name, mode, bf16, scale_to)
    l64, g64 = R.loss_and_grad(s, t, torch.float64, tau, kind)
    _, g32 = R.loss_and_grad(s, t, torch.float32, tau, kind)
    assert bool(torch.isfinite(g32).all())
    M = max(float(s.abs().max()), float(t.abs().max())) / tau + math.log(R.units(s.shape, kind)[1])
    return float(l64), g64.numpy(), cases.rel_err(g32.numpy(), g64.numpy()), M


def hip_distill(s, t, tau, kind, dtype=torch.float32, scale=None):
    import torch_semantic_segmentation_amd as tssa
    x = s.to(DEV).to(dtype).requires_grad_(True)
    loss = tssa.distillation_loss(x, t.to(DEV).to(dtype), tau, kind)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    (loss if scale is None else scale * loss).backward()
    return loss.detach().cpu(), x.grad.detach().float().cpu()


def check(tag, got, want, bf16, tau):
    (loss, grad), (want_loss, want_grad, d_ref, M) = got, want
    d_loss = abs(float(loss) - want_loss)
    loss_bound = 1e-5 * abs(want_loss) + tau ** 2 * K_ROUNDINGS * 2.0 ** -24 * M
    d_grad = cases.rel_err(grad.numpy(), want_grad)
    grad_bound = 2e-2 if bf16 else max(2e-5, 3 * d_ref)
    print('%s loss %.6e abs err %.2e bound %.2e | grad d_ref %.2e hip %.2e bound %.2e'
          % (tag, want_loss, d_loss, loss_bound, d_ref, d_grad, grad_bound))
    assert math.isfinite(float(loss)) and bool(torch.isfinite(grad).all())
    assert d_loss <= loss_bound
    assert d_grad <= grad_bound


@pytest.mark.parametrize('mode', ['indep', 'near'])
@pytest.mark.parametrize('tau', TAUS)
@DTYPES
@KINDS
@pytest.mark.parametrize('name', list(CASES))
def test_loss_and_gradient_vs_f64_restatement(name, kind, dtype, tau, mode):
    bf16 = dtype == torch.bfloat16
    s, t = case_input(name, mode, bf16)
    got = hip_distill(s, t, tau, kind, dtype)
    check('%-7s %-11s %-4s tau %.1f %-5s' % (kind, name, 'bf16' if bf16 else 'f32', tau, mode), got,
          reference(name, mode, bf16, tau, kind), bf16, tau)


@DTYPES
@KINDS
@pytest.mark.parametrize('name', ['sub_wave', 'wide', 'plane'])
def test_identical_inputs_give_exactly_zero(name, kind, dtype):
    """The two softmax states run the same operations on the same bits: the loss is exactly 0.0 and so is every gradient element."""
    s, _ = case_input(name, 'indep', dtype == torch.bfloat16)
    for tau in TAUS:
        loss, grad = hip_distill(s, s.clone(), tau, kind, dtype)
        assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


def padded(values, ld, fill, dtype):
    """(B,C,h,w) values as a view of a [B][h][w][ld] buffer whose pad channels hold `fill`"""
    B, C, h, w = values.shape
    base = torch.full((B, h, w, ld), fill, dtype=dtype, device=DEV)
    base[..., :C] = values.permute(0, 2, 3, 1).to(DEV).to(dtype)
    return base.permute(0, 3, 1, 2)[:, :C]


@DTYPES
@KINDS
@pytest.mark.parametrize('name,extra', [('ragged', 0), ('ragged', 8), ('wide', 0)])
def test_poisoned_pad_channels_reach_no_result(name, extra, kind, dtype):
    """Both operands built by hand on an ld > C buffer (`extra`: a whole pad vector beyond round_up(C, 8)), pads NaN against pads 0:
    the same bits, loss and gradient; the gradient's pad channels are zeros."""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    B, C, h, w = CASES[name]
    ld = ops.round_up(C, 8) + extra
    assert ld > C
    s, t = case_input(name, 'indep', dtype == torch.bfloat16)
    out = []
    for fill in (0.0, float('nan')):
        x = padded(s, ld, fill, dtype).detach().requires_grad_(True)
        tt = padded(t, ld, fill, dtype)
        assert ops.is_nhwc(x) and ops.is_nhwc(tt) and ops.ld(x) == ld
        loss = tssa.distillation_loss(x, tt, 4.0, kind)
        (g,) = torch.autograd.grad(loss, x)
        assert ops.is_nhwc(g) and ops.ld(g) == ld
        rows = torch.as_strided(g, (B, h, w, ld), (h * w * ld, w * ld, ld, 1))
        assert float(rows[..., C:].float().abs().max()) == 0.0 and not bool(torch.isnan(rows.float()).any())
        out.append((loss.cpu(), g.float().cpu()))
    assert math.isfinite(float(out[1][0]))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    check('pads %s %s' % (kind, name), out[1], reference(name, 'indep', dtype == torch.bfloat16, 4.0, kind), dtype == torch.bfloat16, 4.0)


@DTYPES
@KINDS
def test_contiguous_nchw_and_its_nhwc_view_give_the_same_bits(kind, dtype):
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    s, t = case_input('odd_batch', 'indep', dtype == torch.bfloat16)
    out = []
    for nhwc in (False, True):
        x, tt = s.to(DEV).to(dtype), t.to(DEV).to(dtype)
        if nhwc:
            x, tt = ops.to_nhwc(x), ops.to_nhwc(tt)
        assert ops.is_nhwc(x) == nhwc and x.is_contiguous() != nhwc
        x = x.detach().requires_grad_(True)
        loss = tssa.distillation_loss(x, tt, 4.0, kind)
        loss.backward()
        out.append((loss.detach().cpu(), x.grad.float().cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@DTYPES
@KINDS
@pytest.mark.parametrize('name', ['sub_wave', 'wide'])
def test_saturated_logits(name, kind, dtype):
    """Logits scaled to +-80 at tau = 0.5 (|x| / tau = 160): everything finite, the same bounds."""
    bf16 = dtype == torch.bfloat16
    s, t = case_input(name, 'indep', bf16, 80.0)
    assert abs(float(s.abs().max()) - 80.0) < 0.5
    check('saturated %s %s' % (kind, name), hip_distill(s, t, 0.5, kind, dtype), reference(name, 'indep', bf16, 0.5, kind, 80.0), bf16, 0.5)


@KINDS
@pytest.mark.parametrize('name', ['plane', 'ragged', 'odd_batch'])
def test_block_cap_changes_the_grid_not_the_result(name, kind):
    """distill_max_blocks 1, 2, 3 against the default: more trips through the same loops, fewer partial rows (channel kind: fewer,
    longer segments per plane; odd_batch with a cap below its 3 images: a block walks several images).  Every cap meets the bounds;
    the pixel kind's gradient does not depend on the partition at all."""
    from torch_semantic_segmentation_amd import ops
    B, C, h, w = CASES[name]
    s, t = case_input(name, 'indep', False)
    want = reference(name, 'indep', False, 4.0, kind)
    lib = ops.N.lib()
    assert ops.distill_max_blocks == 0
    base = hip_distill(s, t, 4.0, kind)
    check('cap 0 %s %s' % (kind, name), base, want, False, 4.0)
    row = 16 if kind == 'pixel' else 5 * 4 * ops.round_up(C, 8)
    kcode = ops.DISTILL_KINDS[kind]
    default_rows = lib.tss_distill_workspace_bytes(kcode, B, C, h * w, 0) // row
    assert default_rows >= 3
    try:
        for cap in (1, 2, 3):
            ops.distill_max_blocks = cap
            nrows = lib.tss_distill_workspace_bytes(kcode, B, C, h * w, cap)
            assert nrows == row * (cap if kind == 'pixel' else max(cap // B, 1) * B)
            got = hip_distill(s, t, 4.0, kind)
            check('cap %d %s %s' % (cap, kind, name), got, want, False, 4.0)
            assert abs(float(got[0]) - float(base[0])) <= 1e-6 * abs(float(base[0]))
            if kind == 'pixel':
                assert torch.equal(got[1], base[1])
            else:
                assert cases.rel_err(got[1].numpy(), base[1].numpy()) <= 1e-5
    finally:
        ops.distill_max_blocks = 0


@KINDS
@pytest.mark.parametrize('name', ['sub_wave', 'plane'])
def test_two_calls_are_bit_identical(name, kind):
    s, t = case_input(name, 'indep', False)
    a, b = hip_distill(s, t, 4.0, kind), hip_distill(s, t, 4.0, kind)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@KINDS
def test_grad_out_is_honoured_and_the_teacher_gets_no_gradient(kind):
    import torch_semantic_segmentation_amd as tssa
    s, t = case_input('sub_wave', 'indep', False)
    loss, grad = hip_distill(s, t, 4.0, kind)
    loss3, grad3 = hip_distill(s, t, 4.0, kind, scale=0.3)
    assert torch.equal(loss, loss3)
    # grad_out multiplies the finished f32 gradient element: one rounding (and float32(0.3) is not 0.3) -> within one ulp
    want = 0.3 * grad.double()
    assert bool(((grad3.double() - want).abs() <= 2.0 ** -23 * want.abs() + 1e-37).all())
    assert float(grad.abs().max()) > 0
    # grad_out of another float dtype
    x = s.to(DEV).requires_grad_(True)
    tt = t.to(DEV).requires_grad_(True)
    out = tssa.distillation_loss(x, tt, 4.0, kind)
    out.backward(torch.tensor(1.0, dtype=torch.float64, device=DEV))
    assert tt.grad is None and torch.equal(x.grad.cpu(), grad)


@KINDS
def test_forward_and_backward_replay_from_a_captured_graph(kind):
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    s1, t1 = case_input('odd_batch', 'indep', False)
    s2, t2 = (2.0 * torch.roll(v, 1, 0) + 0.25 for v in (s1, t1))
    eager = hip_distill(s2, t2, 4.0, kind)
    xs = ops.to_nhwc(s1.to(DEV)).detach().requires_grad_(True)
    ts = ops.to_nhwc(t1.to(DEV))

    def run():
        loss = tssa.distillation_loss(xs, ts, 4.0, kind)
        return loss, torch.autograd.grad(loss, xs)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grad = run()
    with torch.no_grad():
        xs.copy_(s2.to(DEV))
        ts.copy_(t2.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss.cpu(), eager[0]) and torch.equal(grad.float().cpu(), eager[1])


def test_module_and_argument_errors():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    s, t = case_input('sub_wave', 'indep', False)
    x, tt = s.to(DEV), t.to(DEV)
    m = tssa.DistillationLoss()
    assert (m.temperature, m.kind) == (1.0, 'pixel')
    assert torch.equal(m(x, tt), tssa.distillation_loss(x, tt))
    assert torch.equal(tssa.DistillationLoss(4.0, 'channel')(x, tt), tssa.distillation_loss(x, tt, 4.0, 'channel'))
    assert torch.equal(ops.DistillFn.apply(ops.to_nhwc(x), ops.to_nhwc(tt), 4.0, 'channel'), tssa.distillation_loss(x, tt, 4.0, 'channel'))
    for bad in (lambda: tssa.distillation_loss(x, tt[:, :18]), lambda: tssa.distillation_loss(x, tt[:, :, :4]),
                lambda: tssa.distillation_loss(torch.zeros(1, 257, 2, 2, device=DEV), torch.zeros(1, 257, 2, 2, device=DEV)),
                lambda: tssa.distillation_loss(x, tt, 0.0), lambda: tssa.distillation_loss(x, tt, -1.0),
                lambda: tssa.distillation_loss(x, tt, float('nan')), lambda: tssa.distillation_loss(x, tt, 1.0, 'plane'),
                lambda: tssa.DistillationLoss(kind='feature'), lambda: tssa.DistillationLoss(temperature=0)):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: tssa.distillation_loss(x, tt.bfloat16()), lambda: tssa.distillation_loss(x.double(), tt.double()),
                lambda: tssa.distillation_loss(x.half(), tt.half())):
        with pytest.raises(TypeError):
            bad()
    for bad in (lambda: tssa.distillation_loss(s, t), lambda: tssa.distillation_loss(x, t), lambda: tssa.distillation_loss(s, tt)):
        with pytest.raises(RuntimeError):
            bad()
    # the C side refuses what is outside its contract with TSS_ERR_SHAPE (-2) / TSS_ERR_DTYPE (-1) before it launches anything
    lib, ptr, st = ops.N.lib(), ops.N.ptr, ops.N.stream()
    xn, tn = ops.to_nhwc(x), ops.to_nhwc(tt)
    B, C, h, w = xn.shape
    stats, ws, loss = torch.empty(B * h * w, 4, device=DEV), torch.empty(4096, dtype=torch.uint8, device=DEV), torch.empty((), device=DEV)
    for fwd in (lib.tss_distill_pixel_fwd, lib.tss_distill_channel_fwd):
        def rc(ldx=24, ldt=24, c=C, hw=h * w, tau=1.0, cap=0, dtype=0):
            return fwd(ptr(xn), ldx, ptr(tn), ldt, ptr(stats), ptr(ws), ptr(loss), B, c, hw, tau, cap, dtype, st)
        assert rc() == 0
        assert rc(c=257) == -2 and rc(c=0) == -2 and rc(hw=0) == -2 and rc(tau=0.0) == -2 and rc(tau=-2.0) == -2 and rc(cap=-1) == -2
        assert rc(ldx=20) == -2 and rc(ldt=16) == -2 and rc(dtype=2) == -1
    for bwd in (lib.tss_distill_pixel_bwd, lib.tss_distill_channel_bwd):
        d = torch.empty(B, h, w, 24, device=DEV)
        assert bwd(ptr(xn), 24, ptr(tn), 24, ptr(stats), None, ptr(d), 16, B, C, h * w, 1.0, 0, 0, st) == -2
        assert bwd(ptr(xn), 24, ptr(tn), 24, ptr(stats), None, ptr(d), 24, B, C, h * w, 0.0, 0, 0, st) == -2
    torch.cuda.synchronize()
    assert lib.tss_distill_workspace_bytes(0, B, 257, h * w, 0) == 0 and lib.tss_distill_workspace_bytes(2, B, C, h * w, 0) == 0
    assert lib.tss_distill_workspace_bytes(1, B, 256, h * w, 0) > 0 and lib.tss_distill_workspace_bytes(1, 0, C, h * w, 0) == 0
