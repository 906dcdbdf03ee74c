"""GPU parity, block level: every block type of SURVEY.md §8a rows A-H / K-P, forward + dX + dW (+ BN running
statistics), HIP path (through the C ABI) vs golden vectors generated from the reference itself.
f32 activations; tolerance = the north-star's 1e-3 relative (whole-tensor max norm), with an absolute floor
for gradients that are analytically zero (e.g. the bias of a BatchNorm that feeds another BatchNorm)."""
import math
import os

import numpy as np
import pytest
import torch

from oracle.recipe import formula_state
from tests import cases

pytestmark = pytest.mark.gpu

REL = 1e-3
ABS_FLOOR = 2e-4     # gradients here are sums of O(10^2..10^3) O(1) terms: f32 summation noise of an exact 0
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def golden(golden_dir):
    return {m: cases.load_npz(os.path.join(golden_dir, 'blocks_%s.npz' % m)) for m in ('train', 'eval')}


def close(a, b, rel=REL, floor=ABS_FLOOR):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() <= rel * np.abs(b).max() + floor


def run_block(name, mode, dtype=torch.float32):
    import torch_semantic_segmentation_amd as tssa
    m = cases.product_block(name)
    m.load_state_dict(formula_state(m), strict=True)
    cases.zero_dropout(m)
    m.train(mode == 'train')
    m.to(DEV)
    tssa.set_compute_dtype(m, dtype)
    xs = []
    for x in cases.block_inputs(name):
        is_act = x.shape[1] % 8 == 0
        x = x.to(DEV).to(dtype if is_act else torch.float32)
        xs.append(x.requires_grad_(is_act))
    out = m(*xs)
    out.backward(cases.block_cotangent(out.shape).to(DEV).to(out.dtype))
    torch.cuda.synchronize()
    return m, xs, out


@pytest.mark.parametrize('mode', ['eval', 'train'])
@pytest.mark.parametrize('name', sorted(cases.BLOCK_SHAPES))
def test_block_matches_reference(golden, name, mode):
    g = golden[mode]
    m, xs, out = run_block(name, mode)
    assert tuple(out.shape) == g[name + '/out'].shape
    assert close(out.detach().cpu().numpy(), g[name + '/out']), 'forward'
    for i, x in enumerate(xs):
        if x.grad is not None:
            assert close(x.grad.cpu().numpy(), g['%s/dx%d' % (name, i)]), 'dx%d' % i
    for pname, p in m.named_parameters():
        assert p.grad is not None, pname
        # the 2-sample BatchNorm of the 1x1 pyramid bin is ill-conditioned (xhat = +-1): looser
        rel = 5e-3 if ('pyramids.0' in pname and mode == 'train') else REL
        assert close(p.grad.cpu().numpy(), g['%s/dw.%s' % (name, pname)], rel=rel), pname
    if mode == 'train':
        for bname, b in m.named_buffers():
            if bname.endswith(('running_mean', 'running_var')):
                assert close(b.cpu().numpy(), g['%s/buf.%s' % (name, bname)], floor=1e-6), bname
            if bname.endswith('num_batches_tracked'):
                assert int(b) == 1


@pytest.mark.parametrize('name', ['fast_dw_s1', 'fast_dw_s2', 'fast_dw_d4', 'fast_ds_s1', 'fast_bneck_res', 'fast_bneck_s2',
                                  'ctx_dense3x3', 'fast_pw_act'])
def test_block_matches_cpu_oracle_at_a_size_with_many_tiles_per_block(name):
    """The golden fixtures are 8 x 16 maps: one tile per block everywhere.  Same blocks, same closed-form weights, at
    4 x C x 96 x 160 (persistent blocks sweep several tiles, ragged last tiles, several slab rows per block) against the CPU
    oracle run here: forward, dX, dW within the north-star's 1e-3 (train mode, f32)."""
    import torch_semantic_segmentation_amd as tssa
    from oracle.recipe import lattice_input
    C = cases.BLOCK_SHAPES[name][0][1]
    shape = (4, C, 96, 160)
    x0 = lattice_input(*shape)
    ref = cases.oracle_block(name)
    ref.load_state_dict(formula_state(ref), strict=True)
    cases.zero_dropout(ref)
    ref.train()
    xr = x0.clone().requires_grad_(True)
    outr = ref(xr)
    cot = cases.block_cotangent(outr.shape)
    outr.backward(cot)
    m = cases.product_block(name)
    m.load_state_dict(formula_state(m), strict=True)
    cases.zero_dropout(m)
    m.train().to(DEV)
    tssa.set_compute_dtype(m, torch.float32)
    x = x0.clone().to(DEV).requires_grad_(True)
    out = m(x)
    out.backward(cot.to(DEV))
    assert close(out.detach().cpu().numpy(), outr.detach().numpy()), 'forward'
    assert close(x.grad.cpu().numpy(), xr.grad.numpy(), floor=5e-4), 'dx'
    for (pn, p), (rn, r) in zip(m.named_parameters(), ref.named_parameters()):
        assert p.shape == r.shape, (pn, rn)
        # sums over 61 k pixels in f32; a BatchNorm bias that feeds another BatchNorm has an analytically zero gradient
        # whose computed value is summation noise of that size on BOTH sides (the CPU's is the larger one)
        assert close(p.grad.cpu().numpy(), r.grad.numpy(), rel=2e-3, floor=3e-2), pn


@pytest.mark.parametrize('name', ['fast_bneck_res', 'fast_ds_s2', 'fast_fusion', 'ctx_classifier', 'fast_stem',
                                  'ctx_dense3x3', 'fast_ppm'])
def test_block_bf16_tracks_f32(golden, name):
    """bf16 activations against the reference's f32 golden vectors.  The operands of this fixture are NOT bf16-representable
    (closed-form f32 weights and inputs), so the error includes the rounding of inputs and weights; the bound is therefore
    the yardstick rule of tests/test_gpu_lean_vs_oracle.py -- the lean kernels may be at most 2x as far from the reference
    as the general bf16 kernels on the same case -- under absolute caps (forward 4.5e-2, weight gradients 0.3 relative L2: 8 x 16 maps,
    flipped ReLU masks; the tight pin of the bf16 kernels is tests/test_gpu_lean_vs_oracle.py)."""
    from torch_semantic_segmentation_amd import _native as N
    g = golden['train']

    def l2(a, b):
        a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
        return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12)

    def run(disable):
        N.call('tss_set_option', 1, int(disable))
        try:
            m, xs, out = run_block(name, 'train', torch.bfloat16)
        finally:
            N.call('tss_set_option', 1, 0)
        assert out.dtype == torch.bfloat16
        errs = {'out': l2(out.detach().float().cpu().numpy(), g[name + '/out'])}
        for pname, p in m.named_parameters():
            ref = g['%s/dw.%s' % (name, pname)]
            if p.dim() == 4 and np.linalg.norm(ref) > 1e-2:
                errs[pname] = l2(p.grad.cpu().numpy(), ref)
        return errs
    lean, general = run(False), run(True)
    print(name, {k: ('%.2e' % lean[k], '%.2e' % general[k]) for k in lean})
    for k in lean:
        cap = 4.5e-2 if k == 'out' else 0.3
        assert lean[k] <= min(2 * general[k] + 2e-3, cap), (k, lean[k], general[k])


@pytest.mark.parametrize('name', ['fast_pw_act', 'fast_pw_noact', 'fast_bneck_res', 'fast_bneck_s2', 'fast_ds_s2',
                                  'fast_fusion', 'ctx_pw', 'fast_stem', 'fast_classifier', 'ctx_dense3x3'])
def test_bf16_lean_kernels_agree_with_general_kernels(name):
    """The performance path has lean bf16 kernels (pwfast.hip, stem.hip) next to the general ones that the f32 parity
    tests exercise.  Same bf16 inputs through both: they may differ only by bf16 rounding of intermediates."""
    from torch_semantic_segmentation_amd import _native as N

    def run(disable):
        N.call('tss_set_option', 1, int(disable))
        try:
            m, xs, out = run_block(name, 'train', torch.bfloat16)
        finally:
            N.call('tss_set_option', 1, 0)
        grads = {k: p.grad.detach().float().cpu().numpy() for k, p in m.named_parameters()}
        dx = [x.grad.detach().float().cpu().numpy() for x in xs if x.grad is not None]
        return out.detach().float().cpu().numpy(), dx, grads

    def l2(a, b):
        return np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-12)
    o1, dx1, g1 = run(False)
    o0, dx0, g0 = run(True)
    assert l2(o1, o0) < 1.5e-2
    for a, b in zip(dx1, dx0):
        assert l2(a, b) < 5e-2
    for k in g0:
        if g0[k].ndim == 4 and np.linalg.norm(g0[k]) > 1e-2:
            assert l2(g1[k], g0[k]) < 8e-2, k


@pytest.mark.parametrize('cin,cout,h,w', [(128, 128, 6, 70), (64, 16, 5, 7), (32, 64, 4, 64), (128, 128, 3, 130)])
def test_dense3x3_lean_kernel_agrees_with_general_kernel(cin, cout, h, w):
    """conv3x3.hip (LDS halo tile, nine shifted views, double-buffered bf16 taps) against convgemm's tap loop on the same
    bf16 operands: ConvBlock(k=3) between two 1x1 blocks, so the deferred-BatchNorm prologue, the zero padding of the
    ACTIVATED tensor, the backward ReLU mask and both statistics paths are exercised; ragged and multi-tile rows."""
    import importlib
    from torch import nn
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import _native as N
    C = importlib.import_module('torch_semantic_segmentation_amd.models.contextnet')

    def run(disable):
        torch.manual_seed(11)
        m = nn.Sequential(C.ConvBlock(cin, cin, 1), C.ConvBlock(cin, cout, 3, padding=1), C.ConvBlock(cout, cout, 1)).to(DEV)
        tssa.set_compute_dtype(m, torch.bfloat16)
        m.train()
        x = torch.randn(2, cin, h, w, device=DEV).requires_grad_(True)
        cot = torch.randn(2, cout, h, w, device=DEV)
        N.call('tss_set_option', 1, int(disable))
        try:
            out = m(x)
            out.float().backward(cot)
        finally:
            N.call('tss_set_option', 1, 0)
        return (out.detach().float().cpu().numpy(), x.grad.float().cpu().numpy(),
                {k: p.grad.float().cpu().numpy() for k, p in m.named_parameters()},
                {k: b.detach().float().cpu().numpy() for k, b in m.named_buffers() if b.dtype.is_floating_point})

    def l2(a, b):
        return np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-12)
    o1, dx1, g1, b1 = run(False)
    o0, dx0, g0, b0 = run(True)
    assert l2(o1, o0) < 1.5e-2
    assert l2(dx1, dx0) < 5e-2
    for k in g0:
        if np.linalg.norm(g0[k]) > 1e-2:
            assert l2(g1[k], g0[k]) < 8e-2, k
    for k in b0:      # running statistics come from the lean kernels' slab rows
        assert l2(b1[k], b0[k]) < 1e-2, k


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('shape', [(2, 64, 16, 32), (3, 128, 12, 20)])
def test_pyramid_pooling_all_arms_per_launch_matches_per_arm_operators(dtype, shape):
    """tss_ppm_{pool,concat}_{fwd,bwd} (every arm of the PyramidPoolingModule per launch, BatchNorm + ReLU applied per
    bilinear tap, slab rows written by the gather) against the generic per-arm operators on the same operands."""
    import importlib
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    F_ = importlib.import_module('torch_semantic_segmentation_amd.models.fastscnn')
    B, C, H, W = shape

    def run(fused):
        torch.manual_seed(13)
        m = F_.PyramidPoolingModule(C, C).to(DEV)
        tssa.set_compute_dtype(m, dtype)
        m.train()
        x = torch.randn(B, C, H, W, device=DEV).requires_grad_(True)
        cot = torch.randn(B, C, H, W, device=DEV)
        old = ops.ppm_fused
        ops.ppm_fused = fused
        try:
            out = m(x.to(dtype) if dtype != torch.float32 else x)
            out.float().backward(cot)
        finally:
            ops.ppm_fused = old
        return (out.detach().float().cpu(), x.grad.float().cpu(), {k: p.grad.float().cpu() for k, p in m.named_parameters()},
                {k: b.detach().float().cpu() for k, b in m.named_buffers() if b.dtype.is_floating_point})
    o1, dx1, g1, b1 = run(True)
    o0, dx0, g0, b0 = run(False)
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    assert cases.rel_err(o1, o0) < tol and cases.rel_err(dx1, dx0) < 4 * tol
    for k in g0:
        if g0[k].norm() > 1e-3:
            assert cases.rel_err(g1[k], g0[k]) < 5 * tol, k
    for k in b0:
        assert cases.rel_err(b1[k], b0[k]) < tol, k


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_dropout_folded_into_the_join_is_bit_identical_to_its_own_pass(dtype):
    """Classifier tail (... -> BN -> ReLU -> Dropout -> Conv2d, TSS/models/fastscnn.py:92-98): the join that materialises
    the activation applies the dropout mask itself (same Philox counters as tss_dropout); backward only rescales, because
    out > 0 <=> kept and active.  Same seed, same bits as the separate dropout pass, forward and backward."""
    import importlib
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    F_ = importlib.import_module('torch_semantic_segmentation_amd.models.fastscnn')

    def run(fused):
        torch.manual_seed(17)
        ops._dropout_counters.clear()            # the device-side Philox counter restarts from torch.initial_seed()
        m = F_.Classifier(32, 19).to(DEV)
        m[2].p = 0.3
        tssa.set_compute_dtype(m, dtype)
        m.train()
        x = torch.randn(2, 32, 8, 24, device=DEV).requires_grad_(True)
        old, old_conv = ops.fuse_dropout, ops.fuse_dropout_conv
        ops.fuse_dropout, ops.fuse_dropout_conv = fused, False      # (the convolution-side fold has its own test below)
        try:
            out = m(x.to(dtype) if dtype != torch.float32 else x)
            out.float().backward(torch.ones_like(out, dtype=torch.float32))
        finally:
            ops.fuse_dropout, ops.fuse_dropout_conv = old, old_conv
        return out.detach().float(), x.grad.float(), [p.grad.float().clone() for p in m.parameters()]
    o1, dx1, g1 = run(True)
    o0, dx0, g0 = run(False)
    assert torch.equal(o1, o0) and torch.equal(dx1, dx0)
    for a, b in zip(g1, g0):
        assert cases.rel_err(a.cpu(), b.cpu()) < 1e-5      # weight-gradient sums may differ in order only
    # the mask is real: about 30 % of the (positive) activations feeding the last conv were dropped
    assert (o1 != 0).any()


@pytest.mark.parametrize('cin,classes,shape', [(128, 19, (2, 24, 40)), (32, 19, (2, 8, 24)), (64, 21, (3, 17, 9)), (128, 8, (1, 70, 33))])
@pytest.mark.parametrize('pending', [True, False])
def test_dropout_applied_on_load_by_the_classifier_conv(cin, classes, shape, pending):
    """Classifier tail (... -> BN -> ReLU -> Dropout -> Conv2d(., classes, 1), TSS/models/fastscnn.py:96-97) with the dropout applied
    on load by the convolution (tss_dropout_mask + tss_pwconv_fwd_drop + tss_pwconv_bwd_fused_drop): no pass over the activation.
    Checked against the same layers with the SAME mask (drawn again through the C ABI from the same counter) applied by torch
    to the materialised activation: output, input gradient, every parameter gradient; the mask keeps 1 - p of the elements, changes
    from step to step and repeats from the same seed."""
    import importlib
    from torch import nn
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import _native as N, ops
    F_ = importlib.import_module('torch_semantic_segmentation_amd.models.fastscnn')
    B, H, W = shape
    p_drop = 0.3

    def build():
        torch.manual_seed(41)
        head = [F_.Conv2dBlock(cin, cin, 1)] if pending else []
        m = F_.FusedSequential(*head, nn.Dropout(p_drop), nn.Conv2d(cin, classes, 1)).to(DEV)
        tssa.set_compute_dtype(m, torch.bfloat16)
        return m.train()

    def inputs():
        torch.manual_seed(43)
        x = torch.randn(B, cin, H, W, device=DEV)
        if not pending:
            x = x.relu()
        return ops.to_nhwc(x.to(torch.bfloat16)).requires_grad_(True), torch.randn(B, classes, H, W, device=DEV)

    def grads(m, x):
        return [x.grad.float().clone()] + [q.grad.float().clone() for q in m.parameters()]

    # (1) the fold
    ops._dropout_counters.clear()
    m = build()
    x, cot = inputs()
    seed = int(ops._dropout_counter(x.device).item())
    out = m(x)
    assert int(ops._dropout_counter(x.device).item()) == seed + 1          # the consumer advanced the counter
    out.float().backward(cot)
    o1, g1 = out.detach().float(), grads(m, x)
    out2 = m(inputs()[0]).detach().float()
    assert not torch.equal(out2, o1)                                         # next step, next mask
    ops._dropout_counters.clear()
    m_again = build()
    assert torch.equal(m_again(inputs()[0]).detach().float(), o1)            # same seed, same bits

    # (2) the same mask, applied by torch to the materialised activation
    P = B * H * W
    counter = torch.tensor([seed], dtype=torch.int64, device=DEV)
    mask = torch.empty((P, 16), dtype=torch.uint8, device=DEV)
    N.call('tss_dropout_mask', N.ptr(counter), N.ptr(mask), P, cin, p_drop, N.stream())
    torch.cuda.synchronize()
    bits = (mask[:, :cin // 8].reshape(P, cin // 8, 1) >> torch.arange(8, device=DEV, dtype=torch.uint8).view(1, 1, 8)) & 1
    keep = bits.view(B, H, W, cin).permute(0, 3, 1, 2).float()
    frac = keep.mean().item()
    assert abs(frac - (1 - p_drop)) < 4 * math.sqrt(p_drop * (1 - p_drop) / keep.numel()) + 1e-4
    m0 = build()
    x0, _ = inputs()
    a = ops.materialize(F_.run(m0[0], x0)) if pending else x0
    a_drop = ((a.float() * keep) * (1.0 / (1.0 - p_drop))).to(torch.bfloat16)
    out0 = ops.materialize(ops.conv_unit(ops.to_nhwc(a_drop), m0[-1]))
    out0.float().backward(cot)
    o0, g0 = out0.detach().float(), grads(m0, x0)
    assert cases.rel_err(o1.cpu(), o0.cpu()) < 1e-2
    for a1, a0 in zip(g1, g0):
        if a0.norm() > 1e-3:
            assert cases.rel_err(a1.cpu(), a0.cpu()) < 2e-2


@pytest.mark.parametrize('name', ['fast_bneck_res', 'fast_bneck_s2', 'fast_ds_s2', 'fast_dw_d4', 'fast_dw_s1'])
def test_bf16_lean_kernels_agree_with_general_kernels_at_many_tiles_per_block(name):
    """As test_bf16_lean_kernels_agree_with_general_kernels, at 4 x C x 96 x 160: the persistent loops of the lean kernels
    (cross-tile prefetch, several tiles and slab rows per block, 256-pixel weight-gradient splits) against the general ones."""
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import _native as N
    from oracle.recipe import lattice_input
    C = cases.BLOCK_SHAPES[name][0][1]
    x0 = lattice_input(4, C, 96, 160)

    def run(disable):
        m = cases.product_block(name)
        m.load_state_dict(formula_state(m), strict=True)
        cases.zero_dropout(m)
        m.train().to(DEV)
        tssa.set_compute_dtype(m, torch.bfloat16)
        x = x0.clone().to(DEV).to(torch.bfloat16).requires_grad_(True)
        N.call('tss_set_option', 1, int(disable))
        try:
            out = m(x)
            out.backward(cases.block_cotangent(out.shape).to(DEV).to(out.dtype))
            torch.cuda.synchronize()
        finally:
            N.call('tss_set_option', 1, 0)
        return (out.detach().float().cpu().numpy(), x.grad.float().cpu().numpy(),
                {k: p.grad.float().cpu().numpy() for k, p in m.named_parameters()})

    def l2(a, b):
        return np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-12)
    o1, dx1, g1 = run(False)
    o0, dx0, g0 = run(True)
    assert l2(o1, o0) < 1.5e-2 and l2(dx1, dx0) < 5e-2
    for k in g0:
        if g0[k].ndim == 4 and np.linalg.norm(g0[k]) > 1e-2:
            assert l2(g1[k], g0[k]) < 8e-2, k


def test_cpu_tensors_raise():
    m = cases.product_block('fast_pw_act')
    with pytest.raises(RuntimeError, match='HIP path only'):
        m(torch.zeros(2, 48, 8, 16))


def test_hooks_fire_with_materialized_tensors():
    """DeepSupervisionWrapper pattern (TSS/wrappers/deep_supervision_wrapper.py:23-43): hooks on containers."""
    m = cases.product_model('fastscnn').to(DEV).eval()
    seen = {}
    h1 = m.downsample.register_forward_hook(lambda mod, i, o: seen.__setitem__('down', o))
    h2 = m.features.register_forward_hook(lambda mod, i, o: seen.__setitem__('feat', o))
    h3 = m.features[0][1].conv1.register_forward_hook(lambda mod, i, o: seen.__setitem__('inner', o))
    with torch.no_grad():
        y = m(torch.randn(2, 3, 64, 128, device=DEV))
    for h in (h1, h2, h3):
        h.remove()
    assert tuple(seen['down'].shape) == (2, 64, 8, 16) and tuple(seen['feat'].shape) == (2, 128, 2, 4)
    assert tuple(seen['inner'].shape) == (2, 384, 4, 8) and isinstance(seen['inner'], torch.Tensor)
    assert tuple(y.shape) == (2, 19, 64, 128)
    h = m.downsample[0][0].register_full_backward_hook(lambda *a: None)     # backward hooks on fused leaves: refused, loudly
    with pytest.raises(NotImplementedError):
        m(torch.randn(2, 3, 64, 128, device=DEV))
    h.remove()


def test_leaf_hooks_see_what_the_reference_leaves_produce():
    """SURVEY.md section 8b item (3) for LEAVES (VERDICT r01 missing #4): a forward hook on a Conv2d / BatchNorm2d / ReLU inside
    a fused unit -- the CaptureOutput pattern, TSS/nn/utils.py:7-32 -- fires with the tensor the reference's leaf returns:
    raw conv output, normalised output, activated output.  Checked against the oracle (same weights, same hooks), train
    mode, and the model output is unchanged by the presence of the hooks."""
    from oracle.recipe import lattice_input
    ref = O_build_pair()
    m = cases.product_model('fastscnn')
    m.load_state_dict(ref.state_dict(), strict=True)
    cases.zero_dropout(m); cases.zero_dropout(ref)
    m.to(DEV).train(); ref.train()
    x = lattice_input(2, 3, 64, 128)
    paths = ['downsample.0.0', 'downsample.0.1', 'downsample.0.2', 'features.0.1.conv1.0', 'features.0.1.conv2.1',
             'classifier.0.3', 'classifier.3']
    got, want = {}, {}
    hs = [m.get_submodule(p).register_forward_hook(lambda mod, i, o, p=p: got.__setitem__(p, o.detach().float().cpu())) for p in paths]
    hr = [ref.get_submodule(p).register_forward_hook(lambda mod, i, o, p=p: want.__setitem__(p, o.detach().clone())) for p in paths]
    pre = {}
    hs.append(m.get_submodule('features.0.1.conv2.0').register_forward_pre_hook(lambda mod, i: pre.__setitem__('in', i[0].detach().float().cpu())))
    hr.append(ref.get_submodule('features.0.1.conv2.0').register_forward_pre_hook(lambda mod, i: pre.__setitem__('ref', i[0].detach().clone())))
    out_h = m(x.to(DEV))
    out_r = ref(x)
    for h in hs + hr:
        h.remove()
    assert set(got) == set(paths)
    for p in paths:
        assert tuple(got[p].shape) == tuple(want[p].shape), p
        assert cases.rel_err(got[p].numpy(), want[p].numpy()) < 1e-3, p
    assert cases.rel_err(pre['in'].numpy(), pre['ref'].numpy()) < 1e-3
    assert cases.rel_err(out_h.detach().cpu().numpy(), out_r.detach().numpy()) < 1e-3
    torch.manual_seed(0)
    m2 = cases.product_model('fastscnn')
    m2.load_state_dict({k: v for k, v in ref.state_dict().items()}, strict=False)
    # a hook that tries to REPLACE a fused leaf's output is refused
    h = m.downsample[0][1].register_forward_hook(lambda mod, i, o: o * 2)
    with pytest.raises(NotImplementedError):
        m(x.to(DEV))
    h.remove()


def O_build_pair():
    from oracle import nets as O
    torch.manual_seed(0)
    return O.build('fastscnn')


@pytest.mark.parametrize('name,dtype', [('contextnet14', torch.float16), ('fastscnn', torch.bfloat16), ('fastscnn', torch.float16)])
def test_half_model_runs_and_tracks_f32(name, dtype):
    """`model.to(device).to(dtype)` + a 16-bit batch, as TSS scripts/contextnet/benchmark_contextnet.py:40,62 does it: logits come
    back in that dtype, equal to the f32 model's within bf16 noise; training-mode forward/backward fills 16-bit .grad."""
    torch.manual_seed(0)
    m = cases.product_model(name).to(DEV)
    cases.zero_dropout(m)
    x = torch.randn(2, 3, 64, 128, device=DEV)
    m.eval()
    with torch.no_grad():
        want = m(x)
        m.to(dtype)
        got = m(x.to(dtype))
    assert got.dtype == dtype and tuple(got.shape) == tuple(want.shape)
    err = ((got.float() - want).norm() / want.norm()).item()
    assert err < 5e-2, err
    m.train()
    out = m(x.to(dtype))
    out.float().square().mean().backward()
    assert all(p.grad is not None and p.grad.dtype == dtype and torch.isfinite(p.grad.float()).all() for p in m.parameters())
    assert all(b.dtype == dtype for k, b in m.named_buffers() if k.endswith('running_mean'))
    m.float()
    with torch.no_grad():
        assert m(x).dtype == torch.float32


def test_residual_fan_in_folded_into_the_first_layers_backward_matches_autograds_add():
    """The block input of a residual bottleneck has two consumers; ops.residual_fork hands the skip's gradient to the epilogue of
    conv1's backward-data kernel (tss_pwconv_bwd_data_radd) instead of letting autograd add the two tensors with a launch of its
    own.  Same gradients as the unfolded graph (TSS_FOLD_RESIDUAL=0), up to one bf16 rounding of the sum.  The folded run launches an
    entry point that takes the skip's gradient, and nothing is left behind: a fork of the forward dies with the tensors and the graph."""
    import gc
    import importlib
    import weakref
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    F_ = importlib.import_module('torch_semantic_segmentation_amd.models.fastscnn')
    # the entry points with a residual operand: ops._bwd_pw_sweep (radd_s) and the two folded branches of ops._pw_data_grad (radd)
    takes_residual = {'tss_pwconv_bwd_sweep', 'tss_pwconv_bwd_data_joined', 'tss_pwconv_bwd_data_radd'}
    sequences = []

    def run(fold):
        torch.manual_seed(37)
        m = F_.BottleneckModule(32, 32, expansion=6, repeats=3, stride=1).to(DEV)
        tssa.set_compute_dtype(m, torch.bfloat16)
        m.train()
        x = torch.randn(2, 32, 24, 40, device=DEV).to(torch.bfloat16).requires_grad_(True)     # (a float32 input folds nothing)
        old, orig_fork, orig_call = ops.fold_residual_adds, ops.residual_fork, ops.call
        forks, names = [], []

        def fork_spy(t):
            r = orig_fork(t)
            if r[2] is not None:
                forks.append(weakref.ref(r[2]))
            return r

        def call_spy(name, *a):
            names.append(name)
            return orig_call(name, *a)
        ops.fold_residual_adds, ops.residual_fork, ops.call = fold, fork_spy, call_spy
        try:
            out = ops.materialize(m(x))
            out.float().backward(torch.randn_like(out, dtype=torch.float32))
        finally:
            ops.fold_residual_adds, ops.residual_fork, ops.call = old, orig_fork, orig_call
        res = out.detach().float(), x.grad.float(), {k: p.grad.float() for k, p in m.named_parameters()}
        assert len(forks) == (3 if fold else 0)
        if fold:
            assert takes_residual & set(names), names
        # ... of which only tss_pwconv_bwd_data_radd never runs without a fork's gradient: the first block's input is a leaf (no join
        # in front of it), so its conv1 takes that branch of ops._pw_data_grad exactly when it took the fork off its input
        assert (names.count('tss_pwconv_bwd_data_radd') >= 1) == fold, names
        sequences.append(names)
        del out
        gc.collect()
        assert all(ref() is None for ref in forks)       # nothing outlives the pass (there is no registry to leave an entry in)
        return res
    o1, dx1, g1 = run(True)
    o0, dx0, g0 = run(False)
    assert torch.equal(o1, o0)
    assert sequences[0] != sequences[1]          # the fold changes what is launched: the autograd fallback alone would not
    l2 = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()
    assert l2(dx1, dx0) < 1e-2
    for k in g0:
        if g0[k].norm() > 1e-3:
            ref = g0[k]
            if k.endswith('conv1.1.weight'):
                # the gradient of conv1's BatchNorm weight is analytically zero: a per-channel scale passes the ReLU (beta = 0) and the
                # depthwise convolution and is removed by conv2's per-channel BatchNorm.  Both runs hold the rounding noise of
                # sum(e * xhat) there, so the difference is held against the scale of that sum's terms, the same layer's
                # sum(e) -- its bias gradient -- and not against the noise itself; and each run's own value, whose exact
                # counterpart is 0, is held to the same bound (a wrong e in the folded sum would show at that scale).
                ref = g0[k[:-len('weight')] + 'bias']
                assert max(g1[k].double().norm().item(), g0[k].double().norm().item()) < 2e-2 * ref.double().norm().item(), k
            assert (g1[k].double() - g0[k].double()).norm().item() < 2e-2 * ref.double().norm().item(), k


def _bf16_nhwc_leaf(*shape):
    from torch_semantic_segmentation_amd import ops
    return ops.to_nhwc(torch.randn(*shape, device=DEV).to(torch.bfloat16)).requires_grad_(True)


@pytest.mark.parametrize('maker', ['residual_fork', 'fork_two'])
def test_an_abandoned_fork_note_dies_with_its_tensor(maker):
    """A fork whose handles nobody consumes (a layer raised, a consumer outside the envelope) is gone when the handles are: the notes
    ride on the tensors, there is no table an entry could stay in.  A convolution unit on fresh tensors of the same shape (which may
    well get the ids of the dead ones) therefore finds no fork, no stash and no join."""
    import gc
    import importlib
    import weakref
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    F_ = importlib.import_module('torch_semantic_segmentation_amd.models.fastscnn')
    xa, xb, fork = getattr(ops, maker)(_bf16_nhwc_leaf(1, 8, 4, 8))
    assert fork is not None and xa is not xb
    ref = weakref.ref(fork)
    del xa, xb, fork
    gc.collect()
    assert ref() is None
    torch.manual_seed(71)
    block = F_.Conv2dBlock(8, 8, kernel_size=1).to(DEV)
    tssa.set_compute_dtype(block, torch.bfloat16)
    block.train()
    for _ in range(2):
        y = block.unit(_bf16_nhwc_leaf(1, 8, 4, 8))
        cfg = y.raw.grad_fn.cfg
        assert isinstance(cfg, ops.UnitCfg)
        assert cfg.res_fork is None and cfg.stash_fork is None and cfg.prev_join is None
    torch.cuda.synchronize()


@pytest.mark.parametrize('maker', ['residual_fork', 'fork_two'])
def test_a_note_never_references_the_tensor_that_carries_it(maker):
    """The rule stated at ops._hand: with the collector switched off, reference counting alone frees an abandoned fork together with
    its handles -- there is no cycle through a note."""
    import gc
    import weakref
    from torch_semantic_segmentation_amd import ops
    xa, xb, fork = getattr(ops, maker)(_bf16_nhwc_leaf(1, 8, 4, 8))
    assert fork is not None
    ref = weakref.ref(fork)
    gc.disable()
    try:
        del xa, xb, fork
        dead = ref() is None
    finally:
        gc.enable()
    assert dead


def test_a_join_note_is_single_use_and_keeps_nothing_alive(monkeypatch):
    """The output of a block's ReLU join carries the join's configuration for the next layer's backward-data epilogue: the first taker
    gets it, a second one gets nothing, and once the output and the taker's handle are dropped the configuration is gone."""
    import gc
    import importlib
    import weakref
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    F_ = importlib.import_module('torch_semantic_segmentation_amd.models.fastscnn')

    class WatchedJoinCfg(ops.JoinCfg):           # JoinCfg has __slots__ without __weakref__: this test alone needs to watch one die
        __slots__ = ('__weakref__',)
    monkeypatch.setattr(ops, 'JoinCfg', WatchedJoinCfg)
    torch.manual_seed(73)
    m = F_.BottleneckBlock(32, 32, expansion=6).to(DEV)
    tssa.set_compute_dtype(m, torch.bfloat16)
    m.train()
    h = m(_bf16_nhwc_leaf(2, 32, 8, 8))
    cfg = ops._take_join(h)
    assert isinstance(cfg, WatchedJoinCfg) and cfg.j_a is not None
    assert ops._take_join(h) is None
    ref = weakref.ref(cfg)
    del h, cfg
    gc.collect()
    assert ref() is None
    torch.cuda.synchronize()


@pytest.mark.parametrize('family,cin,cout,stride,shape', [('fastscnn', 64, 64, 1, (2, 24, 40)), ('fastscnn', 64, 96, 2, (2, 24, 40)),
                                                         ('fastscnn', 128, 128, 1, (1, 32, 64)), ('contextnet', 32, 32, 1, (3, 17, 9)),
                                                         ('contextnet', 48, 64, 2, (2, 16, 24))])
def test_eval_block_output_written_by_conv3_epilogue(family, cin, cout, stride, shape):
    """model.eval(), no gradient, bf16: BottleneckBlock's frozen BatchNorm, skip and ReLU run in the epilogue of conv3
    (tss_pwconv_fwd_joined) instead of a join pass.  Against the join form of the same block (TSS_EVAL_EPILOGUE=0 path) and against the
    block evaluated by torch in f32 on the same bf16 input (TSS/models/fastscnn.py:152-161, TSS/models/contextnet.py:139-147)."""
    import importlib
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    M = importlib.import_module('torch_semantic_segmentation_amd.models.' + family)
    torch.manual_seed(53)
    m = M.BottleneckBlock(cin, cout, stride=stride, expansion=6).to(DEV)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.3)
            mod.running_var.uniform_(0.5, 1.5)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.2)
    tssa.set_compute_dtype(m, torch.bfloat16)
    m.eval()
    B, H, W = shape
    x = torch.randn(B, cin, H, W, device=DEV).to(torch.bfloat16)
    calls = []
    orig = ops.conv_unit_joined

    def spy(*a, **k):
        r = orig(*a, **k)
        calls.append(r is not None)
        return r
    ops.conv_unit_joined = spy
    whole = ops.eval_bottleneck
    ops.eval_bottleneck = False          # (round 4: the whole block is one kernel where csrc/bneck.hip covers it; this is the path behind it)
    try:
        with torch.no_grad():
            y1 = m(x).float()
            old = ops.eval_epilogue
            ops.eval_epilogue = False
            try:
                y0 = m(x).float()
            finally:
                ops.eval_epilogue = old
    finally:
        ops.conv_unit_joined = orig
        ops.eval_bottleneck = whole
    assert calls == [True, False]
    # torch, f32, the reference's formula
    with torch.no_grad():
        c1, b1 = m.conv1[0], m.conv1[1]
        c2, b2 = m.conv2[0], m.conv2[1]
        c3, b3 = m.conv3[0], m.conv3[1]
        import torch.nn.functional as F
        t = F.relu(F.batch_norm(F.conv2d(x.float(), c1.weight), b1.running_mean, b1.running_var, b1.weight, b1.bias, False, 0.0, b1.eps))
        t = F.relu(F.batch_norm(F.conv2d(t, c2.weight, stride=stride, padding=1, groups=c2.groups), b2.running_mean, b2.running_var,
                                b2.weight, b2.bias, False, 0.0, b2.eps))
        t = F.batch_norm(F.conv2d(t, c3.weight), b3.running_mean, b3.running_var, b3.weight, b3.bias, False, 0.0, b3.eps)
        ref = F.relu(t + x.float()) if tuple(t.shape) == tuple(x.shape) else F.relu(t)
    assert cases.rel_err(y1.cpu(), y0.cpu()) < 2e-2
    e1 = ((y1 - ref).norm() / ref.norm()).item()
    e0 = ((y0 - ref).norm() / ref.norm()).item()
    assert e1 < 1e-2 and e1 < 1.2 * e0 + 1e-3, (e1, e0)       # (the epilogue form skips one bf16 rounding of the conv output)


@pytest.mark.parametrize('family', ['fastscnn', 'contextnet'])
@pytest.mark.parametrize('extra_consumer', [False, True])
def test_join_backward_rides_in_the_next_layers_backward_data_launch(family, extra_consumer):
    """Three bottleneck blocks in a row (bf16, training): the backward of a block output's join -- ReLU mask + BatchNorm-backward sums --
    runs in the epilogue of the next block's first backward-data launch (tss_pwconv_bwd_data_joined) instead of tss_join_bwd.  Same
    gradients as with the fusion switched off; and when the block output has ANOTHER consumer (deep supervision: a hook feeds it to an
    auxiliary head), autograd hands the join a summed gradient and its own kernel runs on it -- the fallback is exact."""
    import importlib
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    M = importlib.import_module('torch_semantic_segmentation_amd.models.' + family)
    counts = {}

    def run(fused):
        torch.manual_seed(61)
        blocks = [M.BottleneckBlock(32, 48, stride=2, expansion=6), M.BottleneckBlock(48, 48, expansion=6),
                  M.BottleneckBlock(48, 48, expansion=6)]
        m = torch.nn.Sequential(*blocks).to(DEV)
        tssa.set_compute_dtype(m, torch.bfloat16)
        m.train()
        x = ops.to_nhwc(torch.randn(3, 32, 40, 56, device=DEV).to(torch.bfloat16)).requires_grad_(True)
        old, orig = ops.fuse_join_backward, ops.call
        names = []

        def spy(name, *a):
            names.append(name)
            return orig(name, *a)
        ops.fuse_join_backward, ops.call = fused, spy
        try:
            h = x
            aux = 0.0
            for i, blk in enumerate(m):
                h = blk(h)
                if extra_consumer and i == 0:
                    aux = h.float().mean() * 3.0           # a second consumer of the first block's output
            torch.manual_seed(67)
            ((h.float() * torch.randn_like(h, dtype=torch.float32)).sum() + aux).backward()
            torch.cuda.synchronize()
        finally:
            ops.fuse_join_backward, ops.call = old, orig
        counts[fused] = (names.count('tss_join_bwd'), names.count('tss_pwconv_bwd_data_joined'))
        return x.grad.float(), {k: p.grad.float() for k, p in m.named_parameters()}
    dx1, g1 = run(True)
    dx0, g0 = run(False)
    assert counts[False] == (3, 0)
    # blocks 0 and 1 feed an expand convolution; the last block's output feeds the loss
    assert counts[True] == ((2, 2) if extra_consumer else (1, 2)), counts
    def l2(a, b):
        return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()
    assert l2(dx1, dx0) < 5e-3
    for k in g0:
        if g0[k].norm() > 1e-3:
            assert l2(g1[k], g0[k]) < 5e-3, k



# ----------------------------------------------------------------------------- re-entrant backward passes (round 4)

def _fast_features(seed=41):
    import importlib
    import torch_semantic_segmentation_amd as tssa
    F_ = importlib.import_module('torch_semantic_segmentation_amd.models.fastscnn')
    torch.manual_seed(seed)
    m = torch.nn.Sequential(F_.Conv2dBlock(32, 32, 1), F_.BottleneckBlock(32, 32), F_.BottleneckBlock(32, 32),
                            F_.DSConv2dBlock(32, 48, kernel_size=3, padding=1)).to(DEV)
    m.train()
    return m


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _same(a, b):
    """equal to 1e-6 of the tensor's norm (the f32 parity path sums some weight gradients with f32 atomics: order noise ~1e-7);
    analytically-zero gradients (a BatchNorm bias in front of a linear conv + BatchNorm) are rounding noise on both sides"""
    a, b = a.double(), b.double()
    return bool((a - b).norm() <= 1e-6 * max(float(b.norm()), 1.0))


def _run_plain(m, x, cot, direct=True):
    from torch_semantic_segmentation_amd import ops
    for p in m.parameters():
        p.grad = torch.zeros_like(p) if direct else None
    xx = x.clone().requires_grad_(True)
    with ops.direct_grads(direct):
        out = ops.materialize(m(xx))
        out.backward(cot)
    torch.cuda.synchronize()
    return out.detach().clone(), xx.grad.detach().clone(), _grads(m)


def test_checkpointed_block_keeps_the_outer_passes_postponed_work():
    """One BottleneckBlock under torch.utils.checkpoint(use_reentrant=True): its recomputation runs a NESTED backward pass inside the
    outer one.  The postponed weight gradients / row reductions of the outer pass used to be deleted when the graph-task id changed
    (ops._backward_task); now every pass owns its state.  All gradients equal the plain run (f32 path: to 1e-6)."""
    from torch.utils.checkpoint import checkpoint
    from torch_semantic_segmentation_amd import ops
    m = _fast_features()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 32, 24, 40, generator=g).to(DEV)
    cot = torch.randn(2, 48, 24, 40, generator=g).to(DEV)
    out0, dx0, g0 = _run_plain(m, x, cot)

    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    xx = x.clone().requires_grad_(True)
    with ops.direct_grads(True):
        h = ops.materialize(m[0](xx))
        h = checkpoint(lambda t: ops.materialize(m[1](t)), h, use_reentrant=True)
        out = ops.materialize(m[3](m[2](h)))
        out.backward(cot)
    torch.cuda.synchronize()
    assert not ops._passes
    g1 = _grads(m)
    assert _same(out, out0)
    assert _same(xx.grad, dx0)
    for k in g0:
        assert _same(g1[k], g0[k]), k


def test_autograd_grad_inside_a_backward_hook_does_not_touch_the_outer_pass():
    """A tensor hook that runs torch.autograd.grad on an unrelated sub-graph of HIP operators while the outer backward pass is in
    flight: the inner pass completes its own gradients, the outer pass's gradients equal the plain run."""
    from torch_semantic_segmentation_amd import ops
    m = _fast_features()
    side = _fast_features(seed=43)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 32, 24, 40, generator=g).to(DEV)
    cot = torch.randn(2, 48, 24, 40, generator=g).to(DEV)
    out0, dx0, g0 = _run_plain(m, x, cot)
    _, _, gs0 = _run_plain(side, x, cot, direct=False)

    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    inner = {}

    def hook(grad):
        # an inner pass over ANOTHER model, gradients returned (not accumulated directly): it must neither flush nor drop what the
        # outer pass postponed
        with torch.enable_grad(), ops.direct_grads(False):
            so = ops.materialize(side(x.clone().requires_grad_(True)))
            params = list(side.parameters())
            gs = torch.autograd.grad(so, params, cot)
        inner.update({k: v.detach().clone() for (k, _), v in zip(side.named_parameters(), gs)})
        return grad
    xx = x.clone().requires_grad_(True)
    with ops.direct_grads(True):
        h = ops.materialize(m[1](ops.materialize(m[0](xx))))
        h.register_hook(hook)
        out = ops.materialize(m[3](m[2](h)))
        out.backward(cot)
    torch.cuda.synchronize()
    assert not ops._passes
    g1 = _grads(m)
    assert _same(xx.grad, dx0)
    for k in g0:
        assert _same(g1[k], g0[k]), k
    assert set(inner) == set(gs0)
    for k in gs0:
        assert _same(inner[k], gs0[k]), k


def test_two_trainers_in_two_threads_do_not_share_scheduling_state():
    """Two models stepping concurrently from two host threads (each with its own stream): the backward-pass state is per graph task,
    so both produce the gradients of their single-threaded runs."""
    import threading
    from torch_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(7)
    models = [_fast_features(seed=51), _fast_features(seed=52)]
    xs = [torch.randn(2, 32, 24, 40, generator=g).to(DEV) for _ in range(2)]
    cots = [torch.randn(2, 48, 24, 40, generator=g).to(DEV) for _ in range(2)]
    want = [_run_plain(m, x, c) for m, x, c in zip(models, xs, cots)]
    got, errs = [None, None], []
    barrier = threading.Barrier(2)

    def work(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream(device=DEV)):
                barrier.wait()
                for _ in range(5):
                    got[i] = _run_plain(models[i], xs[i], cots[i])
        except Exception as exc:       # noqa: BLE001
            errs.append(exc)
    torch.cuda.synchronize()
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    torch.cuda.synchronize()
    assert not errs, errs
    assert not ops._passes
    for i in range(2):
        assert _same(got[i][1], want[i][1])
        for k in want[i][2]:
            assert _same(got[i][2][k], want[i][2][k]), (i, k)


# ----------------------------------------------------------------------------- eval-mode inverted residual as one kernel (round 4)

@pytest.mark.parametrize('cin,cout,stride,expansion,shape', [
    (64, 64, 1, 6, (2, 64, 40, 72)), (64, 64, 2, 6, (2, 64, 40, 72)), (64, 96, 2, 6, (1, 64, 37, 53)), (96, 96, 1, 6, (2, 96, 19, 33)),
    (96, 128, 1, 6, (1, 96, 32, 64)), (128, 128, 1, 6, (2, 128, 24, 40)), (64, 64, 1, 6, (1, 64, 128, 256)),
    (32, 32, 1, 6, (2, 32, 30, 50)), (32, 48, 2, 6, (2, 32, 30, 50)), (48, 48, 1, 6, (1, 48, 16, 24)),
    (128, 128, 1, 6, (1, 128, 64, 128)), (96, 96, 1, 6, (1, 96, 13, 21))])
@pytest.mark.parametrize('family', ['fast', 'ctx'])
def test_eval_bottleneck_in_one_kernel_vs_f64_oracle_and_layer_by_layer(cin, cout, stride, expansion, shape, family):
    """csrc/bneck.hip (model.eval(), no gradient, bf16: expand -> BN -> ReLU -> depthwise -> BN -> ReLU -> project -> BN -> (+ x) -> ReLU
    in one kernel, the expanded tensors in LDS) against the reference's block in f64 with the bf16 storage format
    (TSS/models/fastscnn.py:138-161, TSS/models/contextnet.py:129-147), bound = 3 x the oracle-vs-oracle noise distance + floor, and
    against the product's own layer-by-layer eval path (TSS_BNECK_EVAL=0) as the yardstick: every tile shape (8 x 16, 8 x 8, stride 2),
    ragged maps, channel counts of both models; 48 -> 288 is outside the kernel's envelope and must fall back silently."""
    import importlib
    import numpy as np
    from torch import nn
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import ops
    from oracle import nets as O
    from oracle.bf16_storage import emulate_bf16_storage
    mod = importlib.import_module('torch_semantic_segmentation_amd.models.' + ('fastscnn' if family == 'fast' else 'contextnet'))
    torch.manual_seed(17)
    ref = (O._FastResidual if family == 'fast' else O._CtxResidual)(cin, cout, stride=stride, expansion=expansion)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(m.weight.to(torch.bfloat16).float())
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.6, 1.4)
                m.bias.uniform_(-0.3, 0.3)
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    g = torch.Generator().manual_seed(18)
    x = torch.randn(*shape, generator=g).to(torch.bfloat16).float()

    def oracle(dither):
        r = (O._FastResidual if family == 'fast' else O._CtxResidual)(cin, cout, stride=stride, expansion=expansion)
        r.load_state_dict(state)
        r.double().eval()
        emulate_bf16_storage(r, dither=dither)
        with torch.no_grad():
            return r(x.double()).numpy()
    want = oracle(None)
    na, nb = oracle(torch.Generator().manual_seed(1013)), oracle(torch.Generator().manual_seed(2017))

    def hip(fused):
        m = mod.BottleneckBlock(cin, cout, stride=stride, expansion=expansion)
        m.load_state_dict(state, strict=True)
        m.to(DEV).eval()
        tssa.set_compute_dtype(m, torch.bfloat16)
        old = ops.eval_bottleneck
        ops.eval_bottleneck = fused
        calls = []
        orig = ops.bottleneck_eval

        def spy(*a, **k):
            out = orig(*a, **k)
            calls.append(out is not None)
            return out
        ops.bottleneck_eval = spy
        try:
            with torch.no_grad():
                out = ops.materialize(m(x.to(DEV).to(torch.bfloat16)))
            torch.cuda.synchronize()
        finally:
            ops.eval_bottleneck = old
            ops.bottleneck_eval = orig
        return out.float().cpu().double().numpy(), calls
    lean, calls1 = hip(True)
    plain, calls0 = hip(False)
    inside = (cin * expansion) % 64 == 0
    assert calls1 == [inside] and calls0 == [False]
    l2 = lambda a, b: float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
    e_lean, e_plain, e_noise = l2(lean, want), l2(plain, want), l2(na, nb)
    bound = min(3.0 * e_noise + 2e-4, 1e-2)
    assert e_lean <= bound, (e_lean, e_plain, e_noise, bound)
    assert e_lean <= 2.0 * e_plain + 4e-3, (e_lean, e_plain)
    assert np.isfinite(lean).all()
