"""tss_stem3x3_bwd_weight_rc (csrc/stem.hip, stem_wgrad_rc_mfma_kernel): the stem's weight gradient with y recomputed inside the kernel.

The claim is bit identity, so every comparison is torch.equal, no tolerance:
  a  the new entry given w against tss_stem3x3_bwd_weight given yraw = tss_stem3x3_fwd(x, w), both adding onto the same nonzero dW, and
     the per-block partial rows they leave in the workspace (same tile plan, same accumulation order)
  b  what the direct forward does not cover is refused with TSS_ERR_SHAPE and nothing is launched
  c  FastSCNN's learning-to-downsample front, train mode, bf16: every parameter gradient with ops.stem_wgrad_recompute on and off; a
     weight changed in place between forward and backward is served by the kernel that reads y
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF, F32 = torch.bfloat16, torch.float32

# (B, Cin, Hin, Win, stride)
SHAPES = [
    (1, 3, 8, 8, 2),          # one partial tile that touches all four image edges
    (2, 3, 18, 34, 2),        # 9 x 17 per image, 306 pixels: two tiles, the second partial; output width not a multiple of 4
    (1, 1, 6, 4, 2),          # Cin = 1, the narrowest image that takes the 16-byte window path
    (1, 3, 5, 3, 2),          # Win < 4: the per-tap path
    (2, 3, 512, 1024, 2),     # 262 144 pixels = 1024 tiles on 512 blocks: two tiles per block, accumulation across tiles
    (1, 3, 8, 8, 1),          # stride 1 (the direct forward takes it)
]


def _native():
    from torch_semantic_segmentation_amd import _native as n
    return n


class Operands:
    def __init__(self, seed, B, Cin, Hin, Win, stride, image_dtype, N=32, act=BF):
        n = _native()
        g = torch.Generator().manual_seed(seed)
        self.B, self.Cin, self.Hin, self.Win, self.stride, self.N = B, Cin, Hin, Win, stride, N
        self.Ho, self.Wo = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
        self.P = B * self.Ho * self.Wo
        self.x = torch.randn((B, Cin, Hin, Win), generator=g).to(image_dtype).to(DEV)
        self.is_f32 = int(image_dtype == F32)
        self.w = (0.25 * torch.randn((N, Cin, 3, 3), generator=g)).to(DEV)
        e = torch.randn((self.P, N), generator=g)
        e = e * (torch.rand((self.P, N), generator=g) < 0.5)          # about half of the gradient is zero (ReLU behind the BatchNorm)
        self.e = e.to(act).to(DEV)
        self.ga, self.gb, self.gce, self.gmu = [(0.5 + torch.rand(N, generator=g)).to(DEV) * s for s in (1.0, -0.75, 0.125, 0.5)]
        self.dw0 = torch.randn((N, Cin, 3, 3), generator=g).to(DEV)
        self.code, self.st = n.dtype_code(act), n.stream()
        self.slabs = n.stat_slabs()
        self.rows = min((self.P + 255) // 256, self.slabs)

    def geometry(self):
        return (self.B, self.Cin, self.Hin, self.Win, self.N, self.stride, self.code, self.st)

    def coeffs(self):
        n = _native()
        return (n.ptr(self.ga), n.ptr(self.gb), n.ptr(self.gce), n.ptr(self.gmu))

    def forward(self):
        n = _native()
        y = torch.full((self.P, self.N), float('nan'), dtype=BF, device=DEV)
        n.call('tss_stem3x3_fwd', n.ptr(self.x), self.is_f32, n.ptr(self.w), n.ptr(y), self.N, None, *self.geometry())
        return y

    def workspace(self):
        return torch.full((self.slabs, self.N * 28), float('nan'), device=DEV)

    def rc_args(self, dw, ws):
        n = _native()
        return (n.ptr(self.e), self.N, n.ptr(self.w), *self.coeffs(), n.ptr(self.x), self.is_f32, n.ptr(dw), n.ptr(ws), *self.geometry())


@pytest.mark.parametrize('image_dtype', [F32, BF], ids=['f32image', 'bf16image'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s[:4])) + '_s%d' % s[4])
def test_recomputed_y_gives_the_bits_of_the_stored_y(shape, image_dtype):
    n = _native()
    o = Operands(1000 + sum(shape), *shape, image_dtype)
    y = o.forward()
    dw_old, dw_new, ws_old, ws_new = o.dw0.clone(), o.dw0.clone(), o.workspace(), o.workspace()
    n.call('tss_stem3x3_bwd_weight', n.ptr(o.e), o.N, n.ptr(y), o.N, *o.coeffs(), n.ptr(o.x), o.is_f32, n.ptr(dw_old), n.ptr(ws_old),
           *o.geometry())
    n.call('tss_stem3x3_bwd_weight_rc', *o.rc_args(dw_new, ws_new))
    torch.cuda.synchronize()
    assert not torch.isnan(y.float()).any()
    assert torch.isfinite(dw_old).all() and not torch.equal(dw_old, o.dw0)
    assert torch.equal(ws_new[:o.rows], ws_old[:o.rows]), 'per-block partial sums differ'
    assert torch.isnan(ws_new[o.rows:]).all(), 'a workspace row past the grid was written'
    assert torch.equal(dw_new, dw_old), (shape, image_dtype, (dw_new - dw_old).abs().max().item())


@pytest.mark.parametrize('N,act', [(64, BF), (32, F32)], ids=['N64', 'f32act'])
def test_out_of_coverage_is_refused_without_a_launch(N, act):
    n = _native()
    o = Operands(7, 1, 3, 8, 8, 2, F32, N=N, act=act)
    dw, ws = o.dw0.clone(), o.workspace()
    rc = getattr(n.lib(), 'tss_stem3x3_bwd_weight_rc')(*o.rc_args(dw, ws))
    torch.cuda.synchronize()
    assert rc == -2      # TSS_ERR_SHAPE
    assert torch.equal(dw, o.dw0) and torch.isnan(ws).all()


# ----------------------------------------------------------------------------------------------------- module level

def _front_gradients(monkeypatch, recompute, bump):
    """parameter gradients of FastSCNN.downsample (stem + two depthwise-separable blocks) after one train-mode forward + backward at
    2 x 3 x 64 x 128 in bf16, and the weight-gradient entries the stem's backward called"""
    import torch_semantic_segmentation_amd as tssa
    from oracle.recipe import formula_state, lattice_input
    from tests import cases
    from torch_semantic_segmentation_amd import ops
    monkeypatch.setattr(ops, 'stem_wgrad_recompute', recompute)
    calls = []
    real = _native().call

    def spy(name, *args):
        if name.startswith('tss_stem3x3_bwd_weight'):
            calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(ops, 'call', spy)
    model = cases.product_model('fastscnn')
    model.load_state_dict(formula_state(model), strict=True)
    model.train().to(DEV)
    tssa.set_compute_dtype(model, BF)
    front = model.downsample
    x = lattice_input(2, 3, 64, 128).to(DEV)
    if bump:     # identity hooks: autograd hands the backward the saved weight as it is then, instead of refusing the changed version
        with torch.autograd.graph.saved_tensors_hooks(lambda t: t, lambda t: t):
            out = ops.materialize(front(x))
        with torch.no_grad():
            front[0][0].weight.mul_(1.5)
    else:
        out = ops.materialize(front(x))
    g = torch.Generator().manual_seed(11)
    out.backward(torch.randn(out.shape, generator=g).to(DEV).to(out.dtype).contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in front.named_parameters()}
    assert all(v is not None and torch.isfinite(v).all() for v in grads.values())
    return grads, calls


@pytest.mark.parametrize('bump', [False, True], ids=['same_weight', 'weight_changed_in_place'])
def test_front_gradients_do_not_depend_on_the_switch(monkeypatch, bump):
    on, calls_on = _front_gradients(monkeypatch, True, bump)
    off, calls_off = _front_gradients(monkeypatch, False, bump)
    assert calls_off == ['tss_stem3x3_bwd_weight']
    assert calls_on == ['tss_stem3x3_bwd_weight' if bump else 'tss_stem3x3_bwd_weight_rc']
    assert sorted(on) == sorted(off) and len(on) >= 3
    for k in on:
        assert torch.equal(on[k], off[k]), k
