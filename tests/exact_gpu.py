"""GPU harness of the exact-operand tests (tests/test_gpu_zoo_exact.py, tests/test_gpu_dw_exact.py): sentinel-padded device buffers with
spare rows, NaN statistics slabs, the dyadic operands of a layer with planted exact zeros, and the checks against tests/exact.py's bounds."""
import torch

from tests import exact as X

DEV = 'cuda:0'
SPARE = 5            # rows of sentinel after the last pixel of every output buffer


def N_():
    from torch_semantic_segmentation_amd import _native
    return _native


def dev(v):
    return None if v is None else v.float().to(DEV)


class Buf:
    """a [P + SPARE][ld] bf16 device buffer, sentinel everywhere, the tensor's rows (f64 [P][C], exact bf16 values) at columns
    [off, off + C); .ptr points at column off"""
    def __init__(self, P, C, ld, off=0, rows=None, dtype=torch.bfloat16):
        self.P, self.C, self.ld, self.off = P, C, ld, off
        t = X.sentinel((P + SPARE, ld), dtype=dtype)
        if rows is not None:
            t[:P, off:off + C] = rows.to(dtype)
        self.t = t.to(DEV)
        self.ptr = self.t.data_ptr() + t.element_size() * off
        self.sbits = X.SENTINEL_BITS32 if dtype == torch.float32 else X.SENTINEL_BITS

    def rows(self):
        return self.t[:self.P, self.off:self.off + self.C].double().cpu()

    def untouched(self):
        """every element outside the tensor's window still holds the sentinel"""
        b = X.bits(self.t.cpu()).clone()
        b[:self.P, self.off:self.off + self.C] = self.sbits
        return bool((b == self.sbits).all())


def nan_slabs(C):
    return torch.full((N_().stat_slabs(), 2 * C), float('nan'), dtype=torch.float64, device=DEV)


def to_rows(t):
    return X.nchw_to_rows(t)


# ----------------------------------------------------------------------------------------------------- operands of a layer
class Layer:
    """dyadic operands of a convolution layer: input x [B][Cin][H][W] with its pending BatchNorm (mean, scale, bias) and ReLU, weights
    [N][Cin][kh][kw], conv bias, and the backward operands e, y [B][N][Ho][Wo] with (ga, gb, gce, gmu)"""
    def __init__(self, seed, B, Cin, H, W, N, kshape, Ho, Wo, affine=True, relu=True, cbias=True):
        g = torch.Generator().manual_seed(seed)
        self.draw_input(g, B, Cin, H, W, affine, relu)
        self.w = X.dyadic((N, Cin) + tuple(kshape), g, emin=-6, emax=-2)
        self.cb = X.dyadic((N,), g) if cbias else None
        self.draw_backward(g, N, Ho, Wo)

    def draw_input(self, g, B, Cin, H, W, affine, relu):
        """x [B][Cin][H][W] with its pending BatchNorm (exact zeros of the pre-activation planted) or materialised (exact zeros of x)"""
        self.B, self.Cin, self.H, self.W, self.relu = B, Cin, H, W, relu
        if affine:
            self.mean, self.bias = X.dyadic((1, Cin, 1, 1), g), X.dyadic((1, Cin, 1, 1), g)
            self.scale = X.pow2((1, Cin, 1, 1), g, 0.5, 4)
            x = X.dyadic((B, Cin, H, W), g)
            self.x = X.plant_zeros(x, self.mean, self.scale, self.bias, g, 0.04)
        else:
            self.mean = self.scale = self.bias = None
            self.x = X.dyadic((B, Cin, H, W), g, zero_frac=0.04)

    def draw_backward(self, g, N, Ho, Wo):
        """e, y [B][N][Ho][Wo] and the BatchNorm-backward coefficients (ga, gb, gce, gmu)"""
        B = self.B
        self.N, self.Ho, self.Wo = N, Ho, Wo
        self.e, self.y = X.dyadic((B, N, Ho, Wo), g), X.dyadic((B, N, Ho, Wo), g)
        self.ga, self.gb = X.pow2((1, N, 1, 1), g, 0.25, 2), X.pow2((1, N, 1, 1), g, 2.0 ** -6, 2.0 ** -3)
        self.gce, self.gmu = X.dyadic((1, N, 1, 1), g), X.dyadic((1, N, 1, 1), g)

    def a(self):
        return X.act(self.x, self.mean, self.scale, self.bias, self.relu)

    def gop(self, mode):
        return X.gcomb(self.e, self.y, self.ga, self.gb, self.gce, self.gmu) if mode == 2 else X.gcomb(self.e, ga=self.ga)

    def mask(self):
        """torch's relu backward: gradient where the pre-activation is > 0 (exact zeros planted among them)"""
        return (X.pre_act(self.x, self.mean, self.scale, self.bias) > 0).double() if self.relu else torch.ones_like(self.x)


def vecs(L):
    """device copies of the per-channel vectors, kept alive by the caller"""
    d = {k: (dev(getattr(L, k, None).reshape(-1)) if getattr(L, k, None) is not None else None)
         for k in ('mean', 'scale', 'bias', 'cb', 'ga', 'gb', 'gce', 'gmu')}
    return d


def check_out(buf, ref, S, K, what):
    out = buf.rows()
    ex = X.conv_excess(out, ref, S, K)
    assert ex <= 0, (what, 'excess over the bound', ex)
    assert buf.untouched(), (what, 'sentinel overwritten')
    return out


def check_stats(slabs, terms, chain, what):
    s = slabs.double().cpu()
    assert not torch.isnan(s).any(), (what, 'a slab row neither written nor zeroed')
    ex = X.stats_excess(s.sum(0), terms, chain)
    assert ex <= 0, (what, 'statistics excess', ex)
