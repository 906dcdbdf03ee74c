"""float64 CPU restatement of tssa.multiscale_argmax_confusion / tss_multiscale_argmax_confusion, its test inputs, and the
derived bound on the float32 kernel's scores against it.

For every map k (NCHW logits [B, C, h_k, w_k], flag flip_k):
    U_k = F.interpolate(low_k.double(), (H, W), mode='bilinear', align_corners=True);  z_k = U_k.flip(-1) if flip_k else U_k
    score = sum_k softmax(z_k, dim=1)   (average='softmax')      or      sum_k z_k   (average='logits')
    pred  = score.argmax(1)             (torch.argmax: the lowest index wins ties)
The flip is taken AFTER the upsample, at full resolution: a map computed from the mirrored image is mirrored back.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of float32 (round to nearest)

# the twelve maps of the tests: six sizes, each plain and flipped, at an output of 40 x 72
SIZES = ((5, 9), (3, 4), (8, 16), (10, 18), (40, 72), (1, 1))
OUT = (40, 72)


def make_maps(sizes=SIZES, B=2, C=19, seed=0):
    """(lows, flips): for every size a plain and a flipped map, float32 tensors holding bf16-representable values (randn * 4
    rounded to bf16), so that the bf16 and the f32 kernel and the restatement all read the same numbers."""
    torch.manual_seed(seed)
    lows, flips = [], []
    for (h, w) in sizes:
        for f in (False, True):
            lows.append((torch.randn(B, C, h, w) * 4).bfloat16().float())
            flips.append(f)
    return lows, flips


def upsampled(lows, flips, size, dtype=torch.float64):
    out = []
    for low, f in zip(lows, flips):
        z = F.interpolate(low.to(dtype), size=size, mode='bilinear', align_corners=True)
        out.append(z.flip(-1) if f else z)
    return out


def scores(lows, flips, size, average='softmax', dtype=torch.float64):
    """(score [B, C, H, W] of `dtype`, arg-max [B, H, W] int64); maps summed in list order."""
    total = None
    for z in upsampled(lows, flips, size, dtype):
        t = torch.softmax(z, dim=1) if average == 'softmax' else z
        total = t if total is None else total + t
    return total, total.argmax(1)


def top2_gap(score):
    """[B, H, W]: best minus second-best score of every pixel."""
    top = score.topk(2, dim=1).values if score.shape[1] > 1 else torch.cat([score, score - float('inf')], 1)
    return top[:, 0] - top[:, 1]


def coord_error(n_in, n_out):
    """max over dst of |float32 source coordinate - exact source coordinate| of the align_corners=True map n_out -> n_in.

    The kernel (and float32 torch) computes scale = fl((n_in-1)/(n_out-1)) and src = fl(scale * dst), and takes the weight
    l1 = src - i0 (exact: both lie in one binade or i0 = 0).  A compiler may contract that subtraction with the product into one
    FMA, which uses the unrounded scale * dst instead; both variants are evaluated here, exactly, rather than bounded: for an
    identity map (n_in == n_out) the coordinates are exact integers and the error is 0, which a 2 u (n_in-1) bound would miss."""
    if n_out <= 1 or n_in <= 1:
        return 0.0
    dst = np.arange(n_out)
    scale32 = np.float32(n_in - 1) / np.float32(n_out - 1)
    exact = dst.astype(np.float64) * (n_in - 1) / (n_out - 1)
    rounded = (scale32 * dst.astype(np.float32)).astype(np.float64)
    unrounded = np.float64(scale32) * dst.astype(np.float64)
    return float(max(np.abs(rounded - exact).max(), np.abs(unrounded - exact).max()))


def margin(K, C, zmax, sizes, size, average='softmax'):
    """Bound on |score_f32 - score_f64| of one class score of one pixel, for K maps of C classes whose logits are at most `zmax`
    in magnitude; `sizes` are the K maps' (h, w), `size` the output (H, W).  First order in u = 2^-24.  Derived, not tuned.

    The logit of one map, z = l0y (l0x a + l1x b) + l1y (l0x c + l1x d) with |a|..|d| <= zmax:
      coordinates   the bilinear surface is continuous and piecewise linear with slope at most 2 zmax per source pixel along
                    each axis (two neighbours differ by at most 2 zmax), so a coordinate that is off by e moves z by at most
                    2 zmax e, also when it crosses into the next cell:  2 zmax (coord_error(h, H) + coord_error(w, W))
      6 u zmax      the roundings of the blend on magnitudes <= zmax: l0x = 1 - l1x, the two products (their magnitudes add up
                    to at most zmax, so together u zmax), the sum -- 3 for a horizontally blended row, carried through the convex
                    vertical blend -- then l0y = 1 - l1y, the two products, the sum.  FMAs only remove roundings.
      dz_k = the sum of the two.
    average='logits':  score = sum_k z_k.  The K-1 additions round partial sums of magnitude <= j zmax:
          sum_k dz_k + u zmax K (K + 1) / 2
    average='softmax': score = sum_k p_k, p = e_c / s, e_c = exp(z_c - m), s = sum_c e_c.
      A perturbation of the logits by at most d moves a softmax output by at most d / 2 (|dp_c| <= p_c sum_j p_j |d_c - d_j|
      <= 2 p_c (1 - p_c) d), a relative perturbation r of the exponentials by at most r / 2 likewise.
      dz_k / 2          the interpolation error above
      2 u zmax          the subtraction z_c - m (|z_c - m| <= 2 zmax: u 2 zmax) and the product with log2(e) inside the
                        exponential (again relative u on the argument, absolute u 2 zmax): 4 u zmax on the logits, halved
      2 u               the exponential itself, 1 ulp = 2 u relative per the HIP math API's table for __expf, as a relative
                        perturbation of 4 u of e_c against e_j, halved
      (C - 1) u         the C - 1 additions of the positive terms of s: relative (C - 1) u on s, times p_c <= 1
      2 u               the reciprocal of s and the product e_c * (1 / s), on p_c <= 1
      and the K - 1 additions of terms <= 1:  u K (K + 1) / 2.
    The inputs are exact on both sides (bf16 widens exactly); the float64 restatement's own error is 1e-9 of this."""
    H, W = size
    assert len(sizes) == K
    dz = [2.0 * zmax * (coord_error(h, H) + coord_error(w, W)) + 6.0 * U * zmax for (h, w) in sizes]
    if average == 'logits':
        return sum(dz) + U * zmax * K * (K + 1) / 2.0
    per_map = 2.0 * U * zmax + 2.0 * U + (C - 1) * U + 2.0 * U
    return sum(d / 2.0 for d in dz) + K * per_map + U * K * (K + 1) / 2.0


def confusion(pred, target, C, ignore_index=255):
    """int64 [C, C], rows = truth; targets equal to ignore_index or outside 0..C-1 are skipped."""
    pred, target = pred.reshape(-1).long(), target.reshape(-1).long()
    keep = (target != ignore_index) & (target >= 0) & (target < C)
    return torch.bincount(target[keep] * C + pred[keep], minlength=C * C).reshape(C, C)
