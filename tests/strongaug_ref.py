"""float64 restatement of tss_strong_augment (tssa.strong_augment: colour jitter and Gaussian blur of a normalised batch), the
elementwise tolerance of the float32 kernel against it, and the cases that tests/test_strongaug_oracle.py (CPU) and
tests/test_gpu_strongaug.py share.

Semantics (include/tss_hip.h): per sample rows color = (apply, fb, fc, fs, dh, ...), radius R, taps w_0..w_8.  apply == 0 and R == 0:
the sample on bits.  Else u_c = x_c std_c + mean_c; if apply: brightness u = clamp(u fb), contrast u = clamp(m + fc (u - m)) with m
the sample's mean grey value (0.299, 0.587, 0.114) AFTER brightness, saturation u = clamp(g + fs (u - g)) with g the pixel's own grey
value, hue = tests/augment_hsv_ref.hsv_shift on 255 u with a shift of 180 dh and ds = dv = 0, divided by 255; blur if R > 0:
horizontal then vertical, mirrored borders that do not repeat the edge pixel, nothing clamped after it; x' = v isd_c + shift_c.

Given numbers, taken as exact by the restatement: the input, the float32 rows (factors, dh, taps), the float32 mean / std and
isd = 1/std, shift = -mean/std formed in float32, and m ROUNDED to float32 (computed here in float64 first).  Everything else is
float64, so the comparison counts the kernel's arithmetic roundings only.

Tolerance (derived, first order in U = 2^-24, nothing tuned; e is the error carried into a step, clamps are 1-Lipschitz, a fused
multiply-add only removes a rounding):
  denormalise   e = U |x std| + U |u|                                         product, sum
  brightness    e = fb e + U |u fb|
  grey          e_g = sum_c k_c e_c + 4 U g                                    the float32 coefficient, product and two sums per term
  mean          e_m = mean(e_g) + U m                                          float64 sums are exact at this order; one rounding to f32
  contrast      e = |1 - fc| e_m + fc e + 2 U fc |u - m| + U |m + fc (u - m)|  difference, product, sum
  saturation    e = |1 - fs| e_g + fs e + 2 U fs |u - g| + U |g + fs (u - g)|
  hue           on p = 255 u, e_in = max_c (255 e_c + U p_c): augment_hsv_ref.hsv_tolerance's chain with ds = dv = 0, where the
                1 / D and 1 / V of the hue and saturation terms cancel:
                  d = (e_in + 510 U) + [D > 0] 2 e_in + V s 44 U + V ((dS + 510 U) / 255 + U) + 4 U V,
                  dS = (255 / V)(1 + min / V) e_in + 3 U S;   44 = that chain's 40 + the product 180 dh (<= 90 U of hue, / 30) + 1
                then e = d / 255 + U |u|.  At D = 0 exactly the definition returns (V, V, V) and the bound holds as it stands (the
                kernel's own chroma is at most 2 e_in and its output lies between its min and max).  The first-order hue term
                assumes e_in << D (second-order terms are e_in / D of it): where 0 < D < 1024 e_in the bound is NOT valid and D is
                added to it -- exact arithmetic keeps every output between the pixel's min and max, for the kernel's input and for
                ours, so the two differ by at most D + e_in.  Those are the elements the first-order bound does not cover;
                `fallback_share` is their share of a case and must stay below 1 %.
  blur pass     e = sum |w| e + (4R + 1) U sum |w| |u|                         at most 2R + 1 roundings on any path of the sum
  renormalise   e = |isd| e + U |v isd| + U |x'|;  bf16 output: + 2^-8 (|x'| + e), half a bf16 ulp of the kernel's value
and the whole is multiplied by 1 + 2^-8 for the second-order terms (<= 2^-10 of the hue term, n U of the others)."""
import functools

import numpy as np

from tests import augment_hsv_ref as HSV

U = 2.0 ** -24
GREY = np.array([0.299, 0.587, 0.114])
FALLBACK = 1024.0
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
VARIANTS = ('radius-1', 'clamp', 'm-before', 'dh-neg')


def constants(mean, std):
    """(mean, std, isd, shift) as float64 [3,1,1] holding the float32 numbers the kernel gets."""
    m = np.zeros(3, np.float32) if mean is None else np.asarray(mean, np.float32)
    s = np.ones(3, np.float32) if std is None else np.asarray(std, np.float32)
    isd, shift = np.float32(1.0) / s, -m / s                      # float32 operations, as the entry point forms them
    return tuple(a.astype(np.float64).reshape(3, 1, 1) for a in (m, s, isd, shift))


def reflect(i, n, border='mirror'):
    if border == 'clamp':
        return np.clip(i, 0, n - 1)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def blur_axis(a, taps, R, axis, border='mirror'):
    """sum_{k=-R..R} w_|k| a(.., refl(i + k), ..) along `axis`, float64."""
    n = a.shape[axis]
    idx = np.arange(n)
    out = np.zeros_like(a, dtype=np.float64)
    for k in range(-R, R + 1):
        out += float(taps[abs(k)]) * np.take(a, reflect(idx + k, n, border), axis=axis)
    return out


def grey(u):
    return np.tensordot(GREY, u, axes=(0, 0))


def bf16_round(a):
    """float32 array rounded to the nearest bfloat16 (ties to even), as float32."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32)


def truncated_taps(taps, R):
    """the taps cut to radius R - 1 and renormalised: the wrong kernel of the discriminating-power check"""
    t = np.zeros(12, np.float64)
    t[:R] = np.asarray(taps[:R], np.float64)
    return t / (t[0] + 2.0 * t[1:].sum())


def jitter(u, e, color, variant=None):
    """the four colour steps on u [3,H,W] with carried error e; returns (u, e, fallback [H,W])"""
    fb, fc, fs, dh = (float(v) for v in color[1:5])
    ub = u * fb
    e = fb * e + U * np.abs(ub)
    u1 = np.clip(ub, 0.0, 1.0)
    g1 = grey(u if variant == 'm-before' else u1)
    e_g = np.tensordot(GREY, e, axes=(0, 0)) + 4.0 * U * np.abs(g1)
    m = float(np.float32(g1.mean()))
    e_m = float(e_g.mean()) + U * abs(m)
    t = m + fc * (u1 - m)
    e = abs(1.0 - fc) * e_m + fc * e + 2.0 * U * fc * np.abs(u1 - m) + U * np.abs(t)
    u2 = np.clip(t, 0.0, 1.0)
    g2 = grey(u2)
    e_g = np.tensordot(GREY, e, axes=(0, 0)) + 4.0 * U * g2
    t = g2 + fs * (u2 - g2)
    e = abs(1.0 - fs) * e_g + fs * e + 2.0 * U * fs * np.abs(u2 - g2) + U * np.abs(t)
    u3 = np.clip(t, 0.0, 1.0)
    p = 255.0 * u3
    e_in = (255.0 * e + U * p).max(0)
    r, g, b = HSV.hsv_shift(p[0], p[1], p[2], 180.0 * (-dh if variant == 'dh-neg' else dh), 0.0, 0.0)
    V, mn = p.max(0), p.min(0)
    D = V - mn
    with np.errstate(divide='ignore', invalid='ignore'):
        S = np.where(V > 0, 255.0 * D / V, 0.0)
        d_S = np.where(V > 0, (255.0 / V) * (1.0 + mn / V), 0.0) * e_in + 3.0 * U * S
    d = (e_in + 510.0 * U) + np.where(D > 0, 2.0 * e_in, 0.0) + V * (S / 255.0) * 44.0 * U + V * ((d_S + 510.0 * U) / 255.0 + U) + 4.0 * U * V
    fallback = (D > 0) & (D < FALLBACK * e_in)
    d = np.where(fallback, d + D, d)
    u4 = np.stack([r, g, b]) / 255.0
    return u4, d[None] / 255.0 + U * np.abs(u4), fallback


def sample(x, color, R, taps, K, bf16=False, variant=None):
    """One sample: x float64 [3,H,W] (the exact input values).  Returns (out, tol, fallback [H,W] bool); out is None for an identity
    sample (apply == 0 and R == 0: the input on bits)."""
    mean, std, isd, shift = K
    apply, R = float(color[0]) != 0.0, int(R)
    fallback = np.zeros(x.shape[1:], bool)
    if not apply and R == 0:
        return None, None, fallback
    u = x * std + mean
    e = U * np.abs(x * std) + U * np.abs(u)
    if apply:
        u, e, fallback = jitter(u, e, color, variant)
    if variant == 'radius-1' and R > 0:
        taps, R = truncated_taps(taps, R), R - 1
    if R > 0:
        for axis in (2, 1):                                           # horizontal, then vertical
            border = 'clamp' if variant == 'clamp' else 'mirror'
            e = blur_axis(e, taps, R, axis, border) + (4 * R + 1) * U * blur_axis(np.abs(u), taps, R, axis, border)
            u = blur_axis(u, taps, R, axis, border)
    y = u * isd + shift
    e = np.abs(isd) * e + U * np.abs(u * isd) + U * np.abs(y)
    if bf16:
        e = e + 2.0 ** -8 * (np.abs(y) + e)
    return y, e * (1.0 + 2.0 ** -8), fallback


def batch(x, color, radius, taps, mean=None, std=None, bf16=False, variant=None):
    """x float64 [B,3,H,W]; returns lists (out, tol, fallback) per sample."""
    K = constants(mean, std)
    res = [sample(x[b], color[b], radius[b], taps[b], K, bf16, variant) for b in range(x.shape[0])]
    return [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]


# ------------------------------------------------------------------------------------------------------------- the shared cases

def wide_taps(R):
    """float32 taps [12] of radius R: a Gaussian of sigma = R / 1.5 cut at R and normalised in float64.  The taps are data to the
    kernel; gaussian_taps cuts at 3 sigma, where the last tap is 1 % of the first -- below half a bf16 ulp of the result, so a
    kernel that dropped it could not be told from a right one in the bf16 cases.  Here the last tap is a third of the first."""
    taps = np.zeros(12, np.float32)
    k = np.arange(R + 1, dtype=np.float64)
    e = np.exp(-k * k / (2.0 * (R / 1.5) ** 2)) if R else np.ones(1)
    taps[:R + 1] = (e / (e[0] + 2.0 * e[1:].sum())).astype(np.float32)
    return taps


def _row(apply=0, fb=1.0, fc=1.0, fs=1.0, dh=0.0, R=0):
    return np.array([apply, fb, fc, fs, dh, 0, 0, 0], np.float32), R, wide_taps(R)


def row_sets():
    """name -> three sample rows.  Between them: all-identity, colour only, blur only, both, every radius 0..8, fb = 0, fc = 0,
    fs = 0 and 2, dh = +-0.5 and 0."""
    col = dict(apply=1, fb=1.2, fc=0.8, fs=1.25, dh=0.15)
    sets = {
        'identity': [_row(), _row(), _row()],
        'mixed': [_row(**col), _row(R=4), _row(apply=1, fb=0.85, fc=1.2, fs=0.8, dh=-0.2, R=8)],
        'degenerate': [_row(apply=1, fb=0.0, fc=0.9, fs=1.1, dh=0.1), _row(apply=1, fb=1.1, fc=0.0, fs=1.2, dh=0.1),
                       _row(apply=1, fb=0.7, fc=1.4, fs=0.0, dh=0.3, R=2)],
        'extreme': [_row(apply=1, fb=1.3, fc=0.6, fs=2.0, dh=0.0), _row(apply=1, fb=0.7, fc=1.4, fs=1.1, dh=0.5, R=3),
                    _row(apply=1, fb=1.0, fc=1.0, fs=0.9, dh=-0.5)],
    }
    for k in range(3):
        sets['radii%d' % k] = [_row(apply=(3 * k + j) % 2, fb=1.3, fc=1.5, fs=0.9, dh=0.05 * (j + 1), R=3 * k + j)
                               for j in range(3)]
    return sets


def sizes(tile):
    th, tw = tile
    return [(9, 16), (23, 40), (2 * th + 5, 2 * tw + 8)]


def case_ids(tile):
    return ['%s-%dx%d-%s-%s' % (name, h, w, dt, 'norm' if norm else 'raw')
            for name in row_sets() for (h, w) in sizes(tile) for dt in ('f32', 'bf16') for norm in (False, True)]


@functools.lru_cache(maxsize=None)
def case(case_id, tile):
    """The inputs of one case (B = 3): dict(x float32 [3,3,H,W] holding the exact input values, bf16, mean, std, color, radius, taps).
    Independent uniform random bytes / 255 per channel, normalised with the ImageNet constants (norm) or not, with exactly-grey and
    exactly-black pixels planted before that; the rows rotate over the samples with the size, so each row meets each size.  The
    planted patches are a 2x2 block of each kind per sample, and at 9x16 one grey pixel in sample 0 and one black one in sample 1:
    with mean / std they are no longer exactly grey after the float32 round trip, so they land in the fallback share."""
    name, size, dt, norm = case_id.rsplit('-', 3)
    H, W = (int(v) for v in size.split('x'))
    si = [s for s in sizes(tile)].index((H, W))
    rows = row_sets()[name]
    rows = rows[si:] + rows[:si]
    rng = np.random.default_rng(sum(map(ord, name)) * 1000 + H * 131 + W)
    by = rng.integers(0, 256, size=(3, 3, H, W)).astype(np.float64)
    if H * W >= 800:
        for b in range(3):
            by[b, :, 3:5, 5:7] = float(rng.integers(1, 255))
            by[b, :, 6:8, 9:11] = 0.0
    else:
        by[0, :, 4, 7] = 77.0
        by[1, :, 2, 3] = 0.0
    x = by / 255.0
    mean, std = (IMAGENET_MEAN, IMAGENET_STD) if norm == 'norm' else (None, None)
    if mean is not None:
        x = (x - np.asarray(mean).reshape(1, 3, 1, 1)) / np.asarray(std).reshape(1, 3, 1, 1)
    x = x.astype(np.float32)
    if dt == 'bf16':
        x = bf16_round(x)
    x.setflags(write=False)
    return dict(x=x, bf16=dt == 'bf16', mean=mean, std=std, color=np.stack([r[0] for r in rows]),
                radius=np.array([r[1] for r in rows], np.int32), taps=np.stack([r[2] for r in rows]), identity=name == 'identity')


@functools.lru_cache(maxsize=None)
def reference(case_id, tile, variant=None):
    """(out, tol, fallback) lists of a case: computed once, shared, not to be modified."""
    c = case(case_id, tile)
    return batch(c['x'].astype(np.float64), c['color'], c['radius'], c['taps'], c['mean'], c['std'], c['bf16'], variant)


def fallback_share(case_id, tile):
    fb = reference(case_id, tile)[2]
    return float(np.mean([f.mean() for f in fb]))
