"""numpy restatement of tss_augment_batch_u8_ex (tssa.augment_batch(..., color=, label_map=)): tests/augment_ref.py's bilinear
blend, then HueSaturationValue on the blended (r, g, b), then Normalize; the nearest-sampled label through a 256-entry table.  And
the tolerance of the float32 kernel against it.

Colour row (apply, dh, ds, dv) of a sample; with apply != 0 every pixel's blend (r, g, b), in grey levels 0..255, becomes
(albumentations' additive HueSaturationValue on cv2's 8-bit HSV scale, kept continuous: nothing is rounded to uint8)

    V = max, m = min, D = V - m;   S = 255 D / V (0 at V = 0)
    H in [0, 180), units of 2 degrees: 0 at D = 0, else 30 (g-b)/D if V == r, else 60 + 30 (b-r)/D if V == g, else
        120 + 30 (r-g)/D; + 180 when negative
    H' = H + dh wrapped once into [0, 180) (|dh| <= 180);  S' = clamp(S + ds, 0, 255);  V' = clamp(V + dv, 0, 255)
    h = H'/30, i = floor(h), f = h - i;  p = V'(1 - S'/255), q = V'(1 - f S'/255), t = V'(1 - (1-f) S'/255)
    (r, g, b) = (V',t,p) (q,V',p) (p,V',t) (p,q,V') (t,p,V') (V',p,q) for i = 0..5

then out = v * sc[c] + sh[c] as in augment_ref.  A wrapped H' can round to 180.0 (a tiny negative hue plus 180): i = 6 is read
as sector 0, where f = 0 gives the same colour.  A grey pixel has H = 0, so ds > 0 tints it red (the reference's behaviour).
Everything here is float64, but for hsv_shift's float32 switch."""
import numpy as np

from tests import augment_ref as R

U = R.U
E_IN = 13.0 * U * 255.0      # float32 error of one blended value: image_tolerance's 14 roundings without the product v * sc


def hsv_shift(r, g, b, dh, ds, dv, dtype=np.float64):
    """The transform above on arrays r, g, b (grey levels) with scalar shifts; returns (r', g', b').  float64 is the restatement;
    dtype=np.float32 evaluates the same operations in float32 (what the kernel does, without its fused multiply-adds)."""
    r, g, b = (np.asarray(a, dtype=dtype) for a in (r, g, b))
    dh, ds, dv = dtype(dh), dtype(ds), dtype(dv)
    V = np.maximum(r, np.maximum(g, b))
    D = V - np.minimum(r, np.minimum(g, b))
    with np.errstate(divide='ignore', invalid='ignore'):
        S = np.where(V > 0, 255.0 * D / V, 0.0)
        num = np.where(V == r, g - b, np.where(V == g, b - r, r - g))
        base = np.where(V == r, 0.0, np.where(V == g, 60.0, 120.0)).astype(dtype)
        H = np.where(D > 0, base + 30.0 * num / D, 0.0)
    H = np.where(H < 0, H + 180.0, H)
    H = H + dh
    H = np.where(H < 0, H + 180.0, np.where(H >= 180.0, H - 180.0, H))
    h = H / 30.0
    fl = np.floor(h)
    f = h - fl
    i = fl.astype(np.int64) % 6
    V2 = np.clip(V + dv, 0.0, 255.0)
    s = np.clip(S + ds, 0.0, 255.0) / 255.0
    p, q, t = V2 * (1.0 - s), V2 * (1.0 - f * s), V2 * (1.0 - (1.0 - f) * s)
    return (np.choose(i, [V2, q, p, p, t, V2]), np.choose(i, [t, V2, V2, q, p, p]), np.choose(i, [p, p, t, V2, V2, q]))


def blend(image, params, crop_size, image_hwc=False):
    """float64 [B, C, ch, cw]: the bilinear blends of augment_ref.augment in grey levels, before Normalize."""
    ch, cw = crop_size
    img = np.asarray(image)
    if image_hwc:
        img = img.transpose(0, 3, 1, 2)
    B, C = img.shape[:2]
    out = np.empty((B, C, ch, cw), np.float64)
    for b in range(B):
        Hs, Ws, oy, ox, flip = (int(v) for v in np.asarray(params)[b, :5])
        Ys = oy + np.arange(ch)
        Xs = ox + (cw - 1 - np.arange(cw) if flip else np.arange(cw))
        for c in range(C):
            out[b, c] = R.sample_bilinear(img[b, c], Ys, Xs, Hs, Ws)
    return out


def shift_blend(grey, color):
    """float64 [B, 3, ch, cw]: `grey` (blend()'s result) with the colour rows [B, 4] applied."""
    out = np.array(grey, dtype=np.float64)
    for b, (apply, dh, ds, dv) in enumerate(np.asarray(color, dtype=np.int64)):
        if apply:
            out[b, 0], out[b, 1], out[b, 2] = hsv_shift(grey[b, 0], grey[b, 1], grey[b, 2], dh, ds, dv)
    return out


def normalize(grey, mean=None, std=None):
    sc, sh = R.constants(grey.shape[1], mean, std)
    return grey * sc[None, :, None, None] + sh[None, :, None, None]


def augment(image, target, params, crop_size, mean=None, std=None, image_hwc=False, color=None, label_map=None):
    """As augment_ref.augment, with colour rows `color` [B, 4] (None: no colour step) and the table `label_map` [256]."""
    out_x = out_y = None
    if image is not None:
        grey = blend(image, params, crop_size, image_hwc)
        out_x = normalize(grey if color is None else shift_blend(grey, color), mean, std)
    if target is not None:
        _, out_y = R.augment(None, target, params, crop_size)
        if label_map is not None:
            out_y = np.asarray(label_map, dtype=np.int64)[out_y]
    return out_x, out_y


def conditioning(grey):
    """(D, V) float64 [B, ch, cw] of the blends: the transform is ill-conditioned where D (hue) or V (saturation) is small."""
    return grey.max(1) - grey.min(1), grey.max(1)


def hsv_tolerance(grey, color, mean=None, std=None):
    """Elementwise bound on |kernel - augment()| for the float32 kernel, shaped like `grey` ([B, 3, ch, cw], blend()'s result).

    Derived, not tuned; first order in u = 2^-24, as augment_ref.image_tolerance, and like it in grey levels until the last line.
    A row with apply = 0 gets image_tolerance itself.  Otherwise, with e = 13 u 255 the error of each of r, g, b on entry (the
    blend: image_tolerance's count without the product v sc), m = min(r, g, b), and |x| <= 255 for V, S, V', S', |30 num / D| <= 30,
    |H| <= 180, |H + dh| <= 360, h <= 6, S'/255 <= 1, f <= 1:

      V' :  dV' = e + 510 u                          V is a selection (error e); one sum V + dv of magnitude <= 510; the clamp is
                                                     1-Lipschitz
      S  :  dS  = (255 / V) (1 + m/V) e + 3 u S      S = 255 (1 - m/V): |dS/dm| = 255 / V, |dS/dV| = 255 m / V^2; roundings: the
                                                     difference D, the product 255 D, the quotient
      S' :  dS' = dS + 510 u                         one sum of magnitude <= 510, clamp
      s = S'/255 :  ds' = dS' / 255 + u              one quotient <= 1
      H  :  dH  = 60 e / D + 480 u                   H = base + 30 num / D with num, D differences of two of (r, g, b): the three
                                                     partial derivatives sum to 60 / D in absolute value; roundings: num and D
                                                     (30 u each after the scaling), product and quotient (30 u each), the sum with
                                                     base and the + 180 (180 u each)
      h  :  dh' = (dH + 360 u + 180 u) / 30 + 6 u = 2 e / D + 40 u      the sum H + dh, a + 180 wrap (the - 180 one is exact), the
                                                     quotient h <= 6; floor and f = h - floor(h) are exact
      p, q, t, V' :  dgrey = dV' + V' (s dh' + ds') + 4 u V'           every output is V' (1 - k s) with k in {0, 1, f, 1 - f}:
                                                     |d/dV'| <= 1, |d/ds| <= V', |d/df| = V' s; at most 4 roundings (1 - f, its
                                                     product with s, 1 - that, the product with V'), each <= u V'
      out = grey sc + sh :  |sc| (dgrey + 255 u) + u |out|

    21 roundings after the blend's 13.  The transform is continuous across its case boundaries (the three hue branches agree where
    two channels tie, H = 0 and H = 180 give one colour, neighbouring sectors agree at f = 0), so a float32 run that takes another
    branch than the float64 one stays inside the same first-order bound.  Fused multiply-adds only remove roundings.
    V' s / D is evaluated as the quotient it is, so the hue term is 2 e V' S' / (255 D): with ds = 0 it is 2 e V'/V and with
    ds = dv = 0 the whole bound has no 1 / D and no 1 / V left (D = 0 has S' = 0: the term is 0, and V = 0 has V' = 0).  Where
    ds > 0 at D = 0, or dv > 0 at V = 0, the bound is infinite: the transform is discontinuous there.  Second-order terms are
    (e / D) of the hue term: 2.5e-5 of it at D = 8.
    In the well-conditioned region (V' ~ V, S' ~ S) this is about (13 + 26 + 26) u 255 from the entry error plus up to 55 u 255 of
    roundings: 1.8e-3 grey levels at most, 4e-4 / std after Normalize."""
    grey = np.asarray(grey, dtype=np.float64)
    B, C = grey.shape[:2]
    assert C == 3
    sc, _ = R.constants(3, mean, std)
    asc = np.abs(sc)[:, None, None]
    tol = np.empty_like(grey)
    for b, (apply, dh, ds, dv) in enumerate(np.asarray(color, dtype=np.int64)):
        if not apply:
            tol[b] = R.image_tolerance(normalize(grey[b:b + 1], mean, std), mean, std)[0]
            continue
        V, m = grey[b].max(0), grey[b].min(0)
        D = V - m
        with np.errstate(divide='ignore', invalid='ignore'):
            S = np.where(V > 0, 255.0 * D / V, 0.0)
            V2 = np.clip(V + float(dv), 0.0, 255.0)
            S2 = np.clip(S + float(ds), 0.0, 255.0)
            s = S2 / 255.0
            s_over_D = np.where(S2 > 0, s / D, 0.0)                          # inf at D = 0 with S' > 0
            d_V2 = E_IN + 510.0 * U
            d_S = np.where(V > 0, (255.0 / V) * (1.0 + m / V), np.inf) * E_IN + 3.0 * U * S    # V = 0: times V' below, 0 or inf
            V2_d_s = np.where(V2 > 0, V2 * ((d_S + 510.0 * U) / 255.0 + U), 0.0)
            V2_s_d_h = np.where(V2 > 0, V2 * (s_over_D * 2.0 * E_IN + s * 40.0 * U), 0.0)
        d_grey = d_V2 + V2_s_d_h + V2_d_s + 4.0 * U * V2
        out = normalize(shift_blend(grey[b:b + 1], [[apply, dh, ds, dv]]), mean, std)[0]
        tol[b] = asc * (d_grey + 255.0 * U)[None] + U * np.abs(out)
    return tol
