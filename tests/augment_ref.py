"""numpy restatement of tssa.augment_batch / tss_augment_batch_u8 (scale -> crop -> flip -> Normalize -> ToTensor on uint8 data),
and the tolerance of the float32 kernel against it.

Sample b has a parameter row (Hs, Ws, oy, ox, flip, 0).  Output pixel (y, x) of a ch x cw crop takes scaled-image pixel
Y = oy + y, X = ox + (cw-1-x if flip else x).

image : bilinear, half-pixel centres, clamped edges (cv2.INTER_LINEAR, F.interpolate(align_corners=False)), integer coordinates:
        n = (2X+1) W - Ws, x0 = floor(n / 2Ws) (a true floor), weight wx = (n - x0 2Ws) / 2Ws of texel x1 = x0 + 1, both indices
        clamped to [0, W-1]; the same vertically.  The four uint8 texels are blended and NOT rounded back to uint8, then
        out = v * sc[c] + sh[c].  Here the weights, the blend and the normalization are float64.
labels: nearest as cv2.INTER_NEAREST, xs = min(floor(X W / Ws), W-1), ys likewise; integers only, values unchanged, int64.

sc / sh are the constants the C entry derives from its float32 mean3 / std3 arguments IN float32: sc = 1 / (255 std),
sh = -mean / std (None: std = 1, mean = 0).  They are part of the interface, so the restatement takes the same float32 values
(widened to float64) and the tolerance below covers the kernel's arithmetic only.
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32 (round to nearest)


def constants(C, mean=None, std=None):
    """(sc, sh) float64 [C], holding the float32 values of tss_augment_batch_u8 / tss_decode_batch_u8."""
    f = np.float32
    sc, sh = np.empty(C, np.float64), np.empty(C, np.float64)
    for c in range(C):
        m = f(mean[c]) if mean is not None else f(0)
        s = f(std[c]) if std is not None else f(1)
        sc[c] = f(1) / (f(255) * s)
        sh[c] = -m / s
    return sc, sh


def linear_taps(coords, n_in, n_scaled):
    """(i0, i1, w1) of the half-pixel bilinear taps of the integer scaled coordinates `coords`: int64, int64, float64."""
    X = np.asarray(coords, dtype=np.int64)
    n = (2 * X + 1) * n_in - n_scaled
    q = np.floor_divide(n, 2 * n_scaled)                 # floors towards -inf: n < 0 at the low edge when upscaling
    w1 = (n - q * 2 * n_scaled).astype(np.float64) / float(2 * n_scaled)
    return np.clip(q, 0, n_in - 1), np.clip(q + 1, 0, n_in - 1), w1


def nearest_index(coords, n_in, n_scaled):
    X = np.asarray(coords, dtype=np.int64)
    return np.minimum(np.floor_divide(X * n_in, n_scaled), n_in - 1)


def sample_bilinear(plane, Ys, Xs, Hs, Ws):
    """float64 [len(Ys), len(Xs)]: the H x W `plane` resized to Hs x Ws, read at scaled rows Ys and columns Xs."""
    p = np.asarray(plane, dtype=np.float64)
    H, W = p.shape
    y0, y1, wy = linear_taps(Ys, H, Hs)
    x0, x1, wx = linear_taps(Xs, W, Ws)
    top = p[y0][:, x0] * (1.0 - wx) + p[y0][:, x1] * wx
    bot = p[y1][:, x0] * (1.0 - wx) + p[y1][:, x1] * wx
    return top * (1.0 - wy)[:, None] + bot * wy[:, None]


def sample_nearest(plane, Ys, Xs, Hs, Ws):
    p = np.asarray(plane)
    H, W = p.shape
    return p[nearest_index(Ys, H, Hs)][:, nearest_index(Xs, W, Ws)]


def augment(image, target, params, crop_size, mean=None, std=None, image_hwc=False):
    """(float64 [B, C, ch, cw] or None, int64 [B, ch, cw] or None) for uint8 image [B,H,W,C] / [B,C,H,W], uint8 target [B,H,W]
    and integer rows params [B, 6]."""
    ch, cw = crop_size
    params = np.asarray(params, dtype=np.int64)
    out_x = out_y = None
    if image is not None:
        img = np.asarray(image)
        if image_hwc:
            img = img.transpose(0, 3, 1, 2)
        B, C = img.shape[:2]
        sc, sh = constants(C, mean, std)
        out_x = np.empty((B, C, ch, cw), np.float64)
    if target is not None:
        tgt = np.asarray(target)
        B = tgt.shape[0]
        out_y = np.empty((B, ch, cw), np.int64)
    for b in range(B):
        Hs, Ws, oy, ox, flip = (int(v) for v in params[b, :5])
        Ys = oy + np.arange(ch)
        Xs = ox + (cw - 1 - np.arange(cw) if flip else np.arange(cw))
        if image is not None:
            for c in range(C):
                out_x[b, c] = sample_bilinear(img[b, c], Ys, Xs, Hs, Ws) * sc[c] + sh[c]
        if target is not None:
            out_y[b] = sample_nearest(tgt[b], Ys, Xs, Hs, Ws)
    return out_x, out_y


def image_tolerance(out, mean=None, std=None):
    """Elementwise bound on |kernel - augment()| for the float32 kernel, shaped like `out` ([B, C, ch, cw], the reference).

    Derived, not tuned (first order in u = 2^-24; every intermediate is a uint8 texel, a convex blend of texels or a partial
    product of one, so its magnitude is at most 255 grey levels, and a relative rounding error u on it moves the output by at
    most u 255 |sc_c|):
      2   the weights wx, wy: numerator and denominator are exact float32 integers (< 2^15), one correctly rounded division
          each; an error u wx in wx moves the row blend by |t01 - t00| wx u <= 255 u, complement included
      2   the complements 1 - wx, 1 - wy
      9   three blends a (1-w) + b w (top row, bottom row, vertical): two products and one sum each
      1   the product v sc_c
     --
     14   roundings on magnitudes <= 255 |sc_c|, plus the final sum v sc_c + sh_c: u |out|.
    So the bound is 14 u 255 |sc_c| + u |out|: 3.7e-6 + u |out| at std 0.225, 8.3e-7 + u |out| without mean / std.  Fused
    multiply-adds only remove roundings.  The texel reads, the indices and the float32 constants sc_c / sh_c are exact on both
    sides; the float64 reference's own error is 1e-9 of this."""
    out = np.asarray(out, dtype=np.float64)
    sc, _ = constants(out.shape[1], mean, std)
    return 14.0 * U * 255.0 * np.abs(sc)[None, :, None, None] + U * np.abs(out)
