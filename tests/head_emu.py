"""numpy f32 emulation of the fused decoder head's register pass (upsample_ce_onepass_kernel of csrc/loss.hip, MODE 0..4, with
upsample_ce_gather_kernel) and of the two arg-max walks (upsample_argmax_kernel; wide_upsample_argmax_kernel's chunks), for
tests/test_exact_bounds.py: one f32 operation per numpy operation, accumulated per lane, per band and per tile in the kernel's order
(rows of a band top to bottom, classes in index order, a gather window lane by lane, the tiles of a cell in (band, strip) order).
exp2 / log2 / the reciprocal of the f32 argument, rounded to f32, stand in for V_EXP_F32 / V_LOG_F32 / V_RCP_F32; products and sums
are rounded separately (no contraction): one of the orders the bounds of tests/exact.py cover.  `defect` injects ONE mistake:

  'edge_lane'      the lanes past the image edge of the last strip count (with column W - 1's label) and match the last cell
  'no_last_flush'  a band's last low-resolution row is not flushed when rB != rA
  'one_tile'       the gather leaves out a cell's tile of the second (neighbouring) strip
  'swap_last_row'  l0 and l1 swapped on the last output row
  'drop_onehot'    the one-hot half of the lane of a 1-lane strip is dropped
  'smooth_once'    the smoothing term eps w_c / C enters once per pixel instead of once per row weight
  'unclamped_i1'   the row tap i1 = i0 + 1 unclamped (the row behind the image; NaN behind the last image)
and for the arg-max: ge=True (>= instead of >), chunk_ge=True (a tie across a chunk boundary goes to the later chunk)."""
import numpy as np

from tests import exact as X

F32 = np.float32
NT = X.HEAD_NT
LOG2E = F32(1.44269504088896340736)
LN2F = F32(0.69314718055994530942)
LN2 = 0.69314718055994530942
NEG = F32(-np.inf)


def _seq_sum(terms, order):
    """f32 sum of terms[..., c] over c in `order`, one addition per class"""
    s = np.zeros(terms.shape[:-1], dtype=F32)
    for c in order:
        s = s + terms[..., c]
    return s


def _nhwc(x, unclamped):
    """[B][h + 1][w][C] f32: the images with the row behind each (the next image's first; NaN behind the last) for 'unclamped_i1'"""
    B, C, h, w = x.shape
    L = np.ascontiguousarray(np.transpose(x.astype(F32), (0, 2, 3, 1)))
    extra = np.full((B, 1, w, C), np.nan, dtype=F32)
    if unclamped:
        extra[:-1, 0] = L[1:, 0]
    return np.concatenate([L, extra], 1)


def ce_pass(x, labels, H, W, mode=0, weight=None, eps=0.0, pix=None, sel=None, grad_out=1.0, ignore_index=255, defect=None,
            class_order=1, coef=None, gamma=0.0, variant=0, alpha=1.0):
    """-> dict(loss, inv_count, dlow [B][C][h][w] f32, pix [B][H][W] f32); x [B][C][h][w] (values exact in f32).
    mode 'focal', 'dice_stats', 'dice_grad': softhead_pass_kernel of csrc/softhead.hip on the same walk (SOFT_MODES below);
    ignore_index None: has_ignore = 0"""
    B, C, h, w = x.shape
    CP = X.head_cp(C)
    geo = X.head_geom(B, C, h, w, H, W)
    L = _nhwc(x, defect == 'unclamped_i1')
    yi0, yi1, yl0, yl1 = X.ac_taps_np(h, H)
    xi0, xi1, xl0, xl1 = X.ac_taps_np(w, W)
    if defect == 'unclamped_i1':
        yi1 = yi0 + 1
    order = list(range(C))[::class_order]
    cw = np.ones(C, dtype=F32) if weight is None else np.asarray(weight, dtype=F32)
    Cw = np.zeros(CP, dtype=F32)
    Cw[:C] = cw
    eps = F32(eps)
    eC = eps / F32(C) if mode == 4 else F32(0)
    om = F32(1) - eps if mode == 4 else F32(1)
    sW = F32(0)
    if mode == 4:
        Wsum = F32(0)
        for c in range(C):
            Wsum = Wsum + cw[c]
        sW = eC * Wsum
    if mode == 2:
        sel = np.asarray(sel, dtype=F32)
        sel_cut, sel_gt, sel_eq = sel[1], sel[2], (F32(0) if sel[0] != 0 else sel[3])
    pix_out = np.zeros((B, H, W), dtype=F32)
    tiles, rows = {}, {}
    lab = np.asarray(labels)
    soft = None
    if mode == 'dice_grad':       # Ca, Cb of the block: coef[c] and coef[24 + c], zeros past C
        coef = np.asarray(coef, dtype=F32)
        Ca, Cb = coef[:CP].copy(), coef[24:24 + CP].copy()
        if defect == 'b_from_a':
            Cb[20:] = coef[20:CP]
        if defect == 'pad_in_S' and CP > C:
            Cb[C:] = Cb[C - 1]
        soft = (Ca, Cb)
    elif mode == 'focal':
        soft = (F32(gamma), variant)
    for b in range(B):
        for band in range(geo['nband']):
            ya, yb = X.head_band(geo, band, H)
            r_first = int(yi0[ya])
            for strip in range(geo['nstrip']):
                xs = strip * NT + np.arange(NT)
                xin = xs < W
                xc = np.where(xin, xs, W - 1)
                live = xin if defect != 'edge_lane' else np.ones(NT, dtype=bool)
                i0x, i1x, l0x, l1x = xi0[xc], xi1[xc], xl0[xc], xl1[xc]
                sc = X.head_strip_cells(w, W, strip)
                cx0, ncell = sc['c0'], sc['ncell']
                Li0 = np.where(live, i0x - cx0, -1)
                Li1 = np.where(live, i1x - cx0, -1)
                win = [X.head_lane_window(w, W, strip, cell) for cell in range(ncell)]
                drop1 = defect == 'drop_onehot' and sc['lanes'] == 1
                tile = np.full((geo['tile_rows'], geo['tile_cells'], CP), np.nan, dtype=F32)
                tiles[(b, band, strip)] = tile

                def load_row(r):
                    a = np.full((NT, CP), NEG, dtype=F32)
                    a[:, :C] = (l0x[:, None] * L[b, r, i0x, :] + l1x[:, None] * L[b, r, i1x, :]) * LOG2E
                    return a

                Hh = [np.zeros((NT, CP), dtype=F32), np.zeros((NT, CP), dtype=F32)]
                Nn = [np.zeros(NT, dtype=F32), np.zeros(NT, dtype=F32)]
                lsum, lcnt = np.zeros(NT, dtype=F32), np.zeros(NT, dtype=F32)

                def flush(r, k, g, a):
                    nonlocal lsum
                    hq = Hh[k].copy()
                    if mode == 4:
                        nk = Nn[k] * eC
                        Nn[k][:] = 0
                        hq = hq + nk[:, None] * Cw[None, :]
                    if mode not in SOFT_MODES:        # the cross-entropy's target-logit term; the soft losses sum theirs per pixel
                        prod = np.zeros((NT, CP), dtype=F32)
                        prod[:, :C] = a[:, :C] * hq[:, :C]
                        lsum = lsum - _seq_sum(prod, range(C))
                    G = g - hq
                    for cell in range(ncell):
                        lo, hi = win[cell]
                        s = np.zeros(CP, dtype=F32)
                        for l in range(lo, hi + 1):
                            wgt = (F32(1) - l1x[l] if Li0[l] == cell else F32(0)) + (l1x[l] if Li1[l] == cell else F32(0))
                            s = s + wgt * G[l]
                        tile[r - r_first, cell] = s
                    Hh[k][:] = 0

                rA = r_first
                rB = rA + (1 if rA < h - 1 else 0)
                kA = 0
                aA, aB = load_row(rA), load_row(rB if defect != 'unclamped_i1' else rA + 1)
                gA, gB = np.zeros((NT, CP), dtype=F32), np.zeros((NT, CP), dtype=F32)
                for y in range(ya, yb):
                    t = lab[b, y, xc if defect == 'edge_lane' else np.where(xin, xs, 0)]
                    if int(yi0[y]) != rA:
                        if mode not in (1, 'dice_stats'):
                            flush(rA, kA, gA, aA)
                        kA ^= 1
                        rA = rB
                        rB = rA + (1 if rA < h - 1 else 0)
                        aA = aB
                        if mode != 'dice_stats':
                            gA, gB = gB, np.zeros((NT, CP), dtype=F32)
                        aB = load_row(rB if defect != 'unclamped_i1' else rA + 1)
                    l0, l1 = yl0[y], yl1[y]
                    if defect == 'swap_last_row' and y == H - 1:
                        l0, l1 = l1, l0
                    z = np.full((NT, CP), F32(0) if defect == 'pad_in_S' else NEG, dtype=F32)
                    with np.errstate(invalid='ignore'):
                        z[:, :C] = l0 * aA[:, :C] + l1 * aB[:, :C]
                        m = z[:, order[0]].copy()
                        for c in order[1:]:
                            m = np.maximum(m, z[:, c])          # fmaxf: the order does not matter
                        e = np.exp2(z - m[:, None]).astype(F32)
                    ssum = _seq_sum(e, order)
                    valid = live & (t >= 0) & (t < C) & ((t != ignore_index) if ignore_index is not None else True)
                    tc = np.where(valid, t, 0).astype(np.int64)
                    lanes = np.nonzero(valid)[0]
                    if mode in SOFT_MODES:
                        if mode == 'dice_stats' and defect == 'edge_N':
                            te = lab[b, y, xc]
                            everyone = (te >= 0) & (te < C) & ((te != ignore_index) if ignore_index is not None else True)
                            cnt_lanes, cnt_t = np.nonzero(everyone)[0], te
                        else:
                            cnt_lanes, cnt_t = lanes, tc
                        with np.errstate(all='ignore'):
                            gA, gB = _soft_pixel(mode, e, z, m, valid, lanes, tc, l0, l1, Hh, kA, gA, gB, lsum, lcnt, soft, defect, cnt_lanes, cnt_t)
                        continue
                    if mode == 1:
                        zt = z[np.arange(NT), tc]
                        d = ((m - zt) + np.log2(ssum).astype(F32)) * LN2F
                        out = np.where(valid, np.fmax(d, F32(0)), F32(0))       # fmaxf: a NaN from a poisoned row comes out as 0
                        pix_out[b, y, xs[xin]] = out[xin]
                        continue
                    wpx = np.ones(NT, dtype=F32)
                    if mode == 2:
                        pl = np.where(xin, np.asarray(pix, dtype=F32)[b, y, np.where(xin, xs, 0)], F32(0))
                        wpx = np.where(pl > sel_cut, sel_gt, np.where(pl == sel_cut, sel_eq, F32(0))).astype(F32)
                    lg = m + np.log2(ssum).astype(F32)
                    if mode >= 3:
                        wt = Cw[tc]
                        wpx = (om * wt).astype(F32) if mode == 4 else wt
                        wsm = wpx + sW if mode == 4 else wt
                        if mode == 4:
                            if defect == 'smooth_once':
                                Nn[kA][lanes] = Nn[kA][lanes] + F32(1)
                            else:
                                Nn[kA][lanes] = Nn[kA][lanes] + l0
                                Nn[kA ^ 1][lanes] = Nn[kA ^ 1][lanes] + l1
                        lsum[lanes] = lsum[lanes] + (wsm * lg)[lanes]
                        lcnt[lanes] = lcnt[lanes] + wt[lanes]
                    else:
                        wsm = wpx
                        lsum[lanes] = lsum[lanes] + lg[lanes]
                        lcnt[lanes] = lcnt[lanes] + F32(1)
                    hl = lanes if not drop1 else lanes[:0]
                    Hh[kA][hl, tc[hl]] = Hh[kA][hl, tc[hl]] + l0 * wpx[hl]
                    Hh[kA ^ 1][hl, tc[hl]] = Hh[kA ^ 1][hl, tc[hl]] + l1 * wpx[hl]
                    inv = np.where(valid, (F32(1) / ssum).astype(F32) * wsm, F32(0)).astype(F32)
                    pz = e * inv[:, None]
                    gA = gA + l0 * pz
                    gB = gB + l1 * pz
                if mode == 1:
                    continue
                if mode == 'dice_stats':      # the block's row: P from the lane sums, I and N from the lane tables, in f64
                    rows[(b, band, strip)] = tuple(q.astype(np.float64).sum(0)[:C] for q in (gA, Hh[0], Hh[1]))
                    continue
                flush(rA, kA, gA, aA)
                if rB != rA and defect != 'no_last_flush':
                    flush(rB, kA ^ 1, gB, aB)
                rows[(b, band, strip)] = (float(np.sum(lsum.astype(np.float64) * (1.0 if mode == 'focal' else LN2))),
                                          float(np.sum(lcnt.astype(np.float64))))
    if mode == 1:
        return dict(pix=pix_out)
    if mode == 'dice_stats':
        return dict(stats=[sum(rows[k][i] for k in sorted(rows)) for i in range(3)])
    if mode == 'focal':           # softhead_focal_finalize_kernel: loss = -alpha sum / n, scale = alpha / n; the gather takes scale
        num, den = sum(rows[k][0] for k in sorted(rows)), sum(rows[k][1] for k in sorted(rows))
        a64 = np.float64(F32(alpha))
        loss = F32(-a64 * num / den) if den > 0 else F32(0)
        inv_count = F32(a64 / den) if den > 0 else F32(0)
    elif mode in (2, 'dice_grad'):
        loss, inv_count = None, F32(1)
    else:
        num = den = 0.0
        for k in sorted(rows):
            num, den = num + rows[k][0], den + rows[k][1]
        loss = F32(num / den) if den > 0 else F32(np.nan)
        inv_count = F32(1.0 / den) if den > 0 else F32(0)
    # the gather: the tiles of a cell in (band, strip) order
    gs = inv_count * F32(grad_out)
    dlow = np.zeros((B, C, h, w), dtype=F32)
    for b in range(B):
        for r in range(h):
            ylo, yhi = X.ac_window(h, H, r)
            for cx in range(w):
                xlo, xhi = X.ac_window(w, W, cx)
                v = np.zeros(CP, dtype=F32)
                for band in range(ylo // geo['band_rows'], yhi // geo['band_rows'] + 1):
                    ya, yb = X.head_band(geo, band, H)
                    r0, r1 = X.head_band_rows(h, H, ya, yb)
                    if r < r0 or r > r1:
                        continue
                    for ns, strip in enumerate(range(xlo // NT, xhi // NT + 1)):
                        sc = X.head_strip_cells(w, W, strip)
                        if cx < sc['c0'] or cx >= sc['c0'] + sc['ncell'] or (defect == 'one_tile' and ns > 0):
                            continue
                        v = v + tiles[(b, band, strip)][r - r0, cx - sc['c0']]
                dlow[b, :, r, cx] = (v * gs)[:C]
    return dict(loss=loss, inv_count=inv_count, dlow=dlow)


SOFT_MODES = ('focal', 'dice_stats', 'dice_grad')


def _soft_pixel(mode, e, z, m, valid, lanes, tc, l0, l1, Hh, kA, gA, gB, lsum, lcnt, soft, defect, cnt_lanes, cnt_t):
    """one output row of softhead_pass_kernel past the exponentials e = exp2(z - m) [NT][CP] (0 for the pad classes): updates the lane
    tables Hh and the lane sums in place and returns (gA, gB).  Defects: focal 'q_one_minus_p', 'no_log1p', 'no_second_term'; the
    Dice ones are prepared by the caller ('b_from_a', 'pad_in_S': the coefficients and the pad logits; 'edge_N': cnt_lanes)"""
    from tests import softloss_emu as SE
    NTn, CP = e.shape
    ar = np.arange(NTn)
    if mode == 'focal':
        gamma, variant = soft
        hot = np.zeros((NTn, CP), dtype=bool)
        hot[lanes, tc[lanes]] = True
        so = _seq_sum(np.where(hot, F32(0), e), range(CP))
        et = np.where(valid, e[ar, tc], F32(0))
        s = so + et
        logs = np.log2(s.astype(np.float64)).astype(F32) * LN2F
        lead = logs * so * (F32(1) / (s - F32(1))).astype(F32)
        lg = logs if defect == 'no_log1p' else np.where(et == 1, np.where(s == 1, so, lead), logs)
        lp = (z[ar, tc] - m) * LN2F - lg
        inv = (F32(1) / s).astype(F32)
        p, q = et * inv, so * inv
        if defect == 'q_one_minus_p':
            q = F32(1) - p
        wq, cf = SE.head_focal_terms(p, q, lp, gamma, variant)
        if defect == 'no_second_term':
            cf = wq
        lsum[lanes] = lsum[lanes] + (wq * lp)[lanes]
        lcnt[lanes] = lcnt[lanes] + F32(1)
        Hh[kA][lanes, tc[lanes]] = Hh[kA][lanes, tc[lanes]] + l0 * cf[lanes]
        Hh[kA ^ 1][lanes, tc[lanes]] = Hh[kA ^ 1][lanes, tc[lanes]] + l1 * cf[lanes]
        pz = e * np.where(valid, cf * inv, F32(0)).astype(F32)[:, None]
        return gA + l0 * pz, gB + l1 * pz
    ssum = _seq_sum(e, range(CP))
    inv = np.where(valid, (F32(1) / ssum).astype(F32), F32(0)).astype(F32)
    p = e * inv[:, None]
    if mode == 'dice_stats':
        Hh[0][lanes, tc[lanes]] = Hh[0][lanes, tc[lanes]] + p[lanes, tc[lanes]]
        Hh[1][cnt_lanes, cnt_t[cnt_lanes]] = Hh[1][cnt_lanes, cnt_t[cnt_lanes]] + F32(1)
        return gA + p, gB
    Ca, Cb = soft
    S = _seq_sum(Cb[None, :] * p, range(CP))
    hotv = Ca[tc] * p[ar, tc]
    S[lanes] = S[lanes] + hotv[lanes]
    Hh[kA][lanes, tc[lanes]] = Hh[kA][lanes, tc[lanes]] - l0 * hotv[lanes]
    Hh[kA ^ 1][lanes, tc[lanes]] = Hh[kA ^ 1][lanes, tc[lanes]] - l1 * hotv[lanes]
    pz = p * (Cb[None, :] - S[:, None])
    return gA + l0 * pz, gB + l1 * pz


def dice_finalize(stats, C, smooth):
    """softhead_dice_finalize_kernel in f64: (coef [64] f32 with a at [0, 24), b at [24, 48), zeros past C; loss f32)"""
    P, I, N = (np.asarray(q, np.float64) for q in stats)
    coef = np.zeros(64, dtype=F32)
    term = np.zeros(C)
    if N.sum() > 0:
        sm = np.float64(F32(smooth))
        den, num = P + N + sm, 2.0 * I + sm
        ok = den > 0
        dd = np.where(ok, den, 1.0)
        term = np.where(ok, 1.0 - num / dd, 1.0)
        coef[:C] = np.where(ok, -2.0 / (C * dd), 0.0)
        coef[24:24 + C] = np.where(ok, num / (C * dd * dd), 0.0)
    return coef, F32(term.sum() / C)


def argmax_walk(x, H, W, class_order=1, ge=False, chunk=None, chunk_ge=False):
    """upsample_argmax_kernel (chunk=None) or wide_upsample_argmax_kernel (chunk=WK: the running best carried from chunk to chunk) in
    f32: [B][H][W] predictions.  class_order=-1 runs the class loop backwards and keeps the lowest index among equal scores (`>=`
    on the way down), the result an order-free kernel must also give"""
    B, C, h, w = x.shape
    L = _nhwc(x, False)
    yi0, yi1, yl0, yl1 = X.ac_taps_np(h, H)
    xi0, xi1, xl0, xl1 = X.ac_taps_np(w, W)
    a = xl0[None, None, :, None] * L[:, :h, xi0, :] + xl1[None, None, :, None] * L[:, :h, xi1, :]         # [B][h][W][C]
    z = yl0[None, :, None, None] * a[:, yi0] + yl1[None, :, None, None] * a[:, yi1]                        # [B][H][W][C]
    best = np.full((B, H, W), NEG, dtype=F32)
    arg = np.zeros((B, H, W), dtype=np.int64)
    for c in (range(C) if class_order == 1 else range(C - 1, -1, -1)):
        zc = z[..., c]
        first = c == (0 if class_order == 1 else C - 1)
        boundary = chunk is not None and chunk_ge and c % chunk == 0
        take = (zc >= best) if (ge or boundary or class_order == -1) else (zc > best)
        take = take | first
        best = np.where(take, zc, best)
        arg = np.where(take, c, arg)
    return arg
