// Cross-entropy over NCHW-planar logits (the caller side of the hot path: nn.CrossEntropyLoss(ignore_index)
// as the training scripts use it), plus the argmax / confusion-matrix pass of the evaluator.
// The planar kernels are instances of the class-plane sweep of losssweep.h (lane layout, labels, validity rule, reductions).
// forward: online log-sum-exp over the C planes -> per-pixel lse (saved), sum of losses + valid count (f64 atomics)
// backward: dlogits[c] = (exp(l_c - lse) - [c == t]) * grad_out / count, recomputed from the saved lse
// ce_fwd_ex / ce_bwd_ex: the same with class weights and label smoothing, per-block partial rows instead of the atomics
#include "headgeom.h"

// The two register kernels of the fused head read CPV channels of a pixel when its pitch holds them; a narrower pitch (C <= 16 with
// ldl = round_up(C, 8)) takes the instance that skips the class groups past C.  Inside TSS_WITH_CLASS_REGS.
#define TSS_WITH_ROW_GUARD(cond, ...)                         \
  do {                                                        \
    if (cond) { constexpr bool GUARDV = true; __VA_ARGS__; }  \
    else { constexpr bool GUARDV = false; __VA_ARGS__; }      \
  } while (0)

namespace {

template <typename T>
__global__ __launch_bounds__(NT) void ce_fwd_kernel(const T* logits, const long long* target, float* lse_out,
                                                    double* acc /*[2]: loss sum, valid count*/, long B, int C,
                                                    long HW, int ignore_index) {
  double lsum = 0.0, lcnt = 0.0;
  for (lsw::Groups g(B, HW); g.more(); g.next()) {
    const long b = g.b(), off = g.off();
    int tv[8];
    float l[8], lt[8];
    lsw::load_labels(target + b * HW + off, C, ignore_index, 1, tv);
    lsw::lse8<true>(logits + b * C * HW + off, C, HW, tv, l, lt);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (tv[j] >= 0) { lsum += (double)(l[j] - lt[j]); lcnt += 1.0; }
    V8<float>::store(lse_out + b * HW + off, l);
  }
  if (lsw::block_sum2(lsum, lcnt)) {
    atomicAdd(acc, lsum);
    atomicAdd(acc + 1, lcnt);
  }
}

__global__ void ce_finalize_kernel(const double* acc, float* loss, float* inv_count) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const double n = acc[1];
    *loss = (float)(acc[0] / n);          // n == 0 -> nan, like torch
    *inv_count = n > 0.0 ? (float)(1.0 / n) : 0.f;
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void ce_bwd_kernel(const T* logits, const long long* target, const float* lse,
                                                    const float* inv_count, const float* grad_out, T* dlogits,
                                                    long B, int C, long HW, int ignore_index) {
  const float gs = (*inv_count) * (grad_out ? *grad_out : 1.f);
  for (lsw::Groups g(B, HW); g.more(); g.next()) {
    const long b = g.b(), off = g.off();
    int tv[8];
    float l[8], w[8];
    lsw::load_labels(target + b * HW + off, C, 0, 0, tv);
    V8<float>::load(lse + b * HW + off, l);
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = lsw::counts(tv[j], ignore_index) ? gs : 0.f;
    lsw::grad8<false>(logits + b * C * HW + off, dlogits + b * C * HW + off, C, HW, tv, l, w);
  }
}

// Class weights w[C] (nullptr: all ones) and label smoothing eps, torch's semantics; the kernels above stay as they are for the
// plain loss.  With W = sum_c w_c and, per valid pixel, s = (1 - eps) w_t + eps W / C:
//   loss = [ (1 - eps) sum w_t (lse - x_t) + eps / C sum sum_c w_c (lse - x_c) ] / den,  den = sum w_t  (sums over the valid pixels)
//   dx_c = ( s p_c - (1 - eps) w_t [c == t] - eps w_c / C ) / den
// The block sums go to a row of the block's own ([grid][2] f64, ce_finalize_rows_kernel<true> adds them in a fixed order): no atomics.
__device__ __forceinline__ float class_weight_sum(const float* cw, int C) {
  if (!cw) return (float)C;
  float W = 0.f;
  for (int c = 0; c < C; ++c) W += cw[c];
  return W;
}

template <typename T, bool SMOOTH>
__global__ __launch_bounds__(NT) void ce_fwd_ex_kernel(const T* logits, const long long* target, const float* cw, float eps,
                                                       float* lse_out, double* rows /*[grid][2]: loss sum, weight sum*/, long B,
                                                       int C, long HW, int ignore_index) {
  const float W = SMOOTH ? class_weight_sum(cw, C) : 0.f, eC = eps / (float)C, om = 1.f - eps;
  double lsum = 0.0, lcnt = 0.0;
  for (lsw::Groups g(B, HW); g.more(); g.next()) {
    const long b = g.b(), off = g.off();
    int tv[8];
    float l[8], lt[8], xw[8];
    lsw::load_labels(target + b * HW + off, C, ignore_index, 1, tv);
    lsw::lse8_weighted<SMOOTH>(logits + b * C * HW + off, C, HW, cw, tv, l, lt, xw);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (tv[j] >= 0) {
        const float wt = cw ? cw[tv[j]] : 1.f;
        float term = wt * (l[j] - lt[j]);
        if (SMOOTH) term = om * term + eC * (W * l[j] - xw[j]);
        lsum += (double)term;
        lcnt += (double)wt;
      }
    V8<float>::store(lse_out + b * HW + off, l);
  }
  if (lsw::block_sum2(lsum, lcnt)) {
    rows[2 * (long)blockIdx.x] = lsum;
    rows[2 * (long)blockIdx.x + 1] = lcnt;
  }
}

template <typename T, bool SMOOTH>
__global__ __launch_bounds__(NT) void ce_bwd_ex_kernel(const T* logits, const long long* target, const float* cw, float eps,
                                                       const float* lse, const float* inv_count, const float* grad_out, T* dlogits,
                                                       long B, int C, long HW, int ignore_index) {
  const float gs = (*inv_count) * (grad_out ? *grad_out : 1.f);
  const float om = (1.f - eps) * gs, uW = SMOOTH ? eps / (float)C * gs : 0.f, sW = SMOOTH ? uW * class_weight_sum(cw, C) : 0.f;
  for (lsw::Groups g(B, HW); g.more(); g.next()) {
    const long b = g.b(), off = g.off();
    int tv[8];
    float l[8], s[8], a[8], u[8];
    lsw::load_labels(target + b * HW + off, C, 0, 0, tv);
    V8<float>::load(lse + b * HW + off, l);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool ok = lsw::counts(tv[j], ignore_index);
      const float wt = ok ? (cw ? cw[tv[j]] : 1.f) : 0.f;
      a[j] = om * wt;
      u[j] = ok ? uW : 0.f;
      s[j] = ok ? a[j] + sW : 0.f;
    }
    lsw::grad8_weighted<SMOOTH>(logits + b * C * HW + off, dlogits + b * C * HW + off, C, HW, cw, tv, l, s, a, u);
  }
}

// ------------------------------------------------------------------------------------------------------------
// Fused decoder head + loss: cross-entropy of the x`scale` bilinearly upsampled logits
// computed straight from the LOW-RES NHWC logits, loss AND gradient in ONE pass.  The (B, C, H, W) full-resolution
// logits -- 318.8 M elements at 8x1024x2048, the largest tensor of the step -- and their gradient never exist: the
// unfused path moves ~3.8 GB for them (upsample, loss, loss backward, two-pass upsample backward: 1.04 ms of a
// 10 ms step), this kernel reads the target once (134 MB) and is bound by the 19 exponentials per pixel.
//
// The mean reduction makes the gradient linear in one unknown scalar (1 / #valid pixels, times grad_out), so the
// forward pass accumulates the UNSCALED low-res gradient and backward is a scale + cast of 6 M elements.
//
// Block layout, workspace layout and the flush protocol: headgeom.h.  Here: the lane keeps the two horizontally interpolated low-res
// rows aA[c], aB[c] in registers, a logit is ONE FMA, z_c = l0y*aA[c] + l1y*aB[c]; softmax, loss and dz_c = (p_c - [t == c]) stay in
// registers; dz is accumulated into gA[c] += l0y*dz_c, gB[c] += l1y*dz_c and a finished low-res row is flushed into the block's own
// tile.  (Round 2 added the rows with f32 global atomics into a zero-filled buffer: last-bit differences from run to run that a
// train step amplifies.)

// MODE 0: mean cross-entropy (loss rows + unscaled gradient tiles).  MODE 1: the per-pixel cross-entropy only, written to `pix`
// ([B][H][W] f32, 0 for ignored pixels) -- the input of the OHEM selection (TSS/losses/ohem_loss.py:11-12 without the 318.8 M-element
// logits).  MODE 2: gradient tiles of a WEIGHTED sum of per-pixel losses, the weight of a pixel derived from its stored loss and
// the selection parameters `sel` = [mode, cut, weight of l > cut, weight of l == cut] (tss_ohem_select): OHEM's backward.
// MODE 3: MODE 0 with class weights `cw` ([C] f32, nullptr: all ones): the pixel weight is w_t, the count row holds sum w_t.
// MODE 4: MODE 3 with label smoothing `eps`: the softmax half carries s = (1 - eps) w_t + eps W / C, the one-hot half (1 - eps) w_t,
// and the uniform part eps w_c / C of the target distribution enters Hh at flush time, once per low-res row, scaled by the sum
// of the row weights of the valid pixels seen (nA, nB: one scalar per row buffer).  MODE 0 / 1 / 2 do not read cw and eps.
// GUARD: the instance for a pitch below CP (ldl < CP, TSS_WITH_ROW_GUARD): its load_row skips the 4-channel groups that start at or
// past C, the contract of headgeom.h's load_row, so that a pixel's reads end inside its pitch.  The instances for ldl >= CP read all
// CP channels of a pixel (inside the pitch) and are the kernels they always were.
template <typename T, int CP, int MODE, bool GUARD>
__global__ __launch_bounds__(NT, (CP <= 20 ? 3 : 2)) void upsample_ce_onepass_kernel(const T* low, long ldl, const long long* target,
                                                                 float* tiles, double* lossrows, int B, int C, int h, int w,
                                                                 int H, int W, int ignore_index, const HeadGeom geo,
                                                                 float* pix, const float* sel, const float* cw, float eps) {
  // block set-up, tables and flush of headgeom.h, written out (see "Who uses what" there)
  const int band_rows = geo.band_rows;
  // Hh[k][lane][c]: the one-hot half of the gradient, sum over the rows seen so far of (row weight) * [target == c], kept
  // per low-res row (k = buffer of row rA / rB).  The softmax half lives in registers (gA, gB); the two meet at flush time.
  // The kernel is VALU-bound (SQ_ACTIVE_INST_VALU = 89 % of the SIMD cycles): a compare + select per class for the one-hot
  // term and for the target logit was 84 of the 332 vector instructions per pixel; this way it is two LDS updates, and the
  // target logits are recovered per low-res row as sum_c a[c] * Hh[c] (same products, summed in a different order).
  __shared__ __align__(16) float Hh[2][NT * CP];
  __shared__ int Li0[NT], Li1[NT], Wlo[MAXCELL], Whi[MAXCELL];
  __shared__ float Ll1[NT];
  __shared__ float Wt[WTAB];                          // gather weights [cell][lane - Wlo[cell]] (fixed for the block)
  __shared__ double red[2][NT / 64];
  __shared__ __align__(16) float Cw[CP];              // MODE 3 / 4: the class weights, 0 for the padding classes
  __shared__ float Nn[2][NT];                         // MODE 4: per row buffer and lane, the sum of the row weights of the valid pixels
  const int tid = threadIdx.x;
  if (MODE >= 3 && tid < CP) Cw[tid] = tid < C ? (cw ? cw[tid] : 1.f) : 0.f;
  if (MODE == 4) { Nn[0][tid] = 0.f; Nn[1][tid] = 0.f; }
  const int nstrip = geo.nstrip, nband = geo.nband;
  float* const tile = tiles + (long)blockIdx.x * geo.tile_rows * geo.tile_cells * CP;
  int bid = blockIdx.x;
  const int strip = bid % nstrip; bid /= nstrip;
  const int band = bid % nband;
  const long b = bid / nband;
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  const int x = strip * NT + tid;
  const bool xin = x < W;
  const Tap tx = ac_tap(sx, xin ? x : W - 1, w);
  // the strip's cells and the band's rows: head_strip_cells and head_band, the gather's expressions, written out like the rest
  const int cx0 = ac_tap(sx, strip * NT, w).i0;                     // first low-res column this strip touches
  const int xl = (strip * NT + NT - 1 < W) ? strip * NT + NT - 1 : W - 1;
  const int ncell = ac_tap(sx, xl, w).i1 - cx0 + 1;                 // <= NT + 2 for W >= w (host-checked)
  const int ya = band * band_rows;
  const int yb = ya + band_rows < H ? ya + band_rows : H;
  Li0[tid] = xin ? tx.i0 - cx0 : -1;      // lanes past the image edge match no cell
  Li1[tid] = xin ? tx.i1 - cx0 : -1;
  Ll1[tid] = tx.l1;
  // widest window of lanes whose taps can include one low-res column: uniform bound from the scale
  const int maxwin = sx > 0.f ? (int)(2.f / sx) + 6 : NT;
  const bool wtab = (long)ncell * maxwin <= WTAB;
  for (int cell = tid; cell < ncell; cell += NT) {   // lanes of this strip whose taps can include low-res column cx0 + cell
    int lo, hi;
    ac_window(sx, cx0 + cell, W, &lo, &hi);
    lo -= strip * NT; hi -= strip * NT;
    lo = lo < 0 ? 0 : lo;
    hi = hi > NT - 1 ? NT - 1 : hi;
    if (wtab && hi - lo + 1 > maxwin) hi = lo + maxwin - 1;        // cannot happen (conservative bound); keeps the table safe
    Wlo[cell] = lo;
    Whi[cell] = hi;
  }
#pragma unroll
  for (int c4 = 0; c4 < CP; c4 += 4) {
    *reinterpret_cast<float4*>(&Hh[0][tid * CP + c4]) = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(&Hh[1][tid * CP + c4]) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  if (wtab) {
    for (int i = tid; i < ncell * maxwin; i += NT) {
      const int cell = i / maxwin, k = i - cell * maxwin;
      const int l = Wlo[cell] + k;
      float wgt = 0.f;
      if (l <= Whi[cell]) { const float l1 = Ll1[l]; wgt = (Li0[l] == cell ? 1.f - l1 : 0.f) + (Li1[l] == cell ? l1 : 0.f); }
      Wt[i] = wgt;
    }
  }

  int rA = ac_tap(sy, ya, h).i0;
  int rB = rA + (rA < h - 1 ? 1 : 0);
  const int r_first = rA;
  float aA[CP], aB[CP], gA[CP], gB[CP];
  auto load_row = [&](int r, float* a) {   // a[c] = l0x * L[r][i0x][c] + l1x * L[r][i1x][c]
    const T* p0 = low + ((b * h + r) * (long)w + tx.i0) * ldl;
    const T* p1 = low + ((b * h + r) * (long)w + tx.i1) * ldl;
#pragma unroll
    for (int c4 = 0; c4 < CP; c4 += 4) {
      float u[4], v[4];
      if (!GUARD || c4 < C) {                // uniform
        V4<T>::load(p0 + c4, u);
        V4<T>::load(p1 + c4, v);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) u[q] = v[q] = 0.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) a[c4 + q] = (c4 + q < C) ? (tx.l0 * u[q] + tx.l1 * v[q]) * LOG2E : -TSS_INF;
    }
  };
  const float eC = MODE == 4 ? eps / (float)C : 0.f;
  float lsum = 0.f, lcnt = 0.f;     // loss sum in base-2 units (the rows carry logits * log2(e): one v_exp per class, no multiply)
  // finished low-res row r (buffer k): the lane's gradient g[] - Hh[k][] is parked in Hh[k] (plain stores), then one thread
  // per (cell, class) gathers the <= ~2*scale+4 lanes whose column taps include that cell and adds the sum to dlow; the
  // lane's target logits of the row leave the loss sum.  (LDS float atomics for the scatter were measured at ~180 cycles
  // per wave instruction: 550 us of a 790 us kernel.)
  auto flush_row = [&](int r, int k, const float* g, const float* a) {
    float* G = Hh[k];
    float zt = 0.f, nk = 0.f;
    if (MODE == 4) { nk = Nn[k][tid] * eC; Nn[k][tid] = 0.f; }      // eps / C * the buffer's row-weight sum
#pragma unroll
    for (int c4 = 0; c4 < CP; c4 += 4) {
      const float4 hv = *reinterpret_cast<const float4*>(G + tid * CP + c4);
      float hq[4] = {hv.x, hv.y, hv.z, hv.w};
      if (MODE == 4) {                                 // the uniform part of the smoothed target; Cw = 0 keeps the padding classes out
        const float4 wv = *reinterpret_cast<const float4*>(Cw + c4);
        hq[0] += nk * wv.x; hq[1] += nk * wv.y; hq[2] += nk * wv.z; hq[3] += nk * wv.w;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) if (c4 + q < C) zt += a[c4 + q] * hq[q];     // padding classes: a = -inf, Hh = 0
      *reinterpret_cast<float4*>(G + tid * CP + c4) = make_float4(g[c4] - hq[0], g[c4 + 1] - hq[1], g[c4 + 2] - hq[2], g[c4 + 3] - hq[3]);
    }
    lsum -= zt;
    __syncthreads();
    float* drow = tile + (long)(r - r_first) * geo.tile_cells * CP;
    for (int i = tid; i < ncell * CP; i += NT) {
      const int cell = i / CP, c = i - cell * CP;
      const int llo = Wlo[cell], lhi = Whi[cell];
      float sum = 0.f;
      if (wtab) {
        const float* wt = Wt + cell * maxwin - llo;
        for (int l = llo; l <= lhi; ++l) sum += wt[l] * G[l * CP + c];
      } else {
        for (int l = llo; l <= lhi; ++l) {
          const float l1 = Ll1[l];
          const float wgt = (Li0[l] == cell ? 1.f - l1 : 0.f) + (Li1[l] == cell ? l1 : 0.f);
          sum += wgt * G[l * CP + c];
        }
      }
      drow[i] = sum;                       // [cell][c]: every element of the block's footprint, exactly once
    }
    __syncthreads();
#pragma unroll
    for (int c4 = 0; c4 < CP; c4 += 4) *reinterpret_cast<float4*>(G + tid * CP + c4) = make_float4(0.f, 0.f, 0.f, 0.f);
  };

 int kA = 0;                                  // Hh[kA] belongs to row rA, Hh[kA ^ 1] to row rB
  load_row(rA, aA);
  load_row(rB, aB);
#pragma unroll
  for (int c = 0; c < CP; ++c) { gA[c] = 0.f; gB[c] = 0.f; }
  __syncthreads();

  const long long* trow = target + (b * H + ya) * (long)W + (xin ? x : 0);
  long long tnext = *trow;
  float sel_cut = 0.f, sel_gt = 0.f, sel_eq = 0.f;
  if (MODE == 2) { sel_cut = sel[1]; sel_gt = sel[2]; sel_eq = sel[0] != 0.f ? 0.f : sel[3]; }
  float om = 1.f, sW = 0.f;                                     // MODE 4: 1 - eps, eps W / C
  if (MODE == 4) {                                              // uniform: scalar loads, scalar registers
    om = 1.f - eps;
    sW = eC * class_weight_sum(cw, C);
  }
  float* prow = (MODE != 0) ? pix + (b * H + ya) * (long)W + (xin ? x : 0) : nullptr;
  for (int y = ya; y < yb; ++y) {
    const long long t = tnext;
    if (y + 1 < yb) tnext = trow[(long)(y + 1 - ya) * W];      // next row's target under this row's arithmetic
    const Tap ty = ac_tap(sy, y, h);                           // uniform over the block
    if (ty.i0 != rA) {                                         // row tap advanced (by exactly one: H >= h)
      if (MODE != 1) flush_row(rA, kA, gA, aA);
      kA ^= 1;
      rA = rB;
      rB = rA + (rA < h - 1 ? 1 : 0);
#pragma unroll
      for (int c = 0; c < CP; ++c) { aA[c] = aB[c]; gA[c] = gB[c]; gB[c] = 0.f; }
      load_row(rB, aB);
    }
    float z[CP];
    float m = -TSS_INF, zt = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      z[c] = (c < C) ? ty.l0 * aA[c] + ty.l1 * aB[c] : -TSS_INF;
      m = fmaxf(m, z[c]);
      if (MODE == 1) zt = (t == (long long)c) ? z[c] : zt;    // the target's logit (log2 units): one select per class, this mode only
    }
    const bool valid = xin && t != ignore_index && t >= 0 && t < C;
    float ssum = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      z[c] = __builtin_amdgcn_exp2f(z[c] - m);          // e_c (0 for the padding classes)
      ssum += z[c];
    }
    if (MODE == 1) {      // per-pixel loss in nats, >= 0 (rounding may give -1e-7), 0 for ignored pixels; nothing else in this mode
      const float d = ((m - zt) + __builtin_amdgcn_logf(ssum)) * 0.69314718055994530942f;
      if (xin) prow[(long)(y - ya) * W] = valid ? fmaxf(d, 0.f) : 0.f;
      continue;
    }
    float wpx = 1.f;      // weight of this pixel's loss in the sum (MODE 2: OHEM's selection)
    if (MODE == 2) {
      const float pl = xin ? prow[(long)(y - ya) * W] : 0.f;
      wpx = pl > sel_cut ? sel_gt : (pl == sel_cut ? sel_eq : 0.f);
    }
    if (MODE >= 3) {      // class weights (and smoothing): wsm scales the softmax half and the lse, wpx the one-hot half
      if (valid) {
        const float wt = Cw[(int)t];
        float wsm = wt;
        wpx = wt;
        if (MODE == 4) { wpx = om * wt; wsm = wpx + sW; Nn[kA][tid] += ty.l0; Nn[kA ^ 1][tid] += ty.l1; }
        lsum += wsm * (m + __builtin_amdgcn_logf(ssum));      // log2
        lcnt += wt;
        Hh[kA][tid * CP + (int)t] += ty.l0 * wpx;
        Hh[kA ^ 1][tid * CP + (int)t] += ty.l1 * wpx;
        wpx = wsm;
      }
    } else if (valid) {
      lsum += m + __builtin_amdgcn_logf(ssum);      // log2
      lcnt += 1.f;
      float* ha = &Hh[kA][tid * CP + (int)t];                 // this lane's own row of the table: no race
      float* hb = &Hh[kA ^ 1][tid * CP + (int)t];
      *ha += ty.l0 * wpx;
      *hb += ty.l1 * wpx;
    }
    const float inv = valid ? __builtin_amdgcn_rcpf(ssum) * wpx : 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const float pz = z[c] * inv;
      gA[c] += ty.l0 * pz;
      gB[c] += ty.l1 * pz;
    }
  }
  if (MODE == 1) return;
  flush_row(rA, kA, gA, aA);
  if (rB != rA) flush_row(rB, kA ^ 1, gB, aB);
  else {   // the band ended on the last low-res row (rB == rA): the l1 weights are zero there, nothing to flush
  }
  if (MODE == 2) return;

  double ds = wave_sum((double)lsum * 0.69314718055994530942), dc = wave_sum((double)lcnt);   // back to nats
  const int wave = tid >> 6;
  if ((tid & 63) == 0) { red[0][wave] = ds; red[1][wave] = dc; }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, c = 0.0;
    for (int wv = 0; wv < NT / 64; ++wv) { a += red[0][wv]; c += red[1][wv]; }
    lossrows[2 * (long)blockIdx.x] = a;
    lossrows[2 * (long)blockIdx.x + 1] = c;
  }
}

template <typename T, int CP>
__global__ __launch_bounds__(NT) void upsample_ce_gather_kernel(const float* tiles, const float* inv_count, const float* grad_out,
                                                                T* dlow, long ldl, int B, int h, int w, int H, int W,
                                                                const HeadGeom geo) {
  head_gather<T, CP>(tiles, inv_count, grad_out, dlow, ldl, B, h, w, H, W, geo);
}

// argmax over class planes (lowest index wins ties, like torch.argmax) + confusion matrix [C][C] (rows = truth)
template <typename T>
__global__ __launch_bounds__(NT) void argmax_confusion_kernel(const T* logits, const long long* target,
                                                              unsigned char* pred_out, unsigned long long* cm,
                                                              long B, int C, long HW, int ignore_index) {
  extern __shared__ unsigned int scm[];  // [C*C]
  for (int i = threadIdx.x; i < C * C; i += blockDim.x) scm[i] = 0u;
  __syncthreads();
  for (lsw::Groups g(B, HW); g.more(); g.next()) {
    const long b = g.b(), off = g.off();
    float best[8];
    int arg[8], tv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { best[j] = -INFINITY; arg[j] = 0; }
    for (int c = 0; c < C; ++c) {
      float v[8];
      V8<T>::load(logits + (b * C + c) * HW + off, v);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (v[j] > best[j] || (c == 0)) { best[j] = v[j]; arg[j] = c; }
    }
    const bool score = cm && target;
    if (score) lsw::load_labels(target + b * HW + off, C, ignore_index, 1, tv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (pred_out) pred_out[b * HW + off + j] = (unsigned char)arg[j];
      if (score && tv[j] >= 0) atomicAdd(&scm[tv[j] * C + arg[j]], 1u);
    }
  }
  __syncthreads();
  if (cm)
    for (int i = threadIdx.x; i < C * C; i += blockDim.x)
      if (scm[i]) atomicAdd(cm + i, (unsigned long long)scm[i]);
}

// Fused evaluation head (eval half): argmax over the classes of the bilinearly upsampled logits
// + confusion-matrix update, straight from the low-res NHWC logits.  Same lane / register layout as
// upsample_ce_onepass_kernel (lane = output column, the two horizontally interpolated low-res rows in registers, one
// FMA per logit); lowest class index wins ties like torch.argmax; rows = truth.  GUARD: as in upsample_ce_onepass_kernel.
template <typename T, int CP, bool GUARD>
__global__ __launch_bounds__(NT, 3) void upsample_argmax_kernel(const T* low, long ldl, const long long* target,
                                                                unsigned char* pred_out, unsigned long long* cm, int B,
                                                                int C, int h, int w, int H, int W, int ignore_index,
                                                                int band_rows) {
  extern __shared__ unsigned int scm[];  // [C*C]
  const int tid = threadIdx.x;
  for (int i = tid; i < C * C; i += NT) scm[i] = 0u;
  __syncthreads();
  // head_block and head_taps written out: through the structs the float32 CP = 20 instance takes 130 registers instead of 128 and
  // loses a wave per SIMD (0.126 -> 0.142 ms at 8 x 19 x 128 x 256 -> 1024 x 2048)
  const int nstrip = (W + NT - 1) / NT, nband = (H + band_rows - 1) / band_rows;
  int bid = blockIdx.x;
  const int strip = bid % nstrip; bid /= nstrip;
  const int band = bid % nband;
  const long b = bid / nband;
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  const int x = strip * NT + tid;
  const bool xin = x < W;
  const Tap tx = ac_tap(sx, xin ? x : W - 1, w);
  int ya, yb;
  head_band(band, band_rows, H, &ya, &yb);
  float aA[CP], aB[CP];
  auto load_row = [&](int r, float* a) {
    const T* p0 = low + ((b * h + r) * (long)w + tx.i0) * ldl;
    const T* p1 = low + ((b * h + r) * (long)w + tx.i1) * ldl;
#pragma unroll
    for (int c4 = 0; c4 < CP; c4 += 4) {
      float u[4], v[4];
      if (!GUARD || c4 < C) {                // uniform
        V4<T>::load(p0 + c4, u);
        V4<T>::load(p1 + c4, v);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) u[q] = v[q] = 0.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) a[c4 + q] = (c4 + q < C) ? tx.l0 * u[q] + tx.l1 * v[q] : -TSS_INF;
    }
  };
  int rA = ac_tap(sy, ya, h).i0;
  int rB = rA + (rA < h - 1 ? 1 : 0);
  load_row(rA, aA);
  load_row(rB, aB);
  for (int y = ya; y < yb; ++y) {
    const Tap ty = ac_tap(sy, y, h);
    if (ty.i0 != rA) {
      rA = rB;
      rB = rA + (rA < h - 1 ? 1 : 0);
#pragma unroll
      for (int c = 0; c < CP; ++c) aA[c] = aB[c];
      load_row(rB, aB);
    }
    float best = -TSS_INF;
    int arg = 0;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const float z = ty.l0 * aA[c] + ty.l1 * aB[c];
      if (c < C && (z > best || c == 0)) { best = z; arg = c; }
    }
    if (xin) {
      const long p = (b * H + y) * (long)W + x;
      if (pred_out) pred_out[p] = (unsigned char)arg;
      if (cm && target) {
        const long long t = target[p];
        if (t != ignore_index && t >= 0 && t < C) atomicAdd(&scm[(int)t * C + arg], 1u);
      }
    }
  }
  __syncthreads();
  if (cm)
    for (int i = tid; i < C * C; i += NT)
      if (scm[i]) atomicAdd(cm + i, (unsigned long long)scm[i]);
}

}  // namespace

extern "C" {

int tss_cross_entropy_fwd(const void* logits, const long long* target, float* lse, double* acc /*[2], zeroed*/,
                          float* loss, float* inv_count, long B, int C, long HW, int ignore_index,
                          int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(tss::planar_shape_ok(B, C, HW, true), TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(logits) && tss::aligned16(lse), TSS_ERR_ALIGN);
  const long groups = B * (HW / 8);
  if (groups == 0) return TSS_OK;
  {
    tss::ProfScope prof(TSS_K_CE_FWD, (hipStream_t)stream, (double)B * HW * (C * tss::esz(dtype) + 12.0), 0);
    TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL(ce_fwd_kernel<TT>, dim3(tss::grid_for(groups, NT)), dim3(NT), 0, (hipStream_t)stream, (const TT*)logits,
                                             target, lse, acc, B, C, HW, ignore_index));
  }
  hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, acc, loss, inv_count);
  return tss::check_last("cross_entropy_fwd");
}

int tss_cross_entropy_bwd(const void* logits, const long long* target, const float* lse, const float* inv_count,
                          const float* grad_out, void* dlogits, long B, int C, long HW, int ignore_index,
                          int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(tss::planar_shape_ok(B, C, HW, true), TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(logits) && tss::aligned16(dlogits) && tss::aligned16(lse), TSS_ERR_ALIGN);
  const long groups = B * (HW / 8);
  if (groups == 0) return TSS_OK;
  tss::ProfScope prof(TSS_K_CE_BWD, (hipStream_t)stream, (double)B * HW * (2.0 * C * tss::esz(dtype) + 12.0), 0);
  TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL(ce_bwd_kernel<TT>, dim3(tss::grid_for(groups, NT)), dim3(NT), 0, (hipStream_t)stream, (const TT*)logits,
                                           target, lse, inv_count, grad_out, (TT*)dlogits, B, C, HW, ignore_index));
  return tss::check_last("cross_entropy_bwd");
}

// Rows of the [rows][2] f64 workspace that tss_cross_entropy_fwd_ex writes (one per block of its grid); 0 for shapes it refuses.
long tss_cross_entropy_ex_rows(long B, long HW) {
  if (B <= 0 || HW <= 0 || (HW % 8) != 0) return 0;
  return tss::grid_for(B * (HW / 8), NT);
}

int tss_cross_entropy_fwd_ex(const void* logits, const long long* target, const float* weight /*[C] or null*/, float label_smoothing,
                             float* lse, double* rows /*[tss_cross_entropy_ex_rows][2], not initialised*/, float* loss,
                             float* inv_count, long B, int C, long HW, int ignore_index, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(tss::planar_shape_ok(B, C, HW) && label_smoothing >= 0.f && label_smoothing <= 1.f && rows, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(logits) && tss::aligned16(lse), TSS_ERR_ALIGN);
  const long groups = B * (HW / 8);
  const int grid = tss::grid_for(groups, NT);
  {
    tss::ProfScope prof(TSS_K_CE_FWD, (hipStream_t)stream, (double)B * HW * (C * tss::esz(dtype) + 12.0), 0);
    if (label_smoothing > 0.f)
      TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL((ce_fwd_ex_kernel<TT, true>), dim3(grid), dim3(NT), 0, (hipStream_t)stream, (const TT*)logits,
                                               target, weight, label_smoothing, lse, rows, B, C, HW, ignore_index));
    else
      TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL((ce_fwd_ex_kernel<TT, false>), dim3(grid), dim3(NT), 0, (hipStream_t)stream, (const TT*)logits,
                                               target, weight, 0.f, lse, rows, B, C, HW, ignore_index));
  }
  hipLaunchKernelGGL(ce_finalize_rows_kernel<true>, dim3(1), dim3(NT), 0, (hipStream_t)stream, rows, grid, loss, inv_count);
  return tss::check_last("cross_entropy_fwd_ex");
}

int tss_cross_entropy_bwd_ex(const void* logits, const long long* target, const float* weight, float label_smoothing, const float* lse,
                             const float* inv_count, const float* grad_out, void* dlogits, long B, int C, long HW, int ignore_index,
                             int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(tss::planar_shape_ok(B, C, HW) && label_smoothing >= 0.f && label_smoothing <= 1.f, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(logits) && tss::aligned16(dlogits) && tss::aligned16(lse), TSS_ERR_ALIGN);
  const long groups = B * (HW / 8);
  const int grid = tss::grid_for(groups, NT);
  tss::ProfScope prof(TSS_K_CE_BWD, (hipStream_t)stream, (double)B * HW * (2.0 * C * tss::esz(dtype) + 12.0), 0);
  if (label_smoothing > 0.f)
    TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL((ce_bwd_ex_kernel<TT, true>), dim3(grid), dim3(NT), 0, (hipStream_t)stream, (const TT*)logits,
                                             target, weight, label_smoothing, lse, inv_count, grad_out, (TT*)dlogits, B, C, HW, ignore_index));
  else
    TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL((ce_bwd_ex_kernel<TT, false>), dim3(grid), dim3(NT), 0, (hipStream_t)stream, (const TT*)logits,
                                             target, weight, 0.f, lse, inv_count, grad_out, (TT*)dlogits, B, C, HW, ignore_index));
  return tss::check_last("cross_entropy_bwd_ex");
}

int tss_argmax_confusion(const void* logits, const long long* target, unsigned char* pred,
                         unsigned long long* confusion /*[C*C] accumulated*/, long B, int C, long HW,
                         int ignore_index, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(tss::planar_shape_ok(B, C, HW, true) && C <= 64, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(logits), TSS_ERR_ALIGN);
  const long groups = B * (HW / 8);
  if (groups == 0) return TSS_OK;
  long grid = tss::grid_for(groups, NT);
  if (grid > 1024) grid = 1024;
  tss::ProfScope prof(TSS_K_ARGMAX, (hipStream_t)stream, (double)B * HW * (C * tss::esz(dtype) + 9.0), 0);
  const size_t sh = (size_t)C * C * sizeof(unsigned int);
  TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL(argmax_confusion_kernel<TT>, dim3((int)grid), dim3(NT), sh, (hipStream_t)stream, (const TT*)logits, target,
                                           pred, confusion, B, C, HW, ignore_index));
  return tss::check_last("argmax_confusion");
}

int tss_upsample_argmax_confusion(const void* low, long ldl, const long long* target, unsigned char* pred,
                                  unsigned long long* confusion /*[C*C] accumulated*/, int B, int C, int h, int w,
                                  int H, int W, int ignore_index, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, 24, ldl, h, w, H, W), TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, false);     // the bands of the loss pass; no tiles here
  const long grid = head_blocks(B, geo);
  tss::ProfScope prof(TSS_K_ARGMAX, (hipStream_t)stream, (double)B * h * w * C * tss::esz(dtype) + (double)B * H * W * 9.0, 0);
  const size_t sh = (size_t)C * C * sizeof(unsigned int);
  TSS_WITH_DTYPE(dtype, TSS_WITH_CLASS_REGS(C, TSS_WITH_ROW_GUARD(ldl < CPV,
    hipLaunchKernelGGL((upsample_argmax_kernel<TT, CPV, GUARDV>), dim3((int)grid), dim3(NT), sh, (hipStream_t)stream,
                       (const TT*)low, ldl, target, pred, confusion, B, C, h, w, H, W, ignore_index, geo.band_rows))));
  return tss::check_last("upsample_argmax_confusion");
}

long tss_upsample_ce_ws(int B, int C, int h, int w, int H, int W) { return head_ws_floats(B, C, 24, h, w, H, W, false); }

int tss_upsample_ce_fwd(const void* low, long ldl, const long long* target, float* ws /* tss_upsample_ce_ws floats, not initialised */,
                        float* loss, float* inv_count,
                        int B, int C, int h, int w, int H, int W, int ignore_index, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, 24, ldl, h, w, H, W), TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low) && tss::aligned16(ws), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, false);
  const long grid = head_blocks(B, geo);
  double* lossrows = reinterpret_cast<double*>(ws);
  float* tiles = ws + grid * 4;
  {
    tss::ProfScope prof(TSS_K_UPSAMPLE_CE_FWD, (hipStream_t)stream,
                        (double)B * h * w * C * (tss::esz(dtype) + 8.0) + (double)B * H * W * 8.0, 0);
    TSS_WITH_DTYPE(dtype, TSS_WITH_CLASS_REGS(C, TSS_WITH_ROW_GUARD(ldl < CPV,
      hipLaunchKernelGGL((upsample_ce_onepass_kernel<TT, CPV, 0, GUARDV>), dim3((int)grid), dim3(NT), 0, (hipStream_t)stream,
                         (const TT*)low, ldl, target, tiles, lossrows, B, C, h, w, H, W, ignore_index, geo, nullptr, nullptr, nullptr, 0.f))));
  }
  hipLaunchKernelGGL(ce_finalize_rows_kernel<false>, dim3(1), dim3(NT), 0, (hipStream_t)stream, lossrows, (int)grid, loss, inv_count);
  return tss::check_last("upsample_ce_fwd");
}

// tss_upsample_ce_fwd with class weights (nullptr: all ones) and label smoothing: the MODE 3 (weights) or MODE 4 (smoothing)
// instance of the pass; same workspace, same gather (tss_upsample_ce_bwd), *inv_count = 1 / sum of the valid pixels' weights.
int tss_upsample_ce_fwd_ex(const void* low, long ldl, const long long* target, const float* weight, float label_smoothing, float* ws,
                           float* loss, float* inv_count, int B, int C, int h, int w, int H, int W, int ignore_index, int dtype,
                           void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, 24, ldl, h, w, H, W) && label_smoothing >= 0.f && label_smoothing <= 1.f, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low) && tss::aligned16(ws), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, false);
  const long grid = head_blocks(B, geo);
  double* lossrows = reinterpret_cast<double*>(ws);
  float* tiles = ws + grid * 4;
  {
    tss::ProfScope prof(TSS_K_UPSAMPLE_CE_FWD, (hipStream_t)stream,
                        (double)B * h * w * C * (tss::esz(dtype) + 8.0) + (double)B * H * W * 8.0, 0);
    if (label_smoothing > 0.f)
      TSS_WITH_DTYPE(dtype, TSS_WITH_CLASS_REGS(C, TSS_WITH_ROW_GUARD(ldl < CPV,
        hipLaunchKernelGGL((upsample_ce_onepass_kernel<TT, CPV, 4, GUARDV>), dim3((int)grid), dim3(NT), 0, (hipStream_t)stream, (const TT*)low, ldl,
                           target, tiles, lossrows, B, C, h, w, H, W, ignore_index, geo, nullptr, nullptr, weight, label_smoothing))));
    else
      TSS_WITH_DTYPE(dtype, TSS_WITH_CLASS_REGS(C, TSS_WITH_ROW_GUARD(ldl < CPV,
        hipLaunchKernelGGL((upsample_ce_onepass_kernel<TT, CPV, 3, GUARDV>), dim3((int)grid), dim3(NT), 0, (hipStream_t)stream, (const TT*)low, ldl,
                           target, tiles, lossrows, B, C, h, w, H, W, ignore_index, geo, nullptr, nullptr, weight, 0.f))));
  }
  hipLaunchKernelGGL(ce_finalize_rows_kernel<true>, dim3(1), dim3(NT), 0, (hipStream_t)stream, lossrows, (int)grid, loss, inv_count);
  return tss::check_last("upsample_ce_fwd_ex");
}

// Per-pixel cross-entropy of the upsampled logits ([B][H][W] f32, 0 for ignored pixels), straight from the low-res logits.
int tss_upsample_pixel_ce(const void* low, long ldl, const long long* target, float* pix, int B, int C, int h, int w, int H, int W,
                          int ignore_index, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, 24, ldl, h, w, H, W) && pix, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, false);
  const long grid = head_blocks(B, geo);
  tss::ProfScope prof(TSS_K_UPSAMPLE_CE_FWD, (hipStream_t)stream, (double)B * h * w * C * tss::esz(dtype) + (double)B * H * W * 12.0, 0);
  TSS_WITH_DTYPE(dtype, TSS_WITH_CLASS_REGS(C, TSS_WITH_ROW_GUARD(ldl < CPV,
    hipLaunchKernelGGL((upsample_ce_onepass_kernel<TT, CPV, 1, GUARDV>), dim3((int)grid), dim3(NT), 0, (hipStream_t)stream,
                       (const TT*)low, ldl, target, nullptr, nullptr, B, C, h, w, H, W, ignore_index, geo, pix, nullptr, nullptr, 0.f))));
  return tss::check_last("upsample_pixel_ce");
}

// Gradient tiles of sum_p weight(pix[p]) * CE_p with weight = sel[2] for pix > sel[1], sel[3] for pix == sel[1] (top-n mode only),
// else 0 (sel = the params of tss_ohem_select).  ws as for tss_upsample_ce_fwd; tss_upsample_ce_bwd (inv_count -> 1.0) gathers.
int tss_upsample_ohem_grad(const void* low, long ldl, const long long* target, const float* pix, const float* sel, float* ws,
                           int B, int C, int h, int w, int H, int W, int ignore_index, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, 24, ldl, h, w, H, W) && pix && sel && ws, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low) && tss::aligned16(ws), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, false);
  const long grid = head_blocks(B, geo);
  float* tiles = ws + grid * 4;
  tss::ProfScope prof(TSS_K_UPSAMPLE_CE_FWD, (hipStream_t)stream, (double)B * h * w * C * (tss::esz(dtype) + 8.0) + (double)B * H * W * 12.0, 0);
  TSS_WITH_DTYPE(dtype, TSS_WITH_CLASS_REGS(C, TSS_WITH_ROW_GUARD(ldl < CPV,
    hipLaunchKernelGGL((upsample_ce_onepass_kernel<TT, CPV, 2, GUARDV>), dim3((int)grid), dim3(NT), 0, (hipStream_t)stream,
                       (const TT*)low, ldl, target, tiles, nullptr, B, C, h, w, H, W, ignore_index, geo, const_cast<float*>(pix), sel, nullptr, 0.f))));
  return tss::check_last("upsample_ohem_grad");
}

int tss_upsample_ce_bwd(const float* ws, const float* inv_count, const float* grad_out, void* dlow, long ldl,
                        int B, int C, int h, int w, int H, int W, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, 24, ldl, h, w, H, W), TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(ws) && tss::aligned16(dlow), TSS_ERR_ALIGN);
  const long n = (long)B * h * w * ldl;
  if (n == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, false);
  const float* tiles = ws + head_blocks(B, geo) * 4;
  tss::ProfScope prof(TSS_K_UPSAMPLE_CE_BWD, (hipStream_t)stream, (double)n * (4.0 + tss::esz(dtype)), 0);
  TSS_WITH_DTYPE(dtype, TSS_WITH_CLASS_REGS(C,
    hipLaunchKernelGGL((upsample_ce_gather_kernel<TT, CPV>), dim3(tss::grid_for(n / 8, NT)), dim3(NT), 0, (hipStream_t)stream,
                       tiles, inv_count, grad_out, (TT*)dlow, ldl, B, h, w, H, W, geo)));
  return tss::check_last("upsample_ce_bwd");
}

}  // extern "C"
