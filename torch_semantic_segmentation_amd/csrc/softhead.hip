// Focal loss and soft Dice loss (softloss.hip's definitions) of the bilinearly upsampled logits, straight from the LOW-RES NHWC logits:
// the fused decoder head of loss.hip for the other two pixel-wise losses.  The (B, C, H, W) logits and their gradient never exist.
//
// Block layout, workspace layout and the flush protocol are those of upsample_ce_onepass_kernel: headgeom.h.  tss_upsample_ce_bwd gathers
// the tiles in a fixed order.  No atomics, no host read-back: capturable, and two runs give the same bits.  A pixel counts iff
// target != ignore_index (has_ignore = 0: no ignore index) and 0 <= target < C.
//
//   focal (C <= 24), one pass: per valid pixel p = p_t, q = sum_{c != t} p_c (summed, not 1 - p), lp = log p_t,
//       w = exp(q^gamma) (variant 0) or q^gamma (variant 1),  coef = w - w'(q) p lp  (w' = gamma q^(gamma-1) w, variant 1: gamma q^(gamma-1);
//       the second term is 0 where q == 0 or gamma == 0),  d(sum_V w lp)/dz_k = -coef (p_k - [k == t]).
//       The block's loss row holds sum w lp and the valid count, the tiles sum coef (p_k - [k == t]), unscaled; the finalize kernel
//       leaves loss = -alpha sum / n and scale = alpha / n (n == 0: both 0), and the gather multiplies by scale * grad_out.
//   focal (24 < C <= 256): tss_upsample_pixel_ce_wide writes ce = -lp per pixel; focal_coef_kernel here turns that array in place into
//       coef (0 for a pixel that does not count) and adds up the loss rows; the MODE 5 instance of wide_ce_kernel (widehead.hip) fills
//       tiles of sum coef (p_k - [k == t]).  On this route p = exp(-ce) and q = 1 - p is formed from the STORED cross-entropy as
//       -expm1(-ce) (no cancellation), not as the sum of the other classes' probabilities: the two agree to the rounding of ce.
//   dice (C <= 24): a statistics pass (per block a row of P_c = sum_V p_c, I_c = sum_V p_c [t == c], N_c = sum_V [t == c]; the dense sum
//       per lane in registers, the two one-hot sums per lane in LDS, the block sum in f64 in a fixed order), a one-block finalize
//       (loss and the 2C coefficients a_c = -2 / (C (U_c + s)), b_c = (2 I_c + s) / (C (U_c + s)^2), U_c = P_c + N_c; all zero when no
//       pixel is valid), and a gradient pass that recomputes the softmax: dz_k = p_k (b_k - S) + [k == t] a_t p_t,
//       S = sum_c b_c p_c + a_t p_t (coefficients in LDS).  tss_upsample_ce_bwd gathers with *inv_count = 1.
#include "headgeom.h"

namespace {

constexpr int WAVES = NT / 64;
constexpr int FIN_NT = 1024;                 // the Dice finalize block: 16 waves, one column of the rows per wave at a time
constexpr int DICE_COEF = 64;                // floats at the head of the Dice workspace: a[24], b[24], padding to 256 bytes
constexpr int CPMAX = 24;
constexpr float LN2F = 0.69314718055994530942f;

enum { SH_FOCAL = 0, SH_DICE_STATS = 1, SH_DICE_GRAD = 2 };

// w and coef = w - w'(q) p lp of one valid pixel (header comment); p, q in [0, 1], lp <= 0
__device__ __forceinline__ void focal_terms(float p, float q, float lp, float gamma, int variant, float* w, float* coef) {
  float qg = 1.f, dqg = 0.f;                                   // q^gamma, gamma q^(gamma-1)
  if (gamma != 0.f) {
    qg = q > 0.f ? exp2f(gamma * __log2f(q)) : 0.f;
    dqg = q > 0.f ? gamma * qg / q : 0.f;
  }
  const float wq = variant == 0 ? __expf(qg) : qg;
  const float dw = variant == 0 ? dqg * wq : dqg;
  *w = wq;
  *coef = wq - dw * p * lp;
}

// rows: SH_FOCAL [nblocks][2] f64 (sum w lp, valid count); SH_DICE_STATS [nblocks][3][C] f64 (P, I, N); SH_DICE_GRAD none.
// coef: SH_DICE_GRAD, a at [0, 24), b at [24, 48), zero past C.  tiles: SH_FOCAL and SH_DICE_GRAD.
template <typename T, int CP, int KIND>
__global__ __launch_bounds__(NT, (CP <= 20 ? 3 : 2)) void softhead_pass_kernel(const T* low, long ldl, const long long* target, float* tiles,
                                                                                double* rows, int C, int h, int w, int H, int W,
                                                                                int ignore_index, int has_ignore, const HeadGeom geo,
                                                                                float gamma, int variant, const float* coef) {
  constexpr bool TILES = KIND != SH_DICE_STATS;
  // Hh[k][lane][c]: SH_FOCAL / SH_DICE_GRAD the one-hot half of the gradient per low-res row buffer; SH_DICE_STATS k = 0: I, k = 1: N per lane
  __shared__ __align__(16) float Hh[2][NT * CP];
  __shared__ GatherLds tabs;
  __shared__ __align__(16) float Ca[CP], Cb[CP];      // SH_DICE_GRAD: the coefficients, 0 for the padding classes
  const int tid = threadIdx.x;
  if (KIND == SH_DICE_GRAD && tid < CP) { Ca[tid] = coef[tid]; Cb[tid] = coef[CPMAX + tid]; }
  float* const tile = TILES ? tiles + (long)blockIdx.x * geo.tile_rows * geo.tile_cells * CP : nullptr;
  const HeadBlock blk = head_block(geo.nstrip, geo.nband, geo.band_rows, H, W);
  const HeadTaps map = head_taps(blk, h, w, H, W);
  const long b = blk.b;
  const int x = blk.x, ya = blk.ya, yb = blk.yb;
  const bool xin = blk.xin;
  const float sy = map.sy;
  const Tap tx = map.tx;
  Gather gt = {};
  if constexpr (TILES) gt = gather_windows(&tabs, blk, map, h, w, W);
#pragma unroll
  for (int c4 = 0; c4 < CP; c4 += 4) {
    *reinterpret_cast<float4*>(&Hh[0][tid * CP + c4]) = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(&Hh[1][tid * CP + c4]) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  if constexpr (TILES) gather_weights(gt);

  int rA = ac_tap(sy, ya, h).i0;
  int rB = rA + (rA < h - 1 ? 1 : 0);
  float aA[CP], aB[CP], gA[CP], gB[CP];      // SH_DICE_STATS: gA holds the lane's sum of p_c, gB is not used
  auto load = [&](int r, float* a) { load_row<CP, true, true>(low, b * h + r, w, ldl, tx, C, a); };
  auto flush_row = [&](int r, int k, const float* g) {
    head_flush_row<CP>(gt, geo, Hh[k], g, r, CP, [](int, float*) {},
                       [&](int tr, int, int, int i, float sum) { tile[(long)tr * geo.tile_cells * CP + i] = sum; });   // [cell][c]
  };

  int kA = 0;                                  // Hh[kA] belongs to row rA, Hh[kA ^ 1] to row rB
  load(rA, aA);
  load(rB, aB);
#pragma unroll
  for (int c = 0; c < CP; ++c) { gA[c] = 0.f; gB[c] = 0.f; }
  __syncthreads();

  const long long* trow = target + (b * H + ya) * (long)W + (xin ? x : 0);
  long long tnext = *trow;
  float lsum = 0.f, lcnt = 0.f;               // per lane over at most 64 rows; f64 from the wave sum on
  for (int y = ya; y < yb; ++y) {
    const long long t = tnext;
    if (y + 1 < yb) tnext = trow[(long)(y + 1 - ya) * W];      // next row's target under this row's arithmetic
    const Tap ty = ac_tap(sy, y, h);                           // uniform over the block
    while (rA < ty.i0) {                                       // row tap advanced (headgeom.h)
      if (TILES) flush_row(rA, kA, gA);
      kA ^= 1;
      rA = rB;
      rB = rA + (rA < h - 1 ? 1 : 0);
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        aA[c] = aB[c];
        if (TILES) { gA[c] = gB[c]; gB[c] = 0.f; }
      }
      load(rB, aB);
    }
    const bool valid = xin && (!has_ignore || t != (long long)ignore_index) && t >= 0 && t < C;
    const int ti = valid ? (int)t : -1;
    float z[CP];
    float m = -TSS_INF, zt = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      z[c] = (c < C) ? ty.l0 * aA[c] + ty.l1 * aB[c] : -TSS_INF;
      m = fmaxf(m, z[c]);
      if (KIND == SH_FOCAL) zt = (ti == c) ? z[c] : zt;        // the target's logit (log2 units)
    }
    if (KIND == SH_FOCAL) {
      float so = 0.f, et = 0.f;                                // sum of exp over the classes != t, the target's exp
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        z[c] = __builtin_amdgcn_exp2f(z[c] - m);               // e_c (0 for the padding classes)
        so += (ti == c) ? 0.f : z[c];
        et = (ti == c) ? z[c] : et;
      }
      float spx = 0.f;                                         // coef / sum of exp: the scale of the softmax half
      if (valid) {
        const float s = so + et;
        // the target holds the maximum: log(1 + so) without the rounding of 1 + so, as log(u) so / (u - 1) with u = fl(1 + so)
        const float lg = (et == 1.f) ? (s == 1.f ? so : __logf(s) * so * __builtin_amdgcn_rcpf(s - 1.f)) : __logf(s);
        const float lp = (zt - m) * LN2F - lg;
        const float inv = __builtin_amdgcn_rcpf(s);
        float wq, cf;
        focal_terms(et * inv, so * inv, lp, gamma, variant, &wq, &cf);
        lsum += wq * lp;
        lcnt += 1.f;
        Hh[kA][tid * CP + ti] += ty.l0 * cf;                   // this lane's own row of the table: no race
        Hh[kA ^ 1][tid * CP + ti] += ty.l1 * cf;
        spx = cf * inv;
      }
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const float pz = z[c] * spx;
        gA[c] += ty.l0 * pz;
        gB[c] += ty.l1 * pz;
      }
    } else {
      float ssum = 0.f;
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        z[c] = __builtin_amdgcn_exp2f(z[c] - m);
        ssum += z[c];
      }
      const float inv = valid ? __builtin_amdgcn_rcpf(ssum) : 0.f;
      float pt = 0.f;
      if (KIND == SH_DICE_STATS) {
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          const float p = z[c] * inv;
          gA[c] += p;
          pt = (ti == c) ? p : pt;
        }
        if (valid) {
          Hh[0][tid * CP + ti] += pt;
          Hh[1][tid * CP + ti] += 1.f;
        }
      } else {
        float S = 0.f;
#pragma unroll
        for (int c4 = 0; c4 < CP; c4 += 4) {
          const float4 bv = *reinterpret_cast<const float4*>(Cb + c4);
          const float bq[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float p = z[c4 + q] * inv;
            z[c4 + q] = p;
            S += bq[q] * p;
            pt = (ti == c4 + q) ? p : pt;
          }
        }
        if (valid) {
          const float hot = Ca[ti] * pt;                       // a_t p_t: the one-hot part of dz, and of S
          S += hot;
          Hh[kA][tid * CP + ti] -= ty.l0 * hot;                // the tile is g - Hh
          Hh[kA ^ 1][tid * CP + ti] -= ty.l1 * hot;
        }
#pragma unroll
        for (int c4 = 0; c4 < CP; c4 += 4) {
          const float4 bv = *reinterpret_cast<const float4*>(Cb + c4);
          const float bq[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float pz = z[c4 + q] * (bq[q] - S);
            gA[c4 + q] += ty.l0 * pz;
            gB[c4 + q] += ty.l1 * pz;
          }
        }
      }
    }
  }

  if (TILES) {
    flush_row(rA, kA, gA);
    if (rB != rA) flush_row(rB, kA ^ 1, gB);     // else the band ended on the last low-res row: the l1 weights are zero there
  }
  const int lane = tid & 63, wave = tid >> 6;
  if (KIND == SH_FOCAL) {
    double ds = (double)lsum, dc = (double)lcnt;
    if (lsw::block_sum2(ds, dc)) {
      rows[2 * (long)blockIdx.x] = ds;
      rows[2 * (long)blockIdx.x + 1] = dc;
    }
  }
  if (KIND == SH_DICE_STATS) {
    double* const row = rows + (long)blockIdx.x * 3 * C;
    // column c of a [lane][CP] table, summed in f64 by one wave: lanes take rows lane, lane + 64, ..., then the butterfly (a fixed order)
    auto colsum = [&](const float* X, int kind) {
      for (int c = wave; c < C; c += WAVES) {
        double s = 0.0;
        for (int l = lane; l < NT; l += 64) s += (double)X[l * CP + c];
        s = wave_sum(s);
        if (lane == 0) row[kind * C + c] = s;
      }
    };
    __syncthreads();
    colsum(Hh[0], 1);
    colsum(Hh[1], 2);
    __syncthreads();
#pragma unroll
    for (int c4 = 0; c4 < CP; c4 += 4)
      *reinterpret_cast<float4*>(&Hh[0][tid * CP + c4]) = make_float4(gA[c4], gA[c4 + 1], gA[c4 + 2], gA[c4 + 3]);
    __syncthreads();
    colsum(Hh[0], 0);
  }
}

// loss = -alpha * sum(rows[.][0]) / n, scale = alpha / n with n = sum(rows[.][1]); n == 0: both 0.  One block, fixed tree.
__global__ __launch_bounds__(NT) void softhead_focal_finalize_kernel(const double* rows, int nrows, float alpha, float* loss, float* scale) {
  double sum, cnt;
  if (lsw::row_sum2(rows, nrows, sum, cnt)) {
    *loss = cnt > 0.0 ? (float)(-(double)alpha * sum / cnt) : 0.f;
    *scale = cnt > 0.0 ? (float)((double)alpha / cnt) : 0.f;
  }
}

// The wide route's planar step, 4 pixels per lane and trip: pix holds the per-pixel cross-entropy ce = -log p_t (>= 0) and leaves as
// coef (0 for a pixel that does not count); the block's row takes sum w lp and the valid count.  q = -expm1(-ce).
__global__ __launch_bounds__(NT) void focal_coef_kernel(float* pix, const long long* target, double* rows, long n, int C, int ignore_index,
                                                        int has_ignore, float gamma, int variant) {
  double lsum = 0.0, lcnt = 0.0;
  const long ngroups = (n + 3) / 4;
  for (long g = (long)blockIdx.x * NT + threadIdx.x; g < ngroups; g += (long)gridDim.x * NT) {
    const long i0 = 4 * g;
    const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
    float ce[4] = {0.f, 0.f, 0.f, 0.f};
    long long t[4] = {-1, -1, -1, -1};
    if (cnt == 4) {
      V4<float>::load(pix + i0, ce);
      const longlong2 ta = *reinterpret_cast<const longlong2*>(target + i0), tb = *reinterpret_cast<const longlong2*>(target + i0 + 2);
      t[0] = ta.x; t[1] = ta.y; t[2] = tb.x; t[3] = tb.y;
    } else {
      for (int j = 0; j < cnt; ++j) { ce[j] = pix[i0 + j]; t[j] = target[i0 + j]; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool valid = (!has_ignore || t[j] != (long long)ignore_index) && t[j] >= 0 && t[j] < C;
      float cf = 0.f;
      if (valid) {
        const float lp = -ce[j];
        float wq;
        focal_terms(__expf(lp), -expm1f(lp), lp, gamma, variant, &wq, &cf);
        lsum += (double)(wq * lp);
        lcnt += 1.0;
      }
      ce[j] = cf;
    }
    if (cnt == 4) V4<float>::store(pix + i0, ce);
    else for (int j = 0; j < cnt; ++j) pix[i0 + j] = ce[j];
  }
  if (lsw::block_sum2(lsum, lcnt)) {
    rows[2 * (long)blockIdx.x] = lsum;
    rows[2 * (long)blockIdx.x + 1] = lcnt;
  }
}

// One block of 16 waves: column j of the [nrows][3][C] rows is summed by one wave (lane = row, stride 64, then the butterfly: a fixed
// order), then thread c turns the sums of class c into its loss term and coef[c] = a_c, coef[24 + c] = b_c (0 for c >= C).
__global__ __launch_bounds__(FIN_NT) void softhead_dice_finalize_kernel(const double* rows, int nrows, int C, float smooth, float* coef,
                                                                        float* loss) {
  __shared__ double col[3 * CPMAX];
  __shared__ double term[CPMAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < 3 * C; j += FIN_NT / 64) {
    double s = 0.0;
    for (int r = lane; r < nrows; r += 64) s += rows[(long)r * 3 * C + j];
    s = wave_sum(s);
    if (lane == 0) col[j] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < CPMAX) {
    const int c = threadIdx.x;
    double t = 0.0, a = 0.0, b = 0.0;
    if (c < C) {
      double nv = 0.0;
      for (int k = 0; k < C; ++k) nv += col[2 * C + k];
      const double I = col[C + c], U = col[c] + col[2 * C + c];
      const double den = U + (double)smooth, num = 2.0 * I + (double)smooth;
      if (nv > 0.0) {
        if (den > 0.0) { t = 1.0 - num / den; a = -2.0 / ((double)C * den); b = num / ((double)C * den * den); }
        else t = 1.0;
      }
    }
    term[c] = t;
    coef[c] = (float)a;
    coef[CPMAX + c] = (float)b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += term[c];
    *loss = (float)(s / (double)C);
  }
}

inline bool softhead_grid_ok(int B, const HeadGeom& geo) { return B >= 0 && head_blocks(B, geo) <= 0x7fffffffL; }

inline double pass_bytes(int B, int C, int h, int w, int H, int W, int dtype) {
  return (double)B * h * w * C * (tss::esz(dtype) + 8.0) + (double)B * H * W * 8.0;
}

}  // namespace

extern "C" {

int tss_upsample_focal_fwd(const void* low, long ldl, const long long* target, float* ws /* tss_upsample_ce_ws floats, not initialised */,
                           float* loss, float* scale, int B, int C, int h, int w, int H, int W, int ignore_index, int has_ignore,
                           float alpha, float gamma, int variant, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, CPMAX, ldl, h, w, H, W) && gamma >= 0.f && (variant == 0 || variant == 1), TSS_ERR_SHAPE);
  TSS_REQUIRE(target && ws && loss && scale, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low) && tss::aligned16(ws), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, false);
  TSS_REQUIRE(softhead_grid_ok(B, geo), TSS_ERR_SHAPE);
  const long grid = head_blocks(B, geo);
  double* rows = reinterpret_cast<double*>(ws);
  float* tiles = ws + grid * 4;
  const hipStream_t st = (hipStream_t)stream;
  {
    tss::ProfScope prof(TSS_K_UPSAMPLE_CE_FWD, st, pass_bytes(B, C, h, w, H, W, dtype), 0);
    TSS_WITH_DTYPE(dtype, TSS_WITH_CLASS_REGS(C,
      hipLaunchKernelGGL((softhead_pass_kernel<TT, CPV, SH_FOCAL>), dim3((int)grid), dim3(NT), 0, st, (const TT*)low, ldl, target, tiles, rows,
                         C, h, w, H, W, ignore_index, has_ignore, geo, gamma, variant, nullptr)));
  }
  hipLaunchKernelGGL(softhead_focal_finalize_kernel, dim3(1), dim3(NT), 0, st, rows, (int)grid, alpha, loss, scale);
  return tss::check_last("upsample_focal_fwd");
}

// Rows of the [rows][2] f64 workspace that tss_focal_coef_from_ce writes (one per block of its grid); 0 for n <= 0.
long tss_focal_coef_rows(long n) {
  if (n <= 0) return 0;
  return tss::grid_for((n + 3) / 4, NT);
}

int tss_focal_coef_from_ce(float* pix, const long long* target, double* rows /*[tss_focal_coef_rows][2], not initialised*/, float* loss,
                           float* scale, long n, int C, int ignore_index, int has_ignore, float alpha, float gamma, int variant,
                           void* stream) {
  TSS_REQUIRE(n > 0 && C > 0 && gamma >= 0.f && (variant == 0 || variant == 1) && pix && target && rows && loss && scale, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(pix) && tss::aligned16(target) && tss::aligned16(rows), TSS_ERR_ALIGN);
  const hipStream_t st = (hipStream_t)stream;
  const int grid = (int)tss_focal_coef_rows(n);
  hipLaunchKernelGGL(focal_coef_kernel, dim3(grid), dim3(NT), 0, st, pix, target, rows, n, C, ignore_index, has_ignore, gamma, variant);
  hipLaunchKernelGGL(softhead_focal_finalize_kernel, dim3(1), dim3(NT), 0, st, rows, grid, alpha, loss, scale);
  return tss::check_last("focal_coef_from_ce");
}

// floats of the Dice workspace: 64 for the coefficients, then [nblocks][3][C] f64 rows; 0 for a refused shape
long tss_upsample_dice_ws(int B, int C, int h, int w, int H, int W) {
  if (B <= 0 || C <= 0 || C > CPMAX || h <= 0 || w <= 0 || H < h || W < w) return 0;
  const HeadGeom g = head_geom(B, C, h, w, H, W, false);
  return DICE_COEF + head_blocks(B, g) * 3 * C * 2;
}

int tss_upsample_dice_fwd(const void* low, long ldl, const long long* target, float* dice_ws /* tss_upsample_dice_ws floats, not initialised */,
                          float* loss, int B, int C, int h, int w, int H, int W, int ignore_index, int has_ignore, float smooth,
                          int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, CPMAX, ldl, h, w, H, W) && smooth >= 0.f && target && dice_ws && loss, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low) && tss::aligned16(dice_ws), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, false);
  TSS_REQUIRE(softhead_grid_ok(B, geo), TSS_ERR_SHAPE);
  const long grid = head_blocks(B, geo);
  double* rows = reinterpret_cast<double*>(dice_ws + DICE_COEF);
  const hipStream_t st = (hipStream_t)stream;
  {
    tss::ProfScope prof(TSS_K_UPSAMPLE_CE_FWD, st, pass_bytes(B, C, h, w, H, W, dtype), 0);
    TSS_WITH_DTYPE(dtype, TSS_WITH_CLASS_REGS(C,
      hipLaunchKernelGGL((softhead_pass_kernel<TT, CPV, SH_DICE_STATS>), dim3((int)grid), dim3(NT), 0, st, (const TT*)low, ldl, target, nullptr,
                         rows, C, h, w, H, W, ignore_index, has_ignore, geo, 0.f, 0, nullptr)));
  }
  hipLaunchKernelGGL(softhead_dice_finalize_kernel, dim3(1), dim3(FIN_NT), 0, st, rows, (int)grid, C, smooth, dice_ws, loss);
  return tss::check_last("upsample_dice_fwd");
}

int tss_upsample_dice_grad(const void* low, long ldl, const long long* target, const float* dice_ws, float* ws /* tss_upsample_ce_ws floats */,
                           int B, int C, int h, int w, int H, int W, int ignore_index, int has_ignore, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, CPMAX, ldl, h, w, H, W) && target && dice_ws && ws, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low) && tss::aligned16(dice_ws) && tss::aligned16(ws), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, false);
  TSS_REQUIRE(softhead_grid_ok(B, geo), TSS_ERR_SHAPE);
  const long grid = head_blocks(B, geo);
  float* tiles = ws + grid * 4;
  tss::ProfScope prof(TSS_K_UPSAMPLE_CE_FWD, (hipStream_t)stream, pass_bytes(B, C, h, w, H, W, dtype), 0);
  TSS_WITH_DTYPE(dtype, TSS_WITH_CLASS_REGS(C,
    hipLaunchKernelGGL((softhead_pass_kernel<TT, CPV, SH_DICE_GRAD>), dim3((int)grid), dim3(NT), 0, (hipStream_t)stream, (const TT*)low, ldl,
                       target, tiles, nullptr, C, h, w, H, W, ignore_index, has_ignore, geo, 0.f, 0, dice_ws)));
  return tss::check_last("upsample_dice_grad");
}

}  // extern "C"
