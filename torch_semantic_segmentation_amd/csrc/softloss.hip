// Focal loss (TSS/losses/focal_loss.py:8-15) and soft Dice loss (TSS/losses/dice_loss.py:8-26) over NCHW-planar logits.
// Instances of the class-plane sweep of losssweep.h: its lane layout, group loop, labels and validity rule (a pixel counts iff
// target != ignore_index, when there is one, and 0 <= target < C), its reductions; the per-pixel log-sum-exp is saved in f32.
//
// No atomics: every block stores its partial sums (f64) into a row of its own in the caller's workspace (plain stores, every
// element that is read was written, nothing zero-filled) and a one-block finalize kernel adds the rows in a fixed order, so
// two runs give the same bits.  max_blocks > 0 caps the grid (tests: several grid-stride trips and several rows at a tiny shape).
//
// focal:  p = s_t, lp = x_t - lse, q = sum_{c != t} s_c  (summed, not 1 - p: that cancels in f32 once p -> 1, where a
//         trained net keeps most pixels);  w = exp(q^gamma) (variant 0, what the reference computes) or q^gamma (variant 1,
//         Lin et al. 2017);  loss = -alpha * sum_V w lp / |V|.
//         dloss/dx_c = A ([c == t] - s_c) alpha grad_out / |V|,  A = -(p w' lp + w),  w' = dw/dp = -gamma q^(gamma-1) w
//         (variant 1: -gamma q^(gamma-1)); gamma == 0: w' = 0; q == 0: the term p w' lp is taken as 0 (its limit).
//         The forward has p, q and lp of a pixel in registers, so it saves A per pixel (0 for a pixel outside V) next to
//         the lse, and the backward is the gradient sweep of losssweep.h (sign reversed): s_c is recomputed from the saved lse.
// dice:   I_c = sum_V p_c [t == c], U_c = sum_V p_c + sum_V [t == c], loss = mean_c 1 - (2 I_c + smooth) / (U_c + smooth)
//         over all C classes (an absent class counts).  Per-class sums live in registers, DICE_CP classes at a time: the sweep
//         reads the planes a second time right after the lse sweep of the same 8 pixels (C <= DICE_CP: once per plane and
//         trip; more classes: one more sweep per DICE_CP classes, the lse read back).  The finalize kernel also writes
//         a_c = -2 / (C (U_c + smooth)), b_c = (2 I_c + smooth) / (C (U_c + smooth)^2); with G_c = a_c [t == c] + b_c the
//         backward is dx_k = p_k (G_k - sum_c p_c G_c) grad_out on V (coefficients in LDS, two sweeps), 0 elsewhere.
// V empty: loss 0, zero gradient (both losses; no host read-back).  A class with U_c + smooth == 0 contributes 1 (the
// limit of 0 / U) and zero coefficients.
#include "losssweep.h"

namespace {

constexpr int NT = lsw::NT;
constexpr int WAVES = NT / 64;
constexpr int DICE_CP = 24;               // class sums held in registers per sweep (3 accumulators each)
constexpr int DICE_MAX_C = 256;
constexpr int DICE_FWD_BLOCKS = 768;     // default cap of the Dice forward grid: 3 blocks per CU are resident (150 VGPRs), a row is 3C doubles
constexpr int FIN_NT = 1024;              // the Dice finalize block: 16 waves, one column of the rows per wave at a time

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

inline int grid_of(long groups, int max_blocks, long default_cap) {
  return tss::grid_for(groups, NT, max_blocks > 0 ? (long)max_blocks : default_cap);
}

// ------------------------------------------------------------------------------------------------------------ focal
template <typename T>
__global__ __launch_bounds__(NT) void focal_fwd_kernel(const T* logits, const long long* target, float* lse_out, float* pixw,
                                                       double* rows /*[gridDim.x][2]: sum of w lp, valid count*/, long B, int C,
                                                       long HW, int ignore_index, int has_ignore, float gamma, int variant) {
  double lsum = 0.0, lcnt = 0.0;
  for (lsw::Groups g(B, HW); g.more(); g.next()) {
    const long b = g.b(), off = g.off();
    const T* base = logits + b * C * HW + off;
    int tv[8];
    lsw::load_labels(target + b * HW + off, C, ignore_index, has_ignore, tv);
    float m[8], so[8], xt[8];           // running maximum over all classes, sum of exp over the classes != t, the target's logit
#pragma unroll
    for (int j = 0; j < 8; ++j) { m[j] = -INFINITY; so[j] = 0.f; xt[j] = 0.f; }
    for (int c = 0; c < C; ++c) {
      float v[8];
      V8<T>::load(base + (long)c * HW, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float mn = fmaxf(m[j], v[j]);
        const bool is = tv[j] == c;
        so[j] = so[j] * __expf(m[j] - mn) + (is ? 0.f : __expf(v[j] - mn));
        m[j] = mn;
        if (is) xt[j] = v[j];
      }
    }
    float l[8], a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool valid = tv[j] >= 0;
      const float et = valid ? __expf(xt[j] - m[j]) : 0.f;
      const float s = so[j] + et;
      const float lg = (et == 1.f) ? log1pf(so[j]) : __logf(s);     // the target holds the maximum: log(1 + so) without the rounding of 1 + so
      l[j] = m[j] + lg;
      a[j] = 0.f;
      if (valid) {
        const float lp = (xt[j] - m[j]) - lg;
        const float inv = 1.f / s;
        const float p = et * inv, q = so[j] * inv;
        float qg = 1.f, dqg = 0.f;                                   // q^gamma, gamma q^(gamma-1)
        if (gamma != 0.f) {
          qg = q > 0.f ? exp2f(gamma * __log2f(q)) : 0.f;
          dqg = q > 0.f ? gamma * qg / q : 0.f;
        }
        const float w = variant == 0 ? __expf(qg) : qg;
        const float wp = variant == 0 ? -dqg * w : -dqg;
        a[j] = -(p * wp * lp + w);
        lsum += (double)(w * lp);
        lcnt += 1.0;
      }
    }
    V8<float>::store(lse_out + b * HW + off, l);
    V8<float>::store(pixw + b * HW + off, a);
  }
  if (lsw::block_sum2(lsum, lcnt)) {
    rows[2 * (long)blockIdx.x] = lsum;
    rows[2 * (long)blockIdx.x + 1] = lcnt;
  }
}

// loss = -alpha * sum(rows[.][0]) / n, scale = alpha / n with n = sum(rows[.][1]); n == 0: both 0.  One block, fixed tree.
__global__ __launch_bounds__(NT) void focal_finalize_kernel(const double* rows, int nrows, float alpha, float* loss, float* scale) {
  double sum, cnt;
  if (lsw::row_sum2(rows, nrows, sum, cnt)) {
    *loss = cnt > 0.0 ? (float)(-(double)alpha * sum / cnt) : 0.f;
    *scale = cnt > 0.0 ? (float)((double)alpha / cnt) : 0.f;
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void focal_bwd_kernel(const T* logits, const long long* target, const float* lse, const float* pixw,
                                                       const float* scale, const float* grad_out, T* dlogits, long B, int C, long HW) {
  const float gs = (*scale) * (grad_out ? *grad_out : 1.f);
  for (lsw::Groups g(B, HW); g.more(); g.next()) {
    const long b = g.b(), off = g.off();
    int tv[8];
    float l[8], a[8];
    lsw::load_labels(target + b * HW + off, C, 0, 0, tv);      // the one-hot term only: a == 0 outside the valid set
    V8<float>::load(lse + b * HW + off, l);
    V8<float>::load(pixw + b * HW + off, a);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] *= gs;
    lsw::grad8<true>(logits + b * C * HW + off, dlogits + b * C * HW + off, C, HW, tv, l, a);
  }
}

// ------------------------------------------------------------------------------------------------------------ dice
// rows[block][kind][c], kind 0: sum_V p_c, 1: sum_V p_c [t == c], 2: sum_V [t == c]
template <typename T>
__global__ __launch_bounds__(NT) void dice_fwd_kernel(const T* logits, const long long* target, float* lse_out, double* rows,
                                                      long B, int C, long HW, int ignore_index, int has_ignore) {
  __shared__ double red[WAVES][3 * DICE_CP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* row = rows + (long)blockIdx.x * 3 * C;
  for (int c0 = 0; c0 < C; c0 += DICE_CP) {
    float aP[DICE_CP], aI[DICE_CP], aN[DICE_CP];
#pragma unroll
    for (int k = 0; k < DICE_CP; ++k) { aP[k] = 0.f; aI[k] = 0.f; aN[k] = 0.f; }
    for (lsw::Groups g(B, HW); g.more(); g.next()) {
      const long b = g.b(), off = g.off();
      const T* base = logits + b * C * HW + off;
      int tv[8];
      lsw::load_labels(target + b * HW + off, C, ignore_index, has_ignore, tv);
      float l[8];
      if (c0 == 0) {
        lsw::lse8<false>(base, C, HW, nullptr, l, nullptr);
        V8<float>::store(lse_out + b * HW + off, l);
      } else {
        V8<float>::load(lse_out + b * HW + off, l);      // this lane's own store of the first sweep
      }
#pragma unroll
      for (int k = 0; k < DICE_CP; ++k) {
        if (c0 + k < C) {                                // uniform
          float v[8];
          V8<T>::load(base + (long)(c0 + k) * HW, v);
          float sp = 0.f, si = 0.f, sn = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float p = tv[j] >= 0 ? __expf(v[j] - l[j]) : 0.f;
            const bool is = tv[j] == c0 + k;
            sp += p;
            si += is ? p : 0.f;
            sn += is ? 1.f : 0.f;
          }
          aP[k] += sp; aI[k] += si; aN[k] += sn;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < DICE_CP; ++k) {
      const double p = wave_sum((double)aP[k]), q = wave_sum((double)aI[k]), n = wave_sum((double)aN[k]);
      if (lane == 0) { red[wave][k] = p; red[wave][DICE_CP + k] = q; red[wave][2 * DICE_CP + k] = n; }
    }
    __syncthreads();
    if (threadIdx.x < 3 * DICE_CP) {
      const int kind = threadIdx.x / DICE_CP, k = threadIdx.x - kind * DICE_CP;
      if (c0 + k < C) {
        double s = 0.0;
        for (int w = 0; w < WAVES; ++w) s += red[w][threadIdx.x];
        row[kind * C + c0 + k] = s;
      }
    }
    __syncthreads();
  }
}

// One block of 16 waves: column j of the rows is summed by one wave (lane = row, stride 64, then the butterfly: a fixed order),
// then thread c turns the sums of class c into its loss term and backward coefficients coef[c] = a_c, coef[C + c] = b_c.
__global__ __launch_bounds__(FIN_NT) void dice_finalize_kernel(const double* rows, int nrows, int C, float smooth, float* coef, float* loss) {
  __shared__ double col[3 * DICE_MAX_C];
  __shared__ double term[DICE_MAX_C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < 3 * C; j += FIN_NT / 64) {
    double s = 0.0;
    for (int r = lane; r < nrows; r += 64) s += rows[(long)r * 3 * C + j];
    s = wave_sum(s);
    if (lane == 0) col[j] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < C) {
    const int c = threadIdx.x;
    double nv = 0.0;
    for (int k = 0; k < C; ++k) nv += col[2 * C + k];
    const double I = col[C + c], U = col[c] + col[2 * C + c];
    const double den = U + (double)smooth, num = 2.0 * I + (double)smooth;
    double t = 0.0, a = 0.0, b = 0.0;
    if (nv > 0.0) {
      if (den > 0.0) { t = 1.0 - num / den; a = -2.0 / ((double)C * den); b = num / ((double)C * den * den); }
      else t = 1.0;
    }
    term[c] = t;
    coef[c] = (float)a;
    coef[C + c] = (float)b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += term[c];
    *loss = (float)(s / (double)C);
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void dice_bwd_kernel(const T* logits, const long long* target, const float* lse, const float* coef,
                                                      const float* grad_out, T* dlogits, long B, int C, long HW, int ignore_index,
                                                      int has_ignore) {
  __shared__ float sa[DICE_MAX_C], sb[DICE_MAX_C];
  for (int c = threadIdx.x; c < C; c += NT) { sa[c] = coef[c]; sb[c] = coef[C + c]; }
  __syncthreads();
  const float go = grad_out ? *grad_out : 1.f;
  for (lsw::Groups g(B, HW); g.more(); g.next()) {
    const long b = g.b(), off = g.off();
    const T* base = logits + b * C * HW + off;
    int tv[8];
    lsw::load_labels(target + b * HW + off, C, ignore_index, has_ignore, tv);
    float l[8], dot[8], gv[8];
    V8<float>::load(lse + b * HW + off, l);
#pragma unroll
    for (int j = 0; j < 8; ++j) { dot[j] = 0.f; gv[j] = tv[j] >= 0 ? go : 0.f; }
    for (int c = 0; c < C; ++c) {                        // sum_c p_c G_c
      float v[8];
      V8<T>::load(base + (long)c * HW, v);
      const float ac = sa[c], bc = sb[c];
#pragma unroll
      for (int j = 0; j < 8; ++j) dot[j] += __expf(v[j] - l[j]) * (bc + (tv[j] == c ? ac : 0.f));
    }
    for (int c = 0; c < C; ++c) {
      float v[8], d[8];
      V8<T>::load(base + (long)c * HW, v);
      const float ac = sa[c], bc = sb[c];
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = __expf(v[j] - l[j]) * ((bc + (tv[j] == c ? ac : 0.f)) - dot[j]) * gv[j];
      V8<T>::store(dlogits + (b * C + c) * HW + off, d);
    }
  }
}

inline size_t dice_coef_bytes(int C) { return up256(sizeof(float) * 2 * (size_t)C); }

}  // namespace

extern "C" {

long tss_focal_workspace_bytes(long B, long HW, int max_blocks) {
  if (B <= 0 || HW <= 0 || (HW % 8) != 0 || max_blocks < 0) return 0;
  return (long)(sizeof(double) * 2 * (size_t)grid_of(B * (HW / 8), max_blocks, 4096));
}

int tss_focal_fwd(const void* logits, const long long* target, float* lse, float* pixel_coef, void* workspace, float* loss, float* scale,
                  long B, int C, long HW, int ignore_index, int has_ignore, float alpha, float gamma, int variant, int max_blocks,
                  int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(tss::planar_shape_ok(B, C, HW) && gamma >= 0.f && (variant == 0 || variant == 1) && max_blocks >= 0, TSS_ERR_SHAPE);
  TSS_REQUIRE(target && lse && pixel_coef && workspace && loss && scale, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(logits) && tss::aligned16(lse) && tss::aligned16(pixel_coef) && tss::aligned16(workspace), TSS_ERR_ALIGN);
  hipStream_t st = (hipStream_t)stream;
  const long groups = B * (HW / 8);
  const int grid = grid_of(groups, max_blocks, 4096);
  double* rows = static_cast<double*>(workspace);
  TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL(focal_fwd_kernel<TT>, dim3(grid), dim3(NT), 0, st, (const TT*)logits, target, lse, pixel_coef, rows,
                                           B, C, HW, ignore_index, has_ignore, gamma, variant));
  hipLaunchKernelGGL(focal_finalize_kernel, dim3(1), dim3(NT), 0, st, rows, grid, alpha, loss, scale);
  return tss::check_last("focal_fwd");
}

int tss_focal_bwd(const void* logits, const long long* target, const float* lse, const float* pixel_coef, const float* scale,
                  const float* grad_out, void* dlogits, long B, int C, long HW, int max_blocks, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(tss::planar_shape_ok(B, C, HW) && max_blocks >= 0 && target && lse && pixel_coef && scale, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(logits) && tss::aligned16(dlogits) && tss::aligned16(lse) && tss::aligned16(pixel_coef), TSS_ERR_ALIGN);
  const long groups = B * (HW / 8);
  TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL(focal_bwd_kernel<TT>, dim3(grid_of(groups, max_blocks, 4096)), dim3(NT), 0, (hipStream_t)stream,
                                           (const TT*)logits, target, lse, pixel_coef, scale, grad_out, (TT*)dlogits, B, C, HW));
  return tss::check_last("focal_bwd");
}

long tss_dice_workspace_bytes(long B, int C, long HW, int max_blocks) {
  if (B <= 0 || HW <= 0 || (HW % 8) != 0 || C <= 0 || C > DICE_MAX_C || max_blocks < 0) return 0;
  return (long)(dice_coef_bytes(C) + sizeof(double) * 3 * (size_t)C * (size_t)grid_of(B * (HW / 8), max_blocks, DICE_FWD_BLOCKS));
}

int tss_dice_fwd(const void* logits, const long long* target, float* lse, void* workspace, float* loss, long B, int C, long HW,
                 int ignore_index, int has_ignore, float smooth, int max_blocks, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(tss::planar_shape_ok(B, C, HW) && C <= DICE_MAX_C && smooth >= 0.f && max_blocks >= 0, TSS_ERR_SHAPE);
  TSS_REQUIRE(target && lse && workspace && loss, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(logits) && tss::aligned16(lse) && tss::aligned16(workspace), TSS_ERR_ALIGN);
  hipStream_t st = (hipStream_t)stream;
  const long groups = B * (HW / 8);
  const int grid = grid_of(groups, max_blocks, DICE_FWD_BLOCKS);
  float* coef = static_cast<float*>(workspace);
  double* rows = reinterpret_cast<double*>(static_cast<char*>(workspace) + dice_coef_bytes(C));
  TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL(dice_fwd_kernel<TT>, dim3(grid), dim3(NT), 0, st, (const TT*)logits, target, lse, rows, B, C, HW,
                                           ignore_index, has_ignore));
  hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(FIN_NT), 0, st, rows, grid, C, smooth, coef, loss);
  return tss::check_last("dice_fwd");
}

int tss_dice_bwd(const void* logits, const long long* target, const float* lse, const void* workspace, const float* grad_out,
                 void* dlogits, long B, int C, long HW, int ignore_index, int has_ignore, int max_blocks, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(tss::planar_shape_ok(B, C, HW) && C <= DICE_MAX_C && max_blocks >= 0 && target && lse && workspace, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(logits) && tss::aligned16(dlogits) && tss::aligned16(lse) && tss::aligned16(workspace), TSS_ERR_ALIGN);
  const long groups = B * (HW / 8);
  TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL(dice_bwd_kernel<TT>, dim3(grid_of(groups, max_blocks, 4096)), dim3(NT), 0, (hipStream_t)stream,
                                           (const TT*)logits, target, lse, static_cast<const float*>(workspace), grad_out, (TT*)dlogits,
                                           B, C, HW, ignore_index, has_ignore));
  return tss::check_last("dice_bwd");
}

}  // extern "C"
