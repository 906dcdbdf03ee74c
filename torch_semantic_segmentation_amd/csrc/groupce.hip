// Per-sample loss groups on the fused head: L = sum_g (sum_{b in g} lambda_b S_b) / N_g, N_g = sum_{b in g} n_b, from the loss rows
// and gradient tiles that an ordinary forward entry (tss_upsample_ce_fwd, _fwd_ex, tss_upsample_ce_wide_fwd) left in its workspace.
// The expensive pass is untouched: its block index is (b * nband + band) * nstrip + strip, so the nband * nstrip rows (sum of the
// loss, sum of the weight) of a sample are contiguous, and its tiles are unscaled.  What changes is what follows it:
//
//   ce_group_finalize_kernel    one block.  (1) S_b, n_b: one wave per sample, lane l adds rows l, l + 64, ... of the sample, then
//                               the xor butterfly -- a fixed order.  (2) thread i, as group i: N_i and A_i = sum lambda_b S_b over the
//                               samples of the group in ascending b, L_i = A_i / N_i (0 for N_i = 0 or an id no sample uses); as
//                               sample i: the same sum N of its own group, scale[i] = lambda_i / N (0 for N = 0).  (3) thread 0 adds
//                               L_g in ascending g.  All of it f64, rounded once on the way out; no atomics, no host read-back.
//                               An empty group gives 0 and a zero gradient (the rule of the focal and Dice operators), not the nan
//                               of the ungrouped mean.  A group id outside [0, B) makes its sample one of weight 0 in no group.
//   *_gather_rows_kernel        head_gather with the scale read per sample (headgeom.h, ROWS).
//   selftrain_weights_kernel    the rows of a self-training step: labelled half group 0 / weight 1, unlabelled half group 1 / weight
//                               lam (mode 0) or lam * sum_b kept_b / (B * n_pixels) (mode 1; an integer sum, then f64, rounded once).
#include "headgeom.h"

namespace {

constexpr int WMAXC = 256;        // as widehead.hip
constexpr int GROUP_MAXB = 1024;  // samples per call: what the finalize block keeps in LDS (32 KB)

__global__ __launch_bounds__(NT) void ce_group_finalize_kernel(const double* rows, int B, int rps, const int* group, const float* weight,
                                                               float* loss, float* scale, float* group_loss) {
  __shared__ double S[GROUP_MAXB], Nn[GROUP_MAXB], Lg[GROUP_MAXB];
  __shared__ int G[GROUP_MAXB];
  __shared__ float Lam[GROUP_MAXB];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int b = wave; b < B; b += NT / 64) {            // uniform over the wave
    const double* r = rows + 2 * (long)b * rps;
    double s = 0.0, n = 0.0;
    for (int i = lane; i < rps; i += 64) { s += r[2 * (long)i]; n += r[2 * (long)i + 1]; }
    s = wave_sum(s);
    n = wave_sum(n);
    if (lane == 0) { S[b] = s; Nn[b] = n; }
  }
  for (int b = tid; b < B; b += NT) {
    const int g = group[b];
    const bool ok = g >= 0 && g < B;
    G[b] = ok ? g : -1;
    Lam[b] = ok ? (weight ? weight[b] : 1.f) : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < B; i += NT) {
    double N = 0.0, A = 0.0;                           // group i
    for (int b = 0; b < B; ++b)
      if (G[b] == i) { N += Nn[b]; A += (double)Lam[b] * S[b]; }
    const double L = N > 0.0 ? A / N : 0.0;
    Lg[i] = L;
    group_loss[i] = (float)L;
    const int g = G[i];                                // sample i: the same sum, in the same order, of its own group
    double Nb = 0.0;
    for (int b = 0; b < B; ++b)
      if (g >= 0 && G[b] == g) Nb += Nn[b];
    scale[i] = Nb > 0.0 ? (float)((double)Lam[i] / Nb) : 0.f;
  }
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int g = 0; g < B; ++g) sum += Lg[g];
    *loss = (float)sum;
  }
}

template <typename T, int CP>
__global__ __launch_bounds__(NT) void upsample_ce_gather_rows_kernel(const float* tiles, const float* scale, const float* grad_out, T* dlow,
                                                                     long ldl, int B, int h, int w, int H, int W, const HeadGeom geo) {
  head_gather<T, CP, true>(tiles, scale, grad_out, dlow, ldl, B, h, w, H, W, geo);
}

__global__ __launch_bounds__(NT) void selftrain_weights_kernel(const unsigned long long* kept, long n_pixels, const float* lam, int mode,
                                                               int* group, float* weight, int B) {
  double wu = (double)*lam;
  if (mode == 1) {
    unsigned long long total = 0ull;                   // integers: exact in any order; every thread holds the same sum
    for (int b = 0; b < B; ++b) total += kept[b];
    wu = wu * (double)total / ((double)B * (double)n_pixels);
  }
  const float wf = (float)wu;
  for (int i = threadIdx.x; i < 2 * B; i += NT) {
    group[i] = i < B ? 0 : 1;
    weight[i] = i < B ? 1.f : wf;
  }
}

// the head's shape rules without a pitch (the finalize sees no map)
inline bool group_shape_ok(int B, int C, int cap, int h, int w, int H, int W) {
  return B >= 0 && B <= GROUP_MAXB && C > 0 && C <= cap && h > 0 && w > 0 && H >= h && W >= w;
}

}  // namespace

extern "C" {

int tss_upsample_ce_group_max_batch(void) { return GROUP_MAXB; }

int tss_upsample_ce_group_finalize(const float* ws, int B, int C, int h, int w, int H, int W, int wide, const int* group,
                                   const float* weight, float* loss, float* scale, float* group_loss, void* stream) {
  TSS_REQUIRE(group_shape_ok(B, C, wide ? WMAXC : 24, h, w, H, W) && ws && group && loss && scale && group_loss, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(ws), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, wide != 0);
  TSS_REQUIRE(head_blocks(B, geo) <= 0x7fffffffL, TSS_ERR_SHAPE);
  hipLaunchKernelGGL(ce_group_finalize_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, reinterpret_cast<const double*>(ws), B,
                     geo.nband * geo.nstrip, group, weight, loss, scale, group_loss);
  return tss::check_last("upsample_ce_group_finalize");
}

int tss_upsample_ce_bwd_rows(const float* ws, const float* scale, const float* grad_out, void* dlow, long ldl,
                             int B, int C, int h, int w, int H, int W, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, 24, ldl, h, w, H, W) && B >= 0 && ws && scale && dlow, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(ws) && tss::aligned16(dlow), TSS_ERR_ALIGN);
  const long n = (long)B * h * w * ldl;
  if (n == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, false);
  const float* tiles = ws + head_blocks(B, geo) * 4;
  tss::ProfScope prof(TSS_K_UPSAMPLE_CE_BWD, (hipStream_t)stream, (double)n * (4.0 + tss::esz(dtype)), 0);
  TSS_WITH_DTYPE(dtype, TSS_WITH_CLASS_REGS(C,
    hipLaunchKernelGGL((upsample_ce_gather_rows_kernel<TT, CPV>), dim3(tss::grid_for(n / 8, NT)), dim3(NT), 0, (hipStream_t)stream,
                       tiles, scale, grad_out, (TT*)dlow, ldl, B, h, w, H, W, geo)));
  return tss::check_last("upsample_ce_bwd_rows");
}

int tss_upsample_ce_wide_bwd_rows(const float* ws, const float* scale, const float* grad_out, void* dlow, long ldl,
                                  int B, int C, int h, int w, int H, int W, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, WMAXC, ldl, h, w, H, W) && B >= 0 && ws && scale && dlow, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(ws) && tss::aligned16(dlow), TSS_ERR_ALIGN);
  const long n = (long)B * h * w * ldl;
  if (n == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, true);
  const float* tiles = ws + head_blocks(B, geo) * 4;
  tss::ProfScope prof(TSS_K_WIDE_CE_BWD, (hipStream_t)stream, (double)n * (4.0 + tss::esz(dtype)), 0);
  TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL((upsample_ce_gather_rows_kernel<TT, 0>), dim3(tss::grid_for(n / 8, NT)), dim3(NT), 0,
                                           (hipStream_t)stream, tiles, scale, grad_out, (TT*)dlow, ldl, B, h, w, H, W, geo));
  return tss::check_last("upsample_ce_wide_bwd_rows");
}

int tss_selftrain_weights(const long long* kept, long n_pixels, const float* lam, int mode, int* group, float* weight, int B,
                          void* stream) {
  TSS_REQUIRE(B >= 1 && B <= GROUP_MAXB / 2 && n_pixels >= 1 && (mode == 0 || mode == 1) && lam && group && weight &&
              (mode == 0 || kept), TSS_ERR_SHAPE);
  TSS_REQUIRE((reinterpret_cast<uintptr_t>(kept) & 7u) == 0 && (reinterpret_cast<uintptr_t>(group) & 3u) == 0 &&
              (reinterpret_cast<uintptr_t>(weight) & 3u) == 0 && (reinterpret_cast<uintptr_t>(lam) & 3u) == 0, TSS_ERR_ALIGN);
  hipLaunchKernelGGL(selftrain_weights_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(kept), n_pixels, lam, mode, group, weight, B);
  return tss::check_last("selftrain_weights");
}

}  // extern "C"
