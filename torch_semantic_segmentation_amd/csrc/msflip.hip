// Multi-scale + horizontal-flip evaluation (the protocol behind the published Cityscapes numbers of this model family):
// the image is resized to several scales, every scale runs plain and mirrored, the class scores are summed at full
// resolution and the arg-max of the sum is scored.
//
//   resize_flip_planar_kernel : NCHW image [B,C,H,W] -> [2B,C,ho,wo], samples B..2B-1 the horizontal mirror of 0..B-1,
//                               one launch (the model then runs once per scale on the 2B batch).
//   multiscale_argmax_kernel  : K low-res NHWC logit maps -> uint8 prediction + confusion-matrix update.  For output
//                               pixel (b, y, x) and map k, z_k[c] = U_k[c, y, flip_k ? W-1-x : x] with U_k the
//                               align_corners=True upsample of map k to H x W (F.interpolate(...).flip(-1): the flip is
//                               taken AFTER the upsample, at full resolution); score[c] = sum_k softmax_c(z_k) (mode 0)
//                               or sum_k z_k[c] (mode 1), maps summed in descriptor order.
// Same lane / register layout as upsample_argmax_kernel (loss.hip): lane = output column, the two horizontally
// interpolated low-res rows of the current map in registers, a logit is one FMA.  A block owns a band of MS_ROWS output
// rows and keeps their MS_ROWS x CP scores in registers; maps are the outer loop, so a map's rows are fetched once per
// band.  The low-res maps total a few MB (L2 / Infinity Cache); only the prediction and the C x C counts reach HBM.
// Counts go through LDS and one integer atomic per non-zero cell: exact and order-independent, so bit-reproducible.
#include "headgeom.h"

namespace {

constexpr int MS_ROWS = 4;     // band height: MS_ROWS x CP score registers per lane; with the two rows and the logits that is past the 168
                               // registers of 3 waves per SIMD (it spilled 59..131 of them there), so the kernel asks for 2

template <typename TO>
__global__ __launch_bounds__(NT) void resize_flip_planar_kernel(const float* x, TO* y, long planes /* B*C */, int Hin, int Win,
                                                                int Hout, int Wout, int flip) {
  const long total = (flip ? 2 : 1) * planes * Hout * Wout;
  const float sy = ac_scale(Hin, Hout), sx = ac_scale(Win, Wout);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % Wout);
    long p = i / Wout;
    const int oy = (int)(p % Hout);
    long pl = p / Hout;
    const bool mirrored = pl >= planes;            // second half of the batch: the same planes, read right to left
    if (mirrored) pl -= planes;
    const Tap ty = ac_tap(sy, oy, Hin), tx = ac_tap(sx, mirrored ? Wout - 1 - ox : ox, Win);
    y[i] = (TO)planar_bilinear(x + pl * Hin * (long)Win, Win, ty, tx);
  }
}

template <typename T, int CP, int MODE>
__global__ __launch_bounds__(NT, 2) void multiscale_argmax_kernel(const MsArgs args, int K, const long long* target,
                                                                  unsigned char* pred_out, unsigned long long* cm, int B, int C,
                                                                  int H, int W, int ignore_index) {
  extern __shared__ unsigned int scm[];  // [C*C]
  const int tid = threadIdx.x;
  for (int i = tid; i < C * C; i += NT) scm[i] = 0u;
  __syncthreads();
  const HeadBlock blk = head_block((W + NT - 1) / NT, (H + MS_ROWS - 1) / MS_ROWS, MS_ROWS, H, W);
  const long b = blk.b;
  const int x = blk.x, ya = blk.ya;
  const bool xin = blk.xin;
  float score[MS_ROWS][CP];
#pragma unroll
  for (int j = 0; j < MS_ROWS; ++j)
#pragma unroll
    for (int c = 0; c < CP; ++c) score[j][c] = 0.f;

  for (int k = 0; k < K; ++k) {
    const MsMap mp = args.m[k];                // uniform: scalar loads from the argument segment
    const int h = mp.h, w = mp.w;
    const long ldl = mp.ldl;
    const HeadTaps map = head_taps(blk, h, w, H, W, mp.flip);
    const float sy = map.sy;
    const Tap tx = map.tx;
    const T* const img = reinterpret_cast<const T*>(mp.low) + (mp.first + b) * h * (long)w * ldl;
    float aA[CP], aB[CP];
    auto load = [&](int r, float* a) { load_row<CP, false, false>(img, r, w, ldl, tx, C, a); };   // pad channels hold anything
    int rA = ac_tap(sy, ya, h).i0;
    int rB = rA + (rA < h - 1 ? 1 : 0);
    load(rA, aA);
    load(rB, aB);
#pragma unroll
    for (int j = 0; j < MS_ROWS; ++j) {
      const int y = ya + j;
      if (y < H) {                             // uniform
        const Tap ty = ac_tap(sy, y, h);
        // h <= H: the row tap advances by at most one per output row in exact arithmetic.  A loop and not an `if`, so that an
        // f32 product that rounds across a row boundary (1 - scale below the rounding error: H in the thousands) still ends on
        // the tap's own rows.  ty.i0 <= h - 1, hence rA < h - 1 inside and rB == rA + 1: every turn moves rA up by one.
        while (rA < ty.i0) {                   // uniform
          rA = rB;
          rB = rA + (rA < h - 1 ? 1 : 0);
#pragma unroll
          for (int c = 0; c < CP; ++c) aA[c] = aB[c];
          load(rB, aB);
        }
        float z[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) z[c] = ty.l0 * aA[c] + ty.l1 * aB[c];
        if (MODE == 1) {
#pragma unroll
          for (int c = 0; c < CP; ++c) score[j][c] += z[c];
        } else {
          float m = z[0];
#pragma unroll
          for (int c = 1; c < CP; ++c) m = (c < C) ? fmaxf(m, z[c]) : m;
          float s = 0.f;
#pragma unroll
          for (int c = 0; c < CP; ++c) { z[c] = (c < C) ? __expf(z[c] - m) : 0.f; s += z[c]; }
          const float inv = 1.f / s;           // s >= 1: the largest term is exp(0)
#pragma unroll
          for (int c = 0; c < CP; ++c) score[j][c] += z[c] * inv;
        }
      }
    }
  }

#pragma unroll
  for (int j = 0; j < MS_ROWS; ++j) {
    const int y = ya + j;
    if (y < H && xin) {
      float best = score[j][0];
      int arg = 0;
#pragma unroll
      for (int c = 1; c < CP; ++c)
        if (c < C && score[j][c] > best) { best = score[j][c]; arg = c; }      // strict: the lowest index wins ties
      const long p = (b * H + y) * (long)W + x;
      if (pred_out) pred_out[p] = (unsigned char)arg;
      if (cm && target) {
        const long long t = target[p];
        if (t != ignore_index && t >= 0 && t < C) atomicAdd(&scm[(int)t * C + arg], 1u);
      }
    }
  }
  __syncthreads();
  if (cm && target)
    for (int i = tid; i < C * C; i += NT)
      if (scm[i]) atomicAdd(cm + i, (unsigned long long)scm[i]);
}

}  // namespace

extern "C" {

int tss_resize_flip_planar(const float* x, void* y, int y_dtype, long B, int C, int Hin, int Win, int Hout, int Wout,
                           int flip, void* stream) {
  TSS_CHECK_DTYPE(y_dtype);
  TSS_REQUIRE(B >= 0 && C >= 0 && Hin > 0 && Win > 0 && Hout >= 0 && Wout >= 0, TSS_ERR_SHAPE);
  const long planes = B * C, nout = (flip ? 2 : 1) * planes;
  const long total = nout * Hout * Wout;
  if (total == 0) return TSS_OK;
  tss::ProfScope prof(TSS_K_RESIZE_FLIP_PLANAR, (hipStream_t)stream,
                      (double)planes * Hin * Win * 4.0 + (double)total * tss::esz(y_dtype), 0);
  TSS_WITH_DTYPE(y_dtype, hipLaunchKernelGGL(resize_flip_planar_kernel<TT>, dim3(tss::grid_for(total, NT)), dim3(NT), 0,
                                             (hipStream_t)stream, x, (TT*)y, planes, Hin, Win, Hout, Wout, flip ? 1 : 0));
  return tss::check_last("resize_flip_planar");
}

int tss_multiscale_argmax_confusion(const tss_msmap* maps, int K, const long long* target, unsigned char* pred,
                                    unsigned long long* confusion /*[C*C] accumulated*/, int B, int C, int H, int W,
                                    int ignore_index, int mode, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(maps && K >= 1 && K <= MS_MAXK && C >= 1 && C <= 24 && B >= 0 && H >= 0 && W >= 0 && (mode == 0 || mode == 1),
              TSS_ERR_SHAPE);
  MsArgs args = {};
  double low_bytes;
  const int err = ms_args(maps, K, B, C, H, W, dtype, &args, &low_bytes);
  if (err != TSS_OK) return err;
  const bool counts = confusion && target;
  if ((long)B * H * W == 0 || (!pred && !counts)) return TSS_OK;
  const long grid = (long)B * ((W + NT - 1) / NT) * ((H + MS_ROWS - 1) / MS_ROWS);
  TSS_REQUIRE(grid <= 0x7fffffffL, TSS_ERR_SHAPE);
  tss::ProfScope prof(TSS_K_MULTISCALE_ARGMAX, (hipStream_t)stream, low_bytes + (double)B * H * W * ((pred ? 1.0 : 0.0) + (counts ? 8.0 : 0.0)), 0);
  const size_t sh = (size_t)C * C * sizeof(unsigned int);
  TSS_WITH_DTYPE(dtype, TSS_WITH_CLASS_REGS(C,
    if (mode == 0) hipLaunchKernelGGL((multiscale_argmax_kernel<TT, CPV, 0>), dim3((int)grid), dim3(NT), sh, (hipStream_t)stream,
                                      args, K, target, pred, confusion, B, C, H, W, ignore_index);
    else hipLaunchKernelGGL((multiscale_argmax_kernel<TT, CPV, 1>), dim3((int)grid), dim3(NT), sh, (hipStream_t)stream,
                            args, K, target, pred, confusion, B, C, H, W, ignore_index)));
  return tss::check_last("multiscale_argmax_confusion");
}

}  // extern "C"
