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
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int MS_ROWS = 4;     // band height: MS_ROWS x CP score registers per lane; with the two rows and the logits that is past the 168
                               // registers of 3 waves per SIMD (it spilled 59..131 of them there), so the kernel asks for 2
constexpr int MS_MAXK = 16;

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

// The descriptors as the kernel takes them: by value, in the kernel argument segment (no device memory, no copy to wait for).
struct MsMap { const void* low; long first; int ldl, h, w, flip; };
struct MsArgs { MsMap m[MS_MAXK]; };

template <typename T, int CP, int MODE>
__global__ __launch_bounds__(NT, 2) void multiscale_argmax_kernel(const MsArgs args, int K, const long long* target,
                                                                  unsigned char* pred_out, unsigned long long* cm, int B, int C,
                                                                  int H, int W, int ignore_index) {
  extern __shared__ unsigned int scm[];  // [C*C]
  const int tid = threadIdx.x;
  for (int i = tid; i < C * C; i += NT) scm[i] = 0u;
  __syncthreads();
  const int nstrip = (W + NT - 1) / NT, nband = (H + MS_ROWS - 1) / MS_ROWS;
  int bid = blockIdx.x;
  const int strip = bid % nstrip; bid /= nstrip;
  const int band = bid % nband;
  const long b = bid / nband;
  const int x = strip * NT + tid;
  const bool xin = x < W;
  const int xc = xin ? x : W - 1;              // lanes past the edge compute column W-1 and write nothing
  const int ya = band * MS_ROWS;
  float score[MS_ROWS][CP];
#pragma unroll
  for (int j = 0; j < MS_ROWS; ++j)
#pragma unroll
    for (int c = 0; c < CP; ++c) score[j][c] = 0.f;

  for (int k = 0; k < K; ++k) {
    const MsMap mp = args.m[k];                // uniform: scalar loads from the argument segment
    const int h = mp.h, w = mp.w;
    const long ldl = mp.ldl;
    const float sy = ac_scale(h, H), sx = ac_scale(w, W);
    const Tap tx = ac_tap(sx, mp.flip ? W - 1 - xc : xc, w);
    const T* const img = reinterpret_cast<const T*>(mp.low) + (mp.first + b) * h * (long)w * ldl;
    float aA[CP], aB[CP];
    auto load_row = [&](int r, float* a) {
      const T* p0 = img + ((long)r * w + tx.i0) * ldl;
      const T* p1 = img + ((long)r * w + tx.i1) * ldl;
#pragma unroll
      for (int c4 = 0; c4 < CP; c4 += 4) {
        float u[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
        if (c4 < C) {                          // uniform; ldl >= round_up(C, 4) (host-checked), nothing past it is read
          V4<T>::load(p0 + c4, u);
          V4<T>::load(p1 + c4, v);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) a[c4 + q] = (c4 + q < C) ? tx.l0 * u[q] + tx.l1 * v[q] : 0.f;   // pad channels hold anything
      }
    };
    int rA = ac_tap(sy, ya, h).i0;
    int rB = rA + (rA < h - 1 ? 1 : 0);
    load_row(rA, aA);
    load_row(rB, aB);
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
          load_row(rB, aB);
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
  double low_bytes = 0.0;
  for (int k = 0; k < K; ++k) {
    const tss_msmap& m = maps[k];
    TSS_REQUIRE(m.low && (m.ldl % 8) == 0 && m.ldl >= (C + 3) / 4 * 4 && m.ldl <= (1L << 30) && m.h >= 1 && m.w >= 1 &&
                m.h <= H && m.w <= W && m.first >= 0, TSS_ERR_SHAPE);
    TSS_REQUIRE(tss::aligned16(m.low), TSS_ERR_ALIGN);
    args.m[k].low = m.low; args.m[k].first = m.first; args.m[k].ldl = (int)m.ldl;
    args.m[k].h = m.h; args.m[k].w = m.w; args.m[k].flip = m.flip ? 1 : 0;
    low_bytes += (double)B * m.h * m.w * C * tss::esz(dtype);
  }
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
