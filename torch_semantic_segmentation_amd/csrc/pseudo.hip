// Pseudo-labels of a teacher, straight from its low-resolution NHWC logits: per output pixel the arg-max class of the bilinearly
// (align_corners=True) upsampled logits, its softmax probability conf = 1 / sum_c exp(z_c - z_arg), and the thresholded label
//   label = conf >= *threshold ? arg : ignore_index          (a byte; the host keeps C <= ignore_index <= 255)
// plus, per sample, the number of labels kept.  Nothing of B x C x H x W elements exists: the stock composition (interpolate ->
// softmax -> max -> where) writes that tensor twice.
//
//   pseudo_label_kernel       the band walk, taps and blend of upsample_argmax_kernel (loss.hip), text for text, so that at
//                             *threshold = 0 the labels are that kernel's predictions; the scores of a pixel are still in registers
//                             after the arg-max, and the sum of exponentials is one more pass over them (C <= 24).
//   wide_pseudo_label_kernel  wide_upsample_argmax_kernel's walk (widehead.hip) by chunks of 16 classes: running (best, index) per
//                             (row, lane) in LDS, then a SECOND walk over the chunks that accumulates sum exp(z - best) in one more
//                             LDS float per (row, lane): maximum first, sum second, the order of the wide multi-scale kernel.
// Both sum in class order in f32.  *threshold is read from device memory (a captured step follows a threshold schedule).  The
// kept pixels are counted per lane in an integer register, summed per block in one LDS word, and leave the block as ONE 64-bit
// integer atomic on kept[b] (a block lies in one sample): integer adds commute, so the count is exact and the same on every run.
// No float atomics, no host read-back.
#include "headgeom.h"

// as loss.hip: the instance for a pitch below CP skips the 4-channel groups that start at or past C
#define TSS_WITH_ROW_GUARD(cond, ...)                         \
  do {                                                        \
    if (cond) { constexpr bool GUARDV = true; __VA_ARGS__; }  \
    else { constexpr bool GUARDV = false; __VA_ARGS__; }      \
  } while (0)

namespace {

constexpr int WK = 16;            // classes per chunk, as widehead.hip
constexpr int WMAXC = 256;

// widehead.hip's blend and chunk loader (file-local there), restated: ONE spelling of the roundings, fma(l0, a, round(l1 b))
__device__ __forceinline__ float wide_blend(float l0, float a, float l1, float b) { return __builtin_fmaf(l0, a, l1 * b); }

template <typename T>
__device__ __forceinline__ void wide_load_row(const T* p0, const T* p1, const Tap tx, int c0, int C, float* a) {
#pragma unroll
  for (int c8 = 0; c8 < WK; c8 += 8) {
    float u[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c0 + c8 < C) {                           // uniform
      V8<T>::load(p0 + c0 + c8, u);
      V8<T>::load(p1 + c0 + c8, v);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) a[c8 + q] = (c0 + c8 + q < C) ? wide_blend(tx.l0, u[q], tx.l1, v[q]) : 0.f;   // pad channels hold anything
  }
}

// the block's kept pixels -> kept[b]: lane counts -> one LDS word -> one 64-bit atomic
__device__ __forceinline__ void kept_out(unsigned int* skept, unsigned int mine, unsigned long long* kept, long b) {
  if (!kept) return;                             // uniform
  if (mine) atomicAdd(skept, mine);
  __syncthreads();
  if (threadIdx.x == 0 && *skept) atomicAdd(kept + b, (unsigned long long)*skept);
}

template <typename T, int CP, bool GUARD>
__global__ __launch_bounds__(NT, 3) void pseudo_label_kernel(const T* low, long ldl, const float* threshold, unsigned char* label,
                                                             float* conf, unsigned long long* kept, int B, int C, int h, int w,
                                                             int H, int W, int ignore_index, int band_rows) {
  __shared__ unsigned int skept;
  const int tid = threadIdx.x;
  if (tid == 0) skept = 0u;
  __syncthreads();
  const float thr = *threshold;
  // the block set-up of upsample_argmax_kernel, written out as there
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
  unsigned int mine = 0u;
  for (int y = ya; y < yb; ++y) {
    const Tap ty = ac_tap(sy, y, h);
    if (ty.i0 != rA) {
      rA = rB;
      rB = rA + (rA < h - 1 ? 1 : 0);
#pragma unroll
      for (int c = 0; c < CP; ++c) aA[c] = aB[c];
      load_row(rB, aB);
    }
    float zs[CP];
    float best = -TSS_INF;
    int arg = 0;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const float z = ty.l0 * aA[c] + ty.l1 * aB[c];
      zs[c] = z;
      if (c < C && (z > best || c == 0)) { best = z; arg = c; }
    }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c)
      if (c < C) s += __expf(zs[c] - best);    // class order; s >= 1: the best class adds exp(0)
    const float cf = 1.f / s;
    if (xin) {
      const long p = (b * H + y) * (long)W + x;
      const bool keep = cf >= thr;
      label[p] = (unsigned char)(keep ? arg : ignore_index);
      if (conf) conf[p] = cf;
      mine += keep ? 1u : 0u;
    }
  }
  kept_out(&skept, mine, kept, b);
}

constexpr size_t wide_pseudo_lds_bytes() { return sizeof(float) * 2 * WROWS * NT + WROWS * NT + 16; }

template <typename T>
__global__ __launch_bounds__(NT, 2) void wide_pseudo_label_kernel(const T* low, long ldl, const float* threshold, unsigned char* label,
                                                                  float* conf, unsigned long long* kept, int C, int h, int w,
                                                                  int H, int W, int ignore_index) {
  extern __shared__ __align__(16) unsigned char wlds[];
  float* const Bs = reinterpret_cast<float*>(wlds);                                  // [WROWS][NT] best score
  float* const Ss = Bs + WROWS * NT;                                                 // [WROWS][NT] sum of exp(z - best)
  unsigned int* const skept = reinterpret_cast<unsigned int*>(Ss + WROWS * NT);      // [1] (+ 3 words of padding)
  unsigned char* const Bi = reinterpret_cast<unsigned char*>(skept + 4);             // [WROWS][NT] best index
  const int tid = threadIdx.x;
  if (tid == 0) *skept = 0u;
  __syncthreads();
  const float thr = *threshold;
  const HeadBlock blk = head_block((W + NT - 1) / NT, (H + WROWS - 1) / WROWS, WROWS, H, W);
  const HeadTaps map = head_taps(blk, h, w, H, W);
  const long b = blk.b;
  const int x = blk.x, ya = blk.ya, yb = blk.yb;
  const bool xin = blk.xin;
  const float sy = map.sy;
  const Tap tx = map.tx;
  const T* const img = low + b * h * (long)w * ldl;
  auto load_row = [&](int r, int c0, float* a) {
    wide_load_row<T>(img + ((long)r * w + tx.i0) * ldl, img + ((long)r * w + tx.i1) * ldl, tx, c0, C, a);
  };
  const int r_first = ac_tap(sy, ya, h).i0;
  // walk 1: wide_upsample_argmax_kernel's, (best, index) of every (row, lane); walk 2: the sum against the finished maximum.
  // Every lane reads and writes only its own LDS cells (column tid): no barrier between the walks.
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    for (int c0 = 0; c0 < C; c0 += WK) {
      int rA = r_first;
      int rB = rA + (rA < h - 1 ? 1 : 0);
      float aA[WK], aB[WK];
      load_row(rA, c0, aA);
      load_row(rB, c0, aB);
      for (int y = ya; y < yb; ++y) {
        const int j = y - ya;
        const Tap ty = ac_tap(sy, y, h);
        while (rA < ty.i0) {
          rA = rB;
          rB = rA + (rA < h - 1 ? 1 : 0);
#pragma unroll
          for (int c = 0; c < WK; ++c) aA[c] = aB[c];
          load_row(rB, c0, aB);
        }
        if (pass == 0) {
          float best = c0 ? Bs[j * NT + tid] : -TSS_INF;
          int arg = c0 ? (int)Bi[j * NT + tid] : 0;
#pragma unroll
          for (int c = 0; c < WK; ++c) {
            const float z = wide_blend(ty.l0, aA[c], ty.l1, aB[c]);
            if (c0 + c < C && (z > best || c0 + c == 0)) { best = z; arg = c0 + c; }
          }
          Bs[j * NT + tid] = best;
          Bi[j * NT + tid] = (unsigned char)arg;
        } else {
          const float best = Bs[j * NT + tid];
          float s = c0 ? Ss[j * NT + tid] : 0.f;
#pragma unroll
          for (int c = 0; c < WK; ++c) {
            const float z = wide_blend(ty.l0, aA[c], ty.l1, aB[c]);
            if (c0 + c < C) s += __expf(z - best);     // class order, across chunks too
          }
          Ss[j * NT + tid] = s;
        }
      }
    }
  }
  unsigned int mine = 0u;
  if (xin) {
    for (int y = ya; y < yb; ++y) {
      const int j = y - ya;
      const float cf = 1.f / Ss[j * NT + tid];
      const bool keep = cf >= thr;
      const long p = (b * H + y) * (long)W + x;
      label[p] = (unsigned char)(keep ? (int)Bi[j * NT + tid] : ignore_index);
      if (conf) conf[p] = cf;
      mine += keep ? 1u : 0u;
    }
  }
  kept_out(skept, mine, kept, b);
}

// what both entries ask beyond head_shape_ok: a label byte that is no class
inline bool pseudo_args_ok(int B, int C, int ignore_index, const float* threshold, const unsigned char* label) {
  return B >= 0 && ignore_index >= C && ignore_index <= 255 && threshold && label;
}

}  // namespace

extern "C" {

int tss_upsample_pseudo_label(const void* low, long ldl, const float* threshold, unsigned char* label, float* conf,
                              unsigned long long* kept, int B, int C, int h, int w, int H, int W, int ignore_index, int dtype,
                              void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, 24, ldl, h, w, H, W) && pseudo_args_ok(B, C, ignore_index, threshold, label), TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, false);     // the bands of tss_upsample_argmax_confusion
  const long grid = head_blocks(B, geo);
  TSS_REQUIRE(grid <= 0x7fffffffL, TSS_ERR_SHAPE);
  tss::ProfScope prof(TSS_K_PSEUDO_LABEL, (hipStream_t)stream,
                      (double)B * h * w * C * tss::esz(dtype) + (double)B * H * W * (conf ? 5.0 : 1.0), 0);
  TSS_WITH_DTYPE(dtype, TSS_WITH_CLASS_REGS(C, TSS_WITH_ROW_GUARD(ldl < CPV,
    hipLaunchKernelGGL((pseudo_label_kernel<TT, CPV, GUARDV>), dim3((int)grid), dim3(NT), 0, (hipStream_t)stream,
                       (const TT*)low, ldl, threshold, label, conf, kept, B, C, h, w, H, W, ignore_index, geo.band_rows))));
  return tss::check_last("upsample_pseudo_label");
}

int tss_upsample_pseudo_label_wide(const void* low, long ldl, const float* threshold, unsigned char* label, float* conf,
                                   unsigned long long* kept, int B, int C, int h, int w, int H, int W, int ignore_index, int dtype,
                                   void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, WMAXC, ldl, h, w, H, W) && pseudo_args_ok(B, C, ignore_index, threshold, label), TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const long grid = (long)B * ((W + NT - 1) / NT) * ((H + WROWS - 1) / WROWS);
  TSS_REQUIRE(grid <= 0x7fffffffL, TSS_ERR_SHAPE);
  tss::ProfScope prof(TSS_K_WIDE_PSEUDO_LABEL, (hipStream_t)stream,
                      2.0 * B * h * w * C * tss::esz(dtype) + (double)B * H * W * (conf ? 5.0 : 1.0), 0);
  TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL((wide_pseudo_label_kernel<TT>), dim3((int)grid), dim3(NT), wide_pseudo_lds_bytes(),
                                           (hipStream_t)stream, (const TT*)low, ldl, threshold, label, conf, kept, C, h, w, H, W,
                                           ignore_index));
  return tss::check_last("upsample_pseudo_label_wide");
}

}  // extern "C"
