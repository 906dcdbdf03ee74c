// Photometric strong augmentation of the student's unlabelled input (ClassMix / DACS / CutMix-Seg / FixMatch): colour jitter and
// Gaussian blur of a NORMALISED batch on the device, so that it sits in the captured step behind the mix.  Per sample three rows in
// device memory: color (apply, fb, fc, fs, dh, 0, 0, 0), radius R in [0, 8], taps (w_0 .. w_8, 0, 0, 0).
//   strongaug_stats_kernel  the contrast step needs the mean grey value m of the sample AFTER brightness: block (part, b) denormalises
//                           its 64th of the sample, applies brightness, forms the grey value per pixel in f32 and sums it in f64;
//                           one f64 partial per block, plain stores, no atomics.  A sample with apply == 0 returns without reading.
//   strongaug_tile_kernel   block = one STRONGAUG_TH x STRONGAUG_TW output tile of one sample.  It loads the tile plus a halo of the
//                           sample's own R with mirrored indices, jitters every pixel on load (the three channels of a pixel in one
//                           thread), keeps the jittered tile in LDS, blurs horizontally into a second LDS buffer and vertically into
//                           registers, renormalises and stores 16-byte vectors.  Every wave re-adds the sample's 64 partials with the
//                           same butterfly, so every block of a sample sees the same m.  apply == 0 && R == 0: a copy on bits.
// No jittered or half-blurred image exists in memory.  Two launches, no float atomics, no host read-back: capturable, and the same
// bits on every run.
#include <float.h>

#include "common.h"

namespace {

constexpr int TH = TSS_STRONGAUG_TH, TW = TSS_STRONGAUG_TW;
constexpr int RMAX = 8;
constexpr int LH = TH + 2 * RMAX, LW = TW + 2 * RMAX;     // the loaded tile at R = 8: 48 x 48
constexpr int PARTS = 64;                                  // f64 partial rows per sample = lanes of a wave
// LDS: 3 x 48 x 48 + 3 x 48 x 32 floats = 46080 bytes: three blocks per CU (160 KiB) at any radius

struct Consts { float3 mean, std, isd, shift; };           // u = x std + mean;  x' = v isd + shift, isd = 1/std, shift = -mean/std

// hsv_shift of augment.hip, restated (same operations in the same order; there it serves the 8-bit pipeline).
//   V = max, D = V - min, S = 255 D / V (0 at V = 0), H = 0 at D = 0, else 30 (g-b)/D | 60 + 30 (b-r)/D | 120 + 30 (r-g)/D for
//   V == r | g | b (first match), + 180 when negative;  H' = H + dh wrapped once into [0, 180), S' and V' clamped to [0, 255];
//   back with the six-sector formula on h = H'/30.  |dh| <= 180.  D = 0 and ds = 0 return (V', V', V') exactly.
__device__ __forceinline__ void hsv_shift(float& r, float& g, float& b, float dh, float ds, float dv) {
  const float V = fmaxf(r, fmaxf(g, b)), D = V - fminf(r, fminf(g, b));
  const float S = 255.f * D / fmaxf(V, FLT_MIN);
  const bool vr = V == r, vg = V == g;
  const float gb = g - b, br = b - r, rg = r - g;
  const float num = vr ? gb : (vg ? br : rg);
  const float base = vr ? 0.f : (vg ? 60.f : 120.f);
  float H = base + 30.f * num / fmaxf(D, FLT_MIN);
  H = H < 0.f ? H + 180.f : H;
  H += dh;
  H = H < 0.f ? H + 180.f : (H >= 180.f ? H - 180.f : H);
  const float h = H / 30.f, fl = floorf(h), f = h - fl;
  const int i = (int)fl;                               // 0..6
  const float V2 = clamp3(V + dv, 0.f, 255.f), s = clamp3(S + ds, 0.f, 255.f) / 255.f;
  const float p = V2 * (1.f - s), q = V2 * (1.f - f * s), t = V2 * (1.f - (1.f - f) * s);
  r = ((i == 0) | (i >= 5)) ? V2 : (i == 1 ? q : (i == 4 ? t : p));
  g = ((i == 1) | (i == 2)) ? V2 : (((i == 0) | (i == 6)) ? t : (i == 3 ? q : p));
  b = ((i == 3) | (i == 4)) ? V2 : (i == 2 ? t : (i == 5 ? q : p));
}

__device__ __forceinline__ float grey_of(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b; }

// mirror reflection without repeating the edge pixel (-1 -> 1, n -> n - 2); the clamp keeps the rows and columns that a ragged
// last tile loads past the halo, and never uses, inside the image
__device__ __forceinline__ int refl(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

__device__ __forceinline__ float load1(const float* p) { return *p; }
__device__ __forceinline__ float load1(const bf16_t* p) { return __uint_as_float((uint32_t)(*reinterpret_cast<const unsigned short*>(p)) << 16); }

// one 16-byte output vector: 4 float | 8 bf16
template <typename T> struct Out;
template <> struct Out<float> {
  static constexpr int VEC = 4;
  static __device__ __forceinline__ void store(float* p, const float v[4]) { V4<float>::store(p, v); }
};
template <> struct Out<bf16_t> {
  static constexpr int VEC = 8;
  static __device__ __forceinline__ void store(bf16_t* p, const float v[8]) { V8<bf16_t>::store(p, v); }
};

template <typename T>
__global__ __launch_bounds__(256) void strongaug_stats_kernel(const T* __restrict__ image, const float* __restrict__ color,
                                                              double* __restrict__ ws, long HW, Consts k) {
  __shared__ double part[4];
  const long b = blockIdx.y;
  if (color[b * 8] == 0.f) return;                         // uniform: the whole block leaves, the sample's rows stay unwritten
  const float fb = color[b * 8 + 1];
  const long groups = HW / 8, per = (groups + PARTS - 1) / PARTS;
  const long g0 = (long)blockIdx.x * per, g1 = g0 + per < groups ? g0 + per : groups;
  const T* const base = image + b * 3 * HW;
  double acc = 0.0;
  for (long g = g0 + threadIdx.x; g < g1; g += 256) {
    float r[8], gg[8], bl[8];
    V8<T>::load(base + g * 8, r);
    V8<T>::load(base + HW + g * 8, gg);
    V8<T>::load(base + 2 * HW + g * 8, bl);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float ur = clamp3((r[j] * k.std.x + k.mean.x) * fb, 0.f, 1.f);
      const float ug = clamp3((gg[j] * k.std.y + k.mean.y) * fb, 0.f, 1.f);
      const float ub = clamp3((bl[j] * k.std.z + k.mean.z) * fb, 0.f, 1.f);
      acc += (double)grey_of(ur, ug, ub);
    }
  }
  acc = wave_sum(acc);                                     // a fixed butterfly, then the four waves in ascending order
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) ws[b * PARTS + blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

template <typename T>
__global__ __launch_bounds__(256) void strongaug_tile_kernel(const T* __restrict__ image, T* __restrict__ out,
                                                             const float* __restrict__ color, const int* __restrict__ radius,
                                                             const float* __restrict__ taps, const double* __restrict__ ws, int H, int W,
                                                             Consts k) {
  __shared__ float s_in[3][LH][LW];
  __shared__ __attribute__((aligned(16))) float s_h[3][LH][TW];
  constexpr int VEC = Out<T>::VEC;
  const int tid = threadIdx.x;
  const long b = blockIdx.z;
  const int ty0 = blockIdx.y * TH, tx0 = blockIdx.x * TW;
  const long HW = (long)H * W;
  const T* const src = image + b * 3 * HW;
  T* const dst = out + b * 3 * HW;

  // the sample's rows: uniform in the block, read once (device rows are clamped into range, not validated)
  const bool apply = color[b * 8] != 0.f;
  int R = radius[b];
  R = R < 0 ? 0 : (R > RMAX ? RMAX : R);

  if (!apply && R == 0) {                                  // identity: the tile on bits (a NaN stays the NaN it was)
    for (int u = tid; u < 3 * TH * (TW / VEC); u += 256) {
      const int xg = u % (TW / VEC), y = (u / (TW / VEC)) % TH, c = u / (TH * (TW / VEC));
      const int gy = ty0 + y, gx = tx0 + xg * VEC;
      if (gy < H && gx < W) {
        const long at = c * HW + (long)gy * W + gx;
        *reinterpret_cast<uint4*>(dst + at) = *reinterpret_cast<const uint4*>(src + at);
      }
    }
    return;
  }

  const float fb = color[b * 8 + 1], fc = color[b * 8 + 2], fs = color[b * 8 + 3];
  const float dh = 180.f * clamp3(color[b * 8 + 4], -0.5f, 0.5f);
  float w[RMAX + 1];
#pragma unroll
  for (int j = 0; j <= RMAX; ++j) w[j] = taps[b * 12 + j];
  float m = 0.f;
  if (apply) {                                             // the same 64 partials, the same butterfly in every wave of every block
    const double s = wave_sum(ws[b * PARTS + (tid & 63)]);
    m = (float)(s / (double)HW);
  }

  // load + jitter: (TH + 2R) x (TW + 2R) pixels with mirrored indices
  const int lh = TH + 2 * R, lw = TW + 2 * R;
  for (int p = tid; p < lh * lw; p += 256) {
    const int ly = p / lw, lx = p - ly * lw;
    const long at = (long)refl(ty0 + ly - R, H) * W + refl(tx0 + lx - R, W);
    float r = load1(src + at) * k.std.x + k.mean.x;
    float g = load1(src + HW + at) * k.std.y + k.mean.y;
    float bl = load1(src + 2 * HW + at) * k.std.z + k.mean.z;
    if (apply) {
      r = clamp3(r * fb, 0.f, 1.f); g = clamp3(g * fb, 0.f, 1.f); bl = clamp3(bl * fb, 0.f, 1.f);
      r = clamp3(m + fc * (r - m), 0.f, 1.f); g = clamp3(m + fc * (g - m), 0.f, 1.f); bl = clamp3(m + fc * (bl - m), 0.f, 1.f);
      const float y = grey_of(r, g, bl);
      r = clamp3(y + fs * (r - y), 0.f, 1.f); g = clamp3(y + fs * (g - y), 0.f, 1.f); bl = clamp3(y + fs * (bl - y), 0.f, 1.f);
      r *= 255.f; g *= 255.f; bl *= 255.f;
      hsv_shift(r, g, bl, dh, 0.f, 0.f);
      r /= 255.f; g /= 255.f; bl /= 255.f;
    }
    s_in[0][ly][lx] = r; s_in[1][ly][lx] = g; s_in[2][ly][lx] = bl;
  }
  __syncthreads();

  // horizontal pass: rows 0 .. lh-1, output columns 0 .. TW-1 (centre at lx = x + R)
  for (int u = tid; u < 3 * lh * TW; u += 256) {
    const int x = u % TW, ly = (u / TW) % lh, c = u / (TW * lh);
    const float* const row = &s_in[c][ly][x + R];
    float acc = row[0];
    if (R > 0) {
      acc *= w[0];
#pragma unroll
      for (int j = 1; j <= RMAX; ++j)
        if (j <= R) acc += w[j] * (row[-j] + row[j]);
    }
    s_h[c][ly][x] = acc;
  }
  __syncthreads();

  // vertical pass into registers, renormalise, store
  for (int u = tid; u < 3 * TH * (TW / VEC); u += 256) {
    const int xg = u % (TW / VEC), y = (u / (TW / VEC)) % TH, c = u / (TH * (TW / VEC));
    const int gy = ty0 + y, gx = tx0 + xg * VEC;
    if (gy >= H || gx >= W) continue;
    float v[VEC];
#pragma unroll
    for (int q = 0; q < VEC; q += 4) {
      const float4 a = *reinterpret_cast<const float4*>(&s_h[c][y + R][xg * VEC + q]);
      v[q] = a.x; v[q + 1] = a.y; v[q + 2] = a.z; v[q + 3] = a.w;
    }
    if (R > 0) {
#pragma unroll
      for (int q = 0; q < VEC; ++q) v[q] *= w[0];
#pragma unroll
      for (int j = 1; j <= RMAX; ++j) {
        if (j <= R) {
#pragma unroll
          for (int q = 0; q < VEC; q += 4) {
            const float4 lo = *reinterpret_cast<const float4*>(&s_h[c][y + R - j][xg * VEC + q]);
            const float4 hi = *reinterpret_cast<const float4*>(&s_h[c][y + R + j][xg * VEC + q]);
            v[q] += w[j] * (lo.x + hi.x); v[q + 1] += w[j] * (lo.y + hi.y);
            v[q + 2] += w[j] * (lo.z + hi.z); v[q + 3] += w[j] * (lo.w + hi.w);
          }
        }
      }
    }
    const float isd = c == 0 ? k.isd.x : (c == 1 ? k.isd.y : k.isd.z);
    const float sh = c == 0 ? k.shift.x : (c == 1 ? k.shift.y : k.shift.z);
#pragma unroll
    for (int q = 0; q < VEC; ++q) v[q] = v[q] * isd + sh;
    Out<T>::store(dst + c * HW + (long)gy * W + gx, v);
  }
}

bool shape_ok(long B, int H, int W) { return B >= 0 && B <= 65535 && H >= 9 && H <= 32768 && W >= 16 && W <= 32768 && (W % 8) == 0; }

}  // namespace

extern "C" {

int tss_strong_augment_tile(int* th, int* tw) {
  if (th) *th = TH;
  if (tw) *tw = TW;
  return TSS_OK;
}

long tss_strong_augment_ws(long B, int H, int W) {
  if (!shape_ok(B, H, W)) return -1;
  return B * PARTS * (long)sizeof(double);
}

int tss_strong_augment(const void* image, void* out, const float* color, const int* radius, const float* taps, const float* mean3,
                       const float* std3, void* ws, long B, int Ci, int H, int W, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(Ci == 3 && shape_ok(B, H, W), TSS_ERR_SHAPE);
  if (B == 0) return TSS_OK;
  TSS_REQUIRE(image && out && color && radius && taps && ws && image != out, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(image) && tss::aligned16(out) && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0 &&
              (reinterpret_cast<uintptr_t>(color) & 3u) == 0 && (reinterpret_cast<uintptr_t>(radius) & 3u) == 0 &&
              (reinterpret_cast<uintptr_t>(taps) & 3u) == 0, TSS_ERR_ALIGN);
  Consts k;
  float mean[3], sd[3], isd[3], sh[3];
  for (int c = 0; c < 3; ++c) {                            // host floats, as tss_augment_batch_u8 forms scale / shift
    mean[c] = mean3 ? mean3[c] : 0.f; sd[c] = std3 ? std3[c] : 1.f;
    isd[c] = 1.f / sd[c]; sh[c] = -mean[c] / sd[c];
  }
  k.mean = make_float3(mean[0], mean[1], mean[2]); k.std = make_float3(sd[0], sd[1], sd[2]);
  k.isd = make_float3(isd[0], isd[1], isd[2]); k.shift = make_float3(sh[0], sh[1], sh[2]);
  const long HW = (long)H * W;
  const dim3 tiles((W + TW - 1) / TW, (H + TH - 1) / TH, (int)B);
  TSS_WITH_DTYPE(dtype, {
    hipLaunchKernelGGL(strongaug_stats_kernel<TT>, dim3(PARTS, (int)B), dim3(256), 0, (hipStream_t)stream, (const TT*)image, color,
                       (double*)ws, HW, k);
    hipLaunchKernelGGL(strongaug_tile_kernel<TT>, tiles, dim3(256), 0, (hipStream_t)stream, (const TT*)image, (TT*)out, color, radius,
                       taps, (const double*)ws, H, W, k);
  });
  return tss::check_last("strong_augment");
}

}  // extern "C"
