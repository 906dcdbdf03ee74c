// Device-side train augmentation (scripts/train_fastscnn.py:62-68: RandomScale -> RandomCrop -> HorizontalFlip -> Normalize ->
// ToTensor): the loader ships the undecorated uint8 frame and uint8 label map, and ONE gather kernel at the top of the
// (captured) step writes the float32 NCHW crop and the int64 target crop the step reads.  Scale, crop origin and flip are
// per-sample rows in device memory, so one captured graph serves every step.
//
// Output pixel (y, x) of sample b with row (Hs, Ws, oy, ox, flip, 0) takes scaled-image pixel Y = oy + y,
// X = ox + (flip ? cw-1-x : x).  Image: bilinear with half-pixel centres and clamped edges (cv2.INTER_LINEAR,
// F.interpolate(align_corners=False)) in INTEGER coordinates: n = (2X+1) W - Ws, x0 = floor(n / 2Ws), weight = (n - x0 2Ws) / 2Ws
// (numerator and denominator exact in f32: one rounding), x1 = x0 + 1, both clamped.  The four uint8 texels are blended in
// f32 and NOT re-quantised to uint8 (cv2 rounds to a grey level there: at most half a grey level apart, on purpose).
// Labels: nearest as cv2.INTER_NEAREST, xs = min(floor(X W / Ws), W-1), integer arithmetic only.
// Every intermediate fits in int32 for sizes up to 8192 ((2X+1) W <= 2^27 + 2^13).
//
// tss_augment_batch_u8_ex is the same launch for scripts/contextnet/train_contextnet.py's pipeline (... HorizontalFlip ->
// HueSaturationValue -> Normalize ...) and for the datasets' TRAIN_MAPPING[label]: a per-sample row (apply, dh, ds, dv) shifts the
// blended (r, g, b) in HSV, on cv2's 8-bit scale kept continuous, in the registers that hold the blend; the nearest-sampled label
// byte goes through a 256-byte table (read through the cache: 8 dependent byte loads per thread next to about a hundred texel
// loads) before it is widened.  Both entries instantiate one kernel body; without colour rows and table they agree bit for bit.
#include <float.h>

#include "common.h"

namespace {

struct AxisTap { int i0, i1; float w1; };

// half-pixel bilinear tap of scaled coordinate `dst` (size `scaled`) on a source axis of `in` texels.  n > -scaled always, so
// n + 2 scaled > 0 and the true floor is one unsigned division.  The clamps also keep a bad parameter row inside the source.
__device__ __forceinline__ AxisTap half_pixel_tap(int dst, int in, int scaled) {
  const int d = 2 * scaled;
  const int n = (2 * dst + 1) * in - scaled;
  const int q = (int)((unsigned)(n + d) / (unsigned)d) - 1;
  AxisTap t;
  t.w1 = (float)(n - q * d) / (float)d;
  t.i0 = min(max(q, 0), in - 1);
  t.i1 = min(max(q + 1, 0), in - 1);
  return t;
}

__device__ __forceinline__ int nearest_index(int dst, int in, int scaled) {
  return min(max((int)((unsigned)(dst * in) / (unsigned)scaled), 0), in - 1);
}

__device__ __forceinline__ float lerp2(float a, float b, float w0, float w1) { return a * w0 + b * w1; }

// albumentations' HueSaturationValue (additive shifts on cv2's 8-bit HSV scale: H in [0, 180) in units of 2 degrees, S and V in
// [0, 255]) of one pixel in grey levels, kept continuous: neither H, S, V nor the result is rounded to uint8.
//   V = max, D = V - min, S = 255 D / V (0 at V = 0), H = 0 at D = 0, else 30 (g-b)/D | 60 + 30 (b-r)/D | 120 + 30 (r-g)/D for
//   V == r | g | b (first match), + 180 when negative;  H' = H + dh wrapped once into [0, 180), S' and V' clamped to [0, 255];
//   back with the six-sector formula on h = H'/30.  |dh| <= 180 (host check).  IEEE divisions; every intermediate is finite for
// finite input.  H' can ROUND to 180 (a tiny negative H + 180): sector 6 is sector 0, where f = 0 gives the same colour.
// A grey pixel has H = 0, so ds > 0 tints it red, as the reference does.  D = 0 and ds = 0 return (V', V', V') exactly.
__device__ __forceinline__ void hsv_shift(float& r, float& g, float& b, float dh, float ds, float dv) {
  const float V = fmaxf(r, fmaxf(g, b)), D = V - fminf(r, fminf(g, b));
  // V = 0 has D = 0 and D = 0 has V == r, num = 0: dividing by the smallest normal number instead gives the S = 0 and H = 0 of
  // the definition without a branch around the division, and changes nothing else (a positive V or D is a blend of bytes, or one
  // rounding of it: thirty orders of magnitude above that number)
  const float S = 255.f * D / fmaxf(V, FLT_MIN);
  const bool vr = V == r, vg = V == g;
  const float gb = g - b, br = b - r, rg = r - g;    // all three, then selects: no branch per pixel
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
  //            sector  0 (6)       1           2           3           4           5
  //                   (V', t, p)  (q, V', p)  (p, V', t)  (p, q, V')  (t, p, V')  (V', p, q)
  r = ((i == 0) | (i >= 5)) ? V2 : (i == 1 ? q : (i == 4 ? t : p));
  g = ((i == 1) | (i == 2)) ? V2 : (((i == 0) | (i == 6)) ? t : (i == 3 ? q : p));
  b = ((i == 3) | (i == 4)) ? V2 : (i == 2 ? t : (i == 5 ? q : p));
}

// One thread = 8 consecutive output pixels of one output row: all C channel planes of the image and the label row segment.
// The vertical tap is computed once per thread; stores are 16-byte vectors, source reads are byte gathers.
// EX: the sample's colour row (color != NULL, C == 3: host check) and the label table (lut != NULL); both NULL = the plain kernel.
template <bool EX>
__global__ __launch_bounds__(256) void augment_u8_kernel(const unsigned char* __restrict__ image, int hwc, float* __restrict__ image_out,
                                                         const unsigned char* __restrict__ target, long long* __restrict__ target_out,
                                                         const int* __restrict__ params, unsigned groups, int C, int H, int W, int ch, int cw,
                                                         float3 scale, float3 shift, const int* __restrict__ color,
                                                         const unsigned char* __restrict__ lut) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;      // groups < 2^31 (host check): 32-bit index arithmetic
  if (i >= groups) return;
  const unsigned gpr = (unsigned)cw >> 3;
  const unsigned row = i / gpr;
  const int x_out = (int)(i - row * gpr) * 8;
  const long b = row / (unsigned)ch;
  const int y = (int)(row - (unsigned)b * (unsigned)ch);
  const int* p = params + b * 6;
  const int Hs = p[0], Ws = p[1], oy = p[2], ox = p[3], flip = p[4];
  const int Y = oy + y;
  const long HW = (long)H * W;

  if (image) {
    const AxisTap ty = half_pixel_tap(Y, H, Hs);
    const float wy1 = ty.w1, wy0 = 1.f - wy1;
    const int pix = hwc ? C : 1;                     // byte distance of neighbouring texels / of the channels of one texel
    const long chan = hwc ? 1 : HW;
    const unsigned char* r0 = image + b * HW * C + (long)ty.i0 * W * pix;
    const unsigned char* r1 = image + b * HW * C + (long)ty.i1 * W * pix;
    float v[3][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int xo = x_out + j;
      const AxisTap tx = half_pixel_tap(ox + (flip ? cw - 1 - xo : xo), W, Ws);
      const float wx1 = tx.w1, wx0 = 1.f - wx1;
      const int a0 = tx.i0 * pix, a1 = tx.i1 * pix;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (c < C) {
          const float t00 = (float)r0[a0 + c * chan], t01 = (float)r0[a1 + c * chan];
          const float t10 = (float)r1[a0 + c * chan], t11 = (float)r1[a1 + c * chan];
          const float g = lerp2(lerp2(t00, t01, wx0, wx1), lerp2(t10, t11, wx0, wx1), wy0, wy1);
          const float sc = c == 0 ? scale.x : (c == 1 ? scale.y : scale.z);
          const float sh = c == 0 ? shift.x : (c == 1 ? shift.y : shift.z);
          v[c][j] = EX ? g : g * sc + sh;            // EX: the blend stays in grey levels until the colour row has been applied
        }
      }
    }
    if constexpr (EX) {
      if (color && color[b * 4] != 0) {              // per sample: uniform in all but the waves that straddle two samples
        const float dh = (float)color[b * 4 + 1], ds = (float)color[b * 4 + 2], dv = (float)color[b * 4 + 3];
#pragma unroll
        for (int j = 0; j < 8; ++j) hsv_shift(v[0][j], v[1][j], v[2][j], dh, ds, dv);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (c < C) {
          const float sc = c == 0 ? scale.x : (c == 1 ? scale.y : scale.z);
          const float sh = c == 0 ? shift.x : (c == 1 ? shift.y : shift.z);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[c][j] = v[c][j] * sc + sh;
        }
      }
    }
    float* o = image_out + ((b * C * ch + y) * (long)cw + x_out);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (c < C) V8<float>::store(o + (long)c * ch * cw, v[c]);
  }

  if (target) {
    const unsigned char* r = target + b * HW + (long)nearest_index(Y, H, Hs) * W;
    long long l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int xo = x_out + j;
      unsigned char t = r[nearest_index(ox + (flip ? cw - 1 - xo : xo), W, Ws)];
      if constexpr (EX) {
        if (lut) t = lut[t];
      }
      l[j] = (long long)t;
    }
    long long* o = target_out + ((long)row * cw + x_out);
#pragma unroll
    for (int j = 0; j < 8; j += 2) *reinterpret_cast<longlong2*>(o + j) = make_longlong2(l[j], l[j + 1]);
  }
}

// Labels of the evaluation path (no augmentation launch to ride on): out[i] = (int64) lut[target[i]].  One thread = 8 labels:
// one 8-byte load, four 16-byte stores; the last thread takes the n % 8 tail byte by byte.
__global__ __launch_bounds__(256) void remap_labels_kernel(const unsigned char* __restrict__ target, const unsigned char* __restrict__ lut,
                                                           long long* __restrict__ out, long n, unsigned groups) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;      // groups < 2^31 (host check)
  if (i >= groups) return;
  const long at = (long)i * 8;
  if (at + 8 <= n) {
    const uint2 w = *reinterpret_cast<const uint2*>(target + at);
    long long l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) l[j] = (long long)lut[((j < 4 ? w.x : w.y) >> (8 * (j & 3))) & 0xffu];
#pragma unroll
    for (int j = 0; j < 8; j += 2) *reinterpret_cast<longlong2*>(out + at + j) = make_longlong2(l[j], l[j + 1]);
  } else {
    for (long k = at; k < n; ++k) out[k] = (long long)lut[target[k]];
  }
}

int launch_augment(bool ex, const unsigned char* image, int image_is_hwc, const float* mean3, const float* std3, float* image_out,
                   const unsigned char* target, long long* target_out, const int* params, const int* color,
                   const unsigned char* label_lut, long B, int C, int H, int W, int crop_h, int crop_w, void* stream) {
  TSS_REQUIRE(B >= 0 && C >= 1 && C <= 3 && H >= 1 && H <= 8192 && W >= 1 && W <= 8192 && crop_h >= 1 && crop_h <= 8192 &&
              crop_w >= 8 && crop_w <= 8192 && (crop_w % 8) == 0, TSS_ERR_SHAPE);
  TSS_REQUIRE(!color || C == 3, TSS_ERR_SHAPE);    // hue needs (r, g, b)
  TSS_REQUIRE((!image || (image_out && tss::aligned16(image_out))) && (!target || (target_out && tss::aligned16(target_out))) &&
              (reinterpret_cast<uintptr_t>(params) & 3u) == 0 && (reinterpret_cast<uintptr_t>(color) & 3u) == 0, TSS_ERR_ALIGN);
  if (B == 0 || (!image && !target)) return TSS_OK;
  TSS_REQUIRE(params != nullptr, TSS_ERR_SHAPE);
  const long groups = B * crop_h * (long)(crop_w / 8);
  const long grid = (groups + 255) / 256;          // one thread per group, no stride loop: 1536 blocks at 8 x 512 x 768
  TSS_REQUIRE(groups <= 0x7fffffffL, TSS_ERR_SHAPE);
  float sc[3] = {1.f / 255.f, 1.f / 255.f, 1.f / 255.f}, sh[3] = {0.f, 0.f, 0.f};
  for (int c = 0; c < C; ++c) {                    // host arrays, as tss_decode_batch_u8: x * (1/(255 std)) - mean/std
    const float m = mean3 ? mean3[c] : 0.f, s = std3 ? std3[c] : 1.f;
    sc[c] = 1.f / (255.f * s); sh[c] = -m / s;
  }
  hipLaunchKernelGGL(ex ? augment_u8_kernel<true> : augment_u8_kernel<false>, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, image,
                     image_is_hwc, image_out, target, target_out, params, (unsigned)groups, C, H, W, crop_h, crop_w,
                     make_float3(sc[0], sc[1], sc[2]), make_float3(sh[0], sh[1], sh[2]), color, label_lut);
  return tss::check_last(ex ? "augment_batch_u8_ex" : "augment_batch_u8");
}

}  // namespace

extern "C" {

int tss_augment_batch_u8(const unsigned char* image, int image_is_hwc, const float* mean3, const float* std3, float* image_out,
                         const unsigned char* target, long long* target_out, const int* params, long B, int C, int H, int W,
                         int crop_h, int crop_w, void* stream) {
  return launch_augment(false, image, image_is_hwc, mean3, std3, image_out, target, target_out, params, nullptr, nullptr, B, C, H, W,
                        crop_h, crop_w, stream);
}

int tss_augment_batch_u8_ex(const unsigned char* image, int image_is_hwc, const float* mean3, const float* std3, float* image_out,
                            const unsigned char* target, long long* target_out, const int* params, const int* color,
                            const unsigned char* label_lut, long B, int C, int H, int W, int crop_h, int crop_w, void* stream) {
  return launch_augment(true, image, image_is_hwc, mean3, std3, image_out, target, target_out, params, color, label_lut, B, C, H, W,
                        crop_h, crop_w, stream);
}

int tss_remap_labels_u8(const unsigned char* target, const unsigned char* label_lut, long long* out, long n, void* stream) {
  TSS_REQUIRE(n >= 0 && (n + 7) / 8 <= 0x7fffffffL, TSS_ERR_SHAPE);
  if (n == 0) return TSS_OK;
  TSS_REQUIRE(target && label_lut && out, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(out) && (reinterpret_cast<uintptr_t>(target) & 7u) == 0, TSS_ERR_ALIGN);
  const long groups = (n + 7) / 8;
  hipLaunchKernelGGL(remap_labels_kernel, dim3((int)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, target, label_lut, out, n,
                     (unsigned)groups);
  return tss::check_last("remap_labels_u8");
}

}  // extern "C"
