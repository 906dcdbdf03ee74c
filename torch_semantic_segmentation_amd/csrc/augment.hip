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

// One thread = 8 consecutive output pixels of one output row: all C channel planes of the image and the label row segment.
// The vertical tap is computed once per thread; stores are 16-byte vectors, source reads are byte gathers.
__global__ __launch_bounds__(256) void augment_u8_kernel(const unsigned char* __restrict__ image, int hwc, float* __restrict__ image_out,
                                                         const unsigned char* __restrict__ target, long long* __restrict__ target_out,
                                                         const int* __restrict__ params, unsigned groups, int C, int H, int W, int ch, int cw,
                                                         float3 scale, float3 shift) {
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
          v[c][j] = g * sc + sh;
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
      l[j] = (long long)r[nearest_index(ox + (flip ? cw - 1 - xo : xo), W, Ws)];
    }
    long long* o = target_out + ((long)row * cw + x_out);
#pragma unroll
    for (int j = 0; j < 8; j += 2) *reinterpret_cast<longlong2*>(o + j) = make_longlong2(l[j], l[j + 1]);
  }
}

}  // namespace

extern "C" {

int tss_augment_batch_u8(const unsigned char* image, int image_is_hwc, const float* mean3, const float* std3, float* image_out,
                         const unsigned char* target, long long* target_out, const int* params, long B, int C, int H, int W,
                         int crop_h, int crop_w, void* stream) {
  TSS_REQUIRE(B >= 0 && C >= 1 && C <= 3 && H >= 1 && H <= 8192 && W >= 1 && W <= 8192 && crop_h >= 1 && crop_h <= 8192 &&
              crop_w >= 8 && crop_w <= 8192 && (crop_w % 8) == 0, TSS_ERR_SHAPE);
  TSS_REQUIRE((!image || (image_out && tss::aligned16(image_out))) && (!target || (target_out && tss::aligned16(target_out))) &&
              (reinterpret_cast<uintptr_t>(params) & 3u) == 0, TSS_ERR_ALIGN);
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
  hipLaunchKernelGGL(augment_u8_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, image, image_is_hwc, image_out, target,
                     target_out, params, (unsigned)groups, C, H, W, crop_h, crop_w, make_float3(sc[0], sc[1], sc[2]),
                     make_float3(sh[0], sh[1], sh[2]));
  return tss::check_last("augment_batch_u8");
}

}  // extern "C"
