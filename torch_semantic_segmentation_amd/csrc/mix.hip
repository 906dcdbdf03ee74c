// The mixing perturbation of mean-teacher self-training (ClassMix, CutMix, DACS) on the device, so that it can be captured with the
// step: no `unique`, no boolean masks, no host synchronisation.
//   classmix_present_kernel, classmix_rank_kernel
//                           per sample: which classes < C occur in the uint8 label map (eight blocks per sample), their rank by (key,
//                           class index) (unsigned), sel[b][c] = 1 for the ceil(n / 2) present classes of smallest rank.  The host
//                           draws the keys.  Integer only.
//   mix_batch_kernel        mask(b, y, x) = sel[b][label[b][y][x]]  or  y0 <= y < y1 && x0 <= x < x1;  per pixel a select ON BITS between
//                           sample b and sample partner[b] of the image (f32 | bf16 planes) and of the label map (widened to int64):
//                           the value that is not chosen is never looked at (a NaN there stays there), the chosen one arrives bit for
//                           bit.  Thread = 8 consecutive pixels of a row, 16-byte vectors; a group whose 8 pixels all take the same
//                           side reads that side only.  One launch.
#include "common.h"

namespace {

constexpr int SEL_NT = 1024;
constexpr int SEL_PARTS = 8;      // blocks per sample of the presence pass: 8 x 32 bytes of presence bits = the sample's 256 bytes of sel

// Pass 1: block (part, b) marks which byte values occur in its eighth of the sample's map and stores its 256 presence bits (8 words,
// plain stores) into sel[b][32 part ..): the output row doubles as the pass's workspace, nothing is zero-filled, no global atomics.
__global__ __launch_bounds__(SEL_NT) void classmix_present_kernel(const unsigned char* __restrict__ label, unsigned char* __restrict__ sel,
                                                                  long HW) {
  __shared__ unsigned int pres[8];
  const int tid = threadIdx.x;
  const long b = blockIdx.y;
  if (tid < 8) pres[tid] = 0u;
  __syncthreads();
  const long per = ((HW + SEL_PARTS - 1) / SEL_PARTS + 15) / 16 * 16;
  long begin = (long)blockIdx.x * per, end = begin + per;
  begin = begin < HW ? begin : HW;
  end = end < HW ? end : HW;
  const unsigned char* const lab = label + b * HW + begin;
  const long n = end - begin;
  unsigned int last = 256u;                                      // label maps are coherent: most bytes repeat the one before
  auto note = [&](unsigned int v) {
    if (v != last) { last = v; atomicOr(&pres[v >> 5], 1u << (v & 31u)); }
  };
  // head bytes up to 16-byte alignment, 16-byte vectors, tail bytes
  long head = (long)((16u - (unsigned)(reinterpret_cast<uintptr_t>(lab) & 15u)) & 15u);
  if (head > n) head = n;
  const long nvec = (n - head) / 16;
  for (long i = tid; i < head; i += SEL_NT) note(lab[i]);
  for (long i = tid; i < nvec; i += SEL_NT) {
    const uint4 r = *reinterpret_cast<const uint4*>(lab + head + i * 16);
    const unsigned int wv[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) note((wv[q] >> (8 * j)) & 0xffu);
  }
  for (long i = head + nvec * 16 + tid; i < n; i += SEL_NT) note(lab[i]);
  __syncthreads();
  if (tid < 8) reinterpret_cast<unsigned int*>(sel + b * 256)[blockIdx.x * 8 + tid] = pres[tid];
}

// Pass 2: one block of 256 threads per sample ORs the eight parts, ranks the present classes < C by (key, class index), unsigned, and
// overwrites the row with the pick (every thread has read the parts before any byte is written: the barrier).
__global__ __launch_bounds__(256) void classmix_rank_kernel(const unsigned int* __restrict__ keys, unsigned char* __restrict__ sel, int C) {
  __shared__ unsigned int pres[8];
  __shared__ unsigned int skey[256];
  const int c = threadIdx.x;
  const long b = blockIdx.x;
  skey[c] = keys[b * 256 + c];
  if (c < 8) {
    const unsigned int* const parts = reinterpret_cast<const unsigned int*>(sel + b * 256);
    unsigned int m = 0u;
    for (int k = 0; k < SEL_PARTS; ++k) m |= parts[k * 8 + c];
    pres[c] = m;
  }
  __syncthreads();
  auto present = [&](int k) { return k < C && ((pres[k >> 5] >> (k & 31)) & 1u) != 0u; };
  int n = 0, rank = 0;
  const unsigned int kc = skey[c];
  for (int k = 0; k < 256; ++k) {
    if (!present(k)) continue;
    ++n;
    const unsigned int kk = skey[k];
    rank += (kk < kc || (kk == kc && k < c)) ? 1 : 0;
  }
  sel[b * 256 + c] = (present(c) && rank < (n + 1) / 2) ? 1 : 0;
}

// ESZ = bytes per image element (4 | 2); words are moved as bits
template <int ESZ>
__global__ __launch_bounds__(256) void mix_batch_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ label,
                                                        const int* __restrict__ partner, const unsigned char* __restrict__ sel,
                                                        const int* __restrict__ boxes, unsigned char* __restrict__ image_out,
                                                        long long* __restrict__ target_out, long B, int Ci, int H, int W) {
  __shared__ unsigned char ssel[256];
  const long b = blockIdx.y;
  if (sel) ssel[threadIdx.x] = sel[b * 256 + threadIdx.x];       // 256 threads
  int pb = partner[b];
  pb = pb < 0 ? 0 : (pb > B - 1 ? (int)(B - 1) : pb);
  int y0 = 0, x0 = 0, y1 = 0, x1 = 0;
  if (boxes) {
    auto clampi = [](int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); };
    y0 = clampi(boxes[b * 4 + 0], H); x0 = clampi(boxes[b * 4 + 1], W);
    y1 = clampi(boxes[b * 4 + 2], H); x1 = clampi(boxes[b * 4 + 3], W);
  }
  __syncthreads();
  const long HW = (long)H * W, groups = HW / 8;
  const int wg = W / 8;
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
    const long off = g * 8;
    const uint2 la = *reinterpret_cast<const uint2*>(label + b * HW + off);
    const uint2 lp = *reinterpret_cast<const uint2*>(label + pb * HW + off);
    unsigned int m = 0u;                                         // bit j: pixel j takes sample b
    if (sel) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        m |= ssel[(la.x >> (8 * j)) & 0xffu] ? (1u << j) : 0u;
        m |= ssel[(la.y >> (8 * j)) & 0xffu] ? (1u << (4 + j)) : 0u;
      }
    } else {
      const int y = (int)(g / wg), x = (int)(g - (long)y * wg) * 8;
      if (y >= y0 && y < y1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) m |= (x + j >= x0 && x + j < x1) ? (1u << j) : 0u;
      }
    }
    long long t[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      t[j] = (long long)((((m >> j) & 1u) ? la.x : lp.x) >> (8 * j) & 0xffu);
      t[4 + j] = (long long)((((m >> (4 + j)) & 1u) ? la.y : lp.y) >> (8 * j) & 0xffu);
    }
#pragma unroll
    for (int j = 0; j < 8; j += 2) *reinterpret_cast<longlong2*>(target_out + b * HW + off + j) = make_longlong2(t[j], t[j + 1]);
    constexpr int NV = ESZ / 2;                                  // 16-byte vectors per 8 pixels
    for (int c = 0; c < Ci; ++c) {
      const unsigned char* const pa = image + ((b * Ci + c) * HW + off) * ESZ;
      const unsigned char* const pp = image + (((long)pb * Ci + c) * HW + off) * ESZ;
      unsigned char* const po = image_out + ((b * Ci + c) * HW + off) * ESZ;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        uint4 o;
        if (m == 0xffu) o = *reinterpret_cast<const uint4*>(pa + 16 * v);
        else if (m == 0u) o = *reinterpret_cast<const uint4*>(pp + 16 * v);
        else {
          const uint4 a = *reinterpret_cast<const uint4*>(pa + 16 * v);
          const uint4 p = *reinterpret_cast<const uint4*>(pp + 16 * v);
          const unsigned int aw[4] = {a.x, a.y, a.z, a.w}, pw[4] = {p.x, p.y, p.z, p.w};
          unsigned int ow[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            unsigned int wm;                                     // bits of word q that come from sample b
            if (ESZ == 4) wm = ((m >> (4 * v + q)) & 1u) ? 0xffffffffu : 0u;
            else wm = (((m >> (2 * q)) & 1u) ? 0x0000ffffu : 0u) | (((m >> (2 * q + 1)) & 1u) ? 0xffff0000u : 0u);
            ow[q] = (aw[q] & wm) | (pw[q] & ~wm);
          }
          o = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        }
        *reinterpret_cast<uint4*>(po + 16 * v) = o;
      }
    }
  }
}

}  // namespace

extern "C" {

int tss_classmix_select(const unsigned char* label, const unsigned int* keys, unsigned char* sel, long B, long HW, int C, void* stream) {
  TSS_REQUIRE(B >= 0 && B <= 65535 && HW >= 0 && C >= 1 && C <= 256 && label && keys && sel, TSS_ERR_SHAPE);
  TSS_REQUIRE((reinterpret_cast<uintptr_t>(sel) & 3u) == 0 && (reinterpret_cast<uintptr_t>(keys) & 3u) == 0, TSS_ERR_ALIGN);
  if (B == 0) return TSS_OK;
  hipLaunchKernelGGL(classmix_present_kernel, dim3(SEL_PARTS, (int)B), dim3(SEL_NT), 0, (hipStream_t)stream, label, sel, HW);
  hipLaunchKernelGGL(classmix_rank_kernel, dim3((int)B), dim3(256), 0, (hipStream_t)stream, keys, sel, C);
  return tss::check_last("classmix_select");
}

int tss_mix_batch(const void* image, const unsigned char* label, const int* partner, const unsigned char* sel, const int* boxes,
                  void* image_out, long long* target_out, long B, int Ci, int H, int W, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(B >= 0 && B <= 65535 && Ci >= 1 && H >= 1 && W >= 8 && (W % 8) == 0 && image && label && partner && image_out && target_out &&
              ((sel != nullptr) != (boxes != nullptr)), TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(image) && tss::aligned16(image_out) && tss::aligned16(target_out) &&
              (reinterpret_cast<uintptr_t>(label) & 7u) == 0, TSS_ERR_ALIGN);
  if (B == 0) return TSS_OK;
  const long groups = (long)H * W / 8;
  const int gx = tss::grid_for(groups, 256, 1024);
  if (dtype == TSS_BF16)
    hipLaunchKernelGGL(mix_batch_kernel<2>, dim3(gx, (int)B), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)image, label, partner,
                       sel, boxes, (unsigned char*)image_out, target_out, B, Ci, H, W);
  else
    hipLaunchKernelGGL(mix_batch_kernel<4>, dim3(gx, (int)B), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)image, label, partner,
                       sel, boxes, (unsigned char*)image_out, target_out, B, Ci, H, W);
  return tss::check_last("mix_batch");
}

}  // extern "C"
