// The one-sweep weight gradient of the tap layers, its building blocks once (fc1d.hip, fcg.hip; operands, checks and launch also sconv.hip):
//   dW[n][c][tap] = sum_p g[p][n] * a[src(p, tap)][c],   g = ca*e + cb*y + cc (BatchNorm backward folded),   a = relu?(x*as + ab).
// The contraction runs over PIXELS, so both MFMA operands are needed pixel-major.  Per stage of PT pixels a thread loads 16-byte rows of
// e, (y,) and of the shifted copies of x, converts them in registers (g_row / a_row), writes them once into the dual-use XOR image of
// common.h -- column chunk cv of g at chunk cv, tap t of a at chunk (1 + t) * NV + cv, planes of 16 chunks (st_off) -- and the waves read
// them back transposed as k-major fragments (tr_off) for the k-step x tap x fragment MFMA loop.  Two stage buffers, one barrier per
// stage: the next stage's loads are issued when the current stage's registers are free and land under its MFMAs.  A block owns a
// contiguous range of stages (stage_range) and leaves one row of partial sums in the workspace, torch's [N][C][taps] order
// (store_rows); tss_dw_reduce_many adds the rows.
//
// An instance supplies: its tiling constants, the address generation of a (pixel, tap), the wave -> fragment assignment, its kernel
// (own template parameters and __launch_bounds__: the register budget is per instance) and its row-count policy.  The MFMA loop is
// written out in each kernel, where the compiler schedules the transposed reads of an instance against that instance's own budget.
// The stride-2 kernels of sconv.hip keep their own written-out device body: built from these pieces the compiler gave them a different
// wait schedule (and sc2_wgrad_kernel<64, *> some 50 more registers); they share the operand struct, the checks and the launch helper.
#pragma once
#include "common.h"

namespace wgs {

struct Operands {
  const bf16_t* e; long lde; const bf16_t* y; long ldyr; const float* ga; const float* gb; const float* gce; const float* gmu;
  const bf16_t* x; long ldx; const float* xm; const float* xs; const float* xb; int x_relu;
  float* ws;                                           // [gridDim.x][N * C * taps]
};

// folded constants of a thread's channel vectors: 8 channels of g starting at gch, 8 channels of a starting at xch
template <bool HASY>
struct Fold {
  float ca[8], cb[HASY ? 8 : 1], cc[HASY ? 8 : 1], as[8], ab[8], relu_lo;
  bool gplain, aplain;                                 // the operand goes to LDS as it arrived

  __device__ __forceinline__ void load(const Operands& g, int gch, int xch) {
    gplain = !HASY && !g.ga; aplain = !g.xs && !g.xm && !g.xb && !g.x_relu;
    const float* safe = reinterpret_cast<const float*>(g.e);
    float v0[8], v1[8], v2[8], v3[8], w0[8], w1[8], w2[8];
    const float* p0 = g.ga ? g.ga + gch : safe; const float* p1 = (HASY && g.gb) ? g.gb + gch : safe;
    const float* p2 = (HASY && g.gce) ? g.gce + gch : safe; const float* p3 = (HASY && g.gmu) ? g.gmu + gch : safe;
    const float* q0 = g.xs ? g.xs + xch : safe; const float* q1 = g.xm ? g.xm + xch : safe; const float* q2 = g.xb ? g.xb + xch : safe;
#pragma unroll
    for (int h = 0; h < 8; h += 4) {
      V4<float>::load(p0 + h, v0 + h); V4<float>::load(p1 + h, v1 + h); V4<float>::load(p2 + h, v2 + h); V4<float>::load(p3 + h, v3 + h);
      V4<float>::load(q0 + h, w0 + h); V4<float>::load(q1 + h, w1 + h); V4<float>::load(q2 + h, w2 + h);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float gav = g.ga ? v0[j] : 1.f;
      ca[j] = gav;
      if (HASY) { cb[j] = v1[j]; cc[j] = -(gav * v2[j]) - v1[j] * v3[j]; }      // g = ga*e + gb*y + cc
      const float sc = g.xs ? w0[j] : 1.f;
      as[j] = sc; ab[j] = (g.xb ? w2[j] : 0.f) - (g.xm ? w1[j] : 0.f) * sc;      // a = relu?(x*as + ab)
    }
    relu_lo = g.x_relu ? 0.f : -TSS_INF;
  }
};

// registers -> one normalised bf16 row of the image; a pixel that does not exist / a tap outside the image contributes zeros
template <bool HASY>
__device__ __forceinline__ uint4 g_row(const uint4& re, const uint4& ry, const Fold<HASY>& f, bool exists) {
  uint4 og = re;
  if (!f.gplain) {
    const uint32_t* ue = reinterpret_cast<const uint32_t*>(&re);
    const uint32_t* uy = reinterpret_cast<const uint32_t*>(&ry);
    bf16x8 o;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      float lo = f.ca[2 * h] * blo(ue[h]), hi = f.ca[2 * h + 1] * bhi(ue[h]);
      if (HASY) { lo += f.cb[2 * h] * blo(uy[h]) + f.cc[2 * h]; hi += f.cb[2 * h + 1] * bhi(uy[h]) + f.cc[2 * h + 1]; }
      o[2 * h] = (bf16_t)lo; o[2 * h + 1] = (bf16_t)hi;
    }
    og = *reinterpret_cast<const uint4*>(&o);
  }
  if (!exists) og = make_uint4(0u, 0u, 0u, 0u);
  return og;
}
template <bool HASY>
__device__ __forceinline__ uint4 a_row(const uint4& rx, const Fold<HASY>& f, bool ok) {
  uint4 oa = rx;
  if (!f.aplain) {
    const uint32_t* ux = reinterpret_cast<const uint32_t*>(&rx);
    bf16x8 o;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      o[2 * h] = (bf16_t)fmaxf(blo(ux[h]) * f.as[2 * h] + f.ab[2 * h], f.relu_lo);
      o[2 * h + 1] = (bf16_t)fmaxf(bhi(ux[h]) * f.as[2 * h + 1] + f.ab[2 * h + 1], f.relu_lo);
    }
    oa = *reinterpret_cast<const uint4*>(&o);
  }
  if (!ok) oa = make_uint4(0u, 0u, 0u, 0u);
  return oa;
}

// the contiguous range of PT-pixel stages of this block
__device__ __forceinline__ void stage_range(long P, int PT, long* begin, long* end) {
  const long nstage = (P + PT - 1) / PT;
  const long per = (nstage + gridDim.x - 1) / gridDim.x;
  *begin = (long)blockIdx.x * per;
  *end = *begin + per;
  if (*end > nstage) *end = nstage;
}

// staging: byte offset of 16-byte column chunk gc of pixel row `row` (planes of 16 chunks, PT rows each)
__device__ __forceinline__ int st_off(int PT, int row, int gc) { return (gc >> 4) * PT * 256 + img_off(row, gc & 15); }
// transposed read h (0, 1) of 16-channel fragment F in a 32-pixel k-step: the block of pixels fq * 8 + 4 h .. + 3; this lane supplies the
// address of pixel fr >> 2, channels 4 (fr & 3) .. + 3
__device__ __forceinline__ int tr_off(int PT, int fr, int fq, int h, int F) {
  return (F >> 3) * PT * 256 + img_off(fq * 8 + 4 * h + (fr >> 2), (F & 7) * 2 + ((fr & 3) >> 1)) + 8 * (fr & 1);
}

// accumulators -> the block's row, [N][C][TAPS] order: this lane holds n = 16 fi + 4 fq + q, c = 16 (fj0 + j) + fr
template <int TAPS, int NJ>
__device__ __forceinline__ void store_rows(float* row, const f32x4 (&acc)[TAPS][NJ], int fi, int fj0, int fq, int fr, int C) {
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) row[((long)(16 * fi + 4 * fq + q) * C + 16 * (fj0 + j) + fr) * TAPS + t] = acc[t][j][q];
}

// ---- host side
inline Operands operands(const void* e, long lde, const void* yraw, long ldyr, const float* ga, const float* gb, const float* gce,
                         const float* gmu, const void* xraw, long ldx, const float* in_mean, const float* in_scale, const float* in_bias,
                         int in_relu, float* ws) {
  return {(const bf16_t*)e, lde, (const bf16_t*)yraw, ldyr, ga, gb, gce, gmu, (const bf16_t*)xraw, ldx, in_mean, in_scale, in_bias, in_relu, ws};
}

// the operand checks of the *_bwd_weight_sweep entry points; `covered`: the instance's own shape conditions
inline int check_operands(int dtype, bool covered, const Operands& o, int Cin, int N) {
  TSS_REQUIRE(dtype == TSS_BF16, TSS_ERR_DTYPE);
  TSS_REQUIRE(covered && (o.lde % 8) == 0 && o.lde >= N && (o.ldx % 8) == 0 && o.ldx >= Cin && o.e && o.x && o.ws, TSS_ERR_SHAPE);
  TSS_REQUIRE(!o.y || ((o.ldyr % 8) == 0 && o.ldyr >= N && o.ga && o.gb && o.gce && o.gmu), TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(o.e) && tss::aligned16(o.x) && (!o.y || tss::aligned16(o.y)), TSS_ERR_ALIGN);
  return TSS_OK;
}

// launch with more dynamic LDS than the default limit: the attribute is raised once per kernel and device
template <auto Kernel, class Args>
void launch_with_smem(int grid, int threads, int smem, hipStream_t stream, const Args& args) {
  static tss::DevOnce attr;
  if (attr.first()) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(threads), smem, stream, args);
}

}  // namespace wgs
