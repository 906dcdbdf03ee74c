// The class-plane sweep of the losses and metrics on NCHW-planar logits, its building blocks once (loss.hip: ce_fwd, ce_bwd,
// ce_finalize_rows, argmax_confusion; ohem.hip: ohem_pixel, ohem_bwd; softloss.hip: focal, Dice; lovasz.hip: key, bwd).
//   A lane owns a GROUP of 8 consecutive pixels of one image (HW % 8 == 0, so a group never straddles two images); every class
//   plane is read / written as 16-byte vectors; the grid strides over the B * HW / 8 groups (Groups).
//   Labels live in the lane as 8 ints (load_labels): the class of a valid pixel, OUT_OF_RANGE or IGNORED for every other one.
//   A pixel counts iff its label is >= 0, that is iff target != ignore_index (when there is one) and 0 <= target < C: the one
//   validity rule of every loss here and of the fused head.  `label == c` is the one-hot term; it is never true for a pixel
//   that does not count.  (Lovasz-Softmax drops only IGNORED pixels; its out-of-range labels are background.)
//   The gradient sweeps of CE, OHEM and focal load the labels WITHOUT the ignore index and give a pixel that does not count
//   the weight 0 (counts()): an ignored label inside [0, C) keeps its one-hot term, so the zero written at its class plane is
//   (e - 1) * 0 = -0 as the formula has it, not +0.
//   lse8       : online log-sum-exp over the C planes, optionally with the pick of the label's logit -> per-pixel lse in f32
//   grad8      : dlogits[c] = (exp(x_c - lse) - [c == label]) * w for all C planes, softmax recomputed from the saved lse
//   lse8_weighted, grad8_weighted : the same two sweeps for the class-weighted, label-smoothed cross-entropy (loss.hip: ce_fwd_ex, ce_bwd_ex)
//   block_sum2 : two f64 sums over the block (wave_sum, LDS, thread 0)
//   row_sum2   : the two columns of [nrows][2] per-block rows summed by one block in a fixed order (the finalize kernels)
//
// An instance supplies: its kernel (name, parameters, __launch_bounds__), what it does with the lse / the picked logit of a
// group (loss terms, saved arrays), the per-pixel weight w of its gradient, and where its block sums go (ce_fwd: f64 atomics;
// focal: a row of its own).  Its entry point supplies the grid; the loop is the same for any grid, so a capped grid
// (softloss_max_blocks) takes the same trips through it as a large image.
// Sweeps that stay written out, and why: focal_fwd_kernel keeps the label's class OUT of its running sum and ends in log1pf
// (a different formula by design); lovasz.hip's softmax_stats is a two-pass f64 softmax; the Dice sums and the Dice gradient carry
// per-class coefficients through the planes.  They share the loop, the labels and the reductions.
#pragma once
#include "common.h"

namespace lsw {

constexpr int NT = 256;                       // threads per block of every kernel built from these pieces
constexpr int OUT_OF_RANGE = -1, IGNORED = -2;

// the groups of this lane, grid-stride:
//   for (lsw::Groups g(B, HW); g.more(); g.next()) { const long b = g.b(), off = g.off(); ... }     image, first pixel within it
// (a struct and not a function that takes the loop body: with the body as a lambda dice_fwd_kernel needed 40 more VGPRs)
struct Groups {
  long i, per, n;                             // group index, groups per image, groups in all
  __device__ __forceinline__ Groups(long B, long HW) : i((long)blockIdx.x * blockDim.x + threadIdx.x), per(HW / 8), n(B * (HW / 8)) {}
  __device__ __forceinline__ bool more() const { return i < n; }
  __device__ __forceinline__ void next() { i += (long)gridDim.x * blockDim.x; }
  __device__ __forceinline__ long b() const { return i / per; }
  __device__ __forceinline__ long off() const { return (i - b() * per) * 8; }      // the same quotient as b(): one division
};

// the 8 labels of a group (target points at the group's first pixel); has_ignore == 0: no label is IGNORED
__device__ __forceinline__ void load_labels(const long long* target, int C, int ignore_index, int has_ignore, int tv[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const long long t = target[j];
    tv[j] = (has_ignore && t == (long long)ignore_index) ? IGNORED : ((t >= 0 && t < C) ? (int)t : OUT_OF_RANGE);
  }
}
// the validity rule on a label that was loaded without the ignore index (has_ignore == 0)
__device__ __forceinline__ bool counts(int tv, int ignore_index) { return tv >= 0 && tv != ignore_index; }

// l[j] = log sum_c exp(x[c][j]) of the 8 pixels at x (plane stride HW), one pass with a running maximum.
// PICK: xt[j] = the logit of class tv[j] (0 where the pixel does not count); otherwise tv and xt are not touched.
template <bool PICK, typename T>
__device__ __forceinline__ void lse8(const T* x, int C, long HW, const int* tv, float l[8], float* xt) {
  float m[8], s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { m[j] = -INFINITY; s[j] = 0.f; if (PICK) xt[j] = 0.f; }
  for (int c = 0; c < C; ++c) {
    float v[8];
    V8<T>::load(x + (long)c * HW, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float mn = fmaxf(m[j], v[j]);
      s[j] = s[j] * __expf(m[j] - mn) + __expf(v[j] - mn);
      m[j] = mn;
      if (PICK && tv[j] == c) xt[j] = v[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) l[j] = m[j] + __logf(s[j]);
}

// dx[c][j] = (exp(x[c][j] - l[j]) - [c == tv[j]]) * w[j] for all C planes; NEGATED: ([c == tv[j]] - exp(..)) * w[j]
template <bool NEGATED, typename T>
__device__ __forceinline__ void grad8(const T* x, T* dx, int C, long HW, const int tv[8], const float l[8], const float w[8]) {
  for (int c = 0; c < C; ++c) {
    float v[8], d[8];
    V8<T>::load(x + (long)c * HW, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float e = __expf(v[j] - l[j]), h = tv[j] == c ? 1.f : 0.f;
      d[j] = (NEGATED ? h - e : e - h) * w[j];
    }
    V8<T>::store(dx + (long)c * HW, d);
  }
}

// lse8 with the label's logit picked and, SMOOTH only, xw[j] = sum_c cw[c] * x[c][j] (cw == nullptr: all ones): the extra term of
// the class-weighted, label-smoothed cross-entropy.  cw[c] is the same address in every lane.
template <bool SMOOTH, typename T>
__device__ __forceinline__ void lse8_weighted(const T* x, int C, long HW, const float* cw, const int* tv, float l[8], float* xt,
                                              float* xw) {
  float m[8], s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { m[j] = -INFINITY; s[j] = 0.f; xt[j] = 0.f; if (SMOOTH) xw[j] = 0.f; }
  for (int c = 0; c < C; ++c) {
    float v[8];
    V8<T>::load(x + (long)c * HW, v);
    const float wc = (SMOOTH && cw) ? cw[c] : 1.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float mn = fmaxf(m[j], v[j]);
      s[j] = s[j] * __expf(m[j] - mn) + __expf(v[j] - mn);
      m[j] = mn;
      if (tv[j] == c) xt[j] = v[j];
      if (SMOOTH) xw[j] = fmaf(wc, v[j], xw[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) l[j] = m[j] + __logf(s[j]);
}

// dx[c][j] = exp(x[c][j] - l[j]) * s[j] - [c == tv[j]] * a[j] - cw[c] * u[j] for all C planes (cw == nullptr: all ones): the
// gradient of the class-weighted, label-smoothed cross-entropy, s = the pixel's total weight, a = its one-hot part, u = its
// uniform part per unit class weight; all three are 0 for a pixel that does not count.  SMOOTH == false: u is not read.
template <bool SMOOTH, typename T>
__device__ __forceinline__ void grad8_weighted(const T* x, T* dx, int C, long HW, const float* cw, const int tv[8], const float l[8],
                                               const float s[8], const float a[8], const float u[8]) {
  for (int c = 0; c < C; ++c) {
    float v[8], d[8];
    V8<T>::load(x + (long)c * HW, v);
    const float wc = (SMOOTH && cw) ? cw[c] : 1.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      d[j] = __expf(v[j] - l[j]) * s[j] - (tv[j] == c ? a[j] : 0.f);
      if (SMOOTH) d[j] -= wc * u[j];
    }
    V8<T>::store(dx + (long)c * HW, d);
  }
}

// a, b summed over the block; true in thread 0, which alone holds the sums.  One call per kernel: the LDS buffer is the
// function's own, and a second call would reuse it with no barrier in between.
__device__ __forceinline__ bool block_sum2(double& a, double& b) {
  __shared__ double red[2][NT / 64];
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x != 0) return false;
  a = 0.0; b = 0.0;
  for (int w = 0; w < NT / 64; ++w) { a += red[0][w]; b += red[1][w]; }
  return true;
}

// a = sum(rows[.][0]), b = sum(rows[.][1]) by one block of NT threads in a fixed order (thread t takes rows t, t + NT, ...,
// then a tree); true in thread 0, the one that finalizes.  One call per kernel, as for block_sum2.
__device__ __forceinline__ bool row_sum2(const double* rows, int nrows, double& a, double& b) {
  __shared__ double red[2][NT];
  a = 0.0; b = 0.0;
  for (int i = threadIdx.x; i < nrows; i += NT) { a += rows[2 * (long)i]; b += rows[2 * (long)i + 1]; }
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = b;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { red[0][threadIdx.x] += red[0][threadIdx.x + s]; red[1][threadIdx.x] += red[1][threadIdx.x + s]; }
    __syncthreads();
  }
  a = red[0][0]; b = red[1][0];
  return threadIdx.x == 0;
}

}  // namespace lsw
