// Logit distillation on the low-resolution NHWC logits (rows of pitch ld >= C, ld % 8 == 0): temperature-softened KL divergence
// between a teacher's and a student's softmax, with the softmax over the classes of a pixel (pixel kind, Hinton et al.) or over the
// positions of a (sample, class) plane (channel kind, Shu et al., ICCV 2021).  x_S = s / tau, x_T = t / tau; a UNIT is a pixel
// (N = C terms) or a plane (N = h w terms); p = softmax(x_T), q = softmax(x_S) over the unit:
//   KL(unit) = sum p (log p - log q),   loss = tau^2 / #units * sum KL,   dloss/ds = tau / #units * (q - p) * grad_out.
// Every pixel counts (no target, no ignore mask).  The teacher is a constant.
//
// Two sweeps per unit.  The first takes the exact maxima m_S, m_T of the unit (of the raw logits; m = max * (1 / tau) is only a
// shift, whatever its rounding).  The second takes, with e = exp(fma(x, 1 / tau, -m)),
//   Z_S = sum e_S,  Z_T = sum e_T,  A = sum e_T (t - s) / tau,   KL = A / Z_T + (m_S - m_T) + log(Z_S / Z_T).
// f32 roundings from the inputs to a unit's KL, k = 16: 1 / tau (1); per softmax the fma, the exp and the sum (2 x 3); A: t - s,
// times 1 / tau, the fma sum, the division (4); m_S - m_T, Z_S / Z_T, the log and the two additions (5).  A sum counts once: its
// lane, block and finalize levels are plain additions of non-negative terms (of any sign for A) in a fixed order.
// One online sweep (running maximum, sums rescaled along) was the alternative: every level of the channel kind's reduction would
// add a subtraction and an exp of its own to each of the three sums, which puts the count past 16; and an empty partial needs
// care there that it does not need here (maximum -inf and sums 0 ARE the identities of max and +, nothing is ever subtracted
// from -inf).  Equal student and teacher bits run the same operations: KL is exactly 0 and so is every gradient element.
//
// What the backward reads is saved as FOUR floats per unit, (m_S, log Z_S, m_T, log Z_T), not as two log-sum-exps: q =
// exp(fma(s, 1 / tau, -m_S) - log Z_S) keeps the probabilities of saturated logits (|x| of a few hundred) to an ulp of the
// small difference, where m + log Z would round at the size of m.
//
// pixel kind:   a lane owns a pixel and walks its ceil(C / 8) 16-byte vectors twice (the second walk hits the cache); the grid
//               strides over the pixels; per-block f64 partial sums go to a row of the workspace, a one-block finalize adds them.
// channel kind: a column reduction.  A lane owns one 16-byte vector (8 channels) of a strip of positions, NT / ceil(C / 8)
//               positions per block and trip, consecutive lanes on consecutive vectors of a row.  An image's h w positions are
//               cut into S segments (as many as the block cap allows: the B C planes alone are far fewer than the CUs), an ITEM
//               is (image, segment); the blocks stride over the items and every item leaves one partial row per sweep (maxima;
//               the three sums).  The second sweep and the finalize reduce the S partial maxima of a plane themselves (exact, so all
//               agree).  The finalize adds the S partial sums of a plane in segment order.
// No atomics, nothing zero-filled, no host read-back: every workspace element that is read was written by the launch before.
// Pad channels c in [C, ld) of the inputs may hold anything (NaN): they are masked where a result could see them (pixel
// kind, backward) or end in partial-row columns nobody reads (channel kind).  The gradient's pad channels are written as zeros.
#include "losssweep.h"

namespace {

constexpr int NT = lsw::NT;
constexpr int MAX_C = 256;
constexpr int PIXEL_BLOCKS = 4096;       // default block caps
constexpr int CHANNEL_BLOCKS = 512;

// ------------------------------------------------------------------------------------------------------------ pixel kind
template <typename T>
__global__ __launch_bounds__(NT) void distill_pixel_fwd_kernel(const T* s, long lds, const T* t, long ldt, float4* stats,
                                                               double* rows /*[gridDim.x][2]: sum of KL, unused*/, long P, int C,
                                                               float inv_tau) {
  const int nch = (C + 7) >> 3;
  double lsum = 0.0, none = 0.0;
  for (long p = (long)blockIdx.x * NT + threadIdx.x; p < P; p += (long)gridDim.x * NT) {
    const T* sp = s + p * lds;
    const T* tp = t + p * ldt;
    float ms = -INFINITY, mt = -INFINITY;
    for (int j = 0; j < nch; ++j) {
      float vs[8], vt[8];
      V8<T>::load(sp + 8 * j, vs);
      V8<T>::load(tp + 8 * j, vt);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bool ok = 8 * j + k < C;
        ms = fmaxf(ms, ok ? vs[k] : -INFINITY);
        mt = fmaxf(mt, ok ? vt[k] : -INFINITY);
      }
    }
    ms *= inv_tau;
    mt *= inv_tau;
    float zs = 0.f, zt = 0.f, a = 0.f;
    for (int j = 0; j < nch; ++j) {
      float vs[8], vt[8];
      V8<T>::load(sp + 8 * j, vs);
      V8<T>::load(tp + 8 * j, vt);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bool ok = 8 * j + k < C;
        const float es = ok ? __expf(fmaf(vs[k], inv_tau, -ms)) : 0.f;
        const float et = ok ? __expf(fmaf(vt[k], inv_tau, -mt)) : 0.f;
        const float d = ok ? (vt[k] - vs[k]) * inv_tau : 0.f;
        zs += es;
        zt += et;
        a = fmaf(et, d, a);
      }
    }
    lsum += (double)(a / zt + (ms - mt) + logf(zs / zt));
    stats[p] = make_float4(ms, logf(zs), mt, logf(zt));
  }
  if (lsw::block_sum2(lsum, none)) {
    rows[2 * (long)blockIdx.x] = lsum;
    rows[2 * (long)blockIdx.x + 1] = 0.0;
  }
}

// loss = norm * sum(rows[.][0]), norm = tau^2 / #pixels.  One block, fixed tree.
__global__ __launch_bounds__(NT) void distill_pixel_finalize_kernel(const double* rows, int nrows, double norm, float* loss) {
  double sum, none;
  if (lsw::row_sum2(rows, nrows, sum, none)) *loss = (float)(norm * sum);
}

// ------------------------------------------------------------------------------------------------------------ channel kind
// The items (image, segment) of the channel kind and what a thread is within its block.
struct Strip {
  int nch, ppb, slot, j;                      // vectors per row, positions per block and trip, this thread's position slot and vector
  long len;                                   // positions per segment
  __device__ __forceinline__ Strip(int C, long HW, int S) {
    nch = (C + 7) >> 3;
    ppb = NT / nch;
    slot = (int)threadIdx.x / nch;
    j = (int)threadIdx.x - slot * nch;
    len = (HW + S - 1) / S;
  }
  __device__ __forceinline__ bool active() const { return slot < ppb; }
};

// red[v][thread], v < NV: combined over the position slots of a block in a fixed tree; the result is in the threads of slot 0.
// MAX: fmaxf, otherwise +.  Ends with the values of slot 0 in registers; a barrier protects the buffer for the next call.
template <int NV, bool MAX>
__device__ __forceinline__ void slot_reduce(float (*red)[NT], const Strip& g, float v[NV]) {
#pragma unroll
  for (int i = 0; i < NV; ++i) red[i][threadIdx.x] = v[i];
  int half = 1;
  while (half < g.ppb) half <<= 1;
  for (half >>= 1; half > 0; half >>= 1) {
    __syncthreads();
    if (g.slot < half && g.slot + half < g.ppb) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const float o = red[i][threadIdx.x + half * g.nch];
        red[i][threadIdx.x] = MAX ? fmaxf(red[i][threadIdx.x], o) : red[i][threadIdx.x] + o;
      }
    }
  }
  if (g.slot == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = red[i][threadIdx.x];
  }
  __syncthreads();
}

// pmax[item][2][CP]: the maxima of the raw student / teacher logits over the item's positions (-inf for an item with none)
template <typename T>
__global__ __launch_bounds__(NT) void distill_channel_max_kernel(const T* s, long lds, const T* t, long ldt, float* pmax, long B, int C,
                                                                 long HW, int S) {
  __shared__ float red[16][NT];
  const Strip g(C, HW, S);
  const int CP = 8 * g.nch;
  for (long item = blockIdx.x; item < B * S; item += gridDim.x) {
    const long b = item / S, seg = item - b * S;
    const long i0 = seg * g.len, i1 = (i0 + g.len < HW) ? i0 + g.len : HW;
    float m[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = -INFINITY;
    if (g.active()) {
      for (long i = i0 + g.slot; i < i1; i += g.ppb) {
        float vs[8], vt[8];
        V8<T>::load(s + (b * HW + i) * lds + 8 * g.j, vs);
        V8<T>::load(t + (b * HW + i) * ldt + 8 * g.j, vt);
#pragma unroll
        for (int k = 0; k < 8; ++k) { m[k] = fmaxf(m[k], vs[k]); m[8 + k] = fmaxf(m[8 + k], vt[k]); }
      }
    }
    slot_reduce<16, true>(red, g, m);
    if (g.slot == 0) {
      V8<float>::store(pmax + (item * 2) * CP + 8 * g.j, m);
      V8<float>::store(pmax + (item * 2 + 1) * CP + 8 * g.j, m + 8);
    }
  }
}

// the maximum of plane (b, c) times 1 / tau: the S partial maxima in segment order (which = 0: student, 1: teacher)
__device__ __forceinline__ float plane_max(const float* pmax, long b, int S, int CP, int which, int c, float inv_tau) {
  float m = -INFINITY;
  for (int q = 0; q < S; ++q) m = fmaxf(m, pmax[((b * S + q) * 2 + which) * CP + c]);
  return m * inv_tau;
}

// psum[item][3][CP]: Z_S, Z_T and A of the item's positions against the plane maxima (0 for an item with none)
template <typename T>
__global__ __launch_bounds__(NT) void distill_channel_sum_kernel(const T* s, long lds, const T* t, long ldt, const float* pmax,
                                                                 float* psum, long B, int C, long HW, int S, float inv_tau) {
  __shared__ float red[24][NT];
  __shared__ float pm[2][MAX_C];
  const Strip g(C, HW, S);
  const int CP = 8 * g.nch;
  long cur = -1;                               // the image whose plane maxima are in pm
  for (long item = blockIdx.x; item < B * S; item += gridDim.x) {
    const long b = item / S, seg = item - b * S;
    const long i0 = seg * g.len, i1 = (i0 + g.len < HW) ? i0 + g.len : HW;
    if (b != cur) {                            // uniform
      __syncthreads();
      for (int idx = threadIdx.x; idx < 2 * CP; idx += NT) {
        const int which = idx / CP, c = idx - which * CP;
        pm[which][c] = plane_max(pmax, b, S, CP, which, c, inv_tau);
      }
      __syncthreads();
      cur = b;
    }
    float acc[24];                             // Z_S, Z_T, A of this lane's 8 channels
#pragma unroll
    for (int k = 0; k < 24; ++k) acc[k] = 0.f;
    if (g.active()) {
      float ms[8], mt[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) { ms[k] = pm[0][8 * g.j + k]; mt[k] = pm[1][8 * g.j + k]; }
      for (long i = i0 + g.slot; i < i1; i += g.ppb) {
        float vs[8], vt[8];
        V8<T>::load(s + (b * HW + i) * lds + 8 * g.j, vs);
        V8<T>::load(t + (b * HW + i) * ldt + 8 * g.j, vt);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float et = __expf(fmaf(vt[k], inv_tau, -mt[k]));
          acc[k] += __expf(fmaf(vs[k], inv_tau, -ms[k]));
          acc[8 + k] += et;
          acc[16 + k] = fmaf(et, (vt[k] - vs[k]) * inv_tau, acc[16 + k]);
        }
      }
    }
    slot_reduce<24, false>(red, g, acc);
    if (g.slot == 0) {
      V8<float>::store(psum + (item * 3) * CP + 8 * g.j, acc);
      V8<float>::store(psum + (item * 3 + 1) * CP + 8 * g.j, acc + 8);
      V8<float>::store(psum + (item * 3 + 2) * CP + 8 * g.j, acc + 16);
    }
  }
}

// One block: thread -> plane (b, c), c < C only; the S partial sums in segment order; stats[plane] and loss = norm * sum of KL
__global__ __launch_bounds__(NT) void distill_channel_finalize_kernel(const float* pmax, const float* psum, float4* stats, float* loss,
                                                                      long B, int C, int S, float inv_tau, double norm) {
  const int CP = 8 * ((C + 7) >> 3);
  double lsum = 0.0, none = 0.0;
  for (long plane = threadIdx.x; plane < B * C; plane += NT) {
    const long b = plane / C;
    const int c = (int)(plane - b * C);
    const float ms = plane_max(pmax, b, S, CP, 0, c, inv_tau), mt = plane_max(pmax, b, S, CP, 1, c, inv_tau);
    float zs = 0.f, zt = 0.f, a = 0.f;
    for (int q = 0; q < S; ++q) {
      const float* row = psum + ((b * S + q) * 3) * CP + c;
      zs += row[0];
      zt += row[CP];
      a += row[2 * CP];
    }
    lsum += (double)(a / zt + (ms - mt) + logf(zs / zt));
    stats[plane] = make_float4(ms, logf(zs), mt, logf(zt));
  }
  if (lsw::block_sum2(lsum, none)) *loss = (float)(norm * lsum);
}

// ------------------------------------------------------------------------------------------------------------ backward
// One elementwise sweep for either kind: a lane takes one 16-byte vector of the gradient, pad vectors included (zeros).
// d = grad_out * (norm * (q - p)), norm = tau / #units.
template <typename T, bool CHANNEL>
__global__ __launch_bounds__(NT) void distill_bwd_kernel(const T* s, long lds, const T* t, long ldt, const float4* stats,
                                                         const float* grad_out, T* ds, long ldd, long P, int C, long HW,
                                                         float inv_tau, float norm) {
  const float go = grad_out ? *grad_out : 1.f;
  const int nv = (int)(ldd >> 3);
  for (long idx = (long)blockIdx.x * NT + threadIdx.x; idx < P * nv; idx += (long)gridDim.x * NT) {
    const long p = idx / nv;
    const int j = (int)(idx - p * nv);
    float d[8];
    if (8 * j >= C) {
#pragma unroll
      for (int k = 0; k < 8; ++k) d[k] = 0.f;
    } else {
      float vs[8], vt[8];
      V8<T>::load(s + p * lds + 8 * j, vs);
      V8<T>::load(t + p * ldt + 8 * j, vt);
      const long b = p / HW;
      float4 st = CHANNEL ? make_float4(0.f, 0.f, 0.f, 0.f) : stats[p];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bool ok = 8 * j + k < C;
        if (CHANNEL && ok) st = stats[b * C + 8 * j + k];
        const float q = __expf(fmaf(vs[k], inv_tau, -st.x) - st.y);
        const float pt = __expf(fmaf(vt[k], inv_tau, -st.z) - st.w);
        d[k] = ok ? go * (norm * (q - pt)) : 0.f;
      }
    }
    V8<T>::store(ds + p * ldd + 8 * j, d);
  }
}

// ------------------------------------------------------------------------------------------------------------ host side
inline bool shape_ok(long B, int C, long HW, long lds, long ldt, float tau, int max_blocks) {
  return B > 0 && HW > 0 && C >= 1 && C <= MAX_C && lds >= C && ldt >= C && (lds % 8) == 0 && (ldt % 8) == 0 && tau > 0.f &&
         max_blocks >= 0 && B <= (1L << 40) / HW;
}

struct Split { int S, grid; long items; };
// the segments per image and the grid of the channel kind: at most `cap` items while the cap allows one item per image
inline Split channel_split(long B, int C, long HW, int max_blocks) {
  const long cap = max_blocks > 0 ? max_blocks : CHANNEL_BLOCKS;
  const int ppb = NT / ((C + 7) / 8);
  long S = (HW + ppb - 1) / ppb;
  const long per = cap / B > 1 ? cap / B : 1;
  if (S > per) S = per;
  Split r;
  r.S = (int)S;
  r.items = B * S;
  r.grid = (int)(r.items < cap ? r.items : cap);
  return r;
}
inline size_t channel_row_floats(int C) { return 8 * (size_t)((C + 7) / 8); }

inline int pixel_grid(long P, int max_blocks) { return tss::grid_for(P, NT, max_blocks > 0 ? (long)max_blocks : PIXEL_BLOCKS); }

template <bool CHANNEL>
int distill_bwd(const void* s, long lds, const void* t, long ldt, const float* stats, const float* grad_out, void* ds, long ldd, long B,
                int C, long HW, float tau, int max_blocks, int dtype, void* stream, const char* what) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(shape_ok(B, C, HW, lds, ldt, tau, max_blocks) && ldd >= C && (ldd % 8) == 0 && stats, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(s) && tss::aligned16(t) && tss::aligned16(ds) && tss::aligned16(stats), TSS_ERR_ALIGN);
  const long P = B * HW;
  const float norm = (float)((double)tau / (CHANNEL ? (double)B * C : (double)P));
  const int grid = tss::grid_for(P * (ldd / 8), NT, max_blocks > 0 ? (long)max_blocks : PIXEL_BLOCKS);
  TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL(HIP_KERNEL_NAME(distill_bwd_kernel<TT, CHANNEL>), dim3(grid), dim3(NT), 0, (hipStream_t)stream, (const TT*)s, lds,
                                           (const TT*)t, ldt, (const float4*)stats, grad_out, (TT*)ds, ldd, P, C, HW, 1.f / tau, norm));
  return tss::check_last(what);
}

}  // namespace

extern "C" {

long tss_distill_workspace_bytes(int kind, long B, int C, long HW, int max_blocks) {
  if ((kind != 0 && kind != 1) || !shape_ok(B, C, HW, MAX_C, MAX_C, 1.f, max_blocks)) return 0;
  if (kind == 0) return (long)(sizeof(double) * 2 * (size_t)pixel_grid(B * HW, max_blocks));
  return (long)(sizeof(float) * 5 * channel_row_floats(C) * (size_t)channel_split(B, C, HW, max_blocks).items);
}

int tss_distill_pixel_fwd(const void* student, long lds, const void* teacher, long ldt, float* stats, void* workspace, float* loss,
                          long B, int C, long HW, float tau, int max_blocks, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(shape_ok(B, C, HW, lds, ldt, tau, max_blocks) && stats && workspace && loss, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(student) && tss::aligned16(teacher) && tss::aligned16(stats) && tss::aligned16(workspace), TSS_ERR_ALIGN);
  hipStream_t st = (hipStream_t)stream;
  const long P = B * HW;
  const int grid = pixel_grid(P, max_blocks);
  double* rows = static_cast<double*>(workspace);
  TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL(distill_pixel_fwd_kernel<TT>, dim3(grid), dim3(NT), 0, st, (const TT*)student, lds,
                                           (const TT*)teacher, ldt, (float4*)stats, rows, P, C, 1.f / tau));
  hipLaunchKernelGGL(distill_pixel_finalize_kernel, dim3(1), dim3(NT), 0, st, rows, grid, (double)tau * (double)tau / (double)P, loss);
  return tss::check_last("distill_pixel_fwd");
}

int tss_distill_pixel_bwd(const void* student, long lds, const void* teacher, long ldt, const float* stats, const float* grad_out,
                          void* dstudent, long ldd, long B, int C, long HW, float tau, int max_blocks, int dtype, void* stream) {
  return distill_bwd<false>(student, lds, teacher, ldt, stats, grad_out, dstudent, ldd, B, C, HW, tau, max_blocks, dtype, stream,
                            "distill_pixel_bwd");
}

int tss_distill_channel_fwd(const void* student, long lds, const void* teacher, long ldt, float* stats, void* workspace, float* loss,
                            long B, int C, long HW, float tau, int max_blocks, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(shape_ok(B, C, HW, lds, ldt, tau, max_blocks) && stats && workspace && loss, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(student) && tss::aligned16(teacher) && tss::aligned16(stats) && tss::aligned16(workspace), TSS_ERR_ALIGN);
  hipStream_t st = (hipStream_t)stream;
  const Split sp = channel_split(B, C, HW, max_blocks);
  float* pmax = static_cast<float*>(workspace);
  float* psum = pmax + 2 * channel_row_floats(C) * (size_t)sp.items;
  const float inv_tau = 1.f / tau;
  TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL(distill_channel_max_kernel<TT>, dim3(sp.grid), dim3(NT), 0, st, (const TT*)student, lds,
                                           (const TT*)teacher, ldt, pmax, B, C, HW, sp.S));
  TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL(distill_channel_sum_kernel<TT>, dim3(sp.grid), dim3(NT), 0, st, (const TT*)student, lds,
                                           (const TT*)teacher, ldt, pmax, psum, B, C, HW, sp.S, inv_tau));
  hipLaunchKernelGGL(distill_channel_finalize_kernel, dim3(1), dim3(NT), 0, st, pmax, psum, (float4*)stats, loss, B, C, sp.S, inv_tau,
                     (double)tau * (double)tau / ((double)B * (double)C));
  return tss::check_last("distill_channel_fwd");
}

int tss_distill_channel_bwd(const void* student, long lds, const void* teacher, long ldt, const float* stats, const float* grad_out,
                            void* dstudent, long ldd, long B, int C, long HW, float tau, int max_blocks, int dtype, void* stream) {
  return distill_bwd<true>(student, lds, teacher, ldt, stats, grad_out, dstudent, ldd, B, C, HW, tau, max_blocks, dtype, stream,
                           "distill_channel_bwd");
}

}  // extern "C"
