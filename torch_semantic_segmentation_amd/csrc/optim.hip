// The end of the train step on the flat f32 buffers (engine.py: FlatAdamW, FlatSGD), all HBM-bound:
//   * adamw_kernel / sgd_kernel: torch.optim.AdamW / SGD per element, hyper-parameters per parameter GROUP (up to
//     TSS_OPT_MAX_GROUPS consecutive ranges of the buffer, the table travels in the kernel arguments)
//   * grad_sqnorm_kernel + grad_sqnorm_final_kernel: the global gradient norm and the clip factor of
//     torch.nn.utils.clip_grad_norm_, f64 partial rows added in a fixed order (no atomics: two runs give the same bits);
//     the step kernels read the factor from the device, the gradient buffer is never rewritten
//   * the <true> instances of the step kernels also keep an exponential moving average of the parameters in a third flat buffer
//     (engine.ModelEMA): the new p[i] is in a register, the average is one more read-modify-write of the same element
//   * ema_rows_kernel: the same average (or a plain copy) over a device table of rows, for what the step does not hold
#include <cmath>
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int MAXG = TSS_OPT_MAX_GROUPS;

// A group as the kernels take it: the caller's row plus the bias corrections of a host-side step counter.
struct OptRow { long end; float lr, weight_decay, beta1, beta2, eps, bc1, bc2s; int flags; };
struct OptArgs { OptRow g[MAXG]; };      // by value, in the kernel argument segment (no device memory, no copy to wait for)

// The factor of update number k (0-based) of the moving average: 1 - d_k, d_k = decay or, warming up, min(decay, (1 + k) / (10 + k)).
// Every operation is an IEEE f32 one (the division is correctly rounded here too), so a host that computes it in f32 gets the same
// bits.
__device__ __forceinline__ float ema_omd(float k, float decay, int warmup) {
  const float d = warmup ? fminf(decay, (1.f + k) / (10.f + k)) : decay;
  return 1.f - d;
}

// state = [ngroups][3] {step, bias_correction1, bias_correction2_sqrt}: one row per group (the betas differ per group)
// ema_state (optional) = {k, omd}: the updates done before the step that follows become k + 1, omd is that step's factor
__global__ void optim_tick_kernel(float* state, const OptArgs a, int ng, int adam, float* ema_state, float decay, int warmup) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (ema_state) {
      const float k = ema_state[0];
      ema_state[1] = ema_omd(k, decay, warmup);
      ema_state[0] = k + 1.f;
    }
#pragma unroll
    for (int k = 0; k < MAXG; ++k) {
      if (k < ng) {
        const float beta1 = a.g[k].beta1, beta2 = a.g[k].beta2;
        const float step = state[3 * k] + 1.f;
        state[3 * k] = step;
        if (adam) {
          state[3 * k + 1] = 1.f - powf(beta1, step);
          state[3 * k + 2] = sqrtf(1.f - powf(beta2, step));
        }
      }
    }
  }
}

// the group of element i: ends are ascending, rows past the last group end at n (never reached by i < n)
__device__ __forceinline__ int group_of(const OptArgs& a, long i) {
  int k = 0;
#pragma unroll
  for (int j = 0; j < MAXG - 1; ++j) k += (i >= a.g[j].end) ? 1 : 0;
  return k;
}

// e' = e + (p - e) * omd, each of the three operations rounded on its own (the callers switch contraction off).  The lerp form: at
// decay = 0.9999 the form d*e + (1 - d)*p rounds the whole update away in f32.
__device__ __forceinline__ float ema_lerp(float e, float p_new, float omd) {
#pragma clang fp contract(off)
  const float t = p_new - e;
  const float u = t * omd;
  return e + u;
}

// EMA: the instance that also averages the new parameters into ema[] (omd from ema_state[1] after the tick, or from omd_host)
template <bool EMA>
__global__ __launch_bounds__(NT) void adamw_kernel(float* p, const float* g, float* m, float* v, long n, const OptArgs a, int ng,
                                                   const float* lr_ptr, const float* state, const float* scale_ptr,
                                                   float grad_scale_host, float* ema, const float* ema_state, float omd_host) {
  // per group: {lr, 1 - lr*weight_decay, 1 - beta1, beta2}, {1 - beta2, bc2s, eps, lr / bc1}.  Learning rate and bias corrections
  // come from the device (state, lr_ptr: the step can be replayed from a captured graph) or from the kernel arguments (one launch
  // when the optimizer step is launched eagerly).
  //
  // Rounding is spelled out (no contraction left to the compiler; the two fused operations are written as fmaf): it is the
  // arithmetic the single-group kernel has always compiled to -- every product and sum rounded on its own, except 1 - lr*wd and
  // g*scale - m -- so the parameters keep their bits whatever else changes around the expressions.
#pragma clang fp contract(off)
  __shared__ float4 tab[MAXG][2];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < MAXG; ++k) {
      if (k < ng) {
        const float beta1 = a.g[k].beta1, beta2 = a.g[k].beta2, weight_decay = a.g[k].weight_decay;
        const float lr = state ? lr_ptr[k] : a.g[k].lr;
        const float bc1 = state ? state[3 * k + 1] : a.g[k].bc1, bc2s = state ? state[3 * k + 2] : a.g[k].bc2s;
        tab[k][0] = make_float4(lr, fmaf(-lr, weight_decay, 1.f), 1.f - beta1, beta2);
        tab[k][1] = make_float4(1.f - beta2, bc2s, a.g[k].eps, lr / bc1);
      }
    }
  }
  __syncthreads();
  const float grad_scale = scale_ptr ? *scale_ptr : grad_scale_host;
  [[maybe_unused]] const float omd_e = EMA ? (ema_state ? ema_state[1] : omd_host) : 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int k = group_of(a, i);
    const float4 t0 = tab[k][0], t1 = tab[k][1];
    const float decay = t0.y, omb1 = t0.z, beta2 = t0.w, omb2 = t1.x, bc2s = t1.y, eps = t1.z, step_size = t1.w;
    const float gr = g[i], m0 = m[i];
    const float gi = gr * grad_scale;
    const float mi = m0 + fmaf(gr, grad_scale, -m0) * omb1;           // m + (g*scale - m) * (1 - beta1)
    const float vi = v[i] * beta2 + (omb2 * gi) * gi;
    const float denom = sqrtf(vi) / bc2s + eps;
    const float pi = p[i] * decay - step_size * (mi / denom);
    p[i] = pi;
    m[i] = mi; v[i] = vi;
    if constexpr (EMA) ema[i] = ema_lerp(ema[i], pi, omd_e);
  }
}

template <bool EMA>
__global__ __launch_bounds__(NT) void sgd_kernel(float* p, const float* g, float* buf, long n, const OptArgs a, int ng,
                                                 const float* lr_ptr, const float* state, const float* scale_ptr,
                                                 float grad_scale_host, int first_host, float* ema, const float* ema_state,
                                                 float omd_host) {
  // per group: {lr, weight_decay, momentum, 1 - dampening}; nesterov flags in a word of their own
  __shared__ float4 tab[MAXG];
  __shared__ int nest[MAXG];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < MAXG; ++k) {
      if (k < ng) {
        tab[k] = make_float4(state ? lr_ptr[k] : a.g[k].lr, a.g[k].weight_decay, a.g[k].beta1, 1.f - a.g[k].beta2);
        nest[k] = a.g[k].flags & TSS_OPT_NESTEROV;
      }
    }
  }
  __syncthreads();
  const float grad_scale = scale_ptr ? *scale_ptr : grad_scale_host;
  const bool first = state ? state[0] == 1.f : first_host != 0;       // every row carries the same counter
  [[maybe_unused]] const float omd_e = EMA ? (ema_state ? ema_state[1] : omd_host) : 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int k = group_of(a, i);
    const float4 t = tab[k];
    const float lr = t.x, weight_decay = t.y, mu = t.z, omd = t.w;
    float gi = g[i] * grad_scale;
    const float pi = p[i];
    if (weight_decay != 0.f) gi += weight_decay * pi;
    if (mu != 0.f) {                                                   // a group without momentum never touches buf
      const float b = first ? gi : mu * buf[i] + omd * gi;
      buf[i] = b;
      gi = nest[k] ? gi + mu * b : b;
    }
    const float pn = pi - lr * gi;
    p[i] = pn;
    if constexpr (EMA) ema[i] = ema_lerp(ema[i], pn, omd_e);
  }
}

// ------------------------------------------------------------------------------------------ gradient norm
constexpr int NORM_MAX_BLOCKS = 1024;
inline int norm_blocks(long n) {            // a function of n only: the summation order (and so the bits) is fixed by n
  long b = (n + 4095) / 4096;               // 4 float4 per thread before the grid is capped
  if (b < 1) b = 1;
  if (b > NORM_MAX_BLOCKS) b = NORM_MAX_BLOCKS;
  return (int)b;
}

// rows[block] = sum of the squares of this block's elements: f32 -> f64 (exact squares), f64 adds, plain store
__global__ __launch_bounds__(NT) void grad_sqnorm_kernel(const float* g, long n, double* rows) {
  __shared__ double red[NT / TSS_WAVE];
  const long n4 = n >> 2;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  double acc = 0.0;
#pragma unroll 4
  for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT) {
    const float4 x = g4[i];
    const double a = (double)x.x, b = (double)x.y, c = (double)x.z, d = (double)x.w;
    acc += a * a; acc += b * b; acc += c * c; acc += d * d;
  }
  if (blockIdx.x == 0 && n4 * 4 + threadIdx.x < n) {                   // up to 3 tail elements
    const double a = (double)g[n4 * 4 + threadIdx.x];
    acc += a * a;
  }
  acc = wave_sum(acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = red[0];
#pragma unroll
    for (int w = 1; w < NT / TSS_WAVE; ++w) s += red[w];
    rows[blockIdx.x] = s;
  }
}

// one block: the rows in a fixed order (the shape of lsw::row_sum2), then norm and clip factor in f64, rounded once each
__global__ __launch_bounds__(NT) void grad_sqnorm_final_kernel(const double* rows, int nrows, float grad_scale, float max_norm,
                                                               float* out) {
  __shared__ double red[NT];
  double a = 0.0;
  for (int i = threadIdx.x; i < nrows; i += NT) a += rows[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double norm = (double)grad_scale * sqrt(red[0]);
    double coef = (double)max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;                 // written so that a NaN norm stays NaN, as torch.clamp(max=1.0) leaves it
    out[0] = (float)norm;
    out[1] = (float)((double)grad_scale * coef);
  }
}

// ------------------------------------------------------------------------------------------ moving average over a table of rows
constexpr int ROWS_BLOCKS = 32;             // blocks per row: the rows are BatchNorm vectors and single parameter tensors

// table: [nrows][4] int64 {src, dst, n, mode}.  Block (x, y) strides over the elements of rows y, y + gridDim.y, ...; 16-byte
// accesses only over the part of a row where source and destination are both 16-byte aligned (same offset within 16 bytes), scalar
// ones before, after and otherwise.  Nothing outside [dst, dst + n) is written.
__global__ __launch_bounds__(NT) void ema_rows_kernel(const long long* table, int nrows, const float* ema_state, float omd_host) {
#pragma clang fp contract(off)
  const float omd = ema_state ? ema_state[1] : omd_host;
  const long tid = (long)blockIdx.x * NT + threadIdx.x, nth = (long)gridDim.x * NT;
  for (int r = blockIdx.y; r < nrows; r += gridDim.y) {
    const long long* t = table + 4l * r;
    const long n = t[2];
    const int mode = (int)t[3];
    if (mode == TSS_EMA_COPY_I64) {
      const long long* src = reinterpret_cast<const long long*>(t[0]);
      long long* dst = reinterpret_cast<long long*>(t[1]);
      for (long i = tid; i < n; i += nth) dst[i] = src[i];
      continue;
    }
    const float* src = reinterpret_cast<const float*>(t[0]);
    float* dst = reinterpret_cast<float*>(t[1]);
    const bool lerp = mode == TSS_EMA_LERP_F32;
    const unsigned long sa = (unsigned long)t[0] & 15u, da = (unsigned long)t[1] & 15u;
    long head = n, n4 = 0;                  // scalar elements in front, float4 groups behind them
    if (sa == da) {
      head = (long)((16u - da) & 15u) >> 2;
      if (head > n) head = n;
      n4 = (n - head) >> 2;
    }
    const long tail = head + 4 * n4;        // first scalar element behind the float4 groups
    const float4* s4 = reinterpret_cast<const float4*>(src + head);
    float4* d4 = reinterpret_cast<float4*>(dst + head);
    for (long i = tid; i < n4; i += nth) {
      const float4 s = s4[i];
      if (lerp) {
        const float4 e = d4[i];
        d4[i] = make_float4(ema_lerp(e.x, s.x, omd), ema_lerp(e.y, s.y, omd), ema_lerp(e.z, s.z, omd), ema_lerp(e.w, s.w, omd));
      } else {
        d4[i] = s;
      }
    }
    for (long j = tid; j < head + (n - tail); j += nth) {
      const long i = j < head ? j : tail + (j - head);
      dst[i] = lerp ? ema_lerp(dst[i], src[i], omd) : src[i];
    }
  }
}

// decay in [0, 1); the factor a host passes for it lies in (0, 1] (warm-up only lowers the decay)
inline bool ema_args_ok(float decay, float omd_host, bool on_device, const float* ema_state) {
  if (!(decay >= 0.f && decay < 1.f)) return false;
  return on_device ? ema_state != nullptr : (omd_host > 0.f && omd_host <= 1.f);
}

// the caller's rows -> kernel arguments; false when they are not consecutive ranges covering [0, n)
bool fill_args(const tss_optgroup* groups, int ng, long n, OptArgs* a) {
  if (!groups || ng < 1 || ng > MAXG || n < 0) return false;
  long at = 0;
  for (int k = 0; k < MAXG; ++k) {
    OptRow& r = a->g[k];
    if (k < ng) {
      const tss_optgroup& s = groups[k];
      if (s.begin != at || s.end < s.begin) return false;
      at = s.end;
      r.end = s.end; r.lr = s.lr; r.weight_decay = s.weight_decay; r.beta1 = s.beta1; r.beta2 = s.beta2; r.eps = s.eps;
      r.bc1 = 1.f; r.bc2s = 1.f; r.flags = s.flags;
    } else {
      r = OptRow{n, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f, 1.f, 0};
    }
  }
  return at == n;
}

inline int step_grid(long n) {
  long grid = (n + NT - 1) / NT;
  if (grid > 2048) grid = 2048;
  return (int)grid;
}

}  // namespace

extern "C" {

int tss_adamw_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n,
                          const tss_optgroup* groups, int ngroups, const float* lr, float* state /*[ngroups][3]*/,
                          const float* scale, float grad_scale, long step_host, void* stream) {
  OptArgs a;
  TSS_REQUIRE(fill_args(groups, ngroups, n, &a) && (state ? lr != nullptr : step_host >= 1), TSS_ERR_SHAPE);
  if (state) hipLaunchKernelGGL(optim_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, a, ngroups, 1, nullptr, 0.f, 0);
  else {
    for (int k = 0; k < ngroups; ++k) {       // as optim_tick_kernel
      a.g[k].bc1 = 1.f - powf(a.g[k].beta1, (float)step_host);
      a.g[k].bc2s = sqrtf(1.f - powf(a.g[k].beta2, (float)step_host));
    }
  }
  if (n == 0) return tss::check_last("adamw_tick");
  tss::ProfScope prof(TSS_K_ADAMW, (hipStream_t)stream, 28.0 * n, 12.0 * n);
  hipLaunchKernelGGL(adamw_kernel<false>, dim3(step_grid(n)), dim3(NT), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, n,
                     a, ngroups, lr, state, scale, grad_scale, nullptr, nullptr, 0.f);
  return tss::check_last("adamw");
}

int tss_adamw_step_groups_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, long n,
                              const tss_optgroup* groups, int ngroups, const float* lr, float* state /*[ngroups][3]*/,
                              const float* scale, float grad_scale, long step_host, float decay, int warmup, float omd_host,
                              float* ema_state /*[2]*/, void* stream) {
  OptArgs a;
  TSS_REQUIRE(fill_args(groups, ngroups, n, &a) && (state ? lr != nullptr : step_host >= 1), TSS_ERR_SHAPE);
  TSS_REQUIRE(ema != nullptr && ema_args_ok(decay, omd_host, state != nullptr, ema_state), TSS_ERR_SHAPE);
  if (state) {
    hipLaunchKernelGGL(optim_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, a, ngroups, 1, ema_state, decay, warmup);
  } else {
    for (int k = 0; k < ngroups; ++k) {       // as optim_tick_kernel
      a.g[k].bc1 = 1.f - powf(a.g[k].beta1, (float)step_host);
      a.g[k].bc2s = sqrtf(1.f - powf(a.g[k].beta2, (float)step_host));
    }
  }
  if (n == 0) return tss::check_last("adamw_tick");
  tss::ProfScope prof(TSS_K_ADAMW, (hipStream_t)stream, 36.0 * n, 15.0 * n);
  hipLaunchKernelGGL(adamw_kernel<true>, dim3(step_grid(n)), dim3(NT), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, n,
                     a, ngroups, lr, state, scale, grad_scale, ema, state ? ema_state : nullptr, omd_host);
  return tss::check_last("adamw_ema");
}

int tss_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n,
                   const float* lr, float beta1, float beta2, float eps, float weight_decay,
                   float* state /*[3]: step, bc1, sqrt(bc2)*/, float grad_scale, float lr_host, long step_host, void* stream) {
  const tss_optgroup one = {0, n, lr_host, weight_decay, beta1, beta2, eps, 0};
  return tss_adamw_step_groups(params, grads, exp_avg, exp_avg_sq, n, &one, 1, lr, state, nullptr, grad_scale, step_host, stream);
}

int tss_sgd_step_groups(float* params, const float* grads, float* momentum_buf, long n, const tss_optgroup* groups, int ngroups,
                        const float* lr, float* state /*[ngroups][3]*/, const float* scale, float grad_scale, long step_host,
                        void* stream) {
  OptArgs a;
  TSS_REQUIRE(fill_args(groups, ngroups, n, &a) && (state ? lr != nullptr : step_host >= 1), TSS_ERR_SHAPE);
  for (int k = 0; k < ngroups; ++k) TSS_REQUIRE(a.g[k].beta1 == 0.f || momentum_buf != nullptr, TSS_ERR_SHAPE);
  if (state) hipLaunchKernelGGL(optim_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, a, ngroups, 0, nullptr, 0.f, 0);
  if (n == 0) return tss::check_last("sgd_tick");
  tss::ProfScope prof(TSS_K_SGD, (hipStream_t)stream, (momentum_buf ? 20.0 : 12.0) * n, 6.0 * n);
  hipLaunchKernelGGL(sgd_kernel<false>, dim3(step_grid(n)), dim3(NT), 0, (hipStream_t)stream, params, grads, momentum_buf, n, a,
                     ngroups, lr, state, scale, grad_scale, step_host == 1 ? 1 : 0, nullptr, nullptr, 0.f);
  return tss::check_last("sgd");
}

int tss_sgd_step_groups_ema(float* params, const float* grads, float* momentum_buf, float* ema, long n, const tss_optgroup* groups,
                            int ngroups, const float* lr, float* state /*[ngroups][3]*/, const float* scale, float grad_scale,
                            long step_host, float decay, int warmup, float omd_host, float* ema_state /*[2]*/, void* stream) {
  OptArgs a;
  TSS_REQUIRE(fill_args(groups, ngroups, n, &a) && (state ? lr != nullptr : step_host >= 1), TSS_ERR_SHAPE);
  for (int k = 0; k < ngroups; ++k) TSS_REQUIRE(a.g[k].beta1 == 0.f || momentum_buf != nullptr, TSS_ERR_SHAPE);
  TSS_REQUIRE(ema != nullptr && ema_args_ok(decay, omd_host, state != nullptr, ema_state), TSS_ERR_SHAPE);
  if (state) {
    hipLaunchKernelGGL(optim_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, a, ngroups, 0, ema_state, decay, warmup);
  }
  if (n == 0) return tss::check_last("sgd_tick");
  tss::ProfScope prof(TSS_K_SGD, (hipStream_t)stream, (momentum_buf ? 28.0 : 20.0) * n, 9.0 * n);
  hipLaunchKernelGGL(sgd_kernel<true>, dim3(step_grid(n)), dim3(NT), 0, (hipStream_t)stream, params, grads, momentum_buf, n, a,
                     ngroups, lr, state, scale, grad_scale, step_host == 1 ? 1 : 0, ema, state ? ema_state : nullptr, omd_host);
  return tss::check_last("sgd_ema");
}

int tss_ema_rows(const long long* table, int nrows, float omd_host, const float* ema_state, void* stream) {
  TSS_REQUIRE(nrows >= 0 && (nrows == 0 || table != nullptr), TSS_ERR_SHAPE);
  TSS_REQUIRE(ema_state != nullptr || (omd_host > 0.f && omd_host <= 1.f), TSS_ERR_SHAPE);
  if (nrows == 0) return TSS_OK;
  hipLaunchKernelGGL(ema_rows_kernel, dim3(ROWS_BLOCKS, nrows < 4096 ? nrows : 4096), dim3(NT), 0, (hipStream_t)stream, table, nrows,
                     ema_state, omd_host);
  return tss::check_last("ema_rows");
}

long tss_grad_sqnorm_workspace_bytes(long n) { return (long)sizeof(double) * norm_blocks(n < 0 ? 0 : n); }

int tss_grad_sqnorm(const float* grads, long n, double* workspace, float grad_scale, float max_norm, float* out, void* stream) {
  TSS_REQUIRE(n >= 0 && workspace && out && (n == 0 || grads), TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(grads), TSS_ERR_ALIGN);
  const int blocks = norm_blocks(n);
  tss::ProfScope prof(TSS_K_GRAD_NORM, (hipStream_t)stream, 4.0 * n, 2.0 * n);
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, grads, n, workspace);
  hipLaunchKernelGGL(grad_sqnorm_final_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, workspace, blocks, grad_scale, max_norm,
                     out);
  return tss::check_last("grad_sqnorm");
}

}  // extern "C"
