// Per-class label histogram (the counts that class-balancing weights come from).  Integer arithmetic only (exact, independent
// of the order).  One lane owns 8 consecutive labels and folds runs of equal labels among them into one LDS add, a block counts
// into LDS counters and adds every non-zero counter to the caller's int64 buffer with one integer atomic per class: the buffer
// accumulates over calls.  max_blocks > 0 caps the grid.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int HIST_MAX_C = 4096;          // LDS counters of the histogram (16 KiB)
constexpr int HIST_BLOCKS = 1024;

inline int grid_of(long groups, int max_blocks, long default_cap) {
  return tss::grid_for(groups, NT, max_blocks > 0 ? (long)max_blocks : default_cap);
}

// counts[c] += number of labels equal to c among target[0..n) that are not ignore_index (has_ignore) and lie in [0, C)
__global__ __launch_bounds__(NT) void label_histogram_kernel(const long long* __restrict__ target, unsigned long long* counts, long n,
                                                             int C, int ignore_index, int has_ignore) {
  __shared__ unsigned int cnt[HIST_MAX_C];
  for (int c = threadIdx.x; c < C; c += NT) cnt[c] = 0u;
  __syncthreads();
  const long groups = (n + 7) / 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += (long)gridDim.x * blockDim.x) {
    const long first = i * 8;
    int cur = -1;
    unsigned int run = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int c = -1;
      if (first + j < n) {
        const long long t = target[first + j];
        if ((!has_ignore || t != (long long)ignore_index) && t >= 0 && t < C) c = (int)t;
      }
      if (c != cur) {
        if (cur >= 0) atomicAdd(&cnt[cur], run);
        cur = c;
        run = 0u;
      }
      ++run;
    }
    if (cur >= 0) atomicAdd(&cnt[cur], run);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += NT)
    if (cnt[c]) atomicAdd(counts + c, (unsigned long long)cnt[c]);
}

}  // namespace

extern "C" {

int tss_label_histogram_max_classes(void) { return HIST_MAX_C; }

int tss_label_histogram(const long long* target, long long* counts, long n, int C, int ignore_index, int has_ignore, int max_blocks,
                        void* stream) {
  TSS_REQUIRE(n >= 0 && n < (1L << 40) && C > 0 && C <= HIST_MAX_C && max_blocks >= 0 && counts && (target || n == 0), TSS_ERR_SHAPE);
  if (n == 0) return TSS_OK;
  hipLaunchKernelGGL(label_histogram_kernel, dim3(grid_of((n + 7) / 8, max_blocks, HIST_BLOCKS)), dim3(NT), 0, (hipStream_t)stream, target,
                     reinterpret_cast<unsigned long long*>(counts), n, C, ignore_index, has_ignore);
  return tss::check_last("label_histogram");
}

}  // extern "C"
