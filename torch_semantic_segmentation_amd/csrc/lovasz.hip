// Lovasz-Softmax loss (TSS/losses/lovasz_softmax_loss.py:7-59), the mIoU surrogate of the Cityscapes recipes.
//   per present class c:  e_i = |fg_i - p_ic|, pixels ordered by descending e, F_r = #foreground among ranks <= r,
//   G = #foreground, J_r = 1 - (G - F_r) / (G + (r+1) - F_r),  loss_c = sum_r e_(r) g_r,  loss = mean_c loss_c
//   variant 0 ('reference'): g_0 = J_0, g_r = J_r - J_0      (lovasz_grad :15-16 as the reference runs it)
//   variant 1 ('berman')   : g_0 = J_0, g_r = J_r - J_{r-1}  (the published successive difference)
// The reference runs C full argsorts, cumsums and a host sync per class; here, per chunk of classes:
//   key build -> 4 x (tile histogram, digit totals, offset scan, stable scatter) -> tile fg counts -> their scan ->
//   closed-form weights, f64 dot product and the scatter of g_rank into a [C][pixels] plane for the backward.
// Segments (classes) are on blockIdx.y and have equal length B*HW: a dropped pixel keeps its slot with a key that
// sorts after every kept one, so kept ranks are unaffected, and it gets weight 0.
// Key: e is in [0,1].  f32 resolves e near 0 to 2^-24 relative but near 1 only to 2^-24 absolute, and errors near 1
// (confident and wrong) hold the first ranks, where a swapped pair moves g the most.  So the key is symmetric:
//   k(e) = bits(e) for e <= 1/2,  2 bits(1/2) - bits(1 - e) above   (1 - e exact in f64; monotonic; k <= 0x7E000000)
// and the sorted key is 0x7E000000 - k, ascending in it = descending in e; dropped pixels carry 0xFFFFFFFF.  The error is
// read back from the key (above 1/2 as 1 - f32(1 - e), in f64).  The LSD sort is stable, which IS the tie rule: equal
// keys keep ascending pixel index.  Integer LDS atomics only build histograms; placement uses a within-tile rank from wave ballots.  No
// floating-point atomics anywhere, every f64 sum has a fixed tree: the result is bit-reproducible.
// The softmax is evaluated in f64 and the error rounded once, into the key, so the order is that of the exact errors to
// 2^-24 relative at both ends (an f32 softmax swaps near-equal errors, and a swapped pair moves g by O(1/U)); ranks and
// counts are integers, g is f64.
#include "losssweep.h"

namespace {

constexpr int NT = lsw::NT;
constexpr int WAVES = NT / 64;
constexpr int ITEMS = 16;                 // elements per lane and tile: 48 VGPRs of (key, payload, rank) in the scatter
constexpr int TILE = NT * ITEMS;          // 4096 pairs per block; a wave owns 1024 consecutive ones
constexpr unsigned int HALF_BITS = 0x3F000000u;
constexpr unsigned int KEY_MAX = 2u * HALF_BITS;
constexpr unsigned int DROPPED = 0xFFFFFFFFu;
constexpr long SORT_BYTES_CAP = 2L << 30;  // bound on the (key, payload) double buffers; more classes -> several chunks

struct Plan {
  long N, ntiles;
  int C, Cc;                              // classes, classes per chunk
  size_t off_G, off_partial, off_W, off_key0, off_key1, off_pay0, off_pay1, off_hist, off_dtot, off_tcnt, total;
};

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// chunk_classes > 0 overrides the bound (tests and tools: the chunked path at small sizes)
inline Plan make_plan(long N, int C, int chunk_classes) {
  Plan p;
  p.N = N; p.C = C;
  p.ntiles = (N + TILE - 1) / TILE;
  long cc = chunk_classes > 0 ? chunk_classes : SORT_BYTES_CAP / (16 * N);
  p.Cc = (int)(cc < 1 ? 1 : (cc > C ? C : cc));
  size_t o = 0;
  p.off_G = o;       o = up256(o + sizeof(unsigned int) * C);
  p.off_partial = o; o = up256(o + sizeof(double) * C * p.ntiles);
  p.off_W = o;       o = up256(o + sizeof(float) * C * N);               // g_rank per class and pixel: all the backward reads
  const size_t plane = up256(sizeof(unsigned int) * (size_t)p.Cc * N);
  p.off_key0 = o; o += plane;
  p.off_key1 = o; o += plane;
  p.off_pay0 = o; o += plane;
  p.off_pay1 = o; o += plane;
  p.off_hist = o;    o = up256(o + sizeof(unsigned int) * (size_t)p.Cc * 256 * p.ntiles);
  p.off_dtot = o;    o = up256(o + sizeof(unsigned int) * (size_t)p.Cc * 256);
  p.off_tcnt = o;    o = up256(o + sizeof(unsigned int) * (size_t)p.Cc * p.ntiles);
  p.total = o;
  return p;
}

// exclusive scan of one value per thread over the block (fixed order); total in every thread
__device__ __forceinline__ unsigned int block_excl_scan(unsigned int v, unsigned int* wsum /*[WAVES]*/, unsigned int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned int x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned int t = __shfl_up(x, off, 64);
    if (lane >= off) x += t;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  unsigned int before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const unsigned int s = wsum[w];
    if (w < wave) before += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return before + x - v;
}

// softmax statistics of 8 neighbouring pixels in f64: row maximum and 1 / sum(exp(z - max))
template <typename T>
__device__ __forceinline__ void softmax_stats(const T* base, int C, long HW, float m[8], double inv[8]) {
  double s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { m[j] = -INFINITY; s[j] = 0.0; }
  for (int c = 0; c < C; ++c) {
    float v[8];
    V8<T>::load(base + (long)c * HW, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], v[j]);
  }
  for (int c = 0; c < C; ++c) {
    float v[8];
    V8<T>::load(base + (long)c * HW, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += exp((double)v[j] - (double)m[j]);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) inv[j] = 1.0 / s[j];
}

// sorted key of an error in [0,1] (see the top of the file), and the error back from it
__device__ __forceinline__ unsigned int error_key(double e) {
  e = fmin(fmax(e, 0.0), 1.0);
  const unsigned int k = e <= 0.5 ? __float_as_uint((float)e) : KEY_MAX - __float_as_uint((float)(1.0 - e));
  return KEY_MAX - k;
}
__device__ __forceinline__ double key_error(unsigned int key) {
  const unsigned int k = KEY_MAX - key;
  return k <= HALF_BITS ? (double)__uint_as_float(k) : 1.0 - (double)__uint_as_float(KEY_MAX - k);
}

// classes [c0, c1): key and payload (pixel | fg << 31) of every pixel, planes of N per class
template <typename T>
__global__ __launch_bounds__(NT) void lovasz_key_kernel(const T* logits, const long long* target, unsigned int* keys,
                                                        unsigned int* pay, long B, int C, long HW, int c0, int c1,
                                                        int ignore_index, int has_ignore) {
  const long N = B * HW;
  for (lsw::Groups g(B, HW); g.more(); g.next()) {
    const long b = g.b(), off = g.off();
    const long pix = b * HW + off;
    const T* base = logits + b * C * HW + off;
    int tv[8];
    lsw::load_labels(target + pix, C, ignore_index, has_ignore, tv);
    float m[8];
    double inv[8];
    softmax_stats(base, C, HW, m, inv);
    for (int c = c0; c < c1; ++c) {
      float v[8];
      V8<T>::load(base + (long)c * HW, v);
      unsigned int k[8], q[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const double p = exp((double)v[j] - (double)m[j]) * inv[j];
        const unsigned int fg = tv[j] == c ? 1u : 0u;
        const bool kept = tv[j] != lsw::IGNORED;       // an out-of-range label is background, not dropped
        k[j] = kept ? error_key(fabs((double)fg - p)) : DROPPED;
        q[j] = (unsigned int)(pix + j) | ((kept ? fg : 0u) << 31);
      }
      uint4* kd = reinterpret_cast<uint4*>(keys + (size_t)(c - c0) * N + pix);
      uint4* qd = reinterpret_cast<uint4*>(pay + (size_t)(c - c0) * N + pix);
      kd[0] = make_uint4(k[0], k[1], k[2], k[3]); kd[1] = make_uint4(k[4], k[5], k[6], k[7]);
      qd[0] = make_uint4(q[0], q[1], q[2], q[3]); qd[1] = make_uint4(q[4], q[5], q[6], q[7]);
    }
  }
}

// hist[class][digit][tile]: digit counts of one tile (digit-major, so the offsets are one scan along a class's rows)
__global__ __launch_bounds__(NT) void lovasz_hist_kernel(const unsigned int* keys, unsigned int* hist, long N, long ntiles, int shift) {
  __shared__ unsigned int h[256];
  const int tid = threadIdx.x;
  const long tile = blockIdx.x, cc = blockIdx.y;
  h[tid] = 0u;
  __syncthreads();
  const unsigned int* k = keys + (size_t)cc * N;
  const long start = tile * TILE;
#pragma unroll 4
  for (int j = 0; j < ITEMS; ++j) {
    const long i = start + (long)j * NT + tid;
    if (i < N) atomicAdd(&h[(k[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[((size_t)cc * 256 + tid) * ntiles + tile] = h[tid];
}

// dtot[class][digit] = sum over tiles; block (digit, class)
__global__ __launch_bounds__(NT) void lovasz_digit_total_kernel(const unsigned int* hist, unsigned int* dtot, long ntiles) {
  __shared__ unsigned int wsum[WAVES];
  const size_t row = (size_t)blockIdx.y * 256 + blockIdx.x;
  const unsigned int* r = hist + row * ntiles;
  unsigned int s = 0;
  for (long i = threadIdx.x; i < ntiles; i += NT) s += r[i];
  unsigned int tot;
  block_excl_scan(s, wsum, &tot);
  if (threadIdx.x == 0) dtot[row] = tot;
}

// hist row (digit, class) -> position of the tile's first element with that digit: all smaller digits, then earlier tiles
__global__ __launch_bounds__(NT) void lovasz_offset_kernel(unsigned int* hist, const unsigned int* dtot, long ntiles) {
  __shared__ unsigned int wsum[WAVES];
  const int d = blockIdx.x;
  const size_t row = (size_t)blockIdx.y * 256 + d;
  unsigned int carry;
  block_excl_scan((int)threadIdx.x < d ? dtot[(size_t)blockIdx.y * 256 + threadIdx.x] : 0u, wsum, &carry);
  unsigned int* r = hist + row * ntiles;
  for (long i0 = 0; i0 < ntiles; i0 += NT) {
    const long i = i0 + threadIdx.x;
    const unsigned int v = i < ntiles ? r[i] : 0u;
    unsigned int tot;
    const unsigned int ex = block_excl_scan(v, wsum, &tot);
    if (i < ntiles) r[i] = carry + ex;
    carry += tot;
  }
}

// Stable scatter of one tile.  A wave owns 1024 consecutive elements and takes them 64 at a time, lane = position, so
// (wave, round, lane) is the input order.  Rank among equal digits = wave-private running count (LDS, one writer per
// digit group: its lowest lane) + equal digits in lower lanes (8 ballots).  Lanes past the end of the class act as the
// largest digit; they come after every real element of the tile, so they shift no real rank, and they are not written.
__global__ __launch_bounds__(NT) void lovasz_scatter_kernel(const unsigned int* kin, const unsigned int* pin, unsigned int* kout,
                                                            unsigned int* pout, const unsigned int* offs, long N, long ntiles, int shift) {
  __shared__ unsigned int cnt_s[WAVES][256];
  __shared__ unsigned int gbase[256];
  volatile unsigned int (*cnt)[256] = cnt_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long tile = blockIdx.x, cc = blockIdx.y;
  const size_t seg = (size_t)cc * N;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) cnt[w][tid] = 0u;
  gbase[tid] = offs[((size_t)cc * 256 + tid) * ntiles + tile];
  __syncthreads();
  const long chunk = tile * TILE + (long)wave * 64 * ITEMS;
  const unsigned long long lt = (1ull << lane) - 1ull;
  unsigned int k[ITEMS], q[ITEMS], rk[ITEMS];
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const long i = chunk + j * 64 + lane;
    k[j] = i < N ? kin[seg + i] : DROPPED;
    q[j] = i < N ? pin[seg + i] : 0u;
  }
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const unsigned int d = (k[j] >> shift) & 255u;
    unsigned long long same = ~0ull;
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1u;
      const unsigned long long bal = __ballot(on);
      same &= on ? bal : ~bal;
    }
    const unsigned int prior = cnt[wave][d];
    __builtin_amdgcn_wave_barrier();
    const unsigned int below = __popcll(same & lt);
    if (below == 0) cnt[wave][d] = prior + __popcll(same);
    __builtin_amdgcn_wave_barrier();
    rk[j] = prior + below;
  }
  __syncthreads();
  {
    unsigned int run = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) { const unsigned int t = cnt[w][tid]; cnt[w][tid] = run; run += t; }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const long i = chunk + j * 64 + lane;
    if (i < N) {
      const unsigned int d = (k[j] >> shift) & 255u;
      const size_t pos = seg + gbase[d] + cnt[wave][d] + rk[j];
      kout[pos] = k[j];
      pout[pos] = q[j];
    }
  }
}

// foreground count of every tile of the sorted payloads
__global__ __launch_bounds__(NT) void lovasz_fgcount_kernel(const unsigned int* pay, unsigned int* tcnt, long N, long ntiles) {
  __shared__ unsigned int wsum[WAVES];
  const long tile = blockIdx.x, cc = blockIdx.y;
  const unsigned int* q = pay + (size_t)cc * N;
  unsigned int s = 0;
#pragma unroll 4
  for (int j = 0; j < ITEMS; ++j) {
    const long i = tile * TILE + (long)j * NT + threadIdx.x;
    if (i < N) s += q[i] >> 31;
  }
  unsigned int tot;
  block_excl_scan(s, wsum, &tot);
  if (threadIdx.x == 0) tcnt[cc * ntiles + tile] = tot;
}

// one block per class: tile counts -> foreground before the tile; the total is G
__global__ __launch_bounds__(NT) void lovasz_tilescan_kernel(unsigned int* tcnt, unsigned int* G, long ntiles, int c0) {
  __shared__ unsigned int wsum[WAVES];
  unsigned int* r = tcnt + (size_t)blockIdx.x * ntiles;
  unsigned int carry = 0;
  for (long i0 = 0; i0 < ntiles; i0 += NT) {
    const long i = i0 + threadIdx.x;
    const unsigned int v = i < ntiles ? r[i] : 0u;
    unsigned int tot;
    const unsigned int ex = block_excl_scan(v, wsum, &tot);
    if (i < ntiles) r[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) G[c0 + blockIdx.x] = carry;
}

// g_r in closed form from integers (I = G - F_r, U = G + (r+1) - F_r; J_r = (r+1)/U since U - I = r+1):
//   berman   : 1/U at a foreground rank, I / (U (U-1)) at a background rank (rank 0 included: both equal J_0)
//   reference: J_0 = 1/U_0 at rank 0, else (r+1)/U - 1/U_0 = ((r+1) U_0 - U) / (U U_0), the numerator exact (< 2^53)
// writes g into W[class][pixel] (a permutation: no conflicts) and the tile's part of sum_r e_r g_r in f64.
__global__ __launch_bounds__(NT) void lovasz_weight_kernel(const unsigned int* keys, const unsigned int* pay, const unsigned int* tbase,
                                                           const unsigned int* G, float* W, double* partial, long N, long ntiles,
                                                           int c0, int variant) {
  __shared__ unsigned int wfg_s[WAVES];
  __shared__ double wacc[WAVES];
  volatile unsigned int* wfg = wfg_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long tile = blockIdx.x, cc = blockIdx.y;
  const int c = c0 + (int)cc;
  const size_t seg = (size_t)cc * N;
  float* Wc = W + (size_t)c * N;
  const long long Gc = G[c];
  if (Gc == 0) {                              // absent class: no loss, zero gradient
#pragma unroll 4
    for (int j = 0; j < ITEMS; ++j) {
      const long i = tile * TILE + (long)j * NT + tid;
      if (i < N) Wc[i] = 0.f;
    }
    if (tid == 0) partial[(size_t)c * ntiles + tile] = 0.0;
    return;
  }
  const long chunk = tile * TILE + (long)wave * 64 * ITEMS;
  unsigned int k[ITEMS], q[ITEMS];
  unsigned int mine = 0;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const long i = chunk + j * 64 + lane;
    k[j] = i < N ? keys[seg + i] : DROPPED;
    q[j] = i < N ? pay[seg + i] : 0u;
    mine += q[j] >> 31;
  }
  mine = (unsigned int)wave_sum((float)mine);          // <= 1024: exact in f32
  if (lane == 0) wfg[wave] = mine;
  __syncthreads();
  long long F = tbase[cc * ntiles + tile];
  for (int w = 0; w < wave; ++w) F += wfg[w];
  const long long U0 = (pay[seg] >> 31) ? Gc : Gc + 1;  // rank 0 is a kept pixel whenever G > 0
  const unsigned long long le = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const long i = chunk + j * 64 + lane;
    const unsigned int fg = q[j] >> 31;
    const unsigned long long bal = __ballot(fg != 0u);
    const long long Fr = F + __popcll(bal & le);
    F += __popcll(bal);
    if (i < N) {
      float g = 0.f;
      if (k[j] != DROPPED) {
        const long long I = Gc - Fr, U = Gc + (i + 1) - Fr;
        double gd;
        if (variant == 1 || i == 0) gd = fg ? 1.0 / (double)U : (double)I / ((double)U * (double)(U - 1));
        else gd = (double)((i + 1) * U0 - U) / ((double)U * (double)U0);
        g = (float)gd;
        acc += key_error(k[j]) * gd;
      }
      Wc[q[j] & 0x7FFFFFFFu] = g;
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) wacc[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < WAVES; ++w) s += wacc[w];
    partial[(size_t)c * ntiles + tile] = s;
  }
}

// one block: loss_c = sum of the tile parts (fixed tree), loss = mean over the present classes (0 when there is none)
__global__ __launch_bounds__(NT) void lovasz_final_kernel(const double* partial, const unsigned int* G, float* loss, float* n_present,
                                                          int C, long ntiles) {
  __shared__ double wacc[WAVES];
  double total = 0.0;
  int present = 0;
  for (int c = 0; c < C; ++c) {
    double s = 0.0;
    for (long i = threadIdx.x; i < ntiles; i += NT) s += partial[(size_t)c * ntiles + i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) wacc[threadIdx.x >> 6] = s;
    __syncthreads();
    if (G[c] > 0u) {
      double lc = 0.0;
      for (int w = 0; w < WAVES; ++w) lc += wacc[w];
      total += lc;
      ++present;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *loss = present > 0 ? (float)(total / (double)present) : 0.f;
    *n_present = (float)present;
  }
}

// dloss/dp_ic = g_rank(i) * (-sign(fg_i - p_ic)) / n_present (0 where the error is 0), then the softmax Jacobian
template <typename T>
__global__ __launch_bounds__(NT) void lovasz_bwd_kernel(const T* logits, const long long* target, const float* W, const float* n_present,
                                                        const float* grad_out, T* dlogits, long B, int C, long HW) {
  const long N = B * HW;
  const double np = (double)*n_present;
  const double scale = np > 0.0 ? (double)(grad_out ? *grad_out : 1.f) / np : 0.0;
  for (lsw::Groups g(B, HW); g.more(); g.next()) {
    const long b = g.b(), off = g.off();
    const long pix = b * HW + off;
    const T* base = logits + b * C * HW + off;
    int tv[8];
    lsw::load_labels(target + pix, C, 0, 0, tv);         // the foreground term only: a dropped pixel has weight 0 in W
    float m[8];
    double inv[8], dot[8];
    softmax_stats(base, C, HW, m, inv);
#pragma unroll
    for (int j = 0; j < 8; ++j) dot[j] = 0.0;
    for (int c = 0; c < C; ++c) {
      float v[8], w[8];
      V8<T>::load(base + (long)c * HW, v);
      V8<float>::load(W + (size_t)c * N + pix, w);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const double p = exp((double)v[j] - (double)m[j]) * inv[j];
        const double diff = (tv[j] == c ? 1.0 : 0.0) - p;
        const double D = diff > 0.0 ? -(double)w[j] : (diff < 0.0 ? (double)w[j] : 0.0);
        dot[j] += D * p;
      }
    }
    for (int c = 0; c < C; ++c) {
      float v[8], w[8], d[8];
      V8<T>::load(base + (long)c * HW, v);
      V8<float>::load(W + (size_t)c * N + pix, w);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const double p = exp((double)v[j] - (double)m[j]) * inv[j];
        const double diff = (tv[j] == c ? 1.0 : 0.0) - p;
        const double D = diff > 0.0 ? -(double)w[j] : (diff < 0.0 ? (double)w[j] : 0.0);
        d[j] = (float)(p * (D - dot[j]) * scale);
      }
      V8<T>::store(dlogits + (b * C + c) * HW + off, d);
    }
  }
}

// the planar rule, and pixel indices and tile counts that fit the 31-bit payload / an int grid
inline bool shape_ok(long B, int C, long HW) {
  return tss::planar_shape_ok(B, C, HW) && B * HW < (1L << 31) && (B * HW + TILE - 1) / TILE <= 0x7FFFFFFFL;
}

}  // namespace

extern "C" {

long tss_lovasz_workspace_bytes(long n_pixels, int C, int chunk_classes) {
  if (n_pixels <= 0 || C <= 0 || n_pixels >= (1L << 31)) return 0;
  return (long)make_plan(n_pixels, C, chunk_classes).total;
}

int tss_lovasz_fwd(const void* logits, const long long* target, void* workspace, float* loss, float* n_present,
                   long B, int C, long HW, int ignore_index, int has_ignore, int variant, int chunk_classes, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(shape_ok(B, C, HW) && (variant == 0 || variant == 1) && chunk_classes >= 0 && target && loss && n_present, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(logits) && workspace && (reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, TSS_ERR_ALIGN);
  hipStream_t st = (hipStream_t)stream;
  const long N = B * HW;
  const Plan pl = make_plan(N, C, chunk_classes);
  char* ws = static_cast<char*>(workspace);
  unsigned int* G = reinterpret_cast<unsigned int*>(ws + pl.off_G);
  double* partial = reinterpret_cast<double*>(ws + pl.off_partial);
  float* W = reinterpret_cast<float*>(ws + pl.off_W);
  unsigned int* key[2] = {reinterpret_cast<unsigned int*>(ws + pl.off_key0), reinterpret_cast<unsigned int*>(ws + pl.off_key1)};
  unsigned int* pay[2] = {reinterpret_cast<unsigned int*>(ws + pl.off_pay0), reinterpret_cast<unsigned int*>(ws + pl.off_pay1)};
  unsigned int* hist = reinterpret_cast<unsigned int*>(ws + pl.off_hist);
  unsigned int* dtot = reinterpret_cast<unsigned int*>(ws + pl.off_dtot);
  unsigned int* tcnt = reinterpret_cast<unsigned int*>(ws + pl.off_tcnt);
  const unsigned int nt = (unsigned int)pl.ntiles;
  for (int c0 = 0; c0 < C; c0 += pl.Cc) {
    const int c1 = c0 + pl.Cc < C ? c0 + pl.Cc : C;
    const unsigned int nc = (unsigned int)(c1 - c0);
    TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL(lovasz_key_kernel<TT>, dim3(tss::grid_for(N / 8, NT)), dim3(NT), 0, st, (const TT*)logits, target,
                                             key[0], pay[0], B, C, HW, c0, c1, ignore_index, has_ignore));
    for (int pass = 0; pass < 4; ++pass) {            // 4 passes: the sorted pairs end in buffer 0
      const int src = pass & 1, dst = src ^ 1, shift = 8 * pass;
      hipLaunchKernelGGL(lovasz_hist_kernel, dim3(nt, nc), dim3(NT), 0, st, key[src], hist, N, pl.ntiles, shift);
      hipLaunchKernelGGL(lovasz_digit_total_kernel, dim3(256, nc), dim3(NT), 0, st, hist, dtot, pl.ntiles);
      hipLaunchKernelGGL(lovasz_offset_kernel, dim3(256, nc), dim3(NT), 0, st, hist, dtot, pl.ntiles);
      hipLaunchKernelGGL(lovasz_scatter_kernel, dim3(nt, nc), dim3(NT), 0, st, key[src], pay[src], key[dst], pay[dst], hist, N, pl.ntiles, shift);
    }
    hipLaunchKernelGGL(lovasz_fgcount_kernel, dim3(nt, nc), dim3(NT), 0, st, pay[0], tcnt, N, pl.ntiles);
    hipLaunchKernelGGL(lovasz_tilescan_kernel, dim3(nc), dim3(NT), 0, st, tcnt, G, pl.ntiles, c0);
    hipLaunchKernelGGL(lovasz_weight_kernel, dim3(nt, nc), dim3(NT), 0, st, key[0], pay[0], tcnt, G, W, partial, N, pl.ntiles, c0, variant);
  }
  hipLaunchKernelGGL(lovasz_final_kernel, dim3(1), dim3(NT), 0, st, partial, G, loss, n_present, C, pl.ntiles);
  return tss::check_last("lovasz_fwd");
}

int tss_lovasz_bwd(const void* logits, const long long* target, const void* workspace, const float* n_present,
                   const float* grad_out, void* dlogits, long B, int C, long HW, int chunk_classes, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(shape_ok(B, C, HW) && chunk_classes >= 0 && target && n_present, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(logits) && tss::aligned16(dlogits) && workspace && (reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, TSS_ERR_ALIGN);
  hipStream_t st = (hipStream_t)stream;
  const long N = B * HW;
  const Plan pl = make_plan(N, C, chunk_classes);
  const float* W = reinterpret_cast<const float*>(static_cast<const char*>(workspace) + pl.off_W);
  TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL(lovasz_bwd_kernel<TT>, dim3(tss::grid_for(N / 8, NT)), dim3(NT), 0, st, (const TT*)logits, target, W,
                                           n_present, grad_out, (TT*)dlogits, B, C, HW));
  return tss::check_last("lovasz_bwd");
}

}  // extern "C"
