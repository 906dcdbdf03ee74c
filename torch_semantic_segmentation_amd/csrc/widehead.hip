// The fused head, its losses and the evaluators for more than 24 classes (up to WMAXC = 256).
//
// The kernels of loss.hip / msflip.hip keep ALL class scores of one pixel in registers (aA, aB, gA, gB, z: 5 x CP floats per
// lane, plus the one-hot table Hh[2][256 x CP] in LDS), which is what stops them at 24 classes.  The kernels here keep the
// same geometry -- block = 256 output columns x a band of output rows, lane = one output column, the two horizontally
// interpolated low-res rows in registers, a logit is one FMA -- but only for a CHUNK of WK = 16 classes at a time: a block
// walks its band once per chunk, and what a pixel has to carry from chunk to chunk sits in LDS, one float per (row, lane):
//   wide_ce_kernel              sweep 1: running maximum / sum of exponentials -> the pixel's log-sum-exp (and the loss terms);
//                               sweep 2: p_c = exp2(z_c - lse), the gradient rows gA / gB and the one-hot table of the chunk,
//                               flushed per low-res row into the block's own tile [rows][cells][CPw] at the chunk's offset.
//   wide_upsample_argmax_kernel running (best score, best index), strict > : the lowest index wins across chunks too.
//   wide_multiscale_argmax_kernel  per map the maximum and 1 / sum of every pixel first (two walks: the same roundings as the
//                               register kernel), then per chunk the maps' softmax terms summed in list order.
//   wide_planar_argmax_kernel   argmax_confusion_kernel without the C <= 64 limit of its LDS counters.
// No tensor of B x C x H x W elements exists; the only per-pixel arrays in memory are the f32 `pix` of the OHEM pair.
// Counts: C x C u32 counters in LDS up to WCM_LDS classes, 64-bit integer atomics on the matrix past that (integer adds
// commute: exact and bit-reproducible).  No float atomics.  LDS is dynamic throughout (the CE pass needs 68 KiB).
#include "headgeom.h"

namespace {

constexpr int WK = 16;            // classes per chunk: 5 x 16 floats of class registers per lane
constexpr int WMAXC = 256;
constexpr int WCM_LDS = 96;       // C x C u32 counters in LDS up to here (36 KiB)
constexpr int MSW_ROWS = 2;       // band of the multi-scale kernel: MS_MAXK x MSW_ROWS x 256 x (max, 1/sum) = 64 KiB
constexpr int WIDE_LDS_CAP = 160 * 1024;
constexpr double LN2 = 0.69314718055994530942;

// l0 a + l1 b with ONE spelling of the roundings, fma(l0, a, round(l1 b)).  Left to the compiler's contraction, a + of two products may
// fuse either of them, and not the same one for every class of an unrolled loop: two equal class planes then differ in the last
// bit and the tie between them no longer goes to the lower index.
__device__ __forceinline__ float wide_blend(float l0, float a, float l1, float b) { return __builtin_fmaf(l0, a, l1 * b); }

// a[c] = l0x * L[r][i0x][c0 + c] + l1x * L[r][i1x][c0 + c] for the chunk's classes (times `mul`), 0 past C; 8-channel
// groups that start at or past C are not read (ldl % 8 == 0 and ldl >= C: a group that starts below C ends inside the pitch)
template <typename T>
__device__ __forceinline__ void wide_load_row(const T* p0, const T* p1, const Tap tx, int c0, int C, float mul, float* a) {
#pragma unroll
  for (int c8 = 0; c8 < WK; c8 += 8) {
    float u[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c0 + c8 < C) {                           // uniform
      V8<T>::load(p0 + c0 + c8, u);
      V8<T>::load(p1 + c0 + c8, v);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) a[c8 + q] = (c0 + c8 + q < C) ? wide_blend(tx.l0, u[q], tx.l1, v[q]) * mul : 0.f;   // pad channels hold anything
  }
}

constexpr size_t wide_ce_lds_bytes() {
  return 64 + sizeof(float) * (WROWS * NT + 2 * NT * WK + WTAB + NT + 2 * NT + WMAXC) + sizeof(int) * (2 * NT + 2 * (NT + 2)) +
         sizeof(short) * (WROWS * NT);
}

// MODE as in upsample_ce_onepass_kernel (loss.hip): 0 mean CE, 1 per-pixel CE -> pix, 2 OHEM gradient tiles from pix and sel,
// 3 class weights, 4 class weights + label smoothing.  ws layout as there, tiles [tile_rows][tile_cells][cpw].
// MODE 5: MODE 2 with the weight of a pixel READ from `pix` (0 for a pixel that does not count) instead of derived from a stored
// loss and `sel`: gradient tiles of sum_p pix[p] * CE_p, the second half of the focal loss past 24 classes (softhead.hip).
template <typename T, int MODE>
__global__ __launch_bounds__(NT, 2) void wide_ce_kernel(const T* low, long ldl, const long long* target, float* tiles, double* lossrows,
                                                        int C, int h, int w, int H, int W, int ignore_index, const HeadGeom geo,
                                                        float* pix, const float* sel, const float* cw, float eps) {
  constexpr bool WEIGHTED = MODE == 3 || MODE == 4;             // class weights in play
  constexpr bool TILES_ONLY = MODE == 2 || MODE == 5;           // no loss terms, no loss rows
  // all of this kernel's LDS is dynamic: wide_allow_lds asks for the whole 160 KiB as dynamic LDS, and the request is refused (the
  // launch then fails) once the kernel also holds static LDS, as a call of lsw::block_sum2 would give it
  extern __shared__ __align__(16) unsigned char wlds[];
  double* const red = reinterpret_cast<double*>(wlds);          // [2][NT / 64]
  float* const Pm = reinterpret_cast<float*>(wlds + 64);        // [WROWS][NT] running maximum, then the log-sum-exp (log2 units)
  float* const Hh = Pm + WROWS * NT;                            // [2][NT * WK] one-hot half of the chunk's gradient (sweep 2)
  float* const Ps = Hh;                                         // [WROWS][NT] running sum (sweep 1 only: shares Hh's space)
  float* const Pz = Hh + NT * WK;                               // [WROWS][NT] MODE 1: the target's logit
  float* const Wt = Hh + 2 * NT * WK;                           // [WTAB] gather weights [cell][lane - Wlo[cell]]
  float* const Ll1 = Wt + WTAB;                                 // [NT]
  float* const Nn = Ll1 + NT;                                   // [2][NT] MODE 4: row-weight sums of the valid pixels per row buffer
  float* const Cw = Nn + 2 * NT;                                // [WMAXC] class weights, 0 past C
  int* const Li0 = reinterpret_cast<int*>(Cw + WMAXC);          // [NT]
  int* const Li1 = Li0 + NT;                                    // [NT]
  int* const Wlo = Li1 + NT;                                    // [NT + 2]
  int* const Whi = Wlo + NT + 2;                                // [NT + 2]
  short* const Tt = reinterpret_cast<short*>(Whi + NT + 2);     // [WROWS][NT] the class of a pixel that counts, else -1
  static_assert(WMAXC == NT && WROWS * NT <= NT * WK, "LDS layout");

  const int tid = threadIdx.x;
  const int cpw = geo.cp;
  Cw[tid] = (WEIGHTED && tid < C) ? (cw ? cw[tid] : 1.f) : 0.f;
  Nn[tid] = 0.f; Nn[NT + tid] = 0.f;
  const int nstrip = geo.nstrip, nband = geo.nband;
  float* const tile = tiles + (long)blockIdx.x * geo.tile_rows * geo.tile_cells * cpw;
  int bid = blockIdx.x;
  const int strip = bid % nstrip; bid /= nstrip;
  const int band = bid % nband;
  const long b = bid / nband;
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  const int x = strip * NT + tid;
  const bool xin = x < W;
  const Tap tx = ac_tap(sx, xin ? x : W - 1, w);
  const int cx0 = ac_tap(sx, strip * NT, w).i0;
  const int xl = (strip * NT + NT - 1 < W) ? strip * NT + NT - 1 : W - 1;
  const int ncell = ac_tap(sx, xl, w).i1 - cx0 + 1;                 // <= NT + 2 for W >= w (host-checked)
  const int ya = band * WROWS;
  const int yb = ya + WROWS < H ? ya + WROWS : H;
  Li0[tid] = xin ? tx.i0 - cx0 : -1;
  Li1[tid] = xin ? tx.i1 - cx0 : -1;
  Ll1[tid] = tx.l1;
  const int maxwin = sx > 0.f ? (int)(2.f / sx) + 6 : NT;
  const bool wtab = (long)ncell * maxwin <= WTAB;
  for (int cell = tid; cell < ncell; cell += NT) {
    int lo, hi;
    ac_window(sx, cx0 + cell, W, &lo, &hi);
    lo -= strip * NT; hi -= strip * NT;
    lo = lo < 0 ? 0 : lo;
    hi = hi > NT - 1 ? NT - 1 : hi;
    if (wtab && hi - lo + 1 > maxwin) hi = lo + maxwin - 1;
    Wlo[cell] = lo;
    Whi[cell] = hi;
  }
  for (int j = 0; j < WROWS; ++j) {               // the band's labels, once: every sweep and chunk reads them from LDS
    const int y = ya + j;
    short tv = -1;
    if (xin && y < yb) {
      const long long t = target[(b * H + y) * (long)W + x];
      if (t != ignore_index && t >= 0 && t < C) tv = (short)t;
    }
    Tt[j * NT + tid] = tv;
    Pm[j * NT + tid] = -TSS_INF;
    Ps[j * NT + tid] = 0.f;
    if (MODE == 1) Pz[j * NT + tid] = 0.f;
  }
  __syncthreads();
  if (wtab) {
    for (int i = tid; i < ncell * maxwin; i += NT) {
      const int cell = i / maxwin, k = i - cell * maxwin;
      const int l = Wlo[cell] + k;
      float wgt = 0.f;
      if (l <= Whi[cell]) { const float l1 = Ll1[l]; wgt = (Li0[l] == cell ? 1.f - l1 : 0.f) + (Li1[l] == cell ? l1 : 0.f); }
      Wt[i] = wgt;
    }
  }
  const float om = MODE == 4 ? 1.f - eps : 1.f;                 // weight of the one-hot part of the target distribution
  const float eC = MODE == 4 ? eps / (float)C : 0.f;
  float sW = 0.f;                                               // eps W / C
  if (MODE == 4) {
    float ws = 0.f;
    for (int c = 0; c < C; ++c) ws += Cw[c];
    sW = eC * ws;
  }

  const int r_first = ac_tap(sy, ya, h).i0;
  const T* const img = low + b * h * (long)w * ldl;
  auto load_row = [&](int r, int c0, float* a) {
    wide_load_row<T>(img + ((long)r * w + tx.i0) * ldl, img + ((long)r * w + tx.i1) * ldl, tx, c0, C, LOG2E, a);
  };

  // ---- sweep 1: the log-sum-exp of every pixel of the band, and the loss terms (all in log2 units)
  double lsum = 0.0;
  float lcnt = 0.f;
  for (int c0 = 0; c0 < C; c0 += WK) {
    int rA = r_first;
    int rB = rA + (rA < h - 1 ? 1 : 0);
    float aA[WK], aB[WK];
    load_row(rA, c0, aA);
    load_row(rB, c0, aB);
    for (int y = ya; y < yb; ++y) {
      const int j = y - ya;
      const Tap ty = ac_tap(sy, y, h);
      while (rA < ty.i0) {                         // uniform; at most one turn in exact arithmetic (H >= h)
        rA = rB;
        rB = rA + (rA < h - 1 ? 1 : 0);
#pragma unroll
        for (int c = 0; c < WK; ++c) aA[c] = aB[c];
        load_row(rB, c0, aB);
      }
      float z[WK];
      float mc = -TSS_INF;
#pragma unroll
      for (int c = 0; c < WK; ++c) {
        z[c] = wide_blend(ty.l0, aA[c], ty.l1, aB[c]);
        if (c0 + c < C) mc = fmaxf(mc, z[c]);
      }
      const float mo = Pm[j * NT + tid];
      const float mn = fmaxf(mo, mc);              // finite: the chunk holds at least one class
      float s = Ps[j * NT + tid] * __builtin_amdgcn_exp2f(mo - mn);     // first chunk: 0 * exp2(-inf) = 0
#pragma unroll
      for (int c = 0; c < WK; ++c) s += (c0 + c < C) ? __builtin_amdgcn_exp2f(z[c] - mn) : 0.f;
      Pm[j * NT + tid] = mn;
      Ps[j * NT + tid] = s;
      if (!TILES_ONLY) {
        const int t = Tt[j * NT + tid];
        const int tc = t - c0;
        if (tc >= 0 && tc < WK) {                  // the one chunk that holds the pixel's class: its logit, by compare
          float zt = 0.f;
#pragma unroll
          for (int c = 0; c < WK; ++c) zt = (tc == c) ? z[c] : zt;
          if (MODE == 1) Pz[j * NT + tid] = zt;
          else lsum -= (double)((WEIGHTED ? om * Cw[t] : 1.f) * zt);
        }
        if (MODE == 4 && t >= 0) {                 // the uniform part of the smoothed target: eps / C * sum_c w_c z_c
          float zs = 0.f;
#pragma unroll
          for (int c = 0; c < WK; ++c) zs += Cw[c0 + c] * z[c];       // past C: weight 0, logit 0
          lsum -= (double)(eC * zs);
        }
      }
    }
  }
  for (int y = ya; y < yb; ++y) {
    const int j = y - ya;
    const float lse = Pm[j * NT + tid] + __builtin_amdgcn_logf(Ps[j * NT + tid]);     // log2
    Pm[j * NT + tid] = lse;
    const int t = Tt[j * NT + tid];
    if (MODE == 1) {      // per-pixel loss in nats, >= 0 (rounding may give -1e-7), 0 for ignored pixels
      if (xin) pix[(b * H + y) * (long)W + x] = t >= 0 ? fmaxf((lse - Pz[j * NT + tid]) * (float)LN2, 0.f) : 0.f;
    } else if (!TILES_ONLY && t >= 0) {
      const float wt = WEIGHTED ? Cw[t] : 1.f;
      lsum += (double)((om * wt + sW) * lse);
      lcnt += wt;
    }
  }
  if (MODE == 1) return;

  // ---- sweep 2: the gradient, chunk by chunk
  __syncthreads();                                 // every lane is done with Ps: its space becomes Hh
#pragma unroll
  for (int c4 = 0; c4 < WK; c4 += 4) {
    *reinterpret_cast<float4*>(&Hh[tid * WK + c4]) = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(&Hh[NT * WK + tid * WK + c4]) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float sel_cut = 0.f, sel_gt = 0.f, sel_eq = 0.f;
  if (MODE == 2) { sel_cut = sel[1]; sel_gt = sel[2]; sel_eq = sel[0] != 0.f ? 0.f : sel[3]; }

  for (int c0 = 0; c0 < C; c0 += WK) {
    // finished low-res row r (buffer k) of this chunk: the lane's g[] - Hh[k][] is parked in Hh[k], one thread per (cell, class)
    // gathers the lanes whose column taps include that cell, plain stores into the block's tile at classes c0 .. c0 + WK - 1
    auto flush_row = [&](int r, int k, const float* g) {
      float* G = Hh + k * NT * WK;
      float nk = 0.f;
      if (MODE == 4) { nk = Nn[k * NT + tid] * eC; Nn[k * NT + tid] = 0.f; }
#pragma unroll
      for (int c4 = 0; c4 < WK; c4 += 4) {
        const float4 hv = *reinterpret_cast<const float4*>(G + tid * WK + c4);
        float hq[4] = {hv.x, hv.y, hv.z, hv.w};
        if (MODE == 4) {
#pragma unroll
          for (int q = 0; q < 4; ++q) hq[q] += nk * Cw[c0 + c4 + q];
        }
        *reinterpret_cast<float4*>(G + tid * WK + c4) = make_float4(g[c4] - hq[0], g[c4 + 1] - hq[1], g[c4 + 2] - hq[2], g[c4 + 3] - hq[3]);
      }
      __syncthreads();
      const int tr = r - r_first;
      if (tr >= 0 && tr < geo.tile_rows) {         // always (the host's tile extent is conservative); keeps the stores inside the tile
        float* drow = tile + (long)tr * geo.tile_cells * cpw;
        for (int i = tid; i < ncell * WK; i += NT) {
          const int cell = i / WK, c = i - cell * WK;
          if (cell >= geo.tile_cells || c0 + c >= cpw) continue;
          const int llo = Wlo[cell], lhi = Whi[cell];
          float sum = 0.f;
          if (wtab) {
            const float* wt = Wt + cell * maxwin - llo;
            for (int l = llo; l <= lhi; ++l) sum += wt[l] * G[l * WK + c];
          } else {
            for (int l = llo; l <= lhi; ++l) {
              const float l1 = Ll1[l];
              const float wgt = (Li0[l] == cell ? 1.f - l1 : 0.f) + (Li1[l] == cell ? l1 : 0.f);
              sum += wgt * G[l * WK + c];
            }
          }
          drow[cell * cpw + c0 + c] = sum;         // [cell][class]: every element of the footprint, once per chunk
        }
      }
      __syncthreads();
#pragma unroll
      for (int c4 = 0; c4 < WK; c4 += 4) *reinterpret_cast<float4*>(G + tid * WK + c4) = make_float4(0.f, 0.f, 0.f, 0.f);
    };

    int rA = r_first;
    int rB = rA + (rA < h - 1 ? 1 : 0);
    int kA = 0;
    float aA[WK], aB[WK], gA[WK], gB[WK];
    load_row(rA, c0, aA);
    load_row(rB, c0, aB);
#pragma unroll
    for (int c = 0; c < WK; ++c) { gA[c] = 0.f; gB[c] = 0.f; }
    for (int y = ya; y < yb; ++y) {
      const int j = y - ya;
      const Tap ty = ac_tap(sy, y, h);
      while (rA < ty.i0) {                         // uniform
        flush_row(rA, kA, gA);
        kA ^= 1;
        rA = rB;
        rB = rA + (rA < h - 1 ? 1 : 0);
#pragma unroll
        for (int c = 0; c < WK; ++c) { aA[c] = aB[c]; gA[c] = gB[c]; gB[c] = 0.f; }
        load_row(rB, c0, aB);
      }
      const int t = Tt[j * NT + tid];
      const bool valid = t >= 0;
      float wpx = 1.f, wsm = 1.f;                  // weights of the one-hot and of the softmax half
      if (TILES_ONLY) {
        const float pl = xin ? pix[(b * H + y) * (long)W + x] : 0.f;
        wpx = MODE == 5 ? pl : (pl > sel_cut ? sel_gt : (pl == sel_cut ? sel_eq : 0.f));
        wsm = wpx;
      }
      if (valid) {
        if (WEIGHTED) { wpx = om * Cw[t]; wsm = wpx + sW; }
        if (MODE == 4) { Nn[kA * NT + tid] += ty.l0; Nn[(kA ^ 1) * NT + tid] += ty.l1; }
        const int tc = t - c0;
        if (tc >= 0 && tc < WK) {                  // this lane's own rows of the table: no race
          Hh[kA * NT * WK + tid * WK + tc] += ty.l0 * wpx;
          Hh[(kA ^ 1) * NT * WK + tid * WK + tc] += ty.l1 * wpx;
        }
      }
      const float inv = valid ? wsm : 0.f;
      const float lse = Pm[j * NT + tid];
#pragma unroll
      for (int c = 0; c < WK; ++c) {
        const float zc = wide_blend(ty.l0, aA[c], ty.l1, aB[c]);
        const float pz = (c0 + c < C) ? __builtin_amdgcn_exp2f(zc - lse) * inv : 0.f;
        gA[c] += ty.l0 * pz;
        gB[c] += ty.l1 * pz;
      }
    }
    flush_row(rA, kA, gA);
    if (rB != rA) flush_row(rB, kA ^ 1, gB);
    else {        // the band ended on the last low-res row: the l1 weights are zero there, nothing to flush; the next chunk starts clean
#pragma unroll
      for (int c4 = 0; c4 < WK; c4 += 4) *reinterpret_cast<float4*>(&Hh[(kA ^ 1) * NT * WK + tid * WK + c4]) = make_float4(0.f, 0.f, 0.f, 0.f);
      Nn[(kA ^ 1) * NT + tid] = 0.f;
    }
  }
  if (TILES_ONLY) return;

  double ds = wave_sum(lsum * LN2), dc = wave_sum((double)lcnt);   // back to nats
  const int wave = tid >> 6;
  if ((tid & 63) == 0) { red[wave] = ds; red[NT / 64 + wave] = dc; }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, c = 0.0;
    for (int wv = 0; wv < NT / 64; ++wv) { a += red[wv]; c += red[NT / 64 + wv]; }
    lossrows[2 * (long)blockIdx.x] = a;
    lossrows[2 * (long)blockIdx.x + 1] = c;
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void wide_ce_gather_kernel(const float* tiles, const float* inv_count, const float* grad_out,
                                                            T* dlow, long ldl, int B, int h, int w, int H, int W, const HeadGeom geo) {
  head_gather<T, 0>(tiles, inv_count, grad_out, dlow, ldl, B, h, w, H, W, geo);
}

// one count of (truth t, prediction arg): LDS counter, or a 64-bit integer atomic on the matrix itself
template <bool LDSCM>
__device__ __forceinline__ void wide_count(unsigned int* scm, unsigned long long* cm, int C, int t, int arg) {
  if (LDSCM) atomicAdd(&scm[t * C + arg], 1u);
  else atomicAdd(cm + (long)t * C + arg, 1ull);
}
template <bool LDSCM>
__device__ __forceinline__ void wide_counts_out(const unsigned int* scm, unsigned long long* cm, int C) {
  if (!LDSCM) return;
  __syncthreads();
  for (int i = threadIdx.x; i < C * C; i += NT)
    if (scm[i]) atomicAdd(cm + i, (unsigned long long)scm[i]);
}

constexpr size_t wide_argmax_lds_bytes(int C, bool ldscm) {
  return sizeof(float) * WROWS * NT + (ldscm ? sizeof(unsigned int) * C * C : 0) + WROWS * NT;
}

// upsample_argmax_kernel (loss.hip) by chunks: the running (best score, best index) of a pixel in LDS, strict > across chunks
template <typename T, bool LDSCM>
__global__ __launch_bounds__(NT, 2) void wide_upsample_argmax_kernel(const T* low, long ldl, const long long* target,
                                                                     unsigned char* pred_out, unsigned long long* cm, int C,
                                                                     int h, int w, int H, int W, int ignore_index) {
  extern __shared__ __align__(16) unsigned char wlds[];
  float* const Bs = reinterpret_cast<float*>(wlds);                        // [WROWS][NT]
  unsigned int* const scm = reinterpret_cast<unsigned int*>(Bs + WROWS * NT);   // [C * C] (LDSCM)
  unsigned char* const Bi = reinterpret_cast<unsigned char*>(scm + (LDSCM ? C * C : 0));   // [WROWS][NT]
  const int tid = threadIdx.x;
  const bool counts = cm && target;
  if (LDSCM) {
    for (int i = tid; i < C * C; i += NT) scm[i] = 0u;
    __syncthreads();
  }
  const HeadBlock blk = head_block((W + NT - 1) / NT, (H + WROWS - 1) / WROWS, WROWS, H, W);
  const HeadTaps map = head_taps(blk, h, w, H, W);
  const long b = blk.b;
  const int x = blk.x, ya = blk.ya, yb = blk.yb;
  const bool xin = blk.xin;
  const float sy = map.sy;
  const Tap tx = map.tx;
  const T* const img = low + b * h * (long)w * ldl;
  auto load_row = [&](int r, int c0, float* a) {
    wide_load_row<T>(img + ((long)r * w + tx.i0) * ldl, img + ((long)r * w + tx.i1) * ldl, tx, c0, C, 1.f, a);
  };
  const int r_first = ac_tap(sy, ya, h).i0;
  for (int c0 = 0; c0 < C; c0 += WK) {
    int rA = r_first;
    int rB = rA + (rA < h - 1 ? 1 : 0);
    float aA[WK], aB[WK];
    load_row(rA, c0, aA);
    load_row(rB, c0, aB);
    for (int y = ya; y < yb; ++y) {
      const int j = y - ya;
      const Tap ty = ac_tap(sy, y, h);
      while (rA < ty.i0) {
        rA = rB;
        rB = rA + (rA < h - 1 ? 1 : 0);
#pragma unroll
        for (int c = 0; c < WK; ++c) aA[c] = aB[c];
        load_row(rB, c0, aB);
      }
      float best = c0 ? Bs[j * NT + tid] : -TSS_INF;
      int arg = c0 ? (int)Bi[j * NT + tid] : 0;
#pragma unroll
      for (int c = 0; c < WK; ++c) {
        const float z = wide_blend(ty.l0, aA[c], ty.l1, aB[c]);
        if (c0 + c < C && (z > best || c0 + c == 0)) { best = z; arg = c0 + c; }
      }
      Bs[j * NT + tid] = best;
      Bi[j * NT + tid] = (unsigned char)arg;
    }
  }
  if (xin) {
    for (int y = ya; y < yb; ++y) {
      const int arg = Bi[(y - ya) * NT + tid];
      const long p = (b * H + y) * (long)W + x;
      if (pred_out) pred_out[p] = (unsigned char)arg;
      if (counts) {
        const long long t = target[p];
        if (t != ignore_index && t >= 0 && t < C) wide_count<LDSCM>(scm, cm, C, (int)t, arg);
      }
    }
  }
  if (counts) wide_counts_out<LDSCM>(scm, cm, C);
}

// the logits of the chunk c0 of one map at the MSW_ROWS rows of a band: f(j, z) per row y = ya + j < H, z[c] past C is 0
template <typename T, typename F>
__device__ __forceinline__ void ms_walk(const MsMap mp, const HeadBlock& blk, int H, int W, int C, int c0, F&& f) {
  const int h = mp.h, w = mp.w;
  const long ldl = mp.ldl;
  const HeadTaps map = head_taps(blk, h, w, H, W, mp.flip);
  const float sy = map.sy;
  const Tap tx = map.tx;
  const int ya = blk.ya;
  const T* const img = reinterpret_cast<const T*>(mp.low) + (mp.first + blk.b) * h * (long)w * ldl;
  float aA[WK], aB[WK];
  int rA = ac_tap(sy, ya, h).i0;
  int rB = rA + (rA < h - 1 ? 1 : 0);
  wide_load_row<T>(img + ((long)rA * w + tx.i0) * ldl, img + ((long)rA * w + tx.i1) * ldl, tx, c0, C, 1.f, aA);
  wide_load_row<T>(img + ((long)rB * w + tx.i0) * ldl, img + ((long)rB * w + tx.i1) * ldl, tx, c0, C, 1.f, aB);
#pragma unroll
  for (int j = 0; j < MSW_ROWS; ++j) {
    const int y = ya + j;
    if (y < H) {                                 // uniform
      const Tap ty = ac_tap(sy, y, h);
      while (rA < ty.i0) {                       // uniform (msflip.hip: a loop, so that a product that rounds across a row boundary still ends on the tap's rows)
        rA = rB;
        rB = rA + (rA < h - 1 ? 1 : 0);
#pragma unroll
        for (int c = 0; c < WK; ++c) aA[c] = aB[c];
        wide_load_row<T>(img + ((long)rB * w + tx.i0) * ldl, img + ((long)rB * w + tx.i1) * ldl, tx, c0, C, 1.f, aB);
      }
      float z[WK];
#pragma unroll
      for (int c = 0; c < WK; ++c) z[c] = wide_blend(ty.l0, aA[c], ty.l1, aB[c]);
      f(j, z);
    }
  }
}

constexpr size_t wide_ms_lds_bytes(int C, int mode, bool ldscm) {
  return (mode == 0 ? sizeof(float) * 2 * MS_MAXK * MSW_ROWS * NT : 0) + (ldscm ? sizeof(unsigned int) * C * C : 0);
}

// multiscale_argmax_kernel (msflip.hip) by chunks.  MODE 0: per map, the maximum over all classes (one walk), then the sum of
// exp(z - max) in class order (a second walk) -- exactly the roundings of the register kernel -- kept as (max, 1 / sum) per map,
// row and lane in LDS; then per chunk score[c] = sum over the maps, in list order, of exp(z - max) * (1 / sum), and the running
// arg-max.  MODE 1: the last step only, on the raw logits.
template <typename T, int MODE, bool LDSCM>
__global__ __launch_bounds__(NT, 2) void wide_multiscale_argmax_kernel(const MsArgs args, int K, const long long* target,
                                                                       unsigned char* pred_out, unsigned long long* cm, int C,
                                                                       int H, int W, int ignore_index) {
  extern __shared__ __align__(16) unsigned char wlds[];
  float* const Mm = reinterpret_cast<float*>(wlds);                        // [K][MSW_ROWS][NT] (MODE 0)
  float* const Mi = Mm + (MODE == 0 ? MS_MAXK * MSW_ROWS * NT : 0);        // [K][MSW_ROWS][NT] (MODE 0)
  unsigned int* const scm = reinterpret_cast<unsigned int*>(Mi + (MODE == 0 ? MS_MAXK * MSW_ROWS * NT : 0));
  const int tid = threadIdx.x;
  const bool counts = cm && target;
  if (LDSCM) {
    for (int i = tid; i < C * C; i += NT) scm[i] = 0u;
    __syncthreads();
  }
  const HeadBlock blk = head_block((W + NT - 1) / NT, (H + MSW_ROWS - 1) / MSW_ROWS, MSW_ROWS, H, W);
  const long b = blk.b;
  const int x = blk.x, ya = blk.ya;
  const bool xin = blk.xin;

  if (MODE == 0) {
    for (int k = 0; k < K; ++k) {
      const MsMap mp = args.m[k];
      float m[MSW_ROWS], s[MSW_ROWS];
#pragma unroll
      for (int j = 0; j < MSW_ROWS; ++j) { m[j] = -TSS_INF; s[j] = 0.f; }
      for (int c0 = 0; c0 < C; c0 += WK)
        ms_walk<T>(mp, blk, H, W, C, c0, [&](int j, const float* z) {
#pragma unroll
          for (int c = 0; c < WK; ++c) m[j] = (c0 + c < C) ? fmaxf(m[j], z[c]) : m[j];
        });
      for (int c0 = 0; c0 < C; c0 += WK)
        ms_walk<T>(mp, blk, H, W, C, c0, [&](int j, const float* z) {
#pragma unroll
          for (int c = 0; c < WK; ++c) s[j] += (c0 + c < C) ? __expf(z[c] - m[j]) : 0.f;
        });
#pragma unroll
      for (int j = 0; j < MSW_ROWS; ++j) {
        Mm[(k * MSW_ROWS + j) * NT + tid] = m[j];
        Mi[(k * MSW_ROWS + j) * NT + tid] = 1.f / s[j];       // s >= 1: the largest term is exp(0)
      }
    }
  }

  float best[MSW_ROWS];
  int arg[MSW_ROWS];
#pragma unroll
  for (int j = 0; j < MSW_ROWS; ++j) { best[j] = 0.f; arg[j] = 0; }
  for (int c0 = 0; c0 < C; c0 += WK) {
    float score[MSW_ROWS][WK];
#pragma unroll
    for (int j = 0; j < MSW_ROWS; ++j)
#pragma unroll
      for (int c = 0; c < WK; ++c) score[j][c] = 0.f;
    for (int k = 0; k < K; ++k) {
      ms_walk<T>(args.m[k], blk, H, W, C, c0, [&](int j, const float* z) {
        if (MODE == 1) {
#pragma unroll
          for (int c = 0; c < WK; ++c) score[j][c] += z[c];
        } else {
          const float m = Mm[(k * MSW_ROWS + j) * NT + tid], inv = Mi[(k * MSW_ROWS + j) * NT + tid];
#pragma unroll
          for (int c = 0; c < WK; ++c) score[j][c] += (c0 + c < C) ? __expf(z[c] - m) * inv : 0.f;
        }
      });
    }
#pragma unroll
    for (int j = 0; j < MSW_ROWS; ++j)
#pragma unroll
      for (int c = 0; c < WK; ++c) {
        if (c0 + c == 0) { best[j] = score[j][0]; arg[j] = 0; }
        else if (c0 + c < C && score[j][c] > best[j]) { best[j] = score[j][c]; arg[j] = c0 + c; }      // strict: the lowest index wins ties
      }
  }
#pragma unroll
  for (int j = 0; j < MSW_ROWS; ++j) {
    const int y = ya + j;
    if (y < H && xin) {
      const long p = (b * H + y) * (long)W + x;
      if (pred_out) pred_out[p] = (unsigned char)arg[j];
      if (counts) {
        const long long t = target[p];
        if (t != ignore_index && t >= 0 && t < C) wide_count<LDSCM>(scm, cm, C, (int)t, arg[j]);
      }
    }
  }
  if (counts) wide_counts_out<LDSCM>(scm, cm, C);
}

// argmax_confusion_kernel (loss.hip) for any C <= 256: argmax over class planes, lowest index wins ties
template <typename T, bool LDSCM>
__global__ __launch_bounds__(NT) void wide_planar_argmax_kernel(const T* logits, const long long* target, unsigned char* pred_out,
                                                                unsigned long long* cm, long B, int C, long HW, int ignore_index) {
  extern __shared__ __align__(16) unsigned char wlds[];
  unsigned int* const scm = reinterpret_cast<unsigned int*>(wlds);        // [C * C] (LDSCM)
  if (LDSCM) {
    for (int i = threadIdx.x; i < C * C; i += NT) scm[i] = 0u;
    __syncthreads();
  }
  const bool counts = cm && target;
  for (lsw::Groups g(B, HW); g.more(); g.next()) {
    const long b = g.b(), off = g.off();
    float best[8];
    int arg[8], tv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { best[j] = -INFINITY; arg[j] = 0; }
    for (int c = 0; c < C; ++c) {
      float v[8];
      V8<T>::load(logits + (b * C + c) * HW + off, v);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (v[j] > best[j] || (c == 0)) { best[j] = v[j]; arg[j] = c; }
    }
    if (counts) lsw::load_labels(target + b * HW + off, C, ignore_index, 1, tv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (pred_out) pred_out[b * HW + off + j] = (unsigned char)arg[j];
      if (counts && tv[j] >= 0) wide_count<LDSCM>(scm, cm, C, tv[j], arg[j]);
    }
  }
  if (counts) wide_counts_out<LDSCM>(scm, cm, C);
}

// the kernels ask for more dynamic LDS than the default limit: raised once per instance and device
template <typename KernelT>
void wide_allow_lds(KernelT kernel, tss::DevOnce& once) {
  if (once.first()) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, WIDE_LDS_CAP);
}

template <typename T, int MODE>
void launch_wide_ce(long grid, hipStream_t stream, const void* low, long ldl, const long long* target, float* tiles, double* lossrows,
                    int C, int h, int w, int H, int W, int ignore_index, const HeadGeom& geo, float* pix, const float* sel,
                    const float* cw, float eps) {
  static tss::DevOnce attr;
  wide_allow_lds(wide_ce_kernel<T, MODE>, attr);
  hipLaunchKernelGGL((wide_ce_kernel<T, MODE>), dim3((int)grid), dim3(NT), wide_ce_lds_bytes(), stream, (const T*)low, ldl, target, tiles,
                     lossrows, C, h, w, H, W, ignore_index, geo, pix, sel, cw, eps);
}

template <typename T, int MODE, bool LDSCM>
void launch_wide_ms(long grid, hipStream_t stream, const MsArgs& args, int K, const long long* target, unsigned char* pred,
                    unsigned long long* cm, int C, int H, int W, int ignore_index) {
  static tss::DevOnce attr;
  wide_allow_lds(wide_multiscale_argmax_kernel<T, MODE, LDSCM>, attr);
  hipLaunchKernelGGL((wide_multiscale_argmax_kernel<T, MODE, LDSCM>), dim3((int)grid), dim3(NT), wide_ms_lds_bytes(C, MODE, LDSCM), stream,
                     args, K, target, pred, cm, C, H, W, ignore_index);
}

}  // namespace

extern "C" {

int tss_widehead_max_classes(void) { return WMAXC; }

long tss_upsample_ce_wide_ws(int B, int C, int h, int w, int H, int W) { return head_ws_floats(B, C, WMAXC, h, w, H, W, true); }

int tss_upsample_ce_wide_fwd(const void* low, long ldl, const long long* target, const float* weight, float label_smoothing, float* ws,
                             float* loss, float* inv_count, int B, int C, int h, int w, int H, int W, int ignore_index, int dtype,
                             void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, WMAXC, ldl, h, w, H, W) && label_smoothing >= 0.f && label_smoothing <= 1.f && B >= 0, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low) && tss::aligned16(ws), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, true);
  const long grid = head_blocks(B, geo);
  TSS_REQUIRE(grid <= 0x7fffffffL, TSS_ERR_SHAPE);
  double* lossrows = reinterpret_cast<double*>(ws);
  float* tiles = ws + grid * 4;
  const hipStream_t st = (hipStream_t)stream;
  const bool plain = !weight && label_smoothing == 0.f;
  {
    tss::ProfScope prof(TSS_K_WIDE_CE_FWD, st, (double)B * h * w * C * (tss::esz(dtype) + 8.0) + (double)B * H * W * 8.0, 0);
    if (plain)
      TSS_WITH_DTYPE(dtype, (launch_wide_ce<TT, 0>(grid, st, low, ldl, target, tiles, lossrows, C, h, w, H, W, ignore_index, geo, nullptr,
                                                   nullptr, nullptr, 0.f)));
    else if (label_smoothing > 0.f)
      TSS_WITH_DTYPE(dtype, (launch_wide_ce<TT, 4>(grid, st, low, ldl, target, tiles, lossrows, C, h, w, H, W, ignore_index, geo, nullptr,
                                                   nullptr, weight, label_smoothing)));
    else
      TSS_WITH_DTYPE(dtype, (launch_wide_ce<TT, 3>(grid, st, low, ldl, target, tiles, lossrows, C, h, w, H, W, ignore_index, geo, nullptr,
                                                   nullptr, weight, 0.f)));
  }
  if (plain) hipLaunchKernelGGL(ce_finalize_rows_kernel<false>, dim3(1), dim3(NT), 0, st, lossrows, (int)grid, loss, inv_count);
  else hipLaunchKernelGGL(ce_finalize_rows_kernel<true>, dim3(1), dim3(NT), 0, st, lossrows, (int)grid, loss, inv_count);
  return tss::check_last("upsample_ce_wide_fwd");
}

int tss_upsample_pixel_ce_wide(const void* low, long ldl, const long long* target, float* pix, int B, int C, int h, int w, int H, int W,
                               int ignore_index, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, WMAXC, ldl, h, w, H, W) && pix && B >= 0, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, true);
  const long grid = head_blocks(B, geo);
  TSS_REQUIRE(grid <= 0x7fffffffL, TSS_ERR_SHAPE);
  tss::ProfScope prof(TSS_K_WIDE_CE_FWD, (hipStream_t)stream, (double)B * h * w * C * tss::esz(dtype) + (double)B * H * W * 12.0, 0);
  TSS_WITH_DTYPE(dtype, (launch_wide_ce<TT, 1>(grid, (hipStream_t)stream, low, ldl, target, nullptr, nullptr, C, h, w, H, W, ignore_index, geo,
                                               pix, nullptr, nullptr, 0.f)));
  return tss::check_last("upsample_pixel_ce_wide");
}

int tss_upsample_ohem_grad_wide(const void* low, long ldl, const long long* target, const float* pix, const float* sel, float* ws,
                                int B, int C, int h, int w, int H, int W, int ignore_index, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, WMAXC, ldl, h, w, H, W) && pix && sel && ws && B >= 0, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low) && tss::aligned16(ws), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, true);
  const long grid = head_blocks(B, geo);
  TSS_REQUIRE(grid <= 0x7fffffffL, TSS_ERR_SHAPE);
  float* tiles = ws + grid * 4;
  tss::ProfScope prof(TSS_K_WIDE_CE_FWD, (hipStream_t)stream, (double)B * h * w * C * (tss::esz(dtype) + 8.0) + (double)B * H * W * 12.0, 0);
  TSS_WITH_DTYPE(dtype, (launch_wide_ce<TT, 2>(grid, (hipStream_t)stream, low, ldl, target, tiles, nullptr, C, h, w, H, W, ignore_index, geo,
                                               const_cast<float*>(pix), sel, nullptr, 0.f)));
  return tss::check_last("upsample_ohem_grad_wide");
}

// Gradient tiles of sum_p coef[p] * CE_p, coef ([B][H][W] f32) 0 for every pixel that does not count (tss_focal_coef_from_ce writes it
// that way): the MODE 5 instance.  ws as for tss_upsample_ce_wide_fwd; tss_upsample_ce_wide_bwd gathers.
int tss_upsample_coef_grad_wide(const void* low, long ldl, const long long* target, const float* coef, float* ws, int B, int C, int h,
                                int w, int H, int W, int ignore_index, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, WMAXC, ldl, h, w, H, W) && coef && ws && B >= 0, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low) && tss::aligned16(ws), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, true);
  const long grid = head_blocks(B, geo);
  TSS_REQUIRE(grid <= 0x7fffffffL, TSS_ERR_SHAPE);
  float* tiles = ws + grid * 4;
  tss::ProfScope prof(TSS_K_WIDE_CE_FWD, (hipStream_t)stream, (double)B * h * w * C * (tss::esz(dtype) + 8.0) + (double)B * H * W * 12.0, 0);
  TSS_WITH_DTYPE(dtype, (launch_wide_ce<TT, 5>(grid, (hipStream_t)stream, low, ldl, target, tiles, nullptr, C, h, w, H, W, ignore_index, geo,
                                               const_cast<float*>(coef), nullptr, nullptr, 0.f)));
  return tss::check_last("upsample_coef_grad_wide");
}

int tss_upsample_ce_wide_bwd(const float* ws, const float* inv_count, const float* grad_out, void* dlow, long ldl,
                             int B, int C, int h, int w, int H, int W, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, WMAXC, ldl, h, w, H, W) && B >= 0, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(ws) && tss::aligned16(dlow), TSS_ERR_ALIGN);
  const long n = (long)B * h * w * ldl;
  if (n == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, true);
  const float* tiles = ws + head_blocks(B, geo) * 4;
  tss::ProfScope prof(TSS_K_WIDE_CE_BWD, (hipStream_t)stream, (double)n * (4.0 + tss::esz(dtype)), 0);
  TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL(wide_ce_gather_kernel<TT>, dim3(tss::grid_for(n / 8, NT)), dim3(NT), 0, (hipStream_t)stream,
                                           tiles, inv_count, grad_out, (TT*)dlow, ldl, B, h, w, H, W, geo));
  return tss::check_last("upsample_ce_wide_bwd");
}

int tss_upsample_argmax_confusion_wide(const void* low, long ldl, const long long* target, unsigned char* pred,
                                       unsigned long long* confusion /*[C*C] accumulated*/, int B, int C, int h, int w,
                                       int H, int W, int ignore_index, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, WMAXC, ldl, h, w, H, W) && B >= 0, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const long grid = (long)B * ((W + NT - 1) / NT) * ((H + WROWS - 1) / WROWS);
  TSS_REQUIRE(grid <= 0x7fffffffL, TSS_ERR_SHAPE);
  tss::ProfScope prof(TSS_K_WIDE_ARGMAX, (hipStream_t)stream, (double)B * h * w * C * tss::esz(dtype) + (double)B * H * W * 9.0, 0);
  if (C <= WCM_LDS)
    TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL((wide_upsample_argmax_kernel<TT, true>), dim3((int)grid), dim3(NT), wide_argmax_lds_bytes(C, true),
                                             (hipStream_t)stream, (const TT*)low, ldl, target, pred, confusion, C, h, w, H, W, ignore_index));
  else
    TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL((wide_upsample_argmax_kernel<TT, false>), dim3((int)grid), dim3(NT), wide_argmax_lds_bytes(C, false),
                                             (hipStream_t)stream, (const TT*)low, ldl, target, pred, confusion, C, h, w, H, W, ignore_index));
  return tss::check_last("upsample_argmax_confusion_wide");
}

int tss_multiscale_argmax_confusion_wide(const tss_msmap* maps, int K, const long long* target, unsigned char* pred,
                                         unsigned long long* confusion /*[C*C] accumulated*/, int B, int C, int H, int W,
                                         int ignore_index, int mode, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(maps && K >= 1 && K <= MS_MAXK && C >= 1 && C <= WMAXC && B >= 0 && H >= 0 && W >= 0 && (mode == 0 || mode == 1),
              TSS_ERR_SHAPE);
  MsArgs args = {};
  double low_bytes;
  const int err = ms_args(maps, K, B, C, H, W, dtype, &args, &low_bytes);
  if (err != TSS_OK) return err;
  const bool counts = confusion && target;
  if ((long)B * H * W == 0 || (!pred && !counts)) return TSS_OK;
  const long grid = (long)B * ((W + NT - 1) / NT) * ((H + MSW_ROWS - 1) / MSW_ROWS);
  TSS_REQUIRE(grid <= 0x7fffffffL, TSS_ERR_SHAPE);
  const hipStream_t st = (hipStream_t)stream;
  tss::ProfScope prof(TSS_K_WIDE_MULTISCALE_ARGMAX, st, low_bytes + (double)B * H * W * ((pred ? 1.0 : 0.0) + (counts ? 8.0 : 0.0)), 0);
  TSS_WITH_DTYPE(dtype,
    if (C <= WCM_LDS) {
      if (mode == 0) launch_wide_ms<TT, 0, true>(grid, st, args, K, target, pred, confusion, C, H, W, ignore_index);
      else launch_wide_ms<TT, 1, true>(grid, st, args, K, target, pred, confusion, C, H, W, ignore_index);
    } else {
      if (mode == 0) launch_wide_ms<TT, 0, false>(grid, st, args, K, target, pred, confusion, C, H, W, ignore_index);
      else launch_wide_ms<TT, 1, false>(grid, st, args, K, target, pred, confusion, C, H, W, ignore_index);
    });
  return tss::check_last("multiscale_argmax_confusion_wide");
}

int tss_argmax_confusion_wide(const void* logits, const long long* target, unsigned char* pred,
                              unsigned long long* confusion /*[C*C] accumulated*/, long B, int C, long HW,
                              int ignore_index, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(tss::planar_shape_ok(B, C, HW, true) && C <= WMAXC && B >= 0 && HW >= 0, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(logits), TSS_ERR_ALIGN);
  const long groups = B * (HW / 8);
  if (groups == 0) return TSS_OK;
  long grid = tss::grid_for(groups, NT);
  if (grid > 1024) grid = 1024;
  tss::ProfScope prof(TSS_K_WIDE_ARGMAX, (hipStream_t)stream, (double)B * HW * (C * tss::esz(dtype) + 9.0), 0);
  if (C <= WCM_LDS)
    TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL((wide_planar_argmax_kernel<TT, true>), dim3((int)grid), dim3(NT), sizeof(unsigned int) * C * C,
                                             (hipStream_t)stream, (const TT*)logits, target, pred, confusion, B, C, HW, ignore_index));
  else
    TSS_WITH_DTYPE(dtype, hipLaunchKernelGGL((wide_planar_argmax_kernel<TT, false>), dim3((int)grid), dim3(NT), 0,
                                             (hipStream_t)stream, (const TT*)logits, target, pred, confusion, B, C, HW, ignore_index));
  return tss::check_last("argmax_confusion_wide");
}

}  // extern "C"
