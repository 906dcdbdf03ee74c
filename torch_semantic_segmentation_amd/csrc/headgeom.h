// The band walk of the fused decoder head: what loss.hip, softhead.hip, widehead.hip, msflip.hip and groupce.hip share.
//
// Block layout.  A block owns 256 consecutive output columns (a strip) x a band of output rows of one image; block index =
//   (b * nband + band) * nstrip + strip (head_block); lane = one output column (head_taps: its column taps in a map).  The column taps
//   of a lane never change and the row taps only every ~scale rows, so the lane keeps the two horizontally interpolated low-res rows
//   rA, rB of its column in registers (aA[c], aB[c]; load_row) and a logit is one blend of the two.
// Workspace layout.  ws = [nblocks][2] f64 loss rows, then [nblocks][tile_rows][tile_cells][cp] f32 tiles.  A low-res cell gets
//   contributions from up to four blocks (two bands x two strips); every block stores ITS contribution to every (row, cell, class) of
//   its footprint into its own tile (plain stores, each element written exactly once, nothing zero-filled) and its loss sums into its
//   own row, and the gather (head_gather) adds the <= 4 tiles of a cell in (band, strip) order: no atomics, the same bits on every run.
//   head_band / head_band_rows / head_strip_cells say which rows and cells a block touches, for the passes and for the gather alike.
// Flush protocol.  The softmax half of the gradient of the two low-res rows lives in registers (gA, gB), the one-hot half per lane in
//   LDS (Hh[k][lane][class], k = buffer of row rA / rB).  When a low-res row is finished (head_flush_row) the lane parks g - Hh[k] in
//   Hh[k], barrier, one thread per (cell, class) sums the lanes whose column taps include the cell (gather_cell; the windows and
//   weights are fixed per block: gather_windows before the block's first barrier, gather_weights after it), stores the sum into the
//   tile, barrier, and the lane clears its part of Hh[k].  (LDS float atomics for the scatter were measured at ~180 cycles per wave
//   instruction.)  An instance that never flushes compiles the tables and the flush out.
// Who uses what.  Host geometry, head_gather and ce_finalize_rows_kernel: every file (groupce.hip: the geometry and the gather with a
//   scale per sample, head_gather's ROWS; its finalize is its own).  head_block / head_taps: softhead_pass_kernel,
//   wide_upsample_argmax_kernel and the two multi-scale kernels.  load_row: softhead.hip and msflip.hip.  The tables and the flush:
//   softhead_pass_kernel.  upsample_ce_onepass_kernel, upsample_argmax_kernel (loss.hip) and wide_ce_kernel keep these steps written
//   out, and every kernel its own advance of the two-row window: the compiler's register allocation and its choice of which products
//   of the unrolled blends to fuse move with the smallest change of those kernels' text (profiles/headwalk_isa.txt), and they are
//   held to the same bits, registers and time.  They follow the protocol above to the letter; a change of it is made there too.
#pragma once
#include "losssweep.h"

namespace {

constexpr int NT = lsw::NT;
constexpr int WROWS = 16;         // output rows per band of the wide (chunked) head: WROWS x 256 floats of LDS per per-pixel quantity
constexpr int MS_MAXK = 16;
constexpr int MAXCELL = NT + 2, WTAB = 1024;
constexpr float LOG2E = 1.44269504088896340736f;

// ---- host side ------------------------------------------------------------------------------------------------
struct HeadGeom { int nstrip, nband, band_rows, tile_rows, tile_cells, cp; };

// What every entry point of the family asks of its shapes: at most `cap` classes (24 in registers, 256 by chunks), whole class groups.
inline bool head_shape_ok(int C, int cap, long ldl, int h, int w, int H, int W) {
  return C > 0 && C <= cap && (ldl % 8) == 0 && ldl >= (C + 3) / 4 * 4 && h > 0 && w > 0 && H >= h && W >= w;
}

// Geometry of a pass (the same on the host, in the pass and in the gather): bands / strips, the tile every block owns and its class pitch.
inline HeadGeom head_geom(int B, int C, int h, int w, int H, int W, bool wide) {
  HeadGeom g;
  g.nstrip = (W + NT - 1) / NT;
  // register kernels: enough blocks to fill the chip, but every band pays two extra row flushes; wide kernels: what their LDS holds
  g.band_rows = wide ? WROWS : 64;
  while (!wide && g.band_rows > 16 && (long)B * g.nstrip * ((H + g.band_rows - 1) / g.band_rows) < 2048) g.band_rows /= 2;
  g.nband = (H + g.band_rows - 1) / g.band_rows;
  // conservative tile extent: a band of R output rows touches at most floor((R - 1) * (h - 1) / (H - 1)) + 3 low-res rows
  // (the pass and the gather index the tile by the rows / cells actually touched, which they both compute exactly)
  const double sy = H > 1 ? (double)(h - 1) / (double)(H - 1) : 0.0, sx = W > 1 ? (double)(w - 1) / (double)(W - 1) : 0.0;
  g.tile_rows = (int)((g.band_rows - 1) * sy) + 3;
  g.tile_cells = (int)((NT - 1) * sx) + 3;
  if (g.tile_rows > h) g.tile_rows = h;
  if (g.tile_cells > w) g.tile_cells = w;
  g.cp = (C + 3) / 4 * 4;
  if (!wide) TSS_WITH_CLASS_REGS(C, g.cp = CPV);   // the same choice as the kernels that fill the tiles
  return g;
}

inline long head_blocks(int B, const HeadGeom& g) { return (long)B * g.nstrip * g.nband; }

// floats of the workspace; 0 for a refused shape
inline long head_ws_floats(int B, int C, int cap, int h, int w, int H, int W, bool wide) {
  if (B <= 0 || C <= 0 || C > cap || h <= 0 || w <= 0 || H < h || W < w) return 0;
  const HeadGeom g = head_geom(B, C, h, w, H, W, wide);
  return head_blocks(B, g) * 4 /* 2 doubles */ + head_blocks(B, g) * g.tile_rows * g.tile_cells * g.cp;
}

// The multi-scale descriptors as the kernels take them: by value, in the kernel argument segment (no device memory, no copy to wait for).
struct MsMap { const void* low; long first; int ldl, h, w, flip; };
struct MsArgs { MsMap m[MS_MAXK]; };

// checks the K descriptors and copies them; *low_bytes = what the maps hold
inline int ms_args(const tss_msmap* maps, int K, int B, int C, int H, int W, int dtype, MsArgs* args, double* low_bytes) {
  *low_bytes = 0.0;
  for (int k = 0; k < K; ++k) {
    const tss_msmap& m = maps[k];
    TSS_REQUIRE(m.low && (m.ldl % 8) == 0 && m.ldl >= (C + 3) / 4 * 4 && m.ldl <= (1L << 30) && m.h >= 1 && m.w >= 1 &&
                m.h <= H && m.w <= W && m.first >= 0, TSS_ERR_SHAPE);
    TSS_REQUIRE(tss::aligned16(m.low), TSS_ERR_ALIGN);
    args->m[k].low = m.low; args->m[k].first = m.first; args->m[k].ldl = (int)m.ldl;
    args->m[k].h = m.h; args->m[k].w = m.w; args->m[k].flip = m.flip ? 1 : 0;
    *low_bytes += (double)B * m.h * m.w * C * tss::esz(dtype);
  }
  return TSS_OK;
}

// ---- block decomposition ----------------------------------------------------------------------------------------
// output rows [ya, yb) of a band
__device__ __forceinline__ void head_band(int band, int band_rows, int H, int* ya, int* yb) {
  *ya = band * band_rows;
  *yb = *ya + band_rows < H ? *ya + band_rows : H;
}
// first / last low-res row the band's block touches, first cell / cell count of a strip (<= NT + 2 for W >= w, host-checked)
__device__ __forceinline__ void head_band_rows(float sy, int ya, int yb, int h, int* r0, int* r1) {
  *r0 = ac_tap(sy, ya, h).i0;
  *r1 = ac_tap(sy, yb - 1, h).i1;
}
__device__ __forceinline__ void head_strip_cells(float sx, int strip, int W, int w, int* c0, int* n) {
  const int xl = (strip * NT + NT - 1 < W) ? strip * NT + NT - 1 : W - 1;
  *c0 = ac_tap(sx, strip * NT, w).i0;
  *n = ac_tap(sx, xl, w).i1 - *c0 + 1;
}

struct HeadBlock { long b; int band, strip, x, xc, ya, yb; bool xin; };   // xc: lanes past the edge compute column W - 1 and write nothing
__device__ __forceinline__ HeadBlock head_block(int nstrip, int nband, int band_rows, int H, int W) {
  HeadBlock k;
  int bid = blockIdx.x;
  k.strip = bid % nstrip; bid /= nstrip;
  k.band = bid % nband;
  k.b = bid / nband;
  k.x = k.strip * NT + threadIdx.x;
  k.xin = k.x < W;
  k.xc = k.xin ? k.x : W - 1;
  head_band(k.band, band_rows, H, &k.ya, &k.yb);
  return k;
}
// the scales of a map (h, w) and the lane's column taps in it; flip: the map is read right to left
struct HeadTaps { float sx, sy; Tap tx; };
__device__ __forceinline__ HeadTaps head_taps(const HeadBlock& k, int h, int w, int H, int W, int flip = 0) {
  HeadTaps t;
  t.sy = ac_scale(h, H); t.sx = ac_scale(w, W);
  t.tx = ac_tap(t.sx, flip ? W - 1 - k.xc : k.xc, w);
  return t;
}

// ---- one row of the two-row register window ------------------------------------------------------------------------
// a[c] = l0x * L[row][i0x][c] + l1x * L[row][i1x][c] of the rows at `base` (LOG2: times log2 e), PAD_INF ? -inf : 0 for the padding
// classes.  4-channel groups that start at or past C are not read (uniform; ldl >= round_up(C, 4), host-checked: a group that starts
// below C ends inside the pitch).
template <int N, bool PAD_INF, bool LOG2, typename T>
__device__ __forceinline__ void load_row(const T* base, long row, int w, long ldl, const Tap tx, int C, float* a) {
  const T* p0 = base + (row * (long)w + tx.i0) * ldl;
  const T* p1 = base + (row * (long)w + tx.i1) * ldl;
#pragma unroll
  for (int c4 = 0; c4 < N; c4 += 4) {
    float u[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
    if (c4 < C) {
      V4<T>::load(p0 + c4, u);
      V4<T>::load(p1 + c4, v);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      a[c4 + q] = (c4 + q < C) ? (LOG2 ? (tx.l0 * u[q] + tx.l1 * v[q]) * LOG2E : tx.l0 * u[q] + tx.l1 * v[q]) : (PAD_INF ? -TSS_INF : 0.f);
  }
}

// ---- gather tables and the row flush ---------------------------------------------------------------------------
struct GatherLds {
  int Li0[NT], Li1[NT], Wlo[MAXCELL], Whi[MAXCELL];   // a lane's two cells (-1 past the image edge); a cell's window of lanes
  float Ll1[NT], Wt[WTAB];                            // a lane's l1; gather weights [cell][lane - Wlo[cell]]
};
struct Gather { GatherLds* t; int r_first, cx0, ncell, maxwin; bool wtab; };   // uniform over the block

// part 1, before the block's barrier: the lane's cells and every cell's window
__device__ __forceinline__ Gather gather_windows(GatherLds* t, const HeadBlock& k, const HeadTaps& m, int h, int w, int W) {
  const int tid = threadIdx.x;
  Gather g;
  int r_last;
  g.t = t;
  head_band_rows(m.sy, k.ya, k.yb, h, &g.r_first, &r_last);
  head_strip_cells(m.sx, k.strip, W, w, &g.cx0, &g.ncell);
  t->Li0[tid] = k.xin ? m.tx.i0 - g.cx0 : -1;
  t->Li1[tid] = k.xin ? m.tx.i1 - g.cx0 : -1;
  t->Ll1[tid] = m.tx.l1;
  g.maxwin = m.sx > 0.f ? (int)(2.f / m.sx) + 6 : NT;   // widest window of lanes whose taps can include one low-res column
  g.wtab = (long)g.ncell * g.maxwin <= WTAB;
  for (int cell = tid; cell < g.ncell; cell += NT) {
    int lo, hi;
    ac_window(m.sx, g.cx0 + cell, W, &lo, &hi);
    lo -= k.strip * NT; hi -= k.strip * NT;
    lo = lo < 0 ? 0 : lo;
    hi = hi > NT - 1 ? NT - 1 : hi;
    if (g.wtab && hi - lo + 1 > g.maxwin) hi = lo + g.maxwin - 1;   // cannot happen (conservative bound); keeps the table safe
    t->Wlo[cell] = lo;
    t->Whi[cell] = hi;
  }
  return g;
}
// part 2, after it: the weights
__device__ __forceinline__ void gather_weights(const Gather& g) {
  GatherLds* const t = g.t;
  if (!g.wtab) return;
  for (int i = threadIdx.x; i < g.ncell * g.maxwin; i += NT) {
    const int cell = i / g.maxwin, k = i - cell * g.maxwin;
    const int l = t->Wlo[cell] + k;
    float wgt = 0.f;
    if (l <= t->Whi[cell]) { const float l1 = t->Ll1[l]; wgt = (t->Li0[l] == cell ? 1.f - l1 : 0.f) + (t->Li1[l] == cell ? l1 : 0.f); }
    t->Wt[i] = wgt;
  }
}
// sum over the lanes whose column taps include `cell` of weight * G[lane][c]
__device__ __forceinline__ float gather_cell(const Gather& g, const float* G, int pitch, int cell, int c) {
  const GatherLds* const t = g.t;
  const int llo = t->Wlo[cell], lhi = t->Whi[cell];
  float sum = 0.f;
  if (g.wtab) {
    const float* wt = t->Wt + cell * g.maxwin - llo;
    for (int l = llo; l <= lhi; ++l) sum += wt[l] * G[l * pitch + c];
  } else {
    for (int l = llo; l <= lhi; ++l) {
      const float l1 = t->Ll1[l];
      const float wgt = (t->Li0[l] == cell ? 1.f - l1 : 0.f) + (t->Li1[l] == cell ? l1 : 0.f);
      sum += wgt * G[l * pitch + c];
    }
  }
  return sum;
}

// Finished low-res row r, whose one-hot table is G = Hh[k] ([lane][PITCH]) and whose softmax half is g[PITCH]: the protocol above.
// adjust(c4, hq) may change the lane's four one-hot values of a class group before they leave g; store(tr, cell, c, i, sum) puts the sum
// of (cell, class c < nclass), i = cell * PITCH + c, into row tr of the tile.  The guards always hold (the host's tile extent is
// conservative); they keep the stores inside the tile.
template <int PITCH, typename Adjust, typename Store>
__device__ __forceinline__ void head_flush_row(const Gather& gt, const HeadGeom& geo, float* G, const float* g, int r, int nclass, Adjust&& adjust,
                                               Store&& store) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int c4 = 0; c4 < PITCH; c4 += 4) {
    const float4 hv = *reinterpret_cast<const float4*>(G + tid * PITCH + c4);
    float hq[4] = {hv.x, hv.y, hv.z, hv.w};
    adjust(c4, hq);
    *reinterpret_cast<float4*>(G + tid * PITCH + c4) = make_float4(g[c4] - hq[0], g[c4 + 1] - hq[1], g[c4 + 2] - hq[2], g[c4 + 3] - hq[3]);
  }
  __syncthreads();
  const int tr = r - gt.r_first;
  if (tr >= 0 && tr < geo.tile_rows) {
    for (int i = tid; i < gt.ncell * PITCH; i += NT) {
      const int cell = i / PITCH, c = i - cell * PITCH;
      if (cell >= geo.tile_cells || c >= nclass) continue;
      store(tr, cell, c, i, gather_cell(gt, G, PITCH, cell, c));   // every element of the block's footprint, exactly once
    }
  }
  __syncthreads();
#pragma unroll
  for (int c4 = 0; c4 < PITCH; c4 += 4) *reinterpret_cast<float4*>(G + tid * PITCH + c4) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- the gather and the row finalize ---------------------------------------------------------------------------
// dlow[b][r][cx][:] = (T)(grad_out / count * sum over the tiles that hold cell (r, cx), in (band, strip) order); thread = one
// cell x 8 channels.  CPT: the tile pitch at compile time; 0, the wide head: geo.cp at run time, bands of WROWS rows.  Channels >= pitch
// (padding) are written as zeros.  ROWS (groupce.hip): inv_count is a row of B per-sample scales and sample b's cells take
// inv_count[b] * grad_out; the instances without it are the text they were.
template <typename T, int CPT, bool ROWS = false>
__device__ __forceinline__ void head_gather(const float* tiles, const float* inv_count, const float* grad_out, T* dlow, long ldl, int B,
                                            int h, int w, int H, int W, const HeadGeom& geo) {
  const float g0 = (ROWS ? 1.f : *inv_count) * (grad_out ? *grad_out : 1.f);   // ROWS: grad_out alone (1.f * x is x)
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  constexpr bool WIDE = CPT == 0;          // the wide head also keeps three compares that always hold, as it always did
  const int cv = (int)(ldl / 8), cp = WIDE ? geo.cp : CPT, band_rows = WIDE ? WROWS : geo.band_rows;
  const long total = (long)B * h * w * cv;
  for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {      // launched with NT threads
    const int c8 = (int)(i % cv) * 8;
    long q = i / cv;
    const int cx = (int)(q % w); q /= w;
    const int r = (int)(q % h);
    const long b = q / h;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    int ylo, yhi, xlo, xhi;
    ac_window(sy, r, H, &ylo, &yhi);
    ac_window(sx, cx, W, &xlo, &xhi);
    for (int band = ylo / band_rows; band <= yhi / band_rows && (WIDE ? c8 < cp : true); ++band) {
      int ya, yb, r0, r1;
      head_band(band, band_rows, H, &ya, &yb);
      head_band_rows(sy, ya, yb, h, &r0, &r1);
      if (r < r0 || r > r1 || (WIDE && r - r0 >= geo.tile_rows)) continue;
      for (int strip = xlo / NT; strip <= xhi / NT; ++strip) {
        int c0, n;
        head_strip_cells(sx, strip, W, w, &c0, &n);
        if (cx < c0 || cx >= c0 + n || (WIDE && cx - c0 >= geo.tile_cells)) continue;
        const float* t = tiles + ((((b * geo.nband + band) * geo.nstrip + strip) * geo.tile_rows + (r - r0)) * (long)geo.tile_cells
                                  + (cx - c0)) * cp + c8;
        if (c8 + 4 <= cp) { float u[4]; V4<float>::load(t, u); v[0] += u[0]; v[1] += u[1]; v[2] += u[2]; v[3] += u[3]; }
        if (c8 + 8 <= cp) { float u[4]; V4<float>::load(t + 4, u); v[4] += u[0]; v[5] += u[1]; v[6] += u[2]; v[7] += u[3]; }
      }
    }
    const float gs = ROWS ? inv_count[b] * g0 : g0;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] *= gs;
    V8<T>::store(dlow + ((b * h + r) * (long)w + cx) * ldl + c8, v);
  }
}

// loss = sum(rows[.][0]) / sum(rows[.][1]) in a fixed order (one block); n == 0 -> nan, like torch.  EX, the weighted / smoothed
// entries: there the numerator of an empty denominator need not be 0 (valid pixels whose class weight is 0 still carry the smoothing
// term), and torch's (1 - eps) * (0 / 0) + ... is nan, not inf.
template <bool EX>
__global__ __launch_bounds__(NT) void ce_finalize_rows_kernel(const double* rows, int nrows, float* loss, float* inv_count) {
  double sum, n;
  if (lsw::row_sum2(rows, nrows, sum, n)) {
    *loss = (EX && !(n > 0.0)) ? __builtin_nanf("") : (float)(sum / n);
    *inv_count = n > 0.0 ? (float)(1.0 / n) : 0.f;
  }
}

}  // namespace
