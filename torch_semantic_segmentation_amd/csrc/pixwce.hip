// Per-pixel loss weights on the fused decoder head: cross-entropy of the bilinearly upsampled logits, every pixel weighted by a map,
// straight from the LOW-RES NHWC logits.  The (B, C, H, W) logits and their gradient never exist.
//
//   k_i = omega_i w_{t_i}  for a valid pixel (target != ignore_index and 0 <= target < C; omega: the float32 [B][H][W] map, w: the class
//   weights, ones without),   loss = sum_valid k_i ce_i / D,   d loss / d z = k_i (p - onehot) / D,
//   D by `norm`: 0 sum_valid k_i (weighted mean), 1 sum_valid w_{t_i} (what the plain loss divides by), 2 the number of pixels B H W,
//   ignored ones included (torch.mean(ce * omega)).
//
// The kernels here leave (sum k ce, D-part) per block and UNSCALED gradient tiles; the division is tss_upsample_ce_group_finalize's
// (groupce.hip: D = 0 gives 0 and a zero gradient) and the gather tss_upsample_ce[_wide]_bwd_rows'.  Block layout, workspace layout and
// the flush protocol: headgeom.h.  No atomics, nothing zero-filled, no host read-back: capturable, the same bits on every run.  omega is
// taken as it is (negative values, nan: 0 * nan = nan); it is USED for a valid pixel only (the register pass loads it one row ahead, before
// the label is known, and discards it under an ignored pixel) and LOADED by lanes inside the image only.
//
//   pixw_ce_pass_kernel (C <= 24)   softhead_pass_kernel<SH_FOCAL>'s one pass with coef := k.  The target's logit leaves the loss per
//       pixel by a per-class select (the focal pass's way, not the one-hot dot product at flush time of upsample_ce_onepass_kernel):
//       ce = (m - z_t) + log2 sum in log2 units -- one subtraction, V_LOG_F32, one addition --, one product with k, one addition into
//       the lane's f32 sum (at most 64 rows); f64 from the wave sum on, where ln 2 is applied.  k = omega Cw[t] is one product; it scales
//       the one-hot table (l0 k, l1 k) and, as k / sum, the softmax half.
//   pixw_coef_kernel (24 < C <= 256)   the planar step between tss_upsample_pixel_ce_wide (ce per pixel) and
//       tss_upsample_coef_grad_wide (MODE 5 of wide_ce_kernel, tiles from a stored coefficient): on the wide head's own grid, one block =
//       one (sample, band of WROWS rows, strip of 256 columns), it turns ce in place into k (0 for a pixel that does not count) and
//       writes the block's row (sum k ce: an f32 product, summed in f64) where the MODE 5 pass leaves the row region unwritten.
//   mix_plane_kernel   mix_batch_kernel's mask (mix.hip, restated) applied to ONE float32 [B][H][W] plane: a select on bits between
//       sample b and sample partner[b], 8 pixels per thread; a group whose 8 pixels take one side reads that side only.
#include "headgeom.h"

namespace {

constexpr int CPMAX = 24;
constexpr int WMAXC = 256;        // as widehead.hip
constexpr double LN2D = 0.69314718055994530942;

template <typename T, int CP>
__global__ __launch_bounds__(NT, (CP <= 20 ? 3 : 2)) void pixw_ce_pass_kernel(const T* low, long ldl, const long long* target,
                                                                               const float* pixw, const float* cweight, float* tiles,
                                                                               double* rows, int C, int h, int w, int H, int W,
                                                                               int ignore_index, int norm, const HeadGeom geo) {
  __shared__ __align__(16) float Hh[2][NT * CP];      // the one-hot half of the gradient per low-res row buffer, [lane][class]
  __shared__ GatherLds tabs;
  __shared__ float Cw[CP];                            // class weights, 0 for the padding classes
  const int tid = threadIdx.x;
  if (tid < CP) Cw[tid] = tid < C ? (cweight ? cweight[tid] : 1.f) : 0.f;
  float* const tile = tiles + (long)blockIdx.x * geo.tile_rows * geo.tile_cells * CP;
  const HeadBlock blk = head_block(geo.nstrip, geo.nband, geo.band_rows, H, W);
  const HeadTaps map = head_taps(blk, h, w, H, W);
  const long b = blk.b;
  const int x = blk.x, ya = blk.ya, yb = blk.yb;
  const bool xin = blk.xin;
  const float sy = map.sy;
  const Tap tx = map.tx;
  const Gather gt = gather_windows(&tabs, blk, map, h, w, W);
#pragma unroll
  for (int c4 = 0; c4 < CP; c4 += 4) {
    *reinterpret_cast<float4*>(&Hh[0][tid * CP + c4]) = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(&Hh[1][tid * CP + c4]) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  gather_weights(gt);

  int rA = ac_tap(sy, ya, h).i0;
  int rB = rA + (rA < h - 1 ? 1 : 0);
  float aA[CP], aB[CP], gA[CP], gB[CP];
  auto load = [&](int r, float* a) { load_row<CP, true, true>(low, b * h + r, w, ldl, tx, C, a); };
  auto flush_row = [&](int r, int k, const float* g) {
    head_flush_row<CP>(gt, geo, Hh[k], g, r, CP, [](int, float*) {},
                       [&](int tr, int, int, int i, float sum) { tile[(long)tr * geo.tile_cells * CP + i] = sum; });   // [cell][c]
  };

  int kA = 0;                                  // Hh[kA] belongs to row rA, Hh[kA ^ 1] to row rB
  load(rA, aA);
  load(rB, aB);
#pragma unroll
  for (int c = 0; c < CP; ++c) { gA[c] = 0.f; gB[c] = 0.f; }
  __syncthreads();

  const long first = (b * H + ya) * (long)W;
  const long long* trow = target + first + (xin ? x : 0);
  const float* wrow = pixw + first + x;        // read by the lanes inside the image only
  long long tnext = *trow;
  float onext = xin ? *wrow : 0.f;
  float lsum = 0.f, dsum = 0.f;                // per lane over at most 64 rows; f64 from the wave sum on
  for (int y = ya; y < yb; ++y) {
    const long long t = tnext;
    const float om = onext;
    if (y + 1 < yb) {                          // next row's target and weight under this row's arithmetic
      tnext = trow[(long)(y + 1 - ya) * W];
      if (xin) onext = wrow[(long)(y + 1 - ya) * W];
    }
    const Tap ty = ac_tap(sy, y, h);           // uniform over the block
    while (rA < ty.i0) {                       // row tap advanced (headgeom.h)
      flush_row(rA, kA, gA);
      kA ^= 1;
      rA = rB;
      rB = rA + (rA < h - 1 ? 1 : 0);
#pragma unroll
      for (int c = 0; c < CP; ++c) { aA[c] = aB[c]; gA[c] = gB[c]; gB[c] = 0.f; }
      load(rB, aB);
    }
    const bool valid = xin && t != (long long)ignore_index && t >= 0 && t < C;
    const int ti = valid ? (int)t : -1;
    float z[CP];
    float m = -TSS_INF, zt = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      z[c] = (c < C) ? ty.l0 * aA[c] + ty.l1 * aB[c] : -TSS_INF;
      m = fmaxf(m, z[c]);
      zt = (ti == c) ? z[c] : zt;              // the target's logit (log2 units)
    }
    float ssum = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      z[c] = __builtin_amdgcn_exp2f(z[c] - m); // e_c (0 for the padding classes)
      ssum += z[c];
    }
    float spx = 0.f;                           // k / sum of exp: the scale of the softmax half
    if (valid) {
      const float cw = Cw[ti];
      const float k = om * cw;
      const float ce = (m - zt) + __builtin_amdgcn_logf(ssum);   // log2 units
      lsum += k * ce;
      dsum += norm == 0 ? k : cw;
      Hh[kA][tid * CP + ti] += ty.l0 * k;      // this lane's own row of the table: no race
      Hh[kA ^ 1][tid * CP + ti] += ty.l1 * k;
      spx = k * __builtin_amdgcn_rcpf(ssum);
    }
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const float pz = z[c] * spx;
      gA[c] += ty.l0 * pz;
      gB[c] += ty.l1 * pz;
    }
  }

  flush_row(rA, kA, gA);
  if (rB != rA) flush_row(rB, kA ^ 1, gB);     // else the band ended on the last low-res row: the l1 weights are zero there
  if (norm == 2) dsum = xin ? (float)(yb - ya) : 0.f;          // every pixel of the image, ignored ones included: an exact count
  double ds = (double)lsum, dc = (double)dsum;
  if (lsw::block_sum2(ds, dc)) {
    rows[2 * (long)blockIdx.x] = ds * LN2D;
    rows[2 * (long)blockIdx.x + 1] = dc;
  }
}

// One block = one (sample, band of WROWS rows, strip of NT columns) of the wide head's grid, lane = one column: pix holds the per-pixel
// cross-entropy in nats and leaves as k = omega w_t (0 for a pixel that does not count); rows[blockIdx] = (sum k ce, D-part).
__global__ __launch_bounds__(NT) void pixw_coef_kernel(float* pix, const long long* target, const float* pixw, const float* cweight,
                                                       double* rows, int C, int H, int W, int ignore_index, int norm, int nstrip,
                                                       int nband) {
  const HeadBlock blk = head_block(nstrip, nband, WROWS, H, W);
  double lsum = 0.0, dsum = 0.0;
  if (blk.xin) {
    for (int y = blk.ya; y < blk.yb; ++y) {
      const long i = (blk.b * H + y) * (long)W + blk.x;
      const long long t = target[i];
      const bool valid = t != (long long)ignore_index && t >= 0 && t < C;
      float k = 0.f;
      if (valid) {
        const float cw = cweight ? cweight[t] : 1.f;
        k = pixw[i] * cw;
        lsum += (double)(k * pix[i]);
        dsum += norm == 0 ? (double)k : (double)cw;
      }
      pix[i] = k;
    }
    if (norm == 2) dsum = (double)(blk.yb - blk.ya);
  }
  if (lsw::block_sum2(lsum, dsum)) {
    rows[2 * (long)blockIdx.x] = lsum;
    rows[2 * (long)blockIdx.x + 1] = dsum;
  }
}

// mix_batch_kernel's mask on one plane of 4-byte words: thread = 8 consecutive pixels of a row
__global__ __launch_bounds__(256) void mix_plane_kernel(const unsigned int* __restrict__ plane, const unsigned char* __restrict__ label,
                                                        const int* __restrict__ partner, const unsigned char* __restrict__ sel,
                                                        const int* __restrict__ boxes, unsigned int* __restrict__ out, long B, int H,
                                                        int W) {
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
    unsigned int m = 0u;                                         // bit j: pixel j takes sample b
    if (sel) {
      const uint2 la = *reinterpret_cast<const uint2*>(label + b * HW + off);
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
    const unsigned int* const pa = plane + b * HW + off;
    const unsigned int* const pp = plane + (long)pb * HW + off;
    unsigned int* const po = out + b * HW + off;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      uint4 o;
      if (m == 0xffu) o = *reinterpret_cast<const uint4*>(pa + 4 * v);
      else if (m == 0u) o = *reinterpret_cast<const uint4*>(pp + 4 * v);
      else {
        const uint4 a = *reinterpret_cast<const uint4*>(pa + 4 * v);
        const uint4 p = *reinterpret_cast<const uint4*>(pp + 4 * v);
        const unsigned int aw[4] = {a.x, a.y, a.z, a.w}, pw[4] = {p.x, p.y, p.z, p.w};
        unsigned int ow[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) ow[q] = ((m >> (4 * v + q)) & 1u) ? aw[q] : pw[q];
        o = make_uint4(ow[0], ow[1], ow[2], ow[3]);
      }
      *reinterpret_cast<uint4*>(po + 4 * v) = o;
    }
  }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" {

int tss_upsample_ce_pixw_fwd(const void* low, long ldl, const long long* target, const float* pixel_weight,
                             const float* class_weight /*[C] or null*/, int norm, float* ws /* tss_upsample_ce_ws floats, not initialised */,
                             int B, int C, int h, int w, int H, int W, int ignore_index, int dtype, void* stream) {
  TSS_CHECK_DTYPE(dtype);
  TSS_REQUIRE(head_shape_ok(C, CPMAX, ldl, h, w, H, W) && B >= 0 && norm >= 0 && norm <= 2, TSS_ERR_SHAPE);
  TSS_REQUIRE(low && target && pixel_weight && ws, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(low) && tss::aligned16(ws) && aligned4(pixel_weight), TSS_ERR_ALIGN);
  if ((long)B * H * W == 0) return TSS_OK;
  const HeadGeom geo = head_geom(B, C, h, w, H, W, false);
  const long grid = head_blocks(B, geo);
  TSS_REQUIRE(grid <= 0x7fffffffL, TSS_ERR_SHAPE);
  double* rows = reinterpret_cast<double*>(ws);
  float* tiles = ws + grid * 4;
  const hipStream_t st = (hipStream_t)stream;
  tss::ProfScope prof(TSS_K_UPSAMPLE_CE_FWD, st, (double)B * h * w * C * (tss::esz(dtype) + 8.0) + (double)B * H * W * 12.0, 0);
  TSS_WITH_DTYPE(dtype, TSS_WITH_CLASS_REGS(C,
    hipLaunchKernelGGL((pixw_ce_pass_kernel<TT, CPV>), dim3((int)grid), dim3(NT), 0, st, (const TT*)low, ldl, target, pixel_weight,
                       class_weight, tiles, rows, C, h, w, H, W, ignore_index, norm, geo)));
  return tss::check_last("upsample_ce_pixw_fwd");
}

int tss_upsample_ce_pixw_coef_wide(float* pix, const long long* target, const float* pixel_weight, const float* class_weight /*[C] or null*/,
                                   int norm, float* ws_rows /* the head of tss_upsample_ce_wide_ws floats */, int B, int C, int H, int W,
                                   int ignore_index, void* stream) {
  TSS_REQUIRE(C > 0 && C <= WMAXC && B >= 0 && H > 0 && W > 0 && norm >= 0 && norm <= 2, TSS_ERR_SHAPE);
  TSS_REQUIRE(pix && target && pixel_weight && ws_rows, TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(ws_rows) && aligned4(pixel_weight) && aligned4(pix), TSS_ERR_ALIGN);
  if (B == 0) return TSS_OK;
  const int nstrip = (W + NT - 1) / NT, nband = (H + WROWS - 1) / WROWS;       // head_geom's for the wide head
  const long grid = (long)B * nstrip * nband;
  TSS_REQUIRE(grid <= 0x7fffffffL, TSS_ERR_SHAPE);
  hipLaunchKernelGGL(pixw_coef_kernel, dim3((int)grid), dim3(NT), 0, (hipStream_t)stream, pix, target, pixel_weight, class_weight,
                     reinterpret_cast<double*>(ws_rows), C, H, W, ignore_index, norm, nstrip, nband);
  return tss::check_last("upsample_ce_pixw_coef_wide");
}

int tss_mix_plane(const float* plane, const unsigned char* label, const int* partner, const unsigned char* sel, const int* boxes,
                  float* out, long B, int H, int W, void* stream) {
  TSS_REQUIRE(B >= 0 && B <= 65535 && H >= 1 && W >= 8 && (W % 8) == 0 && plane && label && partner && out &&
              ((sel != nullptr) != (boxes != nullptr)), TSS_ERR_SHAPE);
  TSS_REQUIRE(tss::aligned16(plane) && tss::aligned16(out) && (reinterpret_cast<uintptr_t>(label) & 7u) == 0, TSS_ERR_ALIGN);
  if (B == 0) return TSS_OK;
  const long groups = (long)H * W / 8;
  const int gx = tss::grid_for(groups, 256, 1024);
  hipLaunchKernelGGL(mix_plane_kernel, dim3(gx, (int)B), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const unsigned int*>(plane),
                     label, partner, sel, boxes, reinterpret_cast<unsigned int*>(out), B, H, W);
  return tss::check_last("mix_plane");
}

}  // extern "C"
