// Block geometry of the register kernels of the fused head (loss.hip, softhead.hip): one definition for every pass that fills
// gradient tiles and for the gather (upsample_ce_gather_kernel) that reads them, so that the files cannot drift apart.
//   block = 256 consecutive output columns (a strip) x a band of output rows of one image; block index = (b * nband + band) * nstrip + strip
//   ws    = [nblocks][2] f64 loss rows, then [nblocks][tile_rows][tile_cells][CP] f32 tiles
#pragma once
#include "losssweep.h"

namespace {

struct CeGeom { int nstrip, nband, band_rows, tile_rows, tile_cells; };

// What every entry point of the upsampled-CE family asks of its shapes: classes in registers (at most 24), whole class groups per pixel.
inline bool upsample_ce_shape_ok(int C, long ldl, int h, int w, int H, int W) {
  return C > 0 && C <= 24 && (ldl % 8) == 0 && ldl >= (C + 3) / 4 * 4 && h > 0 && w > 0 && H >= h && W >= w;
}

// Geometry of the pass (the same on the host, in the pass and in the gather): bands / strips and the tile every block owns.
inline CeGeom ce_geom(int B, int h, int w, int H, int W) {
  constexpr int NT = lsw::NT;
  CeGeom g;
  g.nstrip = (W + NT - 1) / NT;
  // bands: enough blocks to fill the chip, but every band pays two extra row flushes
  g.band_rows = 64;
  while (g.band_rows > 16 && (long)B * g.nstrip * ((H + g.band_rows - 1) / g.band_rows) < 2048) g.band_rows /= 2;
  g.nband = (H + g.band_rows - 1) / g.band_rows;
  // conservative tile extent: a band of R output rows touches at most floor((R - 1) * (h - 1) / (H - 1)) + 3 low-res rows
  // (the pass and the gather index the tile by the rows / cells actually touched, which they both compute exactly)
  const double sy = H > 1 ? (double)(h - 1) / (double)(H - 1) : 0.0, sx = W > 1 ? (double)(w - 1) / (double)(W - 1) : 0.0;
  g.tile_rows = (int)((g.band_rows - 1) * sy) + 3;
  g.tile_cells = (int)((NT - 1) * sx) + 3;
  if (g.tile_rows > h) g.tile_rows = h;
  if (g.tile_cells > w) g.tile_cells = w;
  return g;
}

}  // namespace
