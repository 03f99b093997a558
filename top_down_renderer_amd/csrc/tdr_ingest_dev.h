// tdr_ingest_dev.h — the per-cell bodies of the label-image ingest (tdr_map.hip): the class word of a cell, the column pass
// and the row pass of the windowed distance transform.  The whole-map kernels (tdr_map.hip) and the incremental update
// (tdr_map_incr.hip) both call these, so a cell's record is the same expression on either path, bit for bit.
#ifndef TDR_INGEST_DEV_H_
#define TDR_INGEST_DEV_H_
#include "tdr_common.h"

// Per cell the ingest keeps a word of class bits: bit c = the cell lies inside class c; bit 31 = no known class (mask = 1).
// A label image gives one bit per cell; the per-class rasters of the raster cache may overlap.
#define INGEST_MAXC 16
#define INGEST_UNKNOWN 0x80000000u
// the image pixel cell (yi, xi) reads (:137-138) — row 0 of the map is the bottom row of the image
__device__ inline int64_t ingest_pixel(int yi, int xi, int img_h, int img_w, float resolution) {
  int iy = (int)((float)img_h - (float)yi * resolution - 1.f);
  iy = iy > 0 ? iy : 0;
  int ix = (int)((float)xi * resolution);
  ix = ix < img_w - 1 ? ix : img_w - 1;
  return (int64_t)iy * img_w + ix;
}
// the class word of cell (yi, xi) of a label image through the flatten LUT (:139)
__device__ inline uint32_t ingest_label_word(const uint8_t* __restrict__ img, int img_h, int img_w,
                                             const int32_t* __restrict__ lut, int lut_size, int ncls, int yi, int xi,
                                             float resolution) {
  const int label = img[ingest_pixel(yi, xi, img_h, img_w, resolution)];
  int c = label < lut_size ? lut[label] : -1;
  if (c < 0 || c >= ncls) c = -1;  // :139
  return c < 0 ? INGEST_UNKNOWN : (1u << c);
}

// pass 1 at cell (y, x): per class, distance (in cells, along the column) to the nearest cell of that class, capped at 255
__device__ inline void ingest_coldist_cell(const uint32_t* __restrict__ cls_map, int rows, int cols, int R, int y, int x,
                                           uint8_t* __restrict__ g /* [rows*cols][INGEST_MAXC] */) {
  int gd[INGEST_MAXC];
#pragma unroll
  for (int c = 0; c < INGEST_MAXC; c++) gd[c] = 255;
  for (int d = 0; d <= R; d++) {
    const int ya = y - d, yb = y + d;
    const uint32_t ca = ya >= 0 ? cls_map[(int64_t)ya * cols + x] : 0u;
    const uint32_t cb = yb < rows ? cls_map[(int64_t)yb * cols + x] : 0u;
    const uint32_t either = ca | cb;
#pragma unroll
    for (int c = 0; c < INGEST_MAXC; c++)
      if (((either >> c) & 1u) && gd[c] == 255) gd[c] = d;
  }
  uint8_t* o = g + ((int64_t)y * cols + x) * INGEST_MAXC;
#pragma unroll
  for (int c = 0; c < INGEST_MAXC; c++) o[c] = (uint8_t)gd[c];
}

// pass 2 at cell (y, x): exact squared distance = min over the row window of dx^2 + g^2; then the reference's
// post-processing.  d[0..ncls) = the cell's distances, the return value = `known` (0 or 1)
__device__ inline float ingest_rowmin_cell(const uint32_t* __restrict__ cls_map, const uint8_t* __restrict__ g, int ncls,
                                           int cols, int R, float resolution, int y, int x, float* d_out) {
  int best[INGEST_MAXC];
#pragma unroll
  for (int c = 0; c < INGEST_MAXC; c++) best[c] = 0x7fffffff;
  const int x0 = x - R > 0 ? x - R : 0, x1 = x + R < cols - 1 ? x + R : cols - 1;
  for (int xx = x0; xx <= x1; xx++) {
    const int dx2 = (xx - x) * (xx - x);
    const uint4 gv = *reinterpret_cast<const uint4*>(g + ((int64_t)y * cols + xx) * INGEST_MAXC);
    const unsigned wv[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
    for (int c = 0; c < INGEST_MAXC; c++) {
      const int gd = (int)((wv[c >> 2] >> (8 * (c & 3))) & 0xFF);
      const int cand = gd == 255 ? 0x7fffffff : dx2 + gd * gd;
      best[c] = cand < best[c] ? cand : best[c];
    }
  }
  const bool unknown = (cls_map[(int64_t)y * cols + x] & INGEST_UNKNOWN) != 0;  // no class here (:294-299): mask = 1, distances zeroed (:317)
#pragma unroll
  for (int c = 0; c < INGEST_MAXC; c++) {
    if (c < ncls) {
      float d = best[c] == 0x7fffffff ? 3.0e38f : sqrtf((float)best[c]);  // cv::distanceTransform, precise L2
      d = d * resolution;                                                   // :314
      d = d > 50.f ? 50.f : d;                                              // :315 THRESH_TRUNC
      d_out[c] = unknown ? 0.f : d;
    }
  }
  return unknown ? 0.f : 1.f;
}
#endif  // TDR_INGEST_DEV_H_
