// tdr_raster_dev.h — the bodies of the scan raster (tdr_raster.hip): the bin of a point, its 4-byte key, the keyed count
// of a column tile and the tile's write-out, and the launch shape of an image.  The standalone kernels (tdr_raster.hip) and
// the batched ones (tdr_batch_loop.hip: many clouds in one launch) both call these, so a cloud's image is the same
// expressions, the same tiles and the same thread counts on either path, bit for bit.
#ifndef TDR_RASTER_DEV_H_
#define TDR_RASTER_DEV_H_
#include <algorithm>

#include "tdr_common.h"
#include "tdr_atan2f.h"

// the bin key of a point: col << 20 | class << 16 | row
#define RASTER_NO_BIN 0xFFFFFFFFu
#define RASTER_KEY_MAX_COLS 4095
#define RASTER_KEY_MAX_ROWS 65535

// x, y and label of point q
__device__ __forceinline__ void raster_point(const float* __restrict__ pts, int stride, int ioff, int64_t q, float& x,
                                             float& y, float& cf) {
  const float* p = pts + q * stride;
  if (stride == 4 && ioff == 3) {
    float4 v = *reinterpret_cast<const float4*>(p);
    x = v.x; y = v.y; cf = v.w;
  } else {
    x = p[0]; y = p[1]; cf = p[ioff];
  }
}
__device__ __forceinline__ bool raster_bin(int polar, float res, float ang_res, int rows, int cols, float x, float y,
                                           int& row, int& col) {
  if (x == 0.f && y == 0.f) return false;
  // A non-finite coordinate never lands in the image: the reference's float -> int conversions of NaN / inf give INT_MIN
  // on x86-64, which fails `>= 0` (scan_renderer_polar.cpp:102, scan_renderer.cpp:71); the GPU's conversion of NaN gives
  // 0, so the point is dropped here (organised PCL clouds with is_dense == false carry NaN points).
  if (!(fabsf(x) < INFINITY) || !(fabsf(y) < INFINITY)) return false;
  if (polar) {
    float theta = tdr_atan2f(x, y);  // glibc-exact (tdr_atan2f.h)
    float r = sqrtf(x * x + y * y);
    row = (int)(roundf(theta / ang_res) + (float)(rows / 2));
    col = (int)roundf(r / res);
  } else {
    col = (int)(roundf(x / res) + (float)(cols / 2));
    row = (int)(roundf(y / res) + (float)(rows / 2));
  }
  return row >= 0 && row < rows && col >= 0 && col < cols;
}
// the class of a point's label through the LUT (-1: none)
__device__ __forceinline__ int raster_class(const int32_t* lut, int ncls, float cf) {
  const int pc = (cf == cf) ? (int)cf : -1;   // NaN label: x86 converts to INT_MIN, outside the LUT
  if (pc < 0 || pc > 255) return -1;
  const int c = lut[pc];
  return (c >= 0 && c < ncls) ? c : -1;
}
// phase 1: the key of point q
__device__ __forceinline__ uint32_t raster_key(const float* __restrict__ pts, int stride, int ioff, int64_t q, int polar,
                                               float res, float ang_res, const int32_t* __restrict__ lut, int ncls, int rows,
                                               int cols) {
  float x, y, cf;
  raster_point(pts, stride, ioff, q, x, y, cf);
  int row, col;
  if (!raster_bin(polar, res, ang_res, rows, cols, x, y, row, col)) return RASTER_NO_BIN;
  const int c = raster_class(lut, ncls, cf);
  return c < 0 ? RASTER_NO_BIN : ((uint32_t)col << 20) | ((uint32_t)c << 16) | (uint32_t)row;
}

// phase 2, by the whole workgroup: the tile of columns [col0, col0 + ncol) as u32 counters cnt[ncol][ncls][rows] in LDS
__device__ __forceinline__ void raster_tile_clear(unsigned int* cnt, int tile) {
  for (int t = threadIdx.x; t < tile; t += blockDim.x) cnt[t] = 0;
}
__device__ __forceinline__ void raster_tile_count_keys(unsigned int* cnt, const uint32_t* __restrict__ keys, int64_t n,
                                                       int col0, int ncol, int ncls, int rows) {
  for (int64_t q = threadIdx.x; q < n; q += blockDim.x) {
    const uint32_t key = keys[q];
    const int col = (int)(key >> 20) - col0;
    if (key == RASTER_NO_BIN || col < 0 || col >= ncol) continue;
    atomicAdd(&cnt[(col * ncls + (int)((key >> 16) & 15u)) * rows + (int)(key & 0xFFFFu)], 1u);
  }
}
// the tile written whole, zeros included: the class planes img[ncls][rows * cols] and the packed records pk[rows * cols][rf]
// (either may be null)
__device__ __forceinline__ void raster_tile_write(const unsigned int* cnt, int col0, int ncol, int ncls, int rows, int cols,
                                                  int rf, float* __restrict__ img, float* __restrict__ pk) {
  const int tile = ncol * ncls * rows;
  const int64_t P = (int64_t)rows * cols;
  if (img) {
    for (int t = threadIdx.x; t < tile; t += blockDim.x) {
      int row = t % rows, cc = t / rows;
      int c = cc % ncls, col = cc / ncls;
      img[(int64_t)c * P + row + (int64_t)rows * (col0 + col)] = (float)cnt[t];
    }
  }
  if (pk) {
    const int bins = ncol * rows;
    for (int t = threadIdx.x; t < bins; t += blockDim.x) {
      int row = t % rows, col = t / rows;
      float* o = pk + ((int64_t)(col0 + col) * rows + row) * rf;
      unsigned int tot = 0;
      for (int c = 0; c < ncls; c++) {
        unsigned int v = cnt[(col * ncls + c) * rows + row];
        o[c] = (float)v;
        tot += v;
      }
      for (int c = ncls; c < rf - 1; c++) o[c] = 0.f;
      if (tdr_has_kslot(ncls, rf)) o[rf - 2] = 1.f;
      o[rf - 1] = (float)tot;
    }
  }
}

// ---- host: the launch shape of an image -----------------------------------------------------------------------------
#define RASTER_MAX_LDS (152 * 1024)   // one tile: most of a CU's 160 KB
struct RasterShape {
  int cpt;       // image columns per tile (workgroup)
  size_t lds;    // bytes of a tile's counters
  bool keyed;    // the image's bins fit the 4-byte key
};
// false: one image column does not fit an LDS tile
static inline bool raster_shape(int ncls, int rows, int cols, RasterShape* out) {
  const int64_t per_col = (int64_t)ncls * rows * 4;
  if (per_col > RASTER_MAX_LDS) return false;
  int cpt = (int)std::max<int64_t>(1, (64 * 1024) / per_col);
  cpt = std::min(cpt, cols);
  // enough workgroups to spread over the chip when the image is small
  while (cpt > 1 && cdiv(cols, cpt) < 32) cpt = (cpt + 1) / 2;
  out->cpt = cpt;
  out->lds = (size_t)cpt * per_col;
  out->keyed = cols <= RASTER_KEY_MAX_COLS && rows <= RASTER_KEY_MAX_ROWS;
  return true;
}
// a tile of more than 64 KB (one column, cpt = 1) has to be allowed per kernel and device, once; attr_set: the kernel's own
// 64 flags
static inline hipError_t raster_allow_lds(const void* kernel, size_t lds, bool* attr_set) {
  if (lds <= 64 * 1024) return hipSuccess;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
  if (dev < 64 && attr_set[dev]) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RASTER_MAX_LDS);
  if (e == hipSuccess && dev < 64) attr_set[dev] = true;
  return e;
}

#endif  // TDR_RASTER_DEV_H_
