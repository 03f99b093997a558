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
// one key against the tile: an integer LDS atomic (exact, order-free)
__device__ __forceinline__ void raster_tile_count_key(unsigned int* cnt, uint32_t key, int col0, int ncol, int ncls,
                                                      int rows) {
  const int col = (int)(key >> 20) - col0;
  if (key == RASTER_NO_BIN || col < 0 || col >= ncol) return;
  atomicAdd(&cnt[(col * ncls + (int)((key >> 16) & 15u)) * rows + (int)(key & 0xFFFFu)], 1u);
}
// Every thread of every tile walks all n keys, so the walk is bound by load latency, not by bytes: the keys are read as
// 16-byte vectors, RASTER_KEY_VECS of them in flight per thread, behind a scalar head up to the first 16-byte boundary
// (the workspace need only be 4-byte aligned) and in front of a scalar tail.
#define RASTER_KEY_VECS 4
__device__ __forceinline__ void raster_tile_count_keys(unsigned int* cnt, const uint32_t* __restrict__ keys, int64_t n,
                                                       int col0, int ncol, int ncls, int rows) {
  const int64_t to16 = (int64_t)((4u - (unsigned)((reinterpret_cast<uintptr_t>(keys) >> 2) & 3u)) & 3u);
  const int64_t head = to16 < n ? to16 : n;
  const int64_t nv = (n - head) >> 2;
  if ((int64_t)threadIdx.x < head) raster_tile_count_key(cnt, keys[threadIdx.x], col0, ncol, ncls, rows);
  const uint4* __restrict__ kv = reinterpret_cast<const uint4*>(keys + head);
  for (int64_t q = threadIdx.x; q < nv; q += (int64_t)RASTER_KEY_VECS * blockDim.x) {
    uint4 v[RASTER_KEY_VECS];
#pragma unroll
    for (int u = 0; u < RASTER_KEY_VECS; u++) {
      const int64_t qu = q + (int64_t)u * blockDim.x;
      v[u] = qu < nv ? kv[qu] : make_uint4(RASTER_NO_BIN, RASTER_NO_BIN, RASTER_NO_BIN, RASTER_NO_BIN);
    }
#pragma unroll
    for (int u = 0; u < RASTER_KEY_VECS; u++) {
      raster_tile_count_key(cnt, v[u].x, col0, ncol, ncls, rows);
      raster_tile_count_key(cnt, v[u].y, col0, ncol, ncls, rows);
      raster_tile_count_key(cnt, v[u].z, col0, ncol, ncls, rows);
      raster_tile_count_key(cnt, v[u].w, col0, ncol, ncls, rows);
    }
  }
  const int64_t tail = head + 4 * nv + threadIdx.x;   // at most three keys
  if (tail < n) raster_tile_count_key(cnt, keys[tail], col0, ncol, ncls, rows);
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
// tiles the keyed form asks for: a workgroup per CU of an MI355X (256 CUs) — a constant, not queried from the device, so
// that an image's tiles, like its bits, do not depend on the card; fewer CUs run the tiles in rounds
#define RASTER_KEYED_TILES 256
// false: one image column does not fit an LDS tile.  with_keys: the shape of the keyed form (a key workspace and
// out->keyed) — a tile there costs one more walk over the 4-byte keys and no arithmetic, so the image is cut into a tile
// per CU where it has the columns; without keys every tile computes every point's bin again, and 32 tiles stay enough.
static inline bool raster_shape(int ncls, int rows, int cols, bool with_keys, RasterShape* out) {
  const int64_t per_col = (int64_t)ncls * rows * 4;
  if (per_col > RASTER_MAX_LDS) return false;
  out->keyed = cols <= RASTER_KEY_MAX_COLS && rows <= RASTER_KEY_MAX_ROWS;
  int cpt = (int)std::max<int64_t>(1, (64 * 1024) / per_col);
  cpt = std::min(cpt, cols);
  // enough workgroups to spread over the chip when the image is small
  const int want = (with_keys && out->keyed) ? RASTER_KEYED_TILES : 32;
  while (cpt > 1 && cdiv(cols, cpt) < want) cpt = (cpt + 1) / 2;
  out->cpt = cpt;
  out->lds = (size_t)cpt * per_col;
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
