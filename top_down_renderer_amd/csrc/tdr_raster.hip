// tdr_raster.hip — scan raster (polar and Cartesian) and the packed scan records.
#include "tdr_common.h"
#include "tdr_raster_dev.h"

// ------------------------------------------------------------------------------------------------------------------
// K1: scan raster.  Each workgroup owns a tile of `cpt` image columns (range bins) x all rows x all classes as u32
// counters in LDS, streams every point with coalesced loads and keeps those that fall into its tile.  Integer LDS
// atomics -> exact, order-independent counts; plain coalesced stores out (the tile is written whole, zeros
// included, so no memset pass is needed).
struct RasterArgs {
  const float* pts;
  int stride, ioff;
  int64_t n;
  float res, ang_res;
  const int32_t* lut;
  int ncls, rows, cols, rf, cpt, polar;
  float* img;
  float* pk;
  uint32_t* keys;   // optional [n]: bin of every point, computed once by raster_keys_kernel (col << 20 | class << 16 | row)
};
// Phase 1 (when the caller gave a workspace): the bin of every point once — atan2f / sqrtf per point instead of per
// point and tile — as a 4-byte key the tiles then stream.
__global__ __launch_bounds__(256) void raster_keys_kernel(RasterArgs a) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.n) return;
  a.keys[k] = raster_key(a.pts, a.stride, a.ioff, k, a.polar, a.res, a.ang_res, a.lut, a.ncls, a.rows, a.cols);
}

__global__ __launch_bounds__(1024) void raster_kernel(RasterArgs a) {
  extern __shared__ unsigned int cnt[];  // [cpt][ncls][rows]
  const int col0 = blockIdx.x * a.cpt;
  const int ncol = min(a.cpt, a.cols - col0);
  raster_tile_clear(cnt, ncol * a.ncls * a.rows);
  __shared__ int lut_s[256];
  if (threadIdx.x < 256) lut_s[threadIdx.x] = a.lut[threadIdx.x];
  __syncthreads();
  if (a.keys) {
    raster_tile_count_keys(cnt, a.keys, a.n, col0, ncol, a.ncls, a.rows);
  } else
  for (int64_t k = threadIdx.x; k < a.n; k += blockDim.x) {
    float x, y, cf;
    raster_point(a.pts, a.stride, a.ioff, k, x, y, cf);
    int row, col;
    if (!raster_bin(a.polar, a.res, a.ang_res, a.rows, a.cols, x, y, row, col)) continue;
    col -= col0;
    if (col < 0 || col >= ncol) continue;
    const int c = raster_class(lut_s, a.ncls, cf);
    if (c < 0) continue;
    atomicAdd(&cnt[(col * a.ncls + c) * a.rows + row], 1u);
  }
  __syncthreads();
  raster_tile_write(cnt, col0, ncol, a.ncls, a.rows, a.cols, a.rf, a.img, a.pk);
}

extern "C" int64_t tdr_raster_workspace_bytes(int64_t n) { return n < 1 ? 0 : 4 * n; }
static int launch_raster(const float* pts, int stride, int ioff, int64_t n, float res, float ang_res,
                         const int32_t* lut, int ncls, int rows, int cols, int polar, float* img, float* pk,
                         void* workspace, void* stream) {
  if (ncls < 1 || ncls > TDR_MAX_CLASSES || rows < 1 || cols < 1) return fail(TDR_ERR_ARG, "raster: bad image shape");
  if (n < 0 || (n > 0 && !pts) || !lut) return fail(TDR_ERR_ARG, "raster: null points / lut");
  if (stride < 3 || ioff < 0 || ioff >= stride) return fail(TDR_ERR_ARG, "raster: bad point stride / offset");
  if (!(res > 0.f) || (polar && !(ang_res > 0.f))) return fail(TDR_ERR_ARG, "raster: resolution must be > 0");
  RasterShape sh;
  if (!raster_shape(ncls, rows, cols, workspace && n > 0, &sh)) return fail(TDR_ERR_ARG, "raster: ncls*rows too large for one LDS tile (152 KB)");
  RasterArgs a;
  a.pts = pts; a.stride = stride; a.ioff = ioff; a.n = n; a.res = res; a.ang_res = ang_res; a.lut = lut;
  a.ncls = ncls; a.rows = rows; a.cols = cols; a.rf = tdr_rec_floats(ncls); a.polar = polar; a.img = img; a.pk = pk;
  a.cpt = sh.cpt;
  static bool attr_set[64] = {false};
  HIP_TRY(raster_allow_lds(reinterpret_cast<const void*>(raster_kernel), sh.lds, attr_set));
  a.keys = nullptr;
  if (workspace && n > 0 && sh.keyed) {
    a.keys = reinterpret_cast<uint32_t*>(workspace);
    hipLaunchKernelGGL(raster_keys_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, a);
  }
  hipLaunchKernelGGL(raster_kernel, dim3((unsigned)cdiv(cols, a.cpt)), dim3(1024), sh.lds, (hipStream_t)stream, a);
  LAUNCH_CHECK("raster");
  return TDR_OK;
}

extern "C" int tdr_k_raster_polar(const float* pts, int stride, int ioff, int64_t n, float res, float ang_res,
                                  const int32_t* lut256, int ncls, int nb, int nr, float* img_out, float* pk_out,
                                  void* workspace, void* stream) {
  return launch_raster(pts, stride, ioff, n, res, ang_res, lut256, ncls, nb, nr, 1, img_out, pk_out, workspace, stream);
}
extern "C" int tdr_k_raster_cart(const float* pts, int stride, int ioff, int64_t n, float res, const int32_t* lut256,
                                 int ncls, int rows, int cols, float* img_out, float* pk_out, void* workspace,
                                 void* stream) {
  return launch_raster(pts, stride, ioff, n, res, 1.f, lut256, ncls, rows, cols, 0, img_out, pk_out, workspace, stream);
}

__global__ void pack_scan_kernel(const float* __restrict__ img, int ncls, int rows, int cols, int rf,
                                 float* __restrict__ pk) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t P = (int64_t)rows * cols;
  if (t >= P) return;
  float* o = pk + t * rf;  // t = row + rows*col == (col*rows + row)
  float tot = 0.f;
  for (int c = 0; c < ncls; c++) {
    float v = img[(int64_t)c * P + t];
    o[c] = v;
    tot += v;
  }
  for (int c = ncls; c < rf - 1; c++) o[c] = 0.f;
  if (tdr_has_kslot(ncls, rf)) o[rf - 2] = 1.f;
  o[rf - 1] = tot;
}
extern "C" int tdr_k_pack_scan(const float* img, int ncls, int nb, int nr, float* pk_out, void* stream) {
  if (!img || !pk_out || ncls < 1 || ncls > TDR_MAX_CLASSES || nb < 1 || nr < 1)
    return fail(TDR_ERR_ARG, "pack_scan: bad arguments");
  int64_t P = (int64_t)nb * nr;
  hipLaunchKernelGGL(pack_scan_kernel, dim3((unsigned)cdiv(P, 256)), dim3(256), 0, (hipStream_t)stream, img, ncls, nb,
                     nr, tdr_rec_floats(ncls), pk_out);
  LAUNCH_CHECK("pack_scan");
  return TDR_OK;
}

__global__ void selftest_atan2_kernel(const float* __restrict__ y, const float* __restrict__ x, int64_t n,
                                      float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = tdr_atan2f(y[i], x[i]);
}
extern "C" int tdr_k_selftest_atan2(const float* y, const float* x, int64_t n, float* out, void* stream) {
  if (!y || !x || !out || n < 1) return fail(TDR_ERR_ARG, "selftest_atan2: bad arguments");
  hipLaunchKernelGGL(selftest_atan2_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, y, x, n, out);
  LAUNCH_CHECK("selftest_atan2");
  return TDR_OK;
}
