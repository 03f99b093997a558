// tdr_batch_loop.hip — the two ends of a batched node loop (tdr_batch_render_polar, tdr_batch_pose; include/tdr.h): the
// polar raster of K clouds, one per renderer, and the pose statistics of K filters, each in one launch set for the whole
// batch.  Like tdr_batch.hip, every kernel reads a table with one entry per renderer / filter (tdr_batch.h) and then calls
// the body the standalone kernel calls for that entry — the raster bodies and the launch-shape rule of tdr_raster_dev.h,
// the pose-statistics bodies of tdr_filter_dev.h with about == NULL — with the same thread counts and the same reduction
// order, so every renderer and filter ends bit for bit where its standalone calls leave it.
#include "tdr_common.h"
#include "tdr_raster_dev.h"
#include "tdr_filter_dev.h"
#include "tdr_batch.h"

// ---- raster ------------------------------------------------------------------------------------------------------------
// phase 1 of every cloud: the bin of every point (raster_keys_kernel)
__global__ __launch_bounds__(256) void batch_raster_keys_kernel(const TdrBatchRasterEntry* __restrict__ tab, int k,
                                                                TdrBatchRasterShape a) {
  const TdrBatchRasterEntry& e = tab[batch_find(k, (int)blockIdx.x, [&](int i) { return tab[i].blk_keys; })];
  const int64_t q = (int64_t)(blockIdx.x - e.blk_keys) * blockDim.x + threadIdx.x;
  if (q >= e.n) return;
  e.keys[q] = raster_key(e.pts, e.stride, e.ioff, q, 1, e.res, a.ang_res, e.lut, a.ncls, a.rows, a.cols);
}

// phase 2: grid (column tiles, clouds); the keyed branch of raster_kernel for cloud blockIdx.y
__global__ __launch_bounds__(1024) void batch_raster_kernel(const TdrBatchRasterEntry* __restrict__ tab,
                                                            TdrBatchRasterShape a) {
  extern __shared__ unsigned int cnt[];  // [cpt][ncls][rows]
  const TdrBatchRasterEntry& e = tab[blockIdx.y];
  const int col0 = blockIdx.x * a.cpt;
  const int ncol = min(a.cpt, a.cols - col0);
  raster_tile_clear(cnt, ncol * a.ncls * a.rows);
  __syncthreads();
  raster_tile_count_keys(cnt, e.keys, e.n, col0, ncol, a.ncls, a.rows);
  __syncthreads();
  raster_tile_write(cnt, col0, ncol, a.ncls, a.rows, a.cols, a.rf, e.img, e.pk);
}

// the launch shape of this image shape (raster_shape, as launch_raster takes it); false for shapes launch_raster
// rasterises without keys (those take tdr_k_raster_polar per renderer) or refuses
bool tdr_batch_raster_shape(int ncls, int rows, int cols, float ang_res, TdrBatchRasterShape* out) {
  RasterShape sh;
  if (ncls < 1 || ncls > TDR_MAX_CLASSES || rows < 1 || cols < 1 || !raster_shape(ncls, rows, cols, true, &sh) || !sh.keyed)
    return false;
  TdrBatchRasterShape a;
  a.ang_res = ang_res; a.ncls = ncls; a.rows = rows; a.cols = cols; a.rf = tdr_rec_floats(ncls); a.cpt = sh.cpt;
  *out = a;
  return true;
}

int tdr_batch_raster(const TdrBatchRasterEntry* tab, int k, int blocks_keys, const TdrBatchRasterShape& a, hipStream_t s) {
  if (!tab || k < 1 || blocks_keys < 0) return fail(TDR_ERR_ARG, "batch_raster: bad arguments");
  const size_t lds = (size_t)a.cpt * a.ncls * a.rows * 4;
  static bool attr_set[64] = {false};
  HIP_TRY(raster_allow_lds(reinterpret_cast<const void*>(batch_raster_kernel), lds, attr_set));
  if (blocks_keys > 0)
    hipLaunchKernelGGL(batch_raster_keys_kernel, dim3((unsigned)blocks_keys), dim3(256), 0, s, tab, k, a);
  hipLaunchKernelGGL(batch_raster_kernel, dim3((unsigned)cdiv(a.cols, a.cpt), (unsigned)k), dim3(1024), lds, s, tab, a);
  LAUNCH_CHECK("batch_raster");
  return TDR_OK;
}

// ---- pose statistics ---------------------------------------------------------------------------------------------------
static_assert(TDR_BATCH_MC_SINGLE_MAX_N == MC_SINGLE_MAX_N, "the batch splits small / big filters where tdr_k_mean_cov does");
// the entry's result record: [0, 24) what tdr_k_mean_cov writes, [24] the scale of particle 0 (tdr_filter_scale)

// mean_cov_kernel with about == NULL, one workgroup per filter of at most TDR_BATCH_MC_SINGLE_MAX_N particles
__global__ __launch_bounds__(1024) void batch_mean_cov_kernel(const TdrBatchPoseEntry* __restrict__ tab, int libm_fma) {
  const TdrBatchPoseEntry& e = tab[blockIdx.x];
  mean_cov_body(e.st, e.cap, e.n, nullptr, e.out, libm_fma);
  if (threadIdx.x == 0) e.out[24] = e.st[TDR_ST_SCALE * e.cap];
}
// larger filters: grid.y = filter, MC_WGS workgroups each, the partial sums in the filter's own scratch
__global__ __launch_bounds__(MC_THREADS) void batch_mc_sums_kernel(const TdrBatchPoseEntry* __restrict__ tab, int libm_fma) {
  const TdrBatchPoseEntry& e = tab[blockIdx.y];
  mc_sums_body(e.st, e.cap, e.n, reinterpret_cast<McScratch*>(e.scratch), libm_fma);
}
__global__ __launch_bounds__(MC_THREADS) void batch_mc_cov_kernel(const TdrBatchPoseEntry* __restrict__ tab) {
  const TdrBatchPoseEntry& e = tab[blockIdx.y];
  mc_cov_body(e.st, e.cap, e.n, nullptr, reinterpret_cast<McScratch*>(e.scratch));
}
__global__ __launch_bounds__(MC_THREADS) void batch_mc_final_kernel(const TdrBatchPoseEntry* __restrict__ tab) {
  const TdrBatchPoseEntry& e = tab[blockIdx.x];
  mc_final_body(e.n, nullptr, reinterpret_cast<const McScratch*>(e.scratch), e.out);
  if (threadIdx.x == 0) e.out[24] = e.st[TDR_ST_SCALE * e.cap];
}

int tdr_batch_pose_launch(const TdrBatchPoseEntry* small, int k_small, const TdrBatchPoseEntry* big, int k_big,
                          hipStream_t s) {
  if (k_small < 0 || k_big < 0 || (k_small && !small) || (k_big && !big)) return fail(TDR_ERR_ARG, "batch_pose: bad arguments");
  const int fma = tdr_libm_fma();
  if (k_small > 0)
    hipLaunchKernelGGL(batch_mean_cov_kernel, dim3((unsigned)k_small), dim3(1024), 0, s, small, fma);
  if (k_big > 0) {
    hipLaunchKernelGGL(batch_mc_sums_kernel, dim3(MC_WGS, (unsigned)k_big), dim3(MC_THREADS), 0, s, big, fma);
    hipLaunchKernelGGL(batch_mc_cov_kernel, dim3(MC_WGS, (unsigned)k_big), dim3(MC_THREADS), 0, s, big);
    hipLaunchKernelGGL(batch_mc_final_kernel, dim3((unsigned)k_big), dim3(MC_THREADS), 0, s, big);
  }
  LAUNCH_CHECK("batch_pose");
  return TDR_OK;
}
