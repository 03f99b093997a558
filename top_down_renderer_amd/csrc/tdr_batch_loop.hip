// tdr_batch_loop.hip — the two ends of a batched node loop (tdr_batch_render_polar, tdr_batch_pose; include/tdr.h): the
// polar raster of K clouds, one per renderer, and the pose statistics of K filters, each in one launch set for the whole
// batch.  Like tdr_batch.hip, every kernel reads a table with one entry per renderer / filter (tdr_batch.h) and then does
// exactly what the standalone kernel does for that entry — the arithmetic below is raster_bin's, raster_keys_kernel's and
// raster_kernel's (tdr_raster.hip), mean_cov_kernel's, mc_sums_kernel's, mc_cov_kernel's and mc_final_kernel's
// (tdr_filter.hip) with about == NULL, expression for expression, with the same thread counts and the same reduction
// order: copies, not shared functions, so the existing kernels keep their code.
#include "tdr_common.h"
#include "tdr_atan2f.h"
#include "tdr_sincosf.h"
#include "tdr_batch.h"

// ---- raster ------------------------------------------------------------------------------------------------------------
#define BATCH_RASTER_NO_BIN 0xFFFFFFFFu

__device__ __forceinline__ bool batch_raster_bin(const TdrBatchRasterShape& a, float res, float x, float y, int& row,
                                                 int& col) {
  if (x == 0.f && y == 0.f) return false;
  if (!(fabsf(x) < INFINITY) || !(fabsf(y) < INFINITY)) return false;
  float theta = tdr_atan2f(x, y);
  float r = sqrtf(x * x + y * y);
  row = (int)(roundf(theta / a.ang_res) + (float)(a.rows / 2));
  col = (int)roundf(r / res);
  return row >= 0 && row < a.rows && col >= 0 && col < a.cols;
}

// the cloud whose block range holds block b: the largest k with tab[k].blk_keys <= b
__device__ __forceinline__ int batch_cloud(const TdrBatchRasterEntry* __restrict__ tab, int k, int b) {
  int lo = 0, hi = k - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].blk_keys <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// phase 1 of every cloud: the bin of every point (raster_keys_kernel)
__global__ __launch_bounds__(256) void batch_raster_keys_kernel(const TdrBatchRasterEntry* __restrict__ tab, int k,
                                                                TdrBatchRasterShape a) {
  const TdrBatchRasterEntry& e = tab[batch_cloud(tab, k, (int)blockIdx.x)];
  const int64_t q = (int64_t)(blockIdx.x - e.blk_keys) * blockDim.x + threadIdx.x;
  if (q >= e.n) return;
  const float* p = e.pts + q * e.stride;
  float x, y, cf;
  if (e.stride == 4 && e.ioff == 3) {
    float4 v = *reinterpret_cast<const float4*>(p);
    x = v.x; y = v.y; cf = v.w;
  } else {
    x = p[0]; y = p[1]; cf = p[e.ioff];
  }
  uint32_t key = BATCH_RASTER_NO_BIN;
  int row, col;
  if (batch_raster_bin(a, e.res, x, y, row, col)) {
    const int pc = (cf == cf) ? (int)cf : -1;
    if (pc >= 0 && pc <= 255) {
      const int c = e.lut[pc];
      if (c >= 0 && c < a.ncls) key = ((uint32_t)col << 20) | ((uint32_t)c << 16) | (uint32_t)row;
    }
  }
  e.keys[q] = key;
}

// phase 2: grid (column tiles, clouds); the keyed branch of raster_kernel for cloud blockIdx.y
__global__ __launch_bounds__(1024) void batch_raster_kernel(const TdrBatchRasterEntry* __restrict__ tab,
                                                            TdrBatchRasterShape a) {
  extern __shared__ unsigned int cnt[];  // [cpt][ncls][rows]
  const TdrBatchRasterEntry& e = tab[blockIdx.y];
  const int col0 = blockIdx.x * a.cpt;
  const int ncol = min(a.cpt, a.cols - col0);
  const int tile = ncol * a.ncls * a.rows;
  for (int t = threadIdx.x; t < tile; t += blockDim.x) cnt[t] = 0;
  __syncthreads();
  const int64_t n = e.n;
  const uint32_t* __restrict__ keys = e.keys;
  for (int64_t q = threadIdx.x; q < n; q += blockDim.x) {
    const uint32_t key = keys[q];
    const int col = (int)(key >> 20) - col0;
    if (key == BATCH_RASTER_NO_BIN || col < 0 || col >= ncol) continue;
    atomicAdd(&cnt[(col * a.ncls + (int)((key >> 16) & 15u)) * a.rows + (int)(key & 0xFFFFu)], 1u);
  }
  __syncthreads();
  const int64_t P = (int64_t)a.rows * a.cols;
  float* __restrict__ img = e.img;
  for (int t = threadIdx.x; t < tile; t += blockDim.x) {
    int row = t % a.rows, cc = t / a.rows;
    int c = cc % a.ncls, col = cc / a.ncls;
    img[(int64_t)c * P + row + (int64_t)a.rows * (col0 + col)] = (float)cnt[t];
  }
  float* __restrict__ pk = e.pk;
  const int bins = ncol * a.rows;
  for (int t = threadIdx.x; t < bins; t += blockDim.x) {
    int row = t % a.rows, col = t / a.rows;
    float* o = pk + ((int64_t)(col0 + col) * a.rows + row) * a.rf;
    unsigned int tot = 0;
    for (int c = 0; c < a.ncls; c++) {
      unsigned int v = cnt[(col * a.ncls + c) * a.rows + row];
      o[c] = (float)v;
      tot += v;
    }
    for (int c = a.ncls; c < a.rf - 1; c++) o[c] = 0.f;
    if (tdr_has_kslot(a.ncls, a.rf)) o[a.rf - 2] = 1.f;
    o[a.rf - 1] = (float)tot;
  }
}

// the launch shape launch_raster (tdr_raster.hip) chooses for this image shape; false for shapes it rasterises without
// keys (those take tdr_k_raster_polar per renderer) or refuses
bool tdr_batch_raster_shape(int ncls, int rows, int cols, float ang_res, TdrBatchRasterShape* out) {
  const int64_t per_col = (int64_t)ncls * rows * 4;
  if (ncls < 1 || ncls > TDR_MAX_CLASSES || rows < 1 || cols < 1 || per_col > 152 * 1024) return false;
  if (cols > TDR_BATCH_RASTER_KEY_MAX_COLS || rows > TDR_BATCH_RASTER_KEY_MAX_ROWS) return false;
  TdrBatchRasterShape a;
  a.ang_res = ang_res; a.ncls = ncls; a.rows = rows; a.cols = cols; a.rf = tdr_rec_floats(ncls);
  a.cpt = (int)std::max<int64_t>(1, (64 * 1024) / per_col);
  a.cpt = std::min(a.cpt, cols);
  while (a.cpt > 1 && cdiv(cols, a.cpt) < 32) a.cpt = (a.cpt + 1) / 2;
  *out = a;
  return true;
}

int tdr_batch_raster(const TdrBatchRasterEntry* tab, int k, int blocks_keys, const TdrBatchRasterShape& a, hipStream_t s) {
  if (!tab || k < 1 || blocks_keys < 0) return fail(TDR_ERR_ARG, "batch_raster: bad arguments");
  const size_t lds = (size_t)a.cpt * a.ncls * a.rows * 4;
  if (lds > 64 * 1024) {   // (as launch_raster: one column of more than 64 KB)
    static bool attr_set[64] = {false};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    if (dev >= 64 || !attr_set[dev]) {
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(batch_raster_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
      if (dev < 64) attr_set[dev] = true;
    }
  }
  if (blocks_keys > 0)
    hipLaunchKernelGGL(batch_raster_keys_kernel, dim3((unsigned)blocks_keys), dim3(256), 0, s, tab, k, a);
  hipLaunchKernelGGL(batch_raster_kernel, dim3((unsigned)cdiv(a.cols, a.cpt), (unsigned)k), dim3(1024), lds, s, tab, a);
  LAUNCH_CHECK("batch_raster");
  return TDR_OK;
}

// ---- pose statistics ---------------------------------------------------------------------------------------------------
// block_sum_d (tdr_filter.hip)
__device__ double batch_block_sum_d(double v, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  double t = 0;
  const int nw = blockDim.x >> 6;
  for (int w = 0; w < nw; w++) t += sh[w];
  return t;
}

#define BMC_WGS 128          // MC_WGS
#define BMC_THREADS 256      // MC_THREADS
struct BatchMcScratch {      // McScratch
  double sums[BMC_WGS][8];
  double mom[BMC_WGS][10];
};
static_assert(24 * 4 + sizeof(BatchMcScratch) <= TDR_MEAN_COV_FLOATS * 4, "TDR_MEAN_COV_FLOATS too small");

// the entry's result record: [0, 24) what tdr_k_mean_cov writes, [24] the scale of particle 0 (tdr_filter_scale)
__device__ __forceinline__ void batch_pose_scale(const TdrBatchPoseEntry& e) {
  e.out[24] = e.st[TDR_ST_SCALE * e.cap];
}

// mean_cov_kernel with about == NULL, one workgroup per filter of at most TDR_BATCH_MC_SINGLE_MAX_N particles
__global__ __launch_bounds__(1024) void batch_mean_cov_kernel(const TdrBatchPoseEntry* __restrict__ tab, int libm_fma) {
  __shared__ double shd[16];
  __shared__ float ref[4];
  const TdrBatchPoseEntry& e = tab[blockIdx.x];
  const float* __restrict__ st = e.st;
  const int64_t cap = e.cap, n = e.n;
  float* __restrict__ out = e.out;
  const int tid = threadIdx.x, nt = blockDim.x;
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int64_t p = tid; p < n; p += nt) {
    const float sc = st[TDR_ST_SCALE * cap + p];
    const float x = st[TDR_ST_DX * cap + p] * sc + st[TDR_ST_INIT_X * cap + p];
    const float y = st[TDR_ST_DY * cap + p] * sc + st[TDR_ST_INIT_Y * cap + p];
    const float th = st[TDR_ST_THETA * cap + p];
    acc[0] += x; acc[1] += y; acc[2] += th; acc[3] += sc;
    acc[4] += (double)tdr_libm::cosf_v(th, libm_fma); acc[5] += (double)tdr_libm::sinf_v(th, libm_fma);
    acc[6] += log((double)sc);
  }
  double tot[7];
  for (int k = 0; k < 7; k++) tot[k] = batch_block_sum_d(acc[k], shd);
  if (tid == 0) {
    const float fn = (float)n;
    float mean[4];
    mean[0] = (float)tot[0] / fn; mean[1] = (float)tot[1] / fn; mean[3] = (float)tot[3] / fn;
    mean[2] = atan2f((float)tot[5] / fn, (float)tot[4] / fn);
    for (int k = 0; k < 4; k++) out[k] = mean[k];
    out[20] = (float)exp(tot[6] / (double)n);
    out[21] = out[22] = out[23] = 0.f;
    for (int k = 0; k < 4; k++) ref[k] = mean[k];
    batch_pose_scale(e);
  }
  __syncthreads();
  double c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t p = tid; p < n; p += nt) {
    const float sc = st[TDR_ST_SCALE * cap + p];
    float d[4];
    d[0] = (st[TDR_ST_DX * cap + p] * sc + st[TDR_ST_INIT_X * cap + p]) - ref[0];
    d[1] = (st[TDR_ST_DY * cap + p] * sc + st[TDR_ST_INIT_Y * cap + p]) - ref[1];
    d[2] = st[TDR_ST_THETA * cap + p] - ref[2];
    d[3] = sc - ref[3];
    while (d[2] > M_PI) d[2] = (float)((double)d[2] - 2 * M_PI);
    while (d[2] < -M_PI) d[2] = (float)((double)d[2] + 2 * M_PI);
    int k = 0;
    for (int a = 0; a < 4; a++)
      for (int b = a; b < 4; b++) c[k++] += (double)(d[a] * d[b]);
  }
  double ct[10];
  for (int k = 0; k < 10; k++) ct[k] = batch_block_sum_d(c[k], shd);
  if (tid == 0) {
    int k = 0;
    for (int a = 0; a < 4; a++)
      for (int b = a; b < 4; b++) {
        float v = (float)ct[k++] / (float)(n - 1);
        out[4 + 4 * a + b] = v;
        out[4 + 4 * b + a] = v;
      }
  }
}

// larger filters: grid.y = filter, BMC_WGS workgroups each, the partial sums in the filter's own scratch
__global__ __launch_bounds__(BMC_THREADS) void batch_mc_sums_kernel(const TdrBatchPoseEntry* __restrict__ tab, int libm_fma) {
  __shared__ double shd[16];
  const TdrBatchPoseEntry& e = tab[blockIdx.y];
  const float* __restrict__ st = e.st;
  const int64_t cap = e.cap, n = e.n;
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int64_t p = (int64_t)blockIdx.x * BMC_THREADS + threadIdx.x; p < n; p += (int64_t)BMC_WGS * BMC_THREADS) {
    const float sc = st[TDR_ST_SCALE * cap + p];
    const float x = st[TDR_ST_DX * cap + p] * sc + st[TDR_ST_INIT_X * cap + p];
    const float y = st[TDR_ST_DY * cap + p] * sc + st[TDR_ST_INIT_Y * cap + p];
    const float th = st[TDR_ST_THETA * cap + p];
    acc[0] += x; acc[1] += y; acc[2] += th; acc[3] += sc;
    acc[4] += (double)tdr_libm::cosf_v(th, libm_fma); acc[5] += (double)tdr_libm::sinf_v(th, libm_fma);
    acc[6] += log((double)sc);
  }
  BatchMcScratch* sc = reinterpret_cast<BatchMcScratch*>(e.scratch);
  for (int k = 0; k < 7; k++) {
    const double t = batch_block_sum_d(acc[k], shd);
    if (threadIdx.x == 0) sc->sums[blockIdx.x][k] = t;
  }
}
// mc_means with about == NULL
__device__ __forceinline__ void batch_mc_means(const BatchMcScratch* sc, int64_t n, double* stage, double* sh,
                                               float mean[4], float ref[4], float& geo) {
  __syncthreads();
  for (int t = threadIdx.x; t < BMC_WGS * 8; t += BMC_THREADS) stage[t] = (&sc->sums[0][0])[t];
  __syncthreads();
  if (threadIdx.x < 7) {
    double t = 0;
    for (int g = 0; g < BMC_WGS; g++) t += stage[g * 8 + threadIdx.x];
    sh[threadIdx.x] = t;
  }
  __syncthreads();
  const float fn = (float)n;
  mean[0] = (float)sh[0] / fn; mean[1] = (float)sh[1] / fn; mean[3] = (float)sh[3] / fn;
  mean[2] = atan2f((float)sh[5] / fn, (float)sh[4] / fn);
  geo = (float)exp(sh[6] / (double)n);
  for (int k = 0; k < 4; k++) ref[k] = mean[k];
}
__global__ __launch_bounds__(BMC_THREADS) void batch_mc_cov_kernel(const TdrBatchPoseEntry* __restrict__ tab) {
  __shared__ double shd[16];
  __shared__ double shm[8];
  __shared__ double stage[BMC_WGS * 10];
  const TdrBatchPoseEntry& e = tab[blockIdx.y];
  const float* __restrict__ st = e.st;
  const int64_t cap = e.cap, n = e.n;
  BatchMcScratch* sc = reinterpret_cast<BatchMcScratch*>(e.scratch);
  float mean[4], ref[4], geo;
  batch_mc_means(sc, n, stage, shm, mean, ref, geo);
  double c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t p = (int64_t)blockIdx.x * BMC_THREADS + threadIdx.x; p < n; p += (int64_t)BMC_WGS * BMC_THREADS) {
    const float s = st[TDR_ST_SCALE * cap + p];
    float d[4];
    d[0] = (st[TDR_ST_DX * cap + p] * s + st[TDR_ST_INIT_X * cap + p]) - ref[0];
    d[1] = (st[TDR_ST_DY * cap + p] * s + st[TDR_ST_INIT_Y * cap + p]) - ref[1];
    d[2] = st[TDR_ST_THETA * cap + p] - ref[2];
    d[3] = s - ref[3];
    while (d[2] > M_PI) d[2] = (float)((double)d[2] - 2 * M_PI);
    while (d[2] < -M_PI) d[2] = (float)((double)d[2] + 2 * M_PI);
    int k = 0;
    for (int a = 0; a < 4; a++)
      for (int b = a; b < 4; b++) c[k++] += (double)(d[a] * d[b]);
  }
  for (int k = 0; k < 10; k++) {
    const double t = batch_block_sum_d(c[k], shd);
    if (threadIdx.x == 0) sc->mom[blockIdx.x][k] = t;
  }
}
__global__ __launch_bounds__(BMC_THREADS) void batch_mc_final_kernel(const TdrBatchPoseEntry* __restrict__ tab) {
  __shared__ double shm[8];
  __shared__ double shc[10];
  __shared__ double stage[BMC_WGS * 10];
  const TdrBatchPoseEntry& e = tab[blockIdx.x];
  const int64_t n = e.n;
  float* __restrict__ out = e.out;
  const BatchMcScratch* sc = reinterpret_cast<const BatchMcScratch*>(e.scratch);
  float mean[4], ref[4], geo;
  batch_mc_means(sc, n, stage, shm, mean, ref, geo);
  __syncthreads();
  for (int t = threadIdx.x; t < BMC_WGS * 10; t += BMC_THREADS) stage[t] = (&sc->mom[0][0])[t];
  __syncthreads();
  if (threadIdx.x < 10) {
    double t = 0;
    for (int g = 0; g < BMC_WGS; g++) t += stage[g * 10 + threadIdx.x];
    shc[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 0; k < 4; k++) out[k] = mean[k];
    out[20] = geo;
    out[21] = out[22] = out[23] = 0.f;
    int k = 0;
    for (int a = 0; a < 4; a++)
      for (int b = a; b < 4; b++) {
        const float v = (float)shc[k++] / (float)(n - 1);
        out[4 + 4 * a + b] = v;
        out[4 + 4 * b + a] = v;
      }
    batch_pose_scale(e);
  }
}

int tdr_batch_pose_launch(const TdrBatchPoseEntry* small, int k_small, const TdrBatchPoseEntry* big, int k_big,
                          hipStream_t s) {
  if (k_small < 0 || k_big < 0 || (k_small && !small) || (k_big && !big)) return fail(TDR_ERR_ARG, "batch_pose: bad arguments");
  const int fma = tdr_libm_fma();
  if (k_small > 0)
    hipLaunchKernelGGL(batch_mean_cov_kernel, dim3((unsigned)k_small), dim3(1024), 0, s, small, fma);
  if (k_big > 0) {
    hipLaunchKernelGGL(batch_mc_sums_kernel, dim3(BMC_WGS, (unsigned)k_big), dim3(BMC_THREADS), 0, s, big, fma);
    hipLaunchKernelGGL(batch_mc_cov_kernel, dim3(BMC_WGS, (unsigned)k_big), dim3(BMC_THREADS), 0, s, big);
    hipLaunchKernelGGL(batch_mc_final_kernel, dim3((unsigned)k_big), dim3(BMC_THREADS), 0, s, big);
  }
  LAUNCH_CHECK("batch_pose");
  return TDR_OK;
}
