// tdr_batch.hip — batched filter step (tdr_batch_step, include/tdr.h): the per-particle stages of many filters that share
// one map in one launch each.  Every kernel reads a table with one entry per filter (tdr_batch.h); a workgroup finds its
// filter from its block index and then does exactly what the standalone kernel does for that filter, with that filter's
// pointers and scalars — the arithmetic below is propagate_kernel's (z4 path), resample_dev_kernel's, gather_states_kernel's
// and save_ml_state_kernel's (tdr_filter.hip), expression for expression, so each filter ends bit for bit where its
// standalone calls leave it.
#include "tdr_common.h"
#include "tdr_sincosf.h"
#include "tdr_batch.h"

// the entry whose block range holds block b: the largest k with tab[k].blk <= b (ranges are non-empty and ascending)
template <bool PROP>
__device__ __forceinline__ int batch_entry(const TdrBatchEntry* __restrict__ tab, int k, int b) {
  int lo = 0, hi = k - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((PROP ? tab[mid].blk_prop : tab[mid].blk_res) <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// StateParticle::propagate (state_particle.cpp:57-78) of every particle of every filter; the normals come from each
// filter's own generator (parity mode), so the mt19937 streams stay per filter
__global__ __launch_bounds__(TDR_BATCH_THREADS) void batch_propagate_kernel(const TdrBatchEntry* __restrict__ tab, int k,
                                                                            int libm_fma) {
  const int e = batch_entry<true>(tab, k, (int)blockIdx.x);
  const TdrBatchEntry& f = tab[e];
  const int64_t p = (int64_t)(blockIdx.x - f.blk_prop) * blockDim.x + threadIdx.x;
  if (p >= f.n) return;
  float* __restrict__ st = f.st;
  const int64_t cap = f.cap;
  const float* __restrict__ z4 = f.z4;
  const float tx = f.tx, ty = f.ty, omega = f.omega, pos_cov = f.pos_cov, theta_cov = f.theta_cov;
  float z[4];
  z[0] = z4[4 * p]; z[1] = z4[4 * p + 1]; z[2] = z4[4 * p + 2]; z[3] = z4[4 * p + 3];
  float theta = st[TDR_ST_THETA * cap + p];
  float dx = st[TDR_ST_DX * cap + p], dy = st[TDR_ST_DY * cap + p];
  const float c = tdr_libm::cosf_v(theta, libm_fma), s = tdr_libm::sinf_v(theta, libm_fma);
  const float gx = c * tx + (-s) * ty;
  const float gy = s * tx + c * ty;
  const float lx = dx, ly = dy;
  dx += gx;
  dy += gy;
  const float dist = sqrtf(gx * gx + gy * gy);
  const float sd_pos = pos_cov * dist, sd_th = theta_cov * dist;
  theta += (z[0] * sd_th + 0.f) + omega;
  dx += z[1] * sd_pos + 0.f;
  dy += z[2] * sd_pos + 0.f;
  if (!f.scale_freeze) {
    const float sd_s = (float)fmin(2. / (double)dist, 0.02);
    float scale = st[TDR_ST_SCALE * cap + p];
    scale *= z[3] * sd_s + 1.f;
    st[TDR_ST_SCALE * cap + p] = scale;
  }
  st[TDR_ST_THETA * cap + p] = theta;
  st[TDR_ST_DX * cap + p] = dx;
  st[TDR_ST_DY * cap + p] = dy;
  const float mx = lx - dx, my = ly - dy;
  f.last_dist[p] = sqrtf(mx * mx + my * my);
}

// the systematic resample (particle_filter.cpp:171-185) of every filter: the search over the running maximum with the
// filter's own device uniform, the gather of the chosen states into st_new, and — thread 0 of each filter — the
// pre-resample max-likelihood particle (:145-147)
__global__ __launch_bounds__(TDR_BATCH_THREADS) void batch_resample_kernel(const TdrBatchEntry* __restrict__ tab, int k) {
  const int e = batch_entry<false>(tab, k, (int)blockIdx.x);
  const TdrBatchEntry& f = tab[e];
  const int64_t i = (int64_t)(blockIdx.x - f.blk_res) * blockDim.x + threadIdx.x;
  if (i >= f.n_new) return;
  const int64_t n = f.n, cap = f.cap;
  const float* __restrict__ runmax = f.runmax;
  const float* __restrict__ st = f.st;
  if (i == 0) {
    int64_t best = (int64_t)__float_as_int(f.info[0]);
    if (best < 0 || best >= n) best = 0;
    float v[TDR_ST_FIELDS];
#pragma unroll
    for (int q = 0; q < TDR_ST_FIELDS; q++) { v[q] = st[(int64_t)q * cap + best]; f.ml[q] = v[q]; }
    f.ml[7] = 0.f;
    f.ml[8] = v[TDR_ST_DX] * v[TDR_ST_SCALE] + v[TDR_ST_INIT_X];
    f.ml[9] = v[TDR_ST_DY] * v[TDR_ST_SCALE] + v[TDR_ST_INIT_Y];
    f.ml[10] = v[TDR_ST_THETA];
    f.ml[11] = v[TDR_ST_SCALE];
  }
  const float sample = ((float)i + *f.shift) / (float)f.n_new;  // particle_filter.cpp:176
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (runmax[mid] > sample) hi = mid; else lo = mid + 1;
  }
  f.idx[i] = (int32_t)lo;
#pragma unroll
  for (int q = 0; q < TDR_ST_FIELDS; q++) f.st_new[q * cap + i] = st[q * cap + lo];
}

int tdr_batch_propagate(const TdrBatchEntry* tab, int k, int blocks_prop, hipStream_t s) {
  if (!tab || k < 1 || blocks_prop < 1) return fail(TDR_ERR_ARG, "batch_propagate: bad arguments");
  hipLaunchKernelGGL(batch_propagate_kernel, dim3((unsigned)blocks_prop), dim3(TDR_BATCH_THREADS), 0, s, tab, k,
                     tdr_libm_fma());
  LAUNCH_CHECK("batch_propagate");
  return TDR_OK;
}
int tdr_batch_resample(const TdrBatchEntry* tab, int k, int blocks_res, hipStream_t s) {
  if (!tab || k < 1 || blocks_res < 1) return fail(TDR_ERR_ARG, "batch_resample: bad arguments");
  hipLaunchKernelGGL(batch_resample_kernel, dim3((unsigned)blocks_res), dim3(TDR_BATCH_THREADS), 0, s, tab, k);
  LAUNCH_CHECK("batch_resample");
  return TDR_OK;
}
