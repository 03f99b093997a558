// tdr_batch.hip — batched filter step (tdr_batch_step, include/tdr.h): the per-particle stages of many filters that share
// one map in one launch each.  Every kernel reads a table with one entry per filter (tdr_batch.h); a workgroup finds its
// filter from its block index and then calls the body the standalone kernel calls (tdr_filter_dev.h: propagate_particle,
// resample_pick, gather_particle, ml_index / ml_record) with that filter's pointers and scalars, so each filter ends bit
// for bit where its standalone calls leave it.
#include "tdr_common.h"
#include "tdr_filter_dev.h"
#include "tdr_batch.h"

// StateParticle::propagate (state_particle.cpp:57-78) of every particle of every filter; the normals come from each
// filter's own generator (parity mode), so the mt19937 streams stay per filter
__global__ __launch_bounds__(TDR_BATCH_THREADS) void batch_propagate_kernel(const TdrBatchEntry* __restrict__ tab, int k,
                                                                            int libm_fma) {
  const TdrBatchEntry& f = tab[batch_find(k, (int)blockIdx.x, [&](int i) { return tab[i].blk_prop; })];
  const int64_t p = (int64_t)(blockIdx.x - f.blk_prop) * blockDim.x + threadIdx.x;
  if (p >= f.n) return;
  const float* __restrict__ z4 = f.z4;
  float z[4];
  z[0] = z4[4 * p]; z[1] = z4[4 * p + 1]; z[2] = z4[4 * p + 2]; z[3] = z4[4 * p + 3];
  propagate_particle(f.st, f.cap, p, f.last_dist, z, f.tx, f.ty, f.omega, f.scale_freeze, f.pos_cov, f.theta_cov, libm_fma);
}

// the systematic resample (particle_filter.cpp:171-185) of every filter: the search over the running maximum with the
// filter's own device uniform, the gather of the chosen states into st_new, and — thread 0 of each filter — the
// pre-resample max-likelihood particle (:145-147)
__global__ __launch_bounds__(TDR_BATCH_THREADS) void batch_resample_kernel(const TdrBatchEntry* __restrict__ tab, int k) {
  const TdrBatchEntry& f = tab[batch_find(k, (int)blockIdx.x, [&](int i) { return tab[i].blk_res; })];
  const int64_t i = (int64_t)(blockIdx.x - f.blk_res) * blockDim.x + threadIdx.x;
  if (i >= f.n_new) return;
  if (i == 0) {
    const int64_t best = ml_index(f.info, f.n);
    float v[TDR_ST_FIELDS];
#pragma unroll
    for (int q = 0; q < TDR_ST_FIELDS; q++) v[q] = f.st[(int64_t)q * f.cap + best];
    ml_record(v, f.ml);
  }
  const int64_t j = resample_pick(f.runmax, f.n, f.n_new, i, *f.shift);
  f.idx[i] = (int32_t)j;
  gather_particle(f.st, f.cap, j, f.st_new, f.cap, i);
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
