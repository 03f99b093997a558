// tdr_filter_dev.h — the per-particle and per-workgroup bodies of the filter's propagate, resample, max-likelihood and
// pose-statistics kernels.  The standalone kernels (tdr_filter.hip) and the batched ones (tdr_batch.hip,
// tdr_batch_loop.hip) both call these, so a filter ends on the same expressions, the same thread counts and the same
// reduction order on either path, bit for bit.
#ifndef TDR_FILTER_DEV_H_
#define TDR_FILTER_DEV_H_
#include "tdr_common.h"
#include "tdr_sincosf.h"

// ------------------------------------------------------------------------------------------------------------------
// StateParticle::propagate (state_particle.cpp:57-78) of particle p with the normals z.  z*sigma+mu spelled without
// contraction like libstdc++'s normal_distribution (`__ret * stddev + mean`).
__device__ __forceinline__ void propagate_particle(float* __restrict__ st, int64_t cap, int64_t p,
                                                   float* __restrict__ last_dist, const float z[4], float tx, float ty,
                                                   float omega, int scale_freeze, float pos_cov, float theta_cov,
                                                   int libm_fma) {
  float theta = st[TDR_ST_THETA * cap + p];
  float dx = st[TDR_ST_DX * cap + p], dy = st[TDR_ST_DY * cap + p];
  // Rotation2D<float>(theta) * trans (:58): std::cos / std::sin of a float = the host libm's cosf / sinf, restated
  // bit for bit (tdr_sincosf.h)
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
  if (!scale_freeze) {
    const float sd_s = (float)fmin(2. / (double)dist, 0.02);
    float scale = st[TDR_ST_SCALE * cap + p];
    scale *= z[3] * sd_s + 1.f;
    st[TDR_ST_SCALE * cap + p] = scale;
  }
  st[TDR_ST_THETA * cap + p] = theta;
  st[TDR_ST_DX * cap + p] = dx;
  st[TDR_ST_DY * cap + p] = dy;
  const float mx = lx - dx, my = ly - dy;
  last_dist[p] = sqrtf(mx * mx + my * my);
}

// ------------------------------------------------------------------------------------------------------------------
// The systematic resample (particle_filter.cpp:171-185): the particle that sample i of n_new draws — the first index
// whose running maximum of the running sum exceeds (i + shift) / n_new
__device__ __forceinline__ int64_t resample_pick(const float* __restrict__ runmax, int64_t n, int64_t n_new, int64_t i,
                                                 float shift) {
  const float sample = ((float)i + shift) / (float)n_new;  // particle_filter.cpp:176
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (runmax[mid] > sample) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// particle j of the planes src -> slot i of the planes dst
__device__ __forceinline__ void gather_particle(const float* __restrict__ src, int64_t src_cap, int64_t j,
                                                float* __restrict__ dst, int64_t dst_cap, int64_t i) {
#pragma unroll
  for (int f = 0; f < TDR_ST_FIELDS; f++) dst[f * dst_cap + i] = src[f * src_cap + j];
}

// max_likelihood_particle_ = particles_[argmax] (particle_filter.cpp:145-147): the argmax the weight statistics left in
// info[0], and the 12-float record of that particle — its fields and its mlState (state_particle.cpp:98-102)
__device__ __forceinline__ int64_t ml_index(const float* __restrict__ info, int64_t n) {
  const int64_t best = (int64_t)__float_as_int(info[0]);
  return (best < 0 || best >= n) ? 0 : best;
}
__device__ __forceinline__ void ml_record(const float f[TDR_ST_FIELDS], float* __restrict__ out) {
#pragma unroll
  for (int k = 0; k < TDR_ST_FIELDS; k++) out[k] = f[k];
  out[7] = 0.f;
  out[8] = f[TDR_ST_DX] * f[TDR_ST_SCALE] + f[TDR_ST_INIT_X];
  out[9] = f[TDR_ST_DY] * f[TDR_ST_SCALE] + f[TDR_ST_INIT_Y];
  out[10] = f[TDR_ST_THETA];
  out[11] = f[TDR_ST_SCALE];
}

// ------------------------------------------------------------------------------------------------------------------
// Pose statistics (particle_filter.cpp:191-236) + geometric-mean scale (:343-357).  Double accumulation, fixed order.
__device__ double block_sum_d(double v, double* sh) {
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

// this thread's share (particles p0, p0 + step, ...) of the sums of {x, y, theta, scale, cos, sin, log scale}
__device__ __forceinline__ void mc_first_moments(const float* __restrict__ st, int64_t cap, int64_t n, int64_t p0,
                                                 int64_t step, int libm_fma, double acc[7]) {
  for (int k = 0; k < 7; k++) acc[k] = 0;
  for (int64_t p = p0; p < n; p += step) {
    const float sc = st[TDR_ST_SCALE * cap + p];
    const float x = st[TDR_ST_DX * cap + p] * sc + st[TDR_ST_INIT_X * cap + p];  // mlState, state_particle.cpp:98-102
    const float y = st[TDR_ST_DY * cap + p] * sc + st[TDR_ST_INIT_Y * cap + p];
    const float th = st[TDR_ST_THETA * cap + p];
    acc[0] += x; acc[1] += y; acc[2] += th; acc[3] += sc;
    acc[4] += (double)tdr_libm::cosf_v(th, libm_fma); acc[5] += (double)tdr_libm::sinf_v(th, libm_fma);   // :198-199
    acc[6] += log((double)sc);
  }
}
// mean, geometric-mean scale and the reference point of the covariance from the seven sums: the mean, or `about` — the
// max-likelihood particle's mlState (computeCov, particle_filter.cpp:226-236)
__device__ __forceinline__ void mc_mean_ref(const double tot[7], int64_t n, const float* about, float mean[4], float ref[4],
                                            float& geo) {
  const float fn = (float)n;
  mean[0] = (float)tot[0] / fn; mean[1] = (float)tot[1] / fn; mean[3] = (float)tot[3] / fn;
  mean[2] = atan2f((float)tot[5] / fn, (float)tot[4] / fn);  // :202
  geo = (float)exp(tot[6] / (double)n);                       // freezeScale geo-mean
  for (int k = 0; k < 4; k++) ref[k] = about ? about[k] : mean[k];
}
// this thread's share of the 10 second moments about ref
__device__ __forceinline__ void mc_second_moments(const float* __restrict__ st, int64_t cap, int64_t n, int64_t p0,
                                                  int64_t step, const float* ref, double c[10]) {
  for (int k = 0; k < 10; k++) c[k] = 0;
  for (int64_t p = p0; p < n; p += step) {
    const float sc = st[TDR_ST_SCALE * cap + p];
    float d[4];
    d[0] = (st[TDR_ST_DX * cap + p] * sc + st[TDR_ST_INIT_X * cap + p]) - ref[0];
    d[1] = (st[TDR_ST_DY * cap + p] * sc + st[TDR_ST_INIT_Y * cap + p]) - ref[1];
    d[2] = st[TDR_ST_THETA * cap + p] - ref[2];
    d[3] = sc - ref[3];
    while (d[2] > M_PI) d[2] = (float)((double)d[2] - 2 * M_PI);    // :215
    while (d[2] < -M_PI) d[2] = (float)((double)d[2] + 2 * M_PI);   // :216
    int k = 0;
    for (int a = 0; a < 4; a++)
      for (int b = a; b < 4; b++) c[k++] += (double)(d[a] * d[b]);
  }
}
// the 24 result floats: mean [0, 4), covariance [4, 20), geometric-mean scale [20], zeros
__device__ __forceinline__ void mc_write_mean(float* __restrict__ out, const float mean[4], float geo) {
  for (int k = 0; k < 4; k++) out[k] = mean[k];
  out[20] = geo;
  out[21] = out[22] = out[23] = 0.f;
}
__device__ __forceinline__ void mc_write_cov(float* __restrict__ out, const double ct[10], int64_t n) {
  int k = 0;
  for (int a = 0; a < 4; a++)
    for (int b = a; b < 4; b++) {
      const float v = (float)ct[k++] / (float)(n - 1);  // :219
      out[4 + 4 * a + b] = v;
      out[4 + 4 * b + a] = v;
    }
}

// One workgroup (1024 threads) does everything: up to MC_SINGLE_MAX_N particles.
#define MC_SINGLE_MAX_N 4096
__device__ __forceinline__ void mean_cov_body(const float* __restrict__ st, int64_t cap, int64_t n,
                                              const float* __restrict__ about, float* __restrict__ out, int libm_fma) {
  __shared__ double shd[16];
  __shared__ float ref[4];
  const int tid = threadIdx.x, nt = blockDim.x;
  double acc[7], tot[7];
  mc_first_moments(st, cap, n, tid, nt, libm_fma, acc);
  for (int k = 0; k < 7; k++) tot[k] = block_sum_d(acc[k], shd);
  if (tid == 0) {
    float mean[4], r[4], geo;
    mc_mean_ref(tot, n, about, mean, r, geo);
    mc_write_mean(out, mean, geo);
    for (int k = 0; k < 4; k++) ref[k] = r[k];
  }
  __syncthreads();
  double c[10], ct[10];
  mc_second_moments(st, cap, n, tid, nt, ref, c);
  for (int k = 0; k < 10; k++) ct[k] = block_sum_d(c[k], shd);
  if (tid == 0) mc_write_cov(out, ct, n);
}

// Larger particle sets: the same two reductions over MC_WGS workgroups.  Per-workgroup partial sums (double) go to a
// scratch area; they are combined in workgroup order, so the result is a pure function of the inputs.
//   mc_sums_body  (MC_WGS)  -> partial sums of {x, y, theta, scale, cos, sin, log scale}
//   mc_cov_body   (MC_WGS)  -> every workgroup combines the partial sums (mean / reference), then its share of the
//                              10 second moments about it
//   mc_final_body (1)       -> combines both, writes the 24 result floats
#define MC_WGS 128
#define MC_THREADS 256
struct McScratch {
  double sums[MC_WGS][8];
  double mom[MC_WGS][10];
};
static_assert(24 * 4 + sizeof(McScratch) <= TDR_MEAN_COV_FLOATS * 4, "TDR_MEAN_COV_FLOATS too small");

__device__ __forceinline__ void mc_sums_body(const float* __restrict__ st, int64_t cap, int64_t n, McScratch* sc,
                                             int libm_fma) {
  __shared__ double shd[16];
  double acc[7];
  mc_first_moments(st, cap, n, (int64_t)blockIdx.x * MC_THREADS + threadIdx.x, (int64_t)MC_WGS * MC_THREADS, libm_fma, acc);
  for (int k = 0; k < 7; k++) {
    const double t = block_sum_d(acc[k], shd);
    if (threadIdx.x == 0) sc->sums[blockIdx.x][k] = t;
  }
}
// mean / reference point from the partial sums, identically in every caller (workgroup order); `stage` = MC_WGS*8 doubles
__device__ __forceinline__ void mc_means(const McScratch* sc, int64_t n, const float* about, double* stage,
                                         double* sh /*[8]*/, float mean[4], float ref[4], float& geo) {
  __syncthreads();
  for (int t = threadIdx.x; t < MC_WGS * 8; t += MC_THREADS) stage[t] = (&sc->sums[0][0])[t];   // coalesced
  __syncthreads();
  if (threadIdx.x < 7) {
    double t = 0;
    for (int g = 0; g < MC_WGS; g++) t += stage[g * 8 + threadIdx.x];
    sh[threadIdx.x] = t;
  }
  __syncthreads();
  mc_mean_ref(sh, n, about, mean, ref, geo);
}
__device__ __forceinline__ void mc_cov_body(const float* __restrict__ st, int64_t cap, int64_t n,
                                            const float* __restrict__ about, McScratch* sc) {
  __shared__ double shd[16];
  __shared__ double shm[8];
  __shared__ double stage[MC_WGS * 10];
  float mean[4], ref[4], geo;
  mc_means(sc, n, about, stage, shm, mean, ref, geo);
  double c[10];
  mc_second_moments(st, cap, n, (int64_t)blockIdx.x * MC_THREADS + threadIdx.x, (int64_t)MC_WGS * MC_THREADS, ref, c);
  for (int k = 0; k < 10; k++) {
    const double t = block_sum_d(c[k], shd);
    if (threadIdx.x == 0) sc->mom[blockIdx.x][k] = t;
  }
}
__device__ __forceinline__ void mc_final_body(int64_t n, const float* __restrict__ about, const McScratch* sc,
                                              float* __restrict__ out) {
  __shared__ double shm[8];
  __shared__ double shc[10];
  __shared__ double stage[MC_WGS * 10];
  float mean[4], ref[4], geo;
  mc_means(sc, n, about, stage, shm, mean, ref, geo);
  __syncthreads();
  for (int t = threadIdx.x; t < MC_WGS * 10; t += MC_THREADS) stage[t] = (&sc->mom[0][0])[t];
  __syncthreads();
  if (threadIdx.x < 10) {
    double t = 0;
    for (int g = 0; g < MC_WGS; g++) t += stage[g * 10 + threadIdx.x];
    shc[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    mc_write_mean(out, mean, geo);
    mc_write_cov(out, shc, n);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// computeGMM's i-th sample of num (src/particle_filter.cpp:262-266): mlState().head<3>() = {x, y, theta} of particle
// min(n-1, i*n/num).  The standalone sampler (tdr_filter.hip) and the batched mixture fit (tdr_gmm.hip) both call it.
__device__ __forceinline__ void sample_ml_state(const float* __restrict__ st, int64_t cap, int64_t n, int num, int i,
                                                float out[3]) {
  const int64_t p = min(n - 1, (int64_t)i * n / num);   // :265-266
  const float sc = st[TDR_ST_SCALE * cap + p];
  out[0] = st[TDR_ST_DX * cap + p] * sc + st[TDR_ST_INIT_X * cap + p];
  out[1] = st[TDR_ST_DY * cap + p] * sc + st[TDR_ST_INIT_Y * cap + p];
  out[2] = st[TDR_ST_THETA * cap + p];
}

#endif  // TDR_FILTER_DEV_H_
