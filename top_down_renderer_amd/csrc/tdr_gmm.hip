// tdr_gmm.hip — the mixture fit of tdr_gmm.cpp on the device: computeGMM (src/particle_filter.cpp:252-318) for one
// filter or a batch of filters without the host EM.
//
// THE DEFINITION IS tdr_gmm_fit_host, STATEMENT FOR STATEMENT, and every floating-point sum is formed in the host's
// order (the library is built with -ffp-contract=off, so a device expression rounds like the host's).  What may differ
// from the host's bits are exp / log (device math library against glibc); the hard decisions — the seeding argmin /
// argmax, the Lloyd labels, the empty-cluster test — see the same numbers.
//
// One workgroup of GMM_NT threads per fit.  The <= 1000 x 4 doubles of samples sit in LDS; the responsibilities
// (m x k doubles, the host's [i][k] layout) in a caller-supplied global workspace.  Serial sums are chains:
//   overall mean          one lane per dimension walks the samples in index order
//   Lloyd centres         one lane per (cluster, dimension)
//   M-step                one lane per (cluster, accumulator): nk and the 4 mean sums side by side (the division by nk
//                         follows), then the 10 covariance entries
//   tot += lse            one lane, beside the nk and mean chains of the M-step that follows unless the fit stops
// while everything that is per sample (distances, labels, log-densities, log-sum-exp) runs one sample per lane.  The two
// arg-reductions (nearest to the mean, farthest first) compare (value, index) pairs, which is the host's "strict
// comparison, lowest index wins" in any order.  Every loop is bounded (m, k, 10, max_iter); the convergence exit is
// broadcast through LDS, so it is workgroup-uniform; nothing depends on the workgroup's position in the grid.  The chain
// loops are unrolled by 16 so that a lane's loads run ahead of its dependent adds (the order of the adds is the loop's).
#include <climits>

#include "tdr_common.h"
#include "tdr_filter_dev.h"
#include "tdr_gmm_dev.h"
#include "tdr_sincosf.h"

namespace {

constexpr int D = 4;
constexpr double REG = 1e-6;
constexpr int GMM_NT = 512;
constexpr int GMM_WAVES = GMM_NT / 64;
constexpr int GMM_MAX_M = 1000;           // :262
constexpr int GMM_MAX_K = TDR_GMM_MAX_K;

struct GmmShared {
  double X[GMM_MAX_M * D];
  double aux[GMM_MAX_M];                  // farthest-first: distance to the nearest centre; EM: the samples' lse
  int label[GMM_MAX_M];
  double w[GMM_MAX_K], logw[GMM_MAX_K], logdet[GMM_MAX_K], nk[GMM_MAX_K];
  double mu[GMM_MAX_K][D], nmu[GMM_MAX_K][D], cen[GMM_MAX_K][D];
  double cov[GMM_MAX_K][D * D], L[GMM_MAX_K][D * D], ncov[GMM_MAX_K][D * D];
  double red_v[GMM_WAVES];
  int red_i[GMM_WAVES];
  double mean[D];
  double ll;
  int pick, stop;
};
static_assert(sizeof(GmmShared) <= 64 * 1024, "the fit's LDS must fit the static limit");

__device__ __forceinline__ double dist2(const double* a, const double* b) {
  double s = 0;
  for (int d = 0; d < D; d++) s += (a[d] - b[d]) * (a[d] - b[d]);
  return s;
}

// The index of the smallest (MAXI: largest) value among the lanes' (v, i) pairs, the lowest index among equals; INT_MAX
// when no lane holds a candidate.  Every lane gets the result.
template <bool MAXI>
__device__ __forceinline__ bool better(double v, int i, double bv, int bi) {
  return (MAXI ? v > bv : v < bv) || (v == bv && i < bi);
}
template <bool MAXI>
__device__ int block_arg(GmmShared& S, double v, int i) {
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_down(v, off);
    const int oi = __shfl_down(i, off);
    if (better<MAXI>(ov, oi, v, i)) { v = ov; i = oi; }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { S.red_v[wave] = v; S.red_i[wave] = i; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < GMM_WAVES; k++)
      if (better<MAXI>(S.red_v[k], S.red_i[k], v, i)) { v = S.red_v[k]; i = S.red_i[k]; }
    S.pick = i;
  }
  __syncthreads();
  return S.pick;
}

// cholesky() of tdr_gmm.cpp on cov (row-major 4x4, lower triangle read); false where the host's fails
__device__ __forceinline__ bool cholesky(const double* cov, double* L, double* logdet) {
#pragma unroll
  for (int i = 0; i < D * D; i++) L[i] = 0;
  double ld = 0;
#pragma unroll
  for (int i = 0; i < D; i++) {
#pragma unroll
    for (int j = 0; j <= i; j++) {
      double s = cov[i * D + j];
#pragma unroll
      for (int k = 0; k < j; k++) s -= L[i * D + k] * L[j * D + k];
      if (i == j) {
        if (!(s > 0)) return false;
        L[i * D + i] = sqrt(s);
        ld += log(s);
      } else {
        L[i * D + j] = s / L[j * D + j];
      }
    }
  }
  *logdet = ld;
  return true;
}

// The chains that need nothing but the responsibilities R [m][k], side by side on lanes of different waves: the nk of
// params_from_resp (k chains), its mean sums (4 k chains, divided by nk afterwards) and, with_tot, the E-step's
// `tot += lse` with the convergence test.  The mean sums of a step that then stops are never used.
constexpr int GMM_NK_LANE0 = 64, GMM_MU_LANE0 = 128;
static_assert(GMM_MU_LANE0 + D * GMM_MAX_K <= GMM_NT && GMM_NK_LANE0 + GMM_MAX_K <= GMM_MU_LANE0, "lane ranges");
__device__ void resp_sums(GmmShared& S, const double* __restrict__ R, int m, int k, bool with_tot, double prev) {
  const int t = threadIdx.x;
  if (t == 0) {
    if (with_tot) {
      double tot = 0;
#pragma unroll 16
      for (int i = 0; i < m; i++) tot += S.aux[i];
      const double ll = tot / m;
      S.ll = ll;
      S.stop = fabs(ll - prev) < 1e-6;
    }
  } else if (t >= GMM_NK_LANE0 && t < GMM_NK_LANE0 + k) {
    const int c = t - GMM_NK_LANE0;
    double nk = 0;
#pragma unroll 16
    for (int i = 0; i < m; i++) nk += R[(size_t)i * k + c];
    S.nk[c] = nk;
  } else if (t >= GMM_MU_LANE0 && t < GMM_MU_LANE0 + D * k) {
    const int c = (t - GMM_MU_LANE0) / D, d = (t - GMM_MU_LANE0) % D;
    double s = 0;
#pragma unroll 16
    for (int i = 0; i < m; i++) s += R[(size_t)i * k + c] * S.X[i * D + d];
    S.nmu[c][d] = s;
  }
  __syncthreads();
}

// the rest of params_from_resp of tdr_gmm.cpp, after resp_sums
__device__ void params_from_sums(GmmShared& S, const double* __restrict__ R, int m, int k) {
  const int t = threadIdx.x;
  if (t < D * k) {
    const int c = t / D, d = t % D;
    const double nk = S.nk[c];
    if (nk > 1e-10) S.nmu[c][d] = S.nmu[c][d] / nk;
  }
  __syncthreads();
  if (t < 10 * k) {
    const int c = t / 10, e = t % 10;
    // e -> (a, b), b <= a, in the host's order: (0,0) (1,0) (1,1) (2,0) ...
    const int a = e < 1 ? 0 : e < 3 ? 1 : e < 6 ? 2 : 3;
    const int b = e - a * (a + 1) / 2;
    const double nk = S.nk[c];
    if (nk > 1e-10) {
      const double ma = S.nmu[c][a], mb = S.nmu[c][b];
      double s = 0;
#pragma unroll 16
      for (int i = 0; i < m; i++) s += R[(size_t)i * k + c] * (S.X[i * D + a] - ma) * (S.X[i * D + b] - mb);
      S.ncov[c][a * D + b] = S.ncov[c][b * D + a] = s / nk + (a == b ? REG : 0.0);
    }
  }
  __syncthreads();
  if (t < k) {
    const double nk = S.nk[t];
    if (nk > 1e-10) {   // (an empty cluster keeps its parameters)
      double L[D * D], ld;
      if (cholesky(S.ncov[t], L, &ld)) {   // (a covariance whose Cholesky fails is not adopted)
        const double w = nk / m;
        S.w[t] = w;
        S.logw[t] = log(w);
        S.logdet[t] = ld;
        for (int d = 0; d < D; d++) S.mu[t][d] = S.nmu[t][d];
#pragma unroll
        for (int i = 0; i < D * D; i++) { S.cov[t][i] = S.ncov[t][i]; S.L[t][i] = L[i]; }
      }
    }
  }
  __syncthreads();
}

// log_pdf of tdr_gmm.cpp; c4 = D * log(2 pi) as the host forms it
__device__ __forceinline__ double log_pdf(const GmmShared& S, int c, const double* x, double c4) {
  double y[D];
  double maha = 0;
#pragma unroll
  for (int i = 0; i < D; i++) {
    double s = x[i] - S.mu[c][i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= S.L[c][i * D + k] * y[k];
    y[i] = s / S.L[c][i * D + i];
    maha += y[i] * y[i];
  }
  return S.logw[c] - 0.5 * (c4 + S.logdet[c] + maha);
}

// one fit by one workgroup: the body of both launches below
__device__ __forceinline__ void gmm_fit_body(GmmShared& S, const tdr_gmm_job& job, double c4) {
  const int m = job.m, k = job.k, t = threadIdx.x;
  if (!job.samples || !job.out || !job.workspace || m < 1 || m > GMM_MAX_M || k < 1 || k > GMM_MAX_K || k > m) return;
  double* __restrict__ R = job.workspace;
  for (int i = t; i < m * D; i += GMM_NT) S.X[i] = job.samples[i];
  __syncthreads();
  // ---- seeding: nearest to the overall mean, then farthest-first
  if (t < D) {
    double s = 0;
    for (int i = 0; i < m; i++) s += S.X[i * D + t];
    S.mean[t] = s / m;
  }
  __syncthreads();
  {
    double bv = std::numeric_limits<double>::infinity();
    int bi = INT_MAX;
    for (int i = t; i < m; i += GMM_NT) {
      const double d2 = dist2(&S.X[i * D], S.mean);
      if (d2 < bv) { bv = d2; bi = i; }
      S.aux[i] = std::numeric_limits<double>::infinity();
    }
    int best = block_arg<false>(S, bv, bi);
    if (best == INT_MAX) best = 0;
    if (t < D) S.cen[0][t] = S.X[best * D + t];
    __syncthreads();
  }
  for (int n = 1; n < k; n++) {
    double bv = -1;
    int bi = INT_MAX;
    for (int i = t; i < m; i += GMM_NT) {
      const double d2 = dist2(&S.X[i * D], S.cen[n - 1]);
      const double md = d2 < S.aux[i] ? d2 : S.aux[i];   // std::min(mind[i], d2)
      S.aux[i] = md;
      if (md > bv) { bv = md; bi = i; }
    }
    int best = block_arg<true>(S, bv, bi);
    if (best == INT_MAX) best = 0;
    if (t < D) S.cen[n][t] = S.X[best * D + t];
    __syncthreads();
  }
  // ---- Lloyd
  for (int it = 0; it < 10; it++) {
    for (int i = t; i < m; i += GMM_NT) {
      int best = 0;
      double bd = std::numeric_limits<double>::infinity();
      for (int c = 0; c < k; c++) {
        const double d2 = dist2(&S.X[i * D], S.cen[c]);
        if (d2 < bd) { bd = d2; best = c; }
      }
      S.label[i] = best;
    }
    __syncthreads();
    if (t < D * k) {
      const int c = t / D, d = t % D;
      double s = 0;
      int cnt = 0;
      for (int i = 0; i < m; i++)
        if (S.label[i] == c) { s += S.X[i * D + d]; cnt++; }
      if (cnt > 0) S.cen[c][d] = s / cnt;
    }
    __syncthreads();
  }
  // ---- initial mixture from the hard partition
  if (t < k) {
    const double w = 1.0 / k;
    S.w[t] = w;
    S.logw[t] = log(w);
    S.logdet[t] = 0;                       // cholesky(I): L = I, logdet = 0
    for (int d = 0; d < D; d++) S.mu[t][d] = S.cen[t][d];
    for (int i = 0; i < D * D; i++) S.cov[t][i] = S.L[t][i] = (i % (D + 1) == 0) ? 1.0 : 0.0;
  }
  for (int i = t; i < m; i += GMM_NT) {
    const int l = S.label[i];
    for (int c = 0; c < k; c++) R[(size_t)i * k + c] = c == l ? 1.0 : 0.0;
  }
  __syncthreads();
  resp_sums(S, R, m, k, false, 0.0);
  params_from_sums(S, R, m, k);
  // ---- EM
  const int iters = job.max_iter > 1 ? job.max_iter : 1;
  double prev = -std::numeric_limits<double>::infinity();
  int used = 0;
  for (int it = 0; it < iters; it++) {
    for (int i = t; i < m; i += GMM_NT) {
      double* r = R + (size_t)i * k;
      double mx = -std::numeric_limits<double>::infinity();
      for (int c = 0; c < k; c++) {
        const double lp = log_pdf(S, c, &S.X[i * D], c4);
        r[c] = lp;
        mx = mx < lp ? lp : mx;            // std::max(mx, lp)
      }
      double se = 0;
      for (int c = 0; c < k; c++) se += exp(r[c] - mx);
      const double lse = mx + log(se);
      for (int c = 0; c < k; c++) r[c] = exp(r[c] - lse);
      S.aux[i] = lse;
    }
    __syncthreads();
    resp_sums(S, R, m, k, true, prev);     // tot and the stop flag; beside them the next M-step's first chains
    used = it + 1;
    if (S.stop) break;
    prev = S.ll;
    params_from_sums(S, R, m, k);
  }
  // ---- out: w[k], mu[k][4], cov[k][4][4], ll, iterations used
  double* __restrict__ out = job.out;
  if (t < k) {
    out[t] = S.w[t];
    for (int d = 0; d < D; d++) out[k + t * D + d] = S.mu[t][d];
    for (int i = 0; i < D * D; i++) out[k + k * D + t * D * D + i] = S.cov[t][i];
  }
  if (t == 0) {
    out[(size_t)k * 21] = S.ll;
    out[(size_t)k * 21 + 1] = (double)used;
  }
}

// grid = jobs, from a device table ...
__global__ __launch_bounds__(GMM_NT) void gmm_fit_kernel(const tdr_gmm_job* __restrict__ jobs, double c4) {
  __shared__ GmmShared S;
  const tdr_gmm_job job = jobs[blockIdx.x];
  gmm_fit_body(S, job, c4);
}
// ... and one job as a kernel argument (tdr_k_gmm_fit: no table to upload)
__global__ __launch_bounds__(GMM_NT) void gmm_fit_one_kernel(tdr_gmm_job job, double c4) {
  __shared__ GmmShared S;
  gmm_fit_body(S, job, c4);
}

// {x, y, theta} floats -> {x, y, 50 cos theta, 50 sin theta} doubles: tdr_filter_compute_gmm's conversion, where
// std::cos(float) is the float overload and 50 * cosf(theta) a FLOAT product, widened afterwards
__device__ __forceinline__ void gmm_sample(const float ml[3], double* __restrict__ x, int libm_fma) {
  x[0] = ml[0];
  x[1] = ml[1];
  const uint32_t tb = __float_as_uint(ml[2]);
  if ((tb & 0x7f800000u) == 0x7f800000u) {
    // theta = +-inf / NaN: glibc's (x - x) / (x - x) and the product by 50 leave, on the x86-64 host, the quieted argument
    // for a NaN and the negative default NaN for an infinity; a device subtraction picks its own default NaN, so the
    // host's bits are spelled out (widened: sign, all-ones exponent, the 23 mantissa bits on top)
    const uint32_t nb = (tb & 0x007fffffu) ? (tb | 0x00400000u) : 0xffc00000u;
    const uint64_t db = ((uint64_t)(nb >> 31) << 63) | 0x7ff0000000000000ull | ((uint64_t)(nb & 0x007fffffu) << 29);
    x[2] = x[3] = __longlong_as_double((long long)db);
    return;
  }
  x[2] = 50 * tdr_libm::cosf_v(ml[2], libm_fma);
  x[3] = 50 * tdr_libm::sinf_v(ml[2], libm_fma);
}
__global__ void gmm_samples_kernel(const float* __restrict__ ml3, int num, double* __restrict__ out, int libm_fma) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num) return;
  const float ml[3] = {ml3[3 * i], ml3[3 * i + 1], ml3[3 * i + 2]};
  gmm_sample(ml, out + (size_t)4 * i, libm_fma);
}
// ... of every filter of a batch, from its particle planes (sample_ml_state = tdr_k_sample_ml_states' expression)
__global__ void gmm_batch_samples_kernel(const TdrGmmSampleEntry* __restrict__ tab, int libm_fma) {
  const TdrGmmSampleEntry e = tab[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= e.num) return;
  float ml[3];
  sample_ml_state(e.st, e.cap, e.n, e.num, i, ml);
  gmm_sample(ml, e.samples + (size_t)4 * i, libm_fma);
}

// computeGMM's selection rule (:276-297) over the candidate fits of one filter, as tdr_gmm_select_host applies it
__global__ void gmm_pick_kernel(const tdr_gmm_pick_job* __restrict__ jobs, int n) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n) return;
  const tdr_gmm_pick_job j = jobs[f];
  const int k = j.k;
  if (!j.cand[0] || !j.record || k < 1 || k > GMM_MAX_K) return;
  const double ll = j.cand[0][(size_t)21 * k];
  int dir = 0;
  if (j.cand[1] && k + 1 <= GMM_MAX_K && ll + 0.3 < j.cand[1][(size_t)21 * (k + 1)]) dir = 1;
  if (j.cand[2] && k > 1 && ll - 0.3 < j.cand[2][(size_t)21 * (k - 1)]) dir = -1;
  const int kc = k + dir;
  const double* __restrict__ src = dir == 0 ? j.cand[0] : dir == 1 ? j.cand[1] : j.cand[2];
  double* __restrict__ rec = j.record;
  rec[0] = (double)kc;
  rec[1] = src[(size_t)21 * kc];
  for (int c = 0; c < kc; c++) {
    const double* mu = src + kc + (size_t)c * D;
    const double* cv = src + kc + (size_t)kc * D + (size_t)c * D * D;
    double* o = rec + 2 + 8 * c;
    for (int d = 0; d < D; d++) o[d] = mu[d];
    o[4] = cv[0]; o[5] = cv[1]; o[6] = cv[D]; o[7] = cv[D + 1];
  }
}

double log_2pi_d() { return D * std::log(2 * M_PI); }   // the term of tdr_gmm.cpp's log_pdf, formed as there

}  // namespace

extern "C" {
size_t tdr_gmm_workspace_bytes(int m, int k) {
  if (m < 1 || k < 1) return 0;
  return (size_t)m * (size_t)k * sizeof(double);
}
int tdr_gmm_out_doubles(int k) { return k < 1 ? 0 : 21 * k + 2; }

int tdr_k_gmm_samples(const float* ml3, int num, double* samples_out, void* stream) {
  if (!ml3 || !samples_out || num < 1) return fail(TDR_ERR_ARG, "gmm_samples: bad arguments");
  hipLaunchKernelGGL(gmm_samples_kernel, dim3((unsigned)cdiv(num, 256)), dim3(256), 0, (hipStream_t)stream, ml3, num,
                     samples_out, tdr_libm_fma());
  LAUNCH_CHECK("gmm_samples");
  return TDR_OK;
}

int tdr_k_gmm_fit_jobs(const tdr_gmm_job* jobs_dev, int n_jobs, void* stream) {
  if (!jobs_dev || n_jobs < 1) return fail(TDR_ERR_ARG, "gmm_fit_jobs: bad arguments");
  hipLaunchKernelGGL(gmm_fit_kernel, dim3((unsigned)n_jobs), dim3(GMM_NT), 0, (hipStream_t)stream, jobs_dev, log_2pi_d());
  LAUNCH_CHECK("gmm_fit");
  return TDR_OK;
}

int tdr_k_gmm_fit(const double* samples, int m, int k, int max_iter, double* out, double* workspace, void* stream) {
  if (!samples || !out || !workspace || m < 1 || m > GMM_MAX_M || k < 1 || k > GMM_MAX_K || k > m)
    return fail(TDR_ERR_ARG, "gmm_fit: bad arguments (1 <= k <= min(m, %d), m <= %d)", GMM_MAX_K, GMM_MAX_M);
  const tdr_gmm_job job{samples, m, k, max_iter, 0, out, workspace};
  hipLaunchKernelGGL(gmm_fit_one_kernel, dim3(1), dim3(GMM_NT), 0, (hipStream_t)stream, job, log_2pi_d());
  LAUNCH_CHECK("gmm_fit");
  return TDR_OK;
}

int tdr_k_gmm_pick(const tdr_gmm_pick_job* jobs_dev, int n, void* stream) {
  if (!jobs_dev || n < 1) return fail(TDR_ERR_ARG, "gmm_pick: bad arguments");
  hipLaunchKernelGGL(gmm_pick_kernel, dim3((unsigned)cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, jobs_dev, n);
  LAUNCH_CHECK("gmm_pick");
  return TDR_OK;
}

// the candidate table of tdr_gmm_select_host: cand[0] = k (:259), cand[1] = k + 1 or 0 (:280), cand[2] = k - 1 or 0 (:288)
int tdr_gmm_candidates_host(int num_gaussians, int64_t num_particles, int m, int max_k, int cand[3]) {
  if (!cand || m < 1 || max_k < 1) return fail(TDR_ERR_ARG, "gmm_candidates: bad arguments");
  const int cap = std::min(max_k, m);
  int k = std::max(1, std::min<int>((int)(num_particles / 20) + 1, num_gaussians));
  k = std::min(k, cap);
  cand[0] = k;
  cand[1] = ((int64_t)k * 50 < num_particles && k + 1 <= cap) ? k + 1 : 0;
  cand[2] = k > 1 ? k - 1 : 0;
  return TDR_OK;
}
}  // extern "C"

int tdr_gmm_batch_samples(const TdrGmmSampleEntry* tab_dev, int k, hipStream_t s) {
  if (!tab_dev || k < 1) return fail(TDR_ERR_ARG, "gmm_batch_samples: bad arguments");
  hipLaunchKernelGGL(gmm_batch_samples_kernel, dim3((unsigned)cdiv(GMM_MAX_M, 256), (unsigned)k), dim3(256), 0, s, tab_dev,
                     tdr_libm_fma());
  LAUNCH_CHECK("gmm_batch_samples");
  return TDR_OK;
}
