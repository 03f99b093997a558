// tdr_kld.hip — KLD-sampling count (include/tdr.h, "KLD-sampling count"): the distinct pose bins among the
// particles of a filter, in one pass over the state planes, without a sort.
//   lane = particle: the key is computed in registers (kld_key);
//   wave: equal keys are merged before anything goes to memory.  After a resample neighbours are mostly copies of one source
//     particle, so a lane whose left neighbour holds its key drops out at once; the remaining run heads elect one leader per
//     distinct key in a ballot / readlane loop of register work only (one turn per distinct key of the wave);
//   leaders insert into the job's open-addressing table in global memory, all of a wave's leaders side by side: a plain load
//     first (a slot only ever changes from empty to its key, so a load that shows the key is final), a 64-bit
//     compare-and-swap where it showed the empty word, the next slot otherwise.  An insertion counts exactly when its swap
//     returned the empty word;
//   counts: ballot + bit count per wave, LDS across the four waves, one 64-bit integer atomic per workgroup and word.
// Integer atomics only: {k, skipped} do not depend on the order of anything.
#include "tdr_common.h"
#include "tdr_score_dev.h"   // rot_shift_dev

namespace {
constexpr int KLD_BLOCK = 256;
constexpr int KLD_MAX_BLOCKS = 2048;   // grid.x: a workgroup strides over its job's particles beyond that
constexpr int KLD_JOBS_BLOCKS_X = 256;  // ... and the grid.x of a job table, whose sizes the host does not see
constexpr uint64_t KLD_EMPTY = TDR_KLD_NO_KEY;

struct KldKeyParams {
  float bin_xy;
  int theta_bins, scale_shift;   // 23 - scale_bits
};

__device__ __forceinline__ uint64_t kld_key(const float* __restrict__ st, int64_t cap, int64_t p, const KldKeyParams& kp) {
  const float s = st[TDR_ST_SCALE * cap + p];
  const float cx = st[TDR_ST_DX * cap + p] * s + st[TDR_ST_INIT_X * cap + p];
  const float cy = st[TDR_ST_DY * cap + p] * s + st[TDR_ST_INIT_Y * cap + p];
  const float theta = st[TDR_ST_THETA * cap + p];
  const float hi = st[TDR_ST_HAVE_INIT * cap + p];
  const float inf = __builtin_inff();
  // (a NaN fails every comparison)
  if (!(fabsf(cx) < inf) || !(fabsf(cy) < inf) || !(s > 0.f) || !(s < inf)) return KLD_EMPTY;
  const int ix = (int)floorf(__builtin_amdgcn_fmed3f(cx / kp.bin_xy, -524288.f, 524287.f));
  const int iy = (int)floorf(__builtin_amdgcn_fmed3f(cy / kp.bin_xy, -524288.f, 524287.f));
  const int it = hi != 0.f ? rot_shift_dev(theta, kp.theta_bins) : kp.theta_bins;
  const uint32_t is = __float_as_uint(s) >> kp.scale_shift;
  return (uint64_t)(uint32_t)(ix + 524288) << 43 | (uint64_t)(uint32_t)(iy + 524288) << 23 | (uint64_t)(uint32_t)it << 14 |
         (uint64_t)is;
}

__device__ __forceinline__ uint64_t kld_hash(uint64_t k) {   // the finaliser of MurmurHash3: every key bit reaches every slot bit
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int lane) {   // lane: wave-uniform
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return (uint64_t)hi << 32 | lo;
}

struct KldArgs {
  const tdr_kld_job* jobs;   // DEVICE, or NULL: `one`
  tdr_kld_job one;
  KldKeyParams kp;
};

__global__ __launch_bounds__(KLD_BLOCK) void kld_count_kernel(KldArgs a) {
  const tdr_kld_job job = a.jobs ? a.jobs[blockIdx.y] : a.one;
  const int64_t n = job.n;
  const uint64_t mask = (uint64_t)job.table_slots - 1;
  const int lane = threadIdx.x & 63;
  unsigned n_ins = 0, n_skip = 0;   // wave-uniform
  // every lane of the workgroup makes every turn (the bound is the workgroup's): the ballots see whole waves
  for (int64_t p0 = (int64_t)blockIdx.x * KLD_BLOCK; p0 < n; p0 += (int64_t)gridDim.x * KLD_BLOCK) {
    const int64_t p = p0 + threadIdx.x;
    const bool live = p < n;
    const uint64_t key = live ? kld_key(job.st, job.cap, p, a.kp) : KLD_EMPTY;
    n_skip += (unsigned)__popcll(__ballot(live && key == KLD_EMPTY));
    // run heads: a lane whose left neighbour holds the same key is a copy
    const uint64_t left = (uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(key >> 32), 1) << 32 |
                          (uint32_t)__shfl_up((int)(uint32_t)key, 1);
    bool pending = key != KLD_EMPTY && (lane == 0 || left != key);
    bool leader = false;
    for (;;) {
      const uint64_t m = __ballot(pending);
      if (m == 0) break;
      const int first = __ffsll((unsigned long long)m) - 1;
      const uint64_t fk = readlane64(key, first);
      leader = leader || lane == first;
      pending = pending && key != fk;
    }
    bool inserted = false;
    if (leader) {
      uint64_t slot = kld_hash(key) & mask;
      // at most n keys in >= 2 n slots: an empty slot always ends the walk; the bound only keeps a caller's mistake finite
      for (uint64_t probe = 0; probe <= mask; probe++) {
        uint64_t* w = job.table + slot;
        uint64_t seen = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == KLD_EMPTY) {
          seen = atomicCAS((unsigned long long*)w, (unsigned long long)KLD_EMPTY, (unsigned long long)key);
          if (seen == KLD_EMPTY) {
            inserted = true;
            break;
          }
        }
        if (seen == key) break;
        slot = (slot + 1) & mask;
      }
    }
    n_ins += (unsigned)__popcll(__ballot(inserted));
  }
  __shared__ unsigned sh[2][KLD_BLOCK / 64];
  if (lane == 0) {
    sh[0][threadIdx.x >> 6] = n_ins;
    sh[1][threadIdx.x >> 6] = n_skip;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long t = 0;
    for (int w = 0; w < KLD_BLOCK / 64; w++) t += sh[threadIdx.x][w];
    if (t) atomicAdd((unsigned long long*)job.out2 + threadIdx.x, t);
  }
}

__global__ __launch_bounds__(KLD_BLOCK) void kld_keys_kernel(const float* __restrict__ st, int64_t cap, int64_t n, KldKeyParams kp,
                                                             uint64_t* __restrict__ keys) {
  const int64_t p = (int64_t)blockIdx.x * KLD_BLOCK + threadIdx.x;
  if (p < n) keys[p] = kld_key(st, cap, p, kp);
}

int64_t kld_slots(int64_t n) {
  int64_t s = 64;
  while (s < 2 * n) s <<= 1;
  return s;
}

// the key's share of the parameters (epsilon, z and n_min are the host's)
int kld_key_params(const tdr_kld_params* p, const char* who, KldKeyParams& kp) {
  if (!p) return fail(TDR_ERR_ARG, "%s: null parameters", who);
  if (!(p->bin_xy_px > 0.f) || !std::isfinite(p->bin_xy_px)) return fail(TDR_ERR_ARG, "%s: bin_xy_px = %g (finite, > 0)", who, (double)p->bin_xy_px);
  if (p->theta_bins < 1 || p->theta_bins > 511) return fail(TDR_ERR_ARG, "%s: theta_bins = %d (1 .. 511)", who, p->theta_bins);
  if (p->scale_bits < 0 || p->scale_bits > 6) return fail(TDR_ERR_ARG, "%s: scale_bits = %d (0 .. 6)", who, p->scale_bits);
  kp.bin_xy = p->bin_xy_px;
  kp.theta_bins = p->theta_bins;
  kp.scale_shift = 23 - p->scale_bits;
  return TDR_OK;
}
}  // namespace

extern "C" size_t tdr_kld_workspace_bytes(int64_t n) {
  if (n < 0 || n > ((int64_t)1 << 40)) return 0;
  return (size_t)kld_slots(n) * sizeof(uint64_t);
}

extern "C" int tdr_k_kld_keys(const float* st, int64_t cap, int64_t n, const tdr_kld_params* p, uint64_t* keys_out, void* stream) {
  KldKeyParams kp{};
  if (int rc = kld_key_params(p, "kld_keys", kp)) return rc;
  if (!st || !keys_out) return fail(TDR_ERR_ARG, "kld_keys: null pointer");
  if (n < 0 || cap < n || n > ((int64_t)1 << 31)) return fail(TDR_ERR_ARG, "kld_keys: n = %lld of cap = %lld", (long long)n, (long long)cap);
  if (n == 0) return TDR_OK;
  hipLaunchKernelGGL(kld_keys_kernel, dim3((unsigned)cdiv(n, KLD_BLOCK)), dim3(KLD_BLOCK), 0, (hipStream_t)stream, st, cap, n, kp, keys_out);
  LAUNCH_CHECK("kld_keys");
  return TDR_OK;
}

extern "C" int tdr_k_kld_count(const float* st, int64_t cap, int64_t n, const tdr_kld_params* p, void* workspace, int64_t* out2,
                               void* stream) {
  KldKeyParams kp{};
  if (int rc = kld_key_params(p, "kld_count", kp)) return rc;
  if (!st || !workspace || !out2) return fail(TDR_ERR_ARG, "kld_count: null pointer");
  if (n < 0 || cap < n || n > ((int64_t)1 << 40)) return fail(TDR_ERR_ARG, "kld_count: n = %lld of cap = %lld", (long long)n, (long long)cap);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(out2, 0, 2 * sizeof(int64_t), s));
  if (n == 0) return TDR_OK;
  const int64_t slots = kld_slots(n);
  HIP_TRY(hipMemsetAsync(workspace, 0xFF, (size_t)slots * sizeof(uint64_t), s));
  KldArgs a{};
  a.one = tdr_kld_job{st, cap, n, (uint64_t*)workspace, slots, out2};
  a.kp = kp;
  hipLaunchKernelGGL(kld_count_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n, KLD_BLOCK), KLD_MAX_BLOCKS)), dim3(KLD_BLOCK), 0, s, a);
  LAUNCH_CHECK("kld_count");
  return TDR_OK;
}

extern "C" int tdr_k_kld_count_jobs(const tdr_kld_job* jobs_dev, int n_jobs, const tdr_kld_params* p, void* stream) {
  KldKeyParams kp{};
  if (int rc = kld_key_params(p, "kld_count_jobs", kp)) return rc;
  if (!jobs_dev) return fail(TDR_ERR_ARG, "kld_count_jobs: null jobs");
  if (n_jobs < 0 || n_jobs > 65535) return fail(TDR_ERR_ARG, "kld_count_jobs: %d jobs (0 .. 65535)", n_jobs);
  if (n_jobs == 0) return TDR_OK;
  KldArgs a{};
  a.jobs = jobs_dev;
  a.kp = kp;
  // the jobs' sizes live on the device: a fixed grid.x, and a workgroup past its job's particles leaves at once
  hipLaunchKernelGGL(kld_count_kernel, dim3(KLD_JOBS_BLOCKS_X, (unsigned)n_jobs), dim3(KLD_BLOCK), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK("kld_count_jobs");
  return TDR_OK;
}
