// tdr_recover_sensor.hip — sensor-resetting recovery (include/tdr.h, "sensor resetting"): the three kernels
// around the scoring launch that give every injected slot the best-scoring of C road candidates.
//   the list: the slots tdr_k_inject would inject, ascending.  The shape of the road-list build (tdr_recover.hip):
//     sr_count_kernel   a workgroup owns a run of whole 256-slot tiles; ballot + bit count per wave, the run's count to the
//                       workspace;
//     sr_scan_kernel    ONE workgroup: the exclusive running sum of the runs' counts (at most SR_MAX_BLOCKS) and the total;
//     sr_write_kernel   the predicate again; a listed slot's place = its run's offset + the tiles before it in the run +
//                       the waves before it + the listed lanes below it.  The order is the slot order whatever the grid.
//   sr_candidates_kernel: lane = candidate.  Candidate j of a slot draws the words the plain injection draws with purposes
//     2j (position) and 2j + 1 (heading), so candidate 0 is that injection's particle; one 4-byte load from the road list
//     per candidate, coalesced vector stores to the candidate planes.
//   sr_select_kernel: one wave per listed slot.  Every lane keeps the best of its stride of the C weights in ascending j,
//     the wave then reduces on (key, -j) with a butterfly of shuffles: the order on the pairs is total, so every lane ends
//     with the same pair whatever the reduction order.  Lanes 0..6 copy the winner's seven fields into the slot.
#include "tdr_common.h"
#include "tdr_philox.h"

namespace {
constexpr int SR_BLOCK = 256;
constexpr int SR_WAVES = SR_BLOCK / 64;
constexpr int SR_MAX_BLOCKS = 2048;   // grid.x of the list kernels; a workgroup owns cdiv(tiles, grid.x) tiles in a row
constexpr int SR_MAX_CAND = 4096;

struct SrListArgs {
  int64_t n, slot_begin, tiles_per_block;
  uint32_t k0, k1, d0, d1, threshold24;
};
__device__ __forceinline__ bool sr_listed(const SrListArgs& a, int64_t p) {
  if (p >= a.n) return false;
  const TdrPhilox4 w = tdr_philox4x32((uint32_t)(a.slot_begin + p), a.d0, a.d1, 0u, a.k0, a.k1);
  return (w.w[0] >> 8) < a.threshold24;
}

__global__ __launch_bounds__(SR_BLOCK) void sr_count_kernel(SrListArgs a, int64_t* __restrict__ block_count) {
  __shared__ int sh[SR_WAVES];
  const int64_t t0 = (int64_t)blockIdx.x * a.tiles_per_block;
  int cnt = 0;   // wave-uniform
  for (int64_t t = t0; t < t0 + a.tiles_per_block; t++) cnt += __popcll(__ballot(sr_listed(a, t * SR_BLOCK + threadIdx.x)));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t s = 0;
    for (int w = 0; w < SR_WAVES; w++) s += sh[w];
    block_count[blockIdx.x] = s;
  }
}

// counts [nb <= SR_MAX_BLOCKS] -> exclusive offsets in place; *total = their sum
__global__ __launch_bounds__(SR_BLOCK) void sr_scan_kernel(int64_t* __restrict__ v, int nb, int64_t* __restrict__ total) {
  constexpr int PER = SR_MAX_BLOCKS / SR_BLOCK;
  __shared__ int64_t part[SR_BLOCK];
  int64_t x[PER], sum = 0;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int b = threadIdx.x * PER + k;
    x[k] = b < nb ? v[b] : 0;
    sum += x[k];
  }
  part[threadIdx.x] = sum;
  __syncthreads();
  int64_t before = 0;
  for (int t = 0; t < (int)threadIdx.x; t++) before += part[t];
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int b = threadIdx.x * PER + k;
    if (b < nb) v[b] = before;
    before += x[k];
  }
  if (threadIdx.x == SR_BLOCK - 1) *total = before;
}

__global__ __launch_bounds__(SR_BLOCK) void sr_write_kernel(SrListArgs a, const int64_t* __restrict__ block_off,
                                                            int32_t* __restrict__ list) {
  __shared__ int sh[2][SR_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t0 = (int64_t)blockIdx.x * a.tiles_per_block;
  int64_t base = block_off[blockIdx.x];
  for (int64_t t = t0; t < t0 + a.tiles_per_block; t++) {
    const int64_t p = t * SR_BLOCK + threadIdx.x;
    const bool on = sr_listed(a, p);
    const uint64_t m = __ballot(on);
    int* cnt = sh[(t - t0) & 1];   // two rows: one barrier a tile
    if (lane == 0) cnt[wave] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < SR_WAVES; w++) {
      off += w < wave ? cnt[w] : 0;
      tot += cnt[w];
    }
    // the place is below the number of listed slots up to p: < the total <= n, and the caller's list holds n words
    if (on) list[base + off + __popcll(m & (((uint64_t)1 << lane) - 1))] = (int32_t)p;
    base += tot;
  }
}

struct SrCandArgs {
  const float* st;   // the filter's planes: the slots' scales
  int64_t cap, n, slot_begin;
  const int32_t* list;
  int64_t first, m;
  int32_t C, cols, heading_mode;
  float resolution;
  const uint32_t* road;
  int64_t n_road;
  uint32_t k0, k1, d0, d1;
  float* cst;
  int64_t cand_cap;
};

__global__ __launch_bounds__(SR_BLOCK) void sr_candidates_kernel(SrCandArgs a) {
  const int64_t q = (int64_t)blockIdx.x * SR_BLOCK + threadIdx.x;
  if (q >= a.m * a.C) return;   // m * C <= cand_cap (the launcher's check)
  const int64_t e = q / a.C;
  const uint32_t j = (uint32_t)(q - e * a.C);
  int64_t p = a.list[a.first + e];
  if (p < 0 || p >= a.n) p = 0;   // (a list that is not this filter's: stay inside the planes)
  const uint32_t slot = (uint32_t)(a.slot_begin + p);
  const TdrPhilox4 w = tdr_philox4x32(slot, a.d0, a.d1, 2u * j, a.k0, a.k1);
  const uint32_t cell = a.road[(uint64_t)w.w[1] * (uint64_t)a.n_road >> 32];   // < n_road
  const uint32_t r = cell / (uint32_t)a.cols, c = cell - r * (uint32_t)a.cols;
  const float ux = (float)(w.w[2] >> 24) * 0x1p-8f, uy = (float)(w.w[3] >> 24) * 0x1p-8f;
  float theta = 0.f, have = 0.f;
  if (a.heading_mode == 1) {
    const TdrPhilox4 b = tdr_philox4x32(slot, a.d0, a.d1, 2u * j + 1u, a.k0, a.k1);
    theta = (float)(b.w[0] >> 8) * 0x1p-24f * 6.2831855f - 3.1415927f;
    have = 1.f;
  }
  float* o = a.cst + q;
  o[TDR_ST_INIT_X * a.cand_cap] = ((float)c + ux) * a.resolution;
  o[TDR_ST_INIT_Y * a.cand_cap] = ((float)r + uy) * a.resolution;
  o[TDR_ST_DX * a.cand_cap] = 0.f;
  o[TDR_ST_DY * a.cand_cap] = 0.f;
  o[TDR_ST_THETA * a.cand_cap] = theta;
  o[TDR_ST_SCALE * a.cand_cap] = a.st[TDR_ST_SCALE * a.cap + p];
  o[TDR_ST_HAVE_INIT * a.cand_cap] = have;
}

struct SrSelectArgs {
  float* st;
  int64_t cap, n;
  const int32_t* list;
  int64_t first, m;
  int32_t C;
  const float* cst;
  int64_t cand_cap;
  const float* craw;
  int32_t* pick_out;   // [m], or NULL
  int64_t* written;    // or NULL
};

__global__ __launch_bounds__(SR_BLOCK) void sr_select_kernel(SrSelectArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t e = (int64_t)blockIdx.x * SR_WAVES + wave;   // wave-uniform
  if (threadIdx.x == 0 && a.written) {
    const int64_t here = a.m - (int64_t)blockIdx.x * SR_WAVES;   // >= 1: the grid is cdiv(m, SR_WAVES)
    atomicAdd((unsigned long long*)a.written, (unsigned long long)(here < SR_WAVES ? here : SR_WAVES));
  }
  if (e >= a.m) return;
  const float* w = a.craw + e * a.C;
  // (key, j): a larger key wins, among equal keys the smaller j.  A lane without a candidate holds a key below every
  // candidate's (a NaN's is -1).
  float best = -2.f;
  int bj = 0x7fffffff;
  for (int j = lane; j < a.C; j += 64) {
    const float v = w[j];
    const float key = v != v ? -1.f : v;
    if (key > best) {   // ascending j within a lane: the first of equal keys stays
      best = key;
      bj = j;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ok = __shfl_xor(best, off, 64);
    const int oj = __shfl_xor(bj, off, 64);
    if (ok > best || (ok == best && oj < bj)) {
      best = ok;
      bj = oj;
    }
  }
  // C >= 1: lane 0 held candidate 0, so bj < C on every lane
  const int64_t p = a.list[a.first + e];
  if (p < 0 || p >= a.n) return;   // (a list that is not this filter's)
  if (lane < TDR_ST_FIELDS) a.st[(int64_t)lane * a.cap + p] = a.cst[(int64_t)lane * a.cand_cap + e * a.C + bj];
  if (lane == 0 && a.pick_out) a.pick_out[e] = bj;
}

int sr_list_blocks(int64_t n, int max_blocks) {
  const int mb = max_blocks >= 1 && max_blocks < SR_MAX_BLOCKS ? max_blocks : SR_MAX_BLOCKS;
  return (int)std::min<int64_t>(cdiv(std::max<int64_t>(n, 1), SR_BLOCK), mb);
}
int sr_check_cands(const char* who, int64_t cap, int64_t n, int64_t first, int64_t m, int candidates, int64_t cand_cap) {
  if (n < 0 || cap < n) return fail(TDR_ERR_ARG, "%s: n = %lld of cap = %lld", who, (long long)n, (long long)cap);
  if (candidates < 1 || candidates > SR_MAX_CAND) return fail(TDR_ERR_ARG, "%s: candidates = %d (1 .. %d)", who, candidates, SR_MAX_CAND);
  if (first < 0 || m < 0 || first + m > n)
    return fail(TDR_ERR_ARG, "%s: list entries [%lld, %lld + %lld) of at most n = %lld", who, (long long)first, (long long)first,
                (long long)m, (long long)n);
  if (m * candidates > cand_cap)
    return fail(TDR_ERR_ARG, "%s: %lld slots x %d candidates, room for %lld", who, (long long)m, candidates, (long long)cand_cap);
  return TDR_OK;
}
}  // namespace

extern "C" size_t tdr_inject_list_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return (size_t)sr_list_blocks(n, 0) * sizeof(int64_t);
}

extern "C" int tdr_k_inject_list(int64_t n, int64_t slot_begin, uint64_t seed, uint64_t draw, uint32_t threshold24,
                                 int32_t* list_out, int64_t* count_dev, void* workspace, int max_blocks, void* stream) {
  if (!list_out || !count_dev || !workspace) return fail(TDR_ERR_ARG, "inject_list: null pointer");
  if (n < 0 || slot_begin < 0 || slot_begin + n > ((int64_t)1 << 31))
    return fail(TDR_ERR_ARG, "inject_list: slots [%lld, %lld + %lld) (global index < 2^31)", (long long)slot_begin,
                (long long)slot_begin, (long long)n);
  if (threshold24 > (1u << 24)) return fail(TDR_ERR_ARG, "inject_list: threshold24 = %u (0 .. 2^24)", threshold24);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0 || threshold24 == 0) {   // an empty list: the length alone
    HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(int64_t), s));
    return TDR_OK;
  }
  const int nb = sr_list_blocks(n, max_blocks);
  SrListArgs a{n, slot_begin, cdiv(cdiv(n, SR_BLOCK), nb), (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)draw,
               (uint32_t)(draw >> 32), threshold24};
  int64_t* blocks = reinterpret_cast<int64_t*>(workspace);
  hipLaunchKernelGGL(sr_count_kernel, dim3((unsigned)nb), dim3(SR_BLOCK), 0, s, a, blocks);
  LAUNCH_CHECK("inject_list_count");
  hipLaunchKernelGGL(sr_scan_kernel, dim3(1), dim3(SR_BLOCK), 0, s, blocks, nb, count_dev);
  LAUNCH_CHECK("inject_list_scan");
  hipLaunchKernelGGL(sr_write_kernel, dim3((unsigned)nb), dim3(SR_BLOCK), 0, s, a, (const int64_t*)blocks, list_out);
  LAUNCH_CHECK("inject_list_write");
  return TDR_OK;
}

extern "C" int tdr_k_inject_candidates(const float* st, int64_t cap, int64_t n, int64_t slot_begin, const int32_t* list,
                                       int64_t first, int64_t m, int candidates, const tdr_map_desc* map, const uint32_t* road,
                                       int64_t n_road, uint64_t seed, uint64_t draw, int heading_mode, float* cand_st,
                                       int64_t cand_cap, void* stream) {
  if (!st || !list || !map || !road || !cand_st) return fail(TDR_ERR_ARG, "inject_candidates: null pointer");
  if (map->rows < 1 || map->cols < 1 || (int64_t)map->rows * map->cols > ((int64_t)1 << 31))
    return fail(TDR_ERR_ARG, "inject_candidates: a %d x %d map", map->rows, map->cols);
  if (int rc = sr_check_cands("inject_candidates", cap, n, first, m, candidates, cand_cap)) return rc;
  if (slot_begin < 0 || slot_begin + n > ((int64_t)1 << 31))
    return fail(TDR_ERR_ARG, "inject_candidates: slot_begin = %lld (global index < 2^31)", (long long)slot_begin);
  if (heading_mode < 0 || heading_mode > 1) return fail(TDR_ERR_ARG, "inject_candidates: heading_mode = %d (0 .. 1)", heading_mode);
  if (n_road < 1 || n_road > (int64_t)map->rows * map->cols) return fail(TDR_ERR_ARG, "inject_candidates: %lld road cells", (long long)n_road);
  if (m == 0) return TDR_OK;
  SrCandArgs a{st, cap, n, slot_begin, list, first, m, candidates, map->cols, heading_mode, map->resolution, road, n_road,
               (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)draw, (uint32_t)(draw >> 32), cand_st, cand_cap};
  hipLaunchKernelGGL(sr_candidates_kernel, dim3((unsigned)cdiv(m * candidates, SR_BLOCK)), dim3(SR_BLOCK), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK("inject_candidates");
  return TDR_OK;
}

extern "C" int tdr_k_inject_select(float* st, int64_t cap, int64_t n, const int32_t* list, int64_t first, int64_t m,
                                   int candidates, const float* cand_st, int64_t cand_cap, const float* cand_w,
                                   int32_t* pick_out, int64_t* written_dev, void* stream) {
  if (!st || !list || !cand_st || !cand_w) return fail(TDR_ERR_ARG, "inject_select: null pointer");
  if (int rc = sr_check_cands("inject_select", cap, n, first, m, candidates, cand_cap)) return rc;
  if (m == 0) return TDR_OK;
  SrSelectArgs a{st, cap, n, list, first, m, candidates, cand_st, cand_cap, cand_w, pick_out, written_dev};
  hipLaunchKernelGGL(sr_select_kernel, dim3((unsigned)cdiv(m, SR_WAVES)), dim3(SR_BLOCK), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK("inject_select");
  return TDR_OK;
}
