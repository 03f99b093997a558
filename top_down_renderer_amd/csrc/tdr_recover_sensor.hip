// tdr_recover_sensor.hip — sensor-resetting recovery (include/tdr.h, "sensor resetting"): the three kernels
// around the scoring launch that give every injected slot the best-scoring of C road candidates.
//   the list: the slots tdr_k_inject would inject, ascending: the count / running sum / write of tdr_compact_dev.h behind
//     the predicate SrListed, as the road list (tdr_recover.hip) and the lattice list (tdr_grid.hip) are built.
//   sr_candidates_kernel: lane = candidate.  Candidate j of a slot draws the words the plain injection draws with purposes
//     2j (position) and 2j + 1 (heading), so candidate 0 is that injection's particle; one 4-byte load from the road list
//     per candidate, coalesced vector stores to the candidate planes.
//   sr_select_kernel: one wave per listed slot picks with tdr_wave_pick (tdr_compact_dev.h): every lane keeps the best of
//     its stride of the C weights in ascending j, the wave then reduces on (key, -j) with a butterfly of shuffles.  Lanes
//     0..6 copy the winner's seven fields into the slot.
#include "tdr_common.h"
#include "tdr_compact_dev.h"
#include "tdr_philox.h"

namespace {
using namespace tdrcmp;
constexpr int SR_BLOCK = 256;
constexpr int SR_WAVES = SR_BLOCK / 64;
constexpr int SR_MAX_CAND = 4096;

struct SrListed {   // the predicate of the list (tdr_compact_dev.h)
  int64_t n, slot_begin;
  uint32_t k0, k1, d0, d1, threshold24;
  __device__ __forceinline__ bool operator()(int64_t p) const {
    if (p >= n) return false;
    const TdrPhilox4 w = tdr_philox4x32((uint32_t)(slot_begin + p), d0, d1, 0u, k0, k1);
    return (w.w[0] >> 8) < threshold24;
  }
};

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
  const int bj = tdr_wave_pick(w, a.C, lane);   // the same on every lane, < C
  const int64_t p = a.list[a.first + e];
  if (p < 0 || p >= a.n) return;   // (a list that is not this filter's)
  if (lane < TDR_ST_FIELDS) a.st[(int64_t)lane * a.cap + p] = a.cst[(int64_t)lane * a.cand_cap + e * a.C + bj];
  if (lane == 0 && a.pick_out) a.pick_out[e] = bj;
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
  return cmp_workspace_bytes(n);
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
  SrListed a{n, slot_begin, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)draw, (uint32_t)(draw >> 32), threshold24};
  return cmp_list("inject_list", a, n, list_out, count_dev, workspace, max_blocks, s);
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
