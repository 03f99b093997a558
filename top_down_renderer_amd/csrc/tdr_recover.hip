// tdr_recover.hip — recovery injection (include/tdr.h, "recovery injection"): the road list of a map and
// the kernel that overwrites a random share of a filter's slots with fresh on-road particles.
//   road list: the cells whose class-1 slot is below 1 (ini_on_road's predicate, tdr_init.hip), in ascending cell index.
//     the count / running sum / write of tdr_compact_dev.h behind the predicate RoadCell: the order is the cell order
//     whatever the grid does.
//   inject_kernel: lane = slot.  The Philox words of a slot depend on (seed, draw, slot, purpose) alone (tdr_philox.h), so
//     the result does not depend on the grid, the wave order or the rank.  One 4-byte load from the road list per injected
//     lane (scattered by nature), vector stores to the planes of injected slots only, ballot + bit count per wave and one
//     64-bit integer atomic per wave that injected something.
#include "tdr_common.h"
#include "tdr_compact_dev.h"
#include "tdr_philox.h"

namespace {
constexpr int REC_BLOCK = 256;
constexpr int INJ_MAX_BLOCKS = 2048;    // grid.x: a workgroup strides over its job's slots beyond that
constexpr int INJ_JOBS_BLOCKS_X = 256;  // ... and the grid.x of a job table, whose sizes the host does not see

struct RoadCell {   // the predicate of the road list (tdr_compact_dev.h)
  const float* rec;
  int rf, cols;
  int64_t ncell;
  __device__ __forceinline__ bool operator()(int64_t i) const {
    if (i >= ncell) return false;
    const int64_t r = i / cols, c = i - r * cols;
    return rec[((r + 1) * (cols + 2) + (c + 1)) * rf + 1] < 1.f;
  }
};

struct InjectArgs {
  const tdr_inject_job* jobs;   // DEVICE, or NULL: `one`
  tdr_inject_job one;
};

__global__ __launch_bounds__(REC_BLOCK) void inject_kernel(InjectArgs a) {
  const tdr_inject_job job = a.jobs ? a.jobs[blockIdx.y] : a.one;
  const int64_t n = job.n, cap = job.cap;
  if (job.threshold24 == 0 || job.n_road < 1) return;   // nothing is injected, nothing is counted
  const uint32_t k0 = (uint32_t)job.seed, k1 = (uint32_t)(job.seed >> 32);
  const uint32_t d0 = (uint32_t)job.draw, d1 = (uint32_t)(job.draw >> 32);
  unsigned injected = 0;   // wave-uniform
  // every lane of the workgroup makes every turn (the bound is the workgroup's): the ballot sees whole waves
  for (int64_t p0 = (int64_t)blockIdx.x * REC_BLOCK; p0 < n; p0 += (int64_t)gridDim.x * REC_BLOCK) {
    const int64_t p = p0 + threadIdx.x;
    bool inj = false;
    if (p < n) {
      const uint32_t slot = (uint32_t)(job.slot_begin + p);
      const TdrPhilox4 w = tdr_philox4x32(slot, d0, d1, 0u, k0, k1);
      inj = (w.w[0] >> 8) < job.threshold24;
      if (inj) {
        const uint32_t cell = job.road[(uint64_t)w.w[1] * (uint64_t)job.n_road >> 32];   // < n_road
        const uint32_t r = cell / (uint32_t)job.cols, c = cell - r * (uint32_t)job.cols;
        const float ux = (float)(w.w[2] >> 24) * 0x1p-8f, uy = (float)(w.w[3] >> 24) * 0x1p-8f;
        float* o = job.st + p;
        o[TDR_ST_INIT_X * cap] = ((float)c + ux) * job.resolution;
        o[TDR_ST_INIT_Y * cap] = ((float)r + uy) * job.resolution;
        o[TDR_ST_DX * cap] = 0.f;
        o[TDR_ST_DY * cap] = 0.f;
        float theta = 0.f, have = 0.f;
        if (job.heading_mode == 1) {
          const TdrPhilox4 b = tdr_philox4x32(slot, d0, d1, 1u, k0, k1);
          theta = (float)(b.w[0] >> 8) * 0x1p-24f * 6.2831855f - 3.1415927f;
          have = 1.f;
        }
        o[TDR_ST_THETA * cap] = theta;
        o[TDR_ST_HAVE_INIT * cap] = have;
      }
    }
    injected += (unsigned)__popcll(__ballot(inj));
  }
  if ((threadIdx.x & 63) == 0 && injected && job.injected) atomicAdd((unsigned long long*)job.injected, (unsigned long long)injected);
}

int road_check(const tdr_map_desc* map, const char* who) {
  if (!map || !map->rec) return fail(TDR_ERR_ARG, "%s: null map", who);
  if (map->ncls < 2) return fail(TDR_ERR_ARG, "%s: class 1 (road) is required for the on-road test", who);
  if (map->rows < 1 || map->cols < 1 || (int64_t)map->rows * map->cols > ((int64_t)1 << 31) || map->rec_floats < map->ncls)
    return fail(TDR_ERR_ARG, "%s: a %d x %d map of %d floats a record", who, map->rows, map->cols, map->rec_floats);
  return TDR_OK;
}
}  // namespace

extern "C" size_t tdr_map_road_workspace_bytes(int rows, int cols) {
  if (rows < 1 || cols < 1) return 0;
  return (size_t)cdiv((int64_t)rows * cols, REC_BLOCK) * sizeof(int64_t);
}

extern "C" int tdr_k_map_road_cells(const tdr_map_desc* map, uint32_t* cells_out, int64_t* count_dev, void* workspace,
                                    void* stream) {
  if (int rc = road_check(map, "map_road_cells")) return rc;
  if (!cells_out || !count_dev || !workspace) return fail(TDR_ERR_ARG, "map_road_cells: null pointer");
  hipStream_t s = (hipStream_t)stream;
  RoadCell a{map->rec, map->rec_floats, map->cols, (int64_t)map->rows * map->cols};
  return tdrcmp::cmp_list("map_road_cells", a, a.ncell, cells_out, count_dev, workspace, 0, s);
}

extern "C" uint32_t tdr_inject_threshold_host(double p) {
  const double v = std::floor(p * 16777216.0);
  if (!(v > 0.)) return 0;   // (a NaN too)
  return v >= 16777216.0 ? 16777216u : (uint32_t)v;
}

extern "C" void tdr_philox4x32_host(const uint32_t c[4], const uint32_t k[2], uint32_t out[4]) {
  const TdrPhilox4 w = tdr_philox4x32(c[0], c[1], c[2], c[3], k[0], k[1]);
  for (int i = 0; i < 4; i++) out[i] = w.w[i];
}

extern "C" int tdr_k_inject(float* st, int64_t cap, int64_t n, int64_t slot_begin, const tdr_map_desc* map,
                            const uint32_t* road, int64_t n_road, uint64_t seed, uint64_t draw, uint32_t threshold24,
                            int heading_mode, int64_t* injected_dev, void* stream) {
  if (int rc = road_check(map, "inject")) return rc;
  if (!st || !road) return fail(TDR_ERR_ARG, "inject: null pointer");
  if (n < 0 || cap < n || slot_begin < 0 || slot_begin + n > ((int64_t)1 << 31))
    return fail(TDR_ERR_ARG, "inject: slots [%lld, %lld + %lld) of cap = %lld (global index < 2^31)", (long long)slot_begin,
                (long long)slot_begin, (long long)n, (long long)cap);
  if (n_road < 1 || n_road > (int64_t)map->rows * map->cols) return fail(TDR_ERR_ARG, "inject: %lld road cells", (long long)n_road);
  if (threshold24 > (1u << 24)) return fail(TDR_ERR_ARG, "inject: threshold24 = %u (0 .. 2^24)", threshold24);
  if (heading_mode < 0 || heading_mode > 1) return fail(TDR_ERR_ARG, "inject: heading_mode = %d (0 .. 1)", heading_mode);
  if (n == 0 || threshold24 == 0) return TDR_OK;
  InjectArgs a{};
  a.one = tdr_inject_job{st, cap, n, slot_begin, road, n_road, map->cols, map->resolution, seed, draw, threshold24, heading_mode,
                         injected_dev};
  hipLaunchKernelGGL(inject_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n, REC_BLOCK), INJ_MAX_BLOCKS)), dim3(REC_BLOCK), 0,
                     (hipStream_t)stream, a);
  LAUNCH_CHECK("inject");
  return TDR_OK;
}

extern "C" int tdr_k_inject_jobs(const tdr_inject_job* jobs_dev, int n_jobs, void* stream) {
  if (!jobs_dev) return fail(TDR_ERR_ARG, "inject_jobs: null jobs");
  if (n_jobs < 0 || n_jobs > 65535) return fail(TDR_ERR_ARG, "inject_jobs: %d jobs (0 .. 65535)", n_jobs);
  if (n_jobs == 0) return TDR_OK;
  InjectArgs a{};
  a.jobs = jobs_dev;
  // the jobs' sizes live on the device: a fixed grid.x, and a workgroup past its job's slots leaves at once
  hipLaunchKernelGGL(inject_kernel, dim3(INJ_JOBS_BLOCKS_X, (unsigned)n_jobs), dim3(REC_BLOCK), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK("inject_jobs");
  return TDR_OK;
}
