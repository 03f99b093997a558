// tdr_grid.hip — pose-grid search (include/tdr.h, "pose-grid search"): the kernels around the scoring launch
// that score one scan over a lattice of map cells and find the peaks of the resulting weight plane.
//   the list: the lattice points that stand on a map cell (with road_only: a road cell), ascending: the count / running sum
//     / write of tdr_compact_dev.h behind the predicate GridListed, as the road list and the injected-slot list are built.
//   grid_candidates_kernel: lane = candidate q = (e - first) * H + h.  One 4-byte load from the list, seven coalesced vector
//     stores: consecutive lanes write consecutive words of a plane, whole lines.
//   grid_reduce_kernel: H > 1: one wave per listed point picks with tdr_wave_pick, the pick rule of sensor resetting; lane 0
//     writes W and T, the lanes stride over the vol column (one 4-byte store per plane h: scattered, the price of the
//     [h][g] layout).  H == 1: one lane per point, no reduction.
//   grid_nms_kernel: a 16 x 16 tile of lattice points with its halo of R points a side in LDS (at most 48 x 48 words) as
//     the integer bits of the eligible weights (positive floats order like their bits; 0 = not eligible).  A point is a peak
//     iff no other point of its window holds larger bits, or equal bits at a smaller g.  The peak's sort key
//     (bits << 32 | ~g) goes to the key plane (0: no peak), the count to one 64-bit integer atomic per wave with a peak.
//   The ordered top K: rocPRIM's descending radix sort of the key plane (the order (w descending, g ascending) is total, so
//     the sorted keys are unique), then grid_emit_kernel writes the first K nonzero keys as tdr_grid_peak.
#include <rocprim/device/device_radix_sort.hpp>

#include "tdr_common.h"
#include "tdr_compact_dev.h"

namespace {
using namespace tdrcmp;
constexpr int GR_BLOCK = 256;
constexpr int GR_WAVES = GR_BLOCK / 64;
constexpr int GR_TILE = 16;          // GR_TILE * GR_TILE == GR_BLOCK
constexpr int GR_MAX_R = 16;
constexpr int GR_SIDE = GR_TILE + 2 * GR_MAX_R;
constexpr int GR_MAX_H = 4096;
constexpr int GR_MAX_K = 4096;
constexpr int64_t GR_MAX_POINTS = (int64_t)1 << 24;

struct GridGeom {   // where lattice point g stands
  int32_t c0, r0, step, nx;
  int32_t rows, cols;
  int64_t G;
  __device__ __forceinline__ void cell(int64_t g, int64_t* c, int64_t* r) const {
    const int64_t iy = g / nx, ix = g - iy * nx;
    *c = (int64_t)c0 + ix * step;
    *r = (int64_t)r0 + iy * step;
  }
};

struct GridListed {   // the predicate of the list (tdr_compact_dev.h)
  GridGeom geo;
  const float* rec;   // the map's records, read with road_only alone
  int32_t rf, road_only;
  __device__ __forceinline__ bool operator()(int64_t g) const {
    if (g >= geo.G) return false;
    int64_t c, r;
    geo.cell(g, &c, &r);
    if (c < 0 || r < 0 || c >= geo.cols || r >= geo.rows) return false;
    if (!road_only) return true;
    return rec[((r + 1) * ((int64_t)geo.cols + 2) + (c + 1)) * rf + 1] < 1.f;   // the road list's test (tdr_recover.hip)
  }
};

struct GridCandArgs {
  GridGeom geo;
  const int32_t* list;
  int64_t first, m;
  int32_t H, heading_mode;
  float theta0, dtheta, scale, resolution;
  float* cst;
  int64_t cand_cap;
};

__global__ __launch_bounds__(GR_BLOCK) void grid_candidates_kernel(GridCandArgs a) {
  const int64_t q = (int64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
  if (q >= a.m * a.H) return;   // m * H <= cand_cap (the launcher's check)
  const int64_t e = q / a.H;
  const int h = (int)(q - e * a.H);
  int64_t g = a.list[a.first + e];
  if (g < 0 || g >= a.geo.G) g = 0;   // (a list that is not this lattice's)
  int64_t c, r;
  a.geo.cell(g, &c, &r);
  float theta = 0.f, have = 0.f;
  if (a.heading_mode == 1) {
    theta = a.theta0 + (float)h * a.dtheta;
    have = 1.f;
  }
  float* o = a.cst + q;
  o[TDR_ST_INIT_X * a.cand_cap] = ((float)c + 0.5f) * a.resolution;
  o[TDR_ST_INIT_Y * a.cand_cap] = ((float)r + 0.5f) * a.resolution;
  o[TDR_ST_DX * a.cand_cap] = 0.f;
  o[TDR_ST_DY * a.cand_cap] = 0.f;
  o[TDR_ST_THETA * a.cand_cap] = theta;
  o[TDR_ST_SCALE * a.cand_cap] = a.scale;
  o[TDR_ST_HAVE_INIT * a.cand_cap] = have;
}

struct GridReduceArgs {
  const int32_t* list;
  int64_t first, m, G;
  int32_t H;
  const float* cst;
  int64_t cand_cap;
  const float* craw;
  float *W, *T, *vol;   // vol may be NULL
};

__device__ __forceinline__ void grid_reduce_write(const GridReduceArgs& a, int64_t g, int64_t q, float w) {
  a.W[g] = w;
  a.T[g] = a.cst[TDR_ST_HAVE_INIT * a.cand_cap + q] != 0.f ? a.cst[TDR_ST_THETA * a.cand_cap + q] : __builtin_nanf("");
}

__global__ __launch_bounds__(GR_BLOCK) void grid_reduce_kernel(GridReduceArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t e = (int64_t)blockIdx.x * GR_WAVES + wave;   // wave-uniform
  if (e >= a.m) return;
  const int64_t g = a.list[a.first + e];
  if (g < 0 || g >= a.G) return;   // (a list that is not this lattice's)
  const float* w = a.craw + e * a.H;
  const int bh = tdr_wave_pick(w, a.H, lane);
  if (lane == 0) grid_reduce_write(a, g, e * a.H + bh, w[bh]);
  if (a.vol)
    for (int h = lane; h < a.H; h += 64) a.vol[(int64_t)h * a.G + g] = w[h];
}

__global__ __launch_bounds__(GR_BLOCK) void grid_reduce1_kernel(GridReduceArgs a) {   // H == 1: lane = listed point
  const int64_t e = (int64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
  if (e >= a.m) return;
  const int64_t g = a.list[a.first + e];
  if (g < 0 || g >= a.G) return;
  const float w = a.craw[e];
  grid_reduce_write(a, g, e, w);
  if (a.vol) a.vol[g] = w;
}

struct GridPeakArgs {
  GridGeom geo;
  int32_t ny, R, tiles_x;
  const float *W, *T;
  uint64_t* keys;      // [G]
  int64_t* n_peaks;    // device, zeroed by the launcher
};

__global__ __launch_bounds__(GR_BLOCK) void grid_nms_kernel(GridPeakArgs a) {
  __shared__ uint32_t sh[GR_SIDE * GR_SIDE];
  const int nx = a.geo.nx, ny = a.ny, R = a.R, side = GR_TILE + 2 * R;   // R <= GR_MAX_R: side <= GR_SIDE
  const int by = (int)(blockIdx.x / (unsigned)a.tiles_x), bx = (int)(blockIdx.x - (unsigned)by * (unsigned)a.tiles_x);
  const int x0 = bx * GR_TILE - R, y0 = by * GR_TILE - R;
  for (int i = threadIdx.x; i < side * side; i += GR_BLOCK) {
    const int ly = i / side, lx = i - ly * side;
    const int x = x0 + lx, y = y0 + ly;
    uint32_t v = 0;
    if (x >= 0 && y >= 0 && x < nx && y < ny) {
      const float w = a.W[(int64_t)y * nx + x];
      if (w > 0.f) v = __float_as_uint(w);   // eligible; a NaN, 0 and negative values are not
    }
    sh[i] = v;
  }
  __syncthreads();
  const int tx = threadIdx.x & (GR_TILE - 1), ty = threadIdx.x / GR_TILE;
  const int x = bx * GR_TILE + tx, y = by * GR_TILE + ty;
  const bool inside = x < nx && y < ny;
  const uint32_t mine = inside ? sh[(ty + R) * side + tx + R] : 0u;
  bool peak = mine != 0u;
  if (peak) {
    for (int dy = -R; dy <= R; dy++) {
      const uint32_t* row = sh + (ty + R + dy) * side + tx + R;
      for (int dx = -R; dx <= R; dx++) {
        const uint32_t o = row[dx];
        const bool earlier = dy < 0 || (dy == 0 && dx < 0);   // g' < g in row-major order
        if (o > mine || (o == mine && earlier)) peak = false;
      }
    }
  }
  if (inside) {
    const int64_t g = (int64_t)y * nx + x;
    a.keys[g] = peak ? ((uint64_t)mine << 32 | (uint64_t)(0xffffffffu - (uint32_t)g)) : 0ull;
  }
  const int cnt = __popcll(__ballot(peak));
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd((unsigned long long*)a.n_peaks, (unsigned long long)cnt);
}

__global__ __launch_bounds__(GR_BLOCK) void grid_emit_kernel(GridGeom geo, const uint64_t* __restrict__ sorted, int64_t K,
                                                             const float* __restrict__ T, tdr_grid_peak* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
  if (i >= K) return;   // K <= min(max_peaks, G)
  const uint64_t key = sorted[i];
  if (key == 0) return;   // behind the last peak
  const uint32_t g = 0xffffffffu - (uint32_t)key;
  if ((int64_t)g >= geo.G) return;
  int64_t c, r;
  geo.cell(g, &c, &r);   // a peak is listed: its cell lies inside the map
  tdr_grid_peak p;
  p.g = (int32_t)g;
  p.cell = (uint32_t)(r * geo.cols + c);
  p.w = __uint_as_float((uint32_t)(key >> 32));
  p.theta = T[g];
  out[i] = p;
}

// rocPRIM's scratch for a descending sort of G 64-bit keys; 0: the size query failed (no device).  The last answer is kept:
// a caller asks for the same lattice again and again.
size_t grid_sort_tmp_bytes(int64_t G) {
  static thread_local int64_t last_g = -1;
  static thread_local size_t last_bytes = 0;
  if (G == last_g) return last_bytes;
  size_t bytes = 0;
  uint64_t* k = nullptr;
  hipError_t e = rocprim::radix_sort_keys_desc(nullptr, bytes, k, k, (size_t)G, 0u, 64u, (hipStream_t)0, false);
  if (e != hipSuccess) return 0;
  last_g = G;
  last_bytes = std::max<size_t>(bytes, 1);
  return last_bytes;
}

int grid_map_check(const tdr_map_desc* map, bool need_rec, const char* who) {
  if (!map) return fail(TDR_ERR_ARG, "%s: null map", who);
  if (map->rows < 1 || map->cols < 1 || (int64_t)map->rows * map->cols > ((int64_t)1 << 31))
    return fail(TDR_ERR_ARG, "%s: a %d x %d map", who, map->rows, map->cols);
  if (need_rec) {
    if (!map->rec) return fail(TDR_ERR_ARG, "%s: the map has no records", who);
    if (map->ncls < 2) return fail(TDR_ERR_ARG, "%s: class 1 (road) is required for the on-road test", who);
    if (map->rec_floats < map->ncls) return fail(TDR_ERR_ARG, "%s: %d floats a record for %d classes", who, map->rec_floats, map->ncls);
  }
  return TDR_OK;
}
GridGeom grid_geom(const tdr_map_desc* map, const tdr_grid_spec* sp) {
  return GridGeom{sp->c0, sp->r0, sp->step, sp->nx, map ? map->rows : 0, map ? map->cols : 0, (int64_t)sp->nx * sp->ny};
}
int grid_check_window(const char* who, const tdr_grid_spec* sp, int64_t n_list, int64_t first, int64_t m, int64_t cand_cap) {
  const int64_t G = (int64_t)sp->nx * sp->ny;
  if (n_list < 0 || n_list > G) return fail(TDR_ERR_ARG, "%s: a list of %lld of %lld lattice points", who, (long long)n_list, (long long)G);
  if (first < 0 || m < 0 || first + m > n_list)
    return fail(TDR_ERR_ARG, "%s: list entries [%lld, %lld + %lld) of %lld", who, (long long)first, (long long)first, (long long)m,
                (long long)n_list);
  if (m * sp->n_headings > cand_cap)
    return fail(TDR_ERR_ARG, "%s: %lld points x %d headings, room for %lld", who, (long long)m, sp->n_headings, (long long)cand_cap);
  return TDR_OK;
}
}  // namespace

int tdr_grid_spec_check(const tdr_grid_spec* sp, const char* who) {
  if (!sp) return fail(TDR_ERR_ARG, "%s: null spec", who);
  if (sp->step < 1) return fail(TDR_ERR_ARG, "%s: step = %d (>= 1)", who, sp->step);
  if (sp->nx < 1 || sp->ny < 1 || (int64_t)sp->nx * sp->ny > GR_MAX_POINTS)
    return fail(TDR_ERR_ARG, "%s: a lattice of %d x %d points (>= 1 each, at most 2^24 in all)", who, sp->nx, sp->ny);
  if (sp->road_only < 0 || sp->road_only > 1) return fail(TDR_ERR_ARG, "%s: road_only = %d (0 .. 1)", who, sp->road_only);
  if (sp->heading_mode < 0 || sp->heading_mode > 1) return fail(TDR_ERR_ARG, "%s: heading_mode = %d (0 .. 1)", who, sp->heading_mode);
  if (sp->heading_mode == 1) {
    if (sp->n_headings < 1 || sp->n_headings > GR_MAX_H)
      return fail(TDR_ERR_ARG, "%s: n_headings = %d (1 .. %d)", who, sp->n_headings, GR_MAX_H);
    if (!std::isfinite(sp->theta0) || !std::isfinite(sp->dtheta))
      return fail(TDR_ERR_ARG, "%s: theta0 = %g, dtheta = %g (finite)", who, (double)sp->theta0, (double)sp->dtheta);
  } else if (sp->n_headings != 1) {
    return fail(TDR_ERR_ARG, "%s: n_headings = %d (1 with heading_mode 0)", who, sp->n_headings);
  }
  if (!std::isfinite(sp->scale) || !(sp->scale > 0.f)) return fail(TDR_ERR_ARG, "%s: scale = %g (finite, > 0)", who, (double)sp->scale);
  return TDR_OK;
}

extern "C" size_t tdr_grid_list_workspace_bytes(int nx, int ny) {
  if (nx < 1 || ny < 1 || (int64_t)nx * ny > GR_MAX_POINTS) return 0;
  return cmp_workspace_bytes((int64_t)nx * ny);
}

extern "C" int tdr_k_grid_list(const tdr_map_desc* map, const tdr_grid_spec* spec, int32_t* list_out, int64_t* count_dev,
                               void* workspace, int max_blocks, void* stream) {
  if (!list_out || !count_dev || !workspace) return fail(TDR_ERR_ARG, "grid_list: null pointer");
  if (int rc = tdr_grid_spec_check(spec, "grid_list")) return rc;
  if (int rc = grid_map_check(map, spec->road_only != 0, "grid_list")) return rc;
  GridListed a{grid_geom(map, spec), map->rec, map->rec_floats, spec->road_only};
  return cmp_list("grid_list", a, a.geo.G, list_out, count_dev, workspace, max_blocks, (hipStream_t)stream);
}

extern "C" int tdr_k_grid_candidates(const tdr_map_desc* map, const tdr_grid_spec* spec, const int32_t* list, int64_t n_list,
                                     int64_t first, int64_t m, float* cand_st, int64_t cand_cap, void* stream) {
  if (!list || !cand_st) return fail(TDR_ERR_ARG, "grid_candidates: null pointer");
  if (int rc = tdr_grid_spec_check(spec, "grid_candidates")) return rc;
  if (int rc = grid_map_check(map, false, "grid_candidates")) return rc;
  if (int rc = grid_check_window("grid_candidates", spec, n_list, first, m, cand_cap)) return rc;
  if (m == 0) return TDR_OK;
  GridCandArgs a{grid_geom(map, spec), list, first, m, spec->n_headings, spec->heading_mode, spec->theta0, spec->dtheta,
                 spec->scale, map->resolution, cand_st, cand_cap};
  hipLaunchKernelGGL(grid_candidates_kernel, dim3((unsigned)cdiv(m * spec->n_headings, GR_BLOCK)), dim3(GR_BLOCK), 0,
                     (hipStream_t)stream, a);
  LAUNCH_CHECK("grid_candidates");
  return TDR_OK;
}

extern "C" int tdr_k_grid_reduce(const tdr_grid_spec* spec, const int32_t* list, int64_t n_list, int64_t first, int64_t m,
                                 const float* cand_st, int64_t cand_cap, const float* cand_w, float* w_plane, float* theta_plane,
                                 float* vol, void* stream) {
  if (!list || !cand_st || !cand_w || !w_plane || !theta_plane) return fail(TDR_ERR_ARG, "grid_reduce: null pointer");
  if (int rc = tdr_grid_spec_check(spec, "grid_reduce")) return rc;
  if (int rc = grid_check_window("grid_reduce", spec, n_list, first, m, cand_cap)) return rc;
  if (m == 0) return TDR_OK;
  GridReduceArgs a{list, first, m, (int64_t)spec->nx * spec->ny, spec->n_headings, cand_st, cand_cap, cand_w, w_plane, theta_plane, vol};
  if (spec->n_headings == 1) {
    hipLaunchKernelGGL(grid_reduce1_kernel, dim3((unsigned)cdiv(m, GR_BLOCK)), dim3(GR_BLOCK), 0, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(grid_reduce_kernel, dim3((unsigned)cdiv(m, GR_WAVES)), dim3(GR_BLOCK), 0, (hipStream_t)stream, a);
  }
  LAUNCH_CHECK("grid_reduce");
  return TDR_OK;
}

// [keys 8G][sorted 8G][sort scratch]
extern "C" size_t tdr_grid_peaks_workspace_bytes(int nx, int ny) {
  if (nx < 1 || ny < 1 || (int64_t)nx * ny > GR_MAX_POINTS) return 0;
  const int64_t G = (int64_t)nx * ny;
  const size_t tmp = grid_sort_tmp_bytes(G);
  return tmp ? (size_t)(16 * G + 512) + tmp : 0;   // 0: the sort's size could not be asked
}

extern "C" int tdr_k_grid_peaks(const tdr_map_desc* map, const tdr_grid_spec* spec, const float* w_plane, const float* theta_plane,
                                int nms_radius, int max_peaks, tdr_grid_peak* peaks_out, int64_t* n_peaks_dev, void* workspace,
                                void* stream) {
  if (!w_plane || !theta_plane || !n_peaks_dev || !workspace || (max_peaks > 0 && !peaks_out))
    return fail(TDR_ERR_ARG, "grid_peaks: null pointer");
  if (int rc = tdr_grid_spec_check(spec, "grid_peaks")) return rc;
  if (int rc = grid_map_check(map, false, "grid_peaks")) return rc;
  if (nms_radius < 0 || nms_radius > GR_MAX_R) return fail(TDR_ERR_ARG, "grid_peaks: nms_radius = %d (0 .. %d)", nms_radius, GR_MAX_R);
  if (max_peaks < 0 || max_peaks > GR_MAX_K) return fail(TDR_ERR_ARG, "grid_peaks: max_peaks = %d (0 .. %d)", max_peaks, GR_MAX_K);
  hipStream_t s = (hipStream_t)stream;
  const GridGeom geo = grid_geom(map, spec);
  const int64_t G = geo.G;
  size_t tmp_bytes = max_peaks > 0 ? grid_sort_tmp_bytes(G) : 0;
  if (max_peaks > 0 && tmp_bytes == 0) return fail(TDR_ERR_HIP, "grid_peaks: the radix sort's scratch size could not be asked");
  uint64_t* keys = reinterpret_cast<uint64_t*>(workspace);
  uint64_t* sorted = keys + G;
  void* tmp = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(sorted + G) + 255) & ~(uintptr_t)255);
  HIP_TRY(hipMemsetAsync(n_peaks_dev, 0, sizeof(int64_t), s));
  const int tiles_x = (int)cdiv(spec->nx, GR_TILE), tiles_y = (int)cdiv(spec->ny, GR_TILE);
  GridPeakArgs a{geo, spec->ny, nms_radius, tiles_x, w_plane, theta_plane, keys, n_peaks_dev};
  hipLaunchKernelGGL(grid_nms_kernel, dim3((unsigned)((int64_t)tiles_x * tiles_y)), dim3(GR_BLOCK), 0, s, a);
  LAUNCH_CHECK("grid_nms");
  if (max_peaks == 0) return TDR_OK;
  HIP_TRY(rocprim::radix_sort_keys_desc(tmp, tmp_bytes, keys, sorted, (size_t)G, 0u, 64u, s, false));
  const int64_t K = std::min<int64_t>(max_peaks, G);
  hipLaunchKernelGGL(grid_emit_kernel, dim3((unsigned)cdiv(K, GR_BLOCK)), dim3(GR_BLOCK), 0, s, geo, (const uint64_t*)sorted, K,
                     theta_plane, peaks_out);
  LAUNCH_CHECK("grid_emit");
  return TDR_OK;
}
