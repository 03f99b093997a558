// tdr_fuse.hip — map fusion (include/tdr.h, "map fusion"): localised scans vote into per-class count
// planes over the map's cells, and the label pass turns the votes of the dirty tiles into a label image.
//   fuse_votes_kernel   the transpose of getLocalMap + getCostForRot: scan bin (i, j) adds its count to the cell the window
//                       pairs it with (local_map_cell, tdr_local_cell.h: the gather's own device function)
//   fuse_labels_kernel  one workgroup per listed tile: most-voted class per cell, verdict, the image pixel the ingest samples
//   fuse_decay_kernel   v >>= shift on every plane
// Integer atomics only: the planes do not depend on the order of the adds.
#include "tdr_common.h"
#include "tdr_ingest_dev.h"   // ingest_pixel
#include "tdr_local_cell.h"

#define FUSE_T TDR_MAP_INCR_TILE

struct FuseVotesArgs {
  LocalCellArgs g;          // the map's shape / resolution / table; the pose is the job's
  int ncls, nb, nr;         // nb x nr: the table's shape (0: the map has no table, polar jobs vote nothing)
  const tdr_fuse_job* jobs; // device array, or NULL: `one` is the only job
  tdr_fuse_job one;
  uint32_t* votes;          // [ncls][map_rows][map_cols]
  uint32_t* dirty;          // one bit per FUSE_T^2 tile
  unsigned long long* counters;   // [2]: votes added, votes dropped
};

__device__ __forceinline__ uint32_t fuse_count(float v) {
  return (v >= 1.f && v < 2147483648.f) ? (uint32_t)v : 0u;   // NaN, negatives, fractions below 1, 2^31 and above: no vote
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// grid.x * 256 threads cover the bins of the largest scan, grid.y = the job.  Thread = scan bin b = i + rows * j, so the
// reads of a class image are contiguous.  A bin whose classes all vote 0 does no address work (most bins of a lidar
// render are empty).
__global__ __launch_bounds__(256) void fuse_votes_kernel(FuseVotesArgs a) {
  const tdr_fuse_job job = a.jobs ? a.jobs[blockIdx.y] : a.one;   // (uniform)
  const int64_t P = (int64_t)job.rows * job.cols;
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool shape_ok = job.scan != nullptr && job.rows >= 1 && job.cols >= 1 &&
                        (!job.polar || (a.g.tab != nullptr && job.rows == a.nb && job.cols == a.nr));
  unsigned long long added = 0, dropped = 0;
  if (shape_ok && b < P) {
    uint32_t n[TDR_MAX_CLASSES];
    uint32_t any = 0;
#pragma unroll
    for (int c = 0; c < TDR_MAX_CLASSES; c++) {
      n[c] = c < a.ncls ? fuse_count(job.scan[(int64_t)c * P + b]) : 0u;
      any |= n[c];
    }
    if (any) {
      LocalCellArgs g = a.g;
      g.rows = job.rows; g.cols = job.cols; g.cx = job.cx; g.cy = job.cy;
      int ri, ci;
      bool inb;
      if (job.polar) {
        // scan row i pairs with window row (i - s) mod nb (state_particle.cpp:136-142)
        const int i = (int)(b % job.rows), j = (int)(b / job.rows);
        int iw = i - rot_shift_dev(job.theta, job.rows);
        if (iw < 0) iw += job.rows;
        g.scale_or_rot = job.scale; g.res = job.res;
        inb = local_map_cell<true>(g, (int64_t)iw + (int64_t)job.rows * j, ri, ci);
      } else {
        // the Cartesian score's window: rot = theta, res * scale (tdr_k_score_cart), shift 0
        g.scale_or_rot = job.theta; g.res = job.res * job.scale;
        inb = local_map_cell<false>(g, b, ri, ci);
      }
      unsigned long long sum = 0;
#pragma unroll
      for (int c = 0; c < TDR_MAX_CLASSES; c++) sum += n[c];
      if (inb) {
        const int64_t cell = (int64_t)ri * a.g.map_cols + ci, plane = (int64_t)a.g.map_rows * a.g.map_cols;
#pragma unroll
        for (int c = 0; c < TDR_MAX_CLASSES; c++)
          if (n[c]) atomicAdd(a.votes + c * plane + cell, n[c]);
        const int t = (ri / FUSE_T) * ((a.g.map_cols + FUSE_T - 1) / FUSE_T) + ci / FUSE_T;
        const uint32_t bit = 1u << (t & 31);
        if (!(a.dirty[t >> 5] & bit)) atomicOr(a.dirty + (t >> 5), bit);
        added = sum;
      } else {
        dropped = sum;
      }
    }
  }
  added = wave_sum_u64(added);
  dropped = wave_sum_u64(dropped);
  if ((threadIdx.x & 63) == 0) {
    if (added) atomicAdd(a.counters, added);
    if (dropped) atomicAdd(a.counters + 1, dropped);
  }
}

static int launch_votes(const tdr_map_desc* map, const float* tab, int nb, int nr, const tdr_fuse_job* jobs_dev,
                        const tdr_fuse_job* one, int k, int64_t max_bins, uint32_t* votes, uint32_t* dirty,
                        uint64_t* counters, void* stream) {
  if (!map || !votes || !dirty || !counters) return fail(TDR_ERR_ARG, "fuse_votes: null pointer");
  if (map->ncls < 1 || map->ncls > TDR_MAX_CLASSES || map->rows < 1 || map->cols < 1 || !(map->resolution > 0.f))
    return fail(TDR_ERR_ARG, "fuse_votes: bad map shape / resolution");
  if (k < 1 || k > 65535) return fail(TDR_ERR_ARG, "fuse_votes: %d jobs (1 .. 65535)", k);
  if (max_bins < 1 || max_bins > ((int64_t)1 << 31)) return fail(TDR_ERR_ARG, "fuse_votes: bad max_bins");
  if (tab ? (nb < 1 || nr < 1) : (nb != 0 || nr != 0)) return fail(TDR_ERR_ARG, "fuse_votes: bad table shape");
  FuseVotesArgs a{};
  a.g.map_rows = map->rows; a.g.map_cols = map->cols; a.g.resolution = map->resolution; a.g.tab = tab;
  a.g.libm_fma = tdr_libm_fma();
  a.ncls = map->ncls; a.nb = nb; a.nr = nr;
  a.jobs = jobs_dev;
  if (one) a.one = *one;
  a.votes = votes; a.dirty = dirty; a.counters = (unsigned long long*)counters;
  hipLaunchKernelGGL(fuse_votes_kernel, dim3((unsigned)cdiv(max_bins, 256), (unsigned)k), dim3(256), 0,
                     (hipStream_t)stream, a);
  LAUNCH_CHECK("fuse_votes");
  return TDR_OK;
}

extern "C" int tdr_k_fuse_votes_jobs(const tdr_map_desc* map, const float* tab, int nb, int nr,
                                     const tdr_fuse_job* jobs_dev, int k, int64_t max_bins, uint32_t* votes,
                                     uint32_t* dirty, uint64_t* counters, void* stream) {
  if (!jobs_dev) return fail(TDR_ERR_ARG, "fuse_votes_jobs: null jobs");
  return launch_votes(map, tab, nb, nr, jobs_dev, nullptr, k, max_bins, votes, dirty, counters, stream);
}

extern "C" int tdr_k_fuse_votes(const tdr_map_desc* map, const float* tab, int nb, int nr, const float* scan, int polar,
                                int rows, int cols, float cx, float cy, float theta, float scale, float res,
                                uint32_t* votes, uint32_t* dirty, uint64_t* counters, void* stream) {
  if (!scan) return fail(TDR_ERR_ARG, "fuse_votes: null scan");
  if (rows < 1 || cols < 1) return fail(TDR_ERR_ARG, "fuse_votes: bad scan shape");
  if (polar && (!tab || rows != nb || cols != nr))
    return fail(TDR_ERR_ARG, "fuse_votes: a polar scan of %d x %d bins on a table of %d x %d", rows, cols, nb, nr);
  tdr_fuse_job one{};
  one.scan = scan; one.rows = rows; one.cols = cols; one.polar = polar ? 1 : 0;
  one.cx = cx; one.cy = cy; one.theta = theta; one.scale = scale; one.res = res;
  return launch_votes(map, tab, nb, nr, nullptr, &one, 1, (int64_t)rows * cols, votes, dirty, counters, stream);
}

// ---- labels ---------------------------------------------------------------------------------------------------------------------
struct FuseLabelsArgs {
  const uint32_t* votes;
  int ncls, rows, cols, img_h, img_w;
  float resolution;
  uint8_t class_label[TDR_MAX_CLASSES + 1];
  uint32_t min_votes, share_num, share_den;
  const uint8_t* base;
  uint8_t* current;
  const int32_t* tiles;
  int32_t* out;   // [5]: changed pixels, y min, x min, y max, x max
};
__device__ __forceinline__ int wave_red(int v, int kind) {   // 0: sum, 1: min, 2: max
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int o = __shfl_xor(v, d, 64);
    v = kind == 0 ? v + o : (kind == 1 ? (o < v ? o : v) : (o > v ? o : v));
  }
  return v;
}
__global__ __launch_bounds__(256) void fuse_labels_kernel(FuseLabelsArgs a) {
  const int t = a.tiles[blockIdx.x], tx_n = (a.cols + FUSE_T - 1) / FUSE_T;
  const int ty = t / tx_n, tx = t - ty * tx_n;
  const int64_t plane = (int64_t)a.rows * a.cols;
  int changed = 0, y0 = 0x7fffffff, x0 = 0x7fffffff, y1 = -1, x1 = -1;
  for (int e = threadIdx.x; e < FUSE_T * FUSE_T; e += 256) {
    const int yi = ty * FUSE_T + e / FUSE_T, xi = tx * FUSE_T + e % FUSE_T;
    if (t < 0 || ty >= (a.rows + FUSE_T - 1) / FUSE_T || yi >= a.rows || xi >= a.cols) continue;
    const int64_t cell = (int64_t)yi * a.cols + xi;
    uint64_t total = 0;
    uint32_t best = 0;
    int w = 0;
    for (int c = 0; c < a.ncls; c++) {
      const uint32_t v = a.votes[c * plane + cell];
      total += v;
      if (v > best) { best = v; w = c; }   // strict: the lowest class on a tie
    }
    const bool verdict = total >= (uint64_t)a.min_votes && (uint64_t)best * a.share_den >= total * a.share_num;
    const int64_t pix = ingest_pixel(yi, xi, a.img_h, a.img_w, a.resolution);
    const uint8_t label = verdict ? a.class_label[w] : a.base[pix];
    if (a.current[pix] != label) {
      a.current[pix] = label;
      const int py = (int)(pix / a.img_w), px = (int)(pix - (int64_t)py * a.img_w);
      changed++;
      y0 = py < y0 ? py : y0; y1 = py > y1 ? py : y1;
      x0 = px < x0 ? px : x0; x1 = px > x1 ? px : x1;
    }
  }
  changed = wave_red(changed, 0);
  y0 = wave_red(y0, 1); x0 = wave_red(x0, 1);
  y1 = wave_red(y1, 2); x1 = wave_red(x1, 2);
  if ((threadIdx.x & 63) == 0 && changed) {
    atomicAdd(a.out, changed);
    atomicMin(a.out + 1, y0); atomicMin(a.out + 2, x0);
    atomicMax(a.out + 3, y1); atomicMax(a.out + 4, x1);
  }
}

extern "C" int tdr_k_fuse_labels(const uint32_t* votes, int ncls, int rows, int cols, int img_h, int img_w,
                                 float resolution, const uint8_t* class_label_host, uint32_t min_votes,
                                 uint32_t share_num, uint32_t share_den, const uint8_t* base, uint8_t* current,
                                 const int32_t* tiles, int n_tiles, int32_t* out5, void* stream) {
  if (!votes || !class_label_host || !base || !current || !tiles || !out5) return fail(TDR_ERR_ARG, "fuse_labels: null pointer");
  if (ncls < 1 || ncls > TDR_MAX_CLASSES || rows < 1 || cols < 1 || img_h < 1 || img_w < 1)
    return fail(TDR_ERR_ARG, "fuse_labels: bad shape");
  if (!(resolution >= 1.f)) return fail(TDR_ERR_ARG, "fuse_labels: map resolution %g (cells map to pixels one to one from 1 on)", (double)resolution);
  int mr = 0, mc = 0;
  if (tdr_map_ingest_shape(img_h, img_w, resolution, &mr, &mc) != TDR_OK || mr != rows || mc != cols)
    return fail(TDR_ERR_ARG, "fuse_labels: a %d x %d image at resolution %g is not a %d x %d map", img_h, img_w,
                (double)resolution, rows, cols);
  if (min_votes < 1 || share_den < 1 || share_num > share_den) return fail(TDR_ERR_ARG, "fuse_labels: bad verdict rule");
  if (n_tiles < 0 || n_tiles > tdr_map_incr_tiles(rows, cols)) return fail(TDR_ERR_ARG, "fuse_labels: bad tile count");
  if (n_tiles == 0) return TDR_OK;
  FuseLabelsArgs a{};
  a.votes = votes; a.ncls = ncls; a.rows = rows; a.cols = cols; a.img_h = img_h; a.img_w = img_w; a.resolution = resolution;
  std::memcpy(a.class_label, class_label_host, (size_t)ncls);
  a.min_votes = min_votes; a.share_num = share_num; a.share_den = share_den;
  a.base = base; a.current = current; a.tiles = tiles; a.out = out5;
  hipLaunchKernelGGL(fuse_labels_kernel, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK("fuse_labels");
  return TDR_OK;
}

// ---- decay / reset --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fuse_decay_kernel(uint32_t* votes, int ncls, int rows, int cols, int shift,
                                                         uint32_t* dirty) {
  const int64_t plane = (int64_t)rows * cols, cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= plane) return;
  uint32_t any = 0;
  for (int c = 0; c < ncls; c++) {
    const uint32_t v = votes[c * plane + cell];
    any |= v;
    if (v) votes[c * plane + cell] = shift >= 32 ? 0u : v >> shift;
  }
  if (any) {
    const int ri = (int)(cell / cols), ci = (int)(cell - (int64_t)ri * cols);
    const int t = (ri / FUSE_T) * ((cols + FUSE_T - 1) / FUSE_T) + ci / FUSE_T;
    const uint32_t bit = 1u << (t & 31);
    if (!(dirty[t >> 5] & bit)) atomicOr(dirty + (t >> 5), bit);
  }
}
extern "C" int tdr_k_fuse_decay(uint32_t* votes, int ncls, int rows, int cols, int shift, uint32_t* dirty, void* stream) {
  if (!votes || !dirty) return fail(TDR_ERR_ARG, "fuse_decay: null pointer");
  if (ncls < 1 || ncls > TDR_MAX_CLASSES || rows < 1 || cols < 1 || shift < 0) return fail(TDR_ERR_ARG, "fuse_decay: bad arguments");
  if (shift == 0) return TDR_OK;
  hipLaunchKernelGGL(fuse_decay_kernel, dim3((unsigned)cdiv((int64_t)rows * cols, 256)), dim3(256), 0, (hipStream_t)stream,
                     votes, ncls, rows, cols, shift, dirty);
  LAUNCH_CHECK("fuse_decay");
  return TDR_OK;
}
