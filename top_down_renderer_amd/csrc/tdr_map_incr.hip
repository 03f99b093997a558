// tdr_map_incr.hip — incremental label-image map updates: rebuild only the cells a new image can change, bit for bit.
//
// Why it is exact.  Distances are truncated at 50 (src/top_down_map.cpp:315), so a cell's record depends only on the
// class words inside the (2R+1)^2 box around it, R = ceil(50 / resolution) (the windowed passes of tdr_map.hip rest on
// the same fact).  A cell whose word did not change and that has no changed cell within R keeps its record bit for bit.
// The update works on 32 x 32-cell tiles, which line up with every derived tiling: the known mask's 32 x 32 tiles, the
// class planes' 8 x 8 tiles, the coarse mask's 4 x 4 blocks and the compact records' 4-column tiles.
//
//   incr_detect_kernel    the class word of every cell of the new image (ingest_label_word, tdr_ingest_dev.h) against the
//                         stored one: changed-tile flags + changed-cell count (read back; the host forms the tile lists)
//   incr_commit_kernel    the new words of the changed tiles into the stored words
//   incr_coldist_kernel   the column pass over the changed tiles dilated vertically by ceil(R/32) tiles: a column
//                         distance changes only within R rows of a changed cell of its own column; the others, kept in
//                         the ingest workspace from the last ingest, are still current
//   incr_rowmin_kernel    the row pass over the AFFECTED tiles (changed tiles dilated by ceil(R/32) both ways); with a
//                         compact form it also moves the dictionary's occurrence counts from old values to new ones
//   incr_compact_kernel   the compact records, known mask, class planes and coarse mask of the affected tiles
// The stored words and column distances are the ingest workspace of tdr_k_map_from_labels, which leaves them there.
//
// The dictionary must stay the full build's (tdr_cmap.hip: every distinct value of the map, sorted).  The counts say how
// many (cell, class) values of the guarded grid equal each entry — the values cmap_collect_kernel inserts.  A new value
// that is not in the dictionary, or an entry whose count reaches 0, changes the dictionary: the caller then rebuilds the
// compact form whole (tdr_k_compact_map) and the counts with it.
#include <algorithm>
#include <vector>

#include "tdr_common.h"
#include "tdr_ingest_dev.h"
#include "tdr_score_dev.h"   // the known mask's and the planes' geometry

#define INCR_T TDR_MAP_INCR_TILE   // tile side in cells (tdr.h)
#define INCR_STATUS_BYTES 64   // u64 [0] changed cells, [1] a value outside the dictionary, [2] an entry of count <= 0

static inline int incr_tiles_x(int cols) { return (cols + INCR_T - 1) / INCR_T; }
static inline int incr_tiles_y(int rows) { return (rows + INCR_T - 1) / INCR_T; }
static inline size_t incr_align(size_t n) { return (n + 255) & ~(size_t)255; }

extern "C" int tdr_map_incr_tiles(int rows, int cols) {
  if (rows < 1 || cols < 1) return 0;
  return incr_tiles_x(cols) * incr_tiles_y(rows);
}
extern "C" size_t tdr_map_incr_workspace_bytes(int rows, int cols) {
  const size_t nt = (size_t)tdr_map_incr_tiles(rows, cols);
  return INCR_STATUS_BYTES + incr_align(nt) + 3 * nt * sizeof(int32_t) + 256;
}

// dictionary index of the value with bits v: entry 0 = +0.0f, entries [1, n) ascending by bit pattern (cmap_dictionary);
// -1 when the value is not there
__device__ inline int incr_dict_find(const float* __restrict__ dict, int n, unsigned v) {
  if (v == 0u) return 0;
  int lo = 1, hi = n - 1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    const unsigned m = __float_as_uint(dict[mid]);
    if (m == v) return mid;
    if (m < v) lo = mid + 1;
    else hi = mid - 1;
  }
  return -1;
}

__global__ __launch_bounds__(256) void incr_detect_kernel(const uint8_t* __restrict__ img, int img_h, int img_w,
                                                          const int32_t* __restrict__ lut, int lut_size, int ncls,
                                                          int rows, int cols, float resolution,
                                                          const uint32_t* __restrict__ cls, int tiles_x,
                                                          uint8_t* __restrict__ flags,
                                                          unsigned long long* __restrict__ changed) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int diff = 0;
  if (idx < (int64_t)rows * cols) {
    const int y = (int)(idx / cols), x = (int)(idx % cols);
    if (ingest_label_word(img, img_h, img_w, lut, lut_size, ncls, y, x, resolution) != cls[idx]) {
      diff = 1;
      flags[(y / INCR_T) * tiles_x + x / INCR_T] = 1;
    }
  }
  const int n = __syncthreads_count(diff);
  if (threadIdx.x == 0 && n) atomicAdd(changed, (unsigned long long)n);
}

// the kernels below take one tile of a list per workgroup: tile t = (t / tiles_x, t % tiles_x), cell i of it = row i / 32,
// column i % 32 (a wave covers two rows of 32 consecutive cells)
__global__ __launch_bounds__(256) void incr_commit_kernel(const uint8_t* __restrict__ img, int img_h, int img_w,
                                                          const int32_t* __restrict__ lut, int lut_size, int ncls,
                                                          int rows, int cols, float resolution,
                                                          const int32_t* __restrict__ tiles, int tiles_x,
                                                          uint32_t* __restrict__ cls) {
  const int t = tiles[blockIdx.x], ty = t / tiles_x, tx = t - ty * tiles_x;
  for (int i = threadIdx.x; i < INCR_T * INCR_T; i += blockDim.x) {
    const int y = ty * INCR_T + (i >> 5), x = tx * INCR_T + (i & 31);
    if (y < rows && x < cols)
      cls[(int64_t)y * cols + x] = ingest_label_word(img, img_h, img_w, lut, lut_size, ncls, y, x, resolution);
  }
}

__global__ __launch_bounds__(256) void incr_coldist_kernel(const uint32_t* __restrict__ cls, int rows, int cols, int R,
                                                           const int32_t* __restrict__ tiles, int tiles_x,
                                                           uint8_t* __restrict__ g) {
  const int t = tiles[blockIdx.x], ty = t / tiles_x, tx = t - ty * tiles_x;
  for (int i = threadIdx.x; i < INCR_T * INCR_T; i += blockDim.x) {
    const int y = ty * INCR_T + (i >> 5), x = tx * INCR_T + (i & 31);
    if (y < rows && x < cols) ingest_coldist_cell(cls, rows, cols, R, y, x, g);
  }
}

__global__ __launch_bounds__(256) void incr_rowmin_kernel(const uint32_t* __restrict__ cls, const uint8_t* __restrict__ g,
                                                          int ncls, int rows, int cols, int R, float resolution, int rf,
                                                          const int32_t* __restrict__ tiles, int tiles_x,
                                                          float* __restrict__ rec, const float* __restrict__ dict,
                                                          int dict_n, int* __restrict__ counts,
                                                          unsigned long long* __restrict__ status) {
  // the workgroup's count changes are summed in LDS first: most moves go between a few entries (the truncation value
  // and its neighbours), and one global atomic per entry and tile instead of per cell keeps them off a few L2 lines
  __shared__ int delta[TDR_CMAP_WIDE_MAX_DICT];
  if (counts) {
    for (int j = threadIdx.x; j < dict_n; j += blockDim.x) delta[j] = 0;
    __syncthreads();
  }
  const int t = tiles[blockIdx.x], ty = t / tiles_x, tx = t - ty * tiles_x;
  for (int i = threadIdx.x; i < INCR_T * INCR_T; i += blockDim.x) {
    const int y = ty * INCR_T + (i >> 5), x = tx * INCR_T + (i & 31);
    if (y >= rows || x >= cols) continue;
    float d[INGEST_MAXC];
    const float known = ingest_rowmin_cell(cls, g, ncls, cols, R, resolution, y, x, d);
    float* o = rec + ((int64_t)(y + 1) * (cols + 2) + (x + 1)) * rf;
#pragma unroll
    for (int c = 0; c < INGEST_MAXC; c++) {
      if (c >= ncls) continue;
      const unsigned ov = __float_as_uint(o[c]), nv = __float_as_uint(d[c]);
      if (counts && ov != nv) {
        const int io = incr_dict_find(dict, dict_n, ov), in = incr_dict_find(dict, dict_n, nv);
        if (io >= 0) atomicSub(&delta[io], 1);
        else atomicExch(&status[1], 1ull);   // (cannot happen while the counts describe this map)
        if (in >= 0) atomicAdd(&delta[in], 1);
        else atomicExch(&status[1], 1ull);   // a value the dictionary lacks
      }
      o[c] = d[c];
    }
    o[rf - 1] = known;
    if (tdr_has_kslot(ncls, rf)) o[rf - 2] = known;
  }
  if (counts) {
    __syncthreads();
    for (int j = threadIdx.x; j < dict_n; j += blockDim.x)
      if (delta[j]) atomicAdd(&counts[j], delta[j]);
  }
}

__global__ __launch_bounds__(256) void incr_zero_check_kernel(const int* __restrict__ counts, int dict_n,
                                                              unsigned long long* __restrict__ status) {
  for (int i = threadIdx.x; i < dict_n; i += blockDim.x)
    if (counts[i] <= 0) atomicExch(&status[2], 1ull);
}

struct IncrCompactGeom {
  int cw, lc, tiles_r;     // compact records (cmap_geom, tdr_cmap.hip)
  int wide;
  int kmask_col_words;     // 32 * kmask_trows(rows); 0: no known mask (wide form)
  int plane_tr;            // plane_trows(rows)
  int64_t plane_cells;     // 16-bit cells of one class plane (2 * tdr_cmap_plane_words); 0: no planes
};
// the same fields as cmap_pack_kernel / cmap_kmask_kernel / cmap_plane_kernel / cmap_cmask_kernel write for the cells of one
// affected tile; cells outside the map keep the zeros of the full build
__global__ __launch_bounds__(256) void incr_compact_kernel(const float* __restrict__ rec, int rows, int cols, int rf,
                                                           int ncls, const float* __restrict__ dict, int dict_n,
                                                           const int32_t* __restrict__ tiles, int tiles_x,
                                                           IncrCompactGeom g, uint32_t* __restrict__ crec,
                                                           uint32_t* __restrict__ kmask, uint16_t* __restrict__ planes,
                                                           uint16_t* __restrict__ cmask) {
  const int t = tiles[blockIdx.x], ty = t / tiles_x, tx = t - ty * tiles_x;
  for (int i = threadIdx.x; i < INCR_T * INCR_T; i += blockDim.x) {
    const int r = ty * INCR_T + (i >> 5), c = tx * INCR_T + (i & 31);
    if (r >= rows || c >= cols) continue;
    const float* src = rec + ((int64_t)(r + 1) * (cols + 2) + (c + 1)) * rf;
    const bool known = src[rf - 1] != 0.f;
    const int64_t pt = planes ? ((int64_t)((c >> 3) + 1) * g.plane_tr + ((r >> 3) + 1)) * 64 + (r & 7) * 8 + (c & 7) : 0;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < ncls; k++) {
      int j = incr_dict_find(dict, dict_n, __float_as_uint(src[k]));
      j = j < 0 ? 0 : j;   // (every value is there: the caller checked)
      if (g.wide) w[k / 2] |= ((uint32_t)j << 2) << (16 * (k & 1));
      else w[k / 3] |= (uint32_t)j << (2 + 10 * (k % 3));
      if (planes) planes[(int64_t)k * g.plane_cells + pt] = (uint16_t)(((unsigned)j << 2) | (known ? 0x8000u : 0u));
    }
    if (known) {
      w[g.cw - 1] |= 1u;
      if (!g.wide)
        for (int d = 0; d < g.cw - 1; d++) w[d] |= 1u;
    }
    const int64_t tile = (int64_t)((c >> 2) + 1) * g.tiles_r + ((r >> g.lc) + 1);
    const int within = ((r & ((1 << g.lc) - 1)) << 2) | (c & 3);
    for (int d = 0; d < g.cw; d++) crec[(tile * (4 << g.lc) + within) * g.cw + d] = w[d];
  }
  if (kmask && threadIdx.x < INCR_T) {   // one word per row of the tile
    const int r = ty * INCR_T + threadIdx.x, c0 = tx * INCR_T;
    if (r < rows) {
      uint32_t bits = 0;
      for (int b = 0; b < 32; b++) {
        const int c = c0 + b;
        if (c < cols && rec[((int64_t)(r + 1) * (cols + 2) + (c + 1)) * rf + rf - 1] != 0.f) bits |= 1u << b;
      }
      kmask[(int64_t)(tx + 1) * g.kmask_col_words + r + 32] = bits;
    }
  }
  if (cmask && threadIdx.x >= 64 && threadIdx.x < 128) {   // the tile's 8 x 8 blocks of 4 x 4 cells
    const int i = threadIdx.x - 64;
    const int R = ty * 8 + (i >> 3), C = tx * 8 + (i & 7);
    if (R * 4 < rows && C * 4 < cols) {
      uint16_t v = 0;
      for (int b = 0; b < 16; b++) {
        const int r = R * 4 + (b >> 2), c = C * 4 + (b & 3);
        if (r < rows && c < cols && rec[((int64_t)(r + 1) * (cols + 2) + (c + 1)) * rf + rf - 1] != 0.f) v |= (uint16_t)(1u << b);
      }
      cmask[((int64_t)((C >> 3) + 1) * g.plane_tr + ((R >> 3) + 1)) * 64 + (R & 7) * 8 + (C & 7)] = v;
    }
  }
}

// occurrence counts of the dictionary's entries over every (cell, class) value of the guarded grid
__global__ __launch_bounds__(256) void incr_count_kernel(const float* __restrict__ rec, int64_t gcell, int rf, int ncls,
                                                         const float* __restrict__ dict, int dict_n,
                                                         int* __restrict__ counts) {
  __shared__ int hist[TDR_CMAP_WIDE_MAX_DICT];
  for (int i = threadIdx.x; i < dict_n; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < gcell; idx += (int64_t)gridDim.x * blockDim.x) {
    const float* src = rec + idx * rf;
    unsigned last = __float_as_uint(src[0]);
    int run = 1;
    for (int k = 1; k <= ncls; k++) {   // runs of equal values (the truncation distance) cost one atomic
      const unsigned v = k < ncls ? __float_as_uint(src[k]) : ~last;
      if (k < ncls && v == last) { run++; continue; }
      const int j = incr_dict_find(dict, dict_n, last);
      if (j >= 0) atomicAdd(&hist[j], run);
      last = v;
      run = 1;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < dict_n; i += blockDim.x)
    if (hist[i]) atomicAdd(&counts[i], hist[i]);
}

// the cells of listed tiles, each tile column-major like class_maps_: maps_out [n][ncls][32 * 32] (cell (rl, cl) of the
// tile at cl * 32 + rl), mask_out [n][32 * 32] (1 = unknown); cells outside the map are not written
__global__ __launch_bounds__(256) void incr_gather_kernel(const float* __restrict__ rec, int ncls, int rows, int cols, int rf,
                                                          const int32_t* __restrict__ tiles, int tiles_x,
                                                          float* __restrict__ maps_out, uint8_t* __restrict__ mask_out) {
  const int t = tiles[blockIdx.x], ty = t / tiles_x, tx = t - ty * tiles_x;
  for (int i = threadIdx.x; i < INCR_T * INCR_T; i += blockDim.x) {
    const int r = ty * INCR_T + (i & 31), c = tx * INCR_T + (i >> 5);
    if (r >= rows || c >= cols) continue;
    const float* src = rec + ((int64_t)(r + 1) * (cols + 2) + (c + 1)) * rf;
    for (int k = 0; k < ncls; k++) maps_out[((int64_t)blockIdx.x * ncls + k) * (INCR_T * INCR_T) + i] = src[k];
    mask_out[(int64_t)blockIdx.x * (INCR_T * INCR_T) + i] = src[rf - 1] != 0.f ? 0 : 1;
  }
}

extern "C" int tdr_k_map_dict_counts(const tdr_map_desc* map, int32_t* counts, void* stream) {
  if (!map || !map->rec || !map->dict || !counts || !map->cwords || map->dict_n < 1 || map->dict_n > TDR_CMAP_WIDE_MAX_DICT)
    return fail(TDR_ERR_ARG, "map_dict_counts: the map has no compact form / null pointer");
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int32_t) * TDR_CMAP_WIDE_MAX_DICT, s));
  const int64_t gcell = (int64_t)(map->rows + 2) * (map->cols + 2);
  const int64_t blocks = std::min<int64_t>(cdiv(gcell, 256), 2048);
  hipLaunchKernelGGL(incr_count_kernel, dim3((unsigned)blocks), dim3(256), 0, s, map->rec, gcell, map->rec_floats, map->ncls,
                     map->dict, map->dict_n, (int*)counts);
  LAUNCH_CHECK("map_dict_counts");
  return TDR_OK;
}

extern "C" int tdr_k_map_gather_tiles(const float* rec, int ncls, int rows, int cols, const int32_t* tiles, int n_tiles,
                                      float* maps_out, uint8_t* mask_out, void* stream) {
  if (!rec || !tiles || !maps_out || !mask_out || ncls < 1 || ncls > TDR_MAX_CLASSES || rows < 1 || cols < 1 || n_tiles < 0 ||
      n_tiles > tdr_map_incr_tiles(rows, cols))
    return fail(TDR_ERR_ARG, "map_gather_tiles: bad arguments");
  if (n_tiles == 0) return TDR_OK;
  hipLaunchKernelGGL(incr_gather_kernel, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)stream, rec, ncls, rows, cols,
                     tdr_rec_floats(ncls), tiles, incr_tiles_x(cols), maps_out, mask_out);
  LAUNCH_CHECK("map_gather_tiles");
  return TDR_OK;
}

// flags[ty][tx] dilated by d tiles along y (and along x too when both) -> the list of set tiles
static void incr_dilate(const std::vector<uint8_t>& in, int ty_n, int tx_n, int d, bool both, std::vector<int32_t>& out) {
  std::vector<uint8_t> v((size_t)ty_n * tx_n, 0);
  std::vector<int> pre((size_t)std::max(ty_n, tx_n) + 1);
  for (int x = 0; x < tx_n; x++) {   // along y: a prefix count per tile column
    pre[0] = 0;
    for (int y = 0; y < ty_n; y++) pre[y + 1] = pre[y] + (in[(size_t)y * tx_n + x] ? 1 : 0);
    for (int y = 0; y < ty_n; y++) v[(size_t)y * tx_n + x] = pre[std::min(ty_n, y + d + 1)] - pre[std::max(0, y - d)] > 0;
  }
  out.clear();
  for (int y = 0; y < ty_n; y++) {
    const uint8_t* row = v.data() + (size_t)y * tx_n;
    pre[0] = 0;
    for (int x = 0; x < tx_n; x++) pre[x + 1] = pre[x] + row[x];
    for (int x = 0; x < tx_n; x++) {
      const bool set = both ? pre[std::min(tx_n, x + d + 1)] - pre[std::max(0, x - d)] > 0 : row[x] != 0;
      if (set) out.push_back(y * tx_n + x);
    }
  }
}

extern "C" int tdr_k_map_update_labels(const uint8_t* label_img, int img_h, int img_w, const int32_t* flatten_lut,
                                       int lut_size, tdr_map_desc* map, void* ingest_ws, int32_t* dict_counts,
                                       int64_t max_cells, void* workspace, int32_t* tiles_out, int* n_tiles,
                                       int64_t* changed_cells, int* compact_ok, void* stream) {
  if (!label_img || !flatten_lut || !map || !map->rec || !ingest_ws || !workspace || !tiles_out || !n_tiles ||
      !changed_cells || !compact_ok)
    return fail(TDR_ERR_ARG, "map_update_labels: null pointer");
  const int ncls = map->ncls, rows = map->rows, cols = map->cols, rf = map->rec_floats;
  const float resolution = map->resolution;
  if (ncls < 1 || ncls > TDR_MAX_CLASSES || lut_size < 1 || lut_size > 256 || rf != tdr_rec_floats(ncls))
    return fail(TDR_ERR_ARG, "map_update_labels: bad class count / lut size");
  int ir = 0, ic = 0;
  if (int rc = tdr_map_ingest_shape(img_h, img_w, resolution, &ir, &ic)) return rc;
  if (ir != rows || ic != cols)
    return fail(TDR_ERR_ARG, "map_update_labels: a %d x %d image at resolution %g is not this %d x %d map", img_w, img_h,
                resolution, cols, rows);
  const int R = (int)std::ceil(50.0 / (double)resolution);
  if (R > 250) return fail(TDR_ERR_ARG, "map_update_labels: resolution %g needs a %d-cell window (max 250)", resolution, R);
  if (map->cwords && (!dict_counts || !map->crec || !map->dict))
    return fail(TDR_ERR_ARG, "map_update_labels: a map with a compact form needs its dictionary counts");
  *n_tiles = 0;
  *changed_cells = 0;
  *compact_ok = 0;
  hipStream_t s = (hipStream_t)stream;
  const int tx_n = incr_tiles_x(cols), ty_n = incr_tiles_y(rows), nt = tx_n * ty_n;
  unsigned long long* status = reinterpret_cast<unsigned long long*>(workspace);
  uint8_t* flags = reinterpret_cast<uint8_t*>(workspace) + INCR_STATUS_BYTES;
  int32_t* lists = reinterpret_cast<int32_t*>(flags + incr_align(nt));
  uint32_t* cls = reinterpret_cast<uint32_t*>(ingest_ws);   // the layout of tdr_k_map_from_labels' workspace
  uint8_t* g = reinterpret_cast<uint8_t*>(ingest_ws) + (((size_t)rows * cols * 4 + 255) & ~(size_t)255);
  const int64_t ncell = (int64_t)rows * cols;

  // 1. which tiles hold a cell whose class word changed
  HIP_TRY(hipMemsetAsync(workspace, 0, INCR_STATUS_BYTES + incr_align(nt), s));
  hipLaunchKernelGGL(incr_detect_kernel, dim3((unsigned)cdiv(ncell, 256)), dim3(256), 0, s, label_img, img_h, img_w,
                     flatten_lut, lut_size, ncls, rows, cols, resolution, (const uint32_t*)cls, tx_n, flags, status);
  LAUNCH_CHECK("map_update_labels: detect");
  unsigned long long st[3] = {0, 0, 0};
  std::vector<uint8_t> hflags((size_t)nt);
  HIP_TRY(hipMemcpyAsync(st, status, sizeof(st), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hflags.data(), flags, (size_t)nt, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *changed_cells = (int64_t)st[0];
  if (st[0] == 0) {
    *compact_ok = 1;
    return TDR_OK;
  }
  // 2. the tile lists: changed, column pass (dilated along y), affected (dilated both ways)
  const int D = (R + INCR_T - 1) / INCR_T;
  std::vector<int32_t> chg, col, aff;
  for (int t = 0; t < nt; t++)
    if (hflags[(size_t)t]) chg.push_back(t);
  incr_dilate(hflags, ty_n, tx_n, D, false, col);
  incr_dilate(hflags, ty_n, tx_n, D, true, aff);
  if (max_cells >= 0 && (int64_t)aff.size() * INCR_T * INCR_T > max_cells) {
    *n_tiles = -1;   // the caller's full ingest is cheaper; nothing on the device has changed
    return TDR_OK;
  }
  std::copy(aff.begin(), aff.end(), tiles_out);
  *n_tiles = (int)aff.size();
  std::vector<int32_t> hl;
  hl.reserve(chg.size() + col.size() + aff.size());
  hl.insert(hl.end(), chg.begin(), chg.end());
  hl.insert(hl.end(), col.begin(), col.end());
  hl.insert(hl.end(), aff.begin(), aff.end());
  HIP_TRY(hipMemcpyAsync(lists, hl.data(), hl.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  const int32_t* d_chg = lists;
  const int32_t* d_col = lists + chg.size();
  const int32_t* d_aff = lists + chg.size() + col.size();
  // 3. the windowed distance transform
  const bool counted = map->cwords != 0;
  hipLaunchKernelGGL(incr_commit_kernel, dim3((unsigned)chg.size()), dim3(256), 0, s, label_img, img_h, img_w, flatten_lut,
                     lut_size, ncls, rows, cols, resolution, d_chg, tx_n, cls);
  hipLaunchKernelGGL(incr_coldist_kernel, dim3((unsigned)col.size()), dim3(256), 0, s, (const uint32_t*)cls, rows, cols, R,
                     d_col, tx_n, g);
  hipLaunchKernelGGL(incr_rowmin_kernel, dim3((unsigned)aff.size()), dim3(256), 0, s, (const uint32_t*)cls,
                     (const uint8_t*)g, ncls, rows, cols, R, resolution, rf, d_aff, tx_n, const_cast<float*>(map->rec),
                     map->dict, counted ? map->dict_n : 0, counted ? (int*)dict_counts : (int*)nullptr, status);
  LAUNCH_CHECK("map_update_labels: distance transform");
  // 4. the compact form, when the dictionary stays what it was
  if (!counted) {
    *compact_ok = tdr_cmap_words_total(ncls, rows, cols) == 0 ? 1 : 0;   // a map that may gain a compact form: rebuild
  } else {
    hipLaunchKernelGGL(incr_zero_check_kernel, dim3(1), dim3(256), 0, s, (const int*)dict_counts, map->dict_n, status);
    LAUNCH_CHECK("map_update_labels: dictionary check");
    HIP_TRY(hipMemcpyAsync(st, status, sizeof(st), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!st[1] && !st[2]) {
      const int wide = (map->cwords == 4 && rf == 8 && map->dict_n > TDR_CMAP_MAX_DICT) ? 1 : 0;
      IncrCompactGeom cg;
      cg.cw = map->cwords;
      cg.lc = cg.cw == 1 ? 3 : (cg.cw == 2 ? 2 : 1);
      cg.tiles_r = (rows >> cg.lc) + 2;
      cg.wide = wide;
      uint32_t* crec = const_cast<uint32_t*>(map->crec);
      const size_t tiles_words = (size_t)cg.tiles_r * ((cols >> 2) + 2) * 32;
      uint32_t* kmask = wide ? nullptr : crec + tiles_words;
      cg.kmask_col_words = kmask_trows(rows) * 32;
      cg.plane_tr = plane_trows(rows);
      const size_t pw = wide ? 0 : tdr_cmap_plane_words(ncls, rows, cols);
      cg.plane_cells = (int64_t)pw * 2;
      uint16_t* planes = pw ? reinterpret_cast<uint16_t*>(crec + tdr_cmap_plane_offset_words(ncls, rows, cols)) : nullptr;
      uint16_t* cmask = pw ? planes + (size_t)ncls * pw * 2 : nullptr;
      hipLaunchKernelGGL(incr_compact_kernel, dim3((unsigned)aff.size()), dim3(256), 0, s, (const float*)map->rec, rows,
                         cols, rf, ncls, map->dict, map->dict_n, d_aff, tx_n, cg, crec, kmask, planes, cmask);
      LAUNCH_CHECK("map_update_labels: compact form");
      *compact_ok = 1;
    }
  }
  HIP_TRY(hipStreamSynchronize(s));   // hl lives on this stack frame until the copy is done
  return TDR_OK;
}
