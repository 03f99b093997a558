// tdr_poly.hip — the static vector map's fill on the device: TopDownMap::getRasterMap + samplePts + getClasses
// (src/top_down_map.cpp:328-365, 367-408) for polygons given per flattened class.
//
// The reference evaluates, for every cell (i, j) of the rows x cols map and every edge (a = v[k], b = v[k-1 cyclic]) of
// every polygon, "the edge crosses the cell's ray":
//     (py_i < a.y) != (py_i < b.y)  &&  px_j < a.x + ((b.x - a.x) * (py_i - a.y)) / (b.y - a.y)
// (py_i depends on the row only, px_j on the column only; f32, no FMA, IEEE division) and keeps the cells with an odd
// crossing count: O(cells x edges).  Here the same test is a scanline problem, O(crossings + cells x classes):
//   host   k_v = #{i : py_i < v.y} per vertex (binary search; the row table does not decrease, checked): an edge crosses
//          exactly rows [min(k_a, k_b), max(k_a, k_b)); per polygon the rows it spans.  Edges are laid out by a prefix
//          of their row counts (one record per (row, edge) crossing), polygons by a prefix of their spans (one BIN per
//          (row, polygon)).
//   K1     per crossing: xc with the reference's expression, J = #{j : px_j < xc} (binary search in the column table;
//          NaN xc compares false everywhere: J = 0), counted into its bin.
//   scan   bin starts (rocprim exclusive scan); K2 scatters the J's into their bins.
//   K3     per bin: sort its J's; cell j is inside the polygon iff #{k : J_k > j} is odd, i.e. the cells
//          [J_{m-1}, J_m), [J_{m-3}, J_{m-2}), ..., and [0, J_1) when m is odd.  Each interval adds +1 / -1 to the class's
//          integer difference row (atomics on integers: the sum is order-independent, the result is deterministic).
//   K4-K6  per (row, 64-column chunk): prefix of the difference rows -> count > 0 = inside any polygon of the class
//          (the reference's max over polygons), exclusive classes, the class plane (0 inside, 1 elsewhere) column-major
//          like Eigen's class_maps_; K7 transposes it into the raster-cache layout tdr_k_map_from_rasters ingests.
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "tdr_common.h"

namespace {

// Eigen's LinSpaced<float>(n, low, high) coefficient i (the same as tdr_map.hip's)
float linspaced(int i, int n, float low, float high) {
  const int size1 = (n == 1) ? 1 : n - 1;
  const float step = (n == 1) ? 0.0f : (high - low) / (float)(n - 1);
  if (fabsf(high) < fabsf(low)) return (i == 0) ? low : (high - (float)(size1 - i) * step);
  return (i == size1) ? high : (low + (float)i * step);
}

struct Edge {
  float ax, ay, bx, by;
  int32_t row0;   // first row crossed
  int32_t poly;   // polygon index (into PolyInfo)
};
struct PolyInfo {
  int32_t row0;   // first row of the polygon's span
  int32_t bin0;   // its first bin
  int32_t cls;
};

template <class T>
struct DBuf {
  T* p = nullptr;
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  int alloc(size_t n) {
    hipError_t e = hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return fail(TDR_ERR_NOMEM, "poly_fill: hipMalloc(%zu bytes): %s", n * sizeof(T), hipGetErrorString(e));
    }
    return TDR_OK;
  }
  ~DBuf() {
    if (p) (void)hipFree(p);
  }
};
#define PTRY(expr)                 \
  do {                             \
    int rc_ = (expr);              \
    if (rc_ != TDR_OK) return rc_; \
  } while (0)

__device__ __forceinline__ int count_below(const float* __restrict__ tab, int n, float v) {   // #{k : tab[k] < v}
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// K1: one thread per (row, edge) crossing
__global__ void poly_cross_kernel(const Edge* __restrict__ edges, const int32_t* __restrict__ eoff, int n_edges,
                                  const PolyInfo* __restrict__ polys, const float* __restrict__ py,
                                  const float* __restrict__ px, int cols, int32_t n_cross, int32_t* __restrict__ rec_bin,
                                  int32_t* __restrict__ rec_j, int32_t* __restrict__ bin_cnt) {
  const int32_t t = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= n_cross) return;
  int lo = 0, hi = n_edges;   // the edge: last e with eoff[e] <= t
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (eoff[mid] <= t) lo = mid;
    else hi = mid;
  }
  const Edge e = edges[lo];
  const int row = e.row0 + (t - eoff[lo]);
  const float y = py[row];
  // top_down_map.cpp:341-342, every operation rounded to f32 in this order (-ffp-contract=off, IEEE division)
  const float xc = e.ax + __fdiv_rn((e.bx - e.ax) * (y - e.ay), e.by - e.ay);
  const int J = count_below(px, cols, xc);
  const PolyInfo p = polys[e.poly];
  const int32_t bin = p.bin0 + (row - p.row0);
  rec_bin[t] = bin;
  rec_j[t] = J;
  atomicAdd(&bin_cnt[bin], 1);
}

// K2: the J's into their bins (any order inside a bin: K3 sorts)
__global__ void poly_scatter_kernel(const int32_t* __restrict__ rec_bin, const int32_t* __restrict__ rec_j,
                                    int32_t n_cross, const int32_t* __restrict__ bin_start, int32_t* __restrict__ bin_cnt,
                                    int32_t* __restrict__ sorted) {
  const int32_t t = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= n_cross) return;
  const int32_t b = rec_bin[t];
  const int32_t slot = atomicSub(&bin_cnt[b], 1) - 1;
  sorted[bin_start[b] + slot] = rec_j[t];
}

__device__ void sift_down(int32_t* a, int root, int n) {
  while (true) {
    int c = 2 * root + 1;
    if (c >= n) return;
    if (c + 1 < n && a[c + 1] > a[c]) c++;
    if (a[root] >= a[c]) return;
    const int32_t t = a[root];
    a[root] = a[c];
    a[c] = t;
    root = c;
  }
}

// K3: one thread per (row, polygon) bin: sort, pair, +1 / -1 into the class's difference row.  diff layout:
// [cls][col][row] (a column of the map is contiguous, like the planes)
__global__ void poly_pair_kernel(const int32_t* __restrict__ bin_start, int32_t n_bins, int32_t n_cross,
                                 const PolyInfo* __restrict__ polys, int n_polys, int32_t* __restrict__ sorted, int rows,
                                 int cols, int32_t* __restrict__ diff) {
  const int32_t b = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= n_bins) return;
  int lo = 0, hi = n_polys;   // the polygon: last p with bin0 <= b (every listed polygon has a bin)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (polys[mid].bin0 <= b) lo = mid;
    else hi = mid;
  }
  const PolyInfo p = polys[lo];
  const int row = p.row0 + (b - p.bin0);
  const int32_t s0 = bin_start[b], s1 = (b + 1 < n_bins) ? bin_start[b + 1] : n_cross;
  int32_t* a = sorted + s0;
  const int m = s1 - s0;
  if (m <= 16) {
    for (int i = 1; i < m; i++) {
      const int32_t v = a[i];
      int k = i - 1;
      while (k >= 0 && a[k] > v) { a[k + 1] = a[k]; k--; }
      a[k + 1] = v;
    }
  } else {   // heap sort: O(m log m) for any polygon
    for (int r = m / 2 - 1; r >= 0; r--) sift_down(a, r, m);
    for (int n = m - 1; n > 0; n--) {
      const int32_t t = a[0]; a[0] = a[n]; a[n] = t;
      sift_down(a, 0, n);
    }
  }
  int32_t* d = diff + (size_t)p.cls * cols * rows;
  for (int k = m - 1; k >= 0; k -= 2) {
    const int s = k >= 1 ? a[k - 1] : 0, e = a[k];
    if (s >= e) continue;
    atomicAdd(&d[(size_t)s * rows + row], 1);
    if (e < cols) atomicAdd(&d[(size_t)e * rows + row], -1);
  }
}

#define POLY_CHUNK 64
// K4: per (row, column chunk, class): the chunk's sum of the difference row
__global__ void poly_chunk_sum_kernel(const int32_t* __restrict__ diff, int ncls, int rows, int cols, int nchunk,
                                      int32_t* __restrict__ csum) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)ncls * nchunk * rows) return;
  const int i = (int)(t % rows);
  const int64_t ck = t / rows;   // c * nchunk + k
  const int k = (int)(ck % nchunk), c = (int)(ck / nchunk);
  const int j0 = k * POLY_CHUNK, j1 = min(cols, j0 + POLY_CHUNK);
  const int32_t* d = diff + (size_t)c * cols * rows;
  int32_t s = 0;
  for (int j = j0; j < j1; j++) s += d[(size_t)j * rows + i];
  csum[t] = s;
}
// K5: per (class, row): exclusive prefix over the chunks, in place
__global__ void poly_chunk_prefix_kernel(int32_t* __restrict__ csum, int ncls, int rows, int nchunk) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)ncls * rows) return;
  const int i = (int)(t % rows), c = (int)(t / rows);
  int32_t run = 0;
  for (int k = 0; k < nchunk; k++) {
    int32_t* q = csum + ((size_t)c * nchunk + k) * rows + i;
    const int32_t v = *q;
    *q = run;
    run += v;
  }
}
// K6: per (row, column chunk): running counts of every class, exclusive classes, the planes
__global__ void poly_planes_kernel(const int32_t* __restrict__ diff, const int32_t* __restrict__ csum, int ncls, int rows,
                                   int cols, int nchunk, const uint32_t* __restrict__ excl_above,
                                   uint8_t* __restrict__ planes) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nchunk * rows) return;
  const int i = (int)(t % rows), k = (int)(t / rows);
  int32_t run[TDR_MAX_CLASSES];
  uint32_t above[TDR_MAX_CLASSES];
#pragma unroll
  for (int c = 0; c < TDR_MAX_CLASSES; c++) {
    run[c] = c < ncls ? csum[((size_t)c * nchunk + k) * rows + i] : 0;
    above[c] = c < ncls ? excl_above[c] : 0u;
  }
  const size_t ncell = (size_t)rows * cols;
  const int j0 = k * POLY_CHUNK, j1 = min(cols, j0 + POLY_CHUNK);
  for (int j = j0; j < j1; j++) {
    const size_t cell = (size_t)j * rows + i;
    uint32_t in = 0;
#pragma unroll
    for (int c = 0; c < TDR_MAX_CLASSES; c++)
      if (c < ncls) {
        run[c] += diff[(size_t)c * ncell + cell];
        in |= (run[c] > 0 ? 1u : 0u) << c;
      }
    uint32_t clear = 0;   // getClasses :356-365: u is cleared where a later-listed class c > u lies
#pragma unroll
    for (int c = 0; c < TDR_MAX_CLASSES; c++) clear |= (in & above[c]) ? (1u << c) : 0u;
    in &= ~clear;
#pragma unroll
    for (int c = 0; c < TDR_MAX_CLASSES; c++)
      if (c < ncls) planes[(size_t)c * ncell + cell] = (in >> c) & 1u ? 0 : 1;
  }
}
// K7: column-major 0 / 1 planes -> the raster cache's images: [cls][rows][cols] row-major, row 0 = the map's last row
// (saveRasterizedMaps flips, :208), 0 inside and 255 elsewhere (convertTo(CV_8UC1, 255), :206)
__global__ void poly_raster_kernel(const uint8_t* __restrict__ planes, int rows, int cols, uint8_t* __restrict__ raster) {
  __shared__ uint8_t tile[64][65];
  const int c = blockIdx.z;
  const int i0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
  const size_t ncell = (size_t)rows * cols;
  const uint8_t* src = planes + (size_t)c * ncell;
  uint8_t* dst = raster + (size_t)c * ncell;
  for (int q = threadIdx.x; q < 64 * 64; q += blockDim.x) {
    const int ii = q & 63, jj = q >> 6;   // read down a column
    const int i = i0 + ii, j = j0 + jj;
    if (i < rows && j < cols) tile[jj][ii] = src[(size_t)j * rows + i];
  }
  __syncthreads();
  for (int q = threadIdx.x; q < 64 * 64; q += blockDim.x) {
    const int jj = q & 63, ii = q >> 6;   // write along a row
    const int i = i0 + ii, j = j0 + jj;
    if (i < rows && j < cols) dst[(size_t)(rows - 1 - i) * cols + j] = tile[jj][ii] ? 255 : 0;
  }
}

}  // namespace

// rows / cols of the reference's getRasterMap for an image of W x H px (Eigen::Vector2i map_size = (int) of the SVG's
// float size): class_map(int(H / res), int(W / res)), int / float in f32 (:395-396)
int tdr_poly_grid(int width, int height, float resolution, int* rows, int* cols) {
  if (width < 1 || height < 1 || !(resolution > 0.f) || !std::isfinite(resolution))
    return fail(TDR_ERR_ARG, "map_load_polygons: bad size %d x %d / resolution %g", width, height, (double)resolution);
  const float r = (float)height / resolution, c = (float)width / resolution;
  if (!(r >= 1.f) || !(c >= 1.f) || r > 1048576.f || c > 1048576.f)
    return fail(TDR_ERR_ARG, "map_load_polygons: a %g x %g cell map is empty or too large", (double)r, (double)c);
  *rows = (int)r;
  *cols = (int)c;
  return TDR_OK;
}

// The fill itself (load-time work: allocates, synchronises).  verts / offs / cls: HOST polygons (vertex (x, y) pairs;
// polygon p = vertices [offs[p], offs[p+1]), class cls[p]; polygons of a class outside [0, ncls) are skipped);
// excl_above[u] = bits of the exclusive classes c > u when u itself is in the list, else 0.  Writes the DEVICE arrays
// planes_cm [ncls][rows*cols] (column-major, 0 inside / 1 elsewhere) and, unless NULL, raster [ncls][rows][cols] (the
// class<i>.png layout tdr_k_map_from_rasters reads).
int tdr_poly_fill(const float* verts, const int64_t* offs, const int32_t* cls, int64_t n_poly, int width, int height,
                  float resolution, int ncls, const uint32_t* excl_above, uint8_t* planes_cm, uint8_t* raster,
                  hipStream_t s) {
  int rows = 0, cols = 0;
  PTRY(tdr_poly_grid(width, height, resolution, &rows, &cols));
  // samplePts(center = map_size / 2, rot = 0, ..., cols, rows, res) (:399, :367-389): the row coordinate is
  // LinSpaced(rows, -res (rows-1) / 2, res (rows-1) / 2)[i] + H / 2, the column one the same over cols + W / 2 (the
  // identity rotation adds signed zeros only)
  const float cx = (float)width / 2.f, cy = (float)height / 2.f;
  const float lo_r = (float)((double)(-resolution * (float)(rows - 1)) / 2.),
              hi_r = (float)((double)(resolution * (float)(rows - 1)) / 2.);
  const float lo_c = (float)((double)(-resolution * (float)(cols - 1)) / 2.),
              hi_c = (float)((double)(resolution * (float)(cols - 1)) / 2.);
  std::vector<float> py(rows), px(cols);
  for (int i = 0; i < rows; i++) py[i] = linspaced(i, rows, lo_r, hi_r) + cy;
  for (int j = 0; j < cols; j++) px[j] = linspaced(j, cols, lo_c, hi_c) + cx;
  // both tables rise (LinSpaced over a symmetric range is monotone): the ranges below rely on it
  for (int i = 1; i < rows; i++)
    if (!(py[i - 1] <= py[i])) return fail(TDR_ERR_ARG, "map_load_polygons: row coordinates decrease at %d", i);
  for (int j = 1; j < cols; j++)
    if (!(px[j - 1] <= px[j])) return fail(TDR_ERR_ARG, "map_load_polygons: column coordinates decrease at %d", j);

  // host plan: rows per vertex, crossings per edge, bins per polygon
  std::vector<Edge> edges;
  std::vector<int32_t> eoff;
  std::vector<PolyInfo> polys;
  std::vector<int32_t> kv;
  int64_t n_cross = 0, n_bins = 0;
  for (int64_t p = 0; p < n_poly; p++) {
    if (cls[p] < 0 || cls[p] >= ncls) continue;
    const int64_t v0 = offs[p], v1 = offs[p + 1];
    const int64_t n = v1 - v0;
    if (n < 2) continue;   // one vertex: its only edge is a point, never crossed
    kv.resize((size_t)n);
    int32_t rmin = INT32_MAX, rmax = INT32_MIN;
    for (int64_t k = 0; k < n; k++) {
      const float y = verts[2 * (v0 + k) + 1];
      kv[(size_t)k] = (int32_t)(std::lower_bound(py.begin(), py.end(), y) - py.begin());   // NaN: 0 (compares false)
      rmin = std::min(rmin, kv[(size_t)k]);
      rmax = std::max(rmax, kv[(size_t)k]);
    }
    if (rmax == rmin) continue;
    const int32_t pi = (int32_t)polys.size();
    polys.push_back(PolyInfo{rmin, (int32_t)n_bins, cls[p]});
    n_bins += rmax - rmin;
    for (int64_t k = 0; k < n; k++) {
      const int64_t kb = k == 0 ? n - 1 : k - 1;   // j = the previous vertex, cyclic (:336-347)
      const int32_t ka = kv[(size_t)k], kbb = kv[(size_t)kb];
      if (ka == kbb) continue;
      const float* a = verts + 2 * (v0 + k);
      const float* b = verts + 2 * (v0 + kb);
      edges.push_back(Edge{a[0], a[1], b[0], b[1], std::min(ka, kbb), pi});
      eoff.push_back((int32_t)n_cross);
      n_cross += std::abs(ka - kbb);
    }
    if (n_cross > INT32_MAX - 1 || n_bins > INT32_MAX - 1)
      return fail(TDR_ERR_ARG, "map_load_polygons: more than 2^31 (row, edge) crossings");
  }
  const size_t ncell = (size_t)rows * cols;
  std::vector<uint32_t> above(TDR_MAX_CLASSES, 0u);
  for (int c = 0; c < ncls; c++) above[c] = excl_above[c];

  DBuf<int32_t> d_diff;
  PTRY(d_diff.alloc(ncell * ncls));
  HIP_TRY(hipMemsetAsync(d_diff.p, 0, ncell * ncls * sizeof(int32_t), s));
  if (n_cross > 0) {
    DBuf<Edge> d_edges;
    DBuf<int32_t> d_eoff, d_rec_bin, d_rec_j, d_cnt, d_start, d_sorted;
    DBuf<PolyInfo> d_polys;
    DBuf<float> d_py, d_px;
    PTRY(d_edges.alloc(edges.size()));
    PTRY(d_eoff.alloc(eoff.size()));
    PTRY(d_polys.alloc(polys.size()));
    PTRY(d_py.alloc(rows));
    PTRY(d_px.alloc(cols));
    PTRY(d_rec_bin.alloc((size_t)n_cross));
    PTRY(d_rec_j.alloc((size_t)n_cross));
    PTRY(d_sorted.alloc((size_t)n_cross));
    PTRY(d_cnt.alloc((size_t)n_bins));
    PTRY(d_start.alloc((size_t)n_bins));
    HIP_TRY(hipMemcpyAsync(d_edges.p, edges.data(), edges.size() * sizeof(Edge), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_eoff.p, eoff.data(), eoff.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_polys.p, polys.data(), polys.size() * sizeof(PolyInfo), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_py.p, py.data(), rows * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_px.p, px.data(), cols * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_cnt.p, 0, (size_t)n_bins * sizeof(int32_t), s));
    const int32_t nc = (int32_t)n_cross, nb = (int32_t)n_bins;
    hipLaunchKernelGGL(poly_cross_kernel, dim3((unsigned)cdiv(nc, 256)), dim3(256), 0, s, d_edges.p, d_eoff.p,
                       (int)edges.size(), d_polys.p, d_py.p, d_px.p, cols, nc, d_rec_bin.p, d_rec_j.p, d_cnt.p);
    LAUNCH_CHECK("poly_cross");
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_bytes, d_cnt.p, d_start.p, 0, (size_t)nb, rocprim::plus<int32_t>(), s));
    DBuf<uint8_t> d_tmp;
    PTRY(d_tmp.alloc(tmp_bytes));
    HIP_TRY(rocprim::exclusive_scan(d_tmp.p, tmp_bytes, d_cnt.p, d_start.p, 0, (size_t)nb, rocprim::plus<int32_t>(), s));
    hipLaunchKernelGGL(poly_scatter_kernel, dim3((unsigned)cdiv(nc, 256)), dim3(256), 0, s, d_rec_bin.p, d_rec_j.p, nc,
                       d_start.p, d_cnt.p, d_sorted.p);
    LAUNCH_CHECK("poly_scatter");
    hipLaunchKernelGGL(poly_pair_kernel, dim3((unsigned)cdiv(nb, 256)), dim3(256), 0, s, d_start.p, nb, nc, d_polys.p,
                       (int)polys.size(), d_sorted.p, rows, cols, d_diff.p);
    LAUNCH_CHECK("poly_pair");
    HIP_TRY(hipStreamSynchronize(s));   // (the temporaries above are freed on return)
  }
  const int nchunk = (int)cdiv(cols, POLY_CHUNK);
  DBuf<int32_t> d_csum;
  DBuf<uint32_t> d_above;
  PTRY(d_csum.alloc((size_t)ncls * nchunk * rows));
  PTRY(d_above.alloc(TDR_MAX_CLASSES));
  HIP_TRY(hipMemcpyAsync(d_above.p, above.data(), TDR_MAX_CLASSES * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  const int64_t n4 = (int64_t)ncls * nchunk * rows, n5 = (int64_t)ncls * rows, n6 = (int64_t)nchunk * rows;
  hipLaunchKernelGGL(poly_chunk_sum_kernel, dim3((unsigned)cdiv(n4, 256)), dim3(256), 0, s, d_diff.p, ncls, rows, cols,
                     nchunk, d_csum.p);
  hipLaunchKernelGGL(poly_chunk_prefix_kernel, dim3((unsigned)cdiv(n5, 256)), dim3(256), 0, s, d_csum.p, ncls, rows, nchunk);
  hipLaunchKernelGGL(poly_planes_kernel, dim3((unsigned)cdiv(n6, 256)), dim3(256), 0, s, d_diff.p, d_csum.p, ncls, rows,
                     cols, nchunk, d_above.p, planes_cm);
  if (raster)
    hipLaunchKernelGGL(poly_raster_kernel, dim3((unsigned)cdiv(rows, 64), (unsigned)cdiv(cols, 64), (unsigned)ncls),
                       dim3(256), 0, s, planes_cm, rows, cols, raster);
  LAUNCH_CHECK("poly_planes");
  HIP_TRY(hipStreamSynchronize(s));
  return TDR_OK;
}
