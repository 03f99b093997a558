// tdr_host.cpp — the handle layer of the C ABI (include/tdr.h, "tdr_map_* / tdr_renderer_* / tdr_filter_*"):
// C++ host code that owns device memory and sequences the hand-written HIP kernels (tdr_*.hip) exactly the way
// the reference's classes sequence their Eigen loops.  One handle = one reference object:
//     tdr_map       TopDownMapPolar   (include/top_down_render/top_down_map_polar.h:6-22)
//     tdr_renderer  ScanRendererPolar (include/top_down_render/scan_renderer_polar.h:15-22)
//     tdr_filter    ParticleFilter    (include/top_down_render/particle_filter.h:22-73)
// One caller thread per handle (the reference calls everything from the ROS spinner thread).  A filter lives on one GPU
// or is sharded over the ranks of a tdr_comm (one process per GPU, tdr_comm.cpp: RCCL or caller-supplied transport).
// No CPU fallback: every entry point fails with TDR_ERR_HIP when no device is present.
#include <sys/stat.h>
#include <cerrno>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "tdr.h"
#include "tdr_batch.h"
#include "tdr_config.h"
#include "tdr_gmm_dev.h"

bool tdr_score_polar_float_form(const tdr_map_desc* map, int nb, int nr, int64_t n, int64_t n_total);   // tdr_score.hip

extern "C" int tdr_set_error(int code, const char* msg);  // tdr_core.hip

namespace {

int failh(int code, const char* fmt, ...) {
  char buf[400];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return tdr_set_error(code, buf);
}
#define HTRY(expr)                                                                        \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) return failh(TDR_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define TTRY(expr)            \
  do {                        \
    int rc_ = (expr);         \
    if (rc_ != TDR_OK) return rc_; \
  } while (0)

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;             // owns device memory
  DevBuf& operator=(const DevBuf&) = delete;
  int resize(size_t count) {
    if (count <= n) return TDR_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e != hipSuccess) return failh(TDR_ERR_NOMEM, "hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
    n = count;
    return TDR_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DevBuf() { release(); }
};

}  // namespace

struct tdr_map {
  DevBuf<float> rec;
  DevBuf<float> tab;
  DevBuf<float> fac;   // the table's factors (tdr_polar_factors_host), handed to the filter's tdr_score_ctx
  DevBuf<uint32_t> crec;   // compact form of `rec` (tdr_k_compact_map), when the map has one
  DevBuf<float> cdict;
  DevBuf<uint8_t> cws;
  DevBuf<uint8_t> rec16;   // scratch of the 40-rotation search (tdr_map_desc.rec16), allocated by the first large search
  hipEvent_t rec16_used = nullptr;   // recorded after every search that used rec16; the next one waits for it (map_rec16_*)
  ~tdr_map() { if (rec16_used) (void)hipEventDestroy(rec16_used); }
  std::vector<float> maps_host;  // class_maps_ (column-major), kept for getClassesAtPoint / particle initialisation
  std::vector<uint8_t> mask_host;  // class_mask_ (column-major), kept for the map cache
  tdr_map_desc desc{};
  DevBuf<float> geo_rec;         // geo_maps_[0..1] as a 2-class record map (tdr_k_geo_map_from_map), built on first use
  int geo_pending = 0;           // 0: geo_rec is current (or there is no map); 1: derive from the classes; 2: constant 1
  tdr_map_desc geo_desc{};
  int nb = 0, nr = 0;
  float ang_res = 0;
  int win_rows = 0, win_cols = 0;   // the Cartesian window (tdr_map_set_window); 0: none
  int center_x = 0, center_y = 0;
  bool have_map = false;
  // staging of the run-time map replacement (tdr_map_set_labels: aerial maps keep arriving, top_down_render.cpp:574-600),
  // kept between calls: allocating and freeing ~1 GB per map costs more than the ingest itself
  DevBuf<uint8_t> ing_img, ing_ws, ing_mask;
  DevBuf<int32_t> ing_lut;
  DevBuf<float> ing_maps;
  // incremental updates (tdr_map_update_labels_incremental, csrc/tdr_map_incr.hip).  inc_valid: the map was last set from
  // a label image (tdr_map_set_labels or an incremental update) and ing_img / ing_lut / ing_ws still hold that image, its
  // LUT (inc_lut) and the ingest's class words and column distances.  inc_counts: the dictionary's occurrence counts
  // (tdr_k_map_dict_counts), current while inc_counts_ok; every full compaction clears it.
  bool inc_valid = false, inc_counts_ok = false;
  int inc_img_h = 0, inc_img_w = 0;
  std::vector<int32_t> inc_lut;
  DevBuf<uint8_t> inc_ws, inc_mstage;
  DevBuf<int32_t> inc_counts, inc_dtiles;
  DevBuf<float> inc_stage;
  std::vector<int32_t> inc_tiles;
  std::vector<float> inc_hstage;
  std::vector<uint8_t> inc_hmstage;
};

struct tdr_renderer {
  DevBuf<int32_t> lut;
  DevBuf<float> pts, img, pk, geo;
  DevBuf<uint8_t> keys;  // per-point bin keys of the two-phase raster
  DevBuf<uint8_t> geo_ws;  // sort keys / scratch of the geometric render
  int ncls = 0, rows = 0, cols = 0;  // shape of the last render
  bool have_scan = false;
  bool polar = true;                 // ... and its kind (renderSemanticTopDown of ScanRendererPolar / ScanRenderer)
  // tdr_batch_render_polar renders on the caller's stream without a host wait: `rendered` marks the end of that render
  // (render_async), and every stream that has since read img / pk leaves an event in `readers` for the next batched
  // render to wait on (one per stream: a later record on the same stream covers the earlier reads)
  hipEvent_t rendered = nullptr;
  bool render_async = false;
  mutable std::vector<std::pair<hipStream_t, hipEvent_t>> readers;
  mutable size_t n_readers = 0;
  ~tdr_renderer() {
    if (rendered) { (void)hipEventSynchronize(rendered); (void)hipEventDestroy(rendered); }
    for (auto& e : readers) { (void)hipEventSynchronize(e.second); (void)hipEventDestroy(e.second); }
  }
};

struct tdr_filter {
  tdr_map* map = nullptr;
  tdr_filter_params fp{};
  int64_t n_max = 0, n = 0;
  DevBuf<float> st, st_new, last_dist, raw_w, w, runmax, info, ws, z4, scan_img, scan_pk, stats;
  DevBuf<uint8_t> pfx_ws;  // chunk headers of the multi-workgroup running sum
  DevBuf<int32_t> idx, perm, loc_tmp;
  DevBuf<tdr_state> aos;
  void* rng = nullptr;
  uint64_t seed = 0, step = 0;
  uint64_t prop_calls = 0;    // device RNG: every propagate call draws fresh noise (counter = calls so far)
  bool scale_frozen = false, maybe_uninit = true, parity_rng = true;
  bool cart = false;          // tdr_filter_create_cart: the scoring stage is the Cartesian one (window = the map's)
  DevBuf<float> init_ws;      // ... and the workspace of its heading search, allocated by the first update that runs it
  int locality_every = 1;
  float uniform_scale = 0.f;
  bool rng_owned = true;      // false after tdr_filter_share_rng: the generator belongs to the caller
  DevBuf<float> gmm_samples;  // [num][3] device staging for computeGMM
  DevBuf<double> gmm_dev;     // the device fit: samples [num][4], the candidate fits' outputs and workspaces (gmm_plan)
  int num_gaussians = 1;      // particle_filter.cpp:7
  std::vector<float> gmm_means, gmm_covs;
  DevBuf<float> ml_dev;  // fields + mlState of the max-likelihood particle of the last update (tdr_k_save_ml_state)
  bool have_ml = false;
  // meanLikelihood + computeMeanCov of the CURRENT particle set, as last read back: publishPoseEst asks for both in a row
  // (src/top_down_render.cpp:333, 354), which is one kernel and one read-back here.  Everything that changes the set
  // clears the flag (states_changed).
  float mean_cov_host[24] = {0};
  bool mean_cov_valid = false;
  // scale() of a frozen filter as tdr_batch_pose read it back (cleared with the mean / covariance)
  float scale_host = -1.f;
  bool scale_valid = false;
  void states_changed() { mean_cov_valid = false; scale_valid = false; }
  hipStream_t stream = nullptr;
  tdr_score_ctx* score_ctx = nullptr;   // this filter's own span tuner (and the table's factors) for its scoring launches (tdr.h)
  // The reference's generator in parity mode: the host std::mt19937 `rng` and its continuation on the device, a
  // tdr_rng_pipe (csrc/tdr_rng.hip).  Exactly one of them is current: propagate and the resample's uniform draw continue
  // the stream on the device (drawn ahead, beside the scoring launch), the host engine takes it back when host code
  // draws (particle initialisation).  A generator shared with the caller (tdr_filter_share_rng) stays on the host.
  tdr_rng_pipe* pipe = nullptr;
  // Sharded over the ranks of `comm` (one process per GPU; NULL = the whole filter lives here).  n / n_max stay the
  // GLOBAL counts; this rank holds particles [rank * nl, (rank + 1) * nl), nl = n / world, in st[7][cap] with
  // cap = n_max / world.  raw_glob / ld_glob / w / runmax are global arrays, identical on every rank.
  tdr_comm* comm = nullptr;
  int world = 1, rank = 0;
  int64_t cap = 0;
  DevBuf<float> xchg_in, xchg_out, raw_glob, ld_glob, st_send, st_all, st_glob, pk_recv;
  DevBuf<float> geo_pk;   // packed geometric scan (tdr_filter_update_geo)
  // the particle picture (tdr_filter_visualize): the background as uploaded, the four bit planes, the overlay segments
  // and the published image
  DevBuf<uint8_t> viz_bg, viz_out;
  DevBuf<uint32_t> viz_planes;
  DevBuf<int32_t> viz_segs;
  int viz_h = 0, viz_w = 0;
  int64_t nl() const { return n / world; }
};

// a stream that reads a renderer's render continues after its batched render / notes the read for the next one
static int renderer_wait_render(const tdr_renderer* r, hipStream_t s) {
  if (r->render_async) HTRY(hipStreamWaitEvent(s, r->rendered, 0));
  return TDR_OK;
}
static int renderer_note_read(const tdr_renderer* r, hipStream_t s) {
  size_t i = 0;
  while (i < r->n_readers && r->readers[i].first != s) i++;
  if (i == r->n_readers) {
    if (i == r->readers.size()) {
      hipEvent_t e = nullptr;
      HTRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      r->readers.emplace_back(s, e);
    }
    r->readers[i].first = s;
    r->n_readers++;
  }
  HTRY(hipEventRecord(r->readers[i].second, s));
  return TDR_OK;
}

// .eig files of the reference's map cache (top_down_map.h:29-50)
static std::string cache_dir_or_default(const char* cache_dir) {
  if (cache_dir && *cache_dir) return cache_dir;
  const char* home = getenv("HOME");
  return std::string(home ? home : ".") + "/.ros/xview_cache";
}
int tdr_png_read_gray8(const char* path, std::vector<uint8_t>& px, int& w, int& h);   // tdr_png.cpp
int tdr_png_write_gray8(const char* path, const uint8_t* px, int w, int h);
int tdr_png_read_bgr8(const char* path, std::vector<uint8_t>& bgr, int& w, int& h);

template <class T>
static int read_eig(const std::string& path, std::vector<T>& out, int64_t& rows, int64_t& cols) {
  FILE* fh = fopen(path.c_str(), "rb");
  if (!fh) return failh(TDR_ERR_ARG, "map cache: cannot open %s", path.c_str());
  int64_t hdr[2] = {0, 0};
  bool ok = fread(hdr, sizeof(int64_t), 2, fh) == 2 && hdr[0] > 0 && hdr[1] > 0 && hdr[0] < (1 << 24) && hdr[1] < (1 << 24);
  if (ok) {   // the payload the header promises must be what the file holds (a damaged header must not size the buffer)
    const long at = ftell(fh);
    ok = at >= 0 && fseek(fh, 0, SEEK_END) == 0;
    const long end = ok ? ftell(fh) : -1;
    ok = ok && end >= at && (uint64_t)(end - at) == (uint64_t)hdr[0] * (uint64_t)hdr[1] * sizeof(T) &&
         fseek(fh, at, SEEK_SET) == 0;
  }
  if (ok) {
    out.resize((size_t)hdr[0] * hdr[1]);
    ok = fread(out.data(), sizeof(T), out.size(), fh) == out.size() && fgetc(fh) == EOF;
  }
  fclose(fh);
  if (!ok) return failh(TDR_ERR_ARG, "map cache: %s is not a well-formed .eig file of this scalar type", path.c_str());
  rows = hdr[0];
  cols = hdr[1];
  return TDR_OK;
}
template <class T>
static int write_eig(const std::string& path, const T* data, int64_t rows, int64_t cols) {
  FILE* fh = fopen(path.c_str(), "wb");
  if (!fh) return failh(TDR_ERR_ARG, "map cache: cannot write %s", path.c_str());
  const int64_t hdr[2] = {rows, cols};
  const bool ok = fwrite(hdr, sizeof(int64_t), 2, fh) == 2 && fwrite(data, sizeof(T), (size_t)rows * cols, fh) == (size_t)rows * cols;
  fclose(fh);
  return ok ? TDR_OK : failh(TDR_ERR_ARG, "map cache: short write to %s", path.c_str());
}
// geo_maps_ for a freshly packed map: computed from the class maps like the static-map constructor does
// (src/top_down_map.cpp:48-58), or the constant 1 the dynamic-map path leaves them at (:126-133)
// Nothing on the hot path reads them (the reference's score ignores top_down_geo, state_particle.cpp:145-152): they are
// built — two more distance transforms over the whole map — when something first asks for them (map_ensure_geo).
static int map_make_geo(tdr_map* m, bool constant_one) {
  m->geo_pending = constant_one ? 2 : 1;
  m->geo_rec.release();
  m->geo_desc = tdr_map_desc{};
  return TDR_OK;
}
static int map_ensure_geo(tdr_map* m) {
  if (!m->geo_pending) return TDR_OK;
  const bool constant_one = m->geo_pending == 2;
  const int rows = m->desc.rows, cols = m->desc.cols;
  TTRY(m->geo_rec.resize(tdr_map_rec_floats_total(2, rows, cols)));
  DevBuf<uint8_t> ws;
  if (!constant_one) TTRY(ws.resize(tdr_map_ingest_workspace_bytes(2, rows, cols)));
  TTRY(tdr_k_geo_map_from_map(&m->desc, constant_one ? 1 : 0, m->geo_rec.p, ws.p, nullptr));
  HTRY(hipDeviceSynchronize());
  m->geo_desc = tdr_map_desc{};
  m->geo_desc.rec = m->geo_rec.p;
  m->geo_desc.ncls = 2;
  m->geo_desc.rows = rows;
  m->geo_desc.cols = cols;
  m->geo_desc.rec_floats = tdr_rec_floats(2);
  m->geo_desc.resolution = m->desc.resolution;
  m->geo_pending = 0;
  return TDR_OK;
}

// the compact records of a freshly packed map (desc.rec etc. already set)
static int map_compact(tdr_map* m) {
  m->inc_counts_ok = false;   // the dictionary is built anew
  m->desc.crec = nullptr; m->desc.dict = nullptr; m->desc.dict_n = 0; m->desc.cwords = 0;
  m->desc.rec16 = nullptr;   // sized for the previous grid: the next large init search allocates it again
  const size_t nw = tdr_cmap_words_total(m->desc.ncls, m->desc.rows, m->desc.cols);
  if (nw == 0) return TDR_OK;
  TTRY(m->crec.resize(nw));
  TTRY(m->cdict.resize(TDR_CMAP_WIDE_MAX_DICT));
  TTRY(m->cws.resize(TDR_CMAP_WORKSPACE_BYTES));
  TTRY(tdr_k_compact_map(&m->desc, m->crec.p, m->cdict.p, m->cws.p, nullptr));
  if (m->desc.cwords == 0 && m->desc.dict_n < 0) {   // too many distinct values for 10-bit fields: the wide form
    const size_t nww = tdr_cmap_wide_words_total(m->desc.ncls, m->desc.rows, m->desc.cols);
    TTRY(m->crec.resize(nww));
    TTRY(tdr_k_compact_map_wide(&m->desc, m->crec.p, m->cdict.p, m->cws.p, nullptr));
  }
  if (m->desc.cwords == 0) m->desc.dict_n = 0;
  return TDR_OK;
}

extern "C" {

// ---- TopDownMap(Polar) ------------------------------------------------------------------------------------------------
int tdr_map_create(tdr_map** out) {
  if (!out) return failh(TDR_ERR_ARG, "map_create: null out");
  if (tdr_device_count() < 1) return failh(TDR_ERR_HIP, "map_create: no HIP device (there is no CPU fallback)");
  *out = new tdr_map();
  return TDR_OK;
}
void tdr_map_destroy(tdr_map* m) { delete m; }

// Storage of class_maps_ / class_mask_ (top_down_map.h:77-79) in the form computeDists leaves them
// (top_down_map.cpp:289-326); also the body of TopDownMap::updateMap once the distance transform is done (:146-157).
int tdr_map_set(tdr_map* m, const float* class_maps, const uint8_t* class_mask, int ncls, int rows, int cols,
                float resolution, int center_x, int center_y) {
  if (!m || !class_maps || !class_mask) return failh(TDR_ERR_ARG, "map_set: null pointer");
  if (ncls < 1 || ncls > TDR_MAX_CLASSES || rows < 1 || cols < 1 || !(resolution > 0))
    return failh(TDR_ERR_ARG, "map_set: bad shape / resolution");
  m->inc_valid = false;
  const size_t ncell = (size_t)rows * cols;
  DevBuf<float> d_maps;
  DevBuf<uint8_t> d_mask;
  TTRY(d_maps.resize(ncell * ncls));
  TTRY(d_mask.resize(ncell));
  HTRY(hipMemcpy(d_maps.p, class_maps, ncell * ncls * sizeof(float), hipMemcpyHostToDevice));
  HTRY(hipMemcpy(d_mask.p, class_mask, ncell, hipMemcpyHostToDevice));
  TTRY(m->rec.resize(tdr_map_rec_floats_total(ncls, rows, cols)));
  TTRY(tdr_k_pack_map(d_maps.p, d_mask.p, ncls, rows, cols, m->rec.p, nullptr));
  HTRY(hipDeviceSynchronize());
  m->maps_host.assign(class_maps, class_maps + ncell * ncls);
  m->mask_host.assign(class_mask, class_mask + ncell);
  m->desc.rec = m->rec.p;
  m->desc.ncls = ncls;
  m->desc.rows = rows;
  m->desc.cols = cols;
  m->desc.rec_floats = tdr_rec_floats(ncls);
  m->desc.resolution = resolution;
  m->center_x = center_x;
  m->center_y = center_y;
  TTRY(map_compact(m));
  TTRY(map_make_geo(m, false));
  m->have_map = true;
  if (m->nb > 0) return tdr_map_sample_pts_polar(m, m->nb, m->nr, m->ang_res);
  return TDR_OK;
}

// TopDownMap::updateMap(const cv::Mat&, map_center) (top_down_map.cpp:146-157): loadCompressedRasterMap (:116-144) +
// computeDists (:289-326) for a HOST class-index image (cv::Mat CV_8UC1 layout), all on the device.
int tdr_map_set_labels(tdr_map* m, const uint8_t* label_img, int img_h, int img_w, const int32_t* flatten_lut,
                       int lut_size, int ncls, float resolution, int center_x, int center_y) {
  if (!m || !label_img || !flatten_lut) return failh(TDR_ERR_ARG, "map_set_labels: null pointer");
  int rows = 0, cols = 0;
  TTRY(tdr_map_ingest_shape(img_h, img_w, resolution, &rows, &cols));
  if (ncls < 1 || ncls > TDR_MAX_CLASSES || rows < 1 || cols < 1) return failh(TDR_ERR_ARG, "map_set_labels: bad shape");
  m->inc_valid = false;
  DevBuf<uint8_t>&d_img = m->ing_img, &d_ws = m->ing_ws, &d_mask = m->ing_mask;
  DevBuf<int32_t>& d_lut = m->ing_lut;
  DevBuf<float>& d_maps = m->ing_maps;
  const size_t ncell = (size_t)rows * cols;
  TTRY(d_img.resize((size_t)img_h * img_w));
  TTRY(d_lut.resize((size_t)lut_size));
  TTRY(d_ws.resize(tdr_map_ingest_workspace_bytes(ncls, rows, cols)));
  HTRY(hipMemcpy(d_img.p, label_img, (size_t)img_h * img_w, hipMemcpyHostToDevice));
  HTRY(hipMemcpy(d_lut.p, flatten_lut, (size_t)lut_size * sizeof(int32_t), hipMemcpyHostToDevice));
  TTRY(m->rec.resize(tdr_map_rec_floats_total(ncls, rows, cols)));
  TTRY(tdr_k_map_from_labels(d_img.p, img_h, img_w, d_lut.p, lut_size, ncls, resolution, m->rec.p, d_ws.p, nullptr));
  // host copy of class_maps_ for getClassesAtPoint / particle initialisation
  TTRY(d_maps.resize(ncell * ncls));
  TTRY(d_mask.resize(ncell));
  TTRY(tdr_k_unpack_map(m->rec.p, ncls, rows, cols, d_maps.p, d_mask.p, nullptr));
  m->maps_host.resize(ncell * ncls);
  m->mask_host.resize(ncell);
  HTRY(hipMemcpy(m->maps_host.data(), d_maps.p, ncell * ncls * sizeof(float), hipMemcpyDeviceToHost));
  HTRY(hipMemcpy(m->mask_host.data(), d_mask.p, ncell, hipMemcpyDeviceToHost));
  m->desc.rec = m->rec.p;
  m->desc.ncls = ncls;
  m->desc.rows = rows;
  m->desc.cols = cols;
  m->desc.rec_floats = tdr_rec_floats(ncls);
  m->desc.resolution = resolution;
  m->center_x = center_x;
  m->center_y = center_y;
  TTRY(map_compact(m));
  TTRY(map_make_geo(m, true));   // updateMap leaves geo_maps_ at their constant 1 (:126-133)
  // `if (!class_maps_[1].isZero(0)) have_map_ = true; else "Received map with no road"` (:150-154)
  bool road = false;
  if (ncls > 1)
    for (size_t k = 0; k < ncell && !road; k++) road = m->maps_host[ncell + k] != 0.f;
  if (road) m->have_map = true;
  m->inc_valid = true;   // ing_img / ing_lut / ing_ws now describe this map (tdr_map_update_labels_incremental)
  m->inc_img_h = img_h;
  m->inc_img_w = img_w;
  m->inc_lut.assign(flatten_lut, flatten_lut + lut_size);
  if (m->nb > 0 && m->have_map) return tdr_map_sample_pts_polar(m, m->nb, m->nr, m->ang_res);
  return TDR_OK;
}

// The incremental update of a map whose ing_img now holds the new image (same shape, resolution, classes and LUT as the
// label image the map was last set from): tdr_k_map_update_labels rebuilds the cells within R of a changed cell, the host
// copies change in the affected tiles only.  *too_large: more than max_cells cells would be rebuilt (max_cells < 0: no
// limit); nothing has changed then and the caller takes the full path.
static int map_apply_incremental(tdr_map* m, int center_x, int center_y, int64_t max_cells, int64_t* changed,
                                 bool* too_large) {
  const int ncls = m->desc.ncls, rows = m->desc.rows, cols = m->desc.cols;
  const size_t ncell = (size_t)rows * cols;
  *too_large = false;
  TTRY(m->inc_ws.resize(tdr_map_incr_workspace_bytes(rows, cols)));
  m->inc_tiles.resize((size_t)tdr_map_incr_tiles(rows, cols));
  if (m->desc.cwords && !m->inc_counts_ok) {
    TTRY(m->inc_counts.resize(TDR_CMAP_WIDE_MAX_DICT));
    TTRY(tdr_k_map_dict_counts(&m->desc, m->inc_counts.p, nullptr));
    m->inc_counts_ok = true;
  }
  m->inc_valid = false;   // until the update is through
  int n_tiles = 0, compact_ok = 0;
  TTRY(tdr_k_map_update_labels(m->ing_img.p, m->inc_img_h, m->inc_img_w, m->ing_lut.p, (int)m->inc_lut.size(), &m->desc,
                               m->ing_ws.p, m->desc.cwords ? m->inc_counts.p : nullptr, max_cells, m->inc_ws.p,
                               m->inc_tiles.data(), &n_tiles, changed, &compact_ok, nullptr));
  if (n_tiles < 0) {
    *too_large = true;
    return TDR_OK;
  }
  if (!compact_ok) TTRY(map_compact(m));   // the dictionary changes (or the map may gain a compact form): build it whole
  else m->desc.rec16 = nullptr;            // as map_compact drops it
  // host copies of the affected tiles; `have_map` (sticky, tdr_map_set_labels): while false, class 1 of the previous map
  // was zero everywhere, so only the affected cells can hold road now
  bool road = false;
  if (n_tiles > 0) {
    const size_t tc = (size_t)TDR_MAP_INCR_TILE * TDR_MAP_INCR_TILE;
    TTRY(m->inc_dtiles.resize((size_t)n_tiles));
    TTRY(m->inc_stage.resize((size_t)n_tiles * ncls * tc));
    TTRY(m->inc_mstage.resize((size_t)n_tiles * tc));
    HTRY(hipMemcpy(m->inc_dtiles.p, m->inc_tiles.data(), (size_t)n_tiles * sizeof(int32_t), hipMemcpyHostToDevice));
    TTRY(tdr_k_map_gather_tiles(m->rec.p, ncls, rows, cols, m->inc_dtiles.p, n_tiles, m->inc_stage.p, m->inc_mstage.p,
                                nullptr));
    m->inc_hstage.resize((size_t)n_tiles * ncls * tc);
    m->inc_hmstage.resize((size_t)n_tiles * tc);
    HTRY(hipMemcpy(m->inc_hstage.data(), m->inc_stage.p, m->inc_hstage.size() * sizeof(float), hipMemcpyDeviceToHost));
    HTRY(hipMemcpy(m->inc_hmstage.data(), m->inc_mstage.p, m->inc_hmstage.size(), hipMemcpyDeviceToHost));
    const int T = TDR_MAP_INCR_TILE, tx_n = (cols + T - 1) / T;
    for (int b = 0; b < n_tiles; b++) {
      const int t = m->inc_tiles[(size_t)b], ty = t / tx_n, tx = t - ty * tx_n;
      const int r0 = ty * T, nr = std::min(T, rows - r0);
      for (int cl = 0; cl < T && tx * T + cl < cols; cl++) {
        const size_t dst = (size_t)(tx * T + cl) * rows + r0;   // column-major: the tile's column is nr floats in a row
        for (int k = 0; k < ncls; k++)
          std::memcpy(m->maps_host.data() + (size_t)k * ncell + dst, m->inc_hstage.data() + ((size_t)b * ncls + k) * tc + (size_t)cl * T,
                      (size_t)nr * sizeof(float));
        std::memcpy(m->mask_host.data() + dst, m->inc_hmstage.data() + (size_t)b * tc + (size_t)cl * T, (size_t)nr);
        if (!m->have_map && ncls > 1)
          for (int r = 0; r < nr && !road; r++) road = m->maps_host[ncell + dst + r] != 0.f;
      }
    }
  }
  const bool had_map = m->have_map;
  if (road) m->have_map = true;
  m->center_x = center_x;
  m->center_y = center_y;
  m->inc_valid = true;
  // the polar table depends on the shape and the resolution alone: built already unless this update brought the first map
  if (m->nb > 0 && m->have_map && !had_map) return tdr_map_sample_pts_polar(m, m->nb, m->nr, m->ang_res);
  return TDR_OK;
}

// tdr_map_set_labels' end state, reached by rebuilding only what the new image changes (tdr_map_incr.hip)
int tdr_map_update_labels_incremental(tdr_map* m, const uint8_t* label_img, int img_h, int img_w,
                                      const int32_t* flatten_lut, int lut_size, int ncls, float resolution, int center_x,
                                      int center_y, int64_t* changed_cells) {
  if (!m || !label_img || !flatten_lut || !changed_cells)
    return failh(TDR_ERR_ARG, "map_update_labels_incremental: null pointer");
  *changed_cells = -1;
  const bool same = m->inc_valid && img_h == m->inc_img_h && img_w == m->inc_img_w && ncls == m->desc.ncls &&
                    resolution == m->desc.resolution && lut_size == (int)m->inc_lut.size() &&
                    std::equal(m->inc_lut.begin(), m->inc_lut.end(), flatten_lut);
  if (!same) return tdr_map_set_labels(m, label_img, img_h, img_w, flatten_lut, lut_size, ncls, resolution, center_x, center_y);
  HTRY(hipMemcpy(m->ing_img.p, label_img, (size_t)img_h * img_w, hipMemcpyHostToDevice));
  int64_t changed = 0;
  bool too_large = false;
  TTRY(map_apply_incremental(m, center_x, center_y, (int64_t)((double)m->desc.rows * m->desc.cols * TDR_MAP_INCR_MAX_FRACTION),
                             &changed, &too_large));
  if (too_large) return tdr_map_set_labels(m, label_img, img_h, img_w, flatten_lut, lut_size, ncls, resolution, center_x, center_y);
  *changed_cells = changed;
  return TDR_OK;
}

// the image of the last label-image map with one rectangle overwritten: only the rectangle is uploaded
int tdr_map_patch_labels(tdr_map* m, const uint8_t* patch, int y0, int x0, int h, int w, int center_x, int center_y,
                         int64_t* changed_cells) {
  if (!m || !patch || !changed_cells) return failh(TDR_ERR_ARG, "map_patch_labels: null pointer");
  if (!m->inc_valid)
    return failh(TDR_ERR_ARG, "map_patch_labels: the map was not last set from a label image (tdr_map_set_labels)");
  if (h < 1 || w < 1 || y0 < 0 || x0 < 0 || (int64_t)y0 + h > m->inc_img_h || (int64_t)x0 + w > m->inc_img_w)
    return failh(TDR_ERR_ARG, "map_patch_labels: rectangle (%d, %d) + %d x %d lies outside the %d x %d image", x0, y0, w, h,
                 m->inc_img_w, m->inc_img_h);
  HTRY(hipMemcpy2D(m->ing_img.p + (size_t)y0 * m->inc_img_w + x0, (size_t)m->inc_img_w, patch, (size_t)w, (size_t)w,
                   (size_t)h, hipMemcpyHostToDevice));
  bool too_large = false;
  return map_apply_incremental(m, center_x, center_y, -1, changed_cells, &too_large);
}

int tdr_map_get_desc(const tdr_map* m, tdr_map_desc* out) {
  if (!m || !out) return failh(TDR_ERR_ARG, "map_get_desc: null pointer");
  *out = m->desc;
  return TDR_OK;
}

// TopDownMapPolar::samplePtsPolar (top_down_map_polar.cpp:7-19)
int tdr_map_sample_pts_polar(tdr_map* m, int nb, int nr, float ang_res) {
  if (!m || nb < 1 || nr < 1) return failh(TDR_ERR_ARG, "sample_pts_polar: bad arguments");
  m->nb = nb;
  m->nr = nr;
  m->ang_res = ang_res;
  if (!m->have_map) return TDR_OK;  // table needs params_.resolution; built when the map arrives
  std::vector<float> tab((size_t)2 * nb * nr);
  TTRY(tdr_polar_table_host(nb, nr, ang_res, m->desc.resolution, tab.data()));
  TTRY(m->tab.resize(tab.size()));
  HTRY(hipMemcpy(m->tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
  std::vector<float> fac((size_t)2 * nb + nr);
  TTRY(tdr_polar_factors_host(nb, nr, ang_res, m->desc.resolution, fac.data()));
  TTRY(m->fac.resize(fac.size()));
  HTRY(hipMemcpy(m->fac.p, fac.data(), fac.size() * sizeof(float), hipMemcpyHostToDevice));
  return TDR_OK;
}

// the (theta bins, range bins) given to samplePtsPolar last: the shape ParticleFilter::update's images must have
int tdr_map_set_window(tdr_map* m, int rows, int cols) {
  if (!m || rows < 1 || cols < 1) return failh(TDR_ERR_ARG, "map_set_window: bad arguments");
  m->win_rows = rows;
  m->win_cols = cols;
  return TDR_OK;
}
int tdr_map_window_shape(const tdr_map* m, int* rows, int* cols) {
  if (!m) return failh(TDR_ERR_ARG, "map_window_shape: null map");
  if (rows) *rows = m->win_rows;
  if (cols) *cols = m->win_cols;
  return TDR_OK;
}

int tdr_map_polar_shape(const tdr_map* m, int* nb, int* nr) {
  if (!m || !nb || !nr) return failh(TDR_ERR_ARG, "map_polar_shape: bad arguments");
  *nb = m->nb;
  *nr = m->nr;
  return TDR_OK;
}

int tdr_map_info(const tdr_map* m, int* ncls, int* rows, int* cols, float* resolution, int* have_map) {
  if (!m) return failh(TDR_ERR_ARG, "map_info: null map");
  if (ncls) *ncls = m->desc.ncls;
  if (rows) *rows = m->desc.rows;
  if (cols) *cols = m->desc.cols;
  if (resolution) *resolution = m->desc.resolution;
  if (have_map) *have_map = m->have_map ? 1 : 0;
  return TDR_OK;
}

// TopDownMap::mapCenter() (top_down_map.h:72): the centre given with the last map, whoever set it (the map's own
// updateMap or ParticleFilter::updateMap)
int tdr_map_center(const tdr_map* m, int* center_x, int* center_y) {
  if (!m || !center_x || !center_y) return failh(TDR_ERR_ARG, "map_center: bad arguments");
  *center_x = m->center_x;
  *center_y = m->center_y;
  return TDR_OK;
}

// getLocalMap through the handle: one window, host arrays out
int tdr_map_local_map(tdr_map* m, int polar, float cx, float cy, float scale_or_rot, float res, int rows, int cols,
                      float* dists_out, uint8_t* mask_out) {
  if (!m || !m->have_map || !dists_out || !mask_out) return failh(TDR_ERR_ARG, "map_local_map: no map / null output");
  if (polar) {
    if (m->nb < 1 || !m->tab.p) return failh(TDR_ERR_ARG, "map_local_map: samplePtsPolar was never called");
    rows = m->nb;
    cols = m->nr;
  }
  if (rows < 1 || cols < 1) return failh(TDR_ERR_ARG, "map_local_map: bad window shape");
  const size_t P = (size_t)rows * cols;
  DevBuf<float> d;
  DevBuf<uint8_t> k;
  TTRY(d.resize(P * m->desc.ncls));
  TTRY(k.resize(P));
  if (polar) TTRY(tdr_k_local_map_polar(&m->desc, m->tab.p, rows, cols, cx, cy, scale_or_rot, res, d.p, k.p, nullptr));
  else TTRY(tdr_k_local_map_cart(&m->desc, rows, cols, cx, cy, scale_or_rot, res, d.p, k.p, nullptr));
  HTRY(hipMemcpy(dists_out, d.p, P * m->desc.ncls * sizeof(float), hipMemcpyDeviceToHost));
  HTRY(hipMemcpy(mask_out, k.p, P, hipMemcpyDeviceToHost));
  return TDR_OK;
}

// ActiveLocalizer::getBestRelPos (src/active_localizer.cpp:44-82): every candidate's difference in one launch, then the
// reference's sequential choice — strict `>` over the candidates in loop order, the next distance only while the best
// difference is below 6000 (:58, 70-73).
int tdr_map_best_rel_pos(tdr_map* m, const float* preds, int K, float best_rel_pos[2], float* best_diff) {
  if (!m || !m->have_map || !preds || !best_rel_pos) return failh(TDR_ERR_ARG, "best_rel_pos: no map / null pointer");
  if (m->nb < 1 || !m->tab.p) return failh(TDR_ERR_ARG, "best_rel_pos: samplePtsPolar was never called");
  if (K < 1 || K > TDR_GMM_MAX_K) return failh(TDR_ERR_ARG, "best_rel_pos: %d hypotheses (1 .. %d)", K, TDR_GMM_MAX_K);
  const int ncand_max = 4 * 17;
  std::vector<float> centres((size_t)ncand_max * K * 2), dists(ncand_max), thetas(ncand_max);
  std::vector<int32_t> shifts(K);
  int nt = 0, nd = 0;
  TTRY(tdr_active_candidates_host(preds, K, m->nb, centres.data(), dists.data(), thetas.data(), shifts.data(), &nt, &nd));
  DevBuf<float> d_c;
  DevBuf<int32_t> d_s;
  DevBuf<double> d_out;
  TTRY(d_c.resize(centres.size()));
  TTRY(d_s.resize(K));
  TTRY(d_out.resize(ncand_max));
  HTRY(hipMemcpy(d_c.p, centres.data(), centres.size() * sizeof(float), hipMemcpyHostToDevice));
  HTRY(hipMemcpy(d_s.p, shifts.data(), K * sizeof(int32_t), hipMemcpyHostToDevice));
  HTRY(hipMemset(d_out.p, 0, ncand_max * sizeof(double)));
  TTRY(tdr_k_active_diffs(&m->desc, m->tab.p, m->nb, m->nr, 2.f, d_c.p, d_s.p, K, ncand_max, d_out.p, nullptr));
  std::vector<double> sums(ncand_max);
  HTRY(hipMemcpy(sums.data(), d_out.p, ncand_max * sizeof(double), hipMemcpyDeviceToHost));
  const int cnt = K * (K - 1) / 2 * m->desc.ncls;   // :15
  float best = 0.f, bd = 0.f, bt = 0.f;
  for (int di = 0; di < nd && best < 6000.f; di++)   // :58
    for (int t = 0; t < nt; t++) {
      const float diff = (float)sums[di * 17 + t] / (float)cnt;   // :19 (0 / 0 = NaN for one hypothesis: never wins)
      if (diff > best) { best = diff; bd = dists[di * 17 + t]; bt = thetas[di * 17 + t]; }   // :70-73
    }
  best_rel_pos[0] = bd;
  best_rel_pos[1] = bt;
  if (best_diff) *best_diff = best;
  return TDR_OK;
}

// getLocalGeoMap (top_down_map_polar.cpp:55-76, top_down_map.cpp:461-481): the window of one pose gathered from the two
// geometric layers; dists_out HOST [2][rows*cols]
int tdr_map_local_geo_map(tdr_map* m, int polar, float cx, float cy, float scale_or_rot, float res, int rows, int cols,
                          float* dists_out) {
  if (!m || !m->have_map || !dists_out) return failh(TDR_ERR_ARG, "map_local_geo_map: no map / null output");
  TTRY(map_ensure_geo(m));
  if (polar) {
    if (m->nb < 1 || !m->tab.p) return failh(TDR_ERR_ARG, "map_local_geo_map: samplePtsPolar was never called");
    rows = m->nb;
    cols = m->nr;
  }
  if (rows < 1 || cols < 1) return failh(TDR_ERR_ARG, "map_local_geo_map: bad window shape");
  const size_t P = (size_t)rows * cols;
  DevBuf<float> d;
  DevBuf<uint8_t> k;
  TTRY(d.resize(P * 2));
  TTRY(k.resize(P));
  if (polar) TTRY(tdr_k_local_map_polar(&m->geo_desc, m->tab.p, rows, cols, cx, cy, scale_or_rot, res, d.p, k.p, nullptr));
  else TTRY(tdr_k_local_map_cart(&m->geo_desc, rows, cols, cx, cy, scale_or_rot, res, d.p, k.p, nullptr));
  HTRY(hipMemcpy(dists_out, d.p, P * 2 * sizeof(float), hipMemcpyDeviceToHost));
  return TDR_OK;
}

// ---- the reference's on-disk map cache (src/top_down_map.cpp:226-286) ------------------------------------------------
// ~/.ros/xview_cache/{cached_data.txt, class_map<i>.eig, geo_map<i>.eig, class_mask.eig}; an .eig file is
// `Index rows, Index cols` (2 x int64) followed by the column-major scalars (top_down_map.h:29-50).
// loadCacheMetaData + loadCachedMaps (:226-261).  *loaded = 0 (and TDR_OK) when no cache matches (map_path, num_classes,
// resolution) — the caller then builds the map by other means; a matching but damaged cache is an error.
int tdr_map_load_cache(tdr_map* m, const char* cache_dir, const char* map_path, int num_classes, float resolution,
                       int center_x, int center_y, int* loaded) {
  if (!m || !map_path || !loaded) return failh(TDR_ERR_ARG, "map_load_cache: bad arguments");
  *loaded = 0;
  const std::string dir = cache_dir_or_default(cache_dir);
  FILE* fh = fopen((dir + "/cached_data.txt").c_str(), "r");
  if (!fh) return TDR_OK;
  char line[4096];
  bool match = fgets(line, sizeof(line), fh) != nullptr;
  if (match) {
    line[strcspn(line, "\r\n")] = 0;
    match = std::string(line) == map_path;                                        // :234-235
  }
  if (match) match = fgets(line, sizeof(line), fh) && atoi(line) == num_classes;  // :236-237
  if (match) match = fgets(line, sizeof(line), fh) && std::fabs((float)atof(line) - resolution) <= 0.01f;   // :238-239
  fclose(fh);
  if (!match) return TDR_OK;
  if (num_classes < 1 || num_classes > TDR_MAX_CLASSES) return failh(TDR_ERR_ARG, "map_load_cache: bad class count");
  std::vector<float> maps, one;
  std::vector<uint8_t> mask;
  int64_t rows = 0, cols = 0, r2 = 0, c2 = 0;
  for (int c = 0; c < num_classes; c++) {
    TTRY(read_eig(dir + "/class_map" + std::to_string(c) + ".eig", one, r2, c2));
    if (c == 0) { rows = r2; cols = c2; }
    if (r2 != rows || c2 != cols) return failh(TDR_ERR_ARG, "map_load_cache: class maps differ in shape");
    maps.insert(maps.end(), one.begin(), one.end());
  }
  TTRY(read_eig(dir + "/class_mask.eig", mask, r2, c2));
  if (r2 != rows || c2 != cols) return failh(TDR_ERR_ARG, "map_load_cache: mask shape differs from the class maps");
  TTRY(tdr_map_set(m, maps.data(), mask.data(), num_classes, (int)rows, (int)cols, resolution, center_x, center_y));
  // the cached geometric layers replace the ones tdr_map_set derived (they are the same for a cache this library wrote)
  std::vector<float> g0, g1;
  if (read_eig(dir + "/geo_map0.eig", g0, r2, c2) == TDR_OK && r2 == rows && c2 == cols &&
      read_eig(dir + "/geo_map1.eig", g1, r2, c2) == TDR_OK && r2 == rows && c2 == cols) {
    g0.insert(g0.end(), g1.begin(), g1.end());
    m->geo_pending = 2;        // (cheapest fill: sizes geo_rec and sets geo_desc; the records are overwritten below)
    TTRY(map_ensure_geo(m));
    std::vector<uint8_t> zero((size_t)rows * cols, 0);
    DevBuf<float> d_maps;
    DevBuf<uint8_t> d_mask;
    TTRY(d_maps.resize(g0.size()));
    TTRY(d_mask.resize(zero.size()));
    HTRY(hipMemcpy(d_maps.p, g0.data(), g0.size() * sizeof(float), hipMemcpyHostToDevice));
    HTRY(hipMemcpy(d_mask.p, zero.data(), zero.size(), hipMemcpyHostToDevice));
    TTRY(tdr_k_pack_map(d_maps.p, d_mask.p, 2, (int)rows, (int)cols, m->geo_rec.p, nullptr));
    HTRY(hipDeviceSynchronize());
  }
  *loaded = 1;
  return TDR_OK;
}
// saveCachedMaps (:263-286)
int tdr_map_save_cache(tdr_map* m, const char* cache_dir, const char* map_path) {
  if (!m || !m->have_map || !map_path) return failh(TDR_ERR_ARG, "map_save_cache: no map");
  const std::string dir = cache_dir_or_default(cache_dir);
  const int ncls = m->desc.ncls, rows = m->desc.rows, cols = m->desc.cols;
  const size_t ncell = (size_t)rows * cols;
  // the reference creates the directory (boost::filesystem::create_directory, src/top_down_map.cpp:228-232): one level
  if (mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST)
    return failh(TDR_ERR_ARG, "map_save_cache: cannot create %s (its parent must exist)", dir.c_str());
  FILE* fh = fopen((dir + "/cached_data.txt").c_str(), "w");
  if (!fh) return failh(TDR_ERR_ARG, "map_save_cache: cannot write into %s", dir.c_str());
  fprintf(fh, "%s\n%d\n%g\n", map_path, ncls, (double)m->desc.resolution);
  fclose(fh);
  for (int c = 0; c < ncls; c++)
    TTRY(write_eig(dir + "/class_map" + std::to_string(c) + ".eig", m->maps_host.data() + ncell * c, rows, cols));
  TTRY(write_eig(dir + "/class_mask.eig", m->mask_host.data(), rows, cols));
  DevBuf<float> d_maps;
  DevBuf<uint8_t> d_mask;
  TTRY(d_maps.resize(ncell * 2));
  TTRY(d_mask.resize(ncell));
  TTRY(map_ensure_geo(m));
  TTRY(tdr_k_unpack_map(m->geo_rec.p, 2, rows, cols, d_maps.p, d_mask.p, nullptr));
  std::vector<float> g(ncell * 2);
  HTRY(hipMemcpy(g.data(), d_maps.p, g.size() * sizeof(float), hipMemcpyDeviceToHost));
  TTRY(write_eig(dir + "/geo_map0.eig", g.data(), rows, cols));
  TTRY(write_eig(dir + "/geo_map1.eig", g.data() + ncell, rows, cols));
  return TDR_OK;
}

// TopDownMap::saveRasterizedMaps (top_down_map.cpp:197-211): class<i>.png, 8-bit grey, 0 inside the class and 255
// elsewhere, flipped to look like the input map (:208).  The reference writes its binary rasters before computeDists turns
// them into distances; from the distance maps held here the raster of a class is "known cell at distance 0".
int tdr_map_save_rasters(tdr_map* m, const char* dir) {
  if (!m || !m->have_map || !dir) return failh(TDR_ERR_ARG, "map_save_rasters: no map");
  const int ncls = m->desc.ncls, rows = m->desc.rows, cols = m->desc.cols;
  const size_t ncell = (size_t)rows * cols;
  if (mkdir(dir, 0700) != 0 && errno != EEXIST) return failh(TDR_ERR_ARG, "map_save_rasters: cannot create %s", dir);   // :198
  std::vector<uint8_t> img(ncell);
  for (int c = 0; c < ncls; c++) {
    const float* d = m->maps_host.data() + ncell * c;   // column-major like class_maps_
    for (int r = 0; r < rows; r++)
      for (int x = 0; x < cols; x++) {
        const size_t k = (size_t)x * rows + r;
        img[(size_t)(rows - 1 - r) * cols + x] = (m->mask_host[k] == 0 && d[k] == 0.f) ? 0 : 255;
      }
    TTRY(tdr_png_write_gray8((std::string(dir) + "/class" + std::to_string(c) + ".png").c_str(), img.data(), cols, rows));
  }
  return TDR_OK;
}
// TopDownMap::loadRasterizedMaps (:213-224) followed by what the constructor does with the rasters (:48-58): the geometric
// layers derived from them and computeDists on both — on the device (tdr_k_map_from_rasters).
static int map_load_rasters(tdr_map* m, const char* dir, int num_classes, float resolution, int center_x, int center_y);
static int map_set_from_rasters(tdr_map* m, const uint8_t* d_planes, int num_classes, int rows, int cols,
                                float resolution, int center_x, int center_y);
static int map_adopt_static(tdr_map* m, int num_classes, int rows, int cols, float resolution, int center_x, int center_y);
int tdr_map_load_rasters(tdr_map* m, const char* dir, int num_classes, float resolution, int center_x, int center_y) {
  try {   // (no exception crosses the C ABI: a file that makes an allocation fail is an error code)
    return map_load_rasters(m, dir, num_classes, resolution, center_x, center_y);
  } catch (const std::exception& e) {
    return failh(TDR_ERR_NOMEM, "map_load_rasters: %s", e.what());
  }
}
static int map_load_rasters(tdr_map* m, const char* dir, int num_classes, float resolution, int center_x, int center_y) {
  if (!m || !dir) return failh(TDR_ERR_ARG, "map_load_rasters: null pointer");
  if (num_classes < 1 || num_classes > TDR_MAX_CLASSES || !(resolution > 0.f))
    return failh(TDR_ERR_ARG, "map_load_rasters: bad class count / resolution");
  std::vector<uint8_t> planes, one;
  int w = 0, h = 0;
  for (int c = 0; c < num_classes; c++) {
    int w2 = 0, h2 = 0;
    TTRY(tdr_png_read_gray8((std::string(dir) + "/class" + std::to_string(c) + ".png").c_str(), one, w2, h2));
    if (c == 0) { w = w2; h = h2; }
    if (w2 != w || h2 != h) return failh(TDR_ERR_ARG, "map_load_rasters: class%d.png differs in size from class0.png", c);
    planes.insert(planes.end(), one.begin(), one.end());
  }
  const int rows = h, cols = w;
  DevBuf<uint8_t> d_planes;
  TTRY(d_planes.resize(planes.size()));
  HTRY(hipMemcpy(d_planes.p, planes.data(), planes.size(), hipMemcpyHostToDevice));
  return map_set_from_rasters(m, d_planes.p, num_classes, rows, cols, resolution, center_x, center_y);
}
// what the constructor does with the class rasters of a static map (:48-58), from DEVICE planes in the class<i>.png layout
static int map_set_from_rasters(tdr_map* m, const uint8_t* d_planes, int num_classes, int rows, int cols,
                                float resolution, int center_x, int center_y) {
  m->inc_valid = false;
  DevBuf<uint8_t> d_ws;
  TTRY(d_ws.resize(tdr_map_ingest_workspace_bytes(num_classes, rows, cols)));
  TTRY(m->rec.resize(tdr_map_rec_floats_total(num_classes, rows, cols)));
  TTRY(tdr_k_map_from_rasters(d_planes, num_classes, rows, cols, resolution, m->rec.p, d_ws.p, nullptr));
  return map_adopt_static(m, num_classes, rows, cols, resolution, center_x, center_y);
}
// the rest of the constructor for a static map whose cell records m->rec now hold (:48-63): host copies of class_maps_ /
// class_mask_, compact records, geometric layers derived from the classes, have_map_ = true
static int map_adopt_static(tdr_map* m, int num_classes, int rows, int cols, float resolution, int center_x, int center_y) {
  m->inc_valid = false;
  const size_t ncell = (size_t)rows * cols;
  DevBuf<uint8_t> d_mask;
  DevBuf<float> d_maps;
  TTRY(d_maps.resize(ncell * num_classes));
  TTRY(d_mask.resize(ncell));
  TTRY(tdr_k_unpack_map(m->rec.p, num_classes, rows, cols, d_maps.p, d_mask.p, nullptr));
  m->maps_host.resize(ncell * num_classes);
  m->mask_host.resize(ncell);
  HTRY(hipMemcpy(m->maps_host.data(), d_maps.p, ncell * num_classes * sizeof(float), hipMemcpyDeviceToHost));
  HTRY(hipMemcpy(m->mask_host.data(), d_mask.p, ncell, hipMemcpyDeviceToHost));
  m->desc.rec = m->rec.p;
  m->desc.ncls = num_classes;
  m->desc.rows = rows;
  m->desc.cols = cols;
  m->desc.rec_floats = tdr_rec_floats(num_classes);
  m->desc.resolution = resolution;
  m->center_x = center_x;
  m->center_y = center_y;
  TTRY(map_compact(m));
  TTRY(map_make_geo(m, false));   // getGeoRasterMap + computeDists (:48-58)
  m->have_map = true;             // :63
  if (m->nb > 0) return tdr_map_sample_pts_polar(m, m->nb, m->nr, m->ang_res);
  return TDR_OK;
}

// ---- the static vector map (src/top_down_map.cpp:22-31, 66-110, 328-365, 391-408) -------------------------------------
// the fill runs on the device (csrc/tdr_poly.hip), the planes then take the raster cache's path into the map
}  // extern "C"
int tdr_poly_grid(int width, int height, float resolution, int* rows, int* cols);                  // tdr_poly.hip
int tdr_poly_fill(const float* verts, const int64_t* offs, const int32_t* cls, int64_t n_poly, int width, int height,
                  float resolution, int ncls, const uint32_t* excl_above, uint8_t* planes_cm, uint8_t* raster,
                  hipStream_t s);
int tdr_svg_parse_internal(const char* path, float* w, float* h, std::vector<uint32_t>& keys, std::vector<int64_t>& offs,
                           std::vector<float>& verts);                                               // tdr_svg.cpp

// the checks every polygon entry makes before it touches the device; excl_above[u] = the exclusive classes c > u that
// clear u (u itself listed).  With binary planes the reference's loop (:356-365: plane[u] += 1 - plane[c] for listed
// u < c, then min(., 1)) clears u exactly where any listed c > u is inside: a plane changed earlier in the loop only
// lost cells some still higher listed class covers, so the union over c > u is the same, and repeats change nothing.
static int poly_check(int num_classes, const int32_t* exclusive, int n_excl, float resolution, uint32_t* excl_above,
                      const char* who) {
  if (num_classes < 1 || num_classes > TDR_MAX_CLASSES)
    return failh(TDR_ERR_ARG, "%s: num_classes %d outside [1, %d]", who, num_classes, TDR_MAX_CLASSES);
  if (n_excl < 0 || (n_excl > 0 && !exclusive)) return failh(TDR_ERR_ARG, "%s: null exclusive list", who);
  if (!(resolution > 0.f) || !std::isfinite(resolution)) return failh(TDR_ERR_ARG, "%s: resolution must be > 0", who);
  if ((int)std::ceil(50.0 / (double)resolution) > 250)
    return failh(TDR_ERR_ARG, "%s: resolution %g needs a distance window over 250 cells", who, (double)resolution);
  for (int k = 0; k < TDR_MAX_CLASSES; k++) excl_above[k] = 0;
  uint32_t listed = 0;
  for (int k = 0; k < n_excl; k++) {
    if (exclusive[k] < 0 || exclusive[k] >= num_classes)
      return failh(TDR_ERR_ARG, "%s: exclusive class %d outside [0, %d)", who, exclusive[k], num_classes);
    listed |= 1u << exclusive[k];
  }
  for (int u = 0; u < num_classes; u++)
    if (listed & (1u << u)) excl_above[u] = listed & ~((2u << u) - 1u);
  return TDR_OK;
}

static int map_load_polygons(tdr_map* m, const float* verts, const int64_t* offs, const int32_t* cls, int64_t n_poly,
                             int width, int height, int num_classes, const uint32_t* excl_above, float resolution,
                             int center_x, int center_y, uint8_t* planes_out) {
  int rows = 0, cols = 0;
  TTRY(tdr_poly_grid(width, height, resolution, &rows, &cols));
  const size_t ncell = (size_t)rows * cols;
  DevBuf<uint8_t> d_planes, d_raster;
  TTRY(d_planes.resize(ncell * num_classes));
  TTRY(d_raster.resize(ncell * num_classes));
  TTRY(tdr_poly_fill(verts, offs, cls, n_poly, width, height, resolution, num_classes, excl_above, d_planes.p, d_raster.p,
                     nullptr));
  if (planes_out) HTRY(hipMemcpy(planes_out, d_planes.p, ncell * num_classes, hipMemcpyDeviceToHost));
  d_planes.release();
  return map_set_from_rasters(m, d_raster.p, num_classes, rows, cols, resolution, center_x, center_y);
}

extern "C" {
int tdr_map_load_polygons(tdr_map* m, const float* verts, const int64_t* poly_offsets, const int32_t* poly_class,
                          int64_t n_poly, int width, int height, int num_classes, const int32_t* exclusive, int n_excl,
                          float resolution, int center_x, int center_y, uint8_t* planes_out) {
  const char* who = "map_load_polygons";
  if (n_poly < 0 || (n_poly > 0 && (!verts || !poly_offsets || !poly_class)))
    return failh(TDR_ERR_ARG, "%s: null polygon arrays", who);
  uint32_t above[TDR_MAX_CLASSES];
  TTRY(poly_check(num_classes, exclusive, n_excl, resolution, above, who));
  int rows = 0, cols = 0;
  TTRY(tdr_poly_grid(width, height, resolution, &rows, &cols));
  if (n_poly > 0 && poly_offsets[0] < 0) return failh(TDR_ERR_ARG, "%s: negative vertex offset", who);
  for (int64_t p = 0; p < n_poly; p++)
    if (poly_offsets[p + 1] < poly_offsets[p]) return failh(TDR_ERR_ARG, "%s: vertex offsets decrease at %lld", who, (long long)p);
  if (!m) return failh(TDR_ERR_ARG, "%s: null map", who);
  try {
    return map_load_polygons(m, verts, poly_offsets, poly_class, n_poly, width, height, num_classes, above, resolution,
                             center_x, center_y, planes_out);
  } catch (const std::exception& e) {
    return failh(TDR_ERR_NOMEM, "%s: %s", who, e.what());
  }
}

int tdr_polygon_planes(const float* verts, const int64_t* poly_offsets, const int32_t* poly_class, int64_t n_poly,
                       int width, int height, int num_classes, const int32_t* exclusive, int n_excl, float resolution,
                       uint8_t* planes_out) {
  const char* who = "polygon_planes";
  if (n_poly < 0 || (n_poly > 0 && (!verts || !poly_offsets || !poly_class)))
    return failh(TDR_ERR_ARG, "%s: null polygon arrays", who);
  uint32_t above[TDR_MAX_CLASSES];
  TTRY(poly_check(num_classes, exclusive, n_excl, resolution, above, who));
  int rows = 0, cols = 0;
  TTRY(tdr_poly_grid(width, height, resolution, &rows, &cols));
  if (n_poly > 0 && poly_offsets[0] < 0) return failh(TDR_ERR_ARG, "%s: negative vertex offset", who);
  for (int64_t p = 0; p < n_poly; p++)
    if (poly_offsets[p + 1] < poly_offsets[p]) return failh(TDR_ERR_ARG, "%s: vertex offsets decrease at %lld", who, (long long)p);
  if (!planes_out) return failh(TDR_ERR_ARG, "%s: null planes_out", who);
  if (tdr_device_count() < 1) return failh(TDR_ERR_HIP, "%s: no HIP device (there is no CPU fallback)", who);
  try {
    const size_t ncell = (size_t)rows * cols;
    DevBuf<uint8_t> d_planes;
    TTRY(d_planes.resize(ncell * num_classes));
    TTRY(tdr_poly_fill(verts, poly_offsets, poly_class, n_poly, width, height, resolution, num_classes, above, d_planes.p,
                       nullptr, nullptr));
    HTRY(hipMemcpy(planes_out, d_planes.p, ncell * num_classes, hipMemcpyDeviceToHost));
    return TDR_OK;
  } catch (const std::exception& e) {
    return failh(TDR_ERR_NOMEM, "%s: %s", who, e.what());
  }
}

int tdr_map_load_svg(tdr_map* m, const char* path, const uint32_t* fill_keys, const int32_t* flatten_lut, int lut_size,
                     int num_classes, const int32_t* exclusive, int n_excl, float resolution, int center_x, int center_y) {
  const char* who = "map_load_svg";
  if (!path || lut_size < 0 || (lut_size > 0 && (!fill_keys || !flatten_lut)))
    return failh(TDR_ERR_ARG, "%s: null path / lookup tables", who);
  uint32_t above[TDR_MAX_CLASSES];
  TTRY(poly_check(num_classes, exclusive, n_excl, resolution, above, who));
  if (!m) return failh(TDR_ERR_ARG, "%s: null map", who);
  try {
    float w = 0, h = 0;
    std::vector<uint32_t> keys;
    std::vector<int64_t> offs;
    std::vector<float> verts;
    TTRY(tdr_svg_parse_internal(path, &w, &h, keys, offs, verts));
    // loadSvg :77-103: per LUT index, the polygons of every shape of its colour, into its flattened class
    std::vector<float> cv;
    std::vector<int64_t> co(1, 0);
    std::vector<int32_t> cc;
    for (int l = 0; l < lut_size; l++) {
      if (flatten_lut[l] < 0 || flatten_lut[l] >= num_classes) continue;
      for (size_t p = 0; p < keys.size(); p++) {
        if (keys[p] == TDR_SVG_NO_KEY || keys[p] != (fill_keys[l] & 0xFFFFFFu)) continue;
        cv.insert(cv.end(), verts.begin() + 2 * offs[p], verts.begin() + 2 * offs[p + 1]);
        co.push_back((int64_t)(cv.size() / 2));
        cc.push_back(flatten_lut[l]);
      }
    }
    const int W = (int)w, H = (int)h;   // Eigen::Vector2i map_size{width, height} (:107)
    return map_load_polygons(m, cv.data(), co.data(), cc.data(), (int64_t)cc.size(), W, H, num_classes, above, resolution,
                             center_x, center_y, nullptr);
  } catch (const std::exception& e) {
    return failh(TDR_ERR_NOMEM, "%s: %s", who, e.what());
  }
}

// ---- the static colour raster map (src/top_down_map.cpp:32-42, then :48-63) -----------------------------------------
// cv::imread (csrc/tdr_png.cpp for PNG), color2Ind + loadCompressedRasterMap + computeDists on the device
// (tdr_k_map_from_color), then what the constructor does with every static map.  Geometric layers: on this branch
// loadCompressedRasterMap leaves two constant-1 geo_maps_ (:126-133) and the constructor appends two more (:48-52), so
// getGeoRasterMap (:410-427) and computeDists (:58) see four layers.  getGeoRasterMap zeroes all four, fills layer 1,
// re-binarises all four (layers 2 and 3 become all 1) and sets layer 0 = 1 - layer 1; computeDists transforms each layer
// on its own, and its mask (:294-299: a cell is masked where the four binary values sum past 4 - 1 = 3) is never set,
// since layers 0 + 1 always sum to 1 and layers 2 + 3 to 2 — as with two layers (sum 1, never past 1).  So layers 0 and
// 1 are those of the other static branches.  Layers 2 and 3 are not kept: the cache holds two (:252-256, :277-280) and
// only getLocalGeoMap, which the node does not call, could reach them.
static int color_check(const uint32_t* fill_keys, const int32_t* flatten_lut, int lut_size, int num_classes,
                       float resolution, const char* who) {
  if (!fill_keys || !flatten_lut) return failh(TDR_ERR_ARG, "%s: null lookup tables", who);
  if (lut_size < 1 || lut_size > 256) return failh(TDR_ERR_ARG, "%s: lut_size %d outside [1, 256]", who, lut_size);
  if (num_classes < 1 || num_classes > TDR_MAX_CLASSES)
    return failh(TDR_ERR_ARG, "%s: num_classes %d outside [1, %d]", who, num_classes, TDR_MAX_CLASSES);
  if (!(resolution > 0.f) || !std::isfinite(resolution)) return failh(TDR_ERR_ARG, "%s: resolution must be > 0", who);
  if ((int)std::ceil(50.0 / (double)resolution) > 250)
    return failh(TDR_ERR_ARG, "%s: resolution %g needs a distance window over 250 cells", who, (double)resolution);
  return TDR_OK;
}
static int color_shape(int img_h, int img_w, float resolution, const char* who) {
  if (img_h < 1 || img_w < 1 || img_h > (1 << 24) || img_w > (1 << 24))
    return failh(TDR_ERR_ARG, "%s: image size %d x %d outside [1, 2^24]", who, img_w, img_h);
  int rows = 0, cols = 0;
  TTRY(tdr_map_ingest_shape(img_h, img_w, resolution, &rows, &cols));
  if (rows < 1 || cols < 1) return failh(TDR_ERR_ARG, "%s: image size %d x %d gives an empty map", who, img_w, img_h);
  return TDR_OK;
}
static int map_load_color(tdr_map* m, const uint8_t* bgr, int img_h, int img_w, const uint32_t* fill_keys,
                          const int32_t* flatten_lut, int lut_size, int num_classes, float resolution, int center_x,
                          int center_y) {
  int rows = 0, cols = 0;
  m->inc_valid = false;
  TTRY(tdr_map_ingest_shape(img_h, img_w, resolution, &rows, &cols));
  const size_t nbytes = (size_t)img_h * img_w * 3;
  DevBuf<uint8_t> d_img, d_ws;
  TTRY(d_img.resize(nbytes));
  TTRY(d_ws.resize(tdr_map_ingest_workspace_bytes(num_classes, rows, cols)));
  HTRY(hipMemcpy(d_img.p, bgr, nbytes, hipMemcpyHostToDevice));
  TTRY(m->rec.resize(tdr_map_rec_floats_total(num_classes, rows, cols)));
  TTRY(tdr_k_map_from_color(d_img.p, img_h, img_w, fill_keys, flatten_lut, lut_size, num_classes, resolution, m->rec.p,
                            d_ws.p, nullptr));
  return map_adopt_static(m, num_classes, rows, cols, resolution, center_x, center_y);
}

int tdr_map_load_color_image(tdr_map* m, const uint8_t* bgr, int img_h, int img_w, const uint32_t* fill_keys,
                             const int32_t* flatten_lut, int lut_size, int num_classes, float resolution, int center_x,
                             int center_y) {
  const char* who = "map_load_color_image";
  if (!bgr) return failh(TDR_ERR_ARG, "%s: null image", who);
  TTRY(color_check(fill_keys, flatten_lut, lut_size, num_classes, resolution, who));
  TTRY(color_shape(img_h, img_w, resolution, who));
  if (!m) return failh(TDR_ERR_ARG, "%s: null map", who);
  try {
    return map_load_color(m, bgr, img_h, img_w, fill_keys, flatten_lut, lut_size, num_classes, resolution, center_x,
                          center_y);
  } catch (const std::exception& e) {
    return failh(TDR_ERR_NOMEM, "%s: %s", who, e.what());
  }
}

int tdr_map_load_color_png(tdr_map* m, const char* path, const uint32_t* fill_keys, const int32_t* flatten_lut,
                           int lut_size, int num_classes, float resolution, int center_x, int center_y) {
  const char* who = "map_load_color_png";
  if (!path) return failh(TDR_ERR_ARG, "%s: null path", who);
  TTRY(color_check(fill_keys, flatten_lut, lut_size, num_classes, resolution, who));
  if (!m) return failh(TDR_ERR_ARG, "%s: null map", who);
  try {
    std::vector<uint8_t> bgr;
    int w = 0, h = 0;
    TTRY(tdr_png_read_bgr8(path, bgr, w, h));   // cv::imread (:35)
    TTRY(color_shape(h, w, resolution, who));
    return map_load_color(m, bgr.data(), h, w, fill_keys, flatten_lut, lut_size, num_classes, resolution, center_x,
                          center_y);
  } catch (const std::exception& e) {
    return failh(TDR_ERR_NOMEM, "%s: %s", who, e.what());
  }
}

// TopDownMap::getClassesAtPoint(Vector2i) (top_down_map.cpp:159-170): bit c set = class c present (< 1 px away)
int tdr_map_classes_at_point(const tdr_map* m, int px, int py, uint32_t* class_bits) {
  if (!m || !class_bits || !m->have_map) return failh(TDR_ERR_ARG, "classes_at_point: no map");
  const int rows = m->desc.rows, cols = m->desc.cols;
  const int c0 = (int)((float)px / m->desc.resolution), c1 = (int)((float)py / m->desc.resolution);
  uint32_t bits = 0;
  if (c0 < cols && c1 < rows && c0 >= 0 && c1 >= 0)
    for (int c = 0; c < m->desc.ncls; c++)
      if (m->maps_host[(size_t)c * rows * cols + c1 + (size_t)rows * c0] < 1) bits |= 1u << c;
  *class_bits = bits;
  return TDR_OK;
}

// ---- ScanRenderer(Polar) ------------------------------------------------------------------------------------------------
int tdr_renderer_create(const int32_t* flatten_lut256, tdr_renderer** out) {
  if (!flatten_lut256 || !out) return failh(TDR_ERR_ARG, "renderer_create: null pointer");
  if (tdr_device_count() < 1) return failh(TDR_ERR_HIP, "renderer_create: no HIP device (there is no CPU fallback)");
  tdr_renderer* r = new tdr_renderer();
  int rc = r->lut.resize(256);
  if (rc == TDR_OK && hipMemcpy(r->lut.p, flatten_lut256, 256 * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
    rc = failh(TDR_ERR_HIP, "renderer_create: lut upload failed");
  if (rc != TDR_OK) {
    delete r;
    return rc;
  }
  *out = r;
  return TDR_OK;
}
void tdr_renderer_destroy(tdr_renderer* r) { delete r; }

// renderSemanticTopDown (scan_renderer_polar.cpp:83-109 when polar != 0, scan_renderer.cpp:55-78 otherwise).
// pts: HOST points; imgs_out: HOST [ncls][rows*cols] column-major images, written in place (may be NULL: the render
// then only stays on the device for tdr_filter_update).
int tdr_renderer_render(tdr_renderer* r, int polar, const float* pts, int stride, int ioff, int64_t n, float res,
                        float ang_res, int ncls, int rows, int cols, float* imgs_out) {
  if (!r) return failh(TDR_ERR_ARG, "render: null renderer");
  if (n < 0 || (n > 0 && !pts)) return failh(TDR_ERR_ARG, "render: null points");
  if (ncls < 1 || rows < 1 || cols < 1) return TDR_OK;  // `if (imgs.size() < 1) return;` (:85)
  const size_t P = (size_t)rows * cols;
  if (r->render_async) {   // (a tdr_batch_render_polar still writing img / pk)
    HTRY(hipEventSynchronize(r->rendered));
    r->render_async = false;
  }
  TTRY(r->pts.resize((size_t)std::max<int64_t>(n, 1) * stride));
  TTRY(r->img.resize(P * ncls));
  TTRY(r->pk.resize(P * tdr_rec_floats(ncls)));
  if (n > 0) HTRY(hipMemcpy(r->pts.p, pts, (size_t)n * stride * sizeof(float), hipMemcpyHostToDevice));
  TTRY(r->keys.resize((size_t)tdr_raster_workspace_bytes(std::max<int64_t>(n, 1))));
  if (polar)
    TTRY(tdr_k_raster_polar(r->pts.p, stride, ioff, n, res, ang_res, r->lut.p, ncls, rows, cols, r->img.p, r->pk.p,
                            r->keys.p, nullptr));
  else
    TTRY(tdr_k_raster_cart(r->pts.p, stride, ioff, n, res, r->lut.p, ncls, rows, cols, r->img.p, r->pk.p, r->keys.p,
                           nullptr));
  if (imgs_out) HTRY(hipMemcpy(imgs_out, r->img.p, P * ncls * sizeof(float), hipMemcpyDeviceToHost));
  else HTRY(hipDeviceSynchronize());
  r->ncls = ncls;
  r->rows = rows;
  r->cols = cols;
  r->polar = polar != 0;
  r->have_scan = true;
  return TDR_OK;
}

// renderGeometricTopDown (scan_renderer_polar.cpp:6-81 when polar != 0, scan_renderer.cpp:7-53 otherwise).  pts: HOST
// organised cloud (element idy*width + idx); imgs_out: HOST [2][rows*cols] column-major (ground, obstacles).
int tdr_renderer_render_geo(tdr_renderer* r, int polar, const float* pts, int stride, int64_t width, int64_t height,
                            float res, float ang_res, int rows, int cols, float* imgs_out) {
  if (!r || !imgs_out) return failh(TDR_ERR_ARG, "render_geo: null pointer");
  const int64_t n = width * height;
  if (width < 0 || height < 0 || (n > 0 && !pts)) return failh(TDR_ERR_ARG, "render_geo: bad cloud");
  if (rows < 1 || cols < 1) return TDR_OK;
  const size_t P = (size_t)rows * cols;
  TTRY(r->pts.resize((size_t)std::max<int64_t>(n, 1) * stride));
  TTRY(r->geo.resize(2 * P));
  if (n > 0) HTRY(hipMemcpy(r->pts.p, pts, (size_t)n * stride * sizeof(float), hipMemcpyHostToDevice));
  if (polar) {
    TTRY(r->geo_ws.resize((size_t)tdr_raster_geo_workspace_bytes(std::max<int64_t>(n, 1))));
    TTRY(tdr_k_raster_geo_polar(r->pts.p, stride, width, height, res, ang_res, rows, cols, r->geo.p, r->geo_ws.p, nullptr));
  } else {
    TTRY(tdr_k_raster_geo_cart(r->pts.p, stride, width, height, res, rows, cols, r->geo.p, nullptr));
  }
  HTRY(hipMemcpy(imgs_out, r->geo.p, 2 * P * sizeof(float), hipMemcpyDeviceToHost));
  return TDR_OK;
}

// ---- ParticleFilter ------------------------------------------------------------------------------------------------------
static int filter_create(tdr_map* map, int n_max, const tdr_filter_params* fp, uint32_t seed, tdr_comm* comm,
                         tdr_filter** out) {
  if (!map || !fp || !out || n_max < 1) return failh(TDR_ERR_ARG, "filter_create: bad arguments");
  const int world = comm ? tdr_comm_world(comm) : 1;
  if (n_max % world) return failh(TDR_ERR_ARG, "filter_create: n_max = %d is not a multiple of the %d ranks", n_max, world);
  tdr_filter* f = new tdr_filter();
  f->map = map;
  f->fp = *fp;
  f->n_max = n_max;
  f->comm = comm;
  f->world = world;
  f->rank = comm ? tdr_comm_rank(comm) : 0;
  f->cap = n_max / world;
  f->seed = seed;
  f->rng = tdr_rng_create(seed);  // explicit seed instead of std::random_device (particle_filter.cpp:4-5)
  // seed 0 = "unseeded", like the reference's std::random_device: nothing to reproduce, so propagate draws its noise on
  // the device; a non-zero seed asks for the reference-ordered std::mt19937 stream (tdr_filter_configure overrides)
  f->parity_rng = seed != 0;
  int rc = TDR_OK;
  const size_t cap = (size_t)f->cap, N = (size_t)n_max;
  if (rc == TDR_OK) rc = f->st.resize(TDR_ST_FIELDS * cap);
  if (rc == TDR_OK) rc = f->st_new.resize(TDR_ST_FIELDS * cap);
  if (rc == TDR_OK) rc = f->last_dist.resize(cap);
  if (rc == TDR_OK) rc = f->raw_w.resize(cap);
  if (rc == TDR_OK) rc = f->w.resize(N);
  if (rc == TDR_OK) rc = f->runmax.resize(N);
  if (rc == TDR_OK) rc = f->pfx_ws.resize((size_t)tdr_prefix_workspace_bytes((int64_t)N));
  if (rc == TDR_OK) rc = f->idx.resize(cap);
  if (rc == TDR_OK) rc = f->perm.resize(cap);
  if (rc == TDR_OK) rc = f->info.resize(TDR_UW_INFO_FLOATS);
  if (rc == TDR_OK) rc = f->stats.resize(TDR_MEAN_COV_FLOATS);
  if (rc == TDR_OK) rc = f->aos.resize(N);
  if (rc == TDR_OK) rc = f->z4.resize(4 * cap);
  if (rc == TDR_OK && comm) {
    rc = f->xchg_in.resize(2 * cap);
    if (rc == TDR_OK) rc = f->xchg_out.resize(2 * N);
    if (rc == TDR_OK) rc = f->raw_glob.resize(N);
    if (rc == TDR_OK) rc = f->ld_glob.resize(N);
    if (rc == TDR_OK) rc = f->st_send.resize(TDR_ST_FIELDS * cap);
    if (rc == TDR_OK) rc = f->st_all.resize(TDR_ST_FIELDS * N);
    if (rc == TDR_OK) rc = f->st_glob.resize(TDR_ST_FIELDS * N);
  }
  if (rc == TDR_OK && hipMemset(f->last_dist.p, 0, cap * sizeof(float)) != hipSuccess) rc = failh(TDR_ERR_HIP, "memset");
  if (rc == TDR_OK) rc = tdr_score_ctx_create(&f->score_ctx);
  if (rc != TDR_OK) {
    tdr_filter_destroy(f);
    return rc;
  }
  *out = f;
  return TDR_OK;
}
int tdr_filter_create(tdr_map* map, int n_max, const tdr_filter_params* fp, uint32_t seed, tdr_filter** out) {
  return filter_create(map, n_max, fp, seed, nullptr, out);
}
// the Cartesian filter (BASELINE config 4): the same object, its scoring stage is filter_score's Cartesian branch
int tdr_filter_create_cart(tdr_map* map, int n_max, const tdr_filter_params* fp, uint32_t seed, tdr_filter** out) {
  if (map && (map->win_rows < 1 || map->win_cols < 1))
    return failh(TDR_ERR_ARG, "filter_create_cart: the map has no window (tdr_map_set_window)");
  TTRY(filter_create(map, n_max, fp, seed, nullptr, out));
  (*out)->cart = true;
  return TDR_OK;
}
// particles sharded over the ranks of `comm` (not owned; must outlive the filter)
int tdr_filter_create_sharded(tdr_map* map, int n_max, const tdr_filter_params* fp, uint32_t seed, tdr_comm* comm,
                              tdr_filter** out) {
  if (!comm) return failh(TDR_ERR_ARG, "filter_create_sharded: null comm");
  return filter_create(map, n_max, fp, seed, comm, out);
}
int64_t tdr_filter_num_local(const tdr_filter* f) { return f ? f->nl() : 0; }
void tdr_filter_destroy(tdr_filter* f) {
  if (!f) return;
  if (f->rng && f->rng_owned) tdr_rng_destroy(f->rng);
  tdr_score_ctx_destroy(f->score_ctx);
  tdr_rng_pipe_destroy(f->pipe);
  delete f;
}

static int rng_to_host(tdr_filter* f);   // (below, with the propagate step)
int tdr_filter_configure(tdr_filter* f, int parity_rng, int locality_every) {
  if (!f) return failh(TDR_ERR_ARG, "filter_configure: null filter");
  if (!parity_rng) TTRY(rng_to_host(f));
  f->parity_rng = parity_rng != 0;
  f->locality_every = locality_every;
  return TDR_OK;
}

static void note_uniform_scale(tdr_filter* f, const tdr_state* s, int64_t n) {
  f->uniform_scale = 0.f;
  if (!f->scale_frozen || n < 1 || !(s[0].scale > 0)) return;
  for (int64_t i = 1; i < n; i++)
    if (s[i].scale != s[0].scale) return;
  f->uniform_scale = s[0].scale;
}

// states: the GLOBAL particle array; a sharded filter keeps this rank's slice
int tdr_filter_set_states(tdr_filter* f, const tdr_state* states, int64_t n) {
  if (!f || (n > 0 && !states) || n < 0 || n > f->n_max) return failh(TDR_ERR_ARG, "filter_set_states: bad arguments");
  if (n % f->world) return failh(TDR_ERR_ARG, "filter_set_states: %lld particles over %d ranks", (long long)n, f->world);
  const int64_t nl = n / f->world;
  if (nl > 0) {
    HTRY(hipMemcpy(f->aos.p, states + (size_t)f->rank * nl, (size_t)nl * sizeof(tdr_state), hipMemcpyHostToDevice));
    TTRY(tdr_k_states_aos_to_soa(f->aos.p, nl, f->st.p, f->cap, f->stream));
    HTRY(hipDeviceSynchronize());
  }
  f->n = n;
  f->states_changed();
  f->maybe_uninit = false;
  for (int64_t i = 0; i < n; i++) f->maybe_uninit |= states[i].have_init == 0;
  if (f->fp.fixed_scale > 0) f->scale_frozen = true;
  note_uniform_scale(f, states, n);
  return TDR_OK;
}

// this rank's particles (all of them when the filter is not sharded): n <= tdr_filter_num_local
int tdr_filter_get_states(tdr_filter* f, tdr_state* out, int64_t n) {
  if (!f || !out || n < 0 || n > f->nl()) return failh(TDR_ERR_ARG, "filter_get_states: bad arguments");
  if (n == 0) return TDR_OK;
  TTRY(tdr_k_states_soa_to_aos(f->st.p, f->cap, n, f->aos.p, f->stream));
  HTRY(hipMemcpy(out, f->aos.p, (size_t)n * sizeof(tdr_state), hipMemcpyDeviceToHost));
  return TDR_OK;
}

// The particle loop of initializeParticles on the device, on the filter's own generator (which stays there): every rank
// runs the whole chain and writes its slice; the bookkeeping is tdr_filter_set_states' for the states the loop makes
// (one heading rule and one scale rule for all of them).
static int rng_to_device(tdr_filter* f);
static bool rng_device_capable(const tdr_filter* f);
static int initialize_on_device(tdr_filter* f) {
  tdr_map* m = f->map;
  const tdr_filter_params& p = f->fp;
  int64_t n = std::min<int64_t>(tdr_init_particles_count(&p, (int)f->n_max), f->n_max);
  n -= n % f->world;
  const int64_t nl = n / f->world;
  TTRY(rng_to_device(f));
  DevBuf<uint8_t> ws;
  TTRY(ws.resize(tdr_init_workspace_bytes()));
  int64_t made = 0;
  TTRY(tdr_rng_pipe_init_particles(f->pipe, &m->desc, &p, (int)f->n_max, (int64_t)f->rank * nl, (int64_t)(f->rank + 1) * nl,
                                   f->st.p, f->cap, &made, ws.p, f->stream));
  HTRY(hipStreamSynchronize(f->stream));
  f->n = n;
  f->states_changed();
  f->maybe_uninit = n > 0 && p.init_pos_deg_theta == std::numeric_limits<float>::infinity();
  if (p.fixed_scale > 0) f->scale_frozen = true;
  // note_uniform_scale: a fixed scale is every particle's; the unknown-scale groups hold ten different scales
  f->uniform_scale = (f->scale_frozen && n > 0 && p.fixed_scale > 0) ? p.fixed_scale : 0.f;
  return TDR_OK;
}

// ParticleFilter::initializeParticles (particle_filter.cpp:19-84)
int tdr_filter_initialize_particles(tdr_filter* f) {
  if (!f || !f->map || !f->map->have_map) return failh(TDR_ERR_ARG, "initialize_particles: no map");
  tdr_map* m = f->map;
  tdr_filter_params& p = f->fp;
  if (p.fixed_scale >= 0) f->scale_frozen = true;  // :23-25
  const float inf = std::numeric_limits<float>::infinity();
  if (f->scale_frozen && p.init_pos_m_x != inf) {   // :27-53
    p.init_pos_px_x = (p.init_pos_m_x * p.fixed_scale) + (float)m->center_x;
    p.init_pos_px_y = (p.init_pos_m_y * p.fixed_scale) + (float)m->center_y;
    if (p.init_pos_px_x < 0 || p.init_pos_px_x >= (float)m->desc.cols || p.init_pos_px_y < 0 ||
        p.init_pos_px_y >= (float)m->desc.rows)
      return TDR_OK;  // "No map received for input loc"
    bool good = false;
    for (int dx = -4; dx <= 4 && !good; dx++)
      for (int dy = -4; dy <= 4 && !good; dy++) {
        uint32_t bits = 0;
        TTRY(tdr_map_classes_at_point(m, (int)(p.init_pos_px_x + dx), (int)(p.init_pos_px_y + dy), &bits));
        good = (bits & 2u) != 0;
      }
    if (!good) return TDR_OK;  // "No road in map at init location"
  }
  if (rng_device_capable(f) && tdr_cfg().init_device != 0) return initialize_on_device(f);
  std::vector<tdr_state> states((size_t)f->n_max + 16);
  int64_t n = 0;
  TTRY(rng_to_host(f));
  TTRY(tdr_init_particles_host(f->rng, m->maps_host.data(), m->desc.ncls, m->desc.rows, m->desc.cols,
                               m->desc.resolution, &p, (int)f->n_max, states.data(), &n));
  n = std::min<int64_t>(n, f->n_max);
  n -= n % f->world;
  return tdr_filter_set_states(f, states.data(), n);
}

// the generator's stream continues on the device / on the host (see tdr_filter::rng_dev)
static bool rng_on_device(const tdr_filter* f) { return f->pipe && tdr_rng_pipe_on_device(f->pipe); }
static int rng_to_device(tdr_filter* f) {
  if (rng_on_device(f)) return TDR_OK;
  if (!f->pipe) TTRY(tdr_rng_pipe_create(f->n_max, &f->pipe));
  return tdr_rng_pipe_from_host(f->pipe, f->rng, f->stream);
}
static int rng_to_host(tdr_filter* f) {
  if (!rng_on_device(f)) return TDR_OK;
  return tdr_rng_pipe_to_host(f->pipe, f->rng, f->stream);
}
static bool rng_device_capable(const tdr_filter* f) { return f->rng_owned && f->parity_rng; }

// ParticleFilter::propagate (particle_filter.cpp:86-92)
static int filter_propagate(tdr_filter* f, float tx, float ty, float omega, bool scale_freeze) {
  if (f->n == 0) return TDR_OK;
  f->states_changed();
  const int64_t nl = f->nl();
  const float* z = nullptr;
  if (rng_device_capable(f)) {
    // the reference draws serially in GLOBAL particle order from one generator: every rank continues the same stream on
    // its device (same state everywhere) and keeps the normals of its own particles — nothing is drawn on the host
    TTRY(rng_to_device(f));
    TTRY(tdr_rng_pipe_normals(f->pipe, f->n, (int64_t)f->rank * nl, (int64_t)(f->rank + 1) * nl, scale_freeze ? 1 : 0, &z,
                              f->stream));
  } else if (f->parity_rng) {
    // a generator shared with the caller (StateParticle's surface): the host draws, serially
    std::vector<float> zh((size_t)4 * f->n);
    TTRY(tdr_propagate_normals_host(f->rng, f->n, scale_freeze ? 1 : 0, zh.data()));
    HTRY(hipMemcpyAsync(f->z4.p, zh.data() + (size_t)4 * f->rank * nl, (size_t)4 * nl * sizeof(float),
                        hipMemcpyHostToDevice, f->stream));
    HTRY(hipStreamSynchronize(f->stream));
    z = f->z4.p;
  }
  return tdr_k_propagate(f->st.p, f->cap, nl, f->last_dist.p, tx, ty, omega, scale_freeze ? 1 : 0, f->fp.pos_cov,
                         f->fp.theta_cov, z, f->seed, f->prop_calls++, (int64_t)f->rank * nl, f->stream);
}
int tdr_filter_propagate(tdr_filter* f, float tx, float ty, float omega) {
  if (!f) return failh(TDR_ERR_ARG, "filter_propagate: null filter");
  return filter_propagate(f, tx, ty, omega, f->scale_frozen);
}
// StateParticle::propagate(trans, omega, scale_freeze) (state_particle.cpp:57-78): the freeze flag is the caller's
int tdr_filter_propagate_freeze(tdr_filter* f, float tx, float ty, float omega, int scale_freeze) {
  if (!f) return failh(TDR_ERR_ARG, "filter_propagate_freeze: null filter");
  return filter_propagate(f, tx, ty, omega, scale_freeze != 0);
}
// The filter draws from the caller's std::mt19937 from now on (the reference's particles share ONE generator with
// their filter, state_particle.h:61-64).  `mt19937` must point to a std::mt19937 of the libstdc++ this library was
// built with; it is not owned.
int tdr_filter_share_rng(tdr_filter* f, void* mt19937) {
  if (!f || !mt19937) return failh(TDR_ERR_ARG, "filter_share_rng: bad arguments");
  if (f->pipe) { tdr_rng_pipe_destroy(f->pipe); f->pipe = nullptr; }   // (the filter's own stream ends here)
  if (f->rng && f->rng_owned) tdr_rng_destroy(f->rng);
  f->rng = mt19937;
  f->rng_owned = false;
  f->parity_rng = true;
  return TDR_OK;
}
// StateParticle's constructor with init == true (state_particle.cpp:3-49) for particle 0 of the filter
int tdr_filter_init_one(tdr_filter* f) {
  if (!f || !f->map || !f->map->have_map) return failh(TDR_ERR_ARG, "filter_init_one: no map");
  tdr_map* m = f->map;
  tdr_state st;
  TTRY(rng_to_host(f));
  TTRY(tdr_init_particle_host(f->rng, m->maps_host.data(), m->desc.ncls, m->desc.rows, m->desc.cols, m->desc.resolution,
                              &f->fp, &st));
  return tdr_filter_set_states(f, &st, 1);
}

// ParticleFilter::update (particle_filter.cpp:94-189).  scan_imgs: HOST [ncls][nb*nr] column-major images, or NULL to
// score against `renderer`'s last render without a host round trip.  n_target < 0 keeps the particle count
// (the adaptive count of :151-157 is an explicit input; the reference feeds it from an OpenCV EM thread).
static int filter_score(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, float res);
static int filter_resample(tdr_filter* f, int64_t n_target);
int tdr_filter_update(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, float res, int64_t n_target) {
  if (!f || !f->map || !f->map->have_map) return failh(TDR_ERR_ARG, "filter_update: no map");
  if (f->n == 0) return TDR_OK;  // :96-99
  TTRY(filter_score(f, scan_imgs, renderer, res));
  const int64_t n = f->n, nl = f->nl();
  const float *raw = f->raw_w.p, *ld = f->last_dist.p;
  if (f->comm) {
    // ONE all-gather of {raw weight, last_dist}: afterwards every rank computes the same statistics and the same
    // order-exact running sum on the same global arrays (replaces the north star's all-reduce, whose result
    // would depend on the reduction tree)
    TTRY(tdr_k_shard_pack2(f->raw_w.p, f->last_dist.p, nl, f->xchg_in.p, f->stream));
    TTRY(tdr_comm_all_gather(f->comm, f->xchg_in.p, f->xchg_out.p, (size_t)2 * nl * sizeof(float), f->stream));
    TTRY(tdr_k_shard_unpack2(f->xchg_out.p, f->world, nl, f->raw_glob.p, f->ld_glob.p, f->stream));
    raw = f->raw_glob.p;
    ld = f->ld_glob.p;
  }
  TTRY(tdr_k_update_weights(raw, ld, n, f->w.p, f->info.p, f->stream));
  return filter_resample(f, n_target);
}
// ParticleFilter::update with the geometric images entering the score (state_particle.cpp:145-152, opt-in)
int tdr_filter_update_geo(tdr_filter* f, const float* scan_imgs, const float* geo_imgs, float res, int64_t n_target) {
  if (!f || !f->map || !f->map->have_map) return failh(TDR_ERR_ARG, "filter_update_geo: no map");
  if (!scan_imgs || !geo_imgs) return failh(TDR_ERR_ARG, "filter_update_geo: null images");
  if (f->comm) return failh(TDR_ERR_ARG, "filter_update_geo: not available on a sharded filter");
  if (f->cart) return failh(TDR_ERR_ARG, "filter_update_geo: there is no Cartesian geometric cost");
  if (f->n == 0) return TDR_OK;
  tdr_map* m = f->map;
  if (m->nb < 1 || !m->tab.p) return failh(TDR_ERR_ARG, "filter_update_geo: samplePtsPolar was never called");
  TTRY(map_ensure_geo(m));
  f->fp.num_classes = m->desc.ncls;
  const int ncls = m->desc.ncls, nb = m->nb, nr = m->nr;
  const size_t P = (size_t)nb * nr;
  TTRY(f->scan_img.resize(P * std::max(ncls, 2)));
  TTRY(f->scan_pk.resize(P * tdr_rec_floats(ncls)));
  TTRY(f->geo_pk.resize(P * 4));
  HTRY(hipMemcpyAsync(f->scan_img.p, scan_imgs, P * ncls * sizeof(float), hipMemcpyHostToDevice, f->stream));
  TTRY(tdr_k_pack_scan(f->scan_img.p, ncls, nb, nr, f->scan_pk.p, f->stream));
  HTRY(hipMemcpyAsync(f->scan_img.p, geo_imgs, P * 2 * sizeof(float), hipMemcpyHostToDevice, f->stream));
  TTRY(tdr_k_pack_scan(f->scan_img.p, 2, nb, nr, f->geo_pk.p, f->stream));
  double gs[2] = {0, 0};   // top_down_geo[i].sum(): Eigen's order is unspecified; counts are small integers, any order is exact
  for (int i = 0; i < 2; i++)
    for (size_t k = 0; k < P; k++) gs[i] += (double)geo_imgs[P * i + k];
  const int64_t n = f->n;
  const int32_t* perm = nullptr;
  if (f->locality_every > 0) {
    TTRY(f->loc_tmp.resize(tdr_locality_tmp_ints(n, m->desc.rows, m->desc.cols)));
    TTRY(tdr_k_locality_order(f->st.p, f->cap, n, m->desc.rows, m->desc.cols, f->perm.p, f->loc_tmp.p, f->stream));
    perm = f->perm.p;
  }
  f->states_changed();   // (the init search writes headings)
  TTRY(f->ws.resize(tdr_score_geo_workspace_floats(ncls, nb, nr, n, n)));
  TTRY(tdr_k_score_polar_geo(&m->desc, &m->geo_desc, m->tab.p, f->scan_pk.p, f->geo_pk.p, (float)gs[0], (float)gs[1], nb, nr,
                             res, &f->fp, f->st.p, f->cap, n, n, perm, f->uniform_scale, f->maybe_uninit ? 1 : 0,
                             f->raw_w.p, f->ws.p, f->stream));
  if (f->maybe_uninit && !(f->fp.force_on_map || f->fp.fixed_scale < 0)) f->maybe_uninit = false;
  TTRY(tdr_k_update_weights(f->raw_w.p, f->last_dist.p, n, f->w.p, f->info.p, f->stream));
  return filter_resample(f, n_target);
}
// StateParticle::computeWeight for every particle (state_particle.cpp:157-219): raw weights only, no statistics, no
// resampling; read them with tdr_filter_get_raw_weights
int tdr_filter_compute_weights(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, float res) {
  if (!f || !f->map || !f->map->have_map) return failh(TDR_ERR_ARG, "filter_compute_weights: no map");
  if (f->n == 0) return TDR_OK;
  return filter_score(f, scan_imgs, renderer, res);
}
int tdr_filter_get_raw_weights(tdr_filter* f, float* out, int64_t n) {
  if (!f || !out || n < 0 || n > f->cap) return failh(TDR_ERR_ARG, "filter_get_raw_weights: bad arguments");
  HTRY(hipMemcpy(out, f->raw_w.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return TDR_OK;
}
int tdr_filter_get_last_dist(tdr_filter* f, float* out, int64_t n) {
  if (!f || !out || n < 0 || n > f->cap) return failh(TDR_ERR_ARG, "filter_get_last_dist: bad arguments");
  HTRY(hipMemcpy(out, f->last_dist.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return TDR_OK;
}
// The half records of the 40-rotation search live in ONE scratch per map and every search rebuilds them for its class
// weights, so searches of the map's filters must not overlap in time — whichever streams they run on (the filters' own,
// the batch's).  A search that may use the scratch runs between these two: wait for the last one, leave an event behind.
static int map_rec16_alloc(tdr_map* m, int64_t n) {
  if (m->desc.rec16 || n < tdr_cfg().rec16_min) return TDR_OK;
  const size_t b16 = tdr_map_rec16_bytes(m->desc.ncls, m->desc.rows, m->desc.cols);
  if (b16) {
    TTRY(m->rec16.resize(b16));
    m->desc.rec16 = m->rec16.p;
  }
  return TDR_OK;
}
static int map_rec16_begin(tdr_map* m, hipStream_t s) {
  if (m->rec16_used) HTRY(hipStreamWaitEvent(s, m->rec16_used, 0));
  return TDR_OK;
}
static int map_rec16_end(tdr_map* m, hipStream_t s) {
  if (!m->rec16_used) HTRY(hipEventCreateWithFlags(&m->rec16_used, hipEventDisableTiming));
  HTRY(hipEventRecord(m->rec16_used, s));
  return TDR_OK;
}
static int filter_score(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, float res) {
  tdr_map* m = f->map;
  if (!f->cart && (m->nb < 1 || !m->tab.p)) return failh(TDR_ERR_ARG, "filter_update: samplePtsPolar was never called");
  if (f->cart && (m->win_rows < 1 || m->win_cols < 1)) return failh(TDR_ERR_ARG, "filter_update: the map has no window");
  f->fp.num_classes = m->desc.ncls;
  // (a Cartesian scan is packed like a polar one with nb = the window's rows, nr = its columns: tdr_k_score_cart)
  const int ncls = m->desc.ncls, nb = f->cart ? m->win_rows : m->nb, nr = f->cart ? m->win_cols : m->nr;
  const size_t P = (size_t)nb * nr;
  const size_t pk_floats = P * tdr_rec_floats(ncls);
  const float* pk = nullptr;
  if (scan_imgs) {
    TTRY(f->scan_img.resize(P * ncls));
    TTRY(f->scan_pk.resize(pk_floats));
    HTRY(hipMemcpyAsync(f->scan_img.p, scan_imgs, P * ncls * sizeof(float), hipMemcpyHostToDevice, f->stream));
    TTRY(tdr_k_pack_scan(f->scan_img.p, ncls, nb, nr, f->scan_pk.p, f->stream));
    pk = f->scan_pk.p;
  } else if (renderer) {
    if (!renderer->have_scan) return failh(TDR_ERR_ARG, "filter_update: no scan");
    if (renderer->ncls != ncls || renderer->rows != nb || renderer->cols != nr)
      return failh(TDR_ERR_ARG, "filter_update: render shape %dx%dx%d does not match the map's %dx%dx%d",
                   renderer->ncls, renderer->rows, renderer->cols, ncls, nb, nr);
    if (f->cart && renderer->polar) return failh(TDR_ERR_ARG, "filter_update: a Cartesian filter needs a Cartesian render");
    pk = renderer->pk.p;
    TTRY(renderer_wait_render(renderer, f->stream));
  } else if (!(f->comm && f->rank != 0)) {
    return failh(TDR_ERR_ARG, "filter_update: no scan");
  }
  if (f->comm) {
    // the rasterised scan is produced once, on rank 0, and broadcast (north star): 2 MB at config 2
    TTRY(f->pk_recv.resize(pk_floats));
    if (f->rank == 0) HTRY(hipMemcpyAsync(f->pk_recv.p, pk, pk_floats * sizeof(float), hipMemcpyDeviceToDevice, f->stream));
    TTRY(tdr_comm_broadcast(f->comm, f->pk_recv.p, pk_floats * sizeof(float), 0, f->stream));
    pk = f->pk_recv.p;
  }
  const int64_t n = f->nl();   // this rank's particles
  const int32_t* perm = nullptr;
  if (f->cart) {
    // windows that rotate with the particle: the heading belongs in the order's key.  The search runs first (it only
    // chooses headings), the regular launch then scores every particle, as the polar path does.
    f->states_changed();
    if (f->maybe_uninit) {
      TTRY(f->init_ws.resize(tdr_score_cart_init_workspace_floats(ncls, nb, nr, n, f->n)));
      TTRY(tdr_k_score_cart_init(&m->desc, pk, nb, nr, res, &f->fp, f->st.p, f->cap, n, f->n, f->init_ws.p, f->stream));
      f->maybe_uninit = false;   // no gates: every particle has a heading now
    }
    if (f->locality_every > 0) {
      TTRY(f->loc_tmp.resize(tdr_locality_pose_tmp_ints(n) + 2));
      TTRY(tdr_k_locality_order_pose(f->st.p, f->cap, n, m->desc.rows, m->desc.cols, (float)(nb + nr) / 16.f, f->perm.p,
                                     f->loc_tmp.p, f->stream));
      perm = f->perm.p;
    }
    TTRY(f->ws.resize(tdr_score_cart_workspace_floats(ncls, nb, nr, n, f->n)));
    TTRY(tdr_k_score_cart(&m->desc, pk, nb, nr, res, &f->fp, f->st.p, f->cap, n, f->n, perm, f->raw_w.p, f->ws.p, f->stream));
    if (renderer && !scan_imgs) TTRY(renderer_note_read(renderer, f->stream));
    return TDR_OK;
  }
  if (f->locality_every > 0) {
    TTRY(f->loc_tmp.resize(tdr_locality_tmp_ints(n, m->desc.rows, m->desc.cols)));
    TTRY(tdr_k_locality_order(f->st.p, f->cap, n, m->desc.rows, m->desc.cols, f->perm.p, f->loc_tmp.p, f->stream));
    perm = f->perm.p;
  }
  f->states_changed();   // (the init search writes headings)
  TTRY(f->ws.resize(tdr_score_workspace_floats(ncls, nb, nr, n, f->n)));
  // the search over this many particles pays for pre-split half records
  if (f->maybe_uninit) TTRY(map_rec16_alloc(m, f->n));
  const bool uses_rec16 = f->maybe_uninit && m->desc.rec16 && f->n >= tdr_cfg().rec16_min;
  if (uses_rec16) TTRY(map_rec16_begin(m, f->stream));
  TTRY(tdr_score_ctx_set_polar_factors(f->score_ctx, m->fac.p, nb, nr));
  TTRY(tdr_k_score_polar_ctx(&m->desc, m->tab.p, pk, nb, nr, res, &f->fp, f->st.p, f->cap, n, f->n, perm, f->uniform_scale,
                             f->maybe_uninit ? 1 : 0, f->raw_w.p, f->ws.p, f->score_ctx, f->stream));
  if (uses_rec16) TTRY(map_rec16_end(m, f->stream));
  if (renderer && !scan_imgs) TTRY(renderer_note_read(renderer, f->stream));
  // the search initialises every un-gated particle; only gated ones (state_particle.cpp:163-176) can stay un-initialised
  if (f->maybe_uninit && !(f->fp.force_on_map || f->fp.fixed_scale < 0)) f->maybe_uninit = false;
  return TDR_OK;
}
// statistics are done: running sum, resample, gather, bookkeeping (particle_filter.cpp:151-188)
static int filter_resample(tdr_filter* f, int64_t n_target) {
  const int64_t n = f->n, nl = f->nl();
  int64_t n_new = n;
  if (n_target >= 0) n_new = std::max<int64_t>(1, std::min<int64_t>(n_target, f->n_max));
  n_new = std::max<int64_t>(f->world, n_new - n_new % f->world);   // whole shards
  const int64_t nl_new = n_new / f->world, i0 = (int64_t)f->rank * nl_new;
  TTRY(f->ml_dev.resize(12));
  TTRY(tdr_k_prefix(f->w.p, n, f->runmax.p, f->pfx_ws.p, f->stream));
  // :172-173 (every rank owns an identically seeded generator); each rank draws its own slice [i0, i0 + nl_new) of the new
  // set, idx holds GLOBAL source indices
  const float* shift_dev = nullptr;
  float shift = 0.f;
  if (rng_on_device(f)) TTRY(tdr_rng_pipe_uniform(f->pipe, &shift_dev, f->stream));   // the stream is on the device: so is the draw
  else shift = tdr_rng_uniform_host(f->rng);
  if (f->comm) {
    if (shift_dev) TTRY(tdr_k_resample_dev(f->runmax.p, n, n_new, shift_dev, i0, i0 + nl_new, f->idx.p, f->stream));
    else TTRY(tdr_k_resample(f->runmax.p, n, n_new, shift, i0, i0 + nl_new, f->idx.p, f->stream));
    // the second all-gather: the pre-resample state planes, [rank][7][nl] (28 B x N)
    for (int k = 0; k < TDR_ST_FIELDS; k++)
      HTRY(hipMemcpyAsync(f->st_send.p + (size_t)k * nl, f->st.p + (size_t)k * f->cap, (size_t)nl * sizeof(float),
                          hipMemcpyDeviceToDevice, f->stream));
    TTRY(tdr_comm_all_gather(f->comm, f->st_send.p, f->st_all.p, (size_t)TDR_ST_FIELDS * nl * sizeof(float), f->stream));
    TTRY(tdr_k_gather_states(f->st_all.p, 0, nl, f->idx.p, nl_new, f->st_new.p, f->cap, f->stream));
    TTRY(tdr_k_save_ml_state(f->info.p, f->st_all.p, 0, nl, n, f->ml_dev.p, f->stream));
  } else {
    // index, state rows and max_likelihood_particle_ = particles_[argmax] (:145-147, that particle's pre-resample state,
    // kept on the device: the update returns without waiting for the GPU) in one launch
    TTRY(tdr_k_resample_gather(f->runmax.p, n, n_new, shift_dev, shift, 0, n_new, f->idx.p, f->st.p, f->cap, 0, f->st_new.p,
                               f->cap, f->info.p, f->ml_dev.p, f->stream));
  }
  f->have_ml = true;
  f->states_changed();
  std::swap(f->st.p, f->st_new.p);  // :187
  f->n = n_new;
  f->step++;
  return TDR_OK;
}
// The current particle set of ALL ranks as a plain SoA (pose statistics, the mixture fit): the filter's own arrays when
// it is not sharded, else one all-gather of the state planes.
static int filter_global_states(tdr_filter* f, const float** st, int64_t* cap) {
  if (!f->comm) {
    *st = f->st.p;
    *cap = f->cap;
    return TDR_OK;
  }
  const int64_t nl = f->nl();
  for (int k = 0; k < TDR_ST_FIELDS; k++)
    HTRY(hipMemcpyAsync(f->st_send.p + (size_t)k * nl, f->st.p + (size_t)k * f->cap, (size_t)nl * sizeof(float),
                        hipMemcpyDeviceToDevice, f->stream));
  TTRY(tdr_comm_all_gather(f->comm, f->st_send.p, f->st_all.p, (size_t)TDR_ST_FIELDS * nl * sizeof(float), f->stream));
  TTRY(tdr_k_unshard_states(f->st_all.p, f->world, nl, f->st_glob.p, f->n_max, f->stream));
  *st = f->st_glob.p;
  *cap = f->n_max;
  return TDR_OK;
}

int tdr_filter_get_weights(tdr_filter* f, float* out, int64_t n) {
  if (!f || !out || n < 0 || n > f->n_max) return failh(TDR_ERR_ARG, "filter_get_weights: bad arguments");
  HTRY(hipMemcpy(out, f->w.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return TDR_OK;
}
int tdr_filter_get_resample_indices(tdr_filter* f, int32_t* out, int64_t n) {
  if (!f || !out || n < 0 || n > f->nl()) return failh(TDR_ERR_ARG, "filter_get_resample_indices: bad arguments");
  HTRY(hipMemcpy(out, f->idx.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return TDR_OK;
}

// meanLikelihood + computeMeanCov (particle_filter.cpp:191-220); about_max != 0: maxLikelihood + computeCov (:222-236)
int tdr_filter_mean_cov(tdr_filter* f, int about_max, float state[4], float cov[16]) {
  if (!f) return failh(TDR_ERR_ARG, "filter_mean_cov: null filter");
  if (cov) std::memset(cov, 0, 16 * sizeof(float));
  if (state) std::memset(state, 0, 4 * sizeof(float));
  if (f->n < 1) return TDR_OK;  // :207-209
  float out[24];
  const float* gst = nullptr;
  int64_t gcap = 0;
  // (a sharded filter's ranks make the same calls in the same order, so the cache is valid on all of them or on none:
  // the all-gather inside filter_global_states stays collective)
  if (about_max || !f->mean_cov_valid) TTRY(filter_global_states(f, &gst, &gcap));
  if (!about_max) {
    if (!f->mean_cov_valid) {
      TTRY(tdr_k_mean_cov(gst, gcap, f->n, nullptr, f->stats.p, f->stream));
      HTRY(hipMemcpy(f->mean_cov_host, f->stats.p, sizeof(out), hipMemcpyDeviceToHost));
      f->mean_cov_valid = true;
    }
    std::memcpy(out, f->mean_cov_host, sizeof(out));
    if (state) std::memcpy(state, out, 4 * sizeof(float));
  } else {
    float ref[4] = {0, 0, 0, 0};
    if (!f->have_ml) return failh(TDR_ERR_ARG, "filter_mean_cov: no update yet, there is no max-likelihood particle");
    TTRY(tdr_k_mean_cov(gst, gcap, f->n, f->ml_dev.p + 8, f->stats.p, f->stream));
    HTRY(hipMemcpyAsync(out, f->stats.p, sizeof(out), hipMemcpyDeviceToHost, f->stream));
    HTRY(hipMemcpyAsync(ref, f->ml_dev.p + 8, sizeof(ref), hipMemcpyDeviceToHost, f->stream));
    HTRY(hipStreamSynchronize(f->stream));
    if (state) std::memcpy(state, ref, sizeof(ref));
  }
  if (cov) std::memcpy(cov, out + 4, 16 * sizeof(float));
  return TDR_OK;
}

// freezeScale (particle_filter.cpp:343-357)
int tdr_filter_freeze_scale(tdr_filter* f) {
  if (!f) return failh(TDR_ERR_ARG, "filter_freeze_scale: null filter");
  if (f->scale_frozen || f->n < 1) return TDR_OK;
  const float* gst = nullptr;
  int64_t gcap = 0;
  TTRY(filter_global_states(f, &gst, &gcap));
  TTRY(tdr_k_mean_cov(gst, gcap, f->n, nullptr, f->stats.p, f->stream));
  f->states_changed();
  TTRY(tdr_k_set_scale(f->st.p, f->cap, f->nl(), f->stats.p + 20, f->stream));
  float gm = 0;
  HTRY(hipMemcpy(&gm, f->stats.p + 20, sizeof(float), hipMemcpyDeviceToHost));
  f->scale_frozen = true;
  f->uniform_scale = gm;
  return TDR_OK;
}
int tdr_filter_is_scale_frozen(const tdr_filter* f) { return f && f->scale_frozen; }
// scale() (particle_filter.cpp:359-367)
float tdr_filter_scale(tdr_filter* f) {
  if (!f) return -1.f;
  if (f->fp.fixed_scale > 0) return f->fp.fixed_scale;
  if (f->scale_frozen && f->n > 0) {
    if (f->scale_valid) return f->scale_host;
    float s = -1.f;
    if (hipMemcpy(&s, f->st.p + (size_t)TDR_ST_SCALE * f->cap, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
    return s;
  }
  return -1.f;
}
int64_t tdr_filter_num_particles(const tdr_filter* f) { return f ? f->n : 0; }

// computeGMM (particle_filter.cpp:252-318): <= 1000 strided samples {x, y, 50 cos theta, 50 sin theta} -> mixture
int tdr_filter_compute_gmm(tdr_filter* f) {
  if (!f) return failh(TDR_ERR_ARG, "filter_compute_gmm: null filter");
  if (f->n < 1) return TDR_OK;
  const int num = (int)std::min<int64_t>(1000, f->n);   // :262
  TTRY(f->gmm_samples.resize((size_t)3 * num));
  const float* gst = nullptr;
  int64_t gcap = 0;
  TTRY(filter_global_states(f, &gst, &gcap));
  TTRY(tdr_k_sample_ml_states(gst, gcap, f->n, num, f->gmm_samples.p, f->stream));
  std::vector<float> h((size_t)3 * num);
  HTRY(hipMemcpyAsync(h.data(), f->gmm_samples.p, h.size() * sizeof(float), hipMemcpyDeviceToHost, f->stream));
  HTRY(hipStreamSynchronize(f->stream));
  std::vector<double> x((size_t)4 * num);
  for (int i = 0; i < num; i++) {
    x[4 * i + 0] = h[3 * i + 0];
    x[4 * i + 1] = h[3 * i + 1];
    x[4 * i + 2] = 50 * std::cos(h[3 * i + 2]);   // :269-270 (float argument: the float overload)
    x[4 * i + 3] = 50 * std::sin(h[3 * i + 2]);
  }
  int k = f->num_gaussians;
  std::vector<float> means((size_t)3 * TDR_GMM_MAX_K), covs((size_t)9 * TDR_GMM_MAX_K);
  TTRY(tdr_gmm_select_host(x.data(), num, f->n, &k, TDR_GMM_MAX_K, means.data(), covs.data()));
  f->num_gaussians = k;
  f->gmm_means.assign(means.begin(), means.begin() + 3 * k);
  f->gmm_covs.assign(covs.begin(), covs.begin() + 9 * k);
  return TDR_OK;
}
int tdr_filter_get_gmm(tdr_filter* f, int max_k, int* k_out, float* means, float* covs) {
  if (!f || !k_out) return failh(TDR_ERR_ARG, "filter_get_gmm: bad arguments");
  const int k = (int)(f->gmm_means.size() / 3);
  *k_out = k;
  if (k > max_k) return failh(TDR_ERR_ARG, "filter_get_gmm: %d clusters, room for %d", k, max_k);
  if (means && k) std::memcpy(means, f->gmm_means.data(), f->gmm_means.size() * sizeof(float));
  if (covs && k) std::memcpy(covs, f->gmm_covs.data(), f->gmm_covs.size() * sizeof(float));
  return TDR_OK;
}
int64_t tdr_filter_step_count(const tdr_filter* f) { return f ? (int64_t)f->step : -1; }
int tdr_filter_num_gaussians(const tdr_filter* f) { return f ? f->num_gaussians : 0; }
int tdr_filter_set_num_gaussians(tdr_filter* f, int num_gaussians) {
  if (!f || num_gaussians < 1 || num_gaussians > TDR_GMM_MAX_K)
    return failh(TDR_ERR_ARG, "filter_set_num_gaussians: bad arguments (1 .. %d)", TDR_GMM_MAX_K);
  f->num_gaussians = num_gaussians;
  return TDR_OK;
}
int64_t tdr_filter_adaptive_count(tdr_filter* f) {
  if (!f) return -1;
  const int k = (int)(f->gmm_means.size() / 3);
  if (k == 0) return f->n;
  return tdr_adaptive_count_host(f->gmm_covs.data(), k, f->n, f->n_max);
}

// ---- the particle picture (include/tdr.h, "the particle picture"; kernels in tdr_viz.hip) ---------------------------------
int tdr_filter_set_viz_background(tdr_filter* f, const uint8_t* bgr_host, int H, int W) {
  if (!f || !bgr_host) return failh(TDR_ERR_ARG, "filter_set_viz_background: null argument");
  if (H < 11 || W < 11 || H > 32768 || W > 32768)
    return failh(TDR_ERR_ARG, "filter_set_viz_background: a %d x %d image (11 .. 32768 a side)", H, W);
  const size_t bytes = (size_t)3 * H * W;
  TTRY(f->viz_bg.resize(bytes));
  TTRY(f->viz_planes.resize(4 * tdr_viz_plane_words(H, W)));
  HTRY(hipStreamSynchronize(f->stream));   // (an earlier picture may still read the old background)
  HTRY(hipMemcpy(f->viz_bg.p, bgr_host, bytes, hipMemcpyHostToDevice));
  f->viz_h = H;
  f->viz_w = W;
  return TDR_OK;
}

// (int)((float)dim * s) as the node computes it (src/top_down_render.cpp:442-444), x86's conversion
static int viz_pub_dim(int dim, float s) {
  const float v = (float)dim * s;
  return (v >= -2147483648.f && v < 2147483648.f) ? (int)v : std::numeric_limits<int>::min();
}

int tdr_filter_visualize(tdr_filter* f, float pub_scale, const int32_t* extra_arrows, int m, uint8_t* out_bgr_host,
                         int64_t capacity, int* out_h, int* out_w) {
  if (!f || !out_h || !out_w || m < 0 || (m > 0 && !extra_arrows) || m > (1 << 20))
    return failh(TDR_ERR_ARG, "filter_visualize: bad arguments");
  if (f->comm) return failh(TDR_ERR_ARG, "filter_visualize: a sharded filter has no picture (draw from a one-GPU filter)");
  if (f->viz_h < 1) return failh(TDR_ERR_ARG, "filter_visualize: no background (tdr_filter_set_viz_background)");
  const int H = f->viz_h, W = f->viz_w;
  const int oh = viz_pub_dim(H, pub_scale), ow = viz_pub_dim(W, pub_scale);
  if (oh < 1 || ow < 1 || oh > 32768 || ow > 32768)
    return failh(TDR_ERR_ARG, "filter_visualize: scale %g publishes %d x %d pixels (1 .. 32768 a side)", (double)pub_scale, oh, ow);
  *out_h = oh;
  *out_w = ow;
  if (!out_bgr_host) return TDR_OK;
  const size_t bytes = (size_t)3 * oh * ow;
  if (capacity < 0 || (size_t)capacity < bytes)
    return failh(TDR_ERR_ARG, "filter_visualize: the image needs %zu bytes, room for %lld", bytes, (long long)capacity);
  // layers 4 and 5 on the host: a few hundred integers
  float best[4];
  if (f->have_ml) HTRY(hipMemcpy(best, f->ml_dev.p + 8, sizeof(best), hipMemcpyDeviceToHost));
  const int k = (int)(f->gmm_means.size() / 3);
  std::vector<int32_t> segs((size_t)5 * TDR_VIZ_MAX_SEGS(k, m));
  int nseg = 0;
  TTRY(tdr_viz_overlay_host(f->gmm_means.data(), f->gmm_covs.data(), k, f->have_ml ? best : nullptr, extra_arrows, m, H,
                            segs.data(), TDR_VIZ_MAX_SEGS(k, m), &nseg));
  TTRY(f->viz_segs.resize((size_t)5 * std::max(nseg, 1)));
  TTRY(f->viz_out.resize(bytes));
  const size_t pw = tdr_viz_plane_words(H, W);
  hipStream_t s = f->stream;
  if (nseg) HTRY(hipMemcpyAsync(f->viz_segs.p, segs.data(), (size_t)5 * nseg * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HTRY(hipMemsetAsync(f->viz_planes.p, 0, 4 * pw * sizeof(uint32_t), s));
  TTRY(tdr_k_viz_particles(f->st.p, f->cap, f->n, H, W, f->viz_planes.p, s));
  TTRY(tdr_k_viz_segments(f->viz_segs.p, nseg, H, W, f->viz_planes.p, s));
  TTRY(tdr_k_viz_compose(f->viz_bg.p, H, W, f->viz_planes.p, oh, ow, f->viz_out.p, s));
  HTRY(hipMemcpyAsync(out_bgr_host, f->viz_out.p, bytes, hipMemcpyDeviceToHost, s));
  HTRY(hipStreamSynchronize(s));
  return TDR_OK;
}

// ParticleFilter::updateMap(const cv::Mat& map, map_center) (particle_filter.cpp:320-341) for a class-index image
int tdr_filter_update_map_labels(tdr_filter* f, const uint8_t* label_img, int img_h, int img_w,
                                 const int32_t* flatten_lut, int lut_size, int ncls, float resolution, int center_x,
                                 int center_y) {
  if (!f || !f->map) return failh(TDR_ERR_ARG, "filter_update_map_labels: null filter");
  const int ox = f->map->center_x, oy = f->map->center_y;
  TTRY(tdr_map_set_labels(f->map, label_img, img_h, img_w, flatten_lut, lut_size, ncls, resolution, center_x, center_y));
  f->states_changed();
  if (f->n > 0) return tdr_k_shift_init(f->st.p, f->cap, f->nl(), (float)(center_x - ox), (float)(center_y - oy), f->stream);
  if (f->map->have_map) return tdr_filter_initialize_particles(f);  // :337-340
  return TDR_OK;
}

// tdr_filter_update_map_labels through the incremental map update (tdr_map_update_labels_incremental)
int tdr_filter_update_map_labels_incremental(tdr_filter* f, const uint8_t* label_img, int img_h, int img_w,
                                             const int32_t* flatten_lut, int lut_size, int ncls, float resolution,
                                             int center_x, int center_y, int64_t* changed_cells) {
  if (!f || !f->map) return failh(TDR_ERR_ARG, "filter_update_map_labels_incremental: null filter");
  const int ox = f->map->center_x, oy = f->map->center_y;
  TTRY(tdr_map_update_labels_incremental(f->map, label_img, img_h, img_w, flatten_lut, lut_size, ncls, resolution, center_x,
                                         center_y, changed_cells));
  f->states_changed();
  if (f->n > 0) return tdr_k_shift_init(f->st.p, f->cap, f->nl(), (float)(center_x - ox), (float)(center_y - oy), f->stream);
  if (f->map->have_map) return tdr_filter_initialize_particles(f);  // :337-340
  return TDR_OK;
}
// ... and through tdr_map_patch_labels
int tdr_filter_patch_map_labels(tdr_filter* f, const uint8_t* patch, int y0, int x0, int h, int w, int center_x,
                                int center_y, int64_t* changed_cells) {
  if (!f || !f->map) return failh(TDR_ERR_ARG, "filter_patch_map_labels: null filter");
  const int ox = f->map->center_x, oy = f->map->center_y;
  TTRY(tdr_map_patch_labels(f->map, patch, y0, x0, h, w, center_x, center_y, changed_cells));
  f->states_changed();
  if (f->n > 0) return tdr_k_shift_init(f->st.p, f->cap, f->nl(), (float)(center_x - ox), (float)(center_y - oy), f->stream);
  if (f->map->have_map) return tdr_filter_initialize_particles(f);  // :337-340
  return TDR_OK;
}

// ParticleFilter::updateMap (particle_filter.cpp:320-341), with the map already in distance-map form
int tdr_filter_update_map(tdr_filter* f, const float* class_maps, const uint8_t* class_mask, int ncls, int rows, int cols,
                          float resolution, int center_x, int center_y) {
  if (!f || !f->map) return failh(TDR_ERR_ARG, "filter_update_map: null filter");
  const int ox = f->map->center_x, oy = f->map->center_y;
  TTRY(tdr_map_set(f->map, class_maps, class_mask, ncls, rows, cols, resolution, center_x, center_y));
  f->states_changed();
  if (f->n > 0) return tdr_k_shift_init(f->st.p, f->cap, f->nl(), (float)(center_x - ox), (float)(center_y - oy), f->stream);
  return tdr_filter_initialize_particles(f);  // :337-340
}


// ---- batched filters (tdr_batch_step): many filters on one map, one launch per stage -------------------------------------
// Each filter keeps what is its own: its generator pipe draws its normals and its uniform (per-filter mt19937 streams) and
// its scan is packed into its own buffer.  The stages of the step are then one launch each over a table of the filters:
// propagate and resample (csrc/tdr_batch.hip), the float scoring launch (tdr_score.hip), the statistics and the running
// sum (tdr_prefix.hip).  The locality order is left out: it never changes results (tdr.h).
namespace {
thread_local int g_batch_stats[2] = {0, 0};   // filters of this thread's last batch: batched, standalone
struct BatchCtx {   // per thread: the tables, staged in pinned host memory and copied to the device, reused from call to call
  char* host = nullptr;
  DevBuf<char> dev;
  size_t cap = 0;
  hipEvent_t uploaded = nullptr;   // the last call's copy has read `host`
  hipEvent_t done = nullptr;       // the last call's kernels have read `dev`
  ~BatchCtx() {
    if (uploaded) { (void)hipEventSynchronize(uploaded); (void)hipEventDestroy(uploaded); }
    if (done) { (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
    if (host) (void)hipHostFree(host);
  }
};
thread_local BatchCtx g_batch;
}  // namespace

extern "C" {
int tdr_batch_last_stats(int* batched, int* standalone) {
  if (batched) *batched = g_batch_stats[0];
  if (standalone) *standalone = g_batch_stats[1];
  return TDR_OK;
}

static bool batch_eligible(const tdr_filter* f) {
  const tdr_map* m = f->map;
  // (a filter that may hold a particle without a heading: only with tdr_config_tuning("batch_init_search"))
  const bool uninit_ok = !f->maybe_uninit || tdr_cfg().batch_init_search == 1;
  return !f->comm && rng_device_capable(f) && uninit_ok && f->n >= 1 && f->n <= 32768 &&
         tdr_score_polar_float_form(&m->desc, m->nb, m->nr, f->n, f->n);
}

int tdr_batch_step(tdr_filter* const* filters, int k, const tdr_batch_input* in, void* stream) {
  g_batch_stats[0] = g_batch_stats[1] = 0;
  if (k < 1) return failh(TDR_ERR_ARG, "batch_step: k = %d, at least one filter is needed", k);
  if (!filters || !in) return failh(TDR_ERR_ARG, "batch_step: null %s array", !filters ? "filter" : "input");
  for (int i = 0; i < k; i++)
    if (!filters[i]) return failh(TDR_ERR_ARG, "batch_step: filter %d is null", i);
  {
    std::vector<const tdr_filter*> seen(filters, filters + k);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return failh(TDR_ERR_ARG, "batch_step: a filter appears twice in the batch");
  }
  tdr_map* m = filters[0]->map;
  for (int i = 0; i < k; i++)
    if (filters[i]->map != m) return failh(TDR_ERR_ARG, "batch_step: filter %d is on another map than filter 0", i);
  for (int i = 0; i < k; i++)
    if (filters[i]->cart) return failh(TDR_ERR_ARG, "batch_step: filter %d is a Cartesian filter (batches are polar)", i);
  if (!m || !m->have_map) return failh(TDR_ERR_ARG, "batch_step: the filters' map holds no map");
  if (m->nb < 1 || !m->tab.p) return failh(TDR_ERR_ARG, "batch_step: samplePtsPolar was never called on the map");
  const int ncls = m->desc.ncls, nb = m->nb, nr = m->nr;
  for (int i = 0; i < k; i++) {
    const tdr_renderer* r = in[i].renderer;
    if (!in[i].scan_imgs && !r) return failh(TDR_ERR_ARG, "batch_step: input %d has no scan", i);
    if (!in[i].scan_imgs && !r->have_scan) return failh(TDR_ERR_ARG, "batch_step: input %d: the renderer has no render", i);
    if (!in[i].scan_imgs && (r->ncls != ncls || r->rows != nb || r->cols != nr))
      return failh(TDR_ERR_ARG, "batch_step: input %d: render shape %dx%dx%d does not match the map's %dx%dx%d", i, r->ncls,
                   r->rows, r->cols, ncls, nb, nr);
  }
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> fast;
  for (int i = 0; i < k; i++) {
    tdr_filter* f = filters[i];
    if (batch_eligible(f)) { fast.push_back(i); continue; }
    TTRY(tdr_filter_propagate(f, in[i].tx, in[i].ty, in[i].omega));
    TTRY(tdr_filter_update(f, in[i].scan_imgs, in[i].renderer, in[i].res, in[i].n_target));
    g_batch_stats[1]++;
  }
  const int kf = (int)fast.size();
  if (kf == 0) return TDR_OK;

  BatchCtx& B = g_batch;
  // the batched filters whose 40-rotation search is part of the scoring stage; the largest decides about the map's scratch
  int k_init = 0;
  bool uses_rec16 = false;
  for (int j = 0; j < kf; j++) {
    const tdr_filter* f = filters[fast[j]];
    if (!f->maybe_uninit) continue;
    k_init++;
    TTRY(map_rec16_alloc(m, f->n));
    uses_rec16 |= m->desc.rec16 && f->n >= tdr_cfg().rec16_min;
  }
  // one staging area: [kf] TdrBatchEntry, then the scoring launch's tables (tdr_batch_score_stage_bytes)
  const size_t ent_bytes = (sizeof(TdrBatchEntry) * (size_t)kf + 63) / 64 * 64;
  const size_t stage = ent_bytes + tdr_batch_score_stage_bytes(kf, k_init);
  if (!B.uploaded) HTRY(hipEventCreateWithFlags(&B.uploaded, hipEventDisableTiming));
  if (!B.done) HTRY(hipEventCreateWithFlags(&B.done, hipEventDisableTiming));
  HTRY(hipEventSynchronize(B.uploaded));   // (the previous call's copy has left the pinned buffer)
  if (B.cap < stage) {
    HTRY(hipEventSynchronize(B.done));     // (and its kernels the device buffer that is replaced)
    if (B.host) HTRY(hipHostFree(B.host));
    B.host = nullptr;
    B.cap = 0;
    HTRY(hipHostMalloc((void**)&B.host, stage));
    B.cap = stage;
  }
  TTRY(B.dev.resize(stage));
  TdrBatchEntry* const tab = reinterpret_cast<TdrBatchEntry*>(B.host);
  TdrBatchEntry* const tab_dev = reinterpret_cast<TdrBatchEntry*>(B.dev.p);

  // the batch stream continues after the batched renders it reads, everything already queued on the filters' own
  // streams, and after the previous batch's kernels have read the device tables this call overwrites
  for (int j = 0; j < kf; j++)
    if (!in[fast[j]].scan_imgs) TTRY(renderer_wait_render(in[fast[j]].renderer, s));
  std::vector<hipEvent_t> evs((size_t)kf, nullptr);
  auto destroy_events = [&]() { for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e); };
  int rc = TDR_OK;
  if (hipStreamWaitEvent(s, B.done, 0) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_step: stream wait");
  for (int j = 0; j < kf && rc == TDR_OK; j++) {
    tdr_filter* f = filters[fast[j]];
    rc = rng_to_device(f);
    if (rc == TDR_OK && hipEventCreateWithFlags(&evs[j], hipEventDisableTiming) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_step: event");
    if (rc == TDR_OK && hipEventRecord(evs[j], f->stream) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_step: event record");
    if (rc == TDR_OK && hipStreamWaitEvent(s, evs[j], 0) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_step: stream wait");
  }
  if (rc != TDR_OK) { destroy_events(); return rc; }

  // per filter: its generator's normals and uniform (the pipe orders its own side stream against `s`; the draws keep the
  // standalone order), its scan packed into its own buffer, and its table entries
  const size_t P = (size_t)nb * nr, pk_floats = P * tdr_rec_floats(ncls);
  std::vector<TdrBatchScoreIn> sin((size_t)kf);
  int blocks_prop = 0, blocks_res = 0;
  int64_t n_big = 1;
  for (int j = 0; j < kf && rc == TDR_OK; j++) {
    tdr_filter* f = filters[fast[j]];
    const tdr_batch_input& x = in[fast[j]];
    TdrBatchEntry& e = tab[j];
    e = TdrBatchEntry{};
    f->states_changed();
    f->fp.num_classes = ncls;
    rc = tdr_rng_pipe_normals(f->pipe, f->n, 0, f->n, f->scale_frozen ? 1 : 0, &e.z4, s);
    f->prop_calls++;
    if (rc == TDR_OK) rc = tdr_rng_pipe_uniform(f->pipe, &e.shift, s);
    if (rc == TDR_OK) rc = f->ml_dev.resize(12);
    const float* pk = nullptr;
    if (rc == TDR_OK && x.scan_imgs) {
      rc = f->scan_img.resize(P * ncls);
      if (rc == TDR_OK) rc = f->scan_pk.resize(pk_floats);
      if (rc == TDR_OK && hipMemcpyAsync(f->scan_img.p, x.scan_imgs, P * ncls * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess)
        rc = failh(TDR_ERR_HIP, "batch_step: scan upload");
      if (rc == TDR_OK) rc = tdr_k_pack_scan(f->scan_img.p, ncls, nb, nr, f->scan_pk.p, s);
      pk = f->scan_pk.p;
    } else {
      pk = x.renderer->pk.p;
    }
    if (rc == TDR_OK) rc = f->ws.resize(tdr_score_workspace_floats(ncls, nb, nr, f->n, f->n));
    int64_t n_new = f->n;
    if (x.n_target >= 0) n_new = std::max<int64_t>(1, std::min<int64_t>(x.n_target, f->n_max));
    e.st = f->st.p; e.st_new = f->st_new.p; e.last_dist = f->last_dist.p; e.cap = f->cap; e.n = f->n; e.n_new = n_new;
    e.tx = x.tx; e.ty = x.ty; e.omega = x.omega; e.pos_cov = f->fp.pos_cov; e.theta_cov = f->fp.theta_cov;
    e.scale_freeze = f->scale_frozen ? 1 : 0;
    e.raw_w = f->raw_w.p; e.w_out = f->w.p; e.info_out = f->info.p; e.runmax_out = f->runmax.p;
    e.runmax = f->runmax.p; e.info = f->info.p; e.idx = f->idx.p; e.ml = f->ml_dev.p;
    e.blk_prop = blocks_prop;
    blocks_prop += (int)((f->n + TDR_BATCH_THREADS - 1) / TDR_BATCH_THREADS);
    e.blk_res = blocks_res;
    blocks_res += (int)((n_new + TDR_BATCH_THREADS - 1) / TDR_BATCH_THREADS);
    n_big = std::max(n_big, f->n);
    sin[j] = TdrBatchScoreIn{pk, x.res, &f->fp, f->st.p, f->cap, f->n, f->uniform_scale, f->raw_w.p, f->ws.p,
                             f->maybe_uninit ? 1 : 0};
  }
  if (rc == TDR_OK) rc = tdr_batch_score_build(&m->desc, m->tab.p, nb, nr, kf, sin.data(), B.host + ent_bytes);
  if (rc == TDR_OK && hipMemcpyAsync(B.dev.p, B.host, stage, hipMemcpyHostToDevice, s) != hipSuccess)
    rc = failh(TDR_ERR_HIP, "batch_step: table upload");
  if (rc == TDR_OK && hipEventRecord(B.uploaded, s) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_step: event record");
  // one launch per stage over the whole batch (the scoring launch: utab, score, finalize)
  if (rc == TDR_OK) rc = tdr_batch_propagate(tab_dev, kf, blocks_prop, s);
  if (rc == TDR_OK && uses_rec16) rc = map_rec16_begin(m, s);
  if (rc == TDR_OK) rc = tdr_batch_score_launch(&m->desc, m->tab.p, nb, nr, kf, B.host + ent_bytes, B.dev.p + ent_bytes, s);
  if (rc == TDR_OK && uses_rec16) rc = map_rec16_end(m, s);
  if (rc == TDR_OK) rc = tdr_batch_update_weights(tab_dev, kf, n_big, s);
  if (rc == TDR_OK) rc = tdr_batch_prefix(tab_dev, kf, n_big, s);
  if (rc == TDR_OK) rc = tdr_batch_resample(tab_dev, kf, blocks_res, s);
  if (rc == TDR_OK && hipEventRecord(B.done, s) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_step: event record");
  for (int j = 0; j < kf && rc == TDR_OK; j++)
    if (!in[fast[j]].scan_imgs) rc = renderer_note_read(in[fast[j]].renderer, s);
  if (rc != TDR_OK) { destroy_events(); return rc; }
  for (int j = 0; j < kf; j++) {
    tdr_filter* f = filters[fast[j]];
    f->have_ml = true;
    f->states_changed();
    // the search initialises every un-gated particle; only gated ones can stay un-initialised (filter_score)
    if (f->maybe_uninit && !(f->fp.force_on_map || f->fp.fixed_scale < 0)) f->maybe_uninit = false;
    std::swap(f->st.p, f->st_new.p);   // particle_filter.cpp:187
    f->n = tab[j].n_new;
    f->step++;
  }
  // the filters' own streams continue after the batch
  for (int j = 0; j < kf && rc == TDR_OK; j++)
    if (hipStreamWaitEvent(filters[fast[j]]->stream, B.done, 0) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_step: stream wait");
  destroy_events();
  g_batch_stats[0] = kf;
  return rc;
}
}  // extern "C"

// ---- the two ends of a batched node loop: tdr_batch_render_polar, tdr_batch_pose (csrc/tdr_batch_loop.hip) ---------------
namespace {
struct StageCtx {   // per thread and call kind: pinned staging, its device copy, the events that order their reuse
  char* host = nullptr;
  size_t cap = 0;
  DevBuf<char> dev;
  hipEvent_t uploaded = nullptr;   // the last call's copies have read / written `host`
  hipEvent_t done = nullptr;       // the last call's kernels have read `dev`
  ~StageCtx() {
    if (uploaded) { (void)hipEventSynchronize(uploaded); (void)hipEventDestroy(uploaded); }
    if (done) { (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
    if (host) (void)hipHostFree(host);
  }
  // host >= host_bytes, dev >= dev_bytes; `s` continues after the previous call's kernels
  int reserve(size_t host_bytes, size_t dev_bytes, hipStream_t s) {
    if (!uploaded) HTRY(hipEventCreateWithFlags(&uploaded, hipEventDisableTiming));
    if (!done) HTRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    HTRY(hipEventSynchronize(uploaded));
    if (cap < host_bytes) {
      if (host) HTRY(hipHostFree(host));
      host = nullptr;
      cap = 0;
      HTRY(hipHostMalloc((void**)&host, host_bytes));
      cap = host_bytes;
    }
    if (dev.n < dev_bytes) {
      HTRY(hipEventSynchronize(done));
      TTRY(dev.resize(dev_bytes));
    }
    HTRY(hipStreamWaitEvent(s, done, 0));
    return TDR_OK;
  }
};
thread_local StageCtx g_render_stage, g_pose_stage;
size_t align64(size_t b) { return (b + 63) / 64 * 64; }
}  // namespace

extern "C" {
int tdr_batch_render_polar(tdr_renderer* const* r, int k, const tdr_batch_cloud* clouds, float ang_res, int ncls, int nb,
                           int nr, void* stream) {
  if (k < 1) return failh(TDR_ERR_ARG, "batch_render: k = %d, at least one renderer is needed", k);
  if (!r || !clouds) return failh(TDR_ERR_ARG, "batch_render: null %s array", !r ? "renderer" : "cloud");
  for (int i = 0; i < k; i++)
    if (!r[i]) return failh(TDR_ERR_ARG, "batch_render: renderer %d is null", i);
  {
    std::vector<const tdr_renderer*> seen(r, r + k);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return failh(TDR_ERR_ARG, "batch_render: a renderer appears twice in the batch");
  }
  for (int i = 0; i < k; i++) {
    const tdr_batch_cloud& c = clouds[i];
    if (c.n < 0 || (c.n > 0 && !c.pts)) return failh(TDR_ERR_ARG, "batch_render: cloud %d: null points", i);
    if (c.stride < 3 || c.ioff < 0 || c.ioff >= c.stride)
      return failh(TDR_ERR_ARG, "batch_render: cloud %d: bad point stride / offset %d / %d", i, c.stride, c.ioff);
    if (!(c.res > 0.f)) return failh(TDR_ERR_ARG, "batch_render: cloud %d: resolution must be > 0", i);
  }
  if (!(ang_res > 0.f)) return failh(TDR_ERR_ARG, "batch_render: angular resolution must be > 0");
  if (ncls < 1 || ncls > TDR_MAX_CLASSES || nb < 1 || nr < 1)
    return failh(TDR_ERR_ARG, "batch_render: bad image shape %dx%dx%d", ncls, nb, nr);
  if ((int64_t)ncls * nb * 4 > 152 * 1024) return failh(TDR_ERR_ARG, "batch_render: ncls*rows too large for one LDS tile (152 KB)");
  TdrBatchRasterShape shape{};
  const bool keyed = tdr_batch_raster_shape(ncls, nb, nr, ang_res, &shape);
  hipStream_t s = (hipStream_t)stream;

  // one staging area: [k] entries, then every cloud's points (64-byte aligned); on the device, the keys follow
  const size_t ent_bytes = align64(sizeof(TdrBatchRasterEntry) * (size_t)k);
  std::vector<size_t> pts_off((size_t)k), key_off((size_t)k);
  size_t stage = ent_bytes;
  for (int i = 0; i < k; i++) {
    pts_off[i] = stage;
    stage += align64((size_t)clouds[i].n * clouds[i].stride * sizeof(float));
  }
  size_t dev_bytes = stage;
  for (int i = 0; i < k; i++) {
    key_off[i] = dev_bytes;
    dev_bytes += align64((size_t)clouds[i].n * sizeof(uint32_t));
  }
  StageCtx& B = g_render_stage;
  TTRY(B.reserve(stage, std::max<size_t>(dev_bytes, 64), s));
  const size_t P = (size_t)nb * nr, rf = (size_t)tdr_rec_floats(ncls);
  for (int i = 0; i < k; i++) {
    tdr_renderer* q = r[i];
    TTRY(q->img.resize(P * ncls));
    TTRY(q->pk.resize(P * rf));
    // img / pk are rewritten: after their readers and the renderer's previous batched render
    for (size_t j = 0; j < q->n_readers; j++) HTRY(hipStreamWaitEvent(s, q->readers[j].second, 0));
    TTRY(renderer_wait_render(q, s));
    if (!q->rendered) HTRY(hipEventCreateWithFlags(&q->rendered, hipEventDisableTiming));
  }
  TdrBatchRasterEntry* tab = reinterpret_cast<TdrBatchRasterEntry*>(B.host);
  int blocks_keys = 0;
  for (int i = 0; i < k; i++) {
    const tdr_batch_cloud& c = clouds[i];
    if (c.n > 0) std::memcpy(B.host + pts_off[i], c.pts, (size_t)c.n * c.stride * sizeof(float));
    TdrBatchRasterEntry& e = tab[i];
    e = TdrBatchRasterEntry{};
    e.pts = reinterpret_cast<const float*>(B.dev.p + pts_off[i]);
    e.lut = r[i]->lut.p;
    e.keys = reinterpret_cast<uint32_t*>(B.dev.p + key_off[i]);
    e.img = r[i]->img.p;
    e.pk = r[i]->pk.p;
    e.n = c.n;
    e.res = c.res;
    e.stride = c.stride;
    e.ioff = c.ioff;
    e.blk_keys = blocks_keys;
    blocks_keys += (int)((c.n + 255) / 256);
  }
  HTRY(hipMemcpyAsync(B.dev.p, B.host, stage, hipMemcpyHostToDevice, s));
  HTRY(hipEventRecord(B.uploaded, s));
  if (keyed) {
    TTRY(tdr_batch_raster(reinterpret_cast<const TdrBatchRasterEntry*>(B.dev.p), k, blocks_keys, shape, s));
  } else {   // shapes the standalone raster scores without keys: its own launch per renderer
    for (int i = 0; i < k; i++)
      TTRY(tdr_k_raster_polar(tab[i].pts, clouds[i].stride, clouds[i].ioff, clouds[i].n, clouds[i].res, ang_res, r[i]->lut.p,
                              ncls, nb, nr, r[i]->img.p, r[i]->pk.p, tab[i].keys, s));
  }
  HTRY(hipEventRecord(B.done, s));
  for (int i = 0; i < k; i++) {
    tdr_renderer* q = r[i];
    HTRY(hipEventRecord(q->rendered, s));
    q->render_async = true;
    q->n_readers = 0;
    q->ncls = ncls;
    q->rows = nb;
    q->cols = nr;
    q->polar = true;
    q->have_scan = true;
  }
  return TDR_OK;
}

int tdr_renderer_get_render(const tdr_renderer* r, float* imgs_out, float* pk_out) {
  if (!r) return failh(TDR_ERR_ARG, "renderer_get_render: null renderer");
  if (!r->have_scan) return failh(TDR_ERR_ARG, "renderer_get_render: the renderer has no render");
  const size_t P = (size_t)r->rows * r->cols;
  if (r->render_async) HTRY(hipEventSynchronize(r->rendered));
  if (imgs_out) HTRY(hipMemcpy(imgs_out, r->img.p, P * r->ncls * sizeof(float), hipMemcpyDeviceToHost));
  if (pk_out) HTRY(hipMemcpy(pk_out, r->pk.p, P * tdr_rec_floats(r->ncls) * sizeof(float), hipMemcpyDeviceToHost));
  return TDR_OK;
}

int tdr_batch_pose(tdr_filter* const* f, int k, tdr_pose_stats* out, void* stream) {
  if (k < 1) return failh(TDR_ERR_ARG, "batch_pose: k = %d, at least one filter is needed", k);
  if (!f || !out) return failh(TDR_ERR_ARG, "batch_pose: null %s array", !f ? "filter" : "output");
  for (int i = 0; i < k; i++)
    if (!f[i]) return failh(TDR_ERR_ARG, "batch_pose: filter %d is null", i);
  {
    std::vector<const tdr_filter*> seen(f, f + k);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return failh(TDR_ERR_ARG, "batch_pose: a filter appears twice in the batch");
  }
  for (int i = 0; i < k; i++)
    if (f[i]->map != f[0]->map) return failh(TDR_ERR_ARG, "batch_pose: filter %d is on another map than filter 0", i);
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> small, big;
  for (int i = 0; i < k; i++) {
    tdr_filter* g = f[i];
    tdr_pose_stats& o = out[i];
    o = tdr_pose_stats{};
    o.n = g->n;
    if (g->comm) {   // the all-gather inside is collective: the standalone calls
      TTRY(tdr_filter_mean_cov(g, 0, o.mean, o.cov));
      o.scale = tdr_filter_scale(g);
      continue;
    }
    if (g->n < 1) { o.scale = tdr_filter_scale(g); continue; }   // (zeros, no device work)
    (g->n <= TDR_BATCH_MC_SINGLE_MAX_N ? small : big).push_back(i);
  }
  const int ks = (int)small.size(), kb = (int)big.size(), kd = ks + kb;
  if (kd == 0) return TDR_OK;
  // staging: [kd] entries (small ones first), then the [kd] result records the kernels write and the copy brings back
  const size_t ent_bytes = align64(sizeof(TdrBatchPoseEntry) * (size_t)kd);
  const size_t res_bytes = sizeof(float) * TDR_BATCH_POSE_FLOATS * (size_t)kd;
  StageCtx& B = g_pose_stage;
  TTRY(B.reserve(ent_bytes + res_bytes, ent_bytes + res_bytes, s));
  // after every filter's last step, on whichever stream it ran (tdr_batch_step leaves the filters' streams after it)
  {
    std::vector<hipStream_t> streams;
    for (int i : small) streams.push_back(f[i]->stream);
    for (int i : big) streams.push_back(f[i]->stream);
    std::sort(streams.begin(), streams.end());
    streams.erase(std::unique(streams.begin(), streams.end()), streams.end());
    for (hipStream_t fs : streams) {
      if (fs == s) continue;
      hipEvent_t e = nullptr;
      HTRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      int rc = TDR_OK;
      if (hipEventRecord(e, fs) != hipSuccess || hipStreamWaitEvent(s, e, 0) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_pose: stream order");
      (void)hipEventDestroy(e);
      if (rc != TDR_OK) return rc;
    }
  }
  TdrBatchPoseEntry* tab = reinterpret_cast<TdrBatchPoseEntry*>(B.host);
  float* res_dev = reinterpret_cast<float*>(B.dev.p + ent_bytes);
  float* res_host = reinterpret_cast<float*>(B.host + ent_bytes);
  std::vector<int> order(small);
  order.insert(order.end(), big.begin(), big.end());
  for (int j = 0; j < kd; j++) {
    tdr_filter* g = f[order[j]];
    tab[j] = TdrBatchPoseEntry{g->st.p, g->cap, g->n, res_dev + (size_t)TDR_BATCH_POSE_FLOATS * j, g->stats.p + 24};
  }
  const TdrBatchPoseEntry* tab_dev = reinterpret_cast<const TdrBatchPoseEntry*>(B.dev.p);
  HTRY(hipMemcpyAsync(B.dev.p, B.host, ent_bytes, hipMemcpyHostToDevice, s));
  TTRY(tdr_batch_pose_launch(tab_dev, ks, tab_dev + ks, kb, s));
  HTRY(hipMemcpyAsync(res_host, res_dev, res_bytes, hipMemcpyDeviceToHost, s));
  HTRY(hipEventRecord(B.done, s));
  HTRY(hipEventRecord(B.uploaded, s));
  HTRY(hipEventSynchronize(B.done));   // the one wait of the call
  for (int j = 0; j < kd; j++) {
    tdr_filter* g = f[order[j]];
    const float* rec = res_host + (size_t)TDR_BATCH_POSE_FLOATS * j;
    tdr_pose_stats& o = out[order[j]];
    std::memcpy(g->mean_cov_host, rec, sizeof(g->mean_cov_host));   // the cache tdr_filter_mean_cov(f, 0, ...) reads
    g->mean_cov_valid = true;
    std::memcpy(o.mean, rec, sizeof(o.mean));
    std::memcpy(o.cov, rec + 4, sizeof(o.cov));
    if (g->fp.fixed_scale > 0) {           // tdr_filter_scale
      o.scale = g->fp.fixed_scale;
    } else if (g->scale_frozen) {
      o.scale = rec[24];
      g->scale_host = rec[24];
      g->scale_valid = true;
    } else {
      o.scale = -1.f;
    }
  }
  return TDR_OK;
}
}  // extern "C"

// ---- the mixture fit on the device: tdr_filter_compute_gmm_device, tdr_batch_compute_gmm (csrc/tdr_gmm.hip) ---------------
namespace {
thread_local StageCtx g_gmm_stage;
constexpr size_t GMM_OUT_MAX = 21 * TDR_GMM_MAX_K + 2;

// what one filter's fit needs in its gmm_dev (doubles): samples [4 num] | 3 outputs | the candidates' workspaces
struct GmmPlan {
  int num = 0, cand[3] = {0, 0, 0};
  size_t ws_off[3] = {0, 0, 0}, total = 0;
  static size_t out_off(int num, int j) { return (size_t)4 * num + GMM_OUT_MAX * j; }
};
int gmm_plan(const tdr_filter* f, GmmPlan& p) {
  p.num = (int)std::min<int64_t>(1000, f->n);   // :262
  TTRY(tdr_gmm_candidates_host(f->num_gaussians, f->n, p.num, TDR_GMM_MAX_K, p.cand));
  p.total = GmmPlan::out_off(p.num, 3);
  for (int j = 0; j < 3; j++) {
    p.ws_off[j] = p.total;
    if (p.cand[j]) p.total += tdr_gmm_workspace_bytes(p.num, p.cand[j]) / sizeof(double);
  }
  return TDR_OK;
}

// The two ways the samples reach a filter's gmm_dev.  One filter, possibly sharded: tdr_filter_compute_gmm's sampling
// (filter_global_states + tdr_k_sample_ml_states) and the conversion, on `s`.
int gmm_sample_filter(tdr_filter* f, int num, hipStream_t s) {
  const float* gst = nullptr;
  int64_t gcap = 0;
  TTRY(f->gmm_samples.resize((size_t)3 * num));
  TTRY(filter_global_states(f, &gst, &gcap));
  TTRY(tdr_k_sample_ml_states(gst, gcap, f->n, num, f->gmm_samples.p, s));
  return tdr_k_gmm_samples(f->gmm_samples.p, num, f->gmm_dev.p, s);
}
// A batch: `s` continues after everything already queued on the filters' own streams; the samples are then one launch
// over the uploaded table (tdr_gmm_batch_samples).
int gmm_wait_filters(tdr_filter* const* fl, int k, hipStream_t s) {
  std::vector<hipStream_t> streams;
  for (int i = 0; i < k; i++)
    if (fl[i]->n >= 1) streams.push_back(fl[i]->stream);
  std::sort(streams.begin(), streams.end());
  streams.erase(std::unique(streams.begin(), streams.end()), streams.end());
  for (hipStream_t fs : streams) {
    if (fs == s) continue;
    hipEvent_t e = nullptr;
    HTRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    int rc = TDR_OK;
    if (hipEventRecord(e, fs) != hipSuccess || hipStreamWaitEvent(s, e, 0) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_compute_gmm: stream order");
    (void)hipEventDestroy(e);
    if (rc != TDR_OK) return rc;
  }
  return TDR_OK;
}

// The fit of the filters fl[0 .. k) that hold particles, on `s`: tables, sample(live filters, their plans, the device
// table of their sample entries), every candidate fit, the picks, one read-back, the host conversion.
extern "C++" template <class Sample>
int gmm_device_run(tdr_filter* const* fl, int k, hipStream_t s, Sample sample) {
  std::vector<tdr_filter*> live;
  for (int i = 0; i < k; i++)
    if (fl[i]->n >= 1) live.push_back(fl[i]);
  const int kd = (int)live.size();
  if (kd == 0) return TDR_OK;
  std::vector<GmmPlan> plan((size_t)kd);
  int nj = 0;
  for (int i = 0; i < kd; i++) {
    TTRY(gmm_plan(live[i], plan[i]));
    TTRY(live[i]->gmm_dev.resize(plan[i].total));
    for (int j = 0; j < 3; j++) nj += plan[i].cand[j] != 0;
  }
  // staging: [kd] sample entries, [nj] fit jobs, [kd] pick jobs; then the [kd] records the pick writes and the copy brings back
  const size_t samp_off = 0, job_off = align64(sizeof(TdrGmmSampleEntry) * (size_t)kd);
  const size_t pick_off = job_off + align64(sizeof(tdr_gmm_job) * (size_t)nj);
  const size_t rec_off = pick_off + align64(sizeof(tdr_gmm_pick_job) * (size_t)kd);
  const size_t rec_bytes = sizeof(double) * TDR_GMM_RECORD_DOUBLES * (size_t)kd;
  StageCtx& B = g_gmm_stage;
  TTRY(B.reserve(rec_off + rec_bytes, rec_off + rec_bytes, s));
  TdrGmmSampleEntry* samp = reinterpret_cast<TdrGmmSampleEntry*>(B.host + samp_off);
  tdr_gmm_job* jobs = reinterpret_cast<tdr_gmm_job*>(B.host + job_off);
  tdr_gmm_pick_job* picks = reinterpret_cast<tdr_gmm_pick_job*>(B.host + pick_off);
  double* rec_dev = reinterpret_cast<double*>(B.dev.p + rec_off);
  const double* rec_host = reinterpret_cast<const double*>(B.host + rec_off);
  int jn = 0;
  for (int i = 0; i < kd; i++) {
    tdr_filter* f = live[i];
    const GmmPlan& p = plan[i];
    double* base = f->gmm_dev.p;
    samp[i] = TdrGmmSampleEntry{f->st.p, f->cap, f->n, base, p.num, 0};
    picks[i] = tdr_gmm_pick_job{{nullptr, nullptr, nullptr}, p.cand[0], 0, rec_dev + (size_t)TDR_GMM_RECORD_DOUBLES * i};
    for (int j = 0; j < 3; j++) {
      if (!p.cand[j]) continue;
      double* out = base + GmmPlan::out_off(p.num, j);
      jobs[jn++] = tdr_gmm_job{base, p.num, p.cand[j], 100, 0, out, base + p.ws_off[j]};
      picks[i].cand[j] = out;
    }
  }
  HTRY(hipMemcpyAsync(B.dev.p, B.host, rec_off, hipMemcpyHostToDevice, s));
  HTRY(hipMemsetAsync(rec_dev, 0, rec_bytes, s));   // (a fit that wrote nothing is seen as a count of 0)
  TTRY(sample(live, plan, reinterpret_cast<const TdrGmmSampleEntry*>(B.dev.p + samp_off)));
  TTRY(tdr_k_gmm_fit_jobs(reinterpret_cast<const tdr_gmm_job*>(B.dev.p + job_off), nj, s));
  TTRY(tdr_k_gmm_pick(reinterpret_cast<const tdr_gmm_pick_job*>(B.dev.p + pick_off), kd, s));
  HTRY(hipMemcpyAsync(B.host + rec_off, rec_dev, rec_bytes, hipMemcpyDeviceToHost, s));
  HTRY(hipEventRecord(B.done, s));
  HTRY(hipEventRecord(B.uploaded, s));
  HTRY(hipEventSynchronize(B.done));   // the one wait of the call
  for (int i = 0; i < kd; i++) {
    const int kc = (int)rec_host[(size_t)TDR_GMM_RECORD_DOUBLES * i];
    if (kc < 1 || kc > TDR_GMM_MAX_K) return failh(TDR_ERR_HIP, "compute_gmm_device: the device fit left no mixture");
  }
  for (int i = 0; i < kd; i++) {   // the conversion of tdr_gmm_select_host (:303-312), on the host's libm
    tdr_filter* f = live[i];
    const double* rec = rec_host + (size_t)TDR_GMM_RECORD_DOUBLES * i;
    const int kc = (int)rec[0];
    f->num_gaussians = kc;
    f->gmm_means.resize((size_t)3 * kc);
    f->gmm_covs.resize((size_t)9 * kc);
    for (int c = 0; c < kc; c++) {
      const double* o = rec + 2 + 8 * c;
      f->gmm_means[3 * c + 0] = (float)o[0];
      f->gmm_means[3 * c + 1] = (float)o[1];
      f->gmm_means[3 * c + 2] = (float)std::atan2(o[3], o[2]);
      float* q = f->gmm_covs.data() + 9 * c;
      q[0] = (float)o[4]; q[1] = (float)o[5]; q[2] = 0.f;
      q[3] = (float)o[6]; q[4] = (float)o[7]; q[5] = 0.f;
      q[6] = 0.f; q[7] = 0.f; q[8] = 1.f;
    }
  }
  return TDR_OK;
}
}  // namespace

extern "C" {
int tdr_filter_compute_gmm_device(tdr_filter* f) {
  if (!f) return failh(TDR_ERR_ARG, "filter_compute_gmm_device: null filter");
  if (f->n < 1) return TDR_OK;
  return gmm_device_run(&f, 1, f->stream, [&](const std::vector<tdr_filter*>& live, const std::vector<GmmPlan>& plan,
                                              const TdrGmmSampleEntry*) { return gmm_sample_filter(live[0], plan[0].num, f->stream); });
}

int tdr_batch_compute_gmm(tdr_filter* const* filters, int k, void* stream) {
  if (k < 1) return failh(TDR_ERR_ARG, "batch_compute_gmm: k = %d, at least one filter is needed", k);
  if (!filters) return failh(TDR_ERR_ARG, "batch_compute_gmm: null filter array");
  for (int i = 0; i < k; i++)
    if (!filters[i]) return failh(TDR_ERR_ARG, "batch_compute_gmm: filter %d is null", i);
  {
    std::vector<const tdr_filter*> seen(filters, filters + k);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return failh(TDR_ERR_ARG, "batch_compute_gmm: a filter appears twice in the batch");
  }
  for (int i = 0; i < k; i++)
    if (filters[i]->comm) return failh(TDR_ERR_ARG, "batch_compute_gmm: filter %d is sharded (the gather inside is collective)", i);
  hipStream_t s = (hipStream_t)stream;
  TTRY(gmm_wait_filters(filters, k, s));
  return gmm_device_run(filters, k, s, [&](const std::vector<tdr_filter*>& live, const std::vector<GmmPlan>&,
                                           const TdrGmmSampleEntry* tab_dev) { return tdr_gmm_batch_samples(tab_dev, (int)live.size(), s); });
}
}  // extern "C"

// ---- device self-test of the scoring kernels -------------------------------------------------------------------------------
// The integer-form kernels run hand-scheduled, generated assembly (tdr_score_su_asm.h, tdr_score_cart_asm.h): a toolchain
// change must fail LOUDLY, not shift weights.  A tiny fixed problem, scored every way the library can score it:
//   polar      integer form, dense share through score_polar_su_kernel  ==  all particles through score_polar_ray_kernel
//              (bit for bit: the sums are exact), and both against the float kernel score_polar_kernel (rounding: 3e-6)
//   Cartesian  score_cart_su_kernel (generated loop)  ==  score_cart_skip_kernel<INT> (plain C++)  ==  score_cart_ray_kernel,
//              and against the float kernel
// Each run's variant is a TdrConfigScope on this thread: the process-wide switches are never written.
int tdr_selftest_score(void) {
  constexpr int NCLS = 6, SIZE = 160, NB = 64, NR = 32, CR = 32, CC = 24, N = 512;
  auto selftest_variant = [](int mode, float span, int seg_rows) {   // the configuration in force, with a run's choices
    TdrConfig c = tdr_cfg();
    c.su_mode = mode;
    c.su_span = span;
    c.su_span_fixed = true;
    c.cart_seg_rows = seg_rows;
    return c;
  };
  // a label image: bands of classes, a road grid (class 1), an unlabelled hole
  std::vector<uint8_t> lab((size_t)SIZE * SIZE);
  for (int y = 0; y < SIZE; y++)
    for (int x = 0; x < SIZE; x++) {
      int c = ((x / 13) + 2 * (y / 17)) % NCLS;
      if (c == 1) c = 2;
      if (x % 40 < 3 || y % 40 < 3) c = 1;
      if (x >= 100 && x < 120 && y >= 30 && y < 52) c = 255;   // unknown
      lab[(size_t)y * SIZE + x] = (uint8_t)c;
    }
  int32_t lut[256];
  for (int i = 0; i < 256; i++) lut[i] = i < NCLS ? i : -1;
  tdr_map* m = nullptr;
  TTRY(tdr_map_create(&m));
  struct MapGuard { tdr_map* m; ~MapGuard() { tdr_map_destroy(m); } } mg{m};
  TTRY(tdr_map_set_labels(m, lab.data(), SIZE, SIZE, lut, 256, NCLS, 1.f, 0, 0));
  TTRY(tdr_map_sample_pts_polar(m, NB, NR, (float)(2 * M_PI / NB)));
  // scans: integer counts, mostly one class per bin, some bins with two, many empty
  auto make_scan = [&](int rows, int cols, std::vector<float>& img) {
    img.assign((size_t)NCLS * rows * cols, 0.f);
    uint32_t h = 12345u;
    for (int k = 0; k < rows * cols; k++) {
      h = h * 1664525u + 1013904223u;
      const uint32_t r = h >> 8;
      if (r % 100 < 55) continue;
      const int c = (int)((r >> 7) % NCLS);
      img[(size_t)c * rows * cols + k] = (float)(1 + (r >> 11) % 5);
      if (r % 100 > 96) img[(size_t)((c + 2) % NCLS) * rows * cols + k] = (float)(1 + (r >> 15) % 3);
    }
  };
  std::vector<float> scan_p, scan_c;
  make_scan(NB, NR, scan_p);
  make_scan(CR, CC, scan_c);
  // particles: a cluster inside the map (different headings), a few at the border and outside
  std::vector<tdr_state> st(N);
  {
    uint32_t h = 777u;
    auto u01 = [&]() { h = h * 1664525u + 1013904223u; return (float)(h >> 8) / 16777216.f; };
    for (int p = 0; p < N; p++) {
      tdr_state s{};
      s.init_x_px = 70.f + 14.f * (u01() - 0.5f);
      s.init_y_px = 85.f + 14.f * (u01() - 0.5f);
      s.theta = 0.4f + 0.5f * (u01() - 0.5f);
      s.scale = 1.f;
      s.have_init = 1;
      if (p % 61 == 0) { s.init_x_px = 2.f + 150.f * u01(); s.init_y_px = (p % 2) ? 1.f : 158.f; }
      if (p == 3) { s.init_x_px = -40.f; s.init_y_px = 80.f; }
      st[(size_t)p] = s;
    }
  }
  tdr_filter_params fp{};
  fp.pos_cov = 0.3f; fp.theta_cov = 0.03f; fp.regularization = 0.15f;
  fp.fixed_scale = 1.f; fp.scale_log_min = -0.1f; fp.scale_log_max = 1.f;
  fp.num_classes = NCLS;
  for (int c = 0; c < 16; c++) fp.class_weights[c] = c < NCLS ? 1.f : 0.f;
  tdr_filter* f = nullptr;
  TTRY(tdr_filter_create(m, N, &fp, 1, &f));
  struct FilterGuard { tdr_filter* f; ~FilterGuard() { tdr_filter_destroy(f); } } fg{f};
  TTRY(tdr_filter_set_states(f, st.data(), N));
  std::vector<float> got[6];
  auto rel_ok = [](const std::vector<float>& a, const std::vector<float>& b, double tol, double* worst) {
    *worst = 0;
    for (size_t i = 0; i < a.size(); i++) {
      if (std::isnan(a[i]) != std::isnan(b[i])) return false;
      if (std::isnan(a[i])) continue;
      const double d = std::fabs((double)a[i] - (double)b[i]) / std::max(std::fabs((double)b[i]), 1e-30);
      *worst = std::max(*worst, d);
    }
    return *worst <= tol;
  };
  auto same_bits = [](const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
  };
  // ---- polar: float kernel, integer form (dense share), integer form with every particle ray-mapped
  const struct { int mode; float span; } polar_runs[3] = {{0, 16.f}, {2, 16.f}, {2, 1e-6f}};
  for (int r = 0; r < 3; r++) {
    TdrConfigScope variant(selftest_variant(polar_runs[r].mode, polar_runs[r].span, tdr_cfg().cart_seg_rows));
    TTRY(tdr_filter_compute_weights(f, scan_p.data(), nullptr, 1.f));
    got[r].resize(N);
    TTRY(tdr_filter_get_raw_weights(f, got[r].data(), N));
  }
  double worst = 0;
  if (!same_bits(got[1], got[2]))
    return failh(TDR_ERR_HIP, "selftest: score_polar_su_kernel and score_polar_ray_kernel disagree (exact integer sums must "
                              "be identical): the generated loop does not survive this toolchain");
  if (!rel_ok(got[1], got[0], 3e-6, &worst))
    return failh(TDR_ERR_HIP, "selftest: the polar integer form is %.3g away from the float kernel", worst);
  int finite = 0;
  for (float w : got[1]) finite += std::isfinite(w) && w > 0.f;
  if (finite < N / 2) return failh(TDR_ERR_HIP, "selftest: only %d of %d polar weights are finite", finite, N);
  // ---- Cartesian: float kernel, plain integer kernel, generated loop (two segment lengths), ray-mapped
  {
    const int rf = tdr_rec_floats(NCLS);
    DevBuf<float> img, pk, raw, ws;
    TTRY(img.resize((size_t)NCLS * CR * CC));
    TTRY(pk.resize((size_t)CR * CC * rf));
    TTRY(raw.resize(N));
    TTRY(ws.resize(tdr_score_cart_workspace_floats(NCLS, CR, CC, N, N)));
    HTRY(hipMemcpyAsync(img.p, scan_c.data(), scan_c.size() * sizeof(float), hipMemcpyHostToDevice, f->stream));
    TTRY(tdr_k_pack_scan(img.p, NCLS, CR, CC, pk.p, f->stream));
    const struct { int mode; float span; int seg; } cart_runs[5] = {{0, 16.f, 32}, {2, 0.f, 0}, {2, 0.f, 8}, {2, 0.f, 32}, {2, 1e-6f, 32}};
    std::vector<float> c[5];
    for (int r = 0; r < 5; r++) {
      TdrConfigScope variant(selftest_variant(cart_runs[r].mode, cart_runs[r].span, cart_runs[r].seg));
      TTRY(tdr_k_score_cart(&m->desc, pk.p, CR, CC, 0.75f, &fp, f->st.p, f->cap, N, N, nullptr, raw.p, ws.p, f->stream));
      c[r].resize(N);
      HTRY(hipMemcpyAsync(c[r].data(), raw.p, N * sizeof(float), hipMemcpyDeviceToHost, f->stream));
      HTRY(hipStreamSynchronize(f->stream));
    }
    if (!same_bits(c[1], c[2]) || !same_bits(c[1], c[3]))
      return failh(TDR_ERR_HIP, "selftest: score_cart_su_kernel (generated loop) and score_cart_skip_kernel disagree (exact "
                                "integer sums must be identical): the generated loop does not survive this toolchain");
    if (!same_bits(c[1], c[4])) return failh(TDR_ERR_HIP, "selftest: score_cart_ray_kernel disagrees with the dense kernels");
    if (!rel_ok(c[1], c[0], 3e-6, &worst))
      return failh(TDR_ERR_HIP, "selftest: the Cartesian integer form is %.3g away from the float kernel", worst);
    finite = 0;
    for (float w : c[1]) finite += std::isfinite(w) && w > 0.f;
    if (finite < N / 2) return failh(TDR_ERR_HIP, "selftest: only %d of %d Cartesian weights are finite", finite, N);
  }
  return TDR_OK;
}

}  // extern "C"
