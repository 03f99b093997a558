// tdr_host_map.cpp — TopDownMap(Polar) behind tdr_map_*: create, the dynamic-map entry points (tdr_map_set,
// tdr_map_set_labels, the incremental updates), the polar table, the window queries, getBestRelPos; and the map-side
// helpers the other handle files call (geometric layers, compact records, the init search's scratch).
#include "tdr_host.h"

namespace tdrh {
// geo_maps_ for a freshly packed map: computed from the class maps like the static-map constructor does
// (src/top_down_map.cpp:48-58), or the constant 1 the dynamic-map path leaves them at (:126-133)
// Nothing on the hot path reads them (the reference's score ignores top_down_geo, state_particle.cpp:145-152): they are
// built — two more distance transforms over the whole map — when something first asks for them (map_ensure_geo).
int map_make_geo(tdr_map* m, bool constant_one) {
  m->geo_pending = constant_one ? 2 : 1;
  m->geo_rec.release();
  m->geo_desc = tdr_map_desc{};
  return TDR_OK;
}
int map_ensure_geo(tdr_map* m) {
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
int map_compact(tdr_map* m) {
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

// The half records of the 40-rotation search live in ONE scratch per map and every search rebuilds them for its class
// weights, so searches of the map's filters must not overlap in time — whichever streams they run on (the filters' own,
// the batch's).  A search that may use the scratch runs between these two: wait for the last one, leave an event behind.
int map_rec16_alloc(tdr_map* m, int64_t n) {
  if (m->desc.rec16 || n < tdr_cfg().rec16_min) return TDR_OK;
  const size_t b16 = tdr_map_rec16_bytes(m->desc.ncls, m->desc.rows, m->desc.cols);
  if (b16) {
    TTRY(m->rec16.resize(b16));
    m->desc.rec16 = m->rec16.p;
  }
  return TDR_OK;
}
int map_rec16_begin(tdr_map* m, hipStream_t s) {
  if (m->rec16_used) HTRY(hipStreamWaitEvent(s, m->rec16_used, 0));
  return TDR_OK;
}
int map_rec16_end(tdr_map* m, hipStream_t s) {
  if (!m->rec16_used) HTRY(hipEventCreateWithFlags(&m->rec16_used, hipEventDisableTiming));
  HTRY(hipEventRecord(m->rec16_used, s));
  return TDR_OK;
}
}  // namespace tdrh

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
  m->rec_written();
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
  m->rec_written();
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
  m->rec_written();
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

// ---- the fleet picture's background (include/tdr.h, "the fleet picture"): one device copy for every filter on the map ------
int tdr_map_set_viz_background(tdr_map* m, const uint8_t* bgr_host, int H, int W) {
  if (!m || !bgr_host) return failh(TDR_ERR_ARG, "map_set_viz_background: null argument");
  if (H < 11 || W < 11 || H > 32768 || W > 32768)
    return failh(TDR_ERR_ARG, "map_set_viz_background: a %d x %d image (11 .. 32768 a side)", H, W);
  const size_t bytes = (size_t)3 * H * W;
  HTRY(hipDeviceSynchronize());   // (a picture on any stream may still read the old background)
  TTRY(m->viz_bg.resize(bytes));
  HTRY(hipMemcpy(m->viz_bg.p, bgr_host, bytes, hipMemcpyHostToDevice));
  m->viz_h = H;
  m->viz_w = W;
  return TDR_OK;
}

// ... from a label image: one byte a cell goes up, the colour table is applied on the device (tdr_k_label_picture)
int tdr_map_set_viz_background_labels(tdr_map* m, const uint8_t* labels_host, int H, int W, const uint8_t* lut_bgr) {
  if (!m || !labels_host || !lut_bgr) return failh(TDR_ERR_ARG, "map_set_viz_background_labels: null argument");
  if (H < 11 || W < 11 || H > 32768 || W > 32768)
    return failh(TDR_ERR_ARG, "map_set_viz_background_labels: a %d x %d image (11 .. 32768 a side)", H, W);
  const size_t cells = (size_t)H * W;
  DevBuf<uint8_t> labels;   // staging of this call only
  HTRY(hipDeviceSynchronize());
  TTRY(m->viz_bg.resize(3 * cells));
  TTRY(labels.resize(cells));
  HTRY(hipMemcpy(labels.p, labels_host, cells, hipMemcpyHostToDevice));
  TTRY(tdr_k_label_picture(labels.p, (int64_t)cells, lut_bgr, m->viz_bg.p, nullptr));
  HTRY(hipStreamSynchronize(nullptr));
  m->viz_h = H;
  m->viz_w = W;
  return TDR_OK;
}

}  // extern "C"
