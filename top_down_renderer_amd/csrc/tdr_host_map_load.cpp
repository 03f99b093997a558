// tdr_host_map_load.cpp — the static maps of TopDownMap's constructor behind tdr_map_load_* / tdr_map_save_*: the on-disk
// cache (.eig files, tdr_eig.cpp), the raster cache (class<i>.png), polygons and SVG (tdr_poly.hip, tdr_svg.cpp), the
// colour raster map (tdr_png.cpp).
#include <sys/stat.h>
#include <cerrno>

#include "tdr_host.h"

extern "C" {

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
  m->rec_written();   // before the write: a failed ingest leaves no list marked current
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
  m->rec_written();   // before the write, as in map_set_from_rasters
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

}  // extern "C"
