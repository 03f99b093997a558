// TopDownMap — reference surface: include/top_down_render/top_down_map.h:52-102.  Holds the per-class truncated
// distance maps + unknown mask on the GPU (tdr_map, include/tdr.h).  The reference builds these at load time from an
// SVG / PNG / cache file (src/top_down_map.cpp:9-64, OpenCV + nanosvg).  Here the constructor reads the reference's map
// cache, an SVG vector map (parsed on the host, filled and distance-transformed on the GPU), a colour PNG map (decoded
// on the host, colour lookup and distance transforms on the GPU) or a raster-cache directory.  JPEG maps are not
// decoded: decode them elsewhere and hand the BGR pixels to loadColorRasterMap().  Distance maps computed elsewhere are
// handed over with setDistanceMaps() in the layout of the reference's class_maps_ / class_mask_ members.
#ifndef TOP_DOWN_MAP_H_
#define TOP_DOWN_MAP_H_

#include <stdexcept>
#include <string>
#include <vector>

#include "tdr.h"
#include "top_down_render/scan_viz_device.h"
#include "top_down_render/tdr_compat.h"

class TopDownMap {
 public:
  struct Params {  // top_down_map.h:54-62, member for member
    std::string map_path = "";
    SemanticColorLut color_lut;   // the SVG loader's class colours (unpackColor(ind2Color(cls)), :80-84)
    std::vector<int> flatten_lut;
    int num_classes = 0;
    std::vector<int> exclusive_classes;
    float resolution = 1;
    float out_of_bounds_const = 5;  // unused by the reference too: every out-of-bounds write is a literal 0
  };
  // src/top_down_map.cpp:9-64.  An empty map_path is the dynamic-map case (the map arrives through updateMap).  A static
  // map is taken from the reference's own cache — ~/.ros/xview_cache, written by the reference or by saveCachedMaps() —
  // when its (map_path, num_classes, resolution) match (:18-20, :226-261), else from a raster-cache directory of class<i>.png
  // (:42-46), else — a .svg map_path — from the vector map (:22-31): parse, class fill on the GPU, the raster cache
  // <stem>_raster_cache/class<i>.png, geometric layers and distance maps, then the map cache (:61); else — a .png
  // map_path — from the colour raster map (:32-42): cv::imread's BGR image, color2Ind against the keys of
  // params_.color_lut (the SVG loader's keys), loadCompressedRasterMap, geometric layers and distance maps, then the map
  // cache (:61; no raster cache on this branch).  A file that does not parse or decode leaves the map empty
  // (haveMap() == false, the reason in tdr_last_error()) and writes nothing.  A .jpg map is not decoded: it stays empty
  // (tdr_last_error() says so) until loadColorRasterMap(), setDistanceMaps() or updateMap() provide the map.
  explicit TopDownMap(const Params& params, const char* cache_dir = nullptr) : params_(params) {
    if (tdr_map_create(&m_) != TDR_OK) throw std::runtime_error(std::string("TopDownMap: ") + tdr_last_error());
    if (!params_.map_path.empty() && params_.num_classes > 0) {
      int loaded = 0;
      if (tdr_map_load_cache(m_, cache_dir, params_.map_path.c_str(), params_.num_classes, params_.resolution, 0, 0,
                             &loaded) != TDR_OK) {
        const std::string msg = std::string("TopDownMap: ") + tdr_last_error();
        tdr_map_destroy(m_);
        throw std::runtime_error(msg);
      }
      // a map_path that is neither .svg nor .png / .jpg names a raster-cache directory (:42-46): class<i>.png, read
      // over zlib, distance transforms on the GPU; then the cache is written like the reference does (:61)
      const std::string& mp = params_.map_path;
      const std::string ext = mp.size() >= 4 ? mp.substr(mp.size() - 4) : std::string();
      if (!loaded && ext != ".svg" && ext != ".png" && ext != ".jpg" &&
          tdr_map_load_rasters(m_, mp.c_str(), params_.num_classes, params_.resolution, 0, 0) == TDR_OK)
        (void)tdr_map_save_cache(m_, cache_dir, mp.c_str());
      if (!loaded && ext == ".svg" && load_svg(mp)) {
        (void)tdr_map_save_rasters(m_, (mp.substr(0, mp.size() - 4) + "_raster_cache").c_str());   // :31
        (void)tdr_map_save_cache(m_, cache_dir, mp.c_str());                                       // :61
      }
      if (!loaded && ext == ".png" && load_color_png(mp)) (void)tdr_map_save_cache(m_, cache_dir, mp.c_str());   // :61
      if (!loaded && ext == ".jpg")
        tdr_set_error(TDR_ERR_ARG, "TopDownMap: JPEG maps are not decoded here; decode the map (e.g. cv::imread) and hand "
                                   "its BGR pixels to loadColorRasterMap() / tdr_map_load_color_image()");
    }
  }
  // saveRasterizedMaps / loadRasterizedMaps (:197-224): a directory of class<i>.png (8-bit grey, 0 inside the class,
  // flipped like the reference stores them); load = rasters -> geometric layers -> distance maps, on the GPU
  void saveRasterizedMaps(const std::string& path) {
    if (tdr_map_save_rasters(m_, path.c_str()) != TDR_OK)
      throw std::runtime_error(std::string("saveRasterizedMaps: ") + tdr_last_error());
  }
  void loadRasterizedMaps(const std::string& map_path) {
    if (tdr_map_load_rasters(m_, map_path.c_str(), params_.num_classes, params_.resolution, map_center_[0], map_center_[1]) != TDR_OK)
      throw std::runtime_error(std::string("loadRasterizedMaps: ") + tdr_last_error());
  }
  // saveCachedMaps (:263-286): the cache the constructor above (and the reference) reads
  void saveCachedMaps(const std::string& map_path, const char* cache_dir = nullptr) {
    if (tdr_map_save_cache(m_, cache_dir, map_path.c_str()) != TDR_OK)
      throw std::runtime_error(std::string("saveCachedMaps: ") + tdr_last_error());
  }
  virtual ~TopDownMap() { tdr_map_destroy(m_); }
  TopDownMap(const TopDownMap&) = delete;
  TopDownMap& operator=(const TopDownMap&) = delete;

  // class_maps_[c] (rows = height/resolution, cols = width/resolution, column-major) and class_mask_ (1 = unknown),
  // as computeDists leaves them (src/top_down_map.cpp:289-326).  Also the map side of updateMap (:146-157).
  void setDistanceMaps(const std::vector<Eigen::ArrayXXf>& class_maps, const Eigen::ArrayXXc& class_mask,
                       const Eigen::Vector2i& map_center = Eigen::Vector2i(0, 0)) {
    if (class_maps.empty()) return;
    const int rows = (int)class_maps[0].rows(), cols = (int)class_maps[0].cols(), ncls = (int)class_maps.size();
    std::vector<float> buf((size_t)rows * cols * ncls);
    for (int c = 0; c < ncls; c++)
      std::memcpy(buf.data() + (size_t)c * rows * cols, class_maps[c].data(), (size_t)rows * cols * sizeof(float));
    if (tdr_map_set(m_, buf.data(), class_mask.data(), ncls, rows, cols, params_.resolution, map_center[0],
                    map_center[1]) != TDR_OK)
      throw std::runtime_error(std::string("TopDownMap::setDistanceMaps: ") + tdr_last_error());
    params_.num_classes = ncls;
    map_center_ = map_center;
  }
  // updateMap (src/top_down_map.cpp:146-157) for a class-index image in cv::Mat CV_8UC1 layout (row 0 = top):
  // loadCompressedRasterMap + computeDists run on the GPU.  `flatten_lut` is Params::flatten_lut.
  void updateMap(const uint8_t* label_img, int img_h, int img_w, const Eigen::Vector2i& map_center) {
    std::vector<int32_t> lut(params_.flatten_lut.begin(), params_.flatten_lut.end());
    if (lut.empty() || params_.num_classes < 1) throw std::invalid_argument("updateMap: Params::flatten_lut / num_classes not set");
    if (tdr_map_set_labels(m_, label_img, img_h, img_w, lut.data(), (int)lut.size(), params_.num_classes,
                           params_.resolution, map_center[0], map_center[1]) != TDR_OK)
      throw std::runtime_error(std::string("TopDownMap::updateMap: ") + tdr_last_error());
    map_center_ = map_center;
  }
  void updateMap(const cv::Mat& map, const Eigen::Vector2i& map_center) {  // the reference's signature (:146-157)
    if (map.empty()) throw std::invalid_argument("updateMap: empty image");
    if (map.isContinuous()) return updateMap(map.ptr<uint8_t>(), map.rows, map.cols, map_center);
    std::vector<uint8_t> packed((size_t)map.rows * map.cols);   // a view with row padding: pack the rows
    for (int r = 0; r < map.rows; r++) std::memcpy(packed.data() + (size_t)r * map.cols, map.ptr<uint8_t>(r), (size_t)map.cols);
    updateMap(packed.data(), map.rows, map.cols, map_center);
  }
  // updateMap's end state, byte for byte, reached by rebuilding only the cells a changed class can reach
  // (tdr_map_update_labels_incremental).  Returns the number of cells whose class changed, or -1 when it took the full
  // path (no previous label-image map, another shape / resolution / LUT, or a change over half the map).
  int64_t updateMapIncremental(const uint8_t* label_img, int img_h, int img_w, const Eigen::Vector2i& map_center) {
    std::vector<int32_t> lut(params_.flatten_lut.begin(), params_.flatten_lut.end());
    if (lut.empty() || params_.num_classes < 1)
      throw std::invalid_argument("updateMapIncremental: Params::flatten_lut / num_classes not set");
    int64_t changed = -1;
    if (tdr_map_update_labels_incremental(m_, label_img, img_h, img_w, lut.data(), (int)lut.size(), params_.num_classes,
                                          params_.resolution, map_center[0], map_center[1], &changed) != TDR_OK)
      throw std::runtime_error(std::string("TopDownMap::updateMapIncremental: ") + tdr_last_error());
    map_center_ = map_center;
    return changed;
  }
  int64_t updateMapIncremental(const cv::Mat& map, const Eigen::Vector2i& map_center) {
    if (map.empty()) throw std::invalid_argument("updateMapIncremental: empty image");
    if (map.isContinuous()) return updateMapIncremental(map.ptr<uint8_t>(), map.rows, map.cols, map_center);
    std::vector<uint8_t> packed((size_t)map.rows * map.cols);
    for (int r = 0; r < map.rows; r++) std::memcpy(packed.data() + (size_t)r * map.cols, map.ptr<uint8_t>(r), (size_t)map.cols);
    return updateMapIncremental(packed.data(), map.rows, map.cols, map_center);
  }
  // The last label image with the image rectangle [y0, y0 + h) x [x0, x0 + w) (row 0 = top) overwritten by `patch`
  // (h x w, rows packed), for a host that knows what changed (tdr_map_patch_labels).  Returns the changed-cell count.
  int64_t patchMap(const uint8_t* patch, int y0, int x0, int h, int w, const Eigen::Vector2i& map_center) {
    int64_t changed = -1;
    if (tdr_map_patch_labels(m_, patch, y0, x0, h, w, map_center[0], map_center[1], &changed) != TDR_OK)
      throw std::runtime_error(std::string("TopDownMap::patchMap: ") + tdr_last_error());
    map_center_ = map_center;
    return changed;
  }
  // The constructor's colour-map branch (:32-42, 48-63) for a BGR image the caller decoded (cv::imread's layout: 3 bytes
  // B, G, R per pixel, row 0 = top), e.g. a .jpg map: color2Ind against params_.color_lut, loadCompressedRasterMap,
  // geometric layers and distance maps on the GPU; haveMap() turns true even without road (:63).
  void loadColorRasterMap(const uint8_t* bgr, int img_h, int img_w,
                          const Eigen::Vector2i& map_center = Eigen::Vector2i(0, 0)) {
    std::vector<uint32_t> keys = color_keys();
    std::vector<int32_t> lut(params_.flatten_lut.begin(), params_.flatten_lut.end());
    if (lut.empty() || params_.num_classes < 1)
      throw std::invalid_argument("loadColorRasterMap: Params::flatten_lut / num_classes not set");
    if (tdr_map_load_color_image(m_, bgr, img_h, img_w, keys.data(), lut.data(), (int)lut.size(), params_.num_classes,
                                 params_.resolution, map_center[0], map_center[1]) != TDR_OK)
      throw std::runtime_error(std::string("TopDownMap::loadColorRasterMap: ") + tdr_last_error());
    map_center_ = map_center;
  }
  template <class MatT = cv::Mat>   // a cv::Mat of CV_8UC3 (a template: only instantiated where it is called)
  void loadColorRasterMap(const MatT& bgr, const Eigen::Vector2i& map_center = Eigen::Vector2i(0, 0)) {
    if (bgr.empty() || bgr.elemSize() != 3) throw std::invalid_argument("loadColorRasterMap: needs an 8-bit BGR image");
    if (bgr.isContinuous()) return loadColorRasterMap(bgr.template ptr<uint8_t>(), bgr.rows, bgr.cols, map_center);
    std::vector<uint8_t> packed((size_t)bgr.rows * bgr.cols * 3);   // a view with row padding: pack the rows
    for (int r = 0; r < bgr.rows; r++)
      std::memcpy(packed.data() + (size_t)r * bgr.cols * 3, bgr.template ptr<uint8_t>(r), (size_t)bgr.cols * 3);
    loadColorRasterMap(packed.data(), bgr.rows, bgr.cols, map_center);
  }
  const Params& params() const { return params_; }
  void getClassesAtPoint(const Eigen::Vector2i& center_ind, std::vector<int>& classes) {  // top_down_map.cpp:159-170
    classes.clear();
    uint32_t bits = 0;
    if (tdr_map_classes_at_point(m_, center_ind[0], center_ind[1], &bits) != TDR_OK) return;
    for (int c = 0; c < params_.num_classes; c++)
      if (bits & (1u << c)) classes.push_back(c);
  }
  // getLocalMap (src/top_down_map.cpp:429-459): the Cartesian window of one pose; sizes are read off dists[0] like the
  // reference does; dists.size() < 1 -> nothing happens (:431).  mask: 1 = unknown or outside the map.
  void getLocalMap(Eigen::Vector2f center, float rot, float res, std::vector<Eigen::ArrayXXf>& dists,
                   Eigen::ArrayXXc& mask) {
    if (dists.size() < 1) return;
    local_map(0, center, rot, res, (int)dists[0].rows(), (int)dists[0].cols(), dists, mask);
  }
  // getLocalGeoMap (:461-481): the same window gathered from the two geometric layers geo_maps_ ([0] distance to the
  // nearest cell without a geometric class, [1] with one); dists.size() < 1 -> nothing happens (:464).
  void getLocalGeoMap(Eigen::Vector2f center, float rot, float res, std::vector<Eigen::ArrayXXf>& dists) {
    if (dists.size() < 1) return;
    local_geo_map(0, center, rot, res, (int)dists[0].rows(), (int)dists[0].cols(), dists);
  }
  // Extension: the window shape (rows = y, cols = x) a Cartesian filter scores against (ParticleFilterCartesian,
  // particle_filter_cartesian.h; BASELINE config 4) — the sizes getLocalMap reads off the caller's arrays, fixed for the filter.
  void setWindow(int rows, int cols) {
    if (tdr_map_set_window(m_, rows, cols) != TDR_OK) throw std::invalid_argument(std::string("setWindow: ") + tdr_last_error());
  }
  Eigen::Vector2i windowShape() const {   // (rows, cols) of the last setWindow; (0, 0) before
    int rows = 0, cols = 0;
    tdr_map_window_shape(m_, &rows, &cols);
    return Eigen::Vector2i(rows, cols);
  }
  void getClassesAtPoint(const Eigen::Vector2f& center, std::vector<int>& classes) {      // :172-175
    getClassesAtPoint(Eigen::Vector2i((int)(center[0] / params_.resolution), (int)(center[1] / params_.resolution)), classes);
  }
  Eigen::Vector2i size() const {
    int rows = 0, cols = 0;
    tdr_map_info(m_, nullptr, &rows, &cols, nullptr, nullptr);
    return Eigen::Vector2i(cols, rows);
  }
  Eigen::Vector2i mapCenter() const {   // asks the handle: ParticleFilter::updateMap moves the centre too
    int cx = map_center_[0], cy = map_center_[1];
    tdr_map_center(m_, &cx, &cy);
    return Eigen::Vector2i(cx, cy);
  }
  int numClasses() const { return params_.num_classes; }
  float resolution() const { return params_.resolution; }
  bool haveMap() const {
    int have = 0;
    tdr_map_info(m_, nullptr, nullptr, nullptr, nullptr, &have);
    return have != 0;
  }
  tdr_map* handle() const { return m_; }
  // The road list (extension; include/tdr.h, "recovery injection"): the ascending cell indices r * cols + c of the cells the
  // on-road test of particle initialisation accepts, read back from the device (the map keeps its device copy until its
  // records are written again).  Throws on a map without records, with fewer than two classes or without a road cell.
  std::vector<uint32_t> roadCells() {
    int64_t n = 0;
    if (tdr_map_read_road_cells(m_, nullptr, 0, &n) != TDR_OK) throw std::invalid_argument(std::string("roadCells: ") + tdr_last_error());
    std::vector<uint32_t> out((size_t)n);
    if (tdr_map_read_road_cells(m_, out.data(), n, &n) != TDR_OK) throw std::runtime_error(std::string("roadCells: ") + tdr_last_error());
    return out;
  }
  // The fleet picture's background (include/tdr.h, "the fleet picture"): ONE device copy for every filter on this map,
  // which ParticleFilterBatch::renderFleet draws all of them over.  Kept until it is set again; updateMap leaves it
  // alone.  bgr: an 8-bit image of three channels; or the label image the node colours (aerialMapCallback, :584), one
  // byte a cell, coloured on the device through lut.  The filters' own backgrounds (ParticleFilter::setVizBackground)
  // are separate.
  template <class MatT = cv::Mat>
  void setVizBackground(const MatT& bgr) { tdr_viz::setBackground(m_, bgr); }
  template <class MatT = cv::Mat>
  void setVizBackground(const MatT& labels, const SemanticColorLut& lut) { tdr_viz::setBackgroundLabels(m_, labels, lut); }

 protected:
  void local_map(int polar, const Eigen::Vector2f& center, float scale_or_rot, float res, int rows, int cols,
                 std::vector<Eigen::ArrayXXf>& dists, Eigen::ArrayXXc& mask) {
    const int ncls = params_.num_classes;
    // sizes the call cannot use: a silent return like the reference's (top_down_map.cpp:431, top_down_map_polar.cpp:25),
    // the reason in tdr_last_error()
    if ((int)dists.size() < ncls) { tdr_set_error(TDR_ERR_ARG, "getLocalMap: fewer output arrays than map classes"); return; }
    const size_t P = (size_t)rows * cols;
    for (int c = 0; c < ncls; c++)
      if ((size_t)dists[c].rows() * dists[c].cols() != P) { tdr_set_error(TDR_ERR_ARG, "getLocalMap: output arrays of different sizes"); return; }
    if ((size_t)mask.rows() * mask.cols() != P) { tdr_set_error(TDR_ERR_ARG, "getLocalMap: mask size differs from the windows'"); return; }
    std::vector<float> d(P * ncls);
    std::vector<uint8_t> k(P);
    if (tdr_map_local_map(m_, polar, center[0], center[1], scale_or_rot, res, rows, cols, d.data(), k.data()) != TDR_OK)
      throw std::runtime_error(std::string("getLocalMap: ") + tdr_last_error());
    for (int c = 0; c < ncls; c++) std::memcpy(dists[c].data(), d.data() + P * c, P * sizeof(float));
    std::memcpy(mask.data(), k.data(), P);
  }
  void local_geo_map(int polar, const Eigen::Vector2f& center, float scale_or_rot, float res, int rows, int cols,
                     std::vector<Eigen::ArrayXXf>& dists) {
    const size_t P = (size_t)rows * cols;
    for (size_t c = 0; c < dists.size() && c < 2; c++)
      if ((size_t)dists[c].rows() * dists[c].cols() != P) { tdr_set_error(TDR_ERR_ARG, "getLocalGeoMap: output arrays of different sizes"); return; }
    std::vector<float> d(P * 2);
    if (tdr_map_local_geo_map(m_, polar, center[0], center[1], scale_or_rot, res, rows, cols, d.data()) != TDR_OK)
      throw std::runtime_error(std::string("getLocalGeoMap: ") + tdr_last_error());
    for (size_t c = 0; c < dists.size() && c < 2; c++) std::memcpy(dists[c].data(), d.data() + P * c, P * sizeof(float));
  }
  // the key of LUT index cls: the reference's own expression (:80-84), so this compiles unchanged against
  // semantics_manager's SemanticColorLut.  unpackColor gives B, G, R, so the key of a cv::imread pixel px is
  // px[0] << 16 | px[1] << 8 | px[2]: the SVG fill #ff0000 and the PNG pixel RGB (255, 0, 0) both have the key 0x0000ff.
  std::vector<uint32_t> color_keys() const {
    std::vector<uint32_t> keys;
    for (size_t cls = 0; cls < params_.flatten_lut.size(); cls++) {
      auto color = SemanticColorLut::unpackColor(params_.color_lut.ind2Color(cls));
      keys.push_back((uint32_t)color[0] << 16 | (uint32_t)color[1] << 8 | (uint32_t)color[2]);
    }
    return keys;
  }
  // loadSvg + getRasterMap (:22-31)
  bool load_svg(const std::string& path) {
    std::vector<uint32_t> keys = color_keys();
    std::vector<int32_t> lut(params_.flatten_lut.begin(), params_.flatten_lut.end());
    std::vector<int32_t> excl(params_.exclusive_classes.begin(), params_.exclusive_classes.end());
    return tdr_map_load_svg(m_, path.c_str(), keys.data(), lut.data(), (int)lut.size(), params_.num_classes,
                            excl.data(), (int)excl.size(), params_.resolution, 0, 0) == TDR_OK;
  }
  // cv::imread + color2Ind + loadCompressedRasterMap (:32-42)
  bool load_color_png(const std::string& path) {
    std::vector<uint32_t> keys = color_keys();
    std::vector<int32_t> lut(params_.flatten_lut.begin(), params_.flatten_lut.end());
    if (lut.empty()) return tdr_set_error(TDR_ERR_ARG, "TopDownMap: Params::flatten_lut is empty"), false;
    return tdr_map_load_color_png(m_, path.c_str(), keys.data(), lut.data(), (int)lut.size(), params_.num_classes,
                                  params_.resolution, 0, 0) == TDR_OK;
  }
  Params params_;
  Eigen::Vector2i map_center_;
  tdr_map* m_ = nullptr;
};

#endif  // TOP_DOWN_MAP_H_
