// MapFuser — beyond the reference's surface (its embryo is the offline tool src/refine_map.cpp): localised scans vote into
// the label map on the device, and apply() feeds the relabelled cells through the incremental map update (include/tdr.h,
// "map fusion").
//
//   MapFuser fuser(map, class_label, /*min_votes=*/3, {1, 2});     // map: last set from a label image (updateMap)
//   fuser.addScan(renderer, filter, res);                          // the renderer's last render at the filter's best state
//   fuser.apply({&filter});                                        // the filter scores against the new map from now on
//
// The constructor throws.  The per-scan calls return false without an exception when they are given something they cannot
// use (the project's convention for per-scan calls); the reason is in tdr_last_error().
#ifndef TDR_FACADE_MAP_FUSER_H_
#define TDR_FACADE_MAP_FUSER_H_

#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "top_down_render/particle_filter.h"

class MapFuser {
 public:
  struct Pose {   // what StateParticle::computeWeight passes on: the centre in map pixels, heading, scale
    float x = 0.f, y = 0.f, theta = 0.f, scale = 1.f;
  };
  struct Share {  // a verdict needs the winner to hold at least num / den of a cell's votes
    uint32_t num = 1, den = 2;
  };
  // class_label[c]: the raw label written for class c, the inverse of the map's flatten_lut
  MapFuser(TopDownMap& map, const std::vector<uint8_t>& class_label, uint32_t min_votes, Share share) {
    if ((int)class_label.size() < map.numClasses()) throw std::invalid_argument("MapFuser: one class_label entry per class");
    if (tdr_fuser_create(map.handle(), class_label.data(), min_votes, share.num, share.den, &f_) != TDR_OK)
      throw std::runtime_error(std::string("MapFuser: ") + tdr_last_error());
  }
  ~MapFuser() { tdr_fuser_destroy(f_); }
  MapFuser(const MapFuser&) = delete;
  MapFuser& operator=(const MapFuser&) = delete;

  // the renderer's last semantic render (polar or Cartesian), read on the device
  bool addScan(const ScanRenderer& renderer, const Pose& pose, float res) {
    return tdr_fuser_add(f_, renderer.handle(), pose.x, pose.y, pose.theta, pose.scale, res, &added_, &dropped_) == TDR_OK;
  }
  // ... at the filter's max-likelihood state {x, y, theta, scale} (false before the filter's first update)
  bool addScan(const ScanRenderer& renderer, ParticleFilter& filter, float res) {
    Pose p;
    return best(filter, p) && addScan(renderer, p, res);
  }
  // the scans of a ParticleFilterBatch: one render, filter and res per robot, one launch for all
  bool addScans(const std::vector<const ScanRenderer*>& renderers, const std::vector<ParticleFilter*>& filters,
                const std::vector<float>& res) {
    const size_t k = renderers.size();
    if (k == 0 || filters.size() != k || res.size() != k) return soft_fail("MapFuser::addScans: one renderer, filter and res per robot");
    std::vector<Pose> poses(k);
    for (size_t i = 0; i < k; i++)
      if (!filters[i] || !best(*filters[i], poses[i])) return false;
    return addScans(renderers, poses, res);
  }
  bool addScans(const std::vector<const ScanRenderer*>& renderers, const std::vector<Pose>& poses, const std::vector<float>& res) {
    const size_t k = renderers.size();
    if (k == 0 || poses.size() != k || res.size() != k) return soft_fail("MapFuser::addScans: one renderer, pose and res per robot");
    std::vector<const tdr_renderer*> handles(k, nullptr);
    std::vector<float> p(5 * k);
    for (size_t i = 0; i < k; i++) {
      if (!renderers[i]) return soft_fail("MapFuser::addScans: null renderer");
      handles[i] = renderers[i]->handle();
      const float row[5] = {poses[i].x, poses[i].y, poses[i].theta, poses[i].scale, res[i]};
      std::memcpy(p.data() + 5 * i, row, sizeof(row));
    }
    return tdr_fuser_add_batch(f_, handles.data(), (int)k, p.data(), &added_, &dropped_) == TDR_OK;
  }
  // host images as renderSemanticTopDown fills them, for callers without a renderer
  bool addImages(const std::vector<Eigen::ArrayXXf>& imgs, bool polar, const Pose& pose, float res) {
    if (imgs.empty()) return soft_fail("MapFuser::addImages: no images");
    const int rows = (int)imgs[0].rows(), cols = (int)imgs[0].cols();
    const size_t P = (size_t)rows * cols;
    for (const auto& im : imgs)
      if (im.rows() != rows || im.cols() != cols) return soft_fail("MapFuser::addImages: images of different sizes");
    uint64_t st[9];
    if (tdr_fuser_stats(f_, st) != TDR_OK) return false;
    if (imgs.size() != (size_t)st[4]) return soft_fail("MapFuser::addImages: one image per class of the map");
    std::vector<float> buf(P * imgs.size());
    for (size_t c = 0; c < imgs.size(); c++) std::memcpy(buf.data() + P * c, imgs[c].data(), P * sizeof(float));
    return tdr_fuser_add_images(f_, buf.data(), polar ? 1 : 0, rows, cols, pose.x, pose.y, pose.theta, pose.scale, res,
                                &added_, &dropped_) == TDR_OK;
  }
  uint64_t lastVotesAdded() const { return added_; }
  uint64_t lastVotesDropped() const { return dropped_; }

  // The label pass over the tiles that received votes; the changed rectangle goes into the map and the listed filters of
  // that map.  Returns the number of cells whose class changed; throws when refused.
  int64_t apply(const std::vector<ParticleFilter*>& filters = {}) {
    std::vector<tdr_filter*> handles;
    for (ParticleFilter* f : filters) {
      if (!f) throw std::invalid_argument("MapFuser::apply: null filter");
      handles.push_back(f->handle());
    }
    int64_t changed = 0;
    if (tdr_fuser_apply(f_, handles.empty() ? nullptr : handles.data(), (int)handles.size(), &changed) != TDR_OK)
      throw std::runtime_error(std::string("MapFuser::apply: ") + tdr_last_error());
    return changed;
  }
  void decay(int shift) { check(tdr_fuser_decay(f_, shift), "decay"); }
  void reset() { check(tdr_fuser_reset(f_), "reset"); }
  // after someone else replaced the map: its present label image becomes the base; true when the votes were kept
  bool rebase() {
    int kept = 0;
    check(tdr_fuser_rebase(f_, &kept), "rebase");
    return kept != 0;
  }
  // votes [ncls][rows][cols] (cell (yi, xi) at yi * cols + xi); labels [img_h][img_w], the fused image of the last apply
  std::vector<uint32_t> votes(int* ncls = nullptr, int* rows = nullptr, int* cols = nullptr) const {
    uint64_t st[9];
    check(tdr_fuser_stats(f_, st), "votes");
    std::vector<uint32_t> out((size_t)(st[4] * st[5] * st[6]));
    check(tdr_fuser_get_votes(f_, out.data()), "votes");
    if (ncls) *ncls = (int)st[4];
    if (rows) *rows = (int)st[5];
    if (cols) *cols = (int)st[6];
    return out;
  }
  std::vector<uint8_t> labels(int* img_h = nullptr, int* img_w = nullptr) const {
    uint64_t st[9];
    check(tdr_fuser_stats(f_, st), "labels");
    std::vector<uint8_t> out((size_t)(st[7] * st[8]));
    check(tdr_fuser_get_labels(f_, out.data()), "labels");
    if (img_h) *img_h = (int)st[7];
    if (img_w) *img_w = (int)st[8];
    return out;
  }
  tdr_fuser* handle() const { return f_; }

 private:
  static bool best(ParticleFilter& filter, Pose& p) {
    float s[4], c[16];
    if (tdr_filter_mean_cov(filter.handle(), 1, s, c) != TDR_OK) return false;   // no best particle before the first update
    p.x = s[0]; p.y = s[1]; p.theta = s[2]; p.scale = s[3];
    return true;
  }
  static bool soft_fail(const char* msg) {
    tdr_set_error(TDR_ERR_ARG, msg);
    return false;
  }
  static void check(int rc, const char* what) {
    if (rc != TDR_OK) throw std::runtime_error(std::string("MapFuser::") + what + ": " + tdr_last_error());
  }
  tdr_fuser* f_ = nullptr;
  uint64_t added_ = 0, dropped_ = 0;
};

#endif  // TDR_FACADE_MAP_FUSER_H_
