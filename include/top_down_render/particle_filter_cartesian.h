// ParticleFilterCartesian — a ParticleFilter over a Cartesian TopDownMap (tdr_filter_create_cart, include/tdr.h): the
// particles are scored against the rotated rectangular window of TopDownMap::getLocalMap (BASELINE config 4) instead of
// the polar table.  The reference has no such class: its StateParticle only reaches the polar overloads
// (state_particle.h:61).  The method names and argument meanings are ParticleFilter's.
//
// A class of its own rather than a constructor overload of ParticleFilter: that class keeps a TopDownMapPolar* (map(),
// which ParticleFilterBatch reads, and update()'s check against polarShape()), an overload taking the base class would make
// `ParticleFilter(N, nullptr, ...)` ambiguous, and what a Cartesian filter refuses — the geometric cost, batches, sharding —
// is simply absent here instead of failing at run time.
#ifndef PARTICLE_FILTER_CARTESIAN_H_
#define PARTICLE_FILTER_CARTESIAN_H_

#include <stdexcept>
#include <string>
#include <vector>

#include "top_down_render/particle_viz_device.h"
#include "top_down_render/scan_viz_device.h"
#include "top_down_render/scan_renderer.h"
#include "top_down_render/state_particle.h"
#include "top_down_render/top_down_map.h"

class ParticleFilterCartesian {
 public:
  // map: a TopDownMap whose window is set (TopDownMap::setWindow); seed as ParticleFilter's
  ParticleFilterCartesian(int N, TopDownMap* map, FilterParams& params, uint32_t seed = 0) : map_(map), params_(params) {
    if (!map) throw std::invalid_argument("ParticleFilterCartesian: null map");
    tdr_filter_params c = to_tdr_params(params_, map_->numClasses());
    if (tdr_filter_create_cart(map_->handle(), N, &c, seed, &f_) != TDR_OK) fail("ParticleFilterCartesian");
    if (map_->haveMap() && tdr_filter_initialize_particles(f_) != TDR_OK) {   // particle_filter.cpp:14-16
      const std::string msg = std::string("initializeParticles: ") + tdr_last_error();
      tdr_filter_destroy(f_);   // the destructor does not run for a constructor that throws
      throw std::runtime_error(msg);
    }
  }
  ~ParticleFilterCartesian() { tdr_filter_destroy(f_); }
  ParticleFilterCartesian(const ParticleFilterCartesian&) = delete;
  ParticleFilterCartesian& operator=(const ParticleFilterCartesian&) = delete;

  void propagate(Eigen::Vector2f& trans, float omega) { check(tdr_filter_propagate(f_, trans[0], trans[1], omega), "propagate"); }
  // top_down_scan: one image of the window's shape per class (ScanRenderer::renderSemanticTopDown's output).  The first
  // update of a cold-started filter chooses every particle's heading among the reference's 40 candidates first.  Wrong
  // sizes: nothing is scored, the reason is left in tdr_last_error() (like ParticleFilter::update).
  void update(std::vector<Eigen::ArrayXXf>& top_down_scan, float res) {
    std::vector<float> buf;
    if (pack(top_down_scan, buf)) check(tdr_filter_update(f_, buf.data(), nullptr, res, target_count_), "update");
  }
  // ... against the renderer's last (Cartesian) render, without copying the images through the host
  void update(const ScanRenderer& renderer, float res) {
    check(tdr_filter_update(f_, nullptr, renderer.handle(), res, target_count_), "update");
  }
  // StateParticle::computeWeight for every particle: raw weights only (rawWeights), no statistics, no resampling
  void computeWeight(std::vector<Eigen::ArrayXXf>& top_down_scan, float res) {
    std::vector<float> buf;
    if (pack(top_down_scan, buf)) check(tdr_filter_compute_weights(f_, buf.data(), nullptr, res), "computeWeight");
  }
  void computeWeight(const ScanRenderer& renderer, float res) {
    check(tdr_filter_compute_weights(f_, nullptr, renderer.handle(), res), "computeWeight");
  }
  void computeCov(Eigen::Matrix4f& cov) { stat(1, nullptr, &cov); }
  void maxLikelihood(Eigen::Vector4f& state) { stat(1, &state, nullptr); }
  void computeMeanCov(Eigen::Matrix4f& cov) { stat(0, nullptr, &cov); }
  void meanLikelihood(Eigen::Vector4f& state) { stat(0, &state, nullptr); }
  void freezeScale() { check(tdr_filter_freeze_scale(f_), "freezeScale"); }
  bool isScaleFrozen() { return tdr_filter_is_scale_frozen(f_) != 0; }
  float scale() const { return tdr_filter_scale(f_); }
  int numParticles() const { return (int)tdr_filter_num_particles(f_); }
  void computeGMM() { check(tdr_filter_compute_gmm(f_), "computeGMM"); }
  void computeGMMDevice() { check(tdr_filter_compute_gmm_device(f_), "computeGMMDevice"); }   // the fit as HIP kernels
  void setTargetCount(int n) { target_count_ = n; }
  // KLD-sampling count (ParticleFilter::kldCount): the count the pose bins of the current set ask for; *k: the bins
  int64_t kldCount(const KldParams& p, int64_t* k = nullptr) {
    int64_t target = 0;
    check(tdr_filter_kld_count(f_, &p, k, nullptr, &target), "kldCount");
    return target;
  }
  // Recovery injection (extension; include/tdr.h, "recovery injection"): every slot whose Philox word falls below
  // floor(p * 2^24) becomes a fresh particle on a road cell of the map (tdr_filter_inject); draw = the update count.
  // heading_mode 0: no heading, the next update's 40-rotation search gives one; 1: a uniform heading.  Returns the
  // injected slots (count = false: no read-back and no wait, returns -1).  Weights, their statistics, the generator and
  // the step count stay as they were.  Throws on bad arguments, an empty or sharded filter and a map without road.
  int64_t inject(double p, int heading_mode = 0, uint64_t seed = 0, bool count = true) {
    int64_t injected = -1;
    check(tdr_filter_inject(f_, p, heading_mode, seed, count ? &injected : nullptr), "inject");
    return injected;
  }
  // ... driven by the slow / fast averages of the last update's mean raw weight (tdr_filter_recovery_step): returns the
  // probability the tracker gave; *injected: the slots replaced
  double recoveryStep(tdr_recovery_state& state, const RecoveryParams& rp, int64_t* injected = nullptr) {
    double p = 0.;
    int64_t n = 0;
    check(tdr_filter_recovery_step(f_, &state, &rp, &p, &n), "recoveryStep");
    if (injected) *injected = n;
    return p;
  }
  // Sensor resetting (ParticleFilter::injectSensor / recoveryStepSensor; include/tdr.h, "sensor resetting"): the injected
  // slots take the best-scoring of `candidates` road candidates against the renderer's last Cartesian render (nullptr: the
  // scan the filter kept); heading_mode 0 runs the heading search on the candidates
  int64_t injectSensor(const ScanRenderer* renderer, float res, double p, int candidates, int heading_mode = 0,
                       uint64_t seed = 0, bool count = true) {
    int64_t injected = -1;
    check(tdr_filter_inject_sensor(f_, nullptr, renderer ? renderer->handle() : nullptr, res, p, candidates, heading_mode, seed,
                                   count ? &injected : nullptr), "injectSensor");
    return injected;
  }
  double recoveryStepSensor(tdr_recovery_state& state, const RecoveryParams& rp, int candidates, const ScanRenderer* renderer,
                            float res, int64_t* injected = nullptr) {
    double p = 0.;
    int64_t n = 0;
    check(tdr_filter_recovery_step_sensor(f_, &state, &rp, candidates, nullptr, renderer ? renderer->handle() : nullptr, res, &p,
                                          &n), "recoveryStepSensor");
    if (injected) *injected = n;
    return p;
  }
  // {argmax bits, sum, mean, bottom_stddev, fallback, num_valid, num_under, 0} of the last update (particle_filter.cpp:107-147)
  void weightStats(float out8[8]) { check(tdr_filter_get_weight_stats(f_, out8), "weightStats"); }
  // Pose-grid search (extension; include/tdr.h, "pose-grid search"): the renderer's last render (nullptr: the scan the
  // filter kept) scored over the lattice of `spec` as a particle of this filter would be scored, and the peaks of the
  // weight plane within nms_radius lattice points, the best max_peaks of them in order (tdr_filter_grid_search).  The
  // filter is read, not changed.  Throws on a spec outside its ranges, nms_radius outside 0 .. 16, max_peaks outside
  // 0 .. 4096, a res that is not finite and positive, an empty or sharded filter, and without a scan.
  GridSearchResult gridSearch(const ScanRenderer* renderer, float res, const tdr_grid_spec& spec, int nms_radius = 2,
                              int max_peaks = 8, bool with_vol = false) {
    GridSearchResult out;
    check(gridSearchInto(f_, renderer ? renderer->handle() : nullptr, res, spec, nms_radius, max_peaks, with_vol, out), "gridSearch");
    return out;
  }
  // ... and what turns its peaks into particles: inject() with the caller's cell list (r * cols + c; duplicates weight the
  // draw) in place of the map's road list (tdr_filter_inject_cells)
  int64_t injectCells(const std::vector<uint32_t>& cells, double p, int heading_mode = 0, uint64_t seed = 0, bool count = true) {
    int64_t injected = -1;
    check(tdr_filter_inject_cells(f_, cells.data(), (int64_t)cells.size(), p, heading_mode, seed, count ? &injected : nullptr),
          "injectCells");
    return injected;
  }
  void configure(bool parity_rng, int locality_every) { check(tdr_filter_configure(f_, parity_rng, locality_every), "configure"); }
  void updateMap(const uint8_t* label_img, int img_h, int img_w, const std::vector<int>& flatten_lut,
                 const Eigen::Vector2i& map_center) {
    std::vector<int32_t> lut(flatten_lut.begin(), flatten_lut.end());
    check(tdr_filter_update_map_labels(f_, label_img, img_h, img_w, lut.data(), (int)lut.size(), map_->numClasses(),
                                       map_->resolution(), map_center[0], map_center[1]), "updateMap");
  }
  // The picture drawn on the device (include/tdr.h, "the particle picture"; a definition, parity unpinned): the background
  // is uploaded once (it changes only with the map), renderViz returns the image the node publishes — particles, mixture,
  // best particle, the caller's arrows (the node's ground-truth arrow, :434-439), resized by pub_scale (:442-444).  The
  // vector overload returns the bytes [out_h][out_w][3].
  template <class MatT = cv::Mat>
  void setVizBackground(const MatT& bgr) { tdr_viz::setBackground(f_, bgr); }
  // ... from the label image the node colours (aerialMapCallback, :584): one byte a cell goes up, lut colours it on the device
  template <class MatT = cv::Mat>
  void setVizBackground(const MatT& labels, const SemanticColorLut& lut) { tdr_viz::setBackgroundLabels(f_, labels, lut); }
  template <class MatT = cv::Mat>
  void renderViz(MatT& out, float pub_scale, const std::vector<std::array<int, 4>>& arrows = {}) {
    tdr_viz::render(f_, out, pub_scale, arrows);
  }
  void renderViz(std::vector<uint8_t>& out, int& out_h, int& out_w, float pub_scale,
                 const std::vector<std::array<int, 4>>& arrows = {}) {
    tdr_viz::render(f_, out, out_h, out_w, pub_scale, arrows);
  }
  tdr_filter* handle() const { return f_; }
  TopDownMap* map() const { return map_; }
  void setStates(const std::vector<State>& s) {
    check(tdr_filter_set_states(f_, reinterpret_cast<const tdr_state*>(s.data()), (int64_t)s.size()), "setStates");
  }
  std::vector<State> states() {
    std::vector<State> s((size_t)tdr_filter_num_local(f_));
    if (!s.empty()) check(tdr_filter_get_states(f_, reinterpret_cast<tdr_state*>(s.data()), (int64_t)s.size()), "states");
    return s;
  }
  std::vector<float> weights(int n) {
    std::vector<float> w((size_t)n);
    if (n > 0) check(tdr_filter_get_weights(f_, w.data(), n), "weights");
    return w;
  }
  std::vector<float> rawWeights(int n) {
    std::vector<float> w((size_t)n);
    if (n > 0) check(tdr_filter_get_raw_weights(f_, w.data(), n), "rawWeights");
    return w;
  }
  std::vector<int32_t> resampleIndices() {
    std::vector<int32_t> idx((size_t)tdr_filter_num_local(f_));
    if (!idx.empty()) check(tdr_filter_get_resample_indices(f_, idx.data(), (int64_t)idx.size()), "resampleIndices");
    return idx;
  }

 private:
  // the images as one [ncls][rows*cols] array; false (and the reason in tdr_last_error()) when they cannot be used
  bool pack(const std::vector<Eigen::ArrayXXf>& scan, std::vector<float>& buf) {
    if (scan.empty() || numParticles() == 0) return false;
    const int ncls = map_->numClasses();
    const Eigen::Vector2i shape = map_->windowShape();
    if ((int)scan.size() < ncls) return tdr_set_error(TDR_ERR_ARG, "update: fewer scan images than map classes"), false;
    const size_t P = (size_t)shape[0] * shape[1];
    for (int c = 0; c < ncls; c++)
      if (scan[c].rows() != shape[0] || scan[c].cols() != shape[1])
        return tdr_set_error(TDR_ERR_ARG, "update: a scan image does not have the shape given to setWindow"), false;
    buf.resize(P * ncls);
    for (int c = 0; c < ncls; c++) std::memcpy(buf.data() + P * c, scan[c].data(), P * sizeof(float));
    return true;
  }
  void stat(int about_max, Eigen::Vector4f* state, Eigen::Matrix4f* cov) {
    float s[4], c[16];
    check(tdr_filter_mean_cov(f_, about_max, s, c), "statistics");
    if (state) for (int i = 0; i < 4; i++) (*state)[i] = s[i];
    if (cov) for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) (*cov)(i, j) = c[4 * i + j];
  }
  void check(int rc, const char* what) { if (rc != TDR_OK) fail(what); }
  [[noreturn]] void fail(const char* what) { throw std::runtime_error(std::string(what) + ": " + tdr_last_error()); }

  int target_count_ = -1;
  TopDownMap* map_;
  FilterParams params_;
  tdr_filter* f_ = nullptr;
};

#endif  // PARTICLE_FILTER_CARTESIAN_H_
