// State / FilterParams — the reference's PODs (include/top_down_render/state_particle.h:9-38), unchanged — and
// StateParticle.
// Inside ParticleFilter the per-particle methods (propagate, computeWeight, src/state_particle.cpp:57-78,157-219) run
// batched on the GPU over a structure of arrays; ParticleFilter::states() returns the particles as `State`s.  The
// StateParticle class below keeps the reference's per-particle surface for code that holds single particles: it is a
// one-particle filter on the device (a launch per call — use ParticleFilter for throughput).
#ifndef STATE_PARTICLE_H_
#define STATE_PARTICLE_H_

#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "tdr.h"
#include "top_down_render/top_down_map_polar.h"

typedef struct State {
  float init_x_px = 0;
  float init_y_px = 0;
  float dx_m = 0;
  float dy_m = 0;
  float theta = 0;
  float scale = 1;  // px/m
  bool have_init = false;
} State;
static_assert(sizeof(State) == sizeof(tdr_state), "State must stay byte-compatible with tdr_state (28 bytes)");

typedef struct FilterParams {
  float pos_cov;
  float theta_cov;
  float regularization;
  float init_pos_px_x = -1;
  float init_pos_px_y = -1;
  float init_pos_px_cov = -1;

  float init_pos_m_x = -1;
  float init_pos_m_y = -1;
  float init_pos_deg_theta = -1;
  float init_pos_deg_cov = -1;

  bool force_on_map = false;
  float fixed_scale = -1;
  float scale_log_min = -0.1;
  float scale_log_max = 1;

  std::vector<float> class_weights;
} FilterParams;

// KLD-sampling count (extension; include/tdr.h, "KLD-sampling count"): the pose bins and Fox's bound, with AMCL's usual
// kld_err / kld_z.  ParticleFilter::kldCount, TopDownRenderCore::Config::kld.
struct KldParams : tdr_kld_params {
  KldParams() : tdr_kld_params{4.f, 36, 3, 0.05, 2.326, 100} {}
};
// Recovery injection (extension; include/tdr.h, "recovery injection"): the slow / fast averages of the updates' mean raw
// weight with AMCL's usual recovery_alpha_slow / recovery_alpha_fast, at most half the slots a step, particles without a
// heading.  ParticleFilter::recoveryStep, TopDownRenderCore::Config::recovery.
struct RecoveryParams : tdr_recovery_params {
  RecoveryParams() : tdr_recovery_params{0.001, 0.1, 0.5, 0, 0} {}
};
// Pose-grid search (extension; include/tdr.h, "pose-grid search"): a lattice of map cells without headings (the 40-rotation
// search gives each point one), road cells only, at scale 1; and what ParticleFilter::gridSearch returns: the planes W and
// T (ny rows of nx points; NaN where a point is not listed), vol (H planes, when asked for), the first peaks in the order
// (w descending, g ascending), the number of peaks and of listed points.
struct GridSpec : tdr_grid_spec {
  GridSpec() : tdr_grid_spec{0, 0, 1, 1, 1, 1, 0, 1, 0.f, 0.f, 1.f} {}
  GridSpec(int c0_, int r0_, int step_, int nx_, int ny_) : tdr_grid_spec{c0_, r0_, step_, nx_, ny_, 1, 0, 1, 0.f, 0.f, 1.f} {}
};
struct GridSearchResult {
  int nx = 0, ny = 0, n_headings = 0;
  std::vector<float> w, theta, vol;
  std::vector<tdr_grid_peak> peaks;
  int64_t n_peaks = 0, listed = 0;
};
// ParticleFilter::gridSearch and ParticleFilterCartesian::gridSearch: tdr_filter_grid_search into a GridSearchResult; the
// return code is the caller's to report
inline int gridSearchInto(tdr_filter* f, const tdr_renderer* renderer, float res, const tdr_grid_spec& spec, int nms_radius,
                          int max_peaks, bool with_vol, GridSearchResult& out) {
  const size_t G = spec.nx > 0 && spec.ny > 0 ? (size_t)spec.nx * (size_t)spec.ny : 0;
  const size_t H = spec.n_headings > 0 ? (size_t)spec.n_headings : 0;
  if (G <= ((size_t)1 << 24) && H <= 4096) {   // (a spec beyond its ranges is refused below, before anything is written)
    out.w.resize(G);
    out.theta.resize(G);
    if (with_vol) out.vol.resize(G * H);
  }
  out.peaks.resize(max_peaks > 0 && max_peaks <= 4096 ? (size_t)max_peaks : 0);
  const int rc = tdr_filter_grid_search(f, nullptr, renderer, res, &spec, out.w.data(), out.theta.data(),
                                        with_vol ? out.vol.data() : nullptr, nms_radius, max_peaks, out.peaks.data(), &out.n_peaks,
                                        &out.listed);
  if (rc != TDR_OK) return rc;
  out.nx = spec.nx;
  out.ny = spec.ny;
  out.n_headings = spec.n_headings;
  out.peaks.resize((size_t)(out.n_peaks < (int64_t)out.peaks.size() ? out.n_peaks : (int64_t)out.peaks.size()));
  return rc;
}
inline bool sameKldParams(const tdr_kld_params& a, const tdr_kld_params& b) {
  return a.bin_xy_px == b.bin_xy_px && a.theta_bins == b.theta_bins && a.scale_bits == b.scale_bits &&
         a.epsilon == b.epsilon && a.z == b.z && a.n_min == b.n_min;
}

inline tdr_filter_params to_tdr_params(const FilterParams& p, int num_classes) {
  tdr_filter_params c{};
  c.pos_cov = p.pos_cov; c.theta_cov = p.theta_cov; c.regularization = p.regularization;
  c.init_pos_px_x = p.init_pos_px_x; c.init_pos_px_y = p.init_pos_px_y; c.init_pos_px_cov = p.init_pos_px_cov;
  c.init_pos_m_x = p.init_pos_m_x; c.init_pos_m_y = p.init_pos_m_y;
  c.init_pos_deg_theta = p.init_pos_deg_theta; c.init_pos_deg_cov = p.init_pos_deg_cov;
  c.force_on_map = p.force_on_map ? 1 : 0;
  c.fixed_scale = p.fixed_scale; c.scale_log_min = p.scale_log_min; c.scale_log_max = p.scale_log_max;
  c.num_classes = num_classes;
  for (int i = 0; i < 16; i++) c.class_weights[i] = i < (int)p.class_weights.size() ? p.class_weights[i] : (i < num_classes ? 1.f : 0.f);
  return c;
}

// include/top_down_render/state_particle.h:40-66 in the reference.
class StateParticle {
 public:
  // src/state_particle.cpp:3-49: init == true draws the pose from the shared generator (rejection-sampled onto a
  // road cell), init == false leaves the default State.
  StateParticle(std::mt19937* gen, TopDownMapPolar* map, FilterParams* params, bool init = true)
      : map_(map), params_(params) {
    if (!gen || !map || !params) throw std::invalid_argument("StateParticle: null argument");
    tdr_filter_params c = to_tdr_params(*params_, map_->numClasses());
    if (tdr_filter_create(map_->handle(), 1, &c, /*seed (unused: the generator is shared)*/ 1, &f_) != TDR_OK) fail("StateParticle");
    try {
      check(tdr_filter_share_rng(f_, gen), "share_rng");
      check(tdr_filter_configure(f_, /*parity_rng=*/1, /*locality_every=*/0), "configure");
      if (init && map_->haveMap()) check(tdr_filter_init_one(f_), "init");
      else setState(State());
    } catch (...) {
      tdr_filter_destroy(f_);   // the destructor does not run for a constructor that throws
      throw;
    }
  }
  ~StateParticle() { tdr_filter_destroy(f_); }
  StateParticle(const StateParticle&) = delete;
  StateParticle& operator=(const StateParticle&) = delete;

  void propagate(Eigen::Vector2f& trans, float omega, bool scale_freeze = false) {   // :57-78
    check(tdr_filter_propagate_freeze(f_, trans[0], trans[1], omega, scale_freeze ? 1 : 0), "propagate");
  }
  State state() const {
    State s;
    check(tdr_filter_get_states(f_, reinterpret_cast<tdr_state*>(&s), 1), "state");
    return s;
  }
  Eigen::Vector4f mlState() const {                                                   // :98-102
    const State s = state();
    return Eigen::Vector4f(s.dx_m * s.scale + s.init_x_px, s.dy_m * s.scale + s.init_y_px, s.theta, s.scale);
  }
  void setState(const State& s) { check(tdr_filter_set_states(f_, reinterpret_cast<const tdr_state*>(&s), 1), "setState"); }
  // :157-219.  top_down_geo is accepted and ignored like in the reference's score (:145-152).
  void computeWeight(std::vector<Eigen::ArrayXXf>& top_down_scan, std::vector<Eigen::ArrayXXf>& /*top_down_geo*/, float res) {
    const int ncls = map_->numClasses();
    // (sizes it cannot use: a silent return like the reference's per-scan calls, the reason in tdr_last_error())
    if ((int)top_down_scan.size() < ncls) { tdr_set_error(TDR_ERR_ARG, "computeWeight: fewer scan images than map classes"); return; }
    const Eigen::Vector2i shape = map_->polarShape();
    const size_t P = (size_t)shape[0] * shape[1];
    for (int c = 0; c < ncls; c++)
      if (top_down_scan[c].rows() != shape[0] || top_down_scan[c].cols() != shape[1])
        { tdr_set_error(TDR_ERR_ARG, "computeWeight: scan image shape differs from the shape given to samplePtsPolar"); return; }
    std::vector<float> buf(P * ncls);
    for (int c = 0; c < ncls; c++) std::memcpy(buf.data() + P * c, top_down_scan[c].data(), P * sizeof(float));
    check(tdr_filter_compute_weights(f_, buf.data(), nullptr, res), "computeWeight");
  }
  float weight() const {                                                              // :55
    float w = 0;
    check(tdr_filter_get_raw_weights(f_, &w, 1), "weight");
    return w;
  }
  float lastDist() const {
    float d = 0;
    check(tdr_filter_get_last_dist(f_, &d, 1), "lastDist");
    return d;
  }
  void setScale(float scale) {                                                        // :104-106
    State s = state();
    s.scale = scale;
    setState(s);
  }
  void updateSize() {}   // :108-110 caches the map size in metres; here the gate reads the map at score time

 private:
  void check(int rc, const char* what) const { if (rc != TDR_OK) fail(what); }
  [[noreturn]] void fail(const char* what) const { throw std::runtime_error(std::string("StateParticle::") + what + ": " + tdr_last_error()); }
  TopDownMapPolar* map_;
  FilterParams* params_;
  tdr_filter* f_ = nullptr;
};

#endif  // STATE_PARTICLE_H_
