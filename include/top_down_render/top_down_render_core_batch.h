// top_down_render_core_batch.h — the node's per-scan loop (TopDownRenderCore::takeStep, top_down_render_core.h) for many
// robots on one map at once (extension; the reference runs one loop per node):
//
//   1. render every core's cloud at that core's current_range_scale_ into the core's own renderer: tdr_batch_render_polar
//   2. ParticleFilterBatch::step with the renders as inputs and the priors {trans, yaw}: tdr_batch_step
//   3. the pose statistics of all filters, one read-back: tdr_batch_pose (fills every filter's mean / covariance / scale
//      cache)
//   4. every core's own publishPoseEst() — it reads the cache, so it makes no device call except in the step in which a
//      filter's scale freezes
//   5. one ParticleFilterBatch::computeGMM for the cores whose mixture fit is due (Config::gmm_every): tdr_batch_compute_gmm;
//      one ParticleFilterBatch::kldCount for those whose KLD-sampling count is due (Config::kld_every): tdr_batch_kld_count
//   6. the recovery trackers of the cores whose recovery step is due (Config::recovery_every), one small read-back each,
//      and one ParticleFilterBatch::inject per heading mode for those whose tracker asks for an injection: tdr_batch_inject
//
// Every core ends where cores[i]->takeStep(...) with setDeviceScan(true) leaves it: filter states, weights and generator
// position, PoseEst, currentRangeScale, lastRes, isConverged.  One difference: the host topDown() images are not filled
// (the renders stay on the device; ScanRenderer::handle + tdr_renderer_get_render reads them, and renderPictures draws the
// robots' scan pictures and particle pictures from the device data in two batched calls).
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include "top_down_render/particle_filter_batch.h"
#include "top_down_render/top_down_render_core.h"

class TopDownRenderCoreBatch {
 public:
  // cores: on one map, with one (theta_bins, range_bins); clouds / trans / yaw: one per core.  stream: a hipStream_t
  // (nullptr = the default stream).  Returns false when the map holds no map yet (nothing moves, like takeStep); throws
  // before anything moves on a batch that does not fit, and on a refused call.
  bool takeStep(const std::vector<TopDownRenderCore*>& cores, const std::vector<pcl::PointCloud<PointType>::ConstPtr>& clouds,
                const std::vector<Eigen::Vector2f>& trans, const std::vector<float>& yaw,
                std::vector<TopDownRenderCore::PoseEst>* ests = nullptr, void* stream = nullptr) {
    const size_t k = cores.size();
    if (k < 1) throw std::invalid_argument("TopDownRenderCoreBatch::takeStep: no core");
    if (clouds.size() != k || trans.size() != k || yaw.size() != k)
      throw std::invalid_argument("TopDownRenderCoreBatch::takeStep: one cloud, translation and yaw per core");
    for (size_t i = 0; i < k; i++) {
      const TopDownRenderCore* c = cores[i];
      if (!c || !c->map_ || !c->filter_ || !c->renderer_)
        throw std::invalid_argument("TopDownRenderCoreBatch::takeStep: core " + std::to_string(i) + " is null or not initialised");
      if (c->cfg_.theta_bins != cores[0]->cfg_.theta_bins || c->cfg_.range_bins != cores[0]->cfg_.range_bins)
        throw std::invalid_argument("TopDownRenderCoreBatch::takeStep: core " + std::to_string(i) + " has " +
                                    std::to_string(c->cfg_.theta_bins) + " x " + std::to_string(c->cfg_.range_bins) +
                                    " bins, core 0 " + std::to_string(cores[0]->cfg_.theta_bins) + " x " +
                                    std::to_string(cores[0]->cfg_.range_bins));
      if (c->cfg_.recovery_every > 0 && c->cfg_.recovery_candidates > 1)
        throw std::invalid_argument("TopDownRenderCoreBatch::takeStep: core " + std::to_string(i) + " has recovery_candidates = " +
                                    std::to_string(c->cfg_.recovery_candidates) +
                                    ": sensor resetting is not built for a batch (tdr_batch_inject is the plain injection)");
      if (c->map_ != cores[0]->map_)
        throw std::invalid_argument("TopDownRenderCoreBatch::takeStep: core " + std::to_string(i) + " is on another map than core 0");
    }
    TopDownMapPolar* map = cores[0]->map_;
    if (!map->haveMap()) return false;                                                      // :508-511
    const int nb = cores[0]->cfg_.theta_bins, nr = cores[0]->cfg_.range_bins;
    const float ang_res = (float)(2 * M_PI / nb);

    std::vector<tdr_renderer*> rs(k);
    std::vector<tdr_batch_cloud> cl(k);
    std::vector<ParticleFilter*> filters(k);
    std::vector<const ScanRenderer*> renderers(k);
    std::vector<float> res(k);
    std::vector<MotionPrior> priors(k);
    for (size_t i = 0; i < k; i++) {
      TopDownRenderCore* c = cores[i];
      const pcl::PointCloud<PointType>::ConstPtr& cloud = clouds[i];
      rs[i] = c->renderer_->handle();
      cl[i] = tdr_batch_cloud{};
      cl[i].pts = cloud && !cloud->points.empty() ? reinterpret_cast<const float*>(cloud->points.data()) : nullptr;
      cl[i].n = cloud ? (int64_t)cloud->points.size() : 0;
      cl[i].stride = 8;   // pcl::PointXYZI: x y z pad intensity pad pad pad (as ScanRenderer::render)
      cl[i].ioff = 4;
      cl[i].res = c->current_range_scale_;                                                  // :539
      filters[i] = c->filter_;
      renderers[i] = c->renderer_;
      res[i] = c->current_range_scale_;
      priors[i].tx = trans[i][0];
      priors[i].ty = trans[i][1];
      priors[i].omega = yaw[i];
    }
    if (tdr_batch_render_polar(rs.data(), (int)k, cl.data(), ang_res, map->numClasses(), nb, nr, stream) != TDR_OK)
      throw std::runtime_error(std::string("TopDownRenderCoreBatch::takeStep: ") + tdr_last_error());
    batch_.step(filters, std::vector<std::vector<Eigen::ArrayXXf>>(k), res, priors, renderers, stream);   // :559
    std::vector<tdr_filter*> handles(k);
    for (size_t i = 0; i < k; i++) handles[i] = filters[i]->handle();
    std::vector<tdr_pose_stats> stats(k);
    if (tdr_batch_pose(handles.data(), (int)k, stats.data(), stream) != TDR_OK)
      throw std::runtime_error(std::string("TopDownRenderCoreBatch::takeStep: ") + tdr_last_error());
    if (ests) ests->resize(k);
    std::vector<ParticleFilter*> due;
    std::vector<size_t> kld_due;
    for (size_t i = 0; i < k; i++) {
      cores[i]->last_res_ = res[i];
      TopDownRenderCore::PoseEst e = cores[i]->publishPoseEst();                           // :560
      if (cores[i]->countStepAndGmmDue()) due.push_back(filters[i]);
      if (cores[i]->countStepAndKldDue()) kld_due.push_back(i);
      if (ests) (*ests)[i] = e;
    }
    batch_.computeGMM(due, stream);   // one mixture fit for the cores whose step is due (Config::gmm_every)
    // ... and one bin count for those whose KLD-sampling count is due (Config::kld_every): cores with equal parameters
    // share a tdr_batch_kld_count
    while (!kld_due.empty()) {
      const KldParams& p = cores[kld_due[0]]->cfg_.kld;
      std::vector<size_t> same, rest;
      for (size_t i : kld_due) (sameKldParams(p, cores[i]->cfg_.kld) ? same : rest).push_back(i);
      std::vector<ParticleFilter*> fs;
      for (size_t i : same) fs.push_back(filters[i]);
      std::vector<int64_t> targets;
      batch_.kldCount(fs, p, targets, nullptr, stream);
      for (size_t j = 0; j < same.size(); j++) filters[same[j]]->setTargetCount((int)targets[j]);
      kld_due.swap(rest);
    }
    // recovery: what ParticleFilter::recoveryStep does, the injections of one heading mode sharing a launch
    for (int mode = 0; mode < 2; mode++) {
      std::vector<ParticleFilter*> fs;
      std::vector<TopDownRenderCore*> cs;
      std::vector<double> ps;
      std::vector<uint64_t> seeds;
      for (size_t i = 0; i < k; i++) {
        TopDownRenderCore* c = cores[i];
        if (c->cfg_.recovery_every <= 0 || c->cfg_.recovery.heading_mode != mode) continue;
        if (!c->countStepAndRecoveryDue()) continue;
        float st8[8];
        filters[i]->weightStats(st8);
        tdr_recovery_state next = c->recovery_state_;
        const double p = tdr_recovery_track_host(&next, (double)st8[2], &c->cfg_.recovery);
        c->last_recovery_p_ = p;
        c->last_recovery_injected_ = 0;
        if (p > 0.) {
          fs.push_back(filters[i]);
          cs.push_back(c);
          ps.push_back(p);
          seeds.push_back(c->cfg_.recovery.seed);
          tdr_recovery_reset_host(&next);
        }
        c->recovery_state_ = next;
      }
      if (fs.empty()) continue;
      std::vector<int64_t> injected;
      batch_.inject(fs, ps, mode, seeds, &injected, stream);
      for (size_t j = 0; j < cs.size(); j++) cs[j]->last_recovery_injected_ = injected[j];
    }
    return true;
  }
  // The two per-scan pictures of every core after a takeStep (publishSemanticTopDown, :246-254, and the particle picture,
  // :430-449): tdr_batch_scan_pictures over the cores' renderers and ParticleFilterBatch::renderViz over their filters
  // (each over its own background, ParticleFilter::setVizBackground).  scan_pictures[i] is [range_bins][theta_bins] BGR.
  // arrows: empty, or one list per core.  Throws on a refused call; takeStep itself does not draw.
  void renderPictures(const std::vector<TopDownRenderCore*>& cores, const std::vector<int>& unflatten_lut,
                      const SemanticColorLut& lut, float pub_scale, const std::vector<std::vector<std::array<int, 4>>>& arrows,
                      std::vector<tdr_viz::Image>& scan_pictures, std::vector<tdr_viz::Image>& particle_pictures,
                      void* stream = nullptr) {
    const size_t k = cores.size();
    if (k < 1) throw std::invalid_argument("TopDownRenderCoreBatch::renderPictures: no core");
    std::vector<const tdr_renderer*> rs(k);
    std::vector<ParticleFilter*> filters(k);
    for (size_t i = 0; i < k; i++) {
      if (!cores[i] || !cores[i]->filter_ || !cores[i]->renderer_)
        throw std::invalid_argument("TopDownRenderCoreBatch::renderPictures: core " + std::to_string(i) + " is null or not initialised");
      rs[i] = static_cast<const ScanRenderer*>(cores[i]->renderer_)->handle();
      filters[i] = cores[i]->filter_;
    }
    int h = 0, w = 0;
    tdr_viz::rendererPictureSize(rs[0], h, w);   // (the batch call refuses renders of different shapes)
    const std::vector<int32_t> unf = tdr_viz::unflattenTable(unflatten_lut, cores[0]->map_->numClasses(), "renderPictures");
    const std::array<uint8_t, 768> table = tdr_viz::colourTable(lut);
    const size_t pic = (size_t)3 * h * w;
    std::vector<uint8_t> all(pic * k);
    if (tdr_batch_scan_pictures(rs.data(), (int)k, unf.data(), table.data(), all.data(), stream) != TDR_OK)
      throw std::runtime_error(std::string("TopDownRenderCoreBatch::renderPictures: ") + tdr_last_error());
    scan_pictures.resize(k);
    for (size_t i = 0; i < k; i++) {
      scan_pictures[i].h = h;
      scan_pictures[i].w = w;
      scan_pictures[i].bgr.assign(all.begin() + pic * i, all.begin() + pic * (i + 1));
    }
    batch_.renderViz(filters, pub_scale, arrows, particle_pictures, stream);
  }
  // Every core's cloud after a takeStep in ONE image over the background the cores' map holds
  // (TopDownMap::setVizBackground): ParticleFilterBatch::renderFleet over the cores' filters.  palette: one per core;
  // arrows: one list for the image.  Throws on a refused call.
  void renderFleetPicture(const std::vector<TopDownRenderCore*>& cores, float pub_scale,
                          const std::vector<tdr_viz::FleetColours>& palette, const std::vector<std::array<int, 4>>& arrows,
                          tdr_viz::Image& out, void* stream = nullptr) {
    batch_.renderFleet(coreFilters(cores, "renderFleetPicture"), pub_scale, palette, arrows, out, stream);
  }
  void renderFleetPicture(const std::vector<TopDownRenderCore*>& cores, float pub_scale,
                          const std::vector<tdr_viz::FleetColours>& palette, const std::vector<std::array<int, 4>>& arrows,
                          std::vector<uint8_t>& out, int& out_h, int& out_w, void* stream = nullptr) {
    batch_.renderFleet(coreFilters(cores, "renderFleetPicture"), pub_scale, palette, arrows, out, out_h, out_w, stream);
  }
  // filters of the last step that took the batched path / their standalone calls (ParticleFilterBatch)
  int lastBatched() const { return batch_.lastBatched(); }
  int lastStandalone() const { return batch_.lastStandalone(); }

 private:
  static std::vector<ParticleFilter*> coreFilters(const std::vector<TopDownRenderCore*>& cores, const char* who) {
    if (cores.empty()) throw std::invalid_argument(std::string("TopDownRenderCoreBatch::") + who + ": no core");
    std::vector<ParticleFilter*> filters(cores.size());
    for (size_t i = 0; i < cores.size(); i++) {
      if (!cores[i] || !cores[i]->filter_)
        throw std::invalid_argument(std::string("TopDownRenderCoreBatch::") + who + ": core " + std::to_string(i) +
                                    " is null or not initialised");
      filters[i] = cores[i]->filter_;
    }
    return filters;
  }
  ParticleFilterBatch batch_;
};
