// particle_filter_batch.h — many ParticleFilters that share one TopDownMapPolar stepped together (extension; the reference
// steps one filter per node).  step() = propagate(priors[k]) + update(scans[k], res[k]) of every filter, through
// tdr_batch_step (include/tdr.h): one launch per stage for the filters that qualify, their standalone calls for the
// others, every filter ending bit for bit where those two calls would leave it.
#pragma once

#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "top_down_render/particle_filter.h"

struct MotionPrior {   // the arguments of ParticleFilter::propagate
  float tx = 0.f, ty = 0.f, omega = 0.f;
};

class ParticleFilterBatch {
 public:
  // scans[k]: the filter's per-class images (the shape given to samplePtsPolar), or empty with renderers[k] set.  res: one
  // value per filter.  stream: a hipStream_t (nullptr = the default stream).  Throws on a refused batch.
  void step(const std::vector<ParticleFilter*>& filters, const std::vector<std::vector<Eigen::ArrayXXf>>& scans,
            const std::vector<float>& res, const std::vector<MotionPrior>& priors,
            const std::vector<const ScanRenderer*>& renderers = {}, void* stream = nullptr) {
    const size_t k = filters.size();
    if (scans.size() != k || res.size() != k || priors.size() != k || (!renderers.empty() && renderers.size() != k))
      throw std::invalid_argument("ParticleFilterBatch::step: one scan, res and prior per filter");
    std::vector<tdr_filter*> handles(k, nullptr);
    std::vector<tdr_batch_input> in(k);
    std::vector<std::vector<float>> bufs(k);
    for (size_t i = 0; i < k; i++) {
      if (!filters[i]) throw std::invalid_argument("ParticleFilterBatch::step: null filter");
      handles[i] = filters[i]->handle();
      in[i] = tdr_batch_input{};
      in[i].res = res[i];
      in[i].tx = priors[i].tx;
      in[i].ty = priors[i].ty;
      in[i].omega = priors[i].omega;
      in[i].n_target = filters[i]->nextCount();
      if (!scans[i].empty()) {
        // the images must have the map's class count and samplePtsPolar's shape (tdr_batch_step reads ncls * nb * nr
        // floats): like ParticleFilter::update, but a batch refuses instead of skipping one filter
        const TopDownMapPolar* m = filters[i]->map();
        const int ncls = m->numClasses();
        const Eigen::Vector2i shape = m->polarShape();
        if ((int)scans[i].size() < ncls)
          throw std::invalid_argument("ParticleFilterBatch::step: scan " + std::to_string(i) + " has " +
                                      std::to_string(scans[i].size()) + " images, the map " + std::to_string(ncls) + " classes");
        const size_t P = (size_t)shape[0] * shape[1];
        for (int c = 0; c < ncls; c++)
          if (scans[i][c].rows() != shape[0] || scans[i][c].cols() != shape[1])
            throw std::invalid_argument("ParticleFilterBatch::step: scan " + std::to_string(i) + " image " + std::to_string(c) +
                                        " is " + std::to_string(scans[i][c].rows()) + "x" + std::to_string(scans[i][c].cols()) +
                                        ", samplePtsPolar was given " + std::to_string(shape[0]) + "x" + std::to_string(shape[1]));
        bufs[i].resize(P * ncls);
        for (int c = 0; c < ncls; c++) std::memcpy(bufs[i].data() + P * c, scans[i][c].data(), P * sizeof(float));
        in[i].scan_imgs = bufs[i].data();
      } else if (!renderers.empty() && renderers[i]) {
        in[i].renderer = renderers[i]->handle();
      }
    }
    if (tdr_batch_step(handles.data(), (int)k, in.data(), stream) != TDR_OK)
      throw std::runtime_error(std::string("ParticleFilterBatch::step: ") + tdr_last_error());
    tdr_batch_last_stats(&batched_, &standalone_);
  }
  // computeGMMDevice() of every filter through tdr_batch_compute_gmm: the samples, every candidate fit and the picks are
  // one launch each, with one read-back for the batch.  The filters need not share a map.  Throws on a refused batch
  // (a null or repeated filter, a sharded one) before any filter changes.
  void computeGMM(const std::vector<ParticleFilter*>& filters, void* stream = nullptr) {
    if (filters.empty()) return;
    std::vector<tdr_filter*> handles(filters.size(), nullptr);
    for (size_t i = 0; i < filters.size(); i++) {
      if (!filters[i]) throw std::invalid_argument("ParticleFilterBatch::computeGMM: null filter");
      handles[i] = filters[i]->handle();
    }
    if (tdr_batch_compute_gmm(handles.data(), (int)handles.size(), stream) != TDR_OK)
      throw std::runtime_error(std::string("ParticleFilterBatch::computeGMM: ") + tdr_last_error());
  }
  // kldCount(p) of every filter through tdr_batch_kld_count: one job upload, one fill, one launch and one read-back for
  // the batch; targets[i] (and bins[i], when asked for) are what filters[i]->kldCount(p, &k) returns.  The filters need not
  // share a map.  Throws on a refused batch (bad parameters, a null or repeated filter, a sharded one); no filter changes.
  void kldCount(const std::vector<ParticleFilter*>& filters, const KldParams& p, std::vector<int64_t>& targets,
                std::vector<int64_t>* bins = nullptr, void* stream = nullptr) {
    targets.assign(filters.size(), 0);
    if (bins) bins->assign(filters.size(), 0);
    if (filters.empty()) return;
    std::vector<tdr_filter*> handles(filters.size(), nullptr);
    for (size_t i = 0; i < filters.size(); i++) {
      if (!filters[i]) throw std::invalid_argument("ParticleFilterBatch::kldCount: null filter");
      handles[i] = filters[i]->handle();
    }
    if (tdr_batch_kld_count(handles.data(), (int)handles.size(), &p, bins ? bins->data() : nullptr, nullptr, targets.data(),
                            stream) != TDR_OK)
      throw std::runtime_error(std::string("ParticleFilterBatch::kldCount: ") + tdr_last_error());
  }
  // inject(p[i], heading_mode, seeds[i]) of every filter through tdr_batch_inject: one job upload, one launch and one
  // read-back for the batch; each filter ends byte for byte where its own call leaves it.  The filters need not share a
  // map.  injected: the slots replaced per filter, or nullptr (no read-back, no wait).  Throws on a refused batch.
  void inject(const std::vector<ParticleFilter*>& filters, const std::vector<double>& p, int heading_mode,
              const std::vector<uint64_t>& seeds, std::vector<int64_t>* injected = nullptr, void* stream = nullptr) {
    if (injected) injected->assign(filters.size(), 0);
    if (p.size() != filters.size() || seeds.size() != filters.size())
      throw std::invalid_argument("ParticleFilterBatch::inject: one probability and one seed per filter");
    if (filters.empty()) return;
    std::vector<tdr_filter*> handles(filters.size(), nullptr);
    for (size_t i = 0; i < filters.size(); i++) {
      if (!filters[i]) throw std::invalid_argument("ParticleFilterBatch::inject: null filter");
      handles[i] = filters[i]->handle();
    }
    if (tdr_batch_inject(handles.data(), (int)handles.size(), p.data(), heading_mode, seeds.data(),
                         injected ? injected->data() : nullptr, stream) != TDR_OK)
      throw std::runtime_error(std::string("ParticleFilterBatch::inject: ") + tdr_last_error());
  }
  // renderViz(out, h, w, pub_scale, arrows[k]) of every filter through tdr_batch_visualize: one launch per stage, one
  // read-back and one wait for the batch, each filter over its own background.  arrows: empty, or one list per filter.
  // Throws on a refused batch (a null or repeated filter, a sharded one, one without a background) before any device work.
  void renderViz(const std::vector<ParticleFilter*>& filters, float pub_scale,
                 const std::vector<std::vector<std::array<int, 4>>>& arrows, std::vector<tdr_viz::Image>& outs,
                 void* stream = nullptr) {
    std::vector<tdr_filter*> handles(filters.size(), nullptr);
    for (size_t i = 0; i < filters.size(); i++) {
      if (!filters[i]) throw std::invalid_argument("ParticleFilterBatch::renderViz: null filter");
      handles[i] = filters[i]->handle();
    }
    tdr_viz::renderBatch(handles, pub_scale, arrows, outs, stream);
  }
  // The fleet picture (include/tdr.h): every filter's cloud in ONE image over the background their map holds
  // (TopDownMap::setVizBackground), palette[i] the colours of filter i, arrows one list for the image; one launch per stage,
  // one read-back and one wait.  Throws on a refused call (filters on different maps, a map without a background, more
  // than TDR_FLEET_MAX filters, a null, repeated or sharded filter) before any device work.
  void renderFleet(const std::vector<ParticleFilter*>& filters, float pub_scale,
                   const std::vector<tdr_viz::FleetColours>& palette, const std::vector<std::array<int, 4>>& arrows,
                   tdr_viz::Image& out, void* stream = nullptr) {
    std::vector<tdr_filter*> handles(filters.size(), nullptr);
    for (size_t i = 0; i < filters.size(); i++) {
      if (!filters[i]) throw std::invalid_argument("ParticleFilterBatch::renderFleet: null filter");
      handles[i] = filters[i]->handle();
    }
    tdr_viz::renderFleet(handles, pub_scale, palette, arrows, out, stream);
  }
  void renderFleet(const std::vector<ParticleFilter*>& filters, float pub_scale,
                   const std::vector<tdr_viz::FleetColours>& palette, const std::vector<std::array<int, 4>>& arrows,
                   std::vector<uint8_t>& out, int& out_h, int& out_w, void* stream = nullptr) {
    tdr_viz::Image img;
    renderFleet(filters, pub_scale, palette, arrows, img, stream);
    out.swap(img.bgr);
    out_h = img.h;
    out_w = img.w;
  }
  // tdr_config_tuning("batch_init_search"), process-wide: with true a filter that may still hold a particle without a
  // heading — a cold start (init_pos_deg_theta = inf), a gated filter (force_on_map, unknown scale) — joins the batch, its
  // 40-rotation search part of the batch's scoring stage, same bits; false (the default): its standalone calls inside step()
  static void setInitSearchInBatch(bool on) { tdr_config_tuning("batch_init_search", on ? 1 : 0); }
  static bool initSearchInBatch() { return tdr_config_tuning("batch_init_search", -1) == 1; }
  // filters of the last step that took the batched path / their standalone calls
  int lastBatched() const { return batched_; }
  int lastStandalone() const { return standalone_; }

 private:
  int batched_ = 0, standalone_ = 0;
};
