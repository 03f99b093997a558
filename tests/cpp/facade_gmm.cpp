// facade_gmm.cpp — the adaptive particle count in the node loop (TopDownRenderCore::Config::gmm_every,
// TopDownRenderCoreBatch; include/top_down_render/top_down_render_core.h): the mixture fit runs on the device
// (ParticleFilter::computeGMMDevice, ParticleFilterBatch::computeGMM) after the publishPoseEst of every gmm_every-th step,
// and every update resamples to the count of src/particle_filter.cpp:151-157.
//
//   A  gmm_every = 0 against a core whose Config never names the field: every step the same bits.
//   B  gmm_every = 2, <conv steps> steps: from the first fit on, numParticles() after a step is
//      tdr_adaptive_count_host(the stored clusters' covariances, the count before the step, particle_count); the first fit
//      follows step 2; the pose estimate before and after and the max-likelihood particle are printed for the caller's
//      convergence check.
//   C  TopDownRenderCoreBatch over three cores with gmm_every = 0, 2, 3 against three standalone cores: states, counts,
//      stored mixtures and PoseEst the same bits after every step; tdr_batch_last_stats is what the step left.
// Inputs: raw little-endian files in argv[1] (tests/test_gmm_device.py).  Prints "count <step> <n>" per step of B,
// "pose <x> <y> <theta> <cov00> <cov11>" before and after B, "ml <x> <y>" after B, "stats <step> <batched> <standalone>" per step of C, then "ok".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

#include "top_down_render/top_down_render_core_batch.h"

template <class T>
static std::vector<T> slurp(const std::string& path) {
  std::ifstream in(path, std::ios::binary | std::ios::ate);
  if (!in) throw std::runtime_error("cannot open " + path);
  std::vector<T> v((size_t)in.tellg() / sizeof(T));
  in.seekg(0);
  in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
  return v;
}

static bool same_est(TopDownRenderCore::PoseEst a, TopDownRenderCore::PoseEst b) {
  auto bits = [](const float* x, const float* y, size_t n) { return std::memcmp(x, y, n * sizeof(float)) == 0; };
  return bits(a.cov.data(), b.cov.data(), 16) && a.have_ml == b.have_ml && (!a.have_ml || bits(a.ml_state.data(), b.ml_state.data(), 4)) &&
         bits(&a.scale, &b.scale, 1) && bits(&a.range_scale, &b.range_scale, 1) && a.froze_scale == b.froze_scale &&
         a.converged == b.converged;
}

// the stored mixture as tdr_filter_get_gmm returns it: {k, means[k][3], covs[k][9]}
static std::vector<float> mixture(ParticleFilter* f) {
  float m[3 * TDR_GMM_MAX_K], c[9 * TDR_GMM_MAX_K];
  int k = 0;
  if (tdr_filter_get_gmm(f->handle(), TDR_GMM_MAX_K, &k, m, c) != TDR_OK) throw std::runtime_error(tdr_last_error());
  std::vector<float> out{(float)k};
  out.insert(out.end(), m, m + 3 * k);
  out.insert(out.end(), c, c + 9 * k);
  return out;
}

static void same_filters(ParticleFilter* a, ParticleFilter* b, const std::string& where) {
  const auto sa = a->states(), sb = b->states();
  if (sa.size() != sb.size() || std::memcmp(sa.data(), sb.data(), sa.size() * sizeof(State)) != 0)
    throw std::runtime_error(where + ": particle states differ");
  const auto ma = mixture(a), mb = mixture(b);
  if (ma.size() != mb.size() || std::memcmp(ma.data(), mb.data(), ma.size() * sizeof(float)) != 0)
    throw std::runtime_error(where + ": stored mixtures differ");
  if (tdr_filter_num_gaussians(a->handle()) != tdr_filter_num_gaussians(b->handle()))
    throw std::runtime_error(where + ": cluster counts differ");
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  try {
    int ncls, rows, cols, nb, nr, steps, conv_steps;
    float map_resolution;
    {
      std::ifstream meta(dir + "/meta.txt");
      meta >> ncls >> rows >> cols >> nb >> nr >> steps >> conv_steps >> map_resolution;
      if (!meta) throw std::runtime_error("bad meta.txt");
    }
    auto maps = slurp<float>(dir + "/maps.bin");
    auto mask = slurp<uint8_t>(dir + "/mask.bin");
    auto motion = slurp<float>(dir + "/motion.bin");    // {tx, ty, yaw}
    auto pts = slurp<float>(dir + "/pts.bin");          // [n][8]: pcl::PointXYZI layout

    TopDownMap::Params map_params;
    map_params.num_classes = ncls;
    map_params.resolution = map_resolution;
    for (int c = 0; c < ncls; c++) map_params.flatten_lut.push_back(c);
    TopDownMapPolar map(map_params);
    {
      std::vector<Eigen::ArrayXXf> class_maps;
      for (int c = 0; c < ncls; c++) {
        Eigen::ArrayXXf m(rows, cols);
        std::memcpy(m.data(), maps.data() + (size_t)c * rows * cols, (size_t)rows * cols * sizeof(float));
        class_maps.push_back(m);
      }
      Eigen::ArrayXXc class_mask(rows, cols);
      std::memcpy(class_mask.data(), mask.data(), (size_t)rows * cols);
      map.setDistanceMaps(class_maps, class_mask);
    }
    FilterParams filter_params;
    filter_params.pos_cov = 0.3f;
    filter_params.theta_cov = (float)(M_PI / 100);
    filter_params.regularization = 0.15f;
    filter_params.fixed_scale = 1.f;
    for (int c = 0; c < ncls; c++) filter_params.class_weights.push_back(1.f);
    filter_params.init_pos_m_x = 1e9f;   // initializeParticles returns early: the test brings its own particle sets
    filter_params.init_pos_m_y = 1e9f;
    Eigen::VectorXi flatten_lut = Eigen::VectorXi::Constant(256, -1);
    for (int c = 0; c < ncls; c++) flatten_lut[c] = c;

    pcl::PointCloud<PointType>::Ptr cloud_w(new pcl::PointCloud<PointType>());
    for (size_t i = 0; i < pts.size() / 8; i++) {
      PointType p{};
      p.x = pts[8 * i]; p.y = pts[8 * i + 1]; p.z = pts[8 * i + 2]; p.intensity = pts[8 * i + 4];
      cloud_w->push_back(p);
    }
    pcl::PointCloud<PointType>::ConstPtr cloud = cloud_w;
    Eigen::Vector2f trans(motion[0], motion[1]);
    const float yaw = motion[2];

    auto base_config = [&](int particles, uint32_t seed) {
      TopDownRenderCore::Config cfg;   // (gmm_every is not named here)
      cfg.particle_count = particles;
      cfg.theta_bins = nb;
      cfg.range_bins = nr;
      cfg.seed = seed;
      return cfg;
    };
    auto make_core = [&](const TopDownRenderCore::Config& cfg, const std::vector<State>& st) {
      auto* core = new TopDownRenderCore(cfg);
      core->initialize(&map, filter_params, flatten_lut);
      core->setDeviceScan(true);
      core->filter()->setStates(st);
      return core;
    };
    auto st0 = slurp<State>(dir + "/states_0.bin");

    // ---- A: gmm_every = 0 is a core built without the field
    {
      TopDownRenderCore::Config off = base_config((int)st0.size(), 7);
      off.gmm_every = 0;
      TopDownRenderCore *a = make_core(base_config((int)st0.size(), 7), st0), *b = make_core(off, st0);
      for (int k = 0; k < steps; k++) {
        TopDownRenderCore::PoseEst ea, eb;
        a->takeStep(cloud, trans, yaw, &ea);
        b->takeStep(cloud, trans, yaw, &eb);
        if (!same_est(ea, eb)) throw std::runtime_error("A step " + std::to_string(k) + ": PoseEst differs");
        same_filters(a->filter(), b->filter(), "A step " + std::to_string(k));
        if (a->filter()->numParticles() != (int)st0.size() || mixture(b->filter()).size() != 1)
          throw std::runtime_error("A: gmm_every = 0 changed the particle count or fitted a mixture");
      }
      delete a;
      delete b;
    }

    // ---- B: gmm_every = 2
    {
      TopDownRenderCore::Config cfg = base_config((int)st0.size(), 7);
      cfg.gmm_every = 2;
      TopDownRenderCore* c = make_core(cfg, st0);
      Eigen::Vector4f mean;
      Eigen::Matrix4f cov;
      c->filter()->meanLikelihood(mean);
      c->filter()->computeMeanCov(cov);
      std::printf("pose %.9g %.9g %.9g %.9g %.9g\n", mean[0], mean[1], mean[2], cov(0, 0), cov(1, 1));
      for (int k = 0; k < conv_steps; k++) {   // (on to the step count the convergence criterion is written for)
        const std::vector<float> mix = mixture(c->filter());   // what this step's update sizes the next set from
        const int64_t before = c->filter()->numParticles();
        c->takeStep(cloud, trans, yaw);
        const int64_t after = c->filter()->numParticles();
        const int kc = (int)mix[0];
        const int64_t want = kc == 0 ? before : tdr_adaptive_count_host(mix.data() + 1 + 3 * kc, kc, before, cfg.particle_count);
        if (after != want)
          throw std::runtime_error("B step " + std::to_string(k) + ": " + std::to_string(after) + " particles, :151-157 gives " +
                                   std::to_string(want));
        if ((mixture(c->filter()).size() > 1) != (k + 1 >= 2))   // the first fit follows the 2nd step's publishPoseEst
          throw std::runtime_error("B step " + std::to_string(k) + ": the first fit is not after the 2nd step");
        std::printf("count %d %lld\n", k, (long long)after);
      }
      c->filter()->meanLikelihood(mean);
      c->filter()->computeMeanCov(cov);
      std::printf("pose %.9g %.9g %.9g %.9g %.9g\n", mean[0], mean[1], mean[2], cov(0, 0), cov(1, 1));
      Eigen::Vector4f ml;
      c->filter()->maxLikelihood(ml);
      std::printf("ml %.9g %.9g\n", ml[0], ml[1]);
      delete c;
    }

    // ---- C: three cores, gmm_every = 0, 2, 3, batched against standalone
    {
      const int every[3] = {0, 2, 3};
      std::vector<TopDownRenderCore*> batch, twins;
      std::vector<pcl::PointCloud<PointType>::ConstPtr> clouds(3, cloud);
      std::vector<Eigen::Vector2f> tr(3, trans);
      std::vector<float> yw(3, yaw);
      for (int r = 0; r < 3; r++) {
        auto st = slurp<State>(dir + "/states_" + std::to_string(r) + ".bin");
        TopDownRenderCore::Config cfg = base_config((int)st.size(), 11 + 2 * r);
        cfg.gmm_every = every[r];
        batch.push_back(make_core(cfg, st));
        twins.push_back(make_core(cfg, st));
      }
      TopDownRenderCoreBatch loop;
      for (int k = 0; k < steps; k++) {
        std::vector<TopDownRenderCore::PoseEst> eb;
        if (!loop.takeStep(batch, clouds, tr, yw, &eb)) throw std::runtime_error("takeStep skipped: no map");
        int b = -1, s = -1;
        tdr_batch_last_stats(&b, &s);
        if (b != loop.lastBatched() || s != loop.lastStandalone())
          throw std::runtime_error("C: the mixture fit changed tdr_batch_last_stats");
        std::printf("stats %d %d %d\n", k, b, s);
        for (int r = 0; r < 3; r++) {
          TopDownRenderCore::PoseEst et;
          twins[r]->takeStep(clouds[r], tr[r], yw[r], &et);
          const std::string where = "C step " + std::to_string(k) + " robot " + std::to_string(r);
          if (!same_est(eb[r], et)) throw std::runtime_error(where + ": PoseEst differs");
          same_filters(batch[r]->filter(), twins[r]->filter(), where);
          if (batch[r]->currentRangeScale() != twins[r]->currentRangeScale() || batch[r]->isConverged() != twins[r]->isConverged())
            throw std::runtime_error(where + ": loop state differs");
        }
      }
      if (mixture(batch[0]->filter()).size() != 1 || mixture(batch[1]->filter()).size() == 1 ||
          mixture(batch[2]->filter()).size() == 1)
        throw std::runtime_error("C: the cores with gmm_every > 0, and only they, must hold a mixture");
      for (auto* c : batch) delete c;
      for (auto* c : twins) delete c;
    }
    std::puts("ok");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "facade_gmm failed: %s\n", e.what());
    return 1;
  }
}
