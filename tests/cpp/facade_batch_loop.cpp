// facade_batch_loop.cpp — TopDownRenderCoreBatch (include/top_down_render/top_down_render_core_batch.h) against
// standalone cores: R robots on one map stepped together through the batched node loop, R twins stepped one at a time
// through TopDownRenderCore::takeStep with setDeviceScan(true).  After every step the particle sets must be the same bits
// and PoseEst, currentRangeScale, lastRes and isConverged the same values.  Inputs: raw little-endian files in argv[1]
// (tests/test_batch_loop.py).  Prints one line per step: "step <k> <batched> <standalone> <froze mask> <converged mask>",
// then "ok".
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

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  try {
    int ncls, rows, cols, nb, nr, robots, steps;
    float rs_min, rs_max, target_unc, map_resolution;
    {
      std::ifstream meta(dir + "/meta.txt");
      meta >> ncls >> rows >> cols >> nb >> nr >> robots >> steps >> rs_min >> rs_max >> target_unc >> map_resolution;
      if (!meta) throw std::runtime_error("bad meta.txt");
    }
    auto maps = slurp<float>(dir + "/maps.bin");
    auto mask = slurp<uint8_t>(dir + "/mask.bin");
    auto seeds = slurp<uint32_t>(dir + "/seeds.bin");   // [robots]
    auto motion = slurp<float>(dir + "/motion.bin");    // [robots][3]

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
    filter_params.fixed_scale = -1.f;
    for (int c = 0; c < ncls; c++) filter_params.class_weights.push_back(1.f);
    filter_params.init_pos_m_x = 1e9f;   // initializeParticles returns early: the test brings its own particle sets
    filter_params.init_pos_m_y = 1e9f;
    Eigen::VectorXi flatten_lut = Eigen::VectorXi::Constant(256, -1);
    for (int c = 0; c < ncls; c++) flatten_lut[c] = c;

    std::vector<TopDownRenderCore*> batch, twins;
    std::vector<pcl::PointCloud<PointType>::ConstPtr> clouds;
    std::vector<Eigen::Vector2f> trans;
    std::vector<float> yaw;
    for (int r = 0; r < robots; r++) {
      auto st = slurp<State>(dir + "/states_" + std::to_string(r) + ".bin");
      auto pts = slurp<float>(dir + "/pts_" + std::to_string(r) + ".bin");   // [n][8]: pcl::PointXYZI layout
      pcl::PointCloud<PointType>::Ptr cloud(new pcl::PointCloud<PointType>());
      for (size_t i = 0; i < pts.size() / 8; i++) {
        PointType p{};
        p.x = pts[8 * i]; p.y = pts[8 * i + 1]; p.z = pts[8 * i + 2]; p.intensity = pts[8 * i + 4];
        cloud->push_back(p);
      }
      clouds.push_back(cloud);
      trans.emplace_back(motion[3 * r], motion[3 * r + 1]);
      yaw.push_back(motion[3 * r + 2]);
      for (auto* v : {&batch, &twins}) {
        TopDownRenderCore::Config cfg;
        cfg.particle_count = (int)st.size();
        cfg.range_scale_min = rs_min;
        cfg.range_scale_max = rs_max;
        cfg.target_uncertainty_m = target_unc;
        cfg.theta_bins = nb;
        cfg.range_bins = nr;
        cfg.seed = seeds[r];
        auto* core = new TopDownRenderCore(cfg);
        core->initialize(&map, filter_params, flatten_lut);
        core->setDeviceScan(true);
        core->filter()->setStates(st);
        v->push_back(core);
      }
    }

    TopDownRenderCoreBatch loop;
    auto check_same = [&](int k) {
      for (int r = 0; r < robots; r++) {
        const auto a = batch[r]->filter()->states(), b = twins[r]->filter()->states();
        if (a.size() != b.size() || std::memcmp(a.data(), b.data(), a.size() * sizeof(State)) != 0)
          throw std::runtime_error("step " + std::to_string(k) + ": robot " + std::to_string(r) + ": particle states differ");
        const int n = (int)a.size();
        const auto wa = batch[r]->filter()->rawWeights(n), wb = twins[r]->filter()->rawWeights(n);
        const auto ia = batch[r]->filter()->resampleIndices(), ib = twins[r]->filter()->resampleIndices();
        if (std::memcmp(wa.data(), wb.data(), wa.size() * sizeof(float)) != 0 || ia != ib)
          throw std::runtime_error("step " + std::to_string(k) + ": robot " + std::to_string(r) + ": weights differ");
        if (batch[r]->currentRangeScale() != twins[r]->currentRangeScale() || batch[r]->lastRes() != twins[r]->lastRes() ||
            batch[r]->isConverged() != twins[r]->isConverged())
          throw std::runtime_error("step " + std::to_string(k) + ": robot " + std::to_string(r) + ": loop state differs");
      }
    };
    for (int k = 0; k < steps; k++) {
      std::vector<TopDownRenderCore::PoseEst> eb;
      if (!loop.takeStep(batch, clouds, trans, yaw, &eb)) throw std::runtime_error("takeStep skipped: no map");
      unsigned froze = 0, conv = 0;
      for (int r = 0; r < robots; r++) {
        TopDownRenderCore::PoseEst et;
        twins[r]->takeStep(clouds[r], trans[r], yaw[r], &et);
        if (!same_est(eb[r], et))
          throw std::runtime_error("step " + std::to_string(k) + ": robot " + std::to_string(r) + ": PoseEst differs");
        froze |= (et.froze_scale ? 1u : 0u) << r;
        conv |= (et.converged ? 1u : 0u) << r;
      }
      check_same(k);
      std::printf("step %d %d %d %u %u\n", k, loop.lastBatched(), loop.lastStandalone(), froze, conv);
    }

    // refusals: another map, other bins — thrown before anything moves; the next step still matches the twins
    {
      TopDownMapPolar other(map_params);
      TopDownRenderCore::Config cfg;
      cfg.particle_count = 16;
      cfg.theta_bins = nb;
      cfg.range_bins = nr;
      cfg.seed = 3;
      TopDownRenderCore::Config cfg2 = cfg;
      cfg2.range_bins = nr + 1;
      TopDownRenderCore c_other(cfg), c_bins(cfg2);
      FilterParams fp = filter_params;
      c_other.initialize(&other, fp, flatten_lut);
      c_bins.initialize(&other, fp, flatten_lut);   // (other bins: checked before the map)
      int refused = 0;
      for (TopDownRenderCore* extra : {&c_other, &c_bins}) {
        std::vector<TopDownRenderCore*> cs(batch);
        cs.push_back(extra);
        std::vector<pcl::PointCloud<PointType>::ConstPtr> cl(clouds);
        cl.push_back(clouds[0]);
        std::vector<Eigen::Vector2f> tr(trans);
        tr.push_back(trans[0]);
        std::vector<float> yw(yaw);
        yw.push_back(yaw[0]);
        try {
          loop.takeStep(cs, cl, tr, yw);
        } catch (const std::invalid_argument&) {
          refused++;
        }
      }
      if (refused != 2) throw std::runtime_error("a bad batch was not refused");
      check_same(steps);
      std::vector<TopDownRenderCore::PoseEst> eb;
      loop.takeStep(batch, clouds, trans, yaw, &eb);
      for (int r = 0; r < robots; r++) {
        TopDownRenderCore::PoseEst et;
        twins[r]->takeStep(clouds[r], trans[r], yaw[r], &et);
        if (!same_est(eb[r], et)) throw std::runtime_error("after the refusals: robot " + std::to_string(r) + ": PoseEst differs");
      }
      check_same(steps + 1);
    }
    for (auto* c : batch) delete c;
    for (auto* c : twins) delete c;
    std::puts("ok");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "facade_batch_loop failed: %s\n", e.what());
    return 1;
  }
}
