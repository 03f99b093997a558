// facade_sensor_reset.cpp — sensor resetting (include/tdr.h, "sensor resetting") through the drop-in classes:
//   inject <dir> <candidates> <res>  on the particle sets of states.bin, against the render of pts.bin at <res>:
//                 ParticleFilter::injectSensor (robot r with seed rseed + r) and ParticleFilterCartesian::injectSensor on
//                 robot 0's set (window nb x nr).  Writes out_sensor_<who>_<r>.bin (the states after the call) and prints one
//                 line "<who> <written>" per call
//   loop <dir> <candidates>          TopDownRenderCore::takeStep with Config::recovery_every and recovery_candidates
//   batch <dir> <candidates>         the same core through TopDownRenderCoreBatch::takeStep: refused for candidates > 1
//                                    (prints "refused: <message>" and exits 0 then)
// loop writes out_rec_0.bin (double [steps][4]: the step's probability, the replaced slots, the tracker's slow and fast
// average afterwards) and out_states_0.bin (the particle set after every step).
// Inputs: the raw little-endian files of tests/cpp/facade_recovery.cpp (tests/test_sensor_reset_facade.py writes them).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "top_down_render/particle_filter_cartesian.h"
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
template <class T>
static void dump(const std::string& path, const std::vector<T>& v) {
  std::ofstream out(path, std::ios::binary | std::ios::trunc);
  out.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s inject|loop|batch <dir> <candidates> [<res>]\n", argv[0]); return 2; }
  const std::string mode = argv[1], dir = argv[2];
  const int candidates = std::atoi(argv[3]);
  const float res = argc > 4 ? (float)std::atof(argv[4]) : 1.f;
  try {
    int ncls, rows, cols, nb, nr, npts, npart, steps, robots, recovery_every;
    unsigned seed;
    float fixed_scale, map_resolution;
    double inject_p;
    unsigned long long rseed;
    RecoveryParams rp;
    {
      std::ifstream meta(dir + "/meta.txt");
      meta >> ncls >> rows >> cols >> nb >> nr >> npts >> npart >> seed >> steps >> fixed_scale >> map_resolution >> robots >>
          recovery_every >> rp.alpha_slow >> rp.alpha_fast >> rp.p_max >> rp.heading_mode >> rseed >> inject_p;
      if (!meta) throw std::runtime_error("bad meta.txt");
      rp.seed = rseed;
    }
    auto maps = slurp<float>(dir + "/maps.bin");
    auto mask = slurp<uint8_t>(dir + "/mask.bin");
    auto pts = slurp<float>(dir + "/pts.bin");        // [npts][8]: pcl::PointXYZI layout
    auto st_in = slurp<State>(dir + "/states.bin");   // [robots][npart]
    auto motion = slurp<float>(dir + "/motion.bin");  // [3]: trans x, trans y, yaw of the projected prior
    if (st_in.size() != (size_t)robots * npart) throw std::runtime_error("states.bin does not hold robots * npart states");

    TopDownMap::Params map_params;
    map_params.num_classes = ncls;
    map_params.resolution = map_resolution;
    for (int c = 0; c < ncls; c++) map_params.flatten_lut.push_back(c);
    std::vector<Eigen::ArrayXXf> class_maps;
    for (int c = 0; c < ncls; c++) {
      Eigen::ArrayXXf m(rows, cols);
      std::memcpy(m.data(), maps.data() + (size_t)c * rows * cols, (size_t)rows * cols * sizeof(float));
      class_maps.push_back(m);
    }
    Eigen::ArrayXXc class_mask(rows, cols);
    std::memcpy(class_mask.data(), mask.data(), (size_t)rows * cols);
    TopDownMapPolar map(map_params);
    map.setDistanceMaps(class_maps, class_mask);

    FilterParams filter_params;
    filter_params.pos_cov = 0.3f;
    filter_params.theta_cov = (float)(M_PI / 100);
    filter_params.regularization = 0.15f;
    filter_params.fixed_scale = fixed_scale;
    for (int c = 0; c < ncls; c++) filter_params.class_weights.push_back(1.f);
    filter_params.init_pos_m_x = 1e9f;   // initializeParticles returns early: the test brings its own particle sets
    filter_params.init_pos_m_y = 1e9f;
    auto robot_states = [&](int r) { return std::vector<State>(st_in.begin() + (size_t)r * npart, st_in.begin() + (size_t)(r + 1) * npart); };

    Eigen::VectorXi flatten_lut = Eigen::VectorXi::Constant(256, -1);
    for (int c = 0; c < ncls; c++) flatten_lut[c] = c;
    pcl::PointCloud<PointType>::Ptr cloud(new pcl::PointCloud<PointType>());
    for (int i = 0; i < npts; i++) {
      const float* q = pts.data() + (size_t)i * 8;
      PointType p{};
      p.x = q[0]; p.y = q[1]; p.z = q[2]; p.intensity = q[4];
      cloud->push_back(p);
    }

    if (mode == "inject") {
      map.samplePtsPolar(Eigen::Vector2i(nb, nr), (float)(2 * M_PI / nb));
      ScanRendererPolar renderer(flatten_lut);
      std::vector<Eigen::ArrayXXf> imgs(ncls, Eigen::ArrayXXf(nb, nr));
      renderer.renderSemanticTopDown(cloud, res, (float)(2 * M_PI / nb), imgs);
      for (int r = 0; r < robots; r++) {
        ParticleFilter f(npart, &map, filter_params, seed + r);
        f.setStates(robot_states(r));
        const int64_t n = f.injectSensor(&renderer, res, inject_p, candidates, rp.heading_mode, rp.seed + r);
        std::printf("polar %lld\n", (long long)n);
        dump(dir + "/out_sensor_polar_" + std::to_string(r) + ".bin", f.states());
      }
      TopDownMap cmap(map_params);
      cmap.setDistanceMaps(class_maps, class_mask);
      cmap.setWindow(nb, nr);
      ScanRenderer crenderer(flatten_lut);
      std::vector<Eigen::ArrayXXf> cimgs(ncls, Eigen::ArrayXXf(nb, nr));
      crenderer.renderSemanticTopDown(cloud, res, cimgs);
      ParticleFilterCartesian cf(npart, &cmap, filter_params, seed);
      cf.setStates(robot_states(0));
      std::printf("cart %lld\n", (long long)cf.injectSensor(&crenderer, res, inject_p, candidates, rp.heading_mode, rp.seed));
      dump(dir + "/out_sensor_cart_0.bin", cf.states());
      std::puts("facade_sensor_reset ok");
      return 0;
    }

    TopDownRenderCore::Config cfg;
    cfg.particle_count = npart;
    cfg.theta_bins = nb;
    cfg.range_bins = nr;
    cfg.seed = seed;
    cfg.recovery_every = recovery_every;
    cfg.recovery = rp;
    cfg.recovery_candidates = candidates;
    TopDownRenderCore core(cfg);
    core.initialize(&map, filter_params, flatten_lut);
    core.setDeviceScan(true);
    core.filter()->setStates(robot_states(0));
    const Eigen::Vector2f trans(motion[0], motion[1]);
    if (mode == "batch") {
      TopDownRenderCoreBatch batch;
      std::vector<TopDownRenderCore*> cores(1, &core);
      const std::vector<pcl::PointCloud<PointType>::ConstPtr> clouds(1, cloud);
      const std::vector<Eigen::Vector2f> tr(1, trans);
      const std::vector<float> yaw(1, motion[2]);
      try {
        batch.takeStep(cores, clouds, tr, yaw);
      } catch (const std::invalid_argument& e) {
        std::printf("refused: %s\n", e.what());
        return 0;
      }
      std::puts("stepped");
      return 0;
    }
    if (mode != "loop") throw std::runtime_error("unknown mode " + mode);
    std::vector<double> rec;
    std::vector<State> states;
    for (int s = 0; s < steps; s++) {
      if (!core.takeStep(cloud, trans, motion[2])) throw std::runtime_error("takeStep skipped: no map");
      rec.push_back(core.lastRecoveryP());
      rec.push_back((double)core.lastRecoveryInjected());
      rec.push_back(core.recoveryState().w_slow);
      rec.push_back(core.recoveryState().w_fast);
      auto st = core.filter()->states();
      states.insert(states.end(), st.begin(), st.end());
    }
    dump(dir + "/out_rec_0.bin", rec);
    dump(dir + "/out_states_0.bin", states);
    std::puts("facade_sensor_reset ok");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "facade_sensor_reset failed: %s\n", e.what());
    return 1;
  }
}
