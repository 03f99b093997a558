// facade_recovery.cpp — the recovery injection (include/tdr.h, "recovery injection") through the drop-in classes:
//   inject <dir>  TopDownMap::roadCells, then on the particle sets of states.bin ParticleFilter::inject (robot r with seed
//                 rseed + r), ParticleFilterBatch::inject on fresh filters and ParticleFilterCartesian::inject on robot 0's
//                 set.  Writes out_road.bin, out_inject_<who>_<r>.bin (the states after the call) and prints one line
//                 "<who> <injected>" per call
//   loop <dir>    TopDownRenderCore::takeStep with Config::recovery_every, one core per robot, each stepped on its own
//   batch <dir>   the same robots through TopDownRenderCoreBatch::takeStep
// loop / batch write, per robot r, out_rec_<r>.bin (double [steps][4]: the step's probability, the replaced slots, and the
// tracker's slow and fast average afterwards) and out_states_<r>.bin (the particle sets after every step).
// Inputs: raw little-endian files in <dir> (tests/test_recovery.py writes them and checks everything against
// tests/recovery_ref.py).
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
  if (argc < 3) { std::fprintf(stderr, "usage: %s inject|loop|batch <dir>\n", argv[0]); return 2; }
  const std::string mode = argv[1], dir = argv[2];
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

    if (mode == "inject") {
      map.samplePtsPolar(Eigen::Vector2i(nb, nr), (float)(2 * M_PI / nb));
      dump(dir + "/out_road.bin", map.roadCells());
      std::vector<ParticleFilter*> filters, fresh;
      std::vector<double> ps;
      std::vector<uint64_t> seeds;
      for (int r = 0; r < robots; r++) {
        filters.push_back(new ParticleFilter(npart, &map, filter_params, seed + r));
        filters.back()->setStates(robot_states(r));
        const int64_t n = filters.back()->inject(inject_p, rp.heading_mode, rp.seed + r);
        std::printf("polar %lld\n", (long long)n);
        dump(dir + "/out_inject_polar_" + std::to_string(r) + ".bin", filters.back()->states());
        fresh.push_back(new ParticleFilter(npart, &map, filter_params, seed + r));
        fresh.back()->setStates(robot_states(r));
        ps.push_back(inject_p);
        seeds.push_back(rp.seed + r);
      }
      std::vector<int64_t> injected;
      ParticleFilterBatch().inject(fresh, ps, rp.heading_mode, seeds, &injected);
      for (int r = 0; r < robots; r++) {
        std::printf("batch %lld\n", (long long)injected[r]);
        dump(dir + "/out_inject_batch_" + std::to_string(r) + ".bin", fresh[r]->states());
      }
      for (ParticleFilter* f : filters) delete f;
      for (ParticleFilter* f : fresh) delete f;
      TopDownMap cmap(map_params);
      cmap.setDistanceMaps(class_maps, class_mask);
      cmap.setWindow(nb, nr);
      ParticleFilterCartesian cf(npart, &cmap, filter_params, seed);
      cf.setStates(robot_states(0));
      std::printf("cart %lld\n", (long long)cf.inject(inject_p, rp.heading_mode, rp.seed));
      dump(dir + "/out_inject_cart_0.bin", cf.states());
      std::puts("facade_recovery ok");
      return 0;
    }

    Eigen::VectorXi flatten_lut = Eigen::VectorXi::Constant(256, -1);
    for (int c = 0; c < ncls; c++) flatten_lut[c] = c;
    pcl::PointCloud<PointType>::Ptr cloud(new pcl::PointCloud<PointType>());
    for (int i = 0; i < npts; i++) {
      const float* q = pts.data() + (size_t)i * 8;
      PointType p{};
      p.x = q[0]; p.y = q[1]; p.z = q[2]; p.intensity = q[4];
      cloud->push_back(p);
    }
    std::vector<TopDownRenderCore*> cores;
    for (int r = 0; r < robots; r++) {
      TopDownRenderCore::Config cfg;
      cfg.particle_count = npart;
      cfg.theta_bins = nb;
      cfg.range_bins = nr;
      cfg.seed = seed + r;
      cfg.recovery_every = recovery_every;
      cfg.recovery = rp;
      cfg.recovery.seed = rp.seed + r;
      cores.push_back(new TopDownRenderCore(cfg));
      cores.back()->initialize(&map, filter_params, flatten_lut);
      cores.back()->setDeviceScan(true);
      cores.back()->filter()->setStates(robot_states(r));
    }
    std::vector<std::vector<double>> rec(robots);
    std::vector<std::vector<State>> states(robots);
    auto record = [&](int r) {
      rec[r].push_back(cores[r]->lastRecoveryP());
      rec[r].push_back((double)cores[r]->lastRecoveryInjected());
      rec[r].push_back(cores[r]->recoveryState().w_slow);
      rec[r].push_back(cores[r]->recoveryState().w_fast);
      auto st = cores[r]->filter()->states();
      states[r].insert(states[r].end(), st.begin(), st.end());
    };
    const Eigen::Vector2f trans(motion[0], motion[1]);
    if (mode == "loop") {
      for (int r = 0; r < robots; r++)
        for (int s = 0; s < steps; s++) {
          if (!cores[r]->takeStep(cloud, trans, motion[2])) throw std::runtime_error("takeStep skipped: no map");
          record(r);
        }
    } else if (mode == "batch") {
      TopDownRenderCoreBatch batch;
      const std::vector<pcl::PointCloud<PointType>::ConstPtr> clouds(robots, cloud);
      const std::vector<Eigen::Vector2f> tr(robots, trans);
      const std::vector<float> yaw(robots, motion[2]);
      for (int s = 0; s < steps; s++) {
        if (!batch.takeStep(cores, clouds, tr, yaw)) throw std::runtime_error("takeStep skipped: no map");
        for (int r = 0; r < robots; r++) record(r);
      }
    } else {
      throw std::runtime_error("unknown mode " + mode);
    }
    for (int r = 0; r < robots; r++) {
      dump(dir + "/out_rec_" + std::to_string(r) + ".bin", rec[r]);
      dump(dir + "/out_states_" + std::to_string(r) + ".bin", states[r]);
      delete cores[r];
    }
    std::puts("facade_recovery ok");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "facade_recovery failed: %s\n", e.what());
    return 1;
  }
}
