// facade_grid.cpp — the pose-grid search (include/tdr.h, "pose-grid search") through the drop-in classes:
//   facade_grid <dir> <res> <c0> <r0> <step> <nx> <ny> <road_only> <heading_mode> <n_headings> <theta0> <dtheta> <scale> <R> <K>
// On robot 0's particle set of states.bin, against the render of pts.bin at <res>: ParticleFilter::gridSearch, then
// ParticleFilter::injectCells of the peaks' cells (p = inject_p, the heading mode and seed of meta.txt); the same through
// ParticleFilterCartesian (window nb x nr).  Writes out_grid_<who>_{w,theta,vol,peaks}.bin and out_grid_<who>_states.bin
// (the states after the injection) and prints one line "<who> <listed> <n_peaks> <injected>" per filter.
// Inputs: the raw little-endian files of tests/cpp/facade_recovery.cpp (tests/test_grid_facade.py writes them).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "top_down_render/particle_filter.h"
#include "top_down_render/particle_filter_cartesian.h"
#include "top_down_render/scan_renderer_polar.h"

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

template <class Filter, class Renderer>
static void search_and_inject(const std::string& dir, const char* who, Filter& f, Renderer& renderer, float res, const GridSpec& spec,
                              int R, int K, double p, int heading_mode, uint64_t seed) {
  const GridSearchResult g = f.gridSearch(&renderer, res, spec, R, K, true);
  const std::string base = dir + "/out_grid_" + who;
  dump(base + "_w.bin", g.w);
  dump(base + "_theta.bin", g.theta);
  dump(base + "_vol.bin", g.vol);
  dump(base + "_peaks.bin", g.peaks);
  std::vector<uint32_t> cells;
  for (const tdr_grid_peak& pk : g.peaks) cells.push_back(pk.cell);
  const int64_t injected = cells.empty() ? 0 : f.injectCells(cells, p, heading_mode, seed);
  dump(base + "_states.bin", f.states());
  std::printf("%s %lld %lld %lld\n", who, (long long)g.listed, (long long)g.n_peaks, (long long)injected);
}

int main(int argc, char** argv) {
  if (argc < 16) { std::fprintf(stderr, "usage: %s <dir> <res> <11 spec fields> <R> <K>\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  const float res = (float)std::atof(argv[2]);
  GridSpec spec(std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7]));
  spec.road_only = std::atoi(argv[8]);
  spec.heading_mode = std::atoi(argv[9]);
  spec.n_headings = std::atoi(argv[10]);
  spec.theta0 = (float)std::atof(argv[11]);
  spec.dtheta = (float)std::atof(argv[12]);
  spec.scale = (float)std::atof(argv[13]);
  const int R = std::atoi(argv[14]), K = std::atoi(argv[15]);
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
    if (st_in.size() < (size_t)npart) throw std::runtime_error("states.bin does not hold npart states");
    const std::vector<State> states(st_in.begin(), st_in.begin() + npart);

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

    FilterParams filter_params;
    filter_params.pos_cov = 0.3f;
    filter_params.theta_cov = (float)(M_PI / 100);
    filter_params.regularization = 0.15f;
    filter_params.fixed_scale = fixed_scale;
    for (int c = 0; c < ncls; c++) filter_params.class_weights.push_back(1.f);
    filter_params.init_pos_m_x = 1e9f;   // initializeParticles returns early: the test brings its own particle set
    filter_params.init_pos_m_y = 1e9f;

    Eigen::VectorXi flatten_lut = Eigen::VectorXi::Constant(256, -1);
    for (int c = 0; c < ncls; c++) flatten_lut[c] = c;
    pcl::PointCloud<PointType>::Ptr cloud(new pcl::PointCloud<PointType>());
    for (int i = 0; i < npts; i++) {
      const float* q = pts.data() + (size_t)i * 8;
      PointType p{};
      p.x = q[0]; p.y = q[1]; p.z = q[2]; p.intensity = q[4];
      cloud->push_back(p);
    }

    {
      TopDownMapPolar map(map_params);
      map.setDistanceMaps(class_maps, class_mask);
      map.samplePtsPolar(Eigen::Vector2i(nb, nr), (float)(2 * M_PI / nb));
      ScanRendererPolar renderer(flatten_lut);
      std::vector<Eigen::ArrayXXf> imgs(ncls, Eigen::ArrayXXf(nb, nr));
      renderer.renderSemanticTopDown(cloud, res, (float)(2 * M_PI / nb), imgs);
      ParticleFilter f(npart, &map, filter_params, seed);
      f.setStates(states);
      search_and_inject(dir, "polar", f, renderer, res, spec, R, K, inject_p, rp.heading_mode, rp.seed);
    }
    {
      TopDownMap cmap(map_params);
      cmap.setDistanceMaps(class_maps, class_mask);
      cmap.setWindow(nb, nr);
      ScanRenderer crenderer(flatten_lut);
      std::vector<Eigen::ArrayXXf> cimgs(ncls, Eigen::ArrayXXf(nb, nr));
      crenderer.renderSemanticTopDown(cloud, res, cimgs);
      ParticleFilterCartesian cf(npart, &cmap, filter_params, seed);
      cf.setStates(states);
      search_and_inject(dir, "cart", cf, crenderer, res, spec, R, K, inject_p, rp.heading_mode, rp.seed);
    }
    // what the classes refuse: a spec outside its ranges throws before anything is written
    {
      TopDownMapPolar map(map_params);
      map.setDistanceMaps(class_maps, class_mask);
      map.samplePtsPolar(Eigen::Vector2i(nb, nr), (float)(2 * M_PI / nb));
      ScanRendererPolar renderer(flatten_lut);
      std::vector<Eigen::ArrayXXf> imgs(ncls, Eigen::ArrayXXf(nb, nr));
      renderer.renderSemanticTopDown(cloud, res, (float)(2 * M_PI / nb), imgs);
      ParticleFilter f(npart, &map, filter_params, seed);
      f.setStates(states);
      GridSpec bad = spec;
      bad.step = 0;
      int thrown = 0;
      try { f.gridSearch(&renderer, res, bad); } catch (const std::runtime_error&) { thrown++; }
      try { f.gridSearch(&renderer, res, spec, 17); } catch (const std::runtime_error&) { thrown++; }
      try { f.injectCells(std::vector<uint32_t>(1, (uint32_t)rows * (uint32_t)cols), 0.5); } catch (const std::runtime_error&) { thrown++; }
      std::printf("refused %d\n", thrown);
    }
    std::puts("facade_grid ok");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "facade_grid failed: %s\n", e.what());
    return 1;
  }
}
