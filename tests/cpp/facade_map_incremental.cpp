// facade_map_incremental.cpp — TopDownRenderCore::aerialMapIncremental against aerialMap: two cores over dynamic maps,
// one fed every map message through aerialMap, the other through aerialMapIncremental, with two steps after every
// message.  The particle sets and PoseEst must be the same bits after every step.  Inputs: raw little-endian files in
// argv[1] (tests/test_map_incremental.py).  Prints "msg <k> <changed cells of the incremental core>" per message, then "ok".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

#include "top_down_render/top_down_render_core.h"

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
static bool same_states(const std::vector<State>& a, const std::vector<State>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++) {
    const float fa[6] = {a[i].init_x_px, a[i].init_y_px, a[i].dx_m, a[i].dy_m, a[i].theta, a[i].scale};
    const float fb[6] = {b[i].init_x_px, b[i].init_y_px, b[i].dx_m, b[i].dy_m, b[i].theta, b[i].scale};
    if (std::memcmp(fa, fb, sizeof(fa)) != 0 || a[i].have_init != b[i].have_init) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  try {
    int ncls, h, w, msgs;
    {
      std::ifstream meta(dir + "/meta.txt");
      meta >> ncls >> h >> w >> msgs;
      if (!meta) throw std::runtime_error("bad meta.txt");
    }
    auto imgs = slurp<uint8_t>(dir + "/imgs.bin");   // [msgs][h][w] label images, row 0 = top
    auto pts = slurp<float>(dir + "/pts.bin");       // [n][4]: x, y, z, label
    if (imgs.size() != (size_t)msgs * h * w) throw std::runtime_error("bad imgs.bin");

    TopDownMap::Params map_params;   // an empty map_path: the dynamic map, it arrives through aerialMap
    map_params.num_classes = ncls;
    map_params.resolution = 1.f;
    for (int c = 0; c < ncls; c++) map_params.flatten_lut.push_back(c);
    FilterParams filter_params;
    filter_params.pos_cov = 0.3f;
    filter_params.theta_cov = (float)(M_PI / 100);
    filter_params.regularization = 0.15f;
    for (int c = 0; c < ncls; c++) filter_params.class_weights.push_back(1.f);
    Eigen::VectorXi flatten_lut = Eigen::VectorXi::Constant(256, -1);
    for (int c = 0; c < ncls; c++) flatten_lut[c] = c;
    TopDownRenderCore::Config cfg;
    cfg.particle_count = 3000;
    cfg.theta_bins = 64;
    cfg.range_bins = 24;
    cfg.seed = 17;
    TopDownRenderCore full(cfg), incr(cfg);
    full.initialize(map_params, filter_params, flatten_lut);
    incr.initialize(map_params, filter_params, flatten_lut);

    pcl::PointCloud<PointType>::Ptr cloud(new pcl::PointCloud<PointType>());
    for (size_t i = 0; i + 3 < pts.size(); i += 4) {
      PointType p{};
      p.x = pts[i]; p.y = pts[i + 1]; p.z = pts[i + 2]; p.intensity = pts[i + 3];
      cloud->push_back(p);
    }
    for (int k = 0; k < msgs; k++) {
      cv::Mat img(h, w, imgs.data() + (size_t)k * h * w);
      const Eigen::Vector2i center(w / 2 + k, h / 2 - k);
      full.aerialMap(img, center);
      const int64_t changed = incr.aerialMapIncremental(img, center);
      std::printf("msg %d %lld\n", k, (long long)changed);
      if (!same_states(full.filter()->states(), incr.filter()->states())) {
        std::printf("states differ after message %d\n", k);
        return 1;
      }
      for (int s = 0; s < 2; s++) {
        TopDownRenderCore::PoseEst ea, eb;
        const bool ra = full.takeStep(cloud, Eigen::Vector2f(0.4f, 0.1f), 0.02f, &ea);
        const bool rb = incr.takeStep(cloud, Eigen::Vector2f(0.4f, 0.1f), 0.02f, &eb);
        if (ra != rb || (ra && !same_est(ea, eb)) || !same_states(full.filter()->states(), incr.filter()->states())) {
          std::printf("step %d after message %d differs\n", s, k);
          return 1;
        }
      }
    }
    std::printf("ok\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
