// facade_fleet.cpp — the fleet picture through the C++ classes: TopDownMap::setVizBackground (a BGR image, then a label
// image with padded rows), TopDownRenderCoreBatch::renderFleetPicture and ParticleFilterBatch::renderFleet, on the scene
// tests/test_fleet_viz.py dumped into argv[1].  Three robots on one map take one batched step, robot 0 fits its mixture,
// and all three are drawn in one image; the image is written back as raw bytes with the states, the mixture and the
// max-likelihood state of every robot, for the test's byte comparison.  Prints "ok <robots>".
//
// Inputs (little endian): meta.txt "ncls rows cols nb nr pub_scale bgH bgW labH labW"; maps.bin float [ncls][rows*cols]
// column-major; mask.bin uint8; states_<r>.bin State; pts_<r>.bin float [n][8]; bg.bin uint8 [bgH][bgW][3]; labels.bin
// uint8 [labH][labW]; lut.bin uint32 [256] packed colours; palette.bin uint8 [3][3][3]; arrows.bin int32 [m][4].
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
static void dump(const std::string& path, const void* p, size_t bytes) {
  std::ofstream out(path, std::ios::binary);
  out.write(static_cast<const char*>(p), (std::streamsize)bytes);
  if (!out) throw std::runtime_error("cannot write " + path);
}
static void dumpImage(const std::string& stem, const tdr_viz::Image& img) {
  const int32_t hw[2] = {img.h, img.w};
  dump(stem + "_size.bin", hw, sizeof(hw));
  dump(stem + ".bin", img.bgr.data(), img.bgr.size());
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  const int K = 3;
  try {
    int ncls, rows, cols, nb, nr, bg_h, bg_w, lab_h, lab_w;
    float pub_scale;
    {
      std::ifstream meta(dir + "/meta.txt");
      meta >> ncls >> rows >> cols >> nb >> nr >> pub_scale >> bg_h >> bg_w >> lab_h >> lab_w;
      if (!meta) throw std::runtime_error("bad meta.txt");
    }
    const auto maps = slurp<float>(dir + "/maps.bin");
    const auto mask = slurp<uint8_t>(dir + "/mask.bin");
    const SemanticColorLut color_lut(slurp<uint32_t>(dir + "/lut.bin"));

    TopDownMap::Params map_params;
    map_params.num_classes = ncls;
    map_params.resolution = 1;
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
    FilterParams fp;
    fp.pos_cov = 0.3f;
    fp.theta_cov = (float)(M_PI / 100);
    fp.regularization = 0.15f;
    fp.fixed_scale = 1.f;
    for (int c = 0; c < ncls; c++) fp.class_weights.push_back(1.f);
    fp.init_pos_m_x = 1e9f;   // initializeParticles returns early: the test brings its own particle sets
    fp.init_pos_m_y = 1e9f;
    Eigen::VectorXi flatten_lut = Eigen::VectorXi::Constant(256, -1);
    for (int c = 0; c < ncls; c++) flatten_lut[c] = c;

    std::vector<TopDownRenderCore*> cores;
    std::vector<pcl::PointCloud<PointType>::ConstPtr> clouds;
    for (int r = 0; r < K; r++) {
      const auto st = slurp<State>(dir + "/states_" + std::to_string(r) + ".bin");
      const auto pts = slurp<float>(dir + "/pts_" + std::to_string(r) + ".bin");
      pcl::PointCloud<PointType>::Ptr cloud(new pcl::PointCloud<PointType>());
      for (size_t i = 0; i < pts.size() / 8; i++) {
        PointType p{};
        p.x = pts[8 * i]; p.y = pts[8 * i + 1]; p.z = pts[8 * i + 2]; p.intensity = pts[8 * i + 4];
        cloud->push_back(p);
      }
      clouds.push_back(cloud);
      TopDownRenderCore::Config cfg;
      cfg.particle_count = (int)st.size();
      cfg.theta_bins = nb;
      cfg.range_bins = nr;
      cfg.seed = 51 + (uint32_t)r;
      auto* core = new TopDownRenderCore(cfg);
      core->initialize(&map, fp, flatten_lut);
      core->filter()->setStates(st);
      cores.push_back(core);
    }
    const auto pal_bytes = slurp<uint8_t>(dir + "/palette.bin");
    if (pal_bytes.size() != (size_t)9 * K) throw std::runtime_error("bad palette.bin");
    std::vector<tdr_viz::FleetColours> palette(K);
    std::memcpy(palette.data(), pal_bytes.data(), pal_bytes.size());
    std::vector<std::array<int, 4>> arrows;
    {
      const auto arr = slurp<int32_t>(dir + "/arrows.bin");
      for (size_t i = 0; i < arr.size() / 4; i++) arrows.push_back({arr[4 * i], arr[4 * i + 1], arr[4 * i + 2], arr[4 * i + 3]});
    }

    // the background once, on the map; no filter has one of its own
    auto bg = slurp<uint8_t>(dir + "/bg.bin");
    map.setVizBackground(cv::Mat(bg_h, bg_w, CV_8UC3, bg.data()));

    TopDownRenderCoreBatch loop;
    const std::vector<Eigen::Vector2f> trans(K, Eigen::Vector2f(1.f, 0.f));
    const std::vector<float> yaw(K, 0.01f);
    if (!loop.takeStep(cores, clouds, trans, yaw)) throw std::runtime_error("takeStep skipped: no map");
    cores[0]->filter()->computeGMMDevice();

    tdr_viz::Image fleet, fleet2;
    loop.renderFleetPicture(cores, pub_scale, palette, arrows, fleet);
    ParticleFilterBatch pfb;
    int h2 = 0, w2 = 0;
    pfb.renderFleet({cores[0]->filter(), cores[1]->filter(), cores[2]->filter()}, pub_scale, palette, arrows, fleet2.bgr, h2, w2);
    if (fleet2.bgr != fleet.bgr || h2 != fleet.h || w2 != fleet.w)
      throw std::runtime_error("ParticleFilterBatch::renderFleet and renderFleetPicture differ");
    dumpImage(dir + "/out_fleet", fleet);

    // a filter still has no picture of its own
    bool refused = false;
    try {
      std::vector<uint8_t> one;
      int h = 0, w = 0;
      cores[0]->filter()->renderViz(one, h, w, pub_scale);
    } catch (const std::runtime_error&) {
      refused = true;
    }
    if (!refused) throw std::runtime_error("renderViz drew a filter that has no background of its own");

    // the label background (rows padded: the packing branch) replaces the first; no arrows
    const auto lab = slurp<uint8_t>(dir + "/labels.bin");
    std::vector<uint8_t> padded((size_t)lab_h * (lab_w + 3), 0xEE);
    for (int y = 0; y < lab_h; y++) std::memcpy(padded.data() + (size_t)y * (lab_w + 3), lab.data() + (size_t)y * lab_w, (size_t)lab_w);
    map.setVizBackground(cv::Mat(lab_h, lab_w, CV_8UC1, padded.data(), (size_t)lab_w + 3), color_lut);
    tdr_viz::Image on_labels;
    loop.renderFleetPicture(cores, pub_scale, palette, {}, on_labels);
    dumpImage(dir + "/out_fleet_labels", on_labels);

    for (int r = 0; r < K; r++) {   // what the pictures are pictures of
      const std::string tag = "_" + std::to_string(r) + ".bin";
      const auto st = cores[r]->filter()->states();
      dump(dir + "/out_states" + tag, st.data(), st.size() * sizeof(State));
      Eigen::Vector4f best;
      cores[r]->filter()->maxLikelihood(best);
      dump(dir + "/out_best" + tag, best.data(), 4 * sizeof(float));
      float gm[3 * TDR_GMM_MAX_K], gc[9 * TDR_GMM_MAX_K];
      int k = 0;
      if (tdr_filter_get_gmm(cores[r]->filter()->handle(), TDR_GMM_MAX_K, &k, gm, gc) != TDR_OK) throw std::runtime_error(tdr_last_error());
      std::vector<float> gmm(gm, gm + 3 * k);
      gmm.insert(gmm.end(), gc, gc + 9 * k);
      dump(dir + "/out_gmm" + tag, gmm.data(), gmm.size() * sizeof(float));
    }
    for (auto* c : cores) delete c;
    std::printf("ok %d\n", K);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "facade_fleet failed: %s\n", e.what());
    return 1;
  }
}
