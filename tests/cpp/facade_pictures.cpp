// facade_pictures.cpp — the pictures through the C++ classes: ScanRendererPolar::renderViz / renderVizAnalog,
// tdr_viz::scanPicture at the reference's two call sites (src/top_down_render.cpp:248, :258), the label background
// (ParticleFilter::setVizBackground(labels, lut)), ParticleFilterBatch::renderViz and
// TopDownRenderCoreBatch::renderPictures, on the scene tests/test_viz_batch.py dumped into argv[1].  Two robots on one map
// take one batched step; every picture is written back as raw bytes, with the states, the max-likelihood state and the
// render each is a picture of, for the test's byte comparison.  Prints "ok <range_bins> <theta_bins>".
//
// Inputs (little endian): meta.txt "ncls rows cols nb nr pub_scale analog_scale bgH0 bgW0 bgH1 bgW1"; maps.bin float
// [ncls][rows*cols] column-major; mask.bin uint8; states_<r>.bin State; pts_<r>.bin float [n][8]; bg_0.bin uint8
// [bgH0][bgW0][3]; labels_1.bin uint8 [bgH1][bgW1]; lut.bin uint32 [256] packed colours; unflatten.bin int32 [ncls];
// arrows_<r>.bin int32 [m][4].
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

// The node's members and methods around the scan images, as the reference declares and calls them
// (include/top_down_render/top_down_render.h:60-62, src/top_down_render.cpp:246-264); visualize's body is the one line.
struct Node {
  SemanticColorLut color_lut_;
  std::vector<int> unflatten_lut_;
  cv::Mat published_;   // stands for the image message
  void visualize(std::vector<Eigen::ArrayXXf>& classes, cv::Mat& img) { tdr_viz::scanPicture(classes, unflatten_lut_, color_lut_, img); }
  void publishSemanticTopDown(std::vector<Eigen::ArrayXXf>& top_down, cv::Mat& map_color) {
    visualize(top_down, map_color);   // :248
    published_ = map_color;
  }
  void publishGeometricTopDown(std::vector<Eigen::ArrayXXf>& top_down, cv::Mat& map_color) {
    visualize(top_down, map_color);   // :258
    published_ = map_color;
  }
};

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  try {
    int ncls, rows, cols, nb, nr, bg_h[2], bg_w[2];
    float pub_scale, analog_scale;
    {
      std::ifstream meta(dir + "/meta.txt");
      meta >> ncls >> rows >> cols >> nb >> nr >> pub_scale >> analog_scale >> bg_h[0] >> bg_w[0] >> bg_h[1] >> bg_w[1];
      if (!meta) throw std::runtime_error("bad meta.txt");
    }
    const auto maps = slurp<float>(dir + "/maps.bin");
    const auto mask = slurp<uint8_t>(dir + "/mask.bin");
    const auto packed = slurp<uint32_t>(dir + "/lut.bin");
    const auto unf = slurp<int32_t>(dir + "/unflatten.bin");
    Node node;
    node.color_lut_ = SemanticColorLut(packed);
    node.unflatten_lut_.assign(unf.begin(), unf.end());

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
    std::vector<std::vector<std::array<int, 4>>> arrows(2);
    for (int r = 0; r < 2; r++) {
      const auto st = slurp<State>(dir + "/states_" + std::to_string(r) + ".bin");
      const auto pts = slurp<float>(dir + "/pts_" + std::to_string(r) + ".bin");
      pcl::PointCloud<PointType>::Ptr cloud(new pcl::PointCloud<PointType>());
      for (size_t i = 0; i < pts.size() / 8; i++) {
        PointType p{};
        p.x = pts[8 * i]; p.y = pts[8 * i + 1]; p.z = pts[8 * i + 2]; p.intensity = pts[8 * i + 4];
        cloud->push_back(p);
      }
      clouds.push_back(cloud);
      const auto arr = slurp<int32_t>(dir + "/arrows_" + std::to_string(r) + ".bin");
      for (size_t i = 0; i < arr.size() / 4; i++) arrows[r].push_back({arr[4 * i], arr[4 * i + 1], arr[4 * i + 2], arr[4 * i + 3]});
      TopDownRenderCore::Config cfg;
      cfg.particle_count = (int)st.size();
      cfg.theta_bins = nb;
      cfg.range_bins = nr;
      cfg.seed = 41 + (uint32_t)r;
      auto* core = new TopDownRenderCore(cfg);
      core->initialize(&map, fp, flatten_lut);
      core->filter()->setStates(st);
      cores.push_back(core);
    }
    // robot 0 draws on a BGR image, robot 1 on a label image coloured on the device (rows padded: the packing branch)
    auto bg0 = slurp<uint8_t>(dir + "/bg_0.bin");
    cores[0]->filter()->setVizBackground(cv::Mat(bg_h[0], bg_w[0], CV_8UC3, bg0.data()));
    const auto lab1 = slurp<uint8_t>(dir + "/labels_1.bin");
    std::vector<uint8_t> padded((size_t)bg_h[1] * (bg_w[1] + 3), 0xEE);
    for (int y = 0; y < bg_h[1]; y++) std::memcpy(padded.data() + (size_t)y * (bg_w[1] + 3), lab1.data() + (size_t)y * bg_w[1], (size_t)bg_w[1]);
    cores[1]->filter()->setVizBackground(cv::Mat(bg_h[1], bg_w[1], CV_8UC1, padded.data(), (size_t)bg_w[1] + 3), node.color_lut_);

    TopDownRenderCoreBatch loop;
    const std::vector<Eigen::Vector2f> trans(2, Eigen::Vector2f(1.f, 0.f));
    const std::vector<float> yaw(2, 0.01f);
    if (!loop.takeStep(cores, clouds, trans, yaw)) throw std::runtime_error("takeStep skipped: no map");

    std::vector<tdr_viz::Image> scans, parts, parts2;
    loop.renderPictures(cores, node.unflatten_lut_, node.color_lut_, pub_scale, arrows, scans, parts);
    ParticleFilterBatch pfb;
    pfb.renderViz({cores[0]->filter(), cores[1]->filter()}, pub_scale, arrows, parts2);
    const size_t P = (size_t)nb * nr;
    for (int r = 0; r < 2; r++) {
      const std::string tag = "_" + std::to_string(r) + ".bin";
      if (scans[r].h != nr || scans[r].w != nb) throw std::runtime_error("scan picture of the wrong size");
      dump(dir + "/out_scan" + tag, scans[r].bgr.data(), scans[r].bgr.size());
      dump(dir + "/out_part" + tag, parts[r].bgr.data(), parts[r].bgr.size());
      if (parts2[r].bgr != parts[r].bgr || parts2[r].h != parts[r].h || parts2[r].w != parts[r].w)
        throw std::runtime_error("ParticleFilterBatch::renderViz and renderPictures differ");
      const int32_t hw[2] = {parts[r].h, parts[r].w};
      dump(dir + "/out_part_size" + tag, hw, sizeof(hw));
      // what the pictures are pictures of
      std::vector<float> imgs(P * ncls);
      if (tdr_renderer_get_render(cores[r]->renderer()->handle(), imgs.data(), nullptr) != TDR_OK) throw std::runtime_error(tdr_last_error());
      dump(dir + "/out_imgs" + tag, imgs.data(), imgs.size() * sizeof(float));
      const auto st = cores[r]->filter()->states();
      dump(dir + "/out_states" + tag, st.data(), st.size() * sizeof(State));
      Eigen::Vector4f best;
      cores[r]->filter()->maxLikelihood(best);
      dump(dir + "/out_best" + tag, best.data(), 4 * sizeof(float));
      // the standalone members on the same render: ScanRendererPolar::renderViz in both forms, renderVizAnalog
      std::vector<uint8_t> one;
      int h = 0, w = 0;
      cores[r]->renderer()->renderViz(node.unflatten_lut_, node.color_lut_, one, h, w);
      if (h != nr || w != nb || one != scans[r].bgr) throw std::runtime_error("ScanRendererPolar::renderViz differs from the batch");
      std::vector<uint8_t> buf((size_t)3 * nr * nb, 0);
      cv::Mat m(nr, nb, CV_8UC3, buf.data());
      cores[r]->renderer()->renderViz(node.unflatten_lut_, node.color_lut_, m);
      if (buf != one) throw std::runtime_error("ScanRendererPolar::renderViz(cv::Mat) differs");
      cores[r]->renderer()->renderVizAnalog(r, analog_scale, one, h, w);
      dump(dir + "/out_analog" + tag, one.data(), one.size());
      // the node's two call sites on host images
      std::vector<Eigen::ArrayXXf> top_down;
      for (int c = 0; c < ncls; c++) {
        Eigen::ArrayXXf a(nb, nr);
        std::memcpy(a.data(), imgs.data() + P * c, P * sizeof(float));
        top_down.push_back(a);
      }
      std::vector<uint8_t> sem((size_t)3 * nr * nb, 0), geo((size_t)3 * nr * nb, 0);
      cv::Mat map_color(nr, nb, CV_8UC3, sem.data()), geo_color(nr, nb, CV_8UC3, geo.data());
      node.publishSemanticTopDown(top_down, map_color);
      if (sem != scans[r].bgr) throw std::runtime_error("tdr_viz::scanPicture differs from the device picture");
      std::vector<Eigen::ArrayXXf> two(top_down.begin(), top_down.begin() + 2);
      node.publishGeometricTopDown(two, geo_color);
      dump(dir + "/out_geo" + tag, geo.data(), geo.size());
    }
#ifndef TDR_HAVE_OPENCV
    {   // the stand-in owns no memory: an image of another size is refused
      bool refused = false;
      std::vector<uint8_t> buf((size_t)3 * nr * nb, 0);
      cv::Mat wrong(nb, nr, CV_8UC3, buf.data());
      try {
        cores[0]->renderer()->renderViz(node.unflatten_lut_, node.color_lut_, wrong);
      } catch (const std::invalid_argument&) {
        refused = nb != nr;
      }
      if (!refused && nb != nr) throw std::runtime_error("a wrong-sized cv::Mat was accepted");
    }
#endif
    for (auto* c : cores) delete c;
    std::printf("ok %d %d\n", nr, nb);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "facade_pictures failed: %s\n", e.what());
    return 1;
  }
}
