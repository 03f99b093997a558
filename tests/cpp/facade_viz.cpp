// facade_viz.cpp — setVizBackground / renderViz of ParticleFilter and ParticleFilterCartesian
// (include/top_down_render/particle_viz_device.h) against images tests/test_viz.py wrote from the Python filter on the same
// particles, background and arrows.  Usage: facade_viz <dump file>.  Prints "ok <out_h> <out_w>".
//
// The dump (little endian): int32 {ncls, map rows, map cols, particles, H, W, arrows, out_h, out_w}, float pub_scale, then
//   float  class maps [ncls][rows*cols] column-major, uint8 mask [rows*cols] column-major,
//   State  the particles (28 bytes each), uint8 background [H][W][3], int32 arrows [m][4],
//   uint8  the published image [out_h][out_w][3], uint8 the image at scale 1 without arrows [H][W][3].
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "top_down_render/particle_filter.h"
#include "top_down_render/particle_filter_cartesian.h"

namespace {
template <class T>
std::vector<T> rd(std::FILE* fh, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, fh) != n) throw std::runtime_error("dump file too short");
  return v;
}

// both classes: the published image through the vector overload and through cv::Mat, the plain image without arrows
template <class Filter>
int check(Filter& pf, const std::vector<State>& particles, std::vector<uint8_t>& bg, int H, int W, float scale,
          const std::vector<std::array<int, 4>>& arrows, const std::vector<uint8_t>& want, int oh, int ow,
          const std::vector<uint8_t>& want_plain, const char* who) {
  pf.setStates(particles);
  bool refused = false;   // no background yet
  std::vector<uint8_t> img;
  int h = 0, w = 0;
  try {
    pf.renderViz(img, h, w, scale, arrows);
  } catch (const std::runtime_error&) {
    refused = true;
  }
  if (!refused) return std::fprintf(stderr, "%s: a picture without a background\n", who), 1;
  // a background with padded rows goes through the packing branch
  std::vector<uint8_t> padded((size_t)H * (3 * W + 5), 0xEE);
  for (int r = 0; r < H; r++) std::memcpy(padded.data() + (size_t)r * (3 * W + 5), bg.data() + (size_t)r * 3 * W, (size_t)3 * W);
  pf.setVizBackground(cv::Mat(H, W, CV_8UC3, padded.data(), (size_t)3 * W + 5));
  pf.renderViz(img, h, w, scale, arrows);
  if (h != oh || w != ow || img != want) return std::fprintf(stderr, "%s: the published image differs\n", who), 1;
  pf.setVizBackground(cv::Mat(H, W, CV_8UC3, bg.data()));
  std::vector<uint8_t> buf((size_t)3 * oh * ow, 0);
  cv::Mat out(oh, ow, CV_8UC3, buf.data());
  pf.renderViz(out, scale, arrows);
  if (buf != want) return std::fprintf(stderr, "%s: the cv::Mat image differs\n", who), 1;
  std::vector<uint8_t> plain((size_t)3 * H * W, 0);
  cv::Mat out1(H, W, CV_8UC3, plain.data());
  pf.renderViz(out1, 1.f);
  if (plain != want_plain) return std::fprintf(stderr, "%s: the image without arrows differs\n", who), 1;
#ifndef TDR_HAVE_OPENCV
  refused = false;        // the stand-in owns no memory: an image of another size is refused
  try {
    pf.renderViz(out1, 0.5f);
  } catch (const std::invalid_argument&) {
    refused = true;
  }
  if (!refused) return std::fprintf(stderr, "%s: a wrong-sized cv::Mat was accepted\n", who), 1;
#endif
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return std::fprintf(stderr, "usage: facade_viz <dump file>\n"), 2;
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  try {
    const auto hd = rd<int32_t>(fh, 9);
    const int ncls = hd[0], rows = hd[1], cols = hd[2], n = hd[3], H = hd[4], W = hd[5], m = hd[6], oh = hd[7], ow = hd[8];
    const float scale = rd<float>(fh, 1)[0];
    const size_t cells = (size_t)rows * cols;
    const auto maps = rd<float>(fh, cells * ncls);
    const auto mask = rd<uint8_t>(fh, cells);
    const auto particles = rd<State>(fh, (size_t)n);
    auto bg = rd<uint8_t>(fh, (size_t)3 * H * W);
    const auto arr = rd<int32_t>(fh, (size_t)4 * m);
    const auto want = rd<uint8_t>(fh, (size_t)3 * oh * ow);
    const auto want_plain = rd<uint8_t>(fh, (size_t)3 * H * W);
    std::vector<std::array<int, 4>> arrows;
    for (int i = 0; i < m; i++) arrows.push_back({arr[4 * i], arr[4 * i + 1], arr[4 * i + 2], arr[4 * i + 3]});

    std::vector<Eigen::ArrayXXf> class_maps;
    for (int c = 0; c < ncls; c++) {
      Eigen::ArrayXXf cm(rows, cols);
      std::memcpy(cm.data(), maps.data() + cells * c, cells * sizeof(float));
      class_maps.push_back(cm);
    }
    Eigen::ArrayXXc class_mask(rows, cols);
    std::memcpy(class_mask.data(), mask.data(), cells);
    FilterParams fp;
    fp.pos_cov = 0.3f;
    fp.theta_cov = (float)(M_PI / 100);
    fp.regularization = 0.15f;
    fp.fixed_scale = 1.f;
    fp.init_pos_m_x = 1e9f;   // the constructor's initializeParticles returns early: the particles are set below
    fp.init_pos_m_y = 1e9f;

    TopDownMap::Params map_params;
    map_params.num_classes = ncls;
    map_params.resolution = 1;
    TopDownMapPolar polar_map(map_params);
    polar_map.setDistanceMaps(class_maps, class_mask);
    polar_map.samplePtsPolar(Eigen::Vector2i(16, 8), (float)(2 * M_PI / 16));
    ParticleFilter pf(n, &polar_map, fp, 3);
    if (check(pf, particles, bg, H, W, scale, arrows, want, oh, ow, want_plain, "ParticleFilter")) return 1;

    TopDownMap cart_map(map_params);
    cart_map.setDistanceMaps(class_maps, class_mask);
    cart_map.setWindow(8, 8);
    ParticleFilterCartesian pc(n, &cart_map, fp, 3);
    if (check(pc, particles, bg, H, W, scale, arrows, want, oh, ow, want_plain, "ParticleFilterCartesian")) return 1;
    std::printf("ok %d %d\n", oh, ow);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  std::fclose(fh);
  return 0;
}
