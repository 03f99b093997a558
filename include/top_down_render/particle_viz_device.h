// particle_viz_device.h — the particle picture drawn on the device (include/tdr.h, "the particle picture"): what
// ParticleFilter::setVizBackground / renderViz and ParticleFilterCartesian's pair share.  The node's per-scan drawing
// (src/top_down_render.cpp:430-449: clone the background, visualize, the ground-truth arrow, resize) becomes one call
// that returns the published image; visualize(cv::Mat&) and its host snapshot stay as they are.
#ifndef TOP_DOWN_RENDER_PARTICLE_VIZ_DEVICE_H_
#define TOP_DOWN_RENDER_PARTICLE_VIZ_DEVICE_H_

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "tdr.h"
#include "top_down_render/tdr_compat.h"

namespace tdr_viz {

[[noreturn]] inline void fail(const char* what) { throw std::runtime_error(std::string(what) + ": " + tdr_last_error()); }

// bgr: an 8-bit image of three channels (B, G, R), the one the node draws on.  (Templates on the image type, like the
// members that call them: they are compiled only where a host uses them.)
// The owner is a filter (its own background, the particle picture's) or a map (one background for every filter on it, the
// fleet picture's).
inline int setBackgroundBytes(tdr_filter* f, const uint8_t* bgr, int h, int w) { return tdr_filter_set_viz_background(f, bgr, h, w); }
inline int setBackgroundBytes(tdr_map* m, const uint8_t* bgr, int h, int w) { return tdr_map_set_viz_background(m, bgr, h, w); }
template <class HandleT, class MatT>
void setBackground(HandleT* owner, const MatT& bgr) {
  if (bgr.empty() || bgr.channels() != 3 || bgr.elemSize() != 3)
    throw std::invalid_argument("setVizBackground: an 8-bit image of three channels is needed");
  if (bgr.isContinuous()) {
    if (setBackgroundBytes(owner, bgr.template ptr<uint8_t>(), bgr.rows, bgr.cols) != TDR_OK) fail("setVizBackground");
    return;
  }
  std::vector<uint8_t> packed((size_t)bgr.rows * bgr.cols * 3);
  for (int r = 0; r < bgr.rows; r++)
    std::memcpy(packed.data() + (size_t)r * bgr.cols * 3, bgr.template ptr<uint8_t>(r), (size_t)bgr.cols * 3);
  if (setBackgroundBytes(owner, packed.data(), bgr.rows, bgr.cols) != TDR_OK) fail("setVizBackground");
}

// the published image as bytes [out_h][out_w][3]
inline void render(tdr_filter* f, std::vector<uint8_t>& out, int& out_h, int& out_w, float pub_scale,
                   const std::vector<std::array<int, 4>>& arrows) {
  static_assert(sizeof(std::array<int, 4>) == 4 * sizeof(int32_t), "arrows are int32 [m][4]");
  const int32_t* a = arrows.empty() ? nullptr : reinterpret_cast<const int32_t*>(arrows.data());
  if (tdr_filter_visualize(f, pub_scale, a, (int)arrows.size(), nullptr, 0, &out_h, &out_w) != TDR_OK) fail("renderViz");
  out.resize((size_t)3 * out_h * out_w);
  if (tdr_filter_visualize(f, pub_scale, a, (int)arrows.size(), out.data(), (int64_t)out.size(), &out_h, &out_w) != TDR_OK)
    fail("renderViz");
}

// ... into a cv::Mat.  OpenCV's Mat is (re)allocated as CV_8UC3; the stand-in of tdr_compat.h owns no memory, so the
// caller hands one of the published size (three channels, continuous rows)
template <class MatT>
void render(tdr_filter* f, MatT& out, float pub_scale, const std::vector<std::array<int, 4>>& arrows) {
  static_assert(sizeof(std::array<int, 4>) == 4 * sizeof(int32_t), "arrows are int32 [m][4]");
  const int32_t* a = arrows.empty() ? nullptr : reinterpret_cast<const int32_t*>(arrows.data());
  int oh = 0, ow = 0;
  if (tdr_filter_visualize(f, pub_scale, a, (int)arrows.size(), nullptr, 0, &oh, &ow) != TDR_OK) fail("renderViz");
#ifdef TDR_HAVE_OPENCV
  out.create(oh, ow, 16);   // CV_8UC3 = CV_MAKETYPE(CV_8U, 3)
#else
  if (out.empty() || out.rows != oh || out.cols != ow || out.channels() != 3 || !out.isContinuous())
    throw std::invalid_argument("renderViz: the image must be " + std::to_string(oh) + " x " + std::to_string(ow) +
                                " pixels of three channels");
#endif
  if (tdr_filter_visualize(f, pub_scale, a, (int)arrows.size(), out.template ptr<uint8_t>(), (int64_t)3 * oh * ow, &oh, &ow) != TDR_OK)
    fail("renderViz");
}

}  // namespace tdr_viz

#endif  // TOP_DOWN_RENDER_PARTICLE_VIZ_DEVICE_H_
