// scan_viz_device.h — the node's scan images and its label background coloured on the device (include/tdr.h, "the scan
// picture"): what ScanRenderer::renderViz / renderVizAnalog, ParticleFilter::setVizBackground(labels, lut) and the batched
// pictures share, and the free function that stands in for TopDownRender::visualize (src/top_down_render.cpp:275-305):
//
//     void TopDownRender::visualize(std::vector<Eigen::ArrayXXf>& classes, cv::Mat& img) {
//       tdr_viz::scanPicture(classes, unflatten_lut_, color_lut_, img);
//     }
//
// keeps the call sites :248 and :258 as they are.  A picture is BGR8 [cols][rows][3] of the Eigen images (height = cols).
#ifndef TOP_DOWN_RENDER_SCAN_VIZ_DEVICE_H_
#define TOP_DOWN_RENDER_SCAN_VIZ_DEVICE_H_

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "tdr.h"
#include "top_down_render/particle_viz_device.h"

namespace tdr_viz {

// one published picture as bytes [h][w][3]
struct Image {
  std::vector<uint8_t> bgr;
  int h = 0, w = 0;
};

// The 256 BGR triplets of a SemanticColorLut.  With semantics_manager: a 256 x 1 index image coloured once by
// ind2Color(Mat, Mat), whatever that does per index.  In the stand-in of tdr_compat.h entry i is
// unpackColor(ind2Color(i)) read as {B, G, R}.
inline std::array<uint8_t, 768> colourTable(const SemanticColorLut& lut) {
  std::array<uint8_t, 768> t{};
#ifdef TDR_HAVE_SEMANTICS_MANAGER
  cv::Mat idx(256, 1, CV_8UC1), col;
  for (int i = 0; i < 256; i++) idx.at<uint8_t>(i, 0) = (uint8_t)i;
  const_cast<SemanticColorLut&>(lut).ind2Color(idx, col);   // (whether it is a const member is not visible from the node's source)
  for (int i = 0; i < 256; i++) std::memcpy(&t[3 * (size_t)i], col.ptr<uint8_t>(i), 3);
#else
  for (int i = 0; i < 256; i++) {
    const std::array<uint8_t, 3> c = SemanticColorLut::unpackColor(lut.ind2Color(i));
    t[3 * (size_t)i] = c[0];
    t[3 * (size_t)i + 1] = c[1];
    t[3 * (size_t)i + 2] = c[2];
  }
#endif
  return t;
}

inline std::vector<int32_t> unflattenTable(const std::vector<int>& unflatten_lut, int ncls, const char* who) {
  if ((int)unflatten_lut.size() < ncls)
    throw std::invalid_argument(std::string(who) + ": unflatten_lut has " + std::to_string(unflatten_lut.size()) +
                                " entries, the images " + std::to_string(ncls) + " classes");
  return std::vector<int32_t>(unflatten_lut.begin(), unflatten_lut.begin() + ncls);
}

// The h x w image a picture is written into.  OpenCV's Mat is (re)allocated as CV_8UC3; the stand-in of tdr_compat.h owns
// no memory, so the caller hands one of that size (three channels, continuous rows).
template <class MatT>
uint8_t* pictureTarget(MatT& img, int h, int w, const char* who) {
#ifdef TDR_HAVE_OPENCV
  img.create(h, w, 16);   // CV_8UC3 = CV_MAKETYPE(CV_8U, 3)
#else
  if (img.empty() || img.rows != h || img.cols != w || img.channels() != 3 || !img.isContinuous())
    throw std::invalid_argument(std::string(who) + ": the image must be " + std::to_string(h) + " x " + std::to_string(w) +
                                " pixels of three channels");
#endif
  return img.template ptr<uint8_t>();
}

// TopDownRender::visualize for images the caller holds on the host: the semantic render, the geometric render's two layers
inline void scanPicture(const std::vector<Eigen::ArrayXXf>& classes, const std::vector<int>& unflatten_lut,
                        const SemanticColorLut& lut, uint8_t* out_bgr /* [cols][rows][3] */) {
  if (classes.empty()) throw std::invalid_argument("scanPicture: no images");
  const int ncls = (int)classes.size(), rows = (int)classes[0].rows(), cols = (int)classes[0].cols();
  const size_t P = (size_t)rows * cols;
  std::vector<float> buf(P * ncls);
  for (int c = 0; c < ncls; c++) {
    if (classes[c].rows() != rows || classes[c].cols() != cols) throw std::invalid_argument("scanPicture: images of different sizes");
    std::memcpy(buf.data() + P * c, classes[c].data(), P * sizeof(float));
  }
  const std::vector<int32_t> unf = unflattenTable(unflatten_lut, ncls, "scanPicture");
  const std::array<uint8_t, 768> table = colourTable(lut);
  if (tdr_scan_picture_host(buf.data(), ncls, rows, cols, unf.data(), table.data(), out_bgr) != TDR_OK) fail("scanPicture");
}
template <class MatT>
void scanPicture(const std::vector<Eigen::ArrayXXf>& classes, const std::vector<int>& unflatten_lut, const SemanticColorLut& lut,
                 MatT& img) {
  if (classes.empty()) throw std::invalid_argument("scanPicture: no images");
  scanPicture(classes, unflatten_lut, lut, pictureTarget(img, (int)classes[0].cols(), (int)classes[0].rows(), "scanPicture"));
}
inline void scanPicture(const std::vector<Eigen::ArrayXXf>& classes, const std::vector<int>& unflatten_lut,
                        const SemanticColorLut& lut, Image& img) {
  if (classes.empty()) throw std::invalid_argument("scanPicture: no images");
  img.h = (int)classes[0].cols();
  img.w = (int)classes[0].rows();
  img.bgr.resize((size_t)3 * img.h * img.w);
  scanPicture(classes, unflatten_lut, lut, img.bgr.data());
}

// the scan picture / one analog layer of a renderer's last semantic render, drawn from the device images
inline void rendererPictureSize(const tdr_renderer* r, int& h, int& w) {
  if (tdr_renderer_visualize(r, nullptr, nullptr, nullptr, 0, &h, &w) != TDR_OK) fail("renderViz");
}
inline void rendererPicture(const tdr_renderer* r, const std::vector<int>& unflatten_lut, const SemanticColorLut& lut,
                            uint8_t* out, int h, int w) {
  std::vector<int32_t> unf(unflatten_lut.begin(), unflatten_lut.end());
  unf.resize(std::max<size_t>(unf.size(), TDR_MAX_CLASSES), 255);   // (the handle reads the render's class count of them)
  const std::array<uint8_t, 768> table = colourTable(lut);
  if (tdr_renderer_visualize(r, unf.data(), table.data(), out, (int64_t)3 * h * w, &h, &w) != TDR_OK) fail("renderViz");
}
inline void rendererAnalogSize(const tdr_renderer* r, int cls, float scale, int& h, int& w) {
  if (tdr_renderer_visualize_analog(r, cls, scale, nullptr, 0, &h, &w) != TDR_OK) fail("renderVizAnalog");
}
inline void rendererAnalog(const tdr_renderer* r, int cls, float scale, uint8_t* out, int h, int w) {
  if (tdr_renderer_visualize_analog(r, cls, scale, out, (int64_t)3 * h * w, &h, &w) != TDR_OK) fail("renderVizAnalog");
}

// the particle picture's background from the label image the node colours (aerialMapCallback, :584): labels is an 8-bit
// image of one channel
inline int setBackgroundLabelBytes(tdr_filter* f, const uint8_t* labels, int h, int w, const uint8_t* table) {
  return tdr_filter_set_viz_background_labels(f, labels, h, w, table);
}
inline int setBackgroundLabelBytes(tdr_map* m, const uint8_t* labels, int h, int w, const uint8_t* table) {
  return tdr_map_set_viz_background_labels(m, labels, h, w, table);
}
template <class HandleT, class MatT>
void setBackgroundLabels(HandleT* owner, const MatT& labels, const SemanticColorLut& lut) {
  if (labels.empty() || labels.channels() != 1 || labels.elemSize() != 1)
    throw std::invalid_argument("setVizBackground: an 8-bit label image of one channel is needed");
  const std::array<uint8_t, 768> table = colourTable(lut);
  if (labels.isContinuous()) {
    if (setBackgroundLabelBytes(owner, labels.template ptr<uint8_t>(), labels.rows, labels.cols, table.data()) != TDR_OK)
      fail("setVizBackground");
    return;
  }
  std::vector<uint8_t> packed((size_t)labels.rows * labels.cols);
  for (int r = 0; r < labels.rows; r++)
    std::memcpy(packed.data() + (size_t)r * labels.cols, labels.template ptr<uint8_t>(r), (size_t)labels.cols);
  if (setBackgroundLabelBytes(owner, packed.data(), labels.rows, labels.cols, table.data()) != TDR_OK)
    fail("setVizBackground");
}

// the particle pictures of many filters in one tdr_batch_visualize; arrows: empty, or one list per filter
inline void renderBatch(const std::vector<tdr_filter*>& filters, float pub_scale,
                        const std::vector<std::vector<std::array<int, 4>>>& arrows, std::vector<Image>& outs, void* stream) {
  static_assert(sizeof(std::array<int, 4>) == 4 * sizeof(int32_t), "arrows are int32 [m][4]");
  const size_t k = filters.size();
  if (!arrows.empty() && arrows.size() != k) throw std::invalid_argument("renderViz: one arrow list per filter (or none at all)");
  std::vector<tdr_viz_request> req(k);
  for (size_t i = 0; i < k; i++) {
    req[i] = tdr_viz_request{};
    if (!arrows.empty() && !arrows[i].empty()) {
      req[i].extra_arrows = reinterpret_cast<const int32_t*>(arrows[i].data());
      req[i].m = (int32_t)arrows[i].size();
    }
  }
  if (tdr_batch_visualize(filters.data(), (int)k, pub_scale, req.data(), stream) != TDR_OK) fail("renderViz");   // the sizes
  outs.resize(k);
  for (size_t i = 0; i < k; i++) {
    outs[i].h = req[i].out_h;
    outs[i].w = req[i].out_w;
    outs[i].bgr.resize((size_t)3 * outs[i].h * outs[i].w);
    req[i].out_bgr_host = outs[i].bgr.data();
    req[i].capacity = (int64_t)outs[i].bgr.size();
  }
  if (tdr_batch_visualize(filters.data(), (int)k, pub_scale, req.data(), stream) != TDR_OK) fail("renderViz");
}

// One robot's colours in the fleet picture (include/tdr.h): BGR of its particle arrows, its border dots, its estimate
// (mixture and max-likelihood arrow).  classic() is what renderViz draws one robot with.
struct FleetColours {
  std::array<uint8_t, 3> arrows, dots, estimate;
  static FleetColours classic() { return FleetColours{{0, 0, 255}, {0, 255, 0}, {255, 0, 0}}; }
};
// the fleet picture of filters on one map, over the background the map holds, in one tdr_batch_visualize_fleet
inline void renderFleet(const std::vector<tdr_filter*>& filters, float pub_scale, const std::vector<FleetColours>& palette,
                        const std::vector<std::array<int, 4>>& arrows, Image& out, void* stream) {
  static_assert(sizeof(std::array<int, 4>) == 4 * sizeof(int32_t), "arrows are int32 [m][4]");
  static_assert(sizeof(FleetColours) == 9, "the palette is uint8 [k][3][3]");
  if (palette.size() != filters.size()) throw std::invalid_argument("renderFleet: one FleetColours per filter");
  const int32_t* a = arrows.empty() ? nullptr : reinterpret_cast<const int32_t*>(arrows.data());
  const uint8_t* pal = palette.empty() ? nullptr : reinterpret_cast<const uint8_t*>(palette.data());
  if (tdr_batch_visualize_fleet(filters.data(), (int)filters.size(), pub_scale, pal, a, (int)arrows.size(), nullptr, 0, &out.h,
                                &out.w, stream) != TDR_OK)
    fail("renderFleet");
  out.bgr.resize((size_t)3 * out.h * out.w);
  if (tdr_batch_visualize_fleet(filters.data(), (int)filters.size(), pub_scale, pal, a, (int)arrows.size(), out.bgr.data(),
                                (int64_t)out.bgr.size(), &out.h, &out.w, stream) != TDR_OK)
    fail("renderFleet");
}

}  // namespace tdr_viz

#endif  // TOP_DOWN_RENDER_SCAN_VIZ_DEVICE_H_
