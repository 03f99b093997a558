// facade_color_png.cpp — TopDownMap's constructor on a static colour raster map (reference: src/top_down_map.cpp:9-64
// with a .png map_path): the first construction decodes the PNG, looks the colours up, builds the distance maps and
// writes the map cache (no raster cache on this branch); the second hits the cache (the PNG is moved away meanwhile) and
// holds the same map; a corrupt PNG leaves the map empty and writes nothing; a .jpg stays empty and says why.  Also the
// BGR entry point (loadColorRasterMap) on the pixels of the same map.
// argv: png, cache dir, corrupt png, its cache dir, jpg, its cache dir (tests/test_color_map.py).
#include <cstdio>
#include <string>
#include <vector>

#include "top_down_render/top_down_map.h"

static int fails = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      fails++;                                                  \
    }                                                           \
  } while (0)

static TopDownMap::Params params(const std::string& path) {
  TopDownMap::Params p;
  p.map_path = path;
  // packed colours of LUT indices 0..5 (unpackColor gives B, G, R): RGB red, dark green, green, blue, black, grey
  p.color_lut.setColors({0x0000ffu, 0x008000u, 0x00ff00u, 0xff0000u, 0x000000u, 0x808080u});
  p.flatten_lut = {1, 2, 2, 3, 0, 3};
  p.num_classes = 4;
  p.exclusive_classes = {0, 0, 0, 0, 2, 3};   // not applied on this branch (loadCompressedRasterMap)
  p.resolution = 1.f;
  return p;
}

static std::vector<float> windows(TopDownMap& m) {
  std::vector<float> out;
  for (float cx : {30.f, 120.f, 200.f}) {
    std::vector<Eigen::ArrayXXf> d(4, Eigen::ArrayXXf(50, 60));
    Eigen::ArrayXXc mask(50, 60);
    m.getLocalMap(Eigen::Vector2f(cx, 90.f), 0.3f, 1.f, d, mask);
    for (auto& a : d) out.insert(out.end(), a.data(), a.data() + a.size());
    for (int k = 0; k < (int)mask.size(); k++) out.push_back(mask.data()[k]);
  }
  return out;
}

static bool exists(const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "r");
  if (f) std::fclose(f);
  return f != nullptr;
}

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const std::string png = argv[1], cache = argv[2], bad = argv[3], bad_cache = argv[4], jpg = argv[5],
                    jpg_cache = argv[6];
  std::vector<float> first;
  std::vector<uint8_t> bgr;
  {
    TopDownMap m(params(png), cache.c_str());
    CHECK(m.haveMap());
    CHECK(m.size()[0] == 240 && m.size()[1] == 180);
    std::vector<int> classes;
    m.getClassesAtPoint(Eigen::Vector2i(5, 5), classes);
    CHECK(classes.size() <= 1);
    first = windows(m);
    int w = 0, h = 0;
    CHECK(tdr_png_read_color_host(png.c_str(), nullptr, 0, &w, &h) != TDR_OK && w == 240 && h == 180);
    bgr.resize((size_t)w * h * 3);
    CHECK(tdr_png_read_color_host(png.c_str(), bgr.data(), (int64_t)bgr.size(), &w, &h) == TDR_OK);
  }
  CHECK(exists(cache + "/cached_data.txt") && exists(cache + "/class_map3.eig") && exists(cache + "/geo_map1.eig"));
  CHECK(!exists(png.substr(0, png.size() - 4) + "_raster_cache/class0.png"));
  CHECK(std::rename(png.c_str(), (png + ".away").c_str()) == 0);
  {
    TopDownMap m(params(png), cache.c_str());   // the cache matches (map_path, num_classes, resolution): no decode
    CHECK(m.haveMap());
    CHECK(windows(m) == first);
  }
  CHECK(std::rename((png + ".away").c_str(), png.c_str()) == 0);
  {
    TopDownMap m(params(""));                   // the dynamic-map case, then the caller's own decoded pixels
    CHECK(!m.haveMap());
    m.loadColorRasterMap(cv::Mat(180, 240, CV_8UC3, bgr.data()));
    CHECK(m.haveMap());
    CHECK(windows(m) == first);
    bool threw = false;
    try {
      m.loadColorRasterMap(cv::Mat(180, 240, bgr.data()));   // one channel: refused
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    CHECK(threw);
    CHECK(windows(m) == first);
  }
  {
    TopDownMap m(params(bad), bad_cache.c_str());
    CHECK(!m.haveMap());
    CHECK(std::string(tdr_last_error()).find("png") != std::string::npos);
  }
  {
    TopDownMap m(params(jpg), jpg_cache.c_str());
    CHECK(!m.haveMap());
    CHECK(std::string(tdr_last_error()).find("JPEG maps are not decoded") != std::string::npos);
    CHECK(std::string(tdr_last_error()).find("loadColorRasterMap") != std::string::npos);
  }
  CHECK(!exists(bad_cache + "/cached_data.txt") && !exists(jpg_cache + "/cached_data.txt"));
  std::printf("%s\n", fails ? "facade_color_png FAILED" : "facade_color_png ok");
  return fails ? 1 : 0;
}
