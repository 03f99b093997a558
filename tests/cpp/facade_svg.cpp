// facade_svg.cpp — TopDownMap's constructor on a static vector map (reference: src/top_down_map.cpp:9-64 with a .svg
// map_path): the first construction parses, fills, writes <stem>_raster_cache/class<i>.png and the map cache; the
// second hits the cache (the SVG is moved away meanwhile) and holds the same map; a file that does not parse leaves the
// map empty and writes nothing.  argv: svg, cache dir, bad svg, cache dir for the bad one (tests/test_svg_map.py).
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
  // packed colours of LUT indices 0..5: the SVG keys of #ff0000, green, #00ff00, #0000ff, black / none, grey
  p.color_lut.setColors({0x0000ffu, 0x008000u, 0x00ff00u, 0xff0000u, 0x000000u, 0x808080u});
  p.flatten_lut = {1, 2, 2, 3, 0, 3};
  p.num_classes = 4;
  p.exclusive_classes = {0, 0, 0, 0, 2, 3};   // the node's form: num_classes zeros, then the exclusive classes
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

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const std::string svg = argv[1], cache = argv[2], bad = argv[3], bad_cache = argv[4];
  std::vector<float> first;
  {
    TopDownMap m(params(svg), cache.c_str());
    CHECK(m.haveMap());
    CHECK(m.size()[0] == 240 && m.size()[1] == 180);
    first = windows(m);
  }
  CHECK(std::fopen((cache + "/cached_data.txt").c_str(), "r") != nullptr);
  CHECK(std::rename(svg.c_str(), (svg + ".away").c_str()) == 0);
  {
    TopDownMap m(params(svg), cache.c_str());   // the cache matches (map_path, num_classes, resolution): no parse
    CHECK(m.haveMap());
    CHECK(windows(m) == first);
  }
  CHECK(std::rename((svg + ".away").c_str(), svg.c_str()) == 0);
  {
    TopDownMap m(params(bad), bad_cache.c_str());
    CHECK(!m.haveMap());
    CHECK(std::string(tdr_last_error()).find("size") != std::string::npos);
  }
  std::printf("%s\n", fails ? "facade_svg FAILED" : "facade_svg ok");
  return fails ? 1 : 0;
}
