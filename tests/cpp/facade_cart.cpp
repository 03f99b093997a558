// facade_cart.cpp — ParticleFilterCartesian (include/top_down_render/particle_filter_cartesian.h) over a TopDownMap with
// a window (TopDownMap::setWindow), against values tests/test_cart_facade.py dumps from the Python filter on the same map,
// seed and scans: a cold-start update (every particle gets its heading from the search) and a steady-state step must end
// with the same bytes.  Usage: facade_cart <dump file>.  Prints "ok <particles>".
//
// The dump (little endian): int32 {ncls, map rows, map cols, window rows, window cols, particles, seed}, then
//   float  class maps [ncls][rows*cols] column-major, uint8 mask [rows*cols] column-major,
//   State  the particles (28 bytes each, have_init = 0),
//   float  scan 0, scan 1 [ncls][wrows*wcols] column-major, float res, float tx, ty, omega,
//   after the cold-start update: State [n], float raw weights [n], float weights [n];
//   after propagate + update:    State [n], float raw weights [n], float weights [n].
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "top_down_render/particle_filter_cartesian.h"

namespace {
template <class T>
std::vector<T> rd(std::FILE* fh, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, fh) != n) throw std::runtime_error("dump file too short");
  return v;
}
template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}
bool same_states(const std::vector<State>& a, const std::vector<State>& b) {   // field by field: padding bytes are nobody's
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (std::memcmp(&a[i], &b[i], 6 * sizeof(float)) != 0 || a[i].have_init != b[i].have_init) return false;
  return true;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return std::fprintf(stderr, "usage: facade_cart <dump file>\n"), 2;
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  try {
    const auto hd = rd<int32_t>(fh, 7);
    const int ncls = hd[0], rows = hd[1], cols = hd[2], wr = hd[3], wc = hd[4], n = hd[5];
    const uint32_t seed = (uint32_t)hd[6];
    const size_t cells = (size_t)rows * cols, P = (size_t)wr * wc;
    const auto maps = rd<float>(fh, cells * ncls);
    const auto mask = rd<uint8_t>(fh, cells);
    const auto particles = rd<State>(fh, (size_t)n);
    std::vector<std::vector<Eigen::ArrayXXf>> scans(2);
    for (auto& scan : scans)
      for (int c = 0; c < ncls; c++) {
        Eigen::ArrayXXf img(wr, wc);
        const auto px = rd<float>(fh, P);
        std::memcpy(img.data(), px.data(), P * sizeof(float));
        scan.push_back(img);
      }
    const auto motion = rd<float>(fh, 4);   // res, tx, ty, omega

    TopDownMap::Params map_params;
    map_params.num_classes = ncls;
    map_params.resolution = 1;
    TopDownMap map(map_params);
    std::vector<Eigen::ArrayXXf> class_maps;
    for (int c = 0; c < ncls; c++) {
      Eigen::ArrayXXf m(rows, cols);
      std::memcpy(m.data(), maps.data() + cells * c, cells * sizeof(float));
      class_maps.push_back(m);
    }
    Eigen::ArrayXXc class_mask(rows, cols);
    std::memcpy(class_mask.data(), mask.data(), cells);
    map.setDistanceMaps(class_maps, class_mask);

    FilterParams fp;
    fp.pos_cov = 0.3f;
    fp.theta_cov = (float)(M_PI / 100);
    fp.regularization = 0.15f;
    fp.fixed_scale = 1.f;
    fp.init_pos_m_x = 1e9f;   // the constructor's initializeParticles returns early: the particles are set below
    fp.init_pos_m_y = 1e9f;
    bool refused = false;     // no window yet: no Cartesian filter
    try {
      ParticleFilterCartesian early(n, &map, fp, seed);
    } catch (const std::runtime_error&) {
      refused = true;
    }
    if (!refused) return std::fprintf(stderr, "a map without a window was accepted\n"), 1;
    map.setWindow(wr, wc);
    if (map.windowShape()[0] != wr || map.windowShape()[1] != wc) return std::fprintf(stderr, "windowShape\n"), 1;

    ParticleFilterCartesian pf(n, &map, fp, seed);
    pf.setStates(particles);
    for (int step = 0; step < 2; step++) {
      if (step) {
        Eigen::Vector2f t(motion[1], motion[2]);
        pf.propagate(t, motion[3]);
      }
      pf.update(scans[step], motion[0]);
      const auto want_st = rd<State>(fh, (size_t)n);
      const auto want_raw = rd<float>(fh, (size_t)n), want_w = rd<float>(fh, (size_t)n);
      if (!same_states(pf.states(), want_st)) return std::fprintf(stderr, "step %d: states differ\n", step), 1;
      if (!same(pf.rawWeights(n), want_raw)) return std::fprintf(stderr, "step %d: raw weights differ\n", step), 1;
      if (!same(pf.weights(n), want_w)) return std::fprintf(stderr, "step %d: weights differ\n", step), 1;
      for (const State& s : pf.states())
        if (!s.have_init) return std::fprintf(stderr, "step %d: a particle without a heading\n", step), 1;
    }
    // an image of the wrong shape: nothing is scored, the particle set stays as it is
    const auto before = pf.states();
    std::vector<Eigen::ArrayXXf> bad;
    for (int c = 0; c < ncls; c++) bad.push_back(Eigen::ArrayXXf(wr, wc + 1));
    pf.update(bad, motion[0]);
    if (!same_states(pf.states(), before)) return std::fprintf(stderr, "a wrong-shaped scan moved the filter\n"), 1;
    Eigen::Vector4f mean;
    pf.meanLikelihood(mean);
    std::printf("ok %d\n", pf.numParticles());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  std::fclose(fh);
  return 0;
}
