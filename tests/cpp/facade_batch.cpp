// facade_batch.cpp — ParticleFilterBatch (include/top_down_render/particle_filter_batch.h) against standalone filters:
// three filters on one map stepped together, three twins stepped one at a time through propagate + update; the particle
// sets, weights and resample indices must be the same bits.  Prints "ok <batched> <standalone>" (counts of the last step).
#include <cstdio>
#include <cstring>
#include <random>

#include "top_down_render/particle_filter_batch.h"

int main() {
  try {
    const int ncls = 6, rows = 300, cols = 300, nb = 100, nr = 25;
    TopDownMap::Params map_params;
    map_params.num_classes = ncls;
    map_params.resolution = 1;
    for (int c = 0; c < ncls; c++) map_params.flatten_lut.push_back(c);
    TopDownMapPolar map(map_params);
    std::vector<Eigen::ArrayXXf> class_maps;
    for (int c = 0; c < ncls; c++) {
      Eigen::ArrayXXf m(rows, cols);
      for (int j = 0; j < cols; j++)
        for (int i = 0; i < rows; i++) m(i, j) = (float)((i * (c + 3) + j * (c + 1)) % 11);
      class_maps.push_back(m);
    }
    Eigen::ArrayXXc class_mask(rows, cols);
    std::memset(class_mask.data(), 0, (size_t)rows * cols);
    map.setDistanceMaps(class_maps, class_mask);
    map.samplePtsPolar(Eigen::Vector2i(nb, nr), 2 * (float)M_PI / nb);

    FilterParams fp;
    fp.pos_cov = 0.3f;
    fp.theta_cov = (float)(M_PI / 100);
    fp.regularization = 0.15f;
    fp.fixed_scale = 1.f;
    for (int c = 0; c < ncls; c++) fp.class_weights.push_back(1.f);
    fp.init_pos_m_x = 1e9f;   // the constructor's initializeParticles returns early: the particles are set below
    fp.init_pos_m_y = 1e9f;
    const int counts[3] = {300, 1000, 4096};
    std::vector<ParticleFilter*> batch, twins;
    std::mt19937 gen(5);
    std::uniform_real_distribution<float> ux(60.f, 240.f), ut(-3.f, 3.f);
    for (int k = 0; k < 3; k++) {
      std::vector<State> st((size_t)counts[k]);
      for (auto& s : st) {
        s = State{};
        s.init_x_px = ux(gen);
        s.init_y_px = ux(gen);
        s.theta = ut(gen);
        s.scale = 1.f;
        s.have_init = true;
      }
      for (auto* v : {&batch, &twins}) {
        v->push_back(new ParticleFilter(counts[k], &map, fp, 40 + k));
        v->back()->setStates(st);
      }
    }
    ParticleFilterBatch pb;
    std::uniform_int_distribution<int> cnt(0, 3);
    for (int step = 0; step < 3; step++) {
      std::vector<std::vector<Eigen::ArrayXXf>> scans(3);
      std::vector<float> res;
      std::vector<MotionPrior> priors;
      for (int k = 0; k < 3; k++) {
        for (int c = 0; c < ncls; c++) {
          Eigen::ArrayXXf img(nb, nr);
          for (int i = 0; i < nb * nr; i++) img.data()[i] = (float)(cnt(gen) == 0 ? cnt(gen) : 0);
          scans[k].push_back(img);
        }
        res.push_back(1.f + 0.1f * k);
        MotionPrior p;
        p.tx = 0.5f + 0.2f * k;
        p.ty = 0.1f * step;
        p.omega = 0.01f * (k - 1);
        priors.push_back(p);
      }
      pb.step(batch, scans, res, priors);
      std::vector<Eigen::ArrayXXf> none;
      for (int k = 0; k < 3; k++) {
        Eigen::Vector2f t(priors[k].tx, priors[k].ty);
        twins[k]->propagate(t, priors[k].omega);
        twins[k]->update(scans[k], none, res[k]);
        const int n = (int)twins[k]->numParticles();
        const auto a = batch[k]->states(), b = twins[k]->states();
        const auto wa = batch[k]->weights(n), wb = twins[k]->weights(n);
        if (a.size() != b.size() || std::memcmp(a.data(), b.data(), a.size() * sizeof(State)) != 0 ||
            std::memcmp(wa.data(), wb.data(), wa.size() * sizeof(float)) != 0) {
          std::fprintf(stderr, "filter %d differs after step %d\n", k, step);
          return 1;
        }
      }
    }
    // wrong shapes are refused before any filter moves: a missing class image, an image of the wrong size
    const auto before = batch[0]->states();
    for (int bad = 0; bad < 2; bad++) {
      std::vector<std::vector<Eigen::ArrayXXf>> scans(3);
      for (int k = 0; k < 3; k++)
        for (int c = 0; c < ncls - (bad == 0 && k == 1 ? 1 : 0); c++)
          scans[k].push_back(Eigen::ArrayXXf(nb, nr - (bad == 1 && k == 2 && c == 3 ? 1 : 0)));
      bool refused = false;
      try {
        pb.step(batch, scans, {1.f, 1.f, 1.f}, std::vector<MotionPrior>(3));
      } catch (const std::invalid_argument&) {
        refused = true;
      }
      const auto after = batch[0]->states();
      if (!refused || std::memcmp(before.data(), after.data(), before.size() * sizeof(State)) != 0) {
        std::fprintf(stderr, "wrong shape %d not refused cleanly\n", bad);
        return 1;
      }
    }
    std::printf("ok %d %d\n", pb.lastBatched(), pb.lastStandalone());
    for (auto* f : batch) delete f;
    for (auto* f : twins) delete f;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
