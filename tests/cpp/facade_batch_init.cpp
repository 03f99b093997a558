// facade_batch_init.cpp — ParticleFilterBatch with the init search in the batch (setInitSearchInBatch): four cold-started
// filters (no particle has a heading) on one map stepped together, four twins stepped one at a time through propagate +
// update; no filter may take its standalone calls, not at step 0 either, and the particle sets and weights must be the
// same bits.  Prints "ok <batched> <standalone>" (counts of step 0).
#include <cstdio>
#include <cstring>
#include <random>

#include "top_down_render/particle_filter_batch.h"

int main() {
  try {
    const int ncls = 6, rows = 300, cols = 300, nb = 100, nr = 25, K = 4;
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
    const int counts[K] = {300, 1000, 4096, 9000};
    std::vector<ParticleFilter*> batch, twins;
    std::mt19937 gen(7);
    std::uniform_real_distribution<float> ux(60.f, 240.f);
    for (int k = 0; k < K; k++) {
      std::vector<State> st((size_t)counts[k]);
      for (auto& s : st) {
        s = State{};
        s.init_x_px = ux(gen);
        s.init_y_px = ux(gen);
        s.theta = 0.f;
        s.scale = 1.f;
        s.have_init = false;   // a cold start: the first update searches the 40 rotations
      }
      for (auto* v : {&batch, &twins}) {
        v->push_back(new ParticleFilter(counts[k], &map, fp, 50 + k));
        v->back()->setStates(st);
      }
    }
    if (ParticleFilterBatch::initSearchInBatch()) {
      std::fprintf(stderr, "the switch is on by default\n");
      return 1;
    }
    ParticleFilterBatch::setInitSearchInBatch(true);
    if (!ParticleFilterBatch::initSearchInBatch()) {
      std::fprintf(stderr, "the switch did not take\n");
      return 1;
    }
    ParticleFilterBatch pb;
    std::uniform_int_distribution<int> cnt(0, 3);
    int batched0 = -1, standalone0 = -1;
    for (int step = 0; step < 3; step++) {
      std::vector<std::vector<Eigen::ArrayXXf>> scans(K);
      std::vector<float> res;
      std::vector<MotionPrior> priors;
      for (int k = 0; k < K; k++) {
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
      if (step == 0) { batched0 = pb.lastBatched(); standalone0 = pb.lastStandalone(); }
      if (pb.lastStandalone() != 0 || pb.lastBatched() != K) {
        std::fprintf(stderr, "step %d: %d batched, %d standalone\n", step, pb.lastBatched(), pb.lastStandalone());
        return 1;
      }
      std::vector<Eigen::ArrayXXf> none;
      for (int k = 0; k < K; k++) {
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
        if (step == 0) {   // the search ran: every particle has a heading now, and not all the same one
          bool all_init = true, distinct = false;
          for (const auto& s : a) { all_init &= s.have_init; distinct |= s.theta != a[0].theta; }
          if (!all_init || !distinct) {
            std::fprintf(stderr, "filter %d: the search left no headings\n", k);
            return 1;
          }
        }
      }
    }
    ParticleFilterBatch::setInitSearchInBatch(false);
    std::printf("ok %d %d\n", batched0, standalone0);
    for (auto* f : batch) delete f;
    for (auto* f : twins) delete f;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
