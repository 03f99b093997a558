// tdr_host_filter.cpp — ParticleFilter behind tdr_filter_*: create (polar, Cartesian, sharded), particle
// initialisation, the generator's hand-over between host and device, propagate, update / update_geo /
// compute_weights, resample, pose statistics, freezeScale, the host mixture fit, the particle picture, updateMap.
#include "tdr_host.h"

namespace tdrh {
// the generator's stream continues on the device / on the host (see tdr_filter::rng_dev)
bool rng_on_device(const tdr_filter* f) { return f->pipe && tdr_rng_pipe_on_device(f->pipe); }
int rng_to_device(tdr_filter* f) {
  if (rng_on_device(f)) return TDR_OK;
  if (!f->pipe) TTRY(tdr_rng_pipe_create(f->n_max, &f->pipe));
  return tdr_rng_pipe_from_host(f->pipe, f->rng, f->stream);
}
int rng_to_host(tdr_filter* f) {
  if (!rng_on_device(f)) return TDR_OK;
  return tdr_rng_pipe_to_host(f->pipe, f->rng, f->stream);
}
bool rng_device_capable(const tdr_filter* f) { return f->rng_owned && f->parity_rng; }

// The current particle set of ALL ranks as a plain SoA (pose statistics, the mixture fit): the filter's own arrays when
// it is not sharded, else one all-gather of the state planes.
int filter_global_states(tdr_filter* f, const float** st, int64_t* cap) {
  if (!f->comm) {
    *st = f->st.p;
    *cap = f->cap;
    return TDR_OK;
  }
  const int64_t nl = f->nl();
  for (int k = 0; k < TDR_ST_FIELDS; k++)
    HTRY(hipMemcpyAsync(f->st_send.p + (size_t)k * nl, f->st.p + (size_t)k * f->cap, (size_t)nl * sizeof(float),
                        hipMemcpyDeviceToDevice, f->stream));
  TTRY(tdr_comm_all_gather(f->comm, f->st_send.p, f->st_all.p, (size_t)TDR_ST_FIELDS * nl * sizeof(float), f->stream));
  TTRY(tdr_k_unshard_states(f->st_all.p, f->world, nl, f->st_glob.p, f->n_max, f->stream));
  *st = f->st_glob.p;
  *cap = f->n_max;
  return TDR_OK;
}
}  // namespace tdrh

extern "C" {

// ---- ParticleFilter ------------------------------------------------------------------------------------------------------
static int filter_create(tdr_map* map, int n_max, const tdr_filter_params* fp, uint32_t seed, tdr_comm* comm,
                         tdr_filter** out) {
  if (!map || !fp || !out || n_max < 1) return failh(TDR_ERR_ARG, "filter_create: bad arguments");
  const int world = comm ? tdr_comm_world(comm) : 1;
  if (n_max % world) return failh(TDR_ERR_ARG, "filter_create: n_max = %d is not a multiple of the %d ranks", n_max, world);
  tdr_filter* f = new tdr_filter();
  f->map = map;
  f->fp = *fp;
  f->n_max = n_max;
  f->comm = comm;
  f->world = world;
  f->rank = comm ? tdr_comm_rank(comm) : 0;
  f->cap = n_max / world;
  f->seed = seed;
  f->rng = tdr_rng_create(seed);  // explicit seed instead of std::random_device (particle_filter.cpp:4-5)
  // seed 0 = "unseeded", like the reference's std::random_device: nothing to reproduce, so propagate draws its noise on
  // the device; a non-zero seed asks for the reference-ordered std::mt19937 stream (tdr_filter_configure overrides)
  f->parity_rng = seed != 0;
  int rc = TDR_OK;
  const size_t cap = (size_t)f->cap, N = (size_t)n_max;
  if (rc == TDR_OK) rc = f->st.resize(TDR_ST_FIELDS * cap);
  if (rc == TDR_OK) rc = f->st_new.resize(TDR_ST_FIELDS * cap);
  if (rc == TDR_OK) rc = f->last_dist.resize(cap);
  if (rc == TDR_OK) rc = f->raw_w.resize(cap);
  if (rc == TDR_OK) rc = f->w.resize(N);
  if (rc == TDR_OK) rc = f->runmax.resize(N);
  if (rc == TDR_OK) rc = f->pfx_ws.resize((size_t)tdr_prefix_workspace_bytes((int64_t)N));
  if (rc == TDR_OK) rc = f->idx.resize(cap);
  if (rc == TDR_OK) rc = f->perm.resize(cap);
  if (rc == TDR_OK) rc = f->info.resize(TDR_UW_INFO_FLOATS);
  if (rc == TDR_OK) rc = f->stats.resize(TDR_MEAN_COV_FLOATS);
  if (rc == TDR_OK) rc = f->aos.resize(N);
  if (rc == TDR_OK) rc = f->z4.resize(4 * cap);
  if (rc == TDR_OK && comm) {
    rc = f->xchg_in.resize(2 * cap);
    if (rc == TDR_OK) rc = f->xchg_out.resize(2 * N);
    if (rc == TDR_OK) rc = f->raw_glob.resize(N);
    if (rc == TDR_OK) rc = f->ld_glob.resize(N);
    if (rc == TDR_OK) rc = f->st_send.resize(TDR_ST_FIELDS * cap);
    if (rc == TDR_OK) rc = f->st_all.resize(TDR_ST_FIELDS * N);
    if (rc == TDR_OK) rc = f->st_glob.resize(TDR_ST_FIELDS * N);
  }
  if (rc == TDR_OK && hipMemset(f->last_dist.p, 0, cap * sizeof(float)) != hipSuccess) rc = failh(TDR_ERR_HIP, "memset");
  if (rc == TDR_OK) rc = tdr_score_ctx_create(&f->score_ctx);
  if (rc != TDR_OK) {
    tdr_filter_destroy(f);
    return rc;
  }
  *out = f;
  return TDR_OK;
}
int tdr_filter_create(tdr_map* map, int n_max, const tdr_filter_params* fp, uint32_t seed, tdr_filter** out) {
  return filter_create(map, n_max, fp, seed, nullptr, out);
}
// the Cartesian filter (BASELINE config 4): the same object, its scoring stage is filter_score's Cartesian branch
int tdr_filter_create_cart(tdr_map* map, int n_max, const tdr_filter_params* fp, uint32_t seed, tdr_filter** out) {
  if (map && (map->win_rows < 1 || map->win_cols < 1))
    return failh(TDR_ERR_ARG, "filter_create_cart: the map has no window (tdr_map_set_window)");
  TTRY(filter_create(map, n_max, fp, seed, nullptr, out));
  (*out)->cart = true;
  return TDR_OK;
}
// particles sharded over the ranks of `comm` (not owned; must outlive the filter)
int tdr_filter_create_sharded(tdr_map* map, int n_max, const tdr_filter_params* fp, uint32_t seed, tdr_comm* comm,
                              tdr_filter** out) {
  if (!comm) return failh(TDR_ERR_ARG, "filter_create_sharded: null comm");
  return filter_create(map, n_max, fp, seed, comm, out);
}
int64_t tdr_filter_num_local(const tdr_filter* f) { return f ? f->nl() : 0; }
void tdr_filter_destroy(tdr_filter* f) {
  if (!f) return;
  if (f->rng && f->rng_owned) tdr_rng_destroy(f->rng);
  tdr_score_ctx_destroy(f->score_ctx);
  tdr_rng_pipe_destroy(f->pipe);
  delete f;
}

int tdr_filter_configure(tdr_filter* f, int parity_rng, int locality_every) {
  if (!f) return failh(TDR_ERR_ARG, "filter_configure: null filter");
  if (!parity_rng) TTRY(rng_to_host(f));
  f->parity_rng = parity_rng != 0;
  f->locality_every = locality_every;
  return TDR_OK;
}

static void note_uniform_scale(tdr_filter* f, const tdr_state* s, int64_t n) {
  f->uniform_scale = 0.f;
  if (!f->scale_frozen || n < 1 || !(s[0].scale > 0)) return;
  for (int64_t i = 1; i < n; i++)
    if (s[i].scale != s[0].scale) return;
  f->uniform_scale = s[0].scale;
}

// states: the GLOBAL particle array; a sharded filter keeps this rank's slice
int tdr_filter_set_states(tdr_filter* f, const tdr_state* states, int64_t n) {
  if (!f || (n > 0 && !states) || n < 0 || n > f->n_max) return failh(TDR_ERR_ARG, "filter_set_states: bad arguments");
  if (n % f->world) return failh(TDR_ERR_ARG, "filter_set_states: %lld particles over %d ranks", (long long)n, f->world);
  const int64_t nl = n / f->world;
  if (nl > 0) {
    HTRY(hipMemcpy(f->aos.p, states + (size_t)f->rank * nl, (size_t)nl * sizeof(tdr_state), hipMemcpyHostToDevice));
    TTRY(tdr_k_states_aos_to_soa(f->aos.p, nl, f->st.p, f->cap, f->stream));
    HTRY(hipDeviceSynchronize());
  }
  f->n = n;
  f->states_changed();
  f->maybe_uninit = false;
  for (int64_t i = 0; i < n; i++) f->maybe_uninit |= states[i].have_init == 0;
  if (f->fp.fixed_scale > 0) f->scale_frozen = true;
  note_uniform_scale(f, states, n);
  return TDR_OK;
}

// this rank's particles (all of them when the filter is not sharded): n <= tdr_filter_num_local
int tdr_filter_get_states(tdr_filter* f, tdr_state* out, int64_t n) {
  if (!f || !out || n < 0 || n > f->nl()) return failh(TDR_ERR_ARG, "filter_get_states: bad arguments");
  if (n == 0) return TDR_OK;
  TTRY(tdr_k_states_soa_to_aos(f->st.p, f->cap, n, f->aos.p, f->stream));
  HTRY(hipMemcpy(out, f->aos.p, (size_t)n * sizeof(tdr_state), hipMemcpyDeviceToHost));
  return TDR_OK;
}

// The particle loop of initializeParticles on the device, on the filter's own generator (which stays there): every rank
// runs the whole chain and writes its slice; the bookkeeping is tdr_filter_set_states' for the states the loop makes
// (one heading rule and one scale rule for all of them).
static int initialize_on_device(tdr_filter* f) {
  tdr_map* m = f->map;
  const tdr_filter_params& p = f->fp;
  int64_t n = std::min<int64_t>(tdr_init_particles_count(&p, (int)f->n_max), f->n_max);
  n -= n % f->world;
  const int64_t nl = n / f->world;
  TTRY(rng_to_device(f));
  DevBuf<uint8_t> ws;
  TTRY(ws.resize(tdr_init_workspace_bytes()));
  int64_t made = 0;
  TTRY(tdr_rng_pipe_init_particles(f->pipe, &m->desc, &p, (int)f->n_max, (int64_t)f->rank * nl, (int64_t)(f->rank + 1) * nl,
                                   f->st.p, f->cap, &made, ws.p, f->stream));
  HTRY(hipStreamSynchronize(f->stream));
  f->n = n;
  f->states_changed();
  f->maybe_uninit = n > 0 && p.init_pos_deg_theta == std::numeric_limits<float>::infinity();
  if (p.fixed_scale > 0) f->scale_frozen = true;
  // note_uniform_scale: a fixed scale is every particle's; the unknown-scale groups hold ten different scales
  f->uniform_scale = (f->scale_frozen && n > 0 && p.fixed_scale > 0) ? p.fixed_scale : 0.f;
  return TDR_OK;
}

// ParticleFilter::initializeParticles (particle_filter.cpp:19-84)
int tdr_filter_initialize_particles(tdr_filter* f) {
  if (!f || !f->map || !f->map->have_map) return failh(TDR_ERR_ARG, "initialize_particles: no map");
  tdr_map* m = f->map;
  tdr_filter_params& p = f->fp;
  if (p.fixed_scale >= 0) f->scale_frozen = true;  // :23-25
  const float inf = std::numeric_limits<float>::infinity();
  if (f->scale_frozen && p.init_pos_m_x != inf) {   // :27-53
    p.init_pos_px_x = (p.init_pos_m_x * p.fixed_scale) + (float)m->center_x;
    p.init_pos_px_y = (p.init_pos_m_y * p.fixed_scale) + (float)m->center_y;
    if (p.init_pos_px_x < 0 || p.init_pos_px_x >= (float)m->desc.cols || p.init_pos_px_y < 0 ||
        p.init_pos_px_y >= (float)m->desc.rows)
      return TDR_OK;  // "No map received for input loc"
    bool good = false;
    for (int dx = -4; dx <= 4 && !good; dx++)
      for (int dy = -4; dy <= 4 && !good; dy++) {
        uint32_t bits = 0;
        TTRY(tdr_map_classes_at_point(m, (int)(p.init_pos_px_x + dx), (int)(p.init_pos_px_y + dy), &bits));
        good = (bits & 2u) != 0;
      }
    if (!good) return TDR_OK;  // "No road in map at init location"
  }
  if (rng_device_capable(f) && tdr_cfg().init_device != 0) return initialize_on_device(f);
  std::vector<tdr_state> states((size_t)f->n_max + 16);
  int64_t n = 0;
  TTRY(rng_to_host(f));
  TTRY(tdr_init_particles_host(f->rng, m->maps_host.data(), m->desc.ncls, m->desc.rows, m->desc.cols,
                               m->desc.resolution, &p, (int)f->n_max, states.data(), &n));
  n = std::min<int64_t>(n, f->n_max);
  n -= n % f->world;
  return tdr_filter_set_states(f, states.data(), n);
}


// ParticleFilter::propagate (particle_filter.cpp:86-92)
static int filter_propagate(tdr_filter* f, float tx, float ty, float omega, bool scale_freeze) {
  if (f->n == 0) return TDR_OK;
  f->states_changed();
  // every particle's scale takes a draw of its own: the promise behind uniform_scale (tdr_k_score_polar) ends here
  if (!scale_freeze) f->uniform_scale = 0.f;
  const int64_t nl = f->nl();
  const float* z = nullptr;
  if (rng_device_capable(f)) {
    // the reference draws serially in GLOBAL particle order from one generator: every rank continues the same stream on
    // its device (same state everywhere) and keeps the normals of its own particles — nothing is drawn on the host
    TTRY(rng_to_device(f));
    TTRY(tdr_rng_pipe_normals(f->pipe, f->n, (int64_t)f->rank * nl, (int64_t)(f->rank + 1) * nl, scale_freeze ? 1 : 0, &z,
                              f->stream));
  } else if (f->parity_rng) {
    // a generator shared with the caller (StateParticle's surface): the host draws, serially
    std::vector<float> zh((size_t)4 * f->n);
    TTRY(tdr_propagate_normals_host(f->rng, f->n, scale_freeze ? 1 : 0, zh.data()));
    HTRY(hipMemcpyAsync(f->z4.p, zh.data() + (size_t)4 * f->rank * nl, (size_t)4 * nl * sizeof(float),
                        hipMemcpyHostToDevice, f->stream));
    HTRY(hipStreamSynchronize(f->stream));
    z = f->z4.p;
  }
  return tdr_k_propagate(f->st.p, f->cap, nl, f->last_dist.p, tx, ty, omega, scale_freeze ? 1 : 0, f->fp.pos_cov,
                         f->fp.theta_cov, z, f->seed, f->prop_calls++, (int64_t)f->rank * nl, f->stream);
}
int tdr_filter_propagate(tdr_filter* f, float tx, float ty, float omega) {
  if (!f) return failh(TDR_ERR_ARG, "filter_propagate: null filter");
  return filter_propagate(f, tx, ty, omega, f->scale_frozen);
}
// StateParticle::propagate(trans, omega, scale_freeze) (state_particle.cpp:57-78): the freeze flag is the caller's
int tdr_filter_propagate_freeze(tdr_filter* f, float tx, float ty, float omega, int scale_freeze) {
  if (!f) return failh(TDR_ERR_ARG, "filter_propagate_freeze: null filter");
  return filter_propagate(f, tx, ty, omega, scale_freeze != 0);
}
// The filter draws from the caller's std::mt19937 from now on (the reference's particles share ONE generator with
// their filter, state_particle.h:61-64).  `mt19937` must point to a std::mt19937 of the libstdc++ this library was
// built with; it is not owned.
int tdr_filter_share_rng(tdr_filter* f, void* mt19937) {
  if (!f || !mt19937) return failh(TDR_ERR_ARG, "filter_share_rng: bad arguments");
  if (f->pipe) { tdr_rng_pipe_destroy(f->pipe); f->pipe = nullptr; }   // (the filter's own stream ends here)
  if (f->rng && f->rng_owned) tdr_rng_destroy(f->rng);
  f->rng = mt19937;
  f->rng_owned = false;
  f->parity_rng = true;
  return TDR_OK;
}
// StateParticle's constructor with init == true (state_particle.cpp:3-49) for particle 0 of the filter
int tdr_filter_init_one(tdr_filter* f) {
  if (!f || !f->map || !f->map->have_map) return failh(TDR_ERR_ARG, "filter_init_one: no map");
  tdr_map* m = f->map;
  tdr_state st;
  TTRY(rng_to_host(f));
  TTRY(tdr_init_particle_host(f->rng, m->maps_host.data(), m->desc.ncls, m->desc.rows, m->desc.cols, m->desc.resolution,
                              &f->fp, &st));
  return tdr_filter_set_states(f, &st, 1);
}

// ParticleFilter::update (particle_filter.cpp:94-189).  scan_imgs: HOST [ncls][nb*nr] column-major images, or NULL to
// score against `renderer`'s last render without a host round trip.  n_target < 0 keeps the particle count
// (the adaptive count of :151-157 is an explicit input; the reference feeds it from an OpenCV EM thread).
static int filter_score(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, float res);
static int filter_resample(tdr_filter* f, int64_t n_target);
int tdr_filter_update(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, float res, int64_t n_target) {
  if (!f || !f->map || !f->map->have_map) return failh(TDR_ERR_ARG, "filter_update: no map");
  if (f->n == 0) return TDR_OK;  // :96-99
  TTRY(filter_score(f, scan_imgs, renderer, res));
  const int64_t n = f->n, nl = f->nl();
  const float *raw = f->raw_w.p, *ld = f->last_dist.p;
  if (f->comm) {
    // ONE all-gather of {raw weight, last_dist}: afterwards every rank computes the same statistics and the same
    // order-exact running sum on the same global arrays (replaces the north star's all-reduce, whose result
    // would depend on the reduction tree)
    TTRY(tdr_k_shard_pack2(f->raw_w.p, f->last_dist.p, nl, f->xchg_in.p, f->stream));
    TTRY(tdr_comm_all_gather(f->comm, f->xchg_in.p, f->xchg_out.p, (size_t)2 * nl * sizeof(float), f->stream));
    TTRY(tdr_k_shard_unpack2(f->xchg_out.p, f->world, nl, f->raw_glob.p, f->ld_glob.p, f->stream));
    raw = f->raw_glob.p;
    ld = f->ld_glob.p;
  }
  TTRY(tdr_k_update_weights(raw, ld, n, f->w.p, f->info.p, f->stream));
  return filter_resample(f, n_target);
}
// ParticleFilter::update with the geometric images entering the score (state_particle.cpp:145-152, opt-in)
int tdr_filter_update_geo(tdr_filter* f, const float* scan_imgs, const float* geo_imgs, float res, int64_t n_target) {
  if (!f || !f->map || !f->map->have_map) return failh(TDR_ERR_ARG, "filter_update_geo: no map");
  if (!scan_imgs || !geo_imgs) return failh(TDR_ERR_ARG, "filter_update_geo: null images");
  if (f->comm) return failh(TDR_ERR_ARG, "filter_update_geo: not available on a sharded filter");
  if (f->cart) return failh(TDR_ERR_ARG, "filter_update_geo: there is no Cartesian geometric cost");
  if (f->n == 0) return TDR_OK;
  tdr_map* m = f->map;
  if (m->nb < 1 || !m->tab.p) return failh(TDR_ERR_ARG, "filter_update_geo: samplePtsPolar was never called");
  TTRY(map_ensure_geo(m));
  f->fp.num_classes = m->desc.ncls;
  const int ncls = m->desc.ncls, nb = m->nb, nr = m->nr;
  const size_t P = (size_t)nb * nr;
  TTRY(f->scan_img.resize(P * std::max(ncls, 2)));
  TTRY(f->scan_pk.resize(P * tdr_rec_floats(ncls)));
  TTRY(f->geo_pk.resize(P * 4));
  HTRY(hipMemcpyAsync(f->scan_img.p, scan_imgs, P * ncls * sizeof(float), hipMemcpyHostToDevice, f->stream));
  TTRY(tdr_k_pack_scan(f->scan_img.p, ncls, nb, nr, f->scan_pk.p, f->stream));
  HTRY(hipMemcpyAsync(f->scan_img.p, geo_imgs, P * 2 * sizeof(float), hipMemcpyHostToDevice, f->stream));
  TTRY(tdr_k_pack_scan(f->scan_img.p, 2, nb, nr, f->geo_pk.p, f->stream));
  double gs[2] = {0, 0};   // top_down_geo[i].sum(): Eigen's order is unspecified; counts are small integers, any order is exact
  for (int i = 0; i < 2; i++)
    for (size_t k = 0; k < P; k++) gs[i] += (double)geo_imgs[P * i + k];
  const int64_t n = f->n;
  const int32_t* perm = nullptr;
  if (f->locality_every > 0) {
    TTRY(f->loc_tmp.resize(tdr_locality_tmp_ints(n, m->desc.rows, m->desc.cols)));
    TTRY(tdr_k_locality_order(f->st.p, f->cap, n, m->desc.rows, m->desc.cols, f->perm.p, f->loc_tmp.p, f->stream));
    perm = f->perm.p;
  }
  f->states_changed();   // (the init search writes headings)
  TTRY(f->ws.resize(tdr_score_geo_workspace_floats(ncls, nb, nr, n, n)));
  TTRY(tdr_k_score_polar_geo(&m->desc, &m->geo_desc, m->tab.p, f->scan_pk.p, f->geo_pk.p, (float)gs[0], (float)gs[1], nb, nr,
                             res, &f->fp, f->st.p, f->cap, n, n, perm, f->uniform_scale, f->maybe_uninit ? 1 : 0,
                             f->raw_w.p, f->ws.p, f->stream));
  if (f->maybe_uninit && !(f->fp.force_on_map || f->fp.fixed_scale < 0)) f->maybe_uninit = false;
  TTRY(tdr_k_update_weights(f->raw_w.p, f->last_dist.p, n, f->w.p, f->info.p, f->stream));
  return filter_resample(f, n_target);
}
// StateParticle::computeWeight for every particle (state_particle.cpp:157-219): raw weights only, no statistics, no
// resampling; read them with tdr_filter_get_raw_weights
int tdr_filter_compute_weights(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, float res) {
  if (!f || !f->map || !f->map->have_map) return failh(TDR_ERR_ARG, "filter_compute_weights: no map");
  if (f->n == 0) return TDR_OK;
  return filter_score(f, scan_imgs, renderer, res);
}
int tdr_filter_get_raw_weights(tdr_filter* f, float* out, int64_t n) {
  if (!f || !out || n < 0 || n > f->cap) return failh(TDR_ERR_ARG, "filter_get_raw_weights: bad arguments");
  HTRY(hipMemcpy(out, f->raw_w.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return TDR_OK;
}
int tdr_filter_get_last_dist(tdr_filter* f, float* out, int64_t n) {
  if (!f || !out || n < 0 || n > f->cap) return failh(TDR_ERR_ARG, "filter_get_last_dist: bad arguments");
  HTRY(hipMemcpy(out, f->last_dist.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return TDR_OK;
}
static int filter_score(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, float res) {
  tdr_map* m = f->map;
  if (!f->cart && (m->nb < 1 || !m->tab.p)) return failh(TDR_ERR_ARG, "filter_update: samplePtsPolar was never called");
  if (f->cart && (m->win_rows < 1 || m->win_cols < 1)) return failh(TDR_ERR_ARG, "filter_update: the map has no window");
  f->fp.num_classes = m->desc.ncls;
  // (a Cartesian scan is packed like a polar one with nb = the window's rows, nr = its columns: tdr_k_score_cart)
  const int ncls = m->desc.ncls, nb = f->cart ? m->win_rows : m->nb, nr = f->cart ? m->win_cols : m->nr;
  const size_t P = (size_t)nb * nr;
  const size_t pk_floats = P * tdr_rec_floats(ncls);
  const float* pk = nullptr;
  if (scan_imgs) {
    TTRY(f->scan_img.resize(P * ncls));
    TTRY(f->scan_pk.resize(pk_floats));
    HTRY(hipMemcpyAsync(f->scan_img.p, scan_imgs, P * ncls * sizeof(float), hipMemcpyHostToDevice, f->stream));
    TTRY(tdr_k_pack_scan(f->scan_img.p, ncls, nb, nr, f->scan_pk.p, f->stream));
    pk = f->scan_pk.p;
  } else if (renderer) {
    if (!renderer->have_scan) return failh(TDR_ERR_ARG, "filter_update: no scan");
    if (renderer->ncls != ncls || renderer->rows != nb || renderer->cols != nr)
      return failh(TDR_ERR_ARG, "filter_update: render shape %dx%dx%d does not match the map's %dx%dx%d",
                   renderer->ncls, renderer->rows, renderer->cols, ncls, nb, nr);
    if (f->cart && renderer->polar) return failh(TDR_ERR_ARG, "filter_update: a Cartesian filter needs a Cartesian render");
    pk = renderer->pk.p;
    TTRY(renderer_wait_render(renderer, f->stream));
  } else if (!(f->comm && f->rank != 0)) {
    return failh(TDR_ERR_ARG, "filter_update: no scan");
  }
  if (f->comm) {
    // the rasterised scan is produced once, on rank 0, and broadcast (north star): 2 MB at config 2
    TTRY(f->pk_recv.resize(pk_floats));
    if (f->rank == 0) HTRY(hipMemcpyAsync(f->pk_recv.p, pk, pk_floats * sizeof(float), hipMemcpyDeviceToDevice, f->stream));
    TTRY(tdr_comm_broadcast(f->comm, f->pk_recv.p, pk_floats * sizeof(float), 0, f->stream));
    pk = f->pk_recv.p;
  }
  const int64_t n = f->nl();   // this rank's particles
  const int32_t* perm = nullptr;
  if (f->cart) {
    // windows that rotate with the particle: the heading belongs in the order's key.  The search runs first (it only
    // chooses headings), the regular launch then scores every particle, as the polar path does.
    f->states_changed();
    if (f->maybe_uninit) {
      TTRY(f->init_ws.resize(tdr_score_cart_init_workspace_floats(ncls, nb, nr, n, f->n)));
      TTRY(tdr_k_score_cart_init(&m->desc, pk, nb, nr, res, &f->fp, f->st.p, f->cap, n, f->n, f->init_ws.p, f->stream));
      f->maybe_uninit = false;   // no gates: every particle has a heading now
    }
    if (f->locality_every > 0) {
      TTRY(f->loc_tmp.resize(tdr_locality_pose_tmp_ints(n) + 2));
      TTRY(tdr_k_locality_order_pose(f->st.p, f->cap, n, m->desc.rows, m->desc.cols, (float)(nb + nr) / 16.f, f->perm.p,
                                     f->loc_tmp.p, f->stream));
      perm = f->perm.p;
    }
    TTRY(f->ws.resize(tdr_score_cart_workspace_floats(ncls, nb, nr, n, f->n)));
    TTRY(tdr_k_score_cart(&m->desc, pk, nb, nr, res, &f->fp, f->st.p, f->cap, n, f->n, perm, f->raw_w.p, f->ws.p, f->stream));
    if (renderer && !scan_imgs) TTRY(renderer_note_read(renderer, f->stream));
    return TDR_OK;
  }
  if (f->locality_every > 0) {
    TTRY(f->loc_tmp.resize(tdr_locality_tmp_ints(n, m->desc.rows, m->desc.cols)));
    TTRY(tdr_k_locality_order(f->st.p, f->cap, n, m->desc.rows, m->desc.cols, f->perm.p, f->loc_tmp.p, f->stream));
    perm = f->perm.p;
  }
  f->states_changed();   // (the init search writes headings)
  TTRY(f->ws.resize(tdr_score_workspace_floats(ncls, nb, nr, n, f->n)));
  // the search over this many particles pays for pre-split half records
  if (f->maybe_uninit) TTRY(map_rec16_alloc(m, f->n));
  const bool uses_rec16 = f->maybe_uninit && m->desc.rec16 && f->n >= tdr_cfg().rec16_min;
  if (uses_rec16) TTRY(map_rec16_begin(m, f->stream));
  TTRY(tdr_score_ctx_set_polar_factors(f->score_ctx, m->fac.p, nb, nr));
  TTRY(tdr_k_score_polar_ctx(&m->desc, m->tab.p, pk, nb, nr, res, &f->fp, f->st.p, f->cap, n, f->n, perm, f->uniform_scale,
                             f->maybe_uninit ? 1 : 0, f->raw_w.p, f->ws.p, f->score_ctx, f->stream));
  if (uses_rec16) TTRY(map_rec16_end(m, f->stream));
  if (renderer && !scan_imgs) TTRY(renderer_note_read(renderer, f->stream));
  // the search initialises every un-gated particle; only gated ones (state_particle.cpp:163-176) can stay un-initialised
  if (f->maybe_uninit && !(f->fp.force_on_map || f->fp.fixed_scale < 0)) f->maybe_uninit = false;
  return TDR_OK;
}
// statistics are done: running sum, resample, gather, bookkeeping (particle_filter.cpp:151-188)
static int filter_resample(tdr_filter* f, int64_t n_target) {
  const int64_t n = f->n, nl = f->nl();
  int64_t n_new = n;
  if (n_target >= 0) n_new = std::max<int64_t>(1, std::min<int64_t>(n_target, f->n_max));
  n_new = std::max<int64_t>(f->world, n_new - n_new % f->world);   // whole shards
  const int64_t nl_new = n_new / f->world, i0 = (int64_t)f->rank * nl_new;
  TTRY(f->ml_dev.resize(12));
  TTRY(tdr_k_prefix(f->w.p, n, f->runmax.p, f->pfx_ws.p, f->stream));
  // :172-173 (every rank owns an identically seeded generator); each rank draws its own slice [i0, i0 + nl_new) of the new
  // set, idx holds GLOBAL source indices
  const float* shift_dev = nullptr;
  float shift = 0.f;
  if (rng_on_device(f)) TTRY(tdr_rng_pipe_uniform(f->pipe, &shift_dev, f->stream));   // the stream is on the device: so is the draw
  else shift = tdr_rng_uniform_host(f->rng);
  if (f->comm) {
    if (shift_dev) TTRY(tdr_k_resample_dev(f->runmax.p, n, n_new, shift_dev, i0, i0 + nl_new, f->idx.p, f->stream));
    else TTRY(tdr_k_resample(f->runmax.p, n, n_new, shift, i0, i0 + nl_new, f->idx.p, f->stream));
    // the second all-gather: the pre-resample state planes, [rank][7][nl] (28 B x N)
    for (int k = 0; k < TDR_ST_FIELDS; k++)
      HTRY(hipMemcpyAsync(f->st_send.p + (size_t)k * nl, f->st.p + (size_t)k * f->cap, (size_t)nl * sizeof(float),
                          hipMemcpyDeviceToDevice, f->stream));
    TTRY(tdr_comm_all_gather(f->comm, f->st_send.p, f->st_all.p, (size_t)TDR_ST_FIELDS * nl * sizeof(float), f->stream));
    TTRY(tdr_k_gather_states(f->st_all.p, 0, nl, f->idx.p, nl_new, f->st_new.p, f->cap, f->stream));
    TTRY(tdr_k_save_ml_state(f->info.p, f->st_all.p, 0, nl, n, f->ml_dev.p, f->stream));
  } else {
    // index, state rows and max_likelihood_particle_ = particles_[argmax] (:145-147, that particle's pre-resample state,
    // kept on the device: the update returns without waiting for the GPU) in one launch
    TTRY(tdr_k_resample_gather(f->runmax.p, n, n_new, shift_dev, shift, 0, n_new, f->idx.p, f->st.p, f->cap, 0, f->st_new.p,
                               f->cap, f->info.p, f->ml_dev.p, f->stream));
  }
  f->have_ml = true;
  f->states_changed();
  std::swap(f->st.p, f->st_new.p);  // :187
  f->n = n_new;
  f->step++;
  return TDR_OK;
}

int tdr_filter_get_weights(tdr_filter* f, float* out, int64_t n) {
  if (!f || !out || n < 0 || n > f->n_max) return failh(TDR_ERR_ARG, "filter_get_weights: bad arguments");
  HTRY(hipMemcpy(out, f->w.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return TDR_OK;
}
int tdr_filter_get_resample_indices(tdr_filter* f, int32_t* out, int64_t n) {
  if (!f || !out || n < 0 || n > f->nl()) return failh(TDR_ERR_ARG, "filter_get_resample_indices: bad arguments");
  HTRY(hipMemcpy(out, f->idx.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return TDR_OK;
}

// meanLikelihood + computeMeanCov (particle_filter.cpp:191-220); about_max != 0: maxLikelihood + computeCov (:222-236)
int tdr_filter_mean_cov(tdr_filter* f, int about_max, float state[4], float cov[16]) {
  if (!f) return failh(TDR_ERR_ARG, "filter_mean_cov: null filter");
  if (cov) std::memset(cov, 0, 16 * sizeof(float));
  if (state) std::memset(state, 0, 4 * sizeof(float));
  if (f->n < 1) return TDR_OK;  // :207-209
  float out[24];
  const float* gst = nullptr;
  int64_t gcap = 0;
  // (a sharded filter's ranks make the same calls in the same order, so the cache is valid on all of them or on none:
  // the all-gather inside filter_global_states stays collective)
  if (about_max || !f->mean_cov_valid) TTRY(filter_global_states(f, &gst, &gcap));
  if (!about_max) {
    if (!f->mean_cov_valid) {
      TTRY(tdr_k_mean_cov(gst, gcap, f->n, nullptr, f->stats.p, f->stream));
      HTRY(hipMemcpy(f->mean_cov_host, f->stats.p, sizeof(out), hipMemcpyDeviceToHost));
      f->mean_cov_valid = true;
    }
    std::memcpy(out, f->mean_cov_host, sizeof(out));
    if (state) std::memcpy(state, out, 4 * sizeof(float));
  } else {
    float ref[4] = {0, 0, 0, 0};
    if (!f->have_ml) return failh(TDR_ERR_ARG, "filter_mean_cov: no update yet, there is no max-likelihood particle");
    TTRY(tdr_k_mean_cov(gst, gcap, f->n, f->ml_dev.p + 8, f->stats.p, f->stream));
    HTRY(hipMemcpyAsync(out, f->stats.p, sizeof(out), hipMemcpyDeviceToHost, f->stream));
    HTRY(hipMemcpyAsync(ref, f->ml_dev.p + 8, sizeof(ref), hipMemcpyDeviceToHost, f->stream));
    HTRY(hipStreamSynchronize(f->stream));
    if (state) std::memcpy(state, ref, sizeof(ref));
  }
  if (cov) std::memcpy(cov, out + 4, 16 * sizeof(float));
  return TDR_OK;
}

// freezeScale (particle_filter.cpp:343-357)
int tdr_filter_freeze_scale(tdr_filter* f) {
  if (!f) return failh(TDR_ERR_ARG, "filter_freeze_scale: null filter");
  if (f->scale_frozen || f->n < 1) return TDR_OK;
  const float* gst = nullptr;
  int64_t gcap = 0;
  TTRY(filter_global_states(f, &gst, &gcap));
  TTRY(tdr_k_mean_cov(gst, gcap, f->n, nullptr, f->stats.p, f->stream));
  f->states_changed();
  TTRY(tdr_k_set_scale(f->st.p, f->cap, f->nl(), f->stats.p + 20, f->stream));
  float gm = 0;
  HTRY(hipMemcpy(&gm, f->stats.p + 20, sizeof(float), hipMemcpyDeviceToHost));
  f->scale_frozen = true;
  f->uniform_scale = gm;
  return TDR_OK;
}
int tdr_filter_is_scale_frozen(const tdr_filter* f) { return f && f->scale_frozen; }
// scale() (particle_filter.cpp:359-367)
float tdr_filter_scale(tdr_filter* f) {
  if (!f) return -1.f;
  if (f->fp.fixed_scale > 0) return f->fp.fixed_scale;
  if (f->scale_frozen && f->n > 0) {
    if (f->scale_valid) return f->scale_host;
    float s = -1.f;
    if (hipMemcpy(&s, f->st.p + (size_t)TDR_ST_SCALE * f->cap, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
    return s;
  }
  return -1.f;
}
int64_t tdr_filter_num_particles(const tdr_filter* f) { return f ? f->n : 0; }

// computeGMM (particle_filter.cpp:252-318): <= 1000 strided samples {x, y, 50 cos theta, 50 sin theta} -> mixture
int tdr_filter_compute_gmm(tdr_filter* f) {
  if (!f) return failh(TDR_ERR_ARG, "filter_compute_gmm: null filter");
  if (f->n < 1) return TDR_OK;
  const int num = (int)std::min<int64_t>(1000, f->n);   // :262
  TTRY(f->gmm_samples.resize((size_t)3 * num));
  const float* gst = nullptr;
  int64_t gcap = 0;
  TTRY(filter_global_states(f, &gst, &gcap));
  TTRY(tdr_k_sample_ml_states(gst, gcap, f->n, num, f->gmm_samples.p, f->stream));
  std::vector<float> h((size_t)3 * num);
  HTRY(hipMemcpyAsync(h.data(), f->gmm_samples.p, h.size() * sizeof(float), hipMemcpyDeviceToHost, f->stream));
  HTRY(hipStreamSynchronize(f->stream));
  std::vector<double> x((size_t)4 * num);
  for (int i = 0; i < num; i++) {
    x[4 * i + 0] = h[3 * i + 0];
    x[4 * i + 1] = h[3 * i + 1];
    x[4 * i + 2] = 50 * std::cos(h[3 * i + 2]);   // :269-270 (float argument: the float overload)
    x[4 * i + 3] = 50 * std::sin(h[3 * i + 2]);
  }
  int k = f->num_gaussians;
  std::vector<float> means((size_t)3 * TDR_GMM_MAX_K), covs((size_t)9 * TDR_GMM_MAX_K);
  TTRY(tdr_gmm_select_host(x.data(), num, f->n, &k, TDR_GMM_MAX_K, means.data(), covs.data()));
  f->num_gaussians = k;
  f->gmm_means.assign(means.begin(), means.begin() + 3 * k);
  f->gmm_covs.assign(covs.begin(), covs.begin() + 9 * k);
  return TDR_OK;
}
int tdr_filter_get_gmm(tdr_filter* f, int max_k, int* k_out, float* means, float* covs) {
  if (!f || !k_out) return failh(TDR_ERR_ARG, "filter_get_gmm: bad arguments");
  const int k = (int)(f->gmm_means.size() / 3);
  *k_out = k;
  if (k > max_k) return failh(TDR_ERR_ARG, "filter_get_gmm: %d clusters, room for %d", k, max_k);
  if (means && k) std::memcpy(means, f->gmm_means.data(), f->gmm_means.size() * sizeof(float));
  if (covs && k) std::memcpy(covs, f->gmm_covs.data(), f->gmm_covs.size() * sizeof(float));
  return TDR_OK;
}
int64_t tdr_filter_step_count(const tdr_filter* f) { return f ? (int64_t)f->step : -1; }
int tdr_filter_num_gaussians(const tdr_filter* f) { return f ? f->num_gaussians : 0; }
int tdr_filter_set_num_gaussians(tdr_filter* f, int num_gaussians) {
  if (!f || num_gaussians < 1 || num_gaussians > TDR_GMM_MAX_K)
    return failh(TDR_ERR_ARG, "filter_set_num_gaussians: bad arguments (1 .. %d)", TDR_GMM_MAX_K);
  f->num_gaussians = num_gaussians;
  return TDR_OK;
}
int64_t tdr_filter_adaptive_count(tdr_filter* f) {
  if (!f) return -1;
  const int k = (int)(f->gmm_means.size() / 3);
  if (k == 0) return f->n;
  return tdr_adaptive_count_host(f->gmm_covs.data(), k, f->n, f->n_max);
}

// ---- the particle picture (include/tdr.h, "the particle picture"; kernels in tdr_viz.hip) ---------------------------------
int tdr_filter_set_viz_background(tdr_filter* f, const uint8_t* bgr_host, int H, int W) {
  if (!f || !bgr_host) return failh(TDR_ERR_ARG, "filter_set_viz_background: null argument");
  if (H < 11 || W < 11 || H > 32768 || W > 32768)
    return failh(TDR_ERR_ARG, "filter_set_viz_background: a %d x %d image (11 .. 32768 a side)", H, W);
  const size_t bytes = (size_t)3 * H * W;
  TTRY(f->viz_bg.resize(bytes));
  TTRY(f->viz_planes.resize(4 * tdr_viz_plane_words(H, W)));
  HTRY(hipStreamSynchronize(f->stream));   // (an earlier picture may still read the old background)
  HTRY(hipMemcpy(f->viz_bg.p, bgr_host, bytes, hipMemcpyHostToDevice));
  f->viz_h = H;
  f->viz_w = W;
  return TDR_OK;
}

// ... from the label image the node colours (aerialMapCallback, :584): one byte a cell goes up, the colour table is
// applied on the device (tdr_k_label_picture); viz_out is the labels' staging
int tdr_filter_set_viz_background_labels(tdr_filter* f, const uint8_t* labels_host, int H, int W, const uint8_t* lut_bgr) {
  if (!f || !labels_host || !lut_bgr) return failh(TDR_ERR_ARG, "filter_set_viz_background_labels: null argument");
  if (H < 11 || W < 11 || H > 32768 || W > 32768)
    return failh(TDR_ERR_ARG, "filter_set_viz_background_labels: a %d x %d image (11 .. 32768 a side)", H, W);
  const size_t cells = (size_t)H * W;
  TTRY(f->viz_bg.resize(3 * cells));
  TTRY(f->viz_planes.resize(4 * tdr_viz_plane_words(H, W)));
  HTRY(hipStreamSynchronize(f->stream));   // (an earlier picture may still read the old background, or write viz_out)
  TTRY(f->viz_out.resize(cells));
  HTRY(hipMemcpy(f->viz_out.p, labels_host, cells, hipMemcpyHostToDevice));
  TTRY(tdr_k_label_picture(f->viz_out.p, (int64_t)cells, lut_bgr, f->viz_bg.p, f->stream));
  HTRY(hipStreamSynchronize(f->stream));
  f->viz_h = H;
  f->viz_w = W;
  return TDR_OK;
}

// (int)((float)dim * s) as the node computes it (src/top_down_render.cpp:442-444), x86's conversion
}  // extern "C"
int tdrh::viz_pub_dim(int dim, float s) {
  const float v = (float)dim * s;
  return (v >= -2147483648.f && v < 2147483648.f) ? (int)v : std::numeric_limits<int>::min();
}
extern "C" {

int tdr_filter_visualize(tdr_filter* f, float pub_scale, const int32_t* extra_arrows, int m, uint8_t* out_bgr_host,
                         int64_t capacity, int* out_h, int* out_w) {
  if (!f || !out_h || !out_w || m < 0 || (m > 0 && !extra_arrows) || m > (1 << 20))
    return failh(TDR_ERR_ARG, "filter_visualize: bad arguments");
  if (f->comm) return failh(TDR_ERR_ARG, "filter_visualize: a sharded filter has no picture (draw from a one-GPU filter)");
  if (f->viz_h < 1) return failh(TDR_ERR_ARG, "filter_visualize: no background (tdr_filter_set_viz_background)");
  const int H = f->viz_h, W = f->viz_w;
  const int oh = viz_pub_dim(H, pub_scale), ow = viz_pub_dim(W, pub_scale);
  if (oh < 1 || ow < 1 || oh > 32768 || ow > 32768)
    return failh(TDR_ERR_ARG, "filter_visualize: scale %g publishes %d x %d pixels (1 .. 32768 a side)", (double)pub_scale, oh, ow);
  *out_h = oh;
  *out_w = ow;
  if (!out_bgr_host) return TDR_OK;
  const size_t bytes = (size_t)3 * oh * ow;
  if (capacity < 0 || (size_t)capacity < bytes)
    return failh(TDR_ERR_ARG, "filter_visualize: the image needs %zu bytes, room for %lld", bytes, (long long)capacity);
  // layers 4 and 5 on the host: a few hundred integers
  float best[4];
  if (f->have_ml) HTRY(hipMemcpy(best, f->ml_dev.p + 8, sizeof(best), hipMemcpyDeviceToHost));
  const int k = (int)(f->gmm_means.size() / 3);
  std::vector<int32_t> segs((size_t)5 * TDR_VIZ_MAX_SEGS(k, m));
  int nseg = 0;
  TTRY(tdr_viz_overlay_host(f->gmm_means.data(), f->gmm_covs.data(), k, f->have_ml ? best : nullptr, extra_arrows, m, H,
                            segs.data(), TDR_VIZ_MAX_SEGS(k, m), &nseg));
  TTRY(f->viz_segs.resize((size_t)5 * std::max(nseg, 1)));
  TTRY(f->viz_out.resize(bytes));
  const size_t pw = tdr_viz_plane_words(H, W);
  hipStream_t s = f->stream;
  if (nseg) HTRY(hipMemcpyAsync(f->viz_segs.p, segs.data(), (size_t)5 * nseg * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HTRY(hipMemsetAsync(f->viz_planes.p, 0, 4 * pw * sizeof(uint32_t), s));
  TTRY(tdr_k_viz_particles(f->st.p, f->cap, f->n, H, W, f->viz_planes.p, s));
  TTRY(tdr_k_viz_segments(f->viz_segs.p, nseg, H, W, f->viz_planes.p, s));
  TTRY(tdr_k_viz_compose(f->viz_bg.p, H, W, f->viz_planes.p, oh, ow, f->viz_out.p, s));
  HTRY(hipMemcpyAsync(out_bgr_host, f->viz_out.p, bytes, hipMemcpyDeviceToHost, s));
  HTRY(hipStreamSynchronize(s));
  return TDR_OK;
}

// ParticleFilter::updateMap(const cv::Mat& map, map_center) (particle_filter.cpp:320-341) for a class-index image
int tdr_filter_update_map_labels(tdr_filter* f, const uint8_t* label_img, int img_h, int img_w,
                                 const int32_t* flatten_lut, int lut_size, int ncls, float resolution, int center_x,
                                 int center_y) {
  if (!f || !f->map) return failh(TDR_ERR_ARG, "filter_update_map_labels: null filter");
  const int ox = f->map->center_x, oy = f->map->center_y;
  TTRY(tdr_map_set_labels(f->map, label_img, img_h, img_w, flatten_lut, lut_size, ncls, resolution, center_x, center_y));
  f->states_changed();
  if (f->n > 0) return tdr_k_shift_init(f->st.p, f->cap, f->nl(), (float)(center_x - ox), (float)(center_y - oy), f->stream);
  if (f->map->have_map) return tdr_filter_initialize_particles(f);  // :337-340
  return TDR_OK;
}

// tdr_filter_update_map_labels through the incremental map update (tdr_map_update_labels_incremental)
int tdr_filter_update_map_labels_incremental(tdr_filter* f, const uint8_t* label_img, int img_h, int img_w,
                                             const int32_t* flatten_lut, int lut_size, int ncls, float resolution,
                                             int center_x, int center_y, int64_t* changed_cells) {
  if (!f || !f->map) return failh(TDR_ERR_ARG, "filter_update_map_labels_incremental: null filter");
  const int ox = f->map->center_x, oy = f->map->center_y;
  TTRY(tdr_map_update_labels_incremental(f->map, label_img, img_h, img_w, flatten_lut, lut_size, ncls, resolution, center_x,
                                         center_y, changed_cells));
  f->states_changed();
  if (f->n > 0) return tdr_k_shift_init(f->st.p, f->cap, f->nl(), (float)(center_x - ox), (float)(center_y - oy), f->stream);
  if (f->map->have_map) return tdr_filter_initialize_particles(f);  // :337-340
  return TDR_OK;
}
// ... and through tdr_map_patch_labels
int tdr_filter_patch_map_labels(tdr_filter* f, const uint8_t* patch, int y0, int x0, int h, int w, int center_x,
                                int center_y, int64_t* changed_cells) {
  if (!f || !f->map) return failh(TDR_ERR_ARG, "filter_patch_map_labels: null filter");
  const int ox = f->map->center_x, oy = f->map->center_y;
  TTRY(tdr_map_patch_labels(f->map, patch, y0, x0, h, w, center_x, center_y, changed_cells));
  f->states_changed();
  if (f->n > 0) return tdr_k_shift_init(f->st.p, f->cap, f->nl(), (float)(center_x - ox), (float)(center_y - oy), f->stream);
  if (f->map->have_map) return tdr_filter_initialize_particles(f);  // :337-340
  return TDR_OK;
}

// ParticleFilter::updateMap (particle_filter.cpp:320-341), with the map already in distance-map form
int tdr_filter_update_map(tdr_filter* f, const float* class_maps, const uint8_t* class_mask, int ncls, int rows, int cols,
                          float resolution, int center_x, int center_y) {
  if (!f || !f->map) return failh(TDR_ERR_ARG, "filter_update_map: null filter");
  const int ox = f->map->center_x, oy = f->map->center_y;
  TTRY(tdr_map_set(f->map, class_maps, class_mask, ncls, rows, cols, resolution, center_x, center_y));
  f->states_changed();
  if (f->n > 0) return tdr_k_shift_init(f->st.p, f->cap, f->nl(), (float)(center_x - ox), (float)(center_y - oy), f->stream);
  return tdr_filter_initialize_particles(f);  // :337-340
}

}  // extern "C"
