// tdr_host_recover.cpp — recovery injection (include/tdr.h, "recovery injection"; kernels in csrc/tdr_recover.hip): the
// slow / fast average tracker on the host, the map's road list, and the injection of one filter or a batch:
// tdr_map_road_cells, tdr_filter_get_weight_stats, tdr_filter_inject, tdr_filter_recovery_step, tdr_batch_inject; and sensor
// resetting (include/tdr.h, "sensor resetting"; kernels in csrc/tdr_recover_sensor.hip): the launcher that composes the
// list, the candidates, the filter's own scoring launches and the selection, tdr_filter_inject_sensor,
// tdr_filter_recovery_step_sensor.
#include "tdr_host.h"

namespace tdrh {   // called by tdr_host_grid.cpp too (prototypes in tdr_host.h)
int inject_check_p(double p, int heading_mode, const char* who) {
  if (!std::isfinite(p) || p < 0. || p > 1.) return failh(TDR_ERR_ARG, "%s: p = %g (0 .. 1)", who, p);
  if (heading_mode < 0 || heading_mode > 1) return failh(TDR_ERR_ARG, "%s: heading_mode = %d (0 .. 1)", who, heading_mode);
  return TDR_OK;
}
void inject_note(tdr_filter* f, uint32_t threshold24, int heading_mode) {
  if (threshold24 == 0) return;
  f->states_changed();
  if (heading_mode == 0) f->maybe_uninit = true;
}
}  // namespace tdrh

namespace {
thread_local StageCtx g_inject_stage;

int recovery_check(const tdr_recovery_params* rp, const char* who) {
  if (!rp) return failh(TDR_ERR_ARG, "%s: null parameters", who);
  if (!(rp->alpha_slow > 0.) || !(rp->alpha_slow <= 1.)) return failh(TDR_ERR_ARG, "%s: alpha_slow = %g (0 < alpha <= 1)", who, rp->alpha_slow);
  if (!(rp->alpha_fast > 0.) || !(rp->alpha_fast <= 1.)) return failh(TDR_ERR_ARG, "%s: alpha_fast = %g (0 < alpha <= 1)", who, rp->alpha_fast);
  return inject_check_p(rp->p_max, rp->heading_mode, who);
}
// what every injection asks of a filter, and its map's road list
int inject_check_filter(tdr_filter* f, const char* who, const uint32_t** road, int64_t* n_road) {
  if (f->comm) return failh(TDR_ERR_ARG, "%s: the filter is sharded (the handle path for a rank's slice is not built)", who);
  if (f->n < 1) return failh(TDR_ERR_ARG, "%s: the filter has no particles", who);
  if (!f->map) return failh(TDR_ERR_ARG, "%s: the filter has no map", who);
  return tdr_map_road_cells(f->map, road, n_road);
}
// `s` continues after everything already queued on the filters' own streams
int inject_wait_filters(tdr_filter* const* fl, int k, hipStream_t s) {
  std::vector<hipStream_t> streams;
  for (int i = 0; i < k; i++)
    if (fl[i]->stream != s) streams.push_back(fl[i]->stream);
  std::sort(streams.begin(), streams.end());
  streams.erase(std::unique(streams.begin(), streams.end()), streams.end());
  for (hipStream_t fs : streams) {
    hipEvent_t e = nullptr;
    HTRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    int rc = TDR_OK;
    if (hipEventRecord(e, fs) != hipSuccess || hipStreamWaitEvent(s, e, 0) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_inject: stream order");
    (void)hipEventDestroy(e);
    if (rc != TDR_OK) return rc;
  }
  return TDR_OK;
}

// ---- sensor resetting (include/tdr.h, "sensor resetting"; kernels in csrc/tdr_recover_sensor.hip) ---------------------------
int sensor_check(int candidates, float res, const char* who) {
  if (candidates < 1 || candidates > 4096) return failh(TDR_ERR_ARG, "%s: candidates = %d (1 .. 4096)", who, candidates);
  if (!std::isfinite(res) || !(res > 0.f)) return failh(TDR_ERR_ARG, "%s: res = %g (finite, > 0)", who, (double)res);
  return TDR_OK;
}
}  // namespace

namespace tdrh {   // called by tdr_host_grid.cpp too (prototypes in tdr_host.h)
// The scan of the call as filter_score (tdr_host_filter.cpp) takes it, checked; nothing is written.  NULL, NULL: the packed
// scan the filter keeps from the last scoring call that was handed images.
int sensor_check_scan(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, const char* who) {
  tdr_map* m = f->map;
  if (!m->have_map) return failh(TDR_ERR_ARG, "%s: no map", who);
  if (!f->cart && (m->nb < 1 || !m->tab.p)) return failh(TDR_ERR_ARG, "%s: samplePtsPolar was never called", who);
  if (f->cart && (m->win_rows < 1 || m->win_cols < 1)) return failh(TDR_ERR_ARG, "%s: the map has no window", who);
  const int ncls = m->desc.ncls, nb = f->cart ? m->win_rows : m->nb, nr = f->cart ? m->win_cols : m->nr;
  if (scan_imgs) return TDR_OK;
  if (renderer) {
    if (!renderer->have_scan) return failh(TDR_ERR_ARG, "%s: no scan", who);
    if (renderer->ncls != ncls || renderer->rows != nb || renderer->cols != nr)
      return failh(TDR_ERR_ARG, "%s: render shape %dx%dx%d does not match the map's %dx%dx%d", who, renderer->ncls,
                   renderer->rows, renderer->cols, ncls, nb, nr);
    if (f->cart && renderer->polar) return failh(TDR_ERR_ARG, "%s: a Cartesian filter needs a Cartesian render", who);
    return TDR_OK;
  }
  if (!f->scan_pk.p || f->scan_pk.n < (size_t)nb * nr * tdr_rec_floats(ncls))
    return failh(TDR_ERR_ARG, "%s: no scan (the filter keeps none before its first update or compute_weights from images)", who);
  return TDR_OK;
}
int sensor_take_scan(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, const float** pk) {
  tdr_map* m = f->map;
  const int ncls = m->desc.ncls, nb = f->cart ? m->win_rows : m->nb, nr = f->cart ? m->win_cols : m->nr;
  const size_t P = (size_t)nb * nr;
  *pk = f->scan_pk.p;
  if (scan_imgs) {
    TTRY(f->scan_img.resize(P * ncls));
    TTRY(f->scan_pk.resize(P * tdr_rec_floats(ncls)));
    HTRY(hipMemcpyAsync(f->scan_img.p, scan_imgs, P * ncls * sizeof(float), hipMemcpyHostToDevice, f->stream));
    TTRY(tdr_k_pack_scan(f->scan_img.p, ncls, nb, nr, f->scan_pk.p, f->stream));
    *pk = f->scan_pk.p;
  } else if (renderer) {
    *pk = renderer->pk.p;
    TTRY(renderer_wait_render(renderer, f->stream));
  }
  return TDR_OK;
}
// The raw weights tdr_filter_compute_weights gives nc particles in the states cst (plane stride ccap) in THIS filter:
// filter_score's launches (tdr_host_filter.cpp) with n_total = f->n; init_search: the 40-rotation search first;
// uniform_scale: what set_states would note for the candidates (0: their scales differ), for the polar launch.
int sensor_score(tdr_filter* f, const float* pk, float res, int64_t nc, int64_t ccap, bool init_search, float uniform_scale) {
  tdr_map* m = f->map;
  hipStream_t s = f->stream;
  const int ncls = m->desc.ncls, nb = f->cart ? m->win_rows : m->nb, nr = f->cart ? m->win_cols : m->nr;
  if (f->cart) {
    if (init_search) {
      TTRY(f->sr_init_ws.resize(tdr_score_cart_init_workspace_floats(ncls, nb, nr, nc, f->n)));
      TTRY(tdr_k_score_cart_init(&m->desc, pk, nb, nr, res, &f->fp, f->sr_cst.p, ccap, nc, f->n, f->sr_init_ws.p, s));
    }
    TTRY(f->sr_tmp.resize(tdr_locality_pose_tmp_ints(nc) + 2));
    TTRY(tdr_k_locality_order_pose(f->sr_cst.p, ccap, nc, m->desc.rows, m->desc.cols, (float)(nb + nr) / 16.f, f->sr_perm.p,
                                   f->sr_tmp.p, s));
    TTRY(f->sr_ws.resize(tdr_score_cart_workspace_floats(ncls, nb, nr, nc, f->n)));
    return tdr_k_score_cart(&m->desc, pk, nb, nr, res, &f->fp, f->sr_cst.p, ccap, nc, f->n, f->sr_perm.p, f->sr_craw.p,
                            f->sr_ws.p, s);
  }
  TTRY(f->sr_tmp.resize(tdr_locality_tmp_ints(nc, m->desc.rows, m->desc.cols)));
  TTRY(tdr_k_locality_order(f->sr_cst.p, ccap, nc, m->desc.rows, m->desc.cols, f->sr_perm.p, f->sr_tmp.p, s));
  TTRY(f->sr_ws.resize(tdr_score_workspace_floats(ncls, nb, nr, nc, f->n)));
  // the search over a filter of this many particles reads pre-split half records, as the filter's own does
  if (init_search) TTRY(map_rec16_alloc(m, f->n));
  const bool uses_rec16 = init_search && m->desc.rec16 && f->n >= tdr_cfg().rec16_min;
  if (uses_rec16) TTRY(map_rec16_begin(m, s));
  TTRY(tdr_k_score_polar(&m->desc, m->tab.p, pk, nb, nr, res, &f->fp, f->sr_cst.p, ccap, nc, f->n, f->sr_perm.p,
                         uniform_scale, init_search ? 1 : 0, f->sr_craw.p, f->sr_ws.p, s));
  if (uses_rec16) TTRY(map_rec16_end(m, s));
  return TDR_OK;
}
}  // namespace tdrh

namespace {
// The launcher: the list and ONE wait for its length, then per chunk of whole slots the candidates, their scores in this
// filter and the pick.  written_dev (may be NULL) is incremented by the written slots; *listed: the list's length.
int sensor_inject(tdr_filter* f, const float* pk, float res, uint32_t th, int C, int heading_mode, uint64_t seed,
                  const uint32_t* road, int64_t n_road, int64_t* written_dev, int64_t* listed_out) {
  hipStream_t s = f->stream;
  const int64_t n = f->n;
  *listed_out = 0;
  TTRY(f->sr_list.resize((size_t)n));
  TTRY(f->sr_count.resize(2));
  TTRY(f->sr_list_ws.resize(tdr_inject_list_workspace_bytes(n)));
  TTRY(tdr_k_inject_list(n, 0, seed, f->step, th, f->sr_list.p, f->sr_count.p, f->sr_list_ws.p, 0, s));
  int64_t listed = 0;
  HTRY(hipMemcpyAsync(&listed, f->sr_count.p, sizeof(listed), hipMemcpyDeviceToHost, s));
  HTRY(hipStreamSynchronize(s));
  if (listed < 0 || listed > n) return failh(TDR_ERR_HIP, "filter_inject_sensor: list length %lld out of range", (long long)listed);
  *listed_out = listed;
  if (listed == 0) return TDR_OK;
  f->fp.num_classes = f->map->desc.ncls;
  const int64_t per = std::min<int64_t>(std::max<int64_t>(1, tdr_cfg().inject_cand_chunk / C), listed);   // slots a chunk
  const int64_t ccap = (per * C + 63) / 64 * 64;
  TTRY(f->sr_cst.resize((size_t)TDR_ST_FIELDS * ccap));
  TTRY(f->sr_craw.resize((size_t)ccap));
  TTRY(f->sr_perm.resize((size_t)ccap));
  for (int64_t lo = 0; lo < listed; lo += per) {
    const int64_t mslots = std::min(per, listed - lo), nc = mslots * C;
    TTRY(tdr_k_inject_candidates(f->st.p, f->cap, n, 0, f->sr_list.p, lo, mslots, C, &f->map->desc, road, n_road, seed, f->step,
                                 heading_mode, f->sr_cst.p, ccap, s));
    TTRY(sensor_score(f, pk, res, nc, ccap, heading_mode == 0, f->uniform_scale));
    TTRY(tdr_k_inject_select(f->st.p, f->cap, n, f->sr_list.p, lo, mslots, C, f->sr_cst.p, ccap, f->sr_craw.p, nullptr,
                             written_dev, s));
  }
  return TDR_OK;
}
}  // namespace

extern "C" {
double tdr_recovery_track_host(tdr_recovery_state* s, double w_avg, const tdr_recovery_params* p) {
  if (!s || !p || !std::isfinite(w_avg) || !(w_avg > 0.)) return 0.;
  s->w_slow = s->w_slow == 0. ? w_avg : s->w_slow + p->alpha_slow * (w_avg - s->w_slow);
  s->w_fast = s->w_fast == 0. ? w_avg : s->w_fast + p->alpha_fast * (w_avg - s->w_fast);
  return std::min(p->p_max, std::max(0., 1. - s->w_fast / s->w_slow));
}
void tdr_recovery_reset_host(tdr_recovery_state* s) {
  if (s) s->w_slow = s->w_fast = 0.;
}

int tdr_map_road_cells(tdr_map* m, const uint32_t** cells_dev, int64_t* n_road) {
  if (!m || !cells_dev || !n_road) return failh(TDR_ERR_ARG, "map_road_cells: null pointer");
  if (!m->desc.rec) return failh(TDR_ERR_ARG, "map_road_cells: the map has no records");
  if (m->road_at != m->rec_writes) {
    const size_t ncell = (size_t)m->desc.rows * m->desc.cols;
    HTRY(hipDeviceSynchronize());   // (an injection on another stream may still read the old list)
    TTRY(m->road.resize(ncell));
    TTRY(m->road_count.resize(1));
    TTRY(m->road_ws.resize(tdr_map_road_workspace_bytes(m->desc.rows, m->desc.cols)));
    TTRY(tdr_k_map_road_cells(&m->desc, m->road.p, m->road_count.p, m->road_ws.p, nullptr));
    int64_t cnt = 0;
    HTRY(hipMemcpy(&cnt, m->road_count.p, sizeof(cnt), hipMemcpyDeviceToHost));
    m->road_n = cnt;
    m->road_at = m->rec_writes;
  }
  if (m->road_n < 1) return failh(TDR_ERR_ARG, "map_road_cells: the map has no road cell");
  *cells_dev = m->road.p;
  *n_road = m->road_n;
  return TDR_OK;
}

int tdr_map_read_road_cells(tdr_map* m, uint32_t* out_host, int64_t capacity, int64_t* n_road) {
  const uint32_t* dev = nullptr;
  TTRY(tdr_map_road_cells(m, &dev, n_road));
  if (!out_host) return TDR_OK;
  if (capacity < *n_road) return failh(TDR_ERR_ARG, "map_read_road_cells: %lld road cells, room for %lld", (long long)*n_road, (long long)capacity);
  HTRY(hipMemcpy(out_host, dev, (size_t)*n_road * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return TDR_OK;
}

int tdr_filter_get_weight_stats(tdr_filter* f, float out8[8]) {
  if (!f || !out8) return failh(TDR_ERR_ARG, "filter_get_weight_stats: null pointer");
  if (!f->have_ml) return failh(TDR_ERR_ARG, "filter_get_weight_stats: no update yet");
  HTRY(hipMemcpyAsync(out8, f->info.p, 8 * sizeof(float), hipMemcpyDeviceToHost, f->stream));
  HTRY(hipStreamSynchronize(f->stream));
  return TDR_OK;
}

int tdr_filter_inject(tdr_filter* f, double p, int heading_mode, uint64_t seed, int64_t* injected_out) {
  if (!f) return failh(TDR_ERR_ARG, "filter_inject: null filter");
  TTRY(inject_check_p(p, heading_mode, "filter_inject"));
  const uint32_t* road = nullptr;
  int64_t n_road = 0;
  TTRY(inject_check_filter(f, "filter_inject", &road, &n_road));
  const uint32_t th = tdr_inject_threshold_host(p);
  int64_t* out_dev = nullptr;
  if (injected_out) {
    TTRY(f->inject_out.resize(1));
    out_dev = f->inject_out.p;
    HTRY(hipMemsetAsync(out_dev, 0, sizeof(int64_t), f->stream));
  }
  TTRY(tdr_k_inject(f->st.p, f->cap, f->n, 0, &f->map->desc, road, n_road, seed, f->step, th, heading_mode, out_dev, f->stream));
  inject_note(f, th, heading_mode);
  if (injected_out) {
    HTRY(hipMemcpyAsync(injected_out, out_dev, sizeof(int64_t), hipMemcpyDeviceToHost, f->stream));
    HTRY(hipStreamSynchronize(f->stream));
  }
  return TDR_OK;
}

int tdr_filter_recovery_step(tdr_filter* f, tdr_recovery_state* s, const tdr_recovery_params* rp, double* p_out,
                             int64_t* injected_out) {
  if (!f || !s) return failh(TDR_ERR_ARG, "filter_recovery_step: null pointer");
  TTRY(recovery_check(rp, "filter_recovery_step"));
  if (f->comm) return failh(TDR_ERR_ARG, "filter_recovery_step: the filter is sharded (the handle path for a rank's slice is not built)");
  if (f->n < 1) return failh(TDR_ERR_ARG, "filter_recovery_step: the filter has no particles");
  float st8[8];
  TTRY(tdr_filter_get_weight_stats(f, st8));
  tdr_recovery_state next = *s;
  const double p = tdr_recovery_track_host(&next, (double)st8[2], rp);
  int64_t injected = 0;
  if (p > 0.) {
    TTRY(tdr_filter_inject(f, p, rp->heading_mode, rp->seed, injected_out ? &injected : nullptr));
    tdr_recovery_reset_host(&next);
  }
  *s = next;
  if (p_out) *p_out = p;
  if (injected_out) *injected_out = injected;
  return TDR_OK;
}

int tdr_filter_inject_sensor(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, float res, double p,
                             int candidates, int heading_mode, uint64_t seed, int64_t* injected_out) {
  const char* who = "filter_inject_sensor";
  if (!f) return failh(TDR_ERR_ARG, "%s: null filter", who);
  TTRY(inject_check_p(p, heading_mode, who));
  TTRY(sensor_check(candidates, res, who));
  const uint32_t* road = nullptr;
  int64_t n_road = 0;
  TTRY(inject_check_filter(f, who, &road, &n_road));
  TTRY(sensor_check_scan(f, scan_imgs, renderer, who));
  const uint32_t th = tdr_inject_threshold_host(p);
  const float* pk = nullptr;
  int64_t* out_dev = nullptr;
  if (injected_out) {
    TTRY(f->inject_out.resize(1));
    out_dev = f->inject_out.p;
    HTRY(hipMemsetAsync(out_dev, 0, sizeof(int64_t), f->stream));
  }
  int64_t listed = 0;
  if (th != 0) {
    TTRY(sensor_take_scan(f, scan_imgs, renderer, &pk));
    const int rc = sensor_inject(f, pk, res, th, candidates, heading_mode, seed, road, n_road, out_dev, &listed);
    if (listed > 0) inject_note(f, th, heading_mode);   // (whatever a later chunk's error left written)
    TTRY(rc);
    if (renderer && !scan_imgs) TTRY(renderer_note_read(renderer, f->stream));
  }
  if (injected_out) {
    HTRY(hipMemcpyAsync(injected_out, out_dev, sizeof(int64_t), hipMemcpyDeviceToHost, f->stream));
    HTRY(hipStreamSynchronize(f->stream));
  }
  return TDR_OK;
}

int tdr_filter_recovery_step_sensor(tdr_filter* f, tdr_recovery_state* s, const tdr_recovery_params* rp, int candidates,
                                    const float* scan_imgs, const tdr_renderer* renderer, float res, double* p_out,
                                    int64_t* injected_out) {
  const char* who = "filter_recovery_step_sensor";
  if (!f || !s) return failh(TDR_ERR_ARG, "%s: null pointer", who);
  TTRY(recovery_check(rp, who));
  TTRY(sensor_check(candidates, res, who));
  if (f->comm) return failh(TDR_ERR_ARG, "%s: the filter is sharded (the handle path for a rank's slice is not built)", who);
  if (f->n < 1) return failh(TDR_ERR_ARG, "%s: the filter has no particles", who);
  float st8[8];
  TTRY(tdr_filter_get_weight_stats(f, st8));
  tdr_recovery_state next = *s;
  const double p = tdr_recovery_track_host(&next, (double)st8[2], rp);
  int64_t injected = 0;
  if (p > 0.) {
    TTRY(tdr_filter_inject_sensor(f, scan_imgs, renderer, res, p, candidates, rp->heading_mode, rp->seed,
                                  injected_out ? &injected : nullptr));
    tdr_recovery_reset_host(&next);
  }
  *s = next;
  if (p_out) *p_out = p;
  if (injected_out) *injected_out = injected;
  return TDR_OK;
}

int tdr_batch_inject(tdr_filter* const* filters, int k, const double* p, int heading_mode, const uint64_t* seeds,
                     int64_t* injected_out, void* stream) {
  if (k < 1) return failh(TDR_ERR_ARG, "batch_inject: k = %d, at least one filter is needed", k);
  if (!filters || !p || !seeds) return failh(TDR_ERR_ARG, "batch_inject: null array");
  for (int i = 0; i < k; i++)
    if (!filters[i]) return failh(TDR_ERR_ARG, "batch_inject: filter %d is null", i);
  for (int i = 0; i < k; i++) TTRY(inject_check_p(p[i], heading_mode, "batch_inject"));
  {
    std::vector<const tdr_filter*> seen(filters, filters + k);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return failh(TDR_ERR_ARG, "batch_inject: a filter appears twice in the batch");
  }
  std::vector<const uint32_t*> road((size_t)k);
  std::vector<int64_t> n_road((size_t)k);
  for (int i = 0; i < k; i++) TTRY(inject_check_filter(filters[i], "batch_inject", &road[(size_t)i], &n_road[(size_t)i]));
  hipStream_t s = (hipStream_t)stream;
  // staging: [k] jobs and the [k] counts, uploaded as zeros with the jobs and read back in place
  const size_t out_off = align64(sizeof(tdr_inject_job) * (size_t)k), bytes = out_off + sizeof(int64_t) * (size_t)k;
  StageCtx& B = g_inject_stage;
  TTRY(B.reserve(bytes, bytes, s));
  TTRY(inject_wait_filters(filters, k, s));
  tdr_inject_job* jobs = reinterpret_cast<tdr_inject_job*>(B.host);
  int64_t* out_host = reinterpret_cast<int64_t*>(B.host + out_off);
  int64_t* out_dev = reinterpret_cast<int64_t*>(B.dev.p + out_off);
  for (int i = 0; i < k; i++) {
    const tdr_filter* f = filters[i];
    jobs[i] = tdr_inject_job{f->st.p, f->cap, f->n, 0, road[(size_t)i], n_road[(size_t)i], f->map->desc.cols, f->map->desc.resolution,
                             seeds[i], f->step, tdr_inject_threshold_host(p[i]), heading_mode, injected_out ? out_dev + i : nullptr};
    out_host[i] = 0;
  }
  HTRY(hipMemcpyAsync(B.dev.p, B.host, bytes, hipMemcpyHostToDevice, s));
  TTRY(tdr_k_inject_jobs(reinterpret_cast<const tdr_inject_job*>(B.dev.p), k, s));
  if (injected_out) HTRY(hipMemcpyAsync(out_host, out_dev, sizeof(int64_t) * (size_t)k, hipMemcpyDeviceToHost, s));
  HTRY(hipEventRecord(B.done, s));
  HTRY(hipEventRecord(B.uploaded, s));
  for (int i = 0; i < k; i++) inject_note(filters[i], jobs[i].threshold24, heading_mode);
  // the filters' own streams continue after the injection
  for (int i = 0; i < k; i++)
    if (filters[i]->stream != s) HTRY(hipStreamWaitEvent(filters[i]->stream, B.done, 0));
  if (injected_out) {
    HTRY(hipEventSynchronize(B.done));   // the one wait of the call
    for (int i = 0; i < k; i++) injected_out[i] = out_host[i];
  }
  return TDR_OK;
}
}  // extern "C"
