// tdr_host_batch.cpp — the batched calls on many filters of one map: tdr_batch_step (csrc/tdr_batch.hip) and the two ends
// of a batched node loop, tdr_batch_render_polar and tdr_batch_pose (csrc/tdr_batch_loop.hip), and its pictures,
// tdr_batch_scan_pictures (csrc/tdr_scan_viz.hip) and tdr_batch_visualize (csrc/tdr_viz.hip).  Their per-thread staging
// contexts live here and nowhere else.
#include "tdr_host.h"

// ---- batched filters (tdr_batch_step): many filters on one map, one launch per stage -------------------------------------
// Each filter keeps what is its own: its generator pipe draws its normals and its uniform (per-filter mt19937 streams) and
// its scan is packed into its own buffer.  The stages of the step are then one launch each over a table of the filters:
// propagate and resample (csrc/tdr_batch.hip), the float scoring launch (tdr_score.hip), the statistics and the running
// sum (tdr_prefix.hip).  The locality order is left out: it never changes results (tdr.h).
namespace {
thread_local int g_batch_stats[2] = {0, 0};   // filters of this thread's last batch: batched, standalone
struct BatchCtx {   // per thread: the tables, staged in pinned host memory and copied to the device, reused from call to call
  char* host = nullptr;
  DevBuf<char> dev;
  size_t cap = 0;
  hipEvent_t uploaded = nullptr;   // the last call's copy has read `host`
  hipEvent_t done = nullptr;       // the last call's kernels have read `dev`
  ~BatchCtx() {
    if (uploaded) { (void)hipEventSynchronize(uploaded); (void)hipEventDestroy(uploaded); }
    if (done) { (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
    if (host) (void)hipHostFree(host);
  }
};
thread_local BatchCtx g_batch;
}  // namespace

extern "C" {
int tdr_batch_last_stats(int* batched, int* standalone) {
  if (batched) *batched = g_batch_stats[0];
  if (standalone) *standalone = g_batch_stats[1];
  return TDR_OK;
}

static bool batch_eligible(const tdr_filter* f) {
  const tdr_map* m = f->map;
  // (a filter that may hold a particle without a heading: only with tdr_config_tuning("batch_init_search"))
  const bool uninit_ok = !f->maybe_uninit || tdr_cfg().batch_init_search == 1;
  return !f->comm && rng_device_capable(f) && uninit_ok && f->n >= 1 && f->n <= 32768 &&
         tdr_score_polar_float_form(&m->desc, m->nb, m->nr, f->n, f->n);
}

int tdr_batch_step(tdr_filter* const* filters, int k, const tdr_batch_input* in, void* stream) {
  g_batch_stats[0] = g_batch_stats[1] = 0;
  if (k < 1) return failh(TDR_ERR_ARG, "batch_step: k = %d, at least one filter is needed", k);
  if (!filters || !in) return failh(TDR_ERR_ARG, "batch_step: null %s array", !filters ? "filter" : "input");
  for (int i = 0; i < k; i++)
    if (!filters[i]) return failh(TDR_ERR_ARG, "batch_step: filter %d is null", i);
  {
    std::vector<const tdr_filter*> seen(filters, filters + k);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return failh(TDR_ERR_ARG, "batch_step: a filter appears twice in the batch");
  }
  tdr_map* m = filters[0]->map;
  for (int i = 0; i < k; i++)
    if (filters[i]->map != m) return failh(TDR_ERR_ARG, "batch_step: filter %d is on another map than filter 0", i);
  for (int i = 0; i < k; i++)
    if (filters[i]->cart) return failh(TDR_ERR_ARG, "batch_step: filter %d is a Cartesian filter (batches are polar)", i);
  if (!m || !m->have_map) return failh(TDR_ERR_ARG, "batch_step: the filters' map holds no map");
  if (m->nb < 1 || !m->tab.p) return failh(TDR_ERR_ARG, "batch_step: samplePtsPolar was never called on the map");
  const int ncls = m->desc.ncls, nb = m->nb, nr = m->nr;
  for (int i = 0; i < k; i++) {
    const tdr_renderer* r = in[i].renderer;
    if (!in[i].scan_imgs && !r) return failh(TDR_ERR_ARG, "batch_step: input %d has no scan", i);
    if (!in[i].scan_imgs && !r->have_scan) return failh(TDR_ERR_ARG, "batch_step: input %d: the renderer has no render", i);
    if (!in[i].scan_imgs && (r->ncls != ncls || r->rows != nb || r->cols != nr))
      return failh(TDR_ERR_ARG, "batch_step: input %d: render shape %dx%dx%d does not match the map's %dx%dx%d", i, r->ncls,
                   r->rows, r->cols, ncls, nb, nr);
  }
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> fast;
  for (int i = 0; i < k; i++) {
    tdr_filter* f = filters[i];
    if (batch_eligible(f)) { fast.push_back(i); continue; }
    TTRY(tdr_filter_propagate(f, in[i].tx, in[i].ty, in[i].omega));
    TTRY(tdr_filter_update(f, in[i].scan_imgs, in[i].renderer, in[i].res, in[i].n_target));
    g_batch_stats[1]++;
  }
  const int kf = (int)fast.size();
  if (kf == 0) return TDR_OK;

  BatchCtx& B = g_batch;
  // the batched filters whose 40-rotation search is part of the scoring stage; the largest decides about the map's scratch
  int k_init = 0;
  bool uses_rec16 = false;
  for (int j = 0; j < kf; j++) {
    const tdr_filter* f = filters[fast[j]];
    if (!f->maybe_uninit) continue;
    k_init++;
    TTRY(map_rec16_alloc(m, f->n));
    uses_rec16 |= m->desc.rec16 && f->n >= tdr_cfg().rec16_min;
  }
  // one staging area: [kf] TdrBatchEntry, then the scoring launch's tables (tdr_batch_score_stage_bytes)
  const size_t ent_bytes = (sizeof(TdrBatchEntry) * (size_t)kf + 63) / 64 * 64;
  const size_t stage = ent_bytes + tdr_batch_score_stage_bytes(kf, k_init);
  if (!B.uploaded) HTRY(hipEventCreateWithFlags(&B.uploaded, hipEventDisableTiming));
  if (!B.done) HTRY(hipEventCreateWithFlags(&B.done, hipEventDisableTiming));
  HTRY(hipEventSynchronize(B.uploaded));   // (the previous call's copy has left the pinned buffer)
  if (B.cap < stage) {
    HTRY(hipEventSynchronize(B.done));     // (and its kernels the device buffer that is replaced)
    if (B.host) HTRY(hipHostFree(B.host));
    B.host = nullptr;
    B.cap = 0;
    HTRY(hipHostMalloc((void**)&B.host, stage));
    B.cap = stage;
  }
  TTRY(B.dev.resize(stage));
  TdrBatchEntry* const tab = reinterpret_cast<TdrBatchEntry*>(B.host);
  TdrBatchEntry* const tab_dev = reinterpret_cast<TdrBatchEntry*>(B.dev.p);

  // the batch stream continues after the batched renders it reads, everything already queued on the filters' own
  // streams, and after the previous batch's kernels have read the device tables this call overwrites
  for (int j = 0; j < kf; j++)
    if (!in[fast[j]].scan_imgs) TTRY(renderer_wait_render(in[fast[j]].renderer, s));
  std::vector<hipEvent_t> evs((size_t)kf, nullptr);
  auto destroy_events = [&]() { for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e); };
  int rc = TDR_OK;
  if (hipStreamWaitEvent(s, B.done, 0) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_step: stream wait");
  for (int j = 0; j < kf && rc == TDR_OK; j++) {
    tdr_filter* f = filters[fast[j]];
    rc = rng_to_device(f);
    if (rc == TDR_OK && hipEventCreateWithFlags(&evs[j], hipEventDisableTiming) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_step: event");
    if (rc == TDR_OK && hipEventRecord(evs[j], f->stream) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_step: event record");
    if (rc == TDR_OK && hipStreamWaitEvent(s, evs[j], 0) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_step: stream wait");
  }
  if (rc != TDR_OK) { destroy_events(); return rc; }

  // per filter: its generator's normals and uniform (the pipe orders its own side stream against `s`; the draws keep the
  // standalone order), its scan packed into its own buffer, and its table entries
  const size_t P = (size_t)nb * nr, pk_floats = P * tdr_rec_floats(ncls);
  std::vector<TdrBatchScoreIn> sin((size_t)kf);
  int blocks_prop = 0, blocks_res = 0;
  int64_t n_big = 1;
  for (int j = 0; j < kf && rc == TDR_OK; j++) {
    tdr_filter* f = filters[fast[j]];
    const tdr_batch_input& x = in[fast[j]];
    TdrBatchEntry& e = tab[j];
    e = TdrBatchEntry{};
    f->states_changed();
    f->fp.num_classes = ncls;
    rc = tdr_rng_pipe_normals(f->pipe, f->n, 0, f->n, f->scale_frozen ? 1 : 0, &e.z4, s);
    f->prop_calls++;
    if (rc == TDR_OK) rc = tdr_rng_pipe_uniform(f->pipe, &e.shift, s);
    if (rc == TDR_OK) rc = f->ml_dev.resize(12);
    const float* pk = nullptr;
    if (rc == TDR_OK && x.scan_imgs) {
      rc = f->scan_img.resize(P * ncls);
      if (rc == TDR_OK) rc = f->scan_pk.resize(pk_floats);
      if (rc == TDR_OK && hipMemcpyAsync(f->scan_img.p, x.scan_imgs, P * ncls * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess)
        rc = failh(TDR_ERR_HIP, "batch_step: scan upload");
      if (rc == TDR_OK) rc = tdr_k_pack_scan(f->scan_img.p, ncls, nb, nr, f->scan_pk.p, s);
      pk = f->scan_pk.p;
    } else {
      pk = x.renderer->pk.p;
    }
    if (rc == TDR_OK) rc = f->ws.resize(tdr_score_workspace_floats(ncls, nb, nr, f->n, f->n));
    int64_t n_new = f->n;
    if (x.n_target >= 0) n_new = std::max<int64_t>(1, std::min<int64_t>(x.n_target, f->n_max));
    e.st = f->st.p; e.st_new = f->st_new.p; e.last_dist = f->last_dist.p; e.cap = f->cap; e.n = f->n; e.n_new = n_new;
    e.tx = x.tx; e.ty = x.ty; e.omega = x.omega; e.pos_cov = f->fp.pos_cov; e.theta_cov = f->fp.theta_cov;
    e.scale_freeze = f->scale_frozen ? 1 : 0;
    e.raw_w = f->raw_w.p; e.w_out = f->w.p; e.info_out = f->info.p; e.runmax_out = f->runmax.p;
    e.runmax = f->runmax.p; e.info = f->info.p; e.idx = f->idx.p; e.ml = f->ml_dev.p;
    e.blk_prop = blocks_prop;
    blocks_prop += (int)((f->n + TDR_BATCH_THREADS - 1) / TDR_BATCH_THREADS);
    e.blk_res = blocks_res;
    blocks_res += (int)((n_new + TDR_BATCH_THREADS - 1) / TDR_BATCH_THREADS);
    n_big = std::max(n_big, f->n);
    sin[j] = TdrBatchScoreIn{pk, x.res, &f->fp, f->st.p, f->cap, f->n, f->uniform_scale, f->raw_w.p, f->ws.p,
                             f->maybe_uninit ? 1 : 0};
  }
  if (rc == TDR_OK) rc = tdr_batch_score_build(&m->desc, m->tab.p, nb, nr, kf, sin.data(), B.host + ent_bytes);
  if (rc == TDR_OK && hipMemcpyAsync(B.dev.p, B.host, stage, hipMemcpyHostToDevice, s) != hipSuccess)
    rc = failh(TDR_ERR_HIP, "batch_step: table upload");
  if (rc == TDR_OK && hipEventRecord(B.uploaded, s) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_step: event record");
  // one launch per stage over the whole batch (the scoring launch: utab, score, finalize)
  if (rc == TDR_OK) rc = tdr_batch_propagate(tab_dev, kf, blocks_prop, s);
  if (rc == TDR_OK && uses_rec16) rc = map_rec16_begin(m, s);
  if (rc == TDR_OK) rc = tdr_batch_score_launch(&m->desc, m->tab.p, nb, nr, kf, B.host + ent_bytes, B.dev.p + ent_bytes, s);
  if (rc == TDR_OK && uses_rec16) rc = map_rec16_end(m, s);
  if (rc == TDR_OK) rc = tdr_batch_update_weights(tab_dev, kf, n_big, s);
  if (rc == TDR_OK) rc = tdr_batch_prefix(tab_dev, kf, n_big, s);
  if (rc == TDR_OK) rc = tdr_batch_resample(tab_dev, kf, blocks_res, s);
  if (rc == TDR_OK && hipEventRecord(B.done, s) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_step: event record");
  for (int j = 0; j < kf && rc == TDR_OK; j++)
    if (!in[fast[j]].scan_imgs) rc = renderer_note_read(in[fast[j]].renderer, s);
  if (rc != TDR_OK) { destroy_events(); return rc; }
  for (int j = 0; j < kf; j++) {
    tdr_filter* f = filters[fast[j]];
    f->have_ml = true;
    f->states_changed();
    // the search initialises every un-gated particle; only gated ones can stay un-initialised (filter_score)
    if (f->maybe_uninit && !(f->fp.force_on_map || f->fp.fixed_scale < 0)) f->maybe_uninit = false;
    std::swap(f->st.p, f->st_new.p);   // particle_filter.cpp:187
    f->n = tab[j].n_new;
    f->step++;
  }
  // the filters' own streams continue after the batch
  for (int j = 0; j < kf && rc == TDR_OK; j++)
    if (hipStreamWaitEvent(filters[fast[j]]->stream, B.done, 0) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_step: stream wait");
  destroy_events();
  g_batch_stats[0] = kf;
  return rc;
}
}  // extern "C"

// ---- the two ends of a batched node loop: tdr_batch_render_polar, tdr_batch_pose (csrc/tdr_batch_loop.hip) ---------------
namespace {
thread_local StageCtx g_render_stage, g_pose_stage;
}  // namespace

extern "C" {
int tdr_batch_render_polar(tdr_renderer* const* r, int k, const tdr_batch_cloud* clouds, float ang_res, int ncls, int nb,
                           int nr, void* stream) {
  if (k < 1) return failh(TDR_ERR_ARG, "batch_render: k = %d, at least one renderer is needed", k);
  if (!r || !clouds) return failh(TDR_ERR_ARG, "batch_render: null %s array", !r ? "renderer" : "cloud");
  for (int i = 0; i < k; i++)
    if (!r[i]) return failh(TDR_ERR_ARG, "batch_render: renderer %d is null", i);
  {
    std::vector<const tdr_renderer*> seen(r, r + k);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return failh(TDR_ERR_ARG, "batch_render: a renderer appears twice in the batch");
  }
  for (int i = 0; i < k; i++) {
    const tdr_batch_cloud& c = clouds[i];
    if (c.n < 0 || (c.n > 0 && !c.pts)) return failh(TDR_ERR_ARG, "batch_render: cloud %d: null points", i);
    if (c.stride < 3 || c.ioff < 0 || c.ioff >= c.stride)
      return failh(TDR_ERR_ARG, "batch_render: cloud %d: bad point stride / offset %d / %d", i, c.stride, c.ioff);
    if (!(c.res > 0.f)) return failh(TDR_ERR_ARG, "batch_render: cloud %d: resolution must be > 0", i);
  }
  if (!(ang_res > 0.f)) return failh(TDR_ERR_ARG, "batch_render: angular resolution must be > 0");
  if (ncls < 1 || ncls > TDR_MAX_CLASSES || nb < 1 || nr < 1)
    return failh(TDR_ERR_ARG, "batch_render: bad image shape %dx%dx%d", ncls, nb, nr);
  if ((int64_t)ncls * nb * 4 > 152 * 1024) return failh(TDR_ERR_ARG, "batch_render: ncls*rows too large for one LDS tile (152 KB)");
  TdrBatchRasterShape shape{};
  const bool keyed = tdr_batch_raster_shape(ncls, nb, nr, ang_res, &shape);
  hipStream_t s = (hipStream_t)stream;

  // one staging area: [k] entries, then every cloud's points (64-byte aligned); on the device, the keys follow
  const size_t ent_bytes = align64(sizeof(TdrBatchRasterEntry) * (size_t)k);
  std::vector<size_t> pts_off((size_t)k), key_off((size_t)k);
  size_t stage = ent_bytes;
  for (int i = 0; i < k; i++) {
    pts_off[i] = stage;
    stage += align64((size_t)clouds[i].n * clouds[i].stride * sizeof(float));
  }
  size_t dev_bytes = stage;
  for (int i = 0; i < k; i++) {
    key_off[i] = dev_bytes;
    dev_bytes += align64((size_t)clouds[i].n * sizeof(uint32_t));
  }
  StageCtx& B = g_render_stage;
  TTRY(B.reserve(stage, std::max<size_t>(dev_bytes, 64), s));
  const size_t P = (size_t)nb * nr, rf = (size_t)tdr_rec_floats(ncls);
  for (int i = 0; i < k; i++) {
    tdr_renderer* q = r[i];
    TTRY(q->img.resize(P * ncls));
    TTRY(q->pk.resize(P * rf));
    // img / pk are rewritten: after their readers and the renderer's previous batched render
    for (size_t j = 0; j < q->n_readers; j++) HTRY(hipStreamWaitEvent(s, q->readers[j].second, 0));
    TTRY(renderer_wait_render(q, s));
    if (!q->rendered) HTRY(hipEventCreateWithFlags(&q->rendered, hipEventDisableTiming));
  }
  TdrBatchRasterEntry* tab = reinterpret_cast<TdrBatchRasterEntry*>(B.host);
  int blocks_keys = 0;
  for (int i = 0; i < k; i++) {
    const tdr_batch_cloud& c = clouds[i];
    if (c.n > 0) std::memcpy(B.host + pts_off[i], c.pts, (size_t)c.n * c.stride * sizeof(float));
    TdrBatchRasterEntry& e = tab[i];
    e = TdrBatchRasterEntry{};
    e.pts = reinterpret_cast<const float*>(B.dev.p + pts_off[i]);
    e.lut = r[i]->lut.p;
    e.keys = reinterpret_cast<uint32_t*>(B.dev.p + key_off[i]);
    e.img = r[i]->img.p;
    e.pk = r[i]->pk.p;
    e.n = c.n;
    e.res = c.res;
    e.stride = c.stride;
    e.ioff = c.ioff;
    e.blk_keys = blocks_keys;
    blocks_keys += (int)((c.n + 255) / 256);
  }
  HTRY(hipMemcpyAsync(B.dev.p, B.host, stage, hipMemcpyHostToDevice, s));
  HTRY(hipEventRecord(B.uploaded, s));
  if (keyed) {
    TTRY(tdr_batch_raster(reinterpret_cast<const TdrBatchRasterEntry*>(B.dev.p), k, blocks_keys, shape, s));
  } else {   // shapes the standalone raster scores without keys: its own launch per renderer
    for (int i = 0; i < k; i++)
      TTRY(tdr_k_raster_polar(tab[i].pts, clouds[i].stride, clouds[i].ioff, clouds[i].n, clouds[i].res, ang_res, r[i]->lut.p,
                              ncls, nb, nr, r[i]->img.p, r[i]->pk.p, tab[i].keys, s));
  }
  HTRY(hipEventRecord(B.done, s));
  for (int i = 0; i < k; i++) {
    tdr_renderer* q = r[i];
    HTRY(hipEventRecord(q->rendered, s));
    q->render_async = true;
    q->n_readers = 0;
    q->ncls = ncls;
    q->rows = nb;
    q->cols = nr;
    q->polar = true;
    q->have_scan = true;
  }
  return TDR_OK;
}

int tdr_batch_pose(tdr_filter* const* f, int k, tdr_pose_stats* out, void* stream) {
  if (k < 1) return failh(TDR_ERR_ARG, "batch_pose: k = %d, at least one filter is needed", k);
  if (!f || !out) return failh(TDR_ERR_ARG, "batch_pose: null %s array", !f ? "filter" : "output");
  for (int i = 0; i < k; i++)
    if (!f[i]) return failh(TDR_ERR_ARG, "batch_pose: filter %d is null", i);
  {
    std::vector<const tdr_filter*> seen(f, f + k);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return failh(TDR_ERR_ARG, "batch_pose: a filter appears twice in the batch");
  }
  for (int i = 0; i < k; i++)
    if (f[i]->map != f[0]->map) return failh(TDR_ERR_ARG, "batch_pose: filter %d is on another map than filter 0", i);
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> small, big;
  for (int i = 0; i < k; i++) {
    tdr_filter* g = f[i];
    tdr_pose_stats& o = out[i];
    o = tdr_pose_stats{};
    o.n = g->n;
    if (g->comm) {   // the all-gather inside is collective: the standalone calls
      TTRY(tdr_filter_mean_cov(g, 0, o.mean, o.cov));
      o.scale = tdr_filter_scale(g);
      continue;
    }
    if (g->n < 1) { o.scale = tdr_filter_scale(g); continue; }   // (zeros, no device work)
    (g->n <= TDR_BATCH_MC_SINGLE_MAX_N ? small : big).push_back(i);
  }
  const int ks = (int)small.size(), kb = (int)big.size(), kd = ks + kb;
  if (kd == 0) return TDR_OK;
  // staging: [kd] entries (small ones first), then the [kd] result records the kernels write and the copy brings back
  const size_t ent_bytes = align64(sizeof(TdrBatchPoseEntry) * (size_t)kd);
  const size_t res_bytes = sizeof(float) * TDR_BATCH_POSE_FLOATS * (size_t)kd;
  StageCtx& B = g_pose_stage;
  TTRY(B.reserve(ent_bytes + res_bytes, ent_bytes + res_bytes, s));
  // after every filter's last step, on whichever stream it ran (tdr_batch_step leaves the filters' streams after it)
  {
    std::vector<hipStream_t> streams;
    for (int i : small) streams.push_back(f[i]->stream);
    for (int i : big) streams.push_back(f[i]->stream);
    std::sort(streams.begin(), streams.end());
    streams.erase(std::unique(streams.begin(), streams.end()), streams.end());
    for (hipStream_t fs : streams) {
      if (fs == s) continue;
      hipEvent_t e = nullptr;
      HTRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      int rc = TDR_OK;
      if (hipEventRecord(e, fs) != hipSuccess || hipStreamWaitEvent(s, e, 0) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_pose: stream order");
      (void)hipEventDestroy(e);
      if (rc != TDR_OK) return rc;
    }
  }
  TdrBatchPoseEntry* tab = reinterpret_cast<TdrBatchPoseEntry*>(B.host);
  float* res_dev = reinterpret_cast<float*>(B.dev.p + ent_bytes);
  float* res_host = reinterpret_cast<float*>(B.host + ent_bytes);
  std::vector<int> order(small);
  order.insert(order.end(), big.begin(), big.end());
  for (int j = 0; j < kd; j++) {
    tdr_filter* g = f[order[j]];
    tab[j] = TdrBatchPoseEntry{g->st.p, g->cap, g->n, res_dev + (size_t)TDR_BATCH_POSE_FLOATS * j, g->stats.p + 24};
  }
  const TdrBatchPoseEntry* tab_dev = reinterpret_cast<const TdrBatchPoseEntry*>(B.dev.p);
  HTRY(hipMemcpyAsync(B.dev.p, B.host, ent_bytes, hipMemcpyHostToDevice, s));
  TTRY(tdr_batch_pose_launch(tab_dev, ks, tab_dev + ks, kb, s));
  HTRY(hipMemcpyAsync(res_host, res_dev, res_bytes, hipMemcpyDeviceToHost, s));
  HTRY(hipEventRecord(B.done, s));
  HTRY(hipEventRecord(B.uploaded, s));
  HTRY(hipEventSynchronize(B.done));   // the one wait of the call
  for (int j = 0; j < kd; j++) {
    tdr_filter* g = f[order[j]];
    const float* rec = res_host + (size_t)TDR_BATCH_POSE_FLOATS * j;
    tdr_pose_stats& o = out[order[j]];
    std::memcpy(g->mean_cov_host, rec, sizeof(g->mean_cov_host));   // the cache tdr_filter_mean_cov(f, 0, ...) reads
    g->mean_cov_valid = true;
    std::memcpy(o.mean, rec, sizeof(o.mean));
    std::memcpy(o.cov, rec + 4, sizeof(o.cov));
    if (g->fp.fixed_scale > 0) {           // tdr_filter_scale
      o.scale = g->fp.fixed_scale;
    } else if (g->scale_frozen) {
      o.scale = rec[24];
      g->scale_host = rec[24];
      g->scale_valid = true;
    } else {
      o.scale = -1.f;
    }
  }
  return TDR_OK;
}
}  // extern "C"

// ---- the pictures of a batched node loop: tdr_batch_scan_pictures, tdr_batch_visualize ------------------------------------
namespace {
thread_local StageCtx g_scan_pic_stage, g_viz_stage;

// `s` continues after everything queued on the filters' own streams (tdr_batch_step leaves them after the batch)
int order_after_filters(tdr_filter* const* f, const std::vector<int>& which, hipStream_t s, const char* who) {
  std::vector<hipStream_t> streams;
  for (int i : which) streams.push_back(f[i]->stream);
  std::sort(streams.begin(), streams.end());
  streams.erase(std::unique(streams.begin(), streams.end()), streams.end());
  for (hipStream_t fs : streams) {
    if (fs == s) continue;
    hipEvent_t e = nullptr;
    HTRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    int rc = TDR_OK;
    if (hipEventRecord(e, fs) != hipSuccess || hipStreamWaitEvent(s, e, 0) != hipSuccess) rc = failh(TDR_ERR_HIP, "%s: stream order", who);
    (void)hipEventDestroy(e);
    if (rc != TDR_OK) return rc;
  }
  return TDR_OK;
}
}  // namespace

extern "C" {
int tdr_batch_scan_pictures(const tdr_renderer* const* r, int k, const int32_t* unflatten, const uint8_t* lut_bgr,
                            uint8_t* out_bgr_host, void* stream) {
  if (k < 1) return failh(TDR_ERR_ARG, "batch_scan_pictures: k = %d, at least one renderer is needed", k);
  if (k > 65535) return failh(TDR_ERR_ARG, "batch_scan_pictures: k = %d, at most 65535 renderers", k);
  if (!r || !unflatten || !lut_bgr || !out_bgr_host) return failh(TDR_ERR_ARG, "batch_scan_pictures: null argument");
  for (int i = 0; i < k; i++)
    if (!r[i]) return failh(TDR_ERR_ARG, "batch_scan_pictures: renderer %d is null", i);
  {
    std::vector<const tdr_renderer*> seen(r, r + k);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return failh(TDR_ERR_ARG, "batch_scan_pictures: a renderer appears twice in the batch");
  }
  for (int i = 0; i < k; i++)
    if (!r[i]->have_scan) return failh(TDR_ERR_ARG, "batch_scan_pictures: renderer %d has no render", i);
  const int ncls = r[0]->ncls, rows = r[0]->rows, cols = r[0]->cols;
  for (int i = 1; i < k; i++)
    if (r[i]->ncls != ncls || r[i]->rows != rows || r[i]->cols != cols)
      return failh(TDR_ERR_ARG, "batch_scan_pictures: renderer %d holds a %dx%dx%d render, renderer 0 a %dx%dx%d one", i,
                   r[i]->ncls, r[i]->rows, r[i]->cols, ncls, rows, cols);
  if (ncls > TDR_MAX_CLASSES) return failh(TDR_ERR_ARG, "batch_scan_pictures: %d classes (at most %d)", ncls, TDR_MAX_CLASSES);
  hipStream_t s = (hipStream_t)stream;
  const size_t P = (size_t)rows * cols, pic = 3 * P;
  // staging: [k] jobs; on the device the k pictures follow, consecutive like the caller's array
  const size_t job_bytes = align64(sizeof(tdr_scan_picture_job) * (size_t)k);
  StageCtx& B = g_scan_pic_stage;
  TTRY(B.reserve(job_bytes, job_bytes + pic * k, s));
  tdr_scan_picture_job* tab = reinterpret_cast<tdr_scan_picture_job*>(B.host);
  uint8_t* out_dev = reinterpret_cast<uint8_t*>(B.dev.p + job_bytes);
  for (int i = 0; i < k; i++) {
    TTRY(renderer_wait_render(r[i], s));
    tab[i] = tdr_scan_picture_job{r[i]->img.p, ncls, 0, (int64_t)P, out_dev + pic * i};
  }
  HTRY(hipMemcpyAsync(B.dev.p, B.host, job_bytes, hipMemcpyHostToDevice, s));
  HTRY(hipEventRecord(B.uploaded, s));
  TTRY(tdr_k_scan_picture_jobs(reinterpret_cast<const tdr_scan_picture_job*>(B.dev.p), k, (int64_t)P, unflatten, ncls, lut_bgr, s));
  for (int i = 0; i < k; i++) TTRY(renderer_note_read(r[i], s));
  HTRY(hipMemcpyAsync(out_bgr_host, out_dev, pic * k, hipMemcpyDeviceToHost, s));
  HTRY(hipEventRecord(B.done, s));
  HTRY(hipEventSynchronize(B.done));   // the one wait of the call
  return TDR_OK;
}

int tdr_batch_visualize(tdr_filter* const* f, int k, float pub_scale, tdr_viz_request* req, void* stream) {
  if (k < 1) return failh(TDR_ERR_ARG, "batch_visualize: k = %d, at least one filter is needed", k);
  if (k > 65535) return failh(TDR_ERR_ARG, "batch_visualize: k = %d, at most 65535 filters", k);
  if (!f || !req) return failh(TDR_ERR_ARG, "batch_visualize: null %s array", !f ? "filter" : "request");
  for (int i = 0; i < k; i++)
    if (!f[i]) return failh(TDR_ERR_ARG, "batch_visualize: filter %d is null", i);
  {
    std::vector<const tdr_filter*> seen(f, f + k);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return failh(TDR_ERR_ARG, "batch_visualize: a filter appears twice in the batch");
  }
  std::vector<int> oh((size_t)k), ow((size_t)k);
  for (int i = 0; i < k; i++) {
    const tdr_filter* g = f[i];
    const tdr_viz_request& q = req[i];
    if (g->comm) return failh(TDR_ERR_ARG, "batch_visualize: filter %d is sharded and has no picture (draw from a one-GPU filter)", i);
    if (g->viz_h < 1) return failh(TDR_ERR_ARG, "batch_visualize: filter %d has no background (tdr_filter_set_viz_background)", i);
    if (q.m < 0 || (q.m > 0 && !q.extra_arrows) || q.m > (1 << 20))
      return failh(TDR_ERR_ARG, "batch_visualize: request %d: bad arrows", i);
    oh[i] = viz_pub_dim(g->viz_h, pub_scale);
    ow[i] = viz_pub_dim(g->viz_w, pub_scale);
    if (oh[i] < 1 || ow[i] < 1 || oh[i] > 32768 || ow[i] > 32768)
      return failh(TDR_ERR_ARG, "batch_visualize: filter %d: scale %g publishes %d x %d pixels (1 .. 32768 a side)", i,
                   (double)pub_scale, oh[i], ow[i]);
    const size_t bytes = (size_t)3 * oh[i] * ow[i];
    if (q.out_bgr_host && (q.capacity < 0 || (size_t)q.capacity < bytes))
      return failh(TDR_ERR_ARG, "batch_visualize: request %d: the image needs %zu bytes, room for %lld", i, bytes,
                   (long long)q.capacity);
  }
  // layers 4 (without the max-likelihood arrow, which the segments launch adds from the device state) and 5 on the host
  std::vector<int> drawn;
  std::vector<std::vector<int32_t>> segs((size_t)k);
  std::vector<int> nseg((size_t)k, 0);
  for (int i = 0; i < k; i++) {
    if (!req[i].out_bgr_host) continue;
    const tdr_filter* g = f[i];
    const int kk = (int)(g->gmm_means.size() / 3), cap = TDR_VIZ_MAX_SEGS(kk, req[i].m);
    segs[i].resize((size_t)5 * cap);
    TTRY(tdr_viz_overlay_host(g->gmm_means.data(), g->gmm_covs.data(), kk, nullptr, req[i].extra_arrows, req[i].m, g->viz_h,
                              segs[i].data(), cap, &nseg[i]));
    drawn.push_back(i);
  }
  for (int i = 0; i < k; i++) {
    req[i].out_h = oh[i];
    req[i].out_w = ow[i];
  }
  const int kd = (int)drawn.size();
  if (kd == 0) return TDR_OK;
  hipStream_t s = (hipStream_t)stream;
  // staging, host and device alike: [kd] jobs, every filter's segments; on the device every picture and the planes follow
  const size_t job_bytes = align64(sizeof(tdr_viz_job) * (size_t)kd);
  std::vector<size_t> seg_off((size_t)kd), out_off((size_t)kd), pl_off((size_t)kd);
  size_t up_bytes = job_bytes;
  for (int j = 0; j < kd; j++) {
    seg_off[j] = up_bytes;
    up_bytes += align64((size_t)5 * nseg[drawn[j]] * sizeof(int32_t));
  }
  size_t pic_end = up_bytes;
  for (int j = 0; j < kd; j++) {
    out_off[j] = pic_end;
    pic_end += align64((size_t)3 * oh[drawn[j]] * ow[drawn[j]]);
  }
  size_t dev_bytes = pic_end;
  for (int j = 0; j < kd; j++) {
    pl_off[j] = dev_bytes;
    dev_bytes += align64(4 * tdr_viz_plane_words(f[drawn[j]]->viz_h, f[drawn[j]]->viz_w) * sizeof(uint32_t));
  }
  StageCtx& B = g_viz_stage;
  TTRY(B.reserve(up_bytes, dev_bytes, s));
  TTRY(order_after_filters(f, drawn, s, "batch_visualize"));
  tdr_viz_job* tab = reinterpret_cast<tdr_viz_job*>(B.host);
  int64_t max_n = 0, max_out = 0;
  int max_segs = 0;
  for (int j = 0; j < kd; j++) {
    const int i = drawn[j];
    const tdr_filter* g = f[i];
    if (nseg[i]) std::memcpy(B.host + seg_off[j], segs[i].data(), (size_t)5 * nseg[i] * sizeof(int32_t));
    tdr_viz_job& e = tab[j];
    e = tdr_viz_job{};
    e.st = g->st.p;
    e.cap = g->cap;
    e.n = g->n;
    e.H = g->viz_h;
    e.W = g->viz_w;
    e.planes = reinterpret_cast<uint32_t*>(B.dev.p + pl_off[j]);
    e.background = g->viz_bg.p;
    e.segs = reinterpret_cast<const int32_t*>(B.dev.p + seg_off[j]);
    e.best = g->have_ml ? g->ml_dev.p + 8 : nullptr;
    e.n_segs = nseg[i];
    e.out_h = oh[i];
    e.out_w = ow[i];
    e.out = reinterpret_cast<uint8_t*>(B.dev.p + out_off[j]);
    max_n = std::max(max_n, g->n);
    max_segs = std::max(max_segs, nseg[i]);
    max_out = std::max(max_out, (int64_t)oh[i] * ow[i]);
  }
  const tdr_viz_job* tab_dev = reinterpret_cast<const tdr_viz_job*>(B.dev.p);
  HTRY(hipMemcpyAsync(B.dev.p, B.host, up_bytes, hipMemcpyHostToDevice, s));
  HTRY(hipEventRecord(B.uploaded, s));
  HTRY(hipMemsetAsync(B.dev.p + pic_end, 0, dev_bytes - pic_end, s));
  TTRY(tdr_k_viz_particles_jobs(tab_dev, kd, max_n, s));
  TTRY(tdr_k_viz_segments_jobs(tab_dev, kd, max_segs, s));
  TTRY(tdr_k_viz_compose_jobs(tab_dev, kd, max_out, s));
  // every picture straight into its request's image: a second copy on the host (one read-back into pinned staging, then
  // k memcpys) costs more than the launches and waits the batch saves
  for (int j = 0; j < kd; j++) {
    const int i = drawn[j];
    HTRY(hipMemcpyAsync(req[i].out_bgr_host, B.dev.p + out_off[j], (size_t)3 * oh[i] * ow[i], hipMemcpyDeviceToHost, s));
  }
  HTRY(hipEventRecord(B.done, s));
  HTRY(hipEventSynchronize(B.done));   // the one wait of the call
  return TDR_OK;
}

// the fleet picture (include/tdr.h): k robots on one map in one image over the map's background
int tdr_batch_visualize_fleet(tdr_filter* const* f, int k, float pub_scale, const uint8_t* palette,
                              const int32_t* extra_arrows, int m, uint8_t* out_bgr_host, int64_t capacity, int* out_h,
                              int* out_w, void* stream) {
  if (k < 1 || k > TDR_FLEET_MAX) return failh(TDR_ERR_ARG, "batch_visualize_fleet: k = %d (1 .. %d filters)", k, TDR_FLEET_MAX);
  if (!f) return failh(TDR_ERR_ARG, "batch_visualize_fleet: null filter array");
  if (!out_h || !out_w) return failh(TDR_ERR_ARG, "batch_visualize_fleet: null size pointers");
  for (int i = 0; i < k; i++)
    if (!f[i]) return failh(TDR_ERR_ARG, "batch_visualize_fleet: filter %d is null", i);
  {
    std::vector<const tdr_filter*> seen(f, f + k);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return failh(TDR_ERR_ARG, "batch_visualize_fleet: a filter appears twice in the fleet");
  }
  for (int i = 0; i < k; i++) {
    if (f[i]->comm) return failh(TDR_ERR_ARG, "batch_visualize_fleet: filter %d is sharded and has no picture (draw from a one-GPU filter)", i);
    if (f[i]->map != f[0]->map) return failh(TDR_ERR_ARG, "batch_visualize_fleet: filter %d is on another map than filter 0", i);
  }
  const tdr_map* map = f[0]->map;
  if (!map || map->viz_h < 1) return failh(TDR_ERR_ARG, "batch_visualize_fleet: the map has no background (tdr_map_set_viz_background)");
  if (!palette) return failh(TDR_ERR_ARG, "batch_visualize_fleet: null palette");
  if (m < 0 || (m > 0 && !extra_arrows) || m > (1 << 20)) return failh(TDR_ERR_ARG, "batch_visualize_fleet: bad arrows");
  const int H = map->viz_h, W = map->viz_w;
  const int oh = viz_pub_dim(H, pub_scale), ow = viz_pub_dim(W, pub_scale);
  if (oh < 1 || ow < 1 || oh > 32768 || ow > 32768)
    return failh(TDR_ERR_ARG, "batch_visualize_fleet: scale %g publishes %d x %d pixels (1 .. 32768 a side)", (double)pub_scale, oh, ow);
  const size_t bytes = (size_t)3 * oh * ow;
  if (out_bgr_host && (capacity < 0 || (size_t)capacity < bytes))
    return failh(TDR_ERR_ARG, "batch_visualize_fleet: the image needs %zu bytes, room for %lld", bytes, (long long)capacity);
  // every robot's estimate (without the max-likelihood arrow, which the segments launch adds from the device state) on
  // the host; the caller's arrows go into the last robot's list: its plane 3 is the image's green plane (below)
  std::vector<std::vector<int32_t>> segs((size_t)k);
  std::vector<int> nseg((size_t)k, 0);
  if (out_bgr_host)
    for (int i = 0; i < k; i++) {
      const tdr_filter* g = f[i];
      const int mi = i == k - 1 ? m : 0;
      const int kk = (int)(g->gmm_means.size() / 3), cap = TDR_VIZ_MAX_SEGS(kk, mi);
      segs[i].resize((size_t)5 * cap);
      TTRY(tdr_viz_overlay_host(g->gmm_means.data(), g->gmm_covs.data(), kk, nullptr, extra_arrows, mi, H, segs[i].data(),
                                cap, &nseg[i]));
    }
  *out_h = oh;
  *out_w = ow;
  if (!out_bgr_host) return TDR_OK;
  hipStream_t s = (hipStream_t)stream;
  // staging, host and device alike: [k] jobs, every robot's segments; on the device the picture and the planes follow:
  // robot i's planes 0 - 2 at 3 i plane sizes, the green plane behind the last robot's
  const size_t job_bytes = align64(sizeof(tdr_viz_job) * (size_t)k);
  std::vector<size_t> seg_off((size_t)k);
  size_t up_bytes = job_bytes;
  for (int i = 0; i < k; i++) {
    seg_off[i] = up_bytes;
    up_bytes += align64((size_t)5 * nseg[i] * sizeof(int32_t));
  }
  const size_t pic_end = up_bytes + align64(bytes);
  const size_t pw = tdr_viz_plane_words(H, W);
  const size_t dev_bytes = pic_end + ((size_t)3 * k + 1) * pw * sizeof(uint32_t);
  StageCtx& B = g_viz_stage;
  TTRY(B.reserve(up_bytes, dev_bytes, s));
  std::vector<int> all((size_t)k);
  for (int i = 0; i < k; i++) all[i] = i;
  TTRY(order_after_filters(f, all, s, "batch_visualize_fleet"));
  tdr_viz_job* tab = reinterpret_cast<tdr_viz_job*>(B.host);
  uint32_t* planes = reinterpret_cast<uint32_t*>(B.dev.p + pic_end);
  uint8_t* out_dev = reinterpret_cast<uint8_t*>(B.dev.p + up_bytes);
  int64_t max_n = 0;
  int max_segs = 0;
  for (int i = 0; i < k; i++) {
    const tdr_filter* g = f[i];
    if (nseg[i]) std::memcpy(B.host + seg_off[i], segs[i].data(), (size_t)5 * nseg[i] * sizeof(int32_t));
    tdr_viz_job& e = tab[i];
    e = tdr_viz_job{};
    e.st = g->st.p;
    e.cap = g->cap;
    e.n = g->n;
    e.H = H;
    e.W = W;
    e.planes = planes + (size_t)3 * i * pw;
    e.background = map->viz_bg.p;
    e.segs = reinterpret_cast<const int32_t*>(B.dev.p + seg_off[i]);
    e.best = g->have_ml ? g->ml_dev.p + 8 : nullptr;
    e.n_segs = nseg[i];
    e.out_h = oh;
    e.out_w = ow;
    e.out = out_dev;
    max_n = std::max(max_n, g->n);
    max_segs = std::max(max_segs, nseg[i]);
  }
  const tdr_viz_job* tab_dev = reinterpret_cast<const tdr_viz_job*>(B.dev.p);
  HTRY(hipMemcpyAsync(B.dev.p, B.host, up_bytes, hipMemcpyHostToDevice, s));
  HTRY(hipEventRecord(B.uploaded, s));
  HTRY(hipMemsetAsync(planes, 0, dev_bytes - pic_end, s));
  TTRY(tdr_k_viz_particles_jobs(tab_dev, k, max_n, s));
  TTRY(tdr_k_viz_segments_jobs(tab_dev, k, max_segs, s));
  TTRY(tdr_k_viz_compose_fleet(tab_dev, k, palette, map->viz_bg.p, H, W, planes + (size_t)3 * k * pw, oh, ow, out_dev, s));
  HTRY(hipMemcpyAsync(out_bgr_host, out_dev, bytes, hipMemcpyDeviceToHost, s));
  HTRY(hipEventRecord(B.done, s));
  HTRY(hipEventSynchronize(B.done));   // the one wait of the call
  return TDR_OK;
}
}  // extern "C"
