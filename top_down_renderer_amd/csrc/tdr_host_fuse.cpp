// tdr_host_fuse.cpp — the map fuser behind tdr_fuser_* (include/tdr.h, "map fusion"; kernels in tdr_fuse.hip): the vote
// planes and the dirty bitmap of one map, the adds from renderers or host images, the label pass and its hand-over to the
// incremental map update (tdr_map_patch_labels / tdr_filter_patch_map_labels).  Everything runs on the null stream.
#include "tdr_host.h"

struct tdr_fuser {
  tdr_map* map = nullptr;
  int ncls = 0, rows = 0, cols = 0, img_h = 0, img_w = 0, center_x = 0, center_y = 0;
  float resolution = 0.f;
  uint8_t class_label[TDR_MAX_CLASSES] = {0};
  uint32_t min_votes = 0, share_num = 0, share_den = 0;
  DevBuf<uint32_t> votes, dirty;
  DevBuf<uint8_t> base, current;
  DevBuf<int32_t> tiles, out5;
  DevBuf<uint64_t> counters;
  DevBuf<tdr_fuse_job> jobs;
  DevBuf<float> img;            // staging of tdr_fuser_add_images
  std::vector<uint32_t> dirty_host;
  std::vector<int32_t> tiles_host;
  std::vector<uint8_t> patch;
  uint64_t scans = 0, added = 0, dropped = 0, applies = 0;
  int n_tiles() const { return tdr_map_incr_tiles(rows, cols); }
  size_t dirty_words() const { return ((size_t)n_tiles() + 31) / 32; }
};

// the map still is the one the fuser's planes describe
static int fuser_map_matches(const tdr_fuser* f, const char* who) {
  const tdr_map* m = f->map;
  if (!m->inc_valid) return failh(TDR_ERR_ARG, "%s: the map was not last set from a label image (tdr_fuser_rebase after the next one)", who);
  if (m->desc.ncls != f->ncls || m->desc.rows != f->rows || m->desc.cols != f->cols || m->desc.resolution != f->resolution ||
      m->inc_img_h != f->img_h || m->inc_img_w != f->img_w)
    return failh(TDR_ERR_ARG, "%s: the map changed shape since the fuser was created (tdr_fuser_rebase)", who);
  return TDR_OK;
}

static int fuser_check_labels(const tdr_map* m, const uint8_t* class_label, int ncls, const char* who) {
  for (int c = 0; c < ncls; c++) {
    const int l = class_label[c];
    if (l >= (int)m->inc_lut.size() || m->inc_lut[(size_t)l] != c)
      return failh(TDR_ERR_ARG, "%s: class_label[%d] = %d, which the map's flatten_lut does not send to class %d", who, c, l, c);
  }
  return TDR_OK;
}

// planes, bitmap and images for the map as it is now; the votes are zeroed
static int fuser_take_map(tdr_fuser* f) {
  const tdr_map* m = f->map;
  f->ncls = m->desc.ncls; f->rows = m->desc.rows; f->cols = m->desc.cols; f->resolution = m->desc.resolution;
  f->img_h = m->inc_img_h; f->img_w = m->inc_img_w; f->center_x = m->center_x; f->center_y = m->center_y;
  const size_t nv = (size_t)f->ncls * f->rows * f->cols, npix = (size_t)f->img_h * f->img_w;
  TTRY(f->votes.resize(nv));
  TTRY(f->dirty.resize(f->dirty_words()));
  TTRY(f->base.resize(npix));
  TTRY(f->current.resize(npix));
  TTRY(f->tiles.resize((size_t)f->n_tiles()));
  TTRY(f->out5.resize(5));
  TTRY(f->counters.resize(2));
  HTRY(hipMemset(f->votes.p, 0, nv * sizeof(uint32_t)));
  HTRY(hipMemset(f->dirty.p, 0, f->dirty_words() * sizeof(uint32_t)));
  HTRY(hipMemcpy(f->base.p, m->ing_img.p, npix, hipMemcpyDeviceToDevice));
  HTRY(hipMemcpy(f->current.p, m->ing_img.p, npix, hipMemcpyDeviceToDevice));
  return TDR_OK;
}

static bool pose_ok(float cx, float cy, float theta, float scale, float res) {
  return std::isfinite(cx) && std::isfinite(cy) && std::isfinite(theta) && std::isfinite(scale) && std::isfinite(res) &&
         scale > 0.f && res > 0.f;
}

// a scan of this kind and shape can vote on the fuser's map
static int fuser_check_scan(const tdr_fuser* f, int polar, int ncls, int rows, int cols, const char* who) {
  if (ncls != f->ncls) return failh(TDR_ERR_ARG, "%s: a render of %d classes on a map of %d", who, ncls, f->ncls);
  if (rows < 1 || cols < 1) return failh(TDR_ERR_ARG, "%s: bad render shape", who);
  if (polar && (f->map->nb < 1 || !f->map->tab.p || rows != f->map->nb || cols != f->map->nr))
    return failh(TDR_ERR_ARG, "%s: a polar render of %d x %d bins, the map's table has %d x %d", who, rows, cols, f->map->nb,
                 f->map->nr);
  return TDR_OK;
}

// the jobs (already checked) in one launch; this call's counters
static int fuser_vote(tdr_fuser* f, const std::vector<tdr_fuse_job>& jobs, uint64_t* votes_added, uint64_t* votes_dropped) {
  const int k = (int)jobs.size();
  int64_t max_bins = 1;
  for (const tdr_fuse_job& j : jobs) max_bins = std::max(max_bins, (int64_t)j.rows * j.cols);
  TTRY(f->jobs.resize((size_t)k));
  HTRY(hipMemcpy(f->jobs.p, jobs.data(), (size_t)k * sizeof(tdr_fuse_job), hipMemcpyHostToDevice));
  HTRY(hipMemsetAsync(f->counters.p, 0, 2 * sizeof(uint64_t), nullptr));
  const tdr_map* m = f->map;
  const bool tab = m->nb > 0 && m->tab.p;
  TTRY(tdr_k_fuse_votes_jobs(&m->desc, tab ? m->tab.p : nullptr, tab ? m->nb : 0, tab ? m->nr : 0, f->jobs.p, k, max_bins,
                             f->votes.p, f->dirty.p, f->counters.p, nullptr));
  uint64_t c[2] = {0, 0};
  HTRY(hipMemcpy(c, f->counters.p, sizeof(c), hipMemcpyDeviceToHost));
  f->scans += (uint64_t)k;
  f->added += c[0];
  f->dropped += c[1];
  if (votes_added) *votes_added = c[0];
  if (votes_dropped) *votes_dropped = c[1];
  return TDR_OK;
}

extern "C" {

int tdr_fuser_create(tdr_map* m, const uint8_t* class_label, uint32_t min_votes, uint32_t share_num, uint32_t share_den,
                     tdr_fuser** out) {
  if (!m || !class_label || !out) return failh(TDR_ERR_ARG, "fuser_create: null pointer");
  if (!m->inc_valid) return failh(TDR_ERR_ARG, "fuser_create: the map was not last set from a label image (tdr_map_set_labels)");
  if (!(m->desc.resolution >= 1.f))
    return failh(TDR_ERR_ARG, "fuser_create: map resolution %g (cells map to image pixels one to one from 1 on)", (double)m->desc.resolution);
  if (min_votes == 0) return failh(TDR_ERR_ARG, "fuser_create: min_votes must be at least 1");
  if (share_den == 0 || share_den > (1u << 24) || share_num > share_den)
    return failh(TDR_ERR_ARG, "fuser_create: share %u / %u (0 <= num <= den, 1 <= den <= 2^24)", share_num, share_den);
  TTRY(fuser_check_labels(m, class_label, m->desc.ncls, "fuser_create"));
  tdr_fuser* f = new tdr_fuser();
  f->map = m;
  std::memcpy(f->class_label, class_label, (size_t)m->desc.ncls);
  f->min_votes = min_votes; f->share_num = share_num; f->share_den = share_den;
  const int rc = fuser_take_map(f);
  if (rc != TDR_OK) {
    delete f;
    return rc;
  }
  *out = f;
  return TDR_OK;
}
void tdr_fuser_destroy(tdr_fuser* f) { delete f; }

int tdr_fuser_add_batch(tdr_fuser* f, const tdr_renderer* const* r, int k, const float* poses, uint64_t* votes_added,
                        uint64_t* votes_dropped) {
  if (!f || !r || !poses) return failh(TDR_ERR_ARG, "fuser_add: null pointer");
  if (k < 1 || k > 65535) return failh(TDR_ERR_ARG, "fuser_add: %d renders (1 .. 65535)", k);
  TTRY(fuser_map_matches(f, "fuser_add"));
  std::vector<tdr_fuse_job> jobs((size_t)k);
  for (int i = 0; i < k; i++) {
    const tdr_renderer* ri = r[i];
    if (!ri) return failh(TDR_ERR_ARG, "fuser_add: renderer %d is null", i);
    if (!ri->have_scan) return failh(TDR_ERR_ARG, "fuser_add: renderer %d has no render", i);
    for (int j = 0; j < i; j++)
      if (r[j] == ri) return failh(TDR_ERR_ARG, "fuser_add: renderer %d is listed twice", i);
    TTRY(fuser_check_scan(f, ri->polar, ri->ncls, ri->rows, ri->cols, "fuser_add"));
    const float* p = poses + (size_t)5 * i;
    if (!pose_ok(p[0], p[1], p[2], p[3], p[4]))
      return failh(TDR_ERR_ARG, "fuser_add: pose %d is not finite, or scale / res is not > 0", i);
    tdr_fuse_job& j = jobs[(size_t)i];
    j = tdr_fuse_job{};
    j.scan = ri->img.p; j.rows = ri->rows; j.cols = ri->cols; j.polar = ri->polar ? 1 : 0;
    j.cx = p[0]; j.cy = p[1]; j.theta = p[2]; j.scale = p[3]; j.res = p[4];
  }
  for (int i = 0; i < k; i++) TTRY(renderer_wait_render(r[i], nullptr));
  TTRY(fuser_vote(f, jobs, votes_added, votes_dropped));
  for (int i = 0; i < k; i++) TTRY(renderer_note_read(r[i], nullptr));
  return TDR_OK;
}

int tdr_fuser_add(tdr_fuser* f, const tdr_renderer* r, float cx, float cy, float theta, float scale, float res,
                  uint64_t* votes_added, uint64_t* votes_dropped) {
  const float pose[5] = {cx, cy, theta, scale, res};
  return tdr_fuser_add_batch(f, &r, 1, pose, votes_added, votes_dropped);
}

int tdr_fuser_add_images(tdr_fuser* f, const float* imgs_host, int polar, int rows, int cols, float cx, float cy,
                         float theta, float scale, float res, uint64_t* votes_added, uint64_t* votes_dropped) {
  if (!f || !imgs_host) return failh(TDR_ERR_ARG, "fuser_add_images: null pointer");
  TTRY(fuser_map_matches(f, "fuser_add_images"));
  TTRY(fuser_check_scan(f, polar, f->ncls, rows, cols, "fuser_add_images"));
  if (!pose_ok(cx, cy, theta, scale, res))
    return failh(TDR_ERR_ARG, "fuser_add_images: the pose is not finite, or scale / res is not > 0");
  const size_t n = (size_t)f->ncls * rows * cols;
  TTRY(f->img.resize(n));
  HTRY(hipMemcpy(f->img.p, imgs_host, n * sizeof(float), hipMemcpyHostToDevice));
  std::vector<tdr_fuse_job> jobs(1);
  jobs[0] = tdr_fuse_job{};
  jobs[0].scan = f->img.p; jobs[0].rows = rows; jobs[0].cols = cols; jobs[0].polar = polar ? 1 : 0;
  jobs[0].cx = cx; jobs[0].cy = cy; jobs[0].theta = theta; jobs[0].scale = scale; jobs[0].res = res;
  return fuser_vote(f, jobs, votes_added, votes_dropped);
}

int tdr_fuser_apply(tdr_fuser* f, tdr_filter* const* filters, int k, int64_t* changed_cells) {
  if (!f || !changed_cells || k < 0 || (k > 0 && !filters)) return failh(TDR_ERR_ARG, "fuser_apply: bad arguments");
  for (int i = 0; i < k; i++)
    if (!filters[i] || filters[i]->map != f->map) return failh(TDR_ERR_ARG, "fuser_apply: filter %d is null or on another map", i);
  TTRY(fuser_map_matches(f, "fuser_apply"));
  *changed_cells = 0;
  const size_t words = f->dirty_words();
  f->dirty_host.resize(words);
  HTRY(hipMemcpy(f->dirty_host.data(), f->dirty.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  f->tiles_host.clear();
  for (int t = 0; t < f->n_tiles(); t++)
    if (f->dirty_host[(size_t)t >> 5] >> (t & 31) & 1u) f->tiles_host.push_back(t);
  if (f->tiles_host.empty()) return TDR_OK;
  const int nt = (int)f->tiles_host.size();
  const int32_t init[5] = {0, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::max(), -1, -1};
  HTRY(hipMemcpy(f->tiles.p, f->tiles_host.data(), (size_t)nt * sizeof(int32_t), hipMemcpyHostToDevice));
  HTRY(hipMemcpy(f->out5.p, init, sizeof(init), hipMemcpyHostToDevice));
  TTRY(tdr_k_fuse_labels(f->votes.p, f->ncls, f->rows, f->cols, f->img_h, f->img_w, f->resolution, f->class_label,
                         f->min_votes, f->share_num, f->share_den, f->base.p, f->current.p, f->tiles.p, nt, f->out5.p, nullptr));
  HTRY(hipMemsetAsync(f->dirty.p, 0, words * sizeof(uint32_t), nullptr));
  int32_t o[5];
  HTRY(hipMemcpy(o, f->out5.p, sizeof(o), hipMemcpyDeviceToHost));
  if (o[0] == 0) return TDR_OK;
  const int y0 = o[1], x0 = o[2], h = o[3] - o[1] + 1, w = o[4] - o[2] + 1;
  f->patch.resize((size_t)h * w);
  HTRY(hipMemcpy2D(f->patch.data(), (size_t)w, f->current.p + (size_t)y0 * f->img_w + x0, (size_t)f->img_w, (size_t)w,
                   (size_t)h, hipMemcpyDeviceToHost));
  // (tdr_map_patch_labels takes a rectangle of any size: it never falls back to the full path and never refuses one that
  // lies inside the image)
  TTRY(tdr_map_patch_labels(f->map, f->patch.data(), y0, x0, h, w, f->map->center_x, f->map->center_y, changed_cells));
  for (int i = 0; i < k; i++) {
    int64_t again = 0;   // 0: the map already holds the rectangle
    TTRY(tdr_filter_patch_map_labels(filters[i], f->patch.data(), y0, x0, h, w, f->map->center_x, f->map->center_y, &again));
  }
  f->applies++;
  return TDR_OK;
}

int tdr_fuser_decay(tdr_fuser* f, int shift) {
  if (!f || shift < 0) return failh(TDR_ERR_ARG, "fuser_decay: bad arguments");
  TTRY(tdr_k_fuse_decay(f->votes.p, f->ncls, f->rows, f->cols, shift, f->dirty.p, nullptr));
  HTRY(hipStreamSynchronize(nullptr));
  return TDR_OK;
}
int tdr_fuser_reset(tdr_fuser* f) {
  if (!f) return failh(TDR_ERR_ARG, "fuser_reset: null fuser");
  return tdr_fuser_decay(f, 32);
}

int tdr_fuser_rebase(tdr_fuser* f, int* kept) {
  if (!f || !kept) return failh(TDR_ERR_ARG, "fuser_rebase: null pointer");
  const tdr_map* m = f->map;
  if (!m->inc_valid) return failh(TDR_ERR_ARG, "fuser_rebase: the map was not last set from a label image");
  if (!(m->desc.resolution >= 1.f)) return failh(TDR_ERR_ARG, "fuser_rebase: map resolution %g is below 1", (double)m->desc.resolution);
  if (m->desc.ncls != f->ncls) {   // the class -> label table is the fuser's: it has no meaning for another class count
    return failh(TDR_ERR_ARG, "fuser_rebase: the map now has %d classes, the fuser's table %d (create a new fuser)", m->desc.ncls, f->ncls);
  }
  TTRY(fuser_check_labels(m, f->class_label, f->ncls, "fuser_rebase"));
  const bool same = m->desc.rows == f->rows && m->desc.cols == f->cols && m->desc.resolution == f->resolution &&
                    m->inc_img_h == f->img_h && m->inc_img_w == f->img_w && m->center_x == f->center_x && m->center_y == f->center_y;
  if (!same) {
    TTRY(fuser_take_map(f));
    *kept = 0;
    return TDR_OK;
  }
  // same grid: the votes stay, the new image is base and current, and every tile is looked at again by the next apply
  const size_t npix = (size_t)f->img_h * f->img_w;
  HTRY(hipMemcpy(f->base.p, m->ing_img.p, npix, hipMemcpyDeviceToDevice));
  HTRY(hipMemcpy(f->current.p, m->ing_img.p, npix, hipMemcpyDeviceToDevice));
  HTRY(hipMemset(f->dirty.p, 0xFF, f->dirty_words() * sizeof(uint32_t)));
  *kept = 1;
  return TDR_OK;
}

int tdr_fuser_get_votes(const tdr_fuser* f, uint32_t* votes_out) {
  if (!f || !votes_out) return failh(TDR_ERR_ARG, "fuser_get_votes: null pointer");
  HTRY(hipMemcpy(votes_out, f->votes.p, (size_t)f->ncls * f->rows * f->cols * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return TDR_OK;
}
int tdr_fuser_get_labels(const tdr_fuser* f, uint8_t* labels_out) {
  if (!f || !labels_out) return failh(TDR_ERR_ARG, "fuser_get_labels: null pointer");
  HTRY(hipMemcpy(labels_out, f->current.p, (size_t)f->img_h * f->img_w, hipMemcpyDeviceToHost));
  return TDR_OK;
}
int tdr_fuser_stats(const tdr_fuser* f, uint64_t* out9) {
  if (!f || !out9) return failh(TDR_ERR_ARG, "fuser_stats: null pointer");
  out9[0] = f->scans; out9[1] = f->added; out9[2] = f->dropped; out9[3] = f->applies;
  out9[4] = (uint64_t)f->ncls; out9[5] = (uint64_t)f->rows; out9[6] = (uint64_t)f->cols;
  out9[7] = (uint64_t)f->img_h; out9[8] = (uint64_t)f->img_w;
  return TDR_OK;
}

}  // extern "C"
