/* tdr.h — C ABI of libtdr_hip.so: the MI355X (gfx950) implementation of top_down_renderer's per-scan
 * particle-filter update (scan raster -> per-particle map gather + class-wise score -> weight statistics ->
 * systematic resample, plus propagate).
 *
 * The reference (KumarRobotics/top_down_renderer) has no FFI layer: its boundary is the public C++ surface of
 * library target `top_down_render` (CMakeLists.txt:145-165).  Every entry point below names the reference method
 * (file:line, relative to the reference root) whose work it performs; the headers under include/top_down_render/ rebuild the
 * reference's class names on top of these calls.
 *
 * Conventions
 *  - plain C, no torch / Eigen / PCL types; every function returns an int status (TDR_OK == 0), never throws;
 *  - "tdr_k_*" entry points are stateless launchers: every pointer is a DEVICE pointer unless the name says
 *    `_host`, `stream` is a hipStream_t (NULL = default stream), nothing is allocated, nothing synchronises, and no
 *    state is kept between calls.  What a launcher may be GIVEN is an object the caller owns (tdr_score_ctx: the tuner of
 *    the polar launch; tdr_rng_pipe: the generator's state and what it drew ahead, with a stream of its own).  Load-time entry points (tdr_k_compact_map,
 *    tdr_k_map_from_*) say so where they synchronise.  The tdr_config_* calls and the TDR_* environment variables they
 *    mirror are PROCESS-WIDE switches for A/B measurements and tests (set them before the first launch, not while
 *    another thread launches); results never depend on them unless a comment says so;
 *  - images follow the reference's Eigen::ArrayXXf layout: column-major float32, element (i,j) at i + rows*j,
 *    one image per class, images of one scan contiguous: [ncls][rows*cols];
 *  - particle state on the device is a structure of arrays `float st[TDR_ST_FIELDS][cap]` (plane stride `cap`),
 *    planes in the field order of the reference's `State` (include/top_down_render/state_particle.h:9-17),
 *    have_init stored as 0.0f / 1.0f;
 *  - no CPU fallback exists: without a HIP device every launcher fails with TDR_ERR_HIP.
 */
#ifndef TDR_H_
#define TDR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDR_OK 0
#define TDR_ERR_ARG (-1)      /* bad shape / null pointer / unsupported size (message in tdr_last_error) */
#define TDR_ERR_HIP (-2)      /* HIP runtime error (message in tdr_last_error) */
#define TDR_ERR_NOMEM (-3)

#define TDR_MAX_CLASSES 15
#define TDR_ST_FIELDS 7       /* init_x_px, init_y_px, dx_m, dy_m, theta, scale, have_init */
enum { TDR_ST_INIT_X = 0, TDR_ST_INIT_Y = 1, TDR_ST_DX = 2, TDR_ST_DY = 3, TDR_ST_THETA = 4, TDR_ST_SCALE = 5,
       TDR_ST_HAVE_INIT = 6 };

/* Same bytes as the reference's `State` (state_particle.h:9-17): 6 floats + bool, sizeof == 28. */
typedef struct tdr_state {
  float init_x_px, init_y_px, dx_m, dy_m, theta, scale;
  uint8_t have_init;
  uint8_t pad_[3];
} tdr_state;

/* POD mirror of the reference's `FilterParams` (state_particle.h:19-38). */
typedef struct tdr_filter_params {
  float pos_cov, theta_cov, regularization;
  float init_pos_px_x, init_pos_px_y, init_pos_px_cov;
  float init_pos_m_x, init_pos_m_y, init_pos_deg_theta, init_pos_deg_cov;
  int32_t force_on_map;
  float fixed_scale, scale_log_min, scale_log_max;
  int32_t num_classes;
  float class_weights[16];
} tdr_filter_params;

/* Geometry of the device-resident map produced by tdr_k_pack_map. */
typedef struct tdr_map_desc {
  const float* rec;     /* [(rows+2)*(cols+2)][rec_floats], row-major over the map plus a one-cell guard ring of zero
                           records; per cell {dist_0..dist_{ncls-1}, 0.., [known,] known} (see tdr_k_pack_map) */
  int32_t ncls, rows, cols, rec_floats;   /* rec_floats = 4*ceil((ncls+1)/4) */
  float resolution;     /* TopDownMap::Params::resolution (top_down_map.h:61) */
  /* Optional compact form of the same records (tdr_k_compact_map; cwords == 0: absent).  A cell is cwords dwords of
   * 10-bit indices into `dict` (three per dword, class k in dword k/3 at bit 2 + 10*(k%3)), `known` in bit 0 of every
   * dword; records are tiled 32/(4*cwords) rows x 4 columns per 128-byte line, row-major inside a tile, the tiles column
   * by column over the map (csrc/tdr_cmap.hip); the map's known mask follows the tiles (tdr_cmap_words_total).  Decoding reproduces `rec` bit for bit;
   * the scoring kernels read it instead of `rec` whenever it is present (tdr_config_compact(0) forces `rec`).
   * The WIDE form (tdr_k_compact_map_wide: rec_floats == 8, cwords == 4, dict_n > TDR_CMAP_MAX_DICT) holds 16-bit
   * indices, two per dword (class k in dword k/2 at bit 2 + 16*(k%2)), into a dictionary of up to
   * TDR_CMAP_WIDE_MAX_DICT values. */
  int32_t cwords, dict_n;
  const uint32_t* crec;
  const float* dict;    /* [TDR_CMAP_WIDE_MAX_DICT], entry 0 = +0.0f */
  /* Optional SCRATCH of tdr_map_rec16_bytes(ncls, rows, cols) bytes of device memory (NULL: none).  The 40-rotation
   * search of tdr_k_score_polar(init_search != 0) writes the map's records there as pre-split f16 pairs with the
   * filter's class weights folded in and gathers those (twice as fast as splitting the f32 records per sample; same
   * bits).  Its contents mean nothing between calls; two searches that share one map on different streams need a
   * scratch each. */
  void* rec16;
} tdr_map_desc;

const char* tdr_last_error(void);
int tdr_version(void);
int tdr_device_count(void);
/* floats per map / scan record for `ncls` classes */
int tdr_rec_floats(int ncls);

/* ---- map (storage of TopDownMap, include/top_down_render/top_down_map.h:77-79) ------------------------------ */
/* Interleaves the reference's per-class column-major distance maps `class_maps_` ([ncls][rows*cols], element (r,c)
 * at r + rows*c) and the unknown mask `class_mask_` (u8, 1 = unknown) into cell records (tdr_map_desc.rec).
 * rec_out must hold tdr_map_rec_floats_total(ncls, rows, cols) floats. */
size_t tdr_map_rec_floats_total(int ncls, int rows, int cols);
/* bytes behind tdr_map_desc.rec16; 0 when the class count has no matrix-core search (more than 7 classes) */
size_t tdr_map_rec16_bytes(int ncls, int rows, int cols);
/* Filters of fewer particles than this (n_total of tdr_k_score_polar) ignore rec16 (rebuilding it costs one pass over
 * the map); default 8192.  n >= 0 sets the threshold, n < 0 only returns it. */
int64_t tdr_config_rec16_min_particles(int64_t n);
int tdr_k_pack_map(const float* class_maps, const uint8_t* class_mask, int ncls, int rows, int cols, float* rec_out,
                   void* stream);

/* Compact form of the cell records (csrc/tdr_cmap.hip).  Fills map->crec / dict / dict_n / cwords from map->rec;
 * crec_out: tdr_cmap_words_total(ncls, rows, cols) dwords, dict_out: TDR_CMAP_WIDE_MAX_DICT floats, workspace:
 * TDR_CMAP_WORKSPACE_BYTES, all device memory.  Load-time work: synchronises with `stream`.  Maps with more than
 * TDR_CMAP_MAX_DICT distinct distance values or more than 11 classes have no (narrow) compact form: cwords stays 0,
 * TDR_OK — and dict_n = -(distinct values) when the WIDE form exists for the map (4-7 classes, up to
 * TDR_CMAP_WIDE_MAX_DICT values: 16 bytes per cell instead of 8): tdr_k_compact_map_wide then builds it into
 * tdr_cmap_wide_words_total(ncls, rows, cols) dwords.
 * tdr_k_unpack_compact_map decodes either form back into dense records (rec_out like tdr_k_pack_map's output). */
#define TDR_CMAP_MAX_DICT 1024        /* dictionary entries of the narrow form (10-bit fields) */
#define TDR_CMAP_WIDE_MAX_DICT 4096   /* ... of the wide form (16-bit fields; tdr_k_compact_map_wide) */
#define TDR_CMAP_WORKSPACE_BYTES (16384 * 4 + 16384 * 2 + 256)
int tdr_cmap_words(int ncls);
/* dwords behind crec, three parts:
 *  - the record tiles (tdr_cmap_tile_words);
 *  - the map's KNOWN MASK, one bit per cell in 32 x 32-cell tiles of 32 words (one 128-byte line), the tiles stored tile
 *    column by tile column with a guard band of 32 unknown cells around the map: with r' = r + 32, c' = c + 32 cell (r, c)
 *    is bit c & 31 of word (c' >> 5) * 32 * ((rows >> 5) + 2) + r' (csrc/tdr_score_dev.h: kmask_offset);
 *  - from dword tdr_cmap_plane_offset_words on, the CLASS PLANES (tdr_cmap_plane_words dwords each, 0 = none: the map is
 *    too large for 32-bit offsets): per class one 16-bit value per cell — dictionary index * 4 in bits 2-11, known in bit
 *    15 — in tiles of 8 x 8 cells, tile column by tile column, a guard band of 8 cells (csrc/tdr_score_dev.h:
 *    plane_offset); behind them the COARSE MASK PLANE (tdr_cmap_cmask_words dwords), the same shape and tile-column stride
 *    with a 16-bit cell holding the known bits of a 4 x 4 block of map cells: cell (r >> 2, c >> 2), bit (r & 3) * 4 + (c & 3).
 * Behind the float dictionary, `dict` also carries the dictionary as integers (narrow form): entries [1024, 2048) =
 * value * 2^q as uint32, [2048] = q, [2049] = 1 when every value has that form (csrc/tdr_cmap.hip). */
size_t tdr_cmap_words_total(int ncls, int rows, int cols);
size_t tdr_cmap_tile_words(int ncls, int rows, int cols);
size_t tdr_cmap_plane_offset_words(int ncls, int rows, int cols);
size_t tdr_cmap_plane_words(int ncls, int rows, int cols);
size_t tdr_cmap_cmask_words(int ncls, int rows, int cols);
int tdr_k_compact_map(tdr_map_desc* map, uint32_t* crec_out, float* dict_out, void* workspace, void* stream);
size_t tdr_cmap_wide_words_total(int ncls, int rows, int cols);   /* 0: no wide form for this class count */
int tdr_k_compact_map_wide(tdr_map_desc* map, uint32_t* wrec_out, float* dict_out, void* workspace, void* stream);
int tdr_k_unpack_compact_map(const tdr_map_desc* map, float* rec_out, void* stream);

/* Map ingest on the device: TopDownMap::loadCompressedRasterMap (src/top_down_map.cpp:116-144) +
 * computeDists (:289-326) for a class-index image, the work of TopDownMap::updateMap (:146-157) when a new aerial
 * map arrives.  label_img: DEVICE image, img_h x img_w, row-major u8 (cv::Mat CV_8UC1); flatten_lut: DEVICE int32
 * [lut_size] raw label -> flattened class (params_.flatten_lut).  Writes the cell records of the
 * rows = int(img_h/resolution), cols = int(img_w/resolution) map (tdr_map_ingest_shape) into rec_out
 * (tdr_map_rec_floats_total floats).  The Euclidean distance transform is exact. */
size_t tdr_map_ingest_workspace_bytes(int ncls, int rows, int cols);
int tdr_map_ingest_shape(int img_h, int img_w, float resolution, int* rows, int* cols);
/* Incremental ingest of a label image into a map built by tdr_k_map_from_labels (csrc/tdr_map_incr.hip): the same
 * records (and compact form) tdr_k_map_from_labels (+ tdr_k_compact_map) would build from label_img, reached by
 * rebuilding only the cells within R = ceil(50 / resolution) of a cell whose class changed.  Distances are truncated
 * at 50, so every other cell keeps its record bit for bit.  Work is done on TDR_MAP_INCR_TILE^2-cell tiles.
 *   label_img / flatten_lut: DEVICE, as for tdr_k_map_from_labels; same image shape, LUT and class count as the last
 *     ingest of `map` (the caller checks: only the shape is checked here).
 *   map: rec (updated in place), ncls / rows / cols / resolution, and its compact form if any (crec updated in place;
 *     the dictionary is left as it is).
 *   ingest_ws: the workspace of the last tdr_k_map_from_labels / tdr_k_map_update_labels of this map; it holds the class
 *     words and column distances of the map and is updated.
 *   dict_counts: DEVICE int32 [TDR_CMAP_WIDE_MAX_DICT], the dictionary's occurrence counts (tdr_k_map_dict_counts),
 *     updated; needed when map->cwords != 0, NULL otherwise.
 *   max_cells: when the affected tiles hold more cells than this (< 0: no limit), nothing is done and *n_tiles = -1:
 *     a full ingest is cheaper then.
 *   workspace: DEVICE tdr_map_incr_workspace_bytes(rows, cols) bytes.  tiles_out: HOST int32 [tdr_map_incr_tiles]: the
 *     affected tiles (t = ty * ceil(cols / TILE) + tx), *n_tiles of them: the cells whose records may have changed.
 *   *changed_cells: cells whose class word changed.  *compact_ok = 1: the compact form is current (or the class count
 *     has none); 0: the dictionary changed (a value it lacks, or an entry no cell holds any more) or the map had no
 *     compact form: rebuild it with tdr_k_compact_map (and tdr_k_map_dict_counts after it).
 * Load-time work: synchronises with `stream` twice (the tile lists are formed on the host). */
#define TDR_MAP_INCR_TILE 32
#define TDR_MAP_INCR_MAX_FRACTION 0.5   /* tdr_map_update_labels_incremental: above this share of the map, the full path */
int tdr_map_incr_tiles(int rows, int cols);
size_t tdr_map_incr_workspace_bytes(int rows, int cols);
int tdr_k_map_update_labels(const uint8_t* label_img, int img_h, int img_w, const int32_t* flatten_lut, int lut_size,
                            tdr_map_desc* map, void* ingest_ws, int32_t* dict_counts, int64_t max_cells, void* workspace,
                            int32_t* tiles_out, int* n_tiles, int64_t* changed_cells, int* compact_ok, void* stream);
/* The occurrence count of every dictionary entry over the (cell, class) values of the guarded grid: counts = DEVICE int32
 * [TDR_CMAP_WIDE_MAX_DICT], entries [0, dict_n) written.  Needs map->cwords != 0. */
int tdr_k_map_dict_counts(const tdr_map_desc* map, int32_t* counts, void* stream);
/* The cells of n_tiles listed tiles (DEVICE int32, as tiles_out above) in class_maps_' column-major order per tile:
 * maps_out [n][ncls][TILE * TILE] (cell (r, c) of the tile at c * TILE + r), mask_out [n][TILE * TILE] (1 = unknown).
 * Cells outside the map are not written. */
int tdr_k_map_gather_tiles(const float* rec, int ncls, int rows, int cols, const int32_t* tiles, int n_tiles,
                           float* maps_out, uint8_t* mask_out, void* stream);
/* The same from the per-class rasters of the raster cache: planes [ncls][rows][cols] device bytes = the class<i>.png
 * images as stored (8-bit grey, row 0 = top; src/top_down_map.cpp:213-224 flips and scales them, computeDists :289-326
 * binarises: p <= 127 = inside the class, a cell is unknown where every class holds 255).  Classes may overlap.  The map
 * has the images' shape; rec_out / workspace as for tdr_k_map_from_labels (tdr_map_ingest_workspace_bytes). */
int tdr_k_map_from_rasters(const uint8_t* planes, int ncls, int rows, int cols, float resolution, float* rec_out,
                           void* workspace, void* stream);
int tdr_k_map_from_labels(const uint8_t* label_img, int img_h, int img_w, const int32_t* flatten_lut, int lut_size,
                          int ncls, float resolution, float* rec_out, void* workspace, void* stream);
/* The colour-image form (the constructor's .png / .jpg branch, src/top_down_map.cpp:32-42: cv::imread ->
 * SemanticColorLut::color2Ind -> loadCompressedRasterMap): bgr = DEVICE image, img_h x img_w pixels of 3 bytes B, G, R
 * (cv::imread's layout, rows packed, row 0 = top).  A pixel's key is B << 16 | G << 8 | R; fill_keys / flatten_lut are
 * HOST arrays of lut_size <= 256 entries: LUT index i has the key fill_keys[i] & 0xFFFFFF (the key tdr_map_load_svg takes)
 * and the flattened class flatten_lut[i].  color2Ind is taken as the exact inverse of ind2Color over the LUT: the
 * smallest index whose key matches; a pixel that matches no key, or whose index flattens outside [0, ncls), is unknown.
 * Exclusive classes are not applied (loadCompressedRasterMap does not).  Sampling, rec_out and workspace as for
 * tdr_k_map_from_labels. */
int tdr_k_map_from_color(const uint8_t* bgr, int img_h, int img_w, const uint32_t* fill_keys, const int32_t* flatten_lut,
                         int lut_size, int ncls, float resolution, float* rec_out, void* workspace, void* stream);
/* color2Ind over a whole image: index_out = DEVICE img_h x img_w u8 (CV_8UC1): the LUT index of each pixel of the DEVICE
 * BGR image, 255 where no key matches (so index 255 of a 256-key table cannot be told from no match).  fill_keys: HOST,
 * 1 <= n_keys <= 256, keys as above. */
int tdr_k_color_index(const uint8_t* bgr, int img_h, int img_w, const uint32_t* fill_keys, int n_keys, uint8_t* index_out,
                      void* stream);
/* geo_maps_ (top_down_map.h:79) as a 2-class record map {d_without, d_with, 1, 1}, derived from the class records
 * (getGeoRasterMap top_down_map.cpp:410-427 + computeDists :58; exact distance transform), or — constant_one != 0 — the
 * constant 1 of the dynamic-map path (:126-133).  geo_rec_out: tdr_map_rec_floats_total(2, rows, cols) floats;
 * workspace: tdr_map_ingest_workspace_bytes(2, rows, cols) bytes (may be NULL with constant_one). */
int tdr_k_geo_map_from_map(const tdr_map_desc* map, int constant_one, float* geo_rec_out, void* workspace, void* stream);
/* Cell records back to the reference's layout: class_maps_out [ncls][rows*cols] column-major, class_mask_out u8. */
int tdr_k_unpack_map(const float* rec, int ncls, int rows, int cols, float* class_maps_out, uint8_t* class_mask_out,
                     void* stream);

/* TopDownMapPolar::samplePtsPolar (src/top_down_map_polar.cpp:7-19, via TopDownMap::samplePts
 * src/top_down_map.cpp:367-389): fills the HOST table tab[nb*nr][2] = {cos(theta_i)*r_j, sin(theta_i)*r_j}. */
int tdr_polar_table_host(int nb, int nr, float ang_res, float resolution, float* tab_out);
/* The same table as its two factors, fac_out[2 nb + nr] (HOST): {cos, sin}(theta_i) at [2 i], [2 i + 1], r_j at
 * [2 nb + j] — every table entry is one float product of the two (top_down_map_polar.cpp:17-18).  A DEVICE copy handed
 * to a tdr_score_ctx (tdr_score_ctx_set_polar_factors) lets the ray-mapped kernel multiply the offsets itself instead of
 * reading the table; it checks on the device, every call, that the table it was given is those products, and reads the
 * table when it is not. */
int tdr_polar_factors_host(int nb, int nr, float ang_res, float resolution, float* fac_out);

/* ---- scan raster -------------------------------------------------------------------------------------------- */
/* ScanRendererPolar::renderSemanticTopDown (src/scan_renderer_polar.cpp:83-109).
 * pts: n points, `stride` floats apart (pcl::PointXYZI: stride 8, ioff 4; packed xyzi: stride 4, ioff 3);
 * lut256: flatten_lut_ (int32[256], -1 = ignore).  Outputs (either may be NULL):
 *   img_out  [ncls][nb*nr]   the reference's images (zero-filled, counts as float);
 *   pk_out   [nr][nb][rf]    the same counts interleaved per bin, slot rf-1 = sum over classes (scoring input).
 * workspace: device scratch of tdr_raster_workspace_bytes(n) bytes, or NULL.  With it every point's bin is computed
 * once (one atan2f / sqrtf per point) and the LDS tiles stream 4-byte keys; without it every tile bins every point. */
int64_t tdr_raster_workspace_bytes(int64_t n);
int tdr_k_raster_polar(const float* pts, int stride, int ioff, int64_t n, float res, float ang_res,
                       const int32_t* lut256, int ncls, int nb, int nr, float* img_out, float* pk_out, void* workspace,
                       void* stream);
/* ScanRenderer::renderSemanticTopDown (src/scan_renderer.cpp:55-78); img_out [ncls][rows*cols]. */
int tdr_k_raster_cart(const float* pts, int stride, int ioff, int64_t n, float res, const int32_t* lut256, int ncls,
                      int rows, int cols, float* img_out, float* pk_out, void* workspace, void* stream);
/* renderGeometricTopDown: the ground / obstacle images (dead at the reference's call site,
 * src/top_down_render.cpp:540, but part of the class surface).  pts: the ORGANISED cloud, element idy*width + idx
 * (cloud->at(idx, idy)), `stride` floats apart, x y z first; unorganised clouds have height 1.
 *   polar     (src/scan_renderer_polar.cpp:6-81): img_out [2][nb*nr], [0] ground, [1] obstacles; per theta bin the
 *             returns are walked by range descending — equal ranges in input order, the tie rule where the reference's
 *             std::sort leaves the order open; workspace of tdr_raster_geo_workspace_bytes(width*height) bytes;
 *   Cartesian (src/scan_renderer.cpp:7-53): img_out [2][rows*cols]; every column idx is one scan line walked upwards.
 * Counts are exact.  Points with a non-finite x or y are dropped (the reference indexes with (int)NaN there). */
int64_t tdr_raster_geo_workspace_bytes(int64_t n);
int tdr_k_raster_geo_polar(const float* pts, int stride, int64_t width, int64_t height, float res, float ang_res, int nb,
                           int nr, float* img_out, void* workspace, void* stream);
int tdr_k_raster_geo_cart(const float* pts, int stride, int64_t width, int64_t height, float res, int rows, int cols,
                          float* img_out, void* stream);
/* Builds pk_out from caller-supplied images (ParticleFilter::update is handed images, particle_filter.cpp:94-95). */
int tdr_k_pack_scan(const float* img, int ncls, int nb, int nr, float* pk_out, void* stream);

/* ---- scoring: StateParticle::computeWeight for all particles (src/state_particle.cpp:157-219 =
 *      TopDownMapPolar::getLocalMap src/top_down_map_polar.cpp:21-53 + getCostForRot src/state_particle.cpp:112-155,
 *      driven by ParticleFilter::update src/particle_filter.cpp:104-105) ------------------------------------- */
/* workspace floats needed by tdr_k_score_polar for n particles */
size_t tdr_score_workspace_floats(int ncls, int nb, int nr, int64_t n, int64_t n_total);
/* Scores particles [0,n) of st (plane stride cap) against the packed scan at each particle's own theta; writes raw
 * weights raw_w[n] (NaN = "too much unknown", 0 = gated by force_on_map / scale range, state_particle.cpp:163-176).
 * perm (optional, int32[n]): processing order (a permutation of 0..n-1, e.g. from tdr_k_locality_order) for cache
 * locality; results are independent of it.  tab: DEVICE copy of the table from tdr_polar_table_host.
 * uniform_scale: > 0 is the caller's promise that every particle's scale equals it (fixed or frozen scale,
 * particle_filter.cpp:24,343-357): the sample offsets (tab*scale)*res are then evaluated once per call instead of
 * once per particle and sample — same float operations, same results; <= 0 reads each particle's own scale.
 * init_search != 0: particles whose have_init is 0 (and that are not gated) first run the 40-rotation search of
 * state_particle.cpp:195-206 — one pass over their window scoring all candidate rotations — which sets their theta
 * and have_init in st; they are then scored at that rotation like everyone else (all-NaN searches keep the
 * reference's 1/(FLT_MAX + regularization)).  Batches without such particles exit immediately; nothing synchronises
 * with the host.  Pass 0 when the caller knows every particle is initialised.
 * n_total: the particle count of the WHOLE filter (all ranks of a sharded filter; <= 0 means n).  The kernel splits a
 * particle's score into partial sums over groups of range rings, sized from the image shape and n_total — a small filter
 * gets many short workgroups — so a shard scored on its own gives the same bits as the same particles inside the
 * one-rank filter. */
int tdr_k_score_polar(const tdr_map_desc* map, const float* tab, const float* scan_pk, int nb, int nr, float res,
                      const tdr_filter_params* fp, float* st, int64_t cap, int64_t n, int64_t n_total,
                      const int32_t* perm, float uniform_scale, int init_search, float* raw_w, float* workspace,
                      void* stream);
/* The same with a caller-owned context.  A large launch runs two kernels one after the other on `stream` — dense particles
 * through the shift-uniform kernel, scattered ones through the ray-mapped kernel (tdr_config_shift_uniform below) — and
 * chooses the split between them by timing; the context keeps the tuner's state from call to call.  One context per filter
 * (or per caller thread); calls that share a context must not overlap.  ctx == NULL: tdr_k_score_polar — the configured
 * span, no state.  Results never depend on the context.  Nothing waits on the host either way (the tuner polls its events).
 * tdr_score_ctx_span: the split the context's tuner has settled on so far (map cells). */
typedef struct tdr_score_ctx tdr_score_ctx;
int tdr_score_ctx_create(tdr_score_ctx** out);
void tdr_score_ctx_destroy(tdr_score_ctx* ctx);
float tdr_score_ctx_span(const tdr_score_ctx* ctx);
/* launches of this context that ran at a TRIAL span so far (a benchmark reports how many fell into its timed region) */
int64_t tdr_score_ctx_trial_calls(const tdr_score_ctx* ctx);
/* fac_dev: device copy of tdr_polar_factors_host's output for the (nb, nr) table the context's calls score with; the
 * caller's memory, alive until replaced (NULL: none).  Calls with another shape ignore it. */
int tdr_score_ctx_set_polar_factors(tdr_score_ctx* ctx, const float* fac_dev, int nb, int nr);
int tdr_k_score_polar_ctx(const tdr_map_desc* map, const float* tab, const float* scan_pk, int nb, int nr, float res,
                          const tdr_filter_params* fp, float* st, int64_t cap, int64_t n, int64_t n_total,
                          const int32_t* perm, float uniform_scale, int init_search, float* raw_w, float* workspace,
                          tdr_score_ctx* ctx, void* stream);

/* Scoring WITH the geometric term of getCostForRot (src/state_particle.cpp:145-152: commented out in the reference, whose
 * geometric images are all-zero anyway; opt-in here): cost += (geo_i . shifted geo_cls_i).sum() * 0.01 and
 * normalization += geo_i.sum() for the two geometric layers.  geo_map: the 2-layer map of tdr_k_geo_map_from_map;
 * geo_pk: the two geometric scan images packed by tdr_k_pack_scan(img, 2, nb, nr); geo_sum0/1: the sums of those images.
 * Everything else as tdr_k_score_polar; the init search prices the geometric term for every candidate rotation (one
 * scoring pass per rotation over the batches that hold an un-initialised particle).
 * workspace: tdr_score_geo_workspace_floats. */
size_t tdr_score_geo_workspace_floats(int ncls, int nb, int nr, int64_t n, int64_t n_total);
int tdr_k_score_polar_geo(const tdr_map_desc* map, const tdr_map_desc* geo_map, const float* tab, const float* scan_pk,
                          const float* geo_pk, float geo_sum0, float geo_sum1, int nb, int nr, float res,
                          const tdr_filter_params* fp, float* st, int64_t cap, int64_t n, int64_t n_total,
                          const int32_t* perm, float uniform_scale, int init_search, float* raw_w, float* workspace,
                          void* stream);

/* Cartesian scoring (BASELINE config 4).  The reference's StateParticle only reaches the polar overloads
 * (state_particle.h:61), so there is no reference function to match; the score is DEFINED as the window of
 * TopDownMap::getLocalMap(center, rot = theta, res = res*scale) (src/top_down_map.cpp:429-459) scored by
 * getCostForRot with shift 0 (src/state_particle.cpp:132-143), weight = 1/(cost + regularization), no gates.
 * scan_pk: packed [cols][rows][rf] Cartesian render (tdr_k_raster_cart / tdr_k_pack_scan with nb=rows, nr=cols).
 * n_total: particle count of the whole (possibly sharded) filter, as in tdr_k_score_polar (0 = n): it fixes the split
 * of the window into partial sums, so that a shard scores its particles to the same bits as the one-rank filter. */
size_t tdr_score_cart_workspace_floats(int ncls, int rows, int cols, int64_t n, int64_t n_total);
int tdr_k_score_cart(const tdr_map_desc* map, const float* scan_pk, int rows, int cols, float res,
                     const tdr_filter_params* fp, float* st, int64_t cap, int64_t n, int64_t n_total,
                     const int32_t* perm, float* raw_w, float* workspace, void* stream);
/* The HEADING SEARCH of the Cartesian filter (csrc/tdr_score_cart_init.hip): what StateParticle::computeWeight does for a
 * particle with have_init == 0 (src/state_particle.cpp:195-206), with the Cartesian cost above in place of
 * getCostForRot(..., t).  DEFINITION:
 *  - the candidates are the reference's float loop `for (float t = 0; t < 2*M_PI; t += 2*M_PI/40)` as written (float t,
 *    double increment): the table the polar search uses;
 *  - the cost of candidate t is the Cartesian cost of that particle with theta = t, exactly as tdr_k_score_cart defines it
 *    (a window less than half known gives NaN);
 *  - the first candidate whose cost is strictly smaller than all earlier ones wins; a NaN cost is never chosen;
 *  - afterwards theta = the best t (0 when no candidate was finite) and have_init = 1;
 *  - there are no gates, and particles that already have a heading are not touched: their states stay bit for bit.
 * The search only CHOOSES headings: the weights are what a following tdr_k_score_cart gives at those headings (it scores
 * every particle, as the polar path does after its search).
 * It is composed of a list of the particles without a heading (one small launch; made again in the order of
 * tdr_k_locality_order_pose when it spans several chunks, so that a chunk is a neighbourhood of the map), and per chunk of
 * tdr_config_tuning("cart_init_chunk") listed particles: their candidate states, their order by pose
 * (tdr_k_locality_order_pose at theta_radius = (rows + cols) / 16, what the filters pass as `perm`), ONE tdr_k_score_cart
 * launch over them — the form tdr_config_shift_uniform / tdr_config_cart_skip select, the partial-sum split of n_total, so a
 * candidate's weight is the bits the regular launch gives that particle at that heading and the result does not depend on
 * the chunk size — and a selection.  Nothing is allocated.  The launcher WAITS for `stream` ONCE, to read the list's length: that many chunks are
 * launched, and a call that finds no particle without a heading costs the list launch and no scoring launch.  A caller that
 * knows every particle has a heading does not call it.  Arguments as tdr_k_score_cart (n_total <= 0 means n); errors
 * (TDR_ERR_ARG before any device work): null map / scan / states / workspace, rows < 1, cols < 1, n < 0, n > cap.
 * workspace: tdr_score_cart_init_workspace_floats floats — the list, one chunk's candidate states, raw weights and order,
 * and tdr_score_cart_workspace_floats for one chunk's candidates — read with the cart_init_chunk in force at the call. */
size_t tdr_score_cart_init_workspace_floats(int ncls, int rows, int cols, int64_t n, int64_t n_total);
int tdr_k_score_cart_init(const tdr_map_desc* map, const float* scan_pk, int rows, int cols, float res,
                          const tdr_filter_params* fp, float* st, int64_t cap, int64_t n, int64_t n_total,
                          float* workspace, void* stream);

/* ---- StateParticle::propagate for all particles (src/state_particle.cpp:57-78 via particle_filter.cpp:86-92) -- */
/* z4: optional DEVICE array [n][4] of standard normals {theta, dx, dy, scale} in the reference's consumption
 * order (parity mode, from tdr_propagate_normals_host); NULL = counter-based device RNG keyed by (seed, step). */
int tdr_k_propagate(float* st, int64_t cap, int64_t n, float* last_dist, float tx, float ty, float omega,
                    int scale_freeze, float pos_cov, float theta_cov, const float* z4, uint64_t seed, uint64_t step,
                    int64_t index_base, void* stream);
/* The shared std::mt19937 of the reference (particle_filter.h:52): host-side handle, explicit seed. */
void* tdr_rng_create(uint32_t seed);
void tdr_rng_destroy(void* rng);
float tdr_rng_uniform_host(void* rng);                      /* particle_filter.cpp:172-173 */
int tdr_propagate_normals_host(void* rng, int64_t n, int scale_freeze, float* z4_out);
/* The same stream on the DEVICE (csrc/tdr_rng.hip).  `state`: TDR_RNG_STATE_WORDS device words — a std::mt19937 in
 * libstdc++'s own representation: [0, 624) the engine's state array, [624] the index of the next word (624: a twist comes
 * first), [625] an error flag the kernels raise if a call runs out of its attempt budget (probability ~1e-23; then the state
 * is left alone and tdr_rng_set_state_host refuses it).  tdr_rng_get_state_host / _set_state_host move a host engine's state
 * into and out of that form (HOST arrays), so either side can continue the other's stream.
 * tdr_k_rng_propagate_normals: z4_out (device) [hi - lo][4] = the standard normals {theta, dx, dy, scale} of particles
 * [lo, hi) of a propagate call over n particles — bit for bit what tdr_propagate_normals_host draws for them — and the
 * state moves on by the words the WHOLE call consumes (every rank of a sharded filter passes its own [lo, hi) and keeps
 * the same state).  Marsaglia attempts are independent given the words, so only the generator's state recurrence is
 * serial (one wave); acceptance, ranking and the normals themselves are data-parallel.  workspace: device scratch of
 * tdr_rng_dev_workspace_bytes(n) bytes.  tdr_k_rng_uniform: *out_dev = std::uniform_real_distribution<float>(0, 1)(gen),
 * the draw of the systematic resample (src/particle_filter.cpp:172-173).  Nothing synchronises. */
#define TDR_RNG_STATE_WORDS 640
size_t tdr_rng_dev_workspace_bytes(int64_t n);
int tdr_k_rng_propagate_normals(uint32_t* state, int64_t n, int64_t lo, int64_t hi, int scale_freeze, float* z4_out,
                                void* workspace, void* stream);
int tdr_k_rng_uniform(uint32_t* state, float* out_dev, void* stream);
int tdr_rng_get_state_host(void* rng, uint32_t* words);
int tdr_rng_set_state_host(void* rng, const uint32_t* words);
/* tdr_rng_pipe: the generator of ONE filter on the device, drawing ahead (csrc/tdr_rng.hip).  A filter's step draws in a
 * fixed order — propagate's normals, the resample's uniform, the next step's normals — and none of it depends on the
 * particles: when a propagate call has been served, the pipe draws what the step after it will most likely ask for on a
 * stream of its own, beside the scoring launch.  A call that asks for something else (another particle count, another
 * order, the host engine taking the stream back) makes it drop what it drew ahead and continue from the state the stream
 * really is in: the values handed out are the stream's own in every case.  One pipe per filter, one caller thread; n_max:
 * the largest particle count of a call.  from_host / to_host move the stream between a host std::mt19937 and the device
 * (they synchronise `stream`); normals / uniform are ordered on `stream` and wait for nothing on the host; the device
 * pointers they return stay valid until the next call of the same function. */
typedef struct tdr_rng_pipe tdr_rng_pipe;
int tdr_rng_pipe_create(int64_t n_max, tdr_rng_pipe** out);
void tdr_rng_pipe_destroy(tdr_rng_pipe* p);
int tdr_rng_pipe_on_device(const tdr_rng_pipe* p);
int tdr_rng_pipe_from_host(tdr_rng_pipe* p, void* host_rng, void* stream);
int tdr_rng_pipe_to_host(tdr_rng_pipe* p, void* host_rng, void* stream);
int tdr_rng_pipe_normals(tdr_rng_pipe* p, int64_t n, int64_t lo, int64_t hi, int scale_freeze, const float** z4_out,
                         void* stream);
int tdr_rng_pipe_uniform(tdr_rng_pipe* p, const float** shift_out, void* stream);
/* ParticleFilter::initializeParticles particle loop (src/particle_filter.cpp:57-71) with the StateParticle
 * constructor (src/state_particle.cpp:3-49): host-side, serial mt19937 draws with on-road rejection.
 * class_maps: HOST copy of class_maps_ (column-major [ncls][rows*cols]); out must hold max_num+16 states. */
/* One particle drawn like StateParticle's constructor (src/state_particle.cpp:3-49). */
int tdr_init_particle_host(void* rng, const float* class_maps, int ncls, int rows, int cols, float resolution,
                           const tdr_filter_params* fp, tdr_state* out);
int tdr_init_particles_host(void* rng, const float* class_maps, int ncls, int rows, int cols, float resolution,
                            const tdr_filter_params* fp, int max_num, tdr_state* out, int64_t* n_out);
/* The same particle loop on the DEVICE (csrc/tdr_init.hip): for the same generator state and map it writes the same
 * states as tdr_init_particles_host and leaves the generator at the same word.  rng_state_dev: TDR_RNG_STATE_WORDS device
 * words (tdr_k_rng_propagate_normals); the on-road test reads the class-1 slot of map->rec.  Particles [lo, hi) of the
 * n_out = tdr_init_particles_count(fp, max_num) the loop keeps go to the SoA planes st (stride cap) at index i - lo;
 * dx_m = dy_m = 0.  Every rank of a sharded filter runs the whole chain and writes its own slice.  The stream is read in
 * windows of tdr_config_tuning("init_window_words") words; workspace: tdr_init_workspace_bytes() bytes of device memory,
 * fixed by the window, not by max_num.  Synchronises `stream` once per window.  Errors as the host loop's: fewer than 2
 * classes, a map without a road cell (TDR_ERR_ARG, no word drawn); unknown scale with max_num < 10 keeps 0 particles
 * and draws nothing.  tdr_rng_pipe_init_particles runs it on a pipe's state (the pipe must be on the device): what the
 * pipe drew ahead is dropped and the stream stays on the device. */
int64_t tdr_init_particles_count(const tdr_filter_params* fp, int max_num);
size_t tdr_init_workspace_bytes(void);
int tdr_k_init_particles(uint32_t* rng_state_dev, const tdr_map_desc* map, const tdr_filter_params* fp, int max_num,
                         int64_t lo, int64_t hi, float* st, int64_t cap, int64_t* n_out, void* workspace, void* stream);
int tdr_rng_pipe_init_particles(tdr_rng_pipe* p, const tdr_map_desc* map, const tdr_filter_params* fp, int max_num,
                                int64_t lo, int64_t hi, float* st, int64_t cap, int64_t* n_out, void* workspace,
                                void* stream);

/* ---- ParticleFilter::update, weight statistics (src/particle_filter.cpp:107-147) ---------------------------- */
/* raw_w, last_dist: [n] -> w_out [n] final normalised weights; info_out (device, TDR_UW_INFO_FLOATS floats: the first 8
 * are {argmax (as int bits), sum, mean, bottom_stddev, fallback, num_valid, num_under, 0}, the rest is scratch for
 * the multi-workgroup reductions and the chunk headers of the exact chains).  The result is a pure function of
 * (raw_w, last_dist, n).  `sum`, `mean` and `bottom_stddev` are the reference's serial float32 accumulations bit for
 * bit at every n (csrc/tdr_prefix.hip: uw_small_kernel up to 32768 particles, tdr_chain_total above).  n is limited
 * to what the scratch holds: 40 bytes per chunk of 4096 weights behind ~12 KB of reduction scratch, about 25 million.
 * (Up to about 3.7 million the scratch also holds 24 bytes per 512 weights and 32 KB of slots, with which the chains are
 * summarised over the whole chip; beyond, one workgroup walks the 4096-chunks.) */
#define TDR_UW_INFO_FLOATS 65536
int tdr_k_update_weights(const float* raw_w, const float* last_dist, int64_t n, float* w_out, float* info_out,
                         void* stream);

/* ---- systematic resample (src/particle_filter.cpp:171-185) -------------------------------------------------- */
/* Serial-order float32 running sum of w (the additions of :179 in the same order) and its running maximum.
 * workspace: device scratch of tdr_prefix_workspace_bytes(n) bytes, or NULL.  From 256 to 32 768 weights — the
 * reference's operating point — everything is one launch of one workgroup with the weights in LDS; above, with a
 * workspace, the chain is evaluated by many workgroups (per-chunk parity summaries, see csrc/tdr_prefix.hip); without
 * one, by one workgroup.  The bits written are the serial chain's either way.  tdr_config_prefix_small(0) takes the
 * one-launch kernel and, above 32 768 weights, the wave-chunk path of this chain and of the statistics chains out of
 * the choice (A/B measurements, tests), 1 restores the default, < 0 only queries; env TDR_PFX_SMALL.
 * tdr_prefix_workspace_bytes: 32 bytes per 4096 weights; above 32 768 weights also 24 bytes per 512 weights, 4 per
 * 4096 and about 32 KB. */
int tdr_config_prefix_small(int on);
int64_t tdr_prefix_workspace_bytes(int64_t n);
int tdr_k_prefix(const float* w, int64_t n, float* runmax_out, void* workspace, void* stream);
/* Same, choosing the implementation: mode 0 = one wave adding in index order, 1 = the exact parallel kernel in one
 * workgroup (integer increments per binade), 2 = the multi-workgroup scan (workspace required), 3 = the one-launch
 * kernel (n <= 32 768); all give identical bits.  prefix_out (optional, modes 1 to 3) = raw sums. */
int tdr_k_prefix_mode(const float* w, int64_t n, int mode, float* runmax_out, float* prefix_out, void* workspace,
                      void* stream);
/* idx_out[i - i_begin] = first j with prefix_j > (float(i)+shift)/n_new, else n-1, for i in [i_begin, i_end). */
int tdr_k_resample(const float* runmax, int64_t n, int64_t n_new, float shift, int64_t i_begin, int64_t i_end,
                   int32_t* idx_out, void* stream);
/* The same with the shift read from device memory (tdr_k_rng_uniform): no host value in the step. */
int tdr_k_resample_dev(const float* runmax, int64_t n, int64_t n_new, const float* shift_dev, int64_t i_begin, int64_t i_end,
                       int32_t* idx_out, void* stream);
/* new_particles_[i]->setState(particles_[j]->state()) (:184): dst[f][i] = src[f][idx[i]].
 * src_shard == 0: src is a plain [7][src_cap] SoA.  src_shard > 0: src is the all-gathered [rank][7][src_shard]
 * buffer of a sharded filter and idx holds global particle indices (rank*src_shard + local). */
int tdr_k_gather_states(const float* src, int64_t src_cap, int64_t src_shard, const int32_t* idx, int64_t n_new,
                        float* dst, int64_t dst_cap, void* stream);

/* Buffers of a sharded filter (one rank per GPU): {a, b}[nl] -> one send buffer [2][nl]; the gathered
 * [world][2][nl] -> a_glob / b_glob [world*nl] in global particle order; the gathered state planes [world][7][nl] ->
 * a plain SoA [7][cap]. */
int tdr_k_shard_pack2(const float* a, const float* b, int64_t nl, float* out, void* stream);
int tdr_k_shard_unpack2(const float* in, int world, int64_t nl, float* a_glob, float* b_glob, void* stream);
int tdr_k_unshard_states(const float* in, int world, int64_t nl, float* st, int64_t cap, void* stream);

/* ---- getLocalMap materialised (src/top_down_map_polar.cpp:21-53, src/top_down_map.cpp:429-459) ----------------- */
/* The window of ONE pose as the reference's arrays: dists_out (device) [ncls][rows*cols] column-major images,
 * mask_out (device) [rows*cols], 1 = unknown or outside the map.  Polar: rows = nb, cols = nr, `tab` from
 * tdr_polar_table_host, centre (cx, cy) in metres like StateParticle's (cx / resolution is the cell).  Cartesian:
 * samplePts(center / resolution, rot, cols, rows, res / resolution) (top_down_map.cpp:433-434). */
int tdr_k_local_map_polar(const tdr_map_desc* map, const float* tab, int nb, int nr, float cx, float cy, float scale,
                          float res, float* dists_out, uint8_t* mask_out, void* stream);
int tdr_k_local_map_cart(const tdr_map_desc* map, int rows, int cols, float cx, float cy, float rot, float res,
                         float* dists_out, uint8_t* mask_out, void* stream);

/* ---- ActiveLocalizer (src/active_localizer.cpp; dead at its call sites src/particle_filter.cpp:77-78,316) -------------- */
/* computeTotalDifference (:7-20) over getLocalMap (:22-42) for many candidates at once.  centres (device) [ncand][K][2]:
 * position {x, y} of hypothesis i displaced by candidate q (:62-63); shifts (device) [K]: rot_shift of hypothesis i
 * (:33-36); res: getLocalMap's resolution (2 at :30); (nb, nr) the shape of `tab` (100 x 25 in the reference).
 * sums_out (device) [ncand] doubles: sum over pairs i > j, classes and samples of |L_i - L_j|; the reference's figure is
 * sum / (K (K-1) / 2 * ncls).  K <= 32. */
int tdr_k_active_diffs(const tdr_map_desc* map, const float* tab, int nb, int nr, float res, const float* centres,
                       const int32_t* shifts, int K, int ncand, double* sums_out, void* stream);
/* The candidates of getBestRelPos (:55-77) — distances 50, 75, 100, 125; directions by the float loop `theta += pi / 8`
 * as written — for the HOST arrays preds [K][3] = {x, y, theta}: centres [4 * 17][K][2], dists / thetas [4 * 17] (candidate
 * d * 17 + t), shifts [K]; *ntheta_out directions per distance, *ndist_out distances. */
int tdr_active_candidates_host(const float* preds, int K, int nb, float* centres, float* dists, float* thetas,
                               int32_t* shifts, int* ntheta_out, int* ndist_out);

/* ---- per-step consumers (src/particle_filter.cpp:191-236, 325-334, 343-357) --------------------------------- */
/* out (device, TDR_MEAN_COV_FLOATS floats; the first 24 are the result, the rest is scratch for the multi-workgroup
 * reductions): mean[4] (meanLikelihood :191-203), cov[16] row-major about the mean (computeMeanCov, about == NULL) or
 * about the 4 device floats `about` (computeCov about the max-likelihood mlState :226-236), geometric-mean scale
 * (freezeScale :345-348), 3 spare.  A pure function of (st, n, about). */
#define TDR_MEAN_COV_FLOATS 4800
int tdr_k_mean_cov(const float* st, int64_t cap, int64_t n, const float* about, float* out, void* stream);
int tdr_k_set_scale(float* st, int64_t cap, int64_t n, const float* scale_dev, void* stream);   /* freezeScale :350-352 */
/* max_likelihood_particle_ (:145-147): out12 (device) = the 7 SoA fields of particle argmax (info[0] of
 * tdr_k_update_weights), one spare, then its mlState {x, y, theta, scale} (state_particle.cpp:98-102).  Call before the
 * resampled set replaces `st`. */
int tdr_k_save_ml_state(const float* info, const float* st, int64_t cap, int64_t src_shard, int64_t n, float* out12,
                        void* stream);   /* src_shard > 0: st is the all-gathered [rank][7][src_shard] buffer */
int tdr_k_shift_init(float* st, int64_t cap, int64_t n, float dx, float dy, void* stream);      /* updateMap :325-334 */
/* The three calls an unsharded update ends with, in one launch: idx_out as tdr_k_resample_dev (shift_dev != NULL) or
 * tdr_k_resample (`shift`), dst[f][i - i_begin] = src[f][idx] as tdr_k_gather_states (both source layouts; dst is not src)
 * and out12 as tdr_k_save_ml_state, taken from src — the set BEFORE the resample.  The same bits as the three calls. */
int tdr_k_resample_gather(const float* runmax, int64_t n, int64_t n_new, const float* shift_dev, float shift,
                          int64_t i_begin, int64_t i_end, int32_t* idx_out, const float* src, int64_t src_cap,
                          int64_t src_shard, float* dst, int64_t dst_cap, const float* info, float* out12, void* stream);

/* The scoring kernels read the compact records whenever the map has them (tdr_k_compact_map); tdr_config_compact(0)
 * forces the dense records (A/B measurements, tests), 1 restores the default, < 0 only queries.  Results never depend on
 * it: both forms decode to the same operands.  Returns the value in force. */
int tdr_config_compact(int on);
/* Large polar launches take the INTEGER form of the score.  A scan count is an integer and a distance value of the map
 * an integer multiple of 2^-q (tdr_cmap_words_total above), so a class's product sum is accumulated as a 64-bit integer:
 * exact, hence independent of the order of the additions and of the kernel that forms it.  Two kernels share a launch:
 *  - DENSE particles — those whose 64 neighbours in the locality order lie within the SPAN, a number of map cells (0 =
 *    every particle counts as dense, a very large span = none) — go in (heading bin, Morton) order, every bin padded to
 *    whole waves, lane = particle: the scan side of a sample is a scalar operand and empty scan bins / absent classes are
 *    skipped wave-wide (csrc/tdr_score_su.hip);
 *  - the others one WAVE per particle, lanes = consecutive samples along a ray, gathering 2-byte cells of per-class
 *    planes (csrc/tdr_score_ray.hip).
 * Whichever kernel scores a particle, its weight is the same bits; the float kernel (score_polar_kernel: small filters,
 * shapes and maps the integer form does not cover, scans with fractional or non-finite counts — detected on the device)
 * agrees with it to rounding (<= 1e-6 relative).
 * mode 0 = never, 1 = when the filter holds enough particles per heading bin for the padding to pay (default: 64 x the
 * polar image's rows), 2 = whenever the shapes allow (ring groups and ring count multiples of 4, a map with narrow
 * compact records and class planes); < 0 only returns the mode.
 * The span: a launch with a tdr_score_ctx TUNES it while the filter runs — from the 31st call of a shape on, 2, 8, 16, 24
 * and 40 cells are timed over two scoring calls each (HIP events on the caller's stream, polled, never waited for), the fastest is kept and the trial is
 * repeated every 4000 calls.  Results never depend on it.  tdr_config_shift_uniform_span(cells >= 0) fixes
 * it for every caller; -1 only returns the configured span (16 by default: what a launch without a context uses); -2 goes
 * back to tuning. */
int tdr_config_shift_uniform(int mode);
float tdr_config_shift_uniform_span(float cells);
/* Waves a scattered particle's window is split over in the ray-mapped kernel (1 .. 8; 0 = chosen per launch from its size,
 * the default; < 0 only queries).  The sums are exact integers: results never depend on it (tests). */
int tdr_config_ray_split(int k);
/* Large Cartesian launches (a filter of >= 4096 particles on a map with narrow compact records and class planes) take the
 * INTEGER form too, with the same guarantee as the polar one (tdr_config_shift_uniform above, whose mode 0 switches both
 * off): dense particles through the skipping kernel below with 64-bit integer accumulators, scattered ones one wave each,
 * lanes = consecutive window columns (csrc/tdr_score_cart.hip: score_cart_ray_kernel); the span is four times the polar
 * launch's.  The float kernels score what has no integer form and agree to rounding.
 * The Cartesian scoring has a second kernel that reads the scan side of a sample as a scalar descriptor and gives an empty
 * scan bin one 4-byte gather from the map's known mask instead of the record gather, decode and FMAs
 * (csrc/tdr_score_cart.hip); same partial sums, bit for bit.  It is used whenever the map has narrow compact records;
 * 0 forces the general kernel (A/B measurements, tests), 1 restores the default, < 0 only queries. */
int tdr_config_cart_skip(int on);
/* The 40-rotation search of a particle without a heading (src/state_particle.cpp:195-206) runs on the matrix cores
 * (v_mfma_f32_16x16x32_f16; every record size: 4 / 8 floats through pre-split half records or split on the fly, 12 / 16
 * floats in two groups of 8 slots); 0 forces the vector-unit search (A/B measurements, tests), 1 restores the default,
 * < 0 only queries.  Only the choice among rotations whose costs tie to rounding can differ. */
int tdr_config_init_mfma(int on);
/* The weight statistics of at most 32 768 particles (src/particle_filter.cpp:107-147) evaluate their two serial float
 * chains wave by wave: predicted wave-chunks in parallel, the rest carried through by one wave without workgroup barriers
 * (csrc/tdr_prefix.hip); 0 forces the chunk-by-chunk evaluation on the whole workgroup (A/B measurements, tests), 1
 * restores the default, < 0 only queries.  Same bits either way. */
int tdr_config_uw_waves(int on);
/* diagnostics: scoring launches of this process that took the shift-uniform kernel */
int64_t tdr_shift_uniform_launches(void);

/* ---- measurement ---------------------------------------------------------------------------------------------- */
/* While enabled, every launch of the scoring kernel is bracketed by HIP events on its launch stream;
 * tdr_profile_score_ms synchronises on them, returns the summed duration and the launch count, and resets. */
int tdr_profile_enable(int on);
int tdr_profile_score_ms(double* total_ms, int64_t* launches);
/* While enabled, a polar launch of the integer form also brackets each of its two kernels: the last such launch's durations — shift-uniform kernel over the dense particles,
 * ray-mapped kernel over the scattered ones — and the number of scattered particles (synchronises).  Measurement state is
 * process-wide like the switch itself: one measuring thread. */
int tdr_profile_shares(double* dense_ms, double* scattered_ms, int64_t* scattered_particles);
/* With tdr_profile_enable(2) — never inside a timed region: an atomic per wave-sector slows the kernels — the dense kernels count which loop variant each wave-sector (polar) / wave-segment (Cartesian) ran; reads
 * and resets the 16 counters (synchronises): [0..2] score_polar_su_kernel with the workgroup's staged box — every cell known /
 * every cell inside the map / general; [3..5] the same with the wave's own box; [6] its far path; [8..10]
 * score_cart_su_kernel — all known / inside / general; [11] its plain steps (a box that did not fit).
 * The 40-rotation init search counts the 64-particle batches whose results each of its passes wrote (one atomic per
 * workgroup; a batch with nothing to initialise counts nothing): [12] the matrix-core pass on half records, [13] the one
 * that splits the records on the fly, [14] the one on wide records, [15] the vector kernel — alone, or redoing a search whose
 * scan counts did not fit f16 (then the matrix-core pass has counted the same batches too). */
int tdr_profile_variants(int64_t out[16]);
/* With tdr_profile_enable(2), likewise outside timed regions: how the ray-mapped kernel's gate count ended, for the launches
 * that walk compact bin lists (a context with the table's factors, a direction count that is a multiple of 16 and <= 256).
 * Reads and resets four counters (synchronises): [0] scattered particles whose count was settled by the non-empty bins alone
 * (at least half the samples known, or too few even with every empty bin's cell known); [1] particles whose waves stopped
 * walking the empty bins once the shared count reached half the samples; [2] particles whose empty bins were walked to the
 * end (always, where a particle's waves do not share a workgroup or the window has 2^24 samples or more); [3] blocks of up
 * to 256 empty bins walked, over all waves. */
int tdr_profile_ray_gate(int64_t out[4]);
/* With tdr_profile_enable(2), likewise outside timed regions: what became of the scan bins that hold several classes in
 * score_polar_su_kernel's assembly path (one atomic per wave and counter).  Reads and resets two counters (synchronises):
 * [0] four-ring steps the assembly loop handed to the C++ step ("su_full_list" = 0: every step with such a bin; 1: only
 * steps where a non-finite value is in play); [1] bins the list pass behind the loop scored — with every particle dense,
 * (dense waves) x (bins of the scan with several classes).  (The 16 counters of tdr_profile_variants are all in use.) */
int tdr_profile_su_list(int64_t out[2]);

/* The library reads NOTHING from the process environment: behaviour switches are these calls (and the tdr_config_* calls
 * above), process-wide, meant for A/B measurements, tests and debugging — results never depend on them unless stated.
 * One thread configures, while no other is inside the library.  The library itself never writes them: tdr_selftest_score
 * runs its kernel variants without setting a switch — they are what they were after it, a fixed span included, and no other
 * thread sees them move while it runs.
 * tdr_config_tuning(name, value): value < 0 queries; returns the value in force, -1 for an unknown name.
 *   "score_waves"      waves the float / Cartesian scoring kernels aim for (default 131072)
 *   "score_group"      rings per workgroup of the float and shift-uniform kernels, 0 = from the shapes (changes the
 *                      partition of the FLOAT kernel's sums: its results move in the last bits)
 *   "su_group"         rings per workgroup of the shift-uniform kernel alone (a multiple of 4; integer sums: same bits)
 *   "init_ahead"       record loads in flight in the init search (1-3)
 *   "batch_init_search"  0 (default): a filter that may hold a particle without a heading runs its standalone
 *                      calls inside tdr_batch_step; 1: it joins the batch, its search one launch per pass kind
 *                      for the whole batch (same bits)
 *   "prefix_head"      leading addends the long running sum's walk adds one by one
 *   "ray_block_major"  0: the ray-mapped kernel keeps its first row order (direction-major) also when the caller's context
 *                      holds the table's factors (same bits)
 *   "ray_patch"        0: the ray-mapped kernel walks 64 rings of ONE direction per step also where the patch order applies (a
 *                      context with the table's factors, a direction count that is a multiple of 16, at most 256): 1 (default) =
 *                      4 directions x 16 rings per step, a lane's four descriptors of a unit in one load (same bits)
 *   "ray_borrow"       0: an empty scan bin of the ray-mapped kernel reads its known bit from the coarse mask plane; 1 (default):
 *                      from the class plane its nearest non-empty neighbour of four rings reads anyway (same bits)
 *   "mt_stretches"     0: the reference's random stream is always generated by one wave; 1 (default): calls of more than 128
 *                      state blocks fill stretches side by side, reached by jump-ahead (csrc/tdr_rng.hip) — the same words
 *   "cart_seg_rows"    window rows per segment of score_cart_su_kernel (a multiple of 4; 0: the Cartesian integer form's dense
 *                      share goes through the plain kernel instead — same bits)
 *   "su_tail_groups"   K: how many of the LAST ring groups of score_polar_su_kernel's grid are cut into sector ranges, so that
 *                      the workgroups dispatched last are short and the launch's run-down with them (default 4; a launch
 *                      of fewer than two rounds of the chip's resident workgroups takes none — except under
 *                      tdr_config_shift_uniform(2), where the knobs hold on every shape)
 *   "su_tail_parts"    Q: into how many sector ranges each of them is cut — 1, 2, 4 or 8 (another value: the next lower of
 *                      these).  K = 0 or Q = 1 is the launch without tail units.  Integer sums: same bits for every K, Q.
 *                      The grid then has (groups - K) + K Q rows; each adds its share of a slot's integer sums in place, into
 *                      the one row of sums a slot has.  tdr_score_workspace_floats still GROWS with the rows (nothing is
 *                      clamped: K up to every group, Q up to 8) — like "su_group", set both BEFORE the workspace of a call
 *                      is sized (default 4).  Where tail units apply and the shapes allow, the ring
 *                      groups are 16 rings instead of 8 ("su_group" = 0)
 *   "su_order_bucket"  1 (default): the heading order of an integer-form launch (and the dense / scattered order of the
 *                      Cartesian one) is a one-pass stable bucket sort wherever its table of one word per (512 positions,
 *                      key) stays within 4 n + 65536 words; 0: always rocPRIM's stable sort (A/B) — the same slot list
 *   "init_device"      0: tdr_filter_initialize_particles keeps the serial host loop; 1 (default): a filter that owns its
 *                      generator in parity mode initialises on the device (tdr_k_init_particles — the same states)
 *   "init_window_words" words of the generator's stream per window of tdr_k_init_particles (a multiple of 2048, 2048 to
 *                      2^22; default 2^21; same states)
 *   "cart_init_chunk"  particles without a heading whose candidates one scoring launch of tdr_k_score_cart_init covers
 *                      (>= 1; default 4096: DESIGN.md 5.5; bounds its workspace; same results)
 * One more name, not a part of the list above (tests/test_config_table.py replays that list as it was recorded):
 * "su_full_list" — 1 (default): scan bins that hold several classes are empty to score_polar_su_kernel's assembly loop and
 * are added behind it, sector by sector, from a list (a mask word per ring group and scan row that the preparation writes),
 * each class from its plane; 0: the loop hands every four-ring step that holds such a bin to the C++ step (A/B, tests).
 * Integer sums: same bits.  Ring groups of 4, 8 or 16 rings.
 * "inject_cand_chunk" — candidates one scoring launch of tdr_filter_inject_sensor covers, in whole slots (>= 1; default
 * 65536; bounds the call's buffers; same results: "sensor resetting" below); tdr_filter_grid_search walks its list in the
 * same chunks, in whole lattice points ("pose-grid search" below). */
int64_t tdr_config_tuning(const char* name, int64_t value);
/* The rows of score_polar_su_kernel's grid for nchunks ring groups with the last k cut into q sector ranges each (tests):
 * returns the row count R = (nchunks - k') + k' q', k' = k clamped to [0, nchunks], q' = q rounded down to 1, 2, 4 or 8; for
 * 0 <= row < R also the row's ring group and its sectors [s0, s1) of the 8.  row < 0: R alone. */
int tdr_su_tail_plan(int nchunks, int k, int q, int row, int* group, int* s0, int* s1);
/* The ordering passes of an integer-form launch on their own (tests, timing): the slot list of n particles (states st,
 * capacity cap) over nb heading bins — per bin the particles whose 64 neighbours in the caller's order `perm` (NULL:
 * identity) lie within `span` map cells (span <= 0: all of them), in that order, every bin padded to whole waves with -1;
 * behind the bins the other particles (key nb; nb == 1: the Cartesian launch's two keys).  workspace: device memory of
 * tdr_k_su_order_workspace_ints(n, nb) 4-byte words (never fewer for more particles).  slots_out: tdr_k_su_order_slots(n, nb)
 * words, of which the first counts_out[2] are defined; keys_out: the n keys in the caller's order; counts_out: {padded slots
 * of the bins, particles behind them, both}.  These are device pointers; nb <= 4095.  bucket_out (host memory, may be NULL):
 * 1 when the bucket sort ordered the launch, 0 when rocPRIM's sort did ("su_order_bucket"). */
size_t tdr_k_su_order_workspace_ints(int64_t n, int nb);
int64_t tdr_k_su_order_slots(int64_t n, int nb);
int tdr_k_su_order(const float* st, int64_t cap, int64_t n, const int32_t* perm, int nb, float span, int32_t* workspace,
                   int32_t* slots_out, int32_t* keys_out, int32_t* counts_out, int* bucket_out, void* stream);
/* The ordering passes and the scan-side preparation of an integer-form scoring call on their own (tests, timing): what
 * tdr_k_score_polar_ctx runs in front of its two integer kernels, with the same arguments, on a workspace of
 * tdr_score_workspace_floats floats; `span` as in tdr_k_su_order.  The call must have an integer form (a map with compact
 * records, shapes the shift-uniform kernel takes: tdr_config_shift_uniform).  layout (host, 16 words): {rings per group G of the
 * shift-uniform layout, groups C, padded rings per direction of the preparation's grid, steps per block and blocks per
 * direction of the ray-mapped layout, block-major order 0 | 1, patch order 0 | 1, padded samples T of the ray-mapped layout,
 * bins C nb G of the shift-uniform layout, sectors S per group, words behind the counts, uniform scale 0 | 1, 0...}.  With
 * workspace == NULL only `layout` is filled.  out (host array of 9 device pointers, NULL = not wanted): [0] the uniform-scale
 * table, 2 nb nr floats (untouched without a uniform scale); [1] sample offsets [C][nb][G][2] and [2] scan descriptors
 * [C][nb][G][4] of the shift-uniform layout; [3] boxes [C][S]{min, max, min, max}; [4] sample offsets, 2 T floats, [5]
 * 16-bit descriptors, (T + 1) / 2 words, [6] radii, T / nb floats (written only with the context's factors), of the ray-mapped
 * layout; [7] the list of bins with several classes, nb nr words of which the first n_list are defined, in any order; [8] the
 * words behind the counts: {dense slots, scattered particles, both, n_list, inexact, mass bound, table is not its factors, 3
 * spare}. */
int tdr_k_score_prep(const tdr_map_desc* map, const float* tab, const float* scan_pk, int nb, int nr, float res,
                     const float* st, int64_t cap, int64_t n, int64_t n_total, const int32_t* perm, float uniform_scale,
                     float span, float* workspace, tdr_score_ctx* ctx, int64_t* layout, void* const* out, void* stream);
/* The preparation's mask of the scan bins that hold several classes (tests): after tdr_k_score_prep or a scoring call of
 * these shapes on `workspace` (with "su_full_list" on and ring groups of 4, 8 or 16 rings; otherwise the words are whatever
 * the workspace held), *words = 2 C nb words to `out` (device memory), [C][2 nb]: bit jj of word (group c, scan row i) — and
 * of word nb + i, the rows are stored twice over — says bin (i, ring c G + jj) holds several classes.  workspace or out
 * NULL: *words alone. */
int tdr_k_score_prep_full_mask(const tdr_map_desc* map, int nb, int nr, int64_t n, int64_t n_total, const float* workspace,
                               uint32_t* out, int64_t* words, void* stream);
/* Device self-test of the scoring kernels: a tiny fixed problem (160 x 160 map, 6 classes, 512 particles) scored by every
 * kernel the library has for it.  The integer-form kernels run generated, hand-scheduled assembly; their sums are exact, so
 * score_polar_su_kernel == score_polar_ray_kernel and score_cart_su_kernel == score_cart_skip_kernel == score_cart_ray_kernel
 * BIT FOR BIT, and both agree with the float kernels to rounding (3e-6).  TDR_OK, or an error whose message says which
 * pair disagrees: a toolchain that miscompiles around the generated loops fails loudly here (smoke() calls it). */
int tdr_selftest_score(void);
/* Self-test hook: out[i] = the scoring loop's coordinate rounding of x[i] clamped to [-1, limit] (== roundf). */
int tdr_k_selftest_round(const float* x, int64_t n, float limit, int32_t* out, void* stream);
/* sinf / cosf on the device are the HOST libm's, bit for bit (csrc/tdr_sincosf.h: glibc >= 2.28's double-precision
 * algorithm restated).  glibc ships two builds of it, plain and FMA-contracted, and picks one per CPU at load time;
 * tdr_libm_variant() probes the host's sinf / cosf where the two differ: 1 = fused, 0 = plain, -1 = neither (an
 * unknown libm: the kernels then use the fused form and indices derived from sin / cos are unpinned).
 * tdr_libm_force_variant(0 | 1) overrides the probe (tests), -1 returns to it.  tdr_sincosf_host evaluates the
 * restatement on the host (variant 0 | 1), tdr_k_selftest_sincos on the device with the variant in force. */
int tdr_libm_variant(void);
int tdr_libm_force_variant(int variant);
int tdr_sincosf_host(const float* x, int64_t n, int variant, float* sin_out, float* cos_out);
int tdr_k_selftest_sincos(const float* x, int64_t n, float* sin_out, float* cos_out, void* stream);
/* logf on the device is the host libm's too (csrc/tdr_logf.h; glibc's two builds agree on every argument): the
 * restatement on the host / on the device (libstdc++'s normal_distribution<float> calls it, csrc/tdr_rng.hip). */
int tdr_logf_host(const float* x, int64_t n, float* out);
int tdr_k_selftest_logf(const float* x, int64_t n, float* out, void* stream);
/* Self-test hook: out[i] = the raster kernel's atan2f(y[i], x[i]) (bit-identical to glibc's atan2f). */
int tdr_k_selftest_atan2(const float* y, const float* x, int64_t n, float* out, void* stream);

/* ---- layout helpers ------------------------------------------------------------------------------------------ */
int tdr_k_states_aos_to_soa(const tdr_state* aos, int64_t n, float* st, int64_t cap, void* stream);
int tdr_k_states_soa_to_aos(const float* st, int64_t cap, int64_t n, tdr_state* aos, void* stream);
/* Locality order: perm_out = particle indices grouped by the 4x4 px map tile of their centre (row-major tiles).
 * keys_tmp: int32[tdr_locality_tmp_ints(n, map_rows, map_cols)] scratch. */
size_t tdr_locality_tmp_ints(int64_t n, int map_rows, int map_cols);
int tdr_k_locality_order(const float* st, int64_t cap, int64_t n, int map_rows, int map_cols, int32_t* perm_out,
                         int32_t* keys_tmp, void* stream);
/* The same for windows that rotate with the particle (Cartesian scoring, top_down_map.cpp:367-389): Morton order of
 * (x, y, theta), theta quantised so that one step moves a sample `theta_radius` cells from the centre by half a cell.
 * keys_tmp: tdr_locality_pose_tmp_ints(n) int32 of device scratch, 8-byte aligned. */
size_t tdr_locality_pose_tmp_ints(int64_t n);
int tdr_k_locality_order_pose(const float* st, int64_t cap, int64_t n, int map_rows, int map_cols, float theta_radius,
                              int32_t* perm_out, int32_t* keys_tmp, void* stream);

/* =================================================================================================================
 * Handle layer: C++ host code (csrc/tdr_host_*.cpp) that owns the device memory and sequences the kernels above the way
 * the reference's classes sequence their loops.  HOST pointers in and out; one handle per reference object; one caller
 * thread per handle.  This is what the headers under include/top_down_render/ (the reference's class surface) are
 * written against.
 * ================================================================================================================= */
typedef struct tdr_map tdr_map;            /* TopDownMapPolar   (top_down_map_polar.h:6-22)  */
typedef struct tdr_renderer tdr_renderer;  /* ScanRenderer[Polar] (scan_renderer_polar.h:15-22) */
typedef struct tdr_filter tdr_filter;      /* ParticleFilter    (particle_filter.h:22-73)    */

int tdr_map_create(tdr_map** out);
void tdr_map_destroy(tdr_map* m);
/* class_maps_/class_mask_ as computeDists leaves them (top_down_map.cpp:289-326), column-major HOST arrays; also the
 * map side of TopDownMap::updateMap (:146-157).  center = map_center_. */
int tdr_map_set(tdr_map* m, const float* class_maps, const uint8_t* class_mask, int ncls, int rows, int cols,
                float resolution, int center_x, int center_y);
/* TopDownMap::updateMap(const cv::Mat&, map_center) (top_down_map.cpp:146-157) for a HOST class-index image
 * (CV_8UC1 layout): loadCompressedRasterMap + the exact distance transform of computeDists run on the device.
 * haveMap() turns true only if the map contains road (class 1), like :150-154. */
int tdr_map_set_labels(tdr_map* m, const uint8_t* label_img, int img_h, int img_w, const int32_t* flatten_lut,
                       int lut_size, int ncls, float resolution, int center_x, int center_y);
/* tdr_map_set_labels' end state, byte for byte, reached by rebuilding only what the new image changes (tdr_k_map_update_labels;
 * the host copies change in the affected tiles only).  Takes the full path (tdr_map_set_labels) itself and reports
 * *changed_cells = -1 when the map was not last set from a label image (tdr_map_set_labels or these entries), when the
 * image shape, resolution, class count or LUT differ, or when the affected tiles exceed TDR_MAP_INCR_MAX_FRACTION of
 * the map; else *changed_cells = the cells whose class changed.  A host can call it for every map message. */
int tdr_map_update_labels_incremental(tdr_map* m, const uint8_t* label_img, int img_h, int img_w,
                                      const int32_t* flatten_lut, int lut_size, int ncls, float resolution, int center_x,
                                      int center_y, int64_t* changed_cells);
/* The same for the previous label image with the rectangle [y0, y0 + h) x [x0, x0 + w) of IMAGE pixels (row 0 = top)
 * overwritten by `patch` (HOST, h x w u8, rows packed): only the rectangle is uploaded.  Needs a map last set from a
 * label image (TDR_ERR_ARG otherwise); never takes the full path. */
int tdr_map_patch_labels(tdr_map* m, const uint8_t* patch, int y0, int x0, int h, int w, int center_x, int center_y,
                         int64_t* changed_cells);
/* the map's descriptor as the scoring kernels see it (device pointers owned by the map; read-only) */
int tdr_map_get_desc(const tdr_map* m, tdr_map_desc* out);
int tdr_map_sample_pts_polar(tdr_map* m, int nb, int nr, float ang_res);                 /* top_down_map_polar.cpp:7-19 */
int tdr_map_polar_shape(const tdr_map* m, int* nb, int* nr);   /* the shape of the last samplePtsPolar (0, 0 before) */
/* The Cartesian window (rows = y, cols = x) a Cartesian filter scores against (tdr_filter_create_cart): the shape of the
 * images TopDownMap::getLocalMap is asked for; Python's TopDownMap.setWindow.  rows, cols >= 1.  The shape stays with the
 * handle across map updates.  tdr_map_window_shape: the last one set (0, 0 before). */
int tdr_map_set_window(tdr_map* m, int rows, int cols);
int tdr_map_window_shape(const tdr_map* m, int* rows, int* cols);
int tdr_map_info(const tdr_map* m, int* ncls, int* rows, int* cols, float* resolution, int* have_map);
int tdr_map_center(const tdr_map* m, int* center_x, int* center_y);                      /* mapCenter(), top_down_map.h:72 */
/* getLocalMap (polar != 0: top_down_map_polar.cpp:21-53 with scale_or_rot = scale and the table of
 * tdr_map_sample_pts_polar, rows/cols ignored; else top_down_map.cpp:429-459 with scale_or_rot = rot).
 * dists_out HOST [ncls][rows*cols], mask_out HOST [rows*cols]. */
int tdr_map_local_map(tdr_map* m, int polar, float cx, float cy, float scale_or_rot, float res, int rows, int cols,
                      float* dists_out, uint8_t* mask_out);
int tdr_map_classes_at_point(const tdr_map* m, int px, int py, uint32_t* class_bits);    /* top_down_map.cpp:159-170 */
/* ActiveLocalizer::getBestRelPos (src/active_localizer.cpp:44-82) on the map's table (tdr_map_sample_pts_polar; the
 * reference's local maps are 100 x 25): preds HOST [K][3] = {x, y, theta} of the pose hypotheses (the mixture's means).
 * best_rel_pos = {distance, direction} of the displacement whose local maps differ most, *best_diff that mean difference
 * (0 and {0, 0} when nothing beats 0 — e.g. one hypothesis: the reference's 0 / 0 never wins). */
int tdr_map_best_rel_pos(tdr_map* m, const float* preds, int K, float best_rel_pos[2], float* best_diff);
/* getLocalGeoMap (top_down_map_polar.cpp:55-76 / top_down_map.cpp:461-481): the same window gathered from the two
 * geometric layers geo_maps_ — [0] distance to the nearest cell WITHOUT a geometric class (flattened class >= 3), [1]
 * to the nearest cell WITH one (getGeoRasterMap :410-427 + computeDists), as tdr_map_set derives them; after
 * tdr_map_set_labels both layers are the constant 1 the reference's updateMap path leaves them at (:126-133).
 * dists_out HOST [2][rows*cols]. */
int tdr_map_local_geo_map(tdr_map* m, int polar, float cx, float cy, float scale_or_rot, float res, int rows, int cols,
                          float* dists_out);
/* The reference's on-disk map cache (src/top_down_map.cpp:226-286; .eig = 2 x int64 shape + column-major scalars,
 * top_down_map.h:29-50): cached_data.txt, class_map<i>.eig, geo_map<i>.eig, class_mask.eig under cache_dir (NULL =
 * $HOME/.ros/xview_cache).  load: *loaded = 1 and the map is set when the cache's (map_path, num_classes, resolution)
 * match like loadCacheMetaData, else *loaded = 0.  save writes the files of the map the handle holds. */
int tdr_map_load_cache(tdr_map* m, const char* cache_dir, const char* map_path, int num_classes, float resolution,
                       int center_x, int center_y, int* loaded);
int tdr_map_save_cache(tdr_map* m, const char* cache_dir, const char* map_path);
/* The raster cache (TopDownMap::saveRasterizedMaps / loadRasterizedMaps, src/top_down_map.cpp:197-224): a directory of
 * class<i>.png — 8-bit greyscale, 0 inside class i and 255 elsewhere, stored flipped like the reference stores them — read
 * and written over zlib (no OpenCV).  load = the constructor's path for such a directory (:44-58): rasters -> geometric
 * layers -> distance transforms, on the device; the map takes the images' shape. */
int tdr_map_save_rasters(tdr_map* m, const char* dir);
/* the codec on its own (host only): 8-bit greyscale, non-interlaced PNG; px row-major, row 0 = top.  read: px_out holds
 * `capacity` bytes, *w / *h are set even when the image does not fit (then TDR_ERR_ARG). */
int tdr_png_read_gray8_host(const char* path, uint8_t* px_out, int64_t capacity, int* w, int* h);
int tdr_png_write_gray8_host(const char* path, const uint8_t* px, int w, int h);
int tdr_map_load_rasters(tdr_map* m, const char* dir, int num_classes, float resolution, int center_x, int center_y);
/* The static vector map: TopDownMap::loadSvg + getRasterMap + getClasses (src/top_down_map.cpp:22-31,
 * 66-110, 328-365, 391-408), then the constructor's geometric layers and computeDists (:48-58) through the same device
 * ingest as tdr_map_load_rasters.
 *
 * tdr_svg_parse_host (host only, no device needed): reads an SVG like the reference's nanosvg call
 * (nsvgParseFromFile(path, "px", 96)) and returns what loadSvg keeps of it: size_out = the image's float width / height
 * (after units and viewBox; H_f), and per subpath of every shape one polygon — its fill key (nanosvg's 0xBBGGRR colour
 * & 0xFFFFFF; 0 for fill="none" and for an absent fill; TDR_SVG_NO_KEY for a gradient), the vertex range
 * [offsets_out[p], offsets_out[p+1]) and vertices_out[v] = {x, H_f - y}: the start point and every segment's end point
 * but the last (so a closed subpath loses the copy of its start, an open one its real last point).  Polygons come in
 * document order (the reference reverses the subpaths of a shape; the fill does not depend on the order).
 * Two calls: with keys_out == offsets_out == verts_out == NULL only the counts are written to *n_poly / *n_vert; then
 * with arrays of at least those sizes (*n_poly / *n_vert = their capacities; offsets_out holds n_poly + 1 entries).
 * Supported: svg (width / height in px pt pc mm cm in %, viewBox, preserveAspectRatio), g, path (all commands),
 * rect (rx / ry), circle, ellipse, line, polyline, polygon, transform (matrix translate scale rotate skewX skewY),
 * fill / style= / inheritance from g, defs (skipped), gradients.  Not: strokes, <style> sheets, <use>, text.  A file
 * without a usable size, a non-finite coordinate or more than 2^27 path points: TDR_ERR_ARG. */
#define TDR_SVG_NO_KEY 0xFFFFFFFFu
int tdr_svg_parse_host(const char* path, float size_out[2], int64_t* n_poly, int64_t* n_vert, uint32_t* keys_out,
                       int64_t* offsets_out, float* verts_out);
/* getRasterMap + getClasses for polygons from anywhere, then the ingest (handle layer, HOST arrays): polygon p has the
 * vertices verts[offsets[p] .. offsets[p+1]) ({x, y} pairs, offsets non-decreasing from 0) and the flattened class
 * poly_class[p] (polygons of a class outside [0, num_classes) are skipped).  The map is int(height / resolution) x
 * int(width / resolution) cells sampled at samplePts(center = (width / 2, height / 2), rot 0) (top_down_map.cpp:391-408);
 * a cell is inside a polygon when the even-odd test of :336-347 says so, bit for bit (f32, no FMA, IEEE division).
 * exclusive[n_excl] = params_.exclusive_classes (ids in [0, num_classes)): where a listed class c lies, every listed
 * class u < c is cleared (:356-365).  planes_out: NULL, or HOST [num_classes][rows * cols] u8, column-major, the class
 * planes before the distance transform (0 inside the class, 1 elsewhere).  center = map_center_.  Every argument is
 * checked before any device work.  The fill relies on both sample tables rising (LinSpaced over a symmetric range always
 * does); the host checks it and returns TDR_ERR_ARG if one ever decreased, instead of falling back to a linear count. */
int tdr_map_load_polygons(tdr_map* m, const float* verts, const int64_t* poly_offsets, const int32_t* poly_class,
                          int64_t n_poly, int width, int height, int num_classes, const int32_t* exclusive, int n_excl,
                          float resolution, int center_x, int center_y, uint8_t* planes_out);
/* The fill alone, for callers that ingest the planes themselves: the same arguments and checks, planes_out required
 * (HOST [num_classes][rows * cols], column-major, 0 inside / 1 elsewhere); needs a device, no handle. */
int tdr_polygon_planes(const float* verts, const int64_t* poly_offsets, const int32_t* poly_class, int64_t n_poly,
                       int width, int height, int num_classes, const int32_t* exclusive, int n_excl, float resolution,
                       uint8_t* planes_out);
/* The constructor's SVG branch (:22-31): parse (tdr_svg_parse_host), class assignment like loadSvg (:77-103: LUT index
 * cls collects the polygons whose key is fill_keys[cls] = c[0] << 16 | c[1] << 8 | c[2] of
 * SemanticColorLut::unpackColor(ind2Color(cls)), into flattened class flatten_lut[cls]; entries outside
 * [0, num_classes) are skipped), then tdr_map_load_polygons with width / height = int of the image's float size.  A file
 * that does not parse leaves the handle as it was. */
int tdr_map_load_svg(tdr_map* m, const char* path, const uint32_t* fill_keys, const int32_t* flatten_lut, int lut_size,
                     int num_classes, const int32_t* exclusive, int n_excl, float resolution, int center_x, int center_y);
/* The static colour raster map: the constructor's branch for a .png / .jpg map_path
 * (src/top_down_map.cpp:32-42, then :48-63): cv::imread, color2Ind, loadCompressedRasterMap, then the geometric layers
 * derived from the classes and computeDists on both, have_map = true even for a map without road (:63; unlike
 * tdr_map_set_labels).  The map is int(h / resolution) x int(w / resolution) cells.
 *
 * tdr_png_read_color_host (host only, no device needed): the BGR8 image cv::imread(path) gives for a PNG: every colour
 * type, bit depth and interlace method; palette expanded (tRNS ignored), grey below 8 bits scaled to 8 bits and copied into
 * three channels, alpha dropped, 16-bit samples cut to their high byte, no gamma or colour-space conversion; row 0 = top.
 * bgr_out holds `capacity` bytes (3 * w * h needed); *w / *h are set even when the image does not fit (then TDR_ERR_ARG),
 * so bgr_out = NULL is a size query.  Bad CRCs, truncation, a missing or misplaced PLTE, unknown critical chunks and
 * headers announcing more pixels than the data can hold are refused.  eXIf is ignored (cv::imread may rotate by it).
 *
 * tdr_map_load_color_image: from a HOST BGR image (e.g. a caller's own cv::imread, which also covers .jpg maps);
 * fill_keys / flatten_lut as for tdr_k_map_from_color (HOST, lut_size <= 256), resolution >= 0.2 (the distance window).
 * tdr_map_load_color_png: tdr_png_read_color_host, then the same.  Every argument is checked and the file read before any
 * device work: a failed read or a refused argument leaves the handle as it was. */
int tdr_png_read_color_host(const char* path, uint8_t* bgr_out, int64_t capacity, int* w, int* h);
int tdr_map_load_color_image(tdr_map* m, const uint8_t* bgr, int img_h, int img_w, const uint32_t* fill_keys,
                             const int32_t* flatten_lut, int lut_size, int num_classes, float resolution, int center_x,
                             int center_y);
int tdr_map_load_color_png(tdr_map* m, const char* path, const uint32_t* fill_keys, const int32_t* flatten_lut,
                           int lut_size, int num_classes, float resolution, int center_x, int center_y);

int tdr_renderer_create(const int32_t* flatten_lut256, tdr_renderer** out);              /* scan_renderer.cpp:3-5 */
void tdr_renderer_destroy(tdr_renderer* r);
/* renderSemanticTopDown: polar != 0 -> scan_renderer_polar.cpp:83-109 (rows = theta bins, cols = range bins),
 * else scan_renderer.cpp:55-78.  imgs_out: HOST [ncls][rows*cols] column-major, or NULL to keep the render on the
 * device for tdr_filter_update. */
int tdr_renderer_render(tdr_renderer* r, int polar, const float* pts, int stride, int ioff, int64_t n, float res,
                        float ang_res, int ncls, int rows, int cols, float* imgs_out);

/* renderGeometricTopDown (scan_renderer_polar.cpp:6-81 / scan_renderer.cpp:7-53): HOST organised cloud (element
 * idy*width + idx; pcl clouds: width = cloud->width, height = cloud->height), imgs_out HOST [2][rows*cols]. */
int tdr_renderer_render_geo(tdr_renderer* r, int polar, const float* pts, int stride, int64_t width, int64_t height,
                            float res, float ang_res, int rows, int cols, float* imgs_out);

/* ---- several GPUs: one process (rank) per GPU, particles partitioned contiguously by rank -------------
 * A tdr_comm carries the three exchange steps of a sharded filter — broadcast of the rasterised scan from rank 0,
 * all-gather of {raw weight, last_dist}, all-gather of the state planes — over RCCL (xGMI), called directly on the
 * filter's stream, or over functions the caller supplies (MPI, a test double).  Every rank then computes the weight
 * statistics and the order-exact running sum on the same gathered arrays, so an N-rank filter equals the 1-rank filter
 * bit for bit (tests/test_sharded_handle.py).  The reference has no counterpart: it is one CPU process. */
#define TDR_COMM_ID_BYTES 128
typedef struct tdr_comm tdr_comm;
typedef struct tdr_comm_ops {   /* device pointers; enqueue on `stream` (a hipStream_t) or complete before returning */
  void* ctx;
  int (*all_gather)(void* ctx, const void* send_dev, void* recv_dev, size_t bytes_per_rank, void* stream);
  int (*broadcast)(void* ctx, void* buf_dev, size_t bytes, int root, void* stream);
} tdr_comm_ops;
/* RCCL transport: rank 0 makes the id (ncclGetUniqueId) and hands its 128 bytes to the other ranks by any means; every
 * rank then calls create_rccl with its HIP device current (ncclCommInitRank).  librccl.so is loaded on first use. */
int tdr_comm_rccl_unique_id(void* id_out128);
int tdr_comm_create_rccl(int world_size, int rank, const void* unique_id128, tdr_comm** out);
int tdr_comm_create(int world_size, int rank, const tdr_comm_ops* ops, tdr_comm** out);
void tdr_comm_destroy(tdr_comm* c);
int tdr_comm_world(const tdr_comm* c);
int tdr_comm_rank(const tdr_comm* c);
int tdr_comm_all_gather(tdr_comm* c, const void* send_dev, void* recv_dev, size_t bytes_per_rank, void* stream);
int tdr_comm_broadcast(tdr_comm* c, void* buf_dev, size_t bytes, int root, void* stream);
/* A filter whose particles are sharded over comm's ranks: n_max (the GLOBAL maximum) and every particle count must be
 * multiples of the world size; every rank makes the same calls with the same arguments (same seed: the host generator
 * is replicated), each on its own map handle holding the same map.  set_states takes the GLOBAL array and keeps this
 * rank's slice; get_states / get_raw_weights / get_last_dist / get_resample_indices return this rank's slice
 * (tdr_filter_num_local entries, indices global); get_weights, mean_cov, scale, num_particles are global and identical
 * on every rank.  tdr_filter_update: ranks other than 0 may pass scan_imgs == NULL and renderer == NULL — the packed scan
 * of rank 0 is broadcast. */
int tdr_filter_create_sharded(tdr_map* map, int n_max, const tdr_filter_params* fp, uint32_t seed, tdr_comm* comm,
                              tdr_filter** out);
int64_t tdr_filter_num_local(const tdr_filter* f);

/* seed: the reference seeds its std::mt19937 from std::random_device (src/particle_filter.cpp:4-5), i.e. not
 * reproducibly.  seed == 0 stands for that case: propagate's noise is then drawn on the device (counter-based, 4 us).
 * seed != 0: every draw comes from std::mt19937(seed) in the reference's order, propagate's 4N normals included (host
 * code, ~35 ns per draw) — the mode the parity tests use.  tdr_filter_configure changes the mode afterwards. */
int tdr_filter_create(tdr_map* map, int n_max, const tdr_filter_params* fp, uint32_t seed, tdr_filter** out);
/* A filter whose scoring stage is the CARTESIAN one (tdr_k_score_cart: BASELINE config 4).  The map needs a window
 * (tdr_map_set_window), else TDR_ERR_ARG.  It is an ordinary tdr_filter:
 *  - tdr_filter_update / tdr_filter_compute_weights read HOST [ncls][rows*cols] column-major images of the window's shape,
 *    or a renderer's last CARTESIAN render of that shape (tdr_renderer_render with polar == 0); they order the particles
 *    with tdr_k_locality_order_pose at theta_radius = (rows + cols) / 16, run the heading search
 *    (tdr_k_score_cart_init) while a particle may lack a heading — a cold start, init_pos_deg_theta = inf: the first
 *    update — then tdr_k_score_cart, and continue through the same statistics, running sum, resample, max-likelihood and
 *    pose-statistics stages as a polar filter;
 *  - propagate, the random stream, particle initialisation, set_states / get_states, mean_cov, freeze-scale, GMM /
 *    adaptive count and map updates work as on a polar filter; tdr_batch_pose accepts it (it does not score).
 * Refused with TDR_ERR_ARG, the filter unchanged: tdr_filter_update_geo (there is no Cartesian geometric cost), a Cartesian
 * filter in tdr_batch_step, and sharding (there is no tdr_filter_create_cart_sharded). */
int tdr_filter_create_cart(tdr_map* map, int n_max, const tdr_filter_params* fp, uint32_t seed, tdr_filter** out);
void tdr_filter_destroy(tdr_filter* f);
/* parity_rng: propagate consumes host std::mt19937 normals in the reference's order; 0 = device RNG.
 * locality_every: > 0 processes particles in Morton order of their map position (default 1; results unchanged). */
int tdr_filter_configure(tdr_filter* f, int parity_rng, int locality_every);
/* particle_filter.cpp:19-84.  The loop keeps tdr_init_particles_count(fp, n_max) particles; a filter sharded over W ranks
 * then keeps n - n % W of them (the first ones), so every rank holds the same count.  A filter that owns its generator in
 * parity mode (seed != 0, no tdr_filter_share_rng) draws on the device (tdr_rng_pipe_init_particles): the generator stays
 * there, each rank runs the whole chain and keeps its own slice.  A generator shared with the caller, and
 * tdr_config_tuning("init_device", 0), keep the host loop.  Same states either way. */
int tdr_filter_initialize_particles(tdr_filter* f);
int tdr_filter_set_states(tdr_filter* f, const tdr_state* states, int64_t n);
int tdr_filter_get_states(tdr_filter* f, tdr_state* out, int64_t n);
int tdr_filter_propagate(tdr_filter* f, float tx, float ty, float omega);                /* particle_filter.cpp:86-92 */
/* particle_filter.cpp:94-189.  scan_imgs: HOST [ncls][nb*nr] images or NULL (= renderer's last render, no host round
 * trip), (nb, nr) = tdr_map_polar_shape — the caller checks its images against it, ncls*nb*nr floats are read;
 * n_target < 0 keeps the particle count (explicit input of the adaptive count :151-157).  A filter sharded over W ranks
 * keeps the same number of particles on every rank: n_target is rounded DOWN to a multiple of W (at least W), so a W-rank
 * filter asked for 70 particles at W = 8 resamples 64 and equals, bit for bit, the one-rank filter asked for 64. */
int tdr_filter_update(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, float res, int64_t n_target);
/* The same with the geometric images top_down_geo (HOST [2][nb*nr]) entering the score (tdr_k_score_polar_geo); the
 * reference passes them to update() too but its score ignores them.  Not available on a sharded filter. */
int tdr_filter_update_geo(tdr_filter* f, const float* scan_imgs, const float* geo_imgs, float res, int64_t n_target);
int tdr_filter_get_weights(tdr_filter* f, float* out, int64_t n);
/* The per-particle surface of StateParticle (include/top_down_render/state_particle.h:42-53) on a filter:
 * computeWeight for every particle without statistics / resampling (state_particle.cpp:157-219) and its result
 * (weight(), :55), lastDist(), propagate with the caller's scale_freeze flag (:57-78), the constructor's draw of one
 * particle (:3-49), and the generator shared with the caller (state_particle.h:61-64: `mt19937` is a std::mt19937* of
 * this library's libstdc++, not owned; the filter then consumes it in the reference's draw order). */
int tdr_filter_compute_weights(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, float res);
int tdr_filter_get_raw_weights(tdr_filter* f, float* out, int64_t n);
int tdr_filter_get_last_dist(tdr_filter* f, float* out, int64_t n);
/* scale_freeze == 0 gives every particle's scale a draw of its own, on a frozen or fixed-scale filter too: the filter then
 * no longer treats the scales as one value (the uniform_scale shortcut of tdr_k_score_polar), and the next score reads
 * each particle's own scale.  The frozen flag itself (tdr_filter_is_scale_frozen) is the caller's business and stays. */
int tdr_filter_propagate_freeze(tdr_filter* f, float tx, float ty, float omega, int scale_freeze);
int tdr_filter_init_one(tdr_filter* f);
int tdr_filter_share_rng(tdr_filter* f, void* mt19937);
int tdr_filter_get_resample_indices(tdr_filter* f, int32_t* out, int64_t n);
/* about_max == 0: meanLikelihood + computeMeanCov (:191-220); != 0: maxLikelihood + computeCov (:222-236). */
int tdr_filter_mean_cov(tdr_filter* f, int about_max, float state[4], float cov[16]);
int tdr_filter_freeze_scale(tdr_filter* f);                                              /* :343-357 */
int tdr_filter_is_scale_frozen(const tdr_filter* f);
float tdr_filter_scale(tdr_filter* f);                                                   /* :359-367 */
int64_t tdr_filter_num_particles(const tdr_filter* f);                                   /* :369-371 */
int tdr_filter_update_map(tdr_filter* f, const float* class_maps, const uint8_t* class_mask, int ncls, int rows, int cols,
                          float resolution, int center_x, int center_y);                 /* :320-341 */
int tdr_filter_update_map_labels(tdr_filter* f, const uint8_t* label_img, int img_h, int img_w,
                                 const int32_t* flatten_lut, int lut_size, int ncls, float resolution, int center_x,
                                 int center_y);                                          /* :320-341, cv::Mat form */
/* tdr_filter_update_map_labels through tdr_map_update_labels_incremental / tdr_map_patch_labels: the map is rebuilt
 * where it changed, then the particles shift by the centre's move (or are initialised) exactly as there.  Filters that
 * share the map may each call it: only the first call changes the map, the others find 0 changed cells. */
int tdr_filter_update_map_labels_incremental(tdr_filter* f, const uint8_t* label_img, int img_h, int img_w,
                                             const int32_t* flatten_lut, int lut_size, int ncls, float resolution,
                                             int center_x, int center_y, int64_t* changed_cells);
int tdr_filter_patch_map_labels(tdr_filter* f, const uint8_t* patch, int y0, int x0, int h, int w, int center_x,
                                int center_y, int64_t* changed_cells);
/* ---- adaptive particle count from a Gaussian mixture (src/particle_filter.cpp:151-157, 245-318) ---- */
/* out (device, [num][3] floats): mlState().head<3>() = {x, y, theta} of particle min(n-1, i*n/num) (:262-266). */
int tdr_k_sample_ml_states(const float* st, int64_t cap, int64_t n, int num, float* out, void* stream);
/* Deterministic EM fit of k full-covariance Gaussians to m samples of 4 doubles (host code, tdr_gmm.cpp; the
 * reference uses cv::ml::EM, randomly initialised: parity unpinned).  weights [k], means [k][4], covs [k][4][4]. */
int tdr_gmm_fit_host(const double* samples, int m, int k, int max_iter, double* weights, double* means, double* covs,
                     double* mean_loglik);
/* computeGMM's search for the cluster count around *num_gaussians_io (:259, 276-297) and the conversion of the clusters
 * to means [k][3] = {x, y, atan2} / covs [k][9] (:303-312).  samples [m][4] = {x, y, 50 cos theta, 50 sin theta}. */
int tdr_gmm_select_host(const double* samples, int m, int64_t num_particles, int* num_gaussians_io, int max_k,
                        float* means_out, float* covs_out);
/* num_particles_ of :151-157 from the clusters' covariances. */
int64_t tdr_adaptive_count_host(const float* covs, int k, int64_t last_count, int64_t max_count);
/* Handle layer: computeGMM (:252-318) on the filter's current particles (synchronous; the reference runs it in a
 * detached thread once per second), getGMM (:238-243), and the count of :151-157 from the stored clusters
 * (n_target for tdr_filter_update).  max_k bounds the arrays passed to get_gmm. */
#define TDR_GMM_MAX_K 32
int tdr_filter_compute_gmm(tdr_filter* f);
int tdr_filter_get_gmm(tdr_filter* f, int max_k, int* k_out, float* means, float* covs);
int64_t tdr_filter_adaptive_count(tdr_filter* f);
/* Hooks for tests and drivers (the node loop needs none of them).  num_gaussians_ (:7): the count the next computeGMM
 * searches around — 1 at creation, then what the last one chose; the setter lets a test or a timing tool start a search
 * anywhere.  step_count: the updates the filter has made (computeGMM, on the host or the device, leaves it alone). */
int tdr_filter_num_gaussians(const tdr_filter* f);
int tdr_filter_set_num_gaussians(tdr_filter* f, int num_gaussians);
int64_t tdr_filter_step_count(const tdr_filter* f);

/* ---- the same fit on the device (csrc/tdr_gmm.hip) ----
 * tdr_gmm_fit_host statement for statement, every sum in the host's order, in double: the device's exp / log are the
 * only operations that may round differently.  One workgroup per fit, m <= 1000, k <= TDR_GMM_MAX_K, k <= m.
 * A fit's output `out` is tdr_gmm_out_doubles(k) = 21 k + 2 doubles: w[k], mu[k][4], cov[k][4][4], the mean
 * log-likelihood, the E-steps made.  `workspace` holds the responsibilities: tdr_gmm_workspace_bytes(m, k). */
typedef struct tdr_gmm_job {
  const double* samples;   /* [m][4] device */
  int32_t m, k, max_iter, pad;
  double* out;             /* [21 k + 2] device */
  double* workspace;       /* tdr_gmm_workspace_bytes(m, k) device, the job's own */
} tdr_gmm_job;
/* One filter's cluster-count decision (:276-297): cand[0] = the fit at k, cand[1] = at k + 1 or NULL, cand[2] = at k - 1 or
 * NULL (each a tdr_gmm_job's out).  dir = 0; +1 if cand[1] and ll + 0.3 < ll_up; then -1 if cand[2] and ll - 0.3 < ll_down
 * (the later test wins, as in tdr_gmm_select_host).  record: TDR_GMM_RECORD_DOUBLES doubles — the chosen count, its mean
 * log-likelihood, then per cluster {mu[4], cov(0,0), cov(0,1), cov(1,0), cov(1,1)}. */
typedef struct tdr_gmm_pick_job {
  const double* cand[3];
  int32_t k, pad;
  double* record;
} tdr_gmm_pick_job;
#define TDR_GMM_RECORD_DOUBLES (2 + 8 * TDR_GMM_MAX_K)
size_t tdr_gmm_workspace_bytes(int m, int k);
int tdr_gmm_out_doubles(int k);
/* ml3 [num][3] floats {x, y, theta} (tdr_k_sample_ml_states) -> samples_out [num][4] doubles {x, y, 50 cos theta,
 * 50 sin theta}, bit for bit tdr_filter_compute_gmm's host conversion (float cosf / sinf, float product, widened).
 * For theta = +-inf / NaN the kernel writes the NaN bit patterns an x86-64 glibc host produces (the negative default NaN
 * for an infinity, the quieted argument for a NaN): on a host of another architecture the host call and the device call
 * may then store different NaN bits for such a heading (both are NaN; finite headings do not depend on the host). */
int tdr_k_gmm_samples(const float* ml3, int num, double* samples_out, void* stream);
/* The device twin of tdr_gmm_fit_host: one job, passed to the kernel by value; an asynchronous launch like every tdr_k_*. */
int tdr_k_gmm_fit(const double* samples, int m, int k, int max_iter, double* out, double* workspace, void* stream);
/* n_jobs fits in one launch, one workgroup each; jobs_dev is a device array.  A job with bad sizes writes nothing. */
int tdr_k_gmm_fit_jobs(const tdr_gmm_job* jobs_dev, int n_jobs, void* stream);
int tdr_k_gmm_pick(const tdr_gmm_pick_job* jobs_dev, int n, void* stream);
/* The fits tdr_gmm_select_host makes before it decides: cand[0] = k = clamp(min(n / 20 + 1, num_gaussians), 1,
 * min(max_k, m)); cand[1] = k + 1 if k * 50 < n and k + 1 <= min(max_k, m), else 0; cand[2] = k - 1 if k > 1, else 0. */
int tdr_gmm_candidates_host(int num_gaussians, int64_t num_particles, int m, int max_k, int cand[3]);
/* tdr_filter_compute_gmm with the fit on the device: the same samples (a sharded filter gathers like there and every rank
 * runs the same fit), the candidate fits and the pick on the filter's stream, one read-back of the record, the host's
 * conversion to means / covs.  Stores where tdr_filter_compute_gmm stores, so get_gmm, adaptive_count and the particle
 * picture see it.  Reads the particle states only; a filter with 0 particles is left untouched. */
int tdr_filter_compute_gmm_device(tdr_filter* f);
/* tdr_filter_compute_gmm_device of k filters (polar or Cartesian, on any maps): the samples, every candidate fit and
 * the picks are ONE launch each on `stream`, with one table upload and one read-back.  Each filter ends bit for bit where
 * its own call leaves it.  Refused before any filter changes: null entries, duplicates, sharded filters. */
int tdr_batch_compute_gmm(tdr_filter* const* filters, int k, void* stream);

/* ---- batched filters: many filters on one map stepped together (csrc/tdr_batch.hip) ------------------------------------
 * tdr_batch_step = for every filter k: tdr_filter_propagate(filters[k], in[k].tx, in[k].ty, in[k].omega) followed by
 * tdr_filter_update(filters[k], in[k].scan_imgs, in[k].renderer, in[k].res, in[k].n_target) — every filter ends BIT FOR BIT
 * where those calls leave it (states, raw and normalised weights, statistics, resample indices, max-likelihood state, the
 * generator's position in its stream).  Filters that qualify run on `stream` (a hipStream_t, NULL = the default stream),
 * one launch per stage for the whole batch — propagate, scoring, statistics, running sum, resample — when
 * they are not sharded, draw from the device generator in parity mode
 * (a seeded filter whose generator is its own), have at most 32 768 particles, no particle still without a heading (the
 * 40-rotation search of the first update) and a scoring launch of the float form (small windows and filters, see
 * tdr_config_shift_uniform).  With tdr_config_tuning("batch_init_search", 1) a filter that may still hold a particle
 * without a heading — a cold start (init_pos_deg_theta = inf), or for ever a gated filter (force_on_map, fixed_scale < 0) —
 * joins the batch too: its search takes the pass its standalone call takes (tdr_config_init_mfma) as part of the batch's
 * scoring stage, one launch per pass kind for all such filters, the map's half records built once per set of class weights
 * instead of once per filter.  Every other filter runs its standalone calls inside the same tdr_batch_step, so a batch is
 * always correct.  Each filter's own stream and generator streams are ordered against `stream` with events.
 * Refused with TDR_ERR_ARG before any device work (no filter changes): k < 1, a null array or filter, a filter twice,
 * filters on different maps, a map without samplePtsPolar, an input without a scan, a render whose shape is not the map's.
 * scan_imgs: HOST [ncls][nb*nr] images as for tdr_filter_update, or NULL with `renderer` (its last render, on the device).
 * tdr_batch_last_stats: how many filters of this thread's last tdr_batch_step took the batched path / their standalone calls. */
typedef struct tdr_batch_input {
  const float* scan_imgs;
  const tdr_renderer* renderer;
  float res;
  float tx, ty, omega;
  int64_t n_target;
} tdr_batch_input;
int tdr_batch_step(tdr_filter* const* filters, int k, const tdr_batch_input* in, void* stream);
int tdr_batch_last_stats(int* batched, int* standalone);

/* ---- batched node loop: the render and the pose statistics of many robots at once (csrc/tdr_batch_loop.hip) ------------
 * tdr_batch_render_polar = for every i: tdr_renderer_render(r[i], 1, clouds[i].pts, clouds[i].stride, clouds[i].ioff,
 * clouds[i].n, clouds[i].res, ang_res, ncls, nb, nr, NULL) — each renderer ends holding the same bits on the device
 * (have_scan, shape), ready as a tdr_batch_step / tdr_filter_update input — with one upload of all clouds (staged in a
 * per-thread pinned buffer) and one keys launch + one raster launch on `stream` (shapes the standalone raster bins
 * without keys take its launch per renderer).  No host wait: readers of a renderer's previous render and readers of this
 * one are ordered with events.  Refused with TDR_ERR_ARG before any device work: k < 1, a null array or renderer, a
 * renderer twice, a cloud with n < 0 or n > 0 and null pts, stride < 3, ioff outside [0, stride), res <= 0, ang_res <= 0,
 * a shape outside 1..TDR_MAX_CLASSES x >= 1 x >= 1, ncls * nb * 4 > 152 KB.  pts: HOST.
 * tdr_renderer_get_render: HOST copies of the last render ([ncls][rows*cols] column-major images and the packed records,
 * [rows*cols][tdr_rec_floats(ncls)]); either pointer may be NULL; TDR_ERR_ARG without a render.
 * tdr_batch_pose = for every i: tdr_filter_mean_cov(f[i], 0, mean, cov) and tdr_filter_scale(f[i]), bit for bit, with one
 * launch set for all filters on `stream` (after each filter's own stream), one device-to-host copy and one wait; it
 * fills each filter's mean / covariance cache, so a following tdr_filter_mean_cov(f, 0, ...) / tdr_filter_scale does no
 * device work.  n = 0 gives zeros; sharded filters make their standalone calls inside.  Refused with TDR_ERR_ARG before
 * any device work: k < 1, a null array or filter, a filter twice, filters on different maps. */
typedef struct tdr_batch_cloud {
  const float* pts;
  int stride, ioff;
  int64_t n;
  float res;
} tdr_batch_cloud;
int tdr_batch_render_polar(tdr_renderer* const* r, int k, const tdr_batch_cloud* clouds, float ang_res, int ncls, int nb,
                           int nr, void* stream);
int tdr_renderer_get_render(const tdr_renderer* r, float* imgs_out, float* pk_out);
typedef struct tdr_pose_stats {
  float mean[4];
  float cov[16];
  float scale;
  int64_t n;
} tdr_pose_stats;
int tdr_batch_pose(tdr_filter* const* f, int k, tdr_pose_stats* out, void* stream);

/* ---- the particle picture: the node's map_viz image on the device (src/particle_filter.cpp:373-423, call site
 * src/top_down_render.cpp:430-449) ----------------------------------------------------------------
 * A DEFINITION, parity unpinned (like N3): OpenCV's anti-aliased thick lines blend in particle order, which no parallel
 * drawing reproduces.  Kept from the reference: where things are drawn, the colours, the primitives, the integer
 * conversions, the order of the layers.  Replaced: the coverage rule of a thick anti-aliased line.
 *   Images are BGR8 [H][W][3]; pixels are integers, x to the right, y down, origin top-left.
 *   Segment A -> B (integer endpoints, half width 1 = the reference's thickness 2) covers pixel P, with u = B - A,
 *     w = P - A, L = u.u, d = u.w:  L = 0 or d <= 0: |P - A|^2 <= 1;  d >= L: |P - B|^2 <= 1;  else (ux wy - uy wx)^2 <= L.
 *   Arrow(p1, p2) (cv::arrowedLine, tipLength 0.3): the shaft p1 -> p2 and two tips q -> p2,
 *     q = (lrint(p2.x + tip cos(ang +- pi/4)), lrint(p2.y + tip sin(ang +- pi/4))), tip = sqrt(|p1 - p2|^2) * 0.3,
 *     ang = atan2(p1.y - p2.y, p1.x - p2.x); double arithmetic on the host's libm, lrint rounds half to even.
 *   Disc(c): the 21 pixels with dx^2 + dy^2 <= 5 (a filled radius-2 cv::circle).
 *   float -> int is x86's truncating conversion: INT_MIN for NaN and for values outside [-2^31, 2^31).
 *   Layers, later over earlier:
 *     1 the background;
 *     2 particle arrows (0,0,255): float32 without contraction x = dx_m scale + init_x_px, y = dy_m scale + init_y_px,
 *       pt = ((int)x, (int)((float)H - y)); inside = !(pt.x < 0 || pt.x > W || pt.y < 0 || pt.y > H) (the reference's >:
 *       x = W is inside, its arrow clipped); an inside particle with a finite theta draws Arrow(-dir, dir) moved to pt,
 *       dir = ((int)(cosf(theta) 5), (int)(-sinf(theta) 5)), cosf / sinf the host libm's (csrc/tdr_sincosf.h); a
 *       non-finite theta draws nothing (the reference overflows an int there);
 *     3 border dots (0,255,0): a particle that is not inside draws Disc(clamp(pt.x, 5, W - 5), clamp(pt.y, 5, H - 5)).
 *       Dots lie OVER arrows here; in the reference the two overwrite each other in particle order;
 *     4 mixture and best particle (255,0,0): per component of the last computeGMM, with particle_viz.h's arithmetic (its
 *       closed-form eigen-decomposition, its stop at the first component that is not PSD), the closed polyline through
 *       the 72 vertices (lrint(cx + a cos t cos phi - b sin t sin phi), lrint(cy + a cos t sin phi + b sin t cos phi)),
 *       t = k (pi / 36), (a, b) = 2 ((int)sqrtf(l0), (int)sqrtf(l1)), phi = (double)atan2f(-vy, vx), evaluated in double
 *       from left to right; then the component's heading arrow; after the first update the arrow of the max-likelihood
 *       state (the dir rule at the pt of its mlState);
 *     5 the caller's arrows (0,255,0): Arrow((x1, y1), (x2, y2)) per row of an int32 [m][4] list.
 *   Everything is clipped to the image.  An overlay arrow with an endpoint coordinate beyond +-2^20, and a polyline edge
 *   with such a vertex, is not drawn (32 images away; the coverage arithmetic stays inside 64 bits).
 *   Published size: out_w = (int)((float)W s), out_h = (int)((float)H s) (:442-444).  Equal to the input size: the
 *   composed image.  Otherwise a bilinear resample in fixed point, per axis (x shown):
 *   fx = (float)((ox + 0.5) ((double)W / out_w) - 0.5), sx = floor(fx), fx -= sx; sx < 0: sx = 0, fx = 0; sx >= W - 1:
 *   sx = W - 1, fx = 0; second tap min(sx + 1, W - 1); a1 = lrint(fx 2048) (float product), a0 = 2048 - a1; a channel is
 *   (sum b_i a_j S[y_i][x_j] + 2^21) >> 22.  The project's rule, not cv::resize's.
 *
 * Layer 1.  A call needs four bit planes (arrows, dots, blue, caller's green) of tdr_viz_plane_words(H, W) uint32 each,
 * consecutive, 16-byte aligned, cleared by the caller on the same stream; 11 <= H, W <= 32768.  No allocation, no sync.
 * tdr_viz_arrow_host: the three segments {x1, y1, x2, y2} of Arrow(-(dx, dy), (dx, dy)).  tdr_viz_overlay_host: layers 4
 * and 5 as segments {x1, y1, x2, y2, plane} (plane 2: blue, 3: caller's green) from the mixture (means [k][3] = x, y,
 * theta; covs [k][3][3]), the best state {x, y, theta} (NULL: none) and the caller's arrows; at most
 * TDR_VIZ_MAX_SEGS(k, m) of them.  Both are host functions of the definition. */
#define TDR_VIZ_MAX_SEGS(k, m) (75 * (k) + 3 + 3 * (m))
size_t tdr_viz_plane_words(int H, int W);
int tdr_viz_arrow_host(int dx, int dy, int32_t segs[12]);
int tdr_viz_overlay_host(const float* means, const float* covs, int k, const float* best, const int32_t* arrows, int m,
                         int H, int32_t* segs, int capacity, int* n_out);
int tdr_k_viz_particles(const float* st, int64_t cap, int64_t n, int H, int W, uint32_t* planes, void* stream);
int tdr_k_viz_segments(const int32_t* segs, int m, int H, int W, uint32_t* planes, void* stream);
int tdr_k_viz_compose(const uint8_t* background, int H, int W, const uint32_t* planes, int out_h, int out_w,
                      uint8_t* out_bgr, void* stream);
/* Layer 2.  tdr_filter_set_viz_background uploads the background (host BGR8 [H][W][3]; 11 <= H, W <= 32768) once; the
 * node's changes only with the map.  tdr_filter_visualize draws the picture of the filter's current particles, the mixture
 * of the last tdr_filter_compute_gmm and, after the first update, the max-likelihood state, with `m` caller's arrows
 * (extra_arrows [m][4], may be NULL when m = 0), and reads the published image back into out_bgr_host (`capacity` bytes;
 * 3 * out_h * out_w needed).  *out_h / *out_w are set whenever the published size is valid; out_bgr_host = NULL only asks for them.  Polar and Cartesian
 * filters alike; the filter is not changed.  Refused with TDR_ERR_ARG, the output untouched: no background, a sharded
 * filter, a published dimension of 0 or above 32768 (pub_scale too small or too large, NaN included), too little room. */
int tdr_filter_set_viz_background(tdr_filter* f, const uint8_t* bgr_host, int H, int W);
int tdr_filter_visualize(tdr_filter* f, float pub_scale, const int32_t* extra_arrows, int m, uint8_t* out_bgr_host,
                         int64_t capacity, int* out_h, int* out_w);

/* The batched particle picture: the three stages over a device array of jobs, one launch each for all of them (a job is
 * one picture; blockIdx.y is the job, and a block beyond its job's extent leaves at once).  A job's planes are its own,
 * cleared by the caller.  segs is the job's own list of n_segs segments; best (device {x, y, theta} of the
 * max-likelihood state, or NULL) adds that state's heading arrow as three further segments computed in the launch, so
 * that the host needs no read-back to build the overlay: pass the rest of layer 4 and layer 5 in segs
 * (tdr_viz_overlay_host with best = NULL).  The arrow is the tabulated Arrow(-dir, dir) moved to pt, which equals
 * Arrow(pt - dir, pt + dir): the tips' lrint arguments lie at least 0.04 from a half for every dir, and |pt| <= 2^20.
 * max_n / max_segs / max_out_pixels: the largest n / n_segs / out_h * out_w of the k jobs (they size the grid; a job
 * beyond them is drawn in part only).  k >= 1; no allocation, no sync. */
typedef struct tdr_viz_job {
  const float* st;           /* [7][cap] device states */
  int64_t cap, n;
  int32_t H, W;              /* the background's size */
  uint32_t* planes;          /* 4 * tdr_viz_plane_words(H, W), 16-byte aligned */
  const uint8_t* background; /* [H][W][3] device */
  const int32_t* segs;       /* [n_segs][5] device */
  const float* best;         /* device {x, y, theta}, or NULL */
  int32_t n_segs, pad;
  int32_t out_h, out_w;
  uint8_t* out;              /* [out_h][out_w][3] device */
} tdr_viz_job;
int tdr_k_viz_particles_jobs(const tdr_viz_job* jobs_dev, int k, int64_t max_n, void* stream);
int tdr_k_viz_segments_jobs(const tdr_viz_job* jobs_dev, int k, int max_segs, void* stream);
int tdr_k_viz_compose_jobs(const tdr_viz_job* jobs_dev, int k, int64_t max_out_pixels, void* stream);
/* tdr_batch_visualize: for every i the bytes, *out_h and *out_w of tdr_filter_visualize(f[i], pub_scale, req[i]...).
 * Each filter over its own background (sizes may differ).  The overlays are built on the host and uploaded once; the
 * planes (one arena owned by the calling thread) are cleared with one memset; particles, segments and compose are one
 * launch each on `stream`, which first waits for every filter's own stream; each picture is then copied straight into
 * its request's image and the call waits once, at the end.  Filters with 0 particles, polar and Cartesian filters alike; no filter is changed.  A request with
 * out_bgr_host = NULL only gets its size.  Refused with TDR_ERR_ARG before any device work, every output (images and
 * sizes) untouched: k < 1, a null array or entry, a filter twice, a sharded filter, a filter without a background, an
 * invalid published size, bad arrows, too little room in any request.
 * Out of scope: sharded filters.  One shared device background for several filters and one image of all robots are the
 * fleet picture below; this call keeps one picture and one background per filter. */
typedef struct tdr_viz_request {
  const int32_t* extra_arrows;   /* [m][4], may be NULL when m = 0 */
  int32_t m, pad;
  uint8_t* out_bgr_host;
  int64_t capacity;              /* bytes at out_bgr_host */
  int32_t out_h, out_w;          /* set by the call */
} tdr_viz_request;
int tdr_batch_visualize(tdr_filter* const* f, int k, float pub_scale, tdr_viz_request* req, void* stream);

/* ---- the fleet picture: k robots in one image over one background held by their map ----------------------
 * A DEFINITION like the particle picture, parity unpinned for the same reason (what OpenCV would draw anti-aliased and in
 * particle order is replaced by the coverage rule); the reference shows several robots only as separate displays
 * (survey_mult.rviz).  It draws k filters (1 <= k <= TDR_FLEET_MAX) that share one map over one H x W BGR8 background,
 * 11 <= H, W <= 32768, held by the map handle.  Every primitive, integer conversion, clipping rule and range limit is
 * the particle picture's, unchanged: Arrow, Disc, the segment coverage rule, the mixture polyline, the max-likelihood
 * arrow, the +-2^20 limit, the published size and the fixed-point bilinear resample.  New are the colours and the
 * composition over robots:
 *   Palette: uint8 [k][3][3], for robot i the BGR of its particle arrows, of its border dots and of its estimate.  The
 *     estimate is layer 4 of the particle picture: the mixture's ellipses, their heading arrows and, after the first
 *     update, the max-likelihood arrow.
 *   Per robot three bit planes (arrows, dots, estimate) drawn exactly as planes 0 - 2 of its particle picture; one further
 *     plane for the caller's arrows, one int32 [m][4] list for the whole image.
 *   A pixel takes the first of these that applies:
 *     1 the caller's arrows, (0,255,0);
 *     2 the estimate colour of the HIGHEST-INDEXED robot whose estimate plane covers the pixel;
 *     3 the dot colour of the highest-indexed robot whose dot plane covers it;
 *     4 the arrow colour of the highest-indexed robot whose arrow plane covers it;
 *     5 the background.
 *   The order is layer-major: every robot's dots lie over every robot's arrows and every estimate over every dot,
 *   whatever the indices.  "Highest index wins" makes the image a function of the planes alone: it does not depend on
 *   launch order or on atomics.  With k = 1 and the palette {(0,0,255), (0,255,0), (255,0,0)} the image is
 *   tdr_filter_visualize's, byte for byte.
 * Layer 1.  tdr_k_viz_particles_jobs and tdr_k_viz_segments_jobs draw the whole fleet: one job per robot with its own
 * planes 0 - 2, all jobs with the same H and W.  A segment of plane 3 in robot i's list goes to the words that follow
 * robot i's plane 2, so the caller's arrows travel in ONE robot's list and the plane behind that robot's three is the
 * image's green plane (tdr_batch_visualize_fleet: the last robot's).  tdr_k_viz_compose_fleet composes the published
 * image in one launch: the forms of tdr_k_viz_compose (per-pixel copy; 16 pixels a thread with 16-byte loads and stores
 * when W % 16 == 0 and both images are 16-byte aligned; the four-tap resample composing each tap on the fly).  It reads
 * jobs_dev[i].planes (a job whose H, W differ from the call's, or without planes, draws nothing); palette_host travels in
 * the kernel arguments; background and out_bgr are device images, green_plane tdr_viz_plane_words(H, W) device words.  No
 * allocation, no sync; refused with TDR_ERR_ARG before the launch: null pointers, k outside 1..TDR_FLEET_MAX, H, W or
 * the published size out of range. */
#define TDR_FLEET_MAX 64
int tdr_k_viz_compose_fleet(const tdr_viz_job* jobs_dev, int k, const uint8_t* palette_host, const uint8_t* background,
                            int H, int W, const uint32_t* green_plane, int out_h, int out_w, uint8_t* out_bgr,
                            void* stream);
/* Layer 2.  tdr_map_set_viz_background stores ONE device copy of the background (host BGR8 [H][W][3]) on the map;
 * tdr_map_set_viz_background_labels uploads one byte a cell (uint8 [H][W]) and colours it on the device with lut_bgr (256
 * BGR triplets, tdr_k_label_picture).  Both return after the copy is complete; the background stays until either is
 * called again, and no map update (tdr_map_set*, tdr_filter_update_map*, the incremental updates) touches it, exactly as
 * a filter's own background.  The filters' own backgrounds are another matter: tdr_filter_visualize and
 * tdr_batch_visualize still refuse a filter without its own, whatever its map holds.
 * tdr_batch_visualize_fleet draws the fleet picture of f[0..k-1] over their map's background: `stream` first waits for
 * every filter's own stream; the overlays are built on the host (the max-likelihood arrows in the segments launch, from
 * the device states) and uploaded once; the planes (3k + 1 of them in one arena owned by the calling thread) are cleared
 * with one memset; particles, segments and compose are one launch each; one device-to-host copy into out_bgr_host
 * (`capacity` bytes, 3 * out_h * out_w needed) and one wait.  *out_h / *out_w are set whenever the call is not refused;
 * out_bgr_host = NULL only asks for them.  Polar and Cartesian filters alike, filters with 0 particles too; no filter is
 * changed.  Refused with TDR_ERR_ARG before any device work, the image and the sizes untouched: k < 1 or
 * k > TDR_FLEET_MAX, a null array or entry, a filter twice, a sharded filter, filters on different maps, a map without a
 * background, a null palette, bad arrows, an invalid published size (NaN scale included), too little room.
 * Out of scope: sharded filters, anti-aliasing, several maps or background sizes in one image, more than TDR_FLEET_MAX
 * robots, an arrow list per robot. */
int tdr_map_set_viz_background(tdr_map* m, const uint8_t* bgr_host, int H, int W);
int tdr_map_set_viz_background_labels(tdr_map* m, const uint8_t* labels_host, int H, int W, const uint8_t* lut_bgr);
int tdr_batch_visualize_fleet(tdr_filter* const* f, int k, float pub_scale, const uint8_t* palette,
                              const int32_t* extra_arrows, int m, uint8_t* out_bgr_host, int64_t capacity, int* out_h,
                              int* out_w, void* stream);

/* ---- the scan picture: the node's two scan images and its map background on the device (src/top_down_render.cpp:246-305,
 * :584) ---------------------------------------------------------------------------------------------------
 * All images are BGR8.  `imgs` is the render layout [ncls][rows*cols], column-major: element (i, j) at i + j*rows.
 *   Scan picture (TopDownRender::visualize, :275-305).  The reference builds map_mat(cols, rows) and writes .at(idy, idx)
 *     from cls(idx, idy): the picture is [cols][rows][3] (height = cols, width = rows) and its pixel p = y*rows + x reads
 *     imgs[c][p], the same linear index.  Per pixel, the reference's comparisons as written: best = -inf, worst = +inf,
 *     best_cls = 255; for c = 0 .. ncls-1 in order, v = imgs[c][p]: if (v >= best) { best = v; best_cls = c; }
 *     if (v < worst) worst = v.  A NaN takes part in nothing.  label = 255 when best == worst (all classes equal, all zero
 *     included; always when ncls = 1, or when one class is not NaN); label = 255 when best_cls is still 255 (every value
 *     NaN: the reference indexes out of bounds there); otherwise label = unflatten[best_cls] & 255 (the reference stores
 *     the int into a uint8_t).  Ties go to the LAST class at the maximum (the >=).  The pixel is lut_bgr[label], lut_bgr
 *     the caller's table of 256 BGR triplets: semantics_manager's ind2Color(Mat, Mat) is not in the reference tree, so
 *     the table's contents are the caller's.  Parity unpinned.
 *   Analog picture (visualizeAnalog, :266-273).  One float layer in the same transposed view: a = (float)(255.0 /
 *     (double)scale), t = v * a in float32 without contraction, grey = lrintf(t) (half to even) clamped to [0, 255], and 0
 *     when t is NaN, infinite or outside [-2^31, 2^31) (the project's x86-conversion rule: what cvRound + saturate_cast
 *     give there).  The pixel is (g, g, g).  scale finite and > 0.  A DEFINITION: OpenCV is absent, parity unpinned.
 *   Label picture (aerialMapCallback, :584).  out[p] = lut_bgr[labels[p]] for a uint8 [H][W] label image.
 * Layer 1 (csrc/tdr_scan_viz.hip): device images, host tables (they travel in the kernel arguments), no allocation, no
 * sync.  out_bgr: 3 * npix bytes.  The _jobs forms run k pictures in one launch over a device array of jobs that share
 * the tables; max_npix is the largest npix of the jobs (it sizes the grid; every job is drawn whole whatever it is).
 * Refused with TDR_ERR_ARG before any launch: null pointers, ncls outside 1..TDR_MAX_CLASSES, npix < 1, a scale that is
 * not finite and > 0, k < 1.  A job with bad sizes (ncls above the n_unflatten entries of the table included) writes
 * nothing. */
typedef struct tdr_scan_picture_job {
  const float* imgs;   /* [ncls][npix] device (the analog form: one layer [npix]) */
  int32_t ncls, pad;
  int64_t npix;
  uint8_t* out_bgr;    /* [npix][3] device */
} tdr_scan_picture_job;
typedef struct tdr_label_picture_job {
  const uint8_t* labels;   /* [npix] device */
  int64_t npix;
  uint8_t* out_bgr;        /* [npix][3] device */
} tdr_label_picture_job;
int tdr_k_scan_picture(const float* imgs, int ncls, int64_t npix, const int32_t* unflatten_host,
                       const uint8_t* lut_bgr_host, uint8_t* out_bgr, void* stream);
int tdr_k_analog_picture(const float* img, int64_t npix, float scale, uint8_t* out_bgr, void* stream);
int tdr_k_label_picture(const uint8_t* labels, int64_t npix, const uint8_t* lut_bgr_host, uint8_t* out_bgr, void* stream);
int tdr_k_scan_picture_jobs(const tdr_scan_picture_job* jobs_dev, int k, int64_t max_npix, const int32_t* unflatten_host,
                            int n_unflatten, const uint8_t* lut_bgr_host, void* stream);
int tdr_k_analog_picture_jobs(const tdr_scan_picture_job* jobs_dev, int k, int64_t max_npix, float scale, void* stream);
int tdr_k_label_picture_jobs(const tdr_label_picture_job* jobs_dev, int k, int64_t max_npix, const uint8_t* lut_bgr_host,
                             void* stream);
/* Layer 2.  tdr_renderer_visualize draws the scan picture of the renderer's last semantic render (polar or Cartesian,
 * tdr_renderer_render or tdr_batch_render_polar) from the device images and reads it back: out_bgr_host [cols][rows][3],
 * `capacity` bytes; *out_h = cols and *out_w = rows are set whenever the renderer has a render; out_bgr_host = NULL only
 * asks for them (and needs no tables).  unflatten: the renderer's ncls entries.  tdr_renderer_visualize_analog: layer `cls` of the same render.
 * Refused with TDR_ERR_ARG, the output untouched: no render, too little room, cls outside the render, a bad scale.
 * tdr_scan_picture_host: the scan picture of images the caller holds on the host (the geometric render's two layers,
 * the node's std::vector<Eigen::ArrayXXf>): an upload, one launch, a read-back.
 * tdr_filter_set_viz_background_labels leaves the filter where tdr_filter_set_viz_background leaves it given the
 * host-coloured image of the same labels (uint8 [H][W]): one byte a cell is uploaded and coloured on the device; the
 * same size limits.
 * tdr_batch_scan_pictures: the k scan pictures into out_bgr_host [k][cols][rows][3] with one launch, one device-to-host
 * copy and one wait.  Refused before any device work: k < 1, a null array or entry, a renderer twice, a renderer
 * without a render, renders of different shapes. */
int tdr_renderer_visualize(const tdr_renderer* r, const int32_t* unflatten, const uint8_t* lut_bgr, uint8_t* out_bgr_host,
                           int64_t capacity, int* out_h, int* out_w);
int tdr_renderer_visualize_analog(const tdr_renderer* r, int cls, float scale, uint8_t* out_bgr_host, int64_t capacity,
                                  int* out_h, int* out_w);
int tdr_scan_picture_host(const float* imgs_host, int ncls, int rows, int cols, const int32_t* unflatten,
                          const uint8_t* lut_bgr, uint8_t* out_bgr_host);
int tdr_filter_set_viz_background_labels(tdr_filter* f, const uint8_t* labels_host, int H, int W, const uint8_t* lut_bgr);
int tdr_batch_scan_pictures(const tdr_renderer* const* r, int k, const int32_t* unflatten, const uint8_t* lut_bgr,
                            uint8_t* out_bgr_host, void* stream);

/* ---- map fusion: localised scans vote into the label map on the device (csrc/tdr_fuse.hip, csrc/tdr_host_fuse.cpp;
 * DESIGN.md 5.14) -------------------------------------------------------------------------------------------------------
 * A DEFINITION (the reference has only the embryo, src/refine_map.cpp, an offline tool whose relabelling rule is switched
 * off): parity unpinned.  A robot that localises against a stale aerial map sees the truth in every scan; the filter knows
 * where the scan belongs on the map.  Fusion accumulates the scans' class counts over the map's cells and relabels a cell
 * by its most-voted class; the result goes through tdr_map_patch_labels, so the map, its host copies and its compact form
 * stay coherent.
 *   State.  One uint32 plane per class over the map's cells, votes [ncls][rows][cols] (cell (yi, xi) at yi * cols + xi),
 *     and a dirty bitmap: one bit per TDR_MAP_INCR_TILE^2-cell tile (tile t = ty * ceil(cols / TILE) + tx is bit t & 31 of
 *     word t >> 5; tdr_map_incr_tiles(rows, cols) tiles).
 *   One scan is a render [ncls][rows*cols] (column-major floats, the renderer's layout) with a pose {cx, cy, theta, scale}
 *     and `res`, the quantities StateParticle::computeWeight passes on (cx, cy in the units tdr_k_local_map_* takes).
 *     Polar render (nb x nr, the shape of the map's table): with s = the circular shift getCostForRot computes from theta
 *     (state_particle.cpp:124-128), bin (i, j) of class c with count n adds n to plane c at the cell tdr_k_local_map_polar
 *     addresses for sample k = ((i - s) mod nb) + nb * j at `scale`, `res` — the pairing of scan row and window row of
 *     state_particle.cpp:136-142.  Cartesian render (rows x cols): sample (i, j) votes into the cell tdr_k_local_map_cart
 *     addresses at rot = theta and res * scale, shift 0 (the window of tdr_k_score_cart).  The cell is computed by the
 *     device function the gather itself uses (csrc/tdr_local_cell.h), libm-exact sinf / cosf and rounding included: the
 *     vote step is the transpose of getLocalMap + getCostForRot.
 *   Counts.  A bin value v votes n = (uint32)v when 1 <= v < 2^31, otherwise 0 (NaN, negatives, fractions below 1).
 *     Samples outside the map are dropped and counted.  Known / unknown cells are treated alike.  The adds are device-scope
 *     integer atomics: the planes do not depend on the order of scans or bins.  A cell's count is exact below 2^32 and
 *     WRAPS beyond.
 *   Labels.  Per cell: total = the sum of its votes, w = the class with the most (the lowest index on a tie).  The cell has a
 *     verdict iff total >= min_votes and v_w * share_den >= total * share_num (64-bit integers; share_den <= 2^24 keeps both
 *     products exact).  Its fused label is class_label[w] with a verdict, the BASE label otherwise: the fused image is a
 *     function of (votes, base) alone, not of history.  class_label [ncls] is the caller's class -> raw label table, the
 *     inverse of its flatten_lut.  The label of cell (yi, xi) lives at the image pixel loadCompressedRasterMap samples for
 *     it (top_down_map.cpp:137-138; csrc/tdr_ingest_dev.h), a one-to-one mapping for resolution >= 1 only: maps of a
 *     resolution below 1 are refused.
 * Layer 1: device pointers, no allocation, no sync.  tdr_k_fuse_votes_jobs: k scans in one launch over a DEVICE array of
 * jobs (the K scans of K robots); max_bins = the largest rows * cols of the jobs (it sizes the grid).  map: ncls / rows /
 * cols / resolution are read; tab / nb / nr: the map's polar table (tdr_polar_table_host layout) or NULL / 0 / 0; a polar
 * job of another shape votes nothing.  counters: DEVICE uint64 [2], votes added and votes dropped are ADDED to them.
 * tdr_k_fuse_votes: one scan, through the same launch.  tdr_k_fuse_labels: one workgroup per listed tile (tiles: DEVICE
 * int32 [n_tiles]); `current` is updated in place, out5: DEVICE int32 [5] = {pixels that differed from `current`, then the
 * min y, min x, max y, max x of those pixels}, combined by integer atomics: initialise to {0, INT_MAX, INT_MAX, -1, -1}.
 * class_label_host travels in the kernel arguments.  tdr_k_fuse_decay: v >>= shift on every plane (shift >= 32 zeroes);
 * tiles that held votes become dirty. */
typedef struct tdr_fuse_job {
  const float* scan;   /* [ncls][rows*cols] device */
  int32_t rows, cols;  /* polar: nb, nr */
  int32_t polar, pad;
  float cx, cy, theta, scale, res, pad2;
} tdr_fuse_job;
int tdr_k_fuse_votes_jobs(const tdr_map_desc* map, const float* tab, int nb, int nr, const tdr_fuse_job* jobs_dev, int k,
                          int64_t max_bins, uint32_t* votes, uint32_t* dirty, uint64_t* counters, void* stream);
int tdr_k_fuse_votes(const tdr_map_desc* map, const float* tab, int nb, int nr, const float* scan, int polar, int rows,
                     int cols, float cx, float cy, float theta, float scale, float res, uint32_t* votes, uint32_t* dirty,
                     uint64_t* counters, void* stream);
int tdr_k_fuse_labels(const uint32_t* votes, int ncls, int rows, int cols, int img_h, int img_w, float resolution,
                      const uint8_t* class_label_host, uint32_t min_votes, uint32_t share_num, uint32_t share_den,
                      const uint8_t* base, uint8_t* current, const int32_t* tiles, int n_tiles, int32_t* out5, void* stream);
int tdr_k_fuse_decay(uint32_t* votes, int ncls, int rows, int cols, int shift, uint32_t* dirty, void* stream);
/* Layer 2: the fuser of one map.  tdr_fuser_create needs a map last set from a label image (tdr_map_set_labels or an
 * incremental update); base and `current` are copies of the map's own device image.  Refused: no such map, resolution < 1,
 * share_den == 0 or > 2^24, share_num > share_den, min_votes == 0, flatten_lut[class_label[c]] != c for a class c.
 *   tdr_fuser_add: the renderer's last render, read on the device (ordered against a batched render by the renderer's
 *     events like tdr_filter_update).  tdr_fuser_add_batch: k renders in one launch, poses [k][5] = {cx, cy, theta, scale,
 *     res}.  tdr_fuser_add_images: HOST images [ncls][rows*cols].  votes_added / votes_dropped (may be NULL): this call's.
 *     Refused before any device work: no render, a class count other than the map's, a polar render whose shape is not the
 *     map's table shape, a renderer twice, a non-finite pose, scale <= 0, res <= 0.
 *   tdr_fuser_apply: the label pass over the dirty tiles (the bitmap is cleared); if pixels changed, their bounding
 *     rectangle alone is read back and sent through tdr_map_patch_labels with the map's own centre, then through
 *     tdr_filter_patch_map_labels for each of the k listed filters of that map (k = 0: the map alone), which leaves them
 *     scoring against the new map on their next update.  *changed_cells: the cells whose class changed.
 *   tdr_fuser_decay: tdr_k_fuse_decay.  tdr_fuser_reset: zeroes the votes; tiles that held votes become dirty.
 *   tdr_fuser_rebase: takes the map's present label image as the new base after someone else replaced the map.  The votes
 *     are kept (*kept = 1) only if shape, resolution, class count and centre are unchanged, cleared otherwise.  add and
 *     apply are refused while the map's shape differs from the fuser's.
 *   tdr_fuser_get_votes: HOST uint32 [ncls][rows][cols].  tdr_fuser_get_labels: the fused image, HOST uint8 [img_h][img_w].
 *   tdr_fuser_stats: out9 = {scans added, votes added, votes dropped, applies that changed the map, then the shapes the
 *     two read-backs have: ncls, rows, cols, img_h, img_w}. */
typedef struct tdr_fuser tdr_fuser;
int tdr_fuser_create(tdr_map* m, const uint8_t* class_label, uint32_t min_votes, uint32_t share_num, uint32_t share_den,
                     tdr_fuser** out);
void tdr_fuser_destroy(tdr_fuser* f);
int tdr_fuser_add(tdr_fuser* f, const tdr_renderer* r, float cx, float cy, float theta, float scale, float res,
                  uint64_t* votes_added, uint64_t* votes_dropped);
int tdr_fuser_add_batch(tdr_fuser* f, const tdr_renderer* const* r, int k, const float* poses, uint64_t* votes_added,
                        uint64_t* votes_dropped);
int tdr_fuser_add_images(tdr_fuser* f, const float* imgs_host, int polar, int rows, int cols, float cx, float cy,
                         float theta, float scale, float res, uint64_t* votes_added, uint64_t* votes_dropped);
int tdr_fuser_apply(tdr_fuser* f, tdr_filter* const* filters, int k, int64_t* changed_cells);
int tdr_fuser_decay(tdr_fuser* f, int shift);
int tdr_fuser_reset(tdr_fuser* f);
int tdr_fuser_rebase(tdr_fuser* f, int* kept);
int tdr_fuser_get_votes(const tdr_fuser* f, uint32_t* votes_out);
int tdr_fuser_get_labels(const tdr_fuser* f, uint8_t* labels_out);
int tdr_fuser_stats(const tdr_fuser* f, uint64_t* out9);

/* ---- KLD-sampling count: the pose bins the particle set occupies choose the next count (csrc/tdr_kld.hip,
 * csrc/tdr_host_kld.cpp) --------------------------------------------------------------------------------
 * A DEFINITION (the reference chooses its count from the mixture's ellipse areas, particle_filter.cpp:151-157; this is the
 * rule of KLD-sampling, Fox 2001, AMCL's kld_err / kld_z, applied to the bins the CURRENT set occupies): count the distinct
 * pose-space bins among all n particles, and keep as many particles as that many bins need.  It feeds n_target of
 * tdr_filter_update like tdr_filter_adaptive_count; nothing on the per-scan path changes.
 *   The key of particle p (float32, no contraction):
 *     centre  s = st[SCALE], cx = st[DX] * s + st[INIT_X], cy = st[DY] * s + st[INIT_Y] (the scorer's centre, map pixels);
 *     ix = (int)floorf(med3(cx / bin_xy_px, -524288.f, 524287.f)), iy likewise from cy (IEEE division; floor, not
 *       truncation: -0.5 px lies in bin -1; everything beyond +-2^19 bins shares the outermost bin);
 *     it = the scorer's circular shift of theta (state_particle.cpp:124-128) with theta_bins in place of the scan's direction
 *       count when have_init != 0, and it = theta_bins otherwise: a particle without a heading occupies a bin of its own per
 *       position.  theta is expected finite (the conversion of a non-finite or astronomically large quotient saturates);
 *     is = bits(s) >> (23 - scale_bits): exponent and the top scale_bits mantissa bits (2^scale_bits bins per octave), an
 *       exact integer operation; a fixed or frozen scale gives one value for all particles;
 *     key = (uint64)(ix + 524288) << 43 | (uint64)(iy + 524288) << 23 | (uint64)it << 14 | is   (20 + 20 + 9 + 14 bits:
 *       bit 63 is clear, so the all-ones word TDR_KLD_NO_KEY is no key).
 *     A particle with a non-finite cx, cy or s, or with s <= 0, has no key: it is not counted in k but in `skipped`.  Gated
 *     particles (off the map, scale out of range) are counted like any other: the key depends on the state alone.
 *   k = the number of distinct keys among particles [0, n).
 *   tdr_kld_bound_host, in double, in this order: k < 2 gives 0; otherwise a = 2.0 / (9.0 * (k - 1)),
 *     t = 1.0 - a + sqrt(a) * z, n_kld = ceil(((k - 1) / (2.0 * epsilon)) * (t * t * t)), saturated at 2^62.
 *   tdr_kld_target_host = min(max(n_kld, n_min, 3 * last_count / 4 + 10), max_count): the shrink limit and the cap of
 *     particle_filter.cpp:157, a drop-in for tdr_adaptive_count_host.
 * Layer 1 (device pointers, asynchronous, no allocation).  The kernel: one thread per particle; equal keys are merged among
 * the 64 lanes of a wave; each distinct key of a wave is inserted once into an open-addressing table of 64-bit words in
 * global memory (compare-and-swap, linear probing, empty = all ones), and an insertion counts exactly when its swap found
 * the empty word: integer atomics only, the two words do not depend on order.  workspace: tdr_kld_workspace_bytes(n) bytes
 * (a power of two of slots, at least 2 n).  tdr_k_kld_count fills the table and zeroes out2 on the stream in front of the
 * kernel; out2: DEVICE {k, skipped}.  tdr_k_kld_count_jobs: grid.y = the job, a DEVICE array of jobs; the CALLER has filled
 * every table with all-ones bytes and zeroed every out2 (one fill over adjoining slices).  table_slots: a power of two,
 * >= 2 n, >= 64.  tdr_k_kld_keys: the keys alone, TDR_KLD_NO_KEY where there is none (tests and tools). */
#define TDR_KLD_NO_KEY 0xFFFFFFFFFFFFFFFFull
typedef struct tdr_kld_params {
  float   bin_xy_px;      /* > 0, finite: bin edge in map pixels (the units of the particle centre) */
  int32_t theta_bins;     /* T, 1..511: heading bins over one turn */
  int32_t scale_bits;     /* b, 0..6: mantissa bits of the scale that enter the key (2^b bins per octave) */
  double  epsilon, z;     /* Fox's bound: epsilon > 0, z >= 0 (0.05 and 2.326 are the usual defaults) */
  int64_t n_min;          /* >= 1 */
} tdr_kld_params;
typedef struct tdr_kld_job {
  const float* st;        /* [TDR_ST_FIELDS][cap] device */
  int64_t cap, n;
  uint64_t* table;        /* [table_slots] device, the job's own, all ones */
  int64_t table_slots;
  int64_t* out2;          /* {k, skipped} device, the job's own, zero */
} tdr_kld_job;
size_t tdr_kld_workspace_bytes(int64_t n);
int tdr_k_kld_keys(const float* st, int64_t cap, int64_t n, const tdr_kld_params* p, uint64_t* keys_out, void* stream);
int tdr_k_kld_count(const float* st, int64_t cap, int64_t n, const tdr_kld_params* p, void* workspace, int64_t* out2,
                    void* stream);
int tdr_k_kld_count_jobs(const tdr_kld_job* jobs_dev, int n_jobs, const tdr_kld_params* p, void* stream);
int64_t tdr_kld_bound_host(int64_t k, double epsilon, double z);
int64_t tdr_kld_target_host(int64_t n_kld, int64_t last_count, int64_t n_min, int64_t max_count);
/* Handle layer.  tdr_filter_kld_count: the fill, the kernel and one 16-byte read-back on the filter's stream; the table is
 * the handle's, allocated on first use for n_max.  It READS the states: states, raw and normalised weights, the cached
 * statistics and their validity, the generator's position, tdr_filter_step_count and the stored mixture stay as they were.
 * *target_out = tdr_kld_target_host(bound(k), the filter's count, n_min, its n_max); a filter without particles gives k = 0.
 * Outputs may be NULL.  tdr_batch_kld_count: k filters (polar or Cartesian, on any maps) with one job upload, one fill
 * over the filters' table slices, one launch, one read-back; each filter's numbers equal its own call's.
 * Refused with TDR_ERR_ARG, nothing written, no filter changed: a null filter or parameter pointer, a filter twice, k < 1,
 * bin_xy_px not finite or <= 0, theta_bins outside 1..511, scale_bits outside 0..6, epsilon <= 0 or not finite, z < 0 or
 * not finite, n_min < 1, and SHARDED filters: the distinct count of a sharded set is a global quantity, and combining the
 * ranks' key sets is not built. */
int tdr_filter_kld_count(tdr_filter* f, const tdr_kld_params* p, int64_t* k_out, int64_t* skipped_out, int64_t* target_out);
int tdr_batch_kld_count(tdr_filter* const* filters, int k, const tdr_kld_params* p, int64_t* k_out, int64_t* skipped_out,
                        int64_t* target_out, void* stream);

/* ---- recovery injection: fresh on-road particles for a filter that sits on the wrong place (csrc/tdr_recover.hip,
 * csrc/tdr_host_recover.cpp, csrc/tdr_philox.h) -------------------------------------------------------------
 * A DEFINITION (the reference has no recovery; this is the random-particle injection of augmented MCL, AMCL's
 * recovery_alpha_slow / recovery_alpha_fast, drawn from the map's road cells).  It is a call of its own after
 * tdr_filter_update, like tdr_filter_kld_count: without the call nothing on any existing path changes, the position of
 * the reference's std::mt19937 stream included.
 *   The random source is Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; 10
 *     rounds): philox(counter[4], key[2]) -> 4 words, tdr_philox4x32_host.  A slot's words depend on (seed, draw, slot,
 *     purpose) alone, so an injection is a pure function of its inputs: no grid shape, wave order or rank enters.
 *   The road list of a map: the cell indices r * cols + c, ascending, of every cell whose class-1 slot holds a value < 1.f
 *     (the on-road test of particle initialisation on the device records: unknown cells hold 0 and count as road, as in
 *     the reference).  A lane draws a cell from it in O(1); a per-lane rejection loop would diverge and has a long tail
 *     where road is rare.
 *   Slot i = slot_begin + local (the GLOBAL index, < 2^31), key = {seed lo, seed hi}:
 *     a = philox({i, draw lo, draw hi, 0}, key).  The slot is injected iff (a[0] >> 8) < threshold24, an integer compare;
 *       threshold24 = tdr_inject_threshold_host(p) = floor(p * 2^24) in double, clamped to [0, 2^24] (a NaN gives 0):
 *       0 injects nothing, 2^24 every slot.
 *     cell = road[((uint64)a[1] * n_road) >> 32], r = cell / cols, c = cell % cols.
 *     ux = (a[2] >> 24) * 2^-8, uy = (a[3] >> 24) * 2^-8: eight bits, so (float)c + ux is exact below 2^15 cells a side
 *       and never rounds up into the next cell.
 *     init_x_px = ((float)c + ux) * resolution, init_y_px = ((float)r + uy) * resolution (float32, no contraction),
 *       dx_m = dy_m = 0: x goes with the column, y with the row, as in the StateParticle constructor
 *       (state_particle.cpp:3-49).  At a power-of-two resolution >= 1 the products are exact and the constructor's own
 *       on-road test ((int)((float)(int)x / resolution) per axis) lands on the drawn cell for every injected particle; at
 *       any other resolution the particle is by definition "on the cell it was drawn from", whatever that test rounds to.
 *     scale keeps the value the resample left in the slot: the scale belongs to the sensor-to-map relation that the whole
 *       posterior shares; no transcendental function enters, and a fixed or frozen filter stays uniform.
 *     heading_mode 1: b = philox({i, draw lo, draw hi, 1}, key),
 *       theta = (float)(b[0] >> 8) * 0x1p-24f * 6.2831855f - 3.1415927f, every operation rounded to float32, have_init = 1.
 *     heading_mode 0: theta = 0, have_init = 0: a fresh constructor particle without a heading; the next update's
 *       40-rotation search gives it one.
 *     A slot that is not injected is not written; the padding behind n and the other planes are untouched.
 *   The tracker (host, double): tdr_recovery_track_host(state, w_avg, params): a non-finite or non-positive w_avg leaves
 *     the state alone and returns 0; otherwise each average that is zero is set to w_avg, else w += alpha * (w_avg - w)
 *     (w_slow with alpha_slow first, then w_fast with alpha_fast); p = min(p_max, max(0, 1 - w_fast / w_slow)).
 *     tdr_recovery_reset_host zeroes both averages (AMCL's rule after an injection).  w_avg is info[2] of the update, the
 *     reference's mean over the valid raw weights 1 / (cost + regularization), comparable from scan to scan.
 * Layer 1 (device pointers, asynchronous, no allocation).  tdr_k_map_road_cells: counts per workgroup, a running sum, a
 * write; cells_out holds rows * cols words, *count_dev (DEVICE) the length, workspace tdr_map_road_workspace_bytes(rows,
 * cols) bytes; ncls < 2 is refused as tdr_k_init_particles refuses it, and so are more than 2^31 cells.  tdr_k_inject: one
 * thread per slot, one 4-byte load from the list per injected lane, vector stores to injected slots only;
 * *injected_dev (DEVICE, may be NULL) is INCREMENTED by the number of injected slots with one 64-bit integer atomic per wave
 * that injected something: the caller zeroes it.  tdr_k_inject_jobs: grid.y = the job, a DEVICE array of jobs (filters on any
 * maps: a job carries its map's column count and resolution); the caller has checked what tdr_k_inject checks. */
typedef struct tdr_inject_job {
  float* st;              /* [TDR_ST_FIELDS][cap] device */
  int64_t cap, n, slot_begin;
  const uint32_t* road;   /* [n_road] device */
  int64_t n_road;         /* >= 1 */
  int32_t cols;           /* of the job's map ... */
  float resolution;       /* ... and its resolution */
  uint64_t seed, draw;
  uint32_t threshold24;   /* 0 .. 2^24 */
  int32_t heading_mode;   /* 0 .. 1 */
  int64_t* injected;      /* device, the job's own, or NULL */
} tdr_inject_job;
typedef struct tdr_recovery_state {
  double w_slow, w_fast;
} tdr_recovery_state;
typedef struct tdr_recovery_params {
  double alpha_slow, alpha_fast;   /* in (0, 1]; alpha_slow << alpha_fast (AMCL: 0.001 and 0.1) */
  double p_max;                    /* in [0, 1] */
  int32_t heading_mode;            /* 0 .. 1 */
  uint64_t seed;
} tdr_recovery_params;
void tdr_philox4x32_host(const uint32_t c[4], const uint32_t k[2], uint32_t out[4]);
uint32_t tdr_inject_threshold_host(double p);
double tdr_recovery_track_host(tdr_recovery_state* s, double w_avg, const tdr_recovery_params* p);
void tdr_recovery_reset_host(tdr_recovery_state* s);
size_t tdr_map_road_workspace_bytes(int rows, int cols);
int tdr_k_map_road_cells(const tdr_map_desc* map, uint32_t* cells_out, int64_t* count_dev, void* workspace, void* stream);
int tdr_k_inject(float* st, int64_t cap, int64_t n, int64_t slot_begin, const tdr_map_desc* map, const uint32_t* road,
                 int64_t n_road, uint64_t seed, uint64_t draw, uint32_t threshold24, int heading_mode, int64_t* injected_dev,
                 void* stream);
int tdr_k_inject_jobs(const tdr_inject_job* jobs_dev, int n_jobs, void* stream);
/* Handle layer.  tdr_map_road_cells: the map's road list (DEVICE, the map's own) and its length, built on first use and
 * kept until an entry point writes the map's records (tdr_map_set*, the incremental and patch updates, every loader,
 * tdr_fuser_apply through the patch path): the map counts those writes and the list remembers the count it was built at.
 * A map without records, with fewer than two classes or without a road cell: TDR_ERR_ARG.
 * tdr_filter_get_weight_stats: the first 8 floats of the last update's info (tdr_k_update_weights); TDR_ERR_ARG before the
 * first update.  tdr_filter_inject: draw = tdr_filter_step_count, the road list of the filter's map, the kernel on the
 * filter's stream; injected_out == NULL: no read-back and no wait.  With heading_mode 0 and p > 0 the filter's next update
 * runs the 40-rotation search.  tdr_filter_recovery_step: reads the statistics (one 32-byte read-back), tracks, and when
 * p > 0 injects with the parameters' heading_mode and seed and resets the averages; *p_out, *injected_out may be NULL.
 * tdr_batch_inject: k filters (polar or Cartesian, on any maps), p[k] and seeds[k] one each, with one job upload, one
 * launch, one read-back (injected_out may be NULL: none); each filter ends byte for byte where its own call leaves it.
 * None of them changes raw or normalised weights, the cached weight statistics, the generator's position, the stored
 * mixture or tdr_filter_step_count.  Refused with TDR_ERR_ARG, nothing written: null pointers, p outside [0, 1] or not
 * finite, alphas outside (0, 1], p_max outside [0, 1], heading_mode outside 0..1, a filter without particles or whose map
 * has no road cell, k < 1, a filter twice in a batch, and SHARDED filters (slot_begin makes a rank's slice well defined at
 * layer 1; the handle path for it is not built). */
int tdr_map_road_cells(tdr_map* m, const uint32_t** cells_dev, int64_t* n_road);
/* ... read back: *n_road is set; out_host == NULL only asks for it, else capacity >= *n_road words (TDR_ERR_ARG otherwise) */
int tdr_map_read_road_cells(tdr_map* m, uint32_t* out_host, int64_t capacity, int64_t* n_road);
int tdr_filter_get_weight_stats(tdr_filter* f, float out8[8]);
int tdr_filter_inject(tdr_filter* f, double p, int heading_mode, uint64_t seed, int64_t* injected_out);
int tdr_filter_recovery_step(tdr_filter* f, tdr_recovery_state* s, const tdr_recovery_params* rp, double* p_out,
                             int64_t* injected_out);
int tdr_batch_inject(tdr_filter* const* filters, int k, const double* p, int heading_mode, const uint64_t* seeds,
                     int64_t* injected_out, void* stream);

/* ---- sensor resetting: the injected slots take the best-scoring of C road candidates (csrc/tdr_recover_sensor.hip,
 * csrc/tdr_host_recover.cpp) -----------------------------------------------------------------------------------
 * A DEFINITION, like the recovery injection above, whose words, road list and formulas it uses.  Inputs: a filter and the
 * scan of the step, res, p, candidates = C (1 .. 4096), heading_mode (0 .. 1), seed, draw = the filter's update count.
 *   1. The injected slots are exactly those tdr_k_inject would inject: slot i iff
 *      (philox({i, draw lo, draw hi, 0}, key)[0] >> 8) < threshold24.  The LIST is those slot indices, ascending.
 *   2. Candidate j (0 <= j < C) of slot i, position: a_j = philox({i, draw lo, draw hi, 2j}, key); cell, sub-cell offsets,
 *      init_x_px, init_y_px and dx_m = dy_m = 0 from a_j[1..3] exactly as the injection derives them from a[1..3]; a_j[0] is
 *      unused for j >= 1; scale is the slot's current scale.
 *   3. Its heading.  heading_mode 1: theta from philox({i, draw lo, draw hi, 2j + 1}, key)[0] by the injection's formula,
 *      have_init = 1.  heading_mode 0: theta = 0, have_init = 0.  Candidate 0 is, word for word, the particle the plain
 *      injection writes.
 *   4. A candidate's weight is the raw weight tdr_filter_compute_weights gives a particle in that state in THIS filter: its
 *      map and table, fp, uniform_scale, n_total = the filter's particle count; polar filters: tdr_k_score_polar with
 *      init_search = (heading_mode == 0); Cartesian filters: tdr_k_score_cart_init (mode 0 only), then tdr_k_score_cart.
 *      There is no geometric term.  In mode 0 the search sets the candidate's theta and have_init as for any particle.
 *   5. The pick: key_j = w_j, or -1 where w_j is NaN; the smallest j whose key is the maximum.  A gated candidate (weight 0)
 *      loses to any positive one; if all are NaN, candidate 0 wins.
 *   6. The slot takes the seven state fields of the picked candidate as scoring left them.  Slots that are not on the list
 *      and the padding behind n are not written.
 *   7. Raw and normalised weights, the weight statistics, the generator, the stored mixture and the step count stay as they
 *      are: tdr_filter_inject's contract.
 *   With C = 1 and mode 1 the result is byte for byte tdr_filter_inject's; with C = 1 and mode 0 the slot holds what the
 *   plain injection followed by the next update's search would hold.
 * Layer 1 (device pointers, asynchronous, no allocation).
 *   tdr_k_inject_list: the list of [0, n) (LOCAL indices; the words are those of slot_begin + local) to list_out (n words)
 *     and its length to *count_dev (DEVICE): ballot counts per wave, counts per workgroup, a running sum, a write; workspace
 *     of tdr_inject_list_workspace_bytes(n) bytes.  max_blocks: a bound on the grid (<= 0: the launcher's own; tests) — the
 *     list is the same whatever the grid.  n == 0 or threshold24 == 0: the length alone.
 *   tdr_k_inject_candidates: for list entries [first, first + m) the SoA states [TDR_ST_FIELDS][cand_cap] of their
 *     candidates, candidate q = (e - first) * C + j: one 4-byte road load per candidate, vector stores.
 *   tdr_k_inject_select: one wave per listed slot, the lanes stride over its C weights cand_w[(e - first) * C + j] and the
 *     wave reduces lexicographically on (key, -j), so the result does not depend on the reduction order; the winner's seven
 *     fields go to the slot; pick_out[e - first] = j (may be NULL); *written_dev (DEVICE, may be NULL) is INCREMENTED by the
 *     number of listed slots of the call with one 64-bit integer atomic per workgroup: the caller zeroes it.
 *   Refused with TDR_ERR_ARG before any device work: null pointers, n < 0 or n > cap, slots beyond 2^31, threshold24 above
 *   2^24, first < 0, m < 0, first + m > n, C outside 1 .. 4096, heading_mode outside 0 .. 1, n_road < 1, m * C > cand_cap.
 * Handle layer.  tdr_filter_inject_sensor: the scan as tdr_filter_compute_weights takes it (host images, or a renderer's
 *   last render); scan_imgs == NULL && renderer == NULL: the packed scan the filter keeps from its last update or
 *   compute_weights that was handed images (TDR_ERR_ARG before the first; a renderer's scan stays the renderer's and is not
 *   kept).  The launcher runs the list and WAITS ONCE on the filter's stream for its length; an empty list costs the list
 *   launch and nothing else.  It then walks the list in chunks of max(1, chunk / C) whole slots, chunk =
 *   tdr_config_tuning("inject_cand_chunk") candidates (default 65536; not one of the names listed at tdr_config_tuning:
 *   tests/test_config_table.py replays that list as it was recorded): the candidates, their order by pose (results do not
 *   depend on it), the scoring launch(es) of the filter's kind with n_total = the filter's count, the selection.  (The
 *   Cartesian search, mode 0, waits once more per chunk: tdr_k_score_cart_init reads its own list's length.)  Candidate
 *   states, weights, order and the scorer's workspace are the filter's, allocated on first use and sized by the chunk.
 *   injected_out == NULL: no read-back of the count.  After a call that wrote slots the cached pose statistics are dropped,
 *   and with heading_mode 0 the next update runs the search again (a gated winner can stay without a heading).
 *   tdr_filter_recovery_step_sensor: tdr_filter_recovery_step's tracker and reset rule with this injection.
 *   Refused like tdr_filter_inject, in the same words (sharded filters included), and: candidates outside 1 .. 4096, a res
 *   that is not finite or not positive, a scan of another shape, no scan.  A refused call writes nothing. */
size_t tdr_inject_list_workspace_bytes(int64_t n);
int tdr_k_inject_list(int64_t n, int64_t slot_begin, uint64_t seed, uint64_t draw, uint32_t threshold24, int32_t* list_out,
                      int64_t* count_dev, void* workspace, int max_blocks, void* stream);
int tdr_k_inject_candidates(const float* st, int64_t cap, int64_t n, int64_t slot_begin, const int32_t* list, int64_t first,
                            int64_t m, int candidates, const tdr_map_desc* map, const uint32_t* road, int64_t n_road,
                            uint64_t seed, uint64_t draw, int heading_mode, float* cand_st, int64_t cand_cap, void* stream);
int tdr_k_inject_select(float* st, int64_t cap, int64_t n, const int32_t* list, int64_t first, int64_t m, int candidates,
                        const float* cand_st, int64_t cand_cap, const float* cand_w, int32_t* pick_out, int64_t* written_dev,
                        void* stream);
int tdr_filter_inject_sensor(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, float res, double p,
                             int candidates, int heading_mode, uint64_t seed, int64_t* injected_out);
int tdr_filter_recovery_step_sensor(tdr_filter* f, tdr_recovery_state* s, const tdr_recovery_params* rp, int candidates,
                                    const float* scan_imgs, const tdr_renderer* renderer, float res, double* p_out,
                                    int64_t* injected_out);

/* ---- pose-grid search: one scan scored over a lattice of map cells, the peaks found on the device (csrc/tdr_grid.hip,
 * csrc/tdr_host_grid.cpp) --------------------------------------------------------------------------------------
 * A DEFINITION, like the recovery injection and sensor resetting above (the reference has nothing to match), and a call of
 * its own: without the call every byte of every existing path stays what it is.  Inputs: a filter, the scan, res, a
 * tdr_grid_spec, the radius R and the number K of peaks asked for.
 *   1. Lattice point g = iy * nx + ix (0 <= ix < nx, 0 <= iy < ny) stands on map cell c = c0 + ix * step (column),
 *      r = r0 + iy * step (row), in 64-bit integers.  It is LISTED iff 0 <= c < cols, 0 <= r < rows and, with road_only,
 *      the cell is a road cell by the road list's own test (the class-1 slot of its record holds a value < 1.f).  The LIST
 *      is the listed g, ascending.
 *   2. Candidate (g, h), 0 <= h < H = n_headings: init_x_px = ((float)c + 0.5f) * resolution, init_y_px = ((float)r + 0.5f) *
 *      resolution (float32, no contraction; x goes with the column, as in the injection), dx_m = dy_m = 0, scale =
 *      spec.scale.  heading_mode 1: theta = theta0 + (float)h * dtheta (float32, no contraction), have_init = 1.
 *      heading_mode 0: theta = 0, have_init = 0 (H is 1).
 *   3. A candidate's weight is the raw weight tdr_filter_compute_weights gives a particle in that state in THIS filter:
 *      item 4 of "sensor resetting" with init_search = (heading_mode == 0), n_total = the filter's count, no geometric term.
 *      The polar launch is told the uniform scale that tdr_filter_set_states would note for a set whose scales are all
 *      spec.scale (spec.scale for a filter with a fixed or frozen scale, none otherwise), so a second filter that is handed
 *      the lattice states scores them the same way.
 *   4. Per listed g: key_h = w_h, or -1 where w_h is NaN; the pick is the smallest h whose key is the maximum (the pick rule
 *      of sensor resetting).  W[g] = the pick's weight; T[g] = the pick's theta as scoring left it, or NaN if its have_init
 *      is 0 after scoring.  Unlisted points have W = T = NaN (0x7fc00000).  vol[h * nx * ny + g] = w_h (optional), NaN
 *      for unlisted points.
 *   5. Peaks, radius R (0 .. 16 lattice points, Chebyshev).  g is ELIGIBLE iff W[g] > 0 (NaN, 0 and negative values are not).
 *      g is a peak iff it is eligible and every other lattice point g' of its (2R+1)^2 window inside the lattice is not
 *      eligible, or has W[g'] < W[g], or has W[g'] == W[g] and g' > g.  With R = 0 every eligible point is a peak; a plateau
 *      has exactly one.  The output: n_peaks, and the first min(K, n_peaks) peaks in the order (w descending, g ascending),
 *      K in 0 .. 4096; cell = r * cols + c.  The order is total, so any selection method gives the same bytes.
 * Layer 1 (device pointers, asynchronous, no allocation).
 *   tdr_k_grid_list: the list to list_out (nx * ny words) and its length to *count_dev (DEVICE), by the count / running sum
 *     / write of the road list; workspace of tdr_grid_list_workspace_bytes(nx, ny) bytes; max_blocks as in
 *     tdr_k_inject_list.  The map's records are read with road_only alone.
 *   tdr_k_grid_candidates: for entries [first, first + m) of a list of n_list entries the SoA states
 *     [TDR_ST_FIELDS][cand_cap], candidate q = (e - first) * H + h: one lane per candidate, no loads but the list.
 *   tdr_k_grid_reduce: for the same entries, the weights cand_w[(e - first) * H + h] and the states as scoring left them:
 *     W, T and (vol != NULL) the vol column of every listed point of the window, into planes the caller pre-filled with NaN.
 *     One wave per point and the (key, -h) butterfly of tdr_k_inject_select; H == 1: one lane per point.
 *   tdr_k_grid_peaks: the peaks of the W plane: *n_peaks_dev (DEVICE; set, not incremented) and, with max_peaks > 0, the
 *     first min(max_peaks, n_peaks) entries of peaks_out (DEVICE, max_peaks entries; the rest is not written); workspace of
 *     tdr_grid_peaks_workspace_bytes(nx, ny) bytes (0 for a lattice outside its ranges or when the sort's scratch size
 *     cannot be asked: no device).  A tile of 16 x 16 points with its halo in LDS, comparisons on the
 *     integer bits of the positive floats, then a descending radix sort of the peaks' keys.
 *   Refused with TDR_ERR_ARG before any device work: null pointers, a spec outside the ranges given at the struct, a map
 *   without cells (with road_only: without records or class 1), n_list outside 0 .. nx * ny, first < 0, m < 0,
 *   first + m > n_list, m * H > cand_cap, nms_radius outside 0 .. 16, max_peaks outside 0 .. 4096.
 * Handle layer.  tdr_filter_grid_search: the scan as tdr_filter_inject_sensor takes it (images, a renderer, or NULL, NULL:
 *   the packed scan the filter keeps).  The launcher runs the list and WAITS ONCE for its length, then walks it in chunks of
 *   max(1, tdr_config_tuning("inject_cand_chunk") / H) whole points (candidates, the scoring launches of sensor resetting,
 *   the reduction), then the peaks, then ONE read-back.  w_out, theta_out (nx * ny floats), vol_out (H * nx * ny floats),
 *   peaks_out (max_peaks entries; NULL: no peaks are ordered), n_peaks_out, listed_out (the list's length) are HOST
 *   pointers and may be NULL.  Buffers are the filter's, allocated on first use and sized by the chunk and the lattice.  The
 *   filter's states, raw and normalised weights, weight statistics, generator, mixture, step count and pending heading
 *   search stay as they are; handed images, the filter keeps the packed scan as tdr_filter_inject_sensor does.  Refused like
 *   tdr_filter_inject_sensor (sharded filters and filters without particles included; a map without a road cell is NOT
 *   refused: its road-only list is empty), and: a spec outside its ranges, nms_radius, max_peaks.  A refused call writes
 *   nothing.
 *   tdr_filter_inject_cells: tdr_filter_inject with the caller's cell list (HOST, n_cells words r * cols + c) in place of
 *   the map's road list: the same slots, the same words, the same kernel.  n_cells in 1 .. 2^24 and at most the map's cell
 *   count (tdr_k_inject's bound on a list); every cell < rows * cols, checked on the host; duplicates are allowed and weight
 *   the draw.  This is what turns peaks into particles: with heading_mode 0 the next update's search gives them headings.
 *   The call returns after the list was uploaded.  Refusals and what stays untouched: tdr_filter_inject's. */
typedef struct tdr_grid_spec {
  int32_t c0, r0;        /* map cell (column, row) of lattice point (0, 0); may be negative or beyond the map */
  int32_t step;          /* cells between neighbouring lattice points, >= 1 */
  int32_t nx, ny;        /* lattice points per row, rows; >= 1 each, nx * ny <= 2^24 */
  int32_t road_only;     /* 0 .. 1 */
  int32_t heading_mode;  /* 0: no heading, the 40-rotation search; 1: n_headings fixed headings per point */
  int32_t n_headings;    /* H.  mode 1: 1 .. 4096; mode 0: must be 1 */
  float theta0, dtheta;  /* mode 1, finite: theta_h = theta0 + (float)h * dtheta, float32, no contraction */
  float scale;           /* every candidate's scale; finite, > 0 */
} tdr_grid_spec;
typedef struct tdr_grid_peak {
  int32_t g;
  uint32_t cell;
  float w, theta;
} tdr_grid_peak;
size_t tdr_grid_list_workspace_bytes(int nx, int ny);
int tdr_k_grid_list(const tdr_map_desc* map, const tdr_grid_spec* spec, int32_t* list_out, int64_t* count_dev, void* workspace,
                    int max_blocks, void* stream);
int tdr_k_grid_candidates(const tdr_map_desc* map, const tdr_grid_spec* spec, const int32_t* list, int64_t n_list,
                          int64_t first, int64_t m, float* cand_st, int64_t cand_cap, void* stream);
int tdr_k_grid_reduce(const tdr_grid_spec* spec, const int32_t* list, int64_t n_list, int64_t first, int64_t m,
                      const float* cand_st, int64_t cand_cap, const float* cand_w, float* w_plane, float* theta_plane, float* vol,
                      void* stream);
size_t tdr_grid_peaks_workspace_bytes(int nx, int ny);
int tdr_k_grid_peaks(const tdr_map_desc* map, const tdr_grid_spec* spec, const float* w_plane, const float* theta_plane,
                     int nms_radius, int max_peaks, tdr_grid_peak* peaks_out, int64_t* n_peaks_dev, void* workspace,
                     void* stream);
int tdr_filter_grid_search(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, float res,
                           const tdr_grid_spec* spec, float* w_out, float* theta_out, float* vol_out, int nms_radius,
                           int max_peaks, tdr_grid_peak* peaks_out, int64_t* n_peaks_out, int64_t* listed_out);
int tdr_filter_inject_cells(tdr_filter* f, const uint32_t* cells_host, int64_t n_cells, double p, int heading_mode,
                            uint64_t seed, int64_t* injected_out);

/* internal: lets the handle layer (csrc/tdr_host_*.cpp) report through tdr_last_error() */
int tdr_set_error(int code, const char* msg);

#ifdef __cplusplus
}
#endif
#endif /* TDR_H_ */
