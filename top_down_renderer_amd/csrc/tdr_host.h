// tdr_host.h — what the files of the handle layer (csrc/tdr_host_*.cpp) share; not installed.
// The handle layer is the part of the C ABI behind "tdr_map_* / tdr_renderer_* / tdr_filter_* / tdr_batch_*" in
// include/tdr.h: C++ host code that owns device memory and sequences the hand-written HIP kernels (tdr_*.hip) exactly the
// way the reference's classes sequence their Eigen loops.  One handle = one reference object:
//     tdr_map       TopDownMapPolar   (include/top_down_render/top_down_map_polar.h:6-22)
//     tdr_renderer  ScanRendererPolar (include/top_down_render/scan_renderer_polar.h:15-22)
//     tdr_filter    ParticleFilter    (include/top_down_render/particle_filter.h:22-73)
// One caller thread per handle (the reference calls everything from the ROS spinner thread).  A filter lives on one GPU
// or is sharded over the ranks of a tdr_comm (one process per GPU, tdr_comm.cpp: RCCL or caller-supplied transport).
// No CPU fallback: every entry point fails with TDR_ERR_HIP when no device is present.
// Here: the error macros, DevBuf, the three handle structs, the staging context of the batched calls, and the helpers
// (namespace tdrh) that one file defines and another calls.  A helper with one calling file is static in that file.
#ifndef TDR_HOST_H_
#define TDR_HOST_H_
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "tdr.h"
#include "tdr_batch.h"
#include "tdr_config.h"
#include "tdr_gmm_dev.h"
#include "tdr_internal.h"

namespace tdrh {

#define HTRY(expr)                                                                        \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) return failh(TDR_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define TTRY(expr)            \
  do {                        \
    int rc_ = (expr);         \
    if (rc_ != TDR_OK) return rc_; \
  } while (0)

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;             // owns device memory
  DevBuf& operator=(const DevBuf&) = delete;
  int resize(size_t count) {
    if (count <= n) return TDR_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e != hipSuccess) return failh(TDR_ERR_NOMEM, "hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
    n = count;
    return TDR_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DevBuf() { release(); }
};

// the batched calls' staging (tdr_host_batch.cpp, tdr_host_gmm.cpp); every thread_local object of it stays in one file
struct StageCtx {   // per thread and call kind: pinned staging, its device copy, the events that order their reuse
  char* host = nullptr;
  size_t cap = 0;
  DevBuf<char> dev;
  hipEvent_t uploaded = nullptr;   // the last call's copies have read / written `host`
  hipEvent_t done = nullptr;       // the last call's kernels have read `dev`
  ~StageCtx() {
    if (uploaded) { (void)hipEventSynchronize(uploaded); (void)hipEventDestroy(uploaded); }
    if (done) { (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
    if (host) (void)hipHostFree(host);
  }
  // host >= host_bytes, dev >= dev_bytes; `s` continues after the previous call's kernels
  int reserve(size_t host_bytes, size_t dev_bytes, hipStream_t s) {
    if (!uploaded) HTRY(hipEventCreateWithFlags(&uploaded, hipEventDisableTiming));
    if (!done) HTRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    HTRY(hipEventSynchronize(uploaded));
    if (cap < host_bytes) {
      if (host) HTRY(hipHostFree(host));
      host = nullptr;
      cap = 0;
      HTRY(hipHostMalloc((void**)&host, host_bytes));
      cap = host_bytes;
    }
    if (dev.n < dev_bytes) {
      HTRY(hipEventSynchronize(done));
      TTRY(dev.resize(dev_bytes));
    }
    HTRY(hipStreamWaitEvent(s, done, 0));
    return TDR_OK;
  }
};
inline size_t align64(size_t b) { return (b + 63) / 64 * 64; }
}  // namespace tdrh
using namespace tdrh;

struct tdr_map {
  DevBuf<float> rec;
  DevBuf<float> tab;
  DevBuf<float> fac;   // the table's factors (tdr_polar_factors_host), handed to the filter's tdr_score_ctx
  DevBuf<uint32_t> crec;   // compact form of `rec` (tdr_k_compact_map), when the map has one
  DevBuf<float> cdict;
  DevBuf<uint8_t> cws;
  DevBuf<uint8_t> rec16;   // scratch of the 40-rotation search (tdr_map_desc.rec16), allocated by the first large search
  hipEvent_t rec16_used = nullptr;   // recorded after every search that used rec16; the next one waits for it (map_rec16_*)
  ~tdr_map() { if (rec16_used) (void)hipEventDestroy(rec16_used); }
  std::vector<float> maps_host;  // class_maps_ (column-major), kept for getClassesAtPoint / particle initialisation
  std::vector<uint8_t> mask_host;  // class_mask_ (column-major), kept for the map cache
  tdr_map_desc desc{};
  DevBuf<float> geo_rec;         // geo_maps_[0..1] as a 2-class record map (tdr_k_geo_map_from_map), built on first use
  int geo_pending = 0;           // 0: geo_rec is current (or there is no map); 1: derive from the classes; 2: constant 1
  tdr_map_desc geo_desc{};
  int nb = 0, nr = 0;
  float ang_res = 0;
  int win_rows = 0, win_cols = 0;   // the Cartesian window (tdr_map_set_window); 0: none
  int center_x = 0, center_y = 0;
  bool have_map = false;
  // staging of the run-time map replacement (tdr_map_set_labels: aerial maps keep arriving, top_down_render.cpp:574-600),
  // kept between calls: allocating and freeing ~1 GB per map costs more than the ingest itself
  DevBuf<uint8_t> ing_img, ing_ws, ing_mask;
  DevBuf<int32_t> ing_lut;
  DevBuf<float> ing_maps;
  // incremental updates (tdr_map_update_labels_incremental, csrc/tdr_map_incr.hip).  inc_valid: the map was last set from
  // a label image (tdr_map_set_labels or an incremental update) and ing_img / ing_lut / ing_ws still hold that image, its
  // LUT (inc_lut) and the ingest's class words and column distances.  inc_counts: the dictionary's occurrence counts
  // (tdr_k_map_dict_counts), current while inc_counts_ok; every full compaction clears it.
  bool inc_valid = false, inc_counts_ok = false;
  int inc_img_h = 0, inc_img_w = 0;
  std::vector<int32_t> inc_lut;
  DevBuf<uint8_t> inc_ws, inc_mstage;
  DevBuf<int32_t> inc_counts, inc_dtiles;
  DevBuf<float> inc_stage;
  std::vector<int32_t> inc_tiles;
  std::vector<float> inc_hstage;
  std::vector<uint8_t> inc_hmstage;
  // the fleet picture's background (tdr_map_set_viz_background*): one device copy for every filter on this map; no map
  // update touches it
  DevBuf<uint8_t> viz_bg;
  int viz_h = 0, viz_w = 0;
  // the road list (tdr_map_road_cells, csrc/tdr_recover.hip), built on first use.  rec_writes counts the calls that wrote
  // `rec` (rec_written: every entry point that does makes it); the list is current while road_at equals it.
  DevBuf<uint32_t> road;
  DevBuf<int64_t> road_count;   // the list's length, as the running sum leaves it on the device
  DevBuf<uint8_t> road_ws;
  int64_t road_n = 0;
  uint64_t rec_writes = 0, road_at = ~(uint64_t)0;
  void rec_written() { rec_writes++; }
};

struct tdr_renderer {
  DevBuf<int32_t> lut;
  DevBuf<float> pts, img, pk, geo;
  DevBuf<uint8_t> keys;  // per-point bin keys of the two-phase raster
  DevBuf<uint8_t> geo_ws;  // sort keys / scratch of the geometric render
  int ncls = 0, rows = 0, cols = 0;  // shape of the last render
  bool have_scan = false;
  bool polar = true;                 // ... and its kind (renderSemanticTopDown of ScanRendererPolar / ScanRenderer)
  // tdr_batch_render_polar renders on the caller's stream without a host wait: `rendered` marks the end of that render
  // (render_async), and every stream that has since read img / pk leaves an event in `readers` for the next batched
  // render to wait on (one per stream: a later record on the same stream covers the earlier reads)
  hipEvent_t rendered = nullptr;
  bool render_async = false;
  mutable std::vector<std::pair<hipStream_t, hipEvent_t>> readers;
  mutable size_t n_readers = 0;
  mutable DevBuf<uint8_t> viz_out;   // the scan picture of the last tdr_renderer_visualize(_analog), before its read-back
  ~tdr_renderer() {
    if (rendered) { (void)hipEventSynchronize(rendered); (void)hipEventDestroy(rendered); }
    for (auto& e : readers) { (void)hipEventSynchronize(e.second); (void)hipEventDestroy(e.second); }
  }
};

struct tdr_filter {
  tdr_map* map = nullptr;
  tdr_filter_params fp{};
  int64_t n_max = 0, n = 0;
  DevBuf<float> st, st_new, last_dist, raw_w, w, runmax, info, ws, z4, scan_img, scan_pk, stats;
  DevBuf<uint8_t> pfx_ws;  // chunk headers of the multi-workgroup running sum
  DevBuf<int32_t> idx, perm, loc_tmp;
  DevBuf<tdr_state> aos;
  void* rng = nullptr;
  uint64_t seed = 0, step = 0;
  uint64_t prop_calls = 0;    // device RNG: every propagate call draws fresh noise (counter = calls so far)
  bool scale_frozen = false, maybe_uninit = true, parity_rng = true;
  bool cart = false;          // tdr_filter_create_cart: the scoring stage is the Cartesian one (window = the map's)
  DevBuf<float> init_ws;      // ... and the workspace of its heading search, allocated by the first update that runs it
  int locality_every = 1;
  float uniform_scale = 0.f;
  bool rng_owned = true;      // false after tdr_filter_share_rng: the generator belongs to the caller
  DevBuf<float> gmm_samples;  // [num][3] device staging for computeGMM
  DevBuf<double> gmm_dev;     // the device fit: samples [num][4], the candidate fits' outputs and workspaces (gmm_plan)
  int num_gaussians = 1;      // particle_filter.cpp:7
  std::vector<float> gmm_means, gmm_covs;
  DevBuf<uint64_t> kld_ws;    // tdr_filter_kld_count: the key table for n_max and the two output words, allocated by the first call
  DevBuf<int64_t> inject_out;   // tdr_filter_inject: the count of injected slots, allocated by the first call
  // tdr_filter_inject_sensor (tdr_host_recover.cpp), allocated by the first call: the list of injected slots (n words),
  // {its length, the written slots}, the list build's workspace, and ONE chunk's candidate states, weights, order, the
  // order's scratch and the scorer's workspaces — sized by "inject_cand_chunk", not by the number of candidates
  DevBuf<int32_t> sr_list, sr_perm, sr_tmp;
  DevBuf<int64_t> sr_count;
  DevBuf<uint8_t> sr_list_ws;
  DevBuf<float> sr_cst, sr_craw, sr_ws, sr_init_ws;
  // tdr_filter_grid_search (tdr_host_grid.cpp), allocated by the first call and sized by the lattice: the list of lattice
  // points, {its length, the number of peaks}, the list build's workspace, the W, T and vol planes, the peaks and the
  // workspace of the peak search.  A chunk's candidates, weights and scorer workspaces are the sr_* buffers above.
  // gs_cells: the caller's cell list of tdr_filter_inject_cells.
  DevBuf<int32_t> gs_list;
  DevBuf<int64_t> gs_count;
  DevBuf<uint8_t> gs_list_ws, gs_peaks_ws;
  DevBuf<float> gs_w, gs_t, gs_vol;
  DevBuf<tdr_grid_peak> gs_peaks;
  DevBuf<uint32_t> gs_cells;
  DevBuf<float> ml_dev;  // fields + mlState of the max-likelihood particle of the last update (tdr_k_save_ml_state)
  bool have_ml = false;
  // meanLikelihood + computeMeanCov of the CURRENT particle set, as last read back: publishPoseEst asks for both in a row
  // (src/top_down_render.cpp:333, 354), which is one kernel and one read-back here.  Everything that changes the set
  // clears the flag (states_changed).
  float mean_cov_host[24] = {0};
  bool mean_cov_valid = false;
  // scale() of a frozen filter as tdr_batch_pose read it back (cleared with the mean / covariance)
  float scale_host = -1.f;
  bool scale_valid = false;
  void states_changed() { mean_cov_valid = false; scale_valid = false; }
  hipStream_t stream = nullptr;
  tdr_score_ctx* score_ctx = nullptr;   // this filter's own span tuner (and the table's factors) for its scoring launches (tdr.h)
  // The reference's generator in parity mode: the host std::mt19937 `rng` and its continuation on the device, a
  // tdr_rng_pipe (csrc/tdr_rng.hip).  Exactly one of them is current: propagate and the resample's uniform draw continue
  // the stream on the device (drawn ahead, beside the scoring launch), the host engine takes it back when host code
  // draws (particle initialisation).  A generator shared with the caller (tdr_filter_share_rng) stays on the host.
  tdr_rng_pipe* pipe = nullptr;
  // Sharded over the ranks of `comm` (one process per GPU; NULL = the whole filter lives here).  n / n_max stay the
  // GLOBAL counts; this rank holds particles [rank * nl, (rank + 1) * nl), nl = n / world, in st[7][cap] with
  // cap = n_max / world.  raw_glob / ld_glob / w / runmax are global arrays, identical on every rank.
  tdr_comm* comm = nullptr;
  int world = 1, rank = 0;
  int64_t cap = 0;
  DevBuf<float> xchg_in, xchg_out, raw_glob, ld_glob, st_send, st_all, st_glob, pk_recv;
  DevBuf<float> geo_pk;   // packed geometric scan (tdr_filter_update_geo)
  // the particle picture (tdr_filter_visualize): the background as uploaded, the four bit planes, the overlay segments
  // and the published image
  DevBuf<uint8_t> viz_bg, viz_out;
  DevBuf<uint32_t> viz_planes;
  DevBuf<int32_t> viz_segs;
  int viz_h = 0, viz_w = 0;
  int64_t nl() const { return n / world; }
};

namespace tdrh {
// tdr_host_renderer.cpp
// a stream that reads a renderer's render continues after its batched render / notes the read for the next one
int renderer_wait_render(const tdr_renderer* r, hipStream_t s);
int renderer_note_read(const tdr_renderer* r, hipStream_t s);
// tdr_host_map.cpp: the geometric layers, the compact records, the scratch of the 40-rotation search
int map_make_geo(tdr_map* m, bool constant_one);
int map_ensure_geo(tdr_map* m);
int map_compact(tdr_map* m);
int map_rec16_alloc(tdr_map* m, int64_t n);
int map_rec16_begin(tdr_map* m, hipStream_t s);
int map_rec16_end(tdr_map* m, hipStream_t s);
// tdr_host_filter.cpp: where the generator's stream continues; the particle set of all ranks
bool rng_on_device(const tdr_filter* f);
int rng_to_device(tdr_filter* f);
int rng_to_host(tdr_filter* f);
bool rng_device_capable(const tdr_filter* f);
int filter_global_states(tdr_filter* f, const float** st, int64_t* cap);
int viz_pub_dim(int dim, float s);   // a published dimension of the particle picture; invalid outside 1 .. 32768
// tdr_host_recover.cpp: the checks and notes of an injection; the scan of a sensor-resetting call (checked without a
// write, then taken: packed on the filter's stream) and the raw weights of nc candidate states in f->sr_cst (plane stride
// ccap) as a particle of THIS filter would be scored, to f->sr_craw
int inject_check_p(double p, int heading_mode, const char* who);
void inject_note(tdr_filter* f, uint32_t threshold24, int heading_mode);
int sensor_check_scan(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, const char* who);
int sensor_take_scan(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, const float** pk);
int sensor_score(tdr_filter* f, const float* pk, float res, int64_t nc, int64_t ccap, bool init_search, float uniform_scale);
}  // namespace tdrh
#endif  // TDR_HOST_H_
