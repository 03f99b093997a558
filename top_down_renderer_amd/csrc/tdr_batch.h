// tdr_batch.h — the device tables of a batched filter step (tdr_batch_step, include/tdr.h): one entry per filter of the
// batch, built by the handle layer (tdr_host_batch.cpp) and read by the batched kernels — propagate and resample
// (tdr_batch.hip), statistics and running sum (tdr_prefix.hip: one workgroup per filter), scoring (tdr_score.hip).  A
// workgroup finds its filter from its block index: entry k owns the blocks [blk_prop, next entry's blk_prop) of the
// propagate launch and [blk_res, next entry's blk_res) of the resample launch, and workgroup k of the statistics and
// running-sum launches.  Internal to libtdr_hip.so.
#ifndef TDR_BATCH_H_
#define TDR_BATCH_H_
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "tdr.h"

struct TdrBatchEntry {
  float* st;              // [7][cap] the filter's particle planes
  float* st_new;          // [7][cap] the resampled set (the handle swaps the two afterwards)
  float* last_dist;       // [cap]
  const float* z4;        // [n][4] propagate's normals from the filter's own generator (tdr_rng_pipe_normals)
  const float* runmax;    // [n] running maximum of the running sum (tdr_k_prefix)
  const float* shift;     // the resample's uniform on the device (tdr_rng_pipe_uniform)
  const float* info;      // statistics of tdr_k_update_weights: info[0] = argmax
  int32_t* idx;           // [n_new] resample indices
  float* ml;              // [12] max-likelihood particle (tdr_k_save_ml_state)
  const float* raw_w;     // [n] raw weights of the scoring launch
  float* w_out;           // [n] normalised weights (tdr_k_update_weights)
  float* info_out;        // TDR_UW_INFO_FLOATS statistics
  float* runmax_out;      // [n] running maximum of the running sum (tdr_k_prefix)
  int64_t cap, n, n_new;
  float tx, ty, omega, pos_cov, theta_cov;
  int32_t scale_freeze;
  int32_t blk_prop, blk_res;   // first block of this filter in the propagate / resample launch
};

// the entry whose block range holds block b: the largest e < k with first(e) <= b (ranges are non-empty and ascending)
template <class First>
__device__ __forceinline__ int batch_find(int k, int b, First first) {
  int lo = 0, hi = k - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first(mid) <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// tdr_batch.hip.  tab: device copy of the k entries; blocks_prop / blocks_res: total blocks of the two launches.
int tdr_batch_propagate(const TdrBatchEntry* tab, int k, int blocks_prop, hipStream_t s);
int tdr_batch_resample(const TdrBatchEntry* tab, int k, int blocks_res, hipStream_t s);
#define TDR_BATCH_THREADS 256
// tdr_prefix.hip: tdr_k_update_weights / tdr_k_prefix of every filter (n <= 32 768; n_max: the largest n of the batch)
int tdr_batch_update_weights(const TdrBatchEntry* tab, int k, int64_t n_max, hipStream_t s);
int tdr_batch_prefix(const TdrBatchEntry* tab, int k, int64_t n_max, hipStream_t s);

// tdr_score.hip: the float form of every filter's scoring launch (tdr_k_score_polar_ctx without the locality order), one
// grid — with the 40-rotation search of the filters that ask for it (init_search) in front of it (tdr_score_init.h: one
// launch per pass kind, same bits as the standalone search).  build fills a host staging area of
// tdr_batch_score_stage_bytes(k, k_init) bytes (64-byte aligned); the caller copies it to device memory; launch reads the
// grid sizes from the host copy and the tables from the device copy.  A filter whose launch takes the integer form
// (tdr_score_polar_float_form == false) is refused.
struct TdrBatchScoreIn {
  const float* scan_pk;   // packed scan (tdr_k_pack_scan)
  float res;
  const tdr_filter_params* fp;
  float* st;
  int64_t cap, n;
  float uniform_scale;
  float* raw_w;
  float* ws;              // tdr_score_workspace_floats(ncls, nb, nr, n, n) floats
  int init_search;        // the filter may hold a particle without a heading: its 40-rotation search runs first
};
size_t tdr_batch_score_stage_bytes(int k, int k_init);   // k_init: the filters with init_search set
int tdr_batch_score_build(const tdr_map_desc* map, const float* tab, int nb, int nr, int k, const TdrBatchScoreIn* in,
                          void* host_stage);
int tdr_batch_score_launch(const tdr_map_desc* map, const float* tab, int nb, int nr, int k, const void* host_stage,
                           const void* dev_stage, hipStream_t s);

// ---- the two ends of a batched node loop (tdr_batch_loop.hip): tdr_batch_render_polar and tdr_batch_pose ---------------
// raster: one entry per cloud; entry k owns the blocks [blk_keys, next entry's blk_keys) of the keys launch and row
// blockIdx.y == k of the raster launch.  pts / keys live in the batch's own device buffer, img / pk are the renderer's.
struct TdrBatchRasterEntry {
  const float* pts;
  const int32_t* lut;     // the renderer's LUT (256 entries)
  uint32_t* keys;         // [n] bin keys
  float* img;             // [ncls][rows*cols]
  float* pk;              // [rows*cols][rf]
  int64_t n;
  float res;
  int32_t stride, ioff;
  int32_t blk_keys;
};
struct TdrBatchRasterShape { float ang_res; int ncls, rows, cols, rf, cpt; };
bool tdr_batch_raster_shape(int ncls, int rows, int cols, float ang_res, TdrBatchRasterShape* out);
int tdr_batch_raster(const TdrBatchRasterEntry* tab, int k, int blocks_keys, const TdrBatchRasterShape& a, hipStream_t s);

// pose statistics: one entry per filter with n >= 1; `out` is the filter's TDR_BATCH_POSE_FLOATS-float result record
// ([0, 24) as tdr_k_mean_cov writes them, [24] the scale of particle 0), `scratch` the filter's stats buffer + 24 (the
// partial sums of the multi-workgroup form).  small: n <= TDR_BATCH_MC_SINGLE_MAX_N (one workgroup each), big: the rest.
struct TdrBatchPoseEntry {
  const float* st;
  int64_t cap, n;
  float* out;
  float* scratch;
};
#define TDR_BATCH_POSE_FLOATS 32
#define TDR_BATCH_MC_SINGLE_MAX_N 4096        // MC_SINGLE_MAX_N (tdr_filter_dev.h; tdr_batch_loop.hip asserts they agree)
int tdr_batch_pose_launch(const TdrBatchPoseEntry* small, int k_small, const TdrBatchPoseEntry* big, int k_big,
                          hipStream_t s);

#endif  // TDR_BATCH_H_
