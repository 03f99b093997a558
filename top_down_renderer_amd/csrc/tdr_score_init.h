// tdr_score_init.h — host interface of the 40-rotation init search (tdr_score_init.hip), used by tdr_score.hip.
#ifndef TDR_SCORE_INIT_H_
#define TDR_SCORE_INIT_H_
#include "tdr_common.h"

// state_particle.cpp:195-206 for the n particles of `order` (NULL = identity) that have no heading yet: the candidate
// rotations (init_rot), the matrix-core pass that applies — half records / on the fly / wide / none — the vector kernel
// (everything, or only what the matrix-core pass could not take), and the chosen theta / have_init written to `st`.
// utab: the uniform-scale table or NULL.  res_flag: n floats (0 = untouched, 1 = initialised, 2 = initialised but every
// rotation scored NaN), res_theta = res_flag + npad: n floats; the rotation table lives behind them, at res_theta + npad
// (64 words, tdr_score_workspace_floats).  n_total: the filter's particle count over all ranks (it picks the pass).
int tdr_score_init_search(const tdr_map_desc* map, const float* tab, const float* utab, const float* scan_pk, int nb,
                          int nr, float res, const tdr_filter_params* fp, float* st, int64_t cap, int64_t n,
                          int64_t n_total, const int32_t* order, float* res_flag, int64_t npad, hipStream_t s);
// particles whose search found no valid rotation (res_flag == 2) get the weight 1 / (FLT_MAX + regularization)
int tdr_score_init_fixup(const float* res_flag, int64_t n, float regularization, float* raw_w, hipStream_t s);

// The matrix-core pass the search of a filter of n_total particles takes on this map — the one choice behind the
// standalone and the batched search (the passes pick differently where candidates tie to rounding): pre-split half records
// (map->rec16 set, >= tdr_config_rec16_min_particles particles, up to 7 classes), the f32 records split on the fly
// (8-float records), the wide kernel (12 / 16 floats), or none (the vector kernel alone; tdr_config_init_mfma(0)).
enum { TDR_INIT_PASS_VECTOR = 0, TDR_INIT_PASS_HALF = 1, TDR_INIT_PASS_SPLIT = 2, TDR_INIT_PASS_WIDE = 3 };
int tdr_score_init_pass(const tdr_map_desc* map, int nb, int64_t n_total);

// The searches of k filters of a batch (tdr_batch_step) as one launch per pass kind and instantiation present, called by
// tdr_batch_score_build / _launch.  Per filter what tdr_score_init_search takes: utab is its uniform-scale table or NULL,
// res_flag / npad its workspace as above.  build fills a host staging area of tdr_batch_init_stage_bytes(k) bytes, the
// caller copies it to the device; launch = rotation tables, flags, the passes, the vector kernel, apply — before the
// scoring launch; fixup after it.  Filters on the half-record pass need map->rec16 (the caller allocates it).
struct TdrBatchInitIn {
  const float* scan_pk;
  float res;
  const tdr_filter_params* fp;
  float* st;
  int64_t cap, n;
  const float* utab;
  float* res_flag;
  int64_t npad;
  float* raw_w;
};
size_t tdr_batch_init_stage_bytes(int k);
int tdr_batch_init_build(const tdr_map_desc* map, const float* tab, int nb, int nr, int k, const TdrBatchInitIn* in,
                         void* host_stage);
int tdr_batch_init_launch(const tdr_map_desc* map, int nb, int nr, const void* host_stage, const void* dev_stage,
                          hipStream_t s);
int tdr_batch_init_fixup(const void* host_stage, const void* dev_stage, hipStream_t s);
#endif  // TDR_SCORE_INIT_H_
