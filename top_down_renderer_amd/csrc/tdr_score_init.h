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
#endif  // TDR_SCORE_INIT_H_
