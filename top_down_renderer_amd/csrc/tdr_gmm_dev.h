// tdr_gmm_dev.h — the device table of a batched mixture fit's sampling launch (tdr_batch_compute_gmm, include/tdr.h): one
// entry per filter, built by the handle layer (tdr_host_gmm.cpp), read by gmm_batch_samples_kernel (tdr_gmm.hip).  The fit and
// pick launches read the public tdr_gmm_job / tdr_gmm_pick_job tables.  Internal to libtdr_hip.so.
#ifndef TDR_GMM_DEV_H_
#define TDR_GMM_DEV_H_
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tdr.h"

struct TdrGmmSampleEntry {
  const float* st;     // [7][cap] the filter's particle planes
  int64_t cap, n;
  double* samples;     // [num][4] out: {x, y, 50 cos theta, 50 sin theta}
  int32_t num, pad;    // min(1000, n)
};

// tdr_gmm.hip: tdr_k_sample_ml_states + tdr_k_gmm_samples of every entry, one launch
int tdr_gmm_batch_samples(const TdrGmmSampleEntry* tab_dev, int k, hipStream_t s);

#endif  // TDR_GMM_DEV_H_
