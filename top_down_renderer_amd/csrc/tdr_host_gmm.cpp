// tdr_host_gmm.cpp — computeGMM on the device (csrc/tdr_gmm.hip) for one filter or a batch:
// tdr_filter_compute_gmm_device, tdr_batch_compute_gmm.
#include "tdr_host.h"

// ---- the mixture fit on the device: tdr_filter_compute_gmm_device, tdr_batch_compute_gmm (csrc/tdr_gmm.hip) ---------------
namespace {
thread_local StageCtx g_gmm_stage;
constexpr size_t GMM_OUT_MAX = 21 * TDR_GMM_MAX_K + 2;

// what one filter's fit needs in its gmm_dev (doubles): samples [4 num] | 3 outputs | the candidates' workspaces
struct GmmPlan {
  int num = 0, cand[3] = {0, 0, 0};
  size_t ws_off[3] = {0, 0, 0}, total = 0;
  static size_t out_off(int num, int j) { return (size_t)4 * num + GMM_OUT_MAX * j; }
};
int gmm_plan(const tdr_filter* f, GmmPlan& p) {
  p.num = (int)std::min<int64_t>(1000, f->n);   // :262
  TTRY(tdr_gmm_candidates_host(f->num_gaussians, f->n, p.num, TDR_GMM_MAX_K, p.cand));
  p.total = GmmPlan::out_off(p.num, 3);
  for (int j = 0; j < 3; j++) {
    p.ws_off[j] = p.total;
    if (p.cand[j]) p.total += tdr_gmm_workspace_bytes(p.num, p.cand[j]) / sizeof(double);
  }
  return TDR_OK;
}

// The two ways the samples reach a filter's gmm_dev.  One filter, possibly sharded: tdr_filter_compute_gmm's sampling
// (filter_global_states + tdr_k_sample_ml_states) and the conversion, on `s`.
int gmm_sample_filter(tdr_filter* f, int num, hipStream_t s) {
  const float* gst = nullptr;
  int64_t gcap = 0;
  TTRY(f->gmm_samples.resize((size_t)3 * num));
  TTRY(filter_global_states(f, &gst, &gcap));
  TTRY(tdr_k_sample_ml_states(gst, gcap, f->n, num, f->gmm_samples.p, s));
  return tdr_k_gmm_samples(f->gmm_samples.p, num, f->gmm_dev.p, s);
}
// A batch: `s` continues after everything already queued on the filters' own streams; the samples are then one launch
// over the uploaded table (tdr_gmm_batch_samples).
int gmm_wait_filters(tdr_filter* const* fl, int k, hipStream_t s) {
  std::vector<hipStream_t> streams;
  for (int i = 0; i < k; i++)
    if (fl[i]->n >= 1) streams.push_back(fl[i]->stream);
  std::sort(streams.begin(), streams.end());
  streams.erase(std::unique(streams.begin(), streams.end()), streams.end());
  for (hipStream_t fs : streams) {
    if (fs == s) continue;
    hipEvent_t e = nullptr;
    HTRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    int rc = TDR_OK;
    if (hipEventRecord(e, fs) != hipSuccess || hipStreamWaitEvent(s, e, 0) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_compute_gmm: stream order");
    (void)hipEventDestroy(e);
    if (rc != TDR_OK) return rc;
  }
  return TDR_OK;
}

// The fit of the filters fl[0 .. k) that hold particles, on `s`: tables, sample(live filters, their plans, the device
// table of their sample entries), every candidate fit, the picks, one read-back, the host conversion.
extern "C++" template <class Sample>
int gmm_device_run(tdr_filter* const* fl, int k, hipStream_t s, Sample sample) {
  std::vector<tdr_filter*> live;
  for (int i = 0; i < k; i++)
    if (fl[i]->n >= 1) live.push_back(fl[i]);
  const int kd = (int)live.size();
  if (kd == 0) return TDR_OK;
  std::vector<GmmPlan> plan((size_t)kd);
  int nj = 0;
  for (int i = 0; i < kd; i++) {
    TTRY(gmm_plan(live[i], plan[i]));
    TTRY(live[i]->gmm_dev.resize(plan[i].total));
    for (int j = 0; j < 3; j++) nj += plan[i].cand[j] != 0;
  }
  // staging: [kd] sample entries, [nj] fit jobs, [kd] pick jobs; then the [kd] records the pick writes and the copy brings back
  const size_t samp_off = 0, job_off = align64(sizeof(TdrGmmSampleEntry) * (size_t)kd);
  const size_t pick_off = job_off + align64(sizeof(tdr_gmm_job) * (size_t)nj);
  const size_t rec_off = pick_off + align64(sizeof(tdr_gmm_pick_job) * (size_t)kd);
  const size_t rec_bytes = sizeof(double) * TDR_GMM_RECORD_DOUBLES * (size_t)kd;
  StageCtx& B = g_gmm_stage;
  TTRY(B.reserve(rec_off + rec_bytes, rec_off + rec_bytes, s));
  TdrGmmSampleEntry* samp = reinterpret_cast<TdrGmmSampleEntry*>(B.host + samp_off);
  tdr_gmm_job* jobs = reinterpret_cast<tdr_gmm_job*>(B.host + job_off);
  tdr_gmm_pick_job* picks = reinterpret_cast<tdr_gmm_pick_job*>(B.host + pick_off);
  double* rec_dev = reinterpret_cast<double*>(B.dev.p + rec_off);
  const double* rec_host = reinterpret_cast<const double*>(B.host + rec_off);
  int jn = 0;
  for (int i = 0; i < kd; i++) {
    tdr_filter* f = live[i];
    const GmmPlan& p = plan[i];
    double* base = f->gmm_dev.p;
    samp[i] = TdrGmmSampleEntry{f->st.p, f->cap, f->n, base, p.num, 0};
    picks[i] = tdr_gmm_pick_job{{nullptr, nullptr, nullptr}, p.cand[0], 0, rec_dev + (size_t)TDR_GMM_RECORD_DOUBLES * i};
    for (int j = 0; j < 3; j++) {
      if (!p.cand[j]) continue;
      double* out = base + GmmPlan::out_off(p.num, j);
      jobs[jn++] = tdr_gmm_job{base, p.num, p.cand[j], 100, 0, out, base + p.ws_off[j]};
      picks[i].cand[j] = out;
    }
  }
  HTRY(hipMemcpyAsync(B.dev.p, B.host, rec_off, hipMemcpyHostToDevice, s));
  HTRY(hipMemsetAsync(rec_dev, 0, rec_bytes, s));   // (a fit that wrote nothing is seen as a count of 0)
  TTRY(sample(live, plan, reinterpret_cast<const TdrGmmSampleEntry*>(B.dev.p + samp_off)));
  TTRY(tdr_k_gmm_fit_jobs(reinterpret_cast<const tdr_gmm_job*>(B.dev.p + job_off), nj, s));
  TTRY(tdr_k_gmm_pick(reinterpret_cast<const tdr_gmm_pick_job*>(B.dev.p + pick_off), kd, s));
  HTRY(hipMemcpyAsync(B.host + rec_off, rec_dev, rec_bytes, hipMemcpyDeviceToHost, s));
  HTRY(hipEventRecord(B.done, s));
  HTRY(hipEventRecord(B.uploaded, s));
  HTRY(hipEventSynchronize(B.done));   // the one wait of the call
  for (int i = 0; i < kd; i++) {
    const int kc = (int)rec_host[(size_t)TDR_GMM_RECORD_DOUBLES * i];
    if (kc < 1 || kc > TDR_GMM_MAX_K) return failh(TDR_ERR_HIP, "compute_gmm_device: the device fit left no mixture");
  }
  for (int i = 0; i < kd; i++) {   // the conversion of tdr_gmm_select_host (:303-312), on the host's libm
    tdr_filter* f = live[i];
    const double* rec = rec_host + (size_t)TDR_GMM_RECORD_DOUBLES * i;
    const int kc = (int)rec[0];
    f->num_gaussians = kc;
    f->gmm_means.resize((size_t)3 * kc);
    f->gmm_covs.resize((size_t)9 * kc);
    for (int c = 0; c < kc; c++) {
      const double* o = rec + 2 + 8 * c;
      f->gmm_means[3 * c + 0] = (float)o[0];
      f->gmm_means[3 * c + 1] = (float)o[1];
      f->gmm_means[3 * c + 2] = (float)std::atan2(o[3], o[2]);
      float* q = f->gmm_covs.data() + 9 * c;
      q[0] = (float)o[4]; q[1] = (float)o[5]; q[2] = 0.f;
      q[3] = (float)o[6]; q[4] = (float)o[7]; q[5] = 0.f;
      q[6] = 0.f; q[7] = 0.f; q[8] = 1.f;
    }
  }
  return TDR_OK;
}
}  // namespace

extern "C" {
int tdr_filter_compute_gmm_device(tdr_filter* f) {
  if (!f) return failh(TDR_ERR_ARG, "filter_compute_gmm_device: null filter");
  if (f->n < 1) return TDR_OK;
  return gmm_device_run(&f, 1, f->stream, [&](const std::vector<tdr_filter*>& live, const std::vector<GmmPlan>& plan,
                                              const TdrGmmSampleEntry*) { return gmm_sample_filter(live[0], plan[0].num, f->stream); });
}

int tdr_batch_compute_gmm(tdr_filter* const* filters, int k, void* stream) {
  if (k < 1) return failh(TDR_ERR_ARG, "batch_compute_gmm: k = %d, at least one filter is needed", k);
  if (!filters) return failh(TDR_ERR_ARG, "batch_compute_gmm: null filter array");
  for (int i = 0; i < k; i++)
    if (!filters[i]) return failh(TDR_ERR_ARG, "batch_compute_gmm: filter %d is null", i);
  {
    std::vector<const tdr_filter*> seen(filters, filters + k);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return failh(TDR_ERR_ARG, "batch_compute_gmm: a filter appears twice in the batch");
  }
  for (int i = 0; i < k; i++)
    if (filters[i]->comm) return failh(TDR_ERR_ARG, "batch_compute_gmm: filter %d is sharded (the gather inside is collective)", i);
  hipStream_t s = (hipStream_t)stream;
  TTRY(gmm_wait_filters(filters, k, s));
  return gmm_device_run(filters, k, s, [&](const std::vector<tdr_filter*>& live, const std::vector<GmmPlan>&,
                                           const TdrGmmSampleEntry* tab_dev) { return tdr_gmm_batch_samples(tab_dev, (int)live.size(), s); });
}
}  // extern "C"
