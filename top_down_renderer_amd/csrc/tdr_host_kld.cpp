// tdr_host_kld.cpp — KLD-sampling count (include/tdr.h, "KLD-sampling count"; kernel in csrc/tdr_kld.hip): Fox's bound
// and the target on the host, and the count of one filter or a batch: tdr_filter_kld_count, tdr_batch_kld_count.
#include "tdr_host.h"

namespace {
thread_local StageCtx g_kld_stage;
// the batch's tables, next to one another so that one fill clears them (a single filter uses its own kld_ws)
thread_local DevBuf<uint64_t> g_kld_tables;

int kld_check(const tdr_kld_params* p, const char* who) {
  if (!p) return failh(TDR_ERR_ARG, "%s: null parameters", who);
  if (!(p->bin_xy_px > 0.f) || !std::isfinite(p->bin_xy_px)) return failh(TDR_ERR_ARG, "%s: bin_xy_px = %g (finite, > 0)", who, (double)p->bin_xy_px);
  if (p->theta_bins < 1 || p->theta_bins > 511) return failh(TDR_ERR_ARG, "%s: theta_bins = %d (1 .. 511)", who, p->theta_bins);
  if (p->scale_bits < 0 || p->scale_bits > 6) return failh(TDR_ERR_ARG, "%s: scale_bits = %d (0 .. 6)", who, p->scale_bits);
  if (!(p->epsilon > 0.) || !std::isfinite(p->epsilon)) return failh(TDR_ERR_ARG, "%s: epsilon = %g (finite, > 0)", who, p->epsilon);
  if (!(p->z >= 0.) || !std::isfinite(p->z)) return failh(TDR_ERR_ARG, "%s: z = %g (finite, >= 0)", who, p->z);
  if (p->n_min < 1) return failh(TDR_ERR_ARG, "%s: n_min = %lld (>= 1)", who, (long long)p->n_min);
  return TDR_OK;
}
int64_t kld_target(const tdr_filter* f, const tdr_kld_params* p, int64_t k) {
  return tdr_kld_target_host(tdr_kld_bound_host(k, p->epsilon, p->z), f->n, p->n_min, f->n_max);
}
// `s` continues after everything already queued on the filters' own streams
int kld_wait_filters(tdr_filter* const* fl, int k, hipStream_t s) {
  std::vector<hipStream_t> streams;
  for (int i = 0; i < k; i++)
    if (fl[i]->n >= 1 && fl[i]->stream != s) streams.push_back(fl[i]->stream);
  std::sort(streams.begin(), streams.end());
  streams.erase(std::unique(streams.begin(), streams.end()), streams.end());
  for (hipStream_t fs : streams) {
    hipEvent_t e = nullptr;
    HTRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    int rc = TDR_OK;
    if (hipEventRecord(e, fs) != hipSuccess || hipStreamWaitEvent(s, e, 0) != hipSuccess) rc = failh(TDR_ERR_HIP, "batch_kld_count: stream order");
    (void)hipEventDestroy(e);
    if (rc != TDR_OK) return rc;
  }
  return TDR_OK;
}
}  // namespace

extern "C" {
int64_t tdr_kld_bound_host(int64_t k, double epsilon, double z) {
  if (k < 2) return 0;
  const double km1 = (double)(k - 1);
  const double a = 2.0 / (9.0 * km1);
  const double t = 1.0 - a + std::sqrt(a) * z;
  const double v = std::ceil((km1 / (2.0 * epsilon)) * (t * t * t));
  const double cap = 4611686018427387904.0;   // 2^62
  if (!(v < cap)) return (int64_t)1 << 62;
  return v < 0. ? 0 : (int64_t)v;
}

int64_t tdr_kld_target_host(int64_t n_kld, int64_t last_count, int64_t n_min, int64_t max_count) {
  return std::min<int64_t>(std::max<int64_t>(std::max<int64_t>(n_kld, n_min), 3 * last_count / 4 + 10), max_count);
}

int tdr_filter_kld_count(tdr_filter* f, const tdr_kld_params* p, int64_t* k_out, int64_t* skipped_out, int64_t* target_out) {
  if (!f) return failh(TDR_ERR_ARG, "filter_kld_count: null filter");
  TTRY(kld_check(p, "filter_kld_count"));
  if (f->comm) return failh(TDR_ERR_ARG, "filter_kld_count: the filter is sharded (the distinct count of a sharded set is global; combining the ranks' key sets is not built)");
  int64_t out[2] = {0, 0};
  if (f->n >= 1) {
    // the table for n_max, then the two output words
    const size_t slots = tdr_kld_workspace_bytes(f->n_max) / sizeof(uint64_t);
    TTRY(f->kld_ws.resize(slots + 2));
    int64_t* out_dev = reinterpret_cast<int64_t*>(f->kld_ws.p + slots);
    TTRY(tdr_k_kld_count(f->st.p, f->cap, f->n, p, f->kld_ws.p, out_dev, f->stream));
    HTRY(hipMemcpyAsync(out, out_dev, sizeof(out), hipMemcpyDeviceToHost, f->stream));
    HTRY(hipStreamSynchronize(f->stream));
  }
  if (k_out) *k_out = out[0];
  if (skipped_out) *skipped_out = out[1];
  if (target_out) *target_out = kld_target(f, p, out[0]);
  return TDR_OK;
}

int tdr_batch_kld_count(tdr_filter* const* filters, int k, const tdr_kld_params* p, int64_t* k_out, int64_t* skipped_out,
                        int64_t* target_out, void* stream) {
  if (k < 1) return failh(TDR_ERR_ARG, "batch_kld_count: k = %d, at least one filter is needed", k);
  if (!filters) return failh(TDR_ERR_ARG, "batch_kld_count: null filter array");
  for (int i = 0; i < k; i++)
    if (!filters[i]) return failh(TDR_ERR_ARG, "batch_kld_count: filter %d is null", i);
  TTRY(kld_check(p, "batch_kld_count"));
  {
    std::vector<const tdr_filter*> seen(filters, filters + k);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return failh(TDR_ERR_ARG, "batch_kld_count: a filter appears twice in the batch");
  }
  for (int i = 0; i < k; i++)
    if (filters[i]->comm) return failh(TDR_ERR_ARG, "batch_kld_count: filter %d is sharded (the distinct count of a sharded set is global)", i);
  hipStream_t s = (hipStream_t)stream;
  // staging: [k] jobs and the [k][2] output words, uploaded as zeros with the jobs and read back in place
  const size_t out_off = align64(sizeof(tdr_kld_job) * (size_t)k), bytes = out_off + sizeof(int64_t) * 2 * (size_t)k;
  size_t slots_total = 0;
  for (int i = 0; i < k; i++)
    if (filters[i]->n >= 1) slots_total += tdr_kld_workspace_bytes(filters[i]->n) / sizeof(uint64_t);
  StageCtx& B = g_kld_stage;
  TTRY(B.reserve(bytes, bytes, s));
  if (g_kld_tables.n < slots_total) {
    HTRY(hipEventSynchronize(B.done));   // the last call's kernel has left the old tables
    TTRY(g_kld_tables.resize(slots_total));
  }
  TTRY(kld_wait_filters(filters, k, s));
  tdr_kld_job* jobs = reinterpret_cast<tdr_kld_job*>(B.host);
  int64_t* out_host = reinterpret_cast<int64_t*>(B.host + out_off);
  int64_t* out_dev = reinterpret_cast<int64_t*>(B.dev.p + out_off);
  size_t at = 0;
  for (int i = 0; i < k; i++) {
    const tdr_filter* f = filters[i];
    const int64_t slots = f->n >= 1 ? (int64_t)(tdr_kld_workspace_bytes(f->n) / sizeof(uint64_t)) : 0;
    jobs[i] = tdr_kld_job{f->st.p, f->cap, f->n, g_kld_tables.p + at, slots, out_dev + 2 * i};
    out_host[2 * i] = out_host[2 * i + 1] = 0;
    at += (size_t)slots;
  }
  HTRY(hipMemcpyAsync(B.dev.p, B.host, bytes, hipMemcpyHostToDevice, s));
  if (slots_total) {
    HTRY(hipMemsetAsync(g_kld_tables.p, 0xFF, slots_total * sizeof(uint64_t), s));
    TTRY(tdr_k_kld_count_jobs(reinterpret_cast<const tdr_kld_job*>(B.dev.p), k, p, s));
  }
  HTRY(hipMemcpyAsync(out_host, out_dev, sizeof(int64_t) * 2 * (size_t)k, hipMemcpyDeviceToHost, s));
  HTRY(hipEventRecord(B.done, s));
  HTRY(hipEventRecord(B.uploaded, s));
  HTRY(hipEventSynchronize(B.done));   // the one wait of the call
  for (int i = 0; i < k; i++) {
    if (k_out) k_out[i] = out_host[2 * i];
    if (skipped_out) skipped_out[i] = out_host[2 * i + 1];
    if (target_out) target_out[i] = kld_target(filters[i], p, out_host[2 * i]);
  }
  return TDR_OK;
}
}  // extern "C"
