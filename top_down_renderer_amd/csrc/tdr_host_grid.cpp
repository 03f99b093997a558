// tdr_host_grid.cpp — pose-grid search behind the handle (include/tdr.h, "pose-grid search"; kernels in csrc/tdr_grid.hip):
// tdr_filter_grid_search composes the list, the candidates, the filter's own scoring launches (sensor_score,
// tdr_host_recover.cpp), the reduction and the peak search; tdr_filter_inject_cells is tdr_filter_inject over the caller's
// cell list, which is what turns peaks into particles.
#include "tdr_host.h"

namespace {
constexpr uint32_t NAN_BITS = 0x7fc00000u;   // the NaN of unlisted points (tdr.h)

int grid_check_filter(tdr_filter* f, const char* who) {
  if (f->comm) return failh(TDR_ERR_ARG, "%s: the filter is sharded (the handle path for a rank's slice is not built)", who);
  if (f->n < 1) return failh(TDR_ERR_ARG, "%s: the filter has no particles", who);
  if (!f->map) return failh(TDR_ERR_ARG, "%s: the filter has no map", who);
  return TDR_OK;
}

// the list and ONE wait for its length, then per chunk of whole points the candidates, their scores in this filter and the
// reduction into the planes; the peaks
int grid_run(tdr_filter* f, const float* pk, float res, const tdr_grid_spec* sp, bool want_vol, int R, int K, int64_t* listed_out) {
  hipStream_t s = f->stream;
  tdr_map* m = f->map;
  const int64_t G = (int64_t)sp->nx * sp->ny;
  const int H = sp->n_headings;
  TTRY(f->gs_list.resize((size_t)G));
  TTRY(f->gs_count.resize(2));
  TTRY(f->gs_list_ws.resize(std::max<size_t>(8, tdr_grid_list_workspace_bytes(sp->nx, sp->ny))));
  TTRY(f->gs_w.resize((size_t)G));
  TTRY(f->gs_t.resize((size_t)G));
  if (want_vol) TTRY(f->gs_vol.resize((size_t)G * H));
  TTRY(f->gs_peaks.resize((size_t)std::max(K, 1)));
  const size_t peaks_ws = tdr_grid_peaks_workspace_bytes(sp->nx, sp->ny);
  if (peaks_ws == 0) return failh(TDR_ERR_HIP, "filter_grid_search: the peak search's workspace size could not be asked");
  TTRY(f->gs_peaks_ws.resize(peaks_ws));
  TTRY(tdr_k_grid_list(&m->desc, sp, f->gs_list.p, f->gs_count.p, f->gs_list_ws.p, 0, s));
  HTRY(hipMemsetD32Async((hipDeviceptr_t)f->gs_w.p, (int)NAN_BITS, (size_t)G, s));
  HTRY(hipMemsetD32Async((hipDeviceptr_t)f->gs_t.p, (int)NAN_BITS, (size_t)G, s));
  if (want_vol) HTRY(hipMemsetD32Async((hipDeviceptr_t)f->gs_vol.p, (int)NAN_BITS, (size_t)G * H, s));
  int64_t listed = 0;
  HTRY(hipMemcpyAsync(&listed, f->gs_count.p, sizeof(listed), hipMemcpyDeviceToHost, s));
  HTRY(hipStreamSynchronize(s));
  if (listed < 0 || listed > G) return failh(TDR_ERR_HIP, "filter_grid_search: list length %lld out of range", (long long)listed);
  *listed_out = listed;
  if (listed > 0) {
    f->fp.num_classes = m->desc.ncls;
    const int64_t per = std::min<int64_t>(std::max<int64_t>(1, tdr_cfg().inject_cand_chunk / H), listed);   // points a chunk
    const int64_t ccap = (per * H + 63) / 64 * 64;
    TTRY(f->sr_cst.resize((size_t)TDR_ST_FIELDS * ccap));
    TTRY(f->sr_craw.resize((size_t)ccap));
    TTRY(f->sr_perm.resize((size_t)ccap));
    // what set_states notes for a set whose scales are all spec.scale (note_uniform_scale, tdr_host_filter.cpp)
    const float uniform = f->scale_frozen ? sp->scale : 0.f;
    for (int64_t lo = 0; lo < listed; lo += per) {
      const int64_t mp = std::min(per, listed - lo);
      TTRY(tdr_k_grid_candidates(&m->desc, sp, f->gs_list.p, listed, lo, mp, f->sr_cst.p, ccap, s));
      TTRY(sensor_score(f, pk, res, mp * H, ccap, sp->heading_mode == 0, uniform));
      TTRY(tdr_k_grid_reduce(sp, f->gs_list.p, listed, lo, mp, f->sr_cst.p, ccap, f->sr_craw.p, f->gs_w.p, f->gs_t.p,
                             want_vol ? f->gs_vol.p : nullptr, s));
    }
  }
  return tdr_k_grid_peaks(&m->desc, sp, f->gs_w.p, f->gs_t.p, R, K, f->gs_peaks.p, f->gs_count.p + 1, f->gs_peaks_ws.p, s);
}
}  // namespace

extern "C" {
int tdr_filter_grid_search(tdr_filter* f, const float* scan_imgs, const tdr_renderer* renderer, float res,
                           const tdr_grid_spec* spec, float* w_out, float* theta_out, float* vol_out, int nms_radius,
                           int max_peaks, tdr_grid_peak* peaks_out, int64_t* n_peaks_out, int64_t* listed_out) {
  const char* who = "filter_grid_search";
  if (!f) return failh(TDR_ERR_ARG, "%s: null filter", who);
  TTRY(tdr_grid_spec_check(spec, who));
  if (!std::isfinite(res) || !(res > 0.f)) return failh(TDR_ERR_ARG, "%s: res = %g (finite, > 0)", who, (double)res);
  if (nms_radius < 0 || nms_radius > 16) return failh(TDR_ERR_ARG, "%s: nms_radius = %d (0 .. 16)", who, nms_radius);
  if (max_peaks < 0 || max_peaks > 4096) return failh(TDR_ERR_ARG, "%s: max_peaks = %d (0 .. 4096)", who, max_peaks);
  TTRY(grid_check_filter(f, who));
  tdr_map* m = f->map;
  if (spec->road_only && (!m->desc.rec || m->desc.ncls < 2))
    return failh(TDR_ERR_ARG, "%s: class 1 (road) is required for the on-road test", who);
  TTRY(sensor_check_scan(f, scan_imgs, renderer, who));
  const int K = peaks_out ? max_peaks : 0;
  const int64_t G = (int64_t)spec->nx * spec->ny;
  const float* pk = nullptr;
  TTRY(sensor_take_scan(f, scan_imgs, renderer, &pk));
  int64_t listed = 0;
  TTRY(grid_run(f, pk, res, spec, vol_out != nullptr, nms_radius, K, &listed));
  if (renderer && !scan_imgs) TTRY(renderer_note_read(renderer, f->stream));
  // the one read-back
  hipStream_t s = f->stream;
  int64_t n_peaks = 0;
  std::vector<tdr_grid_peak> peaks((size_t)K);
  if (w_out) HTRY(hipMemcpyAsync(w_out, f->gs_w.p, (size_t)G * sizeof(float), hipMemcpyDeviceToHost, s));
  if (theta_out) HTRY(hipMemcpyAsync(theta_out, f->gs_t.p, (size_t)G * sizeof(float), hipMemcpyDeviceToHost, s));
  if (vol_out) HTRY(hipMemcpyAsync(vol_out, f->gs_vol.p, (size_t)G * spec->n_headings * sizeof(float), hipMemcpyDeviceToHost, s));
  if (K > 0) HTRY(hipMemcpyAsync(peaks.data(), f->gs_peaks.p, (size_t)K * sizeof(tdr_grid_peak), hipMemcpyDeviceToHost, s));
  HTRY(hipMemcpyAsync(&n_peaks, f->gs_count.p + 1, sizeof(n_peaks), hipMemcpyDeviceToHost, s));
  HTRY(hipStreamSynchronize(s));
  if (n_peaks < 0 || n_peaks > G) return failh(TDR_ERR_HIP, "%s: %lld peaks of %lld points", who, (long long)n_peaks, (long long)G);
  if (K > 0) std::memcpy(peaks_out, peaks.data(), (size_t)std::min<int64_t>(K, n_peaks) * sizeof(tdr_grid_peak));
  if (n_peaks_out) *n_peaks_out = n_peaks;
  if (listed_out) *listed_out = listed;
  return TDR_OK;
}

int tdr_filter_inject_cells(tdr_filter* f, const uint32_t* cells_host, int64_t n_cells, double p, int heading_mode,
                            uint64_t seed, int64_t* injected_out) {
  const char* who = "filter_inject_cells";
  if (!f || !cells_host) return failh(TDR_ERR_ARG, "%s: null pointer", who);
  TTRY(inject_check_p(p, heading_mode, who));
  TTRY(grid_check_filter(f, who));
  const tdr_map_desc& d = f->map->desc;
  if (!d.rec || d.rows < 1 || d.cols < 1) return failh(TDR_ERR_ARG, "%s: the map has no records", who);
  if (d.ncls < 2) return failh(TDR_ERR_ARG, "%s: class 1 (road) is required, as for the road list", who);
  const int64_t ncell = (int64_t)d.rows * d.cols;
  if (n_cells < 1 || n_cells > ((int64_t)1 << 24) || n_cells > ncell)
    return failh(TDR_ERR_ARG, "%s: n_cells = %lld (1 .. 2^24, at most the map's %lld cells)", who, (long long)n_cells, (long long)ncell);
  for (int64_t i = 0; i < n_cells; i++)
    if ((int64_t)cells_host[i] >= ncell)
      return failh(TDR_ERR_ARG, "%s: cell %lld is %u, the map has %lld cells", who, (long long)i, cells_host[i], (long long)ncell);
  const uint32_t th = tdr_inject_threshold_host(p);
  hipStream_t s = f->stream;
  // the list of the previous call may still be read on the stream: the copy is ordered behind it
  TTRY(f->gs_cells.resize((size_t)n_cells));
  HTRY(hipMemcpyAsync(f->gs_cells.p, cells_host, (size_t)n_cells * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  int64_t* out_dev = nullptr;
  if (injected_out) {
    TTRY(f->inject_out.resize(1));
    out_dev = f->inject_out.p;
    HTRY(hipMemsetAsync(out_dev, 0, sizeof(int64_t), s));
  }
  TTRY(tdr_k_inject(f->st.p, f->cap, f->n, 0, &d, f->gs_cells.p, n_cells, seed, f->step, th, heading_mode, out_dev, s));
  inject_note(f, th, heading_mode);
  if (injected_out) {
    HTRY(hipMemcpyAsync(injected_out, out_dev, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HTRY(hipStreamSynchronize(s));
  } else {
    HTRY(hipStreamSynchronize(s));   // cells_host is the caller's: the upload has read it when the call returns
  }
  return TDR_OK;
}
}  // extern "C"
