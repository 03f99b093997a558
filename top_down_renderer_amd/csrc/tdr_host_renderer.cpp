// tdr_host_renderer.cpp — ScanRenderer(Polar) behind tdr_renderer_*: create, the semantic and the geometric render,
// the read-back of the last render and its pictures (include/tdr.h, "the scan picture"; kernels in tdr_scan_viz.hip); and
// the two event helpers that order other streams against a batched render.
#include "tdr_host.h"

namespace tdrh {
int renderer_wait_render(const tdr_renderer* r, hipStream_t s) {
  if (r->render_async) HTRY(hipStreamWaitEvent(s, r->rendered, 0));
  return TDR_OK;
}
int renderer_note_read(const tdr_renderer* r, hipStream_t s) {
  size_t i = 0;
  while (i < r->n_readers && r->readers[i].first != s) i++;
  if (i == r->n_readers) {
    if (i == r->readers.size()) {
      hipEvent_t e = nullptr;
      HTRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      r->readers.emplace_back(s, e);
    }
    r->readers[i].first = s;
    r->n_readers++;
  }
  HTRY(hipEventRecord(r->readers[i].second, s));
  return TDR_OK;
}
}  // namespace tdrh

// what tdr_renderer_visualize and tdr_renderer_visualize_analog share: the size, the room, the read-back.  `draw` launches
// the picture of the render into r->viz_out on the null stream.
template <class Draw>
static int renderer_picture(const tdr_renderer* r, const char* who, uint8_t* out_bgr_host, int64_t capacity, int* out_h,
                            int* out_w, Draw draw) {
  *out_h = r->cols;
  *out_w = r->rows;
  if (!out_bgr_host) return TDR_OK;
  const size_t P = (size_t)r->rows * r->cols, bytes = 3 * P;
  if (capacity < 0 || (size_t)capacity < bytes)
    return failh(TDR_ERR_ARG, "%s: the image needs %zu bytes, room for %lld", who, bytes, (long long)capacity);
  TTRY(r->viz_out.resize(bytes));
  TTRY(renderer_wait_render(r, nullptr));
  TTRY(draw((int64_t)P));
  TTRY(renderer_note_read(r, nullptr));
  HTRY(hipMemcpy(out_bgr_host, r->viz_out.p, bytes, hipMemcpyDeviceToHost));
  return TDR_OK;
}

extern "C" {

// ---- ScanRenderer(Polar) ------------------------------------------------------------------------------------------------
int tdr_renderer_create(const int32_t* flatten_lut256, tdr_renderer** out) {
  if (!flatten_lut256 || !out) return failh(TDR_ERR_ARG, "renderer_create: null pointer");
  if (tdr_device_count() < 1) return failh(TDR_ERR_HIP, "renderer_create: no HIP device (there is no CPU fallback)");
  tdr_renderer* r = new tdr_renderer();
  int rc = r->lut.resize(256);
  if (rc == TDR_OK && hipMemcpy(r->lut.p, flatten_lut256, 256 * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
    rc = failh(TDR_ERR_HIP, "renderer_create: lut upload failed");
  if (rc != TDR_OK) {
    delete r;
    return rc;
  }
  *out = r;
  return TDR_OK;
}
void tdr_renderer_destroy(tdr_renderer* r) { delete r; }

// renderSemanticTopDown (scan_renderer_polar.cpp:83-109 when polar != 0, scan_renderer.cpp:55-78 otherwise).
// pts: HOST points; imgs_out: HOST [ncls][rows*cols] column-major images, written in place (may be NULL: the render
// then only stays on the device for tdr_filter_update).
int tdr_renderer_render(tdr_renderer* r, int polar, const float* pts, int stride, int ioff, int64_t n, float res,
                        float ang_res, int ncls, int rows, int cols, float* imgs_out) {
  if (!r) return failh(TDR_ERR_ARG, "render: null renderer");
  if (n < 0 || (n > 0 && !pts)) return failh(TDR_ERR_ARG, "render: null points");
  if (ncls < 1 || rows < 1 || cols < 1) return TDR_OK;  // `if (imgs.size() < 1) return;` (:85)
  const size_t P = (size_t)rows * cols;
  if (r->render_async) {   // (a tdr_batch_render_polar still writing img / pk)
    HTRY(hipEventSynchronize(r->rendered));
    r->render_async = false;
  }
  TTRY(r->pts.resize((size_t)std::max<int64_t>(n, 1) * stride));
  TTRY(r->img.resize(P * ncls));
  TTRY(r->pk.resize(P * tdr_rec_floats(ncls)));
  if (n > 0) HTRY(hipMemcpy(r->pts.p, pts, (size_t)n * stride * sizeof(float), hipMemcpyHostToDevice));
  TTRY(r->keys.resize((size_t)tdr_raster_workspace_bytes(std::max<int64_t>(n, 1))));
  if (polar)
    TTRY(tdr_k_raster_polar(r->pts.p, stride, ioff, n, res, ang_res, r->lut.p, ncls, rows, cols, r->img.p, r->pk.p,
                            r->keys.p, nullptr));
  else
    TTRY(tdr_k_raster_cart(r->pts.p, stride, ioff, n, res, r->lut.p, ncls, rows, cols, r->img.p, r->pk.p, r->keys.p,
                           nullptr));
  if (imgs_out) HTRY(hipMemcpy(imgs_out, r->img.p, P * ncls * sizeof(float), hipMemcpyDeviceToHost));
  else HTRY(hipDeviceSynchronize());
  r->ncls = ncls;
  r->rows = rows;
  r->cols = cols;
  r->polar = polar != 0;
  r->have_scan = true;
  return TDR_OK;
}

// renderGeometricTopDown (scan_renderer_polar.cpp:6-81 when polar != 0, scan_renderer.cpp:7-53 otherwise).  pts: HOST
// organised cloud (element idy*width + idx); imgs_out: HOST [2][rows*cols] column-major (ground, obstacles).
int tdr_renderer_render_geo(tdr_renderer* r, int polar, const float* pts, int stride, int64_t width, int64_t height,
                            float res, float ang_res, int rows, int cols, float* imgs_out) {
  if (!r || !imgs_out) return failh(TDR_ERR_ARG, "render_geo: null pointer");
  const int64_t n = width * height;
  if (width < 0 || height < 0 || (n > 0 && !pts)) return failh(TDR_ERR_ARG, "render_geo: bad cloud");
  if (rows < 1 || cols < 1) return TDR_OK;
  const size_t P = (size_t)rows * cols;
  TTRY(r->pts.resize((size_t)std::max<int64_t>(n, 1) * stride));
  TTRY(r->geo.resize(2 * P));
  if (n > 0) HTRY(hipMemcpy(r->pts.p, pts, (size_t)n * stride * sizeof(float), hipMemcpyHostToDevice));
  if (polar) {
    TTRY(r->geo_ws.resize((size_t)tdr_raster_geo_workspace_bytes(std::max<int64_t>(n, 1))));
    TTRY(tdr_k_raster_geo_polar(r->pts.p, stride, width, height, res, ang_res, rows, cols, r->geo.p, r->geo_ws.p, nullptr));
  } else {
    TTRY(tdr_k_raster_geo_cart(r->pts.p, stride, width, height, res, rows, cols, r->geo.p, nullptr));
  }
  HTRY(hipMemcpy(imgs_out, r->geo.p, 2 * P * sizeof(float), hipMemcpyDeviceToHost));
  return TDR_OK;
}

int tdr_renderer_get_render(const tdr_renderer* r, float* imgs_out, float* pk_out) {
  if (!r) return failh(TDR_ERR_ARG, "renderer_get_render: null renderer");
  if (!r->have_scan) return failh(TDR_ERR_ARG, "renderer_get_render: the renderer has no render");
  const size_t P = (size_t)r->rows * r->cols;
  if (r->render_async) HTRY(hipEventSynchronize(r->rendered));
  if (imgs_out) HTRY(hipMemcpy(imgs_out, r->img.p, P * r->ncls * sizeof(float), hipMemcpyDeviceToHost));
  if (pk_out) HTRY(hipMemcpy(pk_out, r->pk.p, P * tdr_rec_floats(r->ncls) * sizeof(float), hipMemcpyDeviceToHost));
  return TDR_OK;
}

// ---- the scan picture ------------------------------------------------------------------------------------------------------
int tdr_renderer_visualize(const tdr_renderer* r, const int32_t* unflatten, const uint8_t* lut_bgr, uint8_t* out_bgr_host,
                           int64_t capacity, int* out_h, int* out_w) {
  if (!r || !out_h || !out_w || (out_bgr_host && (!unflatten || !lut_bgr)))   // (a size query needs no tables)
    return failh(TDR_ERR_ARG, "renderer_visualize: null argument");
  if (!r->have_scan) return failh(TDR_ERR_ARG, "renderer_visualize: the renderer has no render");
  if (r->ncls > TDR_MAX_CLASSES) return failh(TDR_ERR_ARG, "renderer_visualize: %d classes (at most %d)", r->ncls, TDR_MAX_CLASSES);
  return renderer_picture(r, "renderer_visualize", out_bgr_host, capacity, out_h, out_w, [&](int64_t P) {
    return tdr_k_scan_picture(r->img.p, r->ncls, P, unflatten, lut_bgr, r->viz_out.p, nullptr);
  });
}

int tdr_renderer_visualize_analog(const tdr_renderer* r, int cls, float scale, uint8_t* out_bgr_host, int64_t capacity,
                                  int* out_h, int* out_w) {
  if (!r || !out_h || !out_w) return failh(TDR_ERR_ARG, "renderer_visualize_analog: null argument");
  if (!r->have_scan) return failh(TDR_ERR_ARG, "renderer_visualize_analog: the renderer has no render");
  if (cls < 0 || cls >= r->ncls) return failh(TDR_ERR_ARG, "renderer_visualize_analog: class %d of %d", cls, r->ncls);
  if (!(scale > 0.f) || !(scale < std::numeric_limits<float>::infinity()))
    return failh(TDR_ERR_ARG, "renderer_visualize_analog: scale %g (finite and > 0)", (double)scale);
  return renderer_picture(r, "renderer_visualize_analog", out_bgr_host, capacity, out_h, out_w, [&](int64_t P) {
    return tdr_k_analog_picture(r->img.p + (size_t)cls * P, P, scale, r->viz_out.p, nullptr);
  });
}

int tdr_scan_picture_host(const float* imgs_host, int ncls, int rows, int cols, const int32_t* unflatten,
                          const uint8_t* lut_bgr, uint8_t* out_bgr_host) {
  if (!imgs_host || !unflatten || !lut_bgr || !out_bgr_host) return failh(TDR_ERR_ARG, "scan_picture_host: null argument");
  if (ncls < 1 || ncls > TDR_MAX_CLASSES || rows < 1 || cols < 1)
    return failh(TDR_ERR_ARG, "scan_picture_host: bad image shape %dx%dx%d", ncls, rows, cols);
  if (tdr_device_count() < 1) return failh(TDR_ERR_HIP, "scan_picture_host: no HIP device (there is no CPU fallback)");
  static thread_local DevBuf<float> img;      // kept between calls: the node draws two of these per scan
  static thread_local DevBuf<uint8_t> out;
  const size_t P = (size_t)rows * cols;
  TTRY(img.resize(P * ncls));
  TTRY(out.resize(3 * P));
  HTRY(hipMemcpy(img.p, imgs_host, P * ncls * sizeof(float), hipMemcpyHostToDevice));
  TTRY(tdr_k_scan_picture(img.p, ncls, (int64_t)P, unflatten, lut_bgr, out.p, nullptr));
  HTRY(hipMemcpy(out_bgr_host, out.p, 3 * P, hipMemcpyDeviceToHost));
  return TDR_OK;
}

}  // extern "C"
