// tdr_scan_viz.hip — the node's scan images and its map background coloured on the device (definitions
// in include/tdr.h, "the scan picture"):
//     scan_picture_kernel     per pixel the class with the greatest count -> the caller's colour (TopDownRender::visualize)
//     analog_picture_kernel   one float layer -> grey (visualizeAnalog)
//     label_picture_kernel    a label image through the colour table (aerialMapCallback)
// and their *_jobs_kernel forms: k pictures in one launch over a device array of jobs (blockIdx.y = the job), on the
// same __device__ bodies.
// A thread handles runs of four neighbouring pixels: one 16-byte load per class plane (the lanes of a wave read 1 KB in a
// row) and the twelve output bytes as three words (768 bytes in a row per wave).  Planes that are not 16-byte aligned
// (npix no multiple of 4 with more than one class) and byte-aligned outputs take scalar loads / byte stores, decided
// per launch, never per lane.  The last npix % 4 pixels are one lane each.  The tables (unflatten, the 256 colours)
// travel in the kernel arguments and are staged in LDS, like VizStamps in tdr_viz.hip.  Nothing is allocated, nothing
// waits, and there are no atomics.
#include <climits>

#include "tdr_common.h"

#define SV_RUN 4
#define SV_THREADS 256
#define SV_MAX_BLOCKS 16384   // the grid-stride loops' cap (64 blocks per CU)

namespace {

struct ScanVizTabs {
  int32_t unf[16];      // unflatten[n], n <= TDR_MAX_CLASSES = 15 in [15]
  uint32_t lut[192];    // lut_bgr[256][3], as bytes
};

// the 256 colours as b | g << 8 | r << 16
__device__ __forceinline__ void sv_stage_colours(const ScanVizTabs& tab, uint32_t* s_col) {
  for (int i = threadIdx.x; i < 256; i += SV_THREADS) {
    uint32_t c = 0;
    for (int ch = 0; ch < 3; ch++) {
      const int byte = 3 * i + ch;
      c |= ((tab.lut[byte >> 2] >> (8 * (byte & 3))) & 0xFFu) << (8 * ch);
    }
    s_col[i] = c;
  }
}

__device__ __forceinline__ void sv_store1(uint8_t* __restrict__ out, int64_t p, uint32_t c) {
  out[3 * p] = (uint8_t)c;
  out[3 * p + 1] = (uint8_t)(c >> 8);
  out[3 * p + 2] = (uint8_t)(c >> 16);
}
// the four pixels of run g
__device__ __forceinline__ void sv_store4(uint8_t* __restrict__ out, int64_t g, const uint32_t c[4], bool words) {
  if (words) {
    uint32_t* o = reinterpret_cast<uint32_t*>(out + 12 * g);
    o[0] = c[0] | (c[1] << 24);
    o[1] = (c[1] >> 8) | (c[2] << 16);
    o[2] = (c[2] >> 16) | (c[3] << 8);
  } else {
    for (int j = 0; j < SV_RUN; j++) sv_store1(out, SV_RUN * g + j, c[j]);
  }
}

// the reference's comparisons as written (top_down_render.cpp:284-300)
struct SvPick {
  float best = -INFINITY, worst = INFINITY;
  int cls = 255;
  __device__ __forceinline__ void take(float v, int c) {
    if (v >= best) { best = v; cls = c; }
    if (v < worst) worst = v;
  }
  __device__ __forceinline__ uint32_t label(const int32_t* s_unf) const {
    return (best == worst || cls == 255) ? 255u : (uint32_t)s_unf[cls] & 255u;
  }
};

__device__ __forceinline__ void scan_picture_body(const float* __restrict__ imgs, int ncls, int64_t npix,
                                                  uint8_t* __restrict__ out, const int32_t* s_unf, const uint32_t* s_col,
                                                  int64_t first, int64_t step) {
  const int64_t nrun = npix / SV_RUN;
  const bool wide = (ncls == 1 || npix % SV_RUN == 0) && ((uintptr_t)imgs & 15) == 0;
  const bool words = ((uintptr_t)out & 3) == 0;
  for (int64_t g = first; g < nrun; g += step) {
    SvPick pk[SV_RUN];
    for (int c = 0; c < ncls; c++) {
      const float* q = imgs + (int64_t)c * npix + SV_RUN * g;
      float v[SV_RUN];
      if (wide) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      } else {
        for (int j = 0; j < SV_RUN; j++) v[j] = q[j];
      }
      for (int j = 0; j < SV_RUN; j++) pk[j].take(v[j], c);
    }
    uint32_t col[SV_RUN];
    for (int j = 0; j < SV_RUN; j++) col[j] = s_col[pk[j].label(s_unf)];
    sv_store4(out, g, col, words);
  }
  for (int64_t p = SV_RUN * nrun + first; p < npix; p += step) {   // the tail: fewer than four pixels
    SvPick pk;
    for (int c = 0; c < ncls; c++) pk.take(imgs[(int64_t)c * npix + p], c);
    sv_store1(out, p, s_col[pk.label(s_unf)]);
  }
}

// grey of one value: lrintf(v * a) clamped to [0, 255]; 0 for NaN, an infinity or a product outside int's range
__device__ __forceinline__ uint32_t sv_grey(float v, float a) {
  const float t = v * a;
  if (!(t >= -2147483648.f && t < 2147483648.f)) return 0u;
  const float r = rintf(t);   // half to even
  const uint32_t g = r <= 0.f ? 0u : r >= 255.f ? 255u : (uint32_t)r;
  return g * 0x010101u;
}
__device__ __forceinline__ void analog_picture_body(const float* __restrict__ img, int64_t npix, float a,
                                                    uint8_t* __restrict__ out, int64_t first, int64_t step) {
  const int64_t nrun = npix / SV_RUN;
  const bool wide = ((uintptr_t)img & 15) == 0, words = ((uintptr_t)out & 3) == 0;
  for (int64_t g = first; g < nrun; g += step) {
    const float* q = img + SV_RUN * g;
    float v[SV_RUN];
    if (wide) {
      const float4 t = *reinterpret_cast<const float4*>(q);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
      for (int j = 0; j < SV_RUN; j++) v[j] = q[j];
    }
    uint32_t col[SV_RUN];
    for (int j = 0; j < SV_RUN; j++) col[j] = sv_grey(v[j], a);
    sv_store4(out, g, col, words);
  }
  for (int64_t p = SV_RUN * nrun + first; p < npix; p += step) sv_store1(out, p, sv_grey(img[p], a));
}

__device__ __forceinline__ void label_picture_body(const uint8_t* __restrict__ labels, int64_t npix,
                                                   uint8_t* __restrict__ out, const uint32_t* s_col, int64_t first,
                                                   int64_t step) {
  const int64_t nrun = npix / SV_RUN;
  const bool wide = ((uintptr_t)labels & 3) == 0, words = ((uintptr_t)out & 3) == 0;
  for (int64_t g = first; g < nrun; g += step) {
    uint32_t l;
    if (wide) {
      l = *reinterpret_cast<const uint32_t*>(labels + SV_RUN * g);
    } else {
      const uint8_t* q = labels + SV_RUN * g;
      l = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
    }
    uint32_t col[SV_RUN];
    for (int j = 0; j < SV_RUN; j++) col[j] = s_col[(l >> (8 * j)) & 255u];
    sv_store4(out, g, col, words);
  }
  for (int64_t p = SV_RUN * nrun + first; p < npix; p += step) sv_store1(out, p, s_col[labels[p]]);
}

#define SV_FIRST ((int64_t)blockIdx.x * SV_THREADS + threadIdx.x)
#define SV_STEP ((int64_t)gridDim.x * SV_THREADS)

__global__ __launch_bounds__(SV_THREADS) void scan_picture_kernel(const float* __restrict__ imgs, int ncls, int64_t npix,
                                                                  uint8_t* __restrict__ out, ScanVizTabs tab) {
  __shared__ uint32_t s_col[256];
  __shared__ int32_t s_unf[16];
  sv_stage_colours(tab, s_col);
  if (threadIdx.x < 16) s_unf[threadIdx.x] = tab.unf[threadIdx.x];
  __syncthreads();
  scan_picture_body(imgs, ncls, npix, out, s_unf, s_col, SV_FIRST, SV_STEP);
}
__global__ __launch_bounds__(SV_THREADS) void scan_picture_jobs_kernel(const tdr_scan_picture_job* __restrict__ jobs,
                                                                       ScanVizTabs tab) {
  __shared__ uint32_t s_col[256];
  __shared__ int32_t s_unf[16];
  sv_stage_colours(tab, s_col);
  if (threadIdx.x < 16) s_unf[threadIdx.x] = tab.unf[threadIdx.x];
  __syncthreads();
  const tdr_scan_picture_job j = jobs[blockIdx.y];
  if (!j.imgs || !j.out_bgr || j.ncls < 1 || j.ncls > s_unf[15] || j.npix < 1) return;
  scan_picture_body(j.imgs, j.ncls, j.npix, j.out_bgr, s_unf, s_col, SV_FIRST, SV_STEP);
}

__global__ __launch_bounds__(SV_THREADS) void analog_picture_kernel(const float* __restrict__ img, int64_t npix, float a,
                                                                    uint8_t* __restrict__ out) {
  analog_picture_body(img, npix, a, out, SV_FIRST, SV_STEP);
}
__global__ __launch_bounds__(SV_THREADS) void analog_picture_jobs_kernel(const tdr_scan_picture_job* __restrict__ jobs,
                                                                         float a) {
  const tdr_scan_picture_job j = jobs[blockIdx.y];
  if (!j.imgs || !j.out_bgr || j.npix < 1) return;
  analog_picture_body(j.imgs, j.npix, a, j.out_bgr, SV_FIRST, SV_STEP);
}

__global__ __launch_bounds__(SV_THREADS) void label_picture_kernel(const uint8_t* __restrict__ labels, int64_t npix,
                                                                   uint8_t* __restrict__ out, ScanVizTabs tab) {
  __shared__ uint32_t s_col[256];
  sv_stage_colours(tab, s_col);
  __syncthreads();
  label_picture_body(labels, npix, out, s_col, SV_FIRST, SV_STEP);
}
__global__ __launch_bounds__(SV_THREADS) void label_picture_jobs_kernel(const tdr_label_picture_job* __restrict__ jobs,
                                                                        ScanVizTabs tab) {
  __shared__ uint32_t s_col[256];
  sv_stage_colours(tab, s_col);
  __syncthreads();
  const tdr_label_picture_job j = jobs[blockIdx.y];
  if (!j.labels || !j.out_bgr || j.npix < 1) return;
  label_picture_body(j.labels, j.npix, j.out_bgr, s_col, SV_FIRST, SV_STEP);
}

ScanVizTabs sv_tabs(const int32_t* unflatten, int ncls, const uint8_t* lut_bgr) {
  ScanVizTabs t;
  std::memset(&t, 0, sizeof(t));
  for (int c = 0; c < ncls; c++) t.unf[c] = unflatten[c];
  t.unf[15] = ncls;
  std::memcpy(t.lut, lut_bgr, 768);
  return t;
}
unsigned sv_blocks(int64_t npix) {
  return (unsigned)std::min<int64_t>(std::max<int64_t>(cdiv(cdiv(npix, SV_RUN), SV_THREADS), 1), SV_MAX_BLOCKS);
}
// a = (float)(255.0 / (double)scale); false when scale is not finite and > 0
bool sv_alpha(float scale, float* a) {
  if (!(scale > 0.f) || !(scale < INFINITY)) return false;
  *a = (float)(255.0 / (double)scale);
  return true;
}

}  // namespace

extern "C" int tdr_k_scan_picture(const float* imgs, int ncls, int64_t npix, const int32_t* unflatten_host,
                                  const uint8_t* lut_bgr_host, uint8_t* out_bgr, void* stream) {
  if (!imgs || !unflatten_host || !lut_bgr_host || !out_bgr) return fail(TDR_ERR_ARG, "scan_picture: null pointer");
  if (ncls < 1 || ncls > TDR_MAX_CLASSES || npix < 1)
    return fail(TDR_ERR_ARG, "scan_picture: %d classes of %lld pixels (1..%d classes, at least 1 pixel)", ncls,
                (long long)npix, TDR_MAX_CLASSES);
  hipLaunchKernelGGL(scan_picture_kernel, dim3(sv_blocks(npix)), dim3(SV_THREADS), 0, (hipStream_t)stream, imgs, ncls, npix,
                     out_bgr, sv_tabs(unflatten_host, ncls, lut_bgr_host));
  LAUNCH_CHECK("scan_picture");
  return TDR_OK;
}

extern "C" int tdr_k_analog_picture(const float* img, int64_t npix, float scale, uint8_t* out_bgr, void* stream) {
  if (!img || !out_bgr) return fail(TDR_ERR_ARG, "analog_picture: null pointer");
  if (npix < 1) return fail(TDR_ERR_ARG, "analog_picture: %lld pixels", (long long)npix);
  float a;
  if (!sv_alpha(scale, &a)) return fail(TDR_ERR_ARG, "analog_picture: scale %g (finite and > 0)", (double)scale);
  hipLaunchKernelGGL(analog_picture_kernel, dim3(sv_blocks(npix)), dim3(SV_THREADS), 0, (hipStream_t)stream, img, npix, a,
                     out_bgr);
  LAUNCH_CHECK("analog_picture");
  return TDR_OK;
}

extern "C" int tdr_k_label_picture(const uint8_t* labels, int64_t npix, const uint8_t* lut_bgr_host, uint8_t* out_bgr,
                                   void* stream) {
  if (!labels || !lut_bgr_host || !out_bgr) return fail(TDR_ERR_ARG, "label_picture: null pointer");
  if (npix < 1) return fail(TDR_ERR_ARG, "label_picture: %lld pixels", (long long)npix);
  hipLaunchKernelGGL(label_picture_kernel, dim3(sv_blocks(npix)), dim3(SV_THREADS), 0, (hipStream_t)stream, labels, npix,
                     out_bgr, sv_tabs(nullptr, 0, lut_bgr_host));
  LAUNCH_CHECK("label_picture");
  return TDR_OK;
}

static int sv_jobs_args(const char* who, const void* jobs, int k, int64_t max_npix) {
  if (!jobs) return fail(TDR_ERR_ARG, "%s: null job array", who);
  if (k < 1 || k > 65535) return fail(TDR_ERR_ARG, "%s: k = %d (1 .. 65535 jobs)", who, k);
  if (max_npix < 1) return fail(TDR_ERR_ARG, "%s: max_npix = %lld", who, (long long)max_npix);
  return TDR_OK;
}

extern "C" int tdr_k_scan_picture_jobs(const tdr_scan_picture_job* jobs_dev, int k, int64_t max_npix,
                                       const int32_t* unflatten_host, int n_unflatten, const uint8_t* lut_bgr_host,
                                       void* stream) {
  if (int rc = sv_jobs_args("scan_picture_jobs", jobs_dev, k, max_npix)) return rc;
  if (!unflatten_host || !lut_bgr_host) return fail(TDR_ERR_ARG, "scan_picture_jobs: null table");
  if (n_unflatten < 1 || n_unflatten > TDR_MAX_CLASSES)
    return fail(TDR_ERR_ARG, "scan_picture_jobs: %d unflatten entries (1..%d)", n_unflatten, TDR_MAX_CLASSES);
  hipLaunchKernelGGL(scan_picture_jobs_kernel, dim3(sv_blocks(max_npix), (unsigned)k), dim3(SV_THREADS), 0,
                     (hipStream_t)stream, jobs_dev, sv_tabs(unflatten_host, n_unflatten, lut_bgr_host));
  LAUNCH_CHECK("scan_picture_jobs");
  return TDR_OK;
}

extern "C" int tdr_k_analog_picture_jobs(const tdr_scan_picture_job* jobs_dev, int k, int64_t max_npix, float scale,
                                         void* stream) {
  if (int rc = sv_jobs_args("analog_picture_jobs", jobs_dev, k, max_npix)) return rc;
  float a;
  if (!sv_alpha(scale, &a)) return fail(TDR_ERR_ARG, "analog_picture_jobs: scale %g (finite and > 0)", (double)scale);
  hipLaunchKernelGGL(analog_picture_jobs_kernel, dim3(sv_blocks(max_npix), (unsigned)k), dim3(SV_THREADS), 0,
                     (hipStream_t)stream, jobs_dev, a);
  LAUNCH_CHECK("analog_picture_jobs");
  return TDR_OK;
}

extern "C" int tdr_k_label_picture_jobs(const tdr_label_picture_job* jobs_dev, int k, int64_t max_npix,
                                        const uint8_t* lut_bgr_host, void* stream) {
  if (int rc = sv_jobs_args("label_picture_jobs", jobs_dev, k, max_npix)) return rc;
  if (!lut_bgr_host) return fail(TDR_ERR_ARG, "label_picture_jobs: null table");
  hipLaunchKernelGGL(label_picture_jobs_kernel, dim3(sv_blocks(max_npix), (unsigned)k), dim3(SV_THREADS), 0,
                     (hipStream_t)stream, jobs_dev, sv_tabs(nullptr, 0, lut_bgr_host));
  LAUNCH_CHECK("label_picture_jobs");
  return TDR_OK;
}
