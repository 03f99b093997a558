// tdr_viz.hip — the node's map_viz picture built on the device (definition in include/tdr.h,
// "the particle picture").  The picture is four bit planes over the background — particle arrows, border dots, the blue
// overlay (mixture, best particle), the caller's green arrows — composed into the published BGR image in one pass:
//     viz_particles_kernel   every particle ORs its arrow (a 13 x 13 stamp, tabulated per dir) or its dot into planes 0 / 1
//     viz_segments_kernel    one workgroup per overlay segment ORs its pixels into plane 2 or 3
//     viz_compose_*_kernel   background + planes -> published image (same size: copy with overlay; else the four taps of
//                            the fixed-point bilinear resample are composed on the fly)
//     viz_fleet_*_kernel     the fleet picture: the planes 0 - 2 of k robots and one green plane over one
//                            background, layer-major with the highest index winning, in the same three forms
// Every pixel set is integer arithmetic (viz_covered), so a primitive's pixels do not depend on who draws it; the
// double-precision parts of the definition (arrow tips, ellipse vertices) run on the host (tdr_viz_arrow_host,
// tdr_viz_overlay_host) and reach the device as integers.
//
// Contention: a converged cloud puts every particle on a few dozen pixels.  A workgroup therefore ORs its stamps into a
// 64-row x 256-pixel LDS tile per plane, placed at the least row and word its particles touch, and flushes the tile's
// non-zero words; what falls outside the tile, and the flush, go to global memory with an atomic OR that a plain load
// skips when the bits are already there.  OR is idempotent and bits are never cleared during a call, so the planes are
// the same whichever way a bit travels.
#include <climits>
#include <mutex>

#include "tdr_common.h"
#include "tdr_sincosf.h"

#define VIZ_R 6                      // an arrow's pixels lie within +-6 of pt
#define VIZ_ROWS (2 * VIZ_R + 1)
#define VIZ_DIRS 121                 // dir in [-5, 5]^2 (28 of them are reachable)
#define VIZ_LIM (1 << 20)            // overlay endpoints beyond +-2^20 are not drawn
#define VIZ_TH 64                    // the LDS tile: rows x words
#define VIZ_TW 8
#define VIZ_MAX_DIM 32768

namespace {

// float -> int as x86's cvttss2si does it: truncation inside int's range, INT_MIN outside it and for NaN
__host__ __device__ inline int viz_f2i(float v) { return (v >= -2147483648.f && v < 2147483648.f) ? (int)v : INT_MIN; }

// the coverage rule of a segment of half width 1 between integer endpoints (|coordinates| <= 2^21: no overflow)
__host__ __device__ inline bool viz_covered(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py) {
  const int64_t ux = bx - ax, uy = by - ay, wx = px - ax, wy = py - ay;
  const int64_t L = ux * ux + uy * uy, d = ux * wx + uy * wy;
  if (L == 0 || d <= 0) return wx * wx + wy * wy <= 1;
  if (d >= L) {
    const int64_t vx = px - bx, vy = py - by;
    return vx * vx + vy * vy <= 1;
  }
  int64_t c = ux * wy - uy * wx;
  if (c < 0) c = -c;
  return c < (1 << 22) && c * c <= L;   // (c^2 <= L < 2^44)
}

// the three segments of Arrow(p1, p2): shaft, then the tips at ang + pi/4 and ang - pi/4 (cv::arrowedLine, tipLength 0.3)
void viz_arrow(int64_t x1, int64_t y1, int64_t x2, int64_t y2, int64_t s[12]) {
  const double dx = (double)(x1 - x2), dy = (double)(y1 - y2);
  const double tip = std::sqrt(dx * dx + dy * dy) * 0.3;
  const double ang = std::atan2(dy, dx);
  s[0] = x1; s[1] = y1; s[2] = x2; s[3] = y2;
  for (int i = 0; i < 2; i++) {
    const double a = i == 0 ? ang + M_PI / 4 : ang - M_PI / 4;
    s[4 + 4 * i] = std::lrint((double)x2 + tip * std::cos(a));
    s[5 + 4 * i] = std::lrint((double)y2 + tip * std::sin(a));
    s[6 + 4 * i] = x2;
    s[7 + 4 * i] = y2;
  }
}

// the row masks of Arrow(-dir, dir) for every dir: bit i of row r = pixel (i - 6, r - 6)
struct VizStamps {
  uint32_t w[(VIZ_DIRS * VIZ_ROWS + 1) / 2];   // uint16 rows[VIZ_DIRS][VIZ_ROWS], packed in pairs
};
const VizStamps& viz_stamps() {
  static VizStamps tab;
  static std::once_flag once;
  std::call_once(once, [] {
    std::memset(&tab, 0, sizeof(tab));
    for (int dx = -5; dx <= 5; dx++)
      for (int dy = -5; dy <= 5; dy++) {
        int64_t s[12];
        viz_arrow(-dx, -dy, dx, dy, s);
        for (int r = 0; r < VIZ_ROWS; r++) {
          uint32_t m = 0;
          for (int i = 0; i < VIZ_ROWS; i++)
            for (int k = 0; k < 3; k++)
              if (viz_covered(s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3], i - VIZ_R, r - VIZ_R)) m |= 1u << i;
          const int e = ((dx + 5) * 11 + (dy + 5)) * VIZ_ROWS + r;
          tab.w[e / 2] |= m << (16 * (e & 1));
        }
      }
  });
  return tab;
}

__host__ __device__ inline int viz_row_words(int W) { return (W + 127) / 128 * 4; }   // whole 16-byte groups

// ---- particles -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void viz_or_global(uint32_t* p, uint32_t bits) {
  if ((*p & bits) != bits) atomicOr(p, bits);
}

// the body of the particles stage for workgroup `blk` of one picture (viz_particles_kernel, viz_particles_jobs_kernel)
__device__ __forceinline__ void viz_particles_body(const float* __restrict__ st, int64_t cap, int64_t n, int H, int W,
                                                   int rw, int64_t pw, uint32_t* planes, int fma, const VizStamps& tab,
                                                   int64_t blk) {
  __shared__ uint32_t s_rows[(VIZ_DIRS * VIZ_ROWS + 1) / 2];
  __shared__ uint32_t s_tile[2][VIZ_TH * VIZ_TW];
  __shared__ int s_org[4];   // per plane: first row, first word of the tile
  const int tid = threadIdx.x;
  for (int i = tid; i < (VIZ_DIRS * VIZ_ROWS + 1) / 2; i += 256) s_rows[i] = tab.w[i];
  for (int i = tid; i < 2 * VIZ_TH * VIZ_TW; i += 256) (&s_tile[0][0])[i] = 0;
  if (tid < 4) s_org[tid] = INT_MAX;

  const int64_t p = blk * 256 + tid;
  int kind = -1, cx = 0, cy = 0, di = 0;   // kind 0: arrow, 1: dot
  if (p < n) {
    const float sc = st[TDR_ST_SCALE * cap + p];
    const float x = st[TDR_ST_DX * cap + p] * sc + st[TDR_ST_INIT_X * cap + p];   // mlState (state_particle.cpp:98-102)
    const float y = st[TDR_ST_DY * cap + p] * sc + st[TDR_ST_INIT_Y * cap + p];
    const float th = st[TDR_ST_THETA * cap + p];
    cx = viz_f2i(x);
    cy = viz_f2i((float)H - y);
    if (cx < 0 || cx > W || cy < 0 || cy > H) {
      kind = 1;
      cx = min(max(cx, 5), W - 5);
      cy = min(max(cy, 5), H - 5);
    } else if (fabsf(th) < INFINITY) {   // (a non-finite heading overflows the reference's int: nothing is drawn)
      kind = 0;
      const int dx = (int)(tdr_libm::cosf_v(th, fma) * 5.f), dy = (int)(-tdr_libm::sinf_v(th, fma) * 5.f);
      di = (dx + 5) * 11 + (dy + 5);
    }
  }
  __syncthreads();
  if (kind >= 0) {
    atomicMin(&s_org[2 * kind], max(cy - VIZ_R, 0));
    atomicMin(&s_org[2 * kind + 1], max((cx - VIZ_R) >> 5, 0));
  }
  __syncthreads();
  if (kind >= 0) {
    const int oy = s_org[2 * kind], ow = s_org[2 * kind + 1];
    uint32_t* plane = planes + (int64_t)kind * pw;
    const int x0 = cx - VIZ_R, w0 = x0 >> 5, sh = x0 & 31;
    for (int r = 0; r < VIZ_ROWS; r++) {
      const int y = cy + r - VIZ_R;
      if (y < 0 || y >= H) continue;
      uint32_t m;
      if (kind == 0) {
        const int e = di * VIZ_ROWS + r;
        m = (s_rows[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
      } else {   // Disc: dx^2 + dy^2 <= 5
        const int ar = abs(r - VIZ_R);
        m = ar <= 1 ? 0x1Fu << 4 : ar == 2 ? 0x7u << 5 : 0u;
      }
      if (!m) continue;
      const uint64_t v = (uint64_t)m << sh;
      for (int h = 0; h < 2; h++) {
        const int w = w0 + h;
        uint32_t bits = h ? (uint32_t)(v >> 32) : (uint32_t)v;
        if (w < 0 || w * 32 >= W) continue;
        if (W - w * 32 < 32) bits &= (1u << (W - w * 32)) - 1u;   // clipped at the right edge
        if (!bits) continue;
        const int ty = y - oy, tw = w - ow;
        if (ty < VIZ_TH && tw < VIZ_TW) atomicOr(&s_tile[kind][ty * VIZ_TW + tw], bits);   // (ty, tw >= 0 by the minima)
        else viz_or_global(plane + (int64_t)y * rw + w, bits);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < 2 * VIZ_TH * VIZ_TW; i += 256) {
    const int k = i / (VIZ_TH * VIZ_TW), t = i % (VIZ_TH * VIZ_TW);
    const uint32_t bits = s_tile[k][t];
    if (bits) viz_or_global(planes + (int64_t)k * pw + (int64_t)(s_org[2 * k] + t / VIZ_TW) * rw + s_org[2 * k + 1] + t % VIZ_TW, bits);
  }
}
__global__ __launch_bounds__(256) void viz_particles_kernel(const float* __restrict__ st, int64_t cap, int64_t n, int H,
                                                            int W, int rw, int64_t pw, uint32_t* planes, int fma,
                                                            VizStamps tab) {
  viz_particles_body(st, cap, n, H, W, rw, pw, planes, fma, tab, blockIdx.x);
}

// ---- overlay segments ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t viz_min64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t viz_max64(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ __forceinline__ int64_t viz_floordiv(int64_t a, int64_t b) {
  int64_t q = a / b;
  if ((a % b != 0) && ((a < 0) != (b < 0))) q--;
  return q;
}
// One workgroup per segment {ax, ay, bx, by, plane}.  Along the segment's major axis one thread per coordinate t (one
// beyond either end, for the round caps) tests the pixels within -2 .. +3 of the line's floor there: a covered pixel is
// within 1 of the line at right angles, which is within sqrt(2) along the minor axis.
__device__ __forceinline__ void viz_segment_body(int64_t ax, int64_t ay, int64_t bx, int64_t by, int plane, int H, int W,
                                                 int rw, int64_t pw, uint32_t* planes) {
  if (plane < 0 || plane > 3) return;
  if (ax < -VIZ_LIM || ax > VIZ_LIM || ay < -VIZ_LIM || ay > VIZ_LIM || bx < -VIZ_LIM || bx > VIZ_LIM || by < -VIZ_LIM ||
      by > VIZ_LIM)
    return;
  const int64_t ux = bx - ax, uy = by - ay;
  const bool xmaj = (ux < 0 ? -ux : ux) >= (uy < 0 ? -uy : uy);
  const int64_t a_maj = xmaj ? ax : ay, a_min = xmaj ? ay : ax, b_maj = xmaj ? bx : by;
  const int64_t u_maj = xmaj ? ux : uy, u_min = xmaj ? uy : ux;
  const int64_t lim_maj = xmaj ? W : H, lim_min = xmaj ? H : W;
  const int64_t lo = viz_max64(viz_min64(a_maj, b_maj) - 1, 0), hi = viz_min64(viz_max64(a_maj, b_maj) + 1, lim_maj - 1);
  uint32_t* pl = planes + (int64_t)plane * pw;
  for (int64_t t = lo + threadIdx.x; t <= hi; t += 256) {
    const int64_t c = u_maj == 0 ? a_min : a_min + viz_floordiv((t - a_maj) * u_min, u_maj);
    for (int64_t q = viz_max64(c - 2, 0); q <= viz_min64(c + 3, lim_min - 1); q++) {
      const int64_t px = xmaj ? t : q, py = xmaj ? q : t;
      if (viz_covered(ax, ay, bx, by, px, py)) viz_or_global(pl + py * rw + (px >> 5), 1u << (px & 31));
    }
  }
}
__global__ __launch_bounds__(256) void viz_segments_kernel(const int32_t* __restrict__ segs, int H, int W, int rw,
                                                           int64_t pw, uint32_t* planes) {
  const int32_t* s = segs + 5 * (int64_t)blockIdx.x;
  viz_segment_body(s[0], s[1], s[2], s[3], s[4], H, W, rw, pw, planes);
}

// ---- compose -----------------------------------------------------------------------------------------------------------
// layers, later over earlier: background, plane 0 red, plane 1 green, plane 2 blue, plane 3 green; colours as b | g << 8 | r << 16
__device__ __forceinline__ uint32_t viz_colour(uint32_t bits, uint32_t bg) {
  if (bits & 8u) return 0x00FF00u;
  if (bits & 4u) return 0x0000FFu;
  if (bits & 2u) return 0x00FF00u;
  if (bits & 1u) return 0xFF0000u;
  return bg;
}
__device__ __forceinline__ uint32_t viz_pixel(const uint8_t* __restrict__ bg, const uint32_t* __restrict__ planes, int W,
                                              int rw, int64_t pw, int y, int x) {
  const uint32_t* q = planes + (int64_t)y * rw + (x >> 5);
  const int sh = x & 31;
  const uint32_t bits = ((q[0] >> sh) & 1u) | (((q[pw] >> sh) & 1u) << 1) | (((q[2 * pw] >> sh) & 1u) << 2) |
                        (((q[3 * pw] >> sh) & 1u) << 3);
  if (bits) return viz_colour(bits, 0);
  const uint8_t* b = bg + ((int64_t)y * W + x) * 3;
  return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16);
}

// same size, any width: one thread per pixel
__device__ __forceinline__ void viz_compose_copy_body(const uint8_t* __restrict__ bg, int H, int W, int rw, int64_t pw,
                                                      const uint32_t* __restrict__ planes, uint8_t* __restrict__ out,
                                                      int64_t i) {
  if (i >= (int64_t)H * W) return;
  const uint32_t c = viz_pixel(bg, planes, W, rw, pw, (int)(i / W), (int)(i % W));
  out[3 * i] = (uint8_t)c;
  out[3 * i + 1] = (uint8_t)(c >> 8);
  out[3 * i + 2] = (uint8_t)(c >> 16);
}
__global__ __launch_bounds__(256) void viz_compose_copy_kernel(const uint8_t* __restrict__ bg, int H, int W, int rw,
                                                               int64_t pw, const uint32_t* __restrict__ planes,
                                                               uint8_t* __restrict__ out) {
  viz_compose_copy_body(bg, H, W, rw, pw, planes, out, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// same size, W a multiple of 16 and 16-byte aligned images: one thread per 16 pixels = three 16-byte loads and stores;
// the eight threads of a 128-pixel group read the same 16 bytes of every plane
__device__ __forceinline__ void viz_compose_copy16_body(const uint8_t* __restrict__ bg, int H, int W, int rw, int64_t pw,
                                                        const uint32_t* __restrict__ planes, uint8_t* __restrict__ out,
                                                        int64_t i) {
  const int g = W / 16;
  if (i >= (int64_t)H * g) return;
  const int y = (int)(i / g), xb = (int)(i % g);
  uint32_t m[4];
  for (int k = 0; k < 4; k++) {
    const uint4 v = *reinterpret_cast<const uint4*>(planes + k * pw + (int64_t)y * rw + (xb >> 3) * 4);
    const int c = (xb >> 1) & 3;
    const uint32_t word = c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w;
    m[k] = (word >> (16 * (xb & 1))) & 0xFFFFu;
  }
  const uint4* src = reinterpret_cast<const uint4*>(bg + ((int64_t)y * W + (int64_t)xb * 16) * 3);
  uint4* dst = reinterpret_cast<uint4*>(out + ((int64_t)y * W + (int64_t)xb * 16) * 3);
  uint4 a = src[0], b = src[1], c = src[2];
  if (m[0] | m[1] | m[2] | m[3]) {
    uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
    for (int px = 0; px < 16; px++) {
      const uint32_t bits = ((m[0] >> px) & 1u) | (((m[1] >> px) & 1u) << 1) | (((m[2] >> px) & 1u) << 2) |
                            (((m[3] >> px) & 1u) << 3);
      if (!bits) continue;
      const uint32_t col = viz_colour(bits, 0);
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        const int byte = 3 * px + ch;
        w[byte >> 2] = (w[byte >> 2] & ~(0xFFu << (8 * (byte & 3)))) | (((col >> (8 * ch)) & 0xFFu) << (8 * (byte & 3)));
      }
    }
    a = make_uint4(w[0], w[1], w[2], w[3]);
    b = make_uint4(w[4], w[5], w[6], w[7]);
    c = make_uint4(w[8], w[9], w[10], w[11]);
  }
  dst[0] = a;
  dst[1] = b;
  dst[2] = c;
}
__global__ __launch_bounds__(256) void viz_compose_copy16_kernel(const uint8_t* __restrict__ bg, int H, int W, int rw,
                                                                 int64_t pw, const uint32_t* __restrict__ planes,
                                                                 uint8_t* __restrict__ out) {
  viz_compose_copy16_body(bg, H, W, rw, pw, planes, out, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// the taps of output coordinate o on an axis of n_in source and n_out output pixels: s0, s1 and the weight a1 of s1 (of 2048)
__device__ __forceinline__ void viz_taps(int o, int n_in, int n_out, int& s0, int& s1, int& a1) {
  float f = (float)(((double)o + 0.5) * ((double)n_in / (double)n_out) - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= n_in - 1) { s = n_in - 1; f = 0.f; }
  s0 = s;
  s1 = min(s + 1, n_in - 1);
  a1 = (int)rintf(f * 2048.f);
}
// another size: one thread per output pixel composes its four taps
__device__ __forceinline__ void viz_compose_resize_body(const uint8_t* __restrict__ bg, int H, int W, int rw, int64_t pw,
                                                        const uint32_t* __restrict__ planes, int out_h, int out_w,
                                                        uint8_t* __restrict__ out, int64_t i) {
  if (i >= (int64_t)out_h * out_w) return;
  int x0, x1, ax1, y0, y1, ay1;
  viz_taps((int)(i % out_w), W, out_w, x0, x1, ax1);
  viz_taps((int)(i / out_w), H, out_h, y0, y1, ay1);
  const uint32_t ax0 = 2048u - ax1, ay0 = 2048u - ay1;
  const uint32_t c00 = viz_pixel(bg, planes, W, rw, pw, y0, x0), c01 = viz_pixel(bg, planes, W, rw, pw, y0, x1);
  const uint32_t c10 = viz_pixel(bg, planes, W, rw, pw, y1, x0), c11 = viz_pixel(bg, planes, W, rw, pw, y1, x1);
  for (int ch = 0; ch < 3; ch++) {
    const int sh = 8 * ch;
    const uint32_t v = ay0 * (ax0 * ((c00 >> sh) & 0xFFu) + (uint32_t)ax1 * ((c01 >> sh) & 0xFFu)) +
                       (uint32_t)ay1 * (ax0 * ((c10 >> sh) & 0xFFu) + (uint32_t)ax1 * ((c11 >> sh) & 0xFFu));
    out[3 * i + ch] = (uint8_t)((v + (1u << 21)) >> 22);
  }
}
__global__ __launch_bounds__(256) void viz_compose_resize_kernel(const uint8_t* __restrict__ bg, int H, int W, int rw,
                                                                 int64_t pw, const uint32_t* __restrict__ planes,
                                                                 int out_h, int out_w, uint8_t* __restrict__ out) {
  viz_compose_resize_body(bg, H, W, rw, pw, planes, out_h, out_w, out, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// ---- the job-table forms: k pictures in one launch per stage (blockIdx.y = the job) --------------------------------------
__device__ __forceinline__ bool viz_job_ok(const tdr_viz_job& j) {
  return j.planes && j.H >= 11 && j.W >= 11 && j.H <= VIZ_MAX_DIM && j.W <= VIZ_MAX_DIM;
}

__global__ __launch_bounds__(256) void viz_particles_jobs_kernel(const tdr_viz_job* __restrict__ jobs, int fma,
                                                                 VizStamps tab) {
  const tdr_viz_job j = jobs[blockIdx.y];
  if (!viz_job_ok(j) || !j.st || j.n > j.cap || (int64_t)blockIdx.x * 256 >= j.n) return;   // (the whole workgroup leaves)
  const int rw = viz_row_words(j.W);
  viz_particles_body(j.st, j.cap, j.n, j.H, j.W, rw, (int64_t)j.H * rw, j.planes, fma, tab, blockIdx.x);
}

// Arrow(-dir, dir) per dir as offsets from pt: the three segments' {x1, y1, x2, y2} (|offset| <= 10)
struct VizArrowTab {
  uint32_t w[(VIZ_DIRS * 12 + 3) / 4];   // int8 offs[VIZ_DIRS][12]
};
const VizArrowTab& viz_arrow_tab() {
  static VizArrowTab tab;
  static std::once_flag once;
  std::call_once(once, [] {
    std::memset(&tab, 0, sizeof(tab));
    for (int dx = -5; dx <= 5; dx++)
      for (int dy = -5; dy <= 5; dy++) {
        int64_t s[12];
        viz_arrow(-dx, -dy, dx, dy, s);
        for (int i = 0; i < 12; i++) {
          const int e = ((dx + 5) * 11 + (dy + 5)) * 12 + i;
          tab.w[e / 4] |= ((uint32_t)(s[i] & 0xFF)) << (8 * (e & 3));
        }
      }
  });
  return tab;
}

// Workgroup x of job y draws segment x of the job's list; the three after the list are the heading arrow of the job's
// max-likelihood state, by the particle's rule (viz_particles_body) and tdr_viz_overlay_host's range checks.
__global__ __launch_bounds__(256) void viz_segments_jobs_kernel(const tdr_viz_job* __restrict__ jobs, int fma,
                                                                VizArrowTab tab) {
  const tdr_viz_job j = jobs[blockIdx.y];
  if (!viz_job_ok(j) || j.n_segs < 0) return;
  const int rw = viz_row_words(j.W);
  const int64_t pw = (int64_t)j.H * rw;
  const int i = (int)blockIdx.x;
  if (i < j.n_segs) {
    if (!j.segs) return;
    const int32_t* s = j.segs + 5 * (int64_t)i;
    viz_segment_body(s[0], s[1], s[2], s[3], s[4], j.H, j.W, rw, pw, j.planes);
    return;
  }
  const int t = i - j.n_segs;
  if (t >= 3 || !j.best) return;
  const float x = j.best[0], y = j.best[1], th = j.best[2];
  if (!(fabsf(th) < INFINITY)) return;
  const int64_t cx = viz_f2i(x), cy = viz_f2i((float)j.H - y);
  const int dx = (int)(tdr_libm::cosf_v(th, fma) * 5.f), dy = (int)(-tdr_libm::sinf_v(th, fma) * 5.f);
  auto in_range = [](int64_t v) { return v >= -VIZ_LIM && v <= VIZ_LIM; };
  if (!in_range(cx - dx) || !in_range(cy - dy) || !in_range(cx + dx) || !in_range(cy + dy)) return;
  int64_t q[4];
  for (int c = 0; c < 4; c++) {
    const int e = ((dx + 5) * 11 + (dy + 5)) * 12 + 4 * t + c;
    q[c] = (int64_t)(int8_t)((tab.w[e >> 2] >> (8 * (e & 3))) & 0xFFu) + ((c & 1) ? cy : cx);
  }
  viz_segment_body(q[0], q[1], q[2], q[3], 2, j.H, j.W, rw, pw, j.planes);   // (it drops a segment beyond +-VIZ_LIM itself)
}

__global__ __launch_bounds__(256) void viz_compose_jobs_kernel(const tdr_viz_job* __restrict__ jobs) {
  const tdr_viz_job j = jobs[blockIdx.y];
  if (!viz_job_ok(j) || !j.background || !j.out || j.out_h < 1 || j.out_w < 1 || j.out_h > VIZ_MAX_DIM || j.out_w > VIZ_MAX_DIM)
    return;
  const int rw = viz_row_words(j.W);
  const int64_t pw = (int64_t)j.H * rw, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j.out_h == j.H && j.out_w == j.W) {   // the choices of tdr_k_viz_compose
    if (j.W % 16 == 0 && (((uintptr_t)j.background | (uintptr_t)j.out) & 15) == 0)
      viz_compose_copy16_body(j.background, j.H, j.W, rw, pw, j.planes, j.out, i);
    else
      viz_compose_copy_body(j.background, j.H, j.W, rw, pw, j.planes, j.out, i);
  } else {
    viz_compose_resize_body(j.background, j.H, j.W, rw, pw, j.planes, j.out_h, j.out_w, j.out, i);
  }
}

// ---- the fleet picture: k robots' planes 0 - 2 and one green plane over one background (include/tdr.h) ------------------
// Layer-major, the highest index wins: green, then per layer estimate / dots / arrows the robots from k - 1 down.  The
// image is a function of the planes alone.  A workgroup stages what every pixel needs of the k jobs in LDS: the plane
// pointers (a job of another size, or without planes, gets none and draws nothing) and the colours as b | g << 8 | r << 16.
struct VizPalette {
  uint32_t w[TDR_FLEET_MAX * 9 / 4];   // uint8 [TDR_FLEET_MAX][3][3]
};
struct VizFleet {
  const uint32_t* planes[TDR_FLEET_MAX];
  uint32_t col[TDR_FLEET_MAX * 3];
};
__device__ __forceinline__ void viz_fleet_stage(const tdr_viz_job* __restrict__ jobs, int k, const VizPalette& pal, int H,
                                                int W, VizFleet& s) {
  for (int i = threadIdx.x; i < k; i += 256) {
    const uint32_t* p = jobs[i].planes;
    s.planes[i] = (jobs[i].H == H && jobs[i].W == W) ? p : nullptr;
  }
  for (int i = threadIdx.x; i < 3 * k; i += 256) {
    uint32_t c = 0;
    for (int ch = 0; ch < 3; ch++) {
      const int byte = 3 * i + ch;
      c |= ((pal.w[byte >> 2] >> (8 * (byte & 3))) & 0xFFu) << (8 * ch);
    }
    s.col[i] = c;
  }
  __syncthreads();
}

// one pixel: the colour of the first layer that covers it, else the background's
__device__ __forceinline__ uint32_t viz_fleet_pixel(const VizFleet& s, int k, const uint8_t* __restrict__ bg,
                                                    const uint32_t* __restrict__ green, int W, int rw, int64_t pw, int y,
                                                    int x) {
  const int64_t o = (int64_t)y * rw + (x >> 5);
  const int sh = x & 31;
  if ((green[o] >> sh) & 1u) return 0x00FF00u;
  for (int l = 2; l >= 0; l--)
    for (int r = k - 1; r >= 0; r--) {
      const uint32_t* p = s.planes[r];
      if (p && ((p[l * pw + o] >> sh) & 1u)) return s.col[3 * r + l];
    }
  const uint8_t* b = bg + ((int64_t)y * W + x) * 3;
  return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16);
}

__global__ __launch_bounds__(256) void viz_fleet_copy_kernel(const tdr_viz_job* __restrict__ jobs, int k, VizPalette pal,
                                                             const uint8_t* __restrict__ bg, int H, int W, int rw,
                                                             int64_t pw, const uint32_t* __restrict__ green,
                                                             uint8_t* __restrict__ out) {
  __shared__ VizFleet s;
  viz_fleet_stage(jobs, k, pal, H, W, s);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)H * W) return;
  const uint32_t c = viz_fleet_pixel(s, k, bg, green, W, rw, pw, (int)(i / W), (int)(i % W));
  out[3 * i] = (uint8_t)c;
  out[3 * i + 1] = (uint8_t)(c >> 8);
  out[3 * i + 2] = (uint8_t)(c >> 16);
}

// the pixels of mask m (bit px = pixel px of the group) of a 16-pixel group's twelve words take colour col
__device__ __forceinline__ void viz_paint16(uint32_t w[12], uint32_t m, uint32_t col) {
#pragma unroll
  for (int px = 0; px < 16; px++) {
    if (!((m >> px) & 1u)) continue;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const int byte = 3 * px + ch;
      w[byte >> 2] = (w[byte >> 2] & ~(0xFFu << (8 * (byte & 3)))) | (((col >> (8 * ch)) & 0xFFu) << (8 * (byte & 3)));
    }
  }
}

// same size, W a multiple of 16, 16-byte aligned images: one thread per 16 pixels = three 16-byte loads and stores of the
// image and, per plane, the half word of the group's 16 pixels.  `undecided` holds the pixels no layer has claimed yet;
// the walk over layers and robots ends when it is empty.
__global__ __launch_bounds__(256) void viz_fleet_copy16_kernel(const tdr_viz_job* __restrict__ jobs, int k, VizPalette pal,
                                                               const uint8_t* __restrict__ bg, int H, int W, int rw,
                                                               int64_t pw, const uint32_t* __restrict__ green,
                                                               uint8_t* __restrict__ out) {
  __shared__ VizFleet s;
  viz_fleet_stage(jobs, k, pal, H, W, s);
  const int g = W / 16;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)H * g) return;
  const int y = (int)(i / g), xb = (int)(i % g);
  const int64_t o = (int64_t)y * rw + (xb >> 1);
  const int sh = 16 * (xb & 1);
  const uint4* src = reinterpret_cast<const uint4*>(bg + ((int64_t)y * W + (int64_t)xb * 16) * 3);
  uint4* dst = reinterpret_cast<uint4*>(out + ((int64_t)y * W + (int64_t)xb * 16) * 3);
  const uint4 a = src[0], b = src[1], c = src[2];
  uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
  uint32_t undecided = 0xFFFFu;
  uint32_t m = (green[o] >> sh) & undecided;
  if (m) {
    viz_paint16(w, m, 0x00FF00u);
    undecided &= ~m;
  }
  for (int l = 2; l >= 0 && undecided; l--)
    for (int r = k - 1; r >= 0 && undecided; r--) {
      const uint32_t* p = s.planes[r];
      if (!p) continue;
      m = (p[l * pw + o] >> sh) & undecided;
      if (!m) continue;
      viz_paint16(w, m, s.col[3 * r + l]);
      undecided &= ~m;
    }
  dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
  dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
  dst[2] = make_uint4(w[8], w[9], w[10], w[11]);
}

// another size: one thread per output pixel composes its four taps (viz_compose_resize_body's arithmetic)
__global__ __launch_bounds__(256) void viz_fleet_resize_kernel(const tdr_viz_job* __restrict__ jobs, int k, VizPalette pal,
                                                               const uint8_t* __restrict__ bg, int H, int W, int rw,
                                                               int64_t pw, const uint32_t* __restrict__ green, int out_h,
                                                               int out_w, uint8_t* __restrict__ out) {
  __shared__ VizFleet s;
  viz_fleet_stage(jobs, k, pal, H, W, s);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)out_h * out_w) return;
  int x0, x1, ax1, y0, y1, ay1;
  viz_taps((int)(i % out_w), W, out_w, x0, x1, ax1);
  viz_taps((int)(i / out_w), H, out_h, y0, y1, ay1);
  const uint32_t ax0 = 2048u - ax1, ay0 = 2048u - ay1;
  const uint32_t c00 = viz_fleet_pixel(s, k, bg, green, W, rw, pw, y0, x0), c01 = viz_fleet_pixel(s, k, bg, green, W, rw, pw, y0, x1);
  const uint32_t c10 = viz_fleet_pixel(s, k, bg, green, W, rw, pw, y1, x0), c11 = viz_fleet_pixel(s, k, bg, green, W, rw, pw, y1, x1);
  for (int ch = 0; ch < 3; ch++) {
    const int sh = 8 * ch;
    const uint32_t v = ay0 * (ax0 * ((c00 >> sh) & 0xFFu) + (uint32_t)ax1 * ((c01 >> sh) & 0xFFu)) +
                       (uint32_t)ay1 * (ax0 * ((c10 >> sh) & 0xFFu) + (uint32_t)ax1 * ((c11 >> sh) & 0xFFu));
    out[3 * i + ch] = (uint8_t)((v + (1u << 21)) >> 22);
  }
}

bool viz_dims_ok(int H, int W) { return H >= 11 && W >= 11 && H <= VIZ_MAX_DIM && W <= VIZ_MAX_DIM; }

}  // namespace

extern "C" size_t tdr_viz_plane_words(int H, int W) {
  if (H < 1 || W < 1 || H > VIZ_MAX_DIM || W > VIZ_MAX_DIM) return 0;
  return (size_t)H * viz_row_words(W);
}

extern "C" int tdr_viz_arrow_host(int dx, int dy, int32_t segs[12]) {
  if (!segs || dx < -VIZ_LIM || dx > VIZ_LIM || dy < -VIZ_LIM || dy > VIZ_LIM)
    return fail(TDR_ERR_ARG, "viz_arrow_host: bad arguments");
  int64_t s[12];
  viz_arrow(-dx, -dy, dx, dy, s);
  for (int i = 0; i < 12; i++) segs[i] = (int32_t)s[i];
  return TDR_OK;
}

extern "C" int tdr_viz_overlay_host(const float* means, const float* covs, int k, const float* best,
                                    const int32_t* arrows, int m, int H, int32_t* segs, int capacity, int* n_out) {
  if (k < 0 || m < 0 || (k > 0 && (!means || !covs)) || (m > 0 && !arrows) || !n_out || capacity < 0 ||
      (capacity > 0 && !segs))
    return fail(TDR_ERR_ARG, "viz_overlay_host: bad arguments");
  int n = 0;
  bool full = false;
  auto in_range = [](int64_t v) { return v >= -VIZ_LIM && v <= VIZ_LIM; };
  auto push = [&](int64_t ax, int64_t ay, int64_t bx, int64_t by, int plane) {
    if (!in_range(ax) || !in_range(ay) || !in_range(bx) || !in_range(by)) return;
    if (n >= capacity) { full = true; return; }
    int32_t* o = segs + 5 * (size_t)n++;
    o[0] = (int32_t)ax; o[1] = (int32_t)ay; o[2] = (int32_t)bx; o[3] = (int32_t)by; o[4] = plane;
  };
  auto arrow = [&](int64_t x1, int64_t y1, int64_t x2, int64_t y2, int plane) {
    if (!in_range(x1) || !in_range(y1) || !in_range(x2) || !in_range(y2)) return;
    int64_t s[12];
    viz_arrow(x1, y1, x2, y2, s);
    for (int i = 0; i < 3; i++) push(s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3], plane);
  };
  const int fma = tdr_libm_fma();
  auto heading = [&](float x, float y, float theta, int plane) {   // the `arrow` of particle_viz.h at mlState (x, y, theta)
    if (!(std::fabs(theta) < INFINITY)) return;
    const int64_t cx = viz_f2i(x), cy = viz_f2i((float)H - y);
    const int dx = (int)(tdr_libm::cosf_v(theta, fma) * 5.f), dy = (int)(-tdr_libm::sinf_v(theta, fma) * 5.f);
    arrow(cx - dx, cy - dy, cx + dx, cy + dy, plane);
  };
  for (int g = 0; g < k; g++) {
    const float a = covs[9 * g], b = covs[9 * g + 1], d = covs[9 * g + 4];
    const float tr = a + d, e = (a - d) * (a - d) / 4 + b * b;
    const float disc = std::sqrt(0.f < e ? e : 0.f);
    const float l0 = tr / 2 - disc, l1 = tr / 2 + disc;
    if (l0 < 0 || l1 < 0) break;   // (the reference stops at the first component that is not PSD)
    float vx = b, vy = l0 - a;
    if (std::fabs(vx) + std::fabs(vy) < 1e-12f) { vx = 1; vy = 0; }
    const double phi = (double)std::atan2(-vy, vx);
    const int64_t cx = viz_f2i(means[3 * g]), cy = viz_f2i((float)H - means[3 * g + 1]);
    const double ea = (double)(2 * (int64_t)viz_f2i(std::sqrt(l0))), eb = (double)(2 * (int64_t)viz_f2i(std::sqrt(l1)));
    const double cp = std::cos(phi), sp = std::sin(phi);
    int64_t vxs[72], vys[72];
    for (int j = 0; j < 72; j++) {
      const double t = j * (M_PI / 36), ct = std::cos(t), st = std::sin(t);
      const double X = ((double)cx + (ea * ct) * cp) - (eb * st) * sp;
      const double Y = ((double)cy + (ea * ct) * sp) + (eb * st) * cp;
      vxs[j] = std::fabs(X) <= VIZ_LIM ? std::lrint(X) : INT64_MAX;   // (out of range, NaN included: its edges are dropped)
      vys[j] = std::fabs(Y) <= VIZ_LIM ? std::lrint(Y) : INT64_MAX;
    }
    for (int j = 0; j < 72; j++) push(vxs[j], vys[j], vxs[(j + 1) % 72], vys[(j + 1) % 72], 2);
    heading(means[3 * g], means[3 * g + 1], means[3 * g + 2], 2);
  }
  if (best) heading(best[0], best[1], best[2], 2);
  for (int i = 0; i < m; i++) arrow(arrows[4 * i], arrows[4 * i + 1], arrows[4 * i + 2], arrows[4 * i + 3], 3);
  *n_out = n;
  if (full) return fail(TDR_ERR_ARG, "viz_overlay_host: more than %d segments", capacity);
  return TDR_OK;
}

extern "C" int tdr_k_viz_particles(const float* st, int64_t cap, int64_t n, int H, int W, uint32_t* planes, void* stream) {
  if (!st || !planes || n < 0 || n > cap || !viz_dims_ok(H, W)) return fail(TDR_ERR_ARG, "viz_particles: bad arguments");
  if (n == 0) return TDR_OK;
  hipLaunchKernelGGL(viz_particles_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, st, cap, n, H,
                     W, viz_row_words(W), (int64_t)tdr_viz_plane_words(H, W), planes, tdr_libm_fma(), viz_stamps());
  LAUNCH_CHECK("viz_particles");
  return TDR_OK;
}

extern "C" int tdr_k_viz_segments(const int32_t* segs, int m, int H, int W, uint32_t* planes, void* stream) {
  if (m < 0 || (m > 0 && !segs) || !planes || !viz_dims_ok(H, W)) return fail(TDR_ERR_ARG, "viz_segments: bad arguments");
  if (m == 0) return TDR_OK;
  hipLaunchKernelGGL(viz_segments_kernel, dim3((unsigned)m), dim3(256), 0, (hipStream_t)stream, segs, H, W,
                     viz_row_words(W), (int64_t)tdr_viz_plane_words(H, W), planes);
  LAUNCH_CHECK("viz_segments");
  return TDR_OK;
}

extern "C" int tdr_k_viz_compose(const uint8_t* background, int H, int W, const uint32_t* planes, int out_h, int out_w,
                                 uint8_t* out_bgr, void* stream) {
  if (!background || !planes || !out_bgr || !viz_dims_ok(H, W) || out_h < 1 || out_w < 1 || out_h > VIZ_MAX_DIM ||
      out_w > VIZ_MAX_DIM)
    return fail(TDR_ERR_ARG, "viz_compose: bad arguments");
  if (((uintptr_t)planes & 15) != 0) return fail(TDR_ERR_ARG, "viz_compose: the planes are not 16-byte aligned");
  const int rw = viz_row_words(W);
  const int64_t pw = (int64_t)tdr_viz_plane_words(H, W);
  hipStream_t s = (hipStream_t)stream;
  if (out_h == H && out_w == W) {
    if (W % 16 == 0 && (((uintptr_t)background | (uintptr_t)out_bgr) & 15) == 0)
      hipLaunchKernelGGL(viz_compose_copy16_kernel, dim3((unsigned)cdiv((int64_t)H * (W / 16), 256)), dim3(256), 0, s,
                         background, H, W, rw, pw, planes, out_bgr);
    else
      hipLaunchKernelGGL(viz_compose_copy_kernel, dim3((unsigned)cdiv((int64_t)H * W, 256)), dim3(256), 0, s, background,
                         H, W, rw, pw, planes, out_bgr);
  } else {
    hipLaunchKernelGGL(viz_compose_resize_kernel, dim3((unsigned)cdiv((int64_t)out_h * out_w, 256)), dim3(256), 0, s,
                       background, H, W, rw, pw, planes, out_h, out_w, out_bgr);
  }
  LAUNCH_CHECK("viz_compose");
  return TDR_OK;
}

static int viz_jobs_args(const char* who, const tdr_viz_job* jobs, int k, int64_t extent) {
  if (!jobs) return fail(TDR_ERR_ARG, "%s: null job array", who);
  if (k < 1 || k > 65535) return fail(TDR_ERR_ARG, "%s: k = %d (1 .. 65535 jobs)", who, k);
  if (extent < 0 || cdiv(extent, 256) > INT_MAX) return fail(TDR_ERR_ARG, "%s: bad extent %lld", who, (long long)extent);
  return TDR_OK;
}

extern "C" int tdr_k_viz_particles_jobs(const tdr_viz_job* jobs_dev, int k, int64_t max_n, void* stream) {
  if (int rc = viz_jobs_args("viz_particles_jobs", jobs_dev, k, max_n)) return rc;
  if (max_n == 0) return TDR_OK;
  hipLaunchKernelGGL(viz_particles_jobs_kernel, dim3((unsigned)cdiv(max_n, 256), (unsigned)k), dim3(256), 0,
                     (hipStream_t)stream, jobs_dev, tdr_libm_fma(), viz_stamps());
  LAUNCH_CHECK("viz_particles_jobs");
  return TDR_OK;
}

extern "C" int tdr_k_viz_segments_jobs(const tdr_viz_job* jobs_dev, int k, int max_segs, void* stream) {
  if (int rc = viz_jobs_args("viz_segments_jobs", jobs_dev, k, max_segs)) return rc;
  hipLaunchKernelGGL(viz_segments_jobs_kernel, dim3((unsigned)max_segs + 3u, (unsigned)k), dim3(256), 0,
                     (hipStream_t)stream, jobs_dev, tdr_libm_fma(), viz_arrow_tab());
  LAUNCH_CHECK("viz_segments_jobs");
  return TDR_OK;
}

extern "C" int tdr_k_viz_compose_jobs(const tdr_viz_job* jobs_dev, int k, int64_t max_out_pixels, void* stream) {
  if (int rc = viz_jobs_args("viz_compose_jobs", jobs_dev, k, max_out_pixels)) return rc;
  if (max_out_pixels == 0) return TDR_OK;
  hipLaunchKernelGGL(viz_compose_jobs_kernel, dim3((unsigned)cdiv(max_out_pixels, 256), (unsigned)k), dim3(256), 0,
                     (hipStream_t)stream, jobs_dev);
  LAUNCH_CHECK("viz_compose_jobs");
  return TDR_OK;
}

extern "C" int tdr_k_viz_compose_fleet(const tdr_viz_job* jobs_dev, int k, const uint8_t* palette_host,
                                       const uint8_t* background, int H, int W, const uint32_t* green_plane, int out_h,
                                       int out_w, uint8_t* out_bgr, void* stream) {
  if (!jobs_dev || !palette_host || !background || !green_plane || !out_bgr)
    return fail(TDR_ERR_ARG, "viz_compose_fleet: null argument");
  if (k < 1 || k > TDR_FLEET_MAX) return fail(TDR_ERR_ARG, "viz_compose_fleet: k = %d (1 .. %d robots)", k, TDR_FLEET_MAX);
  if (!viz_dims_ok(H, W) || out_h < 1 || out_w < 1 || out_h > VIZ_MAX_DIM || out_w > VIZ_MAX_DIM)
    return fail(TDR_ERR_ARG, "viz_compose_fleet: a %d x %d image published as %d x %d", H, W, out_h, out_w);
  VizPalette pal;
  std::memset(&pal, 0, sizeof(pal));
  std::memcpy(&pal, palette_host, (size_t)9 * k);
  const int rw = viz_row_words(W);
  const int64_t pw = (int64_t)tdr_viz_plane_words(H, W);
  hipStream_t s = (hipStream_t)stream;
  if (out_h == H && out_w == W) {   // the choices of tdr_k_viz_compose
    if (W % 16 == 0 && (((uintptr_t)background | (uintptr_t)out_bgr) & 15) == 0)
      hipLaunchKernelGGL(viz_fleet_copy16_kernel, dim3((unsigned)cdiv((int64_t)H * (W / 16), 256)), dim3(256), 0, s,
                         jobs_dev, k, pal, background, H, W, rw, pw, green_plane, out_bgr);
    else
      hipLaunchKernelGGL(viz_fleet_copy_kernel, dim3((unsigned)cdiv((int64_t)H * W, 256)), dim3(256), 0, s, jobs_dev, k,
                         pal, background, H, W, rw, pw, green_plane, out_bgr);
  } else {
    hipLaunchKernelGGL(viz_fleet_resize_kernel, dim3((unsigned)cdiv((int64_t)out_h * out_w, 256)), dim3(256), 0, s,
                       jobs_dev, k, pal, background, H, W, rw, pw, green_plane, out_h, out_w, out_bgr);
  }
  LAUNCH_CHECK("viz_compose_fleet");
  return TDR_OK;
}
