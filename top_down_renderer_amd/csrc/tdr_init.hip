// tdr_init.hip — ParticleFilter::initializeParticles (src/particle_filter.cpp:19-84) on the device: the same bytes and the
// same generator position as the serial host loop (tdr_init_particles_host, tdr_filter.hip), with the StateParticle
// constructor (src/state_particle.cpp:3-49) for every draw the reference makes, burnt ones included.
//
// The serial loop is a chain of CONSTRUCTIONS over the generator's word stream.  A construction that starts at word p
// consumes one uniform word for the scale when the scale is unknown (s = p + sigma), then tries until its position is on
// a road cell, then — with a given heading — one accepted Marsaglia attempt for theta.  A uniform try takes two words; a
// normal try is one accepted attempt (the attempts before it are rejected ones, two words each).  Both are the test of a
// two-word window at one position, so with
//   G[i]  the try that starts at word i succeeds (uniform: on road; normal: the attempt is accepted and on road),
//   A[i]  the attempt at word i is accepted,
// and NextG(i) / NextA(i) the first j >= i of the SAME PARITY with G[j] / A[j], the construction that starts at p ends at
//   f(p) = theta given ? NextA(NextG(s) + 2) + 2 : NextG(s) + 2.
// The constructions are the chain P, f(P), f(f(P)), ... from the generator's position P; construction K's index decides
// which particle slot it fills (particle_filter.cpp:57-71).  Per WINDOW of W words of the stream:
//   ini_flags_kernel   G and A at every position, and the suffix minimum of the flagged positions per parity inside
//                      2048-word tiles (one workgroup per tile);
//   ini_tail_kernel    the same over the tiles' minima: NextG / NextA at any position in O(1);
//   ini_head_kernel    the construction the previous window left unfinished (its loop or its theta search goes on here)
//                      -> the first construction that starts inside this window;
//   ini_f_kernel       f at every position (INF: it needs words behind the window);
//   ini_lift_kernel    binary lifting: J_m = f^(2^m), m < L;
//   ini_chain_kernel   element k of the chain = J over the bits of k from the head's end; it writes its construction's
//                      particles straight into the SoA planes and, for the chain's last element in the window, the
//                      carried state (construction index, loop or theta phase, position);
//   mt_advance_kernel  (tdr_rng.hip) the generator behind the window's consumed words.
// The workspace is fixed by W (tdr_config_tuning("init_window_words")), never by the particle count; a construction
// whose rejection loop outlasts a window carries its phase and position into the next one.  The host waits for each
// window's "done" flag.
#include "tdr_common.h"
#include "tdr_mt_dev.h"

#define INI_MT_N 624
#define INI_INF 0x7fffffff
#define INI_MAX_NS 16

struct IniParams {
  const float* rec;
  int rf, rows, cols;
  float res, map_w, map_h;
  int normal;                  // init_pos_px_x > 0: positions from N(init_pos_px, cov), else uniform over the map
  float px, py, pcov;
  int theta;                   // init_pos_deg_theta finite
  float deg, dcov;
  int sigma;                   // 1: unknown scale (one uniform word first, its value unused)
  int per, ns;                 // constructions per group (3, or 1 + 2 ns) and particles per group (1, or ns)
  float fixed_scale;
  float sv[INI_MAX_NS];        // unknown scale: the prototype's copies get (float)pow(10., s) for the reference's s loop
  int64_t ktot;                // constructions of the whole call
  int64_t lo, hi, cap;
  float* st;
  int W, L;
};
struct IniCtl {
  int64_t k0;       // the construction at the window's first word ...
  int32_t phase;    // ... 0: starts there, 1: its rejection loop tries there, 2: its theta attempt search goes on there
  int32_t c;        // ini_head_kernel: the first construction that STARTS in the window (-1: none) ...
  int64_t kb;       // ... and its index
  uint32_t consumed;   // words of this window the chain has used up (mt_advance_kernel's input)
  int32_t done;
  int32_t road;     // the map has a road cell
  int32_t pad[9];
};

// TopDownMap::getClassesAtPoint (top_down_map.cpp:159-170) tested for class 1 on the device records (the class-1 slot holds
// the host copy's floats; unknown cells have distance 0 and count as road, as in the reference)
__device__ __forceinline__ bool ini_on_road(const IniParams& q, float x, float y) {
  const int ix = (int)x, iy = (int)y;
  const int c0 = (int)((float)ix / q.res), c1 = (int)((float)iy / q.res);
  if (!(c0 < q.cols && c1 < q.rows && c0 >= 0 && c1 >= 0)) return false;
  return q.rec[((int64_t)(c1 + 1) * (q.cols + 2) + (c0 + 1)) * q.rf + 1] < 1.f;
}
struct IniTry {
  float x, y;        // the try's position (valid when on)
  float z;           // the attempt's first value y * mult (theta)
  bool accepted, on;
};
// the two words at w[i], w[i + 1]: a uniform try, or a Marsaglia attempt (a normal try / the theta draw)
__device__ IniTry ini_try(const IniParams& q, const uint32_t* __restrict__ w, int64_t i, bool need_value) {
  IniTry t;
  const MtAttempt at = mt_attempt(w, i);
  const float c0 = at.c0, c1 = at.c1, ax = at.x, ay = at.y, r2 = at.r2;
  t.accepted = at.ok;
  t.z = 0.f;
  if (t.accepted && (q.normal || need_value)) {
    const float mult = mt_attempt_mult(r2);
    t.z = ay * mult * 1.f + 0.f;
    if (q.normal) {
      const float vx = ax * mult * 1.f + 0.f;
      // std::min(std::max(v * cov + px, 0.f), map_w), std::max / std::min spelled out
      float x = t.z * q.pcov + q.px, y = vx * q.pcov + q.py;
      x = x < 0.f ? 0.f : x;
      x = q.map_w < x ? q.map_w : x;
      y = y < 0.f ? 0.f : y;
      y = q.map_h < y ? q.map_h : y;
      t.x = x;
      t.y = y;
    }
  }
  if (!q.normal) {
    t.x = (c0 * (1.f - 0.f) + 0.f) * q.map_w;   // uniform_dist(gen) * map_w
    t.y = (c1 * (1.f - 0.f) + 0.f) * q.map_h;
  }
  t.on = (q.normal ? t.accepted : true) && ini_on_road(q, t.x, t.y);
  return t;
}

// construction K's particles: the particle of a fixed-scale group, or the ns copies of an unknown-scale prototype
__device__ void ini_write(const IniParams& q, int64_t K, bool position, float a, float b) {
  int64_t i0;
  int cnt;
  if (!q.sigma) {
    if (K % 3 != 1) return;
    i0 = K / 3;
    cnt = 1;
  } else {
    if (K % q.per != 0) return;
    i0 = (K / q.per) * q.ns;
    cnt = q.ns;
  }
  for (int t = 0; t < cnt; t++) {
    const int64_t i = i0 + t;
    if (i < q.lo || i >= q.hi) continue;
    float* o = q.st + (i - q.lo);
    if (position) {
      o[TDR_ST_INIT_X * q.cap] = a;
      o[TDR_ST_INIT_Y * q.cap] = b;
      o[TDR_ST_DX * q.cap] = 0.f;
      o[TDR_ST_DY * q.cap] = 0.f;
      o[TDR_ST_SCALE * q.cap] = q.sigma ? q.sv[t] : q.fixed_scale;
      if (!q.theta) {
        o[TDR_ST_THETA * q.cap] = 0.f;
        o[TDR_ST_HAVE_INIT * q.cap] = 0.f;
      }
    } else {
      o[TDR_ST_THETA * q.cap] = a;
      o[TDR_ST_HAVE_INIT * q.cap] = 1.f;
    }
  }
}
__device__ __forceinline__ void ini_write_theta(const IniParams& q, int64_t K, float z) {
  const float th = z * q.dcov + q.deg;                                      // state_particle.cpp:35
  ini_write(q, K, false, (float)((double)th * (M_PI / 180)), 0.f);          // :37
}

// NextG (kind 0) / NextA (kind 1) at window position i < W
__device__ __forceinline__ int ini_next(const int* __restrict__ loc, const int* __restrict__ tail, int i, int kind) {
  const int v = loc[i];
  return v != INI_INF ? v : tail[(i / INI_TILE + 1) * 4 + 2 * kind + (i & 1)];
}
// the first position >= W of i's parity (W is even)
__device__ __forceinline__ int ini_past(int i, int W) { return i >= W ? i : W + (i & 1); }

__global__ __launch_bounds__(1024) void ini_flags_kernel(const uint32_t* __restrict__ raw, const uint32_t* __restrict__ state,
                                                         IniParams q, int* __restrict__ locG, int* __restrict__ locA,
                                                         int* __restrict__ tile_min) {
  __shared__ int wm[16][4];
  const uint32_t* __restrict__ w = raw + state[INI_MT_N];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int i0 = blockIdx.x * INI_TILE + 2 * t;
  const IniTry e = ini_try(q, w, i0, false), o = ini_try(q, w, i0 + 1, false);
  int v[4] = {e.on ? i0 : INI_INF, o.on ? i0 + 1 : INI_INF, e.accepted ? i0 : INI_INF, o.accepted ? i0 + 1 : INI_INF};
#pragma unroll
  for (int off = 1; off < 64; off <<= 1)
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int u = __shfl_down(v[k], off, 64);
      if (lane + off < 64) v[k] = min(v[k], u);
    }
  if (lane == 0)
    for (int k = 0; k < 4; k++) wm[wave][k] = v[k];
  __syncthreads();
  for (int w2 = wave + 1; w2 < 16; w2++)
    for (int k = 0; k < 4; k++) v[k] = min(v[k], wm[w2][k]);
  locG[i0] = v[0];
  locG[i0 + 1] = v[1];
  locA[i0] = v[2];
  locA[i0 + 1] = v[3];
  if (t == 0)
    for (int k = 0; k < 4; k++) tile_min[blockIdx.x * 4 + k] = v[k];
}
// tail[t][k] = min over tiles >= t of tile_min[.][k]; tail[ntiles][.] = INF.  One workgroup.
__global__ __launch_bounds__(1024) void ini_tail_kernel(const int* __restrict__ tile_min, int ntiles, int* __restrict__ tail) {
  __shared__ int s[4][INI_MAX_TILES];
  for (int i = threadIdx.x; i < ntiles * 4; i += 1024) s[i & 3][i >> 2] = tile_min[i];
  __syncthreads();
  for (int d = 1; d < ntiles; d <<= 1) {
    int v[8];
    for (int r = 0; r < 8; r++) {
      const int i = threadIdx.x + 1024 * (r >> 2), k = r & 3;
      v[r] = i < ntiles ? (i + d < ntiles ? min(s[k][i], s[k][i + d]) : s[k][i]) : INI_INF;
    }
    __syncthreads();
    for (int r = 0; r < 8; r++) {
      const int i = threadIdx.x + 1024 * (r >> 2), k = r & 3;
      if (i < ntiles) s[k][i] = v[r];
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < (ntiles + 1) * 4; i += 1024) tail[i] = (i >> 2) < ntiles ? s[i & 3][i >> 2] : INI_INF;
}

__device__ void ini_carry(IniCtl* ctl, int64_t K, int phase, int at) {
  ctl->k0 = K;
  ctl->phase = phase;
  ctl->consumed = (uint32_t)at;
}
// the rest of construction K from its theta search at window position e (its position is written)
__device__ bool ini_finish_theta(const IniParams& q, const uint32_t* __restrict__ w, const int* __restrict__ locA,
                                 const int* __restrict__ tail, IniCtl* ctl, int64_t K, int e, int* end) {
  if (e >= q.W) { ini_carry(ctl, K, 2, e); return false; }
  const int a = ini_next(locA, tail, e, 1);
  if (a == INI_INF) { ini_carry(ctl, K, 2, ini_past(e, q.W)); return false; }
  ini_write_theta(q, K, ini_try(q, w, a, true).z);
  *end = a + 2;
  return true;
}
// the rest of construction K from its rejection loop at window position s
__device__ bool ini_finish_loop(const IniParams& q, const uint32_t* __restrict__ w, const int* __restrict__ locG,
                                const int* __restrict__ locA, const int* __restrict__ tail, IniCtl* ctl, int64_t K, int s,
                                int* end) {
  if (s >= q.W) { ini_carry(ctl, K, 1, s); return false; }
  const int j = ini_next(locG, tail, s, 0);
  if (j == INI_INF) { ini_carry(ctl, K, 1, ini_past(s, q.W)); return false; }
  const IniTry t = ini_try(q, w, j, false);
  ini_write(q, K, true, t.x, t.y);
  if (!q.theta) { *end = j + 2; return true; }
  return ini_finish_theta(q, w, locA, tail, ctl, K, j + 2, end);
}

__global__ __launch_bounds__(64) void ini_head_kernel(const uint32_t* __restrict__ raw, const uint32_t* __restrict__ state,
                                                      const int* __restrict__ locG, const int* __restrict__ locA,
                                                      const int* __restrict__ tail, IniParams q, IniCtl* ctl) {
  if (threadIdx.x != 0) return;
  const uint32_t* __restrict__ w = raw + state[INI_MT_N];
  const int64_t K = ctl->k0;
  ctl->c = -1;
  int c = 0;
  int64_t kb = K;
  if (ctl->phase == 1) {
    if (!ini_finish_loop(q, w, locG, locA, tail, ctl, K, 0, &c)) return;
    kb = K + 1;
  } else if (ctl->phase == 2) {
    if (!ini_finish_theta(q, w, locA, tail, ctl, K, 0, &c)) return;
    kb = K + 1;
  }
  if (kb == q.ktot) {   // the call's last construction ended here
    ctl->done = 1;
    ctl->consumed = (uint32_t)c;
    return;
  }
  ctl->c = c;
  ctl->kb = kb;
}

__global__ __launch_bounds__(256) void ini_f_kernel(const int* __restrict__ locG, const int* __restrict__ locA,
                                                    const int* __restrict__ tail, IniParams q, int* __restrict__ J0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= q.W) return;
  int f = INI_INF;
  const int s = i + q.sigma;
  if (s < q.W) {
    const int j = ini_next(locG, tail, s, 0);
    if (j != INI_INF) {
      const int e = j + 2;
      if (!q.theta) {
        f = e;
      } else if (e < q.W) {
        const int a = ini_next(locA, tail, e, 1);
        if (a != INI_INF) f = a + 2;
      }
    }
  }
  J0[i] = f;
}
__global__ __launch_bounds__(256) void ini_lift_kernel(const int* __restrict__ Jp, int W, int* __restrict__ Jn) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W) return;
  const int a = Jp[i];
  Jn[i] = a < W ? Jp[a] : INI_INF;
}

__global__ __launch_bounds__(256) void ini_chain_kernel(const uint32_t* __restrict__ raw, const uint32_t* __restrict__ state,
                                                        const int* __restrict__ locG, const int* __restrict__ locA,
                                                        const int* __restrict__ tail, const int* __restrict__ J, IniParams q,
                                                        int64_t kmax, IniCtl* ctl) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int c0 = ctl->c;
  if (c0 < 0 || k >= kmax) return;
  const int64_t K = ctl->kb + k;
  if (K > q.ktot) return;
  int c = c0;
  for (int m = q.L - 1; m >= 0; m--) {
    if (!((k >> m) & 1)) continue;
    if (c >= q.W) return;
    c = J[(int64_t)m * q.W + c];
    if (c == INI_INF) return;
  }
  if (K == q.ktot) {   // the call's end
    ctl->done = 1;
    ctl->consumed = (uint32_t)c;
    return;
  }
  const uint32_t* __restrict__ w = raw + state[INI_MT_N];
  int end;
  (void)ini_finish_loop(q, w, locG, locA, tail, ctl, K, c + q.sigma, &end);   // (the chain's last element carries)
}

__global__ __launch_bounds__(256) void ini_any_road_kernel(IniParams q, IniCtl* ctl) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)q.rows * q.cols) return;
  const int64_t r = i / q.cols, c = i % q.cols;
  if (q.rec[((r + 1) * (q.cols + 2) + (c + 1)) * q.rf + 1] < 1.f) ctl->road = 1;
}

// ---- host side -----------------------------------------------------------------------------------------------------
struct IniWs {
  int64_t W, nblocks, ntiles, kmax;
  int L;
  size_t off_locG, off_locA, off_min, off_tail, off_J, off_ctl, total;
};
static IniWs ini_ws(int64_t W) {
  IniWs s;
  s.W = W;
  s.nblocks = (INI_MT_N + W + 2) / INI_MT_N + 2;   // from anywhere inside block 0: words up to P + W + 1
  s.ntiles = W / INI_TILE;
  s.kmax = W / 2 + 2;                              // chain elements that fit: c_k >= 2 k, c_k <= W + 1
  s.L = 0;
  while (((int64_t)1 << s.L) < s.kmax) s.L++;
  size_t o = (size_t)s.nblocks * INI_MT_N * 4;
  auto take = [&](size_t bytes) { o = (o + 255) / 256 * 256; const size_t at = o; o += bytes; return at; };
  s.off_locG = take((size_t)W * 4);
  s.off_locA = take((size_t)W * 4);
  s.off_min = take((size_t)s.ntiles * 16);
  s.off_tail = take((size_t)(s.ntiles + 1) * 16);
  s.off_J = take((size_t)s.L * W * 4);
  s.off_ctl = take(sizeof(IniCtl));
  s.total = (o + 255) / 256 * 256;
  return s;
}
extern "C" size_t tdr_init_workspace_bytes(void) { return ini_ws(tdr_cfg().init_window).total; }

// particles the reference's loop keeps: max_num, or (max_num / 10) groups of the scale loop's length
static int ini_scales(float* sv) {
  int ns = 0;
  for (float scale = 0; scale < 1; scale += 1. / 10) {   // particle_filter.cpp:59
    if (ns < INI_MAX_NS) sv[ns] = (float)std::pow(10., (double)scale);   // :63
    ns++;
  }
  return ns;
}
extern "C" int64_t tdr_init_particles_count(const tdr_filter_params* fp, int max_num) {
  if (!fp || max_num < 0) return -1;
  if (fp->fixed_scale >= 0) return max_num;
  float sv[INI_MAX_NS];
  return (int64_t)(max_num / 10) * ini_scales(sv);
}

extern "C" int tdr_k_init_particles(uint32_t* state, const tdr_map_desc* map, const tdr_filter_params* fp, int max_num,
                                    int64_t lo, int64_t hi, float* st, int64_t cap, int64_t* n_out, void* workspace,
                                    void* stream) {
  if (!state || !map || !map->rec || !fp || !n_out || !workspace) return fail(TDR_ERR_ARG, "init_particles: null pointer");
  if (max_num < 0) return fail(TDR_ERR_ARG, "init_particles: bad arguments");
  if (map->ncls < 2) return fail(TDR_ERR_ARG, "init_particles: class 1 (road) is required for the on-road test");
  const int64_t n = tdr_init_particles_count(fp, max_num);
  if (lo < 0 || hi > n || lo > hi || (hi > lo && (!st || cap < hi - lo)))
    return fail(TDR_ERR_ARG, "init_particles: bad range [%lld, %lld) of %lld particles", (long long)lo, (long long)hi, (long long)n);
  hipStream_t s = (hipStream_t)stream;
  const IniWs S = ini_ws(tdr_cfg().init_window);
  char* base = reinterpret_cast<char*>(workspace);
  uint32_t* raw = reinterpret_cast<uint32_t*>(base);
  int* locG = reinterpret_cast<int*>(base + S.off_locG);
  int* locA = reinterpret_cast<int*>(base + S.off_locA);
  int* tmin = reinterpret_cast<int*>(base + S.off_min);
  int* tail = reinterpret_cast<int*>(base + S.off_tail);
  int* J = reinterpret_cast<int*>(base + S.off_J);
  IniCtl* ctl = reinterpret_cast<IniCtl*>(base + S.off_ctl);

  IniParams q{};
  q.rec = map->rec;
  q.rf = map->rec_floats;
  q.rows = map->rows;
  q.cols = map->cols;
  q.res = map->resolution;
  q.map_w = (float)map->cols * map->resolution;
  q.map_h = (float)map->rows * map->resolution;
  q.normal = fp->init_pos_px_x > 0;
  q.px = fp->init_pos_px_x;
  q.py = fp->init_pos_px_y;
  q.pcov = fp->init_pos_px_cov;
  q.theta = fp->init_pos_deg_theta != std::numeric_limits<float>::infinity();
  q.deg = fp->init_pos_deg_theta;
  q.dcov = fp->init_pos_deg_cov;
  q.sigma = fp->fixed_scale < 0;
  q.fixed_scale = fp->fixed_scale;
  q.ns = q.sigma ? ini_scales(q.sv) : 1;
  if (q.ns > INI_MAX_NS) return fail(TDR_ERR_ARG, "init_particles: %d scales per group", q.ns);
  q.per = q.sigma ? 1 + 2 * q.ns : 3;
  q.ktot = q.sigma ? (int64_t)(max_num / 10) * q.per : (int64_t)max_num * 3;
  q.lo = lo;
  q.hi = hi;
  q.cap = cap;
  q.st = st;
  q.W = (int)S.W;
  q.L = S.L;

  // the host loop's pre-check: rejection sampling cannot end on a map without road
  IniCtl c0{};
  c0.c = -1;
  HIP_TRY(hipMemcpyAsync(ctl, &c0, sizeof(c0), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(ini_any_road_kernel, dim3((unsigned)cdiv((int64_t)q.rows * q.cols, 256)), dim3(256), 0, s, q, ctl);
  LAUNCH_CHECK("ini_any_road");
  IniCtl h{};
  HIP_TRY(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (!h.road) return fail(TDR_ERR_ARG, "init_particles: the map has no road cell, rejection sampling cannot end");
  *n_out = n;
  if (q.ktot == 0) return TDR_OK;   // no construction: no word is drawn

  // a construction that has not ended after 2^36 words would not end on the host either (the reference loops forever)
  const int64_t stall_windows = std::max<int64_t>(1, ((int64_t)1 << 36) / S.W);
  int64_t last_k = -1, stalled = 0;
  for (;;) {
    if (int rc = tdr_mt_raw_stream(state, S.nblocks, raw, s)) return rc;
    hipLaunchKernelGGL(ini_flags_kernel, dim3((unsigned)S.ntiles), dim3(1024), 0, s, (const uint32_t*)raw,
                       (const uint32_t*)state, q, locG, locA, tmin);
    LAUNCH_CHECK("ini_flags");
    hipLaunchKernelGGL(ini_tail_kernel, dim3(1), dim3(1024), 0, s, (const int*)tmin, (int)S.ntiles, tail);
    LAUNCH_CHECK("ini_tail");
    hipLaunchKernelGGL(ini_head_kernel, dim3(1), dim3(64), 0, s, (const uint32_t*)raw, (const uint32_t*)state,
                       (const int*)locG, (const int*)locA, (const int*)tail, q, ctl);
    LAUNCH_CHECK("ini_head");
    const unsigned wblocks = (unsigned)cdiv(S.W, 256);
    hipLaunchKernelGGL(ini_f_kernel, dim3(wblocks), dim3(256), 0, s, (const int*)locG, (const int*)locA, (const int*)tail,
                       q, J);
    LAUNCH_CHECK("ini_f");
    for (int m = 1; m < S.L; m++) {
      hipLaunchKernelGGL(ini_lift_kernel, dim3(wblocks), dim3(256), 0, s, (const int*)(J + (size_t)(m - 1) * S.W),
                         (int)S.W, J + (size_t)m * S.W);
      LAUNCH_CHECK("ini_lift");
    }
    hipLaunchKernelGGL(ini_chain_kernel, dim3((unsigned)cdiv(S.kmax, 256)), dim3(256), 0, s, (const uint32_t*)raw,
                       (const uint32_t*)state, (const int*)locG, (const int*)locA, (const int*)tail, (const int*)J, q,
                       S.kmax, ctl);
    LAUNCH_CHECK("ini_chain");
    if (int rc = tdr_mt_advance(raw, S.nblocks, &ctl->consumed, state, s)) return rc;
    HIP_TRY(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h.done) break;
    if (h.consumed == 0) return fail(TDR_ERR_HIP, "init_particles: a window consumed no word");
    if (h.k0 == last_k) {
      if (++stalled > stall_windows)
        return fail(TDR_ERR_ARG, "init_particles: construction %lld found no road cell in 2^36 words", (long long)h.k0);
    } else {
      last_k = h.k0;
      stalled = 0;
    }
  }
  return TDR_OK;
}
