// tdr_score_cart_init.hip — the heading search of the Cartesian filter (include/tdr.h: tdr_k_score_cart_init).
//
// A particle without a heading takes, like StateParticle::computeWeight does for the polar filter
// (src/state_particle.cpp:195-206), the first of the candidates `for (float t = 0; t < 2*M_PI; t += 2*M_PI/40)` whose
// Cartesian cost is strictly smaller than every earlier one; NaN (a window less than half known) is never chosen.
//
// The candidates of one particle share a centre and a scale but no map cells — at radius r they sample a circle — so a
// fused per-particle kernel would share nothing but the scan descriptors, which sit in L2 anyway.  The
// search is therefore COMPOSED from the scoring launch the filter runs anyway:
//   cart_init_list_kernel     lists the particles without a heading (one workgroup: no counter to zero, the same list
//                             every run).  A list longer than one chunk is made again in the order of
//                             tdr_k_locality_order_pose over the filter's particles, so that a chunk of it is a
//                             NEIGHBOURHOOD of the map — as dense as the whole cloud, where a chunk in index order is a
//                             thin sample of it (measured);
//   cart_init_expand_kernel   writes, for a chunk of c listed particles, nrot * c candidate states (theta = t_j,
//                             have_init = 1), candidate-major: neighbours in the list stay neighbours at every heading;
//   tdr_k_locality_order_pose orders the candidates by (x, y, heading) like the filter orders its particles: the scoring
//                             launch takes its dense share from that order (a launch without one counts every particle
//                             as scattered: one wave each, measured 3.7 x the regular launch per candidate);
//   tdr_k_score_cart          scores them — whatever form tdr_config_shift_uniform / tdr_config_cart_skip select today;
//   cart_init_select_kernel   first maximum of the weight per particle (weight = 1 / (cost + regularization) falls as
//                             the cost rises), NaN skipped; writes theta and have_init back.
// The candidate launches split a window into the partial sums the filter's regular launch uses (n_total), so a candidate's
// weight is the bits that launch gives the particle at that heading, and the choice does not depend on the chunk size.
// The host reads the list's length back once (the launcher's only wait): it decides how many chunks are launched, and a
// call that finds no such particle ends after the list kernel.
#include "tdr_common.h"

#define CART_INIT_MAXROT 48

namespace {

struct CartInitRot {
  int nrot;
  float theta[CART_INIT_MAXROT];
};

// the reference's loop as written: float t, double increment (state_particle.cpp:197); init_rot_body's table
const CartInitRot& cart_init_rot() {
  static const CartInitRot r = [] {
    CartInitRot x{};
    for (float t = 0; t < 2 * M_PI && x.nrot < CART_INIT_MAXROT; t += 2 * M_PI / 40) x.theta[x.nrot++] = t;
    return x;
  }();
  return r;
}

inline int64_t pad64(int64_t x) { return cdiv(x, 64) * 64; }

struct CartInitWs {   // offsets in floats, every part 256-byte aligned
  int64_t chunk, ccap;   // listed particles per launch; plane stride of the candidate states (= candidates per launch)
  int64_t list, order, cst, craw, perm, keys, score, total;
};
CartInitWs cart_init_ws(int ncls, int rows, int cols, int64_t n, int64_t n_total) {
  CartInitWs w;
  n = std::max<int64_t>(n, 1);
  w.chunk = std::min<int64_t>(tdr_cfg().cart_init_chunk, n);
  w.ccap = pad64(w.chunk * cart_init_rot().nrot);
  w.list = 0;                                  // int32 [64 + n]: [0] = count, the list from [64]
  w.order = w.list + pad64(64 + n);            // int32 [n]: the particles by pose; its scratch lies in the chunk's part
  w.cst = w.order + pad64(n);
  w.craw = w.cst + TDR_ST_FIELDS * w.ccap;
  w.perm = w.craw + w.ccap;                    // int32 [ccap]: the candidates' locality order
  w.keys = w.perm + w.ccap;                    // ... and its scratch
  w.score = w.keys + pad64((int64_t)tdr_locality_pose_tmp_ints(w.ccap) + 2);
  w.total = w.score + (int64_t)tdr_score_cart_workspace_floats(ncls, rows, cols, w.ccap, n_total > 0 ? n_total : n);
  // (the order's scratch is used before the first chunk, from cst on)
  w.total = std::max(w.total, w.cst + pad64((int64_t)tdr_locality_pose_tmp_ints(n) + 2));
  return w;
}

__global__ __launch_bounds__(1024) void cart_init_list_kernel(const float* __restrict__ have_init, const int32_t* __restrict__ order,
                                                              int64_t n, int32_t* __restrict__ list, int32_t* __restrict__ count) {
  __shared__ int wave_cnt[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  for (int64_t i0 = 0; i0 < n; i0 += 1024) {
    const int64_t i = i0 + threadIdx.x;
    const int32_t p = i < n && order ? order[i] : (int32_t)i;      // order: a permutation of [0, n), or NULL
    const bool un = i < n && have_init[p] == 0.f;
    const uint64_t b = __ballot(un);
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < 16; w++) {
      const int c = wave_cnt[w];
      off += w < wave ? c : 0;
      tot += c;
    }
    if (un) list[base + off + __popcll(b & ((1ull << lane) - 1))] = p;   // base + off + rank <= i < n
    base += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = base;
}

__global__ __launch_bounds__(256) void cart_init_expand_kernel(const float* __restrict__ st, int64_t cap,
                                                               const int32_t* __restrict__ list, int c, CartInitRot rot,
                                                               float* __restrict__ cst, int64_t ccap) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)rot.nrot * c) return;
  const int j = (int)(t / c);
  const int64_t p = list[t - (int64_t)j * c];
  cst[TDR_ST_INIT_X * ccap + t] = st[TDR_ST_INIT_X * cap + p];
  cst[TDR_ST_INIT_Y * ccap + t] = st[TDR_ST_INIT_Y * cap + p];
  cst[TDR_ST_DX * ccap + t] = st[TDR_ST_DX * cap + p];
  cst[TDR_ST_DY * ccap + t] = st[TDR_ST_DY * cap + p];
  cst[TDR_ST_THETA * ccap + t] = rot.theta[j];
  cst[TDR_ST_SCALE * ccap + t] = st[TDR_ST_SCALE * cap + p];
  cst[TDR_ST_HAVE_INIT * ccap + t] = 1.f;
}

// `if (cost < best_cost)` over the candidates in order (state_particle.cpp:200-203) on the weights: the first weight
// larger than every earlier one; a NaN compares false.  No finite candidate: theta = best_theta's initial 0.
__global__ __launch_bounds__(256) void cart_init_select_kernel(const float* __restrict__ craw, const int32_t* __restrict__ list,
                                                               int c, CartInitRot rot, float* __restrict__ st, int64_t cap) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= c) return;
  float best_w = 0.f, best_theta = 0.f;
  for (int j = 0; j < rot.nrot; j++) {
    const float w = craw[(int64_t)j * c + i];
    if (w > best_w) {
      best_w = w;
      best_theta = rot.theta[j];
    }
  }
  const int64_t p = list[i];
  st[TDR_ST_THETA * cap + p] = best_theta;
  st[TDR_ST_HAVE_INIT * cap + p] = 1.f;
}

}  // namespace

extern "C" size_t tdr_score_cart_init_workspace_floats(int ncls, int rows, int cols, int64_t n, int64_t n_total) {
  return (size_t)cart_init_ws(ncls, rows, cols, n, n_total).total;
}

extern "C" int tdr_k_score_cart_init(const tdr_map_desc* map, const float* scan_pk, int rows, int cols, float res,
                                     const tdr_filter_params* fp, float* st, int64_t cap, int64_t n, int64_t n_total,
                                     float* workspace, void* stream) {
  if (!map || !map->rec || !scan_pk || !fp || !st || !workspace) return fail(TDR_ERR_ARG, "score_cart_init: null pointer");
  if (n < 0 || cap < n) return fail(TDR_ERR_ARG, "score_cart_init: n exceeds capacity");
  if (rows < 1 || cols < 1) return fail(TDR_ERR_ARG, "score_cart_init: bad window shape");
  if (n > std::numeric_limits<int32_t>::max()) return fail(TDR_ERR_ARG, "score_cart_init: more than 2^31 particles");
  if (n == 0) return TDR_OK;
  if (n_total <= 0) n_total = n;
  hipStream_t s = (hipStream_t)stream;
  const CartInitRot& rot = cart_init_rot();
  const CartInitWs w = cart_init_ws(map->ncls, rows, cols, n, n_total);
  int32_t* count = reinterpret_cast<int32_t*>(workspace + w.list);
  int32_t* list = count + 64;
  const float theta_radius = (float)(rows + cols) / 16.f;   // the filters' (csrc/tdr_host_filter.cpp, particle_filter.py)
  hipLaunchKernelGGL(cart_init_list_kernel, dim3(1), dim3(1024), 0, s, (const float*)(st + TDR_ST_HAVE_INIT * cap),
                     (const int32_t*)nullptr, n, list, count);
  LAUNCH_CHECK("cart_init_list");
  int32_t listed = 0;
  HIP_TRY(hipMemcpyAsync(&listed, count, sizeof(listed), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (listed < 0 || listed > n) return fail(TDR_ERR_HIP, "score_cart_init: list length %d out of range", listed);
  if (listed > w.chunk) {   // several chunks: each a neighbourhood of the map
    int32_t* order = reinterpret_cast<int32_t*>(workspace + w.order);
    if (int rc = tdr_k_locality_order_pose(st, cap, n, map->rows, map->cols, theta_radius, order,
                                           reinterpret_cast<int32_t*>(workspace + w.cst), stream))
      return rc;
    hipLaunchKernelGGL(cart_init_list_kernel, dim3(1), dim3(1024), 0, s, (const float*)(st + TDR_ST_HAVE_INIT * cap),
                       (const int32_t*)order, n, list, count);
    LAUNCH_CHECK("cart_init_list(ordered)");
  }
  float* cst = workspace + w.cst;
  float* craw = workspace + w.craw;
  int32_t* cperm = reinterpret_cast<int32_t*>(workspace + w.perm);
  int32_t* ckeys = reinterpret_cast<int32_t*>(workspace + w.keys);
  for (int64_t lo = 0; lo < listed; lo += w.chunk) {
    const int c = (int)std::min<int64_t>(w.chunk, listed - lo);
    const int64_t nc = (int64_t)rot.nrot * c;   // <= w.ccap
    hipLaunchKernelGGL(cart_init_expand_kernel, dim3((unsigned)cdiv(nc, 256)), dim3(256), 0, s, (const float*)st, cap,
                       (const int32_t*)(list + lo), c, rot, cst, w.ccap);
    LAUNCH_CHECK("cart_init_expand");
    if (int rc = tdr_k_locality_order_pose(cst, w.ccap, nc, map->rows, map->cols, theta_radius, cperm, ckeys, stream)) return rc;
    if (int rc = tdr_k_score_cart(map, scan_pk, rows, cols, res, fp, cst, w.ccap, nc, n_total, cperm, craw,
                                  workspace + w.score, stream))
      return rc;
    hipLaunchKernelGGL(cart_init_select_kernel, dim3((unsigned)cdiv(c, 256)), dim3(256), 0, s, (const float*)craw,
                       (const int32_t*)(list + lo), c, rot, st, cap);
    LAUNCH_CHECK("cart_init_select");
  }
  return TDR_OK;
}
