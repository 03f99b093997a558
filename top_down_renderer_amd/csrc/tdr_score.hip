// tdr_score.hip — per-particle window gather + class-wise score: polar, Cartesian, finalize; the host side of the scoring
// launches and their process-wide switches.  (The 40-rotation init search: tdr_score_init.hip.)

#include "tdr_common.h"
#include "tdr_batch.h"
#include "tdr_sincosf.h"

// ------------------------------------------------------------------------------------------------------------------
// K2: scoring.  lane = particle, 64 particles per wave, 4 waves per workgroup; grid.y = chunk of range rings.
// All lanes of a wave visit the same window sample (i,j) at the same time, so their map reads fall on neighbouring
// cells when the particles are neighbours (tdr_k_locality_order) and coalesce in L1/L2 instead of being 64
// unrelated gathers; the rotation enters only as a per-lane row offset into the ring of scan records held in LDS.
struct ScoreArgs {
  const float* rec;     // map cell records
  int rows, cols;       // map
  float resolution;
  const float* tab;     // [P][2]
  const float* utab = nullptr;   // [P][2] (tab*scale)*res when all particles share one scale, else NULL
  const float* scan_pk; // [nr][nb][rf]
  int nb, nr;
  float res;
  const float* st;      // [7][cap]
  int64_t cap, n;
  const int32_t* order; // slot -> particle (NULL = identity)
  // UNUSED: no launch sets count, slot_base, kmask_off or kmask_row (the mixed launch that did is tdr_score_ray.hip's now).
  // They stay, with the two loads that read them, because the smaller block gives score_polar_batch_kernel another register
  // assignment — more VGPRs or scratch in three instantiations (profiles/score_split_resources_v1.txt).
  const int32_t* count = nullptr;      // optional device count limiting the active slots
  const int32_t* slot_base = nullptr;  // optional device word: this launch's slot 0 is slot *slot_base of `order` and of `part`
  int use_theta_override = 0;
  float theta_override = 0.f;
  int only_uninit = 0;  // score only workgroups that hold a particle without a heading (the geometric init search)
  int group, nchunks;   // rings per workgroup (score_group_rings), number of groups
  int64_t npad;         // slots padded to a multiple of 64
  float* part;          // [nchunks][rf+1][npad]
  // compact form of the records (tdr_cmap.hip), read by the COMPACT instantiations
  const uint32_t* crec = nullptr;
  const float* dict = nullptr;
  int dict_n = 0;       // dictionary entries in use
  int ctiles_r = 0;     // tiles per tile column
  unsigned kmask_off = 0;   // (unused, see `count`)
  int kmask_row = 0;
  const int32_t* run_if = nullptr; // optional device words (int_form_off): the launch runs only then (the float form of a launch whose
                         // integer form — tdr_score_su.hip, tdr_score_ray.hip — applies)
};

#include "tdr_score_dev.h"   // rot_shift_dev, the coordinate rounding, compact-record geometry / load / decode, the gates
#include "tdr_local_cell.h"  // linspaced_dev, the cell of one window sample (shared with tdr_fuse.hip)
#include "tdr_score_init.h"  // the 40-rotation init search (tdr_score_init.hip)
#include "tdr_score_su.h"    // the shift-uniform kernel's host interface (tdr_score_su.hip)
#include "tdr_score_cart.h"  // CartArgs, the Cartesian kernel that skips empty scan bins (tdr_score_cart.hip)


TDR_TL_BUFFER(g_timeline, tdr_debug_read_timeline)   // (diagnostic build only: tdr_score_dev.h)
// COMPACT: this instantiation reads the compact records (10-bit dictionary indices, decoded through LDS; bit-identical
// operands) instead of the dense ones — a quarter of the bytes through L1 / L2 / HBM for six classes.  It is the one
// that runs whenever the map has a compact form (A/B on MI355X, config 2, 100 k particles, ms per launch dense ->
// compact: bench mix 15.5 -> 9.6, 100 % Gaussian 30 px 7.3 -> 5.9, Gaussian 5 px 6.2 -> 5.8, 100 % uniform 97 -> 67,
// 8 clusters 20.3 -> 6.6); the dense instantiation remains for maps without one (> 1024 distinct values, > 11 classes).
//
// Work decomposition: grid.y = GROUP of a.group consecutive range rings (a constant of the image shape, see
// score_group_rings), so the summation tree of a particle's score is a pure function of the configuration — never of the
// number of particles in the launch or of the rank count.  Inside a group the samples are visited RAY-major: for each
// window row i (a direction) the group's rings in turn, i.e. up to a.group consecutive cells along one ray.  Compact
// records are tiled 4 x 4 cells per 128-byte line, so a ray stays in a tile for ~3 steps: a lane whose neighbours are far
// away (scattered particles) fetches ~0.5 lines per sample instead of one.  The scan rows of the whole group sit in LDS
// ([ring][plane][row], not doubled: the row (i + shift) mod nb is computed once per direction).
// WIDE: the compact records are the wide form (maps of more than 1024 distinct values, tdr_cmap.hip)
// The body for workgroup (bx, by) of the launch: score_polar_kernel and score_polar_batch_kernel (one grid over many
// filters) both call it.
template <int NV4, int U, bool KSLOT, bool USCALE, bool COMPACT, bool WIDE = false>
__device__ __forceinline__ void score_polar_body(const ScoreArgs& a, const unsigned bx, const unsigned by) {
  constexpr int RF = 4 * NV4;
  static_assert(!WIDE || (COMPACT && NV4 == 2), "wide compact records: 8-float dense records only");
  constexpr int CW = WIDE ? 4 : CmapShape<RF, KSLOT>::CW, LC = WIDE ? 1 : CmapShape<RF, KSLOT>::LC;
  constexpr int NDICT = WIDE ? TDR_CMAP_WIDE_MAX_DICT : TDR_CMAP_MAX_DICT;
  TDR_TL_BEGIN(g_timeline)
  extern __shared__ float4 ring[];  // [nb rows][rs]: a row's (ring, plane) records side by side, rs = group * NV4 | 1
  __shared__ float ldict[COMPACT ? NDICT : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t slot = ((int64_t)bx * 4 + wave) * 64 + lane;
  if (a.run_if && !int_form_off(a.run_if)) return;  // (uniform)
  const int64_t nact = a.count ? (int64_t)*a.count : a.n;
  if ((int64_t)bx * 256 >= nact) return;  // whole workgroup idle (uniform)
  const bool valid = slot < nact;
  const int64_t sbase = a.slot_base ? (int64_t)*a.slot_base : 0;
  const int64_t p = a.order ? (int64_t)a.order[sbase + (valid ? slot : 0)] : (valid ? slot : 0);
  if (a.only_uninit && !__syncthreads_or(valid && a.st[TDR_ST_HAVE_INIT * a.cap + p] == 0.f)) return;
  const float scale = a.st[TDR_ST_SCALE * a.cap + p];
  const float cx = a.st[TDR_ST_DX * a.cap + p] * scale + a.st[TDR_ST_INIT_X * a.cap + p];  // state_particle.cpp:161
  const float cy = a.st[TDR_ST_DY * a.cap + p] * scale + a.st[TDR_ST_INIT_Y * a.cap + p];  // :162
  const float off0 = cy / a.resolution;  // top_down_map_polar.cpp:29
  const float off1 = cx / a.resolution;  // :30
  const float theta = a.use_theta_override ? a.theta_override : a.st[TDR_ST_THETA * a.cap + p];
  const int shift = rot_shift_dev(theta, a.nb);  // scan row paired with window row i is (i + shift) mod nb

  const int j0 = by * a.group, gn = min(a.nr - j0, a.group);   // this workgroup's rings: [j0, j0 + gn)
  const int rowstride = (a.cols + 2) * (RF * 4);            // bytes per guarded map row
  const int kbase = (a.cols + 3) * (RF * 4);                // byte offset of cell (0,0)
  const float rmaxf = (float)a.rows, cmaxf = (float)a.cols;
  const char* __restrict__ recb = reinterpret_cast<const char*>(a.rec);
  const char* __restrict__ crecb = reinterpret_cast<const char*>(a.crec);
  const int ckcol = a.ctiles_r * 128 - 16 * CW, ckconst = a.ctiles_r * 128 + 128;   // cmap_offset
  // The sample table is read-only for the whole launch and every lane of a wave reads the same entry: it is addressed
  // through the CONSTANT address space so that these are scalar loads whatever else the kernel contains.  (Left to its
  // own no-clobber analysis the compiler gives up in the compact kernel — the dictionary staging is one store too many —
  // and emits vector loads with a full wait in front of every address computation.)
  typedef const float __attribute__((address_space(4))) * tdr_const_f;
  const tdr_const_f tabc = (tdr_const_f)(USCALE ? a.utab : a.tab);
  auto tab_at = [&](int64_t k) { return make_float2(tabc[2 * k], tabc[2 * k + 1]); };
  const float4* __restrict__ scan4 = reinterpret_cast<const float4*>(a.scan_pk);
  const int nb = a.nb;

  // stage the group's scan rows and (compact) the dictionary
  if constexpr (COMPACT)
    for (int t = threadIdx.x; t < a.dict_n; t += 256) ldict[t] = a.dict[t];
  // One row of the LDS image = the scan records (ring, plane) of one direction, 16 bytes each, side by side: a step
  // reads them with ONE address per lane and immediate offsets.  The row stride is an ODD number of 16-byte slots, so
  // lanes on different rows (different headings) fall on different banks.
  const int rs = (a.group * NV4) | 1;
  for (int jj = 0; jj < gn; jj++)
    for (int t = threadIdx.x; t < nb * NV4; t += 256) {
      const float4 v = scan4[(int64_t)(j0 + jj) * nb * NV4 + t];
      const int row = t / NV4, pl = t - row * NV4;
      ring[row * rs + jj * NV4 + pl] = v;
    }
  __syncthreads();

  // USCALE: every particle has the same scale, so (tab*scale)*res was evaluated once per step into a.utab and is
  // wave-uniform here; otherwise it is evaluated per lane.  Identical float operations either way.
  // Returns the byte offset of the sample's record (dense: guarded row-major grid; compact: tiled).
  typedef float tdr_v2f __attribute__((ext_vector_type(2)));   // both coordinates in one v_pk_add_f32 / v_pk_mul_f32
  const tdr_v2f offv = {off0, off1};
  auto cell_offset = [&](float2 t) -> unsigned {
    tdr_v2f pv = {t.x, t.y};
    if constexpr (!USCALE) pv = (pv * scale) * a.res;  // top_down_map_polar.cpp:28
    pv = pv + offv;                                     // :29-30
    // clamp into the guard ring, then round like `pts.round().cast<int>()` (:31): roundf(x) == floor(fl(x + (0.5 - 2^-25)))
    // on [-1, 2^23] (round_half_away_clamped), the addition done for both coordinates at once
    tdr_v2f qv = {__builtin_amdgcn_fmed3f(pv.x, -1.f, rmaxf), __builtin_amdgcn_fmed3f(pv.y, -1.f, cmaxf)};
    qv = qv + 0.49999997f;
    int ri, ci;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ri) : "v"(qv.x));
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ci) : "v"(qv.y));
    if constexpr (COMPACT) {
      // cells of the guard ring are zero records in their own right (distance 0, unknown): no select needed
      return cmap_offset<CW, LC>(ri, ci, ckcol, ckconst);
    } else {
#if TDR_OOB_ALIAS
      // every out-of-bounds sample reads the SAME guard record (always cache-resident) instead of a distinct one
      const bool inb = (unsigned)ri < (unsigned)a.rows && (unsigned)ci < (unsigned)a.cols;
      return inb ? (unsigned)(__mul24(ri, rowstride) + (ci * (RF * 4) + kbase)) : 0u;
#else
      return (unsigned)(__mul24(ri, rowstride) + (ci * (RF * 4) + kbase));  // v_mad_i32_i24 + v_lshl_add
#endif
    }
  };
  // the record at `off` as the RF operands of the product sums (compact: decoded, bit-identical to the dense record)
  struct Raw { uint32_t w[COMPACT ? CW : 1]; float4 q[COMPACT ? 1 : NV4]; };
  auto load_raw = [&](unsigned off, Raw& r) {
    if constexpr (COMPACT) cmap_load<CW>(crecb, off, r.w);
    else {
#pragma unroll
      for (int v = 0; v < NV4; v++) r.q[v] = *reinterpret_cast<const float4*>(recb + off + 16 * v);
    }
  };
  auto operands = [&](const Raw& r, float (&m)[RF]) {
    if constexpr (WIDE) cmap_decode_wide<RF, KSLOT>(r.w, ldict, m);
    else if constexpr (COMPACT) cmap_decode<RF, KSLOT>(r.w, ldict, m);
    else {
#pragma unroll
      for (int v = 0; v < NV4; v++) { m[4 * v] = r.q[v].x; m[4 * v + 1] = r.q[v].y; m[4 * v + 2] = r.q[v].z; m[4 * v + 3] = r.q[v].w; }
    }
  };

  float acc[RF];
#pragma unroll
  for (int k = 0; k < RF; k++) acc[k] = 0.f;
  float known = 0.f;
  // U samples per step: all addresses first, then all loads (map records + LDS scan records) in flight together, then
  // the FMAs.  The order of the FMAs — direction i ascending, ring ascending within it — is the same in every
  // instantiation and independent of U and of the launch: results are a pure function of the inputs.
  auto step = [&](auto full_step, const unsigned (&boff)[U], const float4* const (&sp)[U], int cnt) {
    constexpr bool FULL = decltype(full_step)::value;   // all U samples are real: no per-sample predicate
    Raw raw[U];
    float4 s[U][NV4];
#pragma unroll
    for (int u = 0; u < U; u++)
      if (FULL || u < cnt) load_raw(boff[u], raw[u]);
#pragma unroll
    for (int u = 0; u < U; u++)
      if (FULL || u < cnt) {
#pragma unroll
        for (int v = 0; v < NV4; v++) s[u][v] = sp[u][v];
      }
#pragma unroll
    for (int u = 0; u < U; u++)
      if (FULL || u < cnt) {
        float m[RF];
        operands(raw[u], m);
#pragma unroll
        for (int v = 0; v < NV4; v++) {
          acc[4 * v + 0] = __builtin_fmaf(s[u][v].x, m[4 * v + 0], acc[4 * v + 0]);
          acc[4 * v + 1] = __builtin_fmaf(s[u][v].y, m[4 * v + 1], acc[4 * v + 1]);
          acc[4 * v + 2] = __builtin_fmaf(s[u][v].z, m[4 * v + 2], acc[4 * v + 2]);
          acc[4 * v + 3] = __builtin_fmaf(s[u][v].w, m[4 * v + 3], acc[4 * v + 3]);
        }
        if (!KSLOT) known += m[RF - 1];
      }
  };
  if (gn >= U) {
    // ray-major: consecutive samples of a lane are consecutive cells along one ray
    const int gfull = gn - gn % U;
    for (int i = 0; i < nb; i++) {
      int row = i + shift;
      row -= row >= nb ? nb : 0;
      const float4* const rl = ring + __mul24(row, rs);
      for (int jj = 0; jj < gfull; jj += U) {
        unsigned boff[U];
        const float4* sp[U];
        const float4* const rj = rl + jj * NV4;
#pragma unroll
        for (int u = 0; u < U; u++) {
          boff[u] = cell_offset(tab_at((int64_t)(j0 + jj + u) * nb + i));
          sp[u] = rj + u * NV4;
        }
        step(std::true_type{}, boff, sp, U);
      }
    }
    if (gfull < gn) {   // the group's last rings when gn is not a multiple of U: a pass of their own over the directions
      for (int i = 0; i < nb; i++) {
        int row = i + shift;
        row -= row >= nb ? nb : 0;
        const float4* const rl = ring + __mul24(row, rs);
        unsigned boff[U];
        const float4* sp[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int jc = min(gfull + u, gn - 1);
          boff[u] = cell_offset(tab_at((int64_t)(j0 + jc) * nb + i));
          sp[u] = rl + jc * NV4;
        }
        step(std::false_type{}, boff, sp, gn - gfull);
      }
    }
  } else {
    // fewer rings than loads to keep in flight (very long rows): U consecutive directions of one ring at a time
    for (int jj = 0; jj < gn; jj++) {
      const float4* const rj = ring + jj * NV4;
      for (int i = 0; i < nb; i += U) {
        unsigned boff[U];
        const float4* sp[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int ic = min(i + u, nb - 1);
          int row = ic + shift;
          row -= row >= nb ? nb : 0;
          boff[u] = cell_offset(tab_at((int64_t)(j0 + jj) * nb + ic));
          sp[u] = rj + __mul24(row, rs);
        }
        step(std::false_type{}, boff, sp, min(U, nb - i));
      }
    }
  }
  if (sbase + slot < a.npad) {
    float* o = a.part + (int64_t)by * (RF + 1) * a.npad + sbase + slot;
#pragma unroll
    for (int k = 0; k < RF; k++) o[(int64_t)k * a.npad] = acc[k];
    o[(int64_t)RF * a.npad] = KSLOT ? acc[RF - 2] : known;
  }
  TDR_TL_END(g_timeline)
}
template <int NV4, int U, bool KSLOT, bool USCALE, bool COMPACT, bool WIDE = false>
__global__ __launch_bounds__(256, COMPACT ? (WIDE ? 3 : 5) : 1) void score_polar_kernel(ScoreArgs a) {
#if TDR_XCD_SWIZZLE
  // Workgroups are dealt round-robin over the 8 XCDs; remap so that each XCD (its own L2) gets a contiguous run of
  // particle batches (Morton neighbours) instead of every 8th one.  Speed only: any mapping gives the same results.
  const unsigned nbx = gridDim.x, per = (nbx + 7) / 8;
  unsigned bx = (blockIdx.x % 8) * per + blockIdx.x / 8;
  if (nbx % 8 != 0) bx = blockIdx.x;  // keep it a bijection
#else
  const unsigned bx = blockIdx.x;
#endif
  score_polar_body<NV4, U, KSLOT, USCALE, COMPACT, WIDE>(a, bx, blockIdx.y);
}
// The float form BEHIND the integer kernels of a launch (a.run_if set): a bounded grid — at most what the chip holds resident
// — whose workgroups walk the launch's workgroup ids (vx, vy), x fastest like the dispatcher.  The flag is read once: while the
// integer form is on, which is every call of a scan and a map that have one, the grid leaves at once instead of starting one
// workgroup per unit that reads the flag and returns.  Per id the body is score_polar_kernel's own (its LDS image staged anew,
// a barrier between two ids): a particle's partial sums are per (slot, ring group) and do not depend on which workgroup forms
// them — the bits of the plain launch.
template <int NV4, int U, bool KSLOT, bool USCALE, bool COMPACT, bool WIDE = false>
__global__ __launch_bounds__(256, COMPACT ? (WIDE ? 3 : 5) : 1) void score_polar_bounded_kernel(ScoreArgs a, unsigned nbx, unsigned nby) {
  if (!int_form_off(a.run_if)) return;   // (uniform)
  a.run_if = nullptr;
  const uint64_t total = (uint64_t)nbx * nby;
  for (uint64_t v = blockIdx.x; v < total; v += gridDim.x) {
    const unsigned vy = (unsigned)(v / nbx), vx = (unsigned)(v - (uint64_t)vy * nbx);
#if TDR_XCD_SWIZZLE
    const unsigned per = (nbx + 7) / 8;
    const unsigned bx = nbx % 8 != 0 ? vx : (vx % 8) * per + vx / 8;
#else
    const unsigned bx = vx;
#endif
    score_polar_body<NV4, U, KSLOT, USCALE, COMPACT, WIDE>(a, bx, vy);
    __syncthreads();   // every wave is through with the LDS image before the next id's is staged
  }
}
// batched filters (tdr_batch_step): filter e owns the blocks [blk[e], blk[e + 1]) of grid.x and grid.y rows
// [0, its nchunks); its ScoreArgs are args[e].  Filters whose USCALE differs from the instantiation's are another launch.
template <int NV4, int U, bool KSLOT, bool USCALE, bool COMPACT, bool WIDE = false>
__global__ __launch_bounds__(256, COMPACT ? (WIDE ? 3 : 5) : 1) void score_polar_batch_kernel(const ScoreArgs* __restrict__ args,
                                                                                              const int32_t* __restrict__ blk, int k) {
  const int e = batch_find(k, (int)blockIdx.x, [&](int i) { return blk[i]; });
  const ScoreArgs a = args[e];
  if ((int)blockIdx.y >= a.nchunks || (a.utab != nullptr) != USCALE) return;   // (uniform)
  score_polar_body<NV4, U, KSLOT, USCALE, COMPACT, WIDE>(a, blockIdx.x - (unsigned)blk[e], blockIdx.y);
}

// K2c: Cartesian scoring (BASELINE config 4).  The reference's StateParticle never reaches the Cartesian
// TopDownMap::getLocalMap, so the Cartesian score is DEFINED as: window sampled by getLocalMap
// (src/top_down_map.cpp:429-459 via samplePts :367-389) at rot = theta, res = res*scale, scored by getCostForRot
// with shift 0 (src/state_particle.cpp:132-143) (definition recorded in include/tdr.h:tdr_k_score_cart and DESIGN.md).
// Same mapping as the polar kernel (lane = particle); the rotation now lives in the sampling, so the scan record of
// sample (i,j) is the same for every lane and comes through the scalar cache instead of LDS.
// (linspaced_dev: tdr_local_cell.h)
template <int NV4, int U, bool KSLOT, bool COMPACT, bool WIDE = false>
__global__ __launch_bounds__(256) void score_cart_kernel(CartArgs a) {
  constexpr int RF = 4 * NV4;
  static_assert(!WIDE || (COMPACT && NV4 == 2), "wide compact records: 8-float dense records only");
  constexpr int CW = WIDE ? 4 : CmapShape<RF, KSLOT>::CW, LC = WIDE ? 1 : CmapShape<RF, KSLOT>::LC;
  __shared__ float ldict[COMPACT ? (WIDE ? TDR_CMAP_WIDE_MAX_DICT : TDR_CMAP_MAX_DICT) : 1];
  if constexpr (COMPACT) {
    for (int t = threadIdx.x; t < a.dict_n; t += 256) ldict[t] = a.dict[t];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t slot = ((int64_t)blockIdx.x * 4 + wave) * 64 + lane;
  if ((int64_t)blockIdx.x * 256 >= a.n) return;
  const bool valid = slot < a.n;
  const int64_t p = a.order ? (int64_t)a.order[valid ? slot : 0] : (valid ? slot : 0);
  const float scale = a.st[TDR_ST_SCALE * a.cap + p];
  const float cx = a.st[TDR_ST_DX * a.cap + p] * scale + a.st[TDR_ST_INIT_X * a.cap + p];
  const float cy = a.st[TDR_ST_DY * a.cap + p] * scale + a.st[TDR_ST_INIT_Y * a.cap + p];
  const float theta = a.st[TDR_ST_THETA * a.cap + p];
  const float off0 = cy / a.resolution;  // samplePts(center/resolution, ...): x_vals += center[1] (top_down_map.cpp:387)
  const float off1 = cx / a.resolution;  // y_vals += center[0] (:388)
  const float resq = (a.res * scale) / a.resolution;  // res/params_.resolution (:434)
  // cos(rot), sin(rot) of top_down_map.cpp:381-385 = the host libm's cosf / sinf, bit for bit (tdr_sincosf.h)
  const float c = tdr_libm::cosf_v(theta, a.libm_fma), s = tdr_libm::sinf_v(theta, a.libm_fma);
  const float ns = -s;
  typedef float tdr_v2f __attribute__((ext_vector_type(2)));
  const tdr_v2f cs = {c, s}, offv = {off0, off1};
  const float lo_r = (float)((double)(-resq * (float)(a.rows - 1)) / 2.), hi_r = (float)((double)(resq * (float)(a.rows - 1)) / 2.);
  const float lo_c = (float)((double)(-resq * (float)(a.cols - 1)) / 2.), hi_c = (float)((double)(resq * (float)(a.cols - 1)) / 2.);
  const float step_r = a.rows == 1 ? 0.f : (hi_r - lo_r) / (float)(a.rows - 1);
  const float step_c = a.cols == 1 ? 0.f : (hi_c - lo_c) / (float)(a.cols - 1);
  const int r1 = a.rows == 1 ? 1 : a.rows - 1, c1 = a.cols == 1 ? 1 : a.cols - 1;

  const int j0 = blockIdx.y * a.cpc, j1 = min(a.cols, j0 + a.cpc);
  const int rowstride = (a.map_cols + 2) * (RF * 4);
  const int kbase = (a.map_cols + 3) * (RF * 4);
  const float rmaxf = (float)a.map_rows, cmaxf = (float)a.map_cols;
  const char* __restrict__ recb = reinterpret_cast<const char*>(a.rec);
  const char* __restrict__ crecb = reinterpret_cast<const char*>(a.crec);
  const int ckcol = a.ctiles_r * 128 - 16 * CW, ckconst = a.ctiles_r * 128 + 128;   // cmap_offset
  // the scan record of sample (i, j) is the same for every lane: read through the CONSTANT address space = scalar loads
  // whatever else the kernel contains (see score_polar_kernel)
  typedef const float __attribute__((address_space(4))) * tdr_const_f;
  const tdr_const_f scanc = (tdr_const_f)a.scan_pk;

  float acc[RF];
#pragma unroll
  for (int k = 0; k < RF; k++) acc[k] = 0.f;
  float known = 0.f;
  // the record of one sample as RF operands: dense records as they are, compact ones decoded (bit-identical)
  auto fetch = [&](unsigned off, float (&m)[RF]) {
    if constexpr (COMPACT) {
      uint32_t w[CW];
      cmap_load<CW>(crecb, off, w);
      if constexpr (WIDE) cmap_decode_wide<RF, KSLOT>(w, ldict, m);
      else cmap_decode<RF, KSLOT>(w, ldict, m);
    } else {
#pragma unroll
      for (int v = 0; v < NV4; v++) {
        const float4 q = *reinterpret_cast<const float4*>(recb + off + 16 * v);
        m[4 * v + 0] = q.x; m[4 * v + 1] = q.y; m[4 * v + 2] = q.z; m[4 * v + 3] = q.w;
      }
    }
  };
  // rotm * pts (:383-385) for window sample (row value yi, column terms AB = {-s * xj, c * xj}), centre added (:387-388),
  // rounded (:437): both coordinates in packed instructions — the same float operations, two at a time
  auto cell_offset = [&](tdr_v2f cyi, tdr_v2f AB) -> unsigned {
    tdr_v2f pv = cyi + AB;         // p0 = c * yi + (-s * xj), p1 = s * yi + c * xj
    pv = pv + offv;
    tdr_v2f qv = {__builtin_amdgcn_fmed3f(pv.x, -1.f, rmaxf), __builtin_amdgcn_fmed3f(pv.y, -1.f, cmaxf)};
    qv = qv + 0.49999997f;         // see round_half_away_clamped
    int ri, ci;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ri) : "v"(qv.x));
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ci) : "v"(qv.y));
    const bool inb = (unsigned)ri < (unsigned)a.map_rows && (unsigned)ci < (unsigned)a.map_cols;
    if constexpr (COMPACT) return cmap_offset<CW, LC>(ri, ci, ckcol, ckconst);
    else return inb ? (unsigned)(__mul24(ri, rowstride) + (ci * (RF * 4) + kbase)) : 0u;
  };
  auto column_terms = [&](int j) -> tdr_v2f {
    const float xj = linspaced_dev(j, c1, lo_c, hi_c, step_c);
    return (tdr_v2f){ns * xj, c * xj};
  };
  // Order: blocks of U window rows, and within a block the chunk's columns one after the other — a patch of U x cpc
  // neighbouring cells (rotated), so that a lane whose neighbours are far away meets each 4 x 4-cell tile of the compact
  // records once per patch instead of once per column.  (Fixed by the configuration: the sums are a pure function of it.)
  int i = 0;
  for (; i + U <= a.rows - 1; i += U) {   // LinSpaced without the select of its last element; the last row: below
    tdr_v2f cyi[U];
#pragma unroll
    for (int u = 0; u < U; u++) cyi[u] = cs * (lo_r + (float)(i + u) * step_r);
    for (int j = j0; j < j1; j++) {
      const tdr_v2f AB = column_terms(j);
      unsigned boff[U];
#pragma unroll
      for (int u = 0; u < U; u++) boff[u] = cell_offset(cyi[u], AB);
      float m[U][RF];
#pragma unroll
      for (int u = 0; u < U; u++) fetch(boff[u], m[u]);
      const int64_t sbase = ((int64_t)j * a.rows + i) * RF;  // wave-uniform
#pragma unroll
      for (int u = 0; u < U; u++) {
#pragma unroll
        for (int k = 0; k < RF; k++) acc[k] = __builtin_fmaf(scanc[sbase + u * RF + k], m[u][k], acc[k]);
        if (!KSLOT) known += m[u][RF - 1];
      }
    }
  }
  for (; i < a.rows; i++) {   // the remaining rows (the last one among them), column by column
    const tdr_v2f cyi = cs * linspaced_dev(i, r1, lo_r, hi_r, step_r);
    for (int j = j0; j < j1; j++) {
      float m[RF];
      fetch(cell_offset(cyi, column_terms(j)), m);
      const int64_t sbase = ((int64_t)j * a.rows + i) * RF;
#pragma unroll
      for (int k = 0; k < RF; k++) acc[k] = __builtin_fmaf(scanc[sbase + k], m[k], acc[k]);
      if (!KSLOT) known += m[RF - 1];
    }
  }
  if (slot < a.npad) {
    float* o = a.part + (int64_t)blockIdx.y * (RF + 1) * a.npad + slot;
#pragma unroll
    for (int k = 0; k < RF; k++) o[(int64_t)k * a.npad] = acc[k];
    o[(int64_t)RF * a.npad] = KSLOT ? acc[RF - 2] : known;
  }
}

// getLocalMap as a function of its own (src/top_down_map_polar.cpp:21-53, src/top_down_map.cpp:429-459): the window
// of ONE pose written out as the reference's arrays — dists [ncls][rows*cols] column-major images, mask [rows*cols]
// (1 = unknown / out of bounds).  The scoring kernels never materialise it; this is the class-surface method and the
// direct parity check of the window addressing (tests/test_gpu_parity.py::test_local_map_*).  One thread per sample,
// the same float operations as the scoring loops.
struct LocalMapArgs {
  const float* rec;
  int map_rows, map_cols, ncls, rf;
  float resolution;
  const float* tab;     // polar: [P][2]
  int rows, cols;       // window shape (polar: nb x nr)
  float cx, cy, scale_or_rot, res;
  float* dists;
  uint8_t* mask;
  int libm_fma;
};
template <bool POLAR>
__global__ void local_map_kernel(LocalMapArgs a) {
  const int64_t P = (int64_t)a.rows * a.cols;
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= P) return;
  LocalCellArgs g;   // the cell of sample k: tdr_local_cell.h, shared with the vote scatter (tdr_fuse.hip)
  g.map_rows = a.map_rows; g.map_cols = a.map_cols; g.resolution = a.resolution; g.tab = a.tab; g.rows = a.rows;
  g.cols = a.cols; g.cx = a.cx; g.cy = a.cy; g.scale_or_rot = a.scale_or_rot; g.res = a.res; g.libm_fma = a.libm_fma;
  int ri, ci;
  const bool inb = local_map_cell<POLAR>(g, k, ri, ci);
  const float* r = a.rec + ((int64_t)(ri + 1) * (a.map_cols + 2) + (ci + 1)) * a.rf;   // guard ring: always valid
  for (int c = 0; c < a.ncls; c++) a.dists[(int64_t)c * P + k] = inb ? r[c] : 0.f;
  a.mask[k] = inb ? (uint8_t)(r[a.rf - 1] == 0.f ? 1 : 0) : (uint8_t)1;
}
static int launch_local_map(bool polar, const tdr_map_desc* map, const float* tab, int rows, int cols, float cx, float cy,
                            float scale_or_rot, float res, float* dists_out, uint8_t* mask_out, void* stream) {
  if (!map || !map->rec || !dists_out || !mask_out || (polar && !tab))
    return fail(TDR_ERR_ARG, "local_map: null pointer");
  if (rows < 1 || cols < 1) return fail(TDR_ERR_ARG, "local_map: bad window shape");
  if (!(map->resolution > 0.f)) return fail(TDR_ERR_ARG, "local_map: map resolution must be > 0");
  LocalMapArgs a;
  a.rec = map->rec; a.map_rows = map->rows; a.map_cols = map->cols; a.ncls = map->ncls; a.rf = map->rec_floats;
  a.resolution = map->resolution; a.tab = tab; a.rows = rows; a.cols = cols; a.cx = cx; a.cy = cy;
  a.scale_or_rot = scale_or_rot; a.res = res; a.dists = dists_out; a.mask = mask_out;
  a.libm_fma = tdr_libm_fma();
  const dim3 grid((unsigned)cdiv((int64_t)rows * cols, 256)), block(256);
  if (polar) hipLaunchKernelGGL((local_map_kernel<true>), grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((local_map_kernel<false>), grid, block, 0, (hipStream_t)stream, a);
  LAUNCH_CHECK("local_map");
  return TDR_OK;
}
extern "C" int tdr_k_local_map_polar(const tdr_map_desc* map, const float* tab, int nb, int nr, float cx, float cy,
                                     float scale, float res, float* dists_out, uint8_t* mask_out, void* stream) {
  return launch_local_map(true, map, tab, nb, nr, cx, cy, scale, res, dists_out, mask_out, stream);
}
extern "C" int tdr_k_local_map_cart(const tdr_map_desc* map, int rows, int cols, float cx, float cy, float rot,
                                    float res, float* dists_out, uint8_t* mask_out, void* stream) {
  return launch_local_map(false, map, nullptr, rows, cols, cx, cy, rot, res, dists_out, mask_out, stream);
}

struct FinalizeArgs {
  const float* part;
  int rf, nchunks;
  int64_t npad, n, cap;
  const int32_t* order;
  const int32_t* count = nullptr;   // optional device count limiting the active slots (unused, see ScoreArgs::count)
  float* st;
  tdr_filter_params fp;
  GateArgs gate;
  int64_t P;
  int ncls;
  int mode = 0;         // 0: write raw weight; 1: init-search accumulate (best cost / theta)
  int first = 0;        // mode 1: first rotation (initialise best)
  float theta_override = 0.f;
  float* raw_w;
  float* best_cost = nullptr;
  float* best_theta = nullptr;
  // the geometric term of getCostForRot (state_particle.cpp:145-152, commented out in the reference; opt-in here):
  // partial sums of a second scoring launch over the 2-layer geometric map and the sums of the two geometric scan images
  const float* gpart = nullptr;   // [gnchunks][5][npad], NULL = no geometric term
  int gnchunks = 0;
  float gsum0 = 0.f, gsum1 = 0.f;
  int only_uninit = 0;  // mode 1: slots whose particle already has a heading are left alone
  int tlog = 0;         // 2^tlog neighbouring lanes share a slot's chunks (launch_finalize)
  const int32_t* run_if = nullptr;   // optional device words: run only when the integer form is off (see ScoreArgs)
  // the integer form (score_finalize_exact_kernel): the head of `part` holds the launch's integer sums
  const uint32_t* ipart = nullptr;   // [2 ncls + 2][npad]: int_add_sums (tdr_score_int_dev.h)
  const uint32_t* dict_tail = nullptr;   // {q, ...}: a sum is a multiple of 2^-q
  const int32_t* counts = nullptr;   // {slots of the dense share, scattered particles, all slots}
  const int32_t* inexact = nullptr;
};

// the body of score_finalize_kernel and of score_finalize_batch_kernel, for thread gid of the launch
__device__ __forceinline__ void score_finalize_body(const FinalizeArgs& a, const int64_t gid) {
  const int T = 1 << a.tlog, t = (int)(gid & (T - 1));
  const int64_t slot = gid >> a.tlog;
  if (a.run_if && !int_form_off(a.run_if)) return;
  const int64_t nact = a.count ? (int64_t)*a.count : a.n;
  if (slot >= nact) return;
  const int64_t p = a.order ? (int64_t)a.order[slot] : slot;
  if (p < 0) return;   // a padding slot of the shift-uniform order (tdr_score_su.h)
  const float scale = a.st[TDR_ST_SCALE * a.cap + p];
  const float cx = a.st[TDR_ST_DX * a.cap + p] * scale + a.st[TDR_ST_INIT_X * a.cap + p];
  const float cy = a.st[TDR_ST_DY * a.cap + p] * scale + a.st[TDR_ST_INIT_Y * a.cap + p];
  if (a.mode == 0 && particle_gated(a.gate, cx, cy, scale)) {
    a.raw_w[p] = 0.f;
    return;
  }
  if (a.mode == 1 && a.only_uninit && a.st[TDR_ST_HAVE_INIT * a.cap + p] != 0.f) return;
  // Per-chunk partial sums -> double totals, chunk order ascending.  The loads of FIN_B chunks x all slots are issued
  // together (independent addresses, coalesced over the particles) before the dependent additions.  A small particle
  // set has many chunks and few slots — 128 x 1000 at the reference's test size — and one lane per slot would wait for
  // memory 32 times in a row: there 2^tlog neighbouring lanes take a contiguous share of a slot's chunks each and
  // their double totals are added up in a fixed butterfly.
  constexpr int FIN_B = 4, FIN_S = TDR_MAX_CLASSES + 2;   // slots: ncls class dots, normalisation, known count
  double tot[FIN_S];
#pragma unroll
  for (int k = 0; k < FIN_S; k++) tot[k] = 0;
  const int64_t cstride = (int64_t)(a.rf + 1) * a.npad;
  auto slot_row = [&](int k) { return k < a.ncls ? k : (k == a.ncls ? a.rf - 1 : a.rf); };
  const int share = (a.nchunks + T - 1) >> a.tlog, cend = min(a.nchunks, (t + 1) * share);
  int c0 = t * share;
  for (; c0 + FIN_B <= cend; c0 += FIN_B) {
    float v[FIN_B][FIN_S];
#pragma unroll
    for (int b = 0; b < FIN_B; b++)
#pragma unroll
      for (int k = 0; k < FIN_S; k++)
        if (k < a.ncls + 2) v[b][k] = a.part[(int64_t)(c0 + b) * cstride + (int64_t)slot_row(k) * a.npad + slot];
#pragma unroll
    for (int b = 0; b < FIN_B; b++)
#pragma unroll
      for (int k = 0; k < FIN_S; k++)
        if (k < a.ncls + 2) tot[k] += (double)v[b][k];
  }
  for (; c0 < cend; c0++) {
#pragma unroll
    for (int k = 0; k < FIN_S; k++)
      if (k < a.ncls + 2) tot[k] += (double)a.part[(int64_t)c0 * cstride + (int64_t)slot_row(k) * a.npad + slot];
  }
  if (T > 1) {   // (the lanes of a slot left or stayed together above)
    for (int sft = T >> 1; sft >= 1; sft >>= 1)
#pragma unroll
      for (int k = 0; k < FIN_S; k++)
        if (k < a.ncls + 2) tot[k] += __shfl_xor(tot[k], sft, 64);
    if (t != 0) return;
  }
  double known = 0, norm = 0;
#pragma unroll
  for (int k = 0; k < FIN_S; k++) {
    if (k == a.ncls) norm = tot[k];
    if (k == a.ncls + 1) known = tot[k];
  }
  // known fraction gate (state_particle.cpp:117-120); counts are exact integers in float
  float cost;
  if ((float)known / (float)a.P < 0.5) {
    cost = __builtin_nanf("");
  } else {
    cost = 0.f;
#pragma unroll
    for (int k = 0; k < TDR_MAX_CLASSES; k++)
      if (k < a.ncls) cost = (float)((double)cost + (double)(float)tot[k] * 0.01 * (double)a.fp.class_weights[k]);  // :136-139
    float normf = (float)norm;
    if (a.gpart) {   // :145-152: cost += (geo_i . geo_cls_i) * 0.01; normalization += geo_i.sum()
      double g[2] = {0, 0};
      const int64_t gstride = (int64_t)5 * a.npad;
      for (int c0g = 0; c0g < a.gnchunks; c0g++) {
        g[0] += (double)a.gpart[(int64_t)c0g * gstride + slot];
        g[1] += (double)a.gpart[(int64_t)c0g * gstride + a.npad + slot];
      }
      cost = (float)((double)cost + (double)(float)g[0] * 0.01);
      normf = normf + a.gsum0;
      cost = (float)((double)cost + (double)(float)g[1] * 0.01);
      normf = normf + a.gsum1;
    }
    cost = cost / normf;  // :154
  }
  if (a.mode == 0) {
    a.raw_w[p] = (float)(1. / (double)(cost + a.fp.regularization));  // :212
  } else {
    float best = a.first ? 3.402823466e+38f : a.best_cost[slot];
    float bt = a.first ? 0.f : a.best_theta[slot];
    if (cost < best) { best = cost; bt = a.theta_override; }  // :200-203 (NaN never wins)
    a.best_cost[slot] = best;
    a.best_theta[slot] = bt;
  }
}
__global__ __launch_bounds__(256) void score_finalize_kernel(FinalizeArgs a) {
  score_finalize_body(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}
// ... behind the exact finalize (a.run_if set): a bounded grid that reads the flag once and walks the launch's threads
// (`total`, whole workgroups) in strides of the grid
__global__ __launch_bounds__(256) void score_finalize_bounded_kernel(FinalizeArgs a, int64_t total) {
  if (!int_form_off(a.run_if)) return;   // (uniform)
  a.run_if = nullptr;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x)
    score_finalize_body(a, g);
}
__global__ __launch_bounds__(256) void score_finalize_batch_kernel(const FinalizeArgs* __restrict__ args,
                                                                   const int32_t* __restrict__ blk, int k) {
  const int e = batch_find(k, (int)blockIdx.x, [&](int i) { return blk[i]; });
  const FinalizeArgs a = args[e];
  score_finalize_body(a, (int64_t)(blockIdx.x - (unsigned)blk[e]) * blockDim.x + threadIdx.x);
}

// The integer form of a launch (tdr_score_su.hip, tdr_score_ray.hip): per slot and class ONE 64-bit integer sum of count x
// (distance 2^q) over the window's samples, and the normalisation and the known-cell count as integers — every row of the
// dense kernel and every wave of the ray-mapped one has added its share in place (int_add_sums, tdr_score_int_dev.h).
// Integer sums are exact: whatever kernel, split or order produced the shares, their total is the same number, and
// so is the weight.  dot_c = total 2^-q rounded to float once (the reference: a float sum of float products in Eigen's
// order, state_particle.cpp:136-138), then the reference's own arithmetic (:136-139, 154, 212).  One thread per slot: it reads
// 2 ncls + 2 words.
// A 64-bit total as a double that rounds to float exactly as the total itself does: up to 53 bits the total; past that
// (double)total would be a rounding of its own, and the float made from it a number rounded TWICE (a total just above the
// middle of two floats lands ON the middle and goes down) — so the 53 leading bits, the last of them set when any bit below
// it is (rounding to odd: a float keeps 24 of them, whether the rest lies below, on or above the middle stays visible).
__device__ __forceinline__ double u64_to_double_sticky(unsigned long long v) {
  const int drop = 11 - __clzll(v);   // bits past the 53rd
  if (drop <= 0) return (double)v;
  const unsigned long long kept = (v >> drop) | ((v & ((1ull << drop) - 1ull)) != 0ull ? 1ull : 0ull);
  return ldexp((double)kept, drop);
}
__global__ __launch_bounds__(256) void score_finalize_exact_kernel(FinalizeArgs a) {
  if (int_form_off(a.inexact)) return;
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= (int64_t)a.counts[2]) return;
  const unsigned long long* const s64 = reinterpret_cast<const unsigned long long*>(a.ipart) + slot;
  unsigned long long tot[TDR_MAX_CLASSES];
#pragma unroll
  for (int k = 0; k < TDR_MAX_CLASSES; k++) tot[k] = k < a.ncls ? s64[(int64_t)k * a.npad] : 0ull;
  const unsigned long long norm = a.ipart[(int64_t)(2 * a.ncls) * a.npad + slot];
  const unsigned long long known = a.ipart[(int64_t)(2 * a.ncls + 1) * a.npad + slot];
  const int64_t p = a.order[slot];
  if (p < 0) return;   // a padding slot of the shift-uniform order
  const float scale = a.st[TDR_ST_SCALE * a.cap + p];
  const float cx = a.st[TDR_ST_DX * a.cap + p] * scale + a.st[TDR_ST_INIT_X * a.cap + p];
  const float cy = a.st[TDR_ST_DY * a.cap + p] * scale + a.st[TDR_ST_INIT_Y * a.cap + p];
  if (particle_gated(a.gate, cx, cy, scale)) {
    a.raw_w[p] = 0.f;
    return;
  }
  float cost;
  if ((float)known / (float)a.P < 0.5) {   // state_particle.cpp:117-120
    cost = __builtin_nanf("");
  } else {
    const int q = (int)a.dict_tail[0];
    cost = 0.f;
#pragma unroll
    for (int k = 0; k < TDR_MAX_CLASSES; k++)
      if (k < a.ncls) {
        const float dot = (float)ldexp(u64_to_double_sticky(tot[k]), -q);   // ONE rounding
        cost = (float)((double)cost + (double)dot * 0.01 * (double)a.fp.class_weights[k]);  // :136-139
      }
    cost = cost / (float)norm;  // :154
  }
  a.raw_w[p] = (float)(1. / (double)(cost + a.fp.regularization));  // :212
}

// FinalizeArgs::tlog: 2^tlog lanes per slot while each still has four chunks and the launch stays within 131 072 lanes
static int finalize_tlog(int nchunks, int64_t nslots) {
  int tl = 0;
  while (tl < 4 && (nchunks >> (tl + 1)) >= 4 && (nslots << (tl + 1)) <= 131072) tl++;
  return tl;
}
// nslots: slots the launch covers (a.n / a.count still bound the active ones)
// Workgroups of a launch that runs only while the integer form is off (run_if): what the chip holds resident — `per_cu` of them
// on each compute unit — and never more than a quarter of TdrConfig::score_waves (four waves a workgroup: tests make it small)
static int64_t bounded_grid(int64_t units, int per_cu) {
  static int cus = 0;   // (one kind of device per process)
  if (cus <= 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
    else return std::max<int64_t>(1, std::min<int64_t>(units, 256 * per_cu));
  }
  const int64_t cap = std::min<int64_t>((int64_t)cus * per_cu, std::max<int64_t>(1, tdr_cfg().score_waves / 4));
  return std::max<int64_t>(1, std::min(units, cap));
}
// bounded (the polar call's float form behind its integer kernels; f.run_if set): the bounded grid
static void launch_finalize(FinalizeArgs& f, int64_t nslots, hipStream_t s, bool bounded = false) {
  f.tlog = finalize_tlog(f.nchunks, nslots);
  const int64_t blocks = cdiv(nslots << f.tlog, 256);
  if (bounded && f.run_if)
    hipLaunchKernelGGL(score_finalize_bounded_kernel, dim3((unsigned)bounded_grid(blocks, 8)), dim3(256), 0, s, f, blocks * 256);
  else
    hipLaunchKernelGGL(score_finalize_kernel, dim3((unsigned)blocks), dim3(256), 0, s, f);
}

// the Cartesian kernel likes twice as many, shorter waves (A/B on MI355X, config 4: x1 183 ms, x2 179 ms, x4 177 ms)
#define TDR_CART_WAVE_MUL 2
static void choose_chunks(int64_t n, int nr, int& rpc, int& nchunks, int target_mul = 1) {
  int64_t nbatches = cdiv(std::max<int64_t>(n, 1), 64);
  int64_t want = std::max<int64_t>(1, cdiv(tdr_cfg().score_waves * target_mul, nbatches));  // enough waves to fill the chip
  nchunks = (int)std::min<int64_t>(nr, want);
  rpc = (int)cdiv(nr, nchunks);
  nchunks = (int)cdiv(nr, rpc);
}

__global__ void utab_kernel(const float* __restrict__ tab, int64_t n2, float scale, float res,
                            float* __restrict__ utab) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n2) utab[k] = (tab[k] * scale) * res;  // `ang_sample_pts_*scale*res` (top_down_map_polar.cpp:28)
}

// Rings per workgroup of score_polar_kernel.  Larger groups give a ray more consecutive cells (tile reuse) and fewer,
// longer workgroups; a small filter needs many short ones to fill 256 CUs.  So the group is sized from the image shape
// (the group's scan rows must fit the LDS budget; 32 KB keeps four workgroups per CU; at most 8 rings; whole steps of
// TDR_SCORE_U) and from the TOTAL particle count of the filter — n_total, the same on every rank of a sharded filter,
// never the size of one launch or shard: the partition of a particle's score into partial sums is then the same in an
// N-rank run as in the 1-rank run.  Aim: >= 2048 workgroups.  tdr_config_tuning("score_group", g) overrides (tuning).
static int score_group_rings(int nb, int nr, int rf, int64_t n_total) {
  const int forced = tdr_cfg().score_group;
  const int64_t ring_bytes = std::max<int64_t>((int64_t)nb * rf * 4, 1);
  int g = (int)std::min<int64_t>(8, (32 * 1024) / ring_bytes);
  const int64_t chunks_wanted = cdiv(2048, cdiv(std::max<int64_t>(n_total, 1), 256));
  g = (int)std::min<int64_t>(g, std::max<int64_t>(1, nr / std::max<int64_t>(chunks_wanted, 1)));
  if (forced > 0) g = forced;
  g = std::max(1, std::min<int>(g, (int)((60 * 1024) / ring_bytes)));
  if (g >= TDR_SCORE_U) g -= g % TDR_SCORE_U;
  return std::max(g, 1);
}
// The scoring workspace (floats): [partial sums nchunks*(rf+1)*npad_part][res_flag | best_cost npad][res_theta |
// best_theta npad][list npad + 64: rotation table of the init search][uniform-scale table 2*nb*nr][shift-uniform order,
// tdr_score_su.h].  npad_part = the slot count of the shift-uniform order where the shapes allow it (its partial sums are
// slot-indexed and the slots include the padding), else npad.
struct ScoreWs {
  int group, nchunks;
  int su_group, su_nchunks;   // the ring groups of the shift-uniform kernel (integer sums: any partition gives the same bits)
  int su_tail_k, su_tail_q, su_rows;   // ... the last of them cut by sector: rows of partial sums per dense slot (su_tail_plan)
  int64_t npad, npad_part, off_aux, off_utab, off_su, total;
  bool su;
  SuWs suw;
};
static ScoreWs score_ws(int ncls, int nb, int nr, int64_t n, int64_t n_total) {
  ScoreWs w;
  const int rf = tdr_rec_floats(ncls);
  if (n_total <= 0) n_total = n;
  w.group = score_group_rings(nb, nr, rf, n_total);
  // the shift-uniform kernel steps through a ray four rings at a time: where it can take the launch the groups are whole
  // fours (a small filter's single-ring groups — the reference's 20 000 particles on 100 x 25 bins — become groups of 4; the
  // last group of an image whose ring count is no multiple of 4 is ragged)
  if (w.group % 4 != 0 && tdr_cmap_words(ncls) != 0 && tdr_su_shape_ok(nb, nr, 4, n_total))
    w.group = std::max(4, w.group - w.group % 4);
  w.nchunks = (int)cdiv(nr, w.group);
  w.npad = cdiv(std::max<int64_t>(n, 1), 64) * 64;
  w.su = tdr_su_shape_ok(nb, nr, w.group, n_total) && tdr_cmap_words(ncls) != 0;
  w.su_group = w.group;
  {
    const int forced = tdr_cfg().su_group;
    // eight rings per group where that divides the image and still leaves thousands of workgroups: a sector's mask is
    // staged half as often (config 2: 3.50 against 3.56 ms; 16 rings: 3.69, the staged boxes grow)
    if (w.su && w.group == 4 && nr % 8 == 0 && cdiv(n_total, 256) * (nr / 8) >= 4096) w.su_group = 8;
    // sixteen where the launch's last groups go as short rows (tail units, tdr_su_tail): the run-down that made long groups
    // lose is gone, and mask stagings, descriptor streams and finalize rows halve again (config 2: 4.41 ms a step with 8-ring
    // groups and tail units, 4.32 with 16; 32 rings: 5.8 — the staged boxes outgrow LDS).  By THIS launch's particle count:
    // integer sums do not care, and a rank's shard must still fill the chip.
    int k16 = 0, q16 = 1;
    if (w.su && w.su_group == 8 && nr % 16 == 0 && cdiv(std::max<int64_t>(n, 1), 256) * (nr / 16) >= 4096)
      tdr_su_tail(nr / 16, std::max<int64_t>(n, 1), &k16, &q16);
    if (k16 > 0) w.su_group = 16;
    if (w.su && forced >= 4 && forced % 4 == 0) w.su_group = forced;
  }
  w.su_nchunks = (int)cdiv(nr, w.su_group);
  tdr_su_tail(w.su_nchunks, std::max<int64_t>(n, 1), &w.su_tail_k, &w.su_tail_q);
  {
    int g, s0, s1;
    w.su_rows = su_tail_plan(w.su_nchunks, w.su_tail_k, w.su_tail_q, -1, &g, &s0, &s1);
  }
  w.npad_part = w.su ? su_npad(std::max<int64_t>(n, 1), nb) : w.npad;
  // partial sums: [chunks][rows][slots] — the float form's rf + 1 rows per chunk.  The integer form (tdr_score_su.hip,
  // tdr_score_ray.hip) needs ONE block of 2 ncls + 2 rows of words at the head, which every row and wave adds to
  // (tdr_score_int_dev.h); the sizing still counts a block per row of the grid, as it did when each row wrote its own
  w.off_aux = w.su ? (int64_t)std::max(std::max(w.nchunks, w.su_rows), TDR_RAY_MAX_SPLIT) * std::max(rf + 1, 2 * ncls + 2) * w.npad_part
                   : (int64_t)w.nchunks * (rf + 1) * w.npad_part;
  w.off_utab = w.off_aux + 3 * w.npad + 64;
  w.off_su = (w.off_utab + 2 * (int64_t)nb * nr + 63) / 64 * 64;
  w.total = w.off_su;
  if (w.su) {
    w.suw = tdr_su_ws(nb, nr, w.su_group, std::max<int64_t>(n, 1));
    w.total += w.suw.total;
  }
  return w;
}
extern "C" size_t tdr_score_workspace_floats(int ncls, int nb, int nr, int64_t n, int64_t n_total) {
  if (ncls < 1 || ncls > TDR_MAX_CLASSES || nb < 1 || nr < 1 || n < 0) return 0;
  return (size_t)score_ws(ncls, nb, nr, n, n_total).total;
}
static int fill_utab(ScoreArgs& a, float* workspace, const ScoreWs& W, float uniform_scale, hipStream_t s) {
  a.utab = nullptr;
  if (!(uniform_scale > 0.f)) return TDR_OK;
  float* ut = workspace + W.off_utab;
  const int64_t n2 = 2 * (int64_t)a.nb * a.nr;
  hipLaunchKernelGGL(utab_kernel, dim3((unsigned)cdiv(n2, 256)), dim3(256), 0, s, a.tab, n2, uniform_scale, a.res, ut);
  LAUNCH_CHECK("utab");
  a.utab = ut;
  return TDR_OK;
}

// Optional in-library timing of the dominant kernel (bench.py's roofline figure): HIP events recorded on the launch
// stream right around score_polar_kernel, read back after the timed region.
static bool g_prof_on = false;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_events;
static size_t g_prof_used = 0;
struct ScoreProfScope {
  hipStream_t s;
  hipEvent_t stop = nullptr;
  explicit ScoreProfScope(hipStream_t s_, bool on = true) : s(s_) {
    if (!g_prof_on || !on) return;
    if (g_prof_used == g_prof_events.size()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
      g_prof_events.emplace_back(a, b);
    }
    auto& ev = g_prof_events[g_prof_used++];
    (void)hipEventRecord(ev.first, s);
    stop = ev.second;
  }
  ~ScoreProfScope() {
    if (stop) (void)hipEventRecord(stop, s);
  }
};
// ... and of each of the two kernels of an integer-form launch on its own: the last launch's {dense, scattered} durations
// and the device words that say how many particles each share held (tdr_profile_shares).
static hipEvent_t g_share_ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
static bool g_share_valid = false;
static const int32_t* g_share_counts = nullptr;
struct ShareProfScope {
  hipStream_t s;
  hipEvent_t stop = nullptr;
  ShareProfScope(int which, hipStream_t s_, bool on) : s(s_) {
    if (!g_prof_on || !on) return;
    for (int k = 0; k < 2; k++)
      if (!g_share_ev[which][k] && hipEventCreate(&g_share_ev[which][k]) != hipSuccess) return;
    (void)hipEventRecord(g_share_ev[which][0], s);
    stop = g_share_ev[which][1];
  }
  ~ShareProfScope() {
    if (stop) (void)hipEventRecord(stop, s);
  }
};
// ... and which loop VARIANT the dense kernels' waves ran, counted on the device while profiling is on (16 counters, see
// tdr_profile_variants in tdr.h): what fraction of the wave-sectors / wave-segments found every reachable cell known.
static uint32_t* g_variant_stats = nullptr;
static bool g_prof_variants = false;   // tdr_profile_enable(2): the counters cost the kernels an atomic per wave-sector
uint32_t* tdr_profile_stats_ptr() {   // NULL unless the variant counters are on (the kernels then count nothing)
  if (!g_prof_on || !g_prof_variants) return nullptr;
  if (!g_variant_stats) {
    if (hipMalloc((void**)&g_variant_stats, 16 * sizeof(uint32_t)) != hipSuccess) { g_variant_stats = nullptr; return nullptr; }
    (void)hipMemset(g_variant_stats, 0, 16 * sizeof(uint32_t));
  }
  return g_variant_stats;
}
extern "C" int tdr_profile_variants(int64_t out[16]) {   // reads and resets (synchronises)
  if (!out) return fail(TDR_ERR_ARG, "profile_variants: null pointer");
  for (int k = 0; k < 16; k++) out[k] = 0;
  if (!g_variant_stats) return TDR_OK;
  uint32_t h[16];
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h, g_variant_stats, sizeof(h), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(g_variant_stats, 0, sizeof(h)));
  for (int k = 0; k < 16; k++) out[k] = h[k];
  return TDR_OK;
}
// ... and how the ray-mapped kernel's gate count ended for each scattered particle (tdr_profile_ray_gate in tdr.h)
static uint32_t* g_gate_stats = nullptr;
uint32_t* tdr_profile_gate_ptr() {
  if (!g_prof_on || !g_prof_variants) return nullptr;
  if (!g_gate_stats) {
    if (hipMalloc((void**)&g_gate_stats, 4 * sizeof(uint32_t)) != hipSuccess) { g_gate_stats = nullptr; return nullptr; }
    (void)hipMemset(g_gate_stats, 0, 4 * sizeof(uint32_t));
  }
  return g_gate_stats;
}
// ... and what became of the shift-uniform kernel's bins with several classes (tdr_profile_su_list in tdr.h)
static uint32_t* g_su_list_stats = nullptr;
uint32_t* tdr_profile_su_list_ptr() {
  if (!g_prof_on || !g_prof_variants) return nullptr;
  if (!g_su_list_stats) {
    if (hipMalloc((void**)&g_su_list_stats, 2 * sizeof(uint32_t)) != hipSuccess) { g_su_list_stats = nullptr; return nullptr; }
    (void)hipMemset(g_su_list_stats, 0, 2 * sizeof(uint32_t));
  }
  return g_su_list_stats;
}
extern "C" int tdr_profile_su_list(int64_t out[2]) {   // reads and resets (synchronises)
  if (!out) return fail(TDR_ERR_ARG, "profile_su_list: null pointer");
  out[0] = out[1] = 0;
  if (!g_su_list_stats) return TDR_OK;
  uint32_t h[2];
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h, g_su_list_stats, sizeof(h), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(g_su_list_stats, 0, sizeof(h)));
  out[0] = h[0]; out[1] = h[1];
  return TDR_OK;
}
extern "C" int tdr_profile_ray_gate(int64_t out[4]) {   // reads and resets (synchronises)
  if (!out) return fail(TDR_ERR_ARG, "profile_ray_gate: null pointer");
  for (int k = 0; k < 4; k++) out[k] = 0;
  if (!g_gate_stats) return TDR_OK;
  uint32_t h[4];
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h, g_gate_stats, sizeof(h), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(g_gate_stats, 0, sizeof(h)));
  for (int k = 0; k < 4; k++) out[k] = h[k];
  return TDR_OK;
}
extern "C" int tdr_profile_enable(int on) {
  g_prof_on = on != 0;
  g_prof_variants = on == 2;
  g_prof_used = 0;
  g_share_valid = false;
  return TDR_OK;
}
extern "C" int tdr_profile_shares(double* dense_ms, double* scattered_ms, int64_t* scattered_particles) {
  if (!dense_ms || !scattered_ms || !scattered_particles) return fail(TDR_ERR_ARG, "profile_shares: null pointer");
  if (!g_share_valid || !g_share_counts) return fail(TDR_ERR_ARG, "profile_shares: no integer-form launch was profiled");
  float ms[2] = {0.f, 0.f};
  for (int k = 0; k < 2; k++) {
    HIP_TRY(hipEventSynchronize(g_share_ev[k][1]));
    HIP_TRY(hipEventElapsedTime(&ms[k], g_share_ev[k][0], g_share_ev[k][1]));
  }
  int32_t counts[3] = {0, 0, 0};
  HIP_TRY(hipMemcpy(counts, g_share_counts, sizeof(counts), hipMemcpyDeviceToHost));
  *scattered_ms = ms[0];
  *dense_ms = ms[1];
  *scattered_particles = counts[1];
  return TDR_OK;
}
extern "C" int tdr_profile_score_ms(double* total_ms, int64_t* launches) {
  if (!total_ms || !launches) return fail(TDR_ERR_ARG, "profile_score_ms: null pointer");
  double tot = 0;
  for (size_t i = 0; i < g_prof_used; i++) {
    HIP_TRY(hipEventSynchronize(g_prof_events[i].second));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, g_prof_events[i].first, g_prof_events[i].second));
    tot += ms;
  }
  *total_ms = tot;
  *launches = (int64_t)g_prof_used;
  g_prof_used = 0;
  return TDR_OK;
}

// The scoring loops address map records with 32-bit byte offsets (v_mad_i32_i24 + 32-bit adds): the guarded record
// grid must stay below 4 GiB (11 583^2 cells of 32 bytes) and a guarded row below 2^24 bytes.
static int check_map_addressing(const tdr_map_desc* map, int rf, const char* who) {
  const uint64_t row_bytes = (uint64_t)(map->cols + 2) * rf * 4;
  const uint64_t total = row_bytes * (uint64_t)(map->rows + 2);
  if (row_bytes >= (1u << 24) || total > 0xFFFFFFFFull)
    return fail(TDR_ERR_ARG, "%s: map of %d x %d cells (%d-float records) exceeds the 4 GiB the kernels address", who,
                map->rows, map->cols, rf);
  return TDR_OK;
}

static bool map_is_wide(const tdr_map_desc* map, int rf) {   // tdr_cmap.hip: 16-bit fields
  return rf == 8 && map->cwords == 4 && map->dict_n > TDR_CMAP_MAX_DICT;
}
static int compact_lc(const tdr_map_desc* map) {   // a tile of compact records = (1 << lc) rows x 4 columns (CmapShape::LC)
  return map->cwords == 1 ? 3 : (map->cwords == 2 ? 2 : 1);
}
static bool map_has_compact(const tdr_map_desc* map, int rf) {
  if (!(tdr_cfg().use_compact && map->cwords > 0 && map->crec && map->dict && map->dict_n > 0 && rf <= 12 &&
        (map->cwords == tdr_cmap_words(map->ncls) || map_is_wide(map, rf))))
    return false;
  if (map->dict_n > (map_is_wide(map, rf) ? TDR_CMAP_WIDE_MAX_DICT : TDR_CMAP_MAX_DICT)) return false;
  return (int64_t)((map->rows >> compact_lc(map)) + 2) * 128 < (1 << 23) && map->cols < (1 << 24);   // cmap_offset: 24-bit operands
}
// The compact-record fields of ScoreArgs / CartArgs: the map's compact form where it has one and it is in use, else none.
// Returns whether the COMPACT instantiations apply.
template <class Args>
static bool set_compact(Args& a, const tdr_map_desc* map, int rf) {
  const bool cm = map_has_compact(map, rf);
  a.crec = cm ? map->crec : nullptr;
  a.dict = cm ? map->dict : nullptr;
  a.dict_n = cm ? map->dict_n : 0;
  a.ctiles_r = cm ? (map->rows >> compact_lc(map)) + 2 : 0;
  return cm;
}
// dynamic LDS of the polar kernel: [row][group * planes | 1] float4 (the dictionary is static LDS on top)
static size_t polar_lds_bytes(int nb, int group, int rf) { return (size_t)nb * ((group * (rf / 4)) | 1) * 16; }

// The instantiation of score_polar_kernel (BATCH: score_polar_batch_kernel) for this map: f(kernel).  Compact records
// exist up to 12-float records, wide ones for 8-float records only: no other combination is instantiated.
// (KIND: 0 score_polar_kernel, 1 score_polar_batch_kernel, 2 score_polar_bounded_kernel)
template <int KIND, class F>
static int with_polar_kernel(const tdr_map_desc* map, int rf, bool us, const char* who, F&& f) {
  const bool cm = map_has_compact(map, rf);
  return with_nv4(rf, who, [&](auto N) {
    return with_flags([&](auto KS, auto US, auto CM, auto WD) {
      constexpr int NV4 = decltype(N)::value;
      constexpr bool ks = decltype(KS)::value, usc = decltype(US)::value, c = decltype(CM)::value, w = decltype(WD)::value;
      if constexpr ((c && NV4 == 4) || (w && !(c && NV4 == 2))) return fail(TDR_ERR_ARG, "%s: no kernel for this record form", who);
      else if constexpr (KIND == 1) return f(score_polar_batch_kernel<NV4, TDR_SCORE_U, ks, usc, c, w>);
      else if constexpr (KIND == 2) return f(score_polar_bounded_kernel<NV4, TDR_SCORE_U, ks, usc, c, w>);
      else return f(score_polar_kernel<NV4, TDR_SCORE_U, ks, usc, c, w>);
    }, tdr_has_kslot(map->ncls, rf), us, cm, cm && map_is_wide(map, rf));
  });
}
template <class K>
static void allow_lds(K kfn, size_t lds) {   // more dynamic LDS than a kernel may ask for by default
  if (lds > 65536) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}
static int launch_score(ScoreArgs a, const tdr_map_desc* map, int rf, hipStream_t s, bool profile = true) {
  ScoreProfScope prof(profile ? s : nullptr, profile);
  set_compact(a, map, rf);
  const dim3 grid((unsigned)cdiv(a.n, 256), (unsigned)a.nchunks), block(256);
  const size_t lds = polar_lds_bytes(a.nb, a.group, rf);
  if (a.run_if) {   // the float form behind the integer kernels: a bounded grid that leaves when the flag is clear
    const bool cm = map_has_compact(map, rf);
    const int per_cu = cm ? (map_is_wide(map, rf) ? 3 : 5) : 1;   // score_polar_bounded_kernel's launch bounds
    const dim3 bgrid((unsigned)bounded_grid((int64_t)grid.x * grid.y, per_cu));
    if (int rc = with_polar_kernel<2>(map, rf, a.utab != nullptr, "score", [&](auto kfn) {
          allow_lds(kfn, lds);
          hipLaunchKernelGGL(kfn, bgrid, block, lds, s, a, grid.x, grid.y);
          return TDR_OK;
        }))
      return rc;
    LAUNCH_CHECK("score_polar_bounded");
    return TDR_OK;
  }
  if (int rc = with_polar_kernel<0>(map, rf, a.utab != nullptr, "score", [&](auto kfn) {
        allow_lds(kfn, lds);
        hipLaunchKernelGGL(kfn, grid, block, lds, s, a);
        return TDR_OK;
      }))
    return rc;
  LAUNCH_CHECK("score_polar");
  return TDR_OK;
}

// tdr_score_ctx (tdr.h): what a scoring call keeps BETWEEN calls — the span tuner of tdr_score_su.h.  It belongs to one
// caller (a filter handle): nothing of it is shared between filters, threads or devices.  Without a context a call uses
// the configured span.  (Rounds 3 and 4 also gave a call a stream of its own to run its two kernels side by side: measured
// on every configuration, the two never overlapped usefully — config 2: 5.22 ms on one stream, 5.32 on two; config 5: 16.4
// against 17.0 — because the dense kernel waits for its gathers right after issuing them and becomes latency-bound as soon
// as another kernel fills the L1's queues.  The kernels of a call now run one after the other on the caller's stream.)
struct tdr_score_ctx {
  int device = 0;
  SpanTuner tuner;
  const float* fac = nullptr;   // the table's factors on the device (tdr_polar_factors_host), the caller's memory
  int fac_nb = 0, fac_nr = 0;
};
extern "C" int tdr_score_ctx_set_polar_factors(tdr_score_ctx* c, const float* fac_dev, int nb, int nr) {
  if (!c || (fac_dev && (nb < 1 || nr < 1))) return fail(TDR_ERR_ARG, "score_ctx_set_polar_factors: bad arguments");
  c->fac = fac_dev;
  c->fac_nb = fac_dev ? nb : 0;
  c->fac_nr = fac_dev ? nr : 0;
  return TDR_OK;
}
extern "C" int tdr_score_ctx_create(tdr_score_ctx** out) {
  if (!out) return fail(TDR_ERR_ARG, "score_ctx_create: null pointer");
  *out = nullptr;
  tdr_score_ctx* c = new (std::nothrow) tdr_score_ctx;
  if (!c) return fail(TDR_ERR_NOMEM, "score_ctx_create: out of memory");
  const hipError_t e = hipGetDevice(&c->device);
  if (e != hipSuccess) {
    delete c;
    return fail(TDR_ERR_HIP, "score_ctx_create: %s", hipGetErrorString(e));
  }
  *out = c;
  return TDR_OK;
}
extern "C" void tdr_score_ctx_destroy(tdr_score_ctx* c) {
  if (!c) return;
  if (c->tuner.e0) (void)hipEventDestroy(c->tuner.e0);
  if (c->tuner.e1) (void)hipEventDestroy(c->tuner.e1);
  delete c;
}
extern "C" float tdr_score_ctx_span(const tdr_score_ctx* c) {   // the span the context's tuner has settled on so far
  return c ? c->tuner.best : tdr_cfg().su_span;
}
extern "C" int64_t tdr_score_ctx_trial_calls(const tdr_score_ctx* c) {   // launches spent on trial spans so far
  return c ? c->tuner.trial_calls : 0;
}
// closes the tuner's measurement on EVERY way out of a call
struct TunerScope {
  tdr_score_ctx* c;
  hipStream_t s;
  TunerScope(tdr_score_ctx* c_, hipStream_t s_) : c(c_), s(s_) {}
  ~TunerScope() {
    if (c) tdr_su_span_end(&c->tuner, s);
  }
};

// The launch's choice between the integer form (tdr_score_su.h) and the float kernel, taken on the host: one place for
// tdr_k_score_polar_ctx and for the callers that must know which form a filter's launch takes (tdr_batch_step).
static bool int_form_applies(const ScoreWs& W, const tdr_map_desc* map, int rf) {
  return W.su && map_has_compact(map, rf) && !map_is_wide(map, rf) && tdr_ray_map_ok(map);
}
bool tdr_score_polar_float_form(const tdr_map_desc* map, int nb, int nr, int64_t n, int64_t n_total) {
  const int rf = tdr_rec_floats(map->ncls);
  return !int_form_applies(score_ws(map->ncls, nb, nr, n, n_total), map, rf);
}
// ---- the argument blocks of a launch, each filled in ONE place -------------------------------------------------------------
// ScoreArgs of a polar launch over `map` with the ring groups of W; the caller adds `part`, `utab` and what is special to it.
static ScoreArgs make_score_args(const tdr_map_desc* map, const float* tab, const float* scan_pk, int nb, int nr, float res,
                                 const float* st, int64_t cap, int64_t n, const int32_t* order, const ScoreWs& W) {
  ScoreArgs a;
  a.rec = map->rec; a.rows = map->rows; a.cols = map->cols; a.resolution = map->resolution;
  a.tab = tab; a.scan_pk = scan_pk; a.nb = nb; a.nr = nr; a.res = res;
  a.st = st; a.cap = cap; a.n = n; a.order = order;
  a.group = W.group; a.nchunks = W.nchunks; a.npad = W.npad;
  a.part = nullptr;
  return a;
}
// FinalizeArgs that turn the float partial sums [nchunks][rf + 1][npad] at `part` into raw weights (mode 0), with the
// polar gates; P: samples of a window.
static FinalizeArgs make_finalize_args(const tdr_map_desc* map, const tdr_filter_params* fp, const float* part, int nchunks,
                                       int64_t npad, int64_t P, float* st, int64_t cap, int64_t n, const int32_t* order,
                                       float* raw_w) {
  FinalizeArgs f;
  f.part = part; f.rf = map->rec_floats; f.nchunks = nchunks; f.npad = npad; f.n = n; f.cap = cap;
  f.order = order; f.st = st; f.fp = *fp;
  f.gate = make_gate(fp, map);
  f.P = P; f.ncls = map->ncls; f.raw_w = raw_w;
  return f;
}
// score_finalize_exact_kernel over the integer sums an integer-form launch left at f.part (slot list, device words {dense
// slots, scattered, both}, the int_form_off words); f then finalizes only what the float kernel had to score
static void launch_finalize_exact(FinalizeArgs& f, const tdr_map_desc* map, int64_t npad, const int32_t* slots,
                                  const int32_t* counts, const int32_t* inexact, hipStream_t s) {
  FinalizeArgs fx = f;
  fx.npad = npad; fx.order = slots; fx.counts = counts; fx.inexact = inexact;
  fx.ipart = reinterpret_cast<const uint32_t*>(f.part);
  fx.dict_tail = reinterpret_cast<const uint32_t*>(map->dict) + 2 * TDR_CMAP_MAX_DICT;
  hipLaunchKernelGGL(score_finalize_exact_kernel, dim3((unsigned)cdiv(npad, 256)), dim3(256), 0, s, fx);
  f.run_if = inexact;
}

// ---- batched filters (tdr_batch_step, tdr_batch.h): the float form of k filters' scoring launches as ONE grid ----------
// Per filter exactly the ScoreArgs / FinalizeArgs tdr_k_score_polar_ctx builds for its float launch (same workspace
// layout, ring groups from its own particle count, its own scan, res and sample offsets); the grid's x blocks are the
// filters' particle blocks side by side, grid.y the largest chunk count.  No locality order (results never depend on it).
namespace {
struct BatchScoreHdr {
  int32_t blocks, max_chunks, fin_blocks, n_uscale;
  int32_t k_init;   // filters whose 40-rotation search runs in this launch (their tables: behind the scoring tables)
  size_t lds;
};
struct UtabEntry {
  float scale, res;
  float* out;   // NULL: the filter reads each particle's own scale
};
struct BatchScoreLayout {
  size_t args, fargs, blk, fblk, utab, total;
};
BatchScoreLayout batch_layout(int k) {
  auto up = [](size_t x) { return (x + 63) / 64 * 64; };
  BatchScoreLayout L;
  L.args = up(sizeof(BatchScoreHdr));
  L.fargs = L.args + up(sizeof(ScoreArgs) * k);
  L.blk = L.fargs + up(sizeof(FinalizeArgs) * k);
  L.fblk = L.blk + up(sizeof(int32_t) * k);
  L.utab = L.fblk + up(sizeof(int32_t) * k);
  L.total = L.utab + up(sizeof(UtabEntry) * k);
  return L;
}
}  // namespace
__global__ void utab_batch_kernel(const float* __restrict__ tab, int64_t n2, const UtabEntry* __restrict__ ut) {
  const UtabEntry e = ut[blockIdx.y];
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e.out && k < n2) e.out[k] = (tab[k] * e.scale) * e.res;  // utab_kernel's expression
}
size_t tdr_batch_score_stage_bytes(int k, int k_init) {
  return k < 1 ? 0 : batch_layout(k).total + tdr_batch_init_stage_bytes(k_init);
}
int tdr_batch_score_build(const tdr_map_desc* map, const float* tab, int nb, int nr, int k, const TdrBatchScoreIn* in,
                          void* host_stage) {
  if (!map || !tab || !in || !host_stage || k < 1 || nb < 1 || nr < 1) return fail(TDR_ERR_ARG, "batch_score: bad arguments");
  const int rf = tdr_rec_floats(map->ncls);
  if (map->rec_floats != rf) return fail(TDR_ERR_ARG, "batch_score: map record size %d != %d", map->rec_floats, rf);
  if ((size_t)2 * nb * rf * 4 > 64 * 1024) return fail(TDR_ERR_ARG, "batch_score: nb too large for the LDS scan ring");
  if (int rc0 = check_map_addressing(map, rf, "batch_score")) return rc0;
  const BatchScoreLayout Lo = batch_layout(k);
  char* base = static_cast<char*>(host_stage);
  BatchScoreHdr& h = *reinterpret_cast<BatchScoreHdr*>(base);
  ScoreArgs* args = reinterpret_cast<ScoreArgs*>(base + Lo.args);
  FinalizeArgs* fargs = reinterpret_cast<FinalizeArgs*>(base + Lo.fargs);
  int32_t* blk = reinterpret_cast<int32_t*>(base + Lo.blk);
  int32_t* fblk = reinterpret_cast<int32_t*>(base + Lo.fblk);
  UtabEntry* ut = reinterpret_cast<UtabEntry*>(base + Lo.utab);
  h = BatchScoreHdr{};
  std::vector<TdrBatchInitIn> iin;
  for (int i = 0; i < k; i++) {
    const TdrBatchScoreIn& x = in[i];
    if (x.n < 1 || x.cap < x.n || !x.fp || x.fp->num_classes != map->ncls) return fail(TDR_ERR_ARG, "batch_score: filter %d", i);
    const ScoreWs W = score_ws(map->ncls, nb, nr, x.n, x.n);
    if (int_form_applies(W, map, rf)) return fail(TDR_ERR_ARG, "batch_score: filter %d takes the integer form", i);
    ScoreArgs a = make_score_args(map, tab, x.scan_pk, nb, nr, x.res, x.st, x.cap, x.n, nullptr, W);
    a.part = x.ws;
    a.utab = x.uniform_scale > 0.f ? x.ws + W.off_utab : nullptr;   // fill_utab's place
    ut[i] = UtabEntry{x.uniform_scale, x.res, const_cast<float*>(a.utab)};
    set_compact(a, map, rf);
    args[i] = a;
    h.lds = std::max(h.lds, polar_lds_bytes(nb, a.group, rf));
    blk[i] = h.blocks;
    h.blocks += (int32_t)cdiv(x.n, 256);
    h.max_chunks = std::max(h.max_chunks, a.nchunks);
    h.n_uscale += a.utab ? 1 : 0;
    FinalizeArgs f = make_finalize_args(map, x.fp, a.part, a.nchunks, a.npad, (int64_t)nb * nr, x.st, x.cap, x.n, nullptr, x.raw_w);
    f.tlog = finalize_tlog(f.nchunks, x.n);
    fargs[i] = f;
    fblk[i] = h.fin_blocks;
    h.fin_blocks += (int32_t)cdiv(x.n << f.tlog, 256);
    // res_flag / res_theta and the rotation table where tdr_k_score_polar_ctx puts them
    if (x.init_search) iin.push_back(TdrBatchInitIn{x.scan_pk, x.res, x.fp, x.st, x.cap, x.n, a.utab, x.ws + W.off_aux, a.npad, x.raw_w});
  }
  h.k_init = (int32_t)iin.size();
  if (h.k_init > 0) return tdr_batch_init_build(map, tab, nb, nr, h.k_init, iin.data(), base + Lo.total);
  return TDR_OK;
}
int tdr_batch_score_launch(const tdr_map_desc* map, const float* tab, int nb, int nr, int k, const void* host_stage,
                           const void* dev_stage, hipStream_t s) {
  if (!map || !tab || !host_stage || !dev_stage || k < 1) return fail(TDR_ERR_ARG, "batch_score: bad arguments");
  const BatchScoreLayout Lo = batch_layout(k);
  const BatchScoreHdr& h = *static_cast<const BatchScoreHdr*>(host_stage);
  const char* d = static_cast<const char*>(dev_stage);
  const ScoreArgs* args = reinterpret_cast<const ScoreArgs*>(d + Lo.args);
  const FinalizeArgs* fargs = reinterpret_cast<const FinalizeArgs*>(d + Lo.fargs);
  const int32_t* blk = reinterpret_cast<const int32_t*>(d + Lo.blk);
  const int32_t* fblk = reinterpret_cast<const int32_t*>(d + Lo.fblk);
  const UtabEntry* ut = reinterpret_cast<const UtabEntry*>(d + Lo.utab);
  const int rf = tdr_rec_floats(map->ncls);
  if (h.n_uscale > 0) {
    const int64_t n2 = 2 * (int64_t)nb * nr;
    hipLaunchKernelGGL(utab_batch_kernel, dim3((unsigned)cdiv(n2, 256), (unsigned)k), dim3(256), 0, s, tab, n2, ut);
    LAUNCH_CHECK("batch_utab");
  }
  // state_particle.cpp:195-206 first, as in tdr_k_score_polar_ctx: the regular pass below then scores every particle at its
  // (possibly just chosen) rotation
  if (h.k_init > 0)
    if (int rc = tdr_batch_init_launch(map, nb, nr, static_cast<const char*>(host_stage) + Lo.total, d + Lo.total, s)) return rc;
  const dim3 grid((unsigned)h.blocks, (unsigned)h.max_chunks);
  for (int us = 1; us >= 0; us--) {   // the filters with a uniform-scale table, then the others: one instantiation each
    if (us ? h.n_uscale == 0 : h.n_uscale == k) continue;
    if (int rc = with_polar_kernel<1>(map, rf, us != 0, "batch_score", [&](auto kfn) {
          allow_lds(kfn, h.lds);
          hipLaunchKernelGGL(kfn, grid, dim3(256), h.lds, s, args, blk, k);
          return TDR_OK;
        }))
      return rc;
  }
  LAUNCH_CHECK("batch_score_polar");
  hipLaunchKernelGGL(score_finalize_batch_kernel, dim3((unsigned)h.fin_blocks), dim3(256), 0, s, fargs, fblk, k);
  LAUNCH_CHECK("batch_score_finalize");
  if (h.k_init > 0) return tdr_batch_init_fixup(static_cast<const char*>(host_stage) + Lo.total, d + Lo.total, s);
  return TDR_OK;
}
// SuLaunch of an integer-form call with the ScoreArgs `a` (a.utab: where the uniform-scale table is or will be) on `workspace`;
// the caller adds the span
static SuLaunch make_su_launch(const tdr_map_desc* map, const ScoreArgs& a, int rf, float uniform_scale, const tdr_score_ctx* ctx,
                               const ScoreWs& W, float* workspace) {
  const int nb = a.nb, nr = a.nr;
  SuLaunch L;
  L.map = map; L.tab = a.utab ? a.utab : a.tab; L.uniform_scale = a.utab != nullptr; L.scan_pk = a.scan_pk;
  L.tab_src = a.tab; L.utab_out = const_cast<float*>(a.utab);
  L.nb = nb; L.nr = nr; L.rf = rf; L.res = a.res; L.st = a.st; L.cap = a.cap; L.n = a.n; L.perm = a.order;
  L.group = W.su_group; L.nchunks = W.su_nchunks; L.npad = W.npad_part; L.part = a.part;
  L.tail_k = W.su_tail_k; L.tail_q = W.su_tail_q; L.rows = W.su_rows;
  L.fac = ctx && ctx->fac && ctx->fac_nb == nb && ctx->fac_nr == nr ? ctx->fac : nullptr;
  L.uscale = uniform_scale;
  L.ray_split = tdr_ray_splits(nb, nr, a.n, tdr_cfg().ray_block_major && L.fac != nullptr);
  L.ws = workspace ? reinterpret_cast<int32_t*>(workspace + W.off_su) : nullptr;   // (NULL: tdr_k_score_prep asking for the shapes)
  L.span = tdr_cfg().su_span;
  return L;
}
// The ordering passes and the scan-side preparation of an integer-form call on their own (include/tdr.h)
extern "C" int tdr_k_score_prep(const tdr_map_desc* map, const float* tab, const float* scan_pk, int nb, int nr, float res,
                                const float* st, int64_t cap, int64_t n, int64_t n_total, const int32_t* perm,
                                float uniform_scale, float span, float* workspace, tdr_score_ctx* ctx, int64_t* layout,
                                void* const* out, void* stream) {
  if (!map || !map->rec || !layout) return fail(TDR_ERR_ARG, "score_prep: null pointer");
  if (n_total <= 0) n_total = n;
  if (n < 1 || cap < n || nb < 1 || nr < 1) return fail(TDR_ERR_ARG, "score_prep: bad shape");
  if (map->ncls < 1 || map->ncls > TDR_MAX_CLASSES) return fail(TDR_ERR_ARG, "score_prep: bad class count");
  const int rf = tdr_rec_floats(map->ncls);
  if (map->rec_floats != rf) return fail(TDR_ERR_ARG, "score_prep: map record size %d != %d", map->rec_floats, rf);
  const ScoreWs W = score_ws(map->ncls, nb, nr, n, n_total);
  if (!int_form_applies(W, map, rf)) return fail(TDR_ERR_ARG, "score_prep: the call has no integer form");
  ScoreArgs a = make_score_args(map, tab, scan_pk, nb, nr, res, st, cap, n, perm, W);
  a.part = workspace;
  a.utab = uniform_scale > 0.f && workspace ? workspace + W.off_utab : nullptr;
  SuLaunch L = make_su_launch(map, a, rf, uniform_scale, ctx, W, workspace);
  L.uniform_scale = uniform_scale > 0.f;
  L.span = span;
  L.part = nullptr;   // no scoring kernel behind this preparation: no sums to zero
  hipStream_t s = (hipStream_t)stream;
  if (!workspace) {   // the shapes alone
    return tdr_su_prep_copy_out(L, W.suw, s, layout, nullptr);
  }
  if (!tab || !scan_pk || !st || !out) return fail(TDR_ERR_ARG, "score_prep: null pointer");
  const int32_t* slots = nullptr;
  const int32_t* counts = nullptr;
  if (int rc = tdr_su_prepare(L, W.suw, s, &slots, &counts)) return rc;
  return tdr_su_prep_copy_out(L, W.suw, s, layout, out);
}
// The preparation's mask of the bins with several classes (include/tdr.h), out of the workspace a call of these shapes used
extern "C" int tdr_k_score_prep_full_mask(const tdr_map_desc* map, int nb, int nr, int64_t n, int64_t n_total,
                                          const float* workspace, uint32_t* out, int64_t* words, void* stream) {
  if (!map || !words) return fail(TDR_ERR_ARG, "score_prep_full_mask: null pointer");
  if (n_total <= 0) n_total = n;
  if (n < 1 || nb < 1 || nr < 1 || map->ncls < 1 || map->ncls > TDR_MAX_CLASSES) return fail(TDR_ERR_ARG, "score_prep_full_mask: bad shape");
  const ScoreWs W = score_ws(map->ncls, nb, nr, n, n_total);
  if (!int_form_applies(W, map, tdr_rec_floats(map->ncls))) return fail(TDR_ERR_ARG, "score_prep_full_mask: the call has no integer form");
  *words = (int64_t)W.su_nchunks * 2 * nb;
  if (!workspace || !out) return TDR_OK;
  HIP_TRY(hipMemcpyAsync(out, reinterpret_cast<const int32_t*>(workspace + W.off_su) + W.suw.full_mask, sizeof(uint32_t) * (size_t)*words,
                         hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return TDR_OK;
}
extern "C" int tdr_k_score_polar(const tdr_map_desc* map, const float* tab, const float* scan_pk, int nb, int nr,
                                 float res, const tdr_filter_params* fp, float* st, int64_t cap, int64_t n,
                                 int64_t n_total, const int32_t* perm, float uniform_scale, int init_search,
                                 float* raw_w, float* workspace, void* stream) {
  return tdr_k_score_polar_ctx(map, tab, scan_pk, nb, nr, res, fp, st, cap, n, n_total, perm, uniform_scale, init_search,
                               raw_w, workspace, nullptr, stream);
}
extern "C" int tdr_k_score_polar_ctx(const tdr_map_desc* map, const float* tab, const float* scan_pk, int nb, int nr,
                                     float res, const tdr_filter_params* fp, float* st, int64_t cap, int64_t n,
                                     int64_t n_total, const int32_t* perm, float uniform_scale, int init_search,
                                     float* raw_w, float* workspace, tdr_score_ctx* ctx, void* stream) {
  if (!map || !map->rec || !tab || !scan_pk || !fp || !st || !raw_w || !workspace)
    return fail(TDR_ERR_ARG, "score: null pointer");
  if (n_total <= 0) n_total = n;
  if (n < 0 || cap < n) return fail(TDR_ERR_ARG, "score: n=%lld exceeds capacity %lld", (long long)n, (long long)cap);
  if (n == 0) return TDR_OK;
  if (nb < 1 || nr < 1) return fail(TDR_ERR_ARG, "score: bad image shape");
  if (map->ncls < 1 || map->ncls > TDR_MAX_CLASSES || fp->num_classes != map->ncls)
    return fail(TDR_ERR_ARG, "score: class count mismatch (map %d, params %d)", map->ncls, fp->num_classes);
  const int rf = tdr_rec_floats(map->ncls);
  if (map->rec_floats != rf) return fail(TDR_ERR_ARG, "score: map record size %d != %d", map->rec_floats, rf);
  if ((size_t)2 * nb * rf * 4 > 64 * 1024) return fail(TDR_ERR_ARG, "score: nb too large for the LDS scan ring");
  if (!(map->resolution > 0.f)) return fail(TDR_ERR_ARG, "score: map resolution must be > 0");
  if (int rc0 = check_map_addressing(map, rf, "score")) return rc0;
  hipStream_t s = (hipStream_t)stream;

  const ScoreWs W = score_ws(map->ncls, nb, nr, n, n_total);
  ScoreArgs a = make_score_args(map, tab, scan_pk, nb, nr, res, st, cap, n, perm, W);
  a.part = workspace;
  // the uniform-scale table: a launch of its own for the float form and in front of the init search; an integer-form call
  // leaves it to its preparation kernel (tdr_su_prepare), which writes the same words
  const bool int_form = int_form_applies(W, map, rf);
  if (int_form && (reinterpret_cast<uintptr_t>(workspace) & 7) != 0)   // the 64-bit class sums at its head (int_add_sums)
    return fail(TDR_ERR_ARG, "score: the workspace must be 8-byte aligned");
  int rc = TDR_OK;
  if (int_form && !init_search) {
    a.utab = uniform_scale > 0.f ? workspace + W.off_utab : nullptr;
  } else if ((rc = fill_utab(a, workspace, W, uniform_scale, s))) {
    return rc;
  }
  float* res_flag = workspace + W.off_aux;   // npad floats; behind them res_theta (npad) and the search's rotation table
  // state_particle.cpp:195-206 first: it fixes theta / have_init of the un-initialised particles, the regular pass
  // below then scores every particle at its (possibly just chosen) rotation
  if (init_search)
    if ((rc = tdr_score_init_search(map, a.tab, a.utab, scan_pk, nb, nr, res, fp, st, cap, n, n_total, perm, res_flag, a.npad, s)))
      return rc;
  FinalizeArgs f = make_finalize_args(map, fp, a.part, a.nchunks, a.npad, (int64_t)nb * nr, st, cap, n, perm, raw_w);
  if (int_form) {
    // The INTEGER form of the launch (tdr_score_su.h): dense particles by heading bin through the shift-uniform kernel,
    // scattered ones — behind the bins in the same slot list — one wave each through the ray-mapped kernel; both form exact
    // integer sums, so a particle's weight does not depend on which of the two scored it.  A scan or a map without
    // an integer form (fractional or non-finite counts; a dictionary finer than 2^-q) raises the device word `inexact`:
    // the integer kernels then return at once and the float kernel below does the launch — nothing is decided on the host.
    const int32_t* slots = nullptr;
    const int32_t* counts = nullptr;   // device words {slots of the dense share, scattered particles behind them, both}
    SuLaunch L = make_su_launch(map, a, rf, uniform_scale, ctx, W, workspace);
    TunerScope tuner_scope(ctx, s);   // (closes the tuner's measurement on every way out)
    L.span = tdr_su_span_begin(ctx ? &ctx->tuner : nullptr,
                               ((int64_t)n << 24) ^ ((int64_t)nb << 12) ^ nr ^ ((int64_t)map->rows << 40), s);
    if ((rc = tdr_su_prepare(L, W.suw, s, &slots, &counts))) return rc;
    const int32_t* inexact = counts + 4;
    {
      ScoreProfScope prof(s);
      {
        ShareProfScope sp(0, s, true);
        if ((rc = tdr_ray_score(L, W.suw, s))) return rc;
      }
      {
        ShareProfScope sp(1, s, true);
        if ((rc = tdr_su_score(L, W.suw, s))) return rc;
      }
      if (g_prof_on) { g_share_valid = true; g_share_counts = counts; }
      // the float form, for the launches the integer form does not cover
      ScoreArgs r = a;
      r.run_if = inexact;
      if ((rc = launch_score(r, map, rf, s, false))) return rc;
    }
    launch_finalize_exact(f, map, W.npad_part, slots, counts, inexact, s);
    LAUNCH_CHECK("score_finalize_exact");
    launch_finalize(f, n, s, true);
  } else {
    if ((rc = launch_score(a, map, rf, s))) return rc;
    launch_finalize(f, n, s);
  }
  LAUNCH_CHECK("score_finalize");
  if (init_search) return tdr_score_init_fixup(res_flag, n, fp->regularization, raw_w, s);
  return TDR_OK;
}

// ---- scoring WITH the geometric term -------------------------------------------------------------------
// getCostForRot's geometric block — cost += (top_down_geo[i] . shifted geo_cls[i]).sum() * 0.01 for the two layers,
// normalization += top_down_geo[i].sum() — is commented out in the reference (src/state_particle.cpp:145-152) and its
// inputs are zero images there (src/top_down_render.cpp:533-540).  It is available here as an opt-in: a second scoring
// launch over the 2-layer geometric map (tdr_k_geo_map_from_map) against the packed geometric scan, combined in the
// finalize step.  The 40-rotation search then has to price the geometric term for every candidate too: it runs as one
// scoring pass per rotation over the workgroups that hold a particle without a heading (the window-gathered-once
// kernels only know the semantic term).
__global__ void init_from_best_kernel(const float* __restrict__ best_cost, const float* __restrict__ best_theta,
                                      const int32_t* __restrict__ order, int64_t n, float* __restrict__ st, int64_t cap,
                                      GateArgs gate, float* __restrict__ res_flag) {
  const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n) return;
  const int64_t p = order ? (int64_t)order[slot] : slot;
  res_flag[p] = 0.f;
  if (st[TDR_ST_HAVE_INIT * cap + p] != 0.f) return;
  const float scale = st[TDR_ST_SCALE * cap + p];
  const float cx = st[TDR_ST_DX * cap + p] * scale + st[TDR_ST_INIT_X * cap + p];
  const float cy = st[TDR_ST_DY * cap + p] * scale + st[TDR_ST_INIT_Y * cap + p];
  if (particle_gated(gate, cx, cy, scale)) return;          // computeWeight returns before the search (:163-176)
  const bool none = !(best_cost[slot] < 3.402823466e+38f);  // every candidate scored NaN: best_theta stays 0 (:193-194)
  st[TDR_ST_THETA * cap + p] = none ? 0.f : best_theta[slot];   // :205
  st[TDR_ST_HAVE_INIT * cap + p] = 1.f;                         // :206
  res_flag[p] = none ? 2.f : 1.f;
}
extern "C" size_t tdr_score_geo_workspace_floats(int ncls, int nb, int nr, int64_t n, int64_t n_total) {
  const int64_t npad = cdiv(std::max<int64_t>(n, 1), 64) * 64;
  const int ggroup = score_group_rings(nb, nr, 4, n_total > 0 ? n_total : n);
  return tdr_score_workspace_floats(ncls, nb, nr, n, n_total) + (size_t)(cdiv(nr, ggroup) * 5 * npad);
}
extern "C" int tdr_k_score_polar_geo(const tdr_map_desc* map, const tdr_map_desc* geo_map, const float* tab,
                                     const float* scan_pk, const float* geo_pk, float geo_sum0, float geo_sum1, int nb,
                                     int nr, float res, const tdr_filter_params* fp, float* st, int64_t cap, int64_t n,
                                     int64_t n_total, const int32_t* perm, float uniform_scale, int init_search,
                                     float* raw_w, float* workspace, void* stream) {
  if (!map || !map->rec || !geo_map || !geo_map->rec || !tab || !scan_pk || !geo_pk || !fp || !st || !raw_w || !workspace)
    return fail(TDR_ERR_ARG, "score_geo: null pointer");
  if (n < 0 || cap < n) return fail(TDR_ERR_ARG, "score_geo: n exceeds capacity");
  if (n == 0) return TDR_OK;
  if (n_total <= 0) n_total = n;
  if (nb < 1 || nr < 1) return fail(TDR_ERR_ARG, "score_geo: bad image shape");
  if (map->ncls < 1 || map->ncls > TDR_MAX_CLASSES || fp->num_classes != map->ncls)
    return fail(TDR_ERR_ARG, "score_geo: class count mismatch");
  if (geo_map->ncls != 2 || geo_map->rec_floats != 4 || geo_map->rows != map->rows || geo_map->cols != map->cols)
    return fail(TDR_ERR_ARG, "score_geo: the geometric map must be the 2-layer map of the same grid");
  const int rf = tdr_rec_floats(map->ncls);
  if (map->rec_floats != rf) return fail(TDR_ERR_ARG, "score_geo: map record size mismatch");
  if ((size_t)nb * rf * 4 > 60 * 1024) return fail(TDR_ERR_ARG, "score_geo: nb too large for the LDS scan ring");
  if (int rc0 = check_map_addressing(map, rf, "score_geo")) return rc0;
  hipStream_t s = (hipStream_t)stream;
  const ScoreWs W = score_ws(map->ncls, nb, nr, n, n_total);
  ScoreArgs a = make_score_args(map, tab, scan_pk, nb, nr, res, st, cap, n, perm, W);
  a.part = workspace;
  int rc = fill_utab(a, workspace, W, uniform_scale, s);
  if (rc) return rc;
  float* best_cost = workspace + W.off_aux;                               // npad floats (res_flag's place)
  float* best_theta = best_cost + a.npad;                                 // npad floats
  float* res_flag = best_theta + a.npad;                                  // npad floats ("list" region)
  ScoreArgs g = a;   // the geometric launch: same particles, same table, the 2-layer map and scan
  g.rec = geo_map->rec; g.scan_pk = geo_pk;
  g.group = score_group_rings(nb, nr, 4, n_total);
  g.nchunks = (int)cdiv(nr, g.group);
  g.part = workspace + tdr_score_workspace_floats(map->ncls, nb, nr, n, n_total);
  FinalizeArgs f = make_finalize_args(map, fp, a.part, a.nchunks, a.npad, (int64_t)nb * nr, st, cap, n, perm, raw_w);
  f.best_cost = best_cost; f.best_theta = best_theta;
  f.gpart = g.part; f.gnchunks = g.nchunks; f.gsum0 = geo_sum0; f.gsum1 = geo_sum1;
  const dim3 fgrid((unsigned)cdiv(n, 256)), fblock(256);
  if (init_search) {
    // state_particle.cpp:195-206 with the geometric term: one pass per candidate rotation, workgroups without an
    // un-initialised particle return at once
    a.only_uninit = g.only_uninit = 1;
    a.use_theta_override = g.use_theta_override = 1;
    f.mode = 1; f.only_uninit = 1;
    int k = 0;
    for (float t = 0; t < 2 * M_PI; t += 2 * M_PI / 40) {   // :197 (float t, double increment)
      a.theta_override = g.theta_override = t;
      if ((rc = launch_score(a, map, rf, s))) return rc;
      if ((rc = launch_score(g, geo_map, 4, s))) return rc;
      f.first = k == 0; f.theta_override = t;
      launch_finalize(f, n, s);
      LAUNCH_CHECK("score_finalize(geo init)");
      k++;
    }
    hipLaunchKernelGGL(init_from_best_kernel, fgrid, fblock, 0, s, (const float*)best_cost, (const float*)best_theta, perm,
                       n, st, cap, f.gate, res_flag);
    LAUNCH_CHECK("init_from_best");
    a.only_uninit = g.only_uninit = 0;
    a.use_theta_override = g.use_theta_override = 0;
  }
  if ((rc = launch_score(a, map, rf, s))) return rc;
  if ((rc = launch_score(g, geo_map, 4, s))) return rc;
  f.mode = 0; f.first = 0; f.theta_override = 0.f; f.only_uninit = 0;
  launch_finalize(f, n, s);
  LAUNCH_CHECK("score_finalize(geo)");
  if (init_search) return tdr_score_init_fixup(res_flag, n, fp->regularization, raw_w, s);
  return TDR_OK;
}

static int64_t cart_part_floats(int ncls, int cols, int64_t n, int64_t n_total) {   // partial sums, 256-byte aligned
  int cpc, nchunks;
  choose_chunks(n_total > 0 ? n_total : n, cols, cpc, nchunks, TDR_CART_WAVE_MUL);
  // (the integer form's slot list pads the dense share to whole waves, its rows are words: 2 per class + 2, and a scattered
  // particle's window may be split over up to TDR_RAY_MAX_SPLIT chunk rows)
  const int64_t npad = su_npad(std::max<int64_t>(n, 1), 1);
  const int rowsmax = std::max(tdr_rec_floats(ncls) + 1, 2 * ncls + 2);
  return cdiv((int64_t)std::max(nchunks, TDR_RAY_MAX_SPLIT) * rowsmax * npad + 64, 64) * 64;
}
extern "C" size_t tdr_score_cart_workspace_floats(int ncls, int rows, int cols, int64_t n, int64_t n_total) {
  // partial sums + the float form's scan descriptors + the integer form's tables and ordering workspace
  return (size_t)(cart_part_floats(ncls, cols, n, n_total) + tdr_cart_desc_words(rows, cols) +
                  tdr_cart_int_words(rows, cols, std::max<int64_t>(n, 1)));
}

extern "C" int tdr_k_score_cart(const tdr_map_desc* map, const float* scan_pk, int rows, int cols, float res,
                                const tdr_filter_params* fp, float* st, int64_t cap, int64_t n, int64_t n_total,
                                const int32_t* perm, float* raw_w, float* workspace, void* stream) {
  if (!map || !map->rec || !scan_pk || !fp || !st || !raw_w || !workspace)
    return fail(TDR_ERR_ARG, "score_cart: null pointer");
  if (n_total <= 0) n_total = n;
  if (n < 0 || cap < n) return fail(TDR_ERR_ARG, "score_cart: n exceeds capacity");
  if (n == 0) return TDR_OK;
  if (rows < 1 || cols < 1) return fail(TDR_ERR_ARG, "score_cart: bad window shape");
  if (fp->num_classes != map->ncls) return fail(TDR_ERR_ARG, "score_cart: class count mismatch");
  const int rf = tdr_rec_floats(map->ncls);
  if (map->rec_floats != rf) return fail(TDR_ERR_ARG, "score_cart: map record size mismatch");
  if (int rc0 = check_map_addressing(map, rf, "score_cart")) return rc0;
  hipStream_t s = (hipStream_t)stream;
  CartArgs a;
  a.rec = map->rec; a.map_rows = map->rows; a.map_cols = map->cols; a.resolution = map->resolution;
  a.scan_pk = scan_pk; a.rows = rows; a.cols = cols; a.res = res;
  a.st = st; a.cap = cap; a.n = n; a.order = perm;
  // chunks of window columns from the filter's TOTAL particle count (the same on every rank of a sharded filter, like
  // score_group_rings): a particle's partial sums are then the same in an N-rank run as in the 1-rank run
  choose_chunks(n_total, cols, a.cpc, a.nchunks, TDR_CART_WAVE_MUL);
  a.npad = cdiv(n, 64) * 64;
  a.part = workspace;
  a.libm_fma = tdr_libm_fma();
  dim3 grid((unsigned)cdiv(n, 256), (unsigned)a.nchunks), block(256);
  const bool ks = tdr_has_kslot(map->ncls, rf);
  const bool cm = set_compact(a, map, rf), wide = cm && map_is_wide(map, rf);
  CartIntOut io{};
  bool int_form = false;
  if (cm && !wide && tdr_cart_skip_ok(map, rf)) {
    ScoreProfScope prof(s);
    uint32_t* desc_ws = reinterpret_cast<uint32_t*>(workspace + cart_part_floats(map->ncls, cols, n, n_total));
    if (tdr_cart_int_ok(map, rf, rows, cols, n_total)) {
      // the integer form: dense particles through the skipping kernel with integer accumulators, scattered ones one wave
      // each through score_cart_ray_kernel; the float skipping kernel behind them for what has no integer form
      int32_t* iws = reinterpret_cast<int32_t*>(desc_ws + tdr_cart_desc_words(rows, cols));
      if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0)   // the 64-bit class sums at its head (int_add_sums)
        return fail(TDR_ERR_ARG, "score_cart: the workspace must be 8-byte aligned");
      // (which particles count as dense: four times the polar launch's span — a Cartesian window is a rotated rectangle of
      // rows x cols cells and neighbours a few dozen cells apart still share most of their lines; measured on config 4, ms per
      // step at 8 / 16 / 32 / 64 cells: 32.6 / 29.2 / 28.8 / 28.5, the float kernel 36.9)
      if (int rc = tdr_cart_int_launch(a, map, rf, desc_ws, iws, 4.f * tdr_cfg().su_span, s, &io)) return rc;
      int_form = true;
    } else if (int rc = tdr_cart_skip_launch(a, map, rf, desc_ws, s)) return rc;
  } else {
    ScoreProfScope prof(s);
    if (int rc = with_nv4(rf, "score_cart", [&](auto N) {
          return with_flags([&](auto KS, auto CM, auto WD) {
            constexpr int NV4 = decltype(N)::value;
            constexpr bool c = decltype(CM)::value, w = decltype(WD)::value;   // compact: up to 12 floats; wide: 8 only
            if constexpr ((c && NV4 == 4) || (w && !(c && NV4 == 2))) return fail(TDR_ERR_ARG, "score_cart: no kernel for this record form");
            else hipLaunchKernelGGL((score_cart_kernel<NV4, TDR_SCORE_U, decltype(KS)::value, c, w>), grid, block, 0, s, a);
            return TDR_OK;
          }, ks, cm, wide);
        }))
      return rc;
  }
  LAUNCH_CHECK("score_cart");
  FinalizeArgs f = make_finalize_args(map, fp, a.part, a.nchunks, a.npad, (int64_t)rows * cols, st, cap, n, perm, raw_w);
  f.gate.force_on_map = 0;   // the Cartesian definition has no gates (include/tdr.h)
  f.gate.scale_unknown = 0;
  if (int_form) launch_finalize_exact(f, map, io.npad, io.slots, io.counts, io.flags, s);
  launch_finalize(f, n, s);
  LAUNCH_CHECK("score_finalize(cart)");
  return TDR_OK;
}

// Self-test hook: the scoring loop's coordinate rounding applied to caller-supplied floats (clamped to [-1, limit]
// like the loop does), so the GPU tests can compare it with roundf over whole float ranges.
__global__ void selftest_round_kernel(const float* __restrict__ x, int64_t n, float limit, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = round_half_away_clamped(__builtin_amdgcn_fmed3f(x[i], -1.f, limit));
}
extern "C" int tdr_k_selftest_round(const float* x, int64_t n, float limit, int32_t* out, void* stream) {
  if (!x || !out || n < 1) return fail(TDR_ERR_ARG, "selftest_round: bad arguments");
  hipLaunchKernelGGL(selftest_round_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, n, limit,
                     out);
  LAUNCH_CHECK("selftest_round");
  return TDR_OK;
}
