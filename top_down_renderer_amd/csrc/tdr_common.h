// tdr_common.h — shared by the HIP translation units of libtdr_hip.so (not installed; the public header is include/tdr.h).
//
// Compile with -ffp-contract=off: every float expression that decides a bin / cell index must round exactly like
// the reference's x86-64 code (no FMA contraction); FMAs are spelled out (__builtin_fmaf) where they are wanted.
//
// Kernel map (reference loop nest -> kernel -> file), see DESIGN.md:
//   K0 pack_map_kernel, ingest_*   class_maps_/class_mask_ (top_down_map.h:77-79), top_down_map.cpp:116-144,289-326  tdr_map.hip
//   K1 raster_keys/raster_kernel   scan_renderer_polar.cpp:93-108 / scan_renderer.cpp:65-77                          tdr_raster.hip
//   K2 score_polar_kernel          top_down_map_polar.cpp:28-52 + state_particle.cpp:132-143 (lane = particle)       tdr_score.hip
//      score_cart_kernel           top_down_map.cpp:429-459 + state_particle.cpp:112-155
//      score_finalize_kernel       state_particle.cpp:117-120,136-139,154,161-176,212
//      score_init(_mfma)_kernel    state_particle.cpp:195-206                                                        tdr_score_init.hip
//   K3 propagate_kernel            state_particle.cpp:57-78                                                          tdr_filter.hip
//   K4 update_weights / uw_pass*   particle_filter.cpp:107-147
//   K5 prefix kernels              particle_filter.cpp:175-183 (the serial float32 running sum, bit-exact)            tdr_prefix.hip
//      resample / gather_states    particle_filter.cpp:172-185                                                       tdr_filter.hip
//   K6 mean_cov / mc_* kernels     particle_filter.cpp:191-236, 343-357
#ifndef TDR_COMMON_H_
#define TDR_COMMON_H_
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <type_traits>
#include <utility>
#include <vector>

#include "tdr.h"
#include "tdr_config.h"
#include "tdr_internal.h"   // the cross-file prototypes no subsystem header holds

// tuning knobs (compile-time)
#ifndef TDR_SCORE_U
#define TDR_SCORE_U 4          // samples whose loads are kept in flight together in the scoring loop
#endif
#ifndef TDR_XCD_SWIZZLE
#define TDR_XCD_SWIZZLE 0
#endif
#ifndef TDR_OOB_ALIAS
#define TDR_OOB_ALIAS 1      // all out-of-bounds samples read one guard record (A/B on MI355X: -11 % on config 2)
#endif

// error plumbing (tdr_core.hip): the message behind tdr_last_error(), per host thread
int tdr_fail(int code, const char* fmt, ...);
#define fail tdr_fail
#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(TDR_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define LAUNCH_CHECK(name)                                                                   \
  do {                                                                                       \
    hipError_t e_ = hipGetLastError();                                                       \
    if (e_ != hipSuccess) return fail(TDR_ERR_HIP, "launch %s: %s", name, hipGetErrorString(e_)); \
  } while (0)

// tdr_core.hip: 1 if the device should evaluate sinf / cosf like glibc's FMA-contracted build, 0 like its plain build
// (whichever the host's libm runs; tdr_sincosf.h)
int tdr_libm_fma();

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Run-time flags -> template arguments, the one way every launch does it:
//     with_flags([&](auto KS, auto US) { launch(kernel<decltype(KS)::value, decltype(US)::value>); return TDR_OK; }, ks, us);
// calls f(std::bool_constant<ks>{}, std::bool_constant<us>{}).  Every combination of the flags is instantiated: a
// combination that has no kernel is excluded with `if constexpr` inside f.
template <class F>
static inline int with_flags(F&& f) { return f(); }
template <class F, class... Rest>
static inline int with_flags(F&& f, bool b, Rest... rest) {
  auto next = [&](auto B) { return with_flags([&](auto... bs) { return f(B, bs...); }, rest...); };
  return b ? next(std::true_type{}) : next(std::false_type{});
}
// ... and the record size rf (4, 8, 12 or 16 floats) -> f(std::integral_constant<int, rf / 4>{})
template <class F>
static inline int with_nv4(int rf, const char* who, F&& f) {
  switch (rf / 4) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});   // 8-11 classes
    case 4: return f(std::integral_constant<int, 4>{});   // 12-15 classes (TDR_MAX_CLASSES)
    default: return fail(TDR_ERR_ARG, "%s: unsupported record size %d", who, rf);
  }
}

#define PFX_HEAD 2048      // tdr_prefix.hip: leading elements added one by one: the running sum crosses most of its binades here
// tdr_init.hip: the windows of tdr_k_init_particles are whole tiles
#define INI_TILE 2048                 // stream positions per workgroup of ini_flags_kernel (1024 per parity)
#define INI_MAX_TILES 2048            // ini_tail_kernel holds the tiles' minima in LDS: W <= 2^22
// tdr_prefix.hip: final value of a serial float32 chain over the raw weights (kind 0: sum of the non-NaN weights;
// kind 1: float-accumulated squared deviations of the weights below *mean_dev), see there.  have_sums: the chunk headers in
// `workspace` already hold the double sums of this chain's chunks (tdr_uw_chunk_pass1 / _pass2 left them there).
// grid: the path above 32 768 addends that summarises wave-chunks of 512 over the whole chip; the caller asks tdr_chain_grid(n)
// and needs tdr_chain_workspace_bytes(n, true) of workspace for it, else (n, false): the 4096-chunk walk.  One value of `grid`
// for the passes and the chains of a call.
int tdr_chain_total(const float* raw, const float* mean_dev, int kind, int64_t n, float* total_out, void* workspace,
                    bool have_sums, bool grid, hipStream_t st);
int64_t tdr_chain_workspace_bytes(int64_t n, bool grid);
bool tdr_chain_grid(int64_t n);
// The serial float chains of particle_filter.cpp:108-126 (`sum`, `bottom_stddev`) evaluated exactly by tdr_chain_total land
// here, and the mean between them.
struct UwExact {
  float sum, mean, bsum, pad;
};
// tdr_prefix.hip: the two counting passes of tdr_k_update_weights above 32 768 weights, one workgroup per chain chunk, each
// also leaving the double sum of the NEXT chain's chunks in the headers (chain_sum_body: the pass reads the array anyway).
// pass 1: cnt_valid[c] = the chunk's non-NaN weights, the `sum` chain's chunk sums.
// pass 2: ex->mean = ex->sum / valid (:117), cnt_under[c] = the chunk's weights below it, the `bottom_stddev` chain's sums.
int tdr_uw_chunk_pass1(const float* raw, int64_t n, void* workspace, bool grid, int* cnt_valid, hipStream_t st);
int tdr_uw_chunk_pass2(const float* raw, int64_t n, UwExact* ex, const int* cnt_valid, void* workspace, bool grid,
                       int* cnt_under, hipStream_t st);
// tdr_prefix.hip: particle_filter.cpp:107-147 for n <= 32768 in one launch, both serial chains exact
int tdr_uw_small(const float* raw, const float* last_dist, int64_t n, float* w, float* info, hipStream_t st);
// tdr_rng.hip: the generator's raw stream of `nblocks` state blocks behind `state`, and the state behind *consumed words of it
int tdr_mt_raw_stream(const uint32_t* state, int64_t nblocks, uint32_t* raw, hipStream_t s);
int tdr_mt_advance(const uint32_t* raw, int64_t nblocks, const uint32_t* consumed, uint32_t* state, hipStream_t s);
// a record with a spare slot (ncls + 2 <= rf) carries `known` twice: slot rf-2 pairs with a constant 1 of the scan record
__host__ __device__ inline bool tdr_has_kslot(int ncls, int rf) { return ncls + 2 <= rf; }
// diagnostics: 16 device counters while tdr_profile_enable(1) is in force, else NULL (tdr_score.hip, tdr_profile_variants)
uint32_t* tdr_profile_stats_ptr();
// likewise the four counters of tdr_profile_ray_gate (tdr_score_ray.hip)
uint32_t* tdr_profile_gate_ptr();
// likewise the two counters of tdr_profile_su_list (tdr_score_su.hip)
uint32_t* tdr_profile_su_list_ptr();
#endif  // TDR_COMMON_H_
