// tdr_config.h — the library's behaviour switches: one struct, read through tdr_cfg() (not installed; the public calls that
// set them are in include/tdr.h).
//
// The contract, said once: the switches are PROCESS-WIDE, meant for A/B measurements, tests and debugging, and set by ONE
// configuring thread while no other thread is inside the library — there is no locking.  Results never depend on a switch
// unless its comment says so.  The library reads nothing from the process environment.  The configuring calls
// (tdr_config_*, tdr_config_tuning: tdr_config.cpp, where the range rules are) always act on the process-wide struct.
// Every reader is host code on the thread that makes the library call, at launch time; a launch's own choices travel in its
// launch struct (SuLaunch: span, ray_split, tail K / Q).
#ifndef TDR_CONFIG_H_
#define TDR_CONFIG_H_
#include <cstdint>

struct TdrConfig {
  // ---- the integer form of the polar / Cartesian score (tdr_score_su.hip, tdr_score_ray.hip, tdr_score_cart.hip)
  int su_mode = 1;   // 0 = never, 1 = when it pays (default), 2 = whenever the shapes allow (tests: small filters, heavy padding)
  // map cells the 64 locality neighbours of a "dense" particle may span: fixed (tdr_config_shift_uniform_span), or — the
  // default — tuned while running, starting from this value (tdr_su_span_begin)
  float su_span = 16.f;
  bool su_span_fixed = false;
  int su_group = 0;   // rings per workgroup of the shift-uniform kernel; 0: from the shapes (tdr_score.hip: score_ws)
  // Tail units (tdr_su_tail): the last K ring groups of a launch go as Q short rows each.  Defaults from the sweep K in {0, 1,
  // 2, 3, 4, 8} x Q in {2, 4, 8} x groups of 8 / 16 / 32 rings: 16 rings, K = 4, Q = 4 — the last 64 of config
  // 2's 256 rings go as rows of 16 rings x 2 sectors: config 2 4.47 -> 4.32 ms a step, config 3's shard 5.57 -> 5.40, config
  // 5's 13.87 -> 13.62.  (That sweep priced every row with a pass of the finalize over its partial sums; the sums are added in
  // place since — tdr_score_int_dev.h — and rows are free there: the sweep has not been redone)
  int su_tail_groups = 4, su_tail_parts = 4;
  int su_order_bucket = 1;   // 0: the heading order always through rocPRIM's sort (A/B; su_seg_table_words has the rule)
  int su_full_list = 1;      // 0: the assembly loop hands a step with a several-class bin to the C++ step (A/B, tests; same bits)
  int ray_split = 0;         // waves per scattered particle; 0: chosen per launch (tdr_ray_splits)
  int ray_borrow = 1;        // empty bins borrow a neighbour's class plane for their known bit (score_prep_kernel)
  int ray_patch = 1;         // 0: the ray order also where the patch order applies (tdr_score_ray.hip; A/B, same bits)
  int ray_block_major = 1;   // 0: the first (direction-major) row order everywhere (tdr_score_ray.hip; A/B, same bits)
  int cart_skip = 1;         // 0: the general Cartesian kernel also where the skipping kernel applies (A/B, tests)
  // rows of a segment of score_cart_su_kernel (a multiple of 4; 0: the assembly loop off — A/B: the plain kernel): the smaller
  // the segment, the smaller the box of cells a wave stages and the likelier it holds no unknown cell; the larger, the fewer
  // box computations.  Measured on config 4 (ms per step): see DESIGN.md 5.5
  int cart_seg_rows = 32;
  int64_t cart_init_chunk = 4096;   // listed particles per scoring launch of tdr_k_score_cart_init
  // ---- the float kernels (tdr_score.hip)
  int use_compact = 1;   // the compact records are used whenever the map has them; 0 forces the dense ones (A/B, tests)
  // many short waves beat few long ones (A/B on MI355X, config 2: 16k waves 21.8 ms, 128k 15.2 ms): workgroups of one ring
  // chunk run together, so the concurrently touched part of the map is a thin annulus that L2 can hold, and the slow
  // (scattered) batches no longer leave a long tail
  int64_t score_waves = 131072;
  int score_group = 0;   // rings per workgroup; 0: from the shapes (score_group_rings)
  // ---- the search of a particle without a heading (tdr_score_init.hip) and the particle initialisation (tdr_init.hip)
  int init_mfma = 1;    // 0 = vector-unit search only (A/B and debugging)
  int init_ahead = 1;   // record loads the half-record search keeps in flight per wave (1..3)
  // Rebuilding the half records is one pass over the whole map: it pays from a few thousand particles on (4000^2 cells:
  // 0.35 ms, the price of searching ~2000 particles with 256 x 256 windows on the fly).  Filters below the threshold
  // ignore the scratch — the filter's TOTAL particle count decides (n_total, the same on every rank), so that the ranks of
  // a sharded filter take the kernel the one-rank filter takes and choose the same rotations where candidates tie.
  // INT64_MAX turns the path off (A/B).
  int64_t rec16_min = 8192;
  // 1 = a filter that may hold a particle without a heading joins the batch of tdr_batch_step, its search part of the batch's
  // scoring stage (0, the default: it runs its standalone calls)
  int batch_init_search = 0;
  int init_device = 1;              // 0: tdr_filter_initialize_particles keeps the host loop (A/B, tests)
  int64_t init_window = 1 << 21;    // words of the generator's stream per window of tdr_k_init_particles
  // ---- sensor-resetting recovery (tdr_host_recover.cpp)
  int64_t inject_cand_chunk = 65536;   // candidates per scoring launch of tdr_filter_inject_sensor, in whole slots
  // ---- weight statistics, running sum, generator (tdr_prefix.hip, tdr_rng.hip)
  int pfx_small = 1;      // 0 = without the one-launch kernel (A/B and debugging)
  int pfx_head = 64;      // leading elements the long running sum's walk adds one by one
  int uw_waves = 1;       // 0 = the chains chunk by chunk on the whole workgroup (A/B and debugging)
  int mt_stretches = 1;   // 0: every call's raw stream on one wave (A/B, tests); 1: long calls in stretches (tdr_mt_raw_stream)
};

// The configuration in force for the calling thread: the process-wide struct, or the innermost TdrConfigScope of this thread.
const TdrConfig& tdr_cfg();

// Installs `c` for the current thread until the end of the scope; other threads keep reading the process-wide struct, and
// so do the configuring calls.  Scopes nest.  (tdr_selftest_score passes its kernel variants down this way.)
class TdrConfigScope {
 public:
  explicit TdrConfigScope(const TdrConfig& c);
  ~TdrConfigScope();
  TdrConfigScope(const TdrConfigScope&) = delete;
  TdrConfigScope& operator=(const TdrConfigScope&) = delete;

 private:
  TdrConfig cfg_;
  const TdrConfig* outer_;
};
#endif  // TDR_CONFIG_H_
