// tdr_score_su.h — host interface of the integer polar scoring path: the shift-uniform kernel for dense particles
// (tdr_score_su.hip) and the ray-mapped kernel for scattered ones (tdr_score_ray.hip), used by tdr_score.hip.
#ifndef TDR_SCORE_SU_H_
#define TDR_SCORE_SU_H_
#include "tdr_common.h"

// slots a launch of n particles can need: every non-empty heading bin rounded up to whole waves
static inline int64_t su_npad(int64_t n, int nb) { return cdiv(n + 63 * std::min<int64_t>(nb, n), 64) * 64; }
// whether the path applies to a launch shape (tdr_config_shift_uniform, padding economics, kernel constraints)
bool tdr_su_shape_ok(int nb, int nr, int group, int64_t n_total);
// The path's share of the scoring workspace, in 4-byte words, carved in this order (each part 256-byte aligned):
struct SuWs {
  int64_t tab_su, desc, bbox, keys_in, keys_out, vals_in, vals_out, ints, slots, sort_tmp, ray_tab, ray_desc, ray_multi, ray_rad, total;
  int64_t seg_hist;           // the bucket sort's table [segments][nb + 1] (su_colscan_kernel); empty where the rule of shapes
                              // leaves the order to rocPRIM
  int64_t ray_clist, ray_ctab;   // the compact bin lists of the patch order's sectors and their table (score_prep_kernel)
  int64_t full_mask;          // [groups][2 nb] words: which bins of a (ring group, scan row) hold several classes — what the
                              // shift-uniform kernel's list pass walks (written while tdr_su_full_list(L) holds)
  // ints: [cnt nb + 1][start nb + 1][slot_start nb + 1][counts 3][n_multi][inexact][mass bound][table is not its factors]
  //       [3 spare]  (int_form_off)
};
#define TDR_SU_TAIL_INTS 10       // the words of `ints` behind the three per-key tables
#define TDR_RAY_MAX_SPLIT 8       // waves a particle's window may be split over (tdr_ray_splits)
SuWs tdr_su_ws(int nb, int nr, int group, int64_t n);

// The ROWS of the shift-uniform kernel's grid (grid.y) — the "plan".  A row is a workgroup's share of a window: a ring group
// and a range of its TDR_SU_NSECT sectors of directions.  The first nchunks - k rows are whole ring groups; each of the LAST k
// groups is cut into q rows of 8 / q sectors (q: 1, 2, 4 or 8, anything else rounds down to one of them; k is clamped to
// nchunks).  The grid is handed out x-fastest, so the short rows are the workgroups dispatched last: the launch's run-down,
// when nothing refills a compute unit, lasts a short row's lifetime instead of a whole group's.  Integer sums do not care how
// a window is partitioned and a sector's mask is staged once either way: the rows change no bit of any weight.
// Returns the row count R = (nchunks - k) + k q; for 0 <= row < R also the row's ring group and sectors [s0, s1).
#define TDR_SU_NSECT 8
__host__ __device__ static inline int su_tail_plan(int nchunks, int k, int q, int row, int* group, int* s0, int* s1) {
  const int lq = q >= 8 ? 3 : (q >= 4 ? 2 : (q >= 2 ? 1 : 0));
  const int kk = k < 0 ? 0 : (k > nchunks ? nchunks : k);
  const int head = nchunks - kk, rows = head + (kk << lq);
  if (row < 0 || row >= rows) return rows;
  if (row < head) {
    *group = row; *s0 = 0; *s1 = TDR_SU_NSECT;
  } else {
    const int t = row - head, part = t & ((1 << lq) - 1);
    *group = head + (t >> lq);
    *s0 = part << (3 - lq);
    *s1 = (part + 1) << (3 - lq);
  }
  return rows;
}
// the split of a launch: tdr_config_tuning("su_tail_groups" / "su_tail_parts") and the rule of the shapes (tdr_score_su.hip)
void tdr_su_tail(int nchunks, int64_t n, int* k, int* q);

struct SuLaunch {
  const tdr_map_desc* map;   // with a narrow compact form
  const float* tab;          // [P][2]: (tab*scale)*res when uniform_scale, else the table itself
  bool uniform_scale;
  const float* tab_src = nullptr;   // the caller's table itself: what the preparation reads (score_prep_kernel) ...
  float* utab_out = nullptr;        // ... and, with a uniform scale, where it writes (tab*scale)*res — `tab` above, filled by it
  const float* scan_pk;
  int nb, nr, rf;
  float res;
  const float* st;
  int64_t cap, n;
  const int32_t* perm;       // caller's locality order (NULL = identity)
  int group, nchunks;
  int tail_k = 0, tail_q = 1;   // the last tail_k ring groups go as tail_q rows each (su_tail_plan) ...
  int rows = 0;              // ... which makes this many rows of the shift-uniform kernel's grid
  int64_t npad;              // slot capacity = stride of the sums (su_npad)
  float* part;               // the launch's integer sums, ONE block [2 ncls + 2][npad] of words that every row and wave adds to
                             // (tdr_score_int_dev.h: int_add_sums); NULL: the preparation alone, nothing to zero
  int ray_split;             // waves per scattered particle (tdr_ray_splits)
  const float* fac;          // the table's factors (tdr_polar_factors_host) or NULL
  float uscale;              // the caller's uniform scale (<= 0: none)
  int32_t* ws;               // tdr_su_ws(...).total words
  float span;                // map cells the 64 locality neighbours of a dense particle may span (tdr_su_span_begin)
};
// Whether the launch's bins with several classes go to the shift-uniform kernel's list pass (tdr_config_tuning(
// "su_full_list"), default 1) instead of being handed from its assembly loop to the C++ step one four-ring step at a time:
// the ring groups the assembly loop takes, whose mask words a wave of the preparation can cut out of one ballot.  Same bits.
static inline bool tdr_su_full_list(const SuLaunch& L) {
  return tdr_cfg().su_full_list && (L.group == 4 || L.group == 8 || L.group == 16);
}
// ordering passes + the scan-side preparation (everything but the scoring kernels).  slots_out: the slot list — the dense
// particles by heading bin, every bin padded to whole waves (-1), then the sparse particles in the caller's order
// (su_key_kernel); counts_out: device words {slots of the heading bins, sparse particles behind them, both together (what
// finalize walks)}.  The preparation is ONE kernel (score_prep_kernel, tdr_score_su.hip) for both scoring kernels: the
// uniform-scale table, the shift-uniform layout (offsets, descriptors, bounding boxes) and the ray-mapped layouts (offsets,
// radii, 16-bit descriptors, the list, the `inexact` words, the mass bound).
int tdr_su_prepare(const SuLaunch& L, const SuWs& W, hipStream_t s, const int32_t** slots_out, const int32_t** counts_out);
// the ordering passes alone (L.st, cap, n, perm, nb, span, ws; nb == 1: no heading bins — the Cartesian score).  box_init
// (optional): box_count boxes {min, max, min, max} that su_offsets_kernel sets to {+FLT_MAX, -FLT_MAX, ...} for the
// preparation to lower / raise.
int tdr_su_order(const SuLaunch& L, const SuWs& W, hipStream_t s, const int32_t** slots_out, const int32_t** counts_out,
                 float* box_init = nullptr, int box_count = 0);
// tests (tdr_k_score_prep): the preparation's products out of L.ws — out[0..8] = utab, tab_su, desc, bbox, tab_ray, desc_ray,
// rad_ray, list, the words behind the counts (device memory, NULL: not wanted) — and the shapes behind their sizes
int tdr_su_prep_copy_out(const SuLaunch& L, const SuWs& W, hipStream_t s, int64_t layout[16], void* const out[9]);
// The span for this launch.  With a fixed span (tdr_config_shift_uniform_span, TDR_SU_SPAN) that one; otherwise it is tuned
// while the filter runs: a few candidates are timed over one launch each (events on `s` around the whole scoring call,
// tdr_su_span_end closes the measurement), the fastest is kept, and the trial is repeated every few thousand launches
// (`shape`: anything that identifies the launch's sizes; a change restarts the trial).  The span only routes particles
// between two kernels that produce identical partial sums: results do not depend on it.
// The tuner's state belongs to the caller's tdr_score_ctx (tdr.h); without one the span is the configured / default one.
// Nothing here waits on the host: a trial whose events have not completed when the next call arrives is repeated.
struct SpanTuner {
  int64_t shape = -1;
  int phase = -2;                     // < 0: skipping; < number of candidates: timing that candidate; else settled
  int settled_launches = 0;
  int trial = 0;                      // timed calls of the current candidate so far
  float best = 16.f;                  // the span in use: what the last COMPLETED round of trials found fastest
  float round_best = 16.f, best_ms = 3.0e38f;   // the fastest candidate of the round in progress, and its time
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool open = false, pending = false;
  int64_t trial_calls = 0;            // launches that ran at a candidate span so far (diagnostics: tdr_score_ctx_trial_calls)
};
float tdr_su_span_begin(SpanTuner* t, int64_t shape, hipStream_t s);
void tdr_su_span_end(SpanTuner* t, hipStream_t s);
// the shift-uniform kernel over the heading bins' slots
int tdr_su_score(const SuLaunch& L, const SuWs& W, hipStream_t s);
// the ray-mapped kernel (tdr_score_ray.hip): whether the map carries what it reads (class planes, integer dictionary
// space), the split of a window over waves, its tables / the `inexact` flag (before either scoring kernel), the launch
bool tdr_ray_map_ok(const tdr_map_desc* map);
int64_t tdr_ray_padded_samples(int nb, int nr);   // window samples with every direction padded to whole blocks of steps
int tdr_ray_splits(int nb, int nr, int64_t n, bool block_major = false);
// The ray-mapped kernel's layouts of a launch (tdr_score_ray.hip has the description): gq steps of 64 rings per block,
// `blocks` blocks per direction; block-major / patch order.  The preparation (tdr_score_su.hip) writes them.
#define RAY_PR 16             // rings of a patch
#define RAY_PG 16             // scan rows of a unit (four steps of four directions)
#define RAY_PATCH_MAX_NB 256
// words of a sector's compact lists: its 1 024 bins in two streams of whole 256-entry blocks (at most five blocks)
#define RAY_CL_WORDS 1280
// no entry: scan row 0 and "ring 64" — the slot behind a segment's radii, whose radius leaves the map: the guard cell,
// unknown — of class 0's plane (an A entry always names a plane), with a count of zero
#define RAY_CL_NONE 0x01001000u
static inline bool ray_bm(const SuLaunch& L) { return tdr_cfg().ray_block_major && L.fac != nullptr; }
static inline bool ray_patch(const SuLaunch& L) { return ray_bm(L) && tdr_cfg().ray_patch && L.nb % RAY_PG == 0 && L.nb <= RAY_PATCH_MAX_NB; }
static inline int ray_gq(int nr, bool bm) { return bm ? 1 : (nr <= 64 ? 1 : (nr <= 128 ? 2 : 4)); }
static inline int ray_blocks(int nr, bool bm) { return (int)cdiv(nr, 64 * ray_gq(nr, bm)); }
int tdr_ray_score(const SuLaunch& L, const SuWs& W, hipStream_t s);
#endif  // TDR_SCORE_SU_H_
