// tdr_score_su.hip — the SHIFT-UNIFORM polar scoring kernel and its ordering passes (host interface: tdr_score_su.h).
//
// score_polar_kernel (tdr_score.hip) pairs window row i with scan row (i + shift) mod nb, shift = the lane's own heading
// bin (state_particle.cpp:124-128): the scan record is a per-lane operand (LDS), and every sample pays the full record
// decode and every class's FMA although a LiDAR scan is sparse — in the config-2 scan 44 % of the (theta, r) bins are
// empty in every class and a non-empty bin holds ~1.0 class (90 % of the class-bins are zero).
//
// Here the particles are processed in (shift, Morton) order with every shift bucket padded to whole waves, so the shift
// is WAVE-uniform: the scan side of a sample is a scalar operand (a four-dword descriptor read through the scalar cache —
// no LDS scan image) and "this bin is empty" / "this bin holds class c only" are wave-uniform branches:
//   every sample        coordinates + the `known` bit from the KNOWN MASK (tdr_cmap.hip), which the workgroup stages in LDS
//                       for the part of the map the windows of its 256 particles cover in the current sector of directions
//   one class present   + ONE dword of the compact record (4-byte gather), one dictionary decode, 2 FMAs (class, norm)
//   several classes     the packed scan record through scalar loads, one decode + FMA per class present
// An empty bin — 44 % of the samples — touches no map record at all; a 64-lane gather is what the L1 address path prices
// highest (>= 16 cycles per CU, tools/ta_cost.hip).  Skipping an FMA whose scan operand is zero leaves the accumulator
// unchanged bit for bit (fma(0, m, acc) == acc for finite m, acc never -0), and the samples of a particle are visited in
// the same order — direction ascending, ring ascending within the group — with the same partition into per-group partial
// sums, so both kernels produce IDENTICAL partial sums (tests/test_shift_uniform.py).  Non-finite dictionary or scan
// values (0 * inf = NaN must not be skipped) turn the skipping off bin by bin (descriptor code SU_CODE_FULL_ALL).
//
// Per launch (all on the caller's stream, nothing synchronises):
//   su_key_kernel      heading bin of every particle (in the caller's locality order) + the histogram of the bins of every
//                      segment of 512 consecutive positions: one row of a table [segment][bin]
//   su_colscan_kernel  the table's columns -> their exclusive prefix over the segments, the column sums (particles per bin)
//   su_offsets_kernel  bucket starts in the padded slot list, number of slots in use; the -1 of the padding slots, the zero
//                      of the words later kernels add to
//   su_rank_scatter_kernel  slot -> particle: a wave per segment, ranks among equal bins by ballots — the (shift, Morton)
//                      order, i.e. a stable sort by bin, in one pass
//   (where the table would be out of proportion — the rule at su_seg_table_words — and under tdr_config_tuning(
//    "su_order_bucket", 0): two fills, su_key_kernel, su_offsets_kernel, rocPRIM's stable radix sort by bin, su_scatter_kernel)
//   score_prep_kernel  the scan side, for this kernel and for the ray-mapped one (tdr_score_ray.hip), one thread per
//                      (direction, ring): the uniform-scale table; sample offset and scan descriptor, group-major (a wave
//                      streams them in order); the bounding box of the sample offsets of every (ring group, sector of
//                      directions), on the words su_offsets_kernel initialised; the ray-mapped layouts and the `inexact` words
//   score_polar_ray_kernel, score_polar_su_kernel, then score_finalize_exact_kernel over the slots (tdr_score.hip)
//
// Compiled with -mllvm -structurizecfg-skip-uniform-regions (build.py): the per-sample dispatch on the descriptor is a
// tree of wave-uniform branches; left to the structuriser each leaf is followed by copies of all accumulators (phi
// merges of its flow blocks: 128 v_mov_b64 in the loop), with uniform regions skipped the leaves are 3-4 instructions.
// Memory operations: the hand-scheduled inner loop (tdr_score_su_asm.h, generated and statically checked by
// tools/gen_su_asm.py) issues its loads and the waits for them inside ONE assembly text with a planned register file — the
// compiler sees a single statement with declared outputs and clobbers.  Everything else in this file loads through plain
// C++ (the compiler tracks the destination registers and places the waits): rounds 3-4 issued the C++ steps' loads through
// separate inline-assembly statements with hand-counted s_waitcnt, which twice let the compiler move a copy between a load
// and its wait ("fragile") — that pattern is gone.
#include <rocprim/device/device_radix_sort.hpp>

#include <atomic>

#include "tdr_score_int_dev.h"
#include "tdr_score_su.h"
#include "tdr_score_su_asm.h"

#define SU_CODE_FULL 0xFFu       // several classes present: packed scan record, classes with a zero count skipped
#define SU_CODE_FULL_ALL 0xFEu   // a non-finite value is in play: every class multiplied like score_polar_kernel does
#define SU_CODE_PAD 0xFDu        // no such ring: the last group of an image whose ring count is no multiple of the group
#define SU_NSECT TDR_SU_NSECT    // 8 sectors of directions per known-mask staging (16: 2 % slower on config 2)
#define SU_BOX_WORDS 4096        // LDS words of the staged known mask: 16 KB (config 2's dense share 2.97 ms at 12 KB, 2.81 at 16
                                 // and at 20 KB, 4.18 at 24 KB, where a sixth wave per SIMD no longer fits; a wave that
                                 // stages a box of its own — the far-apart waves of config 5 — has a quarter of it)

struct SuArgs {
  const uint32_t* crec;    // compact records (narrow form)
  const uint32_t* kmask;   // the map's known mask (behind the tiles of crec)
  int kcolw;               // words of one of its tile columns (32 kmask_trows)
  unsigned kmask_off;      // its byte offset from crec
  const uint32_t* dict_int;   // the dictionary as integers: value * 2^q (tdr_cmap.hip)
  int dict_n, ctiles_r;
  int pkcol;               // class planes (tdr_cmap.hip): bytes of a tile column - 16 (plane_offset); their constants come with the descriptors
  const int32_t* inexact;  // device words (int_form_off): this scan / map has no exact integer form, the launch does nothing
  int rows, cols;          // map
  float resolution;
  const float* tab_su;     // [nchunks][nb][group][2]: (tab*scale)*res (USCALE) or tab
  const uint32_t* desc;    // [nchunks][nb][group][4]: scan descriptor of bin (row, ring), see score_prep_kernel
  const float* bbox;       // [nchunks][SU_NSECT][4]: min / max of tab_su's two coordinates over the sector
  const float* scan_pk;    // [nr][nb][rf]: read for bins holding several classes
  int nb, nr;
  float res;
  const float* st;
  int64_t cap;
  const int32_t* slots;    // padded (shift, Morton) order, -1 = padding; every 64-slot batch holds one shift
  const int32_t* nslots;   // device word: slots in use (a multiple of 64)
  int group, nchunks, ncls;
  int tail_k, tail_q;      // grid.y = the rows of su_tail_plan(nchunks, tail_k, tail_q, ...)
  int64_t npad;            // stride of the sums
  uint32_t* part;          // the launch's sums [2 ncls + 2][npad]: every row adds its share (int_add_sums, tdr_score_int_dev.h)
  uint32_t* stats;         // NULL, or (profiling) counters of the variants the wave-sectors ran: tdr_profile_variants
  const uint32_t* full_mask;   // [nchunks][2 nb]: the bins with several classes (score_prep_kernel), NULL: no list pass — the
                               // assembly loop hands their steps to the C++ step (tdr_config_tuning("su_full_list", 0))
  unsigned pbase, plane_bytes; // class c's plane: plane_offset's constant pbase + c * plane_bytes (the list pass)
  uint32_t* list_stats;    // NULL, or (profiling) {steps handed back to the C++ step, bins the list pass scored}: tdr_profile_su_list
};

// The scan-side preparation of an integer-form launch: ONE kernel, one thread per (scan row / direction i, padded ring j), j
// fastest in a wave; a workgroup is PREP_DIRS neighbouring directions over the same 64 rings.  rp, the padded ring count, is a multiple of 64 that covers the shift-uniform layout (nchunks x group rings) and the
// ray-mapped one (blocks x gq x 64): a wave is 64 consecutive rings of ONE direction, four consecutive lanes are an aligned
// group of four rings — what the shuffles below lean on.  A thread reads its table entry and its bin's scan record once and
// writes, for both scoring kernels:
//   utab (with a uniform scale)  (tab * scale) * res in the table's own order, two roundings (top_down_map_polar.cpp:28): the
//                       float form behind the integer kernels and the ray-mapped kernel's list pass read it
//   tab_su, desc        the shift-uniform layout [nchunks][nb][group]: sample offset and the four-dword scan descriptor
//   bbox                bounding box of the sample offsets of every (ring group, sector of directions): a wave reduces the rings
//                       of each group it holds, the workgroup's waves of one sector meet in LDS, then one atomic min / max
//                       per workgroup, group, sector and box word, on the words su_offsets_kernel initialised ({+FLT_MAX,
//                       -FLT_MAX, ...}; float minima / maxima: any order)
//   tab_ray, rad_ray, desc_ray, list, n_list, inexact[0..2], the mass bound     the ray-mapped kernel's layouts and the
//                       words that decide between the integer and the float form (tdr_score_ray.hip has the layouts)
//   clist, ctab         (patch order only) the sectors' compact bin lists and their table: described where the kernel writes them
// Nothing is kept between calls: the table may change under the same pointer.
//
// Scan descriptor of a bin (shift-uniform layout), four dwords:
//   [0] code: 0 = every class zero; c + 1 = class c alone is non-zero; SU_CODE_FULL = several classes;
//       SU_CODE_FULL_ALL = a non-finite dictionary / scan value: no skipping in this bin
//   [1] the bin's count summed over the classes, as an integer — for a single class: its count
//   [2] a single class: the constant of plane_offset for the class's PLANE (byte offset from crec: pbase + c * plane_bytes) —
//       the 2-byte cell of the one class is what such a bin fetches: tiles of 8 x 8 cells, a third of the lines the 4 x 4-cell
//       record tiles cost a wave whose particles lie a few cells apart (the gathers' lines bound this kernel: DESIGN.md
//       5.1); several classes: the constant of the record offset (cmap_offset)
//   [3] bit 31, on the first bin of a step (4 consecutive rings) only: one of the step's bins is SU_CODE_FULL / SU_CODE_FULL_ALL
//   (the steps that read RECORDS — the C++ steps, for bins with several classes and their neighbours, and the far path —
//    work the record constants of a single class out of its code: su_rec_const / single_class)
// A ring the image does not have (j >= nr) inside the last group: SU_CODE_PAD and the offset of the direction's last real ring
// (inside every box the real ones span); it stays out of the box.
//
// Ray-mapped layouts.  tab_ray[((i * blocks + b) * 64 + l) * GQ + g] = sample offset of (direction i, ring j); desc_ray
// (16-bit) at the same index for scan row i, ring j: code << 12 | count — code 0: nothing for the loop (an empty bin, or one
// that went on the list), c + 1: class c alone.  Rings beyond nr: an offset far outside the map (their cell is the guard
// cell: unknown), descriptor 0.  `list`: bins holding several classes or a count >= 4096, as row << 16 | ring (any order:
// the sums are exact).  inexact[0] is raised when the scan has no integer form: a count that is negative, fractional, not
// finite or >= 2^24, or a dictionary without one (tdr_cmap.hip), or a bound on the total count that reached 2^24; inexact[1]
// collects that bound modulo 2^32 (int_form_off).  fac (optional): the table's factors (tdr_polar_factors_host).  rad_ray[(b * 64 + l) * GQ + g] = ring j's
// radius (rings beyond nr: 1e30 — one of a direction's two products then leaves the map whatever the direction); inexact[2]
// is raised when an entry of the table is not the float product its factors give (with a uniform scale: that product, scaled
// the same way) — the scoring kernel then reads tab_ray instead of multiplying the factors itself.
struct PrepArgs {
  const float* tab;        // the caller's table [nr][nb][2]
  const float* scan_pk;    // [nr][nb][rf]
  int nb, nr, rf, ncls, rp;
  float uscale, res;       // uscale > 0: a uniform scale
  float* utab;             // NULL without a uniform scale
  // shift-uniform layout
  int group, nchunks, ckconst;
  unsigned pbase, plane_bytes;
  const float* dict;
  int dict_n;
  float* tab_su;
  uint32_t* desc;
  float* bbox;
  // ray-mapped layouts
  int gq, blocks, bm, patch, borrow;
  const uint32_t* dict_tail;
  const float* fac;
  float* tab_ray;
  float* rad_ray;
  uint16_t* desc_ray;
  uint32_t* list;
  int32_t* n_list;
  int32_t* inexact;
  uint32_t* clist;         // the compact lists of the patch order's sectors (NULL: none), and their table
  int32_t* ctab;
  uint32_t* full_mask;     // NULL, or [nchunks][2 nb]: bit jj of word (group, scan row i) — and of word nb + i, so that a sector's
                           // rows need no wrap — says bin (i, ring group * G + jj) is SU_CODE_FULL (G divides 64, G <= 32)
  uint32_t* sums;          // NULL (the preparation on its own), or the launch's integer sums: sums_words words, zeroed here
  int64_t sums_words;
};
// float minimum / maximum on a word that holds a float: the sign decides which integer order is the float order (a NaN is left
// out, as fminf / fmaxf leave it out)
__device__ __forceinline__ void atomic_min_float(float* at, float v) {
  if (!(v == v)) return;
  if (__float_as_int(v) >= 0) atomicMin(reinterpret_cast<int*>(at), __float_as_int(v));
  else atomicMax(reinterpret_cast<unsigned*>(at), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_float(float* at, float v) {
  if (!(v == v)) return;
  if (__float_as_int(v) >= 0) atomicMax(reinterpret_cast<int*>(at), __float_as_int(v));
  else atomicMin(reinterpret_cast<unsigned*>(at), __float_as_uint(v));
}
// directions of a workgroup, a wave each: 8, or — a launch that writes the compact lists — the 16 scan rows of a unit, so
// that a workgroup holds one whole SECTOR (16 scan rows x 64 rings = four units) and ranks its bins in LDS
#define PREP_DIRS_COMPACT RAY_PG
#define PREP_KEYS 80   // compact lists: keys unit * 16 + class code (A), 64 + unit (B)
template <int PREP_DIRS>
__device__ __forceinline__ void score_prep_body(const PrepArgs& a, const unsigned block) {
  const int nb = a.nb, nr = a.nr, rf = a.rf, rp = a.rp;
  __shared__ float red[PREP_DIRS][64][4];   // the waves' box candidates
  __shared__ unsigned wg_mass, wg_listed, wg_list_base;
  // compact lists: a scan row's entries per key (then: the entries of the rows before it), the sector's, and where a key's run starts
  __shared__ unsigned crow[PREP_DIRS == PREP_DIRS_COMPACT ? PREP_DIRS : 1][PREP_KEYS], ckeys[PREP_KEYS], cbase[PREP_KEYS];
  if (threadIdx.x == 0) { wg_mass = 0; wg_listed = 0; }
  if constexpr (PREP_DIRS == PREP_DIRS_COMPACT)
    for (int t = threadIdx.x; t < PREP_DIRS * PREP_KEYS; t += 64 * PREP_DIRS) (&crow[0][0])[t] = 0;
  bool bad = false;   // the dictionary is small: every workgroup checks it for itself
  for (int k = threadIdx.x; k < a.dict_n; k += blockDim.x) bad |= !(fabsf(a.dict[k]) <= 3.402823466e+38f);
  const bool dict_bad = __syncthreads_or(bad);   // (also: the three words above are set)
  if (block == 0 && threadIdx.x == 0 && a.dict_tail[1] != 1u) atomicOr(a.inexact, 1);
  // a workgroup: PREP_DIRS neighbouring directions (a wave each) x the same 64 rings — neighbouring directions share the lines
  // of the table and of the scan, and their boxes, the list and the mass bound meet in LDS: the words that many workgroups add
  // to get one atomic per workgroup, not one per wave or bin (same-line atomics are what this kernel's time was)
  const int segs = rp >> 6, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i_raw = (int)(block / segs) * PREP_DIRS + wave, j = (int)(block % segs) * 64 + lane;
  const bool live = i_raw < nb;   // (a whole wave)
  const int i = live ? i_raw : nb - 1;
  const bool real = live && j < nr;
  const int64_t k = (int64_t)(j < nr ? j : nr - 1) * nb + i;   // (no such ring: the direction's last real one)
  // (one request per table entry, two or three per record: a wave's 64 rings of one direction lie nb entries apart, every
  // load touches 64 lines)
  const float2 te = *reinterpret_cast<const float2*>(a.tab + 2 * k);
  float tx = te.x, ty = te.y;
  if (a.utab) {
    tx = (tx * a.uscale) * a.res;   // `ang_sample_pts_*scale*res` (top_down_map_polar.cpp:28)
    ty = (ty * a.uscale) * a.res;
    if (real) *reinterpret_cast<float2*>(a.utab + 2 * k) = make_float2(tx, ty);
  }
  // the bin's record, once (rf is 4, 8 or 12: tdr_su_prepare)
  float rec[12];
#pragma unroll
  for (int q = 0; q < 3; q++) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (real && 4 * q < rf) v = reinterpret_cast<const float4*>(a.scan_pk + k * rf)[q];
    rec[4 * q] = v.x; rec[4 * q + 1] = v.y; rec[4 * q + 2] = v.z; rec[4 * q + 3] = v.w;
  }
  int nz = 0, first = 0;
  bool finite = true, whole = true;
  float vfirst = 0.f, sum = 0.f;
  if (real) {
#pragma unroll
    for (int c = 0; c < 11; c++)
      if (c < a.ncls) {
        const float v = rec[c];
        finite &= fabsf(v) <= 3.402823466e+38f;
        whole &= v >= 0.f && v < 16777216.f && v == floorf(v);
        if (v != 0.f) {
          if (!nz) { first = c; vfirst = v; }
          nz++;
        }
      }
    sum = rf == 4 ? rec[3] : (rf == 8 ? rec[7] : rec[11]);
    whole &= sum >= 0.f && sum < 16777216.f && sum == floorf(sum);
  }
  // ---- the mass bound: a wave's sum
  uint32_t mass = 0;
  if (real && sum >= 1.f && sum < 16777216.f) mass = ((uint32_t)sum >> 8) + 1u;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mass += __shfl_xor(mass, d, 64);
  if (lane == 0 && mass) atomicAdd(&wg_mass, mass);
  // ---- the shift-uniform layout
  const int group = a.group;
  const bool su_live = live && j < a.nchunks * group;
  const int chunk = j / group, jj = j - chunk * group;
  uint32_t code = SU_CODE_PAD, ckc = (uint32_t)a.ckconst;
  float val = 0.f;
  if (real) {
    code = 0;
    // (a non-finite or fractional count: the launch runs in its float form instead — `inexact` below)
    if (dict_bad || !finite) { code = SU_CODE_FULL_ALL; val = sum; }
    else if (nz == 1) { code = (uint32_t)first + 1u; val = vfirst; ckc = a.pbase + (uint32_t)first * a.plane_bytes; }
    else if (nz > 1) { code = SU_CODE_FULL; val = sum; }
  }
  // steps are 4 consecutive bins (group is a multiple of 4, so they are 4 consecutive threads of a wave)
  uint32_t anyfull = code >= SU_CODE_FULL_ALL ? 1u : 0u;
  anyfull |= __shfl_xor(anyfull, 1);
  anyfull |= __shfl_xor(anyfull, 2);
  if (su_live) {
    const int64_t at = ((int64_t)chunk * nb + i) * group + jj;
    *reinterpret_cast<float2*>(a.tab_su + 2 * at) = make_float2(tx, ty);
    *reinterpret_cast<uint4*>(a.desc + 4 * at) = make_uint4(code, (uint32_t)val, ckc, ((jj & 3) == 0 && anyfull) ? 0x80000000u : 0u);
  }
  // the bins with several classes, a word per (ring group, scan row): the wave's 64 rings are whole groups, a group's first
  // lane cuts its slice out of the ballot (the shift-uniform kernel's list pass walks these words)
  if (a.full_mask) {   // (uniform)
    const unsigned long long fullb = __ballot(su_live && code == SU_CODE_FULL);
    if (su_live && jj == 0) {
      const uint32_t wv = (uint32_t)(fullb >> lane) & (group >= 32 ? 0xFFFFFFFFu : (1u << group) - 1u);
      uint32_t* row = a.full_mask + (int64_t)chunk * 2 * nb + i;
      row[0] = wv;
      row[nb] = wv;
    }
  }
  // the boxes: the real rings of a group that this wave holds are consecutive lanes — a segmented reduction towards the
  // segment's first lane (minima and maxima: a lane may meet an operand twice); the waves' candidates meet in LDS below
  // the sector s with s nb / SU_NSECT <= dir < (s + 1) nb / SU_NSECT
  auto sector = [&](int dir) { return (int)((SU_NSECT * ((int64_t)dir + 1) - 1) / nb); };
  {
    const float big = 3.402823466e+38f;
    float lo0 = real ? tx : big, hi0 = real ? tx : -big, lo1 = real ? ty : big, hi1 = real ? ty : -big;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float o0 = __shfl_down(lo0, d, 64), o1 = __shfl_down(hi0, d, 64), o2 = __shfl_down(lo1, d, 64), o3 = __shfl_down(hi1, d, 64);
      const int oc = __shfl_down(chunk, d, 64);
      if (lane + d < 64 && oc == chunk) {
        lo0 = fminf(lo0, o0); hi0 = fmaxf(hi0, o1);
        lo1 = fminf(lo1, o2); hi1 = fmaxf(hi1, o3);
      }
    }
    red[wave][lane][0] = lo0; red[wave][lane][1] = hi0; red[wave][lane][2] = lo1; red[wave][lane][3] = hi1;
  }
  // ---- the ray-mapped layouts
  const bool ray_live = live && j < a.blocks * a.gq * 64;
  uint32_t d = 0;
  bool listed = false;
  unsigned list_rank = 0;
  if (real) {
    if (a.fac) {
      float fx = a.fac[2 * i] * a.fac[2 * nb + j], fy = a.fac[2 * i + 1] * a.fac[2 * nb + j];
      if (a.uscale > 0.f) {
        fx = (fx * a.uscale) * a.res;
        fy = (fy * a.uscale) * a.res;
      }
      if (__float_as_uint(fx) != __float_as_uint(tx) || __float_as_uint(fy) != __float_as_uint(ty)) atomicOr(a.inexact + 2, 1);
    }
    if (!whole) atomicOr(a.inexact, 1);
    else if (nz == 1 && vfirst < 4096.f) d = (uint32_t)vfirst | ((uint32_t)(first + 1) << 12);
    else if (nz >= 1) { listed = true; list_rank = atomicAdd(&wg_listed, 1u); }
  }
  // ---- the compact lists (tdr_score_ray.hip: the patch order with the table's factors).  The workgroup is ONE sector: its
  // four units' A lists — the single-class bins the loop multiplies, unit by unit and class by class inside a unit — then the
  // four B lists: the bins the loop sees as empty (those on `list` too: it counts their cell's known bit).  An entry is
  // (scan row & 15) << 28 | (ring & 63) << 18 | descriptor — bits 25-31 the byte offset of the row's direction pair, bits 16-24
  // that of the ring's radius in the kernel's LDS tables: two shifts decode it.  Rings the image
  // does not have are in neither list.  Inside a class run the entries keep the order scan row, ring: four neighbouring lanes
  // of a gather are then, as far as the scan allows, neighbouring rings of one scan row — the cells one line holds.  No
  // atomics: a wave is a scan row, its ranks are ballots; the rows meet in LDS.
  const bool compact = PREP_DIRS == PREP_DIRS_COMPACT && a.clist != nullptr && j < a.blocks * 64;   // (a whole workgroup)
  unsigned ckey = 0, crank = 0;
  if (compact) {
    const unsigned unit = (unsigned)lane >> 4, code = d >> 12;
    const unsigned long long umask = 0xFFFFull << (16 * unit), below = (1ull << lane) - 1ull;
    ckey = code ? unit * 16u + code : 64u + unit;
    for (unsigned c = 0; c <= (unsigned)a.ncls; c++) {
      const unsigned long long same = __ballot(real && code == c) & umask;
      if (real && code == c) {
        crank = (unsigned)__popcll(same & below);
        if ((same >> lane) == 1ull) crow[wave][ckey] = crank + 1u;   // (the key's last lane of the row)
      }
    }
  }
  const uint32_t centry = (((uint32_t)i & (RAY_PG - 1)) << 28) | (((uint32_t)j & 63u) << 18) | d;
  // An EMPTY bin (and one that went on the list) needs its cell's known bit and nothing else — and every class plane carries that
  // bit (bit 15 of a cell).  Four consecutive lanes of a gather — four consecutive rings of one scan row, in every order —
  // are served together by the L1's address path, at a cost per distinct LINE among them: an empty bin between two bins of
  // class c that reads the coarse mask plane is a line of its own, one that reads class c's plane with a count of zero rides
  // along.  So an empty bin borrows the class of the nearest non-empty bin of its aligned group of four rings (none: code 0,
  // the mask plane, one line for the four); the product with a zero count adds nothing (round 5).
  {
    const uint32_t own = d >> 12;
    const int ql = lane & 3;
    uint32_t c4[4];
#pragma unroll
    for (int q = 0; q < 4; q++) c4[q] = __shfl(own, (lane & 60) + q, 64);   // (threads of a group: the same scan row i, rings 4 q' .. 4 q' + 3)
    if (a.borrow && own == 0) {
      uint32_t pick = 0;
#pragma unroll
      for (int dist = 3; dist >= 1; dist--) {   // the nearest wins (written last)
        if (ql + dist < 4 && c4[(ql + dist) & 3]) pick = c4[(ql + dist) & 3];
        if (ql - dist >= 0 && c4[(ql - dist) & 3]) pick = c4[(ql - dist) & 3];
      }
      d = pick << 12;
    }
  }
  // ---- what the workgroup adds to the launch's words: one atomic each
  __syncthreads();
  if (threadIdx.x == 0) {
    // the bound must never read low: the word wraps at 2^32 (65 536 bins of 2^24 - 1 add up to exactly that), so the addition
    // that carries it to 2^24 or past it raises inexact[0] as well — the word starts at 0 and one addition is at most
    // 512 x 65 536 = 2^25, so the first such addition sees a word below 2^24 and cannot have wrapped it
    if (wg_mass && (uint64_t)atomicAdd(reinterpret_cast<unsigned*>(a.inexact) + 1, wg_mass) + wg_mass >= (1u << 24)) atomicOr(a.inexact, 1);
    wg_list_base = wg_listed ? (unsigned)atomicAdd(a.n_list, (int)wg_listed) : 0u;
  }
  if (compact) {   // (80 keys: 16 rows, then up to 80 additions each — nothing next to the loads above)
    if (threadIdx.x < PREP_KEYS) {
      unsigned run = 0;
      for (int w = 0; w < PREP_DIRS; w++) {
        const unsigned c = crow[w][threadIdx.x];
        crow[w][threadIdx.x] = run;
        run += c;
      }
      ckeys[threadIdx.x] = run;
    }
    __syncthreads();
    if (threadIdx.x < PREP_KEYS) {
      unsigned at = 0;
      for (int q = 0; q < (int)threadIdx.x; q++) at += ckeys[q];
      cbase[threadIdx.x] = at;
    }
  }
  // the box of (ring group, sector): the first of the workgroup's directions in the sector gathers the others'
  if (real && (lane == 0 || jj == 0)) {
    const int sect = sector(i);
    if (wave == 0 || sector(i - 1) != sect) {
      float lo0 = red[wave][lane][0], hi0 = red[wave][lane][1], lo1 = red[wave][lane][2], hi1 = red[wave][lane][3];
      for (int w = wave + 1; w < PREP_DIRS && i + (w - wave) < nb && sector(i + (w - wave)) == sect; w++) {
        lo0 = fminf(lo0, red[w][lane][0]); hi0 = fmaxf(hi0, red[w][lane][1]);
        lo1 = fminf(lo1, red[w][lane][2]); hi1 = fmaxf(hi1, red[w][lane][3]);
      }
      float* box = a.bbox + ((int64_t)chunk * SU_NSECT + sect) * 4;
      atomic_min_float(box, lo0);
      atomic_max_float(box + 1, hi0);
      atomic_min_float(box + 2, lo1);
      atomic_max_float(box + 3, hi1);
    }
  }
  __syncthreads();
  if (listed) a.list[wg_list_base + list_rank] = ((uint32_t)i << 16) | (uint32_t)j;   // (any order: the sums are exact)
  if (compact) {
    // sector = (segment of 64 rings, group of 16 scan rows), numbered as the ray-mapped kernel walks them; its lists have a
    // fixed place (no launch-wide counter): RAY_CL_WORDS words, the A stream from the front in blocks of 256 entries, the B
    // stream from the first block behind it.  A block is stored lane-major — entry r of a stream at (r >> 8) * 256 + (r & 63) * 4
    // + ((r >> 6) & 3) — so that ONE 16-byte load per lane brings a wave the entries of four gathers; what a stream's last
    // block has left is filled with RAY_CL_NONE (the kernel reads whole gathers and tests nothing).  The table, 16 words:
    // per unit {its first A entry, A entries, its first B entry, B entries} (positions in the two streams)
    const int64_t sector = (int64_t)(j >> 6) * (nb / RAY_PG) + i / RAY_PG;
    const unsigned n_a = cbase[64];
    if (threadIdx.x < 512) {
      const unsigned stream = threadIdx.x >> 8, t = threadIdx.x & 255u;
      const unsigned n = stream ? cbase[67] + ckeys[67] - n_a : n_a, blk = (stream ? (n_a + 255u) >> 8 : 0u) + (n >> 8);
      if (t >= (n & 255u) && (n & 255u)) a.clist[sector * RAY_CL_WORDS + blk * 256u + (t & 63u) * 4u + (t >> 6)] = RAY_CL_NONE;
    }
    if (real) {
      unsigned r = cbase[ckey] + crow[wave][ckey] + crank, blk0 = 0;
      if (ckey >= 64u) { r -= n_a; blk0 = (n_a + 255u) >> 8; }
      a.clist[sector * RAY_CL_WORDS + (blk0 + (r >> 8)) * 256u + (r & 63u) * 4u + ((r >> 6) & 3u)] = centry;
    }
    if (threadIdx.x < 4) {
      const unsigned u = threadIdx.x;
      int32_t* t = a.ctab + sector * 16 + 4 * u;
      t[0] = (int32_t)cbase[16 * u];
      t[1] = (int32_t)(cbase[16 * u + 16] - cbase[16 * u]);
      t[2] = (int32_t)(cbase[64 + u] - n_a);
      t[3] = (int32_t)ckeys[64 + u];
    }
  }
  if (!ray_live) return;
  const int g = j >> 6, l = j & 63, b = g / a.gq, gq = a.gq;
  const int64_t at = a.bm ? ((int64_t)b * nb + i) * 64 + l : (((int64_t)i * a.blocks + b) * 64 + l) * gq + (g - b * gq);
  // patch order (descriptors only; the offsets keep the block-major order): unit (ring block j / 16, scan-row group i / 16),
  // lane (i & 3) * 16 + (j & 15), step (i & 15) >> 2 — a lane's four steps side by side
  int64_t at_d = at;
  if (a.patch) at_d = ((((int64_t)(j / RAY_PR) * (nb / RAY_PG) + i / RAY_PG) * 64 + (i & 3) * RAY_PR + (j % RAY_PR)) << 2) + ((i % RAY_PG) >> 2);
  if (a.fac && i == 0) a.rad_ray[((int64_t)b * 64 + l) * gq + (g - b * gq)] = real ? a.fac[2 * nb + j] : 1.0e30f;
  *reinterpret_cast<float2*>(a.tab_ray + 2 * at) = real ? make_float2(tx, ty) : make_float2(-1.0e30f, -1.0e30f);
  a.desc_ray[at_d] = (uint16_t)d;
}
template <int PREP_DIRS>
__global__ __launch_bounds__(64 * PREP_DIRS) void score_prep_kernel(PrepArgs a) {
  // the launch in front of the scoring kernels: its threads zero the sums those add to, in every call (nothing is kept between
  // calls) — stores that need no answer, in front of the loads below
  int_zero_sums(a.sums, a.sums_words, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
  score_prep_body<PREP_DIRS>(a, blockIdx.x);
}

// Sort key of every particle (in the caller's locality order): its heading bin when its neighbourhood is DENSE, nb when
// it is SPARSE — the 64 particles around it in the locality (Morton) order are more than `span` map cells apart.  A
// workgroup of the shift-uniform kernel stages the known mask of everything its 256 particles' windows cover: dense
// particles sorted together keep that box small and share the cache lines of their record gathers.  Sparse ones share
// nothing whatever the order and are bound by the memory system, not by instruction issue: they keep their locality order
// and go through score_polar_kernel (tdr_score.hip), behind the dense ones in the same slot list.
// Histogram of the nb + 1 keys, per workgroup in LDS (a converged filter fills a few bins).  A workgroup takes `per_block`
// consecutive positions (a multiple of 256).  With seg_hist the workgroup's positions are one SEGMENT of the bucket sort
// (su_colscan_kernel) and its histogram is row blockIdx.x of seg_hist[segment][key]: every word of the row is written, nothing
// is zero-filled beforehand.  Without it (the rocPRIM path) the histogram is added to cnt, which the caller has zeroed.
__global__ __launch_bounds__(256) void su_key_kernel(const float* __restrict__ st, int64_t cap, int64_t n,
                                                     const int32_t* __restrict__ perm, int nb, float span, int per_block,
                                                     uint32_t* __restrict__ keys, int32_t* __restrict__ vals,
                                                     int* __restrict__ cnt, int* __restrict__ seg_hist) {
  extern __shared__ int hist[];
  for (int k = threadIdx.x; k <= nb; k += 256) hist[k] = 0;
  __syncthreads();
  for (int it = 0; it < per_block; it += 256) {
    const int64_t t = (int64_t)blockIdx.x * per_block + it + threadIdx.x;
    if (t >= n) break;
    const int32_t p = perm ? perm[t] : (int32_t)t;
    uint32_t key = (uint32_t)rot_shift_dev(st[TDR_ST_THETA * cap + p], nb);
    if (span > 0.f) {
      auto centre = [&](int64_t q, float& x, float& y) {
        const float sc = st[TDR_ST_SCALE * cap + q];
        x = st[TDR_ST_DX * cap + q] * sc + st[TDR_ST_INIT_X * cap + q];
        y = st[TDR_ST_DY * cap + q] * sc + st[TDR_ST_INIT_Y * cap + q];
      };
      const int64_t ta = t >= 32 ? t - 32 : 0, tb = t + 32 < n ? t + 32 : n - 1;
      float x0, y0, x1, y1;
      centre(perm ? perm[ta] : ta, x0, y0);
      centre(perm ? perm[tb] : tb, x1, y1);
      if (!(fabsf(x1 - x0) <= span && fabsf(y1 - y0) <= span)) key = (uint32_t)nb;   // (NaN positions: sparse)
    }
    keys[t] = key;
    vals[t] = p;
    atomicAdd(&hist[key], 1);
  }
  __syncthreads();
  if (seg_hist) {
    int* row = seg_hist + (int64_t)blockIdx.x * (nb + 1);
    for (int k = threadIdx.x; k <= nb; k += 256) row[k] = hist[k];
  } else {
    for (int k = threadIdx.x; k <= nb; k += 256)
      if (hist[k]) atomicAdd(&cnt[k], hist[k]);
  }
}

// ---- the bucket sort: a stable sort by a key of at most 4096 values is one ranked scatter ---------------------------------
// The positions t of the caller's order are cut into segments of SU_SEG consecutive ones; su_key_kernel leaves the table
// seg_hist[segment][key].  Here the table's columns are turned, in place, into their exclusive prefix over the segments —
// seg_hist[s][k] = particles of key k in the segments before s — and the column sums go to cnt[k].  A workgroup takes 64
// keys (a lane each, so a row's words are read side by side), its 16 waves a sixteenth of the segments each: the serial part
// of a workgroup is segments / 16 long whatever the key count.
#define SU_SEG 512
#define SU_COLSCAN_WAVES 16
__global__ __launch_bounds__(64 * SU_COLSCAN_WAVES) void su_colscan_kernel(int* __restrict__ seg_hist, int segs, int nkeys,
                                                                           int* __restrict__ cnt) {
  __shared__ int wsum[SU_COLSCAN_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + lane;
  const bool live = k < nkeys;
  const int per = (segs + SU_COLSCAN_WAVES - 1) / SU_COLSCAN_WAVES;
  const int s0 = min(w * per, segs), s1 = min(s0 + per, segs);
  int* col = seg_hist + (live ? k : 0);
  int sum = 0;
  if (live)
    for (int sgm = s0; sgm < s1; sgm += 8) {   // eight loads in flight
      int v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = sgm + u < s1 ? col[(int64_t)(sgm + u) * nkeys] : 0;
#pragma unroll
      for (int u = 0; u < 8; u++) sum += v[u];
    }
  wsum[w][lane] = sum;
  __syncthreads();
  int run = 0, tot = 0;
#pragma unroll
  for (int j = 0; j < SU_COLSCAN_WAVES; j++) {
    const int v = wsum[j][lane];
    run += j < w ? v : 0;
    tot += v;
  }
  if (!live) return;
  if (w == 0) cnt[k] = tot;
  for (int sgm = s0; sgm < s1; sgm += 8) {   // eight loads in flight, then the serial sums
    int v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = sgm + u < s1 ? col[(int64_t)(sgm + u) * nkeys] : 0;
#pragma unroll
    for (int u = 0; u < 8; u++) {
      if (sgm + u < s1) col[(int64_t)(sgm + u) * nkeys] = run;
      run += v[u];
    }
  }
}

// One workgroup.  The particles of key k start at start[k] in the sorted list and take slots [slot_start[k], + count) of
// the slot list, the count of a heading bin (k < nkeys - 1) rounded up to whole waves.
// counts = {slots of the heading bins (a multiple of 64), sparse particles behind them, both together}
// The bucket sort (pad_slots set) has no filled slot list and no zeroed words to start from: the up to 63 padding slots of a
// heading bin get their -1 here, and the words behind counts (TDR_SU_TAIL_INTS, which later kernels add to) their zero.
// box_init (either path, optional): box_count boxes of {min, max, min, max} get the values score_prep_kernel lowers / raises.
__global__ __launch_bounds__(256) void su_offsets_kernel(const int* __restrict__ cnt, int nkeys, int* __restrict__ start,
                                                         int* __restrict__ slot_start, int* __restrict__ counts,
                                                         int32_t* __restrict__ pad_slots, float* __restrict__ box_init,
                                                         int box_count) {
  __shared__ int sa[256], sb[256];
  for (int k = threadIdx.x; k < 4 * box_count; k += 256) box_init[k] = (k & 1) ? -3.402823466e+38f : 3.402823466e+38f;
  int carry_a = 0, carry_b = 0;
  for (int base = 0; base < nkeys; base += 256) {
    const int k = base + threadIdx.x;
    const int c = k < nkeys ? cnt[k] : 0;
    const int cp = k < nkeys - 1 ? (c + 63) & ~63 : c;
    sa[threadIdx.x] = c;
    sb[threadIdx.x] = cp;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {   // Hillis-Steele inclusive scan
      const int va = threadIdx.x >= d ? sa[threadIdx.x - d] : 0;
      const int vb = threadIdx.x >= d ? sb[threadIdx.x - d] : 0;
      __syncthreads();
      sa[threadIdx.x] += va;
      sb[threadIdx.x] += vb;
      __syncthreads();
    }
    if (k < nkeys) {
      start[k] = carry_a + sa[threadIdx.x] - c;
      slot_start[k] = carry_b + sb[threadIdx.x] - cp;
      if (pad_slots)
        for (int j = c; j < cp; j++) pad_slots[carry_b + sb[threadIdx.x] - cp + j] = -1;
    }
    carry_a += sa[255];
    carry_b += sb[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int sparse = cnt[nkeys - 1];
    counts[0] = carry_b - sparse;
    counts[1] = sparse;
    counts[2] = carry_b;
  }
  if (pad_slots && threadIdx.x >= 3 && threadIdx.x < TDR_SU_TAIL_INTS) counts[threadIdx.x] = 0;
}

__global__ __launch_bounds__(256) void su_scatter_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ vals,
                                                         int64_t n, const int* __restrict__ start,
                                                         const int* __restrict__ slot_start, int32_t* __restrict__ slots) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t k = keys[t];
  slots[slot_start[k] + ((int)t - start[k])] = vals[t];
}

// The bucket sort's scatter.  One wave per segment; it walks the segment 64 positions at a time, in order.  ctr[k] (LDS) is
// the slot of the segment's next particle of key k: slot_start[k] + the key's particles in earlier segments (su_colscan_kernel)
// to begin with.  The lanes that hold the same key find each other by a multi-split over the key's bits; a lane's slot is
// ctr[key] + the equal-key lanes below it, and the last of them moves ctr[key] on.  Segments, 64-groups and lanes are all
// visited in position order: the slot list is the one a stable sort gives.
__global__ __launch_bounds__(64) void su_rank_scatter_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ vals,
                                                             int64_t n, const int* __restrict__ seg_pre,
                                                             const int* __restrict__ slot_start, int nkeys, int bits,
                                                             int32_t* __restrict__ slots) {
  extern __shared__ int ctr[];
  const int lane = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * SU_SEG;
  uint32_t key[SU_SEG / 64];
  int32_t val[SU_SEG / 64];
#pragma unroll
  for (int it = 0; it < SU_SEG / 64; it++) {   // (all of the segment's loads in flight at once, the counters' below too)
    const int64_t t = t0 + it * 64 + lane;
    key[it] = t < n ? keys[t] : 0u;
    val[it] = t < n ? vals[t] : 0;
  }
  const int* row = seg_pre + (int64_t)blockIdx.x * nkeys;
  for (int k0 = lane; k0 < nkeys; k0 += 256) {
    int a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = k0 + 64 * u;
      a[u] = k < nkeys ? slot_start[k] : 0;
      b[u] = k < nkeys ? row[k] : 0;
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (k0 + 64 * u < nkeys) ctr[k0 + 64 * u] = a[u] + b[u];
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < SU_SEG / 64; it++) {
    const bool live = t0 + it * 64 + lane < n;
    uint64_t same = __ballot(live);
    for (int b = 0; b < bits; b++) {
      const bool one = (key[it] >> b) & 1u;
      const uint64_t ones = __ballot(one);
      same &= one ? ones : ~ones;
    }
    const int below = __popcll(same & (((uint64_t)1 << lane) - 1)), all = __popcll(same);
    int at = 0;
    if (live) {
      at = ctr[key[it]];
      slots[at + below] = val[it];
    }
    __syncthreads();   // (one wave: every lane has read its counter)
    if (live && below == all - 1) ctr[key[it]] = at + all;
    __syncthreads();
  }
}

// LDS of the scoring kernel, ONE object so that the dictionary sits at LDS address 0 (the assembly loop reads it there)
struct SuLds {
  uint32_t dict[TDR_CMAP_MAX_DICT];   // integer dictionary
  uint32_t bits[SU_BOX_WORDS];   // the staged known mask: rows rlo..rhi of words wlo..whi of the map's mask
  int box[4];
};

// lane = particle; every wave holds particles of ONE heading bin (see the file comment).  grid.y = a row of su_tail_plan:
// a group of a.group consecutive range rings (score_group_rings: a multiple of 4, nr a multiple of 4) and all of its sectors,
// or — the rows dispatched last — a part of them; samples visited ray-major like
// score_polar_kernel: direction i ascending, the group's rings in steps of 4 consecutive cells along the ray.  The
// directions are walked in SU_NSECT sectors; for each the workgroup stages the known mask of the cells its windows can reach.
TDR_TL_BUFFER(g_timeline_su, tdr_debug_read_timeline_su)   // (diagnostic build only: tdr_score_dev.h)
template <int NV4, bool KSLOT, bool USCALE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6, 8))) void score_polar_su_kernel(SuArgs a) {
  constexpr int RF = 4 * NV4;
  constexpr int ND = CmapShape<RF, KSLOT>::ND, CW = CmapShape<RF, KSLOT>::CW;
  constexpr bool ASM_LOOP = CW == 2 && ND == 6;   // tdr_score_su_asm.h: two-dword records
  __shared__ SuLds lds;
  if (int_form_off(a.inexact)) return;   // (uniform) no integer form of this scan / map: score_polar_kernel does the launch in floats
  for (int t = threadIdx.x; t < a.dict_n; t += 256) lds.dict[t] = a.dict_int[t];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // provably wave-uniform
  const int64_t nsl = (int64_t)__builtin_amdgcn_readfirstlane(*a.nslots);
  if ((int64_t)blockIdx.x * 256 >= nsl) return;   // the whole workgroup is beyond the slots in use (uniform)
  TDR_TL_BEGIN(g_timeline_su)
  const int64_t base = ((int64_t)blockIdx.x * 4 + wave) * 64;
  const bool active = base < nsl;                 // wave-uniform; an idle wave still keeps the barriers below
  const int32_t sp = active ? a.slots[base + lane] : -1;
  const int32_t p0 = a.slots[active ? base : (int64_t)blockIdx.x * 256];   // a batch's first slot is never padding
  const int64_t p = sp >= 0 ? sp : p0;
  const float scale = a.st[TDR_ST_SCALE * a.cap + p];
  const float cx = a.st[TDR_ST_DX * a.cap + p] * scale + a.st[TDR_ST_INIT_X * a.cap + p];  // state_particle.cpp:161
  const float cy = a.st[TDR_ST_DY * a.cap + p] * scale + a.st[TDR_ST_INIT_Y * a.cap + p];  // :162
  const float off0 = cy / a.resolution;  // top_down_map_polar.cpp:29
  const float off1 = cx / a.resolution;  // :30
  const int shift = __builtin_amdgcn_readfirstlane(rot_shift_dev(a.st[TDR_ST_THETA * a.cap + p], a.nb));
  const int nb = a.nb, G = a.group;
  int rgroup = 0, sect0 = 0, sect1 = SU_NSECT;   // this row's ring group and sectors (wave-uniform: scalar arithmetic)
  su_tail_plan(a.nchunks, a.tail_k, a.tail_q, (int)blockIdx.y, &rgroup, &sect0, &sect1);
  const int j0 = rgroup * G, gn = min(a.nr - j0, G);
  const float rmaxf = (float)a.rows, cmaxf = (float)a.cols;
  const int ckcol = a.ctiles_r * 128 - 16 * CW;   // cmap_offset
  const int pkcol = a.pkcol;                      // plane_offset; its constant comes with the descriptor
  // the record constant of a bin for the steps that read records: dword (c / 3) of class c = code - 1 alone (c < 11: c / 3
  // == c * 11 >> 5), dword 0 otherwise (wave-uniform: scalar arithmetic)
  const uint32_t ckconst = (uint32_t)(a.ctiles_r * 128 + 128);
  auto su_rec_const = [&](uint32_t cd) -> uint32_t {
    return cd != 0 && cd < SU_CODE_PAD ? ckconst + 4u * (((cd - 1u) * 11u) >> 5) : ckconst;
  };
  typedef const float __attribute__((address_space(4))) * tdr_const_f;
  typedef const uint32_t __attribute__((address_space(4))) * tdr_const_u;
  const tdr_const_f tbase = (tdr_const_f)a.tab_su + (int64_t)rgroup * nb * G * 2;
  const tdr_const_u dbase = (tdr_const_u)a.desc + (int64_t)rgroup * nb * G * 4;
  const tdr_const_f bbase = (tdr_const_f)a.bbox + (int64_t)rgroup * SU_NSECT * 4;
  const tdr_const_f scanc = (tdr_const_f)a.scan_pk;
  const uint32_t* __restrict__ crec = a.crec;
  const uint32_t* __restrict__ kmask = a.kmask;
  const unsigned lds_base = (unsigned)(uintptr_t)&lds;                // LDS byte address of the dictionary ...
  const unsigned lbits_lds = (unsigned)(uintptr_t)&lds.bits[0];      // ... and of the staged mask

  const tdr_v2f offv = {off0, off1};
  // plain, compiler-tracked loads: a word of the staged mask at an LDS byte address, bytes of the compact map at a byte offset
  typedef const uint32_t __attribute__((address_space(3))) * tdr_lds_u;
  auto lds_word = [](unsigned byte_addr) -> uint32_t { return *reinterpret_cast<tdr_lds_u>((uintptr_t)byte_addr); };
  const char* __restrict__ crecb = reinterpret_cast<const char*>(a.crec);
  auto map_dword = [&](unsigned off) -> uint32_t { return *reinterpret_cast<const uint32_t*>(crecb + off); };
  auto map_ushort = [&](unsigned off) -> uint32_t { return *reinterpret_cast<const uint16_t*>(crecb + off); };
  const bool weird = !(fabsf(off0) <= 1e9f) || !(fabsf(off1) <= 1e9f) || (!USCALE && !(fabsf(scale * a.res) <= 1e9f));
  auto field = [&](const uint32_t (&w)[CW], int k) { return int_record_field(lds.dict, w[k / 3], k); };   // distance k of a record

  // integer sums (see the file comment: exact, so independent of the order and of the kernel that forms them)
  uint64_t acc[ND];
#pragma unroll
  for (int k = 0; k < ND; k++) acc[k] = 0;
  uint32_t norm = 0;
  uint32_t known = 0;
  uint32_t n_hand = 0, n_listed = 0;   // (profiling, wave-uniform) steps the assembly loop handed back, bins the list pass scored

  // A bin that holds class cd - 1 only (cd is wave-uniform): int_add_class with the value looked up from the dword the class
  // lives in (cpp_step) or from the 2-byte cell of the class's plane.
  auto single_class = [&](uint32_t cd, uint32_t v, uint32_t ww) { int_add_class(acc, cd, v, int_record_field(lds.dict, ww, (int)cd - 1)); };
  auto single_class_plane = [&](uint32_t cd, uint32_t v, uint32_t cell) { int_add_class(acc, cd, v, int_dict_at(lds.dict, cell)); };
  // far_steps keeps the switch it had, the lookup inside every case with the field's shift a constant: with the lookup in
  // front of the switch score_polar_su_kernel<3, true, true> spills 8 bytes more (292 against 284; the kernel is pinned at
  // 80 registers)
  auto single_class_far = [&](uint32_t cd, uint32_t v, uint32_t ww) {
    switch (cd) {
#define SU_CASE(K)                                                                                 \
  case K + 1:                                                                                      \
    if constexpr (K < ND) {                                                                        \
      const uint32_t m = int_record_field(lds.dict, ww, K < ND ? K : 0);                           \
      asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc[K < ND ? K : 0]) : "s"(v), "v"(m) : "vcc"); \
    }                                                                                              \
    break;
      SU_CASE(0) SU_CASE(1) SU_CASE(2) SU_CASE(3) SU_CASE(4) SU_CASE(5)
      SU_CASE(6) SU_CASE(7) SU_CASE(8) SU_CASE(9) SU_CASE(10)
#undef SU_CASE
      default: break;
    }
  };
  // a bin with several classes (or a non-finite value in play): the whole record against the packed scan record
  auto full_bin = [&](uint32_t cd, uint32_t v, const uint32_t (&wr)[CW], int kbit, int64_t bin) {
    const tdr_const_f S = scanc + bin * RF;
    norm += v & (0u - (uint32_t)kbit);
#pragma unroll
    for (int k = 0; k < ND; k++) {
      const float sk = S[k];
      if (sk != 0.f) acc[k] += (uint64_t)(uint32_t)sk * (uint64_t)field(wr, k);
    }
  };
  // cell of one sample (top_down_map_polar.cpp:28-31)
  auto cell = [&](float tx, float ty, int& ri, int& ci) {
    tdr_v2f pv = {tx, ty};
    if constexpr (!USCALE) pv = (pv * scale) * a.res;  // top_down_map_polar.cpp:28
    int_cell(pv + offv, rmaxf, cmaxf, ri, ci);          // :29-31
  };

  // One step with the known mask staged in LDS: the 4 samples (i, j0 + jj .. jj + 3), paired with scan row r.  Known bits
  // come from word ri * krow4 + (ci >> 5) * 4 + kconst of the staged mask.  listed: the caller's list pass adds the bins
  // with several classes (SU_CODE_FULL) — they are empty bins here.
  auto cpp_step = [&](int i, int r, int jj, int krow4, int kconst, bool listed) {
    const tdr_const_f T = tbase + ((int64_t)i * G + jj) * 2;
    const tdr_const_u D = dbase + ((int64_t)r * G + jj) * 4;
    uint32_t val[4];
    uint32_t code[4], pad[4];
    uint32_t w[4], bits[4];
    int cis[4];
    unsigned offs[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      code[u] = D[4 * u];
      // A ring the image does not have (SU_CODE_PAD) goes through the step like an EMPTY bin — score_prep_kernel gives it the offset of
      // the direction's last real ring, so its mask lookup stays inside the staged box — and is masked out of the known
      // count below.
      pad[u] = code[u] == SU_CODE_PAD ? 0u : 0xFFFFFFFFu;
      code[u] = code[u] == SU_CODE_PAD || (listed && code[u] == SU_CODE_FULL) ? 0u : code[u];
      val[u] = D[4 * u + 1];
      const uint32_t ckc = su_rec_const(code[u]);
      int ri, ci;
      cell(T[2 * u], T[2 * u + 1], ri, ci);
      cis[u] = ci;
      bits[u] = lds_word(staged_mask_addr(ri, ci, krow4, kconst));
      w[u] = 0;
      offs[u] = 0;
      if (code[u] != 0) {   // wave-uniform: only a non-empty bin needs its record — one dword of it
        offs[u] = cmap_offset_sconst<CW>(ri, ci, ckcol, ckc);
        w[u] = map_dword(offs[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint32_t cd = code[u];
      const int kmsk = staged_mask_bit(bits[u], cis[u]);   // 0 / -1: the cell's known bit
      known -= (uint32_t)kmsk & pad[u];
      if (cd != 0) {   // wave-uniform
        if (cd < SU_CODE_FULL_ALL) {
          // the bin's count x known (state_particle.cpp:141-142)
          norm += (uint32_t)kmsk & val[u];
          single_class(cd, val[u], w[u]);
        } else {
          uint32_t wr[CW];
          wr[0] = w[u];
#pragma unroll
          for (int d = 1; d < CW; d++)
            wr[d] = map_dword(offs[u] + 4u * d);
          full_bin(cd, val[u], wr, kmsk & 1, (int64_t)(j0 + jj + u) * nb + r);
        }
      }
    }
  };
  // The same step when none of its bins holds several classes (the descriptor's flag, wave-uniform): a bin with a class
  // fetches the 2-byte cell of that class's PLANE (8 x 8-cell tiles) instead of a record dword (4 x 4-cell tiles) — a third
  // of the lines for a wave whose particles lie a few cells apart.  The assembly loop does the same.
  auto cpp_step_plane = [&](int i, int r, int jj, int krow4, int kconst) {
    const tdr_const_f T = tbase + ((int64_t)i * G + jj) * 2;
    const tdr_const_u D = dbase + ((int64_t)r * G + jj) * 4;
    uint32_t val[4];
    uint32_t code[4], pad[4];
    uint32_t w[4], bits[4];
    int cis[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      code[u] = D[4 * u];
      pad[u] = code[u] == SU_CODE_PAD ? 0u : 0xFFFFFFFFu;   // (see cpp_step)
      code[u] = code[u] == SU_CODE_PAD ? 0u : code[u];
      val[u] = D[4 * u + 1];
      const uint32_t pkc = D[4 * u + 2];
      int ri, ci;
      cell(T[2 * u], T[2 * u + 1], ri, ci);
      cis[u] = ci;
      bits[u] = lds_word(staged_mask_addr(ri, ci, krow4, kconst));
      w[u] = 0;
      if (code[u] != 0) {   // wave-uniform
        w[u] = map_ushort(plane_offset_sconst(ri, ci, pkcol, pkc));
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int kmsk = staged_mask_bit(bits[u], cis[u]);   // 0 / -1: the cell's known bit
      known -= (uint32_t)kmsk & pad[u];
      if (code[u] != 0) {   // wave-uniform
        norm += (uint32_t)kmsk & val[u];   // the bin's count x known (state_particle.cpp:141-142)
        single_class_plane(code[u], val[u], w[u]);
      }
    }
  };
  // NS consecutive steps of a sector (step k = direction i0 + k / spd, rings (k % spd) * 4 ..) WITHOUT the staged mask:
  // the windows of the workgroup's particles are too far apart to stage (scattered particles: su_key_kernel gives them
  // waves of their own).  Every gather of such a wave misses the caches, so the wave is bound by how many it keeps in
  // flight: the gathers of all 4 NS samples are requested before the first is used — ONE per sample: the mask word of an
  // empty bin (the global mask: 32 x 32-cell tiles, a cache line each), the record dword of a bin with a class (its bit 0 is
  // the known bit: every dword of a compact record carries it, tdr_cmap.hip).
  auto far_steps = [&](auto nsteps_c, int i, int jj) {
    constexpr int NS = decltype(nsteps_c)::value;
    uint32_t w[4 * NS];
    uint32_t cbits[(4 * NS + 5) / 6];   // the column's low 5 bits of every sample (the bit of its mask word), six per word
#pragma unroll
    for (int q = 0; q < (4 * NS + 5) / 6; q++) cbits[q] = 0;
    const int mtrb = a.kcolw * 4, mconst = (int)a.kmask_off + a.kcolw * 4 + 128;   // kmask_offset
    int ii = i, jx = jj;
#pragma unroll
    for (int d = 0; d < NS; d++) {
      int r = ii + shift;
      r -= r >= nb ? nb : 0;
      const tdr_const_f T = tbase + ((int64_t)ii * G + jx) * 2;
      const tdr_const_u D = dbase + ((int64_t)r * G + jx) * 4;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        int ri, ci;
        cell(T[2 * u], T[2 * u + 1], ri, ci);
        unsigned off;
        const int sidx = 4 * d + u;   // (d, u are unrolled: constants after unrolling)
        if (D[4 * u] == 0 || D[4 * u] == SU_CODE_PAD) {   // wave-uniform: an empty bin (or no ring at all) reads the cell's mask word
          off = kmask_offset(ri, ci, mtrb, mconst);
          cbits[sidx / 6] |= (uint32_t)(ci & 31) << (5 * (sidx % 6));
        } else {               // a single class: the dword it lives in; several classes: dword 0
          off = cmap_offset_sconst<CW>(ri, ci, ckcol, su_rec_const(D[4 * u]));
        }
        w[4 * d + u] = map_dword(off);   // (all 4 NS requests are issued before the first value is used below)
      }
      jx += 4;
      if (jx >= ((gn + 3) & ~3)) { jx = 0; ii++; }
    }
    ii = i; jx = jj;
#pragma unroll
    for (int d = 0; d < NS; d++) {
      int r = ii + shift;
      r -= r >= nb ? nb : 0;
      const tdr_const_u D = dbase + ((int64_t)r * G + jx) * 4;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint32_t ww = w[4 * d + u];
        const uint32_t cdr = D[4 * u];
        const uint32_t cd = cdr == SU_CODE_PAD ? 0u : cdr;   // a ring the image does not have: an empty bin that counts nothing
        const int sidx = 4 * d + u;
        const uint32_t kb = cd == 0 ? (ww >> ((cbits[sidx / 6] >> (5 * (sidx % 6))) & 31u)) & 1u : (ww & 1u);
        known += cdr == SU_CODE_PAD ? 0u : kb;
        if (cd != 0) {   // wave-uniform
          const uint32_t v = D[4 * u + 1];
          if (cd < SU_CODE_FULL_ALL) {
            norm += (0u - kb) & v;
            single_class_far(cd, v, ww);
          } else {
            // the other dwords of the record: its offset again (rare: ~1 % of the bins hold several classes)
            // (behind a barrier the optimiser cannot see through: it would keep the coordinates of all 4 NS samples
            // alive from the request pass for the sake of this branch — 8 NS registers, a wave per SIMD less)
            int iq = ii;
            asm volatile("" : "+s"(iq));
            const tdr_const_f T = tbase + ((int64_t)iq * G + jx) * 2;
            int ri, ci;
            cell(T[2 * u], T[2 * u + 1], ri, ci);
            const unsigned off = cmap_offset<CW, (CW == 1 ? 3 : (CW == 2 ? 2 : 1))>(ri, ci, ckcol, a.ctiles_r * 128 + 128);
            uint32_t wr[CW];
            wr[0] = ww;
#pragma unroll
            for (int q = 1; q < CW; q++)
              wr[q] = map_dword(off + 4u * q);
            full_bin(cd, v, wr, (int)kb, (int64_t)(j0 + jx + u) * nb + r);
          }
        }
      }
      jx += 4;
      if (jx >= ((gn + 3) & ~3)) { jx = 0; ii++; }
    }
  };
  constexpr int FAR_DEPTH = 4;   // steps (of 4 samples) a wave of the memory-bound path keeps in flight
  auto far_sector = [&](int i0, int i1) {
    const int gn4 = (gn + 3) & ~3;   // steps cover whole fours of rings; what lies behind the last ring is SU_CODE_PAD
    const int spd = gn4 >> 2, total = (i1 - i0) * spd;
    int i = i0, jj = 0, k = 0;
    auto advance = [&](int steps) {
      jj += 4 * steps;
      while (jj >= gn4) { jj -= gn4; i++; }
    };
    for (; k + FAR_DEPTH <= total; k += FAR_DEPTH) {
      far_steps(std::integral_constant<int, FAR_DEPTH>{}, i, jj);
      advance(FAR_DEPTH);
    }
    for (; k < total; k++) {
      far_steps(std::integral_constant<int, 1>{}, i, jj);
      advance(1);
    }
  };
  // One sector of directions [i0, i1) with the known mask staged in LDS
  // (inside: every cell the workgroup's windows can reach in this sector lies inside the map — the clamp into the guard
  // ring is the identity and the loop without it runs; allknown: every staged mask word is all ones — every sample is a
  // known cell and the loop without clamp and without mask lookups runs)
  auto run_sector = [&](int i0, int i1, int krow4, int kconst, bool inside, bool allknown) {
    if constexpr (ASM_LOOP) {
      if (gn == G && lds_base == 0 && (G == 4 || G == 8 || G == 16)) {
        // the steps of the sector as one stream: step k reads T at byte k * 32 from its start and D at byte k * 64 from the
        // start of scan row (i0 + shift) mod nb, wrapping to row 0; the loop hands a step back (nleft >= 0 on exit), cpp_step
        // does that one, and the loop goes on behind it.  Handed back: without the list pass below every step that holds a
        // bin with several classes; with it only a step with a bin where a non-finite value is in play (SU_CODE_FULL_ALL,
        // which an integer-form launch never meets) — the others run in the loop's second copy of its bodies, in which a
        // bin with several classes is an empty bin
        const int spd = G / 4;                                // steps per direction
        int r0 = i0 + shift;
        r0 -= r0 >= nb ? nb : 0;
        // (readfirstlane: values the compiler cannot prove wave-uniform must not reach an "s" operand)
        uint32_t toff = __builtin_amdgcn_readfirstlane((uint32_t)i0 * (uint32_t)G * 8u);
        uint32_t doff = __builtin_amdgcn_readfirstlane((uint32_t)r0 * (uint32_t)G * 16u);
        uint32_t nleft = __builtin_amdgcn_readfirstlane((uint32_t)((i1 - i0) * spd - 1));
        uint32_t wleft = __builtin_amdgcn_readfirstlane((uint32_t)((nb - r0) * spd - 1));
        const uint32_t wrapm1 = __builtin_amdgcn_readfirstlane((uint32_t)(nb * spd - 1));
        const int kconst_s = __builtin_amdgcn_readfirstlane(kconst);
        const uint64_t half2 = 0x3EFFFFFF3EFFFFFFull;         // {0.49999997f, 0.49999997f}
        // int -> float is a vector instruction: bring the map's limits back to scalar registers
        const float rmax_s = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(rmaxf)));
        const float cmax_s = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(cmaxf)));
        const tdr_v2f scale2 = {scale, scale};
        const uint64_t res2 = (uint64_t)__float_as_uint(a.res) * 0x100000001ull;   // {res, res} in an SGPR pair
        // the loop's operand for wrapm1 carries, in bit 31, whether bins with several classes are empty to the loop and listed
        // below (an operand of its own would be one more scalar register held across the loop)
        const bool flist = a.full_mask != nullptr;
        const uint32_t wrapl = __builtin_amdgcn_readfirstlane(wrapm1 | (flist ? 0x80000000u : 0u));
        while (nleft != 0xFFFFFFFFu) {
#define SU_ASM_OPERANDS                                                                                               \
          /* the accumulators (64-bit) are TIED to v[32:43]: the loop reaches them by VGPR-relative indexing */                \
          : [a0] "+{v[32:33]}"(acc[0]), [a1] "+{v[34:35]}"(acc[1]), [a2] "+{v[36:37]}"(acc[2]), [a3] "+{v[38:39]}"(acc[3]),    \
            [a4] "+{v[40:41]}"(acc[4]), [a5] "+{v[42:43]}"(acc[ND > 5 ? 5 : 0]), [norm] "+v"(norm), [known] "+v"(known),       \
            [toff] "+v"(toff), [doff] "+v"(doff),                                                                             \
            [nleft] "+v"(nleft), [wleft] "+v"(wleft)                                                                   \
          : [offv] "v"(offv), [krow4] "v"(krow4), [pkcol] "v"(pkcol), [tb] "s"(tbase), [db] "s"(dbase),              \
            [rmax] "s"(rmax_s), [cmax] "s"(cmax_s), [half] "s"(half2), [kconst] "s"(kconst_s), [crec] "s"(crec),           \
            [wrapl] "s"(wrapl), [scale2] "v"(scale2), [res2] "s"(res2)                                                 \
          : SU_ASM_CLOBBERS
          if (allknown) {   // wave-uniform
            if constexpr (USCALE) asm volatile(SU_ASM_US_ALLKNOWN SU_ASM_OPERANDS);
            else asm volatile(SU_ASM_PS_ALLKNOWN SU_ASM_OPERANDS);
          } else if (inside) {
            if constexpr (USCALE) asm volatile(SU_ASM_US_NOCLAMP SU_ASM_OPERANDS);
            else asm volatile(SU_ASM_PS_NOCLAMP SU_ASM_OPERANDS);
          } else {
            if constexpr (USCALE) asm volatile(SU_ASM_US SU_ASM_OPERANDS);
            else asm volatile(SU_ASM_PS SU_ASM_OPERANDS);
          }
#undef SU_ASM_OPERANDS
          // (the compiler takes the outputs of an asm statement for divergent)
          toff = __builtin_amdgcn_readfirstlane(toff); doff = __builtin_amdgcn_readfirstlane(doff);
          nleft = __builtin_amdgcn_readfirstlane(nleft); wleft = __builtin_amdgcn_readfirstlane(wleft);
          if (nleft == 0xFFFFFFFFu) break;
          // the step the loop stopped in front of
          // (no division here: it would run on the vector unit and drag the loop's scalar state there with it)
          const int k = (i1 - i0) * spd - 1 - (int)nleft, lsp = G == 4 ? 0 : (G == 8 ? 1 : 2);
          const int i = i0 + (k >> lsp), jj = (k & (spd - 1)) * 4;
          int r = i + shift;
          r -= r >= nb ? nb : 0;
          cpp_step(i, r, jj, krow4, kconst, flist);
          n_hand++;
          toff += 32u;
          doff += 64u;
          if (wleft == 0) { doff = 0; wleft = wrapm1; } else wleft--;
          nleft--;   // 0 -> 0xFFFFFFFF: the sector is done
          toff = __builtin_amdgcn_readfirstlane(toff); doff = __builtin_amdgcn_readfirstlane(doff);
          nleft = __builtin_amdgcn_readfirstlane(nleft); wleft = __builtin_amdgcn_readfirstlane(wleft);
        }
        // The sector's bins with several classes — empty to the loop above, which has counted their known bits.  The mask
        // words of scan rows r0 .. r0 + (i1 - i0) - 1 (stored twice over: no wrap) name them; each is scored from the class
        // planes like the loop's single-class bins, one 2-byte gather per class present.  ~1 % of a LiDAR scan's bins; the
        // sums are exact integers, so adding them here instead of in ray order changes no bit.
        if (flist) {   // (uniform)
          const tdr_const_u fm = (tdr_const_u)a.full_mask + ((int64_t)rgroup * 2 * nb + r0);
          for (int k = 0; k < i1 - i0; k++) {
            uint32_t wv = fm[k];   // (scalar load: wave-uniform)
            if (wv == 0) continue;
            const int i = i0 + k;
            int r = r0 + k;
            r -= r >= nb ? nb : 0;
            do {
              const int jj = __builtin_ctz(wv);
              wv &= wv - 1u;
              n_listed++;
              const tdr_const_f T = tbase + ((int64_t)i * G + jj) * 2;
              const uint32_t total = dbase[((int64_t)r * G + jj) * 4 + 1];
              int ri, ci;
              cell(T[0], T[1], ri, ci);
              int kmsk = -1;   // 0 / -1: the cell's known bit
              if (!allknown) {
                kmsk = staged_mask_bit(lds_word(staged_mask_addr(ri, ci, krow4, kconst_s)), ci);
              }
              norm += (uint32_t)kmsk & total;   // the bin's count x known (state_particle.cpp:141-142)
              const tdr_const_f S = scanc + ((int64_t)(j0 + jj) * nb + r) * RF;
#pragma unroll
              for (int c = 0; c < ND; c++) {
                const float sc = c < a.ncls ? S[c] : 0.f;
                if (sc != 0.f) {   // wave-uniform
                  const uint32_t pc = map_ushort(plane_offset(ri, ci, pkcol, (int)(a.pbase + (uint32_t)c * a.plane_bytes)));
                  acc[c] += (uint64_t)(uint32_t)sc * (uint64_t)int_dict_at(lds.dict, pc);
                }
              }
            } while (wv != 0);
          }
        }
        return;
      }
    }
    for (int i = i0; i < i1; i++) {
      int r = i + shift;
      r -= r >= nb ? nb : 0;
      for (int jj = 0; jj < gn; jj += 4) {
        // (the flag sits on the step's first bin: score_prep_kernel)
        if (dbase[((int64_t)r * G + jj) * 4 + 3] >> 31) cpp_step(i, r, jj, krow4, kconst, false);
        else cpp_step_plane(i, r, jj, krow4, kconst);
      }
    }
  };

  for (int sect = sect0; sect < sect1; sect++) {
    const int i0 = (int)((int64_t)sect * nb / SU_NSECT), i1 = (int)((int64_t)(sect + 1) * nb / SU_NSECT);
    // cells this lane's samples of the sector can fall on: rounding is monotone, so the box of the offsets carries over
    float a0 = bbase[4 * sect], b0 = bbase[4 * sect + 1], a1 = bbase[4 * sect + 2], b1 = bbase[4 * sect + 3];
    if constexpr (!USCALE) {
      const float x0 = (a0 * scale) * a.res, y0 = (b0 * scale) * a.res, x1 = (a1 * scale) * a.res, y1 = (b1 * scale) * a.res;
      a0 = fminf(x0, y0); b0 = fmaxf(x0, y0); a1 = fminf(x1, y1); b1 = fmaxf(x1, y1);
    }
    int rl = (int)fminf(fmaxf(floorf(a0 + off0) - 1.f, -1.f), rmaxf), rh = (int)fminf(fmaxf(ceilf(b0 + off0) + 1.f, -1.f), rmaxf);
    int cl = (int)fminf(fmaxf(floorf(a1 + off1) - 1.f, -1.f), cmaxf), ch = (int)fminf(fmaxf(ceilf(b1 + off1) + 1.f, -1.f), cmaxf);
    if (weird) { rl = -1; rh = a.rows; cl = -1; ch = a.cols; }
    if (!active) { rl = 0x7FFFFFFF; rh = -0x7FFFFFFF; cl = 0x7FFFFFFF; ch = -0x7FFFFFFF; }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      rl = min(rl, __shfl_xor(rl, d)); rh = max(rh, __shfl_xor(rh, d));
      cl = min(cl, __shfl_xor(cl, d)); ch = max(ch, __shfl_xor(ch, d));
    }
    __syncthreads();   // the previous sector's lookups are done (and, the first time, the dictionary is staged)
    if (threadIdx.x == 0) { lds.box[0] = 0x7FFFFFFF; lds.box[1] = -0x7FFFFFFF; lds.box[2] = 0x7FFFFFFF; lds.box[3] = -0x7FFFFFFF; }
    __syncthreads();
    if (lane == 0 && active) {
      atomicMin(&lds.box[0], rl); atomicMax(&lds.box[1], rh); atomicMin(&lds.box[2], cl); atomicMax(&lds.box[3], ch);
    }
    __syncthreads();
    const int rlo = __builtin_amdgcn_readfirstlane(lds.box[0]), rhi = __builtin_amdgcn_readfirstlane(lds.box[1]);   // mask rows
    const int wlo = (__builtin_amdgcn_readfirstlane(lds.box[2]) >> 5) + 1;                                            // mask words
    const int whi = (__builtin_amdgcn_readfirstlane(lds.box[3]) >> 5) + 1;
    const int H = rhi - rlo + 1, Wb = whi - wlo + 1;
    const bool fits = (int64_t)H * Wb <= SU_BOX_WORDS;   // uniform over the workgroup
    uint32_t every = 0xFFFFFFFFu;   // AND of the words this thread staged
    if (fits) {
      const int total = H * Wb;
      // (row fastest: consecutive threads read consecutive words of one tile column of the mask, kmask_offset)
      for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int wc = idx / H, row = idx - wc * H;
        const uint32_t wv = kmask[(int64_t)(wlo + wc) * a.kcolw + (rlo + row + 32)];
        lds.bits[row * Wb + wc] = wv;
        every &= wv;
      }
    }
    const bool allknown = __syncthreads_and(fits && every == 0xFFFFFFFFu);   // (cells outside the map are unknown)
    if (active) {
      const bool inside = rlo >= 0 && rhi < a.rows && __builtin_amdgcn_readfirstlane(lds.box[2]) >= 0 &&
                          __builtin_amdgcn_readfirstlane(lds.box[3]) < a.cols;
      // one call of the sector's loop (two would double the assembly text in the kernel), its box chosen here
      int box_krow4 = Wb * 4, box_kconst = (int)lbits_lds + (1 - wlo - rlo * Wb) * 4;
      int box_ok = fits ? 1 : 0, box_inside = inside ? 1 : 0, box_allknown = allknown ? 1 : 0;
      if (!fits) {
        // The workgroup's windows do not fit one box — its waves belong to different clusters or heading bins (config 5:
        // 8 clusters x 40 headings, more than half of the sectors).  A wave's own 64 particles still lie together: a box
        // per wave in a quarter of the staging area each (rl .. ch: the wave's own bounds after the shuffles above;
        // nothing here crosses waves, so no workgroup barrier: a wave's LDS operations execute in order).
        // score_cart_su_kernel has the same box per segment, in its own text.  One function behind both (bounds and wave
        // reduction, staging with the Cartesian loop) took this kernel's scratch away but config 5's step measured 12.76 ms
        // against 12.68 at a spread of 0.07; the bounds function alone made three instantiations spill more
        // (profiles/int_form_shared_timing_v1.txt "first form", profiles/int_form_shared_kernels_v1.txt).
        const int wrl = __builtin_amdgcn_readfirstlane(rl), wrh = __builtin_amdgcn_readfirstlane(rh);
        const int wcl = __builtin_amdgcn_readfirstlane(cl), wch = __builtin_amdgcn_readfirstlane(ch);
        const int wl = (wcl >> 5) + 1, wh = (wch >> 5) + 1;
        const int Hw = wrh - wrl + 1, Wbw = wh - wl + 1;
        if ((int64_t)Hw * Wbw <= SU_BOX_WORDS / 4) {
          uint32_t* const mine = lds.bits + wave * (SU_BOX_WORDS / 4);
          uint32_t ev = 0xFFFFFFFFu;
          const int total = Hw * Wbw;
          for (int idx = lane; idx < total; idx += 64) {
            const int wc = idx / Hw, row = idx - wc * Hw;
            const uint32_t wv = kmask[(int64_t)(wl + wc) * a.kcolw + (wrl + row + 32)];
            mine[row * Wbw + wc] = wv;
            ev &= wv;
          }
          // the wave reads what its lanes just wrote — through the assembly loop's ds_read as well: order the stores in front
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          box_ok = 1;
          box_krow4 = Wbw * 4;
          box_kconst = (int)lbits_lds + wave * (SU_BOX_WORDS / 4) * 4 + (1 - wl - wrl * Wbw) * 4;
          box_inside = (wrl >= 0 && wrh < a.rows && wcl >= 0 && wch < a.cols) ? 1 : 0;
          box_allknown = __all(ev == 0xFFFFFFFFu) ? 1 : 0;
        }
      }
      // (readfirstlane: the loop's variants are chosen by these, and the compiler must see them wave-uniform)
      box_ok = __builtin_amdgcn_readfirstlane(box_ok);
      box_inside = __builtin_amdgcn_readfirstlane(box_inside);
      box_allknown = __builtin_amdgcn_readfirstlane(box_allknown);
      box_krow4 = __builtin_amdgcn_readfirstlane(box_krow4);
      box_kconst = __builtin_amdgcn_readfirstlane(box_kconst);
      if (a.stats && lane == 0)   // [0..2] the workgroup's box: all known / inside / general; [3..5] the wave's own; [6] far
        atomicAdd(&a.stats[!box_ok ? 6 : ((fits ? 0 : 3) + (box_allknown ? 0 : (box_inside ? 1 : 2)))], 1u);
      if (box_ok) run_sector(i0, i1, box_krow4, box_kconst, box_inside != 0, box_allknown != 0);
      else far_sector(i0, i1);
    }
  }
  if (active) {
    const int64_t slot = base + lane;
    int_add_sums(a.part, a.npad, slot, a.ncls, acc, norm, known);
    if (a.list_stats && lane == 0) {   // (profiling: one atomic per wave and counter)
      if (n_hand) atomicAdd(&a.list_stats[0], n_hand);
      if (n_listed) atomicAdd(&a.list_stats[1], n_listed);
    }
  }
  TDR_TL_END(g_timeline_su)
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// The span (TdrConfig::su_span): fixed by the config call, or — the default — tuned while running.
// Which span is fastest depends on the particle set (how far the same-heading neighbours of a moderately dense particle
// lie apart): measured on MI355X, config 2 wants 8 (7.00 against 7.29 ms at 24), config 5 wants 16 (15.9 against 17.7 at 8),
// a cluster with a single heading wants 24 or more (4.6 against 6.9 ms at 8).
namespace {
// (measured on MI355X with the ray-mapped kernel taking the scattered share, ms per scoring call at 8 / 16 / 24 / 40 cells:
// config 2's mix 5.88 / 5.55 / 5.51 / 5.67, uniform particles 10.7 / 11.0 / - / 11.7, a converged filter 3.1 / 3.05 / - / 3.0)
// (round 4, later: with the table's factors the ray-mapped kernel scores 100 000 uniform particles in 7.6 ms, the mixed
// launch at 8 cells in 8.4 — hence a candidate that sends all but the densest cores to it;
// profiles/r04_time_int_form_c2_v2.txt)
constexpr float kSpanCand[] = {2.f, 8.f, 16.f, 24.f, 40.f};
constexpr int kSpanCands = (int)(sizeof(kSpanCand) / sizeof(kSpanCand[0]));
constexpr int kSpanTrials = 2;        // timed calls per candidate: the faster one counts (a single call is noisy)
constexpr int kSpanSkip = 30;         // calls of a new shape before the first trial (first-use allocations, cold caches, and
                                      // a short run — a benchmark of a few dozen steps — is not worth ten trial calls)
constexpr int kSpanRetune = 4000;     // launches between two trials
}  // namespace
float tdr_su_span_begin(SpanTuner* t, int64_t shape, hipStream_t s) {
  const TdrConfig& cfg = tdr_cfg();
  if (cfg.su_span_fixed || !t) return cfg.su_span;
  if (!t->e0 && (hipEventCreate(&t->e0) != hipSuccess || hipEventCreate(&t->e1) != hipSuccess)) return cfg.su_span;
  if (shape != t->shape) { t->shape = shape; t->phase = -kSpanSkip; t->trial = 0; t->best_ms = 3.0e38f; t->pending = false; t->best = t->round_best = cfg.su_span; }
  if (t->pending) {   // the candidate timed by an earlier launch — if its events are not through yet, ask again next time
    if (hipEventQuery(t->e1) != hipSuccess) return t->best;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t->e0, t->e1) == hipSuccess && ms > 0.f && ms < t->best_ms) {
      t->best_ms = ms;
      t->round_best = kSpanCand[t->phase];
    }
    t->pending = false;
    if (++t->trial >= kSpanTrials) { t->trial = 0; t->phase++; }
    // Only a finished round changes the span in use.  (A caller that runs ahead of the device — a benchmark loop — makes
    // hundreds of calls while one trial's events are pending: they must not run at the first candidate's span just because
    // it is the only one timed so far.  Seen with the candidate of 2 cells in front: 5.3 -> 5.95 ms per config-2 step.)
    if (t->phase >= kSpanCands) { t->settled_launches = 0; t->best = t->round_best; }
  }
  if (t->phase < 0) { t->phase++; return t->best; }
  if (t->phase >= kSpanCands) {
    if (++t->settled_launches < kSpanRetune) return t->best;
    t->phase = 0;   // try them again: the particle set changes as the filter converges
    t->best_ms = 3.0e38f;
    t->round_best = t->best;
  }
  t->open = hipEventRecord(t->e0, s) == hipSuccess;
  t->trial_calls++;
  return kSpanCand[t->phase];
}
void tdr_su_span_end(SpanTuner* t, hipStream_t s) {
  if (tdr_cfg().su_span_fixed || !t || !t->open) return;
  t->open = false;
  t->pending = hipEventRecord(t->e1, s) == hipSuccess;
}
static std::atomic<int64_t> g_su_launches{0};   // diagnostics only
extern "C" int64_t tdr_shift_uniform_launches(void) { return g_su_launches.load(); }
// Padding costs up to 63 idle lanes per heading bin: the order pays once a bin holds a few waves on average.
bool tdr_su_shape_ok(int nb, int nr, int group, int64_t n_total) {
  if (tdr_cfg().su_mode == 0) return false;
  if (group % 4 != 0 || nb > 4095) return false;
  if (tdr_cfg().su_mode == 2) return true;   // tests: small filters and small windows too
  // A small window does not pay for the per-sector set-up of the shift-uniform kernel (bounding box, mask staging, three
  // barriers) nor for a wave per particle: at the reference node's own 100 x 25 bins and 20 000 particles the integer form
  // takes 0.23 ms (0.18 + 0.10, side by side) where the float kernel takes 0.11 (profiles/r04_bench_ref_integer_form_v1.json).
  if ((int64_t)nb * nr < 8192) return false;
  return n_total >= (int64_t)64 * nb;
}
// ---- tail units: the rows of the launch's last ring groups (su_tail_plan, tdr_score_su.h) ---------------------------------
// Once the dispatcher has handed out the last workgroup nothing refills a compute unit: over the last workgroup's lifetime the
// chip runs from six resident workgroups per CU down to none.  Measured on MI355X at config 2 (tools/su_timeline.py,
// profiles/su_timeline_before_v1.txt): 11 200 live workgroups of 370 us each on 1 536 slots, a run-down of 164 us of a 2.87 ms
// kernel, 0.085 ms of it lost against a full chip.  With the last K groups cut into Q rows the run-down lasts a short row's
// lifetime; a sector's mask is staged once either way, so the bulk keeps the economy of its long groups — and 16-ring groups,
// which lost to 8-ring ones on their run-down alone (3.69 against 3.50 ms), now win (tdr_score.hip: score_ws).
// K and Q: TdrConfig::su_tail_groups / su_tail_parts (tdr_config.h has the sweep behind the defaults).
// The rule of the shapes: short rows pay where workgroups QUEUE — a launch of fewer than two rounds of the chip's resident
// workgroups (256 CUs x 6) has no run-down worth shortening.
// Results never depend on it.  (tdr_config_shift_uniform(2), the tests' mode: whatever the knobs say, on any shape.)
void tdr_su_tail(int nchunks, int64_t n, int* k, int* q) {
  *k = std::min(tdr_cfg().su_tail_groups, nchunks);
  *q = tdr_cfg().su_tail_parts;
  if (tdr_cfg().su_mode != 2 && cdiv(std::max<int64_t>(n, 1), 256) * nchunks < 2 * 256 * 6) *k = 0;
  if (*k == 0 || *q == 1) { *k = 0; *q = 1; }
}
extern "C" int tdr_su_tail_plan(int nchunks, int k, int q, int row, int* group, int* s0, int* s1) {   // tests
  int g = 0, a = 0, b = 0;
  const int rows = su_tail_plan(nchunks, k, q, row, &g, &a, &b);
  if (row >= 0 && row < rows) {
    if (group) *group = g;
    if (s0) *s0 = a;
    if (s1) *s1 = b;
  }
  return rows;
}
// The ordering passes' rule of shapes.  The bucket sort (su_colscan_kernel) keeps a table of one word per (segment of SU_SEG
// positions, key): n (nb + 1) / 512 words, a quarter of the particle count at config 2's 256 bins and two words at the
// Cartesian launch's two keys.  It is taken while the table stays in proportion to the particles — segments x keys <= 4 n +
// 65536 — which holds for every n up to nb = 2047 and leaves to rocPRIM's sort the launches of more headings over many
// particles: from n = 16 384 on at nb = 4095, from about 35 000 on at nb = 3000.  (The bound is a choice of proportion, not a
// measured crossover: nobody has timed the bucket sort against the merge sort at such shapes.)  Same slot list either way: a
// stable sort by key has one answer.  tdr_config_tuning("su_order_bucket", 0): always rocPRIM (A/B).
static int64_t su_seg_table_words(int nb, int64_t n) {   // 0: no bucket sort for this shape
  const int64_t words = cdiv(std::max<int64_t>(n, 1), SU_SEG) * ((int64_t)nb + 1);
  return words <= 4 * std::max<int64_t>(n, 1) + 65536 ? words : 0;
}
// words reserved for the table: never fewer for more particles, so that a workspace sized for n holds every launch of up to n
static int64_t su_seg_table_reserve(int nb, int64_t n) {
  const int64_t m = std::max<int64_t>(n, 1);
  return std::min<int64_t>(cdiv(m, SU_SEG) * ((int64_t)nb + 1), 4 * m + 65536);
}
static bool su_order_is_bucket(int nb, int64_t n) { return tdr_cfg().su_order_bucket && su_seg_table_words(nb, n) > 0; }
static size_t su_sort_tmp_bytes(int64_t n) {
  size_t bytes = 0;
  uint32_t* k = nullptr;
  int32_t* v = nullptr;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, bytes, k, k, v, v, (size_t)std::max<int64_t>(n, 1), 0u, 12u,
                                           (hipStream_t)0, false);
  if (e != hipSuccess || bytes == 0) bytes = (size_t)(n + 4096) * 16;   // no device to ask: a generous bound
  return bytes;
}
SuWs tdr_su_ws(int nb, int nr, int group, int64_t n) {
  SuWs w;
  const int64_t nchunks = cdiv(nr, group), nbins = nchunks * nb * group;
  int64_t o = 0;
  auto take = [&](int64_t words) { const int64_t at = o; o += (words + 63) / 64 * 64; return at; };   // 256-byte aligned
  w.tab_su = take(2 * nbins);
  w.desc = take(4 * nbins);
  w.bbox = take(nchunks * SU_NSECT * 4);
  w.keys_in = take(n);
  w.keys_out = take(n);
  w.vals_in = take(n);
  w.vals_out = take(n);
  w.ints = take(3 * ((int64_t)nb + 1) + TDR_SU_TAIL_INTS);   // [cnt][start][slot_start] nb + 1 each, [counts 3][n_multi][inexact][mass bound][table is not its factors]
  w.slots = take(su_npad(n, nb));
  w.sort_tmp = take((int64_t)((su_sort_tmp_bytes(n) + 3) / 4));
  const int64_t T = tdr_ray_padded_samples(nb, nr);
  w.ray_tab = take(2 * T);                     // tdr_score_ray.hip: sample offsets and 16-bit scan descriptors in ray order,
  w.ray_desc = take((T + 1) / 2);              // the list of bins that hold several classes
  w.ray_multi = take((int64_t)nb * nr);
  w.ray_rad = take(T / nb);                    // the rings' radii in ray order (a table given as factors)
  w.seg_hist = take(su_seg_table_reserve(nb, n));   // the bucket sort's table (whatever su_order_bucket says at the time)
  // the patch order's compact lists: RAY_CL_WORDS words and a table of 16 per sector (16 scan rows x 64 rings)
  const bool patch_shape = nb % RAY_PG == 0 && nb <= RAY_PATCH_MAX_NB;
  const int64_t sectors = patch_shape ? (int64_t)(nb / RAY_PG) * ray_blocks(nr, true) : 0;
  w.ray_clist = take(sectors * RAY_CL_WORDS);
  w.ray_ctab = take(sectors * 16);
  w.full_mask = take(nchunks * 2 * nb);   // the bins with several classes, a word per (ring group, scan row), rows twice over
  w.total = o;
  return w;
}

// The ordering passes alone: the slot list — dense particles by heading bin (one bin when L.nb == 1: the Cartesian score has
// no heading bins), every bin padded to whole waves (-1), then the sparse particles in the caller's order — and the counts.
int tdr_su_order(const SuLaunch& L, const SuWs& W, hipStream_t s, const int32_t** slots_out, const int32_t** counts_out,
                 float* box_init, int box_count) {
  int32_t* base = L.ws;
  uint32_t* keys_in = reinterpret_cast<uint32_t*>(base + W.keys_in);
  uint32_t* keys_out = reinterpret_cast<uint32_t*>(base + W.keys_out);
  int32_t* vals_in = base + W.vals_in;
  int32_t* vals_out = base + W.vals_out;
  int* cnt = base + W.ints;
  const int nkeys = L.nb + 1;
  int* start = cnt + nkeys;
  int* slot_start = start + nkeys;
  int* counts = slot_start + nkeys;
  int32_t* slots = base + W.slots;
  const int64_t n = L.n;
  if (su_order_is_bucket(L.nb, n)) {
    // key + segment histograms, column prefixes, offsets (+ padding, + the zeroed words behind counts), ranked scatter
    int* seg_hist = base + W.seg_hist;
    const int64_t segs = cdiv(n, SU_SEG);
    hipLaunchKernelGGL(su_key_kernel, dim3((unsigned)segs), dim3(256), sizeof(int) * (size_t)nkeys, s, L.st, L.cap, n, L.perm,
                       L.nb, L.span, SU_SEG, keys_in, vals_in, (int*)nullptr, seg_hist);
    LAUNCH_CHECK("su_key");
    hipLaunchKernelGGL(su_colscan_kernel, dim3((unsigned)cdiv(nkeys, 64)), dim3(64 * SU_COLSCAN_WAVES), 0, s, seg_hist,
                       (int)segs, nkeys, cnt);
    LAUNCH_CHECK("su_colscan");
    hipLaunchKernelGGL(su_offsets_kernel, dim3(1), dim3(256), 0, s, (const int*)cnt, nkeys, start, slot_start, counts, slots,
                       box_init, box_count);
    LAUNCH_CHECK("su_offsets");
    unsigned bits = 1;
    while ((1u << bits) < (unsigned)nkeys) bits++;
    hipLaunchKernelGGL(su_rank_scatter_kernel, dim3((unsigned)segs), dim3(64), sizeof(int) * (size_t)nkeys, s,
                       (const uint32_t*)keys_in, (const int32_t*)vals_in, n, (const int*)seg_hist, (const int*)slot_start, nkeys,
                       (int)bits, slots);
    LAUNCH_CHECK("su_rank_scatter");
  } else {
    HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)(3 * nkeys + TDR_SU_TAIL_INTS), s));
    HIP_TRY(hipMemsetAsync(slots, 0xFF, sizeof(int32_t) * (size_t)L.npad, s));
    hipLaunchKernelGGL(su_key_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), sizeof(int) * (size_t)nkeys, s, L.st, L.cap, n,
                       L.perm, L.nb, L.span, 256, keys_in, vals_in, cnt, (int*)nullptr);
    LAUNCH_CHECK("su_key");
    hipLaunchKernelGGL(su_offsets_kernel, dim3(1), dim3(256), 0, s, (const int*)cnt, nkeys, start, slot_start, counts,
                       (int32_t*)nullptr, box_init, box_count);
    LAUNCH_CHECK("su_offsets");
    unsigned bits = 1;
    while ((1u << bits) < (unsigned)nkeys) bits++;
    size_t tmp_bytes = su_sort_tmp_bytes(n);
    HIP_TRY(rocprim::radix_sort_pairs(base + W.sort_tmp, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, bits,
                                      s, false));
    hipLaunchKernelGGL(su_scatter_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, (const uint32_t*)keys_out,
                       (const int32_t*)vals_out, n, (const int*)start, (const int*)slot_start, slots);
    LAUNCH_CHECK("su_scatter");
  }
  *slots_out = slots;
  *counts_out = counts;
  return TDR_OK;
}
// The ordering passes on their own (tests, timing): tdr_k_su_order_workspace_ints(n, nb) words of workspace; slots_out
// su_npad(n, nb) words — those behind counts_out[2] are whatever the workspace held or the passes left there —, keys_out the n
// keys in the caller's order, counts_out 3; bucket_out (host, optional): 1 when the bucket sort ran, 0 for rocPRIM's path.
extern "C" size_t tdr_k_su_order_workspace_ints(int64_t n, int nb) {
  if (n < 1 || nb < 1 || nb > 4095) return 0;
  return (size_t)tdr_su_ws(nb, 4, 4, n).total;
}
extern "C" int64_t tdr_k_su_order_slots(int64_t n, int nb) { return n < 1 || nb < 1 ? 0 : su_npad(n, nb); }
extern "C" int tdr_k_su_order(const float* st, int64_t cap, int64_t n, const int32_t* perm, int nb, float span,
                              int32_t* workspace, int32_t* slots_out, int32_t* keys_out, int32_t* counts_out, int* bucket_out,
                              void* stream) {
  if (!st || !workspace || !slots_out || !keys_out || !counts_out) return fail(TDR_ERR_ARG, "su_order: null pointer");
  if (n < 1 || cap < n || nb < 1 || nb > 4095) return fail(TDR_ERR_ARG, "su_order: bad shape");
  hipStream_t s = (hipStream_t)stream;
  const SuWs W = tdr_su_ws(nb, 4, 4, n);
  SuLaunch L{};
  L.st = st; L.cap = cap; L.n = n; L.perm = perm; L.nb = nb; L.span = span; L.ws = workspace;
  L.npad = su_npad(n, nb);
  const int32_t* slots = nullptr;
  const int32_t* counts = nullptr;
  if (bucket_out) *bucket_out = su_order_is_bucket(nb, n) ? 1 : 0;
  if (int rc = tdr_su_order(L, W, s, &slots, &counts)) return rc;
  HIP_TRY(hipMemcpyAsync(slots_out, slots, sizeof(int32_t) * (size_t)L.npad, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(keys_out, workspace + W.keys_in, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(counts_out, counts, sizeof(int32_t) * 3, hipMemcpyDeviceToDevice, s));
  return TDR_OK;
}
// rings per direction of score_prep_kernel's grid: a multiple of 64 that covers both layouts
static int prep_padded_rings(const SuLaunch& L) {
  const bool bm = ray_bm(L);
  const int ray = ray_blocks(L.nr, bm) * ray_gq(L.nr, bm) * 64;
  return (int)(cdiv(std::max(L.nchunks * L.group, ray), 64) * 64);
}
int tdr_su_prepare(const SuLaunch& L, const SuWs& W, hipStream_t s, const int32_t** slots_out, const int32_t** counts_out) {
  int32_t* base = L.ws;
  float* bbox = reinterpret_cast<float*>(base + W.bbox);
  if (L.rf != 4 && L.rf != 8 && L.rf != 12) return fail(TDR_ERR_ARG, "score_prep: no integer form for records of %d floats", L.rf);
  if (int rc = tdr_su_order(L, W, s, slots_out, counts_out, bbox, L.nchunks * SU_NSECT)) return rc;
  int* ints = base + W.ints + 3 * (L.nb + 1);   // [counts 3][n_list][inexact][mass bound][table is not its factors]
  PrepArgs p;
  p.tab = L.tab_src; p.scan_pk = L.scan_pk;
  p.nb = L.nb; p.nr = L.nr; p.rf = L.rf; p.ncls = L.map->ncls; p.rp = prep_padded_rings(L);
  p.uscale = L.uniform_scale ? L.uscale : 0.f; p.res = L.res;
  p.utab = L.uniform_scale ? L.utab_out : nullptr;
  const int lc = L.map->cwords == 1 ? 3 : (L.map->cwords == 2 ? 2 : 1);
  p.group = L.group; p.nchunks = L.nchunks;
  p.ckconst = ((L.map->rows >> lc) + 2) * 128 + 128;   // cmap_offset (tdr_score_dev.h)
  // plane_offset's constant for class 0's plane, as a byte offset from crec (tdr_score_ray.hip uses the same)
  p.plane_bytes = (unsigned)(tdr_cmap_plane_words(L.map->ncls, L.map->rows, L.map->cols) * 4);
  p.pbase = (unsigned)(tdr_cmap_plane_offset_words(L.map->ncls, L.map->rows, L.map->cols) * 4) +
            (unsigned)(plane_trows(L.map->rows) * 128) + 128u;
  p.dict = L.map->dict; p.dict_n = L.map->dict_n;
  p.tab_su = reinterpret_cast<float*>(base + W.tab_su);
  p.desc = reinterpret_cast<uint32_t*>(base + W.desc);
  p.bbox = bbox;
  const bool bm = ray_bm(L);
  p.gq = ray_gq(L.nr, bm); p.blocks = ray_blocks(L.nr, bm); p.bm = bm ? 1 : 0; p.patch = ray_patch(L) ? 1 : 0;
  p.borrow = tdr_cfg().ray_borrow ? 1 : 0;
  p.dict_tail = reinterpret_cast<const uint32_t*>(L.map->dict) + 2 * TDR_CMAP_MAX_DICT;
  p.fac = L.fac;
  p.tab_ray = reinterpret_cast<float*>(base + W.ray_tab);
  p.rad_ray = reinterpret_cast<float*>(base + W.ray_rad);
  p.desc_ray = reinterpret_cast<uint16_t*>(base + W.ray_desc);
  p.list = reinterpret_cast<uint32_t*>(base + W.ray_multi);
  p.n_list = ints + 3; p.inexact = ints + 4;
  p.clist = nullptr; p.ctab = nullptr;
  p.full_mask = tdr_su_full_list(L) ? reinterpret_cast<uint32_t*>(base + W.full_mask) : nullptr;
  p.sums = reinterpret_cast<uint32_t*>(L.part);
  p.sums_words = L.part ? (int64_t)(2 * L.map->ncls + 2) * L.npad : 0;
  if (p.patch) {   // the compact lists: a workgroup per sector (the direction count is a multiple of 16)
    p.clist = reinterpret_cast<uint32_t*>(base + W.ray_clist);
    p.ctab = base + W.ray_ctab;
    hipLaunchKernelGGL(score_prep_kernel<PREP_DIRS_COMPACT>, dim3((unsigned)(L.nb / PREP_DIRS_COMPACT * (p.rp / 64))),
                       dim3(64 * PREP_DIRS_COMPACT), 0, s, p);
  } else {
    hipLaunchKernelGGL(score_prep_kernel<8>, dim3((unsigned)(cdiv(L.nb, 8) * (p.rp / 64))), dim3(64 * 8), 0, s, p);
  }
  LAUNCH_CHECK("score_prep");
  return TDR_OK;
}
// The preparation's products, copied out of a launch's workspace (tdr_k_score_prep, tdr_score.hip): what each holds is
// described at score_prep_kernel; layout: the shapes behind their sizes.
int tdr_su_prep_copy_out(const SuLaunch& L, const SuWs& W, hipStream_t s, int64_t layout[16], void* const out[9]) {
  const bool bm = ray_bm(L);
  const int64_t nbins = (int64_t)L.nchunks * L.nb * L.group, T = tdr_ray_padded_samples(L.nb, L.nr);
  if (layout) {
    const int64_t v[16] = {L.group, L.nchunks, prep_padded_rings(L), ray_gq(L.nr, bm), ray_blocks(L.nr, bm), bm ? 1 : 0,
                           ray_patch(L) ? 1 : 0, T, nbins, SU_NSECT, TDR_SU_TAIL_INTS, L.uniform_scale ? 1 : 0, 0, 0, 0, 0};
    for (int k = 0; k < 16; k++) layout[k] = v[k];
  }
  if (!out || !L.ws) return TDR_OK;
  const int32_t* base = L.ws;
  const struct { const void* src; size_t bytes; } parts[9] = {
      {L.uniform_scale ? L.utab_out : nullptr, sizeof(float) * 2 * (size_t)L.nb * L.nr},
      {base + W.tab_su, sizeof(float) * 2 * (size_t)nbins},
      {base + W.desc, sizeof(uint32_t) * 4 * (size_t)nbins},
      {base + W.bbox, sizeof(float) * 4 * (size_t)L.nchunks * SU_NSECT},
      {base + W.ray_tab, sizeof(float) * 2 * (size_t)T},
      {base + W.ray_desc, sizeof(uint32_t) * (size_t)((T + 1) / 2)},
      {base + W.ray_rad, sizeof(float) * (size_t)(T / L.nb)},
      {base + W.ray_multi, sizeof(uint32_t) * (size_t)L.nb * L.nr},
      {base + W.ints + 3 * (L.nb + 1), sizeof(int32_t) * TDR_SU_TAIL_INTS}};
  for (int k = 0; k < 9; k++)
    if (out[k] && parts[k].src) HIP_TRY(hipMemcpyAsync(out[k], parts[k].src, parts[k].bytes, hipMemcpyDeviceToDevice, s));
  return TDR_OK;
}

int tdr_su_score(const SuLaunch& L, const SuWs& W, hipStream_t s) {
  const tdr_map_desc* map = L.map;
  int32_t* base = L.ws;
  int* nslots = base + W.ints + 3 * (L.nb + 1);   // counts[0]
  SuArgs u;
  const int lc = map->cwords == 1 ? 3 : (map->cwords == 2 ? 2 : 1);
  u.crec = map->crec; u.dict_int = reinterpret_cast<const uint32_t*>(map->dict) + TDR_CMAP_MAX_DICT;
  u.dict_n = map->dict_n; u.ctiles_r = (map->rows >> lc) + 2;
  u.pkcol = plane_trows(map->rows) * 128 - 16;
  u.inexact = nslots + 4;
  u.rows = map->rows; u.cols = map->cols; u.resolution = map->resolution;
  u.tab_su = reinterpret_cast<const float*>(base + W.tab_su);
  u.desc = reinterpret_cast<const uint32_t*>(base + W.desc);
  u.bbox = reinterpret_cast<const float*>(base + W.bbox);
  u.kmask = map->crec + tdr_cmap_tile_words(map->ncls, map->rows, map->cols);
  u.kcolw = kmask_trows(map->rows) * 32;
  u.kmask_off = (unsigned)(tdr_cmap_tile_words(map->ncls, map->rows, map->cols) * 4);
  u.scan_pk = L.scan_pk;
  u.nb = L.nb; u.nr = L.nr; u.res = L.res; u.st = L.st; u.cap = L.cap;
  u.slots = base + W.slots; u.nslots = nslots;
  u.group = L.group; u.nchunks = L.nchunks; u.tail_k = L.tail_k; u.tail_q = L.tail_q; u.ncls = map->ncls; u.npad = L.npad; u.part = reinterpret_cast<uint32_t*>(L.part);
  u.stats = tdr_profile_stats_ptr();
  u.full_mask = tdr_su_full_list(L) ? reinterpret_cast<const uint32_t*>(base + W.full_mask) : nullptr;
  u.plane_bytes = (unsigned)(tdr_cmap_plane_words(map->ncls, map->rows, map->cols) * 4);   // (as tdr_su_prepare has them)
  u.pbase = (unsigned)(tdr_cmap_plane_offset_words(map->ncls, map->rows, map->cols) * 4) + (unsigned)(plane_trows(map->rows) * 128) + 128u;
  u.list_stats = tdr_profile_su_list_ptr();
  int rg, r0, r1;
  const int rows = su_tail_plan(L.nchunks, L.tail_k, L.tail_q, -1, &rg, &r0, &r1);
  if (L.rows != rows) return fail(TDR_ERR_ARG, "score: a grid of %d rows for a plan of %d", L.rows, rows);
  const dim3 grid((unsigned)cdiv(L.npad, 256), (unsigned)rows), block(256);
  const bool ks = tdr_has_kslot(map->ncls, L.rf), us = L.uniform_scale;
#define TDR_LAUNCH_SU(NV4)                                                                         \
  if (ks && us) hipLaunchKernelGGL((score_polar_su_kernel<NV4, true, true>), grid, block, 0, s, u);  \
  else if (ks) hipLaunchKernelGGL((score_polar_su_kernel<NV4, true, false>), grid, block, 0, s, u);  \
  else if (us) hipLaunchKernelGGL((score_polar_su_kernel<NV4, false, true>), grid, block, 0, s, u);  \
  else hipLaunchKernelGGL((score_polar_su_kernel<NV4, false, false>), grid, block, 0, s, u);
  switch (L.rf / 4) {
    case 1: TDR_LAUNCH_SU(1) break;
    case 2: TDR_LAUNCH_SU(2) break;
    case 3: TDR_LAUNCH_SU(3) break;
    default: return fail(TDR_ERR_ARG, "score: no shift-uniform kernel for record size %d", L.rf);
  }
#undef TDR_LAUNCH_SU
  LAUNCH_CHECK("score_polar_su");
  g_su_launches.fetch_add(1);
  return TDR_OK;
}
