// tdr_score_ray.hip — the RAY-MAPPED polar scoring kernel: one WAVE per particle, lanes = consecutive rings of a direction.
//
// For whom.  The scattered particles of a launch (su_key_kernel, tdr_score_su.hip: the uniform tenth of the bench mix,
// particle initialisation, the tails of a cluster).  With lane = particle (score_polar_kernel, score_polar_su_kernel) a
// wave of scattered particles gathers from 64 unrelated windows: 64 cache lines per gather instruction (160 CU cycles
// measured against 16 for <= 4 lines, tools/ta_cost.hip), every line used by ONE sample, and a window's lines are
// requested once per ring group, far apart in time.  Here a wave walks ONE window from its first sample to its last:
// 64 consecutive rings of one direction per step, i.e. 64 cells along a ray —
//   * a gather touches 8-11 lines instead of 64 (a plane tile holds 8 x 8 cells), 2-3 per 16 lanes: the address path's
//     minimum of 16 cycles per instruction,
//   * neighbouring directions follow each other in time: a line fetched for direction i is still in the L2 for i + 1,
//   * what is fetched is the CLASS PLANE of the one class the scan bin holds (2 bytes per cell, tdr_cmap.hip) — or, for an
//     empty bin, the 16 known bits around the cell from the coarse mask plane: 2 400 lines per window on the config-2 scene
//     where the 8-byte records of all classes take 6 700.
// Why it may: the product sums are EXACT integers (a scan count times a dictionary value that is an integer multiple of
// 2^-q, accumulated in 64 bits), so they do not depend on the order of the additions — lane-major here, sample-major in
// the lane = particle kernels — and a particle's weight is the same bits whichever kernel scored it
// (tests/test_shift_uniform.py, tests/test_ray.py).
//
// What bounds it: the L1 address path (every vector memory instruction of a wave costs it >= 16 cycles) and vector issue,
// about equally (the first version: three memory instructions and ~55 vector instructions per step, 53 CU cycles per step
// measured).  So a step of 64 samples is ONE gather and ~21 vector instructions:
//   * the scan descriptors of a lane's rings of one direction are 16 bits each — class code, count — packed side by side:
//     one load per direction brings up to four steps' worth; the sample offsets likewise (two 16-byte loads);
//   * everything that depends on the bin's class only — the byte offset of its plane (the coarse mask plane for an empty
//     bin), the column shift that turns a cell into a mask cell, the bit the cell's `known` flag sits at, the accumulator the
//     product goes to — comes out of a 16-entry table in LDS with one 16-byte read, so there is no branch and no select in
//     the loop: an empty bin multiplies a count of zero;
//   * mask plane and class planes share one offset formula (plane_offset: same tile shape, same tile-column stride);
//   * a lane adds its products into its own 64-bit accumulators in LDS, one per class (ds_add_u64).
// Bins that hold several classes, or a count beyond 12 bits, are "empty" to the loop and go through a list afterwards.
//
// Per launch: score_prep_kernel (tdr_score_su.hip: sample offsets and scan descriptors in ray order, the list, the `inexact`
// flag — the same launch prepares the shift-uniform kernel's side), then
// score_polar_ray_kernel over the sparse share of the slot list; score_finalize_exact_kernel (tdr_score.hip) turns the
// integer sums into weights.
#include "tdr_score_int_dev.h"
#include "tdr_score_su.h"

// ray order: a direction's rings in BLOCKS of GQ steps of 64 rings (GQ = 1, 2 or 4: ray_gq); "row" m = direction * blocks
// + block.  Lane l of step g of block b is ring (b * GQ + g) * 64 + l.
// BLOCK-MAJOR order (bm; launches whose table comes with its factors): one step per row, GQ = 1, and the rows of ring
// segment 0 (rings 0..63, every direction) first, then segment 1's, ...: row m = segment * nb + direction.  The eight
// gathers a wave has in flight are then neighbouring directions of ONE segment (config 2, uniform particles: 9.1 -> 8.4 ms;
// with the offsets read from tab_ray the narrow rows cost more than that gains, so those launches keep the first order).
// tdr_config_tuning("ray_block_major", 0) keeps the first order everywhere (A/B; same bits).
// PATCH order (round 5; block-major launches whose direction count is a multiple of 16 and at most RAY_PATCH_MAX_NB).
// Counters of the block-major ray order (100 000 uniform particles, profiles/r05_pmc_ray_patch_v1.txt): the L1 address path
// 0.87 busy at 38 cycles per step — for THREE vector memory instructions a step (the gather, the 2-byte descriptors, the
// radii), each at least 16 cycles there (four lanes a cycle, whatever a lane fetches).  So the step should cost ONE and a
// quarter:
//   * a UNIT is 16 scan rows x 16 rings = four steps; a lane's four 16-bit descriptors of a unit lie side by side: ONE 8-byte
//     load per unit.  That needs the unit aligned in the descriptor array whatever the particle's heading: units are groups of 16
//     SCAN rows, the window direction of scan row r is (r - shift) mod nb — the window is a full circle, any rotation of the
//     grouping walks all of it;
//   * a step's 64 lanes are 4 neighbouring directions x 16 consecutive rings — a PATCH of the window, not a ray (fewer tiles);
//     the four directions' {cos, sin} pairs are no longer uniform over the wave: they come out of LDS (the factors' direction
//     table, 8 bytes a direction), the lane's radius depends on the ring block only: four registers per 64-ring segment;
//   * order: segment of 64 rings -> group of 16 scan rows -> the segment's four ring blocks -> the unit's four steps, so that
//     what a wave has just fetched is the sector next to the one it fetches now.
// Lane l = direction (l >> 4) of the step's four, ring (l & 15) of the block.  tdr_config_tuning("ray_patch", 0): the ray order
// (A/B; same bits).
// COMPACT lists (round 6; the patch order with the table's factors): the wave walks lists of a sector's non-empty bins, 64 to
// a gather, and the empty bins only as far as the gate needs them — see above ray_body.  They take the place of the patch
// walk above wherever the factors are the table's; the patch walk itself is left for a table that is not its factors'
// products (it reads the offsets from the table, and desc_ray as before).  Measured on config 2 (13 868
// scattered particles, HIP events around the kernel): 1.02 -> 0.93 ms; 1 488 -> 1 041 vector-memory instructions per
// particle; the L1 address path 0.84 -> 0.69 busy, at 35 -> 42 cycles per gather.
// (the first order pads to whole blocks of GQ steps: never less than the block-major order needs)
int64_t tdr_ray_padded_samples(int nb, int nr) { return (int64_t)nb * ray_blocks(nr, false) * ray_gq(nr, false) * 64; }

// The layouts — tab_ray, rad_ray, desc_ray, the list, the `inexact` words — are written by score_prep_kernel
// (tdr_score_su.hip), which describes them.
struct RayArgs {
  const uint32_t* crec;     // compact map: tiles, known mask, class planes, coarse mask plane (byte offsets from here)
  unsigned planes_off;      // byte offset of class plane 0
  unsigned plane_bytes;     // bytes of a class plane
  unsigned cmask_off;       // byte offset of the coarse mask plane
  int pkcol;                // plane_offset: bytes of a tile column - 16 (the same for every plane)
  const uint32_t* dict_int;
  int dict_n;
  int rows, cols;
  float resolution;
  const float* tab;         // [P][2] in the table's own order (the list pass)
  const float* tab_ray;
  const float* fac;         // the table's factors, or NULL; rad_ray: the radii in ray order
  const float* rad_ray;
  float uscale;
  const uint16_t* desc_ray;
  const uint32_t* list;
  const int32_t* n_list;
  const float* scan_pk;
  int rf, ncls, nb, nr, blocks;
  float res;
  const float* st;
  int64_t cap;
  const int32_t* slots;     // the launch's slot list; the sparse share is slots [counts[0], counts[0] + counts[1])
  const int32_t* counts;
  const int32_t* inexact;
  int nsplit;               // waves per particle: each takes a contiguous share of the directions and adds its sums to the slot's
  int64_t npad;
  uint32_t* part;           // the launch's sums [2 ncls + 2][npad], score_polar_su_kernel's too (int_add_sums)
  const uint32_t* clist;    // COMPACT: the sectors' bin lists and their table (score_prep_kernel)
  const int32_t* ctab;
  uint32_t* gate_ctr;       // NULL, or (profiling) the four counters of tdr_profile_ray_gate
};

// FAC: the sample offsets are multiplied out of the table's factors — a direction's pair (uniform over the wave: two scalar
// loads) times the lane's own radii (registers) — instead of read from tab_ray: the same float products the table holds
// (score_prep_kernel checked that), and 16 bytes per lane and row less through the texture path.
// lacc [4 waves][ncls + 1][64 lanes]: a lane's sums per class (slot 0: no class); lut, per class code: {plane constant,
// column shift, known-bit index, accumulator}.  The prologue that fills them, the list pass and the epilogue are
// score_cart_ray_kernel's too: ray_prologue, ray_list_pass, ray_add_sums (tdr_score_int_dev.h).
// PATCH (with BM): the patch order (see the top of the file); ldir: the directions' pairs in LDS
// COMPACT: the entries of gathers 0 .. N - 1 of a step that starts at entry e0 (a multiple of 256) of a stream — one 16-byte
// load per lane and block of four gathers (score_prep_kernel stores the blocks lane-major and fills the last one with
// RAY_CL_NONE: no class, no count, and a radius that leaves the map).
template <int N>
__device__ __forceinline__ void ray_list_load(const uint4* __restrict__ lst, int e0, int lane, uint32_t (&w)[N]) {
  uint4 q[(N + 3) / 4];
#pragma unroll
  for (int b = 0; b < (N + 3) / 4; b++) q[b] = lst[((e0 >> 8) + b) * 64 + lane];
#pragma unroll
  for (int u = 0; u < N; u++) {
    const uint4 qq = q[u >> 2];
    w[u] = (u & 3) == 0 ? qq.x : ((u & 3) == 1 ? qq.y : ((u & 3) == 2 ? qq.z : qq.w));
  }
}
// COMPACT (= PATCH with FAC; round 6).  An empty scan bin adds nothing to a cost and nothing to the normalisation: the loop
// gathers its cell only to count the cell's known bit, and the known count has ONE consumer — the gate of
// state_particle.cpp:117-120, which for P < 2^24 asks whether 2 known >= P (score_finalize_exact_kernel: a correctly rounded
// quotient of two exact floats is below one half exactly when it is).  So score_prep_kernel packs each sector's bins into
// lists: A, the single-class bins with a count below 2^12, unit by unit and class by class; B, the bins the loop sees as
// empty.  An entry carries its position in the sector — scan row & 15, ring & 63, as byte offsets into the two LDS tables
// below — and, A, the descriptor.
//   Phase 1: a wave walks the A lists of its sectors, 64 entries per gather; a lane's direction pair and radius come out of
//     LDS by the entry's position.  Products, normalisation and the A bins' known bits are exact.
//   Phase 2, the gate count: the waves of a particle add their phase-1 counts and their B entries into LDS words and meet at
//     one barrier.  A total of at least P / 2 settles the particle; so does a total that stays below P / 2 even if every B
//     cell were known (it will be NaN).  Otherwise the waves walk their B lists on the mask plane in blocks of up to 256
//     entries, add each block's known bits to the shared word and stop when it has reached P / 2 or the lists end.
// INVARIANT: every unit added to a known count is the known bit of a distinct real sample, so the count the waves add up in
// the launch's sums never exceeds the true one; a wave leaves its B lists unfinished only after the shared total — all of it counted
// by waves that write it out — reached P / 2.  So the added-up count is >= P / 2 exactly when the true count is, and the gate
// falls as it did.  Where a particle's waves do not share a workgroup (a split that does not divide 4) or P >= 2^24 the B
// lists are walked to the end: the exact count.
template <int GQ, bool USCALE, bool FAC, bool BM, bool PATCH>
__device__ __forceinline__ void ray_body(const RayArgs& a, unsigned long long* lacc, uint32_t* ldict, uint4* lut, float2* ldir,
                                         uint32_t (*lgate)[4]) {
  static_assert(!BM || GQ == 1, "block-major: one step per row");
  static_assert(!PATCH || BM, "the patch order is a block-major order");
  constexpr bool COMPACT = PATCH && FAC;
  const int nsparse = a.counts[1];
  if ((int64_t)blockIdx.x * 4 >= (int64_t)nsparse * a.nsplit) return;   // whole workgroup idle (uniform)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned long long* const my = ray_prologue(a, lacc, ldict, lut, wave, lane);
  // COMPACT: the rings' radii behind the accumulators, 65 per segment of 64 rings (a ring the image does not have, and
  // RAY_CL_NONE's slot 64: the cell leaves the map); ldir: the directions' pairs twice over, so that (scan row - shift + nb)
  // needs no wrap
  float* const lrad = reinterpret_cast<float*>(lacc + (size_t)4 * (a.ncls + 1) * 64);
  // the gate count is shared where a particle's waves are waves of one workgroup and the gate is the integer comparison
  const bool gate_shared = COMPACT && 4 % a.nsplit == 0 && (int64_t)a.nb * a.nr < (1 << 24);
  if constexpr (COMPACT) {
    for (int t = threadIdx.x; t < 2 * a.nb + RAY_PG; t += 256) ldir[t] = reinterpret_cast<const float2*>(a.fac)[t % a.nb];
    for (int t = threadIdx.x; t < a.blocks * 65; t += 256) {
      const int sg = t / 65, rr = t - sg * 65, jr = sg * 64 + rr;
      lrad[t] = rr < 64 && jr < a.nr ? a.fac[2 * a.nb + jr] : 1.0e30f;
    }
    if (threadIdx.x < 16) lgate[threadIdx.x >> 2][threadIdx.x & 3] = 0;   // per particle: {phase-1 count, B entries, B count, waves done}
  }
  const unsigned pconst = (unsigned)(a.pkcol + 16) + 128u;   // plane_offset's constant without the plane's own offset
  __syncthreads();
  const int64_t gw = (int64_t)blockIdx.x * 4 + wave;
  const int64_t q = gw / a.nsplit;
  const int part_id = (int)(gw - q * a.nsplit);
  if (q >= nsparse) {   // (wave-uniform; the only barrier below is the gate's)
    if (COMPACT && gate_shared && a.nsplit > 1) __syncthreads();
    return;
  }
  const int64_t slot = (int64_t)a.counts[0] + q;
  const int64_t p = a.slots[slot];
  const float scale = a.st[TDR_ST_SCALE * a.cap + p];
  const float fscale = USCALE ? a.uscale : scale;   // (the caller's promise: the same number)
  const float cx = a.st[TDR_ST_DX * a.cap + p] * scale + a.st[TDR_ST_INIT_X * a.cap + p];  // state_particle.cpp:161
  const float cy = a.st[TDR_ST_DY * a.cap + p] * scale + a.st[TDR_ST_INIT_Y * a.cap + p];  // :162
  const float off0 = cy / a.resolution;  // top_down_map_polar.cpp:29
  const float off1 = cx / a.resolution;  // :30
  const int shift = rot_shift_dev(a.st[TDR_ST_THETA * a.cap + p], a.nb);
  const float rmaxf = (float)a.rows, cmaxf = (float)a.cols;
  const char* __restrict__ crecb = reinterpret_cast<const char*>(a.crec);
  const tdr_v2f offv = {off0, off1};
  auto cell = [&](float tx, float ty, int& ri, int& ci) {
    tdr_v2f pv = {tx, ty};
    if constexpr (!USCALE) pv = (pv * scale) * a.res;  // top_down_map_polar.cpp:28
    int_cell(pv + offv, rmaxf, cmaxf, ri, ci);          // :29-31
  };
  auto cell_fac = [&](tdr_v2f dir, float rad, int& ri, int& ci) {
    tdr_v2f pv = dir * rad;                             // top_down_map_polar.cpp:17-18
    pv = (pv * fscale) * a.res;                         // :28
    int_cell(pv + offv, rmaxf, cmaxf, ri, ci);
  };

  // this wave's share of the window: rows m = direction * blocks + block; a window row meets scan row (m + shift * blocks)
  // mod (nb * blocks)
  const int rows_all = a.nb * a.blocks, per = (rows_all + a.nsplit - 1) / a.nsplit;
  const int m0 = part_id * per, m1 = min(rows_all, m0 + per);
  const int rot = shift * a.blocks;
  int bm_b = m0 / a.nb, bm_i = m0 - bm_b * a.nb;   // BM: the row's block and direction, kept by counting
  uint32_t known = 0, norm = 0;
  constexpr int U = 8 / GQ;   // rows whose gathers are in flight together: 8 steps
  typedef uint16_t desc_t __attribute__((ext_vector_type(GQ)));
  typedef float tab_t __attribute__((ext_vector_type(2 * GQ)));
  typedef float rad_t __attribute__((ext_vector_type(GQ)));
  const desc_t* __restrict__ descv = reinterpret_cast<const desc_t*>(a.desc_ray);
  const tab_t* __restrict__ tabv = reinterpret_cast<const tab_t*>(a.tab_ray);
  const rad_t* __restrict__ radv = reinterpret_cast<const rad_t*>(a.rad_ray);
  const tdr_v2f* __restrict__ dirv = reinterpret_cast<const tdr_v2f*>(a.fac);
  const bool one_block = a.blocks == 1;
  rad_t rad0 = {};
  if constexpr (FAC) rad0 = radv[lane];   // (block 0's; the only block of a window of up to 256 rings)
  // The two halves of a sample stand here and, to the letter, in score_cart_ray_kernel.  As shared forced-inline functions
  // (called directly or through these lambdas, a struct or four scalars per sample, the map pointer with or without
  // restrict) the table-order kernels <2 | 4, *, false, false> were scheduled and allocated differently (<4>: 75 -> 78
  // registers) and 100 000 uniform particles without a caller context took 8.54 ms against 8.32
  // (profiles/int_form_shared_timing_v1.txt, "first form").
  // one sample, first half: everything that depends on the bin's class out of the table, the cell's address, the gather
  auto issue = [&](uint32_t d, int ri, int ci, uint32_t& v, uint32_t& shb, uint32_t& cnt, uint32_t& acc_at) {
    cnt = d & 0xFFFu;
    // one 16-byte LDS read: everything that depends on the bin's class
    const uint4 e = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(lut) + ((d >> 8) & 0xF0u));
    const int rr = ri >> (int)e.y, cc = ci >> (int)e.y;  // a mask cell spans 4 x 4 map cells
    const unsigned off = plane_offset(rr, cc, a.pkcol, (int)e.x);
    // bit of `known`: 15 in a class cell, (row & 3) * 4 + (column & 3) in a mask cell
    shb = ((((uint32_t)ri & 3u) << 2) | ((uint32_t)ci & 3u)) | e.z;
    acc_at = e.w;
    v = *reinterpret_cast<const uint16_t*>(crecb + off);
  };
  // ... second half: the known bit, the normalisation, the product into the lane's accumulator of the class
  auto consume = [&](uint32_t v, uint32_t shb, uint32_t cnt, uint32_t acc_at) {
    uint32_t kbit;
    asm("v_bfe_u32 %0, %1, %2, 1" : "=v"(kbit) : "v"(v), "v"(shb));
    known += kbit;
    norm = __umul24(cnt, kbit) + norm;                  // state_particle.cpp:141-142
    const unsigned long long prod = (unsigned long long)cnt * int_dict_at(ldict, v);   // :136-139, as integers (0 for an empty bin)
    unsigned long long* const acc = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(my) + acc_at);
    __hip_atomic_fetch_add(acc, prod, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // ds_add_u64; the lane's own slot
  };
  auto rows_step = [&](auto cnt_c, int m) {
    constexpr int N = decltype(cnt_c)::value;
    desc_t dd[N];
    tab_t tt[N];
    rad_t rr_[N];
    tdr_v2f dir[N];
#pragma unroll
    for (int u = 0; u < N; u++) {
      int mr = m + u + rot;
      mr -= mr >= rows_all ? rows_all : 0;
      if constexpr (BM) {
        int r = bm_i + shift;
        r -= r >= a.nb ? a.nb : 0;
        mr = bm_b * a.nb + r;
      }
      dd[u] = descv[(int64_t)mr * 64 + lane];
      if constexpr (FAC && BM) {
        dir[u] = dirv[bm_i];
        rr_[u] = radv[(int64_t)bm_b * 64 + lane];
      } else if constexpr (FAC) {
        const int i = one_block ? m + u : (m + u) / a.blocks;
        dir[u] = dirv[i];
        rr_[u] = one_block ? rad0 : radv[(int64_t)(m + u - i * a.blocks) * 64 + lane];
      } else {
        tt[u] = tabv[(int64_t)(m + u) * 64 + lane];
      }
      if constexpr (BM) {
        bm_i++;
        if (bm_i == a.nb) { bm_i = 0; bm_b++; }
      }
    }
    uint32_t v[N * GQ], shb[N * GQ], cnt[N * GQ], acc_at[N * GQ];
#pragma unroll
    for (int u = 0; u < N; u++)
#pragma unroll
      for (int g = 0; g < GQ; g++) {
        const int s = u * GQ + g;
        int ri, ci;
        if constexpr (FAC) cell_fac(dir[u], rr_[u][g], ri, ci);
        else cell(tt[u][2 * g], tt[u][2 * g + 1], ri, ci);
        issue(dd[u][g], ri, ci, v[s], shb[s], cnt[s], acc_at[s]);
      }
#pragma unroll
    for (int s = 0; s < N * GQ; s++) consume(v[s], shb[s], cnt[s], acc_at[s]);
  };
  uint32_t nb_mine = 0;   // COMPACT: B entries of this wave's sectors
  if constexpr (COMPACT) {
    // phase 1: the A lists of this wave's sectors
    const int ngroups = a.nb / RAY_PG, sectors_all = a.blocks * ngroups;
    const int sper = (sectors_all + a.nsplit - 1) / a.nsplit;
    const int s0 = part_id * sper, s1 = min(sectors_all, s0 + sper);
    int seg = s0 / ngroups, pg = s0 - seg * ngroups;
    // (a sector's counts are read one sector ahead: nothing waits for them)
    int4 tn = s0 < s1 ? *reinterpret_cast<const int4*>(a.ctab + (int64_t)s0 * 16 + 12) : make_int4(0, 0, 0, 0);
    for (int sc = s0; sc < s1; sc++) {
      const int n_a = tn.x + tn.y;
      nb_mine += (uint32_t)(tn.z + tn.w);
      tn = *reinterpret_cast<const int4*>(a.ctab + (int64_t)min(sc + 1, s1 - 1) * 16 + 12);
      const uint4* __restrict__ lst = reinterpret_cast<const uint4*>(a.clist + (int64_t)sc * RAY_CL_WORDS);
      const int dbase = (pg * RAY_PG - shift + a.nb) * 8, rbase = seg * 65 * 4;   // byte offsets into ldir, lrad
      const unsigned pbase_a = a.planes_off + pconst - a.plane_bytes;                // class code c + 1: plane c
      auto step_a = [&](auto cnt_c, int e0) {
        constexpr int N = decltype(cnt_c)::value;
        uint32_t w[N], v[N];
        ray_list_load<N>(lst, e0, lane, w);
#pragma unroll
        for (int u = 0; u < N; u++) {
          const float2 dv = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(ldir) + dbase + (w[u] >> 25));
          const float rad = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(lrad) + rbase + ((w[u] >> 16) & 0x1FFu));
          int ri, ci;
          cell_fac((tdr_v2f){dv.x, dv.y}, rad, ri, ci);
          // an A entry has ONE class: its plane, cells as they are, `known` in bit 15 — nothing out of the class table
          const unsigned off = plane_offset(ri, ci, a.pkcol, (int)(pbase_a + ((w[u] >> 12) & 0xFu) * a.plane_bytes));
          v[u] = *reinterpret_cast<const uint16_t*>(crecb + off);
        }
#pragma unroll
        for (int u = 0; u < N; u++) {
          const uint32_t kbit = v[u] >> 15, cnt = w[u] & 0xFFFu;
          known += kbit;
          norm = __umul24(cnt, kbit) + norm;                  // state_particle.cpp:141-142
          const uint32_t D = int_dict_at(ldict, v[u]);
          unsigned long long* const acc = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(my) + ((w[u] >> 3) & 0x1E00u));
          __hip_atomic_fetch_add(acc, (unsigned long long)cnt * D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      };
      // up to 16 gathers (the last one may be part of one) in one or two steps of up to 8 in flight together; a step starts at
      // a block of 256 entries, and neither is left with a single gather to wait for alone
      int e = 0, left = (n_a + 63) >> 6;
      if (left > 12) { step_a(std::integral_constant<int, 8>{}, 0); e = 512; left -= 8; }
      else if (left > 8) { step_a(std::integral_constant<int, 4>{}, 0); e = 256; left -= 4; }
      switch (left) {
        case 8: step_a(std::integral_constant<int, 8>{}, e); break;
        case 7: step_a(std::integral_constant<int, 7>{}, e); break;
        case 6: step_a(std::integral_constant<int, 6>{}, e); break;
        case 5: step_a(std::integral_constant<int, 5>{}, e); break;
        case 4: step_a(std::integral_constant<int, 4>{}, e); break;
        case 3: step_a(std::integral_constant<int, 3>{}, e); break;
        case 2: step_a(std::integral_constant<int, 2>{}, e); break;
        case 1: step_a(std::integral_constant<int, 1>{}, e); break;
        default: break;
      }
      pg++;
      if (pg == ngroups) { pg = 0; seg++; }
    }
  } else if constexpr (PATCH) {
    // the patch order (top of the file): a wave takes a contiguous share of the SECTORS (segment of 64 rings, group of 16 scan
    // rows); a sector = the segment's four ring blocks = four units of four steps; two units' gathers are in flight together
    const int ngroups = a.nb / RAY_PG, sectors_all = a.blocks * ngroups;
    const int sper = (sectors_all + a.nsplit - 1) / a.nsplit;
    const int s0 = part_id * sper, s1 = min(sectors_all, s0 + sper);
    const int pl_d = lane >> 4, pl_r = lane & (RAY_PR - 1);
    const uint2* __restrict__ descq = reinterpret_cast<const uint2*>(a.desc_ray);
    int seg = s0 / ngroups, pg = s0 - seg * ngroups;
    for (int sc = s0; sc < s1; sc++) {
      // the window directions of the sector's four steps: scan row 16 pg + 4 k + (lane >> 4) meets direction (row - shift) mod nb
      int wi[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        int i = pg * RAY_PG + 4 * k + pl_d - shift;
        i += i < 0 ? a.nb : 0;
        wi[k] = i;
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        uint2 dd[2];
#pragma unroll
        for (int u = 0; u < 2; u++) dd[u] = descq[((int64_t)(seg * 4 + 2 * h + u) * ngroups + pg) * 64 + lane];
        uint32_t v[8], shb[8], cnt[8], acc_at[8];
#pragma unroll
        for (int u = 0; u < 2; u++)
#pragma unroll
          for (int k = 0; k < 4; k++) {
            int ri, ci;
            {   // (the table is not its factors' products: its own entries, in its own order)
              const int j = min((seg * 4 + 2 * h + u) * RAY_PR + pl_r, a.nr - 1);
              const int64_t kk = (int64_t)j * a.nb + wi[k];
              if ((seg * 4 + 2 * h + u) * RAY_PR + pl_r < a.nr) cell(a.tab[2 * kk], a.tab[2 * kk + 1], ri, ci);
              else cell(-1.0e30f, -1.0e30f, ri, ci);
            }
            const uint32_t w = k < 2 ? dd[u].x : dd[u].y;
            issue((k & 1) ? (w >> 16) : (w & 0xFFFFu), ri, ci, v[u * 4 + k], shb[u * 4 + k], cnt[u * 4 + k], acc_at[u * 4 + k]);
          }
#pragma unroll
        for (int t = 0; t < 8; t++) consume(v[t], shb[t], cnt[t], acc_at[t]);
      }
      pg++;
      if (pg == ngroups) { pg = 0; seg++; }
    }
  } else {
    int m = m0;
    for (; m + U <= m1; m += U) rows_step(std::integral_constant<int, U>{}, m);
    for (; m < m1; m++) rows_step(std::integral_constant<int, 1>{}, m);
  }

  // the list: bins that hold several classes, or one large count (ray_list_pass)
  ray_list_pass(a, part_id, lane, crecb, ldict, my, norm, [&](uint32_t w, int& ri, int& ci) -> int64_t {
    const int r = (int)(w >> 16), j = (int)(w & 0xFFFFu);
    int i = r - shift;   // the window row that meets scan row r
    i += i < 0 ? a.nb : 0;
    const int64_t k = (int64_t)j * a.nb + i;
    cell(a.tab[2 * k], a.tab[2 * k + 1], ri, ci);
    return (int64_t)j * a.nb + r;
  });
  // phase 2 (COMPACT): the gate count — see the invariant above ray_body
  if constexpr (COMPACT) {
#pragma unroll
    for (int dlt = 32; dlt > 0; dlt >>= 1) known += __shfl_xor(known, dlt, 64);   // (every lane: the wave's phase-1 count)
    const uint32_t P = (uint32_t)((int64_t)a.nb * a.nr);   // (read only where gate_shared: below 2^24)
    uint32_t* const g = lgate[gate_shared ? wave - part_id : 0];   // the particle's words (gate_shared: part_id = wave mod nsplit)
    uint32_t tot_a = known, nb_all = nb_mine;
    if (gate_shared && a.nsplit > 1) {
      if (lane == 0) {
        atomicAdd(&g[0], known);
        atomicAdd(&g[1], nb_mine);
      }
      __syncthreads();   // the one barrier: every wave of the workgroup, idle ones included, arrives once
      tot_a = *reinterpret_cast<volatile uint32_t*>(&g[0]);   // (no wave adds to these two words behind the barrier)
      nb_all = *reinterpret_cast<volatile uint32_t*>(&g[1]);
    }
    const bool settled = gate_shared && (2 * tot_a >= P || 2 * (tot_a + nb_all) < P);
    uint32_t known_b = 0, blocks_b = 0;
    bool early = false;
    if (!settled) {
      const int ngroups = a.nb / RAY_PG, sectors_all = a.blocks * ngroups;
      const int sper = (sectors_all + a.nsplit - 1) / a.nsplit;
      const int s0 = part_id * sper, s1 = min(sectors_all, s0 + sper);
      int seg = s0 / ngroups, pg = s0 - seg * ngroups;
      const uint4 em = lut[0];   // the coarse mask plane: a B entry needs its cell's known bit and nothing else
      for (int sc = s0; sc < s1 && !early; sc++) {
        const int32_t* __restrict__ tb = a.ctab + (int64_t)sc * 16;
        const int n_a = tb[12] + tb[13], n_b = tb[14] + tb[15];
        const uint4* __restrict__ lst = reinterpret_cast<const uint4*>(a.clist + (int64_t)sc * RAY_CL_WORDS + ((n_a + 255) >> 8) * 256);
        const int dbase = (pg * RAY_PG - shift + a.nb) * 8, rbase = seg * 65 * 4;
        auto step_b = [&](auto cnt_c, int e0) {   // known cells among N x 64 entries (wave-uniform)
          constexpr int N = decltype(cnt_c)::value;
          uint32_t w[N], v[N], shb[N];
          ray_list_load<N>(lst, e0, lane, w);
#pragma unroll
          for (int u = 0; u < N; u++) {
            const float2 dv = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(ldir) + dbase + (w[u] >> 25));
            const float rad = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(lrad) + rbase + ((w[u] >> 16) & 0x1FFu));
            int ri, ci;
            cell_fac((tdr_v2f){dv.x, dv.y}, rad, ri, ci);
            const unsigned off = plane_offset(ri >> (int)em.y, ci >> (int)em.y, a.pkcol, (int)em.x);
            shb[u] = (((uint32_t)ri & 3u) << 2) | ((uint32_t)ci & 3u);
            v[u] = *reinterpret_cast<const uint16_t*>(crecb + off);
          }
          uint32_t c = 0;
#pragma unroll
          for (int u = 0; u < N; u++) c += (uint32_t)__popcll(__ballot((v[u] >> shb[u]) & 1u));
          return c;
        };
        for (int e = 0; e < n_b && !early; e += 256) {
          const int left = (n_b - e + 63) >> 6;
          uint32_t c = 0;
          if (left >= 4) c = step_b(std::integral_constant<int, 4>{}, e);
          else if (left == 3) c = step_b(std::integral_constant<int, 3>{}, e);
          else if (left == 2) c = step_b(std::integral_constant<int, 2>{}, e);
          else c = step_b(std::integral_constant<int, 1>{}, e);
          known_b += c;
          blocks_b++;
          if (gate_shared) {
            uint32_t tot_b = known_b;
            if (a.nsplit > 1) {   // the particle's running count: this block's bits in, the total so far out
              uint32_t old = 0;
              if (lane == 0) old = atomicAdd(&g[2], c);
              tot_b = (uint32_t)__builtin_amdgcn_readfirstlane((int)old) + c;
            }
            early = 2 * (tot_a + tot_b) >= P && (e + 256 < n_b || sc + 1 < s1);
          }
        }
        pg++;
        if (pg == ngroups) { pg = 0; seg++; }
      }
      known += known_b;
    }
    if (a.gate_ctr && lane == 0) {   // (profiling) the particle's outcome, by the last of its waves to arrive here
      if (blocks_b) atomicAdd(&a.gate_ctr[3], blocks_b);
      if (!gate_shared) {
        if (part_id == 0) atomicAdd(&a.gate_ctr[2], 1u);
      } else {
        const uint32_t mine = 1u + (settled ? 0u : 0x100u) + (early ? 0x10000u : 0u);
        const uint32_t all = atomicAdd(&g[3], mine) + mine;
        if ((all & 0xFFu) == (uint32_t)a.nsplit) atomicAdd(&a.gate_ctr[(all >> 16) ? 1 : ((all & 0xFF00u) ? 2 : 0)], 1u);
      }
    }
  }
  // (the rings a block pads a direction with fell on the guard cell — unknown — and counted nothing; COMPACT: phase 2 left
  // the wave's known count in every lane)
  ray_add_sums<COMPACT>(a.part, a.npad, slot, a.ncls, lane, my, known, norm);
}
TDR_TL_BUFFER(g_timeline_ray, tdr_debug_read_timeline_ray)   // (diagnostic build only: tdr_score_dev.h)
template <int GQ, bool USCALE, bool BM = false, bool PATCH = false>
__global__ __launch_bounds__(256) void score_polar_ray_kernel(RayArgs a) {
  extern __shared__ unsigned long long lacc[];
  __shared__ uint32_t ldict[TDR_CMAP_MAX_DICT];
  __shared__ uint4 lut[16];
  __shared__ float2 ldir[PATCH ? 2 * RAY_PATCH_MAX_NB + RAY_PG : 1];
  __shared__ uint32_t lgate[4][4];
  if (int_form_off(a.inexact)) return;
#ifdef TDR_SCORE_TIMELINE
  if ((int64_t)blockIdx.x * 4 >= (int64_t)a.counts[1] * a.nsplit) return;   // no stamps for an idle workgroup (ray_body's own test)
#endif
  TDR_TL_BEGIN(g_timeline_ray)
  // with factors that ARE the table's (score_prep_kernel's check; uniform over the launch) the offsets are multiplied out
  if (a.fac && a.inexact[2] == 0) ray_body<GQ, USCALE, true, BM, PATCH>(a, lacc, ldict, lut, ldir, lgate);
  else ray_body<GQ, USCALE, false, BM, PATCH>(a, lacc, ldict, lut, ldir, lgate);
  TDR_TL_END(g_timeline_ray)   // (ray_body's waves return from IT: every thread of a live workgroup arrives here)
}


// ---- host side ---------------------------------------------------------------------------------------------------------

bool tdr_ray_map_ok(const tdr_map_desc* map) {
  return map->crec && map->dict && map->cwords == tdr_cmap_words(map->ncls) && map->dict_n > 0 &&
         map->dict_n <= TDR_CMAP_MAX_DICT && tdr_cmap_plane_words(map->ncls, map->rows, map->cols) != 0;
}
int tdr_ray_splits(int nb, int nr, int64_t n, bool bm) {
  if (tdr_cfg().ray_split > 0) return tdr_cfg().ray_split;   // forced (tdr_config_ray_split)
  // waves per particle: a window is nb * blocks rows of up to four steps; small launches split it to fill the chip (the
  // sums are exact: any split gives the same bits)
  const int64_t rows = (int64_t)nb * ray_blocks(nr, bm);
  int s = 1;
  while (s < TDR_RAY_MAX_SPLIT && n * s < 32768 && rows / (2 * s) >= 8) s *= 2;
  if (s == 1 && rows >= 128) s = 2;
  // (config 2, 100 000 uniform particles at a span of 8, ms per call at 1 / 2 / 4 / 8 waves per particle — block-major:
  // 8.42 / 8.36 / 8.33 / 8.69; the first order: 10.35 / 10.42 / 10.35 / 9.66; the bench mix moves by 1 % at most)
  if (s == 2 && bm && rows >= 512) s = 4;
  if (s == 2 && !bm && rows >= 256) s = 8;
  return s;
}

int tdr_ray_score(const SuLaunch& L, const SuWs& W, hipStream_t s) {
  const tdr_map_desc* map = L.map;
  int32_t* base = L.ws;
  int* ints = base + W.ints + 3 * (L.nb + 1);
  RayArgs r;
  r.crec = map->crec;
  const size_t pw = tdr_cmap_plane_words(map->ncls, map->rows, map->cols);
  r.planes_off = (unsigned)(tdr_cmap_plane_offset_words(map->ncls, map->rows, map->cols) * 4);
  r.plane_bytes = (unsigned)(pw * 4);
  r.cmask_off = r.planes_off + (unsigned)map->ncls * r.plane_bytes;
  r.pkcol = plane_trows(map->rows) * 128 - 16;
  r.dict_int = reinterpret_cast<const uint32_t*>(map->dict) + TDR_CMAP_MAX_DICT;
  r.dict_n = map->dict_n;
  r.rows = map->rows; r.cols = map->cols; r.resolution = map->resolution;
  r.tab = L.tab;
  r.tab_ray = reinterpret_cast<const float*>(base + W.ray_tab);
  r.fac = L.fac;
  r.rad_ray = reinterpret_cast<const float*>(base + W.ray_rad);
  r.uscale = L.uscale;
  r.desc_ray = reinterpret_cast<const uint16_t*>(base + W.ray_desc);
  r.list = reinterpret_cast<const uint32_t*>(base + W.ray_multi);
  r.n_list = ints + 3;
  r.scan_pk = L.scan_pk;
  r.rf = L.rf; r.ncls = map->ncls; r.nb = L.nb; r.nr = L.nr; r.blocks = ray_blocks(L.nr, ray_bm(L)); r.res = L.res;
  r.st = L.st; r.cap = L.cap;
  r.slots = base + W.slots;
  r.counts = ints;
  r.inexact = ints + 4;
  r.nsplit = L.ray_split;
  r.npad = L.npad;
  r.part = reinterpret_cast<uint32_t*>(L.part);
  r.clist = reinterpret_cast<const uint32_t*>(base + W.ray_clist);
  r.ctab = base + W.ray_ctab;
  r.gate_ctr = ray_patch(L) ? tdr_profile_gate_ptr() : nullptr;
  const dim3 grid((unsigned)cdiv(L.n * r.nsplit, 4)), block(256);
  // the lanes' accumulators; behind them, in the patch order, the rings' radii
  const size_t lds = (size_t)4 * (map->ncls + 1) * 64 * sizeof(unsigned long long) + (ray_patch(L) ? (size_t)r.blocks * 65 * sizeof(float) : 0);
#define TDR_LAUNCH_RAY(GQ)                                                                            \
  if (L.uniform_scale) hipLaunchKernelGGL((score_polar_ray_kernel<GQ, true>), grid, block, lds, s, r); \
  else hipLaunchKernelGGL((score_polar_ray_kernel<GQ, false>), grid, block, lds, s, r);
  if (ray_patch(L)) {
    if (L.uniform_scale) hipLaunchKernelGGL((score_polar_ray_kernel<1, true, true, true>), grid, block, lds, s, r);
    else hipLaunchKernelGGL((score_polar_ray_kernel<1, false, true, true>), grid, block, lds, s, r);
  } else if (ray_bm(L)) {
    if (L.uniform_scale) hipLaunchKernelGGL((score_polar_ray_kernel<1, true, true>), grid, block, lds, s, r);
    else hipLaunchKernelGGL((score_polar_ray_kernel<1, false, true>), grid, block, lds, s, r);
  } else switch (ray_gq(L.nr, false)) {
    case 1: TDR_LAUNCH_RAY(1) break;
    case 2: TDR_LAUNCH_RAY(2) break;
    default: TDR_LAUNCH_RAY(4) break;
  }
#undef TDR_LAUNCH_RAY
  LAUNCH_CHECK("score_polar_ray");
  return TDR_OK;
}
