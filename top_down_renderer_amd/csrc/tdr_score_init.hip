// tdr_score_init.hip — the 40-rotation init search of state_particle.cpp:195-206: the vector kernel, the three matrix-core
// kernels (on the fly, wide records, pre-split half records) and the host function that picks among them
// (tdr_score_init.h).  Built with -amdgpu-mfma-vgpr-form (build.py): the only file that issues MFMAs.
#include <algorithm>
#include <cstring>
#include <vector>

#include "tdr_batch.h"       // batch_find
#include "tdr_common.h"
#include "tdr_score_dev.h"   // rot_shift_dev, the coordinate rounding, the gates
#include "tdr_score_init.h"

// The 40-rotation initialisation search of state_particle.cpp:195-206 in ONE pass over the window: the candidate
// rotations are the same for every particle, so for rotation t the scan row paired with window row i — (i + s_t) mod nb
// — is the same for all lanes, and a map record gathered once is multiplied against all candidates' scan records
// (the reference also gathers once and scores 40 times).  One workgroup = one batch of 64 particles; its INIT_WAVES waves
// split the candidates (INIT_TW each), gather the same records (the repeats hit L1) and keep INIT_TW x rf accumulators
// per lane.  A ring of the packed scan is staged in LDS twice over (rows r and r + nb hold scan row r), so the record of
// candidate t at window row i sits at row i + s_t without a wrap, the same address in every lane: an LDS broadcast.
// Sums run in float over the whole window, which is only used to pick the best rotation: the weight itself is then
// produced by the regular scoring pass at that rotation.
#define INIT_TW 6          // candidate rotations per wave
#define INIT_WAVES 8       // waves per workgroup, all on the same 64 particles (A/B on MI355X, 250k particles:
                           // 4x11 401 ms, 6x8 630 ms, 8x6 285 ms, 12x4 422 ms, 16x3 447 ms; scalar-cache scan reads 773 ms)
#define INIT_MAXROT (INIT_WAVES * INIT_TW)
struct InitArgs {
  const float* rec;
  int rows, cols;
  float resolution;
  const float* tab;
  const float* utab;
  const float* scan_pk;
  int nb, nr;
  float res;
  const float* st;     // read-only here: results go to res_theta / res_flag (keeps every other load scalarisable)
  int64_t cap, n;
  const int32_t* order;
  tdr_filter_params fp;
  GateArgs gate;
  int64_t P;
  int ncls;
  const int* nrot;
  const int* shift;    // [nrot] device arrays (filled by init_rot_kernel)
  const float* theta;
  const int* only_if;  // optional: the kernel runs only when this device word is non-zero (fallback after the MFMA pass)
  float* res_theta;  // [n] chosen rotation
  float* res_flag;   // [n] 0 = untouched, 1 = initialised, 2 = initialised but every rotation scored NaN
                     //     (weight 1/(FLT_MAX + reg), state_particle.cpp:193,212)
  uint32_t* stats;   // NULL, or (tdr_profile_enable(2)) the 16 counters of tdr_profile_variants: every workgroup that
                     // writes results adds one to its pass's slot — [12] half records, [13] on the fly, [14] wide, [15] vector
};
// one atomic per workgroup, where its results are written (a workgroup that left early wrote none and counts nothing)
__device__ __forceinline__ void init_count_pass(const InitArgs& a, int slot) {
  if (a.stats && threadIdx.x == 0) atomicAdd(a.stats + slot, 1u);
}
// The matrix-core passes take the weighted distances 0.01 w_c d_c as f16 pairs hi + lo.  lo is exact only while it stays a
// normal f16 (>= 2^-14; below that its step is 2^-24 whatever its size), so every 0.01 w_c is first multiplied by ONE
// power of two that brings the largest of them into [1, 2): exact, the same factor on every candidate's cost — the minimum
// does not move — and with the map's distances (at most 50) far from f16's range at the other end.  An operand
// v = w_c' d_c >= 2^-4 then has hi + lo within 2^-20 of it (relative).
__device__ __forceinline__ float init_weight_pow2(const tdr_filter_params& fp, int ncls) {
  float mx = 0.f;
#pragma unroll
  for (int c = 0; c < TDR_MAX_CLASSES; c++)
    if (c < ncls) mx = fmaxf(mx, fabsf((float)(0.01 * (double)fp.class_weights[c])));
  if (!(mx > 0.f) || !(mx <= 3.402823466e+38f)) return 1.f;
  int e;
  (void)frexpf(mx, &e);   // mx = f * 2^e, f in [0.5, 1)
  return ldexpf(1.f, min(max(1 - e, -100), 100));
}

// ---- what the kernel bodies share ---------------------------------------------------------------------------------------
typedef _Float16 tdr_h8 __attribute__((ext_vector_type(8)));
typedef __fp16 tdr_h2 __attribute__((ext_vector_type(2)));   // what v_cvt_pkrtz_f16_f32 returns
typedef float tdr_f4 __attribute__((ext_vector_type(4)));
typedef float tdr_f2 __attribute__((ext_vector_type(2)));
#define INITM_TILES 3   // matrix-core kernels: 48 candidate rows >= the 40 (41) rotations of the search
static_assert(INITM_TILES * 16 >= INIT_MAXROT || INIT_MAXROT == 48, "rotation tiles");

// The particle of a lane: slot `slot` of the filter's order (a slot past the end reads particle 0 and wants nothing).
struct InitLane {
  int64_t p;
  float scale, cx, cy;
  bool valid, want;   // want: no heading yet and not gated — the search writes this particle's result
};
__device__ __forceinline__ InitLane init_lane(const InitArgs& a, int64_t slot) {
  InitLane l;
  l.valid = slot < a.n;
  l.p = a.order ? (int64_t)a.order[l.valid ? slot : 0] : (l.valid ? slot : 0);
  l.scale = a.st[TDR_ST_SCALE * a.cap + l.p];
  l.cx = a.st[TDR_ST_DX * a.cap + l.p] * l.scale + a.st[TDR_ST_INIT_X * a.cap + l.p];
  l.cy = a.st[TDR_ST_DY * a.cap + l.p] * l.scale + a.st[TDR_ST_INIT_Y * a.cap + l.p];
  l.want = l.valid && a.st[TDR_ST_HAVE_INIT * a.cap + l.p] == 0.f && !particle_gated(a.gate, l.cx, l.cy, l.scale);
  return l;
}
// Byte offset of the dense record (RB bytes) that sample-table entry t reads for a particle of scale `scale` centred at
// (off0, off1) cells: top_down_map_polar.cpp:28-31, the one place where the search and the scoring kernels must agree on
// the cell.  The grid is guarded by one ring of cells; a sample outside it reads the record at offset 0.
template <bool USCALE, int RB>
__device__ __forceinline__ unsigned init_cell_offset(const InitArgs& a, float scale, float off0, float off1, float2 t) {
  float p0, p1;
  if constexpr (USCALE) { p0 = t.x; p1 = t.y; }
  else { p0 = (t.x * scale) * a.res; p1 = (t.y * scale) * a.res; }   // :28
  auto cell = [](float v, float vmax) { return round_half_away_clamped(__builtin_amdgcn_fmed3f(v, -1.f, vmax)); };   // :31
  const int ri = cell(p0 + off0, (float)a.rows), ci = cell(p1 + off1, (float)a.cols);
  const bool inb = (unsigned)ri < (unsigned)a.rows && (unsigned)ci < (unsigned)a.cols;
  return inb ? (unsigned)(__mul24(ri, (a.cols + 2) * RB) + (ci * RB + (a.cols + 3) * RB)) : 0u;
}
// res_theta / res_flag of particle p: candidate bt won, or none did (bt < 0)
__device__ __forceinline__ void init_write_choice(const InitArgs& a, int64_t p, int bt) {
  a.res_theta[p] = bt >= 0 ? a.theta[bt] : 0.f;  // state_particle.cpp:205 (best_theta stays 0 if nothing won)
  a.res_flag[p] = bt < 0 ? 2.f : 1.f;
}
// The end of a matrix-core body.  Lane (col, q) holds rows 4q..4q+3 of every tile for particle `col` — candidate
// 16 T + 4 q + r has the cost accC[T][r] / div(T, r) — and `known` is its share of the particle's known samples (the four
// lanes of a particle share the samples).  Picks the first strict minimum in rotation order, writes it and counts the
// workgroup in slot `stat` of the pass counters.
template <class Div>
__device__ __forceinline__ void init_pick_write(const InitArgs& a, const InitLane& l, int q, int nrot, float known,
                                                const tdr_f4 (&accC)[INITM_TILES], Div div, int stat) {
  known += __shfl_xor(known, 16, 64);
  known += __shfl_xor(known, 32, 64);
  const bool unknown = (known / (float)a.P) < 0.5;   // state_particle.cpp:117-120
  float best = 3.402823466e+38f;
  int bm = -1;
#pragma unroll
  for (int T = 0; T < INITM_TILES; T++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int m = 16 * T + 4 * q + r;
      float cost = accC[T][r] / div(T, r);              // :154
      if (unknown) cost = __builtin_nanf("");
      if (m < nrot && cost < best) { best = cost; bm = m; }   // :200-203 (NaN never wins)
    }
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {   // first minimum in rotation order over the particle's four lanes
    const float oc = __shfl_xor(best, o, 64);
    const int om = __shfl_xor(bm, o, 64);
    const bool take = om >= 0 && (bm < 0 || oc < best || (oc == best && om < bm));
    if (take) { best = oc; bm = om; }
  }
  if (q == 0 && l.want) init_write_choice(a, l.p, bm);
  init_count_pass(a, stat);
}
// the filter's "scan count does not fit f16" word: behind its rotation count (the layout: make_init_args)
__device__ __forceinline__ int* init_inexact_word(const InitArgs& a) { return const_cast<int*>(a.nrot) + 1; }
// x, y as f16 pairs hi + lo (see init_weight_pow2)
__device__ __forceinline__ void init_split_pair(float x, float y, tdr_h2& hi, tdr_h2& lo) {
  hi = __builtin_amdgcn_cvt_pkrtz(x, y);
  lo = __builtin_amdgcn_cvt_pkrtz(x - (float)hi[0], y - (float)hi[1]);
}
// 8 scan counts as one LDS row of 8 x f16; `big` is raised by a count f16 does not hold exactly (above 2048)
__device__ __forceinline__ uint4 init_pack_scan8(const float* f, bool& big) {
  union { tdr_h2 h[4]; uint4 u; } pk;
#pragma unroll
  for (int k = 0; k < 8; k++) big |= f[k] > 2048.f;
#pragma unroll
  for (int c = 0; c < 4; c++) pk.h[c] = __builtin_amdgcn_cvt_pkrtz(f[2 * c], f[2 * c + 1]);
  return pk.u;
}

// Each search kernel is a body (bx: the workgroup's index among its filter's batches of 64 particles) behind two wrappers:
// the standalone kernel passes its kernel arguments and blockIdx.x, the batched one (tdr_batch_step) finds
// its filter from blockIdx.x and reads that filter's InitArgs from a device table — the index is wave-uniform and the
// entry is read before anything is stored, so its fields arrive through scalar loads as kernel arguments do.
// Records of 16 floats: one workgroup per CU fits, two waves per SIMD, whatever the schedule — the kernels say so, and the
// scheduler spends the registers on LDS reads in flight (15 per row; aiming at a third wave it kept one or two: +9 % time).
// Only NV4 == 4 is constrained: 1 to 8 waves is what the other forms have anyway.
#define INIT_WAVES_PER_SIMD(NV4) __attribute__((amdgpu_waves_per_eu(NV4 == 4 ? 2 : 1, NV4 == 4 ? 2 : 8)))
template <int NV4, bool KSLOT, bool USCALE>
__device__ __forceinline__ void score_init_body(const InitArgs& a, int bx) {
  constexpr int RF = 4 * NV4;
  extern __shared__ float4 ring[];  // [NV4 planes][2*nb rows]
  const int nb2 = 2 * a.nb;
  __shared__ float x_cost[INIT_WAVES][64];
  __shared__ int x_rot[INIT_WAVES][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform, and the compiler knows it
  if (a.only_if && *a.only_if == 0) return;               // (uniform) the MFMA pass already produced the results
  const InitLane l = init_lane(a, (int64_t)bx * 64 + lane);   // all waves work on the same 64 particles
  // every wave of the workgroup looks at the same 64 particles, so this per-wave vote is the same in all of them
  // (and, unlike __syncthreads_or, involves no LDS atomic that would stop the compiler from using scalar loads)
  if (__ballot(l.want) == 0) return;  // nothing to initialise in this batch
  const float off0 = l.cy / a.resolution, off1 = l.cx / a.resolution;
  const char* __restrict__ recb = reinterpret_cast<const char*>(a.rec);
  const float2* __restrict__ tab2 = reinterpret_cast<const float2*>(USCALE ? a.utab : a.tab);
  const float4* __restrict__ scan4 = reinterpret_cast<const float4*>(a.scan_pk);
  const int nrot = *a.nrot;
  int sh[INIT_TW];
#pragma unroll
  for (int r = 0; r < INIT_TW; r++) {
    const int t = wave * INIT_TW + r;
    sh[r] = t < nrot ? a.shift[t] : 0;
  }
  tdr_f2 acc[INIT_TW][RF / 2];   // slot pairs: the packed FMA's operands by construction
#pragma unroll
  for (int r = 0; r < INIT_TW; r++)
#pragma unroll
    for (int k = 0; k < RF / 2; k++) acc[r][k] = (tdr_f2){0.f, 0.f};
  float known = 0.f;

  for (int j = 0; j < a.nr; j++) {
    const float2* trow = tab2 + (int64_t)j * a.nb;
    const float4* srow = scan4 + (int64_t)j * a.nb * NV4;  // ring j of the packed scan
    __syncthreads();
    for (int t = threadIdx.x; t < a.nb * NV4; t += 64 * INIT_WAVES) {
      const float4 v = srow[t];
      const int row = t / NV4, pl = t - row * NV4;
      ring[pl * nb2 + row] = v;
      ring[pl * nb2 + row + a.nb] = v;
    }
    __syncthreads();
    for (int i = 0; i < a.nb; i++) {
      const unsigned boff = init_cell_offset<USCALE, RF * 4>(a, l.scale, off0, off1, trow[i]);
      float4 m[NV4];
#pragma unroll
      for (int v = 0; v < NV4; v++) m[v] = *reinterpret_cast<const float4*>(recb + boff + 16 * v);
      if (!KSLOT) known += m[NV4 - 1].w;
#pragma unroll
      for (int r = 0; r < INIT_TW; r++) {
#pragma unroll
        for (int v = 0; v < NV4; v++) {
          const float4 sv = ring[v * nb2 + sh[r] + i];  // same address in every lane: LDS broadcast
          acc[r][2 * v] = __builtin_elementwise_fma((tdr_f2){sv.x, sv.y}, (tdr_f2){m[v].x, m[v].y}, acc[r][2 * v]);
          acc[r][2 * v + 1] = __builtin_elementwise_fma((tdr_f2){sv.z, sv.w}, (tdr_f2){m[v].z, m[v].w}, acc[r][2 * v + 1]);
        }
      }
    }
  }
  // cost of each candidate (state_particle.cpp:117-120,136-139,154), best of this wave's candidates in order
  const float kn = KSLOT ? acc[0][RF / 2 - 1][0] : known;
  const bool unknown = (kn / (float)a.P) < 0.5;
  float cw[RF];
#pragma unroll
  for (int k = 0; k < RF; k++) cw[k] = k < 16 ? a.fp.class_weights[k < 16 ? k : 0] : 0.f;
  float best = 3.402823466e+38f;
  int best_t = -1;
#pragma unroll
  for (int r = 0; r < INIT_TW; r++) {
    const int t = wave * INIT_TW + r;
    float cost = 0.f;
#pragma unroll
    for (int k = 0; k < RF - 1; k++)   // constant indices only: a dynamic index would push the arguments to scratch
      if (k < a.ncls) cost = (float)((double)cost + (double)acc[r][k / 2][k % 2] * 0.01 * (double)cw[k]);
    cost = cost / acc[r][RF / 2 - 1][1];
    if (unknown) cost = __builtin_nanf("");
    if (t < nrot && cost < best) { best = cost; best_t = t; }  // :200-203 (NaN never wins)
  }
  x_cost[wave][lane] = best;
  x_rot[wave][lane] = best_t;
  __syncthreads();
  if (wave == 0 && l.want) {
    float b = 3.402823466e+38f;
    int bt = -1;
    for (int wv = 0; wv < INIT_WAVES; wv++)   // waves hold the candidates in loop order: strict '<' keeps the first minimum
      if (x_cost[wv][lane] < b) { b = x_cost[wv][lane]; bt = x_rot[wv][lane]; }
    init_write_choice(a, l.p, bt);
  }
  init_count_pass(a, 15);
}
template <int NV4, bool KSLOT, bool USCALE>
__global__ __launch_bounds__(64 * INIT_WAVES) INIT_WAVES_PER_SIMD(NV4)
void score_init_kernel(InitArgs a) {
  score_init_body<NV4, KSLOT, USCALE>(a, (int)blockIdx.x);
}
// Batched wrappers: entry e of `args` owns the blocks [blk[e], blk[e + 1]) counted from blk[0] (the launch covers a run of
// the batch's table, `blk` is the cumulative count over the whole table).  A filter whose USCALE differs from the
// instantiation's is another launch over the same run.
// (The entry's pointers are generic ones to the compiler, so the gathers through them are flat loads where the standalone
// kernels issue global loads — as in score_polar_batch_kernel.)
#define INIT_BATCH_FIND()                                                                    \
  const int b = (int)blockIdx.x + blk[0];                                                    \
  const int e = batch_find(k, b, [&](int i) { return blk[i]; });                             \
  const InitArgs a = args[e];                                                                \
  if ((a.utab != nullptr) != USCALE) return; /* (uniform) */                                 \
  const int bx = b - blk[e]
template <int NV4, bool KSLOT, bool USCALE>
__global__ __launch_bounds__(64 * INIT_WAVES) INIT_WAVES_PER_SIMD(NV4)
void score_init_batch_kernel(const InitArgs* __restrict__ args, const int32_t* __restrict__ blk, int k) {
  INIT_BATCH_FIND();
  score_init_body<NV4, KSLOT, USCALE>(a, bx);
}

// The same search on the matrix cores (records of 8 floats, i.e. 4-6 classes).  For one particle the 40 candidate
// costs are  cost[m] = sum_{i,j,c} scan_c[(i + s_m) mod nb, j] * (w_c d_c[cell(i,j)]):  a contraction over
// k = (sample, class) of a matrix A[m][k] that is the same for every particle (shifted scan records, from LDS) with
// the particle's gathered window B[k][n].  v_mfma_f32_16x16x32_f16: 16 rotations x 16 particles x (4 samples x 8
// record slots) per instruction.  Lane l holds, as its B fragment, the 8 slots of the record of particle l&15 at
// sample 4t + (l>>4) — exactly the record it gathered — and as its A fragment the packed scan record at row
// (4t + (l>>4) + s_m), m = l&15 (+16, +32 for the second and third tile of candidates), one ds_read_b128 each.
//   * scan counts are integers: exact in f16 up to 2048 (a larger count raises the filter's "does not fit f16" word,
//     a.nrot[1], and score_init_kernel redoes the search on the vector units);
//   * distances (times 0.01 w_c, in f32, times the one power of two of init_weight_pow2) are split hi + lo into two f16
//     (relative error <= 2^-20 from 2^-4 up, see there), two MFMAs;
//   * the normalisation  sum scanΣ * known  is a third MFMA with only slot 7 of B set; the known count is a plain add.
// Products are exact and accumulate in f32 like the vector version.  Only the choice of the rotation comes out of
// here; the weight itself is computed by the regular scoring pass at that rotation.
//
// UNITW: all class weights are equal — a common factor does not move the minimum, so the distances go in unweighted.
// SEVEN: 7 classes — slot 6 of the record is a seventh distance (no spare slot), slot 7 still `known` / the scan's sum.
template <bool USCALE, bool UNITW, bool SEVEN>
__device__ __forceinline__ void score_init_mfma_body(const InitArgs& a, int bx) {
  constexpr int RF = 8;
  extern __shared__ uint4 ring16[];   // [2*nb] packed scan records as 8 x f16 (row r and r+nb hold scan row r) + 1 zero row
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, q = lane >> 4;
  const InitLane l = init_lane(a, (int64_t)bx * 64 + wave * 16 + col);
  if (!__syncthreads_or(l.want)) return;   // nothing to initialise in this batch of 64 particles
  const float off0 = l.cy / a.resolution, off1 = l.cx / a.resolution;
  const char* __restrict__ recb = reinterpret_cast<const char*>(a.rec);
  const float2* __restrict__ tab2 = reinterpret_cast<const float2*>(USCALE ? a.utab : a.tab);
  const float4* __restrict__ scan4 = reinterpret_cast<const float4*>(a.scan_pk);
  const int nrot = *a.nrot;
  // byte offset of the lane's candidate row within the ring for every tile; candidates past nrot read the zero row
  const int zero_row = 2 * a.nb;
  int sh[INITM_TILES];
#pragma unroll
  for (int T = 0; T < INITM_TILES; T++) {
    const int m = 16 * T + col;
    sh[T] = m < nrot ? a.shift[m] : -1;
  }
  if (threadIdx.x == 0) ring16[zero_row] = make_uint4(0u, 0u, 0u, 0u);
  float wc[7];
#pragma unroll
  for (int c = 0; c < 7; c++) wc[c] = c < a.ncls ? (float)(0.01 * (double)a.fp.class_weights[c]) : 0.f;
  if constexpr (!UNITW) {
    const float w2 = init_weight_pow2(a.fp, a.ncls);
#pragma unroll
    for (int c = 0; c < 7; c++) wc[c] *= w2;
  }
  tdr_f4 accC[INITM_TILES], accN[INITM_TILES];
#pragma unroll
  for (int T = 0; T < INITM_TILES; T++) { accC[T] = (tdr_f4){0.f, 0.f, 0.f, 0.f}; accN[T] = (tdr_f4){0.f, 0.f, 0.f, 0.f}; }
  float known = 0.f;
  const int steps = (a.nb + 3) / 4;

  for (int j = 0; j < a.nr; j++) {
    const float2* trow = tab2 + (int64_t)j * a.nb;
    const float4* srow = scan4 + (int64_t)j * a.nb * 2;
    __syncthreads();
    bool big = false;
    for (int t = threadIdx.x; t < a.nb; t += 256) {
      const float4 v0 = srow[2 * t], v1 = srow[2 * t + 1];
      const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
      const uint4 pk = init_pack_scan8(f, big);
      ring16[t] = pk;
      ring16[t + a.nb] = pk;
    }
    if (big) atomicOr(init_inexact_word(a), 1);
    __syncthreads();
    // software pipeline: the record of step t+1 (and the table entry of step t+2) are requested before the matrix
    // work of step t, so every wave keeps two gathers in flight
    auto tab_at = [&](int t) -> float2 { return trow[min(4 * t + q, a.nb - 1)]; };
    auto rec_addr = [&](float2 tv) { return recb + init_cell_offset<USCALE, RF * 4>(a, l.scale, off0, off1, tv); };
    float2 tv_next = tab_at(1);
    float4 n0, n1;
    {
      const char* r0 = rec_addr(tab_at(0));
      n0 = *reinterpret_cast<const float4*>(r0);
      n1 = *reinterpret_cast<const float4*>(r0 + 16);
    }
    for (int t = 0; t < steps; t++) {
      const int i = 4 * t + q;
      const bool in = i < a.nb;
      const int ic = in ? i : a.nb - 1;
      float4 m0 = n0, m1 = n1;
      {
        const char* r1 = rec_addr(tv_next);        // step t+1 (clamped to the ring: an in-range address)
        tv_next = tab_at(t + 2);
        n0 = *reinterpret_cast<const float4*>(r1);
        n1 = *reinterpret_cast<const float4*>(r1 + 16);
      }
      if (!in) { m0 = make_float4(0.f, 0.f, 0.f, 0.f); m1 = m0; }
      known += m1.w;
      float v[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, SEVEN ? m1.z : 0.f, 0.f};
      if constexpr (!UNITW) {
#pragma unroll
        for (int c = 0; c < 7; c++) v[c] *= wc[c];
      }
      union { tdr_h2 h[4]; tdr_h8 v8; } bh, bl, bn;
#pragma unroll
      for (int c = 0; c < (SEVEN ? 4 : 3); c++) init_split_pair(v[2 * c], v[2 * c + 1], bh.h[c], bl.h[c]);   // v[7] == 0
      const tdr_h2 zero2 = __builtin_amdgcn_cvt_pkrtz(0.f, 0.f);
      if constexpr (!SEVEN) {
        bh.h[3] = zero2;
        bl.h[3] = zero2;
      }
      bn.h[0] = zero2; bn.h[1] = zero2; bn.h[2] = zero2;
      bn.h[3] = __builtin_amdgcn_cvt_pkrtz(0.f, m1.w);
      union { uint4 u; tdr_h8 v8; } av[INITM_TILES];
#pragma unroll
      for (int T = 0; T < INITM_TILES; T++) av[T].u = ring16[sh[T] < 0 ? zero_row : ic + sh[T]];
      // dependent MFMAs (same accumulator) are kept three instructions apart
#pragma unroll
      for (int T = 0; T < INITM_TILES; T++) accC[T] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[T].v8, bh.v8, accC[T], 0, 0, 0);
#pragma unroll
      for (int T = 0; T < INITM_TILES; T++) accN[T] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[T].v8, bn.v8, accN[T], 0, 0, 0);
#pragma unroll
      for (int T = 0; T < INITM_TILES; T++) accC[T] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[T].v8, bl.v8, accC[T], 0, 0, 0);
    }
  }
  init_pick_write(a, l, q, nrot, known, accC, [&](int T, int r) { return accN[T][r]; }, 13);
}
template <bool USCALE, bool UNITW, bool SEVEN>
__global__ __launch_bounds__(256) void score_init_mfma_kernel(InitArgs a) {
  score_init_mfma_body<USCALE, UNITW, SEVEN>(a, (int)blockIdx.x);
}
template <bool USCALE, bool UNITW, bool SEVEN>
__global__ __launch_bounds__(256) void score_init_mfma_batch_kernel(const InitArgs* __restrict__ args,
                                                                    const int32_t* __restrict__ blk, int k) {
  INIT_BATCH_FIND();
  score_init_mfma_body<USCALE, UNITW, SEVEN>(a, bx);
}

// The same for records of 12 and 16 floats (8-15 classes): a sample's record is two groups of 8 slots, each group its own
// pair of fragments — B from the gathered record, A from a second LDS image of the scan row — so a step of 4 samples is
// 2 x (hi + lo) products per tile instead of one, plus the normalisation product on the group that holds slot RF - 1.
// Class weights are always folded in (no unit-weight form); slots past the class count meet a zero weight.
template <int NV4, bool USCALE>
__device__ __forceinline__ void score_init_mfma_wide_body(const InitArgs& a, int bx) {
  constexpr int RF = 4 * NV4, NH = 2;
  static_assert(NV4 == 3 || NV4 == 4, "records of 12 or 16 floats");
  constexpr int HN = (RF - 1) / 8, KN = (RF - 1) % 8;   // group and slot of `known` / the scan's sum
  extern __shared__ uint4 ring16[];   // [2*nb + 1 rows][NH groups]: 8 x f16 each; rows r and r+nb hold scan row r, the last is zero
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, q = lane >> 4;
  const InitLane l = init_lane(a, (int64_t)bx * 64 + wave * 16 + col);
  if (!__syncthreads_or(l.want)) return;   // nothing to initialise in this batch of 64 particles
  const float off0 = l.cy / a.resolution, off1 = l.cx / a.resolution;
  const char* __restrict__ recb = reinterpret_cast<const char*>(a.rec);
  const float2* __restrict__ tab2 = reinterpret_cast<const float2*>(USCALE ? a.utab : a.tab);
  const float4* __restrict__ scan4 = reinterpret_cast<const float4*>(a.scan_pk);
  const int nrot = *a.nrot;
  const int zero_row = 2 * a.nb;
  int sh[INITM_TILES];
#pragma unroll
  for (int T = 0; T < INITM_TILES; T++) {
    const int m = 16 * T + col;
    sh[T] = m < nrot ? a.shift[m] : -1;
  }
  if (threadIdx.x < NH) ring16[zero_row * NH + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
  float wc[16];
#pragma unroll
  for (int c = 0; c < 16; c++) wc[c] = (c < a.ncls && c < TDR_MAX_CLASSES) ? (float)(0.01 * (double)a.fp.class_weights[c < TDR_MAX_CLASSES ? c : 0]) : 0.f;
  {
    const float w2 = init_weight_pow2(a.fp, a.ncls);
#pragma unroll
    for (int c = 0; c < 16; c++) wc[c] *= w2;
  }
  tdr_f4 accC[INITM_TILES], accN[INITM_TILES];
#pragma unroll
  for (int T = 0; T < INITM_TILES; T++) { accC[T] = (tdr_f4){0.f, 0.f, 0.f, 0.f}; accN[T] = (tdr_f4){0.f, 0.f, 0.f, 0.f}; }
  float known = 0.f;
  const int steps = (a.nb + 3) / 4;
  const tdr_h2 zero2 = __builtin_amdgcn_cvt_pkrtz(0.f, 0.f);

  for (int j = 0; j < a.nr; j++) {
    const float2* trow = tab2 + (int64_t)j * a.nb;
    const float4* srow = scan4 + (int64_t)j * a.nb * NV4;
    __syncthreads();
    bool big = false;
    for (int t = threadIdx.x; t < a.nb; t += 256) {
      float f[16];
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const float4 x = v < NV4 ? srow[NV4 * t + (v < NV4 ? v : 0)] : make_float4(0.f, 0.f, 0.f, 0.f);
        f[4 * v] = x.x; f[4 * v + 1] = x.y; f[4 * v + 2] = x.z; f[4 * v + 3] = x.w;
      }
#pragma unroll
      for (int h = 0; h < NH; h++) {
        const uint4 pk = init_pack_scan8(f + 8 * h, big);
        ring16[t * NH + h] = pk;
        ring16[(t + a.nb) * NH + h] = pk;
      }
    }
    if (big) atomicOr(init_inexact_word(a), 1);
    __syncthreads();
    auto tab_at = [&](int t) -> float2 { return trow[min(4 * t + q, a.nb - 1)]; };
    auto rec_addr = [&](float2 tv) { return recb + init_cell_offset<USCALE, RF * 4>(a, l.scale, off0, off1, tv); };
    float2 tv_next = tab_at(1);
    float4 nx[NV4];
    {
      const char* r0 = rec_addr(tab_at(0));
#pragma unroll
      for (int v = 0; v < NV4; v++) nx[v] = *reinterpret_cast<const float4*>(r0 + 16 * v);
    }
    for (int t = 0; t < steps; t++) {
      const int i = 4 * t + q;
      const bool in = i < a.nb;
      const int ic = in ? i : a.nb - 1;
      float v[16];
#pragma unroll
      for (int k = 0; k < 16; k++) v[k] = 0.f;
#pragma unroll
      for (int g = 0; g < NV4; g++) { v[4 * g] = nx[g].x; v[4 * g + 1] = nx[g].y; v[4 * g + 2] = nx[g].z; v[4 * g + 3] = nx[g].w; }
      {
        const char* r1 = rec_addr(tv_next);        // step t+1 (clamped to the ring: an in-range address)
        tv_next = tab_at(t + 2);
#pragma unroll
        for (int g = 0; g < NV4; g++) nx[g] = *reinterpret_cast<const float4*>(r1 + 16 * g);
      }
      if (!in) {
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = 0.f;
      }
      const float kn = v[RF - 1];
      known += kn;
#pragma unroll
      for (int k = 0; k < 16; k++) v[k] *= wc[k];   // (slots past the classes: weight 0)
      union { tdr_h2 h[4]; tdr_h8 v8; } bh[NH], bl[NH], bn;
#pragma unroll
      for (int h = 0; h < NH; h++)
#pragma unroll
        for (int c = 0; c < 4; c++) init_split_pair(v[8 * h + 2 * c], v[8 * h + 2 * c + 1], bh[h].h[c], bl[h].h[c]);
#pragma unroll
      for (int c = 0; c < 4; c++) bn.h[c] = zero2;
      bn.h[KN / 2] = (KN & 1) ? __builtin_amdgcn_cvt_pkrtz(0.f, kn) : __builtin_amdgcn_cvt_pkrtz(kn, 0.f);
      union { uint4 u; tdr_h8 v8; } av[INITM_TILES][NH];
#pragma unroll
      for (int T = 0; T < INITM_TILES; T++)
#pragma unroll
        for (int h = 0; h < NH; h++) av[T][h].u = ring16[(sh[T] < 0 ? zero_row : ic + sh[T]) * NH + h];
      // dependent MFMAs (same accumulator) are kept three instructions apart
#pragma unroll
      for (int h = 0; h < NH; h++) {
#pragma unroll
        for (int T = 0; T < INITM_TILES; T++) accC[T] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[T][h].v8, bh[h].v8, accC[T], 0, 0, 0);
        if (h == HN) {
#pragma unroll
          for (int T = 0; T < INITM_TILES; T++) accN[T] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[T][h].v8, bn.v8, accN[T], 0, 0, 0);
        }
#pragma unroll
        for (int T = 0; T < INITM_TILES; T++) accC[T] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[T][h].v8, bl[h].v8, accC[T], 0, 0, 0);
      }
    }
  }
  init_pick_write(a, l, q, nrot, known, accC, [&](int T, int r) { return accN[T][r]; }, 14);
}
template <int NV4, bool USCALE>
__global__ __launch_bounds__(256) void score_init_mfma_wide_kernel(InitArgs a) {
  score_init_mfma_wide_body<NV4, USCALE>(a, (int)blockIdx.x);
}
template <int NV4, bool USCALE>
__global__ __launch_bounds__(256) void score_init_mfma_wide_batch_kernel(const InitArgs* __restrict__ args,
                                                                         const int32_t* __restrict__ blk, int k) {
  INIT_BATCH_FIND();
  score_init_mfma_wide_body<NV4, USCALE>(a, bx);
}

// ---- the matrix-core search on pre-split half records ------------------------------------------------------------------
// score_init_mfma_kernel spends most of its vector instructions turning a gathered f32 record into the f16 hi / lo
// operands (weights, two conversions and a subtraction per pair, the zeroing of ragged lanes), per sample per particle.
// That work depends on the cell alone.  half_records_kernel does it ONCE per cell into a 32-byte record
//     H = {hi_0 .. hi_5, hi_6 | 0, 0}   L = {lo_0 .. lo_5, lo_6 | 0, unknown}      (f16; hi + lo = 2^k * w_c * 0.01 * d_c,
//                                                                                   2^k: init_weight_pow2; d_c with unitw)
// laid out like the dense records (guarded row-major grid, guard cells = distance 0, unknown; one all-zero record behind
// the grid for lanes without a sample), so that a lane's two 16-byte loads ARE the B fragments: H as it is, L with its
// last half cleared.  The scan side is ONE LDS image per ring, {c_0 .. c_5, c_6 | 0, sum c}: its slot 7 meets a zero in H
// and in the cleared L.  The normalisation  sum_samples (sum c) * known  is taken as  S - sum_samples (sum c) * unknown
// with S the sum of the whole scan (the same for every candidate): the third product, {0 .. 0, unknown}, is issued only
// in steps where some lane of the wave met an unknown cell — none, for a window inside the mapped area.
// Same f16 operands as score_init_mfma_kernel, summed in another order (four rings of one direction per instruction).
// The records carry the class weights, so they are rebuilt at every search (one pass over the map, ~0.35 ms for 4000^2
// cells) into scratch memory the map's owner provides (tdr_map_desc.rec16).
// RF: floats of the dense record read (4: up to 3 classes, 8: 4 to 7) — the half record is the same 32 bytes for both
template <int RF>
__global__ __launch_bounds__(256) void half_records_kernel(const float4* __restrict__ rec, int64_t ncells, int unitw,
                                                           tdr_filter_params fp, int ncls, uint4* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= ncells) return;
  float m[RF];
#pragma unroll
  for (int q = 0; q < RF / 4; q++) {
    const float4 t = rec[(RF / 4) * c + q];
    m[4 * q] = t.x; m[4 * q + 1] = t.y; m[4 * q + 2] = t.z; m[4 * q + 3] = t.w;
  }
  const float known = m[RF - 1];
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; k++) v[k] = (k < RF - 1 && k < 7 && k < ncls) ? m[k < RF ? k : 0] : 0.f;   // the distances
  if (!unitw) {
    const float w2 = init_weight_pow2(fp, ncls);
#pragma unroll
    for (int k = 0; k < 7; k++) v[k] *= k < ncls ? (float)(0.01 * (double)fp.class_weights[k]) * w2 : 0.f;
  }
  union { tdr_h2 h[4]; uint4 u; } H, L;
#pragma unroll
  for (int k = 0; k < 3; k++) init_split_pair(v[2 * k], v[2 * k + 1], H.h[k], L.h[k]);
  H.h[3] = __builtin_amdgcn_cvt_pkrtz(v[6], 0.f);   // slot 7: nothing in H, `unknown` in L
  L.h[3] = __builtin_amdgcn_cvt_pkrtz(v[6] - (float)H.h[3][0], 1.f - known);
  out[2 * c] = H.u;
  out[2 * c + 1] = L.u;
  if (c == 0) {   // the record behind the grid: nothing at all (what lanes without a sample read)
    out[2 * ncells] = make_uint4(0u, 0u, 0u, 0u);
    out[2 * ncells + 1] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// Work of one MFMA (k = 4 samples x 8 slots): the SAME direction i on 4 consecutive range rings — four neighbouring cells
// along a ray for each of the wave's 16 (neighbouring) particles, so that one gather instruction touches few cache
// lines (the L1 looks up one line per clock: with four samples a quarter ring apart the counters showed 42 line
// accesses per instruction and the L1, not the matrix or the vector units, setting the pace).  Rings are staged four at
// a time (one LDS image per ring).
// AHEAD: record loads in flight — those of step t + AHEAD are issued before the matrix work of step t.  The step loop is
// unrolled AHEAD + 1 times so that the buffers rotate by name (no register copies); the step count is padded to a multiple
// of that, the padding steps read the zero guard record.
template <bool USCALE, int AHEAD>
__device__ __forceinline__ void score_init_half_body(const InitArgs& a, int bx, const uint4* __restrict__ rec16, int img,
                                                     int rfs) {
  constexpr int R = AHEAD + 1;
  // LDS: [4 rings][img] scan records {c0..c5, c6|0, sum c} as 8 x f16, row r and r + nb of an image hold scan row r; the
  // img - 2 nb >= R rows behind them stay zero (padding steps; the exact count is chosen on the host so that the four
  // images sit on the banks with the fewest conflicts, init_half_image_rows) — followed by the rings' sample-table rows,
  // [4][nb + 2 R] float2
  extern __shared__ uint4 ringh[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, q = lane >> 4;
  // (an XCD-contiguous order of the workgroups and 1, 2 or 3 record loads in flight all run within 1 %: A/B on MI355X)
  const InitLane l = init_lane(a, (int64_t)bx * 64 + wave * 16 + col);
  if (!__syncthreads_or(l.want)) return;   // nothing to initialise in this batch of 64 particles
  typedef float tdr_v2f __attribute__((ext_vector_type(2)));
  const tdr_v2f offv = {l.cy / a.resolution, l.cx / a.resolution};
  const int rowstride = (a.cols + 2) * 32;
  const int kbase = (a.cols + 3) * 32;
  const float rmaxf = (float)a.rows, cmaxf = (float)a.cols;
  const char* __restrict__ recb = reinterpret_cast<const char*>(rec16);
  const float2* __restrict__ tab2 = reinterpret_cast<const float2*>(USCALE ? a.utab : a.tab);
  const int nrot = *a.nrot;
  const int nb = a.nb;
  const int ntab = nb + 2 * R;    // entries per table row in LDS
  float2* const ltab = reinterpret_cast<float2*>(ringh + 4 * img);
  // LDS byte address of this lane's candidate row at direction 0, per tile (the lane's ring image); candidates past nrot
  // read row 0 (their results are ignored)
  int arow[INITM_TILES];
#pragma unroll
  for (int T = 0; T < INITM_TILES; T++) {
    const int m = 16 * T + col;
    arow[T] = (q * img + (m < nrot ? a.shift[m] : 0)) * 16;
  }
  const int npad = img - 2 * nb;
  for (int t = threadIdx.x; t < 4 * npad; t += 256) ringh[(t / npad) * img + 2 * nb + t % npad] = make_uint4(0u, 0u, 0u, 0u);
  tdr_f4 accC[INITM_TILES], accN[INITM_TILES];   // accN: the normalisation's deficit, sum (sum c) * unknown
#pragma unroll
  for (int T = 0; T < INITM_TILES; T++) { accC[T] = (tdr_f4){0.f, 0.f, 0.f, 0.f}; accN[T] = (tdr_f4){0.f, 0.f, 0.f, 0.f}; }
  unsigned ucount = 0;   // 60 per unknown cell met
  float ssum = 0.f;      // this thread's share of S, the sum of the whole scan
  const int rounds = (nb + R - 1) / R;   // R directions each
  const char* const ringb = reinterpret_cast<const char*>(ringh);
  const float2* const ltq = ltab + q * ntab;
  const unsigned none_off = (unsigned)(a.rows + 2) * (unsigned)(a.cols + 2) * 32u;   // the all-zero record behind the grid

  // byte offset of the half record of table entry tv; a lane without a sample (ring >= nr, padding step) gets `none`
  // (not init_cell_offset: packed arithmetic, a floor conversion and no in-bounds select — tuned as it stands)
  auto rec_off = [&](float2 tv, bool in) -> unsigned {
    tdr_v2f pv = {tv.x, tv.y};
    if constexpr (!USCALE) pv = (pv * l.scale) * a.res;   // top_down_map_polar.cpp:28
    pv = pv + offv;                                      // :29-30
    tdr_v2f qv = {__builtin_amdgcn_fmed3f(pv.x, -1.f, rmaxf), __builtin_amdgcn_fmed3f(pv.y, -1.f, cmaxf)};
    qv = qv + 0.49999997f;                               // :31, see round_half_away_clamped
    int ri, ci;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ri) : "v"(qv.x));
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ci) : "v"(qv.y));
    const unsigned off = (unsigned)(__mul24(ri, rowstride) + (ci * 32 + kbase));   // guard cells: distance 0, unknown
    return in ? off : none_off;
  };

  for (int j0 = 0; j0 < a.nr; j0 += 4) {
    __syncthreads();
    bool big = false;
    for (int t = threadIdx.x; t < 4 * nb; t += 256) {
      const int kb = t / nb, r = t - kb * nb;
      uint4 pc = make_uint4(0u, 0u, 0u, 0u);
      if (j0 + kb < a.nr) {
        // packed scan record of rfs floats: the class counts first, the sum of the counts last
        const float* srow = a.scan_pk + ((int64_t)(j0 + kb) * nb + r) * rfs;
        float cnt[8];
#pragma unroll
        for (int k = 0; k < 7; k++) cnt[k] = k < a.ncls ? srow[k] : 0.f;
        cnt[7] = srow[rfs - 1];
        pc = init_pack_scan8(cnt, big);
        ssum += cnt[7];
      }
      ringh[kb * img + r] = pc;
      ringh[kb * img + r + nb] = pc;
    }
    for (int t = threadIdx.x; t < 4 * ntab; t += 256) {
      const int kb = t / ntab, r = t - kb * ntab;
      ltab[t] = tab2[(int64_t)min(j0 + kb, a.nr - 1) * nb + min(r, nb - 1)];
    }
    if (big) atomicOr(init_inexact_word(a), 1);
    __syncthreads();
    const bool ring_ok = j0 + q < a.nr;
    // Software pipeline: the two record loads of step t + AHEAD are issued before the matrix work of step t (the table
    // entry comes from LDS, so the address costs no trip to memory).  The scheduling barriers keep the compiler from
    // sinking the loads next to their use, which would expose a full memory latency in every step.
    uint4 h[R], l[R];
#pragma unroll
    for (int k = 0; k < AHEAD; k++) {
      const char* r = recb + rec_off(ltq[k], ring_ok && k < nb);
      h[k] = *reinterpret_cast<const uint4*>(r);
      l[k] = *reinterpret_cast<const uint4*>(r + 16);
    }
    int ar[INITM_TILES];
#pragma unroll
    for (int T = 0; T < INITM_TILES; T++) ar[T] = arow[T];
    int inext = AHEAD;   // direction of the loads issued next
    for (int rd = 0; rd < rounds; rd++) {
#pragma unroll
      for (int u = 0; u < R; u++) {
        {
          const char* r = recb + rec_off(ltq[inext], ring_ok && inext < nb);
          h[(u + AHEAD) % R] = *reinterpret_cast<const uint4*>(r);
          l[(u + AHEAD) % R] = *reinterpret_cast<const uint4*>(r + 16);
          inext++;
        }
        __builtin_amdgcn_sched_barrier(0);
        if (rd * R + u < nb) {   // (uniform) not a padding step
          union { uint4 u4; tdr_h8 v8; } bh, bl, bn;
          bh.u4 = h[u];
          bl.u4 = l[u];
          bn.u4 = make_uint4(0u, 0u, 0u, bl.u4.w & 0xFFFF0000u);   // {0 .. 0, unknown}
          bl.u4.w &= 0x0000FFFFu;
          ucount += bn.u4.w >> 24;   // f16 1.0 = 0x3C00: its high byte, 60 per unknown cell
          union { uint4 u4; tdr_h8 v8; } ac[INITM_TILES];
#pragma unroll
          for (int T = 0; T < INITM_TILES; T++) ac[T].u4 = *reinterpret_cast<const uint4*>(ringb + ar[T]);
#pragma unroll
          for (int T = 0; T < INITM_TILES; T++) accC[T] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ac[T].v8, bh.v8, accC[T], 0, 0, 0);
          if (__builtin_amdgcn_ballot_w64(bn.u4.w != 0u) != 0) {   // (uniform) some lane met an unknown cell
#pragma unroll
            for (int T = 0; T < INITM_TILES; T++) accN[T] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ac[T].v8, bn.v8, accN[T], 0, 0, 0);
          }
#pragma unroll
          for (int T = 0; T < INITM_TILES; T++) accC[T] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ac[T].v8, bl.v8, accC[T], 0, 0, 0);
        }
#pragma unroll
        for (int T = 0; T < INITM_TILES; T++) ar[T] += 16;
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  // S: every thread staged its share of every ring
  __syncthreads();
  float* const red = reinterpret_cast<float*>(ringh);
  red[threadIdx.x] = ssum;
  __syncthreads();
  float stotal = 0.f;
  for (int t = 0; t < 256; t++) stotal += red[t];   // same order in every lane
  // samples this lane went through: nb directions on each of its rings j = q, q + 4, ...
  const int my_rings = (a.nr - q + 3) / 4;
  const float known = (float)(my_rings * nb - (int)(ucount / 60u));
  init_pick_write(a, l, q, nrot, known, accC, [&](int T, int r) { return stotal - accN[T][r]; }, 12);
}
template <bool USCALE, int AHEAD>
__global__ __launch_bounds__(256) void score_init_half_kernel(InitArgs a, const uint4* __restrict__ rec16, int img,
                                                              int rfs) {
  score_init_half_body<USCALE, AHEAD>(a, (int)blockIdx.x, rec16, img, rfs);
}
// batched: the half records, the image stride and the scan record size belong to the map and the scan shape — the same
// for every filter of the batch — and stay kernel arguments
template <bool USCALE, int AHEAD>
__global__ __launch_bounds__(256) void score_init_half_batch_kernel(const InitArgs* __restrict__ args,
                                                                    const int32_t* __restrict__ blk, int k,
                                                                    const uint4* __restrict__ rec16, int img, int rfs) {
  INIT_BATCH_FIND();
  score_init_half_body<USCALE, AHEAD>(a, bx, rec16, img, rfs);
}

// candidate rotations of the search, generated exactly like the reference's loop (state_particle.cpp:197: float t,
// double increment) together with their bin shifts (:124-128)
__device__ __forceinline__ void init_rot_body(int nb, int* __restrict__ shift, float* __restrict__ theta,
                                              int* __restrict__ nrot) {
  nrot[1] = 0;   // the "scan counts too large for f16" flag of score_init_mfma_kernel
  int k = 0;
  for (float t = 0; t < 2 * M_PI; t += 2 * M_PI / 40) {
    if (k >= INIT_MAXROT) break;
    theta[k] = t;
    shift[k] = rot_shift_dev(t, nb);
    k++;
  }
  *nrot = k;
}
__global__ void init_rot_kernel(int nb, int* __restrict__ shift, float* __restrict__ theta, int* __restrict__ nrot) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  init_rot_body(nb, shift, theta, nrot);
}

// state_.theta = best_theta; state_.have_init = true (state_particle.cpp:205-206)
__device__ __forceinline__ void init_apply_body(const float* __restrict__ res_theta, const float* __restrict__ res_flag,
                                                int64_t n, float* __restrict__ st, int64_t cap, int64_t p) {
  if (p < n && res_flag[p] != 0.f) {
    st[TDR_ST_THETA * cap + p] = res_theta[p];
    st[TDR_ST_HAVE_INIT * cap + p] = 1.f;
  }
}
__global__ void init_apply_kernel(const float* __restrict__ res_theta, const float* __restrict__ res_flag, int64_t n,
                                  float* __restrict__ st, int64_t cap) {
  init_apply_body(res_theta, res_flag, n, st, cap, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}
// particles whose init search found no valid rotation keep best_cost = FLT_MAX (:193) -> weight 1/(FLT_MAX + reg)
__device__ __forceinline__ void init_fixup_body(const float* __restrict__ res_flag, int64_t n, float regularization,
                                                float* __restrict__ raw_w, int64_t p) {
  if (p < n && res_flag[p] == 2.f) raw_w[p] = (float)(1. / (double)(3.402823466e+38f + regularization));
}
__global__ void init_fixup_kernel(const float* __restrict__ res_flag, int64_t n, float regularization,
                                  float* __restrict__ raw_w) {
  init_fixup_body(res_flag, n, regularization, raw_w, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}
// The small kernels of a batched search, over the same block table as the search kernels (64 particles per block).
// prep: the rotation table of every filter, its f16 flag and its res_flag zeroed (standalone: init_rot_kernel + a memset
// per filter); apply and fixup as above.  `fix` holds what InitArgs does not: the filters' raw weights.
struct InitFixEntry { float* raw_w; float* st; };
__global__ __launch_bounds__(64) void init_prep_batch_kernel(const InitArgs* __restrict__ args,
                                                             const int32_t* __restrict__ blk, int k) {
  const int b = (int)blockIdx.x + blk[0];
  const int e = batch_find(k, b, [&](int i) { return blk[i]; });
  const InitArgs a = args[e];
  const int bx = b - blk[e];
  const int64_t p = (int64_t)bx * 64 + threadIdx.x;
  if (p < a.n) a.res_flag[p] = 0.f;
  if (bx == 0 && threadIdx.x == 0)
    init_rot_body(a.nb, const_cast<int*>(a.shift), const_cast<float*>(a.theta), const_cast<int*>(a.nrot));
}
__global__ __launch_bounds__(64) void init_apply_batch_kernel(const InitArgs* __restrict__ args,
                                                              const InitFixEntry* __restrict__ fix,
                                                              const int32_t* __restrict__ blk, int k) {
  const int b = (int)blockIdx.x + blk[0];
  const int e = batch_find(k, b, [&](int i) { return blk[i]; });
  const InitArgs a = args[e];
  init_apply_body(a.res_theta, a.res_flag, a.n, fix[e].st, a.cap, (int64_t)(b - blk[e]) * 64 + threadIdx.x);
}
__global__ __launch_bounds__(64) void init_fixup_batch_kernel(const InitArgs* __restrict__ args,
                                                              const InitFixEntry* __restrict__ fix,
                                                              const int32_t* __restrict__ blk, int k) {
  const int b = (int)blockIdx.x + blk[0];
  const int e = batch_find(k, b, [&](int i) { return blk[i]; });
  const InitArgs a = args[e];
  init_fixup_body(a.res_flag, a.n, a.fp.regularization, fix[e].raw_w, (int64_t)(b - blk[e]) * 64 + threadIdx.x);
}

// bytes of the scratch behind tdr_map_desc.rec16 (0: this record size has no matrix-core search)
extern "C" size_t tdr_map_rec16_bytes(int ncls, int rows, int cols) {
  if (ncls < 1 || ncls > 7 || rows < 1 || cols < 1) return 0;
  // the search addresses this grid with 32-bit byte offsets and a 24-bit row multiply: a map beyond that has no half
  // records (0: the caller passes none and the search splits the dense records on the fly)
  const uint64_t bytes = (uint64_t)(rows + 2) * (uint64_t)(cols + 2) * 32 + 32;   // + the all-zero record behind the grid
  if (bytes > 0xFFFFFFFFull || (uint64_t)(cols + 2) * 32 >= (1u << 24)) return 0;
  return (size_t)bytes;
}
// Rows per LDS scan image of score_init_half_kernel: 2 nb + R + c with the c in [0, 16) that gives the ds_read_b128 of
// the candidates' rows the fewest bank conflicts.  A lane (candidate m, ring q) reads row q * img + i + shift_m; the LDS
// serves the instruction in four groups of 16 lanes (MI355X_MICROARCH.md, LDS) and two lanes of a group collide when
// their rows differ by a multiple of 16.  The shifts are multiples of nb / 40, so only a few residues occur and the
// image stride decides how the rings' residues interleave (nb = 256: 3.7 LDS cycles per read at the worst stride, 2.0 at
// the best).
static int init_half_image_rows(int nb, int R) {
  int sh[48] = {0};
  int k = 0;
  for (float t = 0; t < 2 * M_PI && k < 48; t += 2 * M_PI / 40) {   // as init_rot_kernel / rot_shift_dev
    int s = (int)round((double)(t * (float)nb / 2) / M_PI);
    s %= nb;
    if (s < 0) s += nb;
    sh[k++] = s;
  }
  static const int grp[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                 {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                 {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                 {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
  int best_c = 0;
  long best = -1;
  for (int c = 0; c < 16; c++) {
    const int img = 2 * nb + R + c;
    long tot = 0;
    for (int T = 0; T < 3; T++)
      for (int i = 0; i < 16; i++)   // the pattern repeats with i mod 16
        for (int g = 0; g < 4; g++) {
          int rows[16], worst = 1;
          for (int l = 0; l < 16; l++) rows[l] = (grp[g][l] >> 4) * img + i + sh[16 * T + (grp[g][l] & 15)];
          for (int x = 0; x < 16; x++) {
            int distinct = 1;   // distinct rows on the bank quad of rows[x]
            for (int y = 0; y < x; y++)
              if ((rows[y] - rows[x]) % 16 == 0 && rows[y] != rows[x]) {
                bool seen = false;
                for (int z = 0; z < y; z++) seen |= rows[z] == rows[y];
                if (!seen) distinct++;
              }
            if (distinct > worst) worst = distinct;
          }
          tot += worst;
        }
    if (best < 0 || tot < best) { best = tot; best_c = c; }
  }
  return 2 * nb + R + best_c;
}

// ---- what the standalone and the batched search share on the host ------------------------------------------------------
// dynamic LDS of each pass, in bytes (the layouts: at the bodies' `extern __shared__` arrays)
static size_t init_lds_vector(int nb, int rf) { return (size_t)2 * nb * rf * 4; }
static size_t init_lds_split(int nb) { return ((size_t)2 * nb + 1) * 16; }
static size_t init_lds_wide(int nb) { return ((size_t)2 * nb + 1) * 2 * 16; }
static size_t init_lds_half(int img, int nb, int R) { return (size_t)4 * img * 16 + (size_t)4 * (nb + 2 * R) * 8; }
// The matrix-core pass of a search — ONE choice for both paths: the passes pick differently where candidates tie to
// rounding (tdr.h, tdr_config_init_mfma), so a batched filter must take the pass its standalone call takes.
int tdr_score_init_pass(const tdr_map_desc* map, int nb, int64_t n_total) {
  const int rf = map->rec_floats;
  const bool ks = tdr_has_kslot(map->ncls, rf);
  if (!tdr_cfg().init_mfma) return TDR_INIT_PASS_VECTOR;
  // (with the most loads in flight, AHEAD = 3, and c = 15 init_half_image_rows gives at most 2 nb + 19 rows; the check keeps
  // the 2 nb + 20 it has always asked for)
  if ((rf == 4 || rf == 8) && map->ncls <= 7 && map->rec16 && tdr_map_rec16_bytes(map->ncls, map->rows, map->cols) != 0 &&
      n_total >= tdr_cfg().rec16_min && init_lds_half(2 * nb + 20, nb, 4) <= 64 * 1024)
    return TDR_INIT_PASS_HALF;
  if (rf == 8 && (ks || map->ncls == 7)) return TDR_INIT_PASS_SPLIT;
  if (rf == 12 || rf == 16) return TDR_INIT_PASS_WIDE;
  return TDR_INIT_PASS_VECTOR;
}
// all class weights equal and positive: a common factor does not move the minimum (UNITW; the half records' `unitw`)
static bool init_unit_weights(const tdr_filter_params* fp, int ncls) {
  bool unitw = true;
  for (int c = 1; c < ncls; c++) unitw &= fp->class_weights[c] == fp->class_weights[0];
  return unitw && fp->class_weights[0] > 0.f;
}
// the arguments of one filter's search; its rotation table lives behind the result arrays:
// [shift INIT_MAXROT][theta INIT_MAXROT][nrot][the "scan count does not fit f16" word]
static InitArgs make_init_args(const tdr_map_desc* map, const float* tab, const float* utab, const float* scan_pk, int nb,
                               int nr, float res, const tdr_filter_params* fp, const float* st, int64_t cap, int64_t n,
                               const int32_t* order, float* res_flag, int64_t npad) {
  InitArgs ia;
  float* res_theta = res_flag + npad;
  ia.rec = map->rec; ia.rows = map->rows; ia.cols = map->cols; ia.resolution = map->resolution;
  ia.tab = tab; ia.utab = utab; ia.scan_pk = scan_pk; ia.nb = nb; ia.nr = nr; ia.res = res;
  ia.st = st; ia.cap = cap; ia.n = n; ia.order = order; ia.fp = *fp; ia.gate = make_gate(fp, map);
  ia.P = (int64_t)nb * nr; ia.ncls = map->ncls; ia.res_flag = res_flag; ia.res_theta = res_theta;
  int* d_shift = reinterpret_cast<int*>(res_theta + npad);
  float* d_theta = reinterpret_cast<float*>(d_shift + INIT_MAXROT);
  ia.shift = d_shift; ia.theta = d_theta; ia.nrot = reinterpret_cast<int*>(d_theta + INIT_MAXROT);
  ia.only_if = nullptr;
  ia.stats = tdr_profile_stats_ptr();
  return ia;
}
// the pre-split half records of `map` for these class weights, into the map owner's scratch
static int launch_half_records(const tdr_map_desc* map, const tdr_filter_params* fp, bool unitw, hipStream_t s) {
  const int64_t ncells = (int64_t)(map->rows + 2) * (map->cols + 2);
  const dim3 hgrid((unsigned)cdiv(ncells, 256)), hblock(256);
  const float4* rec4 = reinterpret_cast<const float4*>(map->rec);
  uint4* r16 = reinterpret_cast<uint4*>(map->rec16);
  if (map->rec_floats == 4) hipLaunchKernelGGL((half_records_kernel<4>), hgrid, hblock, 0, s, rec4, ncells, unitw ? 1 : 0, *fp, map->ncls, r16);
  else hipLaunchKernelGGL((half_records_kernel<8>), hgrid, hblock, 0, s, rec4, ncells, unitw ? 1 : 0, *fp, map->ncls, r16);
  LAUNCH_CHECK("half_records");
  return TDR_OK;
}
// Where a search kernel runs: on one filter — the standalone kernels, `one` going by value — or on a run of a batch's table,
// entries args[0, count) with the cumulative block counts blk (the batched kernels, see INIT_BATCH_FIND).  The two kernels
// of an instantiation take the same arguments behind these.
struct InitTarget {
  const InitArgs* one;
  const InitArgs* args;
  const int32_t* blk;
  int count;
  dim3 grid;
};
template <class KOne, class KBatch, class... Tail>
static void init_launch(const InitTarget& t, KOne one, KBatch batched, unsigned threads, size_t lds, hipStream_t s,
                        Tail... tail) {
  if (t.one) hipLaunchKernelGGL(one, t.grid, dim3(threads), lds, s, *t.one, tail...);
  else hipLaunchKernelGGL(batched, t.grid, dim3(threads), lds, s, t.args, t.blk, t.count, tail...);
}
// The matrix-core pass `pass` (tdr_score_init_pass) on the filters of `t` whose scale mode is `us`; unitw: all their class
// weights are equal (init_unit_weights; the wide pass has no such form).  The vector kernel behind it then runs only for
// a filter whose scan held a count that did not fit f16.
static int launch_init_mfma(int pass, const tdr_map_desc* map, int nb, bool us, bool unitw, const InitTarget& t,
                            hipStream_t s) {
  const int rf = map->rec_floats;
  if (pass == TDR_INIT_PASS_HALF) {
    // pre-split half records (weights folded in), which launch_half_records built into the map owner's scratch
    const int ahead = tdr_cfg().init_ahead, img = init_half_image_rows(nb, ahead + 1);
    const size_t lds = init_lds_half(img, nb, ahead + 1);
    const uint4* r16 = reinterpret_cast<const uint4*>(map->rec16);
    with_flags([&](auto US) {
      constexpr bool U = decltype(US)::value;
      if (ahead == 1) init_launch(t, score_init_half_kernel<U, 1>, score_init_half_batch_kernel<U, 1>, 256, lds, s, r16, img, rf);
      else if (ahead == 2) init_launch(t, score_init_half_kernel<U, 2>, score_init_half_batch_kernel<U, 2>, 256, lds, s, r16, img, rf);
      else init_launch(t, score_init_half_kernel<U, 3>, score_init_half_batch_kernel<U, 3>, 256, lds, s, r16, img, rf);
      return TDR_OK;
    }, us);
    LAUNCH_CHECK(t.one ? "score_init_half" : "batch_score_init_half");
  } else if (pass == TDR_INIT_PASS_SPLIT) {
    // the f32 records split per sample (small filters, maps without the scratch)
    with_flags([&](auto US, auto UW, auto SV) {
      constexpr bool U = decltype(US)::value, W = decltype(UW)::value, V = decltype(SV)::value;
      init_launch(t, score_init_mfma_kernel<U, W, V>, score_init_mfma_batch_kernel<U, W, V>, 256, init_lds_split(nb), s);
      return TDR_OK;
    }, us, unitw, !tdr_has_kslot(map->ncls, rf));
    LAUNCH_CHECK(t.one ? "score_init_mfma" : "batch_score_init_mfma");
  } else {
    // 8-15 classes: two groups of 8 slots per sample
    with_flags([&](auto US, auto R16) {
      constexpr bool U = decltype(US)::value;
      constexpr int NV4 = decltype(R16)::value ? 4 : 3;
      init_launch(t, score_init_mfma_wide_kernel<NV4, U>, score_init_mfma_wide_batch_kernel<NV4, U>, 256, init_lds_wide(nb), s);
      return TDR_OK;
    }, us, rf == 16);
    LAUNCH_CHECK(t.one ? "score_init_mfma_wide" : "batch_score_init_mfma_wide");
  }
  return TDR_OK;
}
// the vector kernel, likewise
static int launch_init_vector(const tdr_map_desc* map, int nb, bool us, const InitTarget& t, hipStream_t s) {
  const int rf = map->rec_floats;
  if (int rc = with_nv4(rf, t.one ? "score" : "batch_init", [&](auto N) {
        return with_flags([&](auto KS, auto US) {
          constexpr int NV4 = decltype(N)::value;
          constexpr bool K = decltype(KS)::value, U = decltype(US)::value;
          init_launch(t, score_init_kernel<NV4, K, U>, score_init_batch_kernel<NV4, K, U>, 64 * INIT_WAVES,
                      init_lds_vector(nb, rf), s);
          return TDR_OK;
        }, tdr_has_kslot(map->ncls, rf), us);
      }))
    return rc;
  LAUNCH_CHECK(t.one ? "score_init" : "batch_score_init");
  return TDR_OK;
}

int tdr_score_init_search(const tdr_map_desc* map, const float* tab, const float* utab, const float* scan_pk, int nb,
                          int nr, float res, const tdr_filter_params* fp, float* st, int64_t cap, int64_t n,
                          int64_t n_total, const int32_t* order, float* res_flag, int64_t npad, hipStream_t s) {
  InitArgs ia = make_init_args(map, tab, utab, scan_pk, nb, nr, res, fp, st, cap, n, order, res_flag, npad);
  hipLaunchKernelGGL(init_rot_kernel, dim3(1), dim3(64), 0, s, nb, const_cast<int*>(ia.shift), const_cast<float*>(ia.theta),
                     const_cast<int*>(ia.nrot));
  LAUNCH_CHECK("init_rot");
  HIP_TRY(hipMemsetAsync(res_flag, 0, sizeof(float) * (size_t)n, s));
  const InitTarget t{&ia, nullptr, nullptr, 0, dim3((unsigned)cdiv(n, 64))};
  const bool us = utab != nullptr, unitw = init_unit_weights(fp, map->ncls);
  const int pass = tdr_score_init_pass(map, nb, n_total);
  if (pass == TDR_INIT_PASS_HALF)
    if (int rc = launch_half_records(map, fp, unitw, s)) return rc;
  if (pass != TDR_INIT_PASS_VECTOR) {
    if (int rc = launch_init_mfma(pass, map, nb, us, unitw, t, s)) return rc;
    // the vector kernel: only what the matrix-core pass could not take.  (t.one points at ia and is read at the launch, so
    // the launch below sees this; a target that held the arguments by value would have to be rebuilt here.)
    ia.only_if = ia.nrot + 1;
  }
  if (int rc = launch_init_vector(map, nb, us, t, s)) return rc;
  hipLaunchKernelGGL(init_apply_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, (const float*)ia.res_theta,
                     (const float*)res_flag, n, st, cap);
  LAUNCH_CHECK("init_apply");
  return TDR_OK;
}
// ---- the searches of a batch (tdr_batch_step with "batch_init_search") -------------------------------------------------
// The filters are sorted into RUNS of one matrix-core pass each — and, for the half-record pass, one set of half records:
// the records fold the class weights in unless all are equal and positive, so half-path filters are grouped by that flag
// and, where it is not set, by the weight vector.  Per run: (the group's half_records_kernel,) one launch per scale mode
// present.  Then one vector-kernel launch per scale mode over the whole table — every filter reads its OWN f16 flag, so a
// filter whose scan holds a count above 2048 sends only itself through the vector kernel — and one apply.
namespace {
struct InitRun { int32_t first, count, pass, unitw, us_mask; };
struct BatchInitHdr { int32_t k, blocks, nruns, us_mask; };
struct BatchInitLayout { size_t runs, args, fix, blk, total; };
BatchInitLayout batch_init_layout(int k) {
  auto up = [](size_t x) { return (x + 63) / 64 * 64; };
  BatchInitLayout L;
  L.runs = up(sizeof(BatchInitHdr));
  L.args = L.runs + up(sizeof(InitRun) * k);
  L.fix = L.args + up(sizeof(InitArgs) * k);
  L.blk = L.fix + up(sizeof(InitFixEntry) * k);
  L.total = L.blk + up(sizeof(int32_t) * (k + 1));
  return L;
}
}  // namespace
size_t tdr_batch_init_stage_bytes(int k) { return k < 1 ? 0 : batch_init_layout(k).total; }
int tdr_batch_init_build(const tdr_map_desc* map, const float* tab, int nb, int nr, int k, const TdrBatchInitIn* in,
                         void* host_stage) {
  if (!map || !tab || !in || !host_stage || k < 1) return fail(TDR_ERR_ARG, "batch_init: bad arguments");
  const BatchInitLayout Lo = batch_init_layout(k);
  char* base = static_cast<char*>(host_stage);
  BatchInitHdr& h = *reinterpret_cast<BatchInitHdr*>(base);
  InitRun* runs = reinterpret_cast<InitRun*>(base + Lo.runs);
  InitArgs* args = reinterpret_cast<InitArgs*>(base + Lo.args);
  InitFixEntry* fix = reinterpret_cast<InitFixEntry*>(base + Lo.fix);
  int32_t* blk = reinterpret_cast<int32_t*>(base + Lo.blk);
  // sort key of a filter: pass, unit-weight flag (the wide pass has no such form), half-record group
  struct Key { int pass, unitw, group, idx; };
  std::vector<Key> keys((size_t)k);
  std::vector<int> group_owner;   // a filter of every half-record group with weights folded in
  for (int i = 0; i < k; i++) {
    const TdrBatchInitIn& x = in[i];
    if (!x.fp || !x.st || !x.res_flag || !x.raw_w || x.n < 1 || x.cap < x.n) return fail(TDR_ERR_ARG, "batch_init: filter %d", i);
    Key q{tdr_score_init_pass(map, nb, x.n), 0, 0, i};
    if (q.pass == TDR_INIT_PASS_HALF || q.pass == TDR_INIT_PASS_SPLIT) q.unitw = init_unit_weights(x.fp, map->ncls) ? 1 : 0;
    if (q.pass == TDR_INIT_PASS_HALF && !q.unitw) {
      size_t g = 0;
      for (; g < group_owner.size(); g++)
        if (std::memcmp(in[group_owner[g]].fp->class_weights, x.fp->class_weights, sizeof(float) * (size_t)std::min(map->ncls, 7)) == 0) break;
      if (g == group_owner.size()) group_owner.push_back(i);
      q.group = (int)g;
    }
    keys[i] = q;
  }
  std::stable_sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) {
    return a.pass != b.pass ? a.pass < b.pass : a.unitw != b.unitw ? a.unitw < b.unitw : a.group < b.group;
  });
  h = BatchInitHdr{k, 0, 0, 0};
  for (int j = 0; j < k; j++) {
    const Key& q = keys[j];
    const TdrBatchInitIn& x = in[q.idx];
    InitArgs a = make_init_args(map, tab, x.utab, x.scan_pk, nb, nr, x.res, x.fp, x.st, x.cap, x.n, nullptr, x.res_flag, x.npad);
    if (q.pass != TDR_INIT_PASS_VECTOR) a.only_if = a.nrot + 1;   // the vector kernel: only what the matrix-core pass could not take
    args[j] = a;
    fix[j] = InitFixEntry{x.raw_w, x.st};
    blk[j] = h.blocks;
    h.blocks += (int32_t)cdiv(x.n, 64);
    const int us_bit = x.utab ? 2 : 1;
    h.us_mask |= us_bit;
    const bool same = j > 0 && keys[j - 1].pass == q.pass && keys[j - 1].unitw == q.unitw && keys[j - 1].group == q.group;
    if (!same) runs[h.nruns++] = InitRun{j, 0, q.pass, q.unitw, 0};
    runs[h.nruns - 1].count++;
    runs[h.nruns - 1].us_mask |= us_bit;
  }
  blk[k] = h.blocks;
  return TDR_OK;
}
int tdr_batch_init_launch(const tdr_map_desc* map, int nb, int nr, const void* host_stage, const void* dev_stage,
                          hipStream_t s) {
  if (!map || !host_stage || !dev_stage) return fail(TDR_ERR_ARG, "batch_init: bad arguments");
  const BatchInitHdr& h = *static_cast<const BatchInitHdr*>(host_stage);
  const int k = h.k;
  const BatchInitLayout Lo = batch_init_layout(k);
  const char* hb = static_cast<const char*>(host_stage);
  const char* d = static_cast<const char*>(dev_stage);
  const InitRun* runs = reinterpret_cast<const InitRun*>(hb + Lo.runs);
  const InitArgs* hargs = reinterpret_cast<const InitArgs*>(hb + Lo.args);
  const int32_t* hblk = reinterpret_cast<const int32_t*>(hb + Lo.blk);
  const InitArgs* args = reinterpret_cast<const InitArgs*>(d + Lo.args);
  const InitFixEntry* fix = reinterpret_cast<const InitFixEntry*>(d + Lo.fix);
  const int32_t* blk = reinterpret_cast<const int32_t*>(d + Lo.blk);
  const dim3 all((unsigned)h.blocks);
  hipLaunchKernelGGL(init_prep_batch_kernel, all, dim3(64), 0, s, args, blk, k);
  LAUNCH_CHECK("batch_init_prep");
  for (int r = 0; r < h.nruns; r++) {
    const InitRun& R = runs[r];
    if (R.pass == TDR_INIT_PASS_VECTOR) continue;
    const InitTarget t{nullptr, args + R.first, blk + R.first, R.count,
                       dim3((unsigned)(hblk[R.first + R.count] - hblk[R.first]))};
    if (R.pass == TDR_INIT_PASS_HALF)
      if (int rc = launch_half_records(map, &hargs[R.first].fp, R.unitw != 0, s)) return rc;
    for (int us = 1; us >= 0; us--)   // the filters with a uniform-scale table, then the others: one instantiation each
      if (R.us_mask & (us ? 2 : 1))
        if (int rc = launch_init_mfma(R.pass, map, nb, us != 0, R.unitw != 0, t, s)) return rc;
  }
  const InitTarget t{nullptr, args, blk, k, all};
  for (int us = 1; us >= 0; us--)
    if (h.us_mask & (us ? 2 : 1))
      if (int rc = launch_init_vector(map, nb, us != 0, t, s)) return rc;
  hipLaunchKernelGGL(init_apply_batch_kernel, all, dim3(64), 0, s, args, fix, blk, k);
  LAUNCH_CHECK("batch_init_apply");
  (void)nr;
  return TDR_OK;
}
int tdr_batch_init_fixup(const void* host_stage, const void* dev_stage, hipStream_t s) {
  if (!host_stage || !dev_stage) return fail(TDR_ERR_ARG, "batch_init: bad arguments");
  const BatchInitHdr& h = *static_cast<const BatchInitHdr*>(host_stage);
  const BatchInitLayout Lo = batch_init_layout(h.k);
  const char* d = static_cast<const char*>(dev_stage);
  hipLaunchKernelGGL(init_fixup_batch_kernel, dim3((unsigned)h.blocks), dim3(64), 0, s,
                     reinterpret_cast<const InitArgs*>(d + Lo.args), reinterpret_cast<const InitFixEntry*>(d + Lo.fix),
                     reinterpret_cast<const int32_t*>(d + Lo.blk), h.k);
  LAUNCH_CHECK("batch_init_fixup");
  return TDR_OK;
}
int tdr_score_init_fixup(const float* res_flag, int64_t n, float regularization, float* raw_w, hipStream_t s) {
  hipLaunchKernelGGL(init_fixup_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, res_flag, n, regularization, raw_w);
  LAUNCH_CHECK("init_fixup");
  return TDR_OK;
}
