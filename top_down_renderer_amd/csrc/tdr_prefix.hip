// tdr_prefix.hip — the serial float32 chains of the filter step, reproduced bit-exactly in parallel: the running sum of
// the resample (particle_filter.cpp:179, every prefix is written) and the two statistics chains of the update (`sum`,
// `bottom_stddev`, :108-126, only the totals are used).
#include "tdr_common.h"
#include "tdr_batch.h"

// Map of the file: entry point -> kernels, by n, and the switch that reaches each path.
//
//  tdr_k_prefix (running sum + running maximum; tdr_k_prefix_mode forces a path)
//    256 <= n <= 32 768                   pfx_small_kernel: one launch, one workgroup, weights in LDS          mode 3
//    n >= 6144 with a workspace           prefix_multi                                                         mode 2
//      n > 32 768                         pfx_chunk_sum_kernel -> pfx_grid_summary_kernel (one wave per wave-chunk of
//                                         512, over the chip) -> pfx_grid_walk_kernel (ONE wave walks the summaries) ->
//                                         pfx_grid_fill_kernel (one wave per wave-chunk).  An input with a negative or NaN
//                                         weight takes the 4096-chunk bodies of the line below inside these launches
//      n <= 32 768, or tdr_config_prefix_small(0)
//                                         pfx_chunk_sum_kernel -> pfx_chunk_summary_kernel -> pfx_walk_kernel (one
//                                         workgroup walks 4096-chunks from the first addend on) -> pfx_chunk_fill_kernel
//    n < 24 576 otherwise                 prefix_serial_kernel: one wave, lane 0 adds in index order           mode 0
//    else                                 prefix_exact_kernel: one workgroup, the older tie-list algorithm     mode 1
//    tdr_config_tuning("prefix_head", n): addends pfx_walk_kernel hands to the serial head of pfx_exact_range at the very start
//  tdr_uw_small (the update's statistics, n <= 32 768)
//    uw_small_kernel<true>: the chains wave by wave (default); <false>: chunk by chunk on the whole workgroup
//    (tdr_config_uw_waves(0))
//  tdr_chain_total (one statistics chain, n > 32 768; called from tdr_filter.hip)
//    [chain_sum_kernel unless the caller's pass left the sums] -> chain_grid_summary_kernel<kind> (one wave per
//    wave-chunk, over the chip) -> chain_grid_walk_kernel<kind> (ONE wave)
//    tdr_config_prefix_small(0), or a caller without room for the wave-chunk records (grid = false): chain_summary_kernel
//    over every 4096-chunk -> chain_walk_kernel (one workgroup, from the first addend on)
//  tdr_uw_chunk_pass1 / _pass2 (tdr_k_update_weights, n > 32 768): uw_chunk_pass1_kernel / uw_chunk_pass2_kernel, one
//    workgroup per chain chunk: the count of valid weights / of weights below the mean, and the chunk and wave-chunk sums
//    of the chain that follows (chain_sum_body)
//  tdr_batch_update_weights / tdr_batch_prefix: uw_small_batch_kernel / pfx_small_batch_kernel, one workgroup per filter
//
// Order of the file: the one-wave serial kernel; the one-workgroup tie-list kernel; the parity-pair chain step and
// what it is made of (written once, used by every kernel behind it); the multi-workgroup kernels at 4096-chunk grain;
// the one-workgroup kernels; the chip-wide kernels at wave-chunk grain, which reuse the one-workgroup kernels' wave-level
// pieces; dispatch.  tests/test_gpu_parity.py compares every path with the CPU chains bit for bit; what the update does
// behind its chains (fill or fallback, the two normalisations, the blend, the first maximum) is held to an exact
// statement, on both one-workgroup kernels and the multi-workgroup passes, in tests/test_uw_exact.py.
//
// ---- one wave, serially --------------------------------------------------------------------------------------------------
// prefix_serial_kernel: lane 0 performs the additions in index order (weights staged through LDS).  Simple, ~10 ns per
// element; kept as the reference implementation and for small n.  The running maximum makes "first j with prefix_j >
// sample" searchable even when weights are negative (NaN fill, :133).
//
// prefix_exact_kernel (below it): while the running sum r stays inside one binade [2^e, 2^(e+1)) it is an integer
// multiple R*u of u = 2^(e-23) and fl(r + w) = (R + q)*u, where q is w/u rounded to nearest — a pure integer increment
// that depends on r only when w/u ends in exactly .5 (tie to even: the parity of R + floor(w/u)).  Per tile of 8192
// weights the workgroup (i) classifies every weight into an integer increment / tie / "needs a real float add" (NaN,
// inf, larger than the binade), (ii) prefix-sums the increments, (iii) resolves the (rare) ties in order on one thread,
// (iv) prefix-sums the tie corrections, (v) finds the first element at which the sum leaves the binade or a real add
// is needed, commits everything before it, performs that one addition in float arithmetic and restarts behind it in
// the new binade.  It handles every running sum (negative, subnormal, inf, NaN) and weights of either sign.
#define TDR_PFX_BLOCK 4096  // elements staged in LDS per pass (64 per lane)
__global__ __launch_bounds__(64) void prefix_serial_kernel(const float* __restrict__ w, int64_t n,
                                                           float* __restrict__ runmax) {
  __shared__ float4 buf4[TDR_PFX_BLOCK / 4];
  float* buf = reinterpret_cast<float*>(buf4);
  const int lane = threadIdx.x;
  float run = 0.f;        // the serial chain lives in lane 0
  float carry_max = -INFINITY;
  for (int64_t base = 0; base < n; base += TDR_PFX_BLOCK) {
    const int cnt = (int)min((int64_t)TDR_PFX_BLOCK, n - base);
    // coalesced stage-in (pad with zeros: x + 0 == x)
    for (int t = lane; t < TDR_PFX_BLOCK; t += 64) buf[t] = (t < cnt) ? w[base + t] : 0.f;
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
      const int q4 = (cnt + 3) / 4;
#pragma unroll 4
      for (int q = 0; q < q4; q++) {
        float4 v = buf4[q];
        run = run + v.x; v.x = run;   // particle_filter.cpp:179, one float add per weight, index order
        run = run + v.y; v.y = run;
        run = run + v.z; v.z = run;
        run = run + v.w; v.w = run;
        buf4[q] = v;
      }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // running maximum of the block's prefix values (max is associative: any order is exact)
    float m = -INFINITY;
    float loc[64];
#pragma unroll
    for (int t = 0; t < 64; t++) {
      float x = buf[lane * 64 + t];
      if (x != x) x = -INFINITY;  // a NaN prefix never exceeds a threshold (`running_sum > sample` is false)
      m = fmaxf(m, x);
      loc[t] = m;
    }
    float incl = m;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      float t = __shfl_up(incl, o, 64);
      if (lane >= o) incl = fmaxf(incl, t);
    }
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = -INFINITY;
    excl = fmaxf(excl, carry_max);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < 64; t++) buf[lane * 64 + t] = fmaxf(loc[t], excl);
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    for (int t = lane; t < cnt; t += 64) runmax[base + t] = buf[t];
    carry_max = fmaxf(__shfl(incl, 63, 64), carry_max);
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- exact parallel prefix in one workgroup: the tie-list algorithm (mode 1; the chunk walk's general fallback) -------------------------------------------------------------------------------------------
#define PFX_THREADS 1024
#define PFX_K 8
#define PFX_TILE (PFX_THREADS * PFX_K)
#define PFX_TIE_CAP 2048   // ties resolved per pass; a (never observed) denser tile is simply cut at that tie

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every outstanding global store
// (~1 us each time); in the prefix kernels the threads exchange data through LDS alone — global memory is read-only
// input (w, chunk headers of an earlier launch) or write-only output — so the store wait would be pure latency.
__device__ __forceinline__ void pfx_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// inclusive block scan (sum) of one value per thread; `sh` holds one slot per wave
template <int NT, class T>
__device__ __forceinline__ T pfx_block_scan(T v, T* sh, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  pfx_sync();
  if (lane == 63) sh[wave] = v;
  pfx_sync();
  T off = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < NT / 64; k++) {
    const T x = sh[k];
    if (k < wave) off += x;
    tot += x;
  }
  total = tot;
  return v + off;
}
template <int NT>
__device__ __forceinline__ float pfx_block_scan_max(float v, float* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    float t = __shfl_up(v, o, 64);
    if (lane >= o) v = fmaxf(v, t);
  }
  pfx_sync();
  if (lane == 63) sh[wave] = v;
  pfx_sync();
  float off = -INFINITY;
  for (int k = 0; k < wave; k++) off = fmaxf(off, sh[k]);
  return fmaxf(v, off);
}

// The running sum carried through [lo, hi) in index order by the whole workgroup (NT threads): r_io / carry_io
// are the (workgroup-uniform) running sum and running maximum before element lo on entry and after element hi-1 on
// exit.  With lo == 0 the first PFX_HEAD elements are added one by one.
template <int NT>
__device__ __forceinline__ void pfx_exact_range(const float* __restrict__ w, long long lo, long long hi,
                                             float* __restrict__ runmax, float* __restrict__ prefix_opt,
                                             float& r_io, float& carry_io, int head_len = PFX_HEAD) {
  const long long n = hi;
  __shared__ long long sh_ll[NT / 64];
  __shared__ int sh_i[NT / 64];
  __shared__ float sh_f[NT / 64];
  __shared__ int tie_pos[PFX_TIE_CAP];         // local element index of every tie in order, weight sign in bit 31
  __shared__ long long tie_sval[PFX_TIE_CAP];  // inclusive increment prefix at the tie
  __shared__ signed char tie_corr[PFX_TIE_CAP];
  __shared__ float head[PFX_HEAD];
  __shared__ float last_val[NT], last_max[NT];
  __shared__ int s_first_bad, s_first_cross, s_first_nz;
  __shared__ float s_r, s_carry;
  __shared__ long long s_base;
  const int tid = threadIdx.x;
  pfx_sync();
  if (tid == 0) { s_r = r_io; s_carry = carry_io; s_base = lo; }
  pfx_sync();
  if (lo == 0) {  // head: plain serial additions by one thread out of LDS
    const int hn = (int)min((long long)head_len, (long long)n);
    for (int t = tid; t < hn; t += NT) head[t] = w[t];
    pfx_sync();
    if (tid == 0) {
      float run = 0.f, mx = -INFINITY;
      for (int t = 0; t < hn; t++) {
        run = run + head[t];  // particle_filter.cpp:179
        if (prefix_opt) prefix_opt[t] = run;
        if (run == run) mx = fmaxf(mx, run);
        head[t] = mx;
      }
      s_r = run; s_carry = mx; s_base = hn;
    }
    pfx_sync();
    for (int t = tid; t < hn; t += NT) runmax[t] = head[t];
    pfx_sync();
  }

  while (true) {
    const long long base = s_base;
    if (base >= n) break;
    const float r = s_r;
    const float carry = s_carry;
    const int cnt = (int)min((long long)(NT * PFX_K), (long long)n - base);
    const unsigned rb = __float_as_uint(r);
    const int re = (rb >> 23) & 0xFF;
    float wv[PFX_K];
#pragma unroll
    for (int k = 0; k < PFX_K; k++) {
      const int li = tid * PFX_K + k;
      wv[k] = (li < cnt) ? w[base + li] : 0.f;
    }
    if (tid == 0) { s_first_bad = (NT * PFX_K); s_first_cross = (NT * PFX_K); s_first_nz = (NT * PFX_K); }
    pfx_sync();  // also: everyone has read s_r / s_carry / s_base

    if (r != r) {  // NaN running sum: every later prefix is NaN, the running maximum stays
#pragma unroll
      for (int k = 0; k < PFX_K; k++) {
        const int li = tid * PFX_K + k;
        if (li < cnt) {
          runmax[base + li] = carry;
          if (prefix_opt) prefix_opt[base + li] = r;
        }
      }
      pfx_sync();
      if (tid == 0) s_base = base + cnt;
      pfx_sync();
      continue;
    }
    const bool r_zero = (rb & 0x7FFFFFFFu) == 0;
    const bool r_slow = (rb >> 31) != 0 || re == 0 || re == 255;  // negative, zero / subnormal, inf: plain float steps
    if (r_slow) {
      int stop = 0;  // leading elements that leave r unchanged (r == +-0 only: skip the run of zero weights)
      if (r_zero) {
#pragma unroll
        for (int k = 0; k < PFX_K; k++) {
          const int li = tid * PFX_K + k;
          if (li < cnt && (__float_as_uint(wv[k]) & 0x7FFFFFFFu) != 0) atomicMin(&s_first_nz, li);
        }
        pfx_sync();
        stop = min(s_first_nz, cnt);
      }
      const float m0 = fmaxf(carry, r);
#pragma unroll
      for (int k = 0; k < PFX_K; k++) {
        const int li = tid * PFX_K + k;
        if (li < stop) {
          runmax[base + li] = m0;
          if (prefix_opt) prefix_opt[base + li] = r;
        }
      }
      pfx_sync();
      if (tid == 0) {
        float nr = r, nc = stop > 0 ? m0 : carry;
        long long nb = base + stop;
        if (stop < cnt) {  // one real float addition (particle_filter.cpp:179)
          nr = r + w[base + stop];
          if (nr == nr) nc = fmaxf(nc, nr);
          runmax[base + stop] = nc;
          if (prefix_opt) prefix_opt[base + stop] = nr;
          nb = base + stop + 1;
        }
        s_r = nr; s_carry = nc; s_base = nb;
      }
      pfx_sync();
      continue;
    }

    // ---- r is a positive normal float: r = R * 2^(e-23), R in [2^23, 2^24)
    const int e = re - 127;
    const long long R = (long long)((rb & 0x7FFFFFu) | 0x800000u);
    long long inc[PFX_K];
    bool tie[PFX_K], neg[PFX_K];
    long long tsum = 0;
    int ntie = 0;
#pragma unroll
    for (int k = 0; k < PFX_K; k++) {
      const int li = tid * PFX_K + k;
      const unsigned b = __float_as_uint(wv[k]);
      const int ew = (b >> 23) & 0xFF;
      unsigned mw = b & 0x7FFFFFu;
      const bool zero = (b & 0x7FFFFFFFu) == 0;
      const int E = ew == 0 ? -126 : ew - 127;
      if (ew != 0) mw |= 0x800000u;
      const int sft = e - E;
      const bool in = li < cnt;
      const bool bad = in && ((ew == 255) || (sft < 0));  // NaN / inf / at least as large as the binade: real add
      neg[k] = (b >> 31) != 0 && !zero;
      const int sc = sft < 0 ? 0 : (sft > 26 ? 26 : sft);
      const unsigned f = mw >> sc;
      const unsigned rem = mw & ((1u << sc) - 1u);
      const unsigned half = sc >= 1 ? (1u << (sc - 1)) : 0u;
      const bool up = sc >= 1 && rem > half;
      tie[k] = in && !bad && sc >= 1 && rem == half;
      long long q = (long long)f + (up ? 1 : 0);  // |w|/u rounded to nearest (ties toward zero, patched below)
      if (neg[k]) q = -q;
      if (!in || bad) q = 0;
      if (bad) atomicMin(&s_first_bad, li);
      inc[k] = q;
      tsum += q;
      ntie += tie[k] ? 1 : 0;
    }
    long long tot_ll;
    const long long sincl = pfx_block_scan<NT, long long>(tsum, sh_ll, tot_ll);
    long long S[PFX_K];  // inclusive prefix of the increments at this thread's elements
    {
      long long acc = sincl - tsum;
#pragma unroll
      for (int k = 0; k < PFX_K; k++) { acc += inc[k]; S[k] = acc; }
    }
    // ---- ties, in element order: the even neighbour wins, which depends on everything before the tie
    int tot_tie;
    const int tincl = pfx_block_scan<NT, int>(ntie, sh_i, tot_tie);
    const int tfirst = tincl - ntie;
    {
      int pos = tfirst;
#pragma unroll
      for (int k = 0; k < PFX_K; k++)
        if (tie[k]) {
          if (pos < PFX_TIE_CAP) {
            tie_pos[pos] = (tid * PFX_K + k) | (neg[k] ? (int)0x80000000 : 0);
            tie_sval[pos] = S[k];
          } else if (pos == PFX_TIE_CAP) {
            atomicMin(&s_first_bad, tid * PFX_K + k);  // more ties than slots: cut the tile here
          }
          pos++;
        }
    }
    pfx_sync();
    if (tid == 0 && tot_tie > 0) {
      long long c = 0;
      const int fb = s_first_bad;
      const int nt = min(tot_tie, PFX_TIE_CAP);
      for (int t = 0; t < nt; t++) {
        const int pk = tie_pos[t];
        const int li = pk & 0x7FFFFFFF;
        signed char corr = 0;
        if (li < fb) {
          const long long V = R + tie_sval[t] + c;  // mantissa if the tie is rounded toward zero
          if (V & 1) corr = (pk < 0) ? -1 : 1;      // exact value is V +- 1/2: move to the even neighbour
        }
        tie_corr[t] = corr;
        c += corr;
      }
    }
    pfx_sync();
    int csum = 0;
    int corr[PFX_K];
    {
      int pos = tfirst;
#pragma unroll
      for (int k = 0; k < PFX_K; k++) {
        corr[k] = 0;
        if (tie[k]) { corr[k] = pos < PFX_TIE_CAP ? tie_corr[pos] : 0; pos++; }
        csum += corr[k];
      }
    }
    int tot_c;
    const int cincl = pfx_block_scan<NT, int>(csum, sh_i, tot_c);
    // ---- mantissas, first element that leaves the binade
    long long state[PFX_K];
    {
      int cacc = cincl - csum;
#pragma unroll
      for (int k = 0; k < PFX_K; k++) {
        cacc += corr[k];
        state[k] = R + S[k] + cacc;
        const int li = tid * PFX_K + k;
        if (li < cnt && (state[k] >= (1ll << 24) || state[k] < (1ll << 23))) atomicMin(&s_first_cross, li);
      }
    }
    pfx_sync();
    const int stop = min(min(s_first_bad, s_first_cross), cnt);
    // ---- commit [0, stop): values and running maximum
    float val[PFX_K], lm[PFX_K];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < PFX_K; k++) {
      const int li = tid * PFX_K + k;
      val[k] = __uint_as_float(((unsigned)re << 23) | ((unsigned)state[k] & 0x7FFFFFu));
      if (li < stop) m = fmaxf(m, val[k]);
      lm[k] = m;
    }
    const float mincl = pfx_block_scan_max<NT>(m, sh_f);
    float mexcl = __shfl_up(mincl, 1, 64);
    {  // exclusive maximum over the preceding threads
      pfx_sync();
      last_max[tid] = mincl;
      pfx_sync();
      mexcl = tid > 0 ? last_max[tid - 1] : -INFINITY;
    }
    const float mbase = fmaxf(carry, mexcl);
    float lastv = r, lastm = carry;
#pragma unroll
    for (int k = 0; k < PFX_K; k++) {
      const int li = tid * PFX_K + k;
      if (li < stop) {
        const float rm = fmaxf(mbase, lm[k]);
        runmax[base + li] = rm;
        if (prefix_opt) prefix_opt[base + li] = val[k];
        lastv = val[k];
        lastm = rm;
      }
    }
    pfx_sync();
    last_val[tid] = lastv;   // value / running max at this thread's last committed element (if any)
    last_max[tid] = lastm;
    pfx_sync();
    if (tid == 0) {
      float pv = r, pm = carry;  // value / running max at element stop-1
      if (stop > 0) {
        const int ot = (stop - 1) / PFX_K;
        pv = last_val[ot];
        pm = last_max[ot];
      }
      long long nb = base + stop;
      if (stop < cnt) {  // one real float addition, then a new binade
        const float nr = pv + w[base + stop];
        if (nr == nr) pm = fmaxf(pm, nr);
        runmax[base + stop] = pm;
        if (prefix_opt) prefix_opt[base + stop] = nr;
        pv = nr;
        nb = base + stop + 1;
      }
      s_r = pv; s_carry = pm; s_base = nb;
    }
    pfx_sync();
  }
  r_io = s_r;
  carry_io = s_carry;
  pfx_sync();
}

__global__ __launch_bounds__(PFX_THREADS) void prefix_exact_kernel(const float* __restrict__ w, int64_t n,
                                                                   float* __restrict__ runmax,
                                                                   float* __restrict__ prefix_opt) {
  float r = 0.f, carry = -INFINITY;
  pfx_exact_range<PFX_THREADS>(w, 0, n, runmax, prefix_opt, r, carry);
}

// ==== exact chains over parity pairs ===================================================================================
// Inside one binade (ulp u) the chain r <- fl(r + x) with x >= 0 is R <- R + a(R & 1): the increment of one addend is
// an integer that depends on the running mantissa only through its PARITY (round-half-even ties).  A run of addends is
// therefore summarised by two integers (D0, D1) — its total increment entered with an even / odd mantissa — and
// summaries compose associatively: (A then B)_p = A_p + B_{(p + A_p) & 1}.  That turns a chain into a scan plus one real
// addition at every binade crossing.  Everything below is built from four pieces, each written once:
//   ChainAddend   what a chain adds: value type, where element i comes from, its classification in a binade, the real add
//   chain_step    one stretch inside a binade: classify, compose and scan the pairs, rebuild every mantissa, find the first
//                 addend that needs a real addition
//   chain_walk    a chunk: steps, what lies before each stop committed to a sink, the real additions in between
//   chain_head_*  the leading addends one by one (the sum starts at zero and doubles every few addends)
// Every value produced is the serial float32 chain's, whatever a prediction was: a wrong one only sends a chunk down the
// slower path.
#define PFXM_THREADS 256
#define PFXM_K 16
#define PFXM_CHUNK (PFXM_THREADS * PFXM_K)
#define PFXM_SAT (1u << 30)
struct PfxChunk {     // 32 bytes per chunk in the caller's workspace
  double sum;         // 1: double sum of the chunk
  int re;             // 2: predicted biased exponent of the running sum, or -1 = irregular
  unsigned d0, d1;    // 2: total increment entered with an even / odd mantissa
  float r0, carry0;   // 3: running sum / running maximum before the chunk's first element (accepted chunks)
  int accepted;       // 3: 1 = pfx_chunk_fill_kernel writes this chunk's outputs
};
static_assert(sizeof(PfxChunk) == 32, "PfxChunk");
// Above 32 768 addends the workspace continues behind the chunk headers with one record per wave-chunk (UWS_WC addends),
// a few control words and the dual slots of the crossing chunks ("the long chains at wave-chunk grain", below).
struct WcRec {        // 24 bytes per wave-chunk
  double sum;         // 1: double sum of the wave-chunk (any order of additions: it feeds predictions only)
  int code;           // 2: -1: carried through; binade; binade | UWS_DUAL_FLAG | slot << 16
  unsigned d0, d1;    // 2: parity pair of a one-binade chunk
  float rin;          // 3: exact running sum in front of the chunk (the running sum's refill)
};
struct WcCtl {
  int slots;          // 1: zeroed; 2: dual slots handed out
  int irregular;      // 3: the running sum's input holds a negative or NaN weight: the 4096-chunk walk took it
  int pad[2];
};
#define UWG_DUAL_SLOTS 32   // 1 KB each; a crossing chunk beyond them is carried through (uws_wave_walk)
struct ChainGridWs {
  PfxChunk* ch;       // [nch]
  WcRec* wc;          // [nwc]
  int* irr;           // [nch] 1: per chunk, a weight that is negative or NaN (running sum only)
  WcCtl* ctl;
  uint4* dual;        // [UWG_DUAL_SLOTS][64]
};
#ifndef PFXW_THREADS
#define PFXW_THREADS 512   // the walking workgroup: PFXW_THREADS x PFXW_K = one chunk (two waves per SIMD: the dependent
#endif                     // instruction chains of one wave hide behind the other's)
#define PFXW_K (PFXM_CHUNK / PFXW_THREADS)
#define CHAIN_K PFXW_K            // addends per lane of a walking wave
#define UWS_WC (64 * CHAIN_K)     // addends per wave-chunk
#define PFXM_RE_MIN 24            // binades (biased exponent, sign bit included) a step works in: positive normal sums
#define PFXM_RE_MAX 254           // whose ulp's reciprocal 2^(150 - re) is a normal float

#ifdef TDR_UW_TIMELINE   // diagnostic build: 100 MHz time stamps at the phase boundaries of uw_small_kernel
__device__ unsigned long long g_uw_tl[16];
extern "C" int tdr_debug_read_uw_timeline(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_uw_tl), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -1;
}
#define UW_STAMP(k) do { __syncthreads(); if (threadIdx.x == 0) g_uw_tl[k] = wall_clock64(); } while (0)
#define UW_COUNT(k) do { if (threadIdx.x == 0) g_uw_tl[k]++; } while (0)
#else
#define UW_STAMP(k) do { } while (0)
#define UW_COUNT(k) do { } while (0)
#endif

// ---- parity pairs and their scans ---------------------------------------------------------------------------------------
struct PfxPair { unsigned a0, a1; };
__device__ __forceinline__ unsigned pfx_sat(unsigned x) { return x > PFXM_SAT ? PFXM_SAT : x; }
// first A, then B
__device__ __forceinline__ PfxPair pfx_compose(PfxPair A, PfxPair B) {
  PfxPair c;
  c.a0 = pfx_sat(A.a0 + ((A.a0 & 1u) ? B.a1 : B.a0));
  c.a1 = pfx_sat(A.a1 + ((A.a1 & 1u) ? B.a0 : B.a1));   // entered odd: the parity after A is (1 + A.a1) & 1
  return c;
}
__device__ __forceinline__ PfxPair pfx_element_pair(unsigned f, bool tie) {
  PfxPair p;
  p.a0 = f + (tie ? (f & 1u) : 0u);         // even mantissa + f + 1/2 -> the even neighbour
  p.a1 = f + (tie ? ((f & 1u) ^ 1u) : 0u);
  return p;
}
// the pair of one lane's K consecutive addends (increments f, bit k of tiebits: addend k is a rounding tie)
template <int K>
__device__ __forceinline__ PfxPair chain_lane_pair(const unsigned (&f)[K], unsigned tiebits) {
  PfxPair mine = {0u, 0u};
#pragma unroll
  for (int k = 0; k < K; k++) mine = pfx_compose(mine, pfx_element_pair(f[k], ((tiebits >> k) & 1u) != 0u));
  return mine;
}
// Inclusive wave scan of pairs with data-parallel-primitive moves instead of LDS permutes (each __shfl_up is a
// ds_bpermute: ~100 clocks of latency, twelve of them in a row per scan).  Lanes without a source lane receive the
// identity pair {0, 0} (compose({0,0}, v) == v), so no lane predicate is needed.  Steps: shift right by 1, 2, 4, 8
// within rows of 16 lanes, then lane 15 of rows 0 / 2 into rows 1 / 3, then lane 31 into rows 2 and 3.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ PfxPair pfx_pair_dpp(PfxPair v) {
  PfxPair t;
  t.a0 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v.a0, CTRL, ROW_MASK, 0xF, false);
  t.a1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v.a1, CTRL, ROW_MASK, 0xF, false);
  return t;
}
__device__ __forceinline__ PfxPair pfx_pair_wave_scan(PfxPair v) {
  v = pfx_compose(pfx_pair_dpp<0x111, 0xF>(v), v);   // row_shr:1
  v = pfx_compose(pfx_pair_dpp<0x112, 0xF>(v), v);   // row_shr:2
  v = pfx_compose(pfx_pair_dpp<0x114, 0xF>(v), v);   // row_shr:4
  v = pfx_compose(pfx_pair_dpp<0x118, 0xF>(v), v);   // row_shr:8
  v = pfx_compose(pfx_pair_dpp<0x142, 0xA>(v), v);   // row_bcast:15 into rows 1 and 3
  v = pfx_compose(pfx_pair_dpp<0x143, 0xC>(v), v);   // row_bcast:31 into rows 2 and 3
  return v;
}
// inclusive scan of per-thread pairs over a workgroup of NT threads; returns the EXCLUSIVE pair of this thread and the
// workgroup total.  `sh` holds one slot per wave; safe to call repeatedly (leading barrier).
template <int NT>
__device__ __forceinline__ PfxPair pfx_pair_scan(PfxPair v, PfxPair* sh, PfxPair& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = pfx_pair_wave_scan(v);
  pfx_sync();
  if (lane == 63) sh[wave] = v;
  pfx_sync();
  PfxPair pre = {0u, 0u}, tot = {0u, 0u};
#pragma unroll
  for (int k = 0; k < NT / 64; k++) {
    const PfxPair x = sh[k];
    if (k < wave) pre = pfx_compose(pre, x);
    tot = pfx_compose(tot, x);
  }
  total = tot;
  // exclusive: the inclusive value of the lane before (wave_shr:1; lane 0 gets the identity)
  PfxPair ex = pfx_pair_dpp<0x138, 0xF>(v);
  return pfx_compose(pre, ex);
}
// the same six moves for a minimum, a double sum, an unsigned sum and a float maximum
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int uws_min_dpp(int v) {
  return min(v, __builtin_amdgcn_update_dpp(0x7FFFFFFF, v, CTRL, ROW_MASK, 0xF, false));
}
__device__ __forceinline__ int uws_wave_min(int v) {   // minimum over the wave, in every lane (uniform)
  v = uws_min_dpp<0x111, 0xF>(v);
  v = uws_min_dpp<0x112, 0xF>(v);
  v = uws_min_dpp<0x114, 0xF>(v);
  v = uws_min_dpp<0x118, 0xF>(v);
  v = uws_min_dpp<0x142, 0xA>(v);
  v = uws_min_dpp<0x143, 0xC>(v);
  return __builtin_amdgcn_readlane(v, 63);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double uws_add_dpp(double v) {   // lanes without a source add 0.0
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xF, false);
  return v + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double uws_wave_scan_d(double v) {   // inclusive sum over the lanes before and this one
  v = uws_add_dpp<0x111, 0xF>(v);
  v = uws_add_dpp<0x112, 0xF>(v);
  v = uws_add_dpp<0x114, 0xF>(v);
  v = uws_add_dpp<0x118, 0xF>(v);
  v = uws_add_dpp<0x142, 0xA>(v);
  v = uws_add_dpp<0x143, 0xC>(v);
  return v;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned uws_addu_dpp(unsigned v) {
  return v + (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ unsigned uws_wave_scan_u(unsigned v) {
  v = uws_addu_dpp<0x111, 0xF>(v);
  v = uws_addu_dpp<0x112, 0xF>(v);
  v = uws_addu_dpp<0x114, 0xF>(v);
  v = uws_addu_dpp<0x118, 0xF>(v);
  v = uws_addu_dpp<0x142, 0xA>(v);
  v = uws_addu_dpp<0x143, 0xC>(v);
  return v;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float pfs_max_dpp(float v) {
  return fmaxf(v, __uint_as_float((unsigned)__builtin_amdgcn_update_dpp((int)0xFF800000u, (int)__float_as_uint(v), CTRL,
                                                                        ROW_MASK, 0xF, false)));
}
__device__ __forceinline__ float pfs_wave_scan_max(float v) {   // inclusive maximum over the lanes before and this one
  v = pfs_max_dpp<0x111, 0xF>(v);
  v = pfs_max_dpp<0x112, 0xF>(v);
  v = pfs_max_dpp<0x114, 0xF>(v);
  v = pfs_max_dpp<0x118, 0xF>(v);
  v = pfs_max_dpp<0x142, 0xA>(v);
  v = pfs_max_dpp<0x143, 0xC>(v);
  return v;
}
__device__ __forceinline__ double uws_readlane_d(double v, int lane) {   // lane: wave-uniform
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                          __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ double chain_readlane(double v, int lane) { return uws_readlane_d(v, lane); }
__device__ __forceinline__ float chain_readlane(float v, int lane) {
  return __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(v), lane));
}
// Workgroup sum of one double per thread: a __shfl_xor tree inside every wave, then the waves in order.  The order of
// the additions is fixed — these sums feed the binade predictions, and a launch stays a pure function of its inputs.
// (uws_sum_d below adds in another order, a DPP scan inside the wave, and is therefore a function of its own: a
// different double sum can flip a prediction — harmless for the bits, but it moves chunks between the fast and the
// slow path.)  Values written to LDS before the call are visible to every thread behind it.
template <int NT>
__device__ __forceinline__ double chain_wg_sum(double acc, double* shd) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) shd[threadIdx.x >> 6] = acc;
  pfx_sync();
  double t = 0.0;
  for (int k = 0; k < NT / 64; k++) t += shd[k];
  return t;
}

// ---- what a chain adds ---------------------------------------------------------------------------------------------------
// The three chains (src/particle_filter.cpp):
//   CHAIN_SUM     :108-116  sum += w             float addends, NaN weights skipped
//   CHAIN_BOTTOM  :118-126  acc += pow(w - mean, 2) over the weights below the mean: (float)((double)acc + x), x a double
//   CHAIN_RUNSUM  :179      running_sum += w     float addends, NaN weights added like any other
enum { CHAIN_SUM = 0, CHAIN_BOTTOM = 1, CHAIN_RUNSUM = 2 };
// where element i comes from: an array in memory (nothing is read where `take` is false) ...
struct ChainGlobal {
  const float* p;
  static constexpr bool lds = false;
  __device__ __forceinline__ float read(long long i, bool take) const { return take ? p[i] : 0.f; }
};
// ... or the image of the weights the one-workgroup kernels keep in their dynamic LDS array.  GUARD = false reads
// unconditionally, ahead of the test (the image ends in UWS_PAD unused words behind the last weight).
__device__ __forceinline__ int uws_idx(int e) { return e + (e >> 5); }   // one pad word per 32: bank spread for strided runs
#define UWS_PAD 16
template <bool GUARD>
struct ChainLds {
  static constexpr bool lds = true;
  __device__ __forceinline__ float read(long long i, bool take) const {
    extern __shared__ float uws_lraw[];
    if (GUARD) return take ? uws_lraw[uws_idx((int)i)] : 0.f;
    return uws_lraw[uws_idx((int)i)];
  }
};
// The real addition, in the reference's types.  float + float equals the double form for every pair of floats —
// (float)((double)a + (double)b) == a + b: 53 >= 2 * 24 + 2 bits, the double sum rounds to the same float — and is a
// third of the dependent latency; so the float chains may be carried in either type, and each use keeps the one its
// timing was measured with.
__device__ __forceinline__ float chain_add(float r, float x) { return r + x; }
__device__ __forceinline__ float chain_add(float r, double x) { return (float)((double)r + x); }
__device__ __forceinline__ bool chain_finite(float x) { return fabsf(x) < INFINITY; }
__device__ __forceinline__ bool chain_finite(double x) { return fabs(x) < INFINITY; }
// One addend x against the binade of a running sum with biased exponent `re` (PFXM_RE_MIN <= re <= PFXM_RE_MAX), ulp
// u = 2^(re-150): f = round-half-down(x/u), tie = the remainder is exactly one half, bad = cannot be an integer
// increment (NaN, inf, negative, or x/u >= bound).  x * 2^(150-re) is exact (a power-of-two scaling inside the normal
// range; a product that underflows is far below one half anyway), and so are floor and the remainder.
//
// The bound.  Anything up to 2^24 keeps the arithmetic right: f < 2^24 and R < 2^24 stay far from the pairs' saturation
// (PFXM_SAT) and a mantissa that reaches 2^24 stops the step, so a large addend only ends a stretch where a smaller bound
// would have ended it one element earlier with the same real addition.  CHAIN_BOUND_24 is what the multi-workgroup running
// sum takes (summary, walk and fill must agree with each other: a chunk accepted by the summary is refilled without a
// stop search).  CHAIN_BOUND_22 serves two needs: the double classifier rounds x/u to the double grid of [2^23, 2^24)
// by adding 2^23, which needs x/u < 2^23; and the wave-level summaries add the f of a whole wave-chunk as plain unsigned
// numbers when no tie occurs (8 per lane < 2^25, 64 lanes < 2^31).  Reading the code, 2^22 would serve every caller with
// the same bits (the bound only moves an element between "scan" and "real addition", which give the same float); the
// bounds are nevertheless kept per use as they were measured.
#define CHAIN_BOUND_24 24
#define CHAIN_BOUND_22 22
template <int LOG2_BOUND>
__device__ __forceinline__ void chain_classify(float x, unsigned re, unsigned& f, bool& tie, bool& bad) {
  const float t = x * __uint_as_float((277u - re) << 23);   // x / u: 2^(150 - re) = 1/u
  bad = !(x >= 0.f) || !(t < (float)(1 << LOG2_BOUND));
  const float fl = floorf(t);
  const float fr = t - fl;
  tie = fr == 0.5f;
  f = (unsigned)fl + (fr > 0.5f ? 1u : 0u);
  if (bad) { f = 0; tie = false; }
}
// A double addend: for a float chain r <- (float)((double)r + x) the step is x first rounded to the double grid of the
// sum's binade — 2^-29 ulp(r), and because R is an integer that rounding does not depend on R — and then to the float
// grid with the parity rule.  (A float addend lies on the double grid or is far below half an ulp, so a float chain
// classified here gives what the float classifier gives.)
template <int LOG2_BOUND>
__device__ __forceinline__ void chain_classify(double x, unsigned re, unsigned& f, bool& tie, bool& bad) {
  const double scale = __longlong_as_double((long long)(1023 + 150 - (int)re) << 52);   // 2^(150 - re) = 1/u
  const double t = x * scale;
  bad = !(x >= 0.0) || !(t < (double)(1 << LOG2_BOUND));   // negative / NaN / inf, or not small against the sum: real add
  const double tg = (t + 8388608.0) - 8388608.0;           // t on the double grid of [2^23, 2^24): multiples of 2^-29
  const double fl = floor(tg);
  const double fr = tg - fl;
  tie = fr == 0.5;
  f = (unsigned)fl + (fr > 0.5 ? 1u : 0u);
  if (bad) { f = 0; tie = false; }
}
// X: the type the addends are carried in (double for CHAIN_BOTTOM; float or double for the two float chains, see
// chain_add); SRC: ChainGlobal / ChainLds; LOG2B: the classifier's bound.  `kind` is a compile-time constant wherever
// it matters (everything here is inlined); the kernels that serve both statistics chains pass it at run time.
template <class X, class SRC, int LOG2B>
struct ChainAddend {
  using value_t = X;
  using src_t = SRC;
  SRC src;
  int kind;     // CHAIN_*
  float mean;   // CHAIN_BOTTOM
  __device__ __forceinline__ X value(float v) const {
    if (kind == CHAIN_RUNSUM) return (X)v;
    if (kind == CHAIN_SUM) return (v != v) ? X(0) : (X)v;       // :111-115
    if (v != v || !(v < mean)) return X(0);                     // :120
    const double d = (double)(v - mean);                        // float subtraction, then pow(double, 2)
    return (X)(d * d);
  }
  __device__ __forceinline__ X load(long long i, bool take) const {   // addend i if `take`, else zero (x + 0 == x)
    const X x = value(src.read(i, take));
    return take ? x : X(0);
  }
  // the K consecutive addends of the calling lane, from its element t0 of the chunk [lo, lo + cnt)
  template <int K>
  __device__ __forceinline__ void load_items(long long lo, int cnt, int t0, X (&xv)[K]) const {
    if constexpr (!SRC::lds && sizeof(X) == sizeof(float)) {
      if (t0 + K <= cnt && ((lo & 3) == 0)) {
        const float4* p = reinterpret_cast<const float4*>(src.p + lo + t0);
#pragma unroll
        for (int k = 0; k < K / 4; k++) {
          const float4 v = p[k];
          xv[4 * k] = value(v.x); xv[4 * k + 1] = value(v.y); xv[4 * k + 2] = value(v.z); xv[4 * k + 3] = value(v.w);
        }
        return;
      }
    }
#pragma unroll
    for (int k = 0; k < K; k++) xv[k] = load(lo + t0 + k, t0 + k < cnt);
  }
  static __device__ __forceinline__ void classify(X x, unsigned re, unsigned& f, bool& tie, bool& bad) {
    chain_classify<LOG2B>(x, re, f, tie, bad);
  }
  __device__ __forceinline__ ChainAddend<double, SRC, CHAIN_BOUND_22> as_double() const { return {src, kind, mean}; }
};
using PfxRunSum = ChainAddend<float, ChainGlobal, CHAIN_BOUND_24>;     // the multi-workgroup running sum (kind CHAIN_RUNSUM)
using ChainStat = ChainAddend<double, ChainGlobal, CHAIN_BOUND_22>;    // the multi-workgroup statistics chains
using UwsAddF = ChainAddend<float, ChainLds<false>, CHAIN_BOUND_22>;   // wave level, out of LDS: the float chains ...
using UwsAddD = ChainAddend<double, ChainLds<false>, CHAIN_BOUND_22>;  // ... and CHAIN_BOTTOM / the element-by-element walker
using UwsWgAdd = ChainAddend<double, ChainLds<true>, CHAIN_BOUND_22>;  // workgroup level, out of LDS (tdr_config_uw_waves(0))
__device__ __forceinline__ float chain_mant(unsigned re, unsigned state) { return __uint_as_float((re << 23) | (state & 0x7FFFFFu)); }

// ---- scope: who carries a stretch ------------------------------------------------------------------------------------------
// a workgroup of NT threads (LDS pair scan, atomicMin in LDS for the stop, LDS broadcast) ...
template <class X> struct ChainWgStop { int stop; unsigned state; X xstop; };
template <int NT, class X>
struct ChainWg {
  static constexpr bool nan_inf_apart = false;
  PfxPair* shp;           // one slot per wave
  ChainWgStop<X>* s;      // (not used without a stop search)
  __device__ __forceinline__ bool leader() const { return threadIdx.x == 0; }
  __device__ __forceinline__ void reset(int cnt) const {
    pfx_sync();
    if (threadIdx.x == 0) s->stop = cnt;
    pfx_sync();
  }
  template <int K>
  __device__ __forceinline__ unsigned enter(unsigned R, const unsigned (&f)[K], unsigned tiebits) const {
    PfxPair total;
    const PfxPair ex = pfx_pair_scan<NT>(chain_lane_pair(f, tiebits), shp, total);
    return R + ((R & 1u) ? ex.a1 : ex.a0);
  }
  __device__ __forceinline__ int first_of(int first, int cnt) const {
    if (first < cnt) atomicMin(&s->stop, first);
    pfx_sync();
    return s->stop;
  }
  // the mantissa behind element stop - 1 (when stop > pos) and the addend at `stop` (when stop < cnt), in every thread
  template <int K>
  __device__ __forceinline__ void pick(const unsigned (&st)[K], const X (&xv)[K], int t0, int pos, int stop, int cnt,
                                       unsigned& sv, X& xstop) const {
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int li = t0 + k;
      if (li >= pos && li == stop - 1) s->state = st[k];
      if (li == stop) s->xstop = xv[k];
    }
    pfx_sync();
    sv = s->state;
    xstop = s->xstop;
  }
};
// ... or one wave (DPP scans, readlane broadcasts, no barrier).  NOTIE: when no lane holds a rounding tie a pair is
// (s, s) and the scan is a plain integer prefix sum (needs CHAIN_BOUND_22).
template <bool NOTIE>
struct ChainWave {
  static constexpr bool nan_inf_apart = true;
  __device__ __forceinline__ bool leader() const { return (threadIdx.x & 63) == 0; }
  __device__ __forceinline__ void reset(int) const {}
  template <int K>
  __device__ __forceinline__ unsigned enter(unsigned R, const unsigned (&f)[K], unsigned tiebits) const {
    if (NOTIE && __ballot(tiebits != 0u) == 0ull) {
      unsigned lane_sum = 0u;
#pragma unroll
      for (int k = 0; k < K; k++) lane_sum += f[k];
      return R + (uws_wave_scan_u(lane_sum) - lane_sum);
    }
    const PfxPair ex = pfx_pair_dpp<0x138, 0xF>(pfx_pair_wave_scan(chain_lane_pair(f, tiebits)));   // exclusive: wave_shr:1
    return R + ((R & 1u) ? ex.a1 : ex.a0);
  }
  __device__ __forceinline__ int first_of(int first, int) const { return uws_wave_min(first); }
  template <int K, class X>
  __device__ __forceinline__ void pick(const unsigned (&st)[K], const X (&xv)[K], int t0, int pos, int stop, int cnt,
                                       unsigned& sv, X& xstop) const {
    unsigned v = 0u;   // in the lane that holds it: the mantissa before the stop, the addend at the stop
    X xs = X(0);
#pragma unroll
    for (int k = 0; k < K; k++) {
      if (t0 + k == stop - 1) v = st[k];
      if (t0 + k == stop) xs = xv[k];
    }
    if (stop > pos) sv = (unsigned)__builtin_amdgcn_readlane((int)v, (stop - 1) / K);
    if (stop < cnt) xstop = chain_readlane(xs, stop / K);
  }
};

// ---- sink: what is written -------------------------------------------------------------------------------------------------
// put(k, li, v): the running sum behind the lane's k-th addend, element li of the chunk, inside a stretch;
// committed(r): a stretch is done, r the sum behind it; put_stop(t0, li, r): element li was really added.
struct ChainNoSink {   // only the total is wanted
  static constexpr bool own_irregular = false;
  __device__ __forceinline__ void put(int, int, float) {}
  __device__ __forceinline__ void committed(float) {}
  __device__ __forceinline__ void put_stop(int, int, float) {}
};
template <int K>
struct ChainRegSink {   // into registers: the caller stores them (pfs_wave_fill: back into the LDS image)
  static constexpr bool own_irregular = false;
  float pv[K];
  __device__ __forceinline__ void put(int k, int, float v) { pv[k] = v; }
  __device__ __forceinline__ void committed(float) {}
  __device__ __forceinline__ void put_stop(int t0, int li, float r) {
#pragma unroll
    for (int k = 0; k < K; k++)
      if (t0 + k == li) pv[k] = r;
  }
};
// the running sum and the running maximum of chunk [lo, ..) to memory; a sum outside the binades a step works in goes
// to the general path, pfx_exact_range (with its serial head at the very start)
struct PfxGlobalSink {
  static constexpr bool own_irregular = true;
  const float* __restrict__ w;
  long long lo;
  float* __restrict__ runmax;
  float* __restrict__ prefix_opt;
  float& carry;
  int head_len;
  __device__ __forceinline__ void put(int, int li, float v) {
    runmax[lo + li] = fmaxf(carry, v);
    if (prefix_opt) prefix_opt[lo + li] = v;
  }
  __device__ __forceinline__ void committed(float r) { carry = fmaxf(carry, r); }   // increments are non-negative: the last committed value is the largest
  __device__ __forceinline__ void put_stop(int, int li, float nr) {
    if (nr == nr) carry = fmaxf(carry, nr);
    if (threadIdx.x == 0) {
      runmax[lo + li] = carry;
      if (prefix_opt) prefix_opt[lo + li] = nr;
    }
  }
  __device__ __forceinline__ void irregular(float& r, int& pos, int cnt) {
    const long long a = lo + pos;
    const long long b = a == 0 ? min((long long)head_len, (long long)cnt) : lo + cnt;
    pfx_exact_range<PFXW_THREADS>(w, a, b, runmax, prefix_opt, r, carry, head_len);
    pos = (int)(b - lo);
  }
};

// ---- the step ----------------------------------------------------------------------------------------------------------------
// One stretch of chunk elements [pos, cnt) inside the binade of r (a positive normal sum, PFXM_RE_MIN <= re <= PFXM_RE_MAX;
// pos, cnt and r uniform over the scope).  Every lane holds K consecutive addends xv from its element t0 on.  Classifies
// them, composes and scans the pairs, rebuilds the mantissa behind each of the lane's addends (st) and returns the
// lane's first element that needs a real addition — an addend the classifier calls bad, or the one that takes the
// mantissa to 2^24 — or cnt.  STOP = false: the caller knows that the whole chunk stays in the binade (an accepted
// chunk of the fill kernel): no masking, no search.
//
// What differs between the uses on purpose, and where it is selected:
//   * ChainWave<true> (pfs_wave_fill): plain integer scan when no lane holds a tie;
//   * STOP = false (pfx_chunk_fill_kernel), which also stores its values as float4s;
//   * a sum outside [PFXM_RE_MIN, PFXM_RE_MAX] never reaches the step; chain_walk sends it to the sink's own handler
//     (PfxGlobalSink: pfx_exact_range), or skips the addends that leave it unchanged and really adds the next one —
//     zero addends; under a scope with nan_inf_apart (the waves) also finite addends of an infinite sum, and a NaN sum
//     ends the chunk at once.
template <bool STOP, class A, int K, class SCOPE>
__device__ __forceinline__ int chain_step(const typename A::value_t (&xv)[K], int t0, int pos, int cnt, float r,
                                          const SCOPE& sc, unsigned (&st)[K]) {
  const unsigned rb = __float_as_uint(r), re = rb >> 23, R = (rb & 0x7FFFFFu) | 0x800000u;
  unsigned f[K];
  unsigned tiebits = 0u;
  int first = cnt;
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int li = t0 + k;
    bool bad, tie;
    A::classify(xv[k], re, f[k], tie, bad);
    if (STOP) {
      if (li < pos || li >= cnt) { f[k] = 0u; tie = false; bad = false; }
      if (bad) first = min(first, li);
    }
    tiebits |= tie ? (1u << k) : 0u;
  }
  unsigned state = sc.enter(R, f, tiebits);   // the exact mantissa before this lane's first element
#pragma unroll
  for (int k = 0; k < K; k++) {
    state += f[k] + (((tiebits >> k) & 1u) ? ((state + f[k]) & 1u) : 0u);   // a tie goes to the even neighbour
    st[k] = state;
    const int li = t0 + k;
    if (STOP && li >= pos && li < cnt && state >= (1u << 24)) first = min(first, li);
  }
  return first;
}
// Chunk elements [pos, cnt) carried through from the running sum r: stretches and real additions in turn.  Per turn:
// the first element that needs a real addition (`stop`), found by a step or, for a sum no step works on, by skipping
// the addends that leave it unchanged; the elements before it committed to the sink; that one addition.  Returns the
// sum behind the chunk.
template <class A, int K, class SCOPE, class SINK>
__device__ __forceinline__ float chain_walk(const A& a, const typename A::value_t (&xv)[K], int t0, int pos, int cnt,
                                            float r, const SCOPE& sc, SINK& sink) {
  using X = typename A::value_t;
  while (pos < cnt) {
#ifdef TDR_UW_TIMELINE
    if (A::src_t::lds && a.kind < 2 && sc.leader()) g_uw_tl[10 + a.kind]++;
#endif
    const unsigned rb = __float_as_uint(r);
    const unsigned re = rb >> 23;   // sign included
    const bool regular = re >= PFXM_RE_MIN && re <= PFXM_RE_MAX;
    if (SCOPE::nan_inf_apart && r != r) {   // NaN stays NaN
#pragma unroll
      for (int k = 0; k < K; k++)
        if (t0 + k >= pos && t0 + k < cnt) sink.put(k, t0 + k, r);
      break;
    }
    if constexpr (SINK::own_irregular) {
      if (!regular) {   // zero / tiny / huge / negative / inf / NaN running sum
        sink.irregular(r, pos, cnt);
        continue;
      }
    }
    sc.reset(cnt);
    int first = cnt;
    unsigned st[K] = {};
    if (!regular) {
      const bool isinf = SCOPE::nan_inf_apart && (rb & 0x7FFFFFFFu) == 0x7F800000u;
#pragma unroll
      for (int k = 0; k < K; k++) {
        const int li = t0 + k;
        const bool acts = isinf ? !chain_finite(xv[k]) : (xv[k] != X(0));
        if (li >= pos && li < cnt && acts) first = min(first, li);
      }
    } else {
      first = chain_step<true, A>(xv, t0, pos, cnt, r, sc, st);
    }
    const int stop = sc.first_of(first, cnt);   // first addend that is really added (cnt: none)
#pragma unroll
    for (int k = 0; k < K; k++)
      if (t0 + k >= pos && t0 + k < stop) sink.put(k, t0 + k, regular ? chain_mant(re, st[k]) : r);
    unsigned sv = 0u;
    X xstop = X(0);
    sc.pick(st, xv, t0, pos, stop, cnt, sv, xstop);
    if (regular) {
      if (stop > pos) r = chain_mant(re, sv);
      sink.committed(r);
    }
    if (stop < cnt) {
      r = chain_add(r, xstop);   // one real addition, in the reference's types
      sink.put_stop(t0, stop, r);
      pos = stop + 1;
    } else {
      pos = cnt;
    }
  }
  return r;
}

// ---- the heads ---------------------------------------------------------------------------------------------------------------
// The first hn addends one by one on one wave: 64 at a time into the lanes, then every lane runs the same chain over
// them.  KEEP (the running sum): every lane keeps the sum behind its own addend and hands it to keep(i, v).
template <bool KEEP, class A, class PUT>
__device__ __forceinline__ float chain_head_lanes(const A& a, int hn, PUT keep) {
  using X = typename A::value_t;
  const int lane = threadIdx.x & 63;
  float run = 0.f;
  X nxt = a.load(min(lane, hn - 1), lane < hn);
  for (int b = 0; b < hn; b += 64) {
    const X cur = nxt;
    nxt = a.load(min(b + 64 + lane, hn - 1), b + 64 + lane < hn);
    float mine = 0.f;
#pragma unroll
    for (int j = 0; j < 64; j++) {
      run = chain_add(run, chain_readlane(cur, j));
      if (KEEP) mine = (lane == j) ? run : mine;
    }
    if (KEEP && b + lane < hn) keep(b + lane, mine);
  }
  return run;
}
template <bool KEEP, class A>
__device__ __forceinline__ float chain_head_lanes(const A& a, int hn) {   // out of the LDS image and back into it
  extern __shared__ float uws_lraw[];
  return chain_head_lanes<KEEP>(a, hn, [](int i, float v) { uws_lraw[uws_idx(i)] = v; });
}
// The first hn <= CHAIN_HEAD addends one by one by a single thread of a workgroup of NT, out of LDS, starting from r0:
// the form of the two workgroup-level walkers (their timing is pinned to it).  Returns the sum in every thread.
#ifndef CHAIN_HEAD
#define CHAIN_HEAD 1024   // leading addends added one by one (<= PFXM_CHUNK)
#endif
template <int NT, class A>
__device__ __forceinline__ float chain_head_serial(const A& a, int hn, float r0) {
  __shared__ double head[CHAIN_HEAD];
  __shared__ float s_head_r;
  pfx_sync();
  for (int t = threadIdx.x; t < hn; t += NT) head[t] = a.load(t, true);
  pfx_sync();
  if (threadIdx.x == 0) {
    float run = r0;
    if (a.kind == CHAIN_SUM) {   // float addends: the float form (chain_add)
      for (int t = 0; t < hn; t++) run = chain_add(run, (float)head[t]);
    } else {
      for (int t = 0; t < hn; t++) run = chain_add(run, head[t]);
    }
    s_head_r = run;
  }
  pfx_sync();
  return s_head_r;
}

// ==== the multi-workgroup chains ==============================================================================================
//   1. *_sum_kernel      — per chunk of PFXM_CHUNK addends: the sum in double
//   2. *_summary_kernel  — per chunk: binade predicted from the double sum of everything before it; (D0, D1) in that
//                          binade, or "irregular" (NaN / inf / negative / addend above the binade)
//   3. *_walk_kernel     — ONE workgroup walks the chunks in order with the exact running sum: a chunk whose prediction
//                          holds (same binade, R + D_p stays below 2^24) is a single integer add; any other chunk (the
//                          ~log2(n) binade crossings, irregular addends, the head) is carried through on the spot
//   4. pfx_chunk_fill_kernel (running sum only) — per accepted chunk: the same scan again, now with the exact starting
//                          mantissa, writes every element's running sum / running maximum
// pfx_*: the running sum, NT x K = 256 x 16 in the grid kernels; chain_*: the statistics chains, 512 x 8.
// ws.wc (n above 32 768, else null): a wave holds one wave-chunk, whose sum goes to its record; the dual-slot counter is
// zeroed for the summaries of the launch behind this one.  FLAGS (the running sum): also ws.irr, does the chunk hold an
// addend that is negative or NaN — then the running sum is not its own running maximum, see pfx_grid_walk_kernel.
template <int NT, int K, bool FLAGS = false, class A>
__device__ __forceinline__ void chain_sum_body(const A& a, int64_t n, const ChainGridWs& ws) {
  static_assert(K == CHAIN_K && NT * K == PFXM_CHUNK, "one wave, one wave-chunk");
  __shared__ double shd[NT / 64];
  __shared__ int shi[FLAGS ? NT / 64 : 1];
  const long long lo = (long long)blockIdx.x * PFXM_CHUNK;
  const int cnt = (int)min((long long)PFXM_CHUNK, (long long)n - lo);
  typename A::value_t xv[K];
  a.load_items(lo, cnt, threadIdx.x * K, xv);
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < K; k++) acc += (double)xv[k];
  if constexpr (FLAGS) {   // (addends behind the chunk's end are zeros; published by the barrier of the sum)
    bool irr = false;
#pragma unroll
    for (int k = 0; k < K; k++) irr |= !(xv[k] >= 0);
    const bool any = __ballot(irr) != 0ull;
    if ((threadIdx.x & 63) == 0) shi[threadIdx.x >> 6] = any ? 1 : 0;
  }
  const double t = chain_wg_sum<NT>(acc, shd);
  if (threadIdx.x == 0) ws.ch[blockIdx.x].sum = t;
  if (ws.wc) {
    if constexpr (FLAGS) {
      if (threadIdx.x == 0) {
        int f = 0;
        for (int k = 0; k < NT / 64; k++) f |= shi[k];
        ws.irr[blockIdx.x] = f;
      }
    }
    if (threadIdx.x < NT / 64 && threadIdx.x * UWS_WC < cnt) ws.wc[blockIdx.x * (NT / 64) + threadIdx.x].sum = shd[threadIdx.x];
    if (blockIdx.x == 0 && threadIdx.x == 0) ws.ctl->slots = 0;
  }
}
template <int NT, int K, class A>
__device__ __forceinline__ void chain_summary_body(const A& a, int64_t n, PfxChunk* __restrict__ ch) {
  __shared__ double shd[NT / 64];
  __shared__ PfxPair shp[NT / 64];
  __shared__ int s_bad;
  const int c = blockIdx.x;
  const long long lo = (long long)c * PFXM_CHUNK;
  const int cnt = (int)min((long long)PFXM_CHUNK, (long long)n - lo);
  // predicted running sum before the chunk: the double sums of the chunks before it, in chunk order per thread
  double acc = 0.0;
  for (int j = threadIdx.x; j < c; j += NT) acc += ch[j].sum;
  if (threadIdx.x == 0) s_bad = 0;
  const double before = chain_wg_sum<NT>(acc, shd);
  const float r_pred = (float)before, r_end = (float)(before + ch[c].sum);
  const unsigned pb = __float_as_uint(r_pred), eb = __float_as_uint(r_end);
  const int re = (pb >> 23) & 0xFF;
  // a chunk that is predicted to start and end in one binade of a positive normal sum; everything else is irregular
  const bool plausible = (pb >> 31) == 0 && re >= PFXM_RE_MIN && re <= PFXM_RE_MAX && (int)((eb >> 23) & 0xFF) == re && (eb >> 31) == 0;
  if (!plausible) {   // uniform across the workgroup
    if (threadIdx.x == 0) { ch[c].re = -1; ch[c].d0 = 0u; ch[c].d1 = 0u; }
    return;
  }
  typename A::value_t xv[K];
  a.load_items(lo, cnt, threadIdx.x * K, xv);
  PfxPair mine = {0u, 0u};
  bool anybad = false;
#pragma unroll
  for (int k = 0; k < K; k++) {
    unsigned f; bool tie, bad;
    A::classify(xv[k], (unsigned)re, f, tie, bad);
    anybad |= bad;
    mine = pfx_compose(mine, pfx_element_pair(f, tie));
  }
  if (anybad) s_bad = 1;   // benign race: every writer stores 1; ordered by the barrier inside the scan
  PfxPair total;
  (void)pfx_pair_scan<NT>(mine, shp, total);
  if (threadIdx.x == 0) {
    const bool ok = s_bad == 0 && total.a0 < (1u << 24) && total.a1 < (1u << 24);
    ch[c].re = ok ? re : -1;
    ch[c].d0 = total.a0;
    ch[c].d1 = total.a1;
  }
}
// The walk over the chunk list [0, nch) by one workgroup of PFXW_THREADS: the headers staged PFXW_BLOCK at a time;
// a chunk whose prediction holds is one integer add, any other goes to slow(c), which carries r (and carry) through it.
// FILL: note r / carry in front of every accepted chunk and mark it, for pfx_chunk_fill_kernel.  (Chunk 0 starts at
// zero or behind a serial head and is never taken as predicted.)
#define PFXW_BLOCK 512   // chunk summaries / headers staged in LDS at a time
template <bool FILL, class CH, class SLOW>
__device__ __forceinline__ void chain_walk_chunks(CH* __restrict__ ch, int nch, float& r, float& carry, SLOW slow) {
  __shared__ int sm_re[PFXW_BLOCK];
  __shared__ unsigned sm_d0[PFXW_BLOCK], sm_d1[PFXW_BLOCK];
  __shared__ int sm_acc[FILL ? PFXW_BLOCK : 1];
  __shared__ float sm_r0[FILL ? PFXW_BLOCK : 1], sm_c0[FILL ? PFXW_BLOCK : 1];
  for (int cb = 0; cb < nch; cb += PFXW_BLOCK) {
    pfx_sync();
    for (int t = threadIdx.x; t < PFXW_BLOCK && cb + t < nch; t += PFXW_THREADS) {
      const PfxChunk x = ch[cb + t];
      sm_re[t] = x.re; sm_d0[t] = x.d0; sm_d1[t] = x.d1;
      if constexpr (FILL) sm_acc[t] = 0;
    }
    pfx_sync();
    const int ce = min(nch, cb + PFXW_BLOCK);
    for (int c = cb; c < ce; c++) {
      const unsigned rb = __float_as_uint(r);
      const int re = (int)(rb >> 23);                   // sign bit included: a negative sum never matches
      const unsigned R = (rb & 0x7FFFFFu) | 0x800000u;
      const unsigned D = (R & 1u) ? sm_d1[c - cb] : sm_d0[c - cb];
      // sm_re is in [PFXM_RE_MIN, PFXM_RE_MAX] or -1; the waves run through this loop unsynchronised and all store the same words
      if (c > 0 && sm_re[c - cb] == re && R + D < (1u << 24)) {
        if constexpr (FILL) { sm_r0[c - cb] = r; sm_c0[c - cb] = carry; sm_acc[c - cb] = 1; }
        r = chain_mant((unsigned)re, R + D);
        carry = fmaxf(carry, r);
      } else {
        slow(c);
      }
#ifdef TDR_PFX_TIMING   // diagnostic build: time stamp (100 MHz) after every chunk in the header's dead `sum` slot
      if constexpr (FILL)
        if (threadIdx.x == 0) *reinterpret_cast<long long*>(&ch[c].sum) = (long long)wall_clock64();
#endif
    }
    if constexpr (FILL) {
      pfx_sync();
      for (int t = threadIdx.x; t < PFXW_BLOCK && cb + t < nch; t += PFXW_THREADS) {   // for pfx_chunk_fill_kernel
        PfxChunk* o = ch + cb + t;
        o->r0 = sm_r0[t];
        o->carry0 = sm_c0[t];
        o->accepted = sm_acc[t];
      }
    }
  }
}

// ---- the running sum ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PFXW_THREADS) void pfx_chunk_sum_kernel(const float* __restrict__ w, int64_t n, ChainGridWs ws) {
  chain_sum_body<PFXW_THREADS, CHAIN_K, true>(ChainAddend<float, ChainGlobal, CHAIN_BOUND_22>{{w}, CHAIN_RUNSUM, 0.f}, n, ws);
}
__global__ __launch_bounds__(PFXM_THREADS) void pfx_chunk_summary_kernel(const float* __restrict__ w, int64_t n,
                                                                         PfxChunk* __restrict__ ch) {
  chain_summary_body<PFXM_THREADS, PFXM_K>(PfxRunSum{{w}, CHAIN_RUNSUM, 0.f}, n, ch);
}
// A chunk the walk cannot take as one integer add (it holds a binade crossing or an irregular weight, or was
// mispredicted), carried through in order by the walking workgroup
__device__ __forceinline__ void pfx_walk_chunk(const float* __restrict__ w, long long lo, int cnt,
                                               float* __restrict__ runmax, float* __restrict__ prefix_opt,
                                               float& r, float& carry, int head_len) {
  __shared__ PfxPair shp[PFXW_THREADS / 64];
  __shared__ ChainWgStop<float> stp;
  const PfxRunSum a{{w}, CHAIN_RUNSUM, 0.f};
  const int t0 = threadIdx.x * PFXW_K;
  float wv[PFXW_K];
  a.load_items(lo, cnt, t0, wv);
  const ChainWg<PFXW_THREADS, float> sc{shp, &stp};
  PfxGlobalSink sink{w, lo, runmax, prefix_opt, carry, head_len};
  r = chain_walk(a, wv, t0, 0, cnt, r, sc, sink);
}
__device__ __forceinline__ void pfx_walk_body(const float* __restrict__ w, int64_t n, PfxChunk* __restrict__ ch, int nch,
                                              float* __restrict__ runmax, float* __restrict__ prefix_opt, int head_len) {
  float r = 0.f, carry = -INFINITY;   // workgroup-uniform
  chain_walk_chunks<true>(ch, nch, r, carry, [&](int c) {
    const long long lo = (long long)c * PFXM_CHUNK;
    const int cnt = (int)min((long long)PFXM_CHUNK, (long long)n - lo);
    pfx_walk_chunk(w, lo, cnt, runmax, prefix_opt, r, carry, head_len);
  });
}
__global__ __launch_bounds__(PFXW_THREADS) void pfx_walk_kernel(const float* __restrict__ w, int64_t n,
                                                               PfxChunk* __restrict__ ch, int nch,
                                                               float* __restrict__ runmax,
                                                               float* __restrict__ prefix_opt, int head_len) {
  pfx_walk_body(w, n, ch, nch, runmax, prefix_opt, head_len);
}
// (on PFXM_THREADS threads; c: the chunk)
__device__ __forceinline__ void pfx_chunk_fill_body(const float* __restrict__ w, int64_t n, const PfxChunk* __restrict__ ch,
                                                    int c, float* __restrict__ runmax, float* __restrict__ prefix_opt) {
  __shared__ PfxPair shp[PFXM_THREADS / 64];
  const PfxChunk hdr = ch[c];
  if (!hdr.accepted) return;   // written by the walk
  const long long lo = (long long)c * PFXM_CHUNK;
  const int cnt = (int)min((long long)PFXM_CHUNK, (long long)n - lo);
  const PfxRunSum a{{w}, CHAIN_RUNSUM, 0.f};
  const int t0 = threadIdx.x * PFXM_K;
  float wv[PFXM_K];
  a.load_items(lo, cnt, t0, wv);
  const ChainWg<PFXM_THREADS, float> sc{shp, nullptr};
  unsigned st[PFXM_K];
  (void)chain_step<false, PfxRunSum>(wv, t0, 0, cnt, hdr.r0, sc, st);
  float val[PFXM_K];
#pragma unroll
  for (int k = 0; k < PFXM_K; k++) val[k] = chain_mant(__float_as_uint(hdr.r0) >> 23, st[k]);
  const float carry = hdr.carry0;
  if (t0 + PFXM_K <= cnt && ((lo & 3) == 0)) {
    float4* o = reinterpret_cast<float4*>(runmax + lo + t0);
#pragma unroll
    for (int k = 0; k < PFXM_K / 4; k++)
      o[k] = make_float4(fmaxf(carry, val[4 * k]), fmaxf(carry, val[4 * k + 1]), fmaxf(carry, val[4 * k + 2]),
                         fmaxf(carry, val[4 * k + 3]));
    if (prefix_opt) {
      float4* q = reinterpret_cast<float4*>(prefix_opt + lo + t0);
#pragma unroll
      for (int k = 0; k < PFXM_K / 4; k++) q[k] = make_float4(val[4 * k], val[4 * k + 1], val[4 * k + 2], val[4 * k + 3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < PFXM_K; k++)
      if (t0 + k < cnt) {
        runmax[lo + t0 + k] = fmaxf(carry, val[k]);
        if (prefix_opt) prefix_opt[lo + t0 + k] = val[k];
      }
  }
}
__global__ __launch_bounds__(PFXM_THREADS) void pfx_chunk_fill_kernel(const float* __restrict__ w, int64_t n,
                                                                      const PfxChunk* __restrict__ ch,
                                                                      float* __restrict__ runmax,
                                                                      float* __restrict__ prefix_opt) {
  pfx_chunk_fill_body(w, n, ch, blockIdx.x, runmax, prefix_opt);
}

// ---- totals of the statistics chains ---------------------------------------------------------------------------------------------
// ParticleFilter::update's statistics (CHAIN_SUM, CHAIN_BOTTOM) are serial chains too, and only their FINAL values are
// used.  Both are carried with the addend as a double made on the fly from (raw, mean).  Chunks as above: double sum ->
// predicted binade + parity summary -> one walking workgroup; no fill pass.
struct ChainSrc {
  const float* raw;    // raw weights
  const float* mean;   // device scalar (kind 1)
  int kind;            // CHAIN_SUM / CHAIN_BOTTOM
};
__device__ __forceinline__ ChainStat chain_stat(const ChainSrc& s) { return {{s.raw}, s.kind, s.kind ? *s.mean : 0.f}; }
__global__ __launch_bounds__(PFXW_THREADS) void chain_sum_kernel(ChainSrc s, int64_t n, ChainGridWs ws) {
  chain_sum_body<PFXW_THREADS, CHAIN_K>(chain_stat(s), n, ws);
}
__global__ __launch_bounds__(PFXW_THREADS) void chain_summary_kernel(ChainSrc s, int64_t n, PfxChunk* __restrict__ ch) {
  chain_summary_body<PFXW_THREADS, CHAIN_K>(chain_stat(s), n, ch);
}
// one chunk on the spot by the whole workgroup, from its element pos on: no outputs, the total only
template <class A>
__device__ __forceinline__ void chain_walk_chunk(const A& a, long long lo, int cnt, float& r, int pos) {
  __shared__ PfxPair shp[PFXW_THREADS / 64];
  __shared__ ChainWgStop<double> stp;
  const int t0 = threadIdx.x * CHAIN_K;
  double xv[CHAIN_K];
  a.load_items(lo, cnt, t0, xv);
  const ChainWg<PFXW_THREADS, double> sc{shp, &stp};
  ChainNoSink sink;
  r = chain_walk(a, xv, t0, pos, cnt, r, sc, sink);
}
__global__ __launch_bounds__(PFXW_THREADS) void chain_walk_kernel(ChainSrc s, int64_t n, const PfxChunk* __restrict__ ch,
                                                                 int nch, float* __restrict__ total_out) {
  const ChainStat a = chain_stat(s);
  // head: the sum of unnormalised weights crosses a binade every time it doubles — about ten times within the first
  // thousand addends — so those are added one by one
  const int hn = (int)min((long long)CHAIN_HEAD, (long long)n);
  float r = chain_head_serial<PFXW_THREADS>(a, hn, 0.f), carry = 0.f;   // workgroup-uniform
  chain_walk_chunks<false>(ch, nch, r, carry, [&](int c) {
    const long long lo = (long long)c * PFXM_CHUNK;
    chain_walk_chunk(a, lo, (int)min((long long)PFXM_CHUNK, (long long)n - lo), r, c == 0 ? hn : 0);
  });
  if (threadIdx.x == 0) *total_out = r;
}
// The workspace of a chain over n addends.  grid: with the wave-chunk records, control words and dual slots of the path
// above 32 768 addends behind the chunk headers.
#define CHAIN_GRID_MIN_N 32769
int64_t tdr_chain_workspace_bytes(int64_t n, bool grid) {
  if (n < 1) return 0;
  const int64_t nch = cdiv(n, (int64_t)PFXM_CHUNK), nwc = cdiv(n, (int64_t)UWS_WC);
  int64_t b = (int64_t)sizeof(PfxChunk) * nch;
  if (grid)
    b += (int64_t)sizeof(WcRec) * nwc + (nwc & 1) * 8 + ((nch * (int64_t)sizeof(int) + 15) & ~(int64_t)15) + (int64_t)sizeof(WcCtl) +
         (int64_t)UWG_DUAL_SLOTS * 64 * (int64_t)sizeof(uint4);
  return b;
}
static ChainGridWs chain_grid_ws(void* workspace, int64_t n, bool grid) {
  const int64_t nch = cdiv(n, (int64_t)PFXM_CHUNK), nwc = cdiv(n, (int64_t)UWS_WC);
  ChainGridWs ws{reinterpret_cast<PfxChunk*>(workspace), nullptr, nullptr, nullptr, nullptr};
  if (!grid) return ws;
  char* p = reinterpret_cast<char*>(workspace) + sizeof(PfxChunk) * nch;   // (32-byte headers: every part stays 16-byte aligned)
  ws.wc = reinterpret_cast<WcRec*>(p); p += sizeof(WcRec) * nwc + (nwc & 1) * 8;
  ws.irr = reinterpret_cast<int*>(p); p += (nch * sizeof(int) + 15) & ~(size_t)15;
  ws.ctl = reinterpret_cast<WcCtl*>(p); p += sizeof(WcCtl);
  ws.dual = reinterpret_cast<uint4*>(p);
  return ws;
}
// Does a chain over n addends take the wave-chunk path?  tdr_config_prefix_small(0) switches it off for the running sum
// AND the statistics chains: the 4096-chunk walk from the first addend on, the independent second evaluation the tests
// compare with.
bool tdr_chain_grid(int64_t n) { return tdr_cfg().pfx_small && n >= CHAIN_GRID_MIN_N; }
// summaries over the chip and the walking wave (chain_grid_summary_kernel / chain_grid_walk_kernel, below)
static void chain_grid_total(const ChainSrc& s, int64_t n, float* total_out, const ChainGridWs& ws, hipStream_t st);
// raw: [n] raw weights; kind 0: total = serial float sum of the non-NaN weights; kind 1: total = serial
// float-accumulated sum of pow(w - *mean_dev, 2) over the non-NaN weights below *mean_dev.  workspace:
// tdr_chain_workspace_bytes(n, grid); grid: the wave-chunk path (the caller asks tdr_chain_grid and has the room).
// total_out: one device float.  have_sums: the workspace holds the chunks' (and wave-chunks') double sums already.
int tdr_chain_total(const float* raw, const float* mean_dev, int kind, int64_t n, float* total_out, void* workspace,
                    bool have_sums, bool grid, hipStream_t st) {
  const int64_t nch64 = cdiv(n, (int64_t)PFXM_CHUNK);
  if (nch64 > (1 << 24)) return fail(TDR_ERR_ARG, "chain_total: n too large");
  if (grid && n < CHAIN_GRID_MIN_N) return fail(TDR_ERR_ARG, "chain_total: the wave-chunk path starts at 32 769 addends");
  const int nch = (int)nch64;
  const ChainGridWs ws = chain_grid_ws(workspace, n, grid);
  ChainSrc s{raw, mean_dev, kind};
  if (!have_sums) hipLaunchKernelGGL(chain_sum_kernel, dim3(nch), dim3(PFXW_THREADS), 0, st, s, n, ws);
  if (grid) {
    chain_grid_total(s, n, total_out, ws, st);
    return TDR_OK;
  }
  hipLaunchKernelGGL(chain_summary_kernel, dim3(nch), dim3(PFXW_THREADS), 0, st, s, n, ws.ch);
  hipLaunchKernelGGL(chain_walk_kernel, dim3(1), dim3(PFXW_THREADS), 0, st, s, n, (const PfxChunk*)ws.ch, nch, total_out);
  return TDR_OK;
}

// ---- the update's two counting passes above 32 768 weights, chunk by chunk -------------------------------------------------
// particle_filter.cpp:108-116 counts the valid weights and :118-125 those below the mean; each pass reads the whole array
// and is followed by a chain over the same array, so it leaves that chain's chunk sums behind (chain_sum_body: a chunk's
// additions in chain_sum_kernel's order).  Counts are integers: exact in any partition, so the grid is the chains' chunks.
template <int NT>
__device__ __forceinline__ int uw_wg_sum_int(int v, int* sh) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  pfx_sync();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  pfx_sync();
  int t = 0;
  for (int k = 0; k < NT / 64; k++) t += sh[k];
  return t;
}
// weights of chunk blockIdx.x that are not NaN and, with BELOW, below `mean`
template <bool BELOW>
__device__ __forceinline__ int uw_chunk_count(const float* __restrict__ raw, int64_t n, float mean, int* sh) {
  const long long lo = (long long)blockIdx.x * PFXM_CHUNK;
  const int cnt = (int)min((long long)PFXM_CHUNK, (long long)n - lo);
  const ChainAddend<float, ChainGlobal, CHAIN_BOUND_22> plain{{raw}, CHAIN_RUNSUM, 0.f};   // the weights as they are
  float v[CHAIN_K];
  const int t0 = threadIdx.x * CHAIN_K;
  plain.load_items(lo, cnt, t0, v);
  int c = 0;
#pragma unroll
  for (int k = 0; k < CHAIN_K; k++) c += (t0 + k < cnt && v[k] == v[k] && (!BELOW || v[k] < mean)) ? 1 : 0;
  return uw_wg_sum_int<PFXW_THREADS>(c, sh);
}
__global__ __launch_bounds__(PFXW_THREADS) void uw_chunk_pass1_kernel(const float* __restrict__ raw, int64_t n,
                                                                     ChainGridWs ws, int* __restrict__ cnt_valid) {
  __shared__ int shc[PFXW_THREADS / 64];
  const int c = uw_chunk_count<false>(raw, n, 0.f, shc);
  if (threadIdx.x == 0) cnt_valid[blockIdx.x] = c;
  chain_sum_body<PFXW_THREADS, CHAIN_K>(ChainStat{{raw}, CHAIN_SUM, 0.f}, n, ws);
}
__global__ __launch_bounds__(PFXW_THREADS) void uw_chunk_pass2_kernel(const float* __restrict__ raw, int64_t n,
                                                                     UwExact* __restrict__ ex,
                                                                     const int* __restrict__ cnt_valid,
                                                                     ChainGridWs ws, int* __restrict__ cnt_under) {
  __shared__ int shc[PFXW_THREADS / 64];
  __shared__ long long shv[PFXW_THREADS / 64];
  // the valid weights of all chunks (every workgroup: the same integer), then the mean (:117) from the exact `sum` chain
  long long nv = 0;
  for (int j = threadIdx.x; j < (int)gridDim.x; j += PFXW_THREADS) nv += cnt_valid[j];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) nv += __shfl_xor(nv, o, 64);
  if ((threadIdx.x & 63) == 0) shv[threadIdx.x >> 6] = nv;
  pfx_sync();
  nv = 0;
  for (int k = 0; k < PFXW_THREADS / 64; k++) nv += shv[k];
  const float mean = ex->sum / (float)nv;
  const int c = uw_chunk_count<true>(raw, n, mean, shc);
  if (threadIdx.x == 0) {
    cnt_under[blockIdx.x] = c;
    if (blockIdx.x == 0) ex->mean = mean;   // every workgroup computed the same value
  }
  chain_sum_body<PFXW_THREADS, CHAIN_K>(ChainStat{{raw}, CHAIN_BOTTOM, mean}, n, ws);
}
int tdr_uw_chunk_pass1(const float* raw, int64_t n, void* workspace, bool grid, int* cnt_valid, hipStream_t st) {
  hipLaunchKernelGGL(uw_chunk_pass1_kernel, dim3((unsigned)cdiv(n, (int64_t)PFXM_CHUNK)), dim3(PFXW_THREADS), 0, st, raw, n,
                     chain_grid_ws(workspace, n, grid), cnt_valid);
  return TDR_OK;
}
int tdr_uw_chunk_pass2(const float* raw, int64_t n, UwExact* ex, const int* cnt_valid, void* workspace, bool grid,
                       int* cnt_under, hipStream_t st) {
  hipLaunchKernelGGL(uw_chunk_pass2_kernel, dim3((unsigned)cdiv(n, (int64_t)PFXM_CHUNK)), dim3(PFXW_THREADS), 0, st, raw, n,
                     ex, cnt_valid, chain_grid_ws(workspace, n, grid), cnt_under);
  return TDR_OK;
}

// ==== ParticleFilter::update's statistics for small particle sets, in ONE launch ==========================================
// src/particle_filter.cpp:107-147 for n <= TDR_UW_SMALL_MAX_N — the reference's own operating point (20 000 particles,
// src/top_down_render.cpp:53).  One workgroup; the raw weights are staged into LDS once (n floats, at most 128 KB) and
// every pass — the two exact serial chains, the counts, fill / normalise / argmax — runs out of LDS; the weights are
// written to memory once, at the end.  Same results as the multi-workgroup path of tdr_filter.hip, bit for bit in
// `sum`, `mean`, `bottom_stddev` (tests/test_gpu_parity.py::test_update_weights_serial_chains_bit_exact).
//
// The chains on the whole workgroup (tdr_config_uw_waves(0)): head one by one, then chunk by chunk with
// chain_walk_chunk (no prediction pass: at most 8 chunks).  (One stretch over the whole array instead of chunks
// re-classifies every remaining addend at each binade crossing: 80 us against 48 at 20 000 weights.)
__device__ __forceinline__ float uws_chain_total(int kind, int n, float mean) {
  const UwsWgAdd a{{}, kind, mean};
  const int hn = min(CHAIN_HEAD, n);
  float r = chain_head_serial<PFXW_THREADS>(a, hn, 0.f);   // workgroup-uniform
  UW_STAMP(kind ? 5 : 2);
  const int nch = (n + PFXM_CHUNK - 1) / PFXM_CHUNK;
  for (int c = 0; c < nch; c++) {
    const int lo = c * PFXM_CHUNK;
    const int cnt = min((int)PFXM_CHUNK, n - lo);
    if (c == 0 && hn >= cnt) continue;
    chain_walk_chunk(a, lo, cnt, r, c == 0 ? hn : 0);
  }
  return r;
}
// ---- the same chains, wave by wave (default) --------------------------------------------------------------------------
// The weights are cut into wave-chunks of 512 (one wave, 8 consecutive addends a lane).  The pass before the chain (the
// count of valid weights / of weights below the mean) leaves the double sum of every wave-chunk's addends behind; from the
// sums before a chunk every wave predicts the binade the chain is in when it enters and leaves it.  Then, side by side:
//   * wave 0 adds the first wave-chunk one by one (the sum starts at zero and doubles every few addends);
//   * the other waves summarise their chunks: a chunk predicted to stay in one binade as its parity pair (D0, D1) there;
//     a chunk predicted to cross into the next binade as the parity pairs of every LANE (8 addends) in both binades.
// One barrier later wave 0 walks the chunk list with the exact running sum, with register-level moves only — no workgroup
// barrier inside the serial part: a one-binade chunk whose prediction holds is one integer add; in a crossing chunk a
// scan of the lane pairs of the first binade finds the lane the sum crosses in, that lane's 8 addends are really added,
// and a scan of the lane pairs of the second binade carries the sum to the chunk's end.  Whatever fits neither (a wrong
// prediction, irregular addends, two crossings in one chunk) is carried through element by element by uws_wave_walk.
// The bits are the serial chain's whatever was predicted, as in the multi-workgroup path.
#define UWS_THREADS 1024
#define UWS_DUAL_SLOTS 8        // crossing chunks summarised lane by lane (the sum doubles log2(n / 512) times behind the head)
#define UWS_DUAL_FLAG 0x100
struct UwsShared {
  double csum[64];                       // double sum of every wave-chunk's addends
  int code[64];                          // -1: carried through; binade; binade | UWS_DUAL_FLAG | slot << 16
  unsigned d0[64], d1[64];               // parity pair of a one-binade chunk
  uint4 dual[UWS_DUAL_SLOTS][64];        // crossing chunks: scans of the lane pairs in the binade entered (x, y) / the next (z, w)
  double shd[UWS_THREADS / 64];
  float total;
};
// wave-chunk [lo, lo + cnt) carried through by the calling wave from its element `pos` on, entered with the running sum r
// (wave-uniform): chain_walk on one wave, every chain with double addends as chain_walk_chunk has them
// (I: int for the LDS image, long long for an array in memory)
template <class A, class I>
__device__ __forceinline__ float uws_wave_walk(const A& a, I lo, int cnt, float r, int pos) {
  const auto ad = a.as_double();
  const int t0 = (threadIdx.x & 63) * CHAIN_K;
  double xv[CHAIN_K];
  ad.load_items(lo, cnt, t0, xv);
  ChainNoSink sink;
  return chain_walk(ad, xv, t0, pos, cnt, r, ChainWave<false>{}, sink);
}
// a chunk summarised lane by lane — the inclusive scans of the lanes' parity pairs in the binade predicted at its entry
// (x, y) and in the next one (z, w) — entered with r; pos: the element of the chunk the returned sum stands before (cnt: the
// chunk is done, else uws_wave_walk takes over there)
template <class A, class I>
__device__ __forceinline__ float uws_wave_dual(const A& a, I lo, int cnt, float r, const uint4* pq, int& pos) {
  const int lane = threadIdx.x & 63, t0 = lane * CHAIN_K;
  const unsigned rb = __float_as_uint(r), re = rb >> 23, R = (rb & 0x7FFFFFu) | 0x800000u;
  const uint4 v = pq[lane];
  const unsigned after = R + ((R & 1u) ? v.y : v.x);   // mantissa behind this lane's addends, while below 2^24
  const unsigned long long cross = __ballot(after >= (1u << 24));
  pos = cnt;
  if (cross == 0ull) return chain_mant(re, (unsigned)__builtin_amdgcn_readlane((int)after, 63));
  const int L = __ffsll((long long)cross) - 1;   // the lane the sum leaves the binade in: its addends are really added
  float rl = chain_mant(re, L > 0 ? (unsigned)__builtin_amdgcn_readlane((int)after, L - 1) : R);   // exact before lane L
  typename A::value_t x[CHAIN_K];
  a.load_items(lo, cnt, t0, x);
#pragma unroll
  for (int k = 0; k < CHAIN_K; k++) rl = chain_add(rl, x[k]);
  const float r2 = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(rl), L));
  const unsigned rb2 = __float_as_uint(r2), R2 = (rb2 & 0x7FFFFFu) | 0x800000u;
  const int next = (L + 1) * CHAIN_K;
  if (next >= cnt) return r2;
  pos = next;
  if ((rb2 >> 23) != re + 1u) return r2;
  // the lanes behind L in the next binade: scan(63) = scan(L) + rest((p + scan(L)) & 1) for an entering parity p, so a
  // scan(L) that is the same for both parities gives the rest for both
  const unsigned qL = (unsigned)__builtin_amdgcn_readlane((int)v.z, L);
  if (qL != (unsigned)__builtin_amdgcn_readlane((int)v.w, L)) return r2;
  const unsigned q63 = (unsigned)__builtin_amdgcn_readlane((int)(((R2 + qL) & 1u) ? v.w : v.z), 63);
  if (q63 >= PFXM_SAT || R2 + (q63 - qL) >= (1u << 24)) return r2;
  pos = cnt;
  return chain_mant(re + 1u, R2 + (q63 - qL));
}
// What is predicted for a wave-chunk from the double sums before and behind it: its binade when it stays in one, its
// binade and UWS_DUAL_FLAG when it crosses into the next one (the caller adds the slot), else -1.
__device__ __forceinline__ int uws_predict(double before, double after, bool& dualc) {
  const int re_b = (int)(__float_as_uint((float)before) >> 23), re_a = (int)(__float_as_uint((float)after) >> 23);   // sign included
  const bool inr = re_b >= PFXM_RE_MIN && re_a <= PFXM_RE_MAX;
  dualc = inr && re_a == re_b + 1;
  return (inr && re_a == re_b) ? re_b : dualc ? (re_b | UWS_DUAL_FLAG) : -1;
}
// One wave summarises wave-chunk [lo, lo + cnt) as `code` (>= 0) predicts: P (lane 63: the chunk's parity pair in the
// binade entered); with UWS_DUAL_FLAG the inclusive scans of the lanes' pairs in that binade and the next go to dual[lane].
// Returns whether every addend could be classified (else the chunk is carried through).
template <class A, class I>
__device__ __forceinline__ bool uws_wave_summary(const A& a, I lo, int cnt, int code, uint4* dual_out, PfxPair& P) {
  const int lane = threadIdx.x & 63, t0 = lane * CHAIN_K;
  PfxPair Q = {0u, 0u};
  bool anybad = false;
  const unsigned re = (unsigned)(code & 0xFF);
  const bool dual = (code & UWS_DUAL_FLAG) != 0;
  typename A::value_t x[CHAIN_K];   // (all eight reads in flight before the first use)
  a.load_items(lo, cnt, t0, x);
  // without a rounding tie in the chunk a lane's pair is (s, s), s the plain sum of its increments
  bool anytie = false;
  unsigned f; bool tie, bad;
#pragma unroll
  for (int k = 0; k < CHAIN_K; k++) {
    A::classify(x[k], re, f, tie, bad);
    anybad |= bad; anytie |= tie;
    P.a0 += f;   // (CHAIN_BOUND_22: no overflow in a lane, none below 2^31 in a wave)
  }
  if (dual) {
#pragma unroll
    for (int k = 0; k < CHAIN_K; k++) {
      A::classify(x[k], re + 1u, f, tie, bad);
      anybad |= bad; anytie |= tie;
      Q.a0 += f;
    }
  }
  if (__ballot(anytie) == 0ull) {
    P.a0 = P.a1 = uws_wave_scan_u(P.a0);
    if (dual) Q.a0 = Q.a1 = uws_wave_scan_u(Q.a0);
  } else {
    // (rare.  The binade is made opaque here so that this branch classifies again instead of keeping the f and tie
    // of all sixteen classifications above alive across the ballot: 16 VGPRs, and uw_small_kernel<true> has none to spare)
    unsigned re_t = re;
    asm volatile("" : "+s"(re_t));
    P = PfxPair{0u, 0u}; Q = PfxPair{0u, 0u};
#pragma unroll
    for (int k = 0; k < CHAIN_K; k++) {
      A::classify(x[k], re_t, f, tie, bad);
      P = pfx_compose(P, pfx_element_pair(f, tie));
    }
    P = pfx_pair_wave_scan(P);
    if (dual) {
#pragma unroll
      for (int k = 0; k < CHAIN_K; k++) {
        A::classify(x[k], re_t + 1u, f, tie, bad);
        Q = pfx_compose(Q, pfx_element_pair(f, tie));
      }
      Q = pfx_pair_wave_scan(Q);
    }
  }
  if (dual) dual_out[lane] = make_uint4(P.a0, P.a1, Q.a0, Q.a1);
  return __ballot(anybad) == 0ull;
}
// what a summarised chunk is noted as for the walk: its code, or -1 where it has to be carried through
__device__ __forceinline__ int uws_summary_code(int code, bool ok, const PfxPair& P) {
  return (ok && ((code & UWS_DUAL_FLAG) || (P.a0 < (1u << 24) && P.a1 < (1u << 24)))) ? code : -1;
}
// The walk.  Lane l holds the summary of wave-chunk base + l (v_code -1 where there is none, and for chunk 0, which the
// head takes); nl: lanes in use; n: addends in all.  The calling wave enters with the exact sum r in front of the first
// summarised chunk and returns the sum behind the last; kind CHAIN_RUNSUM: v_rin, lane l: the sum in front of chunk base + l.
// dual_of(code): the slot a dual chunk's scans were left in.
template <class A, class I, class DUAL>
__device__ __forceinline__ float uws_walk_summaries(const A& a, I n, int base, int nl, int v_code, unsigned v_d0,
                                                    unsigned v_d1, DUAL dual_of, float r, float& v_rin) {
  const int kind = a.kind;
  const int lane = threadIdx.x & 63;
  int c = base == 0 ? 1 : 0;
  while (c < nl) {
    const unsigned rb = __float_as_uint(r);
    const int re = (int)(rb >> 23);
    const unsigned R = (rb & 0x7FFFFFu) | 0x800000u;
    bool overflow = false;   // chunk c was predicted to stay in this binade and does not
    // the run of chunks from c on that were summarised in the binade the sum is in: one scan of their pairs (plain
    // sums when none of them holds a rounding tie) carries the sum through all of them
    const unsigned long long other = ~__ballot(lane < nl && v_code == re) & (~0ull << c);
    const int cend = other ? __ffsll((long long)other) - 1 : 64;   // the run is [c, cend)
    if (cend > c) {
      const bool in_run = lane >= c && lane < cend;
      unsigned after;   // lane l: mantissa behind chunk l, while below 2^24
      if (__ballot(in_run && v_d0 != v_d1) == 0ull) {
        after = R + uws_wave_scan_u(in_run ? v_d0 : 0u);
      } else {
        const PfxPair in = pfx_pair_wave_scan(in_run ? PfxPair{v_d0, v_d1} : PfxPair{0u, 0u});
        after = R + ((R & 1u) ? in.a1 : in.a0);
      }
      const unsigned long long cross = __ballot(in_run && after >= (1u << 24));
      const int c1 = cross ? __ffsll((long long)cross) - 1 : cend;   // chunks [c, c1) are taken
      if (kind == CHAIN_RUNSUM) {
        const unsigned prev = (unsigned)__builtin_amdgcn_update_dpp(0, (int)after, 0x138, 0xF, 0xF, false);   // wave_shr:1
        if (lane >= c && lane < c1) v_rin = lane == c ? r : chain_mant((unsigned)re, prev);
      }
      if (c1 > c) r = chain_mant((unsigned)re, (unsigned)__builtin_amdgcn_readlane((int)after, c1 - 1));
#ifdef TDR_UW_TIMELINE
      if (threadIdx.x == 0) g_uw_tl[12] += c1 - c;
#endif
      c = c1;
      if (c1 == cend) continue;
      overflow = true;
    }
    const I lo = (I)(base + c) * UWS_WC;
    const int cnt = (int)min((I)UWS_WC, n - lo);
    const int code = __builtin_amdgcn_readlane(v_code, c);
    if (kind == CHAIN_RUNSUM) v_rin = (lane == c) ? r : v_rin;
    int pos = 0;
    const int re_now = (int)(__float_as_uint(r) >> 23);
    if (!overflow && code >= 0 && re_now <= PFXM_RE_MAX && (code & 0x1FF) == (re_now | UWS_DUAL_FLAG)) {
      r = uws_wave_dual(a, lo, cnt, r, dual_of(code), pos);
      UW_COUNT(13);
    }
    if (pos < cnt) {
      UW_COUNT(14);
      r = uws_wave_walk(a, lo, cnt, r, pos);
    }
    c++;
  }
  return r;
}
// sh.csum holds the chunks' double sums and a barrier has passed since they were written; rin (kind 2): the running sum
// in front of every wave-chunk
template <class A>
__device__ __forceinline__ float uws_chain_total_waves(const A& a, int n, UwsShared& sh, float* rin = nullptr) {
  const int kind = a.kind;
  constexpr int NW = UWS_THREADS / 64;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwc = (n + UWS_WC - 1) / UWS_WC;   // <= 64
  float r = 0.f;
  if (wave == 0) {
    r = kind == CHAIN_RUNSUM ? chain_head_lanes<true>(a, min(UWS_WC, n)) : chain_head_lanes<false>(a, min(UWS_WC, n));
  } else {
    // the running double sum before / after each chunk -> what is predicted for it (lane c: chunk c)
    int my_code;
    {
      const double own = lane < nwc ? sh.csum[lane] : 0.0;
      const double after = uws_wave_scan_d(own), before = after - own;
      bool dualc;
      const int pred = uws_predict(before, after, dualc);
      const bool have = lane >= 1 && lane < nwc;
      const unsigned long long dm = __ballot(have && dualc);
      const int slot = __popcll(dm & ((1ull << lane) - 1ull));
      my_code = !have ? -1 : !dualc ? pred : slot < UWS_DUAL_SLOTS ? (pred | (slot << 16)) : -1;
    }
    for (int c = wave; c < nwc; c += NW - 1) {   // chunks 1 .. nwc - 1 over waves 1 .. NW - 1
      const int code = __builtin_amdgcn_readlane(my_code, c);
      const int lo = c * UWS_WC, cnt = min(UWS_WC, n - lo);
      PfxPair P = {0u, 0u};
      const bool ok = code >= 0 && uws_wave_summary(a, lo, cnt, code, sh.dual[(code >> 16) & (UWS_DUAL_SLOTS - 1)], P);
      if (lane == 63) {
        sh.code[c] = uws_summary_code(code, ok, P);
        sh.d0[c] = P.a0; sh.d1[c] = P.a1;
      }
    }
  }
  pfx_sync();
  UW_STAMP(kind ? 5 : 2);
  if (wave == 0) {   // the walk
    const bool have = lane >= 1 && lane < nwc;
    const int v_code = have ? sh.code[lane] : -1;
    const unsigned v_d0 = have ? sh.d0[lane] : 0u, v_d1 = have ? sh.d1[lane] : 0u;
    float v_rin = 0.f;   // lane c: the running sum in front of chunk c
    r = uws_walk_summaries(a, n, 0, nwc, v_code, v_d0, v_d1, [&](int code) { return sh.dual[code >> 16]; }, r, v_rin);
    if (kind == CHAIN_RUNSUM) rin[lane] = v_rin;
    if (lane == 0) sh.total = r;
  }
  pfx_sync();
  return sh.total;
}
template <int NT>
__device__ __forceinline__ double uws_sum_d(double v, double* sh) {   // block sum, fixed order: a pure function of the inputs
  v = uws_wave_scan_d(v);   // lane 63: the wave's sum
  pfx_sync();
  if ((threadIdx.x & 63) == 63) sh[threadIdx.x >> 6] = v;
  pfx_sync();
  double t = 0;
  for (int w = 0; w < NT / 64; w++) t += sh[w];
  return t;
}
// the one-workgroup weight statistics: the body of uw_small_kernel and of uw_small_batch_kernel
template <bool WAVES>
__device__ __forceinline__ void uw_small_body(const float* __restrict__ raw, const float* __restrict__ last_dist, int n,
                                              float* __restrict__ w, float* __restrict__ info) {
  extern __shared__ float uws_lraw[];   // [uws_idx(n)]: the raw weights, later the weights being normalised
  float* const lraw = uws_lraw;
  constexpr int nt = WAVES ? UWS_THREADS : PFXW_THREADS;
  __shared__ UwsShared ush;
  double* const shd = ush.shd;
  __shared__ float sh_best[nt / 64];
  __shared__ int sh_besti[nt / 64];
  const int tid = threadIdx.x;
#ifdef TDR_UW_TIMELINE
  if (tid == 0) { for (int k = 10; k < 16; k++) g_uw_tl[k] = 0; }
#endif
  UW_STAMP(0);
  float sum = 0.f, mean = 0.f, bsum = 0.f;
  long long num_valid = 0, num_under = 0;
  double valid_sum = 0.0;   // WAVES: the valid weights summed in double (the sum of the wave-chunks' sums)
  if constexpr (WAVES) {
    // chain 0: stage the weights and count the valid ones (:108-116), `sum`; chain 1: count the weights below the mean,
    // `bottom_stddev` (:118-126).  Either pass works wave-chunk by wave-chunk and leaves the chunks' double sums behind
    // for the chain's predictions.  (Unrolled: `kind` is a constant in each copy — 47 us against 53 with one copy.)
    const int lane = tid & 63, nwc = (n + UWS_WC - 1) / UWS_WC;
#pragma unroll
    for (int kind = 0; kind < 2; kind++) {
      int cnt = 0;
      for (int c = tid >> 6; c < nwc; c += nt / 64) {
        const int base = c * UWS_WC + lane;
        float v[CHAIN_K];
        if (kind == 0) {   // (eight loads of 64 consecutive weights in flight per wave)
#pragma unroll
          for (int m = 0; m < CHAIN_K; m++) v[m] = base + 64 * m < n ? raw[base + 64 * m] : __uint_as_float(0x7FC00000u);
#pragma unroll
          for (int m = 0; m < CHAIN_K; m++)
            if (base + 64 * m < n) lraw[uws_idx(base + 64 * m)] = v[m];
        } else {
#pragma unroll
          for (int m = 0; m < CHAIN_K; m++) {
            const float x = lraw[uws_idx(min(base + 64 * m, n - 1))];
            v[m] = base + 64 * m < n ? x : __uint_as_float(0x7FC00000u);
          }
        }
        double acc = 0;
#pragma unroll
        for (int m = 0; m < CHAIN_K; m++) {
          const bool take = kind == 0 ? v[m] == v[m] : (v[m] == v[m] && v[m] < mean);
          double x = (double)(kind == 0 ? v[m] : v[m] - mean);
          if (kind) x = x * x;
          cnt += take ? 1 : 0;
          acc += take ? x : 0.0;
        }
        acc = uws_wave_scan_d(acc);
        if (lane == 63) ush.csum[c] = acc;
      }
      const long long count = (long long)uws_sum_d<nt>((double)cnt, shd);   // (its barriers also publish the staged weights)
      if (kind == 0) valid_sum = uws_readlane_d(uws_wave_scan_d(lane < nwc ? ush.csum[lane] : 0.0), 63);
      UW_STAMP(kind ? 4 : 1);
      const float total = kind == 0 ? uws_chain_total_waves(UwsAddF{{}, CHAIN_SUM, 0.f}, n, ush)   // serial float chains, exact
                                    : uws_chain_total_waves(UwsAddD{{}, CHAIN_BOTTOM, mean}, n, ush);
      UW_STAMP(kind ? 6 : 3);
      if (kind == 0) {
        sum = total; num_valid = count;
        mean = sum / (float)num_valid;  // :117 (0/0 -> NaN like the reference)
      } else {
        bsum = total; num_under = count;
      }
    }
  } else {
    // stage (four loads in flight per thread), count the valid weights on the way (:108-116)
    double cnt = 0;
    int i = tid;
    for (; i + 3 * nt < n; i += 4 * nt) {
      const float v0 = raw[i], v1 = raw[i + nt], v2 = raw[i + 2 * nt], v3 = raw[i + 3 * nt];
      lraw[uws_idx(i)] = v0; lraw[uws_idx(i + nt)] = v1; lraw[uws_idx(i + 2 * nt)] = v2; lraw[uws_idx(i + 3 * nt)] = v3;
      cnt += (v0 == v0 ? 1.0 : 0.0) + (v1 == v1 ? 1.0 : 0.0) + (v2 == v2 ? 1.0 : 0.0) + (v3 == v3 ? 1.0 : 0.0);
    }
    for (; i < n; i += nt) {
      const float v = raw[i];
      lraw[uws_idx(i)] = v;
      cnt += (v == v) ? 1.0 : 0.0;
    }
    num_valid = (long long)uws_sum_d<nt>(cnt, shd);   // (its barriers also publish the staged weights)
    UW_STAMP(1);
    sum = uws_chain_total(CHAIN_SUM, n, 0.f);   // serial float chain, exact
    UW_STAMP(3);
    mean = sum / (float)num_valid;  // :117 (0/0 -> NaN like the reference)
    // :118-126  bottom_stddev (serial float chain with double addends, exact) and the count below the mean
    double cu = 0;
    for (int i = tid; i < n; i += nt) {
      const float v = lraw[uws_idx(i)];
      cu += (v == v && v < mean) ? 1.0 : 0.0;
    }
    num_under = (long long)uws_sum_d<nt>(cu, shd);
    UW_STAMP(4);
    bsum = uws_chain_total(CHAIN_BOTTOM, n, mean);
    UW_STAMP(6);
  }
  const float bottom = sqrtf(bsum / (float)num_under);
  const bool fallback = (sum == 0.f || num_under < 1);  // :129
  const float fill = mean - bottom;                      // :133
  const float fn = (float)n;
  float fs1;
  double s2 = 0;
  if constexpr (WAVES) {
    // :130-135 without a pass of its own: the filled weights sum to the valid ones plus `fill` for every NaN (all ones in
    // the fallback); the fill itself happens where the weight is read next.  The last travel distances are requested
    // sixteen per thread at a time, ahead of the divisions.  With no NaN there is nothing to fill and `fill` stays out of
    // the sum: it is inf or NaN when `bottom_stddev` or `sum` overflows, and 0 * inf would turn every weight into NaN
    // where the reference, which sums the weights as filled, keeps them finite (tests/test_uw_exact.py).
    const double fill_sum = num_valid == n ? 0.0 : (double)(n - num_valid) * (double)fill;
    fs1 = (float)(fallback ? (double)n : valid_sum + fill_sum);
    UW_STAMP(7);
    for (int i0 = tid; i0 < n; i0 += 16 * nt) {
      float ld[16];
#pragma unroll
      for (int j = 0; j < 16; j++) ld[j] = i0 + j * nt < n ? last_dist[i0 + j * nt] : 0.f;
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int i = i0 + j * nt;
        if (i < n) {   // :135, :138-141
          float v = lraw[uws_idx(i)];
          v = (fallback ? 1.f : (v != v ? fill : v)) / fs1;
          const float d = fminf(ld[j] * 5.f, 1.f);
          v = d * v + (1.f - d) / fn;
          lraw[uws_idx(i)] = v;
          s2 += (double)v;
        }
      }
    }
  } else {
    pfx_sync();                                            // every thread is done reading the raw weights
    double s1a = 0;
    for (int i = tid; i < n; i += nt) {
      float v = lraw[uws_idx(i)];
      v = fallback ? 1.f : (v != v ? fill : v);
      lraw[uws_idx(i)] = v;
      s1a += (double)v;
    }
    fs1 = (float)uws_sum_d<nt>(s1a, shd);
    UW_STAMP(7);
    auto one = [&](int i, float ld) {   // :135, :138-141
      float v = lraw[uws_idx(i)] / fs1;
      const float d = fminf(ld * 5.f, 1.f);
      v = d * v + (1.f - d) / fn;
      lraw[uws_idx(i)] = v;
      s2 += (double)v;
    };
    int i = tid;
    for (; i + 3 * nt < n; i += 4 * nt) {
      const float l0 = last_dist[i], l1 = last_dist[i + nt], l2 = last_dist[i + 2 * nt], l3 = last_dist[i + 3 * nt];
      one(i, l0); one(i + nt, l1); one(i + 2 * nt, l2); one(i + 3 * nt, l3);   // same order as one by one
    }
    for (; i < n; i += nt) one(i, last_dist[i]);
  }
  const float fs2 = (float)uws_sum_d<nt>(s2, shd);
  UW_STAMP(8);
  float best = -INFINITY;
  int besti = 0x7fffffff;
  for (int i = tid; i < n; i += nt) {  // :142, :145-147 (first maximum)
    const float v = lraw[uws_idx(i)] / fs2;
    w[i] = v;
    if (v > best || (v == best && i < besti)) { best = v; besti = i; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_down(best, o, 64);
    const int oi = __shfl_down(besti, o, 64);
    if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
  }
  pfx_sync();
  if ((tid & 63) == 0) { sh_best[tid >> 6] = best; sh_besti[tid >> 6] = besti; }
  pfx_sync();
  if (tid == 0) {
    for (int k = 1; k < nt / 64; k++)
      if (sh_best[k] > best || (sh_best[k] == best && sh_besti[k] < besti)) { best = sh_best[k]; besti = sh_besti[k]; }
    if (besti == 0x7fffffff) besti = 0;
    info[0] = __int_as_float(besti);
    info[1] = sum; info[2] = mean; info[3] = bottom; info[4] = fallback ? 1.f : 0.f;
    info[5] = (float)num_valid; info[6] = (float)num_under; info[7] = 0.f;
  }
  UW_STAMP(9);
}
template <bool WAVES>
__global__ __launch_bounds__(WAVES ? UWS_THREADS : PFXW_THREADS) void uw_small_kernel(const float* __restrict__ raw,
                                                                const float* __restrict__ last_dist, int n,
                                                                float* __restrict__ w, float* __restrict__ info) {
  uw_small_body<WAVES>(raw, last_dist, n, w, info);
}
// batched filters (tdr_batch_step): workgroup k = filter k of the table
template <bool WAVES>
__global__ __launch_bounds__(WAVES ? UWS_THREADS : PFXW_THREADS) void uw_small_batch_kernel(const TdrBatchEntry* __restrict__ tab) {
  const TdrBatchEntry& e = tab[blockIdx.x];
  uw_small_body<WAVES>(e.raw_w, e.last_dist, (int)e.n, e.w_out, e.info_out);
}
int tdr_uw_small(const float* raw, const float* last_dist, int64_t n, float* w, float* info, hipStream_t st) {
  if (n < 1 || n > 32768) return fail(TDR_ERR_ARG, "uw_small: n out of range");
  const size_t lds = ((size_t)n + (size_t)(n >> 5) + 1 + UWS_PAD) * sizeof(float);
  static bool attr_set[64] = {false};   // per device: the attribute lives with the device's copy of the code object
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
  if (dev >= 64 || !attr_set[dev]) {   // more than the default 64 KB of dynamic LDS
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(uw_small_kernel<false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, 133 * 1024) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(uw_small_kernel<true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, 133 * 1024) != hipSuccess)
      return fail(TDR_ERR_HIP, "uw_small: cannot raise the dynamic LDS limit");
    if (dev < 64) attr_set[dev] = true;
  }
  if (tdr_cfg().uw_waves)
    hipLaunchKernelGGL(uw_small_kernel<true>, dim3(1), dim3(UWS_THREADS), lds, st, raw, last_dist, (int)n, w, info);
  else
    hipLaunchKernelGGL(uw_small_kernel<false>, dim3(1), dim3(PFXW_THREADS), lds, st, raw, last_dist, (int)n, w, info);
  return TDR_OK;
}

// ---- the running sum of the resample for small particle sets, in ONE launch ------------------------------------------
// `running_sum += weights_[j]` (src/particle_filter.cpp:179) for n <= 32 768 with the machinery of the statistics chains:
// the weights staged in LDS, wave-chunks predicted and summarised side by side with the one-by-one head, one wave walking
// the chunk list with the exact sum (it notes the sum in front of every chunk), then every wave redoes its chunks from
// their exact starting sums and leaves each addend's running sum in place of the weight; a last pass takes the running
// maximum (the running sum itself when no weight is negative or NaN) and writes the outputs.
struct PfsShared {
  UwsShared u;
  float rin[64];    // running sum in front of every wave-chunk
  float cmax[64];   // largest running sum inside it (NaN skipped)
  int irregular;    // a negative or NaN weight exists: the running sum is not its own running maximum
};
// wave-chunk [lo, lo + cnt) from its exact starting sum r: the running sum behind each of the lane's addends (one scan, a
// second one behind a crossing)
template <class A, class I>
__device__ __forceinline__ void chain_wave_fill(const A& a, I lo, int cnt, float r, float (&pv)[CHAIN_K]) {
  const int t0 = (threadIdx.x & 63) * CHAIN_K;
  float x[CHAIN_K];
  a.load_items(lo, cnt, t0, x);
  ChainRegSink<CHAIN_K> sink;
#pragma unroll
  for (int k = 0; k < CHAIN_K; k++) sink.pv[k] = 0.f;
  (void)chain_walk(a, x, t0, 0, cnt, r, ChainWave<true>{}, sink);
#pragma unroll
  for (int k = 0; k < CHAIN_K; k++) pv[k] = sink.pv[k];
}
// ... out of the LDS image, in place of the weight
__device__ __forceinline__ void pfs_wave_fill(int lo, int cnt, float r) {
  extern __shared__ float uws_lraw[];
  const int t0 = (threadIdx.x & 63) * CHAIN_K;
  float pv[CHAIN_K];
  chain_wave_fill(UwsAddF{{}, CHAIN_RUNSUM, 0.f}, lo, cnt, r, pv);
#pragma unroll
  for (int k = 0; k < CHAIN_K; k++)
    if (t0 + k < cnt) uws_lraw[uws_idx(lo + t0 + k)] = pv[k];
}
// the one-workgroup running sum / running maximum: the body of pfx_small_kernel and of pfx_small_batch_kernel
__device__ __forceinline__ void pfx_small_body(const float* __restrict__ w, int n, float* __restrict__ runmax,
                                               float* __restrict__ prefix_opt) {
  extern __shared__ float uws_lraw[];
  float* const lraw = uws_lraw;
  __shared__ PfsShared sh;
  constexpr int nt = UWS_THREADS, NW = UWS_THREADS / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwc = (n + UWS_WC - 1) / UWS_WC;
  if (tid == 0) sh.irregular = 0;
  pfx_sync();
  // stage wave-chunk by wave-chunk; their double sums for the predictions
  bool irr = false;
  for (int c = wave; c < nwc; c += NW) {
    const int base = c * UWS_WC + lane;
    float v[CHAIN_K];
#pragma unroll
    for (int m = 0; m < CHAIN_K; m++) v[m] = base + 64 * m < n ? w[base + 64 * m] : 0.f;
    double acc = 0;
#pragma unroll
    for (int m = 0; m < CHAIN_K; m++) {
      if (base + 64 * m < n) lraw[uws_idx(base + 64 * m)] = v[m];
      irr |= !(v[m] >= 0.f);
      acc += (double)v[m];
    }
    acc = uws_wave_scan_d(acc);
    if (lane == 63) sh.u.csum[c] = acc;
  }
  if (__ballot(irr) != 0ull && lane == 0) atomicOr(&sh.irregular, 1);
  pfx_sync();
  (void)uws_chain_total_waves(UwsAddF{{}, CHAIN_RUNSUM, 0.f}, n, sh.u, sh.rin);   // (ends in a barrier)
  // every chunk again from its exact starting sum (the first one was filled by the head)
  for (int c = 1 + wave; c < nwc; c += NW) pfs_wave_fill(c * UWS_WC, min(UWS_WC, n - c * UWS_WC), sh.rin[c]);
  pfx_sync();
  if (sh.irregular == 0) {   // the running sum never falls: it is its own running maximum
    for (int i = tid; i < n; i += nt) {
      const float v = lraw[uws_idx(i)];
      runmax[i] = v;
      if (prefix_opt) prefix_opt[i] = v;
    }
    return;
  }
  const int t0 = lane * CHAIN_K;
  for (int c = wave; c < nwc; c += NW) {
    const int lo = c * UWS_WC, cnt = min(UWS_WC, n - lo);
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < CHAIN_K; k++) {
      const float v = lraw[uws_idx(lo + t0 + k)];
      if (t0 + k < cnt && v == v) m = fmaxf(m, v);
    }
    m = pfs_wave_scan_max(m);
    if (lane == 63) sh.cmax[c] = m;
  }
  pfx_sync();
  const float before = pfs_wave_scan_max(lane < nwc ? sh.cmax[lane] : -INFINITY);   // lane c: maximum up to chunk c's end
  for (int c = wave; c < nwc; c += NW) {
    const int lo = c * UWS_WC, cnt = min(UWS_WC, n - lo);
    const float carry = c > 0 ? __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(before), c - 1)) : -INFINITY;
    float pv[CHAIN_K], lm[CHAIN_K];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < CHAIN_K; k++) {
      pv[k] = lraw[uws_idx(lo + t0 + k)];
      if (t0 + k < cnt && pv[k] == pv[k]) m = fmaxf(m, pv[k]);
      lm[k] = m;
    }
    const float incl = pfs_wave_scan_max(m);
    float ex = __uint_as_float((unsigned)__builtin_amdgcn_update_dpp((int)0xFF800000u, (int)__float_as_uint(incl), 0x138, 0xF, 0xF, false));
    ex = fmaxf(ex, carry);
#pragma unroll
    for (int k = 0; k < CHAIN_K; k++)
      if (t0 + k < cnt) {
        runmax[lo + t0 + k] = fmaxf(lm[k], ex);
        if (prefix_opt) prefix_opt[lo + t0 + k] = pv[k];
      }
  }
}
__global__ __launch_bounds__(UWS_THREADS) void pfx_small_kernel(const float* __restrict__ w, int n,
                                                                float* __restrict__ runmax, float* __restrict__ prefix_opt) {
  pfx_small_body(w, n, runmax, prefix_opt);
}
// batched filters (tdr_batch_step): workgroup k = filter k of the table
__global__ __launch_bounds__(UWS_THREADS) void pfx_small_batch_kernel(const TdrBatchEntry* __restrict__ tab) {
  const TdrBatchEntry& e = tab[blockIdx.x];
  pfx_small_body(e.w_out, (int)e.n, e.runmax_out, nullptr);
}
#define TDR_PFX_SMALL_MAX_N 32768
static int pfx_small(const float* w, int64_t n, float* runmax, float* prefix_opt, hipStream_t st) {
  if (n < 1 || n > TDR_PFX_SMALL_MAX_N) return fail(TDR_ERR_ARG, "pfx_small: n out of range");
  const size_t lds = ((size_t)n + (size_t)(n >> 5) + 1 + UWS_PAD) * sizeof(float);
  static bool attr_set[64] = {false};   // per device: the attribute lives with the device's copy of the code object
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
  if (dev >= 64 || !attr_set[dev]) {   // more than the default 64 KB of dynamic LDS
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(pfx_small_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            133 * 1024) != hipSuccess)
      return fail(TDR_ERR_HIP, "pfx_small: cannot raise the dynamic LDS limit");
    if (dev < 64) attr_set[dev] = true;
  }
  hipLaunchKernelGGL(pfx_small_kernel, dim3(1), dim3(UWS_THREADS), lds, st, w, (int)n, runmax, prefix_opt);
  return TDR_OK;
}

// ==== the long chains at wave-chunk grain, over the chip (n > 32 768) =====================================================
// uws_chain_total_waves' algorithm with the addends in memory instead of an LDS image, and the chip instead of one CU:
//   1. the pass that reads every addend before the chain (uw_chunk_pass1 / _pass2, chain_sum_kernel, pfx_chunk_sum_kernel)
//      leaves the double sum of every wave-chunk in its WcRec beside the 4096-chunks' sums, and zeroes the slot counter;
//   2. chain_grid_summary_kernel, one wave per wave-chunk c >= 1: the double sum in front of the chunk (the 4096-chunk sums
//      before it, then the wave-chunks of its own 4096-chunk) -> uws_predict -> uws_wave_summary.  A chunk predicted to
//      cross draws a dual slot from the counter (UWG_DUAL_SLOTS; beyond them it is simply carried through);
//   3. chain_grid_walk_kernel / pfx_grid_walk_kernel, ONE wave: the first wave-chunk one by one (chain_head_lanes), then
//      uws_walk_summaries over the records, 64 at a time — the sum is all that passes from one 64 to the next, so a run of
//      chunks in one binade simply goes on.  The running sum notes the exact sum in front of every wave-chunk (WcRec::rin);
//   4. pfx_grid_fill_kernel (running sum only), one wave per wave-chunk: chain_wave_fill from rin, straight to the outputs.
// The running maximum is the running sum itself while no weight is negative or NaN.  An input that holds one (irr[], left
// by pass 1) takes the 4096-chunk path wholesale instead, inside the same three launches: the summary launch runs
// chain_summary_body on its first nch workgroups, the walk launch pfx_walk_body, the fill launch pfx_chunk_fill_body.
#define UWG_WAVES (PFXM_THREADS / 64)   // waves per workgroup of the summary and fill launches (whose workgroups may have to
                                        // run the 4096-chunk bodies: PFXM_THREADS)
using GridAddF = ChainAddend<float, ChainGlobal, CHAIN_BOUND_22>;   // CHAIN_SUM, CHAIN_RUNSUM
using GridAddD = ChainAddend<double, ChainGlobal, CHAIN_BOUND_22>;  // CHAIN_BOTTOM
// any flag among irr[0, nch)?  (wave-uniform)
__device__ __forceinline__ bool pfx_grid_irregular(const int* __restrict__ irr, int nch) {
  int f = 0;
  for (int j = threadIdx.x & 63; j < nch; j += 64) f |= irr[j];
  return __ballot(f != 0) != 0ull;
}
template <class A>
__device__ __forceinline__ void chain_grid_summary(const A& a, int64_t n, const ChainGridWs& ws) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long nwc = ((long long)n + UWS_WC - 1) / UWS_WC;
  const long long c = 1 + (long long)blockIdx.x * UWG_WAVES + wave;
  if (c >= nwc) return;
  constexpr int PER = PFXM_CHUNK / UWS_WC;   // wave-chunks per chunk
  const int cc = (int)(c / PER);
  double acc = 0.0;
  for (int j = lane; j < cc; j += 64) acc += ws.ch[j].sum;
  if (lane < (int)(c - (long long)cc * PER)) acc += ws.wc[(long long)cc * PER + lane].sum;
  const double before = uws_readlane_d(uws_wave_scan_d(acc), 63);
  bool dualc;
  int code = uws_predict(before, before + ws.wc[c].sum, dualc);
  if (dualc) {   // (wave-uniform)
    int slot = 0;
    if (lane == 0) slot = atomicAdd(&ws.ctl->slots, 1);
    slot = __builtin_amdgcn_readfirstlane(slot);
    code = slot < UWG_DUAL_SLOTS ? (code | (slot << 16)) : -1;
  }
  const long long lo = c * UWS_WC;
  const int cnt = (int)min((long long)UWS_WC, (long long)n - lo);
  PfxPair P = {0u, 0u};
  const bool ok = code >= 0 && uws_wave_summary(a, lo, cnt, code, ws.dual + (size_t)(code >> 16) * 64, P);
  if (lane == 63) {
    WcRec* o = ws.wc + c;
    o->code = uws_summary_code(code, ok, P);
    o->d0 = P.a0; o->d1 = P.a1;
  }
}
// the walking wave: returns the chain's total; kind CHAIN_RUNSUM: keep(i, v) takes the sums behind the first wave-chunk's addends
template <class A, class PUT>
__device__ __forceinline__ float chain_grid_walk(const A& a, int64_t n, const ChainGridWs& ws, PUT keep) {
  const int lane = threadIdx.x & 63;
  const long long nwc = ((long long)n + UWS_WC - 1) / UWS_WC;
  const int hn = (int)min((long long)UWS_WC, (long long)n);
  float r = a.kind == CHAIN_RUNSUM ? chain_head_lanes<true>(a, hn, keep) : chain_head_lanes<false>(a, hn, keep);
  for (long long base = 0; base < nwc; base += 64) {
    const int nl = (int)min(64ll, nwc - base);
    const bool have = lane < nl && base + lane >= 1;
    const WcRec* rec = ws.wc + base + lane;
    const int v_code = have ? rec->code : -1;
    const unsigned v_d0 = have ? rec->d0 : 0u, v_d1 = have ? rec->d1 : 0u;
    float v_rin = 0.f;
    r = uws_walk_summaries(a, (long long)n, (int)base, nl, v_code, v_d0, v_d1,
                           [&](int code) { return ws.dual + (size_t)(code >> 16) * 64; }, r, v_rin);
    if (a.kind == CHAIN_RUNSUM && have) ws.wc[base + lane].rin = v_rin;
  }
  return r;
}
template <int KIND>
__global__ __launch_bounds__(PFXM_THREADS) void chain_grid_summary_kernel(const float* __restrict__ raw,
                                                                          const float* __restrict__ mean_dev, int64_t n,
                                                                          ChainGridWs ws) {
  if constexpr (KIND == CHAIN_SUM) chain_grid_summary(GridAddF{{raw}, CHAIN_SUM, 0.f}, n, ws);
  else chain_grid_summary(GridAddD{{raw}, CHAIN_BOTTOM, *mean_dev}, n, ws);
}
template <int KIND>
__global__ __launch_bounds__(64) void chain_grid_walk_kernel(const float* __restrict__ raw, const float* __restrict__ mean_dev,
                                                             int64_t n, ChainGridWs ws, float* __restrict__ total_out) {
  float r;
  if constexpr (KIND == CHAIN_SUM) r = chain_grid_walk(GridAddF{{raw}, CHAIN_SUM, 0.f}, n, ws, [](int, float) {});
  else r = chain_grid_walk(GridAddD{{raw}, CHAIN_BOTTOM, *mean_dev}, n, ws, [](int, float) {});
  if (threadIdx.x == 0) *total_out = r;
}
static unsigned chain_grid_blocks(int64_t n) { return (unsigned)cdiv(cdiv(n, (int64_t)UWS_WC), (int64_t)UWG_WAVES); }
static void chain_grid_total(const ChainSrc& s, int64_t n, float* total_out, const ChainGridWs& ws, hipStream_t st) {
  const dim3 grid(chain_grid_blocks(n));   // (chunk 0 has no summary: the last workgroup may have a wave to spare)
  if (s.kind == CHAIN_SUM) {
    hipLaunchKernelGGL(chain_grid_summary_kernel<CHAIN_SUM>, grid, dim3(PFXM_THREADS), 0, st, s.raw, s.mean, n, ws);
    hipLaunchKernelGGL(chain_grid_walk_kernel<CHAIN_SUM>, dim3(1), dim3(64), 0, st, s.raw, s.mean, n, ws, total_out);
  } else {
    hipLaunchKernelGGL(chain_grid_summary_kernel<CHAIN_BOTTOM>, grid, dim3(PFXM_THREADS), 0, st, s.raw, s.mean, n, ws);
    hipLaunchKernelGGL(chain_grid_walk_kernel<CHAIN_BOTTOM>, dim3(1), dim3(64), 0, st, s.raw, s.mean, n, ws, total_out);
  }
}
// the running sum's three launches behind pfx_chunk_sum_kernel
__global__ __launch_bounds__(PFXM_THREADS) void pfx_grid_summary_kernel(const float* __restrict__ w, int64_t n, ChainGridWs ws,
                                                                        int nch) {
  if (pfx_grid_irregular(ws.irr, nch)) {   // (the same answer in every wave of the launch)
    if ((int)blockIdx.x < nch) chain_summary_body<PFXM_THREADS, PFXM_K>(PfxRunSum{{w}, CHAIN_RUNSUM, 0.f}, n, ws.ch);
    return;
  }
  chain_grid_summary(GridAddF{{w}, CHAIN_RUNSUM, 0.f}, n, ws);
}
__global__ __launch_bounds__(PFXW_THREADS) void pfx_grid_walk_kernel(const float* __restrict__ w, int64_t n, ChainGridWs ws,
                                                                    int nch, float* __restrict__ runmax,
                                                                    float* __restrict__ prefix_opt, int head_len) {
  const bool irregular = pfx_grid_irregular(ws.irr, nch);
  if (threadIdx.x == 0) ws.ctl->irregular = irregular ? 1 : 0;   // for the fill (the walk overwrites nothing it has read from)
  if (irregular) {
    pfx_walk_body(w, n, ws.ch, nch, runmax, prefix_opt, head_len);
    return;
  }
  if (threadIdx.x >= 64) return;   // one wave walks
  (void)chain_grid_walk(GridAddF{{w}, CHAIN_RUNSUM, 0.f}, n, ws, [&](int i, float v) {
    runmax[i] = v;
    if (prefix_opt) prefix_opt[i] = v;
  });
}
__global__ __launch_bounds__(PFXM_THREADS) void pfx_grid_fill_kernel(const float* __restrict__ w, int64_t n, ChainGridWs ws,
                                                                    int nch, float* __restrict__ runmax,
                                                                    float* __restrict__ prefix_opt) {
  if (ws.ctl->irregular) {
    if ((int)blockIdx.x < nch) pfx_chunk_fill_body(w, n, ws.ch, (int)blockIdx.x, runmax, prefix_opt);
    return;
  }
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), t0 = lane * CHAIN_K;
  const long long c = (long long)blockIdx.x * UWG_WAVES + wave;
  const long long lo = c * UWS_WC;
  if (c == 0 || lo >= (long long)n) return;   // (the first wave-chunk: written by the walking wave's head)
  const int cnt = (int)min((long long)UWS_WC, (long long)n - lo);
  float pv[CHAIN_K];
  chain_wave_fill(GridAddF{{w}, CHAIN_RUNSUM, 0.f}, lo, cnt, ws.wc[c].rin, pv);
  // no weight is negative or NaN: the running sum never falls and is its own running maximum
  if (t0 + CHAIN_K <= cnt) {
    float4* o = reinterpret_cast<float4*>(runmax + lo + t0);
    o[0] = make_float4(pv[0], pv[1], pv[2], pv[3]);
    o[1] = make_float4(pv[4], pv[5], pv[6], pv[7]);
    if (prefix_opt) {
      float4* q = reinterpret_cast<float4*>(prefix_opt + lo + t0);
      q[0] = make_float4(pv[0], pv[1], pv[2], pv[3]);
      q[1] = make_float4(pv[4], pv[5], pv[6], pv[7]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < CHAIN_K; k++)
      if (t0 + k < cnt) {
        runmax[lo + t0 + k] = pv[k];
        if (prefix_opt) prefix_opt[lo + t0 + k] = pv[k];
      }
  }
}
static_assert(CHAIN_K == 8, "pfx_grid_fill_kernel: two float4 per lane");

// Dispatch (tools/bench_prefix_modes.py on MI355X; us at n = 1k / 4k / 8k / 20k / 100k: one wave 16 / 43 / 84 / 208 /
// 1036, one workgroup 60 / 129 / 156 / 235 / 417, multi-workgroup 38 / 59 / 53 / 74 / 101):
#define TDR_PFX_MULTI_MIN_N 6144    // with a workspace: the multi-workgroup scan from here on, one wave below
#define TDR_PFX_EXACT_MIN_N 24576   // without a workspace: one workgroup from here on, one wave below
#define TDR_PFX_SMALL_MIN_N 256     // the one-launch kernel from here up to TDR_PFX_SMALL_MAX_N
// (the size does not depend on tdr_config_prefix_small: a workspace serves either path)
extern "C" int64_t tdr_prefix_workspace_bytes(int64_t n) { return tdr_chain_workspace_bytes(n, n >= CHAIN_GRID_MIN_N); }
static int prefix_multi(const float* w, int64_t n, float* runmax_out, float* prefix_out, void* workspace,
                        hipStream_t st) {
  const int64_t nch64 = cdiv(n, (int64_t)PFXM_CHUNK);
  if (nch64 > (1 << 24)) return fail(TDR_ERR_ARG, "prefix: n too large");
  const int nch = (int)nch64;
  const int head_len = tdr_cfg().pfx_head;
  const bool grid = tdr_chain_grid(n);
  const ChainGridWs ws = chain_grid_ws(workspace, n, grid);
  hipLaunchKernelGGL(pfx_chunk_sum_kernel, dim3(nch), dim3(PFXW_THREADS), 0, st, w, n, ws);
  if (grid) {
    const dim3 blocks(std::max(chain_grid_blocks(n), (unsigned)nch));   // (nch: the 4096-chunk bodies of an irregular input)
    hipLaunchKernelGGL(pfx_grid_summary_kernel, blocks, dim3(PFXM_THREADS), 0, st, w, n, ws, nch);
    hipLaunchKernelGGL(pfx_grid_walk_kernel, dim3(1), dim3(PFXW_THREADS), 0, st, w, n, ws, nch, runmax_out, prefix_out,
                       head_len);
    hipLaunchKernelGGL(pfx_grid_fill_kernel, blocks, dim3(PFXM_THREADS), 0, st, w, n, ws, nch, runmax_out, prefix_out);
    return TDR_OK;
  }
  hipLaunchKernelGGL(pfx_chunk_summary_kernel, dim3(nch), dim3(PFXM_THREADS), 0, st, w, n, ws.ch);
  hipLaunchKernelGGL(pfx_walk_kernel, dim3(1), dim3(PFXW_THREADS), 0, st, w, n, ws.ch, nch, runmax_out, prefix_out, head_len);
  hipLaunchKernelGGL(pfx_chunk_fill_kernel, dim3(nch), dim3(PFXM_THREADS), 0, st, w, n, (const PfxChunk*)ws.ch,
                     runmax_out, prefix_out);
  return TDR_OK;
}
extern "C" int tdr_k_prefix(const float* w, int64_t n, float* runmax_out, void* workspace, void* stream) {
  if (!w || !runmax_out || n < 1) return fail(TDR_ERR_ARG, "prefix: bad arguments");
  if (tdr_cfg().pfx_small && n >= TDR_PFX_SMALL_MIN_N && n <= TDR_PFX_SMALL_MAX_N) {
    const int rc = pfx_small(w, n, runmax_out, nullptr, (hipStream_t)stream);
    if (rc) return rc;
  } else if (workspace && n >= TDR_PFX_MULTI_MIN_N) {
    const int rc = prefix_multi(w, n, runmax_out, nullptr, workspace, (hipStream_t)stream);
    if (rc) return rc;
  } else if (n < TDR_PFX_EXACT_MIN_N)
    hipLaunchKernelGGL(prefix_serial_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, w, n, runmax_out);
  else
    hipLaunchKernelGGL(prefix_exact_kernel, dim3(1), dim3(PFX_THREADS), 0, (hipStream_t)stream, w, n, runmax_out,
                       (float*)nullptr);
  LAUNCH_CHECK("prefix");
  return TDR_OK;
}
// Test / diagnostic entry: mode 0 = serial kernel, 1 = exact parallel kernel in one workgroup, 2 = the multi-workgroup
// scan (needs a workspace of tdr_prefix_workspace_bytes(n)), 3 = the one-launch kernel for n <= 32 768; prefix_out
// (optional, modes 1 to 3) receives the raw running sums.
extern "C" int tdr_k_prefix_mode(const float* w, int64_t n, int mode, float* runmax_out, float* prefix_out,
                                 void* workspace, void* stream) {
  if (!w || !runmax_out || n < 1) return fail(TDR_ERR_ARG, "prefix_mode: bad arguments");
  if (mode == 2 && !workspace) return fail(TDR_ERR_ARG, "prefix_mode: mode 2 needs a workspace");
  if (mode == 3) {
    const int rc = pfx_small(w, n, runmax_out, prefix_out, (hipStream_t)stream);
    if (rc) return rc;
  } else if (mode == 0)
    hipLaunchKernelGGL(prefix_serial_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, w, n, runmax_out);
  else if (mode == 2) {
    const int rc = prefix_multi(w, n, runmax_out, prefix_out, workspace, (hipStream_t)stream);
    if (rc) return rc;
  } else
    hipLaunchKernelGGL(prefix_exact_kernel, dim3(1), dim3(PFX_THREADS), 0, (hipStream_t)stream, w, n, runmax_out,
                       prefix_out);
  LAUNCH_CHECK("prefix_mode");
  return TDR_OK;
}

// ---- batched filters (tdr_batch_step, tdr_batch.h): the statistics and the running sum of k filters of at most 32 768
// particles, one workgroup per filter running uw_small_kernel's / pfx_small_kernel's body on that filter's arrays
static int batch_lds_attr(const void* fn) {
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 133 * 1024) == hipSuccess ? TDR_OK
         : fail(TDR_ERR_HIP, "batch: cannot raise the dynamic LDS limit");
}
int tdr_batch_update_weights(const TdrBatchEntry* tab, int k, int64_t n_max, hipStream_t st) {
  if (!tab || k < 1 || n_max < 1 || n_max > 32768) return fail(TDR_ERR_ARG, "batch_update_weights: bad arguments");
  const size_t lds = ((size_t)n_max + (size_t)(n_max >> 5) + 1 + UWS_PAD) * sizeof(float);
  if (tdr_cfg().uw_waves) {
    if (int rc = batch_lds_attr(reinterpret_cast<const void*>(uw_small_batch_kernel<true>))) return rc;
    hipLaunchKernelGGL(uw_small_batch_kernel<true>, dim3((unsigned)k), dim3(UWS_THREADS), lds, st, tab);
  } else {
    if (int rc = batch_lds_attr(reinterpret_cast<const void*>(uw_small_batch_kernel<false>))) return rc;
    hipLaunchKernelGGL(uw_small_batch_kernel<false>, dim3((unsigned)k), dim3(PFXW_THREADS), lds, st, tab);
  }
  LAUNCH_CHECK("batch_update_weights");
  return TDR_OK;
}
int tdr_batch_prefix(const TdrBatchEntry* tab, int k, int64_t n_max, hipStream_t st) {
  if (!tab || k < 1 || n_max < 1 || n_max > TDR_PFX_SMALL_MAX_N) return fail(TDR_ERR_ARG, "batch_prefix: bad arguments");
  const size_t lds = ((size_t)n_max + (size_t)(n_max >> 5) + 1 + UWS_PAD) * sizeof(float);
  if (int rc = batch_lds_attr(reinterpret_cast<const void*>(pfx_small_batch_kernel))) return rc;
  hipLaunchKernelGGL(pfx_small_batch_kernel, dim3((unsigned)k), dim3(UWS_THREADS), lds, st, tab);
  LAUNCH_CHECK("batch_prefix");
  return TDR_OK;
}
