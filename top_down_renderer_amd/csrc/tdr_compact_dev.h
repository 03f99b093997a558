// tdr_compact_dev.h — what the recovery kernels and the pose-grid search share (tdr_recover.hip, tdr_recover_sensor.hip,
// tdr_grid.hip); not installed.
//   The ordered list of the indices of [0, n) that satisfy a predicate, in three launches:
//     cmp_count_kernel   a workgroup owns a run of whole 256-index tiles; ballot + bit count per wave, the run's count to the
//                        workspace;
//     cmp_scan_kernel    ONE workgroup: the exclusive running sum of the runs' counts (at most CMP_MAX_BLOCKS) and the total;
//     cmp_write_kernel   the predicate again; a listed index's place = its run's offset + the tiles before it in the run +
//                        the waves before it + the listed lanes below it.  The order is the index order whatever the grid.
//   Pred is a struct passed by value: __device__ bool operator()(int64_t i) const, false for i outside [0, n).
//   tdr_wave_pick: the pick rule of sensor resetting over C weights by one wave.
#ifndef TDR_COMPACT_DEV_H_
#define TDR_COMPACT_DEV_H_
#include "tdr_common.h"

namespace tdrcmp {
constexpr int CMP_BLOCK = 256;
constexpr int CMP_WAVES = CMP_BLOCK / 64;
constexpr int CMP_MAX_BLOCKS = 2048;   // grid.x of the list kernels; a workgroup owns cdiv(tiles, grid.x) tiles in a row

template <class Pred>
__global__ __launch_bounds__(CMP_BLOCK) void cmp_count_kernel(Pred pred, int64_t tiles_per_block, int64_t* __restrict__ block_count) {
  __shared__ int sh[CMP_WAVES];
  const int64_t t0 = (int64_t)blockIdx.x * tiles_per_block;
  int cnt = 0;   // wave-uniform
  for (int64_t t = t0; t < t0 + tiles_per_block; t++) cnt += __popcll(__ballot(pred(t * CMP_BLOCK + threadIdx.x)));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t s = 0;
    for (int w = 0; w < CMP_WAVES; w++) s += sh[w];
    block_count[blockIdx.x] = s;
  }
}

// counts [nb <= CMP_MAX_BLOCKS] -> exclusive offsets in place; *total = their sum
static __global__ __launch_bounds__(CMP_BLOCK) void cmp_scan_kernel(int64_t* __restrict__ v, int nb, int64_t* __restrict__ total) {
  constexpr int PER = CMP_MAX_BLOCKS / CMP_BLOCK;
  __shared__ int64_t part[CMP_BLOCK];
  int64_t x[PER], sum = 0;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int b = threadIdx.x * PER + k;
    x[k] = b < nb ? v[b] : 0;
    sum += x[k];
  }
  part[threadIdx.x] = sum;
  __syncthreads();
  int64_t before = 0;
  for (int t = 0; t < (int)threadIdx.x; t++) before += part[t];
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int b = threadIdx.x * PER + k;
    if (b < nb) v[b] = before;
    before += x[k];
  }
  if (threadIdx.x == CMP_BLOCK - 1) *total = before;
}

// list holds at least as many words as the predicate has true indices: a place is below that number
template <class Pred, class Out>
__global__ __launch_bounds__(CMP_BLOCK) void cmp_write_kernel(Pred pred, int64_t tiles_per_block, const int64_t* __restrict__ block_off,
                                                              Out* __restrict__ list) {
  __shared__ int sh[2][CMP_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t0 = (int64_t)blockIdx.x * tiles_per_block;
  int64_t base = block_off[blockIdx.x];
  for (int64_t t = t0; t < t0 + tiles_per_block; t++) {
    const int64_t p = t * CMP_BLOCK + threadIdx.x;
    const bool on = pred(p);
    const uint64_t m = __ballot(on);
    int* cnt = sh[(t - t0) & 1];   // two rows: one barrier a tile
    if (lane == 0) cnt[wave] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < CMP_WAVES; w++) {
      off += w < wave ? cnt[w] : 0;
      tot += cnt[w];
    }
    if (on) list[base + off + __popcll(m & (((uint64_t)1 << lane) - 1))] = (Out)p;
    base += tot;
  }
}

// the grid of a list over [0, n): max_blocks <= 0 or beyond the bound: the bound
static inline int cmp_blocks(int64_t n, int max_blocks) {
  const int mb = max_blocks >= 1 && max_blocks < CMP_MAX_BLOCKS ? max_blocks : CMP_MAX_BLOCKS;
  return (int)std::min<int64_t>(cdiv(std::max<int64_t>(n, 1), CMP_BLOCK), mb);
}
static inline size_t cmp_workspace_bytes(int64_t n) { return (size_t)cmp_blocks(n, 0) * sizeof(int64_t); }

// The three launches for n >= 1.  workspace: cmp_workspace_bytes(n); *count_dev (DEVICE): the list's length.
template <class Pred, class Out>
static int cmp_list(const char* who, Pred pred, int64_t n, Out* list_out, int64_t* count_dev, void* workspace, int max_blocks,
                    hipStream_t s) {
  const int nb = cmp_blocks(n, max_blocks);
  const int64_t tiles_per_block = cdiv(cdiv(n, CMP_BLOCK), nb);
  int64_t* blocks = reinterpret_cast<int64_t*>(workspace);
  hipLaunchKernelGGL(cmp_count_kernel<Pred>, dim3((unsigned)nb), dim3(CMP_BLOCK), 0, s, pred, tiles_per_block, blocks);
  if (hipGetLastError() != hipSuccess) return fail(TDR_ERR_HIP, "launch %s_count", who);
  hipLaunchKernelGGL(cmp_scan_kernel, dim3(1), dim3(CMP_BLOCK), 0, s, blocks, nb, count_dev);
  if (hipGetLastError() != hipSuccess) return fail(TDR_ERR_HIP, "launch %s_scan", who);
  hipLaunchKernelGGL((cmp_write_kernel<Pred, Out>), dim3((unsigned)nb), dim3(CMP_BLOCK), 0, s, pred, tiles_per_block,
                     (const int64_t*)blocks, list_out);
  if (hipGetLastError() != hipSuccess) return fail(TDR_ERR_HIP, "launch %s_write", who);
  return TDR_OK;
}

// (key, j) over the C >= 1 weights w[0 .. C): key_j = w_j, or -1 where w_j is NaN; a larger key wins, among equal keys the
// smaller j.  Every lane keeps the best of its stride in ascending j, the wave then reduces on (key, -j) with a butterfly
// of shuffles: the order on the pairs is total, so every lane returns the same j whatever the reduction order.  A lane
// without a candidate holds a key below every candidate's; lane 0 holds candidate 0, so the result is < C.
__device__ __forceinline__ int tdr_wave_pick(const float* __restrict__ w, int C, int lane) {
  float best = -2.f;
  int bj = 0x7fffffff;
  for (int j = lane; j < C; j += 64) {
    const float v = w[j];
    const float key = v != v ? -1.f : v;
    if (key > best) {   // ascending j within a lane: the first of equal keys stays
      best = key;
      bj = j;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ok = __shfl_xor(best, off, 64);
    const int oj = __shfl_xor(bj, off, 64);
    if (ok > best || (ok == best && oj < bj)) {
      best = ok;
      bj = oj;
    }
  }
  return bj;
}
}  // namespace tdrcmp
#endif  // TDR_COMPACT_DEV_H_
