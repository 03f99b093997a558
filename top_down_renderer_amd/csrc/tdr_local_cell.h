// tdr_local_cell.h — the map cell one window sample reads: the addressing of getLocalMap as a device function of its own
// (polar: src/top_down_map_polar.cpp:28-31; Cartesian: src/top_down_map.cpp:429-437 via samplePts :367-389).
// local_map_kernel (tdr_score.hip) gathers from that cell, fuse_votes_kernel (tdr_fuse.hip) scatters into it: one source,
// so the vote of a scan bin lands in exactly the cell the window pairs with it, bit for bit.
#ifndef TDR_LOCAL_CELL_H_
#define TDR_LOCAL_CELL_H_
#include "tdr_common.h"
#include "tdr_score_dev.h"   // round_half_away_clamped
#include "tdr_sincosf.h"

__device__ __forceinline__ float linspaced_dev(int i, int size1, float low, float high, float step) {
  // Eigen LinSpaced<float>, |high| == |low| here, so never the flipped branch of linspaced_op_impl
  return (i == size1) ? high : (low + (float)i * step);
}

// One window of one pose.  Polar: rows x cols = the table's nb x nr, scale_or_rot = the particle's scale.  Cartesian:
// scale_or_rot = the rotation.  cx, cy in the units tdr_k_local_map_* takes; resolution = the map's.
struct LocalCellArgs {
  int map_rows, map_cols;
  float resolution;
  const float* tab;     // polar: [P][2]
  int rows, cols;       // window shape (polar: nb x nr)
  float cx, cy, scale_or_rot, res;
  int libm_fma;
};
// Sample k = i + rows * j of the window: its cell (ri, ci), clamped to [-1, map_rows] x [-1, map_cols]; returns whether the
// cell lies on the map.
template <bool POLAR>
__device__ __forceinline__ bool local_map_cell(const LocalCellArgs& a, int64_t k, int& ri, int& ci) {
  const float off0 = a.cy / a.resolution, off1 = a.cx / a.resolution;
  float p0, p1;
  if constexpr (POLAR) {
    p0 = (a.tab[2 * k] * a.scale_or_rot) * a.res + off0;      // top_down_map_polar.cpp:28-30
    p1 = (a.tab[2 * k + 1] * a.scale_or_rot) * a.res + off1;
  } else {
    const int i = (int)(k % a.rows), j = (int)(k / a.rows);
    const float resq = a.res / a.resolution;                    // top_down_map.cpp:434
    const float c = tdr_libm::cosf_v(a.scale_or_rot, a.libm_fma), s = tdr_libm::sinf_v(a.scale_or_rot, a.libm_fma);   // :381-385
    const float lo_r = (float)((double)(-resq * (float)(a.rows - 1)) / 2.), hi_r = (float)((double)(resq * (float)(a.rows - 1)) / 2.);
    const float lo_c = (float)((double)(-resq * (float)(a.cols - 1)) / 2.), hi_c = (float)((double)(resq * (float)(a.cols - 1)) / 2.);
    const float step_r = a.rows == 1 ? 0.f : (hi_r - lo_r) / (float)(a.rows - 1);
    const float step_c = a.cols == 1 ? 0.f : (hi_c - lo_c) / (float)(a.cols - 1);
    const float yi = linspaced_dev(i, a.rows == 1 ? 1 : a.rows - 1, lo_r, hi_r, step_r);
    const float xj = linspaced_dev(j, a.cols == 1 ? 1 : a.cols - 1, lo_c, hi_c, step_c);
    p0 = (c * yi + (-s) * xj) + off0;                           // samplePts :383-388
    p1 = (s * yi + c * xj) + off1;
  }
  p0 = __builtin_amdgcn_fmed3f(p0, -1.f, (float)a.map_rows);
  p1 = __builtin_amdgcn_fmed3f(p1, -1.f, (float)a.map_cols);
  ri = round_half_away_clamped(p0);
  ci = round_half_away_clamped(p1);
  return (unsigned)ri < (unsigned)a.map_rows && (unsigned)ci < (unsigned)a.map_cols;
}
#endif  // TDR_LOCAL_CELL_H_
