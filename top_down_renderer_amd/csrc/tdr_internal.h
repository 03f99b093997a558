// tdr_internal.h — prototypes of the functions one translation unit of libtdr_hip.so defines for another that no
// per-subsystem header (tdr_common.h, tdr_batch.h, tdr_score_*.h, tdr_gmm_dev.h) declares.  Declarations only, host
// only; every defining and every calling file includes it (the .hip files through tdr_common.h), so the compiler checks
// each definition against the one prototype.  The tdr_cmap_* sizes and tdr_set_error are in include/tdr.h.
#ifndef TDR_INTERNAL_H_
#define TDR_INTERNAL_H_
#include <cstdint>
#include <string>
#include <vector>

#include "tdr.h"

typedef struct ihipStream_t* hipStream_t;   // as <hip/hip_runtime.h> has it: this header needs no HIP header

// tdr_score.hip: whether tdr_k_score_polar_ctx scores a filter of these shapes with the float kernel (not the integer form)
bool tdr_score_polar_float_form(const tdr_map_desc* map, int nb, int nr, int64_t n, int64_t n_total);

// tdr_png.cpp
int tdr_png_read_gray8(const char* path, std::vector<uint8_t>& px, int& w, int& h);
int tdr_png_write_gray8(const char* path, const uint8_t* px, int w, int h);
int tdr_png_read_bgr8(const char* path, std::vector<uint8_t>& bgr, int& w, int& h);
// tdr_poly.hip
int tdr_poly_grid(int width, int height, float resolution, int* rows, int* cols);
int tdr_poly_fill(const float* verts, const int64_t* offs, const int32_t* cls, int64_t n_poly, int width, int height,
                  float resolution, int ncls, const uint32_t* excl_above, uint8_t* planes_cm, uint8_t* raster,
                  hipStream_t s);
// tdr_grid.hip: the ranges of a tdr_grid_spec (include/tdr.h, "pose-grid search"); TDR_ERR_ARG with `who` in the message
int tdr_grid_spec_check(const tdr_grid_spec* spec, const char* who);
// tdr_svg.cpp
int tdr_svg_parse_internal(const char* path, float* w, float* h, std::vector<uint32_t>& keys, std::vector<int64_t>& offs,
                           std::vector<float>& verts);

namespace tdrh {
// tdr_eig.cpp: the handle layer's error report (printf-style, through tdr_set_error) and the .eig files of the map cache
int failh(int code, const char* fmt, ...);
std::string cache_dir_or_default(const char* cache_dir);
template <class T>
int read_eig(const std::string& path, std::vector<T>& out, int64_t& rows, int64_t& cols);   // T: float, uint8_t
template <class T>
int write_eig(const std::string& path, const T* data, int64_t rows, int64_t cols);
}  // namespace tdrh
#endif  // TDR_INTERNAL_H_
