// tdr_eig.cpp — the corner of the handle layer that needs no device: its error report (failh) and the .eig files of the
// reference's map cache (top_down_map.h:29-50), which tdr_map_load_cache / tdr_map_save_cache read and write.
// No HIP header: this file also builds on its own for a host test (tests/cpp/eig_roundtrip.cpp).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "tdr_internal.h"

namespace tdrh {

int failh(int code, const char* fmt, ...) {
  char buf[400];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return tdr_set_error(code, buf);
}

// .eig files of the reference's map cache (top_down_map.h:29-50)
std::string cache_dir_or_default(const char* cache_dir) {
  if (cache_dir && *cache_dir) return cache_dir;
  const char* home = getenv("HOME");
  return std::string(home ? home : ".") + "/.ros/xview_cache";
}
template <class T>
int read_eig(const std::string& path, std::vector<T>& out, int64_t& rows, int64_t& cols) {
  FILE* fh = fopen(path.c_str(), "rb");
  if (!fh) return failh(TDR_ERR_ARG, "map cache: cannot open %s", path.c_str());
  int64_t hdr[2] = {0, 0};
  bool ok = fread(hdr, sizeof(int64_t), 2, fh) == 2 && hdr[0] > 0 && hdr[1] > 0 && hdr[0] < (1 << 24) && hdr[1] < (1 << 24);
  if (ok) {   // the payload the header promises must be what the file holds (a damaged header must not size the buffer)
    const long at = ftell(fh);
    ok = at >= 0 && fseek(fh, 0, SEEK_END) == 0;
    const long end = ok ? ftell(fh) : -1;
    ok = ok && end >= at && (uint64_t)(end - at) == (uint64_t)hdr[0] * (uint64_t)hdr[1] * sizeof(T) &&
         fseek(fh, at, SEEK_SET) == 0;
  }
  if (ok) {
    out.resize((size_t)hdr[0] * hdr[1]);
    ok = fread(out.data(), sizeof(T), out.size(), fh) == out.size() && fgetc(fh) == EOF;
  }
  fclose(fh);
  if (!ok) return failh(TDR_ERR_ARG, "map cache: %s is not a well-formed .eig file of this scalar type", path.c_str());
  rows = hdr[0];
  cols = hdr[1];
  return TDR_OK;
}
template <class T>
int write_eig(const std::string& path, const T* data, int64_t rows, int64_t cols) {
  FILE* fh = fopen(path.c_str(), "wb");
  if (!fh) return failh(TDR_ERR_ARG, "map cache: cannot write %s", path.c_str());
  const int64_t hdr[2] = {rows, cols};
  const bool ok = fwrite(hdr, sizeof(int64_t), 2, fh) == 2 && fwrite(data, sizeof(T), (size_t)rows * cols, fh) == (size_t)rows * cols;
  fclose(fh);
  return ok ? TDR_OK : failh(TDR_ERR_ARG, "map cache: short write to %s", path.c_str());
}
template int read_eig<float>(const std::string&, std::vector<float>&, int64_t&, int64_t&);
template int read_eig<uint8_t>(const std::string&, std::vector<uint8_t>&, int64_t&, int64_t&);
template int write_eig<float>(const std::string&, const float*, int64_t, int64_t);
template int write_eig<uint8_t>(const std::string&, const uint8_t*, int64_t, int64_t);

}  // namespace tdrh
