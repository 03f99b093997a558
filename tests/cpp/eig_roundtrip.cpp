// The .eig files of the map cache (csrc/tdr_eig.cpp, top_down_map.h:29-50) on the host alone: this program links against
// tdr_eig.cpp and nothing else of the library, and is meant to be built with -fsanitize=address,undefined.
//   * a float matrix and a uint8_t matrix written by write_eig come back from read_eig bit for bit;
//   * a file that is not a well-formed .eig file of the scalar type asked for is refused with an error code and a
//     message, and the caller's vector and shape stay as they were.
// argv[1]: a directory to write into.  Prints "ok"; a failed check prints its line and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tdr.h"
#include "tdr_internal.h"

static int g_code = 0;
static std::string g_msg;
extern "C" int tdr_set_error(int code, const char* msg) {   // the library's lives in tdr_core.hip, behind the HIP runtime
  g_code = code;
  g_msg = msg ? msg : "";
  return code;
}

#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("eig_roundtrip.cpp:%d: %s\n", __LINE__, #cond);   \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

static void put(const std::string& path, const int64_t* hdr, size_t payload_bytes) {
  FILE* fh = std::fopen(path.c_str(), "wb");
  CHECK(fh);
  if (hdr) CHECK(std::fwrite(hdr, sizeof(int64_t), 2, fh) == 2);
  const std::vector<unsigned char> pay(payload_bytes, 0x5a);
  if (payload_bytes) CHECK(std::fwrite(pay.data(), 1, payload_bytes, fh) == payload_bytes);
  CHECK(std::fclose(fh) == 0);
}

// read_eig<T> must refuse `path`: an error code, a message that names the file, and nothing of the caller's changed
template <class T>
static void refused(const std::string& path) {
  const std::vector<T> before(3, (T)7);
  std::vector<T> out(before);
  int64_t rows = -5, cols = -6;
  g_code = 0;
  g_msg.clear();
  const int rc = tdrh::read_eig(path, out, rows, cols);
  CHECK(rc == TDR_ERR_ARG && g_code == rc);
  CHECK(g_msg.find(path) != std::string::npos);
  CHECK(out == before && rows == -5 && cols == -6);
}

int main(int argc, char** argv) {
  CHECK(argc == 2);
  const std::string d = std::string(argv[1]) + "/";

  // round trips, odd shapes; the float matrix holds a NaN, an infinity, a denormal and both zeros: bits, not values
  const int64_t R = 7, C = 5;
  std::vector<float> f((size_t)R * C);
  for (size_t i = 0; i < f.size(); i++) f[i] = 0.37f * (float)i - 3.f;
  const uint32_t special[5] = {0x7fc00001u, 0xff800000u, 0x00000001u, 0x80000000u, 0x00000000u};
  std::memcpy(f.data(), special, sizeof(special));
  std::vector<uint8_t> u((size_t)R * C);
  for (size_t i = 0; i < u.size(); i++) u[i] = (uint8_t)(i * 37 + 11);
  CHECK(tdrh::write_eig(d + "f.eig", f.data(), R, C) == TDR_OK);
  CHECK(tdrh::write_eig(d + "u.eig", u.data(), C, R) == TDR_OK);
  {
    std::vector<float> got;
    int64_t rows = 0, cols = 0;
    CHECK(tdrh::read_eig(d + "f.eig", got, rows, cols) == TDR_OK && rows == R && cols == C);
    CHECK(got.size() == f.size() && std::memcmp(got.data(), f.data(), f.size() * sizeof(float)) == 0);
    std::vector<uint8_t> gu(100, 1);   // (a vector that held something else before)
    CHECK(tdrh::read_eig(d + "u.eig", gu, rows, cols) == TDR_OK && rows == C && cols == R);
    CHECK(gu == u);
  }

  // refused files
  const int64_t h_ok[2] = {R, C}, h_zero[2] = {0, C}, h_neg[2] = {-1, C}, h_huge[2] = {(int64_t)1 << 24, (int64_t)1 << 24};
  const size_t bytes = (size_t)R * C * sizeof(float);
  put(d + "empty.eig", nullptr, 0);
  put(d + "header_only.eig", h_ok, 0);
  put(d + "short.eig", h_ok, bytes - 1);
  put(d + "long.eig", h_ok, bytes + 1);
  put(d + "zero_rows.eig", h_zero, bytes);
  put(d + "neg_rows.eig", h_neg, bytes);
  put(d + "huge.eig", h_huge, bytes);
  for (const char* name : {"empty.eig", "header_only.eig", "short.eig", "long.eig", "zero_rows.eig", "neg_rows.eig", "huge.eig"})
    refused<float>(d + name);
  refused<uint8_t>(d + "f.eig");   // a float file read as uint8_t
  // ... and the same damage at the other scalar size (the payload check is in units of sizeof(T))
  put(d + "short_u8.eig", h_ok, (size_t)R * C - 1);
  put(d + "long_u8.eig", h_ok, (size_t)R * C + 1);
  refused<uint8_t>(d + "short_u8.eig");
  refused<uint8_t>(d + "long_u8.eig");
  refused<float>(d + "u.eig");
  refused<float>(d + "no_such_file.eig");

  // the cache directory: the caller's, or the reference's default under $HOME
  CHECK(tdrh::cache_dir_or_default("/some/where") == "/some/where");
  CHECK(setenv("HOME", "/home/robot", 1) == 0);
  CHECK(tdrh::cache_dir_or_default(nullptr) == "/home/robot/.ros/xview_cache");
  CHECK(tdrh::cache_dir_or_default("") == "/home/robot/.ros/xview_cache");
  std::printf("ok\n");
  return 0;
}
