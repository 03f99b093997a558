// tdr_png.cpp — the 8-bit greyscale PNG files of the reference's raster cache (TopDownMap::saveRasterizedMaps /
// loadRasterizedMaps, src/top_down_map.cpp:197-224: cv::imwrite / cv::imread(IMREAD_GRAYSCALE) of CV_8UC1 images), read and
// written over zlib.  Reader: colour type 0, bit depth 8, non-interlaced — what cv::imwrite produces for these images —
// every filter type; chunk CRCs checked; any other PNG is refused by name.  Writer: filter 0, one IDAT.
// Below them, the colour reader of the static colour map (tdr_png_read_bgr8): any PNG, as cv::imread reads it.
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <exception>
#include <vector>

#include "tdr_common.h"

static uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
static void put32(uint8_t* p, uint32_t v) { p[0] = v >> 24; p[1] = v >> 16; p[2] = v >> 8; p[3] = v; }
static const uint8_t PNG_SIG[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};

int tdr_png_read_gray8(const char* path, std::vector<uint8_t>& px, int& w, int& h) {
  FILE* fh = fopen(path, "rb");
  if (!fh) return fail(TDR_ERR_ARG, "png: cannot open %s", path);
  std::vector<uint8_t> file;
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), fh)) > 0) file.insert(file.end(), buf, buf + got);
  fclose(fh);
  if (file.size() < 8 + 25 || memcmp(file.data(), PNG_SIG, 8) != 0) return fail(TDR_ERR_ARG, "png: %s is not a PNG file", path);
  size_t at = 8;
  bool have_hdr = false, done = false;
  std::vector<uint8_t> idat;
  w = h = 0;
  while (!done) {
    if (at + 12 > file.size()) return fail(TDR_ERR_ARG, "png: %s is truncated", path);
    const uint32_t len = be32(&file[at]);
    if (len > 0x7FFFFFFFu || at + 12 + (size_t)len > file.size()) return fail(TDR_ERR_ARG, "png: %s is truncated", path);
    const uint8_t* type = &file[at + 4];
    const uint8_t* data = &file[at + 8];
    if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), type, 4 + len) != be32(data + len))
      return fail(TDR_ERR_ARG, "png: %s has a chunk with a wrong CRC", path);
    if (!memcmp(type, "IHDR", 4)) {
      if (len != 13) return fail(TDR_ERR_ARG, "png: %s has a malformed header", path);
      const uint32_t ww = be32(data), hh = be32(data + 4);
      if (ww < 1 || hh < 1 || ww > (1u << 24) || hh > (1u << 24)) return fail(TDR_ERR_ARG, "png: %s has an unusable size", path);
      if (data[8] != 8 || data[9] != 0 || data[10] != 0 || data[11] != 0 || data[12] != 0)
        return fail(TDR_ERR_ARG, "png: %s is not an 8-bit greyscale, non-interlaced image (bit depth %d, colour type %d, "
                    "interlace %d)", path, data[8], data[9], data[12]);
      w = (int)ww; h = (int)hh;
      have_hdr = true;
    } else if (!memcmp(type, "IDAT", 4)) {
      if (!have_hdr) return fail(TDR_ERR_ARG, "png: %s has image data before its header", path);
      idat.insert(idat.end(), data, data + len);
    } else if (!memcmp(type, "IEND", 4)) {
      done = true;
    } else if (!(type[0] & 0x20)) {   // an unknown CRITICAL chunk (PLTE has no place in a greyscale image either)
      return fail(TDR_ERR_ARG, "png: %s holds a critical chunk this reader does not know", path);
    }
    at += 12 + (size_t)len;
  }
  if (!have_hdr || idat.empty()) return fail(TDR_ERR_ARG, "png: %s has no image data", path);
  const size_t stride = (size_t)w + 1;
  // deflate expands at most ~1032 : 1: a header that announces more pixels than the image data can hold is refused before
  // anything of that size is allocated (a damaged or hostile file must not be able to ask for 2^48 bytes)
  if ((uint64_t)stride * (uint64_t)h > (uint64_t)idat.size() * 1032u + 64u)
    return fail(TDR_ERR_ARG, "png: %s announces %d x %d pixels but holds %zu bytes of image data", path, w, h, idat.size());
  std::vector<uint8_t> raw(stride * (size_t)h);
  uLongf out_len = (uLongf)raw.size();
  if (uncompress(raw.data(), &out_len, idat.data(), (uLong)idat.size()) != Z_OK || out_len != raw.size())
    return fail(TDR_ERR_ARG, "png: the image data of %s does not inflate to %d x %d bytes", path, w, h);
  px.assign((size_t)w * h, 0);
  for (int y = 0; y < h; y++) {   // unfilter, one byte per pixel
    const uint8_t* in = &raw[stride * y];
    uint8_t* out = &px[(size_t)w * y];
    const uint8_t* up = y ? &px[(size_t)w * (y - 1)] : nullptr;
    const int ft = in[0];
    if (ft > 4) return fail(TDR_ERR_ARG, "png: %s uses filter type %d", path, ft);
    for (int x = 0; x < w; x++) {
      const int a = x ? out[x - 1] : 0, b = up ? up[x] : 0, c = (x && up) ? up[x - 1] : 0;
      int pred = 0;
      if (ft == 1) pred = a;
      else if (ft == 2) pred = b;
      else if (ft == 3) pred = (a + b) >> 1;
      else if (ft == 4) {
        const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
      }
      out[x] = (uint8_t)(in[x + 1] + pred);
    }
  }
  return TDR_OK;
}

int tdr_png_write_gray8(const char* path, const uint8_t* px, int w, int h) {
  if (!px || w < 1 || h < 1) return fail(TDR_ERR_ARG, "png: nothing to write");
  const size_t stride = (size_t)w + 1;
  std::vector<uint8_t> raw(stride * (size_t)h);
  for (int y = 0; y < h; y++) {
    raw[stride * y] = 0;   // filter type 0
    memcpy(&raw[stride * y + 1], px + (size_t)w * y, (size_t)w);
  }
  uLongf zlen = compressBound((uLong)raw.size());
  std::vector<uint8_t> z(zlen);
  if (compress2(z.data(), &zlen, raw.data(), (uLong)raw.size(), 6) != Z_OK) return fail(TDR_ERR_ARG, "png: deflate failed");
  FILE* fh = fopen(path, "wb");
  if (!fh) return fail(TDR_ERR_ARG, "png: cannot write %s", path);
  auto chunk = [&](const char* type, const uint8_t* data, uint32_t len) {
    std::vector<uint8_t> c(12 + (size_t)len);
    put32(&c[0], len);
    memcpy(&c[4], type, 4);
    if (len) memcpy(&c[8], data, len);
    put32(&c[8 + len], (uint32_t)crc32(crc32(0L, Z_NULL, 0), &c[4], 4 + len));
    return fwrite(c.data(), 1, c.size(), fh) == c.size();
  };
  uint8_t hdr[13];
  put32(hdr, (uint32_t)w);
  put32(hdr + 4, (uint32_t)h);
  hdr[8] = 8; hdr[9] = 0; hdr[10] = 0; hdr[11] = 0; hdr[12] = 0;
  const bool ok = fwrite(PNG_SIG, 1, 8, fh) == 8 && chunk("IHDR", hdr, 13) && chunk("IDAT", z.data(), (uint32_t)zlen) &&
                  chunk("IEND", nullptr, 0);
  fclose(fh);
  return ok ? TDR_OK : fail(TDR_ERR_ARG, "png: short write to %s", path);
}

// C-ABI face of the codec (host only, no device): px_out holds capacity bytes; *w / *h are set even when the image does not fit
extern "C" int tdr_png_read_gray8_host(const char* path, uint8_t* px_out, int64_t capacity, int* w, int* h) {
  if (!path || !w || !h) return fail(TDR_ERR_ARG, "png: null pointer");
  try {   // (no exception crosses the C ABI: an allocation failure is an error code)
    std::vector<uint8_t> px;
    if (int rc = tdr_png_read_gray8(path, px, *w, *h)) return rc;
    if (!px_out || capacity < (int64_t)px.size()) return fail(TDR_ERR_ARG, "png: %s needs %zu bytes", path, px.size());
    memcpy(px_out, px.data(), px.size());
    return TDR_OK;
  } catch (const std::exception& e) {
    return fail(TDR_ERR_NOMEM, "png: %s: %s", path, e.what());
  }
}
extern "C" int tdr_png_write_gray8_host(const char* path, const uint8_t* px, int w, int h) {
  if (!path) return fail(TDR_ERR_ARG, "png: null pointer");
  try {
    return tdr_png_write_gray8(path, px, w, h);
  } catch (const std::exception& e) {
    return fail(TDR_ERR_NOMEM, "png: %s: %s", path, e.what());
  }
}

// ---- colour images: the BGR8 image cv::imread(path) (IMREAD_COLOR) gives for a PNG ------------------------------------
// The TopDownMap constructor's colour-map branch (src/top_down_map.cpp:32-42) reads the map with cv::imread, which drives
// libpng.  Every colour type (0, 2, 3, 4, 6), every legal bit depth, both interlace methods and all five filter types are
// read, IDAT may be split over any number of chunks, chunk CRCs are checked.  The conversion follows OpenCV's libpng
// set-up, rule by rule:
//   - palette images are expanded to RGB (png_set_palette_to_rgb); tRNS is ignored (its alpha is stripped again);
//   - greyscale below 8 bits is scaled to 8 bits (png_set_expand_gray_1_2_4_to_8: v * 255 / (2^d - 1)) and copied into
//     all three channels (png_set_gray_to_rgb);
//   - alpha is dropped (png_set_strip_alpha), not composited;
//   - 16-bit samples keep their high byte (png_set_strip_16);
//   - Adam7 files decode to the image the non-interlaced file of the same pixels gives;
//   - no gamma or colour-space conversion: gAMA, sRGB, iCCP, cHRM and text chunks have no effect;
//   - output byte order B, G, R (png_set_bgr), row 0 = the top of the image.
// Not verified here, from memory of libpng 1.6: it zero-fills a 256-entry palette, so a palette index outside the PLTE
// chunk decodes to black.  Known difference: cv::imread may rotate an image by its EXIF orientation; eXIf is ignored here.
// A PLTE chunk in a greyscale image is ignored (libpng: a benign error, a warning on read); in colour types 2 / 6 it is a
// suggested palette and ignored too.  Compressed data past the end of the image is ignored (libpng: a benign error).
namespace {
struct PngHdr {
  int w = 0, h = 0, depth = 0, ctype = 0, interlace = 0;
  int channels() const { return ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : 4; }
  int bits_pp() const { return channels() * depth; }
  size_t row_bytes(int width) const { return ((size_t)width * bits_pp() + 7) / 8; }
};
bool legal_depth(int ctype, int depth) {
  switch (ctype) {
    case 0: return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
    case 3: return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    case 2: case 4: case 6: return depth == 8 || depth == 16;
    default: return false;
  }
}
// the seven Adam7 passes: first column / row and steps; a non-interlaced image is one pass (0, 0, 1, 1)
const int ADAM7[7][4] = {{0, 0, 8, 8}, {4, 0, 8, 8}, {0, 4, 4, 8}, {2, 0, 4, 4}, {0, 2, 2, 4}, {1, 0, 2, 2}, {0, 1, 1, 2}};
int pass_count(int interlace) { return interlace ? 7 : 1; }
void pass_shape(const PngHdr& hd, int p, int& pw, int& ph, int& x0, int& y0, int& dx, int& dy) {
  if (!hd.interlace) { x0 = y0 = 0; dx = dy = 1; }
  else { x0 = ADAM7[p][0]; y0 = ADAM7[p][1]; dx = ADAM7[p][2]; dy = ADAM7[p][3]; }
  pw = hd.w > x0 ? (hd.w - x0 + dx - 1) / dx : 0;
  ph = hd.h > y0 ? (hd.h - y0 + dy - 1) / dy : 0;
}
// the 8-bit value of sample i of an unfiltered row (sub-byte samples are packed from the most significant bit)
inline int sample8(const uint8_t* row, size_t i, int depth) {
  switch (depth) {
    case 16: return row[2 * i];                                             // png_set_strip_16: the high byte
    case 8: return row[i];
    default: {
      const int per = 8 / depth, shift = 8 - depth * (int)(i % per + 1);
      return (row[i / per] >> shift) & ((1 << depth) - 1);                 // the raw value; scaled by the caller
    }
  }
}
}  // namespace

int tdr_png_read_bgr8(const char* path, std::vector<uint8_t>& bgr, int& w, int& h) {
  FILE* fh = fopen(path, "rb");
  if (!fh) return fail(TDR_ERR_ARG, "png: cannot open %s", path);
  std::vector<uint8_t> file;
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), fh)) > 0) file.insert(file.end(), buf, buf + got);
  fclose(fh);
  if (file.size() < 8 || memcmp(file.data(), PNG_SIG, 8) != 0) return fail(TDR_ERR_ARG, "png: %s is not a PNG file", path);
  size_t at = 8;
  bool have_hdr = false, done = false, have_plte = false, seen_idat = false;
  PngHdr hd;
  uint8_t pal[256][3];
  memset(pal, 0, sizeof(pal));   // unverified: libpng 1.6's zero-filled palette — an index past PLTE is black
  std::vector<uint8_t> idat;
  w = h = 0;
  while (!done) {
    if (at + 12 > file.size()) return fail(TDR_ERR_ARG, "png: %s is truncated", path);
    const uint32_t len = be32(&file[at]);
    if (len > 0x7FFFFFFFu || at + 12 + (size_t)len > file.size()) return fail(TDR_ERR_ARG, "png: %s is truncated", path);
    const uint8_t* type = &file[at + 4];
    const uint8_t* data = &file[at + 8];
    if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), type, 4 + len) != be32(data + len))
      return fail(TDR_ERR_ARG, "png: %s has a chunk with a wrong CRC", path);
    const bool is_hdr = !memcmp(type, "IHDR", 4);
    if (!have_hdr && !is_hdr) return fail(TDR_ERR_ARG, "png: %s does not start with its IHDR header", path);
    if (is_hdr) {
      if (have_hdr) return fail(TDR_ERR_ARG, "png: %s has more than one IHDR header", path);
      if (len != 13) return fail(TDR_ERR_ARG, "png: %s has a malformed header", path);
      const uint32_t ww = be32(data), hh = be32(data + 4);
      if (ww < 1 || hh < 1 || ww > (1u << 24) || hh > (1u << 24)) return fail(TDR_ERR_ARG, "png: %s has an unusable size", path);
      hd.w = (int)ww; hd.h = (int)hh; hd.depth = data[8]; hd.ctype = data[9]; hd.interlace = data[12];
      if (!legal_depth(hd.ctype, hd.depth) || data[10] != 0 || data[11] != 0 || hd.interlace > 1)
        return fail(TDR_ERR_ARG, "png: %s has an invalid header (bit depth %d, colour type %d, compression %d, filter %d, "
                    "interlace %d)", path, data[8], data[9], data[10], data[11], data[12]);
      have_hdr = true;
    } else if (!memcmp(type, "PLTE", 4)) {
      if (seen_idat) return fail(TDR_ERR_ARG, "png: %s has its PLTE chunk after the image data (misplaced PLTE)", path);
      if (have_plte) return fail(TDR_ERR_ARG, "png: %s has more than one PLTE chunk", path);
      if (len % 3 != 0 || len < 3 || len > 768) return fail(TDR_ERR_ARG, "png: %s has a malformed PLTE chunk", path);
      if (hd.ctype == 3)
        for (uint32_t k = 0; k < len / 3; k++)
          for (int c = 0; c < 3; c++) pal[k][c] = data[3 * k + c];
      have_plte = true;
    } else if (!memcmp(type, "IDAT", 4)) {
      if (hd.ctype == 3 && !have_plte) return fail(TDR_ERR_ARG, "png: %s is a palette image without a PLTE chunk before "
                                                   "its image data (missing PLTE)", path);
      seen_idat = true;
      idat.insert(idat.end(), data, data + len);
    } else if (!memcmp(type, "IEND", 4)) {
      done = true;
    } else if (!(type[0] & 0x20)) {   // an unknown CRITICAL chunk
      return fail(TDR_ERR_ARG, "png: %s holds a critical chunk this reader does not know (%c%c%c%c)", path, type[0], type[1],
                  type[2], type[3]);
    }   // ancillary chunks (tRNS, gAMA, sRGB, iCCP, cHRM, tEXt, eXIf, ...): no effect
    at += 12 + (size_t)len;
  }
  if (idat.empty()) return fail(TDR_ERR_ARG, "png: %s has no image data", path);
  // the filtered stream: per pass, ph rows of 1 filter byte + the row's bytes (an empty pass has no rows at all)
  uint64_t raw_size = 0;
  for (int p = 0; p < pass_count(hd.interlace); p++) {
    int pw, ph, x0, y0, dx, dy;
    pass_shape(hd, p, pw, ph, x0, y0, dx, dy);
    if (pw > 0 && ph > 0) raw_size += (uint64_t)ph * (1 + hd.row_bytes(pw));
  }
  // deflate expands at most ~1032 : 1: a header that announces more than the image data can hold is refused before
  // anything of that size is allocated (as tdr_png_read_gray8 does)
  if (raw_size > (uint64_t)idat.size() * 1032u + 64u)
    return fail(TDR_ERR_ARG, "png: %s announces %d x %d pixels but holds %zu bytes of image data", path, hd.w, hd.h,
                idat.size());
  std::vector<uint8_t> raw((size_t)raw_size);
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (inflateInit(&zs) != Z_OK) return fail(TDR_ERR_NOMEM, "png: inflateInit failed");
  zs.next_in = idat.data();
  zs.avail_in = (uInt)idat.size();
  size_t out_at = 0;
  int zrc = Z_OK;
  while (out_at < raw.size()) {   // avail_out is a uInt: feed the output in pieces of at most 1 GiB
    const size_t piece = std::min(raw.size() - out_at, (size_t)1 << 30);
    zs.next_out = raw.data() + out_at;
    zs.avail_out = (uInt)piece;
    zrc = inflate(&zs, Z_SYNC_FLUSH);
    out_at += piece - zs.avail_out;
    if (zrc != Z_OK) break;
  }
  inflateEnd(&zs);
  if (out_at != raw.size() || (zrc != Z_OK && zrc != Z_STREAM_END && zrc != Z_BUF_ERROR))
    return fail(TDR_ERR_ARG, "png: the image data of %s does not inflate to %d x %d pixels", path, hd.w, hd.h);
  w = hd.w;
  h = hd.h;
  bgr.assign((size_t)w * h * 3, 0);
  const int bpp = std::max(1, hd.bits_pp() / 8);   // the filters' byte distance to the corresponding byte on the left
  const int gscale = hd.depth < 8 ? 255 / ((1 << hd.depth) - 1) : 1;   // v * 255 / (2^d - 1): 255, 85, 17
  size_t rp = 0;
  std::vector<uint8_t> prev, cur;
  for (int p = 0; p < pass_count(hd.interlace); p++) {
    int pw, ph, x0, y0, dx, dy;
    pass_shape(hd, p, pw, ph, x0, y0, dx, dy);
    if (pw == 0 || ph == 0) continue;
    const size_t rb = hd.row_bytes(pw);
    prev.assign(rb, 0);
    cur.assign(rb, 0);
    for (int r = 0; r < ph; r++) {
      const uint8_t* in = &raw[rp];
      rp += 1 + rb;
      const int ft = in[0];
      if (ft > 4) return fail(TDR_ERR_ARG, "png: %s uses filter type %d", path, ft);
      for (size_t i = 0; i < rb; i++) {   // unfilter (the filters work on bytes, whatever the bit depth)
        const int a = i >= (size_t)bpp ? cur[i - bpp] : 0, b = prev[i], c = i >= (size_t)bpp ? prev[i - bpp] : 0;
        int pred = 0;
        if (ft == 1) pred = a;
        else if (ft == 2) pred = b;
        else if (ft == 3) pred = (a + b) >> 1;
        else if (ft == 4) {
          const int q = a + b - c, pa = abs(q - a), pb = abs(q - b), pc = abs(q - c);
          pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
        }
        cur[i] = (uint8_t)(in[1 + i] + pred);
      }
      uint8_t* orow = &bgr[((size_t)(y0 + r * dy) * w) * 3];
      const int nch = hd.channels();
      for (int x = 0; x < pw; x++) {
        uint8_t* o = orow + (size_t)(x0 + x * dx) * 3;
        const size_t s = (size_t)x * nch;
        if (hd.ctype == 3) {                                    // palette -> RGB
          const int k = sample8(cur.data(), s, hd.depth);
          o[0] = pal[k][2]; o[1] = pal[k][1]; o[2] = pal[k][0];
        } else if (hd.ctype == 0 || hd.ctype == 4) {            // grey (+ alpha, dropped) -> all three channels
          const int g = hd.depth < 8 ? sample8(cur.data(), s, hd.depth) * gscale : sample8(cur.data(), s, hd.depth);
          o[0] = o[1] = o[2] = (uint8_t)g;
        } else {                                                // RGB (+ alpha, dropped) -> B, G, R
          o[0] = (uint8_t)sample8(cur.data(), s + 2, hd.depth);
          o[1] = (uint8_t)sample8(cur.data(), s + 1, hd.depth);
          o[2] = (uint8_t)sample8(cur.data(), s, hd.depth);
        }
      }
      std::swap(prev, cur);
    }
  }
  return TDR_OK;
}

// C-ABI face (host only, no device): bgr_out holds capacity bytes; *w / *h are set even when the image does not fit
extern "C" int tdr_png_read_color_host(const char* path, uint8_t* bgr_out, int64_t capacity, int* w, int* h) {
  if (!path || !w || !h) return fail(TDR_ERR_ARG, "png: null pointer");
  try {   // (no exception crosses the C ABI: an allocation failure is an error code)
    std::vector<uint8_t> bgr;
    if (int rc = tdr_png_read_bgr8(path, bgr, *w, *h)) return rc;
    if (!bgr_out || capacity < (int64_t)bgr.size()) return fail(TDR_ERR_ARG, "png: %s needs %zu bytes", path, bgr.size());
    memcpy(bgr_out, bgr.data(), bgr.size());
    return TDR_OK;
  } catch (const std::exception& e) {
    return fail(TDR_ERR_NOMEM, "png: %s: %s", path, e.what());
  }
}
