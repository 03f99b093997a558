// tdr_svg.cpp — host reader for the static vector map (what TopDownMap::loadSvg, src/top_down_map.cpp:66-110, takes
// from an SVG file).  Written from the SVG 1.1 specification and the behaviour the map loader relies on:
//
//   1. the file is read into an element tree (a small XML reader: comments, processing instructions, DOCTYPE and CDATA
//      skipped, attribute values in either quote with the five predefined entities; a file that ends inside markup or
//      nests deeper than kMaxDepth is refused; elements still open at the end are closed there);
//   2. the tree is walked with an inherited context — the current user-space -> image map and the fill paint — and
//      every path / rect / circle / ellipse / line / polyline / polygon becomes subpaths in image coordinates;
//      <defs> contributes only gradients, a gradient counts as a paint when it (or what it references) has stops;
//   3. every subpath becomes one polygon: its start point and the end point of every segment except the last, so a
//      closed subpath (whose closing segment is always added, even when it has zero length) keeps all its corners and
//      an open one loses its final point; a subpath without segments gives nothing.  Vertex = (x, H - y) with H the
//      image's float height.
//
// The polygons must be the reference's to the bit, which fixes the floating-point work, not the code: coordinates are
// converted to float once, relative coordinates add in float, unit conversions divide by the unit's size and multiply
// by 96 dpi, transforms compose as 2 x 3 float matrices (degrees -> radians as deg / 180 * pi in float), the image map
// is (p + t) * s, all without FMA (the library is built with -ffp-contract=off).  Where the reference's reader departs
// from the specification on well-formed input, the reference wins, and the difference is named where it is handled:
// no preserveAspectRatio stretches the viewBox, meet / slice align the top edge whatever the Y part of the alignment
// says, only ten colour keywords are known (any other is grey), an unresolved
// gradient is colour 0, fill="none" is colour 0, arcs are split into pieces of less than a quarter turn.
// Not read: strokes, <style> sheets, <use>, text, nested viewports (a nested <svg> is a group).
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "tdr.h"
#include "tdr_internal.h"

namespace {

const size_t kMaxBytes = (size_t)1 << 28;       // 256 MiB of SVG text
const size_t kMaxVertices = (size_t)1 << 27;    // polygon vertices over the whole map
const int kMaxDepth = 1024;                     // element nesting
const int kMaxAttrs = 1024;                     // attributes of one element
const float kPi = 3.14159265358979323846f;

int svg_fail(int code, const char* fmt, ...) {
  char buf[400];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return tdr_set_error(code, buf);
}

bool ws(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }
bool dig(char c) { return c >= '0' && c <= '9'; }

// ================================================================ element tree
struct Element {
  std::string name;
  std::vector<std::pair<std::string, std::string>> attrs;
  std::vector<int> children;
  const char* get(const char* key) const {
    for (const auto& a : attrs)
      if (a.first == key) return a.second.c_str();
    return nullptr;
  }
};

class XmlReader {
 public:
  XmlReader(const char* text, size_t n) : p_(text), end_(text + n) {}
  // fills `doc` (element 0 = the root); returns false with `err` set
  bool read(std::vector<Element>& doc, std::string& err) {
    std::vector<int> open;
    bool have_root = false;
    while (p_ < end_) {
      if (*p_ != '<') { ++p_; continue; }   // character data: not used
      if (starts("<!--")) { if (!skip_past("-->")) return bad(err, "unterminated comment"); continue; }
      if (starts("<![CDATA[")) { if (!skip_past("]]>")) return bad(err, "unterminated CDATA"); continue; }
      if (starts("<?")) { if (!skip_past("?>")) return bad(err, "unterminated processing instruction"); continue; }
      if (starts("<!")) { if (!skip_declaration()) return bad(err, "unterminated declaration"); continue; }
      if (starts("</")) {
        p_ += 2;
        const std::string name = read_name();
        skip_ws();
        if (p_ >= end_ || *p_ != '>') return bad(err, "malformed end tag");
        ++p_;
        if (open.empty() || doc[open.back()].name != name) return bad(err, "end tag </" + name + "> does not match");
        open.pop_back();
        continue;
      }
      ++p_;
      Element el;
      el.name = read_name();
      if (el.name.empty()) return bad(err, "malformed start tag");
      bool self_closing = false;
      for (;;) {
        skip_ws();
        if (p_ >= end_) return bad(err, "file ends inside a tag");
        if (*p_ == '>') { ++p_; break; }
        if (*p_ == '/') {
          if (p_ + 1 >= end_ || p_[1] != '>') return bad(err, "stray '/' in a tag");
          p_ += 2;
          self_closing = true;
          break;
        }
        std::string key = read_name();
        skip_ws();
        if (key.empty() || p_ >= end_ || *p_ != '=') return bad(err, "malformed attribute in <" + el.name + ">");
        ++p_;
        skip_ws();
        if (p_ >= end_ || (*p_ != '"' && *p_ != '\'')) return bad(err, "unquoted attribute value");
        const char q = *p_++;
        const char* v0 = p_;
        while (p_ < end_ && *p_ != q) ++p_;
        if (p_ >= end_) return bad(err, "file ends inside an attribute value");
        if ((int)el.attrs.size() >= kMaxAttrs) return bad(err, "too many attributes");
        el.attrs.emplace_back(std::move(key), decode(v0, p_));
        ++p_;
      }
      const int id = (int)doc.size();
      if (open.empty()) {
        if (have_root) return bad(err, "content after the root element");
        have_root = true;
      } else {
        doc[open.back()].children.push_back(id);
      }
      doc.push_back(std::move(el));
      if (!self_closing) {
        if ((int)open.size() >= kMaxDepth) return bad(err, "elements nested too deep");
        open.push_back(id);
      }
    }
    if (!have_root) return bad(err, "no element");
    return true;   // elements still open end with the file
  }

 private:
  const char* p_;
  const char* end_;
  bool bad(std::string& err, const std::string& what) {
    err = what;
    return false;
  }
  bool starts(const char* s) const {
    const size_t n = strlen(s);
    return (size_t)(end_ - p_) >= n && memcmp(p_, s, n) == 0;
  }
  bool skip_past(const char* s) {
    const size_t n = strlen(s);
    for (const char* q = p_; (size_t)(end_ - q) >= n; ++q)
      if (memcmp(q, s, n) == 0) { p_ = q + n; return true; }
    return false;
  }
  bool skip_declaration() {   // <!DOCTYPE ... [ internal subset ] >
    int brackets = 0;
    for (const char* q = p_ + 2; q < end_; ++q) {
      if (*q == '[') brackets++;
      else if (*q == ']') brackets--;
      else if (*q == '>' && brackets <= 0) { p_ = q + 1; return true; }
    }
    return false;
  }
  void skip_ws() { while (p_ < end_ && ws(*p_)) ++p_; }
  std::string read_name() {
    const char* s = p_;
    while (p_ < end_ && !ws(*p_) && *p_ != '>' && *p_ != '/' && *p_ != '=' && *p_ != '<' && *p_ != '"' && *p_ != '\'') ++p_;
    return std::string(s, p_);
  }
  static std::string decode(const char* a, const char* b) {
    static const struct { const char* ent; char c; } ents[] = {
        {"&amp;", '&'}, {"&lt;", '<'}, {"&gt;", '>'}, {"&quot;", '"'}, {"&apos;", '\''}};
    std::string out;
    out.reserve((size_t)(b - a));
    while (a < b) {
      bool hit = false;
      if (*a == '&')
        for (const auto& e : ents) {
          const size_t n = strlen(e.ent);
          if ((size_t)(b - a) >= n && memcmp(a, e.ent, n) == 0) { out.push_back(e.c); a += n; hit = true; break; }
        }
      if (!hit) out.push_back(*a++);
    }
    return out;
  }
};

// ================================================================ numbers and lengths
// One SVG number at *s ([+-] digits [. digits] [(e|E) [+-] digits], either digit run may be empty but not both):
// decimal mantissa (19 significant digits) and exponent, scaled in double, rounded to float once.  Returns false and
// leaves *s when there is no number.
bool read_number(const char*& s, float& out) {
  const char* p = s;
  bool neg = false;
  if (*p == '+' || *p == '-') neg = *p++ == '-';
  uint64_t mant = 0;
  int digits = 0, exp10 = 0;
  bool any = false;
  for (; dig(*p); ++p, any = true) {
    if (digits < 19) { mant = mant * 10 + (uint64_t)(*p - '0'); if (mant) digits++; }
    else exp10++;
  }
  if (*p == '.') {
    ++p;
    for (; dig(*p); ++p, any = true)
      if (digits < 19) { mant = mant * 10 + (uint64_t)(*p - '0'); if (mant) digits++; exp10--; }
  }
  if (!any) return false;
  if ((*p == 'e' || *p == 'E') && (dig(p[1]) || ((p[1] == '+' || p[1] == '-') && dig(p[2])))) {
    ++p;
    bool eneg = false;
    if (*p == '+' || *p == '-') eneg = *p++ == '-';
    long e = 0;
    for (; dig(*p); ++p)
      if (e < 100000) e = e * 10 + (*p - '0');
    exp10 += (int)(eneg ? -e : e);
  }
  static const double pow10[] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11,
                                 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  double v = (double)mant;
  if (mant == 0) v = 0.0;
  else if (exp10 >= 0 && exp10 <= 22) v *= pow10[exp10];
  else if (exp10 < 0 && exp10 >= -22) v /= pow10[-exp10];
  else v *= pow(10.0, (double)exp10);
  out = (float)(neg ? -v : v);
  s = p;
  return true;
}

// a length attribute: number + optional unit; `pct_origin + pct * pct_base / 100` for percentages
struct Viewport {
  float x = 0, y = 0, w = 0, h = 0;   // the root's viewBox (user units)
  float diag() const { return sqrtf(w * w + h * h) / sqrtf(2.0f); }
};
float length(const char* s, float pct_origin, float pct_base) {
  if (!s) return 0.f;
  float v = 0.f;
  if (!read_number(s, v)) return 0.f;
  static const struct { const char* unit; float size, px; } units[] = {   // value / size * px  (96 px per inch)
      {"px", 1.f, 1.f}, {"pt", 72.f, 96.f}, {"pc", 6.f, 96.f}, {"mm", 25.4f, 96.f}, {"cm", 2.54f, 96.f}, {"in", 1.f, 96.f}};
  if (*s == '%') return pct_origin + v / 100.0f * pct_base;
  for (const auto& u : units)
    if (strncmp(s, u.unit, 2) == 0) return v / u.size * u.px;
  return v;   // user units (em / ex are not supported: no font model)
}

// ================================================================ transforms
struct Affine {   // x' = a x + c y + e,  y' = b x + d y + f
  float a = 1, b = 0, c = 0, d = 1, e = 0, f = 0;
};
// the map that applies `first`, then `second`
Affine compose(const Affine& first, const Affine& second) {
  Affine r;
  r.a = first.a * second.a + first.b * second.c;
  r.b = first.a * second.b + first.b * second.d;
  r.c = first.c * second.a + first.d * second.c;
  r.d = first.c * second.b + first.d * second.d;
  r.e = first.e * second.a + first.f * second.c + second.e;
  r.f = first.e * second.b + first.f * second.d + second.f;
  return r;
}
void apply(const Affine& m, float x, float y, float& ox, float& oy) {
  ox = x * m.a + y * m.c + m.e;
  oy = x * m.b + y * m.d + m.f;
}
float radians(float deg) { return deg / 180.0f * kPi; }

// transform="f1(...) f2(...) ...": points go through the last function first
Affine parse_transform(const char* s) {
  Affine total;
  for (;;) {
    while (*s && (ws(*s) || *s == ',')) ++s;
    const char* name = s;
    while (*s && ((*s >= 'a' && *s <= 'z') || (*s >= 'A' && *s <= 'Z'))) ++s;
    const std::string fn(name, s);
    while (*s && ws(*s)) ++s;
    if (fn.empty() || *s != '(') return total;   // end of the list, or not a transform list: keep what was read
    ++s;
    float arg[6] = {0, 0, 0, 0, 0, 0};
    int n = 0;
    for (;;) {
      while (*s && (ws(*s) || *s == ',')) ++s;
      if (*s == ')') { ++s; break; }
      float v;
      if (n >= 6 || !read_number(s, v)) return total;
      arg[n++] = v;
    }
    Affine t;
    if (fn == "matrix" && n == 6) {
      t.a = arg[0]; t.b = arg[1]; t.c = arg[2]; t.d = arg[3]; t.e = arg[4]; t.f = arg[5];
    } else if (fn == "translate" && (n == 1 || n == 2)) {
      t.e = arg[0];
      t.f = n == 2 ? arg[1] : 0.f;
    } else if (fn == "scale" && (n == 1 || n == 2)) {
      t.a = arg[0];
      t.d = n == 2 ? arg[1] : arg[0];
    } else if (fn == "rotate" && (n == 1 || n == 3)) {
      Affine r;
      const float ang = radians(arg[0]);
      r.a = cosf(ang); r.b = sinf(ang); r.c = -r.b; r.d = r.a;
      if (n == 3) {   // about (cx, cy): move it to the origin, turn, move back
        Affine to, back;
        to.e = -arg[1]; to.f = -arg[2];
        back.e = arg[1]; back.f = arg[2];
        t = compose(compose(compose(Affine(), to), r), back);
      } else {
        t = r;
      }
    } else if (fn == "skewX" && n == 1) {
      t.c = tanf(radians(arg[0]));
    } else if (fn == "skewY" && n == 1) {
      t.b = tanf(radians(arg[0]));
    } else {
      continue;   // unknown function or wrong argument count: ignored
    }
    total = compose(t, total);
  }
}

// ================================================================ paint
struct Paint {
  enum Kind { kColor, kNone, kUrl } kind = kColor;
  uint32_t key = 0;      // 0xBBGGRR (black by default)
  std::string ref;       // kUrl: the referenced id
};

int hex_digit(char c) {
  if (dig(c)) return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  if (c >= 'A' && c <= 'F') return c - 'A' + 10;
  return -1;
}
uint32_t bgr(int r, int g, int b) { return (uint32_t)r | (uint32_t)g << 8 | (uint32_t)b << 16; }

Paint parse_paint(std::string v) {
  while (!v.empty() && ws(v.back())) v.pop_back();
  size_t i = 0;
  while (i < v.size() && ws(v[i])) ++i;
  v = v.substr(i);
  Paint p;
  if (v == "none") { p.kind = Paint::kNone; return p; }
  if (v.compare(0, 4, "url(") == 0) {
    p.kind = Paint::kUrl;
    size_t a = 4, b = v.find(')', 4);
    if (b == std::string::npos) b = v.size();
    if (a < b && v[a] == '#') a++;
    p.ref = v.substr(a, b - a).substr(0, 63);
    return p;
  }
  if (!v.empty() && v[0] == '#') {   // #rgb or #rrggbb; any other form is black
    std::vector<int> h;
    for (size_t k = 1; k < v.size(); k++) h.push_back(hex_digit(v[k]));
    bool ok = true;
    for (int x : h) ok = ok && x >= 0;
    if (ok && h.size() == 6) p.key = bgr(h[0] * 16 + h[1], h[2] * 16 + h[3], h[4] * 16 + h[5]);
    else if (ok && h.size() == 3) p.key = bgr(h[0] * 17, h[1] * 17, h[2] * 17);
    return p;
  }
  if (v.compare(0, 4, "rgb(") == 0) {   // three integers, all percentages or none; clamped to [0, 255]
    const char* s = v.c_str() + 4;
    int c[3] = {0, 0, 0};
    bool pct = false;
    for (int k = 0; k < 3; k++) {
      while (*s && (ws(*s) || *s == ',')) ++s;
      bool neg = false;
      if (*s == '+' || *s == '-') neg = *s++ == '-';
      long x = 0;
      for (; dig(*s); ++s)
        if (x < 100000) x = x * 10 + (*s - '0');
      if (*s == '%') { pct = true; ++s; }
      c[k] = (int)(neg ? -x : x);
    }
    for (int& x : c) {
      if (pct) x = x * 255 / 100;
      x = x < 0 ? 0 : x > 255 ? 255 : x;
    }
    p.key = bgr(c[0], c[1], c[2]);
    return p;
  }
  // the reference's reader is built with the ten basic keywords only; every other name is grey there
  static const struct { const char* name; int r, g, b; } names[] = {
      {"black", 0, 0, 0},       {"white", 255, 255, 255}, {"red", 255, 0, 0},     {"green", 0, 128, 0},
      {"blue", 0, 0, 255},      {"yellow", 255, 255, 0},  {"cyan", 0, 255, 255},  {"magenta", 255, 0, 255},
      {"gray", 128, 128, 128},  {"grey", 128, 128, 128}};
  p.key = bgr(128, 128, 128);
  for (const auto& n : names)
    if (v == n.name) p.key = bgr(n.r, n.g, n.b);
  return p;
}

// ================================================================ geometry
struct Pt {
  float x, y;
};
struct Subpath {
  std::vector<Pt> pts;   // start point, then the end point of every segment (user space)
  bool closed = false;
};

// elliptical arc from `from` to `to` (SVG 1.1 F.6.5 centre parameterisation), appended as the end points of pieces of
// less than a quarter turn each: n = 1 + (number of whole quarter turns in the sweep)
void arc_to(std::vector<Pt>& pts, Pt from, Pt to, float rx, float ry, float phi_deg, bool large, bool sweep) {
  rx = fabsf(rx);
  ry = fabsf(ry);
  const float dx = from.x - to.x, dy = from.y - to.y;
  if (sqrtf(dx * dx + dy * dy) < 1e-6f || rx < 1e-6f || ry < 1e-6f) {   // degenerate: a straight segment
    pts.push_back(to);
    return;
  }
  const float phi = radians(phi_deg);
  const float sp = sinf(phi), cp = cosf(phi);
  // F.6.5.1: the start point in the ellipse's frame, relative to the chord's midpoint
  const float xp = cp * dx / 2.0f + sp * dy / 2.0f;
  const float yp = -sp * dx / 2.0f + cp * dy / 2.0f;
  // F.6.6.2: radii too small for the chord grow uniformly
  const float lambda = (xp * xp) / (rx * rx) + (yp * yp) / (ry * ry);
  if (lambda > 1) {
    const float g = sqrtf(lambda);
    rx *= g;
    ry *= g;
  }
  // F.6.5.2: the centre in the ellipse's frame
  const float rx2 = rx * rx, ry2 = ry * ry;
  float num = rx2 * ry2 - rx2 * (yp * yp) - ry2 * (xp * xp);
  const float den = rx2 * (yp * yp) + ry2 * (xp * xp);
  if (num < 0.0f) num = 0.0f;
  float k = den > 0.0f ? sqrtf(num / den) : 0.0f;
  if (large == sweep) k = -k;
  const float cxp = k * rx * yp / ry;
  const float cyp = k * -ry * xp / rx;
  // F.6.5.3: the centre in user space
  const float cx = (from.x + to.x) / 2.0f + cp * cxp - sp * cyp;
  const float cy = (from.y + to.y) / 2.0f + sp * cxp + cp * cyp;
  // F.6.5.5-6: start angle and sweep
  auto angle_between = [](float ux, float uy, float vx, float vy) {
    float cosv = (ux * vx + uy * vy) / (sqrtf(ux * ux + uy * uy) * sqrtf(vx * vx + vy * vy));
    cosv = cosv < -1.0f ? -1.0f : cosv > 1.0f ? 1.0f : cosv;
    const float sign = ux * vy < uy * vx ? -1.0f : 1.0f;
    return sign * acosf(cosv);
  };
  const float ux = (xp - cxp) / rx, uy = (yp - cyp) / ry;
  const float vx = (-xp - cxp) / rx, vy = (-yp - cyp) / ry;
  const float theta1 = angle_between(1.0f, 0.0f, ux, uy);
  float dtheta = angle_between(ux, uy, vx, vy);
  if (!sweep && dtheta > 0) dtheta -= 2 * kPi;
  else if (sweep && dtheta < 0) dtheta += 2 * kPi;
  const float quarters = fabsf(dtheta) / (kPi * 0.5f);
  const int pieces = quarters < 8.f ? (int)(quarters + 1.0f) : 8;   // (|dtheta| < 3 pi for finite input)
  for (int i = 1; i <= pieces; i++) {
    const float t = theta1 + dtheta * ((float)i / (float)pieces);
    const float ex = cosf(t) * rx, ey = sinf(t) * ry;   // on the axis-aligned ellipse, then rotated and moved
    pts.push_back(Pt{ex * cp + ey * -sp + cx, ex * sp + ey * cp + cy});
  }
}

// path data (SVG 1.1 8.3): commands with implicit repetition; parsing stops at the first error, keeping what came before
std::vector<Subpath> parse_path_data(const char* s) {
  std::vector<Subpath> out;
  Subpath cur;
  bool have_cur = false;
  Pt pos{0, 0}, start{0, 0};
  char cmd = 0;
  auto flush = [&]() {
    if (have_cur) out.push_back(std::move(cur));
    cur = Subpath();
    have_cur = false;
  };
  auto skip = [&]() { while (*s && (ws(*s) || *s == ',')) ++s; };
  auto nums = [&](float* v, int n) {
    const char* save = s;
    for (int i = 0; i < n; i++) {
      skip();
      if (!read_number(s, v[i])) { s = save; return false; }
    }
    return true;
  };
  for (;;) {
    skip();
    if (!*s) break;
    const char c = *s;
    if ((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z')) {
      cmd = c;
      ++s;
      if (cmd == 'Z' || cmd == 'z') {   // close: the segment back to the start is always added
        if (have_cur && cur.pts.size() >= 2) {
          cur.pts.push_back(start);
          cur.closed = true;
          flush();
        }
        cur = Subpath();
        pos = start;
        cur.pts.push_back(start);        // a drawing command without a moveto continues from here
        have_cur = true;
        continue;
      }
    } else if (!cmd || cmd == 'Z' || cmd == 'z') {
      break;                             // numbers without a command
    }
    const bool rel = cmd >= 'a' && cmd <= 'z';
    const char up = rel ? (char)(cmd - 32) : cmd;
    float v[7];
    if (up == 'M') {
      if (!nums(v, 2)) break;
      flush();
      pos = rel ? Pt{pos.x + v[0], pos.y + v[1]} : Pt{v[0], v[1]};
      start = pos;
      cur.pts.push_back(pos);
      have_cur = true;
      cmd = rel ? 'l' : 'L';             // further pairs are line-tos
      continue;
    }
    if (!have_cur) break;                // drawing before any moveto
    if (up == 'L' || up == 'T') {
      if (!nums(v, 2)) break;
      pos = rel ? Pt{pos.x + v[0], pos.y + v[1]} : Pt{v[0], v[1]};
    } else if (up == 'H') {
      if (!nums(v, 1)) break;
      pos.x = rel ? pos.x + v[0] : v[0];
    } else if (up == 'V') {
      if (!nums(v, 1)) break;
      pos.y = rel ? pos.y + v[0] : v[0];
    } else if (up == 'C' || up == 'S' || up == 'Q') {   // only the end point matters for the polygon
      const int n = up == 'C' ? 6 : 4;
      if (!nums(v, n)) break;
      pos = rel ? Pt{pos.x + v[n - 2], pos.y + v[n - 1]} : Pt{v[n - 2], v[n - 1]};
    } else if (up == 'A') {
      if (!nums(v, 7)) break;
      const Pt to = rel ? Pt{pos.x + v[5], pos.y + v[6]} : Pt{v[5], v[6]};
      arc_to(cur.pts, pos, to, v[0], v[1], v[2], fabsf(v[3]) > 1e-6, fabsf(v[4]) > 1e-6);
      pos = to;
      continue;
    } else {
      break;                             // unknown command
    }
    cur.pts.push_back(pos);
  }
  flush();
  return out;
}

// ================================================================ the walk
struct Context {
  Affine m;      // user space -> image space before the viewBox map
  Paint fill;
};
struct Gradient {
  std::string id, href;
  int stops = 0;
};
struct Shape {
  uint32_t key;
  std::vector<std::vector<Pt>> polys;   // image space before the viewBox map
};

class Walker {
 public:
  explicit Walker(const std::vector<Element>& doc) : doc_(doc) {}
  std::vector<Shape> shapes;
  Viewport vb;
  size_t vertices = 0;
  bool too_many = false;

  void walk(int id, const Context& parent, int depth) {
    const Element& el = doc_[(size_t)id];
    const std::string& n = el.name;
    if (n == "linearGradient" || n == "radialGradient") return add_gradient(el);
    if (n == "defs") return gradients_in(id);   // nothing in <defs> is drawn
    const bool group = n == "g" || n == "svg";
    const bool shape = n == "path" || n == "rect" || n == "circle" || n == "ellipse" || n == "line" ||
                       n == "polyline" || n == "polygon";
    if (!group && !shape) {   // an element this reader does not know: its children still count, its attributes not
      for (int c : el.children) walk(c, parent, depth + 1);
      return;
    }
    Context ctx = parent;
    if (const char* t = el.get("transform")) ctx.m = compose(parse_transform(t), parent.m);
    if (const char* f = el.get("fill")) ctx.fill = parse_paint(f);
    if (const char* st = el.get("style")) style_fill(st, ctx.fill);   // a style declaration beats the attribute
    if (group) {
      for (int c : el.children) walk(c, ctx, depth + 1);
      return;
    }
    emit(el, ctx);
  }

 private:
  const std::vector<Element>& doc_;
  std::vector<Gradient> grads_;

  void add_gradient(const Element& el) {
    Gradient g;
    if (const char* id = el.get("id")) g.id = std::string(id).substr(0, 63);
    const char* href = el.get("xlink:href");
    if (!href) href = el.get("href");
    if (href && href[0] == '#') g.href = std::string(href + 1).substr(0, 62);
    for (int c : el.children) g.stops += doc_[(size_t)c].name == "stop" ? 1 : 0;
    grads_.push_back(std::move(g));
  }
  void gradients_in(int id) {
    for (int c : doc_[(size_t)id].children) {
      const Element& e = doc_[(size_t)c];
      if (e.name == "linearGradient" || e.name == "radialGradient") add_gradient(e);
      else gradients_in(c);
    }
  }
  const Gradient* find_gradient(const std::string& id) const {   // the latest definition so far wins
    for (size_t i = grads_.size(); i-- > 0;)
      if (grads_[i].id == id) return &grads_[i];
    return nullptr;
  }
  static void style_fill(const char* st, Paint& fill) {
    std::string s(st);
    size_t at = 0;
    while (at <= s.size()) {
      size_t semi = s.find(';', at);
      if (semi == std::string::npos) semi = s.size();
      const std::string decl = s.substr(at, semi - at);
      const size_t colon = decl.find(':');
      if (colon != std::string::npos) {
        std::string prop = decl.substr(0, colon);
        while (!prop.empty() && ws(prop.back())) prop.pop_back();
        size_t b = 0;
        while (b < prop.size() && ws(prop[b])) ++b;
        if (prop.substr(b) == "fill") fill = parse_paint(decl.substr(colon + 1));
      }
      at = semi + 1;
    }
  }
  // the colour key of a paint (TDR_SVG_NO_KEY: a gradient).  An unresolved gradient reference is colour 0, as in the
  // reference's reader; so is fill="none" (the loader compares colours only).
  uint32_t key_of(const Paint& p) const {
    if (p.kind == Paint::kColor) return p.key & 0xFFFFFFu;
    if (p.kind == Paint::kNone) return 0u;
    const Gradient* g = find_gradient(p.ref);
    for (int hop = 0; g && hop < 32; hop++) {
      if (g->stops > 0) return TDR_SVG_NO_KEY;
      g = g->href.empty() ? nullptr : find_gradient(g->href);
    }
    return 0u;
  }
  float len_x(const Element& e, const char* k) const { return length(e.get(k), vb.x, vb.w); }
  float len_y(const Element& e, const char* k) const { return length(e.get(k), vb.y, vb.h); }
  float size_x(const Element& e, const char* k) const { return length(e.get(k), 0.f, vb.w); }
  float size_y(const Element& e, const char* k) const { return length(e.get(k), 0.f, vb.h); }

  static std::vector<Pt> points_list(const char* s) {
    std::vector<Pt> pts;
    float x, y;
    for (;;) {
      while (*s && (ws(*s) || *s == ',')) ++s;
      if (!read_number(s, x)) break;
      while (*s && (ws(*s) || *s == ',')) ++s;
      if (!read_number(s, y)) break;   // an odd number of coordinates: the last one is ignored
      pts.push_back(Pt{x, y});
    }
    return pts;
  }

  void emit(const Element& el, const Context& ctx) {
    const std::string& n = el.name;
    std::vector<Subpath> subs;
    if (n == "path") {
      if (const char* d = el.get("d")) subs = parse_path_data(d);
    } else if (n == "rect") {
      const float x = len_x(el, "x"), y = len_y(el, "y"), w = size_x(el, "width"), h = size_y(el, "height");
      float rx = el.get("rx") ? fabsf(size_x(el, "rx")) : -1.f, ry = el.get("ry") ? fabsf(size_y(el, "ry")) : -1.f;
      if (rx < 0.f) rx = ry;   // one radius given: both are that
      if (ry < 0.f) ry = rx;
      rx = rx < 0.f ? 0.f : rx > w / 2.0f ? w / 2.0f : rx;
      ry = ry < 0.f ? 0.f : ry > h / 2.0f ? h / 2.0f : ry;
      if (w == 0.f || h == 0.f) return;
      Subpath sp;
      sp.closed = true;
      if (rx > 0.f && ry > 0.f)   // each side's straight part, then the quarter ellipse of the next corner
        sp.pts = {{x + rx, y}, {x + w - rx, y}, {x + w, y + ry}, {x + w, y + h - ry}, {x + w - rx, y + h},
                  {x + rx, y + h}, {x, y + h - ry}, {x, y + ry}, {x + rx, y}, {x + rx, y}};
      else
        sp.pts = {{x, y}, {x + w, y}, {x + w, y + h}, {x, y + h}, {x, y}};
      subs.push_back(std::move(sp));
    } else if (n == "circle" || n == "ellipse") {
      const float cx = len_x(el, "cx"), cy = len_y(el, "cy");
      float rx, ry;
      if (n == "circle") rx = ry = fabsf(length(el.get("r"), 0.f, vb.diag()));
      else rx = fabsf(size_x(el, "rx")), ry = fabsf(size_y(el, "ry"));
      if (!(rx > 0.f && ry > 0.f)) return;
      Subpath sp;   // four quarter arcs from the rightmost point, through +y first
      sp.closed = true;
      sp.pts = {{cx + rx, cy}, {cx, cy + ry}, {cx - rx, cy}, {cx, cy - ry}, {cx + rx, cy}, {cx + rx, cy}};
      subs.push_back(std::move(sp));
    } else if (n == "line") {
      Subpath sp;
      sp.pts = {{len_x(el, "x1"), len_y(el, "y1")}, {len_x(el, "x2"), len_y(el, "y2")}};
      subs.push_back(std::move(sp));
    } else {   // polyline / polygon
      Subpath sp;
      if (const char* p = el.get("points")) sp.pts = points_list(p);
      if (n == "polygon" && sp.pts.size() >= 2) {
        sp.pts.push_back(sp.pts[0]);
        sp.closed = true;
      }
      subs.push_back(std::move(sp));
    }
    Shape sh;
    sh.key = key_of(ctx.fill);
    for (const Subpath& sp : subs) {
      // a subpath without a segment gives nothing; the polygon is every point but the last (for a closed subpath the
      // last is the closing segment's end, its start again)
      const size_t nv = sp.pts.size() >= 2 ? sp.pts.size() - 1 : 0;
      if (nv == 0) continue;
      if ((vertices += nv) > kMaxVertices) { too_many = true; return; }
      std::vector<Pt> poly(nv);
      for (size_t i = 0; i < nv; i++) apply(ctx.m, sp.pts[i].x, sp.pts[i].y, poly[i].x, poly[i].y);
      sh.polys.push_back(std::move(poly));
    }
    if (!sh.polys.empty()) shapes.push_back(std::move(sh));
  }
};

// preserveAspectRatio: {align x, align y} in {0 min, 1 mid, 2 max}, mode 0 stretch, 1 meet, 2 slice
struct Aspect {
  int ax = 1, ay = 0, mode = 0;   // absent: the reference's reader stretches the viewBox onto the image
};
Aspect parse_aspect(const char* s) {
  Aspect a;
  if (!s) return a;
  std::string t(s);
  size_t b = 0;
  while (b < t.size() && ws(t[b])) ++b;
  size_t e = b;
  while (e < t.size() && !ws(t[e])) ++e;
  const std::string align = t.substr(b, e - b);
  while (e < t.size() && ws(t[e])) ++e;
  const std::string mode = t.substr(e, 5);
  if (align == "none") return a;
  static const char* axis[3] = {"Min", "Mid", "Max"};
  // the vertical part (YMin / YMid / YMax) is read but not used: the reference's reader always aligns the top edge
  if (align.size() == 8 && align[0] == 'x' && align[4] == 'Y')
    for (int k = 0; k < 3; k++)
      if (align.compare(1, 3, axis[k]) == 0) a.ax = k;
  a.ay = 0;
  a.mode = mode == "slice" ? 2 : 1;
  return a;
}

struct Out {
  float w = 0, h = 0;
  std::vector<uint32_t> keys;
  std::vector<int64_t> offs;
  std::vector<float> verts;
};

int parse_file(const char* path, Out& out) {
  if (!path) return svg_fail(TDR_ERR_ARG, "svg: null path");
  FILE* fh = fopen(path, "rb");
  if (!fh) return svg_fail(TDR_ERR_ARG, "svg: cannot open %s", path);
  std::vector<char> text;
  bool ok = fseek(fh, 0, SEEK_END) == 0;
  const long size = ok ? ftell(fh) : -1;
  ok = ok && size >= 0 && (size_t)size <= kMaxBytes && fseek(fh, 0, SEEK_SET) == 0;
  if (ok) {
    text.resize((size_t)size + 1, 0);
    ok = fread(text.data(), 1, (size_t)size, fh) == (size_t)size;
  }
  fclose(fh);
  if (!ok) return svg_fail(TDR_ERR_ARG, "svg: %s is unreadable or larger than %zu bytes", path, kMaxBytes);

  std::vector<Element> doc;
  std::string err;
  XmlReader xml(text.data(), strlen(text.data()));   // (the text ends at the first NUL byte)
  if (!xml.read(doc, err)) return svg_fail(TDR_ERR_ARG, "svg: %s: %s", path, err.c_str());
  const Element& root = doc[0];
  if (root.name != "svg") return svg_fail(TDR_ERR_ARG, "svg: %s: the root element is <%s>, not <svg>", path, root.name.c_str());

  // the image size: width / height (lengths; a percentage has nothing to refer to), else the viewBox's
  Walker walker(doc);
  Viewport& vb = walker.vb;
  if (const char* v = root.get("viewBox")) {
    float q[4];
    int n = 0;
    for (const char* s = v; n < 4;) {
      while (*s && (ws(*s) || *s == ',')) ++s;
      if (!read_number(s, q[n])) break;
      n++;
    }
    if (n == 4) { vb.x = q[0]; vb.y = q[1]; vb.w = q[2]; vb.h = q[3]; }
  }
  float W = length(root.get("width"), 0.f, 0.f), H = length(root.get("height"), 0.f, 0.f);
  if (W == 0.f) W = vb.w;
  if (H == 0.f) H = vb.h;
  if (vb.w == 0.f) vb.w = W;
  if (vb.h == 0.f) vb.h = H;
  if (!(W > 0.f && H > 0.f && vb.w > 0.f && vb.h > 0.f) || !std::isfinite(W) || !std::isfinite(H) ||
      !std::isfinite(vb.w) || !std::isfinite(vb.h) || W >= 2147483520.f || H >= 2147483520.f)
    return svg_fail(TDR_ERR_ARG, "svg: %s has no usable size (width / height / viewBox)", path);

  walker.walk(0, Context(), 0);
  if (walker.too_many) return svg_fail(TDR_ERR_ARG, "svg: %s has more than %zu polygon vertices", path, kMaxVertices);

  // viewBox -> image: p' = (p + t) * s
  const Aspect asp = parse_aspect(root.get("preserveAspectRatio"));
  float sx = W / vb.w, sy = H / vb.h, tx = -vb.x, ty = -vb.y;
  if (asp.mode != 0) {
    const float s = asp.mode == 1 ? (sx < sy ? sx : sy) : (sx > sy ? sx : sy);
    sx = sy = s;
    auto slack = [](float content, float container, int align) {   // where the content sits in the container
      return align == 0 ? 0.f : align == 2 ? container - content : (container - content) * 0.5f;
    };
    tx += slack(vb.w * s, W, asp.ax) / s;
    ty += slack(vb.h * s, H, asp.ay) / s;
  }
  out.w = W;
  out.h = H;
  out.offs.push_back(0);
  for (const Shape& sh : walker.shapes)
    for (const auto& poly : sh.polys) {
      for (const Pt& p : poly) {
        const float x = (p.x + tx) * sx, y = H - (p.y + ty) * sy;
        if (!std::isfinite(x) || !std::isfinite(y)) return svg_fail(TDR_ERR_ARG, "svg: %s: a coordinate overflows float", path);
        out.verts.push_back(x);
        out.verts.push_back(y);
      }
      out.keys.push_back(sh.key);
      out.offs.push_back((int64_t)(out.verts.size() / 2));
    }
  return TDR_OK;
}

}  // namespace

// internal (tdr_host_map_load.cpp): the parsed map
int tdr_svg_parse_internal(const char* path, float* w, float* h, std::vector<uint32_t>& keys, std::vector<int64_t>& offs,
                           std::vector<float>& verts) {
  try {
    Out o;
    const int rc = parse_file(path, o);
    if (rc != TDR_OK) return rc;
    *w = o.w;
    *h = o.h;
    keys.swap(o.keys);
    offs.swap(o.offs);
    verts.swap(o.verts);
    return TDR_OK;
  } catch (const std::bad_alloc&) {
    return svg_fail(TDR_ERR_NOMEM, "svg: out of host memory");
  } catch (const std::exception& e) {
    return svg_fail(TDR_ERR_ARG, "svg: %s", e.what());
  }
}

extern "C" int tdr_svg_parse_host(const char* path, float size_out[2], int64_t* n_poly, int64_t* n_vert, uint32_t* keys_out,
                                  int64_t* offsets_out, float* verts_out) {
  if (!path || !size_out || !n_poly || !n_vert) return svg_fail(TDR_ERR_ARG, "svg_parse_host: null pointer");
  float w = 0, h = 0;
  std::vector<uint32_t> keys;
  std::vector<int64_t> offs;
  std::vector<float> verts;
  const int rc = tdr_svg_parse_internal(path, &w, &h, keys, offs, verts);
  if (rc != TDR_OK) return rc;
  const int64_t cap_p = *n_poly, cap_v = *n_vert;
  size_out[0] = w;
  size_out[1] = h;
  *n_poly = (int64_t)keys.size();
  *n_vert = (int64_t)(verts.size() / 2);
  if (!keys_out && !offsets_out && !verts_out) return TDR_OK;   // size query
  if (!keys_out || !offsets_out || !verts_out) return svg_fail(TDR_ERR_ARG, "svg_parse_host: give all three arrays or none");
  if (cap_p < *n_poly || cap_v < *n_vert)
    return svg_fail(TDR_ERR_ARG, "svg_parse_host: arrays hold %lld polygons / %lld vertices, the map has %lld / %lld",
                    (long long)cap_p, (long long)cap_v, (long long)*n_poly, (long long)*n_vert);
  if (!keys.empty()) memcpy(keys_out, keys.data(), keys.size() * sizeof(uint32_t));
  memcpy(offsets_out, offs.data(), offs.size() * sizeof(int64_t));
  if (!verts.empty()) memcpy(verts_out, verts.data(), verts.size() * sizeof(float));
  return TDR_OK;
}
