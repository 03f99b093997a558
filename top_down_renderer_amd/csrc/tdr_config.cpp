// tdr_config.cpp — the process-wide TdrConfig, the thread's override of it, and every call that sets a switch: the named
// calls of include/tdr.h and the table behind tdr_config_tuning.  A rule's bound that is a kernel constant comes from the
// header of the file that owns the kernel.
#include "tdr_config.h"

#include <algorithm>
#include <cstring>

#include "tdr_score_su.h"   // TDR_RAY_MAX_SPLIT; tdr_common.h: PFX_HEAD, INI_TILE, INI_MAX_TILES

namespace {
TdrConfig g_cfg;
thread_local const TdrConfig* t_override = nullptr;

// the value as the int-typed switches take it (below -1 is -1: query only)
int as_int(int64_t v) { return (int)std::max<int64_t>(v, -1); }
int64_t set_flag(int& m, int64_t v) {   // < 0: query only
  if (as_int(v) >= 0) m = as_int(v) ? 1 : 0;
  return m;
}
int64_t set_from_0(int& m, int64_t v, int hi) {   // < 0: query only; clamped to hi
  if (v >= 0) m = (int)std::min<int64_t>(v, hi);
  return m;
}

// tdr_config_tuning: name -> member and its normalising rule (the knob list of include/tdr.h)
struct Knob {
  const char* name;
  int64_t (*set)(TdrConfig& c, int64_t v);
};
const Knob kKnobs[] = {
    {"score_waves", [](TdrConfig& c, int64_t v) { if (v > 0) c.score_waves = v; return c.score_waves; }},
    {"score_group", [](TdrConfig& c, int64_t v) -> int64_t { if (v >= 0) c.score_group = (int)v; return c.score_group; }},
    {"su_group", [](TdrConfig& c, int64_t v) -> int64_t { if (v >= 0) c.su_group = (int)v; return c.su_group; }},
    {"batch_init_search", [](TdrConfig& c, int64_t v) { return set_flag(c.batch_init_search, v); }},
    {"init_ahead", [](TdrConfig& c, int64_t v) -> int64_t { if (v >= 1) c.init_ahead = (int)std::min<int64_t>(v, 3); return c.init_ahead; }},
    {"prefix_head", [](TdrConfig& c, int64_t v) -> int64_t { if (as_int(v) >= 0) c.pfx_head = std::min(std::max(as_int(v), 1), PFX_HEAD); return c.pfx_head; }},
    {"ray_borrow", [](TdrConfig& c, int64_t v) { return set_flag(c.ray_borrow, v); }},
    {"ray_patch", [](TdrConfig& c, int64_t v) { return set_flag(c.ray_patch, v); }},
    {"ray_block_major", [](TdrConfig& c, int64_t v) { return set_flag(c.ray_block_major, v); }},
    {"cart_seg_rows", [](TdrConfig& c, int64_t v) -> int64_t { if (as_int(v) >= 0) c.cart_seg_rows = as_int(v) - as_int(v) % 4; return c.cart_seg_rows; }},
    {"mt_stretches", [](TdrConfig& c, int64_t v) { return set_flag(c.mt_stretches, v); }},
    {"su_tail_groups", [](TdrConfig& c, int64_t v) { return set_from_0(c.su_tail_groups, v, 1 << 20); }},
    {"su_tail_parts", [](TdrConfig& c, int64_t v) -> int64_t {   // 1, 2, 4 or 8 (anything else: the next lower of them)
       if (v >= 0) c.su_tail_parts = v >= 8 ? 8 : (v >= 4 ? 4 : (v >= 2 ? 2 : 1));
       return c.su_tail_parts;
     }},
    {"su_order_bucket", [](TdrConfig& c, int64_t v) { return set_flag(c.su_order_bucket, v); }},
    {"su_full_list", [](TdrConfig& c, int64_t v) { return set_flag(c.su_full_list, v); }},
    {"init_device",[](TdrConfig& c, int64_t v) { return set_flag(c.init_device, v); }},
    {"init_window_words", [](TdrConfig& c, int64_t v) {   // < 1: query only; whole tiles, 1 .. INI_MAX_TILES of them
       if (v > 0) c.init_window = std::min<int64_t>((v + INI_TILE - 1) / INI_TILE * INI_TILE, (int64_t)INI_TILE * INI_MAX_TILES);
       return c.init_window;
     }},
    {"cart_init_chunk", [](TdrConfig& c, int64_t v) { if (v >= 1) c.cart_init_chunk = std::min<int64_t>(v, 1 << 24); return c.cart_init_chunk; }},
    {"inject_cand_chunk", [](TdrConfig& c, int64_t v) { if (v >= 1) c.inject_cand_chunk = std::min<int64_t>(v, 1 << 24); return c.inject_cand_chunk; }},
};
}  // namespace

const TdrConfig& tdr_cfg() { return t_override ? *t_override : g_cfg; }
TdrConfigScope::TdrConfigScope(const TdrConfig& c) : cfg_(c), outer_(t_override) { t_override = &cfg_; }
TdrConfigScope::~TdrConfigScope() { t_override = outer_; }

extern "C" {
int64_t tdr_config_tuning(const char* name, int64_t value) {   // value < 0: query only
  if (!name) return -1;
  for (const Knob& k : kKnobs)
    if (std::strcmp(name, k.name) == 0) return k.set(g_cfg, value);
  return -1;
}
// the named calls (include/tdr.h); < 0: query only
int tdr_config_compact(int on) { return (int)set_flag(g_cfg.use_compact, on); }
int tdr_config_shift_uniform(int mode) { return (int)set_from_0(g_cfg.su_mode, mode, 2); }
float tdr_config_shift_uniform_span(float cells) {   // >= 0: fix it (0: every particle counts as dense);
  if (cells >= 0.f) { g_cfg.su_span = cells; g_cfg.su_span_fixed = true; }   // -1: query only; below -1.5: back to tuning
  else if (cells < -1.5f) { g_cfg.su_span = TdrConfig{}.su_span; g_cfg.su_span_fixed = false; }
  return g_cfg.su_span;
}
int tdr_config_ray_split(int k) { return (int)set_from_0(g_cfg.ray_split, k, TDR_RAY_MAX_SPLIT); }   // >= 1: force; 0: per launch
int tdr_config_cart_skip(int on) { return (int)set_flag(g_cfg.cart_skip, on); }
int tdr_config_init_mfma(int on) { return (int)set_flag(g_cfg.init_mfma, on); }
int tdr_config_uw_waves(int on) { return (int)set_flag(g_cfg.uw_waves, on); }
int tdr_config_prefix_small(int on) { return (int)set_flag(g_cfg.pfx_small, on); }
int64_t tdr_config_rec16_min_particles(int64_t n) {
  if (n >= 0) g_cfg.rec16_min = n;
  return g_cfg.rec16_min;
}
}  // extern "C"
