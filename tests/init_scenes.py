"""Scenes and rows of tests/test_init_variants.py — one row per instantiation of the 40-rotation heading search
(csrc/tdr_score_init.hip) — and their exact references (tests/init_exact_ref.py).  CPU only; not a test module:
tests/test_init_exact_ref.py shows on the CPU that every scene is fair (the 90 % condition below).

A scene: a synthetic map of 257^2 cells or less, about 6000 scan points, 200 particles without a heading (a ragged last
batch of 64) around the true pose, and in every scene
  * particles 0-3 far outside the map (every cell unknown: no candidate can win, theta stays 0),
  * particles 4-9 at the border (the window half known, more or less),
  * particles 10-19 with a heading already (untouched),
  * particles 64-127, a whole batch, with a heading already (the workgroup returns early and counts nothing).
mode "pscale": per-particle scales in [0.3, 12] on both sides of the scale gate with fixed_scale = -1, and force_on_map.

CONDITION: in every (scene, mode, scan, weights) a row uses at least 90 % of the searched particles have their cheapest
shift class separated from the next by more than TAU (relative, exact costs) — for those the rules of check_choice pin
theta to one value."""
import numpy as np

import init_exact_ref as X
from top_down_renderer_amd import synth

N_PTS = 6000
BIG = 1 << 30          # tdr_config_rec16_min_particles above any filter here: no half records
W_UNEQUAL = [1.0, 0.5, 2.0, 1.5, 0.7, 1.2, 0.9, 1.1, 0.6, 1.7, 0.8, 1.4, 1.3, 0.55, 1.9]
W_SECOND = [0.25, 1.0, 1.0, 4.0, 1.0, 2.0, 0.5]
HALF, SPLIT, WIDE, VECTOR = 12, 13, 14, 15     # slots of tdr_profile_variants

# name -> ncls, nb, nr, map size, scan resolution, particles
SCENES = {
    "c6": (6, 64, 16, 257, 1.0, 200),
    "c7": (7, 64, 16, 257, 1.0, 200),
    "c3": (3, 64, 16, 257, 1.0, 200),
    "c2": (2, 64, 16, 257, 2.0, 200),            # (a longer reach: with one or two classes the short one leaves ties)
    "c1": (1, 64, 16, 257, 2.0, 200),
    "c6_129x7": (6, 129, 7, 257, 2.0, 200),      # nb no multiple of AHEAD + 1 nor of 4; a ragged ring group of four
    "c3_36x7": (3, 36, 7, 160, 2.0, 200),        # 36 shifts for 40 candidates: the first-of-class rule
    "c6_36x7": (6, 36, 7, 160, 2.0, 200),
    "c6_8x16": (6, 8, 16, 257, 1.0, 200),        # 8 shifts, five candidates each: two classes (first members 13 and 28)
    "c11_8x16": (11, 8, 16, 257, 1.0, 200),      # whose later members sit in a LOWER lane of the matrix-core kernels
    "c6_100x25": (6, 100, 25, 257, 2.0, 200),    # the node's defaults
    "c6_512x4": (6, 512, 4, 257, 4.0, 64),       # the half kernel's LDS does not fit
    "c8": (8, 64, 16, 257, 1.0, 200),
    "c11": (11, 64, 16, 257, 1.0, 200),
    "c12": (12, 64, 16, 257, 1.0, 200),
    "c15": (15, 64, 16, 257, 1.0, 200),
}
_SCENES, _REFS = {}, {}


def scene(name):
    if name not in _SCENES:
        ncls, nb, nr, size, res, n = SCENES[name]
        cfg = synth.Config("init_" + name, N_PTS, ncls, nb, nr, size, n, seed=4100 + sum(map(ord, name)), res=res)
        sc = synth.make_scene(cfg)
        _SCENES[name] = (cfg, sc)
    return _SCENES[name]


def states(name, mode):
    cfg, sc = scene(name)
    n, size = cfg.n_particles, cfg.map_size
    rng = np.random.default_rng(77 + sum(map(ord, name + mode)))
    st = synth.make_particles(cfg, sc.lab, sc.pose, rng, n=n)
    st["have_init"] = 0
    st["theta"] = rng.uniform(-3, 3, n).astype(np.float32)
    st["dx_m"] = rng.normal(0, 2, n).astype(np.float32)
    st["dy_m"] = rng.normal(0, 2, n).astype(np.float32)
    st["init_x_px"][:4] = np.asarray([-3 * size, 4 * size, 0.5 * size, -40], np.float32)
    st["init_y_px"][:4] = np.asarray([0.5 * size, 4 * size, -2 * size, -40], np.float32)
    st["init_x_px"][4:10] = np.asarray([1, size - 2, 0.4 * size, 0.6 * size, 3, size - 3], np.float32)
    st["init_y_px"][4:10] = np.asarray([0.3 * size, 0.7 * size, 1, size - 2, 3, size - 3], np.float32)
    st["dx_m"][:10] = 0
    st["dy_m"][:10] = 0
    st["have_init"][10:20] = 1
    if n > 128:
        st["have_init"][64:128] = 1
    if mode == "pscale":
        st["scale"] = rng.uniform(0.3, 12.0, n).astype(np.float32)
        st["scale"][20:26] = np.asarray([0.3, 0.79, 0.8, 10.0, 10.5, 12.0], np.float32)
    else:
        st["scale"] = 1.0
    return st


def scan(oracle, name, var):
    """var: plain | c2048 | c2049 | sum2200 — one bin of the outer ring holds a class count of exactly 2048 (exact in f16),
    of 2049 (not), or two classes at 1100 (each exact, their sum — the slot the normalisation reads — not)."""
    cfg, sc = scene(name)
    s = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr).copy()
    assert s.max() <= 1000 and s.sum(0).max() <= 1000
    if var != "plain":
        b = cfg.nb * (cfg.nr - 2) + cfg.nb // 3
        s[:, b] = 0
        if var == "sum2200":
            s[0, b] = s[cfg.ncls - 1, b] = 1100
        else:
            s[min(2, cfg.ncls - 1), b] = {"c2048": 2048, "c2049": 2049}[var]
    return s


def weights(ncls, kind, k=1.0):
    base = {"w": W_UNEQUAL, "w2": W_SECOND, "unit": [1.3] * 15}[kind]
    return [float(np.float32(x * k)) for x in base[:ncls]]


def params(ncls, mode, kind, k=1.0):
    return dict(fixed_scale=-1.0 if mode == "pscale" else 1.0, class_weights=weights(ncls, kind, k), regularization=0.7,
                force_on_map=mode == "pscale")


def reference(oracle, name, mode="fixed", var="plain", kind="w", k=1.0, st=None):
    """dict: cfg, sc, st (the states before), scan, params, search (init_exact_ref.Search), raw_o / st_o (the oracle's
    weights and states after its own search).  st: other states than the scene's (not cached)."""
    key = (name, mode, var, kind, k) if st is None else None
    if key not in _REFS:
        cfg, sc = scene(name)
        st = states(name, mode) if st is None else st
        s, pr = scan(oracle, name, var), params(cfg.ncls, mode, kind, k)
        fpo = oracle.make_params(cfg.ncls, **pr)
        tab = oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res, 1.0)
        search = X.Search(oracle, sc.class_maps, sc.class_mask, 1.0, tab, cfg.nb, cfg.nr, s, cfg.res, fpo, st)
        st_o = st.copy()
        om = oracle.OracleMap(sc.class_maps, sc.class_mask, 1.0)
        raw_o = oracle.compute_weights(om, tab, cfg.nb, cfg.nr, s, cfg.res, fpo, st_o)
        out = dict(cfg=cfg, sc=sc, st=st, scan=s, params=pr, search=search, raw_o=raw_o, st_o=st_o, om=om, tab=tab, fpo=fpo)
        if key is None:
            return out
        _REFS[key] = out
    return _REFS[key]


def row(name, scene, slot, mode="fixed", us=False, kind="w", k=1.0, var="plain", fallback=False, mfma=1, rec16_min=BIG,
        ahead=1):
    return dict(name=name, scene=scene, slot=slot, mode=mode, us=us, kind=kind, k=k, var=var, fallback=fallback, mfma=mfma,
                rec16_min=rec16_min, ahead=ahead)


def _rows():
    R = []
    # ---- half records (rec16_min = 0): score_init_half_kernel<USCALE, AHEAD>, half_records_kernel<4 | 8>
    h = lambda name, sc, **kw: R.append(row("half_" + name, sc, HALF, rec16_min=0, **kw))
    h("6cls_kslot", "c6")
    h("6cls_unitw_uscale", "c6", kind="unit", us=True)
    h("7cls_seven_uscale", "c7", us=True)
    h("7cls_unitw", "c7", kind="unit")
    h("3cls_rec4", "c3")
    h("3cls_unitw_uscale", "c3", kind="unit", us=True)
    h("1cls_rec4", "c1", kind="unit")
    h("particle_scales", "c6", mode="pscale")
    for a in (1, 2, 3):
        h(f"ahead{a}_129x7", "c6_129x7", ahead=a, us=a == 2)
    h("ahead3_129x7_particle_scales", "c6_129x7", ahead=3, mode="pscale")
    h("nb36_3cls_first_of_class", "c3_36x7")
    h("nb36_6cls_first_of_class_uscale", "c6_36x7", us=True)
    h("nb36_ahead3", "c6_36x7", ahead=3)
    h("nb8_tie_across_lanes", "c6_8x16")
    h("100x25_node_defaults", "c6_100x25", us=True)
    h("weights_x_2^-10", "c6", k=2.0 ** -10)
    h("weights_x_2^10", "c6", k=2.0 ** 10)
    # ---- on the fly: score_init_mfma_kernel<USCALE, UNITW, SEVEN>, all eight
    for us in (False, True):
        for kind in ("w", "unit"):
            for sc in ("c6", "c7"):
                R.append(row(f"split_{'uscale' if us else 'scale'}_{'unitw' if kind == 'unit' else 'weights'}_"
                             f"{'seven' if sc == 'c7' else 'kslot'}", sc, SPLIT, us=us, kind=kind))
    R.append(row("split_particle_scales", "c6", SPLIT, mode="pscale"))
    R.append(row("split_nb36_first_of_class", "c6_36x7", SPLIT))
    R.append(row("split_nb8_tie_across_lanes", "c6_8x16", SPLIT))
    R.append(row("split_nb512_half_lds_does_not_fit", "c6_512x4", SPLIT, rec16_min=0))
    R.append(row("split_weights_x_2^-10", "c6", SPLIT, k=2.0 ** -10))
    R.append(row("split_weights_x_2^10", "c6", SPLIT, k=2.0 ** 10))
    # ---- wide records: score_init_mfma_wide_kernel<3 | 4, USCALE>
    R.append(row("wide_8cls_rec12_spare_uscale", "c8", WIDE, us=True))
    R.append(row("wide_11cls_rec12", "c11", WIDE))
    R.append(row("wide_12cls_rec16", "c12", WIDE))
    R.append(row("wide_15cls_rec16_uscale", "c15", WIDE, us=True))
    R.append(row("wide_8cls_particle_scales", "c8", WIDE, mode="pscale"))
    R.append(row("wide_nb8_tie_across_lanes", "c11_8x16", WIDE))
    R.append(row("wide_15cls_rec16", "c15", WIDE))
    R.append(row("wide_11cls_rec12_uscale", "c11", WIDE, us=True))
    R.append(row("wide_12cls_rec16_uscale", "c12", WIDE, us=True))
    # ---- vector kernel (init_mfma 0): score_init_kernel<NV4, KSLOT, USCALE>, all sixteen
    for sc in ("c2", "c3", "c6", "c7", "c8", "c11", "c12", "c15"):
        for us in (False, True):
            R.append(row(f"vector_{sc}_{'uscale' if us else 'scale'}", sc, VECTOR, us=us, mfma=0))
    R.append(row("vector_particle_scales", "c6", VECTOR, mode="pscale", mfma=0))
    R.append(row("vector_nb36_first_of_class", "c6_36x7", VECTOR, mfma=0))
    R.append(row("vector_nb8_first_of_class", "c6_8x16", VECTOR, mfma=0))
    R.append(row("vector_default_route_rec4_without_half_records", "c3", VECTOR))
    # ---- fallback: a count of 2048 stays on the matrix cores, 2049 and a sum above 2048 go back to the vector kernel
    for pname, sc, slot, r16 in (("half", "c6", HALF, 0), ("split", "c6", SPLIT, BIG), ("wide", "c11", WIDE, BIG)):
        R.append(row(f"fallback_{pname}_count_2048_stays", sc, slot, var="c2048", rec16_min=r16))
        R.append(row(f"fallback_{pname}_count_2049", sc, slot, var="c2049", rec16_min=r16, fallback=True))
        R.append(row(f"fallback_{pname}_sum_slot_alone", sc, slot, var="sum2200", rec16_min=r16, fallback=True))
    return R


ROWS = _rows()
assert len({r["name"] for r in ROWS}) == len(ROWS)
# the batched search (tdr_batch_step with batch_init_search): filter -> particles, weights, scan
BATCH = [(100, "w", "plain"), (200, "w2", "plain"), (200, "w", "c2049")]
BATCH_SCENE, BATCH_REC16_MIN = "c6", 128
REF_KEYS = sorted({(r["scene"], r["mode"], r["var"], r["kind"], r["k"]) for r in ROWS} |
                  {(BATCH_SCENE, "fixed", var, kind, 1.0) for _, kind, var in BATCH})
