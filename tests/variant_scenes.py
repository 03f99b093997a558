"""The launches of tests/test_loop_variants.py (GPU) and tests/test_variant_scenes_ref.py (CPU): one scene per LOOP VARIANT of
the two dense scoring kernels, each scored with the scans of tests/int_form_cases.py whose form is "integer".  Not a test
module.

score_polar_su_kernel (csrc/tdr_score_su.hip) picks per wave, ring group and sector of directions: the workgroup's staged
box (H x Wb <= SU_BOX_WORDS = 4096 mask words) or, where that does not fit, the wave's own box in a quarter of the area
(<= 1024 words), each with the loop for "every cell known" / "every cell inside the map" / general; or the far path.
score_cart_su_kernel (csrc/tdr_score_cart.hip) picks per wave, group of 8 window columns and segment of cart_seg_rows
window rows: all known / inside / general, or the plain steps where the box exceeds CART_SU_WBOX = 1024 words.  The
kernels count what they picked (tdr_profile_enable(2), tdr_profile_variants); SCENES names the counter each scene is for.

Geometry (mask words are 32 columns wide; particles go to waves in Morton order of their half-cells, the top bit of a
coordinate flips at cell 512; the polar window's ring j has radius j * res, so ring 0 is the particle's own cell):
  * workgroup's box: 256 particles of ONE heading within +-4 cells of a point.  All known: a map without unknown cells, the
    point in the middle.  Inside: the same with an unknown cell at every third row and column — every box is at least 3
    rows high and 3 columns wide, so none is all known.  General: the point 0.2 .. 0.8 cells from the left border, so that
    the boxes of every sector that looks left, and of the first ring group in every sector, reach the guard ring; the
    sectors that look right see known cells only in the later ring groups (the scene ADMITS the all-known counter);
  * the wave's own box: four such clusters of 64, 500 cells apart on an 800 x 800 map: the workgroup's box has more than
    8000 words, each wave's a few dozen;
  * far: each wave's 64 particles on a jittered 8 x 8 grid over its own quarter of the map, 260 .. 300 cells wide: more than
    2000 words per wave.  With a NaN: one particle's x is NaN — its wave's box is the whole map;
  * Cartesian: the same three maps with a cluster of small heading spread; plain steps: scales of 6 .. 9 and centres spread
    over 400 x 400 cells, a segment's box then has far more than 1024 words; a window of 20 columns has a partial last
    column group (two whole groups of 8, then 4 columns in plain C++).
Particle 0 of every clustered scene sits at the cluster's nominal centre, and the centres are where its window serves
int_form_cases._past_2p53 (cells at 1, at sqrt 2 and far whole distances of one class).
"""
import ctypes as C

import numpy as np

from top_down_renderer_amd import synth

import int_form_cases as T

NCLS = T.NCLS
# scan -> (builder's name in int_form_cases, map, polar (nb, nr), Cartesian (rows, cols))
SCANS = {
    "ladder": ("ladder", "scene", (64, 24), (64, 24)),
    "multi": ("multi", "scene", (48, 20), (48, 24)),
    "all_listed": ("all_listed", "scene", (48, 20), (48, 24)),
    "past_2p53": ("past_2p53", "scene", (48, 20), (48, 24)),
    "mass_below": ("mass_below", "dict_edge", (48, 20), (48, 24)),
}
# scene -> kind, particles, map size, unknown cells, counter of tdr_profile_variants the scene is for, counters it admits
# beside it (empty: a pure scene), whether no window may see an unknown cell
SCENES = {
    "wg_all_known": dict(kind="polar", n=256, size=200, holes=False, where="middle", target=0, admits=(), all_known=True),
    "wg_inside": dict(kind="polar", n=256, size=200, holes=True, where="middle", target=1, admits=(), all_known=False),
    "wg_general": dict(kind="polar", n=256, size=200, holes=False, where="border", target=2, admits=(0,), all_known=False),
    "wave_all_known": dict(kind="polar", n=256, size=800, holes=False, where="four", target=3, admits=(), all_known=True),
    "wave_inside": dict(kind="polar", n=256, size=800, holes=True, where="four", target=4, admits=(), all_known=False),
    "wave_general": dict(kind="polar", n=256, size=800, holes=False, where="four borders", target=5, admits=(3,),
                         all_known=False),
    "far": dict(kind="polar", n=256, size=800, holes=True, where="spread", target=6, admits=(), all_known=False),
    "far_nan": dict(kind="polar", n=256, size=800, holes=True, where="spread nan", target=6, admits=(), all_known=False),
    "ragged_wave": dict(kind="polar", n=200, size=200, holes=True, where="middle", target=1, admits=(), all_known=False),
    "cart_all_known": dict(kind="cart", n=256, size=200, holes=False, where="middle", target=8, admits=(), all_known=True),
    "cart_inside": dict(kind="cart", n=256, size=200, holes=True, where="middle", target=9, admits=(), all_known=False),
    "cart_general": dict(kind="cart", n=256, size=200, holes=False, where="border", target=10, admits=(8,),
                         all_known=False),
    "cart_plain_steps": dict(kind="cart", n=256, size=800, holes=True, where="large", target=11, admits=(), all_known=False),
    "cart_partial_group": dict(kind="cart", n=256, size=200, holes=True, where="middle", target=9, admits=(),
                               all_known=False, shape=(48, 20)),
}
POLAR_COUNTERS, CART_COUNTERS = tuple(range(0, 7)), tuple(range(8, 12))
NAN_PARTICLE = 10
CASES = [(scene, scan) for scene in SCENES for scan in SCANS]


def counted(k, launch):
    """launch() with the kernels' variant counters on (k: HipKernels): (its result, the 16 counters of the launches in it)."""
    v = (C.c_int64 * 16)()
    try:
        k.lib.tdr_profile_enable(2)
        assert k.lib.tdr_profile_variants(v) == 0     # (reading resets)
        out = launch()
        assert k.lib.tdr_profile_variants(v) == 0
    finally:
        k.lib.tdr_profile_enable(0)
    return out, [int(x) for x in v]


_MAPS = {}


def _maps(size, map_name, holes):
    """Distance maps of a label image without unlabelled cells ("scene") or the hand-made dictionary map whose largest
    integer is just below 2^32 ("dict_edge"); holes: an unknown cell (value 0, mask 1) at every third row and column."""
    key = (size, map_name, holes)
    if key not in _MAPS:
        rng = np.random.default_rng(8100 + size)
        if map_name == "scene":
            lab = synth.make_label_image(size, NCLS, rng)
            lab[lab < 0] = 0
            maps, _ = synth.label_to_maps(lab, NCLS, 1.0)
        else:
            maps, _ = T._dict_map(rng, size, T.DICT_TOP)
        maps = maps.copy()
        mask = np.zeros((size, size), np.uint8)
        if holes:
            mask[1::3, 1::3] = 1
        maps[:, mask == 1] = 0
        maps.setflags(write=False)
        mask.setflags(write=False)
        _MAPS[key] = (maps, mask)
    return _MAPS[key]


def _grid64(rng, xs, ys):
    """64 coordinate pairs on a jittered 8 x 8 grid over the rectangle xs x ys: their bounding box is nearly all of it."""
    gx, gy = np.meshgrid(np.linspace(*xs, 8), np.linspace(*ys, 8))
    return (gx.ravel() + rng.uniform(-2, 2, 64)).astype(np.float32), (gy.ravel() + rng.uniform(-2, 2, 64)).astype(np.float32)


def _particles(sc, rng, nb):
    n, size, where = sc["n"], sc["size"], sc["where"]
    st = np.zeros(n, synth.STATE_DTYPE)
    st["scale"] = 1.0
    st["have_init"] = 1
    near = lambda c, k: (c + rng.normal(0.0, 1.5, k).clip(-4.0, 4.0)).astype(np.float32)
    edge = lambda k: rng.uniform(0.2, 0.8, k).astype(np.float32)
    # (particle 0 sits at the cluster's nominal centre: int_form_cases._past_2p53 makes its scan from that particle's
    # window, which must hold cells at 1, at sqrt 2 and far ones of one class; the centres are chosen for that)
    mid = size / 2 + 0.25
    if sc["kind"] == "polar":
        st["theta"] = np.float32(2 * np.pi * 5 / nb)            # one heading bin: shift 5
        if where == "middle":
            st["init_x_px"], st["init_y_px"] = near(mid, n), near(mid, n)
        elif where == "border":
            st["init_x_px"], st["init_y_px"] = edge(n), near(110.25, n)
        elif where in ("four", "four borders"):
            for w, (qx, qy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
                s = slice(64 * w, 64 * w + 64)
                if where == "four":
                    st["init_x_px"][s] = near(150.25 + 500 * qx, 64)
                else:                                             # left and right border: the workgroup's box spans the map
                    st["init_x_px"][s] = edge(64) if qx == 0 else size - 1 + 0.45 - edge(64)
                st["init_y_px"][s] = near((150.25 if where == "four" else 100.25) + 500 * qy, 64)
        else:                                                     # spread: a quarter of the map per wave
            for w, (qx, qy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
                s = slice(64 * w, 64 * w + 64)
                span = lambda q: (100.0, 400.0) if q == 0 else (520.0, 780.0)
                st["init_x_px"][s], st["init_y_px"][s] = _grid64(rng, span(qx), span(qy))
            if where == "spread nan":
                st["init_x_px"][NAN_PARTICLE] = np.nan
        if "spread" not in where:
            st["init_x_px"][0] = 0.5 if "border" in where else (mid if where == "middle" else 150.25)
            st["init_y_px"][0] = {"middle": mid, "border": 110.25, "four": 150.25, "four borders": 100.25}[where]
        return st
    if where == "large":
        st["init_x_px"] = rng.uniform(200, 600, n).astype(np.float32)
        st["init_y_px"] = rng.uniform(200, 600, n).astype(np.float32)
        st["theta"] = rng.uniform(-np.pi, np.pi, n).astype(np.float32)
        st["scale"] = rng.uniform(6.0, 9.0, n).astype(np.float32)
        return st
    st["init_y_px"] = near(110.25, n)
    st["init_x_px"] = near(130.25, n) if where == "middle" else rng.uniform(2.0, 3.5, n).astype(np.float32)
    st["theta"] = rng.normal(0.05, 0.02, n).astype(np.float32)
    st["scale"] = rng.uniform(0.95, 1.05, n).astype(np.float32)
    st["init_x_px"][0], st["init_y_px"][0] = 130.25 if where == "middle" else 2.75, 110.25
    st["theta"][0], st["scale"][0] = 0.05, 1.0
    return st


_CACHE, _REF = {}, {}


def make_case(oracle, scene, scan):
    """The dict of int_form_cases.make_case for (scene, scan), with `scene`, `target`, `admits` and `all_known` beside."""
    if (scene, scan) in _CACHE:
        return _CACHE[scene, scan]
    sc = SCENES[scene]
    scan_name, map_name, shape_p, shape_c = SCANS[scan]
    polar = sc["kind"] == "polar"
    a, b = sc.get("shape", shape_p if polar else shape_c)
    res = 1.0 if polar else 0.75
    rng = np.random.default_rng(9000 + 31 * list(SCENES).index(scene) + 7 * list(SCANS).index(scan))
    maps, mask = _maps(sc["size"], map_name, sc["holes"])
    ang_res = np.float32(2 * np.pi / a)
    case = dict(name=f"{scene}-{scan}", kind=sc["kind"], form="integer", shape=(a, b), P=a * b, res=res, ang_res=ang_res,
                maps=maps, mask=mask, states=_particles(sc, rng, a), params=dict(fixed_scale=1.0),
                tab=oracle.polar_table(a, b, ang_res) if polar else None,
                scene=scene, target=sc["target"], admits=sc["admits"], all_known=sc["all_known"])
    case["scan"] = T._past_2p53(oracle, case, rng) if scan_name == "past_2p53" else T.make_scan(scan_name, rng, a * b)
    _CACHE[scene, scan] = case
    return case


def references(oracle, scene, scan):
    """(case, exact reference weights, oracle weights): computed once, shared, never written to."""
    if (scene, scan) not in _REF:
        case = make_case(oracle, scene, scan)
        with np.errstate(all="ignore"):
            exact, orc = T.exact_weights(oracle, case), T.oracle_weights(oracle, case)
        exact.setflags(write=False)
        orc.setflags(write=False)
        _REF[scene, scan] = (case, exact, orc)
    return _REF[scene, scan]
