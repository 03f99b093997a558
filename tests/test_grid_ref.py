"""CPU-only: the NumPy restatement of the pose-grid search (tests/grid_ref.py; include/tdr.h, "pose-grid search") against
hand-worked cases, and the signal the feature rests on: the CPU oracle's weights over a road lattice of synth's c1 scene
put the top peak on the true pose, for the scene's first scan and for the kidnapped robot's."""
import functools

import numpy as np
import pytest

import grid_ref as GR
from test_recovery_ref import hand_map

F32 = np.float32
NAN = float("nan")


def _bits(a):
    return np.asarray(a, F32).view(np.uint32)


# ---- the list ------------------------------------------------------------------------------------------------------------------------
def test_list_on_the_hand_map():
    """The 5 x 5 map with road on (row, col) (0, 3), (2, 1), (4, 4).  A 4 x 4 lattice from (-1, -1) at step 2 stands on
    columns and rows -1, 1, 3, 5: the four points on cells (1, 1), (1, 3), (3, 1), (3, 3) are inside, none of them on road."""
    maps = hand_map()
    sp = GR.Spec(-1, -1, 2, 4, 4, road_only=0)
    assert GR.lattice_list(maps, sp).tolist() == [5, 6, 9, 10]
    assert GR.lattice_list(maps, sp._replace(road_only=1)).tolist() == []
    c, r = GR.cells(sp)
    assert (c[6], r[6]) == (3, 1) and (c[15], r[15]) == (5, 5) and (c[0], r[0]) == (-1, -1)
    # rows 0, 2, 4, 6: cells (0, 1), (0, 3) road, (2, 1) road, (2, 3), (4, 1), (4, 3) are inside; row 6 is not
    sp2 = GR.Spec(-1, 0, 2, 4, 4, road_only=0)
    assert GR.lattice_list(maps, sp2).tolist() == [1, 2, 5, 6, 9, 10]
    assert GR.lattice_list(maps, sp2._replace(road_only=1)).tolist() == [2, 5]
    # step 1 over the whole map is the road list
    sp3 = GR.Spec(0, 0, 1, 5, 5, road_only=1)
    assert GR.lattice_list(maps, sp3).tolist() == [3, 11, 24]
    assert GR.lattice_list(maps, GR.Spec(7, 7, 1, 3, 3, road_only=0)).tolist() == []      # wholly outside


# ---- the candidates --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [1.0, 2.0])
def test_candidate_fields(res):
    sp = GR.Spec(-1, 0, 2, 4, 4, road_only=1, heading_mode=1, n_headings=3, theta0=-1.0, dtheta=0.25, scale=1.5)
    lst = np.array([2, 5], np.int32)                       # cells (row 0, col 3) and (row 2, col 1)
    cand = GR.candidates(sp, lst, res)
    assert cand.shape == (2, 3)
    assert cand["init_x_px"][:, 0].tolist() == [3.5 * res, 1.5 * res] and cand["init_y_px"][:, 0].tolist() == [0.5 * res, 2.5 * res]
    assert (cand["init_x_px"] == cand["init_x_px"][:, :1]).all() and (cand["init_y_px"] == cand["init_y_px"][:, :1]).all()
    assert cand["theta"][1].tolist() == [-1.0, -0.75, -0.5] and (cand["have_init"] == 1).all()
    assert (cand["dx_m"] == 0).all() and (cand["dy_m"] == 0).all() and (cand["scale"] == F32(1.5)).all()
    none = GR.candidates(sp._replace(heading_mode=0, n_headings=1), lst, res)
    assert none.shape == (2, 1) and (none["theta"] == 0).all() and (none["have_init"] == 0).all()
    # float32 at every step: theta_h = theta0 + (float)h * dtheta
    odd = GR.candidates(sp._replace(theta0=0.1, dtheta=0.3, n_headings=5), lst, res)
    assert _bits(odd["theta"][0]).tolist() == _bits([F32(0.1) + F32(h) * F32(0.3) for h in range(5)]).tolist()


# ---- the reduction ---------------------------------------------------------------------------------------------------------------------
def test_reduction_over_three_headings():
    sp = GR.Spec(0, 0, 1, 3, 2, road_only=0, heading_mode=1, n_headings=3, theta0=0.5, dtheta=1.0)
    lst = np.array([0, 2, 3, 5], np.int32)
    w = np.array([[NAN, 2.0, 1.0],        # a NaN loses to any number
                  [0.0, NAN, 0.0],        # a 0 beats a NaN; the first 0
                  [4.0, 7.0, 7.0],        # a tie: the smaller h
                  [NAN, NAN, NAN]], F32)  # all NaN: h = 0, and W is that NaN
    after = GR.candidates(sp, lst, 1.0)
    after["have_init"][1, 0] = 0           # scoring left this pick without a heading
    W, T, vol = GR.reduce(sp, lst, w, after)
    assert GR.pick(w).tolist() == [1, 0, 1, 0]
    assert W[[0, 2, 3]].tolist() == [2.0, 0.0, 7.0] and np.isnan(W[[1, 4, 5]]).all()
    assert T[[0, 3, 5]].tolist() == [1.5, 1.5, 0.5] and np.isnan(T[[1, 2, 4]]).all()
    assert _bits(W[[1, 4]]).tolist() == [0x7FC00000] * 2 and _bits(T[[1, 2, 4]]).tolist() == [0x7FC00000] * 3
    assert vol.shape == (3, 6) and _bits(vol[:, lst]).tolist() == _bits(w.T).tolist() and np.isnan(vol[:, [1, 4]]).all()


# ---- the peaks -------------------------------------------------------------------------------------------------------------------------
PLANE = np.array([[1.0, 5.0, 5.0, 0.0, 2.0],          # a two-cell plateau (g = 1, 2), a 0
                  [1.0, 1.0, 1.0, NAN, 2.5],          # a NaN
                  [3.0, 1.0, 1.0, 1.0, 1.0],
                  [1.0, 1.0, -4.0, 1.0, 4.0]], F32)   # a negative value


def _peaks(R, K):
    sp = GR.Spec(10, 20, 3, 5, 4, road_only=0)
    T = np.arange(20, dtype=F32)
    return GR.peaks(sp, 100, PLANE.ravel(), T, R, K)


def test_peaks_on_the_hand_plane():
    pk, n = _peaks(0, 4096)                                # R = 0: every eligible point
    assert n == 17 and len(pk) == 17 and pk["g"][:5].tolist() == [1, 2, 19, 10, 9]
    pk, n = _peaks(1, 4096)
    assert n == 4 and pk["g"].tolist() == [1, 19, 10, 9] and pk["w"].tolist() == [5.0, 4.0, 3.0, 2.5]
    # cell = r * cols + c with c = 10 + 3 ix, r = 20 + 3 iy; theta is T[g]
    assert pk["cell"].tolist() == [20 * 100 + 13, 29 * 100 + 22, 26 * 100 + 10, 23 * 100 + 22]
    assert pk["theta"].tolist() == [1.0, 19.0, 10.0, 9.0]
    pk, n = _peaks(1, 2)                                   # K below the peak count
    assert n == 4 and pk["g"].tolist() == [1, 19]
    pk, n = _peaks(2, 7)                                   # R = 2: (3, 4) = 4.0 covers 2.5; 3.0 stands two columns from 5.0
    assert n == 2 and pk["g"].tolist() == [1, 19]
    pk, n = _peaks(2, 0)
    assert n == 2 and len(pk) == 0
    flat = GR.peaks(GR.Spec(0, 0, 1, 5, 4, road_only=0), 9, np.full(20, 2.0, F32), np.zeros(20, F32), 16, 8)
    assert flat[1] == 1 and flat[0]["g"].tolist() == [0]   # a plateau has exactly one peak: its smallest g
    none = GR.peaks(GR.Spec(0, 0, 1, 5, 4, road_only=0), 9, np.full(20, NAN, F32), np.zeros(20, F32), 1, 8)
    assert none[1] == 0 and len(none[0]) == 0


# ---- the signal: the oracle's weights over a road lattice of c1 ----------------------------------------------------------------------
BASIN_PX = 12.0          # the basin width of DESIGN.md 5.17
C1_STEP = 8


@functools.lru_cache(maxsize=None)
def c1_scene():
    """synth's c1 scene and the kidnapped robot's pose and scan, built as tests/test_recovery.py::kidnap_run builds them."""
    from top_down_renderer_amd import synth
    sc = synth.make_scene("c1", n_particles=4000)
    rng = np.random.default_rng(77)
    while True:
        pose2 = synth.pick_true_pose(sc.lab, rng, 168)
        if np.hypot(pose2[0] - sc.pose[0], pose2[1] - sc.pose[1]) >= 400:
            break
    pts2 = synth.make_scan(sc.cfg, sc.lab, pose2, rng)
    return sc, pose2, pts2


def c1_spec(step=C1_STEP):
    """Every step-th cell of the 1000 x 1000 map from offset step // 2, road cells only, no heading."""
    n = (1000 - step // 2 + step - 1) // step
    return GR.Spec(step // 2, step // 2, step, n, n, road_only=1, heading_mode=0, n_headings=1, scale=1.0)


@functools.lru_cache(maxsize=None)
def c1_oracle_search(which):
    """The restatement over the CPU oracle's weights (its own 40-rotation search): `which` = "first" or "kidnapped".
    Computed once for the tests that need it."""
    from oracle import c_oracle as oracle
    oracle.build()
    sc, pose2, pts2 = c1_scene()
    cfg = sc.cfg
    pts, pose = (sc.pts, sc.pose) if which == "first" else (pts2, pose2)
    om = oracle.OracleMap(sc.class_maps, sc.class_mask, cfg.map_resolution)
    fp = oracle.make_params(cfg.ncls, fixed_scale=1.0)
    scan = oracle.raster_polar(pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
    tab = oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res, cfg.map_resolution)

    def score(cand):
        st = np.ascontiguousarray(cand.astype(oracle.STATE_DTYPE))
        w = np.asarray(oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan, cfg.res, fp, st), F32)
        return w, st
    W, T, vol, pk, n_peaks, lst = GR.grid_search(sc.class_maps, cfg.map_resolution, c1_spec(), score, 2, 4096)
    return pose, W, T, pk, n_peaks, lst


def peak_distance(peak, pose, cols=1000, resolution=1.0):
    r, c = divmod(int(peak["cell"]), cols)
    return float(np.hypot((c + 0.5) * resolution - pose[0], (r + 0.5) * resolution - pose[1]))


@pytest.mark.parametrize("which", ["first", "kidnapped"])
def test_the_oracles_top_peak_is_the_true_pose(which):
    """Measured with the CPU oracle: 3324 candidates; first scan: best weight 6.0956, 7.0 px from the true pose, the best
    other peak 5.9981 (a gap of 1.6e-2 of the top weight); kidnapped scan: 6.5135, 3.2 px, 6.2102 (4.7e-2)."""
    pose, W, T, pk, n_peaks, lst = c1_oracle_search(which)
    d = peak_distance(pk[0], pose)
    gap = (float(pk["w"][0]) - float(pk["w"][1])) / float(pk["w"][0])
    print(f"{which}: listed {len(lst)}, peaks {n_peaks}, top {pk['w'][0]:.4f} at {d:.1f} px, next {pk['w'][1]:.4f}, gap {gap:.2e}")
    assert len(lst) == 3324 and n_peaks >= 2
    assert d < BASIN_PX
    assert gap > 1e-3
