"""Cartesian filters through the C handle (tdr_filter_create_cart, csrc/tdr_host_filter.cpp) and through the Python
ParticleFilter: both sequence the heading search (tdr_k_score_cart_init) and tdr_k_score_cart into the same step, so they
end with the same bytes; a cold start initialises every heading, checked against the CPU oracle under the rules of
tests/cart_ref.py; what a Cartesian filter refuses is refused without changing it; and a scan rendered from a known pose
localises."""
import ctypes as C

import numpy as np
import pytest
from cart_ref import CASES, check_search, make_case, oracle_candidate_weights

from top_down_renderer_amd import synth


@pytest.fixture(scope="module")
def tdr():
    import torch
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd.kernels import HipKernels
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pkg, HipKernels()


def images(flat, rows, cols):
    """[ncls][rows*cols] column-major images (the oracle's raster) -> (ncls, rows, cols) arrays."""
    return np.ascontiguousarray(flat.reshape(len(flat), cols, rows).transpose(0, 2, 1))


@pytest.fixture(scope="module")
def scene(tdr, oracle):
    """Case c6_32x24 of tests/cart_ref.py on a MapHandle with that window and on a Python TopDownMap."""
    from top_down_renderer_amd import batch
    pkg, k = tdr
    name = "c6_32x24"
    ncls, rows, cols, _ = CASES[name]
    cfg, lab, maps, mask, pose, pts, st = make_case(name)
    scan = oracle.raster_cart(pts, cfg.res, synth.make_lut(ncls), ncls, rows, cols)
    mh = batch.MapHandle(maps, mask, 1.0)
    mh.set_window(rows, cols)
    m = pkg.TopDownMap(pkg.Params(resolution=1.0), maps, mask, kernels=k)
    m.setWindow(rows, cols)
    st.setflags(write=False)
    return dict(cfg=cfg, maps=maps, mask=mask, pts=pts, st=st, scan=scan, mh=mh, m=m, rows=rows, cols=cols, ncls=ncls)


@pytest.mark.gpu
def test_handle_and_python_filters_end_with_identical_bytes(tdr, scene):
    """Same Cartesian map, seed and scans; a cold start for half the particles; four propagate + update steps, the last
    two with another particle count: states, raw weights, weights and resample indices are the same bytes."""
    from top_down_renderer_amd import batch
    pkg, k = tdr
    s = scene
    rows, cols = s["rows"], s["cols"]
    st = s["st"][2:].copy()                    # (without the two particles whose windows are mostly off the map)
    st["have_init"][::2] = 0
    st["theta"][::2] = 0
    params = pkg.FilterParams(fixed_scale=-1.0)          # every particle keeps its own scale
    h = batch.FilterHandle(s["mh"], len(st) + 40, params, seed=11, cart=True)
    h.set_states(st)
    f = pkg.ParticleFilter(len(st) + 40, s["m"], params, seed=11, kernels=k, init_particles=False)
    f.set_states(st)
    rng = np.random.default_rng(2)
    for step, n_target in enumerate((-1, -1, len(st) + 40, 150)):
        scan = s["scan"] + (rng.integers(0, 8, s["scan"].shape) == 0) * step     # another integer scan every step
        scan = np.ascontiguousarray(scan, np.float32)
        n = h.num_particles()
        h.propagate(0.4, 0.1 * step, 0.02)
        f.propagate((0.4, 0.1 * step), 0.02)
        h.update(images(scan, rows, cols), s["cfg"].res, n_target)
        f.update(scan, None, s["cfg"].res, n_target=None if n_target < 0 else n_target)
        assert h.num_particles() == f.numParticles()
        assert h.raw_weights(n).tobytes() == f.raw_weights().tobytes(), step
        assert h._floats(h.L.tdr_filter_get_weights, n).tobytes() == f.weights().tobytes(), step
        assert np.array_equal(h.resample_indices(), f.resample_indices()), step
        a, b = h.states(), f.get_states()
        for name in ("init_x_px", "init_y_px", "dx_m", "dy_m", "theta", "scale", "have_init"):
            assert a[name].tobytes() == b[name].tobytes(), (step, name)
        assert a["have_init"].all()


@pytest.mark.gpu
def test_handle_weights_are_the_same_bytes_as_the_python_filters(tdr, scene):
    """The normalised weights of an update, read before anything else happens, through both paths."""
    from top_down_renderer_amd import batch
    pkg, k = tdr
    s = scene
    st = s["st"][2:66].copy()
    params = pkg.FilterParams(fixed_scale=-1.0)
    h = batch.FilterHandle(s["mh"], len(st), params, seed=3, cart=True)
    h.set_states(st)
    f = pkg.ParticleFilter(len(st), s["m"], params, seed=3, kernels=k, init_particles=False)
    f.set_states(st)
    h.propagate(0.3, 0.0, 0.0)
    f.propagate((0.3, 0.0), 0.0)
    h.update(images(s["scan"], s["rows"], s["cols"]), s["cfg"].res)
    f.update(np.ascontiguousarray(s["scan"]), None, s["cfg"].res)
    assert h.weights().tobytes() == f.weights().tobytes()
    assert abs(float(h.weights().astype(np.float64).sum()) - 1.0) < 1e-5


@pytest.mark.gpu
def test_cold_start_initialises_every_heading_like_the_oracle(tdr, oracle, scene):
    """A filter whose particles all lack a heading: tdr_filter_compute_weights runs the search and the regular launch (no
    resampling, so the headings can be read), tdr_filter_update on a twin does the same and resamples."""
    from top_down_renderer_amd import batch
    pkg, k = tdr
    s = scene
    st = s["st"].copy()
    st["have_init"] = 0
    st["theta"] = 0
    cw = [1.0, 0.5, 2.0, 1.5, 0.25, 1.0]
    params = pkg.FilterParams(fixed_scale=-1.0, class_weights=cw)
    om = oracle.OracleMap(s["maps"], s["mask"], 1.0)
    fpo = oracle.make_params(s["ncls"], class_weights=cw)
    w40 = oracle_candidate_weights(oracle, om, s["rows"], s["cols"], s["scan"], s["cfg"].res, fpo, st)
    h = batch.FilterHandle(s["mh"], len(st), params, seed=5, cart=True)
    h.set_states(st)
    h.compute_weights(images(s["scan"], s["rows"], s["cols"]), s["cfg"].res)
    got_st, got_raw = h.states(), h.raw_weights(len(st))
    check_search(oracle, om, s["rows"], s["cols"], s["scan"], s["cfg"].res, fpo, st, w40, got_st, got_raw)
    # the same through a full update: the same raw weights, and every resampled particle has a heading
    h2 = batch.FilterHandle(s["mh"], len(st), params, seed=5, cart=True)
    h2.set_states(st)
    h2.update(images(s["scan"], s["rows"], s["cols"]), s["cfg"].res)
    assert h2.raw_weights(len(st)).tobytes() == got_raw.tobytes()
    after = h2.states()
    assert after["have_init"].all()
    assert np.array_equal(after["theta"], got_st["theta"][h2.resample_indices()])


@pytest.mark.gpu
def test_compute_weights_equals_the_stateless_launcher_bit_for_bit(tdr, scene):
    from top_down_renderer_amd import batch
    pkg, k = tdr
    s = scene
    st = s["st"].copy()
    params = pkg.FilterParams(fixed_scale=-1.0)
    h = batch.FilterHandle(s["mh"], len(st), params, seed=5, cart=True)
    h.set_states(st)
    h.compute_weights(images(s["scan"], s["rows"], s["cols"]), s["cfg"].res)
    dev = k.zeros((7, len(st)))
    k.states_to_device(st, dev, len(st))
    raw = k.zeros((len(st),))
    k.score_cart(s["m"].dev, s["m"].scan_handle(np.ascontiguousarray(s["scan"])), s["rows"], s["cols"], s["cfg"].res,
                 params.to_c(s["ncls"]), dev, len(st), raw, n_total=len(st))
    k.synchronize()
    assert h.raw_weights(len(st)).tobytes() == raw.cpu().numpy().tobytes()
    # ... and from the renderer's Cartesian render, without host images
    r = batch.Renderer(synth.make_lut(s["ncls"]))
    r.render_cart(s["pts"], 4, 3, s["cfg"].res, s["ncls"], s["rows"], s["cols"])
    h.compute_weights(r, s["cfg"].res)
    assert h.raw_weights(len(st)).tobytes() == raw.cpu().numpy().tobytes()


@pytest.mark.gpu
def test_what_a_cartesian_filter_refuses_leaves_it_unchanged(tdr, scene):
    from top_down_renderer_amd import _lib, batch
    pkg, k = tdr
    s = scene
    L = _lib.load()
    st = s["st"][2:50].copy()
    params = pkg.FilterParams(fixed_scale=-1.0)
    fp = params.to_c(s["ncls"])
    # a map without a window has no Cartesian filter
    bare = batch.MapHandle(s["maps"], s["mask"], 1.0)
    out = C.c_void_p()
    assert L.tdr_filter_create_cart(bare.h, 10, C.byref(fp), 1, C.byref(out)) == -1 and not out.value
    assert b"window" in L.tdr_last_error()
    assert L.tdr_map_set_window(bare.h, 0, 4) == -1
    rows, cols = C.c_int(-1), C.c_int(-1)
    assert L.tdr_map_window_shape(bare.h, C.byref(rows), C.byref(cols)) == 0 and (rows.value, cols.value) == (0, 0)
    assert L.tdr_map_window_shape(s["mh"].h, C.byref(rows), C.byref(cols)) == 0
    assert (rows.value, cols.value) == (s["rows"], s["cols"])

    h = batch.FilterHandle(s["mh"], len(st), params, seed=9, cart=True)
    h.set_states(st)
    before = h.states().tobytes()
    imgs = np.ascontiguousarray(images(s["scan"], s["rows"], s["cols"]).transpose(0, 2, 1))
    geo = np.zeros((2, s["rows"] * s["cols"]), np.float32)
    assert L.tdr_filter_update_geo(h.h, imgs.ctypes.data_as(C.c_void_p), geo.ctypes.data_as(C.c_void_p), C.c_float(1.0),
                                   -1) == -1
    assert b"Cartesian" in L.tdr_last_error()
    # in a batch: refused before any filter moves, also next to a polar filter of the same map
    s["mh"].sample_pts_polar(16, 8, np.float32(2 * np.pi / 16))
    polar = batch.FilterHandle(s["mh"], len(st), params, seed=9)
    polar.set_states(st)
    polar_before = polar.states().tobytes()
    with pytest.raises(_lib.TdrError, match="Cartesian"):
        batch.step_batch([polar, h], [np.zeros((s["ncls"], 16, 8), np.float32), images(s["scan"], s["rows"], s["cols"])],
                         1.0, [(0.1, 0.0, 0.0)] * 2)
    assert polar.states().tobytes() == polar_before
    # a polar render is not a Cartesian scan, whatever its shape
    r = batch.Renderer(synth.make_lut(s["ncls"]))
    r.render_polar(s["pts"], 4, 3, s["cfg"].res, np.float32(2 * np.pi / s["rows"]), s["ncls"], s["rows"], s["cols"])
    with pytest.raises(_lib.TdrError, match="Cartesian"):
        h.update(r, s["cfg"].res)
    assert h.states().tobytes() == before and h.num_particles() == len(st)
    # tdr_batch_pose does not score: a Cartesian filter is welcome there
    stats = (_lib.PoseStatsC * 2)()
    arr = (C.c_void_p * 2)(h.h, polar.h)
    assert L.tdr_batch_pose(arr, 2, stats, None) == 0
    mean, _ = h.mean_cov()
    assert np.array_equal(np.asarray(stats[0].mean[:], np.float32), mean) and stats[0].n == len(st)


# ---- localisation: a check that does not lean on the oracle -------------------------------------------------------------
@pytest.fixture(scope="module")
def loc_scene():
    """A 1000 px map with 6 classes and a scan of 10 000 points seen from a pose on a road, rendered into a 64 x 64 window
    of 1 m cells.  synth.make_scan looks along map direction (a - theta); the Cartesian window of top_down_map.cpp:367-389
    turns the other way round, so the window heading that reproduces the scan is -theta.  (Seed 1235: a pose whose window
    lies on labelled ground — a window inside one of the map's unlabelled holes is less than half known at every heading
    and has no finite cost to search.)"""
    cfg = synth.Config("cartloc", 10000, 6, 64, 64, 1000, 3000, polar=False, seed=1235, res=1.0)
    sc = synth.make_scene(cfg)
    y, x = int(sc.pose[1]), int(sc.pose[0])
    assert sc.class_mask[y - 32:y + 32, x - 32:x + 32].mean() < 0.25
    return sc, float((-sc.pose[2]) % (2 * np.pi))


def _heading_error(theta, truth):
    return np.angle(np.exp(1j * (np.asarray(theta, np.float64) - truth)))


@pytest.mark.gpu
def test_search_recovers_the_heading_of_a_known_pose(tdr, loc_scene):
    """A particle at the pose the scan was rendered from, heading unknown: the cost over the heading has its minimum at
    the true heading, so one of the two candidates that bracket it (9 degrees apart) wins."""
    from top_down_renderer_amd import batch
    pkg, k = tdr
    sc, heading = loc_scene
    cfg = sc.cfg
    mh = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    mh.set_window(cfg.nb, cfg.nr)
    r = batch.Renderer(sc.lut)
    r.render_cart(sc.pts, 4, 3, cfg.res, cfg.ncls, cfg.nb, cfg.nr)
    st = np.zeros(1, synth.STATE_DTYPE)
    st["init_x_px"], st["init_y_px"], st["scale"] = sc.pose[0], sc.pose[1], 1.0
    h = batch.FilterHandle(mh, 1, pkg.FilterParams(fixed_scale=1.0), seed=1, cart=True)
    h.set_states(st)
    h.compute_weights(r, cfg.res)
    got = h.states()
    err = float(_heading_error(got["theta"][0], heading))
    print(f"true window heading {np.rad2deg(heading):.2f} deg, chosen {np.rad2deg(float(got['theta'][0])):.2f} deg")
    assert got["have_init"][0] == 1
    assert abs(err) <= np.deg2rad(9.0), f"the search chose a heading {np.rad2deg(err):.1f} deg off"


@pytest.mark.gpu
def test_cold_started_filter_condenses_around_the_pose(tdr, loc_scene):
    """Closed loop through the handle: 3000 particles, sigma 30 px about the pose plus 10 % spread over the map, no
    headings.  The first update searches; 20 propagate + update steps of 0.2 m (which saturates the blend of
    particle_filter.cpp:137-141) resample.  Bounds of the basin, not of the peak (the likelihood is flat along the road,
    the weights are regularised): the mean ends nearer to the pose than the prior's own standard deviation (30 px), the
    positional variance — started at 30 px plus the uniform share — at least halves, and the mean heading is within one
    candidate spacing (9 degrees) of the truth."""
    from top_down_renderer_amd import batch
    pkg, k = tdr
    sc, heading = loc_scene
    cfg = sc.cfg
    mh = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    mh.set_window(cfg.nb, cfg.nr)
    r = batch.Renderer(sc.lut)
    r.render_cart(sc.pts, 4, 3, cfg.res, cfg.ncls, cfg.nb, cfg.nr)
    st = sc.states.copy()
    st["have_init"] = 0
    st["theta"] = 0
    h = batch.FilterHandle(mh, len(st), pkg.FilterParams(fixed_scale=1.0), seed=5, cart=True)
    h.set_states(st)
    _, cov0 = h.mean_cov()
    for _ in range(20):
        h.propagate(0.2, 0.0, 0.0)
        h.update(r, cfg.res)
    got = h.states()
    assert got["have_init"].all()
    mean, cov = h.mean_cov()
    dist = float(np.hypot(mean[0] - sc.pose[0], mean[1] - sc.pose[1]))
    err = float(np.angle(np.mean(np.exp(1j * _heading_error(got["theta"], heading)))))
    print(f"mean {dist:.1f} px from the pose, heading {np.rad2deg(err):.1f} deg off, positional variance "
          f"{cov[0, 0] + cov[1, 1]:.1f} (was {cov0[0, 0] + cov0[1, 1]:.1f})")
    assert dist < 30.0
    assert cov[0, 0] + cov[1, 1] < 0.5 * (cov0[0, 0] + cov0[1, 1])
    assert abs(err) <= np.deg2rad(9.0)
