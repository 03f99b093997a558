"""The 40-rotation init search inside a batch (tdr_config_tuning("batch_init_search"), csrc/tdr_score_init.hip): with the
switch on, a filter that may hold a particle without a heading — a cold start, a gated filter — takes the batched path of
tdr_batch_step and must still end bit for bit where a twin handle stepped through tdr_filter_propagate + tdr_filter_update
stands: states (the chosen theta, have_init), raw and normalised weights, resample indices, both mean / covariance forms.
Every comparison is an equality; every test restores the switch to 0."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLT_MAX = np.float32(3.402823466e+38)


def _lib():
    from top_down_renderer_amd import _lib as L
    return L


@contextlib.contextmanager
def _switch(on=True):
    from top_down_renderer_amd import batch
    try:
        batch.set_init_search_in_batch(on)
        yield
    finally:
        batch.set_init_search_in_batch(False)


# ---- no device ---------------------------------------------------------------------------------------------------------
def test_tuning_name():
    lib = _lib().load()
    try:
        assert lib.tdr_config_tuning(b"batch_init_search", -1) == 0
        assert lib.tdr_config_tuning(b"batch_init_search", 1) == 1
        assert lib.tdr_config_tuning(b"batch_init_search", -1) == 1
        assert lib.tdr_config_tuning(b"batch_init_search", 0) == 0
    finally:
        lib.tdr_config_tuning(b"batch_init_search", 0)


def test_python_switch():
    from top_down_renderer_amd import batch
    try:
        assert batch.init_search_in_batch() is False
        assert batch.set_init_search_in_batch(True) is True
        assert batch.init_search_in_batch() is True
    finally:
        assert batch.set_init_search_in_batch(False) is False


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _params(ncls, weights=None, force_on_map=0, fixed_scale=1.0):
    fp = _lib().FilterParamsC()
    fp.pos_cov, fp.theta_cov, fp.regularization = 0.3, np.pi / 100, 0.15
    fp.init_pos_px_x = fp.init_pos_px_y = fp.init_pos_px_cov = -1
    fp.init_pos_m_x = fp.init_pos_m_y = float("inf")
    fp.init_pos_deg_theta, fp.init_pos_deg_cov = float("inf"), 10
    fp.force_on_map = force_on_map
    fp.fixed_scale, fp.scale_log_min, fp.scale_log_max, fp.num_classes = fixed_scale, -0.1, 1.0, ncls
    for i in range(ncls):
        fp.class_weights[i] = 1.0 if weights is None else float(weights[i])
    return fp


def _scene(ncls, seed=91):
    from top_down_renderer_amd import batch, synth
    cfg = synth.Config("batch_init", 20000, ncls, 100, 25, 700, 1000, seed=seed)
    sc = synth.make_scene(cfg)
    m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    m.sample_pts_polar(cfg.nb, cfg.nr, float(cfg.ang_res))
    return cfg, sc, m


@pytest.fixture(scope="module")
def scene():
    return _scene(6)


def _states(cfg, sc, n, seed, uninit):
    """uninit: 'some' = the first n // 7 particles have no heading, 'all' = none has."""
    from top_down_renderer_amd import synth
    st = synth.make_particles(cfg, sc.lab, sc.pose, np.random.default_rng(seed), n=n)
    if uninit == "all":
        st["have_init"][:] = 0
    elif uninit == "some":
        st["have_init"][: max(1, n // 7)] = 0
    return st


def _pair(m, fp, st, seed, n_max=None):
    from top_down_renderer_amd import batch
    pair = []
    for _ in range(2):
        f = batch.FilterHandle(m, n_max or len(st), fp, seed=seed)
        f.set_states(st)
        pair.append(f)
    return pair


def _scan(cfg, ncls, rng):
    return rng.integers(0, 4, (ncls, cfg.nb, cfg.nr)).astype(np.float32) * (rng.random((ncls, cfg.nb, cfg.nr)) < 0.2)


def _assert_same(a, b, n_before):
    assert a.num_particles() == b.num_particles()
    assert np.array_equal(a.states().view(np.uint8), b.states().view(np.uint8))
    assert np.array_equal(a.weights()[:n_before], b.weights()[:n_before], equal_nan=True)
    assert np.array_equal(a.raw_weights(n_before), b.raw_weights(n_before), equal_nan=True)
    assert np.array_equal(a.resample_indices(), b.resample_indices())
    for about_max in (False, True):
        sa, ca = a.mean_cov(about_max)
        sb, cb = b.mean_cov(about_max)
        assert np.array_equal(sa, sb, equal_nan=True) and np.array_equal(ca, cb, equal_nan=True)


def _run(cfg, ncls, pairs, steps, expect, rng, n_targets=None, scans_of=None, after_step=None):
    """Steps the first handle of every pair in one step_batch, its twin through propagate + update; compares after every
    step.  expect(step) -> (batched, standalone); scans_of(step, i) overrides filter i's scan; after_step(step)."""
    from top_down_renderer_amd import batch
    k = len(pairs)
    for step in range(steps):
        scans = [_scan(cfg, ncls, rng) for _ in range(k)]
        if scans_of:
            scans = [scans_of(step, i, s) for i, s in enumerate(scans)]
        res = [float(1.0 + 0.05 * i + 0.01 * step) for i in range(k)]
        priors = [(0.5 + 0.1 * i, 0.05 * (i % 3), 0.01 * ((i + step) % 5 - 2)) for i in range(k)]
        nt = n_targets(step) if n_targets else [-1] * k
        n_before = [p[0].num_particles() for p in pairs]
        got = batch.step_batch([p[0] for p in pairs], scans, res, priors, n_targets=nt)
        for (fb, fs), sc_i, r, pr, t in zip(pairs, scans, res, priors, nt):
            fs.propagate(*pr)
            fs.update(sc_i, r, t)
        for (fb, fs), nb4 in zip(pairs, n_before):
            _assert_same(fb, fs, nb4)
        assert got == expect(step), (step, got)
        if after_step:
            after_step(step)


COLD_COUNTS = [1000, 5000, 1, 255, 256]   # (k = 1 is the 1000-particle filter)


def _cold_pairs(m, cfg, sc, k, seed0=11):
    ncls = sc.class_maps.shape[0]
    return [_pair(m, _params(ncls), _states(cfg, sc, COLD_COUNTS[i % len(COLD_COUNTS)], seed0 + i, "all" if i % 2 else "some"),
                  seed0 + i) for i in range(k)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 16])
def test_cold_start_joins_the_batch(scene, k):
    """Cases 1 and 11: every filter has un-initialised particles (some n // 7 of them, some all), the split pass (6 classes,
    fewer than 8192 particles); no filter runs standalone, not at step 0 either; the search picks more than one heading."""
    cfg, sc, m = scene
    L = _lib()
    lib = L.load()
    from top_down_renderer_amd.batch import _scan_images
    with _switch():
        pairs = _cold_pairs(m, cfg, sc, k)
        # Not vacuous: the stepped handles are resampled and propagated by the time they can be read, so the headings the
        # search chose are read from a probe — a third handle of every filter taken through step 0's propagate and scoring
        # alone (tdr_filter_compute_weights: no resample), with step 0's prior, scan and resolution as _run draws them.
        probes = [p[0] for p in _cold_pairs(m, cfg, sc, k)]
        scans0 = [_scan(cfg, 6, r) for r in [np.random.default_rng(5 + k)] for _ in range(k)]
        distinct = []
        for i, pb in enumerate(probes):
            was_uninit = pb.states()["have_init"] == 0
            pb.propagate(0.5 + 0.1 * i, 0.05 * (i % 3), 0.01 * (i % 5 - 2))
            imgs = _scan_images(scans0[i], m)
            L.check(lib.tdr_filter_compute_weights(pb.h, imgs.ctypes.data_as(C.c_void_p), None, C.c_float(1.0 + 0.05 * i)))
            st = pb.states()
            assert st["have_init"].all()
            distinct.append(len(np.unique(st["theta"][was_uninit])))
        assert max(distinct) > 1, distinct
        targets = lambda step: [(-1 if step != 3 or i % 4 else max(1, COLD_COUNTS[i % len(COLD_COUNTS)] // 2)) for i in range(k)]
        _run(cfg, 6, pairs, 6, lambda step: (k, 0), np.random.default_rng(5 + k), targets)


@pytest.mark.gpu
def test_switch_off_keeps_the_split(scene):
    """Case 10: with the switch off (the default) the same cold-start batch reports today's split at step 0."""
    cfg, sc, m = scene
    k = 5
    assert _lib().load().tdr_config_tuning(b"batch_init_search", -1) == 0
    pairs = _cold_pairs(m, cfg, sc, k)
    _run(cfg, 6, pairs, 3, lambda step: (0, k) if step == 0 else (k, 0), np.random.default_rng(77))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["equal", "groups", "mixed_pass"])
def test_half_record_pass(scene, case):
    """Case 2: filters of 8192, 20 000 and 32 768 particles (the half-record pass).  equal: one group; groups: two filters
    with different non-uniform class weights and one with uniform weights — three sets of half records, rebuilt between
    them; mixed_pass: a 1000-particle filter (split on the fly) next to a 20 000-particle one."""
    cfg, sc, m = scene
    w_a = [1.0, 2.0, 0.5, 1.0, 3.0, 1.5]
    w_b = [0.25, 1.0, 1.0, 4.0, 1.0, 2.0]
    spec = {"equal": [(8192, None), (20000, None), (32768, None)],
            "groups": [(8192, w_a), (20000, None), (32768, w_b), (9000, w_a)],
            "mixed_pass": [(1000, None), (20000, None)]}[case]
    with _switch():
        pairs = [_pair(m, _params(6, w), _states(cfg, sc, n, 60 + i, "some" if i % 2 else "all"), 60 + i)
                 for i, (n, w) in enumerate(spec)]
        _run(cfg, 6, pairs, 3, lambda step: (len(spec), 0), np.random.default_rng(19))


@pytest.mark.gpu
@pytest.mark.parametrize("ncls", [3, 7, 11, 15])
def test_record_widths(ncls):
    """Case 3: 3 classes (4-float records: the half pass from 8192 particles on, the vector kernel below), 7 classes (SEVEN),
    11 and 15 classes (the wide kernel: 12- and 16-float records)."""
    cfg, sc, m = _scene(ncls, seed=90 + ncls)
    w = [1.0 + 0.25 * (c % 3) for c in range(ncls)]
    with _switch():
        pairs = [_pair(m, _params(ncls, wt), _states(cfg, sc, n, 70 + i, u), 70 + i)
                 for i, (n, wt, u) in enumerate([(700, None, "all"), (9000, None, "some"), (1300, w, "all"), (8500, w, "some")])]
        _run(cfg, ncls, pairs, 3, lambda step: (4, 0), np.random.default_rng(23 + ncls))


@pytest.mark.gpu
def test_vector_only(scene):
    """Case 4: tdr_config_init_mfma(0) — the vector kernel alone, for the batch and the twins alike."""
    cfg, sc, m = scene
    lib = _lib().load()
    before = lib.tdr_config_init_mfma(-1)
    try:
        lib.tdr_config_init_mfma(0)
        with _switch():
            pairs = [_pair(m, _params(6), _states(cfg, sc, n, 80 + i, "all"), 80 + i) for i, n in enumerate([300, 2000, 9000])]
            _run(cfg, 6, pairs, 3, lambda step: (3, 0), np.random.default_rng(31))
    finally:
        lib.tdr_config_init_mfma(before)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1500, 9000])
def test_f16_flag_is_per_filter(scene, n):
    """Case 5: the middle filter's scan holds one bin of count 3000 (> 2048: not exact in f16), so ITS search is redone by
    the vector kernel; its neighbours keep the matrix-core pass's result.  All three equal their twins."""
    cfg, sc, m = scene

    def scans_of(step, i, s):
        if i == 1 and step == 0:
            s = s.copy()
            s[2, 17, 5] = 3000.0
        return s

    with _switch():
        pairs = [_pair(m, _params(6), _states(cfg, sc, n, 100 + i, "all"), 100 + i) for i in range(3)]
        _run(cfg, 6, pairs, 2, lambda step: (3, 0), np.random.default_rng(37), scans_of=scans_of)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["force_on_map", "unknown_scale"])
def test_gated_filters_stay_in_the_batch(scene, mode):
    """Case 6: gated particles (off the map with force_on_map; a scale outside 10^scale_log_min .. 10^scale_log_max with
    fixed_scale = -1) can stay without a heading, so the filter may hold one for ever — and is batched at every step.
    Not vacuous: a probe handle (propagate + raw weights, no resample — the resample of a full step never draws a particle
    of weight 0, so the stepped handles cannot show it) still holds particles with have_init == 0 and raw weight 0."""
    cfg, sc, m = scene
    L = _lib()
    lib = L.load()
    from top_down_renderer_amd.batch import _scan_images
    k = 3
    fp = _params(6, force_on_map=1) if mode == "force_on_map" else _params(6, fixed_scale=-1.0)
    sts = []
    for i, n in enumerate([500, 3000, 9000]):
        st = _states(cfg, sc, n, 120 + i, "all")
        tenth = np.arange(n) % 10 == 3
        if mode == "force_on_map":
            st["init_x_px"][tenth] = -60.0 - np.arange(tenth.sum()) % 7
        else:
            st["scale"][tenth] = 0.3    # below 10^-0.1
        sts.append(st)
    with _switch():
        pairs = [_pair(m, fp, st, 120 + i) for i, st in enumerate(sts)]
        probe = _pair(m, fp, sts[1], 121)[0]
        probe.propagate(0.6, 0.05, -0.01)
        imgs = _scan_images(_scan(cfg, 6, np.random.default_rng(3)), m)
        L.check(lib.tdr_filter_compute_weights(probe.h, imgs.ctypes.data_as(C.c_void_p), None, C.c_float(1.0)))
        pst, praw = probe.states(), probe.raw_weights(len(sts[1]))
        left = pst["have_init"] == 0
        assert left.sum() >= len(sts[1]) // 20 and (praw[left] == 0).all() and (pst["have_init"] == 1).any()
        _run(cfg, 6, pairs, 5, lambda step: (k, 0), np.random.default_rng(41))


@pytest.mark.gpu
def test_empty_scan(scene):
    """Case 7: an all-zero scan for one filter of the batch: cost and normalisation are 0 / 0, every rotation scores NaN,
    the search flags the particle (res_flag == 2) and the fixup gives it the weight 1 / (FLT_MAX + regularization).  The
    twin's raw weights are asserted to be that value, so the case reaches the path it names (an all-zero scan does)."""
    cfg, sc, m = scene

    def scans_of(step, i, s):
        return np.zeros_like(s) if (i == 1 and step == 0) else s

    with _switch():
        pairs = [_pair(m, _params(6), _states(cfg, sc, n, 140 + i, "all"), 140 + i) for i, n in enumerate([600, 2048, 9000])]
        seen = {}

        def after(step):
            if step == 0:
                seen["raw"] = pairs[1][1].raw_weights(2048).copy()

        _run(cfg, 6, pairs, 2, lambda step: (3, 0), np.random.default_rng(43), scans_of=scans_of, after_step=after)
        want = np.float32(1.0 / (np.float64(FLT_MAX) + np.float64(np.float32(0.15))))
        assert want > 0 and (seen["raw"] == want).all(), (want, np.unique(seen["raw"])[:4])


@pytest.mark.gpu
def test_mixed_scale_modes(scene):
    """Case 8: filters with one scale for all particles (the uniform-scale table) and filters whose particles each have
    their own in one batch — another instantiation of every search kernel, another launch over the same run."""
    cfg, sc, m = scene
    rng = np.random.default_rng(47)
    sts = []
    for i, n in enumerate([400, 1200, 9000, 8200, 2500]):
        st = _states(cfg, sc, n, 160 + i, "all" if i % 2 else "some")
        if i in (1, 3, 4):
            st["scale"] = rng.uniform(0.9, 1.3, n).astype(np.float32)
        sts.append(st)
    with _switch():
        pairs = [_pair(m, _params(6), st, 160 + i) for i, st in enumerate(sts)]
        _run(cfg, 6, pairs, 3, lambda step: (5, 0), np.random.default_rng(53))


@pytest.mark.gpu
def test_renderer_input(scene):
    """Case 9: the scan comes from a renderer's last render on the device (scan_imgs = NULL) for cold-started filters."""
    from top_down_renderer_amd import batch
    cfg, sc, m = scene
    r = batch.Renderer(sc.lut)
    pts = np.zeros((len(sc.pts), 8), np.float32)
    pts[:, :3], pts[:, 4] = sc.pts[:, :3], sc.pts[:, 3]
    r.render_polar(pts, 8, 4, cfg.res, float(cfg.ang_res), sc.class_maps.shape[0], cfg.nb, cfg.nr)
    priors = [(1.0, 0.2, 0.02), (0.7, -0.1, 0.0)]
    with _switch():
        pairs = [_pair(m, _params(6), _states(cfg, sc, n, s, "all"), s) for n, s in ((256, 21), (9000, 23))]
        for step in range(3):
            n_before = [p[0].num_particles() for p in pairs]
            got = batch.step_batch([p[0] for p in pairs], [r, r], cfg.res, priors)
            assert got == (2, 0), (step, got)
            for (fb, fs), pr, nb4 in zip(pairs, priors, n_before):
                fs.propagate(*pr)
                fs.update(r, cfg.res)
                _assert_same(fb, fs, nb4)


# ---- the C++ façade (include/top_down_render/particle_filter_batch.h) -------------------------------------------------
@pytest.fixture(scope="module")
def facade_batch_init_exe():
    import subprocess
    import tempfile
    from top_down_renderer_amd import build
    build.build()
    pkg = os.path.join(ROOT, "top_down_renderer_amd")
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), "facade_batch_init")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_batch_init.cpp"), "-o", exe, "-L", pkg, "-ltdr_hip",
                    f"-Wl,-rpath,{pkg}"], check=True)
    return exe


def test_facade_batch_init_compiles(facade_batch_init_exe):
    assert os.access(facade_batch_init_exe, os.X_OK)


@pytest.mark.gpu
def test_facade_batch_init_matches_standalone(facade_batch_init_exe):
    import subprocess
    out = subprocess.run([facade_batch_init_exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["ok", "4", "0"], out.stdout
