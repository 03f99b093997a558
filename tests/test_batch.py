"""Batched filters (tdr_batch_step, csrc/tdr_batch.hip; Python: top_down_renderer_amd.batch): K filters on one map stepped
together must end bit for bit where twin handles stepped one at a time through tdr_filter_propagate + tdr_filter_update
stand — states, raw and normalised weights, resample indices, max-likelihood state, mean / covariance and the generator's
position — whether a filter took the batched path or its standalone calls."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = [1, 255, 256, 1000, 20000, 32768]


def _lib():
    from top_down_renderer_amd import _lib as L
    return L


# ---- refusals that need no handle (no device) ------------------------------------------------------------------------
def test_refuses_empty_batch():
    L = _lib()
    lib = L.load()
    assert lib.tdr_batch_step(None, 0, None, None) == -1
    assert "at least one filter" in lib.tdr_last_error().decode()


def test_refuses_null_arrays():
    L = _lib()
    lib = L.load()
    ins = (L.BatchInputC * 2)()
    assert lib.tdr_batch_step(None, 2, ins, None) == -1
    assert "null filter array" in lib.tdr_last_error().decode()
    arr = (C.c_void_p * 2)(None, None)
    assert lib.tdr_batch_step(arr, 2, None, None) == -1
    assert "null input array" in lib.tdr_last_error().decode()


def test_refuses_null_filters():
    L = _lib()
    lib = L.load()
    arr = (C.c_void_p * 3)(None, None, None)
    ins = (L.BatchInputC * 3)()
    assert lib.tdr_batch_step(arr, 3, ins, None) == -1
    assert "filter 0 is null" in lib.tdr_last_error().decode()
    b, s = C.c_int(-1), C.c_int(-1)
    assert lib.tdr_batch_last_stats(C.byref(b), C.byref(s)) == 0
    assert (b.value, s.value) == (0, 0)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _params(ncls):
    fp = _lib().FilterParamsC()
    fp.pos_cov, fp.theta_cov, fp.regularization = 0.3, np.pi / 100, 0.15
    fp.init_pos_px_x = fp.init_pos_px_y = fp.init_pos_px_cov = -1
    fp.init_pos_m_x = fp.init_pos_m_y = float("inf")
    fp.init_pos_deg_theta, fp.init_pos_deg_cov = float("inf"), 10
    fp.fixed_scale, fp.scale_log_min, fp.scale_log_max, fp.num_classes = 1.0, -0.1, 1.0, ncls
    for i in range(ncls):
        fp.class_weights[i] = 1.0
    return fp


@pytest.fixture(scope="module")
def scene():
    from top_down_renderer_amd import batch, synth
    cfg = synth.Config("batch", 20000, 6, 100, 25, 700, 1000, seed=91)
    sc = synth.make_scene(cfg)
    m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    m.sample_pts_polar(cfg.nb, cfg.nr, float(cfg.ang_res))
    return cfg, sc, m


def _states(cfg, sc, n, seed, uninit):
    from top_down_renderer_amd import synth
    st = synth.make_particles(cfg, sc.lab, sc.pose, np.random.default_rng(seed), n=n)
    if uninit:
        st["have_init"][: max(1, n // 7)] = 0   # the first update runs the 40-rotation search: the standalone path
    return st


def _make_pair(m, cfg, sc, n, seed, n_max=None, parity=True):
    from top_down_renderer_amd import batch
    fp = _params(sc.class_maps.shape[0])
    st = _states(cfg, sc, n, seed, uninit=seed % 2 == 0)
    pair = []
    for _ in range(2):
        f = batch.FilterHandle(m, n_max or n, fp, seed=seed)
        if not parity:
            f.configure(0)
        f.set_states(st)
        pair.append(f)
    return pair


def _scan(cfg, ncls, rng):
    return rng.integers(0, 4, (ncls, cfg.nb, cfg.nr)).astype(np.float32) * (rng.random((ncls, cfg.nb, cfg.nr)) < 0.2)


def _assert_same(a, b, n_before):
    assert a.num_particles() == b.num_particles()
    assert np.array_equal(a.states().view(np.uint8), b.states().view(np.uint8))
    # the normalised weights belong to the set before the resample (n_before of them: a filter that grew has no more)
    assert np.array_equal(a.weights()[:n_before], b.weights()[:n_before], equal_nan=True)
    assert np.array_equal(a.raw_weights(n_before), b.raw_weights(n_before), equal_nan=True)
    assert np.array_equal(a.resample_indices(), b.resample_indices())
    for about_max in (False, True):
        sa, ca = a.mean_cov(about_max)
        sb, cb = b.mean_cov(about_max)
        assert np.array_equal(sa, sb, equal_nan=True) and np.array_equal(ca, cb, equal_nan=True)


def _run(m, cfg, sc, pairs, steps, expect_batched, rng, n_targets=None, stream=None):
    from top_down_renderer_amd import batch
    ncls = sc.class_maps.shape[0]
    k = len(pairs)
    for step in range(steps):
        scans = [_scan(cfg, ncls, rng) for _ in range(k)]
        res = [float(1.0 + 0.05 * i + 0.01 * step) for i in range(k)]
        priors = [(0.5 + 0.1 * i, 0.05 * (i % 3), 0.01 * ((i + step) % 5 - 2)) for i in range(k)]
        nt = n_targets(step) if n_targets else [-1] * k
        n_before = [p[0].num_particles() for p in pairs]
        got = batch.step_batch([p[0] for p in pairs], scans, res, priors, n_targets=nt, stream=stream)
        for (fb, fs), sc_i, r, pr, t in zip(pairs, scans, res, priors, nt):
            fs.propagate(*pr)
            fs.update(sc_i, r, t)
        for (fb, fs), nb4 in zip(pairs, n_before):
            _assert_same(fb, fs, nb4)
        if expect_batched is not None:
            assert got == expect_batched(step), (step, got)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 16])
def test_batch_equals_standalone(scene, k):
    cfg, sc, m = scene
    pairs = [_make_pair(m, cfg, sc, COUNTS[i % len(COUNTS)], seed=11 + i) for i in range(k)]
    n_uninit = sum(1 for i in range(k) if (11 + i) % 2 == 0)
    # step 0: filters with un-initialised particles take their standalone calls (the init search); afterwards all batch
    expect = lambda step: (k - n_uninit, n_uninit) if step == 0 else (k, 0)
    # a resample to another particle count on one step (n_target), bounded by each filter's n_max
    targets = lambda step: [(-1 if step != 4 or i % 4 else max(1, COUNTS[i % len(COUNTS)] // 2)) for i in range(k)]
    _run(m, cfg, sc, pairs, 10, expect, np.random.default_rng(5 + k), targets)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20000, 32768])
def test_one_large_filter_grows_on_its_own_stream(scene, n):
    """k = 1 at the reference's size and at the limit, a resample to MORE particles (n_max > n), on a non-default stream."""
    import torch
    cfg, sc, m = scene
    pairs = [_make_pair(m, cfg, sc, n - 3000, seed=41, n_max=n)]
    stream = torch.cuda.Stream()
    targets = lambda step: [n if step == 2 else -1]
    _run(m, cfg, sc, pairs, 5, lambda step: (1, 0), np.random.default_rng(n), targets, stream=stream.cuda_stream)
    assert pairs[0][0].num_particles() == n


@pytest.mark.gpu
def test_mixed_batch(scene):
    cfg, sc, m = scene
    pairs = [_make_pair(m, cfg, sc, 1000, seed=3),                      # eligible
             _make_pair(m, cfg, sc, 1000, seed=5, parity=False),        # the counter-based device generator: standalone
             _make_pair(m, cfg, sc, 40000, seed=7)]                     # above 32 768 particles: standalone
    _run(m, cfg, sc, pairs, 4, lambda step: (1, 2), np.random.default_rng(17))


@pytest.mark.gpu
def test_renderer_input(scene):
    from top_down_renderer_amd import batch
    cfg, sc, m = scene
    r = batch.Renderer(sc.lut)
    pts = np.zeros((len(sc.pts), 8), np.float32)
    pts[:, :3], pts[:, 4] = sc.pts[:, :3], sc.pts[:, 3]
    r.render_polar(pts, 8, 4, cfg.res, float(cfg.ang_res), sc.class_maps.shape[0], cfg.nb, cfg.nr)
    pairs = [_make_pair(m, cfg, sc, n, seed=s) for n, s in ((256, 21), (5000, 23))]
    for step in range(3):
        n_before = [p[0].num_particles() for p in pairs]
        got = batch.step_batch([p[0] for p in pairs], [r, r], cfg.res, [(1.0, 0.2, 0.02), (0.7, -0.1, 0.0)])
        assert got == (2, 0)
        for (fb, fs), pr, nb4 in zip(pairs, [(1.0, 0.2, 0.02), (0.7, -0.1, 0.0)], n_before):
            fs.propagate(*pr)
            fs.update(r, cfg.res)
            _assert_same(fb, fs, nb4)


@pytest.mark.gpu
def test_refusals_leave_filters_alone(scene):
    from top_down_renderer_amd import batch, synth
    cfg, sc, m = scene
    L = _lib()
    lib = L.load()
    ncls = sc.class_maps.shape[0]
    rng = np.random.default_rng(29)
    pairs = [_make_pair(m, cfg, sc, 500, seed=31), _make_pair(m, cfg, sc, 700, seed=33)]
    _run(m, cfg, sc, pairs, 1, None, rng)   # (past the init search: both would batch)
    other = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    other.sample_pts_polar(cfg.nb, cfg.nr, float(cfg.ang_res))
    f_other = batch.FilterHandle(other, 64, _params(ncls), seed=35)
    f_other.set_states(synth.make_particles(cfg, sc.lab, sc.pose, np.random.default_rng(1), n=64))
    unsampled = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    f_unsampled = batch.FilterHandle(unsampled, 64, _params(ncls), seed=37)
    r_empty = batch.Renderer(sc.lut)
    r_wrong = batch.Renderer(sc.lut)
    pts = np.zeros((len(sc.pts), 8), np.float32)
    pts[:, :3], pts[:, 4] = sc.pts[:, :3], sc.pts[:, 3]
    r_wrong.render_polar(pts, 8, 4, cfg.res, float(cfg.ang_res), ncls, cfg.nb, cfg.nr + 1)
    a, b = pairs[0][0], pairs[1][0]
    scan = _scan(cfg, ncls, rng)

    def call(filters, inputs):
        arr = (C.c_void_p * len(filters))(*[f.h for f in filters])
        ins = (L.BatchInputC * len(inputs))()
        keep = []
        for i, x in enumerate(inputs):
            if isinstance(x, batch.Renderer):
                ins[i].renderer = x.h
            elif x is not None:
                imgs = np.ascontiguousarray(np.transpose(x, (0, 2, 1)))
                keep.append(imgs)
                ins[i].scan_imgs = imgs.ctypes.data
            ins[i].res, ins[i].tx, ins[i].n_target = 1.0, 1.0, -1
        rc = lib.tdr_batch_step(arr, len(filters), ins, None)
        return rc, lib.tdr_last_error().decode()

    cases = [([a, b, a], [scan, scan, scan], "appears twice"),
             ([a, f_other], [scan, scan], "on another map"),
             ([f_unsampled], [scan], "samplePtsPolar was never called"),
             ([a, b], [scan, None], "input 1 has no scan"),
             ([a, b], [scan, r_empty], "has no render"),
             ([a, b], [r_wrong, scan], "does not match the map's")]
    for filters, inputs, msg in cases:
        before = [(f.states().tobytes(), f.weights().tobytes()) for f in (a, b)]
        rc, err = call(filters, inputs)
        assert rc == -1 and msg in err, (msg, rc, err)
        assert [(f.states().tobytes(), f.weights().tobytes()) for f in (a, b)] == before
    with pytest.raises(ValueError):   # the Python layer checks image shapes itself
        batch.step_batch([a], [scan[:, :, :-1]], 1.0, [(1.0, 0.0, 0.0)])
    # the generators did not move either: the next step still matches the twins
    _run(m, cfg, sc, pairs, 2, lambda step: (2, 0), rng)


# ---- the C++ façade (include/top_down_render/particle_filter_batch.h) -------------------------------------------------
@pytest.fixture(scope="module")
def facade_batch_exe():
    import subprocess
    import tempfile
    from top_down_renderer_amd import build
    build.build()
    pkg = os.path.join(ROOT, "top_down_renderer_amd")
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), "facade_batch")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_batch.cpp"), "-o", exe, "-L", pkg, "-ltdr_hip",
                    f"-Wl,-rpath,{pkg}"], check=True)
    return exe


def test_facade_batch_compiles(facade_batch_exe):
    assert os.access(facade_batch_exe, os.X_OK)


@pytest.mark.gpu
def test_facade_batch_matches_standalone(facade_batch_exe):
    import subprocess
    out = subprocess.run([facade_batch_exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["ok", "3", "0"], out.stdout
