"""The mixture fit on the device (csrc/tdr_gmm.hip): tdr_k_gmm_samples / tdr_k_gmm_fit / the jobs and
pick launches, tdr_filter_compute_gmm_device and tdr_batch_compute_gmm.

The reference for parity is the project's host fit (tdr_gmm_fit_host / tdr_gmm_select_host, themselves held to the NumPy
oracle by tests/test_gmm.py), with that file's tolerances.  The device forms every sum in the host's order, so it should
sit orders of magnitude inside them; every comparison prints its largest difference before it asserts."""
import ctypes as C
import ctypes.util
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
KS = (1, 2, 3, 4, 5, 8, 32)


# ---- fixtures: tests/test_gmm.py's _mixture (the same draws in the same order), keeping the headings -----------------------
def _mixture(rng, centres, sig, n_each, sig_theta):
    xs = []
    for (cx, cy, th), s in zip(centres, sig):
        xy = rng.normal([cx, cy], s, (n_each, 2))
        t = rng.normal(th, sig_theta, n_each)
        xs.append(np.column_stack([xy, 50 * np.cos(t), 50 * np.sin(t), t]))
    x = np.concatenate(xs)
    return x[rng.permutation(len(x))]


@functools.lru_cache(maxsize=None)
def _fixture(name):
    """(samples (m, 4) float64, {x, y, theta} (m, 3) float64)"""
    spec = {"two": (6, [(100, 200, 0.3), (400, 250, -2.0)], [10, 10], 400, 0.001, None),
            "three": (5, [(100, 200, 0.3), (400, 250, -2.0), (250, 600, 1.5)], [8, 15, 5], 300, 0.001, None),
            "one": (7, [(300, 300, 1.0)], [4], 1000, 0.001, None),
            "small": (8, [(50, 60, 0.2), (90, 20, 2.0)], [3, 3], 19, 0.001, 37),
            "wide": (9, [(500, 500, 0)], [150], 1000, 1.5, None)}[name]
    seed, centres, sig, n_each, sig_theta, first = spec
    x = _mixture(np.random.default_rng(seed), centres, sig, n_each, sig_theta)[:first]
    return np.ascontiguousarray(x[:, :4]), np.ascontiguousarray(x[:, [0, 1, 4]])


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def _host_fit_cached(key, k, max_iter):
    return _host_fit(_CASES[key], k, max_iter)


_CASES = {}


def _host_fit(x, k, max_iter=100):
    from top_down_renderer_amd import _lib
    lib = _lib.load()
    x = np.ascontiguousarray(x, np.float64)
    w, mu, cov, ll = np.zeros(k), np.zeros((k, 4)), np.zeros((k, 4, 4)), C.c_double(0)
    assert lib.tdr_gmm_fit_host(_p(x), len(x), k, max_iter, _p(w), _p(mu), _p(cov), C.byref(ll)) == 0
    return w, mu, cov, ll.value


@pytest.fixture(scope="module")
def kern():
    from top_down_renderer_amd.kernels import HipKernels
    return HipKernels()


def _check_fit(kern, x, k, max_iter=100, tag="", key=None):
    """Device fit against the host fit, tests/test_gmm.py's tolerances (|dll| < 1e-8 at k = 32, where the host's two
    statements already differ by 7.8e-10)."""
    if key is not None:
        _CASES[key] = x
        w, mu, cov, ll = _host_fit_cached(key, k, max_iter)
    else:
        w, mu, cov, ll = _host_fit(x, k, max_iter)
    dw, dmu, dcov, dll, used = kern.gmm_fit(kern.to_device(np.ascontiguousarray(x, np.float64)), k, max_iter)
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0  # noqa: E731
    print(f"gmm fit {tag} m={len(x)} k={k} it={used}: max rel dw {rel(dw, w):.3g}  max |dmu| {np.max(np.abs(dmu - mu)):.3g}  "
          f"max |dcov| {np.max(np.abs(dcov - cov)):.3g}  |dll| {abs(dll - ll):.3g}")
    assert np.allclose(dw, w, rtol=1e-8), (tag, k)
    assert np.allclose(dmu, mu, rtol=1e-8, atol=1e-8), (tag, k)
    assert np.allclose(dcov, cov, rtol=1e-6, atol=1e-8), (tag, k)
    assert abs(dll - ll) < (1e-8 if k == 32 else 1e-9), (tag, k)
    assert 1 <= used <= max(1, max_iter)
    return used


# ---- samples -----------------------------------------------------------------------------------------------------------------
def test_samples_are_the_host_conversion_byte_for_byte(kern):
    libm = C.CDLL(ctypes.util.find_library("m"))
    for fn in (libm.cosf, libm.sinf):
        fn.restype, fn.argtypes = C.c_float, [C.c_float]
    pi = np.float32(np.pi)
    special = np.array([0, pi, -pi, pi / 2, -pi / 2, 1e-30, 1e6, np.nan, np.inf, -np.inf], np.float32)
    rng = np.random.default_rng(3)
    for num in (1, 63, 64, 65, 1000):
        th = np.resize(np.concatenate([special, rng.uniform(-7, 7, 23).astype(np.float32)]), num).astype(np.float32)
        ml3 = np.column_stack([rng.uniform(-2000, 2000, num), rng.uniform(-2000, 2000, num), th]).astype(np.float32)
        with np.errstate(invalid="ignore"):
            want = np.empty((num, 4), np.float64)
            want[:, 0], want[:, 1] = ml3[:, 0], ml3[:, 1]
            # 50 * std::cos(float): the float overload, a FLOAT product, widened afterwards
            want[:, 2] = [np.float32(50) * np.float32(libm.cosf(float(t))) for t in th]
            want[:, 3] = [np.float32(50) * np.float32(libm.sinf(float(t))) for t in th]
        got = kern.gmm_samples(kern.to_device(ml3), num).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (num, 4)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), num


# ---- the fit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two", "three", "one", "small", "wide"])
def test_fit_matches_the_host_fit(kern, name):
    x, _ = _fixture(name)
    for k in KS:
        if k <= len(x):
            _check_fit(kern, x, k, tag=name, key=name)


def test_fit_at_the_shapes_where_the_kernel_can_go_wrong(kern):
    one, _ = _fixture("one")
    small, _ = _fixture("small")
    three, _ = _fixture("three")
    _check_fit(kern, one[:1], 1, tag="m=1")
    _check_fit(kern, one[:2], 2, tag="k==m")
    for k in (1, 2, 3):
        _check_fit(kern, small, k, tag="m=37")
    for m in (63, 64, 65, 255, 256, 257, 999, 1000):          # around the wave, half the workgroup and the sample limit
        _check_fit(kern, one[:m], 3, tag="prefix of one")
    for k in (31, 32):
        _check_fit(kern, one, k, tag="one", key="one")
    wide, _ = _fixture("wide")
    for max_iter in (1, 3):                                    # stops on the bound, not on convergence (100 E-steps unbounded)
        assert _check_fit(kern, wide, 3, max_iter, tag="wide max_iter") == max_iter
        assert _check_fit(kern, three, 4, max_iter, tag="three max_iter") == max_iter
    for max_iter in (1, 2):        # the widest case's first steps: a sum out of the host's order would show here already
        _check_fit(kern, wide, 32, max_iter, tag="wide first steps")
    same = np.tile(one[:1], (50, 1))                           # covariance = 1e-6 I, repeated seeds, empty clusters
    for k in (1, 3):
        _check_fit(kern, same, k, tag="identical")
    two_pts = np.tile(one[:2], (50, 1))
    for k in (2, 3):
        _check_fit(kern, two_pts, k, tag="two points")
    # the twin refuses what the host fit refuses
    x = kern.to_device(one)
    out, ws = kern.zeros((700,), x.dtype), kern.zeros((32000,), x.dtype)
    for m, k in ((2, 3), (0, 1), (10, 0), (10, 33), (1001, 2)):
        assert kern.lib.tdr_k_gmm_fit(C.c_void_p(x.data_ptr()), m, k, 100, C.c_void_p(out.data_ptr()),
                                      C.c_void_p(ws.data_ptr()), kern.stream()) != 0


def test_fit_is_deterministic_and_independent_of_its_place_in_the_grid(kern):
    import torch
    from top_down_renderer_amd import _lib
    x, _ = _fixture("two")
    m, k = len(x), 3
    xd = kern.to_device(x)
    a = kern.gmm_fit(xd, k)
    b = kern.gmm_fit(xd, k)
    for u, v in zip(a, b):
        assert np.array_equal(np.asarray(u), np.asarray(v))
    nj, od = 192, 21 * k + 2
    outs = kern.zeros((nj, od), torch.float64)
    wss = kern.zeros((nj, m * k), torch.float64)
    jobs = (_lib.GmmJobC * nj)(*[_lib.GmmJobC(xd.data_ptr(), m, k, 100, 0, outs[j].data_ptr(), wss[j].data_ptr())
                                  for j in range(nj)])
    jd = kern.to_device(np.frombuffer(bytes(jobs), np.uint8))
    assert kern.lib.tdr_k_gmm_fit_jobs(C.c_void_p(jd.data_ptr()), nj, kern.stream()) == 0
    o = outs.cpu().numpy()
    alone = np.concatenate([a[0].ravel(), a[1].ravel(), a[2].ravel(), [a[3], a[4]]])
    for j in (0, 17, 191):
        assert np.array_equal(o[j].view(np.uint64), alone.view(np.uint64)), j


# ---- selection through the handle ------------------------------------------------------------------------------------------------
def _params(ncls):
    from top_down_renderer_amd import _lib
    fp = _lib.FilterParamsC()
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
    """Two maps: a polar one and one with a Cartesian window (a Cartesian filter's)."""
    from top_down_renderer_amd import batch, synth
    cfg = synth.Config("gmmdev", 20000, 6, 100, 25, 700, 1000, seed=91)
    sc = synth.make_scene(cfg)
    m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    m.sample_pts_polar(cfg.nb, cfg.nr, float(cfg.ang_res))
    mc = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    mc.set_window(32, 24)
    return cfg, sc, m, mc


def _states(xyt, n):
    """n particles whose strided samples (particle min(n-1, i*n/num), :265-266) are the fixture's rows (all of them while
    n <= len(xyt) ... the first num otherwise), every other particle a copy of a row near its own place."""
    from top_down_renderer_amd import batch
    m = len(xyt)
    num = min(1000, n)
    src = np.minimum(m - 1, np.arange(n, dtype=np.int64) * min(m, num) // n)
    idx = np.minimum(n - 1, np.arange(num, dtype=np.int64) * n // num)
    src[idx] = np.arange(num) % m
    st = np.zeros(n, batch.STATE_DTYPE)
    st["init_x_px"], st["init_y_px"], st["theta"] = xyt[src, 0], xyt[src, 1], xyt[src, 2]
    st["scale"], st["have_init"] = 1.0, 1
    return st


def _twins(mh, ncls, st, start, cart=False, n_max=None):
    from top_down_renderer_amd import batch
    out = []
    for _ in range(2):
        f = batch.FilterHandle(mh, n_max or len(st), _params(ncls), seed=5, cart=cart)
        f.set_states(st)
        f.set_num_gaussians(start)
        out.append(f)
    return out


def _check_twins(dev, host, tag):
    """dev: after compute_gmm(device=True); host: after compute_gmm(device=False) on the same states."""
    md, cd = dev.get_gmm()
    mh, ch = host.get_gmm()
    print(f"gmm select {tag}: k {dev.num_gaussians()} / {host.num_gaussians()}  max |dmean| "
          f"{np.max(np.abs(md - mh)) if md.shape == mh.shape else -1:.3g}  max |dcov| "
          f"{np.max(np.abs(cd - ch)) if cd.shape == ch.shape else -1:.3g}  count {dev.adaptive_count()} / {host.adaptive_count()}")
    assert dev.num_gaussians() == host.num_gaussians() == len(md) == len(mh), tag
    assert np.allclose(md, mh, atol=1e-4), tag
    assert np.allclose(cd, ch, rtol=1e-4, atol=1e-4), tag
    assert dev.adaptive_count() == host.adaptive_count(), tag


SELECT = [("two", 1), ("two", 2), ("two", 4), ("three", 1), ("three", 2), ("three", 3), ("three", 4), ("one", 1),
          ("one", 2), ("small", 1), ("small", 2), ("small", 3)]


@pytest.mark.parametrize("name,start", SELECT)
def test_device_selection_equals_the_host_selection(scene, name, start):
    cfg, sc, m, mc = scene
    _, xyt = _fixture(name)
    dev, host = _twins(m, sc.class_maps.shape[0], _states(xyt, len(xyt)), start)
    dev.compute_gmm(device=True)
    host.compute_gmm(device=False)
    _check_twins(dev, host, f"{name} from {start}")
    if (name, start) == ("two", 1):
        assert dev.num_gaussians() == 2
    if (name, start) == ("two", 4):
        assert dev.num_gaussians() == 3


@pytest.mark.parametrize("n,start,cart", [(1, 1, False), (19, 2, False), (20, 2, True), (40, 1, False), (999, 2, False),
                                          (1000, 2, True), (1001, 3, False), (20000, 1, False), (20000, 32, False),
                                          (100003, 2, False)])
def test_device_selection_over_particle_counts(scene, n, start, cart):
    cfg, sc, m, mc = scene
    _, xyt = _fixture("two" if n > 40 else "small")
    dev, host = _twins(mc if cart else m, sc.class_maps.shape[0], _states(xyt, n), start, cart=cart)
    dev.compute_gmm(device=True)
    host.compute_gmm(device=False)
    _check_twins(dev, host, f"n={n} from {start}{' cart' if cart else ''}")
    if (n, start) == (40, 1):
        assert dev.num_gaussians() == 1          # k * 50 >= n: k + 1 is never tried (:280)


@pytest.mark.parametrize("cart", [False, True])
def test_device_fit_leaves_the_filter_untouched(scene, cart):
    cfg, sc, m, mc = scene
    ncls = sc.class_maps.shape[0]
    _, xyt = _fixture("two")
    st = _states(xyt, 3000)
    dev, host = _twins(mc if cart else m, ncls, st, 1, cart=cart)
    rng = np.random.default_rng(12)
    shape = (ncls, 32, 24) if cart else (ncls, cfg.nb, cfg.nr)
    scan = rng.integers(0, 4, shape).astype(np.float32) * (rng.random(shape) < 0.2)
    for f in (dev, host):                          # one step first: weights and raw weights exist
        f.propagate(1.0, 0.2, 0.02)
        f.update(scan, 1.0)
    before = (dev.states().copy(), dev.weights().copy(), dev.raw_weights(3000).copy(), dev.resample_indices().copy())
    assert dev.step_count() == host.step_count() == 1
    assert len(dev.get_gmm()[0]) == 0 and dev.adaptive_count() == 3000
    dev.compute_gmm(device=True)
    assert dev.step_count() == 1                   # the step count too
    after = (dev.states(), dev.weights(), dev.raw_weights(3000), dev.resample_indices())
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    md, cd = dev.get_gmm()                         # tdr_filter_get_gmm returns the device fit
    assert len(md) == dev.num_gaussians() >= 1 and cd.shape == (len(md), 3, 3)
    assert np.all(cd[:, 2, 2] == 1) and np.all(cd[:, 2, :2] == 0) and np.all(cd[:, :2, 2] == 0)
    host.compute_gmm(device=False)
    _check_twins(dev, host, "after a step")
    for f in (dev, host):                          # the next step: the twin never ran a device fit
        f.propagate(0.5, -0.1, 0.01)
        f.update(scan, 1.0, n_target=host.adaptive_count())
    assert dev.num_particles() == host.num_particles()
    assert np.array_equal(dev.states().view(np.uint8), host.states().view(np.uint8))
    assert np.array_equal(dev.weights(), host.weights(), equal_nan=True)
    n = 3000
    assert np.array_equal(dev.raw_weights(n), host.raw_weights(n), equal_nan=True)


def test_a_filter_without_particles_is_left_alone(scene):
    from top_down_renderer_amd import batch
    cfg, sc, m, mc = scene
    f = batch.FilterHandle(m, 100, _params(sc.class_maps.shape[0]), seed=5)
    f.set_states(np.zeros(0, batch.STATE_DTYPE))
    assert f.num_particles() == 0
    f.compute_gmm(device=True)                     # TDR_OK
    assert len(f.get_gmm()[0]) == 0 and f.num_gaussians() == 1


# ---- the batch -------------------------------------------------------------------------------------------------------------------
def _gmm_bytes(f):
    md, cd = f.get_gmm()
    return f.num_gaussians(), md.tobytes(), cd.tobytes(), f.adaptive_count()


def _batch_pairs(scene, K):
    """K twin pairs: different n, start counts, polar and Cartesian, two maps, one filter without particles."""
    from top_down_renderer_amd import batch
    cfg, sc, m, mc = scene
    ncls = sc.class_maps.shape[0]
    names = ["two", "three", "small", "one"]
    counts = [800, 3000, 37, 1000, 19, 1001, 20000, 40]
    pairs = []
    for i in range(K):
        cart = i % 3 == 1
        if K >= 3 and i == 2:
            st, start = np.zeros(0, batch.STATE_DTYPE), 1
            pair = _twins(mc if cart else m, ncls, st, start, cart=cart, n_max=64)
        else:
            n = counts[i % len(counts)]
            name = "small" if n <= 40 else names[i % len(names)]
            pair = _twins(mc if cart else m, ncls, _states(_fixture(name)[1], n), 1 + i % 4, cart=cart)
        pairs.append(pair)
    return pairs


@pytest.mark.parametrize("K", [1, 3, 64])
def test_batch_equals_every_filter_s_own_device_fit(scene, K):
    from top_down_renderer_amd import batch
    pairs = _batch_pairs(scene, K)
    batch.compute_gmm_batch([p[0] for p in pairs])
    for a, b in pairs:
        b.compute_gmm(device=True)
    for i, (a, b) in enumerate(pairs):
        assert _gmm_bytes(a) == _gmm_bytes(b), i
    if K >= 3:
        assert pairs[2][0].num_particles() == 0 and len(pairs[2][0].get_gmm()[0]) == 0
    # the same batch in reversed order (fresh twins: a fit moves num_gaussians)
    again = _batch_pairs(scene, K)
    batch.compute_gmm_batch([p[0] for p in again][::-1])
    for i, ((a, _), (c, _)) in enumerate(zip(pairs, again)):
        assert _gmm_bytes(a) == _gmm_bytes(c), i


def test_batch_refusals_change_no_filter(scene):
    from top_down_renderer_amd import _lib, batch
    L = _lib.load()
    cfg, sc, m, mc = scene
    ncls = sc.class_maps.shape[0]
    _, xyt = _fixture("two")
    a, b = _twins(m, ncls, _states(xyt, 800), 1)
    a.compute_gmm(device=True)
    b.compute_gmm(device=True)
    before = (_gmm_bytes(a), _gmm_bytes(b))
    arr = (C.c_void_p * 3)(a.h, None, b.h)
    assert L.tdr_batch_compute_gmm(arr, 3, None) != 0 and "is null" in L.tdr_last_error().decode()
    arr = (C.c_void_p * 3)(a.h, b.h, a.h)
    assert L.tdr_batch_compute_gmm(arr, 3, None) != 0 and "twice" in L.tdr_last_error().decode()
    assert L.tdr_batch_compute_gmm(None, 2, None) != 0
    assert L.tdr_batch_compute_gmm(arr, 0, None) != 0
    assert (_gmm_bytes(a), _gmm_bytes(b)) == before


def test_batch_refuses_a_sharded_filter_which_its_own_call_fits(scene):
    """A one-rank RCCL communicator, like tests/test_sharded_handle.py's one-rank case."""
    from top_down_renderer_amd import _lib
    L = _lib.load()
    cfg, sc, m, mc = scene
    ncls = sc.class_maps.shape[0]
    _, xyt = _fixture("two")
    a, b = _twins(m, ncls, _states(xyt, 800), 1)
    a.compute_gmm(device=True)
    b.compute_gmm(device=True)
    before = (_gmm_bytes(a), _gmm_bytes(b))
    uid = (C.c_char * 128)()
    _lib.check(L.tdr_comm_rccl_unique_id(uid))
    comm, f = C.c_void_p(), C.c_void_p()
    _lib.check(L.tdr_comm_create_rccl(1, 0, uid, C.byref(comm)))
    fp = _params(ncls)
    _lib.check(L.tdr_filter_create_sharded(m.h, 800, C.byref(fp), 7, comm, C.byref(f)))
    try:
        st = _states(xyt, 800)
        _lib.check(L.tdr_filter_set_states(f, _p(st), len(st)))
        arr = (C.c_void_p * 3)(a.h, f, b.h)
        assert L.tdr_batch_compute_gmm(arr, 3, None) != 0 and "sharded" in L.tdr_last_error().decode()
        assert (_gmm_bytes(a), _gmm_bytes(b)) == before
        k = C.c_int(-1)
        _lib.check(L.tdr_filter_get_gmm(f, 32, C.byref(k), None, None))
        assert k.value == 0
        # ... which its own call fits, like the plain filter's
        _lib.check(L.tdr_filter_compute_gmm_device(f))
        means, covs = np.zeros((32, 3), np.float32), np.zeros((32, 9), np.float32)
        _lib.check(L.tdr_filter_get_gmm(f, 32, C.byref(k), _p(means), _p(covs)))
        c, = _twins(m, ncls, st, 1)[:1]
        c.compute_gmm(device=True)
        mc_, cc_ = c.get_gmm()
        assert k.value == len(mc_) and means[: k.value].tobytes() == mc_.tobytes()
        assert covs[: k.value].tobytes() == cc_.tobytes()
    finally:
        L.tdr_filter_destroy(f)
        L.tdr_comm_destroy(comm)


# ---- the Python mirror ------------------------------------------------------------------------------------------------------------
def test_python_filter_compute_gmm_on_the_device_equals_the_handle(scene, kern):
    import top_down_renderer_amd as pkg
    cfg, sc, m, mc = scene
    _, xyt = _fixture("three")
    st = _states(xyt, 900)
    pm = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=kern)
    pm.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    f = pkg.ParticleFilter(len(st), pm, pkg.FilterParams(fixed_scale=1.0), kernels=kern, init_particles=False)
    f.set_states(st)
    h, = _twins(m, sc.class_maps.shape[0], st, 2)[:1]
    f.num_gaussians_ = 2
    f.computeGMM(device=True)
    h.compute_gmm(device=True)
    means, covs = f.getGMM()
    mh, ch = h.get_gmm()
    assert f.num_gaussians_ == h.num_gaussians() == 3
    assert means.tobytes() == mh.tobytes() and covs.tobytes() == ch.tobytes()


# ---- the node loop: gmm_every -----------------------------------------------------------------------------------------------------
LOOP_STEPS = 10
CONV_STEPS = 40     # the gmm_every = 2 core runs on to the step count tests/test_localizes.py's criterion is written for
LOOP_MOTION = (0.2, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def _loop_scenario():
    """2000 particles about the true pose of a 700 x 700 map, 100 x 25 bins; two more robots for the batch."""
    from top_down_renderer_amd import synth
    cfg = synth.Config("gmmloop", 20000, 6, 100, 25, 700, 2000, seed=95, res=4.0)
    sc = synth.make_scene(cfg, with_particles=False)
    robots = [synth.make_particles(cfg, sc.lab, sc.pose, np.random.default_rng(s), n=n, uniform_frac=0.0)
              for s, n in ((31, 2000), (32, 1500), (33, 2000))]
    return sc, cfg, robots


def _pcl(p):
    out = np.zeros((len(p), 8), np.float32)
    out[:, :3], out[:, 4] = p[:, :3], p[:, 3]
    return out


def _converged_on(sc, pose0, pose1, ml):
    """tests/test_localizes.py's criterion (its lines 102-108, after that test's 40 steps) on {x, y, theta, cov00, cov11}
    before and after and on the max-likelihood particle {x, y}."""
    cx, cy, th = sc.pose
    print(f"node loop after {CONV_STEPS} steps: true pose {sc.pose}, before {[float(v) for v in pose0]}, "
          f"after {[float(v) for v in pose1]}, max-likelihood particle {[float(v) for v in ml]}, "
          f"covariance ratio {(pose1[3] + pose1[4]) / (pose0[3] + pose0[4]):.3f}")
    assert np.hypot(pose1[0] - cx, pose1[1] - cy) < 30
    assert abs(np.angle(np.exp(1j * (float(pose1[2]) - th)))) < np.deg2rad(4)
    assert pose1[3] + pose1[4] < 0.1 * (pose0[3] + pose0[4])
    assert np.hypot(ml[0] - cx, ml[1] - cy) < 40


def test_node_loop_adapts_its_particle_count_cpp():
    """tests/cpp/facade_gmm.cpp: gmm_every = 0 is today's loop bit for bit; gmm_every = 2 resamples to the count of
    :151-157; TopDownRenderCoreBatch with gmm_every = 0, 2, 3 equals three standalone cores."""
    import subprocess
    import tempfile
    from top_down_renderer_amd import build
    build.build()
    pkg = os.path.join(ROOT, "top_down_renderer_amd")
    d = tempfile.mkdtemp(prefix="tdr_gmm_loop_")
    exe = os.path.join(d, "facade_gmm")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_gmm.cpp"), "-o", exe, "-L", pkg, "-ltdr_hip",
                    f"-Wl,-rpath,{pkg}"], check=True)
    sc, cfg, robots = _loop_scenario()
    open(os.path.join(d, "meta.txt"), "w").write(
        f"{cfg.ncls} {cfg.map_size} {cfg.map_size} {cfg.nb} {cfg.nr} {LOOP_STEPS} {CONV_STEPS} {cfg.map_resolution}\n")
    np.ascontiguousarray(np.transpose(sc.class_maps, (0, 2, 1)), np.float32).tofile(os.path.join(d, "maps.bin"))
    np.ascontiguousarray(sc.class_mask.T, np.uint8).tofile(os.path.join(d, "mask.bin"))
    np.asarray(LOOP_MOTION, np.float32).tofile(os.path.join(d, "motion.bin"))
    _pcl(sc.pts).tofile(os.path.join(d, "pts.bin"))
    for r, st in enumerate(robots):
        st.tofile(os.path.join(d, f"states_{r}.bin"))
    out = subprocess.run([exe, d], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split()
    assert out.stdout.strip().endswith("ok")
    rows = [ln.split() for ln in out.stdout.strip().split("\n")]
    poses = [[float(v) for v in r[1:]] for r in rows if r[0] == "pose"]
    counts = [int(r[2]) for r in rows if r[0] == "count"]
    stats = [(int(r[2]), int(r[3])) for r in rows if r[0] == "stats"]
    mls = [[float(v) for v in r[1:]] for r in rows if r[0] == "ml"]
    assert len(poses) == 2 and len(mls) == 1 and len(counts) == CONV_STEPS and len(stats) == LOOP_STEPS and lines
    assert counts[0] == counts[1] == 2000 and counts[LOOP_STEPS - 1] < 2000      # the count adapts once there is a mixture
    assert all(s == (3, 0) for s in stats), stats                    # all three robots stay on the batched path
    _converged_on(sc, poses[0], poses[1], mls[0])


def test_python_core_and_loop_batch_adapt_like_the_handle(kern):
    """The Python core with gmm_every = 2 (integer equality with tdr_adaptive_count_host, convergence), gmm_every = 0
    against a core built without the field, and batch.LoopBatch with gmm_every = 0, 2, 3 against three standalone loops."""
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.top_down_render_core import CoreConfig, TopDownRenderCore
    sc, cfg, robots = _loop_scenario()
    ncls, nb, nr = cfg.ncls, cfg.nb, cfg.nr
    lib = kern.lib

    def core(ccfg, st):
        pm = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=kern)
        c = TopDownRenderCore(ccfg, kernels=kern)
        c.initialize(pm, pkg.FilterParams(fixed_scale=1.0), sc.lut, init_particles=False)
        c.filter_.set_states(st)
        return c

    st0 = robots[0]
    a = core(CoreConfig(particle_count=len(st0), theta_bins=nb, range_bins=nr, seed=7), st0)                 # without the field
    b = core(CoreConfig(particle_count=len(st0), theta_bins=nb, range_bins=nr, seed=7, gmm_every=0), st0)
    c = core(CoreConfig(particle_count=len(st0), theta_bins=nb, range_bins=nr, seed=7, gmm_every=2), st0)
    pose0 = list(c.filter_.meanLikelihood()[:3]) + list(np.diag(c.filter_.computeMeanCov())[:2])
    for k in range(LOOP_STEPS):
        ea, eb = a.takeStep(sc.pts, LOOP_MOTION[:2], LOOP_MOTION[2]), b.takeStep(sc.pts, LOOP_MOTION[:2], LOOP_MOTION[2])
        assert ea.cov.tobytes() == eb.cov.tobytes() and ea.ml_state.tobytes() == eb.ml_state.tobytes(), k
        assert a.filter_.numParticles() == b.filter_.numParticles() == len(st0) and len(b.filter_.getGMM()[0]) == 0
        na, nb_ = a.filter_.numParticles(), b.filter_.numParticles()
        sa, sb = kern.states_to_host(a.filter_.st, na, st0.dtype), kern.states_to_host(b.filter_.st, nb_, st0.dtype)
        assert sa.tobytes() == sb.tobytes(), k
        means, covs = c.filter_.getGMM()
        before = c.filter_.numParticles()
        c.takeStep(sc.pts, LOOP_MOTION[:2], LOOP_MOTION[2])
        want = before if len(means) == 0 else int(lib.tdr_adaptive_count_host(
            _p(np.ascontiguousarray(covs, np.float32)), len(means), before, len(st0)))
        assert c.filter_.numParticles() == want, k
        assert (len(c.filter_.getGMM()[0]) > 0) == (k + 1 >= 2), k
    assert c.filter_.numParticles() < len(st0)
    for k in range(LOOP_STEPS, CONV_STEPS):     # on to the step count the convergence criterion is written for
        means, covs = c.filter_.getGMM()
        before = c.filter_.numParticles()
        c.takeStep(sc.pts, LOOP_MOTION[:2], LOOP_MOTION[2])
        assert c.filter_.numParticles() == int(lib.tdr_adaptive_count_host(
            _p(np.ascontiguousarray(covs, np.float32)), len(means), before, len(st0))), k
    pose1 = list(c.filter_.meanLikelihood()[:3]) + list(np.diag(c.filter_.computeMeanCov())[:2])
    _converged_on(sc, pose0, pose1, c.filter_.maxLikelihood()[:2])

    # LoopBatch against standalone loops over handles
    ang_res = float(np.float32(2 * np.pi / nb))
    m = batch.MapHandle(sc.class_maps, sc.class_mask, cfg.map_resolution)
    m.sample_pts_polar(nb, nr, ang_res)
    every = (0, 2, 3)
    cfgs = [CoreConfig(particle_count=len(st), theta_bins=nb, range_bins=nr, gmm_every=g) for st, g in zip(robots, every)]
    fb, ft, rb, rt, cores = [], [], [], [], []
    for i, st in enumerate(robots):
        for fl in (fb, ft):
            f = batch.FilterHandle(m, len(st), _params(ncls), seed=11 + 2 * i)
            f.set_states(st)
            fl.append(f)
        rb.append(batch.Renderer(sc.lut))
        rt.append(batch.Renderer(sc.lut))
        cores.append(TopDownRenderCore(cfgs[i]))
    loop = batch.LoopBatch(fb, rb, cfgs, ang_res, ncls, nb, nr)
    clouds = [(_pcl(sc.pts), 8, 4)] * 3
    for k in range(LOOP_STEPS):
        eb = loop.take_step(clouds, [LOOP_MOTION] * 3)
        assert loop.stats == batch.last_stats() == (3, 0), k      # the fit leaves tdr_batch_last_stats alone
        for i, (f, r, cr) in enumerate(zip(ft, rt, cores)):
            cr.last_res_ = cr.current_range_scale_
            res = float(cr.current_range_scale_)
            r.render_polar(clouds[i][0], 8, 4, res, ang_res, ncls, nb, nr)
            f.propagate(*LOOP_MOTION)
            f.update(r, res, n_target=f.adaptive_count() if every[i] else -1)
            cr.filter_ = batch.HandleView(f)
            et = cr.publishPoseEst()
            cr.filter_ = None
            if cr.countStepAndGmmDue():
                f.compute_gmm(device=True)
            assert eb[i].cov.tobytes() == et.cov.tobytes() and eb[i].ml_state.tobytes() == et.ml_state.tobytes(), (k, i)
            assert (eb[i].range_scale, eb[i].froze_scale, eb[i].converged) == (et.range_scale, et.froze_scale, et.converged)
            assert fb[i].num_particles() == f.num_particles(), (k, i)
            assert fb[i].states().tobytes() == f.states().tobytes(), (k, i)
            assert _gmm_bytes(fb[i]) == _gmm_bytes(f), (k, i)
    assert len(fb[0].get_gmm()[0]) == 0 and fb[0].num_particles() == len(robots[0])
    assert fb[1].num_particles() < len(robots[1]) and fb[2].num_particles() < len(robots[2])
