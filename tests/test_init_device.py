"""Particle initialisation on the device (csrc/tdr_init.hip): ParticleFilter::initializeParticles' serial loop of
rejection-sampled StateParticle constructions (src/particle_filter.cpp:57-71, src/state_particle.cpp:3-49) run as a parallel
chain over the reference's std::mt19937 stream.  Everything is compared with the serial host loop (tdr_init_particles_host)
byte for byte: the states, and the generator's position afterwards.  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

INF = float("inf")
TDR_OK = 0


def _lib():
    from top_down_renderer_amd import _lib
    return _lib.load()


def _check(rc):
    from top_down_renderer_amd._lib import check
    check(rc)


@pytest.fixture(scope="module")
def k():
    import torch
    from top_down_renderer_amd.kernels import HipKernels
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels()


@pytest.fixture(autouse=True)
def _restore_tuning():
    L = _lib()
    dev, window = L.tdr_config_tuning(b"init_device", -1), L.tdr_config_tuning(b"init_window_words", -1)
    yield
    L.tdr_config_tuning(b"init_device", dev)
    L.tdr_config_tuning(b"init_window_words", window)


def _params(ncls, mode="uniform", fixed_scale=1.0, theta=None, centre=(80.0, 60.0), cov=12.0):
    from top_down_renderer_amd._lib import FilterParamsC
    fp = FilterParamsC()
    fp.pos_cov, fp.theta_cov, fp.regularization = 0.3, np.pi / 100, 0.15
    fp.init_pos_px_x = fp.init_pos_px_y = fp.init_pos_px_cov = -1.0
    if mode != "uniform":
        fp.init_pos_px_x, fp.init_pos_px_y, fp.init_pos_px_cov = centre[0], centre[1], cov
    fp.init_pos_m_x = fp.init_pos_m_y = INF
    fp.init_pos_deg_theta, fp.init_pos_deg_cov = (INF, 10.0) if theta is None else (theta, 7.5)
    fp.fixed_scale, fp.scale_log_min, fp.scale_log_max = fixed_scale, -0.1, 1.0
    fp.num_classes = ncls
    for i in range(ncls):
        fp.class_weights[i] = 1.0
    return fp


def _small_map(size=160, ncls=4, seed=3):
    """A synthetic map (roads, rectangles, unknown holes) with a road along its top and left border, so that positions
    clamped to 0 land on road."""
    from top_down_renderer_amd import synth
    lab = synth.make_label_image(size, ncls, np.random.default_rng(seed))
    lab[:3, :] = 1
    lab[:, :3] = 1
    maps, mask = synth.label_to_maps(lab, ncls)
    return maps, mask


def _words_of(rng):
    L = _lib()
    w = np.zeros(640, np.uint32)
    _check(L.tdr_rng_get_state_host(rng, w.ctypes.data_as(C.c_void_p)))
    return w


def _seeded_words(seed, burn):
    L = _lib()
    rng = C.c_void_p(L.tdr_rng_create(C.c_uint32(seed)))
    for _ in range(burn):
        L.tdr_rng_uniform_host(rng)
    w = _words_of(rng)
    L.tdr_rng_destroy(rng)
    return w


def _host_init(words, maps, res, fp, max_num):
    """tdr_init_particles_host from the engine state `words`: (states, rc, engine words afterwards)."""
    from top_down_renderer_amd.synth import STATE_DTYPE
    L = _lib()
    ncls, rows, cols = maps.shape
    maps_cm = np.ascontiguousarray(np.transpose(maps, (0, 2, 1)), np.float32)
    rng = C.c_void_p(L.tdr_rng_create(C.c_uint32(1)))
    _check(L.tdr_rng_set_state_host(rng, words.ctypes.data_as(C.c_void_p)))
    out = np.zeros(max_num + 16, STATE_DTYPE)
    n = C.c_int64(0)
    rc = L.tdr_init_particles_host(rng, maps_cm.ctypes.data_as(C.c_void_p), ncls, rows, cols, C.c_float(res), C.byref(fp),
                                   max_num, out.ctypes.data_as(C.c_void_p), C.byref(n))
    after = _words_of(rng)
    L.tdr_rng_destroy(rng)
    return out[: n.value].copy(), rc, after


def _dev_init(k, words, dmap, fp, max_num, lo=0, hi=None):
    """tdr_k_init_particles from the same state: (states [lo, hi), rc, count, state words afterwards)."""
    from top_down_renderer_amd.synth import STATE_DTYPE
    L = _lib()
    count = int(L.tdr_init_particles_count(C.byref(fp), max_num))
    hi = count if hi is None else hi
    state = k.to_device(words.view(np.int32))
    st = k.zeros((7, max(hi - lo, 1)))
    ws = k.empty((int(L.tdr_init_workspace_bytes()),), __import__("torch").uint8)
    n = C.c_int64(-1)
    rc = L.tdr_k_init_particles(C.c_void_p(state.data_ptr()), C.byref(dmap.desc), C.byref(fp), max_num, lo, hi,
                                C.c_void_p(st.data_ptr()), st.shape[1], C.byref(n), C.c_void_p(ws.data_ptr()), k.stream())
    k.synchronize()
    states = k.states_to_host(st, hi - lo, STATE_DTYPE) if rc == TDR_OK and hi > lo else np.zeros(0, STATE_DTYPE)
    return states, rc, n.value, state.cpu().numpy().view(np.uint32).copy()


def _cells(states, res):
    """The cell getClassesAtPoint reads for each state: ((int)((float)(int)y / res), (int)((float)(int)x / res))."""
    r = np.float32(res)
    cx = (states["init_x_px"].astype(np.int32).astype(np.float32) / r).astype(np.int32)
    cy = (states["init_y_px"].astype(np.int32).astype(np.float32) / r).astype(np.int32)
    return cy, cx


@pytest.fixture(scope="module")
def small(k):
    maps, mask = _small_map()
    return maps, mask, {res: k.make_map(maps, mask, res) for res in (1.0, 0.7)}


# ---- 1. kernel level against the host loop --------------------------------------------------------------------------------
_unknown_hits = []


@pytest.mark.gpu
@pytest.mark.parametrize("res", [1.0, 0.7])
@pytest.mark.parametrize("theta", [None, 30.0])
@pytest.mark.parametrize("fixed_scale", [1.0, -1.0])
@pytest.mark.parametrize("mode", ["uniform", "normal", "normal_border"])
def test_device_loop_is_the_host_loop(k, small, mode, fixed_scale, theta, res):
    maps, mask, dmaps = small
    centre = {"normal": (80.0, 60.0), "normal_border": (2.5, 150.0)}.get(mode, (80.0, 60.0))
    fp = _params(maps.shape[0], "uniform" if mode == "uniform" else "normal", fixed_scale, theta, centre, 15.0)
    for i, n in enumerate((1, 9, 10, 1000, 20_003)):
        words = _seeded_words(1000 + 7 * i + (fixed_scale < 0), burn=(311 * i) % 700)
        ref, rc_h, after_h = _host_init(words, maps, res, fp, n)
        got, rc_d, cnt, after_d = _dev_init(k, words, dmaps[res], fp, n)
        assert rc_h == rc_d == TDR_OK
        assert cnt == len(ref), (n, cnt, len(ref))
        assert got.tobytes() == ref.tobytes(), (mode, fixed_scale, theta, res, n)
        assert np.array_equal(after_d[:625], after_h[:625]) and after_d[625] == 0, "generator position differs"
        if mode == "uniform" and len(ref):
            cy, cx = _cells(ref, res)
            inside = (cy < maps.shape[1]) & (cx < maps.shape[2])
            _unknown_hits.append(int(mask[cy[inside], cx[inside]].sum()))
        if mode == "normal_border" and n == 20_003:
            assert (ref["init_x_px"] == 0).any(), "no position was clamped"
    if mode == "uniform" and n == 20_003:
        assert sum(_unknown_hits) > 0, "no uniform-path particle landed on an unknown cell"


# ---- 2. windows: constructions that span several windows --------------------------------------------------------------------
def _sparse_map(size=256, roads=16, seed=5):
    rng = np.random.default_rng(seed)
    maps = np.full((2, size, size), 5.0, np.float32)
    maps[0] = 0.0
    cells = rng.choice(size * size, roads, replace=False)
    maps[1].reshape(-1)[cells] = 0.0
    return maps, np.zeros((size, size), np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("window,fixed_scale,theta,n", [(4096, 1.0, None, 200), (4096, -1.0, 45.0, 20),
                                                        (6144, 1.0, 12.0, 60)])
def test_constructions_longer_than_a_window(k, window, fixed_scale, theta, n):
    L = _lib()
    maps, mask = _sparse_map()
    dmap = k.make_map(maps, mask, 1.0)
    assert L.tdr_config_tuning(b"init_window_words", window) == window
    fp = _params(2, "uniform", fixed_scale, theta)
    words = _seeded_words(4242, 17)
    ref, rc_h, after_h = _host_init(words, maps, 1.0, fp, n)
    got, rc_d, cnt, after_d = _dev_init(k, words, dmap, fp, n)
    assert rc_h == rc_d == TDR_OK and cnt == len(ref) > 0
    assert got.tobytes() == ref.tobytes()
    assert np.array_equal(after_d[:626], np.append(after_h[:625], 0))


# ---- 7. edge cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_map_without_road_and_empty_calls(k):
    L = _lib()
    maps, mask = _small_map(64)
    maps_noroad = maps.copy()
    maps_noroad[1] = 3.0
    fp = _params(maps.shape[0], "uniform", 1.0, None)
    words = _seeded_words(9, 3)
    _, rc_h, _ = _host_init(words, maps_noroad, 1.0, fp, 50)
    _, rc_d, _, after = _dev_init(k, words, k.make_map(maps_noroad, mask, 1.0), fp, 50)
    assert rc_h == rc_d != TDR_OK
    assert np.array_equal(after, words), "a refused call moved the generator"
    # unknown scale with fewer than 10 particles: no group, no draw
    fp = _params(maps.shape[0], "uniform", -1.0, 20.0)
    dmap = k.make_map(maps, mask, 1.0)
    for n in (0, 1, 9):
        ref, rc_h, after_h = _host_init(words, maps, 1.0, fp, n)
        got, rc_d, cnt, after_d = _dev_init(k, words, dmap, fp, n)
        assert rc_h == rc_d == TDR_OK and cnt == len(ref) == 0
        assert np.array_equal(after_d, words) and np.array_equal(after_h[:625], words[:625])
    # a slice of the particles: exactly those states
    fp = _params(maps.shape[0], "uniform", -1.0, None)
    ref, _, after_h = _host_init(words, maps, 1.0, fp, 100)
    got, rc_d, cnt, after_d = _dev_init(k, words, dmap, fp, 100, lo=37, hi=81)
    assert rc_d == TDR_OK and cnt == 100
    assert got.tobytes() == ref[37:81].tobytes()
    assert np.array_equal(after_d[:625], after_h[:625])
    assert L.tdr_k_init_particles(None, None, None, 10, 0, 0, None, 0, None, None, None) != TDR_OK


# ---- 3. the filter: host loop and device loop, then three steps -------------------------------------------------------------
def _handle_map(maps, mask, nb=48, nr=20):
    L = _lib()
    ncls, H, W = maps.shape
    m = C.c_void_p()
    _check(L.tdr_map_create(C.byref(m)))
    maps_cm = np.ascontiguousarray(np.transpose(maps, (0, 2, 1)), np.float32)
    mask_cm = np.ascontiguousarray(mask.T, np.uint8)
    _check(L.tdr_map_set(m, maps_cm.ctypes.data_as(C.c_void_p), mask_cm.ctypes.data_as(C.c_void_p), ncls, H, W,
                         C.c_float(1.0), 0, 0))
    _check(L.tdr_map_sample_pts_polar(m, nb, nr, C.c_float(2 * np.pi / nb)))
    return m


def _filter_states(f, n):
    from top_down_renderer_amd.synth import STATE_DTYPE
    out = np.zeros(n, STATE_DTYPE)
    _check(_lib().tdr_filter_get_states(f, out.ctypes.data_as(C.c_void_p), n))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("fixed_scale,theta", [(1.0, None), (-1.0, 25.0)])
def test_filter_init_device_equals_host_and_steps_on(k, fixed_scale, theta):
    L = _lib()
    maps, mask = _small_map(200, 4, seed=11)
    ncls, nb, nr = maps.shape[0], 48, 20
    m = _handle_map(maps, mask, nb, nr)
    fp = _params(ncls, "uniform", fixed_scale, theta)
    N = 4000
    fs = []
    for dev in (0, 1):
        L.tdr_config_tuning(b"init_device", dev)
        f = C.c_void_p()
        _check(L.tdr_filter_create(m, N, C.byref(fp), 31, C.byref(f)))
        _check(L.tdr_filter_initialize_particles(f))
        fs.append(f)
    n = int(L.tdr_filter_num_particles(fs[0]))
    assert n == int(L.tdr_filter_num_particles(fs[1])) == N
    assert _filter_states(fs[0], n).tobytes() == _filter_states(fs[1], n).tobytes()
    rng = np.random.default_rng(2)
    for step in range(3):
        scan = np.zeros((ncls, nb * nr), np.float32)
        hit = rng.random((nb * nr,)) < 0.4
        scan[rng.integers(0, ncls, nb * nr)[hit], np.nonzero(hit)[0]] = rng.integers(1, 4, int(hit.sum()))
        res = []
        for f in fs:
            _check(L.tdr_filter_propagate(f, C.c_float(1.5), C.c_float(0.5), C.c_float(0.02)))
            _check(L.tdr_filter_update(f, scan.ctypes.data_as(C.c_void_p), None, C.c_float(1.0), -1))
            nn = int(L.tdr_filter_num_particles(f))
            raw = np.zeros(nn, np.float32)
            _check(L.tdr_filter_get_raw_weights(f, raw.ctypes.data_as(C.c_void_p), nn))
            idx = np.zeros(nn, np.int32)
            _check(L.tdr_filter_get_resample_indices(f, idx.ctypes.data_as(C.c_void_p), nn))
            res.append((raw.tobytes(), idx.tobytes(), _filter_states(f, nn).tobytes()))
        assert res[0] == res[1], f"step {step}"
    for f in fs:
        L.tdr_filter_destroy(f)
    L.tdr_map_destroy(m)


# ---- 4. Python ParticleFilter ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(fixed_scale=-1.0), dict(fixed_scale=1.0, init_pos_px_x=70.0, init_pos_px_y=40.0,
                                                             init_pos_px_cov=20.0, init_pos_deg_theta=-40.0)])
def test_python_filter_initialises_on_the_device(k, oracle, kw):
    import top_down_renderer_amd as pkg
    maps, mask = _small_map(180, 4, seed=8)
    om = oracle.OracleMap(maps, mask, 1.0)
    ref = oracle.initialize_particles(om, oracle.make_params(maps.shape[0], **kw), 2000, oracle.Rng(77))
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), maps, mask, kernels=k)
    f = pkg.ParticleFilter(2000, m, pkg.FilterParams(**kw), seed=77, kernels=k)
    assert f._rng_on_device
    assert f.numParticles() == len(ref)
    assert f.get_states().tobytes() == ref.tobytes()
    # the generator stands where the host loop leaves it: the next propagate draws what the oracle draws next
    L = _lib()
    L.tdr_config_tuning(b"init_device", 0)
    g = pkg.ParticleFilter(2000, m, pkg.FilterParams(**kw), seed=77, kernels=k)
    assert not g._rng_on_device
    for h in (f, g):
        h.propagate((1.0, -0.5), 0.01)
    assert f.get_states().tobytes() == g.get_states().tobytes()


# ---- 5. sharded: every rank runs the chain and keeps its slice --------------------------------------------------------------
@pytest.mark.gpu
def test_sharded_ranks_write_their_slices(k):
    L = _lib()
    vp = C.c_void_p
    maps, mask = _small_map(200, 4, seed=13)
    ncls = maps.shape[0]
    m = _handle_map(maps, mask)
    fp = _params(ncls, "normal", -1.0, 10.0, (100.0, 100.0), 30.0)
    N, world = 1006, 2    # the loop keeps 1000; each rank 500

    AG = C.CFUNCTYPE(C.c_int, vp, vp, vp, C.c_size_t, vp)
    BC = C.CFUNCTYPE(C.c_int, vp, vp, C.c_size_t, C.c_int, vp)

    class Ops(C.Structure):
        _fields_ = [("ctx", vp), ("all_gather", AG), ("broadcast", BC)]
    ops = Ops(None, AG(lambda *a: 1), BC(lambda *a: 1))   # initialisation exchanges nothing
    plain = C.c_void_p()
    _check(L.tdr_filter_create(m, N, C.byref(fp), 5, C.byref(plain)))
    _check(L.tdr_filter_initialize_particles(plain))
    n = int(L.tdr_filter_num_particles(plain))
    assert n == 1000
    full = _filter_states(plain, n)
    ranks, comms = [], []
    for rank in range(world):
        comm = vp()
        _check(L.tdr_comm_create(world, rank, C.byref(ops), C.byref(comm)))
        f = vp()
        _check(L.tdr_filter_create_sharded(m, N, C.byref(fp), 5, comm, C.byref(f)))
        _check(L.tdr_filter_initialize_particles(f))
        assert int(L.tdr_filter_num_particles(f)) == n and int(L.tdr_filter_num_local(f)) == n // world
        ranks.append(f)
        comms.append(comm)
    got = np.concatenate([_filter_states(f, n // world) for f in ranks])
    assert got.tobytes() == full.tobytes()
    # both ranks continue the same stream: a propagate moves every slice like the unsharded filter's
    for f in [plain] + ranks:
        _check(L.tdr_filter_propagate(f, C.c_float(2.0), C.c_float(-1.0), C.c_float(0.05)))
    full = _filter_states(plain, n)
    got = np.concatenate([_filter_states(f, n // world) for f in ranks])
    assert got.tobytes() == full.tobytes()
    for f in [plain] + ranks:
        L.tdr_filter_destroy(f)
    for c in comms:
        L.tdr_comm_destroy(c)
    L.tdr_map_destroy(m)


# ---- 6. full size: 2 000 000 particles on the synthetic 4000^2 map ---------------------------------------------------------
@pytest.mark.gpu
def test_two_million_particles_equal_the_host_loop(k):
    from top_down_renderer_amd import synth
    L = _lib()
    ncls, size, N = 4, 4000, 2_000_000
    lab = synth.make_label_image(size, ncls, np.random.default_rng(0)).astype(np.uint8)   # -1 -> 255: unknown
    lut = np.ascontiguousarray(synth.make_lut(ncls), np.int32)
    m = C.c_void_p()
    _check(L.tdr_map_create(C.byref(m)))
    _check(L.tdr_map_set_labels(m, lab.ctypes.data_as(C.c_void_p), size, size, lut.ctypes.data_as(C.c_void_p), 256, ncls,
                                C.c_float(1.0), 0, 0))
    fp = _params(ncls, "uniform", 1.0, None)
    fs = []
    for dev in (0, 1):
        L.tdr_config_tuning(b"init_device", dev)
        f = C.c_void_p()
        _check(L.tdr_filter_create(m, N, C.byref(fp), 2024, C.byref(f)))
        _check(L.tdr_filter_initialize_particles(f))
        assert int(L.tdr_filter_num_particles(f)) == N
        fs.append(f)
    a, b = _filter_states(fs[0], N), _filter_states(fs[1], N)
    assert a.tobytes() == b.tobytes()
    for f in fs:   # the generators stand at the same word
        _check(L.tdr_filter_propagate(f, C.c_float(1.0), C.c_float(0.0), C.c_float(0.0)))
    assert _filter_states(fs[0], N).tobytes() == _filter_states(fs[1], N).tobytes()
    for f in fs:
        L.tdr_filter_destroy(f)
    L.tdr_map_destroy(m)
