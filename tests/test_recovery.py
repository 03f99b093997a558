"""GPU: the recovery injection (csrc/tdr_recover.hip, csrc/tdr_host_recover.cpp; include/tdr.h, "recovery injection")
against its NumPy restatement (tests/recovery_ref.py), with ==: the road list, the injected states through the launchers,
the handle, the batch, the C++ classes (tests/cpp/facade_recovery.cpp) and the Python mirror; map updates; what is
refused; the node loop with recovery_every; and the closed loop of a kidnapped robot.
Sizes are chosen for where the kernels can go wrong (a lane, a wave less one, a wave, a wave plus one, several workgroups
with a ragged end, more slots than one pass of the grid), not for the workload."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import recovery_ref as RR
from test_recovery_ref import HAND_DRAW, HAND_SEED, hand_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "top_down_renderer_amd")
pytestmark = pytest.mark.gpu
F32 = np.float32
vp = C.c_void_p
SIZES = [1, 63, 64, 65, 4097, 100003]
FIELDS = ("init_x_px", "init_y_px", "dx_m", "dy_m", "theta", "scale")
FULL = 1 << 24


@pytest.fixture(scope="module")
def K():
    import torch
    from top_down_renderer_amd.kernels import HipKernels
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels()


# ---- the road list ---------------------------------------------------------------------------------------------------------------
def _road_maps(rows, cols, ncls, seed, share=0.2):
    """(ncls, rows, cols) maps whose class-1 values sit on both sides of the predicate's edge: 0, 0.5, the float below 1 are
    road; 1, the float above 1 and 3 are not."""
    rng = np.random.default_rng(seed)
    maps = rng.uniform(0.0, 50.0, (ncls, rows, cols)).astype(F32)
    vals = np.array([0.0, 0.5, np.nextafter(F32(1), F32(0)), 1.0, np.nextafter(F32(1), F32(2)), 3.0], F32)
    pick = np.where(rng.random((rows, cols)) < share, rng.integers(0, 3, (rows, cols)), rng.integers(3, 6, (rows, cols)))
    maps[1] = vals[pick]
    return maps


def _single(rows, cols, ncls, cells):
    maps = np.full((ncls, rows, cols), 7.0, F32)
    maps[1].ravel()[list(cells)] = 0.0
    return maps


ROAD_CASES = {
    "hand_5x5": lambda: hand_map(),
    "odd_67x131": lambda: _road_maps(67, 131, 3, 1),
    "many_blocks_1024": lambda: _road_maps(1024, 1024, 4, 2, share=0.13),
    "last_cell_only": lambda: _single(67, 131, 3, [67 * 131 - 1]),
    "first_cell_only": lambda: _single(67, 131, 3, [0]),
    "every_cell": lambda: np.zeros((3, 33, 257), F32),
    "two_classes": lambda: _road_maps(40, 300, 2, 3),
    "fifteen_classes": lambda: _road_maps(40, 300, 15, 4),
}


def _dev_map(K, maps, resolution=1.0):
    return K.make_map(maps, np.zeros(maps.shape[1:], np.uint8), resolution)


def _cells(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", list(ROAD_CASES))
def test_road_list_equals_flatnonzero(K, name):
    maps = ROAD_CASES[name]()
    want = np.flatnonzero(maps[1].ravel() < 1.0)
    assert np.array_equal(RR.road_cells(maps), want)
    got = _cells(K.road_cells(_dev_map(K, maps)))
    assert got.shape == want.shape and np.array_equal(got, want), name
    if name == "hand_5x5":
        assert got.tolist() == [3, 11, 24]
    if name == "every_cell":
        assert len(got) == 33 * 257
    if name == "last_cell_only":
        assert got.tolist() == [67 * 131 - 1]


def test_unknown_cells_count_as_road(K):
    """The unknown mask zeroes no distance by itself; a map built like the reference's (distance 0 on unknown cells,
    synth.label_to_maps) has them on the list."""
    from top_down_renderer_amd import synth
    lab = np.full((20, 30), 0, np.int8)
    lab[5, :] = 1
    lab[10:12, 3:9] = -1
    maps, mask = synth.label_to_maps(lab, 3)
    got = _cells(K.road_cells(K.make_map(maps, mask, 1.0)))
    want = np.flatnonzero(((lab == 1) | (lab < 0)).ravel())
    assert np.array_equal(got, want)


def test_a_map_without_road_or_without_class_1_is_refused(K):
    import torch
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import batch
    from top_down_renderer_amd._lib import TdrError
    maps = np.full((3, 20, 30), 5.0, F32)
    dm = _dev_map(K, maps)
    assert K.road_cells(dm).numel() == 0                     # the launcher: an empty list
    with pytest.raises(ValueError, match="no road"):
        pkg.TopDownMap(pkg.Params(resolution=1.0), maps, np.zeros((20, 30), np.uint8), kernels=K).roadCells()
    with pytest.raises(TdrError, match="no road"):
        batch.MapHandle(maps, np.zeros((20, 30), np.uint8)).road_cells()
    one = _dev_map(K, np.zeros((1, 20, 30), F32))
    cells, cnt, ws = K.empty((600,), torch.int32), K.zeros((1,), torch.int64), K.empty((64,), torch.uint8)
    rc = K.lib.tdr_k_map_road_cells(C.byref(one.desc), vp(cells.data_ptr()), vp(cnt.data_ptr()), vp(ws.data_ptr()), None)
    assert rc == -1 and "class 1" in K.lib.tdr_last_error().decode()
    assert K.lib.tdr_k_map_road_cells(C.byref(dm.desc), None, vp(cnt.data_ptr()), vp(ws.data_ptr()), None) == -1
    assert K.lib.tdr_map_road_workspace_bytes(20, 30) >= 8 and K.lib.tdr_map_road_workspace_bytes(0, 30) == 0


# ---- the injection kernel --------------------------------------------------------------------------------------------------------
def _states(n, seed):
    rng = np.random.default_rng(seed)
    st = np.zeros(n, RR.STATE_DTYPE)
    st["init_x_px"] = rng.normal(-300, 40, n)              # off the map: an injected slot cannot be mistaken for an old one
    st["init_y_px"] = rng.normal(-50, 40, n)
    st["dx_m"] = rng.normal(0, 8, n)
    st["dy_m"] = rng.normal(0, 8, n)
    st["theta"] = rng.uniform(-3, 3, n)
    st["scale"] = np.exp(rng.uniform(-0.3, 1.0, n))
    st["have_init"] = rng.random(n) < 0.9
    return st


def _to_planes(states, cap, fill):
    a = np.full((7, cap), fill, F32)
    n = len(states)
    for i, name in enumerate(FIELDS):
        a[i, :n] = states[name]
    a[6, :n] = states["have_init"].astype(F32)
    return a


@pytest.fixture(scope="module")
def inj_map(K):
    maps = _road_maps(67, 131, 3, 1)
    return maps, {res: _dev_map(K, maps, res) for res in (1.0, 2.0)}, RR.road_cells(maps)


@pytest.mark.parametrize("n", SIZES)
def test_injected_states_equal_the_restatement(K, inj_map, n):
    maps, dms, road_h = inj_map
    road = K.road_cells(dms[1.0])
    assert np.array_equal(_cells(road), road_h)
    st = _states(n, 10 + n)
    cap = n + 7
    cases = [(th, mode, 0, 5, 77, 1.0) for th in (0, 1, 1 << 23, FULL) for mode in (0, 1)]
    cases += [(1 << 23, 1, 12345, (1 << 32) + 5, HAND_SEED, 2.0), (FULL, 0, (1 << 31) - n, (1 << 63) + 9, (1 << 64) - 1, 2.0),
              (1 << 22, 0, 64, 1 << 40, 1 << 33, 1.0)]
    for th, mode, begin, draw, seed, res in cases:
        before = _to_planes(st, cap, -777.0)                 # sentinels behind n
        planes = K.to_device(before)
        got_cnt = K.inject(planes, n, dms[res], road, seed, draw, th, mode, slot_begin=begin)
        want, cnt = RR.inject(st, n, begin, road_h, 131, res, seed, draw, th, mode)
        got = planes.cpu().numpy()
        key = (n, th, mode, begin, draw, seed, res)
        assert got_cnt == cnt, key
        assert got.tobytes() == _to_planes(want, cap, -777.0).tobytes(), key
        changed = (got[:, :n] != before[:, :n]).any(axis=0)
        if th == 0:
            assert cnt == 0 and not changed.any()
        if th == FULL:
            assert cnt == n
        if th == 1:
            assert cnt <= 1                                   # one slot in 2^24 on average
        # every injected particle stands on road by the constructor's own test (power-of-two resolutions)
        sel = want["init_x_px"] >= 0
        assert int(sel.sum()) == cnt and RR.on_road(maps, res, want["init_x_px"][sel], want["init_y_px"][sel]).all(), key
        if cnt:
            assert (want["scale"][sel] == st["scale"][sel]).all()


def test_the_hand_worked_slots_on_the_device(K):
    from test_recovery_ref import HAND_THETA_BITS, HAND_XY, hand_states
    maps = hand_map()
    dm = _dev_map(K, maps, 2.0)
    road = K.road_cells(dm)
    st = hand_states()
    planes = K.to_device(_to_planes(st, 6, 0.0))
    assert K.inject(planes, 4, dm, road, HAND_SEED, HAND_DRAW, 1 << 23, 1) == 3
    got = planes.cpu().numpy()
    for i, (x, y) in HAND_XY.items():
        assert (float(got[0, i]), float(got[1, i])) == (x, y) and got[2, i] == 0 and got[3, i] == 0
        assert int(got[4, i:i + 1].view(np.uint32)[0]) == HAND_THETA_BITS[i] and got[6, i] == 1 and got[5, i] == st["scale"][i]
    assert got[:, [0, 4, 5]].tobytes() == _to_planes(st, 6, 0.0)[:, [0, 4, 5]].tobytes()


def test_same_words_whatever_the_launch(K, inj_map):
    """A slot's words do not depend on the grid: the whole set at once, the same set in two slices with their slot_begin,
    and as jobs of one table."""
    maps, dms, road_h = inj_map
    road = K.road_cells(dms[2.0])
    n, cut = 100003, 4097
    st = _states(n, 3)
    whole = K.to_device(_to_planes(st, n, 0.0))
    cnt = K.inject(whole, n, dms[2.0], road, 9, 3, 1 << 23, 0)
    a = K.to_device(_to_planes(st[:cut], cut + 3, 0.0))
    b = K.to_device(_to_planes(st[cut:], n - cut, 0.0))
    ca = K.inject(a, cut, dms[2.0], road, 9, 3, 1 << 23, 0)
    cb = K.inject(b, n - cut, dms[2.0], road, 9, 3, 1 << 23, 0, slot_begin=cut)
    w = whole.cpu().numpy()
    assert ca + cb == cnt and a.cpu().numpy()[:, :cut].tobytes() == w[:, :cut].tobytes()
    assert b.cpu().numpy().tobytes() == w[:, cut:].tobytes()
    a2 = K.to_device(_to_planes(st[:cut], cut + 3, 0.0))
    b2 = K.to_device(_to_planes(st[cut:], n - cut, 0.0))
    e = K.to_device(_to_planes(st[:5], 5, 0.0))
    got = K.inject_jobs([a2, b2, e], [cut, n - cut, 0], [dms[2.0]] * 3, [road] * 3, [9, 9, 9], [3, 3, 3], [1 << 23, 1 << 23, FULL], 0,
                        slot_begins=[0, cut, 0])
    assert got == [ca, cb, 0]
    assert a2.cpu().numpy().tobytes() == a.cpu().numpy().tobytes() and b2.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert e.cpu().numpy().tobytes() == _to_planes(st[:5], 5, 0.0).tobytes()


def test_launcher_refuses_bad_arguments(K, inj_map):
    import torch
    _, dms, _ = inj_map
    dm = dms[1.0]
    road = K.road_cells(dm)
    before = _to_planes(_states(8, 1), 8, 0.0)
    d = K.to_device(before)
    out = K.zeros((1,), torch.int64)
    L = K.lib

    def call(st=d, cap=8, n=8, begin=0, desc=dm.desc, rd=road, n_road=None, th=FULL, mode=0):
        return L.tdr_k_inject(vp(st.data_ptr()) if st is not None else None, cap, n, begin, C.byref(desc) if desc is not None else None,
                              vp(rd.data_ptr()) if rd is not None else None, road.numel() if n_road is None else n_road, 1, 2, th, mode,
                              vp(out.data_ptr()), None)

    one = _dev_map(K, np.zeros((1, 20, 30), F32))
    for rc in (call(st=None), call(rd=None), call(desc=None), call(n=9), call(n=-1), call(begin=-1), call(begin=(1 << 31) - 7),
               call(n_road=0), call(n_road=67 * 131 + 1), call(th=FULL + 1), call(mode=2), call(mode=-1), call(desc=one.desc)):
        assert rc == -1
    assert L.tdr_k_inject_jobs(None, 1, None) == -1
    K.synchronize()
    assert d.cpu().numpy().tobytes() == before.tobytes() and int(out.item()) == 0
    assert call(n=0) == 0 and call(th=0) == 0 and call(begin=(1 << 31) - 8, th=0) == 0
    K.synchronize()
    assert d.cpu().numpy().tobytes() == before.tobytes() and int(out.item()) == 0


# ---- the handle ------------------------------------------------------------------------------------------------------------------
N_H = 4097


@pytest.fixture(scope="module")
def scene():
    from top_down_renderer_amd import synth
    return synth.make_scene(synth.Config("recovery", 4000, 4, 36, 12, 300, 4096, seed=41, res=2.0))


@pytest.fixture(scope="module")
def facade_exe():
    from top_down_renderer_amd import build
    build.build()
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), "facade_recovery")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_recovery.cpp"), "-o", exe, "-L", PKG, "-ltdr_hip",
                    f"-Wl,-rpath,{PKG}"], check=True)
    return exe


def _handle(scene, kind, n_max, seed=5, m=None):
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.particle_filter import FilterParams
    cfg = scene.cfg
    if m is None:
        m = batch.MapHandle(scene.class_maps, scene.class_mask, cfg.map_resolution)
    r = batch.Renderer(scene.lut)
    if kind == "cart":
        m.set_window(24, 20)
        r.render_cart(scene.pts, 4, 3, cfg.res, cfg.ncls, 24, 20)
    else:
        m.sample_pts_polar(cfg.nb, cfg.nr, float(cfg.ang_res))
        r.render_polar(scene.pts, 4, 3, cfg.res, float(cfg.ang_res), cfg.ncls, cfg.nb, cfg.nr)
    f = batch.FilterHandle(m, n_max, FilterParams(fixed_scale=1.0 if kind == "fixed" else -1.0), seed=seed, cart=kind == "cart")
    return f, r


def _spread_states(scene, n, seed, free_scale):
    from top_down_renderer_amd import synth
    rng = np.random.default_rng(seed)
    st = synth.make_particles(scene.cfg, scene.lab, scene.pose, rng, n=n)
    if free_scale:
        st["scale"] = np.exp(rng.normal(0.0, 0.1, n)).astype(F32)
    return st


def _snapshot(f, n_w=None, states=True):
    """Everything the handle lets out (states=False: but the particle set and what is derived from it)."""
    n = f.num_particles()
    n_w = n if n_w is None else n_w
    means, covs = f.get_gmm()
    s = {"w": f.weights()[:n_w].tobytes(), "raw": f.raw_weights(n_w).tobytes(), "idx": f.resample_indices().tobytes(),
         "steps": f.step_count(), "gmm": means.tobytes() + covs.tobytes(), "n": n, "stats": f.weight_stats().tobytes()}
    if states:
        s["states"] = f.states().tobytes()
        s["mean_cov"] = b"".join(a.tobytes() for a in f.mean_cov())
    return s


def _rows(a):
    return np.frombuffer(a.tobytes(), np.uint8).reshape(len(a), -1)


def _ref_inject(scene, cur, p, mode, seed, draw):
    road = RR.road_cells(scene.class_maps)
    return RR.inject(cur, len(cur), 0, road, scene.cfg.map_size, scene.cfg.map_resolution, seed, draw, RR.threshold(p), mode)


@pytest.mark.parametrize("kind", ["polar", "cart", "fixed"])
def test_handle_injects_and_leaves_the_rest_alone(K, scene, kind, oracle):
    cfg = scene.cfg
    st = _spread_states(scene, N_H - 100, 7, kind != "fixed")
    pair = [_handle(scene, kind, N_H) for _ in range(2)]      # the twin makes the same calls without the injection
    for f, r in pair:
        with pytest.raises(Exception, match="no update yet"):
            f.weight_stats()
        f.set_states(st)
        f.propagate(0.3, 0.1, 0.005)
        f.update(r, cfg.res, 3001)                              # a resampled set of another size
        f.compute_gmm()
    (f, r), (twin, rt) = pair
    assert np.array_equal(f.map.road_cells(), RR.road_cells(scene.class_maps))
    stats = f.weight_stats()
    assert stats[5] > 0 and stats[2] > 0 and np.isclose(stats[1] / stats[5], stats[2], rtol=1e-6)      # mean = sum / num_valid
    for mode, p, seed in ((1, 0.25, 11), (0, 0.5, (1 << 40) + 3)):
        before = _snapshot(f, states=False)
        cur = f.states()
        want, cnt = _ref_inject(scene, cur, p, mode, seed, f.step_count())
        assert f.inject(p, mode, seed) == cnt and 0 < cnt < len(cur)
        got = f.states()
        assert got.tobytes() == want.tobytes(), (kind, mode)
        assert _snapshot(f, states=False) == before == _snapshot(twin, states=False), (kind, mode)
        # the launcher on the same states
        planes = K.to_device(_to_planes(cur, len(cur) + 5, 0.0))
        dm = K.make_map(scene.class_maps, scene.class_mask, cfg.map_resolution)
        assert K.inject(planes, len(cur), dm, K.road_cells(dm), seed, f.step_count(), RR.threshold(p), mode) == cnt
        assert planes.cpu().numpy().tobytes() == _to_planes(want, len(cur) + 5, 0.0).tobytes()
        # the generator stands where the twin's does: the slots that were not injected take the twin's noise
        f.propagate(0.3, 0.1, 0.005)
        twin.propagate(0.3, 0.1, 0.005)
        kept = (_rows(want) == _rows(cur)).all(axis=1)
        assert kept.sum() == len(cur) - cnt
        a, b = f.states(), twin.states()
        assert a[kept].tobytes() == b[kept].tobytes(), (kind, mode)
        assert f.step_count() == twin.step_count() == 1
        twin.set_states(a)                                      # the twin follows, for the next round
    # after the heading_mode 0 injection: the next scoring gives every particle it scores a heading, and its raw weights are
    # the oracle's on the same states (a particle behind a gate of the free scale has no weight and keeps none)
    cur = f.states()
    assert (cur["have_init"] == 0).sum() > 0
    f.compute_weights(r, cfg.res)
    post = f.states()
    raw = f.raw_weights(len(cur))
    om = oracle.OracleMap(scene.class_maps, scene.class_mask, cfg.map_resolution)
    fp = oracle.make_params(cfg.ncls, fixed_scale=1.0 if kind == "fixed" else -1.0)
    st_o = np.ascontiguousarray(cur.astype(oracle.STATE_DTYPE))
    if kind == "cart":   # the oracle has no Cartesian search of its own: its weights at all 40 candidates (tests/cart_ref.py)
        import cart_ref
        scan = oracle.raster_cart(scene.pts, cfg.res, scene.lut, cfg.ncls, 24, 20)
        w40 = cart_ref.oracle_candidate_weights(oracle, om, 24, 20, scan, cfg.res, fp, st_o)
        cart_ref.check_search(oracle, om, 24, 20, scan, cfg.res, fp, st_o, w40, np.ascontiguousarray(post.astype(oracle.STATE_DTYPE)), raw)
    else:                # the oracle's own search on the same states
        scan = oracle.raster_polar(scene.pts, cfg.res, cfg.ang_res, scene.lut, cfg.ncls, cfg.nb, cfg.nr)
        tab = oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res, cfg.map_resolution)
        ref = oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan, cfg.res, fp, st_o)
        ok = ~np.isnan(ref) & (ref != 0)
        assert np.array_equal(np.isnan(raw), np.isnan(ref)) and np.array_equal(raw == 0, ref == 0) and ok.any()
        assert np.array_equal(post["have_init"], st_o["have_init"])
        if kind == "fixed":
            assert (post["have_init"] == 1).all()
        same = post["theta"] == st_o["theta"]
        err = np.abs(raw[ok & same] - ref[ok & same]) / np.abs(ref[ok & same])
        assert err.max(initial=0.0) <= 1e-5, (kind, err.max())
        if not same.all():   # another candidate of the search: the weight is the oracle's at that rotation, a near-tie
            st2 = st_o.copy()
            st2["theta"], st2["have_init"] = post["theta"], 1
            ref2 = oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan, cfg.res, fp, st2)
            d = ok & ~same
            assert (np.abs(raw[d] - ref2[d]) / np.abs(ref2[d])).max(initial=0.0) <= 1e-5
    f.update(r, cfg.res)
    assert (f.states()["have_init"] == 1).all() and f.step_count() == 2


def test_handle_on_a_map_with_an_odd_number_of_cells():
    """67 x 131 = 8777 cells, 5 x 5 = 25: the handle's own list and count buffers, not the launcher's tensors."""
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.particle_filter import FilterParams
    for maps, res in ((_road_maps(67, 131, 3, 1), 2.0), (hand_map(), 1.0), (_single(67, 131, 3, [67 * 131 - 1]), 1.0)):
        rows, cols = maps.shape[1:]
        assert rows * cols % 2 == 1
        m = batch.MapHandle(maps, np.zeros((rows, cols), np.uint8), res)
        m.sample_pts_polar(36, 12, 2 * np.pi / 36)
        want_road = RR.road_cells(maps)
        assert np.array_equal(m.road_cells(), want_road)
        f = batch.FilterHandle(m, 4200, FilterParams(fixed_scale=1.0), seed=3)
        st = _states(4097, 5)
        f.set_states(st)
        for p, mode, seed in ((0.5, 1, 21), (1.0, 0, (1 << 60) + 1)):
            cur = f.states()
            want, cnt = RR.inject(cur, len(cur), 0, want_road, cols, res, seed, 0, RR.threshold(p), mode)
            assert f.inject(p, mode, seed) == cnt and f.states().tobytes() == want.tobytes(), (rows, cols, p, mode)
        assert np.array_equal(m.road_cells(), want_road)      # the cached list


def test_recovery_step_tracks_injects_and_resets(scene):
    from top_down_renderer_amd._lib import RecoveryParamsC, RecoveryStateC
    cfg = scene.cfg
    f, r = _handle(scene, "fixed", 2000)
    f.set_states(_spread_states(scene, 2000, 9, False))
    rp = RecoveryParamsC(0.25, 0.5, 0.25, 1, 99)
    s, t = RecoveryStateC(0.0, 0.0), RR.Tracker(0.25, 0.5, 0.25)
    f.propagate(0.3, 0.1, 0.005)
    f.update(r, cfg.res)
    w = float(f.weight_stats()[2])
    before = f.states()
    assert f.recovery_step(s, rp) == (0.0, 0) and t.track(w) == 0.0      # the first update: both averages take the mean
    assert (s.w_slow, s.w_fast) == (w, w) == (t.w_slow, t.w_fast) and f.states().tobytes() == before.tobytes()
    s.w_slow, s.w_fast = 4 * w, 2 * w                                     # a filter whose weights have dropped
    t.w_slow, t.w_fast = 4 * w, 2 * w
    p = t.track(w)
    assert 0 < p <= 0.25
    want, cnt = _ref_inject(scene, before, p, 1, 99, f.step_count())
    assert f.recovery_step(s, rp) == (p, cnt) and cnt > 0
    assert f.states().tobytes() == want.tobytes() and (s.w_slow, s.w_fast) == (0.0, 0.0)


# ---- map updates ------------------------------------------------------------------------------------------------------------------
def _img(lab):
    return lab[::-1].copy()      # a label image's row 0 is the top: the map's last row


SIDE = 256


def _label_scene():
    """The labels in MAP orientation (row r = map row r): two roads across the map and a stub.  The stub is small enough
    for its removal to stay on the incremental path (the cells within 50 px of it are a fifth of the map)."""
    lab = np.zeros((SIDE, SIDE), np.uint8)
    lab[10:14, :] = 1
    lab[:, 40:44] = 1
    lab[200:204, 100:140] = 1
    lut = np.arange(256, dtype=np.int32)
    lut[3:] = -1                         # raw ids 0..2 are the classes; everything above is unlabelled
    return lab, lut


def _on_cells(states):
    return states["init_y_px"].astype(np.int64) * SIDE + states["init_x_px"].astype(np.int64)


@pytest.mark.parametrize("how", ["patch", "incremental", "set_labels", "fuser"])
def test_no_particle_lands_on_a_removed_road_cell(how):
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.particle_filter import FilterParams
    lab, lut = _label_scene()
    m = batch.MapHandle.from_labels(_img(lab), lut, 3)
    m.sample_pts_polar(36, 12, 2 * np.pi / 36)
    f = batch.FilterHandle(m, 5000, FilterParams(fixed_scale=1.0), seed=3)
    st = np.zeros(5000, RR.STATE_DTYPE)
    st["scale"], st["have_init"] = 1.0, 1
    st["init_x_px"] = st["init_y_px"] = -5.0
    f.set_states(st)
    road0 = m.road_cells()
    assert np.array_equal(road0, np.flatnonzero((lab == 1).ravel()))
    assert f.inject(1.0, 1, 1) == 5000
    assert np.isin(_on_cells(f.states()), road0).all() and len(np.unique(_on_cells(f.states()))) > 400
    lab2 = lab.copy()
    lab2[200:204, 100:140] = 0           # the stub goes
    removed = np.flatnonzero((lab == 1).ravel() & (lab2 != 1).ravel())
    if how == "patch":
        assert f.patch_map_labels(_img(lab2)[SIDE - 204:SIDE - 200, 100:140], SIDE - 204, 100, (0, 0)) == len(removed) == 160
    elif how == "incremental":
        assert f.update_map_labels_incremental(_img(lab2), lut, 3, 1.0, (0, 0)) == len(removed)
    elif how == "set_labels":
        f.update_map_labels(_img(lab2), lut, 3, 1.0, (0, 0))
    else:
        from top_down_renderer_amd import fuse
        fz = fuse.MapFuser(m, class_label=[0, 1, 2], min_votes=1)
        imgs = np.zeros((3, 40, 40), F32)
        imgs[0] = 5.0                    # a Cartesian scan that saw class 0 all around a pose on the stub
        assert fz.add_images(imgs, False, (120.0, 202.0, 0.0, 1.0), 1.0)[0] > 0
        assert fz.apply([f]) > 0
        lab2 = fz.labels()[::-1]         # the fused labels, in map orientation
        removed = np.flatnonzero((lab == 1).ravel() & (lab2 != 1).ravel())
        assert len(removed) > 0
    road1 = m.road_cells()
    assert np.array_equal(road1, np.flatnonzero((lab2 == 1).ravel()))
    assert len(road1) < len(road0) and not np.isin(road1, removed).any()
    f.set_states(st)
    assert f.inject(1.0, 0, 2) == 5000
    cells = _on_cells(f.states())
    assert np.isin(cells, road1).all() and not np.isin(cells, removed).any()


# ---- the batch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 8])
def test_batch_equals_the_single_calls(scene, k):
    from top_down_renderer_amd import batch, synth
    other = synth.make_scene(synth.Config("recovery2", 2000, 4, 36, 12, 200, 1024, seed=43, res=2.0, map_resolution=2.0))
    sizes = [4097, 65, 100003, 1, 63, 64, 2000, 129][:k]
    ps = [0.25, 1.0, 0.05, 1.0, 0.0, 0.5, 2.0 ** -24, 0.75][:k]
    seeds = [100 + i if i % 2 else (1 << 50) + i for i in range(k)]
    maps = [batch.MapHandle(sc.class_maps, sc.class_mask, sc.cfg.map_resolution) for sc in (scene, other)]
    for mode in (0, 1):
        groups = []
        for _ in range(2):
            fs = []
            for i, n in enumerate(sizes):
                sc = other if i % 3 == 1 else scene
                f, _ = _handle(sc, "cart" if i == 2 else "polar", n + i, seed=30 + i, m=maps[1] if sc is other else maps[0])
                f.set_states(_spread_states(sc, n, 40 + i, True))
                fs.append(f)
            groups.append(fs)
        single, batched = groups
        cur = [f.states() for f in single]
        counts = [f.inject(p, mode, s) for f, p, s in zip(single, ps, seeds)]
        got = batch.inject(batched, ps, mode, seeds)
        assert got.tolist() == counts, (k, mode)
        for i, (a, b) in enumerate(zip(single, batched)):
            sc = other if i % 3 == 1 else scene
            want, cnt = _ref_inject(sc, cur[i], ps[i], mode, seeds[i], 0)
            assert cnt == counts[i] and a.states().tobytes() == b.states().tobytes() == want.tobytes(), (k, mode, i)
        assert batch.inject(batched[::-1], ps[::-1], mode, seeds[::-1], count=False) is None      # no read-back
        for a, b in zip(single, batched):
            assert a.states().tobytes() == b.states().tobytes()      # the same draw again: the same particles


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_change_nothing(scene):
    from top_down_renderer_amd import batch
    from top_down_renderer_amd._lib import RecoveryParamsC, RecoveryStateC
    from top_down_renderer_amd.particle_filter import FilterParams, RecoveryParams, recovery_params_c
    f, r = _handle(scene, "polar", 300)
    g, _ = _handle(scene, "polar", 300, seed=6)
    st = _spread_states(scene, 256, 3, True)
    for h in (f, g):
        h.set_states(st)
    f.propagate(0.1, 0.0, 0.0)
    f.update(r, scene.cfg.res)
    L = f.L
    before, before_g = _snapshot(f), g.states().tobytes()
    out = C.c_int64(777)
    pout = C.c_double(777.0)
    o2 = np.full(2, 777, np.int64)
    arr2 = (vp * 2)(f.h, g.h)
    p2, s2 = np.array([0.5, 0.5]), np.array([1, 2], np.uint64)
    state = RecoveryStateC(3.0, 1.0)
    ok = RecoveryParamsC(0.001, 0.1, 0.5, 0, 1)
    nan, inf = float("nan"), float("inf")

    def refused(rc, word):
        assert rc == -1 and word in L.tdr_last_error().decode(), L.tdr_last_error()
        assert out.value == 777 and pout.value == 777.0 and (o2 == 777).all() and (state.w_slow, state.w_fast) == (3.0, 1.0)
        assert _snapshot(f) == before and g.states().tobytes() == before_g

    refused(L.tdr_filter_inject(None, C.c_double(0.5), 0, 1, C.byref(out)), "null")
    for p in (-0.001, 1.001, nan, inf, -inf):
        refused(L.tdr_filter_inject(f.h, C.c_double(p), 0, 1, C.byref(out)), "p =")
        refused(L.tdr_batch_inject(arr2, 2, np.array([0.5, p]).ctypes.data_as(vp), 0, s2.ctypes.data_as(vp), o2.ctypes.data_as(vp), None), "p =")
    for mode in (-1, 2):
        refused(L.tdr_filter_inject(f.h, C.c_double(0.5), mode, 1, C.byref(out)), "heading_mode")
        refused(L.tdr_batch_inject(arr2, 2, p2.ctypes.data_as(vp), mode, s2.ctypes.data_as(vp), o2.ctypes.data_as(vp), None), "heading_mode")
    pa, sa, oa = p2.ctypes.data_as(vp), s2.ctypes.data_as(vp), o2.ctypes.data_as(vp)
    refused(L.tdr_batch_inject(None, 2, pa, 0, sa, oa, None), "null")
    refused(L.tdr_batch_inject(arr2, 2, None, 0, sa, oa, None), "null")
    refused(L.tdr_batch_inject(arr2, 2, pa, 0, None, oa, None), "null")
    refused(L.tdr_batch_inject(arr2, 0, pa, 0, sa, oa, None), "at least one")
    refused(L.tdr_batch_inject((vp * 2)(f.h, None), 2, pa, 0, sa, oa, None), "null")
    refused(L.tdr_batch_inject((vp * 2)(f.h, f.h), 2, pa, 0, sa, oa, None), "twice")
    refused(L.tdr_filter_recovery_step(None, C.byref(state), C.byref(ok), C.byref(pout), C.byref(out)), "null")
    refused(L.tdr_filter_recovery_step(f.h, None, C.byref(ok), C.byref(pout), C.byref(out)), "null")
    refused(L.tdr_filter_recovery_step(f.h, C.byref(state), None, C.byref(pout), C.byref(out)), "null")
    for bad in (RecoveryParamsC(0.0, 0.1, 0.5, 0, 1), RecoveryParamsC(1.5, 0.1, 0.5, 0, 1), RecoveryParamsC(nan, 0.1, 0.5, 0, 1),
                RecoveryParamsC(0.001, 0.0, 0.5, 0, 1), RecoveryParamsC(0.001, -0.1, 0.5, 0, 1), RecoveryParamsC(0.001, 1.01, 0.5, 0, 1),
                RecoveryParamsC(0.001, 0.1, 1.5, 0, 1), RecoveryParamsC(0.001, 0.1, -0.5, 0, 1), RecoveryParamsC(0.001, 0.1, nan, 0, 1),
                RecoveryParamsC(0.001, 0.1, 0.5, 2, 1)):
        refused(L.tdr_filter_recovery_step(f.h, C.byref(state), C.byref(bad), C.byref(pout), C.byref(out)), "recovery_step")
    refused(L.tdr_filter_get_weight_stats(None, np.zeros(8, F32).ctypes.data_as(vp)), "null")
    refused(L.tdr_filter_get_weight_stats(f.h, None), "null")
    refused(L.tdr_filter_get_weight_stats(g.h, np.zeros(8, F32).ctypes.data_as(vp)), "no update")
    refused(L.tdr_filter_recovery_step(g.h, C.byref(state), C.byref(ok), C.byref(pout), C.byref(out)), "no update")
    # a filter without particles; a map without a road cell
    e, _ = _handle(scene, "polar", 64)
    refused(L.tdr_filter_inject(e.h, C.c_double(0.5), 0, 1, C.byref(out)), "no particles")
    refused(L.tdr_batch_inject((vp * 2)(f.h, e.h), 2, pa, 0, sa, oa, None), "no particles")
    noroad = batch.MapHandle(np.full((scene.cfg.ncls, 50, 50), 9.0, F32), np.zeros((50, 50), np.uint8))
    noroad.sample_pts_polar(36, 12, 2 * np.pi / 36)
    h = batch.FilterHandle(noroad, 64, FilterParams(fixed_scale=1.0), seed=1)
    h.set_states(st[:64])
    hb = h.states().tobytes()
    refused(L.tdr_filter_inject(h.h, C.c_double(0.5), 0, 1, C.byref(out)), "no road")
    refused(L.tdr_batch_inject((vp * 2)(f.h, h.h), 2, pa, 0, sa, oa, None), "no road")
    assert h.states().tobytes() == hb
    # outputs are optional; p = 0 is a valid call that injects nothing
    assert L.tdr_filter_inject(f.h, C.c_double(0.0), 0, 1, None) == 0 and _snapshot(f) == before
    assert L.tdr_filter_inject(f.h, C.c_double(0.0), 0, 1, C.byref(out)) == 0 and out.value == 0 and _snapshot(f) == before
    with pytest.raises(ValueError):
        recovery_params_c(RecoveryParams(alpha_slow=0.0))
    with pytest.raises(ValueError):
        recovery_params_c(RecoveryParams(heading_mode=3))


def test_a_sharded_filter_is_refused(scene):
    """One rank over the callback transport: the collectives are copies on the device."""
    from top_down_renderer_amd import FilterParams
    from top_down_renderer_amd._lib import RecoveryParamsC, RecoveryStateC, check
    f, _ = _handle(scene, "polar", 64)
    f.set_states(_spread_states(scene, 64, 1, False))
    L = f.L
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    AG = C.CFUNCTYPE(C.c_int, vp, vp, vp, C.c_size_t, vp)
    BC = C.CFUNCTYPE(C.c_int, vp, vp, C.c_size_t, C.c_int, vp)

    class Ops(C.Structure):
        _fields_ = [("ctx", vp), ("all_gather", AG), ("broadcast", BC)]
    ops = Ops(None, AG(lambda ctx, send, recv, nbytes, stream: hip.hipMemcpy(recv, send, nbytes, 3)),
              BC(lambda ctx, buf, nbytes, root, stream: 0))
    comm, sh = vp(), vp()
    check(L.tdr_comm_create(1, 0, C.byref(ops), C.byref(comm)))
    fp = FilterParams(fixed_scale=1.0).to_c(scene.cfg.ncls)
    check(L.tdr_filter_create_sharded(f.map.h, 64, C.byref(fp), 7, comm, C.byref(sh)))
    try:
        st = np.ascontiguousarray(_spread_states(scene, 64, 2, False))
        check(L.tdr_filter_set_states(sh, st.ctypes.data_as(vp), 64))
        out, o2 = C.c_int64(777), np.full(2, 777, np.int64)
        assert L.tdr_filter_inject(sh, C.c_double(0.5), 0, 1, C.byref(out)) == -1
        assert "sharded" in L.tdr_last_error().decode() and out.value == 777
        p2, s2 = np.array([0.5, 0.5]), np.array([1, 2], np.uint64)
        assert L.tdr_batch_inject((vp * 2)(f.h, sh), 2, p2.ctypes.data_as(vp), 0, s2.ctypes.data_as(vp), o2.ctypes.data_as(vp), None) == -1
        assert "sharded" in L.tdr_last_error().decode() and (o2 == 777).all()
        state, ok = RecoveryStateC(0.0, 0.0), RecoveryParamsC(0.001, 0.1, 0.5, 0, 1)
        assert L.tdr_filter_recovery_step(sh, C.byref(state), C.byref(ok), None, None) == -1
        assert "sharded" in L.tdr_last_error().decode()
        got = np.zeros(64, RR.STATE_DTYPE)
        check(L.tdr_filter_get_states(sh, got.ctypes.data_as(vp), 64))
        assert got.tobytes() == st.tobytes()
    finally:
        L.tdr_filter_destroy(sh)
        L.tdr_comm_destroy(comm)
    import types
    from top_down_renderer_amd import ParticleFilter
    pf = ParticleFilter.__new__(ParticleFilter)
    pf.comm = types.SimpleNamespace(active=True)
    with pytest.raises(ValueError, match="sharded"):
        pf.inject(0.5)


# ---- Python filter and C++ classes ------------------------------------------------------------------------------------------------
STEPS = 12
MOTION = (2.5, 1.5, 0.02)      # the robot's belief walks away from where the scan was taken: the weights fall
LOOP_RP = dict(alpha_slow=0.05, alpha_fast=0.8, p_max=0.3, heading_mode=0, seed=500)


def _write_inputs(d, sc, states, npart, robots, steps, recovery_every, rp, inject_p=0.0, seed=7):
    cfg = sc.cfg
    open(os.path.join(d, "meta.txt"), "w").write(
        f"{cfg.ncls} {cfg.map_size} {cfg.map_size} {cfg.nb} {cfg.nr} {len(sc.pts)} {npart} {seed} {steps} 1.0 "
        f"{cfg.map_resolution} {robots} {recovery_every} {rp['alpha_slow']!r} {rp['alpha_fast']!r} {rp['p_max']!r} "
        f"{rp['heading_mode']} {rp['seed']} {inject_p!r}\n")
    np.ascontiguousarray(np.transpose(sc.class_maps, (0, 2, 1)), F32).tofile(os.path.join(d, "maps.bin"))
    np.ascontiguousarray(sc.class_mask.T, np.uint8).tofile(os.path.join(d, "mask.bin"))
    pcl = np.zeros((len(sc.pts), 8), F32)
    pcl[:, :3], pcl[:, 4] = sc.pts[:, :3], sc.pts[:, 3]
    pcl.tofile(os.path.join(d, "pts.bin"))
    np.ascontiguousarray(states, RR.STATE_DTYPE).tofile(os.path.join(d, "states.bin"))
    np.asarray(MOTION, F32).tofile(os.path.join(d, "motion.bin"))


@pytest.mark.parametrize("mode", [0, 1])
def test_python_filter_and_cpp_classes_equal_the_restatement(K, scene, facade_exe, mode):
    import top_down_renderer_amd as pkg
    cfg, n, p, seed = scene.cfg, 4096, 0.3, 900
    sets = [_spread_states(scene, n, 20 + r, False) for r in range(3)]
    want = [_ref_inject(scene, s, p, mode, seed + r, 0) for r, s in enumerate(sets)]
    # Python ParticleFilter.inject on torch buffers, TopDownMap.roadCells
    m = pkg.TopDownMapPolar(pkg.Params(resolution=cfg.map_resolution), scene.class_maps, scene.class_mask, kernels=K)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    assert np.array_equal(_cells(m.roadCells()), RR.road_cells(scene.class_maps)) and m.roadCells() is m.roadCells()
    pf = pkg.ParticleFilter(n, m, pkg.FilterParams(fixed_scale=1.0), seed=1, kernels=K, init_particles=False)
    for r, (s, (w, cnt)) in enumerate(zip(sets, want)):
        pf.set_states(s)
        assert pf.inject(p, mode, seed + r) == cnt and pf.get_states().tobytes() == w.tobytes()
        assert pf._maybe_uninit == (mode == 0)
    with pytest.raises(ValueError):
        pf.inject(1.5)
    with pytest.raises(ValueError):
        pf.inject(0.5, heading_mode=2)
    # ParticleFilter::inject, ParticleFilterBatch::inject, ParticleFilterCartesian::inject, TopDownMap::roadCells
    d = tempfile.mkdtemp(prefix="tdr_recovery_")
    rp = dict(LOOP_RP, heading_mode=mode, seed=seed)
    _write_inputs(d, scene, np.concatenate(sets), n, 3, 0, 0, rp, inject_p=p)
    r = subprocess.run([facade_exe, "inject", d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.split()[0] in ("polar", "batch", "cart")]
    assert [(w, int(a)) for w, a in lines] == [("polar", c) for _, c in want] + [("batch", c) for _, c in want] + [("cart", want[0][1])]
    assert np.array_equal(np.fromfile(os.path.join(d, "out_road.bin"), np.uint32), RR.road_cells(scene.class_maps))
    for who, rs in (("polar", range(3)), ("batch", range(3)), ("cart", [0])):
        for i in rs:
            assert np.fromfile(os.path.join(d, f"out_inject_{who}_{i}.bin"), RR.STATE_DTYPE).tobytes() == want[i][0].tobytes(), (who, i)


# ---- the node loop ---------------------------------------------------------------------------------------------------------------
def _loop_cfg(scene, every, n, seed=7, rseed=None, **over):
    import top_down_renderer_amd as pkg
    cfg = scene.cfg
    rp = dict(LOOP_RP, **over)
    if rseed is not None:
        rp["seed"] = rseed
    return pkg.CoreConfig(particle_count=n, theta_bins=cfg.nb, range_bins=cfg.nr, seed=seed, recovery_every=every,
                          recovery=pkg.RecoveryParams(**rp))


def _read_loop(d, r, steps, n):
    rec = np.fromfile(os.path.join(d, f"out_rec_{r}.bin"), np.float64).reshape(steps, 4)
    st = np.fromfile(os.path.join(d, f"out_states_{r}.bin"), RR.STATE_DTYPE).reshape(steps, n)
    return rec, st


def _python_core_trace(K, scene, cfgc, states, steps):
    import top_down_renderer_amd as pkg
    cfg = scene.cfg
    m = pkg.TopDownMapPolar(pkg.Params(resolution=cfg.map_resolution), scene.class_maps, scene.class_mask, kernels=K)
    core = pkg.TopDownRenderCore(cfgc, kernels=K)
    core.initialize(m, pkg.FilterParams(fixed_scale=1.0), scene.lut, init_particles=False)
    core.filter_.set_states(states)
    rec, sts = [], []
    for s in range(steps):
        assert core.takeStep(scene.pts, MOTION[:2], MOTION[2]) is not None
        rec.append((core.last_recovery_[0], core.last_recovery_[1], core.recovery_state_.w_slow, core.recovery_state_.w_fast))
        sts.append(core.filter_.get_states())
    return np.array(rec, np.float64), np.stack(sts)


def test_recovery_off_is_the_loop_without_the_field(K, scene):
    import top_down_renderer_amd as pkg
    cfg, n = scene.cfg, 2048
    st = _spread_states(scene, n, 61, False)
    plain = pkg.CoreConfig(particle_count=n, theta_bins=cfg.nb, range_bins=cfg.nr, seed=7)
    rec_a, st_a = _python_core_trace(K, scene, plain, st, 6)
    rec_b, st_b = _python_core_trace(K, scene, _loop_cfg(scene, 0, n, alpha_fast=1.0, p_max=1.0, heading_mode=1), st, 6)
    assert st_a.tobytes() == st_b.tobytes() and not rec_a.any() and not rec_b.any()
    rec_c, st_c = _python_core_trace(K, scene, _loop_cfg(scene, 1, n), st, 6)
    assert rec_c[:, 1].sum() > 0 and st_c.tobytes() != st_a.tobytes()       # ... and with it on, the loop does change


def test_cpp_core_python_core_and_handle_loop_agree(K, scene, facade_exe):
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.particle_filter import FilterParams
    cfg, n = scene.cfg, 4096
    st = _spread_states(scene, n, 60, False)
    d = tempfile.mkdtemp(prefix="tdr_recovery_")
    _write_inputs(d, scene, st, n, 1, STEPS, 1, LOOP_RP)
    r = subprocess.run([facade_exe, "loop", d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rec_c, st_c = _read_loop(d, 0, STEPS, n)
    rec_p, st_p = _python_core_trace(K, scene, _loop_cfg(scene, 1, n), st, STEPS)
    assert rec_c[:, 1].sum() > 0 and (rec_c[:, 0] > 0).sum() >= 2, rec_c     # the tracker did ask for injections
    assert np.array_equal(rec_c, rec_p), (rec_c, rec_p)
    assert st_c.tobytes() == st_p.tobytes()
    # every step's injection is the restatement's: the tracker over the weight statistics, then the slots
    m = batch.MapHandle(scene.class_maps, scene.class_mask, cfg.map_resolution)
    m.sample_pts_polar(cfg.nb, cfg.nr, float(cfg.ang_res))
    f = batch.FilterHandle(m, n, FilterParams(fixed_scale=1.0), seed=7)
    f.set_states(st)
    loop = batch.LoopBatch([f], [batch.Renderer(scene.lut)], _loop_cfg(scene, 1, n), float(cfg.ang_res), cfg.ncls, cfg.nb, cfg.nr)
    pcl = np.zeros((len(scene.pts), 8), F32)
    pcl[:, :3], pcl[:, 4] = scene.pts[:, :3], scene.pts[:, 3]
    t = RR.Tracker(LOOP_RP["alpha_slow"], LOOP_RP["alpha_fast"], LOOP_RP["p_max"])
    for s in range(STEPS):
        loop.take_step([(pcl, 8, 4)], [MOTION])
        p = t.track(float(f.weight_stats()[2]))
        if p > 0:
            t.reset()
        assert (p, t.w_slow, t.w_fast) == (rec_c[s, 0], rec_c[s, 2], rec_c[s, 3]), s
        assert f.states().tobytes() == st_c[s].tobytes(), s
        assert loop.cores[0].last_recovery_ == (rec_c[s, 0], int(rec_c[s, 1]))


def test_batch_cores_equal_single_cores(scene, facade_exe):
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.particle_filter import FilterParams
    cfg, n, robots = scene.cfg, 4096, 3
    sets = np.concatenate([_spread_states(scene, n, 60 + r, False) for r in range(robots)])
    out = {}
    for mode in ("loop", "batch"):
        d = tempfile.mkdtemp(prefix="tdr_recovery_")
        _write_inputs(d, scene, sets, n, robots, STEPS, 2, LOOP_RP)
        r = subprocess.run([facade_exe, mode, d], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[mode] = [_read_loop(d, i, STEPS, n) for i in range(robots)]
    for i in range(robots):
        assert np.array_equal(out["loop"][i][0], out["batch"][i][0]) and out["loop"][i][1].tobytes() == out["batch"][i][1].tobytes(), i
        rec = out["loop"][i][0]                                   # recovery_every = 2: a step that is not due leaves the record
        assert not rec[0].any() and all(np.array_equal(rec[s], rec[s - 1]) for s in range(2, STEPS, 2))
    assert sum(o[0][:, 1].sum() for o in out["loop"]) > 0
    # the Python batch loop: the same robots, seeds as the C++ program gives them
    ang = float(cfg.ang_res)
    m = batch.MapHandle(scene.class_maps, scene.class_mask, cfg.map_resolution)
    m.sample_pts_polar(cfg.nb, cfg.nr, ang)
    fs = []
    for r in range(robots):
        f = batch.FilterHandle(m, n, FilterParams(fixed_scale=1.0), seed=7 + r)
        f.set_states(sets[r * n:(r + 1) * n])
        fs.append(f)
    cfgs = [_loop_cfg(scene, 2, n, seed=7 + r, rseed=LOOP_RP["seed"] + r) for r in range(robots)]
    loop = batch.LoopBatch(fs, [batch.Renderer(scene.lut) for _ in range(robots)], cfgs, ang, cfg.ncls, cfg.nb, cfg.nr)
    pcl = np.zeros((len(scene.pts), 8), F32)
    pcl[:, :3], pcl[:, 4] = scene.pts[:, :3], scene.pts[:, 3]
    for s in range(STEPS):
        loop.take_step([(pcl, 8, 4)] * robots, [MOTION] * robots)
        for r in range(robots):
            assert fs[r].states().tobytes() == out["batch"][r][1][s].tobytes(), (s, r)
            c = loop.cores[r]
            assert (c.last_recovery_[0], c.last_recovery_[1], c.recovery_state_.w_slow, c.recovery_state_.w_fast) == \
                tuple(out["batch"][r][0][s]), (s, r)


# ---- the closed loop: a kidnapped robot --------------------------------------------------------------------------------------------
RADIUS = 40.0      # the max-likelihood bound of test_gpu_filter_converges_on_the_true_pose (tests/test_localizes.py)
# The averages' memories fit the run: the slow one remembers about 20 updates (the 10 before the move must count), the fast
# one about 2.  AMCL's 0.001 / 0.1 are for runs of thousands of updates: there the slow average is still the first update's
# mean when the robot is moved, and no injection is ever asked for (measured: p = 0 on every step).
KIDNAP_RP = dict(alpha_slow=0.05, alpha_fast=0.5, p_max=0.5, heading_mode=0, seed=2026)
STEPS_NEEDED = 9        # measured on the MI355X: the max-likelihood particle is within RADIUS from the 9th step after the move on
STEPS_ALLOWED = 18      # twice that


def kidnap_run(K, recovery_every, steps_after, rp=None, stop_at_radius=True):
    """10 steps at the true pose of synth's c1 scene, then the scans come from a road pose at least 400 px away.  Returns
    (the new pose, per further step: distance of the max-likelihood particle to it, particles within RADIUS of it).
    The cloud starts as the scene's Gaussian about the true pose WITHOUT the scene's 10 % uniform share: a kidnapped robot
    is one whose cloud has condensed, and a uniform share is a recovery of its own (measured on the MI355X: with it, 12 of
    the 4000 particles still stand within RADIUS of the new pose 40 steps after the move, recovery off)."""
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import synth
    sc = synth.make_scene("c1", n_particles=4000)
    cfg = sc.cfg
    rng = np.random.default_rng(77)
    while True:
        pose2 = synth.pick_true_pose(sc.lab, rng, 168)
        if np.hypot(pose2[0] - sc.pose[0], pose2[1] - sc.pose[1]) >= 400:
            break
    pts2 = synth.make_scan(cfg, sc.lab, pose2, rng)
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=K)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    r = pkg.ScanRendererPolar(sc.lut, kernels=K)
    r.set_output_shape(cfg.ncls, cfg.nb, cfg.nr)
    f = pkg.ParticleFilter(len(sc.states), m, pkg.FilterParams(fixed_scale=1.0), seed=5, kernels=K, init_particles=False)
    f.set_states(synth.make_particles(cfg, sc.lab, sc.pose, np.random.default_rng(78), n=len(sc.states), uniform_frac=0.0))
    from top_down_renderer_amd._lib import RecoveryStateC
    state, params = RecoveryStateC(0.0, 0.0), pkg.RecoveryParams(**(rp or KIDNAP_RP))

    def step(s):
        f.propagate((0.2, 0.0), 0.0)
        f.update(r.last_scan(), None, cfg.res)
        if recovery_every and (s + 1) % recovery_every == 0:
            f.recoveryStep(state, params)

    r.renderSemanticTopDown(sc.pts, cfg.res, cfg.ang_res)
    for s in range(10):
        step(s)
    ml = f.maxLikelihood()
    assert np.hypot(ml[0] - sc.pose[0], ml[1] - sc.pose[1]) < 100      # the cloud sits on the first pose
    r.renderSemanticTopDown(pts2, cfg.res, cfg.ang_res)
    trace = []
    for s in range(steps_after):
        step(10 + s)
        ml = f.maxLikelihood()
        st = f.get_states()
        x = st["dx_m"] * st["scale"] + st["init_x_px"]
        y = st["dy_m"] * st["scale"] + st["init_y_px"]
        trace.append((float(np.hypot(ml[0] - pose2[0], ml[1] - pose2[1])), int((np.hypot(x - pose2[0], y - pose2[1]) < RADIUS).sum())))
    return pose2, trace


def test_without_recovery_the_cloud_stays_where_it_was(K):
    _, trace = kidnap_run(K, 0, 40)
    print("kidnap trace without recovery:", trace)
    assert trace[-1][1] == 0, trace


def test_recovery_finds_the_robot_again(K):
    """With recovery_every = 1 the max-likelihood particle is within RADIUS of the new pose after STEPS_ALLOWED steps.
    Measured on the MI355X: the mean raw weight falls from 5.31 to 4.77 with the move, the tracker asks for p = 0.0021 on
    the 4th step after it (9 slots), one of the 9 stands 4 px from the new pose, the max-likelihood particle is within
    RADIUS first on the 5th step and on every step from the 9th (STEPS_NEEDED), and 3662 of the 4000 particles are within
    RADIUS after 80 steps.  The mean weight falls by a tenth only and the averages are reset after an injection, so one small
    injection is all this scene gets: with other memories of the averages (0.1 / 0.9, 0.2 / 1.0: 77 and 174 slots on the
    first step after the move) the run had NOT recovered after 80 steps, the cloud sat on another stretch of road.
    What this asserts is therefore that ONE draw into the basin is enough for the filter to follow it, under this seed; it
    does not show that recovery is robust.  A change to the words a slot draws, to the road list's order or to the scene
    moves that draw, and the run has to be measured again."""
    _, trace = kidnap_run(K, 1, STEPS_ALLOWED)
    first = next((i + 1 for i, (d, _) in enumerate(trace) if d < RADIUS), None)
    print("kidnap trace:", first, trace)
    assert trace[-1][0] < RADIUS, (first, trace[-5:])
    assert trace[-1][1] > 0
