"""GPU: the pose-grid search (csrc/tdr_grid.hip, csrc/tdr_host_grid.cpp; include/tdr.h, "pose-grid search") against its NumPy
restatement (tests/grid_ref.py), with ==: the four kernels through their launchers, the handle against the device's own
scorer (a second filter of the same kind, map, parameters and particle count scores the lattice states), chunking, what
the call leaves alone, the Python filter against the handle, the CPU oracle's top peak, tdr_filter_inject_cells against
the recovery restatement, what is refused, and what the feature is for: the kidnapped robot found with one call.
Sizes are chosen for where the kernels can go wrong (a point, a row, a column, a tile less one, a tile, several tiles with a
ragged end, a grid smaller than the tiles, a wave less one, a wave, a wave plus one), not for the workload."""
import ctypes as C

import numpy as np
import pytest

import grid_ref as GR
import recovery_ref as RR
from test_grid_ref import BASIN_PX, c1_oracle_search, c1_scene, c1_spec, peak_distance
from test_recovery import RADIUS, _dev_map, _handle, _road_maps, _snapshot, _spread_states, _to_planes
from test_sensor_reset import _weight_rows

pytestmark = pytest.mark.gpu
F32 = np.float32
vp = C.c_void_p
NAN = float("nan")
SENT = -777.0


@pytest.fixture(scope="module")
def K():
    import torch
    from top_down_renderer_amd.kernels import HipKernels
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels()


def _c(sp):
    from top_down_renderer_amd import _lib
    return _lib.grid_spec(*sp)


def _planes_of(states):
    return _to_planes(np.ascontiguousarray(states).reshape(-1), states.size, 0.0)


@pytest.fixture(scope="module")
def odd_map(K):
    maps = _road_maps(67, 131, 3, 1)          # an odd number of columns
    return maps, {res: _dev_map(K, maps, res) for res in (1.0, 2.0)}


# ---- the list kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 7), (7, 1), (17, 15), (16, 16), (257, 3)])
def test_list_equals_the_restatement(K, odd_map, nx, ny):
    maps, dms = odd_map
    seen = set()
    for c0, r0, step in ((0, 0, 1), (3, 2, 3), (-5, -3, 3), (-5, -3, 1), (100, 50, 3), (200, 10, 1), (-400, -40, 1), (130, 66, 1)):
        for road_only in (0, 1):
            sp = GR.Spec(c0, r0, step, nx, ny, road_only=road_only)
            want = GR.lattice_list(maps, sp)
            for mb in (0, 1, 3):           # the launcher's grid, one workgroup for every tile, three workgroups
                got = K.grid_list(dms[1.0], _c(sp), max_blocks=mb).cpu().numpy()
                assert got.dtype == np.int32 and np.array_equal(got, want), (sp, mb)
            seen.add((len(want) == 0, len(want) == nx * ny))
    assert (True, False) in seen and ((False, True) in seen or nx > 43)      # wholly outside, wholly inside


# ---- the candidates kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 5, 64])
def test_candidates_equal_the_restatement(K, odd_map, H):
    maps, dms = odd_map
    for mode, res, scale in ((1, 1.0, 1.0), (1, 2.0, 1.375), (0, 2.0, 0.75)):
        if mode == 0 and H != 1:
            continue
        sp = GR.Spec(-5, -3, 3, 17, 15, road_only=0, heading_mode=mode, n_headings=H, theta0=0.1, dtheta=0.3, scale=scale)
        lst_h = GR.lattice_list(maps, sp)
        lst = K.grid_list(dms[res], _c(sp))
        assert np.array_equal(lst.cpu().numpy(), lst_h) and len(lst_h) > 130          # more entries than two waves
        for first, m in ((0, len(lst_h)), (1, len(lst_h) - 2), (67, 3), (len(lst_h) - 1, 1)):
            cand_cap = m * H + 5
            cst = K.to_device(np.full((7, cand_cap), SENT, F32))
            K.grid_candidates(dms[res], _c(sp), lst, first, m, cst)
            want = GR.candidates(sp, lst_h[first:first + m], res)
            got = cst.cpu().numpy()
            assert got[:, :m * H].tobytes() == _planes_of(want).tobytes(), (H, mode, first, m)
            assert (got[:, m * H:] == SENT).all()


# ---- the reduce kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 63, 64, 65, 4096])
def test_reduce_equals_the_restatement(K, H):
    rng = np.random.default_rng(H)
    sp = GR.Spec(0, 0, 1, 9, 5, road_only=0, heading_mode=1, n_headings=H)
    G, m = 45, 11                                          # 11 waves: three workgroups, the last with three waves
    lst_h = np.sort(rng.choice(G, m, replace=False)).astype(np.int32)
    w = _weight_rows(m, H, rng)
    after = np.zeros((m, H), RR.STATE_DTYPE)
    after["theta"] = rng.uniform(-3, 3, (m, H)).astype(F32)
    after["have_init"] = rng.random((m, H)) < 0.7
    after["init_x_px"] = rng.normal(0, 50, (m, H)).astype(F32)
    W, T, vol = GR.reduce(sp, lst_h, w, after)
    assert np.isnan(W[lst_h[1]]) and W[lst_h[0]] == 3.0 and W[lst_h[2]] == 0.0
    lst = K.to_device(lst_h)
    for with_vol in (True, False):
        gw, gt, gv = K.grid_planes(_c(sp), vol=with_vol)
        for first, mm in ((0, 4), (4, m - 4)):            # two windows that split the list
            cst = K.to_device(_planes_of(after[first:first + mm]))
            cw = K.to_device(np.concatenate([w[first:first + mm].ravel(), np.full(3, 1e9, F32)]))
            K.grid_reduce(_c(sp), lst, first, mm, cst, cw, gw, gt, gv)
        assert gw.cpu().numpy().tobytes() == W.tobytes() and gt.cpu().numpy().tobytes() == T.tobytes(), H
        if with_vol:
            assert gv.cpu().numpy().tobytes() == vol.tobytes(), H


# ---- the peaks kernel ------------------------------------------------------------------------------------------------------------------
def _crafted_plane(nx, ny, rng):
    """Eighths between 1/8 and 6, so equal neighbours are common; NaNs, zeros and negative values; plateaus across the
    16-point tile edges in both directions; the largest value twice, far apart."""
    W = (rng.integers(1, 49, (ny, nx)) / 8.0).astype(F32)
    W[rng.random((ny, nx)) < 0.1] = NAN
    W[rng.random((ny, nx)) < 0.05] = 0.0
    W[rng.random((ny, nx)) < 0.05] = -2.0
    if nx > 17 and ny > 17:
        W[14:18, 14:18] = 6.5                              # a plateau over the corner of four tiles
        W[3, 15:17] = 7.0                                  # across a vertical tile edge
        W[15:17, 30] = 7.0                                 # across a horizontal one
        W[ny - 1, nx - 1] = 7.0
    elif nx * ny > 20:
        W.ravel()[15:17] = 7.0
        W.ravel()[-1] = 7.0
    return W


@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 40), (40, 1), (33, 31)])
def test_peaks_equal_the_restatement(K, odd_map, nx, ny):
    maps, dms = odd_map
    rng = np.random.default_rng(nx * 100 + ny)
    sp = GR.Spec(2, 1, 2, nx, ny, road_only=0)
    planes = [_crafted_plane(nx, ny, rng), np.full((ny, nx), NAN, F32), np.full((ny, nx), 2.0, F32)]
    if nx * ny == 1:
        planes.append(np.full((1, 1), 0.0, F32))
    for W in planes:
        T = rng.uniform(-3, 3, nx * ny).astype(F32)
        gw, gt = K.to_device(W.ravel()), K.to_device(T)
        for R in (0, 1, 2, 16):
            want, n_want = GR.peaks(sp, 131, W, T, R, 4096)
            for Kp in (0, 1, 7, 4096):
                got, n_got = K.grid_peaks(dms[1.0], _c(sp), gw, gt, R, Kp)
                assert n_got == n_want, (R, Kp)
                assert got.tobytes() == want[:Kp].tobytes(), (R, Kp, got[:3], want[:3])
        assert gw.cpu().numpy().tobytes() == W.tobytes()
    flat, n_flat = GR.peaks(sp, 131, planes[2], np.zeros(nx * ny, F32), 1, 4096)
    assert n_flat == 1 and flat["g"].tolist() == [0]                  # a plateau has exactly one peak: its smallest g


def test_launchers_refuse_bad_arguments(K, odd_map):
    import torch
    from top_down_renderer_amd import _lib
    maps, dms = odd_map
    dm, L = dms[1.0], K.lib
    ok = GR.Spec(0, 0, 2, 8, 4, road_only=1, heading_mode=1, n_headings=3, theta0=0.0, dtheta=0.1, scale=1.0)
    G = 32
    lst_b = np.arange(G, dtype=np.int32)
    cst_b, cw_b = np.full((7, 16), SENT, F32), np.full(16, 2.0, F32)
    lst, cst, cw = K.to_device(lst_b), K.to_device(cst_b), K.to_device(cw_b)
    gw, gt, gv = K.grid_planes(_c(ok), vol=True)
    cnt, ws = K.to_device(np.array([55], np.int64)), K.empty((1 << 16,), torch.uint8)
    peaks = K.to_device(np.full((8, 4), -5, np.int32))
    one = _dev_map(K, np.zeros((1, 20, 30), F32))
    p = lambda t: vp(t.data_ptr()) if t is not None else None
    ref = lambda s: C.byref(_c(s)) if s is not None else None
    d = lambda m: C.byref(m.desc) if m is not None else None

    def do_list(m=dm, s=ok, out=lst, c=cnt, w=ws):
        return L.tdr_k_grid_list(d(m), ref(s), p(out), p(c), p(w), 0, None)

    def do_cand(m=dm, s=ok, l=lst, n_list=G, first=0, m_=4, o=cst, ccap=16):
        return L.tdr_k_grid_candidates(d(m), ref(s), p(l), n_list, first, m_, p(o), ccap, None)

    def do_red(s=ok, l=lst, n_list=G, first=0, m_=4, o=cst, ccap=16, w=cw, W=gw, T=gt):
        return L.tdr_k_grid_reduce(ref(s), p(l), n_list, first, m_, p(o), ccap, p(w), p(W), p(T), p(gv), None)

    def do_peaks(m=dm, s=ok, W=gw, T=gt, R=2, Kp=8, out=peaks, c=cnt, w=ws):
        return L.tdr_k_grid_peaks(d(m), ref(s), p(W), p(T), R, Kp, p(out), p(c), p(w), None)

    bad_specs = [ok._replace(step=0), ok._replace(nx=0), ok._replace(ny=0), ok._replace(nx=4097, ny=4097), ok._replace(road_only=2),
                 ok._replace(road_only=-1), ok._replace(heading_mode=2), ok._replace(heading_mode=-1), ok._replace(n_headings=0),
                 ok._replace(n_headings=4097), ok._replace(heading_mode=0), ok._replace(theta0=NAN), ok._replace(dtheta=float("inf")),
                 ok._replace(scale=0.0), ok._replace(scale=-1.0), ok._replace(scale=NAN), ok._replace(scale=float("inf"))]
    refused = [f(s=s) for s in bad_specs + [None] for f in (do_list, do_cand, do_red, do_peaks)]
    refused += [do_list(m=None), do_list(out=None), do_list(c=None), do_list(w=None), do_list(m=one),
                do_cand(m=None), do_cand(l=None), do_cand(o=None), do_cand(n_list=-1), do_cand(n_list=G + 1), do_cand(first=-1),
                do_cand(m_=-1), do_cand(first=30, m_=3), do_cand(m_=6, ccap=17),
                do_red(l=None), do_red(o=None), do_red(w=None), do_red(W=None), do_red(T=None), do_red(n_list=G + 1), do_red(first=-1),
                do_red(m_=-1), do_red(first=30, m_=3), do_red(m_=6, ccap=17),
                do_peaks(m=None), do_peaks(W=None), do_peaks(T=None), do_peaks(out=None), do_peaks(c=None), do_peaks(w=None),
                do_peaks(R=-1), do_peaks(R=17), do_peaks(Kp=-1), do_peaks(Kp=4097)]
    assert refused == [-1] * len(refused), refused
    K.synchronize()
    nan_bits = np.full(G, 0x7FC00000, np.uint32).tobytes()
    assert lst.cpu().numpy().tobytes() == lst_b.tobytes() and cst.cpu().numpy().tobytes() == cst_b.tobytes()
    assert gw.cpu().numpy().tobytes() == nan_bits and gt.cpu().numpy().tobytes() == nan_bits and int(cnt.item()) == 55
    assert (peaks.cpu().numpy() == -5).all()
    # empty windows are valid calls; a map without class 1 serves a lattice that does not ask for road
    assert do_cand(m_=0) == 0 and do_red(m_=0) == 0 and do_list(m=one, s=ok._replace(road_only=0)) == 0
    assert do_peaks(Kp=0, out=None) == 0 and int(cnt.item()) == 0
    assert L.tdr_grid_list_workspace_bytes(257, 3) >= 8 * 4 and L.tdr_grid_list_workspace_bytes(0, 3) == 0
    assert L.tdr_grid_peaks_workspace_bytes(33, 31) >= 16 * 33 * 31 and L.tdr_grid_peaks_workspace_bytes(4097, 4097) == 0


# ---- the handle against the device's own scorer ------------------------------------------------------------------------------------------
N_F = 512


@pytest.fixture(scope="module")
def scene():
    return c1_scene()[0]


def _prepared(scene, kind, seed=5):
    """A filter of N_F particles after one update, and its renderer."""
    f, r = _handle(scene, kind, N_F, seed=seed)
    f.set_states(_spread_states(scene, N_F, 7, kind == "polar"))
    f.propagate(0.3, 0.1, 0.005)
    f.update(r, scene.cfg.res)
    return f, r


def _device_scorer(scene, kind, r):
    """score(candidates) through a SECOND filter of the same kind, map, parameters and particle count: set_states +
    compute_weights, N_F candidates a round (the last round padded with its first candidate)."""
    twin, _ = _handle(scene, kind, N_F, seed=99)

    def score(cand):
        ws, after = [], []
        for lo in range(0, len(cand), N_F):
            part = cand[lo:lo + N_F]
            twin.set_states(np.concatenate([part, np.repeat(part[:1], N_F - len(part))]))
            twin.compute_weights(r, scene.cfg.res)
            ws.append(twin.raw_weights(N_F)[:len(part)])
            after.append(twin.states()[:len(part)])
        return np.concatenate(ws), np.concatenate(after)
    return score


def _lattice(scene, mode, H, nx=24, ny=20, scale=1.0):
    """nx x ny points at step 4 about the scene's true pose."""
    c0, r0 = int(scene.pose[0]) - 2 * nx, int(scene.pose[1]) - 2 * ny
    return GR.Spec(c0, r0, 4, nx, ny, road_only=1, heading_mode=mode, n_headings=H, theta0=float(scene.pose[2]) - 0.4, dtheta=0.2,
                   scale=scale)


def _same(res, want):
    W, T, vol, pk, n_peaks, lst = want
    assert res.listed == len(lst) and res.n_peaks == n_peaks
    assert res.w.tobytes() == W.tobytes() and res.theta.tobytes() == T.tobytes()
    assert res.vol.tobytes() == vol.tobytes()
    assert res.peaks.tobytes() == pk[:len(res.peaks)].tobytes() and len(res.peaks) == min(len(pk), 8)


@pytest.mark.parametrize("mode,H", [(0, 1), (1, 1), (1, 5)])
@pytest.mark.parametrize("kind", ["fixed", "polar", "cart"])
def test_handle_equals_the_restatement_over_the_devices_scorer(scene, kind, mode, H):
    cfg = scene.cfg
    f, r = _prepared(scene, kind)
    score = _device_scorer(scene, kind, r)
    L = f.L
    chunk0 = L.tdr_config_tuning(b"inject_cand_chunk", -1)
    assert chunk0 == 65536
    before = _snapshot(f)
    sp = _lattice(scene, mode, H, scale=1.0 if kind != "polar" else 1.25)
    want = GR.grid_search(scene.class_maps, cfg.map_resolution, sp, score, 2, 4096)
    listed = len(want[5])
    assert listed >= 50 and want[4] >= 1 and np.isfinite(want[0][want[5]]).any()
    small = _lattice(scene, mode, H, nx=6, ny=5, scale=sp.scale)._replace(road_only=0)
    want_small = GR.grid_search(scene.class_maps, cfg.map_resolution, small, score, 2, 4096)
    try:
        _same(f.grid_search(r, cfg.res, _c(sp), 2, 8, vol=True), want)
        if mode == 1 and H > 1:
            picks = GR.pick(np.asarray(want[2])[:, want[5]].T)
            assert len(set(picks.tolist())) > 1                     # the reductions do choose
        chunk = -(-listed // 3) * H                                 # the list in three chunks
        assert L.tdr_config_tuning(b"inject_cand_chunk", chunk) == chunk
        _same(f.grid_search(r, cfg.res, _c(sp), 2, 8, vol=True), want)
        chunk = max(H - 1, 1)                                       # a chunk smaller than H: a point each
        assert L.tdr_config_tuning(b"inject_cand_chunk", chunk) == chunk
        _same(f.grid_search(r, cfg.res, _c(small), 2, 8, vol=True), want_small)
        L.tdr_config_tuning(b"inject_cand_chunk", chunk0)
        _same(f.grid_search(r, cfg.res, _c(small), 2, 8, vol=True), want_small)
    finally:
        L.tdr_config_tuning(b"inject_cand_chunk", chunk0)
    assert _snapshot(f) == before, (kind, mode, H)


@pytest.mark.parametrize("kind", ["fixed", "cart"])
def test_the_filter_is_untouched(scene, kind):
    """States, weights, statistics and the step count stay; the next propagate + update equals a twin that made no search."""
    res = scene.cfg.res
    (a, r), (b, _) = _prepared(scene, kind), _prepared(scene, kind)
    assert _snapshot(a) == _snapshot(b)
    before = _snapshot(a)
    got = a.grid_search(r, res, _c(_lattice(scene, 0, 1)), 2, 8)
    assert got.listed > 0 and _snapshot(a) == before
    # no outputs asked for: a valid call
    assert a.L.tdr_filter_grid_search(a.h, None, r.h, C.c_float(res), C.byref(_c(_lattice(scene, 1, 5))), None, None, None, 2, 8, None,
                                      None, None) == 0
    assert _snapshot(a) == before
    for f in (a, b):
        f.propagate(0.2, 0.0, 0.01)
        f.update(r, res)
    assert _snapshot(a) == _snapshot(b)


def test_the_scan_as_images_and_the_kept_scan(scene):
    res = scene.cfg.res
    (a, r), (b, _), (c, _) = (_prepared(scene, "fixed") for _ in range(3))
    sp = _c(_lattice(scene, 0, 1))
    imgs = r.get_render()[0]
    want = a.grid_search(r, res, sp, 2, 8)
    got = b.grid_search(imgs, res, sp, 2, 8)
    assert got.w.tobytes() == want.w.tobytes() and got.peaks.tobytes() == want.peaks.tobytes()
    with pytest.raises(Exception, match="no scan"):
        c.grid_search(None, res, sp, 2, 8)                       # updated from a renderer: the filter kept no scan of its own
    got = b.grid_search(None, res, sp, 2, 8)                     # b kept the images' packed scan
    assert got.w.tobytes() == want.w.tobytes() and got.peaks.tobytes() == want.peaks.tobytes()


# ---- the kidnapped robot: the Python filter, the handle and the CPU oracle -----------------------------------------------------------------
def _python_filter(K, sc, states):
    import top_down_renderer_amd as pkg
    cfg = sc.cfg
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=K)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    r = pkg.ScanRendererPolar(sc.lut, kernels=K)
    r.set_output_shape(cfg.ncls, cfg.nb, cfg.nr)
    f = pkg.ParticleFilter(len(states), m, pkg.FilterParams(fixed_scale=1.0), seed=5, kernels=K, init_particles=False)
    f.set_states(states)
    return f, r


@pytest.fixture(scope="module")
def c1_searches(K):
    """Both c1 scans searched at step 8 (road only, no heading, R = 2, K = 8) by the handle and by the Python filter."""
    from top_down_renderer_amd import batch, synth
    from top_down_renderer_amd.particle_filter import FilterParams
    sc, pose2, pts2 = c1_scene()
    cfg = sc.cfg
    st = synth.make_particles(cfg, sc.lab, sc.pose, np.random.default_rng(78), n=4000, uniform_frac=0.0)
    m = batch.MapHandle(sc.class_maps, sc.class_mask, cfg.map_resolution)
    m.sample_pts_polar(cfg.nb, cfg.nr, float(cfg.ang_res))
    h = batch.FilterHandle(m, 4000, FilterParams(fixed_scale=1.0), seed=5)
    h.set_states(st)
    h0 = h.states().tobytes()
    f, pr = _python_filter(K, sc, st)
    sp = _c(c1_spec())
    out = {}
    for which, pts in (("first", sc.pts), ("kidnapped", pts2)):
        r = batch.Renderer(sc.lut)
        r.render_polar(pts, 4, 3, cfg.res, float(cfg.ang_res), cfg.ncls, cfg.nb, cfg.nr)
        pr.renderSemanticTopDown(pts, cfg.res, cfg.ang_res)
        out[which] = (h.grid_search(r, cfg.res, sp, 2, 8, vol=True), f.gridSearch(pr.last_scan(), cfg.res, sp, 2, 8, vol=True))
    assert h.states().tobytes() == h0
    return out


@pytest.mark.parametrize("which", ["first", "kidnapped"])
def test_python_filter_equals_the_handle(c1_searches, which):
    a, b = c1_searches[which]
    assert a.listed == b.listed == 3324 and a.n_peaks == b.n_peaks
    assert a.w.tobytes() == b.w.tobytes() and a.theta.tobytes() == b.theta.tobytes() and a.vol.tobytes() == b.vol.tobytes()
    assert a.peaks.tobytes() == b.peaks.tobytes() and len(a.peaks) == 8


@pytest.mark.parametrize("which", ["first", "kidnapped"])
def test_the_devices_top_peak_is_the_oracles(c1_searches, which):
    """tests/test_grid_ref.py asserts that the oracle's top peak leads the next by more than 1e-3 of its weight (measured:
    1.6e-2 and 4.7e-2), far above the 1e-5 weight tolerance of the parity tests: the device's top peak is the same point."""
    pose, W, T, pk, n_peaks, lst = c1_oracle_search(which)
    got = c1_searches[which][0]
    d = peak_distance(got.peaks[0], pose)
    print(f"{which}: device top {got.peaks['w'][0]:.4f} at g = {got.peaks['g'][0]}, {d:.1f} px; oracle {pk['w'][0]:.4f} at g = {pk['g'][0]}; "
          f"peaks {got.n_peaks} / {n_peaks}")
    assert got.listed == len(lst)
    assert got.peaks["g"][0] == pk["g"][0] and got.peaks["cell"][0] == pk["cell"][0]
    assert abs(float(got.peaks["w"][0]) - float(pk["w"][0])) <= 1e-5 * float(pk["w"][0])
    assert d < BASIN_PX


# ---- tdr_filter_inject_cells ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rec_scene():
    from top_down_renderer_amd import synth
    return synth.make_scene(synth.Config("recovery", 4000, 4, 36, 12, 300, 4096, seed=41, res=2.0))


@pytest.mark.parametrize("n", [1, 63, 4097])
def test_inject_cells_equals_the_restatement(rec_scene, n):
    cfg = rec_scene.cfg
    road = RR.road_cells(rec_scene.class_maps)
    rng = np.random.default_rng(n)
    cells = rng.choice(cfg.map_size * cfg.map_size, 9).astype(np.uint32)        # any cells, on road or not
    cells = np.concatenate([cells, cells[:4], cells[:1]])                       # duplicates weight the draw
    for mode in (0, 1):
        f, _ = _handle(rec_scene, "fixed", n)
        g, _ = _handle(rec_scene, "fixed", n)
        cur = _spread_states(rec_scene, n, 3, False)
        f.set_states(cur)
        g.set_states(cur)
        for p, seed in ((0.5, 11), (1.0, (1 << 40) + 3), (0.0, 5)):
            cur = f.states()
            want, cnt = RR.inject(cur, n, 0, cells, cfg.map_size, cfg.map_resolution, seed, f.step_count(), RR.threshold(p), mode)
            assert f.inject_cells(cells, p, mode, seed) == cnt and f.states().tobytes() == want.tobytes(), (n, mode, p)
            if p == 1.0:
                assert cnt == n
        # the map's own road list: the bytes of tdr_filter_inject
        f.set_states(cur)
        g.set_states(cur)
        assert f.inject_cells(road, 0.5, mode, 77) == g.inject(0.5, mode, 77)
        assert f.states().tobytes() == g.states().tobytes()
        assert f.inject_cells(road, 0.5, mode, 78, count=False) is None and g.inject(0.5, mode, 78, count=False) is None
        assert f.states().tobytes() == g.states().tobytes()


def test_inject_cells_leaves_weights_and_generator_alone(rec_scene):
    f, r = _handle(rec_scene, "fixed", 1024)
    f.set_states(_spread_states(rec_scene, 1024, 7, False))
    f.propagate(0.3, 0.1, 0.005)
    f.update(r, rec_scene.cfg.res)
    g, _ = _handle(rec_scene, "fixed", 1024)
    g.set_states(_spread_states(rec_scene, 1024, 7, False))
    g.propagate(0.3, 0.1, 0.005)
    g.update(r, rec_scene.cfg.res)
    before = _snapshot(f, states=False)
    road = RR.road_cells(rec_scene.class_maps)
    assert f.inject_cells(road[:50], 0.25, 0, 3) == g.inject(0.25, 0, 3) > 100
    assert _snapshot(f, states=False) == before
    # the generator stands where it stood: after equal states the next step is the twin's
    cur = g.states()
    f.set_states(cur)
    g.set_states(cur)
    for h in (f, g):
        h.propagate(0.2, 0.0, 0.01)
        h.update(r, rec_scene.cfg.res)
    assert _snapshot(f) == _snapshot(g)


# ---- what the handle refuses -----------------------------------------------------------------------------------------------------------------
def test_handle_refusals_write_nothing(scene):
    from top_down_renderer_amd import batch
    res = C.c_float(scene.cfg.res)
    f, r = _prepared(scene, "fixed")
    L = f.L
    before = _snapshot(f)
    ok = _lattice(scene, 1, 3)
    G = ok.nx * ok.ny
    w, t, v = (np.full(G * k, SENT, F32) for k in (1, 1, 3))
    peaks = np.full((8, 4), -5, np.int32)
    n_peaks, listed, out = C.c_int64(777), C.c_int64(777), C.c_int64(777)
    cells = np.array([5, 6, 7], np.uint32)
    ptr = lambda a: a.ctypes.data_as(vp) if a is not None else None

    def refused(rc, word):
        assert rc == -1 and word in L.tdr_last_error().decode(), (rc, L.tdr_last_error())
        assert (w == SENT).all() and (t == SENT).all() and (v == SENT).all() and (peaks == -5).all()
        assert n_peaks.value == 777 and listed.value == 777 and out.value == 777
        assert _snapshot(f) == before

    def search(h=f.h, rh=r.h, rs=res, s=ok, R=2, Kp=8):
        return L.tdr_filter_grid_search(h, None, rh, rs, C.byref(_c(s)) if s is not None else None, ptr(w), ptr(t), ptr(v), R, Kp,
                                        ptr(peaks), C.byref(n_peaks), C.byref(listed))

    def inj(h=f.h, c=cells, n=3, p=0.5, mode=0):
        return L.tdr_filter_inject_cells(h, ptr(c), n, C.c_double(p), mode, 1, C.byref(out))

    refused(search(h=None), "null")
    refused(search(s=None), "null")
    for s, word in ((ok._replace(step=0), "step"), (ok._replace(nx=0), "lattice"), (ok._replace(ny=-1), "lattice"),
                    (ok._replace(nx=4097, ny=4097), "lattice"), (ok._replace(road_only=2), "road_only"),
                    (ok._replace(heading_mode=2), "heading_mode"), (ok._replace(n_headings=0), "n_headings"),
                    (ok._replace(n_headings=4097), "n_headings"), (ok._replace(heading_mode=0), "n_headings"),
                    (ok._replace(theta0=NAN), "theta0"), (ok._replace(dtheta=float("inf")), "dtheta"),
                    (ok._replace(scale=0.0), "scale"), (ok._replace(scale=NAN), "scale")):
        refused(search(s=s), word)
    for bad in (0.0, -1.0, NAN, float("inf")):
        refused(search(rs=C.c_float(bad)), "res =")
    for R in (-1, 17):
        refused(search(R=R), "nms_radius")
    for Kp in (-1, 4097):
        refused(search(Kp=Kp), "max_peaks")
    refused(search(rh=None), "no scan")                          # the filter kept no scan: it was updated from the renderer
    other = batch.Renderer(scene.lut)
    refused(search(rh=other.h), "no scan")
    other.render_polar(scene.pts, 4, 3, scene.cfg.res, float(scene.cfg.ang_res), scene.cfg.ncls, scene.cfg.nb, scene.cfg.nr + 1)
    refused(search(rh=other.h), "shape")
    e, _ = _handle(scene, "fixed", 64)
    refused(search(h=e.h), "no particles")
    refused(inj(h=e.h), "no particles")
    refused(inj(h=None), "null")
    refused(inj(c=None), "null")
    for p in (-0.001, 1.001, NAN, float("inf")):
        refused(inj(p=p), "p =")
    for mode in (-1, 2):
        refused(inj(mode=mode), "heading_mode")
    for n in (0, -1, (1 << 24) + 1):
        refused(inj(n=n), "n_cells")
    ncell = scene.cfg.map_size ** 2
    refused(inj(c=np.array([5, ncell, 7], np.uint32)), "cells")
    assert inj(c=np.array([5, ncell - 1, 7], np.uint32), p=0.0) == 0 and out.value == 0 and _snapshot(f) == before


def test_a_sharded_filter_is_refused(scene):
    """One rank over the callback transport, as tests/test_recovery.py builds it."""
    from top_down_renderer_amd import FilterParams
    from top_down_renderer_amd._lib import check
    f, r = _handle(scene, "fixed", 64)
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
        out = C.c_int64(777)
        sp = _c(_lattice(scene, 0, 1))
        assert L.tdr_filter_grid_search(sh, None, r.h, C.c_float(scene.cfg.res), C.byref(sp), None, None, None, 2, 0, None, C.byref(out),
                                        None) == -1
        assert "sharded" in L.tdr_last_error().decode() and out.value == 777
        cells = np.array([5], np.uint32)
        assert L.tdr_filter_inject_cells(sh, cells.ctypes.data_as(vp), 1, C.c_double(0.5), 0, 1, C.byref(out)) == -1
        assert "sharded" in L.tdr_last_error().decode() and out.value == 777
        got = np.zeros(64, RR.STATE_DTYPE)
        check(L.tdr_filter_get_states(sh, got.ctypes.data_as(vp), 64))
        assert got.tobytes() == st.tobytes()
    finally:
        L.tdr_filter_destroy(sh)
        L.tdr_comm_destroy(comm)


# ---- the closed loop: the kidnapped robot found with one search ------------------------------------------------------------------------------
GRID_STEPS_NEEDED = 2       # measured on the MI355X: the max-likelihood particle is within RADIUS from the 2nd step after the move on
GRID_STEPS_ALLOWED = 4      # twice that (the rule of STEPS_NEEDED / STEPS_ALLOWED in tests/test_recovery.py)
GRID_INJECT_P, GRID_INJECT_SEED = 0.05, 2026


def grid_kidnap_run(K, steps_after):
    """tests/test_recovery.py::kidnap_run with the search in place of the tracker: 10 steps at the true pose of c1, then the
    scans come from the road pose at least 400 px away.  After the first update on the new scan ONE gridSearch (step 8, road
    only, no heading, R = 2, K = 8) and ONE injectCells of its peaks' cells (p = 0.05, no heading).  Returns (the new pose,
    the search's result, per further step: distance of the max-likelihood particle to the new pose, particles within RADIUS)."""
    from top_down_renderer_amd import synth
    sc, pose2, pts2 = c1_scene()
    cfg = sc.cfg
    f, r = _python_filter(K, sc, synth.make_particles(cfg, sc.lab, sc.pose, np.random.default_rng(78), n=4000, uniform_frac=0.0))

    def step():
        f.propagate((0.2, 0.0), 0.0)
        f.update(r.last_scan(), None, cfg.res)

    r.renderSemanticTopDown(sc.pts, cfg.res, cfg.ang_res)
    for _ in range(10):
        step()
    ml = f.maxLikelihood()
    assert np.hypot(ml[0] - sc.pose[0], ml[1] - sc.pose[1]) < 100      # the cloud sits on the first pose
    r.renderSemanticTopDown(pts2, cfg.res, cfg.ang_res)
    trace, found = [], None
    for s in range(steps_after):
        step()
        if s == 0:
            found = f.gridSearch(r.last_scan(), cfg.res, _c(c1_spec()), 2, 8)
            injected = f.injectCells(found.peaks["cell"], GRID_INJECT_P, 0, GRID_INJECT_SEED)
            assert injected > 100
        ml = f.maxLikelihood()
        st = f.get_states()
        x = st["dx_m"] * st["scale"] + st["init_x_px"]
        y = st["dy_m"] * st["scale"] + st["init_y_px"]
        trace.append((float(np.hypot(ml[0] - pose2[0], ml[1] - pose2[1])), int((np.hypot(x - pose2[0], y - pose2[1]) < RADIUS).sum())))
    return pose2, found, trace


def test_one_search_finds_the_robot_again(K):
    """The max-likelihood particle is within RADIUS of the new pose after GRID_STEPS_ALLOWED steps.  Measured on the MI355X:
    the search lists 3324 points and finds 156 peaks; the top one (weight 6.5135) stands 3.2 px from the new pose, the
    other seven of the first eight 320 to 880 px away (6.2102 and below).  The injection writes about 200 slots onto the
    eight cells, 20 of them within RADIUS of the new pose.  Step 1 is the update on the first scan after the move, behind
    which the search and the injection run: its max-likelihood particle is still the old cloud's (471 px).  From step 2
    (GRID_STEPS_NEEDED) on it is within 3 to 8 px on every one of 30 steps, and 1520 of the 4000 particles are within
    RADIUS after 30.  For comparison the uniform injection needed 9 steps and sensor resetting 5."""
    pose2, found, trace = grid_kidnap_run(K, GRID_STEPS_ALLOWED)
    stays = next((i + 1 for i in range(len(trace)) if all(d < RADIUS for d, _ in trace[i:])), None)
    print("grid kidnap trace:", stays, peak_distance(found.peaks[0], pose2), trace)
    assert peak_distance(found.peaks[0], pose2) < BASIN_PX
    assert stays is not None and GRID_STEPS_NEEDED <= stays <= GRID_STEPS_ALLOWED, (stays, trace)
    assert trace[-1][0] < RADIUS, (stays, trace)
    assert trace[-1][1] > 0
