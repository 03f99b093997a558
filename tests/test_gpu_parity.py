"""GPU parity tests: the HIP path (through the C ABI of libtdr_hip.so) against the CPU oracle on the same seeded inputs
and against the committed golden fixtures.  Run on the MI355X box with `pytest -m gpu`.

Tolerances (BASELINE.json north_star): per-particle weights within 1e-5 relative; resample indices bit-exact on
identical weight inputs; raster counts exact (the kernel's atan2f is glibc's algorithm restated, test_atan2f_bit_exact).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WEIGHT_RTOL = 1e-5


@pytest.fixture(scope="module")
def tdr():
    import torch
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd.kernels import HipKernels

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    k = HipKernels()   # raises if libtdr_hip.so is missing: the product has no CPU fallback
    return pkg, k


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "micro.npz"), allow_pickle=False)


def _micro_map(pkg, k, g, nb, nr, ang_res):
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), g["class_maps"], g["class_mask"], kernels=k)
    m.samplePtsPolar((nb, nr), ang_res)
    return m


def _assert_weights(w, ref, rtol=WEIGHT_RTOL):
    assert np.array_equal(np.isnan(w), np.isnan(ref)), (np.isnan(w).sum(), np.isnan(ref).sum())
    ok = ~np.isnan(ref)
    denom = np.maximum(np.abs(ref[ok]), 1e-30)
    err = np.abs(w[ok] - ref[ok]) / denom
    assert err.max(initial=0.0) <= rtol, f"max rel err {err.max():.3e}"


# ---- A1/A2 raster ----------------------------------------------------------------------------------------------------
def test_raster_polar_golden_and_layouts(tdr, g):
    pkg, k = tdr
    ncls, nb, nr, _ = [int(v) for v in g["shape"]]
    r = pkg.ScanRendererPolar(g["lut"], kernels=k)
    imgs = [np.zeros((nb, nr), np.float32, order="F") for _ in range(ncls)]
    r.renderSemanticTopDown(g["pts"], float(g["res"]), float(g["ang_res"]), imgs)
    got = np.stack([im.ravel(order="F") for im in imgs])
    assert np.array_equal(got, g["scan"])
    # pcl::PointXYZI-strided input gives the same image
    pts = g["pts"]
    pcl = np.zeros((len(pts), 8), np.float32)
    pcl[:, :3], pcl[:, 3], pcl[:, 4] = pts[:, :3], 1.0, pts[:, 3]
    imgs2 = [np.ones((nb, nr), np.float32, order="F") for _ in range(ncls)]
    r.renderSemanticTopDown(pcl, float(g["res"]), float(g["ang_res"]), imgs2)
    assert all(np.array_equal(a, b) for a, b in zip(imgs, imgs2))
    # packed scoring layout: [nr][nb][rf], last slot = sum over classes
    rf = k.lib.tdr_rec_floats(ncls)
    pk = r.last_scan()[1].cpu().numpy().reshape(nr, nb, rf)
    for c in range(ncls):
        assert np.array_equal(pk[:, :, c].ravel(), g["scan"][c])
    assert np.array_equal(pk[:, :, rf - 1].ravel(), g["scan"].sum(0))


def test_raster_cart_golden(tdr, g):
    pkg, k = tdr
    r = pkg.ScanRenderer(g["lut"], kernels=k)
    imgs = [np.zeros((12, 10), np.float32, order="F") for _ in range(3)]
    r.renderSemanticTopDown(g["pts"], 0.5, imgs)
    got = np.stack([im.ravel(order="F") for im in imgs])
    assert np.array_equal(got, g["scan_cart_12x10_res0p5"])


def test_raster_empty_cloud(tdr, g):
    pkg, k = tdr
    r = pkg.ScanRendererPolar(g["lut"], kernels=k)
    imgs = [np.ones((16, 8), np.float32, order="F") for _ in range(3)]
    r.renderSemanticTopDown(np.zeros((0, 4), np.float32), 1.0, float(g["ang_res"]), imgs)
    assert not np.stack(imgs).any()


def test_raster_drops_non_finite_points_like_the_reference(tdr, oracle, g):
    """Organised PCL clouds (is_dense == false) carry NaN points; inf and NaN labels can occur too.  On x86-64 the
    reference's float -> int conversions turn them into INT_MIN, which fails its range tests
    (scan_renderer_polar.cpp:100-102, scan_renderer.cpp:69-71): such points are dropped, in both renderers and in
    both raster phases (with and without the key workspace)."""
    pkg, k = tdr
    import ctypes as C
    import torch
    ncls, nb, nr, _ = [int(v) for v in g["shape"]]
    pts = np.ascontiguousarray(g["pts"], np.float32).copy()
    rng = np.random.default_rng(12)
    bad = rng.choice(len(pts), len(pts) // 3, replace=False)
    vals = np.asarray([np.nan, np.inf, -np.inf], np.float32)
    pts[bad[0::4], 0] = vals[rng.integers(0, 3, len(bad[0::4]))]
    pts[bad[1::4], 1] = vals[rng.integers(0, 3, len(bad[1::4]))]
    pts[bad[2::4], 3] = vals[rng.integers(0, 3, len(bad[2::4]))]          # label
    pts[bad[3::4], 0] = np.nan
    pts[bad[3::4], 1] = 0.0
    pts = np.concatenate([pts, np.asarray([[1e30, 1.0, 0, 1], [1.0, -1e30, 0, 1], [2.0, 3.0, 0, -0.5],
                                           [2.0, 3.0, 0, 1e10], [2.0, 3.0, 0, 255.9]], np.float32)])
    lut = np.asarray(g["lut"], np.int32)
    res, ang = float(g["res"]), float(g["ang_res"])
    with np.errstate(all="ignore"):
        ref_p = oracle.raster_polar(pts, res, ang, lut, ncls, nb, nr)
        ref_c = oracle.raster_cart(pts, 0.5, lut, ncls, 12, 10)
    assert ref_p.sum() > 0 and ref_p.sum() < g["scan"].sum()              # some points really were dropped
    pd, ld = k.to_device(pts), k.to_device(lut)
    ws = k.empty((int(k.lib.tdr_raster_workspace_bytes(len(pts))),), torch.uint8)
    for w in (None, ws):
        wp = C.c_void_p(w.data_ptr()) if w is not None else None
        img = k.zeros((ncls, nb * nr))
        assert k.lib.tdr_k_raster_polar(C.c_void_p(pd.data_ptr()), 4, 3, len(pts), C.c_float(res), C.c_float(ang),
                                        C.c_void_p(ld.data_ptr()), ncls, nb, nr, C.c_void_p(img.data_ptr()), None, wp,
                                        k.stream()) == 0
        assert np.array_equal(img.cpu().numpy(), ref_p)
        img = k.zeros((ncls, 12 * 10))
        assert k.lib.tdr_k_raster_cart(C.c_void_p(pd.data_ptr()), 4, 3, len(pts), C.c_float(0.5),
                                       C.c_void_p(ld.data_ptr()), ncls, 12, 10, C.c_void_p(img.data_ptr()), None, wp,
                                       k.stream()) == 0
        assert np.array_equal(img.cpu().numpy(), ref_c)


@pytest.mark.parametrize("name", ["c1", "c2"])
def test_raster_polar_vs_oracle(tdr, oracle, name):
    from top_down_renderer_amd import synth
    pkg, k = tdr
    cfg = synth.CONFIGS[name]
    rng = np.random.default_rng(cfg.seed)
    lab = synth.make_label_image(min(cfg.map_size, 1000), cfg.ncls, rng)
    pose = synth.pick_true_pose(lab, rng, 50)
    pts = synth.make_scan(cfg, lab, pose, rng)
    lut = synth.make_lut(cfg.ncls)
    ref = oracle.raster_polar(pts, cfg.res, cfg.ang_res, lut, cfg.ncls, cfg.nb, cfg.nr)
    r = pkg.ScanRendererPolar(lut, kernels=k)
    r.set_output_shape(cfg.ncls, cfg.nb, cfg.nr)
    r.renderSemanticTopDown(pts, cfg.res, cfg.ang_res)
    got = r.last_images().cpu().numpy()
    # integer work is bit-exact: the raster kernel's atan2f is glibc's algorithm restated (test_atan2f_bit_exact)
    assert np.array_equal(got, ref)


def test_raster_image_column_larger_than_64kb_of_lds(tdr, oracle):
    """6 classes x 4096 direction bins: one image column is 96 KB of LDS counters — more than the default dynamic-LDS
    limit, within the 160 KB of a CU."""
    from top_down_renderer_amd import synth
    pkg, k = tdr
    ncls, nb, nr = 6, 4096, 24
    rng = np.random.default_rng(21)
    pts = np.zeros((60_000, 4), np.float32)
    pts[:, :2] = rng.normal(0, 9, (len(pts), 2))
    pts[:, 3] = rng.integers(0, ncls, len(pts))
    lut = synth.make_lut(ncls)
    ang = np.float32(2 * np.pi / nb)
    ref = oracle.raster_polar(pts, 1.0, ang, lut, ncls, nb, nr)
    r = pkg.ScanRendererPolar(lut, kernels=k)
    r.set_output_shape(ncls, nb, nr)
    r.renderSemanticTopDown(pts, 1.0, ang)
    assert np.array_equal(r.last_images().cpu().numpy(), ref) and ref.sum() > 10_000


def test_raster_with_and_without_workspace(tdr, oracle):
    """tdr_k_raster_polar / _cart: the two-phase raster (bins once, tiles stream keys) and the single-phase one (no
    workspace) write the same images."""
    pkg, k = tdr
    import ctypes as C
    from top_down_renderer_amd import synth
    sc = synth.make_scene("c1", with_particles=False)
    cfg = sc.cfg
    pts = k.to_device(np.ascontiguousarray(sc.pts, np.float32))
    lut = k.to_device(np.asarray(sc.lut, np.int32))
    n = len(sc.pts)
    rf = k.lib.tdr_rec_floats(cfg.ncls)
    ref = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
    ws = k.empty((int(k.lib.tdr_raster_workspace_bytes(n)),), __import__("torch").uint8)
    outs = []
    for w in (None, ws):
        img, pk = k.zeros((cfg.ncls, cfg.nb * cfg.nr)), k.zeros((cfg.nb * cfg.nr * rf,))
        assert k.lib.tdr_k_raster_polar(C.c_void_p(pts.data_ptr()), 4, 3, n, C.c_float(cfg.res), C.c_float(cfg.ang_res),
                                        C.c_void_p(lut.data_ptr()), cfg.ncls, cfg.nb, cfg.nr, C.c_void_p(img.data_ptr()),
                                        C.c_void_p(pk.data_ptr()), C.c_void_p(w.data_ptr()) if w is not None else None,
                                        k.stream()) == 0
        outs.append((img.cpu().numpy(), pk.cpu().numpy()))
        assert np.array_equal(outs[-1][0], ref)
    assert np.array_equal(outs[0][1], outs[1][1])
    refc = oracle.raster_cart(sc.pts, cfg.res, sc.lut, cfg.ncls, 50, 64)
    for w in (None, ws):
        img = k.zeros((cfg.ncls, 50 * 64))
        assert k.lib.tdr_k_raster_cart(C.c_void_p(pts.data_ptr()), 4, 3, n, C.c_float(cfg.res), C.c_void_p(lut.data_ptr()),
                                       cfg.ncls, 50, 64, C.c_void_p(img.data_ptr()), None,
                                       C.c_void_p(w.data_ptr()) if w is not None else None, k.stream()) == 0
        assert np.array_equal(img.cpu().numpy(), refc)


def test_atan2f_bit_exact(tdr):
    """The raster kernel's atan2f against the host libm the reference calls (glibc atan2f), bit for bit."""
    pkg, k = tdr
    import ctypes as C
    import ctypes.util
    libm = C.CDLL(ctypes.util.find_library("m"))
    rng = np.random.default_rng(5)
    n = 1 << 22
    y = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 50.0, 4000.0], n)).astype(np.float32)
    x = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 50.0, 4000.0], n)).astype(np.float32)
    special = np.asarray([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-38, -1e-38, 3e38, 2.0 ** -30, 0.4375,
                          0.6875, 1.1875, 2.4375, 2.0 ** 25, 2.0 ** 61], np.float32)
    yy, xx = np.meshgrid(special, special)
    y = np.concatenate([y, yy.ravel(), np.ones(len(special), np.float32)])
    x = np.concatenate([x, xx.ravel(), special])
    n = len(y)
    out = k.zeros((n,))
    yd, xd = k.to_device(y), k.to_device(x)
    assert k.lib.tdr_k_selftest_atan2(C.c_void_p(yd.data_ptr()), C.c_void_p(xd.data_ptr()), n,
                                      C.c_void_p(out.data_ptr()), k.stream()) == 0
    ref = np.empty(n, np.float32)
    # vectorised call into glibc through numpy's float32 arctan2 would use numpy's own SIMD kernels: call libm directly
    fn = libm.atan2f
    fn.restype, fn.argtypes = C.c_float, [C.c_float, C.c_float]
    step = max(1, n // 200_000)          # 200k spot checks through ctypes + every special pair
    idx = np.unique(np.concatenate([np.arange(0, n, step), np.arange(n - len(special) ** 2 - len(special), n)]))
    got = out.cpu().numpy()
    for i in idx:
        r = np.float32(fn(float(y[i]), float(x[i])))
        assert (np.isnan(r) and np.isnan(got[i])) or r.view(np.uint32) == got[i].view(np.uint32), (y[i], x[i], r, got[i])


def test_fast_coordinate_rounding_equals_roundf(tdr):
    """The scoring loop rounds sample coordinates with floor(fl(x + (0.5 - 2^-25))) after clamping to [-1, limit];
    it must equal C roundf (Eigen's .round(), top_down_map_polar.cpp:31) for every float it can meet."""
    pkg, k = tdr
    import ctypes as C
    import torch
    limit = 4000.0

    def check(x):
        xd = k.to_device(x)
        out = k.zeros((len(x),), torch.int32)
        assert k.lib.tdr_k_selftest_round(C.c_void_p(xd.data_ptr()), len(x), C.c_float(limit),
                                          C.c_void_p(out.data_ptr()), k.stream()) == 0
        xc = np.clip(x.astype(np.float64), -1.0, limit)
        ref = (np.sign(xc) * np.floor(np.abs(xc) + 0.5)).astype(np.int32)
        got = out.cpu().numpy()
        bad = np.nonzero(got != ref)[0]
        assert len(bad) == 0, (x[bad[:5]], got[bad[:5]], ref[bad[:5]])

    # every float in [0, 4] and in [-1.5, -0] (bit patterns are ordered within a sign)
    for lo, hi in ((0x00000000, 0x40800000), (0x80000000, 0xBFC00000)):
        for start in range(lo, hi + 1, 1 << 25):
            bits = np.arange(start, min(start + (1 << 25), hi + 1), dtype=np.uint32)
            check(bits.view(np.float32))
    rng = np.random.default_rng(0)
    check((rng.random(1 << 24) * 4200 - 100).astype(np.float32))
    half = (np.arange(-4, 8200, dtype=np.float32) * 0.5)
    check(np.concatenate([half, np.nextafter(half, np.float32(-1e9)), np.nextafter(half, np.float32(1e9)),
                          np.asarray([np.inf, -np.inf, 1e30, -1e30], np.float32)]))


# ---- A4 table, A5+A8+A9 score ---------------------------------------------------------------------------------------------
def test_polar_table_matches_oracle(tdr, oracle):
    pkg, k = tdr
    for nb, nr, resol in ((16, 8, 1.0), (100, 25, 1.0), (256, 256, 1.0), (100, 50, 0.5)):
        tab = np.empty((nb * nr, 2), np.float32)
        import ctypes as C
        assert k.lib.tdr_polar_table_host(nb, nr, C.c_float(np.float32(2 * np.pi / nb)), C.c_float(resol),
                                          tab.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(tab, oracle.polar_table(nb, nr, np.float32(2 * np.pi / nb), resol))


@pytest.mark.parametrize("name,kw", [("default", {}), ("force_on_map", {"force_on_map": True}),
                                     ("scale_unknown", {"fixed_scale": -1.0, "class_weights": [1.0, 0.5, 2.0],
                                                        "regularization": 0.7})])
def test_score_golden(tdr, oracle, g, name, kw):
    pkg, k = tdr
    ncls, nb, nr, _ = [int(v) for v in g["shape"]]
    m = _micro_map(pkg, k, g, nb, nr, float(g["ang_res"]))
    assert np.array_equal(m.dev.tab_host, g["table"])
    base = dict(fixed_scale=1.0)
    base.update(kw)
    f = pkg.ParticleFilter(32, m, pkg.FilterParams(**base), seed=7, kernels=k, init_particles=False)
    states = np.ascontiguousarray(g["states_in"]).view(pkg.STATE_DTYPE).reshape(-1)
    f.set_states(states)
    f.update(g["scan"], None, float(g["res"]))
    ref_w = g[f"weights_{name}"]
    _assert_weights(f.raw_weights(), ref_w)
    # the init search wrote theta / have_init into the pre-resample buffer
    pre = k.states_to_host(f.st_new, 32, pkg.STATE_DTYPE)
    gated = ref_w == 0
    assert np.all(pre["have_init"][~gated] == 1)
    was_init = states["have_init"] == 1
    assert np.array_equal(pre["theta"][was_init | gated], states["theta"][was_init | gated])   # untouched
    # Un-initialised particles: the chosen rotation must be the reference's, or — where two rotations tie within
    # float rounding (the reference's own Eigen sums have unspecified order) — one whose cost the oracle rates
    # equally good.
    differs = np.nonzero(~np.isclose(pre["theta"], g[f"theta_after_{name}"], rtol=0, atol=0))[0]
    if len(differs):
        chk = states.copy()
        chk["theta"][differs] = pre["theta"][differs]
        chk["have_init"] = 1
        om = oracle.OracleMap(g["class_maps"], g["class_mask"], 1.0)
        w_chk = oracle.compute_weights(om, g["table"], nb, nr, g["scan"], float(g["res"]),
                                       oracle.make_params(ncls, **base), chk)
        _assert_weights(w_chk[differs], ref_w[differs])


def _c1_scene(oracle):
    from top_down_renderer_amd import synth
    sc = synth.make_scene("c1")
    cfg = sc.cfg
    om = oracle.OracleMap(sc.class_maps, sc.class_mask, 1.0)
    scan = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
    tab = oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res, 1.0)
    return sc, cfg, om, scan, tab


def test_score_c1_vs_oracle_and_order_invariance(tdr, oracle):
    pkg, k = tdr
    sc, cfg, om, scan, tab = _c1_scene(oracle)
    st = sc.states.copy()
    st["dx_m"] = np.random.default_rng(1).normal(0, 2, len(st)).astype(np.float32)
    st["scale"] = 1.0
    ref = oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan, cfg.res, oracle.make_params(cfg.ncls), st.copy())
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    out = []
    for loc in (0, 1):
        f = pkg.ParticleFilter(len(st), m, pkg.FilterParams(fixed_scale=1.0), seed=3, kernels=k,
                               init_particles=False, locality_every=loc)
        f.set_states(st)
        f.update(scan, None, cfg.res)
        out.append(f.raw_weights())
        _assert_weights(out[-1], ref)
    # the locality processing order changes which lane scores a particle, never its result
    assert np.array_equal(out[0], out[1], equal_nan=True)


def test_score_non_unit_scale_and_resolution(tdr, oracle):
    """scale != 1 per particle, res != 1, map resolution != 1, nb not a multiple of the unroll, 6 classes."""
    from top_down_renderer_amd import synth
    pkg, k = tdr
    cfg = synth.Config("odd", 5000, 6, 100, 25, 600, 256, seed=77, res=2.5, map_resolution=0.5)
    sc = synth.make_scene(cfg)
    om = oracle.OracleMap(sc.class_maps, sc.class_mask, cfg.map_resolution)
    scan = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
    tab = oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res, cfg.map_resolution)
    st = sc.states.copy()
    rng = np.random.default_rng(2)
    st["scale"] = rng.uniform(0.6, 1.6, len(st)).astype(np.float32)
    st["dy_m"] = rng.normal(0, 3, len(st)).astype(np.float32)
    cw = [1.0, 0.5, 2.0, 1.5, 0.25, 1.0]
    fpo = oracle.make_params(cfg.ncls, fixed_scale=-1.0, class_weights=cw, regularization=0.7, force_on_map=True)
    ref = oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan, cfg.res, fpo, st.copy())
    m = pkg.TopDownMapPolar(pkg.Params(resolution=cfg.map_resolution), sc.class_maps, sc.class_mask, kernels=k)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    f = pkg.ParticleFilter(len(st), m, pkg.FilterParams(fixed_scale=-1.0, class_weights=cw, regularization=0.7,
                                                        force_on_map=True), kernels=k, init_particles=False)
    f.set_states(st)
    f.update(scan, None, cfg.res)
    _assert_weights(f.raw_weights(), ref)


def test_score_cartesian_vs_oracle(tdr, oracle):
    """BASELINE config 4's path at a small shape: Cartesian render (A2) + Cartesian window gather (A7) scored with
    shift 0.  The reference has no Cartesian score function; both sides implement the definition in include/tdr.h."""
    from top_down_renderer_amd import synth
    pkg, k = tdr
    cfg = synth.Config("cart", 8000, 6, 50, 64, 700, 512, polar=False, seed=31, res=0.75)
    sc = synth.make_scene(cfg)
    rows, cols = cfg.nb, cfg.nr
    st = sc.states.copy()
    rng = np.random.default_rng(3)
    st["scale"] = rng.uniform(0.8, 1.25, len(st)).astype(np.float32)
    st["dx_m"] = rng.normal(0, 2, len(st)).astype(np.float32)
    st["init_x_px"][:8] = np.asarray([-50, 5, 700, 695, 350, 350, 0.5, 699.5], np.float32)   # off / at the border
    st["init_y_px"][:8] = np.asarray([350, 350, 350, 350, -40, 698, 0.5, 699.5], np.float32)
    om = oracle.OracleMap(sc.class_maps, sc.class_mask, 1.0)
    scan = oracle.raster_cart(sc.pts, cfg.res, sc.lut, cfg.ncls, rows, cols)
    cw = [1.0, 0.5, 2.0, 1.5, 0.25, 1.0]
    ref = oracle.compute_weights_cart(om, rows, cols, scan, cfg.res, oracle.make_params(cfg.ncls, class_weights=cw),
                                      st.copy())
    assert np.isnan(ref).any() and (~np.isnan(ref)).sum() > 400
    m = pkg.TopDownMap(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.setWindow(rows, cols)
    r = pkg.ScanRenderer(sc.lut, kernels=k)
    r.set_output_shape(cfg.ncls, rows, cols)
    r.renderSemanticTopDown(sc.pts, cfg.res)
    assert np.array_equal(r.last_images().cpu().numpy(), scan)
    for loc in (0, 1):
        f = pkg.ParticleFilter(len(st), m, pkg.FilterParams(fixed_scale=1.0, class_weights=cw), kernels=k,
                               init_particles=False, locality_every=loc)
        f.set_states(st)
        f.update(r.last_scan(), None, cfg.res)
        _assert_weights(f.raw_weights(), ref)   # cos/sin of theta are the host libm's bit for bit (test_libm.py)


@pytest.mark.parametrize("ncls,rows,cols,kind", [(6, 50, 64, "scan"), (3, 33, 21, "scan"), (9, 18, 40, "scan"),
                                                 (6, 37, 29, "dense"), (6, 24, 24, "empty"), (6, 20, 36, "inf")])
def test_cart_skip_kernel_equals_general_kernel(tdr, oracle, ncls, rows, cols, kind):
    """score_cart_skip_kernel (csrc/tdr_score_cart.hip: scalar scan descriptors, an empty bin costs one known-mask gather)
    against score_cart_kernel on the same inputs: raw weights array-equal, and within 1e-5 of the oracle.  Window shapes
    with rows % 4 != 0 (the tail rows), a scan with several classes in every bin, an empty scan, and a non-finite scan
    value (0 x inf must stay NaN: nothing may be skipped in that bin)."""
    from top_down_renderer_amd import synth
    pkg, k = tdr
    cfg = synth.Config("cartskip", 6000, ncls, rows, cols, 500, 700, polar=False, seed=77 + ncls + rows, res=0.75)
    sc = synth.make_scene(cfg)
    st = sc.states.copy()
    rng = np.random.default_rng(5)
    st["scale"] = rng.uniform(0.8, 1.25, len(st)).astype(np.float32)
    st["init_x_px"][:6] = np.asarray([-50, 5, 500, 495, 250, 0.5], np.float32)          # off / at the border
    st["init_y_px"][:6] = np.asarray([250, 250, 250, 250, -40, 0.5], np.float32)
    scan = oracle.raster_cart(sc.pts, cfg.res, sc.lut, ncls, rows, cols)
    if kind == "dense":
        scan = rng.integers(0, 3, scan.shape).astype(np.float32)
    elif kind == "empty":
        scan = np.zeros_like(scan)
    elif kind == "inf":
        scan = scan.copy()
        scan[1, 7] = np.inf
        scan[0, 11] = np.nan
    om = oracle.OracleMap(sc.class_maps, sc.class_mask, 1.0)
    with np.errstate(all="ignore"):
        ref = oracle.compute_weights_cart(om, rows, cols, scan, cfg.res, oracle.make_params(ncls), st.copy())
    m = pkg.TopDownMap(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.setWindow(rows, cols)
    before, before_form = k.lib.tdr_config_cart_skip(-1), k.lib.tdr_config_shift_uniform(-1)
    got = []
    try:
        k.lib.tdr_config_shift_uniform(0)   # the two FLOAT kernels (the integer form: tests/test_ray.py)
        for on in (0, 1):
            k.lib.tdr_config_cart_skip(on)
            f = pkg.ParticleFilter(len(st), m, pkg.FilterParams(fixed_scale=1.0), kernels=k, init_particles=False,
                                   locality_every=1)
            f.set_states(st)
            f.update(np.ascontiguousarray(scan, np.float32), None, cfg.res)
            got.append(f.raw_weights())
    finally:
        k.lib.tdr_config_cart_skip(before)
        k.lib.tdr_config_shift_uniform(before_form)
    assert np.array_equal(got[0], got[1], equal_nan=True)
    _assert_weights(got[1], ref)


def test_local_map_polar_and_cartesian_bit_exact(tdr, oracle):
    """getLocalMap materialised (top_down_map_polar.cpp:21-53, top_down_map.cpp:429-459): the window addressing of the
    scoring kernels as a function of its own — every gathered value and mask bit against the oracle, for poses inside,
    at the border of and outside the map, several scales / rotations / resolutions."""
    from top_down_renderer_amd import synth
    pkg, k = tdr
    cfg = synth.Config("lm", 2000, 5, 36, 20, 300, 8, seed=91, res=1.3, map_resolution=0.5)
    sc = synth.make_scene(cfg, with_particles=False)
    rows, cols = 270, 300                      # non-square map
    maps, mask = np.ascontiguousarray(sc.class_maps[:, :rows, :cols]), np.ascontiguousarray(sc.class_mask[:rows, :cols])
    om = oracle.OracleMap(maps, mask, cfg.map_resolution)
    tab = oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res, cfg.map_resolution)
    mp = pkg.TopDownMapPolar(pkg.Params(resolution=cfg.map_resolution), maps, mask, kernels=k)
    mp.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    mc = pkg.TopDownMap(pkg.Params(resolution=cfg.map_resolution), maps, mask, kernels=k)
    rng = np.random.default_rng(17)
    poses = [(75.0, 60.0), (0.2, 0.2), (149.9, 134.9), (-40.0, 30.0), (400.0, 400.0), (75.25, -3.0)]
    poses += [tuple(rng.uniform(-20, 170, 2)) for _ in range(10)]
    for cx, cy in poses:
        scale, res, rot = float(rng.uniform(0.4, 3.0)), float(rng.choice([0.5, 1.0, 1.3])), float(rng.uniform(-4, 4))
        d_o, k_o = oracle.local_map_polar(om, tab, cx, cy, scale, res)
        d, m = mp.getLocalMap((cx, cy), scale, res)
        assert np.array_equal(np.stack([x.T.ravel() for x in d]), d_o) and np.array_equal(m.T.ravel(), k_o)
        wr, wc = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        d_o, k_o = oracle.local_map_cart(om, cx, cy, rot, res, wr, wc)
        d, m = mc.getLocalMap((cx, cy), rot, res, (wr, wc))
        got = np.stack([x.T.ravel() for x in d])
        assert np.array_equal(got, d_o) and np.array_equal(m.T.ravel(), k_o)   # every sample, every mask bit
    d1, m1 = mp.getLocalMap((75.0, 60.0), 1.3)                     # 3-argument overload: scale = 1 (:78-81)
    d2, m2 = mp.getLocalMap((75.0, 60.0), 1.0, 1.3)
    assert all(np.array_equal(a, b) for a, b in zip(d1, d2)) and np.array_equal(m1, m2)


# ---- compact map records ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls,rows,cols", [(2, 97, 130), (3, 200, 150), (6, 301, 257), (7, 64, 64), (10, 90, 75)])
def test_compact_map_round_trip(tdr, ncls, rows, cols):
    """csrc/tdr_cmap.hip: the compact records (10-bit dictionary indices, tiled) decode to the dense records bit for bit,
    for every record width (1, 2 and 4 dwords), non-square maps and maps whose sides are not multiples of the tile."""
    from top_down_renderer_amd import synth
    pkg, k = tdr
    import ctypes as C
    cfg = synth.Config("cm", 100, ncls, 16, 8, max(rows, cols), 4, seed=300 + ncls)
    sc = synth.make_scene(cfg, with_particles=False)
    maps = np.ascontiguousarray(sc.class_maps[:, :rows, :cols])
    mask = np.ascontiguousarray(sc.class_mask[:rows, :cols])
    m = k.make_map(maps, mask, 1.0)
    assert m.desc.cwords == k.lib.tdr_cmap_words(ncls) and m.desc.cwords in (1, 2, 4)
    assert 1 < m.desc.dict_n <= 1024
    dic = m.dict.cpu().numpy()
    assert dic[0] == 0.0 and set(np.unique(maps)) <= set(dic[: m.desc.dict_n])
    back = k.zeros((m.rec.numel(),))
    assert k.lib.tdr_k_unpack_compact_map(C.byref(m.desc), C.c_void_p(back.data_ptr()), k.stream()) == 0
    assert __import__("torch").equal(back, m.rec)


def test_map_without_compact_form_falls_back_to_dense(tdr, oracle):
    """More than 4096 distinct distance values (here: random floats) or more than 11 classes: no compact records, every
    wave reads the dense ones; scoring is unaffected."""
    from top_down_renderer_amd import synth
    pkg, k = tdr
    cfg = synth.Config("nocm", 3000, 4, 32, 24, 160, 300, seed=71)
    sc = synth.make_scene(cfg)
    maps = sc.class_maps * np.random.default_rng(5).uniform(0.5, 1.0, sc.class_maps.shape).astype(np.float32)
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), maps, sc.class_mask, kernels=k)
    assert m.dev.desc.cwords == 0 and m.dev.crec is None
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    scan = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
    ref = oracle.compute_weights(oracle.OracleMap(maps, sc.class_mask, 1.0), oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res),
                                 cfg.nb, cfg.nr, scan, cfg.res, oracle.make_params(cfg.ncls), sc.states.copy())
    f = pkg.ParticleFilter(len(sc.states), m, pkg.FilterParams(fixed_scale=1.0), kernels=k, init_particles=False)
    f.set_states(sc.states)
    f.update(scan, None, cfg.res)
    _assert_weights(f.raw_weights(), ref)
    assert k.lib.tdr_cmap_words(12) == 0 and k.lib.tdr_cmap_words(11) == 4 and k.lib.tdr_cmap_words(6) == 2


@pytest.mark.parametrize("ncls", [4, 6, 7])
def test_wide_compact_records_for_maps_with_many_distinct_values(tdr, oracle, ncls):
    """More than 1024 distinct distance values (a fine map resolution: min(50, resolution * sqrt(d2)) takes more values)
    but at most 4096, 4-7 classes: the WIDE compact form (16-bit fields, csrc/tdr_cmap.hip) instead of the dense
    fallback.  It decodes to the dense records bit for bit, and the scoring kernel that reads it gives the bits of the
    dense-record kernel — and the oracle's weights to 1e-5."""
    import ctypes as C
    import torch
    from top_down_renderer_amd import synth
    pkg, k = tdr
    cfg = synth.Config("wide", 4000, ncls, 48, 24, 220, 1200, seed=1700 + ncls)
    sc = synth.make_scene(cfg)
    # the scene's class geometry (zero inside a class) with ~3000 distinct distance values outside it
    rng = np.random.default_rng(ncls)
    maps = (rng.integers(1, 3000, sc.class_maps.shape) / 64.0).astype(np.float32)
    maps[sc.class_maps == 0] = 0.0
    assert 1024 < len(np.unique(maps)) <= 4096
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), maps, sc.class_mask, kernels=k)
    d = m.dev.desc
    assert d.cwords == 4 and d.rec_floats == 8 and 1024 < d.dict_n <= 4096
    assert m.dev.crec.numel() == k.lib.tdr_cmap_wide_words_total(ncls, d.rows, d.cols)
    back = k.zeros((m.dev.rec.numel(),))
    assert k.lib.tdr_k_unpack_compact_map(C.byref(d), C.c_void_p(back.data_ptr()), k.stream()) == 0
    assert torch.equal(back, m.dev.rec)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    st = sc.states.copy()
    far = rng.random(len(st)) < 0.1
    st["init_x_px"][far] = rng.uniform(-300, 500, int(far.sum())).astype(np.float32)   # partly outside the map
    scan = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
    ref = oracle.compute_weights(oracle.OracleMap(maps, sc.class_mask, 1.0), oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res),
                                 cfg.nb, cfg.nr, scan, cfg.res, oracle.make_params(cfg.ncls), st.copy())
    before = k.lib.tdr_config_compact(-1)
    out = []
    try:
        for on in (0, 1):
            k.lib.tdr_config_compact(on)
            f = pkg.ParticleFilter(len(st), m, pkg.FilterParams(fixed_scale=1.0), kernels=k, init_particles=False,
                                   locality_every=on)
            f.set_states(st)
            f.update(scan, None, cfg.res)
            out.append(f.raw_weights())
    finally:
        k.lib.tdr_config_compact(before)
    _assert_weights(out[0], ref)
    assert np.array_equal(out[0], out[1], equal_nan=True)
    # the Cartesian score reads the wide form too
    mc = pkg.TopDownMap(pkg.Params(resolution=1.0), maps, sc.class_mask, kernels=k)
    assert mc.dev.desc.cwords == 4
    mc.setWindow(20, 28)
    scan_c = oracle.raster_cart(sc.pts, cfg.res, sc.lut, cfg.ncls, 20, 28)
    fc = pkg.ParticleFilter(len(st), mc, pkg.FilterParams(fixed_scale=1.0), kernels=k, init_particles=False)
    fc.set_states(st)
    fc.update(scan_c, None, cfg.res)
    ref_c = oracle.compute_weights_cart(oracle.OracleMap(maps, sc.class_mask, 1.0), 20, 28, scan_c, cfg.res,
                                        oracle.make_params(cfg.ncls), st.copy())
    _assert_weights(fc.raw_weights(), ref_c)


@pytest.mark.parametrize("ncls,nb,scale_fixed", [(3, 36, True), (6, 64, True), (6, 50, False), (7, 33, True), (9, 40, False)])
def test_compact_and_dense_records_score_identically(tdr, oracle, ncls, nb, scale_fixed):
    """A particle's raw weight does not depend on which record form the launch read: the dense-record kernel
    (tdr_config_compact(0)) and the compact-record kernel give the same bits — and the oracle's weights to 1e-5."""
    from top_down_renderer_amd import synth
    pkg, k = tdr
    cfg = synth.Config("cmix", 4000, ncls, nb, 24, 260, 1500, seed=900 + ncls + nb)
    sc = synth.make_scene(cfg)
    st = sc.states.copy()
    rng = np.random.default_rng(ncls)
    if not scale_fixed:
        st["scale"] = rng.uniform(0.6, 1.7, len(st)).astype(np.float32)
    far = rng.random(len(st)) < 0.1
    st["init_x_px"][far] = rng.uniform(-300, 600, int(far.sum())).astype(np.float32)   # partly outside the map
    params = dict(fixed_scale=1.0 if scale_fixed else -1.0)
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    assert m.dev.desc.cwords > 0
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    scan = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
    ref = oracle.compute_weights(oracle.OracleMap(sc.class_maps, sc.class_mask, 1.0),
                                 oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res), cfg.nb, cfg.nr, scan, cfg.res,
                                 oracle.make_params(cfg.ncls, **params), st.copy())
    before, before_form = k.lib.tdr_config_compact(-1), k.lib.tdr_config_shift_uniform(-1)
    out = []
    try:
        k.lib.tdr_config_shift_uniform(0)   # the float kernel on either record form (the integer form: tests/test_ray.py)
        for on in (0, 1):
            k.lib.tdr_config_compact(on)
            f = pkg.ParticleFilter(len(st), m, pkg.FilterParams(**params), kernels=k, init_particles=False,
                                   locality_every=on)
            f.set_states(st)
            f.update(scan, None, cfg.res)
            out.append(f.raw_weights())
    finally:
        k.lib.tdr_config_compact(before)
        k.lib.tdr_config_shift_uniform(before_form)
    _assert_weights(out[0], ref)
    for o in out[1:]:
        assert np.array_equal(out[0], o, equal_nan=True)


# ---- A10 propagate ------------------------------------------------------------------------------------------------------
def test_propagate_golden(tdr, g):
    pkg, k = tdr
    ncls, nb, nr, _ = [int(v) for v in g["shape"]]
    m = _micro_map(pkg, k, g, nb, nr, float(g["ang_res"]))
    states = np.ascontiguousarray(g["states_in"]).view(pkg.STATE_DTYPE).reshape(-1)
    for freeze in (0, 1):
        f = pkg.ParticleFilter(32, m, pkg.FilterParams(fixed_scale=1.0 if freeze else -1.0), seed=7, kernels=k,
                               init_particles=False)
        f.set_states(states)
        assert f.isScaleFrozen() == bool(freeze)
        z = k.propagate_normals(k.rng_create(7), 32, bool(freeze))
        assert np.array_equal(z, g[f"prop_normals_freeze{freeze}"])   # same std::mt19937 stream, bit for bit
        f.propagate((1.0, 0.25), 0.01)
        got = f.get_states()
        ref = np.ascontiguousarray(g[f"prop_states_freeze{freeze}"]).view(pkg.STATE_DTYPE).reshape(-1)
        for name in ("init_x_px", "init_y_px", "dx_m", "dy_m", "theta", "scale"):
            assert np.array_equal(got[name], ref[name]), name            # bit for bit: same normals, same sinf / cosf
        assert np.array_equal(f.last_dist[:32].cpu().numpy(), g[f"prop_last_dist_freeze{freeze}"])


def test_propagate_device_rng_statistics(tdr, g):
    pkg, k = tdr
    import torch
    n = 200_000
    st = k.zeros((7, n))
    st[5] = 1.0
    last = k.zeros((n,))
    k.propagate(st, n, last, 1.0, 0.0, 0.0, False, 0.3, 0.05, z4=None, seed=5, step=1)
    dx, dy, th, sc = (st[i].double().cpu().numpy() for i in (2, 3, 4, 5))
    assert abs(dx.mean() - 1.0) < 5e-3 and abs(dx.std() - 0.3) < 5e-3
    assert abs(dy.mean()) < 5e-3 and abs(dy.std() - 0.3) < 5e-3
    assert abs(th.std() - 0.05) < 1e-3 and abs(sc.std() - 0.02) < 1e-3
    st2 = k.zeros((7, n))
    st2[5] = 1.0
    k.propagate(st2, n, last, 1.0, 0.0, 0.0, False, 0.3, 0.05, z4=None, seed=5, step=1)
    assert torch.equal(st, st2)   # counter-based: same (seed, step, index) -> same draw


# ---- A12 statistics, A14 resample -------------------------------------------------------------------------------------------
def test_update_weights_vs_oracle(tdr, oracle, g):
    pkg, k = tdr
    rng = np.random.default_rng(3)
    cases = [(g["weights_default"], g["prop_last_dist_freeze1"]),
             (np.full(8, np.nan, np.float32), np.full(8, 0.1, np.float32))]
    raw = (rng.random(50_000).astype(np.float32) * 6 + 0.5)
    raw[rng.random(50_000) < 0.02] = np.nan
    raw[rng.random(50_000) < 0.01] = 0.0
    cases.append((raw, rng.random(50_000).astype(np.float32) * 0.4))
    for raw, ld in cases:
        n = len(raw)
        w = k.zeros((n,))
        info = k.zeros((65536,))
        k.update_weights(k.to_device(raw), k.to_device(ld), n, w, info)
        ref, best, stats = oracle.update_weights(raw, ld)
        got = w.cpu().numpy()
        assert np.allclose(got, ref, rtol=2e-6, atol=0)
        assert int(info[:1].cpu().view(__import__("torch").int32).item()) == best
        assert abs(float(got.astype(np.float64).sum()) - 1.0) < 1e-5


def test_resample_bit_exact(tdr, oracle, g):
    pkg, k = tdr
    import torch
    rng = np.random.default_rng(4)
    big = rng.random(100_000).astype(np.float32) ** 4
    big = (big / big.sum()).astype(np.float32)
    cases = [(g["upd_weights"], 32, 0.37), (g["upd_weights"], 20, 0.37), (g["upd_weights"], 50, 0.37),
             (g["resample_neg_w"], 9, 0.5), (big, 100_000, 0.7731), (big, 75_010, 0.001)]
    for w, n_new, shift in cases:
        n = len(w)
        runmax = k.zeros((n,))
        idx = k.zeros((n_new,), torch.int32)
        k.prefix(k.to_device(w), n, runmax)
        k.resample(runmax, n, n_new, shift, 0, n_new, idx)
        ref = oracle.resample_prefix(w, n_new, shift)
        assert np.array_equal(idx.cpu().numpy(), ref)
    assert np.array_equal(oracle.resample_literal(g["upd_weights"], 32, 0.37), g["resample_idx_32"])


def _prefix_cases():
    rng = np.random.default_rng(0)
    f32 = np.float32
    cases = {}
    for n in (1, 7, 1000, 100_000):
        w = rng.random(n).astype(f32) ** 3
        cases[f"random^3 n={n}"] = (w / w.sum()).astype(f32)
    cases["uniform 1/N"] = np.full(100_000, f32(1e-5))
    cases["power of two"] = np.full(65_536, f32(2.0 ** -16))
    cases["ties forced"] = np.tile(np.asarray([1.0, 2.0 ** -24, 2.0 ** -24, 3 * 2.0 ** -25], f32), 5000)
    cases["half-ulp spam"] = np.concatenate([[f32(1.0)], np.full(20_000, f32(2.0 ** -24))])
    cases["zeros then data"] = np.concatenate([np.zeros(9000, f32), rng.random(5000).astype(f32) * f32(1e-4),
                                               np.zeros(100, f32)])
    cases["negatives"] = ((rng.random(20_000).astype(f32) - f32(0.2)) * f32(1e-4)).astype(f32)
    # sizes of the one-launch kernel (n <= 32 768): ragged chunk ends, ties, crossings at chunk ends, irregular weights
    for n in (513, 4096, 20_000, 32_767, 32_768):
        w = rng.random(n).astype(f32) ** 2
        cases[f"normalised n={n}"] = (w / w.sum()).astype(f32)
    cases["20k dyadic ties"] = (rng.integers(0, 64, 20_000) * f32(2.0 ** -22)).astype(f32)
    w = (rng.random(30_000) * 1e-6).astype(f32); w[511::512] = f32(0.01); cases["30k a jump at every chunk end"] = w
    w = (rng.random(25_000).astype(f32) / f32(12_500)); w[[700, 9000, 9001, 24_999]] = f32(-0.125); w[13_000] = f32(3.0)
    cases["25k negatives and a jump"] = w
    w = np.full(20_000, f32(5e-5)); w[rng.random(20_000) < 0.1] = f32(-3e-6); cases["20k nan-fill negative"] = w
    w = rng.random(20_000).astype(f32); w[12_345] = f32(np.inf); w[15_000] = f32(-np.inf); cases["20k inf then -inf"] = w
    w = rng.random(20_000).astype(f32); w[12_345] = f32(np.nan); cases["20k nan inside"] = w
    cases["20k zeros"] = np.zeros(20_000, f32)
    w = np.zeros(20_000, f32); w[15_000:] = f32(1e-3); cases["20k zeros then data"] = w
    cases["nan-fill negative"] = np.where(rng.random(60_000) < 0.1, f32(-3e-6), rng.random(60_000).astype(f32) * 4e-5).astype(f32)
    cases["wide dynamic range"] = (10.0 ** rng.uniform(-12, -2, 50_000)).astype(f32)
    cases["subnormals"] = (rng.random(3000) * 1e-41).astype(f32)
    cases["big then small"] = np.concatenate([[f32(1e30)], rng.random(3000).astype(f32)])
    cases["nan inside"] = np.concatenate([rng.random(9000).astype(f32), [f32(np.nan)], rng.random(300).astype(f32)])
    cases["inf inside"] = np.concatenate([rng.random(9000).astype(f32), [f32(np.inf)], rng.random(300).astype(f32)])
    w = rng.random(1_000_000).astype(f32) ** 4
    cases["1M random^4"] = (w / w.sum()).astype(f32)
    # large inputs for the multi-workgroup scan: ties in bulk, stagnation, irregular weights deep inside, ragged tail
    cases["300k dyadic ties"] = (rng.integers(0, 64, 300_001) * f32(2.0 ** -22)).astype(f32)
    cases["half-ulp ties"] = np.concatenate([[f32(4096.0)], np.full(200_000, f32(2.0 ** -12), f32),  # exactly half an ulp
                                             np.full(50_000, f32(2.0 ** -13), f32), rng.random(70_000).astype(f32)])
    # the float chain stalls below 2 while the exact sum passes it: every later chunk is mispredicted
    cases["stagnation"] = np.concatenate([[f32(1.9999)], np.full(400_000, f32(2.0 ** -25), f32),
                                          rng.random(30_000).astype(f32) * f32(1e-3)])
    w = (rng.random(500_003).astype(f32) / f32(250_000))
    w[[70_000, 250_001]] = f32(-0.125)
    w[400_000] = f32(3.0)
    cases["500k negatives and a jump"] = w
    w = (rng.random(262_144 + 5).astype(f32) / f32(131_072))
    w[200_000] = f32(np.nan)
    cases["262k nan inside"] = w
    cases["2M uniform"] = np.full(2_000_000, f32(1.0 / 2_000_000), f32)
    w = np.exp(rng.normal(0, 2.0, 800_000)).astype(f32)
    cases["800k lognormal normalised"] = (w / w.sum(dtype=np.float64)).astype(f32)
    return cases


def test_exact_parallel_prefix_is_the_serial_float_chain(tdr):
    """tdr_k_prefix_mode: the one-workgroup parallel kernel (integer increments per binade), the multi-workgroup scan
    (per-chunk parity summaries) and the one-wave serial kernel must all reproduce `running_sum += weights_[j]` (particle_filter.cpp:179) bit for bit, including rounding ties, zero runs,
    negative weights, NaN/inf and binade crossings."""
    pkg, k = tdr
    import ctypes as C
    for name, w in _prefix_cases().items():
        n = len(w)
        with np.errstate(over="ignore", invalid="ignore"):
            ref = np.cumsum(w, dtype=np.float32)                      # sequential float32 accumulation
            refmax = np.maximum.accumulate(np.where(np.isnan(ref), -np.inf, ref)).astype(np.float32)
        wd = k.to_device(w)
        ws = k.prefix_workspace(n)
        for mode in (0, 1, 2, 3):
            if mode == 3 and n > 32768:
                continue
            rm, pf = k.zeros((n,)), k.zeros((n,))
            assert k.lib.tdr_k_prefix_mode(C.c_void_p(wd.data_ptr()), n, mode, C.c_void_p(rm.data_ptr()),
                                           C.c_void_p(pf.data_ptr()) if mode else None,
                                           C.c_void_p(ws.data_ptr()) if n else None, k.stream()) == 0
            assert np.array_equal(rm.cpu().numpy(), refmax), (name, mode)
            if mode:
                assert np.array_equal(pf.cpu().numpy(), ref, equal_nan=True), name
        rm = k.zeros((n,))
        k.prefix(wd, n, rm)                                           # the dispatching entry point
        assert np.array_equal(rm.cpu().numpy(), refmax), name


def test_update_weights_large_n_multi_workgroup(tdr, oracle):
    pkg, k = tdr
    rng = np.random.default_rng(8)
    n = 300_000
    raw = (rng.random(n).astype(np.float32) * 6 + 0.5)
    raw[rng.random(n) < 0.03] = np.nan
    raw[rng.random(n) < 0.01] = 0.0
    ld = rng.random(n).astype(np.float32) * 0.4
    w, info = k.zeros((n,)), k.zeros((65536,))
    k.update_weights(k.to_device(raw), k.to_device(ld), n, w, info)
    ref, best, stats = oracle.update_weights(raw, ld)
    got = w.cpu().numpy()
    # The reference's two serial float chains (`sum`, `bottom_stddev`, particle_filter.cpp:108-126) are reproduced
    # exactly at this size, so the value written into NaN particles is the reference's; what remains are the two
    # normalisation sums, whose order Eigen leaves unspecified.
    valid = ~np.isnan(raw)
    assert np.allclose(got, ref, rtol=3e-6, atol=0)
    assert int(info[:1].cpu().view(__import__("torch").int32).item()) == best
    assert np.array_equal(info[1:4].cpu().numpy(), np.asarray(stats[:3], np.float32))   # sum, mean, bottom_stddev: bit for bit
    # determinism: same inputs, same bits
    w2, info2 = k.zeros((n,)), k.zeros((65536,))
    k.update_weights(k.to_device(raw), k.to_device(ld), n, w2, info2)
    assert np.array_equal(got, w2.cpu().numpy())
    # all-NaN at large n: all-ones fallback
    w3 = k.zeros((n,))
    k.update_weights(k.to_device(np.full(n, np.nan, np.float32)), k.to_device(ld), n, w3, info2)
    assert np.allclose(w3.cpu().numpy(), 1.0 / n, rtol=1e-5)


@pytest.mark.parametrize("kind", ["lognormal", "equal", "dyadic", "tiny", "mostly nan", "one valid"])
@pytest.mark.parametrize("n", [1, 63, 1000, 20_000, 32_768, 40_000, 1_000_003])
def test_update_weights_serial_chains_bit_exact(tdr, oracle, kind, n):
    """`sum`, `mean` and `bottom_stddev` of particle_filter.cpp:108-126 are serial float32 accumulations (the second one
    of double addends); the GPU reproduces them bit for bit at every size — one workgroup up to 32 768 particles
    (uw_small_kernel; 20 000 is the reference's operating point, top_down_render.cpp:53), tdr_chain_total above —
    whatever the weights look like: rounding ties in bulk, huge dynamic range, sums that start tiny, almost no valid
    weight."""
    pkg, k = tdr
    rng = np.random.default_rng(hash(kind) % 1000 + n % 97)
    f32 = np.float32
    if kind == "lognormal":
        raw = np.exp(rng.normal(0, 3, n)).astype(f32)
    elif kind == "equal":
        raw = np.full(n, f32(6.6666665), f32)
        raw[rng.random(n) < 0.3] = f32(3.25)
    elif kind == "dyadic":
        raw = (rng.integers(1, 4096, n) * 2.0 ** -9).astype(f32)
    elif kind == "tiny":
        raw = (rng.random(n) * 1e-30).astype(f32)
    elif kind == "mostly nan":
        raw = rng.random(n).astype(f32) + f32(0.5)
        raw[rng.random(n) < 0.97] = np.nan
    else:
        raw = np.full(n, np.nan, f32)
        raw[n // 3] = f32(2.5)
    if kind not in ("mostly nan", "one valid"):
        raw[rng.random(n) < 0.02] = np.nan
    ld = rng.random(n).astype(f32)
    w, info = k.zeros((n,)), k.zeros((65536,))
    k.update_weights(k.to_device(raw), k.to_device(ld), n, w, info)
    ref, best, stats = oracle.update_weights(raw, ld)
    got_stats = info[1:4].cpu().numpy()
    assert np.array_equal(got_stats, np.asarray(stats[:3], f32), equal_nan=True), (got_stats, stats[:3])
    assert np.allclose(w.cpu().numpy(), ref, rtol=3e-6, atol=0, equal_nan=True)


@pytest.mark.parametrize("n", [1, 7, 511, 512, 513, 4096, 4097, 20_000, 32_767, 32_768])
def test_uw_small_wave_chains_equal_workgroup_chains(tdr, oracle, n):
    """The two evaluations of the statistics chains for n <= 32 768 — wave by wave (default) and chunk by chunk on the
    whole workgroup (tdr_config_uw_waves(0)) — write the same bytes, and both are the oracle's serial chains, on weights
    chosen against the wave path: zero runs at the start and across whole wave-chunks, negative and infinite weights (real
    additions in the middle of predicted chunks), a binade crossing at every chunk end, half-ulp ties in bulk."""
    pkg, k = tdr
    f32 = np.float32
    rng = np.random.default_rng(4200 + n)
    cases = []
    a = np.zeros(n, f32); a[n // 2:] = rng.random(n - n // 2).astype(f32); cases.append(a)            # zeros, then weights
    a = rng.random(n).astype(f32); a[512:1536] = 0; cases.append(a)                                   # a hole of two chunks
    a = rng.random(n).astype(f32) + f32(0.25); a[rng.random(n) < 0.01] *= f32(-1.0); cases.append(a)  # negatives
    a = np.full(n, f32(1.0), f32); a[::2] = f32(1.0 + 2.0 ** -23); cases.append(a)                    # ties against a growing sum
    a = (rng.random(n) * 1e-3).astype(f32); a[511::512] = f32(40.0); cases.append(a)                  # a jump at every chunk end
    a = rng.random(n).astype(f32); a[n // 3] = np.inf; cases.append(a)                                # inf in the middle
    a = np.exp(rng.normal(0, 8, n)).astype(f32); a[rng.random(n) < 0.3] = np.nan; cases.append(a)
    before = k.lib.tdr_config_uw_waves(-1)
    try:
        for ci, raw in enumerate(cases):
            ld = rng.random(n).astype(f32)
            out = []
            for on in (1, 0):
                k.lib.tdr_config_uw_waves(on)
                w, info = k.zeros((n,)), k.zeros((65536,))
                k.update_weights(k.to_device(raw), k.to_device(ld), n, w, info)
                out.append((w.cpu().numpy(), info[:8].cpu().numpy().tobytes(), info[1:4].cpu().numpy()))
            # the chains and the counts bit for bit; the two normalisation sums are double sums in another order (the
            # reference leaves their order to Eigen), so the weights agree to rounding
            assert out[0][1] == out[1][1], f"case {ci}"
            assert np.allclose(out[0][0], out[1][0], rtol=1e-6, atol=0, equal_nan=True), f"case {ci}"
            with np.errstate(all="ignore"):
                _, _, stats = oracle.update_weights(raw, ld)
            assert np.array_equal(out[0][2], np.asarray(stats[:3], f32), equal_nan=True), (ci, out[0][2], stats[:3])
    finally:
        k.lib.tdr_config_uw_waves(before)


@pytest.mark.parametrize("n", [32_768, 32_769, 40_000, 100_000, 300_017])
def test_heads_of_the_long_chains_through_the_one_workgroup_kernels(tdr, oracle, n):
    """Above 32 768 weights the first 32 768 addends of the statistics chains and of the running sum go through the
    one-workgroup kernels (chain_head_kernel, pfx_small_kernel) and the chunk walk starts behind them;
    tdr_config_prefix_small(0) walks the chunks from the first addend on.  Same `sum`, `mean`, `bottom_stddev`, same
    running maxima, bit for bit, and both the oracle's / numpy's serial chains."""
    pkg, k = tdr
    import ctypes as C
    f32 = np.float32
    rng = np.random.default_rng(5100 + n)
    cases = [(1.0 / (rng.random(n) * 20 + 0.15)).astype(f32), np.exp(rng.normal(0, 4, n)).astype(f32),
             (rng.integers(0, 64, n) * 2.0 ** -9).astype(f32)]
    cases[0][rng.random(n) < 0.05] = np.nan
    a = np.zeros(n, f32); a[30_000:] = rng.random(n - 30_000).astype(f32); cases.append(a)   # the head sums to zero
    before = k.lib.tdr_config_prefix_small(-1)
    try:
        for ci, raw in enumerate(cases):
            ld = rng.random(n).astype(f32)
            got = []
            for on in (1, 0):
                k.lib.tdr_config_prefix_small(on)
                w, info = k.zeros((n,)), k.zeros((65536,))
                k.update_weights(k.to_device(raw), k.to_device(ld), n, w, info)
                rm = k.zeros((n,))
                k.prefix(w, n, rm)
                got.append((info[:8].cpu().numpy().tobytes(), w.cpu().numpy(), rm.cpu().numpy()))
            assert got[0][0] == got[1][0], f"case {ci}: statistics"
            assert np.array_equal(got[0][1], got[1][1], equal_nan=True) and np.array_equal(got[0][2], got[1][2]), f"case {ci}"
            with np.errstate(all="ignore"):
                _, _, stats = oracle.update_weights(raw, ld)
                ref = np.cumsum(got[0][1], dtype=f32)
            assert np.array_equal(np.frombuffer(got[0][0], f32)[1:4], np.asarray(stats[:3], f32), equal_nan=True), ci
            assert np.array_equal(got[0][2], np.maximum.accumulate(np.where(np.isnan(ref), -np.inf, ref)).astype(f32)), ci
    finally:
        k.lib.tdr_config_prefix_small(before)


def test_gather_states_and_aos_roundtrip(tdr, g):
    pkg, k = tdr
    import torch
    states = np.ascontiguousarray(g["states_in"]).view(pkg.STATE_DTYPE).reshape(-1)
    st = k.zeros((7, 40))
    k.states_to_device(states, st, 32)
    back = k.states_to_host(st, 32, pkg.STATE_DTYPE)
    assert back.tobytes() == states.tobytes()
    idx = np.asarray([3, 3, 0, 31, 7], np.int32)
    dst = k.zeros((7, 8))
    k.gather_states(st, k.to_device(idx), 5, dst)
    assert k.states_to_host(dst, 5, pkg.STATE_DTYPE).tobytes() == states[idx].tobytes()


# ---- whole step through the mirrored class surface ----------------------------------------------------------------------------
def test_full_step_c1_vs_oracle(tdr, oracle):
    """propagate -> render -> update (score, statistics, resample) exactly like takeStep (src/top_down_render.cpp:505-572),
    GPU classes vs the oracle driven by the same std::mt19937 seed."""
    pkg, k = tdr
    sc, cfg, om, _, tab = _c1_scene(oracle)
    seed = 11
    # oracle
    fpo = oracle.make_params(cfg.ncls)
    st_o = sc.states.copy()
    rng_o = oracle.Rng(seed)
    last_o = oracle.propagate(st_o, 1.0, 0.0, 0.01, True, fpo, rng_o)
    scan_o = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
    raw_o = oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan_o, cfg.res, fpo, st_o)
    w_o, best_o, _ = oracle.update_weights(raw_o, last_o)
    shift_o = rng_o.uniform()
    idx_o = oracle.resample_prefix(w_o, len(st_o), shift_o)
    new_o = oracle.gather_states(st_o, idx_o)
    # GPU, through the reference's class surface
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    f = pkg.ParticleFilter(len(sc.states), m, pkg.FilterParams(fixed_scale=1.0), seed=seed, kernels=k,
                           init_particles=False)
    f.set_states(sc.states)
    r = pkg.ScanRendererPolar(sc.lut, kernels=k)
    r.set_output_shape(cfg.ncls, cfg.nb, cfg.nr)
    f.propagate((1.0, 0.0), 0.01)
    r.renderSemanticTopDown(sc.pts, cfg.res, cfg.ang_res)
    f.update(r.last_scan(), None, cfg.res)
    assert f.last_shift_ == shift_o
    pre = k.states_to_host(f.st_new, len(st_o), pkg.STATE_DTYPE)      # the propagated, pre-resample set
    for name in ("init_x_px", "init_y_px", "dx_m", "dy_m", "theta", "scale", "have_init"):
        assert np.array_equal(pre[name], st_o[name]), name            # propagate: bit for bit
    assert np.array_equal(f.last_dist[: len(st_o)].cpu().numpy(), last_o)
    _assert_weights(f.raw_weights(), raw_o)
    w = f.weights()
    assert np.allclose(w, w_o, rtol=WEIGHT_RTOL, atol=0)
    assert f._argmax() == best_o
    idx = f.resample_indices()
    mism = int((idx != idx_o).sum())
    assert mism <= 2 + len(idx) // 200, f"{mism} resample indices differ"
    got = f.get_states()
    same = idx == idx_o
    for name in ("init_x_px", "init_y_px", "dx_m", "dy_m", "theta", "scale"):
        assert np.array_equal(got[name][same], new_o[name][same]), name
    # resampling identical weights is bit-exact
    import torch
    runmax = k.zeros((len(w_o),))
    idx2 = k.zeros((len(w_o),), torch.int32)
    k.prefix(k.to_device(w_o), len(w_o), runmax)
    k.resample(runmax, len(w_o), len(w_o), shift_o, 0, len(w_o), idx2)
    assert np.array_equal(idx2.cpu().numpy(), idx_o)
    # pose statistics of the SAME particle set (the GPU's resampled one): only the summation order differs (the
    # reference adds serially in float, the kernels in double)
    mean_o, cov_o = oracle.mean_cov(got)
    assert np.allclose(f.meanLikelihood(), mean_o, rtol=2e-5, atol=2e-5)
    assert np.allclose(f.computeMeanCov(), cov_o, rtol=1e-4, atol=1e-4)
    ml = f.maxLikelihood()
    s = st_o[best_o]
    assert np.allclose(ml, [s["dx_m"] * s["scale"] + s["init_x_px"], s["dy_m"] * s["scale"] + s["init_y_px"],
                            s["theta"], s["scale"]], rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("waves", [1, 0])
def test_full_step_at_the_reference_defaults_vs_oracle(tdr, oracle, waves):
    """The reference node's own operating point (src/top_down_render.cpp:53: 20 000 particles, a 100 x 25 polar image, 6
    classes): one step — propagate, render, update — against the oracle over ALL particles: raw weights to 1e-5, the NaN
    pattern, the statistics chains bit for bit given the same raw weights, the normalised weights, the arg-max, and the
    resample indices bit for bit given the same weights.  waves = 1: the one-workgroup statistics evaluate their chains
    wave by wave and the running sum is the one-launch kernel (the defaults); 0: the round-2 evaluations."""
    from top_down_renderer_amd import synth
    pkg, k = tdr
    import torch
    sc = synth.make_scene("ref")
    cfg = sc.cfg
    n = len(sc.states)
    m = pkg.TopDownMapPolar(pkg.Params(resolution=cfg.map_resolution), sc.class_maps, sc.class_mask, kernels=k)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    r = pkg.ScanRendererPolar(sc.lut, kernels=k)
    r.set_output_shape(cfg.ncls, cfg.nb, cfg.nr)
    r.renderSemanticTopDown(sc.pts, cfg.res, cfg.ang_res)
    b_uw, b_px = k.lib.tdr_config_uw_waves(-1), k.lib.tdr_config_prefix_small(-1)
    try:
        k.lib.tdr_config_uw_waves(waves)
        k.lib.tdr_config_prefix_small(waves)
        f = pkg.ParticleFilter(n, m, pkg.FilterParams(fixed_scale=1.0), seed=9, kernels=k, init_particles=False,
                               locality_every=1)   # parity RNG: the reference's mt19937 stream
        f.set_states(sc.states)
        f.propagate((1.0, 0.0), 0.01)
        f.update(r.last_scan(), None, cfg.res, shift=0.61)
        raw, w, idx, amax = f.raw_weights(), f.weights(), f.resample_indices(), f._argmax()
        # the oracle's step on the same inputs
        fpo = oracle.make_params(cfg.ncls)
        st = sc.states.copy()
        last = oracle.propagate(st, 1.0, 0.0, 0.01, True, fpo, oracle.Rng(9))
        scan = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
        ref_raw = oracle.compute_weights(oracle.OracleMap(sc.class_maps, sc.class_mask, cfg.map_resolution),
                                         oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res, cfg.map_resolution), cfg.nb, cfg.nr,
                                         scan, cfg.res, fpo, st)
        _assert_weights(raw, ref_raw)
        ref_w, ref_argmax, ref_stats = oracle.update_weights(ref_raw, last)
        assert np.allclose(w, ref_w, rtol=2e-5, atol=0)
        assert amax == ref_argmax or abs(w[ref_argmax] - w.max()) <= 2e-5 * w.max()
        # the device's statistics on the ORACLE's raw weights: the serial chains bit for bit
        wd, info = k.zeros((n,)), k.zeros((65536,))
        k.update_weights(k.to_device(ref_raw), k.to_device(last), n, wd, info)
        assert np.array_equal(info[1:4].cpu().numpy(), np.asarray(ref_stats[:3], np.float32), equal_nan=True)
        # resampling the ORACLE's weights on the device: the oracle's indices bit for bit
        ref_idx = oracle.resample_prefix(ref_w, n, 0.61)
        runmax = k.empty((n,))
        k.prefix(k.to_device(ref_w), n, runmax)
        out = k.zeros((n,), torch.int32)
        k.resample(runmax, n, n, 0.61, 0, n, out)
        assert np.array_equal(out.cpu().numpy(), ref_idx)
        mism = int((idx != ref_idx).sum())
        assert mism <= 2 + n // 200, f"{mism} resample indices differ"
    finally:
        k.lib.tdr_config_uw_waves(b_uw)
        k.lib.tdr_config_prefix_small(b_px)


def test_full_step_with_an_empty_scan_vs_oracle(tdr, oracle):
    """A scan without a single usable return: every class image is zero, every cost is 0/0, every weight NaN — the
    statistics take the reference's `sum == 0 || num_under_mean < 1` branch (src/particle_filter.cpp:129-131: all weights
    1, then normalised) and the resampling draws from equal weights.  Same result as the oracle, indices included."""
    pkg, k = tdr
    sc, cfg, om, _, tab = _c1_scene(oracle)
    pts = sc.pts.copy()
    pts[:, 0:2] = 0.0          # every point is the sensor origin: skipped by the renderer (scan_renderer_polar.cpp:96)
    seed = 5
    fpo = oracle.make_params(cfg.ncls)
    st_o = sc.states.copy()
    rng_o = oracle.Rng(seed)
    last_o = oracle.propagate(st_o, 0.5, 0.1, 0.02, True, fpo, rng_o)
    scan_o = oracle.raster_polar(pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
    assert not scan_o.any()
    raw_o = oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan_o, cfg.res, fpo, st_o)
    assert np.isnan(raw_o).all()
    w_o, best_o, _ = oracle.update_weights(raw_o, last_o)
    idx_o = oracle.resample_prefix(w_o, len(st_o), rng_o.uniform())
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    f = pkg.ParticleFilter(len(sc.states), m, pkg.FilterParams(fixed_scale=1.0), seed=seed, kernels=k,
                           init_particles=False)
    f.set_states(sc.states)
    r = pkg.ScanRendererPolar(sc.lut, kernels=k)
    r.set_output_shape(cfg.ncls, cfg.nb, cfg.nr)
    f.propagate((0.5, 0.1), 0.02)
    r.renderSemanticTopDown(pts, cfg.res, cfg.ang_res)
    assert not r.last_images().cpu().numpy().any()
    f.update(r.last_scan(), None, cfg.res)
    assert np.isnan(f.raw_weights()).all()
    assert np.array_equal(f.weights(), w_o)
    assert f._argmax() == best_o
    assert np.array_equal(f.resample_indices(), idx_o)


def test_init_search_c1(tdr, oracle):
    pkg, k = tdr
    sc, cfg, om, scan, tab = _c1_scene(oracle)
    st = sc.states[:192].copy()
    st["have_init"] = 0
    st["theta"] = 0
    st_o = st.copy()
    ref = oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan, cfg.res, oracle.make_params(cfg.ncls), st_o)
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    f = pkg.ParticleFilter(len(st), m, pkg.FilterParams(fixed_scale=1.0), kernels=k, init_particles=False)
    f.set_states(st)
    f.update(scan, None, cfg.res)
    _assert_weights(f.raw_weights(), ref)
    pre = k.states_to_host(f.st_new, len(st), pkg.STATE_DTYPE)
    # Rotations may tie to within the rounding of the candidates' float sums: wherever another candidate was chosen, it
    # is a tie of the oracle's minimum (<= 2e-5 on the weight) — no floor on how many agree, every mismatch is checked.
    differ = pre["theta"] != st_o["theta"]
    if differ.any():
        st2 = st_o.copy()
        st2["theta"], st2["have_init"] = pre["theta"], 1
        ref2 = oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan, cfg.res, oracle.make_params(cfg.ncls), st2)
        tie = np.abs(ref2[differ] - ref[differ]) / np.maximum(np.abs(ref[differ]), 1e-30)
        assert np.nanmax(tie, initial=0.0) <= 2e-5, f"chosen rotation is not a near-tie: {np.nanmax(tie):.2e}"
    assert pre["have_init"].all()
    # ... and on the COST, exactly summed: the first candidate of its shift class, within 2e-5 of the minimum
    import init_exact_ref as X
    exact = X.Search(oracle, sc.class_maps, sc.class_mask, 1.0, tab, cfg.nb, cfg.nr, scan, cfg.res,
                     oracle.make_params(cfg.ncls), st)
    X.check_choice(exact, st["theta"], pre["theta"], pre["have_init"], f.raw_weights(), ref, st["have_init"])


@pytest.mark.parametrize("ncls", [8, 11, 12, 15])
def test_init_search_on_the_matrix_cores_for_wide_records(tdr, oracle, ncls):
    """8-15 classes (records of 12 / 16 floats): the 40-rotation search through score_init_mfma_wide_kernel against the
    vector-unit search and the oracle — the same rotation, or a tie of the two costs within 2e-5; weights within 1e-5 at
    the chosen rotation."""
    from top_down_renderer_amd import synth
    pkg, k = tdr
    cfg = synth.Config("initwide", 9000, ncls, 48, 20, 400, 600, seed=300 + ncls)
    sc = synth.make_scene(cfg)
    st = sc.states.copy()
    st["have_init"] = 0
    st["theta"] = 0
    st["init_x_px"][:4] = np.asarray([-300, 3, 399, 200], np.float32)     # all unknown / at the border
    cw = [float(0.5 + (c % 4) * 0.5) for c in range(ncls)]
    om = oracle.OracleMap(sc.class_maps, sc.class_mask, 1.0)
    tab = oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res, 1.0)
    scan = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, ncls, cfg.nb, cfg.nr)
    fpo = oracle.make_params(ncls, class_weights=cw)
    st_o = st.copy()
    ref = oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan, cfg.res, fpo, st_o)
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    before = k.lib.tdr_config_init_mfma(-1)
    got = {}
    try:
        for on in (0, 1):
            k.lib.tdr_config_init_mfma(on)
            f = pkg.ParticleFilter(len(st), m, pkg.FilterParams(fixed_scale=1.0, class_weights=cw), kernels=k,
                                   init_particles=False)
            f.set_states(st)
            k.score(m.dev, m.scan_handle(scan), cfg.res, f.fp_c, f.st, len(st), f.raw_w, init_search=True,
                    uniform_scale=f._uniform_scale)
            got[on] = (f.raw_w[: len(st)].cpu().numpy(), k.states_to_host(f.st, len(st), pkg.STATE_DTYPE))
    finally:
        k.lib.tdr_config_init_mfma(before)
    for on in (0, 1):
        raw, sts = got[on]
        assert sts["have_init"].all()
        same = sts["theta"] == st_o["theta"]
        _assert_weights(raw[same], ref[same])
        if not same.all():
            st2 = st_o.copy()
            st2["theta"], st2["have_init"] = sts["theta"], 1
            ref2 = oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan, cfg.res, fpo, st2)
            _assert_weights(raw[~same], ref2[~same])
            tie = np.abs(ref2[~same] - ref[~same]) / np.maximum(np.abs(ref[~same]), 1e-30)
            assert np.nanmax(tie, initial=0.0) <= 2e-5, f"mfma={on}: chosen rotation is not a near-tie: {np.nanmax(tie):.2e}"
    assert (got[0][1]["theta"] != got[1][1]["theta"]).mean() < 0.02
    # ... and on the COST, exactly summed (the first 160 particles, the four at the edges among them): the first candidate
    # of its shift class, within 2e-5 of the minimum
    import init_exact_ref as X
    nx = 160
    exact = X.Search(oracle, sc.class_maps, sc.class_mask, 1.0, tab, cfg.nb, cfg.nr, scan, cfg.res, fpo, st[:nx])
    for on in (0, 1):
        raw, sts = got[on]
        X.check_choice(exact, st["theta"][:nx], sts["theta"][:nx], sts["have_init"][:nx], raw[:nx], ref[:nx],
                       st["have_init"][:nx])


def test_freeze_scale_and_shift_init(tdr, oracle, g):
    pkg, k = tdr
    ncls, nb, nr, _ = [int(v) for v in g["shape"]]
    m = _micro_map(pkg, k, g, nb, nr, float(g["ang_res"]))
    f = pkg.ParticleFilter(32, m, pkg.FilterParams(fixed_scale=-1.0), kernels=k, init_particles=False)
    states = np.ascontiguousarray(g["states_in"]).view(pkg.STATE_DTYPE).reshape(-1).copy()
    states["scale"] = g["freeze_scale_in"]
    f.set_states(states)
    assert f.scale() == -1.0
    f.freezeScale()
    assert f.isScaleFrozen()
    assert f.scale() == pytest.approx(float(g["freeze_scale_geo_mean"]), rel=2e-6)
    k.shift_init(f.st, 32, 3.0, -2.0)
    got = f.get_states()
    assert np.array_equal(got["init_x_px"], states["init_x_px"] + np.float32(3.0))
    assert np.array_equal(got["init_y_px"], states["init_y_px"] - np.float32(2.0))


def test_initialize_particles_matches_oracle_stream(tdr, oracle):
    """ParticleFilter's constructor path (particle_filter.cpp:19-84): same mt19937 seed -> the same particles."""
    pkg, k = tdr
    from top_down_renderer_amd import synth
    sc = synth.make_scene("c1", with_particles=False)
    om = oracle.OracleMap(sc.class_maps, sc.class_mask, 1.0)
    kw = dict(fixed_scale=1.0, init_pos_px_x=sc.pose[0], init_pos_px_y=sc.pose[1], init_pos_px_cov=10.0,
              init_pos_deg_theta=30.0, init_pos_deg_cov=5.0)
    ref = oracle.initialize_particles(om, oracle.make_params(sc.cfg.ncls, **kw), 300, oracle.Rng(21))
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    f = pkg.ParticleFilter(300, m, pkg.FilterParams(**kw), seed=21, kernels=k)
    assert f.numParticles() == 300
    assert f.get_states().tobytes() == ref.tobytes()
    assert m.getClassesAtPoint((int(ref["init_x_px"][0]), int(ref["init_y_px"][0]))).count(1) == 1


# ---- full BASELINE sizes: configs 2, 3 (one GPU's shard), 4 and 5 (one GPU's shard) ---------------------------------------
# Size-independent properties (weights sum to 1, systematic-resampling counts within floor/ceil of N w, sorted indices,
# processing-order invariance) plus an oracle spot check on particles strided over the whole set.
def _resample_properties(w, idx, n, n_new=None):
    n_new = n if n_new is None else n_new
    assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-5
    assert np.all(np.diff(idx) >= 0) and idx.min() >= 0 and idx.max() < n
    counts = np.bincount(idx, minlength=n)
    exp = n_new * w.astype(np.float64)
    assert counts.sum() == n_new
    assert np.all(counts >= np.floor(exp) - 1)
    # Upper bound for every particle but the last: the reference's scan stops at j == N-1 (particle_filter.cpp:178), so
    # every threshold above the final value of the float32 running sum — which falls short of 1 by the accumulated
    # rounding of N additions — lands on the last particle.
    assert np.all(counts[:-1] <= np.ceil(exp[:-1]) + 1)
    short = 1.0 - float(np.cumsum(w, dtype=np.float32)[-1])
    assert counts[-1] <= np.ceil(exp[-1]) + 1 + max(0.0, short) * n_new + 1


@pytest.fixture(scope="module")
def big_polar(tdr, oracle):
    """Config 2's scene (100k-pt scan, 6 classes, 256x256 polar, 4000^2 map) on the device, shared by the c2 / c3 / c5
    tests below (configs 3 and 5 name the same scan / map shape with other particle sets)."""
    from top_down_renderer_amd import synth
    pkg, k = tdr
    sc = synth.make_scene("c2")
    cfg = sc.cfg
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    r = pkg.ScanRendererPolar(sc.lut, kernels=k)
    r.set_output_shape(cfg.ncls, cfg.nb, cfg.nr)
    r.renderSemanticTopDown(sc.pts, cfg.res, cfg.ang_res)
    scan = r.last_images().cpu().numpy()
    assert np.array_equal(scan, oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr))
    om = oracle.OracleMap(sc.class_maps, sc.class_mask, 1.0)
    tab = oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res, 1.0)
    return sc, cfg, m, r, scan, om, tab


def _full_size_polar(tdr, oracle, big_polar, states, n_sel=64):
    pkg, k = tdr
    sc, cfg, m, r, scan, om, tab = big_polar
    n = len(states)
    res = []
    for loc in (0, 1):
        f = pkg.ParticleFilter(n, m, pkg.FilterParams(fixed_scale=1.0), seed=5, kernels=k, init_particles=False,
                               locality_every=loc)
        f.set_states(states)
        f.propagate((1.0, 0.0), 0.01)
        f.update(r.last_scan(), None, cfg.res)
        res.append((f.raw_weights(), f.weights(), f.resample_indices()))
    raw, w, idx = res[0]
    assert np.array_equal(raw, res[1][0], equal_nan=True) and np.array_equal(idx, res[1][2])  # order invariance
    _resample_properties(w, idx, n)
    # oracle spot check: particles spread over the set, scored from the un-propagated states
    f = pkg.ParticleFilter(n, m, pkg.FilterParams(fixed_scale=1.0), seed=5, kernels=k, init_particles=False,
                           locality_every=1)
    f.set_states(states)
    f.update(scan, None, cfg.res)
    sel = np.arange(0, n, n // n_sel)[:n_sel]
    # ... plus the special cases wherever the set has them: particles whose window leaves the map (centre within a window
    # radius of the border) and particles scored NaN (more than half of the window unknown, state_particle.cpp:117-120)
    raw_all = f.raw_weights()
    cx = states["dx_m"] * states["scale"] + states["init_x_px"]
    cy = states["dy_m"] * states["scale"] + states["init_y_px"]
    edge = np.nonzero((cx < cfg.nr) | (cy < cfg.nr) | (cx > m.cols - cfg.nr) | (cy > m.rows - cfg.nr))[0][:256]
    nan = np.nonzero(np.isnan(raw_all))[0][:256]
    sel = np.unique(np.concatenate([sel, edge, nan]))
    st_sel = np.ascontiguousarray(states[sel])
    ref = oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan, cfg.res, oracle.make_params(cfg.ncls), st_sel)
    return f, sel, st_sel, ref


def test_c2_full_size_properties(tdr, oracle, big_polar):
    """BASELINE configs[1]: 100k particles (90 % Gaussian about the true pose + 10 % uniform)."""
    sc = big_polar[0]
    f, sel, _, ref = _full_size_polar(tdr, oracle, big_polar, sc.states, n_sel=4096)
    assert len(sel) >= 4096      # (all 100 000 against the oracle: tests/test_shift_uniform.py, the c2 full step)
    _assert_weights(f.raw_weights()[sel], ref)


def test_c3_shard_full_size_properties(tdr, oracle, big_polar):
    """BASELINE configs[2] (1M particles over 8 GPUs): one GPU's shard of 125 000 particles of the 1M-particle set."""
    from top_down_renderer_amd import synth
    sc = big_polar[0]
    cfg3 = synth.CONFIGS["c3"]
    rng = np.random.default_rng(cfg3.seed)
    st = synth.make_particles(cfg3, sc.lab, sc.pose, rng, n=cfg3.n_particles)[: cfg3.n_particles // 8].copy()
    assert len(st) == 125_000
    f, sel, _, ref = _full_size_polar(tdr, oracle, big_polar, st, n_sel=4096)
    assert len(sel) >= 4096
    _assert_weights(f.raw_weights()[sel], ref)


def test_c5_shard_full_size_init_search(tdr, oracle, big_polar):
    """BASELINE configs[4] (8 init clusters x 250k particles, no heading, over 8 GPUs): one GPU's share of 250 000
    particles drawn from all 8 clusters, have_init = false — the first update runs the 40-rotation search of
    src/state_particle.cpp:195-206 on the matrix cores at the full shape; the chosen rotation is checked through the
    oracle (candidates can tie to within the rounding of the float sums)."""
    from top_down_renderer_amd import synth
    pkg, k = tdr
    sc, cfg, m, r, scan, om, tab = big_polar
    cfg5 = synth.CONFIGS["c5"]
    st = synth.make_cluster_particles(cfg5, sc.lab, np.random.default_rng(cfg5.seed), n_clusters=8, per_cluster=31_250)
    n = len(st)
    assert n == 250_000 and not st["have_init"].any()
    f = pkg.ParticleFilter(n, m, pkg.FilterParams(fixed_scale=1.0), seed=9, kernels=k, init_particles=False,
                           locality_every=1)
    f.set_states(st)
    f.update(r.last_scan(), None, cfg.res)
    raw, w, idx = f.raw_weights(), f.weights(), f.resample_indices()
    _resample_properties(w, idx, n)
    pre = k.states_to_host(f.st_new, n, pkg.STATE_DTYPE)          # the scored (pre-resample) set
    assert pre["have_init"].all()
    cand = []                                                      # the reference's candidate list (:197)
    t = np.float32(0)
    while t < 2 * np.pi:
        cand.append(t)
        t = np.float32(np.float64(t) + 2 * np.pi / 40)
    assert np.isin(pre["theta"], np.asarray(cand, np.float32)).all()
    sel = np.arange(0, n, n // 2048)[:2048]
    st_o = np.ascontiguousarray(st[sel])
    fpo = oracle.make_params(cfg.ncls)
    ref = oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan, cfg.res, fpo, st_o)     # runs the search too
    same = pre["theta"][sel] == st_o["theta"]
    _assert_weights(raw[sel][same], ref[same])   # (no floor on how many agree: every mismatch must be a tie, below)
    if not same.all():
        st2 = st_o.copy()
        st2["theta"] = pre["theta"][sel]
        st2["have_init"] = 1
        ref2 = oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan, cfg.res, fpo, st2)
        _assert_weights(raw[sel][~same], ref2[~same])
        tie = np.abs(ref2[~same] - ref[~same]) / np.abs(ref[~same])
        assert np.nanmax(tie, initial=0.0) <= 2e-5, "chosen rotation is not a near-tie of the oracle's minimum"
    # a second update starts from initialised particles: the steady-state path on the same shard
    f.update(r.last_scan(), None, cfg.res)
    _resample_properties(f.weights(), f.resample_indices(), n)
    # the search above gathered pre-split half records (tdr_map_desc.rec16); splitting the f32 records on the fly
    # (score_init_mfma_kernel, what small launches and maps without the scratch use) sums the same f16 products in
    # another order: the same rotations up to near-ties
    assert m.dev.rec16 is not None
    m.dev.use_rec16 = False
    try:
        f.set_states(st)
        k.score(m.dev, m.scan_handle(r.last_scan()), cfg.res, f.fp_c, f.st, n, f.raw_w, init_search=True,
                uniform_scale=f._uniform_scale)
    finally:
        m.dev.use_rec16 = True
    again = k.states_to_host(f.st, n, pkg.STATE_DTYPE)
    differ = again["theta"] != pre["theta"]
    assert differ.mean() < 1e-3
    raw2 = f.raw_w[:n].cpu().numpy()
    assert np.array_equal(raw2[~differ], raw[~differ], equal_nan=True)
    if differ.any():
        assert np.nanmax(np.abs(raw2[differ] - raw[differ]) / np.abs(raw[differ])) <= 2e-5


def test_c4_full_size_cartesian(tdr, oracle):
    """BASELINE configs[3]: Cartesian render (scan_renderer.cpp:55-78) + Cartesian window (top_down_map.cpp:429-459),
    6 classes, 512x512 render, 8000x8000 map, 200k particles."""
    from top_down_renderer_amd import synth
    pkg, k = tdr
    sc = synth.make_scene("c4")
    cfg = sc.cfg
    rows, cols = cfg.nb, cfg.nr
    n = len(sc.states)
    assert n == 200_000 and sc.class_maps.shape == (6, 8000, 8000)
    m = pkg.TopDownMap(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.setWindow(rows, cols)
    r = pkg.ScanRenderer(sc.lut, kernels=k)
    r.set_output_shape(cfg.ncls, rows, cols)
    r.renderSemanticTopDown(sc.pts, cfg.res)
    scan = oracle.raster_cart(sc.pts, cfg.res, sc.lut, cfg.ncls, rows, cols)
    assert np.array_equal(r.last_images().cpu().numpy(), scan)
    res = []
    for loc in (0, 1):
        f = pkg.ParticleFilter(n, m, pkg.FilterParams(fixed_scale=1.0), seed=5, kernels=k, init_particles=False,
                               locality_every=loc)
        f.set_states(sc.states)
        f.update(r.last_scan(), None, cfg.res)
        res.append((f.raw_weights(), f.weights(), f.resample_indices()))
    raw, w, idx = res[1]
    assert np.array_equal(raw, res[0][0], equal_nan=True) and np.array_equal(idx, res[0][2])  # order invariance
    _resample_properties(w, idx, n)
    sel = np.arange(0, n, n // 1024)[:1024]
    stt = sc.states
    cx, cy = stt["dx_m"] * stt["scale"] + stt["init_x_px"], stt["dy_m"] * stt["scale"] + stt["init_y_px"]
    half = 0.75 * max(rows, cols) * cfg.res                 # a rotated window reaches half a diagonal from its centre
    edge = np.nonzero((cx < half) | (cy < half) | (cx > 8000 - half) | (cy > 8000 - half))[0][:128]
    sel = np.unique(np.concatenate([sel, edge, np.nonzero(np.isnan(raw))[0][:128]]))   # + windows off the map, NaN scores
    om = oracle.OracleMap(sc.class_maps, sc.class_mask, 1.0)
    ref = oracle.compute_weights_cart(om, rows, cols, scan, cfg.res, oracle.make_params(cfg.ncls),
                                      np.ascontiguousarray(sc.states[sel]))
    _assert_weights(raw[sel], ref)
