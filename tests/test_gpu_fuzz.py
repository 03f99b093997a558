"""Randomised parity sweep on the GPU: seeded random shapes (class count, odd θ/range bin counts, non-square maps, map
and scan resolutions, per-particle scales, particles far outside the map, un-initialised particles, both gates) through
raster -> score -> statistics -> running sum -> resample, each stage against the CPU oracle on the same inputs.
Integer / index stages must agree exactly; weights within 1e-5 relative (BASELINE.json north_star)."""
import os

import numpy as np
import pytest

# TDR_FUZZ_SEEDS=N widens the sweep for a one-off soak run (default: 48 polar cases)
N_SEEDS = int(os.environ.get("TDR_FUZZ_SEEDS", "48"))

pytestmark = pytest.mark.gpu


def _assert_weights(w, ref, rtol):
    assert np.array_equal(np.isnan(w), np.isnan(ref)), (int(np.isnan(w).sum()), int(np.isnan(ref).sum()))
    ok = ~np.isnan(ref)
    err = np.abs(w[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1e-30)
    assert err.max(initial=0.0) <= rtol, f"max rel err {err.max():.3e}"


@pytest.fixture(scope="module")
def env():
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd.kernels import HipKernels
    return pkg, HipKernels()


def _case(seed, ncls=None):
    from top_down_renderer_amd import synth
    rng = np.random.default_rng(9000 + seed)
    ncls = int(rng.integers(1, 9)) if ncls is None else ncls
    if ncls == 1:
        ncls = 2            # the generator keeps class 1 for roads
    nb = int(rng.choice([8, 12, 25, 36, 64, 100, 129]))
    nr = int(rng.choice([4, 7, 16, 25, 40]))
    size = int(rng.choice([96, 160, 257]))
    cfg = synth.Config(f"fuzz{seed}", int(rng.integers(200, 6000)), ncls, nb, nr, size, int(rng.integers(1, 600)),
                       seed=500 + seed, res=float(rng.choice([0.5, 1.0, 1.7, 3.0])),
                       map_resolution=float(rng.choice([0.5, 1.0, 2.0])))
    sc = synth.make_scene(cfg)
    # non-square map: crop the generated square
    rows = int(rng.integers(size // 2, size + 1))
    cols = int(rng.integers(size // 2, size + 1))
    maps = np.ascontiguousarray(sc.class_maps[:, :rows, :cols])
    mask = np.ascontiguousarray(sc.class_mask[:rows, :cols])
    st = sc.states.copy()
    n = len(st)
    fixed = bool(rng.integers(0, 2))
    if not fixed:
        st["scale"] = rng.uniform(0.3, 12.0, n).astype(np.float32)      # both sides of the [0.5, 10] scale gate
    st["dx_m"] = rng.normal(0, 3, n).astype(np.float32)
    st["dy_m"] = rng.normal(0, 3, n).astype(np.float32)
    st["theta"] = rng.uniform(-7, 7, n).astype(np.float32)
    far = rng.random(n) < 0.15                                            # far outside the map, either side
    st["init_x_px"][far] = rng.uniform(-3 * size, 4 * size, int(far.sum())).astype(np.float32)
    st["init_y_px"][far] = rng.uniform(-3 * size, 4 * size, int(far.sum())).astype(np.float32)
    params = dict(fixed_scale=1.0 if fixed else -1.0, class_weights=[float(x) for x in rng.uniform(0.2, 2.5, ncls)],
                  regularization=float(rng.choice([0.15, 0.7, 2.0])), force_on_map=bool(rng.integers(0, 2)))
    if fixed:
        st["scale"] = 1.0
    return cfg, sc, maps, mask, st, params, rng


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_shapes_against_oracle(env, oracle, seed):
    import torch
    pkg, k = env
    cfg, sc, maps, mask, st, params, rng = _case(seed)
    ncls, nb, nr = cfg.ncls, cfg.nb, cfg.nr
    # ---- raster: exact
    r = pkg.ScanRendererPolar(sc.lut, kernels=k)
    r.set_output_shape(ncls, nb, nr)
    r.renderSemanticTopDown(sc.pts, cfg.res, cfg.ang_res)
    scan_o = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, ncls, nb, nr)
    assert np.array_equal(r.last_images().cpu().numpy(), scan_o)
    # ---- score
    om = oracle.OracleMap(maps, mask, cfg.map_resolution)
    tab = oracle.polar_table(nb, nr, cfg.ang_res, cfg.map_resolution)
    fpo = oracle.make_params(ncls, **params)
    raw_o = oracle.compute_weights(om, tab, nb, nr, scan_o, cfg.res, fpo, st.copy())
    m = pkg.TopDownMapPolar(pkg.Params(resolution=cfg.map_resolution), maps, mask, kernels=k)
    m.samplePtsPolar((nb, nr), cfg.ang_res)
    f = pkg.ParticleFilter(len(st), m, pkg.FilterParams(**params), seed=seed, kernels=k, init_particles=False,
                           locality_every=int(rng.integers(0, 2)))
    f.set_states(st)
    shift = float(rng.random())
    f.update(r.last_scan(), None, cfg.res, shift=shift)
    _assert_weights(f.raw_weights(), raw_o, 1e-5)
    # ---- statistics on identical raw weights (the GPU's), then the running sum + resample on identical weights: exact
    raw_g = f.raw_weights()
    ld = np.zeros(len(st), np.float32)
    w_o, best_o, _ = oracle.update_weights(raw_g, ld)
    w_g = f.weights()
    assert np.allclose(w_g, w_o, rtol=3e-6, atol=0) or np.isnan(raw_g).all()
    if not np.isnan(raw_g).all():
        assert f._argmax() == best_o
    idx_o = oracle.resample_prefix(w_g, len(st), shift)
    assert np.array_equal(f.resample_indices(), idx_o)
    got = f.get_states()
    ref = oracle.gather_states(st, idx_o)
    for name in ("init_x_px", "init_y_px", "dx_m", "dy_m", "theta", "scale"):
        assert np.array_equal(got[name], ref[name]), name


@pytest.mark.parametrize("seed,ncls,pile", [(s, None, 0) for s in range(8)] +
                         [(20 + s, 4 + s % 4, 0) for s in range(max(12, N_SEEDS // 4))] +
                         [(40, 6, 3000), (41, 5, 2049)] +
                         [(50, 8, 0), (51, 11, 0), (52, 12, 0), (53, 15, 0)] +   # 12- and 16-float records: vector kernel
                         [(60, 3, 0), (61, 2, 0), (62, 1, 0)])                    # 4-float records
def test_random_init_search_against_oracle(env, oracle, seed, ncls, pile):
    """have_init = false: the 40-rotation search on random shapes; the chosen rotation is verified through the oracle's
    cost at the GPU's theta (candidates can tie to within rounding).  4-7 classes take the matrix-core kernel
    (score_init_mfma_kernel), and up to 7 classes the one on half records (score_init_half_kernel, second pass below);
    `pile` points in one bin push a scan count past what f16 holds exactly, which must send the search back to the
    vector kernel."""
    pkg, k = env
    cfg, sc, maps, mask, st, params, rng = _case(100 + seed, ncls)
    if pile:
        lab = sc.lut[sc.pts[:, 3].astype(np.int64)]
        r = np.hypot(sc.pts[:, 0], sc.pts[:, 1])
        k0 = int(np.nonzero((lab >= 0) & (r > cfg.res) & (r < (cfg.nr - 1) * cfg.res))[0][0])   # a point that lands in the image
        sc.pts = np.concatenate([sc.pts, np.repeat(sc.pts[k0:k0 + 1], pile, axis=0)])
    ncls, nb, nr = cfg.ncls, cfg.nb, cfg.nr
    params["fixed_scale"] = 1.0
    st["scale"] = 1.0
    st["have_init"] = 0
    scan_o = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, ncls, nb, nr)
    if pile:
        assert scan_o.max() >= pile or scan_o.sum(0).max() >= pile
    om = oracle.OracleMap(maps, mask, cfg.map_resolution)
    tab = oracle.polar_table(nb, nr, cfg.ang_res, cfg.map_resolution)
    fpo = oracle.make_params(ncls, **params)
    st_o = st.copy()
    raw_o = oracle.compute_weights(om, tab, nb, nr, scan_o, cfg.res, fpo, st_o)
    m = pkg.TopDownMapPolar(pkg.Params(resolution=cfg.map_resolution), maps, mask, kernels=k)
    m.samplePtsPolar((nb, nr), cfg.ang_res)
    f = pkg.ParticleFilter(len(st), m, pkg.FilterParams(**params), seed=seed, kernels=k, init_particles=False)
    f.set_states(st)
    # the same choice held to the exactly summed COST (the first 160 particles): the first candidate of its shift class,
    # within 2e-5 of the minimum; gated particles untouched; theta 0 where no candidate can win
    import init_exact_ref as X
    nx = min(len(st), 160)
    exact = X.Search(oracle, maps, mask, cfg.map_resolution, tab, nb, nr, scan_o, cfg.res, fpo, st[:nx])

    def search_and_check():
        # score only: read the states back before the resample shuffles them
        f.set_states(st)
        k.score(m.dev, m.scan_handle(scan_o), cfg.res, f.fp_c, f.st, len(st), f.raw_w, init_search=True)
        raw_g = f.raw_w[: len(st)].cpu().numpy()
        got = k.states_to_host(f.st, len(st), st.dtype)
        assert np.array_equal(got["have_init"], st_o["have_init"])
        same = got["theta"] == st_o["theta"]   # (no floor on how many agree: every mismatch must be a tie, below)
        _assert_weights(raw_g[same], raw_o[same], 1e-5)
        # Where another candidate was chosen: the weight is the oracle's AT THAT rotation (1e-5), and that rotation ties
        # with the oracle's minimum to within the rounding of the candidates' float sums (the reference's own Eigen sums
        # have unspecified order) — a margin on the search's choice, not on any weight.
        diff = np.nonzero(~same)[0]
        if len(diff):
            st2 = st_o.copy()
            st2["theta"][diff] = got["theta"][diff]
            st2["have_init"] = 1
            raw2 = oracle.compute_weights(om, tab, nb, nr, scan_o, cfg.res, fpo, st2)
            _assert_weights(raw_g[diff], raw2[diff], 1e-5)
            tie = np.abs(raw2[diff] - raw_o[diff]) / np.maximum(np.abs(raw_o[diff]), 1e-30)
            assert np.nanmax(tie, initial=0.0) <= 2e-5, f"chosen rotation is not a near-tie: {np.nanmax(tie):.2e}"
        X.check_choice(exact, st["theta"][:nx], got["theta"][:nx], got["have_init"][:nx], raw_g[:nx], raw_o[:nx],
                       st["have_init"][:nx])

    search_and_check()
    # The same search on pre-split half records (score_init_half_kernel through tdr_map_desc.rec16; by default only
    # launches of thousands of particles take it): same f16 operands, summed four rings of one direction at a time.
    old_min = int(k.lib.tdr_config_rec16_min_particles(-1))
    try:
        k.lib.tdr_config_rec16_min_particles(0)
        search_and_check()
    finally:
        k.lib.tdr_config_rec16_min_particles(old_min)
    assert (m.dev.rec16 is not None) == (ncls <= 7)     # 1-3 classes (4-float records) take the same search


@pytest.mark.parametrize("seed", range(max(8, N_SEEDS // 6)))
def test_random_cartesian_against_oracle(env, oracle, seed):
    """BASELINE config 4's path (Cartesian raster + window, definition in include/tdr.h) on random shapes."""
    from top_down_renderer_amd import synth
    pkg, k = env
    rng = np.random.default_rng(7000 + seed)
    ncls = int(rng.integers(2, 9))
    rows, cols = int(rng.choice([9, 16, 33, 50])), int(rng.choice([8, 21, 32, 64]))
    size = int(rng.choice([128, 200]))
    cfg = synth.Config(f"cart{seed}", int(rng.integers(500, 5000)), ncls, rows, cols, size, int(rng.integers(1, 400)),
                       polar=False, seed=800 + seed, res=float(rng.choice([0.5, 0.75, 1.0, 2.0])))
    sc = synth.make_scene(cfg)
    st = sc.states.copy()
    n = len(st)
    st["scale"] = rng.uniform(0.7, 1.4, n).astype(np.float32)
    st["dx_m"] = rng.normal(0, 2, n).astype(np.float32)
    far = rng.random(n) < 0.1
    st["init_x_px"][far] = rng.uniform(-size, 2 * size, int(far.sum())).astype(np.float32)
    cw = [float(x) for x in rng.uniform(0.2, 2.5, ncls)]
    om = oracle.OracleMap(sc.class_maps, sc.class_mask, 1.0)
    scan = oracle.raster_cart(sc.pts, cfg.res, sc.lut, ncls, rows, cols)
    ref = oracle.compute_weights_cart(om, rows, cols, scan, cfg.res, oracle.make_params(ncls, class_weights=cw), st.copy())
    m = pkg.TopDownMap(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.setWindow(rows, cols)
    r = pkg.ScanRenderer(sc.lut, kernels=k)
    r.set_output_shape(ncls, rows, cols)
    r.renderSemanticTopDown(sc.pts, cfg.res)
    assert np.array_equal(r.last_images().cpu().numpy(), scan)
    f = pkg.ParticleFilter(n, m, pkg.FilterParams(fixed_scale=1.0, class_weights=cw), kernels=k, init_particles=False,
                           locality_every=int(rng.integers(0, 2)))
    f.set_states(st)
    f.update(r.last_scan(), None, cfg.res)
    _assert_weights(f.raw_weights(), ref, 1e-5)   # cos/sin of theta are the host libm's bit for bit


@pytest.mark.parametrize("seed", range(max(6, N_SEEDS // 5)))
def test_random_statistics_serial_chains_bit_exact(env, oracle, seed):
    """The weight statistics reproduce the reference's serial float chains (`sum`, `mean`, `bottom_stddev`,
    particle_filter.cpp:108-126) bit for bit: random raw-weight vectors of random length, on both sides of the
    32 768-particle switch between the one-workgroup and the multi-workgroup kernels."""
    pkg, k = env
    rng = np.random.default_rng(31000 + seed)
    f32 = np.float32
    n = int(rng.integers(1, 32769)) if seed % 2 else int(rng.integers(32769, 400_000))
    kind = int(rng.integers(0, 5))
    if kind == 0:
        raw = np.exp(rng.normal(0, rng.uniform(0.1, 5), n))
    elif kind == 1:
        raw = rng.integers(1, 1 << int(rng.integers(2, 14)), n) * 2.0 ** -int(rng.integers(0, 20))
    elif kind == 2:
        raw = 1.0 / (rng.random(n) * rng.uniform(0.1, 50) + 0.15)          # 1 / (cost + regularisation)
    elif kind == 3:
        raw = rng.choice(rng.random(int(rng.integers(1, 40))) * 7, n)      # few distinct values: ties in bulk
    else:
        raw = rng.random(n) * 10.0 ** rng.uniform(-35, 30)
    raw = raw.astype(f32)
    raw[rng.random(n) < rng.choice([0.0, 0.01, 0.3, 0.9])] = np.nan
    ld = rng.random(n).astype(f32)
    w, info = k.zeros((n,)), k.zeros((65536,))
    k.update_weights(k.to_device(raw), k.to_device(ld), n, w, info)
    with np.errstate(all="ignore"):
        ref, best, stats = oracle.update_weights(raw, ld)
    assert np.array_equal(info[1:4].cpu().numpy(), np.asarray(stats[:3], f32), equal_nan=True)
    assert np.allclose(w.cpu().numpy(), ref, rtol=3e-6, atol=0, equal_nan=True)
