"""The scoring call with the geometric term (tdr_k_score_polar_geo) writes its uniform-scale table itself, every call: it
runs float kernels only, so nothing else in the call would.  A filter with a fixed scale scores the same particles twice, on a
shape that would take the integer form in the plain call, with the shared workspace overwritten with NaN in between: the
second call's weights are the first's bits, and agree to rounding with the call made with the integer form switched off.
Run with `pytest -m gpu`."""
import numpy as np
import pytest

from test_geo import _geo_scene, _lidar, tdr  # noqa: F401

pytestmark = pytest.mark.gpu


def test_geometric_call_fills_its_scaled_table_every_call(tdr, oracle):
    import torch
    pkg, k = tdr
    cfg, sc = _geo_scene(3)
    rng = np.random.default_rng(3)
    pts, w, h = _lidar(rng, 256, 16, bumps=0.3)
    geo = oracle.raster_geo_polar(pts, w, h, cfg.res, cfg.ang_res, cfg.nb, cfg.nr)
    scan = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    assert m.dev.desc.cwords > 0
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    f = pkg.ParticleFilter(len(sc.states), m, pkg.FilterParams(fixed_scale=1.0), kernels=k, init_particles=False,
                           use_geometric_cost=True)
    f.set_states(sc.states)
    assert f._uniform_scale == 1.0
    n = len(sc.states)
    scan_pk = m.scan_handle(scan)
    geo_pk = k.pack_scan(k.to_device(np.ascontiguousarray(geo[:2], np.float32)), 2, cfg.nb, cfg.nr)
    sums = (float(np.float32(geo[0].astype(np.float64).sum())), float(np.float32(geo[1].astype(np.float64).sum())))

    def score():
        f.raw_w.fill_(-7.0)
        k.score_geo(m.dev, m.geo_dev(), scan_pk, geo_pk, sums, float(cfg.res), f.fp_c, f.st, n, f.raw_w,
                    init_search=False, uniform_scale=f._uniform_scale)
        k.synchronize()
        raw = f.raw_w[:n].cpu().numpy()
        assert not (raw == -7.0).any()
        return raw

    before = k.lib.tdr_config_shift_uniform(-1)
    try:
        k.lib.tdr_config_shift_uniform(0)
        plain = score()
        k.lib.tdr_config_shift_uniform(2)       # the shape now has an integer form in the plain call
        k._ws = torch.full_like(k._ws, float("nan"))
        first = score()
        k._ws = torch.full_like(k._ws, float("nan"))
        second = score()
    finally:
        k.lib.tdr_config_shift_uniform(before)
    assert np.array_equal(second, first, equal_nan=True)
    # (the ring groups of a shape with an integer form are whole fours: another partition of the float sums than `plain`'s,
    # the same weights to rounding — 3e-6, the bound the float form is held to elsewhere in the suite)
    assert np.array_equal(np.isnan(first), np.isnan(plain))
    ok = ~np.isnan(plain)
    assert ok.any()
    assert float(np.max(np.abs(first[ok] - plain[ok]) / np.abs(plain[ok]))) <= 3e-6
