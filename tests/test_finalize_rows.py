"""score_finalize_exact_kernel adds a slot's chunk rows two at a time (csrc/tdr_score.hip): with 1, 2, 3, 5 and 8 rows per
slot — one share with a single row, shares with none, a share with two rows beside shares with one — the weights are one
set of bits (integer sums: any grouping) and the oracle's to 1e-5.  The case that tests/test_ray.py's order-independence
test does not have: row counts that are not a power of two.  (With four shares a slot, a share takes a second step of the
loop only from 9 rows on; the ray kernel writes at most 8, so that is not reached here — it is the dense share of
config-2-sized launches, 28 rows.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_TOTAL = 1_000_000
ALL_RAY = 1e-6   # span: every particle through the ray-mapped kernel, tdr_config_ray_split rows per slot


@pytest.fixture(scope="module")
def tdr():
    import torch
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd.kernels import HipKernels

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pkg, HipKernels()


def test_rows_per_slot_1_2_3_5_8(tdr, oracle):
    import torch
    from top_down_renderer_amd import synth
    pkg, k = tdr
    sc = synth.make_scene(synth.Config("finrows", 6000, 6, 64, 32, 300, 3000, seed=5177))
    cfg = sc.cfg
    st = sc.states.copy()
    n = len(st)
    rng = np.random.default_rng(6)
    st["init_x_px"][::9] = rng.uniform(-100, 400, len(st[::9])).astype(np.float32)   # borders, outside: NaN weights too
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    scan = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
    ref = oracle.compute_weights(oracle.OracleMap(sc.class_maps, sc.class_mask, 1.0),
                                 oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res), cfg.nb, cfg.nr, scan, cfg.res,
                                 oracle.make_params(cfg.ncls, fixed_scale=1.0), st.copy())
    f = pkg.ParticleFilter(n, m, pkg.FilterParams(fixed_scale=1.0), kernels=k, init_particles=False, locality_every=1)
    f.set_states(st)
    loc = k.zeros((f.cap_local,), torch.int32)
    k.locality_order(f.st, n, m.rows, m.cols, loc)
    pk = m.scan_handle(scan)
    before = k.lib.tdr_config_shift_uniform(-1)
    got = {}
    try:
        k.lib.tdr_config_shift_uniform(2)
        k.lib.tdr_config_shift_uniform_span(ALL_RAY)
        for split in (1, 2, 3, 5, 8):
            k.lib.tdr_config_ray_split(split)
            f.raw_w.fill_(-7.0)
            k.score(m.dev, pk, float(cfg.res), f.fp_c, f.st, n, f.raw_w, perm=loc, uniform_scale=f._uniform_scale,
                    n_total=N_TOTAL, ctx=None)
            k.synchronize()
            got[split] = f.raw_w[:n].cpu().numpy()
    finally:
        k.lib.tdr_config_shift_uniform(before)
        k.lib.tdr_config_shift_uniform_span(-2.0)
        k.lib.tdr_config_ray_split(0)
    assert not (got[1] == -7.0).any()
    for split in (2, 3, 5, 8):
        assert np.array_equal(got[1], got[split], equal_nan=True), f"{split} rows per slot"
    assert np.array_equal(np.isnan(got[1]), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = np.abs(got[1][ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1e-30)
    assert err.max(initial=0.0) <= 1e-5, err.max()
